"""tests/helpers/smoothness_checks.py is worth what it catches: faults planted into the yardstick's subject -- a statement's output with one thing wrong,
as a wrong kernel or a wrong statement would leave it -- must each fail the comparison, and the unspoilt output must pass it.  The condition on the
inputs (the decision margin) is shown to refuse an input that sits on the threshold."""
import numpy as np
import pytest

from .helpers import entropy_checks as ec
from .helpers import regularity_checks as rc
from .helpers import smoothness_checks as mc


@pytest.fixture(scope="module")
def subject(pkg):
    joints, trans, lengths, names, ex, table = ec.noisy_call(25)
    signals = rc.signals_of(joints, trans, table)
    return signals, lengths, ex, pkg.pipeline.gait_sparc(signals, lengths, ex, **mc.RULE)


def spoilt(out, **changes):
    made = {k: np.array(v, copy=True) for k, v in out.items()}
    for key, (index, value) in changes.items():
        made[key][index] = value(made[key][index]) if callable(value) else value
    return made


def test_the_unspoilt_statement_passes(subject):
    signals, lengths, ex, out = subject
    worst, margin = mc.compare(out, signals, lengths, ex, mc.RULE)
    print(f"worst ratio {worst:.3e}, margin {margin:.3e}")
    assert worst <= mc.BAR and margin >= mc.MARGIN


FAULTS = (("sparc off by a rounding too many", dict(per_segment=((6, 0, 1), lambda v: v * (1 + 64 * mc.BAR))), False),
          ("dj off in the twelfth place", dict(per_segment=((6, 0, 6), lambda v: v * (1 + 1e-12))), False),
          ("the band one bin short", dict(per_segment=((6, 0, 3), lambda v: v - 1)), True),
          ("the band one bin early", dict(per_segment=((6, 0, 2), lambda v: v + 1)), True),
          ("the peak at its neighbour", dict(per_segment=((6, 0, 4), lambda v: v + 1)), True),
          ("a segment one frame late", dict(per_segment=((6, 0, 0), lambda v: v + 1)), True),
          ("a slot behind the candidates written", dict(per_segment=((15, 0, 1), -4.0)), True),
          ("a NaN row where there is a value", dict(per_segment=((6, 0, slice(1, 8)), np.nan)), True),
          ("one candidate too many", dict(per_sequence=((6, 0, 1), lambda v: v + 1)), True),
          ("n one frame off", dict(per_sequence=((0, 1, 0), lambda v: v - 1)), True),
          ("the mean of the wrong segments", dict(per_sequence=((6, 0, 4), lambda v: v * (1 + 1e-9))), True),
          ("the SD by n - 1", dict(per_sequence=((6, 0, 5), lambda v: v * np.sqrt(9 / 8))), True),
          ("last_hz in bins", dict(per_sequence=((6, 0, 8), lambda v: v * 1024 / 20)), True),
          ("a row where used is 0", dict(per_sequence=((4, 0, 3), 1.0)), True),
          ("the logarithm of the wrong sign", dict(ldlj=((6, 0), lambda v: -v)), True),
          ("the slots of another hop", dict(slot_offsets=(7, 17)), True))


@pytest.mark.parametrize("name,changes,asserts", FAULTS, ids=[f[0] for f in FAULTS])
def test_a_planted_fault_is_caught(subject, name, changes, asserts):
    signals, lengths, ex, out = subject
    assert out["slot_offsets"].tolist() == [0, 3, 3, 3, 3, 4, 5, 16] and out["per_sequence"][6, 0, 1] == 9      # the 400-frame walker with its excluded frames
    bad = spoilt(out, **changes)
    if asserts:
        with pytest.raises(AssertionError):
            mc.compare(bad, signals, lengths, ex, mc.RULE)
    else:
        worst, _ = mc.compare(bad, signals, lengths, ex, mc.RULE)
        print(f"{name}: worst ratio {worst:.3e} against the bar {mc.BAR:.2e}")
        assert worst > mc.BAR


def test_an_input_on_the_threshold_is_refused(pkg):
    """A two-line spectrum whose second line is 0.05 of the first to within a rounding: which side of the threshold it falls on is the rounding's
    choice, so the condition refuses the input before anything is compared."""
    t = np.arange(200, dtype=np.float64)
    x = np.repeat((np.cos(2.0 * np.pi * 4 * t / 64) + 0.05 * np.cos(2.0 * np.pi * 20 * t / 64))[:, None], 4, axis=1)
    rule = mc.rule_of(0, 64, 32, 64)
    margin = mc.yardstick(x[:, 0], **rule)[4]
    print(f"margin {margin:.3e}")
    assert margin < mc.MARGIN
    with pytest.raises(AssertionError):
        mc.compare(pkg.pipeline.gait_sparc(x, **rule), x, [200], None, rule)
