"""A yardstick by numpy.fft, hand-made signals and the case files for the Welch spectrum of the gait signals, shared by the host and the
GPU tests.  Nothing here calls the code under test: what measures it takes the statement as an argument.

THE YARDSTICK.  Rules 1 to 4 with other tools than the code under test has: the segments are laid by a plain loop over the frames, the window is
numpy's cosine, the transform numpy.fft.rfft at nfft points, the average numpy's mean.  It rounds otherwise than a direct sum in a fixed order, so
statement and yardstick differ in the last places: THE BAR is on |statement - yardstick| per bin over the row's largest yardstick bin, 8 times the
worst such ratio measured over SHAPES on the CPU (measure_bound; the record: profiles/gait_spectrum_bounds.txt).  The margin is there because the
set is small and the direct sum's error grows with the segment length.  The device inherits the bar by bit-identity with the statement.

THE NOISY CALL is entropy_checks.noisy_call: seven sequences of 1, 19, 20, 64 (standing), 65 and 130 and 400 frames with 5 mm of seeded noise.
RULES names every value of derivative, segment, hop and nfft that the tests ask for, without their whole product.  THE RUNS: hand-made signals whose
runs of validity begin and end at frames 63, 64 and 65, and runs exactly L - 1, L and L + hop long."""
import numpy as np

from . import gait_checks as gc

FPS = 20.0
RULE = dict(fps=FPS, derivative=2, segment=64, hop=32, nfft=256, f_lo=0.5, f_hi=3.0, min_segments=2)
# (derivative, segment, hop, nfft): derivative 0, 1, 2; L 8, 64, 128, 256; hop L / 8, L / 2, L; N = L, 4 L, 510, 512, 514 (256, 257 and 258 bins) and 1024.
# Every rule lays at least min_segments = 2 segments on the 400-frame walker (the last: 398 second differences hold 3 whole segments of 128)
RULES = ((2, 64, 32, 256), (0, 8, 1, 8), (1, 8, 4, 32), (2, 8, 8, 510), (1, 64, 8, 64), (0, 64, 64, 512), (2, 64, 32, 514), (0, 256, 32, 1024), (1, 256, 128, 256),
         (2, 128, 128, 1024))
LDS_SEGMENTS = 512                                             # csrc/kernels.h's kSpecLdsSegments: more segments than this go to the call's scratch
MEASURED = 1.6e-15                                           # measure_bound's worst ratio, rounded up in the second place (profiles/gait_spectrum_bounds.txt)
BAR = 8.0 * MEASURED


def rule_of(derivative, segment, hop, nfft, **more):
    return dict(RULE, derivative=derivative, segment=segment, hop=hop, nfft=nfft, **more)


def differenced(x, exclude, derivative):
    """y of ONE signal: NaN wherever a frame it reads does not count."""
    x = np.asarray(x, np.float64)
    ok = np.isfinite(x) if exclude is None else np.isfinite(x) & (np.asarray(exclude) == 0)
    y = np.where(ok, x, np.nan)
    with np.errstate(all="ignore"):
        for _ in range(derivative):
            y = np.append(y[1:] - y[:-1], np.nan)
    y[~np.isfinite(y)] = np.nan
    return y


def segments_of(y, segment, hop):
    """The starts of rule 2, by a plain loop over the frames."""
    starts, t, T = [], 0, len(y)
    while t < T:
        if not np.isfinite(y[t]):
            t += 1
            continue
        e = t
        while e < T and np.isfinite(y[e]):
            e += 1
        s = t
        while s + segment <= e:
            starts.append(s)
            s += hop
        t = e
    return starts


def yardstick(x, exclude=None, fps=FPS, derivative=2, segment=64, hop=32, nfft=256, f_lo=0.5, f_hi=3.0, min_segments=2):
    """(psd (nfft/2+1,), n, candidates, used) of ONE signal of ONE sequence, by numpy.fft.rfft."""
    y = differenced(x, exclude, derivative)
    starts = segments_of(y, segment, hop)
    used = len(starts) if len(starts) >= min_segments else 0
    psd = np.full(nfft // 2 + 1, np.nan)
    if used:
        w = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(segment) / segment)
        seg = np.stack([y[s:s + segment] for s in starts])
        X = np.fft.rfft((seg - seg.mean(axis=1, keepdims=True)) * w, n=nfft, axis=1)
        psd = (X.real ** 2 + X.imag ** 2).mean(axis=0) / (fps * (w * w).sum())
        psd[1:nfft // 2] *= 2.0
    return psd, int(np.isfinite(y).sum()), len(starts), used


def ratio(got, want):
    """The worst |got - want| per bin over the row's largest yardstick bin; 0 of two all-NaN or all-zero rows that agree."""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    assert got.shape == want.shape and (np.isnan(got) == np.isnan(want)).all()
    if np.isnan(want).all():
        return 0.0
    top = np.nanmax(want)
    if top == 0.0:
        assert (got == 0.0).all()
        return 0.0
    return float(np.nanmax(np.abs(got - want)) / top)


def runs_call(segment=64, hop=32):
    """(signals (n,4), lengths, exclude): seeded noise whose runs of validity begin and end at frames 63, 64 and 65, by NaN and by exclude, then runs
    exactly segment - 1, segment and segment + hop frames long between NaN frames (derivative 0 keeps a run of x a run of y)."""
    rng = np.random.default_rng(19)
    cases = [(200, (63,), ()), (200, (64,), ()), (200, (65,), (0,)), (200, (0, 1), (63, 64, 65)), (200, (62, 63), (65, 66, 199)), (130, (), (64,)), (200, range(64, 128), ()),
             (200, (), range(0, 64)), (140, range(0, 63), (65,))]
    for run in (segment - 1, segment, segment + hop):
        cases.append((run + 2 + segment, (run, run + 1), ()))      # the run, two NaN frames, then one more segment's worth
        cases.append((run, (), ()))
    lengths = [T for T, _, _ in cases]
    x = rng.standard_normal((sum(lengths), 4))
    ex = np.zeros(sum(lengths), np.int32)
    a = 0
    for T, nans, excluded in cases:
        x[[a + k for k in nans], :] = np.nan
        ex[[a + k for k in excluded]] = 3
        a += T
    return x, lengths, ex


def sinusoid(k0, T=400, nfft=256, fps=FPS, amplitude=0.01):
    """signals (T,4) = a sine at the exact bin frequency k0 fps / nfft on every channel."""
    t = np.arange(T, dtype=np.float64)
    return np.repeat((amplitude * np.sin(2.0 * np.pi * k0 * t / nfft))[:, None], 4, axis=1)


def same_bits(a, b):
    return gc.same_bits(a, b)


def write_case(path, signals, exclude, rule, refused=False):
    """The file tests/helpers/gait_spectrum_check.cpp reads: ONE sequence's signals (T,4) and the call's scalars (refused: a case that the program
    must refuse, and says why; it carries no data)."""
    T = signals.shape[0]
    with open(path, "wb") as f:
        f.write(np.array([T, exclude is not None, rule["derivative"], rule["segment"], rule["hop"], rule["nfft"], rule["min_segments"], not refused], "<i4").tobytes())
        f.write(np.array([rule["fps"], rule["f_lo"], rule["f_hi"]], "<f8").tobytes())
        if refused:
            return path
        f.write(np.ascontiguousarray(signals, "<f8").tobytes())
        if exclude is not None:
            f.write(np.ascontiguousarray(exclude, "<i4").tobytes())
    return path


def parse_output(text):
    """{(what, file, channel): float64 array} of the checker's lines, from their hexadecimal words."""
    out = {}
    for line in text.splitlines():
        part = line.split()
        if part and part[0] in ("psd", "row"):
            out[part[0], part[1], int(part[2])] = np.array([int(w, 16) for w in part[3:]], np.uint64).view(np.float64)
    return out


def shape_set(noisy):
    """(name, signals (n,4), lengths, exclude, rule) of every case the bar is measured over: the noisy call's own signals under RULES, and the runs."""
    signals, lengths, ex = noisy
    cases = [(f"noisy{k}", signals, lengths, ex if k % 2 else None, rule_of(*r)) for k, r in enumerate(RULES)]
    x, run_lengths, run_ex = runs_call()
    cases.append(("runs", x, run_lengths, run_ex, rule_of(0, 64, 32, 256, min_segments=1)))
    x8, run_lengths8, run_ex8 = runs_call(8, 4)
    cases.append(("runs8", x8, run_lengths8, run_ex8, rule_of(0, 8, 4, 32, min_segments=1)))
    return cases


def measure_bound(welch, noisy):
    """(the worst ratio of the statement `welch` against the yardstick over shape_set, the lines of the record)."""
    worst, lines = 0.0, []
    for name, signals, lengths, ex, rule in shape_set(noisy):
        out = welch(signals, lengths, ex, **rule)
        a, here = 0, 0.0
        for q, T in enumerate(lengths):
            for ch in range(4):
                want, n, candidates, used = yardstick(signals[a:a + T, ch], None if ex is None else ex[a:a + T], **rule)
                assert out["per_sequence"][q, ch, :3].tolist() == [n, candidates, used], (name, q, ch)
                here = max(here, ratio(out["psd"][q, ch], want))
            a += T
        lines.append(f"{name}: derivative {rule['derivative']} segment {rule['segment']} hop {rule['hop']} nfft {rule['nfft']}: worst ratio {here:.3e}")
        worst = max(worst, here)
    return worst, lines
