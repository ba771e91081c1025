"""oracle.float64(): the float64 mode the fp32 stage tests (tests/test_gpu_f32_stages.py) take their references from."""
import numpy as np
import torch

from .conftest import rel_err


def test_float64_oracle_agrees_with_fp32_oracle_on_golden_frames(pkg, oracle, synth_weights, synth_smpl):
    """A forward on the 4 golden frames under float64() agrees with the fp32 oracle on `features` and `point_local_feat` to 1e-5 of their scale (the
    fp32 oracle's own rounding), its backbone and head tensors are float64, and leaving the context restores float32."""
    frames = pkg.synth.make_frames(4)
    ref = oracle.grnet_forward(frames, synth_weights, synth_smpl, return_intermediates=True)
    with oracle.float64():
        d = oracle.grnet_forward(frames, synth_weights, synth_smpl, return_intermediates=True)
        assert oracle.conv_bn(torch.zeros(1, 64, 8, 8), synth_weights, "backbone.conv2.weight", "backbone.bn2").dtype == torch.float64
    for k in ("features", "point_local_feat"):
        assert d[k].dtype == np.float64, k
        e = rel_err(ref[k], d[k])
        assert 0 < e <= 1e-5, (k, e)
    assert oracle.conv_bn(torch.zeros(1, 64, 8, 8), synth_weights, "backbone.conv2.weight", "backbone.bn2").dtype == torch.float32
