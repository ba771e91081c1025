#!/usr/bin/env python3
"""Golden vectors for the J_regressor override (VPRegressor.forward, lib/models/pare.py:70-76), produced by RUNNING the reference's own
VPRegressor in this container on the head outputs stored in tests/golden/grnet_n4.npz (pred_rotmat, pred_shape, pred_cam) and on
seed-defined tables (synth.make_joint_regressor).  Only data is written -- tests/golden/vp_jreg.npz: the recipe of each table
(rows, nnz, signed, seed; nnz -1 = dense), H36M_TO_J14 as lib.models.smpl defines it, the reference's kp_3d per case, and kp_2d / theta
of the first case and of the call without a regressor (they must not move).

    python tools/make_goldens_jreg.py <path of the reference checkout>     (default: the path tools/make_goldens.py uses)

Stubs for absent third-party modules and the synthetic SMPL tables are tools/make_goldens.py's.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_goldens as mg  # noqa: E402

ROOT, synth = mg.ROOT, mg.synth

# name -> (rows, nnz or None for dense, signed)
CASES = {
    "a": (17, 32, False),      # sparse, row-stochastic            -> (4,14,3)
    "b": (17, None, False),    # dense, positive                    -> (4,14,3)
    "c": (26, None, True),     # dense, signed                      -> (4,26,3)
    "d": (24, 32, False),      # the `< 24` boundary: no selection  -> (4,24,3)
}
SEED = synth.SMPL_SEED


def main():
    import torch
    torch.manual_seed(0)
    ref = sys.argv[1] if len(sys.argv) > 1 else mg.REF
    tmp, stubs, sd, smpl = mg.setup_workdir()
    os.chdir(tmp)
    sys.path[:0] = [stubs, ref]
    from lib.models.pare import VPRegressor
    from lib.models.smpl import H36M_TO_J14

    g = np.load(os.path.join(ROOT, "tests/golden/grnet_n4.npz"))
    n = int(g["n_frames"])
    patt = {"pred_pose": torch.from_numpy(g["pred_rotmat"]), "pred_shape": torch.from_numpy(g["pred_shape"]),
            "pred_cam": torch.from_numpy(g["pred_cam"])}
    reg = VPRegressor().eval()
    out = {"H36M_TO_J14": np.asarray(H36M_TO_J14, np.int64), "cases": np.asarray(sorted(CASES))}
    with torch.no_grad():
        plain = reg(dict(patt), batch_size=1)[-1]
        assert np.allclose(plain["verts"].numpy()[0, 0], g["verts_frame0"], rtol=0, atol=1e-6), "VPRegressor does not reproduce grnet_n4.npz"
        out["plain_kp_2d"], out["plain_theta"] = plain["kp_2d"].numpy()[0], plain["theta"].numpy()[0]
        for name, (rows, nnz, signed) in sorted(CASES.items()):
            W = synth.make_joint_regressor(rows, nnz=nnz, signed=signed, seed=SEED)
            res = reg(dict(patt), batch_size=1, J_regressor=torch.from_numpy(W))[-1]
            for k in ("verts", "kp_2d", "theta", "rotmat"):
                assert torch.equal(res[k], plain[k]), (name, k)
            kp = res["kp_3d"].numpy()[0]
            out[f"recipe_{name}"] = np.asarray([rows, -1 if nnz is None else nnz, int(signed), SEED], np.int64)
            out[f"kp_3d_{name}"] = kp
            if name == "a":
                out["kp_2d_a"], out["theta_a"] = res["kp_2d"].numpy()[0], res["theta"].numpy()[0]
            print(f"case {name}: table {W.shape} nnz/row {int((W != 0).sum(1).max())} -> kp_3d {kp.shape} absmax {np.abs(kp).max():.4f}")
    assert out["kp_3d_a"].shape == (n, 14, 3) and out["kp_3d_c"].shape == (n, 26, 3) and out["kp_3d_d"].shape == (n, 24, 3)
    p = os.path.join(ROOT, "tests/golden/vp_jreg.npz")
    np.savez_compressed(p, **out)
    print(f"wrote {p} ({os.path.getsize(p) / 1e3:.1f} kB)")


if __name__ == "__main__":
    main()
