"""The J_regressor override (VPRegressor.forward, pare.py:70-76) without a GPU: the C ABI's new entry points exist and refuse a null handle,
the selection constant and the seed-defined tables are pinned to the reference through tests/golden/vp_jreg.npz (written by
tools/make_goldens_jreg.py from the reference's own VPRegressor), and the Python argument checks raise before a handle is needed."""
import ctypes as C
import os

import numpy as np
import pytest

from .conftest import ROOT, rel_err

NEW = ("grnet_set_joint_regressor", "grnet_joint_regressor_rows", "grnet_regress_joints")


@pytest.fixture(scope="module")
def jreg_golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "vp_jreg.npz"))


def table_of(pkg, recipe):
    rows, nnz, signed, seed = (int(v) for v in recipe)
    return pkg.synth.make_joint_regressor(rows, nnz=None if nnz < 0 else nnz, signed=bool(signed), seed=seed)


def test_entry_points_exist_and_refuse_a_null_handle(pkg):
    lib = pkg._lib.load()
    for name in NEW:
        assert name in pkg._lib.EXPORTS and hasattr(lib, name), name
    W = np.zeros((17, 6890), np.float32)
    assert lib.grnet_set_joint_regressor(None, W.ctypes.data_as(C.c_void_p), 17, None, 0) == pkg._lib.EINVAL
    assert lib.grnet_joint_regressor_rows(None) <= 0
    assert lib.grnet_regress_joints(None, None, 1, None, None) == pkg._lib.EINVAL


def test_selection_constant_is_the_reference_s(pkg, jreg_golden):
    assert list(pkg.netspec.H36M_TO_J14) == [int(i) for i in jreg_golden["H36M_TO_J14"]]
    assert len(pkg.netspec.H36M_TO_J14) == 14


def test_fixture_is_what_the_formula_says(pkg, golden, jreg_golden):
    """Frame 0, whose full vertices are in grnet_n4.npz: the float64 product of each recipe's table, then the reference's selection,
    reproduces the reference's kp_3d (its fp32 matmul sits at ~2.5e-7 of float64)."""
    verts0 = golden["grnet_n4"]["verts_frame0"].astype(np.float64)[None]
    want_shape = {"a": (4, 14, 3), "b": (4, 14, 3), "c": (4, 26, 3), "d": (4, 24, 3)}
    assert sorted(str(c) for c in jreg_golden["cases"]) == sorted(want_shape)
    for name, shape in want_shape.items():
        W = table_of(pkg, jreg_golden[f"recipe_{name}"])
        assert jreg_golden[f"kp_3d_{name}"].shape == shape
        full = np.einsum("jv,nvk->njk", W.astype(np.float64), verts0)
        sel = full[:, pkg.netspec.H36M_TO_J14] if W.shape[0] < 24 else full
        err = rel_err(sel[0], jreg_golden[f"kp_3d_{name}"][0])
        print(f"case {name}: rel_err {err:.2e}")
        assert err < 1e-5, (name, err)
    # a regressor moves nothing but kp_3d
    assert np.array_equal(jreg_golden["kp_2d_a"], jreg_golden["plain_kp_2d"]) and np.array_equal(jreg_golden["theta_a"], jreg_golden["plain_theta"])
    assert np.array_equal(jreg_golden["plain_kp_2d"], golden["grnet_n4"]["kp_2d"].reshape(4, 29, 2))


def test_recipes_cover_sparse_dense_signed(pkg, jreg_golden):
    nnz = {n: (table_of(pkg, jreg_golden[f"recipe_{n}"]) != 0).sum(1) for n in "abcd"}
    assert (nnz["a"] == 32).all() and (nnz["b"] == 6890).all() and (nnz["c"] == 6890).all()
    assert table_of(pkg, jreg_golden["recipe_c"]).min() < 0 < table_of(pkg, jreg_golden["recipe_b"]).min()
    np.testing.assert_allclose(table_of(pkg, jreg_golden["recipe_a"]).astype(np.float64).sum(1), 1.0, atol=1e-6)


def test_argument_checks_need_no_handle(pkg):
    resolve = pkg.grnet.resolve_joint_regressor
    with pytest.raises(ValueError, match="6890"):
        resolve(np.zeros((17, 6889), np.float32))
    with pytest.raises(ValueError, match="6890"):
        resolve(np.zeros((6890,), np.float32))
    with pytest.raises(ValueError, match="17"):
        resolve(np.zeros((16, 6890), np.float32))              # the reference's [:, H36M_TO_J14] would raise IndexError
    with pytest.raises(ValueError, match="row indices"):
        resolve(np.zeros((17, 6890), np.float32), select=[0, 17])
    with pytest.raises(ValueError, match="row indices"):
        resolve(np.zeros((17, 6890), np.float32), select=[-1])
    with pytest.raises(ValueError):
        resolve(np.zeros((17, 6890), np.float32), select="h36m")
    W, sel = resolve(np.zeros((17, 6890), np.float64))
    assert W.dtype == np.float32 and W.flags.c_contiguous and sel == pkg.netspec.H36M_TO_J14
    assert resolve(np.zeros((24, 6890), np.float32))[1] is None and resolve(np.zeros((17, 6890), np.float32), select=None)[1] is None
    assert resolve(np.zeros((16, 6890), np.float32), select=[3, 3, 0])[1] == [3, 3, 0]
