"""The float64 value-and-Jacobian entry points on the host (no GPU): the new symbols are declared and exported, and the selftest hook
molann_selftest_item_jacobian_f64 - the unit-cotangent local Jacobian of one item that frames_value_jac_f64_kernel combines with
d y_k / d feat - agrees with torch.autograd.functional.jacobian of the float64 oracle's item formulas to 1e-12 of scale: every item
type, both use_angle_value modes, random atoms and atoms 1000 A from the origin."""

import ctypes
import os

import numpy as np
import pytest
import torch

from molann_amd import _capi
from oracle import molann_oracle as mo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
SYMBOLS = ["molann_value_and_jacobian_f64", "molann_plan_supports_value_and_jacobian_f64", "molann_selftest_item_jacobian_f64"]
CASES = [(mo.BOND, 2, False), (mo.BOND, 2, True), (mo.ANGLE, 3, False), (mo.ANGLE, 3, True), (mo.DIHEDRAL, 4, False),
         (mo.DIHEDRAL, 4, True), (mo.POSITION, 1, False), (mo.POSITION, 1, True)]


def _dp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_declared_and_exported(name):
    header = open(os.path.join(ROOT, "include", "molann_hip.h")).read()
    assert name + "(" in header, name
    assert hasattr(_capi.lib(), name), name


def test_null_arguments():
    L = _capi.lib()
    assert L.molann_plan_supports_value_and_jacobian_f64(None) == _capi.E_NULL
    assert L.molann_value_and_jacobian_f64(None, None, 1, None, None, None, None, None) == _capi.E_NULL
    a = np.zeros(12)
    assert L.molann_selftest_item_jacobian_f64(mo.BOND, 0, None, _dp(a)) == _capi.E_NULL
    assert L.molann_selftest_item_jacobian_f64(mo.BOND, 0, _dp(a), None) == _capi.E_NULL


def _atoms(where, seed):
    """four-atom geometries: random ones, frames of the alanine-dipeptide golden set (atoms 5, 7, 9, 15); `far` moves each by 1000 A
    along a random direction"""
    g = torch.Generator().manual_seed(seed)
    rnd = torch.randn(16, 4, 3, generator=g, dtype=torch.float64) * 1.5
    gold = torch.from_numpy(np.load(os.path.join(GOLDEN, "align_125_rigid.npz"))["x"][:16][:, [4, 6, 8, 14]]).double()
    a = torch.cat([rnd, gold])
    if where == "far":
        t = torch.randn(a.shape[0], 1, 3, generator=g, dtype=torch.float64)
        a = a + 1000.0 * t / t.norm(dim=2, keepdim=True)
    return a


@pytest.mark.parametrize("where", ["random", "far"])
@pytest.mark.parametrize("type_id,n_atoms,uav", CASES)
def test_item_jacobian_matches_oracle(type_id, n_atoms, uav, where):
    L = _capi.lib()
    idx = list(range(n_atoms))
    width = mo.feature_dim(type_id, n_atoms, uav)
    worst = 0.0
    for a in _atoms(where, seed=31 + type_id):
        want = torch.autograd.functional.jacobian(lambda v: mo.feature_forward(v[None, :n_atoms], type_id, idx, uav).reshape(-1), a)
        want = want.reshape(width, 12).numpy()
        an = np.ascontiguousarray(a.numpy())
        got = np.full(36, np.nan)
        assert L.molann_selftest_item_jacobian_f64(type_id, int(uav), _dp(an), _dp(got)) == width
        got = got.reshape(3, 12)
        scale = max(1.0, np.abs(want).max())
        err = np.abs(got[:width] - want).max()
        worst = max(worst, err / scale)
        assert err <= 1e-12 * scale, (type_id, uav, where, err, scale)
        assert not got[width:].any()                       # rows past the item's width
        assert not got[:, 3 * n_atoms:].any()              # atoms past the item's
    print("item %d uav=%s %s: worst error %.3e of scale" % (type_id, uav, where, worst))


def test_unknown_item_type():
    a, out = np.zeros(12), np.zeros(36)
    assert _capi.lib().molann_selftest_item_jacobian_f64(99, 0, _dp(a), _dp(out)) == _capi.E_FEATURE
