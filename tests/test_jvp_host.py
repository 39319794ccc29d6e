"""Forward-mode math on the host (no GPU): the selftest hooks compile the __host__ __device__ item and Kabsch tangents that
frames_jvp_kernel is built from; they must agree with torch.func.jvp through the float64 oracle, and the Kabsch tangent must
be the adjoint of the Kabsch backward.  Also the new entry points' symbols, their null-plan answer, and the refusal of CPU
tensors under torch.func.jvp."""

import ctypes
import os

import numpy as np
import pytest
import torch

from molann_amd import _capi
from oracle import molann_oracle as mo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = [(mo.BOND, 2, False), (mo.ANGLE, 3, False), (mo.ANGLE, 3, True), (mo.DIHEDRAL, 4, False), (mo.DIHEDRAL, 4, True),
         (mo.POSITION, 1, False)]


def _dp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _item_frames(n_atoms, seed):
    """random four-atom geometries and the first frames of the alanine-dipeptide golden set (atoms 5, 7, 9, 15)"""
    g = torch.Generator().manual_seed(seed)
    rnd = torch.randn(24, 4, 3, generator=g, dtype=torch.float64) * 1.5
    gold = torch.from_numpy(np.load(os.path.join(GOLDEN, "align_125_rigid.npz"))["x"][:24][:, [4, 6, 8, 14]]).double()
    return torch.cat([rnd, gold])


@pytest.mark.parametrize("type_id,n_atoms,uav", CASES)
def test_item_tangent_matches_oracle_jvp(type_id, n_atoms, uav):
    L = _capi.lib()
    frames = _item_frames(n_atoms, seed=7 + type_id)
    tangents = torch.randn(frames.shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    idx = list(range(n_atoms))
    for a, t in zip(frames, tangents):
        want, dwant = torch.func.jvp(lambda x: mo.feature_forward(x, type_id, idx, uav), (a[None],), (t[None],))
        want, dwant = want.reshape(-1), dwant.reshape(-1)
        an, tn = np.ascontiguousarray(a.numpy()), np.ascontiguousarray(t.numpy())
        out, dout = np.zeros(3), np.zeros(3)
        w = L.molann_selftest_feature_tangent_f64(type_id, int(uav), _dp(an), _dp(tn), _dp(out), _dp(dout))
        assert w == want.numel()
        scale = max(1.0, float(dwant.abs().max()))
        assert np.abs(out[:w] - want.numpy()).max() <= 1e-12 * max(1.0, float(want.abs().max()))
        assert np.abs(dout[:w] - dwant.numpy()).max() <= 1e-9 * scale, (type_id, uav, dout[:w], dwant)
        # the float32 instantiation: the same formulas at float32 rounding
        af, tf = an.astype(np.float32), tn.astype(np.float32)
        out32, dout32 = np.zeros(3, np.float32), np.zeros(3, np.float32)
        assert L.molann_selftest_feature_tangent_f32(type_id, int(uav), _dp(af), _dp(tf), _dp(out32), _dp(dout32)) == w
        assert np.abs(dout32[:w] - dwant.numpy()).max() <= 1e-3 * scale


def _kabsch_parts(x, v, align, ref):
    """(H, R, dH, e0) of one frame as the kernels form them (double), with R from the float64 solver hook"""
    p, dp = x[align], v[align]
    c, dc = p.mean(0), dp.mean(0)
    H = ((p - c).T @ ref).contiguous()
    dH = ((dp - dc).T @ ref).contiguous()
    e0 = 0.5 * (float(((p - c) ** 2).sum()) + float((ref ** 2).sum())) * 1.0001
    R = np.zeros(9)
    Hn = np.ascontiguousarray(H.numpy())
    assert _capi.lib().molann_selftest_kabsch_rotation_f64(_dp(Hn), e0, _dp(R)) == 0
    return Hn, R, np.ascontiguousarray(dH.numpy()), c, dc


def _alignment_cases():
    xyz = torch.from_numpy(np.load(os.path.join(GOLDEN, "ala_dipeptide_pdb.npz"))["xyz"]).double()
    out = []
    for name in ("align_125_centred.npz", "align_backbone_rigid.npz", "align_P1.npz"):
        d = np.load(os.path.join(GOLDEN, name))
        align = [int(a) - 1 for a in d["align_numbers"]]
        x = torch.from_numpy(d["x"][:12]).double()
        if x.shape[1] == 22:
            ref = mo.center_reference(xyz[align].float()).double()
        else:
            ref = mo.center_reference(x[0, align].float()).double()     # P1: a frame of its own as the reference
        out.append((name, x, align, ref))
    g = torch.Generator().manual_seed(11)
    base = torch.randn(9, 3, generator=g, dtype=torch.float64) * 2.0
    x = base + 0.3 * torch.randn(10, 9, 3, generator=g, dtype=torch.float64)
    out.append(("random", x, [0, 2, 3, 5, 8], mo.center_reference(base[[0, 2, 3, 5, 8]].float()).double()))
    return out


@pytest.mark.parametrize("case", _alignment_cases(), ids=lambda c: c[0])
def test_kabsch_tangent_matches_oracle_jvp(case):
    """dy = (dp - dc) R + (p - c) dR with dR from the tangent hook equals torch.func.jvp of the oracle's alignment (its SVD)"""
    name, xs, align, ref = case
    L = _capi.lib()
    vs = torch.randn(xs.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    for x, v in zip(xs, vs):
        y, dy = torch.func.jvp(lambda a: mo.align_forward(a, align, ref), (x[None],), (v[None],))
        H, R, dH, c, dc = _kabsch_parts(x, v, align, ref)
        dR = np.zeros(9)
        assert L.molann_selftest_kabsch_tangent(_dp(H), _dp(R), _dp(dH), _dp(dR)) == 0
        Rt, dRt = torch.from_numpy(R).view(3, 3), torch.from_numpy(dR).view(3, 3)
        got_y = (x - c) @ Rt
        got_dy = (v - dc) @ Rt + (x - c) @ dRt
        scale = float(y.abs().max())
        assert float((got_y - y[0]).abs().max()) <= 1e-9 * scale, name
        assert float((got_dy - dy[0]).abs().max()) <= 1e-9 * max(scale, float(dy.abs().max())), name


@pytest.mark.parametrize("regime", ["mirror", "flip180", "hinge", "offset"])
def test_kabsch_tangent_on_far_frames_matches_oracle_jvp(regime):
    """The tangent hook on covariances of frames far from the reference (tests/far_frames.py): the d = -1 branch, exact
    180-degree turns, hinge motions, frames 100-1000 A from the origin.  Compared where the rotation is well conditioned."""
    import far_frames as ff
    from molann_amd import workloads as wl
    L = _capi.lib()
    xyz = wl.ALA_DIPEPTIDE_XYZ
    for align in (list(range(22)), [1, 4, 6, 8, 14, 16, 18]):
        ref = mo.center_reference(torch.from_numpy(np.asarray(xyz, np.float32)[align])).double()
        frames = ff.draw(regime, xyz, align, 16, seed=4)
        cond = ff.conditioning(frames, xyz, align)
        xs = torch.from_numpy(frames).double()
        vs = torch.randn(xs.shape, generator=torch.Generator().manual_seed(6), dtype=torch.float64)
        compared = 0
        for x, v, c in zip(xs, vs, cond):
            H, R, dH, cen, dc = _kabsch_parts(x, v, align, ref)
            dR = np.zeros(9)
            assert L.molann_selftest_kabsch_tangent(_dp(H), _dp(R), _dp(dH), _dp(dR)) == 0
            assert np.isfinite(dR).all(), (regime, dR)
            if c < 1e-2:
                continue
            y, dy = torch.func.jvp(lambda a: mo.align_forward(a, align, ref), (x[None],), (v[None],))
            Rt, dRt = torch.from_numpy(R).view(3, 3), torch.from_numpy(dR).view(3, 3)
            got_dy = (v - dc) @ Rt + (x - cen) @ dRt
            assert float(((x - cen) @ Rt - y[0]).abs().max()) <= 1e-9 * float(y.abs().max()), (regime, "y")
            assert float((got_dy - dy[0]).abs().max()) <= 1e-9 * float(dy.abs().max()), (regime, len(align), float(c))
            compared += 1
        assert compared >= len(xs) // 2, (regime, compared)


def test_kabsch_tangent_is_finite_on_singular_covariances():
    """No defined rotation: all align atoms at one point (H = 0: dR = 0) or exactly on a line (rank 1), 1000 A out."""
    L = _capi.lib()
    ref = mo.center_reference(torch.randn(6, 3, generator=torch.Generator().manual_seed(1), dtype=torch.float64)).double()
    line = np.outer(np.arange(6.0) - 2.5, [0.3, 0.5, 0.8])
    for name, P in (("one point", np.full((6, 3), 1000.0)), ("collinear", line + 1000.0), ("collinear at 0", line)):
        x = torch.from_numpy(P)
        for seed in range(4):
            v = torch.randn(x.shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
            H, R, dH, _, _ = _kabsch_parts(x, v, list(range(6)), ref)
            assert np.isfinite(R).all(), name
            dR = np.full(9, np.nan)
            assert L.molann_selftest_kabsch_tangent(_dp(H), _dp(R), _dp(dH), _dp(dR)) == 0
            assert np.isfinite(dR).all(), (name, dR)
            if name == "one point":
                assert not dR.any(), dR


def test_scripted_module_refuses_forward_mode():
    """molann::run has no forward-mode derivative: a dual or torch.func.jvp input raises (pointing to the eager module) before
    any kernel runs, in float32 and float64, instead of returning the primal without a tangent."""
    from torch.autograd import forward_ad as fwAD
    from molann_amd import workloads as wl
    from build_util import workload_model
    for name in ("C3", "A3", "C2"):
        w = wl.get_workload(name)
        scripted = torch.jit.script(workload_model(w, torch.device("cpu")))
        x = w.make_frames(2, seed=1)
        for dtype in (torch.float32, torch.float64):
            m = scripted.to(dtype)
            xd = x.to(dtype)
            with pytest.raises(RuntimeError, match="no forward-mode derivative.*eager molann_amd module"):
                with fwAD.dual_level():
                    m(fwAD.make_dual(xd, torch.ones_like(xd)))
            with pytest.raises(RuntimeError, match="no forward-mode derivative"):
                torch.func.jvp(m, (xd,), (torch.ones_like(xd),))


def test_kabsch_tangent_is_the_adjoint_of_the_backward():
    """<dR, G_R> = <dH, G_H> with G_H from the backward's hook, for random directions and cotangents"""
    L = _capi.lib()
    g = torch.Generator().manual_seed(2)
    for _, xs, align, ref in _alignment_cases():
        for x in xs[:4]:
            v = torch.randn(x.shape, generator=g, dtype=torch.float64)
            H, R, dH, _, _ = _kabsch_parts(x, v, align, ref)
            dH = dH.reshape(9)
            GR = np.ascontiguousarray(torch.randn(9, generator=g, dtype=torch.float64).numpy())
            dR, GH = np.zeros(9), np.zeros(9)
            assert L.molann_selftest_kabsch_tangent(_dp(H), _dp(R), _dp(dH), _dp(dR)) == 0
            assert L.molann_selftest_kabsch_backward_f64(_dp(H), _dp(R), _dp(GR), _dp(GH)) == 0
            lhs, rhs = float(dR @ GR), float(dH @ GH)
            assert abs(lhs - rhs) <= 1e-12 * max(1.0, np.abs(dR).max() * np.abs(GR).sum(), np.abs(dH).max() * np.abs(GH).sum())
            # the float32 backward hook the kernels of float32 plans use: the same identity at float32 rounding
            R32, GR32, GH32 = R.astype(np.float32), GR.astype(np.float32), np.zeros(9, np.float32)
            assert L.molann_selftest_kabsch_backward(_dp(H), _dp(R32), _dp(GR32), _dp(GH32)) == 0
            assert abs(float(dH @ GH32.astype(np.float64)) - lhs) <= 1e-4 * max(1.0, abs(lhs), np.abs(dH).max() * np.abs(GH).sum())


def test_jvp_symbols_declared_exported_and_null_plan():
    L = _capi.lib()
    names = _capi.declared_symbols()
    for n in ("molann_features_jvp_f32", "molann_features_jvp_f64", "molann_selftest_feature_tangent_f32",
              "molann_selftest_feature_tangent_f64", "molann_selftest_kabsch_tangent", "molann_selftest_kabsch_rotation_f64",
              "molann_selftest_kabsch_backward_f64"):
        assert n in names and hasattr(L, n), n
    for fn in (L.molann_features_jvp_f32, L.molann_features_jvp_f64):
        assert fn(None, None, None, 0, 1, None, None, None) == _capi.E_NULL
        assert fn(None, None, None, 4, 2, None, None, None) == _capi.E_NULL
    assert L.molann_selftest_kabsch_tangent(None, None, None, None) == _capi.E_NULL
    assert L.molann_selftest_feature_tangent_f64(0, 0, None, None, None, None) == _capi.E_NULL


def test_cpu_tensors_still_raise_under_forward_mode():
    from molann_amd import workloads as wl
    for name in ("C3", "A3"):
        w = wl.get_workload(name)
        model = wl.build_model(w)
        x = w.make_frames(2, seed=1)
        with pytest.raises(RuntimeError, match="MI355X only"):
            torch.func.jvp(model, (x,), (torch.ones_like(x),))
