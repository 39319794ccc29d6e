"""Second-order math on the host (no GPU): the selftest hooks compile the __host__ __device__ tangents of the reverse pass that
frames_hvp_kernel is built from.  The item backward's tangent and the Kabsch backward's tangent must agree with float64 double
autograd through the oracle's formulas (for the rotation: its SVD) to 1e-12 of scale.  Also the new entry point's symbol and
its answers to a null plan."""

import ctypes
import os

import numpy as np
import pytest
import torch

import far_frames as ff
from molann_amd import _capi
from molann_amd import workloads as wl
from oracle import molann_oracle as mo

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = [(mo.BOND, 2, False), (mo.ANGLE, 3, False), (mo.ANGLE, 3, True), (mo.DIHEDRAL, 4, False), (mo.DIHEDRAL, 4, True),
         (mo.POSITION, 1, False)]


def _dp(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _vjp_and_tangent(vjp, inputs, tangents):
    """(vjp(*inputs), its derivative along `tangents`) by double backward: the gradient of <vjp, w> with respect to the inputs
    is linear in w, and the gradient of <that, tangents> with respect to w is the wanted derivative"""
    xs = [a.clone().requires_grad_(True) for a in inputs]
    out = vjp(*xs)
    w = torch.zeros_like(out, requires_grad=True)
    inner = torch.autograd.grad((out * w).sum(), xs, create_graph=True, allow_unused=True)
    s = sum((i * t).sum() for i, t in zip(inner, tangents) if i is not None)
    (d,) = torch.autograd.grad(s, w, allow_unused=True)
    return out.detach(), (torch.zeros_like(out) if d is None else d)


def _item_frames(seed):
    """random four-atom geometries and frames of the alanine-dipeptide golden set (atoms 5, 7, 9, 15)"""
    g = torch.Generator().manual_seed(seed)
    rnd = torch.randn(24, 4, 3, generator=g, dtype=torch.float64) * 1.5
    gold = torch.from_numpy(np.load(os.path.join(GOLDEN, "align_125_rigid.npz"))["x"][:24][:, [4, 6, 8, 14]]).double()
    return torch.cat([rnd, gold])


@pytest.mark.parametrize("type_id,n_atoms,uav", CASES)
def test_item_backward_tangent_matches_oracle_double_backward(type_id, n_atoms, uav):
    """ga = J^T g and dga = d/de [J(a + e t)^T (g + e dg)] of one item against torch double backward through the oracle's
    feature formula, within 1e-12 of scale"""
    L = _capi.lib()
    gen = torch.Generator().manual_seed(9)
    idx = list(range(n_atoms))
    width = mo.feature_dim(type_id, n_atoms, uav)

    def vjp(x, gg):
        f = mo.feature_forward(x[None, :n_atoms], type_id, idx, uav).reshape(-1)
        (gx,) = torch.autograd.grad((f * gg).sum(), x, create_graph=True)
        return gx

    for a in _item_frames(seed=17 + type_id):
        t = torch.randn(4, 3, generator=gen, dtype=torch.float64)
        g = torch.randn(width, generator=gen, dtype=torch.float64)
        dg = torch.randn(width, generator=gen, dtype=torch.float64)
        ga_want, dga_want = _vjp_and_tangent(vjp, (a, g), (t, dg))
        ga_want = ga_want.reshape(-1).numpy()[:3 * n_atoms]
        dga_want = dga_want.reshape(-1).numpy()[:3 * n_atoms]
        an, tn = np.ascontiguousarray(a.numpy()), np.ascontiguousarray(t.numpy())
        g3, dg3 = np.zeros(3), np.zeros(3)
        g3[:width], dg3[:width] = g.numpy(), dg.numpy()
        ga, dga = np.full(12, np.nan), np.full(12, np.nan)
        n = L.molann_selftest_feature_backward_tangent_f64(type_id, int(uav), _dp(an), _dp(tn), _dp(g3), _dp(dg3), _dp(ga), _dp(dga))
        assert n == n_atoms
        assert np.abs(ga[:3 * n_atoms] - ga_want).max() <= 1e-12 * max(1.0, np.abs(ga_want).max()), (type_id, uav)
        assert np.abs(dga[:3 * n_atoms] - dga_want).max() <= 1e-12 * max(1.0, np.abs(dga_want).max()), (type_id, uav, dga, dga_want)
        assert not ga[3 * n_atoms:].any() and not dga[3 * n_atoms:].any()


def _oracle_rotation(h):
    """the oracle's rotation (ann.py:188-195) of one covariance"""
    u, _, vh = torch.linalg.svd(h)
    d = torch.ones(3, dtype=h.dtype)
    d[2] = torch.sign(torch.linalg.det(u @ vh)).detach()
    return u @ torch.diag(d) @ vh


def _kabsch_case(P, ref, GR, dP, dGR):
    """(hook G_H, hook dG_H, oracle G_H, oracle dG_H) for align atoms P, the centred reference, a cotangent G_R on R and
    directions dP, dG_R: the oracle's G_H = d<G_R, R(H)>/dH through its SVD and its derivative along (dH, dG_R)"""
    L = _capi.lib()
    c, dc = P.mean(0), dP.mean(0)
    H = ((P - c).T @ ref).contiguous()
    dH = ((dP - dc).T @ ref).contiguous()
    e0 = 0.5 * (float(((P - c) ** 2).sum()) + float((ref ** 2).sum())) * 1.0001
    Hn, dHn = np.ascontiguousarray(H.numpy()).reshape(9), np.ascontiguousarray(dH.numpy()).reshape(9)
    R, dR = np.zeros(9), np.zeros(9)
    assert L.molann_selftest_kabsch_rotation_f64(_dp(Hn), e0, _dp(R)) == 0
    assert L.molann_selftest_kabsch_tangent(_dp(Hn), _dp(R), _dp(dHn), _dp(dR)) == 0
    GRn, dGRn = np.ascontiguousarray(GR.numpy()).reshape(9), np.ascontiguousarray(dGR.numpy()).reshape(9)
    GH, dGH = np.full(9, np.nan), np.full(9, np.nan)
    assert L.molann_selftest_kabsch_backward_tangent(_dp(Hn), _dp(R), _dp(GRn), _dp(dHn), _dp(dR), _dp(dGRn), _dp(GH), _dp(dGH)) == 0
    GH0 = np.zeros(9)
    assert L.molann_selftest_kabsch_backward_f64(_dp(Hn), _dp(R), _dp(GRn), _dp(GH0)) == 0
    assert np.array_equal(GH, GH0)      # the value part is the float64 backward's own G_H, bit for bit

    def vjp(h, gr):
        (gh,) = torch.autograd.grad((_oracle_rotation(h) * gr).sum(), h, create_graph=True)
        return gh

    GHw, dGHw = _vjp_and_tangent(vjp, (H, GR), (dH, dGR))
    return GH, dGH, GHw.reshape(-1).numpy(), dGHw.reshape(-1).numpy()


def _kabsch_frames():
    out = []
    xyz = torch.from_numpy(np.load(os.path.join(GOLDEN, "ala_dipeptide_pdb.npz"))["xyz"]).double()
    for name in ("align_125_centred.npz", "align_backbone_rigid.npz"):
        d = np.load(os.path.join(GOLDEN, name))
        align = [int(a) - 1 for a in d["align_numbers"]]
        ref = mo.center_reference(xyz[align].float()).double()
        for x in torch.from_numpy(d["x"][:8]).double():
            out.append((name, x[align], ref))
    g = torch.Generator().manual_seed(21)
    base = torch.randn(7, 3, generator=g, dtype=torch.float64) * 2.0
    ref = mo.center_reference(base.float()).double()
    for _ in range(8):
        out.append(("random", base + 0.4 * torch.randn(7, 3, generator=g, dtype=torch.float64), ref))
    return out


def test_kabsch_backward_tangent_matches_oracle_double_backward():
    """G_H and its derivative along (dH, dR, dG_R) against double autograd through the oracle's SVD, within 1e-12 of scale, on
    random frames and the golden frames of two alignment sets"""
    gen = torch.Generator().manual_seed(4)
    for name, P, ref in _kabsch_frames():
        dP = torch.randn(P.shape, generator=gen, dtype=torch.float64)
        GR = torch.randn(3, 3, generator=gen, dtype=torch.float64)
        dGR = torch.randn(3, 3, generator=gen, dtype=torch.float64)
        GH, dGH, GHw, dGHw = _kabsch_case(P, ref, GR, dP, dGR)
        assert np.abs(GH - GHw).max() <= 1e-12 * max(1.0, np.abs(GHw).max()), name
        assert np.abs(dGH - dGHw).max() <= 1e-12 * max(1.0, np.abs(dGHw).max()), (name, dGH, dGHw)


@pytest.mark.parametrize("regime", list(ff.REGIMES))
def test_kabsch_backward_tangent_on_far_frames(regime):
    """The regimes of tests/far_frames.py on two alignment sets; every result is finite.  A frame whose rotation is well
    conditioned (c = (s2 + d s3) / s1 >= 1e-2) is held to 1e-12 of scale.  An ill-conditioned one (1e-6 <= c < 1e-2) is held to
    1e-14 / c^2 of scale: dG_H divides by the gap c twice, so the rounding of R and H reaches it amplified by 1 / c^2.  Below
    1e-6 the rotation is not defined to double precision and only finiteness is checked."""
    xyz = wl.ALA_DIPEPTIDE_XYZ
    gen = torch.Generator().manual_seed(8)
    compared = 0
    for align in (list(range(22)), [1, 4, 6, 8, 14, 16, 18]):
        ref = mo.center_reference(torch.from_numpy(np.asarray(xyz, np.float32)[align])).double()
        frames = ff.draw(regime, xyz, align, 12, seed=3)
        cond = ff.conditioning(frames, xyz, align)
        for x, c in zip(torch.from_numpy(frames).double(), cond):
            P = x[align]
            dP = torch.randn(P.shape, generator=gen, dtype=torch.float64)
            GR = torch.randn(3, 3, generator=gen, dtype=torch.float64)
            dGR = torch.randn(3, 3, generator=gen, dtype=torch.float64)
            GH, dGH, GHw, dGHw = _kabsch_case(P, ref, GR, dP, dGR)
            assert np.isfinite(GH).all() and np.isfinite(dGH).all(), (regime, c)
            if not c >= 1e-6:
                continue
            rel = 1e-12 if c >= 1e-2 else 1e-14 / c ** 2
            assert np.abs(GH - GHw).max() <= rel * max(1.0, np.abs(GHw).max()), (regime, float(c))
            assert np.abs(dGH - dGHw).max() <= rel * max(1.0, np.abs(dGHw).max()), (regime, float(c))
            compared += 1
    if regime != "degenerate":
        assert compared >= 12, (regime, compared)


def test_kabsch_backward_tangent_is_finite_on_singular_covariances():
    """No defined rotation (all align atoms at one point, or on a line, 1000 A out): G_H and dG_H are finite, and zero at a point"""
    L = _capi.lib()
    line = np.outer(np.arange(6.0) - 2.5, [0.3, 0.5, 0.8])
    gen = torch.Generator().manual_seed(1)
    ref = mo.center_reference(torch.randn(6, 3, generator=gen, dtype=torch.float64)).double()
    for name, P in (("one point", np.full((6, 3), 1000.0)), ("collinear", line + 1000.0)):
        P = torch.from_numpy(P)
        H = np.ascontiguousarray(((P - P.mean(0)).T @ ref).numpy()).reshape(9)
        R = np.zeros(9)
        assert L.molann_selftest_kabsch_rotation_f64(_dp(H), 1.0, _dp(R)) == 0
        for _ in range(3):
            dH, dR, GR, dGR = (np.ascontiguousarray(torch.randn(9, generator=gen, dtype=torch.float64).numpy()) for _ in range(4))
            GH, dGH = np.full(9, np.nan), np.full(9, np.nan)
            assert L.molann_selftest_kabsch_backward_tangent(_dp(H), _dp(R), _dp(GR), _dp(dH), _dp(dR), _dp(dGR), _dp(GH), _dp(dGH)) == 0
            assert np.isfinite(GH).all() and np.isfinite(dGH).all(), name
            if name == "one point":
                assert not GH.any() and not dGH.any()


def test_hvp_symbols_declared_exported_and_null_plan():
    L = _capi.lib()
    names = _capi.declared_symbols()
    for n in ("molann_features_hvp_f64", "molann_selftest_feature_backward_tangent_f64", "molann_selftest_kabsch_backward_tangent"):
        assert n in names and hasattr(L, n), n
    assert L.molann_features_hvp_f64(None, None, None, None, 0, None, None, None) == _capi.E_NULL
    assert L.molann_features_hvp_f64(None, None, None, None, 4, None, None, None) == _capi.E_NULL
    assert L.molann_selftest_kabsch_backward_tangent(None, None, None, None, None, None, None, None) == _capi.E_NULL
    assert L.molann_selftest_feature_backward_tangent_f64(1, 0, None, None, None, None, None, None) == _capi.E_NULL
    a = np.zeros(12)
    assert L.molann_selftest_feature_backward_tangent_f64(9, 0, _dp(a), _dp(a), _dp(a), _dp(a), _dp(a), _dp(a)) == _capi.E_FEATURE
