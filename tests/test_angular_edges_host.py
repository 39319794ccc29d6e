"""The item arithmetic of molann_amd/csrc/molann_math.h at angular extremes, on the CPU: every variant the kernels inline
(eval_item / eval_item_backward in float32, eval_item_tangent_t<float|double>, eval_item_backward_f64 through
item_unit_backward_f64, eval_item_backward_gen<Dual>) runs through its molann_selftest_* hook on the frames of
tests/angular_edges.py - bond angles a few degrees to a thousandth of a degree from straight or folded, dihedrals at cis and
trans where atan2 wraps, dihedrals with a nearly collinear arm - one item at a time, on the raw float32 atoms.

The reference is mpmath at 60 digits on the float32 coordinates as stored: values from atan2 forms, gradients from closed forms
that share nothing with the header's (the angle's through w = u x v, the dihedral's through its two normals).  The same run holds
the oracle's float64 autograd to the float64 bound, so that the GPU tests may trust the oracle on these frames.

Bounds, relative to max(1, the frame's largest entry) for float32 and for all values, and to the frame's largest gradient entry
for float64 gradients (a tangent, a sum of products of gradient and tangent entries, to the sum of their sizes):
  float32 hooks, graded frames   max(the floor of test_host_math.py - 2e-6 for values, 2e-5 for gradients -, 2 x the largest error
                                 of the oracle run in float32 on the same regime and delta)
  float64 hooks, graded frames   16 * 2^-52 / sin^2(theta): a dozen roundings, each amplified by at most 1 / sin^2
  pole frames (0.03 degrees, 0)  an angle-value gradient row is non-finite, as the reference's autograd gives there, or obeys
                                 |d theta / d x_end| <= (1 + 1e-3) / |arm|; never a finite value beyond that
Dihedral values are compared modulo 2 pi.  No frame is left out."""

import ctypes
import math

import mpmath as mp
import numpy as np
import pytest
import torch

import angular_edges as ae
from molann_amd import _capi
from molann_amd import workloads as wl
from oracle import molann_oracle as mo

mp.mp.dps = 60
N = 64
ITEMS = [(ae.ANGLE, [1, 4, 5]), (ae.DIH, [4, 6, 8, 14]), (ae.DIH, [12, 10, 8, 9]), (ae.BOND, [1, 4])]
EPS64 = 2.0 ** -52
TWO_PI = 2.0 * math.pi


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


# ---- the reference: mpmath -------------------------------------------------------------------------------------------------
def _sub(a, b):
    return [a[0] - b[0], a[1] - b[1], a[2] - b[2]]


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _cross(a, b):
    return [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]


def _scale(s, a):
    return [s * a[0], s * a[1], s * a[2]]


def _mp_angle(p):
    """theta and d theta / d atoms [3][3] of the angle at p[1]."""
    u, v = _sub(p[0], p[1]), _sub(p[2], p[1])
    w = _cross(u, v)
    nw = mp.sqrt(_dot(w, w))
    theta = mp.atan2(nw, _dot(u, v))
    if nw == 0:
        return theta, None
    g0 = _scale(1 / (_dot(u, u) * nw), _cross(u, w))
    g2 = _scale(1 / (_dot(v, v) * nw), _cross(w, v))
    g1 = [-(g0[k] + g2[k]) for k in range(3)]
    return theta, [g0, g1, g2]


def _mp_dihedral(p):
    """phi (the reference's convention, ann.py:339-349) and d phi / d atoms [4][3]."""
    b1, b2, b3 = _sub(p[1], p[0]), _sub(p[2], p[1]), _sub(p[3], p[2])
    n1, n2 = _cross(b1, b2), _cross(b2, b3)
    L2 = _dot(b2, b2)
    L = mp.sqrt(L2)
    phi = mp.atan2(_dot(n1, b3) * L, _dot(n1, n2))
    m1, m2 = _dot(n1, n1), _dot(n2, n2)
    if m1 == 0 or m2 == 0:
        return phi, None
    g0 = _scale(-L / m1, n1)
    g3 = _scale(L / m2, n2)
    f1, f3 = _dot(b1, b2) / L2, _dot(b3, b2) / L2
    g1 = [-(f1 + 1) * g0[k] + f3 * g3[k] for k in range(3)]
    g2 = [f1 * g0[k] - (f3 + 1) * g3[k] for k in range(3)]
    return phi, [g0, g1, g2, g3]


def _reference(kind, uav, atoms):
    """(values [w], jacobian [w, n_atoms, 3]) of one item in float64 from mpmath; the jacobian None at an exact pole."""
    p = [[mp.mpf(float(c)) for c in a] for a in atoms]
    val, g = _mp_angle(p) if kind == ae.ANGLE else _mp_dihedral(p)
    if kind == ae.ANGLE:
        outs = [(val, mp.mpf(1))] if uav else [(mp.cos(val), -mp.sin(val))]
    else:
        outs = [(val, mp.mpf(1))] if uav else [(mp.cos(val), -mp.sin(val)), (mp.sin(val), mp.cos(val))]
    vals = np.array([float(o) for o, _ in outs])
    if g is None:
        return vals, None
    return vals, np.array([[[float(s * c) for c in row] for row in g] for _, s in outs])


# ---- the hooks -------------------------------------------------------------------------------------------------------------
def _pad(atoms, dtype):
    """The hooks' 12 coordinates.  The caller keeps the array in a name of its own for as long as the hook reads it."""
    a = np.zeros(12, dtype)
    a[:atoms.size] = atoms.reshape(-1)
    return a


def _hook_feature(kind, uav, atoms):
    a, out = _pad(atoms, np.float32), np.zeros(3, np.float32)
    w = _capi.lib().molann_selftest_feature(kind, int(uav), _ptr(a), _ptr(out))
    return out[:w].astype(np.float64)


def _hook_backward(kind, uav, atoms, g):
    """[n_atoms, 3]: eval_item_backward under the cotangent g [w]."""
    g3 = np.zeros(3, np.float32)
    g3[:len(g)] = g
    a, ga = _pad(atoms, np.float32), np.zeros(12, np.float32)
    assert _capi.lib().molann_selftest_feature_backward(kind, int(uav), _ptr(a), _ptr(g3), _ptr(ga)) == 0
    return ga.reshape(4, 3)[:len(atoms)].astype(np.float64)


def _hook_tangent(kind, uav, atoms, t, dtype):
    fn = _capi.lib().molann_selftest_feature_tangent_f32 if dtype == np.float32 else _capi.lib().molann_selftest_feature_tangent_f64
    a, tt, out, dout = _pad(atoms, dtype), _pad(t, dtype), np.zeros(3, dtype), np.zeros(3, dtype)
    w = fn(kind, int(uav), _ptr(a), _ptr(tt), _ptr(out), _ptr(dout))
    assert w > 0
    return out[:w].astype(np.float64), dout[:w].astype(np.float64)


def _hook_jacobian_f64(kind, uav, atoms):
    a, jac = _pad(atoms, np.float64), np.zeros(36)
    w = _capi.lib().molann_selftest_item_jacobian_f64(kind, int(uav), _ptr(a), _ptr(jac))
    assert w > 0
    return jac.reshape(3, 4, 3)[:w, :len(atoms)]


def _hook_gen_f64(kind, uav, atoms, g):
    """[n_atoms, 3]: the gradient eval_item_backward_gen<Dual> carries as its value part, under the cotangent g."""
    g3 = np.zeros(3)
    g3[:len(g)] = g
    a, t, dg, ga, dga = _pad(atoms, np.float64), np.zeros(12), np.zeros(3), np.zeros(12), np.zeros(12)
    k = _capi.lib().molann_selftest_feature_backward_tangent_f64(kind, int(uav), _ptr(a), _ptr(t), _ptr(g3), _ptr(dg), _ptr(ga), _ptr(dga))
    assert k == len(atoms)
    return ga.reshape(4, 3)[:len(atoms)]


def _oracle(kind, uav, atoms, dtype):
    """(values [n, w], jacobian [n, w, n_atoms, 3]) of the oracle and its autograd in dtype on the item's atoms [n, k, 3]."""
    x = torch.from_numpy(atoms).to(dtype).requires_grad_(True)
    y = mo.feature_forward(x, kind, list(range(atoms.shape[1])), uav)
    jac = []
    for c in range(y.shape[1]):
        (g,) = torch.autograd.grad(y[:, c].sum(), x, retain_graph=True)
        jac.append(g)
    return y.detach().double().numpy(), torch.stack(jac, 1).double().numpy()


def _wrap(d, periodic):
    return np.abs(d - TWO_PI * np.round(d / TWO_PI)) if periodic else np.abs(d)


# ---- graded frames ---------------------------------------------------------------------------------------------------------
def _case(regime, delta):
    """(the edge item's type, its atoms [N, k, 3] float32, the item's sines [N]) at one regime and delta."""
    x, s = ae.draw(regime, delta, wl.ALA_DIPEPTIDE_XYZ, ITEMS, N, seed=17)
    i = ae.roles(ITEMS)[ae.ROLE_OF[regime]]
    kind, idx = ITEMS[i]
    return kind, np.ascontiguousarray(x[:, idx]), s[:, i]


@pytest.mark.parametrize("uav", [False, True], ids=["cos", "value"])
@pytest.mark.parametrize("regime", ae.REGIMES)
def test_graded_frames(regime, uav):
    rng = np.random.default_rng(5)
    worst = {}
    for delta in ae.grades(regime)[0]:
        kind, atoms, sin = _case(regime, delta)
        periodic = uav and kind == ae.DIH
        k = atoms.shape[1]
        ref = [_reference(kind, uav, a) for a in atoms]
        want_v = np.array([r[0] for r in ref])
        want_j = np.array([r[1] for r in ref])                     # [N, w, k, 3]
        w = want_v.shape[1]
        G = rng.uniform(-1.0, 1.0, (N, w)).astype(np.float32)
        T = rng.uniform(-1.0, 1.0, (N, k, 3)).astype(np.float32)
        want_g = np.einsum("nw,nwkc->nkc", G.astype(np.float64), want_j)
        want_t = np.einsum("nwkc,nkc->nw", want_j, T.astype(np.float64))
        s32 = np.maximum(1.0, np.abs(want_j).max((1, 2, 3)))       # float32: max(1, the frame's largest gradient entry)
        s64 = np.abs(want_j).max((1, 2, 3))
        # a tangent is a sum of 3 k products: its scale is the sum of their sizes
        t64 = np.einsum("nwkc,nkc->nw", np.abs(want_j), np.abs(T.astype(np.float64))).max(1)
        t32 = np.maximum(1.0, t64)
        v64 = np.maximum(np.abs(want_v).max(1), 1.0)               # values: an angle near 0 carries the absolute rounding of its S, C
        bound64 = 16.0 * EPS64 / sin ** 2
        # the oracle: float64 within the float64 bound (the GPU tests' reference), float32 for its own error
        o_v, o_j = _oracle(kind, uav, atoms, torch.float64)
        assert (_wrap(o_v - want_v, periodic).max(1) / v64 <= bound64).all(), (regime, delta, "oracle float64 values")
        assert (np.abs(o_j - want_j).max((1, 2, 3)) / s64 <= bound64).all(), (regime, delta, "oracle float64 gradients")
        p_v, p_j = _oracle(kind, uav, atoms, torch.float32)
        assert np.isfinite(p_v).all() and np.isfinite(p_j).all(), (regime, delta, "the float32 oracle is not finite")
        own_v = float(_wrap(p_v - want_v, periodic).max())
        own_g = float((np.abs(np.einsum("nw,nwkc->nkc", G.astype(np.float64), p_j) - want_g).max((1, 2)) / s32).max())
        own_t = float((np.abs(np.einsum("nwkc,nkc->nw", p_j, T.astype(np.float64)) - want_t).max(1) / t32).max())
        tol_v, tol_g, tol_t = max(2e-6, 2.0 * own_v), max(2e-5, 2.0 * own_g), max(2e-5, 2.0 * own_t)
        e = dict.fromkeys(("f32 value", "f32 backward", "f32 tangent", "f32 tangent value", "f64 tangent", "f64 tangent value",
                           "f64 jacobian", "f64 gen"), 0.0)
        for i in range(N):
            a = atoms[i]
            e["f32 value"] = max(e["f32 value"], _wrap(_hook_feature(kind, uav, a) - want_v[i], periodic).max() / tol_v)
            e["f32 backward"] = max(e["f32 backward"], np.abs(_hook_backward(kind, uav, a, G[i]) - want_g[i]).max() / s32[i] / tol_g)
            v, dv = _hook_tangent(kind, uav, a, T[i], np.float32)
            e["f32 tangent value"] = max(e["f32 tangent value"], _wrap(v - want_v[i], periodic).max() / tol_v)
            e["f32 tangent"] = max(e["f32 tangent"], np.abs(dv - want_t[i]).max() / t32[i] / tol_t)
            v, dv = _hook_tangent(kind, uav, a, T[i], np.float64)
            e["f64 tangent value"] = max(e["f64 tangent value"], _wrap(v - want_v[i], periodic).max() / v64[i] / bound64[i])
            e["f64 tangent"] = max(e["f64 tangent"], np.abs(dv - want_t[i]).max() / t64[i] / bound64[i])
            e["f64 jacobian"] = max(e["f64 jacobian"], np.abs(_hook_jacobian_f64(kind, uav, a) - want_j[i]).max() / s64[i] / bound64[i])
            e["f64 gen"] = max(e["f64 gen"], np.abs(_hook_gen_f64(kind, uav, a, G[i].astype(np.float64)) - want_g[i]).max()
                               / s64[i] / bound64[i])
        worst[delta] = e
        print("angular edges host %s %s delta=%g own(v,g,t)=%.2g %.2g %.2g  error/bound: %s" % (
            regime, "value" if uav else "cos", delta, own_v, own_g, own_t, " ".join("%s=%.2g" % kv for kv in e.items())))
    bad = [(d, k, v) for d, e in worst.items() for k, v in e.items() if not v <= 1.0]
    assert not bad, (regime, uav, bad)


# ---- pole frames -----------------------------------------------------------------------------------------------------------
def _row_ok(row, limit):
    """An end atom's gradient row: non-finite, or no longer than the limit."""
    return (not np.isfinite(row).all()) or float(np.linalg.norm(row)) <= limit


@pytest.mark.parametrize("regime", ["straight", "folded"])
@pytest.mark.parametrize("delta", ae.POLE + (1e-3,))
def test_pole_frames_angle_value_gradient_is_bounded_or_not_finite(regime, delta):
    """|d theta / d x_end| = 1 / |arm| exactly, at any angle.  Every variant gives a row that is not finite or within
    (1 + 1e-3) of that; with a tangent on the end atom alone, |d theta| <= (1 + 1e-3) |t| / |arm|."""
    kind, atoms, _ = _case(regime, delta)
    rng = np.random.default_rng(11)
    bad = []
    for i in range(N):
        a = atoms[i]
        arm = float(np.linalg.norm(a[2].astype(np.float64) - a[1].astype(np.float64)))
        lim = (1.0 + 1e-3) / arm
        rows = {"f32 backward": _hook_backward(kind, True, a, [1.0])[2], "f64 jacobian": _hook_jacobian_f64(kind, True, a)[0, 2],
                "f64 gen": _hook_gen_f64(kind, True, a, [1.0])[2]}
        t = np.zeros((3, 3), np.float32)
        t[2] = rng.uniform(-1.0, 1.0, 3)
        tn = float(np.linalg.norm(t[2].astype(np.float64)))
        for name, dt in (("f32 tangent", np.float32), ("f64 tangent", np.float64)):
            _, dv = _hook_tangent(kind, True, a, t, dt)
            if np.isfinite(dv[0]) and abs(dv[0]) > lim * tn:
                bad.append((i, name, float(dv[0]), lim * tn))
        bad += [(i, name, row.tolist(), lim) for name, row in rows.items() if not _row_ok(row, lim)]
    assert not bad, (regime, delta, bad[:6])


def test_helper_builds_what_it_says():
    """The constructed internal coordinates, measured in float64 on the float32 frames: within the rounding of the coordinates
    (1e-5 rad) of the prescribed ones; trans / cis signs alternate; the other items stay generic."""
    xyz = wl.ALA_DIPEPTIDE_XYZ
    ae.check_ownership(ITEMS, [])
    for regime in ae.REGIMES:
        for delta in (10.0, 0.1, 0.0):
            x, s = ae.draw(regime, delta, xyz, ITEMS, 16, seed=3)
            assert x.dtype == np.float32 and x.shape == (16, len(xyz), 3) and s.shape == (16, len(ITEMS))
            X = x.astype(np.float64)
            d = math.radians(delta)
            ang = ae._angle(X[:, 1], X[:, 4], X[:, 5])
            tc = ae.dihedral(X[:, 4], X[:, 6], X[:, 8], X[:, 14])
            arm = ae._angle(X[:, 12], X[:, 10], X[:, 8])
            if regime in ("straight", "folded"):
                assert np.abs(ang - (math.pi - d if regime == "straight" else d)).max() < 1e-5
            elif regime in ("trans", "cis"):
                want = math.pi - d if regime == "trans" else d
                assert np.abs(np.abs(tc) - want).max() < 1e-5
                if delta > 0:
                    assert (np.sign(tc) == np.where(np.arange(16) % 2 == 0, 1.0, -1.0)).all()
            else:
                assert np.abs(arm - (math.pi - d)).max() < 1e-5
            others = [c for c, r in enumerate(("angle", "tc", "arm")) if r != ae.ROLE_OF[regime]]
            assert (s[:, others] > 0.05).all() and (s[:, 3] == 1.0).all()
    x, lab, s = ae.interleaved("straight", (10.0, 0.0), xyz, ITEMS, 12, seed=3)
    assert lab == [None, 10.0, None, 0.0, None, 10.0, None, 0.0, None, 10.0, None, 0.0]
    assert np.array_equal(x[0::2], ae.near(xyz, 12, 3)[0::2])
