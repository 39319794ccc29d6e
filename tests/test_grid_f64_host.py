"""The tabulated bias of the float64 one-launch family on the host (no GPU): one axis' step and one frame's interpolation
(molann_selftest_grid_axis_f64 / molann_selftest_grid_f64 call the kernel's own __host__ __device__ functions) against the formula
written in torch float64, its exact cases and analytic properties, the safety of every index for every bit pattern of y, the table
helper of molann_amd.bias against the hills' selftest, the refusals of MolANN.value_and_grid / PreprocessingANN.value_and_grid that
need no device, the argument checks both share and the C entry's symbols and its answer to a null plan.

The formula (cubic convolution, Catmull-Rom) per axis, u = (y - lower) / h: periodic: u <- u - n floor(u / n), i = min(floor(u),
n - 1), idx_j = (i - 1 + j) mod n, s = 1; not periodic: s = 1 if 0 <= u <= n - 1 else 0 and u clamped to that range, i = min(floor(u),
n - 2), idx_j = clamp(i - 1 + j, 0, n - 1); t = u - i; a_j = w_j(t), b_j = s w'_j(t) / h; V = sum_j T[idx] prod_k a_k, dV/dy_k the same
with b_k in place of a_k."""

import ctypes
import itertools
import math
import os

import numpy as np
import pytest
import torch

from molann_amd import _capi, ann, bias, workloads as wl
from molann_amd.ann import MolANN, PreprocessingANN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["molann_value_and_grid_f64", "molann_plan_supports_value_and_grid_f64", "molann_selftest_grid_axis_f64", "molann_selftest_grid_f64"]
NAN, INF = float("nan"), float("inf")
F64 = torch.float64
TWO_PI = 2.0 * math.pi


def t64(*v):
    return torch.tensor(v, dtype=F64)


def weights(t):
    """(w [4], w' [4]) of the issue's formula for a 0-d float64 tensor t"""
    t2 = t * t
    w = torch.stack([((-t + 2) * t - 1) * t / 2, ((3 * t - 5) * t2 + 2) / 2, ((-3 * t + 4) * t + 1) * t / 2, (t - 1) * t2 / 2])
    dw = torch.stack([(-3 * t2 + 4 * t - 1) / 2, (9 * t2 - 10 * t) / 2, (-9 * t2 + 8 * t + 1) / 2, (3 * t2 - 2 * t) / 2])
    return w, dw


def axis_formula(y, n, lower, h, periodic):
    """(idx [4] ints, a [4], b [4]) of the issue's axis step, in torch float64 (y, lower, h: 0-d tensors)"""
    u = (y - lower) / h
    if periodic:
        u = u - n * torch.floor(u / n)
        i = torch.clamp(torch.floor(u), max=n - 1)
        s = 1.0
    else:
        s = 1.0 if bool((u >= 0) & (u <= n - 1)) else 0.0
        u = torch.clamp(u, 0, n - 1)
        i = torch.clamp(torch.floor(u), max=n - 2)
    t = u - i
    i = int(i)
    idx = [(i - 1 + j) % n if periodic else min(max(i - 1 + j, 0), n - 1) for j in range(4)]
    w, dw = weights(t)
    return idx, w, s * dw / h


def formula(y, table, lower, spacing, periodic):
    """(V, dV/dy [d], sum_p |T_p prod a|, [sum_p |T_p b_k prod_{m != k} a_m|]) of the issue's formula in torch float64"""
    d = table.dim()
    steps = [axis_formula(y[k], table.shape[k], lower[k], spacing[k], periodic[k]) for k in range(d)]
    sub = table[np.ix_(*[s[0] for s in steps])]
    letters = "ijl"[:d]
    eq = letters + "," + ",".join(letters) + "->"
    a, b = [s[1] for s in steps], [s[2] for s in steps]
    mixed = lambda k: [b[m] if m == k else a[m] for m in range(d)]       # noqa: E731
    v = torch.einsum(eq, sub, *a)
    dv = torch.stack([torch.einsum(eq, sub, *mixed(k)) for k in range(d)])
    v_scale = torch.einsum(eq, sub.abs(), *[t.abs() for t in a])
    dv_scale = torch.stack([torch.einsum(eq, sub.abs(), *[t.abs() for t in mixed(k)]) for k in range(d)])
    return v, dv, v_scale, dv_scale


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _grid(table, lower, spacing, periodic):
    d = table.dim()
    return ((ctypes.c_int64 * d)(*table.shape), (ctypes.c_double * d)(*[float(v) for v in lower]), (ctypes.c_double * d)(*[float(v) for v in spacing]),
            None if periodic is None else (ctypes.c_int32 * d)(*[1 if p else 0 for p in periodic]))


def selftest(y, table, lower, spacing, periodic):
    d = table.dim()
    dy = torch.full((d,), 7.5, dtype=F64)
    y = torch.as_tensor(y, dtype=F64).reshape(-1).contiguous()
    v = _capi.lib().molann_selftest_grid_f64(_ptr(y), d, _ptr(table), *_grid(table, lower, spacing, periodic), _ptr(dy))
    return v, dy


def axis_selftest(y, n, lower, h, periodic):
    idx, w, dw = torch.full((4,), -99, dtype=torch.int64), torch.full((4,), 7.5, dtype=F64), torch.full((4,), 7.5, dtype=F64)
    _capi.lib().molann_selftest_grid_axis_f64(float(y), n, float(lower), float(h), 1 if periodic else 0, _ptr(idx), _ptr(w), _ptr(dw))
    return idx.tolist(), w, dw


def _draws(count=2400):
    """Seeded (y, table, lower, spacing, periodic): d = 1..3, 4..9 points per axis, every mix of periodic flags in turn; per axis y
    is, in turn, inside the range, in the first cell, in the last cell (the seam cell of a periodic axis), below the range, above it,
    and up to 10 periods away on either side."""
    g = torch.Generator().manual_seed(57)
    rand = lambda *shape: torch.rand(shape, generator=g, dtype=F64)       # noqa: E731
    mixes = {d: list(itertools.product((False, True), repeat=d)) for d in (1, 2, 3)}
    draws = []
    for i in range(count):
        d = 1 + i % 3
        periodic = mixes[d][(i // 3) % len(mixes[d])]
        shape = [int(n) for n in torch.randint(4, 10, (d,), generator=g)]
        table = 2.0 * torch.randn(shape, generator=g, dtype=F64)
        lower, spacing = 4.0 * rand(d) - 2.0, 0.05 + 1.5 * rand(d)
        y = torch.empty(d, dtype=F64)
        for k in range(d):
            n, lo, h = shape[k], float(lower[k]), float(spacing[k])
            span = (n if periodic[k] else n - 1) * h
            r = float(rand(1))
            where = (i // 7 + 3 * k) % 7
            if where == 0:
                y[k] = lo + r * span
            elif where == 1:
                y[k] = lo + r * h
            elif where == 2:
                y[k] = lo + span - r * h
            elif where == 3:
                y[k] = lo - (0.01 + 3.0 * r) * h
            elif where == 4:
                y[k] = lo + span + (0.01 + 3.0 * r) * h
            else:
                y[k] = lo + r * span + (1 + int(9 * float(rand(1)))) * span * (1 if where == 5 else -1)
        draws.append((y, table, lower, spacing, periodic))
    return draws


def test_selftest_against_the_formula():
    worst_v = worst_dy = 0.0
    draws = _draws()
    assert len(draws) >= 2000
    for y, table, lower, spacing, periodic in draws:
        v, dy = selftest(y, table, lower, spacing, periodic)
        v_want, dy_want, v_scale, dy_scale = formula(y, table, lower, spacing, periodic)
        v_ratio = abs(v - float(v_want)) / (1e-12 * max(1.0, float(v_scale)))
        dy_ratio = float(((dy - dy_want).abs() / (1e-12 * dy_scale.clamp(min=1.0))).max())
        worst_v, worst_dy = max(worst_v, v_ratio), max(worst_dy, dy_ratio)
    print("worst error / bound: V %.3g, dy %.3g" % (worst_v, worst_dy))
    assert worst_v <= 1.0 and worst_dy <= 1.0, (worst_v, worst_dy)


def test_axis_step_against_the_formula():
    """indices equal; weights to a few ulp (the same operations in the same order, up to s / h formed first)"""
    for y, table, lower, spacing, periodic in _draws(600):
        for k in range(table.dim()):
            idx, w, dw = axis_selftest(y[k], table.shape[k], lower[k], spacing[k], periodic[k])
            idx_want, w_want, dw_want = axis_formula(y[k], table.shape[k], lower[k], spacing[k], periodic[k])
            assert idx == idx_want, (float(y[k]), idx, idx_want)
            assert torch.equal(w, w_want), (w, w_want)
            assert float((dw - dw_want).abs().max()) <= 4e-16 * max(1.0, float(dw_want.abs().max()))


def test_exact_cases():
    """lower = 0, spacing = 1: u = y exactly"""
    g = torch.Generator().manual_seed(5)
    for shape, periodic in (((7,), (False,)), ((7,), (True,)), ((5, 6), (False, True)), ((6, 4, 5), (True, False, False)), ((4, 4, 4), (True, True, True))):
        d = len(shape)
        table = torch.randn(shape, generator=g, dtype=F64)
        lower, spacing = [0.0] * d, [1.0] * d
        for point in itertools.product(*[range(n) for n in shape]):
            v, dy = selftest([float(i) for i in point], table, lower, spacing, periodic)
            assert v == float(table[point]), (shape, point)                         # the table's entry, bit for bit
            for k in range(d):
                n, i = shape[k], point[k]
                if periodic[k] or 1 <= i <= n - 2:                                   # an interior point: the centred difference, bit for bit
                    up, down = list(point), list(point)
                    up[k], down[k] = (i + 1) % n, (i - 1) % n
                    assert float(dy[k]) == float((table[tuple(up)] - table[tuple(down)]) / 2), (shape, point, k)
        # outside a non-periodic range: the value at the clamped point, that axis' derivative exactly 0
        for k in range(d):
            if periodic[k]:
                continue
            for out, edge in ((-0.75, 0.0), (-1e6, 0.0), (shape[k] - 1 + 0.3, shape[k] - 1.0), (1e9, shape[k] - 1.0)):
                y = [1.25] * d
                y[k] = out
                v, dy = selftest(y, table, lower, spacing, periodic)
                y[k] = edge
                v_edge, dy_edge = selftest(y, table, lower, spacing, periodic)
                assert v == v_edge and float(dy[k]) == 0.0, (shape, k, out)
                others = [m for m in range(d) if m != k]
                assert torch.equal(dy[others], dy_edge[others])


def test_constant_table():
    g = torch.Generator().manual_seed(6)
    for y, table, lower, spacing, periodic in _draws(300):
        c = float(3.0 * torch.randn(1, generator=g, dtype=F64))
        v, dy = selftest(y, torch.full_like(table, c), lower, spacing, periodic)
        assert abs(v - c) <= 4 * np.spacing(abs(c)), (v, c)
        assert bool((dy.abs() <= 1e-15 * abs(c) / spacing).all()), (dy, c, spacing)


def test_products_of_quadratics_are_reproduced():
    """T = prod_k (p_k + q_k y_k + r_k y_k^2) at the grid points: V and the analytic gradient to 1e-12 of their scale in cells whose
    stencil is not clamped (cells 1 .. n - 3 of a non-periodic axis; not periodic: a quadratic is not)."""
    g = torch.Generator().manual_seed(7)
    rand = lambda *shape: torch.rand(shape, generator=g, dtype=F64)       # noqa: E731
    worst = 0.0
    for trial in range(300):
        d = 1 + trial % 3
        shape = [int(n) for n in torch.randint(4, 10, (d,), generator=g)]
        lower, spacing = 4.0 * rand(d) - 2.0, 0.05 + 1.5 * rand(d)
        coef = torch.randn((d, 3), generator=g, dtype=F64)
        poly = lambda k, z: coef[k, 0] + coef[k, 1] * z + coef[k, 2] * z * z       # noqa: E731
        dpoly = lambda k, z: coef[k, 1] + 2.0 * coef[k, 2] * z                     # noqa: E731
        pts = bias.grid_points(shape, lower, spacing)
        table = torch.ones(shape, dtype=F64)
        for k in range(d):
            table = table * poly(k, pts[k]).reshape([-1 if m == k else 1 for m in range(d)])
        y = torch.stack([lower[k] + (1.0 + (shape[k] - 3) * rand(1)[0]) * spacing[k] for k in range(d)])
        v, dy = selftest(y, table.contiguous(), lower, spacing, [False] * d)
        vals = [poly(k, y[k]) for k in range(d)]
        v_want = math.prod(float(t) for t in vals)
        scale = float(table.abs().max())
        assert abs(v - v_want) <= 1e-12 * max(1.0, scale), (trial, v, v_want)
        worst = max(worst, abs(v - v_want) / max(1.0, scale))
        for k in range(d):
            want = float(dpoly(k, y[k])) * math.prod(float(vals[m]) for m in range(d) if m != k)
            assert abs(float(dy[k]) - want) <= 1e-12 * max(1.0, scale / float(spacing[k])), (trial, k, float(dy[k]), want)
    print("worst value error / scale: %.3g" % worst)


def test_shifting_lower_by_whole_periods():
    worst = 0.0
    for y, table, lower, spacing, periodic in _draws(420):
        if not any(periodic):
            continue
        v, _ = selftest(y, table, lower, spacing, periodic)
        for m in (-5, -2, 1, 3, 5):
            shifted = torch.stack([lower[k] + (m * table.shape[k] * spacing[k] if periodic[k] else 0.0) for k in range(table.dim())])
            v2, _ = selftest(y, table, shifted, spacing, periodic)
            worst = max(worst, abs(v2 - v))
            assert abs(v2 - v) <= 1e-12, (m, v, v2)
    print("worst change of V under a shift of lower by whole periods: %.3g" % worst)


def test_every_index_is_in_range():
    tiny = 5e-324
    for n in (4, 5, 64):
        for periodic in (False, True):
            for lower, h in ((0.0, 1.0), (-1.7, 0.37), (2.5e3, 1e-3)):
                knots = [lower + i * h for i in range(-1, n + 2)]
                ys = [NAN, INF, -INF, 1e308, -1e308, tiny, -tiny, 2.2e-308, -2.2e-308, 0.0, -0.0, lower, lower + (n - 1) * h, lower + n * h]
                for z in knots:
                    ys += [z, float(np.nextafter(z, INF)), float(np.nextafter(z, -INF))]
                for y in ys:
                    idx, w, dw = axis_selftest(y, n, lower, h, periodic)
                    assert all(0 <= i <= n - 1 for i in idx), (y, n, periodic, idx)
                    if not math.isfinite(y):
                        assert bool(torch.isnan(w).all()) and bool(torch.isnan(dw).all()), (y, w, dw)
                    elif abs(y) < 1e300:
                        assert bool(torch.isfinite(w).all()) and bool(torch.isfinite(dw).all()) and abs(float(w.sum()) - 1.0) <= 1e-12, (y, w)
    table = torch.arange(4.0 * 5.0, dtype=F64).reshape(4, 5)
    for bad in (NAN, INF, -INF):
        for k in (0, 1):
            y = [1.5, 1.5]
            y[k] = bad
            v, dy = selftest(y, table, [0.0, 0.0], [1.0, 1.0], [True, False])
            assert math.isnan(v) and bool(torch.isnan(dy).all())
    # bad arguments: NaN, dy untouched
    L = _capi.lib()
    y, dy = t64(1.5, 1.5), torch.full((2,), 7.5, dtype=F64)
    for tab, lo, sp in ((table, [0.0, 0.0], [1.0, 0.0]), (table, [0.0, 0.0], [1.0, -1.0]), (table, [0.0, 0.0], [NAN, 1.0]), (table, [0.0, 0.0], [INF, 1.0]),
                        (table, [0.0, INF], [1.0, 1.0]), (table[:3].contiguous(), [0.0, 0.0], [1.0, 1.0])):
        assert math.isnan(L.molann_selftest_grid_f64(_ptr(y), 2, _ptr(tab), *_grid(tab, lo, sp, None), _ptr(dy))) and bool((dy == 7.5).all())
    shape, lo, sp, _ = _grid(table, [0.0, 0.0], [1.0, 1.0], None)
    assert math.isnan(L.molann_selftest_grid_f64(_ptr(y), 4, _ptr(table), shape, lo, sp, None, _ptr(dy))) and bool((dy == 7.5).all())
    assert math.isnan(L.molann_selftest_grid_f64(_ptr(y), 0, _ptr(table), shape, lo, sp, None, _ptr(dy)))
    assert math.isnan(L.molann_selftest_grid_f64(None, 2, _ptr(table), shape, lo, sp, None, _ptr(dy)))
    assert math.isnan(L.molann_selftest_grid_f64(_ptr(y), 2, None, shape, lo, sp, None, _ptr(dy))) and bool((dy == 7.5).all())
    assert L.molann_selftest_grid_f64(_ptr(y), 2, _ptr(table), shape, lo, sp, None, None) == selftest(y, table, [0.0, 0.0], [1.0, 1.0], None)[0]


def test_hills_on_a_table_converge_to_the_hill_sum():
    """30 hills in 2-D (axis 0 periodic with period 2 pi, axis 1 on [-0.5, 2.5], sigma = (0.35, 0.25)) put on tables of
    32 m x (24 m + 1) points by add_hills_to_grid, m = 1, 2, 4, and interpolated at 300 seeded points (axis 1 within [-0.3, 2.3])
    against molann_selftest_hills_f64: the worst value error falls by >= 6 per halving of the spacing (theory h^3: 8), the worst
    derivative error by >= 3 (theory h^2: 4)."""
    g = torch.Generator().manual_seed(11)
    rand = lambda *shape: torch.rand(shape, generator=g, dtype=F64)       # noqa: E731
    H = 30
    centers = torch.stack([-math.pi + TWO_PI * rand(H), 2.0 * rand(H)], dim=1).contiguous()
    heights = 0.2 + rand(H)
    heights[H // 2] = -heights[H // 2]
    sigma, period = t64(0.35, 0.25), t64(TWO_PI, 0.0)
    points = torch.stack([-3.0 * math.pi + 6.0 * math.pi * rand(300), -0.3 + 2.6 * rand(300)], dim=1).contiguous()
    L = _capi.lib()
    errors = []
    for m in (1, 2, 4):
        shape = (32 * m, 24 * m + 1)
        lower, spacing, periodic = [-math.pi, -0.5], [TWO_PI / shape[0], 3.0 / (shape[1] - 1)], [True, False]
        table = bias.add_hills_to_grid(torch.zeros(shape, dtype=F64), lower, spacing, periodic, centers, heights, sigma, chunk=7)
        # the table holds the hill sum at its points
        for i, j in ((0, 0), (5, 7), (shape[0] - 1, shape[1] - 1)):
            node = t64(lower[0] + i * spacing[0], lower[1] + j * spacing[1])
            want = L.molann_selftest_hills_f64(_ptr(node), 2, _ptr(centers), _ptr(heights), H, _ptr(sigma), 0, _ptr(period), None)
            assert abs(float(table[i, j]) - want) <= 1e-13 * max(1.0, abs(want))
        ev = ed = 0.0
        for y in points:
            dy_want = torch.zeros(2, dtype=F64)
            v_want = L.molann_selftest_hills_f64(_ptr(y), 2, _ptr(centers), _ptr(heights), H, _ptr(sigma), 0, _ptr(period), _ptr(dy_want))
            v, dy = selftest(y, table, lower, spacing, periodic)
            ev, ed = max(ev, abs(v - v_want)), max(ed, float((dy - dy_want).abs().max()))
        errors.append((ev, ed))
        print("h = sigma / %.1f, sigma / %.1f: worst value error %.3e, worst derivative error %.3e" % (0.35 / spacing[0], 0.25 / spacing[1], ev, ed))
    for (ev0, ed0), (ev1, ed1) in zip(errors, errors[1:]):
        print("per halving: value %.2f x, derivative %.2f x" % (ev0 / ev1, ed0 / ed1))
        assert ev0 >= 6.0 * ev1 and ed0 >= 3.0 * ed1, errors


def test_table_helper():
    pts = bias.grid_points((4, 5), [0.5, -1.0], [0.25, 2.0])
    assert torch.equal(pts[0], t64(0.5, 0.75, 1.0, 1.25)) and torch.equal(pts[1], t64(-1.0, 1.0, 3.0, 5.0, 7.0))
    with pytest.raises(ValueError):
        bias.grid_points((4, 5), [0.5], [0.25, 2.0])
    # in place, additive, chunks do not matter beyond rounding; one hill on a periodic axis reaches across the seam
    table = torch.ones((8,), dtype=F64)
    out = bias.add_hills_to_grid(table, [0.0], [0.5], [True], [[3.9]], 2.0, 0.3)
    assert out is table
    want = 1.0 + 2.0 * torch.exp(-0.5 * ((t64(0.1, 0.6, 1.1, 1.6, -1.9, -1.4, -0.9, -0.4)) / 0.3) ** 2)
    assert float((table - want).abs().max()) <= 1e-14
    g = torch.Generator().manual_seed(3)
    c, w, s = torch.randn((50, 3), generator=g, dtype=F64), torch.randn(50, generator=g, dtype=F64), 0.3 + torch.rand((50, 3), generator=g, dtype=F64)
    a = bias.add_hills_to_grid(torch.zeros((5, 6, 7), dtype=F64), [-1.0] * 3, [0.4] * 3, [True, False, True], c, w, s, chunk=1000)
    b = bias.add_hills_to_grid(torch.zeros((5, 6, 7), dtype=F64), [-1.0] * 3, [0.4] * 3, [True, False, True], c, w, s, chunk=3)
    assert float((a - b).abs().max()) <= 1e-13 and float(a.abs().max()) > 0.1
    with pytest.raises(ValueError):
        bias.add_hills_to_grid(torch.zeros((5, 6), dtype=F64), [0.0, 0.0], [1.0, 1.0], None, [[0.0, 0.0]], 1.0, [0.5, 0.0])
    with pytest.raises(TypeError):
        bias.add_hills_to_grid(torch.zeros((5, 6)), [0.0, 0.0], [1.0, 1.0], None, [[0.0, 0.0]], 1.0, 0.5)


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_declared_exported_and_bound(name):
    header = open(os.path.join(ROOT, "include", "molann_hip.h")).read()
    assert name + "(" in header, name
    fn = getattr(_capi.lib(), name)
    assert fn.argtypes is not None and len(fn.argtypes) == {SYMBOLS[0]: 14, SYMBOLS[1]: 1, SYMBOLS[2]: 8, SYMBOLS[3]: 8}[name], name
    assert name in _capi.declared_symbols()


def test_null_plan():
    L = _capi.lib()
    assert L.molann_plan_supports_value_and_grid_f64(None) == _capi.E_NULL
    for n in (1, 0):
        assert L.molann_value_and_grid_f64(None, None, n, None, None, None, None, None, None, None, None, None, None, None) == _capi.E_NULL
    assert _capi.lib().molann_abi_version() == 1


def test_methods_exist_and_say_what_is_out_of_scope():
    assert callable(_capi.Plan.supports_value_and_grid_f64) and callable(_capi.Plan.value_and_grid_f64)
    doc = " ".join(MolANN.value_and_grid.__doc__.split())
    for words in ("float32", "GraphedForces", "No autograd graph is recorded", "at most 3 outputs", "JUMPS at the range's ends", "stored derivatives"):
        assert words in doc, (words, doc)
    assert "No autograd graph is recorded" in " ".join(PreprocessingANN.value_and_grid.__doc__.split())


def test_cpu_tensor_names_the_route_that_remains():
    w = wl.get_workload("C3")
    torch.manual_seed(0)
    base = wl.build_model(w, torch.device("cpu"), 0)
    model = MolANN(base.preprocessing_layer, ann.create_sequential_nn([w.feature_dim(), 5, 2], torch.nn.Tanh())).double().requires_grad_(False)
    x = w.make_frames(3, seed=1).double()
    table = torch.zeros((5, 6), dtype=F64)
    with pytest.raises(NotImplementedError, match=r"use `model\(x\)`, interpolate the table and its derivative with torch, then `value_and_vjp`"):
        model.value_and_grid(x, table, [0.0, 0.0], [1.0, 1.0])
    with pytest.raises(NotImplementedError, match=r"value_and_grid needs a FeatureLayer .* take torch\.autograd\.grad"):
        model.preprocessing_layer.value_and_grid(x, table, [0.0, 0.0], [1.0, 1.0])
    with pytest.raises(NotImplementedError):                            # the gate comes before `into` and before the other arguments
        model.value_and_grid(x, table[:3], [0.0], [-1.0, 1.0], into=(table, table))


def test_float32_x_is_refused_with_the_route():
    x = torch.zeros((5, 22, 3), dtype=torch.float32)
    table = torch.zeros((5, 6), dtype=F64)
    with pytest.raises(TypeError, match=r"value_and_grid is float64: call \.double\(\) .* interpolate the table"):
        ann._one_launch_arguments(ann._GRID, x, (table, [0.0, 0.0], [1.0, 1.0], None), None, 22, 2, (), None)
    with pytest.raises(AssertionError, match="Input should be a 3d torch tensor"):      # x's shape comes first
        ann._one_launch_arguments(ann._GRID, x[:, :-1], (table, [0.0, 0.0], [1.0, 1.0], None), None, 22, 2, (), None)


def test_arguments_are_checked_before_any_device_call():
    """ann._check_grid_args is what both methods call before the plan is looked up; tensors on the meta device stand for 'another
    device' here."""
    n, n_inp, d = 5, 22, 2
    x = torch.zeros((n, n_inp, 3), dtype=F64)
    y, v, dx = torch.zeros((n, d), dtype=F64), torch.zeros(n, dtype=F64), torch.zeros_like(x)
    table = torch.linspace(-1.0, 1.0, 30, dtype=F64).reshape(5, 6)

    def check(table=table, lower=(0.0, -1.0), spacing=(0.5, 0.25), periodic=None, into=None, out_dim=d):
        return ann._check_grid_args("value_and_grid", x, out_dim, table, lower, spacing, periodic, into)

    got = check()
    assert got[0].data_ptr() == table.data_ptr() and got[1] == [0.0, -1.0] and got[2] == [0.5, 0.25] and got[3] == [False, False]
    assert got[4:] == (None, None, None)
    got = check(lower=t64(0.0, -1.0), spacing=torch.tensor([0.5, 0.25]), periodic=[1, 0], into=(y, v, dx))
    assert got[1] == [0.0, -1.0] and got[2] == [0.5, 0.25] and got[3] == [True, False] and got[4] is y and got[5] is v and got[6] is dx
    assert check(periodic=torch.tensor([False, True]))[3] == [False, True]
    assert check(table=table.reshape(30)[:6], lower=[0.0], spacing=[1.0], out_dim=1)[0].shape == (6,)
    for bad in (table.reshape(30), table.reshape(5, 3, 2), table[:3], table[:, :3], table.t(), table[:, ::1].t().contiguous().t(), table.to("meta"),
                torch.zeros((5, 6, 7), dtype=F64)):
        with pytest.raises(ValueError, match="table"):
            check(table=bad)
    for bad in (table.float(), table.to(torch.int64), table.tolist(), None):
        with pytest.raises(TypeError, match="table"):
            check(table=bad)
    for bad in (0.0, -0.5, NAN, INF):
        with pytest.raises(ValueError, match="spacing"):
            check(spacing=(0.5, bad))
    for bad in (NAN, INF, -INF):
        with pytest.raises(ValueError, match="lower"):
            check(lower=(bad, 0.0))
    for what in ("lower", "spacing", "periodic"):
        for bad in ((1.0,), (1.0, 1.0, 1.0), []):
            with pytest.raises(ValueError, match=what):
                check(**{what: bad})
    for what in ("lower", "spacing"):
        with pytest.raises(TypeError, match=what):
            check(**{what: 1.0})
        with pytest.raises(TypeError, match=what):
            check(**{what: ("a", "b")})
        with pytest.raises(ValueError, match=what):
            check(**{what: t64(1.0, 1.0).to("meta")})
    with pytest.raises(TypeError, match="periodic"):
        check(periodic=True)
    with pytest.raises(NotImplementedError, match=r"at most 3 outputs \(got 4\); use `model\(x\)`, interpolate the table"):
        check(table=torch.zeros((4, 4, 4, 4), dtype=F64), lower=[0.0] * 4, spacing=[1.0] * 4, out_dim=4)
    for bad in ((y, dx), (y, v, dx, dx), (y, v, None)):
        with pytest.raises(TypeError, match=r"triple of tensors \(y, bias, dx\)"):
            check(into=bad)
    for bad in ((y.float(), v, dx), (y, v.float(), dx), (y, v, dx.float())):
        with pytest.raises(TypeError, match="float64"):
            check(into=bad)
    for bad in ((y[:4], v, dx), (y, v[:4], dx), (y, v, dx[:, :-1]), (y.t(), v, dx), (y.to("meta"), v, dx)):
        with pytest.raises(ValueError, match="into"):
            check(into=bad)
    with pytest.raises(ValueError, match="spacing"):                                    # the grid is looked at before `into`
        check(spacing=(0.5, 0.0), into=(y.to("meta"), v, dx))
