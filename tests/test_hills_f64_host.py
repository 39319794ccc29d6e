"""The metadynamics hills of the float64 one-launch family on the host (no GPU): one frame's hill sum and its derivative
(molann_selftest_hills_f64 adds up the kernel's own __host__ __device__ function, hill by hill) against the formula written in torch
float64, the refusals of MolANN.value_and_hills / PreprocessingANN.value_and_hills that need no device, the argument checks both
share (run before anything touches a device) and the C entry's symbols and its answer to a null plan."""

import ctypes
import math
import os

import numpy as np
import pytest
import torch

from molann_amd import _capi, ann, workloads as wl
from molann_amd.ann import MolANN, PreprocessingANN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["molann_value_and_hills_f64", "molann_plan_supports_value_and_hills_f64", "molann_selftest_hills_f64"]
NAN = float("nan")


def formula(y, centers, heights, sigma, period):
    """(V, dV/dy, sum_h |g_h|, sum_h |g_h s_k / sigma_k|) of the issue's formula in torch float64: y [d], centers [H, d], heights [H],
    sigma [d] or [H, d], period [d] or None; d = y - c wrapped by d - P round(d / P) where P > 0 (torch.round: ties to even)."""
    d = y[None, :] - centers
    if period is not None:
        periodic = period > 0
        P = torch.where(periodic, period, torch.ones_like(period))
        d = torch.where(periodic[None, :], d - P * torch.round(d / P), d)
    s = d / sigma
    g = heights * torch.exp(-0.5 * (s * s).sum(1))
    terms = g[:, None] * s / sigma
    return g.sum(), -terms.sum(0), g.abs().sum(), terms.abs().sum(0)


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def selftest(y, centers, heights, sigma, period):
    d = y.numel()
    dy = torch.full((d,), 7.5, dtype=torch.float64)
    v = _capi.lib().molann_selftest_hills_f64(_ptr(y), d, _ptr(centers), _ptr(heights), heights.numel(), _ptr(sigma), d if sigma.dim() == 2 else 0,
                                              _ptr(period), _ptr(dy))
    return v, dy


def _draws():
    """3000 seeded (y, centers, heights, sigma, period): d in 1..8, H in 0..40, the widths shared or per hill, a third of the columns
    periodic on average (a third of the draws without a period row at all), heights of both signs with a few zeros."""
    g = torch.Generator().manual_seed(31)
    f64 = dict(generator=g, dtype=torch.float64)
    draws = []
    for i in range(3000):
        d, H = 1 + i % 8, int(torch.randint(0, 41, (1,), generator=g))
        y = 2.0 * torch.randn(d, **f64)
        centers = 2.0 * torch.randn(H, d, **f64)
        heights = 1.5 * torch.randn(H, **f64)
        heights[::5] = 0.0
        sigma = 0.2 + 1.5 * torch.rand((H, d) if i % 2 else (d,), **f64)
        period = None
        if i % 3:
            pick = torch.randint(0, 2, (d,), generator=g) == 0
            period = torch.where(pick, 1.0 + 5.0 * torch.rand(d, **f64), torch.zeros(d, dtype=torch.float64))
            if i % 7 == 0:
                period[0] = -1.0          # P <= 0: not periodic
        draws.append((y, centers, heights, sigma, period))
    return draws


def _within(v, dy, want):
    """the issue's bound: V within 1e-12 max(1, sum |g_h|), dy_k within 1e-12 max(1, sum_h |g_h s_k / sigma_k|); returns the worst ratios"""
    v_want, dy_want, v_scale, dy_scale = want
    v_ratio = abs(v - float(v_want)) / (1e-12 * max(1.0, float(v_scale)))
    dy_ratio = float(((dy - dy_want).abs() / (1e-12 * dy_scale.clamp(min=1.0))).max())
    return v_ratio, dy_ratio


def test_selftest_against_the_formula():
    worst_v = worst_dy = 0.0
    for y, centers, heights, sigma, period in _draws():
        v, dy = selftest(y, centers, heights, sigma, period)
        v_ratio, dy_ratio = _within(v, dy, formula(y, centers, heights, sigma, period))
        worst_v, worst_dy = max(worst_v, v_ratio), max(worst_dy, dy_ratio)
    print("worst error / bound: V %.3g, dy %.3g" % (worst_v, worst_dy))
    assert worst_v <= 1.0 and worst_dy <= 1.0, (worst_v, worst_dy)


def test_edge_cases():
    t = lambda *v: torch.tensor(v, dtype=torch.float64)
    one = t(1.0)
    # d / P exactly +-0.5, +-1.5 with P = 2: rint gives 0, 0, 2, -2 (ties to even), so d wraps to 1, -1, -1, 1; sigma 1, height 1
    for y0, d_want in ((1.0, 1.0), (-1.0, -1.0), (3.0, -1.0), (-3.0, 1.0)):
        v, dy = selftest(t(y0), t(0.0).reshape(1, 1), one, one, t(2.0))
        g = math.exp(-0.5)
        assert abs(v - g) <= 4e-16 and abs(float(dy[0]) + g * d_want) <= 4e-16, (y0, v, dy)
        assert _within(v, dy, formula(t(y0), t(0.0).reshape(1, 1), one, one, t(2.0))) <= (1.0, 1.0)
    # height 0 contributes nothing, exactly; a negative height gives a negative bias
    y, centers, sigma = t(0.3, -0.2), t(0.1, 0.1, -0.4, 0.3).reshape(2, 2), t(0.5, 0.7)
    v, dy = selftest(y, centers, t(0.0, 0.0), sigma, None)
    assert v == 0.0 and bool((dy == 0.0).all())
    v1, dy1 = selftest(y, centers[:1], t(-0.8), sigma, None)
    v2, dy2 = selftest(y, centers, t(-0.8, 0.0), sigma, None)
    assert v1 < 0.0 and v2 == v1 and torch.equal(dy1, dy2)
    assert _within(v1, dy1, formula(y, centers[:1], t(-0.8), sigma, None)) <= (1.0, 1.0)
    # a far hill: exp underflows to exactly 0 and leaves the near hill's bits alone (q = 1/2 (60 / 0.5)^2 = 7200)
    far = torch.cat([centers[:1], t(60.3, -0.2).reshape(1, 2)])
    v3, dy3 = selftest(y, far, t(-0.8, 1.0), sigma, None)
    assert v3 == v1 and torch.equal(dy3, dy1)
    v4, dy4 = selftest(y, far[1:], t(1.0), sigma, None)
    assert v4 == 0.0 and bool((dy4 == 0.0).all())
    # a NaN in y, and a NaN in one centre: a NaN bias and NaN in every column (q is shared by the columns)
    for yy, cc in ((t(NAN, -0.2), centers), (y, t(0.1, 0.1, NAN, 0.3).reshape(2, 2))):
        v, dy = selftest(yy, cc, t(1.0, 1.0), sigma, t(2.0, 0.0))
        assert math.isnan(v) and bool(torch.isnan(dy).all())
    # H = 0, with and without pointers to a table
    v, dy = selftest(y, centers[:0], t(), sigma, None)
    assert v == 0.0 and bool((dy == 0.0).all())
    dy = torch.full((2,), 7.5, dtype=torch.float64)
    assert _capi.lib().molann_selftest_hills_f64(_ptr(y), 2, None, None, 0, _ptr(sigma), 0, None, _ptr(dy)) == 0.0 and bool((dy == 0.0).all())
    # dy may be null; more than 8 columns: NaN, dy untouched
    assert _capi.lib().molann_selftest_hills_f64(_ptr(y), 2, _ptr(centers[:1]), _ptr(t(-0.8)), 1, _ptr(sigma), 0, None, None) == v1
    y9 = torch.zeros(9, dtype=torch.float64)
    dy = torch.full((9,), 7.5, dtype=torch.float64)
    assert math.isnan(_capi.lib().molann_selftest_hills_f64(_ptr(y9), 9, None, None, 0, _ptr(y9 + 1.0), 0, None, _ptr(dy))) and bool((dy == 7.5).all())


def test_shared_and_repeated_sigma_give_the_same_bits():
    for y, centers, heights, sigma, period in _draws()[:400:2]:      # the even draws have one sigma row
        v, dy = selftest(y, centers, heights, sigma, period)
        v2, dy2 = selftest(y, centers, heights, sigma.expand(centers.shape[0], -1).contiguous(), period)
        assert (v == v2 or (math.isnan(v) and math.isnan(v2))) and torch.equal(dy, dy2)


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_declared_exported_and_bound(name):
    header = open(os.path.join(ROOT, "include", "molann_hip.h")).read()
    assert name + "(" in header, name
    fn = getattr(_capi.lib(), name)
    assert fn.argtypes is not None and len(fn.argtypes) == {SYMBOLS[0]: 15, SYMBOLS[1]: 1, SYMBOLS[2]: 9}[name], name
    assert name in _capi.declared_symbols()


def test_null_plan():
    L = _capi.lib()
    assert L.molann_plan_supports_value_and_hills_f64(None) == _capi.E_NULL
    for n in (1, 0):
        for n_hills in (3, 0, -1):
            assert L.molann_value_and_hills_f64(None, None, n, None, None, None, None, n_hills, None, 0, None, None, None, None, None) == _capi.E_NULL
    assert _capi.lib().molann_abi_version() == 1


def test_methods_exist_and_say_what_is_out_of_scope():
    assert callable(_capi.Plan.supports_value_and_hills_f64) and callable(_capi.Plan.value_and_hills_f64)
    doc = " ".join(MolANN.value_and_hills.__doc__.split())
    for words in ("costs a launch", "float32", "GraphedForces", "No autograd graph is recorded", "at most 8 outputs", "cutoff"):
        assert words in doc, (words, doc)
    assert "No autograd graph is recorded" in " ".join(PreprocessingANN.value_and_hills.__doc__.split())


def test_cpu_tensor_names_the_route_that_remains():
    w = wl.get_workload("C3")
    model = wl.build_model(w, torch.device("cpu"), 0).double().requires_grad_(False)
    x = w.make_frames(3, seed=1).double()
    centers, heights, sigma = torch.zeros((4, w.out_dim()), dtype=torch.float64), torch.ones(4, dtype=torch.float64), 0.5
    with pytest.raises(NotImplementedError, match=r"use `model\(x\)`, form the hill sum and its derivative with torch, then `value_and_vjp`"):
        model.value_and_hills(x, centers, heights, sigma)
    with pytest.raises(NotImplementedError, match=r"value_and_hills needs a FeatureLayer .* take torch\.autograd\.grad"):
        model.preprocessing_layer.value_and_hills(x, torch.zeros((4, w.feature_dim()), dtype=torch.float64), heights, sigma)
    with pytest.raises(NotImplementedError):                            # the gate comes before `into` and before the other arguments
        model.value_and_hills(x, centers[:, :-1], heights, -1.0, into=(centers, centers))
    with pytest.raises(NotImplementedError):
        model.preprocessing_layer.value_and_hills(x, centers, heights, sigma, into=(centers,))


def test_float32_x_is_refused_with_the_route():
    x = torch.zeros((5, 22, 3), dtype=torch.float32)
    with pytest.raises(TypeError, match=r"value_and_hills is float64: call \.double\(\) .* form the hill sum"):
        ann._one_launch_arguments(ann._HILLS, x, (torch.zeros((1, 8)), 1.0, 1.0, None), None, 22, 8, (), None)
    with pytest.raises(AssertionError, match="Input should be a 3d torch tensor"):      # x's shape comes first
        ann._one_launch_arguments(ann._HILLS, x[:, :-1], (torch.zeros((1, 8)), 1.0, 1.0, None), None, 22, 8, (), None)


def test_arguments_are_checked_before_any_device_call():
    """ann._check_hills_args is what both methods call before the plan is looked up; tensors on the meta device stand for 'another
    device' here."""
    n, n_inp, d, H = 5, 22, 8, 6
    x = torch.zeros((n, n_inp, 3), dtype=torch.float64)
    y, bias, dx = torch.zeros((n, d), dtype=torch.float64), torch.zeros(n, dtype=torch.float64), torch.zeros_like(x)
    table = torch.linspace(-1.0, 1.0, 10 * d, dtype=torch.float64).reshape(10, d)
    c, w, s = table[:H], torch.linspace(0.2, 1.2, H, dtype=torch.float64), torch.linspace(0.5, 2.0, d, dtype=torch.float64)

    def check(centers=c, heights=w, sigma=s, period=None, into=None, owner=None):
        return ann._check_hills_args("value_and_hills", x, d, centers, heights, sigma, period, into, owner=owner)

    got = check()
    assert got[0].data_ptr() == table.data_ptr() and got[0].shape == (H, d)          # a preallocated table's prefix: as it is
    assert got[1].data_ptr() == w.data_ptr() and got[2].data_ptr() == s.data_ptr() and got[3:] == (None, None, None, None)
    got = check(c.tolist(), 0.7, 0.4, period=[0.0] * d, into=(y, bias, dx))
    assert torch.equal(got[0], c) and torch.equal(got[1], torch.full((H,), 0.7, dtype=torch.float64))
    assert torch.equal(got[2], torch.full((d,), 0.4, dtype=torch.float64)) and got[3].dtype == torch.float64
    assert got[4] is y and got[5] is bias and got[6] is dx
    got = check(c.float(), w.float(), s.expand(H, d))
    assert all(t.dtype == torch.float64 and t.is_contiguous() for t in got[:3]) and got[2].shape == (H, d)
    assert torch.equal(got[0], c.float().double())
    for empty in (table[:0], []):                                                         # no hills yet
        got = check(empty, torch.zeros(0, dtype=torch.float64), s)
        assert got[0].shape == (0, d) and got[1].shape == (0,)
    assert check(table[:0], 1.0, 0.5)[1].shape == (0,)
    assert check(into=[y.reshape(-1), bias, dx.reshape(-1)])[6].dim() == 1              # the element count is what counts
    for bad in (c[:, :-1], c.reshape(-1), c[0], torch.zeros(()), c.to("meta")):
        with pytest.raises(ValueError, match="centers"):
            check(centers=bad)
    with pytest.raises(TypeError, match="centers"):
        check(centers=1.0)
    for bad in (w[:-1], w.reshape(H, 1), torch.ones(H + 1, dtype=torch.float64), w.to("meta")):
        with pytest.raises(ValueError, match="heights"):
            check(heights=bad)
    for bad in (s[:-1], s.reshape(d, 1), s.expand(H + 1, d), s.expand(H - 1, d), s.to("meta")):
        with pytest.raises(ValueError, match="sigma"):
            check(sigma=bad)
    for bad in (s[:-1], s.expand(H, d), s.to("meta")):
        with pytest.raises(ValueError, match="period"):
            check(period=bad)
    for what, good in (("centers", c), ("heights", w), ("sigma", s), ("period", s)):
        with pytest.raises(TypeError, match=what):
            check(**{what: (good * 4).to(torch.int64)})
        with pytest.raises(TypeError, match=what):
            check(**{what: "wide"})
    zero_in_one_row = s.expand(H, d).clone()
    zero_in_one_row[3, 2] = 0.0
    for bad in (0.0, -0.5, NAN, -s, [0.5] * (d - 1) + [0.0], torch.where(s > 1.0, -s, s).float(), zero_in_one_row, s * NAN):
        with pytest.raises(ValueError, match="sigma"):
            check(sigma=bad)
    with pytest.raises(NotImplementedError, match=r"at most 8 outputs \(got 9\); use `model\(x\)`, form the hill sum"):
        ann._check_hills_args("value_and_hills", x, 9, torch.zeros((H, 9), dtype=torch.float64), w, 0.5, None, None)
    for bad in ((y, dx), (y, bias, dx, dx), (y, bias, None), [y.numpy(), bias, dx]):
        with pytest.raises(TypeError, match=r"triple of tensors \(y, bias, dx\)"):
            check(into=bad)
    for bad in ((y.float(), bias, dx), (y, bias.float(), dx), (y, bias, dx.float())):
        with pytest.raises(TypeError, match="float64"):
            check(into=bad)
    for bad in ((y[:4], bias, dx), (y, bias[:4], dx), (y, bias, dx[:, :-1]), (y.t(), bias, dx), (y, torch.zeros(2 * n, dtype=torch.float64)[::2], dx),
                (y.to("meta"), bias, dx), (y, bias.to("meta"), dx), (y, bias, dx.to("meta"))):
        with pytest.raises(ValueError, match="into"):
            check(into=bad)
    with pytest.raises(ValueError, match="sigma"):                                      # `sigma` is looked at before `into`
        check(sigma=-s, into=(y.to("meta"), bias, dx))
