"""The OPES bias of the float64 one-launch family on the host (no GPU): one frame's bias V = scale log(P / norm + epsilon) and its
derivative (molann_selftest_opes_f64 adds up the kernel's own __host__ __device__ functions, kernel by kernel, and transforms the sums)
against the formula written in torch float64 with dy by autograd, the torch helper molann_amd.bias.opes_kernel_sum against the same
formula, the refusals of MolANN.value_and_opes / PreprocessingANN.value_and_opes that need no device, the scalar checks both share
(run before anything touches a device) and the C entry's symbols and its answer to a null plan.

The bounds are those of the hills' host test - a sum within 1e-12 of the sum of its terms' magnitudes - on the sums the logarithm is
taken of, without that test's floor of 1 under the magnitudes (a floor would be carried through 1 / u, up to 1e8 here, and check
nothing): P within dP = 1e-12 sum_h |w_h e_h| and acc_k within 1e-12 sum_h |w_h e_h s_k / sigma_k| over the kernels inside the
cutoff.  With u = P / norm + epsilon and f = scale / (norm u), V is held within |f| dP + 1e-12 max(1, |V|) - dP carried through the
logarithm's derivative, then the logarithm's own rounding - and dy_k within |f| 1e-12 sum_h |w_h e_h s_k / sigma_k| + |dy_k| dP /
(norm u): the bound on the sum of the terms, and dP carried through 1 / u.  Where no kernel is inside the cutoff the bounds are 0 and
dy is 0 exactly.  The draws keep the weights positive, so u >= epsilon."""

import ctypes
import math
import os

import pytest
import torch

from molann_amd import _capi, ann, bias as mb, workloads as wl
from molann_amd.ann import MolANN, PreprocessingANN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["molann_value_and_opes_f64", "molann_plan_supports_value_and_opes_f64", "molann_selftest_opes_f64"]
NAN, INF = float("nan"), float("inf")


def kernel_sum(y, centers, heights, sigma, period, cutoff):
    """(P, q, sum_h |w_h e_h|, sum_h |w_h e_h s_k / sigma_k|, the sums over the kernels inside the cutoff) of the issue's formula in torch float64, differentiable in y: y [d],
    centers [H, d], heights [H], sigma [d] or [H, d], period [d] or None, cutoff a float (inf: none)."""
    d = y[None, :] - centers
    if period is not None:
        periodic = period > 0
        P = torch.where(periodic, period, torch.ones_like(period))
        d = torch.where(periodic[None, :], d - P * torch.round(d / P), d)
    s = d / sigma
    q = (s * s).sum(1)
    c2 = cutoff * cutoff
    c0 = math.exp(-0.5 * c2)
    e = torch.exp(-0.5 * q)
    inside = ~(q >= c2)
    k = torch.where(inside, heights * (e - c0), torch.zeros_like(q))
    terms = torch.where(inside[:, None], (heights * e)[:, None] * s / sigma, torch.zeros_like(s))
    return k.sum(), q, torch.where(inside, heights * e, torch.zeros_like(q)).abs().sum().detach(), terms.abs().sum(0).detach()


def formula(y, centers, heights, sigma, period, scale, norm, epsilon, cutoff):
    """(V, dV/dy by autograd, the bound on V, the bound on dy) of the issue's formula, the bounds as the module's docstring has them."""
    yy = y.clone().requires_grad_(True)
    p, q, p_abs, t_abs = kernel_sum(yy, centers, heights, sigma, period, cutoff)
    u = p / norm + epsilon
    v = scale * torch.log(u)
    (dy,) = torch.autograd.grad(v, yy)
    u, v = float(u.detach()), float(v.detach())
    p_bound = 1e-12 * float(p_abs)
    f = abs(scale) / (norm * u)
    v_bound = f * p_bound + 1e-12 * max(1.0, abs(v))
    dy_bound = f * 1e-12 * t_abs + dy.abs() / u * p_bound / norm
    return v, dy, v_bound, dy_bound, q.detach()


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def selftest(y, centers, heights, sigma, period, scale, norm, epsilon, cutoff):
    d = y.numel()
    dy = torch.full((d,), 7.5, dtype=torch.float64)
    v = _capi.lib().molann_selftest_opes_f64(_ptr(y), d, _ptr(centers), _ptr(heights), heights.numel(), _ptr(sigma), d if sigma.dim() == 2 else 0,
                                             _ptr(period), scale, norm, epsilon, cutoff, _ptr(dy))
    return v, dy


def _draws():
    """1800 seeded (y, centers, heights, sigma, period, scale, norm, epsilon, cutoff): d in {1, 3, 8}, H in 0..40, the widths shared or
    per kernel, half of the columns periodic on average (a third of the draws without a period row), positive weights, the cutoff
    in {inf, 5, 3} and epsilon in {1e-3, 1e-6} in turn, norm = 0.02 of the weights' sum.  y is near a kernel's centre in half the draws."""
    g = torch.Generator().manual_seed(47)
    f64 = dict(generator=g, dtype=torch.float64)
    draws = []
    for i in range(1800):
        d, H = (1, 3, 8)[i % 3], int(torch.randint(0, 41, (1,), generator=g))
        centers = 2.0 * torch.randn(H, d, **f64)
        y = 2.0 * torch.randn(d, **f64)
        if H and (i // 7) % 2:
            y = centers[i % H] + 0.3 * torch.randn(d, **f64)
        heights = 0.2 + torch.rand(H, **f64)
        sigma = 0.2 + 1.5 * torch.rand((H, d) if (i // 3) % 2 else (d,), **f64)
        period = None
        if (i // 6) % 3:
            pick = torch.randint(0, 2, (d,), generator=g) == 0
            period = torch.where(pick, 1.0 + 5.0 * torch.rand(d, **f64), torch.zeros(d, dtype=torch.float64))
            if i % 7 == 0:
                period[0] = -1.0          # P <= 0: not periodic
        cutoff, epsilon = (INF, 5.0, 3.0)[(i // 18) % 3], (1e-3, 1e-6)[(i // 54) % 2]
        norm = 0.02 * max(float(heights.sum()), 1.0)
        draws.append((y, centers, heights, sigma, period, 2.25 if i % 5 else -0.75, norm, epsilon, cutoff))
    return draws


def test_selftest_against_the_formula():
    worst_v = worst_dy = 0.0
    seen, dropped, kept = set(), 0, 0
    for y, centers, heights, sigma, period, scale, norm, epsilon, cutoff in _draws():
        v, dy = selftest(y, centers, heights, sigma, period, scale, norm, epsilon, cutoff)
        v_want, dy_want, v_bound, dy_bound, q = formula(y, centers, heights, sigma, period, scale, norm, epsilon, cutoff)
        if q.numel() and float((q - cutoff * cutoff).abs().min()) < 1e-9:
            continue                      # on the cutoff's edge the two may drop different kernels: the derivative jumps there
        assert abs(v - v_want) <= v_bound and bool(((dy - dy_want).abs() <= dy_bound).all()), (v, v_want, v_bound, dy, dy_want, dy_bound)
        worst_v = max(worst_v, abs(v - v_want) / v_bound)
        worst_dy = max(worst_dy, float(((dy - dy_want).abs() / dy_bound.clamp(min=1e-300)).max()))
        seen.add((y.numel(), sigma.dim(), period is not None, cutoff, epsilon))
        dropped, kept = dropped + int((q >= cutoff * cutoff).sum()), kept + int((q < cutoff * cutoff).sum())
    print("worst error / bound: V %.3g, dy %.3g; %d kernels inside the cutoff, %d outside" % (worst_v, worst_dy, kept, dropped))
    assert len(seen) == 3 * 2 * 2 * 3 * 2, len(seen)        # d x widths x period x cutoff x epsilon: every combination drawn
    assert dropped > 1000 and kept > 1000
    assert worst_v <= 1.0 and worst_dy <= 1.0, (worst_v, worst_dy)


def test_edge_cases():
    t = lambda *v: torch.tensor(v, dtype=torch.float64)       # noqa: E731
    L = _capi.lib()
    y, centers, sigma = t(0.3, -0.2), t(0.1, 0.1, -0.4, 0.3).reshape(2, 2), t(0.5, 0.7)
    w = t(0.8, 0.6)
    scale, norm, eps = 2.25, 0.03, 1e-3
    # no kernels yet: scale log(epsilon) and dy = 0 exactly, with and without pointers to a table
    for cutoff in (INF, 3.0):
        v, dy = selftest(y, centers[:0], t(), sigma, None, scale, norm, eps, cutoff)
        assert v == scale * math.log(eps) and bool((dy == 0.0).all())
        dy = torch.full((2,), 7.5, dtype=torch.float64)
        assert L.molann_selftest_opes_f64(_ptr(y), 2, None, None, 0, None, 0, None, scale, norm, eps, cutoff, _ptr(dy)) == scale * math.log(eps)
        assert bool((dy == 0.0).all())
    # a kernel with q >= c2 adds exact zeros: the table with it and without it gives the same bits; alone it leaves scale log(epsilon)
    v1, dy1 = selftest(y, centers, w, sigma, None, scale, norm, eps, 3.0)
    far = torch.cat([centers, t(0.3 + 3.0 * 0.5, -0.2).reshape(1, 2), t(9.0, 9.0).reshape(1, 2)])       # q = 9 = c2 exactly, and far beyond
    assert float(((far[2] - y) / sigma).pow(2).sum()) == 9.0
    v2, dy2 = selftest(y, far, t(0.8, 0.6, 5.0, 7.0), sigma, None, scale, norm, eps, 3.0)
    assert v2 == v1 and torch.equal(dy2, dy1) and v1 > scale * math.log(eps)
    v3, dy3 = selftest(y, far[2:], t(5.0, 7.0), sigma, None, scale, norm, eps, 3.0)
    assert v3 == scale * math.log(eps) and bool((dy3 == 0.0).all())
    v4, _ = selftest(y, far, t(0.8, 0.6, 5.0, 7.0), sigma, None, scale, norm, eps, 3.5)                 # inside a wider cutoff it counts
    assert v4 != v1
    # a NaN in y: a NaN bias and NaN in every column, at a finite and at an infinite cutoff; so for a NaN in a centre
    for cutoff in (3.0, INF):
        for yy, cc in ((t(NAN, -0.2), centers), (y, t(0.1, 0.1, NAN, 0.3).reshape(2, 2))):
            v, dy = selftest(yy, cc, w, sigma, t(2.0, 0.0), scale, norm, eps, cutoff)
            assert math.isnan(v) and bool(torch.isnan(dy).all()), (cutoff, v, dy)
    # dy may be null; d outside 1..8: NaN, dy untouched
    assert L.molann_selftest_opes_f64(_ptr(y), 2, _ptr(centers), _ptr(w), 2, _ptr(sigma), 0, None, scale, norm, eps, 3.0, None) == v1
    y9 = torch.zeros(9, dtype=torch.float64)
    for d in (0, 9, -1):
        dy = torch.full((9,), 7.5, dtype=torch.float64)
        assert math.isnan(L.molann_selftest_opes_f64(_ptr(y9), d, None, None, 0, _ptr(y9 + 1.0), 0, None, scale, norm, eps, INF, _ptr(dy)))
        assert bool((dy == 7.5).all())
    # no cutoff is the limit of a large one: at cutoff 40 exp(-800) underflows to 0 and nothing here is dropped, bit for bit
    va, dya = selftest(y, centers, w, sigma, None, scale, norm, eps, INF)
    vb, dyb = selftest(y, centers, w, sigma, None, scale, norm, eps, 40.0)
    assert math.exp(-800.0) == 0.0 and va == vb and torch.equal(dya, dyb)


def test_shared_and_repeated_sigma_give_the_same_bits():
    n = 0
    for y, centers, heights, sigma, period, scale, norm, epsilon, cutoff in _draws()[:600]:
        if sigma.dim() != 1:
            continue
        v, dy = selftest(y, centers, heights, sigma, period, scale, norm, epsilon, cutoff)
        v2, dy2 = selftest(y, centers, heights, sigma.expand(centers.shape[0], -1).contiguous(), period, scale, norm, epsilon, cutoff)
        assert v == v2 and torch.equal(dy, dy2)
        n += 1
    assert n >= 200


def test_opes_kernel_sum_against_the_formula():
    g = torch.Generator().manual_seed(5)
    f64 = dict(generator=g, dtype=torch.float64)
    H, d, M = 20, 3, 11
    centers, heights = torch.randn(H, d, **f64), 0.2 + torch.rand(H, **f64)
    points = torch.cat([torch.randn(M - 4, d, **f64), centers[:4] + 0.1])
    period = torch.tensor([0.0, 2.5, 0.0], dtype=torch.float64)
    inside = outside = 0
    for sigma in (0.4 + torch.rand(d, **f64), 0.4 + torch.rand(H, d, **f64)):
        for per in (None, period):
            for cutoff in (None, 3.0):
                got = mb.opes_kernel_sum(points, centers, heights, sigma, per, cutoff, chunk=7)       # 7 + 7 + 6 kernels
                want = torch.stack([kernel_sum(p, centers, heights, sigma, per, INF if cutoff is None else cutoff)[0] for p in points])
                assert got.dtype == torch.float64 and got.shape == (M,)
                assert float((got - want).abs().max()) <= 1e-13 * max(1.0, float(want.abs().max())), (cutoff, got, want)
                lists = mb.opes_kernel_sum(points.tolist(), centers.tolist(), heights.tolist(), sigma, per, cutoff, chunk=20)      # sequences; one chunk
                assert float((got - lists).abs().max()) <= 1e-14 * max(1.0, float(want.abs().max()))
                if cutoff is not None:
                    q = torch.stack([kernel_sum(p, centers, heights, sigma, per, cutoff)[1] for p in points])
                    inside, outside = inside + int((q < 9.0).sum()), outside + int((q >= 9.0).sum())
    assert inside > 0 and outside > 0
    assert float(mb.opes_kernel_sum(points, centers[:0], heights[:0], 0.5).abs().max()) == 0.0          # no kernels: zeros
    one = mb.opes_kernel_sum(points, centers, 0.7, 0.5)                                                 # a float weight and width
    assert float((one - mb.opes_kernel_sum(points, centers, torch.full((H,), 0.7, dtype=torch.float64), torch.full((d,), 0.5, dtype=torch.float64))).abs().max()) <= 1e-15
    assert "opes_kernel_sum" in mb.__all__
    for bad in (dict(sigma=0.0), dict(sigma=-sigma), dict(cutoff=0.0), dict(cutoff=NAN)):
        kw = dict(sigma=sigma, cutoff=None)
        kw.update(bad)
        with pytest.raises(ValueError):
            mb.opes_kernel_sum(points, centers, heights, kw["sigma"], None, kw["cutoff"])
    with pytest.raises(ValueError, match="points"):
        mb.opes_kernel_sum(points[0], centers, heights, 0.5)


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_declared_exported_and_bound(name):
    header = open(os.path.join(ROOT, "include", "molann_hip.h")).read()
    assert name + "(" in header, name
    fn = getattr(_capi.lib(), name)
    assert fn.argtypes is not None and len(fn.argtypes) == {SYMBOLS[0]: 19, SYMBOLS[1]: 1, SYMBOLS[2]: 13}[name], name
    assert name in _capi.declared_symbols()


def test_null_plan():
    L = _capi.lib()
    assert L.molann_plan_supports_value_and_opes_f64(None) == _capi.E_NULL
    for n in (1, 0):
        for n_kernels in (3, 0, -1):
            for cutoff in (3.0, -1.0):        # a null plan is named before a bad scalar is
                assert L.molann_value_and_opes_f64(None, None, n, None, None, None, None, n_kernels, None, 0, None, 2.25, 1.0, 1e-3, cutoff, None, None,
                                                   None, None) == _capi.E_NULL
    assert _capi.lib().molann_abi_version() == 1


def test_methods_exist_and_say_what_is_out_of_scope():
    assert callable(_capi.Plan.supports_value_and_opes_f64) and callable(_capi.Plan.value_and_opes_f64) and callable(_capi.Plan.value_and_opes)
    doc = " ".join(MolANN.value_and_opes.__doc__.split())
    for words in ("float32", "GraphedForces", "No autograd graph is recorded", "at most 8 outputs", "neighbour lists", "depositing",
                  "`value_and_bias`", "opes_kernel_sum"):
        assert words in doc, (words, doc)
    assert "No autograd graph is recorded" in " ".join(PreprocessingANN.value_and_opes.__doc__.split())
    assert ann._ONE_LAUNCH_NAME[ann._OPES] == "value_and_opes" and ann._ONE_LAUNCH_OP[ann._OPES] == "op_opes"


def test_cpu_tensor_names_the_route_that_remains():
    w = wl.get_workload("C3")
    model = wl.build_model(w, torch.device("cpu"), 0).double().requires_grad_(False)
    x = w.make_frames(3, seed=1).double()
    centers, heights, sigma = torch.zeros((4, w.out_dim()), dtype=torch.float64), torch.ones(4, dtype=torch.float64), 0.5
    route = r"use `model\(x\)`, form the kernel sum with `molann_amd\.bias\.opes_kernel_sum`, its logarithm and its derivative with torch, then `value_and_vjp`"
    with pytest.raises(NotImplementedError, match=route):
        model.value_and_opes(x, centers, heights, sigma, 2.25, 1.0, 1e-3)
    with pytest.raises(NotImplementedError, match=route):                       # a float32 CPU tensor: the same refusal
        model.float().value_and_opes(x.float(), centers, heights, sigma, 2.25, 1.0, 1e-3, cutoff=4.0)
    model.double()
    with pytest.raises(NotImplementedError, match=r"value_and_opes needs a FeatureLayer .* take torch\.autograd\.grad"):
        model.preprocessing_layer.value_and_opes(x, torch.zeros((4, w.feature_dim()), dtype=torch.float64), heights, sigma, 2.25, 1.0, 1e-3)
    with pytest.raises(NotImplementedError):                            # the gate comes before the scalars, `into` and the other arguments
        model.value_and_opes(x, centers[:, :-1], heights, -1.0, NAN, -1.0, 0.0, cutoff=-2.0, into=(centers, centers))
    with pytest.raises(NotImplementedError):
        model.preprocessing_layer.value_and_opes(x, centers, heights, sigma, 2.25, 1.0, 1e-3, into=(centers,))


def test_float32_x_is_refused_with_the_route():
    x = torch.zeros((5, 22, 3), dtype=torch.float32)
    extra = (torch.zeros((1, 8)), 1.0, 1.0, 2.25, 1.0, 1e-3, None, None)
    with pytest.raises(TypeError, match=r"value_and_opes is float64: call \.double\(\) .* form the kernel sum"):
        ann._one_launch_arguments(ann._OPES, x, extra, None, 22, 8, (), None)
    with pytest.raises(AssertionError, match="Input should be a 3d torch tensor"):      # x's shape comes first
        ann._one_launch_arguments(ann._OPES, x[:, :-1], extra, None, 22, 8, (), None)


def test_scalars_are_checked_before_any_device_call():
    """ann._check_opes_args is what both methods call before the plan is looked up: the four scalars first, then the cap on the
    outputs, then value_and_hills' own checks of the tensors (tests/test_hills_f64_host.py has those one by one)."""
    n, n_inp, d, H = 5, 22, 8, 6
    x = torch.zeros((n, n_inp, 3), dtype=torch.float64)
    y, bias, dx = torch.zeros((n, d), dtype=torch.float64), torch.zeros(n, dtype=torch.float64), torch.zeros_like(x)
    table = torch.linspace(-1.0, 1.0, 10 * d, dtype=torch.float64).reshape(10, d)
    c, w, s = table[:H], torch.linspace(0.2, 1.2, H, dtype=torch.float64), torch.linspace(0.5, 2.0, d, dtype=torch.float64)

    def check(scale=2.25, norm=0.5, epsilon=1e-3, cutoff=None, centers=c, sigma=s, period=None, into=None, d_out=d):
        return ann._check_opes_args("value_and_opes", x, d_out, centers, w, sigma, scale, norm, epsilon, cutoff, period, into)

    got = check()
    assert got[0].data_ptr() == table.data_ptr() and got[1].data_ptr() == w.data_ptr() and got[2].data_ptr() == s.data_ptr() and got[3] is None
    assert got[4:8] == (2.25, 0.5, 1e-3, INF) and got[8:] == (None, None, None)
    got = check(scale=-3, norm=2, cutoff=4, period=[0.0] * d, into=(y, bias, dx))
    assert got[4:8] == (-3.0, 2.0, 1e-3, 4.0) and all(isinstance(v, float) for v in got[4:8])
    assert got[3].dtype == torch.float64 and got[8] is y and got[9] is bias and got[10] is dx
    assert check(cutoff=INF)[7] == INF
    meta = c.to("meta")                         # stands for 'another device': looked at only after the scalars
    for bad in (dict(scale=NAN), dict(scale=INF), dict(scale=-INF), dict(norm=0.0), dict(norm=-1.0), dict(norm=NAN), dict(norm=INF),
                dict(epsilon=0.0), dict(epsilon=-1e-3), dict(epsilon=NAN), dict(epsilon=INF), dict(cutoff=0.0), dict(cutoff=-3.0), dict(cutoff=NAN)):
        with pytest.raises(ValueError, match=list(bad)[0]):
            check(centers=meta, sigma=-s, d_out=9, **bad)
    for bad in (dict(scale="2"), dict(norm=None), dict(epsilon=torch.tensor(1e-3)), dict(cutoff=[4.0]), dict(scale=True)):
        with pytest.raises(TypeError, match=list(bad)[0]):
            check(centers=meta, **bad)
    with pytest.raises(NotImplementedError, match=r"at most 8 outputs \(got 9\); use `model\(x\)`, form the kernel sum"):
        ann._check_opes_args("value_and_opes", x, 9, torch.zeros((H, 9), dtype=torch.float64), w, 0.5, 2.25, 0.5, 1e-3, None, None, None)
    with pytest.raises(ValueError, match="centers"):
        check(centers=meta)
    with pytest.raises(ValueError, match="sigma"):
        check(sigma=-s, into=(y.to("meta"), bias, dx))
    with pytest.raises(TypeError, match=r"triple of tensors \(y, bias, dx\)"):
        check(into=(y, dx))
