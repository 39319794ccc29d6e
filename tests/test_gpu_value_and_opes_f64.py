"""Float64 values, an OPES bias on them - the logarithm of a kernel density - and its gradient in ONE launch (molann_value_and_opes_f64 ->
frames_value_opes_f64_kernel): V = scale log(P / norm + epsilon), P = sum_h w_h (exp(-q_h / 2) - exp(-c^2 / 2)) over the kernels with
q_h = sum_k (d_hk / sigma_hk)^2 < c^2, d_h = y - c_h wrapped for periodic outputs, against float64 autograd on the CPU through the
oracle's preprocessing, a copy of the head and the formula in torch - never the code under test.  Bounds, the float64 family's: y
within 1e-10 max(1, |y|max), the bias within 1e-10 max(1, |V|max), dx within 1e-9 max(1e-3, |dx|max); the hills test's `_close` prints
every error before it asserts.

The kernel tables are the hills tests' (`_hill_table`, built from the REFERENCE's y with its asserts on near and far kernels and on the
wrap's seam), the heights made positive afterwards; norm = 0.02 x the sum of the heights (0.02 for an empty table, whose sum is 0 and
whose bias does not depend on it), scale = 2.25.  `_table` adds, on reference values: no (frame, kernel) pair has |q - c^2| < 1e-6 (the
derivative jumps there), and every table of two kernels or more under a finite cutoff has a pair inside the cutoff and a pair outside
(kernel 1 is the builder's far kernel; a table of one kernel has its one pair inside)."""

import math

import pytest
import torch

import isolation
import placement as pl
import test_gpu_random_backward as rb
import test_gpu_value_and_hills_f64 as vh
import test_gpu_value_and_restraint_f64 as vr
import test_gpu_value_and_vjp_f64 as vv
from molann_amd import _capi, ann, workloads as wl
from molann_amd.ann import MolANN

pytestmark = pytest.mark.gpu
KERNEL = "frames_value_opes_f64_kernel"
VJP_KERNEL = "frames_value_vjp_f64_kernel"
TWO_PI = 2.0 * math.pi
NAN, INF = float("nan"), float("inf")
CPU = torch.device("cpu")
SCALE = 2.25
ROUTE = r"use `model\(x\)`, form the kernel sum with `molann_amd\.bias\.opes_kernel_sum`, its logarithm and its derivative with torch"


def _density(y, centers, heights, sigma, period, cutoff):
    """(P [n], q [n, H]) of the issue's formula, in torch on y's device: differentiable in y.  cutoff: None or a float."""
    s = vh._wrapped(y, centers, period) / sigma
    q = (s * s).sum(dim=2)
    if centers.shape[0] == 0:
        return (y * 0.0).sum(dim=1), q
    c2 = INF if cutoff is None else cutoff * cutoff
    k = torch.where(q >= c2, torch.zeros_like(q), torch.exp(-0.5 * q) - math.exp(-0.5 * c2))
    return (heights * k).sum(dim=1), q


def _bias(y, table, period, norm, epsilon, cutoff, scale=SCALE):
    p, _ = _density(y, *table, period, cutoff)
    return scale * torch.log(p / norm + epsilon)


def _cotangent(y, table, period, norm, epsilon, cutoff):
    """dV/dy [n, d] of the issue's formula, by torch on y's device."""
    yy = y.detach().clone().requires_grad_(True)
    with torch.enable_grad():
        (g,) = torch.autograd.grad(_bias(yy, table, period, norm, epsilon, cutoff).sum(), yy)
    return g


def _norm(heights):
    return 0.02 * float(heights.sum()) if heights.numel() else 0.02


def _conditions(y_ref, table, period, cutoff):
    """The module docstring's conditions on a table under a cutoff, on reference values; returns (pairs inside, pairs outside)."""
    H = table[0].shape[0]
    if H == 0 or cutoff is None:
        return H * y_ref.shape[0], 0
    _, q = _density(y_ref.detach(), *table, period, cutoff)
    c2 = cutoff * cutoff
    assert float((q - c2).abs().min()) >= 1e-6, "a (frame, kernel) pair within 1e-6 of the cutoff"
    inside, outside = int((q < c2).sum()), int((q >= c2).sum())
    assert inside > 0, "no (frame, kernel) pair inside the cutoff"
    assert outside > 0 or H == 1, "no (frame, kernel) pair outside the cutoff"
    return inside, outside


def _table(y_ref, y_tab, period, n_kernels, per_kernel, seed, cutoffs):
    """((centers, heights, sigma), norm) on the CPU: the hills tests' table with positive heights, the conditions asserted for every cutoff."""
    (c, h, s), _ = vh._hill_table(y_ref, y_tab, period, n_kernels, per_kernel, seed)
    table = (c, h.abs(), s)
    for cutoff in cutoffs:
        _conditions(y_ref, table, period, cutoff)
    return table, _norm(table[1])


def _oracle(xx, y, table, period, norm, epsilon, cutoff):
    """(y, V, dV/dx) by float64 autograd of the formula."""
    v = _bias(y, table, period, norm, epsilon, cutoff)
    (gx,) = torch.autograd.grad(v.sum(), xx, retain_graph=True)
    return y.detach(), v.detach(), gx


def _call(model, x, table, period, norm, epsilon, cutoff, into=None, scale=SCALE):
    """((y, bias, dx), launch info) of the module's method, the tensors moved to x's device."""
    on = lambda t: None if t is None else t.to(x.device)       # noqa: E731
    p = period if period is not None and bool((period > 0).any()) else None
    out = model.value_and_opes(x, on(table[0]), on(table[1]), on(table[2]), scale, norm, epsilon, cutoff, on(p), into=into)
    torch.cuda.synchronize()
    return out, vh._info(model)


def _check(model, xx, y_ref, x, table, period, norm, epsilon, cutoff, what):
    want = _oracle(xx, y_ref, table, period, norm, epsilon, cutoff)
    got, info = _call(model, x, table, period, norm, epsilon, cutoff)
    assert info.startswith(KERNEL + " (values + opes in one launch; ") and info.count("_kernel") == 1, info
    vh._close(got, want, what)
    return got, want, info


# ---- 1. every lane group -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_inp,lanes", [(7, 8), (12, 16), (30, 32), (40, 64)])
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "no_alignment"])
@pytest.mark.parametrize("head", [True, False], ids=["head", "features"])
def test_lane_groups(n_inp, lanes, aligned, head, hip_device):
    """The family's small cases: every lane-group width, with and without an alignment and a head; 5 frames, 9 kernels (a lane with
    two kernels, with one, with none), widths per kernel, output 0 periodic, cutoff 5, epsilon 1e-3; untouched atoms' rows exactly 0."""
    case = vh._small_case(n_inp, aligned, head)
    model = case.build(hip_device).double().requires_grad_(False)
    d_out = case.mlp[-1] if head else case.d_feat()
    if head:       # the head's widest layer input (the 12 feature columns) asks for at least 16 lanes
        lanes = max(lanes, 16)
    period = torch.zeros(d_out, dtype=torch.float64)
    period[0] = 1.3
    args = (case.feats, case.uav, case.align)
    x = case.frames(5, seed=n_inp + 5, dev=CPU).double().to(hip_device)
    x_tab = case.frames(65, seed=900 + n_inp, dev=CPU).double().to(hip_device)
    xx, y_ref = vr._reference_y(model, *args, x)
    _, y_tab = vr._reference_y(model, *args, x_tab)
    table, norm = _table(y_ref, y_tab, period, 9, True, n_inp + 14, (5.0,))
    (y, v, dx), want, info = _check(model, xx, y_ref, x, table, period, norm, 1e-3, 5.0, (case.name, aligned, head))
    assert "%d lanes per frame" % lanes in info, info
    assert float(want[2].abs().max()) > 1e-3, "the reference's forces are (nearly) zero"
    untouched = sorted(set(range(n_inp)) - case.touched())
    assert len(untouched) == n_inp - (7 if aligned or head else 6)
    if untouched:
        assert float(dx[:, untouched].abs().max()) == 0.0


# ---- 2. table sizes, cutoffs, epsilons -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65])
@pytest.mark.parametrize("name", ["C3", "C3_angles"])
def test_table_sizes(name, n, hip_device):
    """C3 (8 outputs, every third periodic) and C3's two dihedral angles (period 2 pi): no kernel yet, one, 40 (widths per kernel); with
    and without a cutoff; epsilon 1e-3 and 1e-6.  Without kernels y has value_and_vjp's bits, the bias is scale log(epsilon) and dx
    is exactly 0, over NaN-filled buffers."""
    if name == "C3":
        w, model, args = vv._shared("C3", hip_device)
        period = vh._period_row(w.out_dim(), 1.1, 3)
    else:
        w, case, model = vr._c3_angles(hip_device)
        args, period = (case.feats, True, case.align), torch.tensor([TWO_PI, TWO_PI], dtype=torch.float64)
    d = period.numel()
    x = w.make_frames(n, seed=140 + n).double().to(hip_device)
    x_tab = w.make_frames(65, seed=145).double().to(hip_device)
    xx, y_ref = vr._reference_y(model, *args, x)
    _, y_tab = vr._reference_y(model, *args, x_tab)
    yv, _, info = vv._call(model, x, torch.ones((n, d), dtype=torch.float64, device=hip_device))
    assert VJP_KERNEL in info
    yv = yv.clone()
    for n_kernels in (0, 1, 40):
        table, norm = _table(y_ref, y_tab, period, n_kernels, n_kernels == 40, 141 + n + n_kernels, (None, 4.0))
        for cutoff in (None, 4.0):
            for epsilon in (1e-3, 1e-6):
                (y, v, dx), want, _ = _check(model, xx, y_ref, x, table, period, norm, epsilon, cutoff, (name, n, n_kernels, cutoff, epsilon))
                assert torch.equal(y, yv)
                if n_kernels == 0:
                    new = lambda *shape: torch.full(shape, NAN, dtype=torch.float64, device=hip_device)       # noqa: E731
                    into = (new(n, d), new(n), new(n, w.n_atoms, 3))
                    (y, v, dx), _ = _call(model, x, table, period, norm, epsilon, cutoff, into=into)
                    assert y is into[0] and torch.equal(y, yv) and bool((dx == 0).all())
                    assert float((v - SCALE * math.log(epsilon)).abs().max()) <= 1e-14 * abs(SCALE * math.log(epsilon))
                else:
                    assert float(want[2].abs().max()) > 1e-3, "the reference's forces are (nearly) zero"


# ---- 3. stepped-down rows, a long table --------------------------------------------------------------------------------------------
def test_stepped_down_rows_and_a_long_table(hip_device):
    """The [3, 682, 2] head of the restraint's test (2051 doubles per frame: two waves per block) through ctypes, with a table of 4099
    kernels (64 rounds of the lanes and 3 kernels more) under a cutoff of 4."""
    dims, block, lds = vr.STEPPED["step_down"]
    n, n_inp, n_kernels, cutoff = 3, 8, 4099, 4.0
    head, xx, y_ref, y_tab = vh._bonds_head(dims, n, n_inp, 3)
    period = torch.tensor([0.7, 0.0], dtype=torch.float64)
    (c, h, s), norm = _table(y_ref, y_tab, period, n_kernels, True, 80, (cutoff,))
    dev = hip_device
    with torch.cuda.device(dev):
        plan = _capi.Plan(n_inp, features=vr.BONDS, layer_dims=dims, activation=_capi.ACT_TANH)
        assert plan.supports_value_and_opes_f64()
        lins = [m for m in head if isinstance(m, torch.nn.Linear)]
        W, B = [lin.weight.to(dev).contiguous() for lin in lins], [lin.bias.to(dev).contiguous() for lin in lins]
        y, v, dx = (torch.full(sh, NAN, dtype=torch.float64, device=dev) for sh in ((n, 2), (n,), (n, n_inp, 3)))
        plan.value_and_opes(xx.detach().to(dev), W, B, c.to(dev), h.to(dev), s.to(dev), period.to(dev), SCALE, norm, 1e-3, cutoff, y, v, dx)
        torch.cuda.synchronize()
        info = plan.last_launch_info()
    assert info == "%s (values + opes in one launch; 64 lanes per frame) grid=%d block=%d lds=%d" % (KERNEL, -(-n // (block // 64)), block, lds), info
    vh._close((y, v, dx), _oracle(xx, y_ref, (c, h, s), period, norm, 1e-3, cutoff), ("step_down", n_kernels))


# ---- 4. larger frames --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [("P1", 9), ("C4", 3)])
def test_larger_frames(name, n, hip_device):
    w, model, args = vv._shared(name, hip_device)
    if name == "C4":
        assert w.n_atoms == 5000 and w.mlp_dims == [85, 128, 64, 8]
    x = w.make_frames(n, seed=7).double().to(hip_device)
    x_tab = w.make_frames(17 if name == "C4" else 65, seed=8).double().to(hip_device)
    period = vh._period_row(w.out_dim(), 1.1, 3)
    xx, y_ref = vr._reference_y(model, *args, x)
    _, y_tab = vr._reference_y(model, *args, x_tab)
    table, norm = _table(y_ref, y_tab, period, 75, True, 60, (4.0,))
    (_, _, dx), want, _ = _check(model, xx, y_ref, x, table, period, norm, 1e-3, 4.0, name)
    assert float(want[2].abs().max()) > 1e-3, "the reference's forces are (nearly) zero"
    untouched = sorted(set(range(w.n_atoms)) - {a - 1 for a in w.touched_atoms()})
    if untouched:
        assert float(dx[:, untouched].abs().max()) == 0.0


# ---- 5. the cap on the outputs -----------------------------------------------------------------------------------------------------
def test_eight_outputs_run_and_nine_are_refused(hip_device):
    w, model, args = vv._shared("C3", hip_device)
    assert w.out_dim() == 8
    x = w.make_frames(9, seed=31).double().to(hip_device)
    x_tab = w.make_frames(65, seed=32).double().to(hip_device)
    period = vh._period_row(8, 1.1, 3)
    xx, y_ref = vr._reference_y(model, *args, x)
    _, y_tab = vr._reference_y(model, *args, x_tab)
    for per_kernel in (False, True):
        table, norm = _table(y_ref, y_tab, period, 37, per_kernel, 33, (5.0,))
        _check(model, xx, y_ref, x, table, period, norm, 1e-3, 5.0, ("C3", per_kernel))
    # features only, the positions of three atoms: 9 outputs
    case = rb.Case("pos3", rb._chain(7, 3), [(rb.POS, [1, 3, 5])], align=[0, 2, 4, 6], mlp=None)
    pre = case.build(hip_device).double().requires_grad_(False)
    assert case.d_feat() == 9
    x9 = case.frames(4, seed=34, dev=CPU).double().to(hip_device)
    new = lambda *shape: torch.full(shape, NAN, dtype=torch.float64, device=hip_device)       # noqa: E731
    y, v, dx = new(4, 9), new(4), new(4, 7, 3)
    c, h, s = torch.zeros((3, 9), dtype=torch.float64, device=hip_device), torch.ones(3, dtype=torch.float64, device=hip_device), \
        torch.ones(9, dtype=torch.float64, device=hip_device)
    with pytest.raises(NotImplementedError, match=r"at most 8 outputs \(got 9\); " + ROUTE):
        pre.value_and_opes(x9, c, h, s, SCALE, 1.0, 1e-3, into=(y, v, dx))
    plan = vv._feature_plan(pre, x9)
    with torch.cuda.device(hip_device):
        assert plan.supports_value_and_restraint_f64() and not plan.supports_value_and_opes_f64()
        assert _capi.lib().molann_plan_supports_value_and_opes_f64(plan._handle) == 0
        for table in ((c, h), (None, None)):
            for cutoff in (4.0, -1.0):            # the cap is named before a bad scalar is
                with pytest.raises(_capi.MolannHipError) as err:
                    plan.value_and_opes_f64(x9, [], [], table[0], table[1], s, None, SCALE, 1.0, 1e-3, cutoff, y, v, dx)
                assert err.value.code == _capi.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (y, v, dx)), "a refusal launched"


# ---- 6. relations to value_and_vjp -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [("C3", 65), ("P1", 9), ("C3_angles", 65)])
def test_y_and_dx_of_value_and_vjp(name, n, hip_device):
    if name == "C3_angles":
        w, case, model = vr._c3_angles(hip_device, bond=True)
        args, d_out = (case.feats, True, case.align), 3
        period = torch.tensor([TWO_PI, TWO_PI, 0.0], dtype=torch.float64)
    else:
        w, model, args = vv._shared(name, hip_device)
        d_out = w.out_dim()
        period = vh._period_row(d_out, 1.1, 2)
    x = w.make_frames(n, seed=90).double().to(hip_device)
    x_tab = w.make_frames(65, seed=92).double().to(hip_device)
    xx, y_ref = vr._reference_y(model, *args, x)
    _, y_tab = vr._reference_y(model, *args, x_tab)
    table, norm = _table(y_ref, y_tab, period, 45, True, 91, (4.0,))
    (y, v, dx), _, _ = _check(model, xx, y_ref, x, table, period, norm, 1e-3, 4.0, name)
    on = tuple(t.to(hip_device) for t in table)
    yv, dxv = vr._vjp(model, x, _cotangent(y, on, period.to(hip_device), norm, 1e-3, 4.0))
    assert torch.equal(y, yv)
    ed, sd = float((dx - dxv).abs().max()), max(1e-3, float(dxv.abs().max()))
    print("%s: dx against value_and_vjp on torch's cotangent %.3e (scale %.3g)" % (name, ed, sd))
    assert ed <= 1e-9 * sd


# ---- 7. determinism, independence --------------------------------------------------------------------------------------------------
def _seeded_table(d, n_kernels, seed, per_kernel=True):
    c, h, s = vh._seeded_table(d, n_kernels, seed, per_kernel)
    return (c, h.abs(), s), _norm(h.abs())


def test_two_calls_give_the_same_bits(hip_device):
    w, model, _ = vv._shared("C3", hip_device)
    n, d = 1025, w.out_dim()
    x = w.make_frames(n, seed=41).double().to(hip_device)
    (table, norm), period = _seeded_table(d, 77, 42), vh._period_row(d, 1.1, 2)
    a, _ = _call(model, x, table, period, norm, 1e-3, 4.0)
    a = [t.clone() for t in a]
    b, info = _call(model, x, table, period, norm, 1e-3, 4.0)
    assert KERNEL in info, info
    assert all(torch.equal(s, t) for s, t in zip(a, b)) and all(bool(torch.isfinite(t).all()) for t in a)
    assert float(a[2].abs().max()) > 0.0 and float((a[1] - SCALE * math.log(1e-3)).abs().max()) > 0.0


@pytest.mark.parametrize("name", ["C3", "small7"])
def test_a_frame_alone_has_its_bits_in_the_batch(name, hip_device):
    """Frame f alone and inside a batch of 65: another block, another slot of the block, the same bits (G = 32 on C3, 8 on small7)."""
    if name == "C3":
        w, model, _ = vv._shared("C3", hip_device)
        x, d = w.make_frames(65, seed=43).double().to(hip_device), w.out_dim()
    else:
        case = vh._small_case(7, True, False)
        model = case.build(hip_device).double().requires_grad_(False)
        x, d = case.frames(65, seed=43, dev=CPU).double().to(hip_device), 6
    (table, norm), period = _seeded_table(d, 45, 44), vh._period_row(d, 1.1, 2)
    full, _ = _call(model, x, table, period, norm, 1e-3, 4.0)
    full = [t.clone() for t in full]
    for f in (0, 9, 33, 64):
        one, _ = _call(model, x[f:f + 1].contiguous(), table, period, norm, 1e-3, 4.0)
        assert all(torch.equal(a[0], b[f]) for a, b in zip(one, full)), f


# ---- 8. no cutoff is the limit of a large one ------------------------------------------------------------------------------------------
def test_cutoff_neutrality(hip_device):
    """cutoff=None against a finite cutoff larger than every sqrt(q) of the case: nothing is dropped, so the two differ by the c0 = exp(-c^2 /
    2) the finite one subtracts from every kernel - u moves by c0 sum(w) / norm, V by scale times that over u, dx by that fraction of
    itself - and by nothing else.  At cutoff 40 c0 = exp(-800) underflows to 0 (and a kernel past 40 widths adds exp(-800) = 0 either
    way): bit for bit."""
    w, model, args = vv._shared("C3", hip_device)
    n, d = 65, w.out_dim()
    x = w.make_frames(n, seed=47).double().to(hip_device)
    x_tab = w.make_frames(65, seed=48).double().to(hip_device)
    period = vh._period_row(d, 1.1, 3)
    xx, y_ref = vr._reference_y(model, *args, x)
    _, y_tab = vr._reference_y(model, *args, x_tab)
    table, norm = _table(y_ref, y_tab, period, 40, True, 49, ())
    assert math.exp(-0.5 * 40.0 * 40.0) == 0.0
    none, _ = _call(model, x, table, period, norm, 1e-3, None)
    none = [t.clone() for t in none]
    at40, _ = _call(model, x, table, period, norm, 1e-3, 40.0)
    assert all(torch.equal(a, b) for a, b in zip(none, at40))
    p_ref, q = _density(y_ref.detach(), *table, period, None)
    reach = float(q.max().sqrt())
    cutoff = max(6.0, math.ceil(reach) + 1.0)
    assert cutoff < 38.0, "the case's farthest pair is too far for a finite c0"
    c0 = math.exp(-0.5 * cutoff * cutoff)
    shift = c0 * float(table[1].sum()) / norm / float((p_ref / norm + 1e-3).min())      # the largest relative move of u
    cut, _ = _call(model, x, table, period, norm, 1e-3, cutoff)
    assert torch.equal(cut[0], none[0])
    ev, ed = float((cut[1] - none[1]).abs().max()), float((cut[2] - none[2]).abs().max())
    print("cutoff %.0f against none: c0 %.3e, u moves by %.3e of itself, bias by %.3e, dx by %.3e" % (cutoff, c0, shift, ev, ed))
    assert ev <= 2.0 * SCALE * shift + 4e-16 * float(none[1].abs().max())
    assert ed <= (2.0 * shift + 4e-16) * float(none[2].abs().max())


# ---- 9. NaN isolation, a frame outside every cutoff ---------------------------------------------------------------------------------
@pytest.mark.parametrize("cutoff", [4.0, None], ids=["cutoff4", "no_cutoff"])
def test_nan_poisons_only_its_frame(cutoff, hip_device):
    w, model, _ = vv._shared("P1", hip_device)
    n, bad, d = 70, 33, w.out_dim()
    x = w.make_frames(n, seed=61).double().to(hip_device)
    (table, norm), period = _seeded_table(d, 45, 62), vh._period_row(d, 1.1, 2)
    names = ("out", "bias", "grad_x")
    clean, _ = _call(model, x, table, period, norm, 1e-3, cutoff)
    clean = dict((k, t.clone()) for k, t in zip(names, clean))
    xb = x.clone()
    xb[bad, 5] = NAN
    got, _ = _call(model, xb, table, period, norm, 1e-3, cutoff)
    got = dict(zip(names, got))
    complaints = isolation.keep_rows_equal(clean, got, [bad], names)
    assert not complaints, complaints
    assert bool(torch.isfinite(clean["bias"]).all()) and bool(torch.isfinite(clean["grad_x"]).all())
    assert bool(torch.isnan(got["out"][bad]).all()) and bool(torch.isnan(got["bias"][bad])) and bool(torch.isnan(got["grad_x"][bad]).any())


def test_a_frame_outside_every_cutoff(hip_device):
    """Kernels half a width from the reference outputs of frames 1.., a twentieth of the outputs' spread wide: frame 0 is outside every
    kernel's cutoff of 4 (asserted on the reference), every other frame inside its own.  Frame 0: bias = scale log(epsilon) up to log's rounding, dx 0
    exactly; the other frames against the oracle."""
    w, model, args = vv._shared("C3", hip_device)
    n, d, cutoff, epsilon = 9, w.out_dim(), 4.0, 1e-3
    x = w.make_frames(n, seed=65).double().to(hip_device)
    xx, y_ref = vr._reference_y(model, *args, x)
    yr = y_ref.detach()
    sigma = 0.05 * yr.std(dim=0).clamp(min=1e-3)
    table = (yr[1:] + 0.5 * sigma, torch.linspace(0.3, 1.1, n - 1, dtype=torch.float64), sigma)
    norm = _norm(table[1])
    _, q = _density(yr, *table, None, cutoff)
    assert float(q[0].min()) >= cutoff * cutoff + 1e-6 and bool((q[1:].min(dim=1).values < 2.5).all())
    _conditions(y_ref, table, None, cutoff)
    (y, v, dx), want, _ = _check(model, xx, y_ref, x, table, None, norm, epsilon, cutoff, "frame 0 outside every cutoff")
    assert abs(float(v[0]) - SCALE * math.log(epsilon)) <= 1e-14 * abs(SCALE * math.log(epsilon))
    assert bool((dx[0] == 0).all()) and float(want[2][1:].abs().amax(dim=(1, 2)).min()) > 1e-3


# ---- 10. into=, conversions, refusals, caller buffers --------------------------------------------------------------------------------
def test_into_conversions_and_refusals(hip_device):
    w, model, _ = vv._shared("C3", hip_device)
    pre = model.preprocessing_layer
    n, d, H = 5, w.out_dim(), 11
    x = w.make_frames(n, seed=51).double().to(hip_device)
    (table, norm) = _seeded_table(d, H, 52, per_kernel=False)
    c, h, s = (t.to(hip_device) for t in table)
    eps = 1e-3
    y, v, dx = (t.clone() for t in model.value_and_opes(x, c, h, s, SCALE, norm, eps, 4.0))
    new = lambda *shape: torch.full(shape, NAN, dtype=torch.float64, device=hip_device)       # noqa: E731
    y2, v2, dx2 = new(n, d), new(n), new(n, w.n_atoms, 3)
    r = model.value_and_opes(x, c, h, s, SCALE, norm, eps, cutoff=4.0, into=(y2, v2, dx2))
    torch.cuda.synchronize()
    assert r[0] is y2 and r[1] is v2 and r[2] is dx2
    assert torch.equal(y2, y) and torch.equal(v2, v) and torch.equal(dx2, dx)
    assert float((v - SCALE * math.log(eps)).abs().max()) > 0.0
    # a float height and width, sequences, an int scale and cutoff, a float32 table: converted
    k1 = model.value_and_opes(x, c, 0.7, 0.9, 2, norm, eps, 4)
    k2 = model.value_and_opes(x, c.tolist(), [0.7] * H, torch.full((H, d), 0.9, dtype=torch.float64, device=hip_device), 2.0, norm, eps, 4.0,
                              period=[0.0] * d)
    assert all(torch.equal(a, b) for a, b in zip(k1, k2))
    k3 = model.value_and_opes(x, c.float(), 0.7, 0.9, 2.0, norm, eps, 4.0)
    assert k3[1].dtype == torch.float64 and float((k3[1] - k1[1]).abs().max()) <= 1e-4 * max(1.0, float(k1[1].abs().max()))
    # cutoff=None, left out, and +inf are one call
    k4, k5, k6 = (model.value_and_opes(x, c, h, s, SCALE, norm, eps, **kw) for kw in (dict(cutoff=None), dict(), dict(cutoff=INF)))
    assert all(torch.equal(a, b) and torch.equal(a, e) for a, b, e in zip(k4, k5, k6))
    # the remembered read-back of a device sigma is value_and_hills': the same tensor keeps the key
    model.value_and_opes(x, c, h, s, SCALE, norm, eps)
    key = model.__dict__["_sigma_key"]
    model.value_and_opes(x, c, h, s, SCALE, norm, eps)
    assert model.__dict__["_sigma_key"] is key
    # features only (4 columns on C3): the same method on the preprocessing layer, a graph is never recorded
    dp = pre.output_dimension()
    assert dp <= 8
    f, vf, dxf = pre.value_and_opes(x.clone().requires_grad_(True), [[0.0] * dp], 1.0, 1.0, 1.0, 1.0, 0.5)
    torch.cuda.synchronize()
    assert KERNEL in ann.last_launch_info(pre) and not (f.requires_grad or vf.requires_grad or dxf.requires_grad)
    assert float((vf - torch.log(torch.exp(-0.5 * (f * f).sum(dim=1)) + 0.5)).abs().max()) <= 1e-12
    y3, v3, dx3 = new(n, d), new(n), new(n, w.n_atoms, 3)
    bad_calls = [
        (TypeError, dict(into=(y3, dx3))), (TypeError, dict(into=(y3.float(), v3, dx3))), (ValueError, dict(into=(y3[:4], v3, dx3))),
        (ValueError, dict(into=(y3, v3.cpu(), dx3))), (ValueError, dict(into=(y3, v3, dx3.transpose(1, 2)))),
        (ValueError, dict(centers=c[:, :-1])), (ValueError, dict(centers=c.cpu())), (ValueError, dict(heights=h[:-1])),
        (ValueError, dict(sigma=s[:-1])), (ValueError, dict(sigma=-s)), (ValueError, dict(sigma=0.0)),
        (ValueError, dict(period=torch.ones(d + 1, dtype=torch.float64, device=hip_device))),
        (TypeError, dict(heights=torch.ones(H, dtype=torch.int64, device=hip_device))),
        (ValueError, dict(scale=NAN)), (ValueError, dict(scale=INF)), (ValueError, dict(norm=0.0)), (ValueError, dict(norm=INF)),
        (ValueError, dict(epsilon=0.0)), (ValueError, dict(epsilon=-1.0)), (ValueError, dict(cutoff=0.0)), (ValueError, dict(cutoff=NAN)),
        (TypeError, dict(norm=torch.tensor(1.0))), (TypeError, dict(scale=None)),
    ]
    for exc, changes in bad_calls:
        kw = dict(centers=c, heights=h, sigma=s, scale=SCALE, norm=norm, epsilon=eps, cutoff=4.0, into=(y3, v3, dx3))
        kw.update(changes)
        with pytest.raises(exc):
            model.value_and_opes(x, **kw)
    with pytest.raises(TypeError, match="float64"):
        model.value_and_opes(x.float(), c, h, s, SCALE, norm, eps)
    with pytest.raises(NotImplementedError, match=ROUTE):
        model.value_and_opes(x.cpu(), c.cpu(), h.cpu(), s.cpu(), SCALE, norm, eps)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (y3, v3, dx3)), "a refusal launched"
    empty = model.value_and_opes(x[:0], c, h, s, SCALE, norm, eps)
    assert [tuple(t.shape) for t in empty] == [(0, d), (0,), (0, w.n_atoms, 3)]


def test_offset_caller_buffers_inside_guard_bands(hip_device):
    """The C entry on buffers carved out of an arena, every one at another residue of 16 bytes, between guard bands: the outputs have
    the bits of the call on fresh tensors, no band and no input is written."""
    w, model, _ = vv._shared("C3", hip_device)
    n, d, H = 65, w.out_dim(), 45
    x = w.make_frames(n, seed=55).double().to(hip_device)
    (table, norm), period = _seeded_table(d, H, 56), vh._period_row(d, 1.1, 2)
    c, h, s, p = (t.to(hip_device) for t in table + (period,))
    entry, lins = model._fast_state(x)["entry"](), [m for m in model.ann_layers if isinstance(m, torch.nn.Linear)]
    fresh = ann._one_launch_ctypes(ann._OPES, entry, x, (c, h, s, p, SCALE, norm, 1e-3, 4.0), None, None, (n, w.n_atoms, 3), d, lins,
                                   rb._align_layer(model))
    torch.cuda.synchronize()
    assert entry.plan.last_launch_info().startswith(KERNEL)
    arena = pl.Arena(hip_device, capacity=8 << 20)
    inputs = (("x", x), ("centers", c), ("heights", h), ("sigma", s), ("period", p))
    outputs = (("out", (n, d)), ("bias", (n,)), ("grad_x", (n, w.n_atoms, 3)))
    views = {}
    for i, (name, data) in enumerate(inputs):
        views[name] = arena.carve(name, data.shape, torch.float64, (i + 1) % 2, data=data)
    for i, (name, shape) in enumerate(outputs):
        views[name] = arena.carve(name, shape, torch.float64, i % 2)
    assert len(set(t.data_ptr() % 16 for t in views.values())) == 2
    with torch.cuda.device(hip_device):
        W, B = [lin.weight.detach().contiguous() for lin in lins], [lin.bias.detach().contiguous() for lin in lins]
        rc = _capi.lib().molann_value_and_opes_f64(entry.plan._handle, views["x"].data_ptr(), n, *_capi._layer_pointers(W, B), views["centers"].data_ptr(),
                                                   views["heights"].data_ptr(), H, views["sigma"].data_ptr(), d, views["period"].data_ptr(), SCALE, norm,
                                                   1e-3, 4.0, views["out"].data_ptr(), views["bias"].data_ptr(), views["grad_x"].data_ptr(),
                                                   torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    assert rc == 0
    assert arena.check() == [] and arena.inputs_changed() == []
    assert all(pl.same_bits(views[name], want) for (name, _), want in zip(outputs, fresh))
    assert bool(torch.isfinite(fresh[2]).all()) and float(fresh[2].abs().max()) > 0.0


# ---- 11. the dispatcher operators, one launch, the C entry's own refusals --------------------------------------------------------------
def test_scripted_model_and_operators(tmp_path, hip_device):
    import warnings
    w, model, _ = vv._shared("C3", hip_device)
    n, d = 65, w.out_dim()
    x = w.make_frames(n, seed=71).double().to(hip_device)
    (table, norm) = _seeded_table(d, 45, 72)
    c, h, s = (t.to(hip_device) for t in table)
    period = vh._period_row(d, 1.1, 2).to(hip_device)
    want = model.value_and_opes(x, c, h, s, SCALE, norm, 1e-3, 4.0, period)
    torch.cuda.synchronize()
    info = model.last_launch_info()
    assert info.startswith(KERNEL + " (values + opes in one launch; ") and info.count("_kernel") == 1 and "||" not in info, info
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.jit.script(model).save(str(tmp_path / "c3_f64.pt"))
    loaded = torch.jit.load(str(tmp_path / "c3_f64.pt"), map_location=hip_device)
    ws = [lin.weight for lin in loaded.linears.children()]
    bs = [lin.bias for lin in loaded.linears.children()]
    desc = list(loaded.desc)
    handle = torch.ops.molann.register_desc(desc)
    by_handle = torch.ops.molann.value_and_opes_h(x, handle, loaded.ref_x, ws, bs, c, h, s, period, SCALE, norm, 1e-3, 4.0, [])
    by_desc = torch.ops.molann.value_and_opes(x, desc, loaded.ref_x, ws, bs, c, h, s, period, SCALE, norm, 1e-3, 4.0, [])
    torch.cuda.synchronize()
    info = torch.ops.molann.launch_info(desc, hip_device.index)
    assert info.count(KERNEL) == 1 and info.count("_kernel") == 1, info
    assert len(by_handle) == 3 and len(by_desc) == 3
    assert all(torch.equal(a, b) for a, b in zip(by_handle, want)) and all(torch.equal(a, b) for a, b in zip(by_desc, want))
    assert float((want[1] - SCALE * math.log(1e-3)).abs().max()) > 0.0 and float(want[2].abs().max()) > 0.0
    plain = torch.ops.molann.value_and_opes(x, desc, loaded.ref_x, ws, bs, c[:0], h[:0], s[0], None, SCALE, norm, 1e-3, INF, [])
    assert all(torch.equal(a, b) for a, b in zip(plain, model.value_and_opes(x, c[:0], h[:0], s[0], SCALE, norm, 1e-3)))
    with pytest.raises(ValueError, match="cutoff"):
        torch.ops.molann.value_and_opes(x, desc, loaded.ref_x, ws, bs, c, h, s, period, SCALE, norm, 1e-3, 0.0, [])


def test_the_c_entrys_return_codes(hip_device):
    """The four scalars are looked at after everything molann_value_and_hills_f64 looks at, each answered with MOLANN_E_DESC, and nothing
    is launched on a refusal."""
    x = wl.get_workload("C3").make_frames(3, seed=91).double().to(hip_device)
    with torch.cuda.device(hip_device):
        p = _capi.Plan(22, features=[(wl.BOND, [0, 1])])
        assert p.supports_value_and_opes_f64()
        new = lambda *shape: torch.full(shape, NAN, dtype=torch.float64, device=hip_device)       # noqa: E731
        y, v, dx = new(3, 1), new(3), new(3, 22, 3)
        one = torch.ones(3, dtype=torch.float64, device=hip_device)          # [3]: room for a misaligned row of 1
        p.value_and_opes_f64(x, [], [], one[:1].reshape(1, 1), one[:1], one[:1], None, 1.0, 1.0, 0.5, None, y, v, dx)
        torch.cuda.synchronize()
        assert p.last_launch_info().startswith(KERNEL)
        bond = (x[:, 0] - x[:, 1]).norm(dim=1)
        assert float((y[:, 0] - bond).abs().max()) <= 1e-12 and float((v - torch.log(torch.exp(-0.5 * (bond - 1.0) ** 2) + 0.5)).abs().max()) <= 1e-12
        y.fill_(NAN)
        v.fill_(NAN)
        dx.fill_(NAN)
        pa = _capi.Plan(22, align_idx=[0, 1, 2, 3], ref_x=torch.zeros(4, 3))     # no items: nothing to bias
        assert not pa.supports_value_and_opes_f64()
        L, stream = _capi.lib(), torch.cuda.current_stream().cuda_stream
        good = dict(scale=2.25, norm=1.0, epsilon=1e-3, cutoff=4.0)

        def raw(plan=p, centers=one.data_ptr(), n_kernels=1, sigma_stride=0, period=None, **scalars):
            a = dict(good)
            a.update(scalars)
            return L.molann_value_and_opes_f64(plan._handle, x.data_ptr(), 3, None, None, centers, one.data_ptr(), n_kernels, one.data_ptr(), sigma_stride,
                                               period, a["scale"], a["norm"], a["epsilon"], a["cutoff"], y.data_ptr(), v.data_ptr(), dx.data_ptr(), stream)

        bad = [dict(scale=NAN), dict(scale=INF), dict(scale=-INF), dict(norm=NAN), dict(norm=INF), dict(norm=0.0), dict(norm=-1.0),
               dict(epsilon=NAN), dict(epsilon=INF), dict(epsilon=0.0), dict(epsilon=-1e-3), dict(cutoff=NAN), dict(cutoff=0.0), dict(cutoff=-4.0),
               dict(cutoff=-INF)]
        for scalars in bad:
            assert raw(**scalars) == _capi.E_DESC, scalars
            # what comes before the scalars keeps its code
            assert raw(plan=pa, **scalars) == _capi.E_STAGE and raw(centers=None, **scalars) == _capi.E_NULL, scalars
            assert raw(centers=one.data_ptr() + 4, **scalars) == _capi.E_ALIGNMENT and raw(period=one.data_ptr() + 4, **scalars) == _capi.E_ALIGNMENT
            assert L.molann_value_and_opes_f64(None, x.data_ptr(), 3, None, None, None, None, 0, None, 0, None, *[dict(good, **scalars)[k] for k in good],
                                               y.data_ptr(), v.data_ptr(), dx.data_ptr(), stream) == _capi.E_NULL
            assert raw(n_kernels=-1, **scalars) == _capi.E_DESC and raw(sigma_stride=2, **scalars) == _capi.E_DESC
        assert raw(n_kernels=-1) == _capi.E_DESC and raw(sigma_stride=2) == _capi.E_DESC and raw(sigma_stride=-1) == _capi.E_DESC
        # n_frames == 0 returns before anything is looked at, bad scalars included
        assert L.molann_value_and_opes_f64(p._handle, None, 0, None, None, None, None, 5, None, 3, None, NAN, -1.0, 0.0, -1.0, None, None, None, stream) == 0
        torch.cuda.synchronize()
        assert all(bool(torch.isnan(t).all()) for t in (y, v, dx)), "a refusal launched"
        assert raw(cutoff=INF) == 0 and raw(centers=one.data_ptr() + 8) == 0 and raw(scale=-2.25) == 0 and raw(scale=0.0) == 0
        torch.cuda.synchronize()
        assert bool(torch.isfinite(v).all())
