"""Float64 values, a metadynamics bias on them - a sum of Gaussian hills - and its gradient in ONE launch (molann_value_and_hills_f64 ->
frames_value_hills_f64_kernel): V = sum_h w_h exp(-1/2 sum_k (d_hk / sigma_hk)^2) with d_h = y - c_h wrapped for periodic outputs,
against float64 autograd on the CPU through the oracle's preprocessing, a copy of the head and the formula in torch (torch.round has
zero gradient, which is the derivative of the wrap almost everywhere).  Bounds, the float64 family's: y within 1e-10 max(1, |y|max),
the bias within 1e-10 max(1, |V|max), dx within 1e-9 max(1e-3, |dx|max).

The hill tables are built from the REFERENCE's y, never from the code under test (`_hill_table`): sigma_k is 0.3-0.6 of the spread of
column k over the reference outputs of a separate seeded 65-frame batch, 0.05-0.15 P for a periodic column; the odd hills' centres are
rows of that batch, the even hills' centres the batch's own reference outputs, frame by frame - in 8 dimensions no row of another batch
comes within a width of a frame by chance - and both get noise of the width's size; periodic centres are shifted by whole periods in
[-2, 2]; heights are in [0.2, 1.2], one of them negative; hill 1 of a table of two or more is put far from frame 0.  The builder asserts on the reference values of every call: as many frames as
can be (half of them, or one for every two hills where the table is shorter than that) have a hill with q_h < 2, so no test passes on
zeros; no periodic (frame, hill, column) lies within 1e-9 P of the wrap's seam |d| = P / 2, so none trips on the kink; and every test
case asserts on the flag the builder returns that some (frame, hill) pair of its calls has q_h > 50 (one pair cannot be near and far
at once; with widths per hill and two hills or more every single call has such a pair, by hill 1)."""

import copy
import math

import pytest
import torch

import test_gpu_random_backward as rb
import test_gpu_value_and_restraint_f64 as vr
import test_gpu_value_and_vjp_f64 as vv
from molann_amd import _capi, ann, workloads as wl
from molann_amd.ann import MolANN, create_sequential_nn
from oracle import molann_oracle as mo

pytestmark = pytest.mark.gpu
KERNEL = "frames_value_hills_f64_kernel"
VJP_KERNEL = "frames_value_vjp_f64_kernel"
RESTRAINT_KERNEL = "frames_value_restraint_f64_kernel"
TWO_PI = 2.0 * math.pi
NAN = float("nan")
CPU = torch.device("cpu")


def _wrapped(y, centers, period):
    """d[n, H, d] of the issue's formula, in torch: differentiable in y."""
    d = y[:, None, :] - centers[None, :, :]
    if period is not None:
        P = torch.where(period > 0, period, torch.ones_like(period))
        d = torch.where(period > 0, d - P * torch.round(d / P), d)
    return d


def _bias(y, centers, heights, sigma, period):
    """(V [n], q [n, H]) of the issue's formula, in torch: differentiable in y."""
    s = _wrapped(y, centers, period) / sigma
    q = 0.5 * (s * s).sum(dim=2)
    return (heights * torch.exp(-q)).sum(dim=1), q


def _cotangent(y, centers, heights, sigma, period):
    """dV/dy [n, d] of the issue's formula, in torch on y's device."""
    s = _wrapped(y, centers, period) / sigma
    g = heights * torch.exp(-0.5 * (s * s).sum(dim=2))
    return -(g[:, :, None] * s / sigma).sum(dim=1)


def _hill_table(y_ref, y_tab, period, n_hills, per_hill, seed):
    """((centers [H, d], heights [H], sigma [d] or [H, d]), far) on the CPU for reference outputs y_ref of the batch and y_tab of the
    separate 65-frame batch, with the conditions of the module's docstring asserted; far: some (frame, hill) pair has q_h > 50."""
    y_ref, y_tab = y_ref.detach(), y_tab.detach()
    (n, d), H = y_ref.shape, n_hills
    g = torch.Generator().manual_seed(seed)
    rand = lambda *shape: torch.rand(shape, generator=g, dtype=torch.float64)      # noqa: E731
    periodic = period > 0
    spread = y_tab.std(dim=0).clamp(min=1e-3) if y_tab.shape[0] > 1 else torch.ones(d, dtype=torch.float64)
    u = rand(H, d) if per_hill else rand(d)
    sigma = torch.where(periodic, (0.05 + 0.10 * u) * period, (0.3 + 0.3 * u) * spread)
    h = torch.arange(H)
    base = torch.where((h % 2 == 0)[:, None], y_ref[(h // 2) % n], y_tab[(h * 7 + seed) % y_tab.shape[0]])
    m = torch.randint(-2, 3, (H, d), generator=g).double() * periodic
    centers = base + (rand(H, d) - 0.5) * sigma
    if H >= 2:      # hill 1 is put far from frame 0: 0.45 P away (at the narrowest width where the widths are per hill), 11 widths where not periodic
        if per_hill:
            sigma[1] = torch.where(periodic, 0.05 * period, sigma[1])
        centers[1] = y_ref[0] + torch.where(periodic, 0.45 * period, 11.0 * (sigma[1] if per_hill else sigma))
    centers = centers + m * period
    heights = 0.2 + rand(H)
    if H > 0:
        heights[H // 2] = -heights[H // 2]
    if H == 0:
        return (centers, heights, sigma), False
    # the conditions, on the reference values
    _, q = _bias(y_ref, centers, heights, sigma, period)
    near = int((q.min(dim=1).values < 2.0).sum())
    assert near >= min((n + 1) // 2, (H + 1) // 2), "too few frames have a hill with q < 2: %d of %d (H = %d)" % (near, n, H)
    far = bool((q > 50.0).any())
    raw = (y_ref[:, None, :] - centers[None, :, :]) / torch.where(periodic, period, torch.ones_like(period))
    turn = (raw - torch.round(raw)).abs()[:, :, periodic]
    assert turn.numel() == 0 or float((0.5 - turn).abs().min()) >= 1e-9, "a periodic element within 1e-9 P of the wrap's seam"
    return (centers, heights, sigma), far


def _oracle(xx, y, centers, heights, sigma, period):
    """(y, V, dV/dx) by float64 autograd of the formula."""
    v, _ = _bias(y, centers, heights, sigma, period)
    (gx,) = torch.autograd.grad(v.sum(), xx)
    return y.detach(), v.detach(), gx


def _close(got, want, what):
    (y, v, dx), (y_want, v_want, gx_want) = got, want
    assert y.dtype == torch.float64 and v.dtype == torch.float64 and dx.dtype == torch.float64
    assert y.shape == y_want.shape and v.shape == v_want.shape and dx.shape == gx_want.shape
    ey, ev, ed = (float((a.detach().cpu() - b).abs().max()) for a, b in ((y, y_want), (v, v_want), (dx, gx_want)))
    sy, sv, sd = max(1.0, float(y_want.abs().max())), max(1.0, float(v_want.abs().max())), max(1e-3, float(gx_want.abs().max()))
    print("%s: y err %.3e (scale %.3g), bias err %.3e (scale %.3g), dx err %.3e (scale %.3g)" % (what, ey, sy, ev, sv, ed, sd))
    assert ey <= 1e-10 * sy, (what, "y", ey, sy)
    assert ev <= 1e-10 * sv, (what, "bias", ev, sv)
    assert ed <= 1e-9 * sd, (what, "dx", ed, sd)


def _info(model):
    return model.last_launch_info() if isinstance(model, MolANN) else ann.last_launch_info(model)


def _call(model, x, centers, heights, sigma, period=None, into=None):
    """((y, bias, dx), launch info) of the module's method, arguments moved to x's device."""
    on = lambda t: None if t is None else t.to(x.device)       # noqa: E731
    out = model.value_and_hills(x, on(centers), on(heights), on(sigma), on(period), into=into)
    torch.cuda.synchronize()
    return out, _info(model)


def _check(model, oracle_args, x, x_tab, period, n_hills, per_hill, seed, what):
    """One model, batch and table size against the oracle; returns the device results, the launch info, the table and the builder's
    flag (some pair has q_h > 50)."""
    xx, y_ref = vr._reference_y(model, *oracle_args, x)
    _, y_tab = vr._reference_y(model, *oracle_args, x_tab)
    table, far = _hill_table(y_ref, y_tab, period, n_hills, per_hill, seed)
    p = period if bool((period > 0).any()) else None
    want = _oracle(xx, y_ref, *table, period)
    assert n_hills == 0 or float(want[1].abs().max()) > 0.05 and float(want[2].abs().max()) > 1e-3, "the reference is (nearly) zero"
    got, info = _call(model, x, *table, p)
    assert info.startswith(KERNEL + " (values + hills in one launch; ") and info.count("_kernel") == 1, info
    _close(got, want, what)
    return got, info, table, far


def _period_row(d, value, every=1):
    p = torch.zeros(d, dtype=torch.float64)
    p[::every] = value
    return p


# ---- 1. every lane group -------------------------------------------------------------------------------------------------------
def _small_case(n_inp, aligned, head):
    """vv._small_case; features only it loses its two position items, whose 6 columns take it past the kernel's 8 outputs (6 are
    left: two dihedrals as cos and sin, an angle, a bond), and atom 6 is then touched by the alignment alone."""
    case = vv._small_case(n_inp, [0, 2, 4, 6] if aligned else None, head=head)
    if not head:
        case = rb.Case(case.name, case.xyz, [f for f in case.feats if f[0] != rb.POS], align=case.align, mlp=None)
        assert case.d_feat() == 6
    return case


@pytest.mark.parametrize("n_inp,lanes", [(7, 8), (12, 16), (30, 32), (40, 64)])
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "no_alignment"])
@pytest.mark.parametrize("head", [True, False], ids=["head", "features"])
def test_lane_groups(n_inp, lanes, aligned, head, hip_device):
    """The family's small cases: every lane-group width, with and without an alignment and a head, 1 and 65 frames, tables of 1, G + 1
    and 2 G + 5 hills (a lane with one hill, with none, with several), every second output periodic, widths per hill; untouched
    atoms' rows exactly 0; a shared sigma row and the same row repeated per hill give the same bits."""
    case = _small_case(n_inp, aligned, head)
    model = case.build(hip_device).double().requires_grad_(False)
    d_out = case.mlp[-1] if head else case.d_feat()
    if head:       # the head's widest layer input (the 12 feature columns) asks for at least 16 lanes
        lanes = max(lanes, 16)
    period = _period_row(d_out, 1.3, 2)
    x_tab = case.frames(65, seed=900 + n_inp, dev=CPU).double().to(hip_device)
    untouched = sorted(set(range(n_inp)) - case.touched())
    assert len(untouched) == n_inp - (7 if aligned or head else 6)
    for n in (1, 65):
        x = case.frames(n, seed=n_inp + n, dev=CPU).double().to(hip_device)
        for n_hills in (1, lanes + 1, 2 * lanes + 5):
            (y, v, dx), info, (c, w, s), far = _check(model, (case.feats, case.uav, case.align), x, x_tab, period, n_hills, True, n_inp + n + n_hills,
                                                 (case.name, aligned, head, n, n_hills))
            assert "%d lanes per frame" % lanes in info, info
            assert far or n_hills == 1, "no (frame, hill) pair with q > 50"
            if untouched:
                assert float(dx[:, untouched].abs().max()) == 0.0
        shared, _ = _call(model, x, c, w, s[0], period)
        rows, _ = _call(model, x, c, w, s[:1].expand(n_hills, d_out).contiguous(), period)
        assert all(torch.equal(a, b) for a, b in zip(shared, rows)) and torch.equal(shared[0], y)


# ---- 2. no hills yet ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["C3", "C3_angles"])
def test_no_hills(name, hip_device):
    """The first step of a run: y has value_and_vjp's bits, the bias and dx are zeros written over NaN-filled buffers; a [0, d] table
    through the module, null pointers through ctypes."""
    if name == "C3":
        w, model, _ = vv._shared("C3", hip_device)
        d = w.out_dim()
    else:
        w, _, model = vr._c3_angles(hip_device)
        d = 2
    n = 65
    x = w.make_frames(n, seed=21).double().to(hip_device)
    new = lambda *shape: torch.full(shape, NAN, dtype=torch.float64, device=hip_device)       # noqa: E731
    yv, _, info = vv._call(model, x, torch.ones((n, d), dtype=torch.float64, device=hip_device))
    assert VJP_KERNEL in info
    yv = yv.clone()
    into = (new(n, d), new(n), new(n, w.n_atoms, 3))
    (y, v, dx), info = _call(model, x, torch.zeros((0, d), dtype=torch.float64), torch.zeros(0, dtype=torch.float64), torch.full((d,), 0.3, dtype=torch.float64),
                             into=into)
    assert info.startswith(KERNEL) and y is into[0] and v is into[1] and dx is into[2]
    assert torch.equal(y, yv) and bool((v == 0).all()) and bool((dx == 0).all())
    table = torch.zeros((16, d), dtype=torch.float64, device=hip_device)          # a preallocated table's empty prefix, widths per hill
    (y, v, dx), _ = _call(model, x, table[:0], torch.zeros(16, dtype=torch.float64, device=hip_device)[:0], table[:0] + 1.0, into=tuple(t.fill_(NAN) for t in into))
    assert torch.equal(y, yv) and bool((v == 0).all()) and bool((dx == 0).all())
    # the ctypes way of the module (it brings the plan's ref_x up to date) with no table at all: null pointers, and no widths either
    if isinstance(model, MolANN):
        entry, lins = model._fast_state(x)["entry"](), [m for m in model.ann_layers if isinstance(m, torch.nn.Linear)]
    else:
        vv._feature_plan(model, x)
        entry, lins = model._plans()[("features", x.device.index)], ()
    sigma = torch.full((d,), 0.3, dtype=torch.float64, device=hip_device)
    for widths in (sigma, None):
        y, v, dx = (t.fill_(NAN) for t in into)
        if widths is None:
            with torch.cuda.device(hip_device):
                W, B = [lin.weight.detach().contiguous() for lin in lins], [lin.bias.detach().contiguous() for lin in lins]
                rc = _capi.lib().molann_value_and_hills_f64(entry.plan._handle, x.data_ptr(), n, *_capi._layer_pointers(W, B), None, None, 0, None, 0, None,
                                                            y.data_ptr(), v.data_ptr(), dx.data_ptr(), torch.cuda.current_stream().cuda_stream)
            assert rc == 0
        else:
            ann._one_launch_ctypes(ann._HILLS, entry, x, (None, None, widths, None), y, (v, dx), (n, w.n_atoms, 3), d, lins, rb._align_layer(model))
        torch.cuda.synchronize()
        assert entry.plan.last_launch_info().startswith(KERNEL)
        assert torch.equal(y, yv) and bool((v == 0).all()) and bool((dx == 0).all())


# ---- 3. the cap on the outputs -----------------------------------------------------------------------------------------------------
def test_eight_outputs_run_and_nine_are_refused(hip_device):
    w, model, args = vv._shared("C3", hip_device)
    assert w.out_dim() == 8
    x = w.make_frames(9, seed=31).double().to(hip_device)
    x_tab = w.make_frames(65, seed=32).double().to(hip_device)
    for per_hill in (False, True):
        assert _check(model, args, x, x_tab, _period_row(8, 1.1, 3), 37, per_hill, 33, ("C3", per_hill))[3], "no (frame, hill) pair with q > 50"
    # features only, the positions of three atoms: 9 outputs
    case = rb.Case("pos3", rb._chain(7, 3), [(rb.POS, [1, 3, 5])], align=[0, 2, 4, 6], mlp=None)
    pre = case.build(hip_device).double().requires_grad_(False)
    assert case.d_feat() == 9
    x9 = case.frames(4, seed=34, dev=CPU).double().to(hip_device)
    new = lambda *shape: torch.full(shape, NAN, dtype=torch.float64, device=hip_device)       # noqa: E731
    y, v, dx = new(4, 9), new(4), new(4, 7, 3)
    c, h, s = torch.zeros((3, 9), dtype=torch.float64, device=hip_device), torch.ones(3, dtype=torch.float64, device=hip_device), \
        torch.ones(9, dtype=torch.float64, device=hip_device)
    with pytest.raises(NotImplementedError, match=r"at most 8 outputs \(got 9\); use `model\(x\)`, form the hill sum and its derivative with torch"):
        pre.value_and_hills(x9, c, h, s, into=(y, v, dx))
    plan = vv._feature_plan(pre, x9)
    with torch.cuda.device(hip_device):
        assert plan.supports_value_and_restraint_f64() and plan.supports_value_and_vjp_f64() and not plan.supports_value_and_hills_f64()
        assert _capi.lib().molann_plan_supports_value_and_hills_f64(plan._handle) == 0
        with pytest.raises(_capi.MolannHipError) as err:
            plan.value_and_hills_f64(x9, [], [], c, h, s, None, y, v, dx)
        assert err.value.code == _capi.E_UNSUPPORTED
        with pytest.raises(_capi.MolannHipError) as err:
            plan.value_and_hills_f64(x9, [], [], None, None, s, None, y, v, dx)
        assert err.value.code == _capi.E_UNSUPPORTED
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (y, v, dx)), "a refusal launched"


# ---- 4. dihedral angles, period 2 pi -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65])
@pytest.mark.parametrize("bond", [False, True], ids=["angles", "angles_and_a_bond"])
def test_c3_dihedral_angles(n, bond, hip_device):
    """The two C3 dihedrals as angle values, period 2 pi, alone and with a bond behind them in one period row; besides the builder's
    hills, hills placed near +-pi: a frame on the other side of the seam feels them through the wrap."""
    w, case, model = vr._c3_angles(hip_device, bond=bond)
    d = 3 if bond else 2
    period = torch.tensor([TWO_PI, TWO_PI, 0.0][:d], dtype=torch.float64)
    x = w.make_frames(n, seed=40 + n).double().to(hip_device)
    x_tab = w.make_frames(65, seed=45).double().to(hip_device)
    far = [_check(model, (case.feats, True, case.align), x, x_tab, period, n_hills, per_hill, 41 + n, ("C3 angles", bond, n, n_hills))[3]
           for n_hills, per_hill in ((23, False), (70, True))]
    assert far[1], "no (frame, hill) pair with q > 50"      # one shared row of widths of 0.05-0.15 P seldom reaches q = 50 inside half a period
    xx, y_ref = vr._reference_y(model, case.feats, True, case.align, x)
    # the extended chain's dihedrals lie on both sides of +-pi themselves
    c = torch.tensor([[3.1, -3.1, 4.7], [-3.13, 3.0, 4.6], [math.pi - 1e-3, -math.pi + 1e-3, 4.9], [-3.05, -3.12, 5.0]], dtype=torch.float64)[:, :d]
    heights, sigma = torch.tensor([0.9, -0.4, 1.1, 0.6], dtype=torch.float64), torch.tensor([0.5, 0.6, 0.2][:d], dtype=torch.float64)
    raw = (y_ref.detach()[:, None, :2] - c[None, :, :2]) / TWO_PI
    assert float((0.5 - (raw - torch.round(raw)).abs()).abs().min()) >= 1e-9
    want = _oracle(xx, y_ref, c, heights, sigma, period)
    assert float(want[1].abs().max()) > 0.05
    got, _ = _call(model, x, c, heights, sigma, period)
    _close(got, want, ("C3 angles near pi", bond, n))


# ---- 5. larger frames, stepped-down rows, a long table -------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [("P1", 9), ("C4", 3)])
def test_larger_frames(name, n, hip_device):
    w, model, args = vv._shared(name, hip_device)
    if name == "C4":
        assert w.n_atoms == 5000 and w.mlp_dims == [85, 128, 64, 8]
    x = w.make_frames(n, seed=7).double().to(hip_device)
    x_tab = w.make_frames(17 if name == "C4" else 65, seed=8).double().to(hip_device)
    (_, _, dx), _, _, far = _check(model, args, x, x_tab, _period_row(w.out_dim(), 1.1, 3), 75, True, 60, name)
    assert far, "no (frame, hill) pair with q > 50"
    untouched = sorted(set(range(w.n_atoms)) - {a - 1 for a in w.touched_atoms()})
    if untouched:
        assert float(dx[:, untouched].abs().max()) == 0.0


def _bonds_head(dims, n, n_inp, seed):
    g = torch.Generator().manual_seed(seed)
    head = create_sequential_nn(dims, torch.nn.Tanh()).double().requires_grad_(False)
    for lin in head:
        if isinstance(lin, torch.nn.Linear):
            lin.weight.copy_(torch.randn(lin.weight.shape, generator=g, dtype=torch.float64) / math.sqrt(lin.in_features))
            lin.bias.copy_(0.1 * torch.randn(lin.bias.shape, generator=g, dtype=torch.float64))
    x = torch.randn((n + 65, n_inp, 3), generator=g, dtype=torch.float64) * 2.0
    xx = x[:n].clone().requires_grad_(True)
    y_ref = head(mo.preprocessing_forward(xx, vr.BONDS, False, None, None))
    y_tab = head(mo.preprocessing_forward(x[n:], vr.BONDS, False, None, None))
    return head, xx, y_ref, y_tab


@pytest.mark.parametrize("n_hills", [40, 4099])
def test_stepped_down_rows_and_a_long_table(n_hills, hip_device):
    """The [3, 682, 2] head of the restraint's test (2051 doubles per frame: two waves per block) through ctypes, with a table of 40
    hills and one of 4099 (64 rounds of the lanes and 3 hills more)."""
    dims, block, lds = vr.STEPPED["step_down"]
    n, n_inp = 3, 8
    head, xx, y_ref, y_tab = _bonds_head(dims, n, n_inp, 3)
    period = torch.tensor([0.7, 0.0], dtype=torch.float64)
    (c, h, s), far = _hill_table(y_ref, y_tab, period, n_hills, True, 80)
    assert far, "no (frame, hill) pair with q > 50"
    dev = hip_device
    with torch.cuda.device(dev):
        plan = _capi.Plan(n_inp, features=vr.BONDS, layer_dims=dims, activation=_capi.ACT_TANH)
        assert plan.supports_value_and_hills_f64()
        lins = [m for m in head if isinstance(m, torch.nn.Linear)]
        W, B = [lin.weight.to(dev).contiguous() for lin in lins], [lin.bias.to(dev).contiguous() for lin in lins]
        y, v, dx = (torch.full(sh, NAN, dtype=torch.float64, device=dev) for sh in ((n, 2), (n,), (n, n_inp, 3)))
        plan.value_and_hills_f64(xx.detach().to(dev), W, B, c.to(dev), h.to(dev), s.to(dev), period.to(dev), y, v, dx)
        torch.cuda.synchronize()
        info = plan.last_launch_info()
    assert info == "%s (values + hills in one launch; 64 lanes per frame) grid=%d block=%d lds=%d" % (KERNEL, -(-n // (block // 64)), block, lds), info
    _close((y, v, dx), _oracle(xx, y_ref, c, h, s, period), ("step_down", n_hills))


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
        period = _period_row(d_out, 1.1, 2)
    x = w.make_frames(n, seed=90).double().to(hip_device)
    x_tab = w.make_frames(65, seed=92).double().to(hip_device)
    (y, v, dx), _, (c, h, s), far = _check(model, args, x, x_tab, period, 45, True, 91, name)
    assert far, "no (frame, hill) pair with q > 50"
    on = lambda t: t.to(hip_device)       # noqa: E731
    yv, dxv = vr._vjp(model, x, _cotangent(y, on(c), on(h), on(s), on(period)))
    assert torch.equal(y, yv)
    ed, sd = float((dx - dxv).abs().max()), max(1e-3, float(dxv.abs().max()))
    print("%s: dx against value_and_vjp on torch's cotangent %.3e (scale %.3g)" % (name, ed, sd))
    assert ed <= 1e-9 * sd


# ---- 7. determinism, independence, NaN -----------------------------------------------------------------------------------------------
def _seeded_table(d, n_hills, seed, per_hill=True):
    g = torch.Generator().manual_seed(seed)
    c = torch.randn((n_hills, d), generator=g, dtype=torch.float64)
    h = 0.2 + torch.rand(n_hills, generator=g, dtype=torch.float64)
    h[n_hills // 2] = -h[n_hills // 2]
    s = 0.4 + torch.rand((n_hills, d) if per_hill else (d,), generator=g, dtype=torch.float64)
    return c, h, s


def test_two_calls_give_the_same_bits(hip_device):
    w, model, _ = vv._shared("C3", hip_device)
    n, d = 4097, w.out_dim()
    x = w.make_frames(n, seed=41).double().to(hip_device)
    table, period = _seeded_table(d, 77, 42), _period_row(d, 1.1, 2)
    a, _ = _call(model, x, *table, period)
    a = [t.clone() for t in a]
    b, info = _call(model, x, *table, period)
    assert KERNEL in info, info
    assert all(torch.equal(s, t) for s, t in zip(a, b)) and all(bool(torch.isfinite(t).all()) for t in a)
    assert float(a[1].abs().max()) > 0.0


@pytest.mark.parametrize("name", ["C3", "small7"])
def test_a_frame_alone_has_its_bits_in_the_batch(name, hip_device):
    """Frame f alone and inside a batch of 65: another block, another slot of the block, the same bits (G = 32 on C3, 8 on small7)."""
    if name == "C3":
        w, model, _ = vv._shared("C3", hip_device)
        x, d = w.make_frames(65, seed=43).double().to(hip_device), w.out_dim()
    else:
        case = _small_case(7, True, False)
        model = case.build(hip_device).double().requires_grad_(False)
        x, d = case.frames(65, seed=43, dev=CPU).double().to(hip_device), 6
    table, period = _seeded_table(d, 45, 44), _period_row(d, 1.1, 2)
    full, _ = _call(model, x, *table, period)
    full = [t.clone() for t in full]
    for f in (0, 9, 33, 64):
        one, _ = _call(model, x[f:f + 1].contiguous(), *table, period)
        assert all(torch.equal(a[0], b[f]) for a, b in zip(one, full)), f


def test_nan_poisons_only_its_frame(hip_device):
    w, model, _ = vv._shared("P1", hip_device)
    n, bad, d = 70, 33, w.out_dim()
    x = w.make_frames(n, seed=61).double().to(hip_device)
    table, period = _seeded_table(d, 45, 62), _period_row(d, 1.1, 2)
    (y0, v0, dx0), _ = _call(model, x, *table, period)
    y0, v0, dx0 = y0.clone(), v0.clone(), dx0.clone()
    keep = torch.ones(n, dtype=torch.bool, device=hip_device)
    keep[bad] = False
    xb = x.clone()
    xb[bad, 5] = NAN
    (y, v, dx), _ = _call(model, xb, *table, period)
    assert torch.equal(y[keep], y0[keep]) and torch.equal(v[keep], v0[keep]) and torch.equal(dx[keep], dx0[keep])
    assert bool(torch.isnan(y[bad]).all()) and bool(torch.isnan(v[bad])) and bool(torch.isnan(dx[bad]).any())


# ---- 8. into=, conversions, refusals -------------------------------------------------------------------------------------------------
def test_into_conversions_and_refusals(hip_device):
    w, model, _ = vv._shared("C3", hip_device)
    pre = model.preprocessing_layer
    n, d, H = 5, w.out_dim(), 11
    x = w.make_frames(n, seed=51).double().to(hip_device)
    c, h, s = (t.to(hip_device) for t in _seeded_table(d, H, 52, per_hill=False))
    (y, v, dx), _ = _call(model, x, c, h, s)
    new = lambda *shape: torch.full(shape, NAN, dtype=torch.float64, device=hip_device)       # noqa: E731
    y2, v2, dx2 = new(n, d), new(n), new(n, w.n_atoms, 3)
    r, _ = _call(model, x, c, h, s, into=(y2, v2, dx2))
    assert r[0] is y2 and r[1] is v2 and r[2] is dx2
    assert torch.equal(y2, y) and torch.equal(v2, v) and torch.equal(dx2, dx)
    # a float height and width, sequences, a float32 table: converted
    k1 = model.value_and_hills(x, c, 0.7, 0.9)
    k2 = model.value_and_hills(x, c.tolist(), [0.7] * H, torch.full((H, d), 0.9, dtype=torch.float64, device=hip_device), period=[0.0] * d)
    assert all(torch.equal(a, b) for a, b in zip(k1, k2))
    k3 = model.value_and_hills(x, c.float(), 0.7, 0.9)
    assert k3[1].dtype == torch.float64 and float((k3[1] - k1[1]).abs().max()) <= 1e-5 * max(1.0, float(k1[1].abs().max()))
    assert float(k1[1].abs().max()) > 0.0 or float(v.abs().max()) > 0.0
    # a device sigma is read back once per version of its storage: the same tensor, and views of one table, keep the key
    model.value_and_hills(x, c, h, s)
    key = model.__dict__["_sigma_key"]
    model.value_and_hills(x, c, h, s)
    assert model.__dict__["_sigma_key"] is key
    widths = torch.full((H + 4, d), 0.9, dtype=torch.float64, device=hip_device)
    model.value_and_hills(x, c, h, widths[:H])
    key = model.__dict__["_sigma_key"]
    model.value_and_hills(x, c[:H - 1], h[:H - 1], widths[:H - 1])
    assert model.__dict__["_sigma_key"] is key
    widths[H - 1, 0] = -1.0                                    # written to: looked at again
    with pytest.raises(ValueError, match="sigma"):
        model.value_and_hills(x, c, h, widths[:H])
    # features only (4 columns on C3): the same method on the preprocessing layer, a graph is never recorded
    dp = pre.output_dimension()
    assert dp <= 8
    f, vf, dxf = pre.value_and_hills(x.clone().requires_grad_(True), [[0.0] * dp], 1.0, 1.0)
    torch.cuda.synchronize()
    assert KERNEL in ann.last_launch_info(pre) and not (f.requires_grad or vf.requires_grad or dxf.requires_grad)
    assert float((vf - torch.exp(-0.5 * (f * f).sum(dim=1))).abs().max()) <= 1e-12
    y3, v3, dx3 = new(n, d), new(n), new(n, w.n_atoms, 3)
    bad_calls = [
        (TypeError, dict(into=(y3, dx3))), (TypeError, dict(into=(y3.float(), v3, dx3))), (ValueError, dict(into=(y3[:4], v3, dx3))),
        (ValueError, dict(into=(y3, v3.cpu(), dx3))), (ValueError, dict(into=(y3, v3, dx3.transpose(1, 2)))),
        (ValueError, dict(centers=c[:, :-1])), (ValueError, dict(centers=c.cpu())), (ValueError, dict(heights=h[:-1])),
        (ValueError, dict(sigma=s[:-1])), (ValueError, dict(sigma=s.expand(H + 1, d))),
        (ValueError, dict(period=torch.ones(d + 1, dtype=torch.float64, device=hip_device))),
        (ValueError, dict(sigma=-s)), (ValueError, dict(sigma=0.0)), (ValueError, dict(sigma=[0.5] * (d - 1) + [NAN])),
        (TypeError, dict(heights=torch.ones(H, dtype=torch.int64, device=hip_device))),
    ]
    for exc, changes in bad_calls:
        kw = dict(centers=c, heights=h, sigma=s, into=(y3, v3, dx3))
        kw.update(changes)
        with pytest.raises(exc):
            model.value_and_hills(x, **kw)
    with pytest.raises(TypeError, match="float64"):
        model.value_and_hills(x.float(), c, h, s)
    with pytest.raises(NotImplementedError, match="value_and_vjp"):
        model.value_and_hills(x.cpu(), c.cpu(), h.cpu(), s.cpu())
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (y3, v3, dx3)), "a refusal launched"
    empty = model.value_and_hills(x[:0], c, h, s)
    assert [tuple(t.shape) for t in empty] == [(0, d), (0,), (0, w.n_atoms, 3)]


# ---- 9. the dispatcher operators ---------------------------------------------------------------------------------------------------
def test_scripted_model_and_operators(tmp_path, hip_device):
    import warnings
    w, model, _ = vv._shared("C3", hip_device)
    n, d = 65, w.out_dim()
    x = w.make_frames(n, seed=71).double().to(hip_device)
    c, h, s = (t.to(hip_device) for t in _seeded_table(d, 45, 72))
    period = _period_row(d, 1.1, 2).to(hip_device)
    want = model.value_and_hills(x, c, h, s, period)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.jit.script(model).save(str(tmp_path / "c3_f64.pt"))
    loaded = torch.jit.load(str(tmp_path / "c3_f64.pt"), map_location=hip_device)
    ws = [lin.weight for lin in loaded.linears.children()]
    bs = [lin.bias for lin in loaded.linears.children()]
    desc = list(loaded.desc)
    handle = torch.ops.molann.register_desc(desc)
    by_handle = torch.ops.molann.value_and_hills_h(x, handle, loaded.ref_x, ws, bs, c, h, s, period, [])
    by_desc = torch.ops.molann.value_and_hills(x, desc, loaded.ref_x, ws, bs, c, h, s, period, [])
    torch.cuda.synchronize()
    info = torch.ops.molann.launch_info(desc, hip_device.index)
    assert info.count(KERNEL) == 1 and info.count("_kernel") == 1, info
    assert len(by_handle) == 3 and len(by_desc) == 3
    assert all(torch.equal(a, b) for a, b in zip(by_handle, want)) and all(torch.equal(a, b) for a, b in zip(by_desc, want))
    assert float(want[1].abs().max()) > 0.0
    plain = torch.ops.molann.value_and_hills(x, desc, loaded.ref_x, ws, bs, c[:0], h[:0], s[0], None, [])
    assert all(torch.equal(a, b) for a, b in zip(plain, model.value_and_hills(x, c[:0], h[:0], s[0])))


# ---- 10. one launch, the neighbours untouched, the C entry's own refusals ------------------------------------------------------------
def test_one_launch_and_the_neighbours_untouched(hip_device):
    w, model, _ = vv._shared("C3", hip_device)
    n, d = 64, w.out_dim()
    x = w.make_frames(n, seed=91).double().to(hip_device)
    _, info = _call(model, x, *_seeded_table(d, 5, 92))
    assert info.startswith(KERNEL) and info.count("_kernel") == 1 and "molann_" not in info and "||" not in info, info
    with torch.cuda.device(hip_device):
        p = _capi.Plan(22, features=[(wl.BOND, [0, 1])])
        assert p.supports_value_and_hills_f64()
        new = lambda *shape: torch.full(shape, NAN, dtype=torch.float64, device=hip_device)       # noqa: E731
        y, v, dx = new(3, 1), new(3), new(3, 22, 3)
        x3 = x[:3].contiguous()
        one = torch.ones(3, dtype=torch.float64, device=hip_device)          # [3]: room for a misaligned row of 1
        p.value_and_hills_f64(x3, [], [], one[:1].reshape(1, 1), one[:1], one[:1], None, y, v, dx)
        torch.cuda.synchronize()
        assert p.last_launch_info().startswith(KERNEL)
        bond = (x3[:, 0] - x3[:, 1]).norm(dim=1)
        assert float((y[:, 0] - bond).abs().max()) <= 1e-12 and float((v - torch.exp(-0.5 * (bond - 1.0) ** 2)).abs().max()) <= 1e-12
        y.fill_(NAN)
        pa = _capi.Plan(22, align_idx=[0, 1, 2, 3], ref_x=torch.zeros(4, 3))     # no items: nothing to bias
        assert not pa.supports_value_and_hills_f64()

        def code(plan, **kw):
            args = dict(centers=one[:1], heights=one[:1], sigma=one[:1], n_hills=1, sigma_stride=0)
            args.update(kw)
            with pytest.raises(_capi.MolannHipError) as err:
                plan.value_and_hills_f64(x3, [], [], args["centers"], args["heights"], args["sigma"], None, y, v, dx, n_hills=args["n_hills"],
                                         sigma_stride=args["sigma_stride"])
            return err.value.code

        assert code(pa) == _capi.E_STAGE
        assert code(p, n_hills=-1) == _capi.E_DESC
        assert code(p, sigma_stride=2) == _capi.E_DESC and code(p, sigma_stride=-1) == _capi.E_DESC
        assert code(p, centers=None) == _capi.E_NULL and code(p, heights=None) == _capi.E_NULL
        L, s = _capi.lib(), torch.cuda.current_stream().cuda_stream
        raw = lambda centers, period: L.molann_value_and_hills_f64(p._handle, x3.data_ptr(), 3, None, None, centers, one.data_ptr(), 1,       # noqa: E731
                                                                   one.data_ptr(), 0, period, y.data_ptr(), v.data_ptr(), dx.data_ptr(), s)
        assert raw(one.data_ptr() + 4, None) == _capi.E_ALIGNMENT and raw(one.data_ptr(), one.data_ptr() + 4) == _capi.E_ALIGNMENT
        torch.cuda.synchronize()
        assert bool(torch.isnan(y).all()), "a refusal launched"
        assert raw(one.data_ptr() + 8, None) == 0
        assert L.molann_value_and_hills_f64(p._handle, None, 0, None, None, None, None, 5, None, 3, None, None, None, None, s) == 0
        torch.cuda.synchronize()
    G = torch.ones((n, d), dtype=torch.float64, device=hip_device)
    m32 = wl.build_model(w, hip_device, 0).requires_grad_(False)
    m32.value_and_vjp(x.float(), G.float())
    torch.cuda.synchronize()
    info32 = m32.last_launch_info()
    assert "f64_kernel" not in info32 and "molann_bwd_ring" in info32, info32
    model.value_and_restraint(x, torch.zeros(d, dtype=torch.float64, device=hip_device), 1.0)
    torch.cuda.synchronize()
    assert model.last_launch_info().startswith(RESTRAINT_KERNEL)
    model.value_and_vjp(x, G)
    torch.cuda.synchronize()
    assert model.last_launch_info().startswith(VJP_KERNEL)
