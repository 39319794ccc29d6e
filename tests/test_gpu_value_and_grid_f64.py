"""Float64 values, a bias interpolated from a table over them and its gradient in ONE launch (molann_value_and_grid_f64 ->
frames_value_grid_f64_kernel): V the cubic-convolution (Catmull-Rom) interpolant of a table on a regular grid, one axis per output,
against float64 autograd on the CPU through the oracle's preprocessing, a copy of the head and the formula in torch (floor and the
clamp to a non-periodic range have the gradient the formula states: 0 outside, 1 inside).  Bounds, the float64 family's (the hills
test's `_close`): y within 1e-10 max(1, |y|max), the bias within 1e-10 max(1, |V|max), dx within 1e-9 max(1e-3, |dx|max).

Every grid is derived from the REFERENCE's y of a first forward, never from the code under test (`_grid_from`): a non-periodic axis
spans the 6th-lowest to the 6th-highest reference value, so frames lie below it, above it, in its first and last cell and inside; a
periodic axis is given 0.7 of that span as its period, so frames wrap and some lie in the seam cell.  Every check asserts on the
reference values that the cells it names are hit, that no y_k lies within 1e-9 h_k of a non-periodic range's end (where the
derivative jumps), and that neither the bias nor dx is nearly zero."""

import itertools
import math

import pytest
import torch

import placement
import test_gpu_random_backward as rb
import test_gpu_value_and_hills_f64 as vh
import test_gpu_value_and_restraint_f64 as vr
import test_gpu_value_and_vjp_f64 as vv
from molann_amd import _capi, ann, workloads as wl
from molann_amd.ann import MolANN

pytestmark = pytest.mark.gpu
KERNEL = "frames_value_grid_f64_kernel"
VJP_KERNEL = "frames_value_vjp_f64_kernel"
TWO_PI = 2.0 * math.pi
NAN = float("nan")
CPU = torch.device("cpu")
F64 = torch.float64


# ---- the formula in torch, differentiable in y ---------------------------------------------------------------------------------------
def _axis(y, n, lower, h, periodic):
    """(idx [N, 4], a [N, 4], cell [N], inside [N]) of the issue's axis step for a column y [N]; a's dependence on y is the formula's."""
    u = (y - lower) / h
    if periodic:
        u = u - n * torch.floor(u / n)
        i = torch.clamp(torch.floor(u), max=n - 1).detach()
        inside = torch.ones_like(u, dtype=torch.bool)
    else:
        inside = ((u >= 0) & (u <= n - 1)).detach()
        u = torch.clamp(u, 0, n - 1)
        i = torch.clamp(torch.floor(u), max=n - 2).detach()
    t = u - i
    t2 = t * t
    a = torch.stack([((-t + 2) * t - 1) * t / 2, ((3 * t - 5) * t2 + 2) / 2, ((-3 * t + 4) * t + 1) * t / 2, (t - 1) * t2 / 2], dim=1)
    j = i.long()[:, None] - 1 + torch.arange(4)[None, :]
    idx = j % n if periodic else j.clamp(0, n - 1)
    return idx, a, i.long(), inside


def _interp(y, table, lower, spacing, periodic):
    """(V [N], cells [N, d], inside [N, d]) of the issue's formula for y [N, d] and a CPU table"""
    d = table.dim()
    steps = [_axis(y[:, k], table.shape[k], lower[k], spacing[k], periodic[k]) for k in range(d)]
    view = lambda t, k: t.reshape([t.shape[0]] + [4 if m == k else 1 for m in range(d)])       # noqa: E731
    sub = table[tuple(view(steps[k][0], k) for k in range(d))]
    for k in range(d):
        sub = sub * view(steps[k][1], k)
    return sub.reshape(y.shape[0], -1).sum(dim=1), torch.stack([s[2] for s in steps], dim=1), torch.stack([s[3] for s in steps], dim=1)


def _oracle(xx, y, table, lower, spacing, periodic):
    """((y, V, dV/dx), dV/dy, cells, inside) by float64 autograd of the formula, with the module's conditions asserted"""
    v, cells, inside = _interp(y, table, lower, spacing, periodic)
    gx, gy = torch.autograd.grad(v.sum(), [xx, y], retain_graph=True)
    for k in range(y.shape[1]):
        if not periodic[k]:
            u = (y.detach()[:, k] - lower[k]) / spacing[k]
            assert float(torch.minimum(u.abs(), (u - (table.shape[k] - 1)).abs()).min()) >= 1e-9, "a y within 1e-9 h of a range's end"
            assert bool((gy[:, k][~inside[:, k]] == 0).all()), "the reference's derivative outside the range is not 0"
    return (y.detach(), v.detach(), gx), gy, cells, inside


def _grid_from(y_ref, shape, periodic):
    """(lower, spacing) for reference outputs y_ref [N >= 24, d]: see the module's docstring"""
    lower, spacing = [], []
    for k, n in enumerate(shape):
        s = torch.sort(y_ref.detach()[:, k]).values
        lo, hi = 0.5 * float(s[5] + s[6]), 0.5 * float(s[-7] + s[-6])
        assert hi - lo > 1e-6, "the reference outputs do not spread"
        lower.append(lo)
        spacing.append(0.7 * (hi - lo) / n if periodic[k] else (hi - lo) / (n - 1))
    return lower, spacing


def _cells_hit(cells, inside, shape, periodic):
    """asserts, on the reference, the cells test 1 names"""
    for k, n in enumerate(shape):
        c, ins = cells[:, k], inside[:, k]
        if periodic[k]:
            assert bool((c == n - 1).any()), "no frame in the seam cell of periodic axis %d" % k
            assert bool(((c >= 1) & (c <= n - 2)).any())
        else:
            assert bool(((c == 0) & ins).any()) and bool(((c == n - 2) & ins).any()), "first or last cell of axis %d not hit" % k
            assert bool(((c >= 1) & (c <= n - 3) & ins).any()), "no interior cell of axis %d hit" % k
            assert bool(((c == 0) & ~ins).any()) and bool(((c == n - 2) & ~ins).any()), "no frame outside axis %d on both sides" % k


def _call(model, x, table, lower, spacing, periodic=None, into=None):
    out = model.value_and_grid(x, table, lower, spacing, periodic, into=into)
    torch.cuda.synchronize()
    return out, vh._info(model)


def _seeded_table(shape, seed):
    return 2.0 * torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=F64)


def _nontrivial(want):
    assert float(want[1].abs().max()) > 0.05 and float(want[2].abs().max()) > 1e-3, "the reference is (nearly) zero"


def _check(model, oracle_args, x, table, lower, spacing, periodic, what):
    xx, y_ref = vr._reference_y(model, *oracle_args, x)
    want, gy, cells, inside = _oracle(xx, y_ref, table, lower, spacing, periodic)
    _nontrivial(want)
    got, info = _call(model, x, table.to(x.device), lower, spacing, periodic)
    assert info.startswith(KERNEL + " (values + grid in one launch; ") and info.count("_kernel") == 1, info
    vh._close(got, want, what)
    return got, info, want, cells, inside


# ---- 1. every lane group -------------------------------------------------------------------------------------------------------------
SHAPES = {1: (5,), 2: (4, 7), 3: (6, 4, 5)}
MIXES = {d: list(itertools.product((False, True), repeat=d)) for d in (1, 2, 3)}
FEATURES = {1: [(rb.BOND, [0, 5])], 2: [(rb.ANGLE, [3, 4, 5]), (rb.BOND, [0, 5])], 3: [(rb.DIH, [0, 1, 2, 3]), (rb.BOND, [0, 5])]}


def _lane_case(n_inp, aligned, head, d):
    align = [0, 2, 4, 6] if aligned else None
    if head:
        case = vv._small_case(n_inp, align, head=True)
        case.mlp = [case.d_feat(), 5, d]
        return case
    case = rb.Case("grid%d_%d" % (n_inp, d), rb._chain(n_inp, 3), FEATURES[d], align=align, mlp=None)
    assert case.d_feat() == d
    return case


@pytest.mark.parametrize("n_inp,lanes", [(7, 8), (12, 16), (30, 32), (40, 64)])
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "no_alignment"])
@pytest.mark.parametrize("head", [True, False], ids=["head", "features"])
def test_lane_groups(n_inp, lanes, aligned, head, hip_device):
    """Every lane-group width, with and without an alignment and a head, 1, 2 and 3 outputs, 65 frames and 1; the 16 cases walk
    through every mix of periodic flags; untouched atoms' rows exactly 0; outside a one-axis table dx is exactly 0."""
    turn = [7, 12, 30, 40].index(n_inp) + 4 * int(aligned) + 8 * int(head)
    if head:       # the head's widest layer input (the 12 feature columns) asks for at least 16 lanes
        lanes = max(lanes, 16)
    for d in (1, 2, 3):
        case = _lane_case(n_inp, aligned, head, d)
        model = case.build(hip_device).double().requires_grad_(False)
        shape, periodic = SHAPES[d], list(MIXES[d][turn % len(MIXES[d])])
        x = case.frames(65, seed=n_inp + d, dev=CPU).double().to(hip_device)
        args = (case.feats, case.uav, case.align)
        _, y_ref = vr._reference_y(model, *args, x)
        lower, spacing = _grid_from(y_ref, shape, periodic)
        table = _seeded_table(shape, 100 + turn + d)
        (y, v, dx), info, want, cells, inside = _check(model, args, x, table, lower, spacing, periodic, (case.name, aligned, head, d, 65))
        assert "%d lanes per frame" % lanes in info, info
        _cells_hit(cells, inside, shape, periodic)
        untouched = sorted(set(range(n_inp)) - case.touched())
        if untouched:
            assert float(dx[:, untouched].abs().max()) == 0.0
        if d == 1 and not periodic[0]:
            outside = (~inside[:, 0]).to(hip_device)
            assert bool(outside.any()) and float(dx[outside].abs().max()) == 0.0 and float(dx[~outside].abs().max()) > 0.0
        f = int(torch.where(inside.all(dim=1), want[1].abs(), torch.zeros(65, dtype=F64)).argmax())     # one frame, inside every axis
        assert bool(inside[f].all())
        _check(model, args, x[f:f + 1].contiguous(), table, lower, spacing, periodic, (case.name, aligned, head, d, 1))


def test_every_mix_of_periodic_flags_is_walked():
    for d in (1, 2, 3):
        assert {tuple(MIXES[d][turn % len(MIXES[d])]) for turn in range(16)} == set(MIXES[d])


# ---- 2. a phi / psi surface ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65])
def test_phi_psi_surface(n, hip_device):
    """The two C3 dihedrals as angle values on a periodic 16 x 16 table from -pi; lower moved by 5 periods either way agrees."""
    w, case, model = vr._c3_angles(hip_device)
    x = w.make_frames(n, seed=40 + n).double().to(hip_device)
    shape, periodic, spacing = (16, 16), [True, True], [TWO_PI / 16] * 2
    table = _seeded_table(shape, 41)
    args = (case.feats, True, case.align)
    xx, y_ref = vr._reference_y(model, *args, x)
    assert float(y_ref.detach().abs().max()) <= math.pi
    want, _, cells, _ = _oracle(xx, y_ref, table, [-math.pi] * 2, spacing, periodic)
    _nontrivial(want)
    assert n == 1 or len({tuple(c) for c in cells.tolist()}) >= 4, "the frames share a cell"
    for shift in (0, 5, -5):
        got, info = _call(model, x, table.to(hip_device), [-math.pi + shift * TWO_PI] * 2, spacing, periodic)
        assert info.startswith(KERNEL)
        vh._close(got, want, ("phi/psi", n, shift))


# ---- 3. larger frames ----------------------------------------------------------------------------------------------------------------
_TWO_OUTPUTS = {}


def _two_outputs(name, dev):
    if name not in _TWO_OUTPUTS:
        _TWO_OUTPUTS[name] = vv._workload(name, dev, head=[16, 2], act=torch.nn.Tanh())
    return _TWO_OUTPUTS[name]


@pytest.mark.parametrize("name,n", [("P1", 9), ("C4", 3)])
def test_larger_frames(name, n, hip_device):
    w, model, args = _two_outputs(name, hip_device)
    if name == "C4":
        assert w.n_atoms == 5000
    x = w.make_frames(n, seed=7).double().to(hip_device)
    _, y_tab = vr._reference_y(model, *args, w.make_frames(33 if name == "C4" else 65, seed=8).double())
    shape, periodic = (6, 9), [False, True]
    lower, spacing = _grid_from(y_tab, shape, periodic)
    (_, _, dx), _, _, _, inside = _check(model, args, x, _seeded_table(shape, 60), lower, spacing, periodic, name)
    assert bool(inside[:, 0].any()), "every frame is outside axis 0"
    untouched = sorted(set(range(w.n_atoms)) - {a - 1 for a in w.touched_atoms()})
    if untouched:
        assert float(dx[:, untouched].abs().max()) == 0.0


# ---- 4. stepped-down rows ------------------------------------------------------------------------------------------------------------
def test_stepped_down_rows(hip_device):
    """The [3, 682, 2] head of the restraint's test (2051 doubles per frame: two waves per block) through ctypes, 5 frames."""
    dims, block, lds = vr.STEPPED["step_down"]
    n, n_inp = 5, 8
    head, xx, y_ref, y_tab = vh._bonds_head(dims, n, n_inp, 3)
    shape, periodic = (5, 6), [True, False]
    lower, spacing = _grid_from(y_tab, shape, periodic)
    table = _seeded_table(shape, 80)
    want, _, _, inside = _oracle(xx, y_ref, table, lower, spacing, periodic)
    _nontrivial(want)
    assert bool(inside[:, 1].any())
    dev = hip_device
    with torch.cuda.device(dev):
        plan = _capi.Plan(n_inp, features=vr.BONDS, layer_dims=dims, activation=_capi.ACT_TANH)
        assert plan.supports_value_and_grid_f64()
        lins = [m for m in head if isinstance(m, torch.nn.Linear)]
        W, B = [lin.weight.to(dev).contiguous() for lin in lins], [lin.bias.to(dev).contiguous() for lin in lins]
        y, v, dx = (torch.full(sh, NAN, dtype=F64, device=dev) for sh in ((n, 2), (n,), (n, n_inp, 3)))
        plan.value_and_grid_f64(xx.detach().to(dev), W, B, table.to(dev), lower, spacing, periodic, y, v, dx)
        torch.cuda.synchronize()
        info = plan.last_launch_info()
    assert info == "%s (values + grid in one launch; 64 lanes per frame) grid=%d block=%d lds=%d" % (KERNEL, -(-n // (block // 64)), block, lds), info
    vh._close((y, v, dx), want, "step_down")


# ---- 5. a large table ----------------------------------------------------------------------------------------------------------------
def test_a_large_table(hip_device):
    """129 x 130 x 131 points under three bonds of separate atom pairs, each short or long in the first eight frames: their reference
    cells are the first or the last of every axis in all eight combinations, so the offsets reach both ends of the table."""
    n_inp, shape, periodic = 8, (129, 130, 131), [False, False, False]
    feats = [(rb.BOND, [0, 1]), (rb.BOND, [2, 3]), (rb.BOND, [4, 5])]
    case = rb.Case("bonds3", rb._chain(n_inp, 3), feats, align=None, mlp=None)
    model = case.build(hip_device).double().requires_grad_(False)
    g = torch.Generator().manual_seed(17)
    n = 24
    x = 3.0 * torch.randn((n, n_inp, 3), generator=g, dtype=F64)
    want_len = 1.0 + 2.0 * torch.rand((n, 3), generator=g, dtype=F64)
    for f, corner in enumerate(itertools.product((1.0, 3.0), repeat=3)):
        want_len[f] = torch.tensor(corner, dtype=F64) + 0.001 * f
    for k in range(3):
        u = torch.randn((n, 3), generator=g, dtype=F64)
        x[:, 2 * k + 1] = x[:, 2 * k] + want_len[:, k, None] * u / u.norm(dim=1, keepdim=True)
    x = x.to(hip_device)
    args = (feats, False, None)
    _, y_ref = vr._reference_y(model, *args, x)
    y0 = y_ref.detach()
    spacing = [float(y0[:, k].max() - y0[:, k].min()) / (shape[k] - 2) for k in range(3)]
    lower = [float(y0[:, k].min()) - 0.5 * spacing[k] for k in range(3)]
    table = _seeded_table(shape, 18)
    (_, _, _), _, _, cells, inside = _check(model, args, x, table, lower, spacing, periodic, "large table")
    assert bool(inside.all())
    corners = {tuple(c) for c in cells[:8].tolist()}
    assert corners == set(itertools.product(*[(0, s - 2) for s in shape])), corners


# ---- 6. bits -------------------------------------------------------------------------------------------------------------------------
def _bits_case(name, dev):
    """(model, 65 frames, oracle arguments, d)"""
    if name == "C3_angles":
        w, case, model = vr._c3_angles(dev)
        return model, w.make_frames(65, seed=43).double().to(dev), (case.feats, True, case.align), 2
    case = _lane_case(7, True, False, 3)
    return case.build(dev).double().requires_grad_(False), case.frames(65, seed=43, dev=CPU).double().to(dev), (case.feats, case.uav, case.align), 3


@pytest.mark.parametrize("name", ["C3_angles", "small7"])
def test_bits(name, hip_device):
    """y is value_and_vjp's; two calls give the same bits; a frame alone has its bits in a batch of 65 (another block, another slot)."""
    model, x, args, d = _bits_case(name, hip_device)
    shape, periodic = SHAPES[d], [True] + [False] * (d - 1)
    _, y_ref = vr._reference_y(model, *args, x)
    lower, spacing = _grid_from(y_ref, shape, periodic)
    table = _seeded_table(shape, 44).to(hip_device)
    full, info = _call(model, x, table, lower, spacing, periodic)
    full = [t.clone() for t in full]
    assert KERNEL in info and all(bool(torch.isfinite(t).all()) for t in full) and float(full[1].abs().max()) > 0.05 and float(full[2].abs().max()) > 1e-3
    yv, _, info = vv._call(model, x, torch.ones((65, d), dtype=F64, device=hip_device))
    assert VJP_KERNEL in info and torch.equal(full[0], yv)
    again, _ = _call(model, x, table, lower, spacing, periodic)
    assert all(torch.equal(a, b) for a, b in zip(full, again))
    for f in (0, 9, 33, 64):
        one, _ = _call(model, x[f:f + 1].contiguous(), table, lower, spacing, periodic)
        assert all(torch.equal(a[0], b[f]) for a, b in zip(one, full)), f


# ---- 7. NaN --------------------------------------------------------------------------------------------------------------------------
def test_nan_poisons_only_its_frame(hip_device):
    model, x, args, d = _bits_case("C3_angles", hip_device)
    n, bad = x.shape[0], 33
    table = _seeded_table((16, 16), 62).to(hip_device)
    grid = ([-math.pi] * 2, [TWO_PI / 16] * 2, [True, False])
    (y0, v0, dx0), _ = _call(model, x, table, *grid)
    y0, v0, dx0 = y0.clone(), v0.clone(), dx0.clone()
    assert float(v0.abs().max()) > 0.05 and float(dx0.abs().max()) > 1e-3
    keep = torch.ones(n, dtype=torch.bool, device=hip_device)
    keep[bad] = False
    xb = x.clone()
    xb[bad] = NAN
    (y, v, dx), _ = _call(model, xb, table, *grid)
    assert torch.equal(y[keep], y0[keep]) and torch.equal(v[keep], v0[keep]) and torch.equal(dx[keep], dx0[keep])
    assert bool(torch.isnan(y[bad]).all()) and bool(torch.isnan(v[bad])) and bool(torch.isnan(dx[bad]).any())


# ---- 8. into=, refusals --------------------------------------------------------------------------------------------------------------
def test_into_and_refusals(hip_device):
    w, model, args = _two_outputs("C3", hip_device)
    n, d = 5, 2
    x = w.make_frames(n, seed=51).double().to(hip_device)
    _, y_tab = vr._reference_y(model, *args, w.make_frames(65, seed=52).double())
    shape, periodic = (5, 6), [False, True]
    lower, spacing = _grid_from(y_tab, shape, periodic)
    table = _seeded_table(shape, 53).to(hip_device)
    (y, v, dx), _ = _call(model, x, table, lower, spacing, periodic)
    new = lambda *sh: torch.full(sh, NAN, dtype=F64, device=hip_device)       # noqa: E731
    y2, v2, dx2 = new(n, d), new(n), new(n, w.n_atoms, 3)
    r, _ = _call(model, x, table, lower, spacing, periodic, into=(y2, v2, dx2))
    assert r[0] is y2 and r[1] is v2 and r[2] is dx2
    assert torch.equal(y2, y) and torch.equal(v2, v) and torch.equal(dx2, dx) and float(v.abs().max()) > 0.0
    # CPU tensors for the grid, no flags = none periodic
    k1 = model.value_and_grid(x, table, torch.tensor(lower, dtype=F64), torch.tensor(spacing, dtype=F64))
    k2 = model.value_and_grid(x, table, lower, spacing, [False, False])
    assert all(torch.equal(a, b) for a, b in zip(k1, k2))
    y3, v3, dx3 = new(n, d), new(n), new(n, w.n_atoms, 3)
    bad_calls = [
        (TypeError, dict(into=(y3, dx3))), (TypeError, dict(into=(y3.float(), v3, dx3))), (ValueError, dict(into=(y3[:4], v3, dx3))),
        (ValueError, dict(into=(y3, v3.cpu(), dx3))), (ValueError, dict(into=(y3, v3, dx3.transpose(1, 2)))),
        (ValueError, dict(table=table.cpu())), (TypeError, dict(table=table.float())), (ValueError, dict(table=table[:3])),
        (ValueError, dict(table=table.t())), (ValueError, dict(table=table.reshape(-1))), (ValueError, dict(spacing=[0.1, 0.0])),
        (ValueError, dict(spacing=[0.1, NAN])), (ValueError, dict(spacing=[0.1, -0.1])), (ValueError, dict(lower=[0.0])),
        (ValueError, dict(periodic=[True])), (ValueError, dict(lower=[0.0, float("inf")])),
    ]
    for exc, changes in bad_calls:
        kw = dict(table=table, lower=lower, spacing=spacing, periodic=periodic, into=(y3, v3, dx3))
        kw.update(changes)
        with pytest.raises(exc):
            model.value_and_grid(x, **kw)
    with pytest.raises(TypeError, match="float64"):
        model.value_and_grid(x.float(), table, lower, spacing)
    with pytest.raises(NotImplementedError, match="value_and_vjp"):
        model.value_and_grid(x.cpu(), table.cpu(), lower, spacing)
    # more than three outputs: the C3 features themselves (two dihedrals as cos and sin, an angle, a bond)
    pre = model.preprocessing_layer
    dp = pre.output_dimension()
    assert dp == 6
    f4, wide = new(n, dp), torch.zeros((4,) * dp, dtype=F64, device=hip_device)
    with pytest.raises(NotImplementedError, match=r"at most 3 outputs \(got 6\); use `model\(x\)`, interpolate the table"):
        pre.value_and_grid(x, wide, [0.0] * dp, [1.0] * dp, into=(f4, v3, dx3))
    plan4 = vv._feature_plan(pre, x)
    with torch.cuda.device(hip_device):
        assert plan4.supports_value_and_restraint_f64() and not plan4.supports_value_and_grid_f64()
        with pytest.raises(_capi.MolannHipError) as err:
            plan4.value_and_grid_f64(x, [], [], wide, [0.0] * dp, [1.0] * dp, None, f4, v3, dx3)
        assert err.value.code == _capi.E_UNSUPPORTED
        # the C entry's own refusals, on a plan it serves
        p = _capi.Plan(22, features=[(wl.BOND, [0, 1])])
        assert p.supports_value_and_grid_f64()
        y1, t1 = new(n, 1), torch.zeros(8, dtype=F64, device=hip_device)

        def code(tab=t1, lo=(0.0,), sp=(1.0,)):
            with pytest.raises(_capi.MolannHipError) as err:
                p.value_and_grid_f64(x, [], [], tab, lo, sp, None, y1, v3, dx3)
            return err.value.code

        assert code(tab=t1[:3]) == _capi.E_DESC and code(sp=(0.0,)) == _capi.E_DESC and code(sp=(NAN,)) == _capi.E_DESC
        assert code(sp=(float("inf"),)) == _capi.E_DESC and code(lo=(NAN,)) == _capi.E_DESC
        L, s = _capi.lib(), torch.cuda.current_stream().cuda_stream
        import ctypes
        one, lo1, sp1 = (ctypes.c_int64 * 1)(8), (ctypes.c_double * 1)(0.0), (ctypes.c_double * 1)(1.0)
        raw = lambda tab, shape, lo, sp: L.molann_value_and_grid_f64(p._handle, x.data_ptr(), n, None, None, tab, shape, lo, sp, None,       # noqa: E731
                                                                     y1.data_ptr(), v3.data_ptr(), dx3.data_ptr(), s)
        assert raw(t1.data_ptr(), None, lo1, sp1) == _capi.E_NULL and raw(t1.data_ptr(), one, None, sp1) == _capi.E_NULL
        assert raw(t1.data_ptr(), one, lo1, None) == _capi.E_NULL and raw(None, one, lo1, sp1) == _capi.E_NULL
        assert raw(t1.data_ptr() + 4, one, lo1, sp1) == _capi.E_ALIGNMENT
        assert L.molann_value_and_grid_f64(p._handle, None, 0, None, None, None, None, None, None, None, None, None, None, s) == 0
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (y3, v3, dx3, y1, f4)), "a refusal launched"
    with torch.cuda.device(hip_device):
        assert vv._feature_plan(vr._c3_angles(hip_device)[2], x).supports_value_and_grid_f64()
    empty = model.value_and_grid(x[:0], table, lower, spacing)
    assert [tuple(t.shape) for t in empty] == [(0, d), (0,), (0, w.n_atoms, 3)]


# ---- 9. the dispatcher operators -----------------------------------------------------------------------------------------------------
def test_scripted_model_and_operators(tmp_path, hip_device):
    import warnings
    w, model, args = _two_outputs("C3", hip_device)
    x = w.make_frames(65, seed=71).double().to(hip_device)
    _, y_ref = vr._reference_y(model, *args, x)
    shape, periodic = (7, 5), [True, False]
    lower, spacing = _grid_from(y_ref, shape, periodic)
    table = _seeded_table(shape, 72).to(hip_device)
    want = model.value_and_grid(x, table, lower, spacing, periodic)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.jit.script(model).save(str(tmp_path / "c3_two_f64.pt"))
    loaded = torch.jit.load(str(tmp_path / "c3_two_f64.pt"), map_location=hip_device)
    ws = [lin.weight for lin in loaded.linears.children()]
    bs = [lin.bias for lin in loaded.linears.children()]
    desc = list(loaded.desc)
    handle = torch.ops.molann.register_desc(desc)
    by_handle = torch.ops.molann.value_and_grid_h(x, handle, loaded.ref_x, ws, bs, table, lower, spacing, periodic, [])
    by_desc = torch.ops.molann.value_and_grid(x, desc, loaded.ref_x, ws, bs, table, lower, spacing, periodic, [])
    torch.cuda.synchronize()
    info = torch.ops.molann.launch_info(desc, hip_device.index)
    assert info.count(KERNEL) == 1 and info.count("_kernel") == 1, info
    assert len(by_handle) == 3 and len(by_desc) == 3
    assert all(torch.equal(a, b) for a, b in zip(by_handle, want)) and all(torch.equal(a, b) for a, b in zip(by_desc, want))
    assert float(want[1].abs().max()) > 0.05 and float(want[2].abs().max()) > 1e-3
    plain = torch.ops.molann.value_and_grid(x, desc, loaded.ref_x, ws, bs, table, lower, spacing, [], [])
    assert all(torch.equal(a, b) for a, b in zip(plain, model.value_and_grid(x, table, lower, spacing)))


# ---- 10. the caller's buffers ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", [1, "mixedA", "mixedB"])
def test_offset_buffers_inside_guard_bands(where, hip_device):
    """x, the table, out, bias and grad_x at offset positions inside guard bands: the bands intact, the inputs unchanged, the bits of
    the call on fresh tensors."""
    model, x, args, d = _bits_case("small7", hip_device)
    shape, periodic = SHAPES[d], [False, True, False]
    _, y_ref = vr._reference_y(model, *args, x)
    lower, spacing = _grid_from(y_ref, shape, periodic)
    table = _seeded_table(shape, 91).to(hip_device)
    want, _ = _call(model, x, table, lower, spacing, periodic)
    want = [t.clone() for t in want]
    assert float(want[1].abs().max()) > 0.05 and float(want[2].abs().max()) > 1e-3
    arena = placement.Arena(hip_device)
    names = ("x", "table", "out", "bias", "grad_x")
    off = placement.offsets(where, names, wide=2)
    xa = arena.carve("x", x.shape, F64, off["x"], data=x)
    ta = arena.carve("table", table.shape, F64, off["table"], data=table)
    into = (arena.carve("out", (65, d), F64, off["out"]), arena.carve("bias", (65,), F64, off["bias"]),
            arena.carve("grad_x", x.shape, F64, off["grad_x"]))
    got, info = _call(model, xa, ta, lower, spacing, periodic, into=into)
    assert KERNEL in info and all(a is b for a, b in zip(got, into))
    assert arena.check() == [] and arena.inputs_changed() == []
    assert all(placement.same_bits(a, b) for a, b in zip(got, want))


# ---- 11. one launch, the neighbours untouched ----------------------------------------------------------------------------------------
def test_one_launch_and_the_neighbours_untouched(hip_device):
    w, model, args = _two_outputs("C3", hip_device)
    n, d = 64, 2
    x = w.make_frames(n, seed=91).double().to(hip_device)
    on = lambda *v: torch.tensor(v, dtype=F64, device=hip_device)       # noqa: E731
    G = torch.ones((n, d), dtype=F64, device=hip_device)
    hills = (on(0.1, -0.2, 0.3, 0.4, -0.3, 0.1).reshape(3, 2), on(0.7, -0.4, 0.9), on(0.5, 0.6))

    def neighbours():
        out = []
        for call, kernel in ((lambda: model.value_and_hills(x, *hills), vh.KERNEL),
                             (lambda: model.value_and_restraint(x, on(0.1, -0.1), 1.5), vr.KERNEL), (lambda: model.value_and_vjp(x, G), VJP_KERNEL)):
            got = call()
            torch.cuda.synchronize()
            assert model.last_launch_info().startswith(kernel)
            out += [t.clone() for t in got]
        return out

    before = neighbours()
    _, y_ref = vr._reference_y(model, *args, x)
    shape, periodic = (5, 6), [True, False]
    lower, spacing = _grid_from(y_ref, shape, periodic)
    (y, v, dx), info = _call(model, x, _seeded_table(shape, 92).to(hip_device), lower, spacing, periodic)
    assert info.startswith(KERNEL + " (values + grid in one launch; ") and info.count("_kernel") == 1 and "molann_" not in info and "||" not in info, info
    assert float(v.abs().max()) > 0.05 and float(dx.abs().max()) > 1e-3 and torch.equal(y, before[-2])
    after = neighbours()
    assert len(before) == 8 and all(placement.same_bits(a, b) for a, b in zip(before, after))
