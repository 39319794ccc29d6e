"""MolANN.value_and_bias / PreprocessingANN.value_and_bias / molann_value_and_bias_f64 on the GPU: a restraint on all outputs, hills and a
table on chosen outputs, the three energies and the gradient of their sum in one launch of frames_value_bias_f64_kernel.

The reference is the CPU float64 oracle of the sibling tests (`vr._reference_y`), and every centre, hill table and grid is built from ITS
y - the chosen columns taken with ``y[:, cols]`` - by the siblings' builders, which assert their conditions on the reference values:
hills near (q < 2) and far (q > 50), no element within 1e-9 of a wrap seam, a flat edge or a range end, the first, last and seam cells
of an axis hit, nothing nearly zero.  Bounds, the family's, each energy column on its own scale: y within 1e-10 max(1, |y|max), each
energy within 1e-10 max(1, |E|max), dx within 1e-9 max(1e-3, |dx|max).  Every call asserts one launch by its info string."""

import ctypes
import math

import pytest
import torch

import placement
import test_gpu_random_backward as rb
import test_gpu_value_and_grid_f64 as vg
import test_gpu_value_and_hills_f64 as vh
import test_gpu_value_and_restraint_f64 as vr
import test_gpu_value_and_vjp_f64 as vv
from molann_amd import _capi, workloads as wl
from molann_amd.bias import Grid, Hills, Restraint

pytestmark = pytest.mark.gpu
KERNEL = "frames_value_bias_f64_kernel"
INFO = KERNEL + " (values + bias in one launch; "
TWO_PI = 2.0 * math.pi
NAN = float("nan")
CPU = torch.device("cpu")
F64 = torch.float64
SEL = 11        # the selection row: 8 hills columns and 3 grid columns


class Terms(object):
    """The three terms on the CPU, built from reference outputs.  r: (z [n, d_out], kappa, period or None, flat or None); h: (columns,
    centers, heights, sigma, period row over the columns); g: (columns, table, lower, spacing, periodic)."""

    def __init__(self, r=None, h=None, g=None):
        self.r, self.h, self.g = r, h, g

    def frame(self, f):
        """the terms of frame f alone: its row of the per-frame centres"""
        r = None if self.r is None else (self.r[0][f:f + 1].contiguous(),) + self.r[1:]
        return Terms(r, self.h, self.g)

    def records(self, dev, identity=False):
        on = lambda t: None if t is None else t.to(dev)       # noqa: E731
        positive = lambda p: None if p is None or not bool((p > 0).any()) else on(p)       # noqa: E731
        R = H = G = None
        if self.r is not None:
            z, kappa, period, flat = self.r
            R = Restraint(on(z), on(kappa), positive(period), on(flat))
        if self.h is not None:
            cols, c, w, s, period = self.h
            H = Hills(on(c), on(w), on(s), positive(period), columns=None if identity else list(cols))
        if self.g is not None:
            cols, table, lower, spacing, periodic = self.g
            G = Grid(on(table), lower, spacing, periodic, columns=None if identity else list(cols))
        return dict(restraint=R, hills=H, grid=G)


def _build(y_ref, y_tab, r=None, h=None, g=None, seed=0):
    """Terms from the reference: r = (period row [d_out], with_flat, free outputs); h = (columns, period row over them, H, per_hill);
    g = (columns, shape, periodic).  Returns (terms, far, grid built from y_ref itself)."""
    y_ref, y_tab = y_ref.detach(), y_tab.detach()
    R = H = G = None
    far, own = True, y_ref.shape[0] >= 24
    if r is not None:
        period, with_flat, free = r
        z, kappa, flat = vr._centres(y_ref, period, with_flat, seed)
        kappa[list(free)] = 0.0
        R = (z, kappa, period, flat)
    if h is not None:
        cols, period, n_hills, per_hill = h
        (c, w, s), far = vh._hill_table(y_ref[:, list(cols)], y_tab[:, list(cols)], period, n_hills, per_hill, seed + 1)
        H = (tuple(cols), c, w, s, period)
    if g is not None:
        cols, shape, periodic = g
        lower, spacing = vg._grid_from((y_ref if own else y_tab)[:, list(cols)], shape, periodic)
        G = (tuple(cols), vg._seeded_table(shape, seed + 2), lower, spacing, list(periodic))
    return Terms(R, H, G), far, own


def _oracle(xx, y, T):
    """((y, energies [n, 3], d(sum)/dx), the table's cells and inside flags or None) by float64 autograd of the three formulas, with
    the table's margins asserted by the sibling's oracle"""
    n = y.shape[0]
    e = [torch.zeros(n, dtype=F64)] * 3
    cells = inside = None
    if T.r is not None:
        z, kappa, period, flat = T.r
        d = vr._wrapped(y, z, period, flat)
        e[0] = 0.5 * (kappa * d * d).sum(dim=1)
    if T.h is not None:
        cols, c, w, s, period = T.h
        e[1] = vh._bias(y[:, list(cols)], c, w, s, period)[0] if c.shape[0] else torch.zeros(n, dtype=F64)
    if T.g is not None:
        cols, table, lower, spacing, periodic = T.g
        (_, e[2], _), _, cells, inside = vg._oracle(xx, y[:, list(cols)], table, lower, spacing, periodic)
        e[2] = vg._interp(y[:, list(cols)], table, lower, spacing, periodic)[0]
    total = sum(t.sum() for t in e if t.requires_grad)
    (gx,) = torch.autograd.grad(total, xx, retain_graph=True)
    return (y.detach(), torch.stack([t.detach() for t in e], dim=1), gx), cells, inside


def _close(got, want, what, present=(True, True, True)):
    (y, e, dx), (y_want, e_want, gx_want) = got, want
    assert all(t.dtype == F64 for t in got) and y.shape == y_want.shape and e.shape == e_want.shape and dx.shape == gx_want.shape
    y, e, dx = y.detach().cpu(), e.detach().cpu(), dx.detach().cpu()
    ey, sy = float((y - y_want).abs().max()), max(1.0, float(y_want.abs().max()))
    ed, sd = float((dx - gx_want).abs().max()), max(1e-3, float(gx_want.abs().max()))
    print("%s: y err %.3e (scale %.3g), dx err %.3e (scale %.3g)" % (what, ey, sy, ed, sd))
    assert ey <= 1e-10 * sy, (what, "y", ey, sy)
    for c, name in enumerate(("E_r", "V_h", "V_g")):
        if not present[c]:
            assert bool((e[:, c] == 0.0).all()) and not bool(torch.signbit(e[:, c]).any()), (what, name, "an absent term's column is not 0.0")
            continue
        ee, se = float((e[:, c] - e_want[:, c]).abs().max()), max(1.0, float(e_want[:, c].abs().max()))
        print("    %s err %.3e (scale %.3g)" % (name, ee, se))
        assert ee <= 1e-10 * se, (what, name, ee, se)
    assert ed <= 1e-9 * sd, (what, "dx", ed, sd)


def _call(model, x, T, into=None, identity=False):
    out = model.value_and_bias(x, into=into, **T.records(x.device, identity))
    torch.cuda.synchronize()
    info = vh._info(model)
    assert info.startswith(INFO) and info.count("_kernel") == 1, info
    return out, info


def _reference_terms(model, args, x, x_tab, spec, seed, what):
    """(terms, the oracle's (y, energies, dx), far) for a model and a batch: everything from the reference's y, with the siblings'
    conditions and 'nothing nearly zero' asserted on the reference values - also where a test only compares the code with itself"""
    xx, y_ref = vr._reference_y(model, *args, x)
    _, y_tab = vr._reference_y(model, *args, x_tab)
    T, far, own = _build(y_ref, y_tab, seed=seed, **spec)
    want, cells, inside = _oracle(xx, y_ref, T)
    present = (T.r is not None, T.h is not None and T.h[1].shape[0] > 0, T.g is not None)
    for c in range(3):
        assert not present[c] or float(want[1][:, c].abs().max()) > 0.05, (what, c, "the reference energy is (nearly) zero")
    assert float(want[2].abs().max()) > 1e-3
    if T.g is not None and own:
        vg._cells_hit(cells, inside, T.g[1].shape, T.g[4])
    return T, want, far


def _check(model, args, x, x_tab, spec, seed, what):
    T, want, far = _reference_terms(model, args, x, x_tab, spec, seed, what)
    got, info = _call(model, x, T)
    _close(got, want, what, (T.r is not None, T.h is not None, T.g is not None))
    return got, info, T, far


# ---- 1. every lane group -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_inp,lanes", [(7, 8), (12, 16), (30, 32), (40, 64)])
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "no_alignment"])
@pytest.mark.parametrize("head", [True, False], ids=["head", "features"])
def test_lane_groups(n_inp, lanes, aligned, head, hip_device):
    """All three terms on 65 frames.  A [d_feat, 5, 4] head: hills on (3, 1), the table on (0, 2) with one periodic axis, output 1
    free of the restraint.  Features only (6 columns): hills on (5, 0, 2), the table on (1, 3)."""
    if head:
        case = vv._small_case(n_inp, [0, 2, 4, 6] if aligned else None, head=True)
        case.mlp = [case.d_feat(), 5, 4]
        d_out, hc, gc = 4, (3, 1), (0, 2)
        lanes = max(lanes, 16)       # the head's widest layer input (the 12 feature columns) asks for at least 16 lanes
    else:
        case = vh._small_case(n_inp, aligned, False)
        d_out, hc, gc = 6, (5, 0, 2), (1, 3)
    model = case.build(hip_device).double().requires_grad_(False)
    x = case.frames(65, seed=n_inp + 3, dev=CPU).double().to(hip_device)
    x_tab = case.frames(65, seed=900 + n_inp, dev=CPU).double().to(hip_device)
    spec = dict(r=(vr._period_row(d_out, 1.3, 2), True, [1]), h=(hc, vr._period_row(len(hc), 1.3, 2), 2 * lanes + 5, True), g=(gc, (5, 6), [True, False]))
    (y, e, dx), info, T, far = _check(model, (case.feats, case.uav, case.align), x, x_tab, spec, n_inp, (case.name, aligned, head))
    assert "%d lanes per frame" % lanes in info and far, info
    assert float(T.r[1][1]) == 0.0
    untouched = sorted(set(range(n_inp)) - case.touched())
    if untouched:
        assert float(dx[:, untouched].abs().max()) == 0.0


# ---- 2. past the single entries' caps ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65])
def test_c3_eight_outputs(n, hip_device):
    """C3's own model, 8 outputs: a table on (6, 1), hills on (0, 3, 7), the restraint on all - value_and_grid refuses this model."""
    w, model, args = vv._shared("C3", hip_device)
    assert w.out_dim() == 8
    x = w.make_frames(n, seed=30 + n).double().to(hip_device)
    x_tab = w.make_frames(65, seed=32).double().to(hip_device)
    spec = dict(r=(vr._period_row(8, 1.1, 3), True, []), h=((0, 3, 7), vr._period_row(3, 0.9, 2), 37, n == 65), g=((6, 1), (6, 7), [False, True]))
    _, _, _, far = _check(model, args, x, x_tab, spec, 33 + n, ("C3", n))
    assert far
    with pytest.raises(NotImplementedError):
        model.value_and_grid(x, torch.zeros((4,) * 3, dtype=F64, device=hip_device), [0.0] * 3, [1.0] * 3)


@pytest.mark.parametrize("n", [1, 65])
def test_positions_and_two_dihedral_angles(n, hip_device):
    """Features only: the 21 position columns of the restraint's test and two dihedral angle values behind them; hills and a periodic
    table from -pi on the two angles (period 2 pi), the restraint on all 23 - value_and_hills refuses this module."""
    feats = [(rb.POS, list(range(7))), (rb.DIH, [0, 1, 2, 3]), (rb.DIH, [2, 3, 4, 5])]
    case = rb.Case("pos7dih", rb._chain(7, 3), feats, align=[0, 2, 4, 6], uav=True, mlp=None)
    model = case.build(hip_device).double().requires_grad_(False)
    assert case.d_feat() == 23
    args = (case.feats, True, case.align)
    x = case.frames(n, seed=70 + n, dev=CPU).double().to(hip_device)
    x_tab = case.frames(65, seed=75, dev=CPU).double().to(hip_device)
    xx, y_ref = vr._reference_y(model, *args, x)
    _, y_tab = vr._reference_y(model, *args, x_tab)
    period = torch.zeros(23, dtype=F64)
    period[21:] = TWO_PI
    T, far, _ = _build(y_ref, y_tab, r=(period, True, []), h=((21, 22), vr._period_row(2, TWO_PI), 23, True), seed=71 + n)
    shape = (8, 9)
    T.g = ((21, 22), vg._seeded_table(shape, 73), [-math.pi] * 2, [TWO_PI / s for s in shape], [True, True])
    assert float(y_ref.detach()[:, 21:].abs().max()) <= math.pi
    want, _, _ = _oracle(xx, y_ref, T)
    assert all(float(want[1][:, c].abs().max()) > 0.05 for c in range(3)) and float(want[2].abs().max()) > 1e-3
    got, info = _call(model, x, T)
    # nine items ask for 16 lanes; a frame's rows are its 23 outputs and the selection row
    assert "16 lanes per frame" in info and info.endswith("lds=%d" % ((256 // 16) * (23 + SEL) * 8)), info
    _close(got, want, ("pos7dih", n))
    with pytest.raises(NotImplementedError):
        model.value_and_hills(x, torch.zeros((1, 23), dtype=F64, device=hip_device), 1.0, 1.0)


# ---- 3. one term alone is the single entry, bit for bit ------------------------------------------------------------------------------
def _three_outputs(name, dev):
    if name == "C3_angles_bond":
        w, case, model = vr._c3_angles(dev, bond=True)
        return model, w.make_frames(65, seed=43).double().to(dev), w.make_frames(65, seed=44).double().to(dev), (case.feats, True, case.align), \
            torch.tensor([TWO_PI, TWO_PI, 0.0], dtype=F64)
    case = vg._lane_case(7, True, False, 3)
    model = case.build(dev).double().requires_grad_(False)
    return model, case.frames(65, seed=43, dev=CPU).double().to(dev), case.frames(65, seed=44, dev=CPU).double().to(dev), \
        (case.feats, case.uav, case.align), torch.tensor([TWO_PI, 0.0, 0.0], dtype=F64)


def _single_calls(model, x, T):
    """the three single entries on the same terms (identity columns): [(y, scalar, dx)] * 3, None for an absent term"""
    rec = T.records(x.device, identity=True)
    out = [None] * 3
    if rec["restraint"] is not None:
        out[0] = model.value_and_restraint(x, *rec["restraint"])
    if rec["hills"] is not None:
        out[1] = model.value_and_hills(x, *rec["hills"][:4])
    if rec["grid"] is not None:
        out[2] = model.value_and_grid(x, *rec["grid"][:4])
    torch.cuda.synchronize()
    return [None if t is None else tuple(v.clone() for v in t) for t in out]


def _alone(model, x, T, c, what):
    got, _ = _call(model, x, T, identity=c != 0)
    single = _single_calls(model, x, T)[c]
    assert torch.equal(got[0], single[0]) and torch.equal(got[1][:, c], single[1]) and torch.equal(got[2], single[2]), what
    others = [k for k in range(3) if k != c]
    assert bool((got[1][:, others] == 0.0).all()) and not bool(torch.signbit(got[1][:, others]).any()), what
    return got


@pytest.mark.parametrize("name", ["C3_angles_bond", "small7"])
def test_one_term_alone_is_the_single_entry(name, hip_device):
    model, x, x_tab, args, period = _three_outputs(name, hip_device)
    _, y_ref = vr._reference_y(model, *args, x)
    _, y_tab = vr._reference_y(model, *args, x_tab)
    cols = (0, 1, 2)
    T, far, _ = _build(y_ref, y_tab, r=(period, True, []), h=(cols, period, 45, True), g=(cols, vg.SHAPES[3], [bool(period[0] > 0), False, True]), seed=5)
    assert far
    got = _alone(model, x, Terms(r=T.r), 0, (name, "restraint"))
    assert float(got[1][:, 0].abs().max()) > 0.05 and float(got[2].abs().max()) > 1e-3
    got = _alone(model, x, Terms(h=T.h), 1, (name, "hills"))
    assert float(got[1][:, 1].abs().max()) > 0.05 and float(got[2].abs().max()) > 1e-3
    got = _alone(model, x, Terms(g=T.g), 2, (name, "grid"))
    assert float(got[1][:, 2].abs().max()) > 0.05 and float(got[2].abs().max()) > 1e-3
    # no hills yet: zeros from both entries
    empty = Terms(h=(cols, torch.zeros((0, 3), dtype=F64), torch.zeros(0, dtype=F64), torch.ones((0, 3), dtype=F64), period))
    got = _alone(model, x, empty, 1, (name, "H = 0"))
    assert float(got[1].abs().max()) == 0.0 and float(got[2].abs().max()) == 0.0


def test_restraint_alone_on_p1(hip_device):
    w, model, args = vv._shared("P1", hip_device)
    x = w.make_frames(9, seed=90).double().to(hip_device)
    _, y_ref = vr._reference_y(model, *args, x)
    T, _, _ = _build(y_ref, y_ref, r=(vr._period_row(w.out_dim(), 1.1, 3), True, []), seed=91)
    got = _alone(model, x, T, 0, "P1")
    assert float(got[1][:, 0].abs().max()) > 0.05


# ---- 4. all three together on identity columns ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["C3_angles_bond", "small7"])
def test_three_terms_on_identity_columns(name, hip_device):
    model, x, x_tab, args, period = _three_outputs(name, hip_device)
    xx, y_ref = vr._reference_y(model, *args, x)
    _, y_tab = vr._reference_y(model, *args, x_tab)
    cols = (0, 1, 2)
    T, _, _ = _build(y_ref, y_tab, r=(period, True, []), h=(cols, period, 45, False), g=(cols, vg.SHAPES[3], [bool(period[0] > 0), True, False]), seed=15)
    want, _, _ = _oracle(xx, y_ref, T)
    got, _ = _call(model, x, T, identity=True)
    listed, _ = _call(model, x, T)
    assert all(torch.equal(a, b) for a, b in zip(got, listed))          # None is the list 0..d-1
    _close(got, want, (name, "three terms"))
    single = _single_calls(model, x, T)
    for c in range(3):
        assert torch.equal(got[0], single[c][0]) and torch.equal(got[1][:, c], single[c][1]), (name, c)
    dx_sum = single[0][2] + single[1][2] + single[2][2]
    ed, sd = float((got[2] - dx_sum).abs().max()), max(1e-3, float(dx_sum.abs().max()))
    print("%s: dx against the sum of the three single calls %.3e (scale %.3g)" % (name, ed, sd))
    assert ed <= 1e-9 * sd


# ---- 5. larger frames and stepped-down rows ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [("P1", 9), ("C4", 3)])
def test_larger_frames(name, n, hip_device):
    w, model, args = vv._shared(name, hip_device)
    d = w.out_dim()
    assert d >= 2
    x = w.make_frames(n, seed=7).double().to(hip_device)
    x_tab = w.make_frames(33 if name == "C4" else 65, seed=8).double().to(hip_device)
    spec = dict(r=(vr._period_row(d, 1.1, 3), True, [0]), h=((d - 1, 0), vr._period_row(2, 0.8, 2), 75, True), g=((0, d - 1), (6, 9), [False, True]))
    (_, _, dx), _, _, far = _check(model, args, x, x_tab, spec, 60, name)
    assert far
    untouched = sorted(set(range(w.n_atoms)) - {a - 1 for a in w.touched_atoms()})
    if untouched:
        assert float(dx[:, untouched].abs().max()) == 0.0


def _rows(dims):
    """doubles of LDS per frame of the entry for a head on d_feat features: the restraint's rows and the selection row"""
    return dims[0] + sum(dims[1:-1]) + 2 * max(dims[:-1]) + dims[-1] + SEL


@pytest.mark.parametrize("name", sorted(vr.STEPPED))
def test_heads_that_step_the_rows_down(name, hip_device):
    """The [3, 682, 2] head through Plan.value_and_bias_f64 with 5 frames, 4099 hills and a (5, 6) table: two waves per block; the
    over_64k head once with a restraint and a table: one wave per block, more LDS than a launch may ask for by default."""
    dims = vr.STEPPED[name][0]
    n, n_inp = 5, 8
    head, xx, y_ref, y_tab = vh._bonds_head(dims, n, n_inp, 3)
    period = torch.tensor([0.7, 0.0], dtype=F64)
    hills = ((1, 0), torch.tensor([0.0, 0.7], dtype=F64), 4099, True) if name == "step_down" else None
    T, far, _ = _build(y_ref, y_tab, r=(period, True, []), h=hills, g=((1, 0), (5, 6), [True, False]), seed=80)
    want, _, inside = _oracle(xx, y_ref, T)
    assert far and bool(inside[:, 1].any()) and float(want[1][:, 2].abs().max()) > 0.05
    per_frame = _rows(dims) * 8
    waves = 4
    while waves > 1 and waves * per_frame > 65536:
        waves //= 2
    assert (name, waves) in (("step_down", 2), ("over_64k", 1)) and (per_frame > 65536) == (name == "over_64k")
    dev = hip_device
    on = lambda t: None if t is None else t.to(dev)       # noqa: E731
    with torch.cuda.device(dev):
        plan = _capi.Plan(n_inp, features=vr.BONDS, layer_dims=dims, activation=_capi.ACT_TANH)
        assert plan.supports_value_and_bias_f64()
        lins = [m for m in head if isinstance(m, torch.nn.Linear)]
        W, B = [lin.weight.to(dev).contiguous() for lin in lins], [lin.bias.to(dev).contiguous() for lin in lins]
        y, e, dx = (torch.full(sh, NAN, dtype=F64, device=dev) for sh in ((n, 2), (n, 3), (n, n_inp, 3)))
        plan.value_and_bias_f64(xx.detach().to(dev), W, B, y, e, dx, restraint=tuple(on(t) for t in T.r),
                                hills=None if T.h is None else (T.h[0],) + tuple(on(t) for t in T.h[1:]), grid=(T.g[0], on(T.g[1])) + T.g[2:])
        torch.cuda.synchronize()
        info = plan.last_launch_info()
    assert info == "%s64 lanes per frame) grid=%d block=%d lds=%d" % (INFO, -(-n // waves), 64 * waves, waves * per_frame), info
    _close((y, e, dx), want, name, (True, T.h is not None, True))


# ---- 6. determinism ------------------------------------------------------------------------------------------------------------------
def _c3_spec():
    """C3's 8 outputs: the restraint on all, hills on (0, 3, 7), the table on (6, 1)"""
    return dict(r=(vr._period_row(8, 1.1, 3), True, []), h=((0, 3, 7), vr._period_row(3, 0.9, 2), 37, True), g=((6, 1), (6, 7), [False, True]))


def _small7_spec():
    """the 7-atom aligned features (6 columns): output 1 free, hills on (5, 0, 2), the table on (1, 3)"""
    return dict(r=(vr._period_row(6, 1.3, 2), True, [1]), h=((5, 0, 2), vr._period_row(3, 1.3, 2), 21, True), g=((1, 3), (5, 6), [True, False]))


def _small7(dev, seed):
    case = vh._small_case(7, True, False)
    model = case.build(dev).double().requires_grad_(False)
    return model, (case.feats, case.uav, case.align), case.frames(65, seed=seed, dev=CPU).double().to(dev), case.frames(65, seed=seed + 500, dev=CPU).double().to(dev)


def test_two_calls_give_the_same_bits(hip_device):
    w, model, args = vv._shared("C3", hip_device)
    x = w.make_frames(4097, seed=21).double().to(hip_device)
    T, _, far = _reference_terms(model, args, x, x[:65], _c3_spec(), 22, "two calls")
    assert far
    first, _ = _call(model, x, T)
    first = [t.clone() for t in first]
    assert all(bool(torch.isfinite(t).all()) for t in first) and all(float(first[1][:, c].abs().max()) > 0.05 for c in range(3))
    second, _ = _call(model, x, T)
    assert all(torch.equal(a, b) for a, b in zip(first, second))


@pytest.mark.parametrize("name", ["C3", "small7"])
def test_a_frame_alone_has_its_bits_in_the_batch(name, hip_device):
    if name == "C3":
        w, model, args = vv._shared("C3", hip_device)
        x, x_tab, spec = w.make_frames(65, seed=23).double().to(hip_device), w.make_frames(65, seed=29).double().to(hip_device), _c3_spec()
    else:
        model, args, x, x_tab = _small7(hip_device, 23)
        spec = _small7_spec()
    T, _, far = _reference_terms(model, args, x, x_tab, spec, 24, name)
    assert far
    full, _ = _call(model, x, T)
    full = [t.clone() for t in full]
    assert all(float(full[1][:, c].abs().max()) > 0.05 for c in range(3)) and float(full[2].abs().max()) > 1e-3
    for f in (0, 9, 33, 64):
        one, _ = _call(model, x[f:f + 1].contiguous(), T.frame(f))
        assert all(torch.equal(a[0], b[f]) for a, b in zip(one, full)), f


# ---- 7. NaN --------------------------------------------------------------------------------------------------------------------------
def test_nan_poisons_only_its_frame(hip_device):
    w, model, args = vv._shared("C3", hip_device)
    n, bad = 65, 33
    x = w.make_frames(n, seed=25).double().to(hip_device)
    T, _, _ = _reference_terms(model, args, x, w.make_frames(65, seed=27).double().to(hip_device), _c3_spec(), 26, "NaN")
    (y0, e0, dx0), _ = _call(model, x, T)
    y0, e0, dx0 = y0.clone(), e0.clone(), dx0.clone()
    keep = torch.ones(n, dtype=torch.bool, device=hip_device)
    keep[bad] = False
    xb = x.clone()
    xb[bad] = NAN
    (y, e, dx), _ = _call(model, xb, T)
    assert torch.equal(y[keep], y0[keep]) and torch.equal(e[keep], e0[keep]) and torch.equal(dx[keep], dx0[keep])
    assert bool(torch.isnan(y[bad]).all()) and bool(torch.isnan(e[bad]).all()) and bool(torch.isnan(dx[bad]).any())


# ---- 8. into=, conversions, refusals -------------------------------------------------------------------------------------------------
def test_into_conversions_and_refusals(hip_device):
    w, model, args = vv._shared("C3", hip_device)
    n, d = 5, 8
    x = w.make_frames(n, seed=51).double().to(hip_device)
    T, _, _ = _reference_terms(model, args, x, w.make_frames(65, seed=53).double().to(hip_device), _c3_spec(), 52, "into")
    rec = T.records(hip_device)
    (y, e, dx), _ = _call(model, x, T)
    new = lambda *sh: torch.full(sh, NAN, dtype=F64, device=hip_device)       # noqa: E731
    y2, e2, dx2 = new(n, d), new(n, 3), new(n, w.n_atoms, 3)
    r, _ = _call(model, x, T, into=(y2, e2, dx2))
    assert r[0] is y2 and r[1] is e2 and r[2] is dx2 and torch.equal(y2, y) and torch.equal(e2, e) and torch.equal(dx2, dx)
    # conversions: CPU float32 rows, lists and numbers cost launches and give the bits of their float64 values
    R, H, G = rec["restraint"], rec["hills"], rec["grid"]
    conv = model.value_and_bias(x, restraint=Restraint(R.center.cpu().tolist(), R.kappa.cpu().tolist(), R.period.cpu().tolist(), R.flat.cpu().tolist()),
                                hills=Hills(H.centers.cpu().tolist(), H.heights.cpu().tolist(), H.sigma.cpu().tolist(), H.period.cpu().tolist(), columns=(0, 3, 7)),
                                grid=Grid(G.table, torch.tensor(G.lower, dtype=F64), tuple(G.spacing), G.periodic, columns=range(6, 0, -5)))
    assert all(torch.equal(a, b) for a, b in zip(conv, (y, e, dx)))
    y3, e3, dx3 = new(n, d), new(n, 3), new(n, w.n_atoms, 3)
    good = dict(rec, into=(y3, e3, dx3))
    bad_calls = [
        (TypeError, dict(into=(y3, dx3))), (TypeError, dict(into=(y3, e3.float(), dx3))), (ValueError, dict(into=(y3, e3[:, 0].contiguous(), dx3))),
        (ValueError, dict(into=(y3, e3.cpu(), dx3))), (ValueError, dict(into=(y3[:4], e3, dx3))),
        (IndexError, dict(hills=Hills(H.centers, H.heights, H.sigma, columns=[0, 3, 8]))), (IndexError, dict(grid=Grid(G.table, G.lower, G.spacing, columns=[8, 1]))),
        (ValueError, dict(hills=Hills(H.centers[:, :2], H.heights, H.sigma, columns=[0, 3, 7]))), (ValueError, dict(hills=Hills(H.centers, H.heights, -H.sigma, columns=[0, 3, 7]))),
        (ValueError, dict(grid=Grid(G.table.cpu(), G.lower, G.spacing, columns=[6, 1]))), (TypeError, dict(grid=Grid(G.table.float(), G.lower, G.spacing, columns=[6, 1]))),
        (ValueError, dict(grid=Grid(G.table, G.lower, [0.1, 0.0], columns=[6, 1]))), (ValueError, dict(grid=Grid(G.table, G.lower, G.spacing, columns=[6]))),
        (ValueError, dict(restraint=Restraint(R.center[:3], R.kappa))), (ValueError, dict(restraint=Restraint(R.center, R.kappa, flat=-R.kappa))),
        (TypeError, dict(restraint=(R.center, R.kappa))), (ValueError, dict(restraint=None, hills=None, grid=None)),
        (NotImplementedError, dict(hills=Hills(torch.zeros((2, 8), dtype=F64, device=hip_device), 1.0, 1.0), restraint=None)),   # the identity list of 8 fits
    ]
    for exc, changes in bad_calls[:-1]:
        with pytest.raises(exc):
            model.value_and_bias(x, **dict(good, **changes))
    model.value_and_bias(x, **dict(rec, **bad_calls[-1][1]))
    with pytest.raises(TypeError, match="float64"):
        model.value_and_bias(x.float(), **rec)
    with pytest.raises(NotImplementedError, match="value_and_vjp"):
        model.value_and_bias(x.cpu(), **rec)
    empty = model.value_and_bias(x[:0], **dict(rec, restraint=Restraint(R.center[0].contiguous(), R.kappa)))
    assert [tuple(t.shape) for t in empty] == [(0, d), (0, 3), (0, w.n_atoms, 3)]
    # the C entry's refusals on a real plan, in the order of the header
    pre = model.preprocessing_layer
    dp = pre.output_dimension()
    f3 = new(n, dp)
    plan = vv._feature_plan(pre, x)
    L, s = _capi.lib(), torch.cuda.current_stream().cuda_stream
    z, k = torch.zeros(dp, dtype=F64, device=hip_device), torch.ones(dp, dtype=F64, device=hip_device)
    c2, h2, s2 = torch.zeros((3, 2), dtype=F64, device=hip_device), torch.ones(3, dtype=F64, device=hip_device), torch.ones(2, dtype=F64, device=hip_device)
    t2 = torch.zeros((5, 6), dtype=F64, device=hip_device)
    R0, H0, G0 = (z, k, None, None, 0), ([4, 1], c2, h2, s2, None, 3, 0), ([0, 5], t2, (5, 6), (0.0, 0.0), (1.0, 1.0), None)

    def code(r=R0, h=H0, g=G0, ptr=lambda t: t.data_ptr(), xp=None, nullterms=False):
        terms, keep = _capi.bias_terms_f64(r, h, g, ptr=ptr)
        rc = L.molann_value_and_bias_f64(plan._handle, x.data_ptr() if xp is None else xp, n, None, None, None if nullterms else ctypes.byref(terms),
                                         f3.data_ptr(), e3.data_ptr(), dx3.data_ptr(), s)
        del keep
        return rc

    with torch.cuda.device(hip_device):
        assert plan.supports_value_and_bias_f64() and not plan.supports_value_and_grid_f64()
        assert code(nullterms=True) == _capi.E_NULL
        assert code(r=(None, k, None, None, 0)) == _capi.E_NULL and code(h=([4, 1], None, h2, s2, None, 3, 0)) == _capi.E_NULL
        assert code(h=([4, 1], c2, h2, None, None, 3, 0)) == _capi.E_NULL and code(g=([0, 5], None, (5, 6), (0.0, 0.0), (1.0, 1.0), None)) == _capi.E_NULL
        assert code(g=([0, 5], t2, None, (0.0, 0.0), (1.0, 1.0), None)) == _capi.E_NULL and code(g=([0, 5], t2, (5, 6), (0.0, 0.0), None, None)) == _capi.E_NULL
        assert code(ptr=lambda t: t.data_ptr() + (4 if t is s2 else 0)) == _capi.E_ALIGNMENT and code(xp=x.data_ptr() + 4) == _capi.E_ALIGNMENT
        # a required pointer that is NULL comes before a misaligned one, a table's host arrays among them
        assert code(g=([0, 5], t2, None, (0.0, 0.0), (1.0, 1.0), None), xp=x.data_ptr() + 4) == _capi.E_NULL
        assert code(g=([0, 5], t2, (5, 6), None, (1.0, 1.0), None), ptr=lambda t: t.data_ptr() + (4 if t is s2 else 0)) == _capi.E_NULL
        assert code(r=None, h=None, g=None) == _capi.E_DESC                                             # no term
        assert code(h=([4, 1], c2, h2, s2, None, -1, 0)) == _capi.E_DESC                                # a negative count
        terms, keep = _capi.bias_terms_f64(R0, H0, G0)
        terms.n_grid_columns = -2
        assert L.molann_value_and_bias_f64(plan._handle, x.data_ptr(), n, None, None, ctypes.byref(terms), f3.data_ptr(), e3.data_ptr(), dx3.data_ptr(), s) == _capi.E_DESC
        assert code(r=(z, k, None, None, 3)) == _capi.E_DESC and code(h=([4, 1], c2, h2, s2, None, 3, 3)) == _capi.E_DESC     # strides
        assert code(g=([0, 5], t2, (3, 6), (0.0, 0.0), (1.0, 1.0), None)) == _capi.E_DESC and code(g=([0, 5], t2, (5, 6), (0.0, 0.0), (1.0, NAN), None)) == _capi.E_DESC
        assert code(h=([4, dp], c2, h2, s2, None, 3, 0)) == _capi.E_INDEX and code(h=([4, 4], c2, h2, s2, None, 3, 0)) == _capi.E_INDEX
        assert code(g=([-1, 5], t2, (5, 6), (0.0, 0.0), (1.0, 1.0), None)) == _capi.E_INDEX and code(g=([5, 5], t2, (5, 6), (0.0, 0.0), (1.0, 1.0), None)) == _capi.E_INDEX
        # a stride, then a column: DESC comes first
        assert code(h=([4, 4], c2, h2, s2, None, 3, 5)) == _capi.E_DESC
        p1 = _capi.Plan(22, features=[(wl.BOND, [0, 1])] * 10)
        c9 = torch.zeros((3, 9), dtype=F64, device=hip_device)
        f10 = new(n, 10)

        def code1(h=None, g=None):
            terms, keep = _capi.bias_terms_f64(None, h, g)
            return L.molann_value_and_bias_f64(p1._handle, x.data_ptr(), n, None, None, ctypes.byref(terms), f10.data_ptr(), e3.data_ptr(), dx3.data_ptr(), s)

        assert code1(h=(list(range(9)), c9, h2, k[:1], None, 3, 0)) == _capi.E_UNSUPPORTED and code1(h=((None, 9), c9, h2, k[:1], None, 3, 0)) == _capi.E_UNSUPPORTED
        assert code1(g=([0, 1, 2, 3], t2, (4, 4, 4, 4), (0.0,) * 4, (1.0,) * 4, None)) == _capi.E_UNSUPPORTED
        assert code1(h=(list(range(8)) + [10], c9, h2, k[:1], None, 3, 0)) == _capi.E_INDEX                 # a column, then the cap: INDEX comes first
        p2 = _capi.Plan(22, features=[(wl.BOND, [0, 1])] * 2)
        terms, keep = _capi.bias_terms_f64(None, ((None, 3), c9, h2, k[:1], None, 3, 0), None)
        assert L.molann_value_and_bias_f64(p2._handle, x.data_ptr(), n, None, None, ctypes.byref(terms), f10.data_ptr(), e3.data_ptr(), dx3.data_ptr(), s) == _capi.E_INDEX
        assert L.molann_value_and_bias_f64(plan._handle, None, 0, None, None, ctypes.byref(terms), None, None, None, s) == 0
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (y3, e3, dx3, f3, f10)), "a refusal launched"


# ---- 9. the caller's buffers ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", [1, "mixedA", "mixedB"])
def test_offset_buffers_inside_guard_bands(where, hip_device):
    """x, the centres, the hill table, the table, out, energies and grad_x at offset positions inside guard bands: the bands intact,
    the inputs unchanged, the bits of the call on fresh tensors."""
    model, args, x, x_tab = _small7(hip_device, 93)
    T, _, _ = _reference_terms(model, args, x, x_tab, _small7_spec(), 94, "guard bands")
    want, _ = _call(model, x, T)
    want = [t.clone() for t in want]
    arena = placement.Arena(hip_device)
    names = ("x", "center", "kappa", "period", "flat", "centers", "heights", "sigma", "hills_period", "table", "out", "energies", "grad_x")
    off = placement.offsets(where, names, wide=2)
    z, kappa, period, flat = T.r
    _, c, h, s, hperiod = T.h
    carve = lambda name, t: arena.carve(name, t.shape, F64, off[name], data=t.to(hip_device))       # noqa: E731
    R = Restraint(carve("center", z), carve("kappa", kappa), carve("period", period), carve("flat", flat))
    H = Hills(carve("centers", c), carve("heights", h), carve("sigma", s), carve("hills_period", hperiod), columns=T.h[0])
    G = Grid(carve("table", T.g[1]), T.g[2], T.g[3], T.g[4], columns=T.g[0])
    into = (arena.carve("out", (65, 6), F64, off["out"]), arena.carve("energies", (65, 3), F64, off["energies"]), arena.carve("grad_x", x.shape, F64, off["grad_x"]))
    got = model.value_and_bias(carve("x", x), restraint=R, hills=H, grid=G, into=into)
    torch.cuda.synchronize()
    assert vh._info(model).startswith(INFO) and all(a is b for a, b in zip(got, into))
    assert arena.check() == [] and arena.inputs_changed() == []
    assert all(placement.same_bits(a, b) for a, b in zip(got, want))


# ---- 10. the dispatcher operators ----------------------------------------------------------------------------------------------------
def test_scripted_model_and_operators(tmp_path, hip_device):
    import warnings
    w, model, args = vv._shared("C3", hip_device)
    x = w.make_frames(65, seed=71).double().to(hip_device)
    T, _, _ = _reference_terms(model, args, x, w.make_frames(65, seed=73).double().to(hip_device), _c3_spec(), 72, "operators")
    want, _ = _call(model, x, T)
    want = [t.clone() for t in want]
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.jit.script(model).save(str(tmp_path / "c3_f64.pt"))
    loaded = torch.jit.load(str(tmp_path / "c3_f64.pt"), map_location=hip_device)
    ws = [lin.weight for lin in loaded.linears.children()]
    bs = [lin.bias for lin in loaded.linears.children()]
    desc = list(loaded.desc)
    handle = torch.ops.molann.register_desc(desc)
    rec = T.records(hip_device)
    R, H, G = rec["restraint"], rec["hills"], rec["grid"]
    tail = (R.center, R.kappa, R.period, R.flat, list(H.columns), H.centers, H.heights, H.sigma, H.period, list(G.columns), G.table, G.lower, G.spacing, G.periodic, [])
    by_handle = torch.ops.molann.value_and_bias_h(x, handle, loaded.ref_x, ws, bs, *tail)
    by_desc = torch.ops.molann.value_and_bias(x, desc, loaded.ref_x, ws, bs, *tail)
    torch.cuda.synchronize()
    info = torch.ops.molann.launch_info(desc, hip_device.index)
    assert info.count(KERNEL) == 1 and info.count("_kernel") == 1, info
    assert len(by_handle) == 3 and len(by_desc) == 3
    assert all(torch.equal(a, b) for a, b in zip(by_handle, want)) and all(torch.equal(a, b) for a, b in zip(by_desc, want))
    # absent terms: none / empty lists
    only_grid = torch.ops.molann.value_and_bias(x, desc, loaded.ref_x, ws, bs, None, None, None, None, [], None, None, None, None, list(G.columns), G.table,
                                                G.lower, G.spacing, [], [])
    plain = model.value_and_bias(x, grid=Grid(G.table, G.lower, G.spacing, columns=G.columns))
    assert all(torch.equal(a, b) for a, b in zip(only_grid, plain)) and float(plain[1][:, :2].abs().max()) == 0.0
    with pytest.raises((IndexError, RuntimeError)):
        torch.ops.molann.value_and_bias(x, desc, loaded.ref_x, ws, bs, None, None, None, None, [], None, None, None, None, [8, 1], G.table, G.lower, G.spacing, [], [])
