"""MolANN.value_and_bias / PreprocessingANN.value_and_bias with an OPES term (`opes=`) / molann_value_and_bias_opes_f64 on the GPU: a
restraint on all outputs (walls), the kernel density of value_and_opes on chosen outputs and a table on chosen outputs, energies [N, 4] =
(E_r, 0, V_g, V_o) and the gradient of their sum in one launch of frames_value_bias_opes_f64_kernel.

The reference is the CPU float64 oracle of the sibling tests (`vr._reference_y`); every centre, kernel table and grid is built from ITS
y - the chosen columns taken with ``y[:, cols]`` - by the siblings' builders (`vb._build`, `vo._table`), which assert their conditions
on the reference values: every (frame, kernel) pair at least 1e-6 from q = c^2, pairs inside and outside the cutoff, nothing within 1e-9
of a wrap seam, a flat edge or a range end.  Bounds, the family's, each energy column on its own scale: y within 1e-10 max(1, |y|max),
each energy within 1e-10 max(1, |E|max), dx within 1e-9 max(1e-3, |dx|max).  Every call asserts one launch by its info string."""

import ctypes
import math

import pytest
import torch

import isolation
import placement
import test_gpu_random_backward as rb
import test_gpu_value_and_bias_f64 as vb
import test_gpu_value_and_grid_f64 as vg
import test_gpu_value_and_hills_f64 as vh
import test_gpu_value_and_opes_f64 as vo
import test_gpu_value_and_restraint_f64 as vr
import test_gpu_value_and_vjp_f64 as vv
from molann_amd import _capi, workloads as wl
from molann_amd.bias import Grid, Hills, Opes, Restraint

pytestmark = pytest.mark.gpu
KERNEL = "frames_value_bias_opes_f64_kernel"
INFO = KERNEL + " (values + bias + opes in one launch; "
PARENT_INFO = "frames_value_bias_f64_kernel (values + bias in one launch; "
TWO_PI = 2.0 * math.pi
NAN, INF = float("nan"), float("inf")
CPU = torch.device("cpu")
F64 = torch.float64
SCALE, EPS = vo.SCALE, 1e-3
NAMES = ("E_r", "V_h", "V_g", "V_o")


class OpesTerm(object):
    """The OPES term on the CPU, built from reference outputs: columns, (centers, heights, sigma), the period row over the columns,
    norm, epsilon, cutoff."""

    def __init__(self, cols, table, period, norm, cutoff, epsilon=EPS, scale=SCALE):
        self.cols, self.table, self.period, self.norm, self.cutoff, self.epsilon, self.scale = tuple(cols), table, period, norm, cutoff, epsilon, scale

    def record(self, dev, identity=False):
        on = lambda t: None if t is None else t.to(dev)       # noqa: E731
        p = self.period if self.period is not None and bool((self.period > 0).any()) else None
        return Opes(on(self.table[0]), on(self.table[1]), on(self.table[2]), self.scale, self.norm, self.epsilon, self.cutoff, on(p),
                    columns=None if identity else list(self.cols))

    def bias(self, y):
        return vo._bias(y[:, list(self.cols)], self.table, self.period, self.norm, self.epsilon, self.cutoff, self.scale)


def _opes(y_ref, y_tab, cols, period, n_kernels, per_kernel, seed, cutoff):
    """The siblings' table on the reference's y[:, cols], its conditions asserted for this cutoff"""
    cols = list(cols)
    table, norm = vo._table(y_ref.detach()[:, cols], y_tab.detach()[:, cols], period, n_kernels, per_kernel, seed, (cutoff,))
    return OpesTerm(cols, table, period, norm, cutoff)


def _oracle(xx, y, T, O):
    """(y, energies [n, 4], d(sum)/dx) by float64 autograd of the formulas, the table's margins asserted by the sibling's oracle"""
    n = y.shape[0]
    zero = torch.zeros(n, dtype=F64)
    v = O.bias(y)
    (gx,) = torch.autograd.grad(v.sum(), xx, retain_graph=True)
    e = [zero, zero, zero, v.detach()]
    if T.r is not None or T.g is not None:
        (_, e3, gx3), _, _ = vb._oracle(xx, y, T)
        e[0], e[2], gx = e3[:, 0], e3[:, 2], gx + gx3
    return y.detach(), torch.stack(e, dim=1), gx


def _close(got, want, what, present):
    (y, e, dx), (y_want, e_want, gx_want) = got, want
    assert all(t.dtype == F64 for t in got) and y.shape == y_want.shape and e.shape == e_want.shape and dx.shape == gx_want.shape
    y, e, dx = y.detach().cpu(), e.detach().cpu(), dx.detach().cpu()
    ey, sy = float((y - y_want).abs().max()), max(1.0, float(y_want.abs().max()))
    ed, sd = float((dx - gx_want).abs().max()), max(1e-3, float(gx_want.abs().max()))
    print("%s: y err %.3e (scale %.3g), dx err %.3e (scale %.3g)" % (what, ey, sy, ed, sd))
    assert ey <= 1e-10 * sy, (what, "y", ey, sy)
    for c, name in enumerate(NAMES):
        if not present[c]:
            assert bool((e[:, c] == 0.0).all()) and not bool(torch.signbit(e[:, c]).any()), (what, name, "an absent term's column is not 0.0")
            continue
        ee, se = float((e[:, c] - e_want[:, c]).abs().max()), max(1.0, float(e_want[:, c].abs().max()))
        print("    %s err %.3e (scale %.3g)" % (name, ee, se))
        assert ee <= 1e-10 * se, (what, name, ee, se)
    assert ed <= 1e-9 * sd, (what, "dx", ed, sd)


def _call(model, x, T, O, into=None, identity=False):
    rec = T.records(x.device, identity)
    out = model.value_and_bias(x, restraint=rec["restraint"], grid=rec["grid"], into=into, opes=O.record(x.device, identity))
    torch.cuda.synchronize()
    info = vh._info(model)
    assert info.startswith(INFO) and info.count("_kernel") == 1, info
    return out, info


def _reference(model, args, x, x_tab, spec, ospec, seed, what):
    """(walls and table, OPES term, the oracle's (y, energies, dx)) for a model and a batch: everything from the reference's y, the
    siblings' conditions and 'nothing nearly zero' asserted on the reference values.  ospec = (columns, period row, kernels, per_kernel,
    cutoff)."""
    xx, y_ref = vr._reference_y(model, *args, x)
    _, y_tab = vr._reference_y(model, *args, x_tab)
    T, _, _ = vb._build(y_ref, y_tab, seed=seed, **spec)
    cols, period, n_kernels, per_kernel, cutoff = ospec
    O = _opes(y_ref, y_tab, cols, period, n_kernels, per_kernel, seed + 3, cutoff)
    want = _oracle(xx, y_ref, T, O)
    for c in (0, 2, 3):
        assert not (T.r, None, T.g, O)[c] or float(want[1][:, c].abs().max()) > 0.05, (what, c, "the reference energy is (nearly) zero")
    assert float(want[2].abs().max()) > 1e-3
    return T, O, want


def _check(model, args, x, x_tab, spec, ospec, seed, what):
    T, O, want = _reference(model, args, x, x_tab, spec, ospec, seed, what)
    got, info = _call(model, x, T, O)
    _close(got, want, what, (T.r is not None, False, T.g is not None, True))
    return got, info, T, O


# ---- 1. every lane group -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_inp,lanes", [(7, 8), (12, 16), (30, 32), (40, 64)])
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "no_alignment"])
@pytest.mark.parametrize("head", [True, False], ids=["head", "features"])
def test_lane_groups(n_inp, lanes, aligned, head, hip_device):
    """65 frames, 2 lanes + 5 kernels (a ragged walk), cutoff 4.  A [d_feat, 5, 4] head: OPES on (3, 1), the table on (0, 2) with one
    periodic axis, a restraint with flat bottoms, output 1 free of it.  Features only (6 columns): OPES on (5, 0, 2), the table on (1, 3)."""
    if head:
        case = vv._small_case(n_inp, [0, 2, 4, 6] if aligned else None, head=True)
        case.mlp = [case.d_feat(), 5, 4]
        d_out, oc, gc = 4, (3, 1), (0, 2)
        lanes = max(lanes, 16)       # the head's widest layer input (the 12 feature columns) asks for at least 16 lanes
        spec = dict(r=(vr._period_row(d_out, 1.3, 2), True, [1]), g=(gc, (5, 6), [True, False]))
    else:
        case = vh._small_case(n_inp, aligned, False)
        d_out, oc, gc = 6, (5, 0, 2), (1, 3)
        spec = dict(g=(gc, (5, 6), [True, False]))
    model = case.build(hip_device).double().requires_grad_(False)
    x = case.frames(65, seed=n_inp + 3, dev=CPU).double().to(hip_device)
    x_tab = case.frames(65, seed=900 + n_inp, dev=CPU).double().to(hip_device)
    ospec = (oc, vr._period_row(len(oc), 1.3, 2), 2 * lanes + 5, True, 4.0)
    (y, e, dx), info, T, O = _check(model, (case.feats, case.uav, case.align), x, x_tab, spec, ospec, n_inp, (case.name, aligned, head))
    assert "%d lanes per frame" % lanes in info, info
    assert not head or float(T.r[1][1]) == 0.0
    untouched = sorted(set(range(n_inp)) - case.touched())
    if untouched:
        assert float(dx[:, untouched].abs().max()) == 0.0


# ---- 2. past the single entries' caps ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65])
def test_c3_eight_outputs(n, hip_device):
    """C3's own model, 8 outputs: OPES on (0, 3, 7), a table on (6, 1), the restraint on all - value_and_grid refuses this model."""
    w, model, args = vv._shared("C3", hip_device)
    assert w.out_dim() == 8
    x = w.make_frames(n, seed=30 + n).double().to(hip_device)
    x_tab = w.make_frames(65, seed=32).double().to(hip_device)
    _check(model, args, x, x_tab, _c3_spec(), _c3_ospec(n == 65), 33 + n, ("C3", n))
    with pytest.raises(NotImplementedError):
        model.value_and_grid(x, torch.zeros((4,) * 3, dtype=F64, device=hip_device), [0.0] * 3, [1.0] * 3)


@pytest.mark.parametrize("n", [1, 65])
def test_positions_and_two_dihedral_angles(n, hip_device):
    """Features only: 21 position columns and two dihedral angle values behind them; OPES and a periodic table from -pi on the two angles
    (period 2 pi), the restraint on all 23 - value_and_opes refuses this module."""
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
    T, _, _ = vb._build(y_ref, y_tab, r=(period, True, []), seed=71 + n)
    shape = (8, 9)
    T.g = ((21, 22), vg._seeded_table(shape, 73), [-math.pi] * 2, [TWO_PI / s for s in shape], [True, True])
    assert float(y_ref.detach()[:, 21:].abs().max()) <= math.pi
    O = _opes(y_ref, y_tab, (21, 22), vr._period_row(2, TWO_PI), 23, True, 74 + n, 4.0)
    want = _oracle(xx, y_ref, T, O)
    assert all(float(want[1][:, c].abs().max()) > 0.05 for c in (0, 2, 3)) and float(want[2].abs().max()) > 1e-3
    got, info = _call(model, x, T, O)
    # nine items ask for 16 lanes; a frame's rows are its 23 outputs and the selection row: the bias kernel's
    assert "16 lanes per frame" in info and info.endswith("lds=%d" % ((256 // 16) * (23 + vb.SEL) * 8)), info
    _close(got, want, ("pos7dih", n), (True, False, True, True))
    with pytest.raises(NotImplementedError):
        model.value_and_opes(x, torch.zeros((1, 23), dtype=F64, device=hip_device), 1.0, 1.0, SCALE, 1.0, EPS)


# ---- 3. OPES alone is the single entry, bit for bit ----------------------------------------------------------------------------------
def _angles(dev, bond):
    w, case, model = vr._c3_angles(dev, bond=bond)
    period = torch.tensor([TWO_PI, TWO_PI, 0.0][:3 if bond else 2], dtype=F64)
    return model, w.make_frames(65, seed=43).double().to(dev), w.make_frames(65, seed=44).double().to(dev), (case.feats, True, case.align), period


def _single_opes(model, x, O):
    out = vo._call(model, x, O.table, O.period, O.norm, O.epsilon, O.cutoff, scale=O.scale)[0]
    return tuple(t.clone() for t in out)


@pytest.mark.parametrize("bond", [False, True], ids=["two_outputs", "three_outputs"])
def test_opes_alone_is_the_single_entry(bond, hip_device):
    model, x, x_tab, args, period = _angles(hip_device, bond)
    d = period.numel()
    _, y_ref = vr._reference_y(model, *args, x)
    _, y_tab = vr._reference_y(model, *args, x_tab)
    for n_kernels, cutoff in ((45, 4.0), (45, None), (0, 4.0)):
        O = _opes(y_ref, y_tab, range(d), period, n_kernels, True, 5, cutoff)
        got, _ = _call(model, x, vb.Terms(), O, identity=True)
        listed, _ = _call(model, x, vb.Terms(), O)
        assert all(torch.equal(a, b) for a, b in zip(got, listed))          # None is the list 0..d-1
        got = [t.clone() for t in got]
        single = _single_opes(model, x, O)
        assert torch.equal(got[0], single[0]) and torch.equal(got[1][:, 3], single[1]) and torch.equal(got[2], single[2]), (bond, n_kernels, cutoff)
        assert bool((got[1][:, :3] == 0.0).all()) and not bool(torch.signbit(got[1][:, :3]).any())
        if n_kernels:
            assert float(got[2].abs().max()) > 1e-3 and float(got[1][:, 3].std()) > 0.05


# ---- 4. restraint + table + OPES against the three single calls ----------------------------------------------------------------------
@pytest.mark.parametrize("name", ["C3_angles_bond", "small7"])
def test_three_terms_against_the_single_calls(name, hip_device):
    """Identity columns on a 3-output model: energies columns 0, 2 and 3 are the single calls', bit for bit; dx is their dx added up to
    1e-15 |dx|max (one rounding of J^T applied to a sum against three of it applied to the parts)."""
    model, x, x_tab, args, period = vb._three_outputs(name, hip_device)
    xx, y_ref = vr._reference_y(model, *args, x)
    _, y_tab = vr._reference_y(model, *args, x_tab)
    cols = (0, 1, 2)
    T, _, _ = vb._build(y_ref, y_tab, r=(period, True, []), g=(cols, vg.SHAPES[3], [bool(period[0] > 0), True, False]), seed=15)
    O = _opes(y_ref, y_tab, cols, period, 45, False, 16, 4.0)
    want = _oracle(xx, y_ref, T, O)
    got, _ = _call(model, x, T, O, identity=True)
    got = [t.clone() for t in got]
    _close(got, want, (name, "three terms"), (True, False, True, True))
    single = vb._single_calls(model, x, T)
    single_o = _single_opes(model, x, O)
    for c, s in ((0, single[0]), (2, single[2]), (3, single_o)):
        assert torch.equal(got[0], s[0]) and torch.equal(got[1][:, c], s[1]), (name, c)
    dx_sum = single[0][2] + single_o[2] + single[2][2]
    ed, sd = float((got[2] - dx_sum).abs().max()), float(dx_sum.abs().max())
    print("%s: dx against the sum of the three single calls %.3e (|dx|max %.3g, ratio %.3e)" % (name, ed, sd, ed / sd))
    assert ed <= 1e-15 * sd, (name, ed, sd)


# ---- 5. corner cases -----------------------------------------------------------------------------------------------------------------
def _c3_spec():
    """C3's 8 outputs: the restraint on all (flat bottoms: walls), the table on (6, 1)"""
    return dict(r=(vr._period_row(8, 1.1, 3), True, []), g=((6, 1), (6, 7), [False, True]))


def _c3_ospec(per_kernel=True, n_kernels=37, cutoff=4.0):
    """OPES on (0, 3, 7), output 0 periodic"""
    return ((0, 3, 7), vr._period_row(3, 0.9, 2), n_kernels, per_kernel, cutoff)


def _parent_call(model, x, T):
    out = model.value_and_bias(x, **T.records(x.device))
    torch.cuda.synchronize()
    info = vh._info(model)
    assert info.startswith(PARENT_INFO) and info.count("_kernel") == 1, info
    return [t.clone() for t in out]


def test_no_kernels_yet(hip_device):
    """n_kernels == 0: V_o = scale log(epsilon) and the OPES share of dx is exactly 0 - with walls and a table dx has the bits of
    value_and_bias with the two alone (its kernel adds nothing for the absent hills), with OPES alone it is 0 everywhere."""
    w, model, args = vv._shared("C3", hip_device)
    x = w.make_frames(65, seed=81).double().to(hip_device)
    T, O, want = _reference(model, args, x, w.make_frames(65, seed=82).double().to(hip_device), _c3_spec(), _c3_ospec(n_kernels=0), 83, "H = 0")
    assert O.table[0].shape == (0, 3)
    (y, e, dx), _ = _call(model, x, T, O)
    _close((y, e, dx), want, "H = 0", (True, False, True, True))
    v0 = SCALE * math.log(EPS)
    assert float((e[:, 3] - v0).abs().max()) <= 1e-14 * abs(v0)
    yp, ep, dxp = _parent_call(model, x, T)
    assert torch.equal(y, yp) and torch.equal(e[:, :3], ep) and torch.equal(dx, dxp)
    (y, e, dx), _ = _call(model, x, vb.Terms(), O)
    assert torch.equal(y, yp) and bool((dx == 0).all()) and bool((e[:, :3] == 0).all()) and float((e[:, 3] - v0).abs().max()) <= 1e-14 * abs(v0)


def test_a_frame_outside_every_cutoff(hip_device):
    """The sibling's table: kernels half a width from the reference outputs of frames 1.., a twentieth of the outputs' spread wide.
    Frame 0 is outside every kernel's cutoff of 4 (asserted on the reference): its V_o is scale log(epsilon) and its dx the bits of the
    walls and the table alone; the other frames against the oracle."""
    w, model, args = vv._shared("C3", hip_device)
    n, cutoff, cols = 9, 4.0, [0, 3, 7]
    x = w.make_frames(n, seed=65).double().to(hip_device)
    xx, y_ref = vr._reference_y(model, *args, x)
    T, _, _ = vb._build(y_ref, vr._reference_y(model, *args, w.make_frames(65, seed=66).double().to(hip_device))[1], seed=67, **_c3_spec())
    yr = y_ref.detach()[:, cols]
    sigma = 0.05 * yr.std(dim=0).clamp(min=1e-3)
    table = (yr[1:] + 0.5 * sigma, torch.linspace(0.3, 1.1, n - 1, dtype=F64), sigma)
    O = OpesTerm(cols, table, None, vo._norm(table[1]), cutoff)
    _, q = vo._density(yr, *table, None, cutoff)
    assert float(q[0].min()) >= cutoff * cutoff + 1e-6 and bool((q[1:].min(dim=1).values < 2.5).all())
    vo._conditions(yr, table, None, cutoff)
    want = _oracle(xx, y_ref, T, O)
    (y, e, dx), _ = _call(model, x, T, O)
    _close((y, e, dx), want, "frame 0 outside every cutoff", (True, False, True, True))
    v0 = SCALE * math.log(EPS)
    assert abs(float(e[0, 3]) - v0) <= 1e-14 * abs(v0)
    yp, ep, dxp = _parent_call(model, x, T)
    assert torch.equal(dx[0], dxp[0]) and torch.equal(e[:, :3], ep) and not torch.equal(dx[1:], dxp[1:])


def test_no_cutoff_is_a_cutoff_past_every_pair(hip_device):
    """cutoff=None and cutoff=40: exp(-800) underflows to 0, so nothing is dropped and nothing subtracted - the same bits."""
    w, model, args = vv._shared("C3", hip_device)
    x = w.make_frames(65, seed=47).double().to(hip_device)
    T, O, _ = _reference(model, args, x, w.make_frames(65, seed=48).double().to(hip_device), _c3_spec(), _c3_ospec(cutoff=None), 49, "no cutoff")
    assert math.exp(-0.5 * 40.0 * 40.0) == 0.0
    none, _ = _call(model, x, T, O)
    none = [t.clone() for t in none]
    O.cutoff = 40.0
    at40, _ = _call(model, x, T, O)
    O.cutoff = INF
    at_inf, _ = _call(model, x, T, O)
    assert all(torch.equal(a, b) for a, b in zip(none, at40)) and all(torch.equal(a, b) for a, b in zip(none, at_inf))


@pytest.mark.parametrize("cutoff", [4.0, None], ids=["cutoff4", "no_cutoff"])
def test_nan_poisons_only_its_frame(cutoff, hip_device):
    w, model, args = vv._shared("C3", hip_device)
    n, bad = 70, 33
    x = w.make_frames(n, seed=25).double().to(hip_device)
    T, O, _ = _reference(model, args, x, w.make_frames(65, seed=27).double().to(hip_device), _c3_spec(), _c3_ospec(cutoff=cutoff), 26, "NaN")
    names = ("out", "energies", "grad_x")
    clean, _ = _call(model, x, T, O)
    clean = dict((k, t.clone()) for k, t in zip(names, clean))
    xb = x.clone()
    xb[bad] = NAN
    got, _ = _call(model, xb, T, O)
    got = dict(zip(names, got))
    complaints = isolation.keep_rows_equal(clean, got, [bad], names)
    assert not complaints, complaints
    assert all(bool(torch.isfinite(t).all()) for t in clean.values())
    assert bool(torch.isnan(got["out"][bad]).all()) and bool(torch.isnan(got["energies"][bad, [0, 2, 3]]).all()) and bool(torch.isnan(got["grad_x"][bad]).any())
    assert float(got["energies"][bad, 1]) == 0.0


# ---- 6. larger frames and stepped-down rows ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [("P1", 9), ("C4", 3)])
def test_larger_frames(name, n, hip_device):
    w, model, args = vv._shared(name, hip_device)
    d = w.out_dim()
    assert d >= 2
    x = w.make_frames(n, seed=7).double().to(hip_device)
    x_tab = w.make_frames(33 if name == "C4" else 65, seed=8).double().to(hip_device)
    spec = dict(r=(vr._period_row(d, 1.1, 3), True, [0]), g=((0, d - 1), (6, 9), [False, True]))
    (_, _, dx), info, _, _ = _check(model, args, x, x_tab, spec, ((d - 1, 0), vr._period_row(2, 0.8, 2), 75, True, 4.0), 60, name)
    assert "64 lanes per frame" in info, info
    untouched = sorted(set(range(w.n_atoms)) - {a - 1 for a in w.touched_atoms()})
    if untouched:
        assert float(dx[:, untouched].abs().max()) == 0.0


@pytest.mark.parametrize("name", sorted(vr.STEPPED))
def test_heads_that_step_the_rows_down(name, hip_device):
    """The [3, 682, 2] head through Plan.value_and_bias_opes_f64 with 5 frames, 4099 kernels and a (5, 6) table: two waves per block;
    the over_64k head with walls, a table and 37 kernels: one wave per block, more LDS than a launch may ask for by default.  The
    rows and the geometry are the bias kernel's."""
    dims = vr.STEPPED[name][0]
    n, n_inp = 5, 8
    head, xx, y_ref, y_tab = vh._bonds_head(dims, n, n_inp, 3)
    period = torch.tensor([0.7, 0.0], dtype=F64)
    T, _, _ = vb._build(y_ref, y_tab, r=(period, True, []), g=((1, 0), (5, 6), [True, False]), seed=80)
    O = _opes(y_ref, y_tab, (1, 0), torch.tensor([0.0, 0.7], dtype=F64), 4099 if name == "step_down" else 37, True, 81, 4.0)
    want = _oracle(xx, y_ref, T, O)
    assert float(want[1][:, 2].abs().max()) > 0.05
    per_frame = vb._rows(dims) * 8
    waves = 4
    while waves > 1 and waves * per_frame > 65536:
        waves //= 2
    assert (name, waves) in (("step_down", 2), ("over_64k", 1)) and (per_frame > 65536) == (name == "over_64k")
    dev = hip_device
    on = lambda t: None if t is None else t.to(dev)       # noqa: E731
    with torch.cuda.device(dev):
        plan = _capi.Plan(n_inp, features=vr.BONDS, layer_dims=dims, activation=_capi.ACT_TANH)
        assert plan.supports_value_and_bias_opes_f64()
        lins = [m for m in head if isinstance(m, torch.nn.Linear)]
        W, B = [lin.weight.to(dev).contiguous() for lin in lins], [lin.bias.to(dev).contiguous() for lin in lins]
        y, e, dx = (torch.full(sh, NAN, dtype=F64, device=dev) for sh in ((n, 2), (n, 4), (n, n_inp, 3)))
        plan.value_and_bias_opes(xx.detach().to(dev), W, B, y, e, dx, (O.cols,) + tuple(on(t) for t in O.table) + (on(O.period), SCALE, O.norm, EPS, 4.0),
                                 restraint=tuple(on(t) for t in T.r), grid=(T.g[0], on(T.g[1])) + T.g[2:])
        torch.cuda.synchronize()
        info = plan.last_launch_info()
    assert info == "%s64 lanes per frame) grid=%d block=%d lds=%d" % (INFO, -(-n // waves), 64 * waves, waves * per_frame), info
    _close((y, e, dx), want, name, (True, False, True, True))


# ---- 7. determinism ------------------------------------------------------------------------------------------------------------------
def _small7_specs():
    """the 7-atom aligned features (6 columns): output 1 free of the restraint, OPES on (5, 0, 2), the table on (1, 3)"""
    return dict(r=(vr._period_row(6, 1.3, 2), True, [1]), g=((1, 3), (5, 6), [True, False])), ((5, 0, 2), vr._period_row(3, 1.3, 2), 21, True, 4.0)


def test_two_calls_give_the_same_bits(hip_device):
    w, model, args = vv._shared("C3", hip_device)
    x = w.make_frames(4097, seed=21).double().to(hip_device)
    T, O, _ = _reference(model, args, x[:65].contiguous(), w.make_frames(65, seed=28).double().to(hip_device), _c3_spec(), _c3_ospec(), 22, "two calls")
    T.r = (T.r[0][0].contiguous(),) + T.r[1:]        # one row of centres for all 4097 frames
    first, _ = _call(model, x, T, O)
    first = [t.clone() for t in first]
    assert all(bool(torch.isfinite(t).all()) for t in first) and all(float(first[1][:, c].abs().max()) > 0.05 for c in (0, 2, 3))
    second, _ = _call(model, x, T, O)
    assert all(torch.equal(a, b) for a, b in zip(first, second))


@pytest.mark.parametrize("name", ["C3", "small7"])
def test_a_frame_alone_has_its_bits_in_the_batch(name, hip_device):
    if name == "C3":
        w, model, args = vv._shared("C3", hip_device)
        x, x_tab, spec, ospec = w.make_frames(65, seed=23).double().to(hip_device), w.make_frames(65, seed=29).double().to(hip_device), _c3_spec(), _c3_ospec()
    else:
        model, args, x, x_tab = vb._small7(hip_device, 23)
        spec, ospec = _small7_specs()
    T, O, _ = _reference(model, args, x, x_tab, spec, ospec, 24, name)
    full, _ = _call(model, x, T, O)
    full = [t.clone() for t in full]
    for f in (0, 9, 33, 64):
        one, _ = _call(model, x[f:f + 1].contiguous(), T.frame(f), O)
        assert all(torch.equal(a[0], b[f]) for a, b in zip(one, full)), f


# ---- 8. into=, conversions, refusals, the caller's buffers ----------------------------------------------------------------------------
def test_into_conversions_and_refusals(hip_device):
    w, model, args = vv._shared("C3", hip_device)
    n, d = 5, 8
    x = w.make_frames(n, seed=51).double().to(hip_device)
    T, O, _ = _reference(model, args, x, w.make_frames(65, seed=53).double().to(hip_device), _c3_spec(), _c3_ospec(), 52, "into")
    rec = T.records(hip_device)
    R, G, P = rec["restraint"], rec["grid"], O.record(hip_device)
    (y, e, dx), _ = _call(model, x, T, O)
    y, e, dx = y.clone(), e.clone(), dx.clone()
    new = lambda *sh: torch.full(sh, NAN, dtype=F64, device=hip_device)       # noqa: E731
    y2, e2, dx2 = new(n, d), new(n, 4), new(n, w.n_atoms, 3)
    r, _ = _call(model, x, T, O, into=(y2, e2, dx2))
    assert r[0] is y2 and r[1] is e2 and r[2] is dx2 and torch.equal(y2, y) and torch.equal(e2, e) and torch.equal(dx2, dx)
    # conversions: lists, numbers and CPU tensors cost launches and give the bits of their float64 values
    conv = model.value_and_bias(x, restraint=Restraint(R.center.cpu().tolist(), R.kappa.cpu().tolist(), R.period.cpu().tolist(), R.flat.cpu().tolist()),
                                grid=Grid(G.table, torch.tensor(G.lower, dtype=F64), tuple(G.spacing), G.periodic, columns=range(6, 0, -5)),
                                opes=Opes(P.centers.cpu().tolist(), P.heights.cpu().tolist(), P.sigma.cpu().tolist(), 2.25, float(P.norm), EPS, 4,
                                          P.period.cpu().tolist(), columns=(0, 3, 7)))
    assert all(torch.equal(a, b) for a, b in zip(conv, (y, e, dx)))
    y3, e3, dx3 = new(n, d), new(n, 4), new(n, w.n_atoms, 3)
    good = dict(restraint=R, grid=G, opes=P, into=(y3, e3, dx3))
    bad_calls = [
        (ValueError, dict(into=(y3, new(n, 3), dx3))),                 # the [N, 3] of the call without `opes`
        (TypeError, dict(into=(y3, dx3))), (TypeError, dict(into=(y3, e3.float(), dx3))), (ValueError, dict(into=(y3, e3.cpu(), dx3))),
        (ValueError, dict(into=(y3[:4], e3, dx3))), (ValueError, dict(into=(y3, e3[:, 0].contiguous(), dx3))),
        (IndexError, dict(opes=P._replace(columns=(0, 3, 8)))), (IndexError, dict(grid=Grid(G.table, G.lower, G.spacing, columns=[8, 1]))),
        (ValueError, dict(opes=P._replace(centers=P.centers[:, :2]))), (ValueError, dict(opes=P._replace(sigma=-P.sigma))),
        (ValueError, dict(opes=P._replace(norm=0.0))), (ValueError, dict(opes=P._replace(cutoff=-4.0))), (TypeError, dict(opes=P._replace(scale="2"))),
        (ValueError, dict(opes=P._replace(centers=P.centers.cpu()))), (TypeError, dict(opes=tuple(P))),
        (ValueError, dict(restraint=Restraint(R.center[:3], R.kappa))), (ValueError, dict(grid=Grid(G.table, G.lower, [0.1, 0.0], columns=[6, 1]))),
        (NotImplementedError, dict(hills=Hills(P.centers, P.heights, P.sigma, columns=[0, 3, 7]))),
    ]
    for exc, changes in bad_calls:
        with pytest.raises(exc):
            model.value_and_bias(x, **dict(good, **changes))
    with pytest.raises(TypeError, match="float64"):
        model.value_and_bias(x.float(), restraint=R, grid=G, opes=P)
    with pytest.raises(NotImplementedError, match="opes_kernel_sum"):
        model.value_and_bias(x.cpu(), restraint=R, grid=G, opes=P)
    empty = model.value_and_bias(x[:0], restraint=Restraint(R.center[0].contiguous(), R.kappa), opes=P)
    assert [tuple(t.shape) for t in empty] == [(0, d), (0, 4), (0, w.n_atoms, 3)]
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (y3, e3, dx3)), "a refusal launched"


@pytest.mark.parametrize("where", [1, "mixedA", "mixedB"])
def test_offset_buffers_inside_guard_bands(where, hip_device):
    """x, the centres, the kernel table, the table, out, energies and grad_x at offset positions inside guard bands: the bands intact,
    the inputs unchanged, the bits of the call on fresh tensors."""
    model, args, x, x_tab = vb._small7(hip_device, 93)
    spec, ospec = _small7_specs()
    T, O, _ = _reference(model, args, x, x_tab, spec, ospec, 94, "guard bands")
    want, _ = _call(model, x, T, O)
    want = [t.clone() for t in want]
    arena = placement.Arena(hip_device)
    names = ("x", "center", "kappa", "period", "flat", "centers", "heights", "sigma", "opes_period", "table", "out", "energies", "grad_x")
    off = placement.offsets(where, names, wide=2)
    z, kappa, period, flat = T.r
    c, h, s = O.table
    carve = lambda name, t: arena.carve(name, t.shape, F64, off[name], data=t.to(hip_device))       # noqa: E731
    R = Restraint(carve("center", z), carve("kappa", kappa), carve("period", period), carve("flat", flat))
    P = Opes(carve("centers", c), carve("heights", h), carve("sigma", s), SCALE, O.norm, EPS, 4.0, carve("opes_period", O.period), columns=O.cols)
    G = Grid(carve("table", T.g[1]), T.g[2], T.g[3], T.g[4], columns=T.g[0])
    into = (arena.carve("out", (65, 6), F64, off["out"]), arena.carve("energies", (65, 4), F64, off["energies"]), arena.carve("grad_x", x.shape, F64, off["grad_x"]))
    got = model.value_and_bias(carve("x", x), restraint=R, grid=G, opes=P, into=into)
    torch.cuda.synchronize()
    assert vh._info(model).startswith(INFO) and all(a is b for a, b in zip(got, into))
    assert arena.check() == [] and arena.inputs_changed() == []
    assert all(placement.same_bits(a, b) for a, b in zip(got, want))


# ---- 9. the dispatcher operators, the C entry's codes --------------------------------------------------------------------------------
def test_scripted_model_and_operators(tmp_path, hip_device):
    import warnings
    w, model, args = vv._shared("C3", hip_device)
    x = w.make_frames(65, seed=71).double().to(hip_device)
    T, O, _ = _reference(model, args, x, w.make_frames(65, seed=73).double().to(hip_device), _c3_spec(), _c3_ospec(), 72, "operators")
    want, _ = _call(model, x, T, O)
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
    R, G, P = rec["restraint"], rec["grid"], O.record(hip_device)
    opes = (list(P.columns), P.centers, P.heights, P.sigma, P.period, SCALE, O.norm, EPS, 4.0)
    tail = (R.center, R.kappa, R.period, R.flat) + opes + (list(G.columns), G.table, G.lower, G.spacing, G.periodic, [])
    by_handle = torch.ops.molann.value_and_bias_opes_h(x, handle, loaded.ref_x, ws, bs, *tail)
    by_desc = torch.ops.molann.value_and_bias_opes(x, desc, loaded.ref_x, ws, bs, *tail)
    torch.cuda.synchronize()
    info = torch.ops.molann.launch_info(desc, hip_device.index)
    assert info.count(KERNEL) == 1 and info.count("_kernel") == 1, info
    assert len(by_handle) == 3 and len(by_desc) == 3
    assert all(torch.equal(a, b) for a, b in zip(by_handle, want)) and all(torch.equal(a, b) for a, b in zip(by_desc, want))
    # absent walls and table: none / empty lists; no kernels yet and no cutoff
    alone = torch.ops.molann.value_and_bias_opes(x, desc, loaded.ref_x, ws, bs, None, None, None, None, *opes[:5], SCALE, O.norm, EPS, INF, [], None, [], [], [], [])
    plain = model.value_and_bias(x, opes=P._replace(cutoff=None))
    assert all(torch.equal(a, b) for a, b in zip(alone, plain)) and float(plain[1][:, :3].abs().max()) == 0.0
    none_yet = torch.ops.molann.value_and_bias_opes(x, desc, loaded.ref_x, ws, bs, None, None, None, None, [0, 3, 7], P.centers[:0], P.heights[:0], P.sigma[0],
                                                    None, SCALE, O.norm, EPS, 4.0, [], None, [], [], [], [])
    assert bool((none_yet[2] == 0).all())
    for bad in (dict(cols=[8, 1, 0]), dict(cols=[]), dict(cutoff=0.0)):
        with pytest.raises((IndexError, ValueError, RuntimeError)):
            torch.ops.molann.value_and_bias_opes(x, desc, loaded.ref_x, ws, bs, None, None, None, None, bad.get("cols", [0, 3, 7]), *opes[1:5], SCALE, O.norm,
                                                 EPS, bad.get("cutoff", 4.0), [], None, [], [], [], [])


def test_the_entry_s_codes_and_their_order(hip_device):
    w, model, _ = vv._shared("C3", hip_device)
    n = 5
    x = w.make_frames(n, seed=51).double().to(hip_device)
    pre = model.preprocessing_layer
    dp = pre.output_dimension()
    new = lambda *sh: torch.full(sh, NAN, dtype=F64, device=hip_device)       # noqa: E731
    f3, e4, dx3 = new(n, dp), new(n, 4), new(n, w.n_atoms, 3)
    plan = vv._feature_plan(pre, x)
    L, s = _capi.lib(), torch.cuda.current_stream().cuda_stream
    dev = dict(dtype=F64, device=hip_device)
    z, k = torch.zeros(dp, **dev), torch.ones(dp, **dev)
    c2, h2, s2 = torch.zeros((3, 2), **dev), torch.ones(3, **dev), torch.ones(2, **dev)
    t2 = torch.zeros((5, 6), **dev)
    good = (2.25, 0.05, 1e-3, 4.0)
    R0, G0, O0 = (z, k, None, None, 0), ([0, 5], t2, (5, 6), (0.0, 0.0), (1.0, 1.0), None), ([4, 1], c2, h2, s2, None, 3, 0) + good

    def code(r=R0, g=G0, o=O0, ptr=lambda t: t.data_ptr(), xp=None, null=(), hills=0, n_frames=n, p=None, out=None, change=None):
        terms, keep = _capi.bias_terms_f64(r, None, g, ptr=ptr)
        terms.n_hills_columns = hills
        term, keep_o = _capi.opes_term_f64(o, ptr=ptr)
        for name, v in (change or {}).items():
            setattr(term, name, v)
        rc = L.molann_value_and_bias_opes_f64((p or plan)._handle, x.data_ptr() if xp is None else xp, n_frames, None, None,
                                              None if "terms" in null else ctypes.byref(terms), None if "opes" in null else ctypes.byref(term),
                                              (out if out is not None else f3).data_ptr(), e4.data_ptr(), dx3.data_ptr(), s)
        del keep, keep_o
        return rc

    E = _capi
    bad_scalars = ([4, 1], c2, h2, s2, None, 3, 0, 2.25, 0.0, 1e-3, 4.0)
    bad_grid = ([0, 5], t2, (5, 6), (0.0, 0.0), (1.0, NAN), None)
    with torch.cuda.device(hip_device):
        assert plan.supports_value_and_bias_opes_f64() and plan.supports_value_and_bias_f64()
        assert L.molann_plan_supports_value_and_bias_opes_f64(plan._handle) == 1
        # 1. MOLANN_E_NULL, then MOLANN_E_ALIGNMENT
        assert code(null=("opes",)) == E.E_NULL and code(r=(None, k, None, None, 0)) == E.E_NULL
        assert code(o=([4, 1], None, h2, s2, None, 3, 0) + good) == E.E_NULL and code(o=([4, 1], c2, h2, None, None, 3, 0) + good) == E.E_NULL
        assert code(g=([0, 5], None, (5, 6), (0.0, 0.0), (1.0, 1.0), None)) == E.E_NULL and code(g=([0, 5], t2, None, (0.0, 0.0), (1.0, 1.0), None)) == E.E_NULL
        assert code(ptr=lambda t: t.data_ptr() + (4 if t is s2 else 0)) == E.E_ALIGNMENT and code(xp=x.data_ptr() + 4) == E.E_ALIGNMENT
        assert code(g=([0, 5], t2, None, (0.0, 0.0), (1.0, 1.0), None), xp=x.data_ptr() + 4) == E.E_NULL             # NULL before ALIGNMENT
        assert code(xp=x.data_ptr() + 4, o=bad_scalars) == E.E_ALIGNMENT                                                # ALIGNMENT before DESC
        # 2. MOLANN_E_DESC
        assert code(change=dict(n_columns=0)) == E.E_DESC and code(change=dict(n_columns=-1)) == E.E_DESC
        assert code(o=([4, 1], c2, h2, s2, None, -1, 0) + good) == E.E_DESC                                           # a negative count
        assert code(o=([4, 1], c2, h2, s2, None, 3, 3) + good) == E.E_DESC and code(r=(z, k, None, None, 3)) == E.E_DESC     # strides
        for scalars in ((NAN, 0.05, 1e-3, 4.0), (2.25, 0.0, 1e-3, 4.0), (2.25, INF, 1e-3, 4.0), (2.25, 0.05, 0.0, 4.0), (2.25, 0.05, 1e-3, 0.0), (2.25, 0.05, 1e-3, NAN)):
            assert code(o=O0[:7] + scalars) == E.E_DESC, scalars
        assert code(g=([0, 5], t2, (3, 6), (0.0, 0.0), (1.0, 1.0), None)) == E.E_DESC and code(g=bad_grid) == E.E_DESC
        # 3. hills columns in `terms`: MOLANN_E_UNSUPPORTED, after DESC and before the columns' codes
        assert code(hills=2) == E.E_UNSUPPORTED
        assert code(hills=2, o=bad_scalars) == E.E_DESC and code(hills=2, g=bad_grid) == E.E_DESC
        assert code(hills=2, o=([4, dp], c2, h2, s2, None, 3, 0) + good) == E.E_UNSUPPORTED
        # 4. the columns
        assert code(o=([4, dp], c2, h2, s2, None, 3, 0) + good) == E.E_INDEX and code(o=([4, 4], c2, h2, s2, None, 3, 0) + good) == E.E_INDEX
        assert code(g=([-1, 5], t2, (5, 6), (0.0, 0.0), (1.0, 1.0), None)) == E.E_INDEX and code(g=([5, 5], t2, (5, 6), (0.0, 0.0), (1.0, 1.0), None)) == E.E_INDEX
        assert code(o=([4, 4], c2, h2, s2, None, 3, 5) + good) == E.E_DESC                                            # a stride, then a column
        p1 = _capi.Plan(22, features=[(wl.BOND, [0, 1])] * 10)
        c9 = torch.zeros((3, 9), **dev)
        f10 = new(n, 10)
        wide = dict(p=p1, out=f10, r=None, g=None)
        assert code(o=(list(range(9)), c9, h2, k[:1], None, 3, 0) + good, **wide) == E.E_UNSUPPORTED
        assert code(o=((None, 9), c9, h2, k[:1], None, 3, 0) + good, **wide) == E.E_UNSUPPORTED
        assert code(o=(list(range(8)) + [10], c9, h2, k[:1], None, 3, 0) + good, **wide) == E.E_INDEX                # INDEX before UNSUPPORTED
        assert code(o=([0], c9, h2, k[:1], None, 3, 0) + good, g=([0, 1, 2, 3], t2, (4, 4, 4, 4), (0.0,) * 4, (1.0,) * 4, None), p=p1, out=f10, r=None) == E.E_UNSUPPORTED
        p2 = _capi.Plan(22, features=[(wl.BOND, [0, 1])] * 2)
        assert code(o=((None, 3), c9, h2, k[:1], None, 3, 0) + good, p=p2, out=f10, r=None, g=None) == E.E_INDEX      # a NULL list longer than out_dim
        # 5. n_frames
        assert code(n_frames=-1) == E.E_DESC and code(n_frames=0) == 0 and code(n_frames=0, o=bad_scalars, hills=2) == 0
        pa = _capi.Plan(22, align_idx=[0, 1, 2, 3], ref_x=torch.zeros(4, 3))     # no items: nothing to bias
        assert code(p=pa, r=None, g=None) == E.E_STAGE
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (e4, dx3, f3, f10)), "a refusal launched"
    # and terms == NULL is a call without walls or a table
    with torch.cuda.device(hip_device):
        assert code(null=("terms",)) == 0
        torch.cuda.synchronize()
        assert bool(torch.isfinite(f3).all()) and bool((e4[:, :3] == 0).all()) and bool(torch.isfinite(dx3).all())


# ---- 10. the call without `opes` is what it was --------------------------------------------------------------------------------------
def test_without_opes_the_parent_s_kernel_and_three_columns(hip_device):
    w, model, args = vv._shared("C3", hip_device)
    x = w.make_frames(65, seed=23).double().to(hip_device)
    T, O, _ = _reference(model, args, x, w.make_frames(65, seed=29).double().to(hip_device), _c3_spec(), _c3_ospec(), 24, "parent")
    _call(model, x, T, O)
    y, e, dx = _parent_call(model, x, T)
    assert e.shape == (65, 3) and bool((e[:, 1] == 0).all())
    out = model.value_and_bias(x, opes=None, **T.records(hip_device))
    torch.cuda.synchronize()
    assert vh._info(model).startswith(PARENT_INFO) and all(torch.equal(a, b) for a, b in zip(out, (y, e, dx)))
    pre = model.preprocessing_layer
    dp = pre.output_dimension()
    f, ef, dxf = pre.value_and_bias(x, restraint=Restraint(torch.zeros(dp, **dict(dtype=F64, device=hip_device)), 1.0))
    torch.cuda.synchronize()
    assert vh._info(pre).startswith(PARENT_INFO) and ef.shape == (65, 3)
    f4, ef4, dxf4 = pre.value_and_bias(x, restraint=Restraint(torch.zeros(dp, **dict(dtype=F64, device=hip_device)), 1.0),
                                       opes=Opes(f[:9, [2, 0]].contiguous(), 1.0, 0.5, SCALE, 0.2, EPS, 4.0, columns=[2, 0]))
    torch.cuda.synchronize()
    assert vh._info(pre).startswith(INFO) and ef4.shape == (65, 4) and torch.equal(f4, f) and torch.equal(ef4[:, 0], ef[:, 0])
