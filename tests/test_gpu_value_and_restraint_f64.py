"""Float64 values, the energy of a harmonic restraint on them and its gradient in ONE launch (molann_value_and_restraint_f64 ->
frames_value_restraint_f64_kernel): E = 1/2 sum_k kappa_k d_k^2 with d = y - center, wrapped for periodic outputs and cut by a flat
bottom, against float64 autograd on the CPU through the oracle's preprocessing and a copy of the head (torch.round has zero gradient,
which is the derivative of the wrap almost everywhere).  Bounds, the float64 family's: y within 1e-10 max(1, |y|max), the energy
within 1e-10 max(1, |E|max), dx within 1e-9 max(1e-3, |dx|max).

The centres are built from the REFERENCE's y, never from the code under test, so that no element sits on a discontinuity:
z = y_ref + delta + m P with an integer m in [-2, 2] for periodic outputs and |delta| drawn from two bands of P_eff (P, or 1 where the
output is not periodic), [0.02, 0.18] and [0.22, 0.45], around the flat half-width h = 0.2 P_eff: at least 0.05 P_eff from the wrap's
seam P / 2 and 0.02 P_eff from the kink |d| = h, with elements inside the flat bottom (zero force) and outside it.  `_centres` asserts
those margins on the reference values of every element."""

import copy
import math

import pytest
import torch

import test_gpu_random_backward as rb
import test_gpu_value_and_vjp_f64 as vv
from molann_amd import _capi, ann, workloads as wl
from molann_amd.ann import MolANN, create_sequential_nn
from oracle import molann_oracle as mo

pytestmark = pytest.mark.gpu
KERNEL = "frames_value_restraint_f64_kernel"
VJP_KERNEL = "frames_value_vjp_f64_kernel"
TWO_PI = 2.0 * math.pi


def _reference_y(model, feats, uav, align, x):
    """(x on the CPU requiring grad, y) by the oracle's preprocessing on the model's own ref_x and a copy of its head."""
    al = rb._align_layer(model)
    ref = al.ref_x.detach().cpu().double() if al is not None else None
    xx = x.detach().cpu().double().requires_grad_(True)
    y = mo.preprocessing_forward(xx, feats, uav, align if al is not None else None, ref)
    if isinstance(model, MolANN):
        y = copy.deepcopy(model.ann_layers).cpu().double()(y)
    return xx, y


def _wrapped(y, z, period, flat):
    """The issue's d, in torch: differentiable in y."""
    d = y - z
    if period is not None:
        P = torch.where(period > 0, period, torch.ones_like(period))
        d = torch.where(period > 0, d - P * torch.round(d / P), d)
    if flat is not None:
        a = d.abs() - flat
        d = torch.where(flat > 0, torch.where(a > 0, torch.copysign(a, d), torch.zeros_like(d)), d)
    return d


def _centres(y_ref, period, with_flat, seed):
    """(z [n, d], kappa [d], flat [d] or None) on the CPU for reference outputs y_ref and a period row (0: not periodic), with the
    margins of the module's docstring asserted on every element."""
    n, d = y_ref.shape
    g = torch.Generator().manual_seed(seed)
    p_eff = torch.where(period > 0, period, torch.ones_like(period))
    inside = torch.rand((n, d), generator=g, dtype=torch.float64) < 0.4
    u = torch.rand((n, d), generator=g, dtype=torch.float64)
    mag = torch.where(inside, 0.02 + 0.16 * u, 0.22 + 0.23 * u) * p_eff
    sign = torch.where(torch.rand((n, d), generator=g) < 0.5, -1.0, 1.0).double()
    m = torch.randint(-2, 3, (n, d), generator=g).double() * (period > 0)
    z = y_ref.detach() + sign * mag + m * period
    kappa = 0.5 + 2.5 * torch.rand(d, generator=g, dtype=torch.float64)
    kappa[-1] = -kappa[-1] if d > 1 else kappa[-1]                     # any sign
    flat = 0.2 * p_eff if with_flat else None
    # the margins, on the reference values of every element
    raw = (y_ref.detach() - z) / p_eff
    turn = raw - torch.round(raw)
    assert bool((turn.abs()[:, period > 0] <= 0.45 + 1e-9).all()), "an element within 0.05 P of the wrap's seam"
    dw = _wrapped(y_ref.detach(), z, period, None)
    assert float((dw + sign * mag).abs().max()) <= 1e-12 * float(p_eff.max()) * 8, "the wrapped d is not -delta"
    assert bool(((dw.abs() - 0.2 * p_eff).abs() >= 0.02 * p_eff * (1 - 1e-9)).all()), "an element within 0.02 P_eff of the kink"
    if with_flat and n * d >= 8:
        zero = _wrapped(y_ref.detach(), z, period, flat) == 0
        assert bool(zero.any()) and not bool(zero.all())
    return z, kappa, flat


def _oracle(xx, y, z, kappa, period, flat):
    """(y, E, dE/dx) by float64 autograd of the formula."""
    d = _wrapped(y, z, period, flat)
    energy = 0.5 * (kappa * d * d).sum(dim=1)
    (gx,) = torch.autograd.grad(energy.sum(), xx)
    return y.detach(), energy.detach(), gx


def _close(got, want, what):
    (y, e, dx), (y_want, e_want, gx_want) = got, want
    assert y.dtype == torch.float64 and e.dtype == torch.float64 and dx.dtype == torch.float64
    assert y.shape == y_want.shape and e.shape == e_want.shape and dx.shape == gx_want.shape
    ey, ee, ed = (float((a.detach().cpu() - b).abs().max()) for a, b in ((y, y_want), (e, e_want), (dx, gx_want)))
    sy, se, sd = max(1.0, float(y_want.abs().max())), max(1.0, float(e_want.abs().max())), max(1e-3, float(gx_want.abs().max()))
    print("%s: y err %.3e (scale %.3g), energy err %.3e (scale %.3g), dx err %.3e (scale %.3g)" % (what, ey, sy, ee, se, ed, sd))
    assert ey <= 1e-10 * sy, (what, "y", ey, sy)
    assert ee <= 1e-10 * se, (what, "energy", ee, se)
    assert ed <= 1e-9 * sd, (what, "dx", ed, sd)


def _call(model, x, z, kappa, period=None, flat=None, into=None):
    """((y, energy, dx), launch info) of the module's method, arguments moved to x's device."""
    dev = x.device
    on = lambda t: None if t is None else t.to(dev)       # noqa: E731
    out = model.value_and_restraint(x, on(z), on(kappa), on(period), on(flat), into=into)
    torch.cuda.synchronize()
    return out, (model.last_launch_info() if isinstance(model, MolANN) else ann.last_launch_info(model))


def _check(model, oracle_args, x, period, with_flat, seed, what, shared_rows=False):
    """One model and batch against the oracle; returns the device results and the terms for further checks."""
    xx, y_ref = _reference_y(model, *oracle_args, x)
    z, kappa, flat = _centres(y_ref, period, with_flat, seed)
    got, info = _call(model, x, z, kappa, period if bool((period > 0).any()) else None, flat)
    assert info.startswith(KERNEL + " (values + restraint in one launch; ") and info.count("_kernel") == 1, info
    _close(got, _oracle(xx, y_ref, z, kappa, period, flat), what)
    return got, info, (z, kappa, flat)


def _period_row(d, value, every=1):
    p = torch.zeros(d, dtype=torch.float64)
    p[::every] = value
    return p


# ---- 1. every lane group -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_inp,lanes", [(7, 8), (12, 16), (30, 32), (40, 64)])
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "no_alignment"])
@pytest.mark.parametrize("head", [True, False], ids=["head", "features"])
def test_lane_groups(n_inp, lanes, aligned, head, hip_device):
    """The family's small cases: every lane-group width, with and without an alignment and a head; every second output periodic, a
    flat bottom on all; untouched atoms' rows exactly 0; a shared centre row and the same row per frame give the same bits."""
    case = vv._small_case(n_inp, [0, 2, 4, 6] if aligned else None, head=head)
    model = case.build(hip_device).double().requires_grad_(False)
    d_out = case.mlp[-1] if head else case.d_feat()
    if head:       # the head's widest layer input (the 12 feature columns) asks for at least 16 lanes
        lanes = max(lanes, 16)
    for n in (1, 65):
        x = case.frames(n, seed=n_inp + n, dev=hip_device).double()
        (y, e, dx), info, (z, kappa, flat) = _check(model, (case.feats, case.uav, case.align), x, _period_row(d_out, 1.3, 2), True, n_inp + n,
                                                    (case.name, aligned, head, n))
        assert "%d lanes per frame" % lanes in info, info
        untouched = sorted(set(range(n_inp)) - case.touched())
        assert len(untouched) == n_inp - 7
        if untouched:
            assert float(dx[:, untouched].abs().max()) == 0.0
        period = _period_row(d_out, 1.3, 2)
        shared, _ = _call(model, x, z[0], kappa, period, flat)
        rows, _ = _call(model, x, z[:1].expand(n, d_out).contiguous(), kappa, period, flat)
        assert all(torch.equal(a, b) for a, b in zip(shared, rows))
        assert torch.equal(shared[0], y) and torch.equal(shared[1][:1], e[:1]) and torch.equal(shared[2][:1], dx[:1])


# ---- 2. more outputs than lanes --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65])
def test_outputs_past_the_lane_group(n, hip_device):
    """Features only, the positions of all 7 atoms aligned on 4 of them: 21 outputs on 8 lanes."""
    case = rb.Case("pos7", rb._chain(7, 3), [(rb.POS, list(range(7)))], align=[0, 2, 4, 6], mlp=None)
    model = case.build(hip_device).double().requires_grad_(False)
    assert case.d_feat() == 21
    x = case.frames(n, seed=70 + n, dev=hip_device).double()
    for with_flat in (False, True):
        _, info, _ = _check(model, (case.feats, case.uav, case.align), x, torch.zeros(21, dtype=torch.float64), with_flat, 71 + n, ("pos7", n, with_flat))
        assert "8 lanes per frame" in info and info.endswith("lds=%d" % ((256 // 8) * 21 * 8)), info


# ---- 3. dihedral angles, period 2 pi ---------------------------------------------------------------------------------------------
def _c3_angles(dev, bond=False):
    """The two C3 dihedrals as angle values (features only, C3's alignment), optionally with a bond behind them."""
    w = wl.get_workload("C3")
    feats = [(t, [a - 1 for a in atoms]) for t, atoms in w.features if t == wl.DIHEDRAL][:2]
    assert len(feats) == 2
    if bond:
        feats = feats + [(wl.BOND, [feats[0][1][0], feats[1][1][-1]])]
    align = [a - 1 for a in w.align]
    xyz = w.make_frames(1, seed=0)[0].numpy()
    case = rb.Case("c3_angles", xyz, feats, align=align, uav=True, mlp=None)
    return w, case, case.build(dev).double().requires_grad_(False)


@pytest.mark.parametrize("n", [1, 65])
@pytest.mark.parametrize("with_flat", [False, True], ids=["harmonic", "flat_bottom"])
def test_c3_dihedral_angles(n, with_flat, hip_device):
    w, case, model = _c3_angles(hip_device)
    x = w.make_frames(n, seed=30 + n).double().to(hip_device)
    _check(model, (case.feats, True, case.align), x, _period_row(2, TWO_PI), with_flat, 31 + n, ("C3 angles", n, with_flat))


@pytest.mark.parametrize("n", [1, 65])
def test_c3_dihedrals_and_a_bond_in_one_period_row(n, hip_device):
    w, case, model = _c3_angles(hip_device, bond=True)
    x = w.make_frames(n, seed=40 + n).double().to(hip_device)
    period = torch.tensor([TWO_PI, TWO_PI, 0.0], dtype=torch.float64)
    _check(model, (case.feats, True, case.align), x, period, True, 41 + n, ("C3 angles + bond", n))


# ---- 4. every activation -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", vv.ACT_MODULES, ids=[a.__name__ for a in vv.ACT_MODULES])
def test_every_activation(act, hip_device):
    w, model, args = vv._workload("C3", hip_device, head=[7, 5, 3], act=act())
    x = w.make_frames(65, seed=5).double().to(hip_device)
    _check(model, args, x, _period_row(3, 0.9, 2), True, 50, act.__name__)


# ---- 5. larger frames ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [("P1", 9), ("C4", 3)])
def test_larger_frames(name, n, hip_device):
    w, model, args = vv._shared(name, hip_device)
    if name == "C4":
        assert w.n_atoms == 5000 and w.mlp_dims == [85, 128, 64, 8]
    x = w.make_frames(n, seed=7).double().to(hip_device)
    (_, _, dx), _, _ = _check(model, args, x, _period_row(w.out_dim(), 1.1, 3), True, 60, name)
    untouched = sorted(set(range(w.n_atoms)) - {a - 1 for a in w.touched_atoms()})
    if untouched:
        assert float(dx[:, untouched].abs().max()) == 0.0


# ---- 6. heads that step the rows down ------------------------------------------------------------------------------------------------
BONDS = [(wl.BOND, [0, 1]), (wl.BOND, [1, 2]), (wl.BOND, [2, 3])]
# the forces' rows of the contract test (2049 and 8203 doubles) and the cotangent row of 2: four waves of one frame each pass 64 KiB
# from 2049 doubles on, one frame passes it from 8193 on
STEPPED = {"step_down": ([3, 682, 2], 128, 2 * 2051 * 8), "over_64k": ([3, 2048, 8, 2048, 2], 64, 8205 * 8)}


@pytest.mark.parametrize("name", sorted(STEPPED))
def test_heads_that_step_the_rows_down(name, hip_device):
    dims, block, lds = STEPPED[name]
    n, n_inp = 4, 8
    g = torch.Generator().manual_seed(len(dims))
    head = create_sequential_nn(dims, torch.nn.Tanh()).double().requires_grad_(False)
    for lin in head:
        if isinstance(lin, torch.nn.Linear):
            lin.weight.copy_(torch.randn(lin.weight.shape, generator=g, dtype=torch.float64) / math.sqrt(lin.in_features))
            lin.bias.copy_(0.1 * torch.randn(lin.bias.shape, generator=g, dtype=torch.float64))
    x = (torch.randn((n, n_inp, 3), generator=g, dtype=torch.float64) * 2.0)
    xx = x.clone().requires_grad_(True)
    y_ref = head(mo.preprocessing_forward(xx, BONDS, False, None, None))
    period = torch.tensor([0.7, 0.0], dtype=torch.float64)
    z, kappa, flat = _centres(y_ref, period, True, 80)
    dev = hip_device
    with torch.cuda.device(dev):
        plan = _capi.Plan(n_inp, features=BONDS, layer_dims=dims, activation=_capi.ACT_TANH)
        assert plan.supports_value_and_restraint_f64()
        lins = [m for m in head if isinstance(m, torch.nn.Linear)]
        W, B = [lin.weight.to(dev).contiguous() for lin in lins], [lin.bias.to(dev).contiguous() for lin in lins]
        y, e, dx = (torch.full(s, float("nan"), dtype=torch.float64, device=dev) for s in ((n, 2), (n,), (n, n_inp, 3)))
        plan.value_and_restraint_f64(x.to(dev), W, B, z.to(dev), kappa.to(dev), period.to(dev), flat.to(dev), y, e, dx)
        torch.cuda.synchronize()
        info = plan.last_launch_info()
    assert info == "%s (values + restraint in one launch; 64 lanes per frame) grid=%d block=%d lds=%d" % (KERNEL, -(-n // (block // 64)), block, lds), info
    _close((y, e, dx), _oracle(xx, y_ref, z, kappa, period, flat), name)


# ---- 7. bit for bit with value_and_vjp ---------------------------------------------------------------------------------------------
def _vjp(model, x, G):
    y, dx, info = vv._call(model, x, G)
    assert VJP_KERNEL in info, info
    return y.clone(), dx.clone()


@pytest.mark.parametrize("name,n", [("C3", 65), ("P1", 9), ("C3_angles", 65)])
def test_bits_of_value_and_vjp(name, n, hip_device):
    if name == "C3_angles":
        w, case, model = _c3_angles(hip_device, bond=True)
        args, d_out = (case.feats, True, case.align), 3
        period = torch.tensor([TWO_PI, TWO_PI, 0.0], dtype=torch.float64)
    else:
        w, model, args = vv._shared(name, hip_device)
        d_out = w.out_dim()
        period = _period_row(d_out, 1.1, 2)
    x = w.make_frames(n, seed=90).double().to(hip_device)
    xx, y_ref = _reference_y(model, *args, x)
    z, kappa, flat = _centres(y_ref, period, True, 91)
    zd, kd = z.to(hip_device), kappa.to(hip_device)
    # no period, no flat: the cotangent is one rounded subtraction and one rounded product, and dx has value_and_vjp's bits for it
    (y, e, dx), _ = _call(model, x, z, kappa)
    yv, dxv = _vjp(model, x, kd * (y - zd))
    assert torch.equal(y, yv) and torch.equal(dx, dxv)
    assert float((e - 0.5 * (kd * (y - zd) ** 2).sum(dim=1)).abs().max()) <= 1e-13 * max(1.0, float(e.abs().max()))
    # with period and flat: value_and_vjp fed the cotangent torch computes
    (y2, e2, dx2), _ = _call(model, x, z, kappa, period, flat)
    assert torch.equal(y2, yv)
    yv2, dxv2 = _vjp(model, x, kd * _wrapped(y2, zd, period.to(hip_device), flat.to(hip_device)))
    ed, sd = float((dx2 - dxv2).abs().max()), max(1e-3, float(dxv2.abs().max()))
    print("%s: dx against value_and_vjp on torch's cotangent %.3e (scale %.3g)" % (name, ed, sd))
    assert ed <= 1e-9 * sd


# ---- 8. determinism, into=, NaN ----------------------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits(hip_device):
    w, model, args = vv._shared("C3", hip_device)
    n, d = 4097, w.out_dim()
    x = w.make_frames(n, seed=41).double().to(hip_device)
    g = torch.Generator().manual_seed(42)
    z, kappa = torch.randn((n, d), generator=g, dtype=torch.float64), torch.rand(d, generator=g, dtype=torch.float64) + 0.5
    period, flat = _period_row(d, 1.1, 2), torch.full((d,), 0.1, dtype=torch.float64)
    a, _ = _call(model, x, z, kappa, period, flat)
    a = [t.clone() for t in a]
    b, info = _call(model, x, z, kappa, period, flat)
    assert KERNEL in info, info
    assert all(torch.equal(s, t) for s, t in zip(a, b)) and all(bool(torch.isfinite(t).all()) for t in a)


def test_into_conversions_and_refusals(hip_device):
    w, model, _ = vv._shared("C3", hip_device)
    pre = model.preprocessing_layer
    n, d = 5, w.out_dim()
    x = w.make_frames(n, seed=51).double().to(hip_device)
    g = torch.Generator().manual_seed(52)
    z, kappa = torch.randn((n, d), generator=g, dtype=torch.float64), torch.rand(d, generator=g, dtype=torch.float64) + 0.5
    flat = torch.full((d,), 0.25, dtype=torch.float64)
    (y, e, dx), _ = _call(model, x, z, kappa, None, flat)
    new = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=hip_device)       # noqa: E731
    y2, e2, dx2 = new(n, d), new(n), new(n, w.n_atoms, 3)
    r, _ = _call(model, x, z, kappa, None, flat, into=(y2, e2, dx2))
    assert r[0] is y2 and r[1] is e2 and r[2] is dx2
    assert torch.equal(y2, y) and torch.equal(e2, e) and torch.equal(dx2, dx)
    # a float kappa, a float32 centre, sequences: converted
    zd = z.to(hip_device)
    k1 = model.value_and_restraint(x, zd, 2.0)
    k2 = model.value_and_restraint(x, zd, torch.full((d,), 2.0, dtype=torch.float64, device=hip_device), flat=[0.0] * d)
    assert all(torch.equal(a, b) for a, b in zip(k1, k2))
    k3 = model.value_and_restraint(x, zd.float(), 2.0)
    assert k3[1].dtype == torch.float64 and float((k3[1] - k1[1]).abs().max()) <= 1e-5 * max(1.0, float(k1[1].abs().max()))
    # features only: the same method on the preprocessing layer, a graph is never recorded
    f, ef, dxf = pre.value_and_restraint(x.clone().requires_grad_(True), [0.0] * pre.output_dimension(), 1.0)
    torch.cuda.synchronize()
    assert KERNEL in ann.last_launch_info(pre) and not (f.requires_grad or ef.requires_grad or dxf.requires_grad)
    assert float((ef - 0.5 * (f * f).sum(dim=1)).abs().max()) <= 1e-12 * max(1.0, float(ef.abs().max()))
    y3, e3, dx3 = new(n, d), new(n), new(n, w.n_atoms, 3)
    bad_calls = [
        (TypeError, dict(into=(y3, dx3))), (TypeError, dict(into=(y3.float(), e3, dx3))), (ValueError, dict(into=(y3[:4], e3, dx3))),
        (ValueError, dict(into=(y3, e3.cpu(), dx3))), (ValueError, dict(into=(y3, e3, dx3.transpose(1, 2)))),
        (ValueError, dict(center=zd[:, :-1])), (ValueError, dict(center=z)), (ValueError, dict(kappa=kappa.to(hip_device)[:-1])),
        (ValueError, dict(period=torch.ones(d + 1, dtype=torch.float64, device=hip_device))),
        (ValueError, dict(flat=-flat.to(hip_device), into=(y3, e3, dx3))), (ValueError, dict(flat=[-1.0] * d, into=(y3, e3, dx3))),
        (TypeError, dict(kappa=torch.ones(d, dtype=torch.int64, device=hip_device))),
    ]
    for exc, changes in bad_calls:
        kw = dict(center=zd, kappa=2.0, into=(y3, e3, dx3))
        kw.update(changes)
        with pytest.raises(exc):
            model.value_and_restraint(x, **kw)
    with pytest.raises(TypeError, match="float64"):
        model.value_and_restraint(x.float(), zd, 2.0)
    with pytest.raises(NotImplementedError, match="value_and_vjp"):
        model.value_and_restraint(x.cpu(), z, 2.0)
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (y3, e3, dx3)), "a refusal launched"
    empty = model.value_and_restraint(x[:0], zd[:0], 2.0)
    assert [tuple(t.shape) for t in empty] == [(0, d), (0,), (0, w.n_atoms, 3)]


def test_nan_poisons_only_its_frame(hip_device):
    w, model, _ = vv._shared("P1", hip_device)
    n, bad, d = 70, 33, w.out_dim()
    x = w.make_frames(n, seed=61).double().to(hip_device)
    g = torch.Generator().manual_seed(62)
    z, kappa = torch.randn((n, d), generator=g, dtype=torch.float64), torch.rand(d, generator=g, dtype=torch.float64) + 0.5
    period, flat = _period_row(d, 1.1, 2), torch.full((d,), 0.1, dtype=torch.float64)
    (y0, e0, dx0), _ = _call(model, x, z, kappa, period, flat)
    y0, e0, dx0 = y0.clone(), e0.clone(), dx0.clone()
    keep = torch.ones(n, dtype=torch.bool, device=hip_device)
    keep[bad] = False
    xb = x.clone()
    xb[bad, 5] = float("nan")
    (y, e, dx), _ = _call(model, xb, z, kappa, period, flat)
    assert torch.equal(y[keep], y0[keep]) and torch.equal(e[keep], e0[keep]) and torch.equal(dx[keep], dx0[keep])
    assert bool(torch.isnan(y[bad]).all()) and bool(torch.isnan(e[bad])) and bool(torch.isnan(dx[bad]).any())
    zb = z.clone()
    zb[bad, 0] = float("nan")                               # output 0 is periodic and has a flat bottom: the NaN survives both
    (y, e, dx), _ = _call(model, x, zb, kappa, period, flat)
    assert torch.equal(y, y0) and torch.equal(e[keep], e0[keep]) and torch.equal(dx[keep], dx0[keep])
    assert bool(torch.isnan(e[bad])) and bool(torch.isnan(dx[bad]).any())


# ---- 9. the dispatcher operators ---------------------------------------------------------------------------------------------------
def test_scripted_model_and_operators(tmp_path, hip_device):
    import warnings
    w, model, _ = vv._shared("C3", hip_device)
    n, d = 65, w.out_dim()
    x = w.make_frames(n, seed=71).double().to(hip_device)
    g = torch.Generator().manual_seed(72)
    z = torch.randn((n, d), generator=g, dtype=torch.float64).to(hip_device)
    kappa = (torch.rand(d, generator=g, dtype=torch.float64) + 0.5).to(hip_device)
    period, flat = _period_row(d, 1.1, 2).to(hip_device), torch.full((d,), 0.1, dtype=torch.float64, device=hip_device)
    want = model.value_and_restraint(x, z, kappa, period, flat)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.jit.script(model).save(str(tmp_path / "c3_f64.pt"))
    loaded = torch.jit.load(str(tmp_path / "c3_f64.pt"), map_location=hip_device)
    ws = [lin.weight for lin in loaded.linears.children()]
    bs = [lin.bias for lin in loaded.linears.children()]
    desc = list(loaded.desc)
    handle = torch.ops.molann.register_desc(desc)
    by_handle = torch.ops.molann.value_and_restraint_h(x, handle, loaded.ref_x, ws, bs, z, kappa, period, flat, [])
    by_desc = torch.ops.molann.value_and_restraint(x, desc, loaded.ref_x, ws, bs, z, kappa, period, flat, [])
    torch.cuda.synchronize()
    info = torch.ops.molann.launch_info(desc, hip_device.index)
    assert info.count(KERNEL) == 1 and info.count("_kernel") == 1, info
    assert len(by_handle) == 3 and len(by_desc) == 3
    assert all(torch.equal(a, b) for a, b in zip(by_handle, want)) and all(torch.equal(a, b) for a, b in zip(by_desc, want))
    plain = torch.ops.molann.value_and_restraint(x, desc, loaded.ref_x, ws, bs, z[0], kappa, None, None, [])
    assert all(torch.equal(a, b) for a, b in zip(plain, model.value_and_restraint(x, z[0], kappa)))


# ---- 10. one launch, the neighbours untouched, the C entry's own refusals ------------------------------------------------------------
def test_one_launch_and_the_neighbours_untouched(hip_device):
    w, model, _ = vv._shared("C3", hip_device)
    n, d = 64, w.out_dim()
    x = w.make_frames(n, seed=91).double().to(hip_device)
    z = torch.zeros(d, dtype=torch.float64)
    _, info = _call(model, x, z, torch.ones(d, dtype=torch.float64))
    assert info.startswith(KERNEL) and info.count("_kernel") == 1 and "molann_" not in info and "||" not in info, info
    G = torch.ones((n, d), dtype=torch.float64, device=hip_device)
    model.value_and_vjp(x, G)
    torch.cuda.synchronize()
    assert model.last_launch_info().startswith(VJP_KERNEL)
    m32 = wl.build_model(w, hip_device, 0).requires_grad_(False)
    m32.value_and_vjp(x.float(), G.float())
    torch.cuda.synchronize()
    info32 = m32.last_launch_info()
    assert "f64_kernel" not in info32 and "molann_bwd_ring" in info32, info32
    with torch.cuda.device(hip_device):
        p = _capi.Plan(22, features=[(wl.BOND, [0, 1])])
        assert p.supports_value_and_restraint_f64()
        new = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=hip_device)       # noqa: E731
        y, e, dx = new(3, 1), new(3), new(3, 22, 3)
        x3 = x[:3].contiguous()
        one = torch.ones(3, dtype=torch.float64, device=hip_device)          # [3]: room for a misaligned row of 1
        p.value_and_restraint_f64(x3, [], [], one[:1], one[:1], None, None, y, e, dx)
        torch.cuda.synchronize()
        assert p.last_launch_info().startswith(KERNEL)
        bond = (x3[:, 0] - x3[:, 1]).norm(dim=1)
        assert float((y[:, 0] - bond).abs().max()) <= 1e-12 and float((e - 0.5 * (bond - 1.0) ** 2).abs().max()) <= 1e-12
        y.fill_(float("nan"))
        pa = _capi.Plan(22, align_idx=[0, 1, 2, 3], ref_x=torch.zeros(4, 3))     # no items: nothing to restrain
        assert not pa.supports_value_and_restraint_f64()

        def code(plan, **kw):
            args = dict(center=one[:1], kappa=one[:1], period=None, flat=None, center_stride=0)
            args.update(kw)
            stride = args.pop("center_stride")
            with pytest.raises(_capi.MolannHipError) as err:
                plan.value_and_restraint_f64(x3, [], [], args["center"], args["kappa"], args["period"], args["flat"], y, e, dx, center_stride=stride)
            return err.value.code

        assert code(pa) == _capi.E_STAGE
        assert code(p, center_stride=2) == _capi.E_DESC and code(p, center_stride=-1) == _capi.E_DESC
        L, s = _capi.lib(), torch.cuda.current_stream().cuda_stream
        raw = lambda period, flat: L.molann_value_and_restraint_f64(p._handle, x3.data_ptr(), 3, None, None, one.data_ptr(), 0, one.data_ptr(),       # noqa: E731
                                                                    period, flat, y.data_ptr(), e.data_ptr(), dx.data_ptr(), s)
        assert raw(one.data_ptr() + 4, None) == _capi.E_ALIGNMENT and raw(None, one.data_ptr() + 4) == _capi.E_ALIGNMENT
        torch.cuda.synchronize()
        assert bool(torch.isnan(y).all()), "a refusal launched"
        assert raw(one.data_ptr() + 8, None) == 0
        assert L.molann_value_and_restraint_f64(p._handle, None, 0, None, None, None, 5, None, None, None, None, None, None, s) == 0
        torch.cuda.synchronize()
