"""The exact second order of the float64 features: molann_features_hvp_f64 (frames_hvp_kernel) and the double-backward nodes
that call it (_FeatBackward64 in molann_amd/ann.py, FeatBackward64Fn in csrc/molann_torch.cpp).

- The kernel, called directly on the plans of every family the float64 backward serves (lane-size, mid-size and large frames,
  with and without alignment, AlignmentLayer as alignment + one position item per atom), against torch double backward through
  the float64 oracle: hx within 1e-12 of the batch's scale, hg within 1e-14 of molann_features_jvp_f64's.  Batches of 1, 63, 64,
  65 and 300 frames; frames at 0, 100 and 1000 A and a batch that mixes them.  (Central differences, the node's former backward,
  reach ~1e-9 at best: these bounds are out of their reach.)
- End to end: a loss on forces (E = sum model(x) G, F = dE/dx with create_graph=True, L = sum F^2) for model.double(), eager and
  scripted, within 1e-11 of the oracle's dL/dx and dL/dtheta; the eager second-order pass is one launch of the new kernel, no
  features_f64, and features_backward_f64 only where a head carries J u back to x (the chain rule's first-order term).
- Edge cases: a zero direction, a direction of 1e-305, no frames, repeated calls, degenerate alignments."""

import copy

import pytest
import torch

import far_frames as ff
import test_gpu_double_backward as db
from molann_amd import _capi
from molann_amd import workloads as wl
from oracle import molann_oracle as mo

pytestmark = pytest.mark.gpu

PLANS = ("C1", "C2", "C3", "C3p", "P1", "P2", "C4", "C5", "A3", "A4", "A5")
SIZES = (1, 63, 64, 65, 300)
GEOMETRIES = ("0", "100", "1000", "mixed")
FAMILIES = ("C3_tanh", "P1", "C3p", "A5", "C4_features")
REACHED = set()
_PLANS = {}


def _plan(name, dev):
    """(workload, plan, float64 oracle of its features) of a family's preprocessing (or alignment) plan"""
    if name not in _PLANS:
        w = wl.get_workload(name)
        al = [a - 1 for a in w.align] if w.align else None
        ref = mo.center_reference(torch.from_numpy(w.ref_xyz[al])).float() if al else None
        if w.kind == "align":
            feats = [(mo.POSITION, list(range(w.n_atoms)))]
        else:
            feats = [(t, [a - 1 for a in atoms]) for t, atoms in w.features]
        with torch.cuda.device(dev):
            plan = _capi.Plan(w.n_atoms, align_idx=al, ref_x=ref, features=feats, use_angle_value=w.use_angle_value)
            ref64 = ref.double() if ref is not None else None
            if ref64 is not None:   # the reference in double, as a `.double()` model's sync_ref gives it (the oracle's own)
                plan.update_ref_f64(ref64.to(dev).contiguous())
                torch.cuda.synchronize()
        _PLANS[name] = (w, plan, lambda x: mo.preprocessing_forward(x, feats, w.use_angle_value, al, ref64))
    return _PLANS[name]


def _frames(w, n, geometry, seed=5):
    """float64 frames on a grid of 2^-16 A (differences of coordinates 1000 A out are exact)"""
    x = torch.round(w.make_frames(n, seed=seed).double() * 65536.0) / 65536.0
    if geometry == "mixed":
        return x + torch.tensor([0.0, 100.0, 1000.0], dtype=torch.float64)[torch.arange(n) % 3].view(-1, 1, 1)
    return x + float(geometry)


def _oracle_hx(fwd, x, g, u):
    xx = x.detach().cpu().double().requires_grad_(True)
    (gx,) = torch.autograd.grad((fwd(xx) * g.cpu()).sum(), xx, create_graph=True)
    (hx,) = torch.autograd.grad((gx * u.cpu()).sum(), xx)
    return hx


def _hvp(plan, x, g, u):
    hx = torch.full_like(x, float("nan"))
    hg = torch.full_like(g, float("nan"))
    plan.features_hvp_f64(x, g, u, hx, hg)
    torch.cuda.synchronize()
    return hx, hg


def _rows_err(got, want):
    """largest error of a row over that row's scale (floored at 1e-3 of the batch's)"""
    got = got.detach().cpu().reshape(want.shape[0], -1)
    want = want.reshape(want.shape[0], -1)
    s = want.abs().amax(dim=1)
    s = s.clamp(min=max(1e-300, 1e-3 * float(s.max())))
    return float(((got - want).abs().amax(dim=1) / s).max())


@pytest.mark.parametrize("name", PLANS)
def test_kernel_matches_oracle_double_backward(name, hip_device):
    w, plan, fwd = _plan(name, hip_device)
    n_max = max(SIZES)
    gen = torch.Generator().manual_seed(13)
    for geometry in GEOMETRIES:
        x = _frames(w, n_max, geometry)
        g = torch.randn(n_max, plan.feature_dim, generator=gen, dtype=torch.float64)
        u = torch.randn(x.shape, generator=gen, dtype=torch.float64)
        want = _oracle_hx(fwd, x, g, u)
        xd, gd, ud = x.to(hip_device), g.to(hip_device), u.to(hip_device)
        for n in SIZES:
            hx, hg = _hvp(plan, xd[:n], gd[:n], ud[:n])
            info = plan.last_launch_info()
            assert info.startswith("frames_hvp_f64_kernel"), info
            assert bool(torch.isfinite(hx).all()) and bool(torch.isfinite(hg).all()), (name, geometry, n)
            # (of the batch's scale: a single row of 64 dihedrals on a 5000-atom chain differs from the oracle's rounding by up
            # to ~1.2e-12 of its own scale)
            err = float((hx.cpu() - want[:n]).abs().max()) / float(want[:n].abs().max())
            assert err <= 1e-12, (name, geometry, n, err, info)
            jt = torch.full((1, n, plan.feature_dim), float("nan"), dtype=torch.float64, device=hip_device)
            plan.features_jvp_f64(xd[:n], ud[:n].unsqueeze(0).contiguous(), None, jt)
            err_g = _rows_err(hg, jt[0].cpu())
            assert err_g <= 1e-14, (name, geometry, n, err_g)
    REACHED.add(("kernel", name))


def _count_launches(monkeypatch):
    calls = {"features_hvp_f64": 0, "features_f64": 0, "features_backward_f64": 0}
    for k in calls:
        orig = getattr(_capi.Plan, k)

        def wrapped(self, *a, _k=k, _orig=orig):
            calls[_k] += 1
            return _orig(self, *a)
        monkeypatch.setattr(_capi.Plan, k, wrapped)
    return calls


@pytest.mark.parametrize("run", ["eager", "scripted"])
@pytest.mark.parametrize("family", FAMILIES)
def test_loss_on_forces_matches_the_oracle(family, run, hip_device, monkeypatch):
    """dL/dx and dL/dtheta of L = |dE/dx|^2 for model.double(), within 1e-11 of the float64 oracle at 0, 100 and 1000 A and in a
    mixed batch; eager: the second-order pass calls the new kernel once and never features_f64"""
    w, model = db._build(family, hip_device)
    m = copy.deepcopy(model).double()
    if run == "scripted":
        m = db._scripted(m, hip_device)
    for geometry in db.GEOMETRIES:
        x = db._frames(w, geometry)
        G = db._cotangent(w, model, x.shape[0])
        F64, gx64, gp64 = db._oracle(family, geometry, w, model, x, G)
        xg = x.to(hip_device, torch.float64).requires_grad_(True)
        params = list(m.parameters())
        out = m(xg)
        (F,) = torch.autograd.grad((out * G.to(hip_device)).sum(), xg, create_graph=True)
        if run == "eager":
            calls = _count_launches(monkeypatch)
        got = torch.autograd.grad((F * F).sum(), [xg] + params, allow_unused=True)
        torch.cuda.synchronize()
        if run == "eager":
            monkeypatch.undo()
            # (a head's chain rule also takes the features' first-order backward once, for the J u term through g)
            first = 1 if isinstance(model, db.MolANN) else 0
            assert calls == {"features_hvp_f64": 1, "features_f64": 0, "features_backward_f64": first}, (family, calls)
        got = [torch.zeros_like(t) if a is None else a for a, t in zip(got, [xg] + params)]
        what = (family, run, geometry)
        assert _rows_err(F, F64) <= 1e-11, what + ("F",)
        assert _rows_err(got[0], gx64) <= 1e-11, what + ("dL/dx", _rows_err(got[0], gx64))
        for i, (a, r) in enumerate(zip(got[1:], gp64)):
            scale = max(1e-3, float(r.abs().max()))
            err = float((a.detach().cpu() - r).abs().max()) / scale
            assert err <= 1e-11, what + ("param %d" % i, err)
    REACHED.add(("e2e", family, run))


@pytest.mark.parametrize("name", ["C3", "P1", "A5", "C4", "P2"])
def test_edge_cases(name, hip_device):
    """A zero direction on one frame gives exactly zero rows there; a direction of 1e-305 gives finite rows equal to 1e-305 times
    those of the unit direction (no step, no clamp); no frames is a no-op; two calls give the same bits"""
    w, plan, _ = _plan(name, hip_device)
    n = 65
    gen = torch.Generator().manual_seed(3)
    x = _frames(w, n, "mixed").to(hip_device)
    g = torch.randn(n, plan.feature_dim, generator=gen, dtype=torch.float64).to(hip_device)
    u = torch.randn(x.shape, generator=gen, dtype=torch.float64).to(hip_device)
    hx, hg = _hvp(plan, x, g, u)
    hx2, hg2 = _hvp(plan, x, g, u)
    assert torch.equal(hx, hx2) and torch.equal(hg, hg2)
    uz = u.clone()
    uz[7] = 0.0
    hxz, hgz = _hvp(plan, x, g, uz)
    assert float(hxz[7].abs().max()) == 0.0 and float(hgz[7].abs().max()) == 0.0
    assert torch.equal(hxz[8:], hx[8:]) and torch.equal(hxz[:7], hx[:7])
    ut = u * 1e-305
    hxt, hgt = _hvp(plan, x, g, ut)
    assert bool(torch.isfinite(hxt).all()) and bool(torch.isfinite(hgt).all())
    assert _rows_err(hxt * 1e305, hx.cpu()) <= 1e-12 and _rows_err(hgt * 1e305, hg.cpu()) <= 1e-12
    e = torch.empty((0,) + tuple(x.shape[1:]), dtype=torch.float64, device=hip_device)
    eg = torch.empty((0, plan.feature_dim), dtype=torch.float64, device=hip_device)
    plan.features_hvp_f64(e, eg, e, e.clone(), eg.clone())
    REACHED.add(("edge", name))


@pytest.mark.parametrize("name", ["C3", "C3p", "A3"])
def test_degenerate_frames_give_finite_rows(name, hip_device):
    """far_frames' degenerate regime (align atoms nearly collinear or at one point) on the plans of position items, and its far
    regimes on every 22-atom plan: finite rows, and the oracle's numbers on well-conditioned frames"""
    w, plan, fwd = _plan(name, hip_device)
    align = [a - 1 for a in w.align]
    gen = torch.Generator().manual_seed(5)
    # (C3's dihedrals sit on its align atoms: collinear align atoms leave its features themselves undefined, as in the oracle)
    for regime in (("degenerate",) if name != "C3" else ()) + ("hinge", "mirror", "flip180", "offset"):
        x = torch.from_numpy(ff.draw(regime, wl.ALA_DIPEPTIDE_XYZ, align, 64, seed=2)).double()
        g = torch.randn(x.shape[0], plan.feature_dim, generator=gen, dtype=torch.float64)
        u = torch.randn(x.shape, generator=gen, dtype=torch.float64)
        hx, hg = _hvp(plan, x.to(hip_device), g.to(hip_device), u.to(hip_device))
        assert bool(torch.isfinite(hx).all()) and bool(torch.isfinite(hg).all()), (name, regime)
        if regime != "degenerate":        # well-conditioned frames of the far regimes: the oracle's numbers
            cond = ff.conditioning(x.float().numpy(), wl.ALA_DIPEPTIDE_XYZ, align)
            keep = torch.from_numpy(cond >= 1e-2)
            want = _oracle_hx(fwd, x[keep], g[keep], u[keep])
            assert _rows_err(hx.cpu()[keep], want) <= 1e-10, (name, regime)
    REACHED.add(("degenerate", name))


def test_every_family_reached_the_kernel():
    want = ({("kernel", p) for p in PLANS} | {("e2e", f, r) for f in FAMILIES for r in ("eager", "scripted")} |
            {("edge", p) for p in ("C3", "P1", "A5", "C4", "P2")} | {("degenerate", p) for p in ("C3", "C3p", "A3")})
    assert want <= REACHED, sorted(want - REACHED)
