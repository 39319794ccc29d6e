"""Forward-mode derivatives on every plan family: fwAD duals, torch.func.jvp and torch.func.jacfwd of the molann_amd modules
(the tangent kernel frames_jvp_kernel behind _FeaturesJvp / _FeaturesTangent in molann_amd/ann.py) against torch.func.jvp of
the float64 oracle, against the existing reverse kernels (Jacobians, the adjoint identity), and the edges: several tangents in
one launch, empty / one-frame / past-one-grid batches, non-contiguous and zero tangents, parameter tangents through
functional_call, and the refusals (ref_x tangents, forward over forward, hessian)."""

import copy
import math

import pytest
import torch
from torch.autograd import forward_ad as fwAD

from molann_amd import ann, workloads as wl
from molann_amd.ann import MolANN, create_sequential_nn
from molann_amd.atomgroup import Universe
from molann_amd.feature import Feature
from oracle import molann_oracle as mo

pytestmark = pytest.mark.gpu

# family -> (workload, head, frames, variant): head None = the workload's own model, "features" = its preprocessing layer, else
# (layer dims, activation) in front of the workload's preprocessing.  variant: None, "noalign", "dupalign" or "uav" (the
# workload's features with use_angle_value flipped).
FAMILIES = {
    "C1": ("C1", None, 24, None),
    "C2": ("C2", None, 24, None),
    "C3_tanh": ("C3", ([6, 32, 8], torch.nn.Tanh), 24, None),
    "C3_relu": ("C3", ([6, 32, 8], torch.nn.ReLU), 24, None),
    "C3_silu": ("C3", ([6, 32, 8], torch.nn.SiLU), 24, None),
    "C3p_66_5_3": ("C3p", ([66, 5, 3], torch.nn.Tanh), 24, None),
    "P1": ("P1", None, 16, None),
    "P2": ("P2", None, 16, None),
    "A3": ("A3", None, 24, None),
    "A5": ("A5", None, 16, None),
    "C4_features": ("C4", "features", 12, None),
    "C5_features": ("C5", "features", 10, None),
    "A4": ("A4", None, 10, None),
    "C3_noalign": ("C3", ([6, 32, 8], torch.nn.Tanh), 24, "noalign"),
    "C3p_dupalign": ("C3p", "features", 24, "dupalign"),
    "C3_uav": ("C3", "features", 24, "uav"),
    "P1_uav": ("P1", "features", 16, "uav"),
}
REACHED = set()


def _spec(family):
    wname, head, n, variant = FAMILIES[family]
    w = wl.get_workload(wname)
    align = None if w.align is None else list(w.align)
    uav = w.use_angle_value
    if variant == "noalign":
        align = None
    elif variant == "dupalign":
        align = align + [align[0]]
    elif variant == "uav":
        uav = not uav
    return w, head, n, align, uav


def _build(family, dev):
    w, head, _, align, uav = _spec(family)
    u = Universe(w.ref_xyz)
    al = ann.AlignmentLayer(u.atoms_by_number(align), u.atoms) if align is not None else None
    if w.kind == "align":
        return al.to(dev)
    feats = [Feature("f%d" % i, wl.TYPE_NAMES[t], u.atoms_by_number(atoms)) for i, (t, atoms) in enumerate(w.features)]
    pp = ann.PreprocessingANN(al, ann.FeatureLayer(feats, u.atoms, uav))
    if head == "features":
        return pp.to(dev)
    torch.manual_seed(11)
    if head is None:
        if not w.mlp_dims:
            return pp.to(dev)
        return MolANN(pp, create_sequential_nn(w.mlp_dims)).to(dev)
    dims, act = head
    return MolANN(pp, create_sequential_nn(dims, activation=act())).to(dev)


def _oracle(family, model):
    """forward(x, params) of the float64 oracle with the model's own head, and the head's params (float64, CPU)"""
    w, _, _, align, uav = _spec(family)
    feats = [(t, [a - 1 for a in atoms]) for t, atoms in w.features]
    al = [a - 1 for a in align] if align is not None else None
    ref_x = mo.center_reference(torch.from_numpy(w.ref_xyz[al])).double() if al else None
    if w.kind == "align":
        return (lambda x, prm: mo.align_forward(x, al, ref_x)), []
    if not isinstance(model, MolANN):
        return (lambda x, prm: mo.preprocessing_forward(x, feats, uav, al, ref_x)), []
    mods = list(model.ann_layers._modules.values())
    act = mods[1]
    params = [t.detach().cpu().double() for lin in mods[0::2] for t in (lin.weight, lin.bias)]

    def forward(x, prm):
        h = mo.preprocessing_forward(x, feats, uav, al, ref_x)
        n = len(prm) // 2
        for l in range(n):
            h = torch.nn.functional.linear(h, prm[2 * l], prm[2 * l + 1])
            if l + 1 < n:
                h = act(h)
        return h
    return forward, params


def _ill_conditioned(w, x):
    """frames where a dihedral's bond angle is within 3 degrees of 0 / 180 (the tangent of the dihedral is then ill-posed)"""
    bad = torch.zeros(x.shape[0], dtype=torch.bool)
    lim = math.sin(math.radians(3.0))
    for t, atoms in w.features:
        if t != mo.DIHEDRAL:
            continue
        a = [x[:, i - 1].double() for i in atoms]
        for p, q, r in ((a[0], a[1], a[2]), (a[1], a[2], a[3])):
            u, v = p - q, r - q
            s = torch.linalg.norm(torch.cross(u, v, dim=1), dim=1) / (torch.linalg.norm(u, dim=1) * torch.linalg.norm(v, dim=1))
            bad |= s < lim
    return bad


def _inputs(family, dtype, seed=5):
    w, _, n, _, _ = _spec(family)
    x = w.make_frames(n, seed=seed).to(dtype)
    v = torch.randn(x.shape, generator=torch.Generator().manual_seed(seed + 1), dtype=torch.float64).to(dtype)
    v[_ill_conditioned(w, x)] = 0
    return w, x, v


def _close(got, want, rel, what):
    """row-wise (per frame) bound relative to each frame's scale, floored at 1e-3 of the batch's"""
    got = got.detach().cpu().double().reshape(want.shape[0], -1)
    want = want.detach().cpu().double().reshape(want.shape[0], -1)
    s = want.abs().amax(dim=1).clamp(min=max(1e-300, 1e-3 * float(want.abs().max())))
    err = ((got - want).abs().amax(dim=1) / s).max()
    assert float(err) <= rel, "%s: %.3g > %.3g" % (what, float(err), rel)


def _jvp_launched(model):
    infos = []
    for m in model.modules():
        if isinstance(m, ann._PlanOwner):
            infos += [e.plan.last_launch_info() for e in m._plans().values() if isinstance(e, ann._PlanEntry)]
    return any(i.startswith("frames_jvp") for i in infos)


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_forward_mode_matches_oracle(family, dtype):
    dev = torch.device("cuda:0")
    model = _build(family, dev)
    if dtype == torch.float64:
        model = copy.deepcopy(model).double()
    w, x, v = _inputs(family, dtype)
    forward, params = _oracle(family, model)
    want, dwant = torch.func.jvp(lambda a: forward(a, params), (x.double(),), (v.double(),))
    xd, vd = x.to(dev), v.to(dev)
    with torch.no_grad():
        plain = model(xd)
    with fwAD.dual_level():
        y = model(fwAD.make_dual(xd, vd))
        p_fw, t_fw = fwAD.unpack_dual(y)
    assert t_fw is not None, "a dual input lost its tangent"
    p_fn, t_fn = torch.func.jvp(model, (xd,), (vd,))
    torch.cuda.synchronize()
    assert _jvp_launched(model), family
    REACHED.add(family)
    rel = 1e-4 if dtype == torch.float32 else 1e-9
    _close(t_fw, dwant, rel, "fwAD tangent")
    _close(t_fn, dwant, rel, "torch.func.jvp tangent")
    assert torch.equal(t_fw, t_fn)
    _close(p_fn, plain, 2e-6 if dtype == torch.float32 else 1e-10, "primal vs model(x)")
    _close(p_fn, want, 1e-5 if dtype == torch.float32 else 1e-9, "primal vs oracle")


def _reverse_jacobian(model, x1):
    """[d_out, n_inp, 3] Jacobian of one frame from the existing reverse kernels (identity cotangents on copies of the frame).
    A float32 plan without a float32 backward kernel (a duplicated alignment atom) is differentiated by the float64 ones."""
    try:
        return _reverse_jacobian_of(model, x1)
    except NotImplementedError:
        return _reverse_jacobian_of(copy.deepcopy(model).double(), x1.double()).to(x1.dtype)


def _reverse_jacobian_of(model, x1):
    with torch.no_grad():
        d = model(x1).reshape(-1).numel()
    xe = x1.expand(d, -1, -1).clone().requires_grad_(True)
    y = model(xe).reshape(d, d)
    eye = torch.eye(d, dtype=y.dtype, device=y.device)
    (g,) = torch.autograd.grad(y, xe, eye)
    return g


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("family", ["C1", "C3_tanh", "C3p_66_5_3", "P1", "A3", "A5", "C3_noalign", "C3p_dupalign", "C3_uav"])
def test_jacfwd_equals_reverse_jacobian(family, dtype):
    dev = torch.device("cuda:0")
    model = _build(family, dev)
    if dtype == torch.float64:
        model = copy.deepcopy(model).double()
    _, x, _ = _inputs(family, dtype)
    x1 = x[:1].to(dev)
    J = torch.func.jacfwd(model)(x1)
    assert _jvp_launched(model)       # (before the reverse kernels below launch on the same plans)
    ref = _reverse_jacobian(model, x1)
    d = ref.shape[0]
    J = J.reshape(d, -1)
    scale = float(ref.abs().max())
    err = float((J.double() - ref.reshape(d, -1).double()).abs().max().detach())
    assert err <= (1e-4 if dtype == torch.float32 else 1e-10) * scale, err


@pytest.mark.parametrize("family", ["C2", "C3_tanh", "C3p_66_5_3", "P1", "A3", "A5", "C4_features", "C3p_dupalign"])
def test_adjoint_identity_against_features_backward_f64(family):
    """<J v, g> = <v, J^T g>: the tangent kernel against molann_features_backward_f64 (the float64 reverse path)"""
    dev = torch.device("cuda:0")
    model = copy.deepcopy(_build(family, dev)).double()
    pp = model.preprocessing_layer if isinstance(model, MolANN) else model
    _, x, v = _inputs(family, torch.float64)
    xd, vd = x.to(dev), v.to(dev)
    _, jv = torch.func.jvp(pp, (xd,), (vd,))
    g = torch.randn(jv.shape, generator=torch.Generator().manual_seed(9), dtype=torch.float64).to(dev)
    xg = xd.clone().requires_grad_(True)
    (jtg,) = torch.autograd.grad(pp(xg), xg, g)
    lhs, rhs = float((jv * g).sum()), float((vd * jtg).sum())
    bound = 1e-12 * float((jv.abs() * g.abs()).sum() + (vd.abs() * jtg.abs()).sum())
    assert abs(lhs - rhs) <= bound, (lhs, rhs)


def test_several_tangents_match_separate_calls_bit_for_bit():
    dev = torch.device("cuda:0")
    for family in ("C3_tanh", "P1", "A3", "C4_features"):
        for dtype in (torch.float32, torch.float64):
            model = _build(family, dev)
            if dtype == torch.float64:
                model = copy.deepcopy(model).double()
            pp = model.preprocessing_layer if isinstance(model, MolANN) else model
            _, x, _ = _inputs(family, dtype)
            xd = x.to(dev)
            V = torch.randn((5,) + tuple(x.shape), generator=torch.Generator().manual_seed(1), dtype=torch.float64).to(dev, dtype)
            batched = torch.func.vmap(lambda t: torch.func.jvp(pp, (xd,), (t,))[1])(V)
            assert "5 tangents" in ann.last_launch_info(pp), ann.last_launch_info(pp)
            single = torch.stack([torch.func.jvp(pp, (xd,), (V[i],))[1] for i in range(5)])
            assert torch.equal(batched, single), family


def test_batch_sizes_zero_one_and_past_one_grid():
    dev = torch.device("cuda:0")
    model = _build("C2", dev)
    w = wl.get_workload("C2")
    for n in (0, 1):
        x = w.make_frames(max(n, 1), seed=2)[:n].to(dev)
        p, t = torch.func.jvp(model, (x,), (torch.ones_like(x),))
        assert p.shape == t.shape == (n, w.feature_dim())
    # C2: 8 lanes per frame, 32 frames per block; past num_cus * 8 blocks the grid strides
    n = torch.cuda.get_device_properties(dev).multi_processor_count * 8 * 32 + 1000
    x = w.make_frames(n, seed=3).to(dev)
    v = torch.randn(x.shape, generator=torch.Generator().manual_seed(4)).to(dev)
    _, t = torch.func.jvp(model, (x,), (v,))
    _, t_tail = torch.func.jvp(model, (x[-3000:],), (v[-3000:],))
    assert torch.equal(t[-3000:], t_tail)
    forward, _ = _oracle("C2", model)
    keep = ~_ill_conditioned(w, x[-3000:].cpu())
    _, want = torch.func.jvp(lambda a: forward(a, []), (x[-3000:].cpu().double(),), (v[-3000:].cpu().double(),))
    _close(t_tail.cpu()[keep], want[keep], 1e-4, "tail of a large batch")


def test_non_contiguous_and_zero_tangents():
    dev = torch.device("cuda:0")
    for family in ("C3_tanh", "A3", "P1"):
        model = _build(family, dev)
        _, x, v = _inputs(family, torch.float32)
        xd, vd = x.to(dev), v.to(dev)
        big = torch.zeros((x.shape[0], x.shape[1], 6), device=dev)
        big[..., ::2] = vd
        vn = big[..., ::2]
        assert not vn.is_contiguous()
        _, t = torch.func.jvp(model, (xd,), (vd,))
        _, tn = torch.func.jvp(model, (xd,), (vn,))
        assert torch.equal(t, tn)
        _, t0 = torch.func.jvp(model, (xd,), (torch.zeros_like(xd),))
        assert torch.equal(t0, torch.zeros_like(t0)), family


def test_parameter_tangents_through_functional_call():
    dev = torch.device("cuda:0")
    for family in ("C3_tanh", "P1"):
        model = _build(family, dev)
        _, x, v = _inputs(family, torch.float32)
        xd, vd = x.to(dev), v.to(dev)
        params = {k: p.detach() for k, p in model.named_parameters()}
        g = torch.Generator().manual_seed(8)
        tp = {k: torch.randn(p.shape, generator=g).to(dev) for k, p in params.items()}
        _, t = torch.func.jvp(lambda prm, a: torch.func.functional_call(model, prm, (a,)), (params, xd), (tp, vd))
        forward, oparams = _oracle(family, model)
        names = [k for k, _ in model.named_parameters()]
        _, want = torch.func.jvp(lambda prm, a: forward(a, prm), ([p.double() for p in oparams], x.double()),
                                 ([tp[k].cpu().double() for k in names], v.double()))
        _close(t, want, 1e-4, "parameter + x tangents")


def test_refusals():
    dev = torch.device("cuda:0")
    model = _build("C3_tanh", dev)
    _, x, v = _inputs("C3_tanh", torch.float32)
    xd, vd = x.to(dev), v.to(dev)
    pp = model.preprocessing_layer
    with pytest.raises(RuntimeError, match="ref_x"):
        bufs = {"preprocessing_layer.align_layer.ref_x": pp.align_layer.ref_x}
        torch.func.jvp(lambda b: torch.func.functional_call(model, b, (xd,), strict=False), (bufs,),
                       ({k: torch.ones_like(t) for k, t in bufs.items()},))
    with pytest.raises(NotImplementedError, match="forward over forward"):
        torch.func.jvp(lambda a: torch.func.jvp(model, (a,), (vd,))[1], (xd,), (vd,))
    with pytest.raises((RuntimeError, NotImplementedError), match="hessian"):
        torch.func.hessian(lambda a: model(a).sum())(xd[:1])
    with pytest.raises(RuntimeError, match="cannot be differentiated again"):
        torch.func.jacrev(lambda a: torch.func.jvp(model, (a,), (vd[:1],))[1])(xd[:1])
    align = ann.AlignmentLayer(Universe(wl.get_workload("A3").ref_xyz).atoms_by_number(wl.get_workload("A3").align),
                               Universe(wl.get_workload("A3").ref_xyz).atoms).to(dev)
    with pytest.raises(RuntimeError, match="ref_x"):
        torch.func.jvp(lambda r: torch.func.functional_call(align, {"ref_x": r}, (xd,)), (align.ref_x,), (torch.ones_like(align.ref_x),))


def test_every_family_reached_the_tangent_kernel():
    missing = set(FAMILIES) - REACHED
    assert not missing, "families that never ran frames_jvp_kernel: %s" % sorted(missing)
