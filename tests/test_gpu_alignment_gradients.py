"""Alignment gradients through every backward kernel family, with the reference state centred, shifted and replaced by the raw
coordinates of another conformation.  The reference's alignment does not depend on where ref_x sits (sum_a (x_a - x_c) = 0 in
prod, ann.py:187), so neither do its outputs or gradients; a user may assign any coordinates to the buffer after __init__.  Each
case: the kernels named in last_launch_info, outputs and gradients (x and parameters) against torch autograd through the float64
oracle with the same ref_x, the shifted run against the centred run of the same module (the raw state is another, rotated
conformation: equal to the oracle, not to the centred run), zero gradient on untouched atoms and x never written."""

import io

import numpy as np
import pytest
import torch

from molann_amd import _capi
from molann_amd import workloads as wl
from molann_amd.ann import AlignmentLayer, FeatureLayer, MolANN, PreprocessingANN, _PlanEntry, create_sequential_nn
from molann_amd.atomgroup import Universe
from molann_amd.feature import Feature
from oracle import molann_oracle as mo

pytestmark = pytest.mark.gpu
POS, DIH, BOND = wl.POSITION, wl.DIHEDRAL, wl.BOND
SHIFT = (3.0, -2.0, 5.0)


def _chain(n, seed):
    return wl.synthetic_chain(n_atoms=n, step=1.4, seed=seed)


class Spec(object):
    """A model: atoms (xyz), 0-based align and feature lists, an MLP head (or none), or the AlignmentLayer alone."""

    def __init__(self, xyz, align, feats=(), mlp=None, align_only=False):
        self.xyz, self.align, self.feats, self.mlp, self.align_only = xyz, list(align), list(feats), mlp, align_only

    def build(self, dev, dtype=torch.float32):
        u = Universe(self.xyz)
        al = AlignmentLayer(u.atoms_by_number([a + 1 for a in self.align]), u.atoms)
        if self.align_only:
            m = al
        else:
            fl = FeatureLayer([Feature("f%d" % i, wl.TYPE_NAMES[t], u.atoms_by_number([a + 1 for a in idx]))
                               for i, (t, idx) in enumerate(self.feats)], u.atoms, False)
            m = PreprocessingANN(al, fl)
            if self.mlp:
                torch.manual_seed(5)
                m = MolANN(m, create_sequential_nn(self.mlp))
        return m.to(dev).to(dtype)

    def touched(self):
        return set(self.align) | {a for _, idx in self.feats for a in idx}

    def other_conformation(self):
        """Raw coordinates of the align atoms in another conformation: noisy, rigidly moved, tens of A from the origin."""
        g = torch.Generator().manual_seed(len(self.xyz))
        x = torch.from_numpy(self.xyz) + 0.3 * torch.randn(self.xyz.shape, generator=g)
        q = torch.randn(4, generator=g)
        R = wl.quaternion_to_matrix((q / q.norm()).unsqueeze(0))[0]
        return (x @ R + torch.tensor([24.0, -31.0, 17.0]))[self.align].float()

    def frames(self, n, seed):
        g = torch.Generator().manual_seed(seed)
        ref = torch.from_numpy(self.xyz)
        x = ref.unsqueeze(0) + 0.2 * torch.randn((n,) + tuple(ref.shape), generator=g)
        q = torch.randn((n, 4), generator=g)
        return (torch.matmul(x, wl.quaternion_to_matrix(q / q.norm(dim=1, keepdim=True))) + 3.0 * torch.randn((n, 1, 3), generator=g)).contiguous()


def _ala():
    return wl.ALA_DIPEPTIDE_XYZ


BB = [a - 1 for a in wl.ALA_BACKBONE]
P_SEL = list(range(1, 166, 4))                             # P2: every fourth atom of the 166-atom chain (42)


def _spec(name):
    if name == "C3p":
        return Spec(_ala(), BB, [(POS, list(range(22)))])
    if name == "L1":                                       # 7 backbone positions + one dihedral (d = 23), head [23, 16, 4]
        return Spec(_ala(), BB, [(POS, BB), (DIH, [4, 6, 8, 14])], [23, 16, 4])
    if name == "B8":                                       # 8 position atoms + 2 dihedrals (10 items), head [28, 32, 8]
        return Spec(_chain(166, 11), P_SEL, [(POS, list(range(10, 160, 19))), (DIH, [20, 21, 22, 23]), (DIH, [90, 91, 92, 93])], [28, 32, 8])
    if name == "P2":
        return Spec(_chain(166, 11), P_SEL, [(POS, P_SEL)])
    if name == "P2head":
        return Spec(_chain(166, 11), P_SEL, [(POS, P_SEL)], [126, 64, 32, 2])
    if name == "B2":                                       # 80 position items
        return Spec(_chain(166, 11), P_SEL, [(POS, list(range(3, 163, 2)))])
    if name == "W2000":                                    # over the 1024-atom limit of the group kernel: one wave per frame
        return Spec(_chain(2000, 5), list(range(7, 2000, 13)), [(POS, list(range(31, 2000, 97))), (BOND, [100, 101]), (BOND, [1500, 1503])])
    if name.startswith("A"):
        n = int(name[1:])
        rng = np.random.default_rng(n)
        return Spec(_chain(n, 3), sorted(rng.choice(n, size=min(300, n // 4), replace=False).tolist()), align_only=True)
    raise KeyError(name)


# family: (spec, env, forward kernel(s), backward kernel, batch sizes)
FAMILIES = {
    "lane_bwd_C3p": ("C3p", {"MOLANN_NO_RING_BWD": "1"}, ("lane",), "molann_lane_bwd", (1, 65, 300)),
    "lane_bwd_L1": ("L1", {"MOLANN_NO_RING_BWD": "1"}, ("lane",), "molann_lane_bwd", (1, 65, 300)),
    "bwd_ring_L1": ("L1", {}, ("lane", "molann_bwd_ring"), "molann_bwd_ring", (1, 65, 300)),
    "group_B8": ("B8", {}, ("frames_ring_kernel",), "frames_group_bwd_kernel<B=8>", (1, 17, 300)),
    "group_B4_P2": ("P2", {}, ("frames_ring_kernel",), "frames_group_bwd_kernel<B=4>", (1, 9, 300)),
    "group_B4_P2head": ("P2head", {}, ("frames_ring_kernel",), "frames_group_bwd_kernel<B=4>", (1, 9, 300)),
    "group_B2": ("B2", {}, ("frames_ring_kernel",), "frames_group_bwd_kernel<B=2>", (1, 5, 300)),
    "wave_gather_2000": ("W2000", {}, ("frames_ring_kernel", "frames_wave_kernel"), "frames_wave_bwd_gather_kernel", (1, 9, 64)),
    "wave_atomics_2000": ("W2000", {"MOLANN_BWD_ATOMICS": "1"}, ("frames_ring_kernel", "frames_wave_kernel"), "frames_wave_bwd_kernel", (1, 9, 64)),
    "align_regs_166": ("A166", {}, ("frames_align_batch_kernel", "frames_align_regs_kernel"), "frames_align_bwd_regs_kernel", (1, 9, 300)),
    "align_regs_1537": ("A1537", {}, ("frames_align_batch_kernel", "frames_align_regs_kernel"), "frames_align_bwd_regs_kernel", (1, 9, 40)),
    "align_regs_5000": ("A5000", {}, ("frames_align_batch_kernel", "frames_align_regs_kernel"), "frames_align_bwd_regs_kernel", (1, 9, 40)),
    "wave_bwd_align_12400": ("A12400", {}, ("frames_wave_kernel", "frames_align"), "frames_wave_bwd", (1, 5)),
}
STATES = ["centred", "shift", "raw"]


def _ref_for(spec, state, centred):
    if state == "centred":
        return centred.clone()
    if state == "shift":
        return centred + torch.tensor(SHIFT, dtype=centred.dtype)
    return spec.other_conformation().to(centred.dtype)


def _align_layer(model):
    if isinstance(model, AlignmentLayer):
        return model
    pp = model.preprocessing_layer if isinstance(model, MolANN) else model
    return pp.align_layer


def _oracle(spec, model, x, G, ref_x):
    """y, dL/dx, dL/d(parameters) of L = sum(y * G) from torch autograd through the float64 oracle."""
    xx = x.detach().cpu().double().requires_grad_(True)
    r = ref_x.detach().cpu().double()
    prm = []
    if spec.align_only:
        y = mo.align_forward(xx, spec.align, r)
    elif spec.mlp:
        lins = [m for m in model.ann_layers if isinstance(m, torch.nn.Linear)]
        ws = [l.weight.detach().cpu().double().requires_grad_(True) for l in lins]
        bs = [l.bias.detach().cpu().double().requires_grad_(True) for l in lins]
        prm = [t for pair in zip(ws, bs) for t in pair]
        y = mo.molann_forward(xx, spec.feats, ws, bs, False, spec.align, r)
    else:
        y = mo.preprocessing_forward(xx, spec.feats, False, spec.align, r)
    (y * G.cpu().double()).sum().backward()
    return y.detach(), xx.grad, [p.grad for p in prm]


def _bound(want):
    return 2e-4 * max(1e-3, float(want.abs().max()))


def _check_close(got, want, bound, what):
    err = float((got.detach().cpu().double() - want).abs().max())
    assert err <= bound, (what, err, bound)


def _infos(model):
    """Launch info of every plan the module and its submodules hold (a model with a head may run its features on the
    PreprocessingANN's plans and its forward and backward on different plans)."""
    infos = [e.plan.last_launch_info() for m in model.modules() if hasattr(m, "_plans")
             for e in m._plans().values() if isinstance(e, _PlanEntry)]
    if isinstance(model, MolANN):
        infos.append(model.last_launch_info())
    return " | ".join(infos)


def _run(model, x, G):
    """(y, dL/dx, parameter gradients, forward info, backward info) of the module under autograd, x untouched."""
    x0 = x.clone()
    xg = x.clone().requires_grad_(True)
    for p in model.parameters():
        p.grad = None
    y = model(xg)
    fwd = _infos(model)
    (y * G).sum().backward()
    torch.cuda.synchronize()
    bwd = _infos(model)
    assert torch.equal(xg.detach(), x0)                    # x is never written
    return y.detach(), xg.grad, [p.grad.clone() for p in model.parameters()], fwd, bwd


@pytest.mark.parametrize("state", STATES)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_alignment_gradient_matrix(family, state, hip_device, monkeypatch):
    spec_name, env, fwd_names, bwd_name, batches = FAMILIES[family]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    spec = _spec(spec_name)
    model = spec.build(hip_device)
    buf = _align_layer(model).ref_x
    centred = buf.detach().cpu().clone()
    ref = _ref_for(spec, state, centred)
    with torch.no_grad():
        buf.copy_(ref.to(hip_device))
    if spec_name == "L1" and not env:
        assert model.plan_for(torch.empty(1, 22, 3, device=hip_device)).backward_kind() == 2
    untouched = sorted(set(range(len(spec.xyz))) - spec.touched())
    g = torch.Generator().manual_seed(len(family) * 7 + STATES.index(state))
    for n in batches:
        x = spec.frames(n, seed=1000 + n).to(hip_device)
        dim = tuple(x.shape) if spec.align_only else (n, (model.ann_layers[-1].out_features if spec.mlp else model.output_dimension()))
        G = torch.randn(dim, generator=g).to(hip_device)
        y, gx, gp, fwd, bwd = _run(model, x, G)
        assert any(f in fwd for f in fwd_names), (family, fwd)
        assert bwd_name in bwd, (family, bwd)
        y_want, gx_want, gp_want = _oracle(spec, model, x, G, ref)
        _check_close(y, y_want, 1e-5 * max(1.0, float(y_want.abs().max())), (family, state, n, "y"))
        _check_close(gx, gx_want, _bound(gx_want), (family, state, n, "x.grad"))
        for i, (p, w) in enumerate(zip(gp, gp_want)):
            _check_close(p, w, _bound(w), (family, state, n, "param %d" % i))
        if untouched and not spec.align_only:
            assert float(gx[:, untouched].abs().max()) == 0.0
        if state == "shift":                               # exact invariance: the centred run of the same module
            with torch.no_grad():
                buf.copy_(centred.to(hip_device))
            y_c, gx_c, gp_c, _, _ = _run(model, x, G)
            with torch.no_grad():
                buf.copy_(ref.to(hip_device))
            _check_close(y, y_c.cpu().double(), 1e-5 * max(1.0, float(y_c.abs().max())), (family, state, n, "y vs centred"))
            _check_close(gx, gx_c.cpu().double(), _bound(gx_c), (family, state, n, "x.grad vs centred"))
            for p, w in zip(gp, gp_c):
                _check_close(p, w.cpu().double(), _bound(w), (family, state, n, "param vs centred"))


@pytest.mark.parametrize("state", ["shift", "raw"])
def test_value_and_vjp_one_launch(state, hip_device):
    spec = _spec("L1")
    model = spec.build(hip_device).requires_grad_(False)
    buf = model.preprocessing_layer.align_layer.ref_x
    ref = _ref_for(spec, state, buf.detach().cpu())
    with torch.no_grad():
        buf.copy_(ref.to(hip_device))
    for n in (1, 65, 300):
        x = spec.frames(n, seed=n).to(hip_device)
        dy = torch.randn((n, 4), generator=torch.Generator().manual_seed(n)).to(hip_device)
        y, dx = model.value_and_vjp(x, dy)
        assert "molann_bwd_ring<values>" in model.last_launch_info(), model.last_launch_info()
        y_want, dx_want, _ = _oracle(spec, model, x, dy, ref)
        _check_close(y, y_want, 1e-5 * max(1.0, float(y_want.abs().max())), (state, n, "y"))
        _check_close(dx, dx_want, _bound(dx_want), (state, n, "dx"))


@pytest.mark.parametrize("spec_name,bwd_name", [("B8", "frames_bwd_f64_kernel"), ("P2", "frames_bwd_f64_kernel")])
@pytest.mark.parametrize("state", ["shift", "raw"])
def test_float64_models(spec_name, bwd_name, state, hip_device):
    spec = _spec(spec_name)
    model = spec.build(hip_device, torch.float64)
    buf = _align_layer(model).ref_x
    ref = _ref_for(spec, state, buf.detach().cpu())
    with torch.no_grad():
        buf.copy_(ref.to(hip_device))
    n = 37
    x = spec.frames(n, seed=7).double().to(hip_device)
    G = torch.randn((n, model.ann_layers[-1].out_features if spec.mlp else model.output_dimension()),
                    generator=torch.Generator().manual_seed(3)).double().to(hip_device)
    y, gx, gp, fwd, bwd = _run(model, x, G)
    assert "frames_f64_kernel" in fwd, fwd
    assert bwd_name in bwd, bwd
    y_want, gx_want, gp_want = _oracle(spec, model, x, G, ref)
    _check_close(y, y_want, 1e-5 * max(1.0, float(y_want.abs().max())), "y")
    _check_close(gx, gx_want, _bound(gx_want), "x.grad")
    for p, w in zip(gp, gp_want):
        _check_close(p, w, _bound(w), "param")


def _reload(model, device):
    b = io.BytesIO()
    torch.jit.save(torch.jit.script(model), b)
    b.seek(0)
    return torch.jit.load(b, map_location=device)


@pytest.mark.parametrize("spec_name,bwd_name", [("L1", "molann_bwd_ring"), ("B8", "frames_group_bwd_kernel<B=8>")])
@pytest.mark.parametrize("state", ["shift", "raw"])
def test_torchscript_saved_and_loaded(spec_name, bwd_name, state, hip_device):
    spec = _spec(spec_name)
    model = spec.build(hip_device)
    buf = _align_layer(model).ref_x
    ref = _ref_for(spec, state, buf.detach().cpu())
    with torch.no_grad():
        buf.copy_(ref.to(hip_device))
    loaded = _reload(model, hip_device)
    n = 65
    x = spec.frames(n, seed=9).to(hip_device)
    xg = x.clone().requires_grad_(True)
    G = torch.randn((n, spec.mlp[-1]), generator=torch.Generator().manual_seed(2)).to(hip_device)
    y = loaded(xg)
    (y * G).sum().backward()
    torch.cuda.synchronize()
    info = torch.ops.molann.launch_info(loaded.desc, hip_device.index)
    assert bwd_name in info, info
    y_want, gx_want, gp_want = _oracle(spec, model, x, G, ref)
    _check_close(y, y_want, 1e-5 * max(1.0, float(y_want.abs().max())), "y")
    _check_close(xg.grad, gx_want, _bound(gx_want), "x.grad")
    for p, w in zip(loaded.parameters(), gp_want):
        _check_close(p.grad, w, _bound(w), "param")
    assert torch.equal(xg.detach(), x)


@pytest.mark.parametrize("state", ["shift", "raw"])
def test_graphed_forces(state, hip_device):
    from molann_amd.graph import GraphedForces
    spec = _spec("B8")
    model = spec.build(hip_device).requires_grad_(False)
    buf = model.preprocessing_layer.align_layer.ref_x
    ref = _ref_for(spec, state, buf.detach().cpu())
    with torch.no_grad():
        buf.copy_(ref.to(hip_device))
    n = 17
    x = spec.frames(n, seed=4).to(hip_device)
    dy = torch.randn((n, 8), generator=torch.Generator().manual_seed(5)).to(hip_device)
    gf = GraphedForces(model, x)
    info = gf._plan.last_launch_info()                     # the backward graph was captured last
    assert "frames_group_bwd_kernel<B=8>" in info, info
    xe = x.clone().requires_grad_(True)
    ye = model(xe)
    (dxe,) = torch.autograd.grad(ye, xe, dy)
    y = gf(x).clone()
    dx = gf.vjp(dy).clone()
    y2, dx2 = gf.value_and_vjp(x, dy)
    torch.cuda.synchronize()
    y_want, dx_want, _ = _oracle(spec, model, x, dy, ref)
    for got_y, got_dx, what in ((y, dx, "replays"), (y2, dx2, "value_and_vjp"), (ye, dxe, "eager")):
        _check_close(got_y, y_want, 1e-5 * max(1.0, float(y_want.abs().max())), (what, "y"))
        _check_close(got_dx, dx_want, _bound(dx_want), (what, "dx"))
    _check_close(dx, dxe.cpu().double(), _bound(dxe), "replays vs eager")


@pytest.mark.parametrize("spec_name,bwd_name", [("C3p", "molann_lane_bwd"), ("P2", "frames_group_bwd_kernel<B=4>")])
def test_c_abi_plan_with_uncentred_reference(spec_name, bwd_name, hip_device):
    """_capi.Plan(ref_x=<raw coordinates>): the plan packs what it is given (centred there) - features_backward and backward."""
    spec = _spec(spec_name)
    ref = spec.other_conformation()
    n = 33
    x = spec.frames(n, seed=12).to(hip_device)
    with torch.cuda.device(hip_device):
        plan = _capi.Plan(len(spec.xyz), align_idx=spec.align, ref_x=ref, features=spec.feats)
        f = torch.empty((n, plan.feature_dim), device=hip_device)
        plan.features(x, f)
        G = torch.randn(tuple(f.shape), generator=torch.Generator().manual_seed(1)).to(hip_device)
        gx1 = torch.full_like(x, float("nan"))
        plan.features_backward(x, G, gx1)
        torch.cuda.synchronize()
        info = plan.last_launch_info()
        gx2 = torch.full_like(x, float("nan"))
        plan.backward(x, G, gx2, None)
        torch.cuda.synchronize()
    assert bwd_name in info, info
    model = spec.build(hip_device)
    y_want, gx_want, _ = _oracle(spec, model, x, G, ref)
    _check_close(f, y_want, 1e-5 * max(1.0, float(y_want.abs().max())), "features")
    _check_close(gx1, gx_want, _bound(gx_want), "features_backward")
    _check_close(gx2, gx_want, _bound(gx_want), "backward")


@pytest.mark.parametrize("spec_name", ["L1", "B8", "A166"])
def test_reference_replacement_reaches_cached_plan(spec_name, hip_device):
    """A cached plan run with the centred reference; then ref_x changed by copy_, by attribute assignment and by load_state_dict:
    the next run equals the oracle with the new reference."""
    spec = _spec(spec_name)
    model = spec.build(hip_device)
    al = _align_layer(model)
    centred = al.ref_x.detach().cpu().clone()
    n = 21
    x = spec.frames(n, seed=15).to(hip_device)
    G = torch.randn(tuple(model(x).shape), generator=torch.Generator().manual_seed(8)).to(hip_device)

    def check(ref, what):
        y, gx, gp, _, _ = _run(model, x, G)
        y_want, gx_want, gp_want = _oracle(spec, model, x, G, ref)
        _check_close(y, y_want, 1e-5 * max(1.0, float(y_want.abs().max())), (what, "y"))
        _check_close(gx, gx_want, _bound(gx_want), (what, "x.grad"))
        for p, w in zip(gp, gp_want):
            _check_close(p, w, _bound(w), (what, "param"))

    check(centred, "centred")
    shifted = centred + torch.tensor(SHIFT)
    with torch.no_grad():
        al.ref_x.copy_(shifted.to(hip_device))
    check(shifted, "copy_")
    raw = spec.other_conformation()
    al.ref_x = raw.to(hip_device)
    check(raw, "assignment")
    raw2 = raw + torch.tensor([-40.0, 12.0, 3.0])
    sd = model.state_dict()
    key = [k for k in sd if k.endswith("ref_x")][0]
    sd[key] = raw2
    model.load_state_dict(sd)
    check(raw2, "load_state_dict")
