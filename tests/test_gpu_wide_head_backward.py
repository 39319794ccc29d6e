"""The backward of wide fp32 heads on the matrix cores (csrc/molann_chain_bwd.inc): molann_mlp_backward_f32 for heads wider than
32 whose chain weight stream is resident, and the head node that carries it (csrc/molann_torch.cpp: HeadFunction; molann_amd/ann.py:
_HeadFunction) - against torch autograd through the fp64 oracle and the reference's own autograd results."""

import copy
import os

import numpy as np
import pytest
import torch

from golden_util import GOLDEN_DIR
from molann_amd import _capi, workloads as wl
from molann_amd.ann import MolANN, _HeadFunction, create_sequential_nn, last_launch_info
from oracle import molann_oracle as mo

pytestmark = pytest.mark.gpu

HEADS = [([6, 64, 64, 8], torch.nn.Tanh), ([6, 48, 33, 5], torch.nn.Sigmoid), ([66, 5, 3], torch.nn.Tanh),
         ([126, 64, 32, 2], torch.nn.SiLU), ([85, 128, 64, 8], torch.nn.Tanh), ([6, 128, 128, 8], torch.nn.ReLU),
         ([6, 100, 70, 3], torch.nn.LeakyReLU), ([85, 40], torch.nn.Tanh)]


FEATURES_OF = {6: "C3", 66: "C3p", 126: "P2", 85: "C4"}     # a workload whose preprocessing gives dims[0] features


def _head_model(dims, act, dev, seed=0):
    """(workload, MolANN): the workload's preprocessing layer in front of a fresh head"""
    w = wl.get_workload(FEATURES_OF[dims[0]])
    base = wl.build_model(w, dev)
    pp = base.preprocessing_layer if isinstance(base, MolANN) else base
    torch.manual_seed(seed)
    return w, MolANN(pp, create_sequential_nn(dims, activation=act()).to(dev))


def _c3_model(dims, act, dev, seed=0):
    return _head_model(dims, act, dev, seed)[1]


@pytest.mark.parametrize("dims,act", HEADS)
@pytest.mark.parametrize("n", [1, 63, 777, 70001])
def test_chain_backward_kernel_vs_fp64_autograd(dims, act, n, hip_device):
    """molann_mlp_backward_f32 alone on the model's plan (C3's preprocessing, or the workload whose features the head reads):
    grad_f and the parameter gradients against a float64 copy of ann_layers; accumulation, optional outputs, run-to-run bit
    identity; the whole-model backward queries are untouched."""
    w, model = _head_model(dims, act, hip_device, seed=len(dims) * 100 + n)
    x = w.make_frames(4, seed=5).to(hip_device).requires_grad_(True)
    plan = model.plan_for(x)
    assert plan.supports_mlp_backward()
    assert not plan.supports_backward() and plan.backward_kind() == 0
    f = (torch.randn((n, dims[0]), generator=torch.Generator().manual_seed(2)) * 1.5).to(hip_device)
    g = torch.randn((n, dims[-1]), generator=torch.Generator().manual_seed(3))
    if act in (torch.nn.ReLU, torch.nn.LeakyReLU):
        # frames with a pre-activation within 1e-4 of the kink may take the other branch in float32 than in float64: no cotangent
        h, near, seen = f.double().cpu(), torch.zeros(n, dtype=torch.bool), 0
        for m in copy.deepcopy(model.ann_layers).double().cpu():
            h = m(h)
            if isinstance(m, torch.nn.Linear):
                seen += 1
                if seen < len(dims) - 1:
                    near |= (h.abs() < 1e-4).any(dim=1)
        g[near] = 0.0
    g = g.to(hip_device)
    gf = torch.full_like(f, float("nan"))
    gp = torch.zeros(plan.grad_params_size(), device=hip_device)
    plan.mlp_backward(f, g, gf, gp)
    assert "molann_chain_bwd" in plan.last_launch_info()
    gp_again = torch.zeros_like(gp)
    plan.mlp_backward(f, g, None, gp_again)
    assert torch.equal(gp, gp_again)                        # no atomics: the same sums, bit for bit
    gp2 = torch.ones_like(gp)                               # accumulated into
    plan.mlp_backward(f, g, None, gp2)
    gf2 = torch.empty_like(f)
    plan.mlp_backward(f, g, gf2, None)
    f64 = f.double().cpu().requires_grad_(True)
    nn64 = copy.deepcopy(model.ann_layers).double().cpu()
    (nn64(f64) * g.double().cpu()).sum().backward()
    s = max(1e-3, float(f64.grad.abs().max()))
    assert float((gf.cpu().double() - f64.grad).abs().max()) <= 2e-4 * s
    assert torch.equal(gf, gf2)
    want = torch.cat([t.grad.reshape(-1) for lin in [m for m in nn64 if isinstance(m, torch.nn.Linear)] for t in (lin.weight, lin.bias)])
    assert gp.numel() == want.numel()
    s = max(1e-3, float(want.abs().max()))
    assert float((gp.cpu().double() - want).abs().max()) <= 2e-4 * s
    assert float((gp2.cpu().double() - 1.0 - want).abs().max()) <= 2e-4 * s + 1e-6


def _oracle(w, model, x, G, act=torch.tanh, create_graph=False):
    """float64 CPU twin: output, and the gradients of sum(out * G) (or, create_graph, of |dE/dx|^2) for x and the parameters"""
    feats = [(t, [a - 1 for a in atoms]) for t, atoms in w.features]
    al = [a - 1 for a in w.align]
    ref_x = mo.center_reference(torch.from_numpy(w.ref_xyz[al])).double()
    lins = [m for m in model.ann_layers if isinstance(m, torch.nn.Linear)]
    xx = x.detach().cpu().double().requires_grad_(True)
    ws = [l.weight.detach().cpu().double().requires_grad_(True) for l in lins]
    bs = [l.bias.detach().cpu().double().requires_grad_(True) for l in lins]
    out = mo.preprocessing_forward(xx, feats, w.use_angle_value, al, ref_x)
    for i, (wt, b) in enumerate(zip(ws, bs)):
        out = out @ wt.T + b
        if i + 1 < len(ws):
            out = act(out)
    E = (out * G.double()).sum()
    if create_graph:
        (F,) = torch.autograd.grad(E, xx, create_graph=True)
        (F * F).sum().backward()
        return F.detach(), xx.grad, [t.grad for pair in zip(ws, bs) for t in pair]
    E.backward()
    return out.detach(), xx.grad, [t.grad for pair in zip(ws, bs) for t in pair]


def _check(model, x, G, want, what, with_x=True):
    _, wx, wp = want
    lins = [m for m in model.ann_layers if isinstance(m, torch.nn.Linear)]
    got = [t.grad for lin in lins for t in (lin.weight, lin.bias)]
    for g, r, name in ([(x.grad, wx, "x")] if with_x else []) + [(a, b, "param %d" % i) for i, (a, b) in enumerate(zip(got, wp))]:
        scale = max(1e-6, float(r.abs().max()))
        assert float((g.cpu().double() - r).abs().max()) <= 2e-4 * scale, (what, name)


def _whole(name, dev):
    """(workload, model, feature list, activation) of the whole models trained here"""
    if name == "C3":
        w = wl.get_workload("C3")
        return w, _c3_model([6, 64, 64, 8], torch.nn.Tanh, dev, seed=3), None
    if name == "C3p":
        w = wl.get_workload("C3p")
        base = wl.build_model(w, dev)
        torch.manual_seed(4)
        return w, MolANN(base, create_sequential_nn([66, 5, 3]).to(dev)), None
    w = wl.get_workload(name)             # P2: the head [126, 64, 32, 2]; C4: [85, 128, 64, 8]
    return w, wl.build_model(w, dev, seed=5), None


@pytest.mark.parametrize("name,n", [("C3", 500), ("C3p", 300), ("P2", 40), ("C4", 6)])
def test_whole_models_train_through_the_chain_backward(name, n, hip_device):
    w, model, _ = _whole(name, hip_device)
    x = w.make_frames(n, seed=9)
    xg = x.to(hip_device).requires_grad_(True)
    G = torch.randn((n, w.out_dim() if w.mlp_dims else model.ann_layers[-1].out_features), generator=torch.Generator().manual_seed(1))
    y = model(xg)
    (y * G.to(hip_device)).sum().backward()
    torch.cuda.synchronize()
    assert "molann_chain_bwd" in last_launch_info(model)
    want = _oracle(w, model, x, G)
    assert float((y.detach().cpu().double() - want[0]).abs().max()) <= 1e-4
    _check(model, xg, G, want, name)


def test_reference_autograd_of_p2_through_the_chain_backward(hip_device):
    """grad_molann_P2 (the reference's own autograd, [126, 64, 32, 2]) met through the new kernel."""
    from test_gpu_backward import _close, _model_from_golden
    d = np.load(os.path.join(GOLDEN_DIR, "grad_molann_P2.npz"))
    model = _model_from_golden(d, hip_device)
    x = torch.from_numpy(d["x"]).to(hip_device).requires_grad_(True)
    out = model(x)
    (out * torch.from_numpy(d["G"]).to(hip_device)).sum().backward()
    torch.cuda.synchronize()
    assert "molann_chain_bwd" in last_launch_info(model)
    _close(x.grad.cpu().numpy(), d["gx_f32"], d["gx_f64"], "grad_x")
    for i, p in enumerate(model.parameters()):
        _close(p.grad.cpu().numpy(), d["gp%d_f32" % i], d["gp%d_f64" % i], "param %d" % i)


@pytest.mark.parametrize("name,n", [("C3", 300), ("C4", 6)])
def test_scripted_model_matches_eager(name, n, hip_device):
    w, model, _ = _whole(name, hip_device)
    x = w.make_frames(n, seed=2)
    G = torch.randn((n, model.ann_layers[-1].out_features), generator=torch.Generator().manual_seed(6)).to(hip_device)
    grads = []
    for run in (model, torch.jit.script(model)):
        model.zero_grad()
        xg = x.to(hip_device).requires_grad_(True)
        (run(xg) * G).sum().backward()
        torch.cuda.synchronize()
        assert "molann_chain_bwd" in model.last_launch_info()
        grads.append([xg.grad.clone()] + [p.grad.clone() for p in model.ann_layers.parameters()])
    for a, b in zip(*grads):
        assert torch.allclose(a, b, rtol=1e-5, atol=1e-6 * max(1e-6, float(b.abs().max())))


@pytest.mark.parametrize("name,n", [("C3", 256), ("C4", 6)])
def test_sgd_steps_track_a_float64_twin(name, n, hip_device):
    """Five SGD steps: in-place updates of the parameters are repacked before the next forward and backward.  The loss after every
    step within 1e-4 of its scale, the parameters after the last within 1e-5 of theirs."""
    w, model, _ = _whole(name, hip_device)
    x = w.make_frames(n, seed=12)
    G = torch.randn((n, model.ann_layers[-1].out_features), generator=torch.Generator().manual_seed(8))
    twin = copy.deepcopy(model).cpu()
    lins = [m for m in model.ann_layers if isinstance(m, torch.nn.Linear)]
    tl = [m for m in twin.ann_layers if isinstance(m, torch.nn.Linear)]
    ws = [l.weight.detach().double().requires_grad_(True) for l in tl]
    bs = [l.bias.detach().double().requires_grad_(True) for l in tl]
    opt = torch.optim.SGD([p for lin in lins for p in (lin.weight, lin.bias)], lr=0.05)
    opt64 = torch.optim.SGD(ws + bs, lr=0.05)
    feats = [(t, [a - 1 for a in atoms]) for t, atoms in w.features]
    al = [a - 1 for a in w.align]
    ref_x = mo.center_reference(torch.from_numpy(w.ref_xyz[al])).double()
    xd = x.to(hip_device)
    for step in range(5):
        opt.zero_grad()
        loss = (model(xd) * G.to(hip_device)).sum()
        loss.backward()
        opt.step()
        opt64.zero_grad()
        loss64 = (mo.molann_forward(x.double(), feats, ws, bs, w.use_angle_value, al, ref_x) * G.double()).sum()
        loss64.backward()
        opt64.step()
        assert abs(float(loss.detach()) - float(loss64.detach())) <= 1e-4 * max(1.0, abs(float(loss64))), step
    assert "molann_chain_bwd" in last_launch_info(model)
    for a, b in zip([p for lin in lins for p in (lin.weight, lin.bias)], [t for pair in zip(ws, bs) for t in pair]):
        assert float((a.detach().cpu().double() - b.detach()).abs().max()) <= 1e-5 * max(1.0, float(b.abs().max()))


def test_create_graph_matches_the_fp64_double_backward(hip_device):
    w, model, _ = _whole("C3", hip_device)
    n = 200
    x = w.make_frames(n, seed=4)
    G = torch.randn((n, 8), generator=torch.Generator().manual_seed(2))
    xg = x.to(hip_device).requires_grad_(True)
    (F,) = torch.autograd.grad((model(xg) * G.to(hip_device)).sum(), xg, create_graph=True)
    (F * F).sum().backward()
    torch.cuda.synchronize()
    F64, gx64, gp64 = _oracle(w, model, x, G, create_graph=True)
    assert float((F.detach().cpu().double() - F64).abs().max()) <= 1e-4 * max(1e-3, float(F64.abs().max()))
    lins = [m for m in model.ann_layers if isinstance(m, torch.nn.Linear)]
    got = [xg.grad] + [t.grad for lin in lins for t in (lin.weight, lin.bias)]
    params = [xg] + [t for lin in lins for t in (lin.weight, lin.bias)]
    for g, r, p in zip(got, [gx64] + gp64, params):      # (the last bias does not reach dE/dx: no gradient on either side)
        g = torch.zeros(p.shape, dtype=torch.float64) if g is None else g.cpu().double()
        r = torch.zeros(p.shape, dtype=torch.float64) if r is None else r
        assert float((g - r).abs().max()) <= 2e-4 * max(1e-3, float(r.abs().max()))


def test_python_head_node_matches_the_kernel(hip_device):
    """The Function of ann.py (what MolANN uses without the operator library) gives the kernel's gradients and repacks."""
    model = _c3_model([6, 64, 64, 8], torch.nn.Tanh, hip_device, seed=7)
    x = wl.get_workload("C3").make_frames(4, seed=5).to(hip_device)
    plan = model.plan_for(x)
    entry = model._fast_state(x)["entry"]()
    lins = [m for m in model.ann_layers if isinstance(m, torch.nn.Linear)]
    f = torch.randn((999, 6), generator=torch.Generator().manual_seed(1)).to(hip_device).requires_grad_(True)
    G = torch.randn((999, 8), generator=torch.Generator().manual_seed(2)).to(hip_device)
    with torch.no_grad():
        lins[1].weight.mul_(0.5)                          # in place: must be repacked
    y = _HeadFunction.apply(f, entry, lins, *[p for lin in lins for p in (lin.weight, lin.bias)])
    (y * G).sum().backward()
    assert "molann_chain_bwd" in plan.last_launch_info()
    f64 = f.detach().double().cpu().requires_grad_(True)
    nn64 = copy.deepcopy(model.ann_layers).double().cpu()
    y64 = nn64(f64)
    assert float((y.detach().cpu().double() - y64.detach()).abs().max()) <= 1e-4
    (y64 * G.double().cpu()).sum().backward()
    for a, b in [(f.grad, f64.grad)] + [(p.grad, q.grad) for p, q in zip(model.ann_layers.parameters(), nn64.parameters())]:
        assert float((a.cpu().double() - b).abs().max()) <= 2e-4 * max(1e-3, float(b.abs().max()))


@pytest.mark.parametrize("case", ["elu", "bf16", "C5_f32", "no_jit"])
def test_other_heads_stay_on_the_torch_composition(case, hip_device, monkeypatch):
    """ELU heads, bf16 heads, streaming heads (C5 in f32) and MOLANN_NO_JIT=1: supports_mlp_backward() is 0 and training still
    matches the oracle."""
    if case == "no_jit":
        monkeypatch.setenv("MOLANN_NO_JIT", "1")
        torch.ops.molann.drop_plans()
    try:
        if case == "C5_f32":
            w = wl.get_workload("C5")
            model = wl.build_model(w, hip_device)
            model.mlp_precision = "f32"
            n, act = 6, torch.tanh
        else:
            w = wl.get_workload("C3")
            a = torch.nn.ELU if case == "elu" else torch.nn.Tanh
            model = _c3_model([6, 64, 64, 8], a, hip_device, seed=11)
            if case == "bf16":
                model.mlp_precision = "bf16"
            n, act = 300, a()
        x = w.make_frames(n, seed=9)
        # (without hipRTC the preprocessing of C3 has no backward kernel: x is data there, the parameters train)
        xg = x.to(hip_device).requires_grad_(case != "no_jit")
        assert not model.plan_for(xg).supports_mlp_backward()
        G = torch.randn((n, model.ann_layers[-1].out_features), generator=torch.Generator().manual_seed(1))
        model.zero_grad()
        (model(xg) * G.to(hip_device)).sum().backward()
        torch.cuda.synchronize()
        assert "molann_chain_bwd" not in last_launch_info(model)
        _check(model, xg, G, _oracle(w, model, x, G, act=act), case, with_x=case != "no_jit")
    finally:
        if case == "no_jit":
            torch.ops.molann.drop_plans()
