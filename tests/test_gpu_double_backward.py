"""create_graph=True on every plan family: a loss on forces.  E = sum(model(x) * G), F = dE/dx with create_graph=True,
L = sum(F * F), then dL/dx and dL/d(every Linear parameter), against torch autograd twice through the float64 oracle
(tests/test_oracle_gradients.py ties the oracle's second order to the reference's grad2_* fixtures).

The second-order terms go through the node whose backward takes central differences of the float64 kernels along the cotangent
(molann_amd/ann.py: _FeatBackward64 and _difference_points; csrc/molann_torch.cpp: FeatBackward64Fn).  Each family names the
node it must reach; each runs eager float32 through the operator library, as model.double(), scripted (saved and reloaded) and
eager float32 through ctypes, on frames at their own coordinates, 100 A and 1000 A from the origin and a batch that mixes the
three.  Then sparse and tiny cotangents, a loss on the parameter gradients alone, a Hessian-vector product, the refusal of
third order on every node type, and a guard that every family was reached."""

import copy
import io

import pytest
import torch

from molann_amd import ann, workloads as wl
from molann_amd.ann import MolANN, create_sequential_nn
from oracle import molann_oracle as mo

pytestmark = pytest.mark.gpu

# family -> (workload, head, kind): head None = the workload's own model, "features" = its preprocessing layer alone, else
# (layer dims, activation) in front of the workload's preprocessing.  kind names the node of the model's output:
#   run      the fused plan (RunFunction / _PlanFunction)        head     the head node (HeadFunction / _HeadFunction)
#   feat     features or alignment alone (_PlanFunction eager, RunFunction scripted)
#   compose  a head without a HIP backward: torch ops over the features' node
FAMILIES = {
    "C1": ("C1", None, "run"),
    "C3_tanh": ("C3", ([6, 32, 8], torch.nn.Tanh), "run"),
    "C3_relu": ("C3", ([6, 32, 8], torch.nn.ReLU), "run"),
    "C3_sigmoid": ("C3", ([6, 32, 8], torch.nn.Sigmoid), "run"),
    "C3_silu": ("C3", ([6, 32, 8], torch.nn.SiLU), "run"),
    "C3_leaky_relu": ("C3", ([6, 32, 8], torch.nn.LeakyReLU), "run"),
    "C3_elu": ("C3", ([6, 32, 8], torch.nn.ELU), "compose"),
    "C3_gelu": ("C3", ([6, 32, 8], torch.nn.GELU), "compose"),
    "C3_softplus": ("C3", ([6, 32, 8], torch.nn.Softplus), "compose"),
    "C2": ("C2", None, "feat"),
    "C3p": ("C3p", None, "feat"),
    "P1": ("P1", None, "run"),
    "P1_features": ("P1", "features", "feat"),
    "P2": ("P2", None, "head"),
    "C4": ("C4", None, "head"),
    "C3_wide": ("C3", ([6, 64, 64, 8], torch.nn.Tanh), "head"),
    "C4_features": ("C4", "features", "feat"),
    "C5": ("C5", None, "compose"),
    "A3": ("A3", None, "feat"),
    "A5": ("A5", None, "feat"),
    "A4": ("A4", None, "feat"),
}
RUNS = ("op", "float64", "scripted", "ctypes")
GEOMETRIES = ("0", "100", "1000", "mixed")
# the node of the model's output a float32 run must go through, per kind and run (None: not checked)
OUT_NODE = {("run", "op"): "RunFunction", ("run", "scripted"): "RunFunction", ("run", "ctypes"): "_PlanFunctionBackward",
            ("head", "op"): "HeadFunction", ("head", "scripted"): "HeadFunction", ("head", "ctypes"): "_HeadFunctionBackward",
            ("feat", "op"): "_PlanFunctionBackward", ("feat", "scripted"): "RunFunction", ("feat", "ctypes"): "_PlanFunctionBackward"}
REACHED = set()
_ORACLE = {}
_OP_RESULTS = {}


def _n_frames(w):
    return 24 if w.n_atoms <= 22 else (16 if w.n_atoms <= 166 else 8)


def _frames(w, geometry, seed=5):
    """Frames on a grid of 2^-10 A, so that the shifts by 100 and 1000 A are exact in float32: the shifted batch is the same
    geometry, and its second-order results must equal the unshifted batch's (translation invariance)."""
    x = w.make_frames(_n_frames(w), seed=seed)
    x = torch.round(x * 1024.0) / 1024.0
    if geometry == "mixed":
        off = torch.tensor([0.0, 100.0, 1000.0])[torch.arange(x.shape[0]) % 3]
        return x + off.view(-1, 1, 1)
    return x + float(geometry)


def _build(family, dev):
    wname, head, _ = FAMILIES[family]
    w = wl.get_workload(wname)
    model = wl.build_model(w, dev)
    if head == "features":
        model = model.preprocessing_layer
    elif head is not None:
        dims, act = head
        torch.manual_seed(11)
        model = MolANN(model.preprocessing_layer, create_sequential_nn(dims, activation=act()).to(dev))
    return w, model


def _cotangent(w, model, n, seed=3):
    shape = (n, w.n_atoms, 3) if w.kind == "align" else (n, model.ann_layers[-1].out_features if isinstance(model, MolANN)
                                                            else w.feature_dim())
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)


def _oracle_forward(w, model):
    """(forward(x, params), params as float64 CPU tensors): the float64 oracle with the model's own head"""
    feats = [(t, [a - 1 for a in atoms]) for t, atoms in w.features]
    al = [a - 1 for a in w.align] if w.align is not None else None
    ref_x = mo.center_reference(torch.from_numpy(w.ref_xyz[al])).double() if al else None
    if w.kind == "align":
        return (lambda x, prm: mo.align_forward(x, al, ref_x)), []
    if not isinstance(model, MolANN):
        return (lambda x, prm: mo.preprocessing_forward(x, feats, w.use_angle_value, al, ref_x)), []
    mods = list(model.ann_layers._modules.values())
    act = mods[1] if len(mods) > 1 else None
    params = [t.detach().cpu().double() for lin in mods[0::2] for t in (lin.weight, lin.bias)]

    def forward(x, prm):
        h = mo.preprocessing_forward(x, feats, w.use_angle_value, al, ref_x)
        n = len(prm) // 2
        for l in range(n):
            h = torch.nn.functional.linear(h, prm[2 * l], prm[2 * l + 1])
            if l + 1 < n:
                h = act(h)
        return h
    return forward, params


def _oracle(family, geometry, w, model, x, G):
    """float64 F, dL/dx and dL/d(parameters) of the family's model (cached: every run of a family sees the same batch)"""
    key = (family, geometry)
    if key not in _ORACLE:
        forward, params = _oracle_forward(w, model)
        xx = x.detach().cpu().double().requires_grad_(True)
        prm = [p.clone().requires_grad_(True) for p in params]
        (F,) = torch.autograd.grad((forward(xx, prm) * G).sum(), xx, create_graph=True)
        got = torch.autograd.grad((F * F).sum(), [xx] + prm, allow_unused=True)
        got = [torch.zeros_like(t) if g is None else g for g, t in zip(got, [xx] + prm)]
        _ORACLE[key] = (F.detach(), got[0], got[1:])
    return _ORACLE[key]


def _node_names(t):
    """names of every autograd node behind t"""
    names, stack, seen = set(), [t.grad_fn], {}
    while stack and len(seen) < 100000:
        fn = stack.pop()
        if fn is None or id(fn) in seen:
            continue
        seen[id(fn)] = fn                 # (held: an id is not reused while the walk runs)
        names.add(fn.name())
        stack.extend(f for f, _ in fn.next_functions)
    return names


def _scripted(model, dev):
    buf = io.BytesIO()
    torch.jit.save(torch.jit.script(model), buf)
    buf.seek(0)
    return torch.jit.load(buf, map_location=dev)


def _second_order(m, x, G):
    """(out, F, dL/dx, [dL/dparameter]) of E = sum(m(x) G), F = dE/dx (create_graph), L = sum(F F)"""
    xg = x.clone().requires_grad_(True)
    params = list(m.parameters())
    out = m(xg)
    (F,) = torch.autograd.grad((out * G).sum(), xg, create_graph=True)
    assert F.requires_grad
    got = torch.autograd.grad((F * F).sum(), [xg] + params, allow_unused=True)
    torch.cuda.synchronize()
    got = [torch.zeros_like(t) if g is None else g for g, t in zip(got, [xg] + params)]
    return out, F, got[0], got[1:]


def _frame_scale(want):
    """each frame held to its own scale (a frame 1000 A out to its own), floored at 1e-3 of the batch's"""
    s = want.reshape(want.shape[0], -1).abs().amax(dim=1)
    return s.clamp(min=max(1e-300, 1e-3 * float(s.max())))


def _rows_close(got, want, rel, what):
    got = got.detach().cpu().double().reshape(want.shape[0], -1)
    err = (got - want.reshape(want.shape[0], -1)).abs().amax(dim=1) / _frame_scale(want)
    assert bool(torch.isfinite(got).all()), what
    assert float(err.max()) <= rel, (what, float(err.max()), int(err.argmax()))


def _param_close(got, want, rel, what):
    for i, (g, r) in enumerate(zip(got, want)):
        scale = max(1e-3, float(r.abs().max()))
        err = float((g.detach().cpu().double() - r).abs().max())
        assert err <= rel * scale, (what, "param %d" % i, err / scale)


def _run_model(run, model, dev):
    """(the module a run calls, its dtype)"""
    if run == "float64":
        return copy.deepcopy(model).double(), torch.float64
    if run == "scripted":
        return _scripted(model, dev), torch.float32
    return model, torch.float32


def _ctypes(model, monkeypatch):
    """the ctypes branch: no operator library (as tests/test_gpu_value_and_vjp_mid.py::test_ctypes_branch_checks_its_arguments)"""
    monkeypatch.setattr(ann, "_run_op", lambda: None)
    for m in model.modules():
        m.__dict__.pop("_fast", None)
        m.__dict__.pop("_fp", None)


def _op(model, monkeypatch):
    monkeypatch.undo()
    for m in model.modules():
        m.__dict__.pop("_fast", None)
        m.__dict__.pop("_fp", None)


@pytest.mark.parametrize("run", RUNS)
@pytest.mark.parametrize("family", list(FAMILIES))
def test_second_order_matches_the_fp64_oracle(family, run, hip_device, monkeypatch):
    """F within 1e-4 (float32) / 1e-9 (float64) and the second-order terms within 2e-4 / 1e-6 of each frame's scale of the float64
    oracle's, at 0, 100 and 1000 A and in a batch that mixes the three; the shifted batches' second-order terms equal the
    unshifted batch's within the same bounds; the nodes of the family are reached; the Python and the operator's nodes agree:
    float64 eager against float64 scripted within 1e-12 of scale, ctypes against the operator in float32."""
    w, model = _build(family, hip_device)
    kind = FAMILIES[family][2]
    m, dtype = _run_model(run, model, hip_device)
    if run == "ctypes":
        _ctypes(model, monkeypatch)
    f_rel, s_rel = (1e-9, 1e-6) if dtype == torch.float64 else (1e-4, 2e-4)
    base, s64 = None, None
    try:
        for geometry in GEOMETRIES:
            x = _frames(w, geometry)
            G = _cotangent(w, model, x.shape[0])
            F64, gx64, gp64 = _oracle(family, geometry, w, model, x, G)
            out, F, gx, gp = _second_order(m, x.to(hip_device, dtype), G.to(hip_device, dtype))
            what = (family, run, geometry)
            assert any("FeatBackward64" in n for n in _node_names(F)), (what, sorted(_node_names(F)))
            want = OUT_NODE.get((kind, run))
            if want is not None:
                assert any(want in n for n in _node_names(out)), (what, want, sorted(_node_names(out)))
            if kind == "compose" and run != "float64":      # the head is torch's own ops, the features' node below them
                assert not any(k in out.grad_fn.name() for k in ("RunFunction", "PlanFunction", "HeadFunction")), (what, out.grad_fn.name())
            if family == "P1" and run == "op":
                assert model.plan_for(x.to(hip_device)).backward_kind() == 1   # the forward kept the features
            _rows_close(F, F64, f_rel, what + ("F",))
            _rows_close(gx, gx64, s_rel, what + ("dL/dx",))
            _param_close(gp, gp64, s_rel, what + ("dL/dp",))
            if base is None:
                base = (gx, gp)
            else:                    # the same frames, translated: the same second-order terms (the oracle's are too)
                _rows_close(gx, base[0].detach().cpu().double(), s_rel, what + ("dL/dx vs unshifted",))
                _param_close(gp, [t.detach().cpu().double() for t in base[1]], s_rel, what + ("dL/dp vs unshifted",))
            if run == "op":
                _OP_RESULTS[(family, geometry)] = (F.detach().cpu(), gx.cpu(), [t.cpu() for t in gp])
            if run == "float64":     # the Python nodes (eager) and the operator's (scripted) take the same steps
                if s64 is None:
                    s64 = _scripted(m, hip_device)
                _, Fs, gxs, gps = _second_order(s64, x.to(hip_device, dtype), G.to(hip_device, dtype))
                assert any("_FeatBackward64Backward" in n for n in _node_names(F)), what
                assert any("FeatBackward64Fn" in n for n in _node_names(Fs)), what
                for a, b, name in [(F, Fs, "F"), (gx, gxs, "dL/dx")] + [(a, b, "param") for a, b in zip(gp, gps)]:
                    scale = max(1e-300, float(b.abs().max()))
                    err = float((a - b).abs().max())
                    assert err <= 1e-12 * scale, what + ("eager vs scripted", name, err / scale)
            if run == "ctypes":      # the Python nodes and the operator's nodes take the same steps
                if (family, geometry) not in _OP_RESULTS:
                    _op(model, monkeypatch)
                    _, Fo, gxo, gpo = _second_order(model, x.to(hip_device), G.to(hip_device, dtype))
                    _OP_RESULTS[(family, geometry)] = (Fo.detach().cpu(), gxo.cpu(), [t.cpu() for t in gpo])
                    _ctypes(model, monkeypatch)
                Fo, gxo, gpo = _OP_RESULTS[(family, geometry)]
                # the second-order terms are float32 here: the two compositions' float64 intermediates differ in their last bits,
                # which now and then moves a float32 rounding (up to 1e-8 of scale seen); 1e-7 is still far below what another
                # step gives at 100 A.  The float64 run above holds the two kinds of node to 1e-12.
                for a, b, name, rel in [(F, Fo, "F", 1e-12), (gx, gxo, "dL/dx", 1e-7)] + [(a, b, "param", 1e-7) for a, b in zip(gp, gpo)]:
                    scale = max(1e-30, float(b.abs().max()))
                    err = float((a.detach().cpu().double() - b.double()).abs().max())
                    assert err <= rel * scale, what + (name, err / scale)
    finally:
        if run == "ctypes":
            _op(model, monkeypatch)
    REACHED.add((family, run))


# ---- further cases ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["float32", "float64"])
@pytest.mark.parametrize("family", ["C3_tanh", "P1", "C3_wide", "A5", "C3p"])
def test_sparse_cotangent_leaves_other_frames_exactly_zero(family, dtype, hip_device):
    """G nonzero on the first frame, the last and a few between: every other row of F and of dL/dx is exactly zero (the step is
    0 there), and the rows that are not are right."""
    w, model = _build(family, hip_device)
    if dtype == torch.float64:
        model = model.double()
    x = _frames(w, "mixed")
    n = x.shape[0]
    G = _cotangent(w, model, n)
    live = torch.zeros(n, dtype=torch.bool)
    live[[0, 3, 7, n - 1]] = True
    G[~live] = 0.0
    _, F, gx, gp = _second_order(model, x.to(hip_device, dtype), G.to(hip_device, dtype))
    assert float(F.detach()[~live.to(hip_device)].abs().max()) == 0.0
    assert float(gx[~live.to(hip_device)].abs().max()) == 0.0
    F64, gx64, gp64 = _oracle(family, "sparse", w, model, x, G)
    rel = (1e-9, 1e-6) if dtype == torch.float64 else (1e-4, 2e-4)
    _rows_close(F[live.to(hip_device)], F64[live], rel[0], (family, "F"))
    _rows_close(gx[live.to(hip_device)], gx64[live], rel[1], (family, "dL/dx"))
    _param_close(gp, gp64, rel[1], (family, "dL/dp"))
    REACHED.add(("sparse", family))


@pytest.mark.parametrize("run", ["op", "float64", "ctypes"])
@pytest.mark.parametrize("family", ["C3_tanh", "P1"])
def test_loss_on_parameter_gradients_alone(family, run, hip_device, monkeypatch):
    """x is data; L = |dE/dtheta|^2 with create_graph=True (the kept-features branch of RunFunction with need_x false), against
    the oracle's dL/dtheta."""
    w, model = _build(family, hip_device)
    m, dtype = _run_model(run, model, hip_device)
    if run == "ctypes":
        _ctypes(model, monkeypatch)
    try:
        x = _frames(w, "100")
        G = _cotangent(w, model, x.shape[0])
        params = list(m.parameters())
        E = (m(x.to(hip_device, dtype)) * G.to(hip_device, dtype)).sum()
        gs = torch.autograd.grad(E, params, create_graph=True)
        L = sum((g * g).sum() for g in gs)
        got = torch.autograd.grad(L, params, allow_unused=True)
        got = [torch.zeros_like(p) if g is None else g for g, p in zip(got, params)]
    finally:
        if run == "ctypes":
            _op(model, monkeypatch)
    forward, p64 = _oracle_forward(w, model)
    prm = [p.clone().requires_grad_(True) for p in p64]
    gs64 = torch.autograd.grad((forward(x.double(), prm) * G).sum(), prm, create_graph=True)
    want = torch.autograd.grad(sum((g * g).sum() for g in gs64), prm, allow_unused=True)
    want = [torch.zeros_like(p) if g is None else g for g, p in zip(want, prm)]
    _param_close(got, want, 1e-6 if dtype == torch.float64 else 2e-4, (family, run))
    REACHED.add(("params_only", family, run))


@pytest.mark.parametrize("run", ["op", "float64", "ctypes"])
@pytest.mark.parametrize("family", ["C3_tanh", "P1"])
def test_hessian_vector_product(family, run, hip_device, monkeypatch):
    """The Hessian of E(x) = sum(model(x) G) along a random v against the oracle's.  torch.autograd.functional.hvp takes it by
    the double-backward trick, which differentiates the gradient's graph twice: third order, refused (RuntimeError), never a
    value without the terms of the features' node.  vhp is one second-order pass, and v^T H = H v (H is symmetric)."""
    w, model = _build(family, hip_device)
    m, dtype = _run_model(run, model, hip_device)
    if run == "ctypes":
        _ctypes(model, monkeypatch)
    try:
        x = _frames(w, "1000")
        G = _cotangent(w, model, x.shape[0])
        v = torch.randn(x.shape, generator=torch.Generator().manual_seed(9), dtype=torch.float64)
        Gd, xd, vd = G.to(hip_device, dtype), x.to(hip_device, dtype), v.to(hip_device, dtype)
        with pytest.raises(RuntimeError):
            torch.autograd.functional.hvp(lambda xx: (m(xx) * Gd).sum(), xd, vd)
        e, hv = torch.autograd.functional.vhp(lambda xx: (m(xx) * Gd).sum(), xd, vd)
    finally:
        if run == "ctypes":
            _op(model, monkeypatch)
    forward, p64 = _oracle_forward(w, model)
    e64, hv64 = torch.autograd.functional.hvp(lambda xx: (forward(xx, p64) * G).sum(), x.double(), v)
    assert abs(float(e) - float(e64)) <= (1e-9 if dtype == torch.float64 else 1e-4) * max(1.0, abs(float(e64)))
    _rows_close(hv, hv64, 1e-6 if dtype == torch.float64 else 2e-4, (family, run, "hvp"))
    REACHED.add(("hvp", family, run))


@pytest.mark.parametrize("run", ["float64", "scripted64"])
@pytest.mark.parametrize("family", ["C3_tanh", "P1", "A5"])
def test_tiny_cotangent(family, run, hip_device):
    """One frame's cotangent on F scaled to ~1e-305 (the 1e-300 clamps of the step): every result finite, that frame's
    second-order row within the bound of its exact value (about 0), the other frames right."""
    w, model = _build(family, hip_device)
    model = model.double()
    m = _scripted(model, hip_device) if run == "scripted64" else model
    x = _frames(w, "100")
    n = x.shape[0]
    G = _cotangent(w, model, n)
    c = torch.ones(n, dtype=torch.float64)
    c[2] = 1e-305
    xg = x.to(hip_device, torch.float64).requires_grad_(True)
    params = list(m.parameters())
    (F,) = torch.autograd.grad((m(xg) * G.to(hip_device)).sum(), xg, create_graph=True)
    got = torch.autograd.grad((F * F * c.view(-1, 1, 1).to(hip_device)).sum(), [xg] + params, allow_unused=True)
    assert all(bool(torch.isfinite(g).all()) for g in got if g is not None)
    forward, p64 = _oracle_forward(w, model)
    xx = x.double().requires_grad_(True)
    prm = [p.clone().requires_grad_(True) for p in p64]
    (F64,) = torch.autograd.grad((forward(xx, prm) * G).sum(), xx, create_graph=True)
    want = torch.autograd.grad((F64 * F64 * c.view(-1, 1, 1)).sum(), [xx] + prm, allow_unused=True)
    gx, gx64 = got[0].cpu(), want[0]
    scale = float(gx64.abs().max())
    assert float((gx - gx64).abs().max()) <= 1e-6 * scale, (family, run)
    assert float(gx[2].abs().max()) <= 1e-6 * scale
    _param_close([torch.zeros_like(p) if g is None else g for g, p in zip(got[1:], params)],
                 [torch.zeros_like(p) if g is None else g for g, p in zip(want[1:], prm)], 1e-6, (family, run))
    REACHED.add(("tiny", family, run))


# node type -> (family, run)
THIRD_ORDER = {"RunFunction": ("C3_tanh", "op"), "HeadFunction": ("C3_wide", "op"), "_HeadFunction": ("C3_wide", "ctypes"),
               "features": ("C2", "op"), "features_scripted": ("C3p", "scripted"), "align": ("A3", "op"),
               "align_scripted": ("A5", "scripted"), "_FeatBackward64": ("P1", "float64"), "kept_features": ("P1", "op")}


@pytest.mark.parametrize("node", list(THIRD_ORDER))
def test_third_order_is_refused(node, hip_device, monkeypatch):
    """A graph for the second-order gradients, differentiated again: RuntimeError on every node type, never a value."""
    family, run = THIRD_ORDER[node]
    w, model = _build(family, hip_device)
    m, dtype = _run_model(run, model, hip_device)
    if run == "ctypes":
        _ctypes(model, monkeypatch)
    try:
        x = _frames(w, "0").to(hip_device, dtype).requires_grad_(True)
        G = _cotangent(w, model, x.shape[0]).to(hip_device, dtype)
        (F,) = torch.autograd.grad((m(x) * G).sum(), x, create_graph=True)
        L = (F * F).sum()
        (g2,) = torch.autograd.grad(L, x, retain_graph=True)          # second order: a value
        assert bool(torch.isfinite(g2).all())
        third = None
        with pytest.raises(RuntimeError):
            (g2,) = torch.autograd.grad(L, x, create_graph=True)
            (third,) = torch.autograd.grad((g2 * g2).sum(), x)        # only if the line above returned
        assert third is None
    finally:
        if run == "ctypes":
            _op(model, monkeypatch)
    REACHED.add(("third", node))


def test_every_family_was_reached(request):
    """The cases record themselves as they pass, so this guard needs all of them in the same session."""
    here = {i.name for i in request.session.items if i.module is request.module and i.name != request.node.name}
    want = {(f, r) for f in FAMILIES for r in RUNS} | {("third", k) for k in THIRD_ORDER}
    want |= {("sparse", f) for f in ["C3_tanh", "P1", "C3_wide", "A5", "C3p"]}
    want |= {("params_only", f, r) for f in ["C3_tanh", "P1"] for r in ["op", "float64", "ctypes"]}
    want |= {("hvp", f, r) for f in ["C3_tanh", "P1"] for r in ["op", "float64", "ctypes"]}
    want |= {("tiny", f, r) for f in ["C3_tanh", "P1", "A5"] for r in ["float64", "scripted64"]}
    n_cases = len(FAMILIES) * len(RUNS) + len(THIRD_ORDER) + 5 * 2 + 6 + 6 + 6
    if len(here) < n_cases:
        pytest.skip("the coverage guard needs every case of this file in this session: %d of %d selected" % (len(here), n_cases))
    missing = sorted(want - REACHED, key=str)
    assert not missing, ("not reached:", missing)
