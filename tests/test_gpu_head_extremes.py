"""Every kernel that holds a copy of the head's activation code - apply_activation and act_derivative of
molann_amd/csrc/molann_math.h, the constexpr wrappers of molann_ring.inc, molann_mlp_jit.inc, molann_mlp_tile.inc and
molann_chain_bwd.inc, the runtime switch of molann_dev_common.inc's fused head, apply_activation_f64 / act_derivative_f64 - on
heads whose hidden pre-activations are saturated, kinked or pinned to the edges of a number format (tests/head_extremes.py).  Every
other GPU test runs default-initialised heads behind features of order 1: |z| < 2.

FAMILIES names, per family, how it is routed (a model on ALA dipeptide or on a 166-atom chain, or a plan for its head alone; the
environment switches; the entry point), the activations it serves and the kernels last_launch_info must show.  Every head has two
hidden layers, so a saturated layer feeds another one.  One model (or plan) is built per (family, activation); the regimes go
through it by writing the parameters in place, as a user would; the launch info carries no build counter, so what is asserted is
that from the second regime on every 128-frame run reports the same kernels with the same geometry and the operator library's
cache holds the same number of plans: nothing is rebuilt.  128 of the suite's ordinary near frames, and 1 and 65 for `mixed`;
nothing is masked.  A final guard needs every (family, activation) reached.

The restraint, hills, grid and bias kernels call the same frame_head_forward_f64 / frame_head_backward_f64 as the three float64
one-launch entries here and are not repeated.

Per case, against float64 autograd through the oracle and a float64 copy of the head (head_extremes.compare):
  - outputs, dL/dx (the Jacobian, the metric) per frame's scale, dL/dW and dL/db per tensor's scale.  float32: max(1e-5 of the
    scale for outputs and 5e-4 for gradients - the wide-head backward its own 2e-4 -, 2 x the error of the oracle run in float32
    on the CPU on the same frames and parameters); float64: 1e-10 and 1e-9.  kernel / bound and kernel / float32-oracle are
    printed before anything is asserted;
  - bf16 heads against the bf16 emulation of test_gpu_mlp_chain.py at its 4e-3 of the output's scale, or twice the emulation's own
    spread under +-1 float32 ulp of every activation where that is more (head_extremes.bf16_bound);
  - pinned: the pinned units' rows of dL/db1 and dL/dW1 are sum g act'(b) and sum g act'(b) feature at the exactly known b,
    within the gradient bound; a unit at +-0 gives exactly 0 for ReLU and 0.01 sum g for LeakyReLU; everything finite;
  - isolation: `mixed` with the saturated units' outgoing weights zeroed equals the oracle of the live sub-network within the
    bound of that sub-network's own float32 run (a control: it has no saturated unit), the cut units' rows of dL/dW and dL/db are
    exactly zero: a saturated unit's rounding does not leak through a shared LDS row or fragment;
  - x and the parameters are never written.
ELU, Softplus and GELU heads in float32 (test_unserved_activations): no head backward kernel is offered or launched and autograd
through the module still meets the gradient bound on `mixed`.

DESIGN.md, "Head extremes", has the measured ratios of one MI355X."""

import gc
import re

import pytest
import torch

import angular_edges as ae
import head_extremes as he
import test_gpu_angular_edges as aet
import test_gpu_far_frames as fft
import test_gpu_mlp_chain as tmc
import test_gpu_random_backward as rb
from molann_amd import _capi
from molann_amd.ann import MolANN, create_sequential_nn
from oracle import molann_oracle as mo

pytestmark = pytest.mark.gpu
N = 128
REACHED = set()
RATIOS = {}                                                # (family, activation) -> {check: (largest error / bound, kernel / oracle)}
RING = r"frames_ring_kernel<ND=\d+,B=8>"
HEAD_BWD = r"molann_mlp_bwd|molann_chain_bwd|molann_group_vjp"

# family: (kind, spec or None, widths (the features' first for a plan), environment, mode, activations, forward kernels, backward
# kernels).  kind "model": a MolANN on the spec of test_gpu_angular_edges.py; "plan": a plan for the head alone, as
# test_gpu_buffer_placement.py.  modes: fwd (no_grad forward), grad (float32 autograd), vjp (value_and_vjp), f64 (model.double():
# no_grad forward and autograd), vjp64 / jac / metric (the float64 one-launch entries), mlp / mlp_bf16 (Plan.mlp_packed), mlp_bwd
# (Plan.mlp_packed and Plan.mlp_backward).
FAMILIES = {
    "lane_jit_bwd_ring": ("model", "ala_pos", [16, 8, 4], {}, "grad", he.SERVED, (r"molann_lane_jit<NL=3>",), (r"molann_bwd_ring ",)),
    "lane_jit_two_kernel_bwd": ("model", "ala_pos", [16, 8, 4], {"MOLANN_NO_RING_BWD": "1"}, "grad", he.SERVED,
                                (r"molann_lane_jit<NL=",), (r"molann_mlp_bwd", r"molann_lane_bwd")),
    "lane_vjp": ("model", "ala_pos", [16, 8, 4], {}, "vjp", he.SERVED, (r"molann_bwd_ring<values>",), ()),
    "lane_aot_head": ("model", "ala_pos", [16, 8, 4], {"MOLANN_NO_JIT": "1"}, "fwd", he.SERVED, (r"frames_lane_kernel<[1-9]",), ()),
    "lane_wide": ("model", "ala_pos", [40, 33, 5], {}, "fwd", he.ALL, (r"molann_lane_jit<NL=3,wide>",), ()),
    "chain_f32": ("plan", None, [33, 40, 24, 7], {}, "mlp", he.ALL, (r"molann_mlp_chain<f32",), ()),
    "chain_bf16": ("plan", None, [33, 40, 24, 7], {}, "mlp_bf16", he.ALL, (r"molann_mlp_chain<bf16",), ()),
    "mfma_f32": ("plan", None, [33, 40, 24, 7], {"MOLANN_NO_JIT": "1"}, "mlp", he.ALL, (r"mlp_mfma_kernel<f32>",), ()),
    "mfma_bf16": ("plan", None, [33, 40, 24, 7], {"MOLANN_NO_JIT": "1"}, "mlp_bf16", he.ALL, (r"mlp_mfma_kernel<bf16>",), ()),
    "chain_bwd": ("plan", None, [6, 100, 70, 3], {}, "mlp_bwd", he.SERVED, (r"molann_mlp_chain<f32",), (r"molann_chain_bwd",)),
    "ring_lane_mlp_group_bwd": ("model", "c166_pos", [32, 16, 8], {}, "grad", he.SERVED, (RING, r"mlp_lane_kernel"),
                                (r"molann_mlp_bwd", r"frames_group_bwd_kernel")),
    "group_vjp": ("model", "c166_pos", [16, 8, 4], {}, "vjp", he.SERVED, (r"molann_group_vjp<B=",), ()),
    "f64_bwd": ("model", "c166_pos", [16, 8, 4], {}, "f64", he.ALL, (r"frames_f64_kernel",), (r"frames_bwd_f64_kernel",)),
    "vjp_f64": ("model", "ala_pos", [16, 8, 4], {}, "vjp64", he.ALL, (r"frames_value_vjp_f64_kernel",), ()),
    "jac_f64": ("model", "ala_pos", [16, 8, 4], {}, "jac", he.ALL, (r"frames_value_jac_f64_kernel",), ()),
    "metric_f64": ("model", "ala_pos", [16, 8, 4], {}, "metric", he.ALL, (r"frames_value_metric_f64_kernel",), ()),
}
F64_MODES = ("f64", "vjp64", "jac", "metric")
CASES = [(f, c) for f, v in FAMILIES.items() for c in v[5]]

_FRAMES = {}


def _cached_plans():
    """The number of plans in the operator library's cache, None without that library."""
    try:
        return int(torch.ops.molann.cached_plans())
    except (AttributeError, RuntimeError):
        return None


def _frames(spec):
    """128 near frames of a spec (float32 numpy), drawn once."""
    if spec not in _FRAMES:
        xyz, align, _ = aet._spec(spec)
        _FRAMES[spec] = ae.near(xyz, N, 17, align)
    return _FRAMES[spec]


class Setup(object):
    """One (family, activation): its model or plan and what the oracle needs."""

    def __init__(self, family, code, dev):
        self.family, self.code, self.dev = family, code, dev
        self.kind, self.spec, widths, _, self.mode, _, self.fwd_pats, self.bwd_pats = FAMILIES[family]
        self.f64 = self.mode in F64_MODES
        self.dtype = torch.float64 if self.f64 else torch.float32
        self.tol = "f64" if self.f64 else ("wide_bwd" if self.mode == "mlp_bwd" else "f32")
        self.infos, self.long_infos, self.phase = [], {}, None
        gc.collect()                                       # earlier tests' models release their cached plans now, not mid-test
        if self.kind == "plan":
            self.dims = list(widths)
            with torch.cuda.device(dev):
                self.plan = tmc._plan(self.dims, code, precision=_capi.MLP_BF16 if self.mode == "mlp_bf16" else _capi.MLP_F32)
            g = torch.Generator().manual_seed(21)
            self.f = torch.randn(N, self.dims[0], generator=g, dtype=torch.float64).float()
            self.model = None
            return
        self.xyz, self.align, self.items = aet._spec(self.spec)
        d = sum(mo.feature_dim(t, len(i), False) for t, i in self.items)
        self.dims = [d] + list(widths)
        pp = rb.Case(self.spec, self.xyz, self.items, self.align, False, None).build(torch.device("cpu"))
        with torch.random.fork_rng(devices=[]):
            model = MolANN(pp, create_sequential_nn(self.dims, activation=he.MODULE[code]())).to(dev)
        self.model = model.double() if self.f64 else model
        if self.mode not in ("grad", "f64"):
            self.model.requires_grad_(False)
        self.ref = rb._align_layer(self.model).ref_x.detach().cpu().double()
        self.lins = [m for m in self.model.ann_layers if isinstance(m, torch.nn.Linear)]
        self.x = torch.from_numpy(_frames(self.spec)).to(dev, self.dtype)

    def write(self, Ws, bs):
        """The parameters written the way a user would: in place, under no_grad."""
        self.Ws, self.bs = [w.to(self.dev) for w in Ws], [b.to(self.dev) for b in bs]
        if self.kind == "plan":
            with torch.cuda.device(self.dev):
                self.plan.update_mlp(self.Ws, self.bs)
            return
        with torch.no_grad():
            for lin, w, b in zip(self.lins, self.Ws, self.bs):
                lin.weight.copy_(w)
                lin.bias.copy_(b)

    def unwritten(self):
        if self.kind == "plan":
            return True
        return all(torch.equal(lin.weight.detach(), w) and torch.equal(lin.bias.detach(), b) for lin, w, b in zip(self.lins, self.Ws, self.bs))

    def cotangent(self, n, seed=5):
        g = torch.Generator().manual_seed(seed)
        return torch.randn(N, self.dims[-1], generator=g, dtype=torch.float64)[:n]

    def note(self, n, info=None):
        info = fft._infos(self.model) if info is None else info
        self.infos.append(info)
        if n == N:
            self.long_infos.setdefault(self.phase, []).append(info)


def _oracle(su, n, Ws, bs, dtype=torch.float64):
    """{y, D, gp, u1, f}: the mode's quantities on the first n frames by autograd in dtype on the CPU."""
    G = su.cotangent(n)
    if su.kind == "plan":
        out = he.head_oracle(su.f[:n], Ws, bs, su.code, G, dtype, grads=su.mode == "mlp_bwd")
        out["f"] = su.f[:n].double()
        return out
    xx = su.x[:n].detach().cpu().to(dtype).requires_grad_(True)
    f = mo.preprocessing_forward(xx, su.items, False, su.align, su.ref.to(dtype))
    Ws = [w.detach().cpu().to(dtype).requires_grad_(True) for w in Ws]
    bs = [b.detach().cpu().to(dtype).requires_grad_(True) for b in bs]
    y, kept = he.head(f, Ws, bs, su.code, keep=True)
    out = {"y": y.detach(), "D": None, "gp": [], "u1": None, "f": f.detach().double()}
    if su.mode == "fwd":
        return out
    if su.mode in ("jac", "metric"):
        J = torch.stack([torch.autograd.grad(y[:, k].sum(), xx, retain_graph=True)[0] for k in range(y.shape[1])], 1)
        out["D"] = J if su.mode == "jac" else torch.einsum("nkac,nlac->nkl", J, J)
        return out
    prm = [t for pair in zip(Ws, bs) for t in pair] if su.mode in ("grad", "f64") else []
    g = torch.autograd.grad((y * G.to(dtype)).sum(), [xx, kept[0][1]] + prm)
    out.update(D=g[0], u1=g[1], gp=list(g[2:]))
    return out


def _run(su, n):
    """The family's kernels on the first n frames: {y, D, gp}; x is never written."""
    out = {"D": None, "gp": []}
    G = su.cotangent(n).to(su.dev, su.dtype)
    if su.kind == "plan":
        f = su.f[:n].to(su.dev).contiguous()
        f0 = f.clone()
        with torch.cuda.device(su.dev):
            y = torch.full((n, su.dims[-1]), float("nan"), device=su.dev)
            su.plan.mlp_packed(f, y)
            torch.cuda.synchronize()
            su.note(n, su.plan.last_launch_info())
            out["y"] = y
            if su.mode == "mlp_bwd":
                gf = torch.full_like(f, float("nan"))
                gp = torch.zeros(su.plan.grad_params_size(), device=su.dev)
                su.plan.mlp_backward(f, G, gf, gp)
                torch.cuda.synchronize()
                su.note(n, su.plan.last_launch_info())
                out["D"], off = gf, 0
                for k, j in zip(su.dims[:-1], su.dims[1:]):
                    out["gp"] += [gp[off:off + j * k].view(j, k), gp[off + j * k:off + j * k + j]]
                    off += j * k + j
        assert torch.equal(f, f0), (su.family, "the features were written")
        return out
    m, x = su.model, su.x[:n].contiguous()
    x0 = x.clone()
    if su.mode in ("fwd", "f64"):
        with torch.no_grad():
            out["y"] = m(x)
        torch.cuda.synchronize()
        su.note(n)
    if su.mode in ("grad", "f64"):
        y, dx, gp, fwd, bwd = fft._run(m, x, G, "grad")
        su.note(n, fwd + " | " + bwd)
        if any("molann_mlp_bwd" in p for p in su.bwd_pats):
            # dL/dx takes two launches on one plan here and the info keeps the last, the preprocessing's: with x as data the
            # backward is molann_mlp_bwd alone, on the features the forward kept
            for p in m.parameters():
                p.grad = None
            y2 = m(x)
            (y2 * G).sum().backward()
            torch.cuda.synchronize()
            data = fft._infos(m)
            su.note(n, data)
            bwd = bwd + " | " + data
            out["y_data"], out["gp_data"] = y2.detach(), [p.grad.clone() for p in m.parameters()]
        missing = [p for p in su.bwd_pats if not re.search(p, bwd)]
        assert not missing, (su.family, missing, bwd)
        if su.mode == "f64":                               # the no_grad forward is the kernels' head, the autograd one torch's
            out["y_autograd"] = y
        else:
            out["y"] = y
        out.update(D=dx, gp=gp)
    elif su.mode in ("vjp", "vjp64"):
        out["y"], out["D"] = m.value_and_vjp(x, G)
    elif su.mode == "jac":
        out["y"], out["D"] = m.value_and_jacobian(x)
    elif su.mode == "metric":
        out["y"], out["D"] = m.value_and_metric(x)
    torch.cuda.synchronize()
    if su.mode not in ("fwd", "grad", "f64"):
        su.note(n)
    assert torch.equal(x, x0), (su.family, "x was written")
    assert su.unwritten(), (su.family, "a parameter was written")
    return out


def _report(su, label, n, res, ratios):
    for name, (err, lim, own) in res.items():
        vs_own = err / own if own else float("nan")
        print("head extremes %s %s %s n=%d %s: error/bound %.3g, kernel/float32 oracle %.3g (kernel %.3g)" % (
            su.family, he.NAMES[su.code], label, n, name, err / lim, vs_own, err))
        key = "param" if name.startswith("param") else name
        a, b = ratios.get(key, (0.0, 0.0))
        ratios[key] = (max(a, err / lim), max(b, vs_own if vs_own == vs_own else 0.0))


def _compare(su, label, n, Ws, bs, got, ratios, problems, want=None, own=None):
    want = _oracle(su, n, Ws, bs) if want is None else want
    if own is None and not su.f64:
        own = _oracle(su, n, Ws, bs, torch.float32)
    if su.mode == "mlp_bf16":
        ref, bound, spread = he.bf16_bound(su.f[:n], Ws, bs, su.code)
        err = float((got["y"].cpu() - ref).abs().max())
        print("head extremes %s %s %s n=%d y: error/bound %.3g (the emulation's own spread %.3g of the scale)" % (
            su.family, he.NAMES[su.code], label, n, err / bound, spread))
        a, b = ratios.get("y", (0.0, 0.0))
        ratios["y"] = (max(a, err / bound), max(b, spread))
        if not (err <= bound and bool(torch.isfinite(got["y"]).all())):
            problems.append((label, n, "y against the bf16 emulation", err, bound))
        return want, {}
    res, bad = he.compare(got, want, own, su.tol)
    if "y_autograd" in got:
        res2, bad2 = he.compare({"y": got["y_autograd"]}, {"y": want["y"]}, None, su.tol)
        res["y under autograd"] = res2["y"]
        bad += bad2
    if "gp_data" in got:
        pick = lambda d: None if d is None else {"y": d["y"], "gp": d["gp"]}
        res2, bad2 = he.compare({"y": got["y_data"], "gp": got["gp_data"]}, pick(want), pick(own), su.tol)
        res.update(("%s, x as data" % k, v) for k, v in res2.items())
        bad += [("%s, x as data" % b[0],) + tuple(b[1:]) for b in bad2]
    _report(su, label, n, res, ratios)
    problems += [(label, n) + tuple(b) for b in bad]
    return want, res


def _live_blocks(gp, dims):
    """The live sub-network's blocks of [dW1, db1, dW2, ...] and the cut units' rows."""
    live = he.live_units(dims)
    blocks, cut, prev = [], [], list(range(dims[0]))
    for l in range(len(dims) - 1):
        rows = live[l] if l < len(live) else list(range(dims[-1]))
        dead = [j for j in range(dims[l + 1]) if j not in rows]
        W, b = gp[2 * l], gp[2 * l + 1]
        blocks += [W[rows][:, prev], b[rows]]
        cut += [W[dead], b[dead]]
        prev = rows
    return blocks, cut


@pytest.mark.parametrize("family,code", CASES, ids=["%s-%s" % (f, he.NAMES[c]) for f, c in CASES])
def test_head_extremes(family, code, hip_device, monkeypatch):
    for k, v in FAMILIES[family][3].items():
        monkeypatch.setenv(k, v)
    su = Setup(family, code, hip_device)
    if su.mode == "mlp_bf16":
        g = torch.Generator().manual_seed(1)
        f = torch.randn(5, su.dims[0], generator=g)
        Ws, bs = he.params(su.dims, "mixed")
        assert torch.equal(he.emulate_bf16(f, Ws, bs, code), tmc._emulate(f, Ws, bs, code))
    ratios, problems, plans = {}, [], None
    for label, regime, part, (Ws, bs) in he.parameter_sets(su.dims, su.dtype):
        su.write(Ws, bs)
        su.phase = label
        for n in (N, 1, 65) if regime == "mixed" else (N,):
            got = _run(su, n)
            want, res = _compare(su, label, n, Ws, bs, got, ratios, problems)
            if regime == "pinned" and got["gp"]:
                units = he.pinned_units(su.dims, su.dtype, part)
                problems += [(label,) + tuple(b) for b in he.check_pinned(got["gp"], want, want["f"], code, units,
                                                                         (res["param 0"][1], res["param 1"][1]))]
        if plans is None:
            plans = _cached_plans()
        if regime == "mixed":                              # isolation
            Wz, (Wl, bl) = he.isolate(Ws, bs, su.dims)
            su.write(Wz, bs)
            su.phase = "isolation"
            got = _run(su, N)
            live = _oracle(su, N, Wl, bl)
            live32 = None if su.f64 else _oracle(su, N, Wl, bl, torch.float32)
            if got["gp"]:
                blocks, cut = _live_blocks(got["gp"], su.dims)
                leak = [i for i, t in enumerate(cut) if t.numel() and float(t.abs().max()) != 0.0]
                if leak:
                    problems.append(("isolation", "gradient rows of cut units are not zero", leak))
                got = dict(got, gp=blocks)
                if "gp_data" in got:
                    got["gp_data"] = _live_blocks(got["gp_data"], su.dims)[0]
            _compare(su, "isolation", N, Wz, bs, got, ratios, problems, want=live, own=live32)
    later = [v for k, v in su.long_infos.items() if k != "control"]       # (the first regime's runs are the ones that build)
    if any(v != later[0] for v in later):
        problems.append(("the launch info changed between regimes", su.long_infos))
    if plans is not None and _cached_plans() != plans:
        problems.append(("plans were built after the first regime", plans, _cached_plans()))
    seen = " | ".join(su.infos)
    missing = [p for p in su.fwd_pats + su.bwd_pats if not re.search(p, seen)]
    RATIOS[(family, he.NAMES[code])] = ratios
    assert not missing, (family, missing, seen)
    assert not problems, (family, he.NAMES[code], problems)
    REACHED.add((family, code))


@pytest.mark.parametrize("code", he.UNSERVED, ids=[he.NAMES[c] for c in he.UNSERVED])
@pytest.mark.parametrize("spec,widths", [("ala_pos", [16, 8, 4]), ("ala", [100, 70, 3])], ids=["small", "wide"])
def test_unserved_activations(spec, widths, code, hip_device):
    """act_derivative answers 1.0 for these codes; only the plans' gate keeps a backward kernel from being built for them."""
    xyz, align, items = aet._spec(spec)
    dims = [sum(mo.feature_dim(t, len(i), False) for t, i in items)] + widths
    pp = rb.Case(spec, xyz, items, align, False, None).build(torch.device("cpu"))
    with torch.random.fork_rng(devices=[]):
        model = MolANN(pp, create_sequential_nn(dims, activation=he.MODULE[code]())).to(hip_device)
    lins = [m for m in model.ann_layers if isinstance(m, torch.nn.Linear)]
    Ws, bs = he.params(dims, "mixed")
    with torch.no_grad():
        for lin, w, b in zip(lins, Ws, bs):
            lin.weight.copy_(w)
            lin.bias.copy_(b)
    x = torch.from_numpy(_frames(spec)).to(hip_device)
    plan = model.plan_for(x)
    assert plan is not None and not plan.supports_backward() and not plan.supports_mlp_backward()
    G = torch.randn(N, dims[-1], generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    y, dx, gp, fwd, bwd = fft._run(model, x, G.to(hip_device, torch.float32), "grad")
    seen = fwd + " | " + bwd
    assert not re.search(HEAD_BWD, seen), seen
    assert set(re.findall(r"molann_lane_jit<NL=(\d+)", seen)) <= {"0"}, seen       # a one-pass backward serves the features alone
    ref = rb._align_layer(model).ref_x.detach().cpu().double()
    outs = []
    for dtype in (torch.float64, torch.float32):
        xx = x.detach().cpu().to(dtype).requires_grad_(True)
        W = [w.to(dtype).requires_grad_(True) for w in Ws]
        b = [t.to(dtype).requires_grad_(True) for t in bs]
        yy = he.head(mo.preprocessing_forward(xx, items, False, align, ref.to(dtype)), W, b, code)
        g = torch.autograd.grad((yy * G.to(dtype)).sum(), [xx] + [t for pair in zip(W, b) for t in pair])
        outs.append({"y": yy.detach(), "D": g[0], "gp": list(g[1:])})
    res, bad = he.compare({"y": y, "D": dx, "gp": gp}, outs[0], outs[1], "f32")
    for name, (err, lim, own) in res.items():
        print("head extremes unserved %s %s %s: error/bound %.3g, kernel/float32 oracle %.3g" % (
            spec, he.NAMES[code], name, err / lim, err / own if own else float("nan")))
    assert not bad, (spec, he.NAMES[code], bad)
    assert all(torch.equal(lin.weight.detach().cpu(), w) and torch.equal(lin.bias.detach().cpu(), t) for lin, w, t in zip(lins, Ws, bs))
    REACHED.add(("unserved", spec, code))


def test_every_head_extreme_family_was_reached(request):
    """The cases are recorded as they pass, so this guard needs all of them in the same session."""
    here = {item.name for item in request.session.items if item.module is request.module}
    wanted = {"test_head_extremes[%s-%s]" % (f, he.NAMES[c]) for f, c in CASES} | \
             {"test_unserved_activations[%s-%s]" % (s, he.NAMES[c]) for s in ("small", "wide") for c in he.UNSERVED}
    if not wanted <= here:
        pytest.skip("the coverage guard needs every family in this session: %d not selected" % len(wanted - here))
    missing = sorted((set(CASES) | {("unserved", s, c) for s in ("ala_pos", "ala") for c in he.UNSERVED}) - REACHED, key=str)
    for key in sorted(RATIOS, key=str):
        print("head extremes ratios %s %s: %s" % (key[0], key[1], " ".join("%s=%.2g/%.2g" % (k, a, b) for k, (a, b) in RATIOS[key].items())))
    assert not missing, ("not reached:", missing)
