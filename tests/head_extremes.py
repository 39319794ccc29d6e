"""Head parameters that push an MLP head's hidden pre-activations z out of the +-2 the default initialisation keeps them in behind
features of order 1, for the tests of every activation copy (tests/test_head_extremes_host.py, test_gpu_head_extremes.py), and the
plain torch head those tests compare with.  No GPU.

`params(dims, regime, ...)` starts from torch.nn.Linear's default initialisation under a seed (what create_sequential_nn gives) and
is deterministic.  A hidden layer is every Linear but the last.  Regimes:

  control     the default initialisation
  mixed       row j of every hidden layer's W and b times MIXED_FACTORS[j % 6] = (1, 1, 4, 16, 64, 256): every frame has live units
              next to saturated ones (powers of two: the products are exact in float32)
  saturated   every hidden row times 64
  pinned      the first k = min(len(list), width // 2) units of the first hidden layer get a zero weight row and a bias from
              `pinned_values`, so z is that bias on every frame; the other units as in control.  A layer narrower than twice the
              list takes it in `n_parts` slices, one parameter set each.

The pinned list holds the places where the activation code changes branch or leaves a format's range: the kink (+-0, +-1e-8),
softplus's threshold (20 and its neighbours), sigmoid' = 0 in float32 (30), expf's overflow (88 / 89), exp2's (104 ~ 150 ln 2 / 1,
130), and exp's in double (750).  Every value is finite.

`bands(z)` is the share of pre-activations with |z| in [0,2), [4,8), [8,20), [20,88.7) and >= 88.7 (|z| in [2,4) is in no band)."""

import numpy as np
import torch

F = torch.nn.functional
TANH, RELU, SIGMOID, IDENTITY, ELU, SILU, SOFTPLUS, LEAKY_RELU, GELU = range(9)
NAMES = ("tanh", "relu", "sigmoid", "identity", "elu", "silu", "softplus", "leaky_relu", "gelu")
FN = {TANH: torch.tanh, RELU: F.relu, SIGMOID: torch.sigmoid, IDENTITY: lambda t: t, ELU: F.elu, SILU: F.silu,
      SOFTPLUS: F.softplus, LEAKY_RELU: F.leaky_relu, GELU: F.gelu}
MODULE = {TANH: torch.nn.Tanh, RELU: torch.nn.ReLU, SIGMOID: torch.nn.Sigmoid, IDENTITY: torch.nn.Identity, ELU: torch.nn.ELU,
          SILU: torch.nn.SiLU, SOFTPLUS: torch.nn.Softplus, LEAKY_RELU: torch.nn.LeakyReLU, GELU: torch.nn.GELU}
ALL = tuple(range(9))
SERVED = (TANH, RELU, SIGMOID, IDENTITY, SILU, LEAKY_RELU)      # act_served(): what the fp32 backward kernels differentiate
UNSERVED = (ELU, SOFTPLUS, GELU)
KINKED = (RELU, LEAKY_RELU)
REGIMES = ("control", "mixed", "saturated", "pinned")
MIXED_FACTORS = (1, 1, 4, 16, 64, 256)
# The seed of the default initialisation.  A property of the inputs, chosen for them: on C3's features and a [6, 16, 8, 4] head
# `saturated` leaves 62 % of the frames without a first-layer unit in [0,2) under this seed (seeds 0 - 7: 27 - 62 %), and the host
# test asks for half.
SEED = 4
BAND_EDGES = ((0.0, 2.0), (4.0, 8.0), (8.0, 20.0), (20.0, 88.7), (88.7, float("inf")))


def pinned_values(dtype=torch.float32):
    """The pinned biases as a tensor of `dtype` (float32 or float64)."""
    np_t = np.float32 if dtype == torch.float32 else np.float64
    twenty = np_t(20.0)
    v = [0.0, -0.0, 1e-8, -1e-8, 20.0, float(np.nextafter(twenty, np_t(np.inf))), float(np.nextafter(twenty, np_t(-np.inf))),
         30.0, -30.0, 88.0, -88.0, 89.0, -89.0, 104.0, -104.0, 130.0, -130.0]
    if dtype == torch.float64:
        v += [750.0, -750.0]
    return torch.tensor(v, dtype=dtype)


def _pinned_per_part(dims, dtype):
    return min(len(pinned_values(dtype)), dims[1] // 2)


def n_parts(dims, dtype=torch.float32):
    """How many parameter sets the pinned list takes on this head."""
    k = _pinned_per_part(dims, dtype)
    return -(-len(pinned_values(dtype)) // k)


def pinned_units(dims, dtype=torch.float32, part=0):
    """[(unit of the first hidden layer, its bias)] of one part."""
    vals, k = pinned_values(dtype), _pinned_per_part(dims, dtype)
    return [(j, vals[i]) for j, i in enumerate(range(part * k, min(len(vals), (part + 1) * k)))]


def default(dims, seed=SEED):
    """(Ws, bs) float32 on the CPU: torch.nn.Linear's default initialisation under `seed`; the global generator is left as it was."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        lins = [torch.nn.Linear(k, j) for k, j in zip(dims[:-1], dims[1:])]
    return [l.weight.detach().clone() for l in lins], [l.bias.detach().clone() for l in lins]


def params(dims, regime, dtype=torch.float32, seed=SEED, part=0):
    """(Ws, bs) of `dtype` on the CPU for a head of widths `dims` (features first): the float32 default initialisation, scaled or
    pinned as the regime says.  float64 parameters are the float32 ones widened, except the pinned biases of float64's own list."""
    assert regime in REGIMES and len(dims) >= 3, (regime, dims)
    Ws, bs = default(dims, seed)
    Ws, bs = [w.to(dtype) for w in Ws], [b.to(dtype) for b in bs]
    for l in range(len(Ws) - 1):
        if regime == "mixed":
            fac = torch.tensor([MIXED_FACTORS[j % 6] for j in range(dims[l + 1])], dtype=dtype)
        elif regime == "saturated":
            fac = torch.full((dims[l + 1],), 64.0, dtype=dtype)
        else:
            continue
        Ws[l] *= fac[:, None]
        bs[l] *= fac
    if regime == "pinned":
        for j, v in pinned_units(dims, dtype, part):
            Ws[0][j] = 0.0
            bs[0][j] = v
    return Ws, bs


def parameter_sets(dims, dtype=torch.float32, seed=SEED):
    """[(label, regime, part, (Ws, bs))]: every regime, pinned once per part."""
    out = [(r, r, 0, params(dims, r, dtype, seed)) for r in REGIMES[:3]]
    return out + [("pinned%d" % p, "pinned", p, params(dims, "pinned", dtype, seed, p)) for p in range(n_parts(dims, dtype))]


def live_units(dims):
    """Per hidden layer, the units `mixed` leaves at factor 1."""
    return [[j for j in range(dims[l + 1]) if MIXED_FACTORS[j % 6] == 1] for l in range(len(dims) - 2)]


def isolate(Ws, bs, dims):
    """`mixed` with the saturated units' outgoing weights zeroed, and the live sub-network (Ws, bs) that must compute the same."""
    live = live_units(dims)
    Wz = [w.clone() for w in Ws]
    for l, keep in enumerate(live):
        dead = [j for j in range(dims[l + 1]) if j not in keep]
        Wz[l + 1][:, dead] = 0.0
    Wl, bl, prev = [], [], list(range(dims[0]))
    for l in range(len(Ws)):
        rows = live[l] if l < len(live) else list(range(dims[-1]))
        Wl.append(Ws[l][rows][:, prev].clone())
        bl.append(bs[l][rows].clone())
        prev = rows
    return Wz, (Wl, bl)


def head(f, Ws, bs, code, keep=False):
    """Linear -> act -> ... -> Linear in the dtype of f; keep: also the hidden pre-activations and activations [(z, h)]."""
    h, kept = f, []
    for i, (w, b) in enumerate(zip(Ws, bs)):
        z = F.linear(h, w.to(h.dtype), b.to(h.dtype))
        if i + 1 == len(Ws):
            return (z, kept) if keep else z
        h = FN[code](z)
        if keep:
            kept.append((z, h))


def hidden_z(f, Ws, bs, code):
    """The hidden pre-activations of every layer [N, sum of hidden widths], float64."""
    with torch.no_grad():
        _, kept = head(f.double(), [w.double() for w in Ws], [b.double() for b in bs], code, keep=True)
    return torch.cat([z for z, _ in kept], 1)


def bands(z):
    """[..., 5]: the share of the last axis of z with |z| in each of BAND_EDGES."""
    a = z.abs()
    return torch.stack([((a >= lo) & (a < hi)).double().mean(-1) for lo, hi in BAND_EDGES], -1)


def act_derivative(code, z):
    """d act / d z at the values z by torch autograd in z's dtype (torch's convention at a kink)."""
    zz = z.detach().clone().requires_grad_(True)
    (g,) = torch.autograd.grad(FN[code](zz).sum(), zz)
    return g


def _bf16(t):
    return t.to(torch.bfloat16).to(torch.float32)


def emulate_bf16(f, Ws, bs, code, ulp=0):
    """The bf16 head's arithmetic model, test_gpu_mlp_chain._emulate for any activation: bf16 weights and features, float32 sums,
    the activation in float32 rounded to bf16.  `ulp` = +-1 moves every activation by one float32 ulp before that rounding: the
    spread between the three results is what bf16 rounding knife-edges alone can move the outputs by."""
    h = _bf16(f.detach().cpu().float()).double()
    for i, (w, b) in enumerate(zip(Ws, bs)):
        z = (h @ _bf16(w.detach().cpu().float()).double().T + b.detach().cpu().double()).float()
        if i + 1 == len(Ws):
            return z
        a = FN[code](z)
        if ulp:
            a = torch.nextafter(a, torch.full_like(a, float("inf") if ulp > 0 else float("-inf")))
        h = _bf16(a).double()


def bf16_bound(f, Ws, bs, code):
    """(reference, bound, spread): test_gpu_mlp_chain.py's 4e-3 of the output's scale, or twice the emulation's own spread under
    +-1 ulp where that is more."""
    ref = emulate_bf16(f, Ws, bs, code)
    spread = max(float((emulate_bf16(f, Ws, bs, code, s) - ref).abs().max()) for s in (1, -1))
    scale = max(1.0, float(ref.abs().max()))
    return ref, max(4e-3 * scale, 2.0 * spread), spread / scale


# ---- the comparisons both test files make --------------------------------------------------------------------------------------
TOL = {"f32": (1e-5, 5e-4), "wide_bwd": (1e-5, 2e-4), "f64": (1e-10, 1e-9)}


def _rows(t):
    return t.detach().cpu().double().flatten(1)


def row_error(got, want):
    """Per frame: the largest error of a derivative row over that frame's scale (its largest entry, floored at 1e-3 of the
    batch's), as test_gpu_angular_edges.py."""
    w = _rows(want)
    s = w.abs().amax(1)
    s = s.clamp(min=max(1e-3 * float(s.max()), 1e-300))
    return (_rows(got) - w).abs().amax(1) / s


def compare(got, want, own, kind):
    """got / want / own: {y, D (per-frame derivative rows or None), gp (parameter gradients)} of the kernel, the float64 oracle
    and the oracle in float32 (None for float64 kernels).  Returns ({check: (error, bound, own error)}, [failures]); a bound is
    max(the tolerance of `kind`, 2 x the float32 oracle's own error), outputs relative to the batch's scale, derivative rows to
    each frame's, parameter gradients to each tensor's."""
    tol_y, tol_d = TOL[kind]
    res, bad = {}, []

    def note(name, err, tol, own_err):
        lim = tol if own_err is None else max(tol, 2.0 * own_err)
        res[name] = (err, lim, own_err)
        if not err <= lim:
            bad.append((name, err, lim))

    scale = max(1.0, float(want["y"].abs().max()))
    note("y", float((_rows(got["y"]) - _rows(want["y"])).abs().max()) / scale, tol_y,
         None if own is None else float((_rows(own["y"]) - _rows(want["y"])).abs().max()) / scale)
    if want.get("D") is not None:
        note("D", float(row_error(got["D"], want["D"]).max()), tol_d, None if own is None else float(row_error(own["D"], want["D"]).max()))
    gp_w = want.get("gp") or []
    assert len(got.get("gp") or []) == len(gp_w), (len(got.get("gp") or []), len(gp_w))
    for i, w in enumerate(gp_w):
        s = max(1e-6, float(w.abs().max()))
        note("param %d" % i, float((got["gp"][i].detach().cpu().double() - w).abs().max()) / s, tol_d,
             None if own is None else float((own["gp"][i].double() - w).abs().max()) / s)
    for k in ("y", "D"):
        if got.get(k) is not None and not bool(torch.isfinite(got[k]).all()):
            bad.append((k, "not finite"))
    for i, p in enumerate(got.get("gp") or []):
        if not bool(torch.isfinite(p).all()):
            bad.append(("param %d" % i, "not finite"))
    return res, bad


def head_oracle(f, Ws, bs, code, G, dtype=torch.float64, grads=True):
    """{y, D = dL/df, gp = [dW1, db1, dW2, ...], u1 = dL/dh1 [N, width]} of L = sum(head(f) * G) by autograd in `dtype` on the CPU."""
    ff = f.detach().cpu().to(dtype).requires_grad_(grads)
    Ws = [w.detach().cpu().to(dtype).requires_grad_(grads) for w in Ws]
    bs = [b.detach().cpu().to(dtype).requires_grad_(grads) for b in bs]
    y, kept = head(ff, Ws, bs, code, keep=True)
    out = {"y": y.detach(), "D": None, "gp": [], "u1": None}
    if grads:
        prm = [t for pair in zip(Ws, bs) for t in pair]
        g = torch.autograd.grad((y * G.detach().cpu().to(dtype)).sum(), [ff, kept[0][1]] + prm)
        out.update(D=g[0], u1=g[1], gp=list(g[2:]))
    return out


def pinned_rows(want, f, code, units, dtype=torch.float64):
    """What the pinned units' rows of db1 and dW1 must be: sum_n u[n, j] act'(b_j) and sum_n u[n, j] act'(b_j) f[n, :], from the
    upstream gradient u = dL/dh1 of the float64 oracle and torch's derivative at exactly b_j.  [(j, db1_j, dW1_j)]."""
    out = []
    for j, v in units:
        d = float(act_derivative(code, v.double().reshape(1))[0])
        u = want["u1"][:, j].double()
        out.append((j, float(u.sum()) * d, (u[:, None] * f.detach().cpu().double()).sum(0) * d))
    return out


def check_pinned(got_gp, want, f, code, units, lims):
    """The pinned rows of the kernel's dL/db1 (got_gp[1]) and dL/dW1 (got_gp[0]) against `pinned_rows`, within the bounds
    `compare` gave those two tensors (lims = (bound of dW1, bound of db1), relative to the tensor's scale); a unit at +-0 follows
    torch's kink convention: exactly 0 for ReLU.  Returns the failures."""
    bad = []
    sW, sb = max(1e-6, float(want["gp"][0].abs().max())), max(1e-6, float(want["gp"][1].abs().max()))
    for (j, db, dW), (_, v) in zip(pinned_rows(want, f, code, units), units):
        gb, gW = float(got_gp[1][j]), got_gp[0][j].detach().cpu().double()
        if not abs(gb - db) <= lims[1] * sb:
            bad.append(("db1", j, float(v), gb, db))
        if not float((gW - dW).abs().max()) <= lims[0] * sW:
            bad.append(("dW1", j, float(v), float((gW - dW).abs().max())))
        if code == RELU and float(v) == 0.0 and not (gb == 0.0 and float(gW.abs().max()) == 0.0):
            bad.append(("ReLU' at the kink is not 0", j, gb))
    return bad
