"""Every kernel family that inlines the item arithmetic of molann_amd/csrc/molann_math.h, on frames at angular extremes
(tests/angular_edges.py): a bond angle within 10 to 0.1 degrees of straight or folded, a dihedral at cis or trans where atan2
wraps, a dihedral with a nearly collinear arm.  The suite's other gradient tests mask exactly these frames; here none is left out.

FAMILIES names, per family, a spec (ALA dipeptide, a 166-atom chain or a 2000-atom chain, each with one angle, two dihedrals and
a bond - the fp32 rotation solve - or with a position item added - the float64 solve and the G_R sums), a head, the environment
switches that route it, the mode, and the kernels last_launch_info must show; every family is built with use_angle_value False
and True, one model shared by the five regimes, and a final guard needs every family reached.

Per family and regime one batch interleaves the graded deltas with near frames (angular_edges.interleaved).  Checked on it:
  - outputs, and dL/dx and dL/d(parameters) (or the Jacobian, the metric, the bias and its forces, the tangents), against float64
    autograd through the oracle on EVERY frame, gradients scaled per frame (each frame's largest entry, floored at 1e-3 of the
    batch's, as test_gpu_jvp.py).  float32: max(the tolerance of test_gpu_far_frames.py - 1e-5 of the scale for outputs, 5e-4 for
    gradients, 1e-4 for tangents as test_gpu_jvp_plans.py -, 2 x the largest error of the oracle run in float32 on the CPU on the
    frames of the same regime and delta).  float64: 1e-10 for values, 1e-9 for derivatives, at every delta;
  - dihedral values modulo 2 pi.  Behind a head a value cannot be wrapped, so a frame within 1e-5 rad (float32; 1e-12 float64) of
    the seam - where float32's rounding of atan2's arguments, 1e-6, decides the side - is held to the oracle with that dihedral on
    the side the kernel's output is closer to; every other frame to the oracle as it is;
  - x never written.
A second batch swaps the graded frames for pole frames (0.03 degrees and 0; straight, folded and arm only):
  - bit for bit: a near frame's output row and derivative rows are those of the graded batch (a NaN or a huge value must not
    cross a lane group, a ring entry or a wave reduction), except the rows of the atomics family;
  - outputs of the cosine and (cos, sin) forms within the ordinary tolerance (straight / folded; for arm, whose dihedral has no
    value at the pole, the other items' columns where the features are the outputs);
  - the invariant of the angle-value gradient (straight / folded, use_angle_value): the rows of the angle's end atom - no other
    item's, in no alignment set - are non-finite, as the reference's autograd gives, or no longer than
    (1 + 1e-3) |dL/d theta| / |arm|.  dL/d theta is the cotangent's column where the features are the outputs, the derivative of
    the bias at the kernel's own outputs for the restraint and the hills, and behind a head its largest value over theta within
    1.5e-3 rad of the true angle (float32's acos is off by up to 6e-4 there) in float64.  A tangent obeys
    |d theta| <= (1 + 1e-3) (|t0 - t1| / |u| + |t2 - t1| / |v|), the metric's diagonal the squares of the three rows' bounds.
Restraint and hills run on dihedral values with period 2 pi, centres at -+(pi - 1e-3) against frames at +-(pi - delta): the
short way round the seam.  frames_hvp_kernel runs on trans / cis with the cosine forms, under test_gpu_second_order_exact.py's
1e-12.  Each check prints kernel error / reference error before it asserts.

DESIGN.md, "Angular extremes", has the measured ratios of one MI355X."""

import copy
import math
import re

import numpy as np
import pytest
import torch

import angular_edges as ae
import test_gpu_far_frames as fft
import test_gpu_random_backward as rb
from molann_amd import _capi
from molann_amd import workloads as wl
from molann_amd.ann import MolANN
from oracle import molann_oracle as mo

pytestmark = pytest.mark.gpu
ANGLE, BOND, DIH, POS = wl.ANGLE, wl.BOND, wl.DIHEDRAL, wl.POSITION
TWO_PI = 2.0 * math.pi
REACHED = set()
RATIOS = {}                                                # (family, uav, regime) -> the largest error / bound of each check


def _chain(n, seed):
    return wl.synthetic_chain(n_atoms=n, step=1.4, seed=seed)


def _spec(name):
    """(xyz, align, items): the edge items' end atoms (angle: third, first dihedral: fourth, second dihedral: first) are no other
    item's and in no alignment set; for ALA everything sits in the first 16 slots (the lane kernel's regs mode)."""
    pos = name.endswith("_pos")
    if name.startswith("ala"):
        items = [(ANGLE, [1, 4, 5]), (DIH, [4, 6, 8, 14]), (DIH, [12, 10, 8, 9]), (BOND, [1, 4])]
        return wl.ALA_DIPEPTIDE_XYZ, [0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11, 13, 15], items + ([(POS, [0, 2, 3])] if pos else [])
    if name.startswith("c166"):
        items = [(ANGLE, [20, 21, 23]), (DIH, [40, 41, 42, 43]), (DIH, [91, 92, 93, 94]), (BOND, [120, 121])]
        return _chain(166, 11), fft.P_SEL, items + ([(POS, list(range(10, 160, 19)))] if pos else [])
    if name.startswith("c2000"):
        items = [(ANGLE, [100, 101, 103]), (DIH, [500, 501, 502, 504]), (DIH, [1500, 1501, 1502, 1503]), (BOND, [1900, 1901])]
        return _chain(2000, 5), list(range(7, 2000, 13)), items + ([(POS, list(range(31, 2000, 97)))] if pos else [])
    raise KeyError(name)


# family: (spec, head widths after the features or None, environment, mode, forward kernels, backward kernel or None, frames).
# modes: fwd (no_grad forward), grad (float32 autograd), f64 (model.double() autograd), vjp / vjp64 (value_and_vjp), jac, metric,
# restraint, hills (the float64 one-launch entry points), jvp32 / jvp64 (torch.func.jvp of the features).
RING = r"frames_ring_kernel<ND=\d+,B=%d>"
FAMILIES = {
    "lane_jit_bwd_ring": ("ala_pos", [16, 4], {}, "grad", (r"molann_lane_jit<NL=2>",), r"molann_bwd_ring ", 256),
    "lane_jit_bwd_ring_f32_solve": ("ala", [16, 4], {}, "grad", (r"molann_lane_jit<NL=2>",), r"molann_bwd_ring ", 256),
    "lane_bwd": ("ala_pos", [16, 4], {"MOLANN_NO_RING_BWD": "1"}, "grad", (r"molann_lane_jit<NL=",), r"molann_lane_bwd", 256),
    "lane_regs": ("ala", None, {"MOLANN_NO_JIT": "1"}, "fwd", (r"frames_lane_kernel<\d+,features_regs>",), None, 256),
    "lane_lds": ("ala_pos", None, {"MOLANN_NO_JIT": "1", "MOLANN_NO_REGS": "1"}, "fwd", (r"frames_lane_kernel<\d+,features_lds>",),
                 None, 256),
    "lane_vjp": ("ala_pos", [16, 4], {}, "vjp", (r"molann_bwd_ring<values>",), None, 256),
    "ring_B8_group_bwd": ("c166_pos", [32, 8], {}, "grad", (RING % 8,), r"frames_group_bwd_kernel<B=", 192),
    "ring_B1": ("c166", [16, 4], {"MOLANN_RING_BATCH": "1"}, "fwd", (r"frames_ring_kernel<ND=\d+> ",), None, 192),
    "wave_166": ("c166_pos", None, {"MOLANN_NO_RING": "1"}, "fwd", (r"frames_wave_kernel<",), None, 192),
    "wave_2000": ("c2000_pos", None, {"MOLANN_NO_RING": "1"}, "fwd", (r"frames_wave_kernel<",), None, 192),
    "wave_gather_2000": ("c2000_pos", None, {}, "grad", (r"frames_(ring|wave)_kernel<",), r"frames_wave_bwd_gather_kernel", 192),
    "wave_atomics_2000": ("c2000", None, {"MOLANN_BWD_ATOMICS": "1"}, "grad", (r"frames_(ring|wave)_kernel<",), r"frames_wave_bwd_kernel",
                          192),
    "group_vjp": ("c166_pos", [16, 4], {}, "vjp", (r"molann_group_vjp<B=",), None, 192),
    "f64_bwd": ("c166_pos", [32, 8], {}, "f64", (r"frames_f64_kernel \(features\)",), r"frames_bwd_f64_kernel", 192),
    "vjp_f64": ("ala_pos", [16, 4], {}, "vjp64", (r"frames_value_vjp_f64_kernel",), None, 256),
    "jac_f64": ("c166", [16, 4], {}, "jac", (r"frames_value_jac_f64_kernel",), None, 192),
    "metric_f64": ("c166_pos", None, {}, "metric", (r"frames_value_metric_f64_kernel",), None, 192),
    "restraint_f64": ("ala", None, {}, "restraint", (r"frames_value_restraint_f64_kernel",), None, 256),
    "hills_f64": ("c166", None, {}, "hills", (r"frames_value_hills_f64_kernel",), None, 192),
    "jvp_f32": ("c166_pos", None, {}, "jvp32", (r"frames_jvp_kernel",), None, 192),
    "jvp_f64": ("ala_pos", None, {}, "jvp64", (r"frames_jvp_f64_kernel",), None, 256),
}
ATOMICS = ("wave_atomics_2000",)                           # dL/dx summed by atomics: not bitwise reproducible
F64_MODES = ("f64", "vjp64", "jac", "metric", "restraint", "hills", "jvp64")
N_TANGENTS = 2


_BATCHES = {}


def _batch(spec, regime, deltas, n, seed):
    """angular_edges.interleaved for a spec, kept for the families that share it."""
    key = (spec, regime, tuple(deltas), n, seed)
    if key not in _BATCHES:
        xyz, align, items = _spec(spec)
        _BATCHES[key] = ae.interleaved(regime, deltas, xyz, items, n, seed=seed, align=align)
    return _BATCHES[key]


class Setup(object):
    """One family's model and what the checks need to know about its plan."""

    def __init__(self, family, uav, dev):
        self.family, self.uav, self.dev = family, uav, dev
        spec, head, _, self.mode, self.fwd_pats, self.bwd_pat, self.n = FAMILIES[family]
        self.spec = spec
        self.xyz, self.align, self.items = _spec(spec)
        d = sum(mo.feature_dim(t, len(i), uav) for t, i in self.items)
        self.case = rb.Case(spec, self.xyz, self.items, self.align, uav, None if head is None else [d] + head)
        self.f64 = self.mode in F64_MODES
        self.dtype = torch.float64 if self.f64 else torch.float32
        model = self.case.build(dev)
        self.model = copy.deepcopy(model).double() if self.f64 else model
        if self.mode not in ("grad", "f64"):
            self.model.requires_grad_(False)
        self.ref = rb._align_layer(self.model).ref_x.detach().cpu().double()
        self.head = rb._head64(self.model) if head is not None else None
        self.d_feat, self.d_out = d, (head[-1] if head is not None else d)
        # the columns of the edge items in the feature row, and which feature columns are angles modulo 2 pi
        col, self.cols, self.periodic = 0, {}, torch.zeros(d, dtype=torch.bool)
        by_item = {v: k for k, v in ae.roles(self.items).items()}
        for i, (t, idx) in enumerate(self.items):
            w = mo.feature_dim(t, len(idx), uav)
            if i in by_item:
                self.cols[by_item[i]] = col
            if t == DIH and uav:
                self.periodic[col] = True
            col += w
        self.infos = []

    def pre(self):
        return self.model.preprocessing_layer if isinstance(self.model, MolANN) else self.model

    def note(self):
        self.infos.append(fft._infos(self.model))
        return self.infos[-1]


# ---- the oracle ------------------------------------------------------------------------------------------------------------
def _wrapped(d, period):
    return d - period * torch.round(d / torch.where(period > 0, period, torch.ones_like(period))) * (period > 0)


def _bias(su, y, extra):
    """The restraint's energy / the hills' bias [N] on outputs y, the composition the kernels implement."""
    if su.mode == "restraint":
        center, kappa, period = (t.to(y.dtype) for t in extra)
        d = _wrapped(y - center, period)
        return 0.5 * (kappa * d * d).sum(1)
    centers, heights, sigma, period = (t.to(y.dtype) for t in extra)
    d = _wrapped(y.unsqueeze(1) - centers.unsqueeze(0), period)       # [N, H, d]
    return (heights * torch.exp(-0.5 * ((d / sigma) ** 2).sum(2))).sum(1)


def _oracle(su, x, extra, dtype=torch.float64, shift=None):
    """{y, D, E, gp} of the mode's quantities through the oracle in dtype on the CPU: D the derivative rows per frame (dL/dx, the
    Jacobian [N, d, n, 3], the metric [N, d, d], the tangents [N, T, d]), E the bias, gp the parameter gradients.  `shift`
    [N, d_feat] is added to the features before the head (a dihedral value moved across the seam)."""
    xx = x.detach().cpu().to(dtype).requires_grad_(True)
    ref = su.ref.to(dtype)
    head = copy.deepcopy(su.head).to(dtype) if su.head is not None else None

    def fwd(a):
        f = mo.preprocessing_forward(a, su.items, su.uav, su.align, ref)
        if shift is not None:
            f = f + shift.to(dtype)
        return head(f) if head is not None else f

    out = {"D": None, "E": None, "gp": []}
    if su.mode in ("jvp32", "jvp64"):
        ts = [torch.func.jvp(fwd, (xx.detach(),), (v.detach().cpu().to(dtype),)) for v in extra]
        out["y"], out["D"] = ts[0][0].detach(), torch.stack([t for _, t in ts], 1).detach()
        return out
    y = fwd(xx)
    out["y"] = y.detach()
    if su.mode == "fwd":
        return out
    if su.mode in ("jac", "metric"):
        J = torch.stack([torch.autograd.grad(y[:, k].sum(), xx, retain_graph=True)[0] for k in range(y.shape[1])], 1)
        out["D"] = J if su.mode == "jac" else torch.einsum("nkac,nlac->nkl", J, J)
        return out
    if su.mode in ("restraint", "hills"):
        E = _bias(su, y, extra)
        out["E"], out["D"] = E.detach(), torch.autograd.grad(E.sum(), xx)[0]
        return out
    prm = [p.requires_grad_(True) for p in head.parameters()] if (head is not None and su.mode in ("grad", "f64")) else []
    g = torch.autograd.grad((y * extra.cpu().to(dtype)).sum(), [xx] + prm)
    out["D"], out["gp"] = g[0], list(g[1:])
    return out


def _run(su, x, extra):
    """The family's kernels on x: the same dictionary as `_oracle`, on the device; x is never written."""
    m, x0 = su.model, x.clone()
    out = {"D": None, "E": None, "gp": []}
    if su.mode == "fwd":
        with torch.no_grad():
            out["y"] = m(x)
    elif su.mode in ("grad", "f64"):
        y, dx, gp, fwd, bwd = fft._run(m, x, extra, "grad")
        su.infos += [fwd, bwd]
        if su.bwd_pat is not None:
            assert re.search(su.bwd_pat, bwd), (su.family, bwd)
        out.update(y=y, D=dx, gp=gp)
    elif su.mode in ("vjp", "vjp64"):
        out["y"], out["D"] = m.value_and_vjp(x, extra)
    elif su.mode == "jac":
        out["y"], out["D"] = m.value_and_jacobian(x)
    elif su.mode == "metric":
        out["y"], out["D"] = m.value_and_metric(x)
    elif su.mode == "restraint":
        out["y"], out["E"], out["D"] = m.value_and_restraint(x, extra[0].to(x.device), extra[1].to(x.device), extra[2].to(x.device))
    elif su.mode == "hills":
        out["y"], out["E"], out["D"] = m.value_and_hills(x, extra[0].to(x.device), extra[1].to(x.device), extra[2].to(x.device),
                                                         extra[3].to(x.device))
    else:
        ts = [torch.func.jvp(m, (x,), (v,)) for v in extra]
        out["y"], out["D"] = ts[0][0], torch.stack([t for _, t in ts], 1)
    torch.cuda.synchronize()
    su.note()
    assert torch.equal(x, x0), (su.family, "x was written")
    return {k: (v.detach() if isinstance(v, torch.Tensor) else v) for k, v in out.items()}


def _extra(su, x, regime, seed):
    """The mode's second argument: the cotangent, the tangents, or the bias's parameters (float64, on the CPU)."""
    g = torch.Generator().manual_seed(seed)
    n = x.shape[0]
    if su.mode in ("grad", "f64", "vjp", "vjp64"):
        return torch.randn((n, su.d_out), generator=g, dtype=torch.float64).to(su.dev, su.dtype)
    if su.mode in ("jvp32", "jvp64"):
        return torch.randn((N_TANGENTS,) + tuple(x.shape), generator=g, dtype=torch.float64).to(su.dev, su.dtype)
    if su.mode not in ("restraint", "hills"):
        return None
    with torch.no_grad():
        y = mo.preprocessing_forward(x.detach().cpu().double(), su.items, su.uav, su.align, su.ref)
    period = torch.where(su.periodic, torch.full((su.d_feat,), TWO_PI, dtype=torch.float64), torch.zeros(su.d_feat, dtype=torch.float64))
    tc = su.cols["tc"]
    if su.mode == "restraint":
        center = y + 0.3 * torch.randn(y.shape, generator=g, dtype=torch.float64)
        if su.uav:      # the centre across the seam from a frame at +-(pi - delta): the short way round is 1e-3 + delta
            center[:, tc] = -torch.sign(y[:, tc]) * (math.pi - 1e-3)
        return center, 0.5 + 2.5 * torch.rand(su.d_feat, generator=g, dtype=torch.float64), period
    centers = torch.stack([y[0], y[1], y.mean(0), y.mean(0)])
    if su.uav:
        centers[2, tc], centers[3, tc] = math.pi - 1e-3, -(math.pi - 1e-3)
    heights = torch.tensor([1.0, -0.5, 1.5, 1.2], dtype=torch.float64)
    sigma = 0.3 + 0.4 * torch.rand(su.d_feat, generator=g, dtype=torch.float64)
    return centers, heights, sigma, period


# ---- the checks ------------------------------------------------------------------------------------------------------------
def _rows(t):
    return t.detach().cpu().double().flatten(1)


def _y_err(su, got, want):
    d = _rows(got) - _rows(want)
    if su.head is None and bool(su.periodic.any()):
        d = torch.where(su.periodic, d - TWO_PI * torch.round(d / TWO_PI), d)
    return d.abs().amax(1)


def _seam_shift(su, x, regime, y_got, tol):
    """For a head behind dihedral values, trans frames: [N, d_feat] moving the tc dihedral of a frame within `tol` of the seam to
    the other side where the outputs y_got are closer to that branch; None when nothing is moved."""
    if su.head is None or not su.uav or regime != "trans":
        return None
    with torch.no_grad():
        f = mo.preprocessing_forward(x.detach().cpu().double(), su.items, su.uav, su.align, su.ref)
        tc = su.cols["tc"]
        seam = (math.pi - f[:, tc].abs()) < tol
        if not bool(seam.any()):
            return None
        S = torch.zeros_like(f)
        S[seam, tc] = -TWO_PI * torch.sign(f[seam, tc])
        ya, yb = su.head(f), su.head(f + S)
        got = _rows(y_got)
        other = seam & ((got - yb).abs().amax(1) < (got - ya).abs().amax(1))
        S[~other] = 0.0
    return S if bool(other.any()) else None


def _label_max(vals, labels):
    out = {}
    for v, l in zip(vals.tolist(), labels):
        out[l] = max(out.get(l, 0.0), v)
    return out


def _check_graded(su, regime, x, labels, got, extra, what):
    """Every frame of the graded batch against the float64 oracle; returns {check: largest error / bound}."""
    seam_tol = 1e-12 if su.f64 else 1e-5
    want = _oracle(su, x, extra, shift=_seam_shift(su, x, regime, got["y"], seam_tol))
    own = None
    if not su.f64:
        x32 = x.detach().cpu().float()
        first = _oracle(su, x32, extra, torch.float32)
        s_own = _seam_shift(su, x, regime, first["y"], seam_tol)
        own_want = want if s_own is None else _oracle(su, x, extra, shift=s_own)
        own = (first, own_want)
    ratios = {}
    tol_y, tol_d = (1e-10, 1e-9) if su.f64 else (1e-5, 1e-4 if su.mode == "jvp32" else 5e-4)
    scale = max(1.0, float(want["y"].abs().max()))

    def per_label(err, tol, own_err, name):
        lim = torch.full_like(err, tol)
        if own_err is not None:
            worst = _label_max(own_err, labels)
            lim = torch.maximum(lim, torch.tensor([2.0 * worst[l] for l in labels], dtype=torch.float64))
        r = err / lim
        for l, v in _label_max(r, labels).items():
            w = _label_max(own_err, labels)[l] if own_err is not None else float("nan")
            print("angular edges %s %s delta=%s %s: error/bound %.3g (kernel %.3g, float32 oracle %.3g)" % (
                what, regime, l, name, v, _label_max(err, labels)[l], w))
        ratios[name] = float(r.max())
        bad = (~(r <= 1.0)).nonzero().flatten().tolist()
        return [(name, i, labels[i], float(err[i]), float(lim[i])) for i in bad[:4]]

    bad = per_label(_y_err(su, got["y"], want["y"]) / scale, tol_y,
                    None if own is None else _y_err(su, own[0]["y"], own[1]["y"]) / scale, "y")
    for key in ("E", "D"):
        if want[key] is None:
            continue
        w = _rows(want[key]) if key == "D" else want[key].double().view(-1, 1)
        s = w.abs().amax(1)
        s = s.clamp(min=1e-3 * float(s.max())) if key == "D" else s.clamp(min=1.0)
        err = (_rows(got[key]) if key == "D" else got[key].cpu().double().view(-1, 1)).sub(w).abs().amax(1) / s
        own_err = None
        if own is not None:
            ow = _rows(own[1][key])
            os_ = ow.abs().amax(1)
            own_err = (_rows(own[0][key]) - ow).abs().amax(1) / os_.clamp(min=1e-3 * float(os_.max()))
        bad += per_label(err, tol_y if key == "E" else tol_d, own_err, key)
    for i, (p, w) in enumerate(zip(got["gp"], want["gp"])):
        s = max(1e-6, float(w.abs().max()))
        e = float((p.cpu().double() - w).abs().max()) / s
        lim = tol_d if own is None else max(tol_d, 2.0 * float((own[0]["gp"][i].double() - own[1]["gp"][i]).abs().max()) / s)
        ratios["param %d" % i] = e / lim
        if not e <= lim:
            bad.append(("param %d" % i, e, lim))
    assert len(got["gp"]) == len(want["gp"])
    assert not bad, (what, regime, bad)
    return ratios


def _theta_sup(su, x_rows, loss, col):
    """Behind a head: the largest |d loss / d theta| [rows] over theta within 1.5e-3 rad of the true angle, in float64."""
    xr = x_rows.detach().cpu().double()
    with torch.no_grad():
        f = mo.preprocessing_forward(xr, su.items, su.uav, su.align, su.ref)
    a = [xr[:, i].numpy() for i in su.items[ae.roles(su.items)["angle"]][1]]
    f[:, col] = torch.from_numpy(ae._angle(*a))
    sup = torch.zeros(len(xr), dtype=torch.float64)
    for off in np.linspace(-1.5e-3, 1.5e-3, 7):
        f2 = f.clone()
        f2[:, col] += float(off)
        f2.requires_grad_(True)
        (g,) = torch.autograd.grad(loss(su.head(f2)).sum(), f2)
        sup = torch.maximum(sup, g[:, col].abs())
    return sup


def _check_invariant(su, x, rows, got, extra, what):
    """The angle-value gradient on pole frames: non-finite rows or rows within (1 + 1e-3) of their exact length."""
    t, idx = su.items[ae.roles(su.items)["angle"]]
    col, end = su.cols["angle"], idx[2]
    xr = x[rows].detach().cpu().double()
    u, v = xr[:, idx[0]] - xr[:, idx[1]], xr[:, idx[2]] - xr[:, idx[1]]
    lu, lv = u.norm(dim=1), v.norm(dim=1)
    slack = 1.0 + 1e-3
    D = got["D"][rows].detach().cpu().double()
    if su.mode in ("jvp32", "jvp64"):
        T = torch.stack([e[rows].detach().cpu().double() for e in extra], 1)          # [rows, T, n, 3]
        lim = slack * ((T[:, :, idx[0]] - T[:, :, idx[1]]).norm(dim=2) / lu[:, None] + (T[:, :, idx[2]] - T[:, :, idx[1]]).norm(dim=2) / lv[:, None])
        val = D[:, :, col].abs()
    elif su.mode == "metric":
        lim = slack ** 2 * (1.0 / lu ** 2 + 1.0 / lv ** 2 + (1.0 / lu + 1.0 / lv) ** 2)
        val = D[:, col, col].abs()
    else:
        if su.mode == "jac":
            s = torch.stack([_theta_sup(su, x[rows], lambda y, k=k: y[:, k], col) for k in range(su.d_out)], 1)    # [rows, d_out]
            val = D[:, :, end].norm(dim=2)
        else:
            val = D[:, end].norm(dim=1)
            if su.mode in ("restraint", "hills"):
                y = got["y"][rows].detach().cpu().double().requires_grad_(True)
                (gy,) = torch.autograd.grad(_bias(su, y, tuple(e[rows] if e.shape[:1] == x.shape[:1] else e for e in extra)).sum(), y)
                s = gy[:, col].abs()
            elif su.head is None:
                s = extra[rows][:, col].detach().cpu().double().abs()
            else:
                G = extra[rows].detach().cpu().double()
                s = _theta_sup(su, x[rows], lambda y: (y * G).sum(1), col)
        lim = slack * s / (lv[:, None] if val.dim() == 2 else lv)
    finite = torch.isfinite(val)
    bad = (finite & ~(val <= lim)).nonzero().tolist()
    print("angular edges %s pole frames: %d of %d gradient entries finite, largest finite / limit %.4g" % (
        what, int(finite.sum()), finite.numel(), float((val / lim)[finite].max()) if bool(finite.any()) else 0.0))
    assert not bad, (what, "a finite angle-value gradient beyond its bound", [(b, float(val[tuple(b)]), float(lim[tuple(b)])) for b in bad[:6]])


def _check_pole(su, regime, x, labels, got, graded, extra, what):
    near = [i for i, l in enumerate(labels) if l is None]
    pole = [i for i, l in enumerate(labels) if l is not None]
    keys = ("y",) if su.family in ATOMICS else ("y", "D", "E")
    for k in keys:
        if got[k] is not None:
            assert bool(torch.isfinite(got[k][near]).all()), (what, regime, k, "a near row is not finite")
            fft._same_rows(got[k].reshape(len(labels), -1), graded[k].reshape(len(labels), -1), near,
                           what + (regime, "near rows next to pole frames", k))
    if not su.uav and (regime != "arm" or su.head is None):
        with torch.no_grad():
            f = mo.preprocessing_forward(x[pole].detach().cpu().double(), su.items, su.uav, su.align, su.ref)
            y_want = su.head(f) if su.head is not None else f
            f32 = mo.preprocessing_forward(x[pole].detach().cpu().float(), su.items, su.uav, su.align, su.ref.float())
            y_own = (copy.deepcopy(su.head).float()(f32) if su.head is not None else f32).double()
        keep = torch.ones(y_want.shape[1], dtype=torch.bool)
        if regime == "arm":
            keep[su.cols["arm"]:su.cols["arm"] + 2] = False
        scale = max(1.0, float(y_want[:, keep].abs().max()))
        err = (got["y"][pole].cpu().double() - y_want)[:, keep].abs().amax(1) / scale
        lim = 1e-10 if su.f64 else max(1e-5, 2.0 * float((y_own - y_want)[:, keep].abs().max()) / scale)
        print("angular edges %s %s pole frames y: error/bound %.3g" % (what, regime, float(err.max()) / lim))
        assert float(err.max()) <= lim, (what, regime, "pole frames y", float(err.max()), lim)
    if su.uav and regime in ("straight", "folded") and su.mode != "fwd":
        _check_invariant(su, x, pole, got, extra, what + (regime,))


@pytest.mark.parametrize("uav", [False, True], ids=["cos", "value"])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_angular_edges(family, uav, hip_device, monkeypatch):
    for k, v in FAMILIES[family][2].items():
        monkeypatch.setenv(k, v)
    su = Setup(family, uav, hip_device)
    what = (family, "value" if uav else "cos")
    for r, regime in enumerate(ae.REGIMES):
        graded, pole = ae.grades(regime)
        xb, labels, _ = _batch(su.spec, regime, graded, su.n, 40 + r)
        x = torch.from_numpy(xb).to(hip_device, su.dtype)
        extra = _extra(su, x, regime, seed=7 + r)
        got = _run(su, x, extra)
        RATIOS[what + (regime,)] = _check_graded(su, regime, x, labels, got, extra, what)
        if pole:
            xp, plabels, _ = _batch(su.spec, regime, pole, su.n, 40 + r)
            xp = torch.from_numpy(xp).to(hip_device, su.dtype)
            _check_pole(su, regime, xp, plabels, _run(su, xp, extra), got, extra, what)
    seen = " | ".join(su.infos)
    missing = [p for p in su.fwd_pats if not re.search(p, seen)]
    assert not missing, (family, missing, seen)
    REACHED.add((family, uav))


# ---- second order: frames_hvp_kernel on trans / cis with the cosine forms ------------------------------------------------------
@pytest.mark.parametrize("spec", ["ala_pos", "c166"])
def test_second_order_at_cis_and_trans(spec, hip_device):
    xyz, align, items = _spec(spec)
    ref = mo.center_reference(torch.from_numpy(np.ascontiguousarray(xyz, np.float32)[align])).float()
    with torch.cuda.device(hip_device):
        plan = _capi.Plan(len(xyz), align_idx=align, ref_x=ref, features=items, use_angle_value=False)
        plan.update_ref_f64(ref.double().to(hip_device).contiguous())
        torch.cuda.synchronize()
    gen = torch.Generator().manual_seed(13)
    for r, regime in enumerate(("trans", "cis")):
        xb, labels, _ = ae.interleaved(regime, ae.grades(regime)[0], xyz, items, 192, seed=60 + r, align=align)
        x = torch.from_numpy(xb).double()
        g = torch.randn(len(x), plan.feature_dim, generator=gen, dtype=torch.float64)
        u = torch.randn(x.shape, generator=gen, dtype=torch.float64)
        xx = x.clone().requires_grad_(True)
        (gx,) = torch.autograd.grad((mo.preprocessing_forward(xx, items, False, align, ref.double()) * g).sum(), xx, create_graph=True)
        (want,) = torch.autograd.grad((gx * u).sum(), xx)
        xd = x.to(hip_device)
        hx, hg = torch.full_like(xd, float("nan")), torch.full((len(x), plan.feature_dim), float("nan"), dtype=torch.float64, device=hip_device)
        with torch.cuda.device(hip_device):
            plan.features_hvp_f64(xd, g.to(hip_device), u.to(hip_device), hx, hg)
        torch.cuda.synchronize()
        assert plan.last_launch_info().startswith("frames_hvp_f64_kernel"), plan.last_launch_info()
        assert torch.equal(xd.cpu(), x)
        err = float((hx.cpu() - want).abs().max()) / float(want.abs().max())
        print("angular edges hvp %s %s: error %.3g of the batch's scale" % (spec, regime, err))
        assert bool(torch.isfinite(hx).all()) and bool(torch.isfinite(hg).all()) and err <= 1e-12, (spec, regime, err)
    REACHED.add(("hvp", spec))


def test_every_angular_edge_family_was_reached(request):
    """The families are recorded as they pass, so this guard needs all of them in the same session."""
    here = {item.name for item in request.session.items if item.module is request.module}
    wanted = {"test_angular_edges[%s-%s]" % (f, u) for f in FAMILIES for u in ("cos", "value")} | \
             {"test_second_order_at_cis_and_trans[%s]" % s for s in ("ala_pos", "c166")}
    if not wanted <= here:
        pytest.skip("the coverage guard needs every family in this session: %d not selected" % len(wanted - here))
    missing = sorted(({(f, u) for f in FAMILIES for u in (False, True)} | {("hvp", "ala_pos"), ("hvp", "c166")}) - REACHED, key=str)
    assert not missing, ("not reached:", missing)
    for key in sorted(RATIOS, key=str):
        print("angular edges ratios", key, " ".join("%s=%.3g" % kv for kv in RATIOS[key].items()))
