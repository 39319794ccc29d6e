"""Gradients of large-frame plans (n_inp > 85: the wave-per-frame backward family) against torch autograd through the float64
oracle, over the plan space launch_wave_bwd and molann_backward_f32 (molann_amd/csrc/molann_capi.inc) accept rather than the
handful of specs the kernels were developed on:

A. random plans: frame sizes on both sides of the group kernel's 1024-atom limit, permuted input groups, items of all four
   types biased to the frame's ends, to the alignment set and to each other, alignment sets of 3 to 300 atoms (sometimes naming
   an atom twice), centred and shifted references, small heads with every activation the head backward implements, the
   AlignmentLayer alone;
B. every dispatch boundary of launch_wave_bwd, each case naming the kernel it must reach;
C. the chunk loops of molann_backward_f32 over its backward workspace, with n past one chunk;
D. the plans of A and B as model.double() (frames_bwd_f64_kernel);
E. a guard that every backward family above was reached.

The cotangent G is nonzero on a few frames only (the first, the last and some in between): the oracle runs on those frames
and still gives the exact parameter gradients, and every other row of dL/dx must be exactly zero, so a kernel that writes a
frame's gradient into another frame's row, or not at all, fails."""

import copy
import re

import numpy as np
import pytest
import torch

from molann_amd import workloads as wl
from molann_amd.ann import AlignmentLayer, FeatureLayer, MolANN, PreprocessingANN, _PlanEntry, create_sequential_nn
from molann_amd.atomgroup import Universe
from molann_amd.feature import Feature
from oracle import molann_oracle as mo

pytestmark = pytest.mark.gpu
ANGLE, BOND, DIH, POS = wl.ANGLE, wl.BOND, wl.DIHEDRAL, wl.POSITION
NEED = {ANGLE: 3, BOND: 2, DIH: 4}
ACTS = {"tanh": torch.nn.Tanh, "relu": torch.nn.ReLU, "sigmoid": torch.nn.Sigmoid, "identity": torch.nn.Identity,
        "silu": torch.nn.SiLU, "leaky_relu": torch.nn.LeakyReLU}
BATCHES = (1, 37, 300, 2111)
FAMILIES = ("frames_group_bwd_kernel<B=8>", "frames_group_bwd_kernel<B=4>", "frames_group_bwd_kernel<B=2>",
            "frames_wave_bwd_gather_kernel", "frames_wave_bwd_kernel", "frames_align_bwd_regs_kernel", "molann_mlp_bwd")
REACHED = set()                                            # backward families seen by A to C (E checks it)


def _note(info):
    for f in FAMILIES:
        if f in info:
            REACHED.add(f)


class Case(object):
    """A model on an input group of n_inp atoms: local (0-based, input-group) indices throughout."""

    def __init__(self, name, xyz, feats=(), align=None, uav=False, mlp=None, act="tanh", align_only=False, shift=None,
                 universe=None, inp=None):
        xyz = np.ascontiguousarray(xyz, dtype=np.float32)
        self.name, self.xyz, self.feats, self.align, self.uav = name, xyz, list(feats), align, uav
        self.mlp, self.act, self.align_only, self.shift = mlp, act, align_only, shift
        self.universe = xyz if universe is None else universe   # the input group is inp (a permuted subset) of the universe
        self.inp = list(range(len(xyz))) if inp is None else list(inp)

    def __repr__(self):
        return "%s(n_inp=%d, items=%d, align=%s, uav=%s, mlp=%s %s, align_only=%s, shift=%s)" % (
            self.name, len(self.xyz), self.n_items(), None if self.align is None else len(self.align), self.uav, self.mlp,
            self.act, self.align_only, self.shift)

    def n_items(self):
        return sum(len(idx) if t == POS else 1 for t, idx in self.feats)

    def d_feat(self):
        return sum(mo.feature_dim(t, len(idx), self.uav) for t, idx in self.feats)

    def touched(self):
        return set(self.align or ()) | {a for _, idx in self.feats for a in idx}

    def build(self, dev):
        u = Universe(self.universe)
        num = lambda local: u.atoms_by_number([self.inp[a] + 1 for a in local])
        inp_ag = num(range(len(self.inp)))
        al = AlignmentLayer(num(self.align), inp_ag) if self.align is not None else None
        if self.align_only:
            m = al
        else:
            fl = FeatureLayer([Feature("f%d" % i, wl.TYPE_NAMES[t], num(idx)) for i, (t, idx) in enumerate(self.feats)],
                              inp_ag, self.uav)
            m = PreprocessingANN(al, fl)
            if self.mlp:
                torch.manual_seed(len(self.xyz) + len(self.feats))
                m = MolANN(m, create_sequential_nn(self.mlp, activation=ACTS[self.act]()))
        m = m.to(dev)
        if al is not None:
            assert al._local_align_atom_indices == list(self.align)
            if self.shift is not None:                     # the reference state assigned after __init__, uncentred
                with torch.no_grad():
                    al.ref_x.copy_(al.ref_x + torch.tensor(self.shift, device=dev))
        return m

    def frames(self, n, seed, dev):
        """Frames on the device: the input group's coordinates + noise, rigidly moved."""
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        ref = torch.from_numpy(self.xyz).to(dev)
        x = ref.unsqueeze(0) + 0.2 * torch.randn((n,) + tuple(ref.shape), generator=g, device=dev)
        q = torch.randn((n, 4), generator=g, device=dev)
        rot = wl.quaternion_to_matrix(q / q.norm(dim=1, keepdim=True))
        return (torch.matmul(x, rot) + 3.0 * torch.randn((n, 1, 3), generator=g, device=dev)).contiguous()

    def well_conditioned(self):
        """The derivative of the Kabsch rotation divides by s_i + s_j (the covariance's singular values; s_2 - s_3 for a
        reflection): a nearly collinear alignment set (s_2 << s_1) makes it ill-conditioned.  A planar one (s_3 = 0, every
        3-atom set) does not."""
        if self.align is None:
            return True
        r = self.xyz[self.align].astype(np.float64)
        r = r - r.mean(0)
        sv = np.linalg.svd(r.T @ r, compute_uv=False)
        return sv[1] / sv[0] >= 0.05


def _align_layer(model):
    if isinstance(model, AlignmentLayer):
        return model
    pp = model.preprocessing_layer if isinstance(model, MolANN) else model
    return pp.align_layer if isinstance(pp.align_layer, AlignmentLayer) else None


def _infos(model):
    """Launch info of every plan the module and its submodules hold, and of the model's own operator plan."""
    infos = [e.plan.last_launch_info() for m in model.modules() if hasattr(m, "_plans")
             for e in m._plans().values() if isinstance(e, _PlanEntry)]
    if isinstance(model, MolANN):
        infos.append(model.last_launch_info())
    return " | ".join(infos)


def _out_dim(case, model):
    return case.mlp[-1] if case.mlp else (model.input_atom_num * 3 if case.align_only else case.d_feat())


def _select(n, rng):
    """The frames the cotangent is nonzero on: all of a small batch, else the first and last four and eight in between."""
    if n <= 40:
        return list(range(n))
    mid = rng.choice(np.arange(4, n - 4), size=8, replace=False).tolist()
    return sorted(set(range(4)) | set(range(n - 4, n)) | set(mid))


def _head64(model):
    return copy.deepcopy(model.ann_layers).cpu().double()


def _dihedral_poles(x, feats):
    """Per frame: a dihedral with a bond angle within about three degrees of 0 or 180 (sin < 0.05), where its gradient is
    ill-conditioned in float32."""
    bad = torch.zeros(x.shape[0], dtype=torch.bool, device=x.device)
    for t, idx in feats:
        if t == DIH:
            for a, b, c in (idx[:3], idx[1:]):
                u, v = x[:, a] - x[:, b], x[:, c] - x[:, b]
                bad |= torch.linalg.cross(u, v).norm(dim=1) < 0.05 * u.norm(dim=1) * v.norm(dim=1)
    return bad


def _kinked(case, model, xs, ref):
    """Per selected frame: some pre-activation of a ReLU / LeakyReLU head within 1e-4 of the kink, or a dihedral pole."""
    poles = _dihedral_poles(xs.detach().cpu().double(), case.feats)
    if not case.mlp or case.act not in ("relu", "leaky_relu"):
        return poles
    with torch.no_grad():
        h = mo.preprocessing_forward(xs.cpu().double(), case.feats, case.uav, case.align, ref)
        bad = torch.zeros(h.shape[0], dtype=torch.bool)
        for m in _head64(model):
            h = m(h)
            if isinstance(m, torch.nn.Linear):
                bad |= (h.abs() < 1e-4).any(dim=1)
    return bad | poles


def _oracle(case, model, xs, Gs, ref):
    """y, dL/dx and dL/d(parameters) of L = sum(y * G) on the selected frames, float64 autograd through the oracle."""
    xx = xs.detach().cpu().double().requires_grad_(True)
    prm = []
    if case.align_only:
        y = mo.align_forward(xx, case.align, ref)
    else:
        y = mo.preprocessing_forward(xx, case.feats, case.uav, case.align, ref)
        if case.mlp:
            head = _head64(model)
            prm = list(head.parameters())
            y = head(y)
    (y * Gs.cpu().double()).sum().backward()
    return y.detach(), xx.grad, [p.grad for p in prm]


def _cotangent(case, model, x, ref, n, seed):
    """(G on the device, selected frames, their cotangent rows): nonzero rows only on selected frames away from a kink."""
    rng = np.random.default_rng(seed)
    sel = _select(n, rng)
    d = _out_dim(case, model)
    Gs = torch.from_numpy(rng.standard_normal((len(sel), d))).float()
    Gs[_kinked(case, model, x[sel], ref)] = 0.0
    G = torch.zeros((n, d), device=x.device)
    G[sel] = Gs.to(x.device)
    if case.align_only:
        G = G.view(n, -1, 3)
        Gs = Gs.view(len(sel), -1, 3)
    return G, sel, Gs


def _run(model, x, G):
    """(y, dL/dx, parameter gradients, launch info) of the module under autograd; x is never written."""
    x0 = x.clone()
    xg = x.clone().requires_grad_(True)
    for p in model.parameters():
        p.grad = None
    y = model(xg)
    (y * G).sum().backward()
    torch.cuda.synchronize()
    assert torch.equal(xg.detach(), x0)
    return y.detach(), xg.grad, [p.grad.clone() for p in model.parameters()], _infos(model)


def _err(got, want):
    return float((got.detach().cpu().double() - want).abs().max())


def _check(case, what, y, gx, gp, sel, want, out_tol, grad_tol, untouched):
    """Outputs and gradients of the selected frames against the oracle; every other row of dL/dx exactly zero."""
    y_want, gx_want, gp_want = want
    e = _err(y[sel], y_want)
    assert e <= out_tol * max(1.0, float(y_want.abs().max())), (case, what, "y", e)
    s = max(1e-6, float(gx_want.abs().max()))
    e = _err(gx[sel], gx_want)
    assert e <= grad_tol * s, (case, what, "x.grad", e, s)
    worst = e / (grad_tol * s)
    assert len(gp) == len(gp_want), (case, what, len(gp), len(gp_want))
    for i, (p, w) in enumerate(zip(gp, gp_want)):
        s = max(1e-6, float(w.abs().max()))
        e = _err(p, w)
        assert e <= grad_tol * s, (case, what, "param %d" % i, e, s)
        worst = max(worst, e / (grad_tol * s))
    rest = torch.ones(gx.shape[0], dtype=torch.bool, device=gx.device)
    rest[sel] = False
    if bool(rest.any()):
        assert float(gx[rest].abs().max()) == 0.0, (case, what, "rows of frames with a zero cotangent")
    if untouched:
        assert float(gx[:, untouched].abs().max()) == 0.0, (case, what, "untouched atoms")
    return worst


def _out_tol(case):
    # position items behind a small alignment set: the fit's fp32 rounding reaches the outputs amplified
    small_fit = case.align is not None and len(set(case.align)) <= 8
    return 1e-4 if (small_fit and (case.align_only or any(t == POS for t, _ in case.feats))) else 2e-5


def _check_case(case, dev, batches, bwd_name=None, f64=True, seed=0):
    """A, B and D for one plan: float32 (and float64) runs at each batch size against the oracle.  Returns the number of
    batches checked (ill-conditioned frames at angle / dihedral poles skip a batch)."""
    model = case.build(dev)
    al = _align_layer(model)
    ref = al.ref_x.detach().cpu().double() if al is not None else None
    model64 = copy.deepcopy(model).double() if f64 else None
    untouched = [] if case.align_only else sorted(set(range(len(case.xyz))) - case.touched())
    checked = 0
    for n in batches:
        x = case.frames(n, seed=1000 * seed + n, dev=dev)
        G, sel, Gs = _cotangent(case, model, x, ref, n, seed=7 * seed + n)
        want = _oracle(case, model, x[sel], Gs, ref)
        if not torch.isfinite(want[1]).all() or float(want[1].abs().max()) > 1e4:
            continue                                       # a frame at an angle / dihedral pole (use_angle_value)
        y, gx, gp, info = _run(model, x, G)
        if bwd_name is not None:
            assert bwd_name in info, (case, n, info)
        _note(info)
        _check(case, ("f32", n, info), y, gx, gp, sel, want, _out_tol(case), 2e-4, untouched)
        plan = model.plan_for(x) if case.mlp else None
        # the same plan through molann_backward_f32 (the large-frame loop).  A plan touching <= 32 atoms whose lane kernel fuses
        # the head has no HIP head backward: its model trains through the torch head, checked above.
        if plan is not None and plan.supports_backward():
            gx2 = torch.full_like(x, float("nan"))
            gp2 = torch.zeros(plan.grad_params_size(), device=dev)
            with torch.cuda.device(dev):
                plan.backward(x, G, gx2, gp2)
            torch.cuda.synchronize()
            info2 = plan.last_launch_info()
            assert "molann_mlp_bwd" in info2, info2
            if bwd_name is not None:
                assert bwd_name in info2, (case, n, info2)
            _note(info2)
            _check(case, ("plan.backward", n, info2), y, gx2, _unflatten(gp2, gp), sel, want, _out_tol(case), 2e-4, untouched)
        if f64:
            y64, gx64, gp64, info64 = _run(model64, x.double(), G.double())
            assert "frames_bwd_f64_kernel" in info64, (case, n, info64)
            _check(case, ("f64", n), y64, gx64, gp64, sel, want, 1e-9, 1e-9, untouched)
        checked += 1
    return checked


def _unflatten(flat, like):
    """molann_backward_f32's parameter gradients (dW_l then db_l, layer after layer) in model.parameters() order."""
    out, off, nl = [], 0, len(like) // 2
    ws, bs = [], []
    for l in range(nl):
        nw, nb = like[2 * l].numel(), like[2 * l + 1].numel()
        ws.append(flat[off:off + nw].view(like[2 * l].shape))
        bs.append(flat[off + nw:off + nw + nb].view(like[2 * l + 1].shape))
        off += nw + nb
    assert off == flat.numel()
    for w, b in zip(ws, bs):
        out += [w, b]
    return out


# ---- A. random large-frame plans -----------------------------------------------------------------------------------------
def _chain(n, seed):
    return wl.synthetic_chain(n_atoms=n, step=1.4, seed=seed)


def _pick(rng, n_inp, k, weights):
    p = weights / weights.sum()
    return rng.choice(n_inp, size=k, replace=False, p=p).tolist()


SIZES = (86, 1025, 166, 5000, 120, 1024, 333, 2500, 1000)   # one draw per frame size
ALIGNS = (0, 3, 5, 8, 40, 300)                               # alignment set sizes, by seed
HEADS = (0, 1, 3, 4, 6, 7)                                   # the draws with a head: one per activation, in sorted(ACTS) order
DUPS = (3, 7)                                                # the draws whose alignment set names an atom twice
ALIGN_ONLY = 8


def _draw(seed):
    """Plan `seed` of the sweep.  The frame size, alignment set size, head, activation, duplicated alignment atom and
    use_angle_value are fixed by the seed so that the sweep covers each of them; the atoms and items are drawn."""
    rng = np.random.default_rng(9000 + seed)
    n_inp = SIZES[seed]
    if rng.random() < 0.35:                                # a permuted subset of a larger universe
        n_u = n_inp + int(rng.integers(1, 60))
        universe = _chain(n_u, seed) if rng.random() < 0.5 else np.cumsum(rng.normal(size=(n_u, 3)) * 0.9, axis=0).astype(np.float32)
        inp = rng.permutation(n_u)[:n_inp].tolist()
    else:
        universe = _chain(n_inp, seed) if rng.random() < 0.5 else np.cumsum(rng.normal(size=(n_inp, 3)) * 0.9, axis=0).astype(np.float32)
        inp = list(range(n_inp))
    xyz = np.ascontiguousarray(universe[inp])
    k_align = min(ALIGNS[seed % len(ALIGNS)], n_inp // 2)
    align = sorted(rng.choice(n_inp, size=int(k_align), replace=False).tolist()) if k_align else None
    if align is not None and seed in DUPS:                 # an alignment set that names an atom twice
        align = align + [align[int(rng.integers(0, len(align)))]]
    uav = bool(seed % 2)
    if seed == ALIGN_ONLY:
        return Case("A%d" % seed, xyz, align=align, align_only=True, universe=universe, inp=inp,
                    shift=tuple(rng.normal(size=3) * 3.0))
    head = seed in HEADS
    # bias: the frame's first and last atoms, the alignment set, atoms already used by an item
    w = np.ones(n_inp)
    w[:3] += 0.02 * n_inp
    w[-3:] += 0.02 * n_inp
    if align is not None:
        w[align] += 0.005 * n_inp
    feats = [(POS, [n_inp - 1, 0])]
    used = [0, n_inp - 1]
    budget = 32 if head else None                          # a head within the fused MLP's limits: d <= 32
    n_feat = int(rng.choice([4, 12, 40, 150]))
    for _ in range(n_feat):
        # (with a head, mostly one-column items: a head plan touching <= 32 atoms is a lane plan whose head is torch's to train)
        t = int(rng.choice([ANGLE, ANGLE, ANGLE, BOND, DIH, POS] if head else [ANGLE, BOND, DIH, POS]))
        k = NEED[t] if t != POS else int(rng.integers(1, 5))
        atoms = _pick(rng, n_inp, k, w)
        if rng.random() < 0.3:                             # share an atom with an earlier item
            a = used[int(rng.integers(0, len(used)))]
            if a not in atoms:
                atoms[int(rng.integers(0, k))] = a
        cand = feats + [(t, atoms)]
        if budget is not None and sum(mo.feature_dim(tt, len(ii), uav) for tt, ii in cand) > budget:
            continue
        feats = cand
        used += atoms
    mlp, act = None, "tanh"
    if head:
        d = sum(mo.feature_dim(t, len(i), uav) for t, i in feats)
        mlp = [d, int(rng.integers(2, 33)), int(rng.integers(1, 9))]
        act = sorted(ACTS)[HEADS.index(seed)]
    shift = tuple(rng.normal(size=3) * 3.0) if (align is not None and rng.random() < 0.5) else None
    return Case("A%d" % seed, xyz, feats, align, uav, mlp, act, shift=shift, universe=universe, inp=inp)


def test_random_large_frame_backward_plans(hip_device):
    """Nine drawn plans at four batch sizes each.  A sweep whose filters drop (nearly) everything checks nothing: at least
    six plans and 20 batches must have been checked."""
    checked = []
    for seed in range(len(SIZES)):
        case = _draw(seed)
        checked.append(_check_case(case, hip_device, BATCHES, seed=seed) if case.well_conditioned() else 0)
    assert sum(1 for c in checked if c) >= 6 and sum(checked) >= 20, checked


# ---- B. dispatch boundaries of launch_wave_bwd ---------------------------------------------------------------------------
def _mixed(n_inp, n_items, seed, align=(), uav=False):
    """n_items items: angles, bonds and dihedrals on both ends of the frame and on alignment atoms, the rest single- and
    multi-atom positions; items share atoms."""
    rng = np.random.default_rng(seed)
    al = list(align)
    feats = [(DIH, [0, 1, 2, 3]), (ANGLE, [n_inp - 1, n_inp - 2, n_inp - 3]), (BOND, [n_inp - 1, 0])]
    if len(al) >= 4:
        feats += [(DIH, al[:4]), (ANGLE, [al[1], n_inp - 1, al[2]])]
    while len(feats) < min(12, n_items):
        t = int(rng.choice([ANGLE, BOND, DIH]))
        feats.append((t, sorted(rng.choice(n_inp, size=NEED[t], replace=False).tolist())))
    w = np.ones(n_inp)
    w[al] += 3.0
    w[[0, n_inp - 1]] += 8.0
    left = n_items - len(feats)
    while left > 0:
        k = min(left, int(rng.integers(1, 5)))
        feats.append((POS, _pick(rng, n_inp, k, w)))
        left -= k
    c = Case("mixed", np.zeros((n_inp, 3), np.float32), feats, uav=uav)
    assert c.n_items() == n_items
    return feats


def _boundary(name):
    """(case, backward kernel it must reach)."""
    x166 = _chain(166, 11)
    a166 = list(range(2, 166, 7))                          # 24 atoms
    if name == "items1400":                                # per_wave > 64 KiB: the atomics kernel without an environment switch
        al = list(range(3, 1500, 37))
        return Case(name, _chain(1500, 6), _mixed(1500, 1400, 6, al), al, shift=(3.0, 0.0, -1.0)), "frames_wave_bwd_kernel"
    if name.startswith("items"):                           # 166 atoms with an alignment: B = 8 / 4 / 2 / gather by n_items
        k = int(name[5:])
        want = {32: "<B=8>", 33: "<B=4>", 64: "<B=4>", 65: "<B=2>", 128: "<B=2>", 129: "gather"}[k]
        if k == 32:                                        # 32 one-column items: d = 32 takes a head too
            feats = [(BOND, [i, i + 3]) for i in range(0, 160, 10)] + [(ANGLE, [i, i + 1, i + 5]) for i in range(3, 160, 10)]
            case = Case(name, x166, feats, a166, True, mlp=[32, 24, 3], act="silu", shift=(2.0, -3.0, 4.0))
        else:
            case = Case(name, x166, _mixed(166, k, k, a166), a166, shift=(2.0, -3.0, 4.0) if k % 2 else None)
        return case, ("frames_wave_bwd_gather_kernel" if want == "gather" else "frames_group_bwd_kernel" + want)
    if name in ("n1024", "n1025"):                         # the group kernel's frame-size limit
        n = int(name[1:])
        al = list(range(5, n, 41))
        return (Case(name, _chain(n, 4), _mixed(n, 40, 3, al), al, shift=(-4.0, 1.0, 2.5)),
                "frames_group_bwd_kernel<B=4>" if n == 1024 else "frames_wave_bwd_gather_kernel")
    if name == "align1000_n1024":                          # the LDS tables of a 1000-atom fit overflow 64 KB
        rng = np.random.default_rng(1)
        al = sorted(rng.choice(1024, size=1000, replace=False).tolist())
        return Case(name, _chain(1024, 8), _mixed(1024, 40, 5, al), al, shift=(1.0, 1.0, -2.0)), "frames_wave_bwd_gather_kernel"
    if name == "dup_align_features":                       # an alignment set naming an atom twice: no bw tables
        al = list(range(4, 300, 15)) + [64]
        return Case(name, _chain(300, 9), _mixed(300, 30, 9, al), al, True, shift=(-2.0, 2.0, 2.0)), "frames_wave_bwd_kernel"
    if name == "dup_align_only":
        al = list(range(4, 300, 15)) + [4]
        return Case(name, _chain(300, 9), align=al, align_only=True, shift=(-2.0, 2.0, 2.0)), "frames_wave_bwd_kernel"
    if name == "align_only_regs":
        al = list(range(1, 700, 9))
        return Case(name, _chain(700, 2), align=al, align_only=True, shift=(5.0, -1.0, 0.5)), "frames_align_bwd_regs_kernel"
    if name == "no_align_400":                             # mid-size frames without an alignment skip the group kernel
        return Case(name, _chain(400, 12), _mixed(400, 60, 12), None, True), "frames_wave_bwd_gather_kernel"
    raise KeyError(name)


BOUNDARIES = ["items32", "items33", "items64", "items65", "items128", "items129", "n1024", "n1025", "align1000_n1024",
              "items1400", "dup_align_features", "dup_align_only", "align_only_regs", "no_align_400"]


@pytest.mark.parametrize("name", BOUNDARIES)
def test_backward_dispatch_boundaries(name, hip_device):
    case, bwd = _boundary(name)
    assert case.well_conditioned(), case
    assert _check_case(case, hip_device, BATCHES, bwd_name=bwd, seed=len(name)) >= 3, case


# ---- C. chunk boundaries of molann_backward_f32's workspace ----------------------------------------------------------------
def _bwork_frames(d_feat):
    # ensure_bwork in molann_amd/csrc/molann_capi.inc: the frames of one chunk of the backward workspace
    return max(4096, min(1 << 20, (64 << 20) // (4 * d_feat)) & ~63)


def _chunk_case(name):
    if name == "large_head":                               # wave-per-frame features (d = 32) -> molann_mlp_bwd -> wave backward
        al = list(range(0, 90, 7))                         # 13 atoms; 41 touched in all, so not a lane plan
        feats = [(POS, [0, 89, 15, 45, 46, 71, 88, 8]), (BOND, [2, 3]), (BOND, [86, 87]), (BOND, [16, 60]), (BOND, [9, 47]),
                 (ANGLE, [80, 81, 82]), (ANGLE, [4, 5, 6]), (ANGLE, [36, 37, 38]), (ANGLE, [22, 23, 24])]
        return Case(name, _chain(90, 21), feats, al, False, mlp=[32, 16, 4], act="tanh", shift=(2.0, 2.0, -3.0)), "frames_group_bwd_kernel<B=8>"
    if name == "C3_no_ring":                               # lane plan, no one-pass kernel: features -> MLP backward -> lane backward
        w = wl.get_workload("C3")
        return Case(name, w.ref_xyz, [(t, [a - 1 for a in atoms]) for t, atoms in w.features], [a - 1 for a in w.align],
                    w.use_angle_value, mlp=list(w.mlp_dims), act="tanh", shift=(1.0, -2.0, 3.0)), "molann_lane_bwd"
    raise KeyError(name)


@pytest.mark.parametrize("name", ["large_head", "C3_no_ring"])
def test_backward_workspace_chunks(name, hip_device, monkeypatch):
    if name == "C3_no_ring":
        monkeypatch.setenv("MOLANN_NO_RING_BWD", "1")
    case, third = _chunk_case(name)
    model = case.build(hip_device)
    # the plan's chunk size, from the launch info of a one-frame backward; it must match the formula
    x1 = case.frames(1, seed=30, dev=hip_device)
    plan = model.plan_for(x1)
    with torch.cuda.device(hip_device):
        plan.backward(x1, torch.ones((1, case.mlp[-1]), device=hip_device), torch.empty_like(x1), None)
    torch.cuda.synchronize()
    m = re.search(r"chunks of (\d+) frames", plan.last_launch_info())
    assert m, plan.last_launch_info()
    bf = int(m.group(1))
    assert bf == _bwork_frames(case.d_feat()), (bf, case.d_feat())
    n = bf + 1000
    x = case.frames(n, seed=31, dev=hip_device)
    sel = list(range(8)) + list(range(bf - 8, bf + 8)) + list(range(n - 8, n))
    rng = np.random.default_rng(5)
    Gs = torch.from_numpy(rng.standard_normal((len(sel), case.mlp[-1]))).float()
    G = torch.zeros((n, case.mlp[-1]), device=hip_device)
    G[sel] = Gs.to(hip_device)
    x0 = x.clone()
    gx = torch.full_like(x, float("nan"))                  # rows left unwritten stay NaN (and fail the zero check)
    gp = torch.zeros(plan.grad_params_size(), device=hip_device)
    with torch.cuda.device(hip_device):
        plan.backward(x, G, gx, gp)
    torch.cuda.synchronize()
    info = plan.last_launch_info()
    assert "molann_mlp_bwd" in info and third in info.split(" || ")[2] and ("chunks of %d frames" % bf) in info, info
    _note(info)
    assert torch.equal(x, x0)
    ref = _align_layer(model).ref_x.detach().cpu().double()
    want = _oracle(case, model, x[sel], Gs, ref)
    gp_list = _unflatten(gp, list(model.parameters()))
    untouched = sorted(set(range(len(case.xyz))) - case.touched())
    y = torch.zeros((n, case.mlp[-1]), device=hip_device)
    with torch.no_grad():
        y[sel] = model(x[sel])
    _check(case, ("chunks", n, bf, info), y, gx, gp_list, sel, want, _out_tol(case), 2e-4, untouched)


# ---- E. every backward family was reached ----------------------------------------------------------------------------------
def test_every_backward_family_was_reached(request):
    """A change to launch_wave_bwd's thresholds that moves a family out of reach of A to C must update this file on purpose.
    The families are recorded by the tests of A to C as they run, so this test needs all of them in the same session."""
    here = {item.name for item in request.session.items if item.module is request.module}
    wanted = {"test_random_large_frame_backward_plans"} | {"test_backward_dispatch_boundaries[%s]" % b for b in BOUNDARIES} | \
             {"test_backward_workspace_chunks[%s]" % c for c in ("large_head", "C3_no_ring")}
    if not wanted <= here:
        pytest.skip("the coverage guard needs every test of A to C in this session: %d not selected" % len(wanted - here))
    missing = [f for f in FAMILIES if f not in REACHED]
    assert not missing, ("not reached (run the whole file):", missing, sorted(REACHED))
