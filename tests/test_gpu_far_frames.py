"""Every kernel that solves for a rotation (kabsch_rotation_t, molann_amd/csrc/molann_math.h), forward and backward, on frames
far from the reference (tests/far_frames.py): hinge motions and independent conformations, mirror images, exact 180-degree
turns, frames 100-1000 A from the origin and noise-free copies, interleaved so that every tile, ring entry and round of a
kernel holds frames that converge in the solver's fixed Newton steps next to frames that take its guarded loop, and single far
frames at the edges of a 64-frame tile.

For each family of the table (a plan, the environment switches that route it, the kernels last_launch_info must name):
  - outputs against the float64 oracle, within twice the error of the reference's own arithmetic in fp32 (and 1e-5 of the
    scale), 1e-9 for model.double();
  - dL/dx and dL/d(Linear parameters) against float64 autograd through the oracle, on frames whose rotation is well
    conditioned and away from dihedral poles (the cotangent is zero on every other frame);
  - bit for bit: a near frame's outputs and dL/dx row do not change when its neighbours are swapped for far ones (a converged
    lane keeps its rotation while its wave stays in the guarded loop), except dL/dx of the atomics family;
  - degenerate align sets (nearly collinear, one point): finite outputs, distances kept by the alignment, invariant features
    equal to the oracle's;
  - x never written, and a final guard that every family was reached."""

import re

import numpy as np
import pytest
import torch

import far_frames as ff
import test_gpu_random_backward as rb
from molann_amd import workloads as wl
from molann_amd.ann import AlignmentLayer, FeatureLayer, MolANN, PreprocessingANN, _PlanEntry, create_sequential_nn
from molann_amd.atomgroup import Universe
from molann_amd.feature import Feature
from oracle import molann_oracle as mo

pytestmark = pytest.mark.gpu
ANGLE, BOND, DIH, POS = wl.ANGLE, wl.BOND, wl.DIHEDRAL, wl.POSITION
ALA = list(range(22))
P_SEL = list(range(2, 166, 4))                             # every fourth atom of the 166-atom chain (42), as P1 / P2
REACHED = set()


class Spec(object):
    """A model on all atoms of xyz: 0-based align and feature lists, an MLP head (or none), or the AlignmentLayer alone."""

    def __init__(self, xyz, align, feats=(), mlp=None, align_only=False, workload=None):
        self.xyz, self.align, self.feats, self.mlp = np.ascontiguousarray(xyz, np.float32), list(align), list(feats), mlp
        self.align_only, self.workload = align_only, workload

    def build(self, dev, dtype):
        if self.workload is not None:
            from build_util import workload_model
            return workload_model(wl.get_workload(self.workload), dev).to(dtype)
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

    def invariant(self):
        """The outputs that do not depend on the rotation: all of an invariant plan's (head included), else the columns of the
        bond / angle / dihedral features of a plan with no head; None when there are none."""
        if self.align_only:
            return None
        if all(t != POS for t, _ in self.feats):
            return slice(None)
        if self.mlp:
            return None
        cols = []
        for t, idx in self.feats:
            d = mo.feature_dim(t, len(idx), False)
            cols += [t != POS] * d
        return torch.tensor(cols) if any(cols) else None


def _spec(name):
    ala = wl.ALA_DIPEPTIDE_XYZ
    chain = lambda n, seed: wl.synthetic_chain(n_atoms=n, step=1.4, seed=seed)
    if name == "ala_pos":                                  # positions of all 22 atoms: fp64 solve
        return Spec(ala, ALA, [(POS, ALA)])
    if name == "ala_head":                                 # positions + a dihedral, head [26, 16, 4]: fp64 solve
        return Spec(ala, ALA, [(POS, [1, 4, 6, 8, 14, 16, 18, 20]), (DIH, [4, 6, 8, 14])], [26, 16, 4])
    if name == "ala_inv":                                  # bonds / angles / dihedrals only, head [6, 16, 4]: KABSCH_F32
        return Spec(ala, ALA, [(DIH, [4, 6, 8, 14]), (DIH, [6, 8, 14, 16]), (BOND, [4, 6]), (ANGLE, [4, 6, 8])], [6, 16, 4])
    if name == "ala_regs":                                 # 16 atoms, align set and items in the first 16 slots: the regs mode
        return Spec(ala, list(range(16)), [(POS, list(range(16)))])
    if name == "R2":                                       # ~200 16-byte windows per frame: ring entries of 2 frames
        return Spec(chain(600, 13), list(range(5, 600, 14)), [(POS, list(range(1, 600, 4)))])
    if name == "ala_align":
        return Spec(ala, ALA, align_only=True)
    if name == "B8":                                       # 8 position atoms + 2 dihedrals, head [28, 32, 8]
        return Spec(chain(166, 11), P_SEL, [(POS, list(range(10, 160, 19))), (DIH, [20, 21, 22, 23]), (DIH, [90, 91, 92, 93])],
                    [28, 32, 8])
    if name == "P2":                                       # the 42 align atoms' positions
        return Spec(chain(166, 11), P_SEL, [(POS, P_SEL)])
    if name == "B2":                                       # 80 position items
        return Spec(chain(166, 11), P_SEL, [(POS, list(range(3, 163, 2)))])
    if name == "W2000":                                    # over the group backward's 1024 atoms: one wave per frame
        return Spec(chain(2000, 5), list(range(7, 2000, 13)),
                    [(POS, list(range(31, 2000, 97))), (BOND, [100, 101]), (BOND, [1500, 1503])])
    if name == "P1":
        w = wl.get_workload("P1")
        return Spec(w.ref_xyz, [a - 1 for a in w.align], [(t, [a - 1 for a in atoms]) for t, atoms in w.features], w.mlp_dims,
                    workload="P1")
    if name.startswith("A"):                               # the AlignmentLayer alone on a chain of n atoms, up to 300 align atoms
        n = int(name[1:])
        rng = np.random.default_rng(n)
        return Spec(chain(n, 3), sorted(rng.choice(n, size=min(300, n // 4), replace=False).tolist()), align_only=True)
    raise KeyError(name)


# family: (spec, environment, mode, forward kernels, backward kernel or None, batch size).  Every forward pattern must appear in
# the launch info of the family's runs (no_grad forward, autograd forward and backward), the backward one in the backward's.
# mode: "fwd" forward only, "grad" float32 autograd, "f64" model.double() under autograd, "vjp" model.value_and_vjp (values
# and the VJP in one launch).
RING = r"frames_ring_kernel<ND=\d+,B=%d>"
FAMILIES = {
    "lane_jit_f64": ("ala_head", {}, "grad", (r"molann_lane_jit<NL=2>",), r"molann_bwd_ring ", 300),
    "lane_jit_f32": ("ala_inv", {}, "grad", (r"molann_lane_jit<NL=2>",), r"molann_bwd_ring ", 300),
    "lane_jit_align_out": ("ala_align", {}, "grad", (r"molann_lane_jit<align_out>",), None, 300),
    "lane_bwd": ("ala_head", {"MOLANN_NO_RING_BWD": "1"}, "grad", (r"molann_lane_jit<NL=",), r"molann_lane_bwd", 300),
    "lane_regs": ("ala_regs", {"MOLANN_NO_JIT": "1"}, "fwd", (r"frames_lane_kernel<0,features_regs>",), None, 300),
    "lane_lds": ("ala_regs", {"MOLANN_NO_JIT": "1", "MOLANN_NO_REGS": "1"}, "fwd", (r"frames_lane_kernel<0,features_lds>",), None,
                 300),
    "lane_vjp": ("ala_head", {}, "vjp", (r"molann_bwd_ring<values>",), None, 300),
    "ring_B8": ("B8", {}, "grad", (RING % 8,), r"frames_group_bwd_kernel<B=8>", 300),
    "ring_B4_group_B2": ("B2", {}, "grad", (RING % 4,), r"frames_group_bwd_kernel<B=2>", 300),
    "ring_B2": ("R2", {}, "grad", (RING % 2,), r"frames_wave_bwd_gather_kernel", 200),
    "group_B4": ("P2", {}, "grad", (RING % 8,), r"frames_group_bwd_kernel<B=4>", 300),
    "ring_B1": ("B8", {"MOLANN_RING_BATCH": "1"}, "fwd", (r"frames_ring_kernel<ND=\d+> ",), None, 300),
    "wave": ("B8", {"MOLANN_NO_RING": "1"}, "fwd", (r"frames_wave_kernel<",), None, 300),
    "wave_gather_2000": ("W2000", {}, "grad", (r"frames_(ring|wave)_kernel<",), r"frames_wave_bwd_gather_kernel", 130),
    "wave_atomics_2000": ("W2000", {"MOLANN_BWD_ATOMICS": "1"}, "grad", (r"frames_(ring|wave)_kernel<",), r"frames_wave_bwd_kernel",
                          130),
    "align_batch_166": ("A166", {}, "grad", (r"frames_align_batch_kernel<",), r"frames_align_bwd_regs_kernel<", 300),
    "align_regs_1537": ("A1537", {}, "grad", (r"frames_align_regs_kernel<",), r"frames_align_bwd_regs_kernel<", 130),
    "align_wave_12400": ("A12400", {}, "grad", (r"frames_wave_kernel<",), r"frames_wave_bwd", 66),
    "group_vjp_P1": ("P1", {}, "vjp", (r"molann_group_vjp<B=",), None, 300),
    "f64_B8": ("B8", {}, "f64", (r"frames_f64_kernel \(features\)",), r"frames_bwd_f64_kernel", 300),
    "f64_align": ("A166", {}, "f64", (r"frames_f64_kernel \(aligned coordinates\)",), r"frames_bwd_f64_kernel", 300),
}
ATOMICS = ("wave_atomics_2000",)                           # dL/dx summed by atomics: not bitwise reproducible


def _align_layer(model):
    if isinstance(model, AlignmentLayer):
        return model
    pp = model.preprocessing_layer if isinstance(model, MolANN) else model
    return pp.align_layer


def _infos(model):
    infos = [e.plan.last_launch_info() for m in model.modules() if hasattr(m, "_plans")
             for e in m._plans().values() if isinstance(e, _PlanEntry)]
    if isinstance(model, MolANN):
        infos.append(model.last_launch_info())
    return " | ".join(infos)


def _run(model, x, G, mode):
    """(y, dL/dx, parameter gradients, forward info, backward info); x is never written."""
    x0 = x.clone()
    if mode == "vjp":
        y, dx = model.value_and_vjp(x, G)
        torch.cuda.synchronize()
        info = _infos(model)
        assert torch.equal(x, x0)
        return y, dx, [], info, info
    xg = x.clone().requires_grad_(True)
    for p in model.parameters():
        p.grad = None
    y = model(xg)
    fwd = _infos(model)
    (y * G).sum().backward()
    torch.cuda.synchronize()
    bwd = _infos(model)
    assert torch.equal(xg.detach(), x0)
    return y.detach(), xg.grad, [p.grad.clone() for p in model.parameters()], fwd, bwd


def _oracle(spec, model, xs, Gs, ref, dtype=torch.float64, grad=True):
    """y (and dL/dx, dL/d(parameters) of sum(y * Gs)) on the frames xs through the oracle, in dtype."""
    xx = xs.detach().cpu().to(dtype).requires_grad_(grad)
    r = ref.to(dtype)
    prm = []
    if spec.align_only:
        y = mo.align_forward(xx, spec.align, r)
    elif spec.mlp:
        lins = [m for m in model.ann_layers if isinstance(m, torch.nn.Linear)]
        ws = [l.weight.detach().cpu().to(dtype).requires_grad_(grad) for l in lins]
        bs = [l.bias.detach().cpu().to(dtype).requires_grad_(grad) for l in lins]
        prm = [t for pair in zip(ws, bs) for t in pair]
        y = mo.molann_forward(xx, spec.feats, ws, bs, False, spec.align, r)
    else:
        y = mo.preprocessing_forward(xx, spec.feats, False, spec.align, r)
    if not grad:
        return y.detach(), None, None
    (y * Gs.cpu().to(dtype)).sum().backward()
    return y.detach(), xx.grad, [p.grad for p in prm]


def _err(got, want):
    return (got.detach().cpu().double() - want.double()).abs()


def _check_outputs(spec, model, x, y, rows, lab, ref, f64, cond, what):
    """Outputs of the frames `rows` against the float64 oracle: within max(1e-5 scale, 2 x the error of the reference's own
    arithmetic in fp32 on the frames of the same regime); model.double(): 1e-9 of the scale on frames whose rotation is
    defined."""
    xs = x[rows].cpu()
    want, _, _ = _oracle(spec, model, xs, None, ref, grad=False)
    scale = max(1.0, float(want.abs().max()))
    err = _err(y[rows], want).flatten(1).max(1).values
    if f64:
        ok = torch.from_numpy(cond[rows] >= 0.01)
        assert float(err[ok].max()) <= 1e-9 * scale, (what, "y", float(err[ok].max()))
        return
    own32, _, _ = _oracle(spec, model, xs.float(), None, ref, dtype=torch.float32, grad=False)
    own = _err(own32, want).flatten(1).max(1).values
    bound = torch.empty_like(own)
    for r in set(lab[i] for i in rows):
        m = torch.tensor([lab[i] == r for i in rows])
        bound[m] = max(1e-5 * scale, 2.0 * float(own[m].max()))
    bad = (err > bound).nonzero().flatten().tolist()
    assert not bad, (what, "y", [(rows[i], lab[rows[i]], float(err[i]), float(bound[i])) for i in bad[:6]])


def _check_grads(spec, model, x, G, gx, gp, sel, Gs, ref, tol, what):
    _, gx_want, gp_want = _oracle(spec, model, x[sel], Gs, ref)
    s = max(1e-6, float(gx_want.abs().max()))
    e = float(_err(gx[sel], gx_want).max())
    assert e <= tol * s, (what, "x.grad", e, s)
    for i, (p, w) in enumerate(zip(gp, gp_want)):
        s = max(1e-6, float(w.abs().max()))
        e = float(_err(p, w).max())
        assert e <= tol * s, (what, "param %d" % i, e, s)
    rest = torch.ones(gx.shape[0], dtype=torch.bool, device=gx.device)
    rest[sel] = False
    if bool(rest.any()):
        assert float(gx[rest].abs().max()) == 0.0, (what, "rows of frames with a zero cotangent")


def _cotangent(spec, model, x, cond, n, dtype, dev, seed):
    """G nonzero on sampled frames (both tile edges, the ends and some in between) whose rotation is well conditioned and
    that sit away from dihedral poles."""
    rng = np.random.default_rng(seed)
    cand = sorted(set(range(4)) | set(range(60, 68)) | set(range(n - 4, n)) | set(rng.choice(n, size=12, replace=False).tolist()))
    cand = [i for i in cand if 0 <= i < n]
    poles = rb._dihedral_poles(x[cand].cpu().double(), spec.feats).numpy()
    sel = [i for i, p in zip(cand, poles) if cond[i] >= 0.05 and not p]
    if spec.align_only:
        shape = (n,) + tuple(x.shape[1:])
    else:
        shape = (n, spec.mlp[-1] if spec.mlp else sum(mo.feature_dim(t, len(idx), False) for t, idx in spec.feats))
    Gs = torch.from_numpy(rng.standard_normal((len(sel),) + shape[1:])).to(dtype)
    G = torch.zeros(shape, dtype=dtype)
    G[sel] = Gs
    return G.to(dev), sel, Gs


def _same_rows(a, b, rows, what):
    rows = torch.tensor(rows, device=a.device)
    diff = (a[rows] != b[rows]).flatten(1).any(1)
    assert not bool(diff.any()), (what, "changed with its neighbours", rows[diff].tolist()[:8])


def _forward(model, x):
    """model(x) under no_grad and the launch info; x is never written."""
    x0 = x.clone()
    with torch.no_grad():
        y = model(x)
    torch.cuda.synchronize()
    assert torch.equal(x, x0)
    return y, _infos(model)


def _degenerate(spec, model, n, dev, dtype, y_near, near, ref, what):
    """Nearly collinear and one-point align sets: finite outputs, the alignment keeps distances, invariant outputs equal the
    oracle's, and the near frames around them unchanged."""
    lab = ["degenerate" if i % 3 == 1 else "near" for i in range(n)]
    xd = torch.from_numpy(ff.compose(lab, spec.xyz, spec.align, seed=31, base=near)).to(dev, dtype)
    y, _ = _forward(model, xd)
    rows = [i for i in range(n) if lab[i] == "degenerate"][:24]
    near_rows = [i for i in range(n) if lab[i] == "near"]
    _same_rows(y, y_near, near_rows, (what, "degenerate batch"))
    assert bool(torch.isfinite(y[near_rows]).all()), (what, "degenerate batch: non-finite output of a near frame")
    # a feature whose atoms all sit at one point has no value in the reference either: finite wherever the oracle is
    want, _, _ = _oracle(spec, model, xd[rows], None, ref, grad=False)
    got = y[rows].detach().cpu().double()
    fin = torch.isfinite(want)
    assert bool(torch.isfinite(got[fin]).all()), (what, "degenerate: non-finite output")
    if spec.align_only:
        atoms = np.random.default_rng(1).choice(len(spec.xyz), size=min(200, len(spec.xyz)), replace=False)
        a, b = got[:, atoms], xd[rows][:, atoms].cpu().double()
        da, db = torch.cdist(a, a), torch.cdist(b, b)
        e = float((da - db).abs().max())
        assert e <= 2e-5 * max(1.0, float(db.max())), (what, "degenerate: distances", e)
    inv = spec.invariant()
    if inv is not None:
        own32, _, _ = _oracle(spec, model, xd[rows].float(), None, ref, dtype=torch.float32, grad=False)
        # (rows with a dihedral at a pole, where fp32 rounding alone moves it, are left out as in the gradient checks)
        f = fin[:, inv] & ~rb._dihedral_poles(xd[rows].cpu().double(), spec.feats).unsqueeze(1)
        g, w, o = got[:, inv], want[:, inv], own32.double()[:, inv]
        if bool(f.any()):
            e, own = float((g[f] - w[f]).abs().max()), float((o[f] - w[f]).abs().max())
            assert e <= max(1e-5 * max(1.0, float(w[f].abs().max())), 2.0 * own), (what, "degenerate: invariant outputs", e, own)


@pytest.mark.parametrize("family", list(FAMILIES))
def test_far_frames(family, hip_device, monkeypatch):
    spec_name, env, mode, fwd_pats, bwd_pat, n = FAMILIES[family]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    spec = _spec(spec_name)
    f64 = mode == "f64"
    dtype = torch.float64 if f64 else torch.float32
    model = spec.build(hip_device, dtype)
    if mode in ("vjp", "fwd"):
        model.requires_grad_(False)
    ref = _align_layer(model).ref_x.detach().cpu().double()
    xyz, al = spec.xyz, spec.align
    near = ff.draw("near", xyz, al, n, seed=len(family))
    labels = {"mixed": ff.interleaved(n), "single": ff.single(n, "mirror")}
    batches = {"mixed": ff.compose(labels["mixed"], xyz, al, seed=7, base=near),
               "single": ff.compose(labels["single"], xyz, al, seed=9, base=near)}
    conds = {k: ff.conditioning(v, xyz, al) for k, v in batches.items()}
    leaves = ff.leaves_fixed_steps(batches["mixed"], xyz, al, 32 if spec_name == "ala_inv" else 64)
    assert leaves.mean() > 0.25, (family, float(leaves.mean()))        # the guarded loop is reached
    x_near = torch.from_numpy(near).to(hip_device, dtype)
    infos = []
    y0n, info = _forward(model, x_near)
    infos.append(info)
    if mode in ("grad", "f64", "vjp"):
        # one cotangent for every batch (nonzero on frames well conditioned in both far batches): near rows compare bit for bit
        cond = np.minimum(conds["mixed"], conds["single"])
        G, sel, Gs = _cotangent(spec, model, torch.from_numpy(batches["mixed"]).to(hip_device, dtype), cond, n, dtype,
                                hip_device, seed=len(family))
        assert len(sel) >= 8, (family, len(sel))
        y0, gx0, _, fwd, bwd = _run(model, x_near, G, mode)
        infos += [fwd, bwd]
        if bwd_pat is not None:
            assert re.search(bwd_pat, bwd), (family, bwd)
    tol = 1e-9 if f64 else 5e-4
    for name, xb in batches.items():
        what = (family, name)
        lab = labels[name]
        x = torch.from_numpy(xb).to(hip_device, dtype)
        far_rows = [i for i in range(n) if lab[i] != "near"]
        near_rows = [i for i in range(n) if lab[i] == "near"]
        rows = sorted(set(far_rows[:6]) | set(far_rows[-6:]) | {0, 63 % n, 64 % n, n - 1} |
                      set(np.random.default_rng(n).choice(n, size=min(16, n), replace=False).tolist()))
        y, info = _forward(model, x)
        infos.append(info)
        _check_outputs(spec, model, x, y, rows, lab, ref, f64, conds[name], what + ("no_grad",))
        _same_rows(y, y0n, near_rows, what + ("no_grad y",))
        if mode == "fwd":
            continue
        y, gx, gp, fwd, bwd = _run(model, x, G, mode)
        infos += [fwd, bwd]
        if bwd_pat is not None:
            assert re.search(bwd_pat, bwd), (what, bwd)
        _check_outputs(spec, model, x, y, sorted(set(rows) | set(sel)), lab, ref, f64, conds[name], what)
        _check_grads(spec, model, x, G, gx, gp, sel, Gs, ref, tol, what)
        _same_rows(y, y0, near_rows, what + ("y",))
        if family not in ATOMICS:
            _same_rows(gx, gx0, near_rows, what + ("dL/dx",))
    _degenerate(spec, model, n, hip_device, dtype, y0n, near, ref, family)
    seen = " | ".join(infos)
    missing = [p for p in fwd_pats if not re.search(p, seen)]
    assert not missing, (family, missing, seen)
    REACHED.add(family)
def test_every_far_frame_family_was_reached(request):
    """The families are recorded by test_far_frames as they pass, so this guard needs all of them in the same session."""
    here = {item.name for item in request.session.items if item.module is request.module}
    wanted = {"test_far_frames[%s]" % f for f in FAMILIES}
    if not wanted <= here:
        pytest.skip("the coverage guard needs every family in this session: %d not selected" % len(wanted - here))
    missing = sorted(set(FAMILIES) - REACHED)
    assert not missing, ("not reached:", missing)
