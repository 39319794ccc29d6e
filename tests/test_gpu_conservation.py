"""Every kernel that hands out a gradient with respect to x, held to zero net force and zero net torque (tests/conservation.py).

The values are invariant under rigid motions of the frame (features of Kabsch-aligned coordinates, bonds, angles, dihedrals), so
per frame sum_a F_a = 0 and sum_a (x_a - c) x F_a = 0 for F = dL/dx, whatever the cotangent.  The oracle tolerances of the other
files (1e-4 to 5e-4 of the gradient's scale in float32, 1e-9 in float64) are orders looser than that: a centroid share, a G_H
term or one atom of an item's backward slightly off passes them and fails here (tests/test_conservation_host.py plants such faults).

Every case runs on frames of tests/far_frames.py: a mixed batch (far_frames.interleaved) and a near batch with a mirror frame at
positions 0, 63, 64 and the last, on the frames `conservation.select` keeps (at least 75 % of every regime).  The kernel's r_F and
r_T are held, per regime, to max(16 u, 4 x the largest residual of the oracle's autograd in the same precision on the same frames
with the same cotangent): `conservation.bound`.  No bound comes from a kernel's output.  Each case asserts the kernel it names in the
launch info, and prints its residuals next to the reference's.

  1. autograd, float32 and float64: every family of test_gpu_far_frames.FAMILIES with a gradient (its plan, environment switches
     and kernel patterns), and two families with an uncentred ref_x;
  2. the float64 one-launch entries vjp, restraint, hills, grid, bias, opes, bias_opes and opes_table (models, tables and builders
     of test_gpu_f64_rounds) on 7 / 12 / 30 / 40 atoms: aligned behind a head, aligned without a head, and without alignment or
     position items; the plan without alignment that keeps its position items is the control and must fail;
  3. value_and_jacobian: every row jac[f, k] as a force, the same shapes;
  4. forward mode: torch.func.jvp along the velocity field of a rigid motion, over that along a field of the same per-atom norms
     and random directions, against the same ratio of torch.func.jvp through the oracle;
  5. second order: h = d/dx <u, dL/dx> from frames_hvp_f64_kernel, directly and under create_graph=True: sum_a h_a = 0."""

import copy
import re

import numpy as np
import pytest
import torch

import conservation as cv
import test_gpu_alignment_gradients as ag
import test_gpu_double_backward as db
import test_gpu_f64_rounds as rounds
import test_gpu_far_frames as fam
import test_gpu_jvp_plans as jp
import test_gpu_random_backward as rb
import test_gpu_second_order_exact as so
import test_gpu_value_and_bias_f64 as vb
import test_gpu_value_and_bias_opes_f64 as vbo
import test_gpu_value_and_grid_f64 as vg
import test_gpu_value_and_hills_f64 as vh
import test_gpu_value_and_jacobian_f64 as vjac
import test_gpu_value_and_opes_f64 as vo
import test_gpu_value_and_restraint_f64 as vr
import test_gpu_value_and_vjp_f64 as vv
from molann_amd import workloads as wl
from oracle import molann_oracle as mo

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
BITS = {F32: 32, F64: 64}
REACHED = set()

# ---- 1. autograd ---------------------------------------------------------------------------------------------------------------
# family -> FAMILIES' row + the shift of ref_x (None: as built, centred)
AUTOGRAD = dict((f, row + (None,)) for f, row in fam.FAMILIES.items() if row[2] in ("grad", "vjp", "f64"))
AUTOGRAD["uncentred_f32"] = ("ala_head", {}, "grad", (r"molann_lane_jit<NL=2>",), r"molann_bwd_ring ", 300, ag.SHIFT)
AUTOGRAD["uncentred_f64"] = ("B8", {}, "f64", (r"frames_f64_kernel \(features\)",), r"frames_bwd_f64_kernel", 300, ag.SHIFT)
# (the seed of a case's batches is its name's length, or the workload's atoms + 1)
# A family of FAMILIES that names no backward kernel: under autograd the AlignmentLayer of 22 atoms runs molann_lane_jit<NL=0>
# forward (its align_out twin only under no_grad) and the ring backward.
BACKWARD_OF = {"lane_jit_align_out": r"molann_bwd_ring "}
ENTRY_N = 66                                               # the one-launch entries: a single batch and a mixed batch of 66, joined
SEEDS = rounds.SEEDS


def _report(what, table):
    for reg, (f, f_ref, t, t_ref) in sorted(table.items()):
        print("conservation %-34s %-8s r_F %.2e (ref %.2e, x%.2f)  r_T %.2e (ref %.2e, x%.2f)"
              % (what, reg, f, f_ref, f / max(f_ref, 1e-300), t, t_ref, t / max(t_ref, 1e-300)))


def _joined(b):
    """The single batch, then the mixed one: far frames at 0, 63, 64 and the single batch's last position"""
    return b["single"][0] + b["mixed"][0], np.concatenate([b["single"][1], b["mixed"][1]])


def _out_shape(spec, x):
    if spec.align_only:
        return tuple(x.shape)
    return (x.shape[0], spec.mlp[-1] if spec.mlp else sum(mo.feature_dim(t, len(i), False) for t, i in spec.feats))


@pytest.mark.parametrize("family", list(AUTOGRAD))
def test_autograd_forces(family, hip_device, monkeypatch):
    spec_name, env, mode, fwd_pats, bwd_pat, n, shift = AUTOGRAD[family]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    spec = fam._spec(spec_name)
    dtype = F64 if mode == "f64" else F32
    model = spec.build(hip_device, dtype)
    if mode == "vjp":
        model.requires_grad_(False)
    buf = fam._align_layer(model).ref_x
    if shift is not None:
        with torch.no_grad():
            buf.copy_(buf + torch.tensor(shift, dtype=dtype, device=hip_device))
        assert float(buf.mean(0).abs().max()) > 1.0
    ref = buf.detach().cpu().double()
    for name, (lab, xb) in cv.batches(spec.xyz, spec.align, n, len(family), spec.feats).items():
        what = "%s %s" % (family, name)
        keep, _ = cv.select(xb, lab, spec.xyz, spec.align, spec.feats, what)
        x = torch.from_numpy(xb).to(hip_device, dtype)
        G = cv.cotangent(_out_shape(spec, x), len(family), dtype)
        _, gx, _, fwd, bwd = fam._run(model, x, G.to(hip_device), mode)
        if mode == "vjp":
            assert all(re.search(p, bwd) for p in fwd_pats), (what, bwd)
        else:
            assert re.search(bwd_pat or BACKWARD_OF[family], bwd), (what, bwd)
        rows = torch.from_numpy(np.nonzero(keep)[0])
        _, gx_ref, _ = fam._oracle(spec, model, x[rows.to(hip_device)], G[rows], ref, dtype=dtype)
        table = cv.check(xb[keep], gx[rows.to(hip_device)], gx_ref, [l for l, k in zip(lab, keep) if k], np.ones(len(rows), bool),
                         BITS[dtype], what, regimes=set(lab))
        _report(what, table)
    REACHED.add(("autograd", family))


# ---- 2. the float64 one-launch entries -----------------------------------------------------------------------------------------
ENTRIES = ("vjp", "restraint", "hills", "grid", "bias", "opes", "bias_opes", "opes_table")
SHAPES = {"head": "head", "aligned": "aligned_features", "invariant": "features"}
ENTRY_CASES = [(e, n_inp, s) for e in ENTRIES for n_inp, _ in rounds.SIZES for s in SHAPES]
JAC_CASES = [("jacobian", n_inp, s) for n_inp, _ in rounds.SIZES for s in SHAPES]


def _entry_case(entry, n_inp, shape):
    case = rounds._case(entry, n_inp, SHAPES[shape])
    if shape == "invariant":                               # no alignment: the position items go
        case = rb.Case(case.name, case.xyz, [f for f in case.feats if f[0] != rb.POS], align=None, mlp=None)
    assert case.align is not None or all(t != rb.POS for t, _ in case.feats)
    return case


def _entry_frames(case, n_inp, seed):
    """(labels, float32 frames, kept mask) of the joined batch, and a second batch for the tables' centres"""
    lab, xb = _joined(cv.batches(case.xyz, case.align, ENTRY_N, n_inp + 100 * seed, case.feats))
    tab = cv.batches(case.xyz, case.align, ENTRY_N, 900 + n_inp + 100 * seed)["mixed"][1]
    return lab, xb, tab


def _record_references(monkeypatch, log):
    """The siblings' reference builders, wrapped to keep dV/dx of the float64 autograd through the oracle they return"""
    def wrap(mod, name, pick):
        orig = getattr(mod, name)

        def wrapped(*a, **k):
            out = orig(*a, **k)
            log[(mod.__name__, name)] = pick(out)
            return out
        monkeypatch.setattr(mod, name, wrapped)
    for mod in (vv, vr, vh, vo):
        wrap(mod, "_oracle", lambda out: out[-1])
    wrap(vg, "_oracle", lambda out: out[0][-1])
    wrap(vb, "_reference_terms", lambda out: out[1][-1])
    wrap(vbo, "_reference", lambda out: out[2][-1])


REFERENCE_OF = {"vjp": (vv, "_oracle"), "restraint": (vr, "_oracle"), "hills": (vh, "_oracle"), "grid": (vg, "_oracle"),
                "bias": (vb, "_reference_terms"), "opes": (vo, "_oracle"), "bias_opes": (vbo, "_reference"), "opes_table": (vo, "_oracle")}


def _entry_context(entry, n_inp, shape, case, dev, monkeypatch):
    """rounds._context on the far-frame batch: the entry's model, terms and reference dV/dx from the first seed whose builders hold
    their margins; the selection's share is asserted on every seed tried"""
    c = rounds.Ctx()
    c.entry, c.shape, c.dev, c.case = entry, SHAPES[shape], dev, case
    c.lanes = rounds._lanes_of(n_inp, c.shape)
    c.model = case.build(dev).double().requires_grad_(False)
    c.args = (case.feats, case.uav, case.align)
    c.d_out = case.mlp[-1] if case.mlp else case.d_feat()
    missed, log = [], {}
    _record_references(monkeypatch, log)
    for seed in SEEDS:
        lab, xb, tab = _entry_frames(case, n_inp, seed)
        c.nb, c.what = len(xb), "%s %s n_inp=%d (seed %d)" % (entry, shape, n_inp, seed)
        c.x, c.x_tab = torch.from_numpy(xb).to(dev, F64), torch.from_numpy(tab).to(dev, F64)
        keep, _ = cv.select(xb, lab, case.xyz, case.align, case.feats, c.what)       # (outside the try: a lost share fails the case)
        try:
            rounds._prepare(c, n_inp + seed)
            mod, name = REFERENCE_OF[entry]
            c.dx_ref = log[(mod.__name__, name)]
            assert tuple(c.dx_ref.shape) == tuple(c.x.shape), (c.what, c.dx_ref.shape)
            live = c.dx_ref.abs().flatten(1).sum(1).numpy() > 0
            # (a bias that is flat on a frame - inside a flat-bottomed restraint, outside a table or past the cutoff of every kernel -
            # has no force to test there: residuals() masks the frame.  Three quarters of the kept frames, and some of every regime,
            # have one; the share is printed.)
            assert (keep & live).sum() >= cv.KEEP * keep.sum(), "the reference's force is zero on %d of %d frames" % ((keep & ~live).sum(), keep.sum())
            for reg in set(lab):
                assert (keep & live)[np.array([l == reg for l in lab])].any(), "the reference's force is zero on every %s frame" % reg
            print("conservation %s: %d of %d selected frames have a force" % (c.what, (keep & live).sum(), keep.sum()))
            if missed:
                print("conservation %s: earlier seeds missed: %s" % (c.what, missed))
            return c, lab, xb, keep & live
        except AssertionError as err:
            missed.append((seed, str(err)[:120]))
    raise AssertionError(("no seed holds the builders' margins", entry, n_inp, shape, missed))


@pytest.mark.parametrize("entry,n_inp,shape", ENTRY_CASES, ids=["%s-%d-%s" % c for c in ENTRY_CASES])
def test_one_launch_forces(entry, n_inp, shape, hip_device, monkeypatch):
    case = _entry_case(entry, n_inp, shape)
    c, lab, xb, keep = _entry_context(entry, n_inp, shape, case, hip_device, monkeypatch)
    out, info = c.call(c.x, c.pf)
    torch.cuda.synchronize()
    assert rounds.KERNELS[entry] in info and info.count("_kernel") == 1, (c.what, info)
    table = cv.check(xb, out["grad_x"], c.dx_ref, lab, keep, 64, c.what)
    _report(c.what, table)
    REACHED.add(("entry", entry, n_inp, shape))


@pytest.mark.parametrize("n_inp", [n for n, _ in rounds.SIZES])
def test_control_position_items_without_alignment_fail(n_inp, hip_device):
    """value_and_vjp on the plan without alignment that keeps its position items: not invariant, and the check says so"""
    case = vv._small_case(n_inp, None, head=False)
    assert any(t == rb.POS for t, _ in case.feats)
    model = case.build(hip_device).double().requires_grad_(False)
    lab, xb, _ = _entry_frames(case, n_inp, 0)
    x = torch.from_numpy(xb).to(hip_device, F64)
    G = cv.cotangent((len(xb), case.d_feat()), n_inp, F64)
    _, dx, info = vv._call(model, x, G.to(hip_device))
    assert vv.KERNEL in info, info
    _, want = vv._oracle(model, case.feats, case.uav, case.align, x, G)
    assert float((dx.cpu() - want).abs().max()) <= 1e-9 * float(want.abs().max())
    r_F, r_T = cv.residuals(xb, dx)
    print("conservation control n_inp=%d: r_F %.2f to %.2f, r_T %.2f to %.2f" % (n_inp, r_F.min(), r_F.max(), r_T.min(), r_T.max()))
    assert r_F.max() > 0.1 and r_T.max() > 0.1
    # the bound of the same plan without its position items (the invariant shape), the same cotangent on the columns that stay
    keep_cols = torch.tensor([t != rb.POS for t, idx in case.feats for _ in range(mo.feature_dim(t, len(idx), case.uav))])
    inv = [f for f in case.feats if f[0] != rb.POS]
    _, want_inv = vv._oracle(model, inv, case.uav, case.align, x, G[:, keep_cols])
    cv.check(xb, want_inv, want_inv, lab, np.ones(len(xb), bool), 64, "control's reference")
    with pytest.raises(AssertionError, match="over the bound"):
        cv.check(xb, dx, want_inv, lab, np.ones(len(xb), bool), 64, "control")
    REACHED.add(("control", n_inp))


# ---- 3. value_and_jacobian -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("entry,n_inp,shape", JAC_CASES, ids=["%s-%d-%s" % c for c in JAC_CASES])
def test_jacobian_rows(entry, n_inp, shape, hip_device):
    case = _entry_case(entry, n_inp, shape)
    model = vjac._build(case, hip_device)
    what = "jacobian %s n_inp=%d" % (shape, n_inp)
    lab, xb, _ = _entry_frames(case, n_inp, 0)
    keep, _ = cv.select(xb, lab, case.xyz, case.align, case.feats, what)
    x = torch.from_numpy(xb).to(hip_device, F64)
    _, jac, info = vjac._call(model, x)
    assert vjac.KERNEL in info and info.count("_kernel") == 1, (what, info)
    _, j_ref = vjac._oracle(case, model, x)
    assert jac.shape == j_ref.shape and jac.dim() == 4
    _report(what, cv.check(xb, jac, j_ref, lab, keep, 64, what))
    REACHED.add(("jacobian", n_inp, shape))


# ---- 4. forward mode -----------------------------------------------------------------------------------------------------------
def _ratio(t):
    """per frame |J v_rigid|max / |J v_shuffled|max from t [2, n, ...]"""
    t = t.detach().cpu().double().flatten(2).abs().amax(2).numpy()
    assert (t[1] > 0).all()
    return t[0] / t[1]


# The plans of test_gpu_jvp_plans with an alignment or without position items: its far-frame plans, and its dispatch boundaries (every
# lane group of frames_jvp with and without the rotation tangent; PAST_GRID's plans are among them) but pos_noalign_* (position items,
# no alignment: not invariant) and align166 / 1537 / 12400 (the far-frame plans A166 / A1537 / A12400 again).
# pos_a6_i7, pos_a3_i17 and pos_a3_i64 stay out as well: their 3 and 6 random align atoms of the chain are nearly collinear,
# (s2 + s3) / s1 of the reference itself under the selection's 0.05, so no noise-free frame can pass it; their lane groups with the
# rotation tangent (8, 32, 64) are those of ala_g8, ala_head and B8.
ILL_CONDITIONED = ("pos_a6_i7", "pos_a3_i17", "pos_a3_i64")
JVP_BOUNDARIES = [b for b in jp.BOUNDARIES if not b.startswith("pos_noalign") and not b.startswith("align") and b not in ILL_CONDITIONED]
JVP_PLANS = jp.FAR + JVP_BOUNDARIES


def _jvp_case(name):
    if name in jp.FAR:
        return jp._far_case(name)
    return jp._boundary(name) + (ENTRY_N,)


@pytest.mark.parametrize("dtype", jp.DTYPES, ids=jp.DT_IDS)
@pytest.mark.parametrize("name", JVP_PLANS)
def test_jvp_along_rigid_motions(name, dtype, hip_device):
    case, G, rot, n = _jvp_case(name)
    assert case.align is not None or all(t != rb.POS for t, _ in case.feats)
    model = jp._build(case, hip_device, dtype)
    f = jp._oracle(case, model, features=True)
    head = copy.deepcopy(model.ann_layers).cpu().to(dtype) if case.mlp else None
    for bname, (lab, xb) in cv.batches(case.xyz, case.align, n, len(name), case.feats, angles=case.uav).items():
        what = "jvp %s %s %s" % (name, jp.DT_IDS[jp.DTYPES.index(dtype)], bname)
        keep, _ = cv.select(xb, lab, case.xyz, case.align, case.feats, what, angles=case.uav)
        v = cv.rigid_tangent(xb, len(name))
        V = torch.from_numpy(np.stack([v, cv.shuffled_tangent(v, len(name))])).to(dtype)
        x = torch.from_numpy(xb).to(dtype)
        xd, Vd = x.to(hip_device), V.to(hip_device)
        runs = [("features", jp._feat(model), f)]
        if head is not None:
            runs.append(("model", model, lambda a: head(f(a))))
        for which, module, oracle in runs:
            got = _ratio(jp._many(module, xd, Vd))
            torch.cuda.synchronize()
            assert jp._jvp_info(model) == (G, rot, 2), (what, jp._jvp_info(model))
            ref = _ratio(torch.stack([torch.func.jvp(oracle, (x[keep],), (V[t][keep],))[1] for t in range(2)]))
            kl = [l for l, k in zip(lab, keep) if k]
            assert set(kl) == set(lab), (what, sorted(set(kl)))
            b = cv.bound(ref, kl, cv.U[BITS[dtype]])
            big, big_ref = cv.largest(got[keep], kl), cv.largest(ref, kl)
            for reg in sorted(b):
                print("conservation %-34s %-8s %-8s |Jv_rigid|/|Jv_shuffled| %.2e (ref %.2e, x%.2f)"
                      % (what, which, reg, big[reg], big_ref[reg], big[reg] / max(big_ref[reg], 1e-300)))
            bad = cv.exceeding(got[keep], kl, b)
            assert not bad, (what, which, bad[:6])
    REACHED.add(("jvp", name, dtype))


# ---- 5. second order -----------------------------------------------------------------------------------------------------------
def _workload_frames(w, what):
    al = [a - 1 for a in w.align] if w.align else None
    feats = [(t, [a - 1 for a in atoms]) for t, atoms in w.features] if w.kind != "align" else []
    lab, xb = _joined(cv.batches(w.ref_xyz, al, ENTRY_N, w.n_atoms + 1, feats, rotation=False))
    keep, _ = cv.select(xb, lab, w.ref_xyz, al, feats, what, rotation=False)      # the net force alone: see conservation.select
    return lab, xb, keep


@pytest.mark.parametrize("name", so.PLANS)
def test_hvp_net_force(name, hip_device):
    """frames_hvp_f64_kernel on the plans' features: sum_a h_a = 0 for any direction u and cotangent g"""
    w, plan, fwd = so._plan(name, hip_device)
    what = "hvp %s" % name
    lab, xb, keep = _workload_frames(w, what)
    x = torch.from_numpy(xb).double()
    g = cv.cotangent((len(xb), plan.feature_dim), 13, F64)
    u = cv.cotangent(tuple(x.shape), 14, F64)
    hx, _ = so._hvp(plan, x.to(hip_device), g.to(hip_device), u.to(hip_device))
    assert plan.last_launch_info().startswith("frames_hvp_f64_kernel"), plan.last_launch_info()
    rows = torch.from_numpy(np.nonzero(keep)[0])
    want = so._oracle_hx(fwd, x[rows], g[rows], u[rows])
    kl = [l for l, k in zip(lab, keep) if k]
    _report(what, cv.check(xb[keep], hx.cpu()[rows], want, kl, np.ones(len(rows), bool), 64, what, torque=False, regimes=set(lab)))
    REACHED.add(("hvp", name))


@pytest.mark.parametrize("family", so.FAMILIES)
def test_force_gradient_net_force(family, hip_device, monkeypatch):
    """h = d/dx <u, dE/dx> of model.double() under create_graph=True: one launch of the second-order kernel, sum_a h_a = 0"""
    w, model = db._build(family, hip_device)
    m = copy.deepcopy(model).double()
    what = "force gradient %s" % family
    lab, xb, keep = _workload_frames(w, what)
    x = torch.from_numpy(xb).double()
    G = db._cotangent(w, model, len(xb))
    u = cv.cotangent(tuple(x.shape), 14, F64)
    xg = x.to(hip_device).requires_grad_(True)
    (F,) = torch.autograd.grad((m(xg) * G.to(hip_device)).sum(), xg, create_graph=True)
    calls = so._count_launches(monkeypatch)
    (h,) = torch.autograd.grad((F * u.to(hip_device)).sum(), xg)
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert calls["features_hvp_f64"] == 1 and calls["features_f64"] == 0, (what, calls)
    forward, params = db._oracle_forward(w, model)
    rows = torch.from_numpy(np.nonzero(keep)[0])
    xx = x[rows].requires_grad_(True)
    (Fr,) = torch.autograd.grad((forward(xx, params) * G[rows]).sum(), xx, create_graph=True)
    (want,) = torch.autograd.grad((Fr * u[rows]).sum(), xx)
    kl = [l for l, k in zip(lab, keep) if k]
    _report(what, cv.check(xb[keep], h.cpu()[rows], want, kl, np.ones(len(rows), bool), 64, what, torque=False, regimes=set(lab)))
    REACHED.add(("force gradient", family))


# ---- the cases' frames, for the host test of the selection ---------------------------------------------------------------------
def selection_cases():
    """(name, xyz, align, feats, n, seed, rotation, angles) of every batch pair `conservation.batches` draws for this file, with the
    arguments its `conservation.select` gets"""
    out = []
    for family, row in AUTOGRAD.items():
        s = fam._spec(row[0])
        out.append(("autograd-" + family, s.xyz, s.align, s.feats, row[5], len(family), True, False))
    for entry, n_inp, shape in ENTRY_CASES + JAC_CASES:
        case = _entry_case(entry, n_inp, shape)
        for seed in (SEEDS if entry != "jacobian" else (0,)):
            out.append(("%s-%d-%s-seed%d" % (entry, n_inp, shape, seed), case.xyz, case.align, case.feats, ENTRY_N, n_inp + 100 * seed, True, False))
    for name in JVP_PLANS:
        case, _, _, n = _jvp_case(name)
        out.append(("jvp-" + name, case.xyz, case.align, case.feats, n, len(name), True, case.uav))
    for name in sorted(set(so.PLANS) | {db.FAMILIES[f][0] for f in so.FAMILIES}):
        w = wl.get_workload(name)
        al = [a - 1 for a in w.align] if w.align else None
        feats = [(t, [a - 1 for a in atoms]) for t, atoms in w.features] if w.kind != "align" else []
        out.append(("hvp-" + name, w.ref_xyz, al, feats, ENTRY_N, w.n_atoms + 1, False, False))
    seen, uniq = set(), []
    for c in out:                                          # the same frames once
        key = (np.asarray(c[1]).tobytes(), repr(c[2]), repr(c[3])) + c[4:]
        if key not in seen:
            seen.add(key)
            uniq.append(c)
    return uniq


def test_every_family_was_reached(request):
    """The cases are recorded as they pass, so this guard needs all of them in the same session."""
    here = {item.name.split("[")[0] for item in request.session.items if item.module is request.module}
    n_here = sum(1 for item in request.session.items if item.module is request.module)
    wanted = ({("autograd", f) for f in AUTOGRAD} | {("entry",) + c for c in ENTRY_CASES} | {("control", n) for n, _ in rounds.SIZES} |
              {("jacobian", n, s) for _, n, s in JAC_CASES} | {("jvp", n, d) for n in JVP_PLANS for d in jp.DTYPES} |
              {("hvp", p) for p in so.PLANS} | {("force gradient", f) for f in so.FAMILIES})
    if len(here) != 8:
        pytest.skip("the coverage guard needs every test of this file in the session: %d of 8 selected" % len(here))
    assert n_here == len(wanted) + 1, ("the file's cases and the guard's list differ", n_here, len(wanted) + 1)
    missing = sorted(map(str, wanted - REACHED))
    assert not missing, ("not reached:", missing)
    assert {f for f, row in fam.FAMILIES.items() if row[2] != "fwd"} <= {k[1] for k in REACHED if k[0] == "autograd"}
    assert {k[1] for k in REACHED if k[0] == "entry"} == set(ENTRIES)
