"""Forward mode (frames_jvp_kernel, molann_amd/csrc/molann_dev_jvp.inc; the vmap rules of _FeaturesJvp / _FeaturesTangent in
molann_amd/ann.py) past the fixed workloads of test_gpu_jvp.py, against torch.func.jvp of the float64 oracle:

1. dispatch boundaries: plans on both sides of 8 / 16 / 32 / 64 lanes per frame (jvp_group: n_items, or max(n_align, n_items)
   with position items behind an alignment), each asserting the lane count and rotation tangent last_launch_info names, at
   1, 64/G -+ 1 and one block -+ 1 frames, past one grid for every G, and a guard that every (G, rotation tangent, dtype) ran;
2. random plans: seeded draws of mixed items on 22-, 166- and 1000-atom frames, 2-5 tangents per launch equal bit for bit to
   one tangent per call;
3. far frames (tests/far_frames.py): hinge, mirror, 180-degree, 100-1000 A and noise-free frames sharing waves with near ones;
   a near frame's primal and tangent do not change when its wave-mates do; degenerate align sets give finite tangents;
4. transforms: vmap(jacfwd) per-frame Jacobians (the [B, T, N] -> [T, B N] fold), chunked vmap, in_dims=1, a batch of x with
   one tangent, x and v batched together, against the oracle and vmap(jacrev) through the reverse kernels;
5. a launch whose v and tangent output exceed 2^31 elements;
6. the C ABI's `out` pointer (the features the tangent kernel writes as well).

Frames are compared where the derivative is well conditioned: the alignment's (s2 + d s3) / s1 >= 1e-2 (plans with position
items behind an alignment), every dihedral's bond angles and, with use_angle_value, every angle at least 3 degrees from 0 / 180;
at least half of every batch must be compared.  Elsewhere tangents must be finite."""

import copy
import math
import re

import numpy as np
import pytest
import torch
from torch.autograd import forward_ad as fwAD

import far_frames as ff
import test_gpu_far_frames as fft
import test_gpu_random_backward as rb
from molann_amd import workloads as wl
from molann_amd.ann import MolANN, _PlanEntry
from oracle import molann_oracle as mo

pytestmark = pytest.mark.gpu
ANGLE, BOND, DIH, POS = wl.ANGLE, wl.BOND, wl.DIHEDRAL, wl.POSITION
REL = {torch.float32: 1e-4, torch.float64: 1e-9}
DTYPES = [torch.float32, torch.float64]
DT_IDS = ["f32", "f64"]
REACHED = set()                                            # (lanes per frame, rotation tangent, dtype) seen by part 1


# ---- helpers ---------------------------------------------------------------------------------------------------------------
def _feat(model):
    """The module whose output is the plan's features (the preprocessing layer of a MolANN)."""
    return model.preprocessing_layer if isinstance(model, MolANN) else model


def _build(case, dev, dtype):
    model = case.build(dev)
    return copy.deepcopy(model).double() if dtype == torch.float64 else model


def _ref(model):
    al = rb._align_layer(model)
    return al.ref_x.detach().cpu().double() if al is not None else None


def _oracle(case, model, features=False):
    """f(x) of the float64 oracle: the features (features=True or no head) or the model's output."""
    ref = _ref(model)
    head = rb._head64(model) if (case.mlp and not features) else None

    def f(x):
        if case.align_only:
            return mo.align_forward(x, case.align, ref)
        y = mo.preprocessing_forward(x, case.feats, case.uav, case.align, ref)
        return head(y) if head is not None else y
    return f


def _oracle_jvp(case, model, x, V, features=False):
    """(primal, [T, N, ...] tangents) of the oracle in float64 on the CPU."""
    f = _oracle(case, model, features)
    x = x.detach().cpu().double()
    outs = [torch.func.jvp(f, (x,), (v.detach().cpu().double(),)) for v in V]
    return outs[0][0].detach(), torch.stack([t for _, t in outs]).detach()


def _rotation_matters(case):
    return case.align is not None and (case.align_only or any(t == POS for t, _ in case.feats))


def _conditioning(x, align, ref):
    """Per frame (s2 + d s3) / s1 of the covariance of the centred align atoms with the reference (float64)."""
    p = x[:, align]
    p = p - p.mean(1, keepdim=True)
    H = p.transpose(1, 2) @ ref
    s = torch.linalg.svdvals(H)
    d = torch.sign(torch.linalg.det(H))
    c = (s[:, 1] + d * s[:, 2]) / s[:, 0].clamp(min=1e-300)
    return torch.where(s[:, 0] > 0, c, torch.zeros_like(c))


def _well(case, x, ref):
    """Frames whose tangent is well conditioned (see the module docstring)."""
    x = x.detach().cpu().double()
    ok = torch.ones(x.shape[0], dtype=torch.bool)
    lim = math.sin(math.radians(3.0))
    for t, idx in case.feats:
        triples = (idx[:3], idx[1:]) if t == DIH else ((idx,) if (t == ANGLE and case.uav) else ())
        for a, b, c in triples:
            u, v = x[:, a] - x[:, b], x[:, c] - x[:, b]
            ok &= torch.linalg.norm(torch.cross(u, v, dim=1), dim=1) >= lim * torch.linalg.norm(u, dim=1) * torch.linalg.norm(v, dim=1)
    if _rotation_matters(case):
        ok &= _conditioning(x, case.align, ref) >= 1e-2
    return ok


def _close(got, want, rel, what, floor=None):
    """Row-wise (per frame) bound relative to each frame's scale, floored at 1e-3 of the batch's (as test_gpu_jvp.py) and at
    `floor` [rows] when given."""
    got = got.detach().cpu().double().reshape(want.shape[0], -1)
    want = want.detach().cpu().double().reshape(want.shape[0], -1)
    assert bool(torch.isfinite(got).all()), (what, "non-finite")
    s = want.abs().amax(dim=1).clamp(min=max(1e-300, 1e-3 * float(want.abs().max())))
    if floor is not None:
        s = torch.maximum(s, floor)
    err = (got - want).abs().amax(dim=1) / s
    assert float(err.max()) <= rel, (what, float(err.max()), rel, int(err.argmax()))


def _head_terms(model, f, dfs):
    """[T, N]: per tangent and frame, the largest output of |W_L| |a'| ... |a'| |W_1| |df|, the size of the terms the head's
    chain rule sums (tanh heads).  A head output whose tangent cancels to much less than that is compared on this scale: the
    head runs on torch's float32 GEMMs, whose rounding is relative to the terms, not to their sum."""
    lins = [m for m in rb._head64(model) if isinstance(m, torch.nn.Linear)]
    out = []
    with torch.no_grad():
        for df in dfs:
            h, s = f, df.abs()
            for l, lin in enumerate(lins):
                z = lin(h)
                s = s @ lin.weight.abs().T
                if l + 1 < len(lins):
                    h = torch.tanh(z)
                    s = s * (1 - h * h)
            out.append(s.amax(dim=1))
    return torch.stack(out)


def _check_tangents(case, model, x, V, T_got, dtype, what, features=False, keep=None):
    """T_got [T, N, ...] against the oracle's on the well-conditioned frames (at least half of them); finite everywhere."""
    assert bool(torch.isfinite(T_got).all()), (what, "non-finite tangent")
    ok = _well(case, x, _ref(model)) if keep is None else keep
    n = x.shape[0]
    assert int(ok.sum()) * 2 >= n, (what, "too few well-conditioned frames", int(ok.sum()), n)
    rows = ok.nonzero().flatten()
    xs, Vs = x[rows.to(x.device)], V[:, rows.to(V.device)]
    _, want = _oracle_jvp(case, model, xs, Vs, features)
    floor = None
    if case.mlp and not features:
        f, dfs = _oracle_jvp(case, model, xs, Vs, features=True)
        floor = _head_terms(model, f, dfs)
    got = T_got[:, rows.to(T_got.device)]
    for t in range(V.shape[0]):
        _close(got[t], want[t], REL[dtype], what + ("tangent %d" % t,), None if floor is None else floor[t])


def _jvp_info(model):
    """(lanes per frame, rotation tangent, tangents) of the model's last frames_jvp launch."""
    infos = [e.plan.last_launch_info() for m in model.modules() if hasattr(m, "_plans")
             for e in m._plans().values() if isinstance(e, _PlanEntry)]
    for i in infos:
        m = re.match(r"frames_jvp(_f64)?_kernel \((\d+) lanes per frame, (\d+) tangents(, rotation tangent)?\)", i)
        if m:
            return int(m.group(2)), m.group(4) is not None, int(m.group(3))
    raise AssertionError("no frames_jvp launch in %s" % infos)


def _tangents(shape, T, seed, dev, dtype):
    g = torch.Generator().manual_seed(seed)
    return torch.randn((T,) + tuple(shape), generator=g, dtype=torch.float64).to(dev, dtype)


def _many(module, x, V):
    """J(x) V[t] for all t in one launch (vmap over torch.func.jvp)."""
    return torch.func.vmap(lambda t: torch.func.jvp(module, (x,), (t,))[1])(V)


def _frames(case, n, seed, dev, dtype, regime="near"):
    return torch.from_numpy(ff.draw(regime, case.xyz, case.align or [], n, seed)).to(dev, dtype)


# ---- 1. dispatch boundaries ------------------------------------------------------------------------------------------------
CHAIN = wl.synthetic_chain(n_atoms=120, step=1.4, seed=17)


def _invariant(n_inp, k, seed):
    """k bond / angle / dihedral items on both ends of the frame and in between (they share atoms)."""
    rng = np.random.default_rng(seed)
    feats = [(DIH, [0, 1, 2, 3]), (ANGLE, [n_inp - 1, n_inp - 2, n_inp - 3]), (BOND, [n_inp - 1, 0])][:k]
    while len(feats) < k:
        t = int(rng.choice([ANGLE, BOND, DIH]))
        s = int(rng.integers(0, n_inp - 4))
        feats.append((t, list(range(s, s + rb.NEED[t]))))   # consecutive atoms: no accidental straight angle
    return feats


def _positions(n_inp, k, seed, extra=()):
    """k position items (one- to four-atom features) and the invariant items `extra`."""
    rng = np.random.default_rng(seed)
    feats, left = list(extra), k
    while left > 0:
        m = min(left, int(rng.integers(1, 5)))
        feats.append((POS, sorted(rng.choice(n_inp, size=m, replace=False).tolist())))
        left -= m
    return feats


def _align(n_inp, k, seed):
    return sorted(np.random.default_rng(seed).choice(n_inp, size=k, replace=False).tolist())


def _boundary(name):
    """(case, lanes per frame, rotation tangent)."""
    g = lambda w: 8 if w <= 8 else 16 if w <= 16 else 32 if w <= 32 else 64
    m = re.fullmatch(r"inv(\d+)", name)
    if m:                                                  # invariant items: G by n_items (odd: behind an alignment)
        k = int(m.group(1))
        al = _align(120, 10, k) if k % 2 else None
        return rb.Case(name, CHAIN, _invariant(120, k, k), al, uav=(k % 3 == 0)), g(k), False
    m = re.fullmatch(r"pos_a(\d+)_i(\d+)", name)
    if m:                                                  # position items behind an alignment: G by max(n_align, n_items)
        na, k = int(m.group(1)), int(m.group(2))
        extra = [(DIH, [10, 11, 12, 13])] if k >= 3 else []
        return (rb.Case(name, CHAIN, _positions(120, k - len(extra), na + k, extra), _align(120, na, na), shift=(1.0, -2.0, 0.5)),
                g(max(na, k)), True)
    m = re.fullmatch(r"pos_noalign_i(\d+)", name)
    if m:                                                  # position items, no alignment: G by n_items, no rotation
        k = int(m.group(1))
        return rb.Case(name, CHAIN, _positions(120, k - 1, k, [(ANGLE, [5, 6, 7])]), None, uav=True), g(k), False
    if name == "dup_align":                                # an alignment set naming an atom twice: n_align = 11
        al = _align(120, 10, 3)
        return rb.Case(name, CHAIN, _positions(120, 3, 4), al + [al[4]]), 16, True
    if name == "permuted":                                 # a permuted subset of a larger universe
        rng = np.random.default_rng(21)
        universe = wl.synthetic_chain(n_atoms=150, step=1.4, seed=21)
        inp = rng.permutation(150)[:100].tolist()
        xyz = np.ascontiguousarray(universe[inp])
        return rb.Case(name, xyz, _positions(100, 5, 22, [(DIH, [3, 40, 7, 90])]), _align(100, 24, 23), universe=universe,
                       inp=inp), 32, True
    m = re.fullmatch(r"align(\d+)", name)
    if m:                                                  # the AlignmentLayer alone: one position item per atom
        s = fft._spec("A" + m.group(1))
        return rb.Case(name, s.xyz, align=s.align, align_only=True), 64, True
    raise KeyError(name)


BOUNDARIES = (["inv%d" % k for k in (7, 8, 9, 16, 17, 32, 33, 64, 65, 200)] +
              ["pos_a40_i2", "pos_a33_i4", "pos_a32_i4", "pos_a17_i2", "pos_a16_i16", "pos_a12_i2", "pos_a8_i8", "pos_a6_i7",
               "pos_a5_i9", "pos_a3_i17", "pos_a4_i33", "pos_a3_i64", "pos_noalign_i5", "pos_noalign_i9", "pos_noalign_i20",
               "pos_noalign_i70", "dup_align", "permuted", "align166", "align1537", "align12400"])


def _run_boundary(case, model, n, seed, dev, dtype, G, rot, regime="near"):
    x = _frames(case, n, seed, dev, dtype, regime)
    V = _tangents(x.shape, 2, seed + 1, dev, dtype)
    x0, V0 = x.clone(), V.clone()
    got = _many(_feat(model), x, V)
    torch.cuda.synchronize()
    assert _jvp_info(model) == (G, rot, 2), (case, n, _jvp_info(model))
    assert torch.equal(x, x0) and torch.equal(V, V0), (case, n, "x or v written")
    return x, V, got


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("name", BOUNDARIES)
def test_jvp_dispatch_boundaries(name, dtype, hip_device):
    case, G, rot = _boundary(name)
    model = _build(case, hip_device, dtype)
    fpb = 4 * (64 // G)                                    # frames per 256-thread block
    for n in sorted({1, 64 // G - 1, 64 // G + 1, fpb - 1, fpb + 1} - {0}):
        x, V, got = _run_boundary(case, model, n, n, hip_device, dtype, G, rot)
        _check_tangents(case, model, x, V, got, dtype, (name, n), features=True)
    REACHED.add((G, rot, dtype))


# one plan per lane count with the rotation tangent, and one without: past one grid (num_cus x 8 blocks), the grid strides
PAST_GRID = {8: ("pos_a6_i7", "inv7"), 16: ("pos_a12_i2", "pos_noalign_i9"), 32: ("pos_a17_i2", "inv17"),
             64: ("pos_a40_i2", "inv65")}


@pytest.mark.parametrize("G", sorted(PAST_GRID))
def test_jvp_past_one_grid(G, hip_device):
    cus = torch.cuda.get_device_properties(hip_device).multi_processor_count
    n = cus * 8 * 4 * (64 // G) + 3 * (64 // G) + 5
    for name in PAST_GRID[G]:
        case, g, rot = _boundary(name)
        assert g == G
        model = _build(case, hip_device, torch.float32)
        x, V, got = _run_boundary(case, model, n, 40 + G, hip_device, torch.float32, G, rot)
        tail = _many(_feat(model), x[-3000:], V[:, -3000:])
        assert torch.equal(got[:, -3000:], tail), (name, "tail of a batch past one grid")
        rows = torch.tensor(sorted(set(range(4)) | set(range(n - 4, n)) |
                                   set(np.random.default_rng(G).choice(n, size=24, replace=False).tolist())), device=hip_device)
        _check_tangents(case, model, x[rows], V[:, rows], got[:, rows], torch.float32, (name, n), features=True)


# ---- 2. random plans -------------------------------------------------------------------------------------------------------
R_SIZES = (22, 166, 1000, 22, 166, 1000, 166, 22)


def _rdraw(seed):
    """Draw `seed`: alignment on for even seeds, use_angle_value for odd, a head for seeds 1, 2, 4, 7."""
    rng = np.random.default_rng(7000 + seed)
    n_inp = R_SIZES[seed]
    xyz = wl.ALA_DIPEPTIDE_XYZ if n_inp == 22 else wl.synthetic_chain(n_atoms=n_inp, step=1.4, seed=seed)
    align = _align(n_inp, min(n_inp, int(rng.choice([3, 7, 12, 30, 60]))), seed) if seed % 2 == 0 else None
    uav, head = bool(seed % 2), seed in (1, 2, 4, 7)
    feats = [(POS, [n_inp - 1, 0])] if seed % 4 != 1 else [(BOND, [0, n_inp - 1])]
    for _ in range(int(rng.integers(3, 40))):
        t = int(rng.choice([ANGLE, BOND, DIH, POS]))
        k = rb.NEED[t] if t != POS else int(rng.integers(1, 5))
        if t == POS or rng.random() < 0.4:
            atoms = sorted(rng.choice(n_inp, size=k, replace=False).tolist())
        else:
            s = int(rng.integers(0, n_inp - k))
            atoms = list(range(s, s + k))
        feats.append((t, atoms))
    mlp = None
    if head:
        mlp = [sum(mo.feature_dim(t, len(i), uav) for t, i in feats), int(rng.integers(4, 24)), int(rng.integers(1, 6))]
    return rb.Case("J%d" % seed, xyz, feats, align, uav, mlp, "tanh")


@pytest.mark.parametrize("seed", range(len(R_SIZES)))
def test_jvp_random_plans(seed, hip_device):
    case = _rdraw(seed)
    T = 2 + seed % 4
    for dtype in DTYPES:
        model = _build(case, hip_device, dtype)
        pp = _feat(model)
        x = _frames(case, 300, 100 + seed, hip_device, dtype)
        V = _tangents(x.shape, T, seed, hip_device, dtype)
        tf = _many(pp, x, V)
        assert _jvp_info(model)[2] == T
        one = torch.stack([torch.func.jvp(pp, (x,), (V[t],))[1] for t in range(T)])
        assert torch.equal(tf, one), (case, dtype, "several tangents differ from one per launch")
        _check_tangents(case, model, x, V, tf, dtype, (case.name, dtype, "features"), features=True)
        if case.mlp:                                       # the head runs on torch's GEMMs: against the oracle only
            ty = _many(model, x, V)
            _check_tangents(case, model, x, V, ty, dtype, (case.name, dtype, "head"))


# ---- 3. far frames ---------------------------------------------------------------------------------------------------------
def _far_case(name):
    """(case, lanes per frame, rotation tangent, frames) for the far-frame families' specs and a G = 8 / 16 plan."""
    if name == "ala_g8":                                   # 8 align atoms, 4 position items: G = 8
        return rb.Case(name, wl.ALA_DIPEPTIDE_XYZ, [(POS, [1, 8, 14, 18])], [0, 4, 6, 8, 10, 14, 16, 18]), 8, True, 300
    if name == "P1":
        w = wl.get_workload("P1")
        return (rb.Case(name, w.ref_xyz, [(t, [a - 1 for a in atoms]) for t, atoms in w.features], [a - 1 for a in w.align],
                        w.use_angle_value, list(w.mlp_dims), "tanh"), 8, False, 300)
    s = fft._spec(name)
    G, n = {"ala_head": (32, 300), "ala_regs": (16, 300), "B8": (64, 300), "R2": (64, 200), "W2000": (64, 130),
            "A166": (64, 300), "A1537": (64, 130), "A12400": (64, 66)}[name]
    return rb.Case(name, s.xyz, s.feats, s.align, False, s.mlp, "tanh", align_only=s.align_only), G, True, n


FAR = ["ala_g8", "ala_regs", "ala_head", "P1", "B8", "R2", "W2000", "A166", "A1537", "A12400"]


def _invariant_cols(case):
    if case.align_only:
        return None
    cols = []
    for t, idx in case.feats:
        cols += [t != POS] * mo.feature_dim(t, len(idx), case.uav)
    return torch.tensor(cols) if any(cols) else None


@pytest.mark.parametrize("dtype", DTYPES, ids=DT_IDS)
@pytest.mark.parametrize("name", FAR)
def test_jvp_far_frames(name, dtype, hip_device):
    case, G, rot, n = _far_case(name)
    model = _build(case, hip_device, dtype)
    pp = _feat(model)
    xyz, al = case.xyz, case.align
    near = ff.draw("near", xyz, al, n, seed=len(name))
    lab = ff.interleaved(n, other=("flip180", "exact", "near"))
    mixed = ff.compose(lab, xyz, al, seed=7, base=near)
    if rot:
        assert ff.leaves_fixed_steps(mixed, xyz, al, 64).mean() > 0.25, name       # the solver's guarded loop is reached
    V = _tangents((n,) + tuple(near.shape[1:]), 2, 3, hip_device, dtype)
    V0 = V.clone()

    def run(frames):
        x = torch.from_numpy(frames).to(hip_device, dtype)
        x0 = x.clone()
        with fwAD.dual_level():
            p = fwAD.unpack_dual(pp(fwAD.make_dual(x, V[0]))).primal
        t = _many(pp, x, V)
        torch.cuda.synchronize()
        assert _jvp_info(model) == (G, rot, 2), (name, _jvp_info(model))
        assert torch.equal(x, x0) and torch.equal(V, V0), (name, "x or v written")
        return x, p, t

    _, p_near, t_near = run(near)
    x, p, t = run(mixed)
    near_rows = torch.tensor([i for i in range(n) if lab[i] == "near"], device=hip_device)
    assert torch.equal(p[near_rows], p_near[near_rows]), (name, "a near frame's primal changed with its wave-mates")
    assert torch.equal(t[:, near_rows], t_near[:, near_rows]), (name, "a near frame's tangent changed with its wave-mates")
    _check_tangents(case, model, x, V, t, dtype, (name, "mixed"), features=True)
    if case.mlp:
        _check_tangents(case, model, x, V, _many(model, x, V), dtype, (name, "mixed, head"))
    if not rot:
        return
    # degenerate align sets (nearly collinear, one point): finite tangents in every column; invariant columns as the oracle's
    dlab = ["degenerate" if i % 3 == 1 else "near" for i in range(n)]
    xd, pd, td = run(ff.compose(dlab, xyz, al, seed=31, base=near))
    rows = torch.tensor([i for i in range(n) if dlab[i] == "degenerate"], device=hip_device)
    nrows = torch.tensor([i for i in range(n) if dlab[i] == "near"], device=hip_device)
    assert torch.equal(td[:, nrows], t_near[:, nrows]) and torch.equal(pd[nrows], p_near[nrows]), (name, "degenerate batch")
    inv = _invariant_cols(case)
    pos = torch.ones(td.shape[-1], dtype=torch.bool) if inv is None else ~inv
    assert bool(torch.isfinite(td[..., pos.to(td.device)]).all()), (name, "degenerate: non-finite position tangent")
    if inv is not None:
        # an item whose atoms sit on the collapsed align set has no value in the oracle either: finite wherever the oracle's
        # tangent is, and equal to it away from angle / dihedral poles
        xs = xd[rows]
        _, want = _oracle_jvp(case, model, xs, V[:, rows], features=True)
        got = td[:, rows].cpu().double()[..., inv]
        want = want[..., inv]
        fin = torch.isfinite(want)
        assert bool(torch.isfinite(got[fin]).all()), (name, "degenerate: non-finite invariant tangent")
        k = _well(rb.Case(name, xyz, case.feats, None, case.uav), xs, None) & fin.all(0).all(1)
        for i in range(V.shape[0]):
            if bool(k.any()):
                _close(got[i][k], want[i][k], REL[dtype], (name, "degenerate: invariant columns"))


# ---- 4. transforms ---------------------------------------------------------------------------------------------------------
def _transform_case(name):
    if name == "C3":                                       # invariant items behind an alignment, head [6, 32, 8]
        w = wl.get_workload("C3")
        return rb.Case(name, w.ref_xyz, [(t, [a - 1 for a in atoms]) for t, atoms in w.features], [a - 1 for a in w.align],
                       w.use_angle_value, list(w.mlp_dims), "tanh")
    s = fft._spec("ala_head")                              # positions + a dihedral behind the 22-atom alignment, head [26, 16, 4]
    return rb.Case(name, s.xyz, s.feats, s.align, False, s.mlp, "tanh")


@pytest.mark.parametrize("name", ["C3", "ala_head"])
def test_jvp_transforms(name, hip_device):
    case = _transform_case(name)
    dev, dtype = hip_device, torch.float32
    model = _build(case, dev, dtype)
    pp = _feat(model)
    n_inp = len(case.xyz)
    x = _frames(case, 1000, 5, dev, dtype)
    keep = _well(case, x, _ref(model))
    # per-frame Jacobians: vmap over frames of jacfwd (vmap over the basis): v arrives as [B, T, 1, n, 3]
    one = lambda a: model(a[None])[0]
    J = torch.func.vmap(torch.func.jacfwd(one))(x)                     # [N, d_out, n_inp, 3]
    assert _jvp_info(model)[2] == 3 * n_inp
    d = J.shape[1]
    basis = torch.eye(3 * n_inp, dtype=torch.float64).view(3 * n_inp, 1, n_inp, 3).expand(-1, x.shape[0], -1, -1)
    _, Jw = _oracle_jvp(case, model, x, basis)                         # [3 n_inp, N, d_out]
    Jw = Jw.permute(1, 2, 0).reshape(x.shape[0], d, n_inp, 3)
    k = keep.nonzero().flatten()
    assert len(k) * 2 >= x.shape[0]
    _close(J[k.to(dev)].reshape(len(k), -1), Jw[k].reshape(len(k), -1), 1e-4, (name, "vmap(jacfwd) vs oracle"))
    Jr = torch.func.vmap(torch.func.jacrev(one))(x)                    # the reverse kernels
    _close(J[k.to(dev)].reshape(len(k), -1), Jr[k.to(dev)].reshape(len(k), -1).double(), 1e-4, (name, "vmap(jacfwd) vs vmap(jacrev)"))
    # the tangent basis through vmap(jvp), chunked and not: bit for bit
    xs = x[:200]
    E = torch.eye(3 * n_inp, dtype=dtype, device=dev).view(3 * n_inp, 1, n_inp, 3).expand(-1, 200, -1, -1)
    f = lambda t: torch.func.jvp(pp, (xs,), (t,))[1]
    full = torch.func.vmap(f)(E)
    for chunk in (1, 7, 64):
        assert torch.equal(torch.func.vmap(f, chunk_size=chunk)(E), full), (name, "chunk_size", chunk)
    Jf = torch.func.vmap(torch.func.jacfwd(lambda a: pp(a[None])[0]))(xs)            # [200, d_feat, n_inp, 3]
    assert torch.equal(Jf, full.permute(1, 2, 0).reshape(Jf.shape)), (name, "vmap(jacfwd) vs vmap(jvp) over the basis")
    # in_dims=1 on v
    V = _tangents(xs.shape, 4, 9, dev, dtype)
    tv = torch.func.vmap(f)(V)
    assert torch.equal(torch.func.vmap(f, in_dims=1)(V.movedim(0, 1).contiguous()), tv), (name, "in_dims=1")
    assert torch.equal(torch.func.vmap(f, in_dims=1)(V.movedim(0, 1)), tv), (name, "in_dims=1, strided")
    # a batch of x with one unbatched tangent, and x and v batched together: B x 50 frames folded into one launch
    X = x[200:400].reshape(4, 50, n_inp, 3)
    v1 = V[0, :50]
    got = torch.func.vmap(lambda a: torch.func.jvp(pp, (a,), (v1,))[1])(X)
    sep = torch.stack([torch.func.jvp(pp, (X[b],), (v1,))[1] for b in range(4)])
    assert torch.equal(got, sep), (name, "vmap over x, v unbatched")
    VB = V[:, :50]
    got2 = torch.func.vmap(lambda a, t: torch.func.jvp(pp, (a,), (t,))[1])(X, VB)
    sep2 = torch.stack([torch.func.jvp(pp, (X[b],), (VB[b],))[1] for b in range(4)])
    assert torch.equal(got2, sep2), (name, "vmap over x and v")
    # and through the model's head against the oracle
    Xf, kf = X.reshape(200, n_inp, 3), keep[200:400]
    gy = torch.func.vmap(lambda a, t: torch.func.jvp(model, (a,), (t,))[1])(X, VB)
    _check_tangents(case, model, Xf, VB.reshape(1, 200, n_inp, 3), gy.reshape(1, 200, -1), dtype, (name, "vmap over x and v"),
                    keep=kf)
    gx = torch.func.vmap(lambda a: torch.func.jvp(model, (a,), (v1,))[1])(X)
    _check_tangents(case, model, Xf, v1.repeat(4, 1, 1)[None], gx.reshape(1, 200, -1), dtype, (name, "vmap over x"), keep=kf)


# ---- 5. offsets past 2^31 elements -----------------------------------------------------------------------------------------
def test_jvp_offsets_past_2_31_elements(hip_device):
    """vmap(jacfwd) of 520 000 frames of the 22-atom all-positions plan: 66 tangents x 520 000 frames x 66 values, more than
    2^31 elements of v and of the tangent output in one launch."""
    free, _ = torch.cuda.mem_get_info(hip_device)
    if free < 64 * 2 ** 30:
        pytest.skip("needs 64 GB of free device memory, %.1f GB free" % (free / 2 ** 30))
    s = fft._spec("ala_pos")
    case = rb.Case("ala_pos", s.xyz, s.feats, s.align)
    pp = case.build(hip_device)
    n = 520_000
    assert 66 * n * 66 > 2 ** 31
    g = torch.Generator(device=hip_device)
    g.manual_seed(3)
    ref = torch.from_numpy(case.xyz).to(hip_device)
    x = ref + 0.2 * torch.randn((n, 22, 3), generator=g, device=hip_device)
    f = torch.func.vmap(torch.func.jacfwd(lambda a: pp(a[None])[0]))
    J = f(x)
    torch.cuda.synchronize()
    assert _jvp_info(pp) == (32, True, 66), _jvp_info(pp)
    head, tail = J[:2000, :, 0, 0].clone(), J[-2000:, :, 0, 0].clone()      # the first tangent
    head_l, tail_l = J[:2000, :, -1, -1].clone(), J[-2000:, :, -1, -1].clone()   # the last
    del J
    Jh, Jt = f(x[:2000]), f(x[-2000:])
    assert torch.equal(head, Jh[:, :, 0, 0]) and torch.equal(head_l, Jh[:, :, -1, -1]), "first 2000 frames"
    assert torch.equal(tail, Jt[:, :, 0, 0]) and torch.equal(tail_l, Jt[:, :, -1, -1]), "last 2000 frames"


# ---- 6. the C ABI's out pointer --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["inv33", "pos_a12_i2", "align166"])
def test_jvp_out_pointer_receives_the_features(name, hip_device):
    case, G, rot = _boundary(name)
    for dtype in DTYPES:
        model = _build(case, hip_device, dtype)
        pp = _feat(model)
        x = _frames(case, 77, 8, hip_device, dtype)
        V = _tangents(x.shape, 3, 4, hip_device, dtype)
        want_t = _many(pp, x, V)                           # (also syncs the plan's reference)
        plan = [e for m in pp.modules() if hasattr(m, "_plans") for e in m._plans().values() if isinstance(e, _PlanEntry)][0].plan
        out = torch.full((77, plan.feature_dim), float("nan"), dtype=dtype, device=hip_device)
        tout = torch.full((3, 77, plan.feature_dim), float("nan"), dtype=dtype, device=hip_device)
        f64 = torch.empty((77, plan.feature_dim), dtype=torch.float64, device=hip_device)
        with torch.cuda.device(hip_device):
            (plan.features_jvp_f64 if dtype == torch.float64 else plan.features_jvp)(x, V, out, tout)
            torch.cuda.synchronize()
            assert _jvp_info(pp) == (G, rot, 3)
            plan.features_f64(x.double(), f64)             # the same plan (and packed reference) in float64
        torch.cuda.synchronize()
        assert torch.equal(tout, want_t.reshape(tout.shape)), (name, dtype, "tangents with `out` given")
        want = f64.cpu()
        got = out.cpu().double()
        scale = float(want.abs().max())
        if dtype == torch.float64:
            err = float((got - want).abs().max())
            assert err <= 1e-12 * scale, (name, err)
        else:                                              # within one float32 rounding of the float64 features
            bad = (got - want).abs() > want.abs() * 2.0 ** -24 * (1 + 1e-6) + 1e-13 * scale
            assert not bool(bad.any()), (name, int(bad.sum()), float((got - want).abs().max()))


# ---- the guard ---------------------------------------------------------------------------------------------------------------
def test_every_lane_group_was_reached(request, hip_device):
    """Every (lanes per frame, rotation tangent, dtype) must have been run by part 1; recorded as its tests pass, so this guard
    needs all of them in the same session."""
    here = {item.name for item in request.session.items if item.module is request.module}
    wanted = {"test_jvp_dispatch_boundaries[%s-%s]" % (b, d) for b in BOUNDARIES for d in DT_IDS}
    if not wanted <= here:
        pytest.skip("the coverage guard needs every boundary test in this session: %d not selected" % len(wanted - here))
    missing = [(G, rot, d) for G in (8, 16, 32, 64) for rot in (False, True) for d in DTYPES if (G, rot, d) not in REACHED]
    assert not missing, ("not reached:", missing)
