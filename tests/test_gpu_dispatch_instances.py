"""Every instance of the mid- and large-frame kernels' dispatch ladders, at both ends of the range of sizes that selects it.

tests/dispatch_instances.py lists the instances (held against the C++ macro lists by tests/test_dispatch_instances_host.py) and, for
each, the first and the last selecting size - for the register kernels one atom in the last four register slots and the exactly-full
frame, for the ring one window in the last LDS-DMA instruction and one short of 64 - with the way to reach it.  One case per
(instance, edge): the case first holds last_launch_info against the instance's name, then the kernel's output against the float64
oracle on the CPU, at one frame and at a batch that gives persistent blocks a second and a third frame (a 32-frame base repeated,
one fresh frame last: the base, the last frame and the rows served as second and third frames against the oracle, the repeats bit
for bit against the base).  Inputs and outputs lie between NaN guard bands (tests/placement.py): the input is never written and
nothing is stored outside the output, in particular behind the last frame at the exactly-full sizes.  The last test holds that
every instance was named in at least two cases.

The large batch runs on the grid the launch itself reports, not on one capped with MOLANN_WAVE_BPC=1: that switch is read once per
process, so a case inside the suite's process cannot set it.  The batch is 2 x grid + 3 turns' worth of frames rather than grid + 3,
which alone gives no block a third turn: 515 frames at 12 288 atoms (150 MB), up to 262 147 at 60 atoms.  A case takes under a
second on an MI355X, the ones that build a plan-specialised kernel (molann_group_vjp) or start the child process a few.

Bounds are those of the tests that were there: test_large_frame_alignment_in_registers (alignment forward),
test_dense_alignment_gradient (dense gradient), test_gpu_mid_frames.py (ring and wave features), test_backward_dispatch_boundaries and
test_frames_per_round (group backward, values + vjp)."""

import collections
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:                                    # (this file is also the program of the MOLANN_WAVE_PRE cases' child process)
    sys.path.insert(0, ROOT)

import dispatch_instances as di                             # noqa: E402
from molann_amd import _capi, workloads as wl               # noqa: E402
from oracle import molann_oracle as mo                     # noqa: E402
from placement import Arena                                 # noqa: E402

pytestmark = pytest.mark.gpu
ANGLE, BOND, DIH, POS = wl.ANGLE, wl.BOND, wl.DIHEDRAL, wl.POSITION
BASE = 32                                                   # frames of the repeated base: a multiple of every round's size
REACHED = collections.Counter()                             # instance name -> cases that named it
WORST = {}                                                  # ladder -> worst error / bound of its cases


def _ids(ladder):
    return [di.case_id(i, e) for i, e in di.cases(ladder)]


@pytest.fixture(scope="module")
def arena(hip_device):
    yield Arena(hip_device, capacity=640 << 20)              # (freed with the fixture, when the module's last test has run)


def _note(ladder, instance, info, ratio):
    assert instance.name in info, (instance.name, info)
    WORST[ladder] = max(WORST.get(ladder, 0.0), ratio)


def _chain(n_inp, seed):
    xyz = np.cumsum(np.random.default_rng(seed).normal(size=(n_inp, 3)) * 0.9, axis=0).astype(np.float32)
    return xyz - xyz.mean(axis=0, keepdims=True)


def _near_frames(xyz, n, g):
    """Frames near the reference with a random rigid motion, as test_large_frame_alignment_in_registers draws them."""
    x = torch.from_numpy(xyz).unsqueeze(0) + 0.2 * torch.randn((n,) + xyz.shape, generator=g)
    q = torch.randn((n, 4), generator=g)
    q = q / q.norm(dim=1, keepdim=True)
    return (torch.einsum("nij,nkj->nki", wl.quaternion_to_matrix(q), x) + 2.0 * torch.randn((n, 1, 3), generator=g)).float().contiguous()


def _grid(info):
    return int(re.search(r"grid=(\d+)", info).group(1))


def _batch(base, fresh, n, dev):
    """n frames on the device: the base repeated, the fresh frame last."""
    reps = -(-n // base.shape[0])
    x = base.to(dev).repeat((reps,) + (1,) * (base.dim() - 1))[:n].contiguous()
    x[n - 1] = fresh.to(dev)[0]
    return x


def _rows(n, grid, unit):
    """Rows held against the oracle: the base, the rows behind the last whole repeat (the last frame among them), and the first frames of the second and third turn of blocks 0 to 2."""
    rows = set(range(min(BASE, n))) | set(range((n - 1) // BASE * BASE, n))     # ... and what follows the last whole repeat: the short last round
    for turn in (1, 2):
        for k in range(3):
            r = (turn * grid + k) * unit
            if r < n:
                rows.add(r)
    return sorted(rows)


def _want_rows(rows, n, want_base, want_fresh):
    return torch.stack([want_fresh[0] if r == n - 1 else want_base[r % BASE] for r in rows])


def _repeats_equal_base(out, n):
    full = (n - 1) // BASE                                  # whole repeats in front of the fresh last frame
    if full >= 2:
        body = out[:full * BASE].view((full, BASE) + tuple(out.shape[1:]))
        assert bool((body == body[:1]).all()), "a repeat of the base differs from the base"


def _two_batches(run, carve, ar, base_in, fresh_in, unit, full_grid_of, want_base, want_fresh, bound, what, exact=True):
    """The case at one frame and at 2 grid + 3 frames (`unit`: frames a block takes per turn).  `carve(n, inputs, off)` places the
    inputs and the outputs in the arena, `off` floats past a 256-byte boundary, and returns (args, out); `run(*args)` launches and
    returns last_launch_info; `full_grid_of(info)`: blocks of a launch that fills the device, from the one-frame launch's info - held
    against the grid the large launch reports (`exact=False`: an upper bound; the rows follow the reported grid).  Several outputs:
    `out`, `want_base`, `want_fresh` and `bound` are tuples.  Returns the worst error / bound and the large launch's info."""
    many = isinstance(bound, tuple)
    wants_b, wants_f, bounds = (want_base, want_fresh, bound) if many else ((want_base,), (want_fresh,), (bound,))
    worst, info1 = 0.0, None
    for n in (1, None):
        if n is None:
            cap = full_grid_of(info1)
            n = unit * 2 * cap + 3
        ar.reset()
        inputs = [_batch(b, f, n, ar.device) for b, f in zip(base_in, fresh_in)] if n > 1 else [b[:1].to(ar.device) for b in base_in]
        args, outs = carve(n, inputs, 0 if n > 1 else 1)
        outs = outs if many else (outs,)
        info = run(*args)
        torch.cuda.synchronize()
        if n == 1:
            info1 = info
            rows = [0]
        else:
            grid = _grid(info)
            assert grid == cap if exact else grid <= cap, (cap, info)     # every block has a second turn, blocks 0 to 2 a third
            rows = _rows(n, grid, unit)
        assert ar.inputs_changed() == [], (what, n, ar.inputs_changed())
        assert ar.check() == [], (what, n, ar.check())
        for out, wb, wf, bd in zip(outs, wants_b, wants_f, bounds):
            if n > 1:
                _repeats_equal_base(out, n)
            want = _want_rows(rows, n, wb, wf) if n > 1 else wb[:1]
            got = out[torch.tensor(rows, device=out.device)].cpu().double()
            assert bool(torch.isfinite(got).all()), (what, n, "a row of the output was not written")
            err = float((got - want).abs().max())
            print("%s n=%d: err %.3g bound %.3g (%s)" % (what, n, err, bd, info))
            assert err <= bd, (what, n, err, bd, info)
            worst = max(worst, err / bd)
    return worst, info


def _align_set(xyz, n_al, rng):
    """n_al alignment atoms, redrawn until the set is well conditioned: the rotation's derivative divides by sums of the covariance's
    singular values, and three nearly collinear atoms leave the oracle's own float32 run far outside the gradient's bound."""
    n_inp = len(xyz)
    if n_al > n_inp:
        return [i % n_inp for i in range(n_al)]             # every atom named twice or more
    for _ in range(200):
        align = sorted(rng.choice(n_inp, size=n_al, replace=False).tolist())
        r = xyz[align].astype(np.float64)
        r = r - r.mean(0)
        sv = np.linalg.svd(r.T @ r, compute_uv=False)
        if n_al > 8 or sv[1] >= 0.1 * sv[0]:                # (a large set has the chain's own shape: taken as drawn)
            return align
    raise AssertionError("no well-conditioned set of %d atoms" % n_al)


def _blocks_per_cu_grid(hip_device):
    cus = torch.cuda.get_device_properties(hip_device).multi_processor_count
    return lambda info: cus * int(re.search(r"(\d+) blocks per CU", info).group(1))


# ---- AlignmentLayer.forward: frames_align_regs_kernel, frames_align_batch_kernel ------------------------------------------------
def _align_forward_case(instance, edge, hip_device, arena, monkeypatch):
    n_inp = edge.size
    for k, v in edge.env.items():
        monkeypatch.setenv(k, v)
    rng = np.random.default_rng(n_inp)
    xyz = _chain(n_inp, n_inp)
    g = torch.Generator().manual_seed(n_inp)
    base, fresh = _near_frames(xyz, BASE, g), _near_frames(xyz, 1, g)
    unit = instance.args[1] if instance.ladder == "ALIGN_BATCH_CASE" else 1
    worst = 0.0
    for n_al in di.align_set_sizes(instance, edge):
        align = _align_set(xyz, n_al, rng)
        ref_x = mo.center_reference(torch.from_numpy(xyz[align])).double()
        both = torch.cat([base, fresh])
        want = mo.align_forward(both.double(), align, ref_x)
        own = float((mo.align_forward(both, align, ref_x.float()).double() - want).abs().max())     # the reference's arithmetic in fp32
        bound = max(1e-5, 2.0 * own)
        with torch.cuda.device(hip_device):
            plan = _capi.Plan(n_inp, align_idx=align, ref_x=torch.from_numpy(xyz[align]))

            def carve(n, inputs, off):
                x = arena.carve("x", (n, n_inp, 3), torch.float32, off, data=inputs[0])
                out = arena.carve("out", (n, n_inp, 3), torch.float32, (off * 3) % 4)
                return (x, out), out

            def run(x, out):
                plan.align(x, out)
                return plan.last_launch_info()
            ratio, info = _two_batches(run, carve, arena, [base], [fresh], unit, _blocks_per_cu_grid(hip_device), want[:BASE], want[BASE:],
                                       bound, "%s %d atoms, %d alignment entries" % (instance.name, n_inp, n_al))
        _note(instance.ladder, instance, info, ratio)
        worst = max(worst, ratio)
    REACHED[instance.name] += 1
    return worst


@pytest.mark.parametrize("instance,edge", di.cases("ALIGN_REGS_CASE"), ids=_ids("ALIGN_REGS_CASE"))
def test_alignment_in_registers(instance, edge, hip_device, arena, monkeypatch):
    _align_forward_case(instance, edge, hip_device, arena, monkeypatch)


@pytest.mark.parametrize("instance,edge", di.cases("ALIGN_BATCH_CASE"), ids=_ids("ALIGN_BATCH_CASE"))
def test_alignment_in_rounds(instance, edge, hip_device, arena, monkeypatch):
    _align_forward_case(instance, edge, hip_device, arena, monkeypatch)


# ---- the dense gradient of AlignmentLayer.forward: frames_align_bwd_regs_kernel --------------------------------------------------
@pytest.mark.parametrize("instance,edge", di.cases("ALIGN_BWD_CASE"), ids=_ids("ALIGN_BWD_CASE"))
def test_dense_alignment_gradient_in_registers(instance, edge, hip_device, arena):
    """dL/dx of L = sum(y * G), y the aligned frame, against float64 autograd through the oracle within 2e-4 of the gradient's scale
    (test_dense_alignment_gradient); the plan is the one AlignmentLayer.forward makes under autograd, one position item per atom."""
    n_inp = edge.size
    rng = np.random.default_rng(n_inp + 1)
    xyz = _chain(n_inp, n_inp + 1)
    g = torch.Generator().manual_seed(n_inp + 1)
    base, fresh = _near_frames(xyz, BASE, g), _near_frames(xyz, 1, g)
    G_base, G_fresh = torch.randn(base.shape, generator=g), torch.randn(fresh.shape, generator=g)
    for n_al in di.align_set_sizes(instance, edge):
        align = _align_set(xyz, n_al, rng)
        ref_x = mo.center_reference(torch.from_numpy(xyz[align])).double()
        xx = torch.cat([base, fresh]).double().requires_grad_(True)
        (mo.align_forward(xx, align, ref_x) * torch.cat([G_base, G_fresh]).double()).sum().backward()
        want = xx.grad
        bound = 2e-4 * float(want.abs().max())
        with torch.cuda.device(hip_device):
            plan = _capi.Plan(n_inp, align_idx=align, ref_x=torch.from_numpy(xyz[align]), features=[(_capi.FEAT_POSITION, list(range(n_inp)))])

            def carve(n, inputs, off):
                x = arena.carve("x", (n, n_inp, 3), torch.float32, off, data=inputs[0])
                G = arena.carve("G", (n, n_inp, 3), torch.float32, (off * 2) % 4, data=inputs[1])
                gx = arena.carve("gx", (n, n_inp, 3), torch.float32, (off * 3) % 4)
                return (x, G, gx), gx

            def run(x, G, gx):
                plan.backward(x, G, gx, None)
                return plan.last_launch_info()
            ratio, info = _two_batches(run, carve, arena, [base, G_base], [fresh, G_fresh], 1, _blocks_per_cu_grid(hip_device),
                                       want[:BASE], want[BASE:], bound, "%s %d atoms, %d alignment atoms" % (instance.name, n_inp, n_al))
        _note(instance.ladder, instance, info, ratio)
    REACHED[instance.name] += 1


# ---- features of frames the lane kernels refuse: frames_ring_kernel, frames_wave_kernel -----------------------------------------
def _ring_items(touched):
    """Items on the touched atoms, every one of them in at least one: bonds over neighbouring pairs, and a dihedral, an angle and two
    positions on the first and the last - the atoms of the image's first and last window, the last of them the frame's last atom."""
    t = list(touched)
    feats = [(DIH, t[:4]), (ANGLE, t[-3:]), (POS, [t[0], t[-1]]), (BOND, [t[0], t[-1]])]
    feats += [(BOND, [t[k], t[k + 1]]) for k in range(0, len(t) - 1, 2)]
    if len(t) % 2:
        feats.append((BOND, [t[-2], t[-1]]))
    return feats


def _features_case(what, name, n_inp, feats, align, env, hip_device, arena, monkeypatch, n_win=None, seed=0):
    """Features of one plan through molann_features_f32 against mo.preprocessing_forward within 1e-5 of the features' scale."""
    for k in ("MOLANN_RING_BATCH", "MOLANN_NO_RING"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    xyz = _chain(n_inp, 7 * n_inp + seed)
    g = torch.Generator().manual_seed(n_inp + seed)
    base, fresh = _near_frames(xyz, BASE, g), _near_frames(xyz, 1, g)
    ref_x = mo.center_reference(torch.from_numpy(xyz[align])).double() if align else None
    want = mo.preprocessing_forward(torch.cat([base, fresh]).double(), feats, False, align, ref_x)
    bound = 1e-5 * max(1.0, float(want.abs().max()))
    cus = torch.cuda.get_device_properties(hip_device).multi_processor_count
    m = re.search(r"B=(\d+)", name) if "ring" in name else None
    unit = int(m.group(1)) if m else 1
    with torch.cuda.device(hip_device):
        plan = _capi.Plan(n_inp, align_idx=align, ref_x=torch.from_numpy(xyz[align]) if align else None, features=feats)
        d = plan.feature_dim
        assert d == want.shape[1]

        def carve(n, inputs, off):
            x = arena.carve("x", (n, n_inp, 3), torch.float32, off, data=inputs[0])
            out = arena.carve("out", (n, d), torch.float32, (off * 3) % 4)
            return (x, out), out

        def run(x, out):
            plan.features(x, out)
            info = plan.last_launch_info()
            assert name in info, (name, info)
            if n_win is not None:
                assert "%d windows)" % n_win in info, (n_win, info)
            return info
        # the ring: one block per CU; the gather kernel: four frames per block, what its launch reports for a batch that fills the device
        full = (lambda info: cus) if "ring" in name else (lambda info: 8 * cus)
        if "ring" not in name:
            unit = 4
        return _two_batches(run, carve, arena, [base], [fresh], unit, full, want[:BASE], want[BASE:], bound, what)


@pytest.mark.parametrize("instance,edge", di.cases("LAUNCH_RING"), ids=_ids("LAUNCH_RING"))
def test_ring_window_counts(instance, edge, hip_device, arena, monkeypatch):
    """A plan whose compact image has exactly the edge's window count; behind an alignment, and without one where that selects the same instance."""
    nd, nb = instance.args
    n_inp, touched = di.ring_plan(edge.size)
    feats = _ring_items(touched)
    assert len(di.compact_windows(touched, n_inp)) == edge.size
    align = touched[::max(1, len(touched) // 40)][:40]
    routes = [(align, edge.env)]
    batch = int(edge.env["MOLANN_RING_BATCH"]) if "MOLANN_RING_BATCH" in edge.env else None
    if di.ring_nb(nd, 0, batch) == nb:
        routes.append((None, edge.env))
    for al, env in routes:
        ratio, info = _features_case("%s, %d windows, %s" % (instance.name, edge.size, "aligned" if al else "no alignment"), instance.name,
                                     n_inp, feats, al, env, hip_device, arena, monkeypatch, n_win=edge.size)
        _note(instance.ladder, instance, info, ratio)
    REACHED[instance.name] += 1


def _items(n_inp, k, seed):
    """k items of all four types on a chain of n_inp atoms: the frame's ends first, then random atoms."""
    rng = np.random.default_rng(seed)
    feats = [(BOND, [n_inp - 1, 0]), (ANGLE, [n_inp - 1, n_inp - 2, n_inp - 3]), (DIH, [0, 1, 2, 3])][:k]
    need = {BOND: 2, ANGLE: 3, DIH: 4, POS: 1}
    order = (BOND, ANGLE, POS, DIH)
    while len(feats) < k:
        t = order[len(feats) % 4]
        a = int(rng.integers(0, n_inp - 4))
        feats.append((t, list(range(a, a + need[t]))))      # neighbours along the chain: well-conditioned angles
    return feats


SMALL_ALIGN = [a for a in range(di.SMALL_LADDER_ATOMS) if a % 3]     # 40 atoms of the 60: more than 32 touched, no lane plan
assert len(SMALL_ALIGN) == 40


_CHILD = {}


def _wave_pre_child(env):
    """MOLANN_WAVE_PRE is read once per process: both of its cases run in one child process started with it."""
    if "out" not in _CHILD:
        e = dict(os.environ)
        e.update(env)
        cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), "wave-pre-child"]
        r = subprocess.run(cmd, env=e, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
        _CHILD["out"] = (r.returncode, r.stdout)
    return _CHILD["out"]


@pytest.mark.parametrize("instance,edge", di.cases("LAUNCH_WAVE"), ids=_ids("LAUNCH_WAVE"))
def test_wave_kernel_item_rounds(instance, edge, hip_device, arena, monkeypatch):
    if "MOLANN_WAVE_PRE" in edge.env:
        code, out = _wave_pre_child(edge.env)
        assert code == 0, out
        m = re.search(r"^case %d: ratio ([0-9.e+-]+) info (.*)$" % edge.size, out, re.M)
        assert m and instance.name in m.group(2), out
        print(m.group(0))
        WORST[instance.ladder] = max(WORST.get(instance.ladder, 0.0), float(m.group(1)))
    else:
        n_inp = di.SMALL_LADDER_ATOMS
        ratio, info = _features_case("%s, %d items" % (instance.name, edge.size), instance.name, n_inp, _items(n_inp, edge.size, edge.size),
                                     SMALL_ALIGN, edge.env, hip_device, arena, monkeypatch, seed=edge.size)
        _note(instance.ladder, instance, info, ratio)
    REACHED[instance.name] += 1


def _vjp_reference(feats, xyz, seed):
    """Frames, cotangent rows and, by float64 autograd through the oracle, y and dL/dx of L = sum(y * G): the base and the fresh frame."""
    g = torch.Generator().manual_seed(seed)
    x = torch.cat([_near_frames(xyz, BASE, g), _near_frames(xyz, 1, g)])
    ref_x = mo.center_reference(torch.from_numpy(xyz[SMALL_ALIGN])).double()
    xx = x.double().requires_grad_(True)
    y = mo.preprocessing_forward(xx, feats, False, SMALL_ALIGN, ref_x)
    G = torch.randn(y.shape, generator=g)
    (y * G.double()).sum().backward()
    return x, G, y.detach(), xx.grad


def _small_plan(feats, xyz):
    return _capi.Plan(len(xyz), align_idx=SMALL_ALIGN, ref_x=torch.from_numpy(xyz[SMALL_ALIGN]), features=feats)


@pytest.mark.parametrize("instance,edge", di.cases("LAUNCH_GROUP_BWD"), ids=_ids("LAUNCH_GROUP_BWD"))
def test_group_backward_item_counts(instance, edge, hip_device, arena):
    """dL/dx of a features plan through molann_backward_f32 within 2e-4 of the gradient's scale (test_backward_dispatch_boundaries).  A
    block's four waves take a round of B frames each per turn; its blocks per CU follow from the LDS the one-frame launch reports."""
    n_inp, b = di.SMALL_LADDER_ATOMS, instance.args[0]
    xyz = _chain(n_inp, 11)
    feats = _items(n_inp, edge.size, edge.size)
    x, G, _, gx_want = _vjp_reference(feats, xyz, 100 + edge.size)
    bound = 2e-4 * max(1e-6, float(gx_want.abs().max()))
    cus = torch.cuda.get_device_properties(hip_device).multi_processor_count
    with torch.cuda.device(hip_device):
        plan = _small_plan(feats, xyz)
        d = plan.feature_dim

        def carve(n, inputs, off):
            xa = arena.carve("x", (n, n_inp, 3), torch.float32, off, data=inputs[0])
            Ga = arena.carve("G", (n, d), torch.float32, (off * 2) % 4, data=inputs[1])
            gx = arena.carve("gx", (n, n_inp, 3), torch.float32, (off * 3) % 4)
            return (xa, Ga, gx), gx

        def run(xa, Ga, gx):
            plan.backward(xa, Ga, gx, None)
            return plan.last_launch_info()
        full = lambda info: cus * max(1, min(8, 160 * 1024 // int(re.search(r"lds=(\d+)", info).group(1))))     # noqa: E731
        ratio, info = _two_batches(run, carve, arena, [x[:BASE], G[:BASE]], [x[BASE:], G[BASE:]], 4 * b, full, gx_want[:BASE], gx_want[BASE:],
                                   bound, "%s, %d items" % (instance.name, edge.size))
    _note(instance.ladder, instance, info, ratio)
    REACHED[instance.name] += 1


@pytest.mark.parametrize("instance,edge", di.cases("molann_group_vjp"), ids=_ids("molann_group_vjp"))
def test_group_vjp_item_counts(instance, edge, hip_device, arena):
    """The features and dL/dx in one launch (molann_value_and_vjp_f32) within 2e-5 of the features' and 2e-4 of the gradient's scale
    (test_frames_per_round).  A block takes a 64-frame tile per turn; the blocks per CU are the kernel's occupancy, which the launch
    info does not print: the batch is sized by its upper bound (the LDS, 32 waves per CU) and the rows follow the reported grid."""
    n_inp = di.SMALL_LADDER_ATOMS
    xyz = _chain(n_inp, 12)
    feats = _items(n_inp, edge.size, edge.size + 1)
    x, G, y_want, gx_want = _vjp_reference(feats, xyz, 200 + edge.size)
    bounds = (2e-5 * max(1.0, float(y_want.abs().max())), 2e-4 * max(1e-6, float(gx_want.abs().max())))
    cus = torch.cuda.get_device_properties(hip_device).multi_processor_count
    with torch.cuda.device(hip_device):
        plan = _small_plan(feats, xyz)
        assert plan.supports_value_and_vjp()
        d = plan.feature_dim

        def carve(n, inputs, off):
            xa = arena.carve("x", (n, n_inp, 3), torch.float32, off, data=inputs[0])
            Ga = arena.carve("G", (n, d), torch.float32, (off * 2) % 4, data=inputs[1])
            y = arena.carve("y", (n, d), torch.float32, (off * 3) % 4)
            gx = arena.carve("gx", (n, n_inp, 3), torch.float32, off)
            return (xa, Ga, y, gx), (y, gx)

        def run(xa, Ga, y, gx):
            plan.value_and_vjp(xa, Ga, y, gx)
            return plan.last_launch_info()

        def cap(info):
            m = re.search(r"(\d+) waves per 64-frame tile\) grid=\d+ block=\d+ lds=(\d+)", info)
            return cus * min(160 * 1024 // int(m.group(2)), 32 // max(1, int(m.group(1)) // 2))
        ratio, info = _two_batches(run, carve, arena, [x[:BASE], G[:BASE]], [x[BASE:], G[BASE:]], 64, cap, (y_want[:BASE], gx_want[:BASE]),
                                   (y_want[BASE:], gx_want[BASE:]), bounds, "%s, %d items" % (instance.name, edge.size), exact=False)
    _note(instance.ladder, instance, info, ratio)
    REACHED[instance.name] += 1


def test_every_instance_ran(request, hip_device):
    """Every reachable instance of the table was named by last_launch_info in at least two cases of this file."""
    here = [item for item in request.session.items if item.module is request.module]
    wanted = sum(len(i.edges) for i in di.TABLE) + 1
    if len(here) != wanted:
        pytest.skip("the guard needs every case of this file in the session: %d of %d selected" % (len(here), wanted))
    print("worst error / bound per ladder: %s" % ", ".join("%s %.3f" % kv for kv in sorted(WORST.items())))
    short = {i.name: REACHED[i.name] for i in di.TABLE if i.unreachable is None and REACHED[i.name] < 2}
    assert not short, short
    assert all(REACHED[i.name] == 0 for i in di.TABLE if i.unreachable is not None)


def _child_main():
    """The cases of frames_wave_kernel<pre=1>, in a process whose environment had MOLANN_WAVE_PRE=1 from its start."""
    dev = torch.device("cuda:0")
    ar = Arena(dev, capacity=64 << 20)

    class _Env(object):                                      # the environment is this process's own: nothing to put back
        @staticmethod
        def setenv(k, v):
            os.environ[k] = v

        @staticmethod
        def delenv(k, raising=False):
            os.environ.pop(k, None)
    inst = [i for i in di.instances("LAUNCH_WAVE") if i.args == (1,)][0]
    for e in inst.edges:
        ratio, info = _features_case("%s, %d items" % (inst.name, e.size), inst.name, di.SMALL_LADDER_ATOMS,
                                     _items(di.SMALL_LADDER_ATOMS, e.size, e.size), SMALL_ALIGN, e.env, dev, ar, _Env, seed=e.size)
        print("case %d: ratio %.4g info %s" % (e.size, ratio, info))


if __name__ == "__main__" and sys.argv[1:] == ["wave-pre-child"]:
    _child_main()
