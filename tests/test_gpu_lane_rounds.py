"""The float32 lane-per-frame kernels past one ring generation per block (tests/lane_rounds.py): molann_lane_jit in its fused, features-only,
training-forward, align_out and wide-head builds, molann_bwd_ring and its <values> build, and the ahead-of-time kernels behind them -
frames_lane_kernel, mlp_lane_kernel, mlp_mfma_kernel, molann_mlp_bwd + molann_lane_bwd - each at a batch that takes every block through
two full generations of its ring (iterations of its grid-stride loop) and into a third in which some blocks own one tile more than the
others and the last tile is ragged (37 frames).

Per case, on the ctypes plan of the model, every buffer carved out of a guarded arena (tests/placement.py: 64 guard rows and more on
both sides, outputs prefilled with a NaN pattern):
  one tile  64 frames: the launch info gives the kernel's own geometry (consumers, loaders, slots; waves per block) - no constant here
            is copied from today's geometry.
  base      BASE = 251 seeded frames (Workload.make_frames) in one launch, held to the float64 oracle at the bound of the entry's own
            small-batch test: this keeps the comparison below from comparing two wrong results.
  caps      2^20 frames on plain tensors: the grids the entry's kernels are capped at, from the launch info.
  long      the base repeated on the device to n frames, n from lane_rounds.batch_size / stride_size for those grids: the info names
            the expected kernel with the one-tile launch's geometry, the grid is the cap the batch was sized for (more tiles than
            blocks), by the model every block ran two full generations; every per-frame output row bit for bit the base launch's row
            f mod 251 - all n rows, with the wrong rows' place in the ring in the message; no guard band written, x and every other
            input unchanged.
The backward cases use a cotangent of small integers, so the last layer's bias gradient - a plain sum of cotangent rows - is exact in
any order and must equal the integer sum bit for bit: every frame of every tile counted once, the ragged tile's dead lanes not.  The
other parameter gradients are held to float64 autograd of ann_layers on the oracle's features, each base row weighted by how often it
occurs, within max(2e-4 max|want|, 4 x the error of the same backward run in float32 on the CPU over the long batch)."""

import copy
import re
import time

import pytest
import torch

import lane_rounds as lr
import placement as pl
import test_gpu_backward as tb
from build_util import oracle_for_workload
from molann_amd import workloads as wl
from molann_amd.ann import AlignmentLayer, MolANN, _PlanEntry, create_sequential_nn
from molann_amd.atomgroup import Universe
from oracle import molann_oracle as mo

pytestmark = pytest.mark.gpu
F32, F64 = torch.float32, torch.float64
BASE = lr.BASE
WIDE = [6, 64, 64, 8]
NO_JIT, NO_REGS = {"MOLANN_NO_JIT": "1"}, {"MOLANN_NO_JIT": "1", "MOLANN_NO_REGS": "1"}
# (table row, workload ("C3w": C3 behind the wide head), environment, entry, the kernel the long launch's info must name)
CASES = [
    ("fused", "C1", {}, "forward", r"^molann_lane_jit<NL=2> "),
    ("fused", "C3", {}, "forward", r"^molann_lane_jit<NL=2> "),
    ("features", "C2", {}, "features", r"^molann_lane_jit<NL=0> "),
    ("features", "C3p", {}, "features", r"^molann_lane_jit<NL=0> "),
    ("features", "C3", {}, "features", r"^molann_lane_jit<NL=0> "),            # the features-only twin of a fused plan
    ("train", "C3", {}, "train", r"^molann_lane_jit<NL=2> "),
    ("align_out", "C3", {}, "align", r"^molann_lane_jit<align_out> "),
    ("wide", "C3w", {}, "forward", r"^molann_lane_jit<NL=3,wide> "),
    ("bwd_ring", "C1", {}, "backward", r"^molann_bwd_ring \("),
    ("bwd_ring", "C3", {}, "backward", r"^molann_bwd_ring \("),
    ("bwd_ring", "C2", {}, "backward", r"^molann_bwd_ring \("),
    ("bwd_ring_values", "C3", {}, "vjp", r"^molann_bwd_ring<values> "),
    ("bwd_ring_values", "C2", {}, "vjp", r"^molann_bwd_ring<values> "),
    ("frames_lane_regs", "C3", NO_JIT, "forward", r"^frames_lane_kernel<2,features_"),
    ("frames_lane_regs", "C2", NO_JIT, "features", r"^frames_lane_kernel<0,features_"),
    ("frames_lane_lds", "C3", NO_REGS, "forward", r"^frames_lane_kernel<2,features_lds>"),
    ("frames_lane_lds", "C2", NO_REGS, "features", r"^frames_lane_kernel<0,features_lds>"),
    ("mlp_lane", "C3", {}, "mlp", r"^mlp_lane_kernel<NL=2> "),
    ("mlp_mfma", "C3w", NO_JIT, "mlp", r"^mlp_mfma_kernel<f32> "),
    ("split_bwd", "C3", {"MOLANN_NO_RING_BWD": "1"}, "backward", r"molann_mlp_bwd .*\|\| molann_lane_bwd .*\|\| chunks of \d+ frames"),
]
IDS = ["%s-%s" % c[:2] for c in CASES]
ROWS = ("fused", "features", "train", "align_out", "wide", "bwd_ring", "bwd_ring_values", "frames_lane_regs", "frames_lane_lds", "mlp_lane",
        "mlp_mfma", "split_bwd")
TWIN_OF = {"forward": r"^molann_lane_jit<NL=2> ", "features": r"^molann_lane_jit<NL=0> "}      # what the training-forward twin is compared with
DONE = {}                                     # case id -> what the case printed: geometry, n, generations, errors
KEPT = {}                                     # entry -> the long launch's outputs, within the training-forward twin's case


# ---- the entries: inputs and outputs by name, and the call on the arena's views ---------------------------------------------------------
def _outs(c, entry, n):
    ni, df, do = c.w.n_atoms, c.plan.feature_dim, c.out_dim
    if entry == "forward" or entry == "mlp":
        return {"out": (n, do)}
    if entry == "features":
        return {"features": (n, df)}
    if entry == "train":
        return {"out": (n, do), "features": (n, df)}
    if entry == "align":
        return {"aligned": (n, ni, 3)}
    if entry == "backward":
        return dict([("grad_x", (n, ni, 3))] + ([("grad_params", (c.plan.grad_params_size(),))] if c.w.mlp_dims else []))
    if entry == "vjp":
        return {"out": (n, do), "grad_x": (n, ni, 3)}
    raise KeyError(entry)


def _call(plan, entry, v):
    if entry == "forward":
        plan.forward_packed(v["x"], v["out"])
    elif entry == "features":
        plan.features(v["x"], v["features"])
    elif entry == "train":
        plan.forward_train(v["x"], v["out"], v["features"])
    elif entry == "align":
        plan.align(v["x"], v["aligned"])
    elif entry == "mlp":
        plan.mlp_packed(v["f"], v["out"])
    elif entry == "backward":
        plan.backward(v["x"], v["grad_out"], v["grad_x"], v.get("grad_params"))
    elif entry == "vjp":
        plan.value_and_vjp(v["x"], v["grad_out"], v["out"], v["grad_x"])
    else:
        raise KeyError(entry)


def _capacity(ins, outs):
    """Bytes of an arena that holds these buffers between their guard bands (`out` twice: the launch on x[1:] carves a second one), and
    what Arena.reset refills behind them"""
    total = pl.RESET_MARGIN + (1 << 20)
    for shape in [tuple(t.shape) for t in ins.values()] + list(outs.values()) + [outs[k] for k in ("out",) if k in outs]:
        row = 4
        for d in shape[1:]:
            row *= d
        numel = shape[0] * (row // 4)
        total += 4 * numel + 2 * max(pl.MIN_BAND, pl.BAND_ROWS * row) + 4 * pl.BOUNDARY
    return total


def _launch(c, entry, ins, n, arena=None):
    """One launch on buffers carved at a 256-byte boundary between guard bands: ({name: view}, info, the arena)"""
    outs = _outs(c, entry, n)
    if arena is None:
        arena = pl.Arena(c.dev, capacity=_capacity(ins, outs))
    arena.reset()
    v = dict((k, arena.carve(k, t.shape, F32, 0, data=t)) for k, t in ins.items())
    for k, shape in outs.items():
        v[k] = arena.carve(k, shape, F32, 0)
    if "grad_params" in outs:
        v["grad_params"].zero_()                   # accumulated into
    with torch.cuda.device(c.dev):
        _call(c.plan, entry, v)
        torch.cuda.synchronize()
    info = c.plan.last_launch_info()
    bad = arena.check() + ["input %s was written" % k for k in arena.inputs_changed()]
    assert not bad, (c.what, entry, n, bad)
    return v, info, arena


# ---- the case: model, plan, base batch and the float64 reference of the base launch -----------------------------------------------------
class Ctx(object):
    pass


def _plans_of(module):
    return [e.plan for e in module._plans().values() if isinstance(e, _PlanEntry)]


def _context(row, cfg, env, entry, dev, monkeypatch):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    c = Ctx()
    c.row, c.cfg, c.entry, c.dev, c.what = row, cfg, entry, dev, "%s-%s" % (row, cfg)
    c.w = w = wl.get_workload("C3" if cfg == "C3w" else cfg)
    model = wl.build_model(w, dev).requires_grad_(False)
    if cfg == "C3w":
        torch.manual_seed(sum(WIDE))
        model = MolANN(model.preprocessing_layer, create_sequential_nn(WIDE).to(dev)).requires_grad_(False)
        w.mlp_dims = list(WIDE)
    c.model = model
    c.x = w.make_frames(BASE, seed=1000 + len(cfg)).to(dev)
    x4 = c.x[:4].contiguous()
    if entry == "align":
        u = Universe(w.ref_xyz)
        c.layer = AlignmentLayer(u.atoms_by_number(w.align), u.atoms).to(dev)
        with torch.no_grad():
            c.layer(x4)
        (c.plan,) = [p for p in _plans_of(c.layer) if p.feature_dim == 0]
    elif isinstance(model, MolANN):
        c.plan = model.plan_for(x4)
    else:
        with torch.no_grad():
            model(x4)
        (c.plan,) = [p for p in _plans_of(model) if p.feature_dim == w.feature_dim()]
    assert c.plan is not None
    c.out_dim = w.mlp_dims[-1] if w.mlp_dims else c.plan.feature_dim
    c.feats = [(t, [a - 1 for a in atoms]) for t, atoms in w.features]
    c.al = [a - 1 for a in w.align] if w.align is not None else None
    c.ref = mo.center_reference(torch.from_numpy(w.ref_xyz[c.al])).double() if c.al else None
    c.f64 = mo.preprocessing_forward(c.x.cpu().double(), c.feats, w.use_angle_value, c.al, c.ref)     # the oracle's features of the base
    c.ins = {"x": c.x}
    if entry == "mlp":
        c.ins = {"f": c.f64.float().to(dev)}
    if entry in ("backward", "vjp"):
        G = torch.randint(-2, 3, (BASE, c.out_dim), generator=torch.Generator().manual_seed(7))
        G[(G == 0).all(1), 0] = 1                  # no all-zero row
        assert int(G.abs().max()) == 2 and not bool((G == 0).all(1).any())
        c.G = G
        c.ins["grad_out"] = G.to(F32).to(dev)
    torch.cuda.synchronize()
    return c


def _head64(c, f):
    lins = [m for m in c.model.ann_layers if isinstance(m, torch.nn.Linear)]
    h = f.double()
    for i, lin in enumerate(lins):
        h = h @ lin.weight.detach().cpu().double().T + lin.bias.detach().cpu().double()
        if i + 1 < len(lins):
            h = torch.tanh(h)
    return h


def _hold_base(c, got):
    """The base launch against float64 at the bound of the entry's own small-batch test; returns the printed figures"""
    w, x, figures = c.w, c.x.cpu(), []

    def hold(name, want, bound, what):
        err = float((got[name].cpu().double().reshape(want.shape) - want).abs().max())
        figures.append("%s %.3g <= %.3g" % (name, err, bound))
        assert bool(torch.isfinite(got[name]).all()) and err <= bound, (c.what, name, err, bound, what)

    if c.entry in ("forward", "train", "vjp") and c.cfg != "C3w":
        hold("out", oracle_for_workload(w, c.model, x, F64), 2e-5, "test_gpu_parity.test_batch_sizes_vs_oracle")
    if c.entry == "forward" and c.cfg == "C3w":    # against a float64 head on the kernel's own features
        with torch.no_grad():
            f = c.model.preprocessing_layer(c.x).cpu()
        hold("out", _head64(c, f), 1e-5, "test_gpu_parity.test_wide_heads_run_inside_the_lane_kernel")
    if c.entry in ("features", "train"):
        hold("features", c.f64, 2e-5, "test_gpu_parity.test_batch_sizes_vs_oracle")
        if c.cfg == "C3":                          # test_gpu_backward.test_forward_train_keeps_features_and_output_bits
            with torch.no_grad():
                assert torch.equal(got["features"], c.model.preprocessing_layer(c.x)), c.what
    if c.entry == "align":
        hold("aligned", mo.align_forward(x.double(), c.al, c.ref), 1e-5, "test_gpu_parity.test_align_batch_sizes_vs_oracle")
    if c.entry == "mlp":
        hold("out", _head64(c, c.ins["f"].cpu()), 1e-5, "test_gpu_mlp_chain / test_gpu_buffer_placement: fp32 heads")
    if c.entry in ("backward", "vjp"):
        gx, _ = tb._oracle_grads(w, c.model, c.x, c.G.to(F32))
        hold("grad_x", gx, 2e-4 * max(1e-3, float(gx.abs().max())), "test_gpu_backward.test_gradients_vs_fp64_oracle")
        untouched = [i for i in range(w.n_atoms) if (i + 1) not in w.touched_atoms()]
        if untouched:
            assert float(got["grad_x"][:, untouched].abs().max()) == 0.0, (c.what, "atoms the plan never reads")
    assert figures, c.what
    return ", ".join(figures)


# ---- the long launch -------------------------------------------------------------------------------------------------------------------
def _dealers(geoms):
    """(units, frames per tile) of every grid-stride kernel: its waves, and for molann_mlp_bwd - whose blocks are dealt the tiles and hand
    them to their waves through a counter - its blocks as well"""
    units, tiles = [], []
    for g in geoms:
        units.append(lr.units_of(g))
        tiles.append(g.tile)
        if g.by_block:
            units.append(g.grid)
            tiles.append(g.tile)
    return units, tiles


def _size(geoms, grids):
    """The batch size for these kernels at these grids"""
    geoms = [g._replace(grid=grid) for g, grid in zip(geoms, grids)]
    if isinstance(geoms[0], lr.Ring):
        assert len(geoms) == 1, geoms
        return lr.batch_size(geoms[0].grid, geoms[0].nslot)
    return lr.stride_size(*_dealers(geoms))


def _full_generations(geoms, n):
    if isinstance(geoms[0], lr.Ring):
        return lr.full_generations(n, geoms[0].grid, geoms[0].nslot)
    return min(lr.full_generations(n, u, 1, t) for u, t in zip(*_dealers(geoms)))


def _caps(c, entry, first, pattern):
    """The grids of the entry's kernels where there is more work than blocks: read from one launch of 2^20 frames on plain tensors.
    (lane_rounds refuses batches beyond 2^21 frames, so a kernel that 2^20 frames do not fill could not be taken through two
    generations: the sizing below fails for it, as it must.)"""
    n = lr.MAX_FRAMES // 2
    v = dict((k, lr.repeated(t, n)) for k, t in c.ins.items())
    for k, shape in _outs(c, entry, n).items():
        v[k] = torch.zeros(shape, dtype=F32, device=c.dev)
    with torch.cuda.device(c.dev):
        _call(c.plan, entry, v)
        torch.cuda.synchronize()
    info = c.plan.last_launch_info()
    found = lr.geometries(info)
    assert re.search(pattern, info) and [g._replace(grid=0) for g in found] == [g._replace(grid=0) for g in first], (c.what, info, first)
    del v
    torch.cuda.empty_cache()
    return [g.grid for g in found]


def _long(c, entry, first, pattern):
    """The long launch of an entry, sized by the geometry of its one-tile launch `first` and the capped grid it reports itself.
    Returns (views, info, arena, Size, geometries)."""
    grids = _caps(c, entry, first, pattern)
    size = _size(first, grids)
    ins = dict((k, lr.repeated(t, size.n)) for k, t in c.ins.items())
    v, info, arena = _launch(c, entry, ins, size.n)
    del ins
    found = lr.geometries(info)
    assert re.search(pattern, info) and [g._replace(grid=0) for g in found] == [g._replace(grid=0) for g in first], (c.what, info, first)
    assert [g.grid for g in found] == grids, (c.what, "the grid is not the cap the batch was sized for", info, grids)
    for g in found:                                # more tiles than blocks (waves): fewer would be another test
        assert -(-size.n // getattr(g, "tile", lr.TILE)) > lr.units_of(g), (c.what, info, size)
    assert _full_generations(found, size.n) >= lr.GENERATIONS, (c.what, info, size)
    m = re.search(r"chunks of (\d+) frames", info)
    if m:
        assert size.n <= int(m.group(1)), (c.what, "the batch crosses a workspace chunk", info, size.n)
    return v, info, arena, size, found


def _same_rows(c, v, base, names, size, geoms):
    lead = geoms[-1] if not isinstance(geoms[0], lr.Ring) else geoms[0]
    grid, nslot = (lead.grid, lead.nslot) if isinstance(lead, lr.Ring) else (lr.units_of(lead), 1)
    wrong = lr.wrong_frames(v, base, names=names)
    assert not wrong, (c.what, names, lr.explain(wrong, grid, nslot, size.n))


def _parameter_gradients(c, gp, n):
    """grad_params of the long launch: the last bias exactly, the others against float64 within max(2e-4 max|want|, 4 own)"""
    lins64 = copy.deepcopy(c.model.ann_layers).double().cpu().requires_grad_(True)
    counts = torch.tensor([n // BASE + (1 if r < n % BASE else 0) for r in range(BASE)])
    assert int(counts.sum()) == n
    got = gp.cpu()
    exact = (c.G.long() * counts[:, None]).sum(0)
    assert int(exact.abs().max()) < 1 << 24 and int((c.G.abs().long() * counts[:, None]).sum(0).max()) < 1 << 24
    last = got[-c.out_dim:]
    assert torch.equal(last.view(torch.int32), exact.to(F32).view(torch.int32)), (c.what, "the last bias gradient is not the integer sum of the "
                                                                                 "cotangent rows", last.tolist(), exact.tolist())
    (lins64(c.f64) * (c.G.double() * counts[:, None].double())).sum().backward()
    want = [p.grad.reshape(-1) for p in lins64.parameters()]
    lins32 = copy.deepcopy(c.model.ann_layers).float().cpu().requires_grad_(True)
    (lins32(lr.repeated(c.f64.float(), n)) * lr.repeated(c.G.to(F32), n)).sum().backward()
    own = [p.grad.reshape(-1).double() for p in lins32.parameters()]
    figures, at = [], 0
    for i, (wt, o) in enumerate(zip(want, own)):
        g = got[at:at + wt.numel()].double()
        at += wt.numel()
        err, own_err, scale = float((g - wt).abs().max()), float((o - wt).abs().max()), float(wt.abs().max())
        bound = max(2e-4 * scale, 4.0 * own_err)
        figures.append("p%d err %.3g own %.3g ratio %.3g (max|want| %.3g, bound %.3g)" % (i, err, own_err, err / max(own_err, 1e-300), scale, bound))
        print("lane rounds %s: parameter %d of %d: err %.4g, own %.4g, err / own %.3g, max|want| %.4g, bound %.4g"
              % (c.what, i, len(want), err, own_err, err / max(own_err, 1e-300), scale, bound))
        assert err <= bound, (c.what, i, err, own_err, scale, bound)
    assert at == got.numel()
    return "; ".join(figures)


@pytest.mark.parametrize("row,cfg,env,entry,pattern", CASES, ids=IDS)
def test_two_generations_and_a_ragged_uneven_third(row, cfg, env, entry, pattern, hip_device, monkeypatch):
    t0 = time.time()
    c = _context(row, cfg, env, entry, hip_device, monkeypatch)
    entries = ["forward", "features", "train"] if entry == "train" else [entry]
    notes = []
    for e in entries:
        # ---- one tile: the kernel's own geometry
        v, info, _ = _launch(c, e, dict((k, t[:64].contiguous()) for k, t in c.ins.items()), 64)
        first = lr.geometries(info)
        assert first and all(g.grid == 1 for g in first if isinstance(g, lr.Ring)), (c.what, info)
        # ---- base: one launch of the 251 frames, against float64
        v, info, _ = _launch(c, e, c.ins, BASE)
        base = dict((k, v[k].clone()) for k in _outs(c, e, BASE))
        c.entry = e
        held = _hold_base(c, base)
        c.entry = entry
        # ---- long
        v, info, arena, size, geoms = _long(c, e, first, pattern if e == entry else TWIN_OF[e])
        names = [k for k in base if k != "grad_params"]
        _same_rows(c, v, base, names, size, geoms)
        gens = _full_generations(geoms, size.n)
        note = "%s: %s | n = %d (%d tiles, %d dealers with one more), %d full generations | base: %s" % (e, info, size.n, size.n_tiles, size.extra, gens, held)
        if "grad_params" in v:
            note += " | " + _parameter_gradients(c, v["grad_params"], size.n)
        if entry == "train":
            KEPT[e] = dict((k, v[k].clone()) for k in names)
        if (row, cfg, e) == ("fused", "C3", "forward"):
            # the same launch on a view one frame in: its data pointer is 8-byte aligned (264-byte frames), whichever kernel serves it
            want = v["out"][1:].clone()
            xv = v["x"][1:]
            assert xv.data_ptr() % 16 == 8 and xv.is_contiguous()
            out = arena.carve("out_view", (size.n - 1, c.out_dim), F32, 0)
            with torch.cuda.device(c.dev):
                c.plan.forward_packed(xv, out)
                torch.cuda.synchronize()
            view_info = c.plan.last_launch_info()
            print("lane rounds %s: x[1:] (8-byte aligned) is served by %s" % (c.what, view_info))
            assert arena.check() == [] and arena.inputs_changed() == [], (c.what, arena.check(), arena.inputs_changed())
            wrong = (out.view(torch.int32) != want.view(torch.int32)).any(1).nonzero().flatten()
            assert wrong.numel() == 0, (c.what, "x[1:]", view_info, lr.explain((wrong[:64] + 1).tolist(), geoms[0].grid, geoms[0].nslot, size.n))
            note += " | x[1:]: " + view_info
        print("lane rounds %s %s" % (c.what, note))
        notes.append((note, gens, size.n))
        del v, arena
        torch.cuda.empty_cache()
    if entry == "train":                           # the twin's outputs and features are the fused forward's and the features launch's
        assert torch.equal(KEPT["train"]["out"], KEPT["forward"]["out"]) and torch.equal(KEPT["train"]["features"], KEPT["features"]["features"])
        KEPT.clear()
    DONE[c.what] = (row, min(g for _, g, _ in notes), [n for n, _, _ in notes], time.time() - t0)
    print("lane rounds %s: passed in %.2f s" % (c.what, time.time() - t0))


def test_every_row_of_the_table_ran_its_generations(request, hip_device):
    """Every kernel row of the table recorded a passed case, past two full generations or iterations.  The cases are recorded as they
    pass, so this guard needs all of them in the same session."""
    here = {item.name for item in request.session.items if item.module is request.module}
    wanted = {"test_two_generations_and_a_ragged_uneven_third[%s]" % i for i in IDS}
    if not wanted <= here:
        pytest.skip("the coverage guard needs every case in this session: %d not selected" % len(wanted - here))
    missing = sorted(set(IDS) - set(DONE))
    assert not missing, ("not reached:", missing)
    assert {row for row, _, _, _ in DONE.values()} == set(ROWS) == {c[0] for c in CASES}
    assert all(gens >= lr.GENERATIONS for _, gens, _, _ in DONE.values()), DONE
    for what, (row, gens, notes, seconds) in sorted(DONE.items()):
        print("lane rounds %s: %d full generations, %.1f s" % (what, gens, seconds))
    print("lane rounds: %d cases, %.1f s in all, the slowest %.2f s" % (len(DONE), sum(d[3] for d in DONE.values()), max(d[3] for d in DONE.values())))
