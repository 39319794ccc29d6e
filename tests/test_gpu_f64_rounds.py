"""Every float64 one-launch kernel past one round per block (tests/f64_rounds.py): frames_value_{vjp,jac,metric,restraint,hills,grid,bias,
opes,bias_opes,opes_table}_f64_kernel<8|16|32|64>, each at a batch of three full rounds of its grid-stride loop and a ragged fourth.

One case per (entry, lane group, plan shape); the models, tables, oracles and bounds are the entries' own test files' (imported, not
copied), the plan shapes those of their `test_lane_groups`: 7 / 12 / 30 / 40 atoms aligned behind a small head (16, 16, 32, 64 lanes:
the head's 12 feature columns ask for 16) and without alignment or head (8, 16, 32, 64 lanes); 7 atoms aligned without a head, the only
shape in which the rotation and its backward run on 8 lanes, eight frames to a wave; and the stepped-down head [3, 682, 2] (two waves
per block) for one entry of each row layout.  The tables are small and ragged: 2 G + 5 hills or kernels with a row of sigma
each, one periodic column, a cutoff of 4; the table of value_and_opes_table has 19 dead rows of NaN behind its live ones; the grid is
vg.SHAPES[2] with one periodic axis.

Per case, three launches:
  base      BASE = 251 seeded frames in one launch (one round), held to float64 autograd through the oracle on the CPU at the bounds of
            the entry's own file, with that file's "the reference is not nearly zero" conditions; everything finite.
  clean     the base repeated on the device to N = 3 grid per_block + tail, N from this launch's own info (f64_rounds.batch_size):
            every block ran three rounds; every per-frame output row bit for bit the base launch's row f mod 251.
  poisoned  the same N with NaN in x (isolation.chosen_atom) of every frame but about 34 - 0, 63, 64, N - 1, a frame of each live slot
            class of the ragged round, seeded ones: the kept frames bit for bit the clean launch's and finite, every poisoned frame's y
            and bias (energy, energies, metric) non-finite.
Every launch runs once.  The shared table and state of value_and_opes_table are compared before and after each launch."""

import contextlib
import io
import time
import zlib

import pytest
import torch

import f64_rounds as fr
import isolation as iso
import opes_run_cases as rc
import placement as pl
import test_gpu_frame_isolation as fi
import test_gpu_opes_run_f64 as vor
import test_gpu_random_backward as rb
import test_gpu_value_and_bias_f64 as vb
import test_gpu_value_and_bias_opes_f64 as vbo
import test_gpu_value_and_grid_f64 as vg
import test_gpu_value_and_hills_f64 as vh
import test_gpu_value_and_jacobian_f64 as vjac
import test_gpu_value_and_metric_f64 as vm
import test_gpu_value_and_opes_f64 as vo
import test_gpu_value_and_restraint_f64 as vr
import test_gpu_value_and_vjp_f64 as vv

pytestmark = pytest.mark.gpu
F64, CPU, NAN = torch.float64, torch.device("cpu"), float("nan")
BASE = fr.BASE
assert BASE == fi.BASE
CUTOFF, EPS = 4.0, 1e-3
SEEDS = (0, 1, 2, 3, 4)                       # a builder that misses its asserted margins on one seed gets the next
KERNELS = {"vjp": vv.KERNEL, "jacobian": vjac.KERNEL, "metric": vm.KERNEL, "restraint": vr.KERNEL, "hills": vh.KERNEL, "grid": vg.KERNEL,
           "bias": vb.KERNEL, "opes": vo.KERNEL, "bias_opes": vbo.KERNEL, "opes_table": vor.KERNEL}
ENTRIES = tuple(KERNELS)
SIZES = ((7, 8), (12, 16), (30, 32), (40, 64))
STEP_DOWN = ("vjp", "jacobian", "restraint", "bias", "bias_opes")       # one entry of each row layout
CASES = ([(e, n_inp, shape) for e in ENTRIES for n_inp, _ in SIZES for shape in ("head", "features")] + [(e, 7, "aligned_features") for e in ENTRIES]
         + [(e, 8, "step_down") for e in STEP_DOWN])
SCALARS = ("energy", "bias", "energies", "metric")
DONE = {}                                     # (entry, n_inp, shape) -> (Rounds, the base's printed errors, seconds)


class Ctx(object):
    pass


def _lanes_of(n_inp, shape):
    if shape == "step_down":
        return 64
    lanes = dict(SIZES)[n_inp]
    return max(lanes, 16) if shape == "head" else lanes       # the head's widest layer input (12 feature columns) asks for 16 lanes


def _case(entry, n_inp, shape):
    """The rb.Case of the entry's own `test_lane_groups` for this shape"""
    head, aligned = shape == "head", shape != "features"
    if shape == "step_down":
        return rb.Case("step_down", rb._chain(8, 3), vr.BONDS, None, mlp=list(vr.STEPPED["step_down"][0]))
    if entry == "grid":
        return vg._lane_case(n_inp, aligned, head, 2)
    if entry in ("bias", "bias_opes") and head:
        case = vv._small_case(n_inp, [0, 2, 4, 6], head=True)
        case.mlp = [case.d_feat(), 5, 4]
        return case
    if entry in ("vjp", "restraint"):
        return vv._small_case(n_inp, [0, 2, 4, 6] if aligned else None, head=head)
    return vh._small_case(n_inp, aligned, head)


def _one_period(d):
    p = torch.zeros(d, dtype=F64)
    p[0] = 1.3
    return p


def _named(names, result):
    """the siblings' `_call` results, (y, ..., info) or ((y, ...), info), as ({name: output}, info)"""
    out, info = result if len(result) == 2 and not isinstance(result[0], torch.Tensor) else (result[:-1], result[-1])
    assert isinstance(info, str) and len(out) == len(names), (names, info)
    return dict(zip(names, out)), info


# ---- the entries: c.pf (per-frame inputs besides x, on the device), c.call(x, pf) -> ({name: output}, info), c.hold(outputs) -------------
def _prepare(c, seed):
    e, model, args, x, dev, G = c.entry, c.model, c.args, c.x, c.dev, c.lanes
    on = lambda t: t.to(dev)       # noqa: E731
    c.pf, c.shared = {}, ()
    n_k = 2 * G + 5
    if e == "vjp":
        cot = torch.randn((c.nb, c.d_out), generator=torch.Generator().manual_seed(seed + 1), dtype=F64).to(dev)
        want = vv._oracle(model, *args, x, cot)
        c.pf = {"G": cot}
        c.call = lambda x, pf: _named(("out", "grad_x"), vv._call(model, x, pf["G"]))
        c.hold = lambda o: vv._close(o["out"], o["grad_x"], *want, what=c.what)
        return
    if e == "jacobian":
        c.call = lambda x, pf: _named(("out", "jac"), vjac._call(model, x))
        c.hold = lambda o: vjac._against_oracle(c.case, model, x, o["out"], o["jac"], c.what)
        return
    if e == "metric":
        c.call = lambda x, pf: _named(("out", "metric"), vm._call(model, x))
        c.hold = lambda o: vm._against_oracle(c.case, model, x, None, o["out"], o["metric"], c.what)
        return
    xx, y_ref = vr._reference_y(model, *args, x)
    _, y_tab = vr._reference_y(model, *args, c.x_tab)
    d = c.d_out
    if e == "restraint":
        period = vr._period_row(d, 1.3, 2)
        z, kappa, flat = vr._centres(y_ref, period, True, seed)
        want = vr._oracle(xx, y_ref, z, kappa, period, flat)
        c.pf = {"z": on(z)}
        c.call = lambda x, pf: _named(("out", "energy", "grad_x"), vr._call(model, x, pf["z"], on(kappa), on(period), on(flat)))
        c.hold = lambda o: vr._close((o["out"], o["energy"], o["grad_x"]), want, c.what)
    elif e == "hills":
        period = _one_period(d)
        table, far = vh._hill_table(y_ref, y_tab, period, n_k, True, seed)
        assert far, "no (frame, hill) pair with q > 50"
        want = vh._oracle(xx, y_ref, *table, period)
        assert float(want[1].abs().max()) > 0.05 and float(want[2].abs().max()) > 1e-3, "the reference is (nearly) zero"
        table = tuple(on(t) for t in table)
        c.call = lambda x, pf: _named(("out", "bias", "grad_x"), vh._call(model, x, *table, on(period)))
        c.hold = lambda o: vh._close((o["out"], o["bias"], o["grad_x"]), want, c.what)
    elif e == "grid":
        shape, periodic = vg.SHAPES[2], [False, True]
        lower, spacing = vg._grid_from(y_ref, shape, periodic)
        table = vg._seeded_table(shape, 100 + seed)
        want = vg._oracle(xx, y_ref, table, lower, spacing, periodic)[0]
        vg._nontrivial(want)
        table = on(table)
        c.call = lambda x, pf: _named(("out", "bias", "grad_x"), vg._call(model, x, table, lower, spacing, periodic))
        c.hold = lambda o: vh._close((o["out"], o["bias"], o["grad_x"]), want, c.what)
    elif e in ("bias", "bias_opes"):
        if c.shape == "step_down":                                  # the siblings' step-down terms on the head's two outputs
            r, cols, gc, p2 = (torch.tensor([0.7, 0.0], dtype=F64), True, []), (1, 0), (1, 0), torch.tensor([0.0, 0.7], dtype=F64)
        elif c.shape == "head":
            r, cols, gc, p2 = (vr._period_row(d, 1.3, 2), True, [1]), (3, 1), (0, 2), _one_period(2)
        else:
            r, cols, gc, p2 = (vr._period_row(d, 1.3, 2), True, [1]) if e == "bias" else None, (5, 0, 2), (1, 3), _one_period(3)
        spec = dict(g=(gc, (5, 6), [True, False]))
        if r is not None:
            spec["r"] = r
        if e == "bias":
            spec["h"] = (cols, p2, n_k, True)
            T, want, far = vb._reference_terms(model, args, x, c.x_tab, spec, seed, c.what)
            assert far, "no (frame, hill) pair with q > 50"
            present = (T.r is not None, True, True)
        else:
            T, O, want = vbo._reference(model, args, x, c.x_tab, spec, (cols, p2, n_k, True, CUTOFF), seed, c.what)
            present = (T.r is not None, False, True, True)
        if T.r is not None:
            c.pf = {"z": on(T.r[0])}
        rest = None if T.r is None else tuple(on(t) for t in T.r[1:])
        terms = lambda pf: vb.Terms(None if rest is None else (pf["z"],) + rest, T.h, T.g)       # noqa: E731
        if e == "bias":
            c.call = lambda x, pf: _named(("out", "energies", "grad_x"), vb._call(model, x, terms(pf)))
            c.hold = lambda o: vb._close((o["out"], o["energies"], o["grad_x"]), want, c.what, present)
        else:
            c.call = lambda x, pf: _named(("out", "energies", "grad_x"), vbo._call(model, x, terms(pf), O))
            c.hold = lambda o: vbo._close((o["out"], o["energies"], o["grad_x"]), want, c.what, present)
    elif e == "opes":
        period = _one_period(d)
        table, norm = vo._table(y_ref, y_tab, period, n_k, True, seed, (CUTOFF,))
        want = vo._oracle(xx, y_ref, table, period, norm, EPS, CUTOFF)
        assert float(want[2].abs().max()) > 1e-3, "the reference's forces are (nearly) zero"
        table = tuple(on(t) for t in table)
        c.call = lambda x, pf: _named(("out", "bias", "grad_x"), vo._call(model, x, table, period, norm, EPS, CUTOFF))
        c.hold = lambda o: vh._close((o["out"], o["bias"], o["grad_x"]), want, c.what)
    elif e == "opes_table":
        period = _one_period(d)
        t = vor._filled_table(dev, y_tab.detach(), n_k, n_k + 19, period, CUTOFF, seed)
        torch.cuda.synchronize()
        n_live, total, _, _ = t.read_state()
        assert n_live == n_k < t.centers.shape[0] and bool(torch.isnan(t.centers[n_live:]).all()) and bool(torch.isnan(t.heights[n_live:]).all())
        live = tuple(v[:n_live].cpu() for v in (t.centers, t.heights, t.sigma))
        inside, outside = vo._conditions(y_ref, live, period, CUTOFF)
        want = vo._oracle(xx, y_ref, live, period, total / n_live, rc.EPSILON, CUTOFF)
        v0 = vo.SCALE * torch.log(torch.tensor(rc.EPSILON, dtype=F64))
        assert float((want[1] - v0).abs().max()) > 0.05 and float(want[2].abs().max()) > 1e-3, "the reference is (nearly) zero"
        c.shared = (t.centers, t.heights, t.sigma, t.state)

        def call(x, pf):
            out = model.value_and_opes_table(x, t, vo.SCALE, rc.EPSILON)
            torch.cuda.synchronize()
            return dict(zip(("out", "bias", "grad_x"), out)), vh._info(model)

        def hold(o):
            vh._close((o["out"], o["bias"], o["grad_x"]), want, c.what)
            same = model.value_and_opes(x, t.centers[:n_live], t.heights[:n_live], t.sigma[:n_live], vo.SCALE, total / n_live, rc.EPSILON, CUTOFF, t.period)
            torch.cuda.synchronize()
            assert all(torch.equal(a, b) for a, b in zip((o["out"], o["bias"], o["grad_x"]), same)), (c.what, "not value_and_opes' bits")
        c.call, c.hold = call, hold
    else:
        raise KeyError(e)


def _launch(c, x, pf):
    """One launch; the shared table and state of value_and_opes_table unchanged by it, bit for bit"""
    before = [t.clone() for t in c.shared]
    out, info = c.call(x, pf)
    torch.cuda.synchronize()
    assert all(pl.same_bits(a, b) for a, b in zip(before, c.shared)), (c.what, "the table or its state was written")
    assert KERNELS[c.entry] in info and info.count("_kernel") == 1 and "%d lanes per frame" % c.lanes in info, (c.what, info)
    sizes = dict((k, v.numel() * 8) for k, v in list(out.items()) + [("x", x)] + list(pf.items()))
    assert max(sizes.values()) < fi.ONE_GB, (c.what, sizes)
    return out, info


def _context(entry, n_inp, shape, dev):
    """The case, its model and base batch, and the entry's terms from the first seed (and base size) whose builders hold their margins"""
    c = Ctx()
    c.entry, c.shape, c.dev, c.lanes = entry, shape, dev, _lanes_of(n_inp, shape)
    c.case = _case(entry, n_inp, shape)
    c.model = c.case.build(dev).double().requires_grad_(False)
    c.args = (c.case.feats, c.case.uav, c.case.align)
    c.d_out = c.case.mlp[-1] if c.case.mlp else c.case.d_feat()
    c.x_tab = c.case.frames(65, seed=900 + n_inp, dev=CPU).double().to(dev)
    missed = []
    for nb in (BASE, 65):                     # the siblings' 65 frames only where no seed holds the margins on 251
        for seed in SEEDS:
            c.nb, c.what = nb, "%s %s n_inp=%d G=%d (base %d, seed %d)" % (entry, shape, n_inp, c.lanes, nb, seed)
            c.x = c.case.frames(nb, seed=n_inp + 11 + 100 * seed, dev=CPU).double().to(dev)
            try:
                _prepare(c, n_inp + seed)
                if missed:
                    print("rounds %s: earlier builds missed their margins: %s" % (c.what, missed))
                return c
            except AssertionError as err:
                missed.append((nb, seed, str(err)[:120]))
    raise AssertionError(("no seed holds the builders' margins", entry, n_inp, shape, missed))


def _kept(r, what):
    g = torch.Generator().manual_seed(zlib.crc32(what.encode()) & 0xFFFF)
    classes = dict((name, fr.frame_of(r, slot, fr.ROUNDS)) for name, slot in r.classes.items())
    assert all(fr.ROUNDS * r.grid * r.per_block <= f < r.n for f in classes.values())
    return sorted({0, 63, 64, r.n - 1} | set(classes.values()) | set(torch.randint(0, r.n, (28,), generator=g).tolist())), classes


@pytest.mark.parametrize("entry,n_inp,shape", CASES, ids=["%s-%d-%s" % c for c in CASES])
def test_three_rounds_and_a_ragged_fourth(entry, n_inp, shape, hip_device):
    t0 = time.time()
    dev = hip_device
    c = _context(entry, n_inp, shape, dev)
    # ---- base: one launch, one round, against the oracle at the entry's own bounds
    base, info = _launch(c, c.x, c.pf)
    printed = io.StringIO()
    with contextlib.redirect_stdout(printed):
        c.hold(base)
    errors = " | ".join(line.strip() for line in printed.getvalue().splitlines())
    assert all(bool(torch.isfinite(v).all()) for v in base.values()), (c.what, "the base launch is not finite")
    grid, block, lanes = fr.geometry(info, fi.GEOMETRY)
    assert lanes == c.lanes and grid == -(-c.nb // (block // lanes)) and (block == 128) == (shape == "step_down"), (c.what, info)
    base = dict((k, v.clone()) for k, v in base.items())
    # ---- clean: three rounds and a ragged fourth, N from the launch's own info
    grid = 8 * torch.cuda.get_device_properties(dev).multi_processor_count
    for _ in range(3):
        r = fr.batch_size(grid, block, lanes, c.nb)
        x = fr.repeated(c.x, r.n)
        pf = dict((k, fr.repeated(v, r.n)) for k, v in c.pf.items())
        long, info = _launch(c, x, pf)
        found = fr.geometry(info, fi.GEOMETRY)
        assert found[1:] == (block, lanes), (c.what, info)
        if found[0] == grid:
            break
        grid, long = found[0], None
    else:
        raise AssertionError((c.what, "the grid does not settle", info))
    assert fr.rounds_run(r.n, grid, r.per_block) >= fr.ROUNDS and grid * r.per_block * fr.ROUNDS < r.n, (c.what, info, r.n)
    print("rounds %s: N = %d, grid = %d x %d frames (block %d), %d full rounds, then %d frames live in (block, wave, group) %s; base: %s"
          % (c.what, r.n, grid, r.per_block, block, fr.rounds_run(r.n, grid, r.per_block), r.tail, r.live, errors))
    wrong = fr.wrong_frames(long, base)
    assert not wrong, (c.what, "%d frames are not the base launch's bits; the first: %d (round %d, block %d, slot %d), grid x per_block = %d"
                       % (len(wrong), wrong[0], wrong[0] // (grid * r.per_block), wrong[0] % (grid * r.per_block) // r.per_block,
                          wrong[0] % r.per_block, grid * r.per_block), wrong[:8])
    # ---- poisoned: NaN in every frame but the kept ones
    keep, classes = _kept(r, c.what)
    keep_t = torch.tensor(keep, device=dev)
    clean = dict((k, v[keep_t].clone()) for k, v in long.items())
    del long
    mask = torch.ones(r.n, dtype=torch.bool, device=dev)
    mask[keep_t] = False
    atom = iso.chosen_atom(c.case.align, c.case.feats)
    x[mask, atom, iso.COORD] = NAN
    got, info2 = _launch(c, x, pf)
    assert info2 == info, (c.what, info2)
    kept = dict((k, v[keep_t]) for k, v in got.items())
    bad = iso.keep_rows_equal(clean, kept, [], sorted(kept))
    assert not bad, (c.what, "kept frames %s" % keep, bad)
    assert all(bool(torch.isfinite(v).all()) for v in kept.values()), (c.what, "kept frames are not finite")
    for name in ["out"] + [s for s in SCALARS if s in got]:
        finite = torch.isfinite(got[name].reshape(r.n, -1)).all(1) & mask
        assert not bool(finite.any()), (c.what, "%s of %d poisoned frames is finite; the first: %d" % (name, int(finite.sum()), int(finite.nonzero()[0])))
    seconds = time.time() - t0
    print("rounds %s: passed in %.2f s; kept %d frames, ragged-round classes %s, atom %d poisoned" % (c.what, seconds, len(keep), classes, atom))
    DONE[(entry, n_inp, shape)] = (r, errors, seconds)
    del got, x, pf
    torch.cuda.empty_cache()


def test_every_entry_lane_group_and_shape_ran_its_rounds(request):
    """All three phases passed, past three rounds per block, for every (entry, lane group, shape): the ten entries on 8, 16, 32 and 64
    lanes, the six OPES instances on 32 and 64 among them, and the two-wave blocks.  The cases are recorded as they pass, so this guard
    needs all of them in the same session."""
    here = {item.name for item in request.session.items if item.module is request.module}
    wanted = {"test_three_rounds_and_a_ragged_fourth[%s-%d-%s]" % c for c in CASES}
    if not wanted <= here:
        pytest.skip("the coverage guard needs every case in this session: %d not selected" % len(wanted - here))
    missing = sorted(set(CASES) - set(DONE))
    assert not missing, ("not reached:", missing)
    reached = {(e, r.lanes, r.block) for (e, _, _), (r, _, _) in DONE.items()}
    assert {(e, g, 256) for e in ENTRIES for g in (8, 16, 32, 64)} | {(e, 64, 128) for e in STEP_DOWN} == reached, sorted(reached)
    assert all(fr.rounds_run(r.n, r.grid, r.per_block) >= fr.ROUNDS for r, _, _ in DONE.values())
    print("rounds: %d cases, %.1f s in all, the slowest %.2f s" % (len(DONE), sum(s for _, _, s in DONE.values()), max(s for _, _, s in DONE.values())))
