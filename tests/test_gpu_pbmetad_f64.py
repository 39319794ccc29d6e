"""Parallel-bias metadynamics on the device: frames_value_pbmetad_f64_kernel (`value_and_pbmetad`: values, K one-dimensional tables
joined by a soft minimum, walls and forces in one launch) and pbmetad_deposit_f64_kernel (`PBMetadRun.deposit`: a step's hills added to
the K tables, every height weighted by its axis' share of the soft minimum).

  frames   against CPU float64 autograd through the oracle's preprocessing, a copy of the head and tests/pbmetad_oracle.py's formula; against
           `value_and_vjp` (y bit for bit, dx for the cotangent the kernel implies) and the host twin on the device's y; rounds past one
           per block, a NaN frame, guard bands, the operator route.
  deposit  the device against its host twin `molann_selftest_pbmetad_deposit_f64` (held against the numpy oracle on the host by
           tests/test_pbmetad_f64_host.py) on that file's shapes and W, with and without a cutoff; run-to-run and split-deposit bits;
           K = 1 against `molann_metad_deposit_f64`; an invalid walker in the second chunk; guard bands.
  loop     bias then deposit, 20 steps of 4 walkers on C3: the eager loop against the CPU loop of the two host twins, and one captured
           graph of the two launches, replayed, against the eager bits."""

import copy
import gc

import numpy as np
import pytest
import torch

import f64_rounds as fr
import isolation
import pbmetad_cases as pc
import pbmetad_oracle as oracle
import placement as pl
import test_gpu_frame_isolation as fi
import test_gpu_random_backward as rb
import test_gpu_value_and_vjp_f64 as vv
from molann_amd import _capi
from molann_amd import bias as mbias
from molann_amd.ann import MolANN, _device_buffer
from oracle import molann_oracle as mo

pytestmark = pytest.mark.gpu
F64, INF, NAN, KT = pc.F64, pc.INF, pc.NAN, pc.KT
KERNEL = "frames_value_pbmetad_f64_kernel"
CUTOFF = 3.3
_MODELS, _LOOP = {}, {}


@pytest.fixture(scope="module", autouse=True)
def _free_models_and_graphs():
    yield
    _MODELS.clear()
    _LOOP.clear()
    gc.collect()
    torch.cuda.empty_cache()


def _model(name, dev):
    if name not in _MODELS:
        _MODELS[name] = vv._workload(name, dev)
    return _MODELS[name]


def _d_out(w, model):
    return model.ann_layers[-1].out_features if isinstance(model, MolANN) else w.feature_dim()


def _tables_for(y_all, columns, K, dev, periodic=None, seed=0):
    """K tables whose grids are built from the model's own outputs: a non-periodic axis covers the middle of the values, so some frames
    lie below and above it; a periodic axis covers half of them, so the others wrap."""
    rng = np.random.RandomState(40 + seed)
    cols = list(range(K)) if columns is None else list(columns)
    shape = [(5, 9, 4, 33, 6, 17, 12, 7)[k] for k in range(K)]
    periodic = [k % 2 == 1 for k in range(K)] if periodic is None else periodic
    lower, spacing = [], []
    for k in range(K):
        v = np.sort(y_all[:, cols[k]].numpy())
        i, j = len(v) // 5, 4 * len(v) // 5
        lo, hi = 0.5 * (v[i - 1] + v[i]), 0.5 * (v[j] + v[j + 1])        # between two values: the derivative jumps at a range's ends
        lower.append(float(lo))
        spacing.append(float((hi - lo) / (shape[k] - (0 if periodic[k] else 1))))
        u = (v - lower[k]) / spacing[k]
        assert periodic[k] or (np.abs(u).min() > 1e-9 and np.abs(u - (shape[k] - 1)).min() > 1e-9), "a y within 1e-9 spacing of an end"
    table = torch.from_numpy(rng.uniform(-3.0, 5.0, size=sum(shape))).to(dev)
    return mbias.PBTables(table, shape, lower, spacing, periodic, columns)


def _cpu(t):
    return t._replace(table=t.table.cpu())


def _reference(model, args, x, tables, walls):
    """y, energies and dx by float64 autograd on the CPU: the oracle's preprocessing on the model's own ref_x, a copy of the head, then
    the formula."""
    feats, uav, align = args
    al = rb._align_layer(model)
    ref = al.ref_x.detach().cpu().double() if al is not None else None
    xx = x.detach().cpu().double().requires_grad_(True)
    y = mo.preprocessing_forward(xx, feats, uav, align if al is not None else None, ref)
    if isinstance(model, MolANN):
        y = copy.deepcopy(model.ann_layers).cpu().double()(y)
    t = _cpu(tables)
    vpb, V = oracle.torch_bias(y, t.table, t.shape, t.lower, t.spacing, t.periodic, t.columns, KT)
    e_r = torch.zeros(x.shape[0], dtype=F64)
    if walls is not None:
        d = y - walls.center.cpu()
        e_r = 0.5 * (walls.kappa.cpu() * d * d).sum(dim=1)
    (gx,) = torch.autograd.grad((vpb + e_r).sum(), xx)
    return y.detach(), torch.cat([e_r.detach()[:, None], vpb.detach()[:, None], V.detach()], dim=1), gx


def _walls(y_all, dev):
    d = y_all.shape[1]
    return mbias.Restraint(y_all.mean(dim=0).to(dev), torch.linspace(0.0, 3.0, d, dtype=F64).to(dev))


def _outputs(model, w, n, dev, seed=3):
    x = w.make_frames(n, seed=seed).double().to(dev)
    d = _d_out(w, model)
    if isinstance(model, MolANN):
        return x, model.value_and_vjp(x, torch.zeros(n, d, dtype=F64, device=dev))[0].cpu()
    plan = vv._feature_plan(model, x)
    y, dx = torch.empty(n, d, dtype=F64, device=dev), torch.empty_like(x)
    with torch.cuda.device(dev):
        plan.value_and_vjp_f64(x, torch.zeros(n, d, dtype=F64, device=dev), [], [], y, dx)
    return x, y.cpu()


def _implied_cotangent(y, e, t, walls):
    """dE_r/dy + w_k V_k' per frame on the host, in the kernel's order of operations: w from the energies' columns 2.. (`oracle.softmin`),
    V_k' from `molann_selftest_grid_axis_f64` at y and the table's four entries, the walls' dy from `molann_selftest_restraint_f64`."""
    import ctypes
    L = _capi.lib()
    K = len(t.shape)
    cols = list(range(K)) if t.columns is None else list(t.columns)
    offs = [sum(t.shape[:k]) for k in range(K)]
    T = t.table.tolist()
    cot = torch.zeros_like(y)
    for f in range(y.shape[0]):
        row = [0.0] * y.shape[1]
        if walls is not None:
            z, kappa = walls.center.cpu().tolist(), walls.kappa.cpu().tolist()
            for k in range(y.shape[1]):
                d = ctypes.c_double(0.0)
                L.molann_selftest_restraint_f64(float(y[f, k]), z[k], kappa[k], 0.0, 0.0, ctypes.byref(d))
                row[k] = d.value
        _, w = oracle.softmin(e[f, 2:].tolist(), KT)
        for k in range(K):
            idx, a, b = (ctypes.c_int64 * 4)(), (ctypes.c_double * 4)(), (ctypes.c_double * 4)()
            L.molann_selftest_grid_axis_f64(float(y[f, cols[k]]), t.shape[k], t.lower[k], t.spacing[k], 1 if t.periodic[k] else 0, idx, a, b)
            v = [T[offs[k] + idx[j]] for j in range(4)]
            dV = ((v[0] * b[0] + v[1] * b[1]) + v[2] * b[2]) + v[3] * b[3]
            row[cols[k]] = row[cols[k]] + w[k] * dV
        cot[f] = torch.tensor(row, dtype=F64)
    return cot


# ============================================================================================== the frame kernel
FRAME_CASES = [("C3", 8, None, False), ("C3", 3, (5, 0, 2), False), ("C3", 3, (5, 0, 2), True), ("C2", 2, (2, 1), False), ("P1", 3, (6, 1, 3), True)]


@pytest.mark.parametrize("n", [1, 5, 65])
@pytest.mark.parametrize("name,K,columns,walled", FRAME_CASES)
def test_the_kernel_matches_float64_autograd_and_the_related_launches(name, K, columns, walled, n, hip_device):
    dev = hip_device
    w, model, args = _model(name, dev)
    x65, y65 = _outputs(model, w, 65, dev)
    periodic = [True] * K if name == "C2" else None
    tables = _tables_for(y65, columns, K, dev, periodic)
    walls = _walls(y65, dev) if walled else None
    x = x65[:n].contiguous()
    y, e, dx = model.value_and_pbmetad(x, tables, KT, restraint=walls)
    torch.cuda.synchronize()
    info = model.last_launch_info() if isinstance(model, MolANN) else model._plans()[("features", dev.index)].plan.last_launch_info()
    assert KERNEL in info and info.count("_kernel") == 1, info
    y_want, e_want, gx_want = _reference(model, args, x, tables, walls)
    what = "%s K=%d columns %s walls %s n=%d" % (name, K, columns, walled, n)
    vv._close(y, dx, y_want, gx_want, what)
    se = max(1.0, float(e_want.abs().max()))
    err = float((e.cpu() - e_want).abs().max())
    print("%s: energies err %.3e (scale %.3g)" % (what, err, se))
    assert err <= 1e-10 * se and e.shape == (n, 2 + K)
    if not walled:
        assert float(e[:, 0].abs().max()) == 0.0
    # ---- y is value_and_vjp's, bit for bit
    assert torch.equal(y.cpu(), y65[:n])
    # ---- the V_k and E_r against the host twin on the device's own y; dx against value_and_vjp fed the cotangent the kernel implies
    t = _cpu(tables)
    r = None if walls is None else (walls.center.cpu(), walls.kappa.cpu(), None, None)
    rows = [pc.host_frame(y.cpu()[f].contiguous(), t, KT, r) for f in range(n)]
    assert all(code == 0 for code, _, _ in rows)
    e_host, dy_host = torch.stack([r_[1] for r_ in rows]), torch.stack([r_[2] for r_ in rows])
    scale = max(1.0, float(t.table.abs().max()))
    cols = [0] + list(range(2, 2 + K))
    assert float((e.cpu()[:, cols] - e_host[:, cols]).abs().max()) <= 1e-12 * scale
    assert float((e.cpu()[:, 1] - e_host[:, 1]).abs().max()) <= 1e-10 * se
    same_v = pl.same_bits(e.cpu()[:, cols], e_host[:, cols])
    # the cotangent the kernel itself implies, recomputed on the host from the DEVICE's energies: the weights from its V_k, V_k' from the
    # axis step on its y, the walls' dy from the restraint's own function
    cot = _implied_cotangent(y.cpu(), e.cpu(), t, walls)
    assert float((cot - dy_host).abs().max()) <= 1e-9 * max(1e-3, float(dy_host.abs().max()))
    _, dx_vjp, _ = vv._call(model, x, cot.to(dev))
    same_dx = torch.equal(dx, dx_vjp)
    sd = max(1e-3, float(dx_vjp.abs().max()))
    assert same_dx or float((dx - dx_vjp).abs().max()) <= 1e-9 * sd
    print("%s: V_k and E_r %s; dx %s" % (what, "the host twin's bits" if same_v else "within 1e-12 of the host twin",
                                         "value_and_vjp's bits" if same_dx else "within the dx bound of value_and_vjp (exp an ulp apart)"))
    # ---- two calls, and a call into the caller's buffers: the same bits
    into = (torch.empty_like(y), torch.empty_like(e), torch.empty_like(dx))
    again = model.value_and_pbmetad(x, tables, KT, restraint=walls, into=into)
    assert all(a.data_ptr() == b.data_ptr() for a, b in zip(again, into))
    assert all(torch.equal(a, b) for a, b in zip(again, (y, e, dx)))


def test_one_axis_is_value_and_grid_on_that_column(hip_device):
    """K = 1: V_PB has the bits of V_0; against `value_and_bias` with the same 1-D table as its grid the bias is within the bound (the
    stencil sum's order differs) and the layout of energies is (0, V, V)."""
    dev = hip_device
    w, model, _ = _model("C3", dev)
    x, y65 = _outputs(model, w, 65, dev)
    tables = _tables_for(y65, (5,), 1, dev)
    y, e, dx = model.value_and_pbmetad(x, tables, KT)
    assert torch.equal(e[:, 1], e[:, 2]) and float(e[:, 0].abs().max()) == 0.0
    _, eb, dxb = model.value_and_bias(x, grid=mbias.Grid(tables.table, tables.lower, tables.spacing, tables.periodic, (5,)))
    assert float((e[:, 1] - eb[:, 2]).abs().max()) <= 1e-10 * max(1.0, float(eb[:, 2].abs().max()))
    assert float((dx - dxb).abs().max()) <= 1e-9 * max(1e-3, float(dxb.abs().max()))


def test_three_rounds_and_a_ragged_fourth(hip_device):
    dev = hip_device
    w, model, _ = _model("C3", dev)
    _, y65 = _outputs(model, w, 65, dev)
    tables, walls = _tables_for(y65, (5, 0, 2), 3, dev), _walls(y65, dev)
    base_x = w.make_frames(fr.BASE, seed=21).double().to(dev)

    def launch(x):
        y, e, dx = model.value_and_pbmetad(x, tables, KT, restraint=walls)
        torch.cuda.synchronize()
        return {"out": y, "energies": e, "grad_x": dx}, model.last_launch_info()

    base, info = launch(base_x)
    assert KERNEL in info
    grid, block, lanes = fr.geometry(info, fi.GEOMETRY)
    assert grid == -(-fr.BASE // (block // lanes))
    grid = 8 * torch.cuda.get_device_properties(dev).multi_processor_count
    for _ in range(3):
        r = fr.batch_size(grid, block, lanes, fr.BASE)
        long, info = launch(fr.repeated(base_x, r.n))
        found = fr.geometry(info, fi.GEOMETRY)
        assert found[1:] == (block, lanes), info
        if found[0] == grid:
            break
        grid = found[0]
    else:
        raise AssertionError(("the grid does not settle", info))
    assert fr.rounds_run(r.n, grid, r.per_block) >= fr.ROUNDS and grid * r.per_block * fr.ROUNDS < r.n
    print("rounds: N = %d, grid = %d x %d frames (block %d), then %d frames live in %s" % (r.n, grid, r.per_block, block, r.tail, r.live))
    assert fr.wrong_frames(long, base) == []


def test_a_nan_frame_changes_no_other_frame(hip_device):
    dev = hip_device
    w, model, _ = _model("C3", dev)
    x, y65 = _outputs(model, w, 65, dev)
    tables, walls = _tables_for(y65, (5, 0, 2), 3, dev), _walls(y65, dev)
    names = ("y", "energies", "dx")
    clean = dict(zip(names, model.value_and_pbmetad(x, tables, KT, restraint=walls)))
    atom = isolation.chosen_atom([a - 1 for a in w.align], [(ty, [a - 1 for a in at]) for ty, at in w.features])
    bad = [0, 7, 8, 63, 64]
    bad_x = isolation.poison({"x": x}, bad, "mixed", where={"x": 3 * atom + isolation.COORD})["x"]
    poisoned = dict(zip(names, model.value_and_pbmetad(bad_x, tables, KT, restraint=walls)))
    torch.cuda.synchronize()
    assert isolation.keep_rows_equal(clean, poisoned, bad, names, frame_dims=dict((k, 0) for k in names)) == []
    assert not bool(torch.isfinite(poisoned["energies"][bad, 1]).any()) and not bool(torch.isfinite(poisoned["dx"][bad]).all(dim=(1, 2)).any())


@pytest.mark.parametrize("offset", [0, 1])
def test_guard_bands_around_the_frame_kernels_buffers(offset, hip_device):
    dev = hip_device
    w, model, _ = _model("C3", dev)
    x65, y65 = _outputs(model, w, 65, dev)
    tables, walls = _tables_for(y65, (5, 0, 2), 3, dev), _walls(y65, dev)
    want = model.value_and_pbmetad(x65, tables, KT, restraint=walls)
    arena = pl.Arena(dev, capacity=4 << 20)
    x = arena.carve("x", x65.shape, F64, offset, data=x65)
    table = arena.carve("table", tables.table.shape, F64, offset, data=tables.table, row_dims=0)
    y, e, dx = arena.carve("y", (65, 8), F64, offset), arena.carve("energies", (65, 5), F64, offset), arena.carve("dx", x65.shape, F64, offset)
    assert all(v.data_ptr() % 16 == 8 * offset for v in (x, table, y, e, dx))
    got = model.value_and_pbmetad(x, tables._replace(table=table), KT, restraint=walls, into=(y, e, dx))
    torch.cuda.synchronize()
    assert arena.check() == [] and arena.inputs_changed() == []
    assert all(torch.equal(a, b) for a, b in zip(got, want))


def test_the_operator_route_gives_the_ctypes_bits(hip_device):
    from molann_amd import script
    script.load_ops()
    dev = hip_device
    w, model, _ = _model("C3", dev)
    x, y65 = _outputs(model, w, 65, dev)
    tables, walls = _tables_for(y65, (5, 0, 2), 3, dev), _walls(y65, dev)
    st = model._fast_state(x)
    assert st["op"] is not None and st["op_pbmetad"] is torch.ops.molann.value_and_pbmetad_h
    by_op = model.value_and_pbmetad(x, tables, KT, restraint=walls)
    y, e, dx = torch.empty(65, 8, dtype=F64, device=dev), torch.empty(65, 5, dtype=F64, device=dev), torch.empty_like(x)
    lins = st["linears"]
    plan = st["entry"]().plan
    with torch.cuda.device(dev):
        st["entry"]().sync_ref(_device_buffer(st["al"].ref_x, x))
        assert plan.supports_value_and_pbmetad_f64()
        plan.value_and_pbmetad_f64(x, [lin.weight.detach().contiguous() for lin in lins], [lin.bias.detach().contiguous() for lin in lins], y, e, dx,
                                   (tables.columns, tables.table, tables.shape, tables.lower, tables.spacing, tables.periodic, KT),
                                   restraint=(walls.center, walls.kappa, None, None))
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(by_op, (y, e, dx)))
    none = torch.ops.molann.value_and_pbmetad_h(x, st["handle"], _device_buffer(st["al"].ref_x, x), [lin.weight for lin in lins],
                                                [lin.bias for lin in lins], None, None, None, None, [5, 0, 2], tables.table, list(tables.shape),
                                                list(tables.lower), list(tables.spacing), list(tables.periodic), KT, [])
    plain = model.value_and_pbmetad(x, tables, KT)
    assert all(torch.equal(a, b) for a, b in zip(none, plain))
    with pytest.raises(ValueError, match="kT"):
        model.value_and_pbmetad(x, tables, 0.0)
    with pytest.raises(TypeError, match="PBTables"):
        model.value_and_pbmetad(x, tables.table, KT)
    with pytest.raises(IndexError):
        model.value_and_pbmetad(x, tables._replace(columns=(5, 0, 8)), KT)
    with pytest.raises(ValueError, match="into"):
        model.value_and_pbmetad(x, tables, KT, into=(y, torch.empty(65, 4, dtype=F64, device=dev), dx))


def test_the_entrys_refusals_launch_nothing(hip_device):
    dev = hip_device
    w, model, _ = _model("C3", dev)
    x, y65 = _outputs(model, w, 65, dev)
    x = x[:5].contiguous()
    tables = _tables_for(y65, (5, 0, 2), 3, dev)
    st = model._fast_state(x)
    plan, lins = st["entry"]().plan, st["linears"]
    W, B = [lin.weight.detach().contiguous() for lin in lins], [lin.bias.detach().contiguous() for lin in lins]
    y, e, dx = (torch.full(s, 7.0, dtype=F64, device=dev) for s in ((5, 8), (5, 5), tuple(x.shape)))

    def code(**c):
        a = dict(columns=tables.columns, shape=tables.shape, lower=tables.lower, spacing=tables.spacing, kT=KT, energies=e)
        a.update(c)
        try:
            with torch.cuda.device(dev):
                plan.value_and_pbmetad_f64(x, W, B, y, a["energies"], dx, (a["columns"], tables.table, a["shape"], a["lower"], a["spacing"],
                                                                        tables.periodic, a["kT"]))
        except _capi.MolannHipError as err:
            return err.code
        return 0

    assert code(columns=(5, 0, 8)) == _capi.E_INDEX and code(columns=(5, 5, 0)) == _capi.E_INDEX
    assert code(shape=(5, 3, 4)) == _capi.E_DESC and code(spacing=(0.1, INF, 0.1)) == _capi.E_DESC
    assert code(kT=0.0) == _capi.E_DESC and code(kT=NAN) == _capi.E_DESC
    assert code(shape=(2 ** 30, 2 ** 30, 4)) == _capi.E_DESC
    assert code(energies=torch.full((5, 4), 7.0, dtype=F64, device=dev)) == _capi.E_DESC       # a row stride of 4 is below 2 + K
    assert code(columns=(5, 0, 8), shape=(5, 3, 4), kT=0.0) == _capi.E_INDEX and code(shape=(5, 3, 4), kT=0.0) == _capi.E_DESC
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in (y, e, dx)), "a refusal launched"
    assert code() == 0


# ============================================================================================== the deposit kernel
def _device(case, dev, cutoff=None, table=None, state=None, log=None, y=None, V=None):
    table = case.table.to(dev) if table is None else table
    state = torch.zeros(8, dtype=F64, device=dev) if state is None else state
    y = case.y.to(dev) if y is None else y
    V = case.e_store.to(dev)[:, 2:2 + case.K] if V is None else V
    arrays = pc.arrays(case.shape, case.lower, case.spacing, case.periodic, case.sigma, case.columns)
    with torch.cuda.device(dev):
        _capi.pbmetad_deposit_f64(table, arrays, y, V, pc.HEIGHT0, pc.INV_DT, KT, cutoff, state, log)
    return table, state


def _assert_same_step(case, got, want, what, cut=False):
    (table, state), (host_table, host_state) = got, want
    torch.cuda.synchronize()
    heights = pc.host_heights(case.V.contiguous())
    worst = 0.0
    for k in range(case.K):
        tol = pc.tolerance(heights[:, k], case.axis(case.table, k))
        err = float((case.axis(table.cpu(), k) - case.axis(host_table, k)).abs().max())
        worst = max(worst, err / tol)
        assert err <= tol, (what, k, err, tol)
    print("%s shape %s W %d: worst error / bound %.3g%s" % (what, case.shape, case.walkers, worst,
                                                            ", the host's bits" if pl.same_bits(table.cpu(), host_table) else ""))
    state = state.cpu()
    assert state[[0, 1, 3, 4, 5, 6, 7]].tolist() == host_state[[0, 1, 3, 4, 5, 6, 7]].tolist()
    assert abs(float(state[2]) - float(host_state[2])) <= 1e-12 * float(host_state[2])
    assert not cut or torch.equal(table.cpu() != case.table, host_table != case.table)


@pytest.mark.parametrize("walkers", pc.WALKERS)
@pytest.mark.parametrize("shape,periodic", [(pc.SHAPE8, pc.PERIODIC8)] + pc.SMALL)
def test_the_deposit_kernel_matches_its_host_twin(shape, periodic, walkers, hip_device):
    case = pc.Case(shape, periodic, walkers)
    _assert_same_step(case, _device(case, hip_device), pc.run_case(case), "no cutoff")
    cut = pc.Case(shape, periodic, walkers, start="random")
    _assert_same_step(cut, _device(cut, hip_device, CUTOFF), pc.run_case(cut, cutoff=CUTOFF), "cutoff 3.3", cut=True)


@pytest.mark.parametrize("w1,w2,cutoff", [(3, 254, None), (64, 65, CUTOFF), (70, 7, CUTOFF)])
def test_two_runs_and_split_deposits_give_the_same_bits(w1, w2, cutoff, hip_device):
    dev = hip_device
    case = pc.Case(pc.SHAPE8, pc.PERIODIC8, w1 + w2, start="random")
    a, b = _device(case, dev, cutoff), _device(case, dev, cutoff)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    table, state = case.table.to(dev), torch.zeros(8, dtype=F64, device=dev)
    y, V = case.y.to(dev), case.e_store.to(dev)[:, 2:]
    for rows in (slice(0, w1), slice(w1, w1 + w2)):             # queued back to back: nothing is read in between
        _device(case, dev, cutoff, table=table, state=state, y=y[rows], V=V[rows])
    assert torch.equal(table, a[0]) and torch.equal(state[:3], a[1][:3]) and state[3:].tolist() == [2.0, 0.0, 0.0, 0.0, 0.0]
    assert not torch.equal(table.cpu(), case.table)


@pytest.mark.parametrize("periodic,cutoff", [(False, None), (True, CUTOFF)])
def test_one_axis_gives_the_bits_of_the_metadynamics_kernel(periodic, cutoff, hip_device):
    dev = hip_device
    case = pc.Case((1025,), (periodic,), 65, start="random")
    log = torch.zeros(65, 2, dtype=F64, device=dev)
    y, V = case.y.to(dev), case.e_store.to(dev)[:, 2:3]
    got = _device(case, dev, cutoff, log=log, y=y, V=V)
    table, state, log1 = case.table.to(dev), torch.zeros(8, dtype=F64, device=dev), torch.zeros(65, 3, dtype=F64, device=dev)
    arrays = _capi.metad_grid_arrays(case.shape, case.lower, case.spacing, case.periodic, case.sigma, None)
    with torch.cuda.device(dev):
        _capi.metad_deposit_f64(table, arrays, y, V[:, 0], pc.HEIGHT0, pc.INV_DT, cutoff, state, log1)
    assert torch.equal(got[0], table) and torch.equal(got[1][:5], state[:5]) and torch.equal(log[:, 1], log1[:, 2]) and torch.equal(log[:, 0], log1[:, 0])


@pytest.mark.parametrize("bad", ["nan_y", "inf_y", "nan_V", "overflow"])
def test_an_invalid_walker_in_the_second_chunk_changes_no_entry(bad, hip_device):
    dev = hip_device
    case = pc.Case((67, 300, 5), (False, True, True), 66, start="random")
    a = 64                                           # the second chunk's first walker
    if bad in ("nan_y", "inf_y"):
        case.y[a, 1] = NAN if bad == "nan_y" else INF
    else:
        case.V[a, 2] = {"nan_V": NAN, "overflow": -1e6}[bad]
    got = _device(case, dev)
    assert got[1][:2].tolist() == [65.0, 1.0]
    rest = [i for i in range(66) if i != a]
    others = _device(case, dev, y=case.y[rest].to(dev), V=case.V[rest].contiguous().to(dev))
    assert torch.equal(got[0], others[0]) and float(got[1][2]) == float(others[1][2])
    alone = _device(case, dev, y=case.y[a:a + 1].to(dev), V=case.V[a:a + 1].contiguous().to(dev))
    assert pl.same_bits(alone[0].cpu(), case.table) and alone[1].tolist() == [0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0]


@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("cutoff", [None, CUTOFF])
def test_guard_bands_around_the_deposits_buffers(cutoff, offset, hip_device):
    """The table, state, log, y and the energies in an arena of guard bands, every one `offset` doubles past a 16-byte boundary, y ten
    columns wide and the energies a slice of a wider tensor."""
    dev = hip_device
    case = pc.Case((67, 300, 5), (False, True, True), 65, n_out=10, columns=(7, 0, 4), v_pad=3, start="random")
    want_log = torch.zeros(70, 6, dtype=F64, device=dev)
    want = _device(case, dev, cutoff, log=want_log)
    arena = pl.Arena(dev, capacity=4 << 20)
    table = arena.carve("table", case.table.shape, F64, offset, row_dims=0)
    state, log = arena.carve("state", (8,), F64, offset, row_dims=0), arena.carve("log", (70, 6), F64, offset)
    y, store = arena.carve("y", case.y.shape, F64, offset, data=case.y), arena.carve("energies", case.e_store.shape, F64, offset, data=case.e_store)
    table.copy_(case.table), state.zero_(), log.zero_()
    got = _device(case, dev, cutoff, table=table, state=state, log=log, y=y, V=store[:, 2:5])
    torch.cuda.synchronize()
    assert arena.check() == [] and arena.inputs_changed() == []
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(log, want_log) and float(state[4]) == 65.0


# ============================================================================================== the loop
STEPS, WALKERS, BIASFACTOR, HEIGHT = 20, 4, 10.0, 1.2


def _loop(dev, kind):
    """The model, the frames, grids that cover the outputs and the run's arguments, once per kind: "all" (K = 8 on all of C3's outputs) or
    "walls" (K = 3 on outputs (5, 0, 2), a restraint on all eight, a cutoff and a log)."""
    if kind not in _LOOP:
        w, model, _ = _model("C3", dev)
        columns = None if kind == "all" else (5, 0, 2)
        K = 8 if kind == "all" else 3
        xs = [w.make_frames(WALKERS, seed=700 + i).double().to(dev) for i in range(STEPS)]
        y_all = torch.cat([model.value_and_vjp(x, torch.zeros(WALKERS, 8, dtype=F64, device=dev))[0] for x in xs]).cpu()
        cols = list(range(8)) if columns is None else list(columns)
        lo, hi = y_all[:, cols].min(dim=0).values, y_all[:, cols].max(dim=0).values
        shape = tuple((19, 23, 300, 17, 29, 21, 18, 25)[k] for k in range(K))
        periodic = [k % 3 == 1 for k in range(K)]
        lower = [float(lo[k] - 0.15 * (hi[k] - lo[k])) for k in range(K)]
        spacing = [float(1.3 * (hi[k] - lo[k])) / (shape[k] - (0 if periodic[k] else 1)) for k in range(K)]
        sigma = [2.3 * s for s in spacing]
        walls = None
        if kind == "walls":
            walls = mbias.Restraint(y_all.mean(dim=0).to(dev), torch.tensor([3.0, 0.0, 5.0, 1.5, 0.0, 2.0, 0.5, 1.0], dtype=F64, device=dev))
        _LOOP[kind] = dict(w=w, model=model, xs=xs, y_all=y_all, shape=shape, lower=lower, spacing=spacing, periodic=periodic, sigma=sigma, K=K,
                           columns=columns, walls=walls, cutoff=None if kind == "all" else 4.1, log_capacity=0 if kind == "all" else 64)
    return _LOOP[kind]


def _new_run(dev, kind):
    L = _loop(dev, kind)
    return mbias.PBMetadRun(L["model"], L["shape"], L["lower"], L["spacing"], KT, BIASFACTOR, HEIGHT, L["sigma"], periodic=L["periodic"],
                            cutoff=L["cutoff"], columns=L["columns"], walls=L["walls"], log_capacity=L["log_capacity"])


def _snapshot(run):
    torch.cuda.synchronize()
    return tuple(v.cpu() for v in ((run.table, run.state) + ((run.log,) if run.log is not None else ())))


def _eager_loop(dev, kind):
    key = kind + " eager"
    if key not in _LOOP:
        L, run = _loop(dev, kind), _new_run(dev, kind)
        steps = []
        for x in L["xs"]:
            y, e, dx = run.bias(x)
            assert run.deposit(y, e) is None
            steps.append(tuple(t.cpu() for t in (y, e, dx)) + (_snapshot(run),))
        _LOOP[key] = steps
        _LOOP[kind + " run"] = run
    return _LOOP[key]


@pytest.mark.parametrize("kind", ["all", "walls"])
def test_the_eager_loop_against_the_cpu_loop_of_the_host_twins(kind, hip_device):
    """Per step the device's y goes to the host: the energies from `molann_selftest_pbmetad_f64` on the host's tables, then the host
    twin's deposit.  The counts of the state are equal; sum_heights follows V, which the two sides interpolate from tables an ulp apart,
    so it is held to 1e-10 relative and printed."""
    dev = hip_device
    L, eager = _loop(dev, kind), _eager_loop(dev, kind)
    K, shape = L["K"], L["shape"]
    table, state = torch.zeros(sum(shape), dtype=F64), torch.zeros(8, dtype=F64)
    log = torch.zeros(L["log_capacity"], 2 * K, dtype=F64) if L["log_capacity"] else None
    tables = mbias.PBTables(table, shape, L["lower"], L["spacing"], L["periodic"], L["columns"])
    walls = None if L["walls"] is None else (L["walls"].center.cpu(), L["walls"].kappa.cpu(), None, None)
    inv_dT = 1.0 / (KT * (BIASFACTOR - 1.0))
    heights = torch.zeros(K, dtype=F64)
    worst_e = 0.0
    for i, (y, e, dx, after) in enumerate(eager):
        assert torch.equal(y, L["y_all"][WALKERS * i:WALKERS * (i + 1)])             # the outputs do not depend on the tables
        rows = [pc.host_frame(y[a].contiguous(), tables, KT, walls) for a in range(WALKERS)]
        assert all(code == 0 for code, _, _ in rows)
        he = torch.stack([r[1] for r in rows])
        scale = max(1.0, float(he.abs().max()))
        assert float((e - he).abs().max()) <= 1e-10 * scale, (i, e, he)
        worst_e = max(worst_e, float((e - he).abs().max()) / scale)
        step_log = torch.zeros(WALKERS, 2 * K, dtype=F64)
        assert pc.host_deposit(table.clone(), shape, L["lower"], L["spacing"], L["periodic"], L["sigma"], L["columns"], y, he[:, 2:], HEIGHT, inv_dT,
                               KT, L["cutoff"], torch.zeros(8, dtype=F64), step_log) == 0
        heights += step_log[:, K:].sum(dim=0)
        assert pc.host_deposit(table, shape, L["lower"], L["spacing"], L["periodic"], L["sigma"], L["columns"], y, he[:, 2:], HEIGHT, inv_dT, KT,
                               L["cutoff"], state, log) == 0
        got_state = after[1]
        assert got_state[[0, 1, 3, 4, 5, 6, 7]].tolist() == state[[0, 1, 3, 4, 5, 6, 7]].tolist(), i
        assert abs(float(got_state[2]) - float(state[2])) <= 1e-10 * float(state[2]), i
    final = eager[-1][3]
    offs = [sum(shape[:k]) for k in range(K + 1)]
    worst = max(float((final[0][offs[k]:offs[k + 1]] - table[offs[k]:offs[k + 1]]).abs().max()) / (pc.BOUND * float(heights[k])) for k in range(K))
    print("%s: 20 steps of 4 walkers, sum of heights %.6g: worst table error / bound %.3g; worst energies error / scale %.3g"
          % (kind, float(state[2]), worst, worst_e))
    assert worst <= 1.0
    assert state.tolist()[:2] == [STEPS * WALKERS, 0.0] and float(state[3]) == STEPS
    first = eager[0][1]
    assert float(first[:, 2:].abs().max()) == 0.0                         # zero tables: every V_k = 0 and V_PB = -kT log K
    assert float((first[:, 1] + KT * float(np.log(K))).abs().max()) <= 1e-10
    if kind == "all":
        assert float(eager[0][2].abs().max()) == 0.0                      # the first step's dx from the tables is exactly 0
    else:
        assert float(first[:, 0].min()) > 0.0 and float(state[4]) == 64.0 and torch.equal(final[2][:, :K], log[:, :K])
        assert float((final[2][:, K:] - log[:, K:]).abs().max()) <= 1e-10 * HEIGHT
        # the first step's dx is the walls' alone: value_and_restraint's bits
        _, _, dxr = L["model"].value_and_restraint(L["xs"][0], L["walls"].center, L["walls"].kappa)
        assert torch.equal(eager[0][2], dxr.cpu())
    assert float(eager[-1][2].abs().max()) > 0.0 and float(eager[-1][1][:, 2:].max()) > 0.0


@pytest.mark.parametrize("kind", ["all", "walls"])
def test_one_captured_graph_replays_the_loop(kind, hip_device):
    """One stream, two launches in a chain: the capture forks nowhere, so the graph is a line of two kernel nodes."""
    dev = hip_device
    L, eager = _loop(dev, kind), _eager_loop(dev, kind)
    run = _new_run(dev, kind)
    x_static = L["xs"][0].clone()
    into = (torch.empty(WALKERS, 8, dtype=F64, device=dev), torch.empty(WALKERS, 2 + L["K"], dtype=F64, device=dev), torch.empty_like(x_static))
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):               # a step outside the capture: plans, libraries and caches are made here
        run.deposit(*run.bias(x_static, into=into)[:2])
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    run.table.zero_(), run.state.zero_()
    if run.log is not None:
        run.log.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run.deposit(*run.bias(x_static, into=into)[:2])
    torch.cuda.synchronize()
    assert float(run.table.abs().max()) == 0.0 and float(run.state.abs().max()) == 0.0, "the capture ran the launches"
    for i, (x, (y, e, dx, after)) in enumerate(zip(L["xs"], eager)):
        x_static.copy_(x)
        graph.replay()
        got = tuple(u.cpu() for u in into)
        assert all(pl.same_bits(a, b) for a, b in zip(got, (y, e, dx))), "step %d: y, energies or dx" % i
        assert all(pl.same_bits(a, b) for a, b in zip(_snapshot(run), after)), "step %d: table, state or log" % i
    del graph


def test_hills_rebuilds_every_table_within_the_tables_bound(hip_device):
    """A run with a log and NO cutoff: `hills(k)` through `add_hills_to_grid` gives table k within 1e-12 (sum_a h_ak + max |T_k before|) -
    the tables start at zero - for the count read from the state and for a count the caller passes."""
    dev = hip_device
    L = _loop(dev, "walls")
    run = mbias.PBMetadRun(L["model"], L["shape"], L["lower"], L["spacing"], KT, BIASFACTOR, HEIGHT, L["sigma"], periodic=L["periodic"],
                           columns=L["columns"], walls=L["walls"], log_capacity=32)
    tables_after = []
    for x in L["xs"][:6]:
        y, e, _ = run.bias(x)
        run.deposit(y, e)
        tables_after.append(run.table.clone())
    assert run.read_state() == dict(run.read_state(), hills=24, refused=0, logged=24, steps=6)
    offs = [sum(L["shape"][:k]) for k in range(4)]
    for k in range(3):
        for n, after in ((None, tables_after[5]), (12, tables_after[2])):
            h = run.hills(k, n)
            assert h.centers.shape == (24 if n is None else n, 1) and h.sigma == [L["sigma"][k]]
            rebuilt = mbias.add_hills_to_grid(torch.zeros(L["shape"][k], dtype=F64, device=dev), [L["lower"][k]], [L["spacing"][k]],
                                              [L["periodic"][k]], h.centers, h.heights, h.sigma)
            tol = pc.tolerance(h.heights.cpu(), torch.zeros(1, dtype=F64))
            err = float((rebuilt - after[offs[k]:offs[k + 1]]).abs().max())
            print("hills(%d, %s): error %.3g, bound %.3g" % (k, n, err, tol))
            assert err <= tol and float(h.heights.sum()) > 0.0


def test_hills_hands_the_log_to_add_hills_to_grid(hip_device):
    dev = hip_device
    L, eager = _loop(dev, "walls"), _eager_loop(dev, "walls")
    run = _LOOP["walls run"]
    assert run.read_state() == dict(hills=80, refused=0, sum_heights=float(eager[-1][3][1][2]), steps=20, logged=64)
    assert [t.numel() for t in run.tables] == list(L["shape"]) and run.records().table.data_ptr() == run.table.data_ptr()
    after16 = eager[15][3][0]                                             # 64 hills: what the log holds
    offs = [sum(L["shape"][:k]) for k in range(4)]
    for k in range(3):
        h = run.hills(k)
        assert h.centers.shape == (64, 1) and h.columns == ((5, 0, 2)[k],) and (h.period is None) == (not L["periodic"][k])
        rebuilt = mbias.add_hills_to_grid(torch.zeros(L["shape"][k], dtype=F64, device=dev), [L["lower"][k]], [L["spacing"][k]], [L["periodic"][k]],
                                          h.centers, h.heights, h.sigma)
        # without the cutoff the run cuts them with: entries within exp(-4.1^2 / 2) of every height
        assert float((rebuilt.cpu() - after16[offs[k]:offs[k + 1]]).abs().max()) <= float(h.heights.sum()) * float(np.exp(-0.5 * 4.1 ** 2))
    with pytest.raises(IndexError):
        run.hills(3)
    with pytest.raises(ValueError, match="log"):
        _LOOP["all run"].hills(0) if "all run" in _LOOP else _new_run(dev, "all").hills(0)
