"""The reweighting offset c(t) of a metadynamics run on the device: `molann_metad_rct_f64` (metad_rct_partial_f64_kernel and
metad_rct_combine_f64_kernel, a chain of two launches) and `bias.MetadRun(rct_stride=)`.

  kernels  the device against its host twin `molann_selftest_metad_rct_f64` (held against the `np.longdouble` oracle on the host by
           tests/test_metad_rct_f64_host.py), against that oracle and against `kT (torch.logsumexp(a0 t) - torch.logsumexp(aV t))` on the
           device table, all within tests/metad_rct_cases.py's bound; where the device's exp gives the host's bits the results are equal,
           and how many are is printed.  One table has one chunk more than the partial launch has blocks.
  bits     two runs torch.equal; guard bands around partials and rct; table and state read only.
  loop     a 17 x 33 table with a cutoff, 4 walkers and 12 steps with rct_stride 1 and 3, plain and with walls and columns: the eager loop
           against the CPU loop of the host twins, and one captured graph of bias, deposit and the two rct launches, replayed, against the
           eager bits."""

import math

import pytest
import torch

import metad_cases as mc
import metad_rct_cases as rc
import metad_rct_oracle as oracle
import placement as pl
import test_gpu_value_and_vjp_f64 as vv
from molann_amd import _capi
from molann_amd import bias as mbias

pytestmark = pytest.mark.gpu
F64, INF, NAN, KT, INV_DT = rc.F64, rc.INF, rc.NAN, rc.KT, rc.INV_DT
MAX_BLOCKS = 1024                       # METAD_RCT_MAX_BLOCKS of molann_metad_rct.h: the partial launch's cap
_LOOP = {}
_BITS = {"equal": 0, "all": 0}


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_behind():
    """The module's shared runs, its models and its frames go when its last test has run, with the device idle: no later test of the
    session finds graphs, streams or device memory of this one."""
    yield
    import gc
    torch.cuda.synchronize()
    _LOOP.clear()
    gc.collect()
    torch.cuda.synchronize()


def _device(table, dev, kT=KT, inv_dT=INV_DT, state=None, stride=1, partials=None, rct=None):
    """One update on the device through the ctypes wrapper: (rct, partials) on the device; `table` may be a CPU tensor."""
    table = table.to(dev)
    partials = torch.zeros(rc.chunks(table.numel()), 4, dtype=F64, device=dev) if partials is None else partials
    rct = torch.zeros(8, dtype=F64, device=dev) if rct is None else rct
    with torch.cuda.device(dev):
        _capi.metad_rct_f64(table, kT, inv_dT, state, stride, partials, rct)
    return rct, partials


def _torch_route(table, kT, inv_dT):
    a0, t = 1.0 / kT + inv_dT, table.reshape(-1)
    return kT * (torch.logsumexp(a0 * t, 0) - torch.logsumexp(inv_dT * t, 0))


def _assert_device(table, dev, what, kT=KT, inv_dT=INV_DT):
    """The device against the twin, the oracle and the torch route on `table` (a CPU tensor)."""
    on_dev = table.to(dev)
    rct, partials = _device(on_dev, dev, kT, inv_dT)
    route = _torch_route(on_dev, kT, inv_dT)
    torch.cuda.synchronize()
    assert pl.same_bits(on_dev.cpu(), table)
    host, host_partials = rc.host_rct(table, kT, inv_dT)
    got, scale = rct.cpu(), rc.BOUND * (kT + abs(float(host[2])))
    same = pl.same_bits(got, host) and pl.same_bits(partials.cpu(), host_partials)
    _BITS["equal"] += int(same)
    _BITS["all"] += 1
    print("%s n %d: device c %.17g, host c %.17g, torch %.17g%s; bit for bit so far: %d of %d"
          % (what, table.numel(), float(got[0]), float(host[0]), float(route), ", the host's bits" if same else "", _BITS["equal"], _BITS["all"]))
    assert got[[1, 2, 5, 6, 7]].tolist() == host[[1, 2, 5, 6, 7]].tolist()
    assert abs(float(got[0]) - float(host[0])) <= scale
    assert all(abs(float(got[i]) - float(host[i])) <= rc.BOUND * max(1.0, abs(float(host[i]))) for i in (3, 4))
    rc.assert_close(got, table, kT, inv_dT, what + ", device against the oracle")
    assert abs(float(route) - float(got[0])) <= scale, (float(route), float(got[0]))
    return got


# ---------------------------------------------------------------------------------------------- the kernels against twin, oracle and torch
@pytest.mark.parametrize("which", sorted(rc.RANGES))
@pytest.mark.parametrize("n", rc.SIZES)
def test_the_kernels_match_twin_oracle_and_torch_on_uniform_tables(n, which, hip_device):
    table = rc.uniform_table(n, which)
    _assert_device(table, hip_device, which)
    plain = _assert_device(table, hip_device, which + ", plain", inv_dT=0.0)
    assert abs(float(plain[4]) - math.log(n)) <= rc.BOUND * max(1.0, math.log(n))


@pytest.mark.parametrize("shape", rc.GROWN)
def test_the_kernels_on_grown_tables(shape, hip_device):
    table = rc.grown_table(shape)
    got = _assert_device(table, hip_device, "grown %s" % (shape,))
    flat = _device(table.reshape(-1), hip_device)[0]
    assert pl.same_bits(flat.cpu(), got)


def test_one_chunk_more_than_the_launch_has_blocks(hip_device):
    n = MAX_BLOCKS * rc.CHUNK + 1
    assert rc.chunks(n) == MAX_BLOCKS + 1
    table = rc.uniform_table(n, "0..50 kT")
    table[-1] = 60.0 * KT                                    # the one entry of the last chunk, block 0's second, is the maximum
    got = _assert_device(table, hip_device, "past the cap")
    assert float(got[2]) == 60.0 * KT


@pytest.mark.parametrize("n", [257, 4097, 524289])
def test_two_runs_give_the_same_bits(n, hip_device):
    table = rc.uniform_table(n, "0..1000 kT").to(hip_device)
    a, b = _device(table, hip_device), _device(table, hip_device)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and float(a[0][1]) == 1.0


# ---------------------------------------------------------------------------------------------- spikes, constants, entries not finite
def test_spikes(hip_device):
    spike = 700.0 * KT
    for at in ([0], [63], [64], [255], [256], [2047], [2048], [4098], [5, 2053], [7, 263]):
        table = torch.zeros(4099, dtype=F64)
        table[at] = spike
        got = _assert_device(table, hip_device, "spike at %s" % at)
        assert float(got[2]) == spike


@pytest.mark.parametrize("n", rc.SIZES)
def test_constant_and_zero_tables_are_exact(n, hip_device):
    dev = hip_device
    rct = _device(torch.full((n,), 3.25, dtype=F64), dev)[0].cpu()
    assert float(rct[0]) == 3.25 and float(rct[2]) == 3.25
    zero, partials = _device(torch.zeros(n, dtype=F64), dev)
    zero = zero.cpu()
    assert float(zero[0]) == 0.0 and abs(math.exp(float(zero[3])) - n) <= 1e-12 * n
    assert float(partials[:, 1].sum()) == n and float(partials[:, 2].sum()) == n and not bool(partials[:, 3].any())
    minus = torch.zeros(n, dtype=F64)
    minus[::3] = -0.0
    assert pl.same_bits(_device(minus, dev)[0].cpu(), rc.host_rct(minus)[0])
    assert float(_device(torch.full((n,), -0.0, dtype=F64), dev)[0][0]) == 0.0


@pytest.mark.parametrize("n", [5, 4099])
def test_entries_that_are_not_finite(n, hip_device):
    dev = hip_device
    base = rc.uniform_table(n, "0..50 kT")
    for where in (0, n // 2, n - 1):
        for value in (NAN, INF, -INF):
            table = base.clone()
            table[where] = value
            on_dev = table.to(dev)
            rct = torch.zeros(8, dtype=F64, device=dev)
            rct[1] = 4.0
            _device(on_dev, dev, rct=rct)
            got = rct.cpu()
            assert float(got[6]) == 1.0 and float(got[1]) == 5.0 and float(got[7]) == 0.0
            assert all(math.isnan(float(got[i])) for i in (0, 2, 3, 4)), got
            assert pl.same_bits(on_dev.cpu(), table)


@pytest.mark.parametrize("stride", [1, 3, 7])
def test_the_stride_is_decided_on_the_device(stride, hip_device):
    dev = hip_device
    table = rc.uniform_table(4097, "0..50 kT").to(dev)
    always, always_partials = _device(table, dev)
    rows = rc.chunks(4097)
    for steps in list(range(9)) + [NAN, -5.0, 1e300]:
        state = torch.tensor([3.0, 1.0, 2.0, steps, 0.0, 0.0, 0.0, 0.0], dtype=F64)
        on_dev = state.to(dev)
        rct, partials = rc.marked(8).to(dev), rc.marked(rows, 4).to(dev)
        _device(table, dev, state=on_dev, stride=stride, partials=partials, rct=rct)
        due, recorded = oracle.due(steps, stride)
        assert pl.same_bits(on_dev.cpu(), state)
        if not due:
            assert pl.same_bits(rct.cpu(), rc.marked(8)) and pl.same_bits(partials.cpu(), rc.marked(rows, 4)), (steps, stride)
        else:
            assert torch.equal(partials, always_partials), (steps, stride)
            assert torch.equal(rct[[0, 2, 3, 4, 6, 7]], always[[0, 2, 3, 4, 6, 7]]) and float(rct[5]) == recorded and float(rct[1]) == 1.0


# ---------------------------------------------------------------------------------------------- buffers
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n", [5, 2049, 4097])
def test_guard_bands_and_read_only_inputs(n, offset, hip_device):
    """partials and rct in an arena of guard bands, `offset` doubles past a 16-byte boundary, with three rows of partials more than the
    call needs; the table and the state carved the same way as inputs."""
    dev = hip_device
    table = rc.uniform_table(n, "0..1000 kT")
    state = torch.tensor([3.0, 1.0, 2.0, 6.0, 0.0, 0.0, 0.0, 0.0], dtype=F64)
    want, want_partials = _device(table, dev, state=state.to(dev), stride=3)
    rows = rc.chunks(n)
    arena = pl.Arena(dev, capacity=4 << 20)
    t = arena.carve("table", (n,), F64, offset, data=table, row_dims=0)
    s = arena.carve("state", (8,), F64, offset, data=state, row_dims=0)
    partials = arena.carve("partials", (rows + 3, 4), F64, offset)
    rct = arena.carve("rct", (8,), F64, offset, row_dims=0)
    assert all(v.data_ptr() % 16 == 8 * offset for v in (t, s, partials, rct))
    _device(t, dev, state=s, stride=3, partials=partials, rct=rct)
    torch.cuda.synchronize()
    assert arena.check() == [] and arena.inputs_changed() == []
    assert torch.equal(rct, want) and torch.equal(partials[:rows], want_partials)
    assert bool((partials[rows:].contiguous().view(torch.int32) == pl.SENTINEL).all()), "a row past molann_metad_rct_chunks(n) was written"


def test_the_operator_gives_the_ctypes_bits(hip_device):
    from molann_amd import script
    script.load_ops()
    dev = hip_device
    table = rc.grown_table((33, 65)).to(dev)
    rows = rc.chunks(table.numel())
    state = torch.tensor([3.0, 1.0, 2.0, 6.0, 0.0, 0.0, 0.0, 0.0], dtype=F64, device=dev)
    want, want_partials = _device(table, dev, state=state, stride=3)
    partials, rct = torch.zeros(rows + 1, 4, dtype=F64, device=dev), torch.zeros(8, dtype=F64, device=dev)
    assert torch.ops.molann.metad_rct(table, state, partials, rct, KT, INV_DT, 3) is None
    assert torch.equal(rct, want) and torch.equal(partials[:rows], want_partials) and not bool(partials[rows:].any())
    torch.ops.molann.metad_rct(table, state, partials, rct, KT, INV_DT, 4)             # 6 is no multiple of 4: nothing is written
    assert torch.equal(rct, want)
    torch.ops.molann.metad_rct(table, None, partials, rct, KT, INV_DT, 4)
    assert float(rct[1]) == 2.0 and float(rct[5]) == 0.0 and float(rct[0]) == float(want[0])
    kept = rct.clone()
    with pytest.raises(ValueError, match="stride"):
        torch.ops.molann.metad_rct(table, state, partials, rct, KT, INV_DT, 0)
    with pytest.raises(ValueError, match="kT"):
        torch.ops.molann.metad_rct(table, state, partials, rct, 0.0, INV_DT, 1)
    with pytest.raises(ValueError, match="partials"):
        torch.ops.molann.metad_rct(table, state, partials[:rows - 1], rct, KT, INV_DT, 1)
    with pytest.raises(ValueError, match="rct"):
        torch.ops.molann.metad_rct(table, state, partials, rct[:4], KT, INV_DT, 1)
    with pytest.raises(ValueError, match="state"):
        torch.ops.molann.metad_rct(table, state[:4], partials, rct, KT, INV_DT, 1)
    with pytest.raises(ValueError, match="table"):
        torch.ops.molann.metad_rct(table[:, ::2], state, partials, rct, KT, INV_DT, 1)
    with pytest.raises(TypeError, match="float64"):
        torch.ops.molann.metad_rct(table.float(), state, partials, rct, KT, INV_DT, 1)
    with pytest.raises(NotImplementedError):
        torch.ops.molann.metad_rct(table.cpu(), None, partials.cpu(), rct.cpu(), KT, INV_DT, 1)
    assert torch.equal(rct, kept)


# ---------------------------------------------------------------------------------------------- the loop
STEPS, WALKERS, BIASFACTOR, HEIGHT, SHAPE, CUTOFF = 12, 4, rc.BIASFACTOR, 1.2, (17, 33), 4.1


def _loop(dev, kind):
    """The model, the frames, a grid that covers the outputs and the run's arguments, once per kind: "plain" (a 2-output head, the table
    on both) or "walls" (a 4-output head, the table on outputs (2, 0), a restraint on all four and a log), as
    tests/test_gpu_metad_run_f64.py has them."""
    if kind not in _LOOP:
        n_out, columns = (2, None) if kind == "plain" else (4, (2, 0))
        w, model, _ = vv._workload("C3", dev, head=[32, n_out], act=torch.nn.Tanh())
        xs = [w.make_frames(WALKERS, seed=700 + i).double().to(dev) for i in range(STEPS)]
        y_all = torch.cat([model.value_and_vjp(x, torch.zeros(WALKERS, n_out, dtype=F64, device=dev))[0] for x in xs]).cpu()
        cols = list(columns) if columns else [0, 1]
        lo, hi = y_all[:, cols].min(dim=0).values, y_all[:, cols].max(dim=0).values
        periodic = [False, True] if kind == "plain" else [False, False]
        lower = [float(lo[k] - 0.15 * (hi[k] - lo[k])) for k in range(2)]
        spacing = [float(1.3 * (hi[k] - lo[k])) / (SHAPE[k] - (0 if periodic[k] else 1)) for k in range(2)]
        walls = None
        if kind == "walls":
            walls = mbias.Restraint(y_all.mean(dim=0).to(dev), torch.tensor([3.0, 0.0, 5.0, 1.5], dtype=F64, device=dev))
        _LOOP[kind] = dict(model=model, xs=xs, y_all=y_all, lower=lower, spacing=spacing, periodic=periodic, sigma=[2.3 * s for s in spacing],
                           columns=columns, walls=walls, log_capacity=0 if kind == "plain" else 64)
    return _LOOP[kind]


def _new_run(dev, kind, rct_stride, table=None):
    L = _loop(dev, kind)
    table = torch.zeros(SHAPE, dtype=F64, device=dev) if table is None else table
    return mbias.MetadRun(L["model"], table, L["lower"], L["spacing"], KT, BIASFACTOR, HEIGHT, L["sigma"], periodic=L["periodic"], cutoff=CUTOFF,
                          columns=L["columns"], walls=L["walls"], log_capacity=L["log_capacity"], rct_stride=rct_stride)


def _snapshot(run):
    torch.cuda.synchronize()
    return tuple(v.cpu() for v in (run.table, run.state) + ((run.log,) if run.log is not None else ()) + ((run.rct,) if run.rct is not None else ()))


def _eager_loop(dev, kind, rct_stride):
    """The eager loop, once: per step (y, bias or energies, dx, rbias) and the table, state, log and rct after it, all on the CPU."""
    key = (kind, rct_stride)
    if key not in _LOOP:
        L, run = _loop(dev, kind), _new_run(dev, kind, rct_stride)
        steps = []
        for x in L["xs"]:
            y, v, dx = run.bias(x)
            assert run.deposit(y, v) is None
            rb = run.rbias(v) if rct_stride is not None else v
            steps.append(tuple(t.cpu() for t in (y, v, dx, rb)) + (_snapshot(run),))
        _LOOP[key] = steps
        _LOOP[key + ("run",)] = run
    return _LOOP[key]


@pytest.mark.parametrize("rct_stride", [1, 3])
@pytest.mark.parametrize("kind", ["plain", "walls"])
def test_the_eager_loop_against_the_cpu_loop_of_the_host_twins(kind, rct_stride, hip_device):
    """Per step the device's y goes to the host: V from `molann_selftest_grid_f64` on the host's table, the host twin's deposit, then the
    host twin's offset with the host's state and the stride.  `updates` and the steps at the update are equal; c and M follow tables an
    ulp apart (the reason tests/test_gpu_metad_run_f64.py gives for sum_heights) and are held to 1e-10 (kT + |M|), not to bits."""
    dev = hip_device
    L, eager = _loop(dev, kind), _eager_loop(dev, kind, rct_stride)
    cols = list(L["columns"]) if L["columns"] else [0, 1]
    table, state, rct = torch.zeros(SHAPE, dtype=F64), torch.zeros(8, dtype=F64), torch.zeros(8, dtype=F64)
    partials = torch.zeros(rc.chunks(table.numel()), 4, dtype=F64)
    log = torch.zeros(L["log_capacity"], 5, dtype=F64) if L["log_capacity"] else None
    shape_a, lower_a, spacing_a, periodic_a, _, _ = _capi.metad_grid_arrays(SHAPE, L["lower"], L["spacing"], L["periodic"], L["sigma"], None)
    worst = 0.0
    for i, (y, v, dx, rb, after) in enumerate(eager):
        sel = y[:, cols].contiguous()
        hv = torch.tensor([_capi.lib().molann_selftest_grid_f64(sel[a].data_ptr(), 2, table.data_ptr(), shape_a, lower_a, spacing_a, periodic_a, None)
                           for a in range(WALKERS)], dtype=F64)
        assert mc.host_deposit(table, L["lower"], L["spacing"], L["periodic"], L["sigma"], L["columns"], y, hv, HEIGHT, INV_DT, CUTOFF, state,
                               log) == 0
        rc.host_rct(table, state=state, stride=rct_stride, partials=partials, rct=rct)
        got = after[-1]
        assert got[[1, 5, 6, 7]].tolist() == rct[[1, 5, 6, 7]].tolist(), (i, got, rct)
        assert float(got[1]) == (i + 1) // rct_stride and float(got[5]) == (i + 1) // rct_stride * rct_stride
        tol = 1e-10 * (KT + abs(float(rct[2])))
        errs = [abs(float(got[k]) - float(rct[k])) for k in (0, 2)]
        worst = max(worst, max(errs) / tol)
        assert max(errs) <= tol, (i, got, rct)
        # rbias is V - c with the c the device held after this step's deposit
        vg = v if kind == "plain" else v[:, 2]
        assert torch.equal(rb, vg - got[0])
    final = eager[-1][4][-1]
    print("%s, stride %d: c %.12g, M %.12g after %d updates; worst error / bound %.3g" % (kind, rct_stride, float(final[0]), float(final[2]),
                                                                                         int(final[1]), worst))
    assert 0.0 < float(final[0]) < float(final[2]) and float(final[1]) == STEPS // rct_stride
    rc.assert_close(final, eager[-1][4][0], what="the device's offset of the device's table")
    run = _LOOP[(kind, rct_stride, "run")]
    assert run.read_rct() == dict(rct=float(final[0]), updates=STEPS // rct_stride, max=float(final[2]), log_sum_0=float(final[3]),
                                  log_sum_V=float(final[4]), steps=STEPS, bad=0)


@pytest.mark.parametrize("kind", ["plain", "walls"])
def test_the_offset_changes_nothing_else(kind, hip_device):
    dev = hip_device
    without, with_it = _eager_loop(dev, kind, None), _eager_loop(dev, kind, 3)
    assert _LOOP[(kind, None, "run")].rct is None and _LOOP[(kind, None, "run")].rct_stride is None
    for a, b in zip(without, with_it):
        assert all(torch.equal(p, q) for p, q in zip(a[:3], b[:3]))
        assert len(b[4]) == len(a[4]) + 1 and all(torch.equal(p, q) for p, q in zip(a[4], b[4][:-1]))
    with pytest.raises(ValueError, match="rct_stride"):
        _LOOP[(kind, None, "run")].rbias(without[0][1].to(dev))
    assert _new_run(dev, kind, 3).deposit(torch.zeros(0, 4, dtype=F64, device=dev), torch.zeros(0, dtype=F64, device=dev)) is None


def test_update_rct_on_a_loaded_table(hip_device):
    dev = hip_device
    loaded = _eager_loop(dev, "plain", 1)[-1][4][0]
    want = _eager_loop(dev, "plain", 1)[-1][4][-1]
    for stride in (None, 5):
        run = _new_run(dev, "plain", stride, table=loaded.to(dev))
        assert (run.rct is None) == (stride is None)
        assert run.update_rct() is None
        got = run.read_rct()
        assert got["rct"] == float(want[0]) and got["max"] == float(want[2]) and got["updates"] == 1 and got["steps"] == 0 and got["bad"] == 0
        run.update_rct()
        assert run.read_rct() == dict(got, updates=2)
        v = torch.tensor([0.5, 2.0], dtype=F64, device=dev)
        energies = torch.stack([v * 0, v * 0, v], dim=1)
        assert torch.equal(run.rbias(v), v - run.rct[0]) and torch.equal(run.rbias(energies), v - run.rct[0])
        with pytest.raises(ValueError):
            run.rbias(torch.zeros(2, 2, dtype=F64, device=dev))
        with pytest.raises(TypeError):
            run.rbias(v.float())


@pytest.mark.parametrize("kind", ["plain", "walls"])
def test_one_captured_graph_replays_the_loop_with_the_offset(kind, hip_device):
    """One stream, four launches in a chain - bias, deposit, the two of the offset: the capture forks nowhere.  The stride is 3 and the
    graph is one: the device decides from the state which replays update."""
    dev = hip_device
    L, eager = _loop(dev, kind), _eager_loop(dev, kind, 3)
    run = _new_run(dev, kind, 3)
    x_static = L["xs"][0].clone()
    n_out = L["y_all"].shape[1]
    into = (torch.empty(WALKERS, n_out, dtype=F64, device=dev), torch.empty((WALKERS,) if kind == "plain" else (WALKERS, 3), dtype=F64, device=dev),
            torch.empty_like(x_static))
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):               # a step outside the capture: plans, libraries and caches are made here
        run.deposit(*run.bias(x_static, into=into)[:2])
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    run.table.zero_(), run.state.zero_(), run.rct.zero_()
    if run.log is not None:
        run.log.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run.deposit(*run.bias(x_static, into=into)[:2])
    torch.cuda.synchronize()
    assert float(run.table.abs().max()) == 0.0 and float(run.state.abs().max()) == 0.0 and float(run.rct.abs().max()) == 0.0, "the capture ran"
    for i, (x, (y, v, dx, rb, after)) in enumerate(zip(L["xs"], eager)):
        x_static.copy_(x)
        graph.replay()
        got = tuple(u.cpu() for u in into)
        assert all(pl.same_bits(a, b) for a, b in zip(got, (y, v, dx))), "step %d: y, V or dx" % i
        assert all(pl.same_bits(a, b) for a, b in zip(_snapshot(run), after)), "step %d: table, state, log or rct" % i
    assert float(run.rct[1]) == STEPS // 3
    del graph
