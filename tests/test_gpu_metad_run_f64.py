"""A whole metadynamics step on the device with no read-back: `MetadRun.bias` (`value_and_grid` / `value_and_bias` on the table as it
is) and metad_deposit_f64_kernel (`MetadRun.deposit`: the step's hills added to the table with well-tempered heights formed on the device).

  kernel  the device against its host twin `molann_selftest_metad_deposit_f64` (held against the numpy oracle on the host by
          tests/test_metad_deposit_f64_host.py) on that file's shapes and on shapes one entry past a tile (256; 16 x 16; 4 x 4 x 16)
          per axis, W in {1, 3, 64, 65, 257}, with and without a cutoff: every entry within tests/metad_cases.py's bound - the device's
          exp may differ from the host's by an ulp - and the counts equal.
  bits    two runs and split deposits: torch.equal.
  loop    bias then deposit, 20 steps of 4 walkers on C3's preprocessing behind a tanh head, plain and with walls and columns: the eager
          loop against the CPU loop of the host twins, and one captured graph of the two launches, replayed, against the eager bits."""

import math

import numpy as np
import pytest
import torch

import isolation
import metad_cases as mc
import metad_oracle as oracle
import placement as pl
import test_gpu_value_and_vjp_f64 as vv
from molann_amd import _capi
from molann_amd import bias as mbias

pytestmark = pytest.mark.gpu
F64, INF, NAN = mc.F64, mc.INF, mc.NAN
CPU = torch.device("cpu")
CUTOFF = 3.3


def _device(case, dev, cutoff=None, table=None, state=None, log=None, y=None, V=None):
    """One deposit of the case's walkers on the device through the ctypes wrapper: (table, state) on the device."""
    table = case.table.to(dev) if table is None else table
    state = torch.zeros(8, dtype=F64, device=dev) if state is None else state
    y = case.y.to(dev) if y is None else y
    V = case.V.contiguous().to(dev) if V is None else V
    arrays = _capi.metad_grid_arrays(case.shape, case.lower, case.spacing, case.periodic, case.sigma, case.columns)
    with torch.cuda.device(dev):
        _capi.metad_deposit_f64(table, arrays, y, V, mc.HEIGHT0, mc.INV_DT, cutoff, state, log)
    return table, state


def _host(case, cutoff=None, log=None):
    table, state = case.table.clone(), torch.zeros(8, dtype=F64)
    assert mc.host_deposit(table, case.lower, case.spacing, case.periodic, case.sigma, case.columns, case.y, case.V, cutoff=cutoff, state=state,
                           log=log) == 0
    return table, state


def _assert_same_step(case, got, want, what, cut=False):
    (table, state), (host_table, host_state) = got, want
    torch.cuda.synchronize()
    heights = mc.host_heights(case.V.contiguous())
    tol = mc.tolerance(heights, case.table)
    err = float((table.cpu() - host_table).abs().max())
    print("%s shape %s W %d: error %.3g, bound %.3g%s" % (what, case.shape, case.walkers, err, tol,
                                                         ", the host's bits" if pl.same_bits(table.cpu(), host_table) else ""))
    assert err <= tol, (err, tol)
    state = state.cpu()
    assert state[[0, 1, 3, 4, 5, 6, 7]].tolist() == host_state[[0, 1, 3, 4, 5, 6, 7]].tolist()
    assert abs(float(state[2]) - float(host_state[2])) <= 1e-12 * float(host_state[2])
    # within a cutoff no term underflows: where the host adds nothing the device adds nothing
    assert not cut or torch.equal(table.cpu() != case.table, host_table != case.table)


# ---------------------------------------------------------------------------------------------- the kernel against its host twin
@pytest.mark.parametrize("walkers", mc.WALKERS)
@pytest.mark.parametrize("shape,periodic", mc.SHAPES + mc.TILE_SHAPES)
def test_the_kernel_matches_its_host_twin(shape, periodic, walkers, hip_device):
    case = mc.Case(shape, periodic, walkers)
    _assert_same_step(case, _device(case, hip_device), _host(case), "no cutoff")
    cut = mc.Case(shape, periodic, walkers, start="random")
    assert oracle.cutoff_margin(shape, cut.lower, cut.spacing, cut.periodic, cut.sigma, None, cut.y.numpy(), CUTOFF) >= 1e-9
    _assert_same_step(cut, _device(cut, hip_device, CUTOFF), _host(cut, CUTOFF), "cutoff 3.3", cut=True)


def test_columns_strides_and_the_log(hip_device):
    dev = hip_device
    case = mc.Case((17, 33), (True, False), 65, n_out=5, columns=(3, 1), v_stride=3, v_offset=2, start="random")
    host_log = torch.zeros(70, 5, dtype=F64)
    want = _host(case, CUTOFF, log=host_log)
    store, log = case.v_store.to(dev), torch.zeros(70, 5, dtype=F64, device=dev)
    got = _device(case, dev, CUTOFF, V=store[:, 2], log=log)
    _assert_same_step(case, got, want, "columns (3, 1), V at stride 3", cut=True)
    assert float(got[1][4]) == 65.0 and torch.equal(log[:, :4].cpu(), host_log[:, :4]) and not bool(log[65:].any())
    assert float((log[:, 4].cpu() - host_log[:, 4]).abs().max()) <= 1e-14 * float(host_log[:, 4].max())
    # a log shorter than the step: the hills past it are deposited and counted all the same
    short = torch.zeros(3, 5, dtype=F64, device=dev)
    again = _device(case, dev, CUTOFF, V=store[:, 2], log=short)
    assert torch.equal(again[0], got[0]) and again[1].tolist() == [65.0, 0.0, float(got[1][2]), 1.0, 3.0, 0.0, 0.0, 0.0]
    assert torch.equal(short, log[:3])


# ---------------------------------------------------------------------------------------------- the same bits
@pytest.mark.parametrize("shape,periodic,w1,w2,cutoff", [((1025,), (True,), 3, 254, None), ((33, 65), (False, True), 64, 65, CUTOFF),
                                                         ((9, 17, 33), (True, False, False), 1, 128, None), ((5, 9, 17), (False, False, True), 70, 7, CUTOFF)])
def test_two_runs_and_split_deposits_give_the_same_bits(shape, periodic, w1, w2, cutoff, hip_device):
    dev = hip_device
    case = mc.Case(shape, periodic, w1 + w2, start="random")
    a, b = _device(case, dev, cutoff), _device(case, dev, cutoff)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    table, state = case.table.to(dev), torch.zeros(8, dtype=F64, device=dev)
    y, V = case.y.to(dev), case.V.to(dev)
    for rows in (slice(0, w1), slice(w1, w1 + w2)):             # queued back to back: nothing is read in between
        _device(case, dev, cutoff, table=table, state=state, y=y[rows], V=V[rows])
    assert torch.equal(table, a[0]) and torch.equal(state[:3], a[1][:3]) and state[3:].tolist() == [2.0, 0.0, 0.0, 0.0, 0.0]
    assert not torch.equal(table.cpu(), case.table)


# ---------------------------------------------------------------------------------------------- buffers and isolation
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("shape,periodic,cutoff", [((257,), (False,), None), ((17, 33), (True, False), CUTOFF), ((5, 9, 17), (False, False, True), None)])
def test_guard_bands_around_every_buffer(shape, periodic, cutoff, offset, hip_device):
    """The table, state, log, y and V in an arena of guard bands, every one `offset` doubles past a 16-byte boundary, y five columns wide
    and V a column of three: nothing before a buffer, nothing after it, the inputs as they were, and the bits of the plain call."""
    dev, d = hip_device, len(shape)
    columns = (3, 1, 4)[:d]
    case = mc.Case(shape, periodic, 65, n_out=5, columns=columns, v_stride=3, v_offset=2, start="random")
    want = _device(case, dev, cutoff, V=case.v_store.to(dev)[:, 2], log=torch.zeros(70, 2 * d + 1, dtype=F64, device=dev))
    arena = pl.Arena(dev, capacity=4 << 20)
    table = arena.carve("table", shape, F64, offset, row_dims=0)
    state, log = arena.carve("state", (8,), F64, offset, row_dims=0), arena.carve("log", (70, 2 * d + 1), F64, offset)
    y, store = arena.carve("y", case.y.shape, F64, offset, data=case.y), arena.carve("V", case.v_store.shape, F64, offset, data=case.v_store)
    table.copy_(case.table), state.zero_(), log.zero_()
    assert all(v.data_ptr() % 16 == 8 * offset for v in (table, state, log, y, store))
    got = _device(case, dev, cutoff, table=table, state=state, log=log, y=y, V=store[:, 2])
    torch.cuda.synchronize()
    assert arena.check() == [] and arena.inputs_changed() == []
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and float(state[4]) == 65.0 and not bool(log[65:].any())


@pytest.mark.parametrize("bad", ["nan_y", "inf_y", "nan_V", "overflow", "underflow"])
def test_an_invalid_walker_changes_no_entry(bad, hip_device):
    dev = hip_device
    case = mc.Case((9, 17, 33), (True, False, False), 66, start="random")
    a = 64                                           # the second chunk's first walker
    if bad in ("nan_y", "inf_y"):
        case.y[a, 1] = NAN if bad == "nan_y" else INF
    else:
        case.V[a] = {"nan_V": NAN, "overflow": -1e5, "underflow": 1e5}[bad]
    got = _device(case, dev)
    _assert_same_step(case, got, _host(case), bad)
    assert got[1][:2].tolist() == [65.0, 1.0]
    rest = [i for i in range(66) if i != a]
    others = _device(case, dev, y=case.y[rest].to(dev), V=case.V[rest].contiguous().to(dev))
    assert torch.equal(got[0], others[0]) and float(got[1][2]) == float(others[1][2])
    alone = _device(case, dev, y=case.y[a:a + 1].to(dev), V=case.V[a:a + 1].contiguous().to(dev))
    assert pl.same_bits(alone[0].cpu(), case.table) and alone[1].tolist() == [0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0]


def test_the_entrys_return_codes_launch_nothing(hip_device):
    dev = hip_device
    case = mc.Case((5, 7), (True, False), 3)
    table, state, y, V = case.table.to(dev), torch.zeros(8, dtype=F64, device=dev), case.y.to(dev), case.V.to(dev)
    L, stream = _capi.lib(), torch.cuda.current_stream().cuda_stream
    shape, lower, spacing, periodic, sigma, columns = _capi.metad_grid_arrays(case.shape, case.lower, case.spacing, case.periodic, case.sigma, None)

    def raw(**c):
        a = dict(table=table.data_ptr(), d=2, shape=shape, sigma=sigma, y=y.data_ptr(), y_stride=2, V=V.data_ptr(), n=3, height0=1.2, inv_dT=0.04,
                 cutoff=INF, state=state.data_ptr(), log=None, cap=0)
        a.update(c)
        return L.molann_metad_deposit_f64(a["table"], a["d"], a["shape"], lower, spacing, periodic, a["sigma"], columns, a["y"], a["y_stride"], a["V"], 1,
                                          a["n"], a["height0"], a["inv_dT"], a["cutoff"], a["state"], a["log"], a["cap"], stream)

    with torch.cuda.device(dev):
        assert raw(table=None) == _capi.E_NULL and raw(shape=None) == _capi.E_NULL and raw(V=None, d=7) == _capi.E_NULL
        assert raw(state=state.data_ptr() + 4) == _capi.E_ALIGNMENT and raw(y=y.data_ptr() + 4, d=0) == _capi.E_ALIGNMENT
        assert raw(d=4) == _capi.E_UNSUPPORTED and raw(d=0, height0=NAN) == _capi.E_UNSUPPORTED
        for change in (dict(height0=0.0), dict(inv_dT=-1.0), dict(cutoff=NAN), dict(cutoff=0.0), dict(n=-1), dict(y_stride=1), dict(cap=-1),
                       dict(sigma=(2 * __import__("ctypes").c_double)(0.3, 0.0))):
            assert raw(**change) == _capi.E_DESC, change
        assert raw(n=0) == 0
        torch.cuda.synchronize()
        assert not bool(table.any()) and not bool(state.any()), "a refusal launched"
        assert raw() == 0
        torch.cuda.synchronize()
        assert state.tolist()[:2] == [3.0, 0.0] and float(table.abs().max()) > 0.0


def test_the_operator_gives_the_ctypes_bits(hip_device):
    from molann_amd import script
    script.load_ops()
    dev = hip_device
    case = mc.Case((17, 33), (True, False), 65, n_out=5, columns=(3, 1), v_stride=3, v_offset=2, start="random")
    store = case.v_store.to(dev)
    want_log = torch.zeros(70, 5, dtype=F64, device=dev)
    want = _device(case, dev, CUTOFF, V=store[:, 2], log=want_log)
    table, state, log, y = case.table.to(dev), torch.zeros(8, dtype=F64, device=dev), torch.zeros(70, 5, dtype=F64, device=dev), case.y.to(dev)
    args = (case.lower, case.spacing, list(case.periodic), case.sigma, [3, 1], y, store[:, 2], mc.HEIGHT0, mc.INV_DT)
    assert torch.ops.molann.metad_step(table, state, log, *args, CUTOFF) is None
    assert torch.equal(table, want[0]) and torch.equal(state, want[1]) and torch.equal(log, want_log)
    assert torch.equal(store, case.v_store.to(dev)) and torch.equal(y, case.y.to(dev))
    none = _device(case, dev, None, V=store[:, 2])
    table2, state2 = case.table.to(dev), torch.zeros(8, dtype=F64, device=dev)
    torch.ops.molann.metad_step(table2, state2, None, *args, INF)
    assert torch.equal(table2, none[0]) and torch.equal(state2, none[1])
    with pytest.raises(ValueError, match="cutoff"):
        torch.ops.molann.metad_step(table, state, log, *args, 0.0)
    with pytest.raises(ValueError, match="state"):
        torch.ops.molann.metad_step(table, state[:4], log, *args, CUTOFF)
    with pytest.raises(ValueError, match="log"):
        torch.ops.molann.metad_step(table, state, log[:, :4], *args, CUTOFF)
    with pytest.raises(ValueError, match="table"):
        torch.ops.molann.metad_step(table[:, ::2], state, None, *args, CUTOFF)
    with pytest.raises(ValueError, match="columns"):
        torch.ops.molann.metad_step(table, state, log, case.lower, case.spacing, [], case.sigma, [3, 5], y, store[:, 2], 1.2, 0.04, CUTOFF)
    with pytest.raises(NotImplementedError):
        torch.ops.molann.metad_step(table.cpu(), state.cpu(), None, case.lower, case.spacing, [], case.sigma, [3, 1], y.cpu(), store[:, 2].cpu(), 1.2,
                                    0.04, CUTOFF)
    assert torch.equal(table, want[0]) and torch.equal(state, want[1])


# ---------------------------------------------------------------------------------------------- the loop
STEPS, WALKERS, KT, BIASFACTOR, HEIGHT = 20, 4, 2.494, 10.0, 1.2
_LOOP = {}


def _loop(dev, kind):
    """The model, the frames, a grid that covers the outputs and the run's arguments, once per kind: "plain" (a 2-output head, the table
    on both) or "walls" (a 4-output head, the table on outputs (2, 0), a restraint on all four, a cutoff and a log)."""
    if kind not in _LOOP:
        n_out, columns = (2, None) if kind == "plain" else (4, (2, 0))
        w, model, _ = vv._workload("C3", dev, head=[32, n_out], act=torch.nn.Tanh())
        xs = [w.make_frames(WALKERS, seed=700 + i).double().to(dev) for i in range(STEPS)]
        y_all = torch.cat([model.value_and_vjp(x, torch.zeros(WALKERS, n_out, dtype=F64, device=dev))[0] for x in xs]).cpu()
        cols = list(columns) if columns else [0, 1]
        lo, hi = y_all[:, cols].min(dim=0).values, y_all[:, cols].max(dim=0).values
        shape = (19, 23)
        periodic = [False, True] if kind == "plain" else [False, False]
        lower = [float(lo[k] - 0.15 * (hi[k] - lo[k])) for k in range(2)]
        spacing = [float(1.3 * (hi[k] - lo[k])) / (shape[k] - (0 if periodic[k] else 1)) for k in range(2)]
        sigma = [2.3 * s for s in spacing]
        walls = None
        if kind == "walls":
            centre = y_all.mean(dim=0)
            walls = mbias.Restraint(centre.to(dev), torch.tensor([3.0, 0.0, 5.0, 1.5], dtype=F64, device=dev))
        _LOOP[kind] = dict(w=w, model=model, xs=xs, y_all=y_all, shape=shape, lower=lower, spacing=spacing, periodic=periodic, sigma=sigma,
                           columns=columns, walls=walls, cutoff=None if kind == "plain" else 4.1, log_capacity=0 if kind == "plain" else 64)
    return _LOOP[kind]


def _new_run(dev, kind):
    L = _loop(dev, kind)
    return mbias.MetadRun(L["model"], torch.zeros(L["shape"], dtype=F64, device=dev), L["lower"], L["spacing"], KT, BIASFACTOR, HEIGHT, L["sigma"],
                          periodic=L["periodic"], cutoff=L["cutoff"], columns=L["columns"], walls=L["walls"], log_capacity=L["log_capacity"])


def _snapshot(run):
    torch.cuda.synchronize()
    return tuple(v.cpu() for v in ((run.table, run.state) + ((run.log,) if run.log is not None else ())))


def _eager_loop(dev, kind):
    """The eager loop, once: per step (y, bias or energies, dx) and the table, state and log after it, all on the CPU."""
    key = kind + " eager"
    if key not in _LOOP:
        L, run = _loop(dev, kind), _new_run(dev, kind)
        steps = []
        for x in L["xs"]:
            y, v, dx = run.bias(x)
            assert run.deposit(y, v) is None
            steps.append(tuple(t.cpu() for t in (y, v, dx)) + (_snapshot(run),))
        _LOOP[key] = steps
        _LOOP[kind + " run"] = run
    return _LOOP[key]


@pytest.mark.parametrize("kind", ["plain", "walls"])
def test_the_eager_loop_against_the_cpu_loop_of_the_host_twins(kind, hip_device):
    """Per step the device's y goes to the host: V from `molann_selftest_grid_f64` on the host's table, then the host twin's deposit.  The
    counts of the state are equal; sum_heights follows V, which the two sides interpolate from tables an ulp apart, so it is held to
    1e-10 relative (V's own bound times inv_dT < 1) and printed.  With walls the first step's dx is the restraint's, so there the
    table's own column of the energies is asserted to be exactly 0 in its place."""
    dev = hip_device
    L, eager = _loop(dev, kind), _eager_loop(dev, kind)
    shape, d = L["shape"], 2
    cols = list(L["columns"]) if L["columns"] else [0, 1]
    table, state = torch.zeros(shape, dtype=F64), torch.zeros(8, dtype=F64)
    log = torch.zeros(L["log_capacity"], 5, dtype=F64) if L["log_capacity"] else None
    shape_a, lower_a, spacing_a, periodic_a, _, _ = _capi.metad_grid_arrays(shape, L["lower"], L["spacing"], L["periodic"], L["sigma"], None)
    inv_dT = 1.0 / (KT * (BIASFACTOR - 1.0))
    heights_sum, worst_v = 0.0, 0.0
    for i, (y, v, dx, after) in enumerate(eager):
        assert torch.equal(y, L["y_all"][WALKERS * i:WALKERS * (i + 1)])             # the outputs do not depend on the table
        vg = v if kind == "plain" else v[:, 2]
        sel = y[:, cols].contiguous()
        hv = torch.tensor([_capi.lib().molann_selftest_grid_f64(sel[a].data_ptr(), d, table.data_ptr(), shape_a, lower_a, spacing_a, periodic_a, None)
                           for a in range(WALKERS)], dtype=F64)
        scale = float(table.abs().max())
        assert float((vg - hv).abs().max()) <= 1e-10 * scale, (i, vg, hv)
        worst_v = max(worst_v, float((vg - hv).abs().max()) / scale if scale else 0.0)
        assert mc.host_deposit(table, L["lower"], L["spacing"], L["periodic"], L["sigma"], L["columns"], y, hv, HEIGHT, inv_dT, L["cutoff"], state,
                               log) == 0
        heights_sum = float(state[2])
        got_state = after[1]
        assert got_state[[0, 1, 3, 4, 5, 6, 7]].tolist() == state[[0, 1, 3, 4, 5, 6, 7]].tolist(), i
        assert abs(float(got_state[2]) - heights_sum) <= 1e-10 * heights_sum, i
    final = eager[-1][3]
    err, tol = float((final[0] - table).abs().max()), mc.BOUND * heights_sum
    print("%s: 20 steps of 4 walkers, sum of heights %.6g (of %g): table error %.3g, bound %.3g; worst V error / scale %.3g; sum_heights %s"
          % (kind, heights_sum, STEPS * WALKERS * HEIGHT, err, tol, worst_v, "the host's bits" if float(final[1][2]) == heights_sum else "an ulp off"))
    assert err <= tol
    assert state.tolist()[:2] == [STEPS * WALKERS, 0.0] and float(state[3]) == STEPS and heights_sum < 0.9 * STEPS * WALKERS * HEIGHT
    if kind == "plain":
        assert float(eager[0][2].abs().max()) == 0.0
    else:
        first = eager[0][1]
        assert float(first[:, 2].abs().max()) == 0.0 and float(first[:, 1].abs().max()) == 0.0 and float(first[:, 0].min()) > 0.0
        assert float(state[4]) == 64.0 and torch.equal(final[2][:, :4], log[:, :4])
        assert float((final[2][:, 4] - log[:, 4]).abs().max()) <= 1e-10 * HEIGHT
    assert float(eager[-1][2].abs().max()) > 0.0
    last = eager[-1][1] if kind == "plain" else eager[-1][1][:, 2]
    assert float(last.max()) > 0.0                                                # walkers stand on the hills of earlier steps


@pytest.mark.parametrize("kind", ["plain", "walls"])
def test_one_captured_graph_replays_the_loop(kind, hip_device):
    """One stream, two launches in a chain: the capture forks nowhere, so the graph is a line of two kernel nodes."""
    dev = hip_device
    L, eager = _loop(dev, kind), _eager_loop(dev, kind)
    run = _new_run(dev, kind)
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
    run.table.zero_(), run.state.zero_()
    if run.log is not None:
        run.log.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        run.deposit(*run.bias(x_static, into=into)[:2])
    torch.cuda.synchronize()
    assert float(run.table.abs().max()) == 0.0 and float(run.state.abs().max()) == 0.0, "the capture ran the launches"
    for i, (x, (y, v, dx, after)) in enumerate(zip(L["xs"], eager)):
        x_static.copy_(x)
        graph.replay()
        got = tuple(u.cpu() for u in into)
        assert all(pl.same_bits(a, b) for a, b in zip(got, (y, v, dx))), "step %d: y, V or dx" % i
        assert all(pl.same_bits(a, b) for a, b in zip(_snapshot(run), after)), "step %d: table, state or log" % i


def test_a_nan_walker_changes_no_other_walkers_outputs_and_no_entry(hip_device):
    dev = hip_device
    L, eager = _loop(dev, "walls"), _eager_loop(dev, "walls")
    run = _new_run(dev, "walls")
    for dst, src in zip((run.table, run.state, run.log), eager[14][3]):
        dst.copy_(src.to(dev))
    x = L["xs"][15]
    clean = dict(zip(("y", "V", "dx"), run.bias(x)))
    assert all(pl.same_bits(clean[k].cpu(), want) for k, want in zip(("y", "V", "dx"), eager[15][:3]))
    bad_x = isolation.poison({"x": x}, [2], "nan", where={"x": 3 * isolation.chosen_atom([a - 1 for a in L["w"].align],
                                                                                       [(ty, [a - 1 for a in at]) for ty, at in L["w"].features])
                                                          + isolation.COORD})["x"]
    poisoned = dict(zip(("y", "V", "dx"), run.bias(bad_x)))
    torch.cuda.synchronize()
    assert isolation.keep_rows_equal(clean, poisoned, [2], ("y", "V", "dx")) == []
    assert not bool(torch.isfinite(poisoned["V"][2]).all())
    # the step refuses that walker alone: the table gets the other three's hills, bit for bit
    run.deposit(poisoned["y"], poisoned["V"])
    three = _new_run(dev, "walls")
    for dst, src in zip((three.table, three.state, three.log), eager[14][3]):
        dst.copy_(src.to(dev))
    keep = [0, 1, 3]
    three.deposit(clean["y"][keep], clean["V"][keep])
    assert torch.equal(run.table, three.table)
    a, b = run.read_state(), three.read_state()
    assert a == dict(b, refused=1) and a["hills"] == 15 * WALKERS + 3 and math.isfinite(a["sum_heights"])
    assert set(a) == {"hills", "refused", "sum_heights", "steps", "logged"}


def test_hills_hands_the_log_to_value_and_hills_and_add_hills_to_grid(hip_device):
    dev = hip_device
    L, eager = _loop(dev, "walls"), _eager_loop(dev, "walls")
    run = _LOOP["walls run"]
    record = run.hills()
    assert record.centers.shape == (64, 2) and record.columns == (2, 0) and record.period is None
    rebuilt = mbias.add_hills_to_grid(torch.zeros(L["shape"], dtype=F64, device=dev), L["lower"], L["spacing"], L["periodic"], record.centers,
                                      record.heights, record.sigma)
    # the first 64 of the 80 hills, without the cutoff the run cuts them with: entries within exp(-4.1^2 / 2) of every height
    assert float((rebuilt.cpu() - eager[15][3][0]).abs().max()) <= 64 * HEIGHT * math.exp(-0.5 * 4.1 ** 2)
    assert float((_snapshot(run)[0] - eager[15][3][0]).max()) > 0.0             # the last 16 hills are in the table and not in the log
    x = L["xs"][3]
    y, energies, _ = L["model"].value_and_bias(x, hills=record)
    direct = L["model"].value_and_bias(x, grid=mbias.Grid(rebuilt, L["lower"], L["spacing"], L["periodic"], (2, 0)))[1]
    torch.cuda.synchronize()
    # the hills themselves against the table they made, interpolated: cubic convolution of a Gaussian 2.3 spacings wide is good to about
    # 1 % of its height, and a wrong column order, width or height would be off by the bias itself
    print("hills %s against their table %s" % (energies[:, 1].tolist(), direct[:, 2].tolist()))
    assert float((energies[:, 1] - direct[:, 2]).abs().max()) <= 0.05 * float(energies[:, 1].abs().max())
    assert float(energies[:, 1].min()) > 0.0
