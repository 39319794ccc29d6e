"""Adaptive, correlated metadynamics hills on the device with no read-back: metad_widths_f64_kernel (`MetadRun.observe` and the first
launch of an adaptive `MetadRun.deposit`) and metad_deposit_cov_f64_kernel (the hills with a full covariance matrix).

  kernel  the deposit against its host twin `molann_selftest_metad_deposit_cov_f64` (held against the numpy oracle on the host by
          tests/test_metad_cov_f64_host.py) on tests/metad_cov_cases.py's shapes, W in {1, 3, 8, 9, 64, 65, 257}, with and without a cutoff:
          every entry within the bound - the device's exp may differ from the host's by an ulp - the counts equal, and under the cutoff
          the same entries changed.  The widths launch against its twin on 257 walkers (two rounds of the block).
  bits    two runs and split deposits: torch.equal.
  loop    bias, observe and deposit, 20 steps of 4 walkers on C3's preprocessing behind a tanh head: "diff" and "geom", plain and with
          walls, columns and rct_stride=2: the eager loop against the CPU loop of the host twins, and one captured graph of the step's
          launches, replayed, against the eager bits."""

import numpy as np
import pytest
import torch

import metad_cases as mc
import metad_cov_cases as cc
import metad_cov_oracle as oracle
import metad_rct_cases as rc
import placement as pl
import test_gpu_value_and_vjp_f64 as vv
from molann_amd import _capi
from molann_amd import bias as mbias

pytestmark = pytest.mark.gpu
F64, INF, NAN = cc.F64, cc.INF, cc.NAN
CUTOFF = 3.3


def _device(case, dev, cutoff=None, table=None, state=None, log=None, y=None, V=None, cov=None):
    """One covariant deposit of the case's walkers on the device through the ctypes wrapper: (table, state) on the device."""
    table = case.table.to(dev) if table is None else table
    state = torch.zeros(8, dtype=F64, device=dev) if state is None else state
    y = case.y.to(dev) if y is None else y
    V = case.V.contiguous().to(dev) if V is None else V
    cov = case.cov.contiguous().to(dev) if cov is None else cov
    arrays = _capi.metad_grid_arrays(case.shape, case.lower, case.spacing, case.periodic, case.sigma, case.columns)
    with torch.cuda.device(dev):
        _capi.metad_deposit_cov_f64(table, arrays, y, V, cov, cc.HEIGHT0, cc.INV_DT, cutoff, state, log)
    return table, state


def _host(case, cutoff=None, log=None):
    table, state = case.table.clone(), torch.zeros(8, dtype=F64)
    assert cc.host_deposit_cov(table, case.lower, case.spacing, case.periodic, case.columns, case.y, case.V, case.cov, cutoff=cutoff, state=state,
                               log=log) == 0
    return table, state


def _assert_same_step(case, got, want, what, cut=False, heights=None):
    (table, state), (host_table, host_state) = got, want
    torch.cuda.synchronize()
    heights = mc.host_heights(case.V.contiguous()) if heights is None else heights
    tol = cc.tolerance(heights, case.table)
    err = float((table.cpu() - host_table).abs().max())
    print("%s shape %s W %d: error %.3g, bound %.3g%s" % (what, case.shape, case.walkers, err, tol,
                                                         ", the host's bits" if pl.same_bits(table.cpu(), host_table) else ""))
    assert err <= tol, (err, tol)
    state = state.cpu()
    assert state[[0, 1, 3, 4, 5, 6, 7]].tolist() == host_state[[0, 1, 3, 4, 5, 6, 7]].tolist()
    assert abs(float(state[2]) - float(host_state[2])) <= 1e-12 * float(host_state[2])
    assert not cut or torch.equal(table.cpu() != case.table, host_table != case.table)


# ---------------------------------------------------------------------------------------------- the kernels against their host twins
@pytest.mark.parametrize("walkers", cc.WALKERS)
@pytest.mark.parametrize("shape,periodic", cc.SHAPES + cc.TILE_SHAPES)
def test_the_deposit_matches_its_host_twin(shape, periodic, walkers, hip_device):
    case = cc.CovCase(shape, periodic, walkers)
    _assert_same_step(case, _device(case, hip_device), _host(case), "no cutoff")
    cut = cc.CovCase(shape, periodic, walkers, start="random")
    assert oracle.cutoff_margin(shape, cut.lower, cut.spacing, cut.periodic, None, cut.y.numpy(), cut.cov.numpy(), CUTOFF) >= 1e-9
    _assert_same_step(cut, _device(cut, hip_device, CUTOFF), _host(cut, CUTOFF), "cutoff 3.3", cut=True)


@pytest.mark.parametrize("shape,periodic", [((67,), (True,)), ((5, 7), (True, False)), ((4, 5, 6), (False, True, False))])
def test_the_widths_launch_matches_its_host_twin(shape, periodic, hip_device):
    """257 walkers - the block's loop runs twice - through 12 observations with a window of 5, emitting on every third, one walker's y
    not finite once; then GEOM with limits from a random metric on reversed columns."""
    dev = hip_device
    case = cc.CovCase(shape, periodic, 257)
    d, T, W = case.d, case.T, 257
    rng = np.random.RandomState(9)
    span = np.asarray(case.spacing)
    ys = case.y.numpy()[None, :, :d] + np.cumsum(rng.normal(size=(12, W, d)) * 0.8 * span + 0.9 * span, axis=0)
    ys[4, 200, d - 1] = NAN
    arrays = _capi.metad_grid_arrays(shape, case.lower, case.spacing, case.periodic, case.sigma, None)
    none = _capi.metad_limit_arrays(None, None, d)
    adapt, state, cov = torch.zeros(W, 1 + d + T, dtype=F64, device=dev), torch.zeros(8, dtype=F64, device=dev), torch.zeros(W, T, dtype=F64, device=dev)
    h_adapt, h_state, h_cov = torch.zeros(W, 1 + d + T, dtype=F64), torch.zeros(8, dtype=F64), torch.zeros(W, T, dtype=F64)
    with torch.cuda.device(dev):
        for i, y in enumerate(ys):
            emit = i % 3 == 2
            _capi.metad_widths_f64(arrays, none, _capi.METAD_COV_DIFF, 5, emit, adapt, state, cov, y=torch.from_numpy(y.copy()).to(dev))
            assert cc.host_widths(shape, case.lower, case.spacing, case.periodic, case.sigma, None, cc.DIFF, 5, emit, h_adapt, h_state, h_cov,
                                  y=torch.from_numpy(y.copy())) == 0
    torch.cuda.synchronize()
    assert state.cpu().tolist() == h_state.tolist() == [12.0 * W - 1, 4.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    for name, got, want in (("adapt", adapt, h_adapt), ("cov", cov, h_cov)):
        err, scale = float((got.cpu() - want).abs().max()), float(want.abs().max())
        print("%s shape %s: error %.3g of scale %.3g%s" % (name, shape, err, scale, ", the host's bits" if pl.same_bits(got.cpu(), want) else ""))
        assert err <= 1e-13 * scale
    assert float(adapt[200, 0]) == 11.0 and torch.equal(adapt[:, 0].cpu(), h_adapt[:, 0])
    n_out = d + 1
    J = rng.normal(size=(W, n_out, 5))
    metric = torch.from_numpy(np.einsum("wik,wjk->wij", J, J))
    columns = list(range(n_out))[::-1][:d]
    g_arrays = _capi.metad_grid_arrays(shape, case.lower, case.spacing, case.periodic, case.sigma, columns)
    lo, hi = [0.9 * s for s in case.sigma], [2.5 * s for s in case.sigma]
    with torch.cuda.device(dev):
        _capi.metad_widths_f64(g_arrays, _capi.metad_limit_arrays(lo, hi, d), _capi.METAD_COV_GEOM, 1, True, None, state, cov, metric=metric.to(dev))
    assert cc.host_widths(shape, case.lower, case.spacing, case.periodic, case.sigma, columns, cc.GEOM, 1, True, None, h_state, h_cov, metric=metric,
                          sigma_min=lo, sigma_max=hi) == 0
    torch.cuda.synchronize()
    assert state.cpu().tolist() == h_state.tolist() and float(state[1]) == 5.0
    err, scale = float((cov.cpu() - h_cov).abs().max()), float(h_cov.abs().max())
    print("geom cov shape %s: error %.3g of scale %.3g%s" % (shape, err, scale, ", the host's bits" if pl.same_bits(cov.cpu(), h_cov) else ""))
    assert err <= 1e-13 * scale


def test_columns_strides_and_the_log(hip_device):
    dev = hip_device
    case = cc.CovCase((17, 33), (True, False), 65, n_out=5, columns=(3, 1), v_stride=3, v_offset=2, cov_width=7, cov_offset=2, start="random")
    host_log = torch.zeros(70, 6, dtype=F64)
    want = _host(case, CUTOFF, log=host_log)
    store, cstore, log = case.v_store.to(dev), case.cov_store.to(dev), torch.zeros(70, 6, dtype=F64, device=dev)
    got = _device(case, dev, CUTOFF, V=store[:, 2], cov=cstore[:, 2:5], log=log)
    _assert_same_step(case, got, want, "columns (3, 1), V at stride 3, cov at stride 7", cut=True)
    assert float(got[1][4]) == 65.0 and torch.equal(log[:, :5].cpu(), host_log[:, :5]) and not bool(log[65:].any())
    assert float((log[:, 5].cpu() - host_log[:, 5]).abs().max()) <= 1e-14 * float(host_log[:, 5].max())
    assert torch.equal(store, case.v_store.to(dev)) and torch.equal(cstore, case.cov_store.to(dev))
    # a log shorter than the step: the hills past it are deposited and counted all the same
    short = torch.zeros(3, 6, dtype=F64, device=dev)
    again = _device(case, dev, CUTOFF, V=store[:, 2], cov=cstore[:, 2:5], log=short)
    assert torch.equal(again[0], got[0]) and again[1].tolist() == [65.0, 0.0, float(got[1][2]), 1.0, 3.0, 0.0, 0.0, 0.0]
    assert torch.equal(short, log[:3])


# ---------------------------------------------------------------------------------------------- the same bits
@pytest.mark.parametrize("shape,periodic,w1,w2,cutoff", [((1025,), (True,), 3, 254, None), ((33, 65), (False, True), 64, 65, CUTOFF),
                                                         ((9, 17, 33), (True, False, False), 1, 128, None), ((5, 9, 17), (False, False, True), 70, 7, CUTOFF)])
def test_two_runs_and_split_deposits_give_the_same_bits(shape, periodic, w1, w2, cutoff, hip_device):
    dev = hip_device
    case = cc.CovCase(shape, periodic, w1 + w2, start="random")
    a, b = _device(case, dev, cutoff), _device(case, dev, cutoff)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    table, state = case.table.to(dev), torch.zeros(8, dtype=F64, device=dev)
    y, V, cov = case.y.to(dev), case.V.to(dev), case.cov.contiguous().to(dev)
    for rows in (slice(0, w1), slice(w1, w1 + w2)):             # queued back to back: nothing is read in between
        _device(case, dev, cutoff, table=table, state=state, y=y[rows], V=V[rows], cov=cov[rows])
    assert torch.equal(table, a[0]) and torch.equal(state[:3], a[1][:3]) and state[3:].tolist() == [2.0, 0.0, 0.0, 0.0, 0.0]
    assert not torch.equal(table.cpu(), case.table)


# ---------------------------------------------------------------------------------------------- buffers and isolation
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("shape,periodic,cutoff", [((257,), (False,), None), ((17, 33), (True, False), CUTOFF), ((5, 9, 17), (False, False, True), None)])
def test_guard_bands_around_every_buffer(shape, periodic, cutoff, offset, hip_device):
    """The table, state, log, y, V, cov, adapt and adapt_state in an arena of guard bands, every one `offset` doubles past a 16-byte
    boundary, y five columns wide, V a column of three and cov columns of a wider tensor: nothing before a buffer, nothing after it, the
    inputs as they were, and the bits of the plain calls."""
    dev, d = hip_device, len(shape)
    columns = (3, 1, 4)[:d]
    case = cc.CovCase(shape, periodic, 65, n_out=5, columns=columns, v_stride=3, v_offset=2, cov_width=9, cov_offset=1, start="random")
    T = case.T
    want = _device(case, dev, cutoff, V=case.v_store.to(dev)[:, 2], cov=case.cov_store.to(dev)[:, 1:1 + T],
                   log=torch.zeros(70, d + T + 1, dtype=F64, device=dev))
    arena = pl.Arena(dev, capacity=4 << 20)
    table = arena.carve("table", shape, F64, offset, row_dims=0)
    state, log = arena.carve("state", (8,), F64, offset, row_dims=0), arena.carve("log", (70, d + T + 1), F64, offset)
    y, store = arena.carve("y", case.y.shape, F64, offset, data=case.y), arena.carve("V", case.v_store.shape, F64, offset, data=case.v_store)
    cstore = arena.carve("cov", case.cov_store.shape, F64, offset, data=case.cov_store)
    table.copy_(case.table), state.zero_(), log.zero_()
    assert all(v.data_ptr() % 16 == 8 * offset for v in (table, state, log, y, store, cstore))
    got = _device(case, dev, cutoff, table=table, state=state, log=log, y=y, V=store[:, 2], cov=cstore[:, 1:1 + T])
    torch.cuda.synchronize()
    assert arena.check() == [] and arena.inputs_changed() == []
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and float(state[4]) == 65.0 and not bool(log[65:].any())
    # the widths launch: adapt, adapt_state and cov_out written in place, y read in place
    adapt, astate, out = arena.carve("adapt", (65, 1 + d + T), F64, offset), arena.carve("astate", (8,), F64, offset, row_dims=0), \
        arena.carve("out", (65, T), F64, offset)
    adapt.zero_(), astate.zero_(), out.zero_()
    plain = (torch.zeros(65, 1 + d + T, dtype=F64, device=dev), torch.zeros(8, dtype=F64, device=dev), torch.zeros(65, T, dtype=F64, device=dev))
    arrays = _capi.metad_grid_arrays(shape, case.lower, case.spacing, case.periodic, case.sigma, columns)
    none = _capi.metad_limit_arrays(None, None, d)
    with torch.cuda.device(dev):
        for emit in (False, True):
            _capi.metad_widths_f64(arrays, none, _capi.METAD_COV_DIFF, 1, emit, adapt, astate, out, y=y)
            _capi.metad_widths_f64(arrays, none, _capi.METAD_COV_DIFF, 1, emit, plain[0], plain[1], plain[2], y=case.y.to(dev))
    torch.cuda.synchronize()
    assert arena.check() == [] and arena.inputs_changed() == []
    assert torch.equal(adapt, plain[0]) and torch.equal(astate, plain[1]) and torch.equal(out, plain[2]) and float(astate[0]) == 130.0


@pytest.mark.parametrize("bad", ["nan_y", "nan_cov", "singular", "overflow"])
def test_an_invalid_walker_changes_no_entry(bad, hip_device):
    dev = hip_device
    case = cc.CovCase((9, 17, 33), (True, False, False), 66, start="random")
    a = 64                                           # the second chunk's first walker
    if bad == "nan_y":
        case.y[a, 1] = NAN
    elif bad == "nan_cov":
        case.cov[a, 4] = NAN
    elif bad == "singular":
        case.cov[a] = 1.0
    else:
        case.V[a] = -1e5
    rest = [i for i in range(66) if i != a]
    heights = mc.host_heights(case.V[rest].contiguous())
    got = _device(case, dev)
    _assert_same_step(case, got, _host(case), bad, heights=heights)
    assert got[1][:2].tolist() == [65.0, 1.0]
    others = _device(case, dev, y=case.y[rest].to(dev), V=case.V[rest].contiguous().to(dev), cov=case.cov[rest].contiguous().to(dev))
    assert torch.equal(got[0], others[0]) and float(got[1][2]) == float(others[1][2])
    alone = _device(case, dev, y=case.y[a:a + 1].to(dev), V=case.V[a:a + 1].contiguous().to(dev), cov=case.cov[a:a + 1].contiguous().to(dev))
    assert pl.same_bits(alone[0].cpu(), case.table) and alone[1].tolist() == [0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0]


def test_the_entries_return_codes_launch_nothing(hip_device):
    dev = hip_device
    case = cc.CovCase((5, 7), (True, False), 3)
    table, state, y, V, cov = case.table.to(dev), torch.zeros(8, dtype=F64, device=dev), case.y.to(dev), case.V.to(dev), case.cov.contiguous().to(dev)
    adapt, astate = torch.zeros(3, 6, dtype=F64, device=dev), torch.zeros(8, dtype=F64, device=dev)
    L, stream = _capi.lib(), torch.cuda.current_stream().cuda_stream
    shape, lower, spacing, periodic, sigma, columns = _capi.metad_grid_arrays(case.shape, case.lower, case.spacing, case.periodic, case.sigma, None)

    def deposit(**c):
        a = dict(table=table.data_ptr(), d=2, shape=shape, y=y.data_ptr(), y_stride=2, V=V.data_ptr(), cov=cov.data_ptr(), cs=3, n=3, height0=1.2,
                 inv_dT=0.04, cutoff=INF, state=state.data_ptr(), log=None, cap=0)
        a.update(c)
        return L.molann_metad_deposit_cov_f64(a["table"], a["d"], a["shape"], lower, spacing, periodic, columns, a["y"], a["y_stride"], a["V"], 1,
                                              a["cov"], a["cs"], a["n"], a["height0"], a["inv_dT"], a["cutoff"], a["state"], a["log"], a["cap"], stream)

    def widths(**c):
        a = dict(d=2, shape=shape, sigma=sigma, y=y.data_ptr(), y_stride=2, n=3, mode=1, window=5, emit=1, adapt=adapt.data_ptr(),
                 astate=astate.data_ptr(), cov=cov.data_ptr(), cs=3)
        a.update(c)
        return L.molann_metad_widths_f64(a["d"], a["shape"], lower, spacing, periodic, a["sigma"], None, None, columns, a["y"], a["y_stride"], None, 0, 0,
                                         a["n"], a["mode"], a["window"], a["emit"], a["adapt"], a["astate"], a["cov"], a["cs"], stream)

    with torch.cuda.device(dev):
        assert deposit(table=None) == _capi.E_NULL and deposit(cov=None, d=7) == _capi.E_NULL
        assert deposit(cov=cov.data_ptr() + 4, d=0) == _capi.E_ALIGNMENT
        assert deposit(d=4) == _capi.E_UNSUPPORTED and deposit(d=0, height0=NAN) == _capi.E_UNSUPPORTED
        for change in (dict(height0=0.0), dict(cutoff=NAN), dict(n=-1), dict(y_stride=1), dict(cap=-1), dict(cs=2), dict(cs=-3)):
            assert deposit(**change) == _capi.E_DESC, change
        assert widths(astate=None) == _capi.E_NULL and widths(adapt=None) == _capi.E_NULL and widths(mode=2) == _capi.E_NULL
        assert widths(adapt=adapt.data_ptr() + 4, d=0) == _capi.E_ALIGNMENT and widths(d=4, window=0) == _capi.E_UNSUPPORTED
        for change in (dict(mode=3), dict(window=0), dict(cs=2), dict(y_stride=1), dict(n=-1)):
            assert widths(**change) == _capi.E_DESC, change
        assert deposit(n=0) == 0 and widths(n=0) == 0
        torch.cuda.synchronize()
        assert not bool(table.any()) and not bool(state.any()) and not bool(adapt.any()) and not bool(astate.any()), "a refusal launched"
        assert torch.equal(cov.cpu(), case.cov)
        assert deposit() == 0
        torch.cuda.synchronize()
        assert state.tolist()[:2] == [3.0, 0.0] and float(table.abs().max()) > 0.0


# ---------------------------------------------------------------------------------------------- the loop
STEPS, WALKERS, KT, BIASFACTOR, HEIGHT, WINDOW = 20, 4, 2.494, 10.0, 1.2, 5
KINDS = ["diff", "diff walls", "geom", "geom walls"]
_LOOP = {}


def _loop(dev, kind):
    """The model, the frames, a grid that covers the outputs and the run's arguments, once per kind: plain (a 2-output head, the table on
    both, axis 1 periodic) or "walls" (a 4-output head, the table on outputs (2, 0), a restraint on all four, a cutoff, a log and
    rct_stride=2).  Between two deposits a "diff" run observes the outputs of two more frames per walker."""
    if kind not in _LOOP:
        mode, walls_kind = kind.split()[0], kind.endswith("walls")
        n_out, columns = (4, (2, 0)) if walls_kind else (2, None)
        w, model, _ = vv._workload("C3", dev, head=[32, n_out], act=torch.nn.Tanh())
        xs = [w.make_frames(WALKERS, seed=700 + i).double().to(dev) for i in range(3 * STEPS)]
        zero = torch.zeros(WALKERS, n_out, dtype=F64, device=dev)
        ys = [model.value_and_vjp(x, zero)[0] for x in xs]
        y_all = torch.cat(ys).cpu()
        cols = list(columns) if columns else [0, 1]
        lo, hi = y_all[:, cols].min(dim=0).values, y_all[:, cols].max(dim=0).values
        shape = (19, 23)
        periodic = [False, False] if walls_kind else [False, True]
        lower = [float(lo[k] - 0.15 * (hi[k] - lo[k])) for k in range(2)]
        spacing = [float(1.3 * (hi[k] - lo[k])) / (shape[k] - (0 if periodic[k] else 1)) for k in range(2)]
        if mode == "diff":
            sigma = [2.3 * s for s in spacing]
        else:                                        # a length in the metric's units: about 2.3 spacings at the median metric
            M = torch.cat([model.value_and_metric(x)[1] for x in xs[:STEPS]]).cpu()
            sigma = [2.3 * spacing[k] / float(M[:, cols[k], cols[k]].median().sqrt()) for k in range(2)]
        walls = None
        if walls_kind:
            walls = mbias.Restraint(y_all.mean(dim=0).to(dev), torch.tensor([3.0, 0.0, 5.0, 1.5], dtype=F64, device=dev))
        _LOOP[kind] = dict(mode=mode, model=model, xs=xs[:STEPS], between=[(ys[STEPS + 2 * i], ys[STEPS + 2 * i + 1]) for i in range(STEPS)],
                           y_all=y_all, shape=shape, lower=lower, spacing=spacing, periodic=periodic, sigma=sigma, columns=columns, walls=walls,
                           cutoff=4.1 if walls_kind else None, log_capacity=64 if walls_kind else 0, rct_stride=2 if walls_kind else None,
                           sigma_min=[0.5 * s for s in spacing], sigma_max=[6.0 * s for s in spacing])
    return _LOOP[kind]


def _new_run(dev, kind):
    L = _loop(dev, kind)
    return mbias.MetadRun(L["model"], torch.zeros(L["shape"], dtype=F64, device=dev), L["lower"], L["spacing"], KT, BIASFACTOR, HEIGHT, L["sigma"],
                          periodic=L["periodic"], cutoff=L["cutoff"], columns=L["columns"], walls=L["walls"], log_capacity=L["log_capacity"],
                          rct_stride=L["rct_stride"], adaptive=L["mode"], window=WINDOW if L["mode"] == "diff" else None, sigma_min=L["sigma_min"],
                          sigma_max=L["sigma_max"], walkers=WALKERS)


def _snapshot(run):
    torch.cuda.synchronize()
    return tuple(v.cpu() for v in (run.table, run.state, run.adapt, run.adapt_state, run.cov) + ((run.log,) if run.log is not None else ())
                 + ((run.rct,) if run.rct is not None else ()))


def _step(run, L, x, between, into=None, metric_into=None):
    y, v, dx = run.bias(x, into=into)
    if L["mode"] == "geom":
        metric = L["model"].value_and_metric(x, into=metric_into)[1]
        assert run.deposit(y, v, metric=metric) is None
    else:
        metric = None
        assert run.deposit(y, v) is None
        for y_mid in between:
            assert run.observe(y_mid) is None
    return y, v, dx, metric


def _eager_loop(dev, kind):
    """The eager loop, once: per step (y, bias or energies, dx, metric) and the run's buffers after it, all on the CPU."""
    key = kind + " eager"
    if key not in _LOOP:
        L, run = _loop(dev, kind), _new_run(dev, kind)
        steps = []
        for x, between in zip(L["xs"], L["between"]):
            out = _step(run, L, x, between)
            steps.append(tuple(None if t is None else t.cpu() for t in out) + (_snapshot(run),))
        _LOOP[key] = steps
        _LOOP[kind + " run"] = run
    return _LOOP[key]


@pytest.mark.parametrize("kind", KINDS)
def test_the_eager_loop_against_the_cpu_loop_of_the_host_twins(kind, hip_device):
    """Per step the device's y (and metric) go to the host: V from `molann_selftest_grid_f64` on the host's table, then the host twins'
    widths and deposit.  The counts are equal; the running statistics follow y alone and are held to 1e-13 of their scale;
    sum_heights follows V, which the two sides interpolate from tables an ulp apart, so it is held to 1e-10 relative, as in
    tests/test_gpu_metad_run_f64.py; the table to BOUND times the summed heights."""
    dev = hip_device
    L, eager = _loop(dev, kind), _eager_loop(dev, kind)
    shape, d, T = L["shape"], 2, 3
    cols = list(L["columns"]) if L["columns"] else [0, 1]
    table, state = torch.zeros(shape, dtype=F64), torch.zeros(8, dtype=F64)
    adapt, astate, cov = torch.zeros(WALKERS, 1 + d + T, dtype=F64), torch.zeros(8, dtype=F64), torch.zeros(WALKERS, T, dtype=F64)
    log = torch.zeros(L["log_capacity"], d + T + 1, dtype=F64) if L["log_capacity"] else None
    shape_a, lower_a, spacing_a, periodic_a, _, _ = _capi.metad_grid_arrays(shape, L["lower"], L["spacing"], L["periodic"], L["sigma"], None)
    inv_dT = 1.0 / (KT * (BIASFACTOR - 1.0))
    mode = cc.DIFF if L["mode"] == "diff" else cc.GEOM

    def widths(emit, y=None, metric=None):
        assert cc.host_widths(shape, L["lower"], L["spacing"], L["periodic"], L["sigma"], L["columns"], mode, WINDOW, emit,
                              adapt if mode == cc.DIFF else None, astate, cov, y=y, metric=metric, sigma_min=L["sigma_min"], sigma_max=L["sigma_max"]) == 0

    for i, (y, v, dx, metric, after) in enumerate(eager):
        vg = v if v.dim() == 1 else v[:, 2]
        sel = y[:, cols].contiguous()
        hv = torch.tensor([_capi.lib().molann_selftest_grid_f64(sel[a].data_ptr(), d, table.data_ptr(), shape_a, lower_a, spacing_a, periodic_a, None)
                           for a in range(WALKERS)], dtype=F64)
        scale = float(table.abs().max())
        assert float((vg - hv).abs().max()) <= 1e-10 * scale, (i, vg, hv)
        widths(True, y=y if mode == cc.DIFF else None, metric=metric)
        assert cc.host_deposit_cov(table, L["lower"], L["spacing"], L["periodic"], L["columns"], y, hv, cov, HEIGHT, inv_dT, L["cutoff"], state, log) == 0
        if mode == cc.DIFF:
            for y_mid in L["between"][i]:
                widths(False, y=y_mid.cpu())
        got_state, got_adapt, got_astate, got_cov = after[1:5]
        assert got_state[[0, 1, 3, 4, 5, 6, 7]].tolist() == state[[0, 1, 3, 4, 5, 6, 7]].tolist(), i
        assert abs(float(got_state[2]) - float(state[2])) <= 1e-10 * float(state[2]), i
        assert got_astate.tolist() == astate.tolist(), i
        assert float((got_cov - cov).abs().max()) <= 1e-13 * float(cov.abs().max()), i
        if mode == cc.DIFF:
            assert float((got_adapt - adapt).abs().max()) <= 1e-13 * float(adapt.abs().max()), i
    final = eager[-1][4]
    heights_sum = float(state[2])
    err, tol = float((final[0] - table).abs().max()), cc.BOUND * heights_sum
    print("%s: 20 steps of 4 walkers, sum of heights %.6g (of %g): table error %.3g, bound %.3g; refused %d; adapt %s, cov %s"
          % (kind, heights_sum, STEPS * WALKERS * HEIGHT, err, tol, int(state[1]), "the host's bits" if pl.same_bits(final[2], adapt) else "close",
             "the host's bits" if pl.same_bits(final[4], cov) else "close"))
    assert err <= tol
    assert float(state[0]) + float(state[1]) == STEPS * WALKERS and float(state[0]) >= 0.9 * STEPS * WALKERS and float(state[3]) == STEPS
    assert heights_sum < 0.95 * STEPS * WALKERS * HEIGHT                          # walkers stand on the hills of earlier steps
    if mode == cc.DIFF:
        assert astate.tolist()[:3] == [3.0 * STEPS * WALKERS, float(STEPS), 0.0] and float(adapt[:, 0].min()) == 3.0 * STEPS
        # past the window the hills are correlated: the covariances differ from diag(sigma^2)
        assert float(cov[:, 1].abs().min()) > 0.0
    else:
        assert astate.tolist()[:3] == [0.0, float(STEPS), 0.0]
    if L["log_capacity"]:
        assert float(state[4]) == 64.0 and torch.equal(final[5][:, :d], log[:, :d])
        assert float((final[5][:, d:d + T] - log[:, d:d + T]).abs().max()) <= 1e-13 * float(log[:, d:d + T].abs().max())
        assert float((final[5][:, d + T] - log[:, d + T]).abs().max()) <= 1e-10 * HEIGHT
        # c(t): the last step is a multiple of the stride, so rct is the final table's
        rct = final[6]
        assert rct[1] == STEPS // 2 and rct[5] == STEPS and rct[6] == 0.0
        want, _ = rc.host_rct(final[0], kT=KT, inv_dT=inv_dT)
        assert abs(float(rct[0]) - float(want[0])) <= 1e-12 * (KT + abs(float(want[2])))


@pytest.mark.parametrize("kind", KINDS)
def test_one_captured_graph_replays_the_loop(kind, hip_device):
    """One stream, the step's launches in a chain (bias, widths, deposit and two observations for "diff"; bias, metric, widths, deposit
    for "geom"; with walls the c(t) pair too): the capture forks nowhere."""
    dev = hip_device
    L, eager = _loop(dev, kind), _eager_loop(dev, kind)
    run = _new_run(dev, kind)
    x_static = L["xs"][0].clone()
    n_out = L["y_all"].shape[1]
    walls_kind = kind.endswith("walls")
    into = (torch.empty(WALKERS, n_out, dtype=F64, device=dev), torch.empty((WALKERS, 3) if walls_kind else (WALKERS,), dtype=F64, device=dev),
            torch.empty_like(x_static))
    metric_into = (torch.empty(WALKERS, n_out, dtype=F64, device=dev), torch.empty(WALKERS, n_out, n_out, dtype=F64, device=dev))
    between = tuple(t.clone() for t in L["between"][0])
    buffers = [run.table, run.state, run.adapt, run.adapt_state, run.cov] + ([run.log] if run.log is not None else []) + \
        ([run.rct] if run.rct is not None else [])
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):               # a step outside the capture: plans, libraries and caches are made here
        _step(run, L, x_static, between, into=into, metric_into=metric_into)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    for b in buffers:
        b.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        _step(run, L, x_static, between, into=into, metric_into=metric_into)
    torch.cuda.synchronize()
    assert all(float(b.abs().max()) == 0.0 for b in buffers), "the capture ran the launches"
    for i, (x, mids, (y, v, dx, metric, after)) in enumerate(zip(L["xs"], L["between"], eager)):
        x_static.copy_(x)
        for dst, src in zip(between, mids):
            dst.copy_(src)
        graph.replay()
        got = tuple(u.cpu() for u in into)
        assert all(pl.same_bits(a, b) for a, b in zip(got, (y, v, dx))), "step %d: y, V or dx" % i
        assert all(pl.same_bits(a, b) for a, b in zip(_snapshot(run), after)), "step %d: table, state, adapt, cov, log or rct" % i


def test_cov_hills_hands_the_log_to_add_cov_hills_to_grid(hip_device):
    dev = hip_device
    for kind in ("diff walls", "geom walls"):
        L, eager = _loop(dev, kind), _eager_loop(dev, kind)
        run = _LOOP[kind + " run"]
        with pytest.raises(ValueError, match="cov_hills"):
            run.hills()
        record = run.cov_hills()
        assert record.centers.shape == (64, 2) and record.covariances.shape == (64, 3) and record.columns == (2, 0) and record.period is None
        rebuilt = mbias.add_cov_hills_to_grid(torch.zeros(L["shape"], dtype=F64, device=dev), L["lower"], L["spacing"], L["periodic"], record.centers,
                                              record.covariances, record.heights, cutoff=L["cutoff"])
        # the first 64 hills are steps 0..15: the table after step 15, rebuilt from the log with the run's cutoff
        assert oracle.cutoff_margin(L["shape"], L["lower"], L["spacing"], L["periodic"], None, record.centers.cpu().numpy(),
                                    record.covariances.cpu().numpy(), L["cutoff"]) >= 1e-9
        want = eager[15][4][0]
        err, tol = float((rebuilt.cpu() - want).abs().max()), cc.BOUND * float(record.heights.sum())
        print("%s: rebuilt from cov_hills: error %.3g, bound %.3g" % (kind, err, tol))
        assert err <= tol
        info = run.read_adaptive()
        assert info["emits"] == STEPS and info["skipped"] == 0 and info["last"].shape == (WALKERS, 3) and info["mean"].shape == (WALKERS, 2)
        with pytest.raises(ValueError, match="walkers"):
            run.deposit(torch.zeros(3, 4, dtype=F64, device=dev), torch.zeros(3, dtype=F64, device=dev))
    with pytest.raises(ValueError, match="observe"):
        _LOOP["geom walls run"].observe(torch.zeros(WALKERS, 4, dtype=F64, device=dev))
    with pytest.raises(TypeError, match="metric"):
        _LOOP["geom walls run"].deposit(torch.zeros(WALKERS, 4, dtype=F64, device=dev), torch.zeros(WALKERS, dtype=F64, device=dev))


def test_a_run_without_adaptive_is_the_run_of_before_bit_for_bit(hip_device):
    dev = hip_device
    case = mc.Case((17, 33), (True, False), 65, start="random")
    model = _loop(dev, "diff")["model"]
    args = (case.lower, case.spacing, KT, BIASFACTOR, HEIGHT, case.sigma)
    old = mbias.MetadRun(model, case.table.to(dev), *args, periodic=case.periodic, cutoff=CUTOFF, log_capacity=70)
    new = mbias.MetadRun(model, case.table.to(dev), *args, periodic=case.periodic, cutoff=CUTOFF, log_capacity=70, adaptive=None, window=None,
                         sigma_min=None, sigma_max=None, walkers=None)
    y, V = case.y.to(dev), case.V.to(dev)
    for run in (old, new):
        run.deposit(y, V), run.deposit(y, V)
    torch.cuda.synchronize()
    assert torch.equal(old.table, new.table) and torch.equal(old.state, new.state) and torch.equal(old.log, new.log)
    assert new.state[5:8].tolist() == [0.0, 0.0, 0.0] and new.log.shape == (70, 5) and new.adapt is None and new.cov is None
    # and both are the fixed-width kernel's: the direct call gives the same bits
    table, state = case.table.to(dev), torch.zeros(8, dtype=F64, device=dev)
    arrays = _capi.metad_grid_arrays(case.shape, case.lower, case.spacing, case.periodic, case.sigma, None)
    with torch.cuda.device(dev):
        for _ in range(2):
            _capi.metad_deposit_f64(table, arrays, y, V, HEIGHT, 1.0 / (KT * (BIASFACTOR - 1.0)), CUTOFF, state, None)
    assert torch.equal(table, new.table)
    assert isinstance(new.hills(), mbias.Hills)
    with pytest.raises(ValueError, match="hills"):
        new.cov_hills()
    with pytest.raises(ValueError):
        new.observe(y)
    with pytest.raises(ValueError, match="metric"):
        new.deposit(y, V, metric=torch.zeros(65, 2, 2, dtype=F64, device=dev))
