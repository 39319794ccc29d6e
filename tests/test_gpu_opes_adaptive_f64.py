"""The OPES step with adaptive widths and in the explore variant on the device: `molann_opes_step_modes_f64` (opes_step_modes_f64_kernel,
one block of 256 threads) against its host twin on the sequences of tests/opes_adaptive_cases.py - the device is fed the outputs and
the bias values the host run used - and `OpesRun(sigma0="adaptive")` / `OpesRun(explore=True)` end to end.

  averages  mean and M2 are only + - * / rint with nothing contracted: before the first deposit they are the host's bits
  the rest  counts, slots, run[0], run[6], run[7] equal; everything else within tests/opes_run_cases.py's bounds
  shapes    W d = 255, 256, 257 and 320 (walker, column) pairs around the block's 256 threads; 257 walkers (the second round of the
            walkers' sums); one walker; the first deposit at W = 64, d = 8, where every thread reads sigma0 rows other threads wrote
  in place  the [W, 5] outputs with columns (4, 1) and column 3 of the [W, 4] energies; adapt between guard bands"""

import math

import pytest
import torch

import opes_adaptive_cases as ac
import opes_adaptive_oracle as adaptive_oracle
import opes_deposit_cases as cases
import opes_run_cases as rc
import placement as pl
import test_gpu_value_and_vjp_f64 as vv
from molann_amd import _capi
from molann_amd import bias as mbias
from molann_amd.bias import Restraint

pytestmark = pytest.mark.gpu
F64 = torch.float64
NAN, INF = float("nan"), float("inf")
_HOST = {}


@pytest.fixture(scope="module", autouse=True)
def _leave_nothing_behind():
    """The module's shared runs, its model and its frames go when its last test has run, with the device idle: no later test of the
    session finds graphs, streams or device memory of this one."""
    yield
    import gc
    torch.cuda.synchronize()
    _HOST.clear()
    _LOOP.clear()
    gc.collect()
    torch.cuda.synchronize()


class _NoModel(object):
    def value_and_opes_table(self, *args, **kwargs):
        raise AssertionError("the step tests deposit only")

    value_and_bias = value_and_opes_table


def _host_sequence(d, walkers, explore, fixed_sigma, with_min, upto):
    """A host run of the sequence's first `upto` calls, once: (calls, snapshots, period, sigma_min)."""
    key = (d, walkers, explore, fixed_sigma, with_min, upto)
    if key not in _HOST:
        y, period = ac.walk(d, walkers, 5000 + 10 * d + walkers)
        # floors between the widths of early and late deposits: a third of the walk's step, which the rescaled widths pass on the way
        sigma_min = torch.full((d,), 0.08 / 3.0, dtype=F64) if with_min else None
        host = ac.HostModes(d, period, None, sigma_min, fixed_sigma, explore, walkers)
        calls, shots = ac.play(host, y, upto=upto)
        _HOST[key] = (calls, shots, period, sigma_min)
    return _HOST[key]


def _device_snapshot(t, run):
    torch.cuda.synchronize()
    return tuple(v.cpu() for v in (t.centers, t.sigma, t.heights, t.state, run.run)) + ((run.adapt.cpu(),) if run.adapt is not None else ())


def _device_sequence(dev, calls, d, walkers, period, sigma_min, explore, fixed_sigma):
    """The recorded calls through `OpesRun.observe` / `OpesRun.deposit`: a snapshot after every call."""
    t = mbias.OpesTable(ac.CAP, d, dev, period=period, cutoff=ac.CUTOFF, threshold=ac.THRESHOLD)
    run = mbias.OpesRun(_NoModel(), t, rc.KT, rc.BIASFACTOR, rc.BARRIER, "adaptive", sigma_min, fixed_sigma, adaptive_stride=ac.STRIDE,
                        walkers=walkers, explore=explore)
    shots = []
    for kind, y, V in calls:
        if kind == "observe":
            assert run.observe(y.to(dev)) is None
        else:
            assert run.deposit(y.to(dev), V.to(dev)) is None
        shots.append(_device_snapshot(t, run))
    return run, shots


def _compare_sequences(got, want, label):
    worst, bits = 0.0, 0
    for i, (g, w) in enumerate(zip(got, want)):
        worst = max(worst, ac.assert_same_modes_run(g, w, (label, i)))
        if i < 3:        # observe, observe, the skipped deposit: the averages are the host's bits, and nothing else has moved
            assert pl.same_bits(g[5][:, :2], w[5][:, :2]), (label, i)
            assert all(pl.same_bits(a, b) for a, b in zip(g[:5], w[:5])), (label, i)
        bits += 1 if all(pl.same_bits(a, b) for a, b in zip(g, w)) else 0
    print("%s: worst error / bound %.3g; %d of %d calls bit for bit" % (label, worst, bits, len(want)))
    return worst


# W d = 255, 256, 257, 320 pairs; 257 walkers; one walker; 12 calls each: through the skipped deposit, the first one and four more
SHAPES = [(255, 1), (32, 8), (257, 1), (40, 8), (1, 1), (1, 8), (3, 2)]


@pytest.mark.parametrize("explore", [False, True], ids=["metad", "explore"])
@pytest.mark.parametrize("walkers,d", SHAPES)
def test_the_shapes_around_the_block_match_the_host_twin(walkers, d, explore, hip_device):
    calls, shots, period, sigma_min = _host_sequence(d, walkers, explore, False, True, 12)
    run, got = _device_sequence(hip_device, calls, d, walkers, period, sigma_min, explore, False)
    _compare_sequences(got, shots, "W %d d %d%s" % (walkers, d, " explore" if explore else ""))
    state = run.read_adaptive()
    assert state["observations"] == 12 and state["started"] and state["sigma0"].shape == (walkers, d) and bool((state["sigma0"] > 0).all())
    assert pl.same_bits(state["mean"], shots[-1][5][:, 0])
    assert int(got[-1][3][0]) >= 1 and float(got[-1][4][0]) == 5.0 * walkers


@pytest.mark.parametrize("explore,fixed_sigma,with_min", [(False, False, True), (True, False, False), (False, True, False), (True, True, True)])
def test_the_whole_sequence_with_its_planted_walkers(explore, fixed_sigma, with_min, hip_device):
    d, walkers = 2, 3
    calls, shots, period, sigma_min = _host_sequence(d, walkers, explore, fixed_sigma, with_min, None)
    run, got = _device_sequence(hip_device, calls, d, walkers, period, sigma_min, explore, fixed_sigma)
    _compare_sequences(got, shots, "64 calls, explore %s fixed %s floor %s" % (explore, fixed_sigma, with_min))
    assert int(got[-1][3][3]) >= 2 and run.read_adaptive()["observations"] == len(ac.SEQUENCE)
    # the NaN walker kept its row on the device as well
    assert pl.same_bits(got[ac.PLANT_NAN][5][walkers - 1], got[ac.PLANT_NAN - 1][5][walkers - 1])
    assert not pl.same_bits(got[ac.PLANT_NAN][5][0, :2], got[ac.PLANT_NAN - 1][5][0, :2])


def test_the_first_deposit_reads_rows_other_threads_wrote(hip_device):
    """W = 64, d = 8: 512 pairs, two per thread, and 64 kernels whose widths every thread forms from all of them right after."""
    d, walkers = 8, 64
    calls, shots, period, sigma_min = _host_sequence(d, walkers, False, False, False, 4)
    run, got = _device_sequence(hip_device, calls, d, walkers, period, sigma_min, False, False)
    _compare_sequences(got, shots, "the first deposit, W 64 d 8")
    first = got[3]
    assert first[4].tolist()[6:] == [4.0, 1.0] and int(first[3][0]) >= 1 and int(first[3][0]) + int(first[3][2]) + int(first[3][3]) == walkers
    want_s0 = torch.sqrt(first[5][:, 1] / 4.0 / rc.BIASFACTOR)
    assert float(((first[5][:, 2] - want_s0).abs() / want_s0).max()) <= 1e-15
    again = _device_sequence(hip_device, calls, d, walkers, period, sigma_min, False, False)[1]
    assert all(pl.same_bits(a, b) for a, b in zip(got[3], again[3]))          # and the same bits on every run


def test_columns_and_energies_are_read_in_place(hip_device):
    """n_out = 5, columns (4, 1), the bias in column 3 of [W, 4] energies: the host twin on the same strided arrays, and the bits of the
    device run on the gathered copy."""
    dev, d, walkers, cols = hip_device, 2, 3, (4, 1)
    calls, shots, period, sigma_min = _host_sequence(d, walkers, False, False, True, 12)
    host = ac.HostModes(d, period, None, sigma_min, False, False, walkers, columns=cols)
    t = mbias.OpesTable(ac.CAP, d, dev, period=period, cutoff=ac.CUTOFF, threshold=ac.THRESHOLD)
    run = mbias.OpesRun(_NoModel(), t, rc.KT, rc.BIASFACTOR, rc.BARRIER, "adaptive", sigma_min, adaptive_stride=ac.STRIDE, walkers=walkers,
                        columns=cols)
    plain, _ = _device_sequence(dev, calls, d, walkers, period, sigma_min, False, False)
    for i, (kind, y, V) in enumerate(calls):
        wide = torch.full((walkers, 5), 1e300 if i % 2 else NAN, dtype=F64)     # the other columns are not looked at, whatever they hold
        wide[:, list(cols)] = y
        if kind == "observe":
            host.call(wide, observe=True)
            run.observe(wide.to(dev))
        else:
            energies = torch.full((walkers, 4), NAN, dtype=F64)
            energies[:, 3] = V
            host.call(wide, energies[:, 3])
            run.deposit(wide.to(dev), energies.to(dev))
        ac.assert_same_modes_run(_device_snapshot(t, run), host.snapshot(), ("columns", i))
        assert all(torch.equal(a, b) for a, b in zip(host.snapshot(), shots[i]))          # the host twin: the gathered run's bits
    assert all(pl.same_bits(a, b) for a, b in zip(_device_snapshot(t, run), _device_snapshot(plain.table, plain)))
    with pytest.raises(ValueError, match="3 walkers"):
        run.observe(torch.zeros(2, 5, dtype=F64, device=dev))
    with pytest.raises(ValueError, match="more than 4 columns"):
        run.observe(torch.zeros(3, 4, dtype=F64, device=dev))


@pytest.mark.parametrize("offset", [0, 1])
def test_adapt_and_every_buffer_between_guard_bands(offset, hip_device):
    """Two observes, the skipped deposit and the first deposit at W = 40, d = 8 (320 pairs), every buffer 8-byte aligned at most and
    between guard bands: nothing before a buffer, nothing after its last row, the inputs as they were, the host twin's values."""
    dev, d, walkers = hip_device, 8, 40
    calls, shots, period, sigma_min = _host_sequence(d, walkers, False, False, True, 12)
    arena = pl.Arena(dev, capacity=4 << 20)
    centers, sigma = arena.carve("centers", (ac.CAP, d), F64, offset), arena.carve("sigma", (ac.CAP, d), F64, offset)
    heights, state = arena.carve("heights", (ac.CAP,), F64, offset, row_dims=0), arena.carve("state", (4,), F64, offset, row_dims=0)
    run = arena.carve("run", (8,), F64, offset, row_dims=0)
    adapt = arena.carve("adapt", (walkers, 3, d), F64, offset)
    per = arena.carve("period", (d,), F64, offset, data=period, row_dims=0)
    smin = arena.carve("sigma_min", (d,), F64, offset, data=sigma_min, row_dims=0)
    for v in (centers, sigma, heights, state, run, adapt):
        v.zero_()
    for i, (kind, y, V) in enumerate(calls[:4]):
        yy = arena.carve("y%d" % i, y.shape, F64, offset, data=y)
        vv_ = None if V is None else arena.carve("V%d" % i, V.shape, F64, offset, data=V, row_dims=0)
        with torch.cuda.device(dev):
            _capi.opes_step_modes_f64(centers, sigma, heights, state, run, per, yy, None, vv_, None, smin, adapt, rc.BETA, rc.BIASFACTOR, ac.STRIDE,
                                      ac.THRESHOLD, ac.CUTOFF, observe=kind == "observe")
        torch.cuda.synchronize()
        assert arena.check() == [] and arena.inputs_changed() == [], (i, arena.check(), arena.inputs_changed())
        got = tuple(v.cpu() for v in (centers, sigma, heights, state, run, adapt))
        ac.assert_same_modes_run(got, shots[i], ("arena", offset, i))
    assert got[4].tolist()[6:] == [4.0, 1.0] and int(got[3][0]) >= 1


@pytest.mark.parametrize("n0,d,wide", [(60, 8, False), (520, 1, True), (520, 8, True)])
def test_without_adapt_and_explore_the_bits_are_the_columns_step(n0, d, wide, hip_device):
    """adapt NULL, explore off: the device's opes_step_columns_f64, bit for bit, on `opes_run_cases.step_scenario`."""
    dev = hip_device
    period, table, y, V, sigma0, sigma_min = rc.step_scenario(n0, d)
    columns = None
    if wide:
        order = [d + 2 - k for k in range(d)]
        full = torch.full((y.shape[0], d + 3), NAN, dtype=F64)
        full[:, order] = y
        y, columns = full, _capi._i32_array(order)
    results = []
    for modes in (False, True):
        t = mbias.OpesTable(600, d, dev, period=period, cutoff=5.0, threshold=1.0)
        t.centers[:n0], t.sigma[:n0], t.heights[:n0] = (v.to(dev) for v in table)
        t.state[:2] = torch.tensor([float(n0), cases.brute_force_S(*table, period, 5.0)], dtype=F64).to(dev)
        run = torch.zeros(8, dtype=F64)
        run[:3] = torch.tensor(rc.RUN0, dtype=F64)
        run, s0, smin = run.to(dev), sigma0.to(dev), sigma_min.to(dev)
        for i in range(0, y.shape[0], 4):
            yi, Vi = y[i:i + 4].contiguous().to(dev), V[i:i + 4].contiguous().to(dev)
            with torch.cuda.device(dev):
                if modes:
                    _capi.opes_step_modes_f64(t.centers, t.sigma, t.heights, t.state, run, t.period, yi, columns, Vi, s0, smin, None, rc.BETA, INF, 0,
                                              1.0, 5.0)
                else:
                    _capi.opes_step_columns_f64(t.centers, t.sigma, t.heights, t.state, run, t.period, yi, columns, Vi, s0, smin, rc.BETA, 1.0, 5.0)
        torch.cuda.synchronize()
        results.append(tuple(v.cpu() for v in (t.centers, t.sigma, t.heights, t.state, run)))
    assert all(pl.same_bits(a, b) for a, b in zip(*results))
    assert int(results[1][3][0]) > n0 and results[1][4].tolist()[6:] == [0.0, 0.0]


def test_a_run_with_given_widths_writes_what_it_wrote(hip_device):
    """`OpesRun` with numeric widths and explore off takes the launches it took: run[6] and run[7] stay 0 and `adapt` is None."""
    dev, n0, d = hip_device, 60, 8
    period, table, y, V, sigma0, sigma_min = rc.step_scenario(n0, d)
    t = mbias.OpesTable(600, d, dev, period=period, cutoff=5.0, threshold=1.0)
    run = mbias.OpesRun(_NoModel(), t, rc.KT, rc.BIASFACTOR, rc.BARRIER, sigma0, sigma_min)
    run.deposit(y[:4].to(dev), V[:4].to(dev))
    assert run.adapt is None and run.run.tolist()[6:] == [0.0, 0.0] and run.read_run()["counter"] == 4
    with pytest.raises(ValueError, match="observe"):
        run.observe(y[:4].to(dev))


# ---------------------------------------------------------------------------------------------- end to end
STEPS, WALKERS, LOOP_CAP = 12, 2, 64
_LOOP = {}


def _loop_model(dev):
    """The C3 workload behind a 2-output head, as tests/test_gpu_opes_run_f64.py has it."""
    if "model" not in _LOOP:
        w, model, _ = vv._workload("C3", dev, head=[32, 2], act=torch.nn.Tanh())
        xs = [w.make_frames(WALKERS, seed=700 + i).double().to(dev) for i in range(2 * STEPS)]
        _LOOP.update(model=model, w=w, xs=xs, period=torch.tensor([0.0, 50.0], dtype=F64))
    return _LOOP


def _new_run(dev, **kw):
    L = _loop_model(dev)
    table = mbias.OpesTable(LOOP_CAP, 2, dev, period=L["period"], cutoff=ac.CUTOFF, threshold=ac.THRESHOLD)
    return mbias.OpesRun(L["model"], table, rc.KT, rc.BIASFACTOR, rc.BARRIER, "adaptive", adaptive_stride=ac.STRIDE, walkers=WALKERS, **kw)


def test_an_adaptive_run_end_to_end_against_the_oracle(hip_device):
    dev = hip_device
    L = _loop_model(dev)
    run = _new_run(dev)
    ref = adaptive_oracle.ModesOracle(LOOP_CAP, 2, L["period"], ac.CUTOFF, ac.THRESHOLD, rc.KT, rc.BIASFACTOR, None, None, False, False, ac.STRIDE,
                                      WALKERS)
    floor = rc.SCALE * math.log(rc.EPSILON)
    for i in range(STEPS):
        y, v, dx = run.bias(L["xs"][i])
        run.deposit(y, v)
        y, v = y.cpu(), v.cpu()                 # the oracle is driven by the device's own outputs and bias
        assert ref.deposit(y, v) == (i >= ac.STRIDE - 1)
        if i < ac.STRIDE:                       # nothing is deposited before the first stride has passed: the bias is its floor
            assert bool((v == floor).all()) and float(dx.abs().max()) == 0.0
    got = _device_snapshot(run.table, run)
    o, n = ref.table, ref.table.n
    assert (int(got[3][0]), int(got[3][2]), int(got[3][3])) == o.counts() and n >= 2
    rows = rc.compare_tables(n, got[:3], (o.centers, o.sigma, o.heights))
    scalars = rc.compare_scalars(got[4], ref.run_values())
    adapt = ac.compare_adapt(got[5], torch.stack(ref.adapt_rows(), dim=1), ref.observations)
    brute = cases.brute_force_S(got[0][:n], got[1][:n], got[2][:n], L["period"], ac.CUTOFF)
    s_ratio = abs(float(got[3][1]) - brute) / (cases.S_BOUND * max(1.0, o.A))
    print("12 steps of 2 walkers: n %d merges %d refused %d; error / bound: rows %.3g scalars %.3g adapt %.3g S %.3g" % (o.counts() + (rows, scalars, adapt, s_ratio)))
    assert rows <= 1.0 and scalars <= 1.0 and adapt <= 1.0 and s_ratio <= 1.0
    assert got[4].tolist()[6:] == [float(STEPS), 1.0] and ref.counter == WALKERS * (STEPS - ac.STRIDE + 1) and ref.invalid == 0
    if o.margins:
        assert min(m[0] for m in o.margins) >= 1e-9 and min(m[1] for m in o.margins) >= 1e-9
    assert float(run.bias(L["xs"][0])[2].abs().max()) > 0.0        # and the bias now pushes


def test_one_captured_graph_replays_bias_observe_bias_deposit(hip_device):
    dev = hip_device
    L = _loop_model(dev)
    eager = _new_run(dev)
    after = []
    for i in range(STEPS):
        eager.observe(*eager.bias(L["xs"][2 * i])[:2])
        eager.deposit(*eager.bias(L["xs"][2 * i + 1])[:2])
        after.append(_device_snapshot(eager.table, eager))
    run = _new_run(dev)
    t = run.table
    xa, xb = L["xs"][0].clone(), L["xs"][1].clone()
    into = (torch.empty(WALKERS, 2, dtype=F64, device=dev), torch.empty(WALKERS, dtype=F64, device=dev), torch.empty_like(xa))

    def step():
        run.observe(*run.bias(xa, into=into)[:2])
        run.deposit(*run.bias(xb, into=into)[:2])

    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):               # a step outside the capture: plans, libraries and caches are made here
        step()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    for v in (t.centers, t.sigma, t.heights, t.state, run.run, run.adapt):
        v.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):               # one stream, four launches in a chain; adapt was allocated by the constructor
        step()
    torch.cuda.synchronize()
    assert float(t.state.abs().max()) == 0.0 and float(run.run.abs().max()) == 0.0 and float(run.adapt.abs().max()) == 0.0, "the capture ran the launches"
    for i in range(STEPS):
        xa.copy_(L["xs"][2 * i])
        xb.copy_(L["xs"][2 * i + 1])
        graph.replay()
        assert all(pl.same_bits(a, b) for a, b in zip(_device_snapshot(t, run), after[i])), "replay %d: table, state, run or adapt" % i
    assert after[-1][4].tolist()[6:] == [2.0 * STEPS, 1.0] and int(after[-1][3][0]) >= 2 and int(after[0][3][0]) == 0 and int(after[1][3][0]) >= 1
    torch.cuda.synchronize()
    del graph                                   # the replays are done: the graph goes before anything it points into


def test_explore_with_walls_through_value_and_bias(hip_device):
    """`OpesRun(explore=True, walls=...)`: the kernels weigh 1, and energies[:, 3] is scale log(P / norm + epsilon) with
    scale = kT (biasfactor - 1) and epsilon = exp(-barrier / scale)."""
    dev = hip_device
    L = _loop_model(dev)
    model, xs = L["model"], L["xs"]
    zero = torch.zeros(2, dtype=F64, device=dev)
    y_all = torch.cat([model.value_and_bias(x, restraint=Restraint(zero, zero))[0] for x in xs[:8]])
    mean, spread = y_all.mean(dim=0), y_all.std(dim=0) + 0.05
    walls = Restraint(mean.contiguous(), (3.0 / spread ** 2).contiguous(), flat=(0.5 * spread).contiguous())
    given = (0.35 * y_all.std(dim=0)).cpu()
    table = mbias.OpesTable(LOOP_CAP, 2, dev, period=L["period"], cutoff=ac.CUTOFF, threshold=ac.THRESHOLD)
    run = mbias.OpesRun(model, table, rc.KT, rc.BIASFACTOR, rc.BARRIER, given, fixed_sigma=True, walls=walls, explore=True)
    assert run.scale == ac.SCALE_X and run.epsilon == ac.EPSILON_X and run.adapt is None
    assert torch.equal(run.sigma0.cpu(), given * math.sqrt(rc.BIASFACTOR))
    for x in xs[:8]:
        y, energies, dx = run.bias(x)
        run.deposit(y, energies)
    n, S, merges, refused = table.read_state()
    assert n >= 2 and refused == 0 and n + merges == 8 * WALKERS
    centers, sigma, heights = table.centers[:n].cpu(), table.sigma[:n].cpu(), table.heights[:n].cpu()
    assert abs(float(heights.sum()) - 8 * WALKERS) <= 1e-12 * 8 * WALKERS                    # fixed widths: every kernel weighs exactly 1
    assert torch.equal(sigma[heights == 1.0], run.sigma0.cpu().expand(int((heights == 1.0).sum()), 2))
    for x in xs[8:12]:
        y, energies, dx = run.bias(x)
        P = mbias.opes_kernel_sum(y.cpu(), centers, heights, sigma, L["period"], ac.CUTOFF)
        want = ac.SCALE_X * torch.log(P / (S / n) + ac.EPSILON_X)
        got = energies[:, 3].cpu()
        assert float(((got - want).abs() / (rc.BOUND * torch.clamp(want.abs(), min=1.0))).max()) <= 1.0, (got, want)
        assert bool((energies[:, 1] == 0.0).all()) and bool(torch.isfinite(dx).all())
    assert run.read_run()["counter"] == 8 * WALKERS and run.run.tolist()[6:] == [0.0, 0.0]
