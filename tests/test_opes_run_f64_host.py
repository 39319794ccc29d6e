"""Whole OPES runs on the host (no GPU): `molann_selftest_opes_table_f64` gives every step's bias from the table's current state and
`molann_selftest_opes_step_f64` - the steps and the scalar functions of opes_step_f64_kernel compiled for the host, with the device's
order of every sum - turns it into the step's kernels and deposits them, against tests/opes_run_oracle.py, a sequential restatement in
plain Python and torch written from the formulas of include/molann_hip.h.  y follows the deposit cases' seeded random walk; both runs
are fed the same bias values (the host twin's), and the oracle's own bias is held against them at every step.

Bounds and where they come from: tests/opes_run_cases.py.  Decisions compare exactly: every search of every run is asserted to be at
least 1e-9 (relative) away from the threshold and from its runner-up, the value the deposit tests assert, and the widths that enter q
differ by a few 1e-16."""

import ctypes
import itertools
import math

import pytest
import torch

from molann_amd import _capi
from molann_amd import bias as mbias

import opes_deposit_cases as cases
import opes_run_cases as rc
import opes_run_oracle as run_oracle

F64 = torch.float64
INF, NAN = math.inf, math.nan
CAP, STEPS = 64, 200
# d, walkers, threshold, fixed sigma, sigma_min, cutoff
RUNS = list(itertools.product((1, 2, 8), (1, 4), (0.0, 1.0), (False, True), (False, True), (INF, 5.0)))
_DONE = {}


def _both_runs(d, width, threshold, fixed_sigma, with_min, cutoff):
    """The host twins' run and the oracle's of a seeded case, computed once and left unchanged: (host, ref, worst bias ratio)."""
    key = (d, width, threshold, fixed_sigma, with_min, cutoff)
    if key not in _DONE:
        period, batches = cases.seeded_run(d, width, threshold, cutoff, deposits=STEPS)
        sigma_min = rc.sigma_min_row(d, STEPS * width) if with_min else None
        host = rc.HostRun(CAP, d, period, cutoff, threshold, rc.sigma0_row(d), sigma_min, fixed_sigma)
        ref = run_oracle.RunOracle(CAP, d, period, cutoff, threshold, rc.KT, rc.BIASFACTOR, rc.BARRIER, rc.sigma0_row(d), sigma_min, fixed_sigma)
        worst_v = 0.0
        for i, (y, _, _) in enumerate(batches):       # every draw goes in: none is left out
            v, dy = host.bias(y)
            if i % 10 == 0 or i == STEPS - 1:
                # the oracle's bias on its own table with the host's norm: P is a sum of n <= 64 positive terms, each an exp at 1-2 ulp
                t = host.table
                want_v, want_dy = ref.bias(y, norm=float(t.state[1]) / t.n if t.n else None)
                worst_v = max(worst_v, float(((v - want_v).abs() / (rc.BOUND * torch.clamp(want_v.abs(), min=1.0))).max()))
                scale_dy = max(1.0, float(want_dy.abs().max()))
                worst_v = max(worst_v, float((dy - want_dy).abs().max()) / (1e-10 * scale_dy))
            host.step(y, v)
            ref.step(y, v)
        _DONE[key] = (host, ref, worst_v, period)
    return _DONE[key]


@pytest.mark.parametrize("d,width,threshold,fixed_sigma,with_min,cutoff", RUNS)
def test_seeded_runs_match_the_oracle(d, width, threshold, fixed_sigma, with_min, cutoff):
    host, ref, worst_v, period = _both_runs(d, width, threshold, fixed_sigma, with_min, cutoff)
    t, o = host.table, ref.table
    n = o.n
    assert t.counts() == o.counts(), (t.counts(), o.counts())
    rows = rc.compare_tables(n, (t.centers, t.sigma, t.heights), (o.centers, o.sigma, o.heights))
    scalars = rc.compare_scalars(host.run, ref.run_values())
    brute = cases.brute_force_S(t.centers[:n], t.sigma[:n], t.heights[:n], period, cutoff)
    s_ratio = abs(float(t.state[1]) - brute) / (cases.S_BOUND * max(1.0, o.A))
    print("n %d merges %d refused %d counter %d neff %.6g sigma_scale %.6g rct %.6g | error / bound: rows %.3g scalars %.3g S %.3g bias %.3g"
          % (t.counts() + (ref.counter, ref.neff, ref.sigma_scale, ref.rct, rows, scalars, s_ratio, worst_v)))
    assert rows <= 1.0 and scalars <= 1.0 and s_ratio <= 1.0 and worst_v <= 1.0
    assert abs(o.S - brute) <= cases.S_BOUND * max(1.0, o.A)          # the oracle's own running sum, by the same bound
    assert float(host.run[6]) == 0.0 and float(host.run[7]) == 0.0
    assert ref.counter == STEPS * width and ref.invalid == 0
    # every decision of every draw was clear of the threshold and of its runner-up
    if threshold > 0:
        worst_thr, worst_gap = min(m[0] for m in o.margins), min(m[1] for m in o.margins)
        print("smallest margins: threshold %.3g, runner-up %.3g" % (worst_thr, worst_gap))
        assert worst_thr >= 1e-9 and worst_gap >= 1e-9, (worst_thr, worst_gap)
    else:
        assert o.margins == [] and o.merges == 0 and n == CAP and o.refused == STEPS * width - CAP
    if fixed_sigma:
        assert float(host.run[4]) == 1.0 and ref.bound_steps == 0


def test_the_runs_met_every_path():
    """Over the seeded runs, on the oracle alone: a chain merge, a refusal at a full table, merges and appends, and steps in which
    sigma_min held a width up - in late steps, not in the first."""
    refs = [(run, _both_runs(*run)[1]) for run in RUNS]
    assert max(r.table.seen["chain_rounds_max"] for _, r in refs) >= 1
    for key in ("full", "merge", "append"):
        assert sum(r.table.seen[key] for _, r in refs) > 0, key
    bound = [r.bound_steps for run, r in refs if run[4] and not run[3]]
    print("steps in which sigma_min bound, per run:", bound)
    assert sum(1 for b in bound if b >= 1) >= len(bound) // 2 and max(bound) < STEPS, bound
    assert all(r.bound_steps == 0 for run, r in refs if not run[4])


# ---------------------------------------------------------------------------------------------- planted cases
def _warm_run(d=3, width=4, steps=12):
    period, batches = cases.seeded_run(d, width, 1.0, 5.0, deposits=steps + 1)
    host = rc.HostRun(32, d, period, 5.0, 1.0)
    for y, _, _ in batches[:steps]:
        host.step(y, host.bias(y)[0])
    return host, batches[steps][0]


@pytest.mark.parametrize("bad", ["nan_V", "inf_V", "overflow_V", "nan_y"])
def test_an_invalid_walker_is_refused_and_changes_nothing_else(bad):
    host, y = _warm_run()
    before = host.snapshot()
    v = host.bias(y)[0]
    y1, v1 = y[:1].clone(), v[:1].clone()
    if bad == "nan_y":
        y1[0, 1] = NAN
    else:
        v1[0] = {"nan_V": NAN, "inf_V": INF, "overflow_V": 1000.0}[bad]      # exp(1000) overflows
    host.step(y1, v1)
    after = host.snapshot()
    assert torch.equal(after[4][:3], before[4][:3])                        # counter, sum_w, sum_w2: the same bits
    assert torch.equal(after[4], before[4])                                 # and so what follows from them
    assert float(after[3][3]) == float(before[3][3]) + 1.0 and torch.equal(after[3][:3], before[3][:3])
    assert all(torch.equal(a, b) for a, b in zip(after[:3], before[:3]))    # no row changed, dead rows included
    # among valid walkers: the others land as the oracle says, the bad one is counted
    y4, v4 = y.clone(), v.clone()
    if bad == "nan_y":
        y4[2, 0] = NAN
    else:
        v4[2] = v1[0]
    ref = run_oracle.RunOracle(32, host.d, host.table.period, 5.0, 1.0, rc.KT, rc.BIASFACTOR, rc.BARRIER, host.sigma0)
    ref.table.fill(*(a[:host.table.n].clone() for a in before[:3]))
    ref.counter, ref.sum_w, ref.sum_w2 = int(before[4][0]), float(before[4][1]), float(before[4][2])
    ref.table.merges, ref.table.refused = int(after[3][2]), int(after[3][3])
    host.step(y4, v4)
    ref.step(y4, v4)
    assert ref.invalid == 1 and int(host.run[0]) == int(before[4][0]) + 3
    assert ref.table.refused >= int(after[3][3]) + 1
    assert host.table.counts() == ref.table.counts()
    n = ref.table.n
    assert rc.compare_tables(n, (host.table.centers, host.table.sigma, host.table.heights), (ref.table.centers, ref.table.sigma, ref.table.heights)) <= 1.0
    assert rc.compare_scalars(host.run, ref.run_values()) <= 1.0
    assert bool(torch.isfinite(host.run).all()) and bool(torch.isfinite(host.table.state).all())


def test_a_state_that_is_not_a_count_is_held_to_the_table():
    """`molann_selftest_opes_table_f64` reads state[0] = NaN or -1 as no kernel and capacity + 5 as capacity."""
    host, y = _warm_run()
    t, L = host.table, _capi.lib()
    t.heights[t.n:] = 0.25
    t.centers[t.n:] = 0.1
    t.sigma[t.n:] = 0.4            # the dead rows hold valid kernels, so that reading all of them gives finite values
    S = float(t.state[1])

    def plain(n, norm):
        dy = torch.empty(host.d, dtype=F64)
        v = L.molann_selftest_opes_f64(y[0].data_ptr(), host.d, t.centers.data_ptr(), t.heights.data_ptr(), n, t.sigma.data_ptr(), host.d,
                                       t.period.data_ptr(), rc.SCALE, norm, rc.EPSILON, t.cutoff, dy.data_ptr())
        return v, dy

    for n0, n_read in ((NAN, 0), (-1.0, 0), (0.0, 0), (float(t.cap + 5), t.cap), (float(t.n), t.n)):
        t.state[0] = n0
        v, dy = host.bias(y[:1])
        want_v, want_dy = plain(n_read, S / n_read if n_read else 1.0)
        assert float(v[0]) == want_v and torch.equal(dy[0], want_dy), n0
        if n_read == 0:
            assert float(v[0]) == rc.SCALE * math.log(rc.EPSILON) and float(dy.abs().max()) == 0.0


def test_a_broken_sum_is_not_guarded():
    host, y = _warm_run()
    for S in (NAN, 0.0, -1.0, INF):
        host.table.state[1] = S
        assert not bool(torch.isfinite(host.bias(y)[0]).any()) or S == INF      # S = +inf: u = epsilon, a finite bias; documented as the caller's
    host.table.state[0] = 0.0
    assert bool(torch.isfinite(host.bias(y)[0]).all())                          # no kernel: norm is not formed


def test_no_walkers_changes_nothing():
    host, _ = _warm_run()
    before = host.snapshot()
    L, t = _capi.lib(), host.table
    assert L.molann_selftest_opes_step_f64(t.centers.data_ptr(), t.sigma.data_ptr(), t.heights.data_ptr(), t.cap, host.d, None, t.state.data_ptr(),
                                           host.run.data_ptr(), None, None, 0, host.sigma0.data_ptr(), None, rc.BETA, 1.0, INF, 0) == 0
    assert L.molann_opes_step_f64(None, None, None, 4, 2, None, None, None, None, None, 0, None, None, 1.0, 1.0, INF, 0, None) == 0    # nothing launched
    assert all(torch.equal(a, b) for a, b in zip(host.snapshot(), before))


def test_the_first_step_of_a_run():
    """An empty table: the bias is scale log(epsilon), every walker's weight exp(beta V) = epsilon^(scale beta)."""
    host = rc.HostRun(8, 2, None, INF, 0.0, fixed_sigma=True)
    y = torch.tensor([[0.0, 0.0], [3.0, 3.0]], dtype=F64)
    v, dy = host.bias(y)
    assert bool((v == rc.SCALE * math.log(rc.EPSILON)).all()) and float(dy.abs().max()) == 0.0
    host.step(y, v)
    w = math.exp(rc.BETA * float(v[0]))
    assert host.table.counts() == (2, 0, 0) and host.run.tolist()[:3] == [2.0, w + w, w * w + w * w]
    assert torch.equal(host.table.heights[:2], torch.tensor([w, w], dtype=F64)) and torch.equal(host.table.sigma[:2], rc.sigma0_row(2).expand(2, 2))
    assert abs(float(host.run[5]) - math.log(w) / rc.BETA) <= 1e-12 * 20 and float(host.run[4]) == 1.0


@pytest.mark.parametrize("width", [1, 4])
@pytest.mark.parametrize("d", [1, 8])
@pytest.mark.parametrize("n0", [60, 520])
def test_the_step_scenarios_of_the_device_test(n0, d, width):
    """tests/test_gpu_opes_run_f64.py runs these on the device against the host twin; here the host twin against the oracle, the paths
    they are built to meet and their margins."""
    host, (period, table, y, V, sigma0, sigma_min) = rc.host_scenario_run(n0, d, width)
    ref = run_oracle.RunOracle(600, d, period, 5.0, 1.0, rc.KT, rc.BIASFACTOR, rc.BARRIER, sigma0, sigma_min, False)
    ref.table.fill(*table)
    ref.counter, ref.sum_w, ref.sum_w2 = int(rc.RUN0[0]), rc.RUN0[1], rc.RUN0[2]
    for i in range(0, y.shape[0], width):
        ref.step(y[i:i + width], V[i:i + width])
    o = ref.table
    assert host.table.counts() == o.counts(), (host.table.counts(), o.counts())
    cases.assert_scenario_paths(o, n0)
    assert ref.bound_steps == 16 // width and 0.4 < ref.sigma_scale < 0.8
    t = host.table
    assert rc.compare_tables(o.n, (t.centers, t.sigma, t.heights), (o.centers, o.sigma, o.heights)) <= 1.0
    assert rc.compare_scalars(host.run, ref.run_values()) <= 1.0
    brute = cases.brute_force_S(t.centers[:o.n], t.sigma[:o.n], t.heights[:o.n], period, 5.0)
    assert abs(float(t.state[1]) - brute) <= cases.S_BOUND * max(1.0, o.A)


# ---------------------------------------------------------------------------------------------- the C entries
def _step_refusals(call):
    """`call(**overrides)` -> code, for the device entry or its host twin: every refusal and their order (molann_opes_deposit_f64's)."""
    ok = torch.zeros(16, dtype=F64)
    p, odd = ok.data_ptr(), ok.data_ptr() + 4
    base = dict(centers=p, sigma=p, heights=p, capacity=4, d=2, period=None, state=p, run=p, y=p, V=p, n_walkers=1, sigma0=p, sigma_min=None,
                beta=1.0, threshold=1.0, cutoff=5.0, fixed_sigma=0)
    for name in ("centers", "sigma", "heights", "state", "run", "y", "V", "sigma0"):
        assert call(**dict(base, **{name: None})) == _capi.E_NULL, name
        assert call(**dict(base, **{name: odd})) == _capi.E_ALIGNMENT, name
        assert call(**dict(base, **{name: None, "d": 0, "period": odd})) == _capi.E_NULL, name      # NULL comes first
    for name in ("period", "sigma_min"):
        assert call(**dict(base, **{name: odd})) == _capi.E_ALIGNMENT
        assert call(**dict(base, **{name: odd, "d": 9})) == _capi.E_ALIGNMENT                        # alignment before d
    for d in (0, -1, 9):
        assert call(**dict(base, d=d)) == _capi.E_DESC
    assert call(**dict(base, capacity=0)) == _capi.E_DESC
    assert call(**dict(base, n_walkers=-1)) == _capi.E_DESC
    assert call(**dict(base, n_walkers=-1, centers=None)) == _capi.E_DESC       # a NULL pointer matters only where n_walkers > 0
    for beta in (0.0, -1.0, NAN, INF):
        assert call(**dict(base, beta=beta)) == _capi.E_DESC
    for thr in (-0.5, NAN, INF):
        assert call(**dict(base, threshold=thr)) == _capi.E_DESC
    for cut in (0.0, -1.0, NAN):
        assert call(**dict(base, cutoff=cut)) == _capi.E_DESC
    # refused before anything is looked at where n_walkers == 0, too
    assert call(**dict(base, n_walkers=0, d=9)) == _capi.E_DESC
    assert call(**dict(base, n_walkers=0, centers=None, y=None)) == 0


def test_every_refusal_of_the_step_entry_and_of_its_host_twin():
    L = _capi.lib()
    order = ("centers", "sigma", "heights", "capacity", "d", "period", "state", "run", "y", "V", "n_walkers", "sigma0", "sigma_min", "beta", "threshold",
             "cutoff", "fixed_sigma")
    _step_refusals(lambda **kw: L.molann_opes_step_f64(*[kw[k] for k in order], None))      # refused before any launch: no GPU needed
    _step_refusals(lambda **kw: L.molann_selftest_opes_step_f64(*[kw[k] for k in order]))


def test_the_bias_entry_without_a_plan_and_its_host_twin():
    """What of molann_value_and_opes_table_f64 can be seen without a device: a NULL plan comes first (the rest of its order is the GPU
    file's); the host twin answers a missing pointer, a bad d or a bad capacity with NaN."""
    L = _capi.lib()
    assert L.molann_plan_supports_value_and_opes_table_f64(None) == _capi.E_NULL
    ok = torch.ones(16, dtype=F64)
    p = ok.data_ptr()
    assert L.molann_value_and_opes_table_f64(None, p, 3, None, None, p, p, p, 4, p, None, 1.0, 1e-3, 5.0, p, p, p, None) == _capi.E_NULL
    assert L.molann_value_and_opes_table_f64(None, None, 0, None, None, None, None, None, 0, None, None, NAN, -1.0, 0.0, None, None, None, None) == _capi.E_NULL
    good = [p, 2, p, p, p, 4, p, None, 1.0, 1e-3, 5.0, None]
    assert math.isfinite(L.molann_selftest_opes_table_f64(*good))
    for i, bad in ((0, None), (1, 0), (1, 9), (2, None), (3, None), (4, None), (5, 0), (6, None)):
        args = list(good)
        args[i] = bad
        assert math.isnan(L.molann_selftest_opes_table_f64(*args)), i


def test_the_symbols_are_declared_exported_and_bound():
    L = _capi.lib()
    for name, res in (("molann_value_and_opes_table_f64", ctypes.c_int), ("molann_plan_supports_value_and_opes_table_f64", ctypes.c_int),
                      ("molann_opes_step_f64", ctypes.c_int), ("molann_selftest_opes_step_f64", ctypes.c_int),
                      ("molann_selftest_opes_table_f64", ctypes.c_double)):
        assert name in _capi.declared_symbols()
        fn = getattr(L, name)
        assert fn.argtypes is not None and fn.restype is res
    assert L.molann_abi_version() == 1
    assert callable(_capi.opes_step_f64) and callable(_capi.Plan.value_and_opes_table_f64)
    assert "OpesRun" in mbias.__all__


def test_the_operators_are_registered():
    from molann_amd import script
    script.load_ops()
    for name in ("value_and_opes_table", "value_and_opes_table_h", "opes_step"):
        assert hasattr(torch.ops.molann, name)
    schema = str(torch.ops.molann.opes_step.default._schema)
    assert "Tensor(a!) centers" in schema and "Tensor(e!) run" in schema and schema.endswith("-> ()")


class _Model(object):
    def value_and_opes_table(self, *args, **kwargs):
        raise AssertionError("not called by the constructor")


def test_opes_run_argument_errors():
    """Every refusal of the constructor comes before any device call: a table cannot be made without a device, so a stand-in that holds
    what the constructor looks at takes its place."""
    table = mbias.OpesTable.__new__(mbias.OpesTable)
    table.d, table.centers = 2, torch.zeros(4, 2, dtype=F64)
    R, good = mbias.OpesRun, dict(kT=1.0, biasfactor=10.0, barrier=20.0, sigma0=[0.3, 0.3])
    run = R(_Model(), table, **good)
    assert run.scale == 0.9 and run.epsilon == math.exp(-20.0 / 0.9) and run.beta == 1.0 and run.run.shape == (8,) and not bool(run.run.any())
    assert R(_Model(), table, 2.5, INF, 20.0, [0.3, 0.3]).scale == 2.5
    with pytest.raises(TypeError, match="value_and_opes_table"):
        R(object(), table, **good)
    with pytest.raises(TypeError, match="OpesTable"):
        R(_Model(), object(), **good)
    for name in ("kT", "biasfactor", "barrier"):
        with pytest.raises(TypeError, match=name):
            R(_Model(), table, **dict(good, **{name: "1"}))
        with pytest.raises(TypeError, match=name):
            R(_Model(), table, **dict(good, **{name: True}))
        for bad in (0.0, -1.0, NAN):
            with pytest.raises(ValueError, match=name):
                R(_Model(), table, **dict(good, **{name: bad}))
    for bad in (1.0, 0.5):
        with pytest.raises(ValueError, match="biasfactor"):
            R(_Model(), table, **dict(good, biasfactor=bad))
    with pytest.raises(ValueError, match="kT"):
        R(_Model(), table, **dict(good, kT=INF))
    with pytest.raises(ValueError, match="underflows"):
        R(_Model(), table, **dict(good, barrier=1e4))
    for name in ("sigma0", "sigma_min"):
        for bad in ([0.3], [0.3, 0.0], [0.3, -0.1], [0.3, NAN], [0.3, INF], torch.tensor([[0.3, 0.3]])):
            with pytest.raises(ValueError, match=name):
                R(_Model(), table, **dict(good, **{name: bad}))
        with pytest.raises(TypeError, match=name):
            R(_Model(), table, **dict(good, **{name: "wide"}))
    with pytest.raises(TypeError, match="sigma0"):
        R(_Model(), table, **dict(good, sigma0=None))


def test_the_methods_exist_and_say_what_is_out_of_scope():
    from molann_amd.ann import MolANN, PreprocessingANN
    for cls in (MolANN, PreprocessingANN):
        assert callable(cls.value_and_opes_table)
    doc = MolANN.value_and_opes_table.__doc__
    assert "molann_value_and_opes_table_f64" in doc and "Out of scope" in doc and "GraphedForces" in doc
    assert "explore" in mbias.OpesRun.__doc__


def test_cpu_tensor_and_a_wrong_table_are_refused_before_any_device_call():
    from molann_amd import ann, workloads as wl
    w = wl.get_workload("C3")
    model = wl.build_model(w, torch.device("cpu"), 0).double().requires_grad_(False)
    x = w.make_frames(3, seed=1).double()
    table = mbias.OpesTable.__new__(mbias.OpesTable)
    table.d, table.centers, table.cutoff = w.out_dim(), torch.zeros(4, w.out_dim(), dtype=F64), None
    with pytest.raises(NotImplementedError, match=r"value_and_opes_table needs a model served by one fused plan.*OpesTable\.read_state"):
        model.value_and_opes_table(x, table, 0.9, 1e-9)
    check = lambda *a: ann._check_opes_table_args("name", x, w.out_dim(), *a, None)       # noqa: E731
    with pytest.raises(TypeError, match="OpesTable"):
        check(object(), 0.9, 1e-9)
    for scale, eps, exc in ((NAN, 1e-9, ValueError), (INF, 1e-9, ValueError), (0.9, 0.0, ValueError), (0.9, NAN, ValueError), ("1", 1e-9, TypeError),
                            (0.9, True, TypeError)):
        with pytest.raises(exc):
            check(table, scale, eps)
    table.d = w.out_dim() - 1
    with pytest.raises(ValueError, match="columns"):
        check(table, 0.9, 1e-9)
    with pytest.raises(NotImplementedError, match="at most 8 outputs"):
        ann._check_opes_table_args("name", x, 9, table, 0.9, 1e-9, None)
