"""The OPES step with adaptive widths and in the explore variant on the host (no GPU): `molann_selftest_opes_step_modes_f64` - the steps
and the scalar functions of opes_step_modes_f64_kernel compiled for the host - against tests/opes_adaptive_oracle.py, a sequential
restatement in plain Python written from the formulas of include/molann_hip.h.  Both are fed the same outputs and the same bias values
(the host twin's); the sequence, the planted values and the bounds: tests/opes_adaptive_cases.py.

Decisions compare exactly: every search of every run is asserted to be at least 1e-9 (relative) away from the threshold and from its
runner-up, and every comparison of a width with its floor at least 1e-9 away from equality - on the oracle alone."""

import ctypes
import itertools
import math

import pytest
import torch

from molann_amd import _capi
from molann_amd import bias as mbias

import opes_adaptive_cases as ac
import opes_adaptive_oracle as adaptive_oracle
import opes_deposit_cases as cases
import opes_run_cases as rc

F64 = torch.float64
INF, NAN = math.inf, math.nan
# d, walkers, explore, fixed sigma, sigma_min
RUNS = list(itertools.product((1, 2, 8), (1, 3), (False, True), (False, True), (False, True)))
_DONE = {}


def _seed(d, walkers, explore, fixed_sigma, with_min):
    return 4000 + 100 * d + 10 * walkers + 4 * explore + 2 * fixed_sigma + with_min


def _oracle(d, walkers, period, explore, fixed_sigma, sigma_min, sigma0=None):
    return adaptive_oracle.ModesOracle(ac.CAP, d, period, ac.CUTOFF, ac.THRESHOLD, rc.KT, rc.BIASFACTOR, sigma0, sigma_min, fixed_sigma, explore,
                                       None if sigma0 is not None else ac.STRIDE, None if sigma0 is not None else walkers)


def _floors(d, walkers, period, explore, fixed_sigma, y):
    """Floors that bind in some steps and not in others: per column half way between the two middle widths of a run of the oracle
    without floors, on the bias of a host run without floors (a floor that IS one of those widths would meet it again, exactly, in the
    steps before it first binds)."""
    host = ac.HostModes(d, period, None, None, fixed_sigma, explore, walkers)
    ref = _oracle(d, walkers, period, explore, fixed_sigma, None)
    widths = []

    class Collect(object):
        def observe(self, yi):
            ref.observe(yi)

        def deposit(self, yi, V):
            if ref.deposit(yi, V):
                widths.append(ref.last_sigma.clone())

    ac.play(host, y, [Collect()])
    ordered = torch.cat(widths).sort(dim=0).values
    m = ordered.shape[0] // 2
    return (0.5 * (ordered[m - 1] + ordered[m])).contiguous()


def _both_runs(d, walkers, explore, fixed_sigma, with_min):
    """The host twin's adaptive run and the oracle's, computed once and left unchanged."""
    key = (d, walkers, explore, fixed_sigma, with_min)
    if key not in _DONE:
        y, period = ac.walk(d, walkers, _seed(*key))
        sigma_min = _floors(d, walkers, period, explore, fixed_sigma, y) if with_min else None
        host = ac.HostModes(d, period, None, sigma_min, fixed_sigma, explore, walkers)
        ref = _oracle(d, walkers, period, explore, fixed_sigma, sigma_min)
        calls, shots = ac.play(host, y, [ref])
        _DONE[key] = (host, ref, calls, shots, period, y)
    return _DONE[key]


def _assert_against_oracle(host, ref, period, label):
    t, o = host.table, ref.table
    n = o.n
    assert t.counts() == o.counts(), (label, t.counts(), o.counts())
    rows = rc.compare_tables(n, (t.centers, t.sigma, t.heights), (o.centers, o.sigma, o.heights))
    scalars = rc.compare_scalars(host.run, ref.run_values())
    brute = cases.brute_force_S(t.centers[:n], t.sigma[:n], t.heights[:n], period, ac.CUTOFF)
    s_ratio = abs(float(t.state[1]) - brute) / (cases.S_BOUND * max(1.0, o.A))
    assert host.run.tolist()[6:] == [float(ref.observations), float(ref.started)], (label, host.run.tolist())
    adapt = 0.0
    if host.adapt is not None:
        adapt = ac.compare_adapt(host.adapt, torch.stack(ref.adapt_rows(), dim=1), ref.observations)
    print("%s: n %d merges %d refused %d counter %d neff %.6g sigma_scale %.6g | error / bound: rows %.3g scalars %.3g S %.3g adapt %.3g"
          % ((label,) + t.counts() + (ref.counter, ref.neff, ref.sigma_scale, rows, scalars, s_ratio, adapt)))
    assert rows <= 1.0 and scalars <= 1.0 and s_ratio <= 1.0 and adapt <= 1.0, label
    return o


def _assert_margins(ref, label):
    o = ref.table
    worst_thr, worst_gap = min(m[0] for m in o.margins), min(m[1] for m in o.margins)
    floor = min([m for _, m in ref.floor_margins], default=INF)
    print("%s: smallest margins: threshold %.3g, runner-up %.3g, floor %.3g" % (label, worst_thr, worst_gap, floor))
    assert worst_thr >= 1e-9 and worst_gap >= 1e-9 and floor >= 1e-9, (label, worst_thr, worst_gap, floor)


@pytest.mark.parametrize("d,walkers,explore,fixed_sigma,with_min", RUNS)
def test_adaptive_runs_match_the_oracle(d, walkers, explore, fixed_sigma, with_min):
    host, ref, calls, shots, period, y = _both_runs(d, walkers, explore, fixed_sigma, with_min)
    _assert_against_oracle(host, ref, period, "adaptive")
    _assert_margins(ref, "adaptive")
    deposits = ac.SEQUENCE.count("deposit")
    assert ref.observations == len(ac.SEQUENCE) and ref.started == 1 and ref.skipped == 1
    assert ref.invalid == 2 and ref.counter == (deposits - 1) * walkers - 2
    assert ref.table.refused >= 2
    # the planted walker's row did not move at the NaN call, and did at the call with the infinite bias
    before, after = shots[ac.PLANT_NAN - 1][5], shots[ac.PLANT_NAN][5]
    assert torch.equal(before[walkers - 1], after[walkers - 1])
    assert walkers == 1 or not torch.equal(before[0, :2], after[0, :2])
    before, after = shots[ac.PLANT_INF - 1][5], shots[ac.PLANT_INF][5]
    assert not torch.equal(before[walkers - 1, :2], after[walkers - 1, :2])
    if with_min:
        raised = sum(1 for r, _ in ref.floor_margins if r)
        assert 0 < raised < len(ref.floor_margins), (raised, len(ref.floor_margins))
    else:
        assert ref.floor_margins == []


def test_the_runs_met_every_path():
    """Over the runs, on the oracle alone: merges and appends, a refusal, and a windowed mean on the other side of the seam from its
    walker's output - the wrap of phase 1 changed a difference."""
    refs = [(run, _both_runs(*run)) for run in RUNS]
    for key in ("merge", "append"):
        assert sum(r[1].table.seen[key] for _, r in refs) > 0, key
    for run, (host, ref, calls, shots, period, y) in refs:
        mean = shots[-1][5][:, 0, 0]
        crossed = False
        for i in range(len(ac.SEQUENCE)):
            raw = y[i, :, 0] - shots[i][5][:, 0, 0]
            crossed = crossed or bool((raw.abs() > 1.0).any())
        assert crossed, run
        assert bool(torch.isfinite(mean).all())


@pytest.mark.parametrize("d,walkers,explore,fixed_sigma,with_min", RUNS)
def test_a_skipped_deposit_and_an_observe_leave_the_table_its_bits(d, walkers, explore, fixed_sigma, with_min):
    host, ref, calls, shots, period, y = _both_runs(d, walkers, explore, fixed_sigma, with_min)
    zero = ac.HostModes(d, period, None, None, fixed_sigma, explore, walkers).snapshot()
    for i in (0, 1, 2):          # observe, observe, the skipped deposit: nothing but run[6] and adapt
        assert all(torch.equal(a, b) for a, b in zip(shots[i][:4], zero[:4])), i
        assert torch.equal(shots[i][4][:6], zero[4][:6]) and shots[i][4].tolist()[6:] == [i + 1.0, 0.0]
        assert not torch.equal(shots[i][5][:, 0], zero[5][:, 0]) and not bool(shots[i][5][:, 2].any())
    assert float(shots[3][3][0]) >= 1.0 and shots[3][4].tolist()[6:] == [4.0, 1.0] and bool((shots[3][5][:, 2] > 0).all())
    for i in range(4, len(ac.SEQUENCE), 2):      # the observes between deposits
        assert all(torch.equal(a, b) for a, b in zip(shots[i][:4], shots[i - 1][:4])), i
        assert torch.equal(shots[i][4][:6], shots[i - 1][4][:6]) and shots[i][4].tolist()[6:] == [i + 1.0, 1.0]
        assert torch.equal(shots[i][5][:, 2], shots[i - 1][5][:, 2])        # sigma0 stays as the first deposit fixed it
    # the first deposit: M2 biasfactor, sigma0 from it
    M2_before, M2_after, s0 = shots[2][5][:, 1], shots[3][5][:, 1], shots[3][5][:, 2]
    assert bool((M2_after > M2_before * (rc.BIASFACTOR - 1.0)).all())
    factor = 1.0 if explore else rc.BIASFACTOR
    want = torch.sqrt(M2_after / 4.0 / factor)
    if with_min:
        want = torch.maximum(want, host.sigma_min)
    assert float(((s0 - want).abs() / want).max()) <= 1e-12


@pytest.mark.parametrize("fixed_sigma,with_min", [(False, False), (False, True), (True, False)])
@pytest.mark.parametrize("walkers", [1, 3])
@pytest.mark.parametrize("d", [1, 2, 8])
def test_explore_with_given_widths_matches_the_oracle(d, walkers, fixed_sigma, with_min):
    """The explore variant with a numeric sigma0: the oracle takes the unbiased widths, the entry the target's, sqrt(biasfactor) times
    as wide - what `OpesRun` stores."""
    y, period = ac.walk(d, walkers, 4900 + 10 * d + walkers)
    given = torch.tensor([ac.SIGMA0_GIVEN + 0.01 * k for k in range(d)], dtype=F64)
    target = given * math.sqrt(rc.BIASFACTOR)
    # the widths fall with (walkers x deposits)^(-1 / (d + 4)): a floor at the width of about a third of the run binds late and not
    # early (3.1: the counter, an integer, never meets that size, so no width meets its floor exactly)
    size = walkers * ac.SEQUENCE.count("deposit") / 3.1
    sigma_min = (target * (size * (d + 2.0) / 4.0) ** (-1.0 / (d + 4.0))).contiguous() if with_min else None
    host = ac.HostModes(d, period, target, sigma_min, fixed_sigma, True)
    ref = _oracle(d, walkers, period, True, fixed_sigma, sigma_min, sigma0=given)

    last = walkers - 1
    for i, kind in enumerate(ac.SEQUENCE):
        if kind == "observe":
            continue
        yi = y[i].clone()
        V = host.bias(yi)
        if i == ac.PLANT_NAN:
            yi[last, d - 1] = NAN
        if i == ac.PLANT_INF:
            V[last] = INF
        host.call(yi, V)
        ref.deposit(yi, V)
    _assert_against_oracle(host, ref, period, "explore, given widths")
    _assert_margins(ref, "explore, given widths")
    assert host.run.tolist()[6:] == [0.0, 0.0] and ref.invalid == 2
    if with_min:
        raised = sum(1 for r, _ in ref.floor_margins if r)
        assert 0 < raised < len(ref.floor_margins), (raised, len(ref.floor_margins))
    # every kernel weighs 1 times its widths' ratio, which is 1 with fixed widths: the heights add up to the number of kernels taken
    if fixed_sigma:
        n = host.table.n
        accepted = ref.counter - (ref.table.refused - ref.invalid)
        assert abs(float(host.table.heights[:n].sum()) - accepted) <= 1e-9 * accepted


# ---------------------------------------------------------------------------------------------- against the columns step
def _columns_twin(table, state, run, period, y, columns, V, sigma0, sigma_min, n_out):
    t = table
    return _capi.lib().molann_selftest_opes_step_columns_f64(
        t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[0].shape[0], t[0].shape[1], None if period is None else period.data_ptr(),
        state.data_ptr(), run.data_ptr(), y.data_ptr(), n_out, columns, V.data_ptr(), 1, y.shape[0], sigma0.data_ptr(), sigma_min.data_ptr(),
        rc.BETA, 1.0, 5.0, 0)


def _modes_twin(table, state, run, period, y, columns, V, sigma0, sigma_min, n_out, biasfactor=NAN):
    t = table
    return _capi.lib().molann_selftest_opes_step_modes_f64(
        t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), t[0].shape[0], t[0].shape[1], None if period is None else period.data_ptr(),
        state.data_ptr(), run.data_ptr(), y.data_ptr(), n_out, columns, V.data_ptr(), 1, y.shape[0], sigma0.data_ptr(), sigma_min.data_ptr(), None,
        rc.BETA, biasfactor, 0, 1.0, 5.0, 0)


def scenario_state(n0, d, capacity=600):
    """`opes_run_cases.step_scenario` as the arrays of a step: ((centers, sigma, heights), state, run, the scenario)."""
    sc = rc.step_scenario(n0, d)
    period, table, y, V, sigma0, sigma_min = sc
    t = cases.HostTable(capacity, d, period, 5.0, 1.0).fill(*table, cases.brute_force_S(*table, period, 5.0))
    run = torch.zeros(8, dtype=F64)
    run[:3] = torch.tensor(rc.RUN0, dtype=F64)
    return (t.centers, t.sigma, t.heights), t.state, run, sc


@pytest.mark.parametrize("wide", [False, True])
@pytest.mark.parametrize("width", [1, 4, 16])
@pytest.mark.parametrize("d", [1, 8])
@pytest.mark.parametrize("n0", [60, 520])
def test_without_adapt_and_explore_the_bits_are_the_columns_step(n0, d, width, wide):
    """adapt NULL, explore off: the table, state and run of molann_selftest_opes_step_columns_f64, bit for bit, whatever `biasfactor`
    and `adaptive_stride` hold - on the outputs as they are, and scattered into a wider y."""
    results = []
    for twin in (_columns_twin, _modes_twin):
        table, state, run, (period, _, y, V, sigma0, sigma_min) = scenario_state(n0, d)
        n_out, columns = d, None
        if wide:
            n_out = d + 3
            order = [(3 * k + 2) % n_out for k in range(d)] if d == 1 else [n_out - 1 - k for k in range(d)]
            full = torch.full((y.shape[0], n_out), NAN, dtype=F64)
            full[:, order] = y
            y, columns = full, _capi._i32_array(order)
        for i in range(0, y.shape[0], width):
            assert twin(table, state, run, period, y[i:i + width].contiguous(), columns, V[i:i + width].contiguous(), sigma0, sigma_min, n_out) == 0
        results.append(table + (state, run))
    assert all(torch.equal(a, b) for a, b in zip(*results))
    assert int(results[0][3][0]) > n0 and results[1][4].tolist()[6:] == [0.0, 0.0]


# ---------------------------------------------------------------------------------------------- the C entries
ORDER = ("centers", "sigma", "heights", "capacity", "d", "period", "state", "run", "y", "y_stride", "columns", "V", "v_stride", "n_walkers", "sigma0",
         "sigma_min", "adapt", "beta", "biasfactor", "adaptive_stride", "threshold", "cutoff", "flags")


def _modes_refusals(call):
    """`call(**overrides)` -> code, for the device entry or its host twin: the sibling's refusals in its order, then the new ones."""
    ok = torch.zeros(64, dtype=F64)
    p, odd = ok.data_ptr(), ok.data_ptr() + 4
    base = dict(centers=p, sigma=p, heights=p, capacity=4, d=2, period=None, state=p, run=p, y=p, y_stride=2, columns=None, V=p, v_stride=1,
                n_walkers=1, sigma0=p, sigma_min=None, adapt=None, beta=1.0, biasfactor=10.0, adaptive_stride=4, threshold=1.0, cutoff=5.0, flags=0)
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
    for beta in (0.0, -1.0, NAN, INF):
        assert call(**dict(base, beta=beta)) == _capi.E_DESC
    for thr in (-0.5, NAN, INF):
        assert call(**dict(base, threshold=thr)) == _capi.E_DESC
    for cut in (0.0, -1.0, NAN):
        assert call(**dict(base, cutoff=cut)) == _capi.E_DESC
    # the columns entry's: strides, then the list
    assert call(**dict(base, y_stride=1)) == _capi.E_DESC and call(**dict(base, v_stride=0)) == _capi.E_DESC
    for cols in ((0, 2), (0, 0), (-1, 0)):
        assert call(**dict(base, columns=_capi._i32_array(cols))) == _capi.E_INDEX
    assert call(**dict(base, columns=_capi._i32_array((0, 2)), y_stride=1)) == _capi.E_DESC          # the strides before the list
    assert call(**dict(base, columns=_capi._i32_array((0, 2)), cutoff=0.0)) == _capi.E_DESC          # the sibling's before the columns'
    # the new ones, after all of them
    assert call(**dict(base, adapt=odd)) == _capi.E_ALIGNMENT
    assert call(**dict(base, adapt=odd, columns=_capi._i32_array((0, 0)))) == _capi.E_INDEX
    assert call(**dict(base, flags=ac.OBSERVE)) == _capi.E_DESC                                      # nothing to observe without adapt
    assert call(**dict(base, flags=ac.OBSERVE | ac.EXPLORE)) == _capi.E_DESC
    for stride in (1, 0, -3):
        assert call(**dict(base, adapt=p, adaptive_stride=stride)) == _capi.E_DESC
    for bf in (1.0, 0.5, NAN, INF, -2.0):
        assert call(**dict(base, adapt=p, biasfactor=bf)) == _capi.E_DESC
        assert call(**dict(base, flags=ac.EXPLORE, biasfactor=bf)) == _capi.E_DESC
    # sigma0 may be NULL where adapt is given, and only there
    assert call(**dict(base, adapt=p, sigma0=None, n_walkers=0)) == 0
    assert call(**dict(base, flags=ac.EXPLORE, sigma0=None)) == _capi.E_NULL
    # refused before anything is looked at where n_walkers == 0, too; and nothing is launched there
    assert call(**dict(base, n_walkers=0, d=9)) == _capi.E_DESC
    assert call(**dict(base, n_walkers=0, flags=ac.OBSERVE)) == _capi.E_DESC
    assert call(**dict(base, n_walkers=0, centers=None, y=None, biasfactor=NAN, adaptive_stride=0)) == 0


def test_every_refusal_of_the_modes_entry_and_of_its_host_twin():
    L = _capi.lib()
    _modes_refusals(lambda **kw: L.molann_opes_step_modes_f64(*[kw[k] for k in ORDER], None))      # refused before any launch: no GPU needed
    _modes_refusals(lambda **kw: L.molann_selftest_opes_step_modes_f64(*[kw[k] for k in ORDER]))


def test_the_host_twin_takes_sigma0_null_with_adapt():
    host = ac.HostModes(2, None, None, None, False, False, walkers=2)
    y = torch.tensor([[0.1, 0.2], [0.3, 0.4]], dtype=F64)
    host.call(y, observe=True)
    assert host.run.tolist() == [0.0] * 6 + [1.0, 0.0] and torch.equal(host.adapt[:, 0], y) and not bool(host.adapt[:, 1:].any())
    host.call(y + 0.5, observe=True)       # tau = 2: the mean moves half way, M2 = 0.5 x 0.25
    assert torch.allclose(host.adapt[:, 0], y + 0.25, rtol=0, atol=1e-15) and torch.allclose(host.adapt[:, 1], torch.full((2, 2), 0.125, dtype=F64))


def test_a_walker_that_never_moved_is_refused_and_sigma_min_is_the_cure():
    y = torch.tensor([[0.25, -0.5]], dtype=F64)
    V = torch.zeros(1, dtype=F64)
    for sigma_min, want in ((None, (0, 0, 1)), (torch.tensor([0.05, 0.05], dtype=F64), (1, 0, 0))):
        host = ac.HostModes(2, None, None, sigma_min, False, False, walkers=1, stride=2)
        host.call(y, observe=True)
        host.call(y, V)
        assert host.table.counts() == want and host.run.tolist()[6:] == [2.0, 1.0]
        assert bool(torch.isfinite(host.table.state).all())
        if sigma_min is not None:
            assert torch.equal(host.table.sigma[0], sigma_min) and float(host.table.heights[0]) == 1.0       # sigma0 = s = the floor: ratio 1


def test_the_symbols_are_declared_exported_and_bound():
    L = _capi.lib()
    for name in ("molann_opes_step_modes_f64", "molann_selftest_opes_step_modes_f64"):
        assert name in _capi.declared_symbols()
        fn = getattr(L, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int
    assert len(L.molann_opes_step_modes_f64.argtypes) == len(ORDER) + 1 and len(L.molann_selftest_opes_step_modes_f64.argtypes) == len(ORDER)
    assert L.molann_abi_version() == 1
    assert callable(_capi.opes_step_modes_f64)
    assert (_capi.OPES_FIXED_SIGMA, _capi.OPES_EXPLORE, _capi.OPES_OBSERVE) == (ac.FIXED, ac.EXPLORE, ac.OBSERVE)


# ---------------------------------------------------------------------------------------------- the Python surface
class _Model(object):
    def value_and_opes_table(self, *args, **kwargs):
        raise AssertionError("not called by the constructor")


def _stand_in_table():
    """A table cannot be made without a device; the constructor's refusals come before any device call, so a stand-in that holds what
    it looks at takes its place (tests/test_opes_run_f64_host.py)."""
    table = mbias.OpesTable.__new__(mbias.OpesTable)
    table.d, table.centers = 2, torch.zeros(4, 2, dtype=F64)
    return table


def test_opes_run_adaptive_and_explore_arguments():
    table = _stand_in_table()
    R, good = mbias.OpesRun, dict(kT=1.0, biasfactor=10.0, barrier=20.0, sigma0="adaptive", adaptive_stride=4, walkers=3)
    run = R(_Model(), table, **good)
    assert run.adaptive and not run.explore and run.sigma0 is None and run.adaptive_stride == 4 and run.walkers == 3
    assert run.adapt.shape == (3, 3, 2) and run.adapt.dtype == F64 and not bool(run.adapt.any()) and not bool(run.run.any())
    assert run.scale == 0.9 and run.epsilon == math.exp(-20.0 / 0.9)
    # any other string, and None, stay the TypeError they were
    for bad in ("wide", "Adaptive", "", None):
        with pytest.raises(TypeError, match="sigma0"):
            R(_Model(), table, **dict(good, sigma0=bad))
    for name, low in (("adaptive_stride", 2), ("walkers", 1)):
        with pytest.raises(TypeError, match=name):
            R(_Model(), table, **{k: v for k, v in good.items() if k != name})        # required with "adaptive"
        for bad in (2.5, "4", True, [4]):
            with pytest.raises(TypeError, match=name):
                R(_Model(), table, **dict(good, **{name: bad}))
        for bad in (low - 1, 0, -1):
            with pytest.raises(ValueError, match=name):
                R(_Model(), table, **dict(good, **{name: bad}))
        with pytest.raises(ValueError, match=name):                                   # and they belong to it
            R(_Model(), table, 1.0, 10.0, 20.0, [0.3, 0.3], **{name: 4})
    assert R(_Model(), table, **dict(good, adaptive_stride=2, walkers=1)).adapt.shape == (1, 3, 2)
    # each of the modes needs a finite biasfactor
    with pytest.raises(ValueError, match="biasfactor"):
        R(_Model(), table, **dict(good, biasfactor=INF))
    with pytest.raises(ValueError, match="biasfactor"):
        R(_Model(), table, 1.0, INF, 20.0, [0.3, 0.3], explore=True)
    assert R(_Model(), table, 1.0, INF, 20.0, [0.3, 0.3]).scale == 1.0                # a run in neither mode keeps +inf
    with pytest.raises(TypeError, match="explore"):
        R(_Model(), table, 1.0, 10.0, 20.0, [0.3, 0.3], explore="yes")
    # explore: the other scalars, the same underflow check, and the target's widths
    x = R(_Model(), table, 1.0, 10.0, 20.0, [0.3, 0.4], explore=True)
    assert x.explore and not x.adaptive and x.adapt is None and x.scale == 9.0 and x.epsilon == math.exp(-20.0 / 9.0)
    assert torch.equal(x.sigma0, torch.tensor([0.3, 0.4], dtype=F64) * math.sqrt(10.0))
    with pytest.raises(ValueError, match="underflows"):
        R(_Model(), table, 1.0, 10.0, 1e4, [0.3, 0.3], explore=True)
    both = R(_Model(), table, **dict(good, explore=True, sigma_min=[0.01, 0.01]))
    assert both.adaptive and both.explore and both.scale == 9.0 and both.sigma0 is None
    # a run in neither mode is as it was
    plain = R(_Model(), table, 1.0, 10.0, 20.0, [0.3, 0.3])
    assert not plain.adaptive and not plain.explore and plain.adapt is None and torch.equal(plain.sigma0, torch.tensor([0.3, 0.3], dtype=F64))


def test_observe_and_the_walker_count_are_checked_before_any_device_call():
    table = _stand_in_table()
    fixed = mbias.OpesRun(_Model(), table, 1.0, 10.0, 20.0, [0.3, 0.3])
    y = torch.zeros(3, 2, dtype=F64)
    with pytest.raises(ValueError, match="observe"):
        fixed.observe(y)
    with pytest.raises(ValueError, match="read_adaptive"):
        fixed.read_adaptive()
    run = mbias.OpesRun(_Model(), table, 1.0, 10.0, 20.0, "adaptive", adaptive_stride=4, walkers=3)
    for call in (lambda v: run.observe(v), lambda v: run.deposit(v, torch.zeros(len(v), dtype=F64)),
                 lambda v: run.observe(v, torch.zeros(len(v), dtype=F64))):
        for w in (2, 4, 0):
            with pytest.raises(ValueError, match="3 walkers"):
                call(torch.zeros(w, 2, dtype=F64))
        with pytest.raises(ValueError, match="y"):
            call(torch.zeros(3, 3, dtype=F64))
        with pytest.raises(TypeError, match="float64"):
            call(torch.zeros(3, 2))
        with pytest.raises(TypeError, match="tensor"):
            call([[0.0, 0.0]] * 3)
    with pytest.raises(ValueError, match="bias"):
        run.deposit(y, torch.zeros(2, dtype=F64))
    state = run.read_adaptive()
    assert state["observations"] == 0 and not state["started"]
    assert all(state[k].shape == (3, 2) and state[k].device.type == "cpu" and not bool(state[k].any()) for k in ("mean", "M2", "sigma0"))
    assert set(run.read_run()) == {"counter", "sum_w", "sum_w2", "neff", "sigma_scale", "rct"}


def test_the_docstrings_name_both_modes():
    doc = mbias.OpesRun.__doc__
    for word in ("adaptive", "explore", "adaptive_stride", "walkers", "observe", "sigma_min", "sqrt(biasfactor)", "molann_opes_step_modes_f64"):
        assert word in doc, word
    out = doc[doc.index("Out of scope"):]
    assert "adaptive" not in out and "explore" not in out
    assert "several ranks" in out and "float32" in out and "more than one block" in out and "TorchScript" in out and "restart" in out
    assert "adaptive" in mbias.OpesRun.observe.__doc__ and "sigma0" in mbias.OpesRun.read_adaptive.__doc__
    header = open(_capi.HEADER_PATH).read()
    assert "molann_opes_step_modes_f64" in header and "OPES_METAD_EXPLORE" in header
