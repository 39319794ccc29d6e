"""The OPES deposit on the host (no GPU): `molann_selftest_opes_deposit_f64` - the steps and the per-kernel functions of
opes_deposit_f64_kernel compiled for the host, with the device's order of every sum - against tests/opes_deposit_oracle.py, a
sequential float64 restatement in plain torch written from the formulas of include/molann_hip.h.

Decisions compare exactly: q has no exp in it, and every search of every run is asserted to be at least 1e-9 (relative) away from the
threshold and from its runner-up, so a last-bit difference in q cannot change a slot.  Heights and centres are sums and products of
a few values: 4 ulp of their scale.  S is held within 1e-12 max(1, A) of the brute force on the final table, A being the sum of the
magnitudes of every term that went into it: the family's sum bound (tests/test_grid_f64_host.py, tests/test_opes_f64_host.py), here
over at most about 4 x 64 terms per update and 200 updates with exp at 1-2 ulp - roughly 5e-14 of A."""

import ctypes
import itertools
import math

import pytest
import torch

from molann_amd import _capi
from molann_amd import bias as mbias

import opes_deposit_cases as cases
import opes_deposit_oracle as oracle

F64 = torch.float64
INF = math.inf
CAP = 64
RUNS = list(itertools.product((1, 2, 3, 8), (1, 4), (0.0, 0.5, 1.0), (INF, 5.0)))
_ORACLE_RUNS = {}


def _oracle_run(d, width, threshold, cutoff):
    """The oracle's run of a seeded case, computed once and left unchanged."""
    key = (d, width, threshold, cutoff)
    if key not in _ORACLE_RUNS:
        period, batches = cases.seeded_run(d, width, threshold, cutoff)
        ref = oracle.Oracle(CAP, d, period, cutoff, threshold)
        for batch in batches:       # every draw goes in: none is left out
            ref.deposit(*batch)
        _ORACLE_RUNS[key] = ref
    return _ORACLE_RUNS[key]


def t(*values):
    return torch.tensor(values, dtype=F64)


@pytest.mark.parametrize("d,width,threshold,cutoff", RUNS)
def test_seeded_runs_match_the_oracle(d, width, threshold, cutoff):
    period, batches = cases.seeded_run(d, width, threshold, cutoff)
    host = cases.HostTable(CAP, d, period, cutoff, threshold)
    ref = _oracle_run(d, width, threshold, cutoff)
    for batch in batches:           # every draw goes in: none is left out
        host.deposit(*batch)
    n = ref.n
    assert host.counts() == ref.counts(), (host.counts(), ref.counts())
    # the same kernels in the same slots
    cases.assert_tables_close(n, (host.centers, host.sigma, host.heights), (ref.centers, ref.sigma, ref.heights), "slot order or values")
    total = float(host.heights[:n].sum())
    accepted = sum(1 for h in ref.history if h[0] in ("append", "merge"))
    assert abs(total - ref.accepted_height) <= accepted * cases.EPS * ref.accepted_height, (total, ref.accepted_height)
    # S against the brute force on the final table
    brute = cases.brute_force_S(host.centers[:n], host.sigma[:n], host.heights[:n], period, cutoff)
    err = abs(float(host.state[1]) - brute)
    print("n %d merges %d refused %d  S %.17g  |S - brute| / max(1, A) = %.3g  (A = %.6g)" % (host.counts() + (float(host.state[1]), err / max(1.0, ref.A), ref.A)))
    assert err <= cases.S_BOUND * max(1.0, ref.A), (float(host.state[1]), brute, ref.A)
    assert abs(ref.S - brute) <= cases.S_BOUND * max(1.0, ref.A)      # the oracle's own running sum, by the same bound
    # every decision of every draw was clear of the threshold and of its runner-up
    if threshold > 0:
        assert len(ref.margins) >= len(batches) * width - 1
        worst_thr, worst_gap = min(m[0] for m in ref.margins), min(m[1] for m in ref.margins)
        print("smallest margins: threshold %.3g, runner-up %.3g" % (worst_thr, worst_gap))
        assert worst_thr >= 1e-9 and worst_gap >= 1e-9, (worst_thr, worst_gap)
    else:
        assert ref.margins == [] and ref.merges == 0 and n == CAP and ref.refused == len(batches) * width - CAP


def test_the_runs_met_every_path():
    """Over the seeded runs: chains of at least two rounds, a hole filled by the taker itself (t == n - 1), a hole filled by another
    kernel, a full table, and merges across the seam of a periodic column each occurred."""
    seen = [_oracle_run(*run).seen for run in RUNS]
    assert max(s["chain_rounds_max"] for s in seen) >= 2
    for key in ("hole_fill_taker_last", "hole_fill", "full", "seam", "merge", "append"):
        assert sum(s[key] for s in seen) > 0, key


# ---------------------------------------------------------------------------------------------- fixed cases
def test_two_identical_kernels_merge_into_one_of_double_height():
    for d in (1, 3, 8):
        c, s = torch.linspace(-0.7, 0.9, d, dtype=F64).reshape(1, d), torch.linspace(0.2, 0.45, d, dtype=F64).reshape(1, d)
        host = cases.HostTable(4, d, None, INF, 1.0).deposit(torch.cat([c, c]), torch.cat([s, s]), t(0.75, 0.75))
        assert host.counts() == (1, 1, 0)
        assert float(host.heights[0]) == 1.5 and torch.equal(host.centers[0], c[0])
        assert bool(((host.sigma[0] - s[0]).abs() <= 2 * cases.EPS * s[0]).all())
        # S of one kernel is its own term
        assert float(host.state[1]) == 1.5


def test_a_tie_goes_to_the_lower_slot():
    host = cases.HostTable(4, 1, None, INF, 1.0)
    host.fill(t(0.5, -0.5).reshape(2, 1), t(0.6, 0.6).reshape(2, 1), t(1.0, 1.0), 0.0)
    host.deposit(t(0.0).reshape(1, 1), t(0.6).reshape(1, 1), t(1.0))
    # both are at q = (0.5 / 0.6)^2 < 1; slot 0 takes it to 0.25, from where slot 1 is 0.75 / 0.6 widths away: no chain
    assert host.counts() == (2, 1, 0)
    assert float(host.heights[0]) == 2.0 and float(host.centers[0, 0]) == 0.25 and float(host.heights[1]) == 1.0 and float(host.centers[1, 0]) == -0.5
    # the mirrored table gives the mirrored answer: slot 0 took it there too
    mirror = cases.HostTable(4, 1, None, INF, 1.0)
    mirror.fill(t(-0.5, 0.5).reshape(2, 1), t(0.6, 0.6).reshape(2, 1), t(1.0, 1.0), 0.0)
    mirror.deposit(t(0.0).reshape(1, 1), t(0.6).reshape(1, 1), t(1.0))
    assert mirror.counts() == (2, 1, 0) and float(mirror.centers[0, 0]) == -0.25 and float(mirror.centers[1, 0]) == 0.5


def test_threshold_zero_only_appends():
    c = torch.zeros(5, 2, dtype=F64)          # five kernels on one spot
    host = cases.HostTable(8, 2, None, 5.0, 0.0).deposit(c, torch.full((5, 2), 0.3, dtype=F64), torch.ones(5, dtype=F64))
    assert host.counts() == (5, 0, 0)
    assert torch.equal(host.centers[:5], c) and bool((host.heights[:5] == 1.0).all())
    k_self = 1.0 - math.exp(-12.5)
    assert abs(float(host.state[1]) - 25 * k_self) <= 1e-12 * 25


@pytest.mark.parametrize("bad", ["nan_center", "inf_center", "nan_sigma", "zero_sigma", "negative_sigma", "inf_sigma", "nan_height", "zero_height",
                                 "negative_height", "inf_height"])
def test_an_invalid_kernel_is_refused_and_the_others_land_as_if_it_were_absent(bad):
    d = 3
    period, batches = cases.seeded_run(d, 4, 1.0, 5.0, deposits=6)
    with_bad, without = cases.HostTable(16, d, period, 5.0, 1.0), cases.HostTable(16, d, period, 5.0, 1.0)
    for b in batches[:5]:
        with_bad.deposit(*b)
        without.deposit(*b)
    c, s, h = (v.clone() for v in batches[5])
    value = {"nan": math.nan, "inf": math.inf, "zero": 0.0, "negative": -0.3}[bad.split("_")[0]]
    {"center": c, "sigma": s, "height": h}[bad.split("_")[1]][2 if bad.endswith("height") else (2, 1)] = value
    keep = [0, 1, 3]
    with_bad.deposit(c, s, h)
    without.deposit(c[keep], s[keep], h[keep])
    assert with_bad.counts()[2] == without.counts()[2] + 1
    assert torch.equal(with_bad.state[:3], without.state[:3])
    for a, b in ((with_bad.centers, without.centers), (with_bad.sigma, without.sigma), (with_bad.heights, without.heights)):
        assert torch.equal(a, b)          # bitwise, dead rows included
    assert bool(torch.isfinite(with_bad.state).all())


def test_no_new_kernels_changes_nothing():
    host = cases.HostTable(4, 2)
    host.state[:] = t(0.0, 0.0, 3.0, 1.0)
    L = _capi.lib()
    assert L.molann_selftest_opes_deposit_f64(host.centers.data_ptr(), host.sigma.data_ptr(), host.heights.data_ptr(), 4, 2, None, host.state.data_ptr(),
                                              None, None, None, 0, 1.0, INF) == 0
    assert L.molann_opes_deposit_f64(None, None, None, 4, 2, None, None, None, None, None, 0, 1.0, INF, None) == 0       # nothing launched
    assert torch.equal(host.state, t(0.0, 0.0, 3.0, 1.0))


def test_a_state_that_is_not_a_count_cannot_reach_past_the_table():
    """n is held to [0, capacity] whatever the state holds: a NaN or a huge count appends nowhere past the last row."""
    for n0, want in ((math.nan, 1), (1e30, 2), (-5.0, 1)):
        host = cases.HostTable(2, 1, None, INF, 0.0)
        host.state[0] = n0
        host.deposit(t(0.3).reshape(1, 1), t(0.2).reshape(1, 1), t(1.0))
        assert int(host.state[0]) == want and int(host.state[3]) == (1 if want == 2 else 0)


def _refusals(call):
    """`call(**overrides)` -> code, for the device entry or its host twin: every refusal and their order."""
    ok = torch.zeros(16, dtype=F64)
    p, odd = ok.data_ptr(), ok.data_ptr() + 4
    base = dict(centers=p, sigma=p, heights=p, capacity=4, d=2, period=None, state=p, new_centers=p, new_sigma=p, new_heights=p, n_new=1,
                threshold=1.0, cutoff=5.0)
    for name in ("centers", "sigma", "heights", "state", "new_centers", "new_sigma", "new_heights"):
        assert call(**dict(base, **{name: None})) == _capi.E_NULL, name
        assert call(**dict(base, **{name: odd})) == _capi.E_ALIGNMENT, name
        assert call(**dict(base, **{name: None, "d": 0, "period": odd})) == _capi.E_NULL, name      # NULL comes first
    assert call(**dict(base, period=odd)) == _capi.E_ALIGNMENT
    assert call(**dict(base, period=odd, d=9)) == _capi.E_ALIGNMENT                                  # alignment before d
    for d in (0, -1, 9):
        assert call(**dict(base, d=d)) == _capi.E_DESC
    assert call(**dict(base, capacity=0)) == _capi.E_DESC
    assert call(**dict(base, n_new=-1)) == _capi.E_DESC
    assert call(**dict(base, n_new=-1, centers=None)) == _capi.E_DESC       # a NULL pointer matters only where n_new > 0
    for thr in (-0.5, math.nan, math.inf):
        assert call(**dict(base, threshold=thr)) == _capi.E_DESC
    for cut in (0.0, -1.0, math.nan):
        assert call(**dict(base, cutoff=cut)) == _capi.E_DESC
    # refused before anything is looked at where n_new == 0, too
    assert call(**dict(base, n_new=0, d=9)) == _capi.E_DESC
    assert call(**dict(base, n_new=0, centers=None, new_centers=None)) == 0


def test_every_refusal_of_the_entry_and_of_its_host_twin():
    L = _capi.lib()
    order = ("centers", "sigma", "heights", "capacity", "d", "period", "state", "new_centers", "new_sigma", "new_heights", "n_new", "threshold", "cutoff")
    _refusals(lambda **kw: L.molann_opes_deposit_f64(*[kw[k] for k in order], None))      # refused before any launch: no GPU needed
    _refusals(lambda **kw: L.molann_selftest_opes_deposit_f64(*[kw[k] for k in order]))


def test_kernel_sum_refusals():
    L = _capi.lib()
    ok = torch.zeros(16, dtype=F64)
    p, odd = ok.data_ptr(), ok.data_ptr() + 4

    def call(points=p, m=2, d=2, centers=p, heights=p, h=3, sigma=p, stride=0, period=None, cutoff=5.0, out=p, grad=None):
        return L.molann_opes_kernel_sum_f64(points, m, d, centers, heights, h, sigma, stride, period, cutoff, out, grad, None)

    assert call(m=-1) == _capi.E_DESC and call(h=-1) == _capi.E_DESC and call(m=0, points=None) == 0
    for name in ("points", "out", "centers", "heights", "sigma"):
        assert call(**{name: None}) == _capi.E_NULL
        assert call(**{name: odd}) == _capi.E_ALIGNMENT
    assert call(grad=odd) == _capi.E_ALIGNMENT and call(period=odd) == _capi.E_ALIGNMENT
    assert call(d=0) == _capi.E_UNSUPPORTED and call(d=9) == _capi.E_UNSUPPORTED
    assert call(stride=1) == _capi.E_DESC and call(cutoff=0.0) == _capi.E_DESC and call(cutoff=math.nan) == _capi.E_DESC


def test_the_symbols_are_declared_exported_and_bound():
    L = _capi.lib()
    for name in ("molann_opes_deposit_f64", "molann_selftest_opes_deposit_f64", "molann_opes_kernel_sum_f64"):
        assert name in _capi.declared_symbols()
        fn = getattr(L, name)
        assert fn.argtypes is not None and fn.restype is ctypes.c_int
    assert L.molann_abi_version() == 1
    assert callable(_capi.opes_deposit_f64) and callable(_capi.opes_kernel_sum_f64)
    assert "OpesTable" in mbias.__all__


def test_the_operators_are_registered():
    from molann_amd import script
    script.load_ops()
    for name in ("opes_deposit", "opes_kernel_sum"):
        assert hasattr(torch.ops.molann, name)
    schema = str(torch.ops.molann.opes_deposit.default._schema)
    assert "Tensor(a!) centers" in schema and "Tensor(d!) state" in schema and schema.endswith("-> ()")


def test_opes_table_argument_errors():
    T = mbias.OpesTable
    with pytest.raises(ValueError, match="capacity"):
        T(0, 2, "cuda")
    for d in (0, 9):
        with pytest.raises(ValueError, match="`d` must be 1..8"):
            T(8, d, "cuda")
    with pytest.raises(TypeError):
        T(8.5, 2, "cuda")
    with pytest.raises(TypeError):
        T(8, True, "cuda")
    for thr in (-1.0, math.nan, math.inf):
        with pytest.raises(ValueError, match="threshold"):
            T(8, 2, "cuda", threshold=thr)
    for cut in (0.0, -2.0, math.nan):
        with pytest.raises(ValueError, match="cutoff"):
            T(8, 2, "cuda", cutoff=cut)
    with pytest.raises(ValueError, match="device memory"):
        T(8, 2, "cpu")


@pytest.mark.parametrize("n0", [60, 250, 520])
@pytest.mark.parametrize("d", [1, 8])
def test_the_prefilled_scenarios_of_the_device_test(n0, d):
    """tests/test_gpu_opes_deposit_f64.py runs these on the device; here the host twin against the oracle, and the paths they are built
    to meet: a chain round whose taker sits in the last slot, one whose hole the last kernel fills, plain merges, 12 appends."""
    cutoff, threshold = 5.0, 1.0
    period, table, new = cases.prefilled_scenario(n0, d)
    brute = cases.brute_force_S(*_csh(table), period, cutoff)
    host = cases.HostTable(600, d, period, cutoff, threshold).fill(*table, brute)
    ref = oracle.Oracle(600, d, period, cutoff, threshold).fill(*table)
    for batch in cases.batches_of(new, 4):
        host.deposit(*batch)
        ref.deposit(*batch)
    assert host.counts() == ref.counts(), (host.counts(), ref.counts())
    cases.assert_scenario_paths(ref, n0)
    assert min(m[0] for m in ref.margins) >= 1e-9 and min(m[1] for m in ref.margins) >= 1e-9
    n = ref.n
    cases.assert_tables_close(n, (host.centers, host.sigma, host.heights), (ref.centers, ref.sigma, ref.heights), "slot order or values")
    brute = cases.brute_force_S(host.centers[:n], host.sigma[:n], host.heights[:n], period, cutoff)
    assert abs(float(host.state[1]) - brute) <= cases.S_BOUND * max(1.0, ref.A), (float(host.state[1]), brute, ref.A)


def _csh(table):
    return table[0], table[1], table[2]
