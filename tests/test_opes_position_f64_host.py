"""The cases of tests/opes_position_cases.py on the host (no GPU): the host twin `molann_selftest_opes_deposit_f64` (and, for a step,
`molann_selftest_opes_step_f64`) against tests/opes_deposit_oracle.py.  tests/test_gpu_opes_position_f64.py runs the same cases on the
device, where the block's geometry - which lane, wave and stride holds a winner or one of two bit-equal distances - decides the answer;
this file proves that each case takes the path it names before a GPU sees it: the takers, no chain round that was not meant, the
counts, and every search that is no tie on purpose at least 1e-9 (relative) clear of its runner-up and of the threshold."""

import math

import pytest
import torch

import opes_deposit_cases as cases
import opes_deposit_oracle as oracle
import opes_position_cases as pc
import opes_run_cases as rc
import opes_run_oracle as run_oracle

F64 = torch.float64
TIES = pc.tie_cases()


@pytest.mark.parametrize("d", [1, 8])
def test_a_winner_at_every_position(d):
    case = pc.every_position(d)
    ratio, ref = pc.assert_takes_its_path(case)
    assert sorted(case.takers) == list(range(520)) and len(ref.margins) == 2 * 520       # a search that merges, one that finds nobody
    print("smallest margins: threshold %.3g, runner-up %.3g; |S - brute| / bound %.3g, A %.6g"
          % (min(m[0] for m in ref.margins), min(m[1] for m in ref.margins), ratio, ref.A))
    assert ref.A > 1000.0           # the bound on S is far below one pair term (5e-3)


@pytest.mark.parametrize("case", TIES, ids=[c.label for c in TIES])
def test_ties_and_near_ties(case):
    _, ref = pc.assert_takes_its_path(case)
    a, b = sorted(case.heights)[:2]
    assert ref.history == [("merge", case.takers[0])]
    if case.tie == "near":
        assert case.takers == [b], "a strictly smaller q beats the lower slot"
    else:
        assert case.takers == [a]
    # the loser's row is as it was, in the twin too
    _, host, _ = pc.reference(case)
    loser = a if case.tie == "near" else b
    assert torch.equal(host.centers[loser], case.table[0][loser]) and torch.equal(host.sigma[loser], case.table[1][loser])


def test_the_tie_pairs_sit_where_the_block_decides():
    """The nine pairs by thread (slot mod 256), wave and stride: adjacent lanes, the two ends of a butterfly step, neighbouring and
    distant waves, the smaller slot in the higher thread, a stride boundary, one thread's two strides, the ragged last stride."""
    where = {p: tuple((s % 256, (s % 256) // 64, s // 256) for s in p) for p in pc.TIE_PAIRS}
    assert where[(0, 1)] == ((0, 0, 0), (1, 0, 0)) and where[(3, 35)][0][0] ^ where[(3, 35)][1][0] == 32
    assert [w[1] for w in where[(63, 64)]] == [0, 1] and [w[1] for w in where[(10, 200)]] == [0, 3]
    assert where[(200, 260)][0][0] > where[(200, 260)][1][0] and [w[2] for w in where[(255, 256)]] == [0, 1]
    assert where[(7, 263)][0][0] == where[(7, 263)][1][0] and where[(263, 519)] == ((7, 0, 1), (7, 0, 2)) and where[(300, 511)][1][2] == 1
    assert len(set(s // 256 for s in pc.TRIPLE)) == 3


@pytest.mark.parametrize("d", [1, 8])
@pytest.mark.parametrize("n0", pc.SIZES)
def test_table_size_edges(n0, d):
    case = pc.size_edge(n0, d)
    _, ref = pc.assert_takes_its_path(case)
    assert ref.history[-1] == ("append", n0) and ref.seen["merge"] == min(n0, 1) * 3


@pytest.mark.parametrize("d", [1, 8])
def test_a_chain_through_the_whole_table(d):
    case = pc.whole_table_chain(d)
    ratio, ref = pc.assert_takes_its_path(case)
    _, host, _ = pc.reference(case)
    assert ref.seen["chain_rounds_max"] == 299 and ref.seen["hole_fill"] >= 250
    assert abs(float(host.heights[0]) - case.total_height) <= 300 * cases.EPS * case.total_height
    print("smallest runner-up gap %.3g; |S - brute| / bound %.3g, A %.6g" % (min(m[1] for m in ref.margins), ratio, ref.A))


@pytest.mark.parametrize("d", [2, 3, 4, 5, 6, 7])
def test_the_prefilled_scenario_at_every_d(d):
    """`prefilled_scenario(60, d)` as deposits of 4 and as steps of 4 walkers: the host twins against the oracles, every decision clear."""
    period, table, new = cases.prefilled_scenario(60, d)
    host = cases.HostTable(pc.CAP, d, period, pc.CUTOFF, pc.THRESHOLD).fill(*table, cases.brute_force_S(*table, period, pc.CUTOFF))
    ref = oracle.Oracle(pc.CAP, d, period, pc.CUTOFF, pc.THRESHOLD).fill(*table)
    for batch in cases.batches_of(new, 4):
        host.deposit(*batch)
        ref.deposit(*batch)
    assert host.counts() == ref.counts()
    # 60 kernels of width 0.3 crowd [-1, 1)^d at small d, so random neighbours join the planted chains there (the planted slots are
    # asserted where they survive, d >= 5, and at d = 2 nothing is appended); at every d: chain rounds, hole fills, merges, and every
    # decision clear
    if d >= 5:
        cases.assert_scenario_paths(ref, 60)
    assert ref.seen["chain_rounds_max"] >= 1 and ref.seen["hole_fill"] >= 2 and ref.merges >= 3 and ref.refused == 0, ref.seen
    assert min(m[0] for m in ref.margins) >= 1e-9 and min(m[1] for m in ref.margins) >= 1e-9
    n = ref.n
    cases.assert_tables_close(n, (host.centers, host.sigma, host.heights), (ref.centers, ref.sigma, ref.heights), d)
    brute = cases.brute_force_S(host.centers[:n], host.sigma[:n], host.heights[:n], period, pc.CUTOFF)
    assert abs(float(host.state[1]) - brute) <= cases.S_BOUND * max(1.0, ref.A)
    # the steps
    run, (period, table, y, V, sigma0, sigma_min) = rc.host_scenario_run(60, d, 4)
    want = run_oracle.RunOracle(pc.CAP, d, period, pc.CUTOFF, pc.THRESHOLD, rc.KT, rc.BIASFACTOR, rc.BARRIER, sigma0, sigma_min, False)
    want.table.fill(*table)
    want.counter, want.sum_w, want.sum_w2 = int(rc.RUN0[0]), rc.RUN0[1], rc.RUN0[2]
    for i in range(0, 16, 4):
        want.step(y[i:i + 4], V[i:i + 4])
    o, t = want.table, run.table
    assert t.counts() == o.counts() and o.refused == 0 and o.merges >= 4 and o.seen["hole_fill"] >= 2
    assert min(m[0] for m in o.margins) >= 1e-9 and min(m[1] for m in o.margins) >= 1e-9
    assert rc.compare_tables(o.n, (t.centers, t.sigma, t.heights), (o.centers, o.sigma, o.heights)) <= 1.0
    assert rc.compare_scalars(run.run, want.run_values()) <= 1.0


@pytest.mark.parametrize("d", [2, 3, 4, 5, 6, 7])
def test_the_density_cases_are_clear_of_the_cutoff(d):
    """What the device's opes_kernel_sum_f64 is held against at every d: no pair on the cutoff's jump (the formula asserts that), most
    kernels inside it, and every point next to a kernel."""
    from test_gpu_opes_deposit_f64 import _density
    points, centers, heights, sigma, period = pc.density_case(d)
    p, dp, bound_p, _ = _density(points, centers, heights, sigma, period, pc.CUTOFF)
    assert float(p.min()) > 0.1 and float(dp.abs().max()) > 0.0 and bool(torch.isfinite(dp).all())
    s = oracle.wrap(points[:, None, :] - centers[None, :, :], period) / sigma
    inside = ((s * s).sum(dim=2) < pc.CUTOFF ** 2).sum(dim=1)
    assert int(inside.min()) >= 64 and int(inside.max()) <= 300, inside       # more kernels than a wave has lanes


@pytest.mark.parametrize("W", pc.WALKER_COUNTS)
def test_a_step_with_many_walkers(W):
    host, (table, y, V, bad, sigma0) = pc.host_walker_run(W)
    assert len(set(bad)) == 3 and all(0 <= a < W for a in bad)
    if W > 256:
        assert 128 <= bad[0] < 192 and bad[1] >= 256
    ref = run_oracle.RunOracle(pc.CAP, 1, None, pc.CUTOFF, pc.THRESHOLD, rc.KT, rc.BIASFACTOR, rc.BARRIER, sigma0, None, False)
    ref.table.fill(*table)
    ref.step(y, V)
    o, t = ref.table, host.table
    assert t.counts() == o.counts() == (60 + W - 3, 0, 3) and ref.invalid == 3
    assert [h[0] for h in o.history].count("append") == W - 3
    assert min(m[0] for m in o.margins) >= 1e-9 and min(m[1] for m in o.margins) >= 1e-9
    assert rc.compare_tables(o.n, (t.centers, t.sigma, t.heights), (o.centers, o.sigma, o.heights)) <= 1.0
    assert rc.compare_scalars(host.run, ref.run_values()) <= 1.0
    count, sum_w, sum_w2 = pc.walker_sums(W)
    assert float(host.run[0]) == count == W - 3
    assert abs(float(host.run[1]) - sum_w) <= rc.BOUND * max(1.0, sum_w) and abs(float(host.run[2]) - sum_w2) <= rc.BOUND * max(1.0, sum_w2)
    brute = cases.brute_force_S(t.centers[:o.n], t.sigma[:o.n], t.heights[:o.n], None, pc.CUTOFF)
    assert abs(float(t.state[1]) - brute) <= cases.S_BOUND * max(1.0, o.A)
    assert bool(torch.isfinite(host.run).all()) and math.isfinite(float(t.state[1]))
