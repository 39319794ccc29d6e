"""The block-parallel half of opes_deposit_f64_kernel and opes_step_f64_kernel - the strided search, the __shfl_xor butterfly on (q, slot)
with its tie rule, the four waves' pairs through LDS, the strided partial sums, `store` and `move` between barriers - on the cases of
tests/opes_position_cases.py, which tests/test_opes_position_f64_host.py holds against the oracle on the CPU.  The host twin has a plain
loop where the device has its geometry, so here the cases are built for the geometry to decide the answer:

  positions  one deposit of 520 kernels, each next to another slot of a 520-kernel table: a winner in every lane, wave and stride
  ties       two (three) slots at bit-equal q in adjacent lanes, at the two ends of a butterfly step, in neighbouring and distant
             waves, with the smaller slot in the higher thread, across a stride boundary, in one thread's two strides and in the
             ragged last stride; and one ulp apart, where the tie rule must not be asked
  sizes      tables of 0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 512 and 513 kernels
  chain      300 kernels collapse into one in 300 merges of one new kernel's chain
  every d    the prefilled scenario as deposits and as steps, and the density, at d = 2 .. 7
  walkers    steps of 65, 257 and 300 walkers with three invalid ones
  state      a count that is NaN, huge or negative, between guard bands

Per deposit: the counts equal the twin's, the oracle's and the case's own; every slot that took kernels holds exactly the fold of
their heights (stated by the case, not by the twin); centres and heights have the twin's bits and widths are within 1 ulp (sqrt) - the
standard of tests/test_gpu_opes_deposit_f64.py; S is within 1e-12 max(1, A) of the brute force on the device's final table."""

import math

import pytest
import torch

import opes_deposit_cases as cases
import opes_deposit_oracle as oracle
import opes_position_cases as pc
import opes_run_cases as rc
import placement as pl
import test_gpu_opes_deposit_f64 as gd
import test_gpu_opes_run_f64 as gr
from molann_amd import _capi
from molann_amd import bias as mbias

pytestmark = pytest.mark.gpu
F64 = torch.float64
NAN = math.nan
TIES = pc.tie_cases()
_WORST = {}


def _deposit(dev, case):
    """The case's one deposit on a fresh device table."""
    total0, _, _ = pc.reference(case)
    t = mbias.OpesTable(case.capacity, case.d, dev, period=None, cutoff=pc.CUTOFF, threshold=case.threshold)
    n0 = case.n0
    if n0:
        t.centers[:n0], t.sigma[:n0], t.heights[:n0] = (v.to(dev) for v in case.table)
    t.state[:2] = torch.tensor([float(n0), total0], dtype=F64).to(dev)
    t.deposit(*(v.to(dev) for v in case.new))
    torch.cuda.synchronize()
    return t


def _check(dev, case, family):
    """The checks every deposit case shares; returns the device's table on the CPU (centers, sigma, heights)."""
    _, host, ref = pc.reference(case)
    t = _deposit(dev, case)
    n, total, merges, refused = t.read_state()
    assert (n, merges, refused) == host.counts() == ref.counts() == case.counts, (case.label, (n, merges, refused), host.counts(), case.counts)
    centers, sigma, heights = t.centers.cpu(), t.sigma.cpu(), t.heights.cpu()
    wrong = [slot for slot, h in case.heights.items() if float(heights[slot]) != h]
    assert wrong == [], "%s: slots %s do not hold the heights of their own kernels" % (case.label, wrong[:8])
    assert pl.same_bits(centers[:n], host.centers[:n]), "%s: centres (or the slot order)" % case.label
    assert pl.same_bits(heights[:n], host.heights[:n]), "%s: heights" % case.label
    ulps = gd._ulps(sigma[:n], host.sigma[:n])
    brute = cases.brute_force_S(centers[:n], sigma[:n], heights[:n], None, pc.CUTOFF)
    ratio = abs(total - brute) / (cases.S_BOUND * max(1.0, ref.A))
    worst = _WORST.setdefault(family, [0.0, 0.0])
    worst[0], worst[1] = max(worst[0], ratio), max(worst[1], ulps)
    print("%s: |S - brute| / bound %.3g (A %.6g), widths %.3g ulp from the host; %s so far: %.3g, %.3g ulp"
          % (case.label, ratio, ref.A, ulps, family, worst[0], worst[1]))
    assert ulps <= 1.0, case.label
    assert ratio <= 1.0, (case.label, total, brute, ref.A)
    return centers, sigma, heights


@pytest.mark.parametrize("d", [1, 8])
def test_a_winner_at_every_position(d, hip_device):
    _check(hip_device, pc.every_position(d), "positions")


@pytest.mark.parametrize("case", TIES, ids=[c.label for c in TIES])
def test_ties_and_near_ties(case, hip_device):
    """The taker, read from the heights: the lower slot of two (three) at bit-equal q, and the nearer one where they differ by an ulp."""
    _, _, heights = _check(hip_device, case, "ties")
    took = [slot for slot in case.heights if float(heights[slot]) != float(case.table[2][slot])]
    assert took == case.takers, (case.label, took, case.takers)


@pytest.mark.parametrize("d", [1, 8])
@pytest.mark.parametrize("n0", pc.SIZES)
def test_table_size_edges(n0, d, hip_device):
    _check(hip_device, pc.size_edge(n0, d), "sizes")


@pytest.mark.parametrize("d", [1, 8])
def test_a_chain_through_the_whole_table(d, hip_device):
    case = pc.whole_table_chain(d)
    _, _, ref = pc.reference(case)
    centers, sigma, heights = _check(hip_device, case, "chain")
    assert abs(float(heights[0]) - case.total_height) <= 300 * cases.EPS * case.total_height, (float(heights[0]), case.total_height)
    cases.assert_tables_close(1, (centers, sigma, heights), (ref.centers, ref.sigma, ref.heights), case.label)


# ---------------------------------------------------------------------------------------------- every d
@pytest.mark.parametrize("d", [2, 3, 4, 5, 6, 7])
def test_deposits_at_every_d(d, hip_device):
    dev = hip_device
    period, table, new = cases.prefilled_scenario(60, d)
    total0 = cases.brute_force_S(*table, period, pc.CUTOFF)
    host = cases.HostTable(pc.CAP, d, period, pc.CUTOFF, pc.THRESHOLD).fill(*table, total0)
    ref = oracle.Oracle(pc.CAP, d, period, pc.CUTOFF, pc.THRESHOLD).fill(*table)
    t = gd._device_table(dev, d, period, table, total0)
    for c, s, h in cases.batches_of(new, 4):
        host.deposit(c, s, h)
        ref.deposit(c, s, h)
        t.deposit(c.to(dev), s.to(dev), h.to(dev))
    n, total, merges, refused = t.read_state()
    assert (n, merges, refused) == host.counts() == ref.counts()
    centers, sigma, heights = t.centers.cpu(), t.sigma.cpu(), t.heights.cpu()
    assert pl.same_bits(centers[:n], host.centers[:n]) and pl.same_bits(heights[:n], host.heights[:n])
    ulps = gd._ulps(sigma[:n], host.sigma[:n])
    brute = cases.brute_force_S(centers[:n], sigma[:n], heights[:n], period, pc.CUTOFF)
    ratio = abs(total - brute) / (cases.S_BOUND * max(1.0, ref.A))
    print("d %d: n %d merges %d; |S - brute| / bound %.3g (A %.6g), widths %.3g ulp from the host" % (d, n, merges, ratio, ref.A, ulps))
    assert ulps <= 1.0 and ratio <= 1.0


@pytest.mark.parametrize("d", [2, 3, 4, 5, 6, 7])
def test_steps_at_every_d(d, hip_device):
    host, sc = rc.host_scenario_run(60, d, 4)
    t, run = gr._device_run(hip_device, sc, 60)
    y, V = sc[2].to(hip_device), sc[3].to(hip_device)
    for i in range(0, 16, 4):
        run.deposit(y[i:i + 4], V[i:i + 4])
    got = gr._snapshot(t, run)
    worst, bits = rc.assert_same_run(got, host.snapshot(), d)
    print("d %d: worst error / bound %.3g, %s" % (d, worst, "the host's bits" if bits else "exp, pow or sqrt an ulp off"))
    assert float(got[4][0]) == rc.RUN0[0] + 16


@pytest.mark.parametrize("d", [2, 3, 4, 5, 6, 7])
def test_the_density_at_every_d(d, hip_device):
    dev = hip_device
    points, centers, heights, sigma, period = pc.density_case(d)
    want_p, want_dp, bound_p, bound_dp = gd._density(points, centers, heights, sigma, period, pc.CUTOFF)
    P = torch.full((5,), NAN, dtype=F64, device=dev)
    dP = torch.full((5, d), NAN, dtype=F64, device=dev)
    with torch.cuda.device(dev):
        _capi.opes_kernel_sum_f64(points.to(dev), centers.to(dev), heights.to(dev), sigma.to(dev), period.to(dev), pc.CUTOFF, P, dP)
    torch.cuda.synchronize()
    err_p, err_dp = (P.cpu() - want_p).abs(), (dP.cpu() - want_dp).abs()
    print("d %d: P worst error / bound %.3g; dP: %.3g" % (d, float((err_p / bound_p).max()), float((err_dp / bound_dp.clamp(min=1e-300)).max())))
    assert bool((err_p <= bound_p).all()) and bool((err_dp <= bound_dp).all())


# ---------------------------------------------------------------------------------------------- many walkers
@pytest.mark.parametrize("W", pc.WALKER_COUNTS)
def test_a_step_with_many_walkers(W, hip_device):
    host, (table, y, V, bad, sigma0) = pc.host_walker_run(W)
    t, run = gr._device_run(hip_device, (None, table, y, V, sigma0, None), 60)
    run.run.zero_()                 # the run has not started
    run.deposit(y.to(hip_device), V.to(hip_device))
    got = gr._snapshot(t, run)
    count, sum_w, sum_w2 = pc.walker_sums(W)
    assert float(got[4][0]) == count == W - 3
    print("W %d: sum_w %.17g (fsum %.17g), sum_w2 %.17g (fsum %.17g)" % (W, float(got[4][1]), sum_w, float(got[4][2]), sum_w2))
    assert abs(float(got[4][1]) - sum_w) <= rc.BOUND * max(1.0, sum_w)
    assert abs(float(got[4][2]) - sum_w2) <= rc.BOUND * max(1.0, sum_w2)
    assert (int(got[3][0]), int(got[3][2]), int(got[3][3])) == (60 + W - 3, 0, 3)
    worst, bits = rc.assert_same_run(got, host.snapshot(), W)
    print("W %d: worst error / bound %.3g, %s" % (W, worst, "the host's bits" if bits else "exp or pow an ulp off"))
    n = 60 + W - 3
    brute = cases.brute_force_S(got[0][:n], got[1][:n], got[2][:n], None, pc.CUTOFF)
    assert abs(float(got[3][1]) - brute) <= cases.S_BOUND * max(1.0, brute)      # every term is positive: A is the sum itself


# ---------------------------------------------------------------------------------------------- a state that is not a count
@pytest.mark.parametrize("offset", [0, 1])
@pytest.mark.parametrize("n0,want_n,want_refused", [(NAN, 1, 0), (1e30, 2, 1), (-5.0, 1, 0)], ids=["nan", "huge", "negative"])
def test_a_state_that_is_not_a_count_stays_inside_the_table(n0, want_n, want_refused, offset, hip_device):
    """Capacity 2, threshold 0 (every kernel is appended): n is held to [0, capacity] before any access, so the kernel lands in row 0
    or is refused by a table that counts as full; no guard band and no input changes, and the state has the host twin's bits."""
    dev = hip_device
    arena = pl.Arena(dev, capacity=1 << 20)
    centers, sigma = arena.carve("centers", (2, 1), F64, offset), arena.carve("sigma", (2, 1), F64, offset)
    heights, state = arena.carve("heights", (2,), F64, offset, row_dims=0), arena.carve("state", (4,), F64, offset, row_dims=0)
    nc = arena.carve("new_centers", (1, 1), F64, offset, data=torch.tensor([[0.3]], dtype=F64))
    ns = arena.carve("new_sigma", (1, 1), F64, offset, data=torch.tensor([[0.2]], dtype=F64))
    nh = arena.carve("new_heights", (1,), F64, offset, data=torch.tensor([1.0], dtype=F64), row_dims=0)
    centers.zero_(), sigma.zero_(), heights.zero_()
    state.copy_(torch.tensor([n0, 0.0, 0.0, 0.0], dtype=F64))
    host = cases.HostTable(2, 1, None, math.inf, 0.0)
    host.state[0] = n0
    host.deposit(torch.tensor([[0.3]], dtype=F64), torch.tensor([[0.2]], dtype=F64), torch.tensor([1.0], dtype=F64))
    with torch.cuda.device(dev):
        _capi.opes_deposit_f64(centers, sigma, heights, state, None, nc, ns, nh, 0.0, None)
    torch.cuda.synchronize()
    assert arena.check() == [] and arena.inputs_changed() == []
    got = state.cpu()
    assert (int(got[0]), int(got[3])) == (want_n, want_refused) == (int(host.state[0]), int(host.state[3])), got
    assert pl.same_bits(got, host.state)
    assert pl.same_bits(centers.cpu(), host.centers) and pl.same_bits(sigma.cpu(), host.sigma) and pl.same_bits(heights.cpu(), host.heights)
