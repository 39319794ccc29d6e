"""The OPES deposit on the device: opes_deposit_f64_kernel (one launch per deposit, `molann_amd.bias.OpesTable.deposit`) against its host
twin `molann_selftest_opes_deposit_f64` on the same inputs, and opes_kernel_sum_f64_kernel against the float64 formula on the CPU.

The tables are tests/opes_deposit_cases.py's prefilled scenarios (checked against the oracle on the host by
tests/test_opes_deposit_f64_host.py): 60, 250 and 520 live kernels under a capacity of 600 - one, two and three strided rounds of the
block's 256 threads, the last one ragged, n crossing 64 and 256 - with d in {1, 8} and 16 new kernels that meet a chain round whose
taker sits in the last slot, one whose hole the last kernel fills, plain merges and 12 appends.  Counts and slots compare exactly,
centres and heights bit for bit (IEEE add, multiply, divide and rint with contraction off), widths within 1 ulp (sqrt), S within
1e-12 max(1, A) of the brute force on the CPU - the host file's bound, A from the oracle."""

import math

import pytest
import torch

import opes_deposit_cases as cases
import opes_deposit_oracle as oracle
import placement as pl
import test_gpu_value_and_vjp_f64 as vv
from molann_amd import _capi
from molann_amd import bias as mbias

pytestmark = pytest.mark.gpu
F64 = torch.float64
INF = math.inf
CAP, CUTOFF, THRESHOLD = 600, 5.0, 1.0
_REFERENCE = {}


def _reference(n0, d):
    """Per scenario, once: the inputs, the prefilled table's S, the host twin's final table (deposits of 4) and the oracle's record."""
    if (n0, d) not in _REFERENCE:
        period, table, new = cases.prefilled_scenario(n0, d)
        total0 = cases.brute_force_S(*table, period, CUTOFF)
        host = cases.HostTable(CAP, d, period, CUTOFF, THRESHOLD).fill(*table, total0)
        ref = oracle.Oracle(CAP, d, period, CUTOFF, THRESHOLD).fill(*table)
        for batch in cases.batches_of(new, 4):
            host.deposit(*batch)
            ref.deposit(*batch)
        assert host.counts() == ref.counts()
        cases.assert_scenario_paths(ref, n0)
        _REFERENCE[(n0, d)] = (period, table, new, total0, host, ref)
    return _REFERENCE[(n0, d)]


def _device_table(dev, d, period, table, total0, threshold=THRESHOLD, cutoff=CUTOFF):
    t = mbias.OpesTable(CAP, d, dev, period=period, cutoff=cutoff, threshold=threshold)
    n0 = table[0].shape[0]
    t.centers[:n0], t.sigma[:n0], t.heights[:n0] = (v.to(dev) for v in table)
    t.state[:2] = torch.tensor([float(n0), total0], dtype=F64).to(dev)
    return t


def _run(dev, n0, d, width):
    period, table, new, total0, _, _ = _reference(n0, d)
    t = _device_table(dev, d, period, table, total0)
    for c, s, h in cases.batches_of(new, width):
        t.deposit(c.to(dev), s.to(dev), h.to(dev))
    torch.cuda.synchronize()
    return t


def _ulps(got, want):
    return float(((got - want).abs() / (cases.EPS * want.abs())).max())


@pytest.mark.parametrize("width", [1, 4])
@pytest.mark.parametrize("d", [1, 8])
@pytest.mark.parametrize("n0", [60, 250, 520])
def test_the_device_matches_its_host_twin(n0, d, width, hip_device):
    period, _, _, _, host, ref = _reference(n0, d)
    t = _run(hip_device, n0, d, width)
    n, total, merges, refused = t.read_state()
    assert (n, merges, refused) == host.counts(), ((n, merges, refused), host.counts())
    assert n > n0 and (n0 > 256 or (n0 < 64 < n) or (n0 < 256 < n))
    centers, sigma, heights = t.centers.cpu(), t.sigma.cpu(), t.heights.cpu()
    assert pl.same_bits(centers[:n], host.centers[:n]), "centres (or the slot order)"
    assert pl.same_bits(heights[:n], host.heights[:n]), "heights"
    worst = _ulps(sigma[:n], host.sigma[:n])
    print("widths: largest difference from the host %.3g ulp (%s)" % (worst, "the same bits" if worst == 0 else "sqrt"))
    assert worst <= 1.0
    brute = cases.brute_force_S(centers[:n], sigma[:n], heights[:n], period, CUTOFF)
    print("S %.17g  host %.17g  brute force %.17g  |S - brute| / max(1, A) = %.3g" % (total, float(host.state[1]), brute, abs(total - brute) / max(1.0, ref.A)))
    assert abs(total - brute) <= cases.S_BOUND * max(1.0, ref.A)


def test_two_runs_give_the_same_bits(hip_device):
    a, b = _run(hip_device, 250, 8, 4), _run(hip_device, 250, 8, 4)
    for x, y in ((a.centers, b.centers), (a.sigma, b.sigma), (a.heights, b.heights), (a.state, b.state)):
        assert pl.same_bits(x, y)


@pytest.mark.parametrize("d", [1, 8])
def test_queued_deposits_equal_one_deposit_of_the_concatenation(d, hip_device):
    """Two deposits queued with no read between them, and sixteen of one kernel each, against one deposit of all sixteen: the launch
    reads n and S where the one before left them, so the bits are the same everywhere, S included."""
    dev = hip_device
    period, table, new, total0, _, _ = _reference(250, d)
    one = _device_table(dev, d, period, table, total0)
    one.deposit(*(v.to(dev) for v in new))
    two = _device_table(dev, d, period, table, total0)
    for c, s, h in cases.batches_of(new, 8):
        two.deposit(c.to(dev), s.to(dev), h.to(dev))
    many = _run(dev, 250, d, 1)
    torch.cuda.synchronize()
    for other in (two, many):
        for x, y in ((one.centers, other.centers), (one.sigma, other.sigma), (one.heights, other.heights), (one.state, other.state)):
            assert pl.same_bits(x, y)


def test_an_invalid_kernel_is_refused_on_the_device(hip_device):
    dev = hip_device
    period, table, new, total0, _, _ = _reference(60, 8)
    c, s, h = (v[:4].clone() for v in new)
    c[2, 3], keep = math.nan, [0, 1, 3]
    with_bad, without = _device_table(dev, 8, period, table, total0), _device_table(dev, 8, period, table, total0)
    with_bad.deposit(c.to(dev), s.to(dev), h.to(dev))
    without.deposit(c[keep].to(dev), s[keep].to(dev), h[keep].to(dev))
    assert with_bad.read_state()[3] == 1 and without.read_state()[3] == 0
    assert pl.same_bits(with_bad.state[:3], without.state[:3])
    for x, y in ((with_bad.centers, without.centers), (with_bad.sigma, without.sigma), (with_bad.heights, without.heights)):
        assert pl.same_bits(x, y)


@pytest.mark.parametrize("offset", [0, 1])
def test_guard_bands_around_the_table_and_rows_past_the_capacity(offset, hip_device):
    """The four buffers and the new kernels in an arena of guard bands, the table FULL after the run (capacity = n0 + 3: appends are
    refused from there on): nothing before a buffer, nothing after its last row, and the inputs as they were."""
    dev, n0, d = hip_device, 60, 8
    period, table, new, total0, _, _ = _reference(n0, d)
    cap = n0 + 3
    arena = pl.Arena(dev, capacity=4 << 20)
    centers, sigma = arena.carve("centers", (cap, d), F64, offset), arena.carve("sigma", (cap, d), F64, offset)
    heights, state = arena.carve("heights", (cap,), F64, offset, row_dims=0), arena.carve("state", (4,), F64, offset, row_dims=0)
    per = arena.carve("period", (d,), F64, offset, data=period, row_dims=0)
    nc, ns = arena.carve("new_centers", new[0].shape, F64, offset, data=new[0]), arena.carve("new_sigma", new[1].shape, F64, offset, data=new[1])
    nh = arena.carve("new_heights", new[2].shape, F64, offset, data=new[2], row_dims=0)
    centers.zero_(), sigma.zero_(), heights.zero_()
    centers[:n0], sigma[:n0], heights[:n0] = (v.to(dev) for v in table)
    state.copy_(torch.tensor([float(n0), total0, 0.0, 0.0], dtype=F64))
    host = cases.HostTable(cap, d, period, CUTOFF, THRESHOLD).fill(*table, total0).deposit(*new)
    with torch.cuda.device(dev):
        _capi.opes_deposit_f64(centers, sigma, heights, state, per, nc, ns, nh, THRESHOLD, CUTOFF)
    torch.cuda.synchronize()
    assert arena.check() == [] and arena.inputs_changed() == []
    got = state.cpu()
    assert (int(got[0]), int(got[2]), int(got[3])) == host.counts() and int(got[0]) == cap and int(got[3]) > 0, (got, host.counts())
    assert pl.same_bits(centers.cpu(), host.centers) and pl.same_bits(heights.cpu(), host.heights)


# ---------------------------------------------------------------------------------------------- the density at arbitrary points
def _density(points, centers, heights, sigma, period, cutoff):
    """(P [M], dP [M, d], the bound on P, the bound on dP) of the formula in float64 on the CPU; the bounds as tests/test_opes_f64_host.py
    has them for the sums before the logarithm: 1e-12 of the sum of the terms' magnitudes."""
    delta = oracle.wrap(points[:, None, :] - centers[None, :, :], period)
    sig = sigma.expand(centers.shape[0], points.shape[1])
    s = delta / sig
    q = (s * s).sum(dim=2)
    c2 = cutoff * cutoff
    inside = q < c2
    e = torch.exp(-0.5 * q)
    terms = torch.where(inside, heights * (e - math.exp(-0.5 * c2)), torch.zeros_like(q))
    grads = torch.where(inside[:, :, None], -(heights * e)[:, :, None] * s / sig, torch.zeros_like(s))
    assert centers.shape[0] == 0 or float((q - c2).abs().min()) > 1e-6         # no pair on the cutoff's jump
    return terms.sum(dim=1), grads.sum(dim=1), 1e-12 * terms.abs().sum(dim=1), 1e-12 * grads.abs().sum(dim=1)


@pytest.mark.parametrize("cutoff", [INF, 5.0], ids=["no_cutoff", "cutoff_5"])
@pytest.mark.parametrize("per_kernel", [False, True], ids=["shared_sigma", "sigma_per_kernel"])
@pytest.mark.parametrize("n_kernels", [0, 1, 300])
@pytest.mark.parametrize("m", [1, 65])
def test_kernel_sum_against_the_formula(m, n_kernels, per_kernel, cutoff, hip_device):
    dev, d = hip_device, 3
    g = torch.Generator().manual_seed(31 * m + n_kernels + (7 if per_kernel else 0))
    period = torch.tensor([2.0, 0.0, 2.0], dtype=F64)
    centers = 2.0 * torch.rand(n_kernels, d, dtype=F64, generator=g) - 1.0
    heights = 0.5 + torch.rand(n_kernels, dtype=F64, generator=g)
    sigma = 0.3 * (0.8 + 0.4 * torch.rand((n_kernels, d) if per_kernel else (d,), dtype=F64, generator=g))
    points = 2.4 * torch.rand(m, d, dtype=F64, generator=g) - 1.2
    if n_kernels:
        points[0] = centers[0] + 0.1          # a point next to a kernel, whatever the draw
    want_p, want_dp, bound_p, bound_dp = _density(points, centers, heights, sigma, period, cutoff)
    on = lambda v: v.to(dev)        # noqa: E731
    P = torch.full((m,), math.nan, dtype=F64, device=dev)
    dP = torch.full((m, d), math.nan, dtype=F64, device=dev)
    with torch.cuda.device(dev):
        alone = _capi.opes_kernel_sum_f64(on(points), on(centers), on(heights), on(sigma), on(period), None if math.isinf(cutoff) else cutoff,
                                          torch.full((m,), math.nan, dtype=F64, device=dev))
        _capi.opes_kernel_sum_f64(on(points), on(centers), on(heights), on(sigma), on(period), None if math.isinf(cutoff) else cutoff, P, dP)
    torch.cuda.synchronize()
    assert pl.same_bits(alone, P)           # with and without the derivative: the same P
    err_p, err_dp = (P.cpu() - want_p).abs(), (dP.cpu() - want_dp).abs()
    print("P: worst error / bound %.3g; dP: %.3g" % (float((err_p / bound_p.clamp(min=1e-300)).max()), float((err_dp / bound_dp.clamp(min=1e-300)).max())))
    assert bool((err_p <= bound_p).all()) and bool((err_dp <= bound_dp).all())
    if n_kernels == 0:
        assert bool((P == 0).all()) and bool((dP == 0).all())
    else:
        assert float(want_p[0]) > 0.1
    # the operator gives the same bits
    from molann_amd import script
    script.load_ops()
    got = torch.ops.molann.opes_kernel_sum(on(points), on(centers), on(heights), on(sigma), on(period), cutoff, True)
    assert pl.same_bits(got[0], P) and pl.same_bits(got[1], dP)


def test_recompute_sum_agrees_with_the_incremental_sum(hip_device):
    _, _, _, _, _, ref = _reference(520, 8)
    t = _run(hip_device, 520, 8, 4)
    n, incremental, _, _ = t.read_state()
    again = float(t.recompute_sum())
    assert t.read_state()[1] == again
    print("incremental %.17g, from scratch %.17g, difference / max(1, A) = %.3g" % (incremental, again, abs(incremental - again) / max(1.0, ref.A)))
    assert abs(incremental - again) <= cases.S_BOUND * max(1.0, ref.A)
    # and the operator deposits as the ctypes call does
    from molann_amd import script
    script.load_ops()
    period, table, new, total0, _, _ = _reference(520, 8)
    dev = hip_device
    other = _device_table(dev, 8, period, table, total0)
    for c, s, h in cases.batches_of(new, 4):
        torch.ops.molann.opes_deposit(other.centers, other.sigma, other.heights, other.state, other.period, c.to(dev), s.to(dev), h.to(dev), THRESHOLD,
                                      CUTOFF)
    torch.cuda.synchronize()
    assert pl.same_bits(other.centers, t.centers) and pl.same_bits(other.sigma, t.sigma) and pl.same_bits(other.heights, t.heights)
    assert pl.same_bits(other.state[[0, 2, 3]], t.state[[0, 2, 3]]) and float(other.state[1]) == incremental


def test_end_to_end_on_c3(hip_device):
    """C3's float64 model, 65 frames: their outputs are deposited as kernels - the widths and the heights by torch arithmetic on the
    device, nothing read back in between - and `value_and_opes` / `value_and_bias` with `table.record(...)` give, bit for bit, what they
    give with the same table uploaded from the CPU."""
    dev = hip_device
    w, model, _ = vv._shared("C3", dev)
    x = w.make_frames(65, seed=411).double().to(dev)
    d = w.out_dim()
    table = mbias.OpesTable(128, d, dev, period=None, cutoff=5.0, threshold=1.0)
    y0, bias0, _ = model.value_and_opes(x, table.centers[:0], table.heights[:0], table.sigma[:0], 2.25, 1.0, 1e-3, 5.0)
    spread = y0.std(dim=0) * 0.4 + 1e-3
    weights = torch.exp(bias0 / 2.25) * 800.0             # the deposits' heights from the bias, on the device
    ref = oracle.Oracle(128, d, None, 5.0, 1.0)
    for lo in range(0, 65, 13):                       # five deposits queued back to back
        table.deposit(y0[lo:lo + 13], spread, weights[lo:lo + 13])
        ref.deposit(y0[lo:lo + 13].cpu(), spread.cpu().expand(13, d), weights[lo:lo + 13].cpu())
    n, total, merges, refused = table.read_state()
    assert (n, merges, refused) == ref.counts() and n + merges == 65 and refused == 0 and n >= 2, ((n, merges, refused), ref.counts())
    rec = table.record(2.25, 0.02 * float(table.heights[:n].sum()), 1e-3)
    assert rec.centers.is_contiguous() and rec.centers.data_ptr() == table.centers.data_ptr() and rec.centers.shape == (n, d)
    fresh = [v.cpu().clone().to(dev) for v in (rec.centers, rec.heights, rec.sigma)]
    got = model.value_and_opes(x, rec.centers, rec.heights, rec.sigma, rec.scale, rec.norm, rec.epsilon, rec.cutoff, rec.period)
    want = model.value_and_opes(x, fresh[0], fresh[1], fresh[2], rec.scale, rec.norm, rec.epsilon, rec.cutoff, None)
    for a, b in zip(got, want):
        assert pl.same_bits(a, b)
    assert bool(torch.isfinite(got[1]).all()) and float(got[2].abs().max()) > 0
    got_b = model.value_and_bias(x, opes=rec)
    want_b = model.value_and_bias(x, opes=mbias.Opes(fresh[0], fresh[1], fresh[2], rec.scale, rec.norm, rec.epsilon, rec.cutoff))
    for a, b in zip(got_b, want_b):
        assert pl.same_bits(a, b)
    # S of the table the run left, against the CPU
    brute = cases.brute_force_S(rec.centers.cpu(), rec.sigma.cpu(), rec.heights.cpu(), None, 5.0)
    assert abs(total - brute) <= cases.S_BOUND * max(1.0, ref.A), (total, brute, ref.A)
