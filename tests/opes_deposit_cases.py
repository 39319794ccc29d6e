"""What the OPES deposit tests share (tests/test_opes_deposit_f64_host.py and tests/test_gpu_opes_deposit_f64.py): seeded runs of new
kernels, the host twin `molann_selftest_opes_deposit_f64` on torch CPU tensors, and the checks of a table against another."""

import math

import torch

from molann_amd import _capi
from molann_amd import bias as mbias

import opes_deposit_oracle as oracle

F64 = torch.float64
EPS = 2.0 ** -52
S_BOUND = 1e-12      # of max(1, A): the family's sum bound (test_grid_f64_host, test_opes_f64_host)


def mixed_period(d):
    """Columns 0, 2, ... periodic with period 2, the others not."""
    return torch.tensor([2.0 if k % 2 == 0 else 0.0 for k in range(d)], dtype=F64)


def seeded_run(d, width, threshold, cutoff, deposits=200):
    """`deposits` batches of `width` kernels along one random walk that starts next to the seam of the periodic columns."""
    seed = 1000 * d + 100 * width + int(10 * threshold) + (1 if math.isfinite(cutoff) else 0)
    g = torch.Generator().manual_seed(seed)
    period = mixed_period(d)
    c, s, h = oracle.random_walk_kernels(g, deposits * width, d, period, start=0.9)
    return period, [(c[i:i + width].contiguous(), s[i:i + width].contiguous(), h[i:i + width].contiguous()) for i in range(0, deposits * width, width)]


class HostTable(object):
    """A table in host memory under `molann_selftest_opes_deposit_f64`."""

    def __init__(self, capacity, d, period=None, cutoff=math.inf, threshold=1.0):
        self.cap, self.d, self.period, self.cutoff, self.threshold = capacity, d, period, float(cutoff), float(threshold)
        self.centers = torch.zeros(capacity, d, dtype=F64)
        self.sigma = torch.zeros(capacity, d, dtype=F64)
        self.heights = torch.zeros(capacity, dtype=F64)
        self.state = torch.zeros(4, dtype=F64)

    def fill(self, centers, sigma, heights, total):
        """Start from a given table of n rows and its S."""
        n = centers.shape[0]
        self.centers[:n], self.sigma[:n], self.heights[:n] = centers, sigma, heights
        self.state[0], self.state[1] = float(n), float(total)
        return self

    def deposit(self, centers, sigma, heights):
        centers, sigma, heights = centers.contiguous(), sigma.contiguous(), heights.contiguous()
        rc = _capi.lib().molann_selftest_opes_deposit_f64(
            self.centers.data_ptr(), self.sigma.data_ptr(), self.heights.data_ptr(), self.cap, self.d,
            None if self.period is None else self.period.data_ptr(), self.state.data_ptr(), centers.data_ptr(), sigma.data_ptr(),
            heights.data_ptr(), centers.shape[0], self.threshold, self.cutoff)
        assert rc == 0, rc
        return self

    @property
    def n(self):
        return int(self.state[0])

    def counts(self):
        return int(self.state[0]), int(self.state[2]), int(self.state[3])


def brute_force_S(centers, sigma, heights, period, cutoff):
    """S of a table by the torch composition the package already had: `bias.opes_kernel_sum` at the table's own centres."""
    if centers.shape[0] == 0:
        return 0.0
    return float(mbias.opes_kernel_sum(centers, centers, heights, sigma, period, None if math.isinf(cutoff) else cutoff).sum())


def assert_tables_close(n, got, want, label):
    """`got` and `want`: (centers, sigma, heights) of two tables with the same n live rows in the same slots.  Heights and centres
    within 4 ulp of their scale (the largest magnitude in the live table: a centre near 0 is the difference of steps of that size),
    every width within 4 ulp of itself."""
    (gc, gs, gh), (wc, ws, wh) = got, want
    if n == 0:
        return
    c_scale = max(float(wc[:n].abs().max()), float(ws[:n].abs().max()))
    assert float((gc[:n] - wc[:n]).abs().max()) <= 4 * EPS * c_scale, label
    assert float((gh[:n] - wh[:n]).abs().max()) <= 4 * EPS * float(wh[:n].abs().max()), label
    assert bool(((gs[:n] - ws[:n]).abs() <= 4 * EPS * ws[:n].abs()).all()), label


def prefilled_scenario(n0, d, seed=0):
    """A table of n0 well-separated kernels (widths near 0.3; d == 1: a jittered lattice of spacing 1, no period; d > 1: uniform in
    [-1, 1)^d under `mixed_period`) with two planted pairs 0.25 apart - slots (5, n0 - 1) and (7, 9) - and 16 new kernels that meet
    every path: one next to slot 5 (merge, then a chain round into the LAST slot, which fills the hole itself), one next to slot 7
    (merge, a chain round into slot 9, the last kernel fills the hole), one next to slot 20 (a plain merge), 12 fresh ones (appended:
    n0 + 10 live kernels in the end unless a random neighbour in d > 1 joins a chain) and one next to the first of those.  Returns (period, (centers, sigma, heights), new kernels)."""
    g = torch.Generator().manual_seed(7000 + 10 * n0 + d + seed)
    col = 1 if d > 1 else 0                           # a column that is not periodic
    step = torch.zeros(d, dtype=F64)
    step[col] = 1.0
    if d == 1:
        period = None
        centers = torch.arange(n0 + 12, dtype=F64).reshape(-1, 1) + 0.1 * (torch.rand(n0 + 12, 1, dtype=F64, generator=g) - 0.5)
    else:
        period = mixed_period(d)
        centers = 2.0 * torch.rand(n0 + 12, d, dtype=F64, generator=g) - 1.0
    sigma = 0.3 * (0.9 + 0.2 * torch.rand(n0 + 16, d, dtype=F64, generator=g))
    heights = 0.5 + torch.rand(n0 + 16, dtype=F64, generator=g)
    table_c, fresh = centers[:n0].clone(), centers[n0:]
    table_c[n0 - 1] = table_c[5] + 0.25 * step
    table_c[9] = table_c[7] + 0.25 * step
    sigma[n0 - 1], sigma[9] = 0.33, 0.33                  # the takers of the chain rounds: 0.275 / 0.33 widths from the merged kernels
    new_c = torch.cat([(table_c[5] - 0.05 * step)[None], (table_c[7] - 0.05 * step)[None], (table_c[20] + 0.1 * step)[None], fresh,
                       (fresh[0] + 0.1 * step)[None]])
    return period, (table_c, sigma[:n0].clone(), heights[:n0].clone()), (new_c, sigma[n0:].clone(), heights[n0:].clone())


def batches_of(new, width):
    c, s, h = new
    return [(c[i:i + width].contiguous(), s[i:i + width].contiguous(), h[i:i + width].contiguous()) for i in range(0, c.shape[0], width)]


def assert_scenario_paths(ref, n0):
    """The oracle's record of a `prefilled_scenario` run: the two planted chain rounds (the first with its taker in the last slot, which
    then fills the hole itself; the second with the last kernel moved into the hole), 12 appends that carry n past n0, a merge into a
    kernel appended in the same run, nothing refused, and every search clear of the threshold and of its runner-up."""
    assert ("chain", 5, n0 - 1, 5) in ref.history and ("chain", 7, 9, 9) in ref.history, ref.history
    assert ref.seen["hole_fill_taker_last"] >= 1 and ref.seen["hole_fill"] >= 2 and ref.seen["append"] == 12 and ref.refused == 0, ref.seen
    assert ref.history[-1][0] == "merge" and ref.history[-1][1] >= n0 - 3 and ref.n > n0 + 4, (ref.history[-1], ref.n)
    assert min(m[0] for m in ref.margins) >= 1e-9 and min(m[1] for m in ref.margins) >= 1e-9
