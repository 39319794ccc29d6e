"""What the OPES run tests share (tests/test_opes_run_f64_host.py and tests/test_gpu_opes_run_f64.py): the run's parameters, the host
twins `molann_selftest_opes_table_f64` and `molann_selftest_opes_step_f64` on torch CPU tensors, and the comparison of two runs.

Bounds.  Counts and slots are equal and `counter` is exact.  Rows, heights and the scalars sum_w, sum_w2, neff, sigma_scale, rct: within
1e-12 max(1, |value|); centres within 1e-12 max(|c|, sigma).  A new kernel is about 30 roundings of 1.1e-16 away from the formula
(`exp`, `pow`, d divisions and products) and a merge is a positive-weight average of two kernels, which does not amplify a relative
error; 200 steps of sums of positive weights add at most 200 x 1.1e-16 to sum_w and sum_w2.  S: within 1e-12 max(1, A) of the brute
force on the final table, A being the sum of the magnitudes of every term that went into it (tests/opes_deposit_cases.py)."""

import math

import torch

from molann_amd import _capi

import opes_deposit_cases as cases

F64 = torch.float64
INF = math.inf
KT, BIASFACTOR, BARRIER = 1.0, 10.0, 20.0
BETA = 1.0 / KT
SCALE = KT * (1.0 - 1.0 / BIASFACTOR)
EPSILON = math.exp(-BARRIER / SCALE)
BOUND = 1e-12


def sigma0_row(d):
    """Widths near the deposit cases' 0.3, another one per column."""
    return torch.tensor([0.3 + 0.01 * k for k in range(d)], dtype=F64)


def sigma_min_row(d, samples):
    """Floors that the rescaled widths reach once neff passes a tenth of the run's samples (neff stays well below the number of
    samples: the weights grow with the bias): they bind in late steps and not early, and in some runs never."""
    return sigma0_row(d) * (0.1 * samples * (d + 2.0) / 4.0) ** (-1.0 / (d + 4.0))


class HostRun(object):
    """A run in host memory under the two host twins."""

    def __init__(self, capacity, d, period=None, cutoff=INF, threshold=1.0, sigma0=None, sigma_min=None, fixed_sigma=False):
        self.table = cases.HostTable(capacity, d, period, cutoff, threshold)
        self.d = d
        self.sigma0 = sigma0_row(d) if sigma0 is None else sigma0.clone()
        self.sigma_min = None if sigma_min is None else sigma_min.clone()
        self.fixed_sigma = fixed_sigma
        self.run = torch.zeros(8, dtype=F64)

    def bias(self, y, scale=SCALE, epsilon=EPSILON):
        """(V [W], dV/dy [W, d]) of `molann_selftest_opes_table_f64` on the table's current state."""
        t, L = self.table, _capi.lib()
        y = y.contiguous()
        v, dy = torch.empty(y.shape[0], dtype=F64), torch.empty(y.shape[0], self.d, dtype=F64)
        for a in range(y.shape[0]):
            v[a] = L.molann_selftest_opes_table_f64(y[a].data_ptr(), self.d, t.centers.data_ptr(), t.heights.data_ptr(), t.sigma.data_ptr(), t.cap,
                                                    t.state.data_ptr(), None if t.period is None else t.period.data_ptr(), scale, epsilon, t.cutoff,
                                                    dy[a].data_ptr())
        return v, dy

    def step(self, y, V):
        t = self.table
        y, V = y.contiguous(), V.contiguous()
        rc = _capi.lib().molann_selftest_opes_step_f64(
            t.centers.data_ptr(), t.sigma.data_ptr(), t.heights.data_ptr(), t.cap, self.d, None if t.period is None else t.period.data_ptr(),
            t.state.data_ptr(), self.run.data_ptr(), y.data_ptr(), V.data_ptr(), y.shape[0], self.sigma0.data_ptr(),
            None if self.sigma_min is None else self.sigma_min.data_ptr(), BETA, t.threshold, t.cutoff, 1 if self.fixed_sigma else 0)
        assert rc == 0, rc
        return self

    def snapshot(self):
        t = self.table
        return tuple(v.clone() for v in (t.centers, t.sigma, t.heights, t.state, self.run))


RUN0 = (50.0, 20.0, 12.0)       # the sums a step scenario starts from: neff = 21^2 / 13


def step_scenario(n0, d):
    """The deposit cases' prefilled scenario as steps of a run: its 16 new kernels' centres are the walkers' outputs y (planted merges,
    the two chain rounds, 12 appends), V in [-3, 0), the run `RUN0` steps old, so that the widths are rescaled (0.52 sigma0 at d = 1,
    0.69 at d = 8) and a floor of 0.22 holds up every width at d = 1 and the narrower ones at d = 8.  Returns (period, (centers, sigma,
    heights), y [16, d], V [16], sigma0 [d], sigma_min [d])."""
    period, table, new = cases.prefilled_scenario(n0, d)
    g = torch.Generator().manual_seed(9100 + n0 + d)
    V = -3.0 * torch.rand(new[0].shape[0], dtype=F64, generator=g)
    return period, table, new[0].contiguous(), V, torch.tensor([0.3 + 0.012 * k for k in range(d)], dtype=F64), torch.full((d,), 0.22, dtype=F64)


def host_scenario_run(n0, d, width, capacity=600, cutoff=5.0, threshold=1.0):
    """The host twins' run of `step_scenario` in steps of `width` walkers: (HostRun, the scenario)."""
    sc = step_scenario(n0, d)
    period, table, y, V, sigma0, sigma_min = sc
    host = HostRun(capacity, d, period, cutoff, threshold, sigma0, sigma_min, False)
    host.table.fill(*table, cases.brute_force_S(*table, period, cutoff))
    host.run[:3] = torch.tensor(RUN0, dtype=F64)
    for i in range(0, y.shape[0], width):
        host.step(y[i:i + width], V[i:i + width])
    return host, sc


def compare_tables(n, got, want):
    """The worst error over its bound of the live rows of two tables (centers, sigma, heights) with the same slots; 0 for n == 0."""
    (gc, gs, gh), (wc, ws, wh) = got, want
    if n == 0:
        return 0.0
    one = torch.ones((), dtype=F64)
    worst = float(((gc[:n] - wc[:n]).abs() / (BOUND * torch.maximum(wc[:n].abs(), ws[:n]))).max())
    worst = max(worst, float(((gs[:n] - ws[:n]).abs() / (BOUND * torch.maximum(one, ws[:n].abs()))).max()))
    return max(worst, float(((gh[:n] - wh[:n]).abs() / (BOUND * torch.maximum(one, wh[:n].abs()))).max()))


def compare_scalars(got, want):
    """The worst error over its bound of (sum_w, sum_w2, neff, sigma_scale, rct); `counter` must be equal."""
    assert int(got[0]) == int(want[0]), (got[0], want[0])
    return max(abs(float(g) - float(w)) / (BOUND * max(1.0, abs(float(w)))) for g, w in zip(list(got)[1:6], list(want)[1:6]))


def assert_same_run(got, want, label):
    """`got`, `want`: (centers, sigma, heights, state, run) of two runs, CPU tensors.  Counts equal, everything else within the module's
    bounds (S against `want`'s within 1e-12 max(1, |S|): the caller holds it against the brute force and A where it has them).  Returns
    (worst ratio, whether every value has the same bits)."""
    gs, ws = got[3], want[3]
    assert (int(gs[0]), int(gs[2]), int(gs[3])) == (int(ws[0]), int(ws[2]), int(ws[3])), (label, gs.tolist(), ws.tolist())
    n = int(ws[0])
    worst = max(compare_tables(n, got[:3], want[:3]), compare_scalars(got[4], want[4]))
    worst = max(worst, abs(float(gs[1]) - float(ws[1])) / (BOUND * max(1.0, abs(float(ws[1])))))
    assert worst <= 1.0, (label, worst)
    assert float(got[4][6]) == 0.0 and float(got[4][7]) == 0.0, label
    bits = all(torch.equal(g[:n], w[:n]) for g, w in zip(got[:3], want[:3])) and torch.equal(gs, ws) and torch.equal(got[4], want[4])
    return worst, bits
