"""What the tests of the OPES step's modes share (tests/test_opes_adaptive_f64_host.py and tests/test_gpu_opes_adaptive_f64.py): the
call sequence, the walkers' outputs, the host twin `molann_selftest_opes_step_modes_f64` on torch CPU tensors and the comparison of two
runs.

Bounds are tests/opes_run_cases.py's, derived there: counts, slots, run[0], run[6] and run[7] equal; everything else within
1e-12 max(1, |value|), centres and means within 1e-12 max(|value|, sigma).  The averages' recursion adds at most one rounding of 1.1e-16
per observation to a mean - its coefficient 1 - 1 / tau does not amplify - and to M2, a sum of non-negative terms (diff and the wrapped
y - mean have the same sign: the second is (1 - 1 / tau) diff up to rounding); the 64 observations of a sequence stay a hundred times
inside the bound.

The sequence (adaptive_stride = 4): observe, observe, deposit (skipped: 3 < 4), deposit (the first), then 30 times observe, deposit.
Walker a's outputs follow a seeded random walk that starts at 0.6 + 0.05 a in every column and drifts upwards in column 0, which is
periodic with period 2 (`opes_deposit_cases.mixed_period`): y and the windowed mean cross the seam at 1 = -1 at different calls.  The
last walker has a NaN output at the deposit PLANT_NAN and an infinite bias at the deposit PLANT_INF.  V is the host twin's bias
(`molann_selftest_opes_table_f64`) on the run's own table, with the explore scalars in the explore variant."""

import math

import torch

from molann_amd import _capi

import opes_deposit_cases as cases
import opes_run_cases as rc

F64 = torch.float64
STRIDE, CAP, CUTOFF, THRESHOLD = 4, 64, 5.0, 1.0
SEQUENCE = ["observe", "observe", "deposit", "deposit"] + ["observe", "deposit"] * 30
PLANT_NAN, PLANT_INF = 21, 31          # indices into SEQUENCE: both deposits
SCALE_X = rc.KT * (rc.BIASFACTOR - 1.0)                 # the explore variant's scale and epsilon
EPSILON_X = math.exp(-rc.BARRIER / SCALE_X)
FIXED, EXPLORE, OBSERVE = 1, 2, 4
SIGMA0_GIVEN = 0.12                    # the numeric sigma0 of the explore case, near the walk's spread over a window


def walk(d, walkers, seed):
    """y [len(SEQUENCE), walkers, d]."""
    g = torch.Generator().manual_seed(seed)
    steps = 0.08 * torch.randn(len(SEQUENCE), walkers, d, dtype=F64, generator=g)
    steps[:, :, 0] += 0.03
    y = torch.cumsum(steps, dim=0) + 0.6 + 0.05 * torch.arange(walkers, dtype=F64)[None, :, None]
    period = cases.mixed_period(d)
    periodic = period > 0
    safe = torch.where(periodic, period, torch.ones_like(period))
    return torch.where(periodic, y - safe * torch.floor(y / safe + 0.5), y), period


class HostModes(object):
    """A run in host memory under `molann_selftest_opes_step_modes_f64`; `sigma0` None: adaptive.  With `columns` the walkers' outputs
    sit in those columns of a wider y."""

    def __init__(self, d, period, sigma0=None, sigma_min=None, fixed_sigma=False, explore=False, walkers=None, stride=STRIDE, capacity=CAP,
                 cutoff=CUTOFF, threshold=THRESHOLD, biasfactor=rc.BIASFACTOR, columns=None):
        self.table = cases.HostTable(capacity, d, period, cutoff, threshold)
        self.d, self.stride, self.biasfactor = d, stride, biasfactor
        self.sigma0 = None if sigma0 is None else sigma0.clone()
        self.sigma_min = None if sigma_min is None else sigma_min.clone()
        self.flags = (FIXED if fixed_sigma else 0) | (EXPLORE if explore else 0)
        self.explore = explore
        self.run = torch.zeros(8, dtype=F64)
        self.adapt = torch.zeros(walkers, 3, d, dtype=F64) if sigma0 is None else None
        self.columns = None if columns is None else _capi._i32_array(columns)

    def bias(self, y):
        """V [W] of `molann_selftest_opes_table_f64` on the table's current state at y [W, d]."""
        t, L = self.table, _capi.lib()
        scale, epsilon = (SCALE_X, EPSILON_X) if self.explore else (rc.SCALE, rc.EPSILON)
        y = y.contiguous()
        v, dy = torch.empty(y.shape[0], dtype=F64), torch.empty(self.d, dtype=F64)
        for a in range(y.shape[0]):
            v[a] = L.molann_selftest_opes_table_f64(y[a].data_ptr(), self.d, t.centers.data_ptr(), t.heights.data_ptr(), t.sigma.data_ptr(), t.cap,
                                                    t.state.data_ptr(), None if t.period is None else t.period.data_ptr(), scale, epsilon, t.cutoff,
                                                    dy.data_ptr())
        return v

    def call(self, y, V=None, observe=False):
        t = self.table
        y = y.contiguous()
        V = y if V is None else V
        rcode = _capi.lib().molann_selftest_opes_step_modes_f64(
            t.centers.data_ptr(), t.sigma.data_ptr(), t.heights.data_ptr(), t.cap, self.d, None if t.period is None else t.period.data_ptr(),
            t.state.data_ptr(), self.run.data_ptr(), y.data_ptr(), y.shape[1], self.columns, V.data_ptr(), V.stride(0) if V.dim() else 1, y.shape[0],
            None if self.sigma0 is None else self.sigma0.data_ptr(), None if self.sigma_min is None else self.sigma_min.data_ptr(),
            None if self.adapt is None else self.adapt.data_ptr(), rc.BETA, self.biasfactor, self.stride, t.threshold, t.cutoff,
            self.flags | (OBSERVE if observe else 0))
        assert rcode == 0, rcode
        return self

    def snapshot(self):
        t = self.table
        return tuple(v.clone() for v in (t.centers, t.sigma, t.heights, t.state, self.run)) + ((self.adapt.clone(),) if self.adapt is not None else ())


def play(host, y, others=(), upto=None):
    """The sequence (its first `upto` calls) on `host` (V from its own table, the planted values put in), and on every run of `others` - anything with
    `observe(y)` and `deposit(y, V)` - with the same y and V.  Returns the calls as (kind, y_i, V_i or None) and, per call, a snapshot of
    `host` after it."""
    calls, shots = [], []
    last = y.shape[1] - 1
    for i, kind in enumerate(SEQUENCE[:upto]):
        yi = y[i].clone()
        if kind == "observe":
            host.call(yi, observe=True)
            for o in others:
                o.observe(yi)
            calls.append((kind, yi, None))
        else:
            V = host.bias(yi)
            if i == PLANT_NAN:
                yi[last, host.d - 1] = math.nan
            if i == PLANT_INF:
                V[last] = math.inf
            host.call(yi, V)
            for o in others:
                o.deposit(yi, V)
            calls.append((kind, yi, V))
        shots.append(host.snapshot())
    return calls, shots


def compare_adapt(got, want, observations):
    """The worst error over its bound of two [W, 3, d] states: means within 1e-12 max(|mean|, sqrt(M2 / observations)), M2 and sigma0
    within 1e-12 max(1, |value|)."""
    one = torch.ones((), dtype=F64)
    spread = torch.sqrt(want[:, 1] / max(observations, 1))
    worst = float(((got[:, 0] - want[:, 0]).abs() / (rc.BOUND * torch.maximum(want[:, 0].abs(), torch.clamp(spread, min=1e-300)))).max())
    for j in (1, 2):
        worst = max(worst, float(((got[:, j] - want[:, j]).abs() / (rc.BOUND * torch.maximum(one, want[:, j].abs()))).max()))
    return worst


def assert_same_modes_run(got, want, label):
    """`got`, `want`: snapshots (centers, sigma, heights, state, run[, adapt]).  Counts, slots, run[0], run[6], run[7] equal, everything
    else within the module's bounds.  Returns the worst ratio."""
    gs, ws = got[3], want[3]
    assert (int(gs[0]), int(gs[2]), int(gs[3])) == (int(ws[0]), int(ws[2]), int(ws[3])), (label, gs.tolist(), ws.tolist())
    n = int(ws[0])
    worst = max(rc.compare_tables(n, got[:3], want[:3]), rc.compare_scalars(got[4], want[4]))
    worst = max(worst, abs(float(gs[1]) - float(ws[1])) / (rc.BOUND * max(1.0, abs(float(ws[1])))))
    assert float(got[4][6]) == float(want[4][6]) and float(got[4][7]) == float(want[4][7]), (label, got[4].tolist(), want[4].tolist())
    if len(want) > 5:
        worst = max(worst, compare_adapt(got[5], want[5], int(want[4][6])))
    assert worst <= 1.0, (label, worst)
    return worst
