"""A sequential float64 restatement of the OPES step in its two other modes (`molann_opes_step_modes_f64`, include/molann_hip.h: widths
measured from the run, and the explore variant) in plain Python on the CPU, written from the formulas and sharing no code with the
library; the deposit itself is tests/opes_deposit_oracle.py's.  The reference of tests/test_opes_adaptive_f64_host.py.

    1. adaptive:  c = observations + 1,  tau = min(c, stride);  per walker with finite outputs and per column:
       diff = wrap(y - mean),  mean += diff / tau,  M2 += diff wrap(y - mean);  observations = c
    2. `observe`, and a deposit while not started and c < stride, end here
    3. w_a = exp(beta V_a) over the valid walkers into counter, sum_w, sum_w2;  neff = (1 + sum_w)^2 / (1 + sum_w2);
       rct = log(sum_w / counter) / beta;  sigma_scale = 1 (fixed sigma) or (size (d + 2) / 4)^(-1 / (d + 4)), size = neff, or counter
       in the explore variant
    4. not adaptive:  sigma_k = max(sigma0_k sigma_scale, sigma_min_k), the explore variant's sigma0 being sqrt(biasfactor) times the
       one given.   adaptive, factor = biasfactor (1 in the explore variant):  on the first deposit M2 *= biasfactor,
       sigma0_ak = max(sqrt(M2_ak / c / factor), sigma_min_k), started;  s_ak = max(sqrt(M2_ak / c / factor) [sigma_scale], sigma_min_k)
    5. height_a = w_a prod_k (sigma0_ak / s_ak), without w_a in the explore variant; NaN for an invalid walker
    6. the kernels (y[a], s_a, height_a) are deposited in order

Besides the table's margins (every search's distance from the threshold and from its runner-up) it records `floor_margins`: per
comparison of a width with its floor, (whether the floor raised it, |s - sigma_min| / sigma_min)."""

import math

import torch

import opes_deposit_oracle as oracle

F64 = torch.float64


def _exp(v):
    try:
        return math.exp(v)
    except OverflowError:
        return math.inf


def _wrap(v, P):
    return v - P * round(v / P) if P > 0.0 else v       # round(): to the nearest integer, ties to even, as rint


class ModesOracle(object):
    def __init__(self, capacity, d, period, cutoff, threshold, kT, biasfactor, sigma0=None, sigma_min=None, fixed_sigma=False, explore=False,
                 adaptive_stride=None, walkers=None):
        self.table = oracle.Oracle(capacity, d, period, cutoff, threshold)
        self.d, self.beta, self.biasfactor = int(d), 1.0 / kT, float(biasfactor)
        self.period = [0.0] * self.d if period is None else [float(p) for p in period]
        self.adaptive, self.explore, self.fixed_sigma = sigma0 is None, bool(explore), bool(fixed_sigma)
        self.sigma_min = None if sigma_min is None else [float(v) for v in sigma_min]
        if self.adaptive:
            self.stride, self.W = int(adaptive_stride), int(walkers)
            self.mean = [[0.0] * self.d for _ in range(self.W)]
            self.M2 = [[0.0] * self.d for _ in range(self.W)]
            self.sigma0 = [[0.0] * self.d for _ in range(self.W)]
        else:
            grow = math.sqrt(self.biasfactor) if self.explore else 1.0
            self.sigma0 = [float(v) * grow for v in sigma0]
        self.observations, self.started = 0, 0
        self.counter, self.sum_w, self.sum_w2 = 0, 0.0, 0.0
        self.neff, self.sigma_scale, self.rct = 0.0, 0.0, 0.0
        self.invalid, self.skipped = 0, 0
        self.floor_margins = []

    # ---- 1
    def _average(self, y):
        self.observations += 1
        tau = float(min(self.observations, self.stride))
        for a in range(self.W):
            row = [float(v) for v in y[a]]
            if not all(math.isfinite(v) for v in row):
                continue
            for k in range(self.d):
                diff = _wrap(row[k] - self.mean[a][k], self.period[k])
                self.mean[a][k] = self.mean[a][k] + diff / tau
                self.M2[a][k] = self.M2[a][k] + diff * _wrap(row[k] - self.mean[a][k], self.period[k])

    def observe(self, y):
        assert self.adaptive
        self._average(torch.as_tensor(y, dtype=F64).reshape(-1, self.d))
        return self

    def _floor(self, s, k):
        if self.sigma_min is None:
            return s
        m = self.sigma_min[k]
        self.floor_margins.append((s < m, abs(s - m) / m))
        return m if s < m else s

    def deposit(self, y, V):
        """Returns whether anything went to the table (False: a deposit before the first stride had passed)."""
        y = torch.as_tensor(y, dtype=F64).reshape(-1, self.d)
        V = [float(v) for v in torch.as_tensor(V, dtype=F64).reshape(-1)]
        if self.adaptive:
            self._average(y)
            if not self.started and self.observations < self.stride:
                self.skipped += 1
                return False
        # ---- 3
        weights = []
        for a, v in enumerate(V):
            w = _exp(self.beta * v)
            ok = math.isfinite(v) and math.isfinite(w) and w > 0.0 and bool(torch.isfinite(y[a]).all())
            weights.append(w if ok else None)
            if ok:
                self.counter += 1
                self.sum_w += w
                self.sum_w2 += w * w
            else:
                self.invalid += 1
        self.neff = (1.0 + self.sum_w) ** 2 / (1.0 + self.sum_w2)
        self.rct = math.log(self.sum_w / self.counter) / self.beta if self.counter > 0 else 0.0
        d = float(self.d)
        size = float(self.counter) if self.explore else self.neff
        if self.fixed_sigma:
            self.sigma_scale = 1.0
        else:
            self.sigma_scale = (size * (d + 2.0) / 4.0) ** (-1.0 / (d + 4.0)) if size > 0.0 else math.inf
        # ---- 4
        n_walkers = y.shape[0]
        if self.adaptive:
            c = float(self.observations)
            factor = 1.0 if self.explore else self.biasfactor
            if not self.started:
                for a in range(self.W):
                    for k in range(self.d):
                        self.M2[a][k] = self.M2[a][k] * self.biasfactor
                        self.sigma0[a][k] = self._floor(math.sqrt(self.M2[a][k] / c / factor), k)
                self.started = 1
            sigma = []
            for a in range(n_walkers):
                row = []
                for k in range(self.d):
                    s = math.sqrt(self.M2[a][k] / c / factor)
                    if not self.fixed_sigma:
                        s = s * self.sigma_scale
                    row.append(self._floor(s, k))
                sigma.append(row)
            sigma0 = self.sigma0
        else:
            row = [self._floor(s0 * self.sigma_scale, k) for k, s0 in enumerate(self.sigma0)]
            sigma = [row] * n_walkers
            sigma0 = [self.sigma0] * n_walkers
        # ---- 5
        heights = []
        for a in range(n_walkers):
            ratio = 1.0
            for k in range(self.d):
                ratio = ratio * (sigma0[a][k] / sigma[a][k]) if sigma[a][k] != 0.0 else math.nan
            heights.append(math.nan if weights[a] is None else (ratio if self.explore else weights[a] * ratio))
        self.last_sigma, self.last_heights = torch.tensor(sigma, dtype=F64), torch.tensor(heights, dtype=F64)
        # ---- 6
        self.table.deposit(y, self.last_sigma, self.last_heights)
        return True

    def run_values(self):
        return (self.counter, self.sum_w, self.sum_w2, self.neff, self.sigma_scale, self.rct, self.observations, self.started)

    def adapt_rows(self):
        """(mean, M2, sigma0) as [W, d] tensors."""
        return tuple(torch.tensor(v, dtype=F64) for v in (self.mean, self.M2, self.sigma0))
