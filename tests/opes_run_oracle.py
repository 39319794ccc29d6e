"""A sequential float64 restatement of a whole OPES step (`molann_opes_step_f64`, include/molann_hip.h) and of the bias read from a
table's state (`molann_value_and_opes_table_f64`) in plain Python and torch on the CPU, written from the formulas and sharing no code
with the library; the deposit itself is tests/opes_deposit_oracle.py's.  The reference of tests/test_opes_run_f64_host.py.

    w_a = exp(beta V_a); valid: V_a, w_a and every y[a, k] finite, w_a > 0; over the valid walkers counter += 1, sum_w += w_a,
    sum_w2 += w_a^2;   neff = (1 + sum_w)^2 / (1 + sum_w2);   rct = log(sum_w / counter) / beta (0 while counter == 0)
    sigma_scale = 1 (fixed sigma) or (neff (d + 2) / 4)^(-1 / (d + 4));   sigma_k = max(sigma0_k sigma_scale, sigma_min_k)
    height_a = w_a prod_k (sigma0_k / sigma_k), NaN for an invalid walker;   the kernels (y[a], sigma, height_a) are deposited in order
    bias: V(y) = scale log(P(y) / norm + epsilon), P = sum_{h<n} heights_h K_h(y), norm = S / n;  n == 0: V = scale log(epsilon)

The table's oracle records the decision margins of every search; this one adds the steps in which sigma_min held a width up."""

import math

import torch

import opes_deposit_oracle as oracle

F64 = torch.float64


def _exp(v):
    try:
        return math.exp(v)
    except OverflowError:
        return math.inf


class RunOracle(object):
    def __init__(self, capacity, d, period, cutoff, threshold, kT, biasfactor, barrier, sigma0, sigma_min=None, fixed_sigma=False):
        self.table = oracle.Oracle(capacity, d, period, cutoff, threshold)
        self.d = int(d)
        self.beta = 1.0 / kT
        self.scale = kT * (1.0 - 1.0 / biasfactor)
        self.epsilon = math.exp(-barrier / self.scale)
        self.sigma0 = [float(v) for v in sigma0]
        self.sigma_min = None if sigma_min is None else [float(v) for v in sigma_min]
        self.fixed_sigma = bool(fixed_sigma)
        self.counter, self.sum_w, self.sum_w2 = 0, 0.0, 0.0
        self.neff, self.sigma_scale, self.rct = 0.0, 0.0, 0.0
        self.bound_steps = 0        # steps in which sigma_min raised a width
        self.invalid = 0

    def bias(self, y, norm=None):
        """(V [W], dV/dy [W, d]) under the table as it is; `norm`: S / n of this table, or another run's value of it."""
        t = self.table
        y = torch.as_tensor(y, dtype=F64).reshape(-1, self.d)
        if t.n == 0:
            return torch.full((y.shape[0],), self.scale * math.log(self.epsilon), dtype=F64), torch.zeros_like(y)
        norm = t.S / t.n if norm is None else norm
        yy = y.clone().requires_grad_(True)
        with torch.enable_grad():
            p = torch.stack([(t.heights[:t.n] * oracle.kernels_at(yy[a], t.centers[:t.n], t.sigma[:t.n], t.period, t.cutoff)).sum()
                             for a in range(y.shape[0])])
            v = self.scale * torch.log(p / norm + self.epsilon)
            (g,) = torch.autograd.grad(v.sum(), yy)
        return v.detach(), g

    def step(self, y, V):
        y = torch.as_tensor(y, dtype=F64).reshape(-1, self.d)
        V = [float(v) for v in torch.as_tensor(V, dtype=F64).reshape(-1)]
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
        self.sigma_scale = 1.0 if self.fixed_sigma else (self.neff * (d + 2.0) / 4.0) ** (-1.0 / (d + 4.0))
        sigma = [s0 * self.sigma_scale for s0 in self.sigma0]
        if self.sigma_min is not None:
            if any(m > s for m, s in zip(self.sigma_min, sigma)):
                self.bound_steps += 1
            sigma = [max(m, s) for m, s in zip(self.sigma_min, sigma)]
        ratio = 1.0
        for s0, s in zip(self.sigma0, sigma):
            ratio *= s0 / s
        heights = torch.tensor([math.nan if w is None else w * ratio for w in weights], dtype=F64)
        self.last_sigma, self.last_heights = torch.tensor(sigma, dtype=F64), heights
        self.table.deposit(y, torch.tensor(sigma, dtype=F64).expand(y.shape[0], self.d), heights)
        return self

    def run_values(self):
        return (self.counter, self.sum_w, self.sum_w2, self.neff, self.sigma_scale, self.rct)
