"""A sequential float64 restatement of the OPES deposit (`molann_opes_deposit_f64`, include/molann_hip.h) in plain torch on the CPU, written
from the formulas and sharing no code with the library: the reference of tests/test_opes_deposit_f64_host.py and of the GPU file.

    K_j(c) = exp(-q / 2) - c0 where q < c2, else 0;   q = sum_k (wrap(c_k - c_jk) / sigma_jk)^2,   c2 = cutoff^2,   c0 = exp(-c2 / 2)
    wrap(delta, P) = delta - P rint(delta / P) where P > 0
    S = sum_{i<n} sum_{j<n} h_j K_j(c_i)

Besides the table it keeps what a test needs to judge a run: the slot history, A = the sum of the magnitudes of every term added to or
subtracted from S, and per search the two margins that say how far the decision was from going the other way."""

import math

import torch

F64 = torch.float64


def wrap(delta, period):
    """delta - P rint(delta / P) in the columns with P > 0; `period`: [d] (0: not periodic) or None."""
    if period is None:
        return delta
    periodic = period > 0
    safe = torch.where(periodic, period, torch.ones_like(period))
    return torch.where(periodic, delta - safe * torch.round(delta / safe), delta)


def kernel_at(points, center, sigma, period, cutoff):
    """K(points[i]) [M] of ONE kernel (center [d], sigma [d])."""
    s = wrap(points - center, period) / sigma
    q = (s * s).sum(dim=-1)
    c2 = cutoff * cutoff
    c0 = math.exp(-0.5 * c2)
    return torch.where(q < c2, torch.exp(-0.5 * q) - c0, torch.zeros_like(q))


def kernels_at(point, centers, sigma, period, cutoff):
    """K_j(point) [H] of MANY kernels (centers [H, d], sigma [H, d]) at one point [d]."""
    s = wrap(point - centers, period) / sigma
    q = (s * s).sum(dim=-1)
    c2 = cutoff * cutoff
    c0 = math.exp(-0.5 * c2)
    return torch.where(q < c2, torch.exp(-0.5 * q) - c0, torch.zeros_like(q))


def brute_force_sum(centers, sigma, heights, period, cutoff):
    """S of a table from scratch, and the sum of its terms' magnitudes."""
    total, mags = 0.0, 0.0
    for j in range(centers.shape[0]):
        terms = heights[j] * kernel_at(centers, centers[j], sigma[j], period, cutoff)
        total += float(terms.sum())
        mags += float(terms.abs().sum())
    return total, mags


class Oracle(object):
    """The table and its state; `deposit` takes new kernels one after the other."""

    def __init__(self, capacity, d, period=None, cutoff=math.inf, threshold=1.0):
        self.cap, self.d = int(capacity), int(d)
        self.period = None if period is None else torch.as_tensor(period, dtype=F64).reshape(d)
        self.cutoff, self.threshold = float(cutoff), float(threshold)
        self.centers = torch.zeros(self.cap, d, dtype=F64)
        self.sigma = torch.zeros(self.cap, d, dtype=F64)
        self.heights = torch.zeros(self.cap, dtype=F64)
        self.n, self.S, self.merges, self.refused = 0, 0.0, 0, 0
        self.A = 0.0                # sum of |term| over everything that went into S
        self.accepted_height = 0.0  # sum of the heights of the kernels that were not refused
        self.history = []           # ("refused", why) | ("append", slot) | ("merge", taker slot) | ("chain", giver, taker, taker's slot after)
        self.margins = []           # per search with a candidate: (|q_min - thr^2| / thr^2, (q_2nd - q_min) / max(q_min, 1e-300))
        self.seen = {"chain_rounds_max": 0, "hole_fill_taker_last": 0, "hole_fill": 0, "full": 0, "seam": 0, "merge": 0, "append": 0}

    def fill(self, centers, sigma, heights):
        """Start from a given table of n rows: its S from scratch, the magnitudes of its terms into A."""
        n = centers.shape[0]
        self.centers[:n], self.sigma[:n], self.heights[:n] = centers, sigma, heights
        self.n = n
        self.S, self.A = brute_force_sum(self.centers[:n], self.sigma[:n], self.heights[:n], self.period, self.cutoff)
        self.accepted_height = float(self.heights[:n].sum())
        return self

    # ---- S: whole kernels leave and enter
    def _terms(self, c, s, h, skip):
        """Every term kernel e = (c, s, h) shares with the live set without the slots in `skip`, and its own."""
        keep = torch.ones(self.n, dtype=torch.bool)
        for k in skip:
            if k is not None and k >= 0:
                keep[k] = False
        live_c, live_s, live_h = self.centers[:self.n][keep], self.sigma[:self.n][keep], self.heights[:self.n][keep]
        mine = h * kernel_at(live_c, c, s, self.period, self.cutoff)             # h_e K_e(c_i)
        theirs = live_h * kernels_at(c, live_c, live_s, self.period, self.cutoff)  # h_i K_i(c_e)
        own = h * (1.0 - math.exp(-0.5 * self.cutoff * self.cutoff))
        return float(mine.sum()) + float(theirs.sum()) + own, float(mine.abs().sum()) + float(theirs.abs().sum()) + abs(own)

    def _remove(self, c, s, h, skip):
        total, mags = self._terms(c, s, h, skip)
        self.S -= total
        self.A += mags

    def _add(self, c, s, h, skip):
        total, mags = self._terms(c, s, h, skip)
        self.S += total
        self.A += mags

    # ---- the search
    def _nearest(self, c, skip):
        """(q_min, slot) over the live kernels without `skip`, in each kernel's own widths; None where there is none."""
        if self.n == 0 or (self.n == 1 and skip == 0):
            return None
        s = wrap(c - self.centers[:self.n], self.period) / self.sigma[:self.n]
        q = (s * s).sum(dim=1)
        if skip is not None and skip >= 0:
            q[skip] = math.inf
        q_min, slot = float(q.min()), int(torch.argmin(q))
        slot = int(torch.nonzero(q == q_min)[0])     # the smallest slot on a tie
        others = q.clone()
        others[slot] = math.inf
        q_2nd = float(others.min())
        thr2 = self.threshold * self.threshold
        self.margins.append((abs(q_min - thr2) / thr2, (q_2nd - q_min) / max(q_min, 1e-300)))
        return q_min, slot

    def _merge(self, t, c, s, h):
        """The giver (c, s, h) into the taker at slot t; returns the merged kernel (not stored)."""
        ct, st, ht = self.centers[t].clone(), self.sigma[t].clone(), float(self.heights[t])
        hm = ht + h
        raw = c - ct
        delta = wrap(raw, self.period)
        if not torch.equal(raw, delta):
            self.seen["seam"] += 1
        cm = ct + (h / hm) * delta
        var = (ht * (st * st) + h * (s * s)) / hm + (ht * h / (hm * hm)) * (delta * delta)    # sigma^2 and delta^2 are formed first
        # math.sqrt rounds correctly; torch.sqrt on the CPU may be an ulp off, which 190 merges into one kernel would carry along
        return cm, torch.tensor([math.sqrt(v) for v in var.tolist()], dtype=F64), hm

    def deposit(self, centers, sigma, heights):
        centers = torch.as_tensor(centers, dtype=F64).reshape(-1, self.d)
        sigma = torch.as_tensor(sigma, dtype=F64).reshape(-1, self.d)
        heights = torch.as_tensor(heights, dtype=F64).reshape(-1)
        thr2 = self.threshold * self.threshold
        for a in range(centers.shape[0]):
            c, s, h = centers[a].clone(), sigma[a].clone(), float(heights[a])
            if not (bool(torch.isfinite(c).all()) and bool(torch.isfinite(s).all()) and math.isfinite(h) and bool((s > 0).all()) and h > 0):
                self.refused += 1
                self.history.append(("refused", "invalid"))
                continue
            g, rounds = -1, 0          # the giver's slot (-1: the new kernel, not in the table yet)
            while self.threshold > 0:
                found = self._nearest(c, g)
                if found is None or not found[0] < thr2:
                    break
                t = found[1]
                ct, st, ht = self.centers[t].clone(), self.sigma[t].clone(), float(self.heights[t])
                if g >= 0:
                    self._remove(c, s, h, (g,))          # R = live without g: the taker is still in it
                self._remove(ct, st, ht, (t, g))
                c, s, h = self._merge(t, c, s, h)
                self._add(c, s, h, (t, g))
                self.centers[t], self.sigma[t], self.heights[t] = c, s, h
                self.merges += 1
                rounds += 1
                if g < 0:
                    self.history.append(("merge", t))
                else:
                    last = self.n - 1
                    if g != last:
                        self.centers[g], self.sigma[g], self.heights[g] = self.centers[last].clone(), self.sigma[last].clone(), self.heights[last].clone()
                        self.seen["hole_fill"] += 1
                    if t == last:
                        self.seen["hole_fill_taker_last"] += 1
                        t = g
                    self.n -= 1
                    self.history.append(("chain", g, found[1], t))
                g = t
            self.seen["chain_rounds_max"] = max(self.seen["chain_rounds_max"], rounds - 1)
            if g >= 0:
                self.accepted_height += float(heights[a])
                self.seen["merge"] += 1
                continue
            if self.n < self.cap:
                self._add(c, s, h, ())
                self.centers[self.n], self.sigma[self.n], self.heights[self.n] = c, s, h
                self.history.append(("append", self.n))
                self.n += 1
                self.accepted_height += float(heights[a])
                self.seen["append"] += 1
            else:
                self.refused += 1
                self.seen["full"] += 1
                self.history.append(("refused", "full"))
        return self

    def counts(self):
        return self.n, self.merges, self.refused


def random_walk_kernels(generator, n, d, period, step=0.45, sigma0=0.3, start=0.0):
    """n kernels along a random walk of `step` widths per column (scaled by 1 / sqrt(d), so that q between neighbours does not grow
    with d) from `start`: centres wrapped into [-P/2, P/2) in periodic columns, widths sigma0 (0.6 .. 1.4), heights 0.5 .. 1.5."""
    steps = torch.randn(n, d, dtype=F64, generator=generator) * (step * sigma0 / math.sqrt(d))
    walk = torch.cumsum(steps, dim=0) + start
    if period is not None:
        p = torch.as_tensor(period, dtype=F64)
        periodic = p > 0
        safe = torch.where(periodic, p, torch.ones_like(p))
        walk = torch.where(periodic, walk - safe * torch.floor(walk / safe + 0.5), walk)
    sigma = sigma0 * (0.6 + 0.8 * torch.rand(n, d, dtype=F64, generator=generator))
    heights = 0.5 + torch.rand(n, dtype=F64, generator=generator)
    return walk, sigma, heights
