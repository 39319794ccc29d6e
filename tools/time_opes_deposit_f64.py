#!/usr/bin/env python3
"""The deposit step of an OPES run and the kernel density at arbitrary points, per call, in the same process, alternating:

    deposit    OpesTable.deposit of ONE kernel (molann_opes_deposit_f64: one launch of one block, nothing read back) into a table of
               100, 1000 and 10000 kernels: the APPEND case (the new kernel is far from every live one: a search, one walk for S, a row
               stored) and the MERGE case (it lands next to a live kernel: a search, two walks, a row stored, the search of the chain)
    torch      the same step in torch ops on the same tensors, with the read-backs its branches need: `torch_deposit` below
    kernel_sum OpesTable.kernel_sum (molann_opes_kernel_sum_f64) at M = H = 1000 and M = 65536, H = 1000
    composed   molann_amd.bias.opes_kernel_sum on the same tensors under no_grad

Times are HIP events around one call, the median of 20 calls after 5 warm-up calls, so they hold the launch and whatever the host
cannot hide behind the device; the median of the rounds' medians is printed.  The table is put back as it was before every call, outside
the events.

    python tools/time_opes_deposit_f64.py                  # d = 2 and 8
    python tools/time_opes_deposit_f64.py --d 2 --kernels 1000
"""
import argparse
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from molann_amd import bias as mb  # noqa: E402

CUTOFF, THRESHOLD = 5.0, 1.0


def timed(fn, setup, calls=20, warmup=5):
    """the median of `calls` calls after `warmup`, each between two HIP events and after `setup()`, in microseconds"""
    for _ in range(warmup):
        setup()
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(calls):
        setup()
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop) * 1e3)
    return statistics.median(times)


def kernel_values(points, center, sigma):
    """K(points[i]) of one kernel, no period"""
    s = (points - center) / sigma
    q = (s * s).sum(dim=-1)
    return torch.where(q < CUTOFF * CUTOFF, torch.exp(-0.5 * q) - math.exp(-0.5 * CUTOFF * CUTOFF), torch.zeros_like(q))


def pair_terms(centers, sigma, heights, c, s, h, keep):
    """sum over the kept live kernels of h K(c_i) + h_i K_i(c), and the kernel's own term"""
    mine = h * kernel_values(centers, c, s)
    sq = (c - centers) / sigma
    q = (sq * sq).sum(dim=-1)
    theirs = heights * torch.where(q < CUTOFF * CUTOFF, torch.exp(-0.5 * q) - math.exp(-0.5 * CUTOFF * CUTOFF), torch.zeros_like(q))
    return ((mine + theirs) * keep).sum() + h * (1.0 - math.exp(-0.5 * CUTOFF * CUTOFF))


def torch_deposit(table, n, c, s, h):
    """One kernel (c [d], s [d], h a 0-dim tensor) into `table` (an OpesTable used as plain buffers) holding n live kernels, the way a
    caller writes it with torch ops: the nearest kernel and the decision need a read-back, so does the chain's search.  Returns n."""
    centers, sigma, heights = table.centers[:n], table.sigma[:n], table.heights[:n]
    sq = (c - centers) / sigma
    q_min, t = (sq * sq).sum(dim=1).min(dim=0)
    q_min, t = float(q_min), int(t)                          # read-back: merge or append, and where
    everyone = torch.ones(n, dtype=torch.float64, device=c.device)
    if q_min < THRESHOLD * THRESHOLD:
        keep = everyone.clone()
        keep[t] = 0.0
        ct, st, ht = centers[t].clone(), sigma[t].clone(), heights[t].clone()
        total = table.state[1] - pair_terms(centers, sigma, heights, ct, st, ht, keep)
        hm = ht + h
        delta = c - ct
        cm = ct + (h / hm) * delta
        sm = torch.sqrt((ht * st * st + h * s * s) / hm + (ht * h / (hm * hm)) * delta * delta)
        table.state[1] = total + pair_terms(centers, sigma, heights, cm, sm, hm, keep)
        centers[t], sigma[t], heights[t] = cm, sm, hm
        sq = (cm - centers) / sigma
        q2 = (sq * sq).sum(dim=1)
        q2[t] = math.inf
        if float(q2.min()) < THRESHOLD * THRESHOLD:          # read-back: does the chain go on (it does not, in this script's tables)
            raise RuntimeError("the timed tables have no chains")
        return n
    table.state[1] = table.state[1] + pair_terms(centers, sigma, heights, c, s, h, everyone)
    table.centers[n], table.sigma[n], table.heights[n] = c, s, h
    return n + 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=0, help="one width instead of 2 and 8")
    ap.add_argument("--kernels", type=int, default=0, help="one table size instead of 100, 1000, 10000")
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    f64 = dict(dtype=torch.float64, device=dev)
    for d in ([args.d] if args.d else [2, 8]):
        for n in ([args.kernels] if args.kernels else [100, 1000, 10000]):
            g = torch.Generator().manual_seed(5)
            # kernels of width 0.3 with no two within the threshold: uniform in a box of side 4 (d = 8: the nearest neighbour is about 3.5
            # widths away at 10000 kernels), a jittered lattice of spacing 1.2 in low dimension
            side = 4.0
            centers = (side * torch.rand(n, d, generator=g, dtype=torch.float64)).to(dev)
            if d <= 2:
                per = int(math.ceil(n ** (1.0 / d)))
                grid = torch.stack(torch.meshgrid(*([torch.arange(per, dtype=torch.float64)] * d), indexing="ij"), dim=-1).reshape(-1, d)[:n]
                centers = (1.2 * grid + 0.1 * torch.rand(n, d, generator=g, dtype=torch.float64)).to(dev)
            table = mb.OpesTable(n + 8, d, dev, cutoff=CUTOFF, threshold=THRESHOLD)
            table.centers[:n], table.sigma[:n], table.heights[:n] = centers, 0.3, 1.0
            table.state[0] = float(n)
            table.recompute_sum(n=n)
            state0, row3 = table.state.clone(), (table.centers[3].clone(), table.sigma[3].clone(), table.heights[3].clone())
            far = (centers.max(dim=0).values + 3.0).reshape(1, d).contiguous()
            near = (centers[3] + 0.05).reshape(1, d).contiguous()
            width, height = torch.full((1, d), 0.3, **f64), torch.ones(1, **f64)

            def restore():
                table.state.copy_(state0)
                table.centers[3], table.sigma[3], table.heights[3] = row3

            results = {}
            with torch.cuda.device(dev):
                for case, c in (("append", far), ("merge", near)):
                    restore()
                    table.deposit(c, width, height)
                    got = table.read_state()
                    restore()
                    n_after = torch_deposit(table, n, c[0], width[0], height[0])
                    torch.cuda.synchronize()
                    assert (got[0], got[2]) == ((n + 1, 0) if case == "append" else (n, 1)) and n_after == got[0], (case, got, n_after)
                    agree = abs(got[1] - float(table.state[1])) / max(1.0, abs(got[1]))
                    t = {"deposit": [], "torch": []}
                    for _ in range(args.rounds):
                        t["deposit"].append(timed(lambda: table.deposit(c, width, height), restore))
                        t["torch"].append(timed(lambda: torch_deposit(table, n, c[0], width[0], height[0]), restore))
                    results[case] = (statistics.median(t["deposit"]), statistics.median(t["torch"]), agree)
            print("d %d, %d kernels: %s" % (d, n, ";  ".join("%s: deposit %.1f us, torch %.1f us (%.1fx), S agrees to %.1e" % (k, a, b, b / a, e)
                                                             for k, (a, b, e) in results.items())), flush=True)
        # the density at arbitrary points, on the last table's first 1000 kernels
        for m in (1000, 65536):
            h = min(1000, n)
            points = (float(centers[:h].max()) * torch.rand(m, d, generator=torch.Generator().manual_seed(9), dtype=torch.float64)).to(dev)
            with torch.cuda.device(dev), torch.no_grad():
                new = table.kernel_sum(points, n=h)
                old = mb.opes_kernel_sum(points, table.centers[:h], table.heights[:h], table.sigma[:h], None, CUTOFF)
                torch.cuda.synchronize()
                agree = float((new - old).abs().max()) / max(1.0, float(old.abs().max()))
                t = {"kernel_sum": [], "grad": [], "composed": []}
                for _ in range(args.rounds):
                    t["kernel_sum"].append(timed(lambda: table.kernel_sum(points, n=h), lambda: None))
                    t["grad"].append(timed(lambda: table.kernel_sum(points, with_grad=True, n=h), lambda: None))
                    t["composed"].append(timed(lambda: mb.opes_kernel_sum(points, table.centers[:h], table.heights[:h], table.sigma[:h], None, CUTOFF),
                                               lambda: None))
            med = dict((k, statistics.median(v)) for k, v in t.items())
            print("d %d, kernel_sum M = %d, H = %d: kernel_sum %.1f us, with dP %.1f us, bias.opes_kernel_sum %.1f us (%.1fx), agree to %.1e"
                  % (d, m, h, med["kernel_sum"], med["grad"], med["composed"], med["composed"] / med["kernel_sum"], agree), flush=True)


if __name__ == "__main__":
    main()
