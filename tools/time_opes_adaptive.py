#!/usr/bin/env python3
"""One whole OPES step with adaptive widths - the bias and forces of W walkers, their running averages, then the deposit of their W
kernels with per-walker widths - on C3's preprocessing behind a [d_feat, 32, 2] tanh head ("C3-head2"), per step, in the same process,
alternating:

    (f) fixed      `OpesRun` with a numeric sigma0, the step this one extends: `bias` then `deposit` (molann_opes_step_f64), eager,
                   and the pair replayed from a graph
    (a) read-back  the route a user had for adaptive widths: `OpesTable.read_state()` (a blocking 32-byte read-back), `table.record`,
                   `value_and_opes`, then the averages, the weights, neff, the per-walker widths and the heights with torch on the
                   device, `OpesTable.deposit`
    (b) eager      `OpesRun(sigma0="adaptive").bias` then `.deposit` (molann_opes_step_modes_f64): two launches, nothing read back
    (c) graph      the pair of (b) captured once in a torch.cuda.graph and replayed
    (x) explore    (b) with `explore=True`
    (o) observe    `OpesRun.observe` alone: the launch an MD step between two deposits adds

at 1 and 64 walkers on tables of 100 and 1000 kernels (tools/time_opes_run.py's: a jittered lattice over the model's outputs,
neighbours 1.5 widths apart).  The adaptive runs are 200 observations old and past their first deposit, each walker's mean at its own
output and its M2 such that its width is the fixed run's sigma0, so (f), (a), (b) and (c) deposit the same kernels up to the step's own
observation.  Times are HIP events around one step, the median of 20 steps after 5 warm-up steps; the median of the rounds' medians
is printed.  The table, its state, the run's sums and the averages are put back before every step, outside the events.  (a), (b) and
(c) leave the same counts and, to rounding, the same S: asserted before anything is timed.

    python tools/time_opes_adaptive.py
    python tools/time_opes_adaptive.py --walkers 64 --kernels 1000
"""
import argparse
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from molann_amd import bias as mb, workloads as wl  # noqa: E402
from molann_amd.ann import MolANN, create_sequential_nn  # noqa: E402

CUTOFF, THRESHOLD = 5.0, 1.0
KT, BIASFACTOR, BARRIER = 1.0, 10.0, 20.0
STRIDE, OBSERVATIONS = 10, 200.0


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


def graphed(dev, fn, restore):
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        restore()
        fn()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    restore()
    with torch.cuda.graph(graph):
        fn()
    return graph


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=0, help="one number of walkers instead of 1 and 64")
    ap.add_argument("--kernels", type=int, default=0, help="one table size instead of 100 and 1000")
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    f64 = dict(dtype=torch.float64, device=dev)
    w = wl.get_workload("C3")
    model = wl.build_model(w, dev)
    torch.manual_seed(11)
    model = MolANN(model.preprocessing_layer, create_sequential_nn([w.feature_dim(), 32, 2], activation=torch.nn.Tanh())).to(dev)
    model = model.double().requires_grad_(False)
    d = 2
    with torch.no_grad():
        visited = model(w.make_frames(4096, seed=3, device=dev).double())
    lo, hi = visited.min(dim=0).values, visited.max(dim=0).values
    for n in ([args.kernels] if args.kernels else [100, 1000]):
        per = int(math.ceil(math.sqrt(n)))
        g = torch.Generator().manual_seed(5)
        grid = torch.stack(torch.meshgrid(torch.arange(per, dtype=torch.float64), torch.arange(per, dtype=torch.float64), indexing="ij"), dim=-1)
        grid = (grid.reshape(-1, 2)[:n] + 0.1 * torch.rand(n, 2, generator=g, dtype=torch.float64)).to(dev)
        spacing = (hi - lo) / per
        sigma0 = (spacing / 1.5).contiguous()
        sigma_min = 0.5 * sigma0
        table = mb.OpesTable(n + 128, d, dev, cutoff=CUTOFF, threshold=THRESHOLD)
        table.centers[:n], table.sigma[:n], table.heights[:n] = lo + grid * spacing, sigma0, 1.0
        table.state[0] = float(n)
        table.recompute_sum(n=n)
        sums = torch.tensor([200.0, 60.0, 30.0], **f64)               # a run that is 200 samples old: neff = 61^2 / 31
        for n_walkers in ([args.walkers] if args.walkers else [1, 64]):
            x = w.make_frames(n_walkers, seed=7, device=dev).double()
            x_static = x.clone()
            into = (torch.empty((n_walkers, d), **f64), torch.empty(n_walkers, **f64), torch.empty_like(x))
            fixed = mb.OpesRun(model, table, KT, BIASFACTOR, BARRIER, sigma0, sigma_min=sigma_min)
            runs = dict(adaptive=mb.OpesRun(model, table, KT, BIASFACTOR, BARRIER, "adaptive", sigma_min=sigma_min, adaptive_stride=STRIDE,
                                            walkers=n_walkers),
                        explore=mb.OpesRun(model, table, KT, BIASFACTOR, BARRIER, "adaptive", sigma_min=sigma_min, adaptive_stride=STRIDE,
                                           walkers=n_walkers, explore=True))
            with torch.no_grad():
                y0 = model(x)
            for name, run in runs.items():
                factor = 1.0 if name == "explore" else BIASFACTOR
                run.adapt[:, 0], run.adapt[:, 1], run.adapt[:, 2] = y0, OBSERVATIONS * factor * sigma0 ** 2, sigma0
                run.run[:3], run.run[6], run.run[7] = sums, OBSERVATIONS, 1.0
            fixed.run[:3] = sums
            run = runs["adaptive"]
            everything = (table.centers, table.sigma, table.heights, table.state, fixed.run, run.run, run.adapt, runs["explore"].run,
                          runs["explore"].adapt)
            saved = [t.clone() for t in everything]
            book, mean, M2 = run.run[:3].clone(), run.adapt[:, 0].clone(), run.adapt[:, 1].clone()      # route (a)'s state, on the device
            s0 = run.adapt[:, 2].clone()

            def restore():
                for dst, src in zip(everything, saved):
                    dst.data.copy_(src)
                book.data.copy_(saved[5][:3])
                mean.data.copy_(saved[6][:, 0])
                M2.data.copy_(saved[6][:, 1])

            def read_back():
                live, total, _, _ = table.read_state()
                rec = table.record(run.scale, total / live, run.epsilon, n=live)
                y, v, _ = model.value_and_opes(x, rec.centers, rec.heights, rec.sigma, rec.scale, rec.norm, rec.epsilon, rec.cutoff, rec.period,
                                               into=into)
                c = OBSERVATIONS + 1.0
                diff = y - mean
                mean.add_(diff / min(c, float(STRIDE)))
                M2.add_(diff * (y - mean))
                wts = torch.exp(run.beta * v)
                book[0] += float(n_walkers)
                book[1] += wts.sum()
                book[2] += (wts * wts).sum()
                neff = (1.0 + book[1]) ** 2 / (1.0 + book[2])
                sigma = torch.maximum(torch.sqrt(M2 / c / BIASFACTOR) * (neff * (d + 2.0) / 4.0) ** (-1.0 / (d + 4.0)), run.sigma_min)
                table.deposit(y, sigma, wts * (s0 / sigma).prod(dim=1))

            def pair(r, xx):
                def step():
                    y, v, _ = r.bias(xx, into=into)
                    r.deposit(y, v)
                return step

            def observe():
                run.observe(into[0])

            with torch.cuda.device(dev):
                ends = []
                for route in (read_back, pair(run, x)):
                    restore()
                    route()
                    ends.append(table.read_state())
                sa, sb = ends
                assert (sa[0], sa[2], sa[3]) == (sb[0], sb[2], sb[3]), (sa, sb)
                agree = abs(sa[1] - sb[1]) / max(1.0, abs(sb[1]))
                graphs = dict(fixed=graphed(dev, pair(fixed, x_static), restore), adaptive=graphed(dev, pair(run, x_static), restore))
                restore()
                graphs["adaptive"].replay()
                sc = table.read_state()
                assert sc == sb, (sc, sb)
                routes = (("f", pair(fixed, x)), ("fg", graphs["fixed"].replay), ("a", read_back), ("b", pair(run, x)),
                          ("c", graphs["adaptive"].replay), ("x", pair(runs["explore"], x)), ("o", observe))
                t = dict((k, []) for k, _ in routes)
                for _ in range(args.rounds):
                    for k, fn in routes:
                        t[k].append(timed(fn, restore))
            m = dict((k, statistics.median(v)) for k, v in t.items())
            print("C3-head2, %d walkers, %d kernels (%d live, %d merges after the step): (f) fixed eager %.1f us, graph %.1f us; (a) read-back %.1f us; "
                  "(b) adaptive eager %.1f us (%.2fx of f, %.2fx faster than a), (c) graph %.1f us (%.2fx of f's graph); (x) explore eager %.1f us; "
                  "(o) observe alone %.1f us; routes agree to %.1e"
                  % (n_walkers, n, sb[0], sb[2], m["f"], m["fg"], m["a"], m["b"], m["b"] / m["f"], m["a"] / m["b"], m["c"], m["c"] / m["fg"], m["x"],
                     m["o"], agree), flush=True)


if __name__ == "__main__":
    main()
