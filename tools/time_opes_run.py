#!/usr/bin/env python3
"""One whole OPES step - the bias and forces of W walkers, then the deposit of their W kernels - on C3's preprocessing behind a
[d_feat, 32, 2] tanh head ("C3-head2"), per step, in the same process, alternating:

    (a) read-back  the route before `value_and_opes_table`: `OpesTable.read_state()` (a blocking 32-byte read-back), `table.record`,
                   `value_and_opes` with n and norm = S / n by value, the weights, neff, the rescaled widths and the heights with torch
                   scalars on the device, `OpesTable.deposit`
    (b) eager      `OpesRun.bias` (molann_value_and_opes_table_f64) then `OpesRun.deposit` (molann_opes_step_f64): two launches,
                   nothing read back
    (c) graph      the pair of (b) captured once in a torch.cuda.graph and replayed

at 1 and 64 walkers on tables of 100 and 1000 kernels (a jittered lattice over the model's outputs, neighbours 1.5 widths apart, so a
walker's kernel merges into a neighbour or is appended, as in a run whose table has filled the visited region).  Times are HIP events
around one step, the median of 20 steps after 5 warm-up steps, so they hold the launches and whatever the host cannot hide behind the
device; the median of the rounds' medians is printed.  The table, its state and the run's sums are put back before every step, outside
the events and through `.data` (so that (a) keeps `value_and_opes`' remembered check of the widths, as it does in a loop while n does
not grow).  The three routes leave the same counts and, to rounding, the same S and sums: asserted before anything is timed.

    python tools/time_opes_run.py
    python tools/time_opes_run.py --walkers 64 --kernels 1000
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
        table = mb.OpesTable(n + 128, d, dev, cutoff=CUTOFF, threshold=THRESHOLD)
        table.centers[:n], table.sigma[:n], table.heights[:n] = lo + grid * spacing, sigma0, 1.0
        table.state[0] = float(n)
        table.recompute_sum(n=n)
        run = mb.OpesRun(model, table, KT, BIASFACTOR, BARRIER, sigma0, sigma_min=0.5 * sigma0)
        run.run[:3] = torch.tensor([200.0, 60.0, 30.0], **f64)        # a run that is 200 samples old: neff = 61^2 / 31
        saved = [t.clone() for t in (table.centers, table.sigma, table.heights, table.state, run.run)]
        book = run.run[:3].clone()                                     # route (a)'s sums, device scalars

        def restore():
            for dst, src in zip((table.centers, table.sigma, table.heights, table.state, run.run), saved):
                dst.data.copy_(src)
            book.data.copy_(saved[4][:3])

        for n_walkers in ([args.walkers] if args.walkers else [1, 64]):
            x = w.make_frames(n_walkers, seed=7, device=dev).double()
            x_static = x.clone()
            into = (torch.empty((n_walkers, d), **f64), torch.empty(n_walkers, **f64), torch.empty_like(x))

            def read_back():
                live, total, _, _ = table.read_state()
                rec = table.record(run.scale, total / live, run.epsilon, n=live)
                y, v, _ = model.value_and_opes(x, rec.centers, rec.heights, rec.sigma, rec.scale, rec.norm, rec.epsilon, rec.cutoff, rec.period,
                                               into=into)
                wts = torch.exp(run.beta * v)
                book[0] += float(n_walkers)
                book[1] += wts.sum()
                book[2] += (wts * wts).sum()
                neff = (1.0 + book[1]) ** 2 / (1.0 + book[2])
                sigma = torch.maximum(run.sigma0 * (neff * (d + 2.0) / 4.0) ** (-1.0 / (d + 4.0)), run.sigma_min)
                table.deposit(y, sigma, wts * (run.sigma0 / sigma).prod())

            def eager():
                y, v, _ = run.bias(x, into=into)
                run.deposit(y, v)

            def staged():
                y, v, _ = run.bias(x_static, into=into)
                run.deposit(y, v)

            with torch.cuda.device(dev):
                ends = []
                for route in (read_back, eager):
                    restore()
                    route()
                    ends.append((table.read_state(), run.run[:3].tolist() if route is eager else book.tolist()))
                (sa, ba), (sb, bb) = ends
                assert (sa[0], sa[2], sa[3]) == (sb[0], sb[2], sb[3]), (sa, sb)
                agree = max(abs(sa[1] - sb[1]) / max(1.0, abs(sb[1])), max(abs(p - q) / max(1.0, abs(q)) for p, q in zip(ba, bb)))
                side = torch.cuda.Stream(device=dev)
                side.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(side):
                    restore()
                    staged()
                torch.cuda.current_stream(dev).wait_stream(side)
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                restore()
                with torch.cuda.graph(graph):
                    staged()
                restore()
                graph.replay()
                sc = table.read_state()
                assert (sc[0], sc[1], sc[2], sc[3]) == (sb[0], sb[1], sb[2], sb[3]), (sc, sb)
                t = {"a": [], "b": [], "c": []}
                for _ in range(args.rounds):
                    t["a"].append(timed(read_back, restore))
                    t["b"].append(timed(eager, restore))
                    t["c"].append(timed(graph.replay, restore))
            a, b, c = (statistics.median(t[k]) for k in "abc")
            print("C3-head2, %d walkers, %d kernels (%d live, %d merges after the step): (a) read-back %.1f us, (b) eager pair %.1f us (%.2fx), "
                  "(c) graph replay %.1f us (%.2fx); routes agree to %.1e" % (n_walkers, n, sb[0], sb[2], a, b, a / b, c, a / c, agree), flush=True)


if __name__ == "__main__":
    main()
