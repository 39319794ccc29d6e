#!/usr/bin/env python3
"""One whole OPES step with walls on a wider model - the bias and forces of W walkers, then the deposit of their W kernels - on C3 with its
own [6, 32, 8] head, OPES on outputs (5, 2), flat-bottomed walls on all 8, per step, in the same process, alternating:

    (a) read-back  the route before `OpesFromTable`: `OpesTable.read_state()` (a blocking 32-byte read-back), `table.record`,
                   `value_and_bias(restraint=walls, opes=record)` with n and norm = S / n by value, the weights, neff, the rescaled
                   widths and the heights with torch scalars on the device, `OpesTable.deposit` of `y[:, columns]`
    (b) eager      `OpesRun(columns=, walls=).bias` (molann_value_and_bias_opes_table_f64) then `.deposit`
                   (molann_opes_step_columns_f64): two launches, nothing read back
    (c) graph      the pair of (b) captured once in a torch.cuda.graph and replayed
    (plain)        beside them, from the same process: the eager pair and the graph replay of the plain `OpesRun` on C3's preprocessing
                   behind a [d_feat, 32, 2] head (tools/time_opes_run.py's model), whose two outputs are the table's columns

at 1 and 64 walkers on tables of 100 and 1000 kernels (a jittered lattice over the two outputs, neighbours 1.5 widths apart, so a
walker's kernel merges into a neighbour or is appended).  The method is tools/time_opes_run.py's: HIP events around one step, the median of
20 steps after 5 warm-up steps, three alternating rounds, the median round; the table, its state and the run's sums are put back before
every step, outside the events and through `.data`.  The three routes leave the same counts and, to rounding, the same S and sums:
asserted before anything is timed.

    python tools/time_opes_run_bias.py
    python tools/time_opes_run_bias.py --walkers 64 --kernels 1000
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
from time_opes_run import BARRIER, BIASFACTOR, CUTOFF, KT, THRESHOLD, timed  # noqa: E402

COLUMNS = (5, 2)


def lattice_table(dev, visited, n, extra=128):
    """(table, sigma0): n kernels on a jittered lattice over the range of `visited` [M, 2], neighbours 1.5 widths apart"""
    lo, hi = visited.min(dim=0).values, visited.max(dim=0).values
    per = int(math.ceil(math.sqrt(n)))
    g = torch.Generator().manual_seed(5)
    grid = torch.stack(torch.meshgrid(torch.arange(per, dtype=torch.float64), torch.arange(per, dtype=torch.float64), indexing="ij"), dim=-1)
    grid = (grid.reshape(-1, 2)[:n] + 0.1 * torch.rand(n, 2, generator=g, dtype=torch.float64)).to(dev)
    spacing = (hi - lo) / per
    sigma0 = (spacing / 1.5).contiguous()
    table = mb.OpesTable(n + extra, 2, dev, cutoff=CUTOFF, threshold=THRESHOLD)
    table.centers[:n], table.sigma[:n], table.heights[:n] = lo + grid * spacing, sigma0, 1.0
    table.state[0] = float(n)
    table.recompute_sum(n=n)
    return table, sigma0


def captured(step, restore, dev):
    """one graph of `step`, after a step on a side stream"""
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        restore()
        step()
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    restore()
    with torch.cuda.graph(graph):
        step()
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
    model = wl.build_model(w, dev).double().requires_grad_(False)           # C3 as it is: MLP [6, 32, 8]
    torch.manual_seed(11)
    head2 = MolANN(wl.build_model(w, dev).preprocessing_layer, create_sequential_nn([w.feature_dim(), 32, 2], activation=torch.nn.Tanh())).to(dev)
    head2 = head2.double().requires_grad_(False)
    d_out, cols = w.out_dim(), list(COLUMNS)
    with torch.no_grad():
        frames = w.make_frames(4096, seed=3, device=dev).double()
        visited, visited2 = model(frames), head2(frames)
    spread = visited.std(dim=0)
    walls = mb.Restraint(visited.mean(dim=0).contiguous(), (3.0 / spread ** 2).contiguous(), flat=(0.5 * spread).contiguous())
    for n in ([args.kernels] if args.kernels else [100, 1000]):
        table, sigma0 = lattice_table(dev, visited[:, cols], n)
        run = mb.OpesRun(model, table, KT, BIASFACTOR, BARRIER, sigma0, sigma_min=0.5 * sigma0, columns=COLUMNS, walls=walls)
        table2, sigma02 = lattice_table(dev, visited2, n)
        run2 = mb.OpesRun(head2, table2, KT, BIASFACTOR, BARRIER, sigma02, sigma_min=0.5 * sigma02)
        for r in (run, run2):
            r.run[:3] = torch.tensor([200.0, 60.0, 30.0], **f64)      # a run that is 200 samples old: neff = 61^2 / 31
        saved = [t.clone() for t in (table.centers, table.sigma, table.heights, table.state, run.run)]
        saved2 = [t.clone() for t in (table2.centers, table2.sigma, table2.heights, table2.state, run2.run)]
        book = run.run[:3].clone()                                     # route (a)'s sums, device scalars

        def restore():
            for dst, src in zip((table.centers, table.sigma, table.heights, table.state, run.run), saved):
                dst.data.copy_(src)
            book.data.copy_(saved[4][:3])

        def restore2():
            for dst, src in zip((table2.centers, table2.sigma, table2.heights, table2.state, run2.run), saved2):
                dst.data.copy_(src)

        for n_walkers in ([args.walkers] if args.walkers else [1, 64]):
            x = w.make_frames(n_walkers, seed=7, device=dev).double()
            x_static = x.clone()
            into = (torch.empty((n_walkers, d_out), **f64), torch.empty((n_walkers, 4), **f64), torch.empty_like(x))
            into2 = (torch.empty((n_walkers, 2), **f64), torch.empty(n_walkers, **f64), torch.empty_like(x))

            def read_back():
                live, total, _, _ = table.read_state()
                rec = table.record(run.scale, total / live, run.epsilon, COLUMNS, n=live)
                y, e, _ = model.value_and_bias(x, restraint=walls, opes=rec, into=into)
                wts = torch.exp(run.beta * e[:, 3])
                book[0] += float(n_walkers)
                book[1] += wts.sum()
                book[2] += (wts * wts).sum()
                neff = (1.0 + book[1]) ** 2 / (1.0 + book[2])
                sigma = torch.maximum(run.sigma0 * (neff * (2 + 2.0) / 4.0) ** (-1.0 / (2 + 4.0)), run.sigma_min)
                table.deposit(y[:, cols], sigma, wts * (run.sigma0 / sigma).prod())

            def eager():
                y, e, _ = run.bias(x, into=into)
                run.deposit(y, e)

            def staged():
                y, e, _ = run.bias(x_static, into=into)
                run.deposit(y, e)

            def plain():
                y, v, _ = run2.bias(x_static, into=into2)
                run2.deposit(y, v)

            with torch.cuda.device(dev):
                ends = []
                for route in (read_back, eager):
                    restore()
                    route()
                    ends.append((table.read_state(), run.run[:3].tolist() if route is eager else book.tolist()))
                (sa, ba), (sb, bb) = ends
                assert (sa[0], sa[2], sa[3]) == (sb[0], sb[2], sb[3]), (sa, sb)
                agree = max(abs(sa[1] - sb[1]) / max(1.0, abs(sb[1])), max(abs(p - q) / max(1.0, abs(q)) for p, q in zip(ba, bb)))
                graph = captured(staged, restore, dev)
                restore()
                graph.replay()
                sc = table.read_state()
                assert (sc[0], sc[1], sc[2], sc[3]) == (sb[0], sb[1], sb[2], sb[3]), (sc, sb)
                graph2 = captured(plain, restore2, dev)
                t = {"a": [], "b": [], "c": [], "pb": [], "pc": []}
                for _ in range(args.rounds):
                    t["a"].append(timed(read_back, restore))
                    t["b"].append(timed(eager, restore))
                    t["c"].append(timed(graph.replay, restore))
                    t["pb"].append(timed(plain, restore2))
                    t["pc"].append(timed(graph2.replay, restore2))
            a, b, c, pb, pc = (statistics.median(t[k]) for k in ("a", "b", "c", "pb", "pc"))
            print("C3 (8 outputs, OPES on %s, walls on all), %d walkers, %d kernels (%d live, %d merges after the step): (a) read-back %.1f us, "
                  "(b) eager pair %.1f us (%.2fx), (c) graph replay %.1f us (%.2fx); plain OpesRun on C3-head2: eager %.1f us, replay %.1f us; "
                  "routes agree to %.1e" % (COLUMNS, n_walkers, n, sb[0], sb[2], a, b, a / b, c, a / c, pb, pc, agree), flush=True)


if __name__ == "__main__":
    main()
