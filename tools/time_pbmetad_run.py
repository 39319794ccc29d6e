#!/usr/bin/env python3
"""One whole parallel-bias metadynamics step - the bias and forces of W walkers under K one-dimensional tables joined by a soft minimum,
then the deposit of their W x K weighted hills - on C3 behind its 8-output head, per step, in the same process, alternating:

    (a) eager   `PBMetadRun.bias` (molann_value_and_pbmetad_f64) then `PBMetadRun.deposit` (molann_pbmetad_deposit_f64): two launches,
                nothing read back
    (b) graph   the pair of (a) captured once in a torch.cuda.graph and replayed
    (c) metad   K = 1 only: the `MetadRun` step (value_and_bias with the table on one column, molann_metad_deposit_f64) on the same 1-D
                table - the path that was there before
    (d) torch   the route without this feature: the forward, K 1-D interpolations, the soft minimum and its autograd in torch,
                `value_and_vjp`, the heights in torch, K calls of `bias.add_hills_to_grid` on the views

for K in {1, 3, 8}, W in {1, 64} and tables of 256 and 4096 points per axis over the model's outputs (sigma = 3 spacings, tables that
already hold a few hundred hills, PLUMED's cutoff of 6.25 widths).  Times are HIP events around one step, the median of 20 steps after 5
warm-up steps; the median of the rounds' medians is printed.  The tables and the state are put back before every step, outside the
events.  Before anything is timed: routes (a) and (d) leave the same tables within the tables' bound (and what the cutoff leaves out),
and the replay gives the eager bits.  The frame kernel's cost above `value_and_vjp` alone is printed per K at 1 and 64 frames.

    python tools/time_pbmetad_run.py
    python tools/time_pbmetad_run.py --axes 8 --walkers 1 --points 4096
"""
import argparse
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from molann_amd import bias as mb, workloads as wl  # noqa: E402

KT, BIASFACTOR, HEIGHT, CUTOFF = 2.494, 10.0, 1.2, 6.25
COLUMNS = {1: (5,), 3: (5, 0, 2), 8: None}


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


def interpolate(y, table, n, lower, spacing):
    """Catmull-Rom on one non-periodic axis with torch: the value at y [W], differentiable in y"""
    u = torch.clamp((y - lower) / spacing, 0.0, n - 1.0)
    i = torch.clamp(torch.floor(u.detach()), max=n - 2).long()
    t = u - i
    w = ((-t ** 3 + 2 * t ** 2 - t) / 2, (3 * t ** 3 - 5 * t ** 2 + 2) / 2, (-3 * t ** 3 + 4 * t ** 2 + t) / 2, (t ** 3 - t ** 2) / 2)
    return sum(table[torch.clamp(i - 1 + j, 0, n - 1)] * w[j] for j in range(4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--axes", type=int, default=0, help="one K instead of 1, 3 and 8")
    ap.add_argument("--walkers", type=int, default=0, help="one number of walkers instead of 1 and 64")
    ap.add_argument("--points", type=int, default=0, help="one table size per axis instead of 256 and 4096")
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    f64 = dict(dtype=torch.float64, device=dev)
    w = wl.get_workload("C3")
    model = wl.build_model(w, dev).double().requires_grad_(False)
    with torch.no_grad():
        visited = model(w.make_frames(4096, seed=3, device=dev).double())
    for n_walkers in ([args.walkers] if args.walkers else [1, 64]):
        x = w.make_frames(n_walkers, seed=7, device=dev).double()
        g = torch.zeros(n_walkers, 8, **f64)
        yv, dxv = torch.empty(n_walkers, 8, **f64), torch.empty_like(x)
        t_vjp = statistics.median(timed(lambda: model.value_and_vjp(x, g, into=(yv, dxv)), lambda: None) for _ in range(args.rounds))
        for K in ([args.axes] if args.axes else [1, 3, 8]):
            columns = COLUMNS[K]
            cols = list(range(8)) if columns is None else list(columns)
            for points in ([args.points] if args.points else [256, 4096]):
                shape = (points,) * K
                lo, hi = visited[:, cols].min(dim=0).values, visited[:, cols].max(dim=0).values
                lower = (lo - 0.1 * (hi - lo)).tolist()
                spacing = [float(1.2 * (hi[k] - lo[k])) / (points - 1) for k in range(K)]
                sigma = [3.0 * s for s in spacing]
                start = torch.zeros(K * points, **f64)
                for k in range(K):
                    mb.add_hills_to_grid(start[k * points:(k + 1) * points], [lower[k]], [spacing[k]], None, visited[:256, cols[k]:cols[k] + 1],
                                         HEIGHT / K, [sigma[k]])
                table = start.clone()
                run = mb.PBMetadRun(model, shape, lower, spacing, KT, BIASFACTOR, HEIGHT, sigma, cutoff=CUTOFF, columns=columns, table=table)
                views = run.tables
                x_static = x.clone()
                into = (torch.empty(n_walkers, 8, **f64), torch.empty(n_walkers, 2 + K, **f64), torch.empty_like(x))
                metad = None
                if K == 1:
                    metad = mb.MetadRun(model, table, lower, spacing, KT, BIASFACTOR, HEIGHT, sigma, cutoff=CUTOFF, columns=columns)
                    into_m = (torch.empty(n_walkers, 8, **f64), torch.empty(n_walkers, 3, **f64), torch.empty_like(x))

                def restore():
                    table.copy_(start)
                    run.state.zero_()

                def eager():
                    y, e, _ = run.bias(x, into=into)
                    run.deposit(y, e)

                def staged():
                    y, e, _ = run.bias(x_static, into=into)
                    run.deposit(y, e)

                def by_metad():
                    y, e, _ = metad.bias(x, into=into_m)
                    metad.deposit(y, e)

                def by_torch():
                    with torch.no_grad():
                        y = model(x)
                    ys = y[:, cols].clone().requires_grad_(True)
                    V = torch.stack([interpolate(ys[:, k], views[k], points, lower[k], spacing[k]) for k in range(K)], dim=1)
                    vpb = -KT * torch.logsumexp(-V / KT, dim=1)
                    (dys,) = torch.autograd.grad(vpb.sum(), ys)
                    cot = torch.zeros_like(y)
                    cot[:, cols] = dys
                    model.value_and_vjp(x, cot, into=(yv, dxv))
                    V = V.detach()
                    heights = HEIGHT * torch.exp(-V * run.inv_dT) * torch.softmax(-V / KT, dim=1)
                    for k in range(K):
                        mb.add_hills_to_grid(views[k], [lower[k]], [spacing[k]], None, y[:, cols[k]:cols[k] + 1], heights[:, k], [sigma[k]])

                with torch.cuda.device(dev):
                    restore()
                    eager()
                    ours, state = table.clone(), run.read_state()
                    restore()
                    by_torch()
                    # with a cutoff the kernel leaves out at most exp(-cutoff^2 / 2) of every height
                    slack = n_walkers * HEIGHT * math.exp(-0.5 * CUTOFF * CUTOFF)
                    agree = float((ours - table).abs().max())
                    assert agree <= 1e-12 * (state["sum_heights"] + float(start.abs().max())) + slack, (agree, slack)
                    assert state["hills"] == n_walkers and state["refused"] == 0
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
                    torch.cuda.synchronize()
                    assert torch.equal(table, ours), "the replay and the eager pair differ"
                    t = {"a": [], "b": [], "c": [], "d": [], "f": []}
                    for _ in range(args.rounds):
                        t["a"].append(timed(eager, restore))
                        t["b"].append(timed(graph.replay, restore))
                        if metad is not None:
                            t["c"].append(timed(by_metad, lambda: (restore(), metad.state.zero_())))
                        t["d"].append(timed(by_torch, restore))
                        t["f"].append(timed(lambda: run.bias(x, into=into), restore))
                a, b, d, f = (statistics.median(t[k]) for k in "abdf")
                c = statistics.median(t["c"]) if t["c"] else None
                print("C3 K=%d, %d points per axis, %d walkers: (a) eager pair %.1f us, (b) graph replay %.1f us, (c) MetadRun step %s, (d) torch "
                      "route %.1f us (%.2fx of a, %.2fx of b); frame kernel %.1f us, %+.1f us over value_and_vjp (%.1f us); routes agree to %.1e"
                      % (K, points, n_walkers, a, b, "-" if c is None else "%.1f us (a / c = %.2f)" % (c, a / c), d, d / a, d / b, f, f - t_vjp,
                         t_vjp, agree), flush=True)
                del graph


if __name__ == "__main__":
    main()
