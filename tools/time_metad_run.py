#!/usr/bin/env python3
"""One whole well-tempered metadynamics step on a table - the bias and forces of W walkers, then the deposit of their W hills - on C3's
preprocessing behind a [d_feat, 32, d] tanh head, per step, in the same process, alternating:

    (a) eager   `MetadRun.bias` (molann_value_and_grid_f64) then `MetadRun.deposit` (molann_metad_deposit_f64): two launches, nothing
                read back
    (b) graph   the pair of (a) captured once in a torch.cuda.graph and replayed
    (c) torch   the route without the deposit kernel: `value_and_grid`, the heights ``height exp(-V / (kT (biasfactor - 1)))`` with torch
                on the device, `bias.add_hills_to_grid` on the device table (it has no cutoff: it writes every entry either way)

at 1 and 64 walkers on tables of 256^2, 1024^2 and 128^3 entries over the model's outputs (sigma = 3 spacings, a table that already
holds a few hundred hills), with PLUMED's cutoff of 6.25 widths and with none.  Times are HIP events around one step, the median of 20
steps after 5 warm-up steps, so they hold the launches and whatever the host cannot hide behind the device; the median of the rounds'
medians is printed.  The table and the state are put back before every step, outside the events.  Routes (a) and (c) without a cutoff
leave the same table to rounding: asserted before anything is timed.

    python tools/time_metad_run.py
    python tools/time_metad_run.py --walkers 1 --table 128,128,128 --cutoff 6.25
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

KT, BIASFACTOR, HEIGHT = 2.494, 10.0, 1.2


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
    ap.add_argument("--table", default="", help="one table shape, e.g. 1024,1024, instead of 256^2, 1024^2 and 128^3")
    ap.add_argument("--cutoff", type=float, default=-1.0, help="one cutoff in widths (0: none) instead of 6.25 and none")
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    f64 = dict(dtype=torch.float64, device=dev)
    w = wl.get_workload("C3")
    base = wl.build_model(w, dev)
    shapes = [tuple(int(n) for n in args.table.split(","))] if args.table else [(256, 256), (1024, 1024), (128, 128, 128)]
    cutoffs = [args.cutoff if args.cutoff > 0 else None] if args.cutoff >= 0 else [6.25, None]
    models = {}
    for shape in shapes:
        d = len(shape)
        if d not in models:
            torch.manual_seed(11)
            model = MolANN(base.preprocessing_layer, create_sequential_nn([w.feature_dim(), 32, d], activation=torch.nn.Tanh())).to(dev)
            model = model.double().requires_grad_(False)
            with torch.no_grad():
                visited = model(w.make_frames(4096, seed=3, device=dev).double())
            models[d] = (model, visited)
        model, visited = models[d]
        lo, hi = visited.min(dim=0).values, visited.max(dim=0).values
        span = (hi - lo) * 1.2
        lower = (lo - 0.1 * (hi - lo)).tolist()
        spacing = [float(span[k]) / (shape[k] - 1) for k in range(d)]
        sigma = [3.0 * s for s in spacing]
        start = torch.zeros(shape, **f64)
        mb.add_hills_to_grid(start, lower, spacing, None, visited[:256], HEIGHT, sigma, chunk=16 if d == 3 else 256)
        for cutoff in cutoffs:
            table = start.clone()
            run = mb.MetadRun(model, table, lower, spacing, KT, BIASFACTOR, HEIGHT, sigma, cutoff=cutoff)

            def restore():
                table.copy_(start)
                run.state.zero_()

            for n_walkers in ([args.walkers] if args.walkers else [1, 64]):
                x = w.make_frames(n_walkers, seed=7, device=dev).double()
                x_static = x.clone()
                into = (torch.empty((n_walkers, d), **f64), torch.empty(n_walkers, **f64), torch.empty_like(x))

                def eager():
                    y, v, _ = run.bias(x, into=into)
                    run.deposit(y, v)

                def staged():
                    y, v, _ = run.bias(x_static, into=into)
                    run.deposit(y, v)

                def by_torch():
                    y, v, _ = model.value_and_grid(x, table, lower, spacing, None, into=into)
                    mb.add_hills_to_grid(table, lower, spacing, None, y, HEIGHT * torch.exp(-v * run.inv_dT), sigma)

                with torch.cuda.device(dev):
                    restore()
                    eager()
                    ours, state = table.clone(), run.read_state()
                    restore()
                    by_torch()
                    # with a cutoff the kernel leaves out at most exp(-cutoff^2 / 2) of every height
                    slack = 0.0 if cutoff is None else n_walkers * HEIGHT * math.exp(-0.5 * cutoff * cutoff)
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
                    t = {"a": [], "b": [], "c": []}
                    for _ in range(args.rounds):
                        t["a"].append(timed(eager, restore))
                        t["b"].append(timed(graph.replay, restore))
                        t["c"].append(timed(by_torch, restore))
                a, b, c = (statistics.median(t[k]) for k in "abc")
                print("C3-head%d, table %s, cutoff %s, %d walkers: (a) eager pair %.1f us, (b) graph replay %.1f us, (c) torch route %.1f us "
                      "(%.2fx of a, %.2fx of b); routes agree to %.1e" % (d, "x".join(str(n) for n in shape), cutoff, n_walkers, a, b, c, c / a,
                                                                         c / b, agree), flush=True)


if __name__ == "__main__":
    main()
