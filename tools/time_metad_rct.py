#!/usr/bin/env python3
"""The reweighting offset c(t) of a metadynamics run kept on the device, on tables of 256^2, 1024^2 and 128^3 entries that hold a few
hundred hills, in the same process, alternating:

    (a) rct     `molann_metad_rct_f64` alone: the partial and the combine launch on the table
    (b) torch   the route without the kernels, on the same table, without its `.item()`:
                ``kT (torch.logsumexp(a0 table) - torch.logsumexp(aV table))``
    (c) steps   `MetadRun.bias` then `MetadRun.deposit` for one walker with a cutoff of 6.25 widths on C3's preprocessing behind a
                [d_feat, 32, d] tanh head, with ``rct_stride`` None (the step without the offset), 1 and 10, eager and as one captured
                graph replayed

Times are HIP events around one call, after 5 warm-up calls, so they hold the launches and whatever the host cannot hide behind the
device; per round the median of 20 calls (and for (c) their mean as well: with a stride of 10 two steps in 20 update, which a median
does not show), and the median of three rounds' figures is printed.  For (c) the table is put back and the state's step count set to the
running step number before every step, outside the events.  Before anything is timed (a) is asserted against (b) within
``1e-12 (kT + |M|)`` and the replayed steps against the eager steps' bits.

    python tools/time_metad_rct.py
    python tools/time_metad_rct.py --table 128,128,128
"""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from molann_amd import _capi, bias as mb, workloads as wl  # noqa: E402
from molann_amd.ann import MolANN, create_sequential_nn  # noqa: E402

KT, BIASFACTOR, HEIGHT, CUTOFF = 2.494, 10.0, 1.2, 6.25


def timed(fn, setup, calls=20, warmup=5):
    """(median, mean) of `calls` calls after `warmup`, each between two HIP events and after `setup()`, in microseconds"""
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
    return statistics.median(times), statistics.fmean(times)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--table", default="", help="one table shape, e.g. 1024,1024, instead of 256^2, 1024^2 and 128^3")
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    f64 = dict(dtype=torch.float64, device=dev)
    w = wl.get_workload("C3")
    base = wl.build_model(w, dev)
    shapes = [tuple(int(n) for n in args.table.split(","))] if args.table else [(256, 256), (1024, 1024), (128, 128, 128)]
    inv_dT = 1.0 / (KT * (BIASFACTOR - 1.0))
    a0 = 1.0 / KT + inv_dT
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
        name = "x".join(str(n) for n in shape)
        with torch.cuda.device(dev):
            # (a) against (b)
            partials = torch.zeros(int(_capi.lib().molann_metad_rct_chunks(start.numel())), 4, **f64)
            rct = torch.zeros(8, **f64)

            def ours():
                _capi.metad_rct_f64(start, KT, inv_dT, None, 1, partials, rct)

            def by_torch():
                flat = start.reshape(-1)
                return KT * (torch.logsumexp(a0 * flat, 0) - torch.logsumexp(inv_dT * flat, 0))

            ours()
            got, want = rct.tolist(), float(by_torch())
            assert abs(got[0] - want) <= 1e-12 * (KT + abs(got[2])), (got, want)
            t = {"a": [], "b": []}
            for _ in range(args.rounds):
                t["a"].append(timed(ours, lambda: None)[0])
                t["b"].append(timed(by_torch, lambda: None)[0])
            a, b = statistics.median(t["a"]), statistics.median(t["b"])
            print("table %s: (a) rct pair %.1f us, (b) torch route %.1f us (%.2fx of a); c %.6f of max %.6f, they agree to %.1e"
                  % (name, a, b, b / a, got[0], got[2], abs(got[0] - want)), flush=True)

            # (c) whole steps
            x = w.make_frames(1, seed=7, device=dev).double()
            step_no = [0]
            cells = {}
            for stride in (None, 1, 10):
                table = start.clone()
                run = mb.MetadRun(model, table, lower, spacing, KT, BIASFACTOR, HEIGHT, sigma, cutoff=CUTOFF, rct_stride=stride)
                into = (torch.empty((1, d), **f64), torch.empty(1, **f64), torch.empty_like(x))

                def restore(run=run, table=table):
                    table.copy_(start)
                    run.state.zero_()
                    run.state[3] = float(step_no[0])
                    step_no[0] += 1

                def step(run=run, into=into):
                    y, v, _ = run.bias(x, into=into)
                    run.deposit(y, v)

                def snapshot(run=run, table=table):
                    torch.cuda.synchronize()
                    return [u.clone() for u in (table, run.state) + ((run.rct,) if run.rct is not None else ())]

                side = torch.cuda.Stream(device=dev)
                side.wait_stream(torch.cuda.current_stream(dev))
                with torch.cuda.stream(side):
                    restore()
                    step()
                torch.cuda.current_stream(dev).wait_stream(side)
                torch.cuda.synchronize()
                graph = torch.cuda.CUDAGraph()
                with torch.cuda.graph(graph):
                    step()
                for k in (9, 10):                                     # off and on a stride of 10
                    if run.rct is not None:
                        run.rct.zero_()
                    step_no[0] = k - 1
                    restore()
                    step()
                    eager = snapshot()
                    if run.rct is not None:
                        run.rct.zero_()
                    step_no[0] = k - 1
                    restore()
                    graph.replay()
                    assert all(torch.equal(p, q) for p, q in zip(eager, snapshot())), "the replay and the eager step differ"
                    assert stride is None or float(run.rct[1]) == (1.0 if k % stride == 0 else 0.0)
                step_no[0] = 0
                cells[stride] = (step, graph, restore, {"eager": [], "graph": []})
            for _ in range(args.rounds):
                for stride in (None, 1, 10):
                    step, graph, restore, t = cells[stride]
                    step_no[0] = 0
                    t["eager"].append(timed(step, restore))
                    step_no[0] = 0
                    t["graph"].append(timed(graph.replay, restore))
            for stride in (None, 1, 10):
                t = cells[stride][3]
                figures = [statistics.median(v[i] for v in t[k]) for k in ("eager", "graph") for i in (0, 1)]
                print("table %s, 1 walker, cutoff %s, rct_stride %s: (c) eager step median %.1f us, mean %.1f us; replayed step median %.1f us, "
                      "mean %.1f us" % (name, CUTOFF, stride, figures[0], figures[1], figures[2], figures[3]), flush=True)
            del cells


if __name__ == "__main__":
    main()
