#!/usr/bin/env python3
"""One whole metadynamics step with adaptive, correlated hills - the bias and forces of W walkers, their covariances, then the deposit of
their W hills - on C3's preprocessing behind a [d_feat, 32, d] tanh head, per step, in the same process, alternating:

    (diff)   `MetadRun(adaptive="diff")`: bias, widths (observe and emit), covariant deposit - 3 launches, eager and as a replayed graph
    (geom)   `MetadRun(adaptive="geom")`: bias, `value_and_metric`, widths, covariant deposit - 4 launches, eager and as a replayed graph

each against two references, never against itself:

    (fixed)  the fixed-sigma step of a `MetadRun` made without `adaptive` (molann_value_and_grid_f64, molann_metad_deposit_f64), eager and
             replayed: what the run cost before
    (torch)  the route without the new kernels: `value_and_grid` (and `value_and_metric`), the running covariance, the limits and the
             heights in torch ops on the device, `bias.add_cov_hills_to_grid` on the device table

on tables of 256^2, 1024^2 and 128^3 entries over the model's outputs (widths of about 3 spacings, a table that already holds a few
hundred hills), with one walker and PLUMED's cutoff of 6.25, and with 64 walkers and no cutoff.  Times are HIP events around one step,
the median of 20 steps after 5 warm-up steps; the median of the rounds' medians is printed.  The table, the state and the running
statistics are put back before every step, outside the events.  The kernels' route and the torch route leave the same table to
rounding: asserted before anything is timed.

    python tools/time_metad_adaptive.py
    python tools/time_metad_adaptive.py --table 128,128,128 --walkers 64
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

KT, BIASFACTOR, HEIGHT, WINDOW = 2.494, 10.0, 1.2, 10


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


def captured(dev, fn, restore):
    """`fn` run once on a side stream, then captured: the graph"""
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


def limited(C, lo2, hi2):
    """SIGMA_MIN / SIGMA_MAX on [W, d, d] matrices with positive diagonals, in torch ops"""
    diag = torch.diagonal(C, dim1=1, dim2=2)
    s = (diag.clamp(lo2, hi2) / diag).sqrt()
    return C * s[:, :, None] * s[:, None, :]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--walkers", type=int, default=0, help="1 (with cutoff 6.25) or 64 (with none) instead of both")
    ap.add_argument("--table", default="", help="one table shape, e.g. 1024,1024, instead of 256^2, 1024^2 and 128^3")
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    f64 = dict(dtype=torch.float64, device=dev)
    w = wl.get_workload("C3")
    base = wl.build_model(w, dev)
    shapes = [tuple(int(n) for n in args.table.split(","))] if args.table else [(256, 256), (1024, 1024), (128, 128, 128)]
    configs = [(1, 6.25), (64, None)]
    if args.walkers:
        configs = [c for c in configs if c[0] == args.walkers]
    models = {}
    for shape in shapes:
        d = len(shape)
        T = d * (d + 1) // 2
        iu = torch.triu_indices(d, d, device=dev)
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
        sigma_min, sigma_max = [1.0 * s for s in spacing], [6.0 * s for s in spacing]
        lo2, hi2 = torch.tensor(sigma_min, **f64) ** 2, torch.tensor(sigma_max, **f64) ** 2
        start = torch.zeros(shape, **f64)
        mb.add_hills_to_grid(start, lower, spacing, None, visited[:256], HEIGHT, sigma, chunk=16 if d == 3 else 256)
        for n_walkers, cutoff in configs:
            x = w.make_frames(n_walkers, seed=7, device=dev).double()
            into = (torch.empty((n_walkers, d), **f64), torch.empty(n_walkers, **f64), torch.empty_like(x))
            metric_into = (torch.empty((n_walkers, d), **f64), torch.empty((n_walkers, d, d), **f64))
            y0, M0 = model.value_and_metric(x)
            geom_sigma = [3.0 * spacing[k] / float(M0[:, k, k].median().sqrt()) for k in range(d)]
            table = start.clone()
            common = dict(cutoff=cutoff, sigma_min=sigma_min, sigma_max=sigma_max, walkers=n_walkers)
            runs = dict(fixed=mb.MetadRun(model, table, lower, spacing, KT, BIASFACTOR, HEIGHT, sigma, cutoff=cutoff),
                        diff=mb.MetadRun(model, table, lower, spacing, KT, BIASFACTOR, HEIGHT, sigma, adaptive="diff", window=WINDOW, **common),
                        geom=mb.MetadRun(model, table, lower, spacing, KT, BIASFACTOR, HEIGHT, geom_sigma, adaptive="geom", **common))
            # the walkers' recent motion: 2 WINDOW observations around their outputs, steps of about 3 spacings, correlated
            gen = torch.Generator(device=dev).manual_seed(5)
            mix = torch.eye(d, **f64) + 0.6 * (torch.ones(d, d, **f64) - torch.eye(d, **f64))
            for _ in range(2 * WINDOW):
                noise = torch.randn(n_walkers, d, generator=gen, **f64) @ mix * torch.tensor(sigma, **f64) * 0.7
                runs["diff"].observe(y0 + noise)
            adapt0 = runs["diff"].adapt.clone()
            t_n, t_mean, t_cov = adapt0[:, 0].clone(), adapt0[:, 1:1 + d].clone(), torch.zeros(n_walkers, d, d, **f64)
            fixed_diag = torch.diag(torch.tensor(sigma, **f64) ** 2).expand(n_walkers, d, d)
            g_sig = torch.tensor(geom_sigma, **f64)

            def restore():
                table.copy_(start)
                for run in runs.values():
                    run.state.zero_()
                runs["diff"].adapt.copy_(adapt0)
                t_n.copy_(adapt0[:, 0])
                t_mean.copy_(adapt0[:, 1:1 + d])
                t_cov[:, iu[0], iu[1]] = adapt0[:, 1 + d:]
                t_cov[:, iu[1], iu[0]] = adapt0[:, 1 + d:]

            def fixed():
                y, v, _ = runs["fixed"].bias(x, into=into)
                runs["fixed"].deposit(y, v)

            def diff():
                y, v, _ = runs["diff"].bias(x, into=into)
                runs["diff"].deposit(y, v)

            def geom():
                y, v, _ = runs["geom"].bias(x, into=into)
                runs["geom"].deposit(y, v, metric=model.value_and_metric(x, into=metric_into)[1])

            def torch_diff():
                y, v, _ = model.value_and_grid(x, table, lower, spacing, None, into=into)
                delta = y - t_mean
                t_mean.add_(delta / WINDOW)
                t_cov.add_((delta[:, :, None] * delta[:, None, :] - t_cov) / WINDOW)
                t_n.add_(1.0)
                C = limited(torch.where((t_n >= WINDOW)[:, None, None], t_cov, fixed_diag), lo2, hi2)
                mb.add_cov_hills_to_grid(table, lower, spacing, None, y, C[:, iu[0], iu[1]], HEIGHT * torch.exp(-v * runs["diff"].inv_dT), cutoff=cutoff)

            def torch_geom():
                y, v, _ = model.value_and_grid(x, table, lower, spacing, None, into=into)
                M = model.value_and_metric(x, into=metric_into)[1]
                C = limited(M * g_sig[:, None] * g_sig[None, :], lo2, hi2)
                mb.add_cov_hills_to_grid(table, lower, spacing, None, y, C[:, iu[0], iu[1]], HEIGHT * torch.exp(-v * runs["geom"].inv_dT), cutoff=cutoff)

            with torch.cuda.device(dev):
                agree = {}
                for name, ours, theirs in (("diff", diff, torch_diff), ("geom", geom, torch_geom)):
                    restore()
                    ours()
                    got, state = table.clone(), runs[name].read_state()
                    restore()
                    theirs()
                    agree[name] = float((got - table).abs().max())
                    # a grid point on the cutoff's edge may fall on either side of it: at most exp(-cutoff^2 / 2) of a height each
                    slack = 0.0 if cutoff is None else n_walkers * HEIGHT * math.exp(-0.5 * cutoff * cutoff)
                    assert agree[name] <= 1e-12 * (state["sum_heights"] + float(start.abs().max())) + slack, (name, agree[name])
                    assert state["hills"] == n_walkers and state["refused"] == 0, (name, state)
                graphs = {name: captured(dev, fn, restore) for name, fn in (("fixed", fixed), ("diff", diff), ("geom", geom))}
                for name, fn in (("fixed", fixed), ("diff", diff), ("geom", geom)):
                    restore()
                    fn()
                    want = table.clone()
                    restore()
                    graphs[name].replay()
                    torch.cuda.synchronize()
                    assert torch.equal(table, want), "the replay and the eager step differ: %s" % name
                routes = [("fixed", fixed), ("fixed graph", graphs["fixed"].replay), ("diff", diff), ("diff graph", graphs["diff"].replay),
                          ("geom", geom), ("geom graph", graphs["geom"].replay), ("torch diff", torch_diff), ("torch geom", torch_geom)]
                t = {name: [] for name, _ in routes}
                for _ in range(args.rounds):
                    for name, fn in routes:
                        t[name].append(timed(fn, restore))
            m = {name: statistics.median(v) for name, v in t.items()}
            print("C3-head%d, table %s, cutoff %s, %d walkers, us per step: fixed %.1f (graph %.1f) | diff %.1f (graph %.1f), torch %.1f | "
                  "geom %.1f (graph %.1f), torch %.1f | diff/fixed %.2fx, geom/fixed %.2fx, torch/diff %.2fx, torch/geom %.2fx; routes agree to "
                  "%.1e, %.1e" % (d, "x".join(str(n) for n in shape), cutoff, n_walkers, m["fixed"], m["fixed graph"], m["diff"], m["diff graph"],
                                  m["torch diff"], m["geom"], m["geom graph"], m["torch geom"], m["diff"] / m["fixed"], m["geom"] / m["fixed"],
                                  m["torch diff"] / m["diff"], m["torch geom"] / m["geom"], agree["diff"], agree["geom"]), flush=True)


if __name__ == "__main__":
    main()
