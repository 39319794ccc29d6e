#!/usr/bin/env python3
"""A restraint, hills and a tabulated bias on chosen outputs of a float64 model per call: molann_value_and_bias_f64's single launch
(frames_value_bias_f64_kernel) against the single-term calls it replaces, in the same process, alternating:

    (a)  bias r+g       model.value_and_bias(x, restraint, grid=..., into=...)
    (a') bias r+h+g     the same with 1000 hills as well
    (b)  restraint, grid, hills   value_and_restraint, value_and_grid and value_and_hills (1000 hills) on the same frames, each on
                        its own, where the single entry serves the model at all; "r+g" and "r+h+g" are the sums of their medians: the
                        calls (a) and (a') replace, back to back
    (c)  vjp, vjp'      value_and_vjp alone on a fixed cotangent, timed twice per round: their difference is the spread of the numbers

    python tools/time_bias_f64.py                          # host time per call (device-synchronised, warm, preallocated): 1, 64 and 65536
                                                           # frames; C3-head2, C3 and P1
    python tools/time_bias_f64.py --case C3 --frames 1048576 --reps 5 --kernels-only
                                                           # (a), (a') and (c) on one batch: run under `rocprofv3 --kernel-trace --stats`
                                                           # for kernel time

C3-head2: C3's preprocessing behind a [d_feat, 32, 2] tanh head; every term on both outputs, so all three single entries serve it.
C3, P1: the workloads' own models with 8 outputs; the restraint on all, the table (64 x 64, axis 0 periodic) on outputs (6, 1), the hills
on (0, 3, 7): value_and_grid refuses these models, and value_and_hills would act on all 8 outputs, so of (b) only the restraint runs."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from molann_amd import workloads as wl  # noqa: E402
from molann_amd.ann import MolANN, create_sequential_nn  # noqa: E402
from molann_amd.bias import Grid, Hills, Restraint  # noqa: E402
from time_hills_f64 import timed  # noqa: E402

F64 = torch.float64


def build(name, dev):
    """(workload, model, hills columns, grid columns); None columns: the identity, and the single entries serve the model"""
    w = wl.get_workload("C3" if name == "C3-head2" else name)
    torch.manual_seed(11)
    model = wl.build_model(w, dev)
    if name == "C3-head2":
        model = MolANN(model.preprocessing_layer, create_sequential_nn([w.feature_dim(), 32, 2], activation=torch.nn.Tanh())).to(dev)
        return w, model.double().requires_grad_(False), None, None
    return w, model.double().requires_grad_(False), (0, 3, 7), (6, 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="", help="C3-head2, C3 or P1 instead of all")
    ap.add_argument("--frames", type=int, default=0, help="one batch size instead of 1, 64 and 65536")
    ap.add_argument("--points", type=int, default=64, help="points per axis of the table")
    ap.add_argument("--hills", type=int, default=1000)
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=5, help="rounds of (a), (c), (b), (c'), (a')")
    ap.add_argument("--kernels-only", action="store_true", help="only (a), (a') and (c), --reps calls each (for a kernel trace)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in ([args.case] if args.case else ["C3-head2", "C3", "P1"]):
        w, model, hc, gc = build(name, dev)
        d = model.ann_layers[-1].out_features
        served = hc is None
        hcols, gcols = list(hc or range(d)), list(gc or range(d))
        g = torch.Generator().manual_seed(1)
        with torch.no_grad():
            y_span = model(w.make_frames(4096, device=dev).double())
        lo, hi = y_span.min(dim=0).values, y_span.max(dim=0).values
        periodic = [True, False]
        spacing = [float(hi[k] - lo[k]) / (args.points if per else args.points - 1) for k, per in zip(gcols, periodic)]
        lower = [float(lo[k]) for k in gcols]
        table = torch.randn((args.points,) * 2, generator=g, dtype=F64).to(dev)
        pick = torch.randint(0, 4096, (args.hills,), generator=g).to(dev)
        centers = (y_span[pick][:, hcols] + 0.1 * torch.randn((args.hills, len(hcols)), generator=g, dtype=F64).to(dev)).contiguous()
        heights = (0.2 + torch.rand(args.hills, generator=g, dtype=F64)).to(dev)
        sigma = torch.full((len(hcols),), 0.3, dtype=F64, device=dev)
        center, kappa = y_span.mean(dim=0).contiguous(), torch.full((d,), 2.0, dtype=F64, device=dev)
        R, H, G = Restraint(center, kappa), Hills(centers, heights, sigma, columns=hc), Grid(table, lower, spacing, periodic, columns=gc)
        for n in ([args.frames] if args.frames else [1, 64, 65536]):
            big = n > (1 << 12)
            reps, rounds = (min(args.reps, 20), min(args.rounds, 3)) if big else (args.reps, args.rounds)
            x = w.make_frames(n, device=dev).double()
            dy = torch.randn((n, d), generator=g, dtype=F64).to(dev)
            y, v, e, dx = (torch.empty(s, dtype=F64, device=dev) for s in ((n, d), (n,), (n, 3), (n, w.n_atoms, 3)))

            def bias_rg():
                model.value_and_bias(x, restraint=R, grid=G, into=(y, e, dx))

            def bias_rhg():
                model.value_and_bias(x, restraint=R, hills=H, grid=G, into=(y, e, dx))

            def vjp():
                model.value_and_vjp(x, dy, into=(y, dx))

            def restraint():
                model.value_and_restraint(x, center, kappa, into=(y, v, dx))

            def grid():
                model.value_and_grid(x, table, lower, spacing, periodic, into=(y, v, dx))

            def hills():
                model.value_and_hills(x, centers, heights, sigma, into=(y, v, dx))

            with torch.cuda.device(dev):
                bias_rg()
                torch.cuda.synchronize()
                what = model.last_launch_info()
                if args.kernels_only:
                    for fn in (bias_rg, bias_rhg, vjp):
                        for _ in range(args.reps):
                            fn()
                    torch.cuda.synchronize()
                    print("%s float64, %d frame(s): %d calls each of bias r+g, bias r+h+g (%d hills) and vjp   [%s]" % (name, n, args.reps, args.hills, what),
                          flush=True)
                    continue
                agree = ""
                if served:      # the sum of the single calls' energies and gradients
                    bias_rhg()
                    e_new, dx_new = e.clone(), dx.clone()
                    e_old, dx_old = torch.zeros_like(e), torch.zeros_like(dx)
                    for c, fn in enumerate((restraint, hills, grid)):
                        fn()
                        e_old[:, c], dx_old = v, dx_old + dx
                    torch.cuda.synchronize()
                    agree = ", energies equal the single calls': %s, dx agrees to %.1e" % (
                        bool(torch.equal(e_new, e_old)), float((dx_new - dx_old).abs().max()) / max(1e-3, float(dx_old.abs().max())))
                things = [("bias r+g", bias_rg), ("vjp", vjp), ("restraint", restraint)] + ([("grid", grid), ("hills", hills)] if served else []) + \
                    [("vjp'", vjp), ("bias r+h+g", bias_rhg)]
                t = dict((key, []) for key, _ in things)
                for _ in range(rounds):
                    for key, fn in things:
                        t[key].append(timed(fn, reps))
            med = dict((k, statistics.median(t_)) for k, t_ in t.items())
            line = "  ".join("%s %.1f us" % kv for kv in med.items())
            if served:
                line += "  restraint + grid %.1f us  restraint + grid + hills %.1f us" % (med["restraint"] + med["grid"], med["restraint"] + med["grid"] + med["hills"])
            print("%s float64, %d frame(s), table %dx%d, %d hills: %s   spread of vjp %.2f us, bias r+g - vjp %+.2f us%s   [%s]"
                  % (name, n, args.points, args.points, args.hills, line, abs(med["vjp"] - med["vjp'"]), med["bias r+g"] - min(med["vjp"], med["vjp'"]),
                     agree, what), flush=True)


if __name__ == "__main__":
    main()
