#!/usr/bin/env python3
"""An OPES term with walls and a table on chosen outputs of a float64 model per call: molann_value_and_bias_opes_f64's single launch
(frames_value_bias_opes_f64_kernel) against the calls it replaces, in the same process, alternating:

    (a)  bias r+o       model.value_and_bias(x, restraint=walls, opes=..., into=...)
    (a') bias r+o+g     the same with the table as well
    (b)  restraint, opes, grid   value_and_restraint, value_and_opes and value_and_grid on the same frames, each on its own, where the
                        single entry serves the model at all; "r+o" and "r+o+g" are the sums of their medians: the calls (a) and (a')
                        replace, back to back
    (c)  opes, vjp, vjp'   value_and_opes alone (where it serves the model) and value_and_vjp alone on a fixed cotangent, timed twice per
                        round: their difference is the spread of the numbers

    python tools/time_bias_opes_f64.py                     # host time per call (device-synchronised, warm, preallocated): 1, 64 and 65536
                                                           # frames with 0, 100 and 1000 kernels at cutoff 4; C3-head2, C3 and P1
    python tools/time_bias_opes_f64.py --case C3 --frames 64 --kernels 1000

C3-head2: C3's preprocessing behind a [d_feat, 32, 2] tanh head; OPES and the table on both outputs, walls on both, so all three single
entries serve it.  C3, P1: the workloads' own models with 8 outputs; walls on all, OPES on (0, 3, 7), the table (64 x 64, axis 0
periodic) on (6, 1): value_and_grid refuses these models and value_and_opes would act on all 8 outputs, so of (b) only the restraint
runs and no sum is formed."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from molann_amd.bias import Grid, Opes, Restraint  # noqa: E402
from time_bias_f64 import build  # noqa: E402
from time_hills_f64 import timed  # noqa: E402

F64 = torch.float64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="", help="C3-head2, C3 or P1 instead of all")
    ap.add_argument("--frames", type=int, default=0, help="one batch size instead of 1, 64 and 65536")
    ap.add_argument("--kernels", type=int, default=-1, help="one table size instead of 0, 100 and 1000")
    ap.add_argument("--points", type=int, default=64, help="points per axis of the table")
    ap.add_argument("--cutoff", type=float, default=4.0)
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=5, help="rounds of (a), (c), (b), (c'), (a')")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    scale, epsilon = 2.25, 1e-3
    for name in ([args.case] if args.case else ["C3-head2", "C3", "P1"]):
        w, model, oc, gc = build(name, dev)
        d = model.ann_layers[-1].out_features
        served = oc is None
        ocols, gcols = list(oc or range(d)), list(gc or range(d))
        g = torch.Generator().manual_seed(1)
        with torch.no_grad():
            y_span = model(w.make_frames(4096, device=dev).double())
        lo, hi = y_span.min(dim=0).values, y_span.max(dim=0).values
        periodic = [True, False]
        spacing = [float(hi[k] - lo[k]) / (args.points if per else args.points - 1) for k, per in zip(gcols, periodic)]
        lower = [float(lo[k]) for k in gcols]
        table = torch.randn((args.points,) * 2, generator=g, dtype=F64).to(dev)
        most = max(args.kernels, 1000)
        pick = torch.randint(0, 4096, (most,), generator=g).to(dev)
        spread = y_span[:, ocols].std(dim=0)
        all_centers = (y_span[pick][:, ocols] + 0.1 * spread * torch.randn((most, len(ocols)), generator=g, dtype=F64).to(dev)).contiguous()
        all_heights = (0.2 + torch.rand(most, generator=g, dtype=F64)).to(dev)
        sigma = (0.3 * spread).contiguous()
        # walls: a flat bottom that holds most of the outputs' range, stiff beyond it
        center, kappa = y_span.mean(dim=0).contiguous(), torch.full((d,), 50.0, dtype=F64, device=dev)
        flat = (1.5 * y_span.std(dim=0)).contiguous()
        R, G = Restraint(center, kappa, flat=flat), Grid(table, lower, spacing, periodic, columns=gc)
        for n in ([args.frames] if args.frames else [1, 64, 65536]):
            big = n > (1 << 12)
            reps, rounds = (min(args.reps, 20), min(args.rounds, 3)) if big else (args.reps, args.rounds)
            x = w.make_frames(n, device=dev).double()
            dy = torch.randn((n, d), generator=g, dtype=F64).to(dev)
            y, v, e, dx = (torch.empty(s, dtype=F64, device=dev) for s in ((n, d), (n,), (n, 4), (n, w.n_atoms, 3)))
            for n_kernels in ([args.kernels] if args.kernels >= 0 else [0, 100, 1000]):
                centers, heights = all_centers[:n_kernels], all_heights[:n_kernels]
                norm = 0.02 * max(float(heights.sum()), 1.0)
                O = Opes(centers, heights, sigma, scale, norm, epsilon, args.cutoff, columns=oc)

                def bias_ro():
                    model.value_and_bias(x, restraint=R, opes=O, into=(y, e, dx))

                def bias_rog():
                    model.value_and_bias(x, restraint=R, grid=G, opes=O, into=(y, e, dx))

                def vjp():
                    model.value_and_vjp(x, dy, into=(y, dx))

                def restraint():
                    model.value_and_restraint(x, center, kappa, flat=flat, into=(y, v, dx))

                def grid():
                    model.value_and_grid(x, table, lower, spacing, periodic, into=(y, v, dx))

                def opes():
                    model.value_and_opes(x, centers, heights, sigma, scale, norm, epsilon, args.cutoff, into=(y, v, dx))

                with torch.cuda.device(dev):
                    bias_ro()
                    torch.cuda.synchronize()
                    what = model.last_launch_info()
                    agree = ""
                    if served:      # the single calls' energies, and the sum of their gradients
                        bias_rog()
                        e_new, dx_new = e.clone(), dx.clone()
                        e_old, dx_old = torch.zeros_like(e), torch.zeros_like(dx)
                        for c, fn in ((0, restraint), (3, opes), (2, grid)):
                            fn()
                            e_old[:, c], dx_old = v, dx_old + dx
                        torch.cuda.synchronize()
                        agree = ", energies equal the single calls': %s, dx agrees to %.1e" % (
                            bool(torch.equal(e_new, e_old)), float((dx_new - dx_old).abs().max()) / max(1e-3, float(dx_old.abs().max())))
                    things = [("bias r+o", bias_ro), ("vjp", vjp), ("restraint", restraint)] + ([("opes", opes), ("grid", grid)] if served else []) + \
                        [("vjp'", vjp), ("bias r+o+g", bias_rog)]
                    t = dict((key, []) for key, _ in things)
                    for _ in range(rounds):
                        for key, fn in things:
                            t[key].append(timed(fn, reps))
                med = dict((k, statistics.median(t_)) for k, t_ in t.items())
                line = "  ".join("%s %.1f us" % kv for kv in med.items())
                if served:
                    line += "  restraint + opes %.1f us  restraint + opes + grid %.1f us" % (med["restraint"] + med["opes"],
                                                                                             med["restraint"] + med["opes"] + med["grid"])
                print("%s float64, %d frame(s), %d kernels, cutoff %s, table %dx%d: %s   spread of vjp %.2f us, bias r+o - vjp %+.2f us%s   [%s]"
                      % (name, n, n_kernels, args.cutoff, args.points, args.points, line, abs(med["vjp"] - med["vjp'"]),
                         med["bias r+o"] - min(med["vjp"], med["vjp'"]), agree, what), flush=True)


if __name__ == "__main__":
    main()
