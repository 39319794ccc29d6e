#!/usr/bin/env python3
"""A bias interpolated from a table on a float64 model per call: molann_value_and_grid_f64's single launch (frames_value_grid_f64_kernel)
against what a caller had before it, in the same process, alternating:

    (a)  grid         model.value_and_grid(x, table, lower, spacing, periodic, into=...)
    (a') grid (plan)  Plan.value_and_grid_f64 on the same buffers: the ctypes call without the module method's argument checks
    (b)  composed     y = model(x); the cubic-convolution interpolation and dV/dy with torch (indices, weights, a gather, einsum);
                      value_and_vjp(x, dV/dy)
    (c)  vjp, vjp'    value_and_vjp alone on a fixed cotangent, timed twice per round: their difference is the spread of the numbers
    (d)  hills        value_and_hills with 1000 and 10000 hills on the same plan and frames: what the table replaces in a long run

A PreprocessingANN has no value_and_vjp method: for the features-only case (b) and (c) call the ctypes plan (`Plan.value_and_vjp_f64`).

    python tools/time_grid_f64.py                          # host time per call (device-synchronised, warm, preallocated): 1, 64 and 65536
                                                           # frames; C3-angles and C3-head2 with tables of 64^2 and 512^2, C3-head3 with 64^3
    python tools/time_grid_f64.py --case C3-head2 --frames 1048576 --points 512 --reps 5 --kernels-only
                                                           # (a), (c) and (d, 1000 hills) on one batch: run under `rocprofv3 --kernel-trace
                                                           # --stats` for kernel time

C3-angles: the two C3 dihedrals as angle values, features only (PreprocessingANN), both axes periodic from -pi.  C3-head2 / C3-head3: C3's
preprocessing (22 atoms, 4 features) behind a [4, 32, 2] / [4, 32, 3] tanh head as `model.double()`, axis 0 periodic; the grid covers the
outputs of 4096 frames."""
import argparse
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from molann_amd import workloads as wl  # noqa: E402
from molann_amd.ann import MolANN, create_sequential_nn  # noqa: E402
from time_hills_f64 import c3_angles, timed  # noqa: E402

F64 = torch.float64


def interpolate(y, table, lower, spacing, periodic):
    """(V [N], dV/dy [N, d]) of the cubic-convolution interpolant with torch on y's device: the composition's middle part"""
    d = table.dim()
    idx, a, b = [], [], []
    for k in range(d):
        n, h = table.shape[k], spacing[k]
        u = (y[:, k] - lower[k]) / h
        if periodic[k]:
            u = u - n * torch.floor(u / n)
            i = torch.clamp(torch.floor(u), max=n - 1)
            s = 1.0 / h
        else:
            s = ((u >= 0) & (u <= n - 1)).to(F64) / h
            u = torch.clamp(u, 0, n - 1)
            i = torch.clamp(torch.floor(u), max=n - 2)
        t = u - i
        t2 = t * t
        j = i.long()[:, None] - 1 + torch.arange(4, device=y.device)[None, :]
        idx.append(j % n if periodic[k] else j.clamp(0, n - 1))
        a.append(torch.stack([((-t + 2) * t - 1) * t / 2, ((3 * t - 5) * t2 + 2) / 2, ((-3 * t + 4) * t + 1) * t / 2, (t - 1) * t2 / 2], dim=1))
        b.append(torch.stack([(-3 * t2 + 4 * t - 1) / 2, (9 * t2 - 10 * t) / 2, (-9 * t2 + 8 * t + 1) / 2, (3 * t2 - 2 * t) / 2], dim=1) * (s[:, None] if not periodic[k] else s))
    view = lambda t, k: t.reshape([t.shape[0]] + [4 if m == k else 1 for m in range(d)])       # noqa: E731
    sub = table[tuple(view(idx[k], k) for k in range(d))]
    letters = "ijl"[:d]
    eq = "n" + letters + "," + ",".join("n" + c for c in letters) + "->n"
    v = torch.einsum(eq, sub, *a)
    dv = torch.stack([torch.einsum(eq, sub, *[b[m] if m == k else a[m] for m in range(d)]) for k in range(d)], dim=1)
    return v, dv


def build(name, dev):
    if name == "C3-angles":
        w = c3_angles()
        return w, wl.build_model(w, dev).double().requires_grad_(False)
    w = wl.get_workload("C3")
    torch.manual_seed(11)
    base = wl.build_model(w, dev)
    model = MolANN(base.preprocessing_layer, create_sequential_nn([w.feature_dim(), 32, int(name[-1])], activation=torch.nn.Tanh())).to(dev)
    return w, model.double().requires_grad_(False)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="", help="C3-angles, C3-head2 or C3-head3 instead of all")
    ap.add_argument("--frames", type=int, default=0, help="one batch size instead of 1, 64 and 65536")
    ap.add_argument("--points", type=int, default=0, help="points per axis instead of 64 and 512 (64 only for C3-head3)")
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=5, help="rounds of (a), (c), (b), (c'), (a'), (d)")
    ap.add_argument("--kernels-only", action="store_true", help="only (a), (c) and (d) with 1000 hills, --reps calls each (for a kernel trace)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in ([args.case] if args.case else ["C3-angles", "C3-head2", "C3-head3"]):
        w, model = build(name, dev)
        whole = isinstance(model, MolANN)
        d = model.ann_layers[-1].out_features if whole else model.output_dimension()
        g = torch.Generator().manual_seed(1)
        with torch.no_grad():
            y_span = model(w.make_frames(4096, device=dev).double())
        for points in ([args.points] if args.points else ([64, 512] if d == 2 else [64])):
            shape = (points,) * d
            if whole:
                periodic = [True] + [False] * (d - 1)
                lo, hi = y_span.min(dim=0).values.tolist(), y_span.max(dim=0).values.tolist()
                spacing = [(hi[k] - lo[k]) / (points if periodic[k] else points - 1) for k in range(d)]
                lower = lo
            else:
                periodic, lower, spacing = [True] * d, [-math.pi] * d, [2.0 * math.pi / points] * d
            table = torch.randn(shape, generator=g, dtype=F64).to(dev)
            n_max = 10000
            centers = (y_span[torch.randint(0, 4096, (n_max,), generator=g).to(dev)] + 0.1 * torch.randn((n_max, d), generator=g, dtype=F64).to(dev)).contiguous()
            heights = (0.2 + torch.rand(n_max, generator=g, dtype=F64)).to(dev)
            sigma = torch.full((d,), 0.3, dtype=F64, device=dev)
            period = torch.tensor([points * spacing[k] if periodic[k] else 0.0 for k in range(d)], dtype=F64, device=dev)
            for n in ([args.frames] if args.frames else [1, 64, 65536]):
                big = n > (1 << 12)
                reps, rounds = (min(args.reps, 20), min(args.rounds, 3)) if big else (args.reps, args.rounds)
                x = w.make_frames(n, device=dev).double()
                dy = torch.randn((n, d), generator=g, dtype=F64).to(dev)
                y, v, dx = torch.empty((n, d), dtype=F64, device=dev), torch.empty(n, dtype=F64, device=dev), torch.empty_like(x)
                if whole:
                    plan = model.plan_for(x)
                    lins = [m for m in model.ann_layers if isinstance(m, torch.nn.Linear)]
                    W, B = [lin.weight.detach().contiguous() for lin in lins], [lin.bias.detach().contiguous() for lin in lins]
                    vjp_into = lambda cot: model.value_and_vjp(x, cot, into=(y, dx))  # noqa: E731
                    info = model.last_launch_info
                else:
                    model(x[:1].clone().requires_grad_(True))                         # makes the features plan and packs its float64 ref_x
                    plan = model._plans()[("features", dev.index)].plan
                    W, B = [], []
                    vjp_into = lambda cot: plan.value_and_vjp_f64(x, cot, [], [], y, dx)   # noqa: E731
                    info = plan.last_launch_info

                def grid():
                    model.value_and_grid(x, table, lower, spacing, periodic, into=(y, v, dx))

                def grid_plan():
                    plan.value_and_grid_f64(x, W, B, table, lower, spacing, periodic, y, v, dx)

                def composed():
                    with torch.no_grad():
                        bias, cot = interpolate(model(x), table, lower, spacing, periodic)
                    vjp_into(cot)
                    return bias

                def vjp():
                    vjp_into(dy)

                def hills(h):
                    return lambda: model.value_and_hills(x, centers[:h], heights[:h], sigma, period, into=(y, v, dx))

                with torch.cuda.device(dev):
                    grid()
                    torch.cuda.synchronize()
                    what = info()
                    if args.kernels_only:
                        for fn in (grid, vjp, hills(1000)):
                            for _ in range(args.reps):
                                fn()
                        torch.cuda.synchronize()
                        print("%s float64, %d frame(s), table %s: %d calls each of grid, vjp and hills (1000)   [%s]"
                              % (name, n, "x".join(str(s) for s in shape), args.reps, what), flush=True)
                        continue
                    v_new, dx_new = v.clone(), dx.clone()
                    v_old = composed()
                    torch.cuda.synchronize()
                    agree = float((v_new - v_old).abs().max()) / max(1.0, float(v_old.abs().max()))
                    agree_dx = float((dx_new - dx).abs().max()) / max(1e-3, float(dx.abs().max()))
                    things = [("grid", grid), ("vjp", vjp), ("composed", composed), ("vjp'", vjp), ("grid (plan)", grid_plan),
                              ("hills 1000", hills(1000))]
                    if not big:
                        things.append(("hills 10000", hills(10000)))
                    t = dict((key, []) for key, _ in things)
                    for _ in range(rounds):
                        for key, fn in things:
                            t[key].append(timed(fn, reps if not key.startswith("hills") else max(5, reps // 10)))
                med = dict((k, statistics.median(t_)) for k, t_ in t.items())
                print("%s float64, %d frame(s), table %s: %s   spread of vjp %.2f us, grid - vjp %+.2f us, bias agrees to %.1e, dx to %.1e   [%s]"
                      % (name, n, "x".join(str(s) for s in shape), "  ".join("%s %.1f us" % kv for kv in med.items()), abs(med["vjp"] - med["vjp'"]),
                         med["grid"] - min(med["vjp"], med["vjp'"]), agree, agree_dx, what), flush=True)


if __name__ == "__main__":
    main()
