#!/usr/bin/env python3
"""A metadynamics bias (a sum of Gaussian hills) on a float64 model per call: molann_value_and_hills_f64's single launch
(frames_value_hills_f64_kernel) against what a caller had before it, in the same process, alternating:

    (a) hills        model.value_and_hills(x, centers[:H], heights[:H], sigma, period, into=...)
    (b) composed     y = model(x); the [N, H, d] differences (wrapped with torch where periodic), the hill sum and dV/dy with torch;
                     value_and_vjp(x, dV/dy)
    (c) vjp, vjp'    value_and_vjp alone on a fixed cotangent, timed twice per round: their difference is the spread of the numbers

A PreprocessingANN has no value_and_vjp method: for the features-only case (b) and (c) call the ctypes plan (`Plan.value_and_vjp_f64`), which
skips the module method's argument checks, so that case also times (a') `Plan.value_and_hills_f64`, the like-for-like partner of (c).

    python tools/time_hills_f64.py                         # host time per call (device-synchronised, warm, preallocated): 1 and 64 frames with
                                                           # 0, 100, 1000 and 10000 hills, then C3 at 65536 frames with 1000 hills
    python tools/time_hills_f64.py --case C3 --frames 65536 --hills 10000 --reps 5 --kernels-only
                                                           # (a) and (c) on one batch: run under `rocprofv3 --kernel-trace --stats` for kernel time

C3 (22 atoms, [6, 32, 8]) as `model.double()`, every second output periodic; C3-angles: the two C3 dihedrals as angle values, features only
(PreprocessingANN), period 2 pi.  One row of widths for all hills."""
import argparse
import math
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from molann_amd import workloads as wl  # noqa: E402
from molann_amd.ann import MolANN  # noqa: E402


def timed(fn, reps):
    for _ in range(min(20, reps)):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


def c3_angles():
    """C3's alignment and its two dihedrals as angle values: a features-only workload (a PreprocessingANN)."""
    c3 = wl.get_workload("C3")
    return wl.Workload("C3-angles", c3.ref_xyz, [f for f in c3.features if f[0] == wl.DIHEDRAL][:2], align=c3.align, use_angle_value=True,
                       rigid_motion=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="", help="C3 or C3-angles instead of both")
    ap.add_argument("--frames", type=int, default=0, help="one batch size instead of 1, 64 (and 65536 on C3)")
    ap.add_argument("--hills", type=int, default=-1, help="one table size instead of 0, 100, 1000, 10000")
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=5, help="rounds of (a), (c), (b), (c')")
    ap.add_argument("--kernels-only", action="store_true", help="only (a) and (c), --reps calls each (for a kernel trace of a large batch)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in ([args.case] if args.case else ["C3", "C3-angles"]):
        w = c3_angles() if name == "C3-angles" else wl.get_workload(name)
        model = wl.build_model(w, dev).double().requires_grad_(False)
        whole = isinstance(model, MolANN)
        d = w.out_dim() if whole else model.output_dimension()
        period = torch.full((d,), 2.0 * math.pi, dtype=torch.float64, device=dev)
        if whole:
            period[1::2] = 0.0
        periodic = period > 0
        p_safe = torch.where(periodic, period, torch.ones_like(period))
        g = torch.Generator().manual_seed(1)
        table = torch.randn((10000, d), generator=g, dtype=torch.float64).to(dev)          # the caller's preallocated table: prefixes of it
        weight = (0.2 + torch.rand(10000, generator=g, dtype=torch.float64)).to(dev)
        sigma = torch.linspace(0.3, 0.6, d, dtype=torch.float64, device=dev)
        sizes = [(args.frames, h) for h in ([args.hills] if args.hills >= 0 else [0, 100, 1000, 10000])] if args.frames else \
            [(n, h) for n in (1, 64) for h in ([args.hills] if args.hills >= 0 else [0, 100, 1000, 10000])] + ([(65536, 1000)] if whole else [])
        for n, n_hills in sizes:
            big = n * max(n_hills, 1) > (1 << 22)
            reps, rounds = (min(args.reps, 5), min(args.rounds, 3)) if big else (args.reps, args.rounds)
            x = w.make_frames(n, device=dev).double()
            centers, heights = table[:n_hills], weight[:n_hills]
            dy = torch.randn((n, d), generator=g, dtype=torch.float64).to(dev)
            y, v, dx = torch.empty((n, d), dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev), torch.empty_like(x)
            if whole:
                vjp_into = lambda cot: model.value_and_vjp(x, cot, into=(y, dx))  # noqa: E731
                info = model.last_launch_info
            else:
                model(x[:1].clone().requires_grad_(True))                         # makes the features plan and packs its float64 ref_x
                plan = model._plans()[("features", dev.index)].plan
                vjp_into = lambda cot: plan.value_and_vjp_f64(x, cot, [], [], y, dx)   # noqa: E731
                info = plan.last_launch_info

            def hills_plan():
                plan.value_and_hills_f64(x, [], [], centers, heights, sigma, period, y, v, dx)

            def hills():
                model.value_and_hills(x, centers, heights, sigma, period, into=(y, v, dx))

            def composed():
                with torch.no_grad():
                    dd = model(x)[:, None, :] - centers[None, :, :]
                    dd = torch.where(periodic, dd - p_safe * torch.round(dd / p_safe), dd)
                    s = dd / sigma
                    gh = heights * torch.exp(-0.5 * (s * s).sum(dim=2))
                    bias = gh.sum(dim=1)
                    cot = -(gh[:, :, None] * s / sigma).sum(dim=1)
                vjp_into(cot)
                return bias

            def vjp():
                vjp_into(dy)

            with torch.cuda.device(dev):
                hills()
                torch.cuda.synchronize()
                what = info()
                if args.kernels_only:
                    for fn in (hills, vjp):
                        for _ in range(args.reps):
                            fn()
                    torch.cuda.synchronize()
                    print("%s float64, %d frame(s), %d hills: %d calls each of hills and vjp   [%s]" % (name, n, n_hills, args.reps, what), flush=True)
                    continue
                v_new, dx_new = v.clone(), dx.clone()
                v_old = composed()
                torch.cuda.synchronize()
                agree = float((v_new - v_old).abs().max()) / max(1.0, float(v_old.abs().max()))
                agree_dx = float((dx_new - dx).abs().max()) / max(1e-3, float(dx.abs().max()))
                things = [("hills", hills), ("vjp", vjp), ("composed", composed), ("vjp'", vjp)]
                if not whole:
                    things.append(("hills (plan)", hills_plan))
                t = dict((key, []) for key, _ in things)
                for _ in range(rounds):
                    for key, fn in things:
                        t[key].append(timed(fn, reps))
            med = dict((k, statistics.median(t_)) for k, t_ in t.items())
            per_pair = (med["hills"] - min(med["vjp"], med["vjp'"])) * 1e3 / (n * n_hills) if n_hills else 0.0
            print("%s float64, %d frame(s), %d hills: %s   spread of vjp %.2f us, hills - vjp %+.2f us (%.3f ns per frame and hill), bias agrees to %.1e, "
                  "dx to %.1e   [%s]"
                  % (name, n, n_hills, "  ".join("%s %.1f us" % kv for kv in med.items()), abs(med["vjp"] - med["vjp'"]),
                     med.get("hills (plan)", med["hills"]) - min(med["vjp"], med["vjp'"]), per_pair, agree, agree_dx, what), flush=True)


if __name__ == "__main__":
    main()
