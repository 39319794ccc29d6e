#!/usr/bin/env python3
"""A harmonic restraint on a float64 model per call: molann_value_and_restraint_f64's single launch (frames_value_restraint_f64_kernel)
against what a caller had before it, in the same process, alternating:

    (a) restraint    model.value_and_restraint(x, center, kappa, period, into=...)
    (b) composed     y = model(x); d = y - center (wrapped with torch where periodic); value_and_vjp(x, kappa * d) and the energy with torch
    (c) vjp, vjp'    value_and_vjp alone on a fixed cotangent, timed twice per round: their difference is the spread of the numbers

A PreprocessingANN has no value_and_vjp method: for the features-only case (b) and (c) call the ctypes plan (`Plan.value_and_vjp_f64`), which
skips the module method's argument checks, so that case also times (a') `Plan.value_and_restraint_f64`, the like-for-like partner of (c).

    python tools/time_restraint_f64.py                     # host time per call (device-synchronised, warm, preallocated) at 1 and 64 frames
    python tools/time_restraint_f64.py --case C3 --frames 1048576 --reps 5 --kernels-only
                                                           # (a) and (c) on one batch: run under `rocprofv3 --kernel-trace --stats` for kernel time

C3 (22 atoms, [6, 32, 8]) and P1 (166 atoms, Kabsch on 42, 8 dihedrals, [16, 32, 8]) as `model.double()`, every second output periodic;
C3-angles: the two C3 dihedrals as angle values, features only (PreprocessingANN), period 2 pi."""
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
    for _ in range(20):
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
    ap.add_argument("--case", default="", help="C3, P1 or C3-angles instead of all three")
    ap.add_argument("--frames", type=int, default=0, help="one batch size instead of 1 and 64")
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--rounds", type=int, default=5, help="rounds of (a), (c), (b), (c')")
    ap.add_argument("--kernels-only", action="store_true", help="only (a) and (c), --reps calls each (for a kernel trace of a large batch)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in ([args.case] if args.case else ["C3", "P1", "C3-angles"]):
        w = c3_angles() if name == "C3-angles" else wl.get_workload(name)
        model = wl.build_model(w, dev).double().requires_grad_(False)
        whole = isinstance(model, MolANN)
        d = w.out_dim() if whole else model.output_dimension()
        period = torch.full((d,), 2.0 * math.pi, dtype=torch.float64, device=dev)
        if whole:
            period[1::2] = 0.0
        periodic = period > 0
        p_safe = torch.where(periodic, period, torch.ones_like(period))
        kappa = torch.linspace(0.5, 2.0, d, dtype=torch.float64, device=dev)
        for n in ([args.frames] if args.frames else [1, 64]):
            x = w.make_frames(n, device=dev).double()
            g = torch.Generator().manual_seed(1)
            center = torch.randn((n, d), generator=g, dtype=torch.float64).to(dev)
            dy = torch.randn((n, d), generator=g, dtype=torch.float64).to(dev)
            y, e, dx = torch.empty((n, d), dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev), torch.empty_like(x)
            if whole:
                forward = lambda: model(x)                                        # noqa: E731
                vjp_into = lambda cot: model.value_and_vjp(x, cot, into=(y, dx))  # noqa: E731
                info = model.last_launch_info
            else:
                model(x[:1].clone().requires_grad_(True))                         # makes the features plan and packs its float64 ref_x
                plan = model._plans()[("features", dev.index)].plan
                forward = lambda: model(x)                                        # noqa: E731
                vjp_into = lambda cot: plan.value_and_vjp_f64(x, cot, [], [], y, dx)   # noqa: E731
                info = plan.last_launch_info

            def restraint_plan():
                plan.value_and_restraint_f64(x, [], [], center, kappa, period, None, y, e, dx)

            def restraint():
                model.value_and_restraint(x, center, kappa, period, into=(y, e, dx))

            def composed():
                with torch.no_grad():
                    dd = forward() - center
                    dd = torch.where(periodic, dd - p_safe * torch.round(dd / p_safe), dd)
                    cot = kappa * dd
                    energy = 0.5 * (cot * dd).sum(dim=1)
                vjp_into(cot)
                return energy

            def vjp():
                vjp_into(dy)

            with torch.cuda.device(dev):
                restraint()
                torch.cuda.synchronize()
                what = info()
                if args.kernels_only:
                    for fn in (restraint, vjp):
                        for _ in range(args.reps):
                            fn()
                    torch.cuda.synchronize()
                    print("%s float64, %d frame(s): %d calls each of restraint and vjp   [%s]" % (name, n, args.reps, what), flush=True)
                    continue
                e_new = e.clone()
                e_old = composed()
                torch.cuda.synchronize()
                agree = float((e_new - e_old).abs().max()) / max(1.0, float(e_old.abs().max()))
                things = [("restraint", restraint), ("vjp", vjp), ("composed", composed), ("vjp'", vjp)]
                if not whole:
                    things.append(("restraint (plan)", restraint_plan))
                t = dict((key, []) for key, _ in things)
                for _ in range(args.rounds):
                    for key, fn in things:
                        t[key].append(timed(fn, args.reps))
            med = dict((k, statistics.median(v)) for k, v in t.items())
            print("%s float64, %d frame(s): %s   spread of vjp %.2f us, restraint - vjp %+.2f us, energies agree to %.1e   [%s]"
                  % (name, n, "  ".join("%s %.1f us" % kv for kv in med.items()), abs(med["vjp"] - med["vjp'"]),
                     med.get("restraint (plan)", med["restraint"]) - min(med["vjp"], med["vjp'"]), agree, what), flush=True)


if __name__ == "__main__":
    main()
