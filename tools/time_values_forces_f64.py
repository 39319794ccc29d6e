#!/usr/bin/env python3
"""Float64 values + forces per call: molann_value_and_vjp_f64's single launch (frames_value_vjp_f64_kernel) against the eager
float64 path `torch.autograd.grad(model(xg), xg, dy)` (frames_f64_kernel, the head and its backward as ATen kernels,
frames_bwd_f64_kernel), in the same process.

    python tools/time_values_forces_f64.py                 # host time per call (device-synchronised, warm) at 1 and 64 frames
    python tools/time_values_forces_f64.py --workload C3 --frames 1048576 --reps 5 --single-only
                                                           # one batch: run under `rocprofv3 --kernel-trace --stats` for kernel time

C3 (22 atoms, [6, 32, 8]) and P1 (166 atoms, Kabsch on 42, 8 dihedrals, [16, 32, 8]) as `model.double()`."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from molann_amd import workloads as wl  # noqa: E402
from molann_amd.graph import GraphedForces  # noqa: E402


def timed(fn, reps):
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="", help="C3 or P1 instead of both")
    ap.add_argument("--frames", type=int, default=0, help="one batch size instead of 1 and 64")
    ap.add_argument("--reps", type=int, default=500)
    ap.add_argument("--single-only", action="store_true", help="only the single launch (for a kernel trace of a large batch)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in ([args.workload] if args.workload else ["C3", "P1"]):
        w = wl.get_workload(name)
        model = wl.build_model(w, dev).double().requires_grad_(False)
        for n in ([args.frames] if args.frames else [1, 64]):
            x = w.make_frames(n, device=dev).double()
            dy = torch.randn((n, w.out_dim()), generator=torch.Generator().manual_seed(1), dtype=torch.float64).to(dev)
            y, dx = torch.empty((n, w.out_dim()), dtype=torch.float64, device=dev), torch.empty_like(x)

            def single():
                model.value_and_vjp(x, dy, into=(y, dx))

            def eager():
                xg = x.detach().requires_grad_(True)
                return torch.autograd.grad(model(xg), xg, dy)

            single()
            torch.cuda.synchronize()
            info = model.last_launch_info()
            res = {"single": timed(single, args.reps)}
            if not args.single_only:
                res["eager"] = timed(eager, args.reps)
                if n <= 4096:
                    g = GraphedForces(model, x)
                    res["replay"] = timed(lambda: g.value_and_vjp(x, dy), args.reps)
            print("%s float64, %d frame(s): %s   [%s]" % (w.name, n, "  ".join("%s %.1f us" % kv for kv in res.items()), info), flush=True)


if __name__ == "__main__":
    main()
