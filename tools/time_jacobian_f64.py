#!/usr/bin/env python3
"""Float64 values + the full Jacobian per call: molann_value_and_jacobian_f64's single launch (frames_value_jac_f64_kernel) against
the route it replaces, molann_value_and_vjp_f64 on `x.expand(d_out, ...)` with identity cotangents (frames_value_vjp_f64_kernel on
d_out copies of every frame), in the same process.

    python tools/time_jacobian_f64.py                      # host time per call (device-synchronised, warm) at 1 and 64 frames
    python tools/time_jacobian_f64.py --route expand       # only the expand route (it runs on a checkout without the new call)
    python tools/time_jacobian_f64.py --workload C3 --frames 131072 --reps 5 --route jacobian
                                                           # one batch: run under `rocprofv3 --kernel-trace --stats` for kernel time

C3 (22 atoms, [6, 32, 8]) and P1 (166 atoms, Kabsch on 42, 8 dihedrals, [16, 32, 8]) as `model.double()`."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from molann_amd import workloads as wl  # noqa: E402


def timed(fn, reps):
    for _ in range(min(20, reps)):
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
    ap.add_argument("--route", default="both", choices=["both", "jacobian", "expand"])
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for name in ([args.workload] if args.workload else ["C3", "P1"]):
        w = wl.get_workload(name)
        model = wl.build_model(w, dev).double().requires_grad_(False)
        d_out = w.out_dim()
        for n in ([args.frames] if args.frames else [1, 64]):
            x = w.make_frames(n, device=dev).double()
            res, infos = {}, []
            if args.route != "expand":
                y = torch.empty((n, d_out), dtype=torch.float64, device=dev)
                jac = torch.empty((n, d_out, w.n_atoms, 3), dtype=torch.float64, device=dev)

                def jacobian():
                    model.value_and_jacobian(x, into=(y, jac))

                jacobian()
                torch.cuda.synchronize()
                infos.append(model.last_launch_info())
                res["jacobian"] = timed(jacobian, args.reps)
            if args.route != "jacobian":
                # frame f's d_out copies are consecutive: dx.view(n, d_out, n_atoms, 3) is the Jacobian
                eye = torch.eye(d_out, dtype=torch.float64, device=dev).repeat(n, 1)
                ye = torch.empty((n * d_out, d_out), dtype=torch.float64, device=dev)
                dx = torch.empty((n * d_out, w.n_atoms, 3), dtype=torch.float64, device=dev)

                def expand():
                    xe = x.unsqueeze(1).expand(-1, d_out, -1, -1).reshape(n * d_out, w.n_atoms, 3)
                    model.value_and_vjp(xe, eye, into=(ye, dx))

                expand()
                torch.cuda.synchronize()
                infos.append(model.last_launch_info())
                res["expand"] = timed(expand, args.reps)
                if args.route == "both":
                    err = float((dx.view(n, d_out, w.n_atoms, 3) - jac).abs().max())
                    assert err <= 1e-12 * float(jac.abs().max()), err
            print("%s float64, %d frame(s), d_out %d: %s   [%s]" % (w.name, n, d_out, "  ".join("%s %.1f us" % kv for kv in res.items()),
                                                                   " | ".join(infos)), flush=True)


if __name__ == "__main__":
    main()
