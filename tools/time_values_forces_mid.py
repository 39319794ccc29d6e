#!/usr/bin/env python3
"""Values + forces of mid-size frames per call: molann_value_and_vjp_f32's single launch (molann_group_vjp) against GraphedForces'
two replays and the three chained ctypes launches (forward_train + mlp_backward + features_backward), all in the same process.

    python tools/time_values_forces_mid.py                 # host time per call (device-synchronised, warm) at 1 and 64 frames
    python tools/time_values_forces_mid.py --frames 1048576 --reps 5
                                                           # one batch: run under `rocprofv3 --kernel-trace --stats` for kernel time

P1 (166 atoms, Kabsch on 42, 8 dihedrals, [16, 32, 8]) and a P1 without alignment (see workloads())."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from molann_amd import workloads as wl  # noqa: E402
from molann_amd.graph import GraphedForces  # noqa: E402


def workloads():
    """P1, and a P1 without alignment with nine dihedrals (36 touched atoms: past the lane kernel's 32, so its features run on
    the wave-per-frame kernels and it has the three-launch backward; with P1's eight the lane kernel would fuse the head)."""
    p1 = wl.get_workload("P1")
    feats = [(wl.DIHEDRAL, tuple(range(s, s + 4))) for s in range(3, 163, 18)]
    na = wl.Workload("P1-noalign", p1.ref_xyz, feats, mlp_dims=[2 * len(feats), 32, 8], frames=p1.frames)
    return [p1, na]


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
    ap.add_argument("--frames", type=int, default=0, help="one batch size instead of 1 and 64")
    ap.add_argument("--reps", type=int, default=500)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for w in workloads():
        model = wl.build_model(w, dev).requires_grad_(False)
        for n in ([args.frames] if args.frames else [1, 64]):
            x = w.make_frames(n, device=dev)
            dy = torch.randn((n, w.out_dim()), generator=torch.Generator().manual_seed(1)).to(dev)
            plan = model.plan_for(x)
            y, dx = torch.empty((n, w.out_dim()), device=dev), torch.empty_like(x)
            f = torch.empty((n, plan.feature_dim), device=dev)
            gf = torch.empty_like(f)

            def single():
                plan.value_and_vjp(x, dy, y, dx)

            def three():
                plan.forward_train(x, y, f)
                plan.mlp_backward(f, dy, gf, None)
                plan.features_backward(x, gf, dx)

            single()
            torch.cuda.synchronize()
            info = plan.last_launch_info()
            res = {"single": timed(single, args.reps)}
            if plan.supports_backward():     # (a plan whose lane kernel fuses its head has no head backward of its own)
                res["three"] = timed(three, args.reps)
                if n <= 4096:
                    g = GraphedForces(model, x)

                    def replays():
                        g.graph.replay()
                        g.bwd_graph.replay()
                    res["replays"] = timed(replays, args.reps)
            res["module"] = timed(lambda: model.value_and_vjp(x, dy, into=(y, dx)), args.reps)
            print("%s, %d frame(s): %s   [%s]" % (w.name, n, "  ".join("%s %.1f us" % kv for kv in res.items()), info), flush=True)


if __name__ == "__main__":
    main()
