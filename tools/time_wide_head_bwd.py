#!/usr/bin/env python3
"""Head forward + backward of wide fp32 heads: the HIP head node (molann_mlp_packed_f32 + molann_mlp_backward_f32, i.e.
molann_mlp_chain / molann_chain_bwd) against the torch composition it replaces (ann_layers under autograd: rocBLAS GEMMs and
ATen activations), on features already in device memory.  Two cases each: gradients for the features and the parameters
(a forces / training step with x-gradients), and parameter gradients only (x is data).
   python tools/time_wide_head_bwd.py [--reps R]      (also under rocprofv3 --kernel-trace --stats -- python ...)
One JSON line per shape and case: times in us per call (median of R timed calls after warm-up, HIP events), and the backward
kernel's alone with its achieved TFLOP/s (useful flops: the hidden layers' recompute, W^T delta where used, dW)."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from molann_amd import workloads as wl
from molann_amd.ann import MolANN, create_sequential_nn

SHAPES = [([6, 64, 64, 8], 1 << 20), ([66, 5, 3], 1 << 20), ([126, 64, 32, 2], 1 << 20), ([85, 128, 64, 8], 262144)]


def median_us(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for dims, n in SHAPES:
        w = wl.get_workload({6: "C3", 66: "C3p", 126: "P2", 85: "C4"}[dims[0]])    # a preprocessing that gives dims[0] features
        base = wl.build_model(w, dev)
        pp = base.preprocessing_layer if isinstance(base, MolANN) else base
        torch.manual_seed(0)
        model = MolANN(pp, create_sequential_nn(dims).to(dev))
        plan = model.plan_for(w.make_frames(4, seed=1).to(dev))
        assert plan.supports_mlp_backward(), dims
        f = torch.randn((n, dims[0]), generator=torch.Generator().manual_seed(1)).to(dev)
        g = torch.randn((n, dims[-1]), generator=torch.Generator().manual_seed(2)).to(dev)
        out = torch.empty((n, dims[-1]), device=dev)
        gf = torch.empty_like(f)
        gp = torch.zeros(plan.grad_params_size(), device=dev)
        params = list(model.ann_layers.parameters())
        jk = [dims[l] * dims[l + 1] for l in range(len(dims) - 1)]
        for case, want_f in (("x_and_params", True), ("params_only", False)):
            def hip():
                plan.mlp_packed(f, out)
                gp.zero_()
                plan.mlp_backward(f, g, gf if want_f else None, gp)

            def bwd_only():
                plan.mlp_backward(f, g, gf if want_f else None, gp)

            fr = f.detach().requires_grad_(want_f)

            def composition():
                y = model.ann_layers(fr)
                torch.autograd.grad(y, ([fr] if want_f else []) + params, g)

            t_hip = median_us(hip, args.reps)
            t_bwd = median_us(bwd_only, args.reps)
            info = plan.last_launch_info()
            t_torch = median_us(composition, args.reps)
            flops = 2.0 * n * (sum(jk[:-1]) + sum(jk) + sum(jk[1:]) + (jk[0] if want_f else 0))
            print(json.dumps({"head": dims, "frames": n, "case": case, "hip_fwd_bwd_us": round(t_hip, 1),
                              "torch_fwd_bwd_us": round(t_torch, 1), "speedup": round(t_torch / t_hip, 2),
                              "chain_bwd_us": round(t_bwd, 1), "chain_bwd_tflops": round(flops / t_bwd * 1e-6, 1),
                              "kernel": info}), flush=True)


if __name__ == "__main__":
    main()
