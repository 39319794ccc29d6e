#!/usr/bin/env python3
"""An OPES bias (the logarithm of a kernel density) on a float64 model per call: molann_value_and_opes_f64's single launch
(frames_value_opes_f64_kernel) against its neighbours, in the same process, alternating:

    (a) opes         model.value_and_opes(x, centers[:K], heights[:K], sigma, scale, norm, epsilon, cutoff, period, into=...)
    (b) hills        model.value_and_hills on the same table: the same walk without the cutoff and the transform
    (c) composed     the route (a) replaces: y = model(x); P with molann_amd.bias.opes_kernel_sum, its logarithm and dV/dy with torch;
                     value_and_vjp(x, dV/dy)

Times are HIP events around one call, the median of 20 calls after 5 warm-up calls, so they hold the launch and whatever the host
cannot hide behind the device.  A PreprocessingANN has no value_and_vjp method: for a features-only case (c) calls the ctypes plan.

    python tools/time_opes_f64.py                          # C3 (8 outputs), C3-angles (2 outputs) and P1: 1, 64 and 65536 frames with 0, 100,
                                                           # 1000 and 10000 kernels, cutoff None and 4
    python tools/time_opes_f64.py --case C3 --frames 64 --kernels 1000 --cutoff 4
    MOLANN_DIAG_LIB=1 python tools/time_opes_f64.py ...    # the same on libmolann_hip_diag.so (a build with another form of the walk, say):
                                                           # the operators always use the release library, so this goes through ctypes;
                                                           # compare it with a run of the release library under --ctypes

One row of widths for all kernels, every second output of a whole model periodic."""
import argparse
import math
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from molann_amd import ann, bias as mb, workloads as wl  # noqa: E402
from molann_amd.ann import MolANN  # noqa: E402


def timed(fn, calls=20, warmup=5):
    """the median of `calls` calls after `warmup`, each between two HIP events, in microseconds"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(calls):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        fn()
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop) * 1e3)
    return statistics.median(times)


def c3_angles():
    """C3's alignment and its two dihedrals as angle values: a features-only workload (a PreprocessingANN)."""
    c3 = wl.get_workload("C3")
    return wl.Workload("C3-angles", c3.ref_xyz, [f for f in c3.features if f[0] == wl.DIHEDRAL][:2], align=c3.align, use_angle_value=True,
                       rigid_motion=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="", help="C3, C3-angles or P1 instead of all three")
    ap.add_argument("--frames", type=int, default=0, help="one batch size instead of 1, 64, 65536")
    ap.add_argument("--kernels", type=int, default=-1, help="one table size instead of 0, 100, 1000, 10000")
    ap.add_argument("--cutoff", type=float, default=-1.0, help="one cutoff instead of none and 4 (0: none)")
    ap.add_argument("--rounds", type=int, default=3, help="rounds of (a), (b), (c); the median of the rounds' medians is printed")
    ap.add_argument("--ctypes", action="store_true", help="(a) and (b) through the ctypes plan, not the dispatcher operators")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.ctypes or os.environ.get("MOLANN_DIAG_LIB") == "1":
        ann._run_op = lambda: None
    for name in ([args.case] if args.case else ["C3", "C3-angles", "P1"]):
        w = c3_angles() if name == "C3-angles" else wl.get_workload(name)
        model = wl.build_model(w, dev).double().requires_grad_(False)
        whole = isinstance(model, MolANN)
        d = w.out_dim() if whole else model.output_dimension()
        if d > 8:
            print("%s: %d outputs, past the kernel's 8: skipped" % (name, d), flush=True)
            continue
        period = torch.full((d,), 2.0 * math.pi, dtype=torch.float64, device=dev)
        if whole:
            period[1::2] = 0.0
        g = torch.Generator().manual_seed(1)
        weight = (0.2 + torch.rand(10000, generator=g, dtype=torch.float64)).to(dev)
        # the caller's preallocated table, prefixes of it: kernels where a run deposits them, on the model's own outputs of 10000 other
        # frames, half a width of noise on each, the widths 0.3-0.6 of the outputs' spread (so a cutoff of 4 keeps some pairs and drops others)
        with torch.no_grad():
            visited = model(w.make_frames(10000, seed=3, device=dev).double())
        sigma = torch.linspace(0.3, 0.6, d, dtype=torch.float64, device=dev) * visited.std(dim=0)
        table = (visited + 0.5 * sigma * torch.randn((10000, d), generator=g, dtype=torch.float64).to(dev)).contiguous()
        scale, epsilon = 2.25, 1e-3
        for n in ([args.frames] if args.frames else [1, 64, 65536]):
            x = w.make_frames(n, device=dev).double()
            y, v, dx = torch.empty((n, d), dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.float64, device=dev), torch.empty_like(x)
            if whole:
                vjp_into = lambda cot: model.value_and_vjp(x, cot, into=(y, dx))  # noqa: E731
                info = model.last_launch_info
            else:
                model(x[:1].clone().requires_grad_(True))                         # makes the features plan and packs its float64 ref_x
                plan = model._plans()[("features", dev.index)].plan
                vjp_into = lambda cot: plan.value_and_vjp_f64(x, cot, [], [], y, dx)   # noqa: E731
                info = plan.last_launch_info
            for n_kernels in ([args.kernels] if args.kernels >= 0 else [0, 100, 1000, 10000]):
                centers, heights = table[:n_kernels], weight[:n_kernels]
                norm = 0.02 * max(float(heights.sum()), 1.0)
                for cutoff in ([args.cutoff if args.cutoff > 0 else None] if args.cutoff >= 0 else [None, 4.0]):
                    big = n * max(n_kernels, 1) > (1 << 26)         # the [N, K, d] temporaries of (c): past 4 GiB each, (c) is not timed

                    def opes():
                        model.value_and_opes(x, centers, heights, sigma, scale, norm, epsilon, cutoff, period, into=(y, v, dx))

                    def hills():
                        model.value_and_hills(x, centers, heights, sigma, period, into=(y, v, dx))

                    def composed():
                        with torch.no_grad():
                            yy = model(x).detach().requires_grad_(True)
                        with torch.enable_grad():
                            u = mb.opes_kernel_sum(yy, centers, heights, sigma, period, cutoff) / norm + epsilon
                            vv = scale * torch.log(u)
                            (cot,) = torch.autograd.grad(vv.sum(), yy, allow_unused=True) if n_kernels else (torch.zeros_like(yy),)
                        vjp_into(cot)
                        return vv.detach()

                    with torch.cuda.device(dev):
                        opes()
                        torch.cuda.synchronize()
                        what = info()
                        v_new, dx_new = v.clone(), dx.clone()
                        kept = float("nan")
                        if n_kernels and cutoff is not None:        # the share of (frame, kernel) pairs inside the cutoff, on 64 frames at most
                            dd = y[:64, None, :] - centers[None, :, :]
                            dd = torch.where(period > 0, dd - period * torch.round(dd / torch.where(period > 0, period, torch.ones_like(period))), dd)
                            kept = float((((dd / sigma) ** 2).sum(dim=2) < cutoff * cutoff).double().mean())
                        things = [("opes", opes), ("hills", hills)]
                        agree = agree_dx = float("nan")
                        if not big:
                            v_old = composed()
                            torch.cuda.synchronize()
                            agree = float((v_new - v_old).abs().max()) / max(1.0, float(v_old.abs().max()))
                            agree_dx = float((dx_new - dx).abs().max()) / max(1e-3, float(dx.abs().max()))
                            things.append(("composed", composed))
                        t = dict((key, []) for key, _ in things)
                        for _ in range(args.rounds):
                            for key, fn in things:
                                t[key].append(timed(fn))
                    med = dict((k, statistics.median(t_)) for k, t_ in t.items())
                    print("%s float64, %d frame(s), %d kernels, cutoff %s: %s   opes - hills %+.2f us, pairs inside the cutoff %.3f, bias agrees to %.1e, "
                          "dx to %.1e   [%s]" % (name, n, n_kernels, cutoff, "  ".join("%s %.1f us" % kv for kv in med.items()), med["opes"] - med["hills"],
                                                 kept, agree, agree_dx, what), flush=True)


if __name__ == "__main__":
    main()
