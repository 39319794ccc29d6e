#!/usr/bin/env python3
"""Float64 values + the metric tensor M = J W J^T per call: molann_value_and_metric_f64's single launch
(frames_value_metric_f64_kernel) against the route it replaces, value_and_jacobian followed by
torch.einsum("fkai,a,flai->fkl", jac, w, jac), on the same frames in one process.  HIP events, the median of 20 calls after 5
warm-up calls; the peak allocated bytes of each route (torch.cuda.max_memory_allocated, x and the weights included).

    python tools/time_metric.py                  # C3 at 1 M frames, P1 at 128 K, C4 at 2048, C3p + [66, 5, 3] at 1 M,
                                                 # C2 + [3, 32, 16] at 1 M (16 outputs)
    python tools/time_metric.py --case P1 --frames 4096"""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from molann_amd import workloads as wl  # noqa: E402
from molann_amd.ann import MolANN, create_sequential_nn  # noqa: E402

CASES = [("C3", 1 << 20), ("P1", 1 << 17), ("C4", 2048), ("C3p+[66,5,3]", 1 << 20),
         ("C2+[3,32,16]", 1 << 20)]   # the last one: 16 outputs, two chunks and four strips (the recomputed rows)
EINSUM = "fkai,a,flai->fkl"


def build(name, dev):
    w = wl.get_workload(name.split("+")[0])
    model = wl.build_model(w, dev)
    if "+" in name:                                        # a features-only workload with the head named behind the +
        dims = [int(v) for v in name.split("+")[1].strip("[]").split(",")]
        assert dims[0] == w.feature_dim(), (dims, w.feature_dim())
        torch.manual_seed(11)
        model = MolANN(model, create_sequential_nn(dims)).to(dev)
    return w, model.double().requires_grad_(False)


def measure(fn, warmup=5, calls=20):
    """(median ms, peak allocated bytes) of fn"""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return sorted(ms)[len(ms) // 2], torch.cuda.max_memory_allocated()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", default="", help="one of %s" % ", ".join(c for c, _ in CASES))
    ap.add_argument("--frames", type=int, default=0)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    for name, n in CASES:
        if args.case and args.case != name:
            continue
        n = args.frames or n
        w, model = build(name, dev)
        x = w.make_frames(n, device=dev).double()
        wt = 0.05 + 1.95 * torch.rand(w.n_atoms, dtype=torch.float64, device=dev)
        res = {}

        def metric():
            res["metric"] = model.value_and_metric(x, weights=wt)

        def route():
            y, jac = model.value_and_jacobian(x)
            res["route"] = (y, torch.einsum(EINSUM, jac, wt, jac))

        t_m, b_m = measure(metric)
        info = model.last_launch_info()
        (y, M), res = res["metric"], {}
        torch.cuda.empty_cache()
        t_r, b_r = measure(route)
        assert torch.equal(y, res["route"][0])
        scale = float(torch.diagonal(M, dim1=1, dim2=2).abs().max())
        err = float((M - res["route"][1]).abs().max())
        assert err <= 1e-11 * scale, (err, scale)
        print("%s float64, %d frames, d_out %d: value_and_metric %.3f ms, peak %.1f MB | value_and_jacobian + einsum %.3f ms, peak %.1f MB"
              "   [%s]" % (name, n, y.shape[1], t_m, b_m / 1e6, t_r, b_r / 1e6, info), flush=True)
        del res, y, M, x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
