#!/usr/bin/env python3
"""Forward mode: the tangent kernel (molann_features_jvp_f32, one tangent, features written too) and torch.func.jvp(model, ...)
end to end against torch.func.jvp of the oracle on the same GPU, at C3, C3p + [66,5,3] (the reference quickstart's Example 1),
P1 and C4.  HIP events, median of the timed repetitions after warm-up.  Algorithmic bytes: the touched atoms of x and of v read
once, f and df written once.  Kernel times for DESIGN.md come from a separate rocprofv3 --kernel-trace --stats run of this file."""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from molann_amd import workloads as wl
from molann_amd.ann import MolANN, create_sequential_nn
from oracle import molann_oracle as mo

COPY_TBPS = 6.29   # measured device-to-device copy rate
dev = torch.device("cuda:0")
CASES = (("C3", None, 1 << 20), ("C3p", [66, 5, 3], 1 << 20), ("P1", None, 1 << 17), ("C4", None, 2048))


def median_ms(fn, warm=5, reps=30):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def model_for(w, head):
    model = wl.build_model(w, dev)
    if head is not None:
        torch.manual_seed(0)
        model = MolANN(model if not isinstance(model, MolANN) else model.preprocessing_layer,
                       create_sequential_nn(head)).to(dev)
    return model


def oracle_fn(w, model):
    feats = [(t, [a - 1 for a in atoms]) for t, atoms in w.features]
    al = [a - 1 for a in w.align] if w.align is not None else None
    ref = mo.center_reference(torch.from_numpy(w.ref_xyz[al])).float().to(dev) if al else None
    lins = [m for m in model.ann_layers if isinstance(m, torch.nn.Linear)] if isinstance(model, MolANN) else []
    ws, bs = [l.weight.detach() for l in lins], [l.bias.detach() for l in lins]

    def f(x):
        h = mo.preprocessing_forward(x, feats, w.use_angle_value, al, ref)
        return mo.mlp_forward(h, ws, bs) if ws else h
    return f


for name, head, n in CASES:
    w = wl.get_workload(name)
    model = model_for(w, head)
    pp = model.preprocessing_layer if isinstance(model, MolANN) else model
    x = w.make_frames(n, seed=1).to(dev)
    v = torch.randn_like(x)
    torch.func.jvp(pp, (x[:4],), (v[:4],))                      # builds the feature plan
    plan = [e for e in pp._plans().values()][-1].plan
    f = torch.empty((n, plan.feature_dim), device=dev)
    df = torch.empty((1, n, plan.feature_dim), device=dev)
    v1 = v.unsqueeze(0)
    k_ms = median_ms(lambda: plan.features_jvp(x, v1, f, df))
    info = plan.last_launch_info()
    touched = set(a - 1 for _, atoms in w.features for a in atoms) | (set(a - 1 for a in w.align) if w.align else set())
    nbytes = n * (2 * len(touched) * 12 + 2 * plan.feature_dim * 4)
    e2e_ms = median_ms(lambda: torch.func.jvp(model, (x,), (v,)))
    of = oracle_fn(w, model)
    o_ms = median_ms(lambda: torch.func.jvp(of, (x,), (v,)), warm=2, reps=5)
    print(json.dumps({"workload": name + ("+%s" % head if head else ""), "frames": n, "kernel": info,
                      "kernel_ms": round(k_ms, 4), "alg_bytes": nbytes, "tbps": round(nbytes / k_ms / 1e9, 3),
                      "copy_fraction": round(nbytes / k_ms / 1e9 / COPY_TBPS, 3), "jvp_model_ms": round(e2e_ms, 4),
                      "jvp_oracle_ms": round(o_ms, 4)}))
