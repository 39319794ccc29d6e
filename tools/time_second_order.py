#!/usr/bin/env python3
"""Second order of the float64 features: the exact kernel (molann_features_hvp_f64, one launch) against the four-launch
central-difference composition it replaces in the double-backward nodes (features_backward_f64 and features_f64 at x +- h u, plus
ATen elementwise work), called directly, at C3, P1, A5 and C4; and one full loss-on-forces step (E = sum model(x) G, F = dE/dx
with create_graph=True, L = |F|^2, L.backward()) of model.double() with the exact node and with the composition (the node's
fallback).  HIP events, median of 20 after 5 warm-up.  Kernel times for DESIGN.md come from a separate
rocprofv3 --kernel-trace --stats run of this file."""
import copy
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from molann_amd import _capi, ann
from molann_amd import workloads as wl
from oracle import molann_oracle as mo

dev = torch.device("cuda:0")
CASES = (("C3", 1 << 20), ("P1", 1 << 17), ("A5", 1 << 17), ("C4", 2048))
REPS = int(os.environ.get("MOLANN_TIME_REPS", "20"))


def median_ms(fn, warm=5, reps=REPS):
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


def plan_of(w):
    al = [a - 1 for a in w.align] if w.align else None
    ref = mo.center_reference(torch.from_numpy(w.ref_xyz[al])).float() if al else None
    feats = [(mo.POSITION, list(range(w.n_atoms)))] if w.kind == "align" else [(t, [a - 1 for a in s]) for t, s in w.features]
    plan = _capi.Plan(w.n_atoms, align_idx=al, ref_x=ref, features=feats, use_angle_value=w.use_angle_value)
    if ref is not None:
        plan.update_ref_f64(ref.double().to(dev).contiguous())
    return plan


def composition(plan, x, g, u, bufs):
    """what _FeatBackward64.backward did before the exact kernel: four launches and the difference arithmetic"""
    gxp, gxm, fp, fm = bufs
    xp, xm, inv = ann._difference_points(x, u)
    plan.features_backward_f64(xp, g, gxp)
    plan.features_backward_f64(xm, g, gxm)
    plan.features_f64(xp, fp)
    plan.features_f64(xm, fm)
    return (gxp - gxm) * inv, (fp - fm) * inv.view(-1, 1)


def loss_step(model, x, G):
    xg = x.detach().requires_grad_(True)
    (F,) = torch.autograd.grad((model(xg) * G).sum(), xg, create_graph=True)
    (F * F).sum().backward()


def unsupported(*a, **k):
    raise _capi.MolannHipError(_capi.E_UNSUPPORTED, "molann_features_hvp_f64")


for name, n in CASES:
    w = wl.get_workload(name)
    plan = plan_of(w)
    x = w.make_frames(n, seed=1).to(dev, torch.float64)
    g = torch.randn(n, plan.feature_dim, device=dev, dtype=torch.float64)
    u = torch.randn_like(x)
    hx, hg = torch.empty_like(x), torch.empty_like(g)
    bufs = (torch.empty_like(x), torch.empty_like(x), torch.empty_like(g), torch.empty_like(g))
    cd_ms = median_ms(lambda: composition(plan, x, g, u, bufs))
    k_ms = median_ms(lambda: plan.features_hvp_f64(x, g, u, hx, hg))
    info = plan.last_launch_info()
    del bufs
    model = copy.deepcopy(wl.build_model(w, dev)).double()
    if w.kind == "align":
        G = torch.randn_like(x)
    else:
        G = torch.randn(n, w.out_dim(), device=dev, dtype=torch.float64)
    step_ms = median_ms(lambda: loss_step(model, x, G))
    real = _capi.Plan.features_hvp_f64
    _capi.Plan.features_hvp_f64 = unsupported      # the node's fallback: the composition
    try:
        step_cd_ms = median_ms(lambda: loss_step(model, x, G))
    finally:
        _capi.Plan.features_hvp_f64 = real
    print(json.dumps({"workload": name, "frames": n, "kernel": info, "composition_ms": round(cd_ms, 4), "hvp_kernel_ms": round(k_ms, 4),
                      "loss_step_ms": round(step_ms, 4), "loss_step_composition_ms": round(step_cd_ms, 4)}), flush=True)
    del model, x, g, u, hx, hg, G
    torch.cuda.empty_cache()
