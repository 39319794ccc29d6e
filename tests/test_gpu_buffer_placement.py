"""Every entry point of the C ABI on the caller's own buffers: offset pointers inside guard bands (tests/placement.py).

include/molann_hip.h promises "any 4-byte aligned pointer works; 16-byte aligned pointers take the wide-load path" (8 bytes for the
float64 entries), and an MD engine hands the library pointers into the middle of its position and force arrays.  The kernels
branch on that placement ("Caller's buffers", has the table); every other test passes fresh torch allocations, which
are 256-byte aligned and have nothing next to them that a test looks at.

Per family of FAMILIES (a plan taken from a model built with test_gpu_random_backward.Case - or, for the head kernels, a plan made
the way test_gpu_mlp_chain.py makes one -, the environment switches that route it, and per entry point the kernel its launch
info must name), per frame size, per frame count of NS and per placement of the call's buffers:
  - the return code is 0 and the launch info names the expected kernel;
  - no guard band of any buffer was written, at either end;
  - every input is bit for bit what was put in;
  - every output is bit for bit that of the all-zero placement of the same call - loads and stores of another width do not change
    arithmetic.  The atomics family (MOLANN_BWD_ATOMICS=1) sums dL/dx with float atomics: held to the float64 oracle instead.
Once per family the all-zero placement is compared bit for bit to the same call on ordinary fresh tensors (the arena changes
nothing) and to float64 autograd through the oracle (the reference of the bitwise checks is anchored), at the tolerances of
test_gpu_angular_edges.py: float32 max(1e-5 of the scale for outputs, 5e-4 for gradients, 1e-4 for tangents, twice the error of
the oracle run in float32), float64 1e-10 / 1e-9, the second-order kernel 1e-12; the head kernels at those of
test_gpu_mlp_chain.py (fp32 1e-5, bf16 4e-3 against its bf16 emulation) and test_gpu_wide_head_backward.py (2e-4).

Refusals: every float32 entry with one pointer moved by 2 bytes, every float64 entry that test_gpu_f64_entry_contract.py does not
pin with one pointer (the W / b tensors included) moved by 4, returns E_ALIGNMENT, launches nothing and writes nothing.

An overrun lands in the arena's slack: the failure is an assertion.  Nothing here can fault by design."""

import copy
import ctypes
import re
import types
import zlib

import numpy as np
import pytest
import torch

import placement as pl
import test_gpu_angular_edges as tae
import test_gpu_far_frames as fft
import test_gpu_mlp_chain as tmc
import test_gpu_random_backward as rb
from molann_amd import _capi
from molann_amd import workloads as wl
from molann_amd.ann import MolANN, _PlanEntry
from oracle import molann_oracle as mo

pytestmark = pytest.mark.gpu
ANGLE, BOND, DIH, POS = wl.ANGLE, wl.BOND, wl.DIHEDRAL, wl.POSITION
F32, F64 = torch.float32, torch.float64
NS = (1, 63, 64, 65, 200, 581)          # a lone frame, both sides of a 64-frame tile, a short last tile, several tiles per block
PLACEMENTS = {F32: (0, 1, 2, 3, "mixedA", "mixedB"), F64: (0, 1, "mixedA", "mixedB")}      # element offsets from a 256-byte boundary
N_ANCHOR = 65                           # the frame count of the fresh-tensor and the oracle comparison
N_TANGENTS = 2
LANE, MID, LARGE, ALIGN_BIG = (20, 21, 22, 23), (164, 165, 166), (2000, 2001), (388, 389)   # frame bytes = 0, 12, 8, 4 (mod 16), ...
REACHED = set()                         # (family, entry) that passed
SEEN = []                               # every launch info

RING = r"frames_ring_kernel<ND=\d+,B=%d>"
FWD_ANY = r"frames_(ring|wave)_kernel<"
# family: (kind, frame sizes, position items, head widths after the features (the last one set per size) or None, environment,
#          {entry: launch-info pattern}).  kind: "model" (rb.Case), "align" (the AlignmentLayer alone), "head" (a plan for its head).
FAMILIES = {
    "lane_jit": ("model", LANE, True, [16, 0], {}, {
        "forward_packed": r"molann_lane_jit<NL=2>", "forward_train": r"molann_lane_jit<NL=2>", "features": r"molann_lane_jit<NL=0>",
        "backward_x": r"molann_bwd_ring ", "backward_p": r"molann_bwd_ring ", "backward_xp": r"molann_bwd_ring ",
        "value_and_vjp": r"molann_bwd_ring<values>", "mlp_packed": r"mlp_lane_kernel<NL=2>", "mlp_backward": r"molann_mlp_bwd",
        "features_backward": r"molann_lane_bwd", "features_jvp": r"frames_jvp_kernel", "align": r"align_out"}),
    "lane_jit_f32_solve": ("model", (20, 23), False, [16, 0], {}, {
        "forward_packed": r"molann_lane_jit<NL=2>", "backward_xp": r"molann_bwd_ring ", "value_and_vjp": r"molann_bwd_ring<values>"}),
    "lane_bwd": ("model", (20, 22), True, [16, 0], {"MOLANN_NO_RING_BWD": "1"}, {
        "backward_xp": r"molann_lane_jit<NL=.*molann_mlp_bwd.*molann_lane_bwd", "backward_x": r"molann_lane_bwd",
        "features_backward": r"molann_lane_bwd"}),
    "lane_regs": ("model", LANE, False, None, {"MOLANN_NO_JIT": "1"}, {
        "features": r"frames_lane_kernel<0,features_regs>", "align": r"frames_lane_kernel<0,align_out>"}),
    "lane_lds": ("model", LANE, True, None, {"MOLANN_NO_JIT": "1", "MOLANN_NO_REGS": "1"}, {
        "features": r"frames_lane_kernel<0,features_lds>"}),
    "lane_aot_head": ("model", LANE, True, [16, 0], {"MOLANN_NO_JIT": "1"}, {"forward_packed": r"frames_lane_kernel<2,features_"}),
    "ring_B8_group_bwd": ("model", MID, True, [32, 0], {}, {
        "forward_packed": RING % 8 + r".*mlp_lane_kernel", "forward_train": RING % 8 + r".*mlp_lane_kernel", "features": RING % 8,
        "backward_xp": r"molann_mlp_bwd.*frames_group_bwd_kernel<B=", "backward_x": r"frames_group_bwd_kernel<B=",
        "features_backward": r"frames_group_bwd_kernel<B=", "mlp_packed": r"mlp_lane_kernel<NL=2>", "mlp_backward": r"molann_mlp_bwd"}),
    "ring_B1": ("model", MID, False, [16, 0], {"MOLANN_RING_BATCH": "1"}, {"forward_packed": r"frames_ring_kernel<ND=\d+> "}),
    "wave_mid": ("model", MID, True, None, {"MOLANN_NO_RING": "1"}, {"features": r"frames_wave_kernel<", "align": r"frames_wave_kernel<.*mode=1|molann_lane_jit<align_out>"}),
    "wave_2000": ("model", LARGE, True, None, {"MOLANN_NO_RING": "1"}, {"features": r"frames_wave_kernel<"}),
    "wave_gather_2000": ("model", LARGE, True, None, {}, {
        "features": FWD_ANY, "features_backward": r"frames_wave_bwd_gather_kernel", "backward_x": r"frames_wave_bwd_gather_kernel"}),
    "wave_atomics_2000": ("model", LARGE, False, None, {"MOLANN_BWD_ATOMICS": "1"}, {"backward_x": r"frames_wave_bwd_kernel"}),
    "group_vjp": ("model", MID, True, [16, 0], {}, {"value_and_vjp": r"molann_group_vjp<B="}),
    "jvp_f32": ("model", MID, True, None, {}, {"features_jvp": r"frames_jvp_kernel"}),
    "align_batch": ("align", MID, False, None, {}, {
        "align": r"frames_align_batch_kernel<", "features": r"frames_align_batch_kernel<", "backward_x": r"frames_align_bwd_regs_kernel<"}),
    "align_regs": ("align", ALIGN_BIG, False, None, {}, {
        "align": r"frames_align_regs_kernel<", "features": r"frames_align_regs_kernel<", "backward_x": r"frames_align_bwd_regs_kernel<"}),
    "mlp_mfma_f32": ("head", (40,), False, [33, 0], {"MOLANN_NO_JIT": "1"}, {"mlp_packed": r"mlp_mfma_kernel<f32>"}),
    "mlp_mfma_bf16": ("head", (40,), False, [33, 0], {"MOLANN_NO_JIT": "1"}, {"mlp_packed": r"mlp_mfma_kernel<bf16>"}),
    "mlp_chain_f32": ("head", (40,), False, [33, 0], {}, {"mlp_packed": r"molann_mlp_chain<f32"}),
    "mlp_chain_bf16": ("head", (40,), False, [33, 0], {}, {"mlp_packed": r"molann_mlp_chain<bf16"}),
    "chain_bwd": ("head", (6,), False, [100, 70, 0], {}, {"mlp_packed": r"molann_mlp_chain<f32", "mlp_backward": r"molann_chain_bwd"}),
    "f64_small": ("model", LANE, True, [16, 0], {}, {
        "align_f64": r"frames_f64_kernel \(aligned coordinates\)", "features_f64": r"frames_f64_kernel \(features\)",
        "forward_f64": r"frames_f64_kernel \(features\) \+ mlp_f64_kernel", "mlp_f64": r"mlp_f64_kernel",
        "features_backward_f64": r"frames_bwd_f64_kernel", "features_jvp_f64": r"frames_jvp_f64_kernel",
        "features_hvp_f64": r"frames_hvp_f64_kernel", "value_and_vjp_f64": r"frames_value_vjp_f64_kernel",
        "value_and_jacobian_f64": r"frames_value_jac_f64_kernel", "value_and_metric_f64": r"frames_value_metric_f64_kernel",
        "value_and_restraint_f64": r"frames_value_restraint_f64_kernel", "value_and_hills_f64": r"frames_value_hills_f64_kernel"}),
    "f64_mid": ("model", (165, 166), True, [16, 0], {}, {
        "align_f64": r"frames_f64_kernel \(aligned coordinates\)", "features_f64": r"frames_f64_kernel \(features\)",
        "forward_f64": r"frames_f64_kernel \(features\) \+ mlp_f64_kernel", "features_backward_f64": r"frames_bwd_f64_kernel",
        "features_jvp_f64": r"frames_jvp_f64_kernel", "features_hvp_f64": r"frames_hvp_f64_kernel",
        "value_and_vjp_f64": r"frames_value_vjp_f64_kernel", "value_and_jacobian_f64": r"frames_value_jac_f64_kernel",
        "value_and_metric_f64": r"frames_value_metric_f64_kernel", "value_and_restraint_f64": r"frames_value_restraint_f64_kernel",
        "value_and_hills_f64": r"frames_value_hills_f64_kernel"}),
}
F64_FAMILIES = ("f64_small", "f64_mid")
# molann_mlp_bwd hands the 64-frame tiles of a block to its waves through an atomic counter (molann_mlp_bwd.inc, `next_tile`: "tiles
# interleaved over the blocks, handed out inside a block") and adds the waves' sums in wave order, so with more than one tile the
# order in which the tiles' contributions to dW / db are added changes from launch to launch - whatever the placement.  Its
# grad_params (and nothing else of these calls) is held to the float64 oracle at every placement once n > 64, at the tolerance
# test_gpu_angular_edges.py holds the parameter gradients of these families to; at n <= 64 it is bit for bit like every other output.
TILE_ORDER = {("lane_jit", "mlp_backward"), ("lane_bwd", "backward_xp"), ("ring_B8_group_bwd", "backward_xp"),
              ("ring_B8_group_bwd", "mlp_backward")}
ATOMICS = ("wave_atomics_2000",)        # dL/dx summed by float atomics: not bitwise reproducible; held to the oracle at every placement
# The kernels the table must reach besides the routed families' own: the head kernels and the alignment kernels
NAMED = (r"mlp_lane_kernel", r"mlp_mfma_kernel<f32>", r"mlp_mfma_kernel<bf16>", r"molann_mlp_chain<f32", r"molann_mlp_chain<bf16",
         r"molann_mlp_bwd", r"molann_chain_bwd", r"frames_align_batch_kernel", r"frames_align_regs_kernel", r"frames_align_bwd_regs_kernel",
         r"frames_hvp_f64_kernel")


def _cases():
    """(family, frame size, last head width): heads end in 4 and in 3, feature rows have 6 / 7 / 8 columns (+ 9 with positions)."""
    out = []
    for fam, (kind, sizes, _, head, _, _) in FAMILIES.items():
        for i, n_inp in enumerate(sizes):
            if kind == "head":
                out += [(fam, n_inp, 4), (fam, n_inp, 3)]
            else:
                out.append((fam, n_inp, (4, 3)[i % 2] if head is not None else (2, 1, 0)[i % 3]))
    return out


CASES = _cases()


# ---- the plans ---------------------------------------------------------------------------------------------------------------
def _spec(n_inp, pos, extra_bonds):
    """(xyz, align, items) on a chain of n_inp atoms: an angle, two dihedrals, a bond (6 columns), `extra_bonds` more bonds, three
    position atoms.  Small frames keep everything in the first 16 slots (the lane kernel's regs mode), as test_gpu_angular_edges."""
    xyz = wl.synthetic_chain(n_atoms=n_inp, step=1.4, seed=11 if n_inp < 1000 else 5)
    if n_inp < 100:
        align = [0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11, 13, 15]
        items = [(ANGLE, [1, 4, 5]), (DIH, [4, 6, 8, 14]), (DIH, [12, 10, 8, 9]), (BOND, [1, 4])]
        more, where = [(BOND, [2, 7]), (BOND, [3, 11])], [0, 2, 3]
    elif n_inp < 1000:
        align = [a for a in fft.P_SEL if a < n_inp]
        items = [(ANGLE, [20, 21, 23]), (DIH, [40, 41, 42, 43]), (DIH, [91, 92, 93, 94]), (BOND, [120, 121])]
        more, where = [(BOND, [60, 63]), (BOND, [130, 140])], [10, 86, n_inp - 1]
    else:
        align = list(range(7, 2000, 13))
        items = [(ANGLE, [100, 101, 103]), (DIH, [500, 501, 502, 504]), (DIH, [1500, 1501, 1502, 1503]), (BOND, [1900, 1901])]
        more, where = [(BOND, [700, 703]), (BOND, [1200, 1210])], [31, 1001, n_inp - 1]
    items = items + more[:extra_bonds] + ([(POS, where)] if pos else [])
    return xyz, align, items


def _frames(xyz, n, seed):
    """[n, n_inp, 3] float64 on the CPU: the chain + 0.05 A of noise, rigidly moved (away from every angular pole)."""
    g = torch.Generator().manual_seed(seed)
    ref = torch.from_numpy(np.ascontiguousarray(xyz, np.float64))
    x = ref.unsqueeze(0) + 0.05 * torch.randn((n,) + tuple(ref.shape), generator=g, dtype=F64)
    q = torch.randn((n, 4), generator=g, dtype=F64)
    rot = wl.quaternion_to_matrix(q / q.norm(dim=1, keepdim=True)).to(F64)
    return (torch.matmul(x, rot) + 3.0 * torch.randn((n, 1, 3), generator=g, dtype=F64)).contiguous()


def _plans_of(model):
    return [e.plan for m in model.modules() if hasattr(m, "_plans") for e in m._plans().values() if isinstance(e, _PlanEntry)]


class Ctx(object):
    """One (family, frame size, width) case: its plans and what the oracle needs."""

    def __init__(self, family, n_inp, tail, dev):
        kind, _, pos, head, _, self.patterns = FAMILIES[family]
        self.family, self.kind, self.n_inp, self.dev = family, kind, n_inp, dev
        self.f64 = family in F64_FAMILIES
        self.dtype = F64 if self.f64 else F32
        self.bf16 = family.endswith("bf16")
        self.align_plan = None
        if kind == "head":                                 # n_inp is the feature dimension here
            self.dims = [n_inp] + head[:-1] + [tail]
            with torch.cuda.device(dev):
                self.plan = tmc._plan(self.dims, _capi.ACT_TANH, precision=_capi.MLP_BF16 if self.bf16 else _capi.MLP_F32)
                self.Ws, self.bs = tmc._params(self.dims, dev, 7)
                self.plan.update_mlp(self.Ws, self.bs)
                if "mlp_backward" in self.patterns:
                    assert self.plan.supports_mlp_backward()        # builds molann_chain_bwd
            self.act = torch.tanh
            self.d_feat, self.d_out, self.head, self.items, self.align, self.ref = self.dims[0], tail, None, [], None, None
            return
        self.xyz, self.align, self.items = _spec(n_inp, pos, tail if head is None else 0)
        x4 = _frames(self.xyz, 4, 1).to(dev, self.dtype)
        if kind == "align":
            self.items = [(POS, list(range(n_inp)))]       # the aligned frame is this plan's feature row
            case = rb.Case(family, self.xyz, (), self.align, False, None, align_only=True)
            model = case.build(dev)
            with torch.no_grad():
                model(x4)                                  # the "align" plan: no items
            model(x4.clone().requires_grad_(True))         # the "align_grad" plan: one position item per atom
            plans = dict((p.feature_dim > 0, p) for p in _plans_of(model))
            self.plan, self.align_plan = plans[True], plans[False]
            self.dims = None
        else:
            d = sum(mo.feature_dim(t, len(i), False) for t, i in self.items)
            self.dims = None if head is None else [d] + head[:-1] + [tail]
            case = rb.Case(family, self.xyz, self.items, self.align, False, self.dims)
            model = case.build(dev)
            if self.f64:
                model = model.double()
            model.requires_grad_(False)
            if isinstance(model, MolANN) and not self.f64:
                self.plan = model.plan_for(x4)
            else:
                with torch.no_grad():
                    model(x4)
                self.plan = [p for p in _plans_of(model) if p.feature_dim == d][-1]
        torch.cuda.synchronize()
        self.model = model
        self.ref = rb._align_layer(model).ref_x.detach().cpu().double()
        self.head = rb._head64(model).requires_grad_(True) if self.dims else None     # the oracle differentiates its copies
        self.d_feat, self.d_out = self.plan.feature_dim, (self.dims[-1] if self.dims else self.plan.feature_dim)
        if self.f64 and self.dims:
            lins = [m for m in model.ann_layers if isinstance(m, torch.nn.Linear)]
            self.Ws, self.bs = [l.weight.detach() for l in lins], [l.bias.detach() for l in lins]

    def seed(self, entry, n):
        return zlib.crc32(("%s %s %d" % (self.family, entry, n)).encode()) & 0x7FFFFFFF

    def x(self, n, entry):
        return _frames(self.xyz, n, self.seed(entry, n) % 1000 + 2).to(self.dtype)

    def randn(self, shape, entry, n, salt=0):
        g = torch.Generator().manual_seed(self.seed(entry, n) + salt)
        return torch.randn(shape, generator=g, dtype=F64).to(self.dtype)


_CTX = {}


def _ctx(family, n_inp, tail, dev, monkeypatch):
    for k, v in FAMILIES[family][4].items():
        monkeypatch.setenv(k, v)
    key = (family, n_inp, tail)
    if key not in _CTX:
        _CTX.clear()                                       # one case's plans at a time
        _CTX[key] = Ctx(family, n_inp, tail, dev)
    return _CTX[key]


# ---- the entry points ---------------------------------------------------------------------------------------------------------
# An entry: its buffers in the order of the C signature, as (name, role, data or shape) - role "in" (data), "out" (shape) or "acc"
# (shape: accumulated into, prefilled by ACC) - and the call on a dictionary of addresses.
def ACC(numel):
    return (torch.arange(numel) % 13).to(F32) * 0.125


def _ptr_array(p, names):
    return (ctypes.c_void_p * max(1, len(names)))(*[p[k] for k in names])


def _layers(cx):
    """The float64 Linear tensors as inputs of the call, and their names"""
    bufs, wn, bn = [], [], []
    for l, (w, b) in enumerate(zip(cx.Ws, cx.bs) if cx.dims else ()):
        bufs += [("W%d" % l, "in", w.cpu()), ("b%d" % l, "in", b.cpu())]
        wn.append("W%d" % l)
        bn.append("b%d" % l)
    return bufs, wn, bn


def _entry(cx, entry, n):
    """(buffers, call(handle, addresses, stream) -> return code, the plan) of an entry on n frames of the case."""
    L, ni, df, do = _capi.lib(), cx.n_inp, cx.d_feat, cx.d_out
    X = lambda: ("x", "in", cx.x(n, entry))                                        # noqa: E731
    R = lambda name, shape, salt=0: (name, "in", cx.randn(shape, entry, n, salt))  # noqa: E731
    plan = cx.plan
    if entry in ("align", "align_f64"):
        fn = L.molann_align_f32 if entry == "align" else L.molann_align_f64
        plan = cx.align_plan or cx.plan
        return [X(), ("out", "out", (n, ni, 3))], lambda h, p, s: fn(h, p["x"], n, p["out"], s), plan
    if entry in ("features", "features_f64"):
        fn = L.molann_features_f32 if entry == "features" else L.molann_features_f64
        return [X(), ("out", "out", (n, df))], lambda h, p, s: fn(h, p["x"], n, p["out"], s), plan
    if entry == "forward_packed":
        return [X(), ("out", "out", (n, do))], lambda h, p, s: L.molann_forward_packed_f32(h, p["x"], n, p["out"], s), plan
    if entry == "mlp_packed":
        return [R("f", (n, df)), ("out", "out", (n, do))], lambda h, p, s: L.molann_mlp_packed_f32(h, p["f"], n, p["out"], s), plan
    if entry == "forward_train":
        return [X(), ("out", "out", (n, do)), ("features", "out", (n, df))], \
            lambda h, p, s: L.molann_forward_train_f32(h, p["x"], n, p["out"], p["features"], s), plan
    if entry in ("backward_x", "backward_p", "backward_xp"):
        bufs = [X(), R("grad_out", (n, do))]
        if "x" in entry[9:]:
            bufs.append(("grad_x", "out", (n, ni, 3)))
        if "p" in entry[9:]:
            bufs.append(("grad_params", "acc", (plan.grad_params_size(),)))
        return bufs, lambda h, p, s: L.molann_backward_f32(h, p["x"], p["grad_out"], n, p.get("grad_x"), p.get("grad_params"), s), plan
    if entry in ("features_backward", "features_backward_f64"):
        fn = L.molann_features_backward_f32 if entry == "features_backward" else L.molann_features_backward_f64
        return [X(), R("grad_f", (n, df)), ("grad_x", "out", (n, ni, 3))], \
            lambda h, p, s: fn(h, p["x"], p["grad_f"], n, p["grad_x"], s), plan
    if entry == "mlp_backward":
        return [R("f", (n, df)), R("grad_out", (n, do), 1), ("grad_f", "out", (n, df)), ("grad_params", "acc", (plan.grad_params_size(),))], \
            lambda h, p, s: L.molann_mlp_backward_f32(h, p["f"], p["grad_out"], n, p["grad_f"], p["grad_params"], s), plan
    if entry == "value_and_vjp":
        return [X(), R("grad_out", (n, do)), ("out", "out", (n, do)), ("grad_x", "out", (n, ni, 3))], \
            lambda h, p, s: L.molann_value_and_vjp_f32(h, p["x"], p["grad_out"], n, p["out"], p["grad_x"], s), plan
    if entry in ("features_jvp", "features_jvp_f64"):
        fn = L.molann_features_jvp_f32 if entry == "features_jvp" else L.molann_features_jvp_f64
        return [X(), R("v", (N_TANGENTS, n, ni, 3)), ("out", "out", (n, df)), ("tangent_out", "out", (N_TANGENTS, n, df))], \
            lambda h, p, s: fn(h, p["x"], p["v"], n, N_TANGENTS, p["out"], p["tangent_out"], s), plan
    if entry == "features_hvp_f64":
        return [X(), R("g", (n, df)), R("u", (n, ni, 3), 1), ("hx", "out", (n, ni, 3)), ("hg", "out", (n, df))], \
            lambda h, p, s: L.molann_features_hvp_f64(h, p["x"], p["g"], p["u"], n, p["hx"], p["hg"], s), plan
    lay, wn, bn = _layers(cx)
    WB = lambda p: (_ptr_array(p, wn), _ptr_array(p, bn))                          # noqa: E731
    if entry == "mlp_f64":
        return [R("f", (n, df))] + lay + [("out", "out", (n, do))], \
            lambda h, p, s: L.molann_mlp_f64(h, p["f"], n, *WB(p), p["out"], s), plan
    if entry == "forward_f64":
        return [X()] + lay + [("work", "out", (n, df)), ("out", "out", (n, do))], \
            lambda h, p, s: L.molann_forward_f64(h, p["x"], n, *WB(p), p["work"], p["out"], s), plan
    if entry == "value_and_vjp_f64":
        return [X(), R("grad_out", (n, do))] + lay + [("out", "out", (n, do)), ("grad_x", "out", (n, ni, 3))], \
            lambda h, p, s: L.molann_value_and_vjp_f64(h, p["x"], p["grad_out"], n, *WB(p), p["out"], p["grad_x"], s), plan
    if entry == "value_and_jacobian_f64":
        return [X()] + lay + [("out", "out", (n, do)), ("jac", "out", (n, do, ni, 3))], \
            lambda h, p, s: L.molann_value_and_jacobian_f64(h, p["x"], n, *WB(p), p["out"], p["jac"], s), plan
    if entry == "value_and_metric_f64":
        w = 0.5 + cx.randn((ni,), entry, n, 2).abs()
        return [X()] + lay + [("atom_weights", "in", w), ("out", "out", (n, do)), ("metric", "out", (n, do, do))], \
            lambda h, p, s: L.molann_value_and_metric_f64(h, p["x"], n, *WB(p), p["atom_weights"], p["out"], p["metric"], s), plan
    if entry == "value_and_restraint_f64":
        center, kappa = cx.randn((n, do), entry, n, 3), 0.5 + cx.randn((do,), entry, n, 4).abs()
        period = torch.where(torch.arange(do) % 2 == 0, torch.full((do,), 2.5, dtype=F64), torch.zeros(do, dtype=F64))
        flat = 0.05 * (torch.arange(do) % 3).to(F64)
        return [X()] + lay + [("center", "in", center), ("kappa", "in", kappa), ("period", "in", period), ("flat", "in", flat),
                              ("out", "out", (n, do)), ("energy", "out", (n,)), ("grad_x", "out", (n, ni, 3))], \
            lambda h, p, s: L.molann_value_and_restraint_f64(h, p["x"], n, *WB(p), p["center"], do, p["kappa"], p["period"], p["flat"],
                                                             p["out"], p["energy"], p["grad_x"], s), plan
    if entry == "value_and_hills_f64":
        H = 5
        centers, heights = cx.randn((H, do), entry, n, 5), cx.randn((H,), entry, n, 6)
        sigma = 0.5 + cx.randn((H, do), entry, n, 7).abs()
        period = torch.where(torch.arange(do) % 2 == 1, torch.full((do,), 3.0, dtype=F64), torch.zeros(do, dtype=F64))
        return [X()] + lay + [("centers", "in", centers), ("heights", "in", heights), ("sigma", "in", sigma), ("period", "in", period),
                              ("out", "out", (n, do)), ("bias", "out", (n,)), ("grad_x", "out", (n, ni, 3))], \
            lambda h, p, s: L.molann_value_and_hills_f64(h, p["x"], n, *WB(p), p["centers"], p["heights"], H, p["sigma"], do, p["period"],
                                                         p["out"], p["bias"], p["grad_x"], s), plan
    raise KeyError(entry)


ROW_DIMS = {"v": 2, "tangent_out": 1}   # [T, N, n_inp, 3] and [T, N, d]: a frame's worth is the last two dimensions / the last one
_ARENA = {}


def _arena(dev):
    if dev not in _ARENA:
        _ARENA[dev] = pl.Arena(dev, capacity=192 << 20)
    return _ARENA[dev]


def _launch(cx, entry, n, placement, spec=None, shift=None, fresh=False):
    """One call.  Returns (return code, launch info before, after, {name: view}, the arena's complaints).  `shift`: (name, bytes)
    moves one address (the refusals); `fresh`: ordinary torch tensors in place of the arena."""
    bufs, call, plan = spec or _entry(cx, entry, n)
    arena = _arena(cx.dev)
    arena.reset()
    offs = pl.offsets(placement, [b[0] for b in bufs], wide=16 // (8 if cx.f64 else 4))
    views = {}
    for name, role, payload in bufs:
        if fresh:
            if role == "in":
                views[name] = payload.to(cx.dev, cx.dtype).contiguous().clone()
            else:
                views[name] = torch.full(payload, float("nan"), dtype=cx.dtype, device=cx.dev)
        elif role == "in":
            views[name] = arena.carve(name, payload.shape, cx.dtype, offs[name], data=payload, row_dims=ROW_DIMS.get(name))
        else:
            views[name] = arena.carve(name, payload, cx.dtype, offs[name], row_dims=ROW_DIMS.get(name))
        if role == "acc":
            views[name].copy_(ACC(views[name].numel()).to(cx.dev))
    p = dict((k, v.data_ptr()) for k, v in views.items())
    if shift is not None:
        p[shift[0]] += shift[1]
    before = plan.last_launch_info()
    with torch.cuda.device(cx.dev):
        rc = call(plan._handle, p, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
    after = plan.last_launch_info()
    complaints = [] if fresh else (arena.check() + ["input %s was written" % k for k in arena.inputs_changed()])
    return rc, before, after, views, complaints


def _outputs(bufs, views):
    return dict((name, views[name].clone()) for name, role, _ in bufs if role != "in")


# ---- the oracle -----------------------------------------------------------------------------------------------------------------
def _su(cx, mode, head):
    return types.SimpleNamespace(mode=mode, ref=cx.ref, head=cx.head if head else None, items=cx.items, uav=False, align=cx.align)


def _mlp64(cx, f):
    """The head in float64 (bf16 plans: test_gpu_mlp_chain's emulation of the kernel's arithmetic)."""
    if cx.kind == "head":
        if cx.bf16:
            return tmc._emulate(f.float(), cx.Ws, cx.bs, _capi.ACT_TANH).double()
        h = f.double()
        for i, (w, b) in enumerate(zip(cx.Ws, cx.bs)):
            h = h @ w.cpu().double().T + b.cpu().double()
            if i + 1 < len(cx.Ws):
                h = cx.act(h)
        return h
    return cx.head(f.double())


def _want(cx, entry, data, dtype=F64):
    """{output name: expected tensor} of an entry through the oracle in dtype (float64: the reference; float32: its own error)."""
    x = data.get("x")
    if entry in ("mlp_packed", "mlp_f64"):
        return {"out": _mlp64(cx, data["f"]).to(dtype)} if dtype == F64 else None
    if entry == "mlp_backward":
        if dtype != F64:
            return None
        f = data["f"].double().requires_grad_(True)
        if cx.kind == "head":
            prm = [t.cpu().double().requires_grad_(True) for pair in zip(cx.Ws, cx.bs) for t in pair]
            h = f
            for i in range(len(cx.Ws)):
                h = h @ prm[2 * i].T + prm[2 * i + 1]
                if i + 1 < len(cx.Ws):
                    h = cx.act(h)
        else:
            head = copy.deepcopy(cx.head)
            prm, h = list(head.parameters()), head(f)
        g = torch.autograd.grad((h * data["grad_out"].double()).sum(), [f] + prm)
        return {"grad_f": g[0], "grad_params": torch.cat([t.reshape(-1) for t in g[1:]]) + ACC(sum(t.numel() for t in g[1:])).double()}
    if entry in ("align", "align_f64"):
        with torch.no_grad():
            return {"out": mo.align_forward(x.to(dtype), cx.align, cx.ref.to(dtype))}
    if entry in ("features", "features_f64", "forward_packed", "forward_train", "forward_f64"):
        o = tae._oracle(_su(cx, "fwd", entry.startswith("forward")), x, None, dtype)
        out = {"out": o["y"]}
        if entry in ("forward_train", "forward_f64"):
            out["features" if entry == "forward_train" else "work"] = tae._oracle(_su(cx, "fwd", False), x, None, dtype)["y"]
        return out
    if entry.startswith("backward_") or entry in ("features_backward", "features_backward_f64"):
        with_head = entry.startswith("backward_") and cx.head is not None
        o = tae._oracle(_su(cx, "grad", with_head), x, data["grad_out" if entry.startswith("backward_") else "grad_f"], dtype)
        out = {}
        if entry != "backward_p":
            out["grad_x"] = o["D"]
        if entry in ("backward_p", "backward_xp"):
            flat = torch.cat([t.reshape(-1) for t in o["gp"]])
            out["grad_params"] = flat + ACC(flat.numel()).to(dtype)
        return out
    if entry in ("value_and_vjp", "value_and_vjp_f64"):
        o = tae._oracle(_su(cx, "vjp", True), x, data["grad_out"], dtype)
        return {"out": o["y"], "grad_x": o["D"]}
    if entry in ("features_jvp", "features_jvp_f64"):
        o = tae._oracle(_su(cx, "jvp64", False), x, list(data["v"]), dtype)
        return {"out": o["y"], "tangent_out": o["D"].transpose(0, 1)}
    if entry == "features_hvp_f64":
        xx = x.double().clone().requires_grad_(True)
        f = mo.preprocessing_forward(xx, cx.items, False, cx.align, cx.ref)
        (gx,) = torch.autograd.grad((f * data["g"]).sum(), xx, create_graph=True)
        (hx,) = torch.autograd.grad((gx * data["u"]).sum(), xx)
        _, hg = torch.func.jvp(lambda a: mo.preprocessing_forward(a, cx.items, False, cx.align, cx.ref), (x.double(),), (data["u"].double(),))
        return {"hx": hx, "hg": hg}
    if entry in ("value_and_jacobian_f64", "value_and_metric_f64"):
        o = tae._oracle(_su(cx, "jac", True), x, None, dtype)
        if entry == "value_and_jacobian_f64":
            return {"out": o["y"], "jac": o["D"]}
        return {"out": o["y"], "metric": torch.einsum("nkac,a,nlac->nkl", o["D"], data["atom_weights"].to(dtype), o["D"])}
    if entry in ("value_and_restraint_f64", "value_and_hills_f64"):
        xx = x.to(dtype).clone().requires_grad_(True)
        y = cx.head.to(dtype)(mo.preprocessing_forward(xx, cx.items, False, cx.align, cx.ref.to(dtype)))
        if entry == "value_and_restraint_f64":
            d = tae._wrapped(y - data["center"], data["period"])
            flat = data["flat"]
            d = torch.where(d.abs() <= flat, torch.zeros_like(d), torch.copysign(d.abs() - flat, d))
            E = 0.5 * (data["kappa"] * d * d).sum(1)
            name = "energy"
        else:
            d = tae._wrapped(y.unsqueeze(1) - data["centers"].unsqueeze(0), data["period"])
            E = (data["heights"] * torch.exp(-0.5 * ((d / data["sigma"]) ** 2).sum(2))).sum(1)
            name = "bias"
        (gx,) = torch.autograd.grad(E.sum(), xx)
        cx.head.double()
        return {"out": y.detach(), name: E.detach(), "grad_x": gx}
    raise KeyError(entry)


VALUES = ("out", "features", "work", "energy", "bias")


def _tolerance(cx, entry, name):
    """The existing tolerance of an output (the tests named in the module's docstring)."""
    if cx.kind == "head" or entry in ("mlp_packed", "mlp_backward"):
        if entry == "mlp_backward":
            return 2e-4                                    # test_gpu_wide_head_backward.py
        return 4e-3 if cx.bf16 else 1e-5                   # test_gpu_mlp_chain.py
    if entry == "features_hvp_f64":
        return 1e-12 if name == "hx" else 1e-9             # test_gpu_second_order_exact.py; hg is a tangent
    if cx.f64:
        return 1e-10 if name in VALUES else 1e-9           # test_gpu_angular_edges.py, float64
    if name in VALUES:
        return 1e-5
    return 1e-4 if entry == "features_jvp" else 5e-4       # test_gpu_angular_edges.py, float32 (tangents: test_gpu_jvp_plans.py)


def _against_oracle(cx, entry, bufs, got, what, kept=None):
    """The outputs `got` of a call (all of them, or some) against float64 through the oracle; returns the complaints.  `kept`: a
    dictionary that keeps the oracle's results for the next call on the same inputs."""
    if kept is None or "want" not in kept:
        data = dict((name, payload.cpu().double()) for name, role, payload in bufs if role == "in")
        want = _want(cx, entry, data)
        own = None if cx.f64 else _want(cx, entry, dict((k, v.float()) for k, v in data.items()), F32)
        if kept is not None:
            kept.update(want=want, own=own)
    else:
        want, own = kept["want"], kept["own"]
    bad = []
    assert set(got) <= set(want), (what, sorted(want), sorted(got))
    for name in got:
        w = want[name]
        w = w.detach().double().reshape(got[name].shape)
        g = got[name].detach().cpu().double()
        tol = _tolerance(cx, entry, name)
        if name in VALUES or name == "grad_params":        # one scale for the batch
            s = max(1.0 if name in VALUES else 1e-6, float(w.abs().max()))
            err = float((g - w).abs().max()) / s
            o = float((own[name].double().reshape(w.shape) - w).abs().max()) / s if own else 0.0
        else:                                              # derivative rows: each frame's largest entry, floored at 1e-3 of the batch's
            lead = 1 if name == "tangent_out" else 0
            rows = lambda t: t.transpose(0, lead).flatten(1)     # noqa: E731
            s = rows(w).abs().amax(1)
            s = s.clamp(min=max(1e-30, 1e-3 * float(s.max())))
            err = float(((rows(g) - rows(w)).abs().amax(1) / s).max())
            o = float(((rows(own[name].double().reshape(w.shape)) - rows(w)).abs().amax(1) / s).max()) if own else 0.0
        lim = max(tol, 2.0 * o)
        print("placement %s %s: kernel %.3g, float32 oracle %.3g, bound %.3g" % (what, name, err, o, lim))
        if not err <= lim:
            bad.append("%s %s: error %.3g over %.3g" % (what, name, err, lim))
    return bad


# ---- the tests --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,n_inp,tail", CASES, ids=["%s-%d-%d" % c for c in CASES])
def test_every_entry_on_offset_buffers(family, n_inp, tail, hip_device, monkeypatch):
    cx = _ctx(family, n_inp, tail, hip_device, monkeypatch)
    bad = []
    for entry, pattern in cx.patterns.items():
        bitwise, found = family not in ATOMICS, len(bad)
        for n in NS:
            spec = _entry(cx, entry, n)
            base, kept = None, {}
            by_oracle = ("grad_params",) if ((family, entry) in TILE_ORDER and n > 64) else ()
            for placement in PLACEMENTS[cx.dtype]:
                what = "%s %s n_inp=%d n=%d at %s" % (family, entry, n_inp, n, placement)
                rc, _, info, views, complaints = _launch(cx, entry, n, placement, spec)
                SEEN.append(info)
                if rc != 0:
                    bad.append("%s: return code %d (%s)" % (what, rc, _capi.error_string(rc)))
                    break
                if not re.search(pattern, info):
                    bad.append("%s: launch info %r lacks %r" % (what, info, pattern))
                bad += ["%s: %s" % (what, c) for c in complaints]
                got = _outputs(spec[0], views)
                if placement == 0:
                    base = got
                    if n == N_ANCHOR and bitwise:          # the arena itself changes nothing
                        _, _, _, fresh, _ = _launch(cx, entry, n, 0, spec, fresh=True)
                        bad += ["%s: %s differs from the call on fresh tensors" % (what, k) for k in got
                                if k not in by_oracle and not pl.same_bits(got[k], fresh[k])]
                elif bitwise:
                    bad += ["%s: %s differs from the all-zero placement" % (what, k) for k in got
                            if k not in by_oracle and not pl.same_bits(got[k], base[k])]
                # float64 through the oracle: everything once per family and size (the anchor of the bitwise checks), and at every
                # call what is not bitwise reproducible.  frames_wave_bwd_kernel (MOLANN_BWD_ATOMICS=1) adds every contribution to
                # dL/dx with a float atomic, in the order the lanes arrive (molann_dev_bwd.inc: "every contribution is a float atomic
                # into it"): its tolerance is the one test_gpu_angular_edges.py holds that family to.
                held = list(got) if (not bitwise or (placement == 0 and n == N_ANCHOR)) else by_oracle
                if held:
                    bad += _against_oracle(cx, entry, spec[0], dict((k, got[k]) for k in held), what, kept)
        if len(bad) == found:
            REACHED.add((family, entry))
    assert not bad, (len(bad), bad[:12])


def _pointers(bufs):
    return [name for name, _, _ in bufs]


F64_PINNED = ("value_and_vjp_f64", "value_and_jacobian_f64", "value_and_metric_f64")      # test_gpu_f64_entry_contract.py


@pytest.mark.parametrize("family", ["lane_jit", "ring_B8_group_bwd", "align_batch", "f64_small"])
def test_misaligned_pointers_are_refused(family, hip_device, monkeypatch):
    """One pointer at a time off by 2 bytes (float32) or 4 (float64): E_ALIGNMENT, nothing launched, nothing written."""
    n_inp = FAMILIES[family][1][1]
    cx = _ctx(family, n_inp, 3 if FAMILIES[family][3] else 1, hip_device, monkeypatch)
    n, bad = 5, []
    for entry in cx.patterns:
        if entry in F64_PINNED:
            continue
        spec = _entry(cx, entry, n)
        rc, _, _, _, _ = _launch(cx, entry, n, 0, spec)     # the kernels are built and the launch info is this entry's
        assert rc == 0, (family, entry, rc)
        for name in _pointers(spec[0]):
            rc, before, after, views, complaints = _launch(cx, entry, n, 1, spec, shift=(name, 4 if cx.f64 else 2))
            what = "%s %s, %s off by %d" % (family, entry, name, 4 if cx.f64 else 2)
            if rc != _capi.E_ALIGNMENT:
                bad.append("%s: return code %d" % (what, rc))
            if before != after:
                bad.append("%s: launch info changed to %r" % (what, after))
            bad += ["%s: %s" % (what, c) for c in complaints]
            arena = _arena(cx.dev)
            for out, role, _ in spec[0]:
                if role == "out" and not arena.holds_sentinel(out):
                    bad.append("%s: %s was written" % (what, out))
                if role == "acc" and not bool(torch.equal(views[out].cpu(), ACC(views[out].numel()))):
                    bad.append("%s: %s was written" % (what, out))
    assert not bad, (len(bad), bad[:12])


def test_plan_updates_read_offset_sources(hip_device, monkeypatch):
    """update_ref, update_ref_f64 and update_mlp with their source tensors in the arena at every residue: the forward that follows
    gives the bits of the aligned sources', and a source off by 2 (4) bytes is refused."""
    L = _capi.lib()
    for family, n_inp in (("lane_jit", 21), ("f64_small", 21)):
        cx = _ctx(family, n_inp, 3, hip_device, monkeypatch)
        entry = "forward_f64" if cx.f64 else "forward_packed"
        spec = _entry(cx, entry, N_ANCHOR)
        rc, _, _, views, _ = _launch(cx, entry, N_ANCHOR, 0, spec)
        assert rc == 0
        want = views["out"].clone()
        lins = [m for m in cx.model.ann_layers if isinstance(m, torch.nn.Linear)]
        ref_dev = rb._align_layer(cx.model).ref_x.detach()
        side = pl.Arena(hip_device, capacity=4 << 20)
        s = lambda: torch.cuda.current_stream().cuda_stream      # noqa: E731
        for k in PLACEMENTS[cx.dtype][:-2]:
            side.reset()
            ref = side.carve("ref", ref_dev.shape, cx.dtype, k, data=ref_dev)
            with torch.cuda.device(hip_device):
                fn = L.molann_plan_update_ref_f64 if cx.f64 else L.molann_plan_update_ref
                assert fn(cx.plan._handle, ref.data_ptr(), s()) == 0
                assert fn(cx.plan._handle, ref.data_ptr() + (4 if cx.f64 else 2), s()) == _capi.E_ALIGNMENT
                if not cx.f64:
                    ws = [side.carve("W%d" % i, l.weight.shape, F32, (k + i) % 4, data=l.weight.detach()) for i, l in enumerate(lins)]
                    bs = [side.carve("b%d" % i, l.bias.shape, F32, (k + i + 1) % 4, data=l.bias.detach()) for i, l in enumerate(lins)]
                    W, B = _capi._layer_pointers(ws, bs)
                    assert L.molann_plan_update_mlp(cx.plan._handle, W, B, s()) == 0
                    W[1] = ws[1].data_ptr() + 2
                    assert L.molann_plan_update_mlp(cx.plan._handle, W, B, s()) == _capi.E_ALIGNMENT
                torch.cuda.synchronize()
            assert side.check() == [] and side.inputs_changed() == []
            rc, _, _, views, complaints = _launch(cx, entry, N_ANCHOR, 0, spec)
            assert rc == 0 and not complaints
            assert pl.same_bits(views["out"], want), (family, k, "the forward after an update from offset sources")
    REACHED.add(("updates", "all"))


# ---- through torch --------------------------------------------------------------------------------------------------------------
def test_autograd_with_offset_views(hip_device, monkeypatch):
    """model(x_view) under autograd with a cotangent that is an offset view (the grad_out.contiguous() passthrough)."""
    cx = _ctx("lane_jit", 21, 3, hip_device, monkeypatch)
    model = copy.deepcopy(cx.model).requires_grad_(True)
    n = N_ANCHOR
    x0, g0 = cx.x(n, "autograd"), cx.randn((n, cx.d_out), "autograd", n)
    results = []
    for k in (0, 1, 3):
        arena = _arena(hip_device)
        arena.reset()
        x = arena.carve("x", x0.shape, F32, k, data=x0).requires_grad_(True)
        g = arena.carve("g", g0.shape, F32, (k + 1) % 4 if k else 0, data=g0)
        for p in model.parameters():
            p.grad = None
        y = model(x)
        y.backward(g)
        torch.cuda.synchronize()
        assert re.search(r"molann_bwd_ring ", fft._infos(model)), fft._infos(model)
        assert arena.check() == [] and arena.inputs_changed() == [], (k, arena.check(), arena.inputs_changed())
        results.append([y.detach().clone(), x.grad.clone()] + [p.grad.clone() for p in model.parameters()])
    for r in results[1:]:
        assert all(pl.same_bits(a, b) for a, b in zip(r, results[0]))
    gp = torch.cat([t.reshape(-1) for t in results[0][2:]])
    bufs = [("x", "in", x0), ("grad_out", "in", g0)]
    bad = _against_oracle(cx, "forward_packed", bufs[:1], {"out": results[0][0]}, "autograd")
    bad += _against_oracle(cx, "backward_xp", bufs, {"grad_x": results[0][1], "grad_params": gp + ACC(gp.numel()).to(hip_device)}, "autograd")
    assert not bad, bad
    REACHED.add(("torch", "autograd"))


def test_into_views_from_the_arena(hip_device, monkeypatch):
    """value_and_vjp (float32 and float64), value_and_jacobian and value_and_restraint with `into=` views carved from the arena."""
    for family, calls in (("lane_jit", ("vjp",)), ("f64_small", ("vjp", "jacobian", "restraint"))):
        cx = _ctx(family, 21, 3, hip_device, monkeypatch)
        n, ni, do = N_ANCHOR, cx.n_inp, cx.d_out
        x0, g0 = cx.x(n, "into"), cx.randn((n, do), "into", n)
        center, kappa = cx.randn((n, do), "into", n, 1), 0.5 + cx.randn((do,), "into", n, 2).abs()
        for call in calls:
            shapes = {"vjp": [(n, do), (n, ni, 3)], "jacobian": [(n, do), (n, do, ni, 3)], "restraint": [(n, do), (n,), (n, ni, 3)]}[call]
            results = []
            for placement in PLACEMENTS[cx.dtype]:
                arena = _arena(hip_device)
                arena.reset()
                names = ["x", "g", "center", "kappa"] + ["into%d" % i for i in range(len(shapes))]
                offs = pl.offsets(placement, names, wide=16 // (8 if cx.f64 else 4))
                x = arena.carve("x", x0.shape, cx.dtype, offs["x"], data=x0)
                g = arena.carve("g", g0.shape, cx.dtype, offs["g"], data=g0)
                c = arena.carve("center", center.shape, cx.dtype, offs["center"], data=center)
                kp = arena.carve("kappa", kappa.shape, cx.dtype, offs["kappa"], data=kappa)
                into = tuple(arena.carve("into%d" % i, s, cx.dtype, offs["into%d" % i]) for i, s in enumerate(shapes))
                if call == "vjp":
                    got = cx.model.value_and_vjp(x, g, into=into)
                elif call == "jacobian":
                    got = cx.model.value_and_jacobian(x, into=into)
                else:
                    got = cx.model.value_and_restraint(x, c, kp, into=into)
                torch.cuda.synchronize()
                assert all(a.data_ptr() == b.data_ptr() for a, b in zip(got, into)), (family, call, "into was not used")
                assert arena.check() == [] and arena.inputs_changed() == [], (family, call, placement, arena.check(), arena.inputs_changed())
                results.append([t.clone() for t in into])
            for r in results[1:]:
                assert all(pl.same_bits(a, b) for a, b in zip(r, results[0])), (family, call)
            plain = {"vjp": lambda: cx.model.value_and_vjp(x0.to(hip_device), g0.to(hip_device)),
                     "jacobian": lambda: cx.model.value_and_jacobian(x0.to(hip_device)),
                     "restraint": lambda: cx.model.value_and_restraint(x0.to(hip_device), center.to(hip_device), kappa.to(hip_device))}[call]()
            assert all(pl.same_bits(a, b) for a, b in zip(plain, results[0])), (family, call, "the arena changed the result")
    REACHED.add(("torch", "into"))


def test_operator_on_an_offset_x(hip_device, monkeypatch):
    """torch.ops.molann.value_and_vjp (the scripted module's operator) on an x and a cotangent that are offset views."""
    from molann_amd import script
    cx = _ctx("lane_jit", 21, 3, hip_device, monkeypatch)
    script.load_ops()
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        scripted = torch.jit.script(copy.deepcopy(cx.model))
    ws, bs = [lin.weight for lin in scripted.linears.children()], [lin.bias for lin in scripted.linears.children()]
    n = N_ANCHOR
    x0, g0 = cx.x(n, "op"), cx.randn((n, cx.d_out), "op", n)
    results = []
    for k in (0, 1, 2, 3):
        arena = _arena(hip_device)
        arena.reset()
        x = arena.carve("x", x0.shape, F32, k, data=x0)
        g = arena.carve("g", g0.shape, F32, (k + 2) % 4 if k else 0, data=g0)
        y, dx = torch.ops.molann.value_and_vjp(x, list(scripted.desc), scripted.ref_x, ws, bs, g, [])
        torch.cuda.synchronize()
        assert arena.check() == [] and arena.inputs_changed() == []
        results.append((y.clone(), dx.clone()))
    for r in results[1:]:
        assert pl.same_bits(r[0], results[0][0]) and pl.same_bits(r[1], results[0][1])
    y, dx = cx.model.value_and_vjp(x0.to(hip_device), g0.to(hip_device))
    assert pl.same_bits(y, results[0][0]) and pl.same_bits(dx, results[0][1])
    REACHED.add(("torch", "operator"))


def test_every_placement_family_was_reached(request):
    """The families are recorded as they pass, so this guard needs all of them in the same session."""
    here = {item.name for item in request.session.items if item.module is request.module}
    wanted = {"test_every_entry_on_offset_buffers[%s-%d-%d]" % c for c in CASES} | \
             {"test_plan_updates_read_offset_sources", "test_autograd_with_offset_views", "test_into_views_from_the_arena",
              "test_operator_on_an_offset_x"}
    if not wanted <= here:
        pytest.skip("the coverage guard needs every family in this session: %d not selected" % len(wanted - here))
    want = {(f, e) for f, v in FAMILIES.items() for e in v[5]} | {("updates", "all"), ("torch", "autograd"), ("torch", "into"), ("torch", "operator")}
    missing = sorted(want - REACHED)
    assert not missing, ("not reached:", missing)
    seen = " | ".join(sorted(set(SEEN)))
    unnamed = [p for p in NAMED if not re.search(p, seen)]
    assert not unnamed, ("kernels no launch info named:", unnamed)
