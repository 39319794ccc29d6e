"""The host contract of the three float64 one-launch entry points - molann_value_and_vjp_f64, molann_value_and_jacobian_f64,
molann_value_and_metric_f64 - as recorded from the commit before their host code was folded into one path: every expected value
below is a literal taken from that commit's run, none is computed by the code under test.

1. Return codes of the C entries for null, negative, misaligned and missing arguments, and the order of those checks.  Every case
   returns before a launch; the buffers are real all the same (with room to spare), so that a check that failed to refuse would launch
   on valid memory.
2. The launch info (kernel name, lanes per frame, block, LDS bytes) of each entry at 4 frames of plans on either side of the lane
   group's 8/9, 16/17 and 32/33 boundaries, of the narrowest head whose rows step the block down from four waves for all three
   kernels, of the narrowest head whose rows exceed 64 KiB for all three (the kernel's dynamic-LDS limit is raised), and of a
   features-only plan with 65 features, which the metric refuses and the Jacobian serves.  The rows, in doubles per frame, behind
   3 features and 2 outputs without an alignment: 3 + the hidden widths + 2 max_w for the forces, 3 + the hidden widths + 2 * 2 * max_w
   for the Jacobian and the metric, max_w the widest layer input.  Four waves of one frame each pass 64 KiB from 2049 doubles on: a
   [3, 682, 2] head for the forces (2049), where the Jacobian has 3413, two waves.  One frame passes 64 KiB from 8193 doubles on.
   Plan creation refuses a head whose two widest consecutive layer inputs pass some 2550 together, so one hidden layer (3 + 3 H)
   cannot get there and two (3 + 3 a + b) cannot either: three it is, [3, a, b, a, 2] with 4 a + b >= 8190, and [3, 2048, 8, 2048, 2]
   has 8203 doubles for the forces and 12299 for the Jacobian (98392 bytes of the compute unit's 163840).  The grid depends on
   the CU count: min(ceil(n / frames per block), 8 blocks per CU).
3. The refusals of the Python methods that the other tests of this family do not cover: the same exception types as before."""

import ctypes

import pytest
import torch

import test_gpu_value_and_vjp_f64 as vj
from molann_amd import _capi, workloads as wl

pytestmark = pytest.mark.gpu
OK, E_NULL, E_DESC, E_STAGE, E_ALIGNMENT, E_UNSUPPORTED = 0, -1, -2, -5, -6, -7
BONDS = [(wl.BOND, [0, 1]), (wl.BOND, [1, 2]), (wl.BOND, [2, 3])]
ENTRIES = ("vjp", "jacobian", "metric")
POINTERS = {"vjp": ("x", "grad_out", "out", "second"), "jacobian": ("x", "out", "second"), "metric": ("x", "out", "second")}
N = 4


class _Args(object):
    """Valid arguments of the three entries for N frames of a plan: device buffers of the right sizes plus one spare double each."""

    def __init__(self, n_inp, dims, dev, d_feat=3):
        d_out = dims[-1] if dims else d_feat
        z = lambda count: torch.zeros(count + 1, dtype=torch.float64, device=dev)       # noqa: E731
        g = torch.Generator().manual_seed(n_inp)
        self.t = {"x": z(N * n_inp * 3), "grad_out": z(N * d_out), "out": z(N * d_out), "atom_w": z(n_inp),
                  "second": z(N * d_out * max(n_inp * 3, d_out))}
        self.t["x"][:N * n_inp * 3] = (torch.randn(N * n_inp * 3, generator=g, dtype=torch.float64) * 2.0).to(dev)
        self.layers = [(z(dims[i + 1] * dims[i]), z(dims[i + 1])) for i in range(len(dims) - 1)]
        self.ptr = dict((k, v.data_ptr()) for k, v in self.t.items())
        self.w = [w.data_ptr() for w, _ in self.layers]
        self.b = [b.data_ptr() for _, b in self.layers]


def _array(pointers):
    return (ctypes.c_void_p * max(1, len(pointers)))(*pointers)


def _raw(entry, handle, ptr, n, W, B, atom_w=None):
    """The C entry itself: W, B host arrays (or None), everything else addresses."""
    L = _capi.lib()
    s = torch.cuda.current_stream().cuda_stream
    if entry == "vjp":
        return L.molann_value_and_vjp_f64(handle, ptr["x"], ptr["grad_out"], n, W, B, ptr["out"], ptr["second"], s)
    if entry == "jacobian":
        return L.molann_value_and_jacobian_f64(handle, ptr["x"], n, W, B, ptr["out"], ptr["second"], s)
    return L.molann_value_and_metric_f64(handle, ptr["x"], n, W, B, atom_w, ptr["out"], ptr["second"], s)


def _with(d, **changes):
    d = dict(d)
    d.update(changes)
    return d


# ---- 1. return codes ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("head", [True, False], ids=["head", "no_head"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_return_codes(entry, head, hip_device):
    dims = [3, 8, 2] if head else []
    got, want = [], []

    def case(what, code, expected):
        got.append((what, code))
        want.append((what, expected))

    with torch.cuda.device(hip_device):
        plan = _capi.Plan(8, features=BONDS, layer_dims=dims or None, activation=_capi.ACT_TANH)
        bare = _capi.Plan(8, align_idx=[0, 1, 2, 3], ref_x=torch.zeros(4, 3))                 # no items
        a = _Args(8, dims, hip_device)
        h, p, W, B = plan._handle, a.ptr, _array(a.w), _array(a.b)
        null = dict((k, None) for k in p)
        case("null plan", _raw(entry, None, p, N, W, B), E_NULL)
        case("null plan, n < 0", _raw(entry, None, p, -1, W, B), E_NULL)
        case("n < 0", _raw(entry, h, p, -1, W, B), E_DESC)
        case("n < 0, null pointers", _raw(entry, h, null, -1, None, None), E_DESC)
        case("n == 0, null pointers", _raw(entry, h, null, 0, None, None), OK)
        case("n == 0, misaligned x", _raw(entry, h, _with(p, x=p["x"] + 4), 0, W, B), OK)
        for k in POINTERS[entry]:
            case("null " + k, _raw(entry, h, _with(p, **{k: None}), N, W, B), E_NULL)
            case(k + " off by 4", _raw(entry, h, _with(p, **{k: p[k] + 4}), N, W, B), E_ALIGNMENT)
        case("null x, out off by 4", _raw(entry, h, _with(p, x=None, out=p["out"] + 4), N, W, B), E_NULL)
        if entry == "metric":
            case("atom weights off by 4", _raw(entry, h, p, N, W, B, p["atom_w"] + 4), E_ALIGNMENT)
            case("atom weights off by 4, null W", _raw(entry, h, p, N, None, B, p["atom_w"] + 4), E_ALIGNMENT)
        case("no items", _raw(entry, bare._handle, p, N, W, B), E_STAGE)
        case("no items, x off by 4", _raw(entry, bare._handle, _with(p, x=p["x"] + 4), N, W, B), E_ALIGNMENT)
        case("no items, null W", _raw(entry, bare._handle, p, N, None, None), E_STAGE)
        case("null W, x off by 4", _raw(entry, h, _with(p, x=p["x"] + 4), N, None, B), E_ALIGNMENT)
        # without a head W and b are not read; with one: null arrays, a null layer, a misaligned layer, in the layers' order
        case("null W", _raw(entry, h, p, N, None, B), E_NULL if head else OK)
        case("null b", _raw(entry, h, p, N, W, None), E_NULL if head else OK)
        if head:
            case("null W[1]", _raw(entry, h, p, N, _array([a.w[0], None]), B), E_NULL)
            case("null b[0]", _raw(entry, h, p, N, W, _array([None, a.b[1]])), E_NULL)
            case("W[0] off by 4", _raw(entry, h, p, N, _array([a.w[0] + 4, a.w[1]]), B), E_ALIGNMENT)
            case("b[1] off by 4", _raw(entry, h, p, N, W, _array([a.b[0], a.b[1] + 4])), E_ALIGNMENT)
            case("W[0] off by 4, null b[1]", _raw(entry, h, p, N, _array([a.w[0] + 4, a.w[1]]), _array([a.b[0], None])), E_ALIGNMENT)
            case("null W[0], b[0] off by 4", _raw(entry, h, p, N, _array([None, a.w[1]]), _array([a.b[0] + 4, a.b[1]])), E_NULL)
        if entry == "metric":
            case("null atom weights", _raw(entry, h, p, N, W, B, None), OK)                 # legal: all ones
        torch.cuda.synchronize()
    print(got)
    assert got == want


# ---- 2. launch info ----------------------------------------------------------------------------------------------------------
INFO = {"vjp": "frames_value_vjp_f64_kernel (values + vjp in one launch; %d lanes per frame) grid=%d block=%d lds=%d",
        "jacobian": "frames_value_jac_f64_kernel (values + Jacobian in one launch; %d lanes per frame) grid=%d block=%d lds=%d",
        "metric": "frames_value_metric_f64_kernel (values + metric in one launch; %d lanes per frame) grid=%d block=%d lds=%d"}
MANY = [(wl.BOND, [i, j]) for i in range(12) for j in range(i + 1, 12)][:65]                 # 65 features of 12 atoms
# name: (atoms, items, head), then (lanes per frame, block, LDS bytes) of the forces and of the Jacobian; the metric's are the
# Jacobian's, None where it refuses the plan
GEOMETRY = {
    "8": ((8, BONDS, [3, 8, 2]), (8, 256, 6912), (8, 256, 11008), True),
    "9": ((9, BONDS, [3, 8, 2]), (16, 256, 3456), (16, 256, 5504), True),
    "17": ((17, BONDS, [3, 8, 2]), (32, 256, 1728), (32, 256, 2752), True),
    "33": ((33, BONDS, [3, 8, 2]), (64, 256, 864), (64, 256, 1376), True),
    "8_no_head": ((8, BONDS, []), (8, 256, 0), (8, 256, 0), True),
    "9_no_head": ((9, BONDS, []), (16, 256, 0), (16, 256, 0), True),
    "17_no_head": ((17, BONDS, []), (32, 256, 0), (32, 256, 0), True),
    "33_no_head": ((33, BONDS, []), (64, 256, 0), (64, 256, 0), True),
    "step_down": ((8, BONDS, [3, 682, 2]), (64, 128, 32784), (64, 128, 54608), True),
    "over_64k": ((8, BONDS, [3, 2048, 8, 2048, 2]), (64, 64, 65624), (64, 64, 98392), True),
    "65_features": ((12, MANY, []), (64, 256, 0), (64, 256, 0), False),
}


@pytest.mark.parametrize("name", sorted(GEOMETRY))
def test_launch_info(name, hip_device):
    (n_inp, items, dims), vjp, jac, metric_serves = GEOMETRY[name]
    cus = torch.cuda.get_device_properties(hip_device).multi_processor_count
    with torch.cuda.device(hip_device):
        plan = _capi.Plan(n_inp, features=items, layer_dims=dims or None, activation=_capi.ACT_TANH)
        a = _Args(n_inp, dims, hip_device, d_feat=len(items))
        W, B = [w[:-1] for w, _ in a.layers], [b[:-1] for _, b in a.layers]
        x, t = a.t["x"][:-1].view(N, n_inp, 3), a.t
        assert plan.supports_value_and_vjp_f64() and plan.supports_value_and_jacobian_f64()
        assert plan.supports_value_and_metric_f64() == metric_serves
        for entry, (lanes, block, lds) in (("vjp", vjp), ("jacobian", jac), ("metric", jac)):
            if entry == "vjp":
                plan.value_and_vjp_f64(x, t["grad_out"], W, B, t["out"], t["second"])
            elif entry == "jacobian":
                plan.value_and_jacobian_f64(x, W, B, t["out"], t["second"])
            elif metric_serves:
                plan.value_and_metric_f64(x, W, B, None, t["out"], t["second"])
            else:
                with pytest.raises(_capi.MolannHipError) as e:
                    plan.value_and_metric_f64(x, W, B, None, t["out"], t["second"])
                assert e.value.code == E_UNSUPPORTED
                assert plan.last_launch_info() == INFO["jacobian"] % (jac[0], grid, jac[1], jac[2])      # nothing was launched
                continue
            torch.cuda.synchronize()
            grid = min(-(-N // (block // lanes)), cus * 8)
            info = plan.last_launch_info()
            print(name, entry, info)
            assert info == INFO[entry] % (lanes, grid, block, lds)


# ---- 3. refusals of the Python methods the other tests leave out -------------------------------------------------------------
def test_python_refusals(hip_device):
    w, model, _ = vj._shared("C3", hip_device)
    pre = model.preprocessing_layer
    x = w.make_frames(5, seed=71).double().to(hip_device)
    d_out, d_feat, n_inp = w.out_dim(), pre.output_dimension(), w.n_atoms
    new = lambda *shape: torch.full(shape, float("nan"), dtype=torch.float64, device=hip_device)       # noqa: E731
    G, y, dx, f, M = new(5, d_out).fill_(1.0), new(5, d_out), new(5, n_inp, 3), new(5, d_feat), new(5, d_feat, d_feat)
    # value_and_vjp in float64: `into` of wrong count and device, grad_out of wrong device and dtype
    for bad in ((y,), (y, dx, dx), (y, None)):
        with pytest.raises(TypeError, match="into"):
            model.value_and_vjp(x, G, into=bad)
    for bad in ((y.cpu(), dx), (y, dx.cpu()), (y, dx[:, :-1])):
        with pytest.raises(ValueError, match="into"):
            model.value_and_vjp(x, G, into=bad)
    with pytest.raises(ValueError, match="grad_out"):
        model.value_and_vjp(x, G.cpu())
    with pytest.raises(ValueError, match="grad_out"):
        model.value_and_vjp(x, None)
    with pytest.raises(TypeError, match="grad_out"):
        model.value_and_vjp(x, G.to(torch.int64))
    # PreprocessingANN.value_and_metric: `into` of wrong count, dtype, shape, stride and device; float32 reference
    for bad in ((f,), (f.float(), M), (f, M.float())):
        with pytest.raises(TypeError, match="into"):
            pre.value_and_metric(x, into=bad)
    for bad in ((f[:4], M), (f, M[:, :-1]), (f, M.transpose(1, 2)[:, :, :4]), (f.t(), M), (f, M.cpu()), (f.cpu(), M)):
        with pytest.raises(ValueError, match="into"):
            pre.value_and_metric(x, into=bad)
    with pytest.raises(TypeError, match="weights"):
        pre.value_and_metric(x, weights=torch.ones(n_inp, device=hip_device))
    m32 = wl.build_model(w, hip_device, 0).requires_grad_(False)
    with pytest.raises(RuntimeError, match="ref_x must be float64"):
        m32.preprocessing_layer.value_and_metric(x)
    with pytest.raises(NotImplementedError, match="einsum"):
        pre.value_and_metric(x.cpu())
    with pytest.raises(NotImplementedError, match="fused plan"):
        model.value_and_vjp(x.cpu(), G.cpu())
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (y, dx, f, M)), "a refusal launched"
