"""Float64 values and the full Jacobian dy/dx in ONE launch (molann_value_and_jacobian_f64 -> frames_value_jac_f64_kernel,
MolANN.value_and_jacobian):

1. against torch.autograd.functional.jacobian of the float64 oracle.  The frames of a batch are independent, so the Jacobian of
   sum_f y[f] with respect to the batch holds every frame's own Jacobian (the same backward passes a per-frame call runs): jac
   within 1e-9 of each frame's Jacobian scale, y within 1e-10.  Only frames the suite's conditioning filter accepts are compared
   (test_gpu_jvp_plans._well, imported), at least half of every batch; the seeds are fixed and chosen so that this holds;
2. against the route it replaces: y bit-equal to value_and_vjp's, jac[:, k] within 1e-12 of scale of value_and_vjp under e_k;
3. dispatch boundaries (8/9, 16/17, 32/33 atoms or items: the lane group last_launch_info names), batch edges, one frame past a
   full grid for every lane group, and a guard that every lane group ran;
4. plan coverage, every activation, far frames sharing waves with near ones, degenerate alignment sets;
5. safety: x and the parameters are not written, two calls give the same bits, into= is filled in place, a captured launch replays
   the same bits; the error paths (no kernel launch)."""

import numpy as np
import pytest
import torch

import far_frames as ff
import test_gpu_jvp_plans as jvp
import test_gpu_random_backward as rb
import test_gpu_value_and_vjp_f64 as vj
from molann_amd import _capi, workloads as wl
from molann_amd.ann import MolANN

pytestmark = pytest.mark.gpu
KERNEL = "frames_value_jac_f64_kernel"
ANGLE, BOND, DIH, POS = wl.ANGLE, wl.BOND, wl.DIHEDRAL, wl.POSITION
REACHED = set()          # lane groups seen by the dispatch tests


# ---- helpers ---------------------------------------------------------------------------------------------------------------
def _build(case, dev):
    return case.build(dev).double().requires_grad_(False)


def _frames(case, n, seed, dev, regime="near"):
    return torch.from_numpy(ff.draw(regime, case.xyz, case.align or [], n, seed)).to(dev, torch.float64)


def _d_out(case):
    return case.mlp[-1] if case.mlp else case.d_feat()


def _call(model, x, into=None):
    """(y, jac, launch info): MolANN.value_and_jacobian, or the plan-level call on a features-only module."""
    if isinstance(model, MolANN):
        y, jac = model.value_and_jacobian(x, into=into)
        torch.cuda.synchronize()
        return y, jac, model.last_launch_info()
    plan = vj._feature_plan(model, x)
    assert plan.supports_value_and_jacobian_f64()
    if into is None:
        into = (torch.full((x.shape[0], plan.feature_dim), float("nan"), dtype=torch.float64, device=x.device),
                torch.full((x.shape[0], plan.feature_dim) + tuple(x.shape[1:]), float("nan"), dtype=torch.float64, device=x.device))
    with torch.cuda.device(x.device):
        plan.value_and_jacobian_f64(x, [], [], into[0], into[1])
    torch.cuda.synchronize()
    return into[0], into[1], plan.last_launch_info()


def _lanes(info):
    assert KERNEL in info, info
    return int(info.split("; ")[1].split(" lanes per frame")[0])


def _oracle(case, model, x):
    """(y [N, d_out], jac [N, d_out, n_inp, 3]) of the float64 oracle on the CPU (see the module docstring)."""
    f = jvp._oracle(case, model)
    xc = x.detach().cpu().double()
    J = torch.autograd.functional.jacobian(lambda v: f(v).sum(0), xc)
    return f(xc).detach(), J.permute(1, 0, 2, 3).contiguous()


def _against_oracle(case, model, x, y, jac, what):
    y_want, j_want = _oracle(case, model, x)
    ok = jvp._well(case, x, jvp._ref(model))
    n = x.shape[0]
    assert int(ok.sum()) * 2 >= n, (what, "too few well-conditioned frames", int(ok.sum()), n)
    yc, jc = y.detach().cpu(), jac.detach().cpu()
    assert jc.shape == j_want.shape and yc.shape == y_want.shape, (what, jc.shape, j_want.shape)
    ey, sy = float((yc[ok] - y_want[ok]).abs().max()), max(1.0, float(y_want[ok].abs().max()))
    s = j_want[ok].reshape(int(ok.sum()), -1).abs().amax(dim=1)
    s = s.clamp(min=max(1e-300, 1e-3 * float(s.max())))
    ej = float(((jc[ok] - j_want[ok]).reshape(int(ok.sum()), -1).abs().amax(dim=1) / s).max())
    print("%s: %d of %d frames, y err %.3e (scale %.3g), jac err %.3e of the frame's scale" % (what, int(ok.sum()), n, ey, sy, ej))
    assert ey <= 1e-10 * sy, (what, "y", ey, sy)
    jvp._close(jc[ok], j_want[ok], 1e-9, what)


def _against_vjp(model, x, y, jac, what):
    """y bit-equal to the VJP kernel's; every jac[:, k] within 1e-12 of scale of its dx under the cotangent e_k."""
    n, d_out = y.shape
    worst = 0.0
    for k in range(d_out):
        G = torch.zeros((n, d_out), dtype=torch.float64, device=x.device)
        G[:, k] = 1.0
        yv, dx, _ = vj._call(model, x, G)
        assert torch.equal(yv, y), (what, "y differs from value_and_vjp's")
        fin = torch.isfinite(dx).reshape(n, -1).all(1)
        assert bool(fin.any())
        scale = max(1e-300, float(dx[fin].abs().max()))
        err = float((jac[fin, k] - dx[fin]).abs().max())
        worst = max(worst, err / scale)
        assert err <= 1e-12 * scale, (what, k, err, scale)
    print("%s: against value_and_vjp, worst %.3e of scale" % (what, worst))


def _check(case, model, x, what, vjp=True):
    x0 = x.clone()
    y, jac, info = _call(model, x)
    assert KERNEL in info, info
    assert torch.equal(x, x0), (what, "x written")
    _against_oracle(case, model, x, y, jac, what)
    if vjp:
        _against_vjp(model, x, y, jac, what)
    return y, jac, info


# ---- 1. plan coverage --------------------------------------------------------------------------------------------------------
CHAIN = wl.synthetic_chain(n_atoms=40, step=1.4, seed=5)
SIX = [(DIH, [0, 1, 2, 3]), (DIH, [2, 3, 4, 5]), (ANGLE, [3, 4, 5]), (BOND, [0, 5])]      # 6 features; atoms 2-5 in several items


def _plan(name):
    """(case, lanes per frame)"""
    small = [(DIH, [0, 1, 2, 3]), (DIH, [2, 3, 4, 5]), (ANGLE, [3, 4, 5]), (BOND, [0, 5]), (POS, [4, 6])]   # vj._small_case's items
    if name == "no_head":
        return rb.Case(name, CHAIN[:12], small, [0, 2, 4, 6]), 16
    if name == "linear":                                   # a single Linear
        return rb.Case(name, CHAIN[:12], small, [0, 2, 4, 6], mlp=[12, 3]), 16
    if name == "quickstart":                               # [66, 5, 3] behind the 66 position features of 22 atoms, 3 align atoms
        return rb.Case(name, wl.ALA_DIPEPTIDE_XYZ, [(POS, list(range(22)))], [1, 4, 6], mlp=[66, 5, 3]), 64
    if name == "h6_32_8":
        return rb.Case(name, CHAIN[:8], SIX, None, mlp=[6, 32, 8], act="silu"), 32
    if name == "h6_64_64_8":
        return rb.Case(name, CHAIN[:8], SIX, [0, 1, 3, 6], mlp=[6, 64, 64, 8]), 64
    if name == "dout1":
        return rb.Case(name, CHAIN[:8], SIX, [0, 1, 3, 6], mlp=[6, 5, 1]), 8
    if name == "dout16":
        return rb.Case(name, CHAIN[:8], SIX, None, uav=True, mlp=[4, 7, 16], act="sigmoid"), 16
    if name == "pos_noalign":
        return rb.Case(name, CHAIN[:9], [(POS, [0, 3, 8]), (BOND, [1, 2])], None, mlp=[10, 4, 2]), 16
    if name == "pos_align":
        return rb.Case(name, CHAIN[:9], [(POS, [0, 3, 8]), (BOND, [1, 2])], [0, 2, 5, 7, 8], shift=(1.0, -2.0, 0.5), mlp=[10, 4, 2]), 16
    if name == "dup_align":                                # an alignment set that names an atom twice
        return rb.Case(name, CHAIN[:12], small, [0, 2, 4, 6, 9, 4]), 16
    if name == "untouched":                                # atoms 7.. are in no item and no alignment set
        return rb.Case(name, CHAIN[:30], small, [0, 2, 4, 6], mlp=[12, 5, 2]), 32
    raise KeyError(name)


PLANS = ["no_head", "linear", "quickstart", "h6_32_8", "h6_64_64_8", "dout1", "dout16", "pos_noalign", "pos_align", "dup_align",
         "untouched"]


@pytest.mark.parametrize("name", PLANS)
def test_plan_coverage(name, hip_device):
    case, G = _plan(name)
    model = _build(case, hip_device)
    x = _frames(case, 19, len(name), hip_device)
    y, jac, info = _check(case, model, x, name)
    assert _lanes(info) == G, info
    assert tuple(jac.shape) == (19, _d_out(case), len(case.xyz), 3)
    untouched = sorted(set(range(len(case.xyz))) - case.touched())
    if name == "untouched":
        assert len(untouched) == 23
    if untouched:                                          # exactly zero in a buffer prefilled with NaN
        into = (torch.full_like(y, float("nan")), torch.full_like(jac, float("nan")))
        y2, jac2, _ = _call(model, x, into=into)
        assert jac2 is into[1] and torch.equal(jac2, jac) and torch.equal(y2, y)
        assert float(jac2[:, :, untouched].abs().max()) == 0.0
        assert not bool((jac2[:, :, untouched] != 0).any())


def _workload_case(name):
    w, model, (feats, uav, al) = vj._shared(name, torch.device("cuda", torch.cuda.current_device()))
    case = rb.Case(name, w.ref_xyz, feats, al, uav, list(w.mlp_dims), "tanh")
    return w, model, case


@pytest.mark.parametrize("name,n,G", [("C3", 33, None), ("P1", 9, 64), ("C4", 4, 64)])
def test_workloads(name, n, G, hip_device):
    """The 22-atom flagship (d_out 8), the 166-atom P1 and a 5000-atom frame with the head [85, 128, 64, 8]."""
    w, model, case = _workload_case(name)
    if name == "C4":
        assert w.n_atoms == 5000
    if name == "P1":
        assert w.n_atoms == 166
    x = w.make_frames(n, seed=7).double().to(hip_device)
    y, jac, info = _check(case, model, x, name, vjp=name != "C4")
    if G is not None:
        assert _lanes(info) == G, info
    if name == "C4":                                       # two outputs against the VJP route
        for k in (0, 7):
            Gk = torch.zeros((n, 8), dtype=torch.float64, device=hip_device)
            Gk[:, k] = 1.0
            yv, dx, _ = vj._call(model, x, Gk)
            assert torch.equal(yv, y)
            assert float((jac[:, k] - dx).abs().max()) <= 1e-12 * float(dx.abs().max())
    untouched = sorted(set(range(w.n_atoms)) - {a - 1 for a in w.touched_atoms()})
    if untouched:
        assert float(jac[:, :, untouched].abs().max()) == 0.0


@pytest.mark.parametrize("act", sorted(rb.ACTS) + ["elu", "softplus", "gelu"])
def test_every_activation(act, hip_device):
    """All nine activations on one small head."""
    mods = dict(rb.ACTS, elu=torch.nn.ELU, softplus=torch.nn.Softplus, gelu=torch.nn.GELU)
    assert len(mods) == 9
    case = rb.Case("act_" + act, CHAIN[:8], SIX, [0, 1, 3, 6], mlp=[6, 5, 4, 3])
    pp = case.build(hip_device).preprocessing_layer
    torch.manual_seed(3)
    from molann_amd.ann import create_sequential_nn
    model = MolANN(pp, create_sequential_nn([6, 5, 4, 3], activation=mods[act]())).to(hip_device).double().requires_grad_(False)
    x = _frames(case, 17, 23, hip_device)
    _check(case, model, x, act)


# ---- 2. dispatch boundaries ------------------------------------------------------------------------------------------------
def _g(w):
    return 8 if w <= 8 else 16 if w <= 16 else 32 if w <= 32 else 64


def _boundary(kind, k, head):
    """`atoms`: k atoms, 4 items; `items`: 8 atoms, k one-column items (bonds, then angles).  head: [d_feat, 3, 2], or none."""
    if kind == "atoms":
        feats = [(DIH, [0, 1, 2, 3]), (ANGLE, [k - 1, k - 2, k - 3]), (BOND, [k - 1, 0]), (POS, [k // 2])]
        xyz, al = CHAIN[:k], [0, 2, 5, k - 1]
    else:
        pairs = [(i, j) for i in range(8) for j in range(i + 1, 8)]
        feats = [(BOND, list(p)) for p in pairs[:min(k, 28)]] + [(ANGLE, [i, i + 1, i + 2]) for i in range(6)][:max(0, k - 28)]
        assert len(feats) == k
        xyz, al = CHAIN[:8], ([0, 3, 4, 7] if k % 2 else None)
    case = rb.Case("%s%d" % (kind, k), xyz, feats, al)
    if head:
        case.mlp = [case.d_feat(), 3, 2]
    return case, _g(max(len(xyz), case.n_items(), case.d_feat() if head else 0))


@pytest.mark.parametrize("head", [False, True], ids=["features", "head"])
@pytest.mark.parametrize("k", [8, 9, 16, 17, 32, 33])
@pytest.mark.parametrize("kind", ["atoms", "items"])
def test_dispatch_boundaries(kind, k, head, hip_device):
    case, G = _boundary(kind, k, head)
    if kind == "atoms":
        assert G == _g(k)
    model = _build(case, hip_device)
    fpb = 4 * (64 // G)                                    # frames per 256-thread block
    for n in sorted({1, 64 // G - 1, 64 // G + 1, fpb - 1, fpb + 1} - {0}):
        x = _frames(case, n, 100 * k + n, hip_device)
        _, _, info = _check(case, model, x, (case.name, head, n), vjp=(n == fpb + 1 and (head or k <= 9)))
        assert _lanes(info) == G, (info, G)
        assert "block=256" in info, info
    REACHED.add(G)


@pytest.mark.parametrize("G", [8, 16, 32, 64])
def test_one_frame_past_a_full_grid(G, hip_device):
    """num_cus x 8 blocks of 256 / G frames, and one more: the grid strides.  A d_out = 2 head keeps the Jacobian small."""
    case, g = _boundary("atoms", {8: 8, 16: 16, 32: 32, 64: 33}[G], True)
    assert g == G
    model = _build(case, hip_device)
    cus = torch.cuda.get_device_properties(hip_device).multi_processor_count
    n = cus * 8 * 4 * (64 // G) + 1
    base = _frames(case, 512, 40 + G, hip_device)
    x = base.repeat((n + 511) // 512, 1, 1)[:n].contiguous()
    x[-1] = _frames(case, 1, 41 + G, hip_device)[0]
    y, jac, info = _call(model, x)
    assert _lanes(info) == G and "grid=%d " % (cus * 8) in info, info
    rows = torch.tensor(sorted(set(range(4)) | set(range(n - 4, n)) |
                               set(np.random.default_rng(G).choice(n, size=24, replace=False).tolist())), device=hip_device)
    _against_oracle(case, model, x[rows], y[rows], jac[rows], (case.name, n))
    yt, jt, _ = _call(model, x[-700:].contiguous())
    assert torch.equal(y[-700:], yt) and torch.equal(jac[-700:], jt), "tail of a batch past one grid"
    assert torch.equal(jac[:512], jac[512:1024]) and torch.equal(y[:512], y[512:1024])
    REACHED.add(G)


def test_every_lane_group_ran(request):
    ran = {i.name.split("[")[0] for i in request.session.items}
    if not {"test_dispatch_boundaries", "test_one_frame_past_a_full_grid"} <= ran:
        pytest.skip("the dispatch tests were deselected")
    assert REACHED == {8, 16, 32, 64}, REACHED


# ---- 3. far frames and degenerate sets ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pos_align", "quickstart", "h6_64_64_8"])
def test_far_frames_share_waves_with_near_frames(name, hip_device):
    """Frames translated by 100 and 1000 A (far_frames' "offset") in one wave with near ones: a near frame's rows do not change
    with its wave-mates, bit for bit; the whole batch against the oracle."""
    case, _ = _plan(name)
    model = _build(case, hip_device)
    n = 48
    near = ff.draw("near", case.xyz, case.align, n, seed=len(name))
    lab = ["offset" if i % 4 == 1 else "near" for i in range(n)]
    mixed = ff.compose(lab, case.xyz, case.align, seed=7, base=near)
    moved = np.abs(mixed.reshape(n, -1)).max(1)
    assert (moved[1::4] > 50.0).all() and moved[1::8].max() < 200.0 and moved[5::8].min() > 500.0      # 100 A and 1000 A
    xn = torch.from_numpy(near).to(hip_device, torch.float64)
    xm = torch.from_numpy(mixed).to(hip_device, torch.float64)
    yn, jn, _ = _call(model, xn)
    yn, jn = yn.clone(), jn.clone()
    ym, jm, _ = _check(case, model, xm, name + " mixed", vjp=False)
    rows = torch.tensor([i for i in range(n) if lab[i] == "near"], device=hip_device)
    assert torch.equal(ym[rows], yn[rows]) and torch.equal(jm[rows], jn[rows]), (name, "a near frame changed with its wave-mates")


@pytest.mark.parametrize("name", ["pos_align", "quickstart"])
def test_degenerate_alignment_sets_give_finite_output(name, hip_device):
    case, _ = _plan(name)
    model = _build(case, hip_device)
    n = 24
    near = ff.draw("near", case.xyz, case.align, n, seed=5)
    lab = ["degenerate" if i % 3 == 1 else "near" for i in range(n)]
    x = torch.from_numpy(ff.compose(lab, case.xyz, case.align, seed=31, base=near)).to(hip_device, torch.float64)
    y, jac, _ = _call(model, x)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(jac).all())
    yn, jn, _ = _call(model, torch.from_numpy(near).to(hip_device, torch.float64))
    rows = torch.tensor([i for i in range(n) if lab[i] == "near"], device=hip_device)
    assert torch.equal(y[rows], yn[rows]) and torch.equal(jac[rows], jn[rows])


# ---- 4. safety properties ------------------------------------------------------------------------------------------------------
def test_inputs_are_not_written_and_two_calls_give_the_same_bits(hip_device):
    w, model, case = _workload_case("C3")
    x = w.make_frames(4097, seed=41).double().to(hip_device)
    x0 = x.clone()
    params = [p.detach().clone() for p in model.parameters()]
    ref0 = rb._align_layer(model).ref_x.detach().clone()
    y1, j1, info = _call(model, x)
    y1, j1 = y1.clone(), j1.clone()
    y2, j2, _ = _call(model, x)
    assert KERNEL in info and info.count("_kernel") == 1, info
    assert torch.equal(y1, y2) and torch.equal(j1, j2)
    assert bool(torch.isfinite(j1).all())
    assert torch.equal(x, x0) and torch.equal(rb._align_layer(model).ref_x, ref0)
    assert all(torch.equal(p, q) for p, q in zip(model.parameters(), params))


def test_into_buffers_are_filled_in_place(hip_device):
    w, model, case = _workload_case("C3")
    x = w.make_frames(5, seed=51).double().to(hip_device)
    y, jac, _ = _call(model, x)
    y2, j2 = torch.full_like(y, float("nan")), torch.full_like(jac, float("nan"))
    p = (y2.data_ptr(), j2.data_ptr())
    r = model.value_and_jacobian(x, into=(y2, j2))
    torch.cuda.synchronize()
    assert r[0] is y2 and r[1] is j2 and (y2.data_ptr(), j2.data_ptr()) == p
    assert torch.equal(y2, y) and torch.equal(j2, jac)
    flat = torch.full((jac.numel(),), float("nan"), dtype=torch.float64, device=hip_device)      # numel is what counts
    model.value_and_jacobian(x, into=(y2, flat))
    torch.cuda.synchronize()
    assert torch.equal(flat.view_as(jac), jac)


def test_a_captured_launch_replays_the_same_bits(hip_device):
    w, model, case = _workload_case("C3")
    xs = w.make_frames(64, seed=61).double().to(hip_device)
    y, jac, _ = _call(model, xs)
    y, jac = y.clone(), jac.clone()
    x = torch.zeros_like(xs)
    yb, jb = torch.empty_like(y), torch.empty_like(jac)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(device=hip_device)
    s.wait_stream(torch.cuda.current_stream(hip_device))
    with torch.cuda.stream(s):
        model.value_and_jacobian(x, into=(yb, jb))          # warm: plan and reference are in place before the capture
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            model.value_and_jacobian(x, into=(yb, jb))
    torch.cuda.current_stream(hip_device).wait_stream(s)
    for _ in range(2):
        x.copy_(xs)
        yb.fill_(float("nan"))
        jb.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(yb, y) and torch.equal(jb, jac)


# ---- 5. error paths (no kernel launch) -------------------------------------------------------------------------------------------
def test_error_paths(hip_device):
    w, model, case = _workload_case("C3")
    x = w.make_frames(5, seed=71).double().to(hip_device)
    d_out = w.out_dim()
    y = torch.empty((5, d_out), dtype=torch.float64, device=hip_device)
    jac = torch.empty((5, d_out, w.n_atoms, 3), dtype=torch.float64, device=hip_device)
    with pytest.raises(TypeError, match=r"model\.double\(\)"):
        model.value_and_jacobian(x.float())
    with pytest.raises(TypeError):
        model.value_and_jacobian(x, into=(y.float(), jac))
    with pytest.raises(TypeError):
        model.value_and_jacobian(x, into=(y, jac.float()))
    with pytest.raises(TypeError):
        model.value_and_jacobian(x, into=(y,))
    with pytest.raises(ValueError):
        model.value_and_jacobian(x, into=(y[:4], jac))
    with pytest.raises(ValueError):
        model.value_and_jacobian(x, into=(y, jac[:, :-1]))
    with pytest.raises(ValueError):
        model.value_and_jacobian(x, into=(y, jac.transpose(2, 3)))
    with pytest.raises(ValueError):
        model.value_and_jacobian(x, into=(y, jac.cpu()))
    with pytest.raises(ValueError):
        model.value_and_jacobian(x, into=(y.cpu(), jac))
    m32 = wl.build_model(w, hip_device, 0).requires_grad_(False)
    with pytest.raises(RuntimeError, match="float64"):
        m32.value_and_jacobian(x)                          # float32 parameters, float64 x
    with pytest.raises(NotImplementedError, match="eye"):
        model.value_and_jacobian(x.cpu())
    y0, j0 = model.value_and_jacobian(x[:0])
    assert tuple(y0.shape) == (0, d_out) and tuple(j0.shape) == (0, d_out, w.n_atoms, 3)
    assert y0.dtype == torch.float64 and j0.dtype == torch.float64 and y0.device == x.device and j0.device == x.device
    if hasattr(torch.ops.molann, "value_and_jacobian"):
        with pytest.raises(TypeError):
            torch.ops.molann.value_and_jacobian_h(x.float(), model._fast["handle"], rb._align_layer(model).ref_x,
                                                  [lin.weight for lin in model._fast["linears"]],
                                                  [lin.bias for lin in model._fast["linears"]], [])


def test_a_plan_the_geometry_refuses(hip_device):
    """2 d_out max_w doubles past the 160 KiB of a compute unit: supports_value_and_jacobian_f64 says no, the call returns
    MOLANN_E_UNSUPPORTED and the method names the route that remains; the VJP kernel still serves the plan."""
    with torch.cuda.device(hip_device):
        p = _capi.Plan(8, features=[(BOND, [0, 1])], layer_dims=[1, 512, 64], activation=0)
        assert p.supports_value_and_vjp_f64() and not p.supports_value_and_jacobian_f64()
        x = torch.zeros((1, 8, 3), dtype=torch.float64, device=hip_device)
        Ws = [torch.zeros((512, 1), dtype=torch.float64, device=hip_device), torch.zeros((64, 512), dtype=torch.float64, device=hip_device)]
        bs = [torch.zeros(512, dtype=torch.float64, device=hip_device), torch.zeros(64, dtype=torch.float64, device=hip_device)]
        y = torch.empty((1, 64), dtype=torch.float64, device=hip_device)
        jac = torch.empty((1, 64, 8, 3), dtype=torch.float64, device=hip_device)
        with pytest.raises(_capi.MolannHipError) as e:
            p.value_and_jacobian_f64(x, Ws, bs, y, jac)
        assert e.value.code == _capi.E_UNSUPPORTED
        small = _capi.Plan(8, features=[(BOND, [0, 1])], layer_dims=[1, 16, 4], activation=0)
        assert small.supports_value_and_jacobian_f64()
        none = _capi.Plan(8, align_idx=[0, 1, 2, 3], ref_x=torch.zeros(4, 3))       # no items: nothing to differentiate
        assert not none.supports_value_and_jacobian_f64()
    case = rb.Case("refused", CHAIN[:8], [(BOND, [0, 1])], None, mlp=[1, 512, 64])
    model = _build(case, hip_device)
    with pytest.raises(NotImplementedError, match="eye"):
        model.value_and_jacobian(_frames(case, 2, 1, hip_device))
