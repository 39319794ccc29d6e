"""Values and forces of frames too large for the lane kernels in ONE launch (molann_value_and_vjp_f32 -> molann_group_vjp):
against the reference's fixture, eager autograd, the float64 oracle on random plans, the Jacobian of a frame, NaN frames,
side streams and graph capture, GraphedForces, and the plans it still refuses."""

import numpy as np
import pytest
import torch

import test_gpu_random_backward as rb
from molann_amd import _capi, workloads as wl
from molann_amd.ann import MolANN, PreprocessingANN

pytestmark = pytest.mark.gpu
KERNEL = "molann_group_vjp"


def _p1(dev):
    from build_util import workload_model
    return workload_model(wl.get_workload("P1"), dev).requires_grad_(False)


def _eager(model, x, dy):
    xe = x.clone().requires_grad_(True)
    ye = model(xe)
    (dxe,) = torch.autograd.grad(ye, xe, dy)
    return ye.detach(), dxe


def _close_to_eager(y, dx, ye, dxe, what):
    ey = float((y - ye).abs().max())
    ed = float((dx - dxe).abs().max())
    assert ey <= 2e-6 * max(1.0, float(ye.abs().max())), (what, "y", ey)
    assert ed <= 1e-6 * max(1.0, float(dxe.abs().max())), (what, "dx", ed)


def test_reference_fixture(hip_device):
    """grad_molann_P1: y and dx against the reference's float64 autograd with the suite's bounds."""
    import os
    from test_gpu_backward import GOLDEN_DIR, _model_from_golden
    d = np.load(os.path.join(GOLDEN_DIR, "grad_molann_P1.npz"))
    model = _model_from_golden(d, hip_device).requires_grad_(False)
    x = torch.from_numpy(d["x"]).to(hip_device)
    G = torch.from_numpy(d["G"]).to(hip_device)
    y, dx = model.value_and_vjp(x, G)
    torch.cuda.synchronize()
    assert KERNEL in model.last_launch_info(), model.last_launch_info()
    assert float(np.abs(y.cpu().double().numpy() - d["out_f64"]).max()) <= 1e-5
    gx = d["gx_f64"]
    assert float(np.abs(dx.cpu().double().numpy() - gx).max()) <= 2e-4 * float(np.abs(gx).max())


@pytest.mark.parametrize("n", [1, 7, 8, 9, 63, 64, 65, 1000, 100003])
def test_p1_against_eager_autograd(n, hip_device):
    """Short rounds, tile edges, a multi-block grid; the module, the ctypes plan and into= give the same bits; x is never written."""
    model = _p1(hip_device)
    w = wl.get_workload("P1")
    x = w.make_frames(n, seed=60 + n).to(hip_device)
    x0 = x.clone()
    dy = torch.randn((n, w.out_dim()), generator=torch.Generator().manual_seed(n)).to(hip_device)
    ye, dxe = _eager(model, x, dy)
    y, dx = model.value_and_vjp(x, dy)
    torch.cuda.synchronize()
    assert KERNEL in model.last_launch_info(), model.last_launch_info()
    _close_to_eager(y, dx, ye, dxe, n)
    plan = model.plan_for(x)
    assert plan.supports_value_and_vjp()
    y2, dx2 = torch.full_like(y, float("nan")), torch.full_like(dx, float("nan"))
    with torch.cuda.device(hip_device):
        plan.value_and_vjp(x, dy, y2, dx2)
    torch.cuda.synchronize()
    assert KERNEL in plan.last_launch_info()
    assert torch.equal(y2, y) and torch.equal(dx2, dx)
    y3, dx3 = torch.empty_like(y), torch.empty_like(dx)
    r = model.value_and_vjp(x, dy, into=(y3, dx3))
    assert r[0].data_ptr() == y3.data_ptr() and r[1].data_ptr() == dx3.data_ptr()
    assert torch.equal(y3, y) and torch.equal(dx3, dx)
    assert torch.equal(x, x0)


def test_ctypes_branch_checks_its_arguments(hip_device, monkeypatch):
    """The ctypes branch (no operator library) checks grad_out and into= as the operator does."""
    from molann_amd import ann
    model = _p1(hip_device)
    w = wl.get_workload("P1")
    x = w.make_frames(5, seed=1).to(hip_device)
    dy = torch.randn((5, w.out_dim()), device=hip_device)
    monkeypatch.setattr(ann, "_run_op", lambda: None)
    model.__dict__.pop("_fast", None)
    y, dx = model.value_and_vjp(x, dy)
    assert KERNEL in model.plan_for(x).last_launch_info()
    ye, dxe = _eager(model, x, dy)
    _close_to_eager(y, dx, ye, dxe, "ctypes")
    with pytest.raises(ValueError):
        model.value_and_vjp(x, dy[:4])
    with pytest.raises(ValueError):
        model.value_and_vjp(x, dy.cpu())
    with pytest.raises(TypeError):
        model.value_and_vjp(x, dy, into=(y.double(), dx))
    with pytest.raises(ValueError):
        model.value_and_vjp(x, dy, into=(y[:4], dx))
    with pytest.raises(ValueError):
        model.value_and_vjp(x, dy, into=(y, dx.transpose(1, 2)))
    model.__dict__.pop("_fast", None)


# ---- random plans against the float64 oracle ------------------------------------------------------------------------------
def _case(seed, n_inp, n_align, n_dih, n_pos, dims, act, uav=False, dup=False, shift=None, no_align=False):
    rng = np.random.default_rng(seed)
    xyz = rb._chain(n_inp, seed)
    feats = []
    for _ in range(n_dih):
        a = int(rng.integers(0, n_inp - 3))
        feats.append((rb.DIH, [a, a + 1, a + 2, a + 3]))
    a = int(rng.integers(0, n_inp - 2))
    feats.append((rb.ANGLE, [a, a + 1, a + 2]))
    a = int(rng.integers(0, n_inp - 1))
    feats.append((rb.BOND, [a, int(rng.integers(0, n_inp))] if a + 1 >= n_inp else [a, a + 1]))
    if n_pos:
        feats.append((rb.POS, sorted(rng.choice(n_inp, size=n_pos, replace=False).tolist())))
    align = None
    if not no_align:
        align = sorted(rng.choice(n_inp, size=n_align, replace=False).tolist())
        if dup:
            align.append(align[len(align) // 2])
    c = rb.Case("vjp%d" % seed, xyz, feats, align=align, uav=uav, mlp=dims, act=act, shift=shift)
    if dims:
        c.mlp = [c.d_feat()] + dims
    return c


CASES = [
    # (seed, n_inp, n_align, dihedrals, positions, hidden + out, activation, use_angle_value, duplicated, shift, no alignment)
    (1, 40, 12, 4, 40, None, "tanh", False, False, None, False),       # 130 feature columns: past the lane kernels' 128
    (2, 166, 42, 6, 2, [24, 6], "relu", True, True, None, False),
    (3, 300, 30, 5, 0, [16, 16, 4], "sigmoid", False, False, (30.0, -12.0, 7.0), False),
    (4, 700, 80, 3, 3, [32], "identity", True, False, None, True),
    (5, 1024, 120, 7, 0, [20, 20, 20, 3], "silu", False, True, None, False),
    (6, 512, 16, 4, 1, [32, 5], "leaky_relu", True, False, (-50.0, 3.0, 100.0), False),
]


@pytest.mark.parametrize("spec", CASES, ids=[str(c[0]) for c in CASES])
def test_random_plans_against_oracle(spec, hip_device):
    seed, n_inp, n_align, n_dih, n_pos, dims, act, uav, dup, shift, no_align = spec
    case = _case(seed, n_inp, n_align, n_dih, n_pos, dims, act, uav=uav, dup=dup, shift=shift, no_align=no_align)
    _check_against_oracle(case, hip_device, seed)


def _check_against_oracle(case, dev, seed, batches=(1, 37, 300), expect_b=None):
    model = case.build(dev).requires_grad_(False)
    al = rb._align_layer(model)
    ref = al.ref_x.detach().cpu().double() if al is not None else None
    checked = 0
    for n in batches:
        x = case.frames(n, seed=1000 * seed + n, dev=dev)
        G, sel, Gs = rb._cotangent(case, model, x, ref, n, seed=7 * seed + n)
        want = rb._oracle(case, model, x[sel], Gs, ref)
        if not torch.isfinite(want[1]).all() or float(want[1].abs().max()) > 1e4:
            continue
        if isinstance(model, MolANN):
            y, dx = model.value_and_vjp(x, G)
            plan = model
        else:
            model(x.clone().requires_grad_(True))          # (creates the module's ctypes plan)
            plan = model._plans()[("features", dev.index)].plan
            y, dx = torch.empty((n, case.d_feat()), device=dev), torch.empty_like(x)
            with torch.cuda.device(dev):
                plan.value_and_vjp(x, G, y, dx)
        torch.cuda.synchronize()
        info = plan.last_launch_info()
        assert KERNEL in info, (case, info)
        if expect_b is not None:
            assert "%s<B=%d>" % (KERNEL, expect_b) in info, (case, info)
        untouched = sorted(set(range(len(case.xyz))) - case.touched())
        rb._check(case, ("value_and_vjp", n, info), y, dx, [], sel, (want[0], want[1], []), rb._out_tol(case), 2e-4, untouched)
        checked += 1
    assert checked > 0
    return model


def test_features_only_plan(hip_device):
    """NL = 0: y = the features, through Plan.value_and_vjp."""
    case = _case(11, 250, 25, 6, 2, None, "tanh")
    model = _check_against_oracle(case, hip_device, 11)
    assert isinstance(model, PreprocessingANN)


@pytest.mark.parametrize("n_items,b", [(20, 8), (50, 4), (90, 2)])
def test_frames_per_round(n_items, b, hip_device):
    """B = 8, 4 and 2 are all reached (items per frame: dihedrals along a 400-atom chain)."""
    case = _case(20 + b, 400, 30, n_items - 2, 0, None, "tanh")
    _check_against_oracle(case, hip_device, 20 + b, batches=(1, 70), expect_b=b)


def test_5000_atom_chain(hip_device):
    """A 5000-atom frame, 8 dihedrals (d = 16 with use_angle_value False), a [16, 32, 8] head, 200 alignment atoms spread over the
    chain.  Both this kernel and the three-launch backward of eager autograd (frames_wave_bwd_gather_kernel above 1024 atoms) form
    the atoms about the centroid in float32; atoms ~100 A from it carry ~1e-5 A of rounding that the dihedrals amplify, and the
    two kernels sum the covariance in different orders: measured 1.3e-5 apart at |dx| 1.8 (not the 1e-6 that P1 holds), and this
    kernel 7.7e-5 from the float64 oracle against 2e-4 * 0.28.  So the check is against the oracle with the suite's rule for such
    cases (test_gpu_backward._close): 2e-4 of the gradient's scale, or no further than twice the three-launch backward is."""
    rng = np.random.default_rng(5)
    xyz = rb._chain(5000, 5)
    feats = [(rb.DIH, [a, a + 1, a + 2, a + 3]) for a in sorted(rng.choice(4990, size=8, replace=False).tolist())]
    align = sorted(rng.choice(5000, size=200, replace=False).tolist())
    case = rb.Case("chain5000", xyz, feats, align=align, mlp=[16, 32, 8], act="tanh")
    model = case.build(hip_device).requires_grad_(False)
    ref = rb._align_layer(model).ref_x.detach().cpu().double()
    for n in (1, 100):
        x = case.frames(n, seed=5000 + n, dev=hip_device)
        G, sel, Gs = rb._cotangent(case, model, x, ref, n, seed=35 + n)
        y_want, gx_want, _ = rb._oracle(case, model, x[sel], Gs, ref)
        ye, dxe = _eager(model, x, G)
        y, dx = model.value_and_vjp(x, G)
        torch.cuda.synchronize()
        assert KERNEL in model.last_launch_info(), model.last_launch_info()
        assert rb._err(y[sel], y_want) <= 2e-5 * max(1.0, float(y_want.abs().max()))
        own = rb._err(dxe[sel], gx_want)
        assert rb._err(dx[sel], gx_want) <= max(2e-4 * float(gx_want.abs().max()), 2.0 * own), (n, own)
        rest = torch.ones(n, dtype=torch.bool, device=hip_device)
        rest[sel] = False
        if bool(rest.any()):
            assert float(dx[rest].abs().max()) == 0.0


def test_jacobian_of_one_frame(hip_device):
    model = _p1(hip_device)
    w = wl.get_workload("P1")
    d_out = w.out_dim()
    x1 = w.make_frames(1, seed=9).to(hip_device)
    yj, J = model.value_and_vjp(x1.expand(d_out, -1, -1).contiguous(), torch.eye(d_out, device=hip_device))
    torch.cuda.synchronize()
    assert KERNEL in model.last_launch_info()
    xe = x1.clone().requires_grad_(True)
    ye = model(xe)
    assert float((yj - ye.detach()).abs().max()) <= 2e-6 * max(1.0, float(ye.abs().max()))
    for k in range(d_out):
        (gk,) = torch.autograd.grad(ye[0, k], xe, retain_graph=True)
        assert float((J[k] - gk[0]).abs().max()) <= 1e-6 * max(1.0, float(gk.abs().max()))


def test_nan_frame_poisons_only_its_rows(hip_device):
    model = _p1(hip_device)
    w = wl.get_workload("P1")
    n, bad = 70, 33
    x = w.make_frames(n, seed=2).to(hip_device)
    dy = torch.randn((n, w.out_dim()), generator=torch.Generator().manual_seed(2)).to(hip_device)
    y0, dx0 = model.value_and_vjp(x, dy)
    y0, dx0 = y0.clone(), dx0.clone()
    xb = x.clone()
    xb[bad, 5] = float("nan")
    y, dx = model.value_and_vjp(xb, dy)
    torch.cuda.synchronize()
    keep = torch.ones(n, dtype=torch.bool, device=hip_device)
    keep[bad] = False
    assert torch.equal(y[keep], y0[keep]) and torch.equal(dx[keep], dx0[keep])
    assert torch.isnan(y[bad]).all()


def test_side_stream_and_graph_capture(hip_device):
    model = _p1(hip_device)
    w = wl.get_workload("P1")
    n = 64
    x = w.make_frames(n, seed=3).to(hip_device)
    dy = torch.randn((n, w.out_dim()), generator=torch.Generator().manual_seed(3)).to(hip_device)
    y0, dx0 = [t.clone() for t in model.value_and_vjp(x, dy)]
    side = torch.cuda.Stream(device=hip_device)
    side.wait_stream(torch.cuda.current_stream(hip_device))
    with torch.cuda.stream(side):
        y1, dx1 = model.value_and_vjp(x, dy)
    torch.cuda.current_stream(hip_device).wait_stream(side)
    torch.cuda.synchronize()
    assert KERNEL in model.last_launch_info()
    assert torch.equal(y1, y0) and torch.equal(dx1, dx0)
    sx, sdy = x.clone(), dy.clone()
    sy, sdx = torch.empty_like(y0), torch.empty_like(dx0)
    model.value_and_vjp(sx, sdy, into=(sy, sdx))     # warm: the kernel is built outside the capture
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        model.value_and_vjp(sx, sdy, into=(sy, sdx))
    x2 = w.make_frames(n, seed=4).to(hip_device)
    dy2 = torch.randn((n, w.out_dim()), generator=torch.Generator().manual_seed(4)).to(hip_device)
    sx.copy_(x2)
    sdy.copy_(dy2)
    g.replay()
    torch.cuda.synchronize()
    y2, dx2 = model.value_and_vjp(x2, dy2)
    torch.cuda.synchronize()
    assert torch.equal(sy, y2) and torch.equal(sdx, dx2)


def test_refusals(hip_device):
    """P2 (a head 126 wide), an ELU head and a bf16 head: no single launch, and supports_value_and_vjp says so."""
    from build_util import workload_model
    w = wl.get_workload("P2")
    model = workload_model(w, hip_device).requires_grad_(False)
    x = w.make_frames(4, seed=1).to(hip_device)
    dy = torch.randn((4, w.out_dim()), device=hip_device)
    with pytest.raises((RuntimeError, NotImplementedError, _capi.MolannHipError)):
        model.value_and_vjp(x, dy)
    assert not model.plan_for(x).supports_value_and_vjp()
    for act, prec in ((_capi.ACT_ELU, _capi.MLP_F32), (_capi.ACT_TANH, _capi.MLP_BF16)):
        with torch.cuda.device(hip_device):
            plan = _capi.Plan(166, align_idx=list(range(2, 166, 4)), ref_x=torch.from_numpy(np.asarray(w.ref_xyz)[2:166:4]).float(),
                              features=[(wl.DIHEDRAL, [i, i + 1, i + 2, i + 3]) for i in range(0, 64, 8)], layer_dims=[16, 32, 8],
                              activation=act, mlp_precision=prec)
        assert not plan.supports_value_and_vjp()
        xs = w.make_frames(2, seed=1).to(hip_device)
        with pytest.raises(_capi.MolannHipError) as e:
            with torch.cuda.device(hip_device):
                plan.value_and_vjp(xs, torch.zeros((2, 8), device=hip_device), torch.empty((2, 8), device=hip_device), torch.empty_like(xs))
        assert e.value.code == _capi.E_UNSUPPORTED


def test_graphed_forces_uses_one_launch(hip_device):
    from molann_amd.graph import GraphedForces
    model = _p1(hip_device)
    w = wl.get_workload("P1")
    for n in (1, 64):
        x = w.make_frames(n, seed=6).to(hip_device)
        dy = torch.randn((n, w.out_dim()), generator=torch.Generator().manual_seed(6)).to(hip_device)
        g = GraphedForces(model, x)
        assert "frames_group_bwd_kernel" in g._plan.last_launch_info()      # the backward graph was captured last
        y, dx = g.value_and_vjp(x, dy)
        torch.cuda.synchronize()
        assert KERNEL in model.last_launch_info(), model.last_launch_info()
        ye, dxe = _eager(model, x, dy)
        _close_to_eager(y, dx, ye, dxe, ("GraphedForces", n))
        yr = g(x).clone()
        dxr = g.vjp(dy).clone()
        torch.cuda.synchronize()
        assert torch.equal(yr, ye)
        assert float((dxr - dxe).abs().max()) <= 1e-6 * max(1.0, float(dxe.abs().max()))
