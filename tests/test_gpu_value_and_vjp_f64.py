"""Float64 values and forces in ONE launch (molann_value_and_vjp_f64 -> frames_value_vjp_f64_kernel): against the reference's float64
fixtures, float64 autograd through the oracle (every activation, batch edges, frame sizes from 3 to 5000 atoms, plans with and
without an alignment), far frames, the eager float64 model, run-to-run bits, into=, the Jacobian of a frame, a NaN frame, the
scripted operator, GraphedForces and the launch info.  Bounds: the float64 suite's own (tests/test_gpu_f64.py)."""

import copy
import os

import numpy as np
import pytest
import torch

import test_gpu_random_backward as rb
from golden_util import GOLDEN_DIR
from molann_amd import _capi, workloads as wl
from molann_amd.ann import MolANN, PreprocessingANN, create_sequential_nn
from oracle import molann_oracle as mo

pytestmark = pytest.mark.gpu
KERNEL = "frames_value_vjp_f64_kernel"


def _close(y, dx, y_want, gx_want, what):
    """y within 1e-10 max(1, |y|max), dx within 1e-9 max(1e-3, |dx|max) of the float64 reference."""
    y_want, gx_want = torch.as_tensor(y_want), torch.as_tensor(gx_want)
    assert y.dtype == torch.float64 and dx.dtype == torch.float64
    ey = float((y.detach().cpu() - y_want).abs().max())
    ed = float((dx.detach().cpu() - gx_want).abs().max())
    sy, sd = max(1.0, float(y_want.abs().max())), max(1e-3, float(gx_want.abs().max()))
    print("%s: y err %.3e (scale %.3g), dx err %.3e (scale %.3g)" % (what, ey, sy, ed, sd))
    assert ey <= 1e-10 * sy, (what, "y", ey, sy)
    assert ed <= 1e-9 * sd, (what, "dx", ed, sd)


def _feature_plan(model, x):
    """The ctypes plan of a features-only module (made, and its float64 ref_x packed, by a forward under grad mode)."""
    model(x[:1].clone().requires_grad_(True))
    return model._plans()[("features", x.device.index)].plan


def _call(model, x, G):
    """(y, dx, launch info): MolANN.value_and_vjp, or the plan-level call on a features-only module."""
    if isinstance(model, MolANN):
        y, dx = model.value_and_vjp(x, G)
        torch.cuda.synchronize()
        return y, dx, model.last_launch_info()
    plan = _feature_plan(model, x)
    assert plan.supports_value_and_vjp_f64()
    y = torch.full((x.shape[0], plan.feature_dim), float("nan"), dtype=torch.float64, device=x.device)
    dx = torch.full_like(x, float("nan"))
    with torch.cuda.device(x.device):
        plan.value_and_vjp_f64(x, G.contiguous(), [], [], y, dx)
    torch.cuda.synchronize()
    return y, dx, plan.last_launch_info()


def _oracle(model, feats, uav, align, x, G):
    """y and J^T G by float64 autograd on the CPU: the oracle's preprocessing on the model's own ref_x, then a copy of its head."""
    al = rb._align_layer(model)
    ref = al.ref_x.detach().cpu().double() if al is not None else None
    xx = x.detach().cpu().double().requires_grad_(True)
    y = mo.preprocessing_forward(xx, feats, uav, align if al is not None else None, ref)
    if isinstance(model, MolANN):
        y = copy.deepcopy(model.ann_layers).cpu().double()(y)
    (gx,) = torch.autograd.grad(y, xx, G.detach().cpu().double())
    return y.detach(), gx


def _workload(name, dev, head=None, act=None):
    """(workload, its float64 model with frozen parameters, oracle arguments)"""
    w = wl.get_workload(name)
    model = wl.build_model(w, dev, 0)
    if head is not None:
        torch.manual_seed(11)
        model = MolANN(model.preprocessing_layer, create_sequential_nn([w.feature_dim()] + head, activation=act)).to(dev)
    model = model.double().requires_grad_(False)
    feats = [(t, [a - 1 for a in atoms]) for t, atoms in w.features]
    al = [a - 1 for a in w.align] if w.align is not None else None
    return w, model, (feats, w.use_angle_value, al)


def _batch(w, model, n, seed, dev):
    x = w.make_frames(n, seed=seed).double().to(dev)
    d_out = model.ann_layers[-1].out_features if isinstance(model, MolANN) else w.feature_dim()
    G = torch.randn((n, d_out), generator=torch.Generator().manual_seed(seed + 1), dtype=torch.float64).to(dev)
    return x, G


_SHARED = {}


def _shared(name, dev):
    """One model per workload for the tests that only read it."""
    if name not in _SHARED:
        _SHARED[name] = _workload(name, dev)
    return _SHARED[name]


# ---- 1. the reference's fixtures ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["grad_molann_C1", "grad_molann_C3", "grad_molann_P1", "grad_molann_P2", "grad_molann_L1_raw",
                                  "grad_features_C2", "grad_features_C3_val", "grad_features_C3p", "grad_features_P2"])
def test_reference_fixtures(name, hip_device):
    from test_gpu_backward import _model_from_golden
    d = np.load(os.path.join(GOLDEN_DIR, name + ".npz"))
    for key in ("x", "G", "out_f64", "gx_f64"):
        assert key in d, (name, key)
    model = _model_from_golden(d, hip_device).double().requires_grad_(False)
    assert isinstance(model, MolANN) == name.startswith("grad_molann"), type(model)
    x = torch.from_numpy(d["x"]).double().to(hip_device)
    G = torch.from_numpy(d["G"]).double().to(hip_device)
    y, dx, info = _call(model, x, G)
    assert KERNEL in info, info
    _close(y, dx, d["out_f64"], d["gx_f64"], name)


# ---- 2. every activation -------------------------------------------------------------------------------------------------------
ACT_MODULES = [torch.nn.Tanh, torch.nn.ReLU, torch.nn.Sigmoid, torch.nn.Identity, torch.nn.ELU, torch.nn.SiLU, torch.nn.Softplus,
               torch.nn.LeakyReLU, torch.nn.GELU]


@pytest.mark.parametrize("act", ACT_MODULES, ids=[a.__name__ for a in ACT_MODULES])
def test_every_activation(act, hip_device):
    w, model, args = _workload("C3", hip_device, head=[7, 5, 3], act=act())
    x, G = _batch(w, model, 65, 5, hip_device)
    y, dx, info = _call(model, x, G)
    assert KERNEL in info, info
    _close(y, dx, *_oracle(model, *args, x, G), what=act.__name__)


# ---- 3. batch edges and frame sizes --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 257])
def test_batch_edges(n, hip_device):
    w, model, args = _shared("C3", hip_device)
    x, G = _batch(w, model, n, 100 + n, hip_device)
    x0 = x.clone()
    y, dx, info = _call(model, x, G)
    assert KERNEL in info, info
    _close(y, dx, *_oracle(model, *args, x, G), what="C3 n=%d" % n)
    assert torch.equal(x, x0)


@pytest.mark.parametrize("name,n", [("P1", 9), ("P2", 9), ("C4", 3), ("C5", 2)])
def test_frame_sizes(name, n, hip_device):
    """166-atom plans, and 5000-atom plans with the heads [85, 128, 64, 8] and [341, 512, 256, 16]."""
    w, model, args = _shared(name, hip_device)
    if name == "C4":
        assert w.n_atoms == 5000 and w.mlp_dims == [85, 128, 64, 8]
    if name == "C5":
        assert w.n_atoms == 5000 and w.mlp_dims == [341, 512, 256, 16]
    x, G = _batch(w, model, n, 7, hip_device)
    y, dx, info = _call(model, x, G)
    assert KERNEL in info, info
    y_want, gx_want = _oracle(model, *args, x, G)
    _close(y, dx, y_want, gx_want, what=name)
    untouched = sorted(set(range(w.n_atoms)) - {a - 1 for a in w.touched_atoms()})
    if untouched:
        assert float(dx[:, untouched].abs().max()) == 0.0


def _small_case(n_inp, align, head=True, act="tanh"):
    """Two dihedrals sharing atoms 2 and 3, an angle and a bond on their atoms, positions of atoms 4 and 6 - 4 and 6 are alignment
    atoms too; the atoms from 7 on are untouched."""
    feats = [(rb.DIH, [0, 1, 2, 3]), (rb.DIH, [2, 3, 4, 5]), (rb.ANGLE, [3, 4, 5]), (rb.BOND, [0, 5]), (rb.POS, [4, 6])]
    c = rb.Case("small%d" % n_inp, rb._chain(n_inp, 3), feats, align=align, mlp=[5, 2] if head else None, act=act)
    if head:
        c.mlp = [c.d_feat()] + c.mlp
    return c


@pytest.mark.parametrize("n_inp,lanes", [(7, 8), (12, 16), (30, 32), (40, 64)])
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "no_alignment"])
@pytest.mark.parametrize("head", [True, False], ids=["head", "features"])
def test_lane_groups_shared_atoms_untouched_atoms(n_inp, lanes, aligned, head, hip_device):
    """Every lane-group width; an alignment atom that is an item atom; atoms named by several items; a plan without alignment;
    untouched atoms' rows exactly 0."""
    case = _small_case(n_inp, [0, 2, 4, 6] if aligned else None, head=head)
    model = case.build(hip_device).double().requires_grad_(False)
    for n in (1, 65):
        x = case.frames(n, seed=n_inp + n, dev=hip_device).double()
        d_out = case.mlp[-1] if head else case.d_feat()
        G = torch.randn((n, d_out), generator=torch.Generator().manual_seed(n), dtype=torch.float64).to(hip_device)
        y, dx, info = _call(model, x, G)
        if head:       # the head's widest layer input (the 12 feature columns) asks for at least 16 lanes
            lanes = max(lanes, 16)
        assert KERNEL in info and "%d lanes per frame" % lanes in info, info
        _close(y, dx, *_oracle(model, case.feats, case.uav, case.align, x, G), what=(case.name, n))
        untouched = sorted(set(range(n_inp)) - case.touched())
        assert len(untouched) == n_inp - 7
        if untouched:
            assert float(dx[:, untouched].abs().max()) == 0.0


def test_three_atom_frame_aligned_on_its_three_atoms(hip_device):
    """A rank-2 covariance."""
    xyz = np.array([[0.0, 0.0, 0.0], [1.4, 0.2, 0.0], [2.0, 1.3, 0.4]], dtype=np.float32)
    feats = [(rb.ANGLE, [0, 1, 2]), (rb.BOND, [0, 2]), (rb.POS, [0, 1, 2])]
    case = rb.Case("tri", xyz, feats, align=[0, 1, 2], mlp=[4, 2], act="tanh")
    case.mlp = [case.d_feat()] + case.mlp
    model = case.build(hip_device).double().requires_grad_(False)
    x = case.frames(33, seed=3, dev=hip_device).double()
    G = torch.randn((33, 2), generator=torch.Generator().manual_seed(3), dtype=torch.float64).to(hip_device)
    y, dx, info = _call(model, x, G)
    assert KERNEL in info, info
    _close(y, dx, *_oracle(model, case.feats, case.uav, case.align, x, G), what="3 atoms")


# ---- 4. far frames -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["C3", "P1"])
def test_far_frames(name, hip_device):
    """Translations of 100 and 1000 A and a random rotation (far_frames' "offset" motions): the plans' items are invariant, so y is
    unchanged and dx is the rotated gradient."""
    from far_frames import _unit, rotations
    w, model, args = _shared(name, hip_device)
    assert all(t != wl.POSITION for t, _ in w.features)
    n = 16
    x, G = _batch(w, model, n, 21, hip_device)
    rng = np.random.default_rng(5)
    Q = torch.from_numpy(rotations(rng, n)).double().to(hip_device)
    mag = np.where(np.arange(n) % 2 == 0, 100.0, 1000.0)
    t = torch.from_numpy(mag[:, None] * _unit(rng, n)).double().to(hip_device)
    xf = (torch.matmul(x, Q) + t[:, None, :]).contiguous()
    y, dx, _ = _call(model, x, G)
    yf, dxf, info = _call(model, xf, G)
    assert KERNEL in info, info
    _close(yf, dxf, y.cpu(), torch.matmul(dx, Q).cpu(), what=name + " moved against near")
    _close(yf, dxf, *_oracle(model, *args, xf, G), what=name + " moved against the oracle")


# ---- 5. the eager float64 model ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [("C3", 65), ("P2", 9)])
def test_consistent_with_eager(name, n, hip_device):
    w, model, _ = _shared(name, hip_device)
    x, G = _batch(w, model, n, 31, hip_device)
    xg = x.clone().requires_grad_(True)
    ye = model(xg)
    (dxe,) = torch.autograd.grad(ye, xg, G)
    y, dx, info = _call(model, x, G)
    assert KERNEL in info, info
    _close(y, dx, ye.detach().cpu(), dxe.cpu(), what=name + " against eager")
    with torch.no_grad():
        _close(y, dx, model(x).cpu(), dxe.cpu(), what=name + " against the no_grad forward")


# ---- 6. the same bits on every run ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", [("C3", 4097), ("P2", 257)])
def test_two_calls_give_the_same_bits(name, n, hip_device):
    w, model, _ = _shared(name, hip_device)
    x, G = _batch(w, model, n, 41, hip_device)
    y1, dx1, _ = _call(model, x, G)
    y1, dx1 = y1.clone(), dx1.clone()
    y2, dx2, info = _call(model, x, G)
    assert KERNEL in info, info
    assert torch.equal(y1, y2) and torch.equal(dx1, dx2)
    assert bool(torch.isfinite(dx1).all())


# ---- 7. into= and dtypes -------------------------------------------------------------------------------------------------------
def test_into_and_dtype_errors(hip_device):
    w, model, _ = _shared("C3", hip_device)
    x, G = _batch(w, model, 5, 51, hip_device)
    y, dx, _ = _call(model, x, G)
    y2, dx2 = torch.full_like(y, float("nan")), torch.full_like(dx, float("nan"))
    r = model.value_and_vjp(x, G, into=(y2, dx2))
    assert r[0] is y2 and r[1] is dx2
    assert torch.equal(y2, y) and torch.equal(dx2, dx)
    r = model.value_and_vjp(x, G.float())                 # a cotangent of another float dtype is converted
    assert r[0].dtype == torch.float64 and float((r[1] - dx).abs().max()) <= 1e-6 * float(dx.abs().max())
    with pytest.raises(TypeError):
        model.value_and_vjp(x, G, into=(y.float(), dx))
    with pytest.raises(TypeError):
        model.value_and_vjp(x, G, into=(y, dx.float()))
    with pytest.raises(ValueError):
        model.value_and_vjp(x, G, into=(y[:4], dx))
    with pytest.raises(ValueError):
        model.value_and_vjp(x, G, into=(y, dx.transpose(1, 2)))
    with pytest.raises(ValueError):
        model.value_and_vjp(x, G[:4])
    with pytest.raises(RuntimeError):
        model.value_and_vjp(x.float(), G.float())         # float64 model, float32 x
    m32 = wl.build_model(w, hip_device, 0).requires_grad_(False)
    with pytest.raises(RuntimeError):
        m32.value_and_vjp(x, G)                           # float32 model, float64 x


# ---- 8. the Jacobian of one frame ----------------------------------------------------------------------------------------------
def test_jacobian_of_one_frame(hip_device):
    w, model, (feats, uav, al) = _shared("P1", hip_device)
    d_out = w.out_dim()
    x1 = w.make_frames(1, seed=9).double().to(hip_device)
    yj, J = model.value_and_vjp(x1.expand(d_out, -1, -1), torch.eye(d_out, dtype=torch.float64, device=hip_device))
    torch.cuda.synchronize()
    assert KERNEL in model.last_launch_info()
    ref = rb._align_layer(model).ref_x.detach().cpu().double()
    head = copy.deepcopy(model.ann_layers).cpu().double()
    Jw = torch.autograd.functional.jacobian(lambda v: head(mo.preprocessing_forward(v, feats, uav, al, ref))[0], x1.cpu())
    _close(yj[:1], J, head(mo.preprocessing_forward(x1.cpu(), feats, uav, al, ref)).detach(), Jw[:, 0], what="Jacobian")
    assert float((yj - yj[:1]).abs().max()) == 0.0


# ---- 9. a NaN frame ------------------------------------------------------------------------------------------------------------
def test_nan_frame_poisons_only_its_rows(hip_device):
    w, model, _ = _shared("P1", hip_device)
    n, bad = 70, 33
    x, G = _batch(w, model, n, 61, hip_device)
    y0, dx0, _ = _call(model, x, G)
    y0, dx0 = y0.clone(), dx0.clone()
    xb = x.clone()
    xb[bad, 5] = float("nan")
    y, dx, _ = _call(model, xb, G)
    keep = torch.ones(n, dtype=torch.bool, device=hip_device)
    keep[bad] = False
    assert torch.equal(y[keep], y0[keep]) and torch.equal(dx[keep], dx0[keep])
    assert torch.isnan(y[bad]).all()


# ---- 10. scripted --------------------------------------------------------------------------------------------------------------
def test_scripted_model_and_operator(tmp_path, hip_device):
    import warnings
    w, model, _ = _shared("C3", hip_device)
    x, G = _batch(w, model, 65, 71, hip_device)
    y, dx, _ = _call(model, x, G)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        torch.jit.script(model).save(str(tmp_path / "c3_f64.pt"))
    loaded = torch.jit.load(str(tmp_path / "c3_f64.pt"), map_location=hip_device)
    with torch.no_grad():
        assert torch.equal(loaded(x), model(x))
    ws = [lin.weight for lin in loaded.linears.children()]
    bs = [lin.bias for lin in loaded.linears.children()]
    handle = torch.ops.molann.register_desc(list(loaded.desc))
    yh, dxh = torch.ops.molann.value_and_vjp_h(x, handle, loaded.ref_x, ws, bs, G, [])
    yd, dxd = torch.ops.molann.value_and_vjp(x, list(loaded.desc), loaded.ref_x, ws, bs, G, [])
    torch.cuda.synchronize()
    assert KERNEL in torch.ops.molann.launch_info(list(loaded.desc), hip_device.index)
    assert torch.equal(yh, y) and torch.equal(dxh, dx)
    assert torch.equal(yd, y) and torch.equal(dxd, dx)


# ---- 11. GraphedForces ---------------------------------------------------------------------------------------------------------
def test_graphed_forces_replays_the_one_launch(hip_device):
    from molann_amd.graph import GraphedForces
    w, model, _ = _shared("C3", hip_device)
    x0, _ = _batch(w, model, 8, 81, hip_device)
    g = GraphedForces(model, x0)
    for seed in (82, 83, 84):
        x, G = _batch(w, model, 8, seed, hip_device)
        yg, dxg = g.value_and_vjp(x, G)
        torch.cuda.synchronize()
        yg, dxg = yg.clone(), dxg.clone()
        y, dx, info = _call(model, x, G)
        assert KERNEL in info, info
        assert torch.equal(yg, y) and torch.equal(dxg, dx)
        with torch.no_grad():
            assert torch.equal(g(x), model(x))
        assert torch.equal(g.vjp(G), dx)


# ---- 12. one launch ------------------------------------------------------------------------------------------------------------
def test_one_launch_and_float32_untouched(hip_device):
    w, model, _ = _shared("C3", hip_device)
    x, G = _batch(w, model, 64, 91, hip_device)
    _, _, info = _call(model, x, G)
    assert info.startswith(KERNEL) and info.count("_kernel") == 1 and "molann_" not in info and "||" not in info, info
    m32 = wl.build_model(w, hip_device, 0).requires_grad_(False)
    m32.value_and_vjp(x.float(), G.float())
    torch.cuda.synchronize()
    info32 = m32.last_launch_info()
    assert KERNEL not in info32 and "molann_bwd_ring" in info32, info32
    with torch.cuda.device(hip_device):
        p = _capi.Plan(22, features=[(wl.BOND, [0, 1])])
        assert p.supports_value_and_vjp_f64()
        y, dx = torch.empty((3, 1), dtype=torch.float64, device=hip_device), torch.empty((3, 22, 3), dtype=torch.float64, device=hip_device)
        p.value_and_vjp_f64(x[:3].contiguous(), torch.ones((3, 1), dtype=torch.float64, device=hip_device), [], [], y, dx)
        torch.cuda.synchronize()
        assert p.last_launch_info().startswith(KERNEL)
        assert float((y[:, 0] - (x[:3, 0] - x[:3, 1]).norm(dim=1)).abs().max()) <= 1e-12
        pa = _capi.Plan(22, align_idx=[0, 1, 2, 3], ref_x=torch.zeros(4, 3))     # no items: nothing to differentiate
        assert not pa.supports_value_and_vjp_f64()
        with pytest.raises(_capi.MolannHipError) as e:
            pa.value_and_vjp_f64(x[:3].contiguous(), torch.ones((3, 1), dtype=torch.float64, device=hip_device), [], [], y, dx)
        assert e.value.code == _capi.E_STAGE
