"""Float64 values and the metric tensor M[f, k, l] = sum_a w_a grad_a y_k . grad_a y_l in ONE launch
(molann_value_and_metric_f64 -> frames_value_metric_f64_kernel, MolANN.value_and_metric, PreprocessingANN.value_and_metric):

1. against the float64 oracle: M_want = einsum(J_want, w, J_want) on the CPU from the Jacobian test's oracle.  The project's bar for
   the Jacobian is 1e-9 of the frame's scale s_f and M is bilinear in J, so a Jacobian within that bar moves M[f, k, l] by at most
   2 * 1e-9 s_f * max_k sum_{a,i} |w_a| |J_want[f, k, a, i]| (the second-order term is 1e-9 of that): this is the bound, with s_f
   clamped as the Jacobian test clamps it.  y within 1e-10.  Only frames the suite's conditioning filter accepts are compared, at
   least half of every batch; the seeds are fixed and were chosen on the CPU so that this holds;
2. against the route it replaces: y bit-equal to value_and_jacobian's, M against the einsum of that call's jac in float64.  The two
   differ in summation order only: |dM_kl| <= max(1e-12, 8 n_inp 2^-53) sqrt(A_kk A_ll), A the same einsum with |w_a| (A = M for
   weights that are not negative) - Cauchy-Schwarz on the magnitudes of the terms;
3. plan shapes: the smallest that reach each code path, and a guard that lane groups 8, 16, 32 and 64 all ran;
4. weights; 5. properties (symmetry bit for bit, diagonal >= 0, inputs not written, two calls and a captured launch give the same bits,
   into=, the operator route and the ctypes route agree bit for bit); 6. error paths, none of which launches."""

import copy

import numpy as np
import pytest
import torch

import far_frames as ff
import test_gpu_jvp_plans as jvp
import test_gpu_random_backward as rb
import test_gpu_value_and_jacobian_f64 as vjac
import test_gpu_value_and_vjp_f64 as vj
from molann_amd import _capi, ann, workloads as wl
from molann_amd.ann import MolANN, PreprocessingANN

pytestmark = pytest.mark.gpu
KERNEL = "frames_value_metric_f64_kernel"
ANGLE, BOND, DIH, POS = wl.ANGLE, wl.BOND, wl.DIHEDRAL, wl.POSITION
CHAIN, SIX = vjac.CHAIN, vjac.SIX
REACHED = set()          # lane groups seen by the plan-shape tests
EINSUM = "fkai,a,flai->fkl"
_build, _frames, _oracle = vjac._build, vjac._frames, vjac._oracle


# ---- helpers ---------------------------------------------------------------------------------------------------------------
def _lanes(info):
    assert KERNEL in info, info
    return int(info.split("; ")[1].split(" lanes per frame")[0])


def _call(model, x, weights=None, into=None):
    """(y, M, launch info) of either module's value_and_metric."""
    y, M = model.value_and_metric(x, weights=weights, into=into)
    torch.cuda.synchronize()
    info = model.last_launch_info() if isinstance(model, MolANN) else ann.last_launch_info(model)
    return y, M, info


def _w(weights, x):
    return weights if weights is not None else torch.ones(x.shape[1], dtype=torch.float64, device=x.device)


def _against_oracle(case, model, x, weights, y, M, what):
    """Item 1 of the module docstring."""
    y_want, j_want = _oracle(case, model, x)
    ok = jvp._well(case, x, jvp._ref(model))
    n = x.shape[0]
    assert int(ok.sum()) * 2 >= n, (what, "too few well-conditioned frames", int(ok.sum()), n)
    w = _w(weights, x).cpu()
    m_want = torch.einsum(EINSUM, j_want, w, j_want)
    yc, mc = y.detach().cpu(), M.detach().cpu()
    assert mc.shape == m_want.shape and yc.shape == y_want.shape, (what, mc.shape, m_want.shape)
    assert bool(torch.isfinite(mc[ok]).all()), (what, "non-finite")
    ey, sy = float((yc[ok] - y_want[ok]).abs().max()), max(1.0, float(y_want[ok].abs().max()))
    s = j_want[ok].reshape(int(ok.sum()), -1).abs().amax(dim=1)
    s = s.clamp(min=max(1e-300, 1e-3 * float(s.max())))
    row = (j_want[ok].abs() * w.abs()[None, None, :, None]).sum(dim=(2, 3)).amax(dim=1)      # max_k sum_{a,i} |w_a| |J[f,k,a,i]|
    err = (mc[ok] - m_want[ok]).abs().reshape(int(ok.sum()), -1).amax(dim=1)
    bound = 2e-9 * s * row
    worst = float((err / bound.clamp(min=1e-300)).max())
    print("%s: %d of %d frames, y err %.3e (scale %.3g), M err %.3e of its bound" % (what, int(ok.sum()), n, ey, sy, worst))
    assert ey <= 1e-10 * sy, (what, "y", ey, sy)
    assert bool((err <= bound).all()), (what, "M", worst, int((err / bound.clamp(min=1e-300)).argmax()))
    return m_want, ok


def _against_route(model, x, weights, y, M, what):
    """Item 2 of the module docstring; returns (jac, its einsum)."""
    yj, jac, _ = vjac._call(model, x)
    assert torch.equal(y, yj), (what, "y differs from value_and_jacobian's")
    w = _w(weights, x)
    m_route = torch.einsum(EINSUM, jac, w, jac)
    a = torch.einsum(EINSUM, jac, w.abs(), jac)
    d = torch.diagonal(a, dim1=1, dim2=2)
    assert bool((d >= 0).all())
    bound = max(1e-12, 8 * x.shape[1] * 2.0 ** -53) * torch.sqrt(d[:, :, None] * d[:, None, :])
    fin = torch.isfinite(m_route).reshape(x.shape[0], -1).all(1) & torch.isfinite(a).reshape(x.shape[0], -1).all(1)
    assert bool(fin.any())
    err = (M - m_route).abs()
    ratio = float((err[fin] / bound[fin].clamp(min=1e-300)).max())
    print("%s: against value_and_jacobian + einsum, worst %.3e of the bound" % (what, ratio))
    assert bool((err[fin] <= bound[fin]).all()), (what, ratio)
    return jac, m_route


def _check(case, model, x, what, weights=None, route=True):
    x0 = x.clone()
    y, M, info = _call(model, x, weights)
    assert KERNEL in info and info.count("_kernel") == 1, info
    assert torch.equal(x, x0), (what, "x written")
    d_out = case.mlp[-1] if case.mlp else case.d_feat()
    assert tuple(y.shape) == (x.shape[0], d_out) and tuple(M.shape) == (x.shape[0], d_out, d_out)
    assert torch.equal(M, M.transpose(1, 2)), (what, "M is not symmetric bit for bit")
    _against_oracle(case, model, x, weights, y, M, what)
    if route:
        _against_route(model, x, weights, y, M, what)
    if weights is None or bool((weights > 0).all()):
        ok = jvp._well(case, x, jvp._ref(model)).to(x.device)
        assert bool((torch.diagonal(M, dim1=1, dim2=2)[ok] >= 0).all()), (what, "negative diagonal")
    return y, M, info


def _workload_case(name, dev, align=True):
    """(workload, its shared float64 model, the oracle's case); align=False: the same plan without its alignment layer."""
    w, model, (feats, uav, al) = vj._shared(name, dev)
    if not align:
        case = rb.Case(name + "_noalign", w.ref_xyz, feats, None, uav, list(w.mlp_dims), "tanh")
        return w, _build(case, dev), case
    return w, model, rb.Case(name, w.ref_xyz, feats, al, uav, list(w.mlp_dims), "tanh")


def _plan(name):
    """(case, lanes per frame) of the small plans."""
    if name == "C3p_head":                                 # position items behind an alignment: every output's rot[k]
        return rb.Case(name, wl.ALA_DIPEPTIDE_XYZ, [(POS, list(range(22)))], [a - 1 for a in wl.ALA_BACKBONE], mlp=[66, 5, 3]), 64
    if name == "dout1":
        return rb.Case(name, CHAIN[:8], SIX, [0, 1, 3, 6], mlp=[6, 5, 1]), 8
    if name == "dout8":
        return rb.Case(name, CHAIN[:8], SIX, None, mlp=[6, 32, 8], act="silu"), 32
    if name == "dout9":                                    # one output past a chunk: a strip of one column
        return rb.Case(name, CHAIN[:8], SIX, [0, 1, 3, 6], mlp=[6, 5, 9]), 16
    if name == "dout16":                                   # the end of the required range: two chunks, four strips
        return rb.Case(name, CHAIN[:8], SIX, None, uav=True, mlp=[4, 7, 16], act="sigmoid"), 16
    if name == "dout20":                                   # three chunks, the last of them partial, strips behind two of them
        return rb.Case(name, CHAIN[:8], SIX, [0, 1, 3, 6], mlp=[6, 7, 20]), 32
    if name == "pos_align":
        return rb.Case(name, CHAIN[:9], [(POS, [0, 3, 8]), (BOND, [1, 2])], [0, 2, 5, 7, 8], shift=(1.0, -2.0, 0.5), mlp=[10, 4, 2]), 16
    raise KeyError(name)


def _weights(kind, n_inp, dev, seed=3):
    g = torch.Generator().manual_seed(seed)
    if kind == "positive":
        w = 0.05 + 1.95 * torch.rand(n_inp, generator=g, dtype=torch.float64)
    elif kind == "mixed":
        w = torch.randn(n_inp, generator=g, dtype=torch.float64)
        assert bool((w < 0).any()) and bool((w > 0).any())
    else:
        raise KeyError(kind)
    return w.to(dev)


# ---- 3. plan shapes (with items 1 and 2 on each) ----------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 65])
def test_c3(n, hip_device):
    """The 22-atom flagship, head [6, 32, 8], two frames per wave and eight per block: one frame, and a last block that is one
    frame short of full or holds a single frame."""
    w, model, case = _workload_case("C3", hip_device)
    assert list(w.mlp_dims) == [6, 32, 8]
    x = w.make_frames(n, seed=7 + n).double().to(hip_device)
    _, _, info = _check(case, model, x, "C3 n=%d" % n)
    assert _lanes(info) == 32, info
    REACHED.add(32)


def test_c3_without_alignment(hip_device):
    w, model, case = _workload_case("C3", hip_device, align=False)
    x = w.make_frames(24, seed=5).double().to(hip_device)
    _check(case, model, x, "C3 without alignment")


@pytest.mark.parametrize("name,n", [("P1", 24), ("C4", 6)])
def test_workloads(name, n, hip_device):
    """The 166-atom P1 and a 5000-atom frame with the head [85, 128, 64, 8]: one wave per frame."""
    w, model, case = _workload_case(name, hip_device)
    assert w.n_atoms == {"P1": 166, "C4": 5000}[name]
    x = w.make_frames(n, seed=7).double().to(hip_device)
    _, _, info = _check(case, model, x, name)
    assert _lanes(info) == 64, info
    REACHED.add(64)


@pytest.mark.parametrize("name", ["C3p_head", "dout1", "dout8", "dout9", "dout16", "dout20"])
def test_small_plans(name, hip_device):
    """Position items behind an alignment, and heads ending in 1, 8, 9, 16 and 20 outputs: both sides of the JAC64_KC chunk, the end
    of the required range and past it."""
    case, G = _plan(name)
    model = _build(case, hip_device)
    x = _frames(case, 24, len(name), hip_device)
    _, _, info = _check(case, model, x, name)
    assert _lanes(info) == G, info
    REACHED.add(G)


def test_features_metric_of_c3(hip_device):
    """PreprocessingANN.value_and_metric on C3's features: d_out = d_feat = 6, no parameter in G; and the identity
    sum_a w_a |grad_a y_k|^2 = dF_k G dF_k^T against the model's own metric (dF by autograd of the head on the CPU)."""
    w, model, (feats, uav, al) = vj._shared("C3", hip_device)
    pp = model.preprocessing_layer
    assert isinstance(pp, PreprocessingANN)
    case = rb.Case("C3_features", w.ref_xyz, feats, al, uav, None)
    x = w.make_frames(24, seed=9).double().to(hip_device)
    wt = _weights("positive", w.n_atoms, hip_device)
    f, G, info = _check(case, pp, x, "C3 features", weights=wt)
    assert tuple(G.shape) == (24, 6, 6) and _lanes(info) == 32, info
    _, M, _ = _call(model, x, wt)
    head = rb._head64(model)
    dF = torch.autograd.functional.jacobian(lambda v: head(v).sum(0), f.cpu()).permute(1, 0, 2)       # [N, d_out, d_feat]
    want = torch.einsum("fki,fij,flj->fkl", dF, G.cpu(), dF)
    scale = torch.diagonal(want, dim1=1, dim2=2).abs().amax(dim=1).clamp(min=1e-300)
    assert float(((M.cpu() - want).abs().reshape(24, -1).amax(dim=1) / scale).max()) <= 1e-9


def test_one_frame_past_a_full_grid(hip_device):
    """num_cus x 8 blocks of 8 frames (32 lanes per frame), and one more: the grid strides."""
    w, model, case = _workload_case("C3", hip_device)
    cus = torch.cuda.get_device_properties(hip_device).multi_processor_count
    n = cus * 8 * 8 + 1
    base = w.make_frames(512, seed=40).double().to(hip_device)
    x = base.repeat((n + 511) // 512, 1, 1)[:n].contiguous()
    x[-1] = w.make_frames(1, seed=41).double().to(hip_device)[0]
    y, M, info = _call(model, x)
    assert _lanes(info) == 32 and "grid=%d " % (cus * 8) in info, info
    assert torch.equal(M, M.transpose(1, 2))
    _against_route(model, x, None, y, M, "C3 past one grid")
    rows = torch.tensor(sorted(set(range(4)) | set(range(n - 4, n)) |
                               set(np.random.default_rng(32).choice(n, size=24, replace=False).tolist())), device=hip_device)
    _against_oracle(case, model, x[rows], None, y[rows], M[rows], "C3 past one grid")
    yt, mt, _ = _call(model, x[-700:].contiguous())
    assert torch.equal(y[-700:], yt) and torch.equal(M[-700:], mt), "tail of a batch past one grid"
    assert torch.equal(M[:512], M[512:1024]) and torch.equal(y[:512], y[512:1024])


def test_every_lane_group_ran(request):
    ran = {i.name.split("[")[0] for i in request.session.items}
    if not {"test_c3", "test_workloads", "test_small_plans"} <= ran:
        pytest.skip("the plan-shape tests were deselected")
    assert REACHED == {8, 16, 32, 64}, REACHED


def test_plans_the_geometry_refuses(hip_device):
    """An output past the cap of 64, and a plan whose rows the Jacobian geometry refuses: supports says no, the call returns
    MOLANN_E_UNSUPPORTED and the method names the route that remains."""
    with torch.cuda.device(hip_device):
        assert _capi.Plan(8, features=[(BOND, [0, 1])], layer_dims=[1, 4, 64], activation=0).supports_value_and_metric_f64()
        assert _capi.Plan(8, features=[(BOND, [0, 1])], layer_dims=[1, 16, 4], activation=0).supports_value_and_metric_f64()
        none = _capi.Plan(8, align_idx=[0, 1, 2, 3], ref_x=torch.zeros(4, 3))       # no items: nothing to differentiate
        assert not none.supports_value_and_metric_f64()
        for dims in ([1, 4, 65], [1, 512, 64]):
            p = _capi.Plan(8, features=[(BOND, [0, 1])], layer_dims=dims, activation=0)
            assert p.supports_value_and_jacobian_f64() == (dims[1] == 4) and not p.supports_value_and_metric_f64()
            x = torch.zeros((1, 8, 3), dtype=torch.float64, device=hip_device)
            Ws = [torch.zeros((dims[1], 1), dtype=torch.float64, device=hip_device),
                  torch.zeros((dims[2], dims[1]), dtype=torch.float64, device=hip_device)]
            bs = [torch.zeros(dims[1], dtype=torch.float64, device=hip_device), torch.zeros(dims[2], dtype=torch.float64, device=hip_device)]
            y = torch.full((1, dims[2]), float("nan"), dtype=torch.float64, device=hip_device)
            M = torch.full((1, dims[2], dims[2]), float("nan"), dtype=torch.float64, device=hip_device)
            with pytest.raises(_capi.MolannHipError) as e:
                p.value_and_metric_f64(x, Ws, bs, None, y, M)
            assert e.value.code == _capi.E_UNSUPPORTED
            torch.cuda.synchronize()
            assert bool(torch.isnan(M).all()) and bool(torch.isnan(y).all())
    for mlp in ([1, 4, 65], [1, 512, 64]):
        case = rb.Case("refused", CHAIN[:8], [(BOND, [0, 1])], None, mlp=mlp)
        model = _build(case, hip_device)
        with pytest.raises(NotImplementedError, match="einsum"):
            model.value_and_metric(_frames(case, 2, 1, hip_device))


# ---- far frames and degenerate sets ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["pos_align", "C3p_head"])
def test_far_frames_share_waves_with_near_frames(name, hip_device):
    """Frames translated by 100 and 1000 A (far_frames' "offset") in one wave with near ones: a near frame's metric does not change
    with its wave-mates, bit for bit; the whole batch against the oracle and the Jacobian route."""
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
    yn, mn, _ = _call(model, xn)
    yn, mn = yn.clone(), mn.clone()
    ym, mm, _ = _check(case, model, xm, name + " mixed")
    rows = torch.tensor([i for i in range(n) if lab[i] == "near"], device=hip_device)
    assert torch.equal(ym[rows], yn[rows]) and torch.equal(mm[rows], mn[rows]), (name, "a near frame changed with its wave-mates")


def test_a_degenerate_alignment_set_gives_finite_output(hip_device):
    case, _ = _plan("pos_align")
    model = _build(case, hip_device)
    n = 24
    near = ff.draw("near", case.xyz, case.align, n, seed=5)
    lab = ["degenerate" if i % 3 == 1 else "near" for i in range(n)]
    x = torch.from_numpy(ff.compose(lab, case.xyz, case.align, seed=31, base=near)).to(hip_device, torch.float64)
    y, M, _ = _call(model, x)
    assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(M).all())
    assert torch.equal(M, M.transpose(1, 2))
    yn, mn, _ = _call(model, torch.from_numpy(near).to(hip_device, torch.float64))
    rows = torch.tensor([i for i in range(n) if lab[i] == "near"], device=hip_device)
    assert torch.equal(y[rows], yn[rows]) and torch.equal(M[rows], mn[rows])


# ---- 4. weights ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["C3", "dout16"])
def test_none_is_bit_equal_to_ones(name, hip_device):
    if name == "C3":
        w, model, case = _workload_case("C3", hip_device)
        x = w.make_frames(33, seed=3).double().to(hip_device)
    else:
        case, _ = _plan(name)
        model = _build(case, hip_device)
        x = _frames(case, 33, 3, hip_device)
    y0, m0, _ = _call(model, x)
    y0, m0 = y0.clone(), m0.clone()
    y1, m1, _ = _call(model, x, torch.ones(x.shape[1], dtype=torch.float64, device=hip_device))
    assert torch.equal(y0, y1) and torch.equal(m0, m1)


@pytest.mark.parametrize("kind", ["positive", "mixed"])
@pytest.mark.parametrize("name", ["C3", "C3p_head", "dout9"])
def test_random_weights(name, kind, hip_device):
    """Weights in [0.05, 2], and weights of both signs - a bilinear form in the weights: no square root, no clamp - against the
    oracle and the Jacobian route."""
    if name == "C3":
        w, model, case = _workload_case("C3", hip_device)
        x = w.make_frames(24, seed=13).double().to(hip_device)
    else:
        case, _ = _plan(name)
        model = _build(case, hip_device)
        x = _frames(case, 24, 13, hip_device)
    wt = _weights(kind, x.shape[1], hip_device)
    w0 = wt.clone()
    y, M, _ = _check(case, model, x, "%s %s weights" % (name, kind), weights=wt)
    assert torch.equal(wt, w0), "weights written"
    if kind == "mixed":                                    # linear in w: M(w) = M(w+) - M(w-)
        _, mp, _ = _call(model, x, wt.clamp(min=0))
        mp = mp.clone()
        _, mn, _ = _call(model, x, (-wt).clamp(min=0))
        _, ma, _ = _call(model, x, wt.abs())
        scale = torch.diagonal(ma, dim1=1, dim2=2).abs().amax(dim=1).clamp(min=1e-300)
        assert float(((M - (mp - mn)).abs().reshape(24, -1).amax(dim=1) / scale).max()) <= 1e-12


@pytest.mark.parametrize("name,atom", [("C3", 8), ("C3p_head", 4), ("C3p_head", 13)])
def test_single_atom_weights(name, atom, hip_device):
    """Zero on every atom but one touched atom (an item atom that is also an alignment atom; one that is not): the oracle's
    single-atom term J[:, :, a] J[:, :, a]^T, by the bound of item 1."""
    if name == "C3":
        w, model, case = _workload_case("C3", hip_device)
        x = w.make_frames(24, seed=17).double().to(hip_device)
    else:
        case, _ = _plan(name)
        model = _build(case, hip_device)
        x = _frames(case, 24, 17, hip_device)
    assert atom in case.touched()
    wt = torch.zeros(x.shape[1], dtype=torch.float64, device=hip_device)
    wt[atom] = 1.5
    y, M, _ = _call(model, x, wt)
    m_want, ok = _against_oracle(case, model, x, wt, y, M, "%s atom %d" % (name, atom))
    _, j_want = _oracle(case, model, x)
    single = 1.5 * torch.einsum("fki,fli->fkl", j_want[:, :, atom], j_want[:, :, atom])
    assert float((m_want - single).abs().max()) <= 1e-14 * max(1.0, float(single.abs().max()))
    assert float(M[ok.to(hip_device)].abs().max()) > 0.0


# ---- 5. properties ---------------------------------------------------------------------------------------------------------------
def test_inputs_are_not_written_and_two_calls_give_the_same_bits(hip_device):
    w, model, case = _workload_case("C3", hip_device)
    x = w.make_frames(4097, seed=41).double().to(hip_device)
    wt = _weights("positive", w.n_atoms, hip_device)
    x0, w0 = x.clone(), wt.clone()
    params = [p.detach().clone() for p in model.parameters()]
    ref0 = rb._align_layer(model).ref_x.detach().clone()
    y1, m1, info = _call(model, x, wt)
    y1, m1 = y1.clone(), m1.clone()
    y2, m2, _ = _call(model, x, wt)
    assert KERNEL in info and info.count("_kernel") == 1, info
    assert torch.equal(y1, y2) and torch.equal(m1, m2)
    assert bool(torch.isfinite(m1).all()) and torch.equal(m1, m1.transpose(1, 2))
    assert bool((torch.diagonal(m1, dim1=1, dim2=2) >= 0).all())
    assert torch.equal(x, x0) and torch.equal(wt, w0) and torch.equal(rb._align_layer(model).ref_x, ref0)
    assert all(torch.equal(p, q) for p, q in zip(model.parameters(), params))


@pytest.mark.parametrize("which", ["model", "features"])
def test_into_buffers_are_filled_in_place(which, hip_device):
    w, model, case = _workload_case("C3", hip_device)
    mod = model if which == "model" else model.preprocessing_layer
    x = w.make_frames(5, seed=51).double().to(hip_device)
    y, M, _ = _call(mod, x)
    y2, m2 = torch.full_like(y, float("nan")), torch.full_like(M, float("nan"))
    p = (y2.data_ptr(), m2.data_ptr())
    r = mod.value_and_metric(x, into=(y2, m2))
    torch.cuda.synchronize()
    assert r[0] is y2 and r[1] is m2 and (y2.data_ptr(), m2.data_ptr()) == p
    assert not bool(torch.isnan(y2).any()) and not bool(torch.isnan(m2).any())
    assert torch.equal(y2, y) and torch.equal(m2, M)
    flat = torch.full((M.numel(),), float("nan"), dtype=torch.float64, device=hip_device)      # numel is what counts
    mod.value_and_metric(x, into=(y2, flat))
    torch.cuda.synchronize()
    assert torch.equal(flat.view_as(M), M)


def test_a_captured_launch_replays_the_same_bits(hip_device):
    w, model, case = _workload_case("C3", hip_device)
    xs = w.make_frames(64, seed=61).double().to(hip_device)
    wt = _weights("positive", w.n_atoms, hip_device)
    y, M, _ = _call(model, xs, wt)
    y, M = y.clone(), M.clone()
    x = torch.zeros_like(xs)
    yb, mb = torch.empty_like(y), torch.empty_like(M)
    g = torch.cuda.CUDAGraph()
    s = torch.cuda.Stream(device=hip_device)
    s.wait_stream(torch.cuda.current_stream(hip_device))
    with torch.cuda.stream(s):
        model.value_and_metric(x, weights=wt, into=(yb, mb))   # warm: plan and reference are in place before the capture
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=s):
            model.value_and_metric(x, weights=wt, into=(yb, mb))
    torch.cuda.current_stream(hip_device).wait_stream(s)
    for _ in range(2):
        x.copy_(xs)
        yb.fill_(float("nan"))
        mb.fill_(float("nan"))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(yb, y) and torch.equal(mb, M)


@pytest.mark.parametrize("name", ["C3", "dout20"])
def test_operator_route_and_ctypes_route_give_the_same_bits(name, hip_device, monkeypatch):
    if name == "C3":
        w, model, case = _workload_case("C3", hip_device)
        x = w.make_frames(37, seed=71).double().to(hip_device)
    else:
        case, _ = _plan(name)
        model = _build(case, hip_device)
        x = _frames(case, 37, 71, hip_device)
    if ann._run_op() is None:
        pytest.fail("the operator library is not loaded: build() makes it")
    wt = _weights("positive", x.shape[1], hip_device)
    assert model._fast_state(x)["op"] is not None
    got = [_call(model, x, wgt) for wgt in (None, wt)]
    got = [(y.clone(), M.clone(), info) for y, M, info in got]
    monkeypatch.setattr(ann, "_run_op", lambda: None)
    plain = copy.deepcopy(model)                           # a copy drops the cached state: this one never sees the operators
    assert plain._fast_state(x)["op"] is None
    for (y, M, info), wgt in zip(got, (None, wt)):
        y2, m2, info2 = _call(plain, x, wgt)
        assert torch.equal(y, y2) and torch.equal(M, m2)
        assert _lanes(info) == _lanes(info2)
    into = (torch.full_like(got[0][0], float("nan")), torch.full_like(got[0][1], float("nan")))
    plain.value_and_metric(x, into=into)
    torch.cuda.synchronize()
    assert torch.equal(into[0], got[0][0]) and torch.equal(into[1], got[0][1])


# ---- 6. error paths (no kernel launch) -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", ["operator", "ctypes"])
def test_error_paths(route, hip_device, monkeypatch):
    w, model, case = _workload_case("C3", hip_device)
    if route == "ctypes":
        monkeypatch.setattr(ann, "_run_op", lambda: None)
        model = copy.deepcopy(model)
    x = w.make_frames(5, seed=71).double().to(hip_device)
    d_out = w.out_dim()
    assert (model._fast_state(x)["op"] is None) == (route == "ctypes")
    y = torch.full((5, d_out), float("nan"), dtype=torch.float64, device=hip_device)
    M = torch.full((5, d_out, d_out), float("nan"), dtype=torch.float64, device=hip_device)
    wt = torch.ones(w.n_atoms, dtype=torch.float64, device=hip_device)
    with pytest.raises(TypeError, match=r"model\.double\(\)"):
        model.value_and_metric(x.float())
    for bad in ((y.float(), M), (y, M.float()), (y,)):
        with pytest.raises(TypeError):
            model.value_and_metric(x, into=bad)
    for bad in ((y[:4], M), (y, M[:, :-1]), (y, M.transpose(1, 2)[:, :, :4]), (y, M.cpu()), (y.cpu(), M)):
        with pytest.raises(ValueError):
            model.value_and_metric(x, into=bad)
    for bad in (wt.float(), wt.to(torch.int64), [1.0] * w.n_atoms):
        with pytest.raises(TypeError, match="weights"):
            model.value_and_metric(x, weights=bad, into=(y, M))
    for bad in (wt[:-1], torch.cat([wt, wt]), wt.cpu()):
        with pytest.raises(ValueError, match="weights"):
            model.value_and_metric(x, weights=bad, into=(y, M))
        with pytest.raises(ValueError, match="weights"):
            model.preprocessing_layer.value_and_metric(x, weights=bad)
    m32 = wl.build_model(w, hip_device, 0).requires_grad_(False)
    with pytest.raises(RuntimeError, match="float64"):
        m32.value_and_metric(x, into=(y, M))               # float32 parameters, float64 x
    with pytest.raises(NotImplementedError, match="einsum"):
        model.value_and_metric(x.cpu())
    with pytest.raises(TypeError):
        model.preprocessing_layer.value_and_metric(x.float())
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all()) and bool(torch.isnan(M).all()), "an error path launched"
    y0, m0 = model.value_and_metric(x[:0])
    assert tuple(y0.shape) == (0, d_out) and tuple(m0.shape) == (0, d_out, d_out)
    assert y0.dtype == torch.float64 and m0.dtype == torch.float64 and y0.device == x.device and m0.device == x.device
    f0, g0 = model.preprocessing_layer.value_and_metric(x[:0])
    assert tuple(f0.shape) == (0, 6) and tuple(g0.shape) == (0, 6, 6) and g0.dtype == torch.float64 and g0.device == x.device
    if route == "operator":
        with pytest.raises(TypeError):
            torch.ops.molann.value_and_metric_h(x.float(), model._fast["handle"], rb._align_layer(model).ref_x,
                                                [lin.weight for lin in model._fast["linears"]],
                                                [lin.bias for lin in model._fast["linears"]], None, [])
