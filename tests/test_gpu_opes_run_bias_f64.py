"""An OPES run with walls, a table and chosen outputs on the device with no read-back: frames_value_bias_opes_table_f64_kernel
(`value_and_bias(opes=OpesFromTable)`: the OPES term's live count and norm from the table's state in device memory) and
opes_step_columns_f64_kernel (`OpesRun(columns=, walls=, grid=).deposit`: the step on the [W, n_out] outputs and the [W, 4] energies
that launch wrote).

  bias   against `value_and_bias(opes=table.record(scale, S / n, epsilon, columns))` with n and S from `read_state()`: torch.equal on
         y, energies and dx - from the two state loads on it is the same code.
  step   the device against its host twin `molann_selftest_opes_step_columns_f64` on tests/opes_run_cases.py's scenarios (counts and
         slots equal, rows and scalars within that module's 1e-12 bounds), and against the device's `opes_step_f64` on the gathered
         copy: torch.equal on table, state and run.
  loop   C3's own 8-output model, OPES on outputs (5, 2), walls on all 8, 30 steps of 4 walkers: the eager loop against the CPU loop
         of the two host twins within the bounds of tests/test_gpu_opes_run_f64.py's loop test, and one captured graph of the two
         launches, replayed, against the eager loop's bits."""

import copy
import ctypes
import math

import pytest
import torch

import isolation
import opes_deposit_cases as cases
import opes_run_cases as rc
import placement as pl
import test_bias_opes_table_f64_host as hb
import test_gpu_opes_run_f64 as orun
import test_gpu_value_and_hills_f64 as vh
import test_gpu_value_and_vjp_f64 as vv
from molann_amd import _capi, ann, workloads as wl
from molann_amd import bias as mbias
from molann_amd.bias import Grid, OpesFromTable, Restraint

pytestmark = pytest.mark.gpu
F64 = torch.float64
NAN, INF = float("nan"), float("inf")
CPU = torch.device("cpu")
KERNEL = "frames_value_bias_opes_table_f64_kernel"
INFO = KERNEL + " (values + bias + opes from the table's state in one launch; "
CAP, CUTOFF, THRESHOLD = 600, 5.0, 1.0
FLOOR = rc.SCALE * math.log(rc.EPSILON)


# ---------------------------------------------------------------------------------------------- the bias from the table's state
def _outputs(model, x, d_out):
    """The model's outputs of x: a restraint that holds nothing."""
    zero = torch.zeros(d_out, dtype=F64, device=x.device)
    y = model.value_and_bias(x, restraint=Restraint(zero, zero))[0]
    torch.cuda.synchronize()
    return y


def _walls(y_tab):
    """Flat-bottomed walls on all outputs, half a spread wide around the mean: some frames are inside, some outside."""
    mean, spread = y_tab.mean(dim=0), y_tab.std(dim=0) + 0.05
    return Restraint(mean.contiguous(), (3.0 / spread ** 2).contiguous(), flat=(0.5 * spread).contiguous())


def _grid(y_tab, columns, seed):
    """A 2-axis table of noise over the range of the outputs `columns`, the first axis periodic."""
    sub = y_tab[:, list(columns)]
    lo, hi = sub.min(dim=0).values.cpu(), sub.max(dim=0).values.cpu()
    shape = (6, 7)
    table = torch.randn(shape, generator=torch.Generator().manual_seed(seed), dtype=F64).to(y_tab.device)
    spacing = [float((hi[k] - lo[k] + 0.2) / (shape[k] - 1)) for k in range(2)]
    return Grid(table, [float(lo[k]) - 0.1 for k in range(2)], spacing, [True, False], columns=columns)


def _same_as_the_record(model, x, table, cols, walls, grid, what):
    n, total, _, _ = table.read_state()
    got = model.value_and_bias(x, restraint=walls, grid=grid, opes=OpesFromTable(table, rc.SCALE, rc.EPSILON, cols))
    torch.cuda.synchronize()
    info = vh._info(model)
    assert info.startswith(INFO) and info.count("_kernel") == 1 and info.count(KERNEL) == 1, info
    want = model.value_and_bias(x, restraint=walls, grid=grid, opes=table.record(rc.SCALE, total / n if n else 1.0, rc.EPSILON, cols, n=n))
    torch.cuda.synchronize()
    assert "frames_value_bias_opes_f64_kernel" in vh._info(model)
    assert len(got) == 3 and all(torch.equal(a, b) for a, b in zip(got, want)), what
    assert [tuple(v.shape) for v in got] == [(x.shape[0], got[0].shape[1]), (x.shape[0], 4), tuple(x.shape)]
    assert bool((got[1][:, 1] == 0.0).all())
    return got, info


@pytest.mark.parametrize("n_inp,lanes", [(7, 8), (12, 16), (30, 32), (40, 64)])
@pytest.mark.parametrize("aligned", [True, False], ids=["aligned", "no_alignment"])
@pytest.mark.parametrize("head", [True, False], ids=["head", "features"])
def test_lane_groups(n_inp, lanes, aligned, head, hip_device):
    """Every lane-group width, with and without an alignment and a head, 1 and 65 frames, 40 live kernels under a capacity of 64, two
    permuted columns, the term's column 0 periodic, cutoff 5, walls on all outputs; once more with a 2-axis table on two other columns
    (the head has two outputs: the same two in the other order)."""
    case = vh._small_case(n_inp, aligned, head)
    model = case.build(hip_device).double().requires_grad_(False)
    d_out = case.mlp[-1] if head else case.d_feat()
    if head:       # the head's widest layer input (the 12 feature columns) asks for at least 16 lanes
        lanes = max(lanes, 16)
    cols, gcols = ((1, 0), (0, 1)) if head else ((4, 1), (5, 2))
    y_tab = _outputs(model, case.frames(65, seed=900 + n_inp, dev=CPU).double().to(hip_device), d_out)
    table = orun._filled_table(hip_device, y_tab[:, list(cols)], 40, 64, torch.tensor([1.3, 0.0], dtype=F64), CUTOFF, n_inp)
    walls = _walls(y_tab)
    for n in (1, 65):
        x = case.frames(n, seed=n_inp + n, dev=CPU).double().to(hip_device)
        for grid in (None, _grid(y_tab, gcols, n_inp)):
            (y, e, dx), info = _same_as_the_record(model, x, table, cols, walls, grid, (case.name, aligned, head, n, grid is not None))
            assert "%d lanes per frame" % lanes in info, info
            assert bool(torch.isfinite(e).all()) and float((e[:, 3] - FLOOR).abs().max()) > 0.0 and float(dx.abs().max()) > 0.0
            assert (grid is None) == bool((e[:, 2] == 0.0).all())
        if n == 65:
            assert float(e[:, 0].abs().max()) > 0.0, "no frame outside the walls"


@pytest.mark.parametrize("n", [1, 65])
@pytest.mark.parametrize("n_live", [0, 1, 300])
def test_table_sizes_on_c3(n_live, n, hip_device):
    """C3 (8 outputs), OPES on (5, 2), walls on all 8 and a table on (7, 0): no kernel yet, one, 300 under a capacity of 600.  Without
    kernels every table tensor holds NaN, V_o is scale log(epsilon) and the OPES share of dx is exactly 0: dx is the call's with walls
    and table alone."""
    w, model, _ = vv._shared("C3", hip_device)
    d = w.out_dim()
    x = w.make_frames(n, seed=21 + n).double().to(hip_device)
    y_tab = _outputs(model, w.make_frames(65, seed=22).double().to(hip_device), d)
    cols = (5, 2)
    walls, grid = _walls(y_tab), _grid(y_tab, (7, 0), 24)
    table = orun._filled_table(hip_device, y_tab[:, list(cols)], n_live, CAP, torch.tensor([0.0, 1.1], dtype=F64), 4.0, 23 + n_live)
    (y, e, dx), _ = _same_as_the_record(model, x, table, cols, walls, grid, (n_live, n))
    plain = model.value_and_bias(x, restraint=walls, grid=grid)
    assert torch.equal(y, plain[0]) and torch.equal(e[:, 0], plain[1][:, 0]) and torch.equal(e[:, 2], plain[1][:, 2])
    if n_live == 0:
        assert bool(torch.isnan(table.centers).all()) and bool(torch.isnan(table.sigma).all()) and bool(torch.isnan(table.heights).all())
        assert bool((e[:, 3] == FLOOR).all()) and torch.equal(dx, plain[2])
    else:
        assert bool(torch.isfinite(e).all()) and not torch.equal(dx, plain[2])
    # a count the table cannot hold is held to it: NaN and -1 read as no kernel, capacity + 5 as the whole table
    if n_live == 300 and n == 1:
        full = orun._filled_table(hip_device, y_tab[:, list(cols)], CAP, CAP, None, 4.0, 29)
        want = model.value_and_bias(x, restraint=walls, grid=grid, opes=full.record(rc.SCALE, full.read_state()[1] / CAP, rc.EPSILON, cols, n=CAP))
        for n0, kernels in ((NAN, 0), (-1.0, 0), (CAP + 5.0, CAP)):
            full.state[0] = n0
            got = model.value_and_bias(x, restraint=walls, grid=grid, opes=OpesFromTable(full, rc.SCALE, rc.EPSILON, cols))
            if kernels:
                assert all(torch.equal(a, b) for a, b in zip(got, want)), n0
            else:
                assert bool((got[1][:, 3] == FLOOR).all()) and torch.equal(got[2], plain[2]), n0


def test_larger_frames_p1(hip_device):
    w, model, _ = vv._shared("P1", hip_device)
    d = w.out_dim()
    cols = (d - 1, 0)
    y_tab = _outputs(model, w.make_frames(65, seed=8).double().to(hip_device), d)
    table = orun._filled_table(hip_device, y_tab[:, list(cols)], 75, 100, torch.tensor([1.1, 0.0], dtype=F64), 4.0, 60)
    (_, e, dx), _ = _same_as_the_record(model, w.make_frames(9, seed=7).double().to(hip_device), table, cols, _walls(y_tab), None, "P1")
    assert bool(torch.isfinite(e).all()) and float(dx.abs().max()) > 0.0


def test_both_ways_to_the_kernel_and_the_callers_buffers(hip_device, monkeypatch):
    """The dispatcher operator and the ctypes plan give the same bits; `into` is written and returned; an empty batch."""
    w, model, _ = vv._shared("C3", hip_device)
    d = w.out_dim()
    if ann._run_op() is None:
        pytest.fail("the operator library is not loaded: build() makes it")
    x = w.make_frames(65, seed=31).double().to(hip_device)
    y_tab = _outputs(model, x, d)
    cols = (5, 2)
    table = orun._filled_table(hip_device, y_tab[:, list(cols)], 45, 64, None, CUTOFF, 32)
    walls, grid = _walls(y_tab), _grid(y_tab, (7, 0), 33)
    rec = OpesFromTable(table, rc.SCALE, rc.EPSILON, cols)
    assert model._fast_state(x)["op"] is not None and model._fast_state(x)["op_bias_opes_table"] is not None
    a = model.value_and_bias(x, restraint=walls, grid=grid, opes=rec)
    torch.cuda.synchronize()
    assert vh._info(model).startswith(INFO)
    into = (torch.full((65, d), NAN, dtype=F64, device=hip_device), torch.full((65, 4), NAN, dtype=F64, device=hip_device), torch.full_like(x, NAN))
    b = model.value_and_bias(x, restraint=walls, grid=grid, opes=rec, into=into)
    assert all(u is v for u, v in zip(b, into)) and all(pl.same_bits(u, v) for u, v in zip(a, b))
    empty = model.value_and_bias(x[:0], opes=rec)
    assert [tuple(t.shape) for t in empty] == [(0, d), (0, 4), (0, w.n_atoms, 3)]
    with pytest.raises(ValueError, match=r"\[65, 8\], \[65, 4\]"):
        model.value_and_bias(x, opes=rec, into=(into[0], into[1][:, :3].contiguous(), into[2]))
    with pytest.raises(ValueError, match="epsilon"):
        model.value_and_bias(x, opes=rec._replace(epsilon=0.0))
    with pytest.raises(IndexError, match="columns"):
        model.value_and_bias(x, opes=rec._replace(columns=(8, 2)))
    monkeypatch.setattr(ann, "_run_op", lambda: None)
    plain = copy.deepcopy(model)                           # a copy drops the cached state: this one never sees the operators
    assert plain._fast_state(x)["op"] is None
    for kw in (dict(restraint=walls, grid=grid), dict(restraint=walls), dict()):
        want = model.value_and_bias(x, opes=rec, **kw)
        c = plain.value_and_bias(x, opes=rec, **kw)
        torch.cuda.synchronize()
        assert vh._info(plain).startswith(INFO) and vh._info(plain).count("_kernel") == 1
        assert all(torch.equal(u, v) for u, v in zip(c, want)), sorted(kw)
    c = plain.value_and_bias(x, restraint=walls, grid=grid, opes=rec, into=tuple(torch.full_like(t, NAN) for t in into))
    assert all(pl.same_bits(u, v) for u, v in zip(a, c))


def test_offset_caller_buffers_inside_guard_bands(hip_device):
    """`into=` buffers carved out of an arena at another residue of 16 bytes each, between guard bands: the outputs have the bits of
    the call on fresh tensors and no band is written."""
    w, model, _ = vv._shared("C3", hip_device)
    n, d = 65, w.out_dim()
    x = w.make_frames(n, seed=55).double().to(hip_device)
    y_tab = _outputs(model, x, d)
    cols = (5, 2)
    table = orun._filled_table(hip_device, y_tab[:, list(cols)], 45, 50, torch.tensor([1.1, 0.0], dtype=F64), 4.0, 56)
    walls, grid = _walls(y_tab), _grid(y_tab, (7, 0), 57)
    rec = OpesFromTable(table, rc.SCALE, rc.EPSILON, cols)
    fresh = model.value_and_bias(x, restraint=walls, grid=grid, opes=rec)
    arena = pl.Arena(hip_device, capacity=8 << 20)
    views = tuple(arena.carve(name, shape, F64, i % 2) for i, (name, shape) in enumerate((("out", (n, d)), ("energies", (n, 4)), ("grad_x", tuple(x.shape)))))
    assert len(set(v.data_ptr() % 16 for v in views)) == 2
    got = model.value_and_bias(x, restraint=walls, grid=grid, opes=rec, into=views)
    torch.cuda.synchronize()
    assert arena.check() == []
    assert all(u is v for u, v in zip(got, views)) and all(pl.same_bits(u, v) for u, v in zip(views, fresh))
    assert bool(torch.isfinite(fresh[2]).all()) and float(fresh[2].abs().max()) > 0.0


def test_the_entrys_codes_and_their_order(hip_device):
    """molann_value_and_bias_opes_table_f64 through ctypes on a real plan (C3's features, 8 columns), the outputs prefilled with NaN:
    molann_value_and_bias_opes_f64's codes in its order, with `capacity` and the table's three scalars in the place of `n_kernels`,
    `sigma_stride` and `norm`, and the table's three pointers and `state` required whatever the live count.  Nothing is written on a
    refusal."""
    w, model, _ = vv._shared("C3", hip_device)
    n = 5
    x = w.make_frames(n, seed=51).double().to(hip_device)
    pre = model.preprocessing_layer
    dp = pre.output_dimension()
    new = lambda *sh: torch.full(sh, NAN, dtype=F64, device=hip_device)       # noqa: E731
    f3, e4, dx3, f10 = new(n, dp), new(n, 4), new(n, w.n_atoms, 3), new(n, 10)
    plan = vv._feature_plan(pre, x)
    L, s = _capi.lib(), torch.cuda.current_stream().cuda_stream
    dev = dict(dtype=F64, device=hip_device)
    z, k = torch.zeros(dp, **dev), torch.ones(dp, **dev)
    c2, h2, s2 = torch.zeros((3, 2), **dev), torch.ones(3, **dev), torch.ones((3, 2), **dev)
    live, empty = torch.tensor([3.0, 2.0, 0.0, 0.0], **dev), torch.zeros(4, **dev)
    per = torch.zeros(2, **dev)
    t2 = torch.zeros((5, 6), **dev)
    good = (2.25, 1e-3, 4.0)
    R0, G0 = (z, k, None, None, 0), ([0, 5], t2, (5, 6), (0.0, 0.0), (1.0, 1.0), None)

    def term(cols=(4, 1), centers=c2, heights=h2, sigma=s2, capacity=3, state=live, period=per, scalars=good):
        return (list(cols) if isinstance(cols, (list, tuple)) and not (len(cols) == 2 and cols[0] is None) else cols, centers, heights, sigma, capacity,
                state, period) + tuple(scalars)

    def code(r=R0, g=G0, o=None, ptr=lambda t: t.data_ptr(), xp=None, null=(), hills=0, n_frames=n, p=None, out=None, change=None):
        terms, keep = _capi.bias_terms_f64(r, None, g, ptr=ptr)
        terms.n_hills_columns = hills
        tt, keep_o = _capi.opes_table_term_f64(term() if o is None else o, ptr=ptr)
        for name, v in (change or {}).items():
            setattr(tt, name, v)
        rc = L.molann_value_and_bias_opes_table_f64((p or plan)._handle, x.data_ptr() if xp is None else xp, n_frames, None, None,
                                                    None if "terms" in null else ctypes.byref(terms), None if "opes" in null else ctypes.byref(tt),
                                                    None if "out" in null else (out if out is not None else f3).data_ptr(),
                                                    None if "energies" in null else e4.data_ptr(), None if "grad_x" in null else dx3.data_ptr(), s)
        del keep, keep_o
        return rc

    E = _capi
    bad_scalars = term(scalars=(2.25, 0.0, 4.0))
    bad_grid = ([0, 5], t2, (5, 6), (0.0, 0.0), (1.0, NAN), None)
    off = lambda which: (lambda t: t.data_ptr() + (4 if t is which else 0))       # noqa: E731
    with torch.cuda.device(hip_device):
        assert plan.supports_value_and_bias_opes_table_f64() and L.molann_plan_supports_value_and_bias_opes_table_f64(plan._handle) == 1
        # 1. MOLANN_E_NULL: the term itself, the outputs, x, the walls' centre, the grid's table and host arrays, and - whatever the live
        #    count, with three kernels and with none - the table's three pointers and its state
        assert code(null=("opes",)) == E.E_NULL and code(r=(None, k, None, None, 0)) == E.E_NULL
        for name in ("out", "energies", "grad_x"):
            assert code(null=(name,)) == E.E_NULL, name
        assert code(xp=0) == E.E_NULL
        for state in (live, empty):
            for name in ("centers", "heights", "sigma", "state"):
                assert code(o=term(**dict({"state": state}, **{name: None}))) == E.E_NULL, (name, state is live)
        assert code(g=([0, 5], None, (5, 6), (0.0, 0.0), (1.0, 1.0), None)) == E.E_NULL and code(g=([0, 5], t2, None, (0.0, 0.0), (1.0, 1.0), None)) == E.E_NULL
        # 2. MOLANN_E_ALIGNMENT: every device pointer, `state` and the optional `period` among them; NULL before it, MOLANN_E_DESC after it
        for which in (c2, h2, s2, live, per, z, k, t2):
            assert code(ptr=off(which)) == E.E_ALIGNMENT
        assert code(xp=x.data_ptr() + 4) == E.E_ALIGNMENT
        assert code(o=term(state=None), xp=x.data_ptr() + 4) == E.E_NULL and code(o=term(capacity=0), xp=x.data_ptr() + 4) == E.E_ALIGNMENT
        assert code(o=bad_scalars, ptr=off(live)) == E.E_ALIGNMENT
        assert code(o=term(period=None)) == 0                                          # the period is optional
        torch.cuda.synchronize()
        assert bool(torch.isfinite(f3).all()) and bool(torch.isfinite(e4).all()) and bool(torch.isfinite(dx3).all())
        for v in (f3, e4, dx3):
            v.fill_(NAN)
        # 3. MOLANN_E_STAGE: a plan without items, after the pointers and before the term's values
        pa = _capi.Plan(22, align_idx=[0, 1, 2, 3], ref_x=torch.zeros(4, 3))
        assert not pa.supports_value_and_bias_opes_table_f64()
        assert code(p=pa, r=None, g=None) == E.E_STAGE and code(p=pa, r=None, g=None, o=term(capacity=0)) == E.E_STAGE
        assert code(p=pa, r=None, g=None, o=term(state=None)) == E.E_NULL
        # 4. MOLANN_E_DESC: the column count, a negative grid count, center_stride, capacity, the three scalars, the grid
        assert code(change=dict(n_columns=0)) == E.E_DESC and code(change=dict(n_columns=-1)) == E.E_DESC
        assert code(r=(z, k, None, None, 3)) == E.E_DESC and code(r=(z, k, None, None, dp + 1)) == E.E_DESC
        for capacity in (0, -1, -(1 << 40)):
            assert code(o=term(capacity=capacity)) == E.E_DESC, capacity
        for scalars in ((NAN, 1e-3, 4.0), (INF, 1e-3, 4.0), (2.25, 0.0, 4.0), (2.25, -1e-3, 4.0), (2.25, NAN, 4.0), (2.25, INF, 4.0), (2.25, 1e-3, 0.0),
                        (2.25, 1e-3, -4.0), (2.25, 1e-3, NAN)):
            assert code(o=term(scalars=scalars)) == E.E_DESC, scalars
        assert code(g=([0, 5], t2, (3, 6), (0.0, 0.0), (1.0, 1.0), None)) == E.E_DESC and code(g=bad_grid) == E.E_DESC
        # 5. hills columns in `terms`: MOLANN_E_UNSUPPORTED, after MOLANN_E_DESC and before the columns' codes
        assert code(hills=2) == E.E_UNSUPPORTED and code(hills=-1) == E.E_UNSUPPORTED
        assert code(hills=2, o=bad_scalars) == E.E_DESC and code(hills=2, g=bad_grid) == E.E_DESC and code(hills=2, o=term(capacity=0)) == E.E_DESC
        assert code(hills=2, o=term(cols=(4, dp))) == E.E_UNSUPPORTED
        # 6. the columns
        assert code(o=term(cols=(4, dp))) == E.E_INDEX and code(o=term(cols=(4, 4))) == E.E_INDEX and code(o=term(cols=(-1, 4))) == E.E_INDEX
        assert code(g=([-1, 5], t2, (5, 6), (0.0, 0.0), (1.0, 1.0), None)) == E.E_INDEX and code(g=([5, 5], t2, (5, 6), (0.0, 0.0), (1.0, 1.0), None)) == E.E_INDEX
        assert code(o=term(cols=(4, 4), capacity=0)) == E.E_DESC                                                   # the capacity, then a column
        p1 = _capi.Plan(22, features=[(wl.BOND, [0, 1])] * 10)
        c9 = torch.zeros((3, 9), **dev)
        wide = dict(p=p1, out=f10, r=None, g=None)
        assert code(o=term(cols=list(range(9)), centers=c9, sigma=c9, period=None), **wide) == E.E_UNSUPPORTED
        assert code(o=term(cols=(None, 9), centers=c9, sigma=c9, period=None), **wide) == E.E_UNSUPPORTED
        assert code(o=term(cols=list(range(8)) + [10], centers=c9, sigma=c9, period=None), **wide) == E.E_INDEX     # INDEX before UNSUPPORTED
        p2 = _capi.Plan(22, features=[(wl.BOND, [0, 1])] * 2)
        assert code(o=term(cols=(None, 3), centers=c9, sigma=c9, period=None), p=p2, out=f10, r=None, g=None) == E.E_INDEX   # a NULL list longer than out_dim
        # 7. n_frames: negative MOLANN_E_DESC; 0 returns before anything of the terms is looked at
        assert code(n_frames=-1) == E.E_DESC and code(n_frames=0) == 0 and code(n_frames=0, o=term(capacity=0, state=None), hills=2) == 0
        assert code(n_frames=0, null=("out", "energies", "grad_x"), xp=0) == 0 and code(n_frames=0, null=("opes",)) == E.E_NULL
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(t).all()) for t in (e4, dx3, f3, f10)), "a refusal launched"
    # terms == NULL is a call without walls or a table; a state of no kernels reads nothing of a NaN table
    with torch.cuda.device(hip_device):
        assert code(null=("terms",)) == 0
        torch.cuda.synchronize()
        assert bool(torch.isfinite(f3).all()) and bool((e4[:, :3] == 0).all()) and bool(torch.isfinite(dx3).all())
        assert code(null=("terms",), o=term(centers=new(3, 2), heights=new(3), sigma=new(3, 2), state=empty, scalars=(rc.SCALE, rc.EPSILON, 4.0))) == 0
        torch.cuda.synchronize()
        assert bool((e4[:, 3] == FLOOR).all()) and float(dx3.abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------- the step against its host twin
class _NoModel(object):
    def value_and_opes_table(self, *args, **kwargs):
        raise AssertionError("the step tests deposit only")

    value_and_bias = value_and_opes_table


def _device_run(dev, sc, n0, columns, capacity=CAP):
    period, table, y, V, sigma0, sigma_min = sc
    t = mbias.OpesTable(capacity, y.shape[1], dev, period=period, cutoff=CUTOFF, threshold=THRESHOLD)
    t.centers[:n0], t.sigma[:n0], t.heights[:n0] = (v.to(dev) for v in table)
    t.state[:2] = torch.tensor([float(n0), cases.brute_force_S(*table, period, CUTOFF)], dtype=F64).to(dev)
    run = mbias.OpesRun(_NoModel(), t, rc.KT, rc.BIASFACTOR, rc.BARRIER, sigma0, sigma_min, columns=columns)
    run.run[:3] = torch.tensor(rc.RUN0, dtype=F64).to(dev)
    return t, run


@pytest.mark.parametrize("width", [1, 4])
@pytest.mark.parametrize("n0", [60, 520])
def test_the_columns_step_matches_its_host_twin_and_the_plain_step(n0, width, hip_device):
    dev = hip_device
    sc = rc.step_scenario(n0, 2)
    wide, energies = hb._scatter(sc[2], sc[3])
    host = hb._fresh_host(sc, n0)
    for i in range(0, 16, width):
        assert hb.columns_step(host, wide[i:i + width], energies[i:i + width]) == 0
    t, run = _device_run(dev, sc, n0, hb.COLS)
    wide_d, energies_d = wide.to(dev), energies.to(dev)
    for i in range(0, 16, width):
        assert run.deposit(wide_d[i:i + width], energies_d[i:i + width]) is None
    got = orun._snapshot(t, run)
    worst, bits = rc.assert_same_run(got, host.snapshot(), (n0, width))
    print("n0 %d W %d: worst error / bound %.3g, %s" % (n0, width, worst, "the host's bits" if bits else "exp or pow an ulp off"))
    assert float(got[4][0]) == rc.RUN0[0] + 16 and int(got[3][2]) > 0
    # the device's plain step on the gathered contiguous copy: the same bits; so is the bias as a [W] tensor
    t2, run2 = orun._device_run(dev, sc, n0)
    y, V = sc[2].to(dev), sc[3].to(dev)
    for i in range(0, 16, width):
        run2.deposit(y[i:i + width], V[i:i + width])
    assert all(torch.equal(a, b) for a, b in zip(got, orun._snapshot(t2, run2)))
    t3, run3 = _device_run(dev, sc, n0, hb.COLS)
    for i in range(0, 16, width):
        run3.deposit(wide_d[i:i + width], V[i:i + width])
    assert all(torch.equal(a, b) for a, b in zip(got, orun._snapshot(t3, run3)))
    assert torch.equal(wide_d.cpu(), wide) and torch.equal(energies_d.cpu(), energies)


def test_the_raw_columns_step_inside_guard_bands(hip_device):
    """The C entry on a table, state, run, outputs and energies carved out of an arena, the table with no row to spare at the start:
    no band and no input is written, and the host twin's run."""
    dev, n0 = hip_device, 60
    sc = rc.step_scenario(n0, 2)
    period, table, y, V, sigma0, sigma_min = sc
    wide, energies = hb._scatter(y, V)
    arena = pl.Arena(dev, capacity=4 << 20)
    centers, sigma = arena.carve("centers", (n0, 2), F64, 1), arena.carve("sigma", (n0, 2), F64, 0)
    heights, state = arena.carve("heights", (n0,), F64, 1, row_dims=0), arena.carve("state", (4,), F64, 0, row_dims=0)
    run = arena.carve("run", (8,), F64, 1, row_dims=0)
    per = arena.carve("period", (2,), F64, 0, data=period, row_dims=0)
    yy, ee = arena.carve("y", wide.shape, F64, 1, data=wide), arena.carve("energies", energies.shape, F64, 0, data=energies)
    s0, smin = arena.carve("sigma0", (2,), F64, 1, data=sigma0, row_dims=0), arena.carve("sigma_min", (2,), F64, 0, data=sigma_min, row_dims=0)
    centers.copy_(table[0]), sigma.copy_(table[1]), heights.copy_(table[2]), run.zero_()
    host = hb._fresh_host(sc, n0, cap=n0)
    state.copy_(host.table.state)
    run[:3] = torch.tensor(rc.RUN0, dtype=F64).to(dev)
    assert hb.columns_step(host, wide, energies) == 0
    with torch.cuda.device(dev):
        _capi.opes_step_columns_f64(centers, sigma, heights, state, run, per, yy, _capi._i32_array(hb.COLS), ee[:, 3], s0, smin, rc.BETA, THRESHOLD,
                                    CUTOFF, False)
    torch.cuda.synchronize()
    assert arena.check() == [] and arena.inputs_changed() == []
    got = tuple(v.cpu() for v in (centers, sigma, heights, state, run))
    rc.assert_same_run(got, host.snapshot(), "arena")
    assert float(got[4][0]) == rc.RUN0[0] + 16 and int(got[3][2]) + int(got[3][3]) > 0


# ---------------------------------------------------------------------------------------------- the loop
STEPS, WALKERS, LOOP_CAP, COLS = 30, 4, 128, (5, 2)
_LOOP = {}


def _loop_model(dev):
    if "model" not in _LOOP:
        w, model, _ = vv._shared("C3", dev)
        d = w.out_dim()
        assert d == 8
        xs = [w.make_frames(WALKERS, seed=500 + i).double().to(dev) for i in range(STEPS)]
        y_all = torch.cat([_outputs(model, x, d) for x in xs])
        sub = y_all[:, list(COLS)].cpu()
        sigma0 = 0.35 * sub.std(dim=0)
        _LOOP.update(model=model, w=w, xs=xs, y_all=y_all.cpu(), sigma0=sigma0, sigma_min=0.7 * sigma0, walls=_walls(y_all),
                     period=torch.tensor([0.0, 4.0 * float(sub[:, 1].abs().max())], dtype=F64))
    return _LOOP


def _new_run(dev):
    L = _loop_model(dev)
    table = mbias.OpesTable(LOOP_CAP, 2, dev, period=L["period"], cutoff=CUTOFF, threshold=THRESHOLD)
    return mbias.OpesRun(L["model"], table, rc.KT, rc.BIASFACTOR, rc.BARRIER, L["sigma0"], L["sigma_min"], columns=COLS, walls=L["walls"])


def _eager_loop(dev):
    """The eager loop, once: per step (y, energies, dx) and the table, state and run after it, all on the CPU."""
    if "eager" not in _LOOP:
        L = _loop_model(dev)
        run = _new_run(dev)
        steps = []
        for x in L["xs"]:
            y, e, dx = run.bias(x)
            assert run.deposit(y, e) is None
            steps.append(tuple(t.cpu() for t in (y, e, dx)) + (orun._snapshot(run.table, run),))
        _LOOP["eager"] = steps
    return _LOOP["eager"]


def test_the_eager_loop_against_the_cpu_loop_of_the_host_twins(hip_device):
    """The bounds of tests/test_gpu_opes_run_f64.py's loop test: the energies within rc.BOUND max(1, |value|) of the bias twin's on the
    host's own table, counts and slots equal and rows and scalars within rc.BOUND by `rc.assert_same_run`, at every step."""
    L, eager = _loop_model(hip_device), _eager_loop(hip_device)
    host = rc.HostRun(LOOP_CAP, 2, L["period"], CUTOFF, THRESHOLD, L["sigma0"], L["sigma_min"], False)
    walls = tuple(None if v is None else v.cpu() for v in (L["walls"].center, L["walls"].kappa, L["walls"].period, L["walls"].flat))
    worst_v = worst = 0.0
    bound_steps = 0
    for i, (y, e, dx, after) in enumerate(eager):
        assert torch.equal(y, L["y_all"][WALKERS * i:WALKERS * (i + 1)])      # the outputs do not depend on the table
        t = host.table
        he = torch.empty(WALKERS, 4, dtype=F64)
        for a in range(WALKERS):
            code, he[a], _ = hb.table_selftest(y[a].contiguous(), COLS, (t.centers, t.heights, t.sigma), t.state, t.period,
                                               (rc.SCALE, rc.EPSILON, CUTOFF), restraint=walls)
            assert code == 0
        # the device sums P lane by lane, the host in one sequence: at most 128 positive terms, each an exp at 1-2 ulp
        worst_v = max(worst_v, float(((e - he).abs() / (rc.BOUND * torch.clamp(he.abs(), min=1.0))).max()))
        assert bool((e[:, 1] == 0.0).all()) and bool((e[:, 2] == 0.0).all())
        assert hb.columns_step(host, y, he) == 0
        ratio, _ = rc.assert_same_run(after, host.snapshot(), "step %d" % i)
        worst = max(worst, ratio)
        bound_steps += int(bool((float(host.run[4]) * L["sigma0"] < L["sigma_min"]).any()))
    print("30 steps of 4 walkers on outputs (5, 2) of 8: n %d merges %d refused %d; worst error / bound: energies %.3g, table and scalars %.3g; "
          "sigma_min held a width up in %d of %d steps; sigma_scale %.4g, neff %.4g"
          % (host.table.counts() + (worst_v, worst, bound_steps, STEPS, float(host.run[4]), float(host.run[3]))))
    assert worst_v <= 1.0
    n, merges, refused = host.table.counts()
    assert merges > 0 and n > 2 and refused == 0 and float(host.run[4]) < 1.0 and 0 < bound_steps < STEPS
    assert float(eager[-1][1][:, 0].abs().max()) > 0.0, "no walker outside the walls"
    # the first step has no kernels: dx is the walls' alone; the last has the OPES share
    plain = L["model"].value_and_bias(L["xs"][0], restraint=L["walls"])
    assert torch.equal(eager[0][2], plain[2].cpu()) and bool((eager[0][1][:, 3] == FLOOR).all())
    last = L["model"].value_and_bias(L["xs"][-1], restraint=L["walls"])
    assert not torch.equal(eager[-1][2], last[2].cpu())


def test_one_captured_graph_replays_the_loop_and_reads_device_memory(hip_device):
    dev = hip_device
    L, eager = _loop_model(dev), _eager_loop(dev)
    run = _new_run(dev)
    t = run.table
    x_static = L["xs"][0].clone()
    into = (torch.empty(WALKERS, 8, dtype=F64, device=dev), torch.empty(WALKERS, 4, dtype=F64, device=dev), torch.empty_like(x_static))
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):               # a step outside the capture: plans, libraries and caches are made here
        run.deposit(*run.bias(x_static, into=into)[:2])
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    for v in (t.centers, t.sigma, t.heights, t.state, run.run):
        v.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):               # one stream, two launches in a chain
        run.deposit(*run.bias(x_static, into=into)[:2])
    torch.cuda.synchronize()
    assert float(t.state.abs().max()) == 0.0 and float(run.run.abs().max()) == 0.0, "the capture ran the launches"
    for i, (x, (y, e, dx, after)) in enumerate(zip(L["xs"], eager)):
        x_static.copy_(x)
        graph.replay()
        got = tuple(u.cpu() for u in into)
        assert all(pl.same_bits(a, b) for a, b in zip(got, (y, e, dx))), "step %d: y, energies or dx" % i
        assert all(pl.same_bits(a, b) for a, b in zip(orun._snapshot(t, run), after)), "step %d: table, state or run" % i
    # another table and state under the same graph: the launches read device memory, nothing was baked in at capture
    last = tuple(u.cpu() for u in into)
    snap = eager[9][3]
    for dst, src in zip((t.centers, t.sigma, t.heights, t.state, run.run), snap):
        dst.copy_(src.to(dev))
    x_static.copy_(L["xs"][10])
    graph.replay()
    got = tuple(u.cpu() for u in into)
    assert all(pl.same_bits(a, b) for a, b in zip(got, eager[10][:3])) and not pl.same_bits(got[1], last[1])
    assert all(pl.same_bits(a, b) for a, b in zip(orun._snapshot(t, run), eager[10][3]))


def test_a_nan_walker_changes_no_other_walkers_outputs_and_is_refused_alone(hip_device):
    dev = hip_device
    L, eager = _loop_model(dev), _eager_loop(dev)
    run = _new_run(dev)
    for dst, src in zip((run.table.centers, run.table.sigma, run.table.heights, run.table.state, run.run), eager[19][3]):
        dst.copy_(src.to(dev))
    x = L["xs"][20]
    clean = dict(zip(("y", "V", "dx"), run.bias(x)))
    assert all(pl.same_bits(clean[k].cpu(), want) for k, want in zip(("y", "V", "dx"), eager[20][:3]))
    bad_x = isolation.poison({"x": x}, [2], "nan", where={"x": 3 * isolation.chosen_atom([a - 1 for a in L["w"].align],
                                                                                       [(ty, [a - 1 for a in at]) for ty, at in L["w"].features])
                                                          + isolation.COORD})["x"]
    poisoned = dict(zip(("y", "V", "dx"), run.bias(bad_x)))
    torch.cuda.synchronize()
    assert isolation.keep_rows_equal(clean, poisoned, [2], ("y", "V", "dx")) == []
    assert not bool(torch.isfinite(poisoned["V"][2, 3])) and bool(torch.isnan(poisoned["dx"][2]).any())
    # and the step refuses that walker alone
    run.deposit(poisoned["y"], poisoned["V"])
    state, scalars = run.table.read_state(), run.read_run()
    assert state[3] == 1 and scalars["counter"] == WALKERS * 20 + 3 and math.isfinite(scalars["neff"]) and math.isfinite(state[1])
