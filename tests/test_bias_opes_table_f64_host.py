"""An OPES run with walls, a table and chosen outputs, without a GPU: the two host twins `molann_selftest_bias_opes_table_f64` (one frame
of molann_value_and_bias_opes_table_f64: n and norm from the table's state) and `molann_selftest_opes_step_columns_f64` (the step on
strided outputs and chosen columns).

  bias      the twin equals `molann_selftest_bias_opes_f64` called with n and S / n formed from the state: `==` on doubles, since from
            there on it is the same code.
  step      on a [W, 8] buffer with columns (5, 2) and the bias in column 3 of a [W, 4] buffer the twin equals
            `molann_selftest_opes_step_f64` on the gathered contiguous copy: table, state and run bit for bit.
  refusals  every code of the two device entries that needs no plan, of their twins, and their order, with nothing written.
  python    `OpesFromTable`, `OpesRun(columns=, walls=, grid=)` and `value_and_bias(opes=OpesFromTable)`: the error types, each before a
            launch (the tables are stand-ins that hold what the checks look at: a table cannot be made without a device)."""

import ctypes
import math

import pytest
import torch

import opes_deposit_cases as cases
import opes_run_cases as rc
import test_bias_opes_f64_host as bo
from molann_amd import _capi, ann
from molann_amd import bias as mbias
from molann_amd.bias import Grid, Hills, Opes, OpesFromTable, OpesRun, OpesTable, Restraint

F64 = torch.float64
NAN, INF = float("nan"), float("inf")
SCALE, EPSILON, CUTOFF = 2.25, 1e-3, 5.0
SYMBOLS = {"molann_value_and_bias_opes_table_f64": 11, "molann_plan_supports_value_and_bias_opes_table_f64": 1, "molann_opes_step_columns_f64": 21,
           "molann_selftest_bias_opes_table_f64": 6, "molann_selftest_opes_step_columns_f64": 20}


def _ptr(t):
    return None if t is None else t.data_ptr()


# ---------------------------------------------------------------------------------------------- the bias from the table's state
def table_selftest(y, cols, table, state, period, scalars=(SCALE, EPSILON, CUTOFF), restraint=None, grid=None, hills_columns=0, no_terms=False,
                   capacity=None):
    """molann_selftest_bias_opes_table_f64 on host tensors: table = (centers [cap, w], heights [cap], sigma [cap, w]); restraint and grid as
    test_bias_opes_f64_host.selftest takes them.  Returns (code, energies, dy)."""
    d_out = y.numel()
    r = g = None
    if restraint is not None:
        r = restraint + (0,)
    if grid is not None:
        gcols, gt, lower, spacing, periodic = grid
        g = ((None, gt.dim()) if gcols is None else gcols, gt, gt.shape, lower, spacing, periodic)
    terms, keep = _capi.bias_terms_f64(r, None, g)
    terms.n_hills_columns = hills_columns
    centers, heights, sigma = table
    width = centers.shape[1]
    term, keep_o = _capi.opes_table_term_f64(((None, width) if cols is None else cols, centers, heights, sigma,
                                              centers.shape[0] if capacity is None else capacity, state, period) + tuple(scalars))
    energies, dy = torch.full((4,), 7.5, dtype=F64), torch.full((d_out,), 7.5, dtype=F64)
    code = _capi.lib().molann_selftest_bias_opes_table_f64(_ptr(y), d_out, None if no_terms else ctypes.byref(terms), ctypes.byref(term),
                                                           _ptr(energies), _ptr(dy))
    del keep, keep_o
    return code, energies, dy


def _kernel_table(cap, width, seed):
    g = torch.Generator().manual_seed(seed)
    centers = 1.5 * torch.randn(cap, width, generator=g, dtype=F64)
    return centers, 0.5 + torch.rand(cap, generator=g, dtype=F64), 0.3 + torch.rand(cap, width, generator=g, dtype=F64)


def _walls_and_grid(d_out, seed):
    g = torch.Generator().manual_seed(seed)
    z, kappa = torch.randn(d_out, generator=g, dtype=F64), 5.0 * torch.rand(d_out, generator=g, dtype=F64)
    flat = 0.5 * torch.rand(d_out, generator=g, dtype=F64)
    table = torch.randn(6, 5, generator=g, dtype=F64)
    return (z, kappa, None, flat), ([d_out - 1, 1], table, [-2.0, -2.0], [0.9, 1.1], [True, False])


@pytest.mark.parametrize("cols", [None, [5, 2, 7]], ids=["identity", "permuted"])
@pytest.mark.parametrize("terms", ["alone", "walls", "grid", "walls+grid"])
def test_the_twin_is_the_other_twin_on_the_states_count_and_norm(cols, terms):
    """Live counts 0, 1, 40 under a capacity of 64; state[0] NaN, negative and above the capacity (held to [0, capacity]); the dead rows
    hold NaN, so reading one would show."""
    d_out, width, cap = 8, 3, 64
    full = _kernel_table(cap, width, 17)
    period = torch.tensor([0.0, 3.0, 0.0], dtype=F64)
    walls, grid = _walls_and_grid(d_out, 18)
    kw = dict(restraint=walls if "walls" in terms else None, grid=grid if "grid" in terms else None)
    g = torch.Generator().manual_seed(19)
    seen = set()
    for state0, n in ((0.0, 0), (1.0, 1), (40.0, 40), (NAN, 0), (-3.0, 0), (-0.0, 0), (0.5, 0), (cap + 5.0, cap), (INF, cap), (40.7, 40)):
        table = tuple(v.clone() for v in full)
        for v in table:
            v[n:] = NAN
        total = 37.5 + 1.25 * n            # any finite S > 0: the twin divides what it finds
        state = torch.tensor([state0, total, 3.0, 1.0], dtype=F64)
        for trial in range(3):
            y = 1.5 * torch.randn(d_out, generator=g, dtype=F64)
            if n and trial:
                y[[0, 1, 2] if cols is None else cols] = table[0][trial % n] + 0.2 * torch.randn(width, generator=g, dtype=F64)
            code, energies, dy = table_selftest(y, cols, table, state, period, **kw)
            norm = total / n if n else 1.0
            want = bo.selftest(y, (cols, table[0][:n], table[1][:n], table[2][:n] if n else table[2][0], period, SCALE, norm, EPSILON, CUTOFF), **kw)
            assert code == 0 and want[0] == 0, (state0, code, want[0])
            assert energies.tolist() == want[1].tolist() and dy.tolist() == want[2].tolist(), (state0, trial)
            assert bool(torch.isfinite(energies).all()) and bool(torch.isfinite(dy).all())
            if n == 0:
                assert energies[3].item() == SCALE * math.log(EPSILON)
                plain = bo.bh.selftest(y, restraint=kw["restraint"], grid=kw["grid"])[2] if terms != "alone" else torch.zeros(d_out, dtype=F64)
                assert torch.equal(dy, plain), "the OPES share of the cotangent is exactly 0 without kernels"
            elif trial:
                seen.add(bool(energies[3].item() > SCALE * math.log(EPSILON) + 1e-6))
    assert seen == {True}, "a frame on a live kernel has a bias above the floor"
    assert state.tolist()[2:] == [3.0, 1.0]


def test_a_broken_sum_is_not_guarded():
    """S is the caller's: with n >= 1 a NaN or a zero S goes into the transform as it is, as on the device."""
    table = _kernel_table(4, 2, 3)
    y = torch.zeros(5, dtype=F64)
    y[[3, 1]] = table[0][0]              # on a kernel: P > 0
    for total in (NAN, 0.0):
        code, energies, dy = table_selftest(y, [3, 1], table, torch.tensor([4.0, total, 0.0, 0.0], dtype=F64), None)
        assert code == 0 and not math.isfinite(energies[3].item()), total
    code, energies, dy = table_selftest(y, [3, 1], table, torch.tensor([0.0, NAN, 0.0, 0.0], dtype=F64), None)
    assert code == 0 and energies[3].item() == SCALE * math.log(EPSILON) and not bool(dy.any())       # no kernels: the norm is not formed


def test_refusals_of_the_bias_twin_in_the_order_of_the_entry():
    E = _capi
    y = torch.linspace(-1.0, 1.0, 10, dtype=F64)
    table, state = _kernel_table(4, 2, 5), torch.tensor([3.0, 2.0, 0.0, 0.0], dtype=F64)
    z, k = torch.zeros(10, dtype=F64), torch.ones(10, dtype=F64)
    grid_t = torch.zeros((4, 5), dtype=F64)
    good_grid, bad_grid = ([9, 0], grid_t, [0.0, 0.0], [1.0, 1.0], None), ([0, 1], grid_t, [0.0, 0.0], [1.0, 0.0], None)
    assert table_selftest(y, [7, 2], table, state, None, restraint=(z, k, None, None), grid=good_grid)[0] == 0
    assert table_selftest(y, [7, 2], table, state, None, no_terms=True)[0] == 0
    wide = _kernel_table(4, 9, 6)
    rows = [
        (dict(capacity=0), E.E_DESC), (dict(capacity=-2), E.E_DESC),
        (dict(scalars=(NAN, EPSILON, CUTOFF)), E.E_DESC), (dict(scalars=(INF, EPSILON, CUTOFF)), E.E_DESC), (dict(scalars=(SCALE, 0.0, CUTOFF)), E.E_DESC),
        (dict(scalars=(SCALE, -1e-3, CUTOFF)), E.E_DESC), (dict(scalars=(SCALE, NAN, CUTOFF)), E.E_DESC), (dict(scalars=(SCALE, EPSILON, 0.0)), E.E_DESC),
        (dict(scalars=(SCALE, EPSILON, NAN)), E.E_DESC), (dict(grid=bad_grid), E.E_DESC),
        # ... before the hills' MOLANN_E_UNSUPPORTED, which comes before the columns' codes
        (dict(capacity=0, hills_columns=2), E.E_DESC), (dict(grid=bad_grid, hills_columns=2), E.E_DESC), (dict(hills_columns=2), E.E_UNSUPPORTED),
        (dict(cols=[2, 10], hills_columns=2), E.E_UNSUPPORTED),
        (dict(cols=[2, 10]), E.E_INDEX), (dict(cols=[-1, 2]), E.E_INDEX), (dict(cols=[4, 4]), E.E_INDEX), (dict(grid=([3, 3],) + good_grid[1:]), E.E_INDEX),
        (dict(cols=list(range(9)), table=wide), E.E_UNSUPPORTED), (dict(cols=None, table=wide), E.E_UNSUPPORTED),
        (dict(cols=[2, 10], capacity=0), E.E_DESC), (dict(cols=[2, 10], grid=bad_grid), E.E_DESC),
    ]
    for change, code in rows:
        args = dict(cols=[7, 2], table=table)
        args.update(change)
        got, energies, dy = table_selftest(y, args.pop("cols"), args.pop("table"), state, None, **args)
        assert got == code, (change, got, code)
        assert bool((energies == 7.5).all()) and bool((dy == 7.5).all()), change
    # what the helper cannot say: a missing pointer (whatever the live count), a count of columns that is not positive
    out = torch.full((14,), 7.5, dtype=F64)
    for change, code in ((dict(centers=None), E.E_NULL), (dict(heights=None), E.E_NULL), (dict(sigma=None), E.E_NULL), (dict(state=None), E.E_NULL),
                         (dict(n_columns=0), E.E_DESC), (dict(n_columns=-1), E.E_DESC), (dict(state=None, capacity=0), E.E_NULL)):
        for live in (0.0, 3.0):
            st = torch.tensor([live, 2.0, 0.0, 0.0], dtype=F64)
            term, keep = _capi.opes_table_term_f64(((None, 2),) + (table[0], table[1], table[2], 4, st, None, SCALE, EPSILON, CUTOFF))
            for name, v in change.items():
                setattr(term, name, v)
            assert _capi.lib().molann_selftest_bias_opes_table_f64(_ptr(y), 10, None, ctypes.byref(term), _ptr(out[:4]), _ptr(out[4:])) == code, change
            assert bool((out == 7.5).all())
    assert _capi.lib().molann_selftest_bias_opes_table_f64(_ptr(y), 10, None, None, _ptr(out[:4]), _ptr(out[4:])) == E.E_NULL
    assert table_selftest(y[:2].contiguous(), None, _kernel_table(4, 3, 7), state, None)[0] == E.E_INDEX      # d_out too small for 0..2


def test_the_bias_entry_without_a_plan():
    """What of molann_value_and_bias_opes_table_f64 can be seen without a device: a NULL plan comes first, whatever else is wrong.  The
    rest of its codes and their order, on a real plan: tests/test_gpu_opes_run_bias_f64.py, test_the_entrys_codes_and_their_order."""
    L = _capi.lib()
    assert L.molann_plan_supports_value_and_bias_opes_table_f64(None) == _capi.E_NULL
    terms, _ = _capi.bias_terms_f64()
    table, state = _kernel_table(4, 2, 5), torch.zeros(4, dtype=F64)
    term, keep = _capi.opes_table_term_f64(((None, 2), table[0], table[1], table[2], 4, state, None, SCALE, EPSILON, CUTOFF))
    for n in (1, 0, -1):
        assert L.molann_value_and_bias_opes_table_f64(None, None, n, None, None, ctypes.byref(terms), ctypes.byref(term), None, None, None, None) == _capi.E_NULL
        assert L.molann_value_and_bias_opes_table_f64(None, None, n, None, None, None, None, None, None, None, None) == _capi.E_NULL
    assert ctypes.sizeof(_capi.OpesTableTermF64) == 11 * 8 and _capi.OpesTableTermF64.scale.offset == 8 * 8 and _capi.OpesTableTermF64.capacity.offset == 5 * 8
    assert ctypes.sizeof(_capi.OpesTermF64) == 12 * 8          # the other term is what it was


# ---------------------------------------------------------------------------------------------- the step on strided outputs
COLS, N_OUT, V_STRIDE = (5, 2), 8, 4
ORDER = ("centers", "sigma", "heights", "capacity", "d", "period", "state", "run", "y", "y_stride", "columns", "V", "v_stride", "n_walkers", "sigma0",
         "sigma_min", "beta", "threshold", "cutoff", "fixed_sigma")


def _scatter(y, V, cols=COLS, n_out=N_OUT, seed=1):
    """y [W, d] into columns `cols` of a [W, n_out] buffer of noise and V into column 3 of a [W, 4] one."""
    g = torch.Generator().manual_seed(seed)
    wide = 3.0 * torch.randn(y.shape[0], n_out, generator=g, dtype=F64)
    wide[:, list(cols)] = y
    energies = 3.0 * torch.randn(y.shape[0], V_STRIDE, generator=g, dtype=F64)
    energies[:, 3] = V
    return wide, energies


def columns_step(host, wide, energies, cols=COLS):
    """`molann_selftest_opes_step_columns_f64` on an `rc.HostRun`'s table and run, the walkers read where they are."""
    t = host.table
    arr = None if cols is None else _capi._i32_array(cols)
    V = energies[:, 3]
    code = _capi.lib().molann_selftest_opes_step_columns_f64(
        _ptr(t.centers), _ptr(t.sigma), _ptr(t.heights), t.cap, host.d, _ptr(t.period), _ptr(t.state), _ptr(host.run), _ptr(wide), wide.stride(0), arr,
        V.data_ptr(), energies.stride(0), wide.shape[0], _ptr(host.sigma0), _ptr(host.sigma_min), rc.BETA, t.threshold, t.cutoff,
        1 if host.fixed_sigma else 0)
    return code


def _fresh_host(sc, n0, cap=600):
    period, table, y, V, sigma0, sigma_min = sc
    host = rc.HostRun(cap, y.shape[1], period, 5.0, 1.0, sigma0, sigma_min, False)
    host.table.fill(*table, cases.brute_force_S(*table, period, 5.0))
    host.run[:3] = torch.tensor(rc.RUN0, dtype=F64)
    return host


@pytest.mark.parametrize("width", [1, 4])
@pytest.mark.parametrize("n0", [60, 520])
def test_the_columns_step_is_the_step_on_the_gathered_copy(n0, width):
    """`rc.step_scenario` at d = 2 (the scenario's d > 1 branch: mixed periods, planted merges, the chain rounds, 12 appends)."""
    want, sc = rc.host_scenario_run(n0, 2, width)
    host = _fresh_host(sc, n0)
    wide, energies = _scatter(sc[2], sc[3])
    before = (wide.clone(), energies.clone())
    for i in range(0, wide.shape[0], width):
        assert columns_step(host, wide[i:i + width], energies[i:i + width]) == 0
    assert all(torch.equal(a, b) for a, b in zip(host.snapshot(), want.snapshot()))
    assert torch.equal(wide, before[0]) and torch.equal(energies, before[1])
    # in two dimensions the scenario's kernels crowd: merges and chain rounds are most of what happens
    assert int(host.table.state[2]) > 0 and int(host.table.state[3]) == 0 and float(host.run[0]) == rc.RUN0[0] + 16


@pytest.mark.parametrize("d", [1, 8])
def test_identity_columns_on_a_dense_buffer_are_the_plain_step(d):
    """columns NULL, y_stride = d, v_stride = 1: `rc.step_scenario`'s d = 1 and d = 8 cases, the plain twin's bits."""
    want, sc = rc.host_scenario_run(60, d, 4)
    host = _fresh_host(sc, 60)
    t, y, V = host.table, sc[2], sc[3]
    for i in range(0, 16, 4):
        yy, vv = y[i:i + 4].contiguous(), V[i:i + 4].contiguous()
        assert _capi.lib().molann_selftest_opes_step_columns_f64(
            _ptr(t.centers), _ptr(t.sigma), _ptr(t.heights), t.cap, d, _ptr(t.period), _ptr(t.state), _ptr(host.run), _ptr(yy), d, None, _ptr(vv), 1, 4,
            _ptr(host.sigma0), _ptr(host.sigma_min), rc.BETA, t.threshold, t.cutoff, 0) == 0
    assert all(torch.equal(a, b) for a, b in zip(host.snapshot(), want.snapshot()))


def test_a_nan_in_an_unchosen_column_refuses_nobody_and_in_a_chosen_one_that_walker_alone():
    n0 = 60
    sc = rc.step_scenario(n0, 2)
    y, V = sc[2][:4], sc[3][:4]
    clean = _fresh_host(sc, n0).step(y, V).snapshot()
    wide, energies = _scatter(y, V)
    # every unchosen output and every other energy column of every walker
    for col in range(N_OUT):
        if col not in COLS:
            wide[:, col] = NAN
    energies[:, :3] = NAN
    host = _fresh_host(sc, n0)
    assert columns_step(host, wide, energies) == 0
    assert all(torch.equal(a, b) for a, b in zip(host.snapshot(), clean)) and int(host.table.state[3]) == 0
    # a chosen output of walker 2, then its bias
    for where in ("y", "V"):
        bad_y, bad_V = y.clone(), V.clone()
        if where == "y":
            bad_y[2, 1] = NAN
        else:
            bad_V[2] = NAN
        want = _fresh_host(sc, n0).step(bad_y, bad_V).snapshot()
        wide, energies = _scatter(bad_y, bad_V)
        host = _fresh_host(sc, n0)
        assert columns_step(host, wide, energies) == 0
        got = host.snapshot()
        assert all(torch.equal(a, b) for a, b in zip(got, want))
        assert int(got[3][3]) == 1 and float(got[4][0]) == rc.RUN0[0] + 3 and bool(torch.isfinite(got[3]).all()) and bool(torch.isfinite(got[4]).all())


def _columns_step_refusals(call):
    """`call(**overrides)` -> code for the device entry or its host twin: molann_opes_step_f64's refusals in its order, then the strides
    (MOLANN_E_DESC), then the list (MOLANN_E_INDEX)."""
    ok = torch.zeros(32, dtype=F64)
    p, odd = ok.data_ptr(), ok.data_ptr() + 4
    cols = _capi._i32_array([5, 2])
    base = dict(centers=p, sigma=p, heights=p, capacity=4, d=2, period=None, state=p, run=p, y=p, y_stride=8, columns=cols, V=p, v_stride=4, n_walkers=1,
                sigma0=p, sigma_min=None, beta=1.0, threshold=1.0, cutoff=5.0, fixed_sigma=0)
    E = _capi
    for name in ("centers", "sigma", "heights", "state", "run", "y", "V", "sigma0"):
        assert call(**dict(base, **{name: None})) == E.E_NULL, name
        assert call(**dict(base, **{name: odd})) == E.E_ALIGNMENT, name
        assert call(**dict(base, **{name: None, "d": 0, "period": odd, "y_stride": 0})) == E.E_NULL, name      # NULL comes first
    for name in ("period", "sigma_min"):
        assert call(**dict(base, **{name: odd})) == E.E_ALIGNMENT
        assert call(**dict(base, **{name: odd, "d": 9, "v_stride": 0})) == E.E_ALIGNMENT                       # alignment before d and strides
    for d in (0, -1, 9):
        assert call(**dict(base, d=d)) == E.E_DESC
    assert call(**dict(base, capacity=0)) == E.E_DESC and call(**dict(base, n_walkers=-1)) == E.E_DESC
    for change in (dict(beta=0.0), dict(beta=NAN), dict(beta=INF), dict(threshold=-0.5), dict(threshold=NAN), dict(cutoff=0.0), dict(cutoff=NAN)):
        assert call(**dict(base, **change)) == E.E_DESC, change
        assert call(**dict(base, columns=_capi._i32_array([5, 5]), **change)) == E.E_DESC, change        # ... before the list
    # the three additions: a bad stride MOLANN_E_DESC, a bad column MOLANN_E_INDEX, the strides first
    for change in (dict(y_stride=1), dict(y_stride=0), dict(y_stride=-8), dict(v_stride=0), dict(v_stride=-1)):
        assert call(**dict(base, **change)) == E.E_DESC, change
        assert call(**dict(base, columns=_capi._i32_array([5, 5]), **change)) == E.E_DESC, change
    for bad in ([5, 5], [-1, 2], [5, 8], [8, 2], [2, 1 << 20]):
        assert call(**dict(base, columns=_capi._i32_array(bad))) == E.E_INDEX, bad
    assert call(**dict(base, y_stride=2, columns=_capi._i32_array([1, 2]))) == E.E_INDEX        # the list against y_stride, not a constant
    assert call(**dict(base, y_stride=2, columns=None, n_walkers=0)) == 0 and call(**dict(base, y_stride=1, columns=None, n_walkers=0)) == E.E_DESC
    # refused where n_walkers == 0 too; a good call with no walkers enqueues nothing and reads nothing
    assert call(**dict(base, n_walkers=0, columns=_capi._i32_array([5, 5]))) == E.E_INDEX
    assert call(**dict(base, n_walkers=0, centers=None, y=None, V=None)) == 0
    assert not bool(ok.any()), "a refusal wrote"


def test_every_refusal_of_the_columns_step_entry_and_of_its_host_twin():
    L = _capi.lib()
    _columns_step_refusals(lambda **kw: L.molann_opes_step_columns_f64(*[kw[k] for k in ORDER], None))      # refused before any launch: no GPU needed
    _columns_step_refusals(lambda **kw: L.molann_selftest_opes_step_columns_f64(*[kw[k] for k in ORDER]))


def test_the_symbols_are_declared_exported_and_bound():
    L = _capi.lib()
    for name, count in SYMBOLS.items():
        assert name in _capi.declared_symbols(), name
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == count and fn.restype is ctypes.c_int, name
    assert L.molann_abi_version() == 1
    assert callable(_capi.opes_step_columns_f64) and callable(_capi.Plan.value_and_bias_opes_table_f64)
    assert callable(_capi.Plan.supports_value_and_bias_opes_table_f64)
    assert "OpesFromTable" in mbias.__all__


def test_the_operators_are_registered():
    from molann_amd import script
    script.load_ops()
    for name in ("value_and_bias_opes_table", "value_and_bias_opes_table_h"):
        assert hasattr(torch.ops.molann, name)
    schema = str(torch.ops.molann.value_and_bias_opes_table_h.default._schema)
    assert "Tensor state" in schema and "float norm" not in schema and "int[] opes_columns" in schema


# ---------------------------------------------------------------------------------------------- the Python checks, device-free
def _stand_in(d=2, capacity=4, device="cpu"):
    """What the checks look at of an `OpesTable`: a table cannot be made without a device."""
    t = OpesTable.__new__(OpesTable)
    t.d, t.capacity, t.cutoff, t.period, t.threshold = d, capacity, None, None, 1.0
    t.centers, t.sigma = torch.zeros(capacity, d, dtype=F64, device=device), torch.zeros(capacity, d, dtype=F64, device=device)
    t.heights, t.state = torch.zeros(capacity, dtype=F64, device=device), torch.zeros(4, dtype=F64, device=device)
    return t


def test_the_record_is_immutable_holds_the_table_and_checks_its_columns():
    t = _stand_in()
    o = OpesFromTable(t, 0.9, 1e-9, columns=[5, 2])
    assert o.table is t and o.columns == (5, 2) and (o.scale, o.epsilon) == (0.9, 1e-9) and OpesFromTable(t, 0.9, 1e-9).columns is None
    assert OpesFromTable(t, 0.9, 1e-9, range(2)).columns == (0, 1)
    with pytest.raises(AttributeError):
        o.scale = 2.0
    assert o._replace(scale=2.0).table is t
    with pytest.raises(TypeError, match="OpesFromTable: `table` must be an OpesTable"):
        OpesFromTable((t.centers, t.heights, t.sigma), 0.9, 1e-9)
    for bad in ("01", 3, {0, 1}, torch.tensor([0, 1]), [0.0, 1.0], [True, False]):
        with pytest.raises(TypeError, match="OpesFromTable: `columns`"):
            OpesFromTable(t, 0.9, 1e-9, columns=bad)
    for bad in ([0, 0], [-1, 0]):
        with pytest.raises(IndexError, match="OpesFromTable: `columns`"):
            OpesFromTable(t, 0.9, 1e-9, columns=bad)
    for bad in ([1], [0, 1, 2]):
        with pytest.raises(ValueError, match=r"one output per column of `table` \(2\)"):
            OpesFromTable(t, 0.9, 1e-9, columns=bad)
    with pytest.raises(NotImplementedError, match=r"at most 8 columns \(got 9\)"):
        OpesFromTable(_stand_in(8), 0.9, 1e-9, columns=list(range(9)))


class _Model(object):
    def __init__(self):
        self.calls = []

    def value_and_opes_table(self, *args, **kwargs):
        self.calls.append(("value_and_opes_table", args, kwargs))
        return "plain"

    def value_and_bias(self, *args, **kwargs):
        self.calls.append(("value_and_bias", args, kwargs))
        return "terms"


class _PlainModel(object):
    def value_and_opes_table(self, *args, **kwargs):
        return "plain"


def test_opes_run_takes_columns_walls_and_a_grid_and_checks_them_once():
    t = _stand_in()
    good = dict(kT=1.0, biasfactor=10.0, barrier=20.0, sigma0=[0.3, 0.3])
    walls = Restraint(torch.zeros(8, dtype=F64), 2.0, flat=torch.ones(8, dtype=F64))
    grid = Grid(torch.zeros(5, 6, dtype=F64), [0.0, 0.0], [1.0, 1.0], columns=[7, 0])
    # with all three None nothing changes: `bias` is value_and_opes_table, and a model without value_and_bias still serves
    m = _Model()
    run = OpesRun(m, t, **good)
    assert run.columns is None and run.walls is None and run.grid is None
    assert run.bias("x", into="into") == "plain" and m.calls == [("value_and_opes_table", ("x", t, run.scale, run.epsilon), dict(into="into"))]
    assert OpesRun(_PlainModel(), t, **good).bias("x") == "plain"
    # otherwise `bias` is value_and_bias with the record of the table
    for kw in (dict(columns=[5, 2]), dict(walls=walls), dict(grid=grid), dict(columns=(5, 2), walls=walls, grid=grid)):
        m = _Model()
        run = OpesRun(m, t, **good, **kw)
        assert run.bias("x", into=None) == "terms"
        name, args, kwargs = m.calls[0]
        assert name == "value_and_bias" and args == ("x",) and kwargs["restraint"] is kw.get("walls") and kwargs["grid"] is kw.get("grid")
        o = kwargs["opes"]
        assert isinstance(o, OpesFromTable) and o.table is t and (o.scale, o.epsilon) == (run.scale, run.epsilon)
        assert o.columns == (None if "columns" not in kw else (5, 2)) and kwargs["into"] is None
        with pytest.raises(TypeError, match="value_and_bias"):
            OpesRun(_PlainModel(), t, **good, **kw)
    for bad, exc in (("52", TypeError), ([5, 5], IndexError), ([-1, 2], IndexError), ([5], ValueError), ([5, 2, 1], ValueError), ([5.0, 2.0], TypeError)):
        with pytest.raises(exc, match="OpesRun"):
            OpesRun(_Model(), t, **good, columns=bad)
    with pytest.raises(TypeError, match="`walls` must be a Restraint"):
        OpesRun(_Model(), t, **good, walls=(torch.zeros(8), 2.0))
    with pytest.raises(TypeError, match="`walls` must be a Restraint"):
        OpesRun(_Model(), t, **good, walls=grid)
    with pytest.raises(TypeError, match="`grid` must be a Grid"):
        OpesRun(_Model(), t, **good, grid=torch.zeros(5, 6, dtype=F64))
    with pytest.raises(TypeError, match="`grid` must be a Grid"):
        OpesRun(_Model(), t, **good, grid=walls)


def test_the_deposit_of_a_run_with_columns_checks_its_tensors_before_any_launch(monkeypatch):
    t = _stand_in()
    run = OpesRun(_Model(), t, 1.0, 10.0, 20.0, [0.3, 0.3], columns=[5, 2])
    monkeypatch.setattr(_capi, "opes_step_columns_f64", lambda *a, **k: pytest.fail("a refusal launched"))
    monkeypatch.setattr(_capi, "opes_step_f64", lambda *a, **k: pytest.fail("the plain step"))
    y, e = torch.zeros(4, 8, dtype=F64), torch.zeros(4, 4, dtype=F64)
    for bad_y, bad_e, exc in ((y.tolist(), e, TypeError), (y, None, TypeError), (y.float(), e, TypeError), (y, e.float(), TypeError),
                              (y.to("meta"), e, ValueError), (y[:, :5], e, ValueError), (y[0], e, ValueError), (y, e[:3], ValueError),
                              (y, e[:, :3], ValueError), (y, torch.zeros(4, 1, dtype=F64), ValueError), (y, torch.zeros(5, dtype=F64), ValueError)):
        with pytest.raises(exc, match="OpesRun.deposit"):
            run.deposit(bad_y, bad_e)
    assert run.deposit(y[:0], e[:0]) is None and run.deposit(y[:0], e[:0, 3]) is None       # no walkers: nothing launched


def test_value_and_bias_checks_an_opes_from_table_before_any_device_call():
    """ann._check_bias_opes_table_args is what both methods call before the plan is looked up; nothing of the table's tensors is read."""
    from molann_amd import workloads as wl
    n, n_inp, d = 5, 22, 12
    x = torch.zeros((n, n_inp, 3), dtype=F64)
    y, energies, dx = torch.zeros((n, d), dtype=F64), torch.zeros((n, 4), dtype=F64), torch.zeros_like(x)
    t = _stand_in(3, 16)
    for v in (t.centers, t.sigma, t.heights, t.state):
        v.fill_(NAN)                               # nothing is looked at: no widths check, no count
    R, G = Restraint(torch.zeros(d, dtype=F64), torch.ones(d, dtype=F64)), Grid(torch.zeros((5, 6), dtype=F64), [0.0, 0.0], [1.0, 1.0], columns=[9, 11])
    O = OpesFromTable(t, 0.9, 1e-9, columns=[11, 0, 4])

    def check(restraint=R, grid=G, opes=O, into=None, d_out=d):
        return ann._check_bias_opes_table_args("value_and_bias", x, d_out, restraint, grid, opes, into)

    r, g, o, *into = check(into=(y, energies, dx))
    assert g[0] == (9, 11) and o[0] == (11, 0, 4) and o[1] is t.centers and o[2] is t.heights and o[3] is t.sigma and o[4] is t.state and o[5] is None
    assert o[6:] == (0.9, 1e-9, INF) and into[0] is y and into[1] is energies and into[2] is dx
    r, g, o, *into = check(restraint=None, grid=None, opes=OpesFromTable(t, 2, 1e-3))
    assert r is None and g is None and o[0] == (0, 1, 2) and o[6:] == (2.0, 1e-3, INF) and into == [None, None, None]
    t.cutoff = 4.0
    assert check()[2][8] == 4.0
    with pytest.raises(IndexError, match=r"opes.columns.*\[0, 12\)"):
        check(opes=O._replace(columns=(0, 12, 4)))
    with pytest.raises(IndexError, match="3 columns but the model has 2 outputs"):
        check(restraint=None, grid=None, opes=O._replace(columns=None), d_out=2)
    for bad in ((0, 4), (0, 4, 11, 2)):         # a record changed through `_replace`: the message names the columns and the table
        with pytest.raises(ValueError, match=r"`opes\.columns` must name one output per column of `opes\.table` \(3\); got %d" % len(bad)):
            check(opes=O._replace(columns=bad))
    with pytest.raises(TypeError, match=r"`opes\.table` must be a molann_amd\.bias\.OpesTable"):
        check(opes=O._replace(table=(t.centers, t.heights)))
    for change, exc in ((dict(scale=INF), ValueError), (dict(scale=NAN), ValueError), (dict(epsilon=0.0), ValueError), (dict(epsilon=NAN), ValueError),
                        (dict(scale="1"), TypeError), (dict(epsilon=True), TypeError), (dict(scale=torch.tensor(1.0)), TypeError)):
        with pytest.raises(exc, match="scale|epsilon"):
            check(opes=O._replace(**change))
    moved = _stand_in(3, 16, device="meta")
    with pytest.raises(ValueError, match="`table` must be on cpu"):
        check(opes=O._replace(table=moved))
    with pytest.raises(ValueError, match="flat"):
        check(restraint=Restraint(R.center, R.kappa, flat=-R.kappa))
    with pytest.raises(ValueError, match="spacing"):
        check(grid=Grid(G.table, [0.0] * 2, [1.0, 0.0], columns=[9, 11]))
    with pytest.raises(TypeError, match=r"triple of tensors \(y, energies, dx\)"):
        check(into=(y, dx))
    for bad in ((y, energies[:, :3].contiguous(), dx), (y, energies[:, 0].contiguous(), dx), (y, energies, dx[1:]), (y, energies.t(), dx)):
        with pytest.raises(ValueError, match=r"\[5, 12\], \[5, 4\]"):
            check(into=bad)
    # the methods: the record's type and hills next to it are refused before the device gate, and the gate names the route that remains
    w = wl.get_workload("C3")
    model = wl.build_model(w, torch.device("cpu"), 0).double().requires_grad_(False)
    xc = w.make_frames(3, seed=1).double()
    t2 = _stand_in(2, 16)
    rec = OpesFromTable(t2, 0.9, 1e-9, columns=[5, 2])
    h = Hills(torch.zeros((4, 2), dtype=F64), 1.0, 0.5)
    for target in (model, model.preprocessing_layer):
        with pytest.raises(NotImplementedError, match=r"`hills` and `opes` in one launch.*add_hills_to_grid.*two calls"):
            target.value_and_bias(xc, hills=h, opes=rec)
        with pytest.raises(TypeError, match=r"`opes` must be None or a molann_amd\.bias\.Opes or OpesFromTable"):
            target.value_and_bias(xc, opes=(t2, 0.9, 1e-9))
    with pytest.raises(NotImplementedError, match=r"value_and_bias needs a model served by one fused plan.*OpesTable\.read_state.*"
                                                  r"value_and_bias\(opes=table\.record\(scale, S / n, epsilon, columns\)\)"):
        model.value_and_bias(xc, restraint=Restraint(torch.zeros(8, dtype=F64), 2.0), opes=rec)
    with pytest.raises(NotImplementedError, match=r"OpesTable\.read_state.*value_and_bias\(opes=table\.record.*torch\.autograd\.grad"):
        model.preprocessing_layer.value_and_bias(xc, opes=rec)
    with pytest.raises(NotImplementedError, match="read_state"):       # the gate comes before `into` and before the record's own arguments
        model.value_and_bias(xc, opes=rec._replace(scale=NAN, columns=(70, 71)), into=(xc,))


def test_the_kind_has_its_rows_and_the_docstrings_say_so():
    from molann_amd.ann import MolANN, PreprocessingANN
    k = ann._BIAS_OPES_TABLE
    assert len({len(t) for t in (ann._ONE_LAUNCH_NAME, ann._ONE_LAUNCH_ROUTE, ann._ONE_LAUNCH_FEATURES_ROUTE, ann._ONE_LAUNCH_PAIR, ann._ONE_LAUNCH_OP)}) == 1
    assert ann._ONE_LAUNCH_NAME[k] == "value_and_bias" and ann._ONE_LAUNCH_OP[k] == "op_bias_opes_table" and ann._ONE_LAUNCH_PAIR[k] == "(y, energies, dx)"
    assert k not in (ann._BIAS_OPES, ann._OPES_TABLE) and ann._ONE_LAUNCH_ROUTE[k].startswith("read the table's state")
    doc = " ".join(MolANN.value_and_bias.__doc__.split())
    for words in ("OpesFromTable", "frames_value_bias_opes_table_f64_kernel", "molann_value_and_bias_opes_table_f64", "Nothing is read back"):
        assert words in doc, words
    assert "OpesFromTable" in PreprocessingANN.value_and_bias.__doc__
    run_doc = " ".join(OpesRun.__doc__.split())
    assert "molann_opes_step_columns_f64" in run_doc and "``walls``" in run_doc and "explore" in run_doc
