"""Adaptive, correlated metadynamics hills on the host (no GPU): `molann_selftest_metad_widths_f64` and
`molann_selftest_metad_deposit_cov_f64` - the kernels' steps through the functions they call (molann_metad_cov.h), compiled for the
host - against tests/metad_cov_oracle.py, a plain numpy restatement that forms a hill's exponent with `np.linalg.solve`; then the
limits, the cutoff, the fixed-width twin on diagonal matrices, the refusals, and `bias.MetadRun`'s new arguments.  Cases and the bound
(1e-12 of the summed heights plus the table's largest entry): tests/metad_cov_cases.py."""

import ctypes
import math

import numpy as np
import pytest
import torch

from molann_amd import bias as mbias

import metad_cases as mc
import metad_cov_cases as cc
import metad_cov_oracle as oracle

F64, INF, NAN = cc.F64, cc.INF, cc.NAN
E_NULL, E_DESC, E_ALIGNMENT, E_UNSUPPORTED = -1, -2, -6, -7
CUTOFF = 3.3


def _run(case, cutoff=None, table=None, state=None, log=None, cov=None, height0=cc.HEIGHT0, inv_dT=cc.INV_DT):
    table = case.table.clone() if table is None else table
    state = torch.zeros(8, dtype=F64) if state is None else state
    code = cc.host_deposit_cov(table, case.lower, case.spacing, case.periodic, case.columns, case.y, case.V, case.cov if cov is None else cov,
                               height0, inv_dT, cutoff, state, log)
    assert code == 0, code
    return table, state


def _oracle(case, cutoff=None, state=None, log=None, cov=None, height0=cc.HEIGHT0, inv_dT=cc.INV_DT):
    return oracle.deposit(case.table.numpy(), case.lower, case.spacing, case.periodic, case.columns, case.y.numpy(), case.V.numpy(),
                          (case.cov if cov is None else cov).numpy(), height0, inv_dT, cutoff, np.zeros(8) if state is None else state, log)


def _assert_close(case, got, want, heights, what=""):
    tol = cc.tolerance(heights, case.table)
    err = float(np.abs(got.numpy() - want).max())
    print("%s shape %s W %d: error %.3g, bound %.3g" % (what, case.shape, case.walkers, err, tol))
    assert err <= tol, (err, tol)


# ---------------------------------------------------------------------------------------------- the deposit's twin against the oracle
@pytest.mark.parametrize("walkers", cc.WALKERS)
@pytest.mark.parametrize("shape,periodic", cc.SHAPES + cc.TILE_SHAPES)
def test_twin_matches_the_oracle(shape, periodic, walkers):
    case = cc.CovCase(shape, periodic, walkers)
    log = torch.zeros(walkers, case.d + case.T + 1, dtype=F64)
    got, state = _run(case, log=log)
    heights = mc.host_heights(case.V)
    want, want_state, want_log = _oracle(case, log=np.zeros(log.shape))
    _assert_close(case, got, want, heights, "oracle")
    assert state[:2].tolist() == [walkers, 0.0] and state[3:].tolist() == [1.0, walkers, 0.0, 0.0, 0.0]
    assert np.array_equal(want_state[[0, 1, 3, 4]], state.numpy()[[0, 1, 3, 4]])
    assert abs(float(state[2]) - want_state[2]) <= 1e-12 * want_state[2]
    d, T = case.d, case.T
    assert np.array_equal(log[:, :d].numpy(), want_log[:, :d])                                  # centres equal
    assert np.array_equal(log[:, d:d + T].numpy(), want_log[:, d:d + T])                        # the covariances are copied: within 1e-14 for sure
    assert float(np.abs(log[:, d + T].numpy() - want_log[:, d + T]).max()) <= 1e-14 * float(want_log[:, d + T].max())


def test_a_table_that_holds_values_already():
    case = cc.CovCase((5, 7), (True, False), 65, start="random")
    got, _ = _run(case)
    _assert_close(case, got, _oracle(case)[0], mc.host_heights(case.V))


@pytest.mark.parametrize("walkers", cc.WALKERS)
@pytest.mark.parametrize("shape,periodic", cc.SHAPES + cc.TILE_SHAPES[:1] + cc.TILE_SHAPES[2:3] + cc.TILE_SHAPES[4:5])
def test_cutoff_changes_the_entries_the_oracle_changes(shape, periodic, walkers):
    case = cc.CovCase(shape, periodic, walkers, start="random")
    margin = oracle.cutoff_margin(shape, case.lower, case.spacing, case.periodic, None, case.y.numpy(), case.cov.numpy(), CUTOFF)
    print("nearest grid point to the cutoff's edge: %.3g (relative, in q)" % margin)
    assert margin >= 1e-9, margin
    got, _ = _run(case, cutoff=CUTOFF)
    want, _, _ = _oracle(case, cutoff=CUTOFF)
    _assert_close(case, got, want, mc.host_heights(case.V))
    before = case.table.numpy()
    changed = got.numpy() != before
    assert np.array_equal(changed, want != before)
    assert np.array_equal(got.numpy()[~changed].view(np.int64), before[~changed].view(np.int64))


@pytest.mark.parametrize("shape,periodic", [((67,), (True,)), ((5, 7), (True, False)), ((17, 33), (True, False)), ((4, 5, 6), (False, True, False)),
                                            ((5, 9, 17), (False, False, True))])
@pytest.mark.parametrize("cutoff", [None, CUTOFF])
def test_a_diagonal_covariance_gives_the_fixed_width_twins_table(shape, periodic, cutoff):
    case = cc.CovCase(shape, periodic, 9, start="random")
    d = case.d
    diag = torch.from_numpy(np.tile(oracle.triangle(np.diag(np.asarray(case.sigma) ** 2)), (9, 1)))
    got, state = _run(case, cutoff=cutoff, cov=diag)
    fixed, fixed_state = case.table.clone(), torch.zeros(8, dtype=F64)
    assert mc.host_deposit(fixed, case.lower, case.spacing, case.periodic, case.sigma, None, case.y, case.V, cutoff=cutoff, state=fixed_state) == 0
    _assert_close(case, got, fixed.numpy(), mc.host_heights(case.V), "fixed sigma")
    assert torch.equal(state, fixed_state)
    if cutoff is not None:
        margin = oracle.cutoff_margin(shape, case.lower, case.spacing, case.periodic, None, case.y.numpy(), diag.numpy(), cutoff)
        assert margin >= 1e-9 and torch.equal(got != case.table, fixed != case.table)
    # one matrix for every walker: cov_stride 0
    shared, _ = _run(case, cutoff=cutoff, cov=diag[:1].expand(9, d * (d + 1) // 2))
    assert torch.equal(shared, got)


def test_columns_out_of_order_on_a_wider_y_and_strided_V_and_cov():
    case = cc.CovCase((5, 7), (True, False), 65, n_out=5, columns=(3, 1), v_stride=3, v_offset=2, cov_width=7, cov_offset=2)
    assert case.V.stride(0) == 3 and case.cov.stride(0) == 7 and case.cov.data_ptr() == case.cov_store.data_ptr() + 16
    y0, v0, c0 = case.y.clone(), case.v_store.clone(), case.cov_store.clone()
    got, state = _run(case)
    _assert_close(case, got, _oracle(case)[0], mc.host_heights(case.V.contiguous()))
    assert torch.equal(case.y, y0) and torch.equal(case.v_store, v0) and torch.equal(case.cov_store, c0)
    plain = cc.CovCase((5, 7), (True, False), 65)
    plain.y, plain.V, plain.cov = case.y[:, [3, 1]].contiguous(), case.V.contiguous(), case.cov.contiguous()
    again, state2 = _run(plain)
    assert torch.equal(got, again) and torch.equal(state, state2)


@pytest.mark.parametrize("shape,periodic,w1,w2,cutoff", [((67,), (True,), 3, 9, None), ((5, 7), (True, False), 64, 65, CUTOFF),
                                                         ((4, 5, 6), (False, True, False), 1, 66, None), ((17, 33), (True, False), 7, 60, CUTOFF)])
def test_two_deposits_give_the_bits_of_one(shape, periodic, w1, w2, cutoff):
    case = cc.CovCase(shape, periodic, w1 + w2, start="random")
    whole, whole_state = _run(case, cutoff=cutoff)
    table, state = case.table.clone(), torch.zeros(8, dtype=F64)
    for rows in (slice(0, w1), slice(w1, w1 + w2)):
        assert cc.host_deposit_cov(table, case.lower, case.spacing, case.periodic, None, case.y[rows].contiguous(), case.V[rows].contiguous(),
                                   case.cov[rows].contiguous(), cutoff=cutoff, state=state) == 0
    assert torch.equal(table, whole)
    assert torch.equal(state[:3], whole_state[:3]) and state[3:].tolist() == [2.0, 0.0, 0.0, 0.0, 0.0]


def test_a_log_shorter_than_the_step():
    case = cc.CovCase((5, 7), (False, True), 5)
    log = torch.full((3, 6), -7.0, dtype=F64)
    state = torch.tensor([10.0, 2.0, 0.5, 7.0, 1.0, 0.0, 0.0, 0.0], dtype=F64)
    _run(case, state=state, log=log)
    heights = mc.host_heights(case.V)
    assert state[:2].tolist() == [15.0, 2.0] and state[3:].tolist() == [8.0, 3.0, 0.0, 0.0, 0.0]
    assert log[0].tolist() == [-7.0] * 6
    for row, a in ((1, 0), (2, 1)):
        assert log[row].tolist() == case.y[a].tolist() + case.cov[a].tolist() + [float(heights[a])]


BAD = ["nan_y", "nan_V", "overflow", "nan_cov", "inf_cov", "singular", "negative", "zero", "indefinite"]


def _spoil(case, a, bad):
    d, T = case.d, case.T
    if bad == "nan_y":
        case.y[a, d - 1] = NAN
    elif bad in ("nan_V", "overflow"):
        case.V[a] = NAN if bad == "nan_V" else -1e5
    elif bad == "nan_cov":
        case.cov[a, T - 1 if d == 1 else 1] = NAN
    elif bad == "inf_cov":
        case.cov[a, 0] = INF
    elif bad == "singular":                      # all ones: rank one (d = 1: replaced by 0, no width at all)
        case.cov[a] = torch.ones(T, dtype=F64) if d > 1 else torch.zeros(1, dtype=F64)
    elif bad == "negative":
        case.cov[a, T - 1] = -float(case.cov[a, T - 1])
    elif bad == "zero":
        case.cov[a] = 0.0
    elif bad == "indefinite":                    # an off-diagonal entry past sqrt(C_ii C_jj) (d = 1: a negative variance)
        if d == 1:
            case.cov[a, 0] = -1.0
        else:
            case.cov[a, 1] = 1.5 * math.sqrt(float(case.cov[a, 0]) * float(oracle.full(case.cov[a].numpy(), d)[1, 1]))


@pytest.mark.parametrize("bad", BAD)
@pytest.mark.parametrize("shape,periodic", [((67,), (True,)), ((5, 7), (True, False)), ((4, 5, 6), (False, True, False))])
def test_an_invalid_walker_changes_no_entry_and_is_refused(shape, periodic, bad):
    case = cc.CovCase(shape, periodic, 4, start="random")
    good, _ = _run(case)
    a = 2
    _spoil(case, a, bad)
    alone = cc.CovCase(shape, periodic, 1, start="random")
    alone.table, alone.y, alone.V, alone.cov = case.table.clone(), case.y[a:a + 1].contiguous(), case.V[a:a + 1].contiguous(), case.cov[a:a + 1].contiguous()
    log = torch.zeros(2, alone.d + alone.T + 1, dtype=F64)
    got, state = _run(alone, log=log)
    assert np.array_equal(got.numpy().view(np.int64), case.table.numpy().view(np.int64))
    assert state.tolist() == [0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0] and not log.any()
    got4, state4 = _run(case)
    rest = cc.CovCase(shape, periodic, 3, start="random")
    rest.table, rest.y, rest.V, rest.cov = case.table.clone(), case.y[[0, 1, 3]].contiguous(), case.V[[0, 1, 3]].contiguous(), case.cov[[0, 1, 3]].contiguous()
    got3, state3 = _run(rest)
    assert torch.equal(got4, got3) and state4.tolist() == [3.0, 1.0, float(state3[2]), 1.0, 0.0, 0.0, 0.0, 0.0]
    assert not torch.equal(got4, good)
    want, want_state, _ = _oracle(case)
    assert want_state[:2].tolist() == [3.0, 1.0]
    _assert_close(case, got4, want, mc.host_heights(rest.V))


# ---------------------------------------------------------------------------------------------- the widths call
GRIDS = [((67,), (True,)), ((5, 7), (True, False)), ((5, 7), (False, False)), ((4, 5, 6), (False, True, False))]


def _walk(rng, case, steps):
    """A random walk of the case's walkers over `steps` observations, a few spacings per step with a drift, so that on a periodic axis
    the running mean crosses the boundary: [steps, W, d]."""
    d = case.d
    span = np.asarray(case.spacing)
    start = case.y.numpy()[:, :d]
    moves = rng.normal(size=(steps, case.walkers, d)) * 0.8 * span + 0.9 * span
    return start[None] + np.cumsum(moves, axis=0)


@pytest.mark.parametrize("shape,periodic", GRIDS)
def test_fifty_observations_against_the_oracle(shape, periodic):
    case = cc.CovCase(shape, periodic, 9)
    d, T, W, window = case.d, case.T, 9, 7
    rng = np.random.RandomState(5)
    ys = _walk(rng, case, 50)
    ys[17, 4, 0] = NAN                                                      # one observation of one walker is skipped
    adapt, adapt_state, cov = torch.zeros(W, 1 + d + T, dtype=F64), torch.zeros(8, dtype=F64), torch.full((W, T), -3.0, dtype=F64)
    want, want_state = np.zeros((W, 1 + d + T)), np.zeros(8)
    period = case.period()
    crossings = 0
    for i, y in enumerate(ys):
        emit = i % 5 == 4
        before = want[:, 1].copy()
        assert cc.host_widths(shape, case.lower, case.spacing, case.periodic, case.sigma, None, cc.DIFF, window, emit, adapt, adapt_state, cov,
                              y=torch.from_numpy(y.copy())) == 0
        want, want_state, want_cov = oracle.widths(cc.DIFF, d, case.lower, period, case.sigma, None, None, None, window, emit, want, want_state, y=y)
        if period[0] > 0 and i > 0:
            crossings += int((want[:, 1] < before - 0.5 * period[0]).sum())
        if emit:
            scale = np.abs(want_cov).max()
            assert float(np.abs(cov.numpy() - want_cov).max()) <= 1e-13 * scale, i
            if i < window - 1:
                assert np.array_equal(cov.numpy(), np.tile(oracle.triangle(np.diag(np.asarray(case.sigma) ** 2)), (W, 1)))
    assert adapt_state.tolist() == want_state.tolist() == [50.0 * W - 1, 10.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert np.array_equal(adapt[:, 0].numpy(), want[:, 0]) and float(adapt[4, 0]) == 49.0
    for lo, hi in ((1, 1 + d), (1 + d, 1 + d + T)):
        scale = np.abs(want[:, lo:hi]).max()
        err = float(np.abs(adapt[:, lo:hi].numpy() - want[:, lo:hi]).max())
        print("shape %s columns %d..%d: error %.3g of scale %.3g" % (shape, lo, hi, err, scale))
        assert err <= 1e-13 * scale
    if period[0] > 0:
        assert crossings >= 3, "the mean was meant to cross the periodic boundary"
        assert (adapt[:, 1].numpy() >= case.lower[0]).all() and (adapt[:, 1].numpy() < case.lower[0] + period[0]).all()


def test_observing_without_emitting_leaves_cov_and_a_bad_row_keeps_its_bits():
    case = cc.CovCase((5, 7), (True, False), 3)
    adapt = torch.from_numpy(np.random.RandomState(1).uniform(0.5, 1.5, size=(3, 6)))
    adapt[:, 0] = torch.tensor([4.0, 0.0, 9.0], dtype=F64)
    before = adapt.clone()
    state, cov = torch.zeros(8, dtype=F64), torch.full((3, 3), -3.0, dtype=F64)
    y = case.y.clone()
    y[2, 1] = INF
    assert cc.host_widths(case.shape, case.lower, case.spacing, case.periodic, case.sigma, None, cc.DIFF, 5, False, adapt, state, cov, y=y) == 0
    assert (cov == -3.0).all() and state.tolist() == [2.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    assert torch.equal(adapt[2], before[2]) and adapt[0, 0] == 5.0
    assert adapt[1].tolist() == [1.0] + y[1].tolist() + [0.0] * 3


@pytest.mark.parametrize("d", [1, 2, 3])
def test_limits_clamp_the_diagonal_exactly_and_keep_the_correlations(d):
    shape, periodic = {1: ((67,), (True,)), 2: ((5, 7), (True, False)), 3: ((4, 5, 6), (False, True, False))}[d]
    case = cc.CovCase(shape, periodic, 64)
    T, W = case.T, 64
    n_out = d + 1
    rng = np.random.RandomState(3)
    J = rng.normal(size=(W, n_out, 5))
    metric = torch.from_numpy(np.einsum("wik,wjk->wij", J, J))
    columns = list(range(n_out))[::-1][:d]
    sigma = [0.4 + 0.1 * k for k in range(d)]
    plain = torch.zeros(W, T, dtype=F64)
    state = torch.zeros(8, dtype=F64)
    assert cc.host_widths(shape, case.lower, case.spacing, case.periodic, sigma, columns, cc.GEOM, 1, True, None, state, plain, metric=metric) == 0
    _, _, want = oracle.widths(cc.GEOM, d, case.lower, case.period(), sigma, None, None, columns, 1, True, None, np.zeros(8), metric=metric.numpy())
    assert float(np.abs(plain.numpy() - want).max()) <= 1e-14 * np.abs(want).max()
    assert state.tolist() == [0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    diag = np.array([[oracle.full(plain[a].numpy(), d)[k, k] for k in range(d)] for a in range(W)])
    lo = [float(np.sqrt(np.percentile(diag[:, k], 30))) for k in range(d)]
    hi = [float(np.sqrt(np.percentile(diag[:, k], 70))) for k in range(d)]
    clamped = torch.zeros(W, T, dtype=F64)
    assert cc.host_widths(shape, case.lower, case.spacing, case.periodic, sigma, columns, cc.GEOM, 1, True, None, state, clamped, metric=metric,
                          sigma_min=lo, sigma_max=hi) == 0
    moved = 0
    for a in range(W):
        C0, C1 = oracle.full(plain[a].numpy(), d), oracle.full(clamped[a].numpy(), d)
        want_C = oracle.limits(C0, lo, hi)
        assert float(np.abs(C1 - want_C).max()) <= 1e-14 * np.abs(want_C).max()
        for k in range(d):
            target = min(max(C0[k, k], lo[k] * lo[k]), hi[k] * hi[k])
            assert C1[k, k] == target                                      # exact
            moved += target != C0[k, k]
        s0, s1 = np.sqrt(np.diag(C0)), np.sqrt(np.diag(C1))
        assert float(np.abs(C0 / np.outer(s0, s0) - C1 / np.outer(s1, s1)).max()) <= 1e-15
        assert oracle.usable(C1)
    assert moved >= W * d // 2
    # a diagonal entry that is not > 0 cannot be scaled: its row and column are cleared
    zero = metric.clone()
    zero[0] = 0.0
    assert cc.host_widths(shape, case.lower, case.spacing, case.periodic, sigma, columns, cc.GEOM, 1, True, None, state, clamped, metric=zero,
                          sigma_min=lo, sigma_max=hi) == 0
    assert np.array_equal(oracle.full(clamped[0].numpy(), d), np.diag(np.asarray(lo) ** 2))


# ---------------------------------------------------------------------------------------------- refusals
def _arr(t, v):
    return None if v is None else (t * len(v))(*v)


def _ptr(v):
    return v.data_ptr() if isinstance(v, torch.Tensor) else v


def _deposit_call(**change):
    case = cc.CovCase((5, 7), (True, False), 3, n_out=3)
    a = dict(table=case.table.clone(), d=2, shape=[5, 7], lower=case.lower, spacing=case.spacing, periodic=[1, 0], columns=[2, 0], y=case.y.data_ptr(),
             y_stride=3, V=case.V.data_ptr(), v_stride=1, cov=case.cov.data_ptr(), cov_stride=3, n=3, height0=1.2, inv_dT=0.04, cutoff=INF,
             state=torch.zeros(8, dtype=F64), log=None, log_capacity=0)
    a.update(change)
    code = cc._capi.lib().molann_selftest_metad_deposit_cov_f64(
        _ptr(a["table"]), a["d"], _arr(ctypes.c_int64, a["shape"]), _arr(ctypes.c_double, a["lower"]), _arr(ctypes.c_double, a["spacing"]),
        _arr(ctypes.c_int32, a["periodic"]), _arr(ctypes.c_int32, a["columns"]), a["y"], a["y_stride"], a["V"], a["v_stride"], a["cov"], a["cov_stride"],
        a["n"], a["height0"], a["inv_dT"], a["cutoff"], _ptr(a["state"]), _ptr(a["log"]), a["log_capacity"])
    return code, a["table"], a["state"], case


DEPOSIT_REFUSALS = [
    (E_NULL, dict(table=None)), (E_NULL, dict(state=None)), (E_NULL, dict(y=None)), (E_NULL, dict(V=None)), (E_NULL, dict(cov=None)),
    (E_NULL, dict(shape=None)), (E_NULL, dict(lower=None)), (E_NULL, dict(spacing=None)),
    (E_ALIGNMENT, dict(table=4)), (E_ALIGNMENT, dict(state=12)), (E_ALIGNMENT, dict(y=4)), (E_ALIGNMENT, dict(V=2)), (E_ALIGNMENT, dict(cov=4)),
    (E_ALIGNMENT, dict(log=4)),
    (E_UNSUPPORTED, dict(d=0)), (E_UNSUPPORTED, dict(d=4)),
    (E_DESC, dict(shape=[3, 7])), (E_DESC, dict(spacing=[0.0, 0.5])), (E_DESC, dict(lower=[0.0, NAN])), (E_DESC, dict(shape=[1 << 16, 1 << 15])),
    (E_DESC, dict(height0=0.0)), (E_DESC, dict(height0=NAN)), (E_DESC, dict(inv_dT=-0.1)), (E_DESC, dict(inv_dT=INF)),
    (E_DESC, dict(cutoff=NAN)), (E_DESC, dict(cutoff=0.0)),
    (E_DESC, dict(y_stride=-3)), (E_DESC, dict(v_stride=-1)), (E_DESC, dict(n=-1)), (E_DESC, dict(log_capacity=-1)),
    (E_DESC, dict(cov_stride=2)), (E_DESC, dict(cov_stride=-3)), (E_DESC, dict(y_stride=2)), (E_DESC, dict(columns=[0, 3])), (E_DESC, dict(columns=[-1, 0])),
]


@pytest.mark.parametrize("code,change", DEPOSIT_REFUSALS, ids=lambda v: "_".join("%s" % k for k in v) if isinstance(v, dict) else str(v))
def test_deposit_refusals_write_nothing(code, change):
    got, table, state, _ = _deposit_call(**change)
    assert got == code, (got, code, change)
    for t in (table, state):
        assert not isinstance(t, torch.Tensor) or not t.any()


def test_deposit_refusals_come_in_their_order_and_no_walkers_is_ok():
    assert _deposit_call()[0] == 0
    assert _deposit_call(table=None, state=12, d=9, height0=NAN)[0] == E_NULL
    assert _deposit_call(state=12, d=9, height0=NAN)[0] == E_ALIGNMENT
    assert _deposit_call(d=9, height0=NAN, shape=[3, 7])[0] == E_UNSUPPORTED
    assert _deposit_call(shape=[3, 7], n=-1)[0] == E_DESC
    assert _deposit_call(n=0, table=None, y=None, V=None, cov=None, state=None, shape=None, lower=None, spacing=None)[0] == 0
    code, table, state, _ = _deposit_call(n=0)
    assert code == 0 and not table.any() and not state.any()
    assert _deposit_call(n=0, state=12)[0] == E_ALIGNMENT and _deposit_call(n=0, d=4)[0] == E_UNSUPPORTED and _deposit_call(n=0, cutoff=NAN)[0] == E_DESC
    assert _deposit_call(n=0, cov_stride=1)[0] == E_DESC
    assert _deposit_call(log=None, log_capacity=5)[0] == 0 and _deposit_call(cov_stride=0)[0] == 0 and _deposit_call(periodic=None)[0] == 0


def _widths_call(**change):
    case = cc.CovCase((5, 7), (True, False), 3, n_out=3)
    metric = torch.eye(3, dtype=F64).repeat(3, 1, 1)
    a = dict(d=2, shape=[5, 7], lower=case.lower, spacing=case.spacing, periodic=[1, 0], sigma=case.sigma, sigma_min=None, sigma_max=None, columns=[2, 0],
             y=case.y.data_ptr(), y_stride=3, metric=metric.data_ptr(), metric_stride=9, metric_ld=3, n=3, mode=cc.DIFF, window=5, emit=1,
             adapt=torch.zeros(3, 6, dtype=F64), adapt_state=torch.zeros(8, dtype=F64), cov=torch.zeros(3, 3, dtype=F64), cov_stride=3)
    a.update(change)
    code = cc._capi.lib().molann_selftest_metad_widths_f64(
        a["d"], _arr(ctypes.c_int64, a["shape"]), _arr(ctypes.c_double, a["lower"]), _arr(ctypes.c_double, a["spacing"]), _arr(ctypes.c_int32, a["periodic"]),
        _arr(ctypes.c_double, a["sigma"]), _arr(ctypes.c_double, a["sigma_min"]), _arr(ctypes.c_double, a["sigma_max"]), _arr(ctypes.c_int32, a["columns"]),
        a["y"], a["y_stride"], a["metric"], a["metric_stride"], a["metric_ld"], a["n"], a["mode"], a["window"], a["emit"], _ptr(a["adapt"]),
        _ptr(a["adapt_state"]), _ptr(a["cov"]), a["cov_stride"])
    return code, a["adapt"], a["adapt_state"], a["cov"], (case, metric)


WIDTHS_REFUSALS = [
    (E_NULL, dict(adapt_state=None)), (E_NULL, dict(shape=None)), (E_NULL, dict(lower=None)), (E_NULL, dict(spacing=None)), (E_NULL, dict(sigma=None)),
    (E_NULL, dict(y=None)), (E_NULL, dict(adapt=None)), (E_NULL, dict(mode=cc.GEOM, metric=None)), (E_NULL, dict(cov=None)),
    (E_ALIGNMENT, dict(adapt=4)), (E_ALIGNMENT, dict(adapt_state=12)), (E_ALIGNMENT, dict(cov=4)), (E_ALIGNMENT, dict(y=2)), (E_ALIGNMENT, dict(metric=4)),
    (E_UNSUPPORTED, dict(d=0)), (E_UNSUPPORTED, dict(d=4)),
    (E_DESC, dict(mode=0)), (E_DESC, dict(mode=3)), (E_DESC, dict(shape=[3, 7])), (E_DESC, dict(spacing=[NAN, 0.5])),
    (E_DESC, dict(sigma=[0.3, 0.0])), (E_DESC, dict(sigma=[NAN, 0.3])), (E_DESC, dict(sigma_min=[-0.1, 0.1])), (E_DESC, dict(sigma_min=[NAN, 0.1])),
    (E_DESC, dict(sigma_min=[INF, 0.1])), (E_DESC, dict(sigma_min=[0.2, 0.2], sigma_max=[0.1, 0.3])), (E_DESC, dict(sigma_max=[NAN, 0.3])),
    (E_DESC, dict(window=0)), (E_DESC, dict(window=-4)), (E_DESC, dict(y_stride=-3)), (E_DESC, dict(n=-1)), (E_DESC, dict(cov_stride=2)),
    (E_DESC, dict(y_stride=2)), (E_DESC, dict(columns=[0, 3])), (E_DESC, dict(columns=[-1, 0])),
    (E_DESC, dict(mode=cc.GEOM, metric_ld=2)), (E_DESC, dict(mode=cc.GEOM, metric_stride=8)), (E_DESC, dict(mode=cc.GEOM, metric_stride=-9)),
]


@pytest.mark.parametrize("code,change", WIDTHS_REFUSALS, ids=lambda v: "_".join("%s" % k for k in v) if isinstance(v, dict) else str(v))
def test_widths_refusals_write_nothing(code, change):
    got, adapt, state, cov, _ = _widths_call(**change)
    assert got == code, (got, code, change)
    for t in (adapt, state, cov):
        assert not isinstance(t, torch.Tensor) or not t.any()


def test_widths_refusals_come_in_their_order_and_no_walkers_is_ok():
    assert _widths_call()[0] == 0 and _widths_call(mode=cc.GEOM, y=None, adapt=None, window=0)[0] == 0
    assert _widths_call(adapt_state=None, cov=4, d=9, window=0)[0] == E_NULL
    assert _widths_call(cov=4, d=9, window=0)[0] == E_ALIGNMENT
    assert _widths_call(d=9, window=0)[0] == E_UNSUPPORTED
    assert _widths_call(window=0)[0] == E_DESC
    assert _widths_call(n=0, adapt_state=None, shape=None, lower=None, spacing=None, sigma=None, y=None, adapt=None, cov=None)[0] == 0
    code, adapt, state, cov, _ = _widths_call(n=0)
    assert code == 0 and not adapt.any() and not state.any() and not cov.any()
    assert _widths_call(n=0, cov=4)[0] == E_ALIGNMENT and _widths_call(n=0, d=4)[0] == E_UNSUPPORTED and _widths_call(n=0, mode=7)[0] == E_DESC
    code, adapt, state, cov, _ = _widths_call(emit=0, cov=None, cov_stride=0)            # observing needs no cov_out
    assert code == 0 and state.tolist()[:3] == [3.0, 0.0, 0.0]
    assert _widths_call(mode=cc.GEOM, metric_stride=0)[0] == 0 and _widths_call(periodic=None, columns=None)[0] == 0


# ---------------------------------------------------------------------------------------------- bias: MetadRun, CovHills, add_cov_hills_to_grid
class _Model(object):
    def value_and_grid(self, *a, **k):
        raise AssertionError("not called")

    value_and_bias = value_and_grid


def test_metadrun_checks_the_adaptive_arguments_without_a_device():
    assert "CovHills" in mbias.__all__ and "add_cov_hills_to_grid" in mbias.__all__
    good = dict(model=_Model(), table=torch.zeros(5, 7, dtype=F64), lower=[0.0, 0.0], spacing=[0.1, 0.1], kT=2.5, biasfactor=10.0, height=1.2,
                sigma=[0.2, 0.2], adaptive="diff", window=5, walkers=4)

    def fails(error, match=None, **change):
        with pytest.raises(error, match=match):
            mbias.MetadRun(**dict(good, **change))

    fails(ValueError, match="device")                                    # a CPU table: everything else passed
    fails(ValueError, match="device", adaptive="geom", window=None)
    fails(ValueError, match="device", sigma_min=[0.1, 0.0], sigma_max=[0.1, INF])
    fails(ValueError, match="device", adaptive=None, window=None, walkers=None)
    fails(ValueError, match="adaptive", adaptive="DIFF")
    fails(ValueError, match="adaptive", adaptive=True)
    fails(ValueError, match="window", window=None)
    fails(ValueError, match="window", window=0)
    fails(TypeError, match="window", window=2.0)
    fails(TypeError, match="window", window=True)
    fails(ValueError, match="window", adaptive="geom")
    fails(ValueError, match="walkers", walkers=None)
    fails(ValueError, match="walkers", walkers=0)
    fails(TypeError, match="walkers", walkers="4")
    fails(ValueError, match="sigma_min", sigma_min=[0.1])
    fails(ValueError, match="sigma_min", sigma_min=[-0.1, 0.1])
    fails(ValueError, match="sigma_min", sigma_min=[INF, 0.1])
    fails(TypeError, match="sigma_min", sigma_min=0.1)
    fails(ValueError, match="sigma_max", sigma_max=[NAN, 0.1])
    fails(ValueError, match="sigma_max", sigma_min=[0.2, 0.2], sigma_max=[0.3, 0.1])
    for name, value in (("window", 5), ("walkers", 4), ("sigma_min", [0.1, 0.1]), ("sigma_max", [0.1, 0.1])):
        fails(ValueError, match=name, **dict(dict(adaptive=None, window=None, walkers=None), **{name: value}))


def test_cov_hills_gives_the_log_back_and_add_cov_hills_to_grid_rebuilds_the_table():
    case = cc.CovCase((5, 7), (True, False), 6)
    log = torch.zeros(4, 6, dtype=F64)
    got, state = _run(case, log=log)
    run = mbias.MetadRun.__new__(mbias.MetadRun)      # a CPU table is refused by the constructor: the record is formed from the fields alone
    run.table, run.log, run.state, run.spacing, run.periodic, run.columns, run.adaptive = got, log, state, case.spacing, list(case.periodic), None, "diff"
    record = run.cov_hills()
    assert isinstance(record, mbias.CovHills) and record.centers.shape == (4, 2) and record.covariances.shape == (4, 3) and record.columns is None
    assert torch.equal(record.centers, case.y[:4]) and torch.equal(record.covariances, case.cov[:4]) and record.period.tolist() == [5 * case.spacing[0], 0.0]
    assert torch.equal(record.heights, mc.host_heights(case.V)[:4]) and run.cov_hills(2).centers.shape == (2, 2)
    with pytest.raises(ValueError, match="cov_hills"):
        run.hills()
    with pytest.raises(ValueError):
        run.cov_hills(5)
    run.adaptive = None
    with pytest.raises(ValueError, match="hills"):
        run.cov_hills()
    for shape, periodic, cutoff in (((5, 7), (True, False), None), ((67,), (True,), CUTOFF), ((4, 5, 6), (False, True, False), None),
                                    ((17, 33), (True, False), CUTOFF)):
        c = cc.CovCase(shape, periodic, 9)
        heights = mc.host_heights(c.V)
        rebuilt = mbias.add_cov_hills_to_grid(torch.zeros(shape, dtype=F64), c.lower, c.spacing, c.periodic, c.y, c.cov, heights, cutoff=cutoff, chunk=4)
        if cutoff is not None:
            assert oracle.cutoff_margin(shape, c.lower, c.spacing, c.periodic, None, c.y.numpy(), c.cov.numpy(), cutoff) >= 1e-9
        _assert_close(c, _run(c, cutoff=cutoff)[0], rebuilt.numpy(), heights, "add_cov_hills_to_grid")
    with pytest.raises(ValueError):
        mbias.add_cov_hills_to_grid(torch.zeros(5, 7, dtype=F64), case.lower, case.spacing, None, case.y, case.cov[:, :2], 1.0)
    with pytest.raises(TypeError):
        mbias.add_cov_hills_to_grid(torch.zeros(5, 7), case.lower, case.spacing, None, case.y, case.cov, 1.0)
