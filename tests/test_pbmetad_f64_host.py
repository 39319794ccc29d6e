"""Parallel-bias metadynamics on the host (no GPU): `molann_selftest_pbmetad_f64` and `molann_selftest_pbmetad_deposit_f64` - the frame
kernel's term and the deposit kernel's tiles, reach test and per-entry sums through the functions the kernels call, compiled for the
host - against tests/pbmetad_oracle.py, a plain numpy / torch loop written from the formulas of include/molann_hip.h, against torch
autograd of the formula and against the existing 1-D deposit twin; then the ordering, the state, the log, the refusals and the
constructors of `bias.PBTables` and `bias.PBMetadRun`.  Cases and bounds: tests/pbmetad_cases.py."""

import ctypes
import math

import numpy as np
import pytest
import torch

from molann_amd import _capi
from molann_amd import bias as mbias

import metad_cases as mc
import pbmetad_cases as pc
import pbmetad_oracle as oracle

F64, INF, NAN, KT = pc.F64, pc.INF, pc.NAN, pc.KT
E_NULL, E_DESC, E_INDEX, E_ALIGNMENT, E_UNSUPPORTED = -1, -2, -3, -6, -7
CUTOFF = 3.3            # in widths; sigma is 0.83 (1 + 0.27 k) spacings, so no grid point is meant to sit on the edge: asserted


# ============================================================================================== the frame twin
def _grid_from(values, n, periodic, below=2, above=2):
    """A grid of n points built from the y values themselves: not periodic, `below` of the sorted values lie under the range and `above`
    over it; periodic, the range covers the middle half, so values wrap from both sides."""
    v = np.sort(np.asarray(values))
    if periodic:
        lo, hi = v[len(v) // 4], v[3 * len(v) // 4]
        return float(lo), float((hi - lo) / n)
    lo, hi = 0.5 * (v[below - 1] + v[below]), 0.5 * (v[-above - 1] + v[-above])
    return float(lo), float((hi - lo) / (n - 1))


def _frame_case(K, d_out, columns, seed, n_frames=24):
    rng = np.random.RandomState(seed)
    y = rng.uniform(-2.0, 2.0, size=(n_frames, d_out))
    cols = list(range(K)) if columns is None else list(columns)
    shape = [(5, 9, 4, 33, 6, 17, 12, 7)[k] for k in range(K)]
    periodic = [k % 2 == 1 for k in range(K)]
    lower, spacing = [], []
    for k in range(K):
        lo, h = _grid_from(y[:, cols[k]], shape[k], periodic[k])
        lower.append(lo)
        spacing.append(h)
    # frames in the first and the last cell of every non-periodic axis and in the seam cell of every periodic one
    for k in range(K):
        n = shape[k]
        if periodic[k]:
            y[0, cols[k]] = lower[k] + (n - 0.4) * spacing[k]
            y[1, cols[k]] = lower[k] + (2 * n - 0.7) * spacing[k]            # a period further: it wraps into the seam cell
        else:
            y[0, cols[k]] = lower[k] + 0.3 * spacing[k]
            y[1, cols[k]] = lower[k] + (n - 1.3) * spacing[k]
    table = torch.from_numpy(rng.uniform(-3.0, 5.0, size=sum(shape)))
    return torch.from_numpy(y), mbias.PBTables(table, shape, lower, spacing, periodic, columns), cols


def _assert_cells_hit(y, tables, cols):
    for k, n in enumerate(tables.shape):
        per = tables.periodic[k]
        cells = [oracle.axis_cell(float(v), n, tables.lower[k], tables.spacing[k], per) for v in y[:, cols[k]]]
        u = (y[:, cols[k]].numpy() - tables.lower[k]) / tables.spacing[k]
        if per:
            assert n - 1 in [c for c, _ in cells], "no frame in the seam cell of axis %d" % k
            assert (u < 0).any() and (u > n).any(), "no frame wraps on axis %d" % k
        else:
            assert (u < 0).any() and (u > n - 1).any(), "no frame below / above axis %d" % k
            inside = [c for c, ok in cells if ok]
            assert 0 in inside and n - 2 in inside and len(inside) >= 3, "first / last cell of axis %d not hit" % k
            assert np.abs(u).min() > 1e-9 and np.abs(u - (n - 1)).min() > 1e-9, "a y within 1e-9 spacing of an end of axis %d" % k


@pytest.mark.parametrize("K,d_out,columns", [(1, 1, None), (2, 2, None), (3, 8, (5, 0, 2)), (8, 8, None), (8, 10, (9, 3, 0, 7, 1, 4, 8, 2))])
@pytest.mark.parametrize("walls", [False, True])
def test_frame_twin_matches_the_oracle_and_autograd(K, d_out, columns, walls):
    y, tables, cols = _frame_case(K, d_out, columns, seed=100 + K + d_out)
    _assert_cells_hit(y, tables, cols)
    restraint = None
    if walls:
        restraint = (torch.linspace(-0.5, 0.5, d_out, dtype=F64), torch.linspace(0.0, 3.0, d_out, dtype=F64), None,
                     torch.full((d_out,), 0.25, dtype=F64))
    yt = y.clone().requires_grad_(True)
    vpb_t, V_t = oracle.torch_bias(yt, tables.table, tables.shape, tables.lower, tables.spacing, tables.periodic, columns, KT)
    dy_t, = torch.autograd.grad(vpb_t.sum(), yt)
    vpb_t, V_t = vpb_t.detach(), V_t.detach()
    worst = [0.0, 0.0]
    for f in range(y.shape[0]):
        code, e, dy = pc.host_frame(y[f].contiguous(), tables, KT, restraint)
        assert code == 0
        want_e, want_dy = oracle.frame(y[f].tolist(), tables.table.numpy(), tables.shape, tables.lower, tables.spacing, tables.periodic, columns, KT,
                                       None if restraint is None else [None if r is None else r.tolist() for r in restraint])
        scale_e = max(1.0, float(np.abs(want_e).max()))
        scale_d = max(1e-3, float(np.abs(want_dy).max()))
        err_e, err_d = float(np.abs(e.numpy() - want_e).max()), float(np.abs(dy.numpy() - want_dy).max())
        worst = [max(worst[0], err_e / (1e-10 * scale_e)), max(worst[1], err_d / (1e-9 * scale_d))]
        assert err_e <= 1e-10 * scale_e and err_d <= 1e-9 * scale_d, (f, err_e, err_d)
        assert abs(float(e[1]) - float(vpb_t[f])) <= 1e-10 * scale_e and float((e[2:] - V_t[f]).abs().max()) <= 1e-10 * scale_e
        if restraint is None:
            assert float(e[0]) == 0.0
            assert float((dy - dy_t[f]).abs().max()) <= 1e-9 * scale_d
    print("K %d d_out %d walls %s: worst error / bound: energies %.3g, dy %.3g" % (K, d_out, walls, worst[0], worst[1]))


def test_one_axis_gives_the_tables_own_bits():
    y, tables, cols = _frame_case(1, 3, (2,), seed=7)
    for f in range(y.shape[0]):
        code, e, dy = pc.host_frame(y[f].contiguous(), tables, KT)
        idx, w, dw = (ctypes.c_int64 * 4)(), (ctypes.c_double * 4)(), (ctypes.c_double * 4)()
        _capi.lib().molann_selftest_grid_axis_f64(float(y[f, 2]), tables.shape[0], tables.lower[0], tables.spacing[0], 0, idx, w, dw)
        T = tables.table.tolist()
        V0 = ((T[idx[0]] * w[0] + T[idx[1]] * w[1]) + T[idx[2]] * w[2]) + T[idx[3]] * w[3]
        dV0 = ((T[idx[0]] * dw[0] + T[idx[1]] * dw[1]) + T[idx[2]] * dw[2]) + T[idx[3]] * dw[3]
        assert code == 0 and float(e[1]) == float(e[2]) == V0            # V_PB has the bits of V_0
        assert dy.tolist() == [0.0, 0.0, dV0]                           # the cotangent the bits of V_0'


def test_two_equal_tables_share_the_bias_in_halves():
    rng = np.random.RandomState(3)
    one = rng.uniform(-2.0, 2.0, size=9)
    tables = mbias.PBTables(torch.from_numpy(np.concatenate([one, one])), (9, 9), (-1.0, -1.0), (0.25, 0.25))
    for v in (-0.7, 0.13, 0.9):
        code, e, dy = pc.host_frame(torch.tensor([v, v], dtype=F64), tables, KT)
        assert code == 0 and float(e[2]) == float(e[3])
        assert abs(float(e[1]) - (float(e[2]) - KT * math.log(2.0))) <= 1e-10 * max(1.0, abs(float(e[2])))
        _, alone, dy1 = pc.host_frame(torch.tensor([v], dtype=F64), mbias.PBTables(torch.from_numpy(one.copy()), (9,), (-1.0,), (0.25,)), KT)
        assert dy.tolist() == [0.5 * float(dy1[0])] * 2                  # w = 1/2 exactly


def test_an_axis_far_above_the_minimum_has_no_share():
    table = torch.cat([torch.full((6,), 1.5, dtype=F64), torch.full((5,), 1.5 + 800.0 * KT, dtype=F64) + torch.arange(5, dtype=F64)])
    tables = mbias.PBTables(table, (6, 5), (0.0, 0.0), (1.0, 1.0))
    code, e, dy = pc.host_frame(torch.tensor([2.5, 1.5], dtype=F64), tables, KT)
    assert code == 0 and math.isfinite(float(e[1])) and float(e[1]) == 1.5
    assert float(dy[1]) == 0.0 and float(e[3]) > 800.0 * KT             # w_1 = exp(-800) is exactly 0, and so is its cotangent column


@pytest.mark.parametrize("bad", [NAN, INF, -INF])
def test_a_value_that_is_not_finite_poisons_its_own_frame(bad):
    y, tables, cols = _frame_case(3, 8, (5, 0, 2), seed=11)
    good = pc.host_frame(y[3].contiguous(), tables, KT)
    row = y[3].clone()
    row[1] = bad                                                         # an unchosen column: nothing changes
    code, e, dy = pc.host_frame(row, tables, KT)
    assert code == 0 and torch.equal(e, good[1]) and torch.equal(dy, good[2])
    row = y[3].clone()
    row[0] = bad                                                         # a chosen one
    code, e, dy = pc.host_frame(row, tables, KT)
    assert code == 0 and math.isnan(float(e[1])) and all(math.isnan(float(dy[c])) for c in cols)
    assert float(e[0]) == 0.0 and dy[[1, 3, 4, 6, 7]].tolist() == [0.0] * 5
    # a table entry that is not finite does the same through V_k
    t2 = tables._replace(table=tables.table.clone())
    t2.table[:] = torch.where(torch.arange(t2.table.numel()) < tables.shape[0], torch.full_like(t2.table, bad), t2.table)
    code, e, dy = pc.host_frame(y[3].contiguous(), t2, KT)
    assert code == 0 and math.isnan(float(e[1])) and all(math.isnan(float(dy[c])) for c in cols)


def test_frame_twin_refusals_in_order_write_nothing():
    y, tables, _ = _frame_case(3, 8, (5, 0, 2), seed=5)
    row = y[0].contiguous()

    def code(t, kT=KT):
        c, e, dy = pc.host_frame(row, t, kT)
        assert c == 0 or (e.tolist() == [7.0] * e.numel() and dy.tolist() == [7.0] * dy.numel())
        return c

    assert code(tables) == 0
    assert code(tables._replace(columns=(5, 0, 8))) == E_INDEX and code(tables._replace(columns=(5, 0, 5))) == E_INDEX
    assert code(tables._replace(shape=(5, 3, 4))) == E_DESC
    assert code(tables._replace(spacing=(0.1, 0.0, 0.1))) == E_DESC and code(tables._replace(lower=(0.0, NAN, 0.0))) == E_DESC
    assert code(tables, kT=0.0) == E_DESC and code(tables, kT=NAN) == E_DESC and code(tables, kT=INF) == E_DESC
    assert code(tables._replace(shape=(2 ** 30, 2 ** 30, 4))) == E_DESC
    # the order: a bad column is seen before a bad grid, a bad grid before a bad kT, a bad kT before the size
    assert code(tables._replace(columns=(5, 0, 8), shape=(5, 3, 4))) == E_INDEX
    assert code(tables._replace(shape=(5, 3, 4)), kT=0.0) == E_DESC
    wide = torch.zeros(36, dtype=F64)
    terms, keep = _capi.pbmetad_terms_f64(((None, 9), wide, (4,) * 9, (0.0,) * 9, (1.0,) * 9, None, KT))
    e, dy = torch.full((11,), 7.0, dtype=F64), torch.full((9,), 7.0, dtype=F64)
    y9 = torch.zeros(9, dtype=F64)
    assert _capi.lib().molann_selftest_pbmetad_f64(y9.data_ptr(), 9, terms, e.data_ptr(), dy.data_ptr()) == E_UNSUPPORTED
    terms.n_columns = 0
    assert _capi.lib().molann_selftest_pbmetad_f64(y9.data_ptr(), 9, terms, e.data_ptr(), dy.data_ptr()) == E_DESC
    assert _capi.lib().molann_selftest_pbmetad_f64(None, 9, terms, e.data_ptr(), dy.data_ptr()) == E_NULL
    assert e.tolist() == [7.0] * 11 and dy.tolist() == [7.0] * 9


# ============================================================================================== the deposit twin
def _oracle(case, cutoff=None, state=None, log=None, height0=pc.HEIGHT0, inv_dT=pc.INV_DT, kT=KT, table=None):
    return oracle.deposit((case.table if table is None else table).numpy(), case.shape, case.lower, case.spacing, case.periodic, case.sigma,
                          case.columns, case.y.numpy(), case.V.numpy(), height0, inv_dT, kT, cutoff, np.zeros(8) if state is None else state, log)


def _assert_tables_close(case, got, want, heights, what="", before=None):
    before = case.table if before is None else before
    worst = 0.0
    for k in range(case.K):
        tol = pc.tolerance(heights[:, k], case.axis(before, k))
        err = float(np.abs(case.axis(got, k).numpy() - case.axis(torch.from_numpy(want), k).numpy()).max())
        worst = max(worst, err / tol)
        assert err <= tol, (k, err, tol)
    print("%s shape %s W %d: worst error / bound %.3g" % (what, case.shape, case.walkers, worst))


@pytest.mark.parametrize("walkers", pc.WALKERS)
def test_deposit_twin_matches_the_oracle_on_eight_axes(walkers):
    case = pc.Case(pc.SHAPE8, pc.PERIODIC8, walkers)
    got, state = pc.run_case(case)
    heights = pc.host_heights(case.V.contiguous())
    want, want_state, _ = _oracle(case)
    _assert_tables_close(case, got, want, heights, "oracle")
    assert state[:2].tolist() == [walkers, 0.0] and state[3:].tolist() == [1.0, 0.0, 0.0, 0.0, 0.0]
    assert abs(float(state[2]) - want_state[2]) <= 1e-12 * want_state[2]
    cut, _ = pc.run_case(case, cutoff=CUTOFF)
    want_cut, _, _ = _oracle(case, cutoff=CUTOFF)
    _assert_tables_close(case, cut, want_cut, heights, "cutoff")
    assert np.array_equal(cut.numpy() != 0, want_cut != 0)


@pytest.mark.parametrize("walkers", (1, 9, 65))
@pytest.mark.parametrize("shape,periodic", pc.SMALL)
def test_deposit_twin_matches_the_oracle_on_few_axes(shape, periodic, walkers):
    case = pc.Case(shape, periodic, walkers, start="random")
    got, _ = pc.run_case(case)
    _assert_tables_close(case, got, _oracle(case)[0], pc.host_heights(case.V.contiguous()))


def test_columns_out_of_order_on_a_wider_y_and_energies_in_place():
    case = pc.Case((5, 300, 67), (True, False, True), 65, n_out=10, columns=(7, 0, 4), v_pad=3)
    assert case.V.stride(0) == 8 and case.V.data_ptr() == case.e_store.data_ptr() + 16
    y0, e0 = case.y.clone(), case.e_store.clone()
    got, state = pc.run_case(case)
    _assert_tables_close(case, got, _oracle(case)[0], pc.host_heights(case.V.contiguous()))
    assert torch.equal(case.y, y0) and torch.equal(case.e_store, e0)
    plain = pc.Case((5, 300, 67), (True, False, True), 65)
    plain.y, plain.V = case.y[:, [7, 0, 4]].contiguous(), case.V.contiguous()
    again, state2 = pc.run_case(plain)
    assert torch.equal(got, again) and torch.equal(state, state2)


def test_a_hill_outside_a_range_and_one_on_a_seam():
    case = pc.Case((67, 67), (False, True), 3)
    case.y[0, 0] = case.lower[0] - 1.5 * case.sigma[0]                    # below point 0 by a width and a half
    case.y[1, 1] = case.lower[1] + (67 - 0.5) * case.spacing[1]          # half way between the last point and the first again
    got, _ = pc.run_case(case)
    _assert_tables_close(case, got, _oracle(case)[0], pc.host_heights(case.V.contiguous()))
    one = pc.Case((67, 67), (False, True), 1)
    one.y[0, 0], one.y[0, 1] = case.y[0, 0], case.y[1, 1]
    alone, _ = pc.run_case(one)
    h = pc.host_heights(one.V.contiguous())
    t0, t1 = one.axis(alone, 0), one.axis(alone, 1)
    assert float(t0[0]) > float(t0[1]) > float(t0[2]) > 0.0
    assert abs(float(t1[0]) - float(t1[66])) <= pc.tolerance(h[:, 1], one.axis(one.table, 1))     # the seam's two sides get the same


def test_cutoff_changes_exactly_the_oracles_entries_and_keeps_the_others_bits():
    case = pc.Case(pc.SHAPE8, pc.PERIODIC8, 9, start="random")
    case.table[::7] = -0.0
    got, _ = pc.run_case(case, cutoff=CUTOFF)
    inside = np.zeros(case.table.numel(), dtype=bool)
    for a in range(case.walkers):
        for k in range(case.K):
            q = oracle.axis_q(case.shape[k], case.lower[k], case.spacing[k], case.periodic[k], case.sigma[k], float(case.y[a, k]))
            assert np.abs(q - CUTOFF ** 2).min() > 1e-9, "a grid point on the cutoff's edge"
            inside[case.offsets[k]:case.offsets[k + 1]] |= q <= CUTOFF ** 2
    bits = lambda t: t.numpy().view(np.int64)  # noqa: E731
    changed = bits(got) != bits(case.table)
    assert np.array_equal(changed, inside)                               # every term is > 0, so an entry inside changes
    assert inside.any() and not inside.all()
    kept = ~inside & (np.arange(inside.size) % 7 == 0)
    assert kept.any() and np.all(np.signbit(got.numpy()[kept])) and np.all(got.numpy()[kept] == 0.0)       # a -0.0 stays -0.0
    _assert_tables_close(case, got, _oracle(case, cutoff=CUTOFF)[0], pc.host_heights(case.V.contiguous()), "cutoff")


@pytest.mark.parametrize("periodic,cutoff", [(False, None), (True, None), (True, CUTOFF)])
@pytest.mark.parametrize("walkers", (1, 9, 65))
def test_one_axis_gives_the_bits_of_the_metadynamics_twin(periodic, cutoff, walkers):
    case = pc.Case((300,), (periodic,), walkers, start="random")
    log = torch.zeros(walkers, 2, dtype=F64)
    got, state = pc.run_case(case, cutoff=cutoff, log=log)
    table, st, log1 = case.table.clone(), torch.zeros(8, dtype=F64), torch.zeros(walkers, 3, dtype=F64)
    assert mc.host_deposit(table, case.lower, case.spacing, case.periodic, case.sigma, None, case.y, case.V[:, 0], pc.HEIGHT0, pc.INV_DT, cutoff,
                           st, log1) == 0
    assert torch.equal(got, table) and torch.equal(state[:5], st[:5]) and torch.equal(log[:, 1], log1[:, 2]) and torch.equal(log[:, 0], log1[:, 0])


@pytest.mark.parametrize("cutoff", [None, CUTOFF])
def test_two_queued_deposits_give_the_bits_of_one(cutoff):
    case = pc.Case((5, 300, 67), (True, False, True), 65, start="random")
    whole, state = pc.run_case(case, cutoff=cutoff)
    table, st = case.table.clone(), torch.zeros(8, dtype=F64)
    for rows in (slice(0, 23), slice(23, 65)):
        assert pc.host_deposit(table, case.shape, case.lower, case.spacing, case.periodic, case.sigma, None, case.y[rows], case.V[rows],
                               cutoff=cutoff, state=st) == 0
    assert torch.equal(table, whole) and torch.equal(st[:3], state[:3]) and st[3] == 2.0


def test_a_height_that_underflows_leaves_its_axis_and_counts_the_walker():
    case = pc.Case((67, 67), (False, True), 1, start="random")
    case.V[0, 0], case.V[0, 1] = 0.0, 800.0 * KT                          # w_1 = exp(-800) = 0: h_1 is exactly 0
    log = torch.zeros(1, 4, dtype=F64)
    got, state = pc.run_case(case, log=log)
    assert torch.equal(case.axis(got, 1), case.axis(case.table, 1)) and not torch.equal(case.axis(got, 0), case.axis(case.table, 0))
    assert state[:2].tolist() == [1.0, 0.0] and float(log[0, 3]) == 0.0 and float(log[0, 2]) == pc.HEIGHT0 == float(state[2])


@pytest.mark.parametrize("kind", ["nan y", "inf y", "nan V", "overflow"])
def test_an_invalid_walker_changes_nothing_and_is_refused(kind):
    case = pc.Case((67, 300), (False, True), 9, n_out=4, columns=(3, 1), start="random")
    clean = pc.Case((67, 300), (False, True), 9, n_out=4, columns=(3, 1), start="random")
    keep = [a for a in range(9) if a != 4]
    clean.y, clean.e_store = case.y[keep].contiguous(), case.e_store[keep].contiguous()
    clean.V = clean.e_store[:, 2:4]
    if kind == "nan y":
        case.y[4, 1] = NAN
    elif kind == "inf y":
        case.y[4, 3] = -INF
    elif kind == "nan V":
        case.V[4, 1] = NAN
    else:
        case.V[4, 0] = -1e6                                               # height0 exp(1e6 / (9 kT)) overflows
    got, state = pc.run_case(case, cutoff=CUTOFF)
    want, want_state = pc.run_case(clean, cutoff=CUTOFF)
    assert torch.equal(got, want) and state[:3].tolist() == [8.0, 1.0, float(want_state[2])]
    case.y[4, 0] = NAN                                                    # an unchosen column is not looked at
    again, _ = pc.run_case(case, cutoff=CUTOFF)
    assert torch.equal(again, got)
    alone = pc.Case((67, 300), (False, True), 1, n_out=4, columns=(3, 1), start="random")
    alone.y, alone.e_store = case.y[4:5].contiguous(), case.e_store[4:5].contiguous()
    alone.V = alone.e_store[:, 2:4]
    got, state = pc.run_case(alone)
    assert torch.equal(got, alone.table) and state[:4].tolist() == [0.0, 1.0, 0.0, 1.0]


def test_state_and_log():
    case = pc.Case((67, 300, 5), (False, True, True), 9)
    heights = pc.host_heights(case.V.contiguous())
    log = torch.full((6, 6), 7.0, dtype=F64)
    state = torch.tensor([10.0, 2.0, 0.5, 4.0, 1.0, 9.0, 9.0, 9.0], dtype=F64)
    _, state = pc.run_case(case, state=state, log=log)
    total = 0.5
    for a in range(9):
        for k in range(3):
            total = total + float(heights[a, k])
    assert state.tolist() == [19.0, 2.0, total, 5.0, 6.0, 9.0, 9.0, 9.0]
    assert log[0].tolist() == [7.0] * 6                                   # rows start at `logged`
    assert torch.equal(log[1:, :3], case.y[:5]) and torch.equal(log[1:, 3:], heights[:5])        # the overflow: five rows fit, all nine deposit
    want_table, want_state, want_log = _oracle(case, state=np.array([10.0, 2.0, 0.5, 4.0, 1.0, 9.0, 9.0, 9.0]), log=np.full((6, 6), 7.0))
    assert want_state[:2].tolist() == [19.0, 2.0] and want_state[3:5].tolist() == [5.0, 6.0]
    assert np.abs(log.numpy() - want_log).max() <= 1e-12 * max(1.0, float(np.abs(want_log).max()))
    for logged, first in ((NAN, 0), (-3.0, 0), (1e300, 6), (INF, 6)):
        log = torch.full((6, 6), 7.0, dtype=F64)
        state = torch.tensor([0.0, 0.0, 0.0, 0.0, logged, 0.0, 0.0, 0.0], dtype=F64)
        pc.run_case(pc.Case((67, 300, 5), (False, True, True), 1), state=state, log=log)
        assert float(state[4]) == min(first + 1, 6) and int((log != 7.0).any(dim=1).sum()) == (1 if first < 6 else 0)


def test_the_logged_hills_rebuild_every_table():
    case = pc.Case((67, 300, 5), (False, True, True), 65, n_out=6, columns=(4, 1, 2))
    log = torch.zeros(65, 6, dtype=F64)
    got, state = pc.run_case(case, log=log)
    heights = pc.host_heights(case.V.contiguous())
    for k in range(3):
        rebuilt = mbias.add_hills_to_grid(torch.zeros(case.shape[k], dtype=F64), [case.lower[k]], [case.spacing[k]], [case.periodic[k]],
                                          log[:, k:k + 1], log[:, 3 + k], [case.sigma[k]])
        assert float((rebuilt - case.axis(got, k)).abs().max()) <= pc.tolerance(heights[:, k], case.axis(case.table, k))


def test_deposit_refusals_in_order_write_nothing():
    case = pc.Case((67, 300), (False, True), 3, n_out=4, columns=(3, 1), start="random")
    lib = _capi.lib()

    def call(table=case.table, shape=case.shape, lower=case.lower, spacing=case.spacing, sigma=case.sigma, columns=case.columns, y=case.y, V=case.V,
             walkers=3, height0=pc.HEIGHT0, inv_dT=pc.INV_DT, kT=KT, cutoff=INF, state=None, log=None, log_capacity=0, y_stride=4, v_stride=4,
             n_axes=None, offset=0):
        before = case.table.clone()
        state = torch.zeros(8, dtype=F64) if state is None else state
        a = pc.arrays(shape, lower, spacing, case.periodic[:len(shape)] if len(shape) <= 2 else None, sigma, columns)
        ptr = lambda t: None if t is None else t.data_ptr() + offset  # noqa: E731
        code = lib.molann_selftest_pbmetad_deposit_f64(ptr(table), len(shape) if n_axes is None else n_axes, a[0], a[1], a[2], a[3], a[4], a[5],
                                                       None if y is None else y.data_ptr(), y_stride, None if V is None else V.data_ptr(), v_stride,
                                                       walkers, height0, inv_dT, kT, cutoff, state.data_ptr(), None if log is None else log.data_ptr(),
                                                       log_capacity)
        assert torch.equal(case.table, before) and (code == 0 or state.tolist() == [0.0] * 8)
        return code

    assert call(table=None) == E_NULL and call(y=None) == E_NULL and call(V=None) == E_NULL
    assert call(offset=4) == E_ALIGNMENT
    assert call(n_axes=0) == E_UNSUPPORTED and call(n_axes=9) == E_UNSUPPORTED
    assert call(shape=(67, 3)) == E_DESC and call(spacing=(0.1, INF)) == E_DESC and call(lower=(NAN, 0.0)) == E_DESC
    assert call(shape=(2 ** 30, 2 ** 30)) == E_DESC
    assert call(sigma=(0.1, 0.0)) == E_DESC and call(sigma=(NAN, 0.1)) == E_DESC
    assert call(height0=0.0) == E_DESC and call(height0=INF) == E_DESC and call(inv_dT=-1.0) == E_DESC and call(inv_dT=NAN) == E_DESC
    assert call(kT=0.0) == E_DESC and call(kT=NAN) == E_DESC
    assert call(cutoff=0.0) == E_DESC and call(cutoff=NAN) == E_DESC
    assert call(y_stride=-1) == E_DESC and call(v_stride=1) == E_DESC and call(walkers=-1) == E_DESC and call(log_capacity=-1) == E_DESC
    assert call(columns=(4, 1)) == E_DESC and call(columns=(-1, 1)) == E_DESC and call(columns=(1, 1)) == E_INDEX
    # the order: alignment before the axes' count, the count before the grid, the grid before the scalars, the scalars before the columns
    assert call(offset=4, n_axes=9) == E_ALIGNMENT and call(n_axes=9, shape=(67, 3)) == E_UNSUPPORTED
    assert call(columns=(1, 1), kT=0.0) == E_DESC
    assert call(walkers=0, table=None, y=None, V=None) == 0               # nothing to do, nothing looked at


# ============================================================================================== the records
def test_pbtables_constructor_errors():
    t = torch.zeros(9, dtype=F64)
    ok = mbias.PBTables(t, (4, 5), (0.0, 0.0), (1.0, 1.0), (True, False), (3, 1))
    assert ok.shape == (4, 5) and ok.columns == (3, 1) and [v.numel() for v in ok.views()] == [4, 5] and ok.views()[1].data_ptr() == t.data_ptr() + 32
    with pytest.raises(TypeError, match="shape"):
        mbias.PBTables(t, 9, (0.0,), (1.0,))
    with pytest.raises(ValueError, match="1 to 8"):
        mbias.PBTables(t, (), (), ())
    with pytest.raises(NotImplementedError, match="1 to 8"):
        mbias.PBTables(torch.zeros(36, dtype=F64), (4,) * 9, (0.0,) * 9, (1.0,) * 9)
    with pytest.raises(ValueError, match="at least 4"):
        mbias.PBTables(t, (3, 6), (0.0, 0.0), (1.0, 1.0))
    with pytest.raises(TypeError, match="lower"):
        mbias.PBTables(t, (4, 5), 0.0, (1.0, 1.0))
    with pytest.raises(ValueError, match="one entry per table"):
        mbias.PBTables(t, (4, 5), (0.0,), (1.0, 1.0))
    with pytest.raises(ValueError, match="spacing"):
        mbias.PBTables(t, (4, 5), (0.0, 0.0), (1.0, 0.0))
    with pytest.raises(ValueError, match="periodic"):
        mbias.PBTables(t, (4, 5), (0.0, 0.0), (1.0, 1.0), (True,))
    with pytest.raises(ValueError, match="one output per table"):
        mbias.PBTables(t, (4, 5), (0.0, 0.0), (1.0, 1.0), None, (1,))
    with pytest.raises(IndexError):
        mbias.PBTables(t, (4, 5), (0.0, 0.0), (1.0, 1.0), None, (1, 1))
    with pytest.raises(TypeError, match="tensor"):
        mbias.PBTables([0.0] * 9, (4, 5), (0.0, 0.0), (1.0, 1.0))
    with pytest.raises(TypeError, match="float64"):
        mbias.PBTables(t.float(), (4, 5), (0.0, 0.0), (1.0, 1.0))
    with pytest.raises(ValueError, match="sum\\(shape\\)"):
        mbias.PBTables(torch.zeros(10, dtype=F64), (4, 5), (0.0, 0.0), (1.0, 1.0))


class _Model(torch.nn.Module):
    def value_and_pbmetad(self, *args, **kwargs):
        raise AssertionError("not called by the constructor")


def test_pbmetadrun_constructor_errors_come_before_the_device_check():
    args = dict(shape=(8, 9), lower=(0.0, 0.0), spacing=(0.5, 0.5), kT=KT, biasfactor=10.0, height=1.2, sigma=(0.3, 0.3))

    def make(**changes):
        kw = dict(args, **changes)
        return mbias.PBMetadRun(kw.pop("model", _Model()), **kw)

    with pytest.raises(TypeError, match="MolANN"):
        make(model=torch.nn.Linear(2, 2))
    with pytest.raises(TypeError, match="shape"):
        make(shape=8)
    with pytest.raises(ValueError, match="at least one axis"):
        make(shape=(), lower=(), spacing=(), sigma=())
    with pytest.raises(NotImplementedError, match="at most 8"):
        make(shape=(4,) * 9, lower=(0.0,) * 9, spacing=(1.0,) * 9, sigma=(1.0,) * 9)
    with pytest.raises(ValueError, match="at least 4"):
        make(shape=(8, 3))
    for what in ("kT", "biasfactor", "height"):
        with pytest.raises(TypeError, match=what):
            make(**{what: "1"})
        with pytest.raises(ValueError, match=what):
            make(**{what: 0.0})
    with pytest.raises(ValueError, match="biasfactor"):
        make(biasfactor=1.0)
    with pytest.raises(ValueError, match="cutoff"):
        make(cutoff=-1.0)
    for what in ("lower", "spacing", "sigma"):
        with pytest.raises(TypeError, match=what):
            make(**{what: 1.0})
        with pytest.raises(ValueError, match=what):
            make(**{what: (0.5,)})
        with pytest.raises(ValueError, match=what):
            make(**{what: (0.5, NAN)})
    with pytest.raises(ValueError, match="sigma"):
        make(sigma=(0.3, 0.0))
    with pytest.raises(ValueError, match="periodic"):
        make(periodic=(True,))
    with pytest.raises(TypeError, match="columns"):
        make(columns=3)
    with pytest.raises(IndexError):
        make(columns=(1, 1))
    with pytest.raises(ValueError, match="one output per axis"):
        make(columns=(1,))
    with pytest.raises(TypeError, match="walls"):
        make(walls=(0.0, 1.0))
    with pytest.raises(TypeError, match="log_capacity"):
        make(log_capacity=True)
    with pytest.raises(ValueError, match="log_capacity"):
        make(log_capacity=-1)
    with pytest.raises(TypeError, match="table"):
        make(table=[0.0] * 17)
    with pytest.raises(TypeError, match="float64"):
        make(table=torch.zeros(17))
    with pytest.raises(ValueError, match="sum\\(shape\\)"):
        make(table=torch.zeros(16, dtype=F64))
    with pytest.raises(ValueError, match="in place"):
        make(table=torch.zeros(34, dtype=F64)[::2])
    # everything else passed: only now the device
    with pytest.raises(ValueError, match="device"):
        make(table=torch.zeros(17, dtype=F64))
    with pytest.raises(ValueError, match="device"):
        make()


def test_the_new_symbols_are_declared_and_bound():
    names = _capi.declared_symbols()
    for name in ("molann_value_and_pbmetad_f64", "molann_plan_supports_value_and_pbmetad_f64", "molann_selftest_pbmetad_f64",
                 "molann_pbmetad_deposit_f64", "molann_selftest_pbmetad_deposit_f64"):
        assert name in names and getattr(_capi.lib(), name).argtypes is not None
    assert "PBMetadRun" in mbias.__all__ and "PBTables" in mbias.__all__
