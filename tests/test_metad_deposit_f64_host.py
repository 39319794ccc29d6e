"""The metadynamics deposit on the host (no GPU): `molann_selftest_metad_deposit_f64` - metad_deposit_f64_kernel's tiles, reach test and
per-entry sums through the functions the kernel calls, compiled for the host - against tests/metad_oracle.py, a plain numpy loop
written from include/molann_hip.h, and against `bias.add_hills_to_grid`; then the ordering, the state, the log, the refusals and
`bias.MetadRun`'s constructor.  Cases and the bound (1e-12 of the summed heights plus the table's largest entry): tests/metad_cases.py."""

import ctypes
import math

import numpy as np
import pytest
import torch

from molann_amd import bias as mbias

import metad_cases as mc
import metad_oracle as oracle

F64, INF, NAN = mc.F64, mc.INF, mc.NAN
E_NULL, E_DESC, E_ALIGNMENT, E_UNSUPPORTED = -1, -2, -6, -7
CUTOFF = 3.3            # in widths; sigma is 0.83 (1 + 0.27 k) spacings, so no grid point is meant to sit on the edge: asserted per case


def _run(case, cutoff=None, table=None, state=None, log=None, height0=mc.HEIGHT0, inv_dT=mc.INV_DT):
    table = case.table.clone() if table is None else table
    state = torch.zeros(8, dtype=F64) if state is None else state
    code = mc.host_deposit(table, case.lower, case.spacing, case.periodic, case.sigma, case.columns, case.y, case.V, height0, inv_dT, cutoff,
                           state, log)
    assert code == 0, code
    return table, state


def _oracle(case, cutoff=None, state=None, log=None, height0=mc.HEIGHT0, inv_dT=mc.INV_DT):
    return oracle.deposit(case.table.numpy(), case.lower, case.spacing, case.periodic, case.sigma, case.columns, case.y.numpy(), case.V.numpy(),
                          height0, inv_dT, cutoff, np.zeros(8) if state is None else state, log)


def _assert_close(case, got, want, heights, what=""):
    tol = mc.tolerance(heights, case.table)
    err = float(np.abs(got.numpy() - want).max())
    print("%s shape %s W %d: error %.3g, bound %.3g" % (what, case.shape, case.walkers, err, tol))
    assert err <= tol, (err, tol)


# ---------------------------------------------------------------------------------------------- the twin against the oracle
@pytest.mark.parametrize("walkers", mc.WALKERS)
@pytest.mark.parametrize("shape,periodic", mc.SHAPES)
def test_twin_matches_the_oracle_and_add_hills_to_grid(shape, periodic, walkers):
    case = mc.Case(shape, periodic, walkers)
    got, state = _run(case)
    heights = mc.host_heights(case.V)
    want, want_state, _ = _oracle(case)
    _assert_close(case, got, want, heights, "oracle")
    torch_table = mbias.add_hills_to_grid(torch.zeros(shape, dtype=F64), case.lower, case.spacing, case.periodic, case.y, heights, case.sigma)
    _assert_close(case, got, torch_table.numpy(), heights, "add_hills_to_grid")
    assert state[:2].tolist() == [walkers, 0.0] and state[3:].tolist() == [1.0, 0.0, 0.0, 0.0, 0.0]
    assert abs(float(state[2]) - want_state[2]) <= 1e-12 * want_state[2]
    assert abs(float(state[2]) - float(heights.sum())) <= 1e-12 * float(heights.sum())


def test_a_table_that_holds_values_already():
    case = mc.Case((5, 7), (True, False), 65, start="random")
    got, _ = _run(case)
    _assert_close(case, got, _oracle(case)[0], mc.host_heights(case.V))


def test_plain_metadynamics_takes_height0():
    case = mc.Case((67,), (True,), 3)
    log = torch.zeros(3, 3, dtype=F64)
    got, state = _run(case, inv_dT=0.0, log=log)
    assert log[:, 2].tolist() == [mc.HEIGHT0] * 3 and float(state[2]) == 3 * mc.HEIGHT0
    _assert_close(case, got, _oracle(case, inv_dT=0.0)[0], log[:, 2])


# ---------------------------------------------------------------------------------------------- placement and addressing
def test_a_hill_outside_a_non_periodic_range_lands_on_the_points_it_reaches():
    case = mc.Case((67,), (False,), 1)
    case.y[0, 0] = case.lower[0] - 1.5 * case.sigma[0]                    # below point 0 by a width and a half
    got, _ = _run(case)
    _assert_close(case, got, _oracle(case)[0], mc.host_heights(case.V))
    assert float(got[0]) > 0.3 * float(mc.host_heights(case.V)[0]) * math.exp(-0.5 * 1.5 ** 2) and float(got[0]) > float(got[1]) > float(got[2])
    cut, _ = _run(case, cutoff=2.0)
    assert float(cut[0]) == float(got[0]) and int((cut != 0).sum()) == int((oracle.entry_q(case.shape, case.lower, case.spacing, case.periodic,
                                                                                            case.sigma, case.y[0].numpy()) <= 4.0).sum())


@pytest.mark.parametrize("shape,periodic,axis", [((67,), (True,), 0), ((5, 7), (True, True), 1), ((4, 5, 6), (False, True, False), 1)])
def test_a_hill_on_a_periodic_seam(shape, periodic, axis):
    case = mc.Case(shape, periodic, 3)
    seam = case.lower[axis] + (shape[axis] - 0.5) * case.spacing[axis]   # half way between the last point and the first again
    case.y[:, axis] = torch.tensor([seam, case.lower[axis], case.lower[axis] + shape[axis] * case.spacing[axis]], dtype=F64)
    got, _ = _run(case)
    _assert_close(case, got, _oracle(case)[0], mc.host_heights(case.V))
    one = mc.Case(shape, periodic, 1)
    one.y[0, axis] = seam
    alone, _ = _run(one)
    first, last = alone.select(axis, 0), alone.select(axis, shape[axis] - 1)
    assert float((first - last).abs().max()) <= mc.tolerance(mc.host_heights(one.V), one.table)      # the seam's two sides get the same
    cut, _ = _run(case, cutoff=CUTOFF)
    want, _, _ = _oracle(case, cutoff=CUTOFF)
    _assert_close(case, cut, want, mc.host_heights(case.V), "cutoff")
    assert np.array_equal(cut.numpy() == 0, want == 0)


def test_columns_out_of_order_on_a_wider_y_and_a_strided_V():
    case = mc.Case((5, 7), (True, False), 65, n_out=5, columns=(3, 1), v_stride=3, v_offset=2)
    assert case.V.stride(0) == 3 and case.V.data_ptr() == case.v_store.data_ptr() + 16
    y0, v0 = case.y.clone(), case.v_store.clone()
    got, state = _run(case)
    heights = mc.host_heights(case.V.contiguous())
    _assert_close(case, got, _oracle(case)[0], heights)
    assert torch.equal(case.y, y0) and torch.equal(case.v_store, v0)
    # the same walkers laid out plainly give the same bits
    plain = mc.Case((5, 7), (True, False), 65)
    plain.y, plain.V = case.y[:, [3, 1]].contiguous(), case.V.contiguous()
    again, state2 = _run(plain)
    assert torch.equal(got, again) and torch.equal(state, state2)
    three = mc.Case((4, 5, 6), (False, True, False), 3, n_out=5, columns=(4, 0, 2))
    _assert_close(three, _run(three)[0], _oracle(three)[0], mc.host_heights(three.V))


# ---------------------------------------------------------------------------------------------- the cutoff
@pytest.mark.parametrize("walkers", mc.WALKERS)
@pytest.mark.parametrize("shape,periodic", mc.SHAPES + mc.TILE_SHAPES[:1] + mc.TILE_SHAPES[2:3] + mc.TILE_SHAPES[4:5])
def test_cutoff_keeps_the_bits_outside_and_matches_inside(shape, periodic, walkers):
    case = mc.Case(shape, periodic, walkers, start="random")
    margin = oracle.cutoff_margin(shape, case.lower, case.spacing, case.periodic, case.sigma, None, case.y.numpy(), CUTOFF)
    print("nearest grid point to the cutoff's edge: %.3g (relative, in q)" % margin)
    assert margin >= 1e-9, margin
    got, _ = _run(case, cutoff=CUTOFF)
    want, _, _ = _oracle(case, cutoff=CUTOFF)
    _assert_close(case, got, want, mc.host_heights(case.V))
    outside = np.ones(shape, dtype=bool)
    for centre in case.y.numpy():
        outside &= oracle.entry_q(shape, case.lower, case.spacing, case.periodic, case.sigma, centre) > CUTOFF ** 2
    before = case.table.numpy()
    assert np.array_equal(got.numpy()[outside].view(np.int64), before[outside].view(np.int64))
    assert np.array_equal(got.numpy() != before, ~outside)        # and every entry inside took at least h exp(-c^2 / 2)


def test_a_negative_zero_outside_the_cutoff_stays_negative_zero():
    case = mc.Case((67,), (False,), 1)
    case.table.fill_(-0.0)
    got, _ = _run(case, cutoff=2.0)
    far = oracle.entry_q(case.shape, case.lower, case.spacing, case.periodic, case.sigma, case.y[0].numpy()) > 4.0
    assert far.any() and np.signbit(got.numpy()[far]).all() and (got.numpy()[~far] > 0).all()


# ---------------------------------------------------------------------------------------------- ordering, state, log
@pytest.mark.parametrize("shape,periodic,w1,w2,cutoff", [((67,), (True,), 3, 5, None), ((5, 7), (True, False), 64, 65, CUTOFF),
                                                         ((4, 5, 6), (False, True, False), 1, 66, None), ((17, 33), (True, False), 7, 60, CUTOFF)])
def test_two_deposits_give_the_bits_of_one(shape, periodic, w1, w2, cutoff):
    case = mc.Case(shape, periodic, w1 + w2, start="random")
    whole, whole_state = _run(case, cutoff=cutoff)
    table, state = case.table.clone(), torch.zeros(8, dtype=F64)
    for rows in (slice(0, w1), slice(w1, w1 + w2)):
        assert mc.host_deposit(table, case.lower, case.spacing, case.periodic, case.sigma, None, case.y[rows].contiguous(),
                               case.V[rows].contiguous(), cutoff=cutoff, state=state) == 0
    assert torch.equal(table, whole)
    assert torch.equal(state[:3], whole_state[:3]) and state[3:].tolist() == [2.0, 0.0, 0.0, 0.0, 0.0]


def test_state_and_log_follow_the_walkers():
    case = mc.Case((5, 7), (False, True), 5)
    case.V[1], case.y[3, 0] = NAN, INF
    state = torch.tensor([10.0, 2.0, 0.5, 7.0, 1.0, 0.0, 0.0, 0.0], dtype=F64)
    log = torch.full((3, 5), -7.0, dtype=F64)
    got, state = _run(case, state=state, log=log)
    heights = mc.host_heights(case.V[[0, 2, 4]].contiguous())
    assert state[:2].tolist() == [13.0, 4.0] and state[3:].tolist() == [8.0, 3.0, 0.0, 0.0, 0.0]
    assert float(state[2]) == ((0.5 + float(heights[0])) + float(heights[1])) + float(heights[2])
    assert log[0].tolist() == [-7.0] * 5                                     # rows before state[4] are the caller's
    for row, a in ((1, 0), (2, 2)):                                          # the third valid walker finds the log full: deposited all the same
        assert log[row].tolist() == case.y[a].tolist() + case.sigma + [float(heights[row - 1])]
    want, want_state, want_log = _oracle(case, state=state.numpy() * 0 + [10.0, 2.0, 0.5, 7.0, 1.0, 0, 0, 0], log=np.full((3, 5), -7.0))
    assert np.array_equal(want_state[[0, 1, 3, 4]], state.numpy()[[0, 1, 3, 4]]) and np.allclose(want_log, log.numpy(), rtol=1e-14, atol=0)
    _assert_close(case, got, want, heights)
    # a state whose logged count is not a row of the log writes no row
    for bad in (NAN, -3.0, 1e300, INF):
        state2, log2 = torch.tensor([0.0, 0.0, 0.0, 0.0, bad, 0.0, 0.0, 0.0], dtype=F64), torch.full((3, 5), -7.0, dtype=F64)
        _run(case, state=state2, log=log2)
        rows = 3 if bad in (NAN, -3.0) else 0
        assert float(state2[4]) == 3.0 and int((log2[:, 0] != -7.0).sum()) == rows


def test_hills_gives_the_log_back_as_a_record():
    case = mc.Case((5, 7), (True, False), 6)
    log = torch.zeros(4, 5, dtype=F64)
    got, state = _run(case, log=log)
    run = mbias.MetadRun.__new__(mbias.MetadRun)      # a CPU table is refused by the constructor: the record is formed from the fields alone
    run.table, run.log, run.state, run.spacing, run.periodic, run.columns = got, log, state, case.spacing, list(case.periodic), None
    assert run.read_state() == dict(hills=6, refused=0, sum_heights=float(state[2]), steps=1, logged=4)
    record = run.hills()
    assert isinstance(record, mbias.Hills) and record.centers.shape == (4, 2) and record.columns is None
    assert torch.equal(record.centers, case.y[:4]) and record.sigma[2].tolist() == case.sigma and record.period.tolist() == [5 * case.spacing[0], 0.0]
    assert torch.equal(record.heights, mc.host_heights(case.V)[:4])
    assert run.hills(2).centers.shape == (2, 2)
    rebuilt = mbias.add_hills_to_grid(torch.zeros(5, 7, dtype=F64), case.lower, case.spacing, case.periodic, record.centers, record.heights, record.sigma)
    four = mc.Case((5, 7), (True, False), 6)
    four.y, four.V = case.y[:4].contiguous(), case.V[:4].contiguous()
    _assert_close(four, _run(four)[0], rebuilt.numpy(), record.heights)
    with pytest.raises(ValueError):
        run.hills(5)
    run.log = None
    with pytest.raises(ValueError):
        run.hills()


@pytest.mark.parametrize("bad", ["nan_y", "inf_y", "nan_V", "overflow", "underflow"])
@pytest.mark.parametrize("shape,periodic", [((67,), (True,)), ((5, 7), (True, False)), ((4, 5, 6), (False, True, False))])
def test_an_invalid_walker_changes_no_entry_and_is_refused(shape, periodic, bad):
    case = mc.Case(shape, periodic, 4, start="random")
    good, good_state = _run(case)
    a = 2
    if bad in ("nan_y", "inf_y"):
        case.y[a, len(shape) - 1] = NAN if bad == "nan_y" else -INF
    else:
        case.V[a] = {"nan_V": NAN, "overflow": -1e5, "underflow": 1e5}[bad]      # exp(+-1e5 / 22.4) is inf, 0
    alone = mc.Case(shape, periodic, 1, start="random")
    alone.table, alone.y, alone.V = case.table.clone(), case.y[a:a + 1].contiguous(), case.V[a:a + 1].contiguous()
    log = torch.zeros(2, 2 * len(shape) + 1, dtype=F64)
    got, state = _run(alone, log=log)
    assert np.array_equal(got.numpy().view(np.int64), case.table.numpy().view(np.int64))
    assert state.tolist() == [0.0, 1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0] and not log.any()
    # among others it changes nothing of theirs: the three valid walkers alone give the same bits
    got4, state4 = _run(case)
    rest = mc.Case(shape, periodic, 3, start="random")
    rest.table, rest.y, rest.V = case.table.clone(), case.y[[0, 1, 3]].contiguous(), case.V[[0, 1, 3]].contiguous()
    got3, state3 = _run(rest)
    assert torch.equal(got4, got3) and state4.tolist() == [3.0, 1.0, float(state3[2]), 1.0, 0.0, 0.0, 0.0, 0.0]
    assert not torch.equal(got4, good)


# ---------------------------------------------------------------------------------------------- refusals
def _call(**change):
    """The twin with one good set of arguments, some replaced; returns (code, table, state)."""
    case = mc.Case((5, 7), (True, False), 3, n_out=3)
    a = dict(table=case.table.clone(), d=2, shape=[5, 7], lower=case.lower, spacing=case.spacing, periodic=[1, 0], sigma=case.sigma, columns=[2, 0],
             y=case.y.data_ptr(), y_stride=3, V=case.V.data_ptr(), v_stride=1, n=3, height0=1.2, inv_dT=0.04, cutoff=INF,
             state=torch.zeros(8, dtype=F64), log=None, log_capacity=0)
    a.update(change)
    arr = lambda t, v: None if v is None else (t * len(v))(*v)  # noqa: E731
    ptr = lambda v: v.data_ptr() if isinstance(v, torch.Tensor) else v  # noqa: E731
    code = mc._capi.lib().molann_selftest_metad_deposit_f64(
        ptr(a["table"]), a["d"], arr(ctypes.c_int64, a["shape"]), arr(ctypes.c_double, a["lower"]), arr(ctypes.c_double, a["spacing"]),
        arr(ctypes.c_int32, a["periodic"]), arr(ctypes.c_double, a["sigma"]), arr(ctypes.c_int32, a["columns"]), a["y"], a["y_stride"], a["V"],
        a["v_stride"], a["n"], a["height0"], a["inv_dT"], a["cutoff"], ptr(a["state"]), ptr(a["log"]), a["log_capacity"])
    return code, a["table"], a["state"], (case.y, case.V)


REFUSALS = [
    (E_NULL, dict(table=None)), (E_NULL, dict(state=None)), (E_NULL, dict(y=None)), (E_NULL, dict(V=None)), (E_NULL, dict(shape=None)),
    (E_NULL, dict(lower=None)), (E_NULL, dict(spacing=None)), (E_NULL, dict(sigma=None)),
    (E_ALIGNMENT, dict(table=4)), (E_ALIGNMENT, dict(state=12)), (E_ALIGNMENT, dict(y=4)), (E_ALIGNMENT, dict(V=2)), (E_ALIGNMENT, dict(log=4)),
    (E_UNSUPPORTED, dict(d=0)), (E_UNSUPPORTED, dict(d=4)),
    (E_DESC, dict(shape=[3, 7])), (E_DESC, dict(spacing=[0.0, 0.5])), (E_DESC, dict(spacing=[0.3, INF])), (E_DESC, dict(spacing=[NAN, 0.5])),
    (E_DESC, dict(lower=[0.0, NAN])), (E_DESC, dict(lower=[-INF, 0.0])), (E_DESC, dict(shape=[1 << 16, 1 << 15])),
    (E_DESC, dict(sigma=[0.3, 0.0])), (E_DESC, dict(sigma=[NAN, 0.3])), (E_DESC, dict(sigma=[0.3, INF])), (E_DESC, dict(sigma=[-0.3, 0.3])),
    (E_DESC, dict(height0=0.0)), (E_DESC, dict(height0=-1.0)), (E_DESC, dict(height0=INF)), (E_DESC, dict(height0=NAN)),
    (E_DESC, dict(inv_dT=-0.1)), (E_DESC, dict(inv_dT=INF)), (E_DESC, dict(inv_dT=NAN)),
    (E_DESC, dict(cutoff=NAN)), (E_DESC, dict(cutoff=0.0)), (E_DESC, dict(cutoff=-2.0)),
    (E_DESC, dict(y_stride=-3)), (E_DESC, dict(v_stride=-1)), (E_DESC, dict(n=-1)), (E_DESC, dict(log_capacity=-1)),
    (E_DESC, dict(y_stride=2)), (E_DESC, dict(columns=[0, 3])), (E_DESC, dict(columns=[-1, 0])),
]


@pytest.mark.parametrize("code,change", REFUSALS, ids=lambda v: "_".join("%s" % k for k in v) if isinstance(v, dict) else str(v))
def test_refusals_write_nothing(code, change):
    got, table, state, _ = _call(**change)
    assert got == code, (got, code, change)
    for t in (table, state):
        assert not isinstance(t, torch.Tensor) or not t.any()


def test_refusals_come_in_their_order_and_no_walkers_is_ok():
    assert _call()[0] == 0
    assert _call(table=None, state=12, d=9, height0=NAN)[0] == E_NULL
    assert _call(state=12, d=9, height0=NAN)[0] == E_ALIGNMENT
    assert _call(d=9, height0=NAN, shape=[3, 7])[0] == E_UNSUPPORTED
    assert _call(shape=[3, 7], n=-1)[0] == E_DESC
    # no walkers: nothing is read, OK - but a malformed description is still refused, in the same order
    code, table, state, _ = _call(n=0, table=None, y=None, V=None, state=None, shape=None, lower=None, spacing=None, sigma=None)
    assert code == 0
    code, table, state, _ = _call(n=0)
    assert code == 0 and not table.any() and not state.any()
    assert _call(n=0, state=12)[0] == E_ALIGNMENT and _call(n=0, d=4)[0] == E_UNSUPPORTED and _call(n=0, cutoff=NAN)[0] == E_DESC
    assert _call(n=-1, table=None)[0] == E_DESC
    assert _call(log=None, log_capacity=5)[0] == 0          # no log: the capacity is not used
    assert _call(v_stride=0)[0] == 0 and _call(periodic=None, columns=None)[0] == 0


# ---------------------------------------------------------------------------------------------- bias.MetadRun
class _Model(object):
    def value_and_grid(self, *a, **k):
        raise AssertionError("not called")

    value_and_bias = value_and_grid


def test_metadrun_is_public_and_checks_its_arguments_once():
    assert "MetadRun" in mbias.__all__
    good = dict(model=_Model(), table=torch.zeros(5, 7, dtype=F64), lower=[0.0, 0.0], spacing=[0.1, 0.1], kT=2.5, biasfactor=10.0, height=1.2,
                sigma=[0.2, 0.2])

    def fails(error, **change):
        with pytest.raises(error):
            mbias.MetadRun(**dict(good, **change))

    fails(ValueError)                                                   # a CPU table: the kernels are HIP kernels
    fails(TypeError, model=object())
    fails(TypeError, table=[[0.0] * 7] * 5)
    fails(TypeError, table=torch.zeros(5, 7))
    fails(ValueError, table=torch.zeros(4, 4, 4, 4, dtype=F64))
    fails(ValueError, table=torch.zeros((), dtype=F64))
    if torch.cuda.is_available():
        good["table"] = torch.zeros(5, 7, dtype=F64, device="cuda")
        mbias.MetadRun(**good)
    # the device is checked last, so every other check is reached without one
    fails(ValueError, table=good["table"][:3])
    fails(ValueError, table=torch.zeros(7, 10, dtype=F64, device=good["table"].device)[:, ::2])
    fails(TypeError, kT="2.5")
    fails(TypeError, kT=True)
    fails(ValueError, kT=0.0)
    fails(ValueError, kT=INF)
    fails(ValueError, biasfactor=1.0)
    fails(ValueError, biasfactor=NAN)
    fails(TypeError, biasfactor=None)
    fails(ValueError, height=0.0)
    fails(ValueError, height=INF)
    fails(TypeError, height=torch.tensor(1.0))
    fails(ValueError, cutoff=0.0)
    fails(ValueError, cutoff=NAN)
    fails(TypeError, cutoff="6")
    fails(ValueError, sigma=[0.2])
    fails(ValueError, sigma=[0.2, 0.0])
    fails(ValueError, sigma=[0.2, NAN])
    fails(TypeError, sigma=0.2)
    fails(ValueError, spacing=[0.1, -0.1])
    fails(ValueError, lower=[0.0, INF])
    fails(ValueError, lower=[0.0])
    fails(ValueError, periodic=[True])
    fails(TypeError, columns=3)
    fails(IndexError, columns=[0, 0])
    fails(IndexError, columns=[-1, 0])
    fails(ValueError, columns=[0])
    fails(TypeError, walls=(1, 2))
    fails(TypeError, log_capacity=2.0)
    fails(TypeError, log_capacity=True)
    fails(ValueError, log_capacity=-1)
