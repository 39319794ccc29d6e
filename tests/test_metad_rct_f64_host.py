"""The reweighting offset c(t) of a metadynamics table on the host (no GPU): `molann_selftest_metad_rct_f64` - the chunks, the tree and the
functions of metad_rct_partial_f64_kernel and metad_rct_combine_f64_kernel compiled for the host - against tests/metad_rct_oracle.py,
whole-table numpy in `np.longdouble`; then the exact cases that catch a miscounted tail, entries that are not finite, the stride, the
refusals and `bias.MetadRun`'s new constructor errors.  Tables and the bound: tests/metad_rct_cases.py."""

import math

import numpy as np
import pytest
import torch

from molann_amd import _capi
from molann_amd import bias as mbias

import metad_rct_cases as rc
import metad_rct_oracle as oracle
import placement as pl

F64, INF, NAN, KT, INV_DT = rc.F64, rc.INF, rc.NAN, rc.KT, rc.INV_DT
E_NULL, E_DESC, E_ALIGNMENT = -1, -2, -6
_WORST = [0.0]


# ---------------------------------------------------------------------------------------------- the twin against the oracle
@pytest.mark.parametrize("which", sorted(rc.RANGES))
@pytest.mark.parametrize("n", rc.SIZES)
def test_twin_matches_the_oracle_on_uniform_tables(n, which):
    table = rc.uniform_table(n, which)
    rct, partials = rc.host_rct(table)
    _WORST[0] = max(_WORST[0], rc.assert_close(rct, table, what=which))
    assert rct[1].item() == 1.0 and rct[5].item() == 0.0 and partials.shape[0] == rc.chunks(n) == -(-n // 2048)
    plain, _ = rc.host_rct(table, inv_dT=0.0)
    _WORST[0] = max(_WORST[0], rc.assert_close(plain, table, inv_dT=0.0, what=which + ", plain"))
    assert abs(float(plain[4]) - math.log(n)) <= rc.BOUND * max(1.0, math.log(n))           # SV = n
    print("worst error / bound so far: %.3g" % _WORST[0])


@pytest.mark.parametrize("shape", rc.GROWN)
def test_twin_matches_the_oracle_on_grown_tables(shape):
    table = rc.grown_table(shape)
    before = table.clone()
    rct, _ = rc.host_rct(table)
    rc.assert_close(rct, table, what="grown %s" % (shape,))
    assert pl.same_bits(table, before)
    flat, _ = rc.host_rct(table.reshape(-1))
    assert pl.same_bits(rct, flat)                                                            # the number of axes does not matter
    assert 0.0 < float(rct[0]) < float(rct[2])                                                # 0 <= min V < c < max V on a table that is not flat


# ---------------------------------------------------------------------------------------------- a spike
SPIKE = 700.0 * KT


@pytest.mark.parametrize("at", [0, 63, 64, 255, 256, 2047, 2048, 4098])
def test_a_spike_of_700_kT(at):
    table = torch.zeros(4099, dtype=F64)
    table[at] = SPIKE
    rct, partials = rc.host_rct(table)
    assert float(rct[2]) == SPIKE and float(partials[:, 0].max()) == SPIKE
    rc.assert_close(rct, table, what="spike at %d" % at)


@pytest.mark.parametrize("pair", [(5, 2048 + 5), (100, 4098), (7, 7 + 256), (2048 + 300, 2048 + 300 + 5 * 256)])
def test_two_equal_spikes(pair):
    """In different chunks, and in one thread's slots (entries 256 apart within a chunk)."""
    table = torch.zeros(4099, dtype=F64)
    table[list(pair)] = SPIKE
    rct, _ = rc.host_rct(table)
    assert float(rct[2]) == SPIKE
    rc.assert_close(rct, table, what="spikes at %s" % (pair,))
    one = torch.zeros(4099, dtype=F64)
    one[pair[0]] = SPIKE
    alone, _ = rc.host_rct(one)
    # both sums are the spikes' alone to 1e-30: S0 and SV double, so c stays and each log-sum gains log 2
    assert abs(float(rct[0]) - float(alone[0])) <= rc.BOUND * (KT + SPIKE)
    assert all(abs(float(rct[i]) - float(alone[i]) - math.log(2.0)) <= rc.BOUND * abs(float(rct[i])) for i in (3, 4))


# ---------------------------------------------------------------------------------------------- exact: a miscounted tail shows
@pytest.mark.parametrize("n", rc.SIZES)
def test_constant_and_zero_tables_are_exact(n):
    rct, _ = rc.host_rct(torch.full((n,), 3.25, dtype=F64))
    assert float(rct[0]) == 3.25 and float(rct[2]) == 3.25
    zero, partials = rc.host_rct(torch.zeros(n, dtype=F64))
    assert float(zero[0]) == 0.0 and abs(math.exp(float(zero[3])) - n) <= 1e-12 * n and abs(math.exp(float(zero[4])) - n) <= 1e-12 * n
    assert float(partials[:, 1].sum()) == n and float(partials[:, 2].sum()) == n and not bool(partials[:, 3].any())
    minus = torch.zeros(n, dtype=F64)
    minus[::3] = -0.0
    mixed, _ = rc.host_rct(minus)
    assert float(mixed[0]) == 0.0 and float(mixed[2]) == 0.0 and float(mixed[3]) == float(zero[3])
    every, _ = rc.host_rct(torch.full((n,), -0.0, dtype=F64))
    assert float(every[0]) == 0.0 and float(every[3]) == float(zero[3])


def test_an_extreme_table_overflows_nowhere():
    table = torch.tensor([1.7e308, -1.7e308, 0.0, 1.7e308, 5.0], dtype=F64)
    for inv_dT in (INV_DT, 0.0):
        rct, _ = rc.host_rct(table, inv_dT=inv_dT)
        assert float(rct[2]) == 1.7e308 and math.isfinite(float(rct[0])) and float(rct[6]) == 0.0
        assert abs(float(rct[4]) - (inv_dT * 1.7e308 + math.log(2.0 if inv_dT else 5.0))) <= rc.BOUND * max(1.0, abs(float(rct[4])))


# ---------------------------------------------------------------------------------------------- entries that are not finite
@pytest.mark.parametrize("n", [5, 4099])
def test_entries_that_are_not_finite_are_counted_and_poison_the_offset(n):
    base = rc.uniform_table(n, "0..50 kT")
    for where in (0, n // 2, n - 1):
        for k, value in enumerate((NAN, INF, -INF)):
            table = base.clone()
            table[where] = value
            if k == 2:
                table[(where + 1) % n] = NAN                                   # two of them
            before = table.clone()
            rct = torch.zeros(8, dtype=F64)
            rct[1] = 4.0
            rc.host_rct(table, rct=rct)
            assert float(rct[6]) == (2.0 if k == 2 else 1.0) and float(rct[1]) == 5.0 and float(rct[7]) == 0.0
            assert all(math.isnan(float(rct[i])) for i in (0, 2, 3, 4)), rct
            assert pl.same_bits(table, before)
            want = oracle.offset(table.numpy(), KT, INV_DT)
            assert want["bad"] == int(rct[6]) and math.isnan(want["c"])
    nothing, _ = rc.host_rct(torch.full((n,), NAN, dtype=F64))
    assert float(nothing[6]) == n and math.isnan(float(nothing[0]))
    # the next update of a mended table is finite again
    again, _ = rc.host_rct(base, rct=nothing)
    assert float(again[6]) == 0.0 and float(again[1]) == 2.0
    rc.assert_close(again, base, what="mended")


# ---------------------------------------------------------------------------------------------- the stride
@pytest.mark.parametrize("stride", [1, 3, 7])
def test_the_stride_is_decided_from_the_state(stride):
    table = rc.uniform_table(4097, "0..50 kT")
    always, always_partials = rc.host_rct(table)
    for steps in list(range(9)) + [NAN, -5.0, 1e300, INF]:
        state = torch.tensor([3.0, 1.0, 2.0, steps, 0.0, 0.0, 0.0, 0.0], dtype=F64)
        kept = state.clone()
        rct, partials = rc.marked(8), rc.marked(rc.chunks(4097), 4)
        rc.host_rct(table, state=state, stride=stride, partials=partials, rct=rct)
        due, recorded = oracle.due(steps, stride)
        assert pl.same_bits(state, kept)
        if not due:
            assert pl.same_bits(rct, rc.marked(8)) and pl.same_bits(partials, rc.marked(rc.chunks(4097), 4)), (steps, stride)
        else:
            assert pl.same_bits(partials, always_partials), (steps, stride)
            assert rct[[0, 2, 3, 4, 6, 7]].tolist() == always[[0, 2, 3, 4, 6, 7]].tolist() and float(rct[5]) == recorded
            assert float(rct[1]) == 1.0                                        # the mark is no count: it reads as 0
    assert oracle.due(6, 3)[0] and not oracle.due(7, 3)[0] and oracle.due(NAN, 7) == (True, 0.0) and oracle.due(-5.0, 3) == (True, 0.0)


def test_updates_count_up():
    table = rc.uniform_table(300, "0..50 kT")
    rct = torch.zeros(8, dtype=F64)
    for k in range(3):
        rc.host_rct(table, rct=rct)
        assert float(rct[1]) == k + 1.0


# ---------------------------------------------------------------------------------------------- refusals
def _refusals(call):
    table = rc.uniform_table(4097, "0..50 kT")
    state = torch.zeros(8, dtype=F64)
    rct, partials = rc.marked(8), rc.marked(3, 4)
    good = dict(table=table.data_ptr(), n=4097, kT=KT, inv_dT=INV_DT, state=state.data_ptr(), stride=1, partials=partials.data_ptr(), rows=3,
                rct=rct.data_ptr())
    odd = lambda t: t.data_ptr() + 4  # noqa: E731
    faults = [(E_NULL, dict(table=None)), (E_NULL, dict(partials=None)), (E_NULL, dict(rct=None)),
              (E_ALIGNMENT, dict(table=odd(table))), (E_ALIGNMENT, dict(state=odd(state))), (E_ALIGNMENT, dict(partials=odd(partials))),
              (E_ALIGNMENT, dict(rct=odd(rct))),
              (E_DESC, dict(n=0)), (E_DESC, dict(n=-3)), (E_DESC, dict(n=2 ** 31)),
              (E_DESC, dict(kT=0.0)), (E_DESC, dict(kT=-1.0)), (E_DESC, dict(kT=NAN)), (E_DESC, dict(kT=INF)),
              (E_DESC, dict(inv_dT=-1e-9)), (E_DESC, dict(inv_dT=NAN)), (E_DESC, dict(inv_dT=INF)),
              (E_DESC, dict(stride=0)), (E_DESC, dict(stride=-2)),
              (E_DESC, dict(rows=2)), (E_DESC, dict(rows=0))]
    for code, change in faults:
        assert call(**dict(good, **change)) == code, change
    # in order: an earlier kind of fault wins over every later one
    assert call(**dict(good, rct=None, table=odd(table), n=0)) == E_NULL
    assert call(**dict(good, rct=odd(rct), n=0, kT=NAN, rows=0)) == E_ALIGNMENT
    assert call(**dict(good, n=2 ** 31, rows=0)) == E_DESC                      # the size before the rows it would need
    assert pl.same_bits(rct, rc.marked(8)) and pl.same_bits(partials, rc.marked(3, 4)), "a refusal wrote"
    return good, rct, partials, (table, state)                                   # the addresses in `good` point into these


ORDER = ("table", "n", "kT", "inv_dT", "state", "stride", "partials", "rows", "rct")


def test_every_refusal_in_order_writes_nothing():
    L = _capi.lib()
    good, rct, partials, alive = _refusals(lambda **kw: L.molann_selftest_metad_rct_f64(*[kw[k] for k in ORDER]))
    _refusals(lambda **kw: L.molann_metad_rct_f64(*[kw[k] for k in ORDER], None))           # refused before any launch: no GPU needed
    assert L.molann_selftest_metad_rct_f64(*[good[k] for k in ORDER]) == 0
    assert float(rct[1]) == 1.0 and math.isfinite(float(rct[0])) and math.isfinite(float(partials.sum()))
    assert L.molann_selftest_metad_rct_f64(*[dict(good, state=None)[k] for k in ORDER]) == 0 and float(rct[1]) == 2.0
    assert [L.molann_metad_rct_chunks(n) for n in (-1, 0, 1, 2048, 2049, 2 ** 31 - 1)] == [0, 0, 1, 1, 2, 2 ** 20]
    assert alive[0].numel() == 4097


def test_the_entries_are_declared():
    L = _capi.lib()
    for name in ("molann_metad_rct_chunks", "molann_metad_rct_f64", "molann_selftest_metad_rct_f64"):
        assert name in _capi.declared_symbols() and hasattr(L, name)
    assert len(L.molann_metad_rct_f64.argtypes) == len(ORDER) + 1 and len(L.molann_selftest_metad_rct_f64.argtypes) == len(ORDER)
    assert callable(_capi.metad_rct_f64) and _capi.ABI_VERSION == 1


# ---------------------------------------------------------------------------------------------- bias.MetadRun
class _Model(object):
    def value_and_grid(self, *a, **k):
        raise AssertionError("not called")

    value_and_bias = value_and_grid


def test_metad_run_checks_rct_stride_before_the_device():
    good = dict(model=_Model(), table=torch.zeros(5, 7, dtype=F64), lower=[0.0, 0.0], spacing=[0.1, 0.1], kT=2.5, biasfactor=10.0, height=1.2,
                sigma=[0.2, 0.2])
    for stride, error in ((True, TypeError), (False, TypeError), (1.5, TypeError), (2.0, TypeError), ("3", TypeError), (0, ValueError),
                          (-1, ValueError)):
        with pytest.raises(error, match="rct_stride"):
            mbias.MetadRun(rct_stride=stride, **good)
    for stride in (None, 1, 10, np.int64(3)):
        with pytest.raises(ValueError, match="device memory"):                 # a CPU table: the device is checked last
            mbias.MetadRun(rct_stride=stride, **good)
    doc = mbias.MetadRun.__doc__
    for word in ("rct_stride", "update_rct", "read_rct", "rbias", "molann_metad_rct_f64"):
        assert word in doc, word
    assert "torch on ``table`` when wanted" not in doc
    run = mbias.MetadRun.__new__(mbias.MetadRun)                               # the record is formed from the fields alone
    run.rct = torch.tensor([1.5, 4.0, 9.0, 3.0, 2.0, 12.0, 0.0, 0.0], dtype=F64)
    assert run.read_rct() == dict(rct=1.5, updates=4, max=9.0, log_sum_0=3.0, log_sum_V=2.0, steps=12, bad=0)
    run.rct = None
    with pytest.raises(ValueError, match="rct_stride"):
        run.read_rct()
