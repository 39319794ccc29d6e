"""Seeded tables for `molann_metad_rct_f64`, the host twin's call and the comparison against tests/metad_rct_oracle.py, shared by the host
and the GPU tests.

The bound, derived and not measured: ``|c - oracle| <= BOUND (kT + |M|)`` and the two log-sums within ``BOUND max(1, |value|)``, BOUND =
1e-12.  The terms that matter have exponents near 0, where an exp of 1-2 ulp and a tree sum of depth <= 11 + log2(chunks) give a few
1e-16 relative in S, that is a few 1e-16 kT in c, plus one rounding of M."""

import math

import numpy as np
import torch

from molann_amd import _capi

import metad_cases as mc
import metad_rct_oracle as oracle

F64 = torch.float64
INF, NAN = math.inf, math.nan
BOUND = 1e-12
KT, BIASFACTOR = 2.494, 10.0                        # kJ/mol at 300 K
INV_DT = 1.0 / (KT * (BIASFACTOR - 1.0))
CHUNK = 2048
# around a wave, a block, a chunk and two chunks; 256 whole chunks and one entry more: the combine block's second stride
SIZES = (4, 5, 255, 256, 257, 2047, 2048, 2049, 4097, 524288, 524289)
RANGES = {"0..50 kT": (0.0, 50.0 * KT), "0..1000 kT": (0.0, 1000.0 * KT), "-3000..-2000": (-3000.0, -2000.0)}
GROWN = ((5, 7), (4, 5, 6), (33, 65))
MARK = 0x7FF8BEEF0BADF00D                           # a NaN with a payload: what a buffer that must keep its bits is filled with


def uniform_table(n, which, seed=0):
    lo, hi = RANGES[which]
    return torch.from_numpy(np.random.RandomState(7 * n % 100003 + seed).uniform(lo, hi, size=n))


def grown_table(shape):
    """A table grown by the deposit's host twin: three steps of 65 walkers from tests/metad_cases.py."""
    table, state = torch.zeros(shape, dtype=F64), torch.zeros(8, dtype=F64)
    for seed in range(3):
        case = mc.Case(shape, (False,) * len(shape), 65, seed=seed)
        assert mc.host_deposit(table, case.lower, case.spacing, case.periodic, case.sigma, None, case.y, case.V, inv_dT=INV_DT, state=state) == 0
    assert float(table.max()) > 0.0
    return table


def chunks(n):
    return int(_capi.lib().molann_metad_rct_chunks(n))


def marked(*shape):
    return torch.full(shape, MARK, dtype=torch.int64).view(F64)


def host_rct(table, kT=KT, inv_dT=INV_DT, state=None, stride=1, partials=None, rct=None):
    """`molann_selftest_metad_rct_f64` on CPU tensors: (rct, partials).  `rct` starts from zeros where none is given."""
    table = table.contiguous()
    partials = torch.zeros(chunks(table.numel()), 4, dtype=F64) if partials is None else partials
    rct = torch.zeros(8, dtype=F64) if rct is None else rct
    code = _capi.lib().molann_selftest_metad_rct_f64(table.data_ptr(), table.numel(), float(kT), float(inv_dT), None if state is None else state.data_ptr(),
                                                     int(stride), partials.data_ptr(), partials.shape[0], rct.data_ptr())
    assert code == 0, code
    return rct, partials


def errors(rct, want, kT=KT):
    """(error / bound) of c and of the two log-sums against the oracle's dict, M being exact; asserts nothing."""
    rct = [float(v) for v in rct]
    scale = BOUND * (kT + abs(float(want["M"])))
    ratios = [abs(np.longdouble(rct[0]) - want["c"]) / scale]
    for got, key in ((rct[3], "log0"), (rct[4], "logV")):
        ratios.append(abs(np.longdouble(got) - want[key]) / (BOUND * max(1.0, abs(float(want[key])))))
    return [float(r) for r in ratios]


def assert_close(rct, table, kT=KT, inv_dT=INV_DT, what=""):
    """The offset, the maximum and the log-sums of `rct` against the oracle on `table`, within the bound; returns the worst error / bound."""
    want = oracle.offset(table.detach().cpu().numpy(), kT, inv_dT)
    ratios = errors(rct, want, kT)
    print("%s n %d: c %.17g, error / bound: c %.3g, log S0 %.3g, log SV %.3g" % (what, table.numel(), float(rct[0]), ratios[0], ratios[1], ratios[2]))
    assert float(rct[2]) == float(want["M"]), (float(rct[2]), float(want["M"]))
    assert float(rct[6]) == 0.0 and float(rct[7]) == 0.0
    assert max(ratios) <= 1.0, ratios
    return max(ratios)
