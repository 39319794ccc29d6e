"""Seeded cases of parallel-bias metadynamics and the host twins' calls, shared by the host and the GPU tests.

The bounds are the project's own.  Frames: the float64 family's - energies within 1e-10 max(1, |V|max), the cotangent within 1e-9
max(1e-3, |dy|max).  Tables: every entry of table k within ``BOUND (sum_a h_ak + max |T_k before|)``, BOUND = 1e-12, by the derivation
of tests/metad_cases.py: a term h exp(-q / 2) carries a few eps h, a height here two more exponentials and a division, a few eps h
more, and adding W <= 257 terms to an entry 257 * 1.1e-16 |t| = 2.9e-14 |t|."""

import math

import numpy as np
import torch

from molann_amd import _capi

F64 = torch.float64
INF, NAN = math.inf, math.nan
BOUND = 1e-12
KT = 2.494
HEIGHT0, INV_DT = 1.2, 1.0 / (KT * 9.0)             # kJ/mol: kT at 300 K, biasfactor 10
WALKERS = (1, 3, 8, 9, 64, 65, 257)                 # one, a few, around a small chunk, a whole chunk of the kernel, one more, several chunks
# K = 8: tiles per axis 1, 2, 5, 1, 1, 3, 1, 2 - the block -> (axis, tile) walk crosses every kind of boundary
SHAPE8 = (4, 257, 1025, 5, 67, 513, 256, 300)
PERIODIC8 = (False, True, False, True, False, True, False, True)
SMALL = [((67,), (False,)), ((67,), (True,)), ((5, 300), (True, False)), ((257, 4, 67), (False, True, True))]


class Case(object):
    """K tables, their grids and W walkers, seeded.  sigma is no multiple of the spacing; the centres lie inside the range and a little
    outside it; the V_k span a few kT, so the weights and the heights differ by orders of magnitude."""

    def __init__(self, shape, periodic, walkers, seed=0, n_out=None, columns=None, v_pad=0, start="zero"):
        K = len(shape)
        rng = np.random.RandomState(1000 * K + 17 * walkers + seed)
        self.shape, self.periodic, self.K, self.walkers = tuple(shape), tuple(periodic), K, walkers
        self.lower = [-1.3 - 0.4 * k for k in range(K)]
        self.spacing = [0.37 + 0.11 * k for k in range(K)]
        self.sigma = [0.83 * self.spacing[k] * (1.0 + 0.27 * k) for k in range(K)]
        self.columns = None if columns is None else list(columns)
        n_out = K if n_out is None else n_out
        cols = list(range(K)) if columns is None else list(columns)
        y = rng.uniform(-3.0, 3.0, size=(walkers, n_out))
        for k in range(K):
            y[:, cols[k]] = self.lower[k] + rng.uniform(-0.2, 1.2, size=walkers) * shape[k] * self.spacing[k]
        self.y = torch.from_numpy(y)
        self.e_store = torch.from_numpy(rng.uniform(-6.0, 8.0, size=(walkers, 2 + K + v_pad)))   # the energies of a bias launch, maybe wider
        self.V = self.e_store[:, 2:2 + K]
        n = sum(shape)
        self.table = torch.zeros(n, dtype=F64) if start == "zero" else torch.from_numpy(rng.uniform(-5.0, 5.0, size=n))
        self.offsets = [sum(shape[:k]) for k in range(K + 1)]

    def axis(self, table, k):
        return table[self.offsets[k]:self.offsets[k + 1]]


def arrays(shape, lower, spacing, periodic, sigma, columns):
    return _capi.metad_grid_arrays(shape, lower, spacing, periodic, sigma, columns)


def host_deposit(table, shape, lower, spacing, periodic, sigma, columns, y, V, height0=HEIGHT0, inv_dT=INV_DT, kT=KT, cutoff=None, state=None,
                 log=None):
    """`molann_selftest_pbmetad_deposit_f64` on CPU tensors, in place; returns the code.  `V` may be columns of a wider tensor."""
    a = arrays(shape, lower, spacing, periodic, sigma, columns)
    return _capi.lib().molann_selftest_pbmetad_deposit_f64(
        table.data_ptr(), len(shape), a[0], a[1], a[2], a[3], a[4], a[5], y.data_ptr(), y.stride(0), V.data_ptr(), V.stride(0), y.shape[0],
        float(height0), float(inv_dT), float(kT), INF if cutoff is None else float(cutoff), state.data_ptr(),
        None if log is None else log.data_ptr(), 0 if log is None else log.shape[0])


def run_case(case, cutoff=None, table=None, state=None, log=None, height0=HEIGHT0, inv_dT=INV_DT, kT=KT):
    table = case.table.clone() if table is None else table
    state = torch.zeros(8, dtype=F64) if state is None else state
    code = host_deposit(table, case.shape, case.lower, case.spacing, case.periodic, case.sigma, case.columns, case.y, case.V, height0, inv_dT, kT,
                        cutoff, state, log)
    assert code == 0, code
    return table, state


def host_heights(V, height0=HEIGHT0, inv_dT=INV_DT, kT=KT):
    """The twin's own heights [W, K] of walkers that are all valid: what it logs for them, one deposit on throw-away tables."""
    n, K = V.shape
    table, state, log = torch.zeros(4 * K, dtype=F64), torch.zeros(8, dtype=F64), torch.zeros(n, 2 * K, dtype=F64)
    y = torch.zeros(n, K, dtype=F64)
    assert host_deposit(table, [4] * K, [0.0] * K, [1.0] * K, None, [1.0] * K, None, y, V, height0, inv_dT, kT, None, state, log) == 0
    assert int(state[0]) == n
    return log[:, K:].clone()


def tolerance(heights_k, before_k):
    return BOUND * (float(heights_k.sum()) + float(before_k.abs().max()))


def host_frame(y, tables, kT, restraint=None):
    """`molann_selftest_pbmetad_f64` on one frame y [d_out] (CPU): (code, energies [2 + K], dy [d_out]).  tables: a `bias.PBTables` on
    the CPU; restraint: None or CPU rows (center, kappa, period, flat)."""
    K = len(tables.shape)
    r = None if restraint is None else tuple(restraint) + (0,)
    terms, keep = _capi.pbmetad_terms_f64(((None, K) if tables.columns is None else tables.columns, tables.table, tables.shape, tables.lower,
                                           tables.spacing, tables.periodic, kT), r)
    energies, dy = torch.full((2 + K,), 7.0, dtype=F64), torch.full((y.numel(),), 7.0, dtype=F64)
    code = _capi.lib().molann_selftest_pbmetad_f64(y.data_ptr(), y.numel(), terms, energies.data_ptr(), dy.data_ptr())
    del keep
    return code, energies, dy
