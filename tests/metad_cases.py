"""Seeded cases of `molann_metad_deposit_f64` and the host twin's call, shared by the host and the GPU tests.

The bound: every table entry within ``BOUND (sum_a h_a + max |table before|)``, BOUND = 1e-12.  A term h exp(-q / 2) carries an
absolute error of a few eps h max_a(a exp(-a)) <= eps h (the exponent's rounding, multiplied by the term's slope), the product of up
to three exponentials at 1-2 ulp a few eps h more, and adding W <= 257 terms to an entry W eps |t| <= 257 * 1.1e-16 |t| = 2.9e-14 |t|
with |t| <= sum_a h_a + max |table before|: 1e-12, the project's float64 bar, leaves about 30x."""

import math

import numpy as np
import torch

from molann_amd import _capi

F64 = torch.float64
INF, NAN = math.inf, math.nan
BOUND = 1e-12
HEIGHT0, INV_DT = 1.2, 1.0 / (2.494 * 9.0)          # kJ/mol: kT at 300 K, biasfactor 10
WALKERS = (1, 3, 64, 65, 257)                       # one, a few, a whole chunk of the 2-D / 3-D kernels, one more, several chunks
# shape, periodic: 1-D at the minimum, one more and past a wave; 2-D with every mix of periodic axes; 3-D
SHAPES = [((4,), (False,)), ((5,), (True,)), ((67,), (False,)), ((67,), (True,)),
          ((5, 7), (False, False)), ((5, 7), (True, False)), ((5, 7), (False, True)), ((5, 7), (True, True)),
          ((4, 5, 6), (False, True, False))]
# one entry past a tile (256; 16 x 16; 4 x 4 x 16) and past several tiles, per axis
TILE_SHAPES = [((257,), (False,)), ((1025,), (True,)), ((17, 33), (True, False)), ((33, 65), (False, True)), ((5, 9, 17), (False, False, True)),
               ((9, 17, 33), (True, False, False))]


class Case(object):
    """A table, its grid and W walkers, seeded.  sigma is no multiple of the spacing; the centres lie inside the range and a little
    outside it; V spans a few kT (biasfactor - 1), so the heights differ by an order of magnitude."""

    def __init__(self, shape, periodic, walkers, seed=0, n_out=None, columns=None, v_stride=1, v_offset=0, start="zero"):
        rng = np.random.RandomState(1000 * len(shape) + 17 * walkers + seed)
        d = len(shape)
        self.shape, self.periodic, self.d, self.walkers = tuple(shape), tuple(periodic), d, walkers
        self.lower = [-1.3 - 0.4 * k for k in range(d)]
        self.spacing = [0.37 + 0.11 * k for k in range(d)]
        self.sigma = [0.83 * self.spacing[k] * (1.0 + 0.27 * k) for k in range(d)]
        self.columns = None if columns is None else list(columns)
        n_out = d if n_out is None else n_out
        cols = list(range(d)) if columns is None else list(columns)
        span = [shape[k] * self.spacing[k] for k in range(d)]
        y = rng.uniform(-3.0, 3.0, size=(walkers, n_out))
        for k in range(d):
            y[:, cols[k]] = self.lower[k] + rng.uniform(-0.2, 1.2, size=walkers) * span[k]
        self.y = torch.from_numpy(y)
        self.v_store = torch.from_numpy(rng.uniform(-30.0, 40.0, size=(walkers, v_stride)))
        self.V = self.v_store[:, v_offset]
        self.table = torch.zeros(shape, dtype=F64) if start == "zero" else torch.from_numpy(rng.uniform(-5.0, 5.0, size=shape))

    def grid(self):
        return dict(lower=self.lower, spacing=self.spacing, periodic=self.periodic, sigma=self.sigma, columns=self.columns)


def _arrays(shape, lower, spacing, periodic, sigma, columns):
    return _capi.metad_grid_arrays(shape, lower, spacing, periodic, sigma, columns)


def host_deposit(table, lower, spacing, periodic, sigma, columns, y, V, height0=HEIGHT0, inv_dT=INV_DT, cutoff=None, state=None, log=None):
    """`molann_selftest_metad_deposit_f64` on CPU tensors, in place; returns the code.  `table`, `y`, `state`, `log` contiguous; `V`
    may be a column of a wider tensor."""
    shape_a, lower_a, spacing_a, periodic_a, sigma_a, columns_a = _arrays(table.shape, lower, spacing, periodic, sigma, columns)
    return _capi.lib().molann_selftest_metad_deposit_f64(
        table.data_ptr(), table.dim(), shape_a, lower_a, spacing_a, periodic_a, sigma_a, columns_a, y.data_ptr(), y.stride(0), V.data_ptr(),
        V.stride(0) if V.dim() else 0, y.shape[0], float(height0), float(inv_dT), INF if cutoff is None else float(cutoff), state.data_ptr(),
        None if log is None else log.data_ptr(), 0 if log is None else log.shape[0])


def host_heights(V, height0=HEIGHT0, inv_dT=INV_DT):
    """The twin's own heights of the walkers whose V gives one (finite and > 0): what it logs for them, one deposit on a throw-away table."""
    n = V.shape[0]
    table, state, log = torch.zeros(4, dtype=F64), torch.zeros(8, dtype=F64), torch.zeros(n, 3, dtype=F64)
    y = torch.zeros(n, 1, dtype=F64)
    assert host_deposit(table, [0.0], [1.0], None, [1.0], None, y, V, height0, inv_dT, None, state, log) == 0
    return log[:int(state[0]), 2].clone()


def tolerance(heights, before):
    return BOUND * (float(heights.sum()) + float(before.abs().max()))
