"""Seeded cases of `molann_metad_deposit_cov_f64`, `molann_metad_widths_f64` and their host twins, shared by the host and the GPU tests.

The table, the grid, the walkers and the bound are tests/metad_cases.py's.  A walker's covariance is ``R o sigma sigma^T`` with R a random
correlation matrix and ``sigma_k`` in [0.3, 0.9] x 3 spacings; every case asserts ``cond(C) <= 100``.  Over 4002 such matrices on the CPU
(1334 per d, 200 displacements each) the largest condition number was 61, the exponent by the Cholesky factor and forward substitution
(the library's) and by `np.linalg.solve` (the oracle's) differed by at most 4.4e-16 per unit height in the term, and the per-axis
reach bound ``q >= delta_k^2 / C_kk`` (to the factor 1 + 1e-12 the kernel allows) was never violated: the
bound ``BOUND (sum_a h_a + max |table before|)``, BOUND = 1e-12, is metad_cases' derivation plus that 4.4e-16 - the same 30x of room."""

import numpy as np
import torch

import metad_cases as mc
import metad_cov_oracle as oracle
from molann_amd import _capi

F64, INF, NAN, BOUND = mc.F64, mc.INF, mc.NAN, mc.BOUND
HEIGHT0, INV_DT = mc.HEIGHT0, mc.INV_DT
WALKERS = (1, 3, 8, 9, 64, 65, 257)        # 8, 9: the 1-D kernel's chunk and one more; 64, 65: the 2-D and 3-D kernels'; several chunks
SHAPES, TILE_SHAPES = mc.SHAPES, mc.TILE_SHAPES
WIDTH = 3.0                                  # "a few spacings"
DIFF, GEOM = oracle.DIFF, oracle.GEOM


def random_covariances(rng, n, spacing):
    """[n, T] upper triangles of ``R o sigma sigma^T``: R = normalised ``A A^T + I`` of a random d x d A, sigma_k = u WIDTH spacing_k with
    u uniform in [0.3, 0.9]."""
    d = len(spacing)
    out = np.zeros((n, oracle.tri_len(d)))
    for a in range(n):
        A = rng.normal(size=(d, d))
        S = A @ A.T + np.eye(d)
        s = np.sqrt(np.diag(S))
        R = S / np.outer(s, s)
        sigma = rng.uniform(0.3, 0.9, size=d) * WIDTH * np.asarray(spacing)
        C = R * np.outer(sigma, sigma)
        assert np.linalg.cond(C) <= 100.0, np.linalg.cond(C)
        out[a] = oracle.triangle(C)
    return out


class CovCase(mc.Case):
    """`metad_cases.Case` plus one covariance per walker, `cov` [W, T] (a column block of `cov_store` where `cov_stride` is wider)."""

    def __init__(self, shape, periodic, walkers, seed=0, cov_width=None, cov_offset=0, **kw):
        super().__init__(shape, periodic, walkers, seed=seed, **kw)
        rng = np.random.RandomState(7000 * len(shape) + 31 * walkers + seed)
        T = oracle.tri_len(self.d)
        width = T if cov_width is None else cov_width
        store = rng.uniform(-1.0, 1.0, size=(walkers, width))
        store[:, cov_offset:cov_offset + T] = random_covariances(rng, walkers, self.spacing)
        self.cov_store = torch.from_numpy(store)
        self.cov = self.cov_store[:, cov_offset:cov_offset + T]
        self.T = T

    def period(self):
        return [self.shape[k] * self.spacing[k] if self.periodic[k] else 0.0 for k in range(self.d)]


def host_deposit_cov(table, lower, spacing, periodic, columns, y, V, cov, height0=HEIGHT0, inv_dT=INV_DT, cutoff=None, state=None, log=None):
    """`molann_selftest_metad_deposit_cov_f64` on CPU tensors, in place; returns the code.  `V` and `cov` may be columns of wider tensors."""
    d = table.dim()
    shape_a, lower_a, spacing_a, periodic_a, _, columns_a = _capi.metad_grid_arrays(table.shape, lower, spacing, periodic, [1.0] * d, columns)
    return _capi.lib().molann_selftest_metad_deposit_cov_f64(
        table.data_ptr(), d, shape_a, lower_a, spacing_a, periodic_a, columns_a, y.data_ptr(), y.stride(0), V.data_ptr(),
        V.stride(0) if V.dim() else 0, cov.data_ptr(), cov.stride(0), y.shape[0], float(height0), float(inv_dT),
        INF if cutoff is None else float(cutoff), state.data_ptr(), None if log is None else log.data_ptr(), 0 if log is None else log.shape[0])


def host_widths(shape, lower, spacing, periodic, sigma, columns, mode, window, emit, adapt, adapt_state, cov, y=None, metric=None, sigma_min=None,
                sigma_max=None):
    """`molann_selftest_metad_widths_f64` on CPU tensors, in place; returns the code."""
    d = len(shape)
    shape_a, lower_a, spacing_a, periodic_a, sigma_a, columns_a = _capi.metad_grid_arrays(shape, lower, spacing, periodic, sigma, columns)
    lo, hi = _capi.metad_limit_arrays(sigma_min, sigma_max, d)
    n_out = 0 if metric is None else metric.shape[-1]
    W = y.shape[0] if y is not None else metric.shape[0]
    return _capi.lib().molann_selftest_metad_widths_f64(
        d, shape_a, lower_a, spacing_a, periodic_a, sigma_a, lo, hi, columns_a, None if y is None else y.data_ptr(), 0 if y is None else y.stride(0),
        None if metric is None else metric.data_ptr(), n_out * n_out, n_out, W, mode, window, 1 if emit else 0,
        None if adapt is None else adapt.data_ptr(), adapt_state.data_ptr(), None if cov is None else cov.data_ptr(),
        0 if cov is None else cov.stride(0))


def tolerance(heights, before):
    return mc.tolerance(heights, before)
