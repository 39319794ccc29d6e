"""An independent numpy restatement of `molann_metad_widths_f64` and `molann_metad_deposit_cov_f64` (include/molann_hip.h): the
observation and the limits as plain loops, a hill's exponent by `np.linalg.solve` on the full matrix, the deposit as a loop over the
walkers and, by numpy, over the grid points.  No tiles, no staging, no Cholesky factor in the exponent, no shared code with the library
- what the host twins and the kernels are checked against."""

import numpy as np

DIFF, GEOM = 1, 2


def tri_len(d):
    return d * (d + 1) // 2


def full(tri, d):
    """The symmetric d x d matrix whose row-major upper triangle is `tri`."""
    C = np.zeros((d, d))
    at = 0
    for i in range(d):
        for j in range(i, d):
            C[i, j] = C[j, i] = tri[at]
            at += 1
    return C


def triangle(C):
    d = C.shape[0]
    return np.array([C[i, j] for i in range(d) for j in range(i, d)], dtype=np.float64)


def observe(row, y, lower, period, window):
    """One observation of `y` [d] by a walker's row (n, mean[d], cov[T]); returns ``(row, skipped)``.  `period[k]` 0: not periodic."""
    d = len(y)
    row = np.array(row, dtype=np.float64)
    if not np.isfinite(y).all():
        return row, True
    decay = 1.0 / window
    if row[0] == 0:
        row[1:1 + d] = y
        row[1 + d:] = 0.0
        row[0] = 1.0
        return row, False
    delta = np.zeros(d)
    for k in range(d):
        dk = y[k] - row[1 + k]
        if period[k] > 0:
            dk = dk - period[k] * np.rint(dk / period[k])
        delta[k] = dk
        m = row[1 + k] + decay * dk
        if period[k] > 0:
            m = m - period[k] * np.floor((m - lower[k]) / period[k])
        row[1 + k] = m
    at = 1 + d
    for i in range(d):
        for j in range(i, d):
            row[at] = row[at] + decay * (delta[i] * delta[j] - row[at])
            at += 1
    row[0] += 1.0
    return row, False


def limits(C, sigma_min, sigma_max):
    """PLUMED's SIGMA_MIN / SIGMA_MAX on a full matrix, k ascending; None: 0 / +inf."""
    C = np.array(C, dtype=np.float64)
    d = C.shape[0]
    for k in range(d):
        lo = 0.0 if sigma_min is None else sigma_min[k] ** 2
        hi = np.inf if sigma_max is None else sigma_max[k] ** 2
        ckk = C[k, k]
        target = lo if ckk < lo else hi if ckk > hi else ckk
        if target != ckk:
            if ckk > 0:
                s = np.sqrt(target / ckk)
                C[k, :] *= s
                C[:, k] *= s
            else:
                C[k, :] = 0.0
                C[:, k] = 0.0
            C[k, k] = target
    return C


def hill_diff(row, sigma, d, window):
    return full(row[1 + d:], d) if row[0] >= window else np.diag(np.asarray(sigma, dtype=np.float64) ** 2)


def hill_geom(metric, columns, sigma):
    s = np.asarray(sigma, dtype=np.float64)
    return np.outer(s, s) * np.asarray(metric)[np.ix_(columns, columns)]


def widths(mode, d, lower, period, sigma, sigma_min, sigma_max, columns, window, emit, adapt, adapt_state, y=None, metric=None):
    """The widths step on numpy arrays: returns ``(adapt, adapt_state, cov)``, `cov` [W, T] or None without `emit`."""
    adapt_state = np.array(adapt_state, dtype=np.float64)
    columns = list(range(d)) if columns is None else list(columns)
    W = len(y) if mode == DIFF else len(metric)
    adapt = None if adapt is None else np.array(adapt, dtype=np.float64)
    cov = np.zeros((W, tri_len(d))) if emit else None
    for a in range(W):
        if mode == DIFF:
            adapt[a], skipped = observe(adapt[a], np.asarray(y, dtype=np.float64)[a, columns], lower, period, window)
            adapt_state[2 if skipped else 0] += 1
            C = hill_diff(adapt[a], sigma, d, window)
        else:
            C = hill_geom(metric[a], columns, sigma)
        if emit:
            cov[a] = triangle(limits(C, sigma_min, sigma_max))
    if emit:
        adapt_state[1] += 1
    return adapt, adapt_state, cov


def usable(C):
    """Finite everywhere and every Cholesky pivot above 1e-12 of its diagonal entry."""
    d = C.shape[0]
    if not np.isfinite(C).all():
        return False
    L = np.zeros((d, d))
    for k in range(d):
        p = C[k, k] - float(np.sum(L[k, :k] ** 2))
        if not p > 1e-12 * C[k, k]:
            return False
        L[k, k] = np.sqrt(p)
        for i in range(k + 1, d):
            L[i, k] = (C[i, k] - float(np.sum(L[i, :k] * L[k, :k]))) / L[k, k]
    return True


def deltas(shape, lower, spacing, periodic, centre):
    """The wrapped ``g - centre`` at every table entry: an array [*shape, d]."""
    d = len(shape)
    out = np.zeros(tuple(shape) + (d,))
    for k in range(d):
        g = lower[k] + np.arange(shape[k], dtype=np.float64) * spacing[k]
        delta = g - centre[k]
        if periodic is not None and periodic[k]:
            P = shape[k] * spacing[k]
            delta = delta - P * np.rint(delta / P)
        view = [1] * d
        view[k] = shape[k]
        out[..., k] = delta.reshape(view)
    return out


def entry_q(shape, lower, spacing, periodic, C, centre):
    """``q = delta^T C^-1 delta`` at every table entry for one centre, by `np.linalg.solve`."""
    dl = deltas(shape, lower, spacing, periodic, centre)
    flat = dl.reshape(-1, len(shape))
    x = np.linalg.solve(C, flat.T).T
    return np.sum(flat * x, axis=1).reshape(shape)


def heights(V, height0, inv_dT):
    with np.errstate(all="ignore"):
        return height0 * np.exp(-np.asarray(V, dtype=np.float64) * inv_dT) if inv_dT > 0 else np.full(len(V), float(height0))


def deposit(table, lower, spacing, periodic, columns, y, V, cov, height0, inv_dT, cutoff, state, log=None):
    """The covariant deposit on numpy arrays: returns ``(table, state, log)`` as new arrays.  `y` [W, n_out], `V` [W], `cov` [W, T]."""
    table, state = np.array(table, dtype=np.float64), np.array(state, dtype=np.float64)
    log = None if log is None else np.array(log, dtype=np.float64)
    shape, d = table.shape, table.ndim
    columns = list(range(d)) if columns is None else list(columns)
    c2 = np.inf if cutoff is None else float(cutoff) ** 2
    centres = np.asarray(y, dtype=np.float64)[:, columns]
    V = np.asarray(V, dtype=np.float64)
    h = heights(V, height0, inv_dT)
    for a in range(len(V)):
        C = full(cov[a], d)
        ok = np.isfinite(V[a]) and np.isfinite(centres[a]).all() and np.isfinite(h[a]) and h[a] > 0 and usable(C)
        if not ok:
            state[1] += 1
            continue
        q = entry_q(shape, lower, spacing, periodic, C, centres[a])
        inside = q <= c2
        term = h[a] * np.exp(-0.5 * q)
        table[inside] = table[inside] + term[inside]
        state[0] += 1
        state[2] += h[a]
        if log is not None and state[4] < log.shape[0]:
            log[int(state[4])] = np.concatenate([centres[a], np.asarray(cov[a], dtype=np.float64), [h[a]]])
            state[4] += 1
    state[3] += 1
    return table, state, log


def cutoff_margin(shape, lower, spacing, periodic, columns, y, cov, cutoff):
    """The smallest ``|q / c^2 - 1|`` over every entry and every finite centre with a usable matrix, q the covariant exponent."""
    d = len(shape)
    columns = list(range(d)) if columns is None else list(columns)
    centres = np.asarray(y, dtype=np.float64)[:, columns]
    c2 = float(cutoff) ** 2
    margin = np.inf
    for a, centre in enumerate(centres):
        C = full(cov[a], d)
        if np.isfinite(centre).all() and usable(C):
            margin = min(margin, float(np.abs(entry_q(shape, lower, spacing, periodic, C, centre) / c2 - 1.0).min()))
    return margin
