"""An independent numpy restatement of `molann_metad_deposit_f64` (include/molann_hip.h): a plain loop over the walkers and, by numpy,
over the grid points.  No tiles, no staging, no shared code with the library - what the host twin and the kernel are checked against."""

import numpy as np


def heights(V, height0, inv_dT):
    """``h_a = height0 exp(-V_a inv_dT)`` and which walkers' heights are finite and > 0."""
    with np.errstate(all="ignore"):
        h = height0 * np.exp(-np.asarray(V, dtype=np.float64) * inv_dT) if inv_dT > 0 else np.full(len(V), float(height0))
    return h


def valid(y, V, h):
    return np.isfinite(V) & np.isfinite(y).all(axis=1) & np.isfinite(h) & (h > 0)


def axis_q(n, lower, spacing, periodic, sigma, yk):
    """``(delta_k / sigma_k)^2`` at every point of one axis for one centre."""
    g = lower + np.arange(n, dtype=np.float64) * spacing
    delta = g - yk
    if periodic:
        P = n * spacing
        delta = delta - P * np.rint(delta / P)
    return (delta / sigma) ** 2


def entry_q(shape, lower, spacing, periodic, sigma, centre):
    """``q = sum_k (delta_k / sigma_k)^2`` at every table entry for one centre, k ascending."""
    d = len(shape)
    q = np.zeros(shape)
    for k in range(d):
        view = [1] * d
        view[k] = shape[k]
        q = q + axis_q(shape[k], lower[k], spacing[k], bool(periodic[k]) if periodic is not None else False, sigma[k], centre[k]).reshape(view)
    return q


def deposit(table, lower, spacing, periodic, sigma, columns, y, V, height0, inv_dT, cutoff, state, log=None):
    """The step on numpy arrays: returns ``(table, state, log)`` as new arrays.  `y` [W, n_out], `V` [W]; `cutoff` None or inf: none."""
    table, state = np.array(table, dtype=np.float64), np.array(state, dtype=np.float64)
    log = None if log is None else np.array(log, dtype=np.float64)
    shape, d = table.shape, table.ndim
    columns = list(range(d)) if columns is None else list(columns)
    c2 = np.inf if cutoff is None else float(cutoff) ** 2
    centres = np.asarray(y, dtype=np.float64)[:, columns]
    V = np.asarray(V, dtype=np.float64)
    h = heights(V, height0, inv_dT)
    ok = valid(centres, V, h)
    for a in range(len(V)):
        if not ok[a]:
            state[1] += 1
            continue
        q = entry_q(shape, lower, spacing, periodic, sigma, centres[a])
        inside = q <= c2
        term = h[a] * np.exp(-0.5 * q)
        table[inside] = table[inside] + term[inside]
        state[0] += 1
        state[2] += h[a]
        if log is not None and state[4] < log.shape[0]:
            log[int(state[4])] = np.concatenate([centres[a], np.asarray(sigma, dtype=np.float64), [h[a]]])
            state[4] += 1
    state[3] += 1
    return table, state, log


def cutoff_margin(shape, lower, spacing, periodic, sigma, columns, y, cutoff):
    """The smallest ``|q / c^2 - 1|`` over every entry and every finite centre: how far the nearest grid point is from the cutoff's edge."""
    d = len(shape)
    columns = list(range(d)) if columns is None else list(columns)
    centres = np.asarray(y, dtype=np.float64)[:, columns]
    c2 = float(cutoff) ** 2
    margin = np.inf
    for centre in centres:
        if np.isfinite(centre).all():
            margin = min(margin, float(np.abs(entry_q(shape, lower, spacing, periodic, sigma, centre) / c2 - 1.0).min()))
    return margin
