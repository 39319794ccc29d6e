"""An independent oracle of parallel-bias metadynamics (`molann_value_and_pbmetad_f64`, `molann_pbmetad_deposit_f64`), written from the
formulas of include/molann_hip.h in plain numpy and torch float64: loops over frames, walkers and axes, whole-table arithmetic, no
tiles, no chunks, none of the library's code.

A 1-D table T of n points at lower + i h is interpolated by cubic convolution (Catmull-Rom): with u = (y - lower) / h, i = floor(u) and
t = u - i, V = sum_j T[i - 1 + j] w_j(t).  Periodic: indices modulo n.  Not periodic: u is held to [0, n - 1] (the derivative is 0
outside), i to [0, n - 2] and the indices to [0, n - 1]."""

import math

import numpy as np
import torch


def _weights(t):
    """The four Catmull-Rom weights at t and their derivatives with respect to t."""
    w = [(-t ** 3 + 2 * t ** 2 - t) / 2, (3 * t ** 3 - 5 * t ** 2 + 2) / 2, (-3 * t ** 3 + 4 * t ** 2 + t) / 2, (t ** 3 - t ** 2) / 2]
    dw = [(-3 * t ** 2 + 4 * t - 1) / 2, (9 * t ** 2 - 10 * t) / 2, (-9 * t ** 2 + 8 * t + 1) / 2, (3 * t ** 2 - 2 * t) / 2]
    return w, dw


def axis_cell(y, n, lower, h, periodic):
    """(cell index i, inside) of a finite y: the cell whose stencil the interpolant uses and whether the derivative is live."""
    u = (y - lower) / h
    if periodic:
        u = u - n * math.floor(u / n)
        return min(max(int(math.floor(u)), 0), n - 1), True
    inside = 0.0 <= u <= n - 1
    u = min(max(u, 0.0), n - 1.0)
    return min(int(math.floor(u)), n - 2), inside


def axis_value(y, T, lower, h, periodic):
    """(V, dV/dy) of one table at one y; NaN for a y that is not finite."""
    n = len(T)
    if not math.isfinite(y):
        return math.nan, math.nan
    u = (y - lower) / h
    s = 1.0
    if periodic:
        u = u - n * math.floor(u / n)
        i = min(max(int(math.floor(u)), 0), n - 1)
    else:
        if not u >= 0.0:
            s, u = 0.0, 0.0
        if not u <= n - 1.0:
            s, u = 0.0, n - 1.0
        i = min(int(math.floor(u)), n - 2)
    w, dw = _weights(u - i)
    V = dV = 0.0
    for j in range(4):
        q = i - 1 + j
        q = q % n if periodic else min(max(q, 0), n - 1)
        V += float(T[q]) * w[j]
        dV += float(T[q]) * dw[j] * s / h
    return V, dV


def softmin(V, kT):
    """(V_PB, w) of a list of V_k: NaN where one is not finite."""
    if not all(math.isfinite(v) for v in V):
        return math.nan, [math.nan] * len(V)
    m = min(V)
    e = [math.exp(-(v - m) / kT) for v in V]
    S = sum(e)
    return m - kT * math.log(S), [x / S for x in e]


def split(table, shape):
    offs = np.concatenate([[0], np.cumsum(shape)])
    return [table[offs[k]:offs[k + 1]] for k in range(len(shape))]


def frame(y, table, shape, lower, spacing, periodic, columns, kT, restraint=None):
    """One frame: (energies [2 + K], dy [d_out]).  restraint: None or (center, kappa, period or None, flat or None), rows of d_out."""
    K = len(shape)
    columns = list(range(K)) if columns is None else list(columns)
    periodic = [False] * K if periodic is None else list(periodic)
    T = split(np.asarray(table), shape)
    dy = [0.0] * len(y)
    e_r = 0.0
    if restraint is not None:
        center, kappa, period, flat = restraint
        for k in range(len(y)):
            d = float(y[k]) - float(center[k])
            P = 0.0 if period is None else float(period[k])
            if P > 0.0:
                d = d - P * round(d / P) if math.isfinite(d) else math.nan
            f = 0.0 if flat is None else float(flat[k])
            if f > 0.0:
                d = 0.0 if abs(d) <= f else math.copysign(abs(d) - f, d)
            e_r += 0.5 * float(kappa[k]) * d * d
            dy[k] = float(kappa[k]) * d
    V, dV = [], []
    for k in range(K):
        v, dv = axis_value(float(y[columns[k]]), T[k], lower[k], spacing[k], periodic[k])
        V.append(v)
        dV.append(dv)
    vpb, w = softmin(V, kT)
    for k in range(K):
        dy[columns[k]] += w[k] * dV[k]
    return [e_r, vpb] + V, dy


def torch_bias(y, table, shape, lower, spacing, periodic, columns, kT):
    """V_PB of frames y [N, d_out] as a differentiable torch expression of y: -kT logsumexp(-V / kT) over the K interpolants."""
    K = len(shape)
    columns = list(range(K)) if columns is None else list(columns)
    periodic = [False] * K if periodic is None else list(periodic)
    T = split(table, shape)
    Vs = []
    for k in range(K):
        n, yk = shape[k], y[:, columns[k]]
        u = (yk - lower[k]) / spacing[k]
        if periodic[k]:
            u = u - n * torch.floor(u / n)
            i = torch.clamp(torch.floor(u.detach()), 0, n - 1).long()
        else:
            u = torch.clamp(u, 0.0, n - 1.0)
            i = torch.clamp(torch.floor(u.detach()), max=n - 2).long()
        t = u - i
        w, _ = _weights(t)
        v = 0.0
        for j in range(4):
            q = i - 1 + j
            q = q % n if periodic[k] else torch.clamp(q, 0, n - 1)
            v = v + T[k][q] * w[j]
        Vs.append(v)
    V = torch.stack(Vs, dim=1)
    return -kT * torch.logsumexp(-V / kT, dim=1), V


def heights(V, height0, inv_dT, kT):
    """A walker's K heights from its K biases; None where the walker is invalid by V or by a height."""
    _, w = softmin(list(V), kT)
    out = []
    for k, v in enumerate(V):
        try:
            h = (height0 * math.exp(-(v * inv_dT)) if inv_dT > 0.0 else height0) * w[k]
        except OverflowError:
            return None
        if not math.isfinite(h):
            return None
        out.append(h)
    return out


def axis_q(n, lower, h, periodic, sigma, y):
    """(delta / sigma)^2 at every point of one axis for a hill centred at y."""
    d = lower + np.arange(n) * h - y
    if periodic:
        P = n * h
        d = d - P * np.round(d / P)
    return (d / sigma) ** 2


def deposit(table, shape, lower, spacing, periodic, sigma, columns, y, V, height0, inv_dT, kT, cutoff, state, log=None):
    """One deposit: returns (table, state, log) as new arrays.  y [W, n_out], V [W, K]."""
    K = len(shape)
    columns = list(range(K)) if columns is None else list(columns)
    periodic = [False] * K if periodic is None else list(periodic)
    table, state = np.array(table, dtype=np.float64), np.array(state, dtype=np.float64)
    log = None if log is None else np.array(log, dtype=np.float64)
    T = split(table, shape)
    c2 = math.inf if cutoff is None else cutoff * cutoff
    logged = 0
    if log is not None:
        s4 = state[4]
        logged = int(min(max(s4, 0.0), log.shape[0])) if math.isfinite(s4) or s4 == math.inf else 0
        logged = log.shape[0] if s4 == math.inf else logged
    for a in range(y.shape[0]):
        centre = [float(y[a, columns[k]]) for k in range(K)]
        h = heights([float(v) for v in V[a]], height0, inv_dT, kT)
        if h is None or not all(math.isfinite(c) for c in centre):
            state[1] += 1.0
            continue
        state[0] += 1.0
        for k in range(K):
            state[2] += h[k]
            if h[k] > 0.0:
                q = axis_q(shape[k], lower[k], spacing[k], periodic[k], sigma[k], centre[k])
                inside = q <= c2
                T[k][inside] += h[k] * np.exp(-0.5 * q[inside])      # an entry outside keeps its bits (a -0.0 too)
        if log is not None and logged < log.shape[0]:
            log[logged] = centre + h
            logged += 1
    state[3] += 1.0
    if log is not None:
        state[4] = float(logged)
    return table, state, log
