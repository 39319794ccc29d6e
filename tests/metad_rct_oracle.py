"""The reweighting offset c(t) of a metadynamics table, written from include/molann_hip.h in whole-table numpy at `np.longdouble`: no
chunks, no tree, no order of its own.  `offset` is the quantity, `due` the stride's rule."""

import math

import numpy as np

LD = np.longdouble


def offset(table, kT, inv_dT):
    """dict(c, M, log0, logV, bad) of the flat table: M the largest finite entry, log0 = a0 M + log S0, logV = aV M + log SV and
    c = M + kT (log S0 - log SV); every value NaN but `bad` where an entry is not finite."""
    v = np.asarray(table, dtype=np.float64).reshape(-1)
    finite = np.isfinite(v)
    bad = int((~finite).sum())
    if bad:
        return dict(c=math.nan, M=math.nan, log0=math.nan, logV=math.nan, bad=bad)
    w = v.astype(LD)
    kT, aV = LD(kT), LD(inv_dT)
    a0 = LD(1) / kT + aV
    M = w.max()
    l0 = np.log(np.exp(a0 * (w - M)).sum(dtype=LD))
    lV = np.log(np.exp(aV * (w - M)).sum(dtype=LD))
    return dict(c=M + kT * (l0 - lV), M=M, log0=a0 * M + l0, logV=aV * M + lV, bad=0)


def due(steps, stride):
    """Whether a call with state[3] = steps updates: a count that is not finite or negative reads as 0; then steps mod stride == 0.
    Returns (due, the steps recorded in slot 5)."""
    steps = float(steps)
    if not (math.isfinite(steps) and steps >= 0.0):
        steps = 0.0
    return math.fmod(steps, float(stride)) == 0.0, steps
