"""Tables for `MolANN.value_and_grid`: a bias on a regular grid over the collective variables.  Plain torch - building or updating a
table is plumbing between steps, not a hot path.

A table has one axis per output, output 0 the slowest; grid point i of axis k sits at ``lower[k] + i * spacing[k]``.  A periodic axis
has period ``n_k * spacing[k]`` (so the point after the last is the first again); any other spans
``[lower[k], lower[k] + (n_k - 1) * spacing[k]]``.  A metadynamics run that starts with `MolANN.value_and_hills` moves to the table
with `add_hills_to_grid`: deposit each new hill onto the table and call `value_and_grid`, whose cost does not grow with the run.

An OPES run (`MolANN.value_and_opes`) keeps its own kernel table; `opes_kernel_sum` gives the kernel density at any points - at the
kernel centres for the normalisation Z, at a new sample for the weight of its deposit.  With walls or a table next to it, or on some
of a wider model's outputs, the kernel table goes into `MolANN.value_and_bias` as an `Opes` record."""

import collections
import operator

import torch

__all__ = ["grid_points", "add_hills_to_grid", "opes_kernel_sum", "Restraint", "Hills", "Grid", "Opes"]

HILLS_MAX_COLUMNS = 8     # HILLS_MAX_D of csrc/molann_math.h
GRID_MAX_COLUMNS = 3      # GRID_MAX_D of csrc/molann_math.h


def _columns(name, columns, cap, route):
    """A record's `columns`: None (the first outputs, as many as the term is wide) or a list / tuple / range of distinct output
    indices >= 0 in any order, returned as a tuple of ints.  Anything else: TypeError; a negative or repeated index: IndexError; more
    than `cap`: NotImplementedError naming the route that remains.  The upper end is checked against the model, in `value_and_bias`."""
    if columns is None:
        return None
    if not isinstance(columns, (list, tuple, range)):
        raise TypeError("%s: `columns` must be None or a list, tuple or range of output indices; got %s" % (name, type(columns).__name__))
    cols = []
    for c in columns:
        if isinstance(c, bool):
            raise TypeError("%s: `columns` must hold integers; got a bool" % name)
        try:
            cols.append(operator.index(c))
        except TypeError:
            raise TypeError("%s: `columns` must hold integers; got %s" % (name, type(c).__name__))
    if any(c < 0 for c in cols):
        raise IndexError("%s: `columns` holds output indices >= 0; got %s" % (name, cols))
    if len(set(cols)) != len(cols):
        raise IndexError("%s: `columns` must be distinct; got %s" % (name, cols))
    if not cols:
        raise ValueError("%s: `columns` must name at least one output (leave the term out for none)" % name)
    if len(cols) > cap:
        raise NotImplementedError("%s: the one-launch kernel serves at most %d columns (got %d); %s" % (name, cap, len(cols), route))
    return tuple(cols)


class Restraint(collections.namedtuple("Restraint", "center kappa period flat")):
    """The harmonic restraint of `MolANN.value_and_bias`, on all outputs: `MolANN.value_and_restraint`'s arguments (``kappa[k] = 0``
    leaves output k free).  Immutable; the tensors are held, not copied."""
    __slots__ = ()

    def __new__(cls, center, kappa, period=None, flat=None):
        return super().__new__(cls, center, kappa, period, flat)


class Hills(collections.namedtuple("Hills", "centers heights sigma period columns")):
    """The metadynamics hills of `MolANN.value_and_bias` on the outputs ``columns`` (distinct indices in any order, at most 8; None:
    the first ``centers.shape[1]``): `MolANN.value_and_hills`' arguments, ``centers`` [H, len(columns)], ``sigma`` and ``period``
    laid out over the chosen outputs in the order of the list.  Immutable; the tensors are held, not copied."""
    __slots__ = ()

    def __new__(cls, centers, heights, sigma, period=None, columns=None):
        columns = _columns("Hills", columns, HILLS_MAX_COLUMNS, "form the hill sum and its derivative on `model(x)[:, columns]` with "
                           "torch, scatter it into a cotangent, then `value_and_vjp`")
        return super().__new__(cls, centers, heights, sigma, period, columns)


class Grid(collections.namedtuple("Grid", "table lower spacing periodic columns")):
    """The tabulated bias of `MolANN.value_and_bias` on the outputs ``columns`` (distinct indices in any order, at most 3; None: the
    first ``table.dim()``): `MolANN.value_and_grid`'s arguments, axis 0 of ``table`` (the slowest) being the first listed output.
    Immutable; the table is held, not copied, and read at launch as it is."""
    __slots__ = ()

    def __new__(cls, table, lower, spacing, periodic=None, columns=None):
        columns = _columns("Grid", columns, GRID_MAX_COLUMNS, "interpolate the table and its derivative on `model(x)[:, columns]` with "
                           "torch, scatter it into a cotangent, then `value_and_vjp`")
        return super().__new__(cls, table, lower, spacing, periodic, columns)


class Opes(collections.namedtuple("Opes", "centers heights sigma scale norm epsilon cutoff period columns")):
    """The OPES term of `MolANN.value_and_bias` on the outputs ``columns`` (distinct indices in any order, at most 8; None: the first
    ``centers.shape[1]``): `MolANN.value_and_opes`' arguments, ``centers`` [H, len(columns)], ``sigma`` and ``period`` laid out over the
    chosen outputs in the order of the list; ``scale``, ``norm``, ``epsilon`` Python floats, ``cutoff`` None (no cutoff) or > 0.
    Immutable (a deposit makes a new record: the tensors are held, not copied, and a new ``norm`` costs nothing)."""
    __slots__ = ()

    def __new__(cls, centers, heights, sigma, scale, norm, epsilon, cutoff=None, period=None, columns=None):
        columns = _columns("Opes", columns, HILLS_MAX_COLUMNS, "form the kernel sum on `model(x)[:, columns]` with `opes_kernel_sum`, its "
                           "logarithm and its derivative with torch, scatter it into a cotangent, then `value_and_vjp`")
        return super().__new__(cls, centers, heights, sigma, scale, norm, epsilon, cutoff, period, columns)


def grid_points(shape, lower, spacing, device=None):
    """The grid's coordinates: a tuple of one float64 tensor per axis, ``lower[k] + arange(shape[k]) * spacing[k]``.
    ``torch.meshgrid(*grid_points(...), indexing="ij")`` gives the coordinates of every table entry."""
    shape, lower, spacing = [int(n) for n in shape], [float(v) for v in lower], [float(v) for v in spacing]
    if not (len(shape) == len(lower) == len(spacing)):
        raise ValueError("grid_points: `shape`, `lower` and `spacing` must have one entry per axis; got %d, %d, %d" % (len(shape), len(lower), len(spacing)))
    return tuple(lo + torch.arange(n, dtype=torch.float64, device=device) * h for n, lo, h in zip(shape, lower, spacing))


def add_hills_to_grid(table, lower, spacing, periodic, centers, heights, sigma, chunk=1024):
    """Adds ``sum_h heights_h exp(-1/2 sum_k (d_hk / sigma_hk)^2)`` - `MolANN.value_and_hills`' bias - onto ``table`` in place, at
    every grid point g: ``d_hk = g_k - centers[h, k]``, wrapped to ``d - P rint(d / P)`` with ``P = n_k spacing[k]`` on a periodic
    axis.  ``table``: float64 with 1 to 3 dimensions; ``lower``, ``spacing``: one float per axis; ``periodic``: one bool per axis or
    None; ``centers``: [H, d]; ``heights``: [H] or a float; ``sigma``: a float, [d] or [H, d], > 0.  The Gaussian is a product over
    the axes, so the hills are taken ``chunk`` at a time and the temporaries are ``chunk * n_k`` values per axis, whatever the
    table's size.  Returns ``table``."""
    if not (isinstance(table, torch.Tensor) and table.dtype == torch.float64 and 1 <= table.dim() <= 3):
        raise TypeError("add_hills_to_grid: `table` must be a float64 tensor with 1 to 3 dimensions")
    d = table.dim()
    periodic = [False] * d if periodic is None else [bool(p) for p in periodic]
    points = grid_points(table.shape, lower, spacing, device=table.device)
    if len(periodic) != d or len(points) != d:
        raise ValueError("add_hills_to_grid: `lower`, `spacing` and `periodic` must have one entry per axis of `table` (%d)" % d)
    f64 = dict(dtype=torch.float64, device=table.device)
    centers = torch.as_tensor(centers, **f64).reshape(-1, d)
    n_hills = centers.shape[0]
    heights = torch.as_tensor(heights, **f64).expand(n_hills)
    sigma = torch.as_tensor(sigma, **f64)
    sigma = sigma.expand(n_hills, d) if sigma.dim() < 2 else sigma
    if sigma.shape != (n_hills, d) or not bool((sigma > 0).all()):
        raise ValueError("add_hills_to_grid: `sigma` must be a float, [d] or [H, d] and > 0 everywhere")
    letters = "ijl"[:d]
    equation = "h," + ",".join("h" + c for c in letters) + "->" + letters
    for start in range(0, n_hills, int(chunk)):
        rows = slice(start, start + int(chunk))
        factors = []
        for k in range(d):
            dk = points[k][None, :] - centers[rows, k, None]
            if periodic[k]:
                P = table.shape[k] * float(spacing[k])
                dk = dk - P * torch.round(dk / P)
            s = dk / sigma[rows, k, None]
            factors.append(torch.exp(-0.5 * s * s))
        table += torch.einsum(equation, heights[rows], *factors)
    return table


def opes_kernel_sum(points, centers, heights, sigma, period=None, cutoff=None, chunk=1024):
    """``P[m] = sum_h heights_h K_h(points[m])`` [M], float64, on points' device: `MolANN.value_and_opes`' kernel density before its
    logarithm, ``K_h = exp(-q_h / 2) - exp(-cutoff^2 / 2)`` where ``q_h = sum_k (d_hk / sigma_hk)^2 < cutoff^2`` and 0 elsewhere,
    ``d_hk = points[m, k] - centers[h, k]`` wrapped to ``d - P rint(d / P)`` where ``period[k] > 0``.  What a caller needs between
    steps: the mean of P over the kernel centres updates Z, P at a new sample picks its deposit's weight.  ``points``: [M, d];
    ``centers``: [H, d]; ``heights``: [H] or a float; ``sigma``: a float, [d] or [H, d], > 0; ``period``: None or [d]; ``cutoff``: None
    (no cutoff) or > 0.  The kernels are taken ``chunk`` at a time, so the temporaries are ``M * chunk * d`` values.  Differentiable in
    ``points`` by autograd."""
    points = points.to(torch.float64) if isinstance(points, torch.Tensor) else torch.as_tensor(points, dtype=torch.float64)
    f64 = dict(dtype=torch.float64, device=points.device)
    if points.dim() != 2:
        raise ValueError("opes_kernel_sum: `points` must be [M, d]; got %s" % list(points.shape))
    d = points.shape[1]
    centers = torch.as_tensor(centers, **f64).reshape(-1, d)
    n_kernels = centers.shape[0]
    heights = torch.as_tensor(heights, **f64).expand(n_kernels)
    sigma = torch.as_tensor(sigma, **f64)
    sigma = sigma.expand(n_kernels, d) if sigma.dim() < 2 else sigma
    if sigma.shape != (n_kernels, d) or not bool((sigma > 0).all()):
        raise ValueError("opes_kernel_sum: `sigma` must be a float, [d] or [H, d] and > 0 everywhere")
    if cutoff is not None and not float(cutoff) > 0.0:
        raise ValueError("opes_kernel_sum: `cutoff` must be None or > 0; got %r" % (cutoff,))
    c2 = float("inf") if cutoff is None else float(cutoff) ** 2
    c0 = torch.exp(torch.tensor(-0.5 * c2, **f64))
    if period is not None:
        period = torch.as_tensor(period, **f64).reshape(d)
        periodic = period > 0
        p_safe = torch.where(periodic, period, torch.ones_like(period))
    total = torch.zeros(points.shape[0], **f64)
    for start in range(0, n_kernels, int(chunk)):
        rows = slice(start, start + int(chunk))
        dd = points[:, None, :] - centers[None, rows, :]
        if period is not None:
            dd = torch.where(periodic, dd - p_safe * torch.round(dd / p_safe), dd)
        s = dd / sigma[None, rows, :]
        q = (s * s).sum(dim=2)
        kernel = torch.where(q >= c2, torch.zeros_like(q), torch.exp(-0.5 * q) - c0)
        total = total + (heights[rows] * kernel).sum(dim=1)
    return total
