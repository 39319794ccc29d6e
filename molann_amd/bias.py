"""Tables for `MolANN.value_and_grid`: a bias on a regular grid over the collective variables.  Plain torch - building or updating a
table is plumbing between steps, not a hot path.

A table has one axis per output, output 0 the slowest; grid point i of axis k sits at ``lower[k] + i * spacing[k]``.  A periodic axis
has period ``n_k * spacing[k]`` (so the point after the last is the first again); any other spans
``[lower[k], lower[k] + (n_k - 1) * spacing[k]]``.  A metadynamics run that starts with `MolANN.value_and_hills` moves to the table
with `add_hills_to_grid`: deposit each new hill onto the table and call `value_and_grid`, whose cost does not grow with the run.

An OPES run (`MolANN.value_and_opes`) keeps its kernel table on the device in an `OpesTable`: `deposit` compresses new kernels into it and
keeps the sum its normalisation Z is formed from, in one launch and with no read-back; `kernel_sum` gives the kernel density at any
points; `record` hands the live rows to `value_and_opes` / `value_and_bias` as an `Opes` record.  `opes_kernel_sum` is the same density
in plain torch, differentiable by autograd.  An `OpesRun` is the whole loop on the device: `bias` evaluates the model and the bias from the
table's state (`MolANN.value_and_opes_table`), `deposit` turns those outputs into the step's kernels and deposits them - two launches
per step, nothing read back, capturable in a graph.  With walls or a table next to it, or on some of a wider model's outputs, the kernel table
goes into `MolANN.value_and_bias` as an `OpesFromTable` record, whose kernel reads the table's state on the device as well -
`OpesRun(columns=, walls=, grid=)` is that loop, still two launches per step - or, with the live count and the norm at hand on the host,
as an `Opes` record.  `OpesRun(sigma0="adaptive")` measures the kernels' widths from the run itself, per walker, in state that stays on
the device, and `OpesRun(explore=True)` is the explore variant: the same two launches per step.

A metadynamics run on a table is a `MetadRun`, the same loop for hills: `bias` is `value_and_grid` (or `value_and_bias` with walls or on
some of a wider model's outputs) on the table as it is, `deposit` adds the step's hills to the table on the device with well-tempered
heights formed from that call's bias (`molann_metad_deposit_f64`) - two launches per step, nothing read back, capturable in a graph -
and `hills` gives the deposited hills back as a `Hills` record; with `rct_stride` the run also keeps the reweighting offset c(t) on the
device (`molann_metad_rct_f64`, two more launches on the steps that update it).  `add_hills_to_grid` stays the way to build a table from hills at hand.
`MetadRun(adaptive="diff")` and `MetadRun(adaptive="geom")` deposit adaptive, correlated hills - multivariate Gaussians whose covariance
is measured from each walker's recent motion, or formed from the metric J J^T of `value_and_metric` - with the running statistics on the
device (`molann_metad_widths_f64`, `molann_metad_deposit_cov_f64`); `cov_hills` gives them back as a `CovHills` record and
`add_cov_hills_to_grid` is their plain-torch route onto a table."""

import collections
import math
import operator

import torch

__all__ = ["grid_points", "add_hills_to_grid", "opes_kernel_sum", "Restraint", "Hills", "Grid", "Opes", "OpesTable", "OpesFromTable", "OpesRun",
           "MetadRun", "CovHills", "add_cov_hills_to_grid", "PBTables", "PBMetadRun"]

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


class PBTables(collections.namedtuple("PBTables", "table shape lower spacing periodic columns")):
    """The K one-dimensional tables of a parallel-bias metadynamics bias (`MolANN.value_and_pbmetad`) on the outputs ``columns`` (distinct
    indices in any order, at most 8; None: the first K): ``table`` a float64 tensor of ``sum(shape)`` values, table k - ``shape[k]`` >= 4
    points at ``lower[k] + i spacing[k]``, periodic with period ``shape[k] spacing[k]`` where ``periodic[k]`` - starting at
    ``sum(shape[:k])``.  Immutable; the table is held, not copied, and read at launch as it is."""
    __slots__ = ()

    def __new__(cls, table, shape, lower, spacing, periodic=None, columns=None):
        columns = _columns("PBTables", columns, HILLS_MAX_COLUMNS, "a parallel bias has at most 8 axes")
        if isinstance(shape, torch.Tensor):
            shape = shape.tolist()
        try:
            shape = tuple(operator.index(n) for n in shape)
        except TypeError:
            raise TypeError("PBTables: `shape` must be a sequence of integers, one per table; got %s" % type(shape).__name__)
        K = len(shape)
        if not 1 <= K <= HILLS_MAX_COLUMNS:
            raise (ValueError if K < 1 else NotImplementedError)("PBTables: 1 to %d tables are served; got %d" % (HILLS_MAX_COLUMNS, K))
        if min(shape) < 4 or sum(shape) >= 2 ** 31:
            raise ValueError("PBTables: every table needs at least 4 points and all of them fewer than 2^31; got %s" % list(shape))
        rows = []
        for what, v in (("lower", lower), ("spacing", spacing)):
            try:
                v = tuple(float(c) for c in (v.tolist() if isinstance(v, torch.Tensor) else v))
            except (TypeError, ValueError):
                raise TypeError("PBTables: `%s` must be a sequence of %d numbers; got %s" % (what, K, type(v).__name__))
            if len(v) != K:
                raise ValueError("PBTables: `%s` must have one entry per table (%d); got %d" % (what, K, len(v)))
            if not all(math.isfinite(c) and (c > 0.0 or what == "lower") for c in v):
                raise ValueError("PBTables: `%s` must be finite%s everywhere; got %s" % (what, "" if what == "lower" else " and > 0", list(v)))
            rows.append(v)
        if periodic is not None:
            periodic = tuple(bool(p) for p in periodic)
            if len(periodic) != K:
                raise ValueError("PBTables: `periodic` must be None or one bool per table (%d); got %d" % (K, len(periodic)))
        if columns is not None and len(columns) != K:
            raise ValueError("PBTables: `columns` must name one output per table (%d); got %d" % (K, len(columns)))
        if not isinstance(table, torch.Tensor):
            raise TypeError("PBTables: `table` must be a tensor; got %s" % type(table).__name__)
        if table.dtype != torch.float64:
            raise TypeError("PBTables: `table` must be float64; got %s" % table.dtype)
        if table.dim() != 1 or table.numel() != sum(shape) or not table.is_contiguous():
            raise ValueError("PBTables: `table` must be contiguous [sum(shape) = %d]; got %s" % (sum(shape), list(table.shape)))
        return super().__new__(cls, table, shape, rows[0], rows[1], periodic, columns)

    def views(self):
        """The K tables as views of ``table``, nothing copied."""
        return tuple(self.table[sum(self.shape[:k]):sum(self.shape[:k + 1])] for k in range(len(self.shape)))


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


class CovHills(collections.namedtuple("CovHills", "centers covariances heights period columns")):
    """The hills of an adaptive `MetadRun`: ``centers`` [H, d], ``covariances`` [H, d (d + 1) / 2] - each the row-major upper triangle
    of the hill's covariance matrix (``c00 c01 c02 c11 c12 c22`` for d = 3) - ``heights`` [H], ``period`` [d] or None and the outputs
    ``columns`` the axes are (None: the first d).  Immutable; the tensors are held, not copied."""
    __slots__ = ()

    def __new__(cls, centers, covariances, heights, period=None, columns=None):
        columns = _columns("CovHills", columns, GRID_MAX_COLUMNS, "a table has at most 3 axes")
        return super().__new__(cls, centers, covariances, heights, period, columns)


def add_cov_hills_to_grid(table, lower, spacing, periodic, centers, covariances, heights, cutoff=None, chunk=8):
    """Adds ``sum_h heights_h exp(-1/2 d_h^T C_h^-1 d_h)`` onto ``table`` in place, at every grid point g within ``cutoff`` (None:
    everywhere; else where ``d^T C^-1 d <= cutoff^2``): ``d_hk = g_k - centers[h, k]``, wrapped to ``d - P rint(d / P)`` with
    ``P = n_k spacing[k]`` on a periodic axis, ``C_h`` the symmetric matrix whose row-major upper triangle is ``covariances[h]``
    [d (d + 1) / 2].  Plain torch on the table's device - the restart route of an adaptive `MetadRun` (`MetadRun.cov_hills`) and an
    independent restatement of `molann_metad_deposit_cov_f64`: the inverse is `torch.linalg.inv`'s.  A hill is not a product over the
    axes, so the temporaries are ``chunk`` tables.  Returns ``table``."""
    if not (isinstance(table, torch.Tensor) and table.dtype == torch.float64 and 1 <= table.dim() <= 3):
        raise TypeError("add_cov_hills_to_grid: `table` must be a float64 tensor with 1 to 3 dimensions")
    d = table.dim()
    periodic = [False] * d if periodic is None else [bool(p) for p in periodic]
    points = grid_points(table.shape, lower, spacing, device=table.device)
    if len(periodic) != d or len(points) != d:
        raise ValueError("add_cov_hills_to_grid: `lower`, `spacing` and `periodic` must have one entry per axis of `table` (%d)" % d)
    f64 = dict(dtype=torch.float64, device=table.device)
    centers = torch.as_tensor(centers, **f64).reshape(-1, d)
    n_hills, T = centers.shape[0], d * (d + 1) // 2
    heights = torch.as_tensor(heights, **f64).expand(n_hills)
    covariances = torch.as_tensor(covariances, **f64)
    if covariances.shape != (n_hills, T):
        raise ValueError("add_cov_hills_to_grid: `covariances` must be [H, %d], the upper triangles; got %s" % (T, list(covariances.shape)))
    if cutoff is not None and not float(cutoff) > 0.0:
        raise ValueError("add_cov_hills_to_grid: `cutoff` must be None or > 0; got %r" % (cutoff,))
    full = torch.zeros(n_hills, d, d, **f64)
    at = 0
    for i in range(d):
        for j in range(i, d):
            full[:, i, j] = covariances[:, at]
            full[:, j, i] = covariances[:, at]
            at += 1
    inverse = torch.linalg.inv(full) if n_hills else full
    for start in range(0, n_hills, int(chunk)):
        rows = slice(start, start + int(chunk))
        deltas = []
        for k in range(d):
            dk = points[k][None, :] - centers[rows, k, None]
            if periodic[k]:
                P = table.shape[k] * float(spacing[k])
                dk = dk - P * torch.round(dk / P)
            view = [dk.shape[0]] + [1] * d
            view[1 + k] = table.shape[k]
            deltas.append(dk.reshape(view))
        q = torch.zeros((deltas[0].shape[0],) + tuple(table.shape), **f64)
        for i in range(d):
            for j in range(d):
                q = q + inverse[rows, i, j].reshape([-1] + [1] * d) * deltas[i] * deltas[j]
        term = heights[rows].reshape([-1] + [1] * d) * torch.exp(-0.5 * q)
        if cutoff is not None:
            term = torch.where(q <= float(cutoff) ** 2, term, torch.zeros_like(term))
        table += term.sum(dim=0)
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


class OpesTable(object):
    """The kernel table of an OPES run in device memory, updated in place by one launch per deposit (`molann_opes_deposit_f64`).

    ``centers`` [capacity, d], ``sigma`` [capacity, d] and ``heights`` [capacity] hold the kernels, rows ``>= n`` are dead storage;
    ``state`` [4] holds ``(n, S, merges, refused)`` with ``S = sum_{i<n} sum_{j<n} heights_j K_j(centers_i)``, the sum OPES normalises
    with (``Z = S / (n * kde_norm)``, so the ``norm`` of `value_and_opes` is ``S / n``; `MolANN.value_and_opes_table` reads it from
    here on the device, and `OpesRun` keeps ``neff`` and the bandwidth rescaling there too).
    ``period``: None or [d] (> 0: that output is periodic); ``cutoff``: None (no cutoff) or > 0, in widths; ``threshold``: a new kernel
    closer than this many widths to a live one is merged into it (0: every kernel is appended).  1 <= d <= 8; a CUDA / HIP device."""

    def __init__(self, capacity, d, device, period=None, cutoff=None, threshold=1.0):
        if isinstance(capacity, bool) or isinstance(d, bool):
            raise TypeError("OpesTable: `capacity` and `d` must be integers")
        capacity, d = operator.index(capacity), operator.index(d)
        if capacity < 1:
            raise ValueError("OpesTable: `capacity` must be >= 1; got %d" % capacity)
        if not 1 <= d <= HILLS_MAX_COLUMNS:
            raise ValueError("OpesTable: `d` must be 1..%d (the one-launch kernels' widest kernel); got %d" % (HILLS_MAX_COLUMNS, d))
        threshold = float(threshold)
        if not (math.isfinite(threshold) and threshold >= 0.0):
            raise ValueError("OpesTable: `threshold` must be finite and >= 0; got %r" % (threshold,))
        if cutoff is not None and not float(cutoff) > 0.0:
            raise ValueError("OpesTable: `cutoff` must be None or > 0; got %r" % (cutoff,))
        device = torch.device(device)
        if device.type != "cuda":
            raise ValueError("OpesTable: the table lives in device memory and its kernels are HIP kernels; got device %s" % device)
        f64 = dict(dtype=torch.float64, device=device)
        if period is not None:
            period = torch.as_tensor(period, **f64)
            if period.shape != (d,):
                raise ValueError("OpesTable: `period` must be None or [%d]; got %s" % (d, list(period.shape)))
            period = period.contiguous()
        self.capacity, self.d, self.device = capacity, d, device
        self.period, self.cutoff, self.threshold = period, None if cutoff is None else float(cutoff), threshold
        self.centers = torch.zeros(capacity, d, **f64)
        self.sigma = torch.zeros(capacity, d, **f64)
        self.heights = torch.zeros(capacity, **f64)
        self.state = torch.zeros(4, **f64)

    def _tensor(self, name, value, shape, what):
        if not isinstance(value, torch.Tensor):
            raise TypeError("OpesTable.%s must be a tensor on %s; got %s" % (name, self.device, type(value).__name__))
        if value.dtype != torch.float64:
            raise TypeError("OpesTable.%s must be float64; got %s" % (name, value.dtype))
        if value.device != self.centers.device or tuple(value.shape) not in shape:
            raise ValueError("OpesTable.%s must be %s on %s; got %s on %s" % (name, what, self.centers.device, list(value.shape), value.device))
        return value.detach()

    def deposit(self, centers, sigma, heights):
        """Compress the new kernels ``centers`` [W, d], ``sigma`` [W, d] or [d], ``heights`` [W] or a float into the table, in order:
        one launch on the current stream, nothing read back, returns None - the tensors may come from torch arithmetic on
        `value_and_opes`' outputs, and deposits may be queued back to back.  A kernel that is not finite, or whose widths or height
        are not > 0, is counted in ``refused`` and changes nothing else; so is a kernel that finds the table full."""
        from . import _capi
        if not (isinstance(centers, torch.Tensor) and centers.dim() == 2):
            raise ValueError("OpesTable.deposit: `centers` must be a [W, %d] tensor" % self.d)
        n_new = centers.shape[0]
        centers = self._tensor("deposit: `centers`", centers, [(n_new, self.d)], "[W, %d]" % self.d).contiguous()
        sigma = self._tensor("deposit: `sigma`", sigma, [(n_new, self.d), (self.d,)], "[W, %d] or [%d]" % (self.d, self.d))
        sigma = sigma.expand(n_new, self.d).contiguous()
        if isinstance(heights, torch.Tensor):
            heights = self._tensor("deposit: `heights`", heights, [(n_new,), ()], "[W] or a scalar").expand(n_new).contiguous()
        else:
            heights = torch.full((n_new,), float(heights), dtype=torch.float64, device=self.centers.device)
        if n_new == 0:
            return None
        with torch.cuda.device(self.centers.device):
            _capi.opes_deposit_f64(self.centers, self.sigma, self.heights, self.state, self.period, centers, sigma, heights, self.threshold,
                                   self.cutoff)
        return None

    def read_state(self):
        """``(n, S, merges, refused)`` as Python numbers: the one 32-byte read-back (it waits for the deposits queued before it)."""
        n, total, merges, refused = self.state.tolist()
        return int(n), total, int(merges), int(refused)

    def kernel_sum(self, points, with_grad=False, n=None):
        """``P[m] = sum_h heights_h K_h(points[m])`` [M] over the live rows, and with ``with_grad`` ``(P, dP)`` with dP [M, d]: one launch
        (`molann_opes_kernel_sum_f64`, the bias kernels' walk).  ``n``: the live count where the caller has it; None reads the state."""
        from . import _capi
        n = self.read_state()[0] if n is None else operator.index(n)
        if not (isinstance(points, torch.Tensor) and points.dim() == 2):
            raise ValueError("OpesTable.kernel_sum: `points` must be a [M, %d] tensor" % self.d)
        points = self._tensor("kernel_sum: `points`", points, [(points.shape[0], self.d)], "[M, %d]" % self.d).contiguous()
        out = torch.empty(points.shape[0], dtype=torch.float64, device=points.device)
        grad = torch.empty(points.shape[0], self.d, dtype=torch.float64, device=points.device) if with_grad else None
        if points.shape[0] == 0:
            return (out, grad) if with_grad else out
        with torch.cuda.device(points.device):
            return _capi.opes_kernel_sum_f64(points, self.centers[:n], self.heights[:n], self.sigma[:n], self.period, self.cutoff, out, grad)

    def recompute_sum(self, n=None):
        """S from scratch, ``kernel_sum(centers[:n]).sum()``, written into ``state[1]`` (a restart, a table the caller edited, a check on
        the incremental sum).  Returns the sum as a tensor on the device."""
        n = self.read_state()[0] if n is None else operator.index(n)
        total = self.kernel_sum(self.centers[:n], n=n).sum()
        self.state[1] = total
        return total

    def record(self, scale, norm, epsilon, columns=None, n=None):
        """The `Opes` record of the live rows - contiguous views ``[:n]``, nothing copied - for `value_and_opes` (unpack its fields)
        and `value_and_bias(opes=...)`.  ``n``: the live count where the caller has it; None reads the state."""
        n = self.read_state()[0] if n is None else operator.index(n)
        return Opes(self.centers[:n], self.heights[:n], self.sigma[:n], scale, norm, epsilon, self.cutoff, self.period, columns)


class OpesFromTable(collections.namedtuple("OpesFromTable", "table scale epsilon columns")):
    """The OPES term of `MolANN.value_and_bias` read from an `OpesTable` where it lives: the kernel forms the live count and the
    normalisation ``S / n`` from ``table.state`` in device memory (`molann_value_and_bias_opes_table_f64`), so nothing is read back and
    the launch can be captured in a graph while the table grows - where `OpesTable.record` needs ``n`` and ``norm`` on the host.  The
    kernels act on the outputs ``columns`` (``table.d`` distinct indices in any order; None: the first ``table.d``); ``scale``,
    ``epsilon`` Python floats; the table's ``cutoff`` and ``period`` are used.  Immutable; the table is held, not copied."""
    __slots__ = ()

    def __new__(cls, table, scale, epsilon, columns=None):
        if not isinstance(table, OpesTable):
            raise TypeError("OpesFromTable: `table` must be an OpesTable; got %s" % type(table).__name__)
        columns = _columns("OpesFromTable", columns, HILLS_MAX_COLUMNS, "form the kernel sum on `model(x)[:, columns]` with `opes_kernel_sum`, "
                           "its logarithm and its derivative with torch, scatter it into a cotangent, then `value_and_vjp`")
        if columns is not None and len(columns) != table.d:
            raise ValueError("OpesFromTable: `columns` must name one output per column of `table` (%d); got %d" % (table.d, len(columns)))
        return super().__new__(cls, table, scale, epsilon, columns)


def _positive(name, what, v, allow_inf=False):
    """A scalar of OpesRun's constructor: a Python number (TypeError), finite - or +inf where allowed - and > 0 (ValueError)."""
    if isinstance(v, bool) or not isinstance(v, (int, float)):
        raise TypeError("%s: `%s` must be a Python float; got %s" % (name, what, type(v).__name__))
    v = float(v)
    if not (v > 0.0 and (math.isfinite(v) or (allow_inf and v == math.inf))):
        raise ValueError("%s: `%s` must be %s and > 0; got %r" % (name, what, "finite or +inf" if allow_inf else "finite", v))
    return v


def _count(name, what, v):
    """An argument that is an integer >= 1, as an int."""
    if isinstance(v, bool):
        raise TypeError("%s: `%s` must be an integer" % (name, what))
    try:
        v = operator.index(v)
    except TypeError:
        raise TypeError("%s: `%s` must be an integer; got %s" % (name, what, type(v).__name__))
    if v < 1:
        raise ValueError("%s: `%s` must be >= 1; got %d" % (name, what, v))
    return v


class OpesRun(object):
    """A whole OPES run (PLUMED's ``OPES_METAD``, with a fixed or an adaptive ``sigma0``, and its explore variant) on the device: two
    launches per step and nothing read back, so the loop queues ahead of the device and can be captured in one ``torch.cuda.graph``.

    ``bias(x)`` is `MolANN.value_and_opes_table` on the table's current state; ``deposit(y, bias)`` is `molann_opes_step_f64` on the
    outputs that call wrote: per walker ``w = exp(bias / kT)``, the running sums ``counter``, ``sum_w``, ``sum_w2``,
    ``neff = (1 + sum_w)^2 / (1 + sum_w2)``, ``rct = kT log(sum_w / counter)``, the widths ``sigma0 * sigma_scale`` with
    ``sigma_scale = (neff (d + 2) / 4)^(-1 / (d + 4))`` (1 with ``fixed_sigma``) held above ``sigma_min``, the heights
    ``w prod_k(sigma0_k / sigma_k)``, and the deposit of the W kernels into ``table`` as `OpesTable.deposit` makes it.  ``run`` [8] on
    the table's device holds ``(counter, sum_w, sum_w2, neff, sigma_scale, rct, observations, started)``, the last two 0 unless the
    run is adaptive.

    With ``columns``, ``walls`` or ``grid`` the run has `MetadRun`'s surface: ``bias(x)`` is `MolANN.value_and_bias` with
    ``restraint=walls, grid=grid, opes=OpesFromTable(table, scale, epsilon, columns)`` (frames_value_bias_opes_table_f64_kernel: the
    state is read on the device there too) and returns ``(y, energies, dx)``, and ``deposit(y, energies)`` is
    `molann_opes_step_columns_f64`, which reads the walkers' centres at ``y[:, columns]`` and their OPES bias at ``energies[:, 3]`` where
    they are - the weights use that bias alone, not the walls or the grid.  Still two launches per step, nothing read back, one graph.
    With all three None nothing changes, bit for bit.

    ``sigma0="adaptive"`` (``SIGMA=ADAPTIVE``, OPES_METAD's default: nobody knows the spread of a learned variable in advance) measures
    the widths from the run, per walker, and needs ``adaptive_stride`` >= 2 and ``walkers`` >= 1.  ``adapt`` [walkers, 3, d] on the
    table's device holds each walker's ``(mean, M2, sigma0)`` and is allocated here, once.  Every ``deposit`` and every ``observe(y)``
    - the call for the MD steps between two deposits, one launch, nothing read back - adds an observation: ``c = observations + 1``,
    ``tau = min(c, adaptive_stride)``, ``diff = y - mean`` (the shorter way round a periodic output), ``mean += diff / tau``,
    ``M2 += diff (y - mean)``; a walker with an output that is not finite keeps its row.  A ``deposit`` before ``adaptive_stride``
    observations have passed stops there and deposits nothing.  The first deposit after them multiplies ``M2`` by ``biasfactor`` (the
    samples so far were unbiased, the later ones come from the flattened distribution) and fixes ``sigma0 = sqrt(M2 / c / biasfactor)``,
    held above ``sigma_min``; from then on walker a's kernel has the widths ``sqrt(M2_a / c / biasfactor) sigma_scale`` held above
    ``sigma_min`` and the height ``w_a prod_k(sigma0_ak / sigma_ak)``.  A walker that never moved has a width of 0 and its kernels are
    refused: ``sigma_min`` is the cure.  Both modes run on `molann_opes_step_modes_f64`.

    ``explore=True`` is ``OPES_METAD_EXPLORE``, what to reach for while the variable is still poor: the table estimates the
    well-tempered distribution itself, so every kernel weighs 1 (times the widths' ratio), ``sigma_scale`` is formed from ``counter``
    instead of ``neff``, ``scale = kT (biasfactor - 1)`` and ``epsilon = exp(-barrier / scale)``.  A numeric ``sigma0`` is the width of
    the unbiased distribution, as without explore: the run stores and uses ``sigma0 sqrt(biasfactor)``, the explore target being
    broader by that factor; an adaptive run measures the target's width directly (no division by ``biasfactor``).  Each of the two
    modes needs a finite ``biasfactor``.  ``columns``, ``walls`` and ``grid`` work with both.

    ``model``: a `MolANN` (or `PreprocessingANN`) whose outputs are the table's ``d`` columns, or a wider one with ``columns``: the
    ``table.d`` outputs the kernels act on, distinct, in any order; ``walls``: a `Restraint` on all outputs or None; ``grid``: a `Grid`
    (a static table from an earlier run, on its own columns) or None; ``table``: an `OpesTable` (its
    ``period``, ``cutoff`` and ``threshold`` are used); ``kT`` > 0; ``biasfactor`` > 1 (+inf: ``scale = kT``); ``barrier`` > 0:
    ``scale = kT (1 - 1 / biasfactor)``, ``epsilon = exp(-barrier / scale)``, ``beta = 1 / kT``.  ``sigma0``, ``sigma_min``: [d]
    numbers or tensors, finite and > 0 (checked here, once: on the device a width that is not > 0 makes every kernel of a step
    invalid and refused).  A walker whose bias or outputs are not finite is counted in the table's ``refused`` and changes nothing
    else.  Out of scope: walkers on several ranks, float32, a step on more than one block, a TorchScript operator for the two modes,
    PLUMED's restart files, a `GraphedForces` wrapper."""

    def __init__(self, model, table, kT, biasfactor, barrier, sigma0, sigma_min=None, fixed_sigma=False, columns=None, walls=None, grid=None,
                 adaptive_stride=None, walkers=None, explore=False):
        from . import _capi
        if not callable(getattr(model, "value_and_opes_table", None)):
            raise TypeError("OpesRun: `model` must be a MolANN or a PreprocessingANN (it has no `value_and_opes_table`); got %s"
                            % type(model).__name__)
        if not (columns is None and walls is None and grid is None) and not callable(getattr(model, "value_and_bias", None)):
            raise TypeError("OpesRun: with `columns`, `walls` or `grid` the `model` must be a MolANN or a PreprocessingANN (it has no "
                            "`value_and_bias`); got %s" % type(model).__name__)
        if not isinstance(table, OpesTable):
            raise TypeError("OpesRun: `table` must be an OpesTable; got %s" % type(table).__name__)
        columns = _columns("OpesRun", columns, HILLS_MAX_COLUMNS, "a kernel table has at most 8 columns")
        if columns is not None and len(columns) != table.d:
            raise ValueError("OpesRun: `columns` must name one output per column of `table` (%d); got %d" % (table.d, len(columns)))
        if walls is not None and not isinstance(walls, Restraint):
            raise TypeError("OpesRun: `walls` must be a Restraint or None; got %s" % type(walls).__name__)
        if grid is not None and not isinstance(grid, Grid):
            raise TypeError("OpesRun: `grid` must be a Grid or None; got %s" % type(grid).__name__)
        kT = _positive("OpesRun", "kT", kT)
        biasfactor = _positive("OpesRun", "biasfactor", biasfactor, allow_inf=True)
        barrier = _positive("OpesRun", "barrier", barrier)
        if not biasfactor > 1.0:
            raise ValueError("OpesRun: `biasfactor` must be > 1; got %r" % (biasfactor,))
        if not isinstance(fixed_sigma, (bool, int)):
            raise TypeError("OpesRun: `fixed_sigma` must be a bool; got %s" % type(fixed_sigma).__name__)
        if not isinstance(explore, (bool, int)):
            raise TypeError("OpesRun: `explore` must be a bool; got %s" % type(explore).__name__)
        adaptive, explore = isinstance(sigma0, str) and sigma0 == "adaptive", bool(explore)
        if (adaptive or explore) and not math.isfinite(biasfactor):
            raise ValueError("OpesRun: `biasfactor` must be finite with `sigma0=\"adaptive\"` and with `explore`; got %r" % (biasfactor,))
        for what, v in (("adaptive_stride", adaptive_stride), ("walkers", walkers)):
            if v is None and not adaptive:
                continue
            if v is None:
                raise TypeError("OpesRun: `sigma0=\"adaptive\"` needs `%s`, an integer" % what)
            if isinstance(v, bool):
                raise TypeError("OpesRun: `%s` must be an integer; got a bool" % what)
            try:
                v = operator.index(v)
            except TypeError:
                raise TypeError("OpesRun: `%s` must be an integer; got %s" % (what, type(v).__name__))
            if adaptive and v < (2 if what == "adaptive_stride" else 1):
                raise ValueError("OpesRun: `%s` must be >= %d; got %d" % (what, 2 if what == "adaptive_stride" else 1, v))
        scale = kT * (biasfactor - 1.0) if explore else kT * (1.0 - 1.0 / biasfactor)
        epsilon = math.exp(-barrier / scale)
        if not epsilon > 0.0:
            raise ValueError("OpesRun: exp(-barrier / (kT (%s))) underflows to 0 for barrier %r; lower the barrier"
                             % ("biasfactor - 1" if explore else "1 - 1 / biasfactor", barrier))
        rows = []
        for what, v in (("sigma0", sigma0), ("sigma_min", sigma_min)):
            if (v is None and what == "sigma_min") or (adaptive and what == "sigma0"):
                rows.append(None)
                continue
            try:
                host = v.detach().to(device="cpu", dtype=torch.float64) if isinstance(v, torch.Tensor) else torch.as_tensor(v, dtype=torch.float64)
            except (TypeError, ValueError, RuntimeError):
                raise TypeError("OpesRun: `%s` must be a tensor or a sequence of %d numbers; got %s" % (what, table.d, type(v).__name__))
            if host.shape != (table.d,):
                raise ValueError("OpesRun: `%s` must be [%d]; got %s" % (what, table.d, list(host.shape)))
            if not bool((torch.isfinite(host) & (host > 0)).all()):
                raise ValueError("OpesRun: `%s` holds widths and must be finite and > 0 everywhere" % what)
            rows.append(host)
        for what, v in (("adaptive_stride", adaptive_stride), ("walkers", walkers)):
            if v is not None and not adaptive:
                raise ValueError("OpesRun: `%s` belongs to `sigma0=\"adaptive\"`; leave it None with given widths" % what)
        self.model, self.table = model, table
        self.kT, self.biasfactor, self.barrier, self.fixed_sigma = kT, biasfactor, barrier, bool(fixed_sigma)
        self.scale, self.epsilon, self.beta = scale, epsilon, 1.0 / kT
        if explore and not adaptive:
            rows[0] = rows[0] * math.sqrt(biasfactor)       # the widths given are the unbiased ones; the explore target is broader
        self.adaptive, self.explore = adaptive, explore
        self.adaptive_stride = operator.index(adaptive_stride) if adaptive else 0
        self.walkers = operator.index(walkers) if adaptive else None
        self.sigma0 = None if adaptive else rows[0].to(table.centers.device).contiguous()
        self.sigma_min = None if rows[1] is None else rows[1].to(table.centers.device).contiguous()
        self.run = torch.zeros(8, dtype=torch.float64, device=table.centers.device)
        self.adapt = torch.zeros(self.walkers, 3, table.d, dtype=torch.float64, device=table.centers.device) if adaptive else None
        self.columns, self.walls, self.grid = columns, walls, grid
        self._plain = columns is None and walls is None and grid is None
        self._opes = OpesFromTable(table, scale, epsilon, columns)
        self._column_array = None if columns is None else _capi._i32_array(columns)

    def bias(self, x, into=None):
        """The walkers ``x`` under the table as it is now, one launch: ``(y, bias, dx)`` of `MolANN.value_and_opes_table`, or - with
        walls, a grid or columns - ``(y, energies, dx)`` of `MolANN.value_and_bias`, ``energies[:, 3]`` the OPES bias."""
        if self._plain:
            return self.model.value_and_opes_table(x, self.table, self.scale, self.epsilon, into=into)
        return self.model.value_and_bias(x, restraint=self.walls, grid=self.grid, opes=self._opes, into=into)

    def deposit(self, y, bias):
        """The step after `bias`, as that call returned them (read only): ``y`` [W, d] and ``bias`` [W]; with walls, a grid or columns
        ``y`` [W, n_out] and ``bias`` [W] or the ``energies`` [W, 4], whose column 3 - the OPES bias alone, without the walls and the
        grid, as OPES_METAD forms its weights - is read in place.  One launch on the current stream, nothing read back, returns None.  In
        an adaptive run ``y`` has ``walkers`` rows, the call is an observation as well, and before ``adaptive_stride`` of them have
        passed it deposits nothing."""
        from . import _capi
        t = self.table
        if self.adaptive or self.explore:
            return self._step_modes("deposit", y, bias, False)
        if not self._plain:
            return self._deposit_columns(y, bias)
        if not (isinstance(y, torch.Tensor) and y.dim() == 2):
            raise ValueError("OpesRun.deposit: `y` must be a [W, %d] tensor" % t.d)
        n_walkers = y.shape[0]
        y = t._tensor("deposit: `y`", y, [(n_walkers, t.d)], "[W, %d]" % t.d).contiguous()
        bias = t._tensor("deposit: `bias`", bias, [(n_walkers,)], "[W]").contiguous()
        if n_walkers == 0:
            return None
        with torch.cuda.device(t.centers.device):
            _capi.opes_step_f64(t.centers, t.sigma, t.heights, t.state, self.run, t.period, y, bias, self.sigma0, self.sigma_min, self.beta,
                                t.threshold, t.cutoff, self.fixed_sigma)
        return None

    def _deposit_columns(self, y, bias):
        """`deposit` of a run with walls, a grid or columns: `molann_opes_step_columns_f64` on the strided outputs."""
        from . import _capi
        t = self.table
        widest = t.d - 1 if self.columns is None else max(self.columns)
        for what, v in (("y", y), ("bias", bias)):
            if not isinstance(v, torch.Tensor):
                raise TypeError("OpesRun.deposit: `%s` must be a tensor on %s; got %s" % (what, t.centers.device, type(v).__name__))
            if v.dtype != torch.float64:
                raise TypeError("OpesRun.deposit: `%s` must be float64; got %s" % (what, v.dtype))
            if v.device != t.centers.device:
                raise ValueError("OpesRun.deposit: `%s` must be on %s; got %s" % (what, t.centers.device, v.device))
        if y.dim() != 2 or y.shape[1] <= widest:
            raise ValueError("OpesRun.deposit: `y` must be [W, more than %d columns]; got %s" % (widest, list(y.shape)))
        n_walkers = y.shape[0]
        if tuple(bias.shape) not in ((n_walkers,), (n_walkers, 4)):
            raise ValueError("OpesRun.deposit: `bias` must be [W] or the energies [W, 4]; got %s" % list(bias.shape))
        if n_walkers == 0:
            return None
        y = y.detach().contiguous()
        V = bias.detach() if bias.dim() == 1 else bias.detach()[:, 3]
        with torch.cuda.device(t.centers.device):
            _capi.opes_step_columns_f64(t.centers, t.sigma, t.heights, t.state, self.run, t.period, y, self._column_array, V, self.sigma0,
                                        self.sigma_min, self.beta, t.threshold, t.cutoff, self.fixed_sigma)
        return None

    def _step_modes(self, name, y, bias, observe):
        """`deposit` and `observe` of an adaptive or an explore run: `molann_opes_step_modes_f64` on the outputs where they are; a plain
        run passes its row stride d and the identity columns."""
        from . import _capi
        t = self.table
        widest = t.d - 1 if self.columns is None else max(self.columns)
        for what, v in (("y", y),) if observe else (("y", y), ("bias", bias)):
            if not isinstance(v, torch.Tensor):
                raise TypeError("OpesRun.%s: `%s` must be a tensor on %s; got %s" % (name, what, t.centers.device, type(v).__name__))
            if v.dtype != torch.float64:
                raise TypeError("OpesRun.%s: `%s` must be float64; got %s" % (name, what, v.dtype))
            if v.device != t.centers.device:
                raise ValueError("OpesRun.%s: `%s` must be on %s; got %s" % (name, what, t.centers.device, v.device))
        if y.dim() != 2 or y.shape[1] <= widest or (self._plain and y.shape[1] != t.d):
            raise ValueError("OpesRun.%s: `y` must be [W, %s]; got %s"
                             % (name, "%d" % t.d if self._plain else "more than %d columns" % widest, list(y.shape)))
        n_walkers = y.shape[0]
        if self.adaptive and n_walkers != self.walkers:
            raise ValueError("OpesRun.%s: the run keeps the averages of %d walkers; got %d" % (name, self.walkers, n_walkers))
        V = None
        if not observe:
            shapes = ((n_walkers,),) if self._plain else ((n_walkers,), (n_walkers, 4))
            if tuple(bias.shape) not in shapes:
                raise ValueError("OpesRun.deposit: `bias` must be [W]%s; got %s" % ("" if self._plain else " or the energies [W, 4]", list(bias.shape)))
            V = bias.detach() if bias.dim() == 1 else bias.detach()[:, 3]
        if n_walkers == 0:
            return None
        y = y.detach().contiguous()
        with torch.cuda.device(t.centers.device):
            _capi.opes_step_modes_f64(t.centers, t.sigma, t.heights, t.state, self.run, t.period, y, self._column_array, V, self.sigma0,
                                      self.sigma_min, self.adapt, self.beta, self.biasfactor, self.adaptive_stride, t.threshold, t.cutoff,
                                      self.fixed_sigma, self.explore, observe)
        return None

    def observe(self, y, energies=None):
        """An MD step between two deposits of an adaptive run: ``y`` as `bias` returned it joins every walker's running mean and M2 and
        ``run[6]`` counts it - OPES updates the averages at every step and deposits at every PACE-th.  ``energies`` is accepted for
        symmetry with `deposit` and ignored.  One launch on the current stream, nothing read back, returns None.  ValueError on a run
        whose widths are given."""
        if not self.adaptive:
            raise ValueError("OpesRun.observe: the run's widths are given (`sigma0` is not \"adaptive\"): there is nothing to observe")
        return self._step_modes("observe", y, None, True)

    def read_adaptive(self):
        """The adaptive state as a dict: ``observations`` and ``started`` (whether the first deposit has fixed ``sigma0``) as Python
        numbers, ``mean``, ``M2`` and ``sigma0`` as [walkers, d] CPU tensors.  A read-back: it waits for the steps queued before it."""
        if not self.adaptive:
            raise ValueError("OpesRun.read_adaptive: the run's widths are given (`sigma0` is not \"adaptive\")")
        run, rows = self.run.tolist(), self.adapt.cpu()
        return dict(observations=int(run[6]), started=bool(run[7]), mean=rows[:, 0].clone(), M2=rows[:, 1].clone(), sigma0=rows[:, 2].clone())

    def read_run(self):
        """``run`` as a dict of Python numbers (``counter``, ``sum_w``, ``sum_w2``, ``neff``, ``sigma_scale``, ``rct``): the one 64-byte
        read-back (it waits for the steps queued before it)."""
        counter, sum_w, sum_w2, neff, sigma_scale, rct = self.run.tolist()[:6]
        return dict(counter=int(counter), sum_w=sum_w, sum_w2=sum_w2, neff=neff, sigma_scale=sigma_scale, rct=rct)


class MetadRun(object):
    """A whole well-tempered metadynamics run on a table (PLUMED's ``METAD`` with ``GRID_*`` and a fixed ``SIGMA``) on the device: two
    launches per step and nothing read back, so the loop queues ahead of the device and can be captured in one ``torch.cuda.graph``.

    ``bias(x)`` is `MolANN.value_and_grid` on the table as it is (with ``walls`` or ``columns``: `MolANN.value_and_bias` with
    ``restraint=walls, grid=Grid(table, ..., columns)``); ``deposit(y, bias)`` is `molann_metad_deposit_f64` on the outputs that call
    wrote: walker a adds ``h_a prod_k exp(-1/2 ((g_k - y_ak) / sigma_k)^2)`` to every table entry within ``cutoff`` widths (None:
    everywhere), ``h_a = height exp(-V_a / (kT (biasfactor - 1)))`` with ``V_a`` the table's bias at the walker without the walls, in
    walker order and with no atomics: the same bits on every run.  ``state`` [8] on the table's device holds ``(hills, refused,
    sum_heights, steps, logged, 0, 0, 0)``; with ``log_capacity`` > 0 the first that many hills are kept in ``log`` [log_capacity,
    2 d + 1] as rows ``(centre, sigma, height)`` for a restart or a reweighting (`hills`).

    ``model``: a `MolANN` (or `PreprocessingANN`) in float64; ``table``: a float64 tensor of 1 to 3 dimensions on a CUDA / HIP device,
    held, not copied, and updated in place; ``lower``, ``spacing``, ``sigma``: one float per axis, ``periodic``: one bool per axis or None,
    as `value_and_grid` takes them; ``kT`` > 0; ``biasfactor`` > 1 (+inf: plain metadynamics, every height is ``height``); ``height``
    > 0; ``cutoff``: None or > 0, in widths (PLUMED cuts at 6.25); ``columns``: None or the outputs the table's axes are; ``walls``: a
    `Restraint` or None.  Everything is checked here, once.  A walker whose bias, outputs or height are not finite, or whose height
    underflows to 0, is counted in ``refused`` and changes no table entry.  With a cutoff a deposit touches only the tiles of the table
    a hill reaches, so its cost is the hills' footprint, not the table's size; without one every entry takes every walker's term, as in
    `add_hills_to_grid` - the torch route (`value_and_grid`, the heights with torch, `add_hills_to_grid` on the device table) was slower
    on every shape measured, by the least, 1.3x, for 64 walkers on 128^3 entries without a cutoff.

    ``rct_stride``: None, or an integer >= 1 (PLUMED's ``CALC_RCT`` with ``RCT_USTRIDE``): the run then keeps the reweighting offset
    c(t) of Tiwary and Parrinello on the device, so that a frame is weighted by ``exp((V - c) / kT)`` with nothing read back.  ``rct``
    [8] holds ``(c, updates, M, a0 M + log S0, aV M + log SV, steps at the update, bad, 0)`` with ``M`` the table's maximum,
    ``S0 = sum exp(a0 (V_g - M))``, ``SV = sum exp(aV (V_g - M))``, ``a0 = 1 / kT + aV``, ``aV = 1 / (kT (biasfactor - 1))`` and
    ``c = M + kT (log S0 - log SV)``: `molann_metad_rct_f64`, a deterministic reduction over the whole table in two launches that
    `deposit` enqueues after its own.  Whether a step updates - ``steps`` a multiple of the stride - is decided on the device from
    ``state``, so one captured graph replays a run with any stride.  ``bad`` counts the table entries that are not finite (``c`` is
    NaN then).  `update_rct` is the update now, `read_rct` the one read-back, `rbias` ``V - c`` on the device.  The update reads
    the whole table where a deposit with a cutoff touches a hill's footprint: 16-23 us for the pair alone and 9-15 us on a replayed
    step (3 us on a step off the stride) on tables of 256^2 to 128^3 entries, against 111-126 us for two ``torch.logsumexp`` on the
    table; no measured shape was slower than that route.

    ``adaptive``: None (the fixed widths above: the same kernels and the same bits as a run made without the argument), ``"diff"`` or
    ``"geom"`` - the adaptive Gaussians of Branduardi, Bussi and Parrinello (PLUMED's ``ADAPTIVE=DIFF`` / ``GEOM``): walker a's hill
    is ``h_a exp(-1/2 delta^T C_a^-1 delta)`` with a full covariance matrix, cut where ``delta^T C_a^-1 delta > cutoff^2``, deposited
    by `molann_metad_deposit_cov_f64`.  Both need ``walkers`` >= 1, the number of rows every `deposit` and `observe` brings; the run
    then holds ``adapt`` [walkers, 1 + d + T] (rows ``(n, mean, cov)``, T = d (d + 1) / 2, a matrix as its row-major upper triangle),
    ``adapt_state`` [8] = ``(observations, emits, skipped, 0...)`` and ``cov`` [walkers, T], the last step's covariances, all on the
    device.  ``"diff"`` needs ``window`` >= 1, in observations: every `observe` and every `deposit` moves each walker's running mean
    and covariance with decay ``1 / window``; a hill takes the running covariance once its walker has ``window`` observations and
    ``diag(sigma^2)`` before, so the run deposits sensible hills from its first step: 3 launches per step (bias, widths, deposit).
    ``"geom"``: ``C_ij = sigma_i sigma_j M_ij`` with M the metric J J^T that `value_and_metric` gives - ``sigma`` is then a length
    in the metric's units - passed to `deposit`: 4 launches per step (bias, metric, widths, deposit).  ``sigma_min``, ``sigma_max``:
    None or one float per axis, PLUMED's ``SIGMA_MIN`` / ``SIGMA_MAX``: a diagonal entry outside ``[sigma_min^2, sigma_max^2]`` is
    moved to the limit and its row and column scaled with it, so the correlations stay.  A walker whose matrix is not positive definite
    (a pivot of its Cholesky factor at most 1e-12 of the diagonal entry) or not finite is refused like any other invalid walker.  The
    log's rows are ``(centre, C, height)``, d + T + 1 wide: `cov_hills`.  A correlated hill is not a product over the axes, so the
    deposit forms one ``exp`` per entry and reaching hill where the fixed-width kernel forms 24-32 per hill and tile: with one walker
    and a cutoff of 6.25 the "diff" step took 1.08-1.14x and the "geom" step 1.57-1.66x the fixed-width step on tables of 256^2 to
    128^3 entries, with 64 walkers and no cutoff 1.2-2.1x and 1.7-2.3x; the torch route (`value_and_grid`, the covariance in torch ops,
    `add_cov_hills_to_grid`) was 5.7-15.9x slower than either on every shape measured - none was slower than it.

    Out of scope: a frame kernel that fuses `value_and_grid` with the metric; heights renormalised by the determinant; a running
    acceleration factor; a TorchScript operator for the adaptive step; walkers on several ranks; float32; tables of more than 3 axes
    (`PBMetadRun` biases up to 8 outputs with one 1-D table each, joined by a soft minimum)."""

    adaptive = None     # the fixed widths, unless the constructor is told otherwise

    def __init__(self, model, table, lower, spacing, kT, biasfactor, height, sigma, periodic=None, cutoff=None, columns=None, walls=None,
                 log_capacity=0, rct_stride=None, adaptive=None, window=None, sigma_min=None, sigma_max=None, walkers=None):
        from . import _capi
        if not (callable(getattr(model, "value_and_grid", None)) and callable(getattr(model, "value_and_bias", None))):
            raise TypeError("MetadRun: `model` must be a MolANN or a PreprocessingANN (it has no `value_and_grid`); got %s" % type(model).__name__)
        if not isinstance(table, torch.Tensor):
            raise TypeError("MetadRun: `table` must be a tensor; got %s" % type(table).__name__)
        if table.dtype != torch.float64:
            raise TypeError("MetadRun: `table` must be float64; got %s" % table.dtype)
        if not 1 <= table.dim() <= GRID_MAX_COLUMNS:
            raise ValueError("MetadRun: `table` must have 1 to %d dimensions; got %d" % (GRID_MAX_COLUMNS, table.dim()))
        if not table.is_contiguous() or table.requires_grad:
            raise ValueError("MetadRun: `table` is updated in place: it must be contiguous and must not require grad")
        if min(table.shape) < 4 or table.numel() >= 2 ** 31:
            raise ValueError("MetadRun: every axis of `table` needs at least 4 points and the table fewer than 2^31; got %s" % list(table.shape))
        d = table.dim()
        kT = _positive("MetadRun", "kT", kT)
        biasfactor = _positive("MetadRun", "biasfactor", biasfactor, allow_inf=True)
        height = _positive("MetadRun", "height", height)
        if not biasfactor > 1.0:
            raise ValueError("MetadRun: `biasfactor` must be > 1; got %r" % (biasfactor,))
        if cutoff is not None:
            cutoff = _positive("MetadRun", "cutoff", cutoff, allow_inf=True)
            cutoff = None if cutoff == math.inf else cutoff
        rows = []
        for what, v in (("lower", lower), ("spacing", spacing), ("sigma", sigma)):
            try:
                v = [float(c) for c in (v.tolist() if isinstance(v, torch.Tensor) else v)]
            except (TypeError, ValueError):
                raise TypeError("MetadRun: `%s` must be a sequence of %d numbers; got %s" % (what, d, type(v).__name__))
            if len(v) != d:
                raise ValueError("MetadRun: `%s` must have one entry per axis of `table` (%d); got %d" % (what, d, len(v)))
            if not all(math.isfinite(c) and (c > 0.0 or what == "lower") for c in v):
                raise ValueError("MetadRun: `%s` must be finite%s everywhere; got %s" % (what, "" if what == "lower" else " and > 0", v))
            rows.append(v)
        if periodic is not None:
            periodic = [bool(p) for p in periodic]
            if len(periodic) != d:
                raise ValueError("MetadRun: `periodic` must be None or one bool per axis of `table` (%d); got %d" % (d, len(periodic)))
        columns = _columns("MetadRun", columns, GRID_MAX_COLUMNS, "a table has at most 3 axes")
        if columns is not None and len(columns) != d:
            raise ValueError("MetadRun: `columns` must name one output per axis of `table` (%d); got %d" % (d, len(columns)))
        if walls is not None and not isinstance(walls, Restraint):
            raise TypeError("MetadRun: `walls` must be a Restraint or None; got %s" % type(walls).__name__)
        if isinstance(log_capacity, bool):
            raise TypeError("MetadRun: `log_capacity` must be an integer")
        log_capacity = operator.index(log_capacity)
        if log_capacity < 0:
            raise ValueError("MetadRun: `log_capacity` must be >= 0; got %d" % log_capacity)
        if rct_stride is not None:
            if isinstance(rct_stride, bool):
                raise TypeError("MetadRun: `rct_stride` must be None or an integer")
            try:
                rct_stride = operator.index(rct_stride)
            except TypeError:
                raise TypeError("MetadRun: `rct_stride` must be None or an integer; got %s" % type(rct_stride).__name__)
            if rct_stride < 1:
                raise ValueError("MetadRun: `rct_stride` must be None or >= 1; got %d" % rct_stride)
        if adaptive is not None and adaptive not in ("diff", "geom"):
            raise ValueError("MetadRun: `adaptive` must be None, \"diff\" or \"geom\"; got %r" % (adaptive,))
        limits = []
        if adaptive is None:
            for what, v in (("window", window), ("sigma_min", sigma_min), ("sigma_max", sigma_max), ("walkers", walkers)):
                if v is not None:
                    raise ValueError("MetadRun: `%s` belongs to an adaptive run (`adaptive` is None)" % what)
        else:
            if walkers is None or (window is None and adaptive == "diff"):
                raise ValueError("MetadRun: adaptive=%r needs `%s`" % (adaptive, "walkers" if walkers is None else "window"))
            if window is not None and adaptive == "geom":
                raise ValueError("MetadRun: `window` belongs to adaptive=\"diff\"")
            walkers = _count("MetadRun", "walkers", walkers)
            window = None if window is None else _count("MetadRun", "window", window)
            for what, v in (("sigma_min", sigma_min), ("sigma_max", sigma_max)):
                if v is not None:
                    try:
                        v = [float(c) for c in (v.tolist() if isinstance(v, torch.Tensor) else v)]
                    except (TypeError, ValueError):
                        raise TypeError("MetadRun: `%s` must be None or a sequence of %d numbers; got %s" % (what, d, type(v).__name__))
                    if len(v) != d:
                        raise ValueError("MetadRun: `%s` must have one entry per axis of `table` (%d); got %d" % (what, d, len(v)))
                    if not all(c >= 0.0 and (math.isfinite(c) or what == "sigma_max") for c in v):
                        raise ValueError("MetadRun: `%s` must be >= 0%s everywhere; got %s" % (what, " and finite" if what == "sigma_min" else "", v))
                limits.append(v)
            if limits[0] is not None and limits[1] is not None and any(hi < lo for lo, hi in zip(*limits)):
                raise ValueError("MetadRun: `sigma_max` must not lie below `sigma_min`; got %s, %s" % (limits[0], limits[1]))
        if table.device.type != "cuda":
            raise ValueError("MetadRun: the table lives in device memory and its kernels are HIP kernels; got device %s" % table.device)
        self.model, self.table, self.walls = model, table.detach(), walls
        self.lower, self.spacing, self.sigma, self.periodic, self.columns = rows[0], rows[1], rows[2], periodic, columns
        self.kT, self.biasfactor, self.height, self.cutoff = kT, biasfactor, height, cutoff
        self.inv_dT = 0.0 if biasfactor == math.inf else 1.0 / (kT * (biasfactor - 1.0))
        self.state = torch.zeros(8, dtype=torch.float64, device=table.device)
        T = d * (d + 1) // 2
        self.log = torch.zeros(log_capacity, (2 * d if adaptive is None else d + T) + 1, dtype=torch.float64, device=table.device) if log_capacity else None
        self.adaptive, self.window, self.walkers = adaptive, window, walkers
        self.sigma_min, self.sigma_max = limits if limits else (None, None)
        self.adapt = self.adapt_state = self.cov = self._limits = None
        if adaptive is not None:
            self.adapt = torch.zeros(walkers, 1 + d + T, dtype=torch.float64, device=table.device)
            self.adapt_state = torch.zeros(8, dtype=torch.float64, device=table.device)
            self.cov = torch.zeros(walkers, T, dtype=torch.float64, device=table.device)
            self._limits = _capi.metad_limit_arrays(self.sigma_min, self.sigma_max, d)
        self._grid = Grid(self.table, self.lower, self.spacing, self.periodic, self.columns)
        self._arrays = _capi.metad_grid_arrays(table.shape, self.lower, self.spacing, self.periodic, self.sigma, self.columns)
        self.rct_stride, self.rct, self._rct_partials = rct_stride, None, None
        if rct_stride is not None:
            self._allocate_rct()

    def _allocate_rct(self):
        from . import _capi
        rows = int(_capi.lib().molann_metad_rct_chunks(self.table.numel()))
        self.rct = torch.zeros(8, dtype=torch.float64, device=self.table.device)
        self._rct_partials = torch.zeros(rows, 4, dtype=torch.float64, device=self.table.device)

    def bias(self, x, into=None):
        """The walkers ``x`` under the table as it is now, one launch: ``(y, bias, dx)`` of `MolANN.value_and_grid`, or - with walls or
        columns - ``(y, energies, dx)`` of `MolANN.value_and_bias`, ``energies[:, 2]`` the table's bias."""
        if self.walls is None and self.columns is None:
            return self.model.value_and_grid(x, self.table, self.lower, self.spacing, self.periodic, into=into)
        return self.model.value_and_bias(x, restraint=self.walls, grid=self._grid, into=into)

    def _walker_rows(self, name, y):
        """``y`` of an adaptive run's `observe` / `deposit`, checked: float64 [walkers, n_out] on the table's device."""
        widest = self.table.dim() - 1 if self.columns is None else max(self.columns)
        if not isinstance(y, torch.Tensor):
            raise TypeError("MetadRun.%s: `y` must be a tensor on %s; got %s" % (name, self.table.device, type(y).__name__))
        if y.dtype != torch.float64:
            raise TypeError("MetadRun.%s: `y` must be float64; got %s" % (name, y.dtype))
        if y.device != self.table.device:
            raise ValueError("MetadRun.%s: `y` must be on %s; got %s" % (name, self.table.device, y.device))
        if y.dim() != 2 or y.shape[1] <= widest:
            raise ValueError("MetadRun.%s: `y` must be [W, more than %d columns]; got %s" % (name, widest, list(y.shape)))
        if y.shape[0] != self.walkers:
            raise ValueError("MetadRun.%s: the run was made for %d walkers; `y` has %d rows" % (name, self.walkers, y.shape[0]))
        return y.detach().contiguous()

    def observe(self, y):
        """``adaptive="diff"`` only: one observation of the walkers ``y`` [walkers, n_out] by their running means and covariances,
        with no hill - the call for the MD steps between two deposits.  One launch, nothing read back, returns None."""
        from . import _capi
        if self.adaptive != "diff":
            raise ValueError("MetadRun.observe: the run measures no widths (it was made with adaptive=%r)" % (self.adaptive,))
        y = self._walker_rows("observe", y)
        with torch.cuda.device(self.table.device):
            _capi.metad_widths_f64(self._arrays, self._limits, _capi.METAD_COV_DIFF, self.window, False, self.adapt, self.adapt_state, self.cov, y=y)
        return None

    def _deposit_adaptive(self, y, bias, metric):
        from . import _capi
        y = self._walker_rows("deposit", y)
        if not isinstance(bias, torch.Tensor):
            raise TypeError("MetadRun.deposit: `bias` must be a tensor on %s; got %s" % (self.table.device, type(bias).__name__))
        if bias.dtype != torch.float64:
            raise TypeError("MetadRun.deposit: `bias` must be float64; got %s" % bias.dtype)
        if bias.device != self.table.device:
            raise ValueError("MetadRun.deposit: `bias` must be on %s; got %s" % (self.table.device, bias.device))
        if tuple(bias.shape) not in ((self.walkers,), (self.walkers, 3)):
            raise ValueError("MetadRun.deposit: `bias` must be [W] or the energies [W, 3]; got %s" % list(bias.shape))
        if self.adaptive == "geom":
            if not isinstance(metric, torch.Tensor):
                raise TypeError("MetadRun.deposit: adaptive=\"geom\" needs `metric`, the [W, n_out, n_out] of `value_and_metric`; got %s"
                                % type(metric).__name__)
            if metric.dtype != torch.float64:
                raise TypeError("MetadRun.deposit: `metric` must be float64; got %s" % metric.dtype)
            if metric.device != self.table.device:
                raise ValueError("MetadRun.deposit: `metric` must be on %s; got %s" % (self.table.device, metric.device))
            if tuple(metric.shape) != (self.walkers, y.shape[1], y.shape[1]):
                raise ValueError("MetadRun.deposit: `metric` must be [%d, %d, %d]; got %s" % (self.walkers, y.shape[1], y.shape[1], list(metric.shape)))
            metric = metric.detach().contiguous()
        elif metric is not None:
            raise ValueError("MetadRun.deposit: `metric` belongs to adaptive=\"geom\"")
        V = bias.detach() if bias.dim() == 1 else bias.detach()[:, 2]
        with torch.cuda.device(self.table.device):
            if self.adaptive == "diff":
                _capi.metad_widths_f64(self._arrays, self._limits, _capi.METAD_COV_DIFF, self.window, True, self.adapt, self.adapt_state, self.cov, y=y)
            else:
                _capi.metad_widths_f64(self._arrays, self._limits, _capi.METAD_COV_GEOM, 1, True, None, self.adapt_state, self.cov, metric=metric)
            _capi.metad_deposit_cov_f64(self.table, self._arrays, y, V, self.cov, self.height, self.inv_dT, self.cutoff, self.state, self.log)
            if self.rct_stride is not None:
                _capi.metad_rct_f64(self.table, self.kT, self.inv_dT, self.state, self.rct_stride, self._rct_partials, self.rct)
        return None

    def deposit(self, y, bias, metric=None):
        """The step after `bias`: ``y`` [W, n_out] and ``bias`` [W], or ``energies`` [W, 3] whose column 2 is read in place, as that call
        returned them (read only).  One launch on the current stream, nothing read back, returns None.  An adaptive run enqueues the
        widths launch (``"diff"``: this step's observation and the covariances; ``"geom"``: the covariances from ``metric``
        [W, n_out, n_out], float64 on the device, as ``model.value_and_metric(x, weights)`` returned it) and then the deposit; W must be
        ``walkers``."""
        from . import _capi
        if self.adaptive is not None:
            return self._deposit_adaptive(y, bias, metric)
        if metric is not None:
            raise ValueError("MetadRun.deposit: `metric` belongs to adaptive=\"geom\"")
        widest = self.table.dim() - 1 if self.columns is None else max(self.columns)
        for what, t in (("y", y), ("bias", bias)):
            if not isinstance(t, torch.Tensor):
                raise TypeError("MetadRun.deposit: `%s` must be a tensor on %s; got %s" % (what, self.table.device, type(t).__name__))
            if t.dtype != torch.float64:
                raise TypeError("MetadRun.deposit: `%s` must be float64; got %s" % (what, t.dtype))
            if t.device != self.table.device:
                raise ValueError("MetadRun.deposit: `%s` must be on %s; got %s" % (what, self.table.device, t.device))
        if y.dim() != 2 or y.shape[1] <= widest:
            raise ValueError("MetadRun.deposit: `y` must be [W, more than %d columns]; got %s" % (widest, list(y.shape)))
        n_walkers = y.shape[0]
        if tuple(bias.shape) not in ((n_walkers,), (n_walkers, 3)):
            raise ValueError("MetadRun.deposit: `bias` must be [W] or the energies [W, 3]; got %s" % list(bias.shape))
        if n_walkers == 0:
            return None
        y = y.detach().contiguous()
        V = bias.detach() if bias.dim() == 1 else bias.detach()[:, 2]
        with torch.cuda.device(self.table.device):
            _capi.metad_deposit_f64(self.table, self._arrays, y, V, self.height, self.inv_dT, self.cutoff, self.state, self.log)
            if self.rct_stride is not None:
                _capi.metad_rct_f64(self.table, self.kT, self.inv_dT, self.state, self.rct_stride, self._rct_partials, self.rct)
        return None

    def update_rct(self):
        """The offset of the table as it is now, whatever the stride - for a table that was loaded rather than grown: two launches on the
        current stream, nothing read back, returns None.  A run made with ``rct_stride=None`` allocates ``rct`` on first use."""
        from . import _capi
        if self.rct is None:
            self._allocate_rct()
        with torch.cuda.device(self.table.device):
            _capi.metad_rct_f64(self.table, self.kT, self.inv_dT, None, 1, self._rct_partials, self.rct)
        return None

    def read_rct(self):
        """``rct`` as a dict of Python numbers (``rct``, ``updates``, ``max``, ``log_sum_0``, ``log_sum_V``, ``steps``, ``bad``): the one
        64-byte read-back (it waits for the steps queued before it)."""
        if self.rct is None:
            raise ValueError("MetadRun.read_rct: the run keeps no offset (`rct_stride` is None and `update_rct` was not called)")
        c, updates, top, log0, logV, steps, bad = self.rct.tolist()[:7]
        return dict(rct=c, updates=int(updates), max=top, log_sum_0=log0, log_sum_V=logV, steps=int(steps), bad=int(bad))

    def rbias(self, bias):
        """PLUMED's ``metad.rbias``: ``V - c`` [W] on the device, nothing read back.  ``bias``: [W], or the energies [W, 3] of `bias`
        whose column 2 is used."""
        if self.rct is None:
            raise ValueError("MetadRun.rbias: the run keeps no offset (`rct_stride` is None and `update_rct` was not called)")
        if not isinstance(bias, torch.Tensor):
            raise TypeError("MetadRun.rbias: `bias` must be a tensor on %s; got %s" % (self.table.device, type(bias).__name__))
        if bias.dtype != torch.float64:
            raise TypeError("MetadRun.rbias: `bias` must be float64; got %s" % bias.dtype)
        if bias.device != self.table.device:
            raise ValueError("MetadRun.rbias: `bias` must be on %s; got %s" % (self.table.device, bias.device))
        if bias.dim() not in (1, 2) or (bias.dim() == 2 and bias.shape[1] != 3):
            raise ValueError("MetadRun.rbias: `bias` must be [W] or the energies [W, 3]; got %s" % list(bias.shape))
        V = bias.detach() if bias.dim() == 1 else bias.detach()[:, 2]
        return V - self.rct[0]

    def read_state(self):
        """``state`` as a dict of Python numbers (``hills``, ``refused``, ``sum_heights``, ``steps``, ``logged``): the one 64-byte
        read-back (it waits for the steps queued before it)."""
        hills, refused, sum_heights, steps, logged = self.state.tolist()[:5]
        return dict(hills=int(hills), refused=int(refused), sum_heights=sum_heights, steps=int(steps), logged=int(logged))

    def hills(self, n=None):
        """The logged hills as a `Hills` record - views of ``log[:n]``, nothing copied - for `MolANN.value_and_hills` (unpack its fields),
        `value_and_bias(hills=...)` and `add_hills_to_grid(table, lower, spacing, periodic, h.centers, h.heights, h.sigma)`.  ``n``: the
        logged count where the caller has it; None reads the state."""
        if self.adaptive is not None:
            raise ValueError("MetadRun.hills: an adaptive run's hills have covariance matrices, not widths: `cov_hills`")
        if self.log is None:
            raise ValueError("MetadRun.hills: the run keeps no log (`log_capacity` is 0)")
        n = self.read_state()["logged"] if n is None else operator.index(n)
        if not 0 <= n <= self.log.shape[0]:
            raise ValueError("MetadRun.hills: `n` must be 0..%d; got %d" % (self.log.shape[0], n))
        d = self.table.dim()
        period = None
        if self.periodic is not None and any(self.periodic):
            period = torch.tensor([self.table.shape[k] * self.spacing[k] if self.periodic[k] else 0.0 for k in range(d)], dtype=torch.float64,
                                  device=self.table.device)
        return Hills(self.log[:n, :d], self.log[:n, 2 * d], self.log[:n, d:2 * d], period, self.columns)

    def _period(self):
        d = self.table.dim()
        if self.periodic is None or not any(self.periodic):
            return None
        return torch.tensor([self.table.shape[k] * self.spacing[k] if self.periodic[k] else 0.0 for k in range(d)], dtype=torch.float64,
                            device=self.table.device)

    def cov_hills(self, n=None):
        """The logged hills of an adaptive run as a `CovHills` record - views of ``log[:n]``, nothing copied - for
        `add_cov_hills_to_grid(table, lower, spacing, periodic, h.centers, h.covariances, h.heights, cutoff)`.  ``n``: the logged count
        where the caller has it; None reads the state."""
        if self.adaptive is None:
            raise ValueError("MetadRun.cov_hills: the run's hills have fixed widths: `hills`")
        if self.log is None:
            raise ValueError("MetadRun.cov_hills: the run keeps no log (`log_capacity` is 0)")
        n = self.read_state()["logged"] if n is None else operator.index(n)
        if not 0 <= n <= self.log.shape[0]:
            raise ValueError("MetadRun.cov_hills: `n` must be 0..%d; got %d" % (self.log.shape[0], n))
        d = self.table.dim()
        T = d * (d + 1) // 2
        return CovHills(self.log[:n, :d], self.log[:n, d:d + T], self.log[:n, d + T], self._period(), self.columns)

    def read_adaptive(self):
        """An adaptive run's statistics as a dict: ``observations``, ``emits``, ``skipped`` (Python ints), ``n`` [walkers], ``mean``
        [walkers, d], ``cov`` [walkers, T] (the running covariances; zeros for ``"geom"``) and ``last`` [walkers, T] (the last step's
        hill covariances) as CPU tensors: the one read-back (it waits for the steps queued before it)."""
        if self.adaptive is None:
            raise ValueError("MetadRun.read_adaptive: the run measures no widths (`adaptive` is None)")
        d = self.table.dim()
        observations, emits, skipped = self.adapt_state.tolist()[:3]
        adapt = self.adapt.cpu()
        return dict(observations=int(observations), emits=int(emits), skipped=int(skipped), n=adapt[:, 0].clone(), mean=adapt[:, 1:1 + d].clone(),
                    cov=adapt[:, 1 + d:].clone(), last=self.cov.cpu())


class PBMetadRun(object):
    """A whole parallel-bias metadynamics run (Pfaendtner and Bonomi, JCTC 2015; PLUMED's ``PBMETAD`` with grids and a fixed ``SIGMA``)
    on the device, on up to 8 outputs: K one-dimensional tables, one per biased output, joined by a soft minimum, so that memory and the
    cost of a step grow linearly in K where a table over K outputs (`MetadRun`) has n^K entries and at most 3 axes.  Two launches per
    step and nothing read back, so the loop queues ahead of the device and can be captured in one ``torch.cuda.graph``.

    ``bias(x)`` is `MolANN.value_and_pbmetad` on the tables as they are: ``(y, energies, dx)`` with ``energies`` [N, 2 + K] =
    ``(E_walls, V_PB, V_0 .. V_{K-1})``, ``V_k`` table k's cubic-convolution interpolant at output ``columns[k]``,
    ``V_PB = -kT log sum_k exp(-V_k / kT)`` formed from the minimum, and ``dx`` the gradient of ``E_walls + V_PB``.  ``deposit(y,
    energies)`` is `molann_pbmetad_deposit_f64` on what that call wrote (columns 2.. are read in place): walker a adds ``h_ak
    exp(-1/2 ((g - y_ak) / sigma_k)^2)`` to every entry of table k within ``cutoff`` widths (None: everywhere), ``h_ak = height
    exp(-V_ak / (kT (biasfactor - 1))) w_ak`` with ``w_ak = exp(-V_ak / kT) / sum_j exp(-V_aj / kT)``, in walker order and with no
    atomics: the same bits on every run.  ``state`` [8] holds ``(hills, refused, sum_heights, steps, logged, 0, 0, 0)`` with
    ``sum_heights`` over walkers and axes; with ``log_capacity`` > 0 the first that many walkers are kept in ``log`` [log_capacity,
    2 K] as rows ``(centre_0.., h_0..)``: `hills`.

    ``model``: a `MolANN` (or `PreprocessingANN`) in float64; ``shape``: K point counts >= 4; ``lower``, ``spacing``, ``sigma``: one
    float per axis; ``periodic``: one bool per axis or None; ``kT`` > 0; ``biasfactor`` > 1 (+inf: every height is ``height w_ak``);
    ``height`` > 0; ``cutoff``: None or > 0, in widths; ``columns``: None (the first K outputs) or the K outputs the axes bias;
    ``walls``: a `Restraint` on all outputs or None; ``table``: None (zeros on the model's device) or a contiguous float64 tensor of
    ``sum(shape)`` values on a CUDA / HIP device, held, not copied, and updated in place.  Everything is checked here, once.  A walker
    with a bias, an output or a height that is not finite is counted in ``refused`` and changes no table; a height that underflows to
    exactly 0 adds nothing to its axis and the walker still counts.

    Out of scope: c(t) and ``rbias``; adaptive widths; per-axis heights or bias factors; partitioned families; walkers on several
    ranks; float32; a TorchScript operator for the deposit."""

    def __init__(self, model, shape, lower, spacing, kT, biasfactor, height, sigma, periodic=None, cutoff=None, columns=None, walls=None,
                 log_capacity=0, table=None):
        from . import _capi
        if not callable(getattr(model, "value_and_pbmetad", None)):
            raise TypeError("PBMetadRun: `model` must be a MolANN or a PreprocessingANN (it has no `value_and_pbmetad`); got %s" % type(model).__name__)
        if isinstance(shape, torch.Tensor):
            shape = shape.tolist()
        try:
            shape = tuple(operator.index(n) for n in shape)
        except TypeError:
            raise TypeError("PBMetadRun: `shape` must be a sequence of integers, one per axis; got %s" % type(shape).__name__)
        K = len(shape)
        if K < 1:
            raise ValueError("PBMetadRun: `shape` must name at least one axis")
        if K > HILLS_MAX_COLUMNS:
            raise NotImplementedError("PBMetadRun: a parallel bias has at most %d axes; got %d" % (HILLS_MAX_COLUMNS, K))
        if min(shape) < 4 or sum(shape) >= 2 ** 31:
            raise ValueError("PBMetadRun: every axis needs at least 4 points and all of them fewer than 2^31; got %s" % list(shape))
        kT = _positive("PBMetadRun", "kT", kT)
        biasfactor = _positive("PBMetadRun", "biasfactor", biasfactor, allow_inf=True)
        height = _positive("PBMetadRun", "height", height)
        if not biasfactor > 1.0:
            raise ValueError("PBMetadRun: `biasfactor` must be > 1; got %r" % (biasfactor,))
        if cutoff is not None:
            cutoff = _positive("PBMetadRun", "cutoff", cutoff, allow_inf=True)
            cutoff = None if cutoff == math.inf else cutoff
        rows = []
        for what, v in (("lower", lower), ("spacing", spacing), ("sigma", sigma)):
            try:
                v = [float(c) for c in (v.tolist() if isinstance(v, torch.Tensor) else v)]
            except (TypeError, ValueError):
                raise TypeError("PBMetadRun: `%s` must be a sequence of %d numbers; got %s" % (what, K, type(v).__name__))
            if len(v) != K:
                raise ValueError("PBMetadRun: `%s` must have one entry per axis (%d); got %d" % (what, K, len(v)))
            if not all(math.isfinite(c) and (c > 0.0 or what == "lower") for c in v):
                raise ValueError("PBMetadRun: `%s` must be finite%s everywhere; got %s" % (what, "" if what == "lower" else " and > 0", v))
            rows.append(v)
        if periodic is not None:
            periodic = [bool(p) for p in periodic]
            if len(periodic) != K:
                raise ValueError("PBMetadRun: `periodic` must be None or one bool per axis (%d); got %d" % (K, len(periodic)))
        columns = _columns("PBMetadRun", columns, HILLS_MAX_COLUMNS, "a parallel bias has at most 8 axes")
        if columns is not None and len(columns) != K:
            raise ValueError("PBMetadRun: `columns` must name one output per axis (%d); got %d" % (K, len(columns)))
        if walls is not None and not isinstance(walls, Restraint):
            raise TypeError("PBMetadRun: `walls` must be a Restraint or None; got %s" % type(walls).__name__)
        if isinstance(log_capacity, bool):
            raise TypeError("PBMetadRun: `log_capacity` must be an integer")
        log_capacity = operator.index(log_capacity)
        if log_capacity < 0:
            raise ValueError("PBMetadRun: `log_capacity` must be >= 0; got %d" % log_capacity)
        if table is None:
            device = next((t.device for t in list(model.parameters()) + list(model.buffers())), torch.device("cpu"))
            if device.type != "cuda":
                raise ValueError("PBMetadRun: the tables live in device memory and their kernels are HIP kernels; the model is on %s" % device)
            table = torch.zeros(sum(shape), dtype=torch.float64, device=device)
        else:
            if not isinstance(table, torch.Tensor):
                raise TypeError("PBMetadRun: `table` must be None or a tensor; got %s" % type(table).__name__)
            if table.dtype != torch.float64:
                raise TypeError("PBMetadRun: `table` must be float64; got %s" % table.dtype)
            if table.dim() != 1 or table.numel() != sum(shape):
                raise ValueError("PBMetadRun: `table` must be [sum(shape) = %d]; got %s" % (sum(shape), list(table.shape)))
            if not table.is_contiguous() or table.requires_grad:
                raise ValueError("PBMetadRun: `table` is updated in place: it must be contiguous and must not require grad")
            if table.device.type != "cuda":
                raise ValueError("PBMetadRun: the tables live in device memory and their kernels are HIP kernels; got device %s" % table.device)
        self.model, self.table, self.walls = model, table.detach(), walls
        self.shape, self.lower, self.spacing, self.sigma, self.periodic, self.columns = shape, rows[0], rows[1], rows[2], periodic, columns
        self.kT, self.biasfactor, self.height, self.cutoff = kT, biasfactor, height, cutoff
        self.inv_dT = 0.0 if biasfactor == math.inf else 1.0 / (kT * (biasfactor - 1.0))
        self.state = torch.zeros(8, dtype=torch.float64, device=table.device)
        self.log = torch.zeros(log_capacity, 2 * K, dtype=torch.float64, device=table.device) if log_capacity else None
        self._records = PBTables(self.table, shape, self.lower, self.spacing, periodic, columns)
        self._arrays = _capi.metad_grid_arrays(shape, self.lower, self.spacing, self.periodic, self.sigma, self.columns)

    @property
    def tables(self):
        """The K tables as views of ``table``, nothing copied."""
        return self._records.views()

    def records(self):
        """The `PBTables` of the run, as `MolANN.value_and_pbmetad` takes it."""
        return self._records

    def bias(self, x, into=None):
        """The walkers ``x`` under the tables as they are now, one launch: ``(y, energies, dx)`` of `MolANN.value_and_pbmetad`."""
        return self.model.value_and_pbmetad(x, self._records, self.kT, restraint=self.walls, into=into)

    def deposit(self, y, energies):
        """The step after `bias`: ``y`` [W, n_out] and ``energies`` [W, 2 + K] as that call returned them (read only; columns 2.. are
        read in place).  One launch on the current stream, nothing read back, returns None."""
        from . import _capi
        K = len(self.shape)
        widest = K - 1 if self.columns is None else max(self.columns)
        for what, t in (("y", y), ("energies", energies)):
            if not isinstance(t, torch.Tensor):
                raise TypeError("PBMetadRun.deposit: `%s` must be a tensor on %s; got %s" % (what, self.table.device, type(t).__name__))
            if t.dtype != torch.float64:
                raise TypeError("PBMetadRun.deposit: `%s` must be float64; got %s" % (what, t.dtype))
            if t.device != self.table.device:
                raise ValueError("PBMetadRun.deposit: `%s` must be on %s; got %s" % (what, self.table.device, t.device))
        if y.dim() != 2 or y.shape[1] <= widest:
            raise ValueError("PBMetadRun.deposit: `y` must be [W, more than %d columns]; got %s" % (widest, list(y.shape)))
        n_walkers = y.shape[0]
        if tuple(energies.shape) != (n_walkers, 2 + K) or energies.stride(1) != 1:
            raise ValueError("PBMetadRun.deposit: `energies` must be the [W, %d] of `bias` with unit stride along a row; got %s"
                             % (2 + K, list(energies.shape)))
        if n_walkers == 0:
            return None
        y = y.detach()
        y = y if y.stride(1) == 1 else y.contiguous()
        with torch.cuda.device(self.table.device):
            _capi.pbmetad_deposit_f64(self.table, self._arrays, y, energies.detach()[:, 2:], self.height, self.inv_dT, self.kT, self.cutoff,
                                      self.state, self.log)
        return None

    def read_state(self):
        """``state`` as a dict of Python numbers (``hills``, ``refused``, ``sum_heights``, ``steps``, ``logged``): the one 64-byte
        read-back (it waits for the steps queued before it)."""
        hills, refused, sum_heights, steps, logged = self.state.tolist()[:5]
        return dict(hills=int(hills), refused=int(refused), sum_heights=sum_heights, steps=int(steps), logged=int(logged))

    def hills(self, k, n=None):
        """The logged hills of axis ``k`` as a `Hills` record on one column - views of ``log[:n]``, nothing copied - for
        `add_hills_to_grid(run.tables[k], [lower[k]], [spacing[k]], [periodic[k]], h.centers, h.heights, h.sigma)`, the restart route.
        ``n``: the logged count where the caller has it; None reads the state."""
        K = len(self.shape)
        if self.log is None:
            raise ValueError("PBMetadRun.hills: the run keeps no log (`log_capacity` is 0)")
        if isinstance(k, bool):
            raise TypeError("PBMetadRun.hills: `k` must be an integer")
        k = operator.index(k)
        if not 0 <= k < K:
            raise IndexError("PBMetadRun.hills: `k` must be 0..%d; got %d" % (K - 1, k))
        n = self.read_state()["logged"] if n is None else operator.index(n)
        if not 0 <= n <= self.log.shape[0]:
            raise ValueError("PBMetadRun.hills: `n` must be 0..%d; got %d" % (self.log.shape[0], n))
        period = None
        if self.periodic is not None and self.periodic[k]:
            period = torch.tensor([self.shape[k] * self.spacing[k]], dtype=torch.float64, device=self.table.device)
        return Hills(self.log[:n, k:k + 1], self.log[:n, K + k], [self.sigma[k]], period, (k if self.columns is None else self.columns[k],))
