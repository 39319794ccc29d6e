"""A non-finite frame changes no other frame, in every entry point of the C ABI and every kernel family (tests/isolation.py).

The family table, the plans, the calls and the oracle are those of test_gpu_buffer_placement.py (imported, not copied), plus the five
float64 entries that table lacks - molann_value_and_grid_f64, molann_value_and_bias_f64, molann_value_and_opes_f64,
molann_value_and_bias_opes_f64 and molann_value_and_opes_table_f64, on small tables made the way their own test files make them (the
grid from the REFERENCE's outputs, test_gpu_value_and_grid_f64._grid_from; the OPES kernels on rows of the reference's outputs, a
width of noise on each; the table entry's dead rows NaN, its state (n, S) with S summed on the host).  The grid entry takes at most
three outputs: it runs on the cases whose head ends in 3; the OPES entries take at most eight: every head here.  The shared inputs of
the OPES entries - the kernel table and, read by every block, the state - must come back from every launch bit for bit.

Per case (family, frame size, head width), per entry and per poisonable input buffer of the entry:

Small batch, N = 200 (three 64-frame tiles and a tail of 8: the last tile and the last round of every several-frames-per-wave kernel
are short).  A clean launch: return code 0, the family's kernel in the launch info, every output within that file's tolerances of
float64 autograd through the oracle and finite, the oracle's values finite.  Two poisoned launches (kind "mixed") with the disjoint
bad sets {0, 63, N-1} and {1, 64, 100, N-2}: return code and launch info as before, every per-frame output bit for bit the clean
launch's on every frame outside the set (isolation.keep_rows_equal), the bad frames' dependent elements (isolation.dependent_elements)
non-finite.  Where the plan has an atom that only a bond names, x is poisoned there as well: the chosen atom's bond shares its
atoms with an angle, whose gradient would cover the bond's rows.  Printed, not asserted: how many elements of the bad frames' rows
are finite where the reference is not.  The reference of a poisoned batch is the same float64 autograd through the oracle; torch's
SVD refuses a matrix that is not finite, so for such a frame it is given NaN factors (`_svd_that_returns_nan`): the reference's NaN
centroid and rotation make everything they reach NaN.

Dense poison: one launch per entry in which every frame but about 34 (the first and the last, 63 and 64, 30 seeded ones) is poisoned
in every per-frame input, at an N at which - by the grid, block, ring and round sizes the launch info reports (GEOMETRY) - every block
runs at least three rounds, and three generations of its ring where it has one: any slot, staging row, LDS scratch or parity buffer
carried from one round to the next carries a NaN.  The batch is a few hundred seeded frames repeated on the device; the clean launch
of the same N is the comparison (the small batch anchored it): kept frames bit-identical and finite.  One launch takes
at most what keeps every buffer under 1 GB and - entries that work through a chunked workspace, launch info "chunk=" / "chunks of" -
one chunk of the plan; a later kernel of a composite launch that would need more for its three rounds has them in its own entry.

Sums over frames (grad_params) are not compared under poison: under x- or f-poison every element the reference makes NaN must be
non-finite; clean, two launches give the same bits except for the TILE_ORDER pairs (held to the oracle).  The ATOMICS family's keep
rows are held to the oracle at that file's tolerance and must be finite.  Every launch runs once; nothing here can fault by design."""

import contextlib
import ctypes
import re

import numpy as np
import pytest
import torch

import isolation as iso
import test_gpu_buffer_placement as bp
import test_gpu_value_and_grid_f64 as vg
import test_gpu_value_and_opes_f64 as vo
from molann_amd import _capi
from oracle import molann_oracle as mo
from test_gpu_angular_edges import _wrapped
from test_gpu_buffer_placement import ATOMICS, CASES, FAMILIES, TILE_ORDER, _against_oracle, _ctx, _entry, _launch, _outputs

pytestmark = pytest.mark.gpu
F64 = torch.float64
N_SMALL = 200
BAD_SETS = ((0, 63, N_SMALL - 1), (1, 64, 100, N_SMALL - 2))
BASE = 251                              # seeded frames the dense batch repeats: a prime, so copies do not line up with tiles
N_FIRST = 20000                         # the dense phase's first guess; it grows to what the launch info asks for
ONE_GB = 1 << 30
GRID, BIAS = "value_and_grid_f64", "value_and_bias_f64"
OPES, BIAS_OPES, OPES_TABLE = "value_and_opes_f64", "value_and_bias_opes_f64", "value_and_opes_table_f64"
OPES_ENTRIES = (OPES, BIAS_OPES, OPES_TABLE)
NEW = (GRID, BIAS) + OPES_ENTRIES       # the entries this file adds to the placement table's
_EXTRA = {GRID: r"frames_value_grid_f64_kernel", BIAS: r"frames_value_bias_f64_kernel", OPES: r"frames_value_opes_f64_kernel",
          BIAS_OPES: r"frames_value_bias_opes_f64_kernel", OPES_TABLE: r"frames_value_opes_table_f64_kernel"}
EXTRA = {"f64_small": dict(_EXTRA), "f64_mid": dict(_EXTRA)}
SMALL, DENSE = set(), {}                # (family, entry) that passed the small batch / {(family, entry): (N, rounds of the first kernel, chunk)}
assert all({"v": 4, "tangent_out": 3}[k] - r - 1 == iso.frame_dim(k) for k, r in bp.ROW_DIMS.items()) and set(bp.ROW_DIMS) == set(iso.FRAME_DIM)


def _patterns(cx):
    extra = dict((e, p) for e, p in EXTRA.get(cx.family, {}).items() if (e != GRID or cx.d_out <= 3) and (e not in OPES_ENTRIES or cx.d_out <= 8))
    return dict(cx.patterns, **extra)


# ---- the five entries the placement table lacks ---------------------------------------------------------------------------------------
_YREF = {}


def _y_ref(cx, entry):
    """The reference's outputs on the case's small batch: what the grids are laid over (never the code under test)."""
    real = getattr(cx, "real", cx)
    key = (real.family, real.n_inp, real.d_out, entry)
    if key not in _YREF:
        _YREF.clear()
        _YREF[key] = bp._want(real, "forward_f64", {"x": real.x(N_SMALL, entry).double()})["out"].detach()
    return _YREF[key]


def _tables(cx, entry):
    """(columns, table, shape, lower, spacing, periodic) of the entry's grid term"""
    y = _y_ref(cx, entry)
    if entry == GRID:
        cols, periodic = list(range(cx.d_out)), [False, True, False][:cx.d_out]
        shape = vg.SHAPES[cx.d_out]
    else:
        cols, periodic, shape = [2, 0], [False, True], vg.SHAPES[2]
    lower, spacing = vg._grid_from(y[:, cols], shape, periodic)
    return cols, vg._seeded_table(shape, 5 + len(cols)), shape, lower, spacing, periodic


HILLS_COLUMNS, N_HILLS = [1, 0], 5
N_KERNELS, CAPACITY, OPES_CUTOFF, OPES_EPS = 7, 12, 4.0, 1e-3


def _opes_columns(cx, entry):
    return list(HILLS_COLUMNS) if entry == BIAS_OPES else list(range(cx.d_out))


def _opes_table(cx, entry):
    """(columns, centers [K, d], heights [K], sigma [K, d], period [d], norm) of the entry's OPES term: K kernels on rows of the
    reference's outputs, a width of noise on each, widths 0.3-0.6 of the outputs' spread, positive heights, column 0 periodic."""
    cols = _opes_columns(cx, entry)
    y = _y_ref(cx, entry)[:, cols]
    g = torch.Generator().manual_seed(len(cols) + 17)
    rand = lambda *shape: torch.rand(shape, generator=g, dtype=F64)       # noqa: E731
    sigma = (0.3 + 0.3 * rand(N_KERNELS, len(cols))) * y.std(dim=0).clamp(min=1e-3)
    centers = y[torch.arange(N_KERNELS) * 29 % y.shape[0]] + (rand(N_KERNELS, len(cols)) - 0.5) * sigma
    heights = 0.2 + rand(N_KERNELS)
    period = torch.zeros(len(cols), dtype=F64)
    period[0] = 2.5
    return cols, centers, heights, sigma, period, vo._norm(heights)


def _opes_state(centers, heights, sigma, period):
    """(n, S, 0, 0) of a table whose live rows are these: S = sum_i sum_j heights_j K_j(centers_i), on the host"""
    total = float(vo._density(centers, centers, heights, sigma, period, OPES_CUTOFF)[0].sum())
    return torch.tensor([float(centers.shape[0]), total, 0.0, 0.0], dtype=F64)


def _dead_rows(t):
    """the table tensor in a capacity of CAPACITY rows, the dead ones NaN"""
    out = torch.full((CAPACITY,) + tuple(t.shape[1:]), float("nan"), dtype=F64)
    out[:t.shape[0]] = t
    return out


def _entry2(cx, entry, n):
    if entry not in NEW:
        return _entry(cx, entry, n)
    L, ni, do = _capi.lib(), cx.n_inp, cx.d_out
    lay, wn, bn = bp._layers(cx)
    WB = lambda p: (bp._ptr_array(p, wn), bp._ptr_array(p, bn))                    # noqa: E731
    x = ("x", "in", cx.x(n, entry))
    if entry in (OPES, OPES_TABLE):
        _, oc, oh, osig, operiod, norm = _opes_table(cx, entry)
        outs = [("out", "out", (n, do)), ("bias", "out", (n,)), ("grad_x", "out", (n, ni, 3))]
        if entry == OPES:
            return [x] + lay + [("centers", "in", oc), ("heights", "in", oh), ("sigma", "in", osig), ("opes_period", "in", operiod)] + outs, \
                lambda h, p, s: L.molann_value_and_opes_f64(h, p["x"], n, *WB(p), p["centers"], p["heights"], N_KERNELS, p["sigma"], do, p["opes_period"],
                                                            vo.SCALE, norm, OPES_EPS, OPES_CUTOFF, p["out"], p["bias"], p["grad_x"], s), cx.plan
        state = _opes_state(oc, oh, osig, operiod)
        return [x] + lay + [("centers", "in", _dead_rows(oc)), ("heights", "in", _dead_rows(oh)), ("sigma", "in", _dead_rows(osig)), ("state", "in", state),
                            ("opes_period", "in", operiod)] + outs, \
            lambda h, p, s: L.molann_value_and_opes_table_f64(h, p["x"], n, *WB(p), p["centers"], p["heights"], p["sigma"], CAPACITY, p["state"],
                                                              p["opes_period"], vo.SCALE, OPES_EPS, OPES_CUTOFF, p["out"], p["bias"], p["grad_x"], s), cx.plan
    cols, table, shape, lower, spacing, periodic = _tables(cx, entry)
    if entry == GRID:
        sh, lo, sp = (ctypes.c_int64 * do)(*shape), (ctypes.c_double * do)(*lower), (ctypes.c_double * do)(*spacing)
        per = (ctypes.c_int32 * do)(*[int(v) for v in periodic])
        return [x] + lay + [("table", "in", table), ("out", "out", (n, do)), ("bias", "out", (n,)), ("grad_x", "out", (n, ni, 3))], \
            lambda h, p, s: L.molann_value_and_grid_f64(h, p["x"], n, *WB(p), p["table"], sh, lo, sp, per, p["out"], p["bias"], p["grad_x"], s), cx.plan
    center, kappa = cx.randn((n, do), entry, n, 3), 0.5 + cx.randn((do,), entry, n, 4).abs()
    period = torch.where(torch.arange(do) % 2 == 0, torch.full((do,), 2.5, dtype=F64), torch.zeros(do, dtype=F64))
    flat = 0.05 * (torch.arange(do) % 3).to(F64)
    if entry == BIAS_OPES:
        oc_cols, oc, oh, osig, operiod, norm = _opes_table(cx, entry)

        def call_opes(h, p, s):
            terms, keep = _capi.bias_terms_f64(("center", "kappa", "period", "flat", do), None, (cols, "table", shape, lower, spacing, periodic),
                                               ptr=lambda name: p[name])
            term, keep_o = _capi.opes_term_f64((oc_cols, "centers", "heights", "sigma", "opes_period", N_KERNELS, len(oc_cols), vo.SCALE, norm, OPES_EPS,
                                                OPES_CUTOFF), ptr=lambda name: p[name])
            rc = L.molann_value_and_bias_opes_f64(h, p["x"], n, *WB(p), ctypes.byref(terms), ctypes.byref(term), p["out"], p["energies"], p["grad_x"], s)
            del keep, keep_o
            return rc

        return [x] + lay + [("center", "in", center), ("kappa", "in", kappa), ("period", "in", period), ("flat", "in", flat),
                            ("centers", "in", oc), ("heights", "in", oh), ("sigma", "in", osig), ("opes_period", "in", operiod), ("table", "in", table),
                            ("out", "out", (n, do)), ("energies", "out", (n, 4)), ("grad_x", "out", (n, ni, 3))], call_opes, cx.plan
    centers, heights = cx.randn((N_HILLS, 2), entry, n, 5), cx.randn((N_HILLS,), entry, n, 6)
    sigma = 0.5 + cx.randn((N_HILLS, 2), entry, n, 7).abs()

    def call(h, p, s):
        terms, keep = _capi.bias_terms_f64(("center", "kappa", "period", "flat", do),
                                           (HILLS_COLUMNS, "centers", "heights", "sigma", None, N_HILLS, 2),
                                           (cols, "table", shape, lower, spacing, periodic), ptr=lambda name: p[name])
        rc = L.molann_value_and_bias_f64(h, p["x"], n, *WB(p), ctypes.byref(terms), p["out"], p["energies"], p["grad_x"], s)
        del keep
        return rc

    return [x] + lay + [("center", "in", center), ("kappa", "in", kappa), ("period", "in", period), ("flat", "in", flat),
                        ("centers", "in", centers), ("heights", "in", heights), ("sigma", "in", sigma), ("table", "in", table),
                        ("out", "out", (n, do)), ("energies", "out", (n, 3)), ("grad_x", "out", (n, ni, 3))], call, cx.plan


def _want2(cx, entry, data):
    """bp._want, and the five new entries by float64 autograd of the formulas of include/molann_hip.h"""
    if entry not in NEW:
        return bp._want(cx, entry, data)
    xx = data["x"].double().clone().requires_grad_(True)
    y = cx.head.double()(mo.preprocessing_forward(xx, cx.items, False, cx.align, cx.ref))
    if entry in OPES_ENTRIES:      # V_o = scale log(P / norm + epsilon), P the kernel sum under the cutoff; the table entry's norm is S / n
        live = int(data["state"][0]) if entry == OPES_TABLE else N_KERNELS
        norm = float(data["state"][1]) / live if entry == OPES_TABLE else _opes_table(cx, entry)[5]
        kernels = tuple(data[k][:live] for k in ("centers", "heights", "sigma"))
        v_o = vo._bias(y[:, _opes_columns(cx, entry)], kernels, data["opes_period"], norm, OPES_EPS, OPES_CUTOFF)
        if entry != BIAS_OPES:
            (gx,) = torch.autograd.grad(v_o.sum(), xx)
            return {"out": y.detach(), "bias": v_o.detach(), "grad_x": gx}
    cols, table, shape, lower, spacing, periodic = _tables(cx, entry)
    vgrid = vg._interp(y[:, cols], table, lower, spacing, periodic)[0]
    if entry == GRID:
        (gx,) = torch.autograd.grad(vgrid.sum(), xx)
        return {"out": y.detach(), "bias": vgrid.detach(), "grad_x": gx}
    d = _wrapped(y - data["center"], data["period"])
    d = torch.where(d.abs() <= data["flat"], torch.zeros_like(d), torch.copysign(d.abs() - data["flat"], d))
    e_r = 0.5 * (data["kappa"] * d * d).sum(1)
    if entry == BIAS_OPES:
        (gx,) = torch.autograd.grad((e_r + vgrid + v_o).sum(), xx)
        return {"out": y.detach(), "energies": torch.stack([e_r, torch.zeros_like(e_r), vgrid, v_o], 1).detach(), "grad_x": gx}
    dh = y[:, HILLS_COLUMNS].unsqueeze(1) - data["centers"].unsqueeze(0)
    v_h = (data["heights"] * torch.exp(-0.5 * ((dh / data["sigma"]) ** 2).sum(2))).sum(1)
    (gx,) = torch.autograd.grad((e_r + v_h + vgrid).sum(), xx)
    return {"out": y.detach(), "energies": torch.stack([e_r, v_h, vgrid], 1).detach(), "grad_x": gx}


def _held(cx, entry, bufs, got, what, kept=None):
    """_against_oracle at that file's tolerances; the new entries bring their reference, and their energies - values, which that
    file's table does not know - are held to the float64 value bound 1e-10 max(1, |E|max) as well."""
    if entry in NEW and (kept is None or "want" not in kept):
        kept = {} if kept is None else kept
        kept.update(want=_want2(cx, entry, dict((name, p.cpu().double()) for name, role, p in bufs if role == "in")), own=None)
    bad = _against_oracle(cx, entry, bufs, got, what, kept)
    if "energies" in got:
        w = kept["want"]["energies"]
        err = float((got["energies"].cpu().double() - w).abs().max()) / max(1.0, float(w.abs().max()))
        if not err <= 1e-10:
            bad.append("%s energies: error %.3g over 1e-10" % (what, err))
    return bad


def _shared_inputs_written(entry, bufs, views):
    """The OPES entries' inputs that no frame owns - the kernel table, the state every block reads - that a launch changed"""
    if entry not in OPES_ENTRIES:
        return []
    return ["%s: the shared input %s was written" % (entry, name) for name, role, payload in bufs
            if role == "in" and name not in iso.PER_FRAME and not bp.pl.same_bits(views[name].cpu(), payload.to(views[name].dtype))]


@contextlib.contextmanager
def _svd_that_returns_nan():
    """torch.linalg.svd refuses a matrix that is not finite; inside, such a matrix of a batch gets NaN factors (and NaN gradients:
    0 * NaN), every other matrix what torch.linalg.svd gives it."""
    real = torch.linalg.svd

    def svd(a, *args, **kw):
        finite = torch.isfinite(a).all(-1).all(-1)
        u, s, vh = real(torch.where(finite[..., None, None], a, torch.eye(a.shape[-1], dtype=a.dtype).expand_as(a)), *args, **kw)
        taint = a.sum((-1, -2)) * 0.0                        # NaN where the matrix is not finite, 0.0 elsewhere
        return u + taint[..., None, None], s + taint[..., None], vh + taint[..., None, None]

    torch.linalg.svd = svd
    try:
        yield
    finally:
        torch.linalg.svd = real


def _want_poisoned(cx, entry, data):
    """The reference of a poisoned batch, as the module's docstring defines it"""
    with _svd_that_returns_nan():
        want = _want2(cx, entry, dict((k, v.cpu().double()) for k, v in data.items()))
    return dict((k, v.detach()) for k, v in want.items())


# ---- the small batch -----------------------------------------------------------------------------------------------------------------
def _where(cx, bufs):
    """{per-frame input: the flat element of a frame's row that is poisoned}, and the chosen atom"""
    atom = iso.chosen_atom(cx.align, cx.items) if cx.kind != "head" else None
    return dict((name, 3 * atom + iso.COORD if name in ("x", "u", "v") else 0) for name, role, _ in bufs
                if role == "in" and name in iso.PER_FRAME), atom


def _bond_only_atom(cx):
    """An atom that a bond names and no angle, dihedral or position item does (None without one): its frame's bond is NaN and no
    other item covers the bond's gradient rows."""
    if cx.kind != "model":
        return None
    other = {a for t, atoms in cx.items if t != bp.BOND for a in atoms}
    lone = [a for t, atoms in cx.items if t == bp.BOND for a in atoms if a not in other]
    return lone[0] if lone else None


def _with(bufs, data):
    return [(name, role, data[name] if role == "in" else payload) for name, role, payload in bufs]


def _rows(t, name, idx):
    return t.movedim(iso.frame_dim(name), 0)[torch.as_tensor(idx, dtype=torch.long, device=t.device)].movedim(0, iso.frame_dim(name))


def _small(cx, entry, pattern):
    family, n = cx.family, N_SMALL
    what = "%s %s n_inp=%d" % (family, entry, cx.n_inp)
    spec = _entry2(cx, entry, n)
    bufs, call, plan = spec
    rc, _, info, views, _ = _launch(cx, entry, n, 0, spec, fresh=True)
    assert rc == 0, (what, rc, _capi.error_string(rc))
    assert re.search(pattern, info), (what, info, pattern)
    clean, kept = _outputs(bufs, views), {}
    bad = _held(cx, entry, bufs, clean, what, kept) + _shared_inputs_written(entry, bufs, views)
    bad += ["%s: clean %s is not finite" % (what, k) for k, v in clean.items() if not bool(torch.isfinite(v).all())]
    bad += ["%s: the reference's %s is not finite" % (what, k) for k, v in kept["want"].items() if not bool(torch.isfinite(v).all())]
    rc, _, _, views, _ = _launch(cx, entry, n, 0, spec, fresh=True)
    assert rc == 0, (what, "the second clean launch", rc)
    again = _outputs(bufs, views)
    if family not in ATOMICS:
        bad += ["%s: %s differs between two clean launches" % (what, k) for k in clean
                if not ((family, entry) in TILE_ORDER and k in iso.SUMS) and not bp.pl.same_bits(clean[k], again[k])]
    if bad:                                                 # no keep row may be excused: everything below rests on this
        return bad
    inputs = dict((name, payload) for name, role, payload in bufs if role == "in")
    where, atom = _where(cx, bufs)
    shapes = dict((name, payload) for name, role, payload in bufs if role != "in")
    per_frame = [k for k in clean if k not in iso.SUMS]
    targets = [(buffer, where, atom) for buffer in where]
    lone = _bond_only_atom(cx)
    if "x" in where and lone is not None:                   # x once more, at an atom that nothing but a bond names
        targets.append(("x", dict(where, x=3 * lone + iso.COORD), lone))
    for buffer, where, atom in targets:
        masks = dict((v, iso.dependent_elements(cx, entry, atom, shapes, buffer, where[buffer], v)) for v in ("nan", "inf"))
        if entry == BIAS_OPES:                               # the column of the hills, which this entry does not have, is 0.0
            for m in masks.values():
                m["energies"][1] = False
        for bad_set in BAD_SETS:
            tag = "%s, %s%s of frames %s poisoned" % (what, buffer, " (atom %d)" % atom if buffer == "x" else "", list(bad_set))
            data = iso.poison(inputs, bad_set, "mixed", where=where, only=(buffer,))
            rc, _, info2, views, _ = _launch(cx, entry, n, 0, (_with(bufs, data), call, plan), fresh=True)
            assert rc == 0 and info2 == info, (tag, rc, info2)
            got = _outputs(bufs, views)
            bad += ["%s: %s" % (tag, c) for c in _shared_inputs_written(entry, _with(bufs, data), views)]
            keep = sorted(set(range(n)) - set(bad_set))
            if family in ATOMICS:
                sub = {"want": dict((k, _rows(v.reshape(shapes[k]), k, keep)) for k, v in kept["want"].items()),
                       "own": dict((k, _rows(v.reshape(shapes[k]), k, keep)) for k, v in kept["own"].items()) if kept["own"] else None}
                bad += _against_oracle(cx, entry, bufs, dict((k, _rows(got[k], k, keep)) for k in per_frame), tag, sub)
                bad += ["%s: kept rows of %s are not finite" % (tag, k) for k in per_frame if not bool(torch.isfinite(_rows(got[k], k, keep)).all())]
            else:
                bad += ["%s: %s" % (tag, c) for c in iso.keep_rows_equal(clean, got, bad_set, per_frame)]
            values = dict((f, iso.value_of(f, "mixed")) for f in bad_set)
            bad += ["%s: %s" % (tag, c) for c in iso.not_non_finite(got, masks, bad_set, values)]
            want = _want_poisoned(cx, entry, data)
            lenient = 0
            for k in per_frame:
                g, w = _rows(got[k], k, bad_set).cpu(), _rows(want[k].reshape(shapes[k]), k, bad_set)
                lenient += int((torch.isfinite(g) & ~torch.isfinite(w)).sum())
            print("isolation %s: %d elements of the bad rows are finite where the reference is not" % (tag, lenient))
            for k in iso.SUMS:
                if k in got and buffer in ("x", "f"):
                    missing = int((torch.isnan(want[k].reshape(-1)) & torch.isfinite(got[k].cpu().reshape(-1))).sum())
                    if missing:
                        bad.append("%s: %d elements of %s are finite where the reference's sum is NaN" % (tag, missing, k))
    return bad


# ---- the dense batch -----------------------------------------------------------------------------------------------------------------
class Dense(object):
    """A case whose per-frame data are BASE seeded frames repeated on the device (as tools/check_large_batch.py builds its batch)"""

    def __init__(self, cx):
        self.real = cx

    def __getattr__(self, name):
        return getattr(self.real, name)

    def _tiled(self, base, dim, n):
        t = base.to(self.real.dev)
        reps = [1] * t.dim()
        reps[dim] = -(-n // BASE)
        return t.repeat(reps).narrow(dim, 0, n).contiguous()

    def x(self, n, entry):
        return self._tiled(self.real.x(BASE, entry), 0, n)

    def randn(self, shape, entry, n, salt=0):
        if n not in shape:
            return self.real.randn(shape, entry, n, salt)
        dim = list(shape).index(n)
        return self._tiled(self.real.randn(tuple(BASE if i == dim else s for i, s in enumerate(shape)), entry, BASE, salt), dim, n)


I = int
# (launch-info pattern of one kernel, groups -> (grid, frames a block takes per round, rounds per generation of its ring))
GEOMETRY = [
    (r"^(molann_lane_jit<[^>]*>|molann_bwd_ring(?:<values>)?) .*ring of (\d+) tiles.* grid=(\d+)", lambda m: (I(m[3]), 64, I(m[2]))),
    (r"^(frames_ring_kernel)<ND=\d+> .*ring of (\d+) frames.* grid=(\d+)", lambda m: (I(m[3]), 1, I(m[2]))),
    (r"^(frames_ring_kernel)<ND=\d+,B=(\d+)> .*ring of (\d+) entries.* grid=(\d+)", lambda m: (I(m[4]), I(m[2]), I(m[3]))),
    (r"^(frames_align_batch_kernel)<U=\d+,B=(\d+)> .* grid=(\d+)", lambda m: (I(m[3]), I(m[2]), 1)),
    (r"^(frames_align_regs_kernel|frames_align_bwd_regs_kernel)<.* grid=(\d+)", lambda m: (I(m[2]), 1, 1)),
    (r"^(frames_lane_kernel|mlp_lane_kernel|molann_lane_bwd|molann_mlp_bwd)\b.* grid=(\d+) block=(\d+)", lambda m: (I(m[2]), I(m[3]), 1)),
    (r"^(frames_wave_kernel|frames_wave_bwd_gather_kernel|frames_wave_bwd_kernel)\b.* grid=(\d+) block=(\d+)", lambda m: (I(m[2]), I(m[3]) // 64, 1)),
    (r"^(frames_group_bwd_kernel)<B=(\d+)>.* grid=(\d+) block=(\d+)", lambda m: (I(m[3]), I(m[2]) * I(m[4]) // 64, 1)),
    (r"^(molann_mlp_chain)<\w+,FB=(\d+).* grid=(\d+) block=(\d+)", lambda m: (I(m[3]), I(m[4]) // 4 * I(m[2]), 1)),     # tiles of 16 waves FB
    (r"^(mlp_mfma_kernel)<.* grid=(\d+) block=(\d+)", lambda m: (I(m[2]), I(m[3]) // 4, 1)),                           # 16 frames per wave
    (r"^(molann_chain_bwd) .* grid=(\d+) block=(\d+)", lambda m: (I(m[2]), I(m[3]) // 4, 1)),                          # tiles of 16 waves
    (r"^(molann_group_vjp)<.* grid=(\d+)", lambda m: (I(m[2]), 64, 1)),
    (r"^(\w+) \((?:values \+ [^;]*; )?(\d+) lanes per frame.* grid=(\d+) block=(\d+)", lambda m: (I(m[3]), I(m[4]) // I(m[2]), 1)),
    (r"^(mlp_f64_kernel) grid=(\d+) block=(\d+)", lambda m: (I(m[2]), I(m[3]) // 64, 1)),                            # a wave per frame
    # these name the bound of the grid (negative here), so that their text does not depend on n: grid = min(rounds needed, bound)
    (r"^(frames_f64_kernel|frames_bwd_f64_kernel)\b.* grid<=(\d+) block=(\d+)", lambda m: (-I(m[2]), I(m[3]) // 64, 1)),
]


def _known_kernel(segment):
    name = re.match(r"\w+", segment)
    return bool(name) and any(re.search(r"[(|]%s[)|<\\ ]" % re.escape(name.group(0)), pattern) for pattern, _ in GEOMETRY)


def _geometry(info, n, dev):
    """[(kernel, grid, frames per block and round, rounds per ring generation, rounds every block runs)] of the launch info's kernels,
    the chunk of a chunked launch (or None), the segments no pattern read."""
    chunk = re.search(r"chunk=(\d+)|chunks of (\d+) frames", info)
    chunk = int(chunk.group(1) or chunk.group(2)) if chunk else None
    n_eff = min(n, chunk) if chunk else n
    found, unread = [], []
    for seg in info.split(" || "):
        for pattern, read in GEOMETRY:
            m = re.search(pattern, seg)
            if m:
                grid, per_round, ring = read(m)
                if grid < 0:
                    grid = min(-(-n_eff // per_round), -grid)
                found.append((m.group(1), grid, per_round, ring, n_eff // (grid * per_round)))
                break
        else:
            if not seg.startswith("chunk"):
                unread.append(seg)
    return found, chunk, unread


def _dense(cx, entry, pattern):
    family = cx.family
    what = "%s %s n_inp=%d dense" % (family, entry, cx.n_inp)
    proxy, n = Dense(cx), N_FIRST
    for _ in range(8):
        spec = _entry2(proxy, entry, n)
        bufs, call, plan = spec
        sizes = dict((name, (p.numel() if role == "in" else int(np.prod(p))) * (8 if cx.f64 else 4)) for name, role, p in bufs)
        # the widest outputs here (the Jacobian of the mid frames, 16 KB per frame) reach three rounds under the limit with every head
        # output kept, so no output's width is cut
        assert max(sizes.values()) < ONE_GB, (what, n, sizes)
        row_bytes = max(v // n for k, v in sizes.items() if k in iso.PER_FRAME or dict((b[0], b[1]) for b in bufs)[k] != "in")
        rc, _, info, views, _ = _launch(cx, entry, n, 0, spec, fresh=True)
        assert rc == 0, (what, n, rc, _capi.error_string(rc))
        assert re.search(pattern, info), (what, info, pattern)
        shared = _shared_inputs_written(entry, bufs, views)
        found, chunk, unread = _geometry(info, n, cx.dev)
        # a composite launch info cuts its parts short: a part without its geometry must still start with the name of a kernel the
        # table reads (that kernel has its own entry), and every part that names a geometry must have been read
        assert found and all("grid" not in s and _known_kernel(s) for s in unread), (what, info, unread)
        # the largest batch of one launch: a buffer under 1 GB, and what the plan's chunked workspace takes at a time
        n_cap = min((ONE_GB - 1) // row_bytes, chunk or (1 << 62)) - 72
        needs = [3 * ring * grid * per_round for _, grid, per_round, ring, _ in found]
        need = max([v for v in needs if v <= n_cap] or [0])
        if n >= need:
            break
        n = -(-need // 64) * 64 + 8                        # and a short last tile
    else:
        raise AssertionError((what, "no N with three rounds per block", n, info))
    # every kernel of the launch ran its three rounds (three generations of its ring), except a kernel that would need a batch past
    # the cap for them: the second kernel of a composite launch, which has an entry of its own in the table
    assert needs[0] <= n_cap and all(rounds >= 3 * ring or v > n_cap for (_, _, _, ring, rounds), v in zip(found, needs)), (what, n, n_cap, info, found)
    g = torch.Generator().manual_seed(bp.zlib.crc32(what.encode()) & 0xFFFF)
    keep = sorted({0, 63, 64, n - 1} | set(torch.randint(0, n, (30,), generator=g).tolist()))
    keep_t = torch.tensor(keep, device=cx.dev)
    per_frame = [name for name, role, _ in bufs if role != "in" and name not in iso.SUMS]
    clean = dict((k, _rows(views[k], k, keep_t).clone()) for k in per_frame)
    mask = torch.ones(n, dtype=torch.bool, device=cx.dev)
    mask[keep_t] = False
    inputs = dict((name, payload) for name, role, payload in bufs if role == "in")
    where, _ = _where(cx, bufs)
    data = iso.poison(inputs, mask, "mixed", where=where)
    del views
    rc, _, info2, views, _ = _launch(cx, entry, n, 0, (_with(bufs, data), call, plan), fresh=True)
    assert rc == 0 and info2 == info, (what, rc, info2)
    got = dict((k, _rows(views[k], k, keep_t).clone()) for k in per_frame)
    bad = shared + _shared_inputs_written(entry, _with(bufs, data), views)
    bad += ["%s: kept rows of %s are not finite" % (what, k) for k in per_frame if not bool(torch.isfinite(got[k]).all())]
    if family in ATOMICS:
        sub = [(name, role, _kept_shape(p, name, len(keep)) if role != "in" else (_rows(p, name, keep_t).cpu() if name in iso.PER_FRAME else p))
               for name, role, p in bufs]
        bad += _held(cx, entry, sub, got, what)
    else:
        bad += ["%s (kept frames %s): %s" % (what, keep, c) for c in iso.keep_rows_equal(clean, got, [], per_frame)]
    print("isolation %s: N = %d, %s%s" % (what, n, "; ".join("%s grid=%d x %d frames, %d rounds per block (ring of %d)" % f for f in
                                                             [(k, gr, pr, ro, ri) for k, gr, pr, ri, ro in found]),
                                           ", chunks of %d" % chunk if chunk else ""))
    DENSE[(family, entry)] = (n, found[0][4], chunk)
    return bad


def _kept_shape(shape, name, n_keep):
    shape = list(shape)
    shape[iso.frame_dim(name)] = n_keep
    return tuple(shape)


# ---- the tests -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,n_inp,tail", CASES, ids=["%s-%d-%d" % c for c in CASES])
def test_a_non_finite_frame_changes_no_other(family, n_inp, tail, hip_device, monkeypatch):
    cx = _ctx(family, n_inp, tail, hip_device, monkeypatch)
    bad = []
    for entry, pattern in _patterns(cx).items():
        found = len(bad)
        bad += _small(cx, entry, pattern)
        if len(bad) == found:
            SMALL.add((family, entry))
        found = len(bad)
        bad += _dense(cx, entry, pattern)
        if len(bad) > found:
            DENSE.pop((family, entry), None)
        torch.cuda.empty_cache()
    for complaint in bad:
        print("isolation FAILED: " + complaint)
    assert not bad, (len(bad), bad[:12])


def test_every_family_and_entry_was_reached(request):
    """Both phases passed for every (family, entry) of the placement table and the five entries added here; the families are recorded
    as they pass, so this guard needs all of them in the same session."""
    here = {item.name for item in request.session.items if item.module is request.module}
    wanted = {"test_a_non_finite_frame_changes_no_other[%s-%d-%d]" % c for c in CASES}
    if not wanted <= here:
        pytest.skip("the coverage guard needs every family in this session: %d not selected" % len(wanted - here))
    want = {(f, e) for f, v in FAMILIES.items() for e in v[5]} | {(f, e) for f, v in EXTRA.items() for e in v}
    assert {(f, e) for f in EXTRA for e in NEW} <= want and len(NEW) == 5
    missing = sorted((want - SMALL) | (want - set(DENSE)))
    assert not missing, ("not reached:", missing)
    for (f, e), (n, rounds, chunk) in sorted(DENSE.items()):
        print("isolation covered %s %s: dense N = %d, at least %d rounds per block%s" % (f, e, n, rounds, ", chunks of %d" % chunk if chunk else ""))
