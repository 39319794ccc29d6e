"""One non-finite frame in a batch: what a kernel may and may not do with it.

The kernels treat the frames of a batch as independent.  An exploded frame (a NaN or Inf coordinate, cotangent, tangent or feature)
must come back non-finite in the results that depend on it and must change no bit of any other frame's results.  A test on finite
data against a tolerance is blind to the commonest leak of kernels of this shape: a neighbour's value multiplied by an exact zero
instead of being selected away (K-padding of matrix operands, rows clamped to the last frame of a short tile, sub-wave reductions,
staging buffers that are zero-filled once and reused).  With finite data the product is invisible; 0 * NaN is not.

  poison(buffers, frames, kind)                      copies of an entry's per-frame inputs with the frames' rows made non-finite
  keep_rows_equal(clean, poisoned, frames, outputs)  complaints naming every per-frame output element outside `frames` that changed
  dependent_elements(cx, entry, atom, ...)           per output, the elements of a bad frame's own rows that must be non-finite

Per-frame inputs are those whose leading dimension is the frame (PER_FRAME); FRAME_DIM names the buffers whose frame is the second
dimension.  Everything else (weights, reference, tables, kappa, sigma ...) is shared by the frames and is never poisoned.

What `dependent_elements` does not name is not asserted: a plan whose items are all invariant under rigid motion may return a finite
bond where a reference that aligns first returns NaN, and +inf is not NaN: tanh(+-inf) is +-1, so behind a saturating activation an
Inf feature legitimately gives finite head outputs, d|r| / dr is 0 in the coordinates that stayed finite, and so on.  The `value`
argument says which of the two the frame got; the Inf rules keep only what every correct evaluation order leaves non-finite.

No GPU is needed to import or use this module."""

import torch

from molann_amd import workloads as wl
from oracle import molann_oracle as mo

PER_FRAME = ("x", "grad_out", "grad_f", "f", "g", "u", "center", "v")
FRAME_DIM = {"v": 1, "tangent_out": 1}                    # [T, N, n_inp, 3] and [T, N, d]; every other per-frame buffer: 0
SUMS = ("grad_params",)                                   # sums over the frames: not per-frame outputs
COORD = 1                                                 # the coordinate of the chosen atom that is made non-finite
KINDS = ("nan", "inf", "mixed")


def frame_dim(name, frame_dims=None):
    return (FRAME_DIM if frame_dims is None else frame_dims).get(name, 0)


def _index(frames, device):
    if isinstance(frames, torch.Tensor):
        return (frames.nonzero().flatten() if frames.dtype == torch.bool else frames.long()).to(device)
    return torch.tensor(sorted(int(f) for f in frames), dtype=torch.long, device=device)


def value_of(frame, kind):
    """"nan" or "inf": what `kind` puts into this frame (mixed: NaN into even frames, +inf into odd ones)."""
    if kind not in KINDS:
        raise ValueError("kind %r is none of %s" % (kind, KINDS))
    return kind if kind != "mixed" else ("nan", "inf")[int(frame) % 2]


def chosen_atom(align, items):
    """The atom of x that is poisoned: the first atom named by a feature item that is an alignment atom as well; without one, the
    first item atom; for a plan without items, the first alignment atom."""
    named = [a for _, atoms in items for a in atoms]
    both = [a for a in named if align is not None and a in set(align)]
    if both:
        return both[0]
    if named:
        return named[0]
    return list(align)[0]


def poison(buffers, frames, kind, where=None, only=None, frame_dims=None):
    """{name: tensor} with the rows of `frames` made non-finite in every per-frame input (or those of `only`): one element of the
    row - `where[name]`, a flat index into the frame's row, by default 0 - becomes NaN (kind "nan"), +inf ("inf") or, by the frame's
    parity, one of the two ("mixed").  Poisoned buffers are copies; shared inputs are returned as they are."""
    if kind not in KINDS:
        raise ValueError("kind %r is none of %s" % (kind, KINDS))
    out = dict(buffers)
    for name, t in buffers.items():
        if name not in PER_FRAME or (only is not None and name not in only):
            continue
        idx = _index(frames, t.device)
        c = t.clone()
        view = c.movedim(frame_dim(name, frame_dims), 0)              # a view: writes go through
        assert idx.numel() == 0 or (int(idx.min()) >= 0 and int(idx.max()) < view.shape[0]), (name, "frames outside the batch")
        flat, sub = int((where or {}).get(name, 0)), []
        for d in reversed(view.shape[1:]):
            sub.append(flat % d)
            flat //= d
        assert flat == 0, (name, "element outside the frame's row")
        nan = torch.full((idx.numel(),), float("nan"), dtype=t.dtype, device=t.device)
        if kind == "inf":
            vals = torch.full_like(nan, float("inf"))
        elif kind == "mixed":
            vals = torch.where(idx % 2 == 1, torch.full_like(nan, float("inf")), nan)
        else:
            vals = nan
        view[(idx,) + tuple(reversed(sub))] = vals
        out[name] = c
    return out


def _bits(t):
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


def keep_rows_equal(clean, poisoned, frames, outputs, frame_dims=None, limit=8):
    """Every per-frame output of `outputs`, bit for bit (compared as integers: NaN != NaN must hide nothing), on all frames outside
    `frames`.  Returns the complaints: at most `limit` per buffer, each naming buffer, frame and element, then the count."""
    bad = []
    for name in outputs:
        if name in SUMS:
            continue
        a, b = clean[name], poisoned[name]
        if a.shape != b.shape or a.dtype != b.dtype:
            bad.append("%s: shape or type changed, %s %s -> %s %s" % (name, tuple(a.shape), a.dtype, tuple(b.shape), b.dtype))
            continue
        fd = frame_dim(name, frame_dims)
        n = a.shape[fd]
        keep = torch.ones(n, dtype=torch.bool, device=a.device)
        keep[_index(frames, a.device)] = False
        ra, rb = (_bits(t.contiguous()).movedim(fd, 0).reshape(n, -1) for t in (a, b))
        diff = (ra != rb) & keep[:, None]
        if bool(diff.any()):
            at = diff.nonzero()
            fa, fb = a.movedim(fd, 0).reshape(n, -1), b.movedim(fd, 0).reshape(n, -1)
            for f, e in at[:limit].tolist():
                bad.append("%s: frame %d element %d changed from %r to %r" % (name, f, e, float(fa[f, e]), float(fb[f, e])))
            bad.append("%s: %d elements in %d kept frames changed" % (name, at.shape[0], int(diff.any(1).sum())))
    return bad


def leaking_frames(clean, poisoned, frames, outputs, frame_dims=None):
    """The kept frames with a changed bit in any per-frame output, sorted."""
    hit = set()
    for name in outputs:
        if name in SUMS:
            continue
        fd = frame_dim(name, frame_dims)
        n = clean[name].shape[fd]
        keep = torch.ones(n, dtype=torch.bool, device=clean[name].device)
        keep[_index(frames, keep.device)] = False
        ra, rb = (_bits(t.contiguous()).movedim(fd, 0).reshape(n, -1) for t in (clean[name], poisoned[name]))
        hit |= set((((ra != rb).any(1)) & keep).nonzero().flatten().tolist())
    return sorted(hit)


# ---- what of the bad frame's own rows must be non-finite -----------------------------------------------------------------------------
def _columns(items):
    """[(type, atoms, first column, width)] of the feature row (angles and dihedrals as cosines and sines)."""
    out, col = [], 0
    for t, atoms in items:
        w = mo.feature_dim(t, len(atoms), False)
        out.append((t, list(atoms), col, w))
        col += w
    return out


def _depends(cx, atom, value):
    """(feature columns, {atom: coordinates of its gradient row}, True when a NaN - not only an Inf - reaches the features) for a
    non-finite x[atom, COORD].  A position item's columns hold R (x - c): with the atom in the alignment the centroid c is
    non-finite and every column of the item is; without, the atom's own three are.  Its gradient rows R^T g are owed nothing: the
    rotation solver answers a covariance that is not finite with the identity (molann_math.h, "zero / non-finite covariance: no
    rotation", pinned by test_host_math.test_kabsch_rotation_degenerate_inputs_are_finite), so they do not see the atom.  A bond's
    value |r| turns NaN into NaN and every coordinate of its gradient g r / |r| with it; Inf it turns into Inf, and r / Inf is 0 in
    the coordinates where r stayed finite: only the poisoned coordinate of the rows is owed then.  An angle's or a dihedral's
    cosine turns Inf into Inf / Inf and every coordinate of its gradient carries it."""
    aligned = cx.align is not None and atom in set(cx.align)
    cols, rows, nan_reaches = set(), {}, False
    for t, atoms, c0, w in _columns(cx.items):
        if t == wl.POSITION:
            if aligned:
                cols |= set(range(c0, c0 + w))
                nan_reaches = True
                for a in atoms:
                    rows.setdefault(a, set())
            elif atom in atoms:
                j = atoms.index(atom)
                cols |= set(range(c0 + 3 * j, c0 + 3 * j + 3))
                nan_reaches = nan_reaches or value == "nan"
            continue
        if atom not in atoms:
            continue
        cols |= set(range(c0, c0 + w))
        nan_reaches = nan_reaches or value == "nan" or t != wl.BOND
        for a in atoms:
            rows.setdefault(a, set()).update((COORD,) if (t == wl.BOND and value == "inf") else (0, 1, 2))
    return cols, rows, nan_reaches


def _item_atoms(cx, col=None):
    """The atoms of the item that owns feature column `col` (a position item: the column's atom), or of every item."""
    out = set()
    for t, atoms, c0, w in _columns(cx.items):
        if col is None:
            out |= set(atoms)
        elif c0 <= col < c0 + w:
            out |= {atoms[(col - c0) // 3]} if t == wl.POSITION else set(atoms)
    return out


HEAD_ENTRIES = ("forward_packed", "forward_train", "backward_x", "backward_p", "backward_xp", "value_and_vjp", "forward_f64",
                "value_and_vjp_f64", "value_and_jacobian_f64", "value_and_metric_f64", "value_and_restraint_f64", "value_and_hills_f64",
                "value_and_grid_f64", "value_and_bias_f64", "value_and_opes_f64", "value_and_bias_opes_f64", "value_and_opes_table_f64")
FEATURE_OUT = {"features": "out", "features_f64": "out", "features_jvp": "out", "features_jvp_f64": "out", "forward_train": "features",
               "forward_f64": "work"}
SCALARS = ("energy", "bias", "energies", "metric")


def dependent_elements(cx, entry, atom, shapes, buffer="x", element=0, value="nan", frame_dims=None):
    """{output: bool mask over one frame's row of it} - the elements that must be non-finite when the frame's `buffer` holds `value`
    ("nan" or "inf") at x / u / v [atom, COORD], or at flat `element` of any other buffer's row.  `shapes`: {output: its full shape}.
    cx needs items, align, n_inp and dims (None without a head).  The rules, for x: feature columns whose item names the atom; every
    head output; the energy and bias scalars; grad_x (Jacobian, second-order) rows and tangent columns at atoms / items that share
    an item with it.  A cotangent reaches the rows of its column's item - behind a head, of every item; a feature row every head
    output.  Inf: see the module's docstring."""
    head = bool(getattr(cx, "dims", None)) and (entry in HEAD_ENTRIES or entry.startswith("mlp_"))
    masks = {}
    for name, shape in shapes.items():
        if name in SUMS:
            continue
        fd = frame_dim(name, frame_dims)
        masks[name] = torch.zeros([s for i, s in enumerate(shape) if i != fd], dtype=torch.bool)

    def rows(name, which):
        """mark rows {atom: coordinates} of a [..., n_inp, 3] output"""
        if name in masks:
            m = masks[name].reshape(-1, cx.n_inp, 3)
            for a, cs in which.items():
                for c in cs:
                    m[:, a, c] = True

    def everything(*names):
        for name in names:
            if name in masks:
                masks[name][...] = True

    full = lambda atoms: dict((a, (0, 1, 2)) for a in atoms)              # noqa: E731
    if entry in ("align", "align_f64"):
        if buffer == "x":                                                 # R (x - c): c is non-finite when the atom is aligned on
            if cx.align is not None and atom in set(cx.align):
                everything("out")
            else:
                rows("out", {atom: (0, 1, 2) if value == "nan" else (COORD,)})
        return masks
    if entry.startswith("mlp_"):                                          # f or grad_out of a head alone
        if buffer == "f" and value == "nan":
            everything("out", "grad_f")
        if buffer == "grad_out":
            everything("grad_f")                                          # linear in the cotangent: Inf stays non-finite
        return masks
    if buffer in ("x", "u", "v"):
        cols, grad_rows, nan_reaches = _depends(cx, atom, value if buffer == "x" else "nan")
        behind_head = head and (nan_reaches or buffer != "x")
        fo = FEATURE_OUT.get(entry)
        if buffer == "x":
            if fo in masks:
                masks[fo][..., sorted(cols)] = True
            if head and nan_reaches:
                everything(*(["out"] + [s for s in SCALARS if s in masks]))
            which = dict((a, cs) for a, cs in grad_rows.items() if cs)
            if behind_head:                                               # every feature's cotangent is NaN
                which = full(grad_rows)
            elif head:                                                    # only an Inf reaches a saturating head: act' = 0
                which = {}
            for name in ("grad_x", "jac", "hx"):
                rows(name, which)
            if "tangent_out" in masks:
                masks["tangent_out"][:, sorted(cols)] = True
            if "hg" in masks:
                masks["hg"][sorted(cols)] = True
        elif buffer == "v":                                               # tangent 0 of the frame; linear in v
            masks["tangent_out"][0, sorted(cols)] = True
        else:                                                             # u of the second-order entry: hx = H u, hg = J u
            rows("hx", full(a for a, cs in grad_rows.items() if cs))
            masks["hg"][sorted(cols)] = True
        return masks
    # a cotangent (grad_out, grad_f, g) or the restraint's centre: linear in it (the centre's wrap: Inf - Inf), Inf stays non-finite
    atoms = _item_atoms(cx) if head else _item_atoms(cx, element)
    for name in ("grad_x", "hx"):
        rows(name, full(atoms))
    if buffer == "center":
        if "energy" in masks:
            everything("energy")
        if "energies" in masks:
            masks["energies"][0] = True                                   # the restraint's term alone
    return masks


def not_non_finite(got, masks, frames, values=None, frame_dims=None, limit=6):
    """Complaints about dependent elements (`masks`: one per output, or {"nan": masks, "inf": masks} picked per frame by `values`
    {frame: "nan" | "inf"}) of the bad frames that are finite."""
    bad = []
    per_value = masks if set(masks) <= {"nan", "inf"} and masks else {"nan": masks, "inf": masks}
    idx = _index(frames, torch.device("cpu")).tolist()
    for name in next(iter(per_value.values())):
        fd = frame_dim(name, frame_dims)
        t = got[name].movedim(fd, 0)
        rows = t[torch.tensor(idx, dtype=torch.long, device=t.device)].cpu()
        for k, f in enumerate(idx):
            m = per_value[(values or {}).get(f, "nan")][name]
            wrong = torch.isfinite(rows[k]) & m
            if bool(wrong.any()):
                if len(bad) < limit:
                    e = wrong.flatten().nonzero().flatten()
                    bad.append("%s: frame %d has %d finite dependent elements (the first: %d = %r)"
                               % (name, f, e.numel(), int(e[0]), float(rows[k].flatten()[e[0]])))
    return bad
