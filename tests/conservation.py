"""Net force and net torque of a gradient, for the tests of every kernel that hands out dL/dx (tests/test_conservation_host.py,
tests/test_gpu_conservation.py).

A value that does not change under rigid motions of the frame (features of Kabsch-aligned coordinates, bonds, angles, dihedrals,
and anything computed from them) has a gradient F = dL/dx with, per frame and in exact arithmetic,

    sum_a F_a = 0                     (translations)
    sum_a (x_a - c) x F_a = 0         (rotations, about any point c)

`residuals` measures both, relative to sum |F_a| and sum |x_a - c| |F_a|, in float64 on the CPU from the exact input values.  A
kernel's residuals are held to `bound`: a few times the residuals of the oracle's autograd in the same precision on the same frames
with the same cotangent, never to anything a kernel computed.  Nothing here imports GPU code."""

import numpy as np
import torch

import far_frames as ff
from molann_amd import workloads as wl

U = {32: 2.0 ** -24, 64: 2.0 ** -53}                       # unit roundoff
FLOOR, FACTOR = 16.0, 4.0
KEEP = 0.75                                                # the share of every regime's frames the selection has to keep
CONDITIONING = 0.05                                        # as test_gpu_far_frames._cotangent


def _f64(t):
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().double().numpy()
    return np.asarray(t, np.float64)


def residuals(x, F):
    """(r_F, r_T) per frame for frames x [n, atoms, 3] and forces F [n, atoms, 3], or per frame and row for F [n, k, atoms, 3]
    (each row of a Jacobian is a force).  r_F = |sum F_a| / sum |F_a|, r_T = |sum (x_a - c) x F_a| / sum |x_a - c| |F_a| with c
    the mean of the atoms whose row of F is nonzero.  NaN where sum |F_a| = 0 (use np.nanmax)."""
    x, F = _f64(x), _f64(F)
    rows = F.ndim == 4
    if not rows:
        F = F[:, None]
    x = x[:, None]                                         # [n, 1, atoms, 3]
    norm = np.linalg.norm(F, axis=-1)                      # [n, k, atoms]
    live = norm > 0
    cnt = live.sum(-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        c = (x * live[..., None]).sum(-2) / cnt[..., None]  # [n, k, 3]
        r = x - c[:, :, None, :]
        sF = norm.sum(-1)
        r_F = np.linalg.norm(F.sum(-2), axis=-1) / sF
        torque = np.cross(r, F).sum(-2)
        r_T = np.linalg.norm(torque, axis=-1) / (np.linalg.norm(r, axis=-1) * norm).sum(-1)
    dead = sF == 0
    r_F[dead], r_T[dead] = np.nan, np.nan
    return (r_F, r_T) if rows else (r_F[:, 0], r_T[:, 0])


def _units(rng, shape):
    v = rng.standard_normal(tuple(shape) + (3,))
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def rigid_tangent(x, seed):
    """v_a = w x (x_a - c) + t, a random unit w and t per frame, c the frame's centroid: the velocity of a rigid motion.
    float64 [n, atoms, 3]."""
    x = _f64(x)
    rng = np.random.default_rng([seed, 1])
    w, t = _units(rng, (len(x), 1)), _units(rng, (len(x), 1))
    return np.cross(w, x - x.mean(1, keepdims=True)) + t


def shuffled_tangent(v, seed):
    """A tangent with v's per-atom norms and random directions (what a JVP along v is normalised with)."""
    v = _f64(v)
    rng = np.random.default_rng([seed, 2])
    return np.linalg.norm(v, axis=-1, keepdims=True) * _units(rng, v.shape[:-1])


def _per_frame(r):
    r = np.asarray(r, np.float64)
    if r.ndim > 1:                                         # Jacobian rows: the frame's largest
        allnan = np.isnan(r).all(1)
        r = np.where(allnan, np.nan, np.nanmax(np.where(np.isnan(r), -np.inf, r), axis=1))
    return r


def bound(ref_residuals, labels, u):
    """{regime: max(16 u, 4 x the reference's largest residual over the regime's frames)}.  The reference is the oracle's autograd
    in the kernel's precision, on the same frames, with the same cotangent.  4: a kernel adds the same terms in another order, and
    uses one-ulp hardware reciprocals and reciprocal square roots where the reference divides; each at most doubles a
    rounding-level residual.  16 u: a lucky reference batch sets no bound below rounding."""
    r = _per_frame(ref_residuals)
    labels = np.asarray(labels)
    assert r.shape == labels.shape, (r.shape, labels.shape)
    out = {}
    for reg in sorted(set(labels.tolist())):
        m = (labels == reg) & ~np.isnan(r)
        out[reg] = max(FLOOR * u, FACTOR * float(r[m].max())) if m.any() else FLOOR * u
    return out


def largest(res, labels):
    """{regime: the largest residual over the regime's frames} (NaN frames left out)"""
    r = _per_frame(res)
    labels = np.asarray(labels)
    return {reg: float(np.nanmax(r[labels == reg])) if (~np.isnan(r[labels == reg])).any() else 0.0 for reg in sorted(set(labels.tolist()))}


def exceeding(res, labels, bounds):
    """[(frame, regime, residual, bound)] of the frames over their regime's bound"""
    r = _per_frame(res)
    return [(i, l, float(r[i]), bounds[l]) for i, l in enumerate(labels) if not np.isnan(r[i]) and not r[i] <= bounds[l]]


def poles(x, feats, angles=False):
    """Per frame: a dihedral with a bond angle within about three degrees of 0 or 180 (as test_gpu_random_backward._dihedral_poles);
    with `angles`, such an angle item too (plans that output the angle's value, whose derivative has the same pole)"""
    x = _f64(x)
    bad = np.zeros(len(x), bool)
    for t, idx in feats:
        triples = (idx[:3], idx[1:]) if t == wl.DIHEDRAL else ((idx,) if angles and t == wl.ANGLE else ())
        for a, b, c in triples:
            p, q = x[:, a] - x[:, b], x[:, c] - x[:, b]
            bad |= np.linalg.norm(np.cross(p, q), axis=1) < 0.05 * np.linalg.norm(p, axis=1) * np.linalg.norm(q, axis=1)
    return bad


def reference_conditioning(xyz, align):
    """(proper, mirror): far_frames.conditioning of the reference against itself, (s2 + s3) / s1, and against its mirror image,
    (s2 - s3) / s1, from the centred align atoms"""
    r = np.asarray(xyz, np.float64)[list(align)]
    r = r - r.mean(0)
    s = np.linalg.svd(r.T @ r, compute_uv=False)
    return (s[1] + s[2]) / s[0], (s[1] - s[2]) / s[0]


def select(frames, labels, xyz, align, feats, what="", rotation=True, angles=False):
    """The frames a conservation check runs on: rotation well conditioned (far_frames.conditioning >= 0.05; every frame of a plan
    without alignment) and no dihedral at a pole.  At least 75 % of every regime's frames stay, or the case fails: there is no
    exemption.  rotation=False leaves the conditioning filter out, for a check of the net force alone: sum_a F_a = 0 comes from the
    centring, exactly, however the rotation is conditioned.  Returns the mask [n] and {regime: (kept, of, lost to the pole filter
    alone)}."""
    n = len(frames)
    aligned = rotation and align is not None and len(align) > 0
    cond = ff.conditioning(frames, xyz, align) >= CONDITIONING if aligned else np.ones(n, bool)
    pole = poles(frames, feats, angles)
    keep = cond & ~pole
    labels = np.asarray(labels)
    share = {}
    for reg in sorted(set(labels.tolist())):
        m = labels == reg
        share[reg] = (int(keep[m].sum()), int(m.sum()), int((cond & pole)[m].sum()))
        assert share[reg][0] >= KEEP * share[reg][1] and share[reg][0] > 0, (what, reg, "kept %d of %d frames (%d lost to poles)" % share[reg])
    return keep, share


def far_regimes(xyz, align):
    """(the far regimes of the mixed batch, the regime of the single far frames).  hinge / mirror / offset and mirror, as
    tests/test_gpu_far_frames.py; an align set whose own mirror image is ill-conditioned ((s2 - s3) / s1 of the reference under the
    threshold: no mirror frame can pass the selection) takes exact 180-degree turns in mirror's place."""
    if align is not None and len(align) and reference_conditioning(xyz, align)[1] < CONDITIONING:
        return ("hinge", "flip180", "offset"), "flip180"
    return ("hinge", "mirror", "offset"), "mirror"


REDRAWS = 8


def _passes(frames, xyz, align, feats, rotation, angles):
    ok = ~poles(frames, feats, angles)
    if rotation and align is not None and len(align):
        ok &= ff.conditioning(frames, xyz, align) >= CONDITIONING
    return ok


def batches(xyz, align, n, seed, feats=(), rotation=True, angles=False, redrawn=None):
    """{"mixed": (labels, frames), "single": (labels, frames)}: far_frames.interleaved, and a near batch with one far frame (see
    far_regimes) at 0, 63, 64 and the last position.  float32 [n, atoms, 3].  A frame that `select` (called with the same feats,
    rotation and angles) would drop - a hinge frame that is an independent, ill-conditioned conformation; one of a plan's many
    dihedrals at a pole - is drawn again, same regime, same position, from the next seed, up to REDRAWS times: the batches keep their
    size and their regimes, and the selection's share holds by construction rather than by the choice of a seed.  A frame drawn again
    comes from a batch composed without `base`: a near frame of the single batch then sits on another draw's conformation, not on
    the mixed batch's row, which no check here relies on.  `redrawn`, a dict, receives {batch: frames drawn again}."""
    al = list(align) if align is not None else []
    near = ff.draw("near", xyz, al, n, seed=seed)
    far, one = far_regimes(xyz, align)
    out = {}
    for name, lab, s in (("mixed", ff.interleaved(n, far=far), 7), ("single", ff.single(n, one), 9)):
        x = ff.compose(lab, xyz, al, seed=s + 16 * seed, base=near)
        first = None
        for r in range(1, REDRAWS + 1):
            bad = ~_passes(x, xyz, align, feats, rotation, angles)
            first = int(bad.sum()) if first is None else first
            if not bad.any():
                break
            x[bad] = ff.compose(lab, xyz, al, seed=s + 16 * seed + 4096 * r)[bad]
        if redrawn is not None:
            redrawn[name] = first
        out[name] = (lab, x)
    return out


def cotangent(shape, seed, dtype):
    """A random cotangent, nonzero on every frame"""
    G = torch.from_numpy(np.random.default_rng([seed, 3]).standard_normal(shape)).to(dtype)
    assert bool((G.reshape(shape[0], -1) != 0).any(1).all())
    return G


def check(x, F, F_ref, labels, keep, bits, what, torque=True, regimes=None):
    """Hold F's residuals on the kept frames to `bound` of F_ref's, per regime.  Returns {regime: (r_F, ref r_F, r_T, ref r_T)} and
    raises on a frame past its bound, or on a regime (of `labels`, or of `regimes` when the caller has filtered them) with no kept
    frame."""
    keep = np.asarray(keep, bool)
    lab = [l for l, k in zip(labels, keep) if k]
    assert lab and set(lab) == set(labels if regimes is None else regimes), (what, "a regime with no selected frame", sorted(set(lab)))
    xs = _f64(x)[keep]
    got, ref = residuals(xs, _f64(F)[keep]), residuals(xs, _f64(F_ref)[keep])
    assert not np.isnan(_per_frame(ref[0])).any(), (what, "the reference's force is zero on a selected frame")
    assert not np.isnan(_per_frame(got[0])).any(), (what, "the force is zero on a selected frame")
    table, bad = {}, []
    for k, name in ((0, "r_F"), (1, "r_T")):
        if k == 1 and not torque:
            continue
        b = bound(ref[k], lab, U[bits])
        bad += [(name,) + e for e in exceeding(got[k], lab, b)]
    lg = [largest(r, lab) for r in got + ref]
    for reg in sorted(set(lab)):
        table[reg] = (lg[0][reg], lg[2][reg], lg[1][reg], lg[3][reg])
    assert not bad, (what, "over the bound: (which, frame of the kept, regime, residual, bound)", bad[:6], table)
    return table
