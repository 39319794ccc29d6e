"""Frames whose angles and dihedrals sit at the places where the item arithmetic (molann_amd/csrc/molann_math.h) is hardest, built
by construction for the tests of every kernel family that calls it (tests/test_angular_edges_host.py, test_gpu_angular_edges.py).

A plan's edge items are its first angle, its first dihedral (`tc`) and its second dihedral (`arm`).  Each has an end atom of its
own - the angle's third atom, the tc dihedral's fourth, the arm dihedral's first - that no other item and no alignment set names,
so moving it changes that item alone and leaves the fit as well conditioned as it was.  `draw` starts from near frames (the
reference + 0.2 A of noise, far_frames.draw), re-places the end atom of the regime's item from internal coordinates (the bond
length kept, the angle and the dihedral prescribed, the perpendicular random) and moves every frame rigidly once more:

  straight / folded   the angle item at pi - delta / delta
  trans / cis         the tc dihedral at +-(pi - delta) / +-delta, signs alternating from frame to frame, its arm angle kept
  arm                 the arm dihedral's 1-2-3 angle at pi - delta, the dihedral itself kept (a generic value)

delta is in degrees.  GRADED are the distances from the pole at which the answers are ill-conditioned and still well defined in
float32; POLE those at which the float32 reference gives NaN gradients on some frames (0.03 degrees) or on most (0).  A dihedral at
cis / trans is not ill-conditioned at all (atan2 wraps there, nothing divides by a small number), so `grades` gives those regimes
every distance down to 0 as graded.  All frames are float32 [n, n_atoms, 3] from a seed; `sines` [n, n_items] holds, in float64
and for the float32 frames as stored, sin of each angle item's angle and the smaller sin of each dihedral's two arm angles (1 for
bonds and positions): what the float64 bounds eps / sin^2 are formed from."""

import numpy as np

import far_frames as ff

ANGLE, BOND, DIH, POS = 0, 1, 2, 3
REGIMES = ("straight", "folded", "trans", "cis", "arm")
GRADED = (10.0, 3.0, 1.0, 0.3, 0.1)
POLE = (0.03, 0.0)
TC_EXTRA = (1e-2, 1e-4, 0.0)


def grades(regime):
    """(graded deltas, pole deltas) of a regime, in degrees."""
    if regime in ("trans", "cis"):
        return GRADED + (POLE[0],) + TC_EXTRA, ()
    return GRADED, POLE


def roles(items):
    """{'angle': i, 'tc': j, 'arm': k}: the positions of the edge items in `items` [(type, atoms)]."""
    ang = [i for i, (t, _) in enumerate(items) if t == ANGLE]
    dih = [i for i, (t, _) in enumerate(items) if t == DIH]
    out = {}
    if ang:
        out["angle"] = ang[0]
    if dih:
        out["tc"] = dih[0]
    if len(dih) > 1:
        out["arm"] = dih[1]
    return out


ROLE_OF = {"straight": "angle", "folded": "angle", "trans": "tc", "cis": "tc", "arm": "arm"}


def end_atom(items, role):
    t, idx = items[roles(items)[role]]
    return idx[2] if role == "angle" else (idx[3] if role == "tc" else idx[0])


def check_ownership(items, align):
    """Every end atom belongs to its item alone and to no alignment set."""
    for role in roles(items):
        e = end_atom(items, role)
        users = [i for i, (_, idx) in enumerate(items) if e in idx]
        assert users == [roles(items)[role]] and e not in set(align), (role, e, users)


def _unit(v):
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def _angle(a, b, c):
    """The angle at b, [n]."""
    u, v = a - b, c - b
    return np.arctan2(np.linalg.norm(np.cross(u, v), axis=-1), (u * v).sum(-1))


def dihedral(a, b, c, d):
    """The dihedral a-b-c-d in the reference's convention (ann.py:339-349), [n]."""
    r12, r23, r34 = b - a, c - b, d - c
    n1, n2 = np.cross(r12, r23), np.cross(r23, r34)
    return np.arctan2((n1 * r34).sum(-1) * np.linalg.norm(r23, axis=-1), (n1 * n2).sum(-1))


def place(a, b, c, r, theta, phi):
    """The point d with |d - c| = r, the angle b-c-d = theta and the dihedral a-b-c-d = phi (all [n] / [n, 3])."""
    bc = _unit(c - b)
    nrm = _unit(np.cross(b - a, bc))
    m = np.cross(nrm, bc)
    r, theta, phi = (np.asarray(v, np.float64)[:, None] for v in (r, theta, phi))
    return c + r * (-np.cos(theta) * bc + np.sin(theta) * np.cos(phi) * m + np.sin(theta) * np.sin(phi) * nrm)


def sines(frames, items):
    x = np.asarray(frames, np.float64)
    out = np.ones((len(x), len(items)))
    for i, (t, idx) in enumerate(items):
        if t == ANGLE:
            out[:, i] = np.sin(_angle(x[:, idx[0]], x[:, idx[1]], x[:, idx[2]]))
        elif t == DIH:
            out[:, i] = np.minimum(np.sin(_angle(x[:, idx[0]], x[:, idx[1]], x[:, idx[2]])),
                                   np.sin(_angle(x[:, idx[1]], x[:, idx[2]], x[:, idx[3]])))
    return out


def draw(regime, delta, xyz, items, n, seed, align=()):
    """(frames float32 [n, n_atoms, 3], sines float64 [n, n_items]) of one regime at `delta` degrees from its pole.  With an
    alignment set: every frame's fit is well conditioned (far_frames.conditioning >= 0.05), asserted, no frame left out."""
    check_ownership(items, align)
    x = ff.draw("near", xyz, list(align), n, seed).astype(np.float64)
    rng = np.random.default_rng([seed, REGIMES.index(regime), int(round(delta * 1e6))])
    d = np.radians(delta)
    role = ROLE_OF[regime]
    t, idx = items[roles(items)[role]]
    P = [x[:, a] for a in idx]
    if role == "angle":                                    # the third atom about the second, measured from the first
        theta = np.full(n, np.pi - d if regime == "straight" else d)
        r = np.linalg.norm(P[2] - P[1], axis=-1)
        new = place(P[1] + rng.standard_normal((n, 3)), P[0], P[1], r, theta, rng.uniform(-np.pi, np.pi, n))
    elif role == "tc":                                     # the fourth atom: arm angle 2-3-4 kept, the dihedral prescribed
        sign = np.where(np.arange(n) % 2 == 0, 1.0, -1.0)
        phi = sign * (np.pi - d if regime == "trans" else d)
        new = place(P[0], P[1], P[2], np.linalg.norm(P[3] - P[2], axis=-1), _angle(P[1], P[2], P[3]), phi)
    else:                                                  # the first atom: the angle 1-2-3 prescribed, the dihedral kept
        phi = dihedral(P[0], P[1], P[2], P[3])
        new = place(P[3], P[2], P[1], np.linalg.norm(P[0] - P[1], axis=-1), np.full(n, np.pi - d), phi)
    x[:, end_atom(items, role)] = new
    x = np.einsum("nai,nij->naj", x, ff.rotations(rng, n)) + 3.0 * rng.standard_normal((n, 1, 3))
    x = np.ascontiguousarray(x, dtype=np.float32)
    if len(align):
        c = ff.conditioning(x, xyz, list(align))
        assert float(c.min()) >= 0.05, (regime, delta, float(c.min()))
    return x, sines(x, items)


def near(xyz, n, seed, align=()):
    """The near frames `draw` starts from (before its own rigid motion): the control, and the near rows of `interleaved`."""
    return ff.draw("near", xyz, list(align), n, seed)


def interleaved(regime, deltas, xyz, items, n, seed, align=()):
    """(frames, labels, sines): every even frame a near frame (label None, the rows of `near`), the odd ones cycling through
    `deltas` (label: the delta), so that every pair of frames - and with it every tile, ring entry and round of a kernel - holds an
    edge frame next to a near one."""
    base = near(xyz, n, seed, align)
    out = np.array(base)
    labels = [None] * n
    deltas = list(deltas)
    drawn = {dl: draw(regime, dl, xyz, items, n, seed, align)[0] for dl in set(deltas)}
    for i in range(1, n, 2):
        dl = deltas[(i // 2) % len(deltas)]
        out[i] = drawn[dl][i]
        labels[i] = dl
    return out, labels, sines(out, items)
