"""Frames far from the reference state, for the tests of the rotation solver every aligning kernel calls (kabsch_rotation_t,
molann_amd/csrc/molann_math.h).

The solver runs Newton on the characteristic quartic of Horn's 4x4 matrix from lam0 = min(e0 / |H|_F, sqrt 3), first NFIX
unconditional steps, then a guarded loop that a wave enters only when one of its frames has not converged.  e0 is tight, and
the fixed steps enough, only for a frame that resembles the reference, which is what the suite's usual frames do (reference +
0.2 A of noise + a rigid motion).  The regimes here are drawn to reach the guarded loop and the solver's other branches:

  near        the usual frames: reference + 0.2 A of noise, a random rotation and a shift of a few A (the control)
  hinge       the atoms past a random pivot turned by 60-180 degrees about an axis through it, + 0.3 A of noise, moved
              rigidly; one frame in four an independent random-walk chain of the same length instead.  Several A RMSD
  mirror      the reference + noise with z -> -z, moved rigidly: det H < 0, the d = -1 branch
  flip180     the reference + noise turned by exactly 180 degrees about a coordinate or a random axis: the optimal quaternion's
              real part is (close to) 0
  offset      hinge frames (three in four) and near frames translated by 100 or 1000 A: absolute box coordinates in fp32
  exact       the reference itself, moved rigidly, no noise
  degenerate  a near frame whose align atoms are nearly collinear, or all at one point: no defined rotation

All frames are float32 arrays [n, n_atoms, 3] built with numpy from a seed.  `conditioning` gives each frame's
(s2 + d*s3) / s1 of the float64 covariance (the rotation is defined where it is > 0); `leaves_fixed_steps` replays the
solver's unconditional Newton steps in numpy and says which frames go on to the guarded loop."""

import numpy as np
import torch

from molann_amd import workloads as wl

REGIMES = ("near", "hinge", "mirror", "flip180", "offset", "exact", "degenerate")
FAR = ("hinge", "mirror", "offset")               # regimes whose frames mostly leave the fixed steps

# The constants of kabsch_rotation_t (molann_math.h) and of its callers: NFIX unconditional Newton steps (5 in fp64, 4 in
# fp32), the step test |step| <= tol * |lam| (1e-14 / 1e-6), the bound |lam| < 4, and the callers' Newton start
# e0 = (sum |p|^2 + sum |ref|^2) / 2 * 1.0001 over the centred align atoms.
NFIX = {64: 5, 32: 4}
TOL = {64: 1e-14, 32: 1e-6}
E0_SLACK = 1.0001


def _unit(rng, n):
    v = rng.standard_normal((n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def rotations(rng, n):
    """n uniformly random proper rotations [n, 3, 3] (row-vector convention: y = x @ R)."""
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return wl.quaternion_to_matrix(torch.from_numpy(q)).numpy()


def axis_angle(axis, angle):
    """Rotation matrices [n, 3, 3] (y = x @ R) by `angle` radians about unit `axis` [n, 3]."""
    x, y, z = axis[:, 0], axis[:, 1], axis[:, 2]
    c, s = np.cos(angle), np.sin(angle)
    C = 1.0 - c
    M = np.stack([c + x * x * C, x * y * C - z * s, x * z * C + y * s,
                  y * x * C + z * s, c + y * y * C, y * z * C - x * s,
                  z * x * C - y * s, z * y * C + x * s, c + z * z * C], axis=1).reshape(-1, 3, 3)
    return np.transpose(M, (0, 2, 1))


def _rigid(rng, x, shift=3.0):
    return np.einsum("nai,nij->naj", x, rotations(rng, len(x))) + shift * rng.standard_normal((len(x), 1, 3))


def draw(regime, xyz, align, n, seed):
    """n float32 frames of one regime for the reference coordinates xyz [n_atoms, 3] and the 0-based align set."""
    rng = np.random.default_rng([seed, REGIMES.index(regime)])
    ref = np.asarray(xyz, np.float64)
    na = len(ref)
    base = np.broadcast_to(ref, (n, na, 3))
    if regime == "near":
        x = _rigid(rng, base + 0.2 * rng.standard_normal((n, na, 3)))
    elif regime == "hinge":
        x = np.array(base)
        lo, hi = na // 4, max(na // 4 + 1, (3 * na) // 4)
        piv = rng.integers(lo, hi, size=n)
        R = axis_angle(_unit(rng, n), np.radians(rng.uniform(60.0, 180.0, size=n)))
        for i in range(n):
            k = piv[i]
            x[i, k + 1:] = (x[i, k + 1:] - x[i, k]) @ R[i] + x[i, k]
        x = x + 0.3 * rng.standard_normal((n, na, 3))
        for i in range(0, n, 4):                   # an independent conformation
            x[i] = wl.synthetic_chain(n_atoms=na, step=1.5, seed=int(rng.integers(1 << 30)))
        x = _rigid(rng, x)
    elif regime == "mirror":
        x = base + 0.2 * rng.standard_normal((n, na, 3))
        x[:, :, 2] *= -1.0
        x = _rigid(rng, x)
    elif regime == "flip180":
        ax = np.concatenate([np.eye(3), _unit(rng, 1)])[np.arange(n) % 4]
        ax[3::4] = _unit(rng, len(ax[3::4]))
        R = 2.0 * ax[:, :, None] * ax[:, None, :] - np.eye(3)
        x = np.einsum("nai,nij->naj", base + 0.2 * rng.standard_normal((n, na, 3)), R) + 3.0 * rng.standard_normal((n, 1, 3))
    elif regime == "offset":
        x = draw("hinge", xyz, align, n, seed + 1).astype(np.float64)
        x[3::4] = draw("near", xyz, align, n, seed + 2)[3::4]
        mag = np.where(np.arange(n) % 2 == 0, 100.0, 1000.0)
        x = x + (mag[:, None] * _unit(rng, n))[:, None, :]
    elif regime == "exact":
        x = _rigid(rng, np.array(base))
    elif regime == "degenerate":
        x = draw("near", xyz, align, n, seed + 3).astype(np.float64)
        al = list(align)
        for i in range(n):
            c = x[i, al].mean(0)
            if i % 2 == 0:                         # nearly collinear: on a line, 1e-3 A off it
                t = np.linspace(-4.0, 4.0, len(al))
                x[i, al] = c + t[:, None] * _unit(rng, 1) + 1e-3 * rng.standard_normal((len(al), 3))
            else:                                  # all at one point
                x[i, al] = c
    else:
        raise KeyError(regime)
    return np.ascontiguousarray(x, dtype=np.float32)


def compose(labels, xyz, align, seed, base=None):
    """Frames [len(labels), n_atoms, 3] with frame i drawn from regime labels[i]; the near frames are base's rows when given
    (so that a batch and its near control share those frames bit for bit)."""
    labels = list(labels)
    out = np.empty((len(labels),) + np.shape(xyz), np.float32)
    for j, r in enumerate(REGIMES):
        pos = [i for i, l in enumerate(labels) if l == r]
        if not pos:
            continue
        if r == "near" and base is not None:
            out[pos] = np.asarray(base)[pos]
        else:
            out[pos] = draw(r, xyz, align, len(pos), seed * 16 + j)
    return out


def interleaved(n, far=("hinge", "mirror", "offset"), other=("flip180", "exact", "near")):
    """Labels of a mixed batch: every odd frame far, every fourth a near frame, the rest flip180 / exact / near.  Every pair,
    and so every 64-frame tile, ring entry of B = 8 / 4 / 2 frames and round of 16 / 8 / 4 frames, holds frames that
    converge in the fixed steps next to frames that do not."""
    lab = []
    for i in range(n):
        if i % 2 == 1:
            lab.append(far[(i // 2) % len(far)])
        elif i % 4 == 0:
            lab.append("near")
        else:
            lab.append(other[(i // 4) % len(other)])
    return lab


def single(n, regime="hinge", at=(0, 63, 64, -1)):
    """Labels of a near batch with one far frame at each position of `at` (negative: from the end) that lies in the batch."""
    lab = ["near"] * n
    for p in at:
        q = p if p >= 0 else n + p
        if 0 <= q < n:
            lab[q] = regime
    return lab


def covariances(frames, xyz, align):
    """(H [n, 3, 3], e0 [n]) as the kernels form them, in float64: H = P^T ref over the centred align atoms (frame P, the
    reference centred), e0 the Newton start of the callers."""
    al = list(align)
    P = np.asarray(frames, np.float64)[:, al]
    P = P - P.mean(1, keepdims=True)
    ref = np.asarray(xyz, np.float32)[al].astype(np.float64)
    ref = ref - ref.mean(0)
    H = np.einsum("nai,aj->nij", P, ref)
    e0 = 0.5 * ((P * P).sum((1, 2)) + (ref * ref).sum()) * E0_SLACK
    return H, e0


def conditioning(frames, xyz, align):
    """Per frame (s2 + d*s3) / s1 of the float64 covariance (s its singular values, d = sign det H): 0 where the optimal proper
    rotation is not unique, small where it is ill-conditioned (its derivative divides by this gap)."""
    H, _ = covariances(frames, xyz, align)
    s = np.linalg.svd(H, compute_uv=False)
    d = np.sign(np.linalg.det(H))
    with np.errstate(divide="ignore", invalid="ignore"):
        c = (s[:, 1] + d * s[:, 2]) / s[:, 0]
    return np.where(s[:, 0] > 0, c, 0.0)


def leaves_fixed_steps(frames, xyz, align, bits=64):
    """Per frame: True when kabsch_rotation_t<T> (T = double for bits=64, float for 32) has not converged after its NFIX
    unconditional Newton steps and goes on to the guarded loop.  A numpy replay of molann_math.h's arithmetic: the scale by an
    fp32 reciprocal square root, the quartic's coefficients, the start lam0 and the steps with an fp32 reciprocal of p'."""
    H, e0 = covariances(frames, xyz, align)
    T = np.float64 if bits == 64 else np.float32
    H, e0 = H.astype(T), e0.astype(T)
    with np.errstate(all="ignore"):
        fro2 = (H * H).sum((1, 2))
        live = (fro2 > 1e-30) & (fro2 < 1e30)   # the others return the identity at once
        s = (np.float32(1.0) / np.sqrt(fro2.astype(np.float32))).astype(T)
        h = H * s[:, None, None]
        hxx, hxy, hxz = h[:, 0, 0], h[:, 0, 1], h[:, 0, 2]
        hyx, hyy, hyz = h[:, 1, 0], h[:, 1, 1], h[:, 1, 2]
        hzx, hzy, hzz = h[:, 2, 0], h[:, 2, 1], h[:, 2, 2]
        k00, k01, k02, k03 = hxx + hyy + hzz, hyz - hzy, hzx - hxz, hxy - hyx
        k11, k12, k13 = hxx - hyy - hzz, hxy + hyx, hzx + hxz
        k22, k23 = -hxx + hyy - hzz, hyz + hzy
        k33 = -hxx - hyy + hzz
        c2 = T(-2) * (h * h).sum((1, 2))
        det_h = hxx * (hyy * hzz - hyz * hzy) - hxy * (hyx * hzz - hyz * hzx) + hxz * (hyx * hzy - hyy * hzx)
        c1 = T(-8) * det_h
        s0, s1, s2 = k00 * k11 - k01 * k01, k00 * k12 - k01 * k02, k00 * k13 - k01 * k03
        s3, s4, s5 = k01 * k12 - k11 * k02, k01 * k13 - k11 * k03, k02 * k13 - k12 * k03
        d5, d4, d3 = k22 * k33 - k23 * k23, k12 * k33 - k13 * k23, k12 * k23 - k13 * k22
        d2, d1, d0 = k02 * k33 - k03 * k23, k02 * k23 - k03 * k22, k02 * k13 - k03 * k12
        c0 = s0 * d5 - s1 * d4 + s2 * d3 + s3 * d2 - s4 * d1 + s5 * d0
        sqrt3 = T(1.7320508075688772)
        lam = np.minimum(e0 * s, sqrt3)
        lam = np.where(lam > 0, lam, sqrt3)
        step = np.zeros_like(lam)
        for _ in range(NFIX[bits]):
            l2 = lam * lam
            p = (l2 + c2) * l2 + (c1 * lam + c0)
            dp = (T(4) * l2 + T(2) * c2) * lam + c1
            step = p * (np.float32(1.0) / dp.astype(np.float32)).astype(T)
            lam = lam - step
        done = (step == step) & (np.abs(lam) < 4) & ~(np.abs(step) > T(TOL[bits]) * np.abs(lam))
    return live & ~done
