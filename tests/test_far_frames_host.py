"""The rotation solver (kabsch_rotation_t, molann_amd/csrc/molann_math.h) compiled for the host, on frames far from the
reference (tests/far_frames.py): hinge motions and independent conformations, mirror images, exact 180-degree turns, frames
100-1000 A from the origin, noise-free copies and degenerate align sets.  The fp64 and fp32 instantiations against numpy's SVD
(the reference's U diag(1, 1, d) Vh), the closed-form backward against float64 autograd through the SVD, and a guard that the
far regimes do take the solver's guarded Newton loop (what tests/test_gpu_far_frames.py relies on to reach it on the device)."""

import ctypes
import os
import re

import numpy as np
import pytest
import torch

import far_frames as ff
from molann_amd import _capi
from molann_amd import workloads as wl


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def _geometry(name):
    """(reference xyz, 0-based align set): align sets of 3 to 300 atoms."""
    if name == "ala3":
        return wl.ALA_DIPEPTIDE_XYZ, [4, 6, 8]
    if name == "ala22":
        return wl.ALA_DIPEPTIDE_XYZ, list(range(22))
    if name == "chain42":                                  # every fourth atom of the 166-atom chain (P1, P2)
        return wl.synthetic_chain(n_atoms=166, step=1.4, seed=11), list(range(2, 166, 4))
    if name == "chain300":
        rng = np.random.default_rng(3)
        return wl.synthetic_chain(n_atoms=1200, step=1.5, seed=3), sorted(rng.choice(1200, size=300, replace=False).tolist())
    if name == "ala_bb":                                   # the 7 backbone atoms: a nearly planar, poorly conditioned set
        return wl.ALA_DIPEPTIDE_XYZ, [a - 1 for a in wl.ALA_BACKBONE]
    raise KeyError(name)


GEOMETRIES = ("ala3", "ala_bb", "ala22", "chain42", "chain300")


def _svd_rotation(H):
    """The reference's rotation (ann.py:188-195) in float64: U diag(1, 1, sign det(U Vh)) Vh, [n, 3, 3]."""
    u, _, vh = np.linalg.svd(H)
    d = np.sign(np.linalg.det(u @ vh))
    D = np.tile(np.eye(3), (len(H), 1, 1))
    D[:, 2, 2] = d
    return u @ D @ vh


def _hook(H, e0, bits):
    L = _capi.lib()
    R = np.zeros((len(H), 9), np.float32)
    for i in range(len(H)):
        r = np.zeros(9, np.float32)
        if bits == 64:
            h = np.ascontiguousarray(H[i].reshape(9), np.float64)
            assert L.molann_selftest_kabsch_rotation(_ptr(h), float(e0[i]), _ptr(r)) == 0
        else:
            h = np.ascontiguousarray(H[i].reshape(9), np.float32)
            assert L.molann_selftest_kabsch_rotation_f32(_ptr(h), np.float32(e0[i]), _ptr(r)) == 0
        R[i] = r
    return R.reshape(-1, 3, 3).astype(np.float64)


@pytest.mark.parametrize("name", ["ala22", "chain42", "chain300"])
def test_far_regimes_reach_the_guarded_loop(name):
    """The reach guard: most hinge, mirror and offset frames leave the fixed Newton steps in both precisions, no near frame
    does, and every 8 consecutive frames of the interleaved layout hold frames of both kinds."""
    xyz, al = _geometry(name)
    n = 400
    for bits in (64, 32):
        for r in ff.FAR:
            frac = float(ff.leaves_fixed_steps(ff.draw(r, xyz, al, n, 1), xyz, al, bits).mean())
            assert frac >= 0.6, (name, bits, r, frac)
        near = ff.leaves_fixed_steps(ff.draw("near", xyz, al, n, 1), xyz, al, bits)
        assert not near.any(), (name, bits, int(near.sum()))
        lab = ff.interleaved(256)
        leaves = ff.leaves_fixed_steps(ff.compose(lab, xyz, al, seed=2), xyz, al, bits).reshape(-1, 8)
        assert leaves.any(1).all() and (~leaves).any(1).all(), (name, bits)


def test_fixed_step_replica_uses_the_solver_constants():
    """far_frames.leaves_fixed_steps replays kabsch_rotation_t with NFIX, the step tolerance and the callers' e0 slack copied
    from the sources: they must still be the sources' values."""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "molann_amd", "csrc")
    src = open(os.path.join(csrc, "molann_math.h")).read()
    m = re.search(r"constexpr int NFIX = F32 \? (\d+) : (\d+);", src)
    assert m and (int(m.group(1)), int(m.group(2))) == (ff.NFIX[32], ff.NFIX[64]), m and m.group(0)
    m = re.search(r"const T tol = F32 \? \(T\)([0-9.e+-]+)f : \(T\)([0-9.e+-]+);", src)
    assert m and (float(m.group(1)), float(m.group(2))) == (ff.TOL[32], ff.TOL[64]), m and m.group(0)
    slack = set()
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".inc", ".h")):
            slack |= set(re.findall(r"kabsch_rotation[_a-z0-9<>, ]*\(h, 0\.5 \*[^;]*\* ([0-9.]+), R\)", open(os.path.join(csrc, f)).read()))
    assert slack == {repr(ff.E0_SLACK)}, slack


@pytest.mark.parametrize("name", GEOMETRIES)
def test_rotation_hooks_against_svd(name):
    """Every regime through the host build of kabsch_rotation (fp64) and kabsch_rotation_f32: on frames whose rotation is
    defined ((s2 + d s3) / s1 >= 0.05) the aligned align atoms equal the SVD's to fp32 accuracy; on every frame, degenerate ones
    included, the result is a finite proper rotation."""
    xyz, al = _geometry(name)
    for r in ff.REGIMES:
        x = ff.draw(r, xyz, al, 150, 7)
        H, e0 = ff.covariances(x, xyz, al)
        cond = ff.conditioning(x, xyz, al)
        P = x[:, al].astype(np.float64)
        P = P - P.mean(1, keepdims=True)
        want = np.einsum("nai,nij->naj", P, _svd_rotation(H))
        scale = np.abs(P).max((1, 2))
        ok = cond >= 0.05
        for bits, tol in ((64, 1e-6), (32, 2e-5)):
            R = _hook(H, e0, bits)
            assert np.isfinite(R).all(), (name, r, bits)
            orth = np.abs(np.einsum("nij,nkj->nik", R, R) - np.eye(3)).max((1, 2))
            assert orth.max() < 1e-5, (name, r, bits, float(orth.max()))
            assert np.abs(np.linalg.det(R) - 1.0).max() < 1e-5, (name, r, bits)
            if ok.any():
                got = np.einsum("nai,nij->naj", P, R)
                err = (np.abs(got - want).max((1, 2)) / scale)[ok]
                assert err.max() <= tol, (name, r, bits, float(err.max()), int(np.argmax(err)))
        if r in ("near", "exact", "flip180", "mirror") and name in ("ala22", "chain42", "chain300"):
            assert ok.all(), (name, r, float(cond.min()))


@pytest.mark.parametrize("name", ["ala22", "chain42", "chain300"])
def test_rotation_backward_against_autograd_on_far_frames(name):
    """kabsch_rotation_backward (the closed form every backward kernel calls) against float64 autograd through the SVD rotation,
    on well-conditioned hinge, mirror, flip180 and offset frames."""
    xyz, al = _geometry(name)
    L = _capi.lib()
    g = np.random.default_rng(9)
    checked = 0
    for r in ("hinge", "mirror", "flip180", "offset"):
        x = ff.draw(r, xyz, al, 60, 11)
        H, _ = ff.covariances(x, xyz, al)
        cond = ff.conditioning(x, xyz, al)
        for i in np.nonzero(cond >= 0.1)[0]:
            Ht = torch.from_numpy(H[i]).requires_grad_(True)
            u, _, vh = torch.linalg.svd(Ht)
            d = torch.sign(torch.linalg.det(u @ vh)).detach()
            R = u @ torch.diag(torch.stack([torch.ones((), dtype=torch.float64), torch.ones((), dtype=torch.float64), d])) @ vh
            GR = torch.from_numpy(g.standard_normal((3, 3)))
            (R * GR).sum().backward()
            want = Ht.grad.numpy().reshape(9)
            Hn = np.ascontiguousarray(H[i].reshape(9))
            Rn = np.ascontiguousarray(R.detach().numpy().reshape(9).astype(np.float32))
            GRn = np.ascontiguousarray(GR.numpy().reshape(9).astype(np.float32))
            GH = np.zeros(9, np.float32)
            assert L.molann_selftest_kabsch_backward(_ptr(Hn), _ptr(Rn), _ptr(GRn), _ptr(GH)) == 0
            s = np.abs(want).max()
            assert np.abs(GH - want).max() <= 1e-4 * s / min(1.0, 10 * cond[i]), (name, r, i, float(cond[i]), GH, want)
            checked += 1
    assert checked >= 100, checked
