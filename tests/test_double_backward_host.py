"""The step of the central differences behind create_graph=True (molann_amd/ann.py: _difference_points, the same step as
csrc/molann_torch.cpp: FeatBackward64Fn), checked without a GPU: the float64 oracle's autograd stands in for the float64 kernels
the GPU takes the differences of, and the differences are compared with the exact double backward.  Frames at their own
coordinates and shifted by 100 and 1000 A: the curvature of bonds, angles, dihedrals and the alignment is set by the
geometry, not by where the frame sits in the box, so the error must not grow with the shift."""

import pytest
import torch

from molann_amd import workloads as wl
from molann_amd.ann import _difference_points
from oracle import molann_oracle as mo

N_FRAMES = 4


def _features(w):
    feats = [(t, [a - 1 for a in atoms]) for t, atoms in w.features]
    al = [a - 1 for a in w.align] if w.align is not None else None
    ref_x = mo.center_reference(torch.from_numpy(w.ref_xyz[al])).double() if al else None
    return lambda x: mo.preprocessing_forward(x, feats, w.use_angle_value, al, ref_x)


@pytest.mark.parametrize("offset", [0.0, 100.0, 1000.0])
@pytest.mark.parametrize("name", ["C3", "P1", "C4"])
def test_central_differences_match_the_exact_double_backward(name, offset):
    """For a cotangent g on the features and v on gx = J(x)^T g: d/dx [v . J(x)^T g] and J(x) v, the two directional
    derivatives _FeatBackward64.backward takes, as central differences at the points _difference_points gives, within 1e-7
    of the exact ones (relative to their largest entry)."""
    w = wl.get_workload(name)
    f = _features(w)
    gen = torch.Generator().manual_seed(17)
    x = w.make_frames(N_FRAMES, seed=5).double() + offset
    g = torch.randn((N_FRAMES, w.feature_dim()), generator=gen, dtype=torch.float64)
    v = torch.randn(x.shape, generator=gen, dtype=torch.float64)
    v[1] *= 1e-3                      # the step is per frame: a frame with a small cotangent takes a long step

    def gx(xx, create_graph=False):
        xx = xx.detach().requires_grad_(True)
        return torch.autograd.grad(f(xx), xx, g, create_graph=create_graph)[0], xx

    first, xx = gx(x, create_graph=True)
    (exact_x,) = torch.autograd.grad((first * v).sum(), xx)
    _, exact_g = torch.autograd.functional.jvp(f, x, v)

    xp, xm, inv = _difference_points(x, v)
    assert inv.shape == (N_FRAMES, 1, 1) and bool((inv > 0).all())
    diff_x = (gx(xp)[0] - gx(xm)[0]) * inv
    with torch.no_grad():
        diff_g = (f(xp) - f(xm)) * inv.view(-1, 1)
    for got, want, what in ((diff_x, exact_x, "d/dx"), (diff_g, exact_g, "J v")):
        for i in range(N_FRAMES):        # each frame against its own scale: frame 1's is 1e-3 of the others'
            scale = float(want[i].abs().max())
            err = float((got[i] - want[i]).abs().max())
            assert err <= 1e-7 * scale, (name, offset, what, i, err / scale)


def test_a_zero_cotangent_gives_zero_step_and_tiny_ones_stay_finite():
    """h = 0 on a frame whose v is zero (its rows stay exactly zero); a cotangent near the bottom of the double range takes a
    finite step and a finite 1 / 2h (the 1e-300 clamps)."""
    x = wl.get_workload("C3").make_frames(3, seed=2).double() + 100.0
    v = torch.randn(x.shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    v[0] = 0.0
    v[2] *= 1e-305
    xp, xm, inv = _difference_points(x, v)
    assert float(inv[0]) == 0.0 and torch.equal(xp[0], x[0]) and torch.equal(xm[0], x[0])
    assert bool(torch.isfinite(xp).all() and torch.isfinite(xm).all() and torch.isfinite(inv).all())
    assert 0.0 < float(inv[2]) < 1e-290
    step = (xp - xm).abs().amax(dim=(1, 2))
    assert float(step[1]) == pytest.approx(1.2e-5, rel=1e-6)
    assert 0.0 < float(step[2]) <= 1.2e-5            # |v|_max below the clamp: a shorter move, never an infinite one
