"""Net force and torque of the oracle's own gradients (tests/conservation.py), on the CPU: what tests/test_gpu_conservation.py
holds every gradient kernel to.

- The oracle's float32 and float64 autograd on 64 frames of each of the six non-degenerate regimes of tests/far_frames.py, for the
  plans ala_head, ala_inv, ala_align, B8, A166 and ala_head with an uncentred ref_x: the residuals stay at rounding level (printed as
  a table), and the gradient of one seed passes `bound` built from another, independent seed.
- Three planted faults on the float32 gradient of ala_head, each of the shape of a term left out or slightly wrong: each passes
  the oracle tolerance the suite holds gradients to (1e-4 of the scale) and fails the conservation check.
- A plan that is not invariant (position items, no alignment) fails it with a residual above 0.1.
- The frame selection keeps at least 75 % of every regime on every (case, batch) the GPU file uses."""

import numpy as np
import pytest
import torch

import conservation as cv
import far_frames as ff
import test_gpu_alignment_gradients as ag
import test_gpu_conservation as gc
import test_gpu_far_frames as fam
from oracle import molann_oracle as mo

REGIMES = tuple(r for r in ff.REGIMES if r != "degenerate")
PLANS = ("ala_head", "ala_inv", "ala_align", "B8", "A166", "ala_head_shift")
N, SEED, OTHER = 64, 3, 11
DT = {32: torch.float32, 64: torch.float64}
_CACHE = {}


def _plan(name):
    """(spec, CPU model, ref_x in float64)"""
    if name not in _CACHE:
        if name == "ala_head_shift":
            spec = fam._spec("ala_head")
            model = spec.build("cpu", torch.float32)
            ref = fam._align_layer(model).ref_x.detach().double() + torch.tensor(ag.SHIFT, dtype=torch.float64)
            assert float(ref.mean(0).abs().max()) > 1.0
        else:
            spec = fam._spec(name)
            model = spec.build("cpu", torch.float32)
            ref = fam._align_layer(model).ref_x.detach().double()
        _CACHE[name] = (spec, model, ref)
    return _CACHE[name]


def _out_shape(spec, x):
    if spec.align_only:
        return tuple(x.shape)
    return (len(x), spec.mlp[-1] if spec.mlp else sum(mo.feature_dim(t, len(i), False) for t, i in spec.feats))


def _forces(name, regime, seed, bits):
    """(frames, kept mask, the oracle's dL/dx in float32 or float64 for a random cotangent, that in float64)"""
    key = (name, regime, seed, bits)
    if key not in _CACHE:
        spec, model, ref = _plan(name)
        x = ff.draw(regime, spec.xyz, spec.align, N, seed)
        keep, _ = cv.select(x, [regime] * N, spec.xyz, spec.align, spec.feats, key)
        xs = torch.from_numpy(x)
        G = cv.cotangent(_out_shape(spec, xs), seed, torch.float64)
        _CACHE[key] = (x, keep, fam._oracle(spec, model, xs, G, ref, dtype=DT[bits])[1].detach())
    return _CACHE[key]


@pytest.mark.parametrize("bits", [32, 64])
@pytest.mark.parametrize("name", PLANS)
def test_oracle_gradients_conserve(name, bits):
    """The residual tables, and: one seed's gradient passes the bound another seed's sets"""
    u = cv.U[bits]
    for regime in REGIMES:
        x, keep, F = _forces(name, regime, SEED, bits)
        x2, keep2, F2 = _forces(name, regime, OTHER, bits)
        r_F, r_T = cv.residuals(x[keep], F[keep])
        q_F, q_T = cv.residuals(x2[keep2], F2[keep2])
        lab, lab2 = [regime] * int(keep.sum()), [regime] * int(keep2.sum())
        print("conservation host %-9s f%d %-8s kept %2d/%d  r_F %.2e (%.1f u)  r_T %.2e (%.1f u)"
              % (name, bits, regime, keep.sum(), N, r_F.max(), r_F.max() / u, r_T.max(), r_T.max() / u))
        assert not np.isnan(r_F).any() and not np.isnan(q_F).any()
        assert not cv.exceeding(r_F, lab, cv.bound(q_F, lab2, u)), (name, regime, "r_F", r_F.max(), q_F.max())
        assert not cv.exceeding(r_T, lab, cv.bound(q_T, lab2, u)), (name, regime, "r_T", r_T.max(), q_T.max())
        # rounding level: the net force within 16 u of sum |F|, and the torque within 16 u (1 + |c| / Rg): the oracle forms x - x_c in
        # its own precision, known to u |x|, against levers of the molecule's radius of gyration Rg (a few A; |c| is 100 to 1000 A in
        # the offset regime).  An uncentred ref_x adds the oracle's own rounding of sum(x - x_c) * mean(ref): the bound of the other
        # seed, above, is its only check.
        if name.endswith("_shift"):
            continue
        xs = x[keep].astype(np.float64)
        c = xs.mean(1, keepdims=True)
        lever = 1.0 + float((np.linalg.norm(c, axis=-1)[:, 0] / np.sqrt(((xs - c) ** 2).sum(-1).mean(1))).max())
        assert r_F.max() <= 16 * u, (name, regime, r_F.max() / u)
        assert r_T.max() <= 16 * u * lever, (name, regime, r_T.max() / u, lever)


def _twist(x, F, eps, scale):
    r = x - x.mean(1, keepdims=True)
    w = np.array([0.6, 0.0, 0.8])
    return F + eps * scale * np.cross(w, r) / np.abs(r).max()


FAULTS = {
    # a constant on every row: a centroid share that is slightly off
    "constant": lambda x, F, s: F + 1e-5 * s,
    # one atom's row scaled by 1 + 2e-5: one atom of an item's backward
    "one_atom": lambda x, F, s: np.concatenate([F[:, :4], F[:, 4:5] * (1 + 2e-5), F[:, 5:]], 1),
    # a force field w x (x_a - c) of 1e-5 of the scale: a term of the rotation's backward slightly off
    "twist": lambda x, F, s: _twist(x, F, 1e-5, s),
}


@pytest.mark.parametrize("fault", sorted(FAULTS))
def test_planted_faults_pass_the_oracle_tolerance_and_fail_conservation(fault):
    caught = []
    for regime in REGIMES:
        x, keep, F32 = _forces("ala_head", regime, SEED, 32)
        _, _, F64 = _forces("ala_head", regime, SEED, 64)
        x, F32, F64 = x[keep].astype(np.float64), F32[keep].double().numpy(), F64[keep].numpy()
        scale = np.abs(F64).max()
        bad = FAULTS[fault](x, F32, scale)
        err0, err = np.abs(F32 - F64).max() / scale, np.abs(bad - F64).max() / scale
        assert err <= 0.5e-4 and np.abs(bad - F32).max() >= 5e-6 * scale, (fault, regime, err0, err)    # changed, and well under the suite's 1e-4
        lab = [regime] * len(x)
        ref = cv.residuals(x, F32)
        got = cv.residuals(x, bad)
        over = [bool(cv.exceeding(got[k], lab, cv.bound(ref[k], lab, cv.U[32]))) for k in (0, 1)]
        print("conservation host fault %-8s %-8s err/scale %.1e (clean %.1e)  r_F %.1e (clean %.1e)  r_T %.1e (clean %.1e)  caught %s"
              % (fault, regime, err, err0, np.nanmax(got[0]), ref[0].max(), np.nanmax(got[1]), ref[1].max(), over))
        if any(over):
            caught.append(regime)
        if fault in ("constant", "one_atom"):              # a net force: r_F sees it in every regime, 100-1000 A out as well
            assert over[0], (fault, regime, "not caught by r_F")
    # (100-1000 A out the reference's own torque residual is up to 1.4e-5: a pure torque of this size could hide there, and only there)
    assert set(REGIMES) - set(caught) <= {"offset"}, (fault, caught)


def test_a_plan_that_is_not_invariant_fails():
    """Position items with no alignment: the gradient is the cotangent itself"""
    spec = fam._spec("ala_head")
    x = ff.draw("near", spec.xyz, spec.align, N, SEED)
    xx = torch.from_numpy(x).double().requires_grad_(True)
    y = mo.preprocessing_forward(xx, spec.feats, False, None, None)
    (y * cv.cotangent(tuple(y.shape), SEED, torch.float64)).sum().backward()
    r_F, r_T = cv.residuals(x, xx.grad)
    print("conservation host control: r_F %.2f to %.2f, r_T %.2f to %.2f" % (r_F.min(), r_F.max(), r_T.min(), r_T.max()))
    assert r_F.max() > 0.1 and r_T.max() > 0.1
    lab = ["near"] * N
    assert len(cv.exceeding(r_F, lab, {"near": 0.1})) > N // 2


def test_residuals_masks_and_shapes():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((5, 6, 3)) + 50.0
    F = np.zeros((5, 6, 3))
    F[:, 1], F[:, 4] = [1.0, 2.0, 3.0], [-1.0, -2.0, -3.0]                # equal and opposite, not along the line between them
    F[3] = 0.0
    r_F, r_T = cv.residuals(x, F)
    assert np.isnan(r_F[3]) and np.isnan(r_T[3]) and (r_F[[0, 1, 2, 4]] < 1e-16).all() and (r_T[[0, 1, 2, 4]] > 1e-2).all()
    d = x[:, 4] - x[:, 1]
    F[:, 1], F[:, 4] = d, -d                                              # a central force: no torque, c between the two
    r_F, r_T = cv.residuals(x, F)
    assert (r_F < 1e-15).all() and (r_T < 1e-15).all()
    J = np.stack([F, 2 * F, np.zeros_like(F)], 1)                         # Jacobian rows
    j_F, j_T = cv.residuals(x, J)
    assert j_F.shape == (5, 3) and np.isnan(j_F[:, 2]).all() and np.allclose(j_T[:, 0], r_T) and np.allclose(j_T[:, 1], r_T)
    b = cv.bound(np.array([1e-9, 3e-7, np.nan, 2e-7]), ["a", "b", "b", "b"], cv.U[32])
    assert b == {"a": 16 * cv.U[32], "b": 4 * 3e-7}
    v = cv.rigid_tangent(x, 1)
    s = cv.shuffled_tangent(v, 1)
    assert np.allclose(np.linalg.norm(v, axis=-1), np.linalg.norm(s, axis=-1)) and not np.allclose(v, s)
    dist = lambda y: np.linalg.norm(y[:, :, None] - y[:, None], axis=-1)      # noqa: E731
    assert np.abs(dist(x + 1e-6 * v) - dist(x)).max() < 1e-11              # rigid to first order
    assert np.abs(dist(x + 1e-6 * s) - dist(x)).max() > 1e-8


def test_the_jvp_plans_left_out_are_ill_conditioned():
    """Why test_gpu_conservation leaves three dispatch-boundary plans out: the align set's own conditioning is under the threshold"""
    for name in gc.ILL_CONDITIONED:
        c, _, _ = gc.jp._boundary(name)
        assert cv.reference_conditioning(c.xyz, c.align)[0] < cv.CONDITIONING, name


@pytest.mark.parametrize("case", gc.selection_cases(), ids=lambda c: c[0])
def test_selection_keeps_three_quarters_of_every_regime(case):
    """Every (plan, batch) the GPU file runs: the same call it makes, which asserts the share; the pole filter's own share printed"""
    what, xyz, align, feats, n, seed, rotation, angles = case
    redrawn = {}
    for name, (lab, x) in cv.batches(xyz, align, n, seed, feats, rotation, angles, redrawn).items():
        _, share = cv.select(x, lab, xyz, align, feats, (what, name), rotation=rotation, angles=angles)
        print("conservation host selection %s %s: %d of %d frames drawn again; (kept, of, lost to poles) %s" % (what, name, redrawn[name], n, share))
        assert all(0 < k >= cv.KEEP * of for k, of, _ in share.values())
