"""The head-parameter builders of tests/head_extremes.py, the scalar activation code of molann_amd/csrc/molann_math.h on the values
those builders reach (through the host build's self-test hooks), and the condition the reference alone must meet: the oracle run
in float32 on the CPU stays inside every fixed bound tests/test_gpu_head_extremes.py holds the kernels to.  No GPU.

The host build runs libm where the device runs its own exp2 / exp / rcp, so the scalar tests say that the FORMULAS hold out to
|z| = 130 (float64: 750); what the device's arithmetic makes of them is the GPU file's question."""

import numpy as np
import pytest
import torch

import head_extremes as he
from molann_amd import _capi
from molann_amd import workloads as wl
from oracle import molann_oracle as mo

DIMS = [6, 16, 8, 4]
N = 128
_CACHE = {}


def _features():
    """C3's features of 128 frames through the float64 oracle, computed once."""
    if "f" not in _CACHE:
        w = wl.get_workload("C3")
        x = w.make_frames(N, seed=3).double()
        feats = [(t, [a - 1 for a in atoms]) for t, atoms in w.features]
        al = [a - 1 for a in w.align]
        ref = mo.center_reference(torch.from_numpy(w.ref_xyz[al])).double()
        with torch.no_grad():
            _CACHE["f"] = mo.preprocessing_forward(x, feats, w.use_angle_value, al, ref)
    return _CACHE["f"]


# ---- the builders --------------------------------------------------------------------------------------------------------------
def test_builders_are_deterministic_and_leave_the_generator_alone():
    state = torch.random.get_rng_state()
    for regime in he.REGIMES:
        a, b = he.params(DIMS, regime), he.params(DIMS, regime)
        assert all(torch.equal(p, q) for p, q in zip(a[0] + a[1], b[0] + b[1])), regime
    assert torch.equal(torch.random.get_rng_state(), state)
    Wc, bc = he.params(DIMS, "control")
    Wm, bm = he.params(DIMS, "mixed")
    fac = torch.tensor([he.MIXED_FACTORS[j % 6] for j in range(16)], dtype=torch.float32)
    assert torch.equal(Wm[0], Wc[0] * fac[:, None]) and torch.equal(bm[0], bc[0] * fac)
    assert torch.equal(Wm[-1], Wc[-1]) and torch.equal(bm[-1], bc[-1])            # the output layer is never scaled
    W64 = he.params(DIMS, "control", torch.float64)[0]
    assert all(torch.equal(a.double(), b) for a, b in zip(Wc, W64))


@pytest.mark.parametrize("code", [he.TANH, he.SIGMOID])
def test_mixed_has_live_units_next_to_every_band(code):
    f = _features()
    share = he.bands(he.hidden_z(f, *he.params(DIMS, "mixed"), code))               # [N, 5]
    print("mixed %s: least share of a frame in [0,2) %.3f, batch shares %s" % (
        he.NAMES[code], float(share[:, 0].min()), share.mean(0).tolist()))
    assert float(share[:, 0].min()) >= 0.25
    assert bool((share[:, 1:].sum(0) > 0).all()), share.mean(0)
    control = he.bands(he.hidden_z(f, *he.params(DIMS, "control"), code))
    assert float(control[:, 0].min()) >= 0.9                                          # what every other GPU test runs on


def test_saturated_leaves_no_live_unit_in_the_first_layer():
    f = _features()
    z1 = he.hidden_z(f, *he.params(DIMS, "saturated"), he.TANH)[:, :DIMS[1]]
    none_live = (z1.abs() >= 2.0).all(1)
    print("saturated: %d of %d frames have no first-layer unit in [0,2)" % (int(none_live.sum()), N))
    assert float(none_live.double().mean()) >= 0.5


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("dims", [DIMS, [6, 100, 70, 3], [33, 40, 24, 7]], ids=str)
def test_pinned_units_reproduce_their_bias(dims, dtype):
    """z of a pinned unit is its bias bit for bit on every frame, in the head's own dtype.  (A bias of -0.0 comes out as +0.0: the
    zero products sum to +0 and +0 + -0 = +0 in IEEE arithmetic, whatever computes it.  Both zeros are the same side of the kink;
    the value is checked for equality there, every other one for its bits.)"""
    g = torch.Generator().manual_seed(1)
    f = _features().to(dtype) if dims[0] == 6 else torch.randn(N, dims[0], generator=g, dtype=torch.float64).to(dtype)
    vals, seen = he.pinned_values(dtype), []
    assert bool(torch.isfinite(vals).all())
    for part in range(he.n_parts(dims, dtype)):
        Ws, bs = he.params(dims, "pinned", dtype, part=part)
        units = he.pinned_units(dims, dtype, part)
        assert 0 < len(units) <= dims[1] // 2
        with torch.no_grad():
            _, kept = he.head(f, Ws, bs, he.TANH, keep=True)
        z1 = kept[0][0]
        for j, v in units:
            col = z1[:, j]
            if float(v) == 0.0:
                assert bool((col == 0.0).all())
            else:
                assert torch.equal(col.view(torch.int32 if dtype == torch.float32 else torch.int64),
                                   v.expand(N).contiguous().view(torch.int32 if dtype == torch.float32 else torch.int64)), (j, float(v))
            seen.append(float(v))
        Wc, bc = he.params(dims, "control", dtype)
        rest = [j for j in range(dims[1]) if j >= len(units)]
        assert torch.equal(Ws[0][rest], Wc[0][rest]) and torch.equal(bs[0][rest], bc[0][rest])
    assert len(seen) == len(vals) and np.array_equal(np.array(seen), vals.double().numpy())    # the whole list, in order
    v32 = he.pinned_values(torch.float32)
    assert float(v32[5]) == 20.0 + 2.0 ** -19 and float(v32[6]) == 20.0 - 2.0 ** -19              # float32's neighbours of 20
    assert float(he.pinned_values(torch.float64)[5]) == 20.0 + 2.0 ** -48


# ---- the scalar functions ------------------------------------------------------------------------------------------------------
def _grid(dtype):
    top = 130.0 if dtype == torch.float32 else 750.0
    g = torch.cat([torch.linspace(-top, top, 2601, dtype=torch.float64), torch.linspace(-12, 12, 961, dtype=torch.float64),
                   he.pinned_values(dtype).double()])
    return g.to(dtype).double()                                                       # the values as the hook receives them


@pytest.mark.parametrize("code", he.ALL, ids=he.NAMES)
def test_activation_values_out_to_130(code):
    """apply_activation within test_host_math.py's bound (atol 3e-7, rtol 3e-7) of torch in float64, finite for every finite z."""
    z = _grid(torch.float32)
    want = he.FN[code](z).numpy()
    fn = _capi.lib().molann_selftest_activation
    got = np.array([fn(code, float(v)) for v in z.tolist()])
    assert np.isfinite(got).all(), z[~np.isfinite(got)]
    err = np.abs(got - want) - (3e-7 + 3e-7 * np.abs(want))
    assert (err <= 0).all(), (float(z[int(err.argmax())]), float(got[int(err.argmax())]), float(want[int(err.argmax())]))


@pytest.mark.parametrize("code", he.ALL, ids=he.NAMES)
def test_act_derivative_f64_out_to_750(code):
    """act_derivative_f64 within test_act_derivative_f64_host.py's bound (1e-13 + 1e-12 |want|) of torch's float64 autograd, at the
    kink torch's convention exactly, finite for every finite z."""
    z = _grid(torch.float64)
    want = he.act_derivative(code, z)
    fn = _capi.lib().molann_selftest_act_derivative_f64
    got = torch.tensor([fn(code, float(v)) for v in z.tolist()], dtype=torch.float64)
    assert bool(torch.isfinite(got).all()), z[~torch.isfinite(got)]
    err = (got - want).abs() - (1e-13 + 1e-12 * want.abs())
    worst = int(err.argmax())
    assert bool((err <= 0).all()), (float(z[worst]), float(got[worst]), float(want[worst]))
    at0 = z == 0.0
    assert int(at0.sum()) >= 2 and torch.equal(got[at0], want[at0])


@pytest.mark.parametrize("code", he.SERVED, ids=[he.NAMES[c] for c in he.SERVED])
def test_act_derivative_f32_out_to_130(code):
    """The float32 act_derivative (from h; SiLU from z) of the six served codes within test_host_math.py's absolute 2e-6 of torch's
    float64 autograd, at +-0 torch's float32 convention exactly, finite."""
    z = _grid(torch.float32)
    want = he.act_derivative(code, z)
    fn = _capi.lib().molann_selftest_act_derivative
    got = torch.tensor([fn(code, float(v)) for v in z.tolist()], dtype=torch.float64)
    assert bool(torch.isfinite(got).all()), z[~torch.isfinite(got)]
    err = (got - want).abs()
    assert float(err.max()) <= 2e-6, (float(z[int(err.argmax())]), float(err.max()))
    at0 = z == 0.0
    assert int(at0.sum()) >= 2 and torch.equal(got[at0], he.act_derivative(code, z[at0].float()).double())


def test_unserved_codes_have_no_float32_derivative():
    """act_derivative falls through to 1.0 for ELU, Softplus and GELU: nothing may reach it with them.  Pinned here so that a
    fourth served code changes this test and the plans' gate (act_served) together."""
    fn = _capi.lib().molann_selftest_act_derivative
    for code in he.UNSERVED:
        assert [fn(code, v) for v in (-3.0, 0.5)] == [1.0, 1.0], code


# ---- the reference alone -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("code", he.ALL, ids=he.NAMES)
@pytest.mark.parametrize("dims", [DIMS, [6, 100, 70, 3]], ids=str)
def test_float32_oracle_meets_the_fixed_bounds(dims, code):
    """The oracle in float32 on the CPU, every regime: finite; the pinned units' rows of dL/db1 and dL/dW1 equal to
    sum g act'(b) (feature) within the gradient bound; `mixed` with the saturated units cut off equal to the live sub-network
    within the bound of the live sub-network's own float32 run.  (Every other bound of the GPU file is max(a tolerance, twice this
    oracle's error): met by the oracle by construction.)"""
    f = _features()
    G = torch.randn(N, dims[-1], generator=torch.Generator().manual_seed(5), dtype=torch.float64)
    kind = "wide_bwd" if dims[1] > 32 else "f32"
    for label, regime, part, (Ws, bs) in he.parameter_sets(dims):
        want = he.head_oracle(f, Ws, bs, code, G)
        own = he.head_oracle(f.float(), Ws, bs, code, G, torch.float32)
        res, bad = he.compare(own, want, own, kind)
        assert not bad, (label, bad)
        if regime == "pinned":
            bad = he.check_pinned(own["gp"], want, f, code, he.pinned_units(dims, torch.float32, part), (res["param 0"][1], res["param 1"][1]))
            assert not bad, (label, bad)
        if regime == "mixed":
            Wz, (Wl, bl) = he.isolate(Ws, bs, dims)
            live = he.head_oracle(f, Wl, bl, code, G)
            live32 = he.head_oracle(f.float(), Wl, bl, code, G, torch.float32)
            cut32 = he.head_oracle(f.float(), Wz, bs, code, G, torch.float32)
            res, bad = he.compare({"y": cut32["y"], "D": cut32["D"], "gp": []}, {"y": live["y"], "D": live["D"], "gp": []},
                                  {"y": live32["y"], "D": live32["D"], "gp": []}, kind)
            assert not bad, (label, "isolation", bad)


@pytest.mark.parametrize("code", he.ALL, ids=he.NAMES)
def test_bf16_emulation_spread(code):
    """The bf16 reference's own spread under +-1 float32 ulp of every activation, per regime: printed, finite, and the bound built
    from it never below test_gpu_mlp_chain.py's 4e-3."""
    dims = [33, 40, 24, 7]
    f = torch.randn(N, dims[0], generator=torch.Generator().manual_seed(2))
    for label, _, _, (Ws, bs) in he.parameter_sets(dims):
        ref, bound, spread = he.bf16_bound(f, Ws, bs, code)
        print("bf16 emulation %s %s: spread %.3g of the scale" % (he.NAMES[code], label, spread))
        assert bool(torch.isfinite(ref).all()) and bound >= 4e-3 * max(1.0, float(ref.abs().max()))
