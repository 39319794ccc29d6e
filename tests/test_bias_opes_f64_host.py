"""molann_value_and_bias_opes_f64 without a GPU: the host selftest of one frame (restraint on all outputs, an OPES term and a table on
chosen columns) against the formulas in torch float64 with dy by autograd and, bit for bit, against the single selftests on y[columns]
added in the order restraint, OPES, table; every refusal code and the order of the codes; the `Opes` record and the Python refusals
that need no device; the exported symbols."""

import ctypes
import itertools
import math
import os

import numpy as np
import pytest
import torch

import test_bias_f64_host as bh
import test_grid_f64_host as gh
import test_hills_f64_host as hh
import test_opes_f64_host as oh
import test_restraint_f64_host as rh
from molann_amd import _capi, ann, bias, workloads as wl
from molann_amd.ann import MolANN, PreprocessingANN
from molann_amd.bias import Grid, Hills, Opes, Restraint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["molann_value_and_bias_opes_f64", "molann_plan_supports_value_and_bias_opes_f64", "molann_selftest_bias_opes_f64"]
F64 = torch.float64
INF = float("inf")
SCALARS = (2.25, 0.05, 1e-3, 4.0)


def selftest(y, opes, restraint=None, grid=None, hills_columns=0, no_terms=False):
    """molann_selftest_bias_opes_f64 on host tensors: opes (columns or None, centers, heights, sigma, period or None, scale, norm, epsilon,
    cutoff); restraint (z, kappa, period or None, flat or None); grid (columns or None, table, lower, spacing, periodic or None).
    `no_terms` passes NULL for the terms.  Returns (code, energies, dy)."""
    d_out = y.numel()
    r = g = None
    if restraint is not None:
        r = restraint + (0,)
    if grid is not None:
        cols, table, lower, spacing, periodic = grid
        g = ((None, table.dim()) if cols is None else cols, table, table.shape, lower, spacing, periodic)
    terms, keep = _capi.bias_terms_f64(r, None, g)
    terms.n_hills_columns = hills_columns
    cols, centers, heights, sigma, period, scale, norm, epsilon, cutoff = opes
    width = centers.shape[1]
    term, keep_o = _capi.opes_term_f64(((None, width) if cols is None else cols, centers, heights, sigma, period, centers.shape[0],
                                        width if sigma.dim() == 2 else 0, scale, norm, epsilon, cutoff), ptr=lambda t: t.data_ptr())
    energies, dy = torch.full((4,), 7.5, dtype=F64), torch.full((d_out,), 7.5, dtype=F64)
    code = _capi.lib().molann_selftest_bias_opes_f64(hh._ptr(y), d_out, None if no_terms else ctypes.byref(terms), ctypes.byref(term),
                                                     hh._ptr(energies), hh._ptr(dy))
    del keep, keep_o
    return code, energies, dy


def _draws(count=2400):
    """Seeded frames: d_out 1..12, every subset of {restraint, table} with the OPES term in turn, column lists of every kind (identity,
    ascending, reversed, random; they overlap each other and the restrained outputs whenever d_out is small), H 0..40, shared or
    per-kernel widths, mixed periodic columns, cutoff inf / 5 / 3, flat bottoms.  y sits near a kernel's centre in half the draws."""
    g = torch.Generator().manual_seed(83)
    f64 = dict(generator=g, dtype=F64)
    subsets = list(itertools.product((False, True), repeat=2))
    draws = []
    for i in range(count):
        d_out = 1 + i % 12
        has_r, has_g = subsets[(i // 12) % 4]
        y = 2.0 * torch.randn(d_out, **f64)
        r = gr = None
        width = 1 + int(torch.randint(0, min(d_out, 8), (1,), generator=g))
        H = int(torch.randint(0, 41, (1,), generator=g))
        cols = bh._columns(g, d_out, width, i // 3)
        centers = 2.0 * torch.randn(H, width, **f64)
        if H and (i // 7) % 2:
            y[list(range(width)) if cols is None else cols] = centers[i % H] + 0.3 * torch.randn(width, **f64)
        heights = 0.2 + torch.rand(H, **f64)
        sigma = 0.2 + 1.5 * torch.rand((H, width) if i % 2 else (width,), **f64)
        period = None
        if i % 3:
            period = torch.where(torch.randint(0, 2, (width,), generator=g) == 0, 1.0 + 5.0 * torch.rand(width, **f64), torch.zeros(width, dtype=F64))
        cutoff, epsilon = (INF, 5.0, 3.0)[(i // 4) % 3], (1e-3, 1e-6)[(i // 48) % 2]
        norm = 0.02 * max(float(heights.sum()), 1.0)
        o = (cols, centers, heights, sigma, period, 2.25 if i % 5 else -0.75, norm, epsilon, cutoff)
        if has_r:
            kappa = 20.0 * torch.randn(d_out, **f64)
            kappa[::3] = 0.0
            pick = torch.randint(0, 3, (2, d_out), generator=g)
            rperiod = torch.where(pick[0] == 0, 0.5 + 6.0 * torch.rand(d_out, **f64), torch.zeros(d_out, dtype=F64))
            flat = torch.where(pick[1] == 0, 2.0 * torch.rand(d_out, **f64), torch.zeros(d_out, dtype=F64))
            r = (2.0 * torch.randn(d_out, **f64), kappa, rperiod if i % 5 else None, flat if i % 4 else None)
        if has_g:
            gw = 1 + int(torch.randint(0, min(d_out, 3), (1,), generator=g))
            shape = [int(n) for n in torch.randint(4, 9, (gw,), generator=g)]
            periodic = [bool(b) for b in torch.randint(0, 2, (gw,), generator=g)]
            lower, spacing = (4.0 * torch.rand(gw, **f64) - 3.0).tolist(), (0.2 + 1.0 * torch.rand(gw, **f64)).tolist()
            gr = (bh._columns(g, d_out, gw, i // 5), 2.0 * torch.randn(shape, **f64), lower, spacing, periodic if i % 6 else None)
        draws.append((y, o, r, gr))
    return draws


def test_selftest_against_the_formulas_and_the_single_selftests():
    """Bounds: per energy column and for dy the single terms' bounds of test_restraint_f64_host (4 ulp of the term's scale, summed over
    the outputs for the energy), test_opes_f64_host (its v_bound and dy_bound) and test_grid_f64_host (1e-12 max(1, sum of the terms'
    magnitudes)), added up.  Bits: the energies are the single selftests' on y[columns], dy their results added in the order restraint,
    OPES, table; column 1 (hills) is +0.0 always."""
    worst = [0.0] * 4
    seen = {"overlap": 0, "reversed": 0, "no_kernels": 0, "past_caps": 0, "flat": 0, "periodic": 0, "per_kernel": 0, "cut": 0}
    combos = set()
    for y, o, r, g in _draws():
        d_out = y.numel()
        code, energies, dy = selftest(y, o, r, g)
        assert code == 0
        ocols = bh._cols(o, o[1].shape[1])
        v_want, dv_want, v_bound, dv_bound, q = oh.formula(y[ocols], *o[1:])
        if q.numel() and float((q - o[8] * o[8]).abs().min()) < 1e-9:
            continue                      # on the cutoff's edge the two may drop different kernels: the derivative jumps there
        e_tol = torch.zeros(4, dtype=F64)
        dy_want, dy_tol, dy_bits, e_bits = torch.zeros(d_out, dtype=F64), torch.zeros(d_out, dtype=F64), torch.zeros(d_out, dtype=F64), [0.0] * 4
        e_want = [0.0] * 4
        if r is not None:
            z, kappa, period, flat = r
            zero = torch.zeros(d_out, dtype=F64)
            seen["flat"] += flat is not None
            period, flat = zero if period is None else period, zero if flat is None else flat
            e_k, dy_k, d = rh.formula(y, z, kappa, period, flat)
            scale = torch.maximum(d.abs(), z.abs()) * kappa.abs()
            dy_tol += 4.0 * torch.from_numpy(np.spacing(scale.numpy()))
            e_terms = 0.5 * scale * torch.maximum(d.abs(), z.abs())
            e_tol[0] = float((4.0 * torch.from_numpy(np.spacing(e_terms.numpy()))).sum()) + d_out * float(np.spacing(float(e_terms.sum())))
            e_want[0], dy_want = float(e_k.sum()), dy_want + dy_k
            e_single, dy_single = rh.selftest(y, z, kappa, period, flat)
            total = 0.0
            for v in e_single.tolist():
                total += v
            e_bits[0], dy_bits = total, dy_single.clone()
        e_want[3], e_tol[3] = v_want, v_bound
        dy_want[ocols] += dv_want
        dy_tol[ocols] += dv_bound
        v_single, dv_single = oh.selftest(y[ocols].contiguous(), *o[1:])
        e_bits[3] = v_single
        dy_bits[ocols] = dy_bits[ocols] + dv_single
        seen["no_kernels"] += o[1].shape[0] == 0
        seen["reversed"] += ocols != sorted(ocols)
        seen["past_caps"] += d_out > 8
        seen["periodic"] += o[4] is not None and bool((o[4] > 0).any())
        seen["per_kernel"] += o[3].dim() == 2
        seen["cut"] += bool((q >= o[8] * o[8]).any())
        if g is not None:
            cols = bh._cols(g, g[1].dim())
            periodic = g[4] if g[4] is not None else [False] * len(cols)
            v, dv, v_scale, dv_scale = gh.formula(y[cols], g[1], torch.tensor(g[2], dtype=F64), torch.tensor(g[3], dtype=F64), periodic)
            e_want[2], e_tol[2] = float(v), 1e-12 * max(1.0, float(v_scale))
            dy_want[cols] += dv
            dy_tol[cols] += 1e-12 * dv_scale.clamp(min=1.0)
            v_single, dv_single = gh.selftest(y[cols], g[1], g[2], g[3], g[4])
            e_bits[2] = v_single
            dy_bits[cols] = dy_bits[cols] + dv_single
            seen["overlap"] += bool(set(cols) & set(ocols))
        combos.add((r is not None, g is not None, o[8]))
        for c in range(4):
            present = (r, None, g, o)[c] is not None
            if not present:
                assert energies[c].item() == 0.0 and not np.signbit(energies[c].item())
                continue
            worst[c] = max(worst[c], abs(float(energies[c]) - e_want[c]) / float(e_tol[c]))
        worst[1] = max(worst[1], float(((dy - dy_want).abs() / dy_tol.clamp(min=1e-300)).max()))
        assert energies.tolist() == e_bits, (energies.tolist(), e_bits)
        assert torch.equal(dy, dy_bits)
    print("worst error / bound: E_r %.3g, dy %.3g, V_g %.3g, V_o %.3g; cases %s" % (*worst, seen))
    assert all(v > 20 for v in seen.values()), seen
    assert len(combos) == 2 * 2 * 3, combos       # every subset of {restraint, table} at every cutoff
    assert max(worst) <= 1.0, worst


def test_opes_alone_is_the_single_selftest_and_null_terms_are_no_terms():
    g = torch.Generator().manual_seed(5)
    y = torch.randn(6, generator=g, dtype=F64)
    centers, heights, sigma = torch.randn((9, 3), generator=g, dtype=F64), torch.rand(9, generator=g, dtype=F64) + 0.1, torch.full((3,), 0.8, dtype=F64)
    for cols in (None, [4, 0, 5]):
        o = (cols, centers, heights, sigma, None) + SCALARS
        picked = y[[0, 1, 2] if cols is None else cols].contiguous()
        v, dv = oh.selftest(picked, centers, heights, sigma, None, *SCALARS)
        for kw in (dict(), dict(no_terms=True)):
            code, energies, dy = selftest(y, o, **kw)
            want = torch.zeros(6, dtype=F64)
            want[[0, 1, 2] if cols is None else cols] += dv
            assert code == 0 and energies.tolist() == [0.0, 0.0, 0.0, v] and torch.equal(dy, want)
            assert not any(np.signbit(e) for e in energies[:3].tolist())
    # no kernels: scale log(epsilon), no share of dy, the table's pointers not needed
    code, energies, dy = selftest(y, (None, centers[:0], heights[:0], sigma, None) + SCALARS, restraint=(torch.zeros(6, dtype=F64), torch.ones(6, dtype=F64), None, None))
    assert code == 0 and energies[3].item() == SCALARS[0] * math.log(SCALARS[2]) and torch.equal(dy, y) and energies[0].item() > 0.0
    term, _ = _capi.opes_term_f64(((None, 3), None, None, None, None, 0, 0) + SCALARS)
    out = torch.full((10,), 7.5, dtype=F64)
    assert _capi.lib().molann_selftest_bias_opes_f64(hh._ptr(y), 6, None, ctypes.byref(term), hh._ptr(out[:4]), hh._ptr(out[4:])) == 0
    assert out[3].item() == SCALARS[0] * math.log(SCALARS[2]) and bool((out[4:] == 0.0).all())


def test_selftest_refusals_in_the_order_of_the_entry():
    E = _capi
    y = torch.linspace(-1.0, 1.0, 10, dtype=F64)
    z, k = torch.zeros(10, dtype=F64), torch.ones(10, dtype=F64)
    centers, heights, sigma = torch.zeros((3, 2), dtype=F64), torch.ones(3, dtype=F64), torch.ones(2, dtype=F64)
    table = torch.zeros((4, 5), dtype=F64)
    wide = lambda n: torch.zeros((3, n), dtype=F64)        # noqa: E731

    def opes(cols, c=centers, s=sigma, scalars=SCALARS):
        return (cols, c, heights, s, None) + tuple(scalars)

    def grid(cols, t=table, lower=(0.0, 0.0), spacing=(1.0, 1.0)):
        return (cols, t, list(lower)[:t.dim()], list(spacing)[:t.dim()], None)

    assert selftest(y, opes([7, 2]), (z, k, None, None), grid([9, 0]))[0] == 0
    out = torch.full((14,), 7.5, dtype=F64)
    terms, _ = _capi.bias_terms_f64()
    assert _capi.lib().molann_selftest_bias_opes_f64(hh._ptr(y), 10, ctypes.byref(terms), None, hh._ptr(out[:4]), hh._ptr(out[4:])) == E.E_NULL   # opes is required
    assert bool((out == 7.5).all())
    bad_grid, bad_cols, hills = grid([0, 1], table, (0.0, 0.0), (1.0, 0.0)), opes([2, 10]), dict(hills_columns=2)
    cases = [
        # MOLANN_E_DESC: the count, the stride, the four scalars, the grid
        (dict(opes=opes([7, 2], scalars=(float("nan"), 0.05, 1e-3, 4.0))), E.E_DESC),
        (dict(opes=opes([7, 2], scalars=(2.25, 0.0, 1e-3, 4.0))), E.E_DESC),
        (dict(opes=opes([7, 2], scalars=(2.25, 0.05, -1e-3, 4.0))), E.E_DESC),
        (dict(opes=opes([7, 2], scalars=(2.25, 0.05, 1e-3, 0.0))), E.E_DESC),
        (dict(opes=opes([7, 2], scalars=(2.25, 0.05, 1e-3, float("nan")))), E.E_DESC),
        (dict(opes=opes([7, 2]), grid=bad_grid), E.E_DESC),
        # ... before the hills' MOLANN_E_UNSUPPORTED, which comes before the columns' codes
        (dict(opes=opes([7, 2], scalars=(2.25, 0.0, 1e-3, 4.0)), **hills), E.E_DESC),
        (dict(opes=opes([7, 2]), grid=bad_grid, **hills), E.E_DESC),
        (dict(opes=opes([7, 2]), **hills), E.E_UNSUPPORTED),
        (dict(opes=bad_cols, **hills), E.E_UNSUPPORTED),
        (dict(opes=opes([7, 2]), hills_columns=-1), E.E_UNSUPPORTED),
        # the columns: MOLANN_E_INDEX, MOLANN_E_UNSUPPORTED past 8 / 3, INDEX before UNSUPPORTED, the OPES list before the table's
        (dict(opes=bad_cols), E.E_INDEX), (dict(opes=opes([-1, 2])), E.E_INDEX), (dict(opes=opes([4, 4])), E.E_INDEX),
        (dict(opes=opes([7, 2]), grid=grid([3, 3])), E.E_INDEX), (dict(opes=opes([7, 2]), grid=grid([0, 10])), E.E_INDEX),
        (dict(opes=opes(list(range(9)), wide(9), torch.ones(9, dtype=F64))), E.E_UNSUPPORTED),
        (dict(opes=opes(None, wide(9), torch.ones(9, dtype=F64))), E.E_UNSUPPORTED),
        (dict(opes=opes(list(range(8)) + [8, 8], wide(10), torch.ones(10, dtype=F64))), E.E_INDEX),
        (dict(opes=opes(list(range(9)), wide(9), torch.ones(9, dtype=F64)), grid=grid([3, 3])), E.E_UNSUPPORTED),
        (dict(opes=opes([7, 2]), grid=(None, torch.zeros((4, 4, 4, 4), dtype=F64), [0.0] * 4, [1.0] * 4, None)), E.E_UNSUPPORTED),
        (dict(opes=bad_cols, grid=bad_grid), E.E_DESC),
    ]
    for bad, code in cases:
        got, energies, dy = selftest(y, bad.pop("opes"), **bad)
        assert got == code, (bad, got, code)
        assert bool((energies == 7.5).all()) and bool((dy == 7.5).all())
    # counts and strides the helper above cannot say
    for change, code in ((dict(n_columns=0), E.E_DESC), (dict(n_columns=-2), E.E_DESC), (dict(n_kernels=-1), E.E_DESC), (dict(sigma_stride=1), E.E_DESC),
                         (dict(sigma_stride=10), E.E_DESC), (dict(n_kernels=3, centers=None), E.E_NULL), (dict(n_kernels=3, sigma=None), E.E_NULL)):
        term, keep = _capi.opes_term_f64(((None, 2), centers, heights, sigma, None, 3, 0) + SCALARS)
        for name, v in change.items():
            setattr(term, name, v)
        assert _capi.lib().molann_selftest_bias_opes_f64(hh._ptr(y), 10, None, ctypes.byref(term), hh._ptr(out[:4]), hh._ptr(out[4:])) == code, change
        assert bool((out == 7.5).all())
    short = y[:2].contiguous()
    assert selftest(short, opes(None, wide(3), torch.ones(3, dtype=F64)))[0] == E.E_INDEX      # d_out too small for 0..2
    assert selftest(short, opes(None), grid=grid(None, torch.zeros((4, 4, 4), dtype=F64), (0.0,) * 3, (1.0,) * 3))[0] == E.E_INDEX


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_declared_exported_and_bound(name):
    header = open(os.path.join(ROOT, "include", "molann_hip.h")).read()
    assert name + "(" in header, name
    fn = getattr(_capi.lib(), name)
    assert fn.argtypes is not None and len(fn.argtypes) == {SYMBOLS[0]: 11, SYMBOLS[1]: 1, SYMBOLS[2]: 6}[name], name
    assert name in _capi.declared_symbols()


def test_null_plan_and_abi():
    L = _capi.lib()
    assert L.molann_plan_supports_value_and_bias_opes_f64(None) == _capi.E_NULL
    terms, _ = _capi.bias_terms_f64()
    term, _ = _capi.opes_term_f64(((None, 2), None, None, None, None, 0, 0) + SCALARS)
    for n in (1, 0, -1):
        assert L.molann_value_and_bias_opes_f64(None, None, n, None, None, ctypes.byref(terms), ctypes.byref(term), None, None, None, None) == _capi.E_NULL
        assert L.molann_value_and_bias_opes_f64(None, None, n, None, None, None, None, None, None, None, None) == _capi.E_NULL
    assert L.molann_abi_version() == 1
    # the structs' layouts are the header's: the old one unchanged, the new one 12 fields on 8-byte boundaries
    assert ctypes.sizeof(_capi.BiasTermsF64) == 20 * 8 and ctypes.sizeof(_capi.OpesTermF64) == 12 * 8 and _capi.OpesTermF64.scale.offset == 8 * 8


def test_methods_exist_and_say_what_is_out_of_scope():
    assert callable(_capi.Plan.supports_value_and_bias_opes_f64) and callable(_capi.Plan.value_and_bias_opes_f64) and callable(_capi.Plan.value_and_bias_opes)
    doc = " ".join(MolANN.value_and_bias.__doc__.split())
    for words in ("``opes``", "frames_value_bias_opes_f64_kernel", "[N, 4]", "add_hills_to_grid", "more than one OPES term"):
        assert words in doc, (words, doc)
    assert "opes" in PreprocessingANN.value_and_bias.__doc__ and "``opes=``" in MolANN.value_and_opes.__doc__
    assert "Opes" in bias.__all__
    assert ann._ONE_LAUNCH_NAME[ann._BIAS_OPES] == "value_and_bias" and ann._ONE_LAUNCH_OP[ann._BIAS_OPES] == "op_bias_opes"
    assert len({len(t) for t in (ann._ONE_LAUNCH_NAME, ann._ONE_LAUNCH_ROUTE, ann._ONE_LAUNCH_FEATURES_ROUTE, ann._ONE_LAUNCH_PAIR, ann._ONE_LAUNCH_OP)}) == 1
    for text in (open(os.path.join(ROOT, "include", "molann_hip.h")).read(), open(os.path.join(ROOT, "molann_amd", "csrc", "molann_dev_opes_f64.inc")).read(),
                 MolANN.value_and_opes.__doc__):
        assert "an OPES term inside" not in " ".join(text.split())


def test_the_record_is_immutable_and_checks_its_columns():
    t = torch.zeros((4, 2), dtype=F64)
    o = Opes(t, 1.0, 0.5, 2.25, 1.0, 1e-3, columns=[3, 1])
    assert o.columns == (3, 1) and o.cutoff is None and o.period is None and (o.scale, o.norm, o.epsilon) == (2.25, 1.0, 1e-3)
    assert Opes(t, 1.0, 0.5, 2.25, 1.0, 1e-3, 4.0, None, range(2)).columns == (0, 1) and Opes(t, 1.0, 0.5, 2.25, 1.0, 1e-3, cutoff=4.0).columns is None
    with pytest.raises(AttributeError):
        o.norm = 2.0
    assert o._replace(norm=2.0).norm == 2.0 and o._replace(norm=2.0).centers is t
    for bad in ("01", 3, {0, 1}, torch.tensor([0, 1]), [0.0, 1.0], [True, False], [0, "1"]):
        with pytest.raises(TypeError, match="Opes: `columns`"):
            Opes(t, 1.0, 0.5, 2.25, 1.0, 1e-3, columns=bad)
    for bad in ([0, 0], [2, 1, 2], [-1, 0]):
        with pytest.raises(IndexError, match="Opes: `columns`"):
            Opes(t, 1.0, 0.5, 2.25, 1.0, 1e-3, columns=bad)
    with pytest.raises(NotImplementedError, match=r"Opes: .*at most 8 columns \(got 9\).*opes_kernel_sum.*value_and_vjp"):
        Opes(t, 1.0, 0.5, 2.25, 1.0, 1e-3, columns=list(range(9)))


def test_cpu_tensor_names_the_route_and_the_terms_are_checked_before_the_gate():
    w = wl.get_workload("C3")
    model = wl.build_model(w, torch.device("cpu"), 0).double().requires_grad_(False)
    x = w.make_frames(3, seed=1).double()
    d = w.out_dim()
    r = Restraint(torch.zeros(d, dtype=F64), 2.0)
    o = Opes(torch.zeros((4, 3), dtype=F64), 1.0, 0.5, 2.25, 1.0, 1e-3, 4.0, columns=[0, 3, 7])
    h = Hills(torch.zeros((4, 2), dtype=F64), 1.0, 0.5)
    with pytest.raises(NotImplementedError, match=r"the kernel sum with `molann_amd\.bias\.opes_kernel_sum`, their derivatives with torch, then `value_and_vjp`"):
        model.value_and_bias(x, restraint=r, opes=o)
    with pytest.raises(NotImplementedError, match=r"opes_kernel_sum`\) with torch and take torch\.autograd\.grad"):
        model.preprocessing_layer.value_and_bias(x, opes=Opes(torch.zeros((4, 2), dtype=F64), 1.0, 0.5, 2.25, 1.0, 1e-3))
    with pytest.raises(NotImplementedError, match="opes_kernel_sum"):     # the gate comes before `into` and before the term's own arguments
        model.value_and_bias(x, opes=Opes(None, 1.0, -0.5, float("nan"), 0.0, 1e-3, columns=[70]), into=(x,))
    for target in (model, model.preprocessing_layer):
        with pytest.raises(ValueError, match="at least one of `restraint`, `hills` and `grid`"):
            target.value_and_bias(x, opes=None)
        with pytest.raises(NotImplementedError, match=r"`hills` and `opes` in one launch.*add_hills_to_grid.*two calls"):    # before the device gate
            target.value_and_bias(x, hills=h, opes=o)
        for bad in (h, r, (o.centers, 1.0, 0.5, 2.25, 1.0, 1e-3), "opes"):
            with pytest.raises(TypeError, match=r"`opes` must be None or a molann_amd\.bias\.Opes"):
                target.value_and_bias(x, restraint=r if target is model else None, opes=bad)
    # without `opes` the call is what it was: the same route strings
    with pytest.raises(NotImplementedError, match=r"form the terms and their derivatives on the chosen columns with torch, then `value_and_vjp`"):
        model.value_and_bias(x, restraint=r)


def test_arguments_are_checked_before_any_device_call():
    """ann._check_bias_opes_args is what both methods call before the plan is looked up: the columns against the model, then the
    restraint, the OPES term (by _check_opes_args with the term's width) and the table, then `into` with energies [N, 4]."""
    n, n_inp, d = 5, 22, 12
    x = torch.zeros((n, n_inp, 3), dtype=F64)
    y, energies, dx = torch.zeros((n, d), dtype=F64), torch.zeros((n, 4), dtype=F64), torch.zeros_like(x)
    z, k = torch.zeros(d, dtype=F64), torch.ones(d, dtype=F64)
    centers, heights, sigma = torch.zeros((4, 3), dtype=F64), torch.ones(4, dtype=F64), torch.full((3,), 0.5, dtype=F64)
    table = torch.zeros((5, 6), dtype=F64)
    R, G = Restraint(z, k), Grid(table, [0.0, 0.0], [1.0, 1.0], [True, False], columns=[9, 11])
    O = Opes(centers, heights, sigma, 2.25, 1.0, 1e-3, 4.0, columns=[11, 0, 4])

    def check(restraint=R, grid=G, opes=O, into=None, d_out=d):
        return ann._check_bias_opes_args("value_and_bias", x, d_out, restraint, grid, opes, into)

    r, g, o, *into = check(into=(y, energies, dx))
    assert r[0].data_ptr() == z.data_ptr() and r[2:] == (None, None)
    assert g[0] == (9, 11) and g[1].data_ptr() == table.data_ptr() and g[2:] == ([0.0, 0.0], [1.0, 1.0], [True, False])
    assert o[0] == (11, 0, 4) and o[1].data_ptr() == centers.data_ptr() and o[3].data_ptr() == sigma.data_ptr() and o[4] is None
    assert o[5:] == (2.25, 1.0, 1e-3, 4.0) and into[0] is y and into[1] is energies and into[2] is dx
    r, g, o, *into = check(restraint=None, grid=None, opes=Opes(centers.tolist(), 0.7, 0.4, 2, 1, 1e-3))
    assert r is None and g is None and o[0] == (0, 1, 2) and o[8] == INF and into == [None, None, None]
    assert torch.equal(o[2], torch.full((4,), 0.7, dtype=F64)) and torch.equal(o[3], torch.full((3,), 0.4, dtype=F64))      # the conversions
    with pytest.raises(IndexError, match=r"opes.columns.*\[0, 12\)"):
        check(opes=O._replace(columns=(0, 12, 4)))
    with pytest.raises(IndexError, match="3 columns but the model has 2 outputs"):
        check(restraint=None, grid=None, opes=O._replace(columns=None), d_out=2)
    with pytest.raises(NotImplementedError, match="at most 8 opes columns"):
        check(opes=Opes(torch.zeros((4, 9), dtype=F64), heights, 0.5, 2.25, 1.0, 1e-3))
    with pytest.raises(ValueError, match=r"`opes.centers` must be \[H, columns\].*no kernels yet"):
        check(opes=Opes([], [], 0.5, 2.25, 1.0, 1e-3))
    assert check(opes=Opes([], [], 0.5, 2.25, 1.0, 1e-3, columns=[11, 0]))[2][1].shape == (0, 2)
    # the term's own checks, with the term's width in place of the number of outputs; the scalars' ValueErrors are value_and_opes'
    with pytest.raises(ValueError, match=r"centers.*\[4, 3\]"):
        check(opes=O._replace(centers=torch.zeros((4, 12), dtype=F64)))
    with pytest.raises(ValueError, match="sigma"):
        check(opes=O._replace(sigma=sigma * 0.0))
    for change, words in ((dict(scale=INF), "`scale` must be finite"), (dict(norm=0.0), "`norm` must be finite and > 0"),
                          (dict(epsilon=-1.0), "`epsilon` must be finite and > 0"), (dict(cutoff=0.0), r"`cutoff` must be None \(no cutoff\) or > 0")):
        with pytest.raises(ValueError, match=words):
            check(opes=O._replace(**change))
    with pytest.raises(TypeError, match="`norm` must be a Python float"):
        check(opes=O._replace(norm=torch.tensor(1.0)))
    with pytest.raises(ValueError, match="flat"):
        check(restraint=Restraint(z, k, flat=-k))
    with pytest.raises(ValueError, match="spacing"):
        check(grid=Grid(table, [0.0] * 2, [1.0, 0.0], columns=[9, 11]))
    # `into`: a triple with energies [N, 4]; the [N, 3] of the call without `opes` is refused
    with pytest.raises(TypeError, match=r"triple of tensors \(y, energies, dx\)"):
        check(into=(y, dx))
    with pytest.raises(TypeError, match="float64"):
        check(into=(y, energies.float(), dx))
    for bad in ((y, energies[:, :3].contiguous(), dx), (y, energies[:, 0].contiguous(), dx), (y[:, :3].contiguous(), energies, dx), (y, energies, dx[1:]),
                (y, energies.t(), dx), (y, energies.to("meta"), dx)):
        with pytest.raises(ValueError, match=r"\[5, 12\], \[5, 4\]"):
            check(into=bad)
    # and without an OPES term `into` is what it was
    assert ann._check_bias_args("value_and_bias", x, d, R, None, G, (y, energies[:, :3].contiguous(), dx))[3] is y
