"""molann_value_and_bias_f64 without a GPU: the host selftest of one frame (restraint on all outputs, hills and a table on chosen
columns) against the formulas in torch and, bit for bit, against the three single selftests on y[columns]; the Python refusals that
need no device; the exported symbols."""

import ctypes
import itertools
import os

import numpy as np
import pytest
import torch

import test_grid_f64_host as gh
import test_hills_f64_host as hh
import test_restraint_f64_host as rh
from molann_amd import _capi, ann, bias, workloads as wl
from molann_amd.ann import MolANN, PreprocessingANN
from molann_amd.bias import Grid, Hills, Restraint

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["molann_value_and_bias_f64", "molann_plan_supports_value_and_bias_f64", "molann_selftest_bias_f64"]
F64 = torch.float64


def selftest(y, restraint=None, hills=None, grid=None):
    """molann_selftest_bias_f64 on host tensors: restraint (z, kappa, period or None, flat or None); hills (columns or None, centers,
    heights, sigma, period or None); grid (columns or None, table, lower, spacing, periodic or None).  Returns (code, energies, dy)."""
    d_out = y.numel()
    r = h = g = None
    if restraint is not None:
        r = restraint + (0,)
    if hills is not None:
        cols, centers, heights, sigma, period = hills
        width = centers.shape[1]
        h = ((None, width) if cols is None else cols, centers, heights, sigma, period, centers.shape[0], width if sigma.dim() == 2 else 0)
    if grid is not None:
        cols, table, lower, spacing, periodic = grid
        g = ((None, table.dim()) if cols is None else cols, table, table.shape, lower, spacing, periodic)
    terms, keep = _capi.bias_terms_f64(r, h, g)
    energies, dy = torch.full((3,), 7.5, dtype=F64), torch.full((d_out,), 7.5, dtype=F64)
    code = _capi.lib().molann_selftest_bias_f64(hh._ptr(y), d_out, ctypes.byref(terms), hh._ptr(energies), hh._ptr(dy))
    del keep
    return code, energies, dy


def _columns(g, d_out, width, i):
    """`width` distinct outputs: ascending, reversed, or in a random order, in turn; None (the identity) now and then"""
    perm = torch.randperm(d_out, generator=g)[:width].tolist()
    return [None, sorted(perm), sorted(perm, reverse=True), perm][i % 4]


def _draws(count=2100):
    """Seeded frames: d_out 1..12, every subset of the three terms in turn, column lists of every kind (they overlap each other and the
    restrained outputs whenever d_out is small), H 0..40, shared or per-hill widths, mixed periodic flags, flat bottoms."""
    g = torch.Generator().manual_seed(77)
    f64 = dict(generator=g, dtype=F64)
    subsets = [s for s in itertools.product((False, True), repeat=3) if any(s)]
    draws = []
    for i in range(count):
        d_out = 1 + i % 12
        has_r, has_h, has_g = subsets[(i // 12) % 7]
        y = 2.0 * torch.randn(d_out, **f64)
        r = h = gr = None
        if has_r:
            kappa = 20.0 * torch.randn(d_out, **f64)
            kappa[::3] = 0.0
            pick = torch.randint(0, 3, (2, d_out), generator=g)
            period = torch.where(pick[0] == 0, 0.5 + 6.0 * torch.rand(d_out, **f64), torch.zeros(d_out, dtype=F64))
            flat = torch.where(pick[1] == 0, 2.0 * torch.rand(d_out, **f64), torch.zeros(d_out, dtype=F64))
            r = (2.0 * torch.randn(d_out, **f64), kappa, period if i % 5 else None, flat if i % 4 else None)
        if has_h:
            width = 1 + int(torch.randint(0, min(d_out, 8), (1,), generator=g))
            H = int(torch.randint(0, 41, (1,), generator=g))
            heights = 1.5 * torch.randn(H, **f64)
            heights[::5] = 0.0
            sigma = 0.2 + 1.5 * torch.rand((H, width) if i % 2 else (width,), **f64)
            period = None
            if i % 3:
                period = torch.where(torch.randint(0, 2, (width,), generator=g) == 0, 1.0 + 5.0 * torch.rand(width, **f64), torch.zeros(width, dtype=F64))
            h = (_columns(g, d_out, width, i // 3), 2.0 * torch.randn(H, width, **f64), heights, sigma, period)
        if has_g:
            width = 1 + int(torch.randint(0, min(d_out, 3), (1,), generator=g))
            shape = [int(n) for n in torch.randint(4, 9, (width,), generator=g)]
            periodic = [bool(b) for b in torch.randint(0, 2, (width,), generator=g)]
            lower, spacing = (4.0 * torch.rand(width, **f64) - 3.0).tolist(), (0.2 + 1.0 * torch.rand(width, **f64)).tolist()
            gr = (_columns(g, d_out, width, i // 5), 2.0 * torch.randn(shape, **f64), lower, spacing, periodic if i % 6 else None)
        draws.append((y, r, h, gr))
    return draws


def _cols(term, width):
    return list(range(width)) if term[0] is None else list(term[0])


def test_selftest_against_the_formulas_and_the_single_selftests():
    """Bounds: per energy column and for dy the single terms' bounds of test_restraint_f64_host (4 ulp of the term's scale, summed over
    the outputs for the energy), test_hills_f64_host and test_grid_f64_host (1e-12 max(1, sum of the terms' magnitudes)), added up.
    Bits: the energies are the single selftests' on y[columns], dy their results added in the order restraint, hills, table."""
    worst = [0.0] * 4
    seen = {"overlap": 0, "reversed": 0, "no_hills": 0, "past_caps": 0}
    for y, r, h, g in _draws():
        d_out = y.numel()
        code, energies, dy = selftest(y, r, h, g)
        assert code == 0
        e_tol = torch.zeros(3, dtype=F64)
        dy_want, dy_tol, dy_bits, e_bits = torch.zeros(d_out, dtype=F64), torch.zeros(d_out, dtype=F64), torch.zeros(d_out, dtype=F64), [0.0] * 3
        e_want = [0.0] * 3
        if r is not None:
            z, kappa, period, flat = r
            zero = torch.zeros(d_out, dtype=F64)
            period, flat = zero if period is None else period, zero if flat is None else flat
            e_k, dy_k, d = rh.formula(y, z, kappa, period, flat)
            scale = torch.maximum(d.abs(), z.abs()) * kappa.abs()
            dy_tol += 4.0 * torch.from_numpy(np.spacing(scale.numpy()))
            # every term within 4 ulp of its scale, and the sum of d_out terms rounds d_out - 1 times more
            e_terms = 0.5 * scale * torch.maximum(d.abs(), z.abs())
            e_tol[0] = float((4.0 * torch.from_numpy(np.spacing(e_terms.numpy()))).sum()) + d_out * float(np.spacing(float(e_terms.sum())))
            e_want[0], dy_want = float(e_k.sum()), dy_want + dy_k
            e_single, dy_single = rh.selftest(y, z, kappa, period, flat)
            total = 0.0
            for v in e_single.tolist():
                total += v
            e_bits[0], dy_bits = total, dy_single.clone()
        if h is not None:
            cols = _cols(h, h[1].shape[1])
            v, dv, v_scale, dv_scale = hh.formula(y[cols], h[1], h[2], h[3], h[4])
            e_want[1], e_tol[1] = float(v), 1e-12 * max(1.0, float(v_scale))
            dy_want[cols] += dv
            dy_tol[cols] += 1e-12 * dv_scale.clamp(min=1.0)
            v_single, dv_single = hh.selftest(y[cols].contiguous(), h[1], h[2], h[3], h[4])
            e_bits[1] = v_single
            dy_bits[cols] = dy_bits[cols] + dv_single
            seen["no_hills"] += h[1].shape[0] == 0
            seen["reversed"] += cols != sorted(cols)
            seen["past_caps"] += d_out > 8
        if g is not None:
            cols = _cols(g, g[1].dim())
            periodic = g[4] if g[4] is not None else [False] * len(cols)
            v, dv, v_scale, dv_scale = gh.formula(y[cols], g[1], torch.tensor(g[2], dtype=F64), torch.tensor(g[3], dtype=F64), periodic)
            e_want[2], e_tol[2] = float(v), 1e-12 * max(1.0, float(v_scale))
            dy_want[cols] += dv
            dy_tol[cols] += 1e-12 * dv_scale.clamp(min=1.0)
            v_single, dv_single = gh.selftest(y[cols], g[1], g[2], g[3], g[4])
            e_bits[2] = v_single
            dy_bits[cols] = dy_bits[cols] + dv_single
            if h is not None:
                seen["overlap"] += bool(set(cols) & set(_cols(h, h[1].shape[1])))
        for c in range(3):
            present = (r, h, g)[c] is not None
            if not present:
                assert energies[c].item() == 0.0 and not np.signbit(energies[c].item())
                continue
            worst[c] = max(worst[c], abs(float(energies[c]) - e_want[c]) / float(e_tol[c]))
        worst[3] = max(worst[3], float(((dy - dy_want).abs() / dy_tol.clamp(min=1e-300)).max()))
        assert energies.tolist() == e_bits, (energies.tolist(), e_bits)
        assert torch.equal(dy, dy_bits)
    print("worst error / bound: E_r %.3g, V_h %.3g, V_g %.3g, dy %.3g; cases %s" % (*worst, seen))
    assert all(v > 20 for v in seen.values()), seen
    assert max(worst) <= 1.0, worst


def test_selftest_refusals_in_the_order_of_the_entry():
    y = torch.linspace(-1.0, 1.0, 10, dtype=F64)
    z, k = torch.zeros(10, dtype=F64), torch.ones(10, dtype=F64)
    centers, heights, sigma = torch.zeros((3, 2), dtype=F64), torch.ones(3, dtype=F64), torch.ones(2, dtype=F64)
    table = torch.zeros((4, 5), dtype=F64)
    hills = lambda cols, c=centers, s=sigma: (cols, c, heights, s, None)       # noqa: E731
    grid = lambda cols, t=table, lower=(0.0, 0.0), spacing=(1.0, 1.0): (cols, t, list(lower)[:t.dim()], list(spacing)[:t.dim()], None)   # noqa: E731
    wide = lambda n: torch.zeros((3, n), dtype=F64)        # noqa: E731
    assert selftest(y, (z, k, None, None), hills([7, 2]), grid([9, 0]))[0] == 0
    terms, _ = _capi.bias_terms_f64()
    out = torch.full((13,), 7.5, dtype=F64)
    assert _capi.lib().molann_selftest_bias_f64(hh._ptr(y), 10, ctypes.byref(terms), hh._ptr(out[:3]), hh._ptr(out[3:])) == _capi.E_DESC    # no term
    assert _capi.lib().molann_selftest_bias_f64(hh._ptr(y), 10, None, hh._ptr(out[:3]), hh._ptr(out[3:])) == _capi.E_NULL
    assert bool((out == 7.5).all())
    for bad, code in ((dict(hills=hills([2, 10])), _capi.E_INDEX), (dict(hills=hills([-1, 2])), _capi.E_INDEX), (dict(hills=hills([4, 4])), _capi.E_INDEX),
                      (dict(grid=grid([3, 3])), _capi.E_INDEX), (dict(grid=grid([0, 10])), _capi.E_INDEX),
                      (dict(hills=(list(range(9)), wide(9), heights, torch.ones(9, dtype=F64), None)), _capi.E_UNSUPPORTED),
                      (dict(hills=(None, wide(9), heights, torch.ones(9, dtype=F64), None)), _capi.E_UNSUPPORTED),
                      (dict(hills=(list(range(8)) + [8, 8], wide(10), heights, torch.ones(10, dtype=F64), None)), _capi.E_INDEX),   # INDEX before UNSUPPORTED
                      (dict(grid=(None, torch.zeros((4, 4, 4, 4), dtype=F64), [0.0] * 4, [1.0] * 4, None)), _capi.E_UNSUPPORTED),
                      (dict(grid=grid([0, 1], table, (0.0, 0.0), (1.0, 0.0))), _capi.E_DESC)):
        got, energies, dy = selftest(y, **bad)
        assert got == code, (bad, got, code)
        assert bool((energies == 7.5).all()) and bool((dy == 7.5).all())
    short = y[:2].contiguous()
    assert selftest(short, hills=(None, wide(3), heights, torch.ones(3, dtype=F64), None))[0] == _capi.E_INDEX      # d_out too small for 0..2
    assert selftest(short, grid=grid(None, torch.zeros((4, 4, 4), dtype=F64), (0.0,) * 3, (1.0,) * 3))[0] == _capi.E_INDEX


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_declared_exported_and_bound(name):
    header = open(os.path.join(ROOT, "include", "molann_hip.h")).read()
    assert name + "(" in header, name
    fn = getattr(_capi.lib(), name)
    assert fn.argtypes is not None and len(fn.argtypes) == {SYMBOLS[0]: 10, SYMBOLS[1]: 1, SYMBOLS[2]: 5}[name], name
    assert name in _capi.declared_symbols()


def test_null_plan_and_abi():
    L = _capi.lib()
    assert L.molann_plan_supports_value_and_bias_f64(None) == _capi.E_NULL
    terms, _ = _capi.bias_terms_f64()
    for n in (1, 0):
        assert L.molann_value_and_bias_f64(None, None, n, None, None, ctypes.byref(terms), None, None, None, None) == _capi.E_NULL
        assert L.molann_value_and_bias_f64(None, None, n, None, None, None, None, None, None, None) == _capi.E_NULL
    assert L.molann_abi_version() == 1
    # the struct's layout is the header's: 20 fields, pointers and 64-bit counts on 8-byte boundaries
    assert ctypes.sizeof(_capi.BiasTermsF64) == 20 * 8 and _capi.BiasTermsF64.n_grid_columns.offset == 13 * 8


def test_methods_exist_and_say_what_is_out_of_scope():
    assert callable(_capi.Plan.supports_value_and_bias_f64) and callable(_capi.Plan.value_and_bias_f64)
    for method in (MolANN.value_and_bias, PreprocessingANN.value_and_bias):
        doc = " ".join(method.__doc__.split())
        for words in ("ONE kernel launch", "No autograd graph is recorded", "energies"):
            assert words in doc, (words, doc)
    doc = " ".join(MolANN.value_and_bias.__doc__.split())
    for words in ("float32", "more than one term of a kind", "GraphedForces", "gradients with respect to parameters or bias tables"):
        assert words in doc, (words, doc)
    # the single entries name the call that answers what they leave out
    assert "value_and_bias" in MolANN.value_and_grid.__doc__ and "value_and_bias" in MolANN.value_and_hills.__doc__
    assert set(("Restraint", "Hills", "Grid")) <= set(bias.__all__)


def test_records_are_immutable_and_check_their_columns():
    t = torch.zeros((4, 4), dtype=F64)
    h = Hills(torch.zeros((2, 2)), 1.0, 0.5, columns=[3, 1])
    g = Grid(t, [0.0, 0.0], [1.0, 1.0], columns=(6, 1))
    r = Restraint(0.0, 2.0)
    assert h.columns == (3, 1) and g.columns == (6, 1) and g.periodic is None and h.period is None and r.period is None and r.flat is None
    assert Hills(t, 1.0, 0.5).columns is None and Grid(t, [0.0] * 2, [1.0] * 2, columns=range(2)).columns == (0, 1)
    for rec in (h, g, r):
        with pytest.raises(AttributeError):
            rec.columns = (0,)
    for bad in ("01", 3, {0, 1}, torch.tensor([0, 1]), [0.0, 1.0], [True, False], [0, "1"]):
        with pytest.raises(TypeError, match="columns"):
            Hills(t, 1.0, 0.5, columns=bad)
        with pytest.raises(TypeError, match="columns"):
            Grid(t, [0.0] * 2, [1.0] * 2, columns=bad)
    for bad in ([0, 0], [2, 1, 2], [-1, 0]):
        with pytest.raises(IndexError, match="columns"):
            Hills(t, 1.0, 0.5, columns=bad)
        with pytest.raises(IndexError, match="columns"):
            Grid(t, [0.0] * 2, [1.0] * 2, columns=bad)
    with pytest.raises(NotImplementedError, match=r"at most 8 columns \(got 9\).*value_and_vjp"):
        Hills(t, 1.0, 0.5, columns=list(range(9)))
    with pytest.raises(NotImplementedError, match=r"at most 3 columns \(got 4\).*value_and_vjp"):
        Grid(t, [0.0] * 4, [1.0] * 4, columns=[0, 1, 2, 3])


def test_cpu_tensor_names_the_route_and_the_terms_are_checked_before_the_gate():
    w = wl.get_workload("C3")
    model = wl.build_model(w, torch.device("cpu"), 0).double().requires_grad_(False)
    x = w.make_frames(3, seed=1).double()
    d = w.out_dim()
    r = Restraint(torch.zeros(d, dtype=F64), 2.0)
    g = Grid(torch.zeros((5, 6), dtype=F64), [0.0, 0.0], [1.0, 1.0], columns=[6, 1])
    with pytest.raises(NotImplementedError, match=r"form the terms and their derivatives on the chosen columns with torch, then `value_and_vjp`"):
        model.value_and_bias(x, restraint=r, grid=g)
    with pytest.raises(NotImplementedError, match=r"form the terms with torch and take torch\.autograd\.grad"):
        model.preprocessing_layer.value_and_bias(x, restraint=Restraint(torch.zeros(w.feature_dim(), dtype=F64), 2.0))
    with pytest.raises(NotImplementedError):                 # the gate comes before `into` and before the terms' own arguments
        model.value_and_bias(x, restraint=Restraint(torch.zeros(d - 1, dtype=F64), 2.0), grid=Grid(None, [0.0], [1.0], columns=[70]), into=(x,))
    for target in (model, model.preprocessing_layer):
        with pytest.raises(ValueError, match="at least one of `restraint`, `hills` and `grid`"):         # what needs no device comes first
            target.value_and_bias(x)
        for bad in (dict(restraint=(r.center, 2.0)), dict(hills=g), dict(grid=r), dict(grid=(g.table, [0.0] * 2, [1.0] * 2))):
            with pytest.raises(TypeError, match="molann_amd.bias"):
                target.value_and_bias(x, **bad)


def test_arguments_are_checked_before_any_device_call():
    """ann._check_bias_args is what both methods call before the plan is looked up: the columns against the model, then every term by
    its single call's check with the term's width, then `into`."""
    n, n_inp, d = 5, 22, 12
    x = torch.zeros((n, n_inp, 3), dtype=F64)
    y, energies, dx = torch.zeros((n, d), dtype=F64), torch.zeros((n, 3), dtype=F64), torch.zeros_like(x)
    z, k = torch.zeros(d, dtype=F64), torch.ones(d, dtype=F64)
    centers, heights, sigma = torch.zeros((4, 3), dtype=F64), torch.ones(4, dtype=F64), torch.full((3,), 0.5, dtype=F64)
    table = torch.zeros((5, 6), dtype=F64)
    R, H, G = Restraint(z, k), Hills(centers, heights, sigma, columns=[11, 0, 4]), Grid(table, [0.0, 0.0], [1.0, 1.0], [True, False], columns=[9, 11])

    def check(restraint=R, hills=H, grid=G, into=None, d_out=d):
        return ann._check_bias_args("value_and_bias", x, d_out, restraint, hills, grid, into)

    r, h, g, *into = check(into=(y, energies, dx))
    assert r[0].data_ptr() == z.data_ptr() and r[1].data_ptr() == k.data_ptr() and r[2:] == (None, None)
    assert h[0] == (11, 0, 4) and h[1].data_ptr() == centers.data_ptr() and h[3].data_ptr() == sigma.data_ptr() and h[4] is None
    assert g[0] == (9, 11) and g[1].data_ptr() == table.data_ptr() and g[2:] == ([0.0, 0.0], [1.0, 1.0], [True, False])
    assert into[0] is y and into[1] is energies and into[2] is dx
    r, h, g, *into = check(restraint=None, hills=Hills(centers.tolist(), 0.7, 0.4), grid=Grid(table, [0.0] * 2, [1.0] * 2))
    assert r is None and h[0] == (0, 1, 2) and g[0] == (0, 1) and into == [None, None, None]
    assert torch.equal(h[2], torch.full((4,), 0.7, dtype=F64)) and torch.equal(h[3], torch.full((3,), 0.4, dtype=F64))      # the conversions
    assert check(hills=None, grid=None)[1:3] == (None, None)
    with pytest.raises(IndexError, match=r"hills.columns.*\[0, 12\)"):
        check(hills=Hills(centers, heights, sigma, columns=[0, 12, 4]))
    with pytest.raises(IndexError, match=r"grid.columns.*\[0, 5\)"):
        check(restraint=None, hills=None, d_out=5)
    with pytest.raises(IndexError, match="3 columns but the model has 2 outputs"):
        check(restraint=None, hills=Hills(centers, heights, sigma), grid=None, d_out=2)
    with pytest.raises(NotImplementedError, match="at most 8 hills columns"):
        check(hills=Hills(torch.zeros((4, 9), dtype=F64), heights, 0.5))
    with pytest.raises(NotImplementedError, match="at most 8 hills columns"):          # the cap, then the model: the C entry's order
        check(restraint=None, hills=Hills(torch.zeros((4, 9), dtype=F64), heights, 0.5), grid=None, d_out=8)
    with pytest.raises(ValueError, match=r"pass `columns` or a \[0, columns\] tensor"):     # no hills yet, as a list: the width is not told
        check(hills=Hills([], [], 0.5))
    assert check(hills=Hills([], [], 0.5, columns=[11, 0]))[1][1].shape == (0, 2)
    assert check(hills=Hills(torch.zeros((0, 3), dtype=F64), torch.zeros(0, dtype=F64), 0.5))[1][0] == (0, 1, 2)
    with pytest.raises(NotImplementedError, match="at most 3 grid columns"):
        check(grid=Grid(torch.zeros((4, 4, 4, 4), dtype=F64), [0.0] * 4, [1.0] * 4))
    # the terms' own checks, with the term's width in place of the number of outputs
    with pytest.raises(ValueError, match="center"):
        check(restraint=Restraint(z[:3], k))
    with pytest.raises(ValueError, match=r"centers.*\[4, 3\]"):
        check(hills=Hills(torch.zeros((4, 12), dtype=F64), heights, 0.5, columns=[11, 0, 4]))
    with pytest.raises(ValueError, match="sigma"):
        check(hills=Hills(centers, heights, sigma * 0.0, columns=[11, 0, 4]))
    with pytest.raises(ValueError, match="flat"):
        check(restraint=Restraint(z, k, flat=-k))
    with pytest.raises(ValueError, match=r"table.*per grid column \(2\)"):
        check(grid=Grid(torch.zeros((5, 6, 4), dtype=F64), [0.0] * 2, [1.0] * 2, columns=[9, 11]))
    with pytest.raises(ValueError, match="spacing"):
        check(grid=Grid(table, [0.0] * 2, [1.0, 0.0], columns=[9, 11]))
    with pytest.raises(ValueError, match=r"`lower` must hold one value per grid column \(2\); got 3"):    # the term's columns, not the model's outputs
        check(grid=Grid(table, [0.0] * 3, [1.0] * 2, columns=[9, 11]))
    with pytest.raises(TypeError, match="table"):
        check(grid=Grid(table.float(), [0.0] * 2, [1.0] * 2, columns=[9, 11]))
    # `into`: a triple with energies [N, 3]
    with pytest.raises(TypeError, match=r"triple of tensors \(y, energies, dx\)"):
        check(into=(y, dx))
    with pytest.raises(TypeError, match="float64"):
        check(into=(y, energies.float(), dx))
    for bad in ((y, energies[:, 0].contiguous(), dx), (y[:, :3].contiguous(), energies, dx), (y, energies, dx[1:]), (y, energies.t(), dx),
                (y, energies.to("meta"), dx)):
        with pytest.raises(ValueError, match=r"\[5, 12\], \[5, 3\]"):
            check(into=bad)
