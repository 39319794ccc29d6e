"""The harmonic restraint of the float64 one-launch family on the host (no GPU): the term the kernel applies to one output
(molann_selftest_restraint_f64 calls the kernel's own __host__ __device__ function) against the formula written in torch float64, the
refusals of MolANN.value_and_restraint / PreprocessingANN.value_and_restraint that need no device, the argument checks both share
(run before anything touches a device) and the C entry's symbols and its answer to a null plan."""

import ctypes
import math
import os

import numpy as np
import pytest
import torch

from molann_amd import _capi, ann, workloads as wl
from molann_amd.ann import MolANN, PreprocessingANN

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["molann_value_and_restraint_f64", "molann_plan_supports_value_and_restraint_f64", "molann_selftest_restraint_f64"]
NAN = float("nan")


def formula(y, z, kappa, period, flat):
    """(energy term, dy, d) of the issue's formula, elementwise in torch float64: d = y - z; wrapped by d - P round(d / P) where P > 0
    (torch.round: ties to even); where h > 0, copysign(|d| - h, d) beyond the flat bottom and 0 inside it, a NaN left as it is."""
    d = y - z
    periodic = period > 0
    P = torch.where(periodic, period, torch.ones_like(period))
    d = torch.where(periodic, d - P * torch.round(d / P), d)
    a = d.abs() - flat
    cut = torch.where(a > 0, torch.copysign(a, d), torch.where(a <= 0, torch.zeros_like(d), d))
    d = torch.where(flat > 0, cut, d)
    return 0.5 * kappa * d * d, kappa * d, d


def selftest(y, z, kappa, period, flat):
    fn = _capi.lib().molann_selftest_restraint_f64
    e, dy = np.empty(len(y)), np.empty(len(y))
    cot = ctypes.c_double()
    for i, args in enumerate(zip(y.tolist(), z.tolist(), kappa.tolist(), period.tolist(), flat.tolist())):
        e[i] = fn(*args, ctypes.byref(cot))
        dy[i] = cot.value
    return torch.from_numpy(e), torch.from_numpy(dy)


def _inputs():
    """4096 seeded (y, z, kappa, P, h) - a third of them periodic, a third with a flat bottom, independently - and the edge cases."""
    g = torch.Generator().manual_seed(20)
    n = 4096
    y = 8.0 * torch.randn(n, generator=g, dtype=torch.float64)
    z = 8.0 * torch.randn(n, generator=g, dtype=torch.float64)
    kappa = 50.0 * torch.randn(n, generator=g, dtype=torch.float64)
    pick = torch.randint(0, 3, (2, n), generator=g)
    period = torch.where(pick[0] == 0, torch.rand(n, generator=g, dtype=torch.float64) * 6.0 + 0.5, torch.zeros(n, dtype=torch.float64))
    period[::7] = 2.0 * math.pi * (pick[0][::7] == 0)
    period[5::11] = -1.0                                    # P <= 0: not periodic
    flat = torch.where(pick[1] == 0, torch.rand(n, generator=g, dtype=torch.float64) * 2.0, torch.zeros(n, dtype=torch.float64))
    edge = [  # y, z, kappa, P, h
        (1.0, 0.0, 3.0, 2.0, 0.0), (-1.0, 0.0, 3.0, 2.0, 0.0), (3.0, 0.0, 3.0, 2.0, 0.0), (-3.0, 0.0, 3.0, 2.0, 0.0),     # d / P = +-0.5, +-1.5
        (1.5, 0.5, 3.0, 2.0, 0.25), (-0.5, 0.5, 3.0, 2.0, 0.25),
        (1.75, 0.5, 2.0, 0.0, 1.25), (-0.75, 0.5, 2.0, 0.0, 1.25), (1.0, 0.0, 2.0, 2.0, 1.0),                                # |d| == h
        (0.3, 0.1, 7.0, 0.0, 0.0), (0.3, 0.1, 7.0, 0.0, 0.5), (0.3, 0.1, 7.0, 3.0, 0.0),                                    # h = 0, P = 0
        (2.0, -1.0, -4.0, 0.0, 0.0), (2.0, -1.0, -4.0, 5.0, 0.5), (2.0, -1.0, 0.0, 0.0, 0.0),                               # kappa < 0, = 0
        (NAN, 0.5, 2.0, 0.0, 0.0), (NAN, 0.5, 2.0, 0.0, 0.7), (NAN, 0.5, 2.0, 2.0, 0.0), (NAN, 0.5, 2.0, 2.0, 0.7),         # y = NaN
        (0.5, NAN, 2.0, 0.0, 0.7),
        (-0.0, 0.0, 3.0, 0.0, 0.0), (-0.0, 0.0, 3.0, 2.0, 0.0), (-0.0, 0.0, 3.0, 0.0, 0.5), (-0.0, 0.0, -3.0, 2.0, 0.5),   # d = -0.0
    ]
    e = torch.tensor(edge, dtype=torch.float64)
    return tuple(torch.cat([a, e[:, i]]) for i, a in enumerate((y, z, kappa, period, flat))), len(edge)


def test_selftest_against_the_formula():
    (y, z, kappa, period, flat), n_edge = _inputs()
    e, dy = selftest(y, z, kappa, period, flat)
    e_want, dy_want, d = formula(y, z, kappa, period, flat)
    nan = torch.isnan(dy_want)
    assert int(nan.sum()) == 5 and torch.equal(torch.isnan(dy), nan) and torch.equal(torch.isnan(e), nan)
    ok = ~nan
    scale = torch.maximum(d.abs(), z.abs())[ok] * kappa.abs()[ok]
    dy_tol = 4.0 * torch.from_numpy(np.spacing(scale.numpy()))
    e_tol = 4.0 * torch.from_numpy(np.spacing((0.5 * scale * torch.maximum(d.abs(), z.abs())[ok]).numpy()))
    dy_err, e_err = (dy - dy_want)[ok].abs(), (e - e_want)[ok].abs()
    print("dy: worst err / tol %.3g, energy: %.3g" % (float((dy_err / dy_tol).max()), float((e_err / e_tol).max())))
    assert bool((dy_err <= dy_tol).all()) and bool((e_err <= e_tol).all())
    # the edge cases, by value: ties to even, the kink, the signs
    got = dy[-n_edge:].tolist()
    assert got[0:4] == [3.0, -3.0, -3.0, 3.0], got[0:4]           # rint(+-0.5) = 0, rint(+-1.5) = +-2
    assert got[4:6] == [2.25, -2.25], got[4:6]                     # d = +-1 (a tie), 0.25 of it flat
    assert got[6:9] == [0.0, 0.0, 0.0], got[6:9]                   # |d| == h: the wall starts there
    assert got[12] == -12.0 and got[14] == 0.0
    assert all(v == 0.0 for v in got[-4:]), got[-4:]
    assert (e[-n_edge:][ok[-n_edge:]] * kappa[-n_edge:][ok[-n_edge:]] >= 0).all()   # the energy has kappa's sign


def test_without_period_and_flat_dy_is_the_rounded_product_bit_for_bit():
    (y, z, kappa, period, flat), _ = _inputs()
    plain = ~torch.isnan(y) & ~torch.isnan(z)
    y, z, kappa = y[plain], z[plain], kappa[plain]
    zero = torch.zeros_like(y)
    for period in (zero, zero - 1.0):
        _, dy = selftest(y, z, kappa, period, zero)
        assert torch.equal(dy, kappa * (y - z))
    assert _capi.lib().molann_selftest_restraint_f64(1.0, 0.25, 2.0, 0.0, 0.0, None) == 0.5 * 2.0 * 0.75 * 0.75     # dy may be null


@pytest.mark.parametrize("name", SYMBOLS)
def test_symbol_declared_exported_and_bound(name):
    header = open(os.path.join(ROOT, "include", "molann_hip.h")).read()
    assert name + "(" in header, name
    fn = getattr(_capi.lib(), name)
    assert fn.argtypes is not None and len(fn.argtypes) == {SYMBOLS[0]: 14, SYMBOLS[1]: 1, SYMBOLS[2]: 6}[name], name
    assert name in _capi.declared_symbols()


def test_null_plan():
    L = _capi.lib()
    assert L.molann_plan_supports_value_and_restraint_f64(None) == _capi.E_NULL
    for n in (1, 0):
        assert L.molann_value_and_restraint_f64(None, None, n, None, None, None, 0, None, None, None, None, None, None, None) == _capi.E_NULL
    assert _capi.lib().molann_abi_version() == 1


def test_methods_exist_and_say_what_is_out_of_scope():
    assert callable(_capi.Plan.supports_value_and_restraint_f64) and callable(_capi.Plan.value_and_restraint_f64)
    for method in (MolANN.value_and_restraint, PreprocessingANN.value_and_restraint):
        doc = " ".join(method.__doc__.split())
        for words in ("costs a launch", "float32", "GraphedForces", "No autograd graph is recorded"):
            assert words in doc, (words, doc)


def test_cpu_tensor_names_the_route_that_remains():
    w = wl.get_workload("C3")
    model = wl.build_model(w, torch.device("cpu"), 0).double().requires_grad_(False)
    x = w.make_frames(3, seed=1).double()
    center, kappa = torch.zeros(w.out_dim(), dtype=torch.float64), 2.0
    with pytest.raises(NotImplementedError, match=r"use `model\(x\)`, form `kappa \* d` and the energy with torch, then `value_and_vjp`"):
        model.value_and_restraint(x, center, kappa)
    with pytest.raises(NotImplementedError, match=r"form the energy with torch and take torch\.autograd\.grad"):
        model.preprocessing_layer.value_and_restraint(x, torch.zeros(w.feature_dim(), dtype=torch.float64), kappa)
    with pytest.raises(NotImplementedError):                            # the gate comes before `into` and before the other arguments
        model.value_and_restraint(x, center[:-1], kappa, flat=-center, into=(center, center))
    with pytest.raises(NotImplementedError):
        model.preprocessing_layer.value_and_restraint(x, center, kappa, into=(center,))


def test_arguments_are_checked_before_any_device_call():
    """ann._check_restraint_args is what both methods call before the plan is looked up; tensors on the meta device stand for 'another
    device' here."""
    n, n_inp, d = 5, 22, 8
    x = torch.zeros((n, n_inp, 3), dtype=torch.float64)
    y, energy, dx = torch.zeros((n, d), dtype=torch.float64), torch.zeros(n, dtype=torch.float64), torch.zeros_like(x)
    z, k = torch.linspace(-1.0, 1.0, d, dtype=torch.float64), torch.linspace(0.5, 2.0, d, dtype=torch.float64)

    def check(center=z, kappa=k, period=None, flat=None, into=None):
        return ann._check_restraint_args("value_and_restraint", x, d, center, kappa, period, flat, into)

    got = check()
    assert got[0] is not None and got[0].data_ptr() == z.data_ptr() and got[1].data_ptr() == k.data_ptr()       # float64: as they are
    assert got[2:] == (None, None, None, None, None)
    got = check(z.expand(n, d), 3.0, period=[0.0] * d, flat=k.float(), into=(y, energy, dx))
    assert got[0].shape == (n, d) and got[0].is_contiguous() and torch.equal(got[1], torch.full((d,), 3.0, dtype=torch.float64))
    assert got[2].dtype == torch.float64 and torch.equal(got[3], k.float().double()) and got[4] is y and got[5] is energy and got[6] is dx
    assert check(into=[y.reshape(-1), energy, dx.reshape(-1)])[6].dim() == 1            # the element count is what counts
    for bad in (z[:-1], z.reshape(1, d), z.expand(n + 1, d), z.expand(n, d).reshape(-1), torch.zeros(())):
        with pytest.raises(ValueError, match="center"):
            check(center=bad)
    for what in ("kappa", "period", "flat"):
        for bad in (k[:-1], k.expand(n, d), k.reshape(d, 1), k.to("meta")):
            with pytest.raises(ValueError, match=what):
                check(**{what: bad})
        with pytest.raises(TypeError, match=what):
            check(**{what: k.to(torch.int64)})
        with pytest.raises(TypeError, match=what):
            check(**{what: "stiff"})
    with pytest.raises(ValueError, match="center"):
        check(center=z.to("meta"))
    for bad in (-k, [0.0] * (d - 1) + [-1e-300], torch.where(k > 1.0, -k, k).float()):
        with pytest.raises(ValueError, match="flat"):
            check(flat=bad)
    assert check(flat=torch.zeros(d, dtype=torch.float64))[3] is not None               # zeros: no flat bottom, not an error
    for bad in ((y, dx), (y, energy, dx, dx), (y, energy, None), [y.numpy(), energy, dx]):
        with pytest.raises(TypeError, match=r"triple of tensors \(y, energy, dx\)"):
            check(into=bad)
    for bad in ((y.float(), energy, dx), (y, energy.float(), dx), (y, energy, dx.float())):
        with pytest.raises(TypeError, match="float64"):
            check(into=bad)
    for bad in ((y[:4], energy, dx), (y, energy[:4], dx), (y, energy, dx[:, :-1]), (y.t(), energy, dx), (y, torch.zeros(2 * n, dtype=torch.float64)[::2], dx),
                (y.to("meta"), energy, dx), (y, energy.to("meta"), dx), (y, energy, dx.to("meta"))):
        with pytest.raises(ValueError, match="into"):
            check(into=bad)
    with pytest.raises(ValueError, match="flat"):                                       # `flat` is looked at before `into`
        check(flat=-k, into=(y.to("meta"), energy, dx))
