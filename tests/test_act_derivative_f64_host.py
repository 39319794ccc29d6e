"""act_derivative_f64 (molann_math.h: the derivative the float64 head's backward multiplies by, computed from the pre-activation)
against torch's float64 autograd of the matching torch.nn.functional, through the host build of the same function; and the new
float64 entry points in the header and the library.  No GPU."""

import ctypes

import pytest
import torch

from molann_amd import _capi

F = torch.nn.functional
ACTS = {
    _capi.ACT_TANH: torch.tanh, _capi.ACT_RELU: F.relu, _capi.ACT_SIGMOID: torch.sigmoid, _capi.ACT_IDENTITY: lambda z: z,
    _capi.ACT_ELU: F.elu, _capi.ACT_SILU: F.silu, _capi.ACT_SOFTPLUS: F.softplus, _capi.ACT_LEAKY_RELU: F.leaky_relu,
    _capi.ACT_GELU: F.gelu,
}
KINKED = (_capi.ACT_RELU, _capi.ACT_LEAKY_RELU)


@pytest.mark.parametrize("code", sorted(ACTS))
def test_act_derivative_f64_matches_torch_autograd(code):
    """atol 1e-13, rtol 1e-12: the double rounding of a few elementary functions."""
    fn = _capi.lib().molann_selftest_act_derivative_f64
    z = torch.linspace(-25, 25, 401, dtype=torch.float64)
    if code in KINKED:
        z = z[z.abs() >= 1e-3]
    if code == _capi.ACT_SOFTPLUS:
        z = torch.cat([z, torch.tensor([20.0 - 1e-6, 20.0 + 1e-6], dtype=torch.float64)])
    zg = z.clone().requires_grad_(True)
    (want,) = torch.autograd.grad(ACTS[code](zg).sum(), zg)
    got = torch.tensor([fn(code, float(v)) for v in z.tolist()], dtype=torch.float64)
    err = (got - want).abs()
    bound = 1e-13 + 1e-12 * want.abs()
    worst = int(torch.argmax(err - bound))
    print("act %d: max |err| %.3e at z = %g" % (code, float(err.max()), float(z[worst])))
    assert bool((err <= bound).all()), (code, float(z[worst]), float(got[worst]), float(want[worst]))


def test_new_symbols_are_declared_and_exported():
    declared = _capi.declared_symbols()
    L = ctypes.CDLL(_capi.LIB_PATH)
    for name in ("molann_value_and_vjp_f64", "molann_plan_supports_value_and_vjp_f64", "molann_selftest_act_derivative_f64"):
        assert name in declared, name
        assert hasattr(L, name), name
    assert L.molann_plan_supports_value_and_vjp_f64(None) == _capi.E_NULL
    assert L.molann_value_and_vjp_f64(None, None, None, 0, None, None, None, None, None) == _capi.E_NULL
