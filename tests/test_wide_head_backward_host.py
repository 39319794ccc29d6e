"""The backward of wide fp32 heads (csrc/molann_chain_bwd.inc): source generation and hipRTC compilation need no GPU."""

import ctypes

import pytest

from molann_amd import _capi, workloads as wl

CHAIN_BWD = 256 | 1      # molann_debug_jit: generate and compile molann_chain_bwd

# (dims, activation code): tanh 0, ReLU 1, sigmoid 2, identity 3, SiLU 5, LeakyReLU 7
HEADS = [([6, 64, 64, 8], 0), ([6, 48, 33, 5], 2), ([66, 5, 3], 0), ([126, 64, 32, 2], 5), ([85, 128, 64, 8], 0),
         ([6, 128, 128, 8], 1), ([6, 100, 70, 3], 7), ([6, 40], 3), ([85, 40], 0)]


def _run(dims, act, mode=CHAIN_BWD, precision=_capi.MLP_F32):
    d, keep = _capi.workload_desc(wl.get_workload("C3"))
    ld = (ctypes.c_int32 * len(dims))(*dims)
    d.n_layers, d.layer_dims, d.activation, d.mlp_precision = len(dims) - 1, ld, act, precision
    buf = ctypes.create_string_buffer(1 << 22)
    rc = _capi.lib().molann_debug_jit(ctypes.byref(d), mode, buf, 1 << 22)
    return rc, buf.value.decode()


@pytest.mark.parametrize("dims,act", HEADS)
def test_chain_backward_compiles(dims, act):
    """Host geometry (LDS layout, waves per block, gradient-buffer offsets) against the kernel's own static_asserts: the
    specialised source cross-compiles for gfx950 for every head the GPU tests train."""
    rc, src = _run(dims, act)
    assert rc > 1000, (rc, src[:3000])
    rc, src = _run(dims, act, mode=256)
    assert "molann_chain_bwd" in src
    assert "constexpr int DIMS[] = {%s};" % ", ".join(str(v) for v in dims) in src
    n_params = sum(dims[l + 1] * dims[l] + dims[l + 1] for l in range(len(dims) - 1))
    assert "constexpr int N_PARAMS = %d;" % n_params in src


def test_chain_backward_waves_fit_the_lds():
    """The widest heads still fit a 64-frame tile beside their weights; the C4 head's source names four waves."""
    for dims, act in [([85, 128, 64, 8], 0), ([6, 128, 128, 8], 1)]:
        rc, src = _run(dims, act, mode=256)
        assert rc > 1000
        assert "constexpr int WAVES = 4;" in src


@pytest.mark.parametrize("dims,act,precision", [([6, 64, 64, 8], 4, _capi.MLP_F32), ([6, 64, 64, 8], 8, _capi.MLP_F32),
                                                ([6, 64, 64, 8], 6, _capi.MLP_F32), ([6, 64, 64, 8], 0, _capi.MLP_BF16),
                                                ([341, 512, 256, 16], 0, _capi.MLP_F32)])
def test_chain_backward_refuses_what_it_does_not_serve(dims, act, precision):
    """ELU, GELU, Softplus, bf16 heads and streaming heads (C5) are not built."""
    rc, _ = _run(dims, act, mode=256, precision=precision)
    assert rc == _capi.E_UNSUPPORTED


def test_supports_mlp_backward_is_bound():
    assert hasattr(_capi.Plan, "supports_mlp_backward")
    assert _capi.lib().molann_plan_supports_mlp_backward(None) == _capi.E_NULL
