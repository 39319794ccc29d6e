"""Values + vector-Jacobian product of mid-size and large frames in one launch (csrc/molann_group_vjp.inc): source generation
and hipRTC compilation need no GPU."""

import ctypes

import pytest

from molann_amd import _capi, workloads as wl

GROUP_VJP = 512 | 1      # molann_debug_jit: generate and compile molann_group_vjp


def _desc(name, dims=None, act=None, precision=None, align=True, n_inp=None):
    d, keep = _capi.workload_desc(wl.get_workload(name))
    if n_inp is not None:
        d.n_inp = n_inp
    if dims is not None:
        ld = (ctypes.c_int32 * len(dims))(*dims)
        keep.append(ld)
        d.n_layers, d.layer_dims = len(dims) - 1, ld
    if act is not None:
        d.activation = act
    if precision is not None:
        d.mlp_precision = precision
    if not align:
        d.n_align = 0
    return d, keep


def _run(d, mode=GROUP_VJP):
    buf = ctypes.create_string_buffer(1 << 23)
    rc = _capi.lib().molann_debug_jit(ctypes.byref(d), mode, buf, 1 << 23)
    return rc, buf.value.decode()


# (workload, head dims or None for the workload's own, activation, with alignment, expected B)
PLANS = [("P1", None, None, True, 8),                    # 166 atoms, Kabsch on 42, 8 dihedrals, [16, 32, 8] tanh
         ("P1", None, None, False, 8),                   # the same without an alignment
         ("P1", [16, 32, 32, 32, 4], 5, True, 8),        # four layers of SiLU: the weight fragments in the LDS image
         ("P1@5000", None, None, True, 8),               # P1's items and alignment in a 5000-atom frame
         ("P2", [126, 0], None, True, 4)]                # features only (42 position items: B = 4), no head


@pytest.mark.parametrize("name,dims,act,align,b", PLANS)
def test_group_vjp_compiles(name, dims, act, align, b):
    """Host geometry (LDS layout, frames per round) against the kernel's own static_asserts: the specialised source
    cross-compiles for gfx950."""
    n_inp = None
    if "@" in name:
        name, n_inp = name.split("@")[0], int(name.split("@")[1])
    if dims == [126, 0]:
        d, keep = _desc(name, align=align)
        d.n_layers = 0
    else:
        d, keep = _desc(name, dims=dims, act=act, align=align, n_inp=n_inp)
    rc, src = _run(d)
    assert rc > 1000, (rc, src[:3000])
    rc, src = _run(d, mode=512)
    assert "molann_group_vjp" in src
    assert "constexpr int B = %d;" % b in src
    assert "constexpr bool WITH_VALUES = true;" in src
    if dims == [126, 0]:
        assert "constexpr int NL = 0;" in src and "constexpr int D_FEAT = 126;" in src
    else:
        want = dims if dims is not None else wl.get_workload(name).mlp_dims
        assert "constexpr int DIMS[] = {%s};" % ", ".join(str(v) for v in want) in src
    assert ("constexpr int N_ALIGN = 0;" in src) == (not align)
    assert "constexpr int FRAME_DW = %d;" % (3 * (n_inp or wl.get_workload(name).n_atoms)) in src


def test_group_vjp_frames_per_round_follow_the_items():
    """B = 8 up to 32 items per frame, 4 up to 64, 2 beyond (at least two frames per round): features-only plans of n bonds
    on the 5000-atom chain with its 312-atom alignment."""
    w = wl.get_workload("C4")
    for n_items, b in ((32, 8), (33, 4), (64, 4), (65, 2), (300, 2)):
        d, keep = _desc("C4")
        d.n_layers = 0
        idx = list(range(n_items + 1))
        ft = (ctypes.c_int32 * n_items)(*([wl.BOND] * n_items))
        fp = (ctypes.c_int32 * (n_items + 1))(*[2 * i for i in range(n_items + 1)])
        fi = (ctypes.c_int32 * (2 * n_items))(*[a for i in range(n_items) for a in (idx[i], idx[i + 1])])
        keep += [ft, fp, fi]
        d.n_features, d.feat_type, d.feat_ptr, d.feat_idx = n_items, ft, fp, fi
        rc, src = _run(d, mode=512)
        assert rc > 1000, (n_items, rc, src[:2000])
        assert "constexpr int B = %d;" % b in src, (n_items, w.name)
        assert "constexpr int N_ITEMS = %d;" % n_items in src


@pytest.mark.parametrize("dims,act,precision", [([126, 64, 32, 2], 0, _capi.MLP_F32),     # wide head
                                                ([16, 32, 8], 4, _capi.MLP_F32),          # ELU
                                                ([16, 32, 8], 6, _capi.MLP_F32),          # GELU
                                                ([16, 32, 8], 8, _capi.MLP_F32),          # Softplus
                                                ([16, 32, 8], 0, _capi.MLP_BF16),         # bf16
                                                ([16, 32, 32, 32, 32, 8], 0, _capi.MLP_F32)])  # five layers
def test_group_vjp_refuses_what_it_does_not_serve(dims, act, precision):
    d, keep = _desc("P2" if dims[0] == 126 else "P1", dims=dims, act=act, precision=precision)
    rc, _ = _run(d)
    assert rc == _capi.E_UNSUPPORTED


def test_supports_value_and_vjp_is_bound():
    assert hasattr(_capi.Plan, "supports_value_and_vjp")
    assert _capi.lib().molann_plan_supports_value_and_vjp(None) == _capi.E_NULL
