"""ctypes binding of ``libmolann_hip.so`` (the C ABI declared in ``include/molann_hip.h``).

Nothing here computes anything: it marshals index lists into a ``molann_plan_desc``, keeps the opaque
plan alive, and passes raw device pointers + the current HIP stream to the launch functions.  If the
library is missing the import of this module fails loudly; there is no CPU fallback.
"""

import ctypes
import os
import re
import subprocess

import torch  # imported first so that libamdhip64.so.7 is torch's copy (same SONAME, loaded once)

_HERE = os.path.dirname(os.path.abspath(__file__))
_CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.path.join(_CSRC, "libmolann_hip.so")
# the diagnostics build (honours MOLANN_DEBUG_* / MOLANN_ELIDE_INVARIANT_ALIGNMENT): tools/ only, opt-in by name
DIAG_LIB_PATH = os.path.join(_CSRC, "libmolann_hip_diag.so")
SAN_LIB_PATH = os.path.join(_CSRC, "libmolann_hip_san.so")   # `make san`: host code under ASan + UBSan (CPU tests only)
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "molann_hip.h")

ABI_VERSION = 1
FEAT_ANGLE, FEAT_BOND, FEAT_DIHEDRAL, FEAT_POSITION = 0, 1, 2, 3
ACT_TANH, ACT_RELU, ACT_SIGMOID, ACT_IDENTITY, ACT_ELU, ACT_SILU, ACT_SOFTPLUS, ACT_LEAKY_RELU, ACT_GELU = range(9)
MLP_F32, MLP_BF16 = 0, 1
MAX_LAYERS = 16

E_NULL, E_DESC, E_INDEX, E_FEATURE, E_STAGE, E_ALIGNMENT, E_UNSUPPORTED, E_NOT_PACKED, E_DEVICE = range(-1, -10, -1)


class MolannHipError(RuntimeError):
    def __init__(self, code, what):
        self.code = code
        super(MolannHipError, self).__init__("%s failed: [%d] %s" % (what, code, error_string(code)))


class PlanDesc(ctypes.Structure):
    _fields_ = [
        ("abi_version", ctypes.c_int32), ("n_inp", ctypes.c_int32),
        ("n_align", ctypes.c_int32), ("align_idx", ctypes.POINTER(ctypes.c_int32)),
        ("ref_x", ctypes.POINTER(ctypes.c_float)),
        ("n_features", ctypes.c_int32), ("feat_type", ctypes.POINTER(ctypes.c_int32)),
        ("feat_ptr", ctypes.POINTER(ctypes.c_int32)), ("feat_idx", ctypes.POINTER(ctypes.c_int32)),
        ("use_angle_value", ctypes.c_int32),
        ("n_layers", ctypes.c_int32), ("layer_dims", ctypes.POINTER(ctypes.c_int32)),
        ("activation", ctypes.c_int32), ("mlp_precision", ctypes.c_int32),
    ]


def build_library(force=False):
    """Compile csrc/: libmolann_hip.so (hipcc, gfx950, seconds) and libmolann_torch.so (g++, the TorchScript
    operators over the same ABI).  make decides what is stale.  Used by __graft_entry__.build()."""
    if force:
        subprocess.check_call(["make", "-C", _CSRC, "clean"])
    subprocess.check_call(["make", "-C", _CSRC, "all"])
    return LIB_PATH


class BiasTermsF64(ctypes.Structure):
    """molann_bias_terms_f64 of include/molann_hip.h: the terms of `molann_value_and_bias_f64`."""
    _fields_ = [("center", ctypes.c_void_p), ("center_stride", ctypes.c_int64), ("kappa", ctypes.c_void_p),
                ("restraint_period", ctypes.c_void_p), ("flat", ctypes.c_void_p),
                ("n_hills_columns", ctypes.c_int32), ("hills_columns", ctypes.POINTER(ctypes.c_int32)),
                ("centers", ctypes.c_void_p), ("heights", ctypes.c_void_p), ("n_hills", ctypes.c_int64), ("sigma", ctypes.c_void_p),
                ("sigma_stride", ctypes.c_int64), ("hills_period", ctypes.c_void_p),
                ("n_grid_columns", ctypes.c_int32), ("grid_columns", ctypes.POINTER(ctypes.c_int32)),
                ("table", ctypes.c_void_p), ("shape", ctypes.POINTER(ctypes.c_int64)), ("lower", ctypes.POINTER(ctypes.c_double)),
                ("spacing", ctypes.POINTER(ctypes.c_double)), ("periodic", ctypes.POINTER(ctypes.c_int32))]


def bias_terms_f64(restraint=None, hills=None, grid=None, ptr=lambda t: t.data_ptr()):
    """A `BiasTermsF64` and the host arrays it points into (keep both alive for the call).  restraint: (center, kappa, period, flat,
    center_stride); hills: (columns, centers, heights, sigma, period, n_hills, sigma_stride); grid: (columns, table, shape, lower,
    spacing, periodic); None: the term is absent.  Tensors give their addresses through `ptr`; columns None is the identity list and
    needs the count in its place: (None, n)."""
    t, keep = BiasTermsF64(), []

    def address(v):
        return None if v is None else ptr(v)

    def host(ctype, values):
        if values is None:
            return None
        arr = (ctype * max(len(values), 1))(*values)
        keep.append(arr)
        return arr

    def columns(cols):
        if isinstance(cols, tuple) and len(cols) == 2 and cols[0] is None:
            return int(cols[1]), None
        cols = [int(c) for c in cols]
        return len(cols), host(ctypes.c_int32, cols)

    if restraint is not None:
        center, kappa, period, flat, stride = restraint
        t.center, t.center_stride, t.kappa, t.restraint_period, t.flat = address(center), stride, address(kappa), address(period), address(flat)
    if hills is not None:
        cols, centers, heights, sigma, period, n_hills, stride = hills
        t.n_hills_columns, arr = columns(cols)
        if arr is not None:
            t.hills_columns = arr
        t.centers, t.heights, t.n_hills, t.sigma, t.sigma_stride, t.hills_period = \
            address(centers), address(heights), n_hills, address(sigma), stride, address(period)
    if grid is not None:
        cols, table, shape, lower, spacing, periodic = grid
        t.n_grid_columns, arr = columns(cols)
        if arr is not None:
            t.grid_columns = arr
        t.table = address(table)
        for name, ctype, values in (("shape", ctypes.c_int64, None if shape is None else [int(v) for v in shape]),
                                    ("lower", ctypes.c_double, None if lower is None else [float(v) for v in lower]),
                                    ("spacing", ctypes.c_double, None if spacing is None else [float(v) for v in spacing]),
                                    ("periodic", ctypes.c_int32, None if periodic is None else [1 if v else 0 for v in periodic])):
            arr = host(ctype, values)
            if arr is not None:
                setattr(t, name, arr)
    return t, keep


class PbmetadTermsF64(ctypes.Structure):
    """molann_pbmetad_terms_f64 of include/molann_hip.h: the terms of `molann_value_and_pbmetad_f64`."""
    _fields_ = [("center", ctypes.c_void_p), ("center_stride", ctypes.c_int64), ("kappa", ctypes.c_void_p),
                ("restraint_period", ctypes.c_void_p), ("flat", ctypes.c_void_p),
                ("n_columns", ctypes.c_int32), ("columns", ctypes.POINTER(ctypes.c_int32)),
                ("table", ctypes.c_void_p), ("shape", ctypes.POINTER(ctypes.c_int64)), ("lower", ctypes.POINTER(ctypes.c_double)),
                ("spacing", ctypes.POINTER(ctypes.c_double)), ("periodic", ctypes.POINTER(ctypes.c_int32)), ("kT", ctypes.c_double)]


def pbmetad_terms_f64(tables, restraint=None, ptr=lambda t: t.data_ptr()):
    """A `PbmetadTermsF64` and the host arrays it points into (keep both alive for the call).  tables: (columns, table, shape, lower,
    spacing, periodic, kT) - columns None is the identity list and needs the count in its place: (None, K); shape, lower, spacing or
    periodic None stays NULL; restraint: None or (center, kappa, period, flat, center_stride).  Tensors give their addresses through
    `ptr`."""
    t, keep = PbmetadTermsF64(), []

    def host(ctype, values):
        if values is None:
            return None
        arr = (ctype * max(len(values), 1))(*values)
        keep.append(arr)
        return arr

    if restraint is not None:
        center, kappa, period, flat, stride = restraint
        t.center, t.center_stride, t.kappa, t.restraint_period, t.flat = (None if center is None else ptr(center), stride, None if kappa is None else ptr(kappa),
                                                                          None if period is None else ptr(period), None if flat is None else ptr(flat))
    cols, table, shape, lower, spacing, periodic, kT = tables
    if isinstance(cols, tuple) and len(cols) == 2 and cols[0] is None:
        t.n_columns = int(cols[1])
    else:
        t.n_columns = len(cols)
        arr = host(ctypes.c_int32, [int(c) for c in cols])
        if arr is not None:
            t.columns = arr
    t.table = None if table is None else ptr(table)
    for name, ctype, values in (("shape", ctypes.c_int64, None if shape is None else [int(v) for v in shape]),
                                ("lower", ctypes.c_double, None if lower is None else [float(v) for v in lower]),
                                ("spacing", ctypes.c_double, None if spacing is None else [float(v) for v in spacing]),
                                ("periodic", ctypes.c_int32, None if periodic is None else [1 if v else 0 for v in periodic])):
        arr = host(ctype, values)
        if arr is not None:
            setattr(t, name, arr)
    t.kT = float(kT)
    return t, keep


class OpesTermF64(ctypes.Structure):
    """molann_opes_term_f64 of include/molann_hip.h: the OPES term of `molann_value_and_bias_opes_f64`."""
    _fields_ = [("n_columns", ctypes.c_int32), ("columns", ctypes.POINTER(ctypes.c_int32)),
                ("centers", ctypes.c_void_p), ("heights", ctypes.c_void_p), ("n_kernels", ctypes.c_int64), ("sigma", ctypes.c_void_p),
                ("sigma_stride", ctypes.c_int64), ("period", ctypes.c_void_p),
                ("scale", ctypes.c_double), ("norm", ctypes.c_double), ("epsilon", ctypes.c_double), ("cutoff", ctypes.c_double)]


def opes_term_f64(opes, ptr=lambda t: t.data_ptr()):
    """An `OpesTermF64` and the host array it points into (keep both alive for the call).  opes: (columns, centers, heights, sigma,
    period, n_kernels, sigma_stride, scale, norm, epsilon, cutoff); tensors give their addresses through `ptr`; columns None is the
    identity list and needs the count in its place: (None, n); cutoff None is +inf."""
    cols, centers, heights, sigma, period, n_kernels, stride, scale, norm, epsilon, cutoff = opes
    o, keep = OpesTermF64(), []
    if isinstance(cols, tuple) and len(cols) == 2 and cols[0] is None:
        o.n_columns = int(cols[1])
    else:
        arr = _i32_array(cols)
        keep.append(arr)
        o.n_columns, o.columns = len(cols), arr
    o.centers, o.heights, o.sigma, o.period = (None if v is None else ptr(v) for v in (centers, heights, sigma, period))
    o.n_kernels, o.sigma_stride = n_kernels, stride
    o.scale, o.norm, o.epsilon, o.cutoff = float(scale), float(norm), float(epsilon), float("inf") if cutoff is None else float(cutoff)
    return o, keep


class OpesTableTermF64(ctypes.Structure):
    """molann_opes_table_term_f64 of include/molann_hip.h: the OPES term of `molann_value_and_bias_opes_table_f64`."""
    _fields_ = [("n_columns", ctypes.c_int32), ("columns", ctypes.POINTER(ctypes.c_int32)),
                ("centers", ctypes.c_void_p), ("heights", ctypes.c_void_p), ("sigma", ctypes.c_void_p), ("capacity", ctypes.c_int64),
                ("state", ctypes.c_void_p), ("period", ctypes.c_void_p),
                ("scale", ctypes.c_double), ("epsilon", ctypes.c_double), ("cutoff", ctypes.c_double)]


def opes_table_term_f64(opes, ptr=lambda t: t.data_ptr()):
    """An `OpesTableTermF64` and the host array it points into (keep both alive for the call).  opes: (columns, centers, heights, sigma,
    capacity, state, period, scale, epsilon, cutoff); tensors give their addresses through `ptr`; columns None is the identity list and
    needs the count in its place: (None, n); cutoff None is +inf."""
    cols, centers, heights, sigma, capacity, state, period, scale, epsilon, cutoff = opes
    o, keep = OpesTableTermF64(), []
    if isinstance(cols, tuple) and len(cols) == 2 and cols[0] is None:
        o.n_columns = int(cols[1])
    else:
        arr = _i32_array(cols)
        keep.append(arr)
        o.n_columns, o.columns = len(cols), arr
    o.centers, o.heights, o.sigma, o.state, o.period = (None if v is None else ptr(v) for v in (centers, heights, sigma, state, period))
    o.capacity = int(capacity)
    o.scale, o.epsilon, o.cutoff = float(scale), float(epsilon), float("inf") if cutoff is None else float(cutoff)
    return o, keep


_lib = None


def lib():
    """The loaded library (raises if it has not been built: no silent fallback)."""
    global _lib
    if _lib is None:
        path = DIAG_LIB_PATH if os.environ.get("MOLANN_DIAG_LIB") == "1" else LIB_PATH
        if os.environ.get("MOLANN_SAN_LIB") == "1":   # tests/test_sanitized_host.py: the ASan + UBSan build of the host half
            path = SAN_LIB_PATH
        if not os.path.exists(path):
            raise ImportError("%s not found: run `make -C %s%s` (or __graft_entry__.build())"
                              % (path, _CSRC, " diag" if path == DIAG_LIB_PATH else (" san" if path == SAN_LIB_PATH else "")))
        L = ctypes.CDLL(path)
        vp, i32, i64, f32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
        sigs = {
            "molann_abi_version": (i32, []),
            "molann_error_string": (ctypes.c_char_p, [i32]),
            "molann_build_kind": (ctypes.c_char_p, []),
            "molann_plan_create": (i32, [ctypes.POINTER(PlanDesc), ctypes.POINTER(vp)]),
            "molann_plan_destroy": (i32, [vp]),
            "molann_plan_feature_dim": (i32, [vp]),
            "molann_plan_out_dim": (i32, [vp]),
            "molann_plan_kernel_family": (i32, [vp]),
            "molann_plan_update_ref": (i32, [vp, vp, vp]),
            "molann_plan_update_mlp": (i32, [vp, ctypes.POINTER(vp), ctypes.POINTER(vp), vp]),
            "molann_align_f32": (i32, [vp, vp, i64, vp, vp]),
            "molann_features_f32": (i32, [vp, vp, i64, vp, vp]),
            "molann_forward_packed_f32": (i32, [vp, vp, i64, vp, vp]),
            "molann_forward_f32": (i32, [vp, vp, i64, ctypes.POINTER(vp), ctypes.POINTER(vp), vp, vp]),
            "molann_mlp_packed_f32": (i32, [vp, vp, i64, vp, vp]),
            "molann_plan_update_ref_f64": (i32, [vp, vp, vp]),
            "molann_align_f64": (i32, [vp, vp, i64, vp, vp]),
            "molann_features_f64": (i32, [vp, vp, i64, vp, vp]),
            "molann_mlp_f64": (i32, [vp, vp, i64, ctypes.POINTER(vp), ctypes.POINTER(vp), vp, vp]),
            "molann_forward_f64": (i32, [vp, vp, i64, ctypes.POINTER(vp), ctypes.POINTER(vp), vp, vp, vp]),
            "molann_plan_last_launch_info": (i32, [vp, ctypes.c_char_p, i32]),
            "molann_plan_grad_params_size": (i32, [vp]),
            "molann_plan_supports_backward": (i32, [vp]),
            "molann_plan_backward_kind": (i32, [vp]),
            "molann_plan_supports_mlp_backward": (i32, [vp]),
            "molann_plan_supports_value_and_vjp": (i32, [vp]),
            "molann_backward_f32": (i32, [vp, vp, vp, i64, vp, vp, vp]),
            "molann_value_and_vjp_f32": (i32, [vp, vp, vp, i64, vp, vp, vp]),
            "molann_value_and_vjp_f64": (i32, [vp, vp, vp, i64, ctypes.POINTER(vp), ctypes.POINTER(vp), vp, vp, vp]),
            "molann_plan_supports_value_and_vjp_f64": (i32, [vp]),
            "molann_value_and_jacobian_f64": (i32, [vp, vp, i64, ctypes.POINTER(vp), ctypes.POINTER(vp), vp, vp, vp]),
            "molann_plan_supports_value_and_jacobian_f64": (i32, [vp]),
            "molann_value_and_metric_f64": (i32, [vp, vp, i64, ctypes.POINTER(vp), ctypes.POINTER(vp), vp, vp, vp, vp]),
            "molann_plan_supports_value_and_metric_f64": (i32, [vp]),
            "molann_value_and_restraint_f64": (i32, [vp, vp, i64, ctypes.POINTER(vp), ctypes.POINTER(vp), vp, i64, vp, vp, vp, vp, vp, vp, vp]),
            "molann_plan_supports_value_and_restraint_f64": (i32, [vp]),
            "molann_value_and_hills_f64": (i32, [vp, vp, i64, ctypes.POINTER(vp), ctypes.POINTER(vp), vp, vp, i64, vp, i64, vp, vp, vp, vp, vp]),
            "molann_plan_supports_value_and_hills_f64": (i32, [vp]),
            "molann_value_and_opes_f64": (i32, [vp, vp, i64, ctypes.POINTER(vp), ctypes.POINTER(vp), vp, vp, i64, vp, i64, vp] + [ctypes.c_double] * 4
                                          + [vp, vp, vp, vp]),
            "molann_plan_supports_value_and_opes_f64": (i32, [vp]),
            "molann_value_and_grid_f64": (i32, [vp, vp, i64, ctypes.POINTER(vp), ctypes.POINTER(vp), vp, vp, vp, vp, vp, vp, vp, vp, vp]),
            "molann_plan_supports_value_and_grid_f64": (i32, [vp]),
            "molann_value_and_bias_f64": (i32, [vp, vp, i64, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(BiasTermsF64), vp, vp, vp, vp]),
            "molann_plan_supports_value_and_bias_f64": (i32, [vp]),
            "molann_value_and_bias_opes_f64": (i32, [vp, vp, i64, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(BiasTermsF64),
                                               ctypes.POINTER(OpesTermF64), vp, vp, vp, vp]),
            "molann_plan_supports_value_and_bias_opes_f64": (i32, [vp]),
            "molann_opes_deposit_f64": (i32, [vp, vp, vp, i64, i32, vp, vp, vp, vp, vp, i64, ctypes.c_double, ctypes.c_double, vp]),
            "molann_opes_kernel_sum_f64": (i32, [vp, i64, i32, vp, vp, i64, vp, i64, vp, ctypes.c_double, vp, vp, vp]),
            "molann_value_and_opes_table_f64": (i32, [vp, vp, i64, ctypes.POINTER(vp), ctypes.POINTER(vp), vp, vp, vp, i64, vp, vp]
                                                + [ctypes.c_double] * 3 + [vp, vp, vp, vp]),
            "molann_plan_supports_value_and_opes_table_f64": (i32, [vp]),
            "molann_opes_step_f64": (i32, [vp, vp, vp, i64, i32, vp, vp, vp, vp, vp, i64, vp, vp] + [ctypes.c_double] * 3 + [i32, vp]),
            "molann_value_and_bias_opes_table_f64": (i32, [vp, vp, i64, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(BiasTermsF64),
                                                     ctypes.POINTER(OpesTableTermF64), vp, vp, vp, vp]),
            "molann_plan_supports_value_and_bias_opes_table_f64": (i32, [vp]),
            "molann_opes_step_columns_f64": (i32, [vp, vp, vp, i64, i32, vp, vp, vp, vp, i64, ctypes.POINTER(ctypes.c_int32), vp, i64, i64, vp, vp]
                                             + [ctypes.c_double] * 3 + [i32, vp]),
            "molann_selftest_bias_opes_table_f64": (i32, [vp, i32, ctypes.POINTER(BiasTermsF64), ctypes.POINTER(OpesTableTermF64), vp, vp]),
            "molann_selftest_opes_step_columns_f64": (i32, [vp, vp, vp, i64, i32, vp, vp, vp, vp, i64, ctypes.POINTER(ctypes.c_int32), vp, i64, i64,
                                                            vp, vp] + [ctypes.c_double] * 3 + [i32]),
            "molann_opes_step_modes_f64": (i32, [vp, vp, vp, i64, i32, vp, vp, vp, vp, i64, ctypes.POINTER(ctypes.c_int32), vp, i64, i64, vp, vp, vp,
                                                 ctypes.c_double, ctypes.c_double, i64, ctypes.c_double, ctypes.c_double, i32, vp]),
            "molann_selftest_opes_step_modes_f64": (i32, [vp, vp, vp, i64, i32, vp, vp, vp, vp, i64, ctypes.POINTER(ctypes.c_int32), vp, i64, i64,
                                                          vp, vp, vp, ctypes.c_double, ctypes.c_double, i64, ctypes.c_double, ctypes.c_double, i32]),
            "molann_metad_deposit_f64": (i32, [vp, i32, vp, vp, vp, vp, vp, vp, vp, i64, vp, i64, i64] + [ctypes.c_double] * 3 + [vp, vp, i64, vp]),
            "molann_metad_widths_f64": (i32, [i32] + [vp] * 9 + [i64, vp, i64, i64, i64, i32, i64, i32, vp, vp, vp, i64, vp]),
            "molann_selftest_metad_widths_f64": (i32, [i32] + [vp] * 9 + [i64, vp, i64, i64, i64, i32, i64, i32, vp, vp, vp, i64]),
            "molann_metad_deposit_cov_f64": (i32, [vp, i32, vp, vp, vp, vp, vp, vp, i64, vp, i64, vp, i64, i64] + [ctypes.c_double] * 3
                                             + [vp, vp, i64, vp]),
            "molann_selftest_metad_deposit_cov_f64": (i32, [vp, i32, vp, vp, vp, vp, vp, vp, i64, vp, i64, vp, i64, i64] + [ctypes.c_double] * 3
                                                      + [vp, vp, i64]),
            "molann_value_and_pbmetad_f64": (i32, [vp, vp, i64, ctypes.POINTER(vp), ctypes.POINTER(vp), ctypes.POINTER(PbmetadTermsF64), vp, vp, i64,
                                             vp, vp]),
            "molann_plan_supports_value_and_pbmetad_f64": (i32, [vp]),
            "molann_selftest_pbmetad_f64": (i32, [vp, i32, ctypes.POINTER(PbmetadTermsF64), vp, vp]),
            "molann_pbmetad_deposit_f64": (i32, [vp, i32, vp, vp, vp, vp, vp, vp, vp, i64, vp, i64, i64] + [ctypes.c_double] * 4 + [vp, vp, i64, vp]),
            "molann_selftest_pbmetad_deposit_f64": (i32, [vp, i32, vp, vp, vp, vp, vp, vp, vp, i64, vp, i64, i64] + [ctypes.c_double] * 4
                                                    + [vp, vp, i64]),
            "molann_metad_rct_chunks": (i64, [i64]),
            "molann_metad_rct_f64": (i32, [vp, i64, ctypes.c_double, ctypes.c_double, vp, i64, vp, i64, vp, vp]),
            "molann_selftest_metad_rct_f64": (i32, [vp, i64, ctypes.c_double, ctypes.c_double, vp, i64, vp, i64, vp]),
            "molann_forward_train_f32": (i32, [vp, vp, i64, vp, vp, vp]),
            "molann_features_backward_f64": (i32, [vp, vp, vp, i64, vp, vp]),
            "molann_features_backward_f32": (i32, [vp, vp, vp, i64, vp, vp]),
            "molann_mlp_backward_f32": (i32, [vp, vp, vp, i64, vp, vp, vp]),
            "molann_debug_read_stamps": (i32, [vp]),
            "molann_debug_jit": (i32, [ctypes.POINTER(PlanDesc), i32, ctypes.c_char_p, i32]),
            "molann_selftest_kabsch_rotation": (i32, [vp, ctypes.c_double, vp]),
            "molann_selftest_kabsch_rotation_f32": (i32, [vp, f32, vp]),
            "molann_selftest_feature": (i32, [i32, i32, vp, vp]),
            "molann_selftest_activation": (f32, [i32, f32]),
            "molann_selftest_feature_backward": (i32, [i32, i32, vp, vp, vp]),
            "molann_selftest_kabsch_backward": (i32, [vp, vp, vp, vp]),
            "molann_selftest_act_derivative": (f32, [i32, f32]),
            "molann_selftest_act_derivative_f64": (ctypes.c_double, [i32, ctypes.c_double]),
            "molann_selftest_restraint_f64": (ctypes.c_double, [ctypes.c_double] * 5 + [ctypes.POINTER(ctypes.c_double)]),
            "molann_selftest_hills_f64": (ctypes.c_double, [vp, i32, vp, vp, i64, vp, i64, vp, vp]),
            "molann_selftest_opes_f64": (ctypes.c_double, [vp, i32, vp, vp, i64, vp, i64, vp] + [ctypes.c_double] * 4 + [vp]),
            "molann_selftest_opes_deposit_f64": (i32, [vp, vp, vp, i64, i32, vp, vp, vp, vp, vp, i64, ctypes.c_double, ctypes.c_double]),
            "molann_selftest_opes_table_f64": (ctypes.c_double, [vp, i32, vp, vp, vp, i64, vp, vp] + [ctypes.c_double] * 3 + [vp]),
            "molann_selftest_opes_step_f64": (i32, [vp, vp, vp, i64, i32, vp, vp, vp, vp, vp, i64, vp, vp] + [ctypes.c_double] * 3 + [i32]),
            "molann_selftest_metad_deposit_f64": (i32, [vp, i32, vp, vp, vp, vp, vp, vp, vp, i64, vp, i64, i64] + [ctypes.c_double] * 3
                                                  + [vp, vp, i64]),
            "molann_selftest_grid_axis_f64": (None, [ctypes.c_double, i64, ctypes.c_double, ctypes.c_double, i32, vp, vp, vp]),
            "molann_selftest_grid_f64": (ctypes.c_double, [vp, i32, vp, vp, vp, vp, vp, vp]),
            "molann_selftest_bias_f64": (i32, [vp, i32, ctypes.POINTER(BiasTermsF64), vp, vp]),
            "molann_selftest_bias_opes_f64": (i32, [vp, i32, ctypes.POINTER(BiasTermsF64), ctypes.POINTER(OpesTermF64), vp, vp]),
            "molann_selftest_item_jacobian_f64": (i32, [i32, i32, vp, vp]),
            "molann_features_jvp_f32": (i32, [vp, vp, vp, i64, i32, vp, vp, vp]),
            "molann_features_jvp_f64": (i32, [vp, vp, vp, i64, i32, vp, vp, vp]),
            "molann_selftest_feature_tangent_f32": (i32, [i32, i32, vp, vp, vp, vp]),
            "molann_selftest_feature_tangent_f64": (i32, [i32, i32, vp, vp, vp, vp]),
            "molann_selftest_kabsch_rotation_f64": (i32, [vp, ctypes.c_double, vp]),
            "molann_selftest_kabsch_tangent": (i32, [vp, vp, vp, vp]),
            "molann_selftest_kabsch_backward_f64": (i32, [vp, vp, vp, vp]),
            "molann_features_hvp_f64": (i32, [vp, vp, vp, vp, i64, vp, vp, vp]),
            "molann_selftest_feature_backward_tangent_f64": (i32, [i32, i32, vp, vp, vp, vp, vp, vp]),
            "molann_selftest_kabsch_backward_tangent": (i32, [vp, vp, vp, vp, vp, vp, vp, vp]),
        }
        for name, (res, args) in sigs.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        if L.molann_abi_version() != ABI_VERSION:
            raise ImportError("libmolann_hip.so ABI %d != binding ABI %d" % (L.molann_abi_version(), ABI_VERSION))
        _lib = L
    return _lib


def declared_symbols():
    """Every function name declared in include/molann_hip.h."""
    text = open(HEADER_PATH).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(molann_[a-z0-9_]+)\s*\(", text)))


def build_kind():
    """"release" or "diagnostics" (see include/molann_hip.h)."""
    return lib().molann_build_kind().decode()


def error_string(code):
    return lib().molann_error_string(int(code)).decode()


def _check(code, what):
    if code != 0:
        raise MolannHipError(code, what)


def _i32_array(values):
    arr = (ctypes.c_int32 * max(1, len(values)))(*[int(v) for v in values])
    return arr


def _layer_pointers(weights, biases):
    """The Linear tensors as the two host arrays of device pointers the C ABI takes (one null entry each for no layers)."""
    kind = ctypes.c_void_p * max(1, len(weights))
    return kind(*[w.data_ptr() for w in weights]), kind(*[b.data_ptr() for b in biases])


class Plan(object):
    """Owns one ``molann_plan``.  All index lists are positions inside the n_inp axis."""

    def __init__(self, n_inp, align_idx=None, ref_x=None, features=None, use_angle_value=False,
                 layer_dims=None, activation=ACT_TANH, mlp_precision=MLP_F32):
        self._handle = None
        L = lib()
        d = PlanDesc()
        d.abi_version = ABI_VERSION
        d.n_inp = int(n_inp)
        keep = []
        if align_idx is not None and len(align_idx) > 0:
            a = _i32_array(align_idx)
            r = torch.as_tensor(ref_x, dtype=torch.float32).detach().cpu().contiguous().reshape(-1)
            if r.numel() != 3 * len(align_idx):
                raise ValueError("ref_x must be [n_align, 3]")
            rbuf = (ctypes.c_float * r.numel())(*r.tolist())
            d.n_align, d.align_idx, d.ref_x = len(align_idx), a, rbuf
            keep += [a, rbuf]
        features = list(features or [])
        if features:
            ft = _i32_array([t for t, _ in features])
            ptr, flat = [0], []
            for _, idx in features:
                flat.extend(int(i) for i in idx)
                ptr.append(len(flat))
            fp, fi = _i32_array(ptr), _i32_array(flat)
            d.n_features, d.feat_type, d.feat_ptr, d.feat_idx = len(features), ft, fp, fi
            keep += [ft, fp, fi]
        d.use_angle_value = 1 if use_angle_value else 0
        if layer_dims:
            ld = _i32_array(layer_dims)
            d.n_layers, d.layer_dims = len(layer_dims) - 1, ld
            keep.append(ld)
        d.activation = int(activation)
        d.mlp_precision = int(mlp_precision)
        h = ctypes.c_void_p()
        _check(L.molann_plan_create(ctypes.byref(d), ctypes.byref(h)), "molann_plan_create")
        self._handle = h
        self.n_inp = int(n_inp)
        self.n_align = int(d.n_align)
        self.n_layers = int(d.n_layers)
        self.activation = int(activation)
        self.feature_dim = L.molann_plan_feature_dim(h)
        self.out_dim = L.molann_plan_out_dim(h)
        self.kernel_family = L.molann_plan_kernel_family(h)
        self.device = torch.cuda.current_device()

    def close(self):
        if self._handle is not None and _lib is not None:
            _lib.molann_plan_destroy(self._handle)
        self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:  # interpreter shutdown
            pass

    @staticmethod
    def _stream():
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def update_ref(self, ref_x):
        _check(lib().molann_plan_update_ref(self._handle, ctypes.c_void_p(ref_x.data_ptr()), self._stream()),
               "molann_plan_update_ref")

    def update_ref_f64(self, ref_x):
        _check(lib().molann_plan_update_ref_f64(self._handle, ctypes.c_void_p(ref_x.data_ptr()), self._stream()),
               "molann_plan_update_ref_f64")

    def align_f64(self, x, out):
        return self._run("molann_align_f64", x, out, x.shape[0])

    def features_f64(self, x, out):
        return self._run("molann_features_f64", x, out, x.shape[0])

    def forward_f64(self, x, weights, biases, work, out):
        W, B = _layer_pointers(weights, biases)
        _check(lib().molann_forward_f64(self._handle, x.data_ptr(), x.shape[0], W, B, work.data_ptr(), out.data_ptr(),
                                        self._stream()), "molann_forward_f64")
        return out

    def features_backward_f64(self, x, grad_f, grad_x):
        code = _lib.molann_features_backward_f64(self._handle, x.data_ptr(), grad_f.data_ptr(), x.shape[0], grad_x.data_ptr(),
                                                 torch.cuda.current_stream().cuda_stream)
        if code != 0:
            raise MolannHipError(code, "molann_features_backward_f64")

    def _jvp(self, fn_name, x, v, out, tangent_out):
        n_t = v.shape[0]
        code = getattr(_lib, fn_name)(self._handle, x.data_ptr(), v.data_ptr(), x.shape[0], n_t,
                                      out.data_ptr() if out is not None else None, tangent_out.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream)
        if code != 0:
            raise MolannHipError(code, fn_name)
        return tangent_out

    def features_jvp(self, x, v, out, tangent_out):
        """tangent_out[t] = J(x) v[t] of `features` (float32): x [N, n_inp, 3], v [T, N, n_inp, 3] and tangent_out
        [T, N, feature_dim] contiguous; `out` [N, feature_dim] receives the features too unless None."""
        return self._jvp("molann_features_jvp_f32", x, v, out, tangent_out)

    def features_jvp_f64(self, x, v, out, tangent_out):
        """`features_jvp` in float64."""
        return self._jvp("molann_features_jvp_f64", x, v, out, tangent_out)

    def features_hvp_f64(self, x, g, u, hx, hg):
        """The derivative of `features_backward_f64` along u, exact, in one launch: ``hx = d/dx <u, J(x)^T g>`` [N, n_inp, 3] and
        ``hg = J(x) u`` [N, feature_dim]; x, u, hx [N, n_inp, 3] and g, hg [N, feature_dim], float64, contiguous."""
        code = _lib.molann_features_hvp_f64(self._handle, x.data_ptr(), g.data_ptr(), u.data_ptr(), x.shape[0], hx.data_ptr(),
                                            hg.data_ptr(), torch.cuda.current_stream().cuda_stream)
        if code != 0:
            raise MolannHipError(code, "molann_features_hvp_f64")

    def mlp_f64(self, f, weights, biases, out):
        W, B = _layer_pointers(weights, biases)
        _check(lib().molann_mlp_f64(self._handle, f.data_ptr(), f.shape[0], W, B, out.data_ptr(), self._stream()), "molann_mlp_f64")
        return out

    def update_mlp(self, weights, biases):
        W, B = _layer_pointers(weights, biases)
        _check(lib().molann_plan_update_mlp(self._handle, W, B, self._stream()), "molann_plan_update_mlp")

    def _run(self, fn_name, x, out, n):
        code = getattr(_lib, fn_name)(self._handle, x.data_ptr(), n, out.data_ptr(),
                                      torch.cuda.current_stream().cuda_stream)
        if code != 0:
            raise MolannHipError(code, fn_name)
        return out

    def align(self, x, out):
        return self._run("molann_align_f32", x, out, x.shape[0])

    def features(self, x, out):
        return self._run("molann_features_f32", x, out, x.shape[0])

    def forward_packed(self, x, out):
        return self._run("molann_forward_packed_f32", x, out, x.shape[0])

    def mlp_packed(self, f, out):
        return self._run("molann_mlp_packed_f32", f, out, f.shape[0])

    def supports_backward(self):
        return lib().molann_plan_supports_backward(self._handle) == 1

    def supports_mlp_backward(self):
        """True when `mlp_backward` serves this plan's head (the fused family's kernel, or the wide fp32 head's)."""
        return lib().molann_plan_supports_mlp_backward(self._handle) == 1

    def supports_value_and_vjp(self):
        """True when `value_and_vjp` serves this plan (one launch); builds that kernel, so call it before a graph capture."""
        return lib().molann_plan_supports_value_and_vjp(self._handle) == 1

    def backward_kind(self):
        """2: `backward` is one pass over x; 1: several launches (keep the features of the forward: `forward_train`); 0: none."""
        return lib().molann_plan_backward_kind(self._handle)

    def grad_params_size(self):
        return lib().molann_plan_grad_params_size(self._handle)

    def backward(self, x, grad_out, grad_x, grad_params):
        """grad_x / grad_params may be None; grad_params is accumulated into."""
        code = _lib.molann_backward_f32(self._handle, x.data_ptr(), grad_out.data_ptr(), x.shape[0],
                                        grad_x.data_ptr() if grad_x is not None else None,
                                        grad_params.data_ptr() if grad_params is not None else None,
                                        torch.cuda.current_stream().cuda_stream)
        if code != 0:
            raise MolannHipError(code, "molann_backward_f32")

    def value_and_vjp(self, x, grad_out, out, grad_x):
        """out = forward(x) and grad_x = the vector-Jacobian product for `grad_out`, one launch (plans for which
        `supports_value_and_vjp()` holds)."""
        code = _lib.molann_value_and_vjp_f32(self._handle, x.data_ptr(), grad_out.data_ptr(), x.shape[0], out.data_ptr(), grad_x.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream)
        if code != 0:
            raise MolannHipError(code, "molann_value_and_vjp_f32")
        return out, grad_x

    def supports_value_and_vjp_f64(self):
        """True when `value_and_vjp_f64` serves this plan: feature items, and a frame's rows fit the LDS (nothing is built)."""
        return lib().molann_plan_supports_value_and_vjp_f64(self._handle) == 1

    def _launch(self, fn_name, *args):
        """An entry point on this plan and the current stream, `args` between the two; a non-zero code raises."""
        code = getattr(_lib, fn_name)(self._handle, *args, torch.cuda.current_stream().cuda_stream)
        if code != 0:
            raise MolannHipError(code, fn_name)

    def value_and_vjp_f64(self, x, grad_out, weights, biases, out, grad_x):
        """`value_and_vjp` in float64, one launch of frames_value_vjp_f64_kernel: `weights` / `biases` are the float64 Linear
        tensors on x's device, read as they are (empty lists for a plan without a head)."""
        W, B = _layer_pointers(weights, biases)
        self._launch("molann_value_and_vjp_f64", x.data_ptr(), grad_out.data_ptr(), x.shape[0], W, B, out.data_ptr(), grad_x.data_ptr())
        return out, grad_x

    def supports_value_and_jacobian_f64(self):
        """True when `value_and_jacobian_f64` serves this plan: feature items, and a frame's rows fit the LDS (nothing is built)."""
        return lib().molann_plan_supports_value_and_jacobian_f64(self._handle) == 1

    def value_and_jacobian_f64(self, x, weights, biases, out, jac):
        """out[N, d_out] and jac[N, d_out, n_inp, 3] = d out / d x in float64, one launch of frames_value_jac_f64_kernel: `weights` /
        `biases` are the float64 Linear tensors on x's device, read as they are (empty lists for a plan without a head)."""
        W, B = _layer_pointers(weights, biases)
        self._launch("molann_value_and_jacobian_f64", x.data_ptr(), x.shape[0], W, B, out.data_ptr(), jac.data_ptr())
        return out, jac

    def supports_value_and_metric_f64(self):
        """True when `value_and_metric_f64` serves this plan: `value_and_jacobian_f64` serves it and it has at most 64 outputs
        (nothing is built)."""
        return lib().molann_plan_supports_value_and_metric_f64(self._handle) == 1

    def value_and_metric_f64(self, x, weights, biases, atom_weights, out, metric):
        """out[N, d_out] and metric[N, d_out, d_out] = sum_a w_a (d out_k / d x_a) . (d out_l / d x_a) in float64, one launch of
        frames_value_metric_f64_kernel: `weights` / `biases` are the float64 Linear tensors on x's device, read as they are (empty
        lists for a plan without a head); `atom_weights` holds the n_inp float64 values w_a on x's device, or is None for all ones."""
        W, B = _layer_pointers(weights, biases)
        self._launch("molann_value_and_metric_f64", x.data_ptr(), x.shape[0], W, B,
                     atom_weights.data_ptr() if atom_weights is not None else None, out.data_ptr(), metric.data_ptr())
        return out, metric

    def supports_value_and_restraint_f64(self):
        """True when `value_and_restraint_f64` serves this plan: feature items, and a frame's rows (the forces' and one cotangent
        row of d_out) fit the LDS (nothing is built)."""
        return lib().molann_plan_supports_value_and_restraint_f64(self._handle) == 1

    def value_and_restraint_f64(self, x, weights, biases, center, kappa, period, flat, out, energy, grad_x, center_stride=None):
        """out[N, d_out], energy[N] = 1/2 sum_k kappa_k d_k^2 (d = out - center, wrapped by `period`, cut by `flat`) and grad_x[N, n_inp, 3]
        = d energy / d x in float64, one launch of frames_value_restraint_f64_kernel.  `weights` / `biases` as `value_and_vjp_f64`
        takes them; `center` holds d_out float64 values for all frames or [N, d_out] (`center_stride`: 0 or d_out, by default told from
        center's size); `kappa` d_out values; `period`, `flat` d_out values or None.  All on x's device."""
        W, B = _layer_pointers(weights, biases)
        d_out = out.numel() // max(x.shape[0], 1)
        if center_stride is None:
            center_stride = 0 if center.numel() == d_out else d_out
        self._launch("molann_value_and_restraint_f64", x.data_ptr(), x.shape[0], W, B, center.data_ptr(), center_stride, kappa.data_ptr(),
                     period.data_ptr() if period is not None else None, flat.data_ptr() if flat is not None else None, out.data_ptr(),
                     energy.data_ptr(), grad_x.data_ptr())
        return out, energy, grad_x

    def supports_value_and_hills_f64(self):
        """True when `value_and_hills_f64` serves this plan: `value_and_restraint_f64` serves it and it has at most 8 outputs (nothing
        is built)."""
        return lib().molann_plan_supports_value_and_hills_f64(self._handle) == 1

    def value_and_hills_f64(self, x, weights, biases, centers, heights, sigma, period, out, bias, grad_x, n_hills=None, sigma_stride=None):
        """out[N, d_out], bias[N] = sum_h heights_h exp(-1/2 sum_k (d_hk / sigma_hk)^2) (d_h = out - centers_h, wrapped by `period`) and
        grad_x[N, n_inp, 3] = d bias / d x in float64, one launch of frames_value_hills_f64_kernel.  `weights` / `biases` as
        `value_and_vjp_f64` takes them; `centers` [H, d_out] and `heights` [H] float64 (None where there are no hills; `n_hills` by default
        heights' size); `sigma` d_out float64 values for all hills or [H, d_out] (`sigma_stride`: 0 or d_out, by default told from sigma's
        dimensions); `period` d_out values or None.  All on x's device."""
        W, B = _layer_pointers(weights, biases)
        if n_hills is None:
            n_hills = heights.numel() if heights is not None else 0
        if sigma_stride is None:
            sigma_stride = sigma.shape[-1] if sigma.dim() == 2 else 0
        self._launch("molann_value_and_hills_f64", x.data_ptr(), x.shape[0], W, B, centers.data_ptr() if centers is not None else None,
                     heights.data_ptr() if heights is not None else None, n_hills, sigma.data_ptr(), sigma_stride,
                     period.data_ptr() if period is not None else None, out.data_ptr(), bias.data_ptr(), grad_x.data_ptr())
        return out, bias, grad_x

    def supports_value_and_opes_f64(self):
        """True when `value_and_opes_f64` serves this plan: `value_and_hills_f64` serves it (nothing is built)."""
        return lib().molann_plan_supports_value_and_opes_f64(self._handle) == 1

    def value_and_opes_f64(self, x, weights, biases, centers, heights, sigma, period, scale, norm, epsilon, cutoff, out, bias, grad_x,
                           n_kernels=None, sigma_stride=None):
        """out[N, d_out], bias[N] = scale log(P / norm + epsilon) with P = sum_h heights_h (exp(-q_h / 2) - exp(-cutoff^2 / 2)) over the
        kernels with q_h = sum_k (d_hk / sigma_hk)^2 < cutoff^2 (d_h = out - centers_h, wrapped by `period`) and grad_x[N, n_inp, 3] =
        d bias / d x in float64, one launch of frames_value_opes_f64_kernel.  The tensors as `value_and_hills_f64` takes them; `scale`,
        `norm`, `epsilon`, `cutoff` floats (`cutoff` None or +inf: no cutoff)."""
        W, B = _layer_pointers(weights, biases)
        if n_kernels is None:
            n_kernels = heights.numel() if heights is not None else 0
        if sigma_stride is None:
            sigma_stride = sigma.shape[-1] if sigma.dim() == 2 else 0
        self._launch("molann_value_and_opes_f64", x.data_ptr(), x.shape[0], W, B, centers.data_ptr() if centers is not None else None,
                     heights.data_ptr() if heights is not None else None, n_kernels, sigma.data_ptr() if sigma is not None else None, sigma_stride,
                     period.data_ptr() if period is not None else None, float(scale), float(norm), float(epsilon),
                     float("inf") if cutoff is None else float(cutoff), out.data_ptr(), bias.data_ptr(), grad_x.data_ptr())
        return out, bias, grad_x

    value_and_opes = value_and_opes_f64

    def supports_value_and_opes_table_f64(self):
        """True when `value_and_opes_table_f64` serves this plan: `value_and_opes_f64` serves it (nothing is built)."""
        return lib().molann_plan_supports_value_and_opes_table_f64(self._handle) == 1

    def value_and_opes_table_f64(self, x, weights, biases, centers, heights, sigma, state, period, scale, epsilon, cutoff, out, bias, grad_x):
        """`value_and_opes_f64` on a table whose live count and normalisation the kernel reads from `state` [4] = (n, S, merges, refused)
        in device memory (n held to [0, capacity], norm = S / n), one launch of frames_value_opes_table_f64_kernel: nothing is read
        back.  `centers` [capacity, d_out], `heights` [capacity] and `sigma` [capacity, d_out] are the table's storage (an
        `OpesTable`'s tensors); `period` d_out values or None; `scale`, `epsilon`, `cutoff` floats (`cutoff` None or +inf: no cutoff)."""
        W, B = _layer_pointers(weights, biases)
        self._launch("molann_value_and_opes_table_f64", x.data_ptr(), x.shape[0], W, B, centers.data_ptr(), heights.data_ptr(), sigma.data_ptr(),
                     centers.shape[0], state.data_ptr(), period.data_ptr() if period is not None else None, float(scale), float(epsilon),
                     float("inf") if cutoff is None else float(cutoff), out.data_ptr(), bias.data_ptr(), grad_x.data_ptr())
        return out, bias, grad_x

    value_and_opes_table = value_and_opes_table_f64

    def supports_value_and_grid_f64(self):
        """True when `value_and_grid_f64` serves this plan: `value_and_restraint_f64` serves it and it has at most 3 outputs (nothing
        is built)."""
        return lib().molann_plan_supports_value_and_grid_f64(self._handle) == 1

    def value_and_grid_f64(self, x, weights, biases, table, lower, spacing, periodic, out, bias, grad_x):
        """out[N, d_out], bias[N] = the cubic-convolution interpolant of `table` at out and grad_x[N, n_inp, 3] = d bias / d x in float64,
        one launch of frames_value_grid_f64_kernel.  `weights` / `biases` as `value_and_vjp_f64` takes them; `table` a contiguous
        float64 tensor on x's device with one axis per output (its shape is the grid's); `lower`, `spacing`: d_out floats; `periodic`:
        d_out bools or None - host values, read during the call."""
        W, B = _layer_pointers(weights, biases)
        d = table.dim()
        shape = (ctypes.c_int64 * d)(*table.shape)
        lo = (ctypes.c_double * d)(*[float(v) for v in lower])
        h = (ctypes.c_double * d)(*[float(v) for v in spacing])
        per = (ctypes.c_int32 * d)(*[1 if v else 0 for v in periodic]) if periodic is not None else None
        self._launch("molann_value_and_grid_f64", x.data_ptr(), x.shape[0], W, B, table.data_ptr(), shape, lo, h, per, out.data_ptr(),
                     bias.data_ptr(), grad_x.data_ptr())
        return out, bias, grad_x

    def supports_value_and_bias_f64(self):
        """True when `value_and_bias_f64` serves this plan: a frame's rows (the restraint's and the selection row of 11) fit the LDS,
        whatever the number of outputs (nothing is built)."""
        return lib().molann_plan_supports_value_and_bias_f64(self._handle) == 1

    def value_and_bias_f64(self, x, weights, biases, out, energies, grad_x, restraint=None, hills=None, grid=None):
        """out[N, d_out], energies[N, 3] = (restraint, hills, table) and grad_x[N, n_inp, 3] = d(their sum) / d x in float64, one launch
        of frames_value_bias_f64_kernel.  `weights` / `biases` as `value_and_vjp_f64` takes them.  restraint: None or (center, kappa,
        period, flat) as `value_and_restraint_f64`, on all outputs; hills: None or (columns, centers, heights, sigma, period) on the
        listed outputs (at most 8; None: the first centers.shape[1]); grid: None or (columns, table, lower, spacing, periodic) on the
        listed outputs (at most 3; None: the first table.dim()).  Device tensors on x's device; columns, lower, spacing, periodic
        are host values, read during the call."""
        W, B = _layer_pointers(weights, biases)
        d_out = out.numel() // max(x.shape[0], 1)
        r = h = g = None
        if restraint is not None:
            center, kappa, period, flat = restraint
            r = (center, kappa, period, flat, 0 if center.numel() == d_out and center.dim() < 2 else d_out)
        if hills is not None:
            cols, centers, heights, sigma, period = hills
            n_hills = centers.shape[0]
            width = centers.shape[1] if cols is None else len(cols)
            h = ((None, width) if cols is None else cols, centers if n_hills else None, heights if n_hills else None,
                 sigma if n_hills else None, period, n_hills, width if sigma.dim() == 2 else 0)
        if grid is not None:
            cols, table, lower, spacing, periodic = grid
            g = ((None, table.dim()) if cols is None else cols, table, table.shape, lower, spacing, periodic)
        terms, keep = bias_terms_f64(r, h, g)
        self._launch("molann_value_and_bias_f64", x.data_ptr(), x.shape[0], W, B, ctypes.byref(terms), out.data_ptr(), energies.data_ptr(),
                     grad_x.data_ptr())
        del keep
        return out, energies, grad_x

    def supports_value_and_pbmetad_f64(self):
        """True when `value_and_pbmetad_f64` serves this plan: `value_and_bias_f64` serves it (nothing is built)."""
        return lib().molann_plan_supports_value_and_pbmetad_f64(self._handle) == 1

    def value_and_pbmetad_f64(self, x, weights, biases, out, energies, grad_x, tables, restraint=None):
        """out[N, d_out], energies[N, 2 + K] = (restraint, V_PB, V_0 ..) and grad_x[N, n_inp, 3] = d(restraint + V_PB) / d x in float64,
        one launch of frames_value_pbmetad_f64_kernel.  `weights` / `biases` as `value_and_vjp_f64` takes them.  tables: (columns, table,
        shape, lower, spacing, periodic, kT) - the K one-dimensional tables back to back in `table` on x's device, the rest host values
        read during the call; restraint: None or (center, kappa, period, flat) as `value_and_restraint_f64`, on all outputs.  The
        energies' row stride is passed on, so a slice of a wider tensor serves."""
        W, B = _layer_pointers(weights, biases)
        d_out = out.numel() // max(x.shape[0], 1)
        r = None
        if restraint is not None:
            center, kappa, period, flat = restraint
            r = (center, kappa, period, flat, 0 if center.numel() == d_out and center.dim() < 2 else d_out)
        terms, keep = pbmetad_terms_f64(tables, r)
        stride = energies.stride(0) if energies.dim() == 2 and energies.shape[0] > 1 else energies.shape[-1]
        self._launch("molann_value_and_pbmetad_f64", x.data_ptr(), x.shape[0], W, B, ctypes.byref(terms), out.data_ptr(), energies.data_ptr(),
                     stride, grad_x.data_ptr())
        del keep
        return out, energies, grad_x

    def supports_value_and_bias_opes_f64(self):
        """True when `value_and_bias_opes_f64` serves this plan: `value_and_bias_f64` serves it (nothing is built)."""
        return lib().molann_plan_supports_value_and_bias_opes_f64(self._handle) == 1

    def value_and_bias_opes_f64(self, x, weights, biases, out, energies, grad_x, opes, restraint=None, grid=None):
        """out[N, d_out], energies[N, 4] = (restraint, 0, table, OPES) and grad_x[N, n_inp, 3] = d(their sum) / d x in float64, one launch
        of frames_value_bias_opes_f64_kernel.  `weights` / `biases` as `value_and_vjp_f64` takes them.  opes: (columns, centers, heights,
        sigma, period, scale, norm, epsilon, cutoff) on the listed outputs (at most 8; None: the first centers.shape[1]), the tensors as
        `value_and_opes_f64` takes them over those outputs, `cutoff` None or +inf for none; restraint, grid: None or as
        `value_and_bias_f64` takes them.  Device tensors on x's device; columns, the four scalars, lower, spacing, periodic are host
        values, read during the call."""
        W, B = _layer_pointers(weights, biases)
        d_out = out.numel() // max(x.shape[0], 1)
        r = g = None
        if restraint is not None:
            center, kappa, period, flat = restraint
            r = (center, kappa, period, flat, 0 if center.numel() == d_out and center.dim() < 2 else d_out)
        if grid is not None:
            cols, table, lower, spacing, periodic = grid
            g = ((None, table.dim()) if cols is None else cols, table, table.shape, lower, spacing, periodic)
        cols, centers, heights, sigma, period, scale, norm, epsilon, cutoff = opes
        n_kernels = centers.shape[0]
        width = centers.shape[1] if cols is None else len(cols)
        term, keep_o = opes_term_f64(((None, width) if cols is None else cols, centers if n_kernels else None, heights if n_kernels else None,
                                      sigma if n_kernels else None, period, n_kernels, width if sigma.dim() == 2 else 0, scale, norm, epsilon,
                                      cutoff))
        terms, keep = bias_terms_f64(r, None, g)
        self._launch("molann_value_and_bias_opes_f64", x.data_ptr(), x.shape[0], W, B, ctypes.byref(terms), ctypes.byref(term), out.data_ptr(),
                     energies.data_ptr(), grad_x.data_ptr())
        del keep, keep_o
        return out, energies, grad_x

    value_and_bias_opes = value_and_bias_opes_f64

    def supports_value_and_bias_opes_table_f64(self):
        """True when `value_and_bias_opes_table_f64` serves this plan: `value_and_bias_f64` serves it (nothing is built)."""
        return lib().molann_plan_supports_value_and_bias_opes_table_f64(self._handle) == 1

    def value_and_bias_opes_table_f64(self, x, weights, biases, out, energies, grad_x, opes, restraint=None, grid=None):
        """`value_and_bias_opes_f64` on a kernel table whose live count and normalisation the kernel reads from `state` [4] in device
        memory, one launch of frames_value_bias_opes_table_f64_kernel: nothing is read back.  opes: (columns, centers, heights, sigma,
        state, period, scale, epsilon, cutoff) - the table's storage ``[capacity, len(columns)]``, ``[capacity]``, ``[capacity,
        len(columns)]`` and its state, contiguous float64 on x's device; restraint, grid: None or as `value_and_bias_f64` takes them."""
        W, B = _layer_pointers(weights, biases)
        d_out = out.numel() // max(x.shape[0], 1)
        r = g = None
        if restraint is not None:
            center, kappa, period, flat = restraint
            r = (center, kappa, period, flat, 0 if center.numel() == d_out and center.dim() < 2 else d_out)
        if grid is not None:
            cols, table, lower, spacing, periodic = grid
            g = ((None, table.dim()) if cols is None else cols, table, table.shape, lower, spacing, periodic)
        cols, centers, heights, sigma, state, period, scale, epsilon, cutoff = opes
        term, keep_o = opes_table_term_f64(((None, centers.shape[1]) if cols is None else cols, centers, heights, sigma, centers.shape[0], state,
                                            period, scale, epsilon, cutoff))
        terms, keep = bias_terms_f64(r, None, g)
        self._launch("molann_value_and_bias_opes_table_f64", x.data_ptr(), x.shape[0], W, B, ctypes.byref(terms), ctypes.byref(term),
                     out.data_ptr(), energies.data_ptr(), grad_x.data_ptr())
        del keep, keep_o
        return out, energies, grad_x

    value_and_bias_opes_table = value_and_bias_opes_table_f64

    def forward_train(self, x, out, features):
        """`forward_packed` that also keeps the features (for `mlp_backward` + `features_backward`)."""
        code = _lib.molann_forward_train_f32(self._handle, x.data_ptr(), x.shape[0], out.data_ptr(), features.data_ptr(),
                                             torch.cuda.current_stream().cuda_stream)
        if code != 0:
            raise MolannHipError(code, "molann_forward_train_f32")
        return out

    def features_backward(self, x, grad_f, grad_x):
        """dL/dx of `features` for the same x."""
        code = _lib.molann_features_backward_f32(self._handle, x.data_ptr(), grad_f.data_ptr(), x.shape[0], grad_x.data_ptr(),
                                                 torch.cuda.current_stream().cuda_stream)
        if code != 0:
            raise MolannHipError(code, "molann_features_backward_f32")

    def mlp_backward(self, f, grad_out, grad_f, grad_params):
        """Backward of `mlp_packed` for the same f; grad_f / grad_params may be None; grad_params is accumulated into."""
        code = _lib.molann_mlp_backward_f32(self._handle, f.data_ptr(), grad_out.data_ptr(), f.shape[0],
                                            grad_f.data_ptr() if grad_f is not None else None,
                                            grad_params.data_ptr() if grad_params is not None else None,
                                            torch.cuda.current_stream().cuda_stream)
        if code != 0:
            raise MolannHipError(code, "molann_mlp_backward_f32")

    def last_launch_info(self):
        buf = ctypes.create_string_buffer(256)
        lib().molann_plan_last_launch_info(self._handle, buf, 256)
        return buf.value.decode()


def _address(t):
    return None if t is None else t.data_ptr()


def opes_deposit_f64(centers, sigma, heights, state, period, new_centers, new_sigma, new_heights, threshold, cutoff=None):
    """`molann_opes_deposit_f64` on torch's current stream: the new kernels (`new_centers` [W, d], `new_sigma` [W, d], `new_heights` [W])
    are compressed into the table `centers` [cap, d], `sigma` [cap, d], `heights` [cap] in place and `state` [4] = (n, S, merges, refused)
    is updated, in one launch; nothing is read back.  Contiguous float64 tensors on one device (`period`: [d] or None); `cutoff` None
    is +inf.  The tensors' shapes are the caller's to check (`molann_amd.bias.OpesTable` does)."""
    code = lib().molann_opes_deposit_f64(centers.data_ptr(), sigma.data_ptr(), heights.data_ptr(), centers.shape[0], centers.shape[1],
                                         _address(period), state.data_ptr(), new_centers.data_ptr(), new_sigma.data_ptr(),
                                         new_heights.data_ptr(), new_centers.shape[0], float(threshold),
                                         float("inf") if cutoff is None else float(cutoff), torch.cuda.current_stream().cuda_stream)
    _check(code, "molann_opes_deposit_f64")


def opes_step_f64(centers, sigma, heights, state, run, period, y, V, sigma0, sigma_min, beta, threshold, cutoff=None, fixed_sigma=False):
    """`molann_opes_step_f64` on torch's current stream: from `y` [W, d] and `V` [W] (the outputs and biases a bias launch just wrote, read
    only) this step's kernels are formed - weights exp(beta V), the effective sample size, the rescaled widths `sigma0` [d] held above
    `sigma_min` ([d] or None), the heights - and compressed into the table `centers` [cap, d], `sigma` [cap, d], `heights` [cap] in place;
    `state` [4] = (n, S, merges, refused) and `run` [8] = (counter, sum_w, sum_w2, neff, sigma_scale, rct, 0, 0) are updated, in one
    launch; nothing is read back.  Contiguous float64 tensors on one device (`period`: [d] or None); `cutoff` None is +inf.  The tensors'
    shapes are the caller's to check (`molann_amd.bias.OpesRun` does)."""
    code = lib().molann_opes_step_f64(centers.data_ptr(), sigma.data_ptr(), heights.data_ptr(), centers.shape[0], centers.shape[1],
                                      _address(period), state.data_ptr(), run.data_ptr(), y.data_ptr(), V.data_ptr(), y.shape[0],
                                      sigma0.data_ptr(), _address(sigma_min), float(beta), float(threshold),
                                      float("inf") if cutoff is None else float(cutoff), 1 if fixed_sigma else 0,
                                      torch.cuda.current_stream().cuda_stream)
    _check(code, "molann_opes_step_f64")


def opes_step_columns_f64(centers, sigma, heights, state, run, period, y, columns, V, sigma0, sigma_min, beta, threshold, cutoff=None,
                          fixed_sigma=False):
    """`molann_opes_step_columns_f64` on torch's current stream: `opes_step_f64` with walker a's centre read at ``y[a, columns[k]]`` of
    `y` [W, n_out] (its row stride is passed on) and its bias at `V` ([W], or a column of a wider tensor: its stride is passed on).
    `columns`: a ctypes array of d int32 (`_i32_array`), made once, or None for the first d outputs.  The tensors' shapes are the
    caller's to check (`molann_amd.bias.OpesRun` does)."""
    n_walkers = y.shape[0]
    code = lib().molann_opes_step_columns_f64(centers.data_ptr(), sigma.data_ptr(), heights.data_ptr(), centers.shape[0], centers.shape[1],
                                              _address(period), state.data_ptr(), run.data_ptr(), y.data_ptr(),
                                              y.stride(0) if n_walkers > 1 else y.shape[1], columns, V.data_ptr(),
                                              V.stride(0) if n_walkers > 1 else 1, n_walkers, sigma0.data_ptr(), _address(sigma_min), float(beta),
                                              float(threshold), float("inf") if cutoff is None else float(cutoff), 1 if fixed_sigma else 0,
                                              torch.cuda.current_stream().cuda_stream)
    _check(code, "molann_opes_step_columns_f64")


OPES_FIXED_SIGMA, OPES_EXPLORE, OPES_OBSERVE = 1, 2, 4      # the bits of molann_opes_step_modes_f64's `flags`


def opes_step_modes_f64(centers, sigma, heights, state, run, period, y, columns, V, sigma0, sigma_min, adapt, beta, biasfactor, adaptive_stride,
                        threshold, cutoff=None, fixed_sigma=False, explore=False, observe=False):
    """`molann_opes_step_modes_f64` on torch's current stream: `opes_step_columns_f64` with widths measured from the run where `adapt`
    ([W, 3, d] rows of (mean, M2, sigma0), updated in place; `sigma0` may then be None) is given, and the explore variant with
    `explore`; `observe`: the averages alone (`V` None: not read).  `run[6]` counts the observations, `run[7]` says whether the first
    deposit has fixed sigma0.  The tensors' shapes are the caller's to check (`molann_amd.bias.OpesRun` does)."""
    n_walkers = y.shape[0]
    if V is None:
        V = y
    flags = (OPES_FIXED_SIGMA if fixed_sigma else 0) | (OPES_EXPLORE if explore else 0) | (OPES_OBSERVE if observe else 0)
    code = lib().molann_opes_step_modes_f64(centers.data_ptr(), sigma.data_ptr(), heights.data_ptr(), centers.shape[0], centers.shape[1],
                                            _address(period), state.data_ptr(), run.data_ptr(), y.data_ptr(),
                                            y.stride(0) if n_walkers > 1 else y.shape[1], columns, V.data_ptr(),
                                            V.stride(0) if n_walkers > 1 else 1, n_walkers, _address(sigma0), _address(sigma_min), _address(adapt),
                                            float(beta), float(biasfactor), int(adaptive_stride), float(threshold),
                                            float("inf") if cutoff is None else float(cutoff), flags, torch.cuda.current_stream().cuda_stream)
    _check(code, "molann_opes_step_modes_f64")


def metad_grid_arrays(shape, lower, spacing, periodic, sigma, columns):
    """The host arrays `molann_metad_deposit_f64` reads during the call, as ctypes arrays: ``(shape, lower, spacing, periodic, sigma,
    columns)``; `periodic` and `columns` may be None (NULL: no periodic axis, the first outputs)."""
    d = len(shape)
    I = lambda v: None if v is None else (ctypes.c_int32 * d)(*[int(c) for c in v])  # noqa: E731
    F = lambda v: (ctypes.c_double * d)(*[float(c) for c in v])  # noqa: E731
    return (ctypes.c_int64 * d)(*[int(n) for n in shape]), F(lower), F(spacing), I(periodic), F(sigma), I(columns)


def metad_deposit_f64(table, arrays, y, V, height0, inv_dT, cutoff, state, log=None):
    """`molann_metad_deposit_f64` on torch's current stream: the hills of the walkers `y` [W, n_out] (centres in the columns the arrays
    name) with biases `V` ([W], or a column of a wider tensor: its stride is passed on) are added to `table` in place with heights
    ``height0 exp(-V inv_dT)``; `state` [8] and `log` ([capacity, 2 d + 1] or None) are updated, in one launch; nothing is read back.
    `arrays`: `metad_grid_arrays`, made once.  float64 tensors on one device, `table`, `y`, `state`, `log` contiguous; `cutoff` None is
    +inf.  The tensors' shapes are the caller's to check (`molann_amd.bias.MetadRun` does)."""
    shape, lower, spacing, periodic, sigma, columns = arrays
    code = lib().molann_metad_deposit_f64(table.data_ptr(), len(shape), shape, lower, spacing, periodic, sigma, columns, y.data_ptr(), y.stride(0),
                                          V.data_ptr(), V.stride(0), y.shape[0], float(height0), float(inv_dT),
                                          float("inf") if cutoff is None else float(cutoff), state.data_ptr(), _address(log),
                                          0 if log is None else log.shape[0], torch.cuda.current_stream().cuda_stream)
    _check(code, "molann_metad_deposit_f64")


def pbmetad_deposit_f64(table, arrays, y, V, height0, inv_dT, kT, cutoff, state, log=None):
    """`molann_pbmetad_deposit_f64` on torch's current stream: the hills of the walkers `y` [W, n_out] (centres in the columns the arrays
    name) with per-axis biases `V` ([W, K], or columns of a wider tensor: its row stride is passed on) are added to the K one-dimensional
    tables back to back in `table`, every height weighted by its axis' share of the soft minimum at `kT`; `state` [8] and `log`
    ([capacity, 2 K] or None) are updated, in one launch; nothing is read back.  `arrays`: `metad_grid_arrays` over the K axes, made
    once.  float64 tensors on one device, `table`, `state`, `log` contiguous; `cutoff` None is +inf.  The tensors' shapes are the
    caller's to check (`molann_amd.bias.PBMetadRun` does)."""
    shape, lower, spacing, periodic, sigma, columns = arrays
    code = lib().molann_pbmetad_deposit_f64(table.data_ptr(), len(shape), shape, lower, spacing, periodic, sigma, columns, y.data_ptr(),
                                            y.stride(0) if y.shape[0] > 1 else y.shape[1], V.data_ptr(),
                                            V.stride(0) if V.shape[0] > 1 else max(V.shape[1], len(shape)), y.shape[0], float(height0),
                                            float(inv_dT), float(kT), float("inf") if cutoff is None else float(cutoff), state.data_ptr(),
                                            _address(log), 0 if log is None else log.shape[0], torch.cuda.current_stream().cuda_stream)
    _check(code, "molann_pbmetad_deposit_f64")


METAD_COV_DIFF, METAD_COV_GEOM = 1, 2


def metad_limit_arrays(sigma_min, sigma_max, d):
    """``(sigma_min, sigma_max)`` of `molann_metad_widths_f64` as ctypes arrays; None stays None (NULL: 0, +inf)."""
    F = lambda v: None if v is None else (ctypes.c_double * d)(*[float(c) for c in v])  # noqa: E731
    return F(sigma_min), F(sigma_max)


def metad_widths_f64(arrays, limits, mode, window, emit, adapt, adapt_state, cov, y=None, metric=None):
    """`molann_metad_widths_f64` on torch's current stream, one launch, nothing read back.  `mode` METAD_COV_DIFF: the rows of `adapt`
    [W, 1 + d + T] take one observation of `y` [W, n_out]; METAD_COV_GEOM: the covariances come from `metric` [W, n_out, n_out]
    (contiguous).  With `emit` the walkers' hill covariances go to `cov` [W, T]; `adapt_state` [8] counts.  `arrays`:
    `metad_grid_arrays`, `limits`: `metad_limit_arrays`, made once.  float64 tensors on one device, contiguous; their shapes are the
    caller's to check (`molann_amd.bias.MetadRun` does)."""
    shape, lower, spacing, periodic, sigma, columns = arrays
    n_walkers = cov.shape[0]
    n_out = 0 if metric is None else metric.shape[-1]
    code = lib().molann_metad_widths_f64(len(shape), shape, lower, spacing, periodic, sigma, limits[0], limits[1], columns, _address(y),
                                         0 if y is None else y.stride(0), _address(metric), n_out * n_out, n_out, n_walkers, int(mode), int(window),
                                         1 if emit else 0, _address(adapt), adapt_state.data_ptr(), cov.data_ptr(), cov.stride(0),
                                         torch.cuda.current_stream().cuda_stream)
    _check(code, "molann_metad_widths_f64")


def metad_deposit_cov_f64(table, arrays, y, V, cov, height0, inv_dT, cutoff, state, log=None):
    """`molann_metad_deposit_cov_f64` on torch's current stream: `metad_deposit_f64` with walker a's hill a multivariate Gaussian of
    covariance `cov[a]` ([W, T] upper triangles, or columns of a wider tensor: its stride is passed on); `log` is [capacity, d + T + 1]
    or None.  One launch, nothing read back.  The `sigma` of `arrays` is not read."""
    shape, lower, spacing, periodic, _, columns = arrays
    code = lib().molann_metad_deposit_cov_f64(table.data_ptr(), len(shape), shape, lower, spacing, periodic, columns, y.data_ptr(), y.stride(0),
                                              V.data_ptr(), V.stride(0), cov.data_ptr(), cov.stride(0), y.shape[0], float(height0), float(inv_dT),
                                              float("inf") if cutoff is None else float(cutoff), state.data_ptr(), _address(log),
                                              0 if log is None else log.shape[0], torch.cuda.current_stream().cuda_stream)
    _check(code, "molann_metad_deposit_cov_f64")


def metad_rct_f64(table, kT, inv_dT, state, stride, partials, rct):
    """`molann_metad_rct_f64` on torch's current stream: the reweighting offset c(t) of `table` (any shape, read flat) into `rct` [8], through
    `partials` [at least `molann_metad_rct_chunks(table.numel())`, 4]; two launches, nothing read back.  `state` [8] or None: with a state
    the device skips the update unless ``state[3]`` is a multiple of `stride`.  Contiguous float64 tensors on one device; their shapes are
    the caller's to check (`molann_amd.bias.MetadRun` does)."""
    code = lib().molann_metad_rct_f64(table.data_ptr(), table.numel(), float(kT), float(inv_dT), _address(state), int(stride), partials.data_ptr(),
                                      partials.shape[0], rct.data_ptr(), torch.cuda.current_stream().cuda_stream)
    _check(code, "molann_metad_rct_f64")


def opes_kernel_sum_f64(points, centers, heights, sigma, period, cutoff, P, dP=None):
    """`molann_opes_kernel_sum_f64` on torch's current stream: P[M] (and dP[M, d] where given) of `points` [M, d] under the table
    `centers` [H, d], `heights` [H], `sigma` [d] or [H, d]; one launch.  Contiguous float64 tensors on one device; `cutoff` None is
    +inf.  Returns P, or (P, dP)."""
    n_kernels, d = centers.shape[0], points.shape[1]
    code = lib().molann_opes_kernel_sum_f64(points.data_ptr(), points.shape[0], d, centers.data_ptr() if n_kernels else None,
                                            heights.data_ptr() if n_kernels else None, n_kernels, sigma.data_ptr() if n_kernels else None,
                                            d if sigma.dim() == 2 else 0, _address(period), float("inf") if cutoff is None else float(cutoff),
                                            P.data_ptr(), _address(dP), torch.cuda.current_stream().cuda_stream)
    _check(code, "molann_opes_kernel_sum_f64")
    return P if dP is None else (P, dP)


def workload_desc(w):
    """``(PlanDesc, keep)`` for a `molann_amd.workloads.Workload` (0-based indices, zero reference coordinates): what
    `molann_debug_jit` cross-compiles a plan's specialised kernels from without a device.  `keep` holds the ctypes arrays
    the description points into."""
    d = PlanDesc()
    d.abi_version, d.n_inp = ABI_VERSION, w.n_atoms
    keep = []
    I = lambda v: (ctypes.c_int32 * max(1, len(v)))(*v)  # noqa: E731
    if w.align:
        a, r = I([x - 1 for x in w.align]), (ctypes.c_float * (3 * len(w.align)))()
        d.n_align, d.align_idx, d.ref_x = len(w.align), a, r
        keep += [a, r]
    ptr, flat = [0], []
    for _, atoms in w.features:
        flat += [x - 1 for x in atoms]
        ptr.append(len(flat))
    ft, fp, fi = I([t for t, _ in w.features]), I(ptr), I(flat)
    d.n_features, d.feat_type, d.feat_ptr, d.feat_idx = len(w.features), ft, fp, fi
    keep += [ft, fp, fi]
    if w.mlp_dims:
        ld = I(w.mlp_dims)
        d.n_layers, d.layer_dims = len(w.mlp_dims) - 1, ld
        keep.append(ld)
    return d, keep
