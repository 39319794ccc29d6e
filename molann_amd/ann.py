"""`molann.ann`'s module API on the MI355X: same classes, constructor signatures, attributes,
error behaviour and state_dict keys; `forward` runs hand-written gfx950 kernels through the C ABI
in ``libmolann_hip.so`` (see ``include/molann_hip.h``).

    AlignmentLayer(align_atom_group, input_atom_group)           ann.py:69-199
    FeatureMap(feature, input_atom_group, use_angle_value)       ann.py:201-356
    FeatureLayer(feature_list, input_atom_group, use_angle_value) ann.py:358-474
    PreprocessingANN(align_layer, feature_layer)                 ann.py:476-565
    MolANN(preprocessing_layer, ann_layers)                      ann.py:567-624
    create_sequential_nn(layer_dims, activation)                 ann.py:37-67

There is no CPU or composite-PyTorch fallback: a forward on anything but a float32 or float64 tensor that
lives on a HIP device raises.  float64 (`model.double()(x.double())`, which the reference supports because its
modules follow x.dtype) runs the `molann_*_f64` kernels; under grad mode its features are differentiated by
`molann_features_backward_f64` and its MLP runs as the torch module it is.  float32 gradients (w.r.t. x and the Linear parameters) come from hand-written backward
kernels: fused with the MLP for the plans the lane-per-frame kernel serves (22-atom class, MLP widths <= 32),
features only on large frames (one wave per frame).  With an MLP outside the fused kernel (wider, ELU / GELU /
Softplus, or any MLP on large frames) a forward under grad mode takes features and their gradient from the
kernels and runs ``ann_layers`` as the torch module it is.  Forward mode (``torch.autograd.forward_ad`` duals, ``torch.func.jvp`` /
``jacfwd`` / ``vmap``) takes its own path, only when a tangent is present: the features and their tangents from the tangent
kernel (`_FeaturesJvp`, `_FeaturesTangent`), ``ann_layers`` as the torch module it is.
"""

import math

import torch
import torch._C._functorch as _functorch
import pandas as pd
from torch.autograd import forward_ad as _fwAD

from . import _capi
from . import bias as _bias

_ACT_CODES = (
    (torch.nn.Tanh, _capi.ACT_TANH, lambda m: True),
    (torch.nn.ReLU, _capi.ACT_RELU, lambda m: True),
    (torch.nn.Sigmoid, _capi.ACT_SIGMOID, lambda m: True),
    (torch.nn.Identity, _capi.ACT_IDENTITY, lambda m: True),
    (torch.nn.ELU, _capi.ACT_ELU, lambda m: m.alpha == 1.0),
    (torch.nn.SiLU, _capi.ACT_SILU, lambda m: True),
    (torch.nn.Softplus, _capi.ACT_SOFTPLUS, lambda m: m.beta == 1.0 and m.threshold == 20.0),
    (torch.nn.LeakyReLU, _capi.ACT_LEAKY_RELU, lambda m: m.negative_slope == 0.01),
    (torch.nn.GELU, _capi.ACT_GELU, lambda m: getattr(m, "approximate", "none") == "none"),
)


def create_sequential_nn(layer_dims, activation=torch.nn.Tanh()):
    """Feed-forward network ``Linear -> act -> ... -> Linear`` (no activation after the last layer).

    Module names follow the reference (`ann.py:63-65`) so that state_dict keys are interchangeable:
    ``'{i}th_layer'`` and ``'activation of {i}th_layer'``; one activation object is shared.
    """
    assert len(layer_dims) >= 2, 'Error: at least 2 layers are needed to define a neural network (length={})!'.format(len(layer_dims))
    net = torch.nn.Sequential()
    n_linear = len(layer_dims) - 1
    for i in range(1, n_linear + 1):
        net.add_module('%dth_layer' % i, torch.nn.Linear(layer_dims[i - 1], layer_dims[i]))
        if i < n_linear:
            net.add_module('activation of %dth_layer' % i, activation)
    return net


def _activation_code(module):
    for cls, code, ok in _ACT_CODES:
        if type(module) is cls and ok(module):
            return code
    return None


def recognise_mlp(ann_layers):
    """``(linears, activation_code)`` if ``ann_layers`` is a Sequential of the shape
    `create_sequential_nn` builds with an activation the kernels implement, else ``None``.
    Walks ``_modules`` (``children()`` de-duplicates the shared activation object)."""
    if not isinstance(ann_layers, torch.nn.Sequential):
        return None
    mods = list(ann_layers._modules.values())
    if not mods or len(mods) % 2 == 0:
        return None
    linears, code = [], None
    for i, m in enumerate(mods):
        if i % 2 == 0:
            if type(m) is not torch.nn.Linear or m.bias is None:
                return None
            linears.append(m)
        else:
            c = _activation_code(m)
            if c is None or (code is not None and c != code):
                return None
            code = c
    for a, b in zip(linears[:-1], linears[1:]):
        if a.out_features != b.in_features:
            return None
    if len(linears) > _capi.MAX_LAYERS:
        return None
    return linears, (_capi.ACT_IDENTITY if code is None else code)


_RUN_OP = []


def _run_op():
    """``torch.ops.molann.run`` if csrc/libmolann_torch.so has been built, else None (then ctypes serves every call)."""
    if not _RUN_OP:
        import os
        if os.environ.get("MOLANN_DIAG_LIB") == "1":   # tools/ on the diagnostics build: the operator library is
            _RUN_OP.append(None)                        # linked against the release build, so ctypes serves every call
            return None
        try:
            from . import script
            script.load_ops()
            _RUN_OP.append(torch.ops.molann.run)
        except ImportError:
            _RUN_OP.append(None)
    return _RUN_OP[0]


def _local_indices(input_indices, wanted, what):
    try:
        return [input_indices.index(int(i)) for i in wanted]
    except ValueError:
        raise ValueError(what)


def _check_input(x, input_atom_num):
    assert isinstance(x, torch.Tensor), 'Input x is not a torch tensor'
    assert x.size(1) == input_atom_num and x.size(2) == 3, \
        f'Input should be a 3d torch tensor, with sizes [*, {input_atom_num}, 3]. Actual sizes: {x.shape}'


def _wants_grad(x, grad_sources=()):
    return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in grad_sources))


def _device_input(x, grad_sources=(), backward_ok=False):
    """The tensor the kernels read: float32 or float64, on a HIP device, contiguous.  Everything else raises."""
    if not x.is_cuda:
        raise RuntimeError("molann_amd runs on the MI355X only: got a %s tensor (no CPU path; move x and the "
                           "module to a HIP device)" % x.device.type)
    if x.dtype not in (torch.float32, torch.float64):
        raise TypeError("molann_amd kernels are float32 / float64; got %s" % x.dtype)
    if not backward_ok and _wants_grad(x, grad_sources):
        raise NotImplementedError("no backward kernel for this module / plan yet: call it under "
                                  "torch.no_grad() (or freeze the parameters)")
    return x if x.is_contiguous() else x.contiguous()


def _release_plans(desc, device):
    """weakref.finalize callback of a MolANN: its plans in the operator library's cache go with it."""
    try:
        torch.ops.molann.release(desc, device)
    except Exception:   # interpreter shutdown / library gone
        pass


class _PlanFunction(torch.autograd.Function):
    """forward = one fused launch of the plan; backward = molann_backward_f32: one pass over x that recomputes the forward
    per frame (nothing but x is saved), runs the MLP's backward on the matrix cores and the analytic reverse mode of
    the preprocessing.  Where that kernel could not be built (`backward_kind() == 1`) the forward also keeps the
    features and the backward is two launches, molann_mlp_backward_f32 and molann_features_backward_f32.
    `params` are the Linear weights/biases in layer order (may be empty)."""

    @staticmethod
    def forward(ctx, x, entry, with_mlp, *params):
        plan = entry.plan
        out = torch.empty((x.shape[0], plan.out_dim if with_mlp else plan.feature_dim), dtype=torch.float32, device=x.device)
        feat = None
        # What the backward will need is known here.  Gradients for x: one pass over x does everything (backward_kind 2),
        # nothing to keep.  Parameters only (x is data): the MLP's backward alone, on the features this forward keeps
        # (C3: 63 us per 1 M frames instead of 104 for the pass over x).
        if with_mlp and entry.backward_kind() != 1 and ctx.needs_input_grad[0]:
            plan.forward_packed(x, out)
        elif with_mlp:
            feat = torch.empty((x.shape[0], plan.feature_dim), dtype=torch.float32, device=x.device)
            try:
                plan.forward_train(x, out, feat)
            except _capi.MolannHipError as e:       # no feature-keeping twin of this plan's kernel: the backward recomputes
                if e.code != _capi.E_UNSUPPORTED:
                    raise
                feat = None
                plan.forward_packed(x, out)
        else:
            plan.features(x, out)
        if feat is None:
            ctx.save_for_backward(x)
        else:
            ctx.save_for_backward(x, feat)
        ctx.entry, ctx.shapes = entry, [tuple(p.shape) for p in params]
        ctx.with_mlp, ctx.params = with_mlp, params      # (create_graph=True: the backward is then rebuilt as a differentiable composition)
        return out

    @staticmethod
    def backward(ctx, grad_out):
        # Grad mode is on inside a backward only under create_graph=True: the caller wants to differentiate these gradients
        # again (a loss on forces; the reference can, through plain autograd incl. its SVD, ann.py:188-197).  The kernels'
        # results carry no graph, so the gradient is rebuilt as a DIFFERENTIABLE composition: the float64 features with their
        # double-differentiable backward (_FeatBackward64), the MLP as ATen ops on the live parameters.
        if torch.is_grad_enabled():
            return _double_backward(ctx, grad_out)
        x = ctx.saved_tensors[0]
        feat = ctx.saved_tensors[1] if len(ctx.saved_tensors) > 1 else None
        plan = ctx.entry.plan
        need_x = ctx.needs_input_grad[0]
        need_p = any(ctx.needs_input_grad[3:])
        gx = torch.empty_like(x) if need_x else None
        gp = torch.zeros(plan.grad_params_size(), dtype=torch.float32, device=x.device) if need_p else None
        g = grad_out.contiguous()
        if g.dtype != torch.float32:
            g = g.float()
        with torch.cuda.device(x.device):
            if feat is None:
                plan.backward(x, g, gx, gp)
            else:
                gf = torch.empty_like(feat) if need_x else None
                plan.mlp_backward(feat, g, gf, gp)
                if need_x:
                    plan.features_backward(x, gf, gx)
        grads, off = [], 0
        for i, shp in enumerate(ctx.shapes):
            n = 1
            for d in shp:
                n *= d
            grads.append(gp[off:off + n].view(shp) if (need_p and ctx.needs_input_grad[3 + i]) else None)
            off += n
        return (gx, None, None) + tuple(grads)


class _HeadFunction(torch.autograd.Function):
    """The head of a model whose backward is two nodes: the preprocessing's (its own HIP backward), then this one.  For wide fp32
    heads that `Plan.supports_mlp_backward()` accepts where `supports_backward()` does not: forward = `mlp_packed` on the
    features, backward = `mlp_backward` (molann_chain_bwd: grad_f and the parameter gradients on the matrix cores).
    `params` are the Linear weights/biases in layer order; `linears` the modules, repacked before each launch (`sync_mlp`)."""

    @staticmethod
    def forward(ctx, feat, entry, linears, *params):
        plan = entry.plan
        entry.sync_mlp(linears)
        out = torch.empty((feat.shape[0], plan.out_dim), dtype=torch.float32, device=feat.device)
        if feat.shape[0] > 0:
            plan.mlp_packed(feat, out)
        ctx.save_for_backward(feat)
        ctx.entry, ctx.linears, ctx.params = entry, linears, params
        ctx.shapes = [tuple(p.shape) for p in params]
        return out

    @staticmethod
    def backward(ctx, grad_out):
        feat = ctx.saved_tensors[0]
        params = list(ctx.params)
        if torch.is_grad_enabled():
            # create_graph=True: the head rebuilt as ATen ops on the live parameters, differentiated with a graph
            act = _ACT_FNS[ctx.entry.plan.activation]
            wanted = [(0, feat)] if ctx.needs_input_grad[0] else []
            wanted += [(3 + i, p) for i, p in enumerate(params) if ctx.needs_input_grad[3 + i]]
            out = [None] * (3 + len(params))
            if not wanted:
                return tuple(out)
            y, n = feat, len(params) // 2
            for l in range(n):
                y = torch.nn.functional.linear(y, params[2 * l], params[2 * l + 1])
                if l + 1 < n:
                    y = act(y)
            got = torch.autograd.grad(y, [t for _, t in wanted], grad_out, create_graph=True, allow_unused=True)
            for (i, _), gi in zip(wanted, got):
                out[i] = gi
            return tuple(out)
        plan = ctx.entry.plan
        need_f = ctx.needs_input_grad[0]
        need_p = any(ctx.needs_input_grad[3:])
        gf = torch.empty_like(feat) if need_f else None
        gp = torch.zeros(plan.grad_params_size(), dtype=torch.float32, device=feat.device) if need_p else None
        g = grad_out.contiguous()
        if g.dtype != torch.float32:
            g = g.float()
        if feat.shape[0] > 0 and (need_f or need_p):
            with torch.cuda.device(feat.device):
                ctx.entry.sync_mlp(ctx.linears)
                plan.mlp_backward(feat, g, gf, gp)
        elif need_f:
            gf.zero_()
        grads, off = [], 0
        for i, shp in enumerate(ctx.shapes):
            n = 1
            for d in shp:
                n *= d
            grads.append(gp[off:off + n].view(shp) if (need_p and ctx.needs_input_grad[3 + i]) else None)
            off += n
        return (gf, None, None) + tuple(grads)


class _PlanFunction64(torch.autograd.Function):
    """The float64 features of a plan (`model.double()`): forward = molann_features_f64, backward =
    molann_features_backward_f64 (everything recomputed in double from x).  The MLP of a float64 model is torch's."""

    @staticmethod
    def forward(ctx, x, entry):
        out = torch.empty((x.shape[0], entry.plan.feature_dim), dtype=torch.float64, device=x.device)
        entry.plan.features_f64(x, out)
        ctx.save_for_backward(x)
        ctx.entry = entry
        return out

    @staticmethod
    def backward(ctx, grad_out):
        (x,) = ctx.saved_tensors
        g = grad_out.contiguous()
        if g.dtype != torch.float64:
            g = g.double()
        if torch.is_grad_enabled():          # create_graph=True: the same product, as a node that can be differentiated again
            return _FeatBackward64.apply(x, g, ctx.entry), None
        gx = torch.empty_like(x)
        with torch.cuda.device(x.device):
            ctx.entry.plan.features_backward_f64(x, g, gx)
        return gx, None


def _difference_points(x, v):
    """``(x + h v, x - h v, 1 / 2h)`` of the central differences in `_FeatBackward64.backward`, per frame, with the step
    ``h = 6e-6 / |v|_max`` (``h = 0`` and ``1 / 2h = 0`` on a frame where v is zero: its rows stay exactly zero).  A move of
    6e-6 in the coordinates' own unit: the optimum of a second-order formula in double (truncation ~ (h / l)^2, rounding ~
    1e-16 / h) for the length scale l of the geometry - bonds, angles, dihedrals, the aligned set - which is where the
    curvature comes from, not where the frame sits in the box.  (A step that grew with |x|_max gave truncation errors that
    grow like |x|^2: 1e-5 of scale at 100 A from the origin.)  csrc/molann_torch.cpp: FeatBackward64Fn takes the same step."""
    vmax = v.abs().amax(dim=(1, 2), keepdim=True)
    h = torch.where(vmax > 0, 6e-6 / vmax.clamp(min=1e-300), torch.zeros_like(vmax))
    inv = torch.where(h > 0, 0.5 / h.clamp(min=1e-300), torch.zeros_like(h))
    return (x + h * v).contiguous(), (x - h * v).contiguous(), inv


class _FeatBackward64(torch.autograd.Function):
    """``gx = J(x)^T g`` of the float64 features (`molann_features_backward_f64`) as a node that can itself be differentiated -
    what ``create_graph=True`` needs (second-order terms of a loss on forces; the reference gets them from autograd through its
    SVD, `ann.py:188-197`).  For a cotangent ``v`` on ``gx`` its backward needs ``d/dx [v . J(x)^T g]`` and ``d/dg [v . J(x)^T g] = J(x) v``:
    both are directional derivatives along ``v`` - of the first-order kernel's own output and of the features - and one launch of
    `molann_features_hvp_f64` gives both EXACTLY (the float64 backward's closed forms differentiated on a dual number).  Central
    differences of the float64 kernels at the points `_difference_points` gives remain only for a plan that kernel would refuse
    with MOLANN_E_UNSUPPORTED (there is none: every plan the float64 backward serves is covered).  Itself first-order: under
    ``create_graph=True`` its backward raises, as FeatBackward64Fn's does (``once_differentiable`` would not: the error node it
    leaves hangs off detached copies, so ``torch.autograd.grad`` with respect to x prunes it and drops the term in silence)."""

    @staticmethod
    def forward(ctx, x, g, entry):
        gx = torch.empty_like(x)
        with torch.cuda.device(x.device):
            entry.plan.features_backward_f64(x, g, gx)
        ctx.save_for_backward(x, g)
        ctx.entry = entry
        return gx

    @staticmethod
    def backward(ctx, v):
        if torch.is_grad_enabled():
            raise RuntimeError("molann_amd: gradients of order three are not available (the double backward is first-order itself)")
        x, g = ctx.saved_tensors
        plan = ctx.entry.plan
        v = v.contiguous().double()
        hx, hg = torch.empty_like(x), torch.empty_like(g)
        try:
            with torch.cuda.device(x.device):
                plan.features_hvp_f64(x, g, v, hx, hg)
            return (hx if ctx.needs_input_grad[0] else None), (hg if ctx.needs_input_grad[1] else None), None
        except _capi.MolannHipError as e:
            if e.code != _capi.E_UNSUPPORTED:
                raise
        xp, xm, inv = _difference_points(x, v)
        gxp, gxm = torch.empty_like(x), torch.empty_like(x)
        fp = torch.empty((x.shape[0], plan.feature_dim), dtype=torch.float64, device=x.device)
        fm = torch.empty_like(fp)
        with torch.cuda.device(x.device):
            if ctx.needs_input_grad[0]:
                plan.features_backward_f64(xp, g, gxp)
                plan.features_backward_f64(xm, g, gxm)
            if ctx.needs_input_grad[1]:
                plan.features_f64(xp, fp)
                plan.features_f64(xm, fm)
        grad_x = (gxp - gxm) * inv if ctx.needs_input_grad[0] else None
        grad_g = (fp - fm) * inv.view(-1, 1) if ctx.needs_input_grad[1] else None
        return grad_x, grad_g, None


_ACT_FNS = {
    _capi.ACT_TANH: torch.tanh, _capi.ACT_RELU: torch.relu, _capi.ACT_SIGMOID: torch.sigmoid, _capi.ACT_IDENTITY: (lambda t: t),
    _capi.ACT_ELU: torch.nn.functional.elu, _capi.ACT_SILU: torch.nn.functional.silu, _capi.ACT_SOFTPLUS: torch.nn.functional.softplus,
    _capi.ACT_LEAKY_RELU: torch.nn.functional.leaky_relu, _capi.ACT_GELU: torch.nn.functional.gelu,
}


def _double_backward(ctx, grad_out):
    """The gradients of a `_PlanFunction` node as a differentiable composition (create_graph=True): features in float64 through
    `_PlanFunction64` (whose backward is `_FeatBackward64`), the MLP as ATen ops on the live parameters, `torch.autograd.grad`
    with ``create_graph=True`` over it."""
    x = ctx.saved_tensors[0]
    entry, params = ctx.entry, list(ctx.params)
    with torch.enable_grad():
        y = _PlanFunction64.apply(x.double(), entry).to(x.dtype)
        if ctx.with_mlp:
            act = _ACT_FNS[entry.plan.activation]
            n = len(params) // 2
            for l in range(n):
                y = torch.nn.functional.linear(y, params[2 * l], params[2 * l + 1])
                if l + 1 < n:
                    y = act(y)
        wanted = [(0, x)] if ctx.needs_input_grad[0] else []
        wanted += [(3 + i, p) for i, p in enumerate(params) if ctx.needs_input_grad[3 + i]]
        got = torch.autograd.grad(y, [t for _, t in wanted], grad_out, create_graph=True, allow_unused=True) if wanted else ()
    out = [None] * (3 + len(params))
    for (i, _), gi in zip(wanted, got):
        out[i] = gi
    return tuple(out)


# ---- forward mode (torch.autograd.forward_ad, torch.func.jvp / jacfwd / vmap) ----------------------------------------------
# A module's forward takes the path below only when a tangent is present: an input that is a forward-AD dual or a tensor a
# torch.func transform wraps.  Every other call keeps its own path (fast path, operator, ctypes, graphs, scripting) untouched.
def _transform_active():
    """True inside an `fwAD.dual_level()` or a torch.func transform: only then can a tensor carry a tangent."""
    return _fwAD._current_level >= 0 or _functorch.maybe_current_level() is not None


def _has_tangent(t):
    if not isinstance(t, torch.Tensor):
        return False
    if _functorch.is_functorch_wrapped_tensor(t):
        return True
    return _fwAD._current_level >= 0 and _fwAD.unpack_dual(t).tangent is not None


def _refuse_ref_tangent(align_layer):
    if align_layer is not None and _has_tangent(align_layer.ref_x):
        raise RuntimeError("molann_amd: no forward-mode derivative with respect to the alignment reference ref_x (tangents are "
                           "provided for the coordinates x and the ann_layers parameters only)")


def _tangent_input(x):
    """x as the forward-mode kernels read it; raises as `_device_input` does."""
    if not x.is_cuda:
        raise RuntimeError("molann_amd runs on the MI355X only: got a %s tensor (no CPU path; move x and the "
                           "module to a HIP device)" % x.device.type)
    if x.dtype not in (torch.float32, torch.float64):
        raise TypeError("molann_amd kernels are float32 / float64; got %s" % x.dtype)
    return x


class _FeaturesJvp(torch.autograd.Function):
    """The features of a plan where a tangent is present.  forward = molann_features_f32 / _f64 (what the plain path
    computes), backward = molann_features_backward_f32 / _f64 (`_FeaturesVjp`), jvp = the forward-mode kernel
    (`_FeaturesTangent`: frames_jvp_kernel).  New-style (setup_context) and with a vmap rule, so that torch.func can
    transform it."""

    @staticmethod
    def forward(x, entry):
        x = x.contiguous()
        out = torch.empty((x.shape[0], entry.plan.feature_dim), dtype=x.dtype, device=x.device)
        if x.shape[0] > 0:
            with torch.cuda.device(x.device):
                if x.dtype == torch.float64:
                    entry.plan.features_f64(x, out)
                else:
                    entry.plan.features(x, out)
        return out

    @staticmethod
    def setup_context(ctx, inputs, output):
        x, entry = inputs
        ctx.entry = entry
        ctx.save_for_backward(x)
        ctx.save_for_forward(x)

    @staticmethod
    def backward(ctx, grad_out):
        (x,) = ctx.saved_tensors
        return _FeaturesVjp.apply(x, grad_out, ctx.entry), None

    @staticmethod
    def jvp(ctx, x_t, _entry_t):
        (x,) = ctx.saved_tensors
        return _FeaturesTangent.apply(x, x_t, ctx.entry)

    @staticmethod
    def vmap(info, in_dims, x, entry):
        # a batch of x is more frames
        x = x.movedim(in_dims[0], 0)
        b, n = x.shape[0], x.shape[1]
        f = _FeaturesJvp.apply(x.reshape((b * n,) + tuple(x.shape[2:])), entry)
        return f.view(b, n, f.shape[-1]), 0


class _FeaturesTangent(torch.autograd.Function):
    """``J(x) v`` of a plan's features: v is [N, n_inp, 3] or [T, N, n_inp, 3] (T tangents in one launch: one read of x and
    one rotation solve per frame).  Its vmap rule folds a batch of tangents into T and a batch of x into frames, which is
    what torch.func.jacfwd (vmap over jvp) needs.  It is itself first-order: differentiating it again (hessian, reverse over
    forward, forward over forward) raises."""

    @staticmethod
    def forward(x, v, entry):
        one = v.dim() == 3
        v = v.unsqueeze(0) if one else v
        x = x.contiguous()
        v = v.to(x.dtype).contiguous()
        plan = entry.plan
        out = torch.empty((v.shape[0], x.shape[0], plan.feature_dim), dtype=x.dtype, device=x.device)
        if x.shape[0] > 0 and v.shape[0] > 0:
            with torch.cuda.device(x.device):
                if x.dtype == torch.float64:
                    plan.features_jvp_f64(x, v, None, out)
                else:
                    plan.features_jvp(x, v, None, out)
        return out[0] if one else out

    @staticmethod
    def setup_context(ctx, inputs, output):
        pass

    @staticmethod
    def backward(ctx, grad):
        raise RuntimeError("molann_amd: the forward-mode tangent of the features cannot be differentiated again (no derivative "
                           "of J(x) v with respect to x or v: reverse over forward mode and torch.func.hessian are not provided)")

    @staticmethod
    def jvp(ctx, *tangents):
        raise NotImplementedError("molann_amd: nested forward mode (forward over forward) is not provided: the tangent kernel is "
                                  "first-order")

    @staticmethod
    def vmap(info, in_dims, x, v, entry):
        xd, vd, _ = in_dims
        b = info.batch_size
        if xd is None:
            v = v.movedim(vd, 0)                     # [B, N, n, 3] or [B, T, N, n, 3]: B (x T) tangents
            if v.dim() == 4:
                return _FeaturesTangent.apply(x, v, entry), 0
            t = v.shape[1]
            out = _FeaturesTangent.apply(x, v.reshape((b * t,) + tuple(v.shape[2:])), entry)
            return out.view(b, t, out.shape[1], out.shape[2]), 0
        x = x.movedim(xd, 0)                         # a batch of frames: fold it into N
        n = x.shape[1]
        xs = x.reshape((b * n,) + tuple(x.shape[2:]))
        v = v.movedim(vd, 0) if vd is not None else v.expand((b,) + tuple(v.shape))
        if v.dim() == 4:                             # [B, N, n, 3]
            out = _FeaturesTangent.apply(xs, v.reshape(xs.shape), entry)
            return out.view(b, n, out.shape[-1]), 0
        t = v.shape[1]                               # [B, T, N, n, 3] -> [T, B N, n, 3]
        out = _FeaturesTangent.apply(xs, v.transpose(0, 1).reshape((t,) + tuple(xs.shape)), entry)
        return out.view(t, b, n, out.shape[-1]).transpose(0, 1), 0


class _FeaturesVjp(torch.autograd.Function):
    """``J(x)^T g`` of `_FeaturesJvp` through the existing backward kernels, with a vmap rule (torch.func.jacrev).  First-order:
    its own derivatives (create_graph, hessian) raise."""

    @staticmethod
    def forward(x, g, entry):
        x = x.contiguous()
        g = g.to(x.dtype).contiguous()
        gx = torch.empty_like(x)
        if x.shape[0] > 0:
            with torch.cuda.device(x.device):
                if x.dtype == torch.float64:
                    entry.plan.features_backward_f64(x, g, gx)
                else:
                    entry.plan.features_backward(x, g, gx)
        return gx

    @staticmethod
    def setup_context(ctx, inputs, output):
        pass

    @staticmethod
    def backward(ctx, grad):
        raise RuntimeError("molann_amd: second derivatives are not provided where a forward-mode tangent is present "
                           "(torch.func.hessian, create_graph=True on a forward-mode path)")

    @staticmethod
    def jvp(ctx, *tangents):
        raise NotImplementedError("molann_amd: forward over reverse mode (torch.func.hessian) is not provided: it needs the "
                                  "derivative of the features' backward")

    @staticmethod
    def vmap(info, in_dims, x, g, entry):
        b = info.batch_size
        x = x.movedim(in_dims[0], 0) if in_dims[0] is not None else x.expand((b,) + tuple(x.shape))
        g = g.movedim(in_dims[1], 0) if in_dims[1] is not None else g.expand((b,) + tuple(g.shape))
        n = x.shape[1]
        gx = _FeaturesVjp.apply(x.reshape((b * n,) + tuple(x.shape[2:])), g.reshape(b * n, g.shape[-1]), entry)
        return gx.view(x.shape), 0


def _device_buffer(ref_x, x):
    """The module's `ref_x` buffer must live where x lives and have its dtype (the reference's matmul, ann.py:187,
    raises RuntimeError for mixed devices and for mixed dtypes too)."""
    if ref_x.device != x.device:
        raise RuntimeError("Expected all tensors to be on the same device: ref_x is on %s, x on %s "
                           "(move the module with .to(x.device))" % (ref_x.device, x.device))
    if ref_x.dtype != x.dtype:
        raise RuntimeError("expected ref_x and x to have the same dtype, but got ref_x %s and x %s (call .double() / "
                           ".float() on the module)" % (ref_x.dtype, x.dtype))
    return ref_x


class _PlanOwner(object):
    """Mixin: per-device cache of C-ABI plans, dropped on copy / pickling (plans hold device memory)."""

    def _plans(self):
        cache = self.__dict__.get("_plan_cache")
        if cache is None:
            cache = {}
            self.__dict__["_plan_cache"] = cache
        return cache

    def refresh_parameters(self):
        """Re-read `ref_x` and the Linear parameters at the next forward.  Needed only after writing them in a way
        their version counters do not show (`p.data.mul_()`, `p.data.copy_()`, a detached alias): ordinary in-place
        ops, optimizer steps, load_state_dict, .to() and replaced Parameters are seen without it."""
        for e in self._plans().values():
            if isinstance(e, _PlanEntry):
                e.invalidate()
        st = self.__dict__.get("_fast")
        if st is not None and st.get("desc") is not None and st.get("op") is not None:
            torch.ops.molann.invalidate(st["desc"], st["sig"][5])
        for m in self.children():
            if isinstance(m, _PlanOwner):
                m.refresh_parameters()

    def __getstate__(self):
        state = dict(self.__dict__)
        state.pop("_plan_cache", None)
        state.pop("_fast", None)
        state.pop("_fp", None)
        state.pop("_flat_key", None)
        state.pop("_sigma_key", None)
        return state

    def __deepcopy__(self, memo):
        import copy
        cls = self.__class__
        new = cls.__new__(cls)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            if k not in ("_plan_cache", "_fast", "_fp", "_flat_key", "_sigma_key"):
                new.__dict__[k] = copy.deepcopy(v, memo)
        return new


class _TensorKey(object):
    """Which tensor was packed: the OBJECT (weak reference: an address the allocator reuses cannot pass for it), its
    storage address and its version counter.  In-place writes through `.data` bump neither: `refresh_parameters()`."""
    __slots__ = ("ref", "ptr", "version")

    def __init__(self, t):
        import weakref
        self.ref, self.ptr, self.version = weakref.ref(t), t.data_ptr(), t._version

    def matches(self, t):
        return self.ref() is t and self.ptr == t.data_ptr() and self.version == t._version


class _PrefixKey(object):
    """Which rows of a table were checked: the `_TensorKey` of the tensor that owns the storage (the table itself for a view such as
    ``table[:h]``, whose version counter every view shares) and the checked view's address and size.  A later view of the same table
    from the same address with no more elements matches until the table is written to - a caller that appends a row writes to it."""
    __slots__ = ("base", "ptr", "numel")

    @staticmethod
    def _owner(t):
        return t._base if t._base is not None else t

    def __init__(self, t):
        self.base, self.ptr, self.numel = _TensorKey(self._owner(t)), t.data_ptr(), t.numel()

    def matches(self, t):
        return self.base.matches(self._owner(t)) and self.ptr == t.data_ptr() and t.numel() <= self.numel


class _PlanEntry(object):
    """A plan plus the versions of the live tensors (ref_x buffer, Linear parameters) packed in it."""

    def __init__(self, plan):
        self.plan = plan
        self.ref_key = None
        self.mlp_key = None
        self._bwd_kind = None

    def backward_kind(self):
        if self._bwd_kind is None:
            self._bwd_kind = self.plan.backward_kind()     # a property of the plan: asked (and built) once
        return self._bwd_kind

    def invalidate(self):
        self.ref_key = self.mlp_key = None

    def sync_ref(self, ref_x):
        if self.ref_key is None or not self.ref_key.matches(ref_x):
            if ref_x.dtype == torch.float64:      # the buffer of a `.double()` model: kept in double
                r = ref_x.contiguous()
                self.plan.update_ref_f64(r)
            else:
                r = ref_x if (ref_x.dtype == torch.float32 and ref_x.is_contiguous()) else ref_x.float().contiguous()
                self.plan.update_ref(r)
            self.ref_key = _TensorKey(ref_x)
            self._ref_hold = r

    def sync_mlp(self, linears):
        params = [p for lin in linears for p in (lin.weight, lin.bias)]
        if self.mlp_key is None or len(self.mlp_key) != len(params) or \
                not all(k.matches(p) for k, p in zip(self.mlp_key, params)):
            ws = [lin.weight.detach().contiguous() for lin in linears]
            bs = [lin.bias.detach().contiguous() for lin in linears]
            self.plan.update_mlp(ws, bs)
            self.mlp_key = [_TensorKey(p) for p in params]


def _feature_spec(feature_layer_or_map):
    maps = feature_layer_or_map.feature_map_list if isinstance(feature_layer_or_map, FeatureLayer) else [feature_layer_or_map]
    spec = [(fm.type_id, list(fm._local_atom_indices)) for fm in maps]
    uav = bool(maps[0].use_angle_value)
    return spec, uav


def _get_entry(owner, x, tag, build):
    key = (tag, x.device.index)
    cache = owner._plans()
    entry = cache.get(key)
    if entry is None:
        with torch.cuda.device(x.device):
            entry = _PlanEntry(build())
        cache[key] = entry
    return entry


def last_launch_info(module):
    """Launch info of the plan a molann_amd module used last ('' before its first forward)."""
    if isinstance(module, MolANN) and module.__dict__.get("_fast", {}).get("op") is not None:
        return module.last_launch_info()
    cache = module._plans()
    entries = [e for e in cache.values() if isinstance(e, _PlanEntry)]
    return entries[-1].plan.last_launch_info() if entries else ""


class AlignmentLayer(_PlanOwner, torch.nn.Module):
    r"""Kabsch superposition of every frame onto the (centred) coordinates of ``align_atom_group``:
    :math:`x \mapsto (x - c(x)) R(x)`, all ``n_inp`` atoms returned (`ann.py:157-199`)."""

    def __init__(self, align_atom_group, input_atom_group):
        super(AlignmentLayer, self).__init__()
        self.align_atom_indices = align_atom_group.ix.tolist()
        self.input_atom_indices = input_atom_group.ix.tolist()
        self.input_atom_num = len(input_atom_group)
        ref_x = torch.from_numpy(align_atom_group.positions)
        self.register_buffer('ref_x', ref_x)
        self.ref_x = self.ref_x - torch.mean(self.ref_x, 0)       # centred once (ann.py:140-141)
        self._local_align_atom_indices = _local_indices(self.input_atom_indices, self.align_atom_indices,
                                                        "Atoms used for alignment must be among the input")

    def show_info(self):
        print(f'\n{self.input_atom_num} atoms used for input, (0-based) global indices: \n', self.input_atom_indices)
        print(f'\n{len(self._local_align_atom_indices)} atoms used for alignment, with (0-based) global indices: \n',
              self.align_atom_indices)
        print('local indices\n', self._local_align_atom_indices)
        print('\ncoordinates of reference state used in aligment:\n', self.ref_x.cpu().numpy())

    def __prepare_scriptable__(self):
        """`torch.jit.script(align)` (`test/test_molann.py:46`) compiles this instead, see molann_amd/script.py."""
        from . import script
        return script.ScriptPlan(script.make_desc(script.KIND_ALIGN, self.input_atom_num,
                                                  align_idx=self._local_align_atom_indices), ref_x=self.ref_x)

    def _entry(self, x):
        entry = _get_entry(self, x, "align", lambda: _capi.Plan(
            self.input_atom_num, align_idx=self._local_align_atom_indices, ref_x=self.ref_x))
        entry.sync_ref(_device_buffer(self.ref_x, x))
        return entry

    def forward(self, x):
        _check_input(x, self.input_atom_num)
        tangent = _transform_active() and (_has_tangent(x) or _has_tangent(self.ref_x))
        x = _tangent_input(x) if tangent else _device_input(x, backward_ok=True)

        def build():   # the aligned frame == alignment + one position item per atom: that plan has backward and tangent kernels
            return _capi.Plan(self.input_atom_num, align_idx=self._local_align_atom_indices, ref_x=self.ref_x,
                              features=[(_capi.FEAT_POSITION, list(range(self.input_atom_num)))])
        if tangent:
            _refuse_ref_tangent(self)
            entry = _get_entry(self, x, "align_grad", build)
            with torch.cuda.device(x.device):
                entry.sync_ref(_device_buffer(self.ref_x, x))
            return _FeaturesJvp.apply(x, entry).view(x.shape[0], self.input_atom_num, 3)
        if x.shape[0] == 0:
            return torch.empty_like(x)
        if _wants_grad(x):
            entry = _get_entry(self, x, "align_grad", build)
            with torch.cuda.device(x.device):
                entry.sync_ref(_device_buffer(self.ref_x, x))
                if x.dtype == torch.float64:
                    return _PlanFunction64.apply(x, entry).view(x.shape[0], self.input_atom_num, 3)
                if not entry.plan.supports_backward():
                    raise NotImplementedError("no backward kernel for this alignment plan (large frames): use torch.no_grad()")
                return _PlanFunction.apply(x, entry, False).view(x.shape[0], self.input_atom_num, 3)
        out = torch.empty_like(x)
        with torch.cuda.device(x.device):
            plan = self._entry(x).plan
            if x.dtype == torch.float64:
                plan.align_f64(x, out)
            else:
                plan.align(x, out)
        return out


class FeatureMap(_PlanOwner, torch.nn.Module):
    """One feature (angle / bond / dihedral / position) of every frame (`ann.py:288-356`)."""

    def __init__(self, feature, input_atom_group, use_angle_value=False):
        super(FeatureMap, self).__init__()
        self.feature = feature
        self.type_id = feature.get_type_id()
        self.use_angle_value = use_angle_value
        self.input_atom_indices = input_atom_group.ix.tolist()
        self.input_atom_num = len(input_atom_group)
        self._local_atom_indices = _local_indices(self.input_atom_indices, feature.get_atom_indices() - 1,
                                                  "Atoms used in feature must be among the input")

    def dim(self):
        """1 for angle / bond / dihedral value, 2 for dihedral (cos, sin), 3k for k positions."""
        if self.type_id in (0, 1):
            return 1
        if self.type_id == 2:
            return 1 if self.use_angle_value == True else 2  # noqa: E712 (mirrors the reference's comparison)
        if self.type_id == 3:
            return 3 * len(self.feature.get_atom_indices())
        return 0

    def forward(self, x):
        _check_input(x, self.input_atom_num)
        return _run_features(self, x, None)

    def __prepare_scriptable__(self):
        return _script_features(self, None)


class FeatureLayer(_PlanOwner, torch.nn.Module):
    """All features of a list, concatenated column-wise in list order (`ann.py:454-474`)."""

    def __init__(self, feature_list, input_atom_group, use_angle_value=False):
        super(FeatureLayer, self).__init__()
        assert len(feature_list) > 0, 'Error: feature list is empty!'
        self.feature_list = feature_list
        self.feature_map_list = torch.nn.ModuleList([FeatureMap(f, input_atom_group, use_angle_value) for f in feature_list])
        self.input_atom_num = len(input_atom_group)

    def get_feature_info(self):
        return pd.concat([f.get_feature_info() for f in self.feature_list], ignore_index=True)

    def get_feature(self, idx):
        return self.feature_list[idx]

    def output_dimension(self):
        return sum([f_map.dim() for f_map in self.feature_map_list])

    def forward(self, x):
        _check_input(x, self.input_atom_num)
        return _run_features(self, x, None)

    def __prepare_scriptable__(self):
        return _script_features(self, None)


def _script_features(feature_owner, align_layer):
    """The ScriptPlan of a FeatureMap / FeatureLayer, optionally behind an AlignmentLayer."""
    from . import script
    spec, uav = _feature_spec(feature_owner)
    if align_layer is None:
        return script.ScriptPlan(script.make_desc(script.KIND_FEATURES, feature_owner.input_atom_num, features=spec,
                                                  use_angle_value=uav))
    return script.ScriptPlan(script.make_desc(script.KIND_FEATURES, feature_owner.input_atom_num,
                                              align_idx=align_layer._local_align_atom_indices, features=spec,
                                              use_angle_value=uav), ref_x=align_layer.ref_x)


def _run_features(feature_owner, x, align_layer, plan_owner=None):
    """features (optionally of the aligned frame) through one fused launch."""
    tangent = _transform_active() and (_has_tangent(x) or (align_layer is not None and _has_tangent(align_layer.ref_x)))
    if tangent:
        _refuse_ref_tangent(align_layer)
        x = _tangent_input(x)
    else:
        x = _device_input(x, backward_ok=True)
    spec, uav = _feature_spec(feature_owner)
    owner = plan_owner if plan_owner is not None else feature_owner

    def build():
        if align_layer is None:
            return _capi.Plan(feature_owner.input_atom_num, features=spec, use_angle_value=uav)
        return _capi.Plan(feature_owner.input_atom_num, align_idx=align_layer._local_align_atom_indices,
                          ref_x=align_layer.ref_x, features=spec, use_angle_value=uav)

    entry = _get_entry(owner, x, "features", build)
    if tangent:
        with torch.cuda.device(x.device):
            if align_layer is not None:
                entry.sync_ref(_device_buffer(align_layer.ref_x, x))
        return _FeaturesJvp.apply(x, entry)
    if x.shape[0] == 0:
        return torch.empty((0, entry.plan.feature_dim), dtype=x.dtype, device=x.device)
    if x.dtype == torch.float64:
        with torch.cuda.device(x.device):
            if align_layer is not None:
                entry.sync_ref(_device_buffer(align_layer.ref_x, x))
            if _wants_grad(x):
                return _PlanFunction64.apply(x, entry)
            out = torch.empty((x.shape[0], entry.plan.feature_dim), dtype=torch.float64, device=x.device)
            entry.plan.features_f64(x, out)
        return out
    with torch.cuda.device(x.device):
        if align_layer is not None:
            entry.sync_ref(_device_buffer(align_layer.ref_x, x))
        if _wants_grad(x):
            if not entry.plan.supports_backward():
                raise NotImplementedError("no backward kernel for this plan (large frames): use torch.no_grad()")
            return _PlanFunction.apply(x, entry, False)
        out = torch.empty((x.shape[0], entry.plan.feature_dim), dtype=torch.float32, device=x.device)
        entry.plan.features(x, out)
    return out


# ---- The calls that give the values and a derivative in one launch: MolANN.value_and_vjp / value_and_jacobian / value_and_metric /
# value_and_restraint / value_and_hills / value_and_grid / value_and_bias and PreprocessingANN.value_and_metric / value_and_restraint /
# value_and_hills / value_and_grid / value_and_bias, and value_and_opes and value_and_opes_table of both.  What differs
# between them, by kind; the checks and the two ways to the kernel are written once below.
_VJP, _JACOBIAN, _METRIC, _RESTRAINT, _HILLS, _GRID, _BIAS, _OPES, _BIAS_OPES, _OPES_TABLE, _BIAS_OPES_TABLE = 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10
_PBMETAD = 11             # value_and_pbmetad: K one-dimensional tables joined by a soft minimum (a kernel of its own)
_HILLS_MAX_D_OUT = 8      # HILLS64_MAX_D_OUT of csrc/molann_value_f64.inc: the kernel's cotangent sums are a register array
_JACOBIAN_ROUTE = "use value_and_vjp on x.expand(d_out, -1, -1) with torch.eye(d_out) as cotangent"
_METRIC_ROUTE = 'use value_and_jacobian and torch.einsum("fkai,a,flai->fkl", jac, w, jac)'
_RESTRAINT_ROUTE = "use `model(x)`, form `kappa * d` and the energy with torch, then `value_and_vjp`"
_RESTRAINT_FEATURES_ROUTE = "use `module(x)` on an x that requires grad, form the energy with torch and take torch.autograd.grad"
_HILLS_ROUTE = "use `model(x)`, form the hill sum and its derivative with torch, then `value_and_vjp`"
_HILLS_FEATURES_ROUTE = "use `module(x)` on an x that requires grad, form the hill sum with torch and take torch.autograd.grad"
_GRID_MAX_D_OUT = 3       # GRID64_MAX_D_OUT of csrc/molann_value_f64.inc: the table has one axis per output
_GRID_ROUTE = "use `model(x)`, interpolate the table and its derivative with torch, then `value_and_vjp`"
_GRID_FEATURES_ROUTE = "use `module(x)` on an x that requires grad, interpolate the table with torch and take torch.autograd.grad"
_BIAS_ROUTE = "use `model(x)`, form the terms and their derivatives on the chosen columns with torch, then `value_and_vjp`"
_BIAS_FEATURES_ROUTE = "use `module(x)` on an x that requires grad, form the terms with torch and take torch.autograd.grad"
_OPES_ROUTE = "use `model(x)`, form the kernel sum with `molann_amd.bias.opes_kernel_sum`, its logarithm and its derivative with torch, then `value_and_vjp`"
_OPES_FEATURES_ROUTE = ("use `module(x)` on an x that requires grad, form the kernel sum with `molann_amd.bias.opes_kernel_sum` and its logarithm with "
                        "torch and take torch.autograd.grad")
# value_and_bias with an OPES term (_BIAS_OPES, a kernel of its own): what remains where it refuses
_BIAS_OPES_ROUTE = ("use `model(x)`, form the walls and the table on the chosen columns and the kernel sum with `molann_amd.bias.opes_kernel_sum`, "
                    "their derivatives with torch, then `value_and_vjp`")
_BIAS_OPES_FEATURES_ROUTE = ("use `module(x)` on an x that requires grad, form the walls, the table and the kernel sum "
                             "(`molann_amd.bias.opes_kernel_sum`) with torch and take torch.autograd.grad")
_HILLS_AND_OPES_ROUTE = ("`hills` and `opes` in one launch are not served: move the hills onto a table with `molann_amd.bias.add_hills_to_grid` and "
                         "pass it as `grid`, or make two calls (`value_and_bias` with the hills, `value_and_opes` or `value_and_bias` with `opes`) "
                         "and add their dx")
# value_and_opes_table (_OPES_TABLE): value_and_opes on an `OpesTable` whose state the kernel reads; what remains where it refuses
_OPES_TABLE_ROUTE = "read the table's state (`OpesTable.read_state`), then `value_and_opes` on `table.record(scale, S / n, epsilon)`, or: " + _OPES_ROUTE
_OPES_TABLE_FEATURES_ROUTE = ("read the table's state (`OpesTable.read_state`), then `value_and_opes` on `table.record(scale, S / n, epsilon)`, or: "
                              + _OPES_FEATURES_ROUTE)
# value_and_bias with an `OpesFromTable` (_BIAS_OPES_TABLE, a kernel of its own that reads the table's state): what remains where it refuses
_BIAS_OPES_TABLE_ROUTE = ("read the table's state (`OpesTable.read_state`), then `value_and_bias(opes=table.record(scale, S / n, epsilon, columns))`, "
                          "or: " + _BIAS_OPES_ROUTE)
_BIAS_OPES_TABLE_FEATURES_ROUTE = ("read the table's state (`OpesTable.read_state`), then `value_and_bias(opes=table.record(scale, S / n, epsilon, "
                                   "columns))`, or: " + _BIAS_OPES_FEATURES_ROUTE)
# value_and_pbmetad (_PBMETAD): what remains where it refuses
_PBMETAD_ROUTE = ("use `model(x)`, interpolate the K tables and their derivatives on `y[:, columns]` with torch, form the soft minimum "
                  "`-kT logsumexp(-V / kT)` and its weights, scatter `w_k V_k'` into a cotangent, then `value_and_vjp`")
_PBMETAD_FEATURES_ROUTE = ("use `module(x)` on an x that requires grad, interpolate the K tables with torch, form the soft minimum "
                           "`-kT logsumexp(-V / kT)` and take torch.autograd.grad")
_ONE_LAUNCH_NAME = ("value_and_vjp", "value_and_jacobian", "value_and_metric", "value_and_restraint", "value_and_hills", "value_and_grid",
                    "value_and_bias", "value_and_opes", "value_and_bias", "value_and_opes_table", "value_and_bias", "value_and_pbmetad")
# the route that remains where the call refuses
_ONE_LAUNCH_ROUTE = (None, _JACOBIAN_ROUTE, _METRIC_ROUTE, _RESTRAINT_ROUTE, _HILLS_ROUTE, _GRID_ROUTE, _BIAS_ROUTE, _OPES_ROUTE, _BIAS_OPES_ROUTE,
                     _OPES_TABLE_ROUTE, _BIAS_OPES_TABLE_ROUTE, _PBMETAD_ROUTE)
_ONE_LAUNCH_FEATURES_ROUTE = (None, None, None, _RESTRAINT_FEATURES_ROUTE, _HILLS_FEATURES_ROUTE, _GRID_FEATURES_ROUTE, _BIAS_FEATURES_ROUTE,
                              _OPES_FEATURES_ROUTE, _BIAS_OPES_FEATURES_ROUTE, _OPES_TABLE_FEATURES_ROUTE, _BIAS_OPES_TABLE_FEATURES_ROUTE,
                              _PBMETAD_FEATURES_ROUTE)
_ONE_LAUNCH_PAIR = ("(y, dx)", "(y, jac)", "(y, M)", "(y, energy, dx)", "(y, bias, dx)", "(y, bias, dx)", "(y, energies, dx)", "(y, bias, dx)",
                    "(y, energies, dx)", "(y, bias, dx)", "(y, energies, dx)", "(y, energies, dx)")   # what `into` holds
# the dispatcher operator, in MolANN._fast_state
_ONE_LAUNCH_OP = ("op_vjp", "op_jacobian", "op_metric", "op_restraint", "op_hills", "op_grid", "op_bias", "op_opes", "op_bias_opes", "op_opes_table",
                  "op_bias_opes_table", "op_pbmetad")
_BIAS_KINDS = (_RESTRAINT, _HILLS, _GRID)      # the calls that return (y, a scalar per frame, dx)


def _check_into(name, x, into, dtype, out_dim, second_shape, pair):
    """`into` of a one-launch call, before any launch: a pair of contiguous tensors of `dtype` on x's device that hold [N, out_dim]
    and `second_shape`'s elements.  Returns the pair, (None, None) for None."""
    if into is None:
        return None, None
    if len(into) != 2 or not all(isinstance(t, torch.Tensor) for t in into):
        raise TypeError("%s: `into` must be a pair of tensors %s" % (name, pair))
    y, second = into
    if y.dtype != dtype or second.dtype != dtype:
        raise TypeError("%s: `into` must be %s like x; got %s, %s" % (name, str(dtype)[6:], y.dtype, second.dtype))
    if not (y.is_contiguous() and second.is_contiguous()) or y.numel() != x.shape[0] * out_dim or second.numel() != math.prod(second_shape) \
            or y.device != x.device or second.device != x.device:
        raise ValueError("%s: `into` must be contiguous {[%d, %d], %s} on %s" % (name, x.shape[0], out_dim, list(second_shape), x.device))
    return y, second


def _check_into_triple(name, x, into, out_dim, kind=_RESTRAINT, width=None):
    """`into` of value_and_restraint, value_and_hills and value_and_grid, before any launch, with `_check_into`'s checks: a triple of contiguous float64 tensors on x's
    device that hold [N, out_dim], [N] ([N, 3] for value_and_bias, [N, 4] with an OPES term) and x's elements.  Returns the triple, (None, None, None) for None."""
    if into is None:
        return None, None, None
    if len(into) != 3 or not all(isinstance(t, torch.Tensor) for t in into):
        raise TypeError("%s: `into` must be a triple of tensors %s" % (name, _ONE_LAUNCH_PAIR[kind]))
    if any(t.dtype != torch.float64 for t in into):
        raise TypeError("%s: `into` must be float64 like x; got %s" % (name, ", ".join(str(t.dtype) for t in into)))
    n = x.shape[0]
    per = 3 if kind == _BIAS else 4 if kind in (_BIAS_OPES, _BIAS_OPES_TABLE) else width if kind == _PBMETAD else 1
    counts = (n * out_dim, n * per, x.numel())
    if not all(t.is_contiguous() and t.numel() == c and t.device == x.device for t, c in zip(into, counts)):
        raise ValueError("%s: `into` must be contiguous {[%d, %d], %s, %s} on %s"
                         % (name, n, out_dim, [n, per] if per > 1 else [n], list(x.shape), x.device))
    return tuple(into)


def _restraint_row(name, what, v, x, shapes):
    """One argument of value_and_restraint on its way to what the kernel reads (float64, contiguous, on x's device, of one of
    `shapes`): a float64 tensor on x's device passes as it is; a tensor of another floating dtype, a number (filling the row) or a
    sequence will be converted, which costs a launch.  This is the check: `_check_restraint_args` converts after all of them."""
    if isinstance(v, torch.Tensor):
        if not v.dtype.is_floating_point:
            raise TypeError("%s: `%s` must be a floating-point tensor; got %s" % (name, what, v.dtype))
        if v.device != x.device:
            raise ValueError("%s: `%s` must be on %s; got %s" % (name, what, x.device, v.device))
        t = v.detach()
    elif isinstance(v, (int, float)) and not isinstance(v, bool):
        t = torch.full(shapes[0], float(v), dtype=torch.float64)
    else:
        try:
            t = torch.as_tensor(v, dtype=torch.float64)
        except (TypeError, ValueError, RuntimeError):
            raise TypeError("%s: `%s` must be a tensor, a number or a sequence of numbers; got %s" % (name, what, type(v).__name__))
    if tuple(t.shape) not in shapes:
        raise ValueError("%s: `%s` must have shape %s; got %s" % (name, what, " or ".join(str(list(sh)) for sh in shapes), list(t.shape)))
    return t


def _check_restraint_args(name, x, out_dim, center, kappa, period, flat, into, owner=None):
    """The `center`, `kappa`, `period`, `flat` and `into` checks of value_and_restraint, all before any launch on x's device; returns
    (center, kappa, period, flat, y, energy, dx) as the kernel takes them (None where they are).  A negative `flat` is a ValueError:
    host values are looked at as they are, a device tensor is read back once and remembered on `owner` until it is written to."""
    n = x.shape[0]
    rows = [_restraint_row(name, "center", center, x, ((out_dim,), (n, out_dim))),
            _restraint_row(name, "kappa", kappa, x, ((out_dim,),)),
            None if period is None else _restraint_row(name, "period", period, x, ((out_dim,),)),
            None if flat is None else _restraint_row(name, "flat", flat, x, ((out_dim,),))]
    if flat is not None:
        key = owner.__dict__.get("_flat_key") if owner is not None and isinstance(flat, torch.Tensor) else None
        if key is None or not key.matches(flat):
            if bool((rows[3] < 0).any()):
                raise ValueError("%s: `flat` holds the half-widths of the flat bottoms and must not be negative" % name)
            if owner is not None and isinstance(flat, torch.Tensor) and flat.is_cuda:
                owner.__dict__["_flat_key"] = _TensorKey(flat)
    triple = _check_into_triple(name, x, into, out_dim)
    rows = [t if t is None or (t.dtype == torch.float64 and t.device == x.device and t.is_contiguous())
            else t.to(device=x.device, dtype=torch.float64).contiguous() for t in rows]
    return tuple(rows) + triple


def _check_hills_args(name, x, out_dim, centers, heights, sigma, period, into, owner=None, unit="output"):
    """The `centers`, `heights`, `sigma`, `period` and `into` checks of value_and_hills, all before any launch on x's device, with
    `_restraint_row`'s rules for what passes as it is and what is converted; returns (centers, heights, sigma, period, y, bias, dx) as
    the kernel takes them (None where they are).  More than 8 outputs: NotImplementedError.  The number of hills H is centers' first
    dimension and may be 0.  A `sigma` that is not > 0 everywhere (a NaN too) is a ValueError: host values are looked at as they are, a
    device tensor is read back once and remembered on `owner` until it - or, for a view like ``table[:h]``, the table it is a view
    of - is written to (`_PrefixKey`)."""
    if out_dim > _HILLS_MAX_D_OUT:
        raise NotImplementedError("%s: the one-launch kernel serves at most %d %ss (got %d); %s" % (name, _HILLS_MAX_D_OUT, unit, out_dim, _HILLS_ROUTE))
    if isinstance(centers, torch.Tensor):
        n_hills = centers.shape[0] if centers.dim() == 2 else 0
    elif hasattr(centers, "__len__"):
        n_hills = len(centers)
    else:
        raise TypeError("%s: `centers` must be a tensor or a sequence of rows [H, %d] (one column per %s); got %s" % (name, out_dim, unit, type(centers).__name__))
    if not isinstance(centers, torch.Tensor) and n_hills == 0:
        centers = torch.empty((0, out_dim), dtype=torch.float64)
    rows = [_restraint_row(name, "centers", centers, x, ((n_hills, out_dim),)),
            _restraint_row(name, "heights", heights, x, ((n_hills,),)),
            _restraint_row(name, "sigma", sigma, x, ((out_dim,), (n_hills, out_dim))),
            None if period is None else _restraint_row(name, "period", period, x, ((out_dim,),))]
    key = owner.__dict__.get("_sigma_key") if owner is not None and isinstance(sigma, torch.Tensor) else None
    if key is None or not key.matches(sigma):
        if not bool((rows[2] > 0).all()):
            raise ValueError("%s: `sigma` holds the hills' widths and must be > 0 everywhere" % name)
        if owner is not None and isinstance(sigma, torch.Tensor) and sigma.is_cuda:
            owner.__dict__["_sigma_key"] = _PrefixKey(sigma)
    triple = _check_into_triple(name, x, into, out_dim, _HILLS)
    rows = [t if t is None or (t.dtype == torch.float64 and t.device == x.device and t.is_contiguous())
            else t.to(device=x.device, dtype=torch.float64).contiguous() for t in rows]
    return tuple(rows) + triple


def _check_opes_args(name, x, out_dim, centers, heights, sigma, scale, norm, epsilon, cutoff, period, into, owner=None):
    """The checks of value_and_opes, all before any launch on x's device: the four scalars as Python numbers (`scale` finite, `norm` and
    `epsilon` finite and > 0, `cutoff` None - no cutoff, passed on as +inf - or > 0 and not NaN: ValueError; anything that is no number:
    TypeError), more than 8 outputs (NotImplementedError naming the route), then `_check_hills_args` on the table, the widths, the period
    and `into`.  Returns (centers, heights, sigma, period, scale, norm, epsilon, cutoff, y, bias, dx) as the kernel takes them."""
    vals = []
    for what, v in (("scale", scale), ("norm", norm), ("epsilon", epsilon), ("cutoff", math.inf if cutoff is None else cutoff)):
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise TypeError("%s: `%s` must be a Python float%s; got %s" % (name, what, " or None" if what == "cutoff" else "", type(v).__name__))
        vals.append(float(v))
    scale, norm, epsilon, cutoff = vals
    if not math.isfinite(scale):
        raise ValueError("%s: `scale` must be finite; got %r" % (name, scale))
    for what, v in (("norm", norm), ("epsilon", epsilon)):
        if not (math.isfinite(v) and v > 0.0):
            raise ValueError("%s: `%s` must be finite and > 0; got %r" % (name, what, v))
    if not cutoff > 0.0:
        raise ValueError("%s: `cutoff` must be None (no cutoff) or > 0; got %r" % (name, cutoff))
    if out_dim > _HILLS_MAX_D_OUT:
        raise NotImplementedError("%s: the one-launch kernel serves at most %d outputs (got %d); %s" % (name, _HILLS_MAX_D_OUT, out_dim, _OPES_ROUTE))
    checked = _check_hills_args(name, x, out_dim, centers, heights, sigma, period, into, owner=owner)
    return checked[:4] + (scale, norm, epsilon, cutoff) + checked[4:]


def _check_opes_table_args(name, x, out_dim, table, scale, epsilon, into, owner=None):
    """The checks of value_and_opes_table, all before any launch on x's device and with nothing read back: `table` a
    `molann_amd.bias.OpesTable` (TypeError) with ``table.d == out_dim`` on x's device (ValueError), `scale` and `epsilon` as
    `_check_opes_args` takes them, more than 8 outputs (NotImplementedError naming the route), `into`.  The widths are not looked at: they
    are the deposits' and live in device memory.  Returns (centers, heights, sigma, state, period, scale, epsilon, cutoff, y, bias, dx) as
    the kernel takes them, the cutoff and the period being the table's."""
    if not isinstance(table, _bias.OpesTable):
        raise TypeError("%s: `table` must be a molann_amd.bias.OpesTable; got %s" % (name, type(table).__name__))
    vals = []
    for what, v in (("scale", scale), ("epsilon", epsilon)):
        if isinstance(v, bool) or not isinstance(v, (int, float)):
            raise TypeError("%s: `%s` must be a Python float; got %s" % (name, what, type(v).__name__))
        vals.append(float(v))
    scale, epsilon = vals
    if not math.isfinite(scale):
        raise ValueError("%s: `scale` must be finite; got %r" % (name, scale))
    if not (math.isfinite(epsilon) and epsilon > 0.0):
        raise ValueError("%s: `epsilon` must be finite and > 0; got %r" % (name, epsilon))
    if out_dim > _HILLS_MAX_D_OUT:
        raise NotImplementedError("%s: the one-launch kernel serves at most %d outputs (got %d); %s" % (name, _HILLS_MAX_D_OUT, out_dim, _OPES_ROUTE))
    if table.d != out_dim:
        raise ValueError("%s: `table` holds kernels of %d columns but the model has %d outputs" % (name, table.d, out_dim))
    if table.centers.device != x.device:
        raise ValueError("%s: `table` must be on %s; got %s" % (name, x.device, table.centers.device))
    triple = _check_into_triple(name, x, into, out_dim, _HILLS)
    return (table.centers, table.heights, table.sigma, table.state, table.period, scale, epsilon,
            math.inf if table.cutoff is None else table.cutoff) + triple


def _grid_floats(name, what, v, out_dim, unit="output"):
    """`lower` or `spacing` of value_and_grid: a sequence, or a CPU tensor, of out_dim numbers, as a list of floats."""
    if isinstance(v, torch.Tensor):
        if v.device.type != "cpu":
            raise ValueError("%s: `%s` holds host values: a sequence or a CPU tensor of %d floats; got a tensor on %s" % (name, what, out_dim, v.device))
        v = v.reshape(-1).tolist() if v.dim() <= 1 else v
    try:
        vals = [float(t) for t in v]
    except (TypeError, ValueError, RuntimeError):
        raise TypeError("%s: `%s` must be a sequence or a CPU tensor of %d floats; got %s" % (name, what, out_dim, type(v).__name__))
    if len(vals) != out_dim:
        raise ValueError("%s: `%s` must hold one value per %s (%d); got %d" % (name, what, unit, out_dim, len(vals)))
    return vals


def _check_grid_args(name, x, out_dim, table, lower, spacing, periodic, into, owner=None, unit="output"):
    """The `table`, `lower`, `spacing`, `periodic` and `into` checks of value_and_grid, all before any launch on x's device; returns
    (table, lower, spacing, periodic, y, bias, dx) as the kernel takes them: the table as it is, three lists of out_dim host values
    (`periodic` all False for None), y, bias, dx None without `into`.  More than 3 outputs: NotImplementedError.  Nothing is
    converted: a table that is not float64, contiguous, on x's device, with one dimension of at least 4 points per output is an
    error, and so is a spacing that is not finite and > 0 or a lower that is not finite."""
    if out_dim > _GRID_MAX_D_OUT:
        raise NotImplementedError("%s: the one-launch kernel serves at most %d %ss (got %d); %s" % (name, _GRID_MAX_D_OUT, unit, out_dim, _GRID_ROUTE))
    if not isinstance(table, torch.Tensor):
        raise TypeError("%s: `table` must be a float64 tensor with one dimension per %s; got %s" % (name, unit, type(table).__name__))
    if table.dtype != torch.float64:
        raise TypeError("%s: `table` must be float64; got %s" % (name, table.dtype))
    if table.device != x.device:
        raise ValueError("%s: `table` must be on %s; got %s" % (name, x.device, table.device))
    if table.dim() != out_dim or any(n < 4 for n in table.shape):
        raise ValueError("%s: `table` must have one dimension of at least 4 points per %s (%d); got %s" % (name, unit, out_dim, list(table.shape)))
    if not table.is_contiguous():
        raise ValueError("%s: `table` must be contiguous (%s 0 is its slowest axis)" % (name, unit))
    if table.numel() >= 2 ** 31:
        raise ValueError("%s: `table` must hold fewer than 2^31 points; got %d" % (name, table.numel()))
    lower, spacing = _grid_floats(name, "lower", lower, out_dim, unit), _grid_floats(name, "spacing", spacing, out_dim, unit)
    if not all(math.isfinite(h) and h > 0.0 for h in spacing):
        raise ValueError("%s: `spacing` holds the grid's steps and must be finite and > 0; got %s" % (name, spacing))
    if not all(math.isfinite(v) for v in lower):
        raise ValueError("%s: `lower` holds the position of the grid's first point and must be finite; got %s" % (name, lower))
    if periodic is None:
        periodic = [False] * out_dim
    else:
        if isinstance(periodic, torch.Tensor):
            periodic = periodic.reshape(-1).tolist()
        try:
            periodic = [bool(p) for p in periodic]
        except TypeError:
            raise TypeError("%s: `periodic` must be None or a sequence of %d bools; got %s" % (name, out_dim, type(periodic).__name__))
        if len(periodic) != out_dim:
            raise ValueError("%s: `periodic` must hold one bool per %s (%d); got %d" % (name, unit, out_dim, len(periodic)))
    return (table.detach(), lower, spacing, periodic) + _check_into_triple(name, x, into, out_dim, _GRID)


def _check_bias_terms(name, restraint, hills, grid, opes=None):
    """The terms of value_and_bias as they come, before anything needs a device: each None or its record of `molann_amd.bias` (whose
    construction has checked its `columns`), and at least one of them; `hills` and `opes` together: NotImplementedError naming the
    routes that remain."""
    for what, term, cls in (("restraint", restraint, _bias.Restraint), ("hills", hills, _bias.Hills), ("grid", grid, _bias.Grid),
                            ("opes", opes, (_bias.Opes, _bias.OpesFromTable))):
        if term is not None and not isinstance(term, cls):
            raise TypeError("%s: `%s` must be None or a molann_amd.bias.%s; got %s"
                            % (name, what, cls.__name__ if isinstance(cls, type) else "Opes or OpesFromTable", type(term).__name__))
    if restraint is None and hills is None and grid is None and opes is None:
        raise ValueError("%s: at least one of `restraint`, `hills` and `grid` must be given" % name)
    if hills is not None and opes is not None:
        raise NotImplementedError("%s: %s" % (name, _HILLS_AND_OPES_ROUTE))


def _bias_columns(name, what, columns, width, cap, out_dim):
    """The column list of a term of value_and_bias against the model: None is the first `width` outputs.  An index >= out_dim or an
    identity list longer than out_dim: IndexError; more than `cap` columns: NotImplementedError."""
    if columns is None:      # the cap, then the model: the order of the C entry
        if width > cap:
            raise NotImplementedError("%s: the one-launch kernel serves at most %d %s columns (got %d); %s" % (name, cap, what, width, _BIAS_ROUTE))
        if width > out_dim:
            raise IndexError("%s: `%s` has %d columns but the model has %d outputs" % (name, what, width, out_dim))
        return tuple(range(width))
    if any(c >= out_dim for c in columns):
        raise IndexError("%s: `%s.columns` must lie in [0, %d); got %s" % (name, what, out_dim, list(columns)))
    return columns


def _hills_width(name, centers, what="hills"):
    """The number of columns of a `Hills` (or an `Opes`, by `what`) without `columns`: centers' second dimension, or the length of its first row.  An empty
    sequence has neither: ValueError (a ``[0, d]`` tensor, or `columns`, says what is meant)."""
    if isinstance(centers, torch.Tensor) and centers.dim() == 2:
        return centers.shape[1]
    rows = len(centers) if hasattr(centers, "__len__") else 0
    if rows and hasattr(centers[0], "__len__"):
        return len(centers[0])
    raise ValueError("%s: `%s.centers` must be [H, columns] to tell the columns the %s act on; for no %s yet pass `columns` or a "
                     "[0, columns] tensor (got %s)" % (name, what, "kernels" if what == "opes" else what, "kernels" if what == "opes" else what,
                                                       list(centers.shape) if isinstance(centers, torch.Tensor) else type(centers).__name__))


def _check_bias_args(name, x, out_dim, restraint, hills, grid, into, owner=None):
    """The checks of value_and_bias after the gate, all before any launch on x's device: the column lists against the model, then every
    term by the check of its single call with the term's width in place of the number of outputs (the same conversions and remembered
    read-backs), then `into`.  Returns ((center, kappa, period, flat) or None, (columns, centers, heights, sigma, period) or None,
    (columns, table, lower, spacing, periodic) or None, y, energies, dx)."""
    hc = gc = None
    if hills is not None:
        width = len(hills.columns) if hills.columns is not None else _hills_width(name, hills.centers)
        hc = _bias_columns(name, "hills", hills.columns, width, _bias.HILLS_MAX_COLUMNS, out_dim)
    if grid is not None:
        width = grid.table.dim() if isinstance(grid.table, torch.Tensor) and grid.columns is None else 1
        gc = _bias_columns(name, "grid", grid.columns, width, _bias.GRID_MAX_COLUMNS, out_dim)
    r = h = g = None
    if restraint is not None:
        r = _check_restraint_args(name, x, out_dim, restraint.center, restraint.kappa, restraint.period, restraint.flat, None, owner=owner)[:4]
    if hills is not None:
        h = (hc,) + _check_hills_args(name, x, len(hc), hills.centers, hills.heights, hills.sigma, hills.period, None, owner=owner, unit="hills column")[:4]
    if grid is not None:
        g = (gc,) + _check_grid_args(name, x, len(gc), grid.table, grid.lower, grid.spacing, grid.periodic, None, owner=owner, unit="grid column")[:4]
    return (r, h, g) + _check_into_triple(name, x, into, out_dim, _BIAS)


def _check_bias_opes_args(name, x, out_dim, restraint, grid, opes, into, owner=None):
    """The checks of value_and_bias with an OPES term after the gate, as `_check_bias_args` makes them: the column lists against the
    model, then the restraint and the table by the checks of their single calls, the OPES term by `_check_opes_args` with the term's
    width ``len(columns)`` in place of the number of outputs (the same conversions, the same remembered `sigma` read-back, the same
    scalar ValueErrors), then `into` with energies [N, 4].  Returns ((center, kappa, period, flat) or None, (columns, table, lower,
    spacing, periodic) or None, (columns, centers, heights, sigma, period, scale, norm, epsilon, cutoff), y, energies, dx)."""
    width = len(opes.columns) if opes.columns is not None else _hills_width(name, opes.centers, "opes")
    oc = _bias_columns(name, "opes", opes.columns, width, _bias.HILLS_MAX_COLUMNS, out_dim)
    gc = None
    if grid is not None:
        width = grid.table.dim() if isinstance(grid.table, torch.Tensor) and grid.columns is None else 1
        gc = _bias_columns(name, "grid", grid.columns, width, _bias.GRID_MAX_COLUMNS, out_dim)
    r = g = None
    if restraint is not None:
        r = _check_restraint_args(name, x, out_dim, restraint.center, restraint.kappa, restraint.period, restraint.flat, None, owner=owner)[:4]
    o = (oc,) + _check_opes_args(name, x, len(oc), opes.centers, opes.heights, opes.sigma, opes.scale, opes.norm, opes.epsilon, opes.cutoff,
                                 opes.period, None, owner=owner)[:8]
    if grid is not None:
        g = (gc,) + _check_grid_args(name, x, len(gc), grid.table, grid.lower, grid.spacing, grid.periodic, None, owner=owner, unit="grid column")[:4]
    return (r, g, o) + _check_into_triple(name, x, into, out_dim, _BIAS_OPES)


def _check_bias_opes_table_args(name, x, out_dim, restraint, grid, opes, into, owner=None):
    """The checks of value_and_bias with an `OpesFromTable` after the gate, as `_check_bias_opes_args` makes them, all before any launch
    and with nothing read back: the column lists against the model, then the restraint and the table by the checks of their single calls,
    the record's table, scale and epsilon by `_check_opes_table_args` with the term's width ``table.d`` in place of the number of outputs,
    then `into` with energies [N, 4].  The widths are not looked at: they are the deposits' and live in device memory.  Returns ((center,
    kappa, period, flat) or None, (columns, table, lower, spacing, periodic) or None, (columns, centers, heights, sigma, state, period,
    scale, epsilon, cutoff), y, energies, dx)."""
    if not isinstance(opes.table, _bias.OpesTable):
        raise TypeError("%s: `opes.table` must be a molann_amd.bias.OpesTable; got %s" % (name, type(opes.table).__name__))
    width = opes.table.d
    if opes.columns is not None and len(opes.columns) != width:      # a record changed through `_replace`
        raise ValueError("%s: `opes.columns` must name one output per column of `opes.table` (%d); got %d" % (name, width, len(opes.columns)))
    oc = _bias_columns(name, "opes", opes.columns, width, _bias.HILLS_MAX_COLUMNS, out_dim)
    gc = None
    if grid is not None:
        gwidth = grid.table.dim() if isinstance(grid.table, torch.Tensor) and grid.columns is None else 1
        gc = _bias_columns(name, "grid", grid.columns, gwidth, _bias.GRID_MAX_COLUMNS, out_dim)
    r = g = None
    if restraint is not None:
        r = _check_restraint_args(name, x, out_dim, restraint.center, restraint.kappa, restraint.period, restraint.flat, None, owner=owner)[:4]
    o = (oc,) + _check_opes_table_args(name, x, len(oc), opes.table, opes.scale, opes.epsilon, None, owner=owner)[:8]
    if grid is not None:
        g = (gc,) + _check_grid_args(name, x, len(gc), grid.table, grid.lower, grid.spacing, grid.periodic, None, owner=owner, unit="grid column")[:4]
    return (r, g, o) + _check_into_triple(name, x, into, out_dim, _BIAS_OPES_TABLE)


def _check_pbmetad_args(name, x, out_dim, tables, kT, restraint, into, owner=None):
    """The checks of value_and_pbmetad after the gate, all before any launch on x's device and with nothing read back: the record (whose
    construction has checked its shapes and its `columns`) against the model and x's device, kT, the restraint by the check of its
    single call, then `into` with energies [N, 2 + K].  Returns ((center, kappa, period, flat) or None, (columns, table, shape, lower,
    spacing, periodic, kT), y, energies, dx)."""
    if not isinstance(tables, _bias.PBTables):
        raise TypeError("%s: `tables` must be a molann_amd.bias.PBTables; got %s" % (name, type(tables).__name__))
    if restraint is not None and not isinstance(restraint, _bias.Restraint):
        raise TypeError("%s: `restraint` must be None or a molann_amd.bias.Restraint; got %s" % (name, type(restraint).__name__))
    if isinstance(kT, bool) or not isinstance(kT, (int, float)):
        raise TypeError("%s: `kT` must be a Python float; got %s" % (name, type(kT).__name__))
    kT = float(kT)
    if not (kT > 0.0 and math.isfinite(kT)):
        raise ValueError("%s: `kT` must be finite and > 0; got %r" % (name, kT))
    K = len(tables.shape)
    cols = tables.columns
    if cols is None:
        if K > out_dim:
            raise IndexError("%s: `tables` has %d axes but the model has %d outputs" % (name, K, out_dim))
        cols = tuple(range(K))
    elif len(cols) != K:      # a record changed through `_replace`
        raise ValueError("%s: `tables.columns` must name one output per table (%d); got %d" % (name, K, len(cols)))
    elif any(c >= out_dim for c in cols):
        raise IndexError("%s: `tables.columns` must lie in [0, %d); got %s" % (name, out_dim, list(cols)))
    table = tables.table
    if not isinstance(table, torch.Tensor) or table.dtype != torch.float64:
        raise TypeError("%s: `tables.table` must be a float64 tensor" % name)
    if table.device != x.device:
        raise ValueError("%s: `tables.table` must be on %s; got %s" % (name, x.device, table.device))
    if table.dim() != 1 or table.numel() != sum(tables.shape) or not table.is_contiguous():
        raise ValueError("%s: `tables.table` must be contiguous [sum(shape) = %d]; got %s" % (name, sum(tables.shape), list(table.shape)))
    periodic = [False] * K if tables.periodic is None else [bool(p) for p in tables.periodic]
    r = None
    if restraint is not None:
        r = _check_restraint_args(name, x, out_dim, restraint.center, restraint.kappa, restraint.period, restraint.flat, None, owner=owner)[:4]
    t = (cols, table.detach(), [int(n) for n in tables.shape], [float(v) for v in tables.lower], [float(v) for v in tables.spacing], periodic, kT)
    return (r, t) + _check_into_triple(name, x, into, out_dim, _PBMETAD, width=2 + K)


def _check_grad_out(name, x, out_dim, grad_out):
    if not isinstance(grad_out, torch.Tensor) or grad_out.numel() != x.shape[0] * out_dim or grad_out.device != x.device:
        raise ValueError("%s: grad_out must hold [%d, %d] values on %s" % (name, x.shape[0], out_dim, x.device))


def _check_atom_weights(name, x, n_inp, weights):
    """The atom weights of value_and_metric: None, or n_inp float64 values on x's device, returned flat and contiguous."""
    if weights is None:
        return None
    if not isinstance(weights, torch.Tensor) or weights.dtype != torch.float64:
        raise TypeError("%s: `weights` must be None or a float64 tensor of %d values; got %s"
                        % (name, n_inp, weights.dtype if isinstance(weights, torch.Tensor) else type(weights).__name__))
    if weights.numel() != n_inp or weights.device != x.device:
        raise ValueError("%s: `weights` must hold %d values (one per atom) on %s; got %d on %s"
                         % (name, n_inp, x.device, weights.numel(), weights.device))
    return weights.detach().reshape(-1).contiguous()


def _check_metric_args(name, x, n_inp, out_dim, weights, into):
    """The `weights` and `into` checks of value_and_metric (before any launch); returns (weights or None, y, M) with y, M None where
    `into` is."""
    weights = _check_atom_weights(name, x, n_inp, weights)
    return (weights,) + _check_into(name, x, into, torch.float64, out_dim, (x.shape[0], out_dim, out_dim), _ONE_LAUNCH_PAIR[_METRIC])


def _one_launch_arguments(kind, x, extra, into, n_inp, out_dim, lins, al, owner=None):
    """The float64 one-launch calls after the caller's gate (a HIP tensor, modules one plan serves), in this order: x's shape, float64
    x, float64 head (the alignment's ref_x where there is no head) on x's device, x detached and contiguous, the extra argument
    (`grad_out`, the metric's atom weights, the restraint's (center, kappa, period, flat), the hills' (centers, heights, sigma,
    period), the grid's (table, lower, spacing, periodic)), `into`.  Returns (x, extra, y, second, second's shape), y and second None without `into`; the restraint's second is the
    pair (energy, dx), the hills' and the grid's (bias, dx)."""
    name = _ONE_LAUNCH_NAME[kind]
    _check_input(x, n_inp)
    if x.dtype != torch.float64:
        raise TypeError("%s is float64: call %s and pass a float64 x (got %s); for float32 %s"
                        % (name, "model.double()" if lins else ".double()", x.dtype, _ONE_LAUNCH_ROUTE[kind]))
    if lins:
        w0 = lins[0].weight
        if w0.device != x.device or w0.dtype != torch.float64:
            raise RuntimeError("ann_layers must be float64 on %s for a float64 input (got %s on %s): call .double()"
                               % (x.device, w0.dtype, w0.device))
    elif al is not None and (al.ref_x.dtype != torch.float64 or al.ref_x.device != x.device):
        raise RuntimeError("the alignment layer's ref_x must be float64 on %s for a float64 input (got %s on %s): call .double()"
                           % (x.device, al.ref_x.dtype, al.ref_x.device))
    x = x.detach()
    x = x if x.is_contiguous() else x.contiguous()
    n = x.shape[0]
    if kind == _VJP:
        shape = (n, n_inp, 3)
        _check_grad_out(name, x, out_dim, extra)
        if not extra.dtype.is_floating_point:
            raise TypeError("%s: grad_out must be a floating-point tensor; got %s" % (name, extra.dtype))
    elif kind == _JACOBIAN:
        shape = (n, out_dim, n_inp, 3)
    elif kind == _BIAS:
        checked = _check_bias_args(name, x, out_dim, *extra, into, owner=owner)
        return x, checked[:3], checked[3], (checked[4], checked[5]) if checked[3] is not None else None, (n, n_inp, 3)
    elif kind == _BIAS_OPES:
        checked = _check_bias_opes_args(name, x, out_dim, *extra, into, owner=owner)
        return x, checked[:3], checked[3], (checked[4], checked[5]) if checked[3] is not None else None, (n, n_inp, 3)
    elif kind == _BIAS_OPES_TABLE:
        checked = _check_bias_opes_table_args(name, x, out_dim, *extra, into, owner=owner)
        return x, checked[:3], checked[3], (checked[4], checked[5]) if checked[3] is not None else None, (n, n_inp, 3)
    elif kind == _PBMETAD:
        checked = _check_pbmetad_args(name, x, out_dim, *extra, into, owner=owner)
        return x, checked[:2], checked[2], (checked[3], checked[4]) if checked[2] is not None else None, (n, n_inp, 3)
    elif kind == _OPES:
        checked = _check_opes_args(name, x, out_dim, *extra, into, owner=owner)
        return x, checked[:8], checked[8], (checked[9], checked[10]) if checked[8] is not None else None, (n, n_inp, 3)
    elif kind == _OPES_TABLE:
        checked = _check_opes_table_args(name, x, out_dim, *extra, into, owner=owner)
        return x, checked[:8], checked[8], (checked[9], checked[10]) if checked[8] is not None else None, (n, n_inp, 3)
    elif kind in _BIAS_KINDS:
        checked = (_check_restraint_args, _check_hills_args, _check_grid_args)[kind - _RESTRAINT](name, x, out_dim, *extra, into, owner=owner)
        return x, checked[:4], checked[4], (checked[5], checked[6]) if checked[4] is not None else None, (n, n_inp, 3)
    else:
        shape = (n, out_dim, out_dim)
        extra = _check_atom_weights(name, x, n_inp, extra)
    y, second = _check_into(name, x, into, torch.float64, out_dim, shape, _ONE_LAUNCH_PAIR[kind])
    if kind == _VJP and not (extra.dtype == torch.float64 and extra.is_contiguous()):
        extra = extra.double().contiguous()
    return x, extra, y, second, shape


def _one_launch_ctypes(kind, entry, x, extra, y, second, shape, out_dim, lins, al):
    """The ctypes way to the kernel of a float64 one-launch call whose arguments `_one_launch_arguments` has checked."""
    plan = entry.plan
    with torch.cuda.device(x.device):
        if kind == _OPES:
            if not plan.supports_value_and_opes_f64():
                raise NotImplementedError("value_and_opes: one frame's rows exceed the LDS of a compute unit for this model; " + _OPES_ROUTE)
        elif kind == _OPES_TABLE:
            if not plan.supports_value_and_opes_table_f64():
                raise NotImplementedError("value_and_opes_table: one frame's rows exceed the LDS of a compute unit for this model; " + _OPES_ROUTE)
        elif kind == _BIAS_OPES:
            if not plan.supports_value_and_bias_opes_f64():
                raise NotImplementedError("value_and_bias: one frame's rows exceed the LDS of a compute unit for this model; " + _BIAS_OPES_ROUTE)
        elif kind == _BIAS_OPES_TABLE:
            if not plan.supports_value_and_bias_opes_table_f64():
                raise NotImplementedError("value_and_bias: one frame's rows exceed the LDS of a compute unit for this model; " + _BIAS_OPES_TABLE_ROUTE)
        elif kind == _PBMETAD:
            if not plan.supports_value_and_pbmetad_f64():
                raise NotImplementedError("value_and_pbmetad: one frame's rows exceed the LDS of a compute unit for this model; " + _PBMETAD_ROUTE)
        elif kind in _BIAS_KINDS or kind == _BIAS:
            if not (plan.supports_value_and_restraint_f64, plan.supports_value_and_hills_f64, plan.supports_value_and_grid_f64,
                    plan.supports_value_and_bias_f64)[kind - _RESTRAINT]():
                raise NotImplementedError("%s: one frame's rows exceed the LDS of a compute unit for this model; %s"
                                          % (_ONE_LAUNCH_NAME[kind], _ONE_LAUNCH_ROUTE[kind]))
        elif kind != _VJP and not (plan.supports_value_and_jacobian_f64() if kind == _JACOBIAN else plan.supports_value_and_metric_f64()):
            if kind == _JACOBIAN:
                raise NotImplementedError("value_and_jacobian: one frame's rows exceed the LDS of a compute unit for this model; "
                                          + _JACOBIAN_ROUTE)
            raise NotImplementedError("value_and_metric: no single-launch kernel for this %s (more than 64 %s, or one frame's rows exceed "
                                      "the LDS of a compute unit); " % (("model", "outputs") if lins else ("module", "features"))
                                      + _METRIC_ROUTE)
        if al is not None:
            entry.sync_ref(_device_buffer(al.ref_x, x))
        if y is None:
            y = torch.empty((x.shape[0], out_dim), dtype=torch.float64, device=x.device)
            second = torch.empty(shape, dtype=torch.float64, device=x.device)
            if kind in _BIAS_KINDS or kind == _OPES or kind == _OPES_TABLE:
                second = (torch.empty((x.shape[0],), dtype=torch.float64, device=x.device), second)
            if kind == _BIAS or kind == _BIAS_OPES or kind == _BIAS_OPES_TABLE:
                second = (torch.empty((x.shape[0], 3 if kind == _BIAS else 4), dtype=torch.float64, device=x.device), second)
            if kind == _PBMETAD:
                second = (torch.empty((x.shape[0], 2 + len(extra[1][0])), dtype=torch.float64, device=x.device), second)
        if kind == _PBMETAD:
            if x.shape[0] > 0:
                plan.value_and_pbmetad_f64(x, [lin.weight.detach().contiguous() for lin in lins], [lin.bias.detach().contiguous() for lin in lins],
                                           y, *second, extra[1], restraint=extra[0])
            return (y,) + tuple(second)
        if kind == _BIAS_OPES_TABLE:
            if x.shape[0] > 0:
                plan.value_and_bias_opes_table_f64(x, [lin.weight.detach().contiguous() for lin in lins],
                                                   [lin.bias.detach().contiguous() for lin in lins], y, *second, extra[2], restraint=extra[0],
                                                   grid=extra[1])
            return (y,) + tuple(second)
        if kind == _BIAS_OPES:
            if x.shape[0] > 0:
                plan.value_and_bias_opes_f64(x, [lin.weight.detach().contiguous() for lin in lins], [lin.bias.detach().contiguous() for lin in lins],
                                             y, *second, extra[2], restraint=extra[0], grid=extra[1])
            return (y,) + tuple(second)
        if kind == _BIAS:
            if x.shape[0] > 0:
                plan.value_and_bias_f64(x, [lin.weight.detach().contiguous() for lin in lins], [lin.bias.detach().contiguous() for lin in lins],
                                        y, *second, restraint=extra[0], hills=extra[1], grid=extra[2])
            return (y,) + tuple(second)
        if kind == _RESTRAINT:
            if x.shape[0] > 0:
                plan.value_and_restraint_f64(x, [lin.weight.detach().contiguous() for lin in lins], [lin.bias.detach().contiguous() for lin in lins],
                                             *extra, y, *second, center_stride=out_dim if extra[0].dim() == 2 else 0)
            return (y,) + tuple(second)
        if kind == _HILLS:
            if x.shape[0] > 0:
                plan.value_and_hills_f64(x, [lin.weight.detach().contiguous() for lin in lins], [lin.bias.detach().contiguous() for lin in lins],
                                         *extra, y, *second)
            return (y,) + tuple(second)
        if kind == _OPES:
            if x.shape[0] > 0:
                plan.value_and_opes_f64(x, [lin.weight.detach().contiguous() for lin in lins], [lin.bias.detach().contiguous() for lin in lins],
                                        *extra, y, *second)
            return (y,) + tuple(second)
        if kind == _OPES_TABLE:
            if x.shape[0] > 0:
                plan.value_and_opes_table_f64(x, [lin.weight.detach().contiguous() for lin in lins], [lin.bias.detach().contiguous() for lin in lins],
                                              *extra, y, *second)
            return (y,) + tuple(second)
        if kind == _GRID:
            if x.shape[0] > 0:
                plan.value_and_grid_f64(x, [lin.weight.detach().contiguous() for lin in lins], [lin.bias.detach().contiguous() for lin in lins],
                                        *extra, y, *second)
            return (y,) + tuple(second)
        if x.shape[0] > 0:
            W = [lin.weight.detach().contiguous() for lin in lins]
            B = [lin.bias.detach().contiguous() for lin in lins]
            if kind == _VJP:
                plan.value_and_vjp_f64(x, extra, W, B, y, second)
            elif kind == _JACOBIAN:
                plan.value_and_jacobian_f64(x, W, B, y, second)
            else:
                plan.value_and_metric_f64(x, W, B, extra, y, second)
    return y, second


class PreprocessingANN(_PlanOwner, torch.nn.Module):
    """``feature_layer(align_layer(x))``; ``align_layer=None`` means no alignment (`ann.py:533-565`)."""

    def __init__(self, align_layer, feature_layer):
        super(PreprocessingANN, self).__init__()
        self.align_layer = align_layer if align_layer is not None else torch.nn.Identity()
        self.feature_layer = feature_layer

    def output_dimension(self):
        return self.feature_layer.output_dimension()

    def _fusable(self):
        return isinstance(self.feature_layer, FeatureLayer) and \
            (isinstance(self.align_layer, AlignmentLayer) or type(self.align_layer) is torch.nn.Identity)

    def forward(self, x):
        if not self._fusable():
            return self.feature_layer(self.align_layer(x))
        al = self.align_layer if isinstance(self.align_layer, AlignmentLayer) else None
        if al is not None:
            _check_input(x, al.input_atom_num)
            assert al.input_atom_num == self.feature_layer.input_atom_num, \
                f'Input should be a 3d torch tensor, with sizes [*, {self.feature_layer.input_atom_num}, 3]. Actual sizes: {x.shape}'
        _check_input(x, self.feature_layer.input_atom_num)
        return _run_features(self.feature_layer, x, al, plan_owner=self)

    def value_and_metric(self, x, weights=None, into=None):
        """``(feat, G)`` with ``feat = self(x)`` [N, d_feat] and the metric tensor of the features
        ``G[f, k, l] = sum_a w_a grad_a feat_k(x_f) . grad_a feat_l(x_f)`` [N, d_feat, d_feat], float64, in ONE kernel launch
        (`molann_value_and_metric_f64`, frames_value_metric_f64_kernel, on this module's float64 feature plan): the Jacobian
        contracted with itself over the atoms where it is computed, never stored.  ``weights``: None (all ones) or a float64 tensor of
        n_inp values on x's device (inverse masses, diffusion coefficients; any sign).  G holds no parameter: for any head behind
        these features ``sum_a w_a |grad_a y_k|^2 = dF_k G dF_k^T`` with ``dF = d y / d feat``, so a loss built from gradient norms
        needs G once per dataset and no second-order pass through the preprocessing.  No autograd graph is recorded;
        ``into=(feat, G)`` reuses the caller's buffers.  The same bits on every call, G symmetric bit for bit; ``weights=None`` gives
        the bits of ``torch.ones``."""
        if not (isinstance(x, torch.Tensor) and x.is_cuda and self._fusable()):
            raise NotImplementedError("value_and_metric needs a FeatureLayer behind an AlignmentLayer or none, float64, on a HIP tensor; "
                                      "otherwise " + _METRIC_ROUTE)
        fl = self.feature_layer
        al = self.align_layer if isinstance(self.align_layer, AlignmentLayer) else None
        d = fl.output_dimension()
        x, weights, y, M, shape = _one_launch_arguments(_METRIC, x, weights, into, fl.input_atom_num, d, (), al)
        spec, uav = _feature_spec(fl)

        def build():
            if al is None:
                return _capi.Plan(fl.input_atom_num, features=spec, use_angle_value=uav)
            return _capi.Plan(fl.input_atom_num, align_idx=al._local_align_atom_indices, ref_x=al.ref_x, features=spec, use_angle_value=uav)

        return _one_launch_ctypes(_METRIC, _get_entry(self, x, "features", build), x, weights, y, M, shape, d, (), al)

    def value_and_restraint(self, x, center, kappa, period=None, flat=None, into=None):
        """``(feat, energy, dx)``: `MolANN.value_and_restraint` on the features themselves, float64, in ONE kernel launch
        (`molann_value_and_restraint_f64`, frames_value_restraint_f64_kernel, on this module's float64 feature plan; no head).
        ``energy[f] = 1/2 sum_k kappa_k d_k^2`` with ``d = feat - center`` and ``dx = d energy / d x``; forces are ``-dx``.  Umbrella
        sampling on raw dihedral angles: ``use_angle_value=True`` and ``period = 2 pi``.  ``center`` [d_feat] or [N, d_feat], ``kappa``
        a float or [d_feat], ``period`` / ``flat`` None or [d_feat], as `MolANN.value_and_restraint` takes them (a float64 tensor on
        x's device passes as it is; every conversion costs a launch).  No autograd graph is recorded; ``into=(feat, energy, dx)``
        reuses the caller's buffers.  The same bits on every call.  Out of scope: float32, a `GraphedForces` replay, other bias shapes,
        gradients with respect to centres or stiffnesses."""
        return self._bias_on_features(_RESTRAINT, x, (center, kappa, period, flat), into)

    def value_and_hills(self, x, centers, heights, sigma, period=None, into=None):
        """``(feat, bias, dx)``: `MolANN.value_and_hills` on the features themselves, float64, in ONE kernel launch
        (`molann_value_and_hills_f64`, frames_value_hills_f64_kernel, on this module's float64 feature plan; no head): a metadynamics
        bias ``bias[f] = sum_h heights_h exp(-1/2 sum_k (d_hk / sigma_hk)^2)``, ``d_h = feat - centers_h``, and ``dx = d bias / d x``;
        forces are ``-dx``.  Metadynamics on raw dihedral angles: ``use_angle_value=True`` and ``period = 2 pi``.  ``centers``
        [H, d_feat], ``heights`` [H] or a float, ``sigma`` a float, [d_feat] or [H, d_feat], ``period`` None or [d_feat], as
        `MolANN.value_and_hills` takes them; at most 8 features.  No autograd graph is recorded; ``into=(feat, bias, dx)`` reuses the
        caller's buffers.  The same bits on every call."""
        return self._bias_on_features(_HILLS, x, (centers, heights, sigma, period), into)

    def value_and_grid(self, x, table, lower, spacing, periodic=None, into=None):
        """``(feat, bias, dx)``: `MolANN.value_and_grid` on the features themselves, float64, in ONE kernel launch
        (`molann_value_and_grid_f64`, frames_value_grid_f64_kernel, on this module's float64 feature plan; no head): the bias
        interpolated from ``table`` (cubic convolution on a regular grid, one axis per feature) and ``dx = d bias / d x``; forces are
        ``-dx``.  A phi / psi surface on raw dihedral angles: ``use_angle_value=True``, ``lower = -pi``, ``spacing = 2 pi / n`` and
        ``periodic = True``.  ``table``, ``lower``, ``spacing``, ``periodic`` as `MolANN.value_and_grid` takes them; at most 3 features.
        No autograd graph is recorded; ``into=(feat, bias, dx)`` reuses the caller's buffers.  The same bits on every call."""
        return self._bias_on_features(_GRID, x, (table, lower, spacing, periodic), into)

    def value_and_bias(self, x, restraint=None, hills=None, grid=None, into=None, opes=None):
        """``(feat, energies, dx)``: `MolANN.value_and_bias` on the features themselves, float64, in ONE kernel launch
        (`molann_value_and_bias_f64`, frames_value_bias_f64_kernel, on this module's float64 feature plan; no head): a restraint on
        all features, hills on up to 8 chosen features and a table on up to 3, ``energies[f] = (E_r, V_h, V_g)`` and ``dx`` the gradient
        of their sum; forces are ``-dx``.  Position columns under walls and two raw dihedral angles under metadynamics:
        ``use_angle_value=True``, the angles' indices as ``columns`` and ``period = 2 pi``.  The terms are `molann_amd.bias.Restraint`,
        `Hills` and `Grid`, as `MolANN.value_and_bias` takes them.  No autograd graph is recorded; ``into=(feat, energies, dx)``
        reuses the caller's buffers.  The same bits on every call.  ``opes``: a `molann_amd.bias.Opes` in the place of ``hills``, as
        `MolANN.value_and_bias` takes it (frames_value_bias_opes_f64_kernel, ``energies`` [N, 4] = ``(E_r, 0, V_g, V_o)``): OPES on two raw
        dihedral angles of a module with any number of features, with walls and a periodic table next to it.  A
        `molann_amd.bias.OpesFromTable` in its place reads the live count and the norm from the table's state on the device
        (frames_value_bias_opes_table_f64_kernel), as `MolANN.value_and_bias` takes it."""
        _check_bias_terms("value_and_bias", restraint, hills, grid, opes)
        if opes is not None:
            return self._bias_on_features(_BIAS_OPES_TABLE if isinstance(opes, _bias.OpesFromTable) else _BIAS_OPES, x, (restraint, grid, opes), into)
        return self._bias_on_features(_BIAS, x, (restraint, hills, grid), into)

    def value_and_opes(self, x, centers, heights, sigma, scale, norm, epsilon, cutoff=None, period=None, into=None):
        """``(feat, bias, dx)``: `MolANN.value_and_opes` on the features themselves, float64, in ONE kernel launch
        (`molann_value_and_opes_f64`, frames_value_opes_f64_kernel, on this module's float64 feature plan; no head): an OPES bias
        ``bias[f] = scale log(P(feat[f]) / norm + epsilon)`` on the kernel density ``P = sum_h heights_h (exp(-q_h / 2) - exp(-cutoff^2 /
        2))`` over the kernels with ``q_h = sum_k (d_hk / sigma_hk)^2 < cutoff^2``, and ``dx = d bias / d x``; forces are ``-dx``.  OPES
        on raw dihedral angles: ``use_angle_value=True`` and ``period = 2 pi``.  The arguments as `MolANN.value_and_opes` takes them; at
        most 8 features.  No autograd graph is recorded; ``into=(feat, bias, dx)`` reuses the caller's buffers.  The same bits on every
        call."""
        return self._bias_on_features(_OPES, x, (centers, heights, sigma, scale, norm, epsilon, cutoff, period), into)

    def value_and_opes_table(self, x, table, scale, epsilon, into=None):
        """``(feat, bias, dx)``: `MolANN.value_and_opes_table` on the features themselves, float64, in ONE kernel launch
        (`molann_value_and_opes_table_f64`, frames_value_opes_table_f64_kernel, on this module's float64 feature plan; no head):
        `value_and_opes` on a `molann_amd.bias.OpesTable` whose live count and normalisation the kernel reads from the table's state
        in device memory, so nothing is read back.  The arguments as `MolANN.value_and_opes_table` takes them; ``table.d`` features."""
        return self._bias_on_features(_OPES_TABLE, x, (table, scale, epsilon), into)

    def value_and_pbmetad(self, x, tables, kT, restraint=None, into=None):
        """``(feat, energies, dx)``: `MolANN.value_and_pbmetad` on the features themselves, float64, in ONE kernel launch
        (`molann_value_and_pbmetad_f64`, frames_value_pbmetad_f64_kernel, on this module's float64 feature plan; no head): a
        parallel-bias metadynamics bias on up to 8 chosen features, one 1-D table each.  Raw dihedral angles: ``use_angle_value=True``,
        ``lower = -pi``, ``spacing = 2 pi / n`` and ``periodic = True`` per axis.  The arguments as `MolANN.value_and_pbmetad` takes
        them.  No autograd graph is recorded; ``into=(feat, energies, dx)`` reuses the caller's buffers.  The same bits on every call."""
        return self._bias_on_features(_PBMETAD, x, (tables, kT, restraint), into)

    def _bias_on_features(self, kind, x, extra, into):
        """value_and_restraint / value_and_hills / value_and_grid / value_and_bias / value_and_opes / value_and_opes_table of this module: the gate, the checks and the ctypes plan of the features."""
        if not (isinstance(x, torch.Tensor) and x.is_cuda and self._fusable()):
            raise NotImplementedError("%s needs a FeatureLayer behind an AlignmentLayer or none, float64, on a HIP tensor; "
                                      "otherwise %s" % (_ONE_LAUNCH_NAME[kind], _ONE_LAUNCH_FEATURES_ROUTE[kind]))
        fl = self.feature_layer
        al = self.align_layer if isinstance(self.align_layer, AlignmentLayer) else None
        d = fl.output_dimension()
        x, extra, y, second, shape = _one_launch_arguments(kind, x, extra, into, fl.input_atom_num, d, (), al, owner=self)
        spec, uav = _feature_spec(fl)

        def build():
            if al is None:
                return _capi.Plan(fl.input_atom_num, features=spec, use_angle_value=uav)
            return _capi.Plan(fl.input_atom_num, align_idx=al._local_align_atom_indices, ref_x=al.ref_x, features=spec, use_angle_value=uav)

        return _one_launch_ctypes(kind, _get_entry(self, x, "features", build), x, extra, y, second, shape, d, (), al)

    def __prepare_scriptable__(self):
        if not self._fusable():
            return torch.nn.Sequential(self.align_layer, self.feature_layer)
        al = self.align_layer if isinstance(self.align_layer, AlignmentLayer) else None
        return _script_features(self.feature_layer, al)


class MolANN(_PlanOwner, torch.nn.Module):
    """``ann_layers(preprocessing_layer(x))`` (`ann.py:606-624`).

    When ``ann_layers`` is a Sequential of Linear layers with one of the supported activations (what
    `create_sequential_nn` builds) the whole forward is one fused plan; any other module receives the
    features computed on the GPU.  ``mlp_precision='bf16'`` selects bf16 weights/activations with fp32
    accumulation on the bf16 MFMA for wide MLPs (the reference has no such mode).
    """

    def __init__(self, preprocessing_layer, ann_layers, mlp_precision="f32"):
        super(MolANN, self).__init__()
        self.preprocessing_layer = preprocessing_layer
        self.ann_layers = ann_layers
        assert mlp_precision in ("f32", "bf16")
        self.mlp_precision = mlp_precision

    def get_preprocessing_layer(self):
        return self.preprocessing_layer

    def __prepare_scriptable__(self):
        """`torch.jit.script(molann).save(...)` (`test/test_molann.py:114`, `README.rst:49`): the fused plan as
        one operator call when ann_layers is recognised, else the scripted preprocessing followed by ann_layers."""
        from . import script
        pp = self.preprocessing_layer
        rec = recognise_mlp(self.ann_layers)
        if rec is None or not (isinstance(pp, PreprocessingANN) and pp._fusable()):
            return torch.nn.Sequential(pp, self.ann_layers)
        linears, act = rec
        al = pp.align_layer if isinstance(pp.align_layer, AlignmentLayer) else None
        spec, uav = _feature_spec(pp.feature_layer)
        dims = [linears[0].in_features] + [lin.out_features for lin in linears]
        assert dims[0] == pp.feature_layer.output_dimension(), \
            'ann_layers expects %d inputs but the feature layer produces %d' % (dims[0], pp.feature_layer.output_dimension())
        desc = script.make_desc(script.KIND_FORWARD, pp.feature_layer.input_atom_num,
                                align_idx=al._local_align_atom_indices if al is not None else None, features=spec,
                                use_angle_value=uav, layer_dims=dims, activation=act,
                                mlp_precision=_capi.MLP_BF16 if self.mlp_precision == "bf16" else _capi.MLP_F32)
        return script.ScriptPlan(desc, ref_x=al.ref_x if al is not None else None, linears=linears)

    def plan_for(self, x):
        """The C-ABI plan (ctypes, `_capi.Plan`) of this model on x's device with `ref_x` and the Linear parameters packed:
        what tools/ and the tests of single entry points work on.  None if the model is not served by one fused plan."""
        st = self._fast_state(x)
        if not st["fused"]:
            return None
        entry = st["entry"]()
        with torch.cuda.device(x.device):
            if st["al"] is not None:
                entry.sync_ref(_device_buffer(st["al"].ref_x, x))
            entry.sync_mlp(st["linears"])
        return entry.plan

    def value_and_vjp(self, x, grad_out, into=None):
        """``(y, dx)`` with ``y = self(x)`` and ``dx = sum_k grad_out[:, k] d y[:, k] / d x`` in ONE kernel launch
        (`molann_value_and_vjp_f32`: the one-pass backward recomputes the forward anyway and, in this build, stores it too).
        For a caller that needs a collective variable and its forces at every step (`README.rst:49`): ~half the host time of a
        forward plus a backward.  The full Jacobian of a float64 model: `value_and_jacobian`, one launch that reads x and solves the
        rotation once per frame (``x.expand(d_out, -1, -1)`` with ``torch.eye(d_out)`` as cotangent repeats both per output; it
        remains the route for float32).
        No autograd graph is recorded (parameters are data); ``into=(y, dx)`` reuses the caller's buffers.  Models served by one
        fused plan whose backward is the one-pass kernel, and models on larger frames (molann_group_vjp) with no head or a head of
        at most 4 layers, every width <= 32, fp32, tanh / ReLU / sigmoid / identity / SiLU / LeakyReLU; float32.

        float64 (`model.double()` and a float64 x; `molann_value_and_vjp_f64`, one launch of frames_value_vjp_f64_kernel): every
        model served by one fused plan - any frame size, with or without an alignment, a head of any width with any of the
        nine activations.  Each row of dx is stored once, its terms summed in a fixed order: the same bits on every call."""
        st = self._one_launch_state(x, _VJP, "float32 or float64")
        if x.dtype == torch.float64:
            return self._one_launch_f64(_VJP, st, x, grad_out, into)
        al, fl = st["al"], st["fl"]
        _check_input(x, fl.input_atom_num)
        if x.dtype != torch.float32:
            raise TypeError("value_and_vjp is float32 / float64; got %s" % x.dtype)
        x = x.detach()
        x = x if x.is_contiguous() else x.contiguous()
        lins = st["linears"]
        if st["op"] is not None:
            y, dx = st["op_vjp"](x, st["handle"], _device_buffer(al.ref_x, x) if al is not None else st["no_ref"],
                                 [lin.weight for lin in lins], [lin.bias for lin in lins], grad_out, list(into) if into is not None else [])
            return y, dx
        n, out_dim = x.shape[0], st["out_dim"]
        _check_grad_out("value_and_vjp", x, out_dim, grad_out)
        y, dx = _check_into("value_and_vjp", x, into, torch.float32, out_dim, x.shape, _ONE_LAUNCH_PAIR[_VJP])
        entry = st["entry"]()
        with torch.cuda.device(x.device):
            if al is not None:
                entry.sync_ref(_device_buffer(al.ref_x, x))
            entry.sync_mlp(lins)
            if not entry.plan.supports_value_and_vjp():
                raise NotImplementedError("value_and_vjp: no single-launch kernel for this model: it serves the one-pass backward's plans "
                                          "and larger frames with no head or a head of at most 4 layers, every width <= 32, fp32, "
                                          "tanh / ReLU / sigmoid / identity / SiLU / LeakyReLU")
            if into is None:
                y, dx = torch.empty((n, out_dim), dtype=torch.float32, device=x.device), torch.empty_like(x)
            g = grad_out if (grad_out.dtype == torch.float32 and grad_out.is_contiguous()) else grad_out.float().contiguous()
            entry.plan.value_and_vjp(x, g, y, dx)
        return y, dx

    def _one_launch_state(self, x, kind, dtypes):
        """The fused-plan gate of the one-launch calls: this model's state on x's device, or the refusal that names the route that
        remains."""
        st = self._fast_state(x) if isinstance(x, torch.Tensor) and x.is_cuda else None
        if st is None or not st["fused"]:
            route = _ONE_LAUNCH_ROUTE[kind]
            raise NotImplementedError("%s needs a model served by one fused plan on a HIP device (a feature layer and a Linear / activation "
                                      "head, %s, on a HIP tensor)%s" % (_ONE_LAUNCH_NAME[kind], dtypes, "; otherwise " + route if route else ""))
        return st

    def _one_launch_f64(self, kind, st, x, extra, into):
        """A float64 one-launch call of a model the gate has passed: the arguments are checked once for both ways to the kernel (the
        dispatcher operator where that library is built, else the ctypes plan)."""
        al, lins, out_dim = st["al"], st["linears"], st["out_dim"]
        x, extra, y, second, shape = _one_launch_arguments(kind, x, extra, into, st["fl"].input_atom_num, out_dim, lins, al, owner=self)
        if st["op"] is None:
            return _one_launch_ctypes(kind, st["entry"](), x, extra, y, second, shape, out_dim, lins, al)
        op, ref = st[_ONE_LAUNCH_OP[kind]], _device_buffer(al.ref_x, x) if al is not None else st["no_ref"]
        W, B, into = [lin.weight for lin in lins], [lin.bias for lin in lins], list(into) if into is not None else []
        if kind in _BIAS_KINDS or kind == _OPES or kind == _OPES_TABLE:
            return tuple(op(x, st["handle"], ref, W, B, *extra, into))
        if kind == _BIAS:
            r, h, g = extra
            return tuple(op(x, st["handle"], ref, W, B, *(r or (None,) * 4), *((list(h[0]),) + h[1:] if h else ([], None, None, None, None)),
                            *((list(g[0]),) + g[1:] if g else ([], None, [], [], [])), into))
        if kind == _PBMETAD:
            r, t = extra
            return tuple(op(x, st["handle"], ref, W, B, *(r or (None,) * 4), list(t[0]), *t[1:], into))
        if kind == _BIAS_OPES or kind == _BIAS_OPES_TABLE:   # the same places in both operators: the record's fields follow its columns
            r, g, o = extra
            return tuple(op(x, st["handle"], ref, W, B, *(r or (None,) * 4), list(o[0]), *o[1:],
                            *((list(g[0]),) + g[1:] if g else ([], None, [], [], [])), into))
        y, second = op(x, st["handle"], ref, W, B, into) if kind == _JACOBIAN else op(x, st["handle"], ref, W, B, extra, into)
        return y, second

    def value_and_jacobian(self, x, into=None):
        """``(y, jac)`` with ``y = self(x)`` [N, d_out] and ``jac[f, k] = d y[f, k] / d x[f]`` [N, d_out, n_inp, 3], float64, in ONE
        kernel launch (`molann_value_and_jacobian_f64`, frames_value_jac_f64_kernel): what a collective variable hands an MD engine
        (every component's derivative with respect to the positions) and what a loss built from ``grad_x y_k`` for every k needs.
        x, the rotation, the features and the head forward are read and computed once per frame; ``y`` is `value_and_vjp`'s, bit for
        bit.  No autograd graph is recorded (parameters are data); ``into=(y, jac)`` reuses the caller's buffers.  Every row of
        ``jac`` is stored once, its terms summed in a fixed order: the same bits on every call.  `model.double()` and a float64 x
        on a HIP device; a model served by one fused plan."""
        return self._one_launch_f64(_JACOBIAN, self._one_launch_state(x, _JACOBIAN, "float64"), x, None, into)

    def value_and_metric(self, x, weights=None, into=None):
        """``(y, M)`` with ``y = self(x)`` [N, d_out] and the metric tensor of the outputs
        ``M[f, k, l] = sum_a w_a grad_a y_k(x_f) . grad_a y_l(x_f)`` [N, d_out, d_out], float64, in ONE kernel launch
        (`molann_value_and_metric_f64`, frames_value_metric_f64_kernel): `value_and_jacobian`'s Jacobian contracted with itself over
        the atoms in the wave that computes it, never stored - with inverse masses the metric of the string method, of
        temperature-accelerated MD and of effective dynamics along a collective variable; its diagonal is ``|grad y_k|^2``.
        ``weights``: None (all ones) or a float64 tensor of n_inp values on x's device, any sign.  ``y`` is `value_and_jacobian`'s, bit
        for bit.  No autograd graph is recorded (parameters are data); ``into=(y, M)`` reuses the caller's buffers.  The terms are
        summed in a fixed order and M[f, k, l], M[f, l, k] are stored from one value: the same bits on every call, M symmetric bit for
        bit, ``weights=None`` the bits of ``torch.ones``.  With G the same quantity of the features
        (`PreprocessingANN.value_and_metric`), ``sum_a w_a |grad_a y_k|^2 = dF_k G dF_k^T``, ``dF = d y / d feat``.
        `model.double()` and a float64 x on a HIP device; a model served by one fused plan with at most 64 outputs."""
        return self._one_launch_f64(_METRIC, self._one_launch_state(x, _METRIC, "float64"), x, weights, into)

    def value_and_restraint(self, x, center, kappa, period=None, flat=None, into=None):
        """``(y, energy, dx)`` with ``y = self(x)`` [N, d_out], the energy of a harmonic restraint on it
        ``energy[f] = 1/2 sum_k kappa_k d_k^2``, ``d_k = y[f, k] - center[f, k]`` [N], and ``dx = d energy / d x = J^T (kappa d)``
        [N, n_inp, 3] (the gradient, like `value_and_vjp`'s dx: forces are ``-dx``), float64, in ONE kernel launch
        (`molann_value_and_restraint_f64`, frames_value_restraint_f64_kernel): what umbrella sampling, steered MD, the string method's
        restrained replicas and TAMD's extended variable do with a collective variable at every step.  The cotangent ``kappa d``
        depends on y, so `value_and_vjp` needs a forward, four or five elementwise launches and then computes the forward again; here
        it is formed in the lanes that hold y.  ``center``: [d_out] (all frames) or [N, d_out]; ``kappa``: a float or [d_out], any
        sign; ``period``: None or [d_out], an entry > 0 wraps that output's d to ``d - P rint(d / P)`` (angles), an entry <= 0 leaves it;
        ``flat``: None or [d_out], an entry h > 0 gives that output a flat-bottomed well (``d = 0`` for ``|d| <= h``,
        ``copysign(|d| - h, d)`` beyond), a negative entry raises ValueError.  A float64 tensor on x's device passes as it is; a tensor
        of another floating dtype, a Python number or a sequence is converted, and each conversion costs a launch (a device ``flat``
        is read back once, when it is first seen or after it was written to).  ``y`` is `value_and_vjp`'s, bit for bit, and with
        ``period=None, flat=None`` so is ``dx`` for the cotangent ``kappa * (y - center)``.  A NaN poisons its own frame only.  No
        autograd graph is recorded (parameters are data); ``into=(y, energy, dx)`` reuses the caller's buffers.  The energy is summed
        in a fixed order and every row of dx is stored once: the same bits on every call.  `model.double()` and a float64 x on a HIP
        device; a model served by one fused plan.  Out of scope: float32, a `GraphedForces` replay of this launch, bias shapes other
        than this one, gradients with respect to parameters, centres or stiffnesses."""
        return self._one_launch_f64(_RESTRAINT, self._one_launch_state(x, _RESTRAINT, "float64"), x, (center, kappa, period, flat), into)

    def value_and_hills(self, x, centers, heights, sigma, period=None, into=None):
        """``(y, bias, dx)`` with ``y = self(x)`` [N, d_out], a metadynamics bias on it - a sum of H Gaussian hills -
        ``bias[f] = sum_h heights_h exp(-1/2 sum_k (d_hk / sigma_hk)^2)``, ``d_hk = y[f, k] - centers[h, k]`` [N], and
        ``dx = d bias / d x = J^T (d bias / d y)`` [N, n_inp, 3] (the gradient, like `value_and_vjp`'s dx: forces are ``-dx``), float64,
        in ONE kernel launch (`molann_value_and_hills_f64`, frames_value_hills_f64_kernel): what metadynamics does with a collective
        variable at every step, and what reweighting a stored trajectory under a final bias does on a large batch.  The cotangent
        depends on y, so `value_and_vjp` needs a forward, a dozen launches over an [N, H, d_out] temporary and then computes the forward
        again; here the lanes that hold y walk the hill table.  ``centers``: [H, d_out]; ``heights``: [H] or a float, any sign;
        ``sigma``: a float, [d_out] (all hills) or [H, d_out] (adaptive widths), > 0 everywhere or ValueError; ``period``: None or
        [d_out], an entry > 0 wraps that output's d to ``d - P rint(d / P)`` (angles), an entry <= 0 leaves it.  H may be 0 (the first
        step of a run): the bias and dx are zeros.  A float64 contiguous tensor on x's device passes as it is - the prefix
        ``centers[:h]`` of a preallocated table is one; a tensor of another floating dtype, a Python number or a sequence is converted,
        and each conversion costs a launch (a device ``sigma`` is read back once, when it is first seen or after it was written to:
        pass the same tensor every step, or views ``widths[:h]`` of the same table - adaptive widths are then read back after each
        deposit, which writes a row, and not on the steps between).  No cutoff: a far hill's exp underflows to 0.  ``y`` is `value_and_vjp`'s, bit for
        bit.  A NaN poisons its own frame only.  No autograd graph is recorded (parameters and hills are data);
        ``into=(y, bias, dx)`` reuses the caller's buffers.  Every sum has a fixed order and every row of dx is stored once: the same
        bits on every call, whatever N.  `model.double()` and a float64 x on a HIP device; a model served by one fused plan with at
        most 8 outputs (NotImplementedError beyond; hills on some of a wider model's outputs, or together with walls or a table:
        `value_and_bias`).  Out of scope: float32, a `GraphedForces` replay of this launch, depositing hills
        (append rows to your own tensors; well-tempered scaling uses the returned bias), cutoffs (a bias on a grid: `value_and_grid`), gradients with
        respect to parameters or hills."""
        return self._one_launch_f64(_HILLS, self._one_launch_state(x, _HILLS, "float64"), x, (centers, heights, sigma, period), into)

    def value_and_opes(self, x, centers, heights, sigma, scale, norm, epsilon, cutoff=None, period=None, into=None):
        """``(y, bias, dx)`` with ``y = self(x)`` [N, d_out], an OPES bias on it (on-the-fly probability enhanced sampling, PLUMED's
        ``OPES_METAD``) - not a sum of hills but the logarithm of a kernel density -
        ``bias[f] = scale log(P(y[f]) / norm + epsilon)``, ``P(y) = sum_h heights_h K_h(y)``,
        ``K_h = exp(-q_h / 2) - exp(-cutoff^2 / 2)`` where ``q_h = sum_k (d_hk / sigma_hk)^2 < cutoff^2`` and 0 elsewhere,
        ``d_hk = y[f, k] - centers[h, k]``, and ``dx = d bias / d x = J^T (d bias / d y)`` [N, n_inp, 3] (the gradient, like
        `value_and_vjp`'s dx: forces are ``-dx``), float64, in ONE kernel launch (`molann_value_and_opes_f64`,
        frames_value_opes_f64_kernel): the lanes that hold y walk the kernel table, as `value_and_hills` does, and take the logarithm
        where the sums are.  Kernel compression keeps an OPES table at 10^2 - 10^3 entries for a whole run, which is where that walk
        beats every other route.  ``centers`` [H, d_out], ``heights`` [H] or a float (the kernels' weights; negative ones are not
        checked and may take the logarithm's argument below 0: NaN or -inf for that frame), ``sigma`` a float, [d_out] or [H, d_out],
        > 0 everywhere or ValueError, ``period`` None or [d_out]: as `value_and_hills` takes them, with its conversions and its
        remembered ``sigma`` read-back (pass prefixes ``table[:h]`` of preallocated tensors).  ``scale`` (kT (1 - 1 / biasfactor)),
        ``norm`` (the normalisation Z times the sum of the weights), ``epsilon`` and ``cutoff`` are Python floats that travel in the
        launch's arguments, so changing Z at every deposit costs nothing: ``scale`` finite, ``norm`` and ``epsilon`` finite and > 0,
        ``cutoff`` None (no cutoff) or > 0, else ValueError before any launch.  A kernel is dropped where ``q_h >= cutoff^2``: the
        derivative jumps there, as in every OPES code.  H may be 0 (the first step of a run): the bias is ``scale log(epsilon)`` and dx
        zeros, and so they are for a frame outside every kernel's cutoff.  ``y`` is `value_and_vjp`'s, bit for bit.  A NaN poisons its
        own frame only, at a finite cutoff too.  No autograd graph is recorded (parameters and kernels are data);
        ``into=(y, bias, dx)`` reuses the caller's buffers.  Every sum has a fixed order and every row of dx is stored once: the same
        bits on every call, whatever N.  `model.double()` and a float64 x on a HIP device; a model served by one fused plan with at
        most 8 outputs (NotImplementedError beyond).  Out of scope: depositing, merging or compressing kernels and the update of Z
        (between steps, on your own tensors: `molann_amd.bias.opes_kernel_sum` gives P at the kernel centres; on the device:
        `molann_amd.bias.OpesTable`, and `value_and_opes_table` / `molann_amd.bias.OpesRun` for the whole loop), float32, a
        `GraphedForces` replay of this launch, neighbour lists, gradients with respect to the table or the parameters.  OPES on some of
        a wider model's outputs, or together with walls or a table: `value_and_bias` with ``opes=``."""
        return self._one_launch_f64(_OPES, self._one_launch_state(x, _OPES, "float64"), x,
                                    (centers, heights, sigma, scale, norm, epsilon, cutoff, period), into)

    def value_and_opes_table(self, x, table, scale, epsilon, into=None):
        """``(y, bias, dx)``: `value_and_opes` on a `molann_amd.bias.OpesTable`, with the live count and the normalisation read by the
        kernel from the table's state in device memory - ``n = state[0]`` held to ``[0, capacity]`` and ``norm = S / n = state[1] /
        state[0]``, OPES' ``Z kde_norm`` - instead of passed by value, float64, in ONE kernel launch
        (`molann_value_and_opes_table_f64`, frames_value_opes_table_f64_kernel).  Nothing is read back and nothing about the table is
        baked into the launch, so a bias and a deposit (`OpesTable.deposit`, `molann_amd.bias.OpesRun.deposit`) queue back to back
        step after step, and the pair can be captured once in a ``torch.cuda.graph`` and replayed while the table grows.  For the same
        n and norm, ``y``, ``bias`` and ``dx`` are `value_and_opes`' on ``table.record(scale, S / n, epsilon)``, bit for bit.
        ``table``: an `OpesTable` with ``table.d == d_out`` on x's device; its ``cutoff``, ``period`` and capacity are used.
        ``scale`` finite and ``epsilon`` finite and > 0, Python floats, else ValueError before any launch.  An empty table (the first
        step of a run): ``bias = scale log(epsilon)`` and dx zeros, and nothing of the table is read.  A state whose S is not finite
        and > 0 while n >= 1 gives NaN or inf for every frame: it is not guarded (`OpesTable.recompute_sum` restores S).  A NaN frame
        poisons its own outputs only.  No autograd graph is recorded; ``into=(y, bias, dx)`` reuses the caller's buffers.  The same
        bits on every call.  `model.double()` and a float64 x on a HIP device; a model served by one fused plan with at most 8
        outputs (on some of a wider model's outputs, or with walls or a table next to it: `value_and_bias` with
        ``opes=molann_amd.bias.OpesFromTable(...)``).  Out of scope: float32, a `GraphedForces` wrapper."""
        return self._one_launch_f64(_OPES_TABLE, self._one_launch_state(x, _OPES_TABLE, "float64"), x, (table, scale, epsilon), into)

    def value_and_grid(self, x, table, lower, spacing, periodic=None, into=None):
        """``(y, bias, dx)`` with ``y = self(x)`` [N, d_out], a bias interpolated from a table over it, ``bias[f] = V(y[f])`` [N], and
        ``dx = d bias / d x = J^T (d bias / d y)`` [N, n_inp, 3] (the gradient, like `value_and_vjp`'s dx: forces are ``-dx``), float64,
        in ONE kernel launch (`molann_value_and_grid_f64`, frames_value_grid_f64_kernel).  The table is what MD engines interpolate
        instead of walking 10^4 - 10^5 hills at every step - accumulated metadynamics hills (`molann_amd.bias.add_hills_to_grid`), a
        converged free-energy surface, an ABF or OPES estimate, a bias read from another program, walls - so a call costs the same
        whatever the table was made from: 4^d_out loads per frame.  ``table``: a float64 contiguous tensor on x's device with
        ``d_out <= 3`` dimensions of at least 4 points each, output 0 its slowest axis; it is read at launch as it is (nothing is
        converted or cached: update it in place between steps).  ``lower``, ``spacing``: sequences or CPU tensors of d_out floats,
        grid point i of axis k sits at ``lower[k] + i spacing[k]``, the spacing finite and > 0; ``periodic``: None or d_out bools, a
        periodic axis has period ``n_k spacing[k]`` (an angle: ``lower = -pi``, ``spacing = 2 pi / n_k``), any other spans
        ``[lower, lower + (n_k - 1) spacing]``.  They are host values and travel in the launch's arguments.  V is the
        cubic-convolution (Catmull-Rom) interpolant: four neighbours per axis, wrapped on a periodic axis, the edge's value repeated on
        any other; it takes the table's value at a grid point, is C1 inside the range and across the periodic seam, and ``dx`` is the
        exact gradient of V, so energy is conserved.  Its error against the function the table samples falls as h^3 (the derivative's
        as h^2).  Outside a non-periodic range the bias is the edge's value and that axis' derivative exactly 0: the derivative JUMPS
        at the range's ends, so keep walls and everything a trajectory visits inside the range.  ``y`` is `value_and_vjp`'s, bit for
        bit.  A NaN or an infinite output poisons its own frame only, and no table index leaves the table whatever y holds.  No autograd
        graph is recorded (parameters and the table are data); ``into=(y, bias, dx)`` reuses the caller's buffers.  Every sum has a
        fixed order and every row of dx is stored once: the same bits on every call, whatever N.  `model.double()` and a float64 x on a
        HIP device; a model served by one fused plan with at most 3 outputs (NotImplementedError beyond).  Out of scope: float32, more
        than 3 table axes (a table on some of a wider model's outputs, or together with walls or hills: `value_and_bias`), tables with stored derivatives, depositing into the table inside the launch,
        a `GraphedForces` replay of this launch, gradients with respect to the table or the parameters."""
        return self._one_launch_f64(_GRID, self._one_launch_state(x, _GRID, "float64"), x, (table, lower, spacing, periodic), into)

    def value_and_bias(self, x, restraint=None, hills=None, grid=None, into=None, opes=None):
        """``(y, energies, dx)`` with ``y = self(x)`` [N, d_out], up to three bias terms on chosen outputs, ``energies[f] = (E_r, V_h,
        V_g)`` [N, 3], and ``dx = d(E_r + V_h + V_g) / d x`` [N, n_inp, 3] (the gradient: forces are ``-dx``), float64, in ONE kernel
        launch (`molann_value_and_bias_f64`, frames_value_bias_f64_kernel): what a production step of enhanced sampling carries -
        metadynamics on a table plus walls, hills on top - for the cost of one pass over the frame, where `value_and_restraint`,
        `value_and_hills` and `value_and_grid` back to back compute the rotation, the features, the head and its backward three times.
        ``restraint``: a `molann_amd.bias.Restraint` ``(center, kappa, period=None, flat=None)`` on ALL outputs, as
        `value_and_restraint` takes them (``kappa[k] = 0`` leaves output k free).  ``hills``: a `molann_amd.bias.Hills` ``(centers,
        heights, sigma, period=None, columns=None)`` as `value_and_hills` takes them, on the outputs ``columns`` - distinct indices in
        any order, at most 8; ``centers`` [H, len(columns)], ``sigma`` and ``period`` are laid out in the order of the list; None
        means the first ``centers.shape[1]`` outputs.  ``grid``: a `molann_amd.bias.Grid` ``(table, lower, spacing, periodic=None,
        columns=None)`` as `value_and_grid` takes them, on at most 3 outputs, axis 0 of the table being the first listed.  The lists
        may overlap each other and the restrained outputs, so a model with any number of outputs takes a table on two of them.  Any
        term may be None, not all three (ValueError); an absent term's energy is exactly 0.  The three energies are kept apart:
        well-tempered heights and reweighting need ``V_h`` / ``V_g`` without the walls.  Periods, flat bottoms, per-frame centres,
        ``H = 0``, shared or per-hill widths, periodic or clamped axes, conversions and the remembered ``sigma`` / ``flat`` read-backs
        are the single calls'.  ``y`` is `value_and_vjp`'s, bit for bit; with one term alone on identity columns its energy and
        ``dx`` are the single call's, bit for bit.  An output's cotangent is the restraint's, then the hills' is added, then the
        table's: a fixed order, the same bits on every call, whatever N.  A frame that is not finite gets NaN and no other frame
        does.  Columns that are not integers, or a term that is not its record: TypeError; an index outside the outputs or repeated:
        IndexError; more than 8 / 3 columns: NotImplementedError.  No autograd graph is recorded; ``into=(y, energies, dx)`` reuses
        the caller's buffers.  `model.double()` and a float64 x on a HIP device; a model served by one fused plan.  Out of scope:
        float32, more than one term of a kind, a restraint on a list of columns (use ``kappa = 0``), a `GraphedForces` replay of this
        launch, gradients with respect to parameters or bias tables.

        ``opes``: a `molann_amd.bias.Opes` ``(centers, heights, sigma, scale, norm, epsilon, cutoff=None, period=None, columns=None)``, the
        kernel density of `value_and_opes` on the outputs ``columns`` (distinct, any order, at most 8; None: the first
        ``centers.shape[1]``) - an OPES run with walls (a flat-bottom ``restraint``) and, if there is one, a static table from an earlier
        run, on a model with any number of outputs, still ONE launch (`molann_value_and_bias_opes_f64`,
        frames_value_bias_opes_f64_kernel: a kernel of its own, `value_and_bias` without ``opes`` is what it was).  Then ``energies`` is
        [N, 4] ``= (E_r, V_h, V_g, V_o)``: columns 0 to 2 mean what they mean without ``opes``, ``V_h`` is exactly 0.0 and ``V_o = scale
        log(P / norm + epsilon)``; ``dx = d(E_r + V_o + V_g) / d x``, an output's cotangent being the restraint's, then the OPES
        derivative, then the table's.  The record's arguments are checked as `value_and_opes` checks them, with ``len(columns)`` in the
        place of d_out (conversions, the remembered ``sigma`` read-back, the scalars' ValueErrors); ``H = 0`` gives ``V_o = scale
        log(epsilon)`` and no share of dx.  With ``opes`` alone on identity columns ``V_o`` and ``dx`` are `value_and_opes`', bit for
        bit.  ``hills`` and ``opes`` together: NotImplementedError - move the hills onto a table with
        `molann_amd.bias.add_hills_to_grid` and pass it as ``grid``, or make two calls.  Out of scope as well: more than one OPES term,
        depositing or compressing kernels.

        ``opes`` may also be a `molann_amd.bias.OpesFromTable` ``(table, scale, epsilon, columns=None)``: the same term on an
        `OpesTable` where it lives, the live count ``n = state[0]`` (held to ``[0, capacity]``) and ``norm = S / n`` read by the kernel
        from the table's state in device memory as `value_and_opes_table` reads them (`molann_value_and_bias_opes_table_f64`,
        frames_value_bias_opes_table_f64_kernel, one launch).  Nothing is read back - no ``read_state()``, no widths looked at - so the
        call queues behind a deposit and is captured in a ``torch.cuda.graph`` while the table grows (`molann_amd.bias.OpesRun` with
        ``columns``, ``walls`` or ``grid`` is that loop).  ``(y, energies [N, 4], dx)`` and ``into`` as with an `Opes`; for the same n
        and norm they are the bits of ``opes=table.record(scale, S / n, epsilon, columns)``.  An empty table: ``V_o = scale
        log(epsilon)`` and no share of dx, nothing of the table read.  ``table.d`` columns on x's device, ``scale`` finite and
        ``epsilon`` finite and > 0, else ValueError before any launch; ``hills`` next to it: NotImplementedError as above."""
        _check_bias_terms("value_and_bias", restraint, hills, grid, opes)
        if opes is not None:
            kind = _BIAS_OPES_TABLE if isinstance(opes, _bias.OpesFromTable) else _BIAS_OPES
            return self._one_launch_f64(kind, self._one_launch_state(x, kind, "float64"), x, (restraint, grid, opes), into)
        return self._one_launch_f64(_BIAS, self._one_launch_state(x, _BIAS, "float64"), x, (restraint, hills, grid), into)

    def value_and_pbmetad(self, x, tables, kT, restraint=None, into=None):
        """``(y, energies, dx)`` with ``y = self(x)`` [N, d_out], a PARALLEL-BIAS METADYNAMICS bias on K <= 8 chosen outputs (Pfaendtner
        and Bonomi, JCTC 2015; PLUMED's ``PBMETAD``) and ``dx`` [N, n_inp, 3] the gradient of its sum with the walls, float64, in ONE
        kernel launch (`molann_value_and_pbmetad_f64`, frames_value_pbmetad_f64_kernel).  ``tables``: a `molann_amd.bias.PBTables`
        ``(table, shape, lower, spacing, periodic=None, columns=None)`` - K one-dimensional tables back to back in one float64 tensor
        on x's device, table k on output ``columns[k]`` (None: the first K).  ``energies`` [N, 2 + K] ``= (E_r, V_PB, V_0 .. V_{K-1})``:
        ``V_k`` is table k's cubic-convolution interpolant (`value_and_grid`'s on one axis: periodic or held at the edge's value outside
        its range), ``V_PB = m - kT log sum_k exp(-(V_k - m) / kT)`` with ``m = min_k V_k`` - the soft minimum
        ``-kT log sum_k exp(-V_k / kT)`` - and ``dx = J^T (dE_r/dy + w_k V_k')`` with ``w_k`` the axes' shares of that sum.  Memory and
        cost grow linearly in K, where a table over K outputs has n^K entries and `value_and_grid` serves 3.  ``kT``: a Python float
        > 0.  ``restraint``: None or a `molann_amd.bias.Restraint` on all outputs (walls), ``E_r`` exactly 0 without one.  With K = 1
        ``V_PB`` and ``dx`` are the single table's, bit for bit.  ``y`` is `value_and_vjp`'s, bit for bit.  A frame whose ``V_k`` is not
        finite gets NaN and no other frame does.  Every sum has a fixed order: the same bits on every call, whatever N.  Nothing is read
        back, so the call queues behind a deposit and is captured in a ``torch.cuda.graph`` while the tables grow
        (`molann_amd.bias.PBMetadRun` is that loop).  No autograd graph is recorded; ``into=(y, energies, dx)`` reuses the caller's
        buffers.  `model.double()` and a float64 x on a HIP device; a model served by one fused plan.  Out of scope: float32, c(t),
        per-axis kT, gradients with respect to the tables."""
        return self._one_launch_f64(_PBMETAD, self._one_launch_state(x, _PBMETAD, "float64"), x, (tables, kT, restraint), into)

    def _tangent_present(self, x):
        if _has_tangent(x):
            return True
        al = getattr(self.preprocessing_layer, "align_layer", None)
        if isinstance(al, AlignmentLayer) and _has_tangent(al.ref_x):
            return True
        return any(_has_tangent(p) for p in self.ann_layers.parameters())

    def last_launch_info(self):
        """Name + geometry of the kernels the last forward launched (bench / profiles / tests)."""
        st = self.__dict__.get("_fast")
        if st is not None and st.get("fused") and st.get("op") is not None:
            return torch.ops.molann.launch_info(st["desc"], st["sig"][5])
        return last_launch_info(self)

    def _fast_state(self, x):
        """Everything about this model that does not change from call to call (which modules it is made
        of, the recognised MLP, the plan), rebuilt only when the module tree or the device changes."""
        pp = self.preprocessing_layer
        nn = self.ann_layers
        fl = getattr(pp, "feature_layer", None)
        al = getattr(pp, "align_layer", None)
        sig = (id(pp), id(nn), id(fl), id(al), len(getattr(nn, "_modules", ())), x.device.index, self.mlp_precision)
        st = self.__dict__.get("_fast")
        if st is not None and st["sig"] == sig:
            return st
        rec = recognise_mlp(nn)
        st = {"sig": sig, "fused": False}
        if rec is not None and isinstance(pp, PreprocessingANN) and pp._fusable():
            linears, act = rec
            al = al if isinstance(al, AlignmentLayer) else None
            spec, uav = _feature_spec(fl)
            dims = [linears[0].in_features] + [lin.out_features for lin in linears]
            assert dims[0] == fl.output_dimension(), \
                'ann_layers expects %d inputs but the feature layer produces %d' % (dims[0], fl.output_dimension())

            def build():
                return _capi.Plan(fl.input_atom_num,
                                  align_idx=al._local_align_atom_indices if al is not None else None,
                                  ref_x=al.ref_x if al is not None else None,
                                  features=spec, use_angle_value=uav, layer_dims=dims, activation=act,
                                  mlp_precision=_capi.MLP_BF16 if self.mlp_precision == "bf16" else _capi.MLP_F32)

            tag = ("forward", tuple(dims), act, self.mlp_precision)
            st.update(fused=True, linears=linears, al=al, fl=fl, out_dim=dims[-1],
                      entry=lambda: _get_entry(self, x, tag, build),   # the ctypes plan, built when first needed
                      params=[p for lin in linears for p in (lin.weight, lin.bias)])
            # inference calls go through the dispatcher operator of csrc/molann_torch.cpp when that library is
            # built (same C ABI, same plan cache logic in C++): 8.5 us per call instead of 15.6 us through
            # ctypes for a 1024-frame batch (tools/latency_c1.py)
            st["op"] = _run_op()
            if st["op"] is not None:
                st["op_vjp"], st["op_jacobian"], st["op_metric"] = (torch.ops.molann.value_and_vjp_h, torch.ops.molann.value_and_jacobian_h,
                                                                    torch.ops.molann.value_and_metric_h)
                st["op_restraint"], st["op_hills"] = torch.ops.molann.value_and_restraint_h, torch.ops.molann.value_and_hills_h
                st["op_grid"], st["op_bias"] = torch.ops.molann.value_and_grid_h, torch.ops.molann.value_and_bias_h
                st["op_opes"], st["op_bias_opes"] = torch.ops.molann.value_and_opes_h, torch.ops.molann.value_and_bias_opes_h
                st["op_opes_table"], st["op_bias_opes_table"] = torch.ops.molann.value_and_opes_table_h, torch.ops.molann.value_and_bias_opes_table_h
                st["op_pbmetad"] = torch.ops.molann.value_and_pbmetad_h
                from . import script
                st["desc"] = script.make_desc(script.KIND_FORWARD, fl.input_atom_num,
                                              align_idx=al._local_align_atom_indices if al is not None else None,
                                              features=spec, use_angle_value=uav, layer_dims=dims, activation=act,
                                              mlp_precision=_capi.MLP_BF16 if self.mlp_precision == "bf16" else _capi.MLP_F32)
                st["no_ref"] = torch.zeros(0, 3)
                st["handle"] = torch.ops.molann.register_desc(st["desc"])
                import weakref
                weakref.finalize(self, _release_plans, st["desc"], x.device.index)
                # the inference fast path of forward(): everything it compares or passes, looked up once
                self.__dict__["_fp"] = (x.device, (fl.input_atom_num, 3), pp, nn, al, fl, len(nn._modules), st["handle"], torch.ops.molann.run_h,
                                        st["no_ref"], [lin._parameters for lin in linears], self.mlp_precision)
        if not (st["fused"] and st.get("op") is not None):
            self.__dict__.pop("_fp", None)
        self.__dict__["_fast"] = st
        return st

    def forward(self, x):
        # ---- forward mode: a tangent on x or on the ann_layers parameters (fwAD dual, torch.func transform).  The preprocessing
        # layer's tangent kernel, then ann_layers as the torch module it is (torch's forward AD of Linear and the activations).
        if _transform_active() and self._tangent_present(x):
            return self.ann_layers(self.preprocessing_layer(x))
        # ---- inference fast path (a 1024-frame call is ~3 us of kernel: the host side is what a caller waits for; tools/latency_breakdown.py).
        # Taken only when nothing it skips could matter: the same module objects as when the plan was made, a float32 [N > 0, n_inp, 3]
        # tensor on the plan's device, nothing to record for autograd.  Everything else takes the general path below, checks and all.
        fp = self.__dict__.get("_fp")
        if fp is not None and type(x) is torch.Tensor and x.dtype is torch.float32 and x.device == fp[0] and x.dim() == 3 \
                and tuple(x.shape[1:]) == fp[1] and x.shape[0] > 0:
            mods = self._modules
            pp, nn = fp[2], fp[3]
            if mods["preprocessing_layer"] is pp and mods["ann_layers"] is nn and len(nn._modules) == fp[6] and self.mlp_precision == fp[11] \
                    and pp._modules["feature_layer"] is fp[5] and (pp._modules["align_layer"] is fp[4] or fp[4] is None and type(pp._modules["align_layer"]) is torch.nn.Identity):
                plist = fp[10]
                grad = torch.is_grad_enabled() and (x.requires_grad or any(d["weight"].requires_grad or d["bias"].requires_grad for d in plist))
                ref = fp[4]._buffers["ref_x"] if fp[4] is not None else fp[9]
                w0 = plist[0]["weight"]
                if not grad and w0.dtype is torch.float32 and w0.device == fp[0] and (fp[4] is None or (ref.dtype is torch.float32 and ref.device == fp[0])):
                    return fp[8](x, fp[7], ref, [d["weight"] for d in plist], [d["bias"] for d in plist])
        assert isinstance(x, torch.Tensor), 'Input x is not a torch tensor'
        st = self._fast_state(x) if x.is_cuda else None
        if st is None or not st["fused"]:
            if recognise_mlp(self.ann_layers) is None or not (isinstance(self.preprocessing_layer, PreprocessingANN)
                                                              and self.preprocessing_layer._fusable()):
                return self.ann_layers(self.preprocessing_layer(x))
            _check_input(x, self.preprocessing_layer.feature_layer.input_atom_num)
            _device_input(x)          # raises: not a device tensor
        al, fl = st["al"], st["fl"]
        if al is not None:
            _check_input(x, al.input_atom_num)
        _check_input(x, fl.input_atom_num)
        x = _device_input(x, grad_sources=st["params"], backward_ok=True)
        if x.shape[0] == 0:
            return torch.empty((0, st["out_dim"]), dtype=x.dtype, device=x.device)
        if x.dtype == torch.float64 and _wants_grad(x, st["params"]):
            # float64 training / forces: features and their gradient from the float64 kernels, ann_layers as the torch module it is
            return self.ann_layers(self.preprocessing_layer(x))
        if x.dtype == torch.float64:
            # `model.double()(x.double())`: the float64 kernels, the Linear parameters read as they are
            lins = st["linears"]
            w0 = lins[0].weight
            if w0.device != x.device or w0.dtype != torch.float64:
                raise RuntimeError("ann_layers must be float64 on %s for a float64 input (got %s on %s): call .double()"
                                   % (x.device, w0.dtype, w0.device))
            entry = st["entry"]()
            with torch.cuda.device(x.device):
                if al is not None:
                    entry.sync_ref(_device_buffer(al.ref_x, x))
                work = torch.empty((x.shape[0], entry.plan.feature_dim), dtype=torch.float64, device=x.device)
                out = torch.empty((x.shape[0], st["out_dim"]), dtype=torch.float64, device=x.device)
                entry.plan.forward_f64(x, [lin.weight.detach().contiguous() for lin in lins],
                                       [lin.bias.detach().contiguous() for lin in lins], work, out)
            return out
        if _wants_grad(x, st["params"]):
            w0 = st["linears"][0].weight
            if w0.device != x.device or w0.dtype != torch.float32:
                raise RuntimeError("ann_layers must be float32 on %s (got %s on %s)" % (x.device, w0.dtype, w0.device))
            if st.get("fused_bwd") is None:           # asked once: the answer is a property of the plan
                with torch.cuda.device(x.device):
                    if st["op"] is not None:
                        st["fused_bwd"] = bool(torch.ops.molann.supports_backward(
                            x, st["desc"], _device_buffer(al.ref_x, x) if al is not None else st["no_ref"]))
                    else:
                        st["fused_bwd"] = bool(st["entry"]().plan.supports_backward())
            if st["fused_bwd"] and st["op"] is not None:
                # the dispatcher operator's autograd node (csrc/molann_torch.cpp): the same kernels and the same choice between the
                # one-pass backward and the MLP's backward on kept features when x is data.  A training step costs ~100 us of
                # host time through it against ~195 through the Python autograd.Function below (tools/host_overhead.py)
                lins = st["linears"]
                return st["op"](x, st["desc"], _device_buffer(al.ref_x, x) if al is not None else st["no_ref"],
                                [lin.weight for lin in lins], [lin.bias for lin in lins])
            if st["fused_bwd"]:
                entry = st["entry"]()
                with torch.cuda.device(x.device):
                    if al is not None:
                        entry.sync_ref(_device_buffer(al.ref_x, x))
                    entry.sync_mlp(st["linears"])
                    return _PlanFunction.apply(x, entry, True, *st["params"])
            if st.get("head_bwd") is None:            # asked once, like fused_bwd
                with torch.cuda.device(x.device):
                    if st["op"] is not None:
                        st["head_bwd"] = bool(torch.ops.molann.supports_mlp_backward(
                            x, st["desc"], _device_buffer(al.ref_x, x) if al is not None else st["no_ref"]))
                    else:
                        st["head_bwd"] = bool(st["entry"]().plan.supports_mlp_backward())
            if st["head_bwd"]:
                # A wide fp32 head with a HIP backward (molann_chain_bwd): the preprocessing layer's node, then the head's.  Through
                # the dispatcher operator where that library is built (the plan its launch info reports), else the Function above.
                feat = self.preprocessing_layer(x)
                if feat.dtype != torch.float32 or not feat.is_contiguous():
                    feat = feat.float().contiguous()
                lins = st["linears"]
                if st["op"] is not None:
                    return torch.ops.molann.run_head(feat, st["desc"], _device_buffer(al.ref_x, x) if al is not None else st["no_ref"],
                                                     [lin.weight for lin in lins], [lin.bias for lin in lins])
                entry = st["entry"]()
                with torch.cuda.device(x.device):
                    return _HeadFunction.apply(feat, entry, lins, *st["params"])
            # No HIP backward for the head (ELU, GELU, Softplus; bf16 or streaming heads; no hipRTC).  Training still works when the
            # preprocessing has one (small frames): features and their gradient from the HIP kernels, the MLP and
            # its gradient as the user's own torch module on the device - what already happens for ann_layers
            # this file does not recognise.  Large frames raise inside the preprocessing layer.
            return self.ann_layers(self.preprocessing_layer(x))
        w0 = st["linears"][0].weight
        if w0.device != x.device or w0.dtype != torch.float32:
            raise RuntimeError("ann_layers must be float32 on %s (got %s on %s)" % (x.device, w0.dtype, w0.device))
        if st["op"] is not None:
            lins = st["linears"]   # nothing here requires grad under an enabled grad mode: the operator records nothing
            return st["op"](x, st["desc"], _device_buffer(al.ref_x, x) if al is not None else st["no_ref"],
                            [lin.weight for lin in lins], [lin.bias for lin in lins])
        entry = st["entry"]()
        out = torch.empty((x.shape[0], st["out_dim"]), dtype=torch.float32, device=x.device)
        if x.device.index == torch.cuda.current_device():
            if al is not None:
                entry.sync_ref(_device_buffer(al.ref_x, x))
            entry.sync_mlp(st["linears"])
            entry.plan.forward_packed(x, out)
        else:
            with torch.cuda.device(x.device):
                if al is not None:
                    entry.sync_ref(_device_buffer(al.ref_x, x))
                entry.sync_mlp(st["linears"])
                entry.plan.forward_packed(x, out)
        return out
