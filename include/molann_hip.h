/*
 * molann_hip.h - C ABI of the MI355X (gfx950) implementation of molann's per-frame forward path
 *
 *     x[N, n_inp, 3]  ->  AlignmentLayer (Kabsch)  ->  FeatureLayer  ->  MLP  ->  y[N, d_out]
 *
 * The reference (zwpku/molann v1.1.7) is pure Python: it has no FFI for this path.  The interface a
 * replacement sits behind is the forward of its torch.nn.Modules (molann/ann.py); each entry point
 * below names the reference method it replaces.  A host binding (ctypes, see INTEGRATION.md, and
 * molann_amd/_capi.py) builds one immutable plan per module and then calls the launch functions with
 * raw device pointers.
 *
 * Conventions
 *   - return value: 0 = ok; negative = MOLANN_E_* (bad argument / unsupported); positive = hipError_t.
 *   - every `x`, `out`, `W[i]`, `b[i]`, `ref_x` passed to a LAUNCH function is a DEVICE pointer owned
 *     by the caller; pointers inside molann_plan_desc are HOST pointers, read during plan_create only.
 *   - launch functions only enqueue work on `stream`: no host synchronisation, no allocation
 *     (graph-capturable).  They are thread-safe for distinct plans; one plan may be used from several
 *     streams as long as molann_plan_update_* calls are ordered before the launches that need them.
 *     A plan whose MLP is not fused into the frame kernel (wide MLPs / large frames) owns a feature
 *     workspace, a side stream and events: its forward calls are serialised by the library itself (a
 *     host mutex around the enqueue; a caller on another stream first waits for the event recorded
 *     behind the previous call), so they are safe from any stream or thread but do not overlap.
 *     The same protocol covers the backward's plan-owned workspaces (per-block parameter sums; the recomputed
 *     features of the three-launch path).  The FIRST call of an entry point whose kernel is built lazily (the
 *     backward kernels, molann_forward_train_f32, molann_features_f32 on a plan with a fused MLP, molann_align_f32
 *     on small frames) compiles it with hipRTC and may allocate its workspace: make that call outside a graph
 *     capture (molann_plan_backward_kind builds the backward ahead of time).
 *   - x is [n_frames, n_inp, 3] fp32, contiguous, frame-major / atom-major / xyz-minor (the layout of
 *     the tensor the reference's forward receives, ann.py:170).
 *   - Caller's buffers.  Every DEVICE pointer a call takes - x, cotangents, tangents, outputs, gradients, feature rows, tables, and
 *     the ref_x / W[i] / b[i] tensors - may point anywhere into a larger array of the caller's, aligned to its element: 4 bytes
 *     for the float32 entries, 8 for the float64 ones; a pointer that is not is refused with MOLANN_E_ALIGNMENT before anything
 *     is launched or written.  Nothing more is asked: 16-byte aligned pointers take the wide loads and stores, others the narrow
 *     ones, each buffer by its own address, with the same bits either way.  A call reads nothing outside its inputs and writes
 *     exactly its outputs' elements - never a byte before, between or behind them, whatever n_frames, the frame size and the
 *     output width are (tests/test_gpu_buffer_placement.py holds every entry to this inside guard bands).
 *   - Frames are independent.  A value that is not finite (NaN, +-Inf) in one frame's rows of x, of a cotangent, of a tangent or
 *     of a feature row makes that frame's results that depend on it non-finite and changes no bit of any other frame's results,
 *     whatever n_frames is and wherever in the batch the frame sits.  "Depend": the feature columns whose item names the atom (a
 *     position item's through the centroid, when the atom is aligned on), every head output, the energies and biases, and the
 *     gradient, Jacobian and tangent rows of atoms that share a bond, angle or dihedral with it; the rotation of a frame whose
 *     covariance is not finite is the identity, so rows that see the atom through the rotation alone may stay finite; +-Inf
 *     behind a saturating activation is a finite number, and a bond of length Inf has gradient 0 in the coordinates that stayed
 *     finite.  The sums over frames (grad_params) are the exception, as in torch: one such frame makes the elements it reaches NaN.
 *     tests/test_gpu_frame_isolation.py holds every entry to this.
 *   - n_frames == 0 is legal and does nothing (the reference returns an empty tensor).
 *   - code object: gfx950 only.
 */
#ifndef MOLANN_HIP_H
#define MOLANN_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MOLANN_ABI_VERSION 1

/* feature type ids: molann/feature.py:87-97 */
#define MOLANN_FEAT_ANGLE 0
#define MOLANN_FEAT_BOND 1
#define MOLANN_FEAT_DIHEDRAL 2
#define MOLANN_FEAT_POSITION 3

/* activation between the Linear layers of create_sequential_nn (ann.py:37,64) */
#define MOLANN_ACT_TANH 0
#define MOLANN_ACT_RELU 1
#define MOLANN_ACT_SIGMOID 2
#define MOLANN_ACT_IDENTITY 3
#define MOLANN_ACT_ELU 4
#define MOLANN_ACT_SILU 5
#define MOLANN_ACT_SOFTPLUS 6
#define MOLANN_ACT_LEAKY_RELU 7 /* slope 0.01 */
#define MOLANN_ACT_GELU 8       /* erf form (torch.nn.GELU default) */

/* MLP arithmetic */
#define MOLANN_MLP_F32 0  /* fp32 weights, fp32 FMA / fp32-input MFMA (exact fp32) */
#define MOLANN_MLP_BF16 1 /* bf16 weights + activations, fp32 accumulate on bf16 MFMA */

#define MOLANN_MAX_LAYERS 16

/* error codes (negative) */
#define MOLANN_OK 0
#define MOLANN_E_NULL (-1)        /* a required pointer is NULL */
#define MOLANN_E_DESC (-2)        /* inconsistent plan description (sizes, counts) */
#define MOLANN_E_INDEX (-3)       /* an atom index is outside [0, n_inp) */
#define MOLANN_E_FEATURE (-4)     /* unknown feature type or wrong atom count for its type */
#define MOLANN_E_STAGE (-5)       /* the plan lacks the stage this call needs (no align / features / MLP) */
#define MOLANN_E_ALIGNMENT (-6)   /* pointer not aligned to its element: 4 bytes (float32 entries), 8 (float64 entries) */
#define MOLANN_E_UNSUPPORTED (-7) /* shape outside what the kernels cover */
#define MOLANN_E_NOT_PACKED (-8)  /* forward_packed before any plan_update_mlp */
#define MOLANN_E_DEVICE (-9)      /* no gfx950 device */

typedef struct molann_plan molann_plan;         /* opaque; owns a small device blob */
typedef struct ihipStream_t* molann_stream_t;   /* == hipStream_t */

/*
 * Everything the modules fix at construction time.
 *   AlignmentLayer.__init__  ann.py:123-146  -> n_align, align_idx (= _local_align_atom_indices), ref_x
 *   FeatureMap.__init__      ann.py:244-263  -> feat_type / feat_idx (= _local_atom_indices), use_angle_value
 *   FeatureLayer.__init__    ann.py:418-427  -> the list order = output column order (ann.py:473)
 *   create_sequential_nn     ann.py:37-67    -> layer_dims, activation
 * A stage that is absent has its count set to 0.
 */
typedef struct molann_plan_desc {
    int32_t abi_version;       /* MOLANN_ABI_VERSION */
    int32_t n_inp;             /* atoms per frame, ann.py:133 */

    int32_t n_align;           /* 0: no AlignmentLayer (PreprocessingANN uses Identity, ann.py:542) */
    const int32_t* align_idx;  /* [n_align] positions inside the n_inp axis, ann.py:144 */
    const float* ref_x;        /* [n_align*3] reference coordinates ALREADY centred, ann.py:140-141 */

    int32_t n_features;        /* 0: no FeatureLayer */
    const int32_t* feat_type;  /* [n_features] MOLANN_FEAT_* */
    const int32_t* feat_ptr;   /* [n_features+1] offsets into feat_idx */
    const int32_t* feat_idx;   /* positions inside the n_inp axis, ann.py:261, in the order given */
    int32_t use_angle_value;   /* ann.py:253 */

    int32_t n_layers;          /* number of Linear layers; 0: no MLP */
    const int32_t* layer_dims; /* [n_layers+1]; layer_dims[0] must equal the feature dimension */
    int32_t activation;        /* MOLANN_ACT_* */
    int32_t mlp_precision;     /* MOLANN_MLP_* */
} molann_plan_desc;

/* -- plan ------------------------------------------------------------------------------------- */

/* Validates the description (the reference raises ValueError / AssertionError for the same
 * conditions at module construction, ann.py:146,263,423 and feature.py:88-94), copies it to the
 * current device and returns the plan.  Allocates; call once per module. */
int molann_plan_create(const molann_plan_desc* desc, molann_plan** out_plan);
int molann_plan_destroy(molann_plan* plan);

/* FeatureLayer.output_dimension() ann.py:446-452 (0 when the plan has no features). */
int molann_plan_feature_dim(const molann_plan* plan);
/* Width of what molann_forward_* writes: last layer_dims entry, or the feature dim without an MLP. */
int molann_plan_out_dim(const molann_plan* plan);
/* Which kernel family serves the frames of this plan: 0 = lane-per-frame (LDS-staged small frames),
 * 1 = wave-per-frame (gathered large frames). */
int molann_plan_kernel_family(const molann_plan* plan);

/* The module's `ref_x` buffer is live state (register_buffer, ann.py:137: load_state_dict / .to()
 * can replace it).  Re-reads it from DEVICE memory [n_align*3], already centred (4-byte aligned, as every float32 pointer). */
int molann_plan_update_ref(molann_plan* plan, const float* ref_x, molann_stream_t stream);

/* The Linear parameters are live (trainable).  Re-reads W[i] ([dims[i+1], dims[i]] row-major,
 * torch.nn.Linear layout) and b[i] ([dims[i+1]]) from DEVICE memory into the plan's packed copy.
 * W and b themselves are HOST arrays of n_layers device pointers. */
int molann_plan_update_mlp(molann_plan* plan, const float* const* W, const float* const* b,
                           molann_stream_t stream);

/* -- launches --------------------------------------------------------------------------------- */

/* AlignmentLayer.forward ann.py:157-199: out_xyz[N, n_inp, 3] = (x - c(x)) . R(x). */
int molann_align_f32(const molann_plan* plan, const float* x, int64_t n_frames, float* out_xyz,
                     molann_stream_t stream);

/* PreprocessingANN.forward ann.py:553-565 (= FeatureLayer.forward ann.py:454-474 when the plan has
 * no alignment): out[N, feature_dim]. */
int molann_features_f32(const molann_plan* plan, const float* x, int64_t n_frames, float* out,
                        molann_stream_t stream);

/* MolANN.forward ann.py:620-624 with the packed copy of the weights: out[N, out_dim]. */
int molann_forward_packed_f32(const molann_plan* plan, const float* x, int64_t n_frames, float* out,
                              molann_stream_t stream);

/* MolANN.forward reading the live parameters: molann_plan_update_mlp + molann_forward_packed_f32. */
int molann_forward_f32(molann_plan* plan, const float* x, int64_t n_frames, const float* const* W,
                       const float* const* b, float* out, molann_stream_t stream);

/* ann_layers alone on precomputed features f[N, layer_dims[0]] (create_sequential_nn's Sequential,
 * ann.py:60-65): out[N, out_dim].  Uses the packed weights. */
int molann_mlp_packed_f32(const molann_plan* plan, const float* f, int64_t n_frames, float* out,
                          molann_stream_t stream);

/* -- float64 ---------------------------------------------------------------------------------- */
/* The reference's modules follow x.dtype: after `model.double()` the same forward runs in float64 (ann.py:187-197,
 * 323-354).  These entry points are that mode: x, out, W[i], b[i], ref_x are DEVICE pointers to
 * doubles (8-byte aligned), the plan is the same one (index tables do not depend on the dtype).  Everything is
 * computed in double; nothing is packed: the Linear parameters are read from the caller's tensors at every call.
 * Written for agreement with the reference's float64 run to rounding, not for speed (one wave per frame). */

/* The `ref_x` buffer of a `.double()` AlignmentLayer: DEVICE [n_align*3] doubles, already centred. */
int molann_plan_update_ref_f64(molann_plan* plan, const double* ref_x, molann_stream_t stream);
/* AlignmentLayer.forward ann.py:157-199 in float64. */
int molann_align_f64(const molann_plan* plan, const double* x, int64_t n_frames, double* out_xyz, molann_stream_t stream);
/* PreprocessingANN.forward / FeatureLayer.forward ann.py:454-474, 553-565 in float64: out[N, feature_dim]. */
int molann_features_f64(const molann_plan* plan, const double* x, int64_t n_frames, double* out, molann_stream_t stream);
/* dL/dx of molann_features_f64 for the same x (the reference differentiates its float64 forward with autograd too):
 * grad_f[N, feature_dim] -> grad_x[N, n_inp, 3], doubles, any frame size.  The MLP of a float64 model is differentiated by
 * the caller (torch autograd over its own Linear modules). */
int molann_features_backward_f64(const molann_plan* plan, const double* x, const double* grad_f, int64_t n_frames, double* grad_x,
                                 molann_stream_t stream);

/* -- forward mode ----------------------------------------------------------------------------- */
/* Directional derivatives of the feature stage (what torch.autograd.forward_ad, torch.func.jvp and torch.func.jacfwd ask
 * the reference's autograd for): tangent_out[t] = J(x) v[t], the Jacobian of molann_features_f32 / _f64 at x applied to
 * each of n_tangents >= 1 tangents.  v is [n_tangents, n_frames, n_inp, 3] and tangent_out [n_tangents, n_frames,
 * feature_dim], contiguous; out[n_frames, feature_dim] receives the features themselves (nullable: then not written).  The
 * tangents of a frame share one read of x, one rotation solve and one evaluation of the features: a frame's Jacobian
 * (3 n_inp tangents) costs one solve.  Every plan with feature items, any frame size, with or without a head (the feature
 * stage only, like molann_features_f32).  Everything is computed in double and rounded on the store (frames_jvp_kernel;
 * lane groups of 8..64 per frame; no atomics, so the results are identical run to run).  Pointers 4-byte (f32) / 8-byte
 * (f64) aligned; n_tangents < 1: MOLANN_E_DESC. */
int molann_features_jvp_f32(const molann_plan* plan, const float* x, const float* v, int64_t n_frames, int n_tangents, float* out,
                            float* tangent_out, molann_stream_t stream);
int molann_features_jvp_f64(const molann_plan* plan, const double* x, const double* v, int64_t n_frames, int n_tangents, double* out,
                            double* tangent_out, molann_stream_t stream);

/* -- second order ----------------------------------------------------------------------------- */
/* The derivative of molann_features_backward_f64 along a direction, for create_graph=True through the float64 features (a
 * loss on forces): for a cotangent g[n_frames, feature_dim] and a direction u[n_frames, n_inp, 3],
 *   hx[n_frames, n_inp, 3]       = d/dx <u, J(x)^T g> = sum_k g_k Hess f_k(x) u   (the second-order adjoint),
 *   hg[n_frames, feature_dim]    = J(x) u.
 * Exact: the float64 backward's closed forms differentiated on a dual number, the rotation's tangent from the closed form of
 * its adjoint (no difference quotients, no step).  Every plan with feature items (as molann_features_backward_f64), any frame
 * size.  One launch (frames_hvp_f64_kernel; lane groups of 8..64 per frame; no atomics, so the results are identical run to
 * run).  All pointers 8-byte aligned, contiguous. */
int molann_features_hvp_f64(const molann_plan* plan, const double* x, const double* g, const double* u, int64_t n_frames, double* hx,
                            double* hg, molann_stream_t stream);

/* ann_layers ann.py:60-65 in float64 on features f[N, layer_dims[0]]: W, b HOST arrays of n_layers device pointers. */
int molann_mlp_f64(const molann_plan* plan, const double* f, int64_t n_frames, const double* const* W, const double* const* b,
                   double* out, molann_stream_t stream);
/* MolANN.forward ann.py:620-624 in float64; features_work is a caller-owned DEVICE buffer of n_frames * feature_dim
 * doubles (launch functions do not allocate). */
int molann_forward_f64(const molann_plan* plan, const double* x, int64_t n_frames, const double* const* W, const double* const* b,
                       double* features_work, double* out, molann_stream_t stream);

/* -- backward (the reference relies on torch autograd, incl. through its SVD) -------- */

/* Floats of the parameter-gradient buffer: for every Linear layer dW[J][K] (torch layout) then db[J]. */
int molann_plan_grad_params_size(const molann_plan* plan);

/* 1 if molann_backward_f32 can serve this plan (see below), else 0. */
int molann_plan_supports_backward(const molann_plan* plan);

/* How molann_backward_f32 serves this plan: 2 = one pass over x (recompute + MLP on the matrix cores + reverse mode in one
 * kernel: nothing worth saving from the forward), 1 = two or three launches (a caller that keeps the features of its
 * forward, molann_forward_train_f32, saves their recompute), 0 = not at all.  Builds the kernel it reports (hipRTC). */
int molann_plan_backward_kind(molann_plan* plan);

/* Gradients of molann_forward_packed_f32 (plans with an MLP) / molann_features_f32 (plans without) for the
 * same x: grad_out[N, out_dim] -> grad_x[N, n_inp, 3] (written; zeros for atoms the plan does not touch;
 * may be NULL) and grad_params (ACCUMULATED into with float atomics, so zero it first; may be NULL).
 * Nothing is saved from the forward.  One launch (molann_plan_backward_kind 2: loaders stream x through a ring in LDS,
 * consumers recompute the forward per frame, run the MLP's backward on the matrix cores and the analytic reverse mode
 * of the preprocessing) plus the reduction of the per-block parameter sums; where that kernel cannot be built, plans
 * with an MLP run three launches per chunk of frames - the features (recomputed into a workspace the plan allocates at
 * its first backward), molann_mlp_backward_f32 and molann_features_backward_f32 - and a caller that kept the features
 * of its forward (molann_forward_train_f32) calls those two itself and saves the recompute.
 * Available for plans served by the lane-per-frame kernel with the MLP fused (or no MLP) and tanh / ReLU /
 * sigmoid / identity / SiLU / LeakyReLU (kernels compiled with hipRTC at the first call); for feature
 * plans without an MLP on large frames (one wave per frame; frames up to 1024 atoms with an alignment: eight / four / two
 * frames per wave and round); and for large-frame plans whose MLP is within the fused MLP's limits (every width and the
 * feature dim <= 32, <= 4 layers, the activations above): the three launches, the features recomputed by the plan's
 * forward kernel; otherwise MOLANN_E_UNSUPPORTED. */
int molann_backward_f32(molann_plan* plan, const float* x, const float* grad_out, int64_t n_frames, float* grad_x,
                        float* grad_params, molann_stream_t stream);

/* out[N, out_dim] = molann_forward_packed_f32(x) (molann_features_f32(x) for a plan without an MLP; MolANN.forward ann.py:620-624)
 * AND grad_x[N, n_inp, 3] = the vector-Jacobian product for the cotangent grad_out[N, out_dim], in ONE launch: the one-pass
 * backward recomputes the forward per frame anyway; this build of it also stores the outputs.  For a host that differentiates a
 * small batch at every step (a collective variable and its forces inside an MD engine, README.rst:49): one launch instead of a
 * forward and a backward.  The Jacobian of one frame: a batch of out_dim copies of it with the identity as grad_out.  Parameters
 * are data (no parameter gradients).  Served: plans with molann_plan_backward_kind == 2, and frames too large for the lane
 * kernels (mid-size and large frames, backward kind 1) whose head is within the fused MLP's limits - every width and the feature
 * dimension <= 32, <= 4 layers, fp32, tanh / ReLU / sigmoid / identity / SiLU / LeakyReLU - or that have no head: one
 * plan-specialised kernel (molann_group_vjp) for forward_train + mlp_backward + features_backward.  MOLANN_E_UNSUPPORTED otherwise
 * (see molann_plan_supports_value_and_vjp).  First call: hipRTC, outside a capture; after that the call only enqueues on
 * `stream` (no workspace, no event): thread-safe and capturable. */
int molann_value_and_vjp_f32(molann_plan* plan, const float* x, const float* grad_out, int64_t n_frames, float* out,
                             float* grad_x, molann_stream_t stream);

/* 1 when molann_value_and_vjp_f32 serves the plan, 0 otherwise.  Builds the kernel it reports (call it before a capture). */
int molann_plan_supports_value_and_vjp(molann_plan* plan);

/* molann_value_and_vjp_f32 in float64 (`model.double()`): out[N, out_dim] = molann_forward_f64(x) (molann_features_f64(x) for a
 * plan without an MLP) AND grad_x[N, n_inp, 3] = the vector-Jacobian product for grad_out[N, out_dim], everything in double, in
 * ONE launch of frames_value_vjp_f64_kernel (ahead of time: no hipRTC).  W, b as molann_forward_f64 takes them (HOST arrays of
 * n_layers device pointers to the torch.nn.Linear tensors, read as they are; ignored - may be NULL - for a plan without an MLP).
 * Parameters are data.  Every plan with feature items, with or without an alignment, any frame size, any head (all nine
 * activations); lane groups of 8..64 per frame.  Each row of grad_x is stored once (zeros for atoms the plan does not touch), its
 * terms summed in a plan-time order: no atomics, the same bits on every run.  MOLANN_E_STAGE for a plan without items,
 * MOLANN_E_UNSUPPORTED only where one frame's rows (feature_dim + the hidden widths + twice the widest of them, in doubles)
 * exceed the LDS of a compute unit.  All pointers 8-byte aligned, contiguous.  The call only enqueues on `stream` (no workspace, no
 * event): thread-safe and capturable. */
int molann_value_and_vjp_f64(molann_plan* plan, const double* x, const double* grad_out, int64_t n_frames, const double* const* W,
                             const double* const* b, double* out, double* grad_x, molann_stream_t stream);

/* 1 when molann_value_and_vjp_f64 serves the plan (feature items, and a frame's rows fit the LDS), 0 otherwise. */
int molann_plan_supports_value_and_vjp_f64(const molann_plan* plan);

/* Values AND the full Jacobian of a float64 model in ONE launch of frames_value_jac_f64_kernel (ahead of time: no hipRTC):
 * out[N, out_dim] = molann_value_and_vjp_f64's out, bit for bit, and jac[N, out_dim, n_inp, 3] with jac[f, k] = d out[f, k] / d x[f]
 * (out_dim = feature_dim for a plan without an MLP), everything in double.  x, the Kabsch solve, the features and the head forward
 * are read and computed once per frame, each item's backward once per output column of the item; the out_dim rows are linear
 * combinations of those.  W, b as molann_value_and_vjp_f64 takes them.  Every row of every jac[f, k] is stored once (zeros for atoms
 * the plan does not touch), its terms summed in a plan-time order: no atomics, the same bits on every run.  MOLANN_E_STAGE for a
 * plan without items, MOLANN_E_UNSUPPORTED where one frame's rows (feature_dim + the hidden widths + 2 out_dim times the widest
 * layer input, + 12 out_dim with an alignment, in doubles) exceed the LDS of a compute unit.  n_frames < 0: MOLANN_E_DESC;
 * n_frames == 0: nothing is read or launched.  All pointers 8-byte aligned, contiguous.  The call only enqueues on `stream` (no
 * workspace, no event): thread-safe and capturable. */
int molann_value_and_jacobian_f64(molann_plan* plan, const double* x, int64_t n_frames, const double* const* W, const double* const* b,
                                  double* out, double* jac, molann_stream_t stream);

/* 1 when molann_value_and_jacobian_f64 serves the plan (feature items, and a frame's rows fit the LDS), 0 otherwise. */
int molann_plan_supports_value_and_jacobian_f64(const molann_plan* plan);

/* Values AND the metric tensor of a float64 model in ONE launch of frames_value_metric_f64_kernel (ahead of time: no hipRTC):
 * out[N, out_dim] = molann_value_and_jacobian_f64's out, bit for bit, and metric[N, out_dim, out_dim] with
 *   metric[f, k, l] = sum_a atom_w[a] * (d out[f, k] / d x[f, a]) . (d out[f, l] / d x[f, a])
 * (out_dim = feature_dim for a plan without an MLP), everything in double: the Jacobian contracted with itself over the atoms in
 * the wave that computes it, never stored.  atom_w: n_inp doubles on the device (inverse masses, diffusion coefficients; any sign),
 * or NULL for all ones - the same bits as an array of ones.  W, b as molann_value_and_jacobian_f64 takes them.  Parameters are
 * data.  On a plan without an MLP the metric G of the features holds no parameter, and for any head behind it
 * sum_a w_a |grad_a y_k|^2 = dF_k G dF_k^T with dF = d y / d features.  The terms are summed in a fixed order and metric[f, k, l] and
 * metric[f, l, k] are stored from one value: no atomics, the same bits on every run, symmetric bit for bit.  MOLANN_E_STAGE for a
 * plan without items, MOLANN_E_UNSUPPORTED where molann_value_and_jacobian_f64 refuses the plan or out_dim > 64.  n_frames < 0:
 * MOLANN_E_DESC; n_frames == 0: nothing is read or launched.  All pointers 8-byte aligned, contiguous.  The call only enqueues on
 * `stream` (no workspace, no event): thread-safe and capturable. */
int molann_value_and_metric_f64(molann_plan* plan, const double* x, int64_t n_frames, const double* const* W, const double* const* b,
                                const double* atom_w, double* out, double* metric, molann_stream_t stream);

/* 1 when molann_value_and_metric_f64 serves the plan (molann_value_and_jacobian_f64 serves it and out_dim <= 64), 0 otherwise. */
int molann_plan_supports_value_and_metric_f64(const molann_plan* plan);

/* Values, the energy of a harmonic restraint on them AND its gradient in ONE launch of frames_value_restraint_f64_kernel (ahead of
 * time: no hipRTC): out[N, out_dim] = molann_value_and_vjp_f64's out, bit for bit (out_dim = feature_dim for a plan without an MLP),
 *   energy[f] = 1/2 sum_k kappa[k] d_k^2,   d_k = out[f, k] - center[f * center_stride + k],
 * and grad_x[N, n_inp, 3] = d energy / d x = J^T (kappa d) - the gradient, as molann_value_and_vjp_f64's grad_x: forces are its
 * negative - everything in double.  Where period[k] > 0 output k is periodic and d_k is wrapped to d_k - period[k] rint(d_k /
 * period[k]) (ties to even); period[k] <= 0: not periodic, so one row serves angles next to distances.  Where flat[k] > 0 the well
 * has a flat bottom of that half-width: d_k = 0 for |d_k| <= flat[k], copysign(|d_k| - flat[k], d_k) beyond it.  A NaN stays a NaN
 * (in its frame's out, energy and grad_x only).  center: out_dim doubles for all frames (center_stride 0) or a row per frame
 * (center_stride = out_dim); any other stride: MOLANN_E_DESC.  kappa: out_dim doubles, any sign.  period, flat: out_dim doubles
 * each, or NULL for none.  All on the device.  The cotangent kappa d is formed in the lanes that computed out - what
 * molann_value_and_vjp_f64 cannot do, because its cotangent must exist before the launch; with period and flat NULL grad_x has the
 * bits of molann_value_and_vjp_f64 for grad_out = kappa * (out - center).  W, b as molann_value_and_vjp_f64 takes them.  Parameters,
 * centres and stiffnesses are data.  energy[f] is one sum in a fixed order, every row of grad_x is stored once (zeros for atoms the
 * plan does not touch): no atomics, the same bits on every run.  Every plan molann_value_and_vjp_f64 serves, unless one frame's rows
 * (that call's + out_dim, in doubles) exceed the LDS of a compute unit: MOLANN_E_UNSUPPORTED; MOLANN_E_STAGE for a plan without
 * items.  n_frames < 0: MOLANN_E_DESC; n_frames == 0: nothing is read or launched.  All pointers 8-byte aligned, contiguous.  The
 * call only enqueues on `stream` (no workspace, no event): thread-safe and capturable. */
int molann_value_and_restraint_f64(molann_plan* plan, const double* x, int64_t n_frames, const double* const* W, const double* const* b,
                                   const double* center, int64_t center_stride, const double* kappa, const double* period,
                                   const double* flat, double* out, double* energy, double* grad_x, molann_stream_t stream);

/* 1 when molann_value_and_restraint_f64 serves the plan (feature items, and a frame's rows fit the LDS), 0 otherwise. */
int molann_plan_supports_value_and_restraint_f64(const molann_plan* plan);

/* Values, a metadynamics bias on them - a sum of Gaussian hills - AND its gradient in ONE launch of frames_value_hills_f64_kernel
 * (ahead of time: no hipRTC): out[N, out_dim] = molann_value_and_vjp_f64's out, bit for bit (out_dim = feature_dim for a plan
 * without an MLP),
 *   bias[f] = sum_h heights[h] exp(-1/2 sum_k (d_hk / sigma_hk)^2),   d_hk = out[f, k] - centers[h * out_dim + k],
 * and grad_x[N, n_inp, 3] = d bias / d x = J^T (d bias / d out) - the gradient, as molann_value_and_vjp_f64's grad_x: forces are its
 * negative - everything in double.  Where period[k] > 0 output k is periodic and d_hk is wrapped to d - period[k] rint(d /
 * period[k]) (ties to even, molann_value_and_restraint_f64's rule); period[k] <= 0: not periodic.  centers: n_hills rows of out_dim
 * doubles; heights: n_hills doubles of any sign; sigma_hk = sigma[h * sigma_stride + k] > 0 (not checked here): one row of out_dim
 * widths for every hill (sigma_stride 0) or a row per hill (sigma_stride = out_dim, adaptive widths); any other stride:
 * MOLANN_E_DESC.  period: out_dim doubles, or NULL for none.  All on the device; the caller appends hills to its own table between
 * steps and passes the count - the table is read at launch, nothing is cached.  n_hills == 0 (the first step of a run) stores out,
 * bias = 0 and grad_x = 0, and centers, heights and sigma may then be NULL; n_hills < 0: MOLANN_E_DESC.  No cutoff: a far hill's exp
 * underflows to 0.  A NaN in a frame's out makes that frame's bias and grad_x NaN and no other's.  A frame's hills are summed in a
 * fixed order, every row of grad_x is stored once (zeros for atoms the plan does not touch): no atomics, the same bits on every run,
 * whatever n_frames.  W, b as molann_value_and_vjp_f64 takes them; parameters and hills are data.  Every plan
 * molann_value_and_restraint_f64 serves with out_dim <= 8 (the cotangent sums of a lane live in registers): MOLANN_E_UNSUPPORTED
 * otherwise; MOLANN_E_STAGE for a plan without items.  n_frames < 0: MOLANN_E_DESC; n_frames == 0: nothing is read or launched.  All
 * pointers 8-byte aligned, contiguous.  The call only enqueues on `stream` (no workspace, no event): thread-safe and capturable. */
int molann_value_and_hills_f64(molann_plan* plan, const double* x, int64_t n_frames, const double* const* W, const double* const* b,
                               const double* centers, const double* heights, int64_t n_hills, const double* sigma, int64_t sigma_stride,
                               const double* period, double* out, double* bias, double* grad_x, molann_stream_t stream);

/* 1 when molann_value_and_hills_f64 serves the plan (molann_value_and_restraint_f64 serves it and out_dim <= 8), 0 otherwise. */
int molann_plan_supports_value_and_hills_f64(const molann_plan* plan);

/* Values, an OPES bias on them - the logarithm of a KERNEL DENSITY (on-the-fly probability enhanced sampling, PLUMED's OPES_METAD) - AND
 * its gradient in ONE launch of frames_value_opes_f64_kernel (ahead of time: no hipRTC): out[N, out_dim] = molann_value_and_vjp_f64's
 * out, bit for bit,
 *   P(y)    = sum_h heights[h] K_h(y),   K_h = exp(-q_h / 2) - exp(-cutoff^2 / 2) where q_h < cutoff^2, else 0,
 *   q_h     = sum_k (d_hk / sigma_hk)^2,   d_hk = out[f, k] - centers[h * out_dim + k],
 *   bias[f] = scale log(P(out[f]) / norm + epsilon),
 * and grad_x[N, n_inp, 3] = d bias / d x = J^T (d bias / d out) - the gradient: forces are its negative - everything in double.
 * centers, heights, n_kernels, sigma, sigma_stride and period as molann_value_and_hills_f64 takes them (the wrap of a periodic output,
 * one row of widths or one per kernel, the table required only where n_kernels > 0, read at launch, nothing cached).  scale (the
 * caller's kT (1 - 1 / biasfactor)), norm (its normalisation Z times the sum of the weights), epsilon and cutoff are host values and
 * travel in the launch's arguments: changing them at every deposit costs nothing.  cutoff = +inf: no cutoff.  A kernel is dropped when
 * q_h >= cutoff^2 is true, so the derivative JUMPS there, as it does in every OPES code.  n_kernels == 0 (the first step of a run):
 * bias = scale log(epsilon), grad_x = 0.  The same for a frame outside every kernel's cutoff.  Negative heights are not checked; a
 * frame with P / norm + epsilon <= 0 gets what log and the division give (NaN or +-inf) and no other frame does.  A NaN in a
 * frame's out makes that frame's bias and grad_x NaN and no other's, at a finite cutoff too.  Every sum has a fixed order, every row
 * of grad_x is stored once: no atomics, the same bits on every run, whatever n_frames.  Plans, argument checks, their order and their
 * codes are molann_value_and_hills_f64's (out_dim <= 8: MOLANN_E_UNSUPPORTED beyond); after them a scale that is not finite, a norm or
 * an epsilon that is not finite and > 0, a cutoff that is NaN or not > 0: MOLANN_E_DESC.  The call only enqueues on `stream` (no
 * workspace, no event): thread-safe and capturable.  Depositing, merging and compressing kernels and the sum the normalisation is
 * formed from: molann_opes_deposit_f64, between steps, on the same table.  Out of scope: float32; neighbour lists; gradients with
 * respect to the table or the parameters.  An OPES term on some of a wider model's outputs, or together with walls or a table:
 * molann_value_and_bias_opes_f64. */
int molann_value_and_opes_f64(molann_plan* plan, const double* x, int64_t n_frames, const double* const* W, const double* const* b,
                              const double* centers, const double* heights, int64_t n_kernels, const double* sigma, int64_t sigma_stride,
                              const double* period, double scale, double norm, double epsilon, double cutoff, double* out, double* bias,
                              double* grad_x, molann_stream_t stream);

/* 1 when molann_value_and_opes_f64 serves the plan (molann_value_and_hills_f64 serves it), 0 otherwise. */
int molann_plan_supports_value_and_opes_f64(const molann_plan* plan);

/* Values, a bias interpolated from a TABLE over them AND its gradient in ONE launch of frames_value_grid_f64_kernel (ahead of time: no
 * hipRTC): out[N, out_dim] = molann_value_and_vjp_f64's out, bit for bit (out_dim = feature_dim for a plan without an MLP),
 * bias[N] = V(out) and grad_x[N, n_inp, 3] = d bias / d x = J^T (d bias / d out) - the gradient: forces are its negative - everything
 * in double, 1 <= out_dim <= 3.  The table holds a bias on a regular grid over the outputs - accumulated metadynamics hills, a
 * free-energy surface, an ABF or OPES estimate, walls - so a call's cost does not depend on what the table was made from.  table: a
 * DEVICE pointer to prod_k shape[k] doubles, row-major with output 0 the slowest axis (offset (i_0 n_1 + i_1) n_2 + i_2); shape, lower,
 * spacing, periodic: HOST arrays of out_dim entries, read during the call (periodic may be NULL: no axis is periodic).  Grid point i of
 * axis k sits at lower[k] + i spacing[k]; a periodic axis has period shape[k] spacing[k], any other spans [lower, lower + (n - 1) h].
 * V is the cubic-convolution (Catmull-Rom) interpolant: per axis u = (out_k - lower_k) / h_k, wrapped into [0, n_k) where periodic,
 * else clamped to [0, n_k - 1]; a cell i, t = u - i, four neighbours i - 1 .. i + 2 (wrapped, or the edge's value repeated) with
 * weights w_0 = ((-t + 2) t - 1) t / 2, w_1 = ((3 t - 5) t^2 + 2) / 2, w_2 = ((-3 t + 4) t + 1) t / 2, w_3 = (t - 1) t^2 / 2;
 * V = sum over the 4^out_dim stencil points of table[...] prod_k w_jk(t_k), and d bias / d out_k the exact derivative of that sum: V is
 * C1 inside the range and across a periodic seam and takes the table's value at a grid point.  Outside a non-periodic range the bias is
 * the edge's value and that axis' derivative exactly 0, so the derivative JUMPS at the range's ends: keep walls inside the range.
 * Every table index is in range for every bit pattern of out; a frame whose out is not finite gets a NaN bias and grad_x and no other
 * frame does.  A frame's stencil is summed in a fixed order and every row of grad_x is stored once: no atomics, the same bits on every
 * run, whatever n_frames.  W, b as molann_value_and_vjp_f64 takes them; parameters and the table are data.  Every plan
 * molann_value_and_restraint_f64 serves with out_dim <= 3: MOLANN_E_UNSUPPORTED otherwise; MOLANN_E_STAGE for a plan without items.
 * After these checks: a NULL shape, lower or spacing: MOLANN_E_NULL; shape[k] < 4, a spacing that is not finite and > 0, a lower that
 * is not finite, or 2^31 table points or more: MOLANN_E_DESC.  n_frames < 0: MOLANN_E_DESC; n_frames == 0: nothing is read or
 * launched.  x, table, out, bias, grad_x 8-byte aligned, contiguous.  The call only enqueues on `stream` (no workspace, no event):
 * thread-safe and capturable. */
int molann_value_and_grid_f64(molann_plan* plan, const double* x, int64_t n_frames, const double* const* W, const double* const* b,
                              const double* table, const int64_t* shape, const double* lower, const double* spacing, const int32_t* periodic,
                              double* out, double* bias, double* grad_x, molann_stream_t stream);

/* 1 when molann_value_and_grid_f64 serves the plan (molann_value_and_restraint_f64 serves it and out_dim <= 3), 0 otherwise. */
int molann_plan_supports_value_and_grid_f64(const molann_plan* plan);

/* Values, UP TO THREE BIAS TERMS ON CHOSEN OUTPUTS and the gradient of their sum in ONE launch of frames_value_bias_f64_kernel (ahead of
 * time: no hipRTC): what a production step of enhanced sampling carries - a tabulated metadynamics bias plus walls, hills on top - at
 * the cost of one pass over the frame.  out[N, out_dim] = molann_value_and_vjp_f64's out, bit for bit; energies[N, 3] = (E_r, V_h, V_g),
 * kept apart because well-tempered heights and reweighting need V_h / V_g without the walls, an absent term's column exactly 0.0;
 * grad_x[N, n_inp, 3] = d(E_r + V_h + V_g) / dx - the gradient: forces are its negative.  Everything in double.
 *   E_r: molann_value_and_restraint_f64's energy on ALL out_dim outputs (kappa_k = 0 leaves output k free); absent when kappa == NULL.
 *        center (center_stride 0 or out_dim), kappa, restraint_period, flat: DEVICE pointers as that call takes them.
 *   V_h: molann_value_and_hills_f64's bias on the n_hills_columns <= 8 outputs hills_columns[0..n) - a HOST array of distinct indices in
 *        any order, NULL for 0..n-1; absent when n_hills_columns == 0.  centers[n_hills, n], heights[n_hills], sigma ([n], sigma_stride 0,
 *        or [n_hills, n], sigma_stride n), hills_period [n] or NULL: DEVICE pointers, laid out over the chosen columns in the order of
 *        the list.  n_hills may be 0: centers, heights and sigma are not read then.
 *   V_g: molann_value_and_grid_f64's interpolant on the n_grid_columns <= 3 outputs grid_columns[0..n) (HOST, NULL for 0..n-1), axis 0
 *        of the table being the first listed output; absent when n_grid_columns == 0.  table: a DEVICE pointer; shape, lower, spacing,
 *        periodic (may be NULL): HOST arrays of n entries, read during the call.
 * The two lists may overlap each other and the restrained outputs.  An absent term's pointers are not looked at.  The cotangent of an
 * output is the restraint's kappa d (0 without one), then the hills' derivative is added, then the table's: a fixed order, and with it,
 * the fixed order of every sum and one store per row of grad_x, the same bits on every run, whatever n_frames.  With one term alone
 * (identity lists) the term's energy and grad_x are the single call's, bit for bit.  Every table index is in range for every bit
 * pattern of out; a frame that is not finite gets NaN and no other frame does.
 * Every plan molann_value_and_restraint_f64 serves whose rows and one more of 11 doubles fit the LDS, whatever out_dim.  Refusals, in
 * this order, nothing being written: a NULL plan, terms, x, out, energies, grad_x or pointer a present term requires (shape, lower and
 * spacing of a present table among them): MOLANN_E_NULL; a pointer that is not 8-byte aligned: MOLANN_E_ALIGNMENT; MOLANN_E_STAGE /
 * MOLANN_E_UNSUPPORTED as molann_value_and_restraint_f64; no term present, a negative count, a stride other than 0 or the term's
 * width, a grid molann_value_and_grid_f64 refuses: MOLANN_E_DESC; a column outside [0, out_dim) or repeated within its list:
 * MOLANN_E_INDEX; more than 8 hills columns or 3 grid columns: MOLANN_E_UNSUPPORTED; a NULL list longer than out_dim: MOLANN_E_INDEX.
 * n_frames < 0: MOLANN_E_DESC; n_frames == 0: nothing is read or launched.  The call only enqueues on `stream` (no workspace, no
 * atomics, no event): thread-safe and capturable. */
typedef struct molann_bias_terms_f64 {
    /* restraint on all outputs; absent when kappa == NULL */
    const double* center; int64_t center_stride; const double *kappa, *restraint_period, *flat;
    /* hills on n_hills_columns <= 8 outputs; absent when n_hills_columns == 0 */
    int32_t n_hills_columns; const int32_t* hills_columns;
    const double *centers, *heights; int64_t n_hills; const double* sigma; int64_t sigma_stride; const double* hills_period;
    /* table on n_grid_columns <= 3 outputs; absent when n_grid_columns == 0 */
    int32_t n_grid_columns; const int32_t* grid_columns;
    const double* table; const int64_t* shape; const double *lower, *spacing; const int32_t* periodic;
} molann_bias_terms_f64;
int molann_value_and_bias_f64(molann_plan* plan, const double* x, int64_t n_frames, const double* const* W, const double* const* b,
                              const molann_bias_terms_f64* terms, double* out, double* energies, double* grad_x, molann_stream_t stream);

/* 1 when molann_value_and_bias_f64 serves the plan (its rows fit the LDS of a compute unit; no cap on out_dim), 0 otherwise. */
int molann_plan_supports_value_and_bias_f64(const molann_plan* plan);

/* Values, an OPES BIAS ON CHOSEN OUTPUTS TOGETHER WITH WALLS AND A TABLE, and the gradient of their sum in ONE launch of
 * frames_value_bias_opes_f64_kernel (ahead of time: no hipRTC): molann_value_and_bias_f64 with the kernel density of
 * molann_value_and_opes_f64 in the place of the hills - what an OPES run with walls carries at every step, on a model of any out_dim.
 * out[N, out_dim] = molann_value_and_vjp_f64's out, bit for bit; energies[N, 4] = (E_r, V_h, V_g, V_o): columns 0..2 mean what they mean
 * in molann_value_and_bias_f64's energies, V_h is always exactly 0.0 (hills are no term of this call), an absent term's column exactly
 * 0.0; grad_x[N, n_inp, 3] = d(E_r + V_o + V_g) / dx - the gradient: forces are its negative.  Everything in double.
 *   E_r, V_g: the restraint and the table of `terms`, as molann_value_and_bias_f64 takes them (a flat-bottom restraint is a pair of
 *        walls).  terms may be NULL: neither.  terms->n_hills_columns != 0: MOLANN_E_UNSUPPORTED - move the hills onto a table, or make
 *        two calls.
 *   V_o: molann_value_and_opes_f64's bias scale log(P / norm + epsilon) on the n_columns <= 8 outputs columns[0..n) - a HOST array of
 *        distinct indices in any order, NULL for 0..n-1.  centers[n_kernels, n], heights[n_kernels], sigma ([n], sigma_stride 0, or
 *        [n_kernels, n], sigma_stride n), period [n] or NULL: DEVICE pointers, laid out over the chosen columns in the order of the
 *        list.  n_kernels may be 0: centers, heights and sigma are not read then, V_o = scale log(epsilon) and its share of grad_x is
 *        exactly 0.  scale, norm, epsilon, cutoff (+inf: none) are host values and travel in the launch's arguments; a kernel is dropped
 *        when q_h >= cutoff^2 is true.  `opes` is required.
 * The lists may overlap each other and the restrained outputs.  An absent term's pointers are not looked at.  The cotangent of an output
 * is the restraint's kappa d (0 without one), then the OPES derivative is added, then the table's: a fixed order, and with it, the fixed
 * order of every sum and one store per row of grad_x, the same bits on every run, whatever n_frames.  With the OPES term alone (identity
 * list) V_o and grad_x are molann_value_and_opes_f64's, bit for bit.  A frame that is not finite gets NaN and no other frame does, at a
 * finite cutoff too.  Plans: molann_value_and_bias_f64's, whatever out_dim (same rows, same launch geometry).  Refusals, in this order,
 * nothing being written: a NULL plan, opes, x, out, energies, grad_x or pointer a present term requires (the kernel table where
 * n_kernels > 0; shape, lower and spacing of a present table): MOLANN_E_NULL; a pointer that is not 8-byte aligned: MOLANN_E_ALIGNMENT;
 * MOLANN_E_STAGE / MOLANN_E_UNSUPPORTED as molann_value_and_bias_f64; n_columns <= 0, a negative count, a stride other than 0 or the
 * term's width, scalars molann_value_and_opes_f64 refuses, a grid molann_value_and_grid_f64 refuses: MOLANN_E_DESC; hills columns in
 * `terms`: MOLANN_E_UNSUPPORTED; a column outside [0, out_dim) or repeated within its list: MOLANN_E_INDEX; more than 8 OPES columns or 3
 * grid columns: MOLANN_E_UNSUPPORTED; a NULL list longer than out_dim: MOLANN_E_INDEX.  n_frames < 0: MOLANN_E_DESC; n_frames == 0:
 * nothing is read or launched.  The call only enqueues on `stream` (no workspace, no atomics, no event): thread-safe and capturable.
 * Out of scope: hills and OPES in one launch; more than one OPES term; float32; depositing or compressing kernels; gradients with
 * respect to tables or parameters. */
typedef struct molann_opes_term_f64 {
    /* the outputs the kernels act on: a HOST list, distinct, any order, <= 8; NULL: 0..n_columns-1 */
    int32_t n_columns; const int32_t* columns;
    /* the kernel table over the listed columns: DEVICE pointers */
    const double *centers, *heights; int64_t n_kernels; const double* sigma; int64_t sigma_stride; const double* period;
    /* host values; cutoff = +inf: none */
    double scale, norm, epsilon, cutoff;
} molann_opes_term_f64;
int molann_value_and_bias_opes_f64(molann_plan* plan, const double* x, int64_t n_frames, const double* const* W, const double* const* b,
                                   const molann_bias_terms_f64* terms, const molann_opes_term_f64* opes, double* out, double* energies,
                                   double* grad_x, molann_stream_t stream);

/* 1 when molann_value_and_bias_opes_f64 serves the plan (molann_value_and_bias_f64 serves it), 0 otherwise. */
int molann_plan_supports_value_and_bias_opes_f64(const molann_plan* plan);

/* The deposit step of an OPES run in ONE launch of opes_deposit_f64_kernel (one block of 256 threads, ahead of time: no hipRTC, no plan):
 * n_new new kernels (new_centers[n_new, d], new_sigma[n_new, d], new_heights[n_new]) are compressed, in order, into a table in
 * caller-owned device memory, in place - centers[capacity, d], sigma[capacity, d] (a row per kernel: sigma_stride = d for
 * molann_value_and_opes_f64) and heights[capacity], 1 <= d <= 8, period[d] or NULL as the OPES entries take it - and
 *   state[0] = n, the live kernels (an exact integer in a double; rows >= n are dead storage, rows >= capacity are never touched),
 *   state[1] = S = sum_{i<n} sum_{j<n} heights_j K_j(centers_i), the sum OPES normalises with (the caller's Z = S / (n kde_norm)),
 *   state[2] = the merges performed so far,     state[3] = the new kernels refused so far
 * are updated.  K_j is molann_value_and_opes_f64's kernel with the cutoff given here.  The launch reads n and S on the device and stores
 * them at its end: the host needs neither to enqueue, so deposits queue back to back and the new kernels may come from torch
 * arithmetic on a bias kernel's outputs with no synchronisation.  Per new kernel a:
 *   1. a value that is not finite, a width or a height that is not > 0: refused += 1 and nothing else changes;
 *   2. where threshold > 0 and n > 0, the live kernel t with the smallest q = sum_k (wrap(c_ak - c_tk) / sigma_tk)^2 (the smallest slot
 *      on a tie) takes a when q < threshold^2: h' = h_t + h_a, delta = wrap(c_a - c_t), c' = c_t + (h_a / h') delta,
 *      sigma'^2 = (h_t sigma_t^2 + h_a sigma_a^2) / h' + (h_t h_a / h'^2) delta^2, merges += 1, the merged kernel stays in slot t;
 *   3. the search is repeated from the merged kernel, its own slot left out: while a kernel t2 lies within the threshold the merged
 *      kernel merges into t2 by the same formulas, the last live kernel moves into the slot it leaves and n -= 1;
 *   4. otherwise a is appended at slot n while n < capacity, and refused += 1 when the table is full.
 * S follows by removing and adding whole kernels (for e against the live set R without it: sum_{i in R} [h_e K_e(c_i) + h_i K_i(c_e)] +
 * h_e (1 - exp(-cutoff^2 / 2))), every sum in a fixed order with no atomics: the same bits on every run, and two queued deposits give
 * the bits of one deposit of the concatenated kernels.  threshold = 0 only appends.  Refusals, in this order, with nothing enqueued: a
 * NULL table, state or new pointer where n_new > 0: MOLANN_E_NULL; a pointer that is not 8-byte aligned: MOLANN_E_ALIGNMENT; d outside
 * 1..8, capacity < 1, n_new < 0, a threshold that is not finite or < 0, a cutoff that is NaN or not > 0 (+inf: none): MOLANN_E_DESC.
 * n_new == 0: MOLANN_OK, nothing launched.  The call only enqueues on `stream` (no workspace, no event): thread-safe on distinct tables
 * and capturable.  neff, the bandwidth rescaling and the heights of a step's kernels, formed on the device from a bias launch's outputs:
 * molann_opes_step_f64; the bias from this state with no read-back: molann_value_and_opes_table_f64.  Out of scope: more than one
 * block; neighbour lists; float32. */
int molann_opes_deposit_f64(double* centers, double* sigma, double* heights, int64_t capacity, int32_t d, const double* period, double* state,
                            const double* new_centers, const double* new_sigma, const double* new_heights, int64_t n_new, double threshold,
                            double cutoff, molann_stream_t stream);

/* The kernel density of an OPES table at arbitrary points in ONE launch of opes_kernel_sum_f64_kernel (no plan): P[m] = sum_h heights[h]
 * K_h(points[m]) for points[n_points, d] and, where dP is not NULL, dP[n_points, d] = dP / dpoints - molann_value_and_opes_f64's P and
 * its walk, before the logarithm.  centers, heights, n_kernels, sigma, sigma_stride (0 or d), period and cutoff as that entry takes
 * them; n_kernels == 0: P = 0, dP = 0, no table pointer read.  The sum over a table's own centres is the S of molann_opes_deposit_f64
 * from scratch.  The same bits on every run.  Refusals: a negative count: MOLANN_E_DESC (n_points == 0: MOLANN_OK); a NULL points, P or
 * table pointer where n_kernels > 0: MOLANN_E_NULL; 8-byte alignment: MOLANN_E_ALIGNMENT; d outside 1..8: MOLANN_E_UNSUPPORTED; a
 * sigma_stride that is neither 0 nor d, a cutoff that is NaN or not > 0: MOLANN_E_DESC. */
int molann_opes_kernel_sum_f64(const double* points, int64_t n_points, int32_t d, const double* centers, const double* heights, int64_t n_kernels,
                               const double* sigma, int64_t sigma_stride, const double* period, double cutoff, double* P, double* dP,
                               molann_stream_t stream);

/* molann_value_and_opes_f64 on a table kept by molann_opes_deposit_f64 / molann_opes_step_f64, in ONE launch of
 * frames_value_opes_table_f64_kernel (ahead of time: no hipRTC): the live count and the normalisation are read from the table's state in
 * device memory, not passed by value, so the host needs neither - no read-back between a deposit and the next bias, and the launch can
 * be captured in a graph and replayed while the table grows.  centers[capacity, out_dim], sigma[capacity, out_dim] (a row per kernel) and
 * heights[capacity] are the table's storage, state[4] = (n, S, merges, refused) its state; every lane forms n = state[0] held to
 * [0, capacity] (a NaN or a negative value: 0) and norm = S / n - OPES' Z kde_norm, with Z = S / (n kde_norm) - and from there on the
 * kernel is molann_value_and_opes_f64's: called with that n, that norm and sigma_stride = out_dim it gives the same bits in out, bias and
 * grad_x.  scale, epsilon and cutoff travel by value as there.  n == 0 (the first step of a run): bias = scale log(epsilon), grad_x
 * exactly 0, nothing of the table is read and norm is not formed.  A state whose S is not finite and > 0 while n >= 1 gives NaN or inf
 * for every frame: it is not guarded - a table whose state the caller broke is the caller's (molann_opes_kernel_sum_f64 over the
 * centres restores S).  Refusals, in molann_value_and_vjp_f64's order and with nothing written: a NULL plan, x, table pointer, state, out,
 * bias or grad_x: MOLANN_E_NULL; 8-byte alignment (period too): MOLANN_E_ALIGNMENT; a plan without items: MOLANN_E_STAGE; the head's
 * tensors; a plan molann_value_and_opes_f64 does not serve: MOLANN_E_UNSUPPORTED; capacity < 1, a scale that is not finite, an epsilon
 * that is not finite and > 0, a cutoff that is NaN or not > 0 (+inf: none): MOLANN_E_DESC.  n_frames == 0: MOLANN_OK.  The same on
 * some of a wider model's outputs, or together with walls or a table: molann_value_and_bias_opes_table_f64.  Out of scope: float32. */
int molann_value_and_opes_table_f64(molann_plan* plan, const double* x, int64_t n_frames, const double* const* W, const double* const* b,
                                    const double* centers, const double* heights, const double* sigma, int64_t capacity, const double* state,
                                    const double* period, double scale, double epsilon, double cutoff, double* out, double* bias, double* grad_x,
                                    molann_stream_t stream);

/* 1 when molann_value_and_opes_table_f64 serves the plan (molann_value_and_opes_f64 serves it), 0 otherwise. */
int molann_plan_supports_value_and_opes_table_f64(const molann_plan* plan);

/* A whole OPES step after the bias launch, in ONE launch of opes_step_f64_kernel (one block of 256 threads, ahead of time: no hipRTC, no
 * plan): from y[n_walkers, d] and V[n_walkers] - the out and bias that molann_value_and_opes_table_f64 (or molann_value_and_opes_f64) just
 * wrote, read only here - it forms this step's kernels and deposits them as molann_opes_deposit_f64 does, on the same table and state,
 * and keeps run[8] = (counter, sum_w, sum_w2, neff, sigma_scale, rct, 0, 0) in device memory.  OPES_METAD's update with a fixed sigma0
 * (not the explore variant):
 *   1. w_a = exp(beta V_a), beta = 1 / kT.  A walker is valid when V_a, w_a and every y[a, k] are finite and w_a > 0; over the valid
 *      walkers counter += 1, sum_w += w_a, sum_w2 += w_a^2 (the step's sums are formed first, in a fixed order, then added);
 *   2. neff = (1 + sum_w)^2 / (1 + sum_w2); rct = log(sum_w / counter) / beta, 0 while counter == 0; sigma_scale = 1 where fixed_sigma
 *      is not 0, else (neff (d + 2) / 4)^(-1 / (d + 4));
 *   3. sigma_k = sigma0_k sigma_scale, raised to sigma_min_k where sigma_min is not NULL, the same for every walker of the step;
 *      height_a = w_a prod_k (sigma0_k / sigma_k);
 *   4. the kernels (y[a], sigma, height_a), a ascending, go through molann_opes_deposit_f64's steps.  An invalid walker's height is NaN,
 *      so it is refused and counted in state[3]; a sigma0 or sigma_min that is not > 0 and finite makes every kernel of the step
 *      invalid (they live in device memory: check them where they are made).
 * The bias kernel's norm needs none of these: it is S / n.  Every sum has a fixed order and there are no atomics: the same bits on
 * every run.  Refusals, in molann_opes_deposit_f64's order, with nothing enqueued: a NULL table, state, run, y, V or sigma0 where
 * n_walkers > 0: MOLANN_E_NULL; a pointer that is not 8-byte aligned (period and sigma_min too): MOLANN_E_ALIGNMENT; d outside 1..8,
 * capacity < 1, n_walkers < 0, a beta that is not finite and > 0, a threshold that is not finite or < 0, a cutoff that is NaN or not > 0:
 * MOLANN_E_DESC.  n_walkers == 0: MOLANN_OK, nothing launched.  The call only enqueues on `stream` (no workspace, no event, nothing
 * allocated): capturable, and a bias launch and this one queue back to back with nothing read back.  Adaptive sigma and the explore
 * variant: molann_opes_step_modes_f64.  Out of scope: walkers on several ranks; more than one block; float32. */
int molann_opes_step_f64(double* centers, double* sigma, double* heights, int64_t capacity, int32_t d, const double* period, double* state,
                         double* run, const double* y, const double* V, int64_t n_walkers, const double* sigma0, const double* sigma_min,
                         double beta, double threshold, double cutoff, int32_t fixed_sigma, molann_stream_t stream);

/* molann_value_and_bias_opes_f64 on a table kept by molann_opes_deposit_f64 / molann_opes_step_f64 / molann_opes_step_columns_f64, in ONE
 * launch of frames_value_bias_opes_table_f64_kernel (ahead of time: no hipRTC): the OPES term's live count and normalisation are read
 * from the table's state in device memory, as molann_value_and_opes_table_f64 reads them, so an OPES run with walls, a table, or a model
 * wider than the kernel table needs no read-back between a deposit and the next bias, and the launch can be captured in a graph and
 * replayed while the table grows.  `terms` (the restraint and the tabulated bias; may be NULL) is molann_value_and_bias_opes_f64's.
 * `opes_table` is required: centers[capacity, n_columns], sigma[capacity, n_columns] (a row per kernel) and heights[capacity] are the
 * table's storage over the listed columns, in the order of the list, state[4] = (n, S, merges, refused) its state - DEVICE pointers, all
 * four required whatever the live count, which only the device knows; period [n_columns] or NULL.  Every lane forms n = state[0] held
 * to [0, capacity] (a NaN or a negative value: 0) and norm = S / n, and from there on the kernel is molann_value_and_bias_opes_f64's:
 * called with that n, that norm and sigma_stride = n_columns it gives the same bits in out, energies[N, 4] = (E_r, 0, V_g, V_o) and
 * grad_x.  n == 0: V_o = scale log(epsilon), its share of grad_x exactly 0, nothing of the kernel table is read and norm is not
 * formed.  A state whose S is not finite and > 0 while n >= 1 gives NaN or inf for every frame: it is not guarded.  Refusals, in
 * molann_value_and_bias_opes_f64's order and with nothing written: a NULL plan, opes_table, x, out, energies, grad_x, kernel table
 * pointer, state, or pointer a present term requires: MOLANN_E_NULL; 8-byte alignment: MOLANN_E_ALIGNMENT; MOLANN_E_STAGE /
 * MOLANN_E_UNSUPPORTED as molann_value_and_bias_f64; n_columns <= 0, a negative grid count, a center_stride other than 0 or out_dim,
 * capacity < 1, scalars molann_value_and_opes_table_f64 refuses, a grid molann_value_and_grid_f64 refuses: MOLANN_E_DESC; hills columns
 * in `terms`: MOLANN_E_UNSUPPORTED; then the lists as molann_value_and_bias_opes_f64 has them.  n_frames < 0: MOLANN_E_DESC;
 * n_frames == 0: nothing is read or launched.  The call only enqueues on `stream` (no workspace, no atomics, no event): thread-safe and
 * capturable.  Out of scope: hills and OPES in one launch; more than one OPES term; float32. */
typedef struct molann_opes_table_term_f64 {
    /* the outputs the kernels act on: a HOST list, distinct, any order, <= 8; NULL: 0..n_columns-1 */
    int32_t n_columns; const int32_t* columns;
    /* the kernel table's storage over the listed columns and its state: DEVICE pointers */
    const double *centers, *heights, *sigma; int64_t capacity; const double* state; const double* period;
    /* host values; cutoff = +inf: none */
    double scale, epsilon, cutoff;
} molann_opes_table_term_f64;
int molann_value_and_bias_opes_table_f64(molann_plan* plan, const double* x, int64_t n_frames, const double* const* W, const double* const* b,
                                         const molann_bias_terms_f64* terms, const molann_opes_table_term_f64* opes_table, double* out,
                                         double* energies, double* grad_x, molann_stream_t stream);

/* 1 when molann_value_and_bias_opes_table_f64 serves the plan (molann_value_and_bias_f64 serves it), 0 otherwise. */
int molann_plan_supports_value_and_bias_opes_table_f64(const molann_plan* plan);

/* molann_opes_step_f64 on strided outputs and chosen columns, in ONE launch of opes_step_columns_f64_kernel: walker a's centre is
 * y[a * y_stride + columns[k]], k < d, and its bias V[a * v_stride] - so the out[n_walkers, out_dim] (y_stride = out_dim) and column 3
 * of the energies[n_walkers, 4] (V = energies + 3, v_stride = 4) that molann_value_and_bias_opes_table_f64 just wrote are read in
 * place.  The weight uses that OPES bias alone, not the walls or the table, as OPES_METAD does.  columns: a HOST list of d distinct
 * indices in [0, y_stride), NULL for 0..d-1, carried by value.  A walker's validity looks at its V and its d chosen outputs only.  On
 * the same walkers the table, state and run are molann_opes_step_f64's on the gathered copy, bit for bit.  Refusals: molann_opes_step_f64's,
 * in its order; then y_stride < d or v_stride < 1: MOLANN_E_DESC; a column outside [0, y_stride) or repeated: MOLANN_E_INDEX - with
 * nothing enqueued.  n_walkers == 0: MOLANN_OK, nothing launched.  Capturable, as molann_opes_step_f64. */
int molann_opes_step_columns_f64(double* centers, double* sigma, double* heights, int64_t capacity, int32_t d, const double* period, double* state,
                                 double* run, const double* y, int64_t y_stride, const int32_t* columns, const double* V, int64_t v_stride,
                                 int64_t n_walkers, const double* sigma0, const double* sigma_min, double beta, double threshold, double cutoff,
                                 int32_t fixed_sigma, molann_stream_t stream);

/* molann_opes_step_columns_f64 in OPES_METAD's other two modes, in ONE launch of opes_step_modes_f64_kernel (one block of 256 threads,
 * ahead of time): widths measured from the run itself (SIGMA=ADAPTIVE) where `adapt` is not NULL, and the explore variant
 * (OPES_METAD_EXPLORE) where bit 1 of `flags` is set.  flags: bit 0 fixed_sigma, bit 1 explore, bit 2 observe only; other bits are
 * ignored.  adapt[n_walkers, 3, d]: a DEVICE array of (mean, M2, sigma0) rows per walker, zeros before the first call, kept by the
 * caller between the calls; run[6] is the number of observations and run[7] is 0 until the first deposit has fixed sigma0, then 1
 * (both stay 0 without adapt).  `sigma0` is read only where adapt is NULL and may be NULL otherwise.  wrap_k(v) = v - P rint(v / P)
 * where period[k] = P > 0.  In order, k ascending, nothing contracted:
 *   1. with adapt: c = run[6] + 1, tau = min(c, adaptive_stride); for every walker whose d chosen outputs are finite and every k:
 *      diff = wrap_k(y_ak - mean_ak), mean_ak += diff / tau, M2_ak += diff wrap_k(y_ak - mean_ak) with the new mean (the mean is not
 *      wrapped back); any other walker keeps its row; run[6] = c.  Each (walker, column) pair is independent of every other: no
 *      reduction, the same bits on every run, and on the host.
 *   2. observe only, or a deposit with run[7] == 0 and c < adaptive_stride (nothing is deposited before the first stride has passed):
 *      the call ends here; the table, state and run[0..5] keep their bits.  With observe only V is not read, but must be a pointer
 *      molann_opes_step_columns_f64 accepts (y will do).
 *   3. the sums and scalars of molann_opes_step_f64; the explore variant takes `counter`, not neff, for sigma_scale (neff and rct are
 *      formed from the weights all the same).
 *   4. without adapt: molann_opes_step_f64's widths.  With adapt, factor = biasfactor (1 in the explore variant): on the first deposit
 *      (run[7] == 0), for every walker and k, M2_ak *= biasfactor - the samples so far were unbiased, the later ones come from the
 *      flattened distribution - and sigma0_ak = sqrt((M2_ak / c) / factor) raised to sigma_min_k, and run[7] = 1; on every deposit
 *      s_ak = sqrt((M2_ak / c) / factor), times sigma_scale unless fixed_sigma, raised to sigma_min_k once, at the end, and
 *      ratio_a = prod_k (sigma0_ak / s_ak).
 *   5. height_a = w_a ratio_a, or ratio_a alone in the explore variant (every kernel weighs 1: S / n does not change with that
 *      scale); NaN for an invalid walker.  A width of 0 - a walker that never moved, no sigma_min - makes its kernel invalid as well.
 *   6. molann_opes_deposit_f64's steps.
 * In the explore variant the caller's bias launch uses scale = kT (biasfactor - 1) and epsilon = exp(-barrier / scale), and a sigma0
 * given without adapt is the target's width, sqrt(biasfactor) times the unbiased one.  Without adapt and without the explore bit the
 * table, state and run are molann_opes_step_columns_f64's, bit for bit.  Refusals, with nothing enqueued: molann_opes_step_columns_f64's,
 * in its order (sigma0 may be NULL with adapt); then adapt not 8-byte aligned: MOLANN_E_ALIGNMENT; observe only without adapt,
 * adaptive_stride < 2 with adapt, a biasfactor that is not finite and > 1 with adapt or in the explore variant: MOLANN_E_DESC.
 * n_walkers == 0: MOLANN_OK, nothing launched.  Capturable, as molann_opes_step_f64.  Out of scope: walkers on several ranks; more than
 * one block; float32; a TorchScript operator. */
int molann_opes_step_modes_f64(double* centers, double* sigma, double* heights, int64_t capacity, int32_t d, const double* period, double* state,
                               double* run, const double* y, int64_t y_stride, const int32_t* columns, const double* V, int64_t v_stride,
                               int64_t n_walkers, const double* sigma0, const double* sigma_min, double* adapt, double beta, double biasfactor,
                               int64_t adaptive_stride, double threshold, double cutoff, int32_t flags, molann_stream_t stream);

/* The deposit step of a METADYNAMICS run on a table, in ONE launch of metad_deposit_f64_kernel (ahead of time: no hipRTC, no plan): the
 * hills of n_walkers walkers are added, in place, to the table molann_value_and_grid_f64 / molann_value_and_bias_f64 interpolate, with
 * well-tempered heights formed on the device from the bias those launches wrote.  table: a DEVICE pointer to prod_k shape[k] doubles,
 * 1 <= d <= 3 axes, layout and axes exactly molann_value_and_grid_f64's (row-major, output 0 slowest; point i of axis k at
 * lower[k] + i spacing[k]; a periodic axis has period shape[k] spacing[k]); shape, lower, spacing, periodic (may be NULL: none),
 * sigma[d] and columns[d] (may be NULL: 0..d-1) are HOST arrays, read during the call.  Walker a's centre is y[a y_stride + columns[k]]
 * and its bias V[a v_stride] (DEVICE, read only), so the column V_g = energies[:, 2] of molann_value_and_bias_f64 and the chosen outputs
 * of a wider model are read where they are.  Per walker a, ascending:
 *   1. h_a = height0 exp(-V_a inv_dT), inv_dT = 1 / (kT (biasfactor - 1)); inv_dT = 0: plain metadynamics, h_a = height0;
 *   2. the walker is valid when V_a, every y[a, columns[k]] and h_a are finite and h_a > 0; any other changes no table entry and is
 *      counted in state[1];
 *   3. every grid point g gets table[g] = table[g] + h_a prod_k exp(-1/2 (delta_k / sigma_k)^2), delta_k = g_k - y_ak, wrapped to
 *      delta - P rint(delta / P) on a periodic axis (bias.add_hills_to_grid's rule); a hill centred outside a non-periodic range lands
 *      on the points it reaches;
 *   4. with a cutoff c (in widths) only where q = sum_k (delta_k / sigma_k)^2 <= c^2: an entry outside keeps its bits, and a tile of
 *      the table (256 entries: 256, 16 x 16, 4 x 4 x 16) that no valid hill reaches is neither read nor written.  +inf: no cutoff.
 * An entry is written by one thread, which adds the walkers' terms in their order, ((t + c_1) + c_2) + ...: no atomics, the same bits
 * on every run and for every launch geometry, and two queued deposits give the bits of one deposit of the concatenated walkers.
 * state[8] (DEVICE) = (hills, refused, sum_heights, steps, logged, 0, 0, 0), exact integers in doubles, updated by one thread in walker
 * order (entries 5..7 are not touched); log (DEVICE, may be NULL) [log_capacity, 2 d + 1] gets one row (centre_k..., sigma_k..., height)
 * per valid walker at row state[4] (held to [0, log_capacity] whatever its bits) while that is below log_capacity - a hill past the
 * capacity is deposited and counted in hills all the same.  The host needs nothing of state to enqueue the next step.  Refusals, in
 * this order, with nothing enqueued: a NULL table, state, y, V, shape, lower, spacing or sigma where n_walkers > 0: MOLANN_E_NULL; a
 * table, state, y, V or log that is not 8-byte aligned: MOLANN_E_ALIGNMENT; d outside 1..3: MOLANN_E_UNSUPPORTED; a grid
 * molann_value_and_grid_f64 refuses (shape[k] < 4, a spacing that is not finite and > 0, a lower that is not finite, 2^31 points or
 * more), a sigma or a height0 that is not finite and > 0, an inv_dT that is not finite and >= 0, a cutoff that is NaN or not > 0, a
 * negative stride, count or capacity, a column outside [0, y_stride): MOLANN_E_DESC.  n_walkers == 0: MOLANN_OK, nothing launched.
 * The call only enqueues on `stream` (no workspace, no event, nothing allocated): thread-safe on distinct tables and capturable.  Out
 * of scope: adaptive widths (molann_metad_widths_f64 and molann_metad_deposit_cov_f64 below); the reweighting offset c(t)
 * (molann_metad_rct_f64 after this call); walkers on several ranks; float32; more than 3 axes. */
int molann_metad_deposit_f64(double* table, int32_t d, const int64_t* shape, const double* lower, const double* spacing, const int32_t* periodic,
                             const double* sigma, const int32_t* columns, const double* y, int64_t y_stride, const double* V, int64_t v_stride,
                             int64_t n_walkers, double height0, double inv_dT, double cutoff, double* state, double* log, int64_t log_capacity,
                             molann_stream_t stream);

/* The reweighting offset c(t) of a METADYNAMICS run from its device-resident table (Tiwary-Parrinello reweighting; PLUMED's CALC_RCT,
 * RCT_USTRIDE, metad.rct): a frame of the run is weighted by exp((V(s, t) - c(t)) / kT).  Two launches, a chain on `stream`
 * (metad_rct_partial_f64_kernel, metad_rct_combine_f64_kernel; ahead of time: no hipRTC, no plan), with no atomics: a deterministic
 * reduction, the same bits on every run and for every launch geometry.  table: a DEVICE pointer to n_entries doubles, read flat and
 * read only - the number of axes does not matter.  With a0 = 1 / kT + inv_dT and aV = inv_dT (inv_dT = 1 / (kT (biasfactor - 1)), what
 * molann_metad_deposit_f64 takes; 0: plain metadynamics):
 *   M = max_g V_g,  S0 = sum_g exp(a0 (V_g - M)),  SV = sum_g exp(aV (V_g - M)),  c = M + kT (log S0 - log SV)
 * = kT log(sum exp(a0 V) / sum exp(aV V)) with no exponent above 0, whatever the table holds.  The table is cut into chunks of 2048
 * consecutive entries; partials (DEVICE) [partial_rows, 4] gets one row (m_c, s0_c, sV_c, bad_c) per chunk - exactly
 * molann_metad_rct_chunks(n_entries) rows are written - and the second launch combines the rows.  The order of every sum is fixed
 * (molann_amd/csrc/molann_metad_rct.h documents it).  rct (DEVICE) [8] = (c, updates, M, a0 M + log S0, aV M + log SV, steps at this update,
 * bad, 0): `updates` is rct[1] + 1 (not finite or negative reads as 0), `bad` the number of entries that are not finite, which enter
 * neither the maximum nor the sums; with bad > 0 slots 0, 2, 3 and 4 are NaN.  state (DEVICE, may be NULL): the state[8] of
 * molann_metad_deposit_f64, of which state[3] = steps is read on the device by both launches (not finite or negative reads as 0): when
 * steps is no multiple of `stride` neither partials nor rct is written, so one captured graph serves a run with any stride; NULL: the
 * update always happens and slot 5 is 0.  Refusals, in this order, with nothing enqueued and nothing written: a NULL table, partials or
 * rct: MOLANN_E_NULL; a table, state, partials or rct that is not 8-byte aligned: MOLANN_E_ALIGNMENT; n_entries < 1 or >= 2^31, a kT that
 * is not finite and > 0, an inv_dT that is not finite and >= 0, stride < 1, partial_rows < molann_metad_rct_chunks(n_entries):
 * MOLANN_E_DESC.  The call only enqueues (no workspace of its own, no event, nothing allocated): capturable.  Out of scope: a running
 * acceleration factor; V - c written per walker; float32; a single-launch reduction. */
int64_t molann_metad_rct_chunks(int64_t n_entries); /* rows of partials needed: ceil(n_entries / 2048); 0 for n_entries < 1 */
int molann_metad_rct_f64(const double* table, int64_t n_entries, double kT, double inv_dT, const double* state, int64_t stride, double* partials,
                         int64_t partial_rows, double* rct, molann_stream_t stream);

/* ADAPTIVE, CORRELATED HILLS of a metadynamics run (the adaptive Gaussians of Branduardi, Bussi and Parrinello; PLUMED's METAD
 * ADAPTIVE=DIFF / GEOM): a hill is a multivariate Gaussian h exp(-1/2 delta^T C^-1 delta) with a full covariance matrix C.  A matrix is
 * stored as its row-major upper triangle, T = d (d + 1) / 2 doubles (c00 c01 c02 c11 c12 c22 for d = 3).  Two calls, ONE launch each
 * (metad_widths_f64_kernel, metad_deposit_cov_f64_kernel; ahead of time: no hipRTC, no plan); molann_amd/csrc/molann_metad_cov.h holds
 * the arithmetic, which the host twins share.
 *
 * molann_metad_widths_f64 keeps the walkers' running statistics and writes the step's covariances.  shape, lower, spacing, periodic
 * (may be NULL), sigma[d], sigma_min[d] (may be NULL: 0), sigma_max[d] (may be NULL: +inf) and columns[d] (may be NULL: 0..d-1) are HOST
 * arrays of the grid molann_metad_deposit_f64 takes, read during the call.  mode 1 (DIFF): walker a's row of adapt (DEVICE)
 * [n_walkers, 1 + d + T] = (n_a, mean, cov) takes one observation of y[a y_stride + columns[k]] (DEVICE, read only) with
 * decay = 1 / window: a y that is not finite leaves the row's bits and is counted in adapt_state[2]; n_a == 0: mean = y, cov = 0,
 * n_a = 1; otherwise delta_k = y_k - mean_k (wrapped to delta - P rint(delta / P) on a periodic axis), mean_k += decay delta_k (then
 * mean_k -= P floor((mean_k - lower_k) / P) on a periodic axis), cov_ij += decay (delta_i delta_j - cov_ij), n_a += 1.  The hill's
 * covariance is cov once n_a >= window and diag(sigma_k^2) before.  mode 2 (GEOM): nothing is observed (adapt and y may be NULL) and
 * C_ij = sigma_i sigma_j metric[a metric_stride + columns[i] metric_ld + columns[j]] (DEVICE, read only: the J J^T of
 * molann_value_and_metric_f64, read in place).  Then the limits, k ascending: target = clamp(C_kk, sigma_min_k^2, sigma_max_k^2); where
 * target != C_kk, row and column k are multiplied by sqrt(target / C_kk) and C_kk = target exactly (C_kk not > 0: the off-diagonal
 * entries of k become 0).  With emit != 0 the result goes to cov_out[a cov_stride + ...] (DEVICE); with emit == 0 the call only
 * observes - the call for the MD steps between two deposits - and cov_out is not touched.  adapt_state[8] (DEVICE) = (observations,
 * emits, skipped, 0...), counts in doubles updated by one thread (entries 3..7 are not touched).  Refusals, in this order, with
 * nothing enqueued: a NULL adapt_state, shape, lower, spacing or sigma, a NULL y or adapt in mode 1, metric in mode 2, cov_out with
 * emit, where n_walkers > 0: MOLANN_E_NULL; an adapt, adapt_state, cov_out, y or metric that is not 8-byte aligned:
 * MOLANN_E_ALIGNMENT; d outside 1..3: MOLANN_E_UNSUPPORTED; another mode, a grid molann_value_and_grid_f64 refuses, a sigma that is not
 * finite and > 0, a sigma_min that is not finite and >= 0, a sigma_max below sigma_min, window < 1 in mode 1, a negative stride or
 * count, cov_stride < T with emit, a column outside [0, y_stride) (mode 1) or [0, metric_ld) (mode 2), a metric_stride that is neither
 * 0 nor at least metric_ld^2: MOLANN_E_DESC.  n_walkers == 0: MOLANN_OK, nothing launched.
 *
 * molann_metad_deposit_cov_f64 is molann_metad_deposit_f64 with walker a's covariance cov[a cov_stride + ...] (DEVICE, read only;
 * cov_stride 0: one matrix for all) in the place of sigma: the same table, grid arrays, y, V, heights, state slots, order of additions
 * (walker order, no atomics, the same bits on every run) and tiles.  C = L L^T with pivots p_k = C_kk - sum_{j<k} L_kj^2; the matrix is
 * usable when every entry is finite and every p_k > 1e-12 C_kk.  A walker is valid when molann_metad_deposit_f64's conditions hold and
 * its matrix is usable; any other changes no entry and is counted in state[1].  Every grid point gets table[g] += h_a exp(-(0.5 q)),
 * q = |L^-1 delta|^2 by forward substitution (no inverse is formed), where q <= cutoff^2.  A tile is skipped for a hill only when a
 * single axis's bound delta_k^2 / C_kk over the tile exceeds cutoff^2 (1 + 1e-12) - q >= delta_k^2 / C_kk by Cauchy-Schwarz; the bounds
 * are not summed - and every entry decides by its own q, so skipping changes no result; a tile no hill reaches is neither read nor
 * written.  log (DEVICE, may be NULL) [log_capacity, d + T + 1] gets one row (centre_k..., C in its triangle, height) per valid walker.
 * Refusals, in this order, with nothing enqueued: a NULL table, state, y, V, cov, shape, lower or spacing where n_walkers > 0:
 * MOLANN_E_NULL; a table, state, y, V, cov or log that is not 8-byte aligned: MOLANN_E_ALIGNMENT; d outside 1..3: MOLANN_E_UNSUPPORTED;
 * what molann_metad_deposit_f64 answers with MOLANN_E_DESC (but for sigma), or a cov_stride that is neither 0 nor at least T:
 * MOLANN_E_DESC.  n_walkers == 0: MOLANN_OK, nothing launched.  Both calls only enqueue on `stream` (no workspace, no event, nothing
 * allocated): capturable.  The deposit never reads adapt: every block of it would race the one writer, so the covariances go through
 * cov_out.  Out of scope: a frame kernel that fuses the bias with the metric; heights renormalised by the determinant; walkers on
 * several ranks; float32; more than 3 axes. */
int molann_metad_widths_f64(int32_t d, const int64_t* shape, const double* lower, const double* spacing, const int32_t* periodic, const double* sigma,
                            const double* sigma_min, const double* sigma_max, const int32_t* columns, const double* y, int64_t y_stride,
                            const double* metric, int64_t metric_stride, int64_t metric_ld, int64_t n_walkers, int32_t mode, int64_t window, int32_t emit,
                            double* adapt, double* adapt_state, double* cov_out, int64_t cov_stride, molann_stream_t stream);
int molann_metad_deposit_cov_f64(double* table, int32_t d, const int64_t* shape, const double* lower, const double* spacing, const int32_t* periodic,
                                 const int32_t* columns, const double* y, int64_t y_stride, const double* V, int64_t v_stride, const double* cov,
                                 int64_t cov_stride, int64_t n_walkers, double height0, double inv_dT, double cutoff, double* state, double* log,
                                 int64_t log_capacity, molann_stream_t stream);

/* PARALLEL-BIAS METADYNAMICS (Pfaendtner and Bonomi, JCTC 2015; PLUMED's PBMETAD) on 1 <= K <= 8 chosen outputs: K one-dimensional
 * tables, one per output, joined by a soft minimum, so that memory and the cost of a step grow linearly in K where a table over K
 * outputs has n^K entries.  Two calls, each ONE launch (ahead of time: no hipRTC); a run alternates them with nothing read back.
 *
 * molann_value_and_pbmetad_f64 (frames_value_pbmetad_f64_kernel): out[N, out_dim] = molann_value_and_vjp_f64's out, bit for bit;
 * energies[N, energies_stride >= 2 + K] = (E_r, V_PB, V_0 .. V_{K-1}); grad_x[N, n_inp, 3] = d(E_r + V_PB) / dx.  With
 * y_k = out[columns[k]] (columns: a HOST array of K distinct indices in any order, NULL for 0..K-1):
 *   V_k  = table k's Catmull-Rom interpolant at y_k, molann_value_and_grid_f64's on one axis: shape[k] >= 4 points at
 *          lower[k] + i spacing[k], periodic with period shape[k] spacing[k] where periodic[k] != 0 (periodic may be NULL: none).  The
 *          K tables lie back to back in ONE buffer `table` (DEVICE) of sum_k shape[k] < 2^31 doubles, table k at sum_{j<k} shape[j];
 *          shape, lower, spacing, periodic: HOST arrays of K entries, read during the call;
 *   m = min_k V_k, e_k = exp(-(V_k - m) / kT), S = ((e_0 + e_1) + ...), w_k = e_k / S, V_PB = m - kT log S, dV_PB/dy_k = w_k V_k'.
 *          K = 1: V_PB = V_0 and the cotangent V_0', bit for bit.  A V_k that is not finite makes that frame's V_PB and grad_x NaN and
 *          changes no other frame;
 *   E_r: molann_value_and_restraint_f64's energy on ALL out_dim outputs; absent when kappa == NULL: exactly 0, its pointers not read.
 * Every sum has a fixed order: the same bits on every run, whatever n_frames.  Plans: molann_value_and_bias_f64's.  Refusals, in this
 * order, nothing being written: a NULL plan, terms, x, out, energies, grad_x, table, shape, lower, spacing or center of a present
 * restraint: MOLANN_E_NULL; a pointer that is not 8-byte aligned: MOLANN_E_ALIGNMENT; MOLANN_E_STAGE / MOLANN_E_UNSUPPORTED as
 * molann_value_and_bias_f64; n_columns < 1: MOLANN_E_DESC, > 8: MOLANN_E_UNSUPPORTED; a column repeated or outside [0, out_dim):
 * MOLANN_E_INDEX; an axis molann_value_and_grid_f64 refuses, a kT that is not finite and > 0, 2^31 entries or more, an energies_stride
 * below 2 + K, a center_stride other than 0 or out_dim: MOLANN_E_DESC.  n_frames < 0: MOLANN_E_DESC; n_frames == 0: nothing is read or
 * launched.  The call only enqueues on `stream` (no workspace, no atomics, no event): thread-safe and capturable.
 *
 * molann_pbmetad_deposit_f64 (pbmetad_deposit_f64_kernel): the hills of n_walkers walkers are added, in place, to the K tables.
 * Walker a's centre on axis k is y[a y_stride + columns[k]] and its bias V[a v_stride + k] (DEVICE, read only; v_stride >= K), so
 * columns 2.. of the energies above are read where they are.  Per walker a, ascending: w_ak as above from (V_a0 .. V_a,K-1);
 * h_ak = height0 exp(-V_ak inv_dT) w_ak (inv_dT = 1 / (kT (biasfactor - 1)); 0: h_ak = height0 w_ak); the walker is valid when every
 * V_ak, centre and h_ak is finite - any other changes no table and is counted in state[1]; then
 * T_k[g] = T_k[g] + h_ak exp(-1/2 (delta / sigma_k)^2) where h_ak > 0 and (delta / sigma_k)^2 <= cutoff^2 (+inf: everywhere), delta
 * and its periodic wrap being molann_metad_deposit_f64's.  An h_ak that underflows to exactly 0 leaves table k's bits; the walker still
 * counts as a hill.  An entry is written by one thread, which adds the walkers' terms in their order: no atomics, the same bits on
 * every run, and two queued deposits give the bits of one deposit of the concatenated walkers; with K = 1 the bits of
 * molann_metad_deposit_f64.  A tile of 256 entries that no hill reaches is neither read nor written.  state[8] (DEVICE) = (hills,
 * refused, sum_heights = sum_a sum_k h_ak, steps, logged, 0, 0, 0); log (DEVICE, may be NULL) [log_capacity, 2 K] gets one row
 * (centre_0.., h_0..) per valid walker, by molann_metad_deposit_f64's overflow rule.  Refusals: molann_metad_deposit_f64's, in its
 * order, per axis (n_axes outside 1..8: MOLANN_E_UNSUPPORTED; 2^31 entries or more in all, a kT that is not finite and > 0, a v_stride
 * below K: MOLANN_E_DESC), then a repeated column: MOLANN_E_INDEX.  n_walkers == 0: MOLANN_OK, nothing launched.  The call only
 * enqueues on `stream`: capturable.  Out of scope: c(t); adaptive widths; per-axis heights or bias factors; partitioned families;
 * walkers on several ranks; float32. */
typedef struct molann_pbmetad_terms_f64 {
    /* restraint on all outputs; absent when kappa == NULL */
    const double* center; int64_t center_stride; const double *kappa, *restraint_period, *flat;
    /* the K tables */
    int32_t n_columns; const int32_t* columns;
    const double* table; const int64_t* shape; const double *lower, *spacing; const int32_t* periodic;
    double kT;
} molann_pbmetad_terms_f64;
int molann_value_and_pbmetad_f64(molann_plan* plan, const double* x, int64_t n_frames, const double* const* W, const double* const* b,
                                 const molann_pbmetad_terms_f64* terms, double* out, double* energies, int64_t energies_stride, double* grad_x,
                                 molann_stream_t stream);
/* 1 when molann_value_and_pbmetad_f64 serves the plan (molann_value_and_bias_f64 serves it), 0 otherwise. */
int molann_plan_supports_value_and_pbmetad_f64(const molann_plan* plan);
int molann_pbmetad_deposit_f64(double* table, int32_t n_axes, const int64_t* shape, const double* lower, const double* spacing,
                               const int32_t* periodic, const double* sigma, const int32_t* columns, const double* y, int64_t y_stride,
                               const double* V, int64_t v_stride, int64_t n_walkers, double height0, double inv_dT, double kT, double cutoff,
                               double* state, double* log, int64_t log_capacity, molann_stream_t stream);

/* molann_forward_packed_f32 that also writes features[N, feature_dim] (what molann_features_f32 would give), for a
 * backward through molann_mlp_backward_f32 + molann_features_backward_f32 without the recompute.  Plans whose MLP
 * is fused into the lane kernel, and large-frame plans with a head within the fused MLP's limits (the features are written
 * where the caller keeps them and the head reads them there) - the ones molann_plan_supports_backward accepts with an MLP;
 * same `out` bit for bit. */
int molann_forward_train_f32(molann_plan* plan, const float* x, int64_t n_frames, float* out, float* features,
                             molann_stream_t stream);

/* dL/dx of molann_features_f32 (PreprocessingANN.forward ann.py:553-565) for the same x:
 * grad_f[N, feature_dim] -> grad_x[N, n_inp, 3].  On a plan with an MLP this is the preprocessing half of its
 * backward. */
int molann_features_backward_f32(molann_plan* plan, const float* x, const float* grad_f, int64_t n_frames,
                                 float* grad_x, molann_stream_t stream);

/* Backward of molann_mlp_packed_f32 (create_sequential_nn's Sequential, ann.py:60-65) for the same f[N, layer_dims[0]]:
 * grad_out[N, out_dim] -> grad_f[N, layer_dims[0]] (written; may be NULL) and grad_params (accumulated; may be NULL;
 * layout of molann_plan_grad_params_size).  fp32 matrix cores; plans for which molann_plan_supports_mlp_backward is 1. */
int molann_mlp_backward_f32(molann_plan* plan, const float* f, const float* grad_out, int64_t n_frames, float* grad_f,
                            float* grad_params, molann_stream_t stream);

/* 1 when molann_mlp_backward_f32 serves the plan's head: every plan with an MLP for which molann_plan_supports_backward is 1,
 * and fp32 heads wider than 32 whose chain weight stream is resident in LDS (tanh, ReLU, sigmoid, identity, SiLU,
 * LeakyReLU; hipRTC present, MOLANN_NO_JIT unset).  The latter leave molann_plan_supports_backward / _backward_kind as
 * they are: the whole-model backward still runs the preprocessing and the head as two nodes.  Builds the kernel it reports. */
int molann_plan_supports_mlp_backward(molann_plan* plan);

/* -- misc ------------------------------------------------------------------------------------- */
int molann_abi_version(void);
/* "release" (the product library: reads no switch that changes or skips part of the computation) or
 * "diagnostics" (libmolann_hip_diag.so, `make diag`: additionally honours MOLANN_DEBUG_*,
 * MOLANN_ELIDE_INVARIANT_ALIGNMENT, MOLANN_JIT_EXTRA_FLAGS for tools/; never used for a reported number). */
const char* molann_build_kind(void);
const char* molann_error_string(int code);
/* Name + launch geometry of the kernels the last launch on this plan used (for bench / profiles).
 * Writes a NUL-terminated string of at most `cap` bytes; returns its length. */
int molann_plan_last_launch_info(const molann_plan* plan, char* buf, int cap);

/* Diagnostic / test hook: the source of the plan-specialised lane kernel for a description (copied to
 * buf, NUL-terminated, at most cap bytes) and, if do_compile != 0, a hipRTC compile of it for gfx950 (no
 * GPU needed).  do_compile bit 0: compile; bit 1: the backward kernel instead of the forward one; bit 9 (512): the one-launch
 * values + vector-Jacobian product of frames the lane kernels do not take (molann_group_vjp), as a plan would specialise it.
 * Returns the source length; on a compile failure a positive hiprtcResult and the log in buf. */
int molann_debug_jit(const molann_plan_desc* desc, int do_compile, char* buf, int cap);

/* Diagnostic (diagnostics build only): per-phase shader-clock sums recorded when MOLANN_DEBUG_ABLATE has bit 32
 * set (see tools/stamps.py); reads and clears 16 counters.  Synchronises the device: never on a product path. */
int molann_debug_read_stamps(unsigned long long* out16);

/* Self-test hooks: the __host__ __device__ math the kernels are built from, compiled for the HOST, so
 * the CPU test-suite can check it against the oracle without a GPU.  Not a product path. */
int molann_selftest_kabsch_rotation(const double* H9, double e0, float* R9);
/* the fp32 instantiation of the same solver (plans whose items are all bond / angle / dihedral) */
int molann_selftest_kabsch_rotation_f32(const float* H9, float e0, float* R9);
int molann_selftest_feature(int type, int use_angle_value, const float* atoms_xyz, float* out3);
float molann_selftest_activation(int act, float v);
int molann_selftest_feature_backward(int type, int use_angle_value, const float* atoms_xyz, const float* g3, float* ga12);
int molann_selftest_kabsch_backward(const double* H9, const float* R9, const float* GR9, float* GH9);
float molann_selftest_act_derivative(int act, float z);
/* the float64 head's derivative of activation `act` at the pre-activation z (all nine codes) */
double molann_selftest_act_derivative_f64(int act, double z);
/* one output's term of molann_value_and_restraint_f64, the function its kernel calls: returns 1/2 kappa d^2 and stores dy = kappa d
 * (d = y - z, wrapped where period > 0, cut where flat > 0); dy may be NULL */
double molann_selftest_restraint_f64(double y, double z, double kappa, double period, double flat, double* dy);
/* one frame's hill sum of molann_value_and_hills_f64 on the host, through the function its kernel calls per hill: returns the bias
 * of y[d] under the table and stores dy[k] = d bias / d y_k (dy may be NULL); hills are added in ascending order.  d outside 1..8, a
 * negative n_hills or a missing pointer: NaN, dy untouched */
double molann_selftest_hills_f64(const double* y, int d, const double* centers, const double* heights, int64_t n_hills, const double* sigma,
                                 int64_t sigma_stride, const double* period, double* dy);
/* one frame's bias of molann_value_and_opes_f64 on the host, through the functions its kernel calls per kernel and per frame: returns
 * scale log(P / norm + epsilon) for y[d] under the table and stores dy[k] = d bias / d y_k (dy may be NULL); kernels are added in
 * ascending order; the four scalars are used as they come.  d outside 1..8, a negative n_kernels or a missing pointer: NaN, dy
 * untouched */
double molann_selftest_opes_f64(const double* y, int d, const double* centers, const double* heights, int64_t n_kernels, const double* sigma,
                                int64_t sigma_stride, const double* period, double scale, double norm, double epsilon, double cutoff,
                                double* dy);
/* molann_opes_deposit_f64 on the host: the same arguments as HOST pointers, the same steps through the functions its kernel calls, the
 * same refusals and the device's order of every sum */
int molann_selftest_opes_deposit_f64(double* centers, double* sigma, double* heights, int64_t capacity, int32_t d, const double* period,
                                     double* state, const double* new_centers, const double* new_sigma, const double* new_heights, int64_t n_new,
                                     double threshold, double cutoff);
/* one frame's bias of molann_value_and_opes_table_f64 on the host: n and norm from state[4] as its kernel forms them (state[0] NaN or
 * below 1: no kernel; above capacity: capacity), then molann_selftest_opes_f64 on the first n rows with a row of widths per kernel.
 * d outside 1..8, capacity < 1 or a missing pointer: NaN, dy untouched */
double molann_selftest_opes_table_f64(const double* y, int d, const double* centers, const double* heights, const double* sigma, int64_t capacity,
                                      const double* state, const double* period, double scale, double epsilon, double cutoff, double* dy);
/* molann_opes_step_f64 on the host: the same arguments as HOST pointers, the same steps through the functions its kernel calls, the
 * same refusals and the device's order of every sum */
int molann_selftest_opes_step_f64(double* centers, double* sigma, double* heights, int64_t capacity, int32_t d, const double* period, double* state,
                                  double* run, const double* y, const double* V, int64_t n_walkers, const double* sigma0, const double* sigma_min,
                                  double beta, double threshold, double cutoff, int32_t fixed_sigma);
/* molann_metad_deposit_f64 on the host: the same arguments as HOST pointers, the same refusals, the same tiles, and per entry the
 * walkers' terms in their order through the functions its kernel calls */
int molann_selftest_metad_deposit_f64(double* table, int32_t d, const int64_t* shape, const double* lower, const double* spacing,
                                      const int32_t* periodic, const double* sigma, const int32_t* columns, const double* y, int64_t y_stride,
                                      const double* V, int64_t v_stride, int64_t n_walkers, double height0, double inv_dT, double cutoff,
                                      double* state, double* log, int64_t log_capacity);
/* molann_metad_rct_f64 on the host: the same arguments as HOST pointers, the same refusals, the same chunks, the same tree and the
 * same functions */
int molann_selftest_metad_rct_f64(const double* table, int64_t n_entries, double kT, double inv_dT, const double* state, int64_t stride,
                                  double* partials, int64_t partial_rows, double* rct);
/* molann_metad_widths_f64 and molann_metad_deposit_cov_f64 on the host: the same arguments as HOST pointers, the same refusals, the
 * same tiles, and per walker and per entry the functions their kernels call */
int molann_selftest_metad_widths_f64(int32_t d, const int64_t* shape, const double* lower, const double* spacing, const int32_t* periodic,
                                     const double* sigma, const double* sigma_min, const double* sigma_max, const int32_t* columns, const double* y,
                                     int64_t y_stride, const double* metric, int64_t metric_stride, int64_t metric_ld, int64_t n_walkers, int32_t mode,
                                     int64_t window, int32_t emit, double* adapt, double* adapt_state, double* cov_out, int64_t cov_stride);
int molann_selftest_metad_deposit_cov_f64(double* table, int32_t d, const int64_t* shape, const double* lower, const double* spacing,
                                          const int32_t* periodic, const int32_t* columns, const double* y, int64_t y_stride, const double* V,
                                          int64_t v_stride, const double* cov, int64_t cov_stride, int64_t n_walkers, double height0, double inv_dT,
                                          double cutoff, double* state, double* log, int64_t log_capacity);
/* one frame of molann_value_and_pbmetad_f64 on the host, through the functions its kernel calls and in one lane's order (every pointer
 * of `terms` a HOST pointer here; center is one row): energies[2 + K] = (E_r, V_PB, V_0 ..), dy[d_out] = the cotangent.  Returns
 * MOLANN_OK, or the code molann_value_and_pbmetad_f64 gives the same terms (nothing written then) */
int molann_selftest_pbmetad_f64(const double* y, int d_out, const molann_pbmetad_terms_f64* terms, double* energies, double* dy);
/* molann_pbmetad_deposit_f64 on the host: the same arguments as HOST pointers, the same refusals, the same tiles, and per entry the
 * walkers' terms in their order through the functions its kernel calls */
int molann_selftest_pbmetad_deposit_f64(double* table, int32_t n_axes, const int64_t* shape, const double* lower, const double* spacing,
                                        const int32_t* periodic, const double* sigma, const int32_t* columns, const double* y, int64_t y_stride,
                                        const double* V, int64_t v_stride, int64_t n_walkers, double height0, double inv_dT, double kT,
                                        double cutoff, double* state, double* log, int64_t log_capacity);
/* one axis' step of molann_value_and_grid_f64 on the host, through the function its kernel calls: the four table indices, the four
 * weights and the four derivative weights (s w' / spacing) for output value y on an axis of n points; any of the three may be NULL */
void molann_selftest_grid_axis_f64(double y, int64_t n, double lower, double spacing, int32_t periodic, int64_t idx[4], double w[4], double dw[4]);
/* one frame's interpolation of molann_value_and_grid_f64 on the host, through the functions its kernel calls (table: a HOST pointer
 * here): returns the bias of y[d] and stores dy[k] = d bias / d y_k (dy may be NULL); stencil points are added in ascending order.  d
 * outside 1..3, a missing pointer (periodic may be NULL) or a grid molann_value_and_grid_f64 answers with MOLANN_E_DESC: NaN, dy
 * untouched */
double molann_selftest_grid_f64(const double* y, int d, const double* table, const int64_t* shape, const double* lower, const double* spacing,
                                const int32_t* periodic, double* dy);
/* one frame of molann_value_and_bias_f64 on the host, through the functions its kernel calls, with its column mapping and its order of
 * additions (every pointer of `terms` a HOST pointer here; center is one row): energies3 = (E_r, V_h, V_g), dy[d_out] = the cotangent.
 * Returns MOLANN_OK, or the code molann_value_and_bias_f64 gives the same terms (nothing written then) */
int molann_selftest_bias_f64(const double* y, int d_out, const molann_bias_terms_f64* terms, double* energies3, double* dy);
/* one frame of molann_value_and_bias_opes_f64 on the host, through the functions its kernel calls, with its column mapping and its order
 * of additions (every pointer of `terms` and `opes` a HOST pointer here; center is one row): energies4 = (E_r, 0, V_g, V_o), dy[d_out] =
 * the cotangent.  Returns MOLANN_OK, or the code molann_value_and_bias_opes_f64 gives the same terms (nothing written then) */
int molann_selftest_bias_opes_f64(const double* y, int d_out, const molann_bias_terms_f64* terms, const molann_opes_term_f64* opes,
                                  double* energies4, double* dy);
/* one frame of molann_value_and_bias_opes_table_f64 on the host (every pointer of `terms` and `opes_table` a HOST pointer here): n and
 * norm from state[4] as its kernel forms them, then molann_selftest_bias_opes_f64's steps on the first n rows with a row of widths per
 * kernel - the same code, so the same doubles.  Returns MOLANN_OK, or the code molann_value_and_bias_opes_table_f64 gives the same terms
 * (nothing written then) */
int molann_selftest_bias_opes_table_f64(const double* y, int d_out, const molann_bias_terms_f64* terms, const molann_opes_table_term_f64* opes_table,
                                        double* energies4, double* dy);
/* molann_opes_step_columns_f64 on the host: the same arguments as HOST pointers, the same steps through the functions its kernel calls,
 * the same refusals and the device's order of every sum */
int molann_selftest_opes_step_columns_f64(double* centers, double* sigma, double* heights, int64_t capacity, int32_t d, const double* period,
                                          double* state, double* run, const double* y, int64_t y_stride, const int32_t* columns, const double* V,
                                          int64_t v_stride, int64_t n_walkers, const double* sigma0, const double* sigma_min, double beta,
                                          double threshold, double cutoff, int32_t fixed_sigma);
/* molann_opes_step_modes_f64 on the host: the same arguments as HOST pointers (adapt too), the same steps through the functions its
 * kernel calls, the same refusals and the device's order of every sum */
int molann_selftest_opes_step_modes_f64(double* centers, double* sigma, double* heights, int64_t capacity, int32_t d, const double* period,
                                        double* state, double* run, const double* y, int64_t y_stride, const int32_t* columns, const double* V,
                                        int64_t v_stride, int64_t n_walkers, const double* sigma0, const double* sigma_min, double* adapt,
                                        double beta, double biasfactor, int64_t adaptive_stride, double threshold, double cutoff, int32_t flags);
/* the unit-cotangent local Jacobian frames_value_jac_f64_kernel combines: jac36[c][j][xyz] = d(output column c of the item) /
 * d(atom j) for the item's 4 atoms (rows past the item's width are 0); returns the width */
int molann_selftest_item_jacobian_f64(int type, int use_angle_value, const double* atoms_xyz, double* jac36);
/* forward mode: the item's values and their derivatives along the atoms' tangents (t12: 4 atoms x xyz); return the width */
int molann_selftest_feature_tangent_f32(int type, int use_angle_value, const float* atoms_xyz, const float* t12, float* out3,
                                        float* dout3);
int molann_selftest_feature_tangent_f64(int type, int use_angle_value, const double* atoms_xyz, const double* t12, double* out3,
                                        double* dout3);
/* the rotation in double, the tangent dR of the rotation for a covariance direction dH, and the backward in double */
int molann_selftest_kabsch_rotation_f64(const double* H9, double e0, double* R9);
int molann_selftest_kabsch_tangent(const double* H9, const double* R9, const double* dH9, double* dR9);
int molann_selftest_kabsch_backward_f64(const double* H9, const double* R9, const double* GR9, double* GH9);
/* second order: the float64 item backward (ga12: 4 atoms x xyz) and its derivative along atom tangents t12 and a cotangent
 * tangent dg3 (return the atom count); the Kabsch backward G_H and its derivative along (dH, dR, dG_R) */
int molann_selftest_feature_backward_tangent_f64(int type, int use_angle_value, const double* atoms_xyz, const double* t12,
                                                 const double* g3, const double* dg3, double* ga12, double* dga12);
int molann_selftest_kabsch_backward_tangent(const double* H9, const double* R9, const double* GR9, const double* dH9, const double* dR9,
                                            const double* dGR9, double* GH9, double* dGH9);

#ifdef __cplusplus
}
#endif
#endif /* MOLANN_HIP_H */
