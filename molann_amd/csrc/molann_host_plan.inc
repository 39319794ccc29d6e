// molann_host_plan.inc - part of libmolann_hip.so, included by molann_kernels.hip (one translation unit: the kernels' host stubs and the
// launches that use them must see each other).  Host: diagnostics switches, struct molann_plan, description validation, launch geometry, kernel arguments.
namespace {

inline int ceil_to(int v, int m) { return (v + m - 1) / m * m; }

// Switches that change WHAT is computed, skip part of it, or exist only for experiments (MOLANN_DEBUG_*,
// MOLANN_ELIDE_INVARIANT_ALIGNMENT, MOLANN_JIT_EXTRA_FLAGS) are read by the diagnostics build alone
// (`make diag` -> libmolann_hip_diag.so, -DMOLANN_DIAGNOSTICS; tools/ loads it with MOLANN_DIAG_LIB=1).  The
// product library never looks at them: molann_build_kind() says which one is loaded.
inline const char* diag_env(const char* name) {
#ifdef MOLANN_DIAGNOSTICS
    return getenv(name);
#else
    (void)name;
    return nullptr;
#endif
}

// switches read once per process (never on the launch path)
struct DebugEnv {
    int ablate, lds_pad, wave_bpc, wave_pre;
    DebugEnv() {
        const char* e;
        ablate = (e = diag_env("MOLANN_DEBUG_ABLATE")) ? atoi(e) : 0;
        lds_pad = (e = diag_env("MOLANN_DEBUG_LDS_PAD")) ? atoi(e) : 0;
        wave_bpc = (e = getenv("MOLANN_WAVE_BPC")) ? atoi(e) : 0;
        wave_pre = (e = getenv("MOLANN_WAVE_PRE")) ? atoi(e) : -1; // item rounds preloaded by frames_wave_kernel
    }
};
const DebugEnv& debug_env() {
    static const DebugEnv env;
    return env;
}

} // namespace

// =============================================================================================
// plan
// =============================================================================================
struct molann_plan {
    int device;
    int num_cus;
    int n_inp, n_align, n_features, n_items, d_feat, use_angle_value;
    int n_layers, act, mlp_prec;
    int dims[MOLANN_MAX_LAYERS + 1];
    int out_dim;
    int family;        // 0 lane-per-frame, 1 wave-per-frame
    bool fused_mlp;    // lane kernel runs the MLP itself
    bool lane_mlp;     // the MLP is within the fused MLP's limits: on its own it runs in mlp_lane_kernel
    bool has_position_items; // the forward mode needs the rotation's tangent (molann_jvp.inc)
    // device memory (one allocation)
    unsigned char* blob;
    int* d_align_idx;
    float* d_ref;      // [3a] + 6 constants
    double* d_ref64;   // the same in fp64 (covariance accumulation)
    ItemDev* d_items;
    float* d_wlane;    // fused layout
    void* d_wmfma;     // mfma layout
    float* d_work;     // two feature chunks [2][work_frames][d_feat] (ping-pong between gather and MLP kernels)
    long work_frames;
    hipStream_t side;  // the MLP kernel of chunk i runs here while the caller's stream gathers chunk i+1
    hipEvent_t ev_feat[2], ev_mlp[2];
    // The workspace, the side stream and these events belong to the plan: forwards of one plan issued from different
    // streams (or threads) are ordered one after the other - the host side by launch_mu, the device side by making a
    // new caller's stream wait for ev_done, recorded behind the previous call's join.
    hipEvent_t ev_done;
    hipStream_t last_stream;
    bool have_done;
    std::mutex* launch_mu;
    std::mutex* jit_mu;        // the lazily built kernels (features twin, backward pair, backward workspace)
    int kp[MOLANN_MAX_LAYERS], jp[MOLANN_MAX_LAYERS];
    long moff[MOLANN_MAX_LAYERS];
    int mlp_ld[2], mlp_lds_per_wave;
    // lane kernel geometry: [0] feature mode (tile + staging columns), [1] align-out mode (tile only)
    struct LaneGeom { int lds_per_wave, fbuf_off, wpb, ok; } geom[2];
    // register-resident mode: <= 16 touched atoms ("slots", align atoms first) and tables in slot indices
    // plan-specialised lane kernel (hipRTC), feature mode; nullptr -> generic kernel
    hipModule_t jit_mod;
    hipFunction_t jit_fn;
    int jit_nl;          // Linear layers fused into it (0: features only)
    LaneGeom jit_geom;   // its own LDS geometry: the compact tile (touched 16-byte windows only) + staging columns
    int jit_waves;       // waves per SIMD it was compiled for
    int jit_ncons, jit_nload, jit_nslot, jit_bpc, jit_lds_block; // loader / consumer block geometry of the specialised forward kernel
    bool jit_only;       // no ahead-of-time kernel serves this plan's fused forward (large frame / 33..64 features)
    char jit_note[96];
    struct JitSpecBox* spec;   // what the specialised kernels are generated from (kept for the lazy backward build)
    hipModule_t bwd_mod;
    hipFunction_t bwd_fn;      // backward of the preprocessing (molann_lane_bwd.inc), compiled at the first backward
    int bwd_state;             // 0 not tried, 1 ready, -1 unavailable
    hipModule_t rbwd_mod;
    hipFunction_t rbwd_fn;     // the whole backward in one pass over x (molann_bwd_ring.inc), compiled at the first backward
    int rbwd_state, rbwd_ncons, rbwd_nload, rbwd_nslot, rbwd_lds;
    hipModule_t vjp_mod;
    hipFunction_t vjp_fn;      // the one-pass backward that also stores the forward's outputs (molann_value_and_vjp_f32), same geometry
    int vjp_state;
    hipModule_t gvjp_mod;
    hipFunction_t gvjp_fn;     // values + vjp in one launch for frames the lane kernels do not take (molann_group_vjp.inc), built at the first use
    int gvjp_state, gvjp_b, gvjp_wpb, gvjp_lds, gvjp_bpc;
    int* d_va_atoms; int* d_va_ptr; int* d_va_list;   // ... its touched atoms and what each gathers (group_vjp_tables)
    int va_touched, va_list_len;
    int* d_hv_ptr; int* d_hv_list;   // second order (molann_hvp.inc): per atom, its item slots (4 it + j) and align slots (-(i + 1))
    hipModule_t mbwd_mod;
    hipFunction_t mbwd_fn;     // backward of the fused family's MLP (molann_mlp_bwd.inc), compiled at the first backward
    int mbwd_state, mbwd_wpb;
    hipModule_t cbwd_mod;
    hipFunction_t cbwd_fn;     // backward of a wide fp32 head (molann_chain_bwd.inc), compiled at the first backward
    int cbwd_state, cbwd_waves; // state: 0 not tried, 1 ready, -1 unavailable; waves: 0 when the plan's head is not one it serves
    // features-only twin of a forward kernel that has the MLP fused in (what molann_features_f32 and the backward's
    // recompute launch on such a plan), compiled at the first use
    struct JitSpecBox* align_spec;  // AlignmentLayer.forward as alignment + one position item per atom through the specialised kernel
    struct JitSpecBox* mlp_spec;    // a small head behind a wave-per-frame kernel: layer sizes and packed layout for molann_mlp_bwd
    hipModule_t align_mod;
    hipFunction_t align_fn;    // ... compiled at the first molann_align_f32
    int align_state;
    hipModule_t wide_mod;
    hipFunction_t wide_fn;     // the whole forward of a plan whose MLP is wider than 32 in ONE lane kernel (WIDE_MLP: the chain MLP's arithmetic on a
                               // weight stream resident in LDS); nullptr -> features kernel + chain MLP kernel
    int wide_ncons, wide_nload, wide_nslot, wide_bpc, wide_lds_block;
    hipModule_t train_mod;
    hipFunction_t train_fn;    // the fused forward kernel that also writes the features (molann_forward_train_f32), same geometry
    int train_state;
    hipModule_t feat_mod;
    hipFunction_t feat_fn;
    int feat_state, feat_ncons, feat_nload, feat_nslot, feat_bpc, feat_lds_block;
    float* d_gpart;            // molann_mlp_bwd's parameter sums, one row per block: [num_cus][n_grad_params]
    hipEvent_t ev_bwork;       // the backward workspaces (d_gpart, d_bwork) are shared by all streams: see launch_mu
    hipStream_t bwork_stream;
    bool have_bwork;
    float* d_bwork;            // molann_backward_f32 on a plan with an MLP: features and their gradient, [2][bwork_frames][d_feat]
    long bwork_frames;
    int n_grad_params;         // floats of the parameter-gradient buffer (dW_l[J][K], db_l[J] per layer)
    // plan-specialised wide bf16 MLP (molann_mlp_jit.inc); nullptr -> mlp_mfma_kernel<bf16>
    hipModule_t chain_mod;
    hipFunction_t chain_fn;
    unsigned char* d_wchain;   // weight fragments in consumption order, then the padded fp32 biases
    long chain_stream_bytes;
    int chain_fb;              // 16-frame blocks per wave
    int chain_waves;           // waves per block: 4 (weights streamed through LDS slabs) or 8 (weight stream resident in LDS)
    int chain_nslab;           // LDS slab buffers of the streamed weights (2 to 4; 1: resident)
    char chain_note[96];
    char mlp_info[96];         // name + geometry of the last MLP kernel launch
    // large frames through frames_ring_kernel: per-frame window list, LDS positions of the alignment atoms and of the
    // items' atoms inside the staged image; ring_nd = LDS-DMA instructions per frame (0: frames_wave_kernel serves the plan)
    int align_first;           // align_idx[0]
    int* d_ring_win;
    int* d_ring_align_pos;
    ItemDev* d_ring_items;
    int ring_nd, ring_nwin;
    // large frames, backward without atomics (frames_wave_bwd_gather_kernel): touched atoms, CSR of their (item, atom) pairs
    int* d_bw_atoms; int* d_bw_ptr; int* d_bw_list; int* d_bw_align;
    int bw_list_len;
    bool dense_positions;   // a feature plan that IS the aligned frame: one position item per atom, in order (AlignmentLayer under autograd)
    int* d_align_slot;      // ... [n_inp]: the atom's place in the alignment set or -1
    int bw_touched;
    int n_slots;
    bool regs_mode;
    int* d_slots;
    ItemDev* d_items_slot;
    bool mlp_packed;
    char last_info[256];
};

namespace {

#define HIP_TRY(expr)                      \
    do {                                   \
        hipError_t _e = (expr);            \
        if (_e != hipSuccess) return (int)_e; \
    } while (0)

// waves never share LDS, so the block size is free: take the one that packs most waves into the CU's
// 160 KiB (blocks <= 64 KiB: the LDS-DMA destination offset is 16 bits), larger block on ties
void lane_geometry(molann_plan::LaneGeom& g, int tile_bytes, int cols_needed) {
    const int tile_pad = ceil_to(tile_bytes, 16);
    const int fbuf_bytes = ceil_to(cols_needed * FB_STRIDE * 4, 16);
    g.fbuf_off = tile_pad;
    g.lds_per_wave = tile_pad + fbuf_bytes;
    const long L = g.lds_per_wave;
    int best = 0, best_waves = 0;
    for (int wpb = 4; wpb >= 1; --wpb) {
        if (wpb * L > 65536) continue;
        long waves = wpb * (163840 / (wpb * L));
        if (waves > 32) waves = 32;
        if (waves > best_waves) { best_waves = (int)waves; best = wpb; }
    }
    g.wpb = best;
    g.ok = (best >= 1 && best_waves >= 4) ? 1 : 0; // fewer than 4 waves per CU: use the wave-per-frame kernel
}

int validate_desc(const molann_plan_desc* d) {
    if (!d) return MOLANN_E_NULL;
    if (d->abi_version != MOLANN_ABI_VERSION) return MOLANN_E_DESC;
    if (d->n_inp <= 0 || d->n_align < 0 || d->n_features < 0 || d->n_layers < 0) return MOLANN_E_DESC;
    if (d->n_layers > MOLANN_MAX_LAYERS) return MOLANN_E_UNSUPPORTED;
    if (d->n_align == 0 && d->n_features == 0 && d->n_layers == 0) return MOLANN_E_DESC;
    if (d->n_align > 0) {
        if (!d->align_idx || !d->ref_x) return MOLANN_E_NULL;
        for (int i = 0; i < d->n_align; ++i)
            if (d->align_idx[i] < 0 || d->align_idx[i] >= d->n_inp) return MOLANN_E_INDEX;
    }
    if (d->n_features > 0) {
        if (!d->feat_type || !d->feat_ptr || !d->feat_idx) return MOLANN_E_NULL;
        if (d->feat_ptr[0] != 0) return MOLANN_E_DESC;
        for (int f = 0; f < d->n_features; ++f) {
            const int cnt = d->feat_ptr[f + 1] - d->feat_ptr[f];
            const int t = d->feat_type[f];
            if (cnt < 0) return MOLANN_E_DESC;
            if (t == MOLANN_FEAT_ANGLE) { if (cnt != 3) return MOLANN_E_FEATURE; }   // feature.py:88
            else if (t == MOLANN_FEAT_BOND) { if (cnt != 2) return MOLANN_E_FEATURE; }   // feature.py:91
            else if (t == MOLANN_FEAT_DIHEDRAL) { if (cnt != 4) return MOLANN_E_FEATURE; } // feature.py:94
            else if (t == MOLANN_FEAT_POSITION) { if (cnt < 1) return MOLANN_E_FEATURE; }
            else return MOLANN_E_FEATURE;                                                  // feature.py:82
            for (int i = d->feat_ptr[f]; i < d->feat_ptr[f + 1]; ++i)
                if (d->feat_idx[i] < 0 || d->feat_idx[i] >= d->n_inp) return MOLANN_E_INDEX;
        }
    }
    if (d->n_layers > 0) {
        if (!d->layer_dims) return MOLANN_E_NULL;
        for (int i = 0; i <= d->n_layers; ++i)
            if (d->layer_dims[i] <= 0) return MOLANN_E_DESC;
        if (d->activation < 0 || d->activation > MOLANN_ACT_GELU) return MOLANN_E_UNSUPPORTED;
        if (d->mlp_precision != MOLANN_MLP_F32 && d->mlp_precision != MOLANN_MLP_BF16) return MOLANN_E_UNSUPPORTED;
    }
    return MOLANN_OK;
}

int grid_for(const molann_plan* p, long work_items, int items_per_block, int blocks_per_cu) {
    long need = (work_items + items_per_block - 1) / items_per_block;
    long cap = (long)p->num_cus * blocks_per_cu;
    long g = need < cap ? need : cap;
    return (int)(g < 1 ? 1 : g);
}

void fill_pre_args(const molann_plan* p, PreArgs& a, long n_frames, int mode, int out_cols, bool with_mlp,
                   const void* x, const void* out) {
    memset(&a, 0, sizeof(a));
    a.n_frames = n_frames;
    a.n_inp = p->n_inp;
    a.frame_dw = 3 * p->n_inp;
    a.mode = mode;
    a.n_align = p->n_align;
    a.n_items = p->n_items;
    a.out_cols = out_cols > 0 ? out_cols : 1;
    a.step_f = 64 / a.out_cols;
    a.step_c = 64 % a.out_cols;
    const molann_plan::LaneGeom& g = p->geom[mode == 1 ? 1 : 0];
    a.lds_per_wave = g.lds_per_wave;
    a.fbuf_off = g.fbuf_off;
    a.n_slots = p->n_slots;
    a.x_wide = (((uintptr_t)x) & 15) == 0;
    a.out_wide = (((uintptr_t)out) & 15) == 0;
    a.n_layers = with_mlp ? p->n_layers : 0;
    a.act = p->act;
    for (int i = 0; i <= p->n_layers; ++i) a.dims[i] = p->dims[i];
    a.out_vec4 = (a.out_wide && (a.out_cols & 3) == 0) ? 1 : 0;
    a.ablate = debug_env().ablate;
}


// per atom of the frame (hv_ptr: n_inp + 1 offsets into hv_list): the slots 4 it + j of the items that name it (item order), then
// -(i + 1) for each place i it holds in the alignment set (an atom named twice there has two rows) - frames_hvp_kernel's gather
inline void hvp_tables(int n_inp, const std::vector<ItemDev>& items, const int* align_idx, int n_align, std::vector<int>& ptr,
                       std::vector<int>& list) {
    std::vector<std::vector<int>> per(n_inp);
    for (size_t it = 0; it < items.size(); ++it)
        for (int j = 0; j < item_atoms(items[it].type); ++j) per[items[it].idx[j]].push_back((int)(4 * it + j));
    for (int i = 0; i < n_align; ++i) per[align_idx[i]].push_back(-(i + 1));
    ptr.assign(1, 0);
    list.clear();
    for (int k = 0; k < n_inp; ++k) {
        list.insert(list.end(), per[k].begin(), per[k].end());
        ptr.push_back((int)list.size());
    }
}

} // namespace
