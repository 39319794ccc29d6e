// molann_capi.inc - part of libmolann_hip.so, included by molann_kernels.hip (one translation unit: the kernels' host stubs and the
// launches that use them must see each other).  The C ABI (include/molann_hip.h).
// =============================================================================================
// C ABI
// =============================================================================================
extern "C" {

int molann_abi_version(void) { return MOLANN_ABI_VERSION; }

const char* molann_build_kind(void) {
#ifdef MOLANN_DIAGNOSTICS
    return "diagnostics";
#else
    return "release";
#endif
}

const char* molann_error_string(int code) {
    switch (code) {
    case MOLANN_OK: return "ok";
    case MOLANN_E_NULL: return "required pointer is NULL";
    case MOLANN_E_DESC: return "inconsistent plan description";
    case MOLANN_E_INDEX: return "atom index outside [0, n_inp)";
    case MOLANN_E_FEATURE: return "unknown feature type or wrong atom count for its type";
    case MOLANN_E_STAGE: return "plan lacks the stage this call needs";
    case MOLANN_E_ALIGNMENT: return "pointer is not aligned to its element (4 bytes for the float32 entries, 8 for the float64 ones)";
    case MOLANN_E_UNSUPPORTED: return "shape not covered by the gfx950 kernels";
    case MOLANN_E_NOT_PACKED: return "MLP weights were never packed (call molann_plan_update_mlp)";
    case MOLANN_E_DEVICE: return "no gfx950 device";
    default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown error";
    }
}

int molann_plan_feature_dim(const molann_plan* p) { return p ? p->d_feat : MOLANN_E_NULL; }
int molann_plan_out_dim(const molann_plan* p) { return p ? p->out_dim : MOLANN_E_NULL; }
int molann_plan_kernel_family(const molann_plan* p) { return p ? p->family : MOLANN_E_NULL; }

int molann_plan_last_launch_info(const molann_plan* p, char* buf, int cap) {
    if (!p || !buf || cap <= 0) return MOLANN_E_NULL;
    snprintf(buf, (size_t)cap, "%s", p->last_info);
    return (int)strlen(buf);
}

int molann_plan_update_ref(molann_plan* p, const float* ref_x, molann_stream_t stream) {
    if (!p || !ref_x) return MOLANN_E_NULL;
    if (p->n_align <= 0) return MOLANN_E_STAGE;
    if (((uintptr_t)ref_x) & 3) return MOLANN_E_ALIGNMENT;
    hipLaunchKernelGGL(pack_ref_kernel<float>, dim3(1), dim3(256), 0, (hipStream_t)stream, p->d_ref, p->d_ref64, ref_x, p->n_align);
    return (int)hipGetLastError();
}

int molann_plan_update_ref_f64(molann_plan* p, const double* ref_x, molann_stream_t stream) {
    if (!p || !ref_x) return MOLANN_E_NULL;
    if (p->n_align <= 0) return MOLANN_E_STAGE;
    if (((uintptr_t)ref_x) & 7) return MOLANN_E_ALIGNMENT;
    hipLaunchKernelGGL(pack_ref_kernel<double>, dim3(1), dim3(256), 0, (hipStream_t)stream, p->d_ref, p->d_ref64, ref_x, p->n_align);
    return (int)hipGetLastError();
}

int molann_plan_update_mlp(molann_plan* p, const float* const* W, const float* const* b, molann_stream_t stream) {
    if (!p || !W || !b) return MOLANN_E_NULL;
    if (p->n_layers <= 0) return MOLANN_E_STAGE;
    PackArgs a;
    memset(&a, 0, sizeof(a));
    a.n_layers = p->n_layers;
    for (int i = 0; i <= p->n_layers; ++i) a.dims[i] = p->dims[i];
    for (int l = 0; l < p->n_layers; ++l) {   // every tensor is looked at before anything is packed: a refusal leaves the plan's copies as they were
        if (!W[l] || !b[l]) return MOLANN_E_NULL;
        if ((((uintptr_t)W[l]) & 3) || (((uintptr_t)b[l]) & 3)) return MOLANN_E_ALIGNMENT;
        a.W[l] = W[l]; a.b[l] = b[l];
        a.kp[l] = p->kp[l]; a.jp[l] = p->jp[l]; a.moff[l] = p->moff[l];
    }
    a.fused = p->fused_mlp ? 1 : 0;
    a.bf16 = p->mlp_prec == MOLANN_MLP_BF16;
    if (p->fused_mlp || p->lane_mlp)
        hipLaunchKernelGGL(pack_lane_kernel, dim3(8), dim3(256), 0, (hipStream_t)stream, p->d_wlane, a);
    // the MFMA copy serves molann_mlp_packed_f32 and the unfused forward
    hipLaunchKernelGGL(pack_mfma_kernel, dim3(64, p->n_layers), dim3(256), 0, (hipStream_t)stream, p->d_wmfma, a);
    if (p->chain_fn || p->wide_fn) {
        const ChainGeom g = chain_geom(p->dims, p->n_layers, p->mlp_prec == MOLANN_MLP_BF16);
        ChainPackArgs c;
        memset(&c, 0, sizeof(c));
        c.n_layers = g.nl; c.npair = g.npair(); c.bf16 = g.bf16; c.stream_bytes = p->chain_stream_bytes;
        for (int i = 0; i <= g.nl; ++i) { c.dims[i] = g.dims[i]; c.bias_off[i] = g.bias_off(i); }
        for (int l = 0; l < g.nl; ++l) { c.W[l] = W[l]; c.b[l] = b[l]; }
        int start = 0;
        for (int q = 0; q < c.npair; ++q) {
            c.pair_start[q] = start; c.slab_frags[q] = g.slab_frags(q); c.ks_in[q] = g.ks(2 * q);
            start += g.nchunk(q) * g.slab_frags(q);
        }
        c.pair_start[c.npair] = start;
        hipLaunchKernelGGL(pack_chain_kernel, dim3(256), dim3(256), 0, (hipStream_t)stream, p->d_wchain, c);
    }
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) p->mlp_packed = true;
    return (int)e;
}

static int check_io(const void* x, const void* out, int64_t n) {
    if (n < 0) return MOLANN_E_DESC;
    if (n == 0) return MOLANN_OK;
    if (!x || !out) return MOLANN_E_NULL;
    if ((((uintptr_t)x) & 3) || (((uintptr_t)out) & 3)) return MOLANN_E_ALIGNMENT;
    return MOLANN_OK;
}

int molann_align_f32(const molann_plan* cp, const float* x, int64_t n, float* out_xyz, molann_stream_t stream) {
    if (!cp) return MOLANN_E_NULL;
    molann_plan* p = const_cast<molann_plan*>(cp);
    if (p->n_align <= 0) return MOLANN_E_STAGE;
    const int c = check_io(x, out_xyz, n);
    if (c != MOLANN_OK || n == 0) return c;
    if (p->align_spec && p->align_state >= 0 && (debug_env().ablate & ~(32 | 512)) == 0) {
        if (p->align_state == 0) {
            std::lock_guard<std::mutex> lock(*p->jit_mu);
            if (p->align_state == 0) {
                BuiltKernel k;
                const bool built = build_kernel(jit_source(p->align_spec->j), "molann_lane_jit", "-fno-slp-vectorize", "alignment jit", k);
                p->align_mod = k.mod; p->align_fn = k.fn;
                p->align_state = built ? 1 : -1;
            }
        }
        if (p->align_state == 1) {
            const JitSpec& j = p->align_spec->j;
            const long n_tiles = (n + 63) / 64;
            const int grid = grid_for(p, n_tiles, 1, j.bpc);
            struct { const float* x; float* out; const double* ref64; const float* wfrag; long n; int out_vec4, pad_;
                     unsigned long long* stamps; const float* ref32; float* feat; } ka = {x, out_xyz, p->d_ref64, nullptr, (long)n, 0, 0, nullptr, p->d_ref, nullptr};
            size_t ksz = sizeof(ka);
            void* cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &ka, HIP_LAUNCH_PARAM_BUFFER_SIZE, &ksz, HIP_LAUNCH_PARAM_END};
            const int block = 64 * (j.ncons + j.nload);
            const hipError_t le = hipModuleLaunchKernel(p->align_fn, grid, 1, 1, block, 1, 1, 0, (hipStream_t)stream, nullptr, cfg);
            snprintf(p->last_info, sizeof(p->last_info), "molann_lane_jit<align_out> (plan-specialised; %d consumer waves + %d loader, ring of %d tiles) grid=%d block=%d lds=%d",
                     j.ncons, j.nload, j.nslot, grid, block, j.lds_block);
            return (int)le;
        }
    }
    return launch_pre(p, x, n, out_xyz, 1, false, (hipStream_t)stream);
}

int molann_features_f32(const molann_plan* cp, const float* x, int64_t n, float* out, molann_stream_t stream) {
    if (!cp) return MOLANN_E_NULL;
    molann_plan* p = const_cast<molann_plan*>(cp);
    if (p->n_items <= 0) return MOLANN_E_STAGE;
    const int c = check_io(x, out, n);
    if (c != MOLANN_OK || n == 0) return c;
    return launch_pre(p, x, n, out, 0, false, (hipStream_t)stream);
}

int molann_mlp_packed_f32(const molann_plan* cp, const float* f, int64_t n, float* out, molann_stream_t stream) {
    if (!cp) return MOLANN_E_NULL;
    molann_plan* p = const_cast<molann_plan*>(cp);
    if (p->n_layers <= 0) return MOLANN_E_STAGE;
    if (!p->mlp_packed) return MOLANN_E_NOT_PACKED;
    const int c = check_io(f, out, n);
    if (c != MOLANN_OK || n == 0) return c;
    const int e = launch_mlp(p, f, n, p->dims[0], out, (hipStream_t)stream);
    snprintf(p->last_info, sizeof(p->last_info), "%s", p->mlp_info);
    return e;
}

int molann_forward_packed_f32(const molann_plan* cp, const float* x, int64_t n, float* out, molann_stream_t stream) {
    if (!cp) return MOLANN_E_NULL;
    molann_plan* p = const_cast<molann_plan*>(cp);
    if (p->n_layers <= 0 || p->n_items <= 0) return MOLANN_E_STAGE;
    if (!p->mlp_packed) return MOLANN_E_NOT_PACKED;
    const int c = check_io(x, out, n);
    if (c != MOLANN_OK || n == 0) return c;
    if (p->fused_mlp) return launch_pre(p, x, n, out, 0, true, (hipStream_t)stream);
    if (p->wide_fn && (debug_env().ablate == 0)) return launch_wide(p, x, (long)n, out, (hipStream_t)stream);
    // unfused: features of a chunk -> plan workspace (cache resident) -> MFMA MLP.  Two workspace halves:
    // the MLP of chunk i runs on the plan's side stream while this stream already gathers chunk i+1
    // (HBM-bound gather next to an MFMA/L2-bound kernel); events fork and join, so capture still works.
    char info[256];
    info[0] = 0;
    hipStream_t main = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(*p->launch_mu);
    if (p->have_done && p->last_stream != main) HIP_TRY(hipStreamWaitEvent(main, p->ev_done, 0)); // another stream used the workspace last
    int i = 0, rc = MOLANN_OK;
    bool mlp_recorded[2] = {false, false};
    if (n <= p->work_frames) {
        // one chunk: nothing to overlap, so both kernels go to the caller's stream back to back - handing the chunk to the side
        // stream and back costs two cross-stream waits (~15 us each on this stack: [6, 64, 64, 8] at 1 M frames 226 -> 196 us)
        rc = launch_pre(p, x, (long)n, p->d_work, 0, false, main);
        if (rc == MOLANN_OK) {
            snprintf(info, sizeof(info), "%s", p->last_info);
            rc = launch_mlp(p, p->d_work, (long)n, p->d_feat, out, main);
        }
        if (hipEventRecord(p->ev_done, main) == hipSuccess) { p->have_done = true; p->last_stream = main; }
        if (rc != MOLANN_OK) return rc;
        snprintf(p->last_info, sizeof(p->last_info), "%.130s || %.90s chunk=%ld", info, p->mlp_info, p->work_frames);
        return MOLANN_OK;
    }
    for (int64_t s = 0; s < n && rc == MOLANN_OK; s += p->work_frames, ++i) {
        const int h = i & 1;
        const long m = (long)std::min<int64_t>(p->work_frames, n - s);
        float* work = p->d_work + (size_t)h * p->work_frames * p->d_feat;
        if (i >= 2 && (rc = (int)hipStreamWaitEvent(main, p->ev_mlp[h], 0)) != 0) break; // this half is free again
        if ((rc = launch_pre(p, x + s * (long)p->n_inp * 3, m, work, 0, false, main)) != 0) break;
        if (s == 0) snprintf(info, sizeof(info), "%s", p->last_info);
        if ((rc = (int)hipEventRecord(p->ev_feat[h], main)) != 0) break;
        if ((rc = (int)hipStreamWaitEvent(p->side, p->ev_feat[h], 0)) != 0) break;
        rc = launch_mlp(p, work, m, p->d_feat, out + s * (long)p->out_dim, p->side);
        const int er = (int)hipEventRecord(p->ev_mlp[h], p->side); // also behind a failed launch: the join below needs it
        if (er == 0) mlp_recorded[h] = true;
        if (rc == 0) rc = er;
    }
    // join - on the error paths too: whatever reached the side stream is ordered before the caller's next work
    for (int h = 0; h < 2; ++h)
        if (mlp_recorded[h]) {
            const int er = (int)hipStreamWaitEvent(main, p->ev_mlp[h], 0);
            if (rc == 0) rc = er;
        }
    if (hipEventRecord(p->ev_done, main) == hipSuccess) { p->have_done = true; p->last_stream = main; }
    if (rc != MOLANN_OK) return rc;
    snprintf(p->last_info, sizeof(p->last_info), "%.130s || %.90s chunk=%ld", info, p->mlp_info, p->work_frames);
    return MOLANN_OK;
}

int molann_forward_f32(molann_plan* p, const float* x, int64_t n, const float* const* W, const float* const* b,
                       float* out, molann_stream_t stream) {
    const int e = molann_plan_update_mlp(p, W, b, stream);
    if (e != MOLANN_OK) return e;
    return molann_forward_packed_f32(p, x, n, out, stream);
}

// The fused forward that also keeps the features, for a backward that does not recompute them
int molann_forward_train_f32(molann_plan* p, const float* x, int64_t n, float* out, float* features, molann_stream_t stream) {
    if (!p) return MOLANN_E_NULL;
    if (p->n_layers <= 0 || p->n_items <= 0) return MOLANN_E_STAGE;
    if (!p->fused_mlp && !(p->family == 1 && p->lane_mlp)) return MOLANN_E_UNSUPPORTED;
    if (!p->mlp_packed) return MOLANN_E_NOT_PACKED;
    const int c = check_io(x, out, n);
    if (c != MOLANN_OK || n == 0) return c;
    if (!features) return MOLANN_E_NULL;
    if (((uintptr_t)features) & 3) return MOLANN_E_ALIGNMENT;
    if (!p->fused_mlp) { // a small head behind a wave-per-frame kernel: the features land where the caller keeps them, the head reads them there
        std::lock_guard<std::mutex> lock(*p->launch_mu);
        int rc = launch_pre(p, x, (long)n, features, 0, false, (hipStream_t)stream);
        char info[160];
        snprintf(info, sizeof(info), "%.159s", p->last_info);
        if (rc == MOLANN_OK) rc = launch_mlp(p, features, (long)n, p->d_feat, out, (hipStream_t)stream);
        if (rc == MOLANN_OK) snprintf(p->last_info, sizeof(p->last_info), "%.130s || %.90s", info, p->mlp_info);
        return rc;
    }
    return launch_pre(p, x, (long)n, out, 0, true, (hipStream_t)stream, features);
}


// ---- float64 entry points (the reference's modules follow x.dtype) -------------------------------------------------
static int check_io_f64(const void* x, const void* out, int64_t n) {
    if (n < 0) return MOLANN_E_DESC;
    if (n == 0) return MOLANN_OK;
    if (!x || !out) return MOLANN_E_NULL;
    if ((((uintptr_t)x) & 7) || (((uintptr_t)out) & 7)) return MOLANN_E_ALIGNMENT;
    return MOLANN_OK;
}

static int launch_f64(const molann_plan* p, const double* x, int64_t n, double* out, int mode, hipStream_t stream, const char* what) {
    F64Args a;
    a.n_frames = n; a.n_inp = p->n_inp; a.n_align = p->n_align; a.n_items = p->n_items; a.out_cols = p->d_feat; a.mode = mode;
    const int grid = grid_for(p, n, 4, 8);
    hipLaunchKernelGGL(frames_f64_kernel, dim3(grid), dim3(256), 0, stream, x, out, p->d_align_idx, p->d_ref64, p->d_items, a);
    // the geometry as the plan's bound, not this call's grid: the text does not change with n_frames (a block takes four frames a round)
    snprintf(const_cast<molann_plan*>(p)->last_info, sizeof(p->last_info), "frames_f64_kernel (%s) grid<=%d block=256", what, grid_for(p, 1L << 40, 4, 8));
    return (int)hipGetLastError();
}

int molann_align_f64(const molann_plan* p, const double* x, int64_t n, double* out_xyz, molann_stream_t stream) {
    if (!p) return MOLANN_E_NULL;
    if (p->n_align <= 0) return MOLANN_E_STAGE;
    const int c = check_io_f64(x, out_xyz, n);
    if (c != MOLANN_OK || n == 0) return c;
    return launch_f64(p, x, n, out_xyz, 1, (hipStream_t)stream, "aligned coordinates");
}

int molann_features_f64(const molann_plan* p, const double* x, int64_t n, double* out, molann_stream_t stream) {
    if (!p) return MOLANN_E_NULL;
    if (p->n_items <= 0) return MOLANN_E_STAGE;
    const int c = check_io_f64(x, out, n);
    if (c != MOLANN_OK || n == 0) return c;
    return launch_f64(p, x, n, out, 0, (hipStream_t)stream, "features");
}

// dL/dx of molann_features_f64 for the same x: grad_f[N, feature_dim] -> grad_x[N, n_inp, 3], everything in double
int molann_features_backward_f64(const molann_plan* p, const double* x, const double* grad_f, int64_t n, double* grad_x, molann_stream_t stream) {
    if (!p) return MOLANN_E_NULL;
    if (p->n_items <= 0) return MOLANN_E_STAGE;
    if (n < 0) return MOLANN_E_DESC;
    if (n == 0) return MOLANN_OK;
    if (!x || !grad_f || !grad_x) return MOLANN_E_NULL;
    if ((((uintptr_t)x) & 7) || (((uintptr_t)grad_f) & 7) || (((uintptr_t)grad_x) & 7)) return MOLANN_E_ALIGNMENT;
    F64Args a;
    a.n_frames = n; a.n_inp = p->n_inp; a.n_align = p->n_align; a.n_items = p->n_items; a.out_cols = p->d_feat; a.mode = 0;
    const int grid = grid_for(p, n, 4, 8);
    hipLaunchKernelGGL(frames_bwd_f64_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, grad_f, grad_x, p->d_align_idx, p->d_ref64, p->d_items, a);
    snprintf(const_cast<molann_plan*>(p)->last_info, sizeof(p->last_info), "frames_bwd_f64_kernel grid<=%d block=256", grid_for(p, 1L << 40, 4, 8));
    return (int)hipGetLastError();
}

// The arguments of molann_mlp_f64, all looked at before anything is launched (molann_forward_f64 asks before its first kernel too):
// MOLANN_OK with the head's description in m and its LDS bytes in lds, or the refusal.
static int mlp_f64_arguments(const molann_plan* p, const double* f, int64_t n, const double* const* W, const double* const* b, const double* out,
                             F64Mlp& m, size_t& lds) {
    if (!p || !W || !b) return MOLANN_E_NULL;
    if (p->n_layers <= 0) return MOLANN_E_STAGE;
    const int c = check_io_f64(f, out, n);
    if (c != MOLANN_OK || n == 0) return c;
    memset(&m, 0, sizeof(m));
    m.n_layers = p->n_layers; m.act = p->act;
    for (int i = 0; i <= p->n_layers; ++i) { m.dims[i] = p->dims[i]; m.max_w = std::max(m.max_w, p->dims[i]); }
    for (int l = 0; l < p->n_layers; ++l) {
        if (!W[l] || !b[l]) return MOLANN_E_NULL;
        if ((((uintptr_t)W[l]) & 7) || (((uintptr_t)b[l]) & 7)) return MOLANN_E_ALIGNMENT;
        m.W[l] = W[l]; m.b[l] = b[l];
    }
    lds = (size_t)4 * 2 * m.max_w * sizeof(double);
    return lds > 65536 ? MOLANN_E_UNSUPPORTED : MOLANN_OK;
}

int molann_mlp_f64(const molann_plan* p, const double* f, int64_t n, const double* const* W, const double* const* b, double* out,
                   molann_stream_t stream) {
    F64Mlp m;
    size_t lds = 0;
    const int c = mlp_f64_arguments(p, f, n, W, b, out, m, lds);
    if (c != MOLANN_OK || n == 0) return c;
    const int grid = grid_for(p, n, 4, 8);
    hipLaunchKernelGGL(mlp_f64_kernel, dim3(grid), dim3(256), lds, (hipStream_t)stream, f, out, (long)n, m);
    snprintf(const_cast<molann_plan*>(p)->last_info, sizeof(p->last_info), "mlp_f64_kernel grid=%d block=256 lds=%zu", grid, lds);
    return (int)hipGetLastError();
}

int molann_forward_f64(const molann_plan* p, const double* x, int64_t n, const double* const* W, const double* const* b,
                       double* features_work, double* out, molann_stream_t stream) {
    if (!p) return MOLANN_E_NULL;
    if (p->n_layers <= 0 || p->n_items <= 0) return MOLANN_E_STAGE;
    if (n > 0 && !features_work) return MOLANN_E_NULL;
    int e = check_io_f64(x, features_work, n);
    if (e != MOLANN_OK || n == 0) return e;
    {   // the head's arguments before the features are launched: a refusal writes nothing
        F64Mlp m;
        size_t lds = 0;
        if ((e = mlp_f64_arguments(p, features_work, n, W, b, out, m, lds)) != MOLANN_OK) return e;
    }
    if ((e = molann_features_f64(p, x, n, features_work, stream)) != MOLANN_OK) return e;
    if ((e = molann_mlp_f64(p, features_work, n, W, b, out, stream)) != MOLANN_OK) return e;
    snprintf(const_cast<molann_plan*>(p)->last_info, sizeof(p->last_info), "frames_f64_kernel (features) + mlp_f64_kernel grid<=%d block=256 each",
             grid_for(p, 1L << 40, 4, 8));
    return e;
}

int molann_plan_grad_params_size(const molann_plan* p) { return p ? p->n_grad_params : MOLANN_E_NULL; }

int molann_plan_supports_backward(const molann_plan* p) {
    if (!p) return MOLANN_E_NULL;
    if (!p->geom[0].ok) { // large frames: the features (frames_wave_bwd_kernel), and a head within the fused MLP's limits behind them
        if (p->n_items <= 0) return 0;
        if (p->n_layers == 0) return 1;
        return (p->mlp_spec && p->mbwd_state >= 0 && rtc_api()->ok && act_served(p->act)) ? 1 : 0;
    }
    if (!p->spec || p->n_items <= 0 || p->bwd_state < 0 || !rtc_api()->ok) return 0;
    if (p->n_layers > 0 && (!p->fused_mlp || p->d_feat > LANE_MLP_MAX_WIDTH || p->mbwd_state < 0)) return 0;
    if (p->n_layers > 0 && !act_served(p->act)) return 0;
    return 1;
}

namespace {
// ---- backward: lazily built kernels and workspaces --------------------------------------------------------------------
// The workspaces (parameter partial sums, recomputed features) belong to the plan and are shared by all streams: the
// enqueue is serialised by launch_mu and a caller on another stream first waits for the event recorded behind the
// previous backward (the protocol of the unfused forward).
struct BwdGuard {
    molann_plan* p;
    hipStream_t s;
    std::unique_lock<std::mutex> lock;
    int rc;
    BwdGuard(molann_plan* plan, hipStream_t stream) : p(plan), s(stream), lock(*plan->launch_mu), rc(0) {
        if (p->have_bwork && p->bwork_stream != s) rc = (int)hipStreamWaitEvent(s, p->ev_bwork, 0);
    }
    ~BwdGuard() {
        if (hipEventRecord(p->ev_bwork, s) == hipSuccess) { p->have_bwork = true; p->bwork_stream = s; }
    }
};

int ensure_bwd_event(molann_plan* p) { // jit_mu held
    if (!p->ev_bwork) HIP_TRY(hipEventCreateWithFlags(&p->ev_bwork, hipEventDisableTiming));
    return MOLANN_OK;
}

// the MLP's description for its backward kernel: the lane plan's own, or the one made for a small head behind a wave-per-frame kernel
const JitSpecBox* mlp_box(const molann_plan* p) { return (p->spec && p->spec->j.n_layers > 0) ? p->spec : p->mlp_spec; }

int ensure_mlp_bwd(molann_plan* p) {
    if (!mlp_box(p)) return MOLANN_E_UNSUPPORTED;
    if (p->mbwd_state == 0 || !p->d_gpart) {
        std::lock_guard<std::mutex> lock(*p->jit_mu);
        if (p->mbwd_state == 0) {
            const int wpb = mlp_bwd_wpb(mlp_box(p)->j.dims, p->act);
            BuiltKernel k;
            const bool built = wpb >= 1 && build_kernel(jit_source_mlp_bwd(*mlp_box(p), wpb), "molann_mlp_bwd", nullptr, "mlp backward jit", k);
            p->mbwd_mod = k.mod; p->mbwd_fn = k.fn; p->mbwd_wpb = wpb;
            p->mbwd_state = built ? 1 : -1;
        }
        if (p->mbwd_state == 1 && !p->d_gpart) {
            { const int er = ensure_bwd_event(p); if (er != MOLANN_OK) return er; }
            HIP_TRY(hipMalloc((void**)&p->d_gpart, (size_t)p->num_cus * std::max(1, p->n_grad_params) * 4));
        }
    }
    return p->mbwd_state == 1 ? MOLANN_OK : MOLANN_E_UNSUPPORTED;
}

int ensure_chain_bwd(molann_plan* p) {
    if (p->cbwd_waves <= 0) return MOLANN_E_UNSUPPORTED;
    if (p->cbwd_state == 0 || !p->d_gpart) {
        std::lock_guard<std::mutex> lock(*p->jit_mu);
        if (p->cbwd_state == 0) {
            JitSpecBox b;      // (the head's sizes and the layout of its fp32 weight copy)
            set_layout(b, p->kp, p->jp, p->moff, p->n_layers);
            BuiltKernel k;
            const bool built = build_kernel(jit_source_chain_bwd(std::vector<int>(p->dims, p->dims + p->n_layers + 1), b.kp, b.jp, b.woff, p->act, p->cbwd_waves),
                                            "molann_chain_bwd", nullptr, "chain backward jit", k);
            p->cbwd_mod = k.mod; p->cbwd_fn = k.fn;
            p->cbwd_state = built ? 1 : -1;
        }
        if (p->cbwd_state == 1 && !p->d_gpart) {
            { const int er = ensure_bwd_event(p); if (er != MOLANN_OK) return er; }
            HIP_TRY(hipMalloc((void**)&p->d_gpart, (size_t)p->num_cus * std::max(1, p->n_grad_params) * 4));
        }
    }
    return p->cbwd_state == 1 ? MOLANN_OK : MOLANN_E_UNSUPPORTED;
}

int ensure_features_bwd(molann_plan* p, molann_plan::LaneGeom& g) {
    features_bwd_geometry(p->n_inp, g);
    if (!g.ok) return MOLANN_E_UNSUPPORTED;
    if (p->bwd_state == 0) {
        std::lock_guard<std::mutex> lock(*p->jit_mu);
        if (p->bwd_state == 0) {
            JitSpecBox b = *p->spec;
            b.j.wpb = g.wpb;
            BuiltKernel k;
            const bool built = build_kernel(jit_source_bwd(b, g.lds_per_wave), "molann_lane_bwd", nullptr, "backward jit", k);
            p->bwd_mod = k.mod; p->bwd_fn = k.fn;
            p->bwd_state = built ? 1 : -1;
        }
    }
    return p->bwd_state == 1 ? MOLANN_OK : MOLANN_E_UNSUPPORTED;
}

// the one-pass backward of the plan (molann_bwd_ring.inc): built at the first backward; a build that does not fit the LDS or
// needs scratch memory (register spills) leaves the two-kernel path in charge
int ensure_ring_bwd(molann_plan* p) {
    if (p->rbwd_state == 0 || (p->rbwd_state == 1 && p->n_grad_params > 0 && !p->d_gpart)) {
        std::lock_guard<std::mutex> lock(*p->jit_mu);
        if (p->rbwd_state == 0) {
            int st = -1;
            JitSpecBox b = *p->spec;
            const char* off = getenv("MOLANN_NO_RING_BWD");
            if (!(off && off[0] == '1') && p->geom[0].ok && bwd_ring_geometry(b.j, p->n_grad_params)) {
                // The kernel lives at the edge of its 256 registers.  Without SLP vectorisation first (C3: 2267 vector instructions and
                // no scratch, against 2564 + 16 spilled registers with it); the default for the plans that spill without it.
                const std::string src = jit_source_bwd_ring(b);
                for (int attempt = 0; attempt < 2 && st != 1; ++attempt) {
                    BuiltKernel k;
                    if (!build_kernel(src, "molann_bwd_ring", attempt == 0 ? "-fno-slp-vectorize" : nullptr, "one-pass backward", k)) continue;
                    if (k.scratch != 0) {
                        if (getenv("MOLANN_JIT_VERBOSE")) fprintf(stderr, "molann one-pass backward, build %d not used (scratch=%d)\n", attempt, k.scratch);
                        k.unload();
                        continue;
                    }
                    p->rbwd_mod = k.mod; p->rbwd_fn = k.fn;
                    p->rbwd_ncons = b.j.ncons; p->rbwd_nload = b.j.nload; p->rbwd_nslot = b.j.nslot; p->rbwd_lds = b.j.lds_block;
                    st = 1;
                }
            }
            p->rbwd_state = st;
        }
        if (p->rbwd_state == 1 && p->n_grad_params > 0 && !p->d_gpart) {
            { const int er = ensure_bwd_event(p); if (er != MOLANN_OK) return er; }
            HIP_TRY(hipMalloc((void**)&p->d_gpart, (size_t)p->num_cus * p->n_grad_params * 4));
        }
    }
    return p->rbwd_state == 1 ? MOLANN_OK : MOLANN_E_UNSUPPORTED;
}

// molann_bwd_ring (+ reduce_rows_kernel); with parameter gradients the caller holds the workspace (BwdGuard)
int launch_ring_bwd(molann_plan* p, const float* x, const float* grad_out, long n, float* grad_x, float* grad_params, hipStream_t stream,
                    float* values = nullptr) {
    const long n_tiles = (n + 63) / 64;
    const int grid = (int)std::max<long>(1, std::min<long>(p->num_cus, n_tiles));
    const bool params = grad_params && p->n_grad_params > 0;
    struct { const float* x; const float* gout; const double* ref64; const float* ref32; const float* wnat; float* gx; float* gp; long n; float* y; } ka =
        {x, grad_out, p->d_ref64, p->d_ref, (const float*)p->d_wmfma, grad_x, params ? p->d_gpart : nullptr, n, values};
    size_t ksz = sizeof(ka);
    void* cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &ka, HIP_LAUNCH_PARAM_BUFFER_SIZE, &ksz, HIP_LAUNCH_PARAM_END};
    const int block = 64 * (p->rbwd_ncons + p->rbwd_nload);
    const hipError_t le = hipModuleLaunchKernel(values ? p->vjp_fn : p->rbwd_fn, grid, 1, 1, block, 1, 1, 0, stream, nullptr, cfg);
    if (le != hipSuccess) return (int)le;
    if (params) {
        hipLaunchKernelGGL(reduce_rows_kernel, dim3((p->n_grad_params + 63) / 64), dim3(1024), 0, stream, p->d_gpart, grid, p->n_grad_params,
                           grad_params);
        HIP_TRY(hipGetLastError());
    }
    snprintf(p->last_info, sizeof(p->last_info), "molann_bwd_ring%s (plan-specialised; %d consumer waves + %d loader, ring of %d tiles) grid=%d block=%d lds=%d%s",
             values ? "<values>" : "", p->rbwd_ncons, p->rbwd_nload, p->rbwd_nslot, grid, block, p->rbwd_lds, params ? " + reduce_rows_kernel" : "");
    return MOLANN_OK;
}

// molann_lane_bwd: grad_f -> grad_x (no workspace)
int launch_features_bwd(molann_plan* p, const molann_plan::LaneGeom& g, const float* x, const float* grad_f, long n, float* grad_x,
                        hipStream_t stream) {
    const long n_tiles = (n + 63) / 64;
    int bpc = (int)(163840 / ((long)g.wpb * g.lds_per_wave));
    if (bpc < 1) bpc = 1;
    if (bpc * g.wpb > 8) bpc = std::max(1, 8 / g.wpb);
    const int grid = grid_for(p, n_tiles, g.wpb, bpc);
    struct { const float* x; const float* gf; const double* ref64; float* gx; long n; int x_wide; } ka =
        {x, grad_f, p->d_ref64, grad_x, n, (((uintptr_t)x) & 15) == 0 ? 1 : 0};
    size_t ksz = sizeof(ka);
    void* cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &ka, HIP_LAUNCH_PARAM_BUFFER_SIZE, &ksz, HIP_LAUNCH_PARAM_END};
    const hipError_t le = hipModuleLaunchKernel(p->bwd_fn, grid, 1, 1, 64 * g.wpb, 1, 1, (unsigned)((size_t)g.wpb * g.lds_per_wave), stream,
                                                nullptr, cfg);
    snprintf(p->last_info, sizeof(p->last_info), "molann_lane_bwd (plan-specialised) grid=%d block=%d", grid, 64 * g.wpb);
    return (int)le;
}

// molann_chain_bwd (+ reduce_rows_kernel when parameter gradients are wanted); the caller holds the workspace (BwdGuard).
// One block per CU at most (its weight copy fills the LDS), tiles of 16 WAVES frames handed out statically: the grid, and with it
// every block's partial sums, depend on n alone.
int launch_chain_bwd(molann_plan* p, const float* f, const float* grad_out, long n, float* grad_f, float* grad_params, hipStream_t stream) {
    const long n_tiles = (n + 16 * p->cbwd_waves - 1) / (16 * p->cbwd_waves);
    const int grid = (int)std::max<long>(1, std::min<long>(p->num_cus, n_tiles));
    struct { const float* f; const float* gout; const float* wnat; float* gf; float* gp; long n; } ka =
        {f, grad_out, (const float*)p->d_wmfma, grad_f, grad_params ? p->d_gpart : nullptr, n};
    size_t ksz = sizeof(ka);
    void* cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &ka, HIP_LAUNCH_PARAM_BUFFER_SIZE, &ksz, HIP_LAUNCH_PARAM_END};
    const hipError_t le = hipModuleLaunchKernel(p->cbwd_fn, grid, 1, 1, 64 * p->cbwd_waves, 1, 1, 0, stream, nullptr, cfg);
    if (le != hipSuccess) return (int)le;
    if (grad_params) {
        hipLaunchKernelGGL(reduce_rows_kernel, dim3((p->n_grad_params + 63) / 64), dim3(1024), 0, stream, p->d_gpart, grid, p->n_grad_params,
                           grad_params);
        HIP_TRY(hipGetLastError());
    }
    snprintf(p->last_info, sizeof(p->last_info), "molann_chain_bwd (plan-specialised) grid=%d block=%d%s", grid, 64 * p->cbwd_waves,
             grad_params ? " + reduce_rows_kernel" : "");
    return MOLANN_OK;
}

// molann_mlp_bwd (+ reduce_rows_kernel when parameter gradients are wanted); the caller holds the workspace (BwdGuard)
int launch_mlp_bwd(molann_plan* p, const float* f, const float* grad_out, long n, float* grad_f, float* grad_params, hipStream_t stream) {
    const long n_tiles = (n + 63) / 64;
    const int grid = (int)std::max<long>(1, std::min<long>(p->num_cus, (n_tiles + p->mbwd_wpb - 1) / p->mbwd_wpb)); // one block per CU
    struct { const float* f; const float* gout; const float* wnat; float* gf; float* gp; long n; } ka =
        {f, grad_out, (const float*)p->d_wmfma, grad_f, grad_params ? p->d_gpart : nullptr, n};
    size_t ksz = sizeof(ka);
    void* cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &ka, HIP_LAUNCH_PARAM_BUFFER_SIZE, &ksz, HIP_LAUNCH_PARAM_END};
    const hipError_t le = hipModuleLaunchKernel(p->mbwd_fn, grid, 1, 1, 64 * p->mbwd_wpb, 1, 1, 0, stream, nullptr, cfg);
    if (le != hipSuccess) return (int)le;
    if (grad_params) {
        hipLaunchKernelGGL(reduce_rows_kernel, dim3((p->n_grad_params + 63) / 64), dim3(1024), 0, stream, p->d_gpart, grid, p->n_grad_params,
                           grad_params);
        HIP_TRY(hipGetLastError());
    }
    snprintf(p->last_info, sizeof(p->last_info), "molann_mlp_bwd (plan-specialised) grid=%d block=%d%s", grid, 64 * p->mbwd_wpb,
             grad_params ? " + reduce_rows_kernel" : "");
    return MOLANN_OK;
}
} // namespace

// the backward's workspace (recomputed features and their gradients, two halves), allocated at the first backward that needs it
static int ensure_bwork(molann_plan* p) {
    if (!p->d_bwork) {
        std::lock_guard<std::mutex> lock(*p->jit_mu);
        if (!p->d_bwork) {
            long bf = std::min<long>(1l << 20, (64l << 20) / ((long)p->d_feat * 4)) & ~63l;
            bf = std::max<long>(bf, 4096);
            float* w = nullptr;
            HIP_TRY(hipMalloc((void**)&w, 2 * (size_t)bf * p->d_feat * 4));
            p->bwork_frames = bf;
            p->d_bwork = w;
        }
    }
    return MOLANN_OK;
}

// dL/dx of the features of LARGE frames (one wave per frame): grad_f[N, d_feat] -> grad_x[N, n_inp, 3]
static int launch_wave_bwd(molann_plan* p, const float* x, const float* grad_f, int64_t n, float* grad_x, hipStream_t stream) {
    if (!grad_x) return MOLANN_OK;
    if ((((uintptr_t)x) & 3) || (((uintptr_t)grad_f) & 3) || (((uintptr_t)grad_x) & 3)) return MOLANN_E_ALIGNMENT;
    PreArgs a;
    fill_pre_args(p, a, n, 0, p->d_feat, false, x, grad_x);
    // the aligned frame itself (one position item per atom): the dense gradient, cotangent and frame in registers
    if (p->dense_positions && p->n_inp <= 24 * 512) {
        AlignRegsArgs ra;
        memset(&ra, 0, sizeof(ra));
        ra.n_frames = n; ra.n_inp = p->n_inp; ra.n_align = p->n_align; ra.first_align = p->align_first;
        // the cotangent in registers (x passes through): as the forward, the fewest data waves with <= 24 atoms per thread
        int W = 1;
        while ((p->n_inp + 64 * W - 1) / (64 * W) > 24) W *= 2;
        const int units = ((p->n_inp + 64 * W - 1) / (64 * W) + 3) / 4;
        const void* fn = nullptr;
#define ALIGN_BWD_CASE(WW, UU) if (W == WW && units == UU) fn = (const void*)frames_align_bwd_regs_kernel<WW, UU>;
        ALIGN_BWD_CASE(1, 1) ALIGN_BWD_CASE(1, 2) ALIGN_BWD_CASE(1, 3) ALIGN_BWD_CASE(1, 4) ALIGN_BWD_CASE(1, 5) ALIGN_BWD_CASE(1, 6)
        ALIGN_BWD_CASE(2, 4) ALIGN_BWD_CASE(2, 5) ALIGN_BWD_CASE(2, 6) ALIGN_BWD_CASE(4, 4) ALIGN_BWD_CASE(4, 5) ALIGN_BWD_CASE(4, 6)
        ALIGN_BWD_CASE(8, 4) ALIGN_BWD_CASE(8, 5) ALIGN_BWD_CASE(8, 6)
#undef ALIGN_BWD_CASE
        if (fn) {
            int occ = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, 64 * (W + 2), 0) != hipSuccess || occ < 1) occ = 1;
            occ = std::min(occ, std::max(2, (int)(245760 / (24l * p->n_inp))));      // ~240 KB of frame + cotangent in flight per CU
            if (debug_env().wave_bpc > 0) occ = std::min(occ, debug_env().wave_bpc);
            const int grid = (int)std::min<long>(n, (long)p->num_cus * occ);
            void* kargs[] = {(void*)&x, (void*)&grad_f, (void*)&grad_x, (void*)&p->d_align_idx, (void*)&p->d_align_slot, (void*)&p->d_ref, (void*)&p->d_ref64, (void*)&ra};
            const hipError_t le = hipLaunchKernel(fn, dim3(grid), dim3(64 * (W + 2)), kargs, 0, stream);
            snprintf(p->last_info, sizeof(p->last_info), "frames_align_bwd_regs_kernel<W=%d,U=%d> (%d data waves + a forward and a backward solver wave, %d blocks per CU) grid=%d block=%d",
                     W, units, W, occ, grid, 64 * (W + 2));
            return le != hipSuccess ? (int)le : (int)hipGetLastError();
        }
    }
    const int per_wave = ((p->n_items * 48 + 15) / 16) * 16;   // g_y of every item's four atoms
    // mid-size frames with an alignment: B frames per wave and round (frames_group_bwd_kernel), the tables in LDS
    if (p->bw_touched > 0 && p->n_align > 0 && getenv("MOLANN_BWD_ATOMICS") == nullptr && getenv("MOLANN_NO_BWD_GROUP") == nullptr &&
        (p->n_inp <= 1024 || getenv("MOLANN_BWD_GROUP_ALL") != nullptr)) {
        const int wpb = 4;
        int nb = 8;
        while (nb > 1 && (long)nb * p->n_items > 256) nb /= 2;
        GroupBwdArgs gb;
        memset(&gb, 0, sizeof(gb));
        gb.n_touched = p->bw_touched; gb.n_list = p->bw_list_len; gb.gy_frame = 12 * p->n_items;
        size_t off = (size_t)ceil_to(8 * (3 * p->n_align + 8), 16);
        gb.off_ref32 = (int)off; off += (size_t)ceil_to(4 * (3 * p->n_align + 8), 16);
        gb.off_align = (int)off; off += (size_t)ceil_to(4 * p->n_align, 16);
        gb.off_items = (int)off; off += (size_t)32 * p->n_items;
        gb.off_bw_atoms = (int)off; off += (size_t)ceil_to(4 * p->bw_touched, 16);
        gb.off_bw_ptr = (int)off; off += (size_t)ceil_to(4 * (p->bw_touched + 1), 16);
        gb.off_bw_list = (int)off; off += (size_t)ceil_to(4 * p->bw_list_len, 16);
        gb.off_bw_align = (int)off; off += (size_t)ceil_to(4 * p->bw_touched, 16);
        gb.off_gy = (int)off; off += (size_t)wpb * nb * gb.gy_frame * 4;
        if (nb > 1 && off <= 65536) {
            const long n_rounds = (n + nb - 1) / nb;
            const int bpc = (int)std::max<size_t>(1, std::min<size_t>(8, 160 * 1024 / off));
            const int grid = grid_for(p, n_rounds, wpb, bpc);
#define LAUNCH_GROUP_BWD(BB) hipLaunchKernelGGL((frames_group_bwd_kernel<BB>), dim3(grid), dim3(64 * wpb), off, stream, x, grad_f, grad_x, p->d_align_idx, p->d_ref, \
                                            p->d_ref64, p->d_items, p->d_bw_atoms, p->d_bw_ptr, p->d_bw_list, p->d_bw_align, a, gb)
            if (nb == 8) LAUNCH_GROUP_BWD(8);
            else if (nb == 4) LAUNCH_GROUP_BWD(4);
            else LAUNCH_GROUP_BWD(2);
#undef LAUNCH_GROUP_BWD
            snprintf(p->last_info, sizeof(p->last_info), "frames_group_bwd_kernel<B=%d> (frames_wave_bwd on %d frames per wave and round) grid=%d block=%d lds=%zu",
                     nb, nb, grid, 64 * wpb, off);
            return (int)hipGetLastError();
        }
    }
    if (p->bw_touched > 0 && per_wave <= 65536 && getenv("MOLANN_BWD_ATOMICS") == nullptr) {
        const int wpb = std::max(1, std::min(4, 65536 / per_wave));
        const int bpc = std::max(1, std::min(8, 160 * 1024 / (wpb * per_wave)));
        const int grid = grid_for(p, n, wpb, bpc);
        BwGatherArgs b = {p->bw_touched, per_wave};
        hipLaunchKernelGGL(frames_wave_bwd_gather_kernel, dim3(grid), dim3(64 * wpb), (size_t)wpb * per_wave, stream, x, grad_f,
                           grad_x, p->d_align_idx, p->d_ref, p->d_ref64, p->d_items, p->d_bw_atoms, p->d_bw_ptr, p->d_bw_list, p->d_bw_align,
                           a, b);
        snprintf(p->last_info, sizeof(p->last_info), "frames_wave_bwd_gather_kernel grid=%d block=%d lds=%d", grid, 64 * wpb, wpb * per_wave);
        return (int)hipGetLastError();
    }
    const int wpb = 4;
    const int grid = grid_for(p, n, wpb, 8);
    hipLaunchKernelGGL(frames_wave_bwd_kernel, dim3(grid), dim3(64 * wpb), 0, stream, x, grad_f, grad_x,
                       p->d_align_idx, p->d_ref, p->d_ref64, p->d_items, a);
    snprintf(p->last_info, sizeof(p->last_info), "frames_wave_bwd_kernel grid=%d block=%d", grid, 64 * wpb);
    return (int)hipGetLastError();
}

// dL/dx and dL/d(parameters) of molann_forward_packed_f32 / molann_features_f32 for the same x.
int molann_backward_f32(molann_plan* p, const float* x, const float* grad_out, int64_t n, float* grad_x, float* grad_params,
                        molann_stream_t stream) {
    if (!p) return MOLANN_E_NULL;
    if (n < 0) return MOLANN_E_DESC;
    if (n == 0) return MOLANN_OK;
    if (!x || !grad_out) return MOLANN_E_NULL;
    if (!p->geom[0].ok && p->n_items > 0 && p->n_layers == 0) // large frames: one wave per frame, no parameters
        return launch_wave_bwd(p, x, grad_out, n, grad_x, (hipStream_t)stream);
    if (!p->geom[0].ok && p->n_items > 0) { // large frames, a small head: features (recomputed) -> MLP backward -> wave-per-frame backward
        if (!molann_plan_supports_backward(p)) return MOLANN_E_UNSUPPORTED;
        if (!p->mlp_packed) return MOLANN_E_NOT_PACKED;
        if ((((uintptr_t)x) & 3) || (((uintptr_t)grad_out) & 3) || (((uintptr_t)grad_x) & 3) || (((uintptr_t)grad_params) & 3)) return MOLANN_E_ALIGNMENT;
        if (!grad_x && !grad_params) return MOLANN_OK;
        int rc = ensure_mlp_bwd(p);
        if (rc != MOLANN_OK) return rc;
        if ((rc = ensure_bwork(p)) != MOLANN_OK) return rc;
        hipStream_t main = (hipStream_t)stream;
        BwdGuard guard(p, main);
        if (guard.rc != 0) return guard.rc;
        float* wf = p->d_bwork;
        float* wg = p->d_bwork + (size_t)p->bwork_frames * p->d_feat;
        char info[3][96];
        info[0][0] = info[1][0] = info[2][0] = 0;
        for (int64_t s = 0; s < n && rc == MOLANN_OK; s += p->bwork_frames) {
            const long m = (long)std::min<int64_t>(p->bwork_frames, n - s);
            const float* xs = x + s * (long)p->n_inp * 3;
            if ((rc = launch_pre(p, xs, m, wf, 0, false, main)) != 0) break;
            if (s == 0) snprintf(info[0], sizeof(info[0]), "%.95s", p->last_info);
            if ((rc = launch_mlp_bwd(p, wf, grad_out + s * (long)p->out_dim, m, grad_x ? wg : nullptr, grad_params, main)) != 0) break;
            if (s == 0) snprintf(info[1], sizeof(info[1]), "%.95s", p->last_info);
            if (grad_x && (rc = launch_wave_bwd(p, xs, wg, m, grad_x + s * (long)p->n_inp * 3, main)) != 0) break;
            if (s == 0 && grad_x) snprintf(info[2], sizeof(info[2]), "%.95s", p->last_info);
        }
        if (rc == MOLANN_OK)
            snprintf(p->last_info, sizeof(p->last_info), "%.72s || %.72s || %.72s || chunks of %ld frames", info[0], info[1], info[2], p->bwork_frames);
        return rc;
    }
    if (!p->spec || p->n_items <= 0) return MOLANN_E_UNSUPPORTED;
    if (p->n_layers == 0 || molann_plan_supports_backward(p)) { // one pass over x when the plan's kernel could be built
        if (p->n_layers > 0 && !p->mlp_packed) return MOLANN_E_NOT_PACKED;
        if ((((uintptr_t)x) & 3) || (((uintptr_t)grad_out) & 3) || (((uintptr_t)grad_x) & 3) || (((uintptr_t)grad_params) & 3)) return MOLANN_E_ALIGNMENT;
        if (!grad_x && !(grad_params && p->n_layers > 0)) return MOLANN_OK;
        const int er = ensure_ring_bwd(p);
        if (er == MOLANN_OK) {
            if (!(grad_params && p->n_grad_params > 0)) return launch_ring_bwd(p, x, grad_out, (long)n, grad_x, nullptr, (hipStream_t)stream);
            BwdGuard guard(p, (hipStream_t)stream);
            if (guard.rc != 0) return guard.rc;
            return launch_ring_bwd(p, x, grad_out, (long)n, grad_x, grad_params, (hipStream_t)stream);
        }
        if (er != MOLANN_E_UNSUPPORTED) return er;
    }
    if (p->n_layers == 0) return molann_features_backward_f32(p, x, grad_out, n, grad_x, stream);
    // plans with an MLP, nothing saved from the forward: features (recomputed) -> MLP backward -> preprocessing backward,
    // in chunks through the plan's backward workspace (allocated at the first call, like the kernels are compiled then)
    if (!molann_plan_supports_backward(p)) return MOLANN_E_UNSUPPORTED;
    if (!p->mlp_packed) return MOLANN_E_NOT_PACKED;
    if ((((uintptr_t)x) & 3) || (((uintptr_t)grad_out) & 3) || (((uintptr_t)grad_x) & 3) || (((uintptr_t)grad_params) & 3)) return MOLANN_E_ALIGNMENT;
    if (!grad_x && !grad_params) return MOLANN_OK;
    molann_plan::LaneGeom g;
    int rc = ensure_mlp_bwd(p);
    if (rc == MOLANN_OK && grad_x) rc = ensure_features_bwd(p, g);
    if (rc != MOLANN_OK) return rc;
    if ((rc = ensure_bwork(p)) != MOLANN_OK) return rc;
    hipStream_t main = (hipStream_t)stream;
    BwdGuard guard(p, main);
    if (guard.rc != 0) return guard.rc;
    float* wf = p->d_bwork;
    float* wg = p->d_bwork + (size_t)p->bwork_frames * p->d_feat;
    char info[3][96];
    info[0][0] = info[1][0] = info[2][0] = 0;
    for (int64_t s = 0; s < n && rc == MOLANN_OK; s += p->bwork_frames) {
        const long m = (long)std::min<int64_t>(p->bwork_frames, n - s);
        const float* xs = x + s * (long)p->n_inp * 3;
        if ((rc = launch_pre(p, xs, m, wf, 0, false, main)) != 0) break;
        if (s == 0) snprintf(info[0], sizeof(info[0]), "%.95s", p->last_info);
        if ((rc = launch_mlp_bwd(p, wf, grad_out + s * (long)p->out_dim, m, grad_x ? wg : nullptr, grad_params, main)) != 0) break;
        if (s == 0) snprintf(info[1], sizeof(info[1]), "%.95s", p->last_info);
        if (grad_x && (rc = launch_features_bwd(p, g, xs, wg, m, grad_x + s * (long)p->n_inp * 3, main)) != 0) break;
        if (s == 0 && grad_x) snprintf(info[2], sizeof(info[2]), "%.95s", p->last_info);
    }
    if (rc == MOLANN_OK)
        snprintf(p->last_info, sizeof(p->last_info), "%.72s || %.72s || %.72s || chunks of %ld frames", info[0], info[1], info[2], p->bwork_frames);
    return rc;
}

namespace {
// the one-pass backward's build that also stores the forward's outputs (molann_bwd_ring.inc, WITH_VALUES), built at the first use
int ensure_ring_vjp(molann_plan* p) {
    const int er = ensure_ring_bwd(p);       // the geometry is the one-pass backward's
    if (er != MOLANN_OK) return er;
    if (p->vjp_state == 0) {
        std::lock_guard<std::mutex> lock(*p->jit_mu);
        if (p->vjp_state == 0) {
            int st = -1;
            JitSpecBox b = *p->spec;
            if (bwd_ring_geometry(b.j, p->n_grad_params)) {
                b.j.with_values = true;
                const std::string src = jit_source_bwd_ring(b);
                for (int attempt = 0; attempt < 2 && st != 1; ++attempt) {   // (scratch is tolerated here: a latency path, not a throughput path)
                    BuiltKernel k;
                    if (!build_kernel(src, "molann_bwd_ring", attempt == 0 ? "-fno-slp-vectorize" : nullptr, "value + vjp build", k)) continue;
                    p->vjp_mod = k.mod; p->vjp_fn = k.fn;
                    st = 1;
                }
            }
            p->vjp_state = st;
        }
    }
    return p->vjp_state == 1 ? MOLANN_OK : MOLANN_E_UNSUPPORTED;
}

// Frames the lane kernels do not take (mid-size and large): molann_group_vjp.inc, for heads within the fused MLP's limits (every
// width and the feature dimension <= 32, <= 4 layers, fp32; tanh, ReLU, sigmoid, identity, SiLU, LeakyReLU - the fp32 MFMA
// copy of the weights is packed for every plan) and for features-only plans.  Built at the first use; E_UNSUPPORTED where the
// tables do not fit the LDS at B >= 2 or hipRTC is missing.
bool group_vjp_serves(const molann_plan* p) {
    if (p->geom[0].ok || p->n_items <= 0 || p->va_touched <= 0 || !rtc_api()->ok) return false;
    return p->n_layers == 0 || head_is_small(p->dims, p->n_layers, p->d_feat, p->mlp_prec, p->act);
}

int ensure_group_vjp(molann_plan* p) {
    if (!group_vjp_serves(p)) return MOLANN_E_UNSUPPORTED;
    if (p->gvjp_state == 0) {
        std::lock_guard<std::mutex> lock(*p->jit_mu);
        if (p->gvjp_state == 0) {
            int st = -1;
            std::vector<int> dims;
            JitSpecBox b;
            if (p->n_layers > 0) dims.assign(p->dims, p->dims + p->n_layers + 1);
            set_layout(b, p->kp, p->jp, p->moff, p->n_layers);
            GroupVjpGeom g;
            BuiltKernel k;
            if (group_vjp_geometry(dims, p->act, p->d_feat, p->n_align, p->n_items, p->va_touched, p->va_list_len, g) &&
                build_kernel(jit_source_group_vjp(dims, b.kp, b.jp, b.woff, p->act, p->d_feat, p->n_inp, p->n_align, p->n_items, p->va_touched, p->va_list_len, g),
                             "molann_group_vjp", nullptr, "group value + vjp build", k)) {
                // blocks per CU at the launch's block size: all WPB waves (batches of at most one tile per CU), or half of them
                const int waves = g.wpb > 1 ? g.wpb / 2 : 1;
                int occ = 0;
                if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&occ, k.fn, 64 * waves, 0) != hipSuccess || occ < 1)
                    occ = std::max(1, std::min(163840 / g.lds, 32 / waves));
                p->gvjp_mod = k.mod; p->gvjp_fn = k.fn;
                p->gvjp_b = g.b; p->gvjp_wpb = g.wpb; p->gvjp_lds = g.lds; p->gvjp_bpc = occ;
                st = 1;
            }
            p->gvjp_state = st;
        }
    }
    return p->gvjp_state == 1 ? MOLANN_OK : MOLANN_E_UNSUPPORTED;
}

// one block per 64-frame tile (tiles strided over the blocks): WPB waves per block while the batch has at most one tile per CU
// (latency: a round per wave), else half of them and as many blocks as the CUs hold.  No workspace, nothing but the enqueue.
int launch_group_vjp(molann_plan* p, const float* x, const float* grad_out, long n, float* out, float* grad_x, hipStream_t stream) {
    const long n_tiles = (n + 63) / 64;
    const bool wide = n_tiles <= p->num_cus || p->gvjp_wpb == 1;
    const int waves = wide ? p->gvjp_wpb : p->gvjp_wpb / 2;
    const int grid = (int)std::max<long>(1, std::min<long>((long)p->num_cus * (wide ? 1 : p->gvjp_bpc), n_tiles));
    struct { const float* x; const float* gout; const double* ref64; const float* ref32; const int* align; const int* items; const int* atoms;
             const int* ptr; const int* list; const float* wnat; float* out; float* gx; long n; } ka =
        {x, grad_out, p->d_ref64, p->d_ref, p->d_align_idx, (const int*)p->d_items, p->d_va_atoms, p->d_va_ptr, p->d_va_list,
         (const float*)p->d_wmfma, out, grad_x, n};
    size_t ksz = sizeof(ka);
    void* cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &ka, HIP_LAUNCH_PARAM_BUFFER_SIZE, &ksz, HIP_LAUNCH_PARAM_END};
    const hipError_t le = hipModuleLaunchKernel(p->gvjp_fn, grid, 1, 1, 64 * waves, 1, 1, 0, stream, nullptr, cfg);
    if (le != hipSuccess) return (int)le;
    snprintf(p->last_info, sizeof(p->last_info), "molann_group_vjp<B=%d> (values + vjp in one launch; %d waves per 64-frame tile) grid=%d block=%d lds=%d",
             p->gvjp_b, waves, grid, 64 * waves, p->gvjp_lds);
    return MOLANN_OK;
}
} // namespace

// The forward's outputs AND the vector-Jacobian product of a batch in ONE launch: the one-pass backward recomputes the forward per
// frame anyway, so a build of it that also stores the outputs (WITH_VALUES: one more product on the matrix cores, from the
// activations already in its scratch) returns both.  For callers that differentiate a small batch at every step with a cotangent
// they know up front - or want the Jacobian: a batch of d_out copies of a frame with the identity as cotangent (README.rst:49's
// use, a collective variable inside an MD engine).  Parameters are data here (no parameter gradients).  Plans the one-pass
// backward serves (molann_plan_backward_kind == 2), and frames the lane kernels do not take (molann_group_vjp.inc: the three
// launches of their backward as one); E_UNSUPPORTED otherwise.  The first call builds the kernel: outside a capture.
int molann_value_and_vjp_f32(molann_plan* p, const float* x, const float* grad_out, int64_t n, float* out, float* grad_x, molann_stream_t stream) {
    if (!p) return MOLANN_E_NULL;
    if (n < 0) return MOLANN_E_DESC;
    if (n == 0) return MOLANN_OK;
    if (!x || !grad_out || !out || !grad_x) return MOLANN_E_NULL;
    if ((((uintptr_t)x) & 3) || (((uintptr_t)grad_out) & 3) || (((uintptr_t)grad_x) & 3) || (((uintptr_t)out) & 3)) return MOLANN_E_ALIGNMENT;
    if (!p->geom[0].ok) {
        const int er = ensure_group_vjp(p);
        if (er != MOLANN_OK) return er;
        if (p->n_layers > 0 && !p->mlp_packed) return MOLANN_E_NOT_PACKED;
        return launch_group_vjp(p, x, grad_out, (long)n, out, grad_x, (hipStream_t)stream);
    }
    if (!p->spec || p->n_items <= 0) return MOLANN_E_UNSUPPORTED;
    if (p->n_layers > 0 && (!molann_plan_supports_backward(p) || !p->fused_mlp)) return MOLANN_E_UNSUPPORTED;
    if (p->n_layers > 0 && !p->mlp_packed) return MOLANN_E_NOT_PACKED;
    const int er = ensure_ring_vjp(p);
    if (er != MOLANN_OK) return er;
    return launch_ring_bwd(p, x, grad_out, (long)n, grad_x, nullptr, (hipStream_t)stream, out);
}

// 1 when molann_value_and_vjp_f32 serves the plan, 0 otherwise.  Builds the kernel it reports.
int molann_plan_supports_value_and_vjp(molann_plan* p) {
    if (!p) return MOLANN_E_NULL;
    if (!p->geom[0].ok) return ensure_group_vjp(p) == MOLANN_OK ? 1 : 0;
    if (!p->spec || p->n_items <= 0) return 0;
    if (p->n_layers > 0 && (!molann_plan_supports_backward(p) || !p->fused_mlp)) return 0;
    return ensure_ring_vjp(p) == MOLANN_OK ? 1 : 0;
}

// how molann_backward_f32 will serve this plan: 2 one pass over x (nothing worth saving from the forward), 1 two kernels
// (a caller that keeps the features of its forward saves their recompute), 0 not at all.  Builds the kernel it reports.
int molann_plan_backward_kind(molann_plan* p) {
    if (!p) return MOLANN_E_NULL;
    if (!molann_plan_supports_backward(p)) return 0;
    if (!p->geom[0].ok || !p->spec) return 1;
    return ensure_ring_bwd(p) == MOLANN_OK ? 2 : 1;
}

// dL/dx of molann_features_f32 for the same x: grad_f[N, feature_dim] -> grad_x[N, n_inp, 3]
int molann_features_backward_f32(molann_plan* p, const float* x, const float* grad_f, int64_t n, float* grad_x, molann_stream_t stream) {
    if (!p) return MOLANN_E_NULL;
    if (n < 0) return MOLANN_E_DESC;
    if (n == 0) return MOLANN_OK;
    if (!x || !grad_f) return MOLANN_E_NULL;
    if (!p->geom[0].ok) { // large frames: the wave-per-frame kernel
        if (p->n_items <= 0) return MOLANN_E_UNSUPPORTED;
        return launch_wave_bwd(p, x, grad_f, n, grad_x, (hipStream_t)stream);
    }
    if (!p->spec || p->n_items <= 0) return MOLANN_E_UNSUPPORTED;
    if (!grad_x) return MOLANN_OK;
    if ((((uintptr_t)x) & 3) || (((uintptr_t)grad_f) & 3) || (((uintptr_t)grad_x) & 3)) return MOLANN_E_ALIGNMENT;
    molann_plan::LaneGeom g;
    const int rc = ensure_features_bwd(p, g);
    if (rc != MOLANN_OK) return rc;
    return launch_features_bwd(p, g, x, grad_f, (long)n, grad_x, (hipStream_t)stream);
}

// 1 when molann_mlp_backward_f32 serves the plan's head: the fused family's kernel (molann_mlp_bwd.inc) or, for a wide fp32 head
// whose chain stream is resident, molann_chain_bwd.inc.  Builds the kernel it reports.
int molann_plan_supports_mlp_backward(molann_plan* p) {
    if (!p) return MOLANN_E_NULL;
    if (p->n_layers <= 0) return 0;
    if (mlp_box(p) && molann_plan_supports_backward(p)) return 1;
    return ensure_chain_bwd(p) == MOLANN_OK ? 1 : 0;
}

// dL/df and dL/d(parameters) of molann_mlp_packed_f32 for the same f (the fused family: every width <= 32; a wide fp32 head
// with a resident chain stream)
int molann_mlp_backward_f32(molann_plan* p, const float* f, const float* grad_out, int64_t n, float* grad_f, float* grad_params,
                            molann_stream_t stream) {
    if (!p) return MOLANN_E_NULL;
    if (n < 0) return MOLANN_E_DESC;
    if (n == 0) return MOLANN_OK;
    if (!f || !grad_out) return MOLANN_E_NULL;
    if (p->n_layers <= 0) return MOLANN_E_STAGE;
    const bool chain = !(mlp_box(p) && molann_plan_supports_backward(p));
    if (chain && p->cbwd_waves <= 0) return MOLANN_E_UNSUPPORTED;
    if (!p->mlp_packed) return MOLANN_E_NOT_PACKED;
    if ((((uintptr_t)f) & 3) || (((uintptr_t)grad_out) & 3) || (((uintptr_t)grad_f) & 3) || (((uintptr_t)grad_params) & 3)) return MOLANN_E_ALIGNMENT;
    if (!grad_f && !grad_params) return MOLANN_OK;
    if (chain) {
        const int rc = ensure_chain_bwd(p);
        if (rc != MOLANN_OK) return rc;
        if (!grad_params) return launch_chain_bwd(p, f, grad_out, (long)n, grad_f, nullptr, (hipStream_t)stream);
        BwdGuard guard(p, (hipStream_t)stream);
        if (guard.rc != 0) return guard.rc;
        return launch_chain_bwd(p, f, grad_out, (long)n, grad_f, grad_params, (hipStream_t)stream);
    }
    const int rc = ensure_mlp_bwd(p);
    if (rc != MOLANN_OK) return rc;
    if (!grad_params) return launch_mlp_bwd(p, f, grad_out, (long)n, grad_f, nullptr, (hipStream_t)stream); // no workspace involved
    BwdGuard guard(p, (hipStream_t)stream);
    if (guard.rc != 0) return guard.rc;
    return launch_mlp_bwd(p, f, grad_out, (long)n, grad_f, grad_params, (hipStream_t)stream);
}

// the hook's answer: the source in buf and its length; compiled too when asked (bit 1) - then a failure leaves the build log in buf
static int debug_jit_answer(const std::string& src, int do_compile, const char* flags, char* buf, int cap) {
    if (buf && cap > 0) snprintf(buf, (size_t)cap, "%s", src.c_str());
    if (do_compile & 1) {
        std::vector<char> code;
        std::string log;
        const int rc = jit_compile(src, code, log, flags);
        if (rc != 0) {
            if (buf && cap > 0) snprintf(buf, (size_t)cap, "%s", log.c_str());
            return rc > 0 ? rc : MOLANN_E_UNSUPPORTED;
        }
    }
    return (int)src.size();
}

// diagnostic / test hook: generate (and optionally compile, needs no GPU) a plan-specialised kernel's source for a description.
// Returns the source length, or a negative MOLANN_E_* / positive hiprtcResult.  Items, slots, windows, the head's layout and the
// chain geometry are plan_choose's, every kernel's own geometry comes from the function its builder calls, so the source is the one
// a plan of this description builds.  A kernel the plan would not build for the description is generated all the same (a head is
// also asked for on its own, under a feature list that is not its input: E_DESC is plan creation's refusal, not the hook's).
int molann_debug_jit(const molann_plan_desc* d, int do_compile, char* buf, int cap) {
    const int v = validate_desc(d);
    if (v != MOLANN_OK) return v;
    PlanChoice c;
    const int chosen = plan_choose(d, c);
    if (chosen != MOLANN_OK && chosen != MOLANN_E_DESC) return chosen;
    const int nl = d->n_layers, act = d->activation;
    std::vector<int> dims;
    if (nl > 0) dims.assign(d->layer_dims, d->layer_dims + nl + 1);
    JitSpecBox b;      // the backward kernels read the fp32 copy of the weights
    {
        int kp[MOLANN_MAX_LAYERS], jp[MOLANN_MAX_LAYERS];
        long off[MOLANN_MAX_LAYERS];
        mlp_layout(d->layer_dims, nl, false, kp, jp, off);
        set_layout(b, kp, jp, off, nl);
    }
    if (do_compile & 512) { // values + vjp in one launch for frames the lane kernels do not take (ensure_group_vjp)
        if (c.items.empty()) return MOLANN_E_UNSUPPORTED;
        if (nl > 0 && !head_is_small(d->layer_dims, nl, std::max(c.d_feat, d->layer_dims[0]), d->mlp_precision, act)) return MOLANN_E_UNSUPPORTED;
        std::vector<int> atoms, ptr, list;
        group_vjp_tables(d->n_inp, c.items, d->align_idx, d->n_align, atoms, ptr, list);
        GroupVjpGeom g;
        if (!group_vjp_geometry(dims, act, c.d_feat, d->n_align, (int)c.items.size(), (int)atoms.size(), (int)list.size(), g)) return MOLANN_E_UNSUPPORTED;
        return debug_jit_answer(jit_source_group_vjp(dims, b.kp, b.jp, b.woff, act, c.d_feat, d->n_inp, d->n_align, (int)c.items.size(), (int)atoms.size(),
                                                     (int)list.size(), g), do_compile, nullptr, buf, cap);
    }
    if (do_compile & 256) { // the backward of a wide fp32 head with a resident stream (ensure_chain_bwd)
        if (nl <= 0) return MOLANN_E_STAGE;
        if (d->mlp_precision != MOLANN_MLP_F32 || !act_served(act) || !chain_resident(c.cg)) return MOLANN_E_UNSUPPORTED;
        const int waves = chain_bwd_waves(b.kp, b.jp);
        if (waves <= 0) return MOLANN_E_UNSUPPORTED;
        return debug_jit_answer(jit_source_chain_bwd(dims, b.kp, b.jp, b.woff, act, waves), do_compile, nullptr, buf, cap);
    }
    if (do_compile & 4) { // the chain MLP kernel at the FB plan creation starts from
        if (nl <= 0) return MOLANN_E_STAGE;
        const int fb = chain_fb_bound(c.cg);
        if (fb == 0) return MOLANN_E_UNSUPPORTED;
        return debug_jit_answer(jit_source_chain(c.cg, act, fb), do_compile, nullptr, buf, cap);
    }
    if (!c.lane_spec_ok) return MOLANN_E_UNSUPPORTED;
    JitSpec j = c.fwd;     // with the whole head in the kernel, whether or not the plan fuses it
    j.n_layers = nl; j.out_cols = c.out_dim; j.dims = dims;
    if (do_compile & 128) { // the WIDE_MLP build (the whole forward of a wide head in the lane kernel)
        if (nl <= 0 || d->mlp_precision != MOLANN_MLP_F32) return MOLANN_E_STAGE;
        if (!chain_resident(c.cg) || c.cg.total_frags() * 1024 > 112 * 1024) return MOLANN_E_UNSUPPORTED;
        j = wide_lane_spec(d, c);
    }
    molann_plan::LaneGeom g;
    jit_geometry(j, g, c.d_feat, c.cols_needed, j.wide_mlp ? 8 : 14);
    if (!g.ok || 3 * d->n_inp < 4) return MOLANN_E_UNSUPPORTED;
    j.save_feat = (do_compile & 32) != 0 && nl > 0;   // the feature-keeping twin of the fused forward
    if (!(do_compile & 2)) return debug_jit_answer(jit_source(j), do_compile, "-fno-slp-vectorize", buf, cap);
    b.j = j;               // the backward kernels of the same plan
    if (do_compile & (16 | 8))
        for (int w : dims) if (w > LANE_MLP_MAX_WIDTH) return MOLANN_E_UNSUPPORTED;
    if (do_compile & 16) { // ... in one pass (ensure_ring_bwd; bit 64: the build that also stores the forward's outputs, ensure_ring_vjp)
        if (!bwd_ring_geometry(b.j, grad_params_count(d->layer_dims, nl))) return MOLANN_E_UNSUPPORTED;
        b.j.with_values = (do_compile & 64) != 0;
        return debug_jit_answer(jit_source_bwd_ring(b), do_compile, nullptr, buf, cap);
    }
    if (do_compile & 8) { // ... its MLP half (ensure_mlp_bwd)
        if (nl <= 0) return MOLANN_E_STAGE;
        const int wpb = mlp_bwd_wpb(dims, act);
        if (wpb < 1) return MOLANN_E_UNSUPPORTED;
        return debug_jit_answer(jit_source_mlp_bwd(b, wpb), do_compile, nullptr, buf, cap);
    }
    molann_plan::LaneGeom gb; // ... its preprocessing half (ensure_features_bwd)
    features_bwd_geometry(d->n_inp, gb);
    b.j.wpb = gb.wpb;
    return debug_jit_answer(jit_source_bwd(b, gb.lds_per_wave), do_compile, nullptr, buf, cap);
}

// diagnostic: read and clear the phase-stamp sums (16 x u64; [0..5] consumer phases, [6] clock ratio, [7] = number of
// consumer waves that reported, [8..10] loader: waiting for a free slot / issuing DMA / waiting for a tile to land,
// [11] loader waves, [12] tiles issued)
int molann_debug_read_stamps(unsigned long long* out16) {
    if (!out16) return MOLANN_E_NULL;
    unsigned long long zero[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_stamps), sizeof(zero)));
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), zero, sizeof(zero)));
    return MOLANN_OK;
}

// ---- self-test hooks: the same __host__ __device__ source, compiled for the host -------------
int molann_selftest_kabsch_rotation(const double* H9, double e0, float* R9) {
    if (!H9 || !R9) return MOLANN_E_NULL;
    double h[9];
    float r[9];
    for (int i = 0; i < 9; ++i) h[i] = H9[i];
    kabsch_rotation(h, e0, r);
    for (int i = 0; i < 9; ++i) R9[i] = r[i];
    return MOLANN_OK;
}

int molann_selftest_kabsch_rotation_f32(const float* H9, float e0, float* R9) {
    if (!H9 || !R9) return MOLANN_E_NULL;
    float h[9], r[9];
    for (int i = 0; i < 9; ++i) h[i] = H9[i];
    kabsch_rotation_f32(h, e0, r);
    for (int i = 0; i < 9; ++i) R9[i] = r[i];
    return MOLANN_OK;
}

int molann_selftest_feature(int type, int use_angle_value, const float* a, float* out3) {
    if (!a || !out3) return MOLANN_E_NULL;
    int it;
    if (type == MOLANN_FEAT_ANGLE) it = use_angle_value ? IT_ANGLE_VAL : IT_ANGLE_COS;
    else if (type == MOLANN_FEAT_BOND) it = IT_BOND;
    else if (type == MOLANN_FEAT_DIHEDRAL) it = use_angle_value ? IT_DIHEDRAL_VAL : IT_DIHEDRAL_CS;
    else if (type == MOLANN_FEAT_POSITION) it = IT_POSITION;
    else return MOLANN_E_FEATURE;
    float v[3] = {0.f, 0.f, 0.f};
    const int w = eval_item(it, v3(a[0], a[1], a[2]), v3(a[3], a[4], a[5]), v3(a[6], a[7], a[8]), v3(a[9], a[10], a[11]), v);
    for (int i = 0; i < w; ++i) out3[i] = v[i];
    return w;
}

float molann_selftest_activation(int act, float v) { return apply_activation(act, v); }

int molann_selftest_feature_backward(int type, int use_angle_value, const float* a, const float* g3, float* ga12) {
    if (!a || !g3 || !ga12) return MOLANN_E_NULL;
    int it;
    if (type == MOLANN_FEAT_ANGLE) it = use_angle_value ? IT_ANGLE_VAL : IT_ANGLE_COS;
    else if (type == MOLANN_FEAT_BOND) it = IT_BOND;
    else if (type == MOLANN_FEAT_DIHEDRAL) it = use_angle_value ? IT_DIHEDRAL_VAL : IT_DIHEDRAL_CS;
    else if (type == MOLANN_FEAT_POSITION) it = IT_POSITION;
    else return MOLANN_E_FEATURE;
    V3 g[4] = {v3(0, 0, 0), v3(0, 0, 0), v3(0, 0, 0), v3(0, 0, 0)};
    const float gg[3] = {g3[0], g3[1], g3[2]};
    eval_item_backward(it, v3(a[0], a[1], a[2]), v3(a[3], a[4], a[5]), v3(a[6], a[7], a[8]), v3(a[9], a[10], a[11]), gg, g[0],
                       g[1], g[2], g[3]);
    for (int i = 0; i < 4; ++i) { ga12[3 * i] = g[i].x; ga12[3 * i + 1] = g[i].y; ga12[3 * i + 2] = g[i].z; }
    return MOLANN_OK;
}

int molann_selftest_kabsch_backward(const double* H9, const float* R9, const float* GR9, float* GH9) {
    if (!H9 || !R9 || !GR9 || !GH9) return MOLANN_E_NULL;
    double h[9];
    float r[9], gr[9], gh[9];
    for (int i = 0; i < 9; ++i) { h[i] = H9[i]; r[i] = R9[i]; gr[i] = GR9[i]; }
    kabsch_rotation_backward(h, r, gr, gh);
    for (int i = 0; i < 9; ++i) GH9[i] = gh[i];
    return MOLANN_OK;
}

float molann_selftest_act_derivative(int act, float z) { return act_derivative(act, z, apply_activation(act, z)); }

static int selftest_item_type(int type, int use_angle_value) {
    if (type == MOLANN_FEAT_ANGLE) return use_angle_value ? IT_ANGLE_VAL : IT_ANGLE_COS;
    if (type == MOLANN_FEAT_BOND) return IT_BOND;
    if (type == MOLANN_FEAT_DIHEDRAL) return use_angle_value ? IT_DIHEDRAL_VAL : IT_DIHEDRAL_CS;
    if (type == MOLANN_FEAT_POSITION) return IT_POSITION;
    return -1;
}

int molann_selftest_feature_tangent_f32(int type, int use_angle_value, const float* a, const float* t, float* out3, float* dout3) {
    if (!a || !t || !out3 || !dout3) return MOLANN_E_NULL;
    const int it = selftest_item_type(type, use_angle_value);
    if (it < 0) return MOLANN_E_FEATURE;
    float v[3] = {0.f, 0.f, 0.f}, dv[3] = {0.f, 0.f, 0.f};
    const int w = eval_item_tangent(it, v3(a[0], a[1], a[2]), v3(a[3], a[4], a[5]), v3(a[6], a[7], a[8]), v3(a[9], a[10], a[11]),
                                    v3(t[0], t[1], t[2]), v3(t[3], t[4], t[5]), v3(t[6], t[7], t[8]), v3(t[9], t[10], t[11]), v, dv);
    for (int i = 0; i < w; ++i) { out3[i] = v[i]; dout3[i] = dv[i]; }
    return w;
}

int molann_selftest_feature_tangent_f64(int type, int use_angle_value, const double* a, const double* t, double* out3, double* dout3) {
    if (!a || !t || !out3 || !dout3) return MOLANN_E_NULL;
    const int it = selftest_item_type(type, use_angle_value);
    if (it < 0) return MOLANN_E_FEATURE;
    double v[3] = {0., 0., 0.}, dv[3] = {0., 0., 0.};
    const int w = eval_item_tangent_f64(it, v3d(a[0], a[1], a[2]), v3d(a[3], a[4], a[5]), v3d(a[6], a[7], a[8]), v3d(a[9], a[10], a[11]),
                                        v3d(t[0], t[1], t[2]), v3d(t[3], t[4], t[5]), v3d(t[6], t[7], t[8]), v3d(t[9], t[10], t[11]), v, dv);
    for (int i = 0; i < w; ++i) { out3[i] = v[i]; dout3[i] = dv[i]; }
    return w;
}

int molann_selftest_kabsch_rotation_f64(const double* H9, double e0, double* R9) {
    if (!H9 || !R9) return MOLANN_E_NULL;
    double h[9], r[9];
    for (int i = 0; i < 9; ++i) h[i] = H9[i];
    kabsch_rotation_t<double, double>(h, e0, r);
    for (int i = 0; i < 9; ++i) R9[i] = r[i];
    return MOLANN_OK;
}

int molann_selftest_kabsch_tangent(const double* H9, const double* R9, const double* dH9, double* dR9) {
    if (!H9 || !R9 || !dH9 || !dR9) return MOLANN_E_NULL;
    double h[9], r[9], dh[9], dr[9];
    for (int i = 0; i < 9; ++i) { h[i] = H9[i]; r[i] = R9[i]; dh[i] = dH9[i]; }
    kabsch_rotation_tangent_t<double>(h, r, dh, dr);
    for (int i = 0; i < 9; ++i) dR9[i] = dr[i];
    return MOLANN_OK;
}

int molann_selftest_kabsch_backward_f64(const double* H9, const double* R9, const double* GR9, double* GH9) {
    if (!H9 || !R9 || !GR9 || !GH9) return MOLANN_E_NULL;
    double h[9], r[9], gr[9], gh[9];
    for (int i = 0; i < 9; ++i) { h[i] = H9[i]; r[i] = R9[i]; gr[i] = GR9[i]; }
    kabsch_rotation_backward_t<double, double>(h, r, gr, gh);
    for (int i = 0; i < 9; ++i) GH9[i] = gh[i];
    return MOLANN_OK;
}

} // extern "C"
