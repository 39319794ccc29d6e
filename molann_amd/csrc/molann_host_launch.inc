// molann_host_launch.inc - part of libmolann_hip.so, included by molann_kernels.hip (one translation unit: the kernels' host stubs and the
// launches that use them must see each other).  Host: launch_pre (alignment / features / fused forward: which kernel serves a plan) and launch_mlp.
namespace {

// preprocessing (align / features / fused forward) for n_frames starting at x -> out
int launch_pre(molann_plan* p, const float* x, long n_frames, float* out, int mode, bool with_mlp,
               hipStream_t stream, float* feat_out = nullptr) {
    // a feature plan that is the aligned frame (one position item per atom; AlignmentLayer.forward under autograd): its feature
    // rows [N, 3 n_inp] are what the alignment kernels write
    if (mode == 0 && !with_mlp && p->dense_positions && !feat_out) mode = 1;
    const int out_cols = mode == 1 ? 0 : (with_mlp ? p->out_dim : p->d_feat);
    PreArgs a;
    fill_pre_args(p, a, n_frames, mode, out_cols, with_mlp, x, out);
    // the plan-specialised lane kernel first: it serves every plan it was built for, including few-atom plans on
    // frames too large for the ahead-of-time lane kernel's dense tile
    const bool jit_allowed = mode == 0 && (a.ablate & ~(32 | 64 | 128 | 256 | 512 | 1024 | 2048)) == 0;
    auto launch_jit = [&](hipFunction_t fn, int nl, int ncons, int nload, int nslot, int bpc, int lds_block) {
        const long n_tiles = (n_frames + 63) / 64;
        const int jgrid = grid_for(p, n_tiles, 1, bpc);   // every block needs at least one tile
        const size_t jlds = (size_t)debug_env().lds_pad;   // the kernel declares its block's LDS statically
        unsigned long long* stamps = nullptr;
        if (a.ablate & 32) (void)hipGetSymbolAddress((void**)&stamps, HIP_SYMBOL(g_stamps));
        struct { const float* x; float* out; const double* ref64; const float* wfrag; long n; int out_vec4, pad_;
                 unsigned long long* stamps; const float* ref32; float* feat; } ka = {x, out, p->d_ref64, p->d_wlane, n_frames, a.out_vec4, 0,
                                                                                     stamps, p->d_ref, feat_out};
        size_t ksz = sizeof(ka);
        void* cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &ka, HIP_LAUNCH_PARAM_BUFFER_SIZE, &ksz, HIP_LAUNCH_PARAM_END};
        const int jblock = 64 * (ncons + nload);
        const hipError_t le = hipModuleLaunchKernel(fn, jgrid, 1, 1, jblock, 1, 1, (unsigned)jlds, stream, nullptr, cfg);
        snprintf(p->last_info, sizeof(p->last_info), "molann_lane_jit<NL=%d> (plan-specialised; %d consumer waves + %d loader, ring of %d tiles) grid=%d block=%d lds=%d",
                 nl, ncons, nload, nslot, jgrid, jblock, lds_block);
        return (int)le;
    };
    if (feat_out) { // training forward: the fused kernel's twin that keeps the features, built now
        if (!(jit_allowed && with_mlp && p->jit_fn && p->jit_nl == p->n_layers && p->jit_nl > 0 && p->spec)) return MOLANN_E_UNSUPPORTED;
        if (p->train_state == 0) {
            std::lock_guard<std::mutex> lock(*p->jit_mu);
            if (p->train_state == 0) {
                JitSpec j = p->spec->j;
                j.save_feat = true;
                BuiltKernel k;
                const bool built = build_kernel(jit_source(j), "molann_lane_jit", "-fno-slp-vectorize", "training-forward jit", k);
                p->train_mod = k.mod; p->train_fn = k.fn;
                p->train_state = built ? 1 : -1;
            }
        }
        if (p->train_state != 1) return MOLANN_E_UNSUPPORTED;
        return launch_jit(p->train_fn, p->jit_nl, p->jit_ncons, p->jit_nload, p->jit_nslot, p->jit_bpc, p->jit_lds_block);
    }
    if (jit_allowed && p->jit_fn && p->jit_nl == (with_mlp ? p->n_layers : 0))
        return launch_jit(p->jit_fn, p->jit_nl, p->jit_ncons, p->jit_nload, p->jit_nslot, p->jit_bpc, p->jit_lds_block);
    if (jit_allowed && !with_mlp && p->jit_fn && p->jit_nl > 0 && p->spec && p->feat_state >= 0) {
        // features of a plan whose forward kernel has the MLP fused in: the same kernel text without the MLP, built now
        if (p->feat_state == 0) {
            std::lock_guard<std::mutex> lock(*p->jit_mu);
            if (p->feat_state == 0) {
                JitSpec j = p->spec->j;
                j.n_layers = 0; j.out_cols = j.d_feat; j.dims.clear();
                molann_plan::LaneGeom g;
                memset(&g, 0, sizeof(g));
                jit_geometry(j, g, std::max(1, j.d_feat), std::max(1, j.d_feat));
                BuiltKernel k;
                const bool built = g.ok && build_kernel(jit_source(j), "molann_lane_jit", "-fno-slp-vectorize", "features jit", k);
                p->feat_mod = k.mod; p->feat_fn = k.fn;
                p->feat_ncons = j.ncons; p->feat_nload = j.nload; p->feat_nslot = j.nslot; p->feat_bpc = j.bpc; p->feat_lds_block = j.lds_block;
                p->feat_state = built ? 1 : -1;
            }
        }
        if (p->feat_state == 1)
            return launch_jit(p->feat_fn, 0, p->feat_ncons, p->feat_nload, p->feat_nslot, p->feat_bpc, p->feat_lds_block);
    }
    const molann_plan::LaneGeom& g = p->geom[mode == 1 ? 1 : 0];
    if (mode == 0 && p->jit_only && (with_mlp || !g.ok)) return MOLANN_E_UNSUPPORTED; // served by the specialised kernel only, and a diagnostic switch excluded it
    if (g.ok) {
        const int wpb = g.wpb;
        const long n_tiles = (n_frames + 63) / 64;
        int bpc = (int)(163840 / ((long)wpb * g.lds_per_wave));
        if (bpc < 1) bpc = 1;
        if (bpc * wpb > 16) bpc = std::max(1, 16 / wpb);
        const int grid = grid_for(p, n_tiles, wpb, bpc);
        size_t lds = (size_t)wpb * g.lds_per_wave;
        lds += (size_t)debug_env().lds_pad; // diagnostic: lower the occupancy
        const dim3 block(64 * wpb);
        const int w = with_mlp ? p->n_layers : 0;
        const bool regs = p->regs_mode;
#define LAUNCH_LANE(W, M)                                                                                         \
    hipLaunchKernelGGL((frames_lane_kernel<W, M>), dim3(grid), block, lds, stream, x, out, p->d_align_idx, p->d_ref, \
                       p->d_ref64, (M == 2 ? p->d_items_slot : p->d_items), p->d_slots, p->d_wlane, a)
#define LAUNCH_LANE_W(M)            \
    if (w == 0) LAUNCH_LANE(0, M);  \
    else if (w == 1) LAUNCH_LANE(1, M); \
    else if (w == 2) LAUNCH_LANE(2, M); \
    else if (w == 3) LAUNCH_LANE(3, M); \
    else LAUNCH_LANE(4, M)
        if (mode == 1) LAUNCH_LANE(0, 1);
        else if (regs) { LAUNCH_LANE_W(2); }
        else { LAUNCH_LANE_W(0); }
#undef LAUNCH_LANE_W
#undef LAUNCH_LANE
        snprintf(p->last_info, sizeof(p->last_info), "frames_lane_kernel<%d,%s> grid=%d block=%d lds=%zu", w,
                 mode == 1 ? "align_out" : (regs ? "features_regs" : "features_lds"), grid, 64 * wpb, lds);
    } else if (mode == 0 && p->ring_nd > 0 && getenv("MOLANN_NO_RING") == nullptr) {
        // large frames, features: every frame staged once into an LDS ring by loader waves (frames_ring_kernel)
        const int nd = p->ring_nd;
        // frames per ring entry: with an alignment, as many as keep an entry within 8 KB (one rotation solve per entry:
        // frames_ring_kernel); MOLANN_RING_BATCH=1: one frame per entry whatever the size
        int nb = (p->n_align > 0 && nd <= 4) ? 8 / nd : 1;
        if (nd == 3) nb = 2;
        { const char* e = getenv("MOLANN_RING_BATCH"); if (e && atoi(e) >= 1 && atoi(e) < nb) nb = atoi(e) >= 4 ? 4 : (atoi(e) >= 2 ? 2 : 1); }
        if (nd * nb > 8) nb = 1;
        const int img = nd * nb * 1024;
        RingArgs ra;
        memset(&ra, 0, sizeof(ra));
        ra.n_frames = n_frames; ra.frame_bytes = 12 * p->n_inp; ra.n_align = p->n_align; ra.n_items = p->n_items;
        ra.out_cols = a.out_cols; ra.n_win = p->ring_nwin;
        ra.n_slot = std::min(16, (163840 - RING_HEADER - (nb > 1 ? ceil_to(28 * p->n_align, 16) : 0)) / img);
        ra.n_load = ra.n_slot >= 6 ? 2 : 1;
        // a consumer keeps its slot while it computes from the image: slots = consumers + what the loaders keep in flight
        ra.n_cons = std::max(1, std::min(14, ra.n_slot - 2 * ra.n_load));
        ra.depth = std::max(0, std::min(std::min(6, 63 / (nd * nb)), (ra.n_slot - ra.n_cons) / ra.n_load - 1));
        // entries of several small frames: the loaders are the limit (a wave's gathers of a few dozen windows retire about one per
        // 1000 cycles whatever the depth, so the rate grows with the number of loader waves) and the consumers - one short
        // reduction and one solve per entry - need few waves.  P1, 524 288 frames: 8 + 4 waves 287 us, 6 + 6 232, 5 + 7 211, 4 + 8 217-225,
        // 3 + 9 285; consumers that do nothing (8 + 4): 272.  Larger plans keep eight consumers.
        if (nb >= 4 && ra.n_slot >= 16) {
            const bool light = p->n_align <= 64 && (long)nb * p->n_items <= 128;
            ra.n_cons = light ? 5 : 8; ra.n_load = light ? 7 : 4; ra.depth = light ? 0 : 1;
        }
        if (nb > 1) ra.n_cons = std::min(ra.n_cons, 12 - ra.n_load);      // the B > 1 kernels are built for blocks of <= 12 waves
        if (debug_env().wave_bpc > 0) ra.n_cons = std::max(1, std::min(ra.n_cons, debug_env().wave_bpc)); // MOLANN_WAVE_BPC: experiment with fewer consumers
        { const char* e = getenv("MOLANN_RING_NT"); ra.nt = e ? (e[0] == '1') : 1; }
        if (const char* e = diag_env("MOLANN_DEBUG_RING")) {   // experiments: "slots,consumers,loaders,depth"
            int ns = 0, nc = 0, nl = 0, dp = 0;
            if (sscanf(e, "%d,%d,%d,%d", &ns, &nc, &nl, &dp) == 4 && ns >= 1 && ns <= 16 && nc >= 1 && nl >= 1 && nc + nl <= (nb > 1 ? 12 : 16) &&
                (size_t)RING_HEADER + (size_t)ns * img + (nb > 1 ? ceil_to(28 * p->n_align, 16) : 0) <= 163840 && dp >= 0 && (dp + 1) * nd * nb <= 63) {
                ra.n_slot = ns; ra.n_cons = nc; ra.n_load = nl; ra.depth = dp;
            }
        }
        { const char* e = diag_env("MOLANN_DEBUG_RING_FLAGS"); ra.flags = e ? atoi(e) : 0; }
        const int block = 64 * (ra.n_cons + ra.n_load);
        const size_t tab = nb > 1 ? (size_t)ceil_to(28 * p->n_align, 16) : 0;     // B > 1: the consumers' alignment tables
        const size_t lds = (size_t)RING_HEADER + (size_t)ra.n_slot * img + tab;
        const int grid = (int)std::min<long>((n_frames + nb - 1) / nb, p->num_cus);
#define LAUNCH_RING(N, NB)                                                                                                \
    if (nd == N && nb == NB) {                                                                                            \
        static bool attr_set = false;                                                                                     \
        if (!attr_set) { (void)hipFuncSetAttribute((const void*)frames_ring_kernel<N, NB>, hipFuncAttributeMaxDynamicSharedMemorySize, 163840); attr_set = true; } \
        hipLaunchKernelGGL((frames_ring_kernel<N, NB>), dim3(grid), dim3(block), lds, stream, x, out, p->d_ring_win, p->d_ring_align_pos, \
                           p->d_ref, p->d_ref64, p->d_ring_items, ra);                                                     \
        launched = true;                                                                                                  \
    }
        bool launched = false;
        LAUNCH_RING(1, 8) LAUNCH_RING(1, 4) LAUNCH_RING(1, 2) LAUNCH_RING(1, 1)
        LAUNCH_RING(2, 4) LAUNCH_RING(2, 2) LAUNCH_RING(2, 1) LAUNCH_RING(3, 2) LAUNCH_RING(3, 1) LAUNCH_RING(4, 2) LAUNCH_RING(4, 1)
        LAUNCH_RING(6, 1) LAUNCH_RING(8, 1) LAUNCH_RING(10, 1) LAUNCH_RING(12, 1) LAUNCH_RING(14, 1) LAUNCH_RING(16, 1)
        LAUNCH_RING(18, 1) LAUNCH_RING(20, 1) LAUNCH_RING(22, 1) LAUNCH_RING(24, 1) LAUNCH_RING(26, 1) LAUNCH_RING(28, 1) LAUNCH_RING(30, 1) LAUNCH_RING(32, 1)
        if (!launched) return MOLANN_E_UNSUPPORTED;
#undef LAUNCH_RING
        if (nb == 1)
            snprintf(p->last_info, sizeof(p->last_info), "frames_ring_kernel<ND=%d> (%d consumer + %d loader waves, ring of %d frames, %d windows) grid=%d block=%d lds=%zu",
                     nd, ra.n_cons, ra.n_load, ra.n_slot, p->ring_nwin, grid, block, lds);
        else
            snprintf(p->last_info, sizeof(p->last_info), "frames_ring_kernel<ND=%d,B=%d> (%d consumer + %d loader waves, ring of %d entries of %d frames, %d windows) grid=%d block=%d lds=%zu",
                     nd, nb, ra.n_cons, ra.n_load, ra.n_slot, nb, p->ring_nwin, grid, block, lds);
    } else if (mode == 1 && getenv("MOLANN_NO_RING") == nullptr && p->n_inp <= 384 && getenv("MOLANN_NO_ALIGN_BATCH") == nullptr) {
        // AlignmentLayer.forward on mid-size frames: rounds of B >= 4 consecutive frames, one rotation solve per round
        // (frames_align_batch_kernel).  Measured, 1 M frames: 60 atoms 1.64 -> 0.33 ms, 166 atoms 1.86 -> 0.97 ms (4.3 TB/s), 320 atoms
        // 2.09 -> 1.73; from ~400 atoms on a frame per round (below) is as fast or faster (700 atoms: 5.0 against 4.3 TB/s with B = 2).
        AlignRegsArgs ra;
        memset(&ra, 0, sizeof(ra));
        ra.n_frames = n_frames; ra.n_inp = p->n_inp; ra.n_align = p->n_align;
        ra.first_align = p->align_first;
        { const char* e = diag_env("MOLANN_DEBUG_ALIGN_FLAGS"); ra.flags = e ? atoi(e) : 0; }
        int nb = 16;
        while (nb > 4 && nb * p->n_inp > 1536) nb /= 2;
        const int per_lane = (nb * p->n_inp + 63) / 64;
        const int units = per_lane <= 8 ? 2 : (per_lane <= 16 ? 4 : 6);
        const void* fn = nullptr;
#define ALIGN_BATCH_CASE(UU, BB) if (units == UU && nb == BB) fn = (const void*)frames_align_batch_kernel<UU, BB>;
        ALIGN_BATCH_CASE(2, 16) ALIGN_BATCH_CASE(4, 16) ALIGN_BATCH_CASE(6, 16) ALIGN_BATCH_CASE(4, 8) ALIGN_BATCH_CASE(6, 8)
        ALIGN_BATCH_CASE(4, 4) ALIGN_BATCH_CASE(6, 4)
#undef ALIGN_BATCH_CASE
        if (!fn) return MOLANN_E_UNSUPPORTED;
        int occ = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, 128, 0) != hipSuccess || occ < 1) occ = 1;
        if (debug_env().wave_bpc > 0) occ = std::min(occ, debug_env().wave_bpc);
        const long n_rounds = (n_frames + nb - 1) / nb;
        const int grid = (int)std::min<long>(n_rounds, (long)p->num_cus * occ);
        void* kargs[] = {(void*)&x, (void*)&out, (void*)&p->d_align_idx, (void*)&p->d_ref, (void*)&p->d_ref64, (void*)&ra};
        const hipError_t le = hipLaunchKernel(fn, dim3(grid), dim3(128), kargs, 0, stream);
        snprintf(p->last_info, sizeof(p->last_info), "frames_align_batch_kernel<U=%d,B=%d> (rounds of %d frames: a data wave + a solver wave of %d-lane groups, %d blocks per CU) grid=%d block=128",
                 units, nb, nb, 64 / nb, occ, grid);
        if (le != hipSuccess) return (int)le;
    } else if (mode == 1 && getenv("MOLANN_NO_RING") == nullptr && p->n_inp <= 24 * 512) {
        // AlignmentLayer.forward on large frames: the frame held in the registers of a block of W waves (molann_align_regs.inc)
        AlignRegsArgs ra;
        memset(&ra, 0, sizeof(ra));
        ra.n_frames = n_frames; ra.n_inp = p->n_inp; ra.n_align = p->n_align;
        ra.first_align = p->align_first;
        { const char* e = diag_env("MOLANN_DEBUG_ALIGN_FLAGS"); ra.flags = e ? atoi(e) : 0; }
        int W = 1;
        while ((p->n_inp + 64 * W - 1) / (64 * W) > 24) W *= 2;
        const int units = ((p->n_inp + 64 * W - 1) / (64 * W) + 3) / 4;       // atoms per thread, in fours
        const void* fn = nullptr;
#define ALIGN_REGS_CASE(WW, U) if (W == WW && units == U) fn = (const void*)frames_align_regs_kernel<WW, U>;
        ALIGN_REGS_CASE(1, 1) ALIGN_REGS_CASE(1, 2) ALIGN_REGS_CASE(1, 3) ALIGN_REGS_CASE(1, 4) ALIGN_REGS_CASE(1, 5) ALIGN_REGS_CASE(1, 6)
        ALIGN_REGS_CASE(2, 4) ALIGN_REGS_CASE(2, 5) ALIGN_REGS_CASE(2, 6) ALIGN_REGS_CASE(4, 4) ALIGN_REGS_CASE(4, 5) ALIGN_REGS_CASE(4, 6)
        ALIGN_REGS_CASE(8, 4) ALIGN_REGS_CASE(8, 5) ALIGN_REGS_CASE(8, 6)
#undef ALIGN_REGS_CASE
        if (!fn) return MOLANN_E_UNSUPPORTED;
        int occ = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, 64 * (W + 1), 0) != hipSuccess || occ < 1) occ = 1;
        // frames in flight per CU: two blocks of the 5000-atom class (measured, A4: 7.9 / 6.4 / 7.4 ms per 262 144 frames at 1 / 2 / 3
        // blocks per CU), more of the smaller ones: about 120 KB of frames per CU
        occ = std::min(occ, std::max(2, (int)(122880 / (12l * p->n_inp))));
        if (debug_env().wave_bpc > 0) occ = std::min(occ, debug_env().wave_bpc);
        const int grid = (int)std::min<long>(n_frames, (long)p->num_cus * occ);
        void* kargs[] = {(void*)&x, (void*)&out, (void*)&p->d_align_idx, (void*)&p->d_ref, (void*)&p->d_ref64, (void*)&ra};
        const hipError_t le = hipLaunchKernel(fn, dim3(grid), dim3(64 * (W + 1)), kargs, 0, stream);
        snprintf(p->last_info, sizeof(p->last_info), "frames_align_regs_kernel<W=%d,U=%d> (%d data waves + 1 solver per frame, %d atoms per thread, %d blocks per CU) grid=%d block=%d",
                 W, units, W, 4 * units, occ, grid, 64 * (W + 1));
        if (le != hipSuccess) return (int)le;
    } else {
        const int wpb = 4;
        // blocks per CU: all wave slots.  (The gather is HBM-latency bound and wants every wave it can get; the MLP
        // kernel on the plan's side stream takes the CUs it needs as gather blocks retire.  Measured, 262144
        // frames: C5 5.8e7 / 6.8e7 / 7.3e7 frames/s at 2 / 4 / 8 blocks per CU.  MOLANN_WAVE_BPC to experiment.)
        int bpc = 8;
        if (debug_env().wave_bpc > 0) bpc = debug_env().wave_bpc;
        const int grid = grid_for(p, n_frames, wpb, bpc);
        // item rounds (64 items each) whose atoms are loaded with the alignment atoms.  Measured (PMC, C5, 256 items):
        // 4 rounds: 519 TCC misses/frame, 279 us per 21 845 frames; two-phase: 603 misses/frame, 291 us.  With one
        // round or less (C4) the extra registers cost more occupancy than the shared lines save: two-phase.
        int pre = (mode == 1 || p->n_items <= 64) ? 0 : (p->n_items <= 128 ? 2 : 4);
        if (debug_env().wave_pre >= 0) pre = debug_env().wave_pre;
#define LAUNCH_WAVE(P)                                                                                                    \
    hipLaunchKernelGGL(frames_wave_kernel<P>, dim3(grid), dim3(64 * wpb), 0, stream, x, out, p->d_align_idx, p->d_ref, \
                       p->d_ref64, p->d_items, a)
        if (pre >= 4) LAUNCH_WAVE(4);
        else if (pre >= 2) LAUNCH_WAVE(2);
        else if (pre == 1) LAUNCH_WAVE(1);
        else LAUNCH_WAVE(0);
#undef LAUNCH_WAVE
        snprintf(p->last_info, sizeof(p->last_info), "frames_wave_kernel<pre=%d> grid=%d block=%d mode=%d", pre >= 4 ? 4 : (pre >= 2 ? 2 : pre),
                 grid, 64 * wpb, mode);
    }
    return (int)hipGetLastError();
}

// the whole forward of a plan with a wide MLP in one launch of the WIDE_MLP build of the lane kernel
int launch_wide(molann_plan* p, const float* x, long n_frames, float* out, hipStream_t stream) {
    const long n_tiles = (n_frames + 63) / 64;
    const int grid = grid_for(p, n_tiles, 1, p->wide_bpc);
    struct { const float* x; float* out; const double* ref64; const float* wfrag; long n; int out_vec4, pad_;
             unsigned long long* stamps; const float* ref32; float* feat; } ka =
        {x, out, p->d_ref64, (const float*)p->d_wchain, n_frames, 0, 0, nullptr, p->d_ref, (float*)(p->d_wchain + p->chain_stream_bytes)};
    size_t ksz = sizeof(ka);
    void* cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &ka, HIP_LAUNCH_PARAM_BUFFER_SIZE, &ksz, HIP_LAUNCH_PARAM_END};
    const int block = 64 * (p->wide_ncons + p->wide_nload);
    const hipError_t le = hipModuleLaunchKernel(p->wide_fn, grid, 1, 1, block, 1, 1, 0, stream, nullptr, cfg);
    snprintf(p->last_info, sizeof(p->last_info), "molann_lane_jit<NL=%d,wide> (plan-specialised; %d consumer waves + %d loader, ring of %d tiles, %ld KB of weights resident) grid=%d block=%d lds=%d",
             p->n_layers, p->wide_ncons, p->wide_nload, p->wide_nslot, p->chain_stream_bytes / 1024, grid, block, p->wide_lds_block);
    return (int)le;
}

int launch_mlp(molann_plan* p, const float* feat, long n_frames, int in_stride, float* out, hipStream_t stream) {
    if (p->lane_mlp) { // a small head: a wave per 64-frame tile, the fused MLP's stage on rows read from memory (mlp_lane_kernel)
        PreArgs a;
        memset(&a, 0, sizeof(a));
        a.n_frames = n_frames; a.n_layers = p->n_layers; a.act = p->act; a.out_cols = p->out_dim;
        for (int i = 0; i <= p->n_layers; ++i) a.dims[i] = p->dims[i];
        a.out_vec4 = (p->out_dim % 4 == 0) && (((uintptr_t)out & 15) == 0);
        a.lds_per_wave = ceil_to(((p->dims[0] + 3) & ~3) * FB_STRIDE * 4, 16);
        const int wpb = 4;
        const long n_tiles = (n_frames + 63) / 64;
        const int grid = grid_for(p, n_tiles, wpb, 4);
        const size_t lds = (size_t)wpb * a.lds_per_wave;
        snprintf(p->mlp_info, sizeof(p->mlp_info), "mlp_lane_kernel<NL=%d> grid=%d block=%d lds=%zu", p->n_layers, grid, 64 * wpb, lds);
#define LAUNCH_MLP_LANE(N) hipLaunchKernelGGL((mlp_lane_kernel<N>), dim3(grid), dim3(64 * wpb), lds, stream, feat, out, p->d_wlane, in_stride, a)
        switch (p->n_layers) {
        case 1: LAUNCH_MLP_LANE(1); break;
        case 2: LAUNCH_MLP_LANE(2); break;
        case 3: LAUNCH_MLP_LANE(3); break;
        default: LAUNCH_MLP_LANE(4); break;
        }
#undef LAUNCH_MLP_LANE
        return (int)hipGetLastError();
    }
    if (p->chain_fn) { // plan-specialised chain kernel: one 4-wave block per CU, 64*FB frames per block and tile
        const int cw = p->chain_waves > 0 ? p->chain_waves : 4;
        const long tile = 16l * cw * p->chain_fb, n_tiles = (n_frames + tile - 1) / tile;
        const int grid = (int)std::min<long>(n_tiles, p->num_cus);
        struct { const float* feat; float* out; const unsigned char* w; const float* b; long n; int in_stride; } ka =
            {feat, out, p->d_wchain, (const float*)(p->d_wchain + p->chain_stream_bytes), n_frames, in_stride};
        size_t ksz = sizeof(ka);
        void* cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &ka, HIP_LAUNCH_PARAM_BUFFER_SIZE, &ksz, HIP_LAUNCH_PARAM_END};
        char ring[24] = "";
        if (cw != 8) snprintf(ring, sizeof(ring), "; %d slab buffers", p->chain_nslab);
        snprintf(p->mlp_info, sizeof(p->mlp_info), "molann_mlp_chain<%s,FB=%d%s> (plan-specialised%s) grid=%d block=%d",
                 p->mlp_prec == MOLANN_MLP_BF16 ? "bf16" : "f32", p->chain_fb, cw == 8 ? ",resident" : "", ring, grid, 64 * cw);
        return (int)hipModuleLaunchKernel(p->chain_fn, grid, 1, 1, 64 * cw, 1, 1, 0, stream, nullptr, cfg);
    }
    MlpArgs a;
    memset(&a, 0, sizeof(a));
    a.n_frames = n_frames;
    a.n_layers = p->n_layers;
    a.act = p->act;
    for (int i = 0; i <= p->n_layers; ++i) a.dims[i] = p->dims[i];
    for (int i = 0; i < p->n_layers; ++i) { a.kp[i] = p->kp[i]; a.jp[i] = p->jp[i]; a.woff[i] = p->moff[i]; }
    a.ld[0] = p->mlp_ld[0];
    a.ld[1] = p->mlp_ld[1];
    a.lds_per_wave = p->mlp_lds_per_wave;
    a.in_stride = in_stride;
    // block size that packs most waves into the CU's LDS (waves are independent), larger block on ties
    int wpb = 1, best_waves = 0;
    for (int w = 4; w >= 1; --w) {
        if ((long)w * p->mlp_lds_per_wave > 65536 && w > 1) continue;
        long waves = w * (163840 / ((long)w * p->mlp_lds_per_wave));
        if (waves > 16) waves = 16;
        if (waves > best_waves) { best_waves = (int)waves; wpb = w; }
    }
    int bpc = (int)(163840 / ((long)wpb * p->mlp_lds_per_wave));
    if (bpc < 1) bpc = 1;
    if (bpc * wpb > 16) bpc = std::max(1, 16 / wpb);
    const long n_blocks = (n_frames + 15) / 16;
    const int grid = grid_for(p, n_blocks, wpb, bpc);
    const size_t lds = (size_t)wpb * p->mlp_lds_per_wave;
    snprintf(p->mlp_info, sizeof(p->mlp_info), "mlp_mfma_kernel<%s> grid=%d block=%d lds=%zu", p->mlp_prec == MOLANN_MLP_BF16 ? "bf16" : "f32",
             grid, 64 * wpb, lds);
    if (p->mlp_prec == MOLANN_MLP_BF16)
        hipLaunchKernelGGL((mlp_mfma_kernel<true>), dim3(grid), dim3(64 * wpb), lds, stream, feat, out, p->d_wmfma, a);
    else
        hipLaunchKernelGGL((mlp_mfma_kernel<false>), dim3(grid), dim3(64 * wpb), lds, stream, feat, out, p->d_wmfma, a);
    return (int)hipGetLastError();
}

} // namespace
