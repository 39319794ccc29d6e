// molann_bwd_ring.inc - the whole backward of a lane-per-frame plan in ONE pass over x, specialised for one plan
// (hipRTC, gfx950; compiled behind the preamble + molann_ring.inc + molann_mlp_tile.inc).
//
// The reference gets its gradients from torch autograd through ~60 ATen ops per forward, including the backward of a
// batched LAPACK SVD (ann.py:188) and the Linear / activation nodes of ann_layers (ann.py:60-65, 620-624).  Here:
//
//   loader waves      the touched 16-byte windows of x -> ring of tile slots in LDS (the forward kernel's loader)
//   consumer waves    one lane per frame, 64 frames per tile:
//     recompute       Kabsch, aligned atoms, feature table                         (per lane, molann_math.h)
//     MLP             forward of the hidden layers, input gradients, dW / db       (fp32 matrix cores:
//                     through a [unit][frame] scratch in the consumer's LDS buffer  molann_mlp_tile.inc)
//     reverse mode    feature table, rotation apply, closed-form Kabsch backward, centring   (per lane)
//     grad_x tile     zeros + the touched atoms' gradients in the same LDS buffer -> coalesced 16-byte stores
//
// Nothing is saved from the forward and nothing but x, grad_out and grad_x crosses HBM: the arithmetic of a tile runs
// while the loaders stream the next ones.  dW / db stay in registers over all of a consumer's tiles and leave as one
// row of partial sums per block (reduce_rows_kernel adds the rows).  Plans whose register need does not fit (the
// compiler reports scratch) keep the two-kernel path (molann_mlp_bwd.inc + molann_lane_bwd.inc).
//
// Preamble: that of molann_lane_jit.inc - here FB_OFF / FB_BYTES name the consumers' buffers (max of the dense
// gradient tile, the MLP scratch and the parameter sums) - plus KP / JP / WOFF / GOFF / N_PARAMS of molann_mlp_bwd.inc.

static_assert(N_ROWS * SSTR * 4 <= FB_BYTES && TILE_BYTES <= FB_BYTES && N_PARAMS * 4 <= FB_BYTES, "consumer buffer");
static_assert(!FRAG_LDS || IMG_OFF + FRAG.count * 256 <= LDS_BLOCK, "fragment image");

extern "C" __global__ __launch_bounds__(64 * (NCONS + NLOAD), 1) void molann_bwd_ring(const float* __restrict__ x, const float* __restrict__ gout,
                                                                                     const double* __restrict__ ref64_g, const float* __restrict__ ref32_g,
                                                                                     const float* __restrict__ wnat, float* __restrict__ gx,
                                                                                     float* __restrict__ gparams /* [gridDim.x][N_PARAMS] partial sums */,
                                                                                     long n_frames, float* __restrict__ yout /* WITH_VALUES builds: the forward's [N, OUTC] */) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[LDS_BLOCK];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    lds_word_t ready = (lds_word_t)(smem);            // [NSLOT]
    lds_word_t done = (lds_word_t)(smem + 64);        // [NSLOT]
    lds_word_t next = (lds_word_t)(smem + 128);       // next tile of the block nobody has taken yet
    lds_word_t fin = (lds_word_t)(smem + 132);        // consumers that have written their parameter sums
    unsigned char* const ring = smem + RING_OFF;

    const long n_tiles = (n_frames + 63) >> 6;
    const BlockTiles bt = block_tiles(n_tiles, (long)blockIdx.x, (long)gridDim.x);     // tiles interleaved over the blocks (molann_ring.inc)
    const int n_b = bt.n_b;

    if (threadIdx.x < 2 * 16 + 2) ((volatile int*)smem)[threadIdx.x] = 0;   // ready[16], done[16], next, fin
    __syncthreads();

    if (wave >= NCONS) {
        ring_loader(x, n_frames, bt, ring, ready, done, wave - NCONS, lane, nullptr);
        return;
    }

    // =============================== consumers =======================================================
    float* const S = (float*)(smem + FB_OFF + (size_t)wave * FB_BYTES);   // MLP scratch, then the gradient tile
    const auto ref64 = (const __attribute__((address_space(4))) double*)ref64_g; // wave-uniform: scalar loads
    const auto ref32 = (const __attribute__((address_space(4))) float*)ref32_g;
    const bool want_gx = gx != nullptr, want_gp = gparams != nullptr && NL > 0;
    constexpr int OUTC = NL > 0 ? DIMS[NL] : D_FEAT;

    // ---- operand fragments of the weights and the parameter sums, once per wave (molann_mlp_tile.inc) ------------
    float* const img = (float*)(smem + IMG_OFF);
    MlpTileState mlp;
    if constexpr (NL > 0) mlp_tile_init(mlp, wnat, img, lane);
    // The whole buffer starts as zeros.  The MLP phase never writes anything but zeros to the rows K .. pad4(K) of a scratch
    // region (the padding its k-steps read), and the gradient tile takes its own entries back (7.), so both views of the
    // buffer find the zeros they rely on.
    for (int i = lane; i < FB_BYTES / 16; i += 64) ((f32x4*)S)[i] = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (;;) {
        int n = 0;
        if (lane == 0) n = __hip_atomic_fetch_add((__attribute__((address_space(3))) int*)next, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        n = __builtin_amdgcn_readfirstlane(n);
        if (n >= n_b) break;
        const long t = ring_tile(bt, n);
        const long rem = n_frames - t * 64;
        const int nfr = rem < 64 ? (int)rem : 64;
        const bool live = lane < nfr;              // lanes past the end recompute the last frame and contribute nothing
        const int fl = live ? lane : nfr - 1;
        const int s = n % NSLOT, gen = n / NSLOT;
        const unsigned char* slot = ring + (size_t)s * TILE_STRIDE;
        // ---- 0. this frame's grad_out row: asked for before the wait for the tile -----------------------------
        float gv[OUTC];
        {
            const float* grow = gout + (t * 64 + fl) * (long)OUTC;
#pragma unroll
            for (int c = 0; c < OUTC; ++c) gv[c] = grow[c];
        }
        // ---- 1. the tile's windows -> registers, slot handed back ------------------------------------------------
        lds_wait_ge(ready + s, gen + 1);
        const f32x4* fr = (const f32x4*)slot + fl * NWIN;
        f32x4 wv[NWIN];
#pragma unroll
        for (int k = 0; k < NWIN; ++k) wv[k] = fr[k];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the reads have RETURNED before the loader may overwrite the slot
#pragma unroll
        for (int k = 0; k < NWIN; ++k) asm volatile("" : "+v"(wv[k]));
        done[s] = gen + 1;
        V3 a[N_SLOTS];
#pragma unroll
        for (int u = 0; u < N_SLOTS; ++u) {
            const int d0 = 3 * SLOT_ATOM[u];
            a[u] = v3(wv[win_of(d0)][d0 - WIN_START[win_of(d0)]], wv[win_of(d0 + 1)][d0 + 1 - WIN_START[win_of(d0 + 1)]],
                      wv[win_of(d0 + 2)][d0 + 2 - WIN_START[win_of(d0 + 2)]]);
        }

        // ---- 2. forward recompute: Kabsch (ann.py:179-195), aligned atoms, feature table (ann.py:323-354) -------
        float R[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
        KT h[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // in the forward kernel's precision (float for plans that do not see the rotation's accuracy)
        V3 c0 = v3(0.f, 0.f, 0.f), dl = v3(0.f, 0.f, 0.f);
        V3 y[N_SLOTS];
        if constexpr (N_ALIGN > 0) {
            KT e0;
            covariance<KT>(a, KabschReal<KABSCH_F32>::pick(ref32, ref64), c0, dl, h, e0);
            kabsch_rotation_t<KT>(h, e0, R);
#pragma unroll
            for (int u = 0; u < N_SLOTS; ++u) y[u] = rotate((a[u] - c0) - dl, R);
        } else {
#pragma unroll
            for (int u = 0; u < N_SLOTS; ++u) y[u] = a[u];
        }
        // the backward's atoms of the bond / angle / dihedral items: the rotated differences of the INPUT atoms (align_item_atoms), which
        // do not carry the rounding of an aligned atom's distance to the centroid; kept over the MLP, where the raw atoms do not stay
        V3 yd[N_ITEMS > 0 ? N_ITEMS : 1][3];
        if constexpr (N_ALIGN > 0) {
#pragma unroll
            for (int it = 0; it < N_ITEMS; ++it) {
                if (ITEM_TYPE[it] != IT_POSITION) {
                    V3 q0 = a[ITEM_IDX[it][0]], q1 = a[ITEM_IDX[it][1]], q2 = a[ITEM_IDX[it][2]], q3 = a[ITEM_IDX[it][3]];
                    align_item_atoms(ITEM_TYPE[it], q0, q1, q2, q3, c0, dl, R);
                    yd[it][0] = q0; yd[it][1] = q2; yd[it][2] = q3;
                }
            }
        }
        float f[D_FEAT > 0 ? D_FEAT : 1];
#pragma unroll
        for (int it = 0; it < N_ITEMS; ++it) {
            float v[3];
            const int w = eval_item(ITEM_TYPE[it], y[ITEM_IDX[it][0]], y[ITEM_IDX[it][1]], y[ITEM_IDX[it][2]], y[ITEM_IDX[it][3]], v);
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if (j < w) f[ITEM_COL[it] + j] = v[j];
        }

        // ---- 3. the MLP on the matrix cores: dL/d features, dW, db -------------------------------------------------
        float gf[D_FEAT > 0 ? D_FEAT : 1];
        if constexpr (NL == 0) {
#pragma unroll
            for (int k = 0; k < D_FEAT; ++k) gf[k] = live ? gv[k] : 0.f;
            if constexpr (WITH_VALUES) {
                if (yout && live) {
#pragma unroll
                    for (int k = 0; k < D_FEAT; ++k) yout[(t * 64 + lane) * (long)D_FEAT + k] = f[k];
                }
            }
        } else {
float gm[OUTC];
#pragma unroll
            for (int c = 0; c < OUTC; ++c) gm[c] = live ? gv[c] : 0.f;
            mlp_tile_backward(mlp, S, img, lane, f, gm, want_gp, want_gx, wnat, (WITH_VALUES && yout) ? yout + t * 64 * (long)OUTC : nullptr, nfr);
#pragma unroll
            for (int k = 0; k < D_FEAT; ++k) gf[k] = S[(GF_ROW + k) * SSTR + lane]; // (unused without grad_x)
        }

        if (want_gx) {
            // ---- 4. feature table backward: dL / d aligned atoms --------------------------------------
            V3 gy[N_SLOTS];
#pragma unroll
            for (int u = 0; u < N_SLOTS; ++u) gy[u] = v3(0.f, 0.f, 0.f);
#pragma unroll
            for (int it = 0; it < N_ITEMS; ++it) {
                float g3[3] = {0.f, 0.f, 0.f};
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    if (j < item_width(ITEM_TYPE[it])) g3[j] = gf[ITEM_COL[it] + j];
                V3 q0 = y[ITEM_IDX[it][0]], q1 = y[ITEM_IDX[it][1]], q2 = y[ITEM_IDX[it][2]], q3 = y[ITEM_IDX[it][3]];
                if constexpr (N_ALIGN > 0) {
                    if (ITEM_TYPE[it] != IT_POSITION) { q0 = yd[it][0]; q1 = v3(0.f, 0.f, 0.f); q2 = yd[it][1]; q3 = yd[it][2]; }
                }
                eval_item_backward(ITEM_TYPE[it], q0, q1, q2, q3, g3,
                                   gy[ITEM_IDX[it][0]], gy[ITEM_IDX[it][1]], gy[ITEM_IDX[it][2]], gy[ITEM_IDX[it][3]]);
            }
            // ---- 5. rotation apply, Kabsch and centring backward: dL / d raw atoms -----------------------
            V3 ga[N_SLOTS];
            if constexpr (N_ALIGN > 0) {
                float GR[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, GH[9];
#pragma unroll
                for (int u = 0; u < N_SLOTS; ++u) {
                    if (SLOT_USED[u]) { // y_u = p_u R :  G_R += p_u^T g_y ,  g_p = g_y R^T
                        const V3 g = gy[u];
                        // p_u = y_u R^T (R is a rotation): the raw atoms need not stay in registers over the MLP
                        const V3 yu = y[u];
                        const V3 pu = v3(fmaf(yu.z, R[2], fmaf(yu.y, R[1], yu.x * R[0])), fmaf(yu.z, R[5], fmaf(yu.y, R[4], yu.x * R[3])),
                                         fmaf(yu.z, R[8], fmaf(yu.y, R[7], yu.x * R[6])));
                        GR[0] = fmaf(pu.x, g.x, GR[0]); GR[1] = fmaf(pu.x, g.y, GR[1]); GR[2] = fmaf(pu.x, g.z, GR[2]);
                        GR[3] = fmaf(pu.y, g.x, GR[3]); GR[4] = fmaf(pu.y, g.y, GR[4]); GR[5] = fmaf(pu.y, g.z, GR[5]);
                        GR[6] = fmaf(pu.z, g.x, GR[6]); GR[7] = fmaf(pu.z, g.y, GR[7]); GR[8] = fmaf(pu.z, g.z, GR[8]);
                        ga[u] = v3(fmaf(g.z, R[2], fmaf(g.y, R[1], g.x * R[0])), fmaf(g.z, R[5], fmaf(g.y, R[4], g.x * R[3])),
                                   fmaf(g.z, R[8], fmaf(g.y, R[7], g.x * R[6])));
                    } else {
                        ga[u] = v3(0.f, 0.f, 0.f);
                    }
                }
                kabsch_rotation_backward_t<KT>(h, R, GR, GH);
                V3 gc = v3(0.f, 0.f, 0.f);
#pragma unroll
                for (int u = 0; u < N_SLOTS; ++u) {
                    if (u < N_ALIGN) { // H = sum_i p_i ref_i^T :  g_p[i] += G_H ref_i
                        const float rx = ref32[3 * u], ry = ref32[3 * u + 1], rz = ref32[3 * u + 2];
                        ga[u] = ga[u] + v3(fmaf(GH[2], rz, fmaf(GH[1], ry, GH[0] * rx)), fmaf(GH[5], rz, fmaf(GH[4], ry, GH[3] * rx)),
                                           fmaf(GH[8], rz, fmaf(GH[7], ry, GH[6] * rx)));
                    }
                    gc = gc + ga[u]; // p_u = a_u - centroid:  g_centroid = - sum_u g_p[u]
                }
                constexpr float inv_a = 1.0f / (N_ALIGN > 0 ? (float)N_ALIGN : 1.0f);
#pragma unroll
                for (int u = 0; u < N_ALIGN; ++u) ga[u] = ga[u] - inv_a * gc; // centroid = mean of the align atoms
            } else {
#pragma unroll
                for (int u = 0; u < N_SLOTS; ++u) ga[u] = gy[u];
            }
            // ---- 6. grad_x tile in the buffer: zeros where the MLP scratch was, the touched atoms' gradients ----------
            __builtin_amdgcn_wave_barrier();
            if constexpr (NL > 0) {
                constexpr int used16 = (N_ROWS * SSTR * 4 + 15) / 16 < TILE_BYTES / 16 ? (N_ROWS * SSTR * 4 + 15) / 16 : TILE_BYTES / 16;
                for (int c = lane; c < used16; c += 64) ((f32x4*)S)[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
            if (live) {
                float* row = S + lane * FRAME_DW;
#pragma unroll
                for (int u = 0; u < N_SLOTS; ++u) { row[3 * SLOT_ATOM[u]] = ga[u].x; row[3 * SLOT_ATOM[u] + 1] = ga[u].y; row[3 * SLOT_ATOM[u] + 2] = ga[u].z; }
            }
            __builtin_amdgcn_wave_barrier();
            // ---- 7. coalesced store; the touched positions go back to zero behind it ---------------------------------
            float* gdst = gx + t * 64 * (long)FRAME_DW;
            const int ndw = nfr * FRAME_DW;
            if ((((size_t)gx) & 15) == 0) {
                const int nchunk = ndw >> 2;
                for (int c = lane; c < nchunk; c += 64) ((f32x4*)gdst)[c] = ((const f32x4*)S)[c];
                for (int c = (nchunk << 2) + lane; c < ndw; c += 64) gdst[c] = S[c];
            } else {
                for (int c = lane; c < ndw; c += 64) gdst[c] = S[c];
            }
            __builtin_amdgcn_wave_barrier();
            if (live) {
                float* row = S + lane * FRAME_DW;
#pragma unroll
                for (int u = 0; u < N_SLOTS; ++u) { row[3 * SLOT_ATOM[u]] = 0.f; row[3 * SLOT_ATOM[u] + 1] = 0.f; row[3 * SLOT_ATOM[u] + 2] = 0.f; }
            }
        }
        __builtin_amdgcn_wave_barrier();
    }

    if constexpr (NL > 0) {
        if (want_gp) {
            // ---- the block's sums: every consumer's accumulators -> its buffer in gradient-buffer order; the last one to
            // arrive adds them and stores the block's row
            __builtin_amdgcn_wave_barrier();
mlp_tile_store_sums(mlp, S, lane);
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the sums are in LDS before this consumer counts itself in
            int arrived = 0;
            if (lane == 0) arrived = __hip_atomic_fetch_add((__attribute__((address_space(3))) int*)fin, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_WORKGROUP);
            arrived = __builtin_amdgcn_readfirstlane(arrived);
            if (arrived == NCONS - 1) {
                float* row = gparams + (long)blockIdx.x * N_PARAMS;
                for (int i = lane; i < N_PARAMS; i += 64) {
                    float sum = 0.f;
#pragma unroll
                    for (int w = 0; w < NCONS; ++w) sum += ((const float*)(smem + FB_OFF + (size_t)w * FB_BYTES))[i];
                    row[i] = sum;
                }
            }
        }
    }
}
