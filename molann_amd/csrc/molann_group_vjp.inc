// molann_group_vjp.inc - the forward's outputs AND dL/dx for a known cotangent in ONE launch, for plans whose frames are too
// large for the lane-per-frame kernels (mid-size and large frames), specialised for one plan (hipRTC, gfx950; compiled behind
// the preamble of molann_mlp_bwd.inc + molann_mlp_tile.inc).  What molann_value_and_vjp_f32 launches for these plans in place of
// forward_train + mlp_backward (x only) + features_backward.
//
// One block owns a 64-frame tile, processed as 64 / B rounds of B consecutive frames with GL = 64 / B lanes per frame (the
// scheme of frames_group_bwd_kernel<B>); the block's waves take the rounds in turn, so a small batch runs on as many waves as
// it has rounds.  LDS is laid out for WPB waves; the launch may use fewer (blockDim: the host picks half of them for batches with
// more tiles than CUs, where two blocks per CU hide each other's head phase).  The plan's tables (packed reference, alignment
// atoms, items, touched-atom lists) go to LDS once per block.
//
//   A  forward      per round: centroid, covariance butterfly inside the group, fp64 Kabsch solve, the items' features into the
//                   block's [unit][frame] scratch S.  R, H, c0 and dl of every frame stay in LDS for C (no second solve).
//   B  head         wave 0: each lane takes its frame's feature row through mlp_tile_backward (x-only mode, WITH_VALUES):
//                   y -> out, dL/df -> S rows GF_ROW ...  Features-only plans (NL == 0) store y = f and put the cotangent in S in A.
//   C  backward     per round: item backward into the frame's g_y buffer, G_R, kabsch_rotation_backward, the centroid term
//                   inv_a * sum g_p on the centred reference, then every touched atom gathers its own contributions, rotates
//                   them back, adds its alignment rows and stores its three floats behind the round's zero-filled rows.
//
// Touched-atom lists (molann_plan_create: group_vjp_tables): per atom, entries e >= 0 name the g_y slot 4 it + j of an item atom,
// entries e < 0 the alignment row -1 - e (an atom named twice in the alignment set has two rows).
// Frames past the end of the batch recompute the last frame with a zero cotangent and store nothing; rounds wholly past the end
// are skipped.  Parameters are data here (no parameter gradients, no workspace): the launch only enqueues work.
//
// Preamble: NL, ACT, DIMS, KP / JP / WOFF / GOFF / N_PARAMS, FRAG_LDS, WITH_VALUES (molann_mlp_bwd.inc's), and B, WPB, N_ALIGN,
// N_ITEMS, D_FEAT, FRAME_DW, N_TOUCHED, N_LIST, S_ROWS, the byte offsets OFF_* and LDS_BYTES (host: group_vjp_geometry).

constexpr int GL = 64 / B;
constexpr int OUTC = NL > 0 ? DIMS[NL] : D_FEAT;
constexpr int GY_FRAME = 12 * N_ITEMS;     // floats of one frame's g_y buffer: [item][atom of item][xyz]
struct FrameState { double h[9]; float R[9], c0[3], dl[3], pad; };
static_assert(B == 2 || B == 4 || B == 8, "frames per round");
static_assert(sizeof(FrameState) == FRAME_STATE_BYTES, "frame state");
static_assert(S_ROWS >= N_ROWS && S_ROWS >= D_FEAT && OFF_ST - OFF_S >= S_ROWS * SSTR * 4, "scratch rows");
static_assert(OFF_GY - OFF_ST >= 64 * FRAME_STATE_BYTES && LDS_BYTES - OFF_GY >= WPB * B * GY_FRAME * 4, "per-frame buffers");
static_assert(!FRAG_LDS || OFF_S - OFF_IMG >= FRAG.count * 256, "fragment image");

__device__ __forceinline__ V3 load_atom(const float* __restrict__ xf, int k) { return v3(xf[3 * k], xf[3 * k + 1], xf[3 * k + 2]); }
__device__ __forceinline__ V3 rotate_back(V3 g, const float (&R)[9]) {   // g R^T
    return v3(fmaf(g.z, R[2], fmaf(g.y, R[1], g.x * R[0])), fmaf(g.z, R[5], fmaf(g.y, R[4], g.x * R[3])), fmaf(g.z, R[8], fmaf(g.y, R[7], g.x * R[6])));
}
__device__ __forceinline__ float group_sum_f(float v) {
    v += dpp_mov<0xB1>(v); v += dpp_mov<0x4E>(v); v += dpp_mov<0x141>(v);
    if constexpr (GL >= 16) v += dpp_mov<0x140>(v);
    if constexpr (GL >= 32) v += __shfl_xor(v, 16, 64);
    return v;
}
__device__ __forceinline__ double group_sum_d(double v) {
    auto step = [](double x_, auto mover) {
        const long long bb = __builtin_bit_cast(long long, x_);
        const int lo = mover((int)(bb & 0xffffffffll)), hi = mover((int)(bb >> 32));
        return __builtin_bit_cast(double, ((long long)hi << 32) | (unsigned int)lo);
    };
    v += step(v, [](int w) { return __builtin_amdgcn_update_dpp(0, w, 0xB1, 0xf, 0xf, true); });
    v += step(v, [](int w) { return __builtin_amdgcn_update_dpp(0, w, 0x4E, 0xf, 0xf, true); });
    v += step(v, [](int w) { return __builtin_amdgcn_update_dpp(0, w, 0x141, 0xf, 0xf, true); });
    if constexpr (GL >= 16) v += step(v, [](int w) { return __builtin_amdgcn_update_dpp(0, w, 0x140, 0xf, 0xf, true); });
    if constexpr (GL >= 32) v += __shfl_xor(v, 16, 64);
    return v;
}

extern "C" __global__ __launch_bounds__(64 * WPB) void molann_group_vjp(const float* __restrict__ x, const float* __restrict__ gout,
                                                                        const double* __restrict__ ref64_g, const float* __restrict__ ref32_g,
                                                                        const int* __restrict__ align_g, const int* __restrict__ items_g,
                                                                        const int* __restrict__ atoms_g, const int* __restrict__ ptr_g,
                                                                        const int* __restrict__ list_g, const float* __restrict__ wnat,
                                                                        float* __restrict__ out, float* __restrict__ gx, long n_frames) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[LDS_BYTES];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    double* t_ref64 = (double*)smem;
    float* t_ref32 = (float*)(smem + OFF_REF32);
    int* t_align = (int*)(smem + OFF_ALIGN);
    int* t_items = (int*)(smem + OFF_ITEMS);             // 8 ints per item (ItemDev)
    int* t_atoms = (int*)(smem + OFF_ATOMS);
    int* t_ptr = (int*)(smem + OFF_PTR);
    int* t_list = (int*)(smem + OFF_LIST);
    float* img = (float*)(smem + OFF_IMG);
    float* S = (float*)(smem + OFF_S);                   // the tile's [unit][frame] scratch
    FrameState* st = (FrameState*)(smem + OFF_ST);       // [64]
    constexpr int n_ref = 3 * N_ALIGN + 8;               // the packed reference: coordinates, then its constants
    const int nw = (int)(blockDim.x >> 6);               // waves of this launch (<= WPB)
    for (int i = threadIdx.x; i < n_ref; i += blockDim.x) { t_ref64[i] = ref64_g[i]; t_ref32[i] = ref32_g[i]; }
    for (int i = threadIdx.x; i < N_ALIGN; i += blockDim.x) t_align[i] = align_g[i];
    for (int i = threadIdx.x; i < 8 * N_ITEMS; i += blockDim.x) t_items[i] = items_g[i];
    for (int i = threadIdx.x; i < N_TOUCHED; i += blockDim.x) t_atoms[i] = atoms_g[i];
    for (int i = threadIdx.x; i <= N_TOUCHED; i += blockDim.x) t_ptr[i] = ptr_g[i];
    for (int i = threadIdx.x; i < N_LIST; i += blockDim.x) t_list[i] = list_g[i];
    // rows K .. pad4(K) of every scratch region are read as zeros by the head's k-steps and only ever written with zeros
    for (int i = threadIdx.x; i < S_ROWS * SSTR; i += blockDim.x) S[i] = 0.f;
    MlpTileState mlp;
    if constexpr (NL > 0)
        if (wave == 0) mlp_tile_init(mlp, wnat, img, lane);
    __syncthreads();

    const int gb = lane / GL, gj = lane % GL;
    float* gyf = (float*)(smem + OFF_GY) + (wave * B + gb) * GY_FRAME;     // this lane's frame: [item][atom of item][xyz]
    constexpr bool has_align = N_ALIGN > 0;
    constexpr int cb = 3 * N_ALIGN;
    const double srx = t_ref64[cb], sry = t_ref64[cb + 1], srz = t_ref64[cb + 2], gref = t_ref64[cb + 3];
    const float inv_a = t_ref32[cb + 4], fa = t_ref32[cb + 5];

    const long n_tiles = (n_frames + 63) >> 6;
    for (long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const long base = t * 64;
        const int nfr = n_frames - base < 64 ? (int)(n_frames - base) : 64;
        const int n_rounds = (nfr + B - 1) / B;
        // ---- A. forward: rotation and features of the round's frames -------------------------------------------------------------
        for (int r = wave; r < n_rounds; r += nw) {
            const int col = r * B + gb;                                     // the frame's column in S
            const bool valid = col < nfr;
            const long f = base + (valid ? col : nfr - 1);
            const float* xf = x + f * (long)FRAME_DW;
            float R[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
            double h[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.};
            V3 c0 = v3(0.f, 0.f, 0.f), dl = v3(0.f, 0.f, 0.f);
            if constexpr (has_align) {
                float sx = 0.f, sy = 0.f, sz = 0.f, g = 0.f;
                c0 = load_atom(xf, t_align[0]);
#pragma unroll 4
                for (int i = gj; i < N_ALIGN; i += GL) {
                    const double rx = t_ref64[3 * i], ry = t_ref64[3 * i + 1], rz = t_ref64[3 * i + 2];
                    const V3 p = load_atom(xf, t_align[i]) - c0;
                    sx += p.x; sy += p.y; sz += p.z;
                    g = fmaf(p.x, p.x, fmaf(p.y, p.y, fmaf(p.z, p.z, g)));
                    const double px = p.x, py = p.y, pz = p.z;
                    h[0] = fma(px, rx, h[0]); h[1] = fma(px, ry, h[1]); h[2] = fma(px, rz, h[2]);
                    h[3] = fma(py, rx, h[3]); h[4] = fma(py, ry, h[4]); h[5] = fma(py, rz, h[5]);
                    h[6] = fma(pz, rx, h[6]); h[7] = fma(pz, ry, h[7]); h[8] = fma(pz, rz, h[8]);
                }
                sx = group_sum_f(sx); sy = group_sum_f(sy); sz = group_sum_f(sz); g = group_sum_f(g);
#pragma unroll
                for (int i = 0; i < 9; ++i) h[i] = group_sum_d(h[i]);
                dl = v3(sx * inv_a, sy * inv_a, sz * inv_a);
                const double dx = dl.x, dy = dl.y, dz = dl.z;
                h[0] = fma(-dx, srx, h[0]); h[1] = fma(-dx, sry, h[1]); h[2] = fma(-dx, srz, h[2]);
                h[3] = fma(-dy, srx, h[3]); h[4] = fma(-dy, sry, h[4]); h[5] = fma(-dy, srz, h[5]);
                h[6] = fma(-dz, srx, h[6]); h[7] = fma(-dz, sry, h[7]); h[8] = fma(-dz, srz, h[8]);
                const float gp = fmaxf(g - fa * dot(dl, dl), 0.f);
                kabsch_rotation(h, 0.5 * ((double)gp + gref) * 1.0001, R);
                if (gj == 0) {   // (every lane of the group holds the same totals)
                    FrameState& s = st[col];
#pragma unroll
                    for (int i = 0; i < 9; ++i) { s.h[i] = h[i]; s.R[i] = R[i]; }
                    s.c0[0] = c0.x; s.c0[1] = c0.y; s.c0[2] = c0.z;
                    s.dl[0] = dl.x; s.dl[1] = dl.y; s.dl[2] = dl.z;
                }
            }
            for (int it = gj; it < N_ITEMS; it += GL) {   // the features as the forward kernels compute them (align_item_atoms)
                const int* d = t_items + 8 * it;
                const int type = d[0], c = d[1];
                V3 p0 = load_atom(xf, d[2]), p1 = load_atom(xf, d[3]), p2 = load_atom(xf, d[4]), p3 = load_atom(xf, d[5]);
                if constexpr (has_align) align_item_atoms(type, p0, p1, p2, p3, c0, dl, R);
                float v[3];
                const int w = eval_item(type, p0, p1, p2, p3, v);
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    if (j < w) {
                        if constexpr (NL == 0) {   // y = f, and the cotangent takes the features' place in S
                            if (valid) out[f * D_FEAT + c + j] = v[j];
                            S[(c + j) * SSTR + col] = valid ? gout[f * D_FEAT + c + j] : 0.f;
                        } else {
                            S[(c + j) * SSTR + col] = v[j];
                        }
                    }
                }
            }
        }
        __syncthreads();
        // ---- B. the head on the matrix cores: y -> out, dL/df -> S rows GF_ROW .. ----------------------------------------------
        if constexpr (NL > 0) {
            if (wave == 0) {
                const bool live = lane < nfr;
                const long fl = base + (live ? lane : nfr - 1);
                float fv[D_FEAT], gv[OUTC];
#pragma unroll
                for (int c = 0; c < D_FEAT; ++c) fv[c] = S[c * SSTR + lane];
#pragma unroll
                for (int c = 0; c < OUTC; ++c) gv[c] = live ? gout[fl * OUTC + c] : 0.f;
                mlp_tile_backward(mlp, S, img, lane, fv, gv, false, true, wnat, out + base * OUTC, nfr);
            }
            __syncthreads();
        }
        // ---- C. backward of the features, the rotation and the centring; grad_x rows out -------------------------------------------
        for (int r = wave; r < n_rounds; r += nw) {
            const int col = r * B + gb;
            const bool valid = col < nfr;
            const long f = base + (valid ? col : nfr - 1);
            const float* xf = x + f * (long)FRAME_DW;
            {   // zero the round's gradient rows (contiguous); the touched atoms' stores land behind them
                const int left = nfr - r * B;
                const int n_dw = (left < B ? left : B) * FRAME_DW;
                float* g0 = gx + (base + r * B) * (long)FRAME_DW;
                for (int c = lane; c < n_dw; c += 64) g0[c] = 0.f;
            }
            float R[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
            double h[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.};
            V3 c0 = v3(0.f, 0.f, 0.f), dl = v3(0.f, 0.f, 0.f);
            if constexpr (has_align) {
                const FrameState& s = st[col];
#pragma unroll
                for (int i = 0; i < 9; ++i) { h[i] = s.h[i]; R[i] = s.R[i]; }
                c0 = v3(s.c0[0], s.c0[1], s.c0[2]);
                dl = v3(s.dl[0], s.dl[1], s.dl[2]);
            }
            // items of the lane's frame: g_y of their atoms -> LDS;  G_R += p^T g_y,  sum of g_y
            float GR[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            V3 gysum = v3(0.f, 0.f, 0.f);
            for (int it = gj; it < N_ITEMS; it += GL) {
                const int* d = t_items + 8 * it;
                const int type = d[0], c = d[1];
                const int w = item_width(type);
                float g3[3];
#pragma unroll
                for (int j = 0; j < 3; ++j) g3[j] = j < w ? S[(GF_ROW + c + j) * SSTR + col] : 0.f;
                // (the arithmetic of frames_group_bwd_kernel: the same gradients as the three-launch backward, up to the features)
                V3 pc[4], y[4], gy[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    pc[j] = load_atom(xf, d[2 + j]);
                    y[j] = pc[j];
                    if constexpr (has_align) pc[j] = (pc[j] - c0) - dl;
                    gy[j] = v3(0.f, 0.f, 0.f);
                }
                if constexpr (has_align) align_item_atoms(type, y[0], y[1], y[2], y[3], c0, dl, R);   // as the forward above
                eval_item_backward(type, y[0], y[1], y[2], y[3], g3, gy[0], gy[1], gy[2], gy[3]);
                const int na = item_atoms(type);
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const V3 gg = j < na ? gy[j] : v3(0.f, 0.f, 0.f);
                    float* dst = gyf + (4 * it + j) * 3;
                    dst[0] = gg.x; dst[1] = gg.y; dst[2] = gg.z;
                    if (has_align && j < na) {
                        GR[0] = fmaf(pc[j].x, gg.x, GR[0]); GR[1] = fmaf(pc[j].x, gg.y, GR[1]); GR[2] = fmaf(pc[j].x, gg.z, GR[2]);
                        GR[3] = fmaf(pc[j].y, gg.x, GR[3]); GR[4] = fmaf(pc[j].y, gg.y, GR[4]); GR[5] = fmaf(pc[j].y, gg.z, GR[5]);
                        GR[6] = fmaf(pc[j].z, gg.x, GR[6]); GR[7] = fmaf(pc[j].z, gg.y, GR[7]); GR[8] = fmaf(pc[j].z, gg.z, GR[8]);
                        gysum = gysum + gg;
                    }
                }
            }
            // rotation backward; the centroid's share: centroid = mean of the alignment rows, sum of g_p = (sum of g_y) R^T
            float GH[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            V3 gcen = v3(0.f, 0.f, 0.f);
            if constexpr (has_align) {
#pragma unroll
                for (int i = 0; i < 9; ++i) GR[i] = group_sum_f(GR[i]);
                gysum = v3(group_sum_f(gysum.x), group_sum_f(gysum.y), group_sum_f(gysum.z));
                kabsch_rotation_backward(h, R, GR, GH);
                gcen = inv_a * rotate_back(gysum, R);
            }
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); // the zero stores are acknowledged, the g_y are in LDS
            // touched atoms of the lane's frame: own contributions summed, rotated back, alignment rows, plain stores
            for (int a = gj; a < N_TOUCHED; a += GL) {
                V3 gg = v3(0.f, 0.f, 0.f), rsum = v3(0.f, 0.f, 0.f);
                float n_rows = 0.f;
                const int k1 = t_ptr[a + 1];
                for (int k = t_ptr[a]; k < k1; ++k) {
                    const int e = t_list[k];
                    if (e >= 0) {
                        const float* src = gyf + 3 * e;
                        gg = gg + v3(src[0], src[1], src[2]);
                    } else {   // H = sum_i p_i ref_i^T :  g_p[i] += G_H ref_i - g_centroid
                        const int i = -1 - e;
                        rsum = rsum + v3(t_ref32[3 * i], t_ref32[3 * i + 1], t_ref32[3 * i + 2]);
                        n_rows += 1.f;
                    }
                }
                V3 gp = gg;
                if constexpr (has_align) {
                    gp = rotate_back(gg, R);
                    if (n_rows > 0.f)
                        gp = gp + (v3(fmaf(GH[2], rsum.z, fmaf(GH[1], rsum.y, GH[0] * rsum.x)), fmaf(GH[5], rsum.z, fmaf(GH[4], rsum.y, GH[3] * rsum.x)),
                                      fmaf(GH[8], rsum.z, fmaf(GH[7], rsum.y, GH[6] * rsum.x))) - n_rows * gcen);
                }
                if (valid) {
                    float* dst = gx + f * (long)FRAME_DW + 3 * t_atoms[a];
                    dst[0] = gp.x; dst[1] = gp.y; dst[2] = gp.z;
                }
            }
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the g_y buffer is read before the next round's items overwrite it
        }
        __syncthreads();   // S and the frame states are free for the next tile
    }
}
