// molann_dev_bwd.inc - part of libmolann_hip.so, included by molann_kernels.hip (one translation unit: the kernels' host stubs and the
// launches that use them must see each other).  reduce_rows_kernel and the backward of large frames (frames_wave_bwd_kernel, frames_wave_bwd_gather_kernel).
namespace {

// =============================================================================================
// dst[i] += sum over rows of part[row][i]: the per-block parameter sums of molann_mlp_bwd (one writer per element).
// Block = 64 elements x 16 row groups, so a thread's chain of loads is n_rows / 16 long.
__global__ __launch_bounds__(1024) void reduce_rows_kernel(const float* __restrict__ part, int n_rows, int n, float* __restrict__ dst) {
    __shared__ float acc[16][64];
    const int x = threadIdx.x & 63, y = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + x;
    float s0 = 0.f, s1 = 0.f;
    if (i < n) {
        int r = y;
        for (; r + 16 < n_rows; r += 32) { s0 += part[(long)r * n + i]; s1 += part[(long)(r + 16) * n + i]; }
        if (r < n_rows) s0 += part[(long)r * n + i];
    }
    acc[y][x] = s0 + s1;
    __syncthreads();
    if (y == 0 && i < n) {
        float s = 0.f;
#pragma unroll
        for (int g = 0; g < 16; ++g) s += acc[g][x];
        dst[i] += s;
    }
}

// frames_wave_bwd_kernel: dL/dx of frames_wave_kernel (features of large frames), one wave per frame
// =============================================================================================
// grad_out[f][d_feat] -> grad_x[f][n_inp][3].  The frame's gradient row is zeroed with coalesced stores, then
// every contribution is a float atomic into it (an atom may sit in several items and in the alignment set).
//   items (lanes):  y_j = ((p_j - c0) - dl) R ;  g_y from eval_item_backward ;  g_p = g_y R^T ;
//                   G_R += (p_j - c)^T g_y ;  g_sum += g_p
//   wave:           G_R, g_sum reduced ;  G_H = kabsch_rotation_backward(H, R, G_R)
//   align atoms:    g_p[i] += G_H ref_i - g_sum / a        (H = sum_i p_i ref_i^T, c = mean of the align atoms)
// The forward quantities (c, H, R) are recomputed exactly as frames_wave_kernel computes them.
__global__ __launch_bounds__(256) void frames_wave_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gout,
                                                              float* __restrict__ gx, const int* __restrict__ align_idx,
                                                              const float* __restrict__ ref, const double* __restrict__ ref64,
                                                              const ItemDev* __restrict__ items, PreArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int wpb = (int)(blockDim.x >> 6);
    const auto refc = as_const(ref);
    const bool has_align = a.n_align > 0;

    for (long f = (long)blockIdx.x * wpb + wave; f < a.n_frames; f += (long)gridDim.x * wpb) {
        const float* xf = x + f * (long)a.frame_dw;
        float* gxf = gx + f * (long)a.frame_dw;
        const float* gf = gout + f * (long)a.out_cols;
        // ---- 0. zero this frame's gradient row; the stores must have landed before the atomics below
        if (a.out_wide && (a.frame_dw & 3) == 0) {
            for (int c = lane; c < (a.frame_dw >> 2); c += 64) ((f32x4*)gxf)[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
        } else {
            for (int c = lane; c < a.frame_dw; c += 64) gxf[c] = 0.f;
        }
        // ---- 1. forward recompute: centre, covariance, rotation
        float R[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
        double h[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.};
        V3 c0 = v3(0.f, 0.f, 0.f), dl = v3(0.f, 0.f, 0.f);
        if (has_align) {
            const int k0 = as_const(align_idx)[0];
            c0 = load_atom(xf, k0);
            float sx = 0.f, sy = 0.f, sz = 0.f, g = 0.f;
#pragma unroll 4
            for (int i = lane; i < a.n_align; i += 64) {
                const int k = align_idx[i];
                const double rx = ref64[3 * i], ry = ref64[3 * i + 1], rz = ref64[3 * i + 2];
                const V3 p = load_atom(xf, k) - c0;
                sx += p.x; sy += p.y; sz += p.z;
                g = fmaf(p.x, p.x, fmaf(p.y, p.y, fmaf(p.z, p.z, g)));
                const double px = p.x, py = p.y, pz = p.z;
                h[0] = fma(px, rx, h[0]); h[1] = fma(px, ry, h[1]); h[2] = fma(px, rz, h[2]);
                h[3] = fma(py, rx, h[3]); h[4] = fma(py, ry, h[4]); h[5] = fma(py, rz, h[5]);
                h[6] = fma(pz, rx, h[6]); h[7] = fma(pz, ry, h[7]); h[8] = fma(pz, rz, h[8]);
            }
            sx = wave_sum(sx); sy = wave_sum(sy); sz = wave_sum(sz); g = wave_sum(g);
#pragma unroll
            for (int i = 0; i < 9; ++i) h[i] = wave_sum(h[i]);
            const int cb = 3 * a.n_align;
            const auto r64c = as_const(ref64);
            const double srx = r64c[cb], sry = r64c[cb + 1], srz = r64c[cb + 2], gref = r64c[cb + 3];
            const float inv_a = refc[cb + 4], fa = refc[cb + 5];
            dl = v3(sx * inv_a, sy * inv_a, sz * inv_a);
            const double dx = dl.x, dy = dl.y, dz = dl.z;
            h[0] = fma(-dx, srx, h[0]); h[1] = fma(-dx, sry, h[1]); h[2] = fma(-dx, srz, h[2]);
            h[3] = fma(-dy, srx, h[3]); h[4] = fma(-dy, sry, h[4]); h[5] = fma(-dy, srz, h[5]);
            h[6] = fma(-dz, srx, h[6]); h[7] = fma(-dz, sry, h[7]); h[8] = fma(-dz, srz, h[8]);
            const float gp = fmaxf(g - fa * dot(dl, dl), 0.f);
            kabsch_rotation(h, 0.5 * ((double)gp + gref) * 1.0001, R);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); // the zero stores are acknowledged

        // ---- 2. items
        float GR[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        V3 gsum = v3(0.f, 0.f, 0.f);
        for (int it = lane; it < a.n_items; it += 64) {
            const int4 d0 = ((const int4*)items)[2 * it];
            const int2 d1 = ((const int2*)items)[4 * it + 2];
            const int type = d0.x, col = d0.y;
            const int idx[4] = {d0.z, d0.w, d1.x, d1.y};
            V3 pc[4], y[4], gy[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                pc[j] = load_atom(xf, idx[j]);
                y[j] = pc[j];
                if (has_align) pc[j] = (pc[j] - c0) - dl;
                gy[j] = v3(0.f, 0.f, 0.f);
            }
            // (bond / angle / dihedral items on the rotated differences of the input atoms, as the forward: align_item_atoms)
            if (has_align) align_item_atoms(type, y[0], y[1], y[2], y[3], c0, dl, R);
            const int w = item_width(type);
            float g3[3] = {gf[col], w > 1 ? gf[col + 1] : 0.f, w > 2 ? gf[col + 2] : 0.f};
            eval_item_backward(type, y[0], y[1], y[2], y[3], g3, gy[0], gy[1], gy[2], gy[3]);
            const int na = item_atoms(type);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j < na) {
                    const V3 g = gy[j];
                    V3 gp = g;
                    if (has_align) { // y = pc R :  G_R += pc^T g ,  g_p = g R^T
                        GR[0] = fmaf(pc[j].x, g.x, GR[0]); GR[1] = fmaf(pc[j].x, g.y, GR[1]); GR[2] = fmaf(pc[j].x, g.z, GR[2]);
                        GR[3] = fmaf(pc[j].y, g.x, GR[3]); GR[4] = fmaf(pc[j].y, g.y, GR[4]); GR[5] = fmaf(pc[j].y, g.z, GR[5]);
                        GR[6] = fmaf(pc[j].z, g.x, GR[6]); GR[7] = fmaf(pc[j].z, g.y, GR[7]); GR[8] = fmaf(pc[j].z, g.z, GR[8]);
                        gp = v3(fmaf(g.z, R[2], fmaf(g.y, R[1], g.x * R[0])), fmaf(g.z, R[5], fmaf(g.y, R[4], g.x * R[3])),
                                fmaf(g.z, R[8], fmaf(g.y, R[7], g.x * R[6])));
                        gsum = gsum + gp;
                    }
                    float* dst = gxf + 3 * idx[j];
                    atomicAdd(dst, gp.x); atomicAdd(dst + 1, gp.y); atomicAdd(dst + 2, gp.z);
                }
            }
        }
        // ---- 3. rotation and centring backward through the alignment atoms
        if (has_align) {
#pragma unroll
            for (int i = 0; i < 9; ++i) GR[i] = wave_sum(GR[i]);
            gsum = v3(wave_sum(gsum.x), wave_sum(gsum.y), wave_sum(gsum.z));
            float GH[9];
            kabsch_rotation_backward(h, R, GR, GH);
            const float inv_a = refc[3 * a.n_align + 4];
            const V3 gcen = inv_a * gsum;
            for (int i = lane; i < a.n_align; i += 64) {
                const int k = align_idx[i];
                const float rx = ref[3 * i], ry = ref[3 * i + 1], rz = ref[3 * i + 2];
                const V3 add = v3(fmaf(GH[2], rz, fmaf(GH[1], ry, GH[0] * rx)), fmaf(GH[5], rz, fmaf(GH[4], ry, GH[3] * rx)),
                                  fmaf(GH[8], rz, fmaf(GH[7], ry, GH[6] * rx))) - gcen;
                float* dst = gxf + 3 * k;
                atomicAdd(dst, add.x); atomicAdd(dst + 1, add.y); atomicAdd(dst + 2, add.z);
            }
        }
    }
}

// frames_wave_bwd_gather_kernel: the same gradient without atomics (they were 9/10 of frames_wave_bwd_kernel's time: C4 80 us per
// 1000 frames against 8 for the forward with the same scattered loads).  Items (lanes) leave their atoms' gradients g_y in the
// wave's LDS buffer; then every TOUCHED ATOM (lanes again) adds up its own contributions - the lists are made at plan creation
// (bw_atoms: touched atoms; bw_ptr / bw_list: CSR of (item, atom-of-item) pairs per touched atom; bw_align: its place in the
// alignment set or -1) - rotates the sum back once, adds the alignment terms and stores its three floats behind the zero-fill.
struct BwGatherArgs { int n_touched, lds_per_wave; };
__global__ __launch_bounds__(256) void frames_wave_bwd_gather_kernel(const float* __restrict__ x, const float* __restrict__ gout,
                                                                     float* __restrict__ gx, const int* __restrict__ align_idx,
                                                                     const float* __restrict__ ref, const double* __restrict__ ref64,
                                                                     const ItemDev* __restrict__ items, const int* __restrict__ bw_atoms,
                                                                     const int* __restrict__ bw_ptr, const int* __restrict__ bw_list,
                                                                     const int* __restrict__ bw_align, PreArgs a, BwGatherArgs b) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int wpb = (int)(blockDim.x >> 6);
    float* gyb = (float*)(smem + (size_t)wave * b.lds_per_wave);   // [item][atom of item][xyz]
    const auto refc = as_const(ref);
    const bool has_align = a.n_align > 0;

    for (long f = (long)blockIdx.x * wpb + wave; f < a.n_frames; f += (long)gridDim.x * wpb) {
        const float* xf = x + f * (long)a.frame_dw;
        float* gxf = gx + f * (long)a.frame_dw;
        const float* gf = gout + f * (long)a.out_cols;
        // ---- 0. zero this frame's gradient row
        if (a.out_wide && (a.frame_dw & 3) == 0) {
            for (int c = lane; c < (a.frame_dw >> 2); c += 64) ((f32x4*)gxf)[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
        } else {
            for (int c = lane; c < a.frame_dw; c += 64) gxf[c] = 0.f;
        }
        // ---- 1. forward recompute: centre, covariance, rotation (as frames_wave_bwd_kernel)
        float R[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
        double h[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.};
        V3 c0 = v3(0.f, 0.f, 0.f), dl = v3(0.f, 0.f, 0.f);
        if (has_align) {
            const int k0 = as_const(align_idx)[0];
            c0 = load_atom(xf, k0);
            float sx = 0.f, sy = 0.f, sz = 0.f, g = 0.f;
#pragma unroll 4
            for (int i = lane; i < a.n_align; i += 64) {
                const int k = align_idx[i];
                const double rx = ref64[3 * i], ry = ref64[3 * i + 1], rz = ref64[3 * i + 2];
                const V3 p = load_atom(xf, k) - c0;
                sx += p.x; sy += p.y; sz += p.z;
                g = fmaf(p.x, p.x, fmaf(p.y, p.y, fmaf(p.z, p.z, g)));
                const double px = p.x, py = p.y, pz = p.z;
                h[0] = fma(px, rx, h[0]); h[1] = fma(px, ry, h[1]); h[2] = fma(px, rz, h[2]);
                h[3] = fma(py, rx, h[3]); h[4] = fma(py, ry, h[4]); h[5] = fma(py, rz, h[5]);
                h[6] = fma(pz, rx, h[6]); h[7] = fma(pz, ry, h[7]); h[8] = fma(pz, rz, h[8]);
            }
            sx = wave_sum(sx); sy = wave_sum(sy); sz = wave_sum(sz); g = wave_sum(g);
#pragma unroll
            for (int i = 0; i < 9; ++i) h[i] = wave_sum(h[i]);
            const int cb = 3 * a.n_align;
            const auto r64c = as_const(ref64);
            const double srx = r64c[cb], sry = r64c[cb + 1], srz = r64c[cb + 2], gref = r64c[cb + 3];
            const float inv_a = refc[cb + 4], fa = refc[cb + 5];
            dl = v3(sx * inv_a, sy * inv_a, sz * inv_a);
            const double dx = dl.x, dy = dl.y, dz = dl.z;
            h[0] = fma(-dx, srx, h[0]); h[1] = fma(-dx, sry, h[1]); h[2] = fma(-dx, srz, h[2]);
            h[3] = fma(-dy, srx, h[3]); h[4] = fma(-dy, sry, h[4]); h[5] = fma(-dy, srz, h[5]);
            h[6] = fma(-dz, srx, h[6]); h[7] = fma(-dz, sry, h[7]); h[8] = fma(-dz, srz, h[8]);
            const float gp = fmaxf(g - fa * dot(dl, dl), 0.f);
            kabsch_rotation(h, 0.5 * ((double)gp + gref) * 1.0001, R);
        }
        // ---- 2. items: g_y of their atoms -> LDS;  G_R += p^T g_y,  sum of g_y
        float GR[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        V3 gysum = v3(0.f, 0.f, 0.f);
        for (int it = lane; it < a.n_items; it += 64) {
            const int4 d0 = ((const int4*)items)[2 * it];
            const int2 d1 = ((const int2*)items)[4 * it + 2];
            const int type = d0.x, col = d0.y;
            const int idx[4] = {d0.z, d0.w, d1.x, d1.y};
            V3 pc[4], y[4], gy[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                pc[j] = load_atom(xf, idx[j]);
                y[j] = pc[j];
                if (has_align) pc[j] = (pc[j] - c0) - dl;
                gy[j] = v3(0.f, 0.f, 0.f);
            }
            // (bond / angle / dihedral items on the rotated differences of the input atoms, as the forward: align_item_atoms)
            if (has_align) align_item_atoms(type, y[0], y[1], y[2], y[3], c0, dl, R);
            const int w = item_width(type);
            float g3[3] = {gf[col], w > 1 ? gf[col + 1] : 0.f, w > 2 ? gf[col + 2] : 0.f};
            eval_item_backward(type, y[0], y[1], y[2], y[3], g3, gy[0], gy[1], gy[2], gy[3]);
            const int na = item_atoms(type);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const V3 g = j < na ? gy[j] : v3(0.f, 0.f, 0.f);
                float* dst = gyb + (4 * it + j) * 3;
                dst[0] = g.x; dst[1] = g.y; dst[2] = g.z;
                if (has_align && j < na) {
                    GR[0] = fmaf(pc[j].x, g.x, GR[0]); GR[1] = fmaf(pc[j].x, g.y, GR[1]); GR[2] = fmaf(pc[j].x, g.z, GR[2]);
                    GR[3] = fmaf(pc[j].y, g.x, GR[3]); GR[4] = fmaf(pc[j].y, g.y, GR[4]); GR[5] = fmaf(pc[j].y, g.z, GR[5]);
                    GR[6] = fmaf(pc[j].z, g.x, GR[6]); GR[7] = fmaf(pc[j].z, g.y, GR[7]); GR[8] = fmaf(pc[j].z, g.z, GR[8]);
                    gysum = gysum + g;
                }
            }
        }
        // ---- 3. rotation backward; the centroid's share
        float GH[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        V3 gcen = v3(0.f, 0.f, 0.f);
        if (has_align) {
#pragma unroll
            for (int i = 0; i < 9; ++i) GR[i] = wave_sum(GR[i]);
            gysum = v3(wave_sum(gysum.x), wave_sum(gysum.y), wave_sum(gysum.z));
            kabsch_rotation_backward(h, R, GR, GH);
            const V3 gs = v3(fmaf(gysum.z, R[2], fmaf(gysum.y, R[1], gysum.x * R[0])), fmaf(gysum.z, R[5], fmaf(gysum.y, R[4], gysum.x * R[3])),
                             fmaf(gysum.z, R[8], fmaf(gysum.y, R[7], gysum.x * R[6])));   // sum of g_p = (sum of g_y) R^T
            gcen = refc[3 * a.n_align + 4] * gs;
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); // the zero stores are acknowledged, the g_y are in LDS
        // ---- 4. touched atoms: own contributions summed, rotated back, alignment terms, plain stores
        for (int t = lane; t < b.n_touched; t += 64) {
            V3 g = v3(0.f, 0.f, 0.f);
            const int k1 = bw_ptr[t + 1];
            for (int k = bw_ptr[t]; k < k1; ++k) {
                const float* src = gyb + 3 * bw_list[k];
                g = g + v3(src[0], src[1], src[2]);
            }
            V3 gp = g;
            if (has_align) {
                gp = v3(fmaf(g.z, R[2], fmaf(g.y, R[1], g.x * R[0])), fmaf(g.z, R[5], fmaf(g.y, R[4], g.x * R[3])),
                        fmaf(g.z, R[8], fmaf(g.y, R[7], g.x * R[6])));
                const int i = bw_align[t];
                if (i >= 0) {
                    const float rx = ref[3 * i], ry = ref[3 * i + 1], rz = ref[3 * i + 2];
                    gp = gp + (v3(fmaf(GH[2], rz, fmaf(GH[1], ry, GH[0] * rx)), fmaf(GH[5], rz, fmaf(GH[4], ry, GH[3] * rx)),
                                  fmaf(GH[8], rz, fmaf(GH[7], ry, GH[6] * rx))) - gcen);
                }
            }
            float* dst = gxf + 3 * bw_atoms[t];
            dst[0] = gp.x; dst[1] = gp.y; dst[2] = gp.z;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the LDS buffer is read before the next frame's items overwrite it
    }
}

// frames_group_bwd_kernel: the same gradient on MID-SIZE frames, B frames per wave and round (round 3).
// frames_wave_bwd_gather_kernel runs one frame per wave through six dependent trips to memory (alignment table -> atoms, item
// table -> atoms, contribution lists -> stores) and two wave-redundant fp64 solves: ~27 us per frame and wave, 3.5 ms per 1 M
// frames of the 166-atom P1 whatever the frame holds.  Here a wave takes B CONSECUTIVE frames per round, a group of GL = 64 / B
// lanes each: lane (b, j) sums frame b's covariance over alignment atoms j, j + GL, .., a butterfly inside the group totals the
// sums, every lane solves its frame's rotation (and, later, its backward) once per round; the items and the touched atoms of
// frame b are spread over the group's lanes.  Every table (alignment atoms, reference, items, contribution lists) is copied to
// LDS once per block; the items' atoms and cotangents are requested before the solve.  Same arithmetic per frame.
struct GroupBwdArgs {
    int n_touched, n_list;
    int gy_frame;       // floats of one frame's [item][atom of item][xyz] buffer
    int off_ref32, off_align, off_items, off_bw_atoms, off_bw_ptr, off_bw_list, off_bw_align, off_gy;   // byte offsets in LDS (ref64 at 0)
};

template <int B>
__global__ __launch_bounds__(256) void frames_group_bwd_kernel(const float* __restrict__ x, const float* __restrict__ gout,
                                                               float* __restrict__ gx, const int* __restrict__ align_idx,
                                                               const float* __restrict__ ref, const double* __restrict__ ref64,
                                                               const ItemDev* __restrict__ items, const int* __restrict__ bw_atoms,
                                                               const int* __restrict__ bw_ptr, const int* __restrict__ bw_list,
                                                               const int* __restrict__ bw_align, PreArgs a, GroupBwdArgs b) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int GL = 64 / B;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int wpb = (int)(blockDim.x >> 6);
    double* t_ref64 = (double*)smem;
    float* t_ref32 = (float*)(smem + b.off_ref32);
    int* t_align = (int*)(smem + b.off_align);
    int* t_items = (int*)(smem + b.off_items);            // 8 ints per item
    int* t_bw_atoms = (int*)(smem + b.off_bw_atoms);
    int* t_bw_ptr = (int*)(smem + b.off_bw_ptr);
    int* t_bw_list = (int*)(smem + b.off_bw_list);
    int* t_bw_align = (int*)(smem + b.off_bw_align);
    const int n_ref = 3 * a.n_align + 8;                   // the packed reference: coordinates, then its constants
    for (int i = threadIdx.x; i < n_ref; i += blockDim.x) { t_ref64[i] = ref64[i]; t_ref32[i] = ref[i]; }
    for (int i = threadIdx.x; i < a.n_align; i += blockDim.x) t_align[i] = align_idx[i];
    for (int i = threadIdx.x; i < 8 * a.n_items; i += blockDim.x) t_items[i] = ((const int*)items)[i];
    for (int i = threadIdx.x; i < b.n_touched; i += blockDim.x) { t_bw_atoms[i] = bw_atoms[i]; t_bw_align[i] = bw_align[i]; }
    for (int i = threadIdx.x; i <= b.n_touched; i += blockDim.x) t_bw_ptr[i] = bw_ptr[i];
    for (int i = threadIdx.x; i < b.n_list; i += blockDim.x) t_bw_list[i] = bw_list[i];
    __syncthreads();

    const int gb = lane / GL, gj = lane % GL;
    float* gyf = (float*)(smem + b.off_gy) + ((size_t)wave * B + gb) * b.gy_frame;    // this lane's frame: [item][atom of item][xyz]
    const bool has_align = a.n_align > 0;
    const int cb = 3 * a.n_align;
    const double srx = t_ref64[cb], sry = t_ref64[cb + 1], srz = t_ref64[cb + 2], gref = t_ref64[cb + 3];
    const float inv_a = t_ref32[cb + 4], fa = t_ref32[cb + 5];
    auto group_sum_f = [](float v) {
        v += dpp_mov<0xB1>(v); v += dpp_mov<0x4E>(v); v += dpp_mov<0x141>(v);
        if constexpr (GL >= 16) v += dpp_mov<0x140>(v);
        if constexpr (GL >= 32) v += __shfl_xor(v, 16, 64);
        return v;
    };
    auto group_sum_d = [](double v) {
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
    };

    const long n_rounds = (a.n_frames + B - 1) / B;
    for (long q = (long)blockIdx.x * wpb + wave; q < n_rounds; q += (long)gridDim.x * wpb) {
        const long f0 = q * B;
        const bool valid = f0 + gb < a.n_frames;
        const long f = valid ? f0 + gb : a.n_frames - 1;       // (a short last round: the last frame again, nothing stored for it)
        const float* xf = x + f * (long)a.frame_dw;
        float* gxf = gx + f * (long)a.frame_dw;
        const float* gf = gout + f * (long)a.out_cols;
        // ---- 0. zero the round's gradient rows (contiguous)
        {
            const long left = a.n_frames - f0;
            const long n_dw = (left < B ? left : (long)B) * a.frame_dw;
            float* g0 = gx + f0 * (long)a.frame_dw;
            for (long c = lane; c < n_dw; c += 64) g0[c] = 0.f;
        }
        // ---- 1. forward recompute: centre, covariance (the group's lanes over the alignment atoms), rotation
        float R[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
        double h[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.};
        V3 c0 = v3(0.f, 0.f, 0.f), dl = v3(0.f, 0.f, 0.f);
        float sx = 0.f, sy = 0.f, sz = 0.f, g = 0.f;
        if (has_align) {
            c0 = load_atom(xf, t_align[0]);
#pragma unroll 4
            for (int i = gj; i < a.n_align; i += GL) {
                const double rx = t_ref64[3 * i], ry = t_ref64[3 * i + 1], rz = t_ref64[3 * i + 2];
                const V3 p = load_atom(xf, t_align[i]) - c0;
                sx += p.x; sy += p.y; sz += p.z;
                g = fmaf(p.x, p.x, fmaf(p.y, p.y, fmaf(p.z, p.z, g)));
                const double px = p.x, py = p.y, pz = p.z;
                h[0] = fma(px, rx, h[0]); h[1] = fma(px, ry, h[1]); h[2] = fma(px, rz, h[2]);
                h[3] = fma(py, rx, h[3]); h[4] = fma(py, ry, h[4]); h[5] = fma(py, rz, h[5]);
                h[6] = fma(pz, rx, h[6]); h[7] = fma(pz, ry, h[7]); h[8] = fma(pz, rz, h[8]);
            }
        }
        // the first pass of items: atoms and cotangents requested now, the solve runs under their latency
        const int it0 = gj;
        const bool live0 = it0 < a.n_items;
        int d_type = 0, d_col = 0, d_idx[4] = {0, 0, 0, 0};
        V3 pre[4];
        float g3pre[3] = {0.f, 0.f, 0.f};
        {
            const int* d = t_items + 8 * (live0 ? it0 : 0);
            d_type = d[0]; d_col = d[1]; d_idx[0] = d[2]; d_idx[1] = d[3]; d_idx[2] = d[4]; d_idx[3] = d[5];
#pragma unroll
            for (int j = 0; j < 4; ++j) pre[j] = load_atom(xf, d_idx[j]);
            const int w = item_width(d_type);
            g3pre[0] = gf[d_col]; g3pre[1] = w > 1 ? gf[d_col + 1] : 0.f; g3pre[2] = w > 2 ? gf[d_col + 2] : 0.f;
        }
        if (has_align) {
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
        }
        // ---- 2. items of the lane's frame: g_y of their atoms -> LDS;  G_R += p^T g_y,  sum of g_y
        float GR[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        V3 gysum = v3(0.f, 0.f, 0.f);
        for (int it = it0; it < a.n_items; it += GL) {
            int type = d_type, col = d_col;
            V3 pc[4];
            float g3[3];
            if (it == it0) {
#pragma unroll
                for (int j = 0; j < 4; ++j) pc[j] = pre[j];
                g3[0] = g3pre[0]; g3[1] = g3pre[1]; g3[2] = g3pre[2];
            } else {
                const int* d = t_items + 8 * it;
                type = d[0]; col = d[1];
#pragma unroll
                for (int j = 0; j < 4; ++j) pc[j] = load_atom(xf, d[2 + j]);
                const int w = item_width(type);
                g3[0] = gf[col]; g3[1] = w > 1 ? gf[col + 1] : 0.f; g3[2] = w > 2 ? gf[col + 2] : 0.f;
            }
            V3 y[4], gy[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                y[j] = pc[j];
                if (has_align) pc[j] = (pc[j] - c0) - dl;
                gy[j] = v3(0.f, 0.f, 0.f);
            }
            if (has_align) align_item_atoms(type, y[0], y[1], y[2], y[3], c0, dl, R);   // as the forward
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
        // ---- 3. rotation backward; the centroid's share
        float GH[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        V3 gcen = v3(0.f, 0.f, 0.f);
        if (has_align) {
#pragma unroll
            for (int i = 0; i < 9; ++i) GR[i] = group_sum_f(GR[i]);
            gysum = v3(group_sum_f(gysum.x), group_sum_f(gysum.y), group_sum_f(gysum.z));
            kabsch_rotation_backward(h, R, GR, GH);
            const V3 gs = v3(fmaf(gysum.z, R[2], fmaf(gysum.y, R[1], gysum.x * R[0])), fmaf(gysum.z, R[5], fmaf(gysum.y, R[4], gysum.x * R[3])),
                             fmaf(gysum.z, R[8], fmaf(gysum.y, R[7], gysum.x * R[6])));   // sum of g_p = (sum of g_y) R^T
            gcen = inv_a * gs;
        }
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory"); // the zero stores are acknowledged, the g_y are in LDS
        // ---- 4. touched atoms of the lane's frame: own contributions summed, rotated back, alignment terms, plain stores
        for (int t = gj; t < b.n_touched; t += GL) {
            V3 gg = v3(0.f, 0.f, 0.f);
            const int k1 = t_bw_ptr[t + 1];
            for (int k = t_bw_ptr[t]; k < k1; ++k) {
                const float* src = gyf + 3 * t_bw_list[k];
                gg = gg + v3(src[0], src[1], src[2]);
            }
            V3 gp = gg;
            if (has_align) {
                gp = v3(fmaf(gg.z, R[2], fmaf(gg.y, R[1], gg.x * R[0])), fmaf(gg.z, R[5], fmaf(gg.y, R[4], gg.x * R[3])),
                        fmaf(gg.z, R[8], fmaf(gg.y, R[7], gg.x * R[6])));
                const int i = t_bw_align[t];
                if (i >= 0) {
                    const float rx = t_ref32[3 * i], ry = t_ref32[3 * i + 1], rz = t_ref32[3 * i + 2];
                    gp = gp + (v3(fmaf(GH[2], rz, fmaf(GH[1], ry, GH[0] * rx)), fmaf(GH[5], rz, fmaf(GH[4], ry, GH[3] * rx)),
                                  fmaf(GH[8], rz, fmaf(GH[7], ry, GH[6] * rx))) - gcen);
                }
            }
            if (valid) {
                float* dst = gxf + 3 * t_bw_atoms[t];
                dst[0] = gp.x; dst[1] = gp.y; dst[2] = gp.z;
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); // the LDS buffer is read before the next round's items overwrite it
    }
}

} // namespace
