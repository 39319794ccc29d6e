// molann_lane_bwd.inc - backward of the lane-per-frame preprocessing (Kabsch + feature table), specialised for one
// plan (hipRTC, gfx950).
//
// The reference gets its gradients from torch autograd through ~60 ATen ops per forward, including the
// backward of a batched LAPACK SVD (ann.py:188).  Here one kernel recomputes the forward per frame (nothing
// is saved but x) and runs the analytic reverse mode of csrc/molann_math.h:
//
//   grad_f[N, D_FEAT]  ->  feature table backward (eval_item_backward)
//                      ->  rotation apply + closed-form Kabsch backward (kabsch_rotation_backward)
//                      ->  centring backward  ->  grad_x[N, N_INP, 3]   (zeros for untouched atoms)
//
// grad_f is the caller's gradient for plans without an MLP, and the output of molann_mlp_bwd.inc (the MLP's backward on
// the matrix cores, which also produces the parameter gradients) for plans with one.
//
// Same preamble as molann_lane_jit.inc with NL = 0.
#include "molann_math.h"

using namespace molann;
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) const void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;

constexpr int FRAME_DW = 3 * N_INP;
constexpr int FRAME_BYTES = 4 * FRAME_DW;
constexpr int TILE_BYTES = 64 * FRAME_BYTES;

extern "C" __global__ __launch_bounds__(64 * WPB) __attribute__((amdgpu_waves_per_eu(2))) void molann_lane_bwd(const float* __restrict__ x, const float* __restrict__ gfeat,
                                                                      const double* __restrict__ ref64_g, float* __restrict__ gx,
                                                                      long n_frames, int x_wide) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float* tile = (float*)(smem + (size_t)wave * LDS_PER_WAVE);
    const auto ref64 = (const __attribute__((address_space(4))) double*)ref64_g;
    const long n_tiles = (n_frames + 63) >> 6;

    for (long t = (long)blockIdx.x * WPB + wave; t < n_tiles; t += (long)gridDim.x * WPB) {
        const long rem = n_frames - t * 64;
        const int nfr = rem < 64 ? (int)rem : 64;
        const int valid_bytes = nfr * FRAME_BYTES;
        // ---- 1. stage the tile (dense LDS-DMA), wait, copy the touched atoms to registers -------------
        {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            const unsigned char* gsrc = (const unsigned char*)x + t * (long)TILE_BYTES;
            if (x_wide) {
                const int nchunk = valid_bytes >> 4;
#pragma unroll
                for (int c0 = 0; c0 < (TILE_BYTES >> 4); c0 += 64) {
                    const int c = c0 + lane;
                    if (c < nchunk)
                        __builtin_amdgcn_global_load_lds((gptr_t)(gsrc + (size_t)c * 16), (lptr_t)((unsigned char*)tile + (size_t)c0 * 16), 16, 0, 0);
                }
                const int rem_dw = (valid_bytes & 15) >> 2;
                if (lane < rem_dw)
                    __builtin_amdgcn_global_load_lds((gptr_t)(gsrc + (size_t)nchunk * 16 + lane * 4), (lptr_t)((unsigned char*)tile + (size_t)nchunk * 16), 4, 0, 0);
            } else {
                const int ndw = valid_bytes >> 2;
                for (int c0 = 0; c0 < ndw; c0 += 64) {
                    const int c = c0 + lane;
                    if (c < ndw)
                        __builtin_amdgcn_global_load_lds((gptr_t)(gsrc + (size_t)c * 4), (lptr_t)((unsigned char*)tile + (size_t)c0 * 4), 4, 0, 0);
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        const bool live = lane < nfr;              // lanes past the end recompute the last frame and contribute nothing
        const int fl = live ? lane : nfr - 1;
        const float* fr = tile + fl * FRAME_DW;
        V3 a[N_SLOTS];
#pragma unroll
        for (int u = 0; u < N_SLOTS; ++u) a[u] = v3(fr[3 * SLOT_ATOM[u]], fr[3 * SLOT_ATOM[u] + 1], fr[3 * SLOT_ATOM[u] + 2]);

        // ---- 2. forward recompute: Kabsch, aligned atoms, features ------------------------------------
        float R[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
        double h64[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.};
        V3 p[N_SLOTS], y[N_SLOTS];
        if constexpr (N_ALIGN > 0) {
            const V3 c0 = a[0];
            float sx = 0.f, sy = 0.f, sz = 0.f, g = 0.f;
#pragma unroll
            for (int i = 0; i < N_ALIGN; ++i) {
                const double rx = ref64[3 * i], ry = ref64[3 * i + 1], rz = ref64[3 * i + 2];
                const V3 q = a[i] - c0;
                sx += q.x; sy += q.y; sz += q.z;
                g = fmaf(q.x, q.x, fmaf(q.y, q.y, fmaf(q.z, q.z, g)));
                const double px = q.x, py = q.y, pz = q.z;
                h64[0] = fma(px, rx, h64[0]); h64[1] = fma(px, ry, h64[1]); h64[2] = fma(px, rz, h64[2]);
                h64[3] = fma(py, rx, h64[3]); h64[4] = fma(py, ry, h64[4]); h64[5] = fma(py, rz, h64[5]);
                h64[6] = fma(pz, rx, h64[6]); h64[7] = fma(pz, ry, h64[7]); h64[8] = fma(pz, rz, h64[8]);
            }
            constexpr int cb = 3 * N_ALIGN;
            const double srx = ref64[cb], sry = ref64[cb + 1], srz = ref64[cb + 2], gref = ref64[cb + 3];
            constexpr float fa = (float)N_ALIGN, inv_a = 1.0f / (N_ALIGN > 0 ? fa : 1.0f);
            const V3 dl = v3(sx * inv_a, sy * inv_a, sz * inv_a);
            const double dx = dl.x, dy = dl.y, dz = dl.z;
            h64[0] = fma(-dx, srx, h64[0]); h64[1] = fma(-dx, sry, h64[1]); h64[2] = fma(-dx, srz, h64[2]);
            h64[3] = fma(-dy, srx, h64[3]); h64[4] = fma(-dy, sry, h64[4]); h64[5] = fma(-dy, srz, h64[5]);
            h64[6] = fma(-dz, srx, h64[6]); h64[7] = fma(-dz, sry, h64[7]); h64[8] = fma(-dz, srz, h64[8]);
            const float gp = fmaxf(g - fa * dot(dl, dl), 0.f);
            kabsch_rotation(h64, 0.5 * ((double)gp + gref) * 1.0001, R);
#pragma unroll
            for (int u = 0; u < N_SLOTS; ++u) {
                p[u] = (a[u] - c0) - dl;
                y[u] = rotate(p[u], R);
            }
        } else {
#pragma unroll
            for (int u = 0; u < N_SLOTS; ++u) { p[u] = a[u]; y[u] = a[u]; }
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

        // ---- 3. dL / d features of this lane's frame -----------------------------------------------------
        float gf[D_FEAT > 0 ? D_FEAT : 1];
        {
            const float* grow = gfeat + (t * 64 + fl) * (long)D_FEAT;
#pragma unroll
            for (int k = 0; k < D_FEAT; ++k) gf[k] = live ? grow[k] : 0.f;
        }

        {
            // ---- 5. feature table backward: dL / d aligned atoms --------------------------------------
            V3 gy[N_SLOTS];
#pragma unroll
            for (int u = 0; u < N_SLOTS; ++u) gy[u] = v3(0.f, 0.f, 0.f);
#pragma unroll
            for (int it = 0; it < N_ITEMS; ++it) {
                float g3[3] = {0.f, 0.f, 0.f};
#pragma unroll
                for (int j = 0; j < 3; ++j)
                    if (j < item_width(ITEM_TYPE[it])) g3[j] = gf[ITEM_COL[it] + j];
                // (bond / angle / dihedral items on the rotated differences of the input atoms: align_item_atoms)
                V3 q0 = y[ITEM_IDX[it][0]], q1 = y[ITEM_IDX[it][1]], q2 = y[ITEM_IDX[it][2]], q3 = y[ITEM_IDX[it][3]];
                if constexpr (N_ALIGN > 0) {
                    if (ITEM_TYPE[it] != IT_POSITION) {
                        q0 = a[ITEM_IDX[it][0]]; q1 = a[ITEM_IDX[it][1]]; q2 = a[ITEM_IDX[it][2]]; q3 = a[ITEM_IDX[it][3]];
                        align_item_atoms(ITEM_TYPE[it], q0, q1, q2, q3, v3(0.f, 0.f, 0.f), v3(0.f, 0.f, 0.f), R);   // (no position item here)
                    }
                }
                eval_item_backward(ITEM_TYPE[it], q0, q1, q2, q3, g3,
                                   gy[ITEM_IDX[it][0]], gy[ITEM_IDX[it][1]], gy[ITEM_IDX[it][2]], gy[ITEM_IDX[it][3]]);
            }
            // ---- 6. rotation apply, Kabsch and centring backward: dL / d raw atoms -----------------------
            V3 ga[N_SLOTS];
            if constexpr (N_ALIGN > 0) {
                float GR[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, GH[9];
#pragma unroll
                for (int u = 0; u < N_SLOTS; ++u) {
                    if (SLOT_USED[u]) { // y_u = p_u R :  G_R += p_u^T g_y ,  g_p = g_y R^T
                        const V3 g = gy[u];
                        GR[0] = fmaf(p[u].x, g.x, GR[0]); GR[1] = fmaf(p[u].x, g.y, GR[1]); GR[2] = fmaf(p[u].x, g.z, GR[2]);
                        GR[3] = fmaf(p[u].y, g.x, GR[3]); GR[4] = fmaf(p[u].y, g.y, GR[4]); GR[5] = fmaf(p[u].y, g.z, GR[5]);
                        GR[6] = fmaf(p[u].z, g.x, GR[6]); GR[7] = fmaf(p[u].z, g.y, GR[7]); GR[8] = fmaf(p[u].z, g.z, GR[8]);
                        ga[u] = v3(fmaf(g.z, R[2], fmaf(g.y, R[1], g.x * R[0])), fmaf(g.z, R[5], fmaf(g.y, R[4], g.x * R[3])),
                                   fmaf(g.z, R[8], fmaf(g.y, R[7], g.x * R[6])));
                    } else {
                        ga[u] = v3(0.f, 0.f, 0.f);
                    }
                }
                kabsch_rotation_backward(h64, R, GR, GH);
                V3 gc = v3(0.f, 0.f, 0.f);
#pragma unroll
                for (int u = 0; u < N_SLOTS; ++u) {
                    if (u < N_ALIGN) { // H = sum_i p_i ref_i^T :  g_p[i] += G_H ref_i
                        const float rx = (float)ref64[3 * u], ry = (float)ref64[3 * u + 1], rz = (float)ref64[3 * u + 2];
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
            // ---- 7. grad_x tile: zeros, the touched atoms' gradients, coalesced store ------------------
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            for (int c = lane; c < (TILE_BYTES >> 4); c += 64) ((f32x4*)tile)[c] = (f32x4){0.f, 0.f, 0.f, 0.f};
            if (live) {
                float* row = tile + lane * FRAME_DW;
#pragma unroll
                for (int u = 0; u < N_SLOTS; ++u) { row[3 * SLOT_ATOM[u]] = ga[u].x; row[3 * SLOT_ATOM[u] + 1] = ga[u].y; row[3 * SLOT_ATOM[u] + 2] = ga[u].z; }
            }
            float* gdst = gx + t * 64 * (long)FRAME_DW;
            const int ndw = valid_bytes >> 2;
            if ((((size_t)gx) & 15) == 0) {
                const int nchunk = ndw >> 2;
                for (int c = lane; c < nchunk; c += 64) ((f32x4*)gdst)[c] = ((const f32x4*)tile)[c];
                for (int c = (nchunk << 2) + lane; c < ndw; c += 64) gdst[c] = tile[c];
            } else {
                for (int c = lane; c < ndw; c += 64) gdst[c] = tile[c];
            }
        }
    }
}
