// molann_chain_bwd.inc - backward of the WIDE fp32 heads (a width above 32, the chain forward of molann_mlp_jit.inc) on the
// fp32 matrix cores, specialised for one plan (hipRTC, gfx950).  Serves molann_mlp_backward_f32 where molann_mlp_bwd.inc
// (every width <= 32) cannot:
//
//   f[N, D0], grad_out[N, OUT]  ->  grad_f[N, D0] (optional), one row of dW / db partial sums per block (optional)
//
// v_mfma_f32_16x16x4_f32 throughout (exact fp32 products and sums).  Lane l of a 16x16x4 MFMA holds A[i][k] and B[k][i]
// with i = l & 15, k = l >> 4, and its accumulator D[4 (l >> 4) + r][l & 15], r = 0..3.
//
//   * Weights: the plan's natural fp32 copy (pack_mfma_kernel: Wp[Jp][Kp], zero padded, then bias[Jp] per layer) is copied
//     into LDS once per block with a row stride of Kp + 4.  The forward reads W[16 jb + i][16 kb + 4q .. +3] as one
//     16-byte read (the A operands of four MFMAs); the backward reads W^T[16 kb + i][16 jb + 4q + r] = W[16 jb + 4q + r][16 kb + i]
//     as four scalar reads (the +4 of the stride puts the four lane groups on different banks).  No second, transposed copy.
//   * A wave owns 16 frames of the block's tile of 16 WAVES frames and computes transposed, D[unit][frame]: the accumulator
//     block of layer l (lane (frame i, q) holds units 16 jb + 4q + r) is, activated, the B operand of k-block jb of layer l + 1
//     (k slot q of MFMA r <-> unit 16 jb + 4q + r).  The forward is recomputed per tile and its activations stay in registers.
//   * delta of the last layer = grad_out (the last layer is linear); delta_{l-1} = (W_l^T delta_l) * act'(z_{l-1}), on the
//     matrix cores from the same registers; grad_f = W_0^T delta_0.
//   * dW_l[j][k] = sum_f delta_l[j][f] a_l[k][f] needs frames as the K dimension, i.e. frames in the k slots: delta_l and a_l
//     of the whole tile go through LDS ([unit][frame], row stride T + 4: conflict-free both ways), and every 16x16 block of
//     dW_l (plus one block per 16 units for db_l: B = 1) belongs to ONE wave of the block, which accumulates it over all of
//     the block's tiles in registers.  The block's row of partial sums is written once at the end, every element by one
//     lane: no atomics, and the same N gives the same grid, the same tiles per block and the same sums, bit for bit.
//   * Frames past N recompute frame N - 1 with a zero grad_out row: zero deltas, no contribution.  Units padded to 16 have
//     zero weights and biases, so their deltas are zero and they reach neither grad_f nor a stored dW element.
//
// Preamble (generated from the plan, molann_host_jit.inc: jit_source_chain_bwd): NL, ACT, WAVES, DIMS, KP / JP / WOFF (the
// fp32 copy), GOFF / N_PARAMS (the gradient buffer: dW[J][K] then db[J] per layer).
#include "molann_math.h"

using namespace molann;

typedef float f32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float act1(float v) {
    if constexpr (ACT == 0) return act_tanh(v);
    else if constexpr (ACT == 2) return act_sigmoid(v);
    else if constexpr (ACT == 3) return v;
    else return apply_activation(ACT, v);
}

constexpr int T = 16 * WAVES;                        // frames per block tile
constexpr int TSTR = T + 4;                          // [unit][frame] tile rows
constexpr bool NEED_Z = ACT == 5;                    // SiLU: the derivative needs the pre-activation; the others get it from h
constexpr int UB(int l) { return JP[l] / 16; }       // 16-unit blocks of layer l's output
constexpr int KB(int l) { return KP[l] / 16; }       // 16-unit blocks of layer l's input
constexpr int WSTR(int l) { return KP[l] + 4; }
constexpr int LW_OFF(int l) { int s = 0; for (int i = 0; i < l; ++i) s += JP[i] * WSTR(i) + JP[i]; return s; }
constexpr int LB_OFF(int l) { return LW_OFF(l) + JP[l] * WSTR(l); }
constexpr int W_FLOATS = LW_OFF(NL);
constexpr int tile_rows() { int m = 0; for (int l = 0; l < NL; ++l) m = JP[l] + KP[l] > m ? JP[l] + KP[l] : m; return m; }
constexpr int LDS_FLOATS = W_FLOATS + tile_rows() * TSTR;
constexpr int HO(int l) { int s = 0; for (int i = 0; i < l; ++i) s += UB(i); return s; }   // hidden layer l's blocks in H / Z
constexpr int NH = NL > 1 ? HO(NL - 1) : 1;
constexpr int NPAIR(int l) { return UB(l) * (KB(l) + 1); }                               // dW blocks + db blocks of layer l
constexpr int MP(int l) { return (NPAIR(l) + WAVES - 1) / WAVES; }                         // ... per wave
constexpr int GO(int l) { int s = 0; for (int i = 0; i < l; ++i) s += MP(i); return s; }
constexpr int NG = GO(NL);
constexpr int maxub() { int m = 1; for (int l = 0; l < NL; ++l) m = UB(l) > m ? UB(l) : m; return m; }
constexpr int MAXUB = maxub();
static_assert(LDS_FLOATS * 4 <= 163840, "weights + tile exceed the CU's LDS");

template <int I> struct Ic { static constexpr int value = I; };
template <int I, int N, typename F>
__device__ __forceinline__ void sfor(F&& f) {
    if constexpr (I < N) { f(Ic<I>{}); sfor<I + 1, N>(f); }
}
template <int I, int N, typename F>
__device__ __forceinline__ void sfor_down(F&& f) {   // I = N - 1 .. 0
    if constexpr (N > 0) { f(Ic<N - 1>{}); sfor_down<I, N - 1>(f); }
}

__device__ __forceinline__ f32x4 mma4(const f32x4& a, const f32x4& b, f32x4 acc) {
#pragma unroll
    for (int r = 0; r < 4; ++r) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r], b[r], acc, 0, 0, 0);
    return acc;
}

extern "C" __global__ __launch_bounds__(64 * WAVES) void molann_chain_bwd(const float* __restrict__ feat, const float* __restrict__ gout,
                                                                          const float* __restrict__ wnat, float* __restrict__ gfeat,
                                                                          float* __restrict__ gparams /* [gridDim.x][N_PARAMS] */, long n_frames) {
    __shared__ __attribute__((aligned(16))) float lds[LDS_FLOATS];
    float* TD = lds + W_FLOATS;                        // delta_l [JP][TSTR], then a_l [KP][TSTR]
    const int lane = threadIdx.x & 63, i16 = lane & 15, q4 = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const bool want_gp = gparams != nullptr, want_gf = gfeat != nullptr;
    constexpr int D0 = DIMS[0], OUTC = DIMS[NL];
    const long n_tiles = (n_frames + T - 1) / T;
    if ((long)blockIdx.x >= n_tiles) return;

    // ---- the weight copy -> LDS (row stride Kp + 4), once ----------------------------------------------------------------
    sfor<0, NL>([&](auto lc) {
        constexpr int l = decltype(lc)::value;
        constexpr int q = KP[l] / 4;
        for (int e = threadIdx.x; e < JP[l] * q; e += 64 * WAVES) {
            const int j = e / q, k4 = e - j * q;
            *(f32x4*)(lds + LW_OFF(l) + j * WSTR(l) + 4 * k4) = *(const f32x4*)(wnat + WOFF[l] + (long)j * KP[l] + 4 * k4);
        }
        for (int j = threadIdx.x; j < JP[l]; j += 64 * WAVES) lds[LB_OFF(l) + j] = wnat[WOFF[l] + (long)JP[l] * KP[l] + j];
    });
    __syncthreads();

    f32x4 GW[NG > 0 ? NG : 1];
#pragma unroll
    for (int m = 0; m < NG; ++m) GW[m] = (f32x4){0.f, 0.f, 0.f, 0.f};

    for (long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const long frame = t * T + 16 * wave + i16;
        const bool live = frame < n_frames;
        const long fl = live ? frame : n_frames - 1;
        // ---- input rows as B operands: lane (frame, q) holds k = 16 kb + 4q + r -------------------------------------------
        f32x4 X[KB(0)];
        {
            const float* row = feat + fl * D0;
#pragma unroll
            for (int kb = 0; kb < KB(0); ++kb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int k = 16 * kb + 4 * q4 + r;
                    X[kb][r] = k < D0 ? row[k] : 0.f;
                }
        }
        // ---- forward of the hidden layers (the last layer's output is not needed) ------------------------------------------
        f32x4 H[NH];
        f32x4 Z[NEED_Z ? NH : 1];
        sfor<0, NL - 1>([&](auto lc) {
            constexpr int l = decltype(lc)::value;
            const float* W = lds + LW_OFF(l);
            f32x4 acc[UB(l)];
#pragma unroll
            for (int jb = 0; jb < UB(l); ++jb) acc[jb] = *(const f32x4*)(lds + LB_OFF(l) + 16 * jb + 4 * q4);
#pragma unroll
            for (int kb = 0; kb < KB(l); ++kb) {
                f32x4 b;
                if constexpr (l == 0) b = X[kb];
                else b = H[HO(l - 1) + kb];
#pragma unroll
                for (int jb = 0; jb < UB(l); ++jb)
                    acc[jb] = mma4(*(const f32x4*)(W + (16 * jb + i16) * WSTR(l) + 16 * kb + 4 * q4), b, acc[jb]);
            }
#pragma unroll
            for (int jb = 0; jb < UB(l); ++jb) {
                if constexpr (NEED_Z) Z[HO(l) + jb] = acc[jb];
                H[HO(l) + jb] = (f32x4){act1(acc[jb][0]), act1(acc[jb][1]), act1(acc[jb][2]), act1(acc[jb][3])};
            }
        });
        // ---- delta of the last layer: grad_out (zero past N and past OUT) ------------------------------------------------
        f32x4 D[MAXUB];
        {
            const float* grow = gout + fl * OUTC;
#pragma unroll
            for (int jb = 0; jb < UB(NL - 1); ++jb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int u = 16 * jb + 4 * q4 + r;
                    D[jb][r] = (live && u < OUTC) ? grow[u] : 0.f;
                }
        }
        // ---- backward, last layer first -----------------------------------------------------------------------------------
        sfor_down<0, NL>([&](auto lc) {
            constexpr int l = decltype(lc)::value;
            if (want_gp) {
                // delta_l and a_l of the whole tile -> LDS [unit][frame]
                float* TA = TD + JP[l] * TSTR;
                const int col = 16 * wave + i16;
#pragma unroll
                for (int jb = 0; jb < UB(l); ++jb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) TD[(16 * jb + 4 * q4 + r) * TSTR + col] = D[jb][r];
#pragma unroll
                for (int kb = 0; kb < KB(l); ++kb) {
                    f32x4 a;
                    if constexpr (l == 0) a = X[kb];
                    else a = H[HO(l - 1) + kb];
#pragma unroll
                    for (int r = 0; r < 4; ++r) TA[(16 * kb + 4 * q4 + r) * TSTR + col] = a[r];
                }
                __syncthreads();
                // this wave's blocks of dW_l / db_l: block p = jb (KB + 1) + kb, p = wave + WAVES m; frames are the k's
#pragma unroll 1
                for (int s = 0; s < T / 4; ++s) {
#pragma unroll
                    for (int m = 0; m < MP(l); ++m) {
                        const int p = wave + WAVES * m;
                        if (p < NPAIR(l)) {
                            const int jb = p / (KB(l) + 1), kb = p - jb * (KB(l) + 1);
                            const float a = TD[(16 * jb + i16) * TSTR + 4 * s + q4];
                            const float b = kb < KB(l) ? TA[(16 * kb + i16) * TSTR + 4 * s + q4] : 1.f;
                            GW[GO(l) + m] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, GW[GO(l) + m], 0, 0, 0);
                        }
                    }
                }
                __syncthreads();   // the tile is read by every wave before the next layer (or tile) overwrites it
            }
            if (l > 0 || want_gf) {
                // P[k][f] = sum_j W_l[j][k] delta_l[j][f]
                const float* W = lds + LW_OFF(l);
                f32x4 P[KB(l)];
#pragma unroll
                for (int kb = 0; kb < KB(l); ++kb) P[kb] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int jb = 0; jb < UB(l); ++jb)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float* wr = W + (16 * jb + 4 * q4 + r) * WSTR(l) + i16;
#pragma unroll
                        for (int kb = 0; kb < KB(l); ++kb) P[kb] = __builtin_amdgcn_mfma_f32_16x16x4f32(wr[16 * kb], D[jb][r], P[kb], 0, 0, 0);
                    }
                if constexpr (l > 0) {
#pragma unroll
                    for (int kb = 0; kb < KB(l); ++kb)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const float h = H[HO(l - 1) + kb][r];
                            float z = h;                               // ReLU / LeakyReLU: h > 0 iff z > 0
                            if constexpr (NEED_Z) z = Z[HO(l - 1) + kb][r];
                            D[kb][r] = P[kb][r] * act_derivative(ACT, z, h);
                        }
                } else if (live) {
                    float* grow = gfeat + frame * D0;
#pragma unroll
                    for (int kb = 0; kb < KB(0); ++kb)
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int k = 16 * kb + 4 * q4 + r;
                            if (k < D0) grow[k] = P[kb][r];
                        }
                }
            }
        });
    }
    if (want_gp) {
        // ---- this block's row of partial sums: lane (i, q) of block (jb, kb) holds dW[16 jb + 4q + r][16 kb + i] ----------
        float* row = gparams + (long)blockIdx.x * N_PARAMS;
        sfor<0, NL>([&](auto lc) {
            constexpr int l = decltype(lc)::value;
            constexpr int K = DIMS[l], J = DIMS[l + 1];
#pragma unroll
            for (int m = 0; m < MP(l); ++m) {
                const int p = wave + WAVES * m;
                if (p < NPAIR(l)) {
                    const int jb = p / (KB(l) + 1), kb = p - jb * (KB(l) + 1);
                    const int k = 16 * kb + i16;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int j = 16 * jb + 4 * q4 + r;
                        if (j >= J) continue;
                        if (kb < KB(l)) {
                            if (k < K) row[GOFF[l] + j * K + k] = GW[GO(l) + m][r];
                        } else if (i16 == 0) {
                            row[GOFF[l] + J * K + j] = GW[GO(l) + m][r];
                        }
                    }
                }
            }
        });
    }
}
