// molann_mlp_tile.inc - the backward of a narrow MLP (every width <= 32) for ONE 64-frame tile on the fp32 matrix cores, shared by
// molann_mlp_bwd.inc (the MLP's backward as a kernel of its own) and molann_bwd_ring.inc (the one-pass backward).
//
// One wave, a [unit][frame] scratch S in LDS (row stride 68 floats: bank = 4 row + frame, conflict-free operand reads).  Every
// product is a v_mfma_f32_16x16x4_f32 whose B operand is read from the scratch in natural order (lane (q, n): row 4 ks + q,
// frame 16 fb + n), so no fragment needs a permuted copy of the weights:
//
//   forward (hidden layers)   z_l = W_l a_l + b_l          A = W_l  rows,   B = a_l rows      a_{l+1} = act(z_l) -> scratch
//   input gradient            g_l = W_l^T delta_l          A = W_l^T rows,  B = delta_l rows  delta_{l-1} = g_l . act'(a_l), written IN PLACE
//                                                          over a_l (its last reader, dW_l, has run)
//   weight gradient           dW_l += delta_l a_l^T        A = delta_l rows (k = frame), B = a_l rows (k = frame): 16 k-steps add the
//                                                          tile's 64 frames into 16x16 blocks that stay in registers over all tiles
//   bias gradient             db_l += row sums of delta_l  (DPP all-reduce over the 16 frames of a lane row, 4 frame blocks added first)
//
// The loops over the layers are compile-time recursions (static_for).  Weight fragments: one register per lane each, or
// (FRAG_LDS) one float per lane in an LDS image read where used.
//
// Needs from the preamble: NL, ACT, DIMS, KP / JP / WOFF (the fp32 weight copy: Wp[Jp][Kp] then bias[Jp] per layer), GOFF / N_PARAMS
// (gradient buffer: dW[J][K] then db[J] per layer), FRAG_LDS; act1() from the including file.

#ifndef MOLANN_RING_INC   // compiled without molann_ring.inc (molann_mlp_bwd.inc): the few things the tile code takes from there
#include "molann_math.h"
using namespace molann;
typedef float f32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float act1(float v) {
    if constexpr (ACT == 0) return act_tanh(v);
    else if constexpr (ACT == 2) return act_sigmoid(v);
    else if constexpr (ACT == 3) return v;
    else return apply_activation(ACT, v);
}
#endif

constexpr int SSTR = 68;                        // [unit][frame] scratch: bank = 4 row + frame
constexpr int MAXB = 2, MAXS = 8;               // 16-unit blocks / 4-unit k-steps per layer (width <= 32)
constexpr int NLM = NL > 0 ? NL : 1;
constexpr int pad4(int v) { return (v + 3) & ~3; }
constexpr int blocks16(int v) { return (v + 15) >> 4; }
constexpr bool NEED_Z = ACT == 5;               // SiLU: the derivative needs the pre-activation as well
constexpr int act_row(int l) { int r = 0; for (int i = 0; i < l; ++i) r += pad4(DIMS[i]); return r; }
constexpr int z_row(int l) { int r = act_row(NL); for (int i = 0; i < l; ++i) r += pad4(DIMS[i + 1]); return r; }
constexpr int Z_END = NL > 0 ? (NEED_Z ? z_row(NL - 1) : act_row(NL)) : 0;
constexpr int d_row(int l) { return l == NL - 1 ? Z_END : act_row(l + 1); }   // a hidden layer's delta overwrites its output in place
constexpr int n_rows() {
    if (NL == 0) return 0;
    int m = Z_END + pad4(DIMS[NL]);
    for (int l = 0; l < NL; ++l) {
        const int a = act_row(l) + 16 * blocks16(DIMS[l]), d = d_row(l) + 16 * blocks16(DIMS[l + 1]);
        m = a > m ? a : m;
        m = d > m ? d : m;
    }
    return m;
}
constexpr int N_ROWS = n_rows();
constexpr int GF_ROW = 0;                       // dL/d features overwrites the features once dW_0 has read them

// Operand fragments of the weights: per lane one register each - or, FRAG_LDS (MLPs whose fragments do not fit the 256 registers
// beside the per-lane state: three layers of 32), one float per lane in a block-wide LDS image at IMG_OFF, read where used.
// Compact numbering of the fragments that exist for this plan's shapes: forward A (hidden layers), backward A, bias rows.
struct FragIds { int fwd[NLM][MAXB][MAXS], bwd[NLM][MAXB][MAXS], bias[NLM][MAXB]; int count; };
constexpr FragIds frag_ids() {
    FragIds t = {};
    int n = 0;
    for (int l = 0; l < NL; ++l)
        for (int b = 0; b < MAXB; ++b) {
            for (int s = 0; s < MAXS; ++s) {
                t.fwd[l][b][s] = (l + 1 < NL && 16 * b < DIMS[l + 1] && 4 * s < DIMS[l]) ? n++ : -1;
                t.bwd[l][b][s] = (16 * b < DIMS[l] && 4 * s < DIMS[l + 1]) ? n++ : -1;
            }
            t.bias[l][b] = (l + 1 < NL && 16 * b < DIMS[l + 1]) ? n : -1;
            if (t.bias[l][b] >= 0) n += 4;
        }
    t.count = n;
    return t;
}
constexpr FragIds FRAG = frag_ids();

// compile-time loop: f(IC<I>{}) for I = 0 .. N-1, every iteration its own instantiation (a `#pragma unroll` over the layers is
// only a request, and a loop the optimizer leaves rolled turns the per-layer register arrays into scratch memory)
template <int I> struct IC { static constexpr int value = I; };
template <int I, int N, typename F>
__device__ __forceinline__ void static_for(F&& f) {
    if constexpr (I < N) { f(IC<I>{}); static_for<I + 1, N>(f); }
}

template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
    return __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, v), CTRL, 0xf, 0xf, true));
}
__device__ __forceinline__ float row_sum16(float v) { // sum over the 16 lanes of a row, result in every lane of the row
    v += dpp_mov<0xB1>(v);
    v += dpp_mov<0x4E>(v);
    v += dpp_mov<0x141>(v);
    v += dpp_mov<0x140>(v);
    return v;
}


// The weight fragments of one wave and its parameter sums
struct MlpTileState {
    float afwd[NLM][MAXB][MAXS], abwd[NLM][MAXB][MAXS];
    f32x4 bias[NLM][MAXB], wacc[NLM][MAXB][MAXB], bacc[NLM][MAXB];
};

// fragments from the plan's fp32 weight copy (registers, or the LDS image `img`: every wave writes the whole image itself - the
// same values - so no hand-off between waves is needed), parameter sums cleared
__device__ __forceinline__ void mlp_tile_init(MlpTileState& st, const float* __restrict__ wnat, float* img, int lane) {
    const int q = lane >> 4, n16 = lane & 15;
    float (&afwd)[NLM][MAXB][MAXS] = st.afwd;
    float (&abwd)[NLM][MAXB][MAXS] = st.abwd;
    f32x4 (&bias)[NLM][MAXB] = st.bias;
    f32x4 (&wacc)[NLM][MAXB][MAXB] = st.wacc;
    f32x4 (&bacc)[NLM][MAXB] = st.bacc;
    if constexpr (NL > 0) {
#pragma unroll
        for (int l = 0; l < NL; ++l) {
            const float* W = wnat + WOFF[l];
#pragma unroll
            for (int b = 0; b < MAXB; ++b) {
#pragma unroll
                for (int s = 0; s < MAXS; ++s) {
                    if (l + 1 < NL && 16 * b < DIMS[l + 1] && 4 * s < DIMS[l]) {
                        const float v = W[(16 * b + n16) * KP[l] + 4 * s + q];
                        if constexpr (FRAG_LDS) img[FRAG.fwd[l][b][s] * 64 + lane] = v; else afwd[l][b][s] = v;
                    }
                    if (16 * b < DIMS[l] && 4 * s < DIMS[l + 1]) {
                        const float v = W[(4 * s + q) * KP[l] + 16 * b + n16];
                        if constexpr (FRAG_LDS) img[FRAG.bwd[l][b][s] * 64 + lane] = v; else abwd[l][b][s] = v;
                    }
                }
                if (l + 1 < NL && 16 * b < DIMS[l + 1])
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float v = W[JP[l] * KP[l] + 16 * b + 4 * q + r];
                        if constexpr (FRAG_LDS) img[(FRAG.bias[l][b] + r) * 64 + lane] = v; else bias[l][b][r] = v;
                    }
                bacc[l][b] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kb = 0; kb < MAXB; ++kb) wacc[l][b][kb] = (f32x4){0.f, 0.f, 0.f, 0.f};
            }
        }
    }
}

// One tile: f[D0] = this lane's input row, gv[OUTC] = its grad_out row (zeros for a lane past the end).  Adds the tile into the
// parameter sums (want_gp) and leaves dL/d input in the scratch rows GF_ROW .. (want_gf; the caller reads S[(GF_ROW + k) * SSTR + lane]).
// WITH_VALUES builds (molann_value_and_vjp_f32): yrow != nullptr -> the tile's OUTPUT rows y = W a + b of the last layer are
// stored there as well (yrow[frame * OUTC + unit], frames < nfr), from the activations the backward has in its scratch anyway.
__device__ __forceinline__ void mlp_tile_backward(MlpTileState& st, float* S, const float* img, int lane, const float (&f)[DIMS[0]],
                                                  const float (&gv)[DIMS[NL > 0 ? NL : 0]], bool want_gp, bool want_gx,
                                                  const float* __restrict__ wnat = nullptr, float* __restrict__ yrow = nullptr, int nfr = 0) {
    const int q = lane >> 4, n16 = lane & 15;
    constexpr int D0 = DIMS[0], OUTC = DIMS[NL > 0 ? NL : 0];
    float (&afwd)[NLM][MAXB][MAXS] = st.afwd;
    float (&abwd)[NLM][MAXB][MAXS] = st.abwd;
    f32x4 (&bias)[NLM][MAXB] = st.bias;
    f32x4 (&wacc)[NLM][MAXB][MAXB] = st.wacc;
    f32x4 (&bacc)[NLM][MAXB] = st.bacc;
    #pragma unroll
    for (int c = 0; c < D0; ++c) S[(act_row(0) + c) * SSTR + lane] = f[c];
#pragma unroll
    for (int c = 0; c < OUTC; ++c) S[(d_row(NL - 1) + c) * SSTR + lane] = gv[c];
    __builtin_amdgcn_wave_barrier();
    // forward through the hidden layers
    static_for<0, (NL > 0 ? NL - 1 : 0)>([&](auto lc) {
        constexpr int l = decltype(lc)::value;
        const int K = DIMS[l], J = DIMS[l + 1];
        f32x4 D[MAXB][4];
#pragma unroll
        for (int jb = 0; jb < MAXB; ++jb)
#pragma unroll
            for (int fb = 0; fb < 4; ++fb) {
                if constexpr (FRAG_LDS) {
                    if (16 * jb < J)
#pragma unroll
                        for (int r = 0; r < 4; ++r) D[jb][fb][r] = img[(FRAG.bias[l][jb] + r) * 64 + lane];
                } else {
                    D[jb][fb] = bias[l][jb];
                }
            }
#pragma unroll
        for (int ks = 0; ks < MAXS; ++ks) {
            if (4 * ks < K) {
                float B[4];
#pragma unroll
                for (int fb = 0; fb < 4; ++fb) B[fb] = S[(act_row(l) + 4 * ks + q) * SSTR + 16 * fb + n16];
#pragma unroll
                for (int jb = 0; jb < MAXB; ++jb)
                    if (16 * jb < J)
#pragma unroll
                        for (int fb = 0; fb < 4; ++fb) D[jb][fb] = __builtin_amdgcn_mfma_f32_16x16x4f32(FRAG_LDS ? img[FRAG.fwd[l][jb][ks] * 64 + lane] : afwd[l][jb][ks], B[fb], D[jb][fb], 0, 0, 0);
            }
        }
#pragma unroll
        for (int jb = 0; jb < MAXB; ++jb)
            if (16 * jb < J)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * jb + 4 * q + r;
                    if (row < pad4(J)) {
#pragma unroll
                        for (int fb = 0; fb < 4; ++fb) {
                            const float z = D[jb][fb][r];
                            S[(act_row(l + 1) + row) * SSTR + 16 * fb + n16] = row < J ? act1(z) : 0.f;
                            if constexpr (NEED_Z) S[(z_row(l) + row) * SSTR + 16 * fb + n16] = z;
                        }
                    }
                }
        __builtin_amdgcn_wave_barrier();
    });
    if constexpr (WITH_VALUES) {
        if (yrow) {   // the last layer's forward, fragments straight from the fp32 weight copy (this build serves small batches)
            constexpr int l = NL - 1;
            const int K = DIMS[l], J = DIMS[l + 1];
            const float* W = wnat + WOFF[l];
#pragma unroll
            for (int jb = 0; jb < MAXB; ++jb) {
                if (16 * jb < J) {
                    f32x4 D[4];
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float b = W[JP[l] * KP[l] + 16 * jb + 4 * q + r];
#pragma unroll
                        for (int fb = 0; fb < 4; ++fb) D[fb][r] = b;
                    }
#pragma unroll
                    for (int ks = 0; ks < MAXS; ++ks) {
                        if (4 * ks < K) {
                            const float A = W[(16 * jb + n16) * KP[l] + 4 * ks + q];
#pragma unroll
                            for (int fb = 0; fb < 4; ++fb)
                                D[fb] = __builtin_amdgcn_mfma_f32_16x16x4f32(A, S[(act_row(l) + 4 * ks + q) * SSTR + 16 * fb + n16], D[fb], 0, 0, 0);
                        }
                    }
#pragma unroll
                    for (int fb = 0; fb < 4; ++fb) {
                        const int frame = 16 * fb + n16;
#pragma unroll
                        for (int r = 0; r < 4; ++r) {
                            const int unit = 16 * jb + 4 * q + r;
                            if (frame < nfr && unit < J) yrow[frame * J + unit] = D[fb][r];
                        }
                    }
                }
            }
        }
    }
    // backward, last layer first
    f32x4 dsum[MAXB]; // the current layer's delta summed over the four frame blocks, as the matrix cores lay it out: lane (q, n)
                      // register r = unit 16 jb + 4 q + r, frames n, 16 + n, 32 + n, 48 + n (the bias gradient's row sums start from it)
#pragma unroll
    for (int jb = 0; jb < MAXB; ++jb)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * jb + 4 * q + r;
            float sum = 0.f;
            if (16 * jb < OUTC && row < pad4(OUTC))
#pragma unroll
                for (int fb = 0; fb < 4; ++fb) sum += S[(d_row(NL - 1) + row) * SSTR + 16 * fb + n16];
            dsum[jb][r] = sum;
        }
    static_for<0, NL>([&](auto lc) {
        constexpr int l = NL - 1 - decltype(lc)::value;
        const int K = DIMS[l], J = DIMS[l + 1];
        if (want_gp) {
#pragma unroll
            for (int ks = 0; ks < 16; ++ks) {
                float av[MAXB], bv[MAXB];
#pragma unroll
                for (int jb = 0; jb < MAXB; ++jb)
                    if (16 * jb < J) av[jb] = S[(d_row(l) + 16 * jb + n16) * SSTR + 4 * ks + q];
#pragma unroll
                for (int kb = 0; kb < MAXB; ++kb)
                    if (16 * kb < K) bv[kb] = S[(act_row(l) + 16 * kb + n16) * SSTR + 4 * ks + q];
#pragma unroll
                for (int jb = 0; jb < MAXB; ++jb)
                    if (16 * jb < J)
#pragma unroll
                        for (int kb = 0; kb < MAXB; ++kb)
                            if (16 * kb < K) wacc[l][jb][kb] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[jb], bv[kb], wacc[l][jb][kb], 0, 0, 0);
            }
#pragma unroll
            for (int jb = 0; jb < MAXB; ++jb)
                if (16 * jb < J)
#pragma unroll
                    for (int r = 0; r < 4; ++r) bacc[l][jb][r] += row_sum16(dsum[jb][r]);
        }
        if (l > 0 || want_gx) {
            f32x4 G[MAXB][4];
#pragma unroll
            for (int kb = 0; kb < MAXB; ++kb)
#pragma unroll
                for (int fb = 0; fb < 4; ++fb) G[kb][fb] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int js = 0; js < MAXS; ++js) {
                if (4 * js < J) {
                    float B[4];
#pragma unroll
                    for (int fb = 0; fb < 4; ++fb) B[fb] = S[(d_row(l) + 4 * js + q) * SSTR + 16 * fb + n16];
#pragma unroll
                    for (int kb = 0; kb < MAXB; ++kb)
                        if (16 * kb < K)
#pragma unroll
                            for (int fb = 0; fb < 4; ++fb) G[kb][fb] = __builtin_amdgcn_mfma_f32_16x16x4f32(FRAG_LDS ? img[FRAG.bwd[l][kb][js] * 64 + lane] : abwd[l][kb][js], B[fb], G[kb][fb], 0, 0, 0);
                }
            }
            __builtin_amdgcn_wave_barrier();
#pragma unroll
            for (int kb = 0; kb < MAXB; ++kb)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * kb + 4 * q + r;
                    float sum = 0.f;
                    if (16 * kb < K && row < pad4(K)) {
#pragma unroll
                        for (int fb = 0; fb < 4; ++fb) {
                            if (l > 0) {
                                const float h = S[(act_row(l) + row) * SSTR + 16 * fb + n16];
                                const float z = NEED_Z ? S[(z_row(l > 0 ? l - 1 : 0) + row) * SSTR + 16 * fb + n16] : h; // ReLU / LeakyReLU: sign(z) = sign(h)
                                const float d = row < K ? G[kb][fb][r] * act_derivative(ACT, z, h) : 0.f;
                                S[(d_row(l > 0 ? l - 1 : 0) + row) * SSTR + 16 * fb + n16] = d;
                                sum += d;
                            } else {
                                // rows K .. pad4(K) are the next tile's K-padding: G is 0 * delta there, NaN for a frame that is not finite
                                S[(GF_ROW + row) * SSTR + 16 * fb + n16] = row < K ? G[kb][fb][r] : 0.f;
                            }
                        }
                    }
                    dsum[kb][r] = sum;
                }
            __builtin_amdgcn_wave_barrier();
        }
    });
}

// the wave's parameter sums -> its scratch in gradient-buffer order (dW[J][K] then db[J], layer after layer)
__device__ __forceinline__ void mlp_tile_store_sums(const MlpTileState& st, float* S, int lane) {
    const int q = lane >> 4, n16 = lane & 15;
    const f32x4 (&wacc)[NLM][MAXB][MAXB] = st.wacc;
    const f32x4 (&bacc)[NLM][MAXB] = st.bacc;
    #pragma unroll
    for (int l = 0; l < NL; ++l) {
        const int K = DIMS[l], J = DIMS[l + 1];
#pragma unroll
        for (int jb = 0; jb < MAXB; ++jb) {
            if (16 * jb < J) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int j = 16 * jb + 4 * q + r;
#pragma unroll
                    for (int kb = 0; kb < MAXB; ++kb) {
                        const int kk = 16 * kb + n16;
                        if (16 * kb < K && j < J && kk < K) S[GOFF[l] + j * K + kk] = wacc[l][jb][kb][r];
                    }
                    if (n16 == 0 && j < J) S[GOFF[l] + J * K + j] = bacc[l][jb][r];
                }
            }
        }
    }
}
