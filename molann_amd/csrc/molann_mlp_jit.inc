// molann_mlp_jit.inc - wide MLP (C5 class: [341, 512, 256, 16], bf16 or fp32) SPECIALISED for one plan.
//
// Replaces mlp_mfma_kernel<bf16> (molann_kernels.hip), which gives every wave 16 frames and streams all the
// weights from L2 for each of them (L2-bound at a few percent of the bf16 MFMA rate).  Here
//   * the MLP is computed transposed, D[unit][frame] = W . X (v_mfma_f32_16x16x32_bf16: A = 16 units x 32 k of
//     W, B = 32 k x 16 frames), and a wave owns 16*FB frames: one A fragment read from LDS feeds FB MFMAs;
//   * activations never leave registers.  The accumulator layout of a 16x16 block (lane (frame = l&15,
//     q = l>>4) holds units 4q..4q+3) IS a B-operand layout for the next layer once the next layer's k order
//     is permuted to match: k slot s of lane group q in k-step ks <-> unit 16(2ks + (s>>2)) + 4q + (s&3).
//     The weight fragments are packed with that permutation (pack_chain_kernel), so act() + bf16 pack is all
//     that happens between two layers;
//   * layers are taken in pairs (P, C): P's outputs are produced 32 units at a time (from the pair's full
//     input, held as B operands in registers) and each chunk is at once one k-step of C, whose accumulators
//     for ALL its units stay live.  C's output is the next pair's input.  A last layer without partner is a
//     P whose chunks go to memory;
//   * the weights form one stream of 1-KiB fragments in exactly the order the MFMAs consume them.  The four
//     waves of a block walk it together through two LDS slabs filled by LDS-DMA (global_load_lds, one
//     fragment per instruction): one barrier per slab, the next slab in flight while this one is consumed.
//
// BF16 = false builds the same kernel on the fp32 MFMA (v_mfma_f32_16x16x4_f32, exact fp32 products and sums): a
// 1-KiB fragment is then 16 units x 16 k (lane (i, q) holds W[16 jb + i][16 g + 4q .. +3], four MFMAs per fragment
// and frame block), a chunk is ONE 16-unit block, and an accumulator block is the next layer's B operand as it is.
//
// RESIDENT (round 3): an MLP whose whole weight stream fits the CU's LDS beside nothing else (fp32 heads up to about
// [d, 128, 128, 8]: C4's [85, 128, 64, 8] is 84 KB, [6, 64, 64, 8] 24 KB) does not stream at all: every block copies the
// stream into LDS once, one barrier, and the chunks then index the resident image - no wait, no barrier and no DMA inside
// the loop over the tiles - with eight waves per block (two per SIMD: one wave's dependent MFMA chains and activations
// run under the other's).  Streaming, [6, 64, 64, 8] met five barriers per 256 frames and ran at 58 TFLOP/s.
//
// Preamble (generated from the plan): NL, DIMS[NL+1], ACT, FB (16-frame blocks per wave), BF16, RESIDENT, WAVES, NSLAB (slab buffers,
// chain_nslab in molann_host_jit.inc).
// Compiled a second way (round 3): behind molann_ring.inc inside molann_lane_jit.inc with MOLANN_CHAIN_CORE_ONLY defined, where
// the chain's arithmetic (run_pair on an LDS-resident stream) is the MLP stage of the lane kernel's consumer waves (WIDE_MLP).
#ifndef MOLANN_RING_INC
#include "molann_math.h"

using namespace molann;

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;
#endif
typedef short bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4u __attribute__((ext_vector_type(4), aligned(4)));

#ifdef MOLANN_CHAIN_CORE_ONLY
constexpr int FB = 4;                 // the lane kernel's tile: four blocks of 16 frames
constexpr bool BF16 = false, RESIDENT = true;
constexpr int WAVES = NCONS, NSLAB = 1;
constexpr int CHAIN_DIAG = 0;
#endif
constexpr int CB = BF16 ? 2 : 1;                                     // 16-unit blocks per chunk = per k-step of the next layer
constexpr int KW = BF16 ? 32 : 16;                                   // k's per fragment
constexpr int cdiv(int a, int b) { return (a + b - 1) / b; }
constexpr int UB(int l) { return cdiv(DIMS[l + 1], 16); }           // 16-unit blocks of layer l's output
constexpr int UBP(int l) { return cdiv(UB(l), CB) * CB; }           // ... padded to whole chunks
constexpr int KS(int l) { return l == 0 ? cdiv(DIMS[0], KW) : UBP(l - 1) / CB; } // k-steps (fragments per unit block) of layer l
constexpr int NPAIR = (NL + 1) / 2;
constexpr bool HAS_C(int p) { return 2 * p + 1 < NL; }
constexpr int NCHUNK(int p) { return UBP(2 * p) / CB; }
constexpr int SLAB_FRAGS(int p) { return CB * KS(2 * p) + (HAS_C(p) ? UB(2 * p + 1) : 0); }
constexpr int slab_max() {
    int m = 0;
    for (int p = 0; p < NPAIR; ++p) m = SLAB_FRAGS(p) > m ? SLAB_FRAGS(p) : m;
    return m;
}
constexpr int SLAB_BYTES = slab_max() * 1024;
constexpr long stream_bytes() {
    long s = 0;
    for (int p = 0; p < NPAIR; ++p) s += (long)NCHUNK(p) * SLAB_FRAGS(p) * 1024;
    return s;
}
constexpr int BIAS_OFF(int l) {
    int s = 0;
    for (int i = 0; i < l; ++i) s += 16 * UBP(i);
    return s;
}
constexpr int TILE_FRAMES = WAVES * 16 * FB;
constexpr long PAIR_BASE(int p) {     // stream offset of pair p's first slab
    long s = 0;
    for (int i = 0; i < p; ++i) s += (long)NCHUNK(i) * SLAB_FRAGS(i) * 1024;
    return s;
}
// streaming: a ring of NSLAB slab buffers, NSLAB - 1 slabs in flight ahead of the one being consumed (round 3: with two
// buffers the DMA of slab g + 1 had only slab g's MFMAs to hide under - C5's chunk is 0.9 us of MFMA, a fragment's trip from L2
// 2-3 us - and the kernel ran at the DMA's latency: 20 % of the bf16 MFMA rate).  NSLAB comes from the preamble: as many buffers,
// up to four, as fit 160 KB less 2 KB.
static_assert(RESIDENT ? NSLAB == 1 : (NSLAB >= 2 && NSLAB <= 4 && (long)NSLAB * SLAB_BYTES <= 160 * 1024 - 2048), "NSLAB");
constexpr int PD = NSLAB - 1;                                        // prefetch distance, in slabs
constexpr int SLAB_SHARE(int p) { return cdiv(SLAB_FRAGS(p), WAVES); }   // DMA instructions per wave and slab (the same for every wave)
constexpr int share_min() {
    int m = 1 << 20;
    for (int p = 0; p < NPAIR; ++p) m = SLAB_SHARE(p) < m ? SLAB_SHARE(p) : m;
    return m;
}
constexpr int WAIT_NEWER = (PD - 1) * share_min() < 63 ? (PD - 1) * share_min() : 63;   // loads this wave issued for the slabs behind the current one: at least
constexpr int slabs_per_tile() {
    int n = 0;
    for (int p = 0; p < NPAIR; ++p) n += NCHUNK(p);
    return n;
}
constexpr long LDS_BYTES = RESIDENT ? stream_bytes() : (long)NSLAB * SLAB_BYTES;

#ifndef MOLANN_RING_INC
__device__ __forceinline__ float act1(float v) {
    if constexpr (ACT == 0) return act_tanh(v);
    else if constexpr (ACT == 2) return act_sigmoid(v);
    else if constexpr (ACT == 3) return v;
    else return apply_activation(ACT, v);
}
#endif

__device__ __forceinline__ unsigned pack_bf16(float lo, float hi) { // round-to-nearest-even, lo in bits 0..15
    const __bf16 a = (__bf16)lo, b = (__bf16)hi;
    return (unsigned)__builtin_bit_cast(unsigned short, a) | ((unsigned)__builtin_bit_cast(unsigned short, b) << 16);
}

// One 16-byte register quad per lane either way: a weight fragment (A) or the B operand of one k-step.
//   bf16: 8 values, one MFMA 16x16x32;   fp32: 4 values, four MFMAs 16x16x4 (k = 16 g + 4 q + r, r = 0..3)
typedef f32x4 mquad_t;
// NR: fp32 only - how many of the fragment's four MFMAs hold any k below the layer's input width (layer 0's last k-step)
template <int NR = 4>
__device__ __forceinline__ f32x4 mma(const mquad_t& a, const mquad_t& b, f32x4 acc) {
    if constexpr (BF16) {
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), acc, 0, 0, 0);
    } else {
#pragma unroll
        for (int r = 0; r < NR; ++r) acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a[r], b[r], acc, 0, 0, 0);
        return acc;
    }
}
// fp32, layer 0: k = 16 ks + 4 r + q, so MFMA r of k-step ks is live iff 16 ks + 4 r < DIMS[0]
constexpr int live_r(int l, int ks) {
    if (BF16 || l != 0) return 4;
    const int left = DIMS[0] - 16 * ks;
    return left >= 16 ? 4 : (left <= 0 ? 1 : (left + 3) / 4);
}

// CB accumulator blocks (units 4q..4q+3 of each) -> the B operand of one k-step of the next layer
template <bool ACTIVATE>
__device__ __forceinline__ mquad_t to_operand(const f32x4& b0, const f32x4& b1) {
    if constexpr (BF16) {
        float v[8] = {b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
        if constexpr (ACTIVATE) {
#pragma unroll
            for (int i = 0; i < 8; ++i) v[i] = act1(v[i]);
        }
        typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
        const u32x4 u = {pack_bf16(v[0], v[1]), pack_bf16(v[2], v[3]), pack_bf16(v[4], v[5]), pack_bf16(v[6], v[7])};
        return __builtin_bit_cast(mquad_t, u);
    } else {
        if constexpr (ACTIVATE) return (f32x4){act1(b0[0]), act1(b0[1]), act1(b0[2]), act1(b0[3])};
        else return b0;
    }
}

template <int I> struct KsC { static constexpr int value = I; };
template <int I, int N, typename F>
__device__ __forceinline__ void static_for_ks(F&& f) {   // compile-time loop over the k-steps (the live MFMA count is per k-step)
    if constexpr (I < N) { f(KsC<I>{}); static_for_ks<I + 1, N>(f); }
}

struct Ctx {
    const unsigned char* wstream; // fragments, consumption order
    const float* biases;          // fp32, BIAS_OFF(l) + unit
    float* out;
    unsigned char* smem;          // NSLAB slab buffers (streaming) / the whole stream (resident)
    long n_frames, frame0;        // frame0: first frame of this wave in the current tile
    long next_off;                // stream offset of the slab that is prefetched next
    long pf_left;                 // slabs this block has still to request
    int pf_pair, pf_chunk;        // which slab that is (pair, chunk inside the pair)
    int inflight;                 // slabs requested and not yet consumed
    int g;                        // slabs consumed so far by this block (buffer = g mod NSLAB)
    int lane, wave, i16, q4;
    bool more_tiles;              // (resident build: unused)
};

template <int P = 0>
__device__ __forceinline__ int slab_frags_rt(int p) {
    if constexpr (P >= NPAIR) return 0;
    else return p == P ? SLAB_FRAGS(P) : slab_frags_rt<P + 1>(p);
}
template <int P = 0>
__device__ __forceinline__ int nchunk_rt(int p) {
    if constexpr (P >= NPAIR) return 1;
    else return p == P ? NCHUNK(P) : nchunk_rt<P + 1>(p);
}

// request the next slab of the stream (if the block still needs one) into the buffer behind the newest: every wave issues the
// same number of LDS-DMA instructions (its share, padded with repeats of the slab's last fragment), so that the counted wait
// in slab_advance holds for all of them
__device__ __forceinline__ void slab_request(Ctx& cx) {
    if (cx.pf_left <= 0) return;
    const int nf = slab_frags_rt(cx.pf_pair);
    const int share = (nf + WAVES - 1) / WAVES;
    unsigned char* dst = cx.smem + (size_t)((cx.g + cx.inflight) % NSLAB) * SLAB_BYTES;
    const unsigned char* src = cx.wstream + cx.next_off;
    for (int i = 0; i < share; ++i) {
        int f = cx.wave + i * WAVES;
        f = f < nf ? f : nf - 1;
        __builtin_amdgcn_global_load_lds((gptr_t)(src + (size_t)f * 1024 + cx.lane * 16), (lptr_t)(dst + (size_t)f * 1024), 16, 0, 0);
    }
    cx.next_off += (long)nf * 1024;
    if (++cx.pf_chunk == nchunk_rt(cx.pf_pair)) {
        cx.pf_chunk = 0;
        if (++cx.pf_pair == NPAIR) { cx.pf_pair = 0; cx.next_off = 0; }
    }
    cx.pf_left -= 1;
    cx.inflight += 1;
}

// the slab about to be consumed: wait for this wave's share of it (the PD - 1 slabs requested behind it may stay in flight),
// meet the other waves (theirs has landed, and everybody is done with the previous slab), then request the slab PD ahead
// into the buffer the previous one occupied.
// (CHAIN_DIAG, diagnostics build only, timing ablations with wrong results: 2 no DMA behind the prologue and no wait for it,
// 4 no barrier either, 1 input rows loaded for a block's first tile only, 8 one fragment read per chunk instead of all)
__device__ __forceinline__ const unsigned char* slab_advance(Ctx& cx) {
    if constexpr (CHAIN_DIAG & 2) {
        if constexpr (!(CHAIN_DIAG & 4)) __syncthreads();
        const unsigned char* cur = cx.smem + (size_t)(cx.g % NSLAB) * SLAB_BYTES;
        cx.g += 1;
        return cur;
    }
    if (cx.inflight >= PD && PD > 1) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(WAIT_NEWER) : "memory");
    else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const unsigned char* cur = cx.smem + (size_t)(cx.g % NSLAB) * SLAB_BYTES;
    cx.inflight -= 1;
    cx.g += 1;
    slab_request(cx);
    return cur;
}

__device__ __forceinline__ mquad_t lds_frag(const unsigned char* slab, int frag, int lane) {
    if constexpr ((CHAIN_DIAG & 8) != 0) { mquad_t v = *(const mquad_t*)(slab + lane * 16); v[0] += (float)frag; return v; }
    return *(const mquad_t*)(slab + (size_t)frag * 1024 + lane * 16);
}

// accumulator block of the LAST layer -> out[frame][unit]; unit0 = first unit of the block
__device__ __forceinline__ void store_block(const Ctx& cx, const f32x4& acc, int fb, int unit0) {
    constexpr int J = DIMS[NL];
    const long frame = cx.frame0 + 16 * fb + cx.i16;
    const int u = unit0 + 4 * cx.q4;
    if (frame >= cx.n_frames) return;
    float* dst = cx.out + frame * (long)J + u;
    if constexpr (J % 4 == 0) {
        if (u < J) *(f32x4u*)dst = acc;
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (u + r < J) dst[r] = acc[r];
    }
}

template <int P, int KSIN>
__device__ __forceinline__ void run_pair(mquad_t (&bin)[KSIN][FB], Ctx& cx) {
    constexpr int lP = 2 * P, lC = 2 * P + 1;
    constexpr bool hasC = HAS_C(P);
    constexpr bool p_last = (lP == NL - 1), c_last = hasC && (lC == NL - 1);
    constexpr int NCH = NCHUNK(P);
    constexpr int UBC = hasC ? UB(hasC ? lC : 0) : 1;
    constexpr int NF = SLAB_FRAGS(P);
    static_assert(KSIN == KS(lP), "input k-steps");

    f32x4 cacc[UBC][FB];
    if constexpr (hasC) {
#pragma unroll
        for (int jb = 0; jb < UBC; ++jb) {
            const f32x4 b = *(const f32x4*)(cx.biases + BIAS_OFF(hasC ? lC : 0) + 16 * jb + 4 * cx.q4);
#pragma unroll
            for (int fb = 0; fb < FB; ++fb) cacc[jb][fb] = b;
        }
    }
#pragma unroll 1
    for (int c = 0; c < NCH; ++c) { // chunk c: CB unit blocks of layer lP = k-step c of layer lC
        const unsigned char* S;
        if constexpr (RESIDENT) S = cx.smem + PAIR_BASE(P) + (size_t)c * NF * 1024;
        else S = slab_advance(cx);
        f32x4 pacc[CB][FB];
#pragma unroll
        for (int h = 0; h < CB; ++h) {
            const f32x4 b = *(const f32x4*)(cx.biases + BIAS_OFF(lP) + 16 * CB * c + 16 * h + 4 * cx.q4);
#pragma unroll
            for (int fb = 0; fb < FB; ++fb) pacc[h][fb] = b;
        }
        static_for_ks<0, KSIN>([&](auto kc) {
            constexpr int ks = decltype(kc)::value;
#pragma unroll
            for (int h = 0; h < CB; ++h) {
                const mquad_t a = lds_frag(S, CB * ks + h, cx.lane);
#pragma unroll
                for (int fb = 0; fb < FB; ++fb) pacc[h][fb] = mma<live_r(lP, ks)>(a, bin[ks][fb], pacc[h][fb]);
            }
        });
        // (Measured and dropped, round 3: the biases added behind the MFMAs instead of starting the accumulators, and a
        // sched_group_barrier pipeline keeping six fragment reads in flight: 548 -> 522-528 TFLOP/s.  The timing ablations
        // (CHAIN_DIAG) say where a C5 tile's time goes: 0.27 ms of MFMA per 1 M frames, 0.38 of activations / packing /
        // accumulator reads that one wave per SIMD does not overlap with them, 0.32 of input rows loaded at the tile's
        // start with nothing to run beside, 0.20 of weight DMA and its bookkeeping, 0.07 of fragment reads.)
        if constexpr (p_last) {
#pragma unroll
            for (int h = 0; h < CB; ++h)
#pragma unroll
                for (int fb = 0; fb < FB; ++fb) store_block(cx, pacc[h][fb], fb, 16 * CB * c + 16 * h);
        } else {
            mquad_t bch[FB];
#pragma unroll
            for (int fb = 0; fb < FB; ++fb) bch[fb] = to_operand<true>(pacc[0][fb], pacc[CB - 1][fb]);
#pragma unroll
            for (int jb = 0; jb < UBC; ++jb) {
                const mquad_t a = lds_frag(S, CB * KSIN + jb, cx.lane);
#pragma unroll
                for (int fb = 0; fb < FB; ++fb) cacc[jb][fb] = mma(a, bch[fb], cacc[jb][fb]);
            }
        }
    }
    if constexpr (c_last) {
#pragma unroll
        for (int jb = 0; jb < UBC; ++jb)
#pragma unroll
            for (int fb = 0; fb < FB; ++fb) store_block(cx, cacc[jb][fb], fb, 16 * jb);
    } else if constexpr (hasC) {
        constexpr int KSN = UBP(hasC ? lC : 0) / CB;
        mquad_t bnext[KSN][FB];
#pragma unroll
        for (int ks = 0; ks < KSN; ++ks)
#pragma unroll
            for (int fb = 0; fb < FB; ++fb) {
                const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
                const int b1 = CB * ks + CB - 1;
                bnext[ks][fb] = to_operand<true>(cacc[CB * ks][fb], b1 < UBC ? cacc[b1 < UBC ? b1 : 0][fb] : zero);
            }
        run_pair<P + 1, KSN>(bnext, cx);
    }
}

#ifndef MOLANN_CHAIN_CORE_ONLY
extern "C" __global__ __launch_bounds__(64 * WAVES) void molann_mlp_chain(const float* __restrict__ feat, float* __restrict__ out,
                                                                         const unsigned char* __restrict__ wstream,
                                                                         const float* __restrict__ biases, long n_frames,
                                                                         int in_stride) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[LDS_BYTES];
    Ctx cx;
    cx.wstream = wstream; cx.biases = biases; cx.out = out; cx.smem = smem; cx.n_frames = n_frames;
    cx.lane = threadIdx.x & 63;
    cx.wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    cx.i16 = cx.lane & 15; cx.q4 = cx.lane >> 4;
    cx.g = 0;
    const long n_tiles = (n_frames + TILE_FRAMES - 1) / TILE_FRAMES;
    if ((long)blockIdx.x >= n_tiles) return;
    if constexpr (RESIDENT) {
        // the whole stream -> LDS, once
        for (int f = cx.wave; f < (int)(stream_bytes() / 1024); f += WAVES)
            __builtin_amdgcn_global_load_lds((gptr_t)(wstream + (size_t)f * 1024 + cx.lane * 16), (lptr_t)(smem + (size_t)f * 1024), 16, 0, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        cx.next_off = 0;
    } else {
        // prologue: the first PD slabs of the stream
        const long my_tiles = (n_tiles - 1 - (long)blockIdx.x) / gridDim.x + 1;
        cx.pf_left = my_tiles * slabs_per_tile();
        cx.pf_pair = 0; cx.pf_chunk = 0; cx.next_off = 0; cx.inflight = 0;
        for (int i = 0; i < PD; ++i) slab_request(cx);
    }

    constexpr int K0 = DIMS[0], KS0 = KS(0);
    for (long t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        cx.frame0 = t * TILE_FRAMES + (long)cx.wave * 16 * FB;
        cx.more_tiles = t + gridDim.x < n_tiles;
        // ---- this wave's input rows as B operands: lane (frame i16 of block fb, q) holds the k's of its quad in
        // k-step ks: bf16 k = 32 ks + 8q .. +7, fp32 k = 16 ks + 4q .. +3 (contiguous in the feature row either way)
        mquad_t bin[KS0][FB];
        if ((CHAIN_DIAG & 1) != 0 && t != (long)blockIdx.x) {
#pragma unroll
            for (int ks = 0; ks < KS0; ++ks)
#pragma unroll
                for (int fb = 0; fb < FB; ++fb) { const float v = (float)(cx.lane + ks + fb) * 1e-3f; bin[ks][fb] = (mquad_t){v, v, v, v}; }
        } else
#pragma unroll
        for (int fb = 0; fb < FB; ++fb) {
            long frame = cx.frame0 + 16 * fb + cx.i16;
            if (frame >= n_frames) frame = n_frames - 1; // clamped rows are computed and not stored
            const float* row = feat + frame * (long)in_stride;
#pragma unroll
            for (int ks = 0; ks < KS0; ++ks) {
                constexpr int KQ = KW / 4;                 // k's per lane quad
                const int k0 = KW * ks + KQ * cx.q4;
                f32x4 lo, hi = {0.f, 0.f, 0.f, 0.f};
                if constexpr (!BF16) {     // fp32: k = 16 ks + 4 r + q (pack_chain_kernel)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int k = 16 * ks + 4 * r + cx.q4;
                        lo[r] = k < K0 ? row[k] : 0.f;
                    }
                } else if (KW * ks + KW <= K0) { // whole k-step inside the row
                    lo = *(const f32x4u*)(row + k0);
                    if constexpr (BF16) hi = *(const f32x4u*)(row + k0 + 4);
                } else {
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        lo[s] = k0 + s < K0 ? row[k0 + s] : 0.f;
                        if constexpr (BF16) hi[s] = k0 + 4 + s < K0 ? row[k0 + 4 + s] : 0.f;
                    }
                }
                bin[ks][fb] = to_operand<false>(lo, hi);
            }
        }
        run_pair<0, KS0>(bin, cx);
    }
}
#endif
