// molann_dev_mlp.inc - part of libmolann_hip.so, included by molann_kernels.hip (one translation unit: the kernels' host stubs and the
// launches that use them must see each other).  mlp_mfma_kernel (ahead-of-time wide MLP) and the pack kernels (live parameters -> plan-owned copies).
namespace {

// =============================================================================================
// mlp_mfma_kernel: wide MLP over precomputed features, one wave per 16-frame row block
// =============================================================================================
// Packed weights, layer l (fp32 path): Wp[Jp][Kp] row-major (torch.nn.Linear layout, zero padded to
// Jp = ceil16(J), Kp = ceil16(K)), then bias[Jp].  v_mfma_f32_16x16x4_f32 wants, per k-step, lane l
// to hold A[row l&15][k = l>>4] and B[k = l>>4][col l&15]; the k order inside a 16-wide group is
// free as long as A and B agree, so lane quad q = l>>4 takes the 4 CONTIGUOUS k's 4q..4q+3 of the
// group (one 16-byte load each for A from LDS and B from the weight row) and feeds them to 4 MFMAs.
struct MlpArgs {
    long n_frames;
    int n_layers;
    int act;
    int dims[MOLANN_MAX_LAYERS + 1];
    int kp[MOLANN_MAX_LAYERS];    // padded K per layer
    int jp[MOLANN_MAX_LAYERS];    // padded J per layer
    long woff[MOLANN_MAX_LAYERS]; // element offset of layer l in the packed buffer
    int ld[2];                    // LDS row strides (elements): buffer 0 feeds even layers, buffer 1 odd layers
    int lds_per_wave;             // bytes
    int in_stride;                // row stride of the input features (floats)
};

__device__ __forceinline__ unsigned short f2bf(float f) { // round-to-nearest-even, NaN kept
    __bf16 b = (__bf16)f;
    return __builtin_bit_cast(unsigned short, b);
}

// NBW n-blocks (16 output columns each) advance together: one A fragment read from LDS feeds NBW MFMAs on
// NBW independent accumulator chains, their B fragments (weight rows, 16 B per lane) stream from L2.
template <bool BF16, int NBW, typename elem_t>
__device__ __forceinline__ void mlp_nblocks(const elem_t* __restrict__ W, const float* __restrict__ bias, const elem_t* cur,
                                            int ld_cur, elem_t* nxt, int ld_nxt, float* __restrict__ out, long frame0,
                                            int nrow, int n0, int Kp, int J, bool last, int act, int r16, int q) {
    constexpr int KG = BF16 ? 32 : 16; // k's consumed per group (bf16: one MFMA; f32: four MFMAs)
    constexpr int KQ = BF16 ? 8 : 4;   // contiguous k's per lane quad
    f32x4 acc[NBW];
    const elem_t* wrow[NBW];
#pragma unroll
    for (int b = 0; b < NBW; ++b) {
        const float bj = bias[n0 + 16 * b + r16]; // C[row 4q+reg][col r16]: bias depends on the column only
        acc[b] = (f32x4){bj, bj, bj, bj};
        wrow[b] = W + (long)(n0 + 16 * b + r16) * Kp + q * KQ;
    }
    const elem_t* arow = cur + r16 * ld_cur + q * KQ;
#pragma unroll 2
    for (int kg = 0; kg < Kp; kg += KG) {
        if constexpr (BF16) {
            const bf16x8 av = *(const bf16x8*)(arow + kg);
            bf16x8 bv[NBW];
#pragma unroll
            for (int b = 0; b < NBW; ++b) bv[b] = *(const bf16x8*)(wrow[b] + kg);
#pragma unroll
            for (int b = 0; b < NBW; ++b) acc[b] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av, bv[b], acc[b], 0, 0, 0);
        } else {
            const f32x4 av = *(const f32x4*)(arow + kg);
            f32x4 bv[NBW];
#pragma unroll
            for (int b = 0; b < NBW; ++b) bv[b] = *(const f32x4*)(wrow[b] + kg);
#pragma unroll
            for (int s = 0; s < 4; ++s)
#pragma unroll
                for (int b = 0; b < NBW; ++b) acc[b] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[s], bv[b][s], acc[b], 0, 0, 0);
        }
    }
#pragma unroll
    for (int b = 0; b < NBW; ++b) {
        const int col = n0 + 16 * b + r16;
        if (last) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 4 * q + r;
                if (row < nrow && col < J) out[(frame0 + row) * (long)J + col] = acc[b][r];
            }
        } else {
            float h[4] = {acc[b][0], acc[b][1], acc[b][2], acc[b][3]};
            activate<4, false>(act, h);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float v = col < J ? h[r] : 0.f; // padded columns feed zero into the next layer
                if constexpr (BF16) nxt[(4 * q + r) * ld_nxt + col] = f2bf(v);
                else nxt[(4 * q + r) * ld_nxt + col] = v;
            }
        }
    }
}

template <bool BF16>
__global__ __launch_bounds__(256) void mlp_mfma_kernel(const float* __restrict__ feat, float* __restrict__ out,
                                                       const void* __restrict__ wpack_v, MlpArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    using elem_t = typename std::conditional<BF16, unsigned short, float>::type;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int wpb = (int)(blockDim.x >> 6);
    const int r16 = lane & 15, q = lane >> 4;
    elem_t* buf[2];
    buf[0] = (elem_t*)(smem + (size_t)wave * a.lds_per_wave);
    buf[1] = buf[0] + 16 * a.ld[0];
    const elem_t* wpack = (const elem_t*)wpack_v;
    const long n_blocks = (a.n_frames + 15) >> 4;

    for (long rb = (long)blockIdx.x * wpb + wave; rb < n_blocks; rb += (long)gridDim.x * wpb) {
        const long frame0 = rb << 4;
        const long remf = a.n_frames - frame0;
        const int nrow = remf < 16 ? (int)remf : 16;
        // ---- stage the 16 input rows into LDS (zero padded to kp[0]) -------------------------
        {
            const int K0 = a.dims[0], Kp0 = a.kp[0];
#pragma unroll 4
            for (int r = 0; r < 16; ++r) {
                const float* src = feat + (frame0 + (r < nrow ? r : nrow - 1)) * (long)a.in_stride;
                for (int k = lane; k < Kp0; k += 64) {
                    const float v = k < K0 ? src[k] : 0.f;
                    if constexpr (BF16) buf[0][r * a.ld[0] + k] = f2bf(v);
                    else buf[0][r * a.ld[0] + k] = v;
                }
            }
        }
        for (int l = 0; l < a.n_layers; ++l) {
            const int Kp = a.kp[l], Jp = a.jp[l], J = a.dims[l + 1];
            const elem_t* W = wpack + a.woff[l];
            const float* bias = (const float*)(W + (long)Jp * Kp);
            const bool last = (l + 1 == a.n_layers);
            const elem_t* cur = buf[l & 1];
            elem_t* nxt = buf[(l + 1) & 1];
            const int ld_cur = a.ld[l & 1], ld_nxt = a.ld[(l + 1) & 1];
            int n0 = 0;
            for (; n0 + 64 <= Jp; n0 += 64)
                mlp_nblocks<BF16, 4>(W, bias, cur, ld_cur, nxt, ld_nxt, out, frame0, nrow, n0, Kp, J, last, a.act, r16, q);
            for (; n0 < Jp; n0 += 16)
                mlp_nblocks<BF16, 1>(W, bias, cur, ld_cur, nxt, ld_nxt, out, frame0, nrow, n0, Kp, J, last, a.act, r16, q);
            if (!last) { // zero the k padding of the next layer beyond Jp (kp[l+1] may exceed Jp)
                const int Kn = a.kp[l + 1];
                for (int k = Jp + lane; k < Kn; k += 64)
                    for (int r = 0; r < 16; ++r) nxt[r * ld_nxt + k] = (elem_t)0;
            }
        }
    }
}

// =============================================================================================
// pack kernels (live parameters -> plan-owned padded copies)
// =============================================================================================
struct PackArgs {
    const float* W[MOLANN_MAX_LAYERS];
    const float* b[MOLANN_MAX_LAYERS];
    int dims[MOLANN_MAX_LAYERS + 1];
    int n_layers;
    int fused;      // also write the lane kernel's per-lane MFMA fragments
    // mfma layout
    int kp[MOLANN_MAX_LAYERS];
    int jp[MOLANN_MAX_LAYERS];
    long moff[MOLANN_MAX_LAYERS];
    int bf16;
};

// Per-lane MFMA fragments of the fused MLP (frames_lane_kernel): for layer l, unit block ub, k-step ks,
// lane (i = lane&15, q = lane>>4):  A = W_l[16ub + i][k],  k = 4ks + q for layer 0 and
// k = 16(ks>>2) + 4q + (ks&3) for the following layers; then the bias fragments b_l[16ub + 4q + r].
__global__ void pack_lane_kernel(float* __restrict__ dst, PackArgs p) {
    const int NL = p.n_layers;
    const int base = NL * 1024 + NL * 512;
    const int total = base + 1024; // + layer 0's k-steps 8..15 (feature dims 33..64, specialised kernel only)
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < total; e += gridDim.x * blockDim.x) {
        const int lane = e & 63, i = lane & 15, q = lane >> 4;
        float v = 0.f;
        if (e < NL * 1024) {
            const int ks = (e >> 6) & 7, ub = (e >> 9) & 1, l = e >> 10;
            const int K = p.dims[l], J = p.dims[l + 1];
            const int j = 16 * ub + i;
            const int k = l == 0 ? 4 * ks + q : 16 * (ks >> 2) + 4 * q + (ks & 3);
            if (j < J && k < K) v = p.W[l][(long)j * K + k];
        } else if (e < base) {
            const int f = e - NL * 1024;
            const int r = (f >> 6) & 3, ub = (f >> 8) & 1, l = f >> 9;
            const int j = 16 * ub + 4 * q + r;
            if (j < p.dims[l + 1]) v = p.b[l][j];
        } else {
            const int f = e - base;
            const int ks = 8 + ((f >> 6) & 7), ub = (f >> 9) & 1;
            const int K = p.dims[0], J = p.dims[1];
            const int j = 16 * ub + i, k = 4 * ks + q;
            if (j < J && k < K) v = p.W[0][(long)j * K + k];
        }
        dst[e] = v;
    }
}

// mfma layout, layer l: Wp[Jp][Kp] (zero padded; fp32 or bf16) then bias[Jp] (fp32)
__global__ void pack_mfma_kernel(void* __restrict__ dst_v, PackArgs p) {
    const int l = blockIdx.y;
    const int K = p.dims[l], J = p.dims[l + 1], Kp = p.kp[l], Jp = p.jp[l];
    const long nW = (long)Jp * Kp;
    for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < nW + Jp; e += (long)gridDim.x * blockDim.x) {
        if (e < nW) {
            const int j = (int)(e / Kp), k = (int)(e - (long)j * Kp);
            const float v = (j < J && k < K) ? p.W[l][(long)j * K + k] : 0.f;
            if (p.bf16) ((unsigned short*)dst_v)[p.moff[l] + e] = f2bf(v);
            else ((float*)dst_v)[p.moff[l] + e] = v;
        } else {
            const int j = (int)(e - nW);
            const float v = j < J ? p.b[l][j] : 0.f;
            if (p.bf16) ((float*)((unsigned short*)dst_v + p.moff[l] + nW))[j] = v;
            else ((float*)dst_v)[p.moff[l] + nW + j] = v;
        }
    }
}


// ---- chain MLP (molann_mlp_jit.inc): host mirror of the kernel text's constexpr geometry --------------------
struct ChainGeom {
    int nl;
    int bf16; // 1: bf16 MFMA 16x16x32 (32 k's per fragment, chunks of two 16-unit blocks); 0: fp32 MFMA 16x16x4 (16, one)
    int dims[MOLANN_MAX_LAYERS + 1];
    int cb() const { return bf16 ? 2 : 1; }
    int kw() const { return bf16 ? 32 : 16; }
    int ub(int l) const { return (dims[l + 1] + 15) / 16; }
    int ubp(int l) const { return (ub(l) + cb() - 1) / cb() * cb(); }
    int ks(int l) const { return l == 0 ? (dims[0] + kw() - 1) / kw() : ubp(l - 1) / cb(); }
    int npair() const { return (nl + 1) / 2; }
    bool has_c(int p) const { return 2 * p + 1 < nl; }
    int nchunk(int p) const { return ubp(2 * p) / cb(); }
    int slab_frags(int p) const { return cb() * ks(2 * p) + (has_c(p) ? ub(2 * p + 1) : 0); }
    int slab_max() const { int m = 0; for (int p = 0; p < npair(); ++p) m = std::max(m, slab_frags(p)); return m; }
    long total_frags() const { long s = 0; for (int p = 0; p < npair(); ++p) s += (long)nchunk(p) * slab_frags(p); return s; }
    int bias_off(int l) const { int s = 0; for (int i = 0; i < l; ++i) s += 16 * ubp(i); return s; }
    // registers (VGPR + AGPR) the kernel keeps live per 16-frame block: the pair's input operands, the C
    // layer's accumulators, the P chunk, and half of the next pair's operands while they are being formed
    int regs_per_fb() const {
        int m = 0;
        for (int p = 0; p < npair(); ++p) {
            const int ksin = ks(2 * p), ubc = has_c(p) ? ub(2 * p + 1) : 0, ksn = has_c(p) ? ubp(2 * p + 1) / cb() : 0;
            m = std::max(m, 4 * (ksin + ubc + cb() + (ksn + 1) / 2));
        }
        return m;
    }
};

struct ChainPackArgs {
    const float* W[MOLANN_MAX_LAYERS];
    const float* b[MOLANN_MAX_LAYERS];
    int dims[MOLANN_MAX_LAYERS + 1];
    int n_layers, npair, bf16;
    int pair_start[MOLANN_MAX_LAYERS / 2 + 1]; // first fragment of pair p (last entry: total)
    int slab_frags[MOLANN_MAX_LAYERS / 2];
    int ks_in[MOLANN_MAX_LAYERS / 2];
    int bias_off[MOLANN_MAX_LAYERS + 1];
    long stream_bytes;
};

// Fragment F of the stream = 64 lanes x 16 B: lane (i = l&15, q = l>>4) holds A[j = 16 ub + i][k slot s = 0..7];
// layer 0: k = 32 ks + 8q + s (the order of the feature row), later layers: k = 16(2ks + (s>>2)) + 4q + (s&3)
// (the order the previous layer's accumulators come in).  Order of fragments: see molann_mlp_jit.inc.
__global__ void pack_chain_kernel(unsigned char* __restrict__ dst, ChainPackArgs a) {
    const long tid = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const long nthreads = (long)gridDim.x * blockDim.x;
    const long total = (long)a.pair_start[a.npair] * 64;
    for (long e = tid; e < total; e += nthreads) {
        const int F = (int)(e >> 6), lane = (int)(e & 63), i = lane & 15, q = lane >> 4;
        int p = 0;
        while (p + 1 < a.npair && F >= a.pair_start[p + 1]) ++p;
        const int rel = F - a.pair_start[p], c = rel / a.slab_frags[p], f = rel % a.slab_frags[p];
        const int cb = a.bf16 ? 2 : 1;
        int l, ub, ks;
        if (f < cb * a.ks_in[p]) { l = 2 * p; ks = f / cb; ub = cb * c + f % cb; }
        else { l = 2 * p + 1; ub = f - cb * a.ks_in[p]; ks = c; }
        const int K = a.dims[l], J = a.dims[l + 1], j = 16 * ub + i;
        uint4 w;
        if (a.bf16) {
            unsigned short v[8];
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                const int k = l == 0 ? 32 * ks + 8 * q + s : 16 * (2 * ks + (s >> 2)) + 4 * q + (s & 3);
                v[s] = f2bf((j < J && k < K) ? a.W[l][(long)j * K + k] : 0.f);
            }
            w.x = v[0] | ((unsigned)v[1] << 16); w.y = v[2] | ((unsigned)v[3] << 16);
            w.z = v[4] | ((unsigned)v[5] << 16); w.w = v[6] | ((unsigned)v[7] << 16);
        } else { // fp32: later layers k = 16 ks + 4q + r (the order the previous layer's accumulators come in); layer 0, whose B operand
                 // is read from the feature row in any order, k = 16 ks + 4r + q: MFMA r of a k-step then covers features 4r .. 4r + 3,
                 // and the MFMAs past the feature dimension are not issued at all (6 features: two of four)
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int k = l == 0 ? 16 * ks + 4 * r + q : 16 * ks + 4 * q + r;
                v[r] = (j < J && k < K) ? a.W[l][(long)j * K + k] : 0.f;
            }
            w.x = __float_as_uint(v[0]); w.y = __float_as_uint(v[1]); w.z = __float_as_uint(v[2]); w.w = __float_as_uint(v[3]);
        }
        *(uint4*)(dst + (size_t)F * 1024 + lane * 16) = w;
    }
    float* bias = (float*)(dst + a.stream_bytes);
    for (long e = tid; e < a.bias_off[a.n_layers]; e += nthreads) {
        int l = 0;
        while (l + 1 < a.n_layers && e >= a.bias_off[l + 1]) ++l;
        const int u = (int)e - a.bias_off[l];
        bias[e] = u < a.dims[l + 1] ? a.b[l][u] : 0.f;
    }
}

// ref_x (device, as the module holds it: centred by __init__, or anything assigned to the buffer since) -> plan copy,
// centred here, + the constants the kernels need after it.  The alignment does not depend on where ref_x sits
// (sum_a (x_a - x_c) = 0 in prod, ann.py:187), so centring is exact; it makes the sums s_r = sum r (3a .. 3a + 2)
// vanish up to rounding, so the backward kernels that leave out the centroid term -G_H s_r / n stay right.
// fp32 buffers: dst = fp32(r - mean), dst64 = dst exactly (the kernels' fp32 and fp64 copies agree, as before).
template <typename S> // S = float: the module's buffer as the reference builds it; double: a `.double()` model's buffer
__global__ void pack_ref_kernel(float* __restrict__ dst, double* __restrict__ dst64, const S* __restrict__ ref,
                                int n_align) {
    if (blockIdx.x != 0) return;
    __shared__ double red[4][256];
    __shared__ double mean[3];
    double s[4] = {0., 0., 0., 0.};
    for (int i = threadIdx.x; i < n_align; i += blockDim.x)
        for (int c = 0; c < 3; ++c) s[c] += (double)ref[3 * i + c];
    for (int c = 0; c < 3; ++c) red[c][threadIdx.x] = s[c];
    __syncthreads();
    for (int w = blockDim.x >> 1; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
            for (int c = 0; c < 3; ++c) red[c][threadIdx.x] += red[c][threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0)
        for (int c = 0; c < 3; ++c) mean[c] = red[c][0] / (double)n_align;
    __syncthreads();
    for (int c = 0; c < 4; ++c) s[c] = 0.;
    for (int i = threadIdx.x; i < n_align; i += blockDim.x) {
        double r[3];
        for (int c = 0; c < 3; ++c) {
            const double v = (double)ref[3 * i + c] - mean[c];
            const float f = (float)v;
            r[c] = sizeof(S) == sizeof(float) ? (double)f : v;
            dst[3 * i + c] = f;
            dst64[3 * i + c] = r[c];
        }
        s[0] += r[0]; s[1] += r[1]; s[2] += r[2];
        s[3] += r[0] * r[0] + r[1] * r[1] + r[2] * r[2];
    }
    for (int c = 0; c < 4; ++c) red[c][threadIdx.x] = s[c];
    __syncthreads();
    for (int w = blockDim.x >> 1; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w)
            for (int c = 0; c < 4; ++c) red[c][threadIdx.x] += red[c][threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        float* c = dst + 3 * n_align;
        double* c64 = dst64 + 3 * n_align;
        for (int k = 0; k < 4; ++k) { c[k] = (float)red[k][0]; c64[k] = red[k][0]; }
        c[4] = 1.0f / (float)n_align;
        c[5] = (float)n_align;
        c64[4] = 1.0 / (double)n_align;
        c64[5] = (double)n_align;
    }
}

} // namespace
