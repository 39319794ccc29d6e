// molann_dev_opes_deposit_f64.inc - part of libmolann_hip.so, included by molann_kernels.hip after molann_dev_bias_opes_f64.inc.  The other
// half of an OPES run, between the steps that molann_value_and_opes_f64 serves: opes_deposit_f64_kernel compresses new kernels into a
// device-resident table in place and keeps the sum S its normalisation is formed from (molann_opes_deposit_f64 launches it), and
// opes_kernel_sum_f64_kernel gives the kernel density at arbitrary points (molann_opes_kernel_sum_f64).  The scalar bookkeeping of OPES
// (neff, the bandwidth rescaling, the heights) on the device and the bias that reads this state: molann_dev_opes_table_f64.inc.  Out of
// scope: deposits on more than one block; neighbour lists; float32.
namespace {

// =============================================================================================
// opes_deposit_f64_kernel: ONE block of 256 threads runs opes_deposit_steps_f64 (molann_math.h) on centers[cap, d], sigma[cap, d],
// heights[cap] and state[4] = (n, S, merges, refused).  Every thread holds n, S and the kernels in hand (the giver, the taker) in
// registers and computes the same values from the same broadcasts, so every decision is uniform and state needs no LDS; thread 0
// stores it at the end.  The launch reads n and S on the device: the host enqueues deposits back to back without knowing them.
//   search: thread t takes slots t, t + 256, ... ascending (opes_merge_distance_f64: no exp, the host's bits), keeps the smallest q and
//     on a tie the smallest slot; a butterfly of __shfl_xor on the pair inside the wave, then the four waves' pairs through LDS, every
//     thread reading all four in order.  A NaN q loses every comparison.
//   sums: the same strided partials (opes_pair_term_f64, two exp per term), group_sum<64> in the wave, then ((w0 + w1) + w2) + w3 from LDS:
//     a fixed order and no atomics, the same bits on every run.  Rows sit in L2 after the first walk; 1000 kernels x 8 columns do not
//     fit LDS next to a useful block and do not need to.
//   writes: lanes < d of wave 0 store a row (vector stores, plain C++), between __syncthreads(), which orders them before the block's
//     next reads.  Rows >= n are dead storage, rows >= cap are never touched (n is held to [0, cap] whatever state holds).
// LDS: the four reduction slots.
// =============================================================================================
struct OpesDepositDev {
    double* centers;
    double* sigma;
    double* heights;
    const double* period;
    const double* new_centers;
    const double* new_sigma;
    const double* new_heights;
    int d;
    double* red_q;         // [4] in LDS
    long long* red_k;      // [4] in LDS

    __device__ __forceinline__ void read_row(const double* c, const double* s, const double* h, long row, double (&co)[HILLS_MAX_D],
                                             double (&so)[HILLS_MAX_D], double& ho) const {
#pragma unroll
        for (int k = 0; k < HILLS_MAX_D; ++k) {
            co[k] = k < d ? c[row * d + k] : 0.0;
            so[k] = k < d ? s[row * d + k] : 1.0;
        }
        ho = h[row];
    }
    __device__ __forceinline__ void load_new(long a, double (&c)[HILLS_MAX_D], double (&s)[HILLS_MAX_D], double& h) const {
        read_row(new_centers, new_sigma, new_heights, a, c, s, h);
    }
    __device__ __forceinline__ void load(long slot, double (&c)[HILLS_MAX_D], double (&s)[HILLS_MAX_D], double& h) const {
        read_row(centers, sigma, heights, slot, c, s, h);
    }
    __device__ __forceinline__ void store(long slot, const double (&c)[HILLS_MAX_D], const double (&s)[HILLS_MAX_D], double h) const {
        __syncthreads();    // every thread has read what it needed of this row
        const int t = threadIdx.x;
        if (t < d) {
            double cv = 0.0, sv = 0.0;
#pragma unroll
            for (int k = 0; k < HILLS_MAX_D; ++k)
                if (t == k) { cv = c[k]; sv = s[k]; }
            centers[slot * d + t] = cv;
            sigma[slot * d + t] = sv;
        }
        if (t == 0) heights[slot] = h;
        __syncthreads();
    }
    __device__ __forceinline__ void move(long from, long to) const {
        __syncthreads();
        const int t = threadIdx.x;
        if (t < d) {
            centers[to * d + t] = centers[from * d + t];
            sigma[to * d + t] = sigma[from * d + t];
        }
        if (t == 0) heights[to] = heights[from];
        __syncthreads();
    }
    __device__ __forceinline__ bool nearest(const double (&c)[HILLS_MAX_D], long n, long skip, double& q_out, long& slot_out) const {
        const double inf = __builtin_huge_val();
        const long long none = 0x7fffffffffffffffll;
        double q = inf;
        long long slot = none;
        for (long k = threadIdx.x; k < n; k += 256) {
            if (k == skip) continue;
            const double qk = opes_merge_distance_f64(c, centers + k * d, sigma + k * d, period, d);
            if (qk < q) { q = qk; slot = k; }
        }
        auto take = [&](double oq, long long ok) {
            if (oq < q || (oq == q && ok < slot)) { q = oq; slot = ok; }
        };
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) {
            const double oq = __shfl_xor(q, m, 64);
            const long long ok = __shfl_xor(slot, m, 64);
            take(oq, ok);
        }
        if ((threadIdx.x & 63) == 0) { red_q[threadIdx.x >> 6] = q; red_k[threadIdx.x >> 6] = slot; }
        __syncthreads();
        q = red_q[0]; slot = red_k[0];
#pragma unroll
        for (int w = 1; w < 4; ++w) take(red_q[w], red_k[w]);
        __syncthreads();    // the slots are free again
        q_out = q; slot_out = (long)slot;
        return slot != none;
    }
    __device__ __forceinline__ double pair_sum(const double (&ce)[HILLS_MAX_D], const double (&se)[HILLS_MAX_D], double he, long n, long skip_a,
                                               long skip_b, double c2, double c0) const {
        double inv[HILLS_MAX_D];
        hill_inverse_widths_f64(se, d, inv);
        double part = 0.0;
        for (long i = threadIdx.x; i < n; i += 256) {
            if (i == skip_a || i == skip_b) continue;
            part = part + opes_pair_term_f64(ce, se, inv, he, centers + i * d, sigma + i * d, heights[i], period, c2, c0, d);
        }
        part = group_sum<64>(part);
        if ((threadIdx.x & 63) == 0) red_q[threadIdx.x >> 6] = part;
        __syncthreads();
        const double total = ((red_q[0] + red_q[1]) + red_q[2]) + red_q[3];
        __syncthreads();
        return total;
    }
};

__global__ __launch_bounds__(256) void opes_deposit_f64_kernel(double* centers, double* sigma, double* heights, long capacity, int d,
                                                               const double* period, double* state, const double* new_centers,
                                                               const double* new_sigma, const double* new_heights, long n_new, double threshold,
                                                               double cutoff) {
    __shared__ double red_q[4];
    __shared__ long long red_k[4];
    OpesDepositDev ex = {centers, sigma, heights, period, new_centers, new_sigma, new_heights, d, red_q, red_k};
    long n = opes_live_count_f64(state[0], capacity);
    double S = state[1], merges = state[2], refused = state[3];
    opes_deposit_steps_f64(ex, capacity, d, period, n_new, threshold, cutoff, n, S, merges, refused);
    __syncthreads();    // every thread has read state
    if (threadIdx.x == 0) {
        state[0] = (double)n; state[1] = S; state[2] = merges; state[3] = refused;
    }
}

// =============================================================================================
// opes_kernel_sum_f64_kernel: P[m] = sum_h heights_h K_h(points[m]) and, where dP is not null, dP[m, k] = dP/dpoints[m, k], for
// points[M, d].  A wave per point in a grid-stride loop: lanes k < d put the point's row into the wave's LDS row, every lane walks kernels
// lane, lane + 64, ... by frame_opes_walk_f64<64> of molann_dev_opes_f64.inc as it is (the bias kernels' walk, sums and order), lane 0
// stores P and lanes k < d store -acc[k].  sigma is one row (stride 0) or a row per kernel (d); n_kernels == 0: P = 0, dP = 0 and no
// table pointer is read.  No atomics: the same bits on every run, whatever M.
// =============================================================================================
__global__ __launch_bounds__(256) void opes_kernel_sum_f64_kernel(const double* __restrict__ points, const double* __restrict__ centers,
                                                                  const double* __restrict__ heights, const double* __restrict__ sigma,
                                                                  const double* __restrict__ period, double* __restrict__ P,
                                                                  double* __restrict__ dP, long n_points, long n_kernels, long sigma_stride,
                                                                  double cutoff, int d) {
    __shared__ double rows[4][HILLS_MAX_D];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double* y = rows[wave];
    for (long m = (long)blockIdx.x * 4 + wave; m < n_points; m += (long)gridDim.x * 4) {
        if (lane < d) y[lane] = points[m * d + lane];
        lds_wave_sync();
        double acc[HILLS_MAX_D] = {0., 0., 0., 0., 0., 0., 0., 0.};
        const double p = frame_opes_walk_f64<64>(y, centers, heights, sigma, period, n_kernels, sigma_stride, cutoff, d, lane, acc);
        if (lane == 0) P[m] = p;
        if (dP) {
#pragma unroll
            for (int k = 0; k < HILLS_MAX_D; ++k)
                if (lane == k && k < d) dP[m * d + k] = -acc[k];
        }
        lds_wave_sync();   // every lane has read the row
    }
}

} // namespace
