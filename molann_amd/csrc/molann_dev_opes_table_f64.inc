// molann_dev_opes_table_f64.inc - part of libmolann_hip.so, included by molann_kernels.hip after molann_dev_opes_deposit_f64.inc.  Where the
// two halves of an OPES run meet: frames_value_opes_table_f64_kernel evaluates the bias on a device-resident table whose live count and
// normalisation it reads from the table's state (molann_value_and_opes_table_f64 launches it), and opes_step_f64_kernel turns the outputs
// and biases that launch wrote into this step's kernels - weights, effective sample size, rescaled widths, heights - and deposits them
// (molann_opes_step_f64).  Neither needs a value from the host, so the pair queues, and is captured in a graph, with no read-back.  The
// same pair for a run with walls, a table or a wider model - value_and_bias(opes=) reading the state, and the step on strided outputs
// and chosen columns - is molann_dev_bias_opes_table_f64.inc, which keeps this file's argument layout; the step with adaptive sigma and
// the explore variant is molann_dev_opes_adaptive_f64.inc.  Out of scope: walkers on several ranks; float32; a step on more than one
// block; a GraphedForces wrapper.
namespace {

// =============================================================================================
// frames_value_opes_table_f64_kernel<G>: frames_value_opes_f64_kernel (molann_dev_opes_f64.inc) with n_kernels and norm taken from
// state[4] = (n, S, merges, refused) in device memory instead of the launch's arguments: once, before the frame loop, every lane forms
// n = opes_live_count_f64(state[0], capacity) (held to [0, capacity] whatever the bits) and, where n >= 1, norm = S / n
// (opes_table_norm_f64) - uniform loads and one division.  The term (frame_opes_value_term_f64) and the loop around it
// (frame_value_term_loop_f64) are that kernel's text, so for the same n and norm the outputs are its bits.  sigma has a row per
// kernel (stride d_out).  n == 0: no walk, no table pointer read, norm not formed, bias = scale log(epsilon), cot exactly 0.  A state
// whose S is not finite and > 0 while n >= 1 gives NaN or inf for every frame: the state is the caller's.
// =============================================================================================
struct OpesTableF64Args : VjpF64Args {
    long capacity;
    double scale, epsilon, cutoff;
};

template <int G>
__global__ __launch_bounds__(256) void frames_value_opes_table_f64_kernel(const double* __restrict__ x, const double* __restrict__ centers,
                                                                          const double* __restrict__ heights, const double* __restrict__ sigma,
                                                                          const double* __restrict__ state, const double* __restrict__ period,
                                                                          double* __restrict__ out, double* __restrict__ bias,
                                                                          double* __restrict__ gx, const int* __restrict__ align_idx,
                                                                          const double* __restrict__ ref64, const ItemDev* __restrict__ items,
                                                                          const int* __restrict__ hv_ptr, const int* __restrict__ hv_list,
                                                                          OpesTableF64Args a, F64Mlp m) {
    static_assert(HILLS_MAX_D <= G, "lane k of a group stores cot[k]");
    // the table's state: the same two values in every lane
    const long n_kernels = opes_live_count_f64(state[0], a.capacity);
    double norm = 1.0;      // n == 0: P = 0 and zero sums, whatever the norm
    if (n_kernels > 0) norm = opes_table_norm_f64(state[1], n_kernels);
    frame_value_term_loop_f64<G>(x, out, gx, align_idx, ref64, items, hv_ptr, hv_list, a, m, blockDim.x,
                                 [&](long f, int gl, double* cot, double* of) __attribute__((always_inline)) {
        frame_opes_value_term_f64<G>(cot, of, bias + f, centers, heights, sigma, period, n_kernels, (long)a.d_out, a.cutoff, a.scale, norm,
                                     a.epsilon, a.d_out, gl);
    });
}

// =============================================================================================
// opes_step_f64_kernel: ONE block of 256 threads runs opes_step_steps_f64 (molann_math.h) on the table, state[4] and
// run[8] = (counter, sum_w, sum_w2, neff, sigma_scale, rct, 0, 0), from y[W, d] and V[W] - the `out` and `bias` a bias launch just
// wrote, read only here.  The executor is the deposit kernel's (OpesDepositDev: its search, its walk, its writes) with two additions:
//   walker_sums: thread t takes walkers t, t + 256, ... ascending (opes_walker_weight_f64, one exp each) and adds the valid ones to
//     its three partial sums; group_sum<64> in the wave, then ((w0 + w1) + w2) + w3 from LDS, a sum at a time: pair_sum's scheme, a fixed
//     order and no atomics.
//   load_new(a): y's row a, the step's widths and opes_walker_height_f64 - every thread forms the same exp again, so nothing travels
//     through memory; an invalid walker's height is NaN and the deposit's validity check refuses it.
// Every thread holds run, n, S and the counts in registers and computes the same values; thread 0 stores state and run at the end
// (vector stores, plain C++).  LDS: the deposit kernel's four reduction slots.
// =============================================================================================
struct OpesStepDev : OpesDepositDev {
    const double* V;
    double beta;
    double ratio;
    double step_sigma[HILLS_MAX_D];

    __device__ __forceinline__ double block_sum(double part) const {
        part = group_sum<64>(part);
        if ((threadIdx.x & 63) == 0) red_q[threadIdx.x >> 6] = part;
        __syncthreads();
        const double total = ((red_q[0] + red_q[1]) + red_q[2]) + red_q[3];
        __syncthreads();    // the slots are free again
        return total;
    }
    __device__ __forceinline__ void walker_sums(long n_walkers, double& count, double& sum_w, double& sum_w2) const {
        double pc = 0.0, pw = 0.0, pw2 = 0.0;
        for (long a = threadIdx.x; a < n_walkers; a += 256) {
            double w;
            if (opes_walker_weight_f64(beta, V[a], new_centers + a * d, d, w)) opes_walker_add_f64(w, pc, pw, pw2);
        }
        count = block_sum(pc);
        sum_w = block_sum(pw);
        sum_w2 = block_sum(pw2);
    }
    __device__ __forceinline__ void load_new(long a, double (&c)[HILLS_MAX_D], double (&s)[HILLS_MAX_D], double& h) const {
#pragma unroll
        for (int k = 0; k < HILLS_MAX_D; ++k) {
            c[k] = k < d ? new_centers[a * d + k] : 0.0;
            s[k] = k < d ? step_sigma[k] : 1.0;
        }
        h = opes_walker_height_f64(beta, V[a], new_centers + a * d, d, ratio);
    }
};

__global__ __launch_bounds__(256) void opes_step_f64_kernel(double* centers, double* sigma, double* heights, long capacity, int d,
                                                            const double* period, double* state, double* run, const double* y, const double* V,
                                                            long n_walkers, const double* sigma0, const double* sigma_min, double beta,
                                                            double threshold, double cutoff, int fixed_sigma) {
    __shared__ double red_q[4];
    __shared__ long long red_k[4];
    OpesStepDev ex = {{centers, sigma, heights, period, y, nullptr, nullptr, d, red_q, red_k}, V, beta, 1.0, {1., 1., 1., 1., 1., 1., 1., 1.}};
    long n = opes_live_count_f64(state[0], capacity);
    double S = state[1], merges = state[2], refused = state[3];
    double r[8] = {run[0], run[1], run[2], 0., 0., 0., 0., 0.};
    opes_step_steps_f64(ex, capacity, d, period, n_walkers, threshold, cutoff, beta, fixed_sigma, sigma0, sigma_min, n, S, merges, refused, r);
    __syncthreads();    // every thread has read state and run
    if (threadIdx.x == 0) {
        state[0] = (double)n; state[1] = S; state[2] = merges; state[3] = refused;
#pragma unroll
        for (int i = 0; i < 8; ++i) run[i] = r[i];
    }
}

} // namespace
