// molann_dev_opes_adaptive_f64.inc - part of libmolann_hip.so, included by molann_kernels.hip after molann_dev_bias_opes_table_f64.inc.  The
// step of an OPES run in OPES_METAD's two other modes: widths measured from the run's own outputs (SIGMA=ADAPTIVE) and the explore
// variant (OPES_METAD_EXPLORE).  opes_step_modes_f64_kernel is opes_step_columns_f64_kernel (molann_dev_bias_opes_table_f64.inc: the same
// strided, column-mapped reading of the walkers, the same sums, the same deposit executor) running opes_step_modes_steps_f64
// (molann_opes_modes.h) in place of opes_step_steps_f64, with the per-walker state adapt[W, 3, d] = (mean, M2, sigma0) kept in device memory
// between the steps (molann_opes_step_modes_f64 launches it).  Out of scope: walkers on several ranks; float32; a step on more than one
// block; a TorchScript operator.
namespace {

// =============================================================================================
// opes_step_modes_f64_kernel: ONE block of 256 threads.  What the executor adds to OpesStepColumnsDev:
//   observe: thread t takes the (walker, column) pairs t, t + 256, ... of the W d pairs; a pair reads and writes its own mean and M2
//     and nothing of another pair, so there is no reduction and no atomic, and every run gives the same bits.  A walker counts when its
//     d gathered outputs are finite - every thread that holds one of its pairs reads all d - and keeps its row otherwise.
//   first_deposit: the same pairs; M2 <- M2 biasfactor and sigma0 (opes_adapt_first_f64).
//   Both end with __syncthreads(): load_new(a) reads walker a's whole row in EVERY thread, rows that other threads have just written.
//   load_new(a): the gathered centre, the widths and their ratio from adapt's row (opes_adaptive_widths_f64: d square roots, formed
//     again in every thread, as every thread forms the same exp) or the step's shared widths without adapt, and the height
//     (opes_walker_height_modes_f64).
// A deposit before the first stride has passed, and `observe`, return after the averages: thread 0 stores run[6] and nothing else.
// Every thread holds run, n, S and the counts in registers; thread 0 stores them at the end (vector stores, plain C++).  LDS: the
// deposit kernel's four reduction slots.
// =============================================================================================
struct OpesStepModesDev : OpesStepColumnsDev {      // its fields, its gather and its walker_sums
    double* adapt;                // [W, 3, d] or nullptr
    const double* sigma_min;      // [d] or nullptr
    double width_count, width_factor, width_scale;
    int fixed_sigma, explore;

    // column k of walker a, k a run-time index: comparisons on a compile-time j, no indexed register array
    __device__ __forceinline__ double output(long a, int k) const {
        const double* row = new_centers + a * y_stride;
        int ck = 0;
#pragma unroll
        for (int j = 0; j < HILLS_MAX_D; ++j)
            if (j == k) ck = col[j];
        return row[ck];
    }
    __device__ __forceinline__ void observe(long n_walkers, double tau) const {
        const long pairs = n_walkers * d;
        for (long p = threadIdx.x; p < pairs; p += 256) {
            const long a = p / d;
            const int k = (int)(p - a * d);
            double yc[HILLS_MAX_D];
            gather(a, yc);
            if (!opes_outputs_finite_f64(yc, d)) continue;
            double* row = adapt + a * 3 * d;
            double mean = row[k], M2 = row[d + k];
            opes_adapt_observe_f64(output(a, k), period ? period[k] : 0.0, tau, mean, M2);
            row[k] = mean;
            row[d + k] = M2;
        }
        __syncthreads();    // the rows are whole before any thread reads another thread's pair
    }
    __device__ __forceinline__ void first_deposit(long n_walkers, double count, double factor, double biasfactor, const double* smin) const {
        const long pairs = n_walkers * d;
        for (long p = threadIdx.x; p < pairs; p += 256) {
            const long a = p / d;
            const int k = (int)(p - a * d);
            double* row = adapt + a * 3 * d;
            double M2 = row[d + k], s0;
            opes_adapt_first_f64(count, factor, biasfactor, smin ? smin[k] : 0.0, M2, s0);
            row[d + k] = M2;
            row[2 * d + k] = s0;
        }
        __syncthreads();    // M2 and sigma0 are whole before load_new reads them
    }
    __device__ __forceinline__ void load_new(long a, double (&c)[HILLS_MAX_D], double (&s)[HILLS_MAX_D], double& h) const {
        gather(a, c);
        double ratio_a = ratio;
        if (adapt) {
            const double* row = adapt + a * 3 * d;
            ratio_a = opes_adaptive_widths_f64(row + d, row + 2 * d, sigma_min, width_count, width_factor, width_scale, fixed_sigma, d, s);
        } else {
#pragma unroll
            for (int k = 0; k < HILLS_MAX_D; ++k) s[k] = k < d ? step_sigma[k] : 1.0;
        }
        h = opes_walker_height_modes_f64(beta, V[a * v_stride], c, d, ratio_a, explore);
    }
};

__global__ __launch_bounds__(256) void opes_step_modes_f64_kernel(double* centers, double* sigma, double* heights, long capacity, int d,
                                                                  const double* period, double* state, double* run, const double* y,
                                                                  long y_stride, OpesStepColumns cols, const double* V, long v_stride,
                                                                  long n_walkers, const double* sigma0, const double* sigma_min, double* adapt,
                                                                  double beta, double biasfactor, double adaptive_stride, double threshold,
                                                                  double cutoff, int flags) {
    __shared__ double red_q[4];
    __shared__ long long red_k[4];
    OpesStepModesDev ex = {{{{centers, sigma, heights, period, y, nullptr, nullptr, d, red_q, red_k}, V, beta, 1.0, {1., 1., 1., 1., 1., 1., 1., 1.}},
                            y_stride, v_stride, {cols.col[0], cols.col[1], cols.col[2], cols.col[3], cols.col[4], cols.col[5], cols.col[6], cols.col[7]}},
                           adapt, sigma_min, 1.0, 1.0, 1.0, 0, 0};
    long n = opes_live_count_f64(state[0], capacity);
    double S = state[1], merges = state[2], refused = state[3];
    double r[8] = {run[0], run[1], run[2], run[3], run[4], run[5], run[6], run[7]};
    const bool deposited = opes_step_modes_steps_f64(ex, capacity, d, period, n_walkers, threshold, cutoff, beta, flags, adapt != nullptr, sigma0,
                                                     sigma_min, biasfactor, adaptive_stride, n, S, merges, refused, r);
    __syncthreads();    // every thread has read state and run
    if (threadIdx.x == 0) {
        if (deposited) {
            state[0] = (double)n; state[1] = S; state[2] = merges; state[3] = refused;
#pragma unroll
            for (int i = 0; i < 8; ++i) run[i] = r[i];
        } else {
            run[6] = r[6];
        }
    }
}

} // namespace
