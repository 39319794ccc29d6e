// molann_dev_opes_f64.inc - part of libmolann_hip.so, included by molann_kernels.hip after molann_dev_metric_f64.inc.  Float64 values, an
// OPES bias on them - the logarithm of a kernel density - and its gradient in one launch (molann_value_and_opes_f64 launches it).
// Depositing, merging and compressing kernels and the sum the normalisation is formed from: molann_dev_opes_deposit_f64.inc.  Out of
// scope: float32; a GraphedForces replay; neighbour lists; gradients with respect to the table or the parameters.  An OPES term next to
// walls and a table, on chosen outputs: frames_value_bias_opes_f64_kernel of molann_dev_bias_opes_f64.inc, which calls this file's walk;
// the same term on a device-resident table: molann_dev_opes_table_f64.inc.
namespace {

// =============================================================================================
// frames_value_opes_f64_kernel<G>: x[N, n_inp, 3] -> y[N, d_out] = frames_value_vjp_f64_kernel's y, bit for bit,
// bias[N] = V(y) = scale log(P(y) / norm + epsilon) with P(y) = sum_h w_h (exp(-q_h / 2) - exp(-cutoff^2 / 2)) over the kernels with
// q_h = sum_k ((y_k - c_hk) / sigma_hk)^2 < cutoff^2 (the difference wrapped by period_k: opes_term_f64 of molann_math.h) and
// gx[N, n_inp, 3] = dV/dx = J(x)^T dV/dy, everything in double, d_out <= HILLS_MAX_D.  Lanes, grid-stride loop, rows and steps 1-6 are
// frame_value_term_loop_f64's (molann_dev_vjp_f64.inc); the term between steps 3 and 4 (frame_opes_value_term_f64):
//   3h. lanes k, k + G, ... store y[k] = cot[k].  Lane gl takes kernels gl, gl + G, ... in ascending order (frame_opes_walk_f64), P and
//      the d_out sums stay in registers; one group_sum per accumulator; then opes_transform_f64 in every lane on the group's sums (the
//      same values in every lane), cot[k] = dV/dy_k from lane k and bias[f] from lane 0.  Every sum has a fixed order: the same bits on
//      every run, whatever N and the frame's slot in its block; no atomics, no workspace.  n_kernels == 0: P = 0 and zero sums without
//      the walk or the group sums, so bias = scale log(epsilon) and cot is exactly 0; the table pointers are not read.
// sigma: one row for every kernel (sigma_stride 0) or a row per kernel (d_out); period: null for none.  scale, norm, epsilon and cutoff
// travel by value: the caller changes the normalisation at every deposit.
// =============================================================================================
struct OpesF64Args : VjpF64Args {
    long n_kernels;
    long sigma_stride;   // doubles between the kernels' rows of sigma: 0 or d_out
    double scale, norm, epsilon, cutoff;
};

// Step 3h's walk, frame_hill_walk_f64's with opes_term_f64 in place of the hill: y is the frame's row of d values in LDS (a broadcast
// read), lane gl takes kernels gl, gl + G, ... ascending.  Returns the group's P; acc[k < d] leaves as the group's sum of
// w e s_k / sigma_k.  n_kernels == 0 is a uniform skip: 0, acc as it came (zeros), no pointer read.
template <int G>
__device__ __forceinline__ double frame_opes_walk_f64(const double* y, const double* __restrict__ centers, const double* __restrict__ heights,
                                                      const double* __restrict__ sigma, const double* __restrict__ period, long n_kernels,
                                                      long sigma_stride, double cutoff, int d, int gl, double (&acc)[HILLS_MAX_D]) {
    double p = 0.;
    if (n_kernels > 0) {    // the first step of a run has no table: no walk, no sums
        const bool shared = sigma_stride == 0;
        double inv[HILLS_MAX_D] = {0., 0., 0., 0., 0., 0., 0., 0.};
        if (shared) hill_inverse_widths_f64(sigma, d, inv);
        double c2, c0;
        opes_cutoff_f64(cutoff, c2, c0);
        for (long hh = gl; hh < n_kernels; hh += G)
            p += opes_term_f64(y, centers + hh * d, sigma + hh * sigma_stride, inv, shared, period, heights[hh], c2, c0, d, acc);
        p = group_sum<G>(p);
#pragma unroll
        for (int k = 0; k < HILLS_MAX_D; ++k)
            if (k < d) acc[k] = group_sum<G>(acc[k]);
    }
    return p;
}

// Step 3h, one text for frames_value_opes_f64_kernel and frames_value_opes_table_f64_kernel (molann_dev_opes_table_f64.inc): y is stored,
// the walk and opes_transform_f64 run on cot, and after a sync lane k stores cot[k] = dV/dy_k and lane 0 the frame's bias.  n_kernels,
// sigma_stride and norm come by value - from the arguments or from a table's state, which is all the two kernels differ in.
template <int G>
__device__ __forceinline__ void frame_opes_value_term_f64(double* cot, double* of, double* bias_f, const double* __restrict__ centers,
                                                          const double* __restrict__ heights, const double* __restrict__ sigma,
                                                          const double* __restrict__ period, long n_kernels, long sigma_stride, double cutoff,
                                                          double scale, double norm, double epsilon, int d, int gl) {
    for (int k = gl; k < d; k += G) of[k] = cot[k];
    double acc[HILLS_MAX_D] = {0., 0., 0., 0., 0., 0., 0., 0.};
    const double p = frame_opes_walk_f64<G>(cot, centers, heights, sigma, period, n_kernels, sigma_stride, cutoff, d, gl, acc);
    double dv[HILLS_MAX_D];
    const double v = opes_transform_f64(p, acc, scale, norm, epsilon, d, dv);
    lds_wave_sync();   // every lane has read y from cot
#pragma unroll
    for (int k = 0; k < HILLS_MAX_D; ++k)
        if (gl == k && k < d) cot[k] = dv[k];
    if (gl == 0) *bias_f = v;
}

template <int G>
__global__ __launch_bounds__(256) void frames_value_opes_f64_kernel(const double* __restrict__ x, const double* __restrict__ centers,
                                                                    const double* __restrict__ heights, const double* __restrict__ sigma,
                                                                    const double* __restrict__ period, double* __restrict__ out,
                                                                    double* __restrict__ bias, double* __restrict__ gx,
                                                                    const int* __restrict__ align_idx, const double* __restrict__ ref64,
                                                                    const ItemDev* __restrict__ items, const int* __restrict__ hv_ptr,
                                                                    const int* __restrict__ hv_list, OpesF64Args a, F64Mlp m) {
    static_assert(HILLS_MAX_D <= G, "lane k of a group stores cot[k]");
    frame_value_term_loop_f64<G>(x, out, gx, align_idx, ref64, items, hv_ptr, hv_list, a, m, blockDim.x,
                                 [&](long f, int gl, double* cot, double* of) __attribute__((always_inline)) {
        frame_opes_value_term_f64<G>(cot, of, bias + f, centers, heights, sigma, period, a.n_kernels, a.sigma_stride, a.cutoff, a.scale,
                                     a.norm, a.epsilon, a.d_out, gl);
    });
}

} // namespace
