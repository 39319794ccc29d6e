// molann_dev_hills_f64.inc - part of libmolann_hip.so, included by molann_kernels.hip after molann_dev_restraint_f64.inc.  Float64 values,
// a metadynamics bias on them - a sum of Gaussian hills - and its gradient in one launch (molann_value_and_hills_f64 launches it).
namespace {

// =============================================================================================
// frames_value_hills_f64_kernel<G>: x[N, n_inp, 3] -> y[N, d_out] = frames_value_vjp_f64_kernel's y, bit for bit,
// bias[N] = V(y) = sum_h w_h exp(-1/2 sum_k ((y_k - c_hk) / sigma_hk)^2) over a table of n_hills hills (the difference wrapped by
// period_k: hill_term_f64 of molann_math.h) and gx[N, n_inp, 3] = dV/dx = J(x)^T dV/dy, everything in double, d_out <= HILLS_MAX_D.
// Lanes, grid-stride loop, rows and steps 1-6 are frame_value_term_loop_f64's (molann_dev_vjp_f64.inc); the term between
// steps 3 and 4:
//   3h. lanes k, k + G, ... store y[k] = cot[k].  Lane gl takes hills gl, gl + G, ... in ascending order: y comes from cot (every lane
//      of the group reads the same LDS word: a broadcast), the hill's row from global memory through the caches (every group of a
//      block walks the same rows in the same order); V and the d_out cotangent sums stay in registers (a fixed array, unrolled).
//      One group_sum per accumulator; then cot[k] = dV/dy_k replaces y and the group's lane 0 stores bias[f].  Every sum has a fixed
//      order: the same bits on every run, whatever N and the frame's slot in its block.  n_hills == 0: bias 0, cot 0, and neither
//      the walk nor the sums run.  One row of widths for every hill: its 1 / sigma_k are formed once per frame, not per hill.
// sigma: one row for every hill (sigma_stride 0) or a row per hill (d_out); period: null for none.
// =============================================================================================
struct HillsF64Args : VjpF64Args {
    long n_hills;
    long sigma_stride;   // doubles between the hills' rows of sigma: 0 or d_out
};

// Step 3h's walk, one text for this kernel and frames_value_bias_f64_kernel (molann_dev_bias_f64.inc): y is the frame's row of d values in
// LDS (a broadcast read), lane gl takes hills gl, gl + G, ... ascending.  Returns the group's V; acc[k < d] leaves as the group's sum of
// the hills' g s_k / sigma_k, so dV/dy_k is -acc[k].  n_hills == 0 is a uniform skip: 0, acc as it came (zeros), no pointer read.
template <int G>
__device__ __forceinline__ double frame_hill_walk_f64(const double* y, const double* __restrict__ centers, const double* __restrict__ heights,
                                                      const double* __restrict__ sigma, const double* __restrict__ period, long n_hills,
                                                      long sigma_stride, int d, int gl, double (&acc)[HILLS_MAX_D]) {
    double v = 0.;
    if (n_hills > 0) {    // the first step of a run has no table: no walk, no sums
        const bool shared = sigma_stride == 0;
        double inv[HILLS_MAX_D] = {0., 0., 0., 0., 0., 0., 0., 0.};
        if (shared) hill_inverse_widths_f64(sigma, d, inv);
        for (long hh = gl; hh < n_hills; hh += G)
            v += hill_term_f64(y, centers + hh * d, sigma + hh * sigma_stride, inv, shared, period, heights[hh], d, acc);
        v = group_sum<G>(v);
#pragma unroll
        for (int k = 0; k < HILLS_MAX_D; ++k)
            if (k < d) acc[k] = group_sum<G>(acc[k]);
    }
    return v;
}

template <int G>
__global__ __launch_bounds__(256) void frames_value_hills_f64_kernel(const double* __restrict__ x, const double* __restrict__ centers,
                                                                     const double* __restrict__ heights, const double* __restrict__ sigma,
                                                                     const double* __restrict__ period, double* __restrict__ out,
                                                                     double* __restrict__ bias, double* __restrict__ gx,
                                                                     const int* __restrict__ align_idx, const double* __restrict__ ref64,
                                                                     const ItemDev* __restrict__ items, const int* __restrict__ hv_ptr,
                                                                     const int* __restrict__ hv_list, HillsF64Args a, F64Mlp m) {
    static_assert(HILLS_MAX_D <= G, "lane k of a group stores cot[k]");
    frame_value_term_loop_f64<G>(x, out, gx, align_idx, ref64, items, hv_ptr, hv_list, a, m, blockDim.x,
                                 [&](long f, int gl, double* cot, double* of) __attribute__((always_inline)) {
        // ---- 3h. the hills on the outputs
        for (int k = gl; k < a.d_out; k += G) of[k] = cot[k];
        double acc[HILLS_MAX_D] = {0., 0., 0., 0., 0., 0., 0., 0.};
        const double v = frame_hill_walk_f64<G>(cot, centers, heights, sigma, period, a.n_hills, a.sigma_stride, a.d_out, gl, acc);
        lds_wave_sync();   // every lane has read y from cot
#pragma unroll
        for (int k = 0; k < HILLS_MAX_D; ++k)
            if (gl == k && k < a.d_out) cot[k] = -acc[k];
        if (gl == 0) bias[f] = v;
    });
}

} // namespace
