// molann_dev_restraint_f64.inc - part of libmolann_hip.so, included by molann_kernels.hip after molann_dev_vjp_f64.inc.  Float64 values,
// the energy of a harmonic restraint on them and its gradient in one launch (molann_value_and_restraint_f64 launches it).
namespace {

// =============================================================================================
// frames_value_restraint_f64_kernel<G>: x[N, n_inp, 3] -> y[N, d_out] = frames_value_vjp_f64_kernel's y, bit for bit,
// energy[N] = 1/2 sum_k kappa_k d_k^2 with d_k = y_k - center_k (wrapped by period_k, cut by flat_k: restraint_term_f64 of
// molann_math.h) and gx[N, n_inp, 3] = dE/dx = J(x)^T (kappa d), everything in double.  Lanes, grid-stride loop, rows and steps 1-6 are
// frame_value_term_loop_f64's (molann_dev_vjp_f64.inc); the term between steps 3 and 4:
//   3r. outputs (lanes k, k + G, ...: any d_out): y[k] = cot[k] is stored, cot[k] = dy_k replaces it, the lane adds its energy terms
//      (k ascending); the frame's energy is one group_sum of the lanes' sums, stored once by the group's lane 0: a fixed order, the
//      same bits on every run.
// center: one row for every frame (center_stride 0) or a row per frame (d_out); period, flat: null for none.
// =============================================================================================
struct RestraintF64Args : VjpF64Args {
    long center_stride;   // doubles between the frames' rows of center: 0 or d_out
};

template <int G>
__global__ __launch_bounds__(256) void frames_value_restraint_f64_kernel(const double* __restrict__ x, const double* __restrict__ center,
                                                                         const double* __restrict__ kappa, const double* __restrict__ period,
                                                                         const double* __restrict__ flat, double* __restrict__ out,
                                                                         double* __restrict__ energy, double* __restrict__ gx,
                                                                         const int* __restrict__ align_idx, const double* __restrict__ ref64,
                                                                         const ItemDev* __restrict__ items, const int* __restrict__ hv_ptr,
                                                                         const int* __restrict__ hv_list, RestraintF64Args a, F64Mlp m) {
    frame_value_term_loop_f64<G>(x, out, gx, align_idx, ref64, items, hv_ptr, hv_list, a, m, blockDim.x,
                                 [&](long f, int gl, double* cot, double* of) __attribute__((always_inline)) {
        // ---- 3r. the restraint on the outputs
        const double* zf = center + f * a.center_stride;
        double e = 0.;
        for (int k = gl; k < a.d_out; k += G) {
            const double y = cot[k];
            of[k] = y;
            double dy;
            e += restraint_term_f64(y, zf[k], kappa[k], period ? period[k] : 0.0, flat ? flat[k] : 0.0, dy);
            cot[k] = dy;
        }
        e = group_sum<G>(e);
        if (gl == 0) energy[f] = e;
    });
}

} // namespace
