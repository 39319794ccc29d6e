// molann_dev_restraint_f64.inc - part of libmolann_hip.so, included by molann_kernels.hip after molann_dev_vjp_f64.inc.  Float64 values,
// the energy of a harmonic restraint on them and its gradient in one launch (molann_value_and_restraint_f64 launches it).
namespace {

// =============================================================================================
// frames_value_restraint_f64_kernel<G>: x[N, n_inp, 3] -> y[N, d_out] = frames_value_vjp_f64_kernel's y, bit for bit,
// energy[N] = 1/2 sum_k kappa_k d_k^2 with d_k = y_k - center_k (wrapped by period_k, cut by flat_k: restraint_term_f64 of
// molann_math.h) and gx[N, n_inp, 3] = dE/dx = J(x)^T (kappa d), everything in double.  The cotangent kappa d depends on y, so it is
// formed where y is: lanes, grid-stride loop and steps as frames_value_vjp_f64_kernel, whose device functions do the work.  A frame's
// LDS rows are that kernel's (none without a head) and one more, cot[d_out]:
//   1.-3. rotation, features, head forward.  The outputs - the last layer's with a head, the features without one - are written to
//      cot, not to y: a lane never reads y back from global memory.
//   3r. outputs (lanes k, k + G, ...: any d_out): y[k] = cot[k] is stored, cot[k] = dy_k replaces it, the lane adds its energy terms
//      (k ascending); the frame's energy is one group_sum of the lanes' sums, stored once by the group's lane 0: a fixed order, the
//      same bits on every run.
//   4.-6. head backward, the rotation's backward and the per-atom gather on cot (frame_head_backward_f64 / frame_rotation_vjp_f64 /
//      frame_atoms_vjp_f64): with the cotangent kappa (y - center) the bits of frames_value_vjp_f64_kernel.
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
    static_assert(G == 8 || G == 16 || G == 32 || G == 64, "lane group of 8..64");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int gl = threadIdx.x & (G - 1);
    const int slot = threadIdx.x / G;
    const long per_block = blockDim.x / G;
    const long frame_dw = 3l * a.n_inp;
    const bool has_align = a.n_align > 0;
    const bool has_head = m.n_layers > 0;
    // cot first, then the rows of frames_value_vjp_f64_kernel where there is a head (lds_per_frame = d_out without one)
    double* cot = (double*)smem + (size_t)slot * a.lds_per_frame;
    double* feat = cot + a.d_out;
    double* zrows = feat + a.d_feat;
    double* row0 = zrows + (a.lds_per_frame - a.d_out - a.d_feat - 2 * a.max_w);
    double* row1 = row0 + a.max_w;
    for (long f = (long)blockIdx.x * per_block + slot; f < a.n_frames; f += (long)gridDim.x * per_block) {
        const double* xf = x + f * frame_dw;
        double* gxf = gx + f * frame_dw;
        const double* zf = center + f * a.center_stride;
        double* of = out + f * (long)a.d_out;
        // ---- 1. centroid, covariance, rotation
        double R[9] = {1., 0., 0., 0., 1., 0., 0., 0., 1.};
        double h[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.};
        V3d c = v3d(0., 0., 0.);
        if (has_align) frame_rotation_f64<G>(xf, align_idx, ref64, a.n_align, gl, c, h, R);
        // ---- 2. features
        frame_features_f64<G>(xf, items, a.n_items, gl, has_align, c, R, has_head ? feat : cot);
        lds_wave_sync();
        // ---- 3. head forward, its last layer into cot
        double* zl = zrows;
        if (has_head) zl = frame_head_forward_f64<G>(m, gl, feat, zrows, row0, row1, cot);
        // ---- 3r. the restraint on the outputs
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
        lds_wave_sync();
        // ---- 4. head backward
        const double* df = cot;     // dL/dfeat: the cotangent itself without a head
        if (has_head) df = frame_head_backward_f64<G>(m, gl, cot, zl, row0, row1);
        // ---- 5. what the items give the rotation's backward
        double GH[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.};
        V3d cen = v3d(0., 0., 0.);
        if (has_align) frame_rotation_vjp_f64<G>(xf, ref64, items, a.n_items, a.n_align, gl, df, c, h, R, GH, cen);
        // ---- 6. atoms (lanes): every row once, its terms in plan order
        frame_atoms_vjp_f64<G>(xf, gxf, ref64, items, hv_ptr, hv_list, a.n_inp, gl, df, has_align, c, R, GH, cen);
        lds_wave_sync();   // the next frame's rows are this frame's
    }
}

} // namespace
