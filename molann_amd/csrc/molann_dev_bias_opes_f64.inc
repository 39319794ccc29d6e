// molann_dev_bias_opes_f64.inc - part of libmolann_hip.so, included by molann_kernels.hip after molann_dev_bias_f64.inc and
// molann_dev_opes_f64.inc.  Float64 values, an OPES bias on chosen outputs together with a harmonic restraint (walls) on all of them and a
// tabulated bias on chosen outputs, and the gradient of their sum in one launch (molann_value_and_bias_opes_f64 launches it).  A kernel
// instance of its own: frames_value_bias_f64_kernel and frames_value_opes_f64_kernel keep their code.  The same kernel with n_kernels and
// norm read from a device-resident table's state instead of the arguments: frames_value_bias_opes_table_f64_kernel of
// molann_dev_bias_opes_table_f64.inc.
// Out of scope: hills and OPES in one launch (two table walks and 16 more live accumulators in a kernel that sits at the register file's
// end at G = 8; the caller moves the hills onto a table with molann_amd.bias.add_hills_to_grid, or makes two calls); more than one OPES
// term; float32; a GraphedForces replay; depositing or compressing kernels; gradients with respect to tables or parameters.
namespace {

// =============================================================================================
// frames_value_bias_opes_f64_kernel<G>: frames_value_bias_f64_kernel with the OPES walk in the place of the hill walk.
// x[N, n_inp, 3] -> y[N, d_out] = frames_value_vjp_f64_kernel's y, bit for bit, energies[N, 4] = (E_r, V_h, V_g, V_o) with V_h exactly
// 0.0 (hills are no term of this kernel: column k means what it means in frames_value_bias_f64_kernel's energies) and
// gx[N, n_inp, 3] = d(E_r + V_o + V_g)/dx = J(x)^T (dE_r/dy + dV_o/dy + dV_g/dy), everything in double:
//   E_r = 1/2 sum_k kappa_k d_k^2 over all d_out outputs (restraint_term_f64), absent where has_restraint == 0,
//   V_o = scale log(P / norm + epsilon), the bias of frames_value_opes_f64_kernel on the n_oc <= HILLS_MAX_D outputs oc[0..n_oc),
//   V_g = the table of frames_value_grid_f64_kernel on the n_gc <= GRID_MAX_D outputs gc[0..n_gc), absent where n_gc == 0.
// An absent restraint or table is a uniform branch on the arguments: none of its pointers is read and its energy is exactly 0.
// n_kernels == 0 is frame_opes_walk_f64's uniform skip: V_o = scale log(epsilon), its share of the cotangent exactly 0, no table pointer
// read.  Lanes, grid-stride loop, rows (bias64_rows: cot[d_out], the forces' rows where there is a head, ysel[BIAS_SEL]) and steps as
// frames_value_bias_f64_kernel:
//   1.-3. rotation, features, head forward; the outputs go to cot, not to y.
//   3b. lanes j gather ysel[j] = cot[oc[j]] and ysel[HILLS_MAX_D + j] = cot[gc[j]]; after a sync lanes k, k + G, ... store y[k] and
//      cot[k] = the restraint's dy_k (0 without one); the kernel walk on ysel (frame_opes_walk_f64) and opes_transform_f64 in every lane on
//      the group's sums; the stencil on ysel + HILLS_MAX_D (frame_grid_stencil_f64).  After a sync lane j adds dv[j] into cot[oc[j]], after
//      another acc_g[j] into cot[gc[j]]: the columns of a list are distinct, so no two lanes meet, and the order of the additions into an
//      output is fixed: restraint, OPES, table.  Lane 0 stores the four energies.  Every sum has a fixed order, no atomics, no
//      workspace: the same bits on every run, whatever N and the frame's slot in its block.  A y that is not finite makes this frame's
//      energies and gx NaN and no other frame's (opes_term_f64 keeps a kernel unless q >= c2 is true; grid_axis_f64 keeps every index
//      in range).
//   4.-6. head backward, the rotation's backward and the per-atom gather on cot, as the bias kernel.
// =============================================================================================
struct BiasOpesF64Args : VjpF64Args {
    int has_restraint;            // != 0: center and kappa are read
    int n_oc, n_gc;               // the OPES term's and the table's column counts; n_gc == 0: the table is absent
    int oc[HILLS_MAX_D];          // the outputs the kernels act on, in the order of the kernel table's columns
    int gc[GRID_MAX_D];           // the outputs the table's axes are, axis 0 (the slowest) first
    long center_stride;           // doubles between the frames' rows of center: 0 or d_out
    long n_kernels;
    long sigma_stride;            // doubles between the kernels' rows of sigma: 0 or n_oc
    double scale, norm, epsilon, cutoff;
    long n[GRID_MAX_D];           // the grid, as GridF64Args
    double lower[GRID_MAX_D];
    double h[GRID_MAX_D];
    int periodic[GRID_MAX_D];
};

template <int G>
__global__ __launch_bounds__(256) void frames_value_bias_opes_f64_kernel(
    const double* __restrict__ x, const double* __restrict__ center, const double* __restrict__ kappa, const double* __restrict__ rperiod,
    const double* __restrict__ flat, const double* __restrict__ centers, const double* __restrict__ heights, const double* __restrict__ sigma,
    const double* __restrict__ operiod, const double* __restrict__ table, double* __restrict__ out, double* __restrict__ energies,
    double* __restrict__ gx, const int* __restrict__ align_idx, const double* __restrict__ ref64, const ItemDev* __restrict__ items,
    const int* __restrict__ hv_ptr, const int* __restrict__ hv_list, BiasOpesF64Args a, F64Mlp m) {
    static_assert(G == 8 || G == 16 || G == 32 || G == 64, "lane group of 8..64");
    static_assert(HILLS_MAX_D <= G && GRID_MAX_D <= G, "lane j of a group gathers and scatters column j of a list");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int gl = threadIdx.x & (G - 1);
    const int slot = threadIdx.x / G;
    const long per_block = blockDim.x / G;
    const long frame_dw = 3l * a.n_inp;
    const bool has_align = a.n_align > 0;
    const bool has_head = m.n_layers > 0;
    // the rows of frames_value_bias_f64_kernel: cot, the forces' rows where there is a head, ysel
    double* cot = (double*)smem + (size_t)slot * a.lds_per_frame;
    double* feat = cot + a.d_out;
    double* zrows = feat + a.d_feat;
    double* row0 = zrows + (a.lds_per_frame - BIAS_SEL - a.d_out - a.d_feat - 2 * a.max_w);
    double* row1 = row0 + a.max_w;
    double* ysel = cot + (a.lds_per_frame - BIAS_SEL);
    for (long f = (long)blockIdx.x * per_block + slot; f < a.n_frames; f += (long)gridDim.x * per_block) {
        const double* xf = x + f * frame_dw;
        double* gxf = gx + f * frame_dw;
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
        // ---- 3b. the bias terms on the outputs: first the chosen columns into ysel, by comparisons (a list stays in scalar registers)
#pragma unroll
        for (int j = 0; j < HILLS_MAX_D; ++j)
            if (gl == j && j < a.n_oc) ysel[j] = cot[a.oc[j]];
#pragma unroll
        for (int j = 0; j < GRID_MAX_D; ++j)
            if (gl == j && j < a.n_gc) ysel[HILLS_MAX_D + j] = cot[a.gc[j]];
        lds_wave_sync();   // ysel is whole before cot changes
        double e = 0.;
        if (a.has_restraint) {
            const double* zf = center + f * a.center_stride;
            for (int k = gl; k < a.d_out; k += G) {
                const double y = cot[k];
                of[k] = y;
                double dy;
                e += restraint_term_f64(y, zf[k], kappa[k], rperiod ? rperiod[k] : 0.0, flat ? flat[k] : 0.0, dy);
                cot[k] = dy;
            }
            e = group_sum<G>(e);
        } else {
            for (int k = gl; k < a.d_out; k += G) {
                of[k] = cot[k];
                cot[k] = 0.;
            }
        }
        double vg = 0.;
        double acc_o[HILLS_MAX_D] = {0., 0., 0., 0., 0., 0., 0., 0.};
        double acc_g[GRID_MAX_D] = {0., 0., 0.};
        const double p = frame_opes_walk_f64<G>(ysel, centers, heights, sigma, operiod, a.n_kernels, a.sigma_stride, a.cutoff, a.n_oc, gl, acc_o);
        double dv[HILLS_MAX_D];
        const double vo = opes_transform_f64(p, acc_o, a.scale, a.norm, a.epsilon, a.n_oc, dv);
        if (a.n_gc > 0) vg = frame_grid_stencil_f64<G>(ysel + HILLS_MAX_D, table, a.n, a.lower, a.h, a.periodic, a.n_gc, gl, acc_g);
        lds_wave_sync();   // the restraint's cot is whole
#pragma unroll
        for (int j = 0; j < HILLS_MAX_D; ++j)
            if (gl == j && j < a.n_oc) cot[a.oc[j]] += dv[j];
        lds_wave_sync();
#pragma unroll
        for (int j = 0; j < GRID_MAX_D; ++j)
            if (gl == j && j < a.n_gc) cot[a.gc[j]] += acc_g[j];
        if (gl == 0) {
            double* ef = energies + 4 * f;
            ef[0] = e; ef[1] = 0.; ef[2] = vg; ef[3] = vo;
        }
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
