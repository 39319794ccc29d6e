// molann_dev_grid_f64.inc - part of libmolann_hip.so, included by molann_kernels.hip after molann_dev_hills_f64.inc.  Float64 values, a
// bias interpolated from a table over them and its gradient in one launch (molann_value_and_grid_f64 launches it).
namespace {

// =============================================================================================
// frames_value_grid_f64_kernel<G>: x[N, n_inp, 3] -> y[N, d_out] = frames_value_vjp_f64_kernel's y, bit for bit,
// bias[N] = V(y), the cubic-convolution (Catmull-Rom) interpolant of a table on a regular grid over the d_out <= GRID_MAX_D outputs
// (grid_axis_f64 / grid_stencil_term_f64 of molann_math.h), and gx[N, n_inp, 3] = dV/dx = J(x)^T dV/dy, everything in double.  The cost
// of a frame does not depend on what the table was made from: 4^d_out loads.  Lanes, grid-stride loop, rows and steps are those of
// frame_value_term_loop_f64 (molann_dev_vjp_f64.inc), written out: this is the one kernel of the family that keeps a loop of its own.
// Called through the shared loop it computes the same bits but runs 1-3.5 % slower at every batch size (the geometry's scalar registers
// are spilled differently around the stencil; DESIGN.md, "One frame loop for the value-and-bias kernels"), so a change to steps 1-6 is
// made here as well.  A frame's LDS rows are cot[d_out], then frames_value_vjp_f64_kernel's where there is a head:
//   1.-3. rotation, features, head forward; the outputs go to cot, not to y.
//   3g. lanes k, k + G, ... store y[k] = cot[k].  Every lane forms the d_out axis steps from cot (every lane of the group reads the
//      same LDS word: a broadcast): four indices, four weights and four derivative weights per axis, in registers.  Lane gl takes the
//      stencil points p = gl, gl + G, ... < 4^d_out in ascending order, j_k = (p >> 2k) & 3; a point is one load from global memory
//      through the caches, its offset formed in long; the rounds are unrolled and their loads unconditional (see the loop).  V and
//      the d_out derivative sums stay in registers (a fixed array, unrolled).
//      One group_sum per accumulator; then cot[k] = dV/dy_k replaces y and the group's lane 0 stores bias[f].  Every sum has a fixed
//      order: the same bits on every run, whatever N and the frame's slot in its block.  Every index is in its axis' range for every
//      bit pattern of y, so no load leaves the table; a y that is not finite makes this frame's bias and gx NaN.
//   4.-6. head backward, the rotation's backward and the per-atom gather on cot, as the restraint kernel.
// The grid's geometry travels by value in the arguments: nothing of it is read from memory.
// =============================================================================================
struct GridF64Args : VjpF64Args {
    long n[GRID_MAX_D];           // points per axis (output 0 is the slowest axis of the table)
    double lower[GRID_MAX_D];     // the position of point 0
    double h[GRID_MAX_D];         // the spacing
    int periodic[GRID_MAX_D];     // != 0: the axis has period n h
};

// Step 3g's axis steps and stencil loop, one text for this kernel and frames_value_bias_f64_kernel (molann_dev_bias_f64.inc): y is the
// frame's row of d values in LDS (a broadcast read), lane gl takes the stencil points gl, gl + G, ... < 4^d ascending.  Returns the
// group's V; acc[k < d] leaves as the group's dV/dy_k.
template <int G>
__device__ __forceinline__ double frame_grid_stencil_f64(const double* y, const double* __restrict__ table, const long (&n)[GRID_MAX_D],
                                                         const double (&lower)[GRID_MAX_D], const double (&spacing)[GRID_MAX_D],
                                                         const int (&periodic)[GRID_MAX_D], int d, int gl, double (&acc)[GRID_MAX_D]) {
    const int points = 1 << (2 * d);
    long idx[GRID_MAX_D][4];
    double wa[GRID_MAX_D][4], wb[GRID_MAX_D][4];
#pragma unroll
    for (int k = 0; k < GRID_MAX_D; ++k) {
        if (k < d) {
            grid_axis_f64(y[k], n[k], lower[k], spacing[k], periodic[k] != 0, idx[k], wa[k], wb[k]);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) { idx[k][j] = 0; wa[k][j] = 0.; wb[k][j] = 0.; }
        }
    }
    double v = 0.;
    // 64 / G rounds whatever d: a round past the last point loads a point again (p wraps, the address is a stencil point's)
    // and adds nothing, so no load sits behind a branch and all of a lane's loads are in flight together
#pragma unroll
    for (int r = 0; r < 64 / G; ++r) {
        const int p = gl + r * G;
        double term[GRID_MAX_D];
        const double t = grid_stencil_term_f64(p & (points - 1), d, table, n, idx, wa, wb, term);
        const bool mine = p < points;
        v += mine ? t : 0.;
#pragma unroll
        for (int k = 0; k < GRID_MAX_D; ++k) acc[k] += mine ? term[k] : 0.;
    }
    v = group_sum<G>(v);
#pragma unroll
    for (int k = 0; k < GRID_MAX_D; ++k)
        if (k < d) acc[k] = group_sum<G>(acc[k]);
    return v;
}

template <int G>
__global__ __launch_bounds__(256) void frames_value_grid_f64_kernel(const double* __restrict__ x, const double* __restrict__ table,
                                                                    double* __restrict__ out, double* __restrict__ bias,
                                                                    double* __restrict__ gx, const int* __restrict__ align_idx,
                                                                    const double* __restrict__ ref64, const ItemDev* __restrict__ items,
                                                                    const int* __restrict__ hv_ptr, const int* __restrict__ hv_list,
                                                                    GridF64Args a, F64Mlp m) {
    static_assert(G == 8 || G == 16 || G == 32 || G == 64, "lane group of 8..64");
    static_assert(GRID_MAX_D <= G, "lane k of a group stores cot[k]");
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
        // ---- 3g. the table on the outputs
        for (int k = gl; k < a.d_out; k += G) of[k] = cot[k];
        double acc[GRID_MAX_D] = {0., 0., 0.};
        const double v = frame_grid_stencil_f64<G>(cot, table, a.n, a.lower, a.h, a.periodic, a.d_out, gl, acc);
        lds_wave_sync();   // every lane has read y from cot
#pragma unroll
        for (int k = 0; k < GRID_MAX_D; ++k)
            if (gl == k && k < a.d_out) cot[k] = acc[k];
        if (gl == 0) bias[f] = v;
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
