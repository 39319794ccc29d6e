// molann_dev_bias_opes_table_f64.inc - part of libmolann_hip.so, included by molann_kernels.hip after molann_dev_opes_table_f64.inc.  What an
// OPES run with walls, a table or a wider model carries at every step with nothing read back: frames_value_bias_opes_table_f64_kernel is
// frames_value_bias_opes_f64_kernel (molann_dev_bias_opes_f64.inc) on a device-resident kernel table whose live count and normalisation
// it reads from the table's state (molann_value_and_bias_opes_table_f64 launches it), and opes_step_columns_f64_kernel is
// opes_step_f64_kernel (molann_dev_opes_table_f64.inc) reading the walkers from the [W, out_dim] outputs and the [W, 4] energies that
// launch wrote (molann_opes_step_columns_f64).  Instances of their own: the kernels they follow keep their code.
// The step with adaptive sigma and the explore variant: molann_dev_opes_adaptive_f64.inc.  Out of scope: hills and OPES in one launch;
// walkers on several ranks; float32; a step on more than one block; a GraphedForces wrapper.
namespace {

// =============================================================================================
// frames_value_bias_opes_table_f64_kernel<G>: frames_value_bias_opes_f64_kernel with n_kernels and norm taken from
// state[4] = (n, S, merges, refused) in device memory, exactly as frames_value_opes_table_f64_kernel takes them: once, before the frame
// loop, every lane forms n = opes_live_count_f64(state[0], capacity) and, where n >= 1, norm = opes_table_norm_f64(state[1], n) - two
// uniform loads and one division per launch, none of them inside the frame loop.  sigma has a row per kernel (stride n_oc).  The gather
// into ysel, the restraint, the walk (frame_opes_walk_f64), opes_transform_f64, the stencil, the order of the additions into cot
// (restraint, OPES, table), the four energies (E_r, 0, V_g, V_o) and steps 4-6 are that kernel's, through the same device functions: for
// the same n and norm the outputs are its bits.  n == 0: no walk, no table pointer read, norm not formed, V_o = scale log(epsilon), the
// OPES share of cot exactly 0.  A state whose S is not finite and > 0 while n >= 1 gives NaN or inf for every frame: the state is the
// caller's.
// =============================================================================================
struct BiasOpesTableF64Args : VjpF64Args {
    int has_restraint;            // != 0: center and kappa are read
    int n_oc, n_gc;               // the OPES term's and the table's column counts; n_gc == 0: the table is absent
    int oc[HILLS_MAX_D];          // the outputs the kernels act on, in the order of the kernel table's columns
    int gc[GRID_MAX_D];           // the outputs the table's axes are, axis 0 (the slowest) first
    long center_stride;           // doubles between the frames' rows of center: 0 or d_out
    long capacity;                // the kernel table's rows; the live count comes from state[0], held to [0, capacity]
    double scale, epsilon, cutoff;
    long n[GRID_MAX_D];           // the grid, as GridF64Args
    double lower[GRID_MAX_D];
    double h[GRID_MAX_D];
    int periodic[GRID_MAX_D];
};

template <int G>
__global__ __launch_bounds__(256) void frames_value_bias_opes_table_f64_kernel(
    const double* __restrict__ x, const double* __restrict__ center, const double* __restrict__ kappa, const double* __restrict__ rperiod,
    const double* __restrict__ flat, const double* __restrict__ centers, const double* __restrict__ heights, const double* __restrict__ sigma,
    const double* __restrict__ state, const double* __restrict__ operiod, const double* __restrict__ table, double* __restrict__ out,
    double* __restrict__ energies, double* __restrict__ gx, const int* __restrict__ align_idx, const double* __restrict__ ref64,
    const ItemDev* __restrict__ items, const int* __restrict__ hv_ptr, const int* __restrict__ hv_list, BiasOpesTableF64Args a, F64Mlp m) {
    static_assert(G == 8 || G == 16 || G == 32 || G == 64, "lane group of 8..64");
    static_assert(HILLS_MAX_D <= G && GRID_MAX_D <= G, "lane j of a group gathers and scatters column j of a list");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int gl = threadIdx.x & (G - 1);
    const int slot = threadIdx.x / G;
    const long per_block = blockDim.x / G;
    const long frame_dw = 3l * a.n_inp;
    const bool has_align = a.n_align > 0;
    const bool has_head = m.n_layers > 0;
    // the kernel table's state: the same two values in every lane
    const long n_kernels = opes_live_count_f64(state[0], a.capacity);
    double norm = 1.0;      // n == 0: P = 0 and zero sums, whatever the norm
    if (n_kernels > 0) norm = opes_table_norm_f64(state[1], n_kernels);
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
        const double p = frame_opes_walk_f64<G>(ysel, centers, heights, sigma, operiod, n_kernels, (long)a.n_oc, a.cutoff, a.n_oc, gl, acc_o);
        double dv[HILLS_MAX_D];
        const double vo = opes_transform_f64(p, acc_o, a.scale, norm, a.epsilon, a.n_oc, dv);
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

// =============================================================================================
// opes_step_columns_f64_kernel: opes_step_f64_kernel with a strided, column-mapped reading of the walkers - walker a's centre is
// y[a * y_stride + col[k]], k < d, and its bias V[a * v_stride], so the out[W, out_dim] and column 3 of the energies[W, 4] that a
// frames_value_bias_opes_table_f64_kernel launch wrote are read in place.  The executor gathers a walker's d chosen outputs into
// registers (col is carried by value: comparisons on a compile-time k, no indexed register array) and hands them to
// opes_walker_weight_f64 and opes_walker_height_f64 as they are, so a walker's validity looks at V and its d chosen outputs only, and
// for the same walkers the table, state and run are opes_step_f64_kernel's on the gathered copy, bit for bit.  Everything else - the
// sums' order, opes_step_steps_f64, the deposit executor, thread 0's stores - is that kernel's.
// =============================================================================================
struct OpesStepColumnsDev : OpesStepDev {       // its fields and its block_sum; new_centers is y
    long y_stride, v_stride;
    int col[HILLS_MAX_D];

    __device__ __forceinline__ void gather(long a, double (&yc)[HILLS_MAX_D]) const {
        const double* row = new_centers + a * y_stride;
#pragma unroll
        for (int k = 0; k < HILLS_MAX_D; ++k) yc[k] = k < d ? row[col[k]] : 0.0;
    }
    __device__ __forceinline__ void walker_sums(long n_walkers, double& count, double& sum_w, double& sum_w2) const {
        double pc = 0.0, pw = 0.0, pw2 = 0.0;
        for (long a = threadIdx.x; a < n_walkers; a += 256) {
            double w, yc[HILLS_MAX_D];
            gather(a, yc);
            if (opes_walker_weight_f64(beta, V[a * v_stride], yc, d, w)) opes_walker_add_f64(w, pc, pw, pw2);
        }
        count = block_sum(pc);
        sum_w = block_sum(pw);
        sum_w2 = block_sum(pw2);
    }
    __device__ __forceinline__ void load_new(long a, double (&c)[HILLS_MAX_D], double (&s)[HILLS_MAX_D], double& h) const {
        gather(a, c);
#pragma unroll
        for (int k = 0; k < HILLS_MAX_D; ++k) s[k] = k < d ? step_sigma[k] : 1.0;
        h = opes_walker_height_f64(beta, V[a * v_stride], c, d, ratio);
    }
};

struct OpesStepColumns {    // the column list of a step, by value
    int col[HILLS_MAX_D];
};

__global__ __launch_bounds__(256) void opes_step_columns_f64_kernel(double* centers, double* sigma, double* heights, long capacity, int d,
                                                                    const double* period, double* state, double* run, const double* y,
                                                                    long y_stride, OpesStepColumns cols, const double* V, long v_stride,
                                                                    long n_walkers, const double* sigma0, const double* sigma_min, double beta,
                                                                    double threshold, double cutoff, int fixed_sigma) {
    __shared__ double red_q[4];
    __shared__ long long red_k[4];
    OpesStepColumnsDev ex = {{{centers, sigma, heights, period, y, nullptr, nullptr, d, red_q, red_k}, V, beta, 1.0, {1., 1., 1., 1., 1., 1., 1., 1.}},
                             y_stride, v_stride, {cols.col[0], cols.col[1], cols.col[2], cols.col[3], cols.col[4], cols.col[5], cols.col[6], cols.col[7]}};
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
