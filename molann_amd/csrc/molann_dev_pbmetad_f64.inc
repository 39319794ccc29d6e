// molann_dev_pbmetad_f64.inc - part of libmolann_hip.so, included by molann_kernels.hip after molann_dev_metad_cov_f64.inc.  Float64
// values, a parallel-bias metadynamics bias on up to PBMETAD_MAX_K chosen outputs - K one-dimensional tables joined by a soft minimum
// (molann_pbmetad.h) - an optional restraint on all outputs, and the gradient of their sum in one launch (molann_value_and_pbmetad_f64
// launches it).
namespace {

// =============================================================================================
// frames_value_pbmetad_f64_kernel<G>: x[N, n_inp, 3] -> y[N, d_out] = frames_value_vjp_f64_kernel's y, bit for bit,
// energies[N, e_stride >= 2 + K] = (E_r, V_PB, V_0 .. V_{K-1}) and gx[N, n_inp, 3] = J(x)^T (dE_r/dy + dV_PB/dy), everything in double:
//   E_r  = the restraint of frames_value_restraint_f64_kernel on all d_out outputs; absent (has_restraint == 0, a uniform branch on the
//          arguments): exactly 0 and none of its pointers is read,
//   V_k  = table k's Catmull-Rom interpolant at output col[k] (pbmetad_axis_value_f64), V_PB their soft minimum at kT with the weights
//          w_k (pbmetad_softmin_f64), dV_PB/dy[col[k]] = w_k V_k'.
// Lanes, grid-stride loop, rows and steps 1-6 are frame_value_term_loop_f64's (molann_dev_vjp_f64.inc) on the row geometry of
// frames_value_bias_f64_kernel: a frame's rows carry BIAS_SEL more doubles than the loop uses, ysel, which lie between the hidden
// layers' rows and the two rows of the widest layer input (the loop places those two at the end of the frame's rows).  The term:
//   3p. lane j < K gathers ysel[j] = cot[col[j]]; after a sync the restraint's loop stores y and leaves its dy (0 without one) in cot;
//       lane j takes its axis step, four unconditional loads and the two sums and leaves V_j in ysel[j], whose only reader it was.  After a
//       sync every lane reads the K values as a broadcast and forms m, S and w in the one order of pbmetad_softmin_f64; lane j adds
//       w_j V_j' into cot[col[j]] - the columns are distinct, so no two lanes meet - and lane 0 stores the energies' row.
// Every sum has a fixed order: the same bits on every run, whatever N and the frame's slot in its block.  Every table index is in range
// for every bit pattern of y (grid_axis_f64); a V_k that is not finite makes this frame's V_PB and gx NaN and no other frame's.
// The column list, the K grids, their offsets in the table and kT travel by value in the arguments.
// =============================================================================================
struct PbmetadF64Args : VjpF64Args {
    int has_restraint;                // != 0: center and kappa are read
    int K;
    int col[PBMETAD_MAX_K];           // the output that axis k biases
    int periodic[PBMETAD_MAX_K];
    long n[PBMETAD_MAX_K];            // points of table k
    long off[PBMETAD_MAX_K];          // where table k starts: sum_{j < k} n_j
    double lower[PBMETAD_MAX_K];
    double h[PBMETAD_MAX_K];
    long center_stride;               // doubles between the frames' rows of center: 0 or d_out
    long e_stride;                    // doubles between the frames' rows of energies: >= 2 + K
    double kT;
};

template <int G>
__global__ __launch_bounds__(256) void frames_value_pbmetad_f64_kernel(
    const double* __restrict__ x, const double* __restrict__ center, const double* __restrict__ kappa, const double* __restrict__ rperiod,
    const double* __restrict__ flat, const double* __restrict__ table, double* __restrict__ out, double* __restrict__ energies,
    double* __restrict__ gx, const int* __restrict__ align_idx, const double* __restrict__ ref64, const ItemDev* __restrict__ items,
    const int* __restrict__ hv_ptr, const int* __restrict__ hv_list, PbmetadF64Args a, F64Mlp m) {
    static_assert(PBMETAD_MAX_K <= G && PBMETAD_MAX_K <= BIAS_SEL, "lane j of a group owns axis j and word j of the selection row");
    frame_value_term_loop_f64<G>(x, out, gx, align_idx, ref64, items, hv_ptr, hv_list, a, m, blockDim.x,
                                 [&](long f, int gl, double* cot, double* of) __attribute__((always_inline)) {
        // ---- 3p. the parallel bias on the chosen outputs
        double* ysel = cot + (a.lds_per_frame - 2 * a.max_w - BIAS_SEL);
        // this lane's axis, by comparisons (the arguments' arrays stay in scalar registers)
        int col = 0, per = 0;
        long n = 4, off = 0;
        double lower = 0., h = 1.;
#pragma unroll
        for (int j = 0; j < PBMETAD_MAX_K; ++j)
            if (gl == j) { col = a.col[j]; per = a.periodic[j]; n = a.n[j]; off = a.off[j]; lower = a.lower[j]; h = a.h[j]; }
        const bool mine = gl < a.K;
        if (mine) ysel[gl] = cot[col];
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
        double dv = 0.;
        if (mine) {
            double v;
            pbmetad_axis_value_f64(ysel[gl], table + off, n, lower, h, per != 0, v, dv);
            ysel[gl] = v;
        }
        lds_wave_sync();   // the K values are whole, and so is the restraint's cot
        double V[PBMETAD_MAX_K], w[PBMETAD_MAX_K];
#pragma unroll
        for (int k = 0; k < PBMETAD_MAX_K; ++k) V[k] = k < a.K ? ysel[k] : 0.;
        const double vpb = pbmetad_softmin_f64(V, a.K, a.kT, w);
        double wj = 0.;
#pragma unroll
        for (int j = 0; j < PBMETAD_MAX_K; ++j)
            if (gl == j) wj = w[j];
        if (mine) cot[col] = pbmetad_cotangent_f64(cot[col], wj, dv);
        if (gl == 0) {
            double* ef = energies + f * a.e_stride;
            ef[0] = e; ef[1] = vpb;
#pragma unroll
            for (int k = 0; k < PBMETAD_MAX_K; ++k)
                if (k < a.K) ef[2 + k] = V[k];
        }
    });
}

} // namespace
