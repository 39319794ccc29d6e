// molann_metad_deposit_f64.inc - part of libmolann_hip.so, included by molann_kernels.hip after molann_opes_deposit_f64.inc.  The host side
// of molann_dev_metad_deposit_f64.inc (see include/molann_hip.h): molann_metad_deposit_f64 checks its arguments and enqueues one launch -
// no plan, no workspace, no event - and molann_selftest_metad_deposit_f64 runs the same step on host arrays, tile by tile and walker by
// walker through the functions the kernel calls.
namespace {

// the arguments molann_metad_deposit_f64 and its host twin share, in the order of the refusals; then the kernel's arguments are in `a`
inline int metad_deposit_arguments(double* table, int32_t d, const int64_t* shape, const double* lower, const double* spacing, const int32_t* periodic,
                                   const double* sigma, const int32_t* columns, const double* y, int64_t y_stride, const double* V, int64_t v_stride,
                                   int64_t n_walkers, double height0, double inv_dT, double cutoff, double* state, double* log, int64_t log_capacity,
                                   MetadDepositArgs& a) {
    const bool arrays = shape && lower && spacing && sigma;
    if (n_walkers > 0 && (!table || !state || !y || !V || !arrays)) return MOLANN_E_NULL;
    if (((uintptr_t)table | (uintptr_t)state | (uintptr_t)y | (uintptr_t)V | (uintptr_t)log) & 7) return MOLANN_E_ALIGNMENT;
    if (d < 1 || d > GRID_MAX_D) return MOLANN_E_UNSUPPORTED;
    int per[GRID_MAX_D];
    if (arrays) {
        if (!grid_geometry_f64(d, shape, lower, spacing, periodic, a.n, a.lower, a.h, per)) return MOLANN_E_DESC;
        for (int k = 0; k < d; ++k)
            if (!std::isfinite(sigma[k]) || !(sigma[k] > 0.0)) return MOLANN_E_DESC;
    }
    if (!std::isfinite(height0) || !(height0 > 0.0)) return MOLANN_E_DESC;
    if (!std::isfinite(inv_dT) || !(inv_dT >= 0.0)) return MOLANN_E_DESC;
    if (!(cutoff > 0.0)) return MOLANN_E_DESC;
    if (y_stride < 0 || v_stride < 0 || n_walkers < 0 || log_capacity < 0) return MOLANN_E_DESC;
    for (int k = 0; k < d; ++k) {
        const int64_t c = columns ? columns[k] : k;
        if (c < 0 || c >= y_stride) return MOLANN_E_DESC;
    }
    if (n_walkers == 0) return MOLANN_OK;
    a.table = table; a.state = state; a.log = log; a.y = y; a.V = V;
    for (int k = 0; k < GRID_MAX_D; ++k) {
        a.P[k] = k < d && per[k] ? (double)a.n[k] * a.h[k] : 0.0;
        a.sigma[k] = k < d ? sigma[k] : 1.0;
        a.col[k] = k < d ? (columns ? columns[k] : k) : 0;
    }
    a.y_stride = (long)y_stride; a.v_stride = (long)v_stride; a.n_walkers = (long)n_walkers; a.log_capacity = log ? (long)log_capacity : 0;
    a.height0 = height0; a.inv_dT = inv_dT; a.c2 = cutoff * cutoff;
    return MOLANN_OK;
}

// the tiles of the table, metad_tile_extent(d, k) points along axis k: how many along each axis, and in all
inline long metad_tiles(const MetadDepositArgs& a, int d, long (&tiles)[GRID_MAX_D]) {
    long all = 1;
    for (int k = 0; k < GRID_MAX_D; ++k) {
        tiles[k] = k < d ? (a.n[k] + metad_tile_extent(d, k) - 1) / metad_tile_extent(d, k) : 1;
        all *= tiles[k];
    }
    return all;
}

// metad_deposit_f64_kernel's step on the host: per tile the walkers that reach it, per entry their terms in the walkers' order
inline void metad_deposit_host(const MetadDepositArgs& a, int d) {
    const long W = a.n_walkers;
    std::vector<double> h(W), yv(W * GRID_MAX_D, 0.0);
    std::vector<char> valid(W), reach(W);
    double hills = a.state[0], refused = a.state[1], sum_heights = a.state[2];
    long logged = a.log ? opes_live_count_f64(a.state[4], a.log_capacity) : a.log_capacity;
    for (long w = 0; w < W; ++w) {
        const double V = a.V[w * a.v_stride];
        double y[GRID_MAX_D] = {0., 0., 0.};
        for (int k = 0; k < d; ++k) y[k] = yv[w * GRID_MAX_D + k] = a.y[w * a.y_stride + a.col[k]];
        h[w] = metad_height_f64(a.height0, V, a.inv_dT);
        valid[w] = metad_walker_valid_f64(V, y, h[w], d);
        metad_state_walker_f64(valid[w] != 0, h[w], y, a.sigma, d, a.log, a.log_capacity, hills, refused, sum_heights, logged);
    }
    long tiles[GRID_MAX_D];
    const long all = metad_tiles(a, d, tiles);
    for (long b = 0; b < all; ++b) {
        long i0[GRID_MAX_D] = {0, 0, 0}, i1[GRID_MAX_D] = {0, 0, 0};
        long r = b;
        for (int k = d - 1; k >= 0; --k) {
            const int T = metad_tile_extent(d, k);
            i0[k] = (r % tiles[k]) * T;
            r /= tiles[k];
            i1[k] = std::min<long>(i0[k] + T - 1, a.n[k] - 1);
        }
        bool any = false;
        for (long w = 0; w < W; ++w) {
            double qk[GRID_MAX_D] = {0., 0., 0.};
            for (int k = 0; k < d; ++k)
                qk[k] = metad_axis_reach_f64(i0[k], i1[k], yv[w * GRID_MAX_D + k], a.lower[k], a.h[k], a.P[k], a.sigma[k]);
            reach[w] = valid[w] && metad_q_f64(qk, d) <= a.c2;
            any = any || reach[w];
        }
        if (!any) continue;
        long idx[GRID_MAX_D] = {0, 0, 0};
        for (idx[0] = i0[0]; idx[0] <= i1[0]; ++idx[0])
            for (idx[1] = i0[1]; idx[1] <= i1[1]; ++idx[1])
                for (idx[2] = i0[2]; idx[2] <= i1[2]; ++idx[2]) {
                    long off = 0;
                    for (int k = 0; k < d; ++k) off = off * a.n[k] + idx[k];
                    double acc = a.table[off];
                    bool touched = false;
                    for (long w = 0; w < W; ++w) {
                        if (!reach[w]) continue;
                        double q[GRID_MAX_D] = {0., 0., 0.}, e[GRID_MAX_D] = {1., 1., 1.};
                        for (int k = 0; k < d; ++k)
                            metad_axis_factor_f64(metad_axis_delta_f64(idx[k], yv[w * GRID_MAX_D + k], a.lower[k], a.h[k], a.P[k]), a.sigma[k], q[k], e[k]);
                        if (metad_q_f64(q, d) <= a.c2) {
                            acc = acc + metad_term_f64(h[w], e, d);
                            touched = true;
                        }
                    }
                    if (touched) a.table[off] = acc;
                }
    }
    a.state[0] = hills; a.state[1] = refused; a.state[2] = sum_heights; a.state[3] = a.state[3] + 1.0;
    if (a.log) a.state[4] = (double)logged;
}

} // namespace

extern "C" {

int molann_metad_deposit_f64(double* table, int32_t d, const int64_t* shape, const double* lower, const double* spacing, const int32_t* periodic,
                             const double* sigma, const int32_t* columns, const double* y, int64_t y_stride, const double* V, int64_t v_stride,
                             int64_t n_walkers, double height0, double inv_dT, double cutoff, double* state, double* log, int64_t log_capacity,
                             molann_stream_t stream) {
    MetadDepositArgs a = {};
    const int e = metad_deposit_arguments(table, d, shape, lower, spacing, periodic, sigma, columns, y, y_stride, V, v_stride, n_walkers, height0,
                                          inv_dT, cutoff, state, log, log_capacity, a);
    if (e != MOLANN_OK || n_walkers == 0) return e;
    long tiles[GRID_MAX_D];
    const dim3 grid((unsigned)metad_tiles(a, d, tiles)), block(METAD_TILE);    // fewer than 2^31 points, so fewer tiles than that
    if (d == 1) hipLaunchKernelGGL(metad_deposit_f64_kernel<1>, grid, block, 0, (hipStream_t)stream, a);
    else if (d == 2) hipLaunchKernelGGL(metad_deposit_f64_kernel<2>, grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(metad_deposit_f64_kernel<3>, grid, block, 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int molann_selftest_metad_deposit_f64(double* table, int32_t d, const int64_t* shape, const double* lower, const double* spacing,
                                      const int32_t* periodic, const double* sigma, const int32_t* columns, const double* y, int64_t y_stride,
                                      const double* V, int64_t v_stride, int64_t n_walkers, double height0, double inv_dT, double cutoff,
                                      double* state, double* log, int64_t log_capacity) {
    MetadDepositArgs a = {};
    const int e = metad_deposit_arguments(table, d, shape, lower, spacing, periodic, sigma, columns, y, y_stride, V, v_stride, n_walkers, height0,
                                          inv_dT, cutoff, state, log, log_capacity, a);
    if (e != MOLANN_OK || n_walkers == 0) return e;
    metad_deposit_host(a, (int)d);
    return MOLANN_OK;
}

} // extern "C"
