// molann_metad_cov_f64.inc - part of libmolann_hip.so, included by molann_kernels.hip after molann_metad_rct_f64.inc.  The host side of
// molann_dev_metad_cov_f64.inc (see include/molann_hip.h): molann_metad_widths_f64 and molann_metad_deposit_cov_f64 check their arguments
// and enqueue one launch each - no plan, no workspace, no event - and the two selftests run the same steps on host arrays through the
// functions the kernels call.
namespace {

// the arguments molann_metad_widths_f64 and its host twin share, in the order of the refusals; then the kernel's arguments are in `a`
inline int metad_widths_arguments(int32_t d, const int64_t* shape, const double* lower, const double* spacing, const int32_t* periodic, const double* sigma,
                                  const double* sigma_min, const double* sigma_max, const int32_t* columns, const double* y, int64_t y_stride,
                                  const double* metric, int64_t metric_stride, int64_t metric_ld, int64_t n_walkers, int32_t mode, int64_t window,
                                  int32_t emit, double* adapt, double* adapt_state, double* cov_out, int64_t cov_stride, MetadWidthsArgs& a) {
    const bool arrays = shape && lower && spacing && sigma;
    const bool diff = mode == METAD_COV_DIFF, geom = mode == METAD_COV_GEOM;
    if (n_walkers > 0 && (!adapt_state || !arrays || (diff && (!y || !adapt)) || (geom && !metric) || (emit && !cov_out))) return MOLANN_E_NULL;
    if (((uintptr_t)adapt | (uintptr_t)adapt_state | (uintptr_t)cov_out | (uintptr_t)y | (uintptr_t)metric) & 7) return MOLANN_E_ALIGNMENT;
    if (d < 1 || d > GRID_MAX_D) return MOLANN_E_UNSUPPORTED;
    if (!diff && !geom) return MOLANN_E_DESC;
    long n[GRID_MAX_D];
    double h[GRID_MAX_D];
    int per[GRID_MAX_D];
    if (arrays) {
        if (!grid_geometry_f64(d, shape, lower, spacing, periodic, n, a.lower, h, per)) return MOLANN_E_DESC;
        for (int k = 0; k < d; ++k) {
            if (!std::isfinite(sigma[k]) || !(sigma[k] > 0.0)) return MOLANN_E_DESC;
            const double lo = sigma_min ? sigma_min[k] : 0.0, hi = sigma_max ? sigma_max[k] : INFINITY;
            if (!(lo >= 0.0) || !(hi >= lo) || !std::isfinite(lo)) return MOLANN_E_DESC;
        }
    }
    if (diff && window < 1) return MOLANN_E_DESC;
    if (y_stride < 0 || metric_stride < 0 || metric_ld < 0 || n_walkers < 0) return MOLANN_E_DESC;
    if (emit && cov_stride < metad_cov_len(d)) return MOLANN_E_DESC;
    for (int k = 0; k < d; ++k) {
        const int64_t c = columns ? columns[k] : k;
        if (c < 0 || (diff && c >= y_stride) || (geom && c >= metric_ld)) return MOLANN_E_DESC;
    }
    if (geom && metric_ld > 0 && metric_stride > 0 && metric_stride / metric_ld < metric_ld) return MOLANN_E_DESC;    // a walker's metric is ld x ld
    if (n_walkers == 0) return MOLANN_OK;
    a.adapt = diff ? adapt : nullptr; a.adapt_state = adapt_state; a.cov_out = cov_out; a.y = y; a.metric = metric;
    for (int k = 0; k < GRID_MAX_D; ++k) {
        a.P[k] = k < d && per[k] ? (double)n[k] * h[k] : 0.0;
        a.sigma[k] = k < d ? sigma[k] : 1.0;
        a.sigma_min[k] = k < d && sigma_min ? sigma_min[k] : 0.0;
        a.sigma_max[k] = k < d && sigma_max ? sigma_max[k] : INFINITY;
        a.col[k] = k < d ? (columns ? columns[k] : k) : 0;
    }
    a.y_stride = (long)y_stride; a.metric_stride = (long)metric_stride; a.metric_ld = (long)metric_ld; a.cov_stride = (long)cov_stride;
    a.n_walkers = (long)n_walkers;
    a.window = diff ? (double)window : 1.0; a.decay = diff ? 1.0 / (double)window : 1.0;
    a.d = (int)d; a.mode = (int)mode; a.emit = emit ? 1 : 0;
    return MOLANN_OK;
}

// the arguments molann_metad_deposit_cov_f64 and its host twin share, in the order of the refusals
inline int metad_deposit_cov_arguments(double* table, int32_t d, const int64_t* shape, const double* lower, const double* spacing, const int32_t* periodic,
                                       const int32_t* columns, const double* y, int64_t y_stride, const double* V, int64_t v_stride, const double* cov,
                                       int64_t cov_stride, int64_t n_walkers, double height0, double inv_dT, double cutoff, double* state, double* log,
                                       int64_t log_capacity, MetadDepositCovArgs& a) {
    const bool arrays = shape && lower && spacing;
    if (n_walkers > 0 && (!table || !state || !y || !V || !cov || !arrays)) return MOLANN_E_NULL;
    if (((uintptr_t)table | (uintptr_t)state | (uintptr_t)y | (uintptr_t)V | (uintptr_t)cov | (uintptr_t)log) & 7) return MOLANN_E_ALIGNMENT;
    if (d < 1 || d > GRID_MAX_D) return MOLANN_E_UNSUPPORTED;
    int per[GRID_MAX_D];
    if (arrays && !grid_geometry_f64(d, shape, lower, spacing, periodic, a.n, a.lower, a.h, per)) return MOLANN_E_DESC;
    if (!std::isfinite(height0) || !(height0 > 0.0)) return MOLANN_E_DESC;
    if (!std::isfinite(inv_dT) || !(inv_dT >= 0.0)) return MOLANN_E_DESC;
    if (!(cutoff > 0.0)) return MOLANN_E_DESC;
    if (y_stride < 0 || v_stride < 0 || n_walkers < 0 || log_capacity < 0) return MOLANN_E_DESC;
    if (cov_stride != 0 && cov_stride < metad_cov_len(d)) return MOLANN_E_DESC;    // 0: every walker reads one matrix
    for (int k = 0; k < d; ++k) {
        const int64_t c = columns ? columns[k] : k;
        if (c < 0 || c >= y_stride) return MOLANN_E_DESC;
    }
    if (n_walkers == 0) return MOLANN_OK;
    a.table = table; a.state = state; a.log = log; a.y = y; a.V = V; a.cov = cov;
    for (int k = 0; k < GRID_MAX_D; ++k) {
        a.P[k] = k < d && per[k] ? (double)a.n[k] * a.h[k] : 0.0;
        a.col[k] = k < d ? (columns ? columns[k] : k) : 0;
    }
    a.y_stride = (long)y_stride; a.v_stride = (long)v_stride; a.cov_stride = (long)cov_stride; a.n_walkers = (long)n_walkers;
    a.log_capacity = log ? (long)log_capacity : 0;
    a.height0 = height0; a.inv_dT = inv_dT; a.c2 = cutoff * cutoff;
    return MOLANN_OK;
}

// metad_widths_f64_kernel's step on the host
inline void metad_widths_host(const MetadWidthsArgs& a) {
    long skipped = 0;
    for (long w = 0; w < a.n_walkers; ++w) skipped += metad_widths_walker_f64(a, w);
    metad_widths_state_f64(a, skipped);
}

// metad_deposit_cov_f64_kernel's step on the host: per tile the walkers that reach it, per entry their terms in the walkers' order
inline void metad_deposit_cov_host(const MetadDepositCovArgs& a, int d) {
    const long W = a.n_walkers;
    std::vector<double> h(W), yv(W * GRID_MAX_D, 0.0), Cv(W * METAD_COV_MAX_T), Lv(W * METAD_COV_MAX_T);
    std::vector<char> valid(W), reach(W);
    double hills = a.state[0], refused = a.state[1], sum_heights = a.state[2];
    long logged = a.log ? opes_live_count_f64(a.state[4], a.log_capacity) : a.log_capacity;
    for (long w = 0; w < W; ++w) {
        const double V = a.V[w * a.v_stride];
        double y[GRID_MAX_D] = {0., 0., 0.}, C[METAD_COV_MAX_T], L[METAD_COV_MAX_T];
        for (int k = 0; k < d; ++k) y[k] = yv[w * GRID_MAX_D + k] = a.y[w * a.y_stride + a.col[k]];
        metad_cov_load_f64(a.cov + w * a.cov_stride, d, C);
        const bool usable = metad_cov_factor_f64(C, d, L);
        for (int k = 0; k < METAD_COV_MAX_T; ++k) { Cv[w * METAD_COV_MAX_T + k] = C[k]; Lv[w * METAD_COV_MAX_T + k] = L[k]; }
        h[w] = metad_height_f64(a.height0, V, a.inv_dT);
        valid[w] = metad_walker_valid_f64(V, y, h[w], d) && usable;
        metad_cov_state_walker_f64(valid[w] != 0, h[w], y, C, d, a.log, a.log_capacity, hills, refused, sum_heights, logged);
    }
    long tiles[GRID_MAX_D] = {1, 1, 1};
    long all = 1;
    for (int k = 0; k < d; ++k) {
        tiles[k] = (a.n[k] + metad_tile_extent(d, k) - 1) / metad_tile_extent(d, k);
        all *= tiles[k];
    }
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
            double y[GRID_MAX_D], C[METAD_COV_MAX_T];
            for (int k = 0; k < GRID_MAX_D; ++k) y[k] = yv[w * GRID_MAX_D + k];
            for (int k = 0; k < METAD_COV_MAX_T; ++k) C[k] = Cv[w * METAD_COV_MAX_T + k];
            reach[w] = valid[w] && metad_cov_reach_f64(i0, i1, y, a.lower, a.h, a.P, C, d, a.c2);
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
                        double delta[GRID_MAX_D] = {0., 0., 0.}, L[METAD_COV_MAX_T];
                        for (int k = 0; k < d; ++k) delta[k] = metad_axis_delta_f64(idx[k], yv[w * GRID_MAX_D + k], a.lower[k], a.h[k], a.P[k]);
                        for (int k = 0; k < METAD_COV_MAX_T; ++k) L[k] = Lv[w * METAD_COV_MAX_T + k];
                        const double q = metad_cov_q_f64(delta, L, d);
                        if (q <= a.c2) {
                            acc = acc + metad_cov_term_f64(h[w], q);
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

int molann_metad_widths_f64(int32_t d, const int64_t* shape, const double* lower, const double* spacing, const int32_t* periodic, const double* sigma,
                            const double* sigma_min, const double* sigma_max, const int32_t* columns, const double* y, int64_t y_stride,
                            const double* metric, int64_t metric_stride, int64_t metric_ld, int64_t n_walkers, int32_t mode, int64_t window, int32_t emit,
                            double* adapt, double* adapt_state, double* cov_out, int64_t cov_stride, molann_stream_t stream) {
    MetadWidthsArgs a = {};
    const int e = metad_widths_arguments(d, shape, lower, spacing, periodic, sigma, sigma_min, sigma_max, columns, y, y_stride, metric, metric_stride,
                                         metric_ld, n_walkers, mode, window, emit, adapt, adapt_state, cov_out, cov_stride, a);
    if (e != MOLANN_OK || n_walkers == 0) return e;
    hipLaunchKernelGGL(metad_widths_f64_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int molann_selftest_metad_widths_f64(int32_t d, const int64_t* shape, const double* lower, const double* spacing, const int32_t* periodic,
                                     const double* sigma, const double* sigma_min, const double* sigma_max, const int32_t* columns, const double* y,
                                     int64_t y_stride, const double* metric, int64_t metric_stride, int64_t metric_ld, int64_t n_walkers, int32_t mode,
                                     int64_t window, int32_t emit, double* adapt, double* adapt_state, double* cov_out, int64_t cov_stride) {
    MetadWidthsArgs a = {};
    const int e = metad_widths_arguments(d, shape, lower, spacing, periodic, sigma, sigma_min, sigma_max, columns, y, y_stride, metric, metric_stride,
                                         metric_ld, n_walkers, mode, window, emit, adapt, adapt_state, cov_out, cov_stride, a);
    if (e != MOLANN_OK || n_walkers == 0) return e;
    metad_widths_host(a);
    return MOLANN_OK;
}

int molann_metad_deposit_cov_f64(double* table, int32_t d, const int64_t* shape, const double* lower, const double* spacing, const int32_t* periodic,
                                 const int32_t* columns, const double* y, int64_t y_stride, const double* V, int64_t v_stride, const double* cov,
                                 int64_t cov_stride, int64_t n_walkers, double height0, double inv_dT, double cutoff, double* state, double* log,
                                 int64_t log_capacity, molann_stream_t stream) {
    MetadDepositCovArgs a = {};
    const int e = metad_deposit_cov_arguments(table, d, shape, lower, spacing, periodic, columns, y, y_stride, V, v_stride, cov, cov_stride, n_walkers,
                                              height0, inv_dT, cutoff, state, log, log_capacity, a);
    if (e != MOLANN_OK || n_walkers == 0) return e;
    long tiles = 1;
    for (int k = 0; k < d; ++k) tiles *= (a.n[k] + metad_tile_extent(d, k) - 1) / metad_tile_extent(d, k);
    const dim3 grid((unsigned)tiles), block(METAD_TILE);    // fewer than 2^31 points, so fewer tiles than that
    if (d == 1) hipLaunchKernelGGL(metad_deposit_cov_f64_kernel<1>, grid, block, 0, (hipStream_t)stream, a);
    else if (d == 2) hipLaunchKernelGGL(metad_deposit_cov_f64_kernel<2>, grid, block, 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(metad_deposit_cov_f64_kernel<3>, grid, block, 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int molann_selftest_metad_deposit_cov_f64(double* table, int32_t d, const int64_t* shape, const double* lower, const double* spacing,
                                          const int32_t* periodic, const int32_t* columns, const double* y, int64_t y_stride, const double* V,
                                          int64_t v_stride, const double* cov, int64_t cov_stride, int64_t n_walkers, double height0, double inv_dT,
                                          double cutoff, double* state, double* log, int64_t log_capacity) {
    MetadDepositCovArgs a = {};
    const int e = metad_deposit_cov_arguments(table, d, shape, lower, spacing, periodic, columns, y, y_stride, V, v_stride, cov, cov_stride, n_walkers,
                                              height0, inv_dT, cutoff, state, log, log_capacity, a);
    if (e != MOLANN_OK || n_walkers == 0) return e;
    metad_deposit_cov_host(a, (int)d);
    return MOLANN_OK;
}

} // extern "C"
