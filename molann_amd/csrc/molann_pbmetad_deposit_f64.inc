// molann_pbmetad_deposit_f64.inc - part of libmolann_hip.so, included by molann_kernels.hip after molann_metad_cov_f64.inc.  The host side of
// molann_dev_pbmetad_deposit_f64.inc (see include/molann_hip.h): molann_pbmetad_deposit_f64 checks its arguments and enqueues one launch -
// no plan, no workspace, no event - and molann_selftest_pbmetad_deposit_f64 runs the same step on host arrays, axis by axis, tile by tile
// and walker by walker through the functions the kernel calls.
namespace {

// the arguments molann_pbmetad_deposit_f64 and its host twin share, in the order of the refusals (molann_metad_deposit_f64's, extended to
// K axes); then the kernel's arguments are in `a`
inline int pbmetad_deposit_arguments(double* table, int32_t K, const int64_t* shape, const double* lower, const double* spacing,
                                     const int32_t* periodic, const double* sigma, const int32_t* columns, const double* y, int64_t y_stride,
                                     const double* V, int64_t v_stride, int64_t n_walkers, double height0, double inv_dT, double kT, double cutoff,
                                     double* state, double* log, int64_t log_capacity, PbmetadDepositArgs& a) {
    const bool arrays = shape && lower && spacing && sigma;
    if (n_walkers > 0 && (!table || !state || !y || !V || !arrays)) return MOLANN_E_NULL;
    if (((uintptr_t)table | (uintptr_t)state | (uintptr_t)y | (uintptr_t)V | (uintptr_t)log) & 7) return MOLANN_E_ALIGNMENT;
    if (K < 1 || K > PBMETAD_MAX_K) return MOLANN_E_UNSUPPORTED;
    int per[PBMETAD_MAX_K] = {};
    if (arrays) {
        int64_t entries = 0;
        for (int k = 0; k < K; ++k) {
            long n1[GRID_MAX_D];
            double lo1[GRID_MAX_D], h1[GRID_MAX_D];
            int per1[GRID_MAX_D];
            const int32_t periodic_k = periodic ? periodic[k] : 0;
            if (!grid_geometry_f64(1, shape + k, lower + k, spacing + k, &periodic_k, n1, lo1, h1, per1)) return MOLANN_E_DESC;
            a.n[k] = n1[0]; a.lower[k] = lo1[0]; a.h[k] = h1[0]; per[k] = per1[0];
            a.off[k] = (long)entries;
            entries += shape[k];
            if (entries >= (int64_t(1) << 31)) return MOLANN_E_DESC;
        }
        for (int k = 0; k < K; ++k)
            if (!std::isfinite(sigma[k]) || !(sigma[k] > 0.0)) return MOLANN_E_DESC;
    }
    if (!std::isfinite(height0) || !(height0 > 0.0)) return MOLANN_E_DESC;
    if (!std::isfinite(inv_dT) || !(inv_dT >= 0.0)) return MOLANN_E_DESC;
    if (!std::isfinite(kT) || !(kT > 0.0)) return MOLANN_E_DESC;
    if (!(cutoff > 0.0)) return MOLANN_E_DESC;
    if (y_stride < 0 || v_stride < K || n_walkers < 0 || log_capacity < 0) return MOLANN_E_DESC;
    for (int k = 0; k < K; ++k) {
        const int64_t c = columns ? columns[k] : k;
        if (c < 0 || c >= y_stride) return MOLANN_E_DESC;
        for (int j = 0; j < k; ++j)
            if (c == (columns ? columns[j] : j)) return MOLANN_E_INDEX;
    }
    if (n_walkers == 0) return MOLANN_OK;
    a.table = table; a.state = state; a.log = log; a.y = y; a.V = V;
    for (int k = 0; k < PBMETAD_MAX_K; ++k) {
        if (k >= K) { a.n[k] = 4; a.off[k] = 0; a.lower[k] = 0.0; a.h[k] = 1.0; }
        a.P[k] = k < K && per[k] ? (double)a.n[k] * a.h[k] : 0.0;
        a.sigma[k] = k < K ? sigma[k] : 1.0;
        a.col[k] = k < K ? (columns ? columns[k] : k) : 0;
    }
    a.K = K;
    a.y_stride = (long)y_stride; a.v_stride = (long)v_stride; a.n_walkers = (long)n_walkers; a.log_capacity = log ? (long)log_capacity : 0;
    a.height0 = height0; a.inv_dT = inv_dT; a.kT = kT; a.c2 = cutoff * cutoff;
    return MOLANN_OK;
}

inline long pbmetad_deposit_blocks(const PbmetadDepositArgs& a) {
    long all = 0;
    for (int k = 0; k < a.K; ++k) all += pbmetad_axis_tiles(a.n[k]);
    return all;
}

// pbmetad_deposit_f64_kernel's step on the host: per axis and tile the walkers that reach it, per entry their terms in the walkers' order
inline void pbmetad_deposit_host(const PbmetadDepositArgs& a) {
    const long W = a.n_walkers;
    const int K = a.K;
    std::vector<double> hv(W * PBMETAD_MAX_K), yv(W * PBMETAD_MAX_K);
    std::vector<char> valid(W), reach(W);
    double hills = a.state[0], refused = a.state[1], sum_heights = a.state[2];
    long logged = a.log ? opes_live_count_f64(a.state[4], a.log_capacity) : a.log_capacity;
    for (long w = 0; w < W; ++w) {
        double V[PBMETAD_MAX_K], y[PBMETAD_MAX_K], hk[PBMETAD_MAX_K];
        for (int k = 0; k < PBMETAD_MAX_K; ++k) {
            V[k] = k < K ? a.V[w * a.v_stride + k] : 0.;
            y[k] = k < K ? a.y[w * a.y_stride + a.col[k]] : 0.;
        }
        valid[w] = pbmetad_walker_heights_f64(V, y, K, a.height0, a.inv_dT, a.kT, hk);
        for (int k = 0; k < PBMETAD_MAX_K; ++k) { hv[w * PBMETAD_MAX_K + k] = hk[k]; yv[w * PBMETAD_MAX_K + k] = y[k]; }
        pbmetad_state_walker_f64(valid[w] != 0, hk, y, K, a.log, a.log_capacity, hills, refused, sum_heights, logged);
    }
    for (int k = 0; k < K; ++k)
        for (long tile = 0; tile < pbmetad_axis_tiles(a.n[k]); ++tile) {
            const long i0 = tile * METAD_TILE, i1 = std::min<long>(i0 + METAD_TILE - 1, a.n[k] - 1);
            bool any = false;
            for (long w = 0; w < W; ++w) {
                reach[w] = valid[w] && pbmetad_axis_reaches_f64(hv[w * PBMETAD_MAX_K + k], i0, i1, yv[w * PBMETAD_MAX_K + k], a.lower[k], a.h[k],
                                                                a.P[k], a.sigma[k], a.c2);
                any = any || reach[w];
            }
            if (!any) continue;
            for (long i = i0; i <= i1; ++i) {
                double acc = a.table[a.off[k] + i];
                bool touched = false;
                for (long w = 0; w < W; ++w)
                    if (reach[w] && pbmetad_entry_add_f64(i, hv[w * PBMETAD_MAX_K + k], yv[w * PBMETAD_MAX_K + k], a.lower[k], a.h[k], a.P[k],
                                                          a.sigma[k], a.c2, acc))
                        touched = true;
                if (touched) a.table[a.off[k] + i] = acc;
            }
        }
    a.state[0] = hills; a.state[1] = refused; a.state[2] = sum_heights; a.state[3] = a.state[3] + 1.0;
    if (a.log) a.state[4] = (double)logged;
}

} // namespace

extern "C" {

int molann_pbmetad_deposit_f64(double* table, int32_t n_axes, const int64_t* shape, const double* lower, const double* spacing,
                               const int32_t* periodic, const double* sigma, const int32_t* columns, const double* y, int64_t y_stride,
                               const double* V, int64_t v_stride, int64_t n_walkers, double height0, double inv_dT, double kT, double cutoff,
                               double* state, double* log, int64_t log_capacity, molann_stream_t stream) {
    PbmetadDepositArgs a = {};
    const int e = pbmetad_deposit_arguments(table, n_axes, shape, lower, spacing, periodic, sigma, columns, y, y_stride, V, v_stride, n_walkers,
                                            height0, inv_dT, kT, cutoff, state, log, log_capacity, a);
    if (e != MOLANN_OK || n_walkers == 0) return e;
    const dim3 grid((unsigned)pbmetad_deposit_blocks(a)), block(METAD_TILE);    // fewer than 2^31 entries, so fewer tiles than that
    hipLaunchKernelGGL(pbmetad_deposit_f64_kernel, grid, block, 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int molann_selftest_pbmetad_deposit_f64(double* table, int32_t n_axes, const int64_t* shape, const double* lower, const double* spacing,
                                        const int32_t* periodic, const double* sigma, const int32_t* columns, const double* y, int64_t y_stride,
                                        const double* V, int64_t v_stride, int64_t n_walkers, double height0, double inv_dT, double kT,
                                        double cutoff, double* state, double* log, int64_t log_capacity) {
    PbmetadDepositArgs a = {};
    const int e = pbmetad_deposit_arguments(table, n_axes, shape, lower, spacing, periodic, sigma, columns, y, y_stride, V, v_stride, n_walkers,
                                            height0, inv_dT, kT, cutoff, state, log, log_capacity, a);
    if (e != MOLANN_OK || n_walkers == 0) return e;
    pbmetad_deposit_host(a);
    return MOLANN_OK;
}

} // extern "C"
