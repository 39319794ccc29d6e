// molann_metad_rct_f64.inc - part of libmolann_hip.so, included by molann_kernels.hip after molann_metad_deposit_f64.inc.  The host side of
// molann_dev_metad_rct_f64.inc (see include/molann_hip.h): molann_metad_rct_f64 checks its arguments and enqueues the two launches - no
// plan, no workspace of its own, no event - and molann_selftest_metad_rct_f64 runs the same chunks, the same tree and the same functions
// (molann_metad_rct.h) on host arrays.
namespace {

// the arguments molann_metad_rct_f64 and its host twin share, in the order of the refusals; then the kernels' arguments are in `a`
inline int metad_rct_arguments(const double* table, int64_t n_entries, double kT, double inv_dT, const double* state, int64_t stride, double* partials,
                               int64_t partial_rows, double* rct, MetadRctArgs& a) {
    if (!table || !partials || !rct) return MOLANN_E_NULL;
    if (((uintptr_t)table | (uintptr_t)state | (uintptr_t)partials | (uintptr_t)rct) & 7) return MOLANN_E_ALIGNMENT;
    if (n_entries < 1 || n_entries >= ((int64_t)1 << 31)) return MOLANN_E_DESC;
    if (!std::isfinite(kT) || !(kT > 0.0)) return MOLANN_E_DESC;
    if (!std::isfinite(inv_dT) || !(inv_dT >= 0.0)) return MOLANN_E_DESC;
    if (stride < 1) return MOLANN_E_DESC;
    if (partial_rows < metad_rct_chunks((long)n_entries)) return MOLANN_E_DESC;
    a.table = table; a.state = state; a.partials = partials; a.rct = rct;
    a.n = (long)n_entries; a.chunks = metad_rct_chunks((long)n_entries); a.stride = (long)stride;
    a.kT = kT; a.aV = inv_dT; a.a0 = 1.0 / kT + inv_dT;
    return MOLANN_OK;
}

// the two kernels on the host: chunk by chunk with 256 thread values in an array, then the combine step's 256 threads
inline void metad_rct_host(const MetadRctArgs& a) {
    double steps;
    if (!metad_rct_due_f64(a.state, a.stride, steps)) return;
    double xm[METAD_RCT_THREADS], x0[METAD_RCT_THREADS], xV[METAD_RCT_THREADS], xb[METAD_RCT_THREADS];
    std::vector<double> slots((size_t)METAD_RCT_THREADS * METAD_RCT_SLOTS);
    std::vector<char> inside((size_t)METAD_RCT_THREADS * METAD_RCT_SLOTS);
    for (long c = 0; c < a.chunks; ++c) {
        for (int t = 0; t < METAD_RCT_THREADS; ++t) {
            double v[METAD_RCT_SLOTS];
            bool live[METAD_RCT_SLOTS];
            for (int j = 0; j < METAD_RCT_SLOTS; ++j) {
                const long g = c * METAD_RCT_CHUNK + t + (long)j * METAD_RCT_THREADS;
                live[j] = g < a.n;
                v[j] = live[j] ? a.table[g] : 0.0;
                slots[(size_t)t * METAD_RCT_SLOTS + j] = v[j];
                inside[(size_t)t * METAD_RCT_SLOTS + j] = live[j];
            }
            int bad;
            xm[t] = metad_rct_thread_max_f64(v, live, bad);
            xb[t] = (double)bad;
        }
        const double m = metad_rct_tree_f64(xm, MetadRctMax());
        for (int t = 0; t < METAD_RCT_THREADS; ++t) {
            double v[METAD_RCT_SLOTS];
            bool live[METAD_RCT_SLOTS];
            for (int j = 0; j < METAD_RCT_SLOTS; ++j) {
                v[j] = slots[(size_t)t * METAD_RCT_SLOTS + j];
                live[j] = inside[(size_t)t * METAD_RCT_SLOTS + j] != 0;
            }
            metad_rct_thread_sums_f64(v, live, m, a.a0, a.aV, x0[t], xV[t]);
        }
        double* p = a.partials + c * METAD_RCT_ROW;
        p[0] = m;
        p[1] = metad_rct_tree_f64(x0, MetadRctAdd());
        p[2] = metad_rct_tree_f64(xV, MetadRctAdd());
        p[3] = metad_rct_tree_f64(xb, MetadRctAdd());
    }
    for (int t = 0; t < METAD_RCT_THREADS; ++t) xm[t] = metad_rct_combine_max_f64(a.partials, a.chunks, t);
    const double M = metad_rct_tree_f64(xm, MetadRctMax());
    for (int t = 0; t < METAD_RCT_THREADS; ++t) metad_rct_combine_sums_f64(a.partials, a.chunks, t, M, a.a0, a.aV, x0[t], xV[t], xb[t]);
    const double S0 = metad_rct_tree_f64(x0, MetadRctAdd()), SV = metad_rct_tree_f64(xV, MetadRctAdd()), bad = metad_rct_tree_f64(xb, MetadRctAdd());
    metad_rct_final_f64(M, S0, SV, bad, a.kT, a.a0, a.aV, steps, a.rct);
}

} // namespace

extern "C" {

int64_t molann_metad_rct_chunks(int64_t n_entries) { return n_entries < 1 ? 0 : (int64_t)metad_rct_chunks((long)n_entries); }

int molann_metad_rct_f64(const double* table, int64_t n_entries, double kT, double inv_dT, const double* state, int64_t stride, double* partials,
                         int64_t partial_rows, double* rct, molann_stream_t stream) {
    MetadRctArgs a = {};
    const int e = metad_rct_arguments(table, n_entries, kT, inv_dT, state, stride, partials, partial_rows, rct, a);
    if (e != MOLANN_OK) return e;
    const dim3 grid((unsigned)std::min<long>(a.chunks, METAD_RCT_MAX_BLOCKS)), block(METAD_RCT_THREADS);
    hipLaunchKernelGGL(metad_rct_partial_f64_kernel, grid, block, 0, (hipStream_t)stream, a);
    hipLaunchKernelGGL(metad_rct_combine_f64_kernel, dim3(1), block, 0, (hipStream_t)stream, a);
    return (int)hipGetLastError();
}

int molann_selftest_metad_rct_f64(const double* table, int64_t n_entries, double kT, double inv_dT, const double* state, int64_t stride,
                                  double* partials, int64_t partial_rows, double* rct) {
    MetadRctArgs a = {};
    const int e = metad_rct_arguments(table, n_entries, kT, inv_dT, state, stride, partials, partial_rows, rct, a);
    if (e != MOLANN_OK) return e;
    metad_rct_host(a);
    return MOLANN_OK;
}

} // extern "C"
