// molann_opes_deposit_f64.inc - part of libmolann_hip.so, included by molann_kernels.hip after molann_value_f64.inc.  The host side of
// molann_dev_opes_deposit_f64.inc (see include/molann_hip.h): molann_opes_deposit_f64 and molann_opes_kernel_sum_f64 check their
// arguments and enqueue one launch each - no plan, no workspace, no event - and molann_selftest_opes_deposit_f64 runs the deposit on host
// arrays through the same steps and the same per-kernel functions, with the device's order of every sum.  molann_opes_step_f64 (a whole
// OPES step: opes_step_f64_kernel of molann_dev_opes_table_f64.inc) and its twin molann_selftest_opes_step_f64 follow the same pattern, and so
// do molann_opes_step_columns_f64 (the step on strided outputs and chosen columns: opes_step_columns_f64_kernel of
// molann_dev_bias_opes_table_f64.inc) and molann_selftest_opes_step_columns_f64, and molann_opes_step_modes_f64 (that step with adaptive
// widths and the explore variant: opes_step_modes_f64_kernel of molann_dev_opes_adaptive_f64.inc) and molann_selftest_opes_step_modes_f64.
namespace {

// the device's block on the host: the same strided partials, the same butterfly, the same order of the four waves
struct OpesDepositHost {
    double* centers;
    double* sigma;
    double* heights;
    const double* period;
    const double* new_centers;
    const double* new_sigma;
    const double* new_heights;
    int d;

    void read_row(const double* c, const double* s, const double* h, long row, double (&co)[HILLS_MAX_D], double (&so)[HILLS_MAX_D], double& ho) const {
        for (int k = 0; k < HILLS_MAX_D; ++k) {
            co[k] = k < d ? c[row * d + k] : 0.0;
            so[k] = k < d ? s[row * d + k] : 1.0;
        }
        ho = h[row];
    }
    void load_new(long a, double (&c)[HILLS_MAX_D], double (&s)[HILLS_MAX_D], double& h) const { read_row(new_centers, new_sigma, new_heights, a, c, s, h); }
    void load(long slot, double (&c)[HILLS_MAX_D], double (&s)[HILLS_MAX_D], double& h) const { read_row(centers, sigma, heights, slot, c, s, h); }
    void store(long slot, const double (&c)[HILLS_MAX_D], const double (&s)[HILLS_MAX_D], double h) const {
        for (int k = 0; k < d; ++k) { centers[slot * d + k] = c[k]; sigma[slot * d + k] = s[k]; }
        heights[slot] = h;
    }
    void move(long from, long to) const {
        for (int k = 0; k < d; ++k) { centers[to * d + k] = centers[from * d + k]; sigma[to * d + k] = sigma[from * d + k]; }
        heights[to] = heights[from];
    }
    // the smallest q, then the smallest slot: ascending slots and a strict comparison give the pair the device's reduction gives
    bool nearest(const double (&c)[HILLS_MAX_D], long n, long skip, double& q_out, long& slot_out) const {
        double q = HUGE_VAL;
        long slot = -1;
        bool any = false;
        for (long k = 0; k < n; ++k) {
            if (k == skip) continue;
            const double qk = opes_merge_distance_f64(c, centers + k * d, sigma + k * d, period, d);
            if (qk < q) { q = qk; slot = k; any = true; }
        }
        q_out = q; slot_out = slot;
        return any;
    }
    double pair_sum(const double (&ce)[HILLS_MAX_D], const double (&se)[HILLS_MAX_D], double he, long n, long skip_a, long skip_b, double c2,
                    double c0) const {
        double inv[HILLS_MAX_D];
        hill_inverse_widths_f64(se, d, inv);
        double part[256];
        for (int t = 0; t < 256; ++t) {
            part[t] = 0.0;
            for (long i = t; i < n; i += 256) {
                if (i == skip_a || i == skip_b) continue;
                part[t] = part[t] + opes_pair_term_f64(ce, se, inv, he, centers + i * d, sigma + i * d, heights[i], period, c2, c0, d);
            }
        }
        return block_sum(part);
    }
    // the block's sum of 256 partials: group_sum<64>'s butterfly in each wave, then ((w0 + w1) + w2) + w3
    static double block_sum(double (&part)[256]) {
        double next[64];
        for (int w = 0; w < 4; ++w)
            for (int m = 32; m >= 1; m >>= 1) {
                for (int l = 0; l < 64; ++l) next[l] = part[64 * w + l] + part[64 * w + (l ^ m)];
                for (int l = 0; l < 64; ++l) part[64 * w + l] = next[l];
            }
        return ((part[0] + part[64]) + part[128]) + part[192];
    }
};

// opes_step_f64_kernel's executor on the host (OpesStepDev): the deposit's, the walkers' sums in the block's order, and the new kernels
// formed from y, V and the step's widths
struct OpesStepHost : OpesDepositHost {
    const double* V;
    double beta;
    double ratio;
    double step_sigma[HILLS_MAX_D];

    void walker_sums(long n_walkers, double& count, double& sum_w, double& sum_w2) const {
        double pc[256], pw[256], pw2[256];
        for (int t = 0; t < 256; ++t) {
            pc[t] = pw[t] = pw2[t] = 0.0;
            for (long a = t; a < n_walkers; a += 256) {
                double w;
                if (opes_walker_weight_f64(beta, V[a], new_centers + a * d, d, w)) opes_walker_add_f64(w, pc[t], pw[t], pw2[t]);
            }
        }
        count = block_sum(pc);
        sum_w = block_sum(pw);
        sum_w2 = block_sum(pw2);
    }
    void load_new(long a, double (&c)[HILLS_MAX_D], double (&s)[HILLS_MAX_D], double& h) const {
        for (int k = 0; k < HILLS_MAX_D; ++k) {
            c[k] = k < d ? new_centers[a * d + k] : 0.0;
            s[k] = k < d ? step_sigma[k] : 1.0;
        }
        h = opes_walker_height_f64(beta, V[a], new_centers + a * d, d, ratio);
    }
};

// opes_step_columns_f64_kernel's executor on the host (OpesStepColumnsDev): OpesStepHost with walker a's centre gathered from
// y[a * y_stride + col[k]] and its bias read at V[a * v_stride]
struct OpesStepColumnsHost : OpesStepHost {       // its fields; new_centers is y
    long y_stride, v_stride;
    int col[HILLS_MAX_D];

    void gather(long a, double (&yc)[HILLS_MAX_D]) const {
        const double* row = new_centers + a * y_stride;
        for (int k = 0; k < HILLS_MAX_D; ++k) yc[k] = k < d ? row[col[k]] : 0.0;
    }
    void walker_sums(long n_walkers, double& count, double& sum_w, double& sum_w2) const {
        double pc[256], pw[256], pw2[256];
        for (int t = 0; t < 256; ++t) {
            pc[t] = pw[t] = pw2[t] = 0.0;
            for (long a = t; a < n_walkers; a += 256) {
                double w, yc[HILLS_MAX_D];
                gather(a, yc);
                if (opes_walker_weight_f64(beta, V[a * v_stride], yc, d, w)) opes_walker_add_f64(w, pc[t], pw[t], pw2[t]);
            }
        }
        count = block_sum(pc);
        sum_w = block_sum(pw);
        sum_w2 = block_sum(pw2);
    }
    void load_new(long a, double (&c)[HILLS_MAX_D], double (&s)[HILLS_MAX_D], double& h) const {
        gather(a, c);
        for (int k = 0; k < HILLS_MAX_D; ++k) s[k] = k < d ? step_sigma[k] : 1.0;
        h = opes_walker_height_f64(beta, V[a * v_stride], c, d, ratio);
    }
};

// opes_step_modes_f64_kernel's executor on the host (OpesStepModesDev): the pairs in ascending order - each is independent of every
// other, so the order does not matter - and no barrier
struct OpesStepModesHost : OpesStepColumnsHost {
    double* adapt;
    const double* sigma_min;
    double width_count, width_factor, width_scale;
    int fixed_sigma, explore;

    void observe(long n_walkers, double tau) const {
        for (long a = 0; a < n_walkers; ++a) {
            double yc[HILLS_MAX_D];
            gather(a, yc);
            if (!opes_outputs_finite_f64(yc, d)) continue;
            double* row = adapt + a * 3 * d;
            for (int k = 0; k < d; ++k) opes_adapt_observe_f64(yc[k], period ? period[k] : 0.0, tau, row[k], row[d + k]);
        }
    }
    void first_deposit(long n_walkers, double count, double factor, double biasfactor, const double* smin) const {
        for (long a = 0; a < n_walkers; ++a) {
            double* row = adapt + a * 3 * d;
            for (int k = 0; k < d; ++k) opes_adapt_first_f64(count, factor, biasfactor, smin ? smin[k] : 0.0, row[d + k], row[2 * d + k]);
        }
    }
    void load_new(long a, double (&c)[HILLS_MAX_D], double (&s)[HILLS_MAX_D], double& h) const {
        gather(a, c);
        double ratio_a = ratio;
        if (adapt) {
            const double* row = adapt + a * 3 * d;
            ratio_a = opes_adaptive_widths_f64(row + d, row + 2 * d, sigma_min, width_count, width_factor, width_scale, fixed_sigma, d, s);
        } else {
            for (int k = 0; k < HILLS_MAX_D; ++k) s[k] = k < d ? step_sigma[k] : 1.0;
        }
        h = opes_walker_height_modes_f64(beta, V[a * v_stride], c, d, ratio_a, explore);
    }
};

// what molann_opes_step_columns_f64 and its host twin add to opes_step_arguments, after it: the strides (MOLANN_E_DESC), then the list -
// d distinct indices in [0, y_stride), NULL for 0..d-1 (MOLANN_E_INDEX); then the list is in `cols`
inline int opes_step_columns_arguments(int32_t d, int64_t y_stride, const int32_t* columns, int64_t v_stride, int (&cols)[HILLS_MAX_D]) {
    if (y_stride < d || v_stride < 1) return MOLANN_E_DESC;
    for (int k = 0; k < HILLS_MAX_D; ++k) cols[k] = 0;
    for (int32_t j = 0; j < d; ++j) {
        const int32_t cj = columns ? columns[j] : j;
        if (cj < 0 || cj >= y_stride) return MOLANN_E_INDEX;
        for (int32_t i = 0; i < j; ++i)
            if (cols[i] == cj) return MOLANN_E_INDEX;
        cols[j] = cj;
    }
    return MOLANN_OK;
}

// the arguments molann_opes_step_f64 and its host twin share, in molann_opes_deposit_f64's order of refusals
inline int opes_step_arguments(const double* centers, const double* sigma, const double* heights, int64_t capacity, int32_t d, const double* period,
                               const double* state, const double* run, const double* y, const double* V, int64_t n_walkers, const double* sigma0,
                               const double* sigma_min, double beta, double threshold, double cutoff) {
    if (n_walkers > 0 && (!centers || !sigma || !heights || !state || !run || !y || !V || !sigma0)) return MOLANN_E_NULL;
    if (((uintptr_t)centers | (uintptr_t)sigma | (uintptr_t)heights | (uintptr_t)period | (uintptr_t)state | (uintptr_t)run | (uintptr_t)y |
         (uintptr_t)V | (uintptr_t)sigma0 | (uintptr_t)sigma_min) & 7)
        return MOLANN_E_ALIGNMENT;
    if (d < 1 || d > HILLS_MAX_D) return MOLANN_E_DESC;
    if (capacity < 1) return MOLANN_E_DESC;
    if (n_walkers < 0) return MOLANN_E_DESC;
    if (!std::isfinite(beta) || !(beta > 0.0)) return MOLANN_E_DESC;
    if (!std::isfinite(threshold) || threshold < 0.0) return MOLANN_E_DESC;
    if (!(cutoff > 0.0)) return MOLANN_E_DESC;
    return MOLANN_OK;
}

// the arguments molann_opes_deposit_f64 and its host twin share, in the order of the refusals
inline int opes_deposit_arguments(const double* centers, const double* sigma, const double* heights, int64_t capacity, int32_t d,
                                  const double* period, const double* state, const double* new_centers, const double* new_sigma,
                                  const double* new_heights, int64_t n_new, double threshold, double cutoff) {
    if (n_new > 0 && (!centers || !sigma || !heights || !state || !new_centers || !new_sigma || !new_heights)) return MOLANN_E_NULL;
    if (((uintptr_t)centers | (uintptr_t)sigma | (uintptr_t)heights | (uintptr_t)period | (uintptr_t)state | (uintptr_t)new_centers |
         (uintptr_t)new_sigma | (uintptr_t)new_heights) & 7)
        return MOLANN_E_ALIGNMENT;
    if (d < 1 || d > HILLS_MAX_D) return MOLANN_E_DESC;
    if (capacity < 1) return MOLANN_E_DESC;
    if (n_new < 0) return MOLANN_E_DESC;
    if (!std::isfinite(threshold) || threshold < 0.0) return MOLANN_E_DESC;
    if (!(cutoff > 0.0)) return MOLANN_E_DESC;
    return MOLANN_OK;
}

// what molann_opes_step_modes_f64 and its host twin refuse: opes_step_arguments (sigma0 may be NULL where adapt is given: adapt stands in
// for it), opes_step_columns_arguments, then adapt's alignment, observe-only without adapt, a stride < 2 with adapt, and in either mode a
// biasfactor that is not finite and > 1
inline int opes_step_modes_arguments(const double* centers, const double* sigma, const double* heights, int64_t capacity, int32_t d,
                                     const double* period, const double* state, const double* run, const double* y, int64_t y_stride,
                                     const int32_t* columns, const double* V, int64_t v_stride, int64_t n_walkers, const double* sigma0,
                                     const double* sigma_min, const double* adapt, double beta, double biasfactor, int64_t adaptive_stride,
                                     double threshold, double cutoff, int32_t flags, int (&cols)[HILLS_MAX_D]) {
    int e = opes_step_arguments(centers, sigma, heights, capacity, d, period, state, run, y, V, n_walkers, (adapt && !sigma0) ? adapt : sigma0,
                                sigma_min, beta, threshold, cutoff);
    if (e == MOLANN_OK) e = opes_step_columns_arguments(d, y_stride, columns, v_stride, cols);
    if (e != MOLANN_OK) return e;
    if ((uintptr_t)adapt & 7) return MOLANN_E_ALIGNMENT;
    if (!adapt && (flags & OPES_FLAG_OBSERVE)) return MOLANN_E_DESC;
    if (adapt && adaptive_stride < 2) return MOLANN_E_DESC;
    if ((adapt || (flags & OPES_FLAG_EXPLORE)) && !(std::isfinite(biasfactor) && biasfactor > 1.0)) return MOLANN_E_DESC;
    return MOLANN_OK;
}

} // namespace

extern "C" {

int molann_opes_deposit_f64(double* centers, double* sigma, double* heights, int64_t capacity, int32_t d, const double* period, double* state,
                            const double* new_centers, const double* new_sigma, const double* new_heights, int64_t n_new, double threshold,
                            double cutoff, molann_stream_t stream) {
    const int e = opes_deposit_arguments(centers, sigma, heights, capacity, d, period, state, new_centers, new_sigma, new_heights, n_new, threshold,
                                         cutoff);
    if (e != MOLANN_OK || n_new == 0) return e;
    hipLaunchKernelGGL(opes_deposit_f64_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, centers, sigma, heights, (long)capacity, (int)d, period,
                       state, new_centers, new_sigma, new_heights, (long)n_new, threshold, cutoff);
    return (int)hipGetLastError();
}

int molann_selftest_opes_deposit_f64(double* centers, double* sigma, double* heights, int64_t capacity, int32_t d, const double* period,
                                     double* state, const double* new_centers, const double* new_sigma, const double* new_heights, int64_t n_new,
                                     double threshold, double cutoff) {
    const int e = opes_deposit_arguments(centers, sigma, heights, capacity, d, period, state, new_centers, new_sigma, new_heights, n_new, threshold,
                                         cutoff);
    if (e != MOLANN_OK || n_new == 0) return e;
    OpesDepositHost ex = {centers, sigma, heights, period, new_centers, new_sigma, new_heights, (int)d};
    long n = opes_live_count_f64(state[0], (long)capacity);
    double S = state[1], merges = state[2], refused = state[3];
    opes_deposit_steps_f64(ex, (long)capacity, (int)d, period, (long)n_new, threshold, cutoff, n, S, merges, refused);
    state[0] = (double)n; state[1] = S; state[2] = merges; state[3] = refused;
    return MOLANN_OK;
}

int molann_opes_step_f64(double* centers, double* sigma, double* heights, int64_t capacity, int32_t d, const double* period, double* state, double* run,
                         const double* y, const double* V, int64_t n_walkers, const double* sigma0, const double* sigma_min, double beta,
                         double threshold, double cutoff, int32_t fixed_sigma, molann_stream_t stream) {
    const int e = opes_step_arguments(centers, sigma, heights, capacity, d, period, state, run, y, V, n_walkers, sigma0, sigma_min, beta, threshold,
                                      cutoff);
    if (e != MOLANN_OK || n_walkers == 0) return e;
    hipLaunchKernelGGL(opes_step_f64_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, centers, sigma, heights, (long)capacity, (int)d, period, state,
                       run, y, V, (long)n_walkers, sigma0, sigma_min, beta, threshold, cutoff, fixed_sigma != 0 ? 1 : 0);
    return (int)hipGetLastError();
}

int molann_selftest_opes_step_f64(double* centers, double* sigma, double* heights, int64_t capacity, int32_t d, const double* period, double* state,
                                  double* run, const double* y, const double* V, int64_t n_walkers, const double* sigma0, const double* sigma_min,
                                  double beta, double threshold, double cutoff, int32_t fixed_sigma) {
    const int e = opes_step_arguments(centers, sigma, heights, capacity, d, period, state, run, y, V, n_walkers, sigma0, sigma_min, beta, threshold,
                                      cutoff);
    if (e != MOLANN_OK || n_walkers == 0) return e;
    OpesStepHost ex = {{centers, sigma, heights, period, y, nullptr, nullptr, (int)d}, V, beta, 1.0, {1., 1., 1., 1., 1., 1., 1., 1.}};
    long n = opes_live_count_f64(state[0], (long)capacity);
    double S = state[1], merges = state[2], refused = state[3];
    double r[8] = {run[0], run[1], run[2], 0., 0., 0., 0., 0.};
    opes_step_steps_f64(ex, (long)capacity, (int)d, period, (long)n_walkers, threshold, cutoff, beta, fixed_sigma != 0 ? 1 : 0, sigma0, sigma_min, n, S,
                        merges, refused, r);
    state[0] = (double)n; state[1] = S; state[2] = merges; state[3] = refused;
    for (int i = 0; i < 8; ++i) run[i] = r[i];
    return MOLANN_OK;
}

int molann_opes_step_columns_f64(double* centers, double* sigma, double* heights, int64_t capacity, int32_t d, const double* period, double* state,
                                 double* run, const double* y, int64_t y_stride, const int32_t* columns, const double* V, int64_t v_stride,
                                 int64_t n_walkers, const double* sigma0, const double* sigma_min, double beta, double threshold, double cutoff,
                                 int32_t fixed_sigma, molann_stream_t stream) {
    int e = opes_step_arguments(centers, sigma, heights, capacity, d, period, state, run, y, V, n_walkers, sigma0, sigma_min, beta, threshold, cutoff);
    OpesStepColumns cols;
    if (e == MOLANN_OK) e = opes_step_columns_arguments(d, y_stride, columns, v_stride, cols.col);
    if (e != MOLANN_OK || n_walkers == 0) return e;
    hipLaunchKernelGGL(opes_step_columns_f64_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, centers, sigma, heights, (long)capacity, (int)d, period,
                       state, run, y, (long)y_stride, cols, V, (long)v_stride, (long)n_walkers, sigma0, sigma_min, beta, threshold, cutoff,
                       fixed_sigma != 0 ? 1 : 0);
    return (int)hipGetLastError();
}

int molann_selftest_opes_step_columns_f64(double* centers, double* sigma, double* heights, int64_t capacity, int32_t d, const double* period,
                                          double* state, double* run, const double* y, int64_t y_stride, const int32_t* columns, const double* V,
                                          int64_t v_stride, int64_t n_walkers, const double* sigma0, const double* sigma_min, double beta,
                                          double threshold, double cutoff, int32_t fixed_sigma) {
    int e = opes_step_arguments(centers, sigma, heights, capacity, d, period, state, run, y, V, n_walkers, sigma0, sigma_min, beta, threshold, cutoff);
    OpesStepColumnsHost ex = {{{centers, sigma, heights, period, y, nullptr, nullptr, (int)d}, V, beta, 1.0, {1., 1., 1., 1., 1., 1., 1., 1.}},
                              (long)y_stride, (long)v_stride, {0, 0, 0, 0, 0, 0, 0, 0}};
    if (e == MOLANN_OK) e = opes_step_columns_arguments(d, y_stride, columns, v_stride, ex.col);
    if (e != MOLANN_OK || n_walkers == 0) return e;
    long n = opes_live_count_f64(state[0], (long)capacity);
    double S = state[1], merges = state[2], refused = state[3];
    double r[8] = {run[0], run[1], run[2], 0., 0., 0., 0., 0.};
    opes_step_steps_f64(ex, (long)capacity, (int)d, period, (long)n_walkers, threshold, cutoff, beta, fixed_sigma != 0 ? 1 : 0, sigma0, sigma_min, n, S,
                        merges, refused, r);
    state[0] = (double)n; state[1] = S; state[2] = merges; state[3] = refused;
    for (int i = 0; i < 8; ++i) run[i] = r[i];
    return MOLANN_OK;
}

int molann_opes_step_modes_f64(double* centers, double* sigma, double* heights, int64_t capacity, int32_t d, const double* period, double* state,
                               double* run, const double* y, int64_t y_stride, const int32_t* columns, const double* V, int64_t v_stride,
                               int64_t n_walkers, const double* sigma0, const double* sigma_min, double* adapt, double beta, double biasfactor,
                               int64_t adaptive_stride, double threshold, double cutoff, int32_t flags, molann_stream_t stream) {
    OpesStepColumns cols;
    const int e = opes_step_modes_arguments(centers, sigma, heights, capacity, d, period, state, run, y, y_stride, columns, V, v_stride, n_walkers,
                                            sigma0, sigma_min, adapt, beta, biasfactor, adaptive_stride, threshold, cutoff, flags, cols.col);
    if (e != MOLANN_OK || n_walkers == 0) return e;
    hipLaunchKernelGGL(opes_step_modes_f64_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, centers, sigma, heights, (long)capacity, (int)d, period,
                       state, run, y, (long)y_stride, cols, V, (long)v_stride, (long)n_walkers, sigma0, sigma_min, adapt, beta, biasfactor,
                       (double)adaptive_stride, threshold, cutoff, (int)(flags & 7));
    return (int)hipGetLastError();
}

int molann_selftest_opes_step_modes_f64(double* centers, double* sigma, double* heights, int64_t capacity, int32_t d, const double* period,
                                        double* state, double* run, const double* y, int64_t y_stride, const int32_t* columns, const double* V,
                                        int64_t v_stride, int64_t n_walkers, const double* sigma0, const double* sigma_min, double* adapt,
                                        double beta, double biasfactor, int64_t adaptive_stride, double threshold, double cutoff, int32_t flags) {
    OpesStepModesHost ex = {{{{centers, sigma, heights, period, y, nullptr, nullptr, (int)d}, V, beta, 1.0, {1., 1., 1., 1., 1., 1., 1., 1.}},
                             (long)y_stride, (long)v_stride, {0, 0, 0, 0, 0, 0, 0, 0}},
                            adapt, sigma_min, 1.0, 1.0, 1.0, 0, 0};
    const int e = opes_step_modes_arguments(centers, sigma, heights, capacity, d, period, state, run, y, y_stride, columns, V, v_stride, n_walkers,
                                            sigma0, sigma_min, adapt, beta, biasfactor, adaptive_stride, threshold, cutoff, flags, ex.col);
    if (e != MOLANN_OK || n_walkers == 0) return e;
    long n = opes_live_count_f64(state[0], (long)capacity);
    double S = state[1], merges = state[2], refused = state[3];
    double r[8] = {run[0], run[1], run[2], run[3], run[4], run[5], run[6], run[7]};
    const bool deposited = opes_step_modes_steps_f64(ex, (long)capacity, (int)d, period, (long)n_walkers, threshold, cutoff, beta, (int)(flags & 7),
                                                     adapt != nullptr, sigma0, sigma_min, biasfactor, (double)adaptive_stride, n, S, merges, refused, r);
    if (deposited) {
        state[0] = (double)n; state[1] = S; state[2] = merges; state[3] = refused;
        for (int i = 0; i < 8; ++i) run[i] = r[i];
    } else {
        run[6] = r[6];
    }
    return MOLANN_OK;
}

int molann_opes_kernel_sum_f64(const double* points, int64_t n_points, int32_t d, const double* centers, const double* heights, int64_t n_kernels,
                               const double* sigma, int64_t sigma_stride, const double* period, double cutoff, double* P, double* dP,
                               molann_stream_t stream) {
    if (n_points < 0 || n_kernels < 0) return MOLANN_E_DESC;
    if (n_points == 0) return MOLANN_OK;
    if (!points || !P || (n_kernels > 0 && (!centers || !heights || !sigma))) return MOLANN_E_NULL;
    if (((uintptr_t)points | (uintptr_t)P | (uintptr_t)dP | (uintptr_t)centers | (uintptr_t)heights | (uintptr_t)sigma | (uintptr_t)period) & 7)
        return MOLANN_E_ALIGNMENT;
    if (d < 1 || d > HILLS_MAX_D) return MOLANN_E_UNSUPPORTED;
    if (sigma_stride != 0 && sigma_stride != d) return MOLANN_E_DESC;
    if (!(cutoff > 0.0)) return MOLANN_E_DESC;
    const int64_t blocks = (n_points + 3) / 4;
    const int grid = (int)std::min<int64_t>(blocks, 2048);    // 8 blocks of 4 waves per compute unit; the loop strides over the rest
    hipLaunchKernelGGL(opes_kernel_sum_f64_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, points, centers, heights, sigma, period, P, dP,
                       (long)n_points, (long)n_kernels, (long)sigma_stride, cutoff, (int)d);
    return (int)hipGetLastError();
}

} // extern "C"
