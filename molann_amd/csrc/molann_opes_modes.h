// molann_opes_modes.h - the arithmetic of an OPES step with adaptive widths and in the explore variant, one copy for the device
// (opes_step_modes_f64_kernel, molann_dev_opes_adaptive_f64.inc) and for the host twin (molann_opes_deposit_f64.inc).  It continues
// molann_math.h's OPES section and is built from its pieces (opes_walker_weight_f64, opes_run_scalars_f64, opes_step_widths_f64,
// opes_deposit_steps_f64), but lives in a header of its own: molann_math.h travels inside the library as the source of the kernels
// compiled at run time, none of which uses any of this, and stays byte for byte what those kernels were built from before.
// Included by molann_kernels.hip after molann_math.h.
#pragma once
#include "molann_math.h"

namespace molann {

// The step with OPES_METAD's two other modes (opes_step_modes_f64_kernel and its host twin): widths measured from the run
// (SIGMA=ADAPTIVE) and the explore variant (OPES_METAD_EXPLORE).  adapt[W, 3, d] holds (mean, M2, sigma0) per walker between the steps,
// run[6] the number of observations and run[7] whether the first deposit has fixed sigma0.  Nothing is contracted, and phase 1 is only
// + - * / rint: the host and the device get the same bits there.
//
// wrap_k of opes_merge_distance_f64: d - P rint(d / P) where P > 0
MOLANN_HD double opes_wrap_f64(double dk, double P) {
#pragma clang fp contract(off)
    if (P > 0.0) {
        const double turns = rint(dk / P);
        const double whole = P * turns;
        dk = dk - whole;
    }
    return dk;
}

// opes_walker_weight_f64's rule on the outputs alone: every y_k finite
MOLANN_HD bool opes_outputs_finite_f64(const double* y, int d) {
    bool ok = true;
#pragma unroll
    for (int k = 0; k < HILLS_MAX_D; ++k)
        if (k < d) ok = ok && fabs(y[k]) <= 1.7976931348623157e308;
    return ok;
}

// one observation of one (walker, column) pair: the running mean with weight 1 / tau (tau = min(observations, adaptive_stride): an
// exponential window once the first stride has passed) and Welford's sum with it, differences taken the shorter way round a periodic
// output.  The mean is not wrapped back: every reader wraps differences.
MOLANN_HD void opes_adapt_observe_f64(double y, double P, double tau, double& mean, double& M2) {
#pragma clang fp contract(off)
    const double diff = opes_wrap_f64(y - mean, P);
    mean = mean + diff / tau;
    const double after = opes_wrap_f64(y - mean, P);
    M2 = M2 + diff * after;
}

// the first deposit of an adaptive run, one pair: the samples so far were unbiased and the later ones come from the distribution
// flattened by `biasfactor`, so M2 is carried over as M2 biasfactor; sigma0 = sqrt((M2 / count) / factor), raised to sigma_min
// (0: none) - factor = biasfactor gives the unbiased width back, factor = 1 (explore) the width of the flattened target.
MOLANN_HD void opes_adapt_first_f64(double count, double factor, double biasfactor, double sigma_min, double& M2, double& sigma0) {
#pragma clang fp contract(off)
    M2 = M2 * biasfactor;
    double s = sqrt((M2 / count) / factor);
    if (s < sigma_min) s = sigma_min;
    sigma0 = s;
}

// the widths of one walker's kernel in an adaptive run: s_k = sqrt((M2_k / count) / factor), times sigma_scale unless fixed_sigma,
// raised to sigma_min_k once, at the end (s_k < sigma_min_k: a NaN stays).  Returns prod_k (sigma0_k / s_k), k ascending, as
// opes_step_widths_f64 does.  A width of 0 (a walker that never moved, no sigma_min) gives a ratio that is not finite and a kernel that
// opes_kernel_valid_f64 refuses.
MOLANN_HD double opes_adaptive_widths_f64(const double* M2, const double* sigma0, const double* sigma_min, double count, double factor,
                                          double sigma_scale, int fixed_sigma, int d, double (&sigma)[HILLS_MAX_D]) {
#pragma clang fp contract(off)
    double ratio = 1.0;
#pragma unroll
    for (int k = 0; k < HILLS_MAX_D; ++k) {
        sigma[k] = 1.0;
        if (k < d) {
            double s = sqrt((M2[k] / count) / factor);
            if (!fixed_sigma) s = s * sigma_scale;
            if (sigma_min && s < sigma_min[k]) s = sigma_min[k];
            sigma[k] = s;
            ratio = ratio * (sigma0[k] / s);
        }
    }
    return ratio;
}

// the bandwidth rescaling of opes_run_scalars_f64 on another sample size: the explore variant takes the counter, not neff
MOLANN_HD double opes_silverman_scale_f64(double size, int d, int fixed_sigma) {
#pragma clang fp contract(off)
    const double dd = (double)d;
    return fixed_sigma ? 1.0 : pow((size * (dd + 2.0)) / 4.0, -1.0 / (dd + 4.0));
}

// opes_walker_height_f64 in both modes: w_a ratio, or ratio alone in the explore variant, where every kernel weighs 1 (the table's
// S / n does not change with that scale); NaN for a walker that does not count
MOLANN_HD double opes_walker_height_modes_f64(double beta, double V, const double* y, int d, double ratio, int explore) {
#pragma clang fp contract(off)
    double w;
    const bool ok = opes_walker_weight_f64(beta, V, y, d, w);
    return ok ? (explore ? ratio : w * ratio) : __builtin_nan("");
}

#define OPES_FLAG_FIXED_SIGMA 1
#define OPES_FLAG_EXPLORE 2
#define OPES_FLAG_OBSERVE 4

// The step in its modes, one copy for the device and the host.  `ex` is opes_step_steps_f64's executor with three additions:
// observe(W, tau) runs opes_adapt_observe_f64 on every pair of a walker whose d outputs are finite, first_deposit(W, count, factor,
// biasfactor, sigma_min) runs opes_adapt_first_f64 on every pair - both end with the block's barrier on the device - and load_new(a)
// forms walker a's widths from its row of adapt (opes_adaptive_widths_f64 with ex.width_*) and its height by
// opes_walker_height_modes_f64.  In order: 1. the averages (adaptive); 2. return for `observe`, and for a deposit before the first
// stride has passed - n, S, merges, refused and run[0..5] are not touched; 3. the sums and the scalars, the explore variant taking
// the counter for Silverman's rule; 4. the widths (the first deposit fixes sigma0 before them); 5. the heights, in load_new; 6. the deposit.
// Without adapt and without explore these are opes_step_steps_f64's operations in its order: the same bits.  Returns whether the step
// went past 2: where it did not, only run[6] has changed and the caller leaves the table's state as it is.
template <class Ex>
MOLANN_HD bool opes_step_modes_steps_f64(Ex& ex, long capacity, int d, const double* period, long n_walkers, double threshold, double cutoff,
                                         double beta, int flags, bool adaptive, const double* sigma0, const double* sigma_min, double biasfactor,
                                         double adaptive_stride, long& n, double& S, double& merges, double& refused, double (&run)[8]) {
#pragma clang fp contract(off)
    const int fixed_sigma = (flags & OPES_FLAG_FIXED_SIGMA) ? 1 : 0;
    const int explore = (flags & OPES_FLAG_EXPLORE) ? 1 : 0;
    double observations = 0.0;
    if (adaptive) {
        observations = run[6] + 1.0;
        const double tau = observations < adaptive_stride ? observations : adaptive_stride;
        ex.observe(n_walkers, tau);
        run[6] = observations;
        if ((flags & OPES_FLAG_OBSERVE) || (run[7] == 0.0 && observations < adaptive_stride)) return false;
    } else {
        run[6] = 0.0;
        run[7] = 0.0;
    }
    double count, sum_w, sum_w2;
    ex.walker_sums(n_walkers, count, sum_w, sum_w2);
    run[0] = run[0] + count;
    run[1] = run[1] + sum_w;
    run[2] = run[2] + sum_w2;
    opes_run_scalars_f64(run[0], run[1], run[2], beta, d, fixed_sigma, run[3], run[4], run[5]);
    if (explore) run[4] = opes_silverman_scale_f64(run[0], d, fixed_sigma);
    ex.explore = explore;
    if (adaptive) {
        const double factor = explore ? 1.0 : biasfactor;
        if (run[7] == 0.0) {
            ex.first_deposit(n_walkers, observations, factor, biasfactor, sigma_min);
            run[7] = 1.0;
        }
        ex.width_count = observations;
        ex.width_factor = factor;
        ex.width_scale = run[4];
        ex.fixed_sigma = fixed_sigma;
    } else {
        ex.ratio = opes_step_widths_f64(sigma0, sigma_min, run[4], d, ex.step_sigma);
    }
    opes_deposit_steps_f64(ex, capacity, d, period, n_walkers, threshold, cutoff, n, S, merges, refused);
    return true;
}

} // namespace molann
