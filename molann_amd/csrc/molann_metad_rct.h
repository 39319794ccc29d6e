// molann_metad_rct.h - the arithmetic of a metadynamics run's reweighting offset c(t) (Tiwary-Parrinello; PLUMED's CALC_RCT), one copy for
// the device (metad_rct_partial_f64_kernel and metad_rct_combine_f64_kernel, molann_dev_metad_rct_f64.inc) and for the host twin
// (molann_metad_rct_f64.inc).  It lives in a header of its own, not in molann_math.h: that file travels inside the library as the source
// of the kernels compiled at run time, none of which uses any of this, and stays byte for byte what those kernels were built from.
// Included by molann_kernels.hip after molann_math.h.
//
// The table is read flat, V_g for g < n.  With beta = 1 / kT, a0 = beta + inv_dT and aV = inv_dT (inv_dT = 1 / (kT (biasfactor - 1)), 0 for
// plain metadynamics):
//   M = max_g V_g,   S0 = sum_g exp(a0 (V_g - M)),   SV = sum_g exp(aV (V_g - M)),   c = M + kT (log S0 - log SV)
// which is kT log(Z_0 / Z_V) with kT (a0 - aV) = 1 used, so no a M is formed and cancelled.  Every exponent is <= 0 and S0, SV >= 1.
//
// The order of the sums is fixed and has nothing to do with the launch:
//   * chunk c is the entries [2048 c, 2048 c + 2048) of the table, cut at n; slot j of thread t of a chunk is entry 2048 c + 256 j + t
//     (j < 8, t < 256), so a wave's load of one slot is 512 consecutive bytes;
//   * a thread's maximum and its two sums take its slots in the order j = 0..7 (metad_rct_thread_max_f64, metad_rct_thread_sums_f64); an
//     entry that is not finite or lies past n enters neither and is counted in `bad` where it lies inside n;
//   * THE TREE joins 256 thread values x_0..x_255: within each wave of 64, for off = 32, 16, 8, 4, 2, 1 in turn,
//     x_i = op(x_i, x_{i + off}) for every i < off at once, which leaves the wave's value in x_0; the four waves' values w_0..w_3 are joined
//     as op(op(w_0, w_1), op(w_2, w_3)) (metad_rct_quad_f64).  metad_rct_tree_f64 is that tree on an array; the kernels run the same
//     pairs with __shfl_down and four doubles of LDS.  op is MetadRctMax or MetadRctAdd;
//   * the combine step's thread t takes the chunks t, t + 256, ... ascending (metad_rct_combine_max_f64, metad_rct_combine_sums_f64) and
//     the 256 thread values go through the same tree.
// Nothing is contracted: the host and the device differ only where their exp and log do.
#pragma once
#include "molann_math.h"

namespace molann {

constexpr int METAD_RCT_THREADS = 256, METAD_RCT_SLOTS = 8, METAD_RCT_CHUNK = METAD_RCT_THREADS * METAD_RCT_SLOTS;
constexpr int METAD_RCT_ROW = 4;            // a row of partials: (m_c, s0_c, sV_c, bad_c)
constexpr long METAD_RCT_MAX_BLOCKS = 1024;  // of the partial launch; a block walks its chunks by the grid's size

MOLANN_HD constexpr long metad_rct_chunks(long n) { return (n + METAD_RCT_CHUNK - 1) / METAD_RCT_CHUNK; }

MOLANN_HD bool metad_rct_finite_f64(double v) { return fabs(v) <= 1.7976931348623157e308; }

// a count kept in a double, as the deposit reads its own: not finite or negative reads as 0
MOLANN_HD double metad_rct_count_f64(double v) { return v >= 0.0 && v <= 1.7976931348623157e308 ? v : 0.0; }

// whether this call updates: always without a state, else when the steps the deposit has counted are a multiple of the stride
// (fmod is exact).  `steps` is what slot 5 of rct records.
MOLANN_HD bool metad_rct_due_f64(const double* state, long stride, double& steps) {
    steps = 0.0;
    if (!state) return true;
    steps = metad_rct_count_f64(state[3]);
    return fmod(steps, (double)stride) == 0.0;
}

// the later of two equals stays out: with the fixed tree a table of +0.0 and -0.0 has one maximum on the host and on the device
MOLANN_HD double metad_rct_max2_f64(double a, double b) { return b > a ? b : a; }
struct MetadRctMax { MOLANN_HD double operator()(double a, double b) const { return metad_rct_max2_f64(a, b); } };
struct MetadRctAdd { MOLANN_HD double operator()(double a, double b) const { return a + b; } };

// exp(a (v - m)) for v <= m: the difference is held to -DBL_MAX, so a = 0 gives 1 where v - m overflows, not 0 inf
MOLANN_HD double metad_rct_term_f64(double a, double v, double m) {
#pragma clang fp contract(off)
    double diff = v - m;
    if (diff < -1.7976931348623157e308) diff = -1.7976931348623157e308;
    const double x = a * diff;
    return exp(x);
}

// a thread's slots, j ascending: live[j] is whether slot j lies inside the table
MOLANN_HD double metad_rct_thread_max_f64(const double (&v)[METAD_RCT_SLOTS], const bool (&live)[METAD_RCT_SLOTS], int& bad) {
    double m = -INFINITY;
    bad = 0;
#pragma unroll
    for (int j = 0; j < METAD_RCT_SLOTS; ++j)
        if (live[j]) {
            if (metad_rct_finite_f64(v[j])) m = metad_rct_max2_f64(m, v[j]);
            else ++bad;
        }
    return m;
}

MOLANN_HD void metad_rct_thread_sums_f64(const double (&v)[METAD_RCT_SLOTS], const bool (&live)[METAD_RCT_SLOTS], double m, double a0, double aV,
                                         double& s0, double& sV) {
#pragma clang fp contract(off)
    s0 = 0.0;
    sV = 0.0;
#pragma unroll
    for (int j = 0; j < METAD_RCT_SLOTS; ++j)
        if (live[j] && metad_rct_finite_f64(v[j])) {
            s0 = s0 + metad_rct_term_f64(a0, v[j], m);
            sV = sV + metad_rct_term_f64(aV, v[j], m);
        }
}

template <class Op>
MOLANN_HD double metad_rct_quad_f64(double w0, double w1, double w2, double w3, Op op) { return op(op(w0, w1), op(w2, w3)); }

// THE TREE on x[256], in place
template <class Op>
MOLANN_HD double metad_rct_tree_f64(double* x, Op op) {
    for (int w = 0; w < METAD_RCT_THREADS; w += 64)
        for (int off = 32; off >= 1; off >>= 1)
            for (int i = 0; i < off; ++i) x[w + i] = op(x[w + i], x[w + i + off]);
    return metad_rct_quad_f64(x[0], x[64], x[128], x[192], op);
}

// the combine step's thread t: its chunks' maxima, then its chunks' sums moved to the table's maximum M.  A chunk without a finite
// entry (m_c = -inf, sums 0) adds nothing.
MOLANN_HD double metad_rct_combine_max_f64(const double* partials, long rows, int t) {
    double m = -INFINITY;
    for (long c = t; c < rows; c += METAD_RCT_THREADS) m = metad_rct_max2_f64(m, partials[c * METAD_RCT_ROW]);
    return m;
}

MOLANN_HD void metad_rct_combine_sums_f64(const double* partials, long rows, int t, double M, double a0, double aV, double& s0, double& sV,
                                          double& bad) {
#pragma clang fp contract(off)
    s0 = 0.0;
    sV = 0.0;
    bad = 0.0;
    for (long c = t; c < rows; c += METAD_RCT_THREADS) {
        const double* p = partials + c * METAD_RCT_ROW;
        bad = bad + p[3];
        if (p[0] > -INFINITY) {
            const double t0 = p[1] * metad_rct_term_f64(a0, p[0], M);
            const double tV = p[2] * metad_rct_term_f64(aV, p[0], M);
            s0 = s0 + t0;
            sV = sV + tV;
        }
    }
}

// rct[8] = (c, updates + 1, M, a0 M + log S0, aV M + log SV, steps at this update, bad, 0); with a bad entry slots 0, 2, 3, 4 are NaN
MOLANN_HD void metad_rct_final_f64(double M, double S0, double SV, double bad, double kT, double a0, double aV, double steps, double* rct) {
#pragma clang fp contract(off)
    const double l0 = log(S0), lV = log(SV);
    const double gap = l0 - lV;
    const double lift = kT * gap;
    const double p0 = a0 * M, pV = aV * M;
    const bool ok = !(bad > 0.0);
    const double nan = NAN;
    const double updates = metad_rct_count_f64(rct[1]);
    rct[0] = ok ? M + lift : nan;
    rct[1] = updates + 1.0;
    rct[2] = ok ? M : nan;
    rct[3] = ok ? p0 + l0 : nan;
    rct[4] = ok ? pV + lV : nan;
    rct[5] = steps;
    rct[6] = bad;
    rct[7] = 0.0;
}

} // namespace molann
