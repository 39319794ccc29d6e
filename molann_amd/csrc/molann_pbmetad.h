// molann_pbmetad.h - the arithmetic of parallel-bias metadynamics (Pfaendtner and Bonomi, JCTC 2015; PLUMED's PBMETAD), one copy for the
// device (frames_value_pbmetad_f64_kernel of molann_dev_pbmetad_f64.inc, pbmetad_deposit_f64_kernel of molann_dev_pbmetad_deposit_f64.inc)
// and for the two host twins (molann_value_f64.inc, molann_pbmetad_deposit_f64.inc).  It lives in a header of its own, not in
// molann_math.h: that file travels inside the library as the source of the kernels compiled at run time, none of which uses any of this,
// and stays byte for byte what those kernels were built from.  Included by molann_kernels.hip after molann_math.h.
//
// K <= PBMETAD_MAX_K one-dimensional tables T_k (n_k >= 4 points at lower_k + i h_k, periodic with period n_k h_k or not) lie back to back
// in one buffer.  Per frame, with y_k the k-th chosen output:
//   V_k  = ((T_k[i0] a0 + T_k[i1] a1) + T_k[i2] a2) + T_k[i3] a3,   V_k' the same sum with b for a      (idx, a, b = grid_axis_f64)
//   m    = min_k V_k,   e_k = exp(-((V_k - m) / kT)),   S = ((e_0 + e_1) + ...) k ascending,   w_k = e_k / S
//   V_PB = m - kT log S,   dV_PB / dy_k = w_k V_k'
// With K = 1: e_0 = exp(-0) = 1, S = 1, w_0 = 1 and V_PB = V_0 - kT 0 = V_0, exactly.  A V_k that is not finite makes V_PB and every w
// NaN.  Per walker of a deposit, from the V_k a bias launch wrote: h_k = metad_height_f64(height0, V_k, inv_dT) w_k; the walker is valid
// when every V_k, every centre and every h_k is finite; then T_k[g] = T_k[g] + h_k exp(-1/2 (delta / sigma_k)^2) where h_k > 0 and
// (delta / sigma_k)^2 <= cutoff^2, with metad_axis_delta_f64 / metad_axis_factor_f64 / metad_axis_reach_f64 of molann_math.h.
// Nothing is contracted: the host and the device differ only where their exp and log do.
#pragma once
#include "molann_math.h"

namespace molann {

constexpr int PBMETAD_MAX_K = HILLS_MAX_D;     // axes of a parallel bias
constexpr int PBMETAD_CHUNK = 64;              // walkers a deposit block stages at a time

MOLANN_HD bool pbmetad_finite_f64(double v) { return fabs(v) <= 1.7976931348623157e308; }

// one axis: the table's value and derivative at y.  The four loads are unconditional and every index is in range for every bit pattern
// of y (grid_axis_f64); the sums have one order.
MOLANN_HD void pbmetad_axis_value_f64(double y, const double* T, long n, double lower, double h, bool periodic, double& V, double& dV) {
#pragma clang fp contract(off)
    long idx[4];
    double a[4], b[4];
    grid_axis_f64(y, n, lower, h, periodic, idx, a, b);
    const double t0 = T[idx[0]], t1 = T[idx[1]], t2 = T[idx[2]], t3 = T[idx[3]];
    V = ((t0 * a[0] + t1 * a[1]) + t2 * a[2]) + t3 * a[3];
    dV = ((t0 * b[0] + t1 * b[1]) + t2 * b[2]) + t3 * b[3];
}

// the soft minimum of V[0..K) and every axis' share of it: returns V_PB, w[k] = e_k / S (0 for k >= K)
MOLANN_HD double pbmetad_softmin_f64(const double (&V)[PBMETAD_MAX_K], int K, double kT, double (&w)[PBMETAD_MAX_K]) {
#pragma clang fp contract(off)
    bool finite = true;
    double m = V[0];
#pragma unroll
    for (int k = 0; k < PBMETAD_MAX_K; ++k)
        if (k < K) {
            finite = finite && pbmetad_finite_f64(V[k]);
            m = V[k] < m ? V[k] : m;
        }
    double S = 0.0;
#pragma unroll
    for (int k = 0; k < PBMETAD_MAX_K; ++k) {
        w[k] = 0.0;
        if (k < K) {
            w[k] = exp(-((V[k] - m) / kT));
            S = k == 0 ? w[0] : S + w[k];
        }
    }
#pragma unroll
    for (int k = 0; k < PBMETAD_MAX_K; ++k)
        if (k < K) w[k] = finite ? w[k] / S : (double)NAN;
    return finite ? m - kT * log(S) : (double)NAN;   // all finite: every e_k in [0, 1] and the minimum's is 1, so 1 <= S <= K
}

// an output's cotangent takes its axis' share of the parallel bias' derivative: one product, one sum
MOLANN_HD double pbmetad_cotangent_f64(double cot, double w, double dV) {
#pragma clang fp contract(off)
    const double t = w * dV;
    return cot + t;
}

// a walker's K heights from its K biases; returns whether the walker deposits (every V_k, centre and height finite)
MOLANN_HD bool pbmetad_walker_heights_f64(const double (&V)[PBMETAD_MAX_K], const double (&y)[PBMETAD_MAX_K], int K, double height0, double inv_dT,
                                          double kT, double (&h)[PBMETAD_MAX_K]) {
#pragma clang fp contract(off)
    double w[PBMETAD_MAX_K];
    pbmetad_softmin_f64(V, K, kT, w);
    bool ok = true;
#pragma unroll
    for (int k = 0; k < PBMETAD_MAX_K; ++k) {
        h[k] = 0.0;
        if (k < K) {
            h[k] = metad_height_f64(height0, V[k], inv_dT) * w[k];
            ok = ok && pbmetad_finite_f64(V[k]) && pbmetad_finite_f64(y[k]) && pbmetad_finite_f64(h[k]);
        }
    }
    return ok;
}

// whether a valid walker's hill on one axis reaches the entries i0..i1 (a height of exactly 0 adds nothing anywhere)
MOLANN_HD bool pbmetad_axis_reaches_f64(double hk, long i0, long i1, double y, double lower, double h, double P, double sigma, double c2) {
    return hk > 0.0 && metad_axis_reach_f64(i0, i1, y, lower, h, P, sigma) <= c2;
}

// entry i of an axis takes one reaching hill: metad_deposit_f64_kernel<1>'s arithmetic per entry; returns whether acc changed hands
MOLANN_HD bool pbmetad_entry_add_f64(long i, double hk, double y, double lower, double h, double P, double sigma, double c2, double& acc) {
#pragma clang fp contract(off)
    double q, e;
    metad_axis_factor_f64(metad_axis_delta_f64(i, y, lower, h, P), sigma, q, e);
    if (!(q <= c2)) return false;
    acc = acc + hk * e;
    return true;
}

// One walker's step of state = (hills, refused, sum_heights, steps, logged, ...), in walker order by one thread: a valid walker is
// counted, its K heights added (k ascending) and its row (centre_0.., h_0..) appended to log[log_capacity, 2 K] while there is room; any
// other is refused.  `logged` comes from opes_live_count_f64, so a row index lies in [0, log_capacity) whatever the state held.
MOLANN_HD void pbmetad_state_walker_f64(bool valid, const double (&h)[PBMETAD_MAX_K], const double (&y)[PBMETAD_MAX_K], int K, double* log,
                                        long log_capacity, double& hills, double& refused, double& sum_heights, long& logged) {
#pragma clang fp contract(off)
    if (!valid) {
        refused = refused + 1.0;
        return;
    }
    hills = hills + 1.0;
#pragma unroll
    for (int k = 0; k < PBMETAD_MAX_K; ++k)
        if (k < K) sum_heights = sum_heights + h[k];
    if (logged < log_capacity) {
        double* row = log + logged * (2 * K);
#pragma unroll
        for (int k = 0; k < PBMETAD_MAX_K; ++k)
            if (k < K) { row[k] = y[k]; row[K + k] = h[k]; }
        logged += 1;
    }
}

} // namespace molann
