// molann_metad_cov.h - the arithmetic of metadynamics hills with a full covariance matrix (the adaptive Gaussians of Branduardi, Bussi and
// Parrinello, JCTC 2012; PLUMED's METAD ADAPTIVE=DIFF and ADAPTIVE=GEOM), one copy for the device (metad_widths_f64_kernel and
// metad_deposit_cov_f64_kernel, molann_dev_metad_cov_f64.inc) and for the host twins (molann_metad_cov_f64.inc).  Like molann_metad_rct.h it
// lives in a header of its own, not in molann_math.h, which travels inside the library as the source of the kernels compiled at run time
// and stays byte for byte what those were built from.  Included by molann_kernels.hip after molann_metad_rct.h.
//
// d <= GRID_MAX_D = 3 axes.  In memory a covariance is the row-major upper triangle, T = d (d + 1) / 2 doubles (c00 c01 c02 c11 c12 c22 for
// d = 3): entry (i, j), i <= j, sits at metad_cov_at(d, i, j).  In registers every function here holds it in the d = 3 layout whatever d
// is (unused diagonal entries 1, unused off-diagonal entries 0) and every loop runs over GRID_MAX_D with a `k < d` guard, so the local
// arrays are indexed by constants and nothing goes to scratch.  Nothing is contracted: the device and the host differ only by exp.
//
// OBSERVATION (DIFF).  A walker's row of `adapt` is (n_a, mean[d], cov[T]); decay = 1 / window.  A y that is not finite leaves the row's
// bits (the caller counts it).  n_a == 0: mean = y, cov = 0, n_a = 1.  Otherwise delta_k = y_k - mean_k, wrapped to
// delta - P rint(delta / P) on a periodic axis (metad_axis_delta_f64's rule); mean_k += decay delta_k, then on a periodic axis
// mean_k -= P floor((mean_k - lower_k) / P); cov_ij += decay (delta_i delta_j - cov_ij) with the deltas formed before the mean moved;
// n_a += 1.
//
// THE HILL'S COVARIANCE.  DIFF: cov_a once n_a >= window, diag(sigma_k^2) before.  GEOM: C_ij = sigma_i sigma_j M[col_i, col_j], M the
// metric J J^T the caller passes.
//
// LIMITS (PLUMED's SIGMA_MIN / SIGMA_MAX), k ascending: target = clamp(C_kk, sigma_min_k^2, sigma_max_k^2).  Where target != C_kk and
// C_kk > 0, row and column k are multiplied by sqrt(target / C_kk) and C_kk is set to target exactly - a congruence with a diagonal
// matrix, so a positive-definite matrix stays one and every correlation C_ij / sqrt(C_ii C_jj) keeps its value.  Where target != C_kk
// and C_kk is not > 0, the off-diagonal entries of k become 0 and C_kk = target.  Limits 0 and +inf change nothing.
//
// FACTOR AND EXPONENT.  C = L L^T with pivots p_k = C_kk - sum_{j<k} L_kj^2; the matrix is USABLE when every entry is finite and every
// p_k > 1e-12 C_kk (which a C_kk <= 0 fails).  z_k = (delta_k - sum_{j<k} L_kj z_j) / L_kk, q = sum_k z_k^2 with k ascending, and the
// term is h exp(-(0.5 q)).  No inverse matrix is formed.  L is kept in the same triangle: L_kj, j <= k, at (j, k).
//
// REACH.  For every k, q = delta^T C^-1 delta >= delta_k^2 / C_kk: with e_k the k-th unit vector, Cauchy-Schwarz in the inner product of
// C^-1 gives delta_k^2 = (e_k^T C C^-1 delta)^2 <= (e_k^T C e_k) (delta^T C^-1 delta) = C_kk q.  So a tile's per-axis lower bound is
// metad_axis_reach_f64(i0, i1, y_k, lower_k, h_k, P_k, sqrt(C_kk)), a bound of delta_k^2 / C_kk over the tile's indices, and a hill is
// skipped for a tile only when SOME SINGLE AXIS's bound exceeds c2 (1 + 1e-12) - the factor covers the roundings of sqrt, the division
// and the computed q.  The bounds are NOT summed: the sum bounds q only where the Gaussian is a product over the axes.  Every entry
// still decides by its own q <= c2, so skipping can never change a result; it only saves work.
#pragma once
#include "molann_math.h"

namespace molann {

constexpr int METAD_COV_MAX_T = GRID_MAX_D * (GRID_MAX_D + 1) / 2;
constexpr int METAD_COV_DIFF = 1, METAD_COV_GEOM = 2;    // the widths call's `mode`

MOLANN_HD constexpr int metad_cov_len(int d) { return d * (d + 1) / 2; }
MOLANN_HD constexpr int metad_cov_at(int d, int i, int j) { return i * d - i * (i - 1) / 2 + (j - i); }    // i <= j
MOLANN_HD constexpr int metad_cov_sym(int i, int j) { return i <= j ? metad_cov_at(GRID_MAX_D, i, j) : metad_cov_at(GRID_MAX_D, j, i); }
MOLANN_HD constexpr int metad_cov_row(int d) { return 1 + d + metad_cov_len(d); }    // doubles in a walker's row of adapt
MOLANN_HD constexpr int metad_cov_log_row(int d) { return d + metad_cov_len(d) + 1; }

MOLANN_HD bool metad_cov_finite_f64(double v) { return fabs(v) <= 1.7976931348623157e308; }

// memory (d's triangle, any stride the caller resolved) <-> registers (the d = 3 layout)
MOLANN_HD void metad_cov_load_f64(const double* p, int d, double (&C)[METAD_COV_MAX_T]) {
#pragma unroll
    for (int i = 0; i < GRID_MAX_D; ++i)
#pragma unroll
        for (int j = i; j < GRID_MAX_D; ++j) C[metad_cov_sym(i, j)] = j < d ? p[metad_cov_at(d, i, j)] : i == j ? 1.0 : 0.0;
}
MOLANN_HD void metad_cov_store_f64(const double (&C)[METAD_COV_MAX_T], int d, double* p) {
#pragma unroll
    for (int i = 0; i < GRID_MAX_D; ++i)
#pragma unroll
        for (int j = i; j < GRID_MAX_D; ++j)
            if (j < d) p[metad_cov_at(d, i, j)] = C[metad_cov_sym(i, j)];
}
MOLANN_HD void metad_cov_diag_f64(const double (&sigma)[GRID_MAX_D], int d, double (&C)[METAD_COV_MAX_T]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < GRID_MAX_D; ++i)
#pragma unroll
        for (int j = i; j < GRID_MAX_D; ++j) C[metad_cov_sym(i, j)] = i != j ? 0.0 : i < d ? sigma[i] * sigma[i] : 1.0;
}

// one observation of y by a walker's row (n_a, mean[d], cov[T]); false: y is not finite and the row keeps its bits
MOLANN_HD bool metad_cov_observe_f64(double* row, const double (&y)[GRID_MAX_D], const double (&lower)[GRID_MAX_D], const double (&P)[GRID_MAX_D], int d,
                                     double decay) {
#pragma clang fp contract(off)
    bool finite = true;
#pragma unroll
    for (int k = 0; k < GRID_MAX_D; ++k)
        if (k < d) finite = finite && metad_cov_finite_f64(y[k]);
    if (!finite) return false;
    double* mean = row + 1;
    double* cov = row + 1 + d;
    if (row[0] == 0.0) {
#pragma unroll
        for (int k = 0; k < GRID_MAX_D; ++k)
            if (k < d) mean[k] = y[k];
#pragma unroll
        for (int k = 0; k < METAD_COV_MAX_T; ++k)
            if (k < metad_cov_len(d)) cov[k] = 0.0;
        row[0] = 1.0;
        return true;
    }
    double delta[GRID_MAX_D] = {0., 0., 0.};
#pragma unroll
    for (int k = 0; k < GRID_MAX_D; ++k)
        if (k < d) {
            double dk = y[k] - mean[k];
            if (P[k] > 0.0) {
                const double turns = rint(dk / P[k]);
                const double whole = P[k] * turns;
                dk = dk - whole;
            }
            delta[k] = dk;
            const double step = decay * dk;
            double m = mean[k] + step;
            if (P[k] > 0.0) {
                const double turns = floor((m - lower[k]) / P[k]);
                const double whole = P[k] * turns;
                m = m - whole;
            }
            mean[k] = m;
        }
#pragma unroll
    for (int i = 0; i < GRID_MAX_D; ++i)
#pragma unroll
        for (int j = i; j < GRID_MAX_D; ++j)
            if (j < d) {
                const double c = cov[metad_cov_at(d, i, j)];
                const double prod = delta[i] * delta[j];
                const double step = decay * (prod - c);
                cov[metad_cov_at(d, i, j)] = c + step;
            }
    row[0] = row[0] + 1.0;
    return true;
}

// DIFF's hill: the running covariance once the row holds `window` observations, the run's fixed widths before
MOLANN_HD void metad_cov_hill_diff_f64(const double* row, const double (&sigma)[GRID_MAX_D], int d, double window, double (&C)[METAD_COV_MAX_T]) {
    if (row[0] >= window) metad_cov_load_f64(row + 1 + d, d, C);
    else metad_cov_diag_f64(sigma, d, C);
}

// GEOM's hill: C_ij = (sigma_i sigma_j) M[col_i ld + col_j], M one walker's metric
MOLANN_HD void metad_cov_hill_geom_f64(const double* M, long ld, const int (&col)[GRID_MAX_D], const double (&sigma)[GRID_MAX_D], int d,
                                       double (&C)[METAD_COV_MAX_T]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int i = 0; i < GRID_MAX_D; ++i)
#pragma unroll
        for (int j = i; j < GRID_MAX_D; ++j) {
            double c = i == j ? 1.0 : 0.0;
            if (j < d) {
                const double s = sigma[i] * sigma[j];
                c = s * M[(long)col[i] * ld + col[j]];
            }
            C[metad_cov_sym(i, j)] = c;
        }
}

MOLANN_HD void metad_cov_limits_f64(double (&C)[METAD_COV_MAX_T], const double (&sigma_min)[GRID_MAX_D], const double (&sigma_max)[GRID_MAX_D], int d) {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < GRID_MAX_D; ++k)
        if (k < d) {
            const double ckk = C[metad_cov_sym(k, k)];
            const double lo = sigma_min[k] * sigma_min[k], hi = sigma_max[k] * sigma_max[k];
            const double target = ckk < lo ? lo : ckk > hi ? hi : ckk;
            if (target != ckk) {
                const bool scale = ckk > 0.0;
                const double s = scale ? sqrt(target / ckk) : 0.0;
#pragma unroll
                for (int i = 0; i < GRID_MAX_D; ++i)
                    if (i != k && i < d) C[metad_cov_sym(i, k)] = scale ? C[metad_cov_sym(i, k)] * s : 0.0;
                C[metad_cov_sym(k, k)] = target;
            }
        }
}

// C = L L^T; true where the matrix is usable.  L of a matrix that is not usable is never read.
MOLANN_HD bool metad_cov_factor_f64(const double (&C)[METAD_COV_MAX_T], int d, double (&L)[METAD_COV_MAX_T]) {
#pragma clang fp contract(off)
    bool ok = true;
#pragma unroll
    for (int i = 0; i < GRID_MAX_D; ++i)
#pragma unroll
        for (int j = i; j < GRID_MAX_D; ++j) {
            if (j < d) ok = ok && metad_cov_finite_f64(C[metad_cov_sym(i, j)]);
            L[metad_cov_sym(i, j)] = i == j ? 1.0 : 0.0;
        }
#pragma unroll
    for (int k = 0; k < GRID_MAX_D; ++k)
        if (k < d) {
            const double ckk = C[metad_cov_sym(k, k)];
            double p = ckk;
#pragma unroll
            for (int j = 0; j < k; ++j) {
                const double l = L[metad_cov_sym(j, k)];
                p = p - l * l;
            }
            ok = ok && p > 1e-12 * ckk;
            const double lkk = sqrt(p);
            L[metad_cov_sym(k, k)] = lkk;
#pragma unroll
            for (int i = k + 1; i < GRID_MAX_D; ++i)
                if (i < d) {
                    double s = C[metad_cov_sym(k, i)];
#pragma unroll
                    for (int j = 0; j < k; ++j) s = s - L[metad_cov_sym(j, i)] * L[metad_cov_sym(j, k)];
                    L[metad_cov_sym(k, i)] = s / lkk;
                }
        }
    return ok;
}

// q = |L^-1 delta|^2 by the forward substitution, k ascending
MOLANN_HD double metad_cov_q_f64(const double (&delta)[GRID_MAX_D], const double (&L)[METAD_COV_MAX_T], int d) {
#pragma clang fp contract(off)
    const double z0 = delta[0] / L[metad_cov_sym(0, 0)];
    double q = z0 * z0;
    if (d > 1) {
        const double z1 = (delta[1] - L[metad_cov_sym(0, 1)] * z0) / L[metad_cov_sym(1, 1)];
        q = q + z1 * z1;
        if (d > 2) {
            const double s = L[metad_cov_sym(0, 2)] * z0 + L[metad_cov_sym(1, 2)] * z1;
            const double z2 = (delta[2] - s) / L[metad_cov_sym(2, 2)];
            q = q + z2 * z2;
        }
    }
    return q;
}

MOLANN_HD double metad_cov_term_f64(double h, double q) {
#pragma clang fp contract(off)
    return h * exp(-(0.5 * q));
}

// whether a hill may reach the tile i0..i1: no single axis's bound exceeds c2 (1 + 1e-12) (REACH above; c2 = +inf: always)
MOLANN_HD bool metad_cov_reach_f64(const long (&i0)[GRID_MAX_D], const long (&i1)[GRID_MAX_D], const double (&y)[GRID_MAX_D], const double (&lower)[GRID_MAX_D],
                                   const double (&h)[GRID_MAX_D], const double (&P)[GRID_MAX_D], const double (&C)[METAD_COV_MAX_T], int d, double c2) {
#pragma clang fp contract(off)
    const double edge = c2 * (1.0 + 1e-12);
    bool reach = true;
#pragma unroll
    for (int k = 0; k < GRID_MAX_D; ++k)
        if (k < d) reach = reach && !(metad_axis_reach_f64(i0[k], i1[k], y[k], lower[k], h[k], P[k], sqrt(C[metad_cov_sym(k, k)])) > edge);
    return reach;
}

// metad_state_walker_f64 for a hill with a covariance: the log's row is (y_k..., C in d's triangle, h), d + T + 1 doubles
MOLANN_HD void metad_cov_state_walker_f64(bool valid, double h, const double (&y)[GRID_MAX_D], const double (&C)[METAD_COV_MAX_T], int d, double* log,
                                          long log_capacity, double& hills, double& refused, double& sum_heights, long& logged) {
#pragma clang fp contract(off)
    if (!valid) {
        refused = refused + 1.0;
        return;
    }
    hills = hills + 1.0;
    sum_heights = sum_heights + h;
    if (logged < log_capacity) {
        double* row = log + logged * metad_cov_log_row(d);
#pragma unroll
        for (int k = 0; k < GRID_MAX_D; ++k)
            if (k < d) row[k] = y[k];
        metad_cov_store_f64(C, d, row + d);
        row[d + metad_cov_len(d)] = h;
        logged += 1;
    }
}

} // namespace molann
