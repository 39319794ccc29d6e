// san_metad_cov.cpp - the host twins of the adaptive metadynamics hills, molann_selftest_metad_widths_f64 and
// molann_selftest_metad_deposit_cov_f64, under AddressSanitizer and UndefinedBehaviorSanitizer in a stand-alone program: host code only,
// no GPU, nothing preloaded.  Every buffer is sized exactly (heap vectors): the table to its entries, y, V, cov and the metric to their
// strides' last element, adapt to its rows, the log to its capacity, so a read or a write past any of them is reported.  It runs a few
// hundred generated steps - every d, periodic and not, with and without a cutoff, strided inputs, a log shorter than the step - and
// malformed ones: NaN and infinite covariances, singular, negative and indefinite matrices, y that is not finite, bad strides and each
// refusal.  Build and run, from the repository root:
//
//   make -C molann_amd/csrc san
//   /opt/rocm/bin/hipcc -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       -Iinclude tools/san_metad_cov.cpp -Lmolann_amd/csrc -lmolann_hip_san -Wl,-rpath,$PWD/molann_amd/csrc -o tools/san_metad_cov
//   tools/san_metad_cov
//
// Prints one line per group and "ok"; any other end is a finding.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "molann_hip.h"

static int failures = 0;
#define EXPECT(cond)                                                          \
    do {                                                                      \
        if (!(cond)) {                                                        \
            std::printf("line %d: %s\n", __LINE__, #cond);                    \
            ++failures;                                                       \
        }                                                                     \
    } while (0)

static double uniform(uint64_t& s) {      // a small generator of its own: the same values everywhere
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    return (double)(s >> 11) / 9007199254740992.0;
}

struct Grid {
    int32_t d;
    int64_t shape[3];
    double lower[3], spacing[3];
    int32_t periodic[3];
    int64_t entries() const { return shape[0] * (d > 1 ? shape[1] : 1) * (d > 2 ? shape[2] : 1); }
};

static const Grid GRIDS[] = {{1, {4, 1, 1}, {-1.3, 0, 0}, {0.37, 1, 1}, {0, 0, 0}},        {1, {257, 1, 1}, {-1.3, 0, 0}, {0.37, 1, 1}, {1, 0, 0}},
                             {2, {5, 7, 1}, {-1.3, -1.7, 0}, {0.37, 0.48, 1}, {1, 0, 0}},  {2, {17, 33, 1}, {-1.3, -1.7, 0}, {0.37, 0.48, 1}, {0, 1, 0}},
                             {3, {4, 5, 6}, {-1.3, -1.7, -2.1}, {0.37, 0.48, 0.59}, {0, 1, 0}},
                             {3, {5, 9, 17}, {-1.3, -1.7, -2.1}, {0.37, 0.48, 0.59}, {1, 0, 1}}};

static int tri(int d) { return d * (d + 1) / 2; }

// a positive-definite matrix in the upper triangle: B B^T + I scaled to a few spacings
static void random_cov(uint64_t& seed, const Grid& g, double* c) {
    const int d = g.d;
    double B[3][3], C[3][3];
    for (int i = 0; i < d; ++i)
        for (int j = 0; j < d; ++j) B[i][j] = 2.0 * uniform(seed) - 1.0;
    for (int i = 0; i < d; ++i)
        for (int j = 0; j < d; ++j) {
            double s = i == j ? 1.0 : 0.0;
            for (int k = 0; k < d; ++k) s += B[i][k] * B[j][k];
            C[i][j] = s * (1.5 * g.spacing[i]) * (1.5 * g.spacing[j]);
        }
    int at = 0;
    for (int i = 0; i < d; ++i)
        for (int j = i; j < d; ++j) c[at++] = C[i][j];
}

// one deposit with exactly sized, strided buffers; `spoil` makes walker 1's matrix or centre malformed
static void one_deposit(const Grid& g, int64_t W, double cutoff, int64_t y_extra, int64_t v_stride, int64_t cov_extra, int64_t log_rows, int spoil,
                        uint64_t seed) {
    const int d = g.d, T = tri(d);
    const int64_t y_stride = d + y_extra, cov_stride = T + cov_extra;
    int32_t columns[3];
    for (int k = 0; k < d; ++k) columns[k] = (int32_t)(y_stride - 1 - k);      // the last columns, in reverse
    std::vector<double> table(g.entries()), y((W - 1) * y_stride + y_stride), V((W - 1) * v_stride + 1), cov((W - 1) * cov_stride + T), state(8, 0.0),
        log(log_rows * (d + T + 1), -7.0);
    for (double& v : table) v = 10.0 * uniform(seed) - 5.0;
    for (double& v : y) v = 0.0;
    for (int64_t w = 0; w < W; ++w) {
        for (int k = 0; k < d; ++k) y[w * y_stride + columns[k]] = g.lower[k] + (1.4 * uniform(seed) - 0.2) * g.shape[k] * g.spacing[k];
        V[w * v_stride] = 70.0 * uniform(seed) - 30.0;
        random_cov(seed, g, &cov[w * cov_stride]);
    }
    int64_t bad = 0;
    if (spoil && W > 1) {
        double* c = &cov[1 * cov_stride];
        bad = 1;
        switch (spoil) {
        case 1: c[T - 1] = NAN; break;
        case 2: c[0] = INFINITY; break;
        case 3: for (int k = 0; k < T; ++k) c[k] = d > 1 ? 1.0 : 0.0; break;          // rank one (d = 1: no width)
        case 4: c[T - 1] = -c[T - 1]; break;
        case 5: for (int k = 0; k < T; ++k) c[k] = 0.0; break;
        case 6: if (d > 1) c[1] = 10.0 * std::sqrt(c[0] * c[d]); else c[0] = -1.0; break;    // |c01| > sqrt(c00 c11)
        case 7: y[1 * y_stride + columns[0]] = NAN; break;
        case 8: V[1 * v_stride] = -1e5; break;                                         // the height overflows
        default: bad = 0;
        }
    }
    const std::vector<double> before = table;
    const int e = molann_selftest_metad_deposit_cov_f64(table.data(), d, g.shape, g.lower, g.spacing, g.periodic, columns, y.data(), y_stride, V.data(),
                                                        v_stride, cov.data(), cov_stride, W, 1.2, 1.0 / (2.494 * 9.0), cutoff, state.data(),
                                                        log_rows ? log.data() : nullptr, log_rows);
    EXPECT(e == MOLANN_OK);
    EXPECT(state[0] == (double)(W - bad) && state[1] == (double)bad && state[3] == 1.0);
    EXPECT(state[4] == (double)(log_rows ? (W - bad < log_rows ? W - bad : log_rows) : 0));
    bool finite = true, changed = false;
    for (size_t i = 0; i < table.size(); ++i) {
        finite = finite && std::isfinite(table[i]);
        changed = changed || table[i] != before[i];
    }
    EXPECT(finite && (changed || W == bad || std::isfinite(cutoff)));      // with a cutoff a hill outside the range may reach no point
    if (W == 1 && bad == 0 && log_rows > 0) EXPECT(log[0] == y[columns[0]] && log[d] == cov[0] && log[d + T] > 0.0);
    for (int64_t r = (int64_t)state[4] * (d + T + 1); r < (int64_t)log.size(); ++r) EXPECT(log[r] == -7.0);
}

// a walk of observations with exactly sized buffers, emitting now and then, one y not finite; then GEOM from a random metric
static void one_widths(const Grid& g, int64_t W, int64_t window, int64_t y_extra, int64_t cov_extra, bool limits, uint64_t seed) {
    const int d = g.d, T = tri(d);
    const int64_t y_stride = d + y_extra, cov_stride = T + cov_extra, row = 1 + d + T;
    int32_t columns[3];
    for (int k = 0; k < d; ++k) columns[k] = (int32_t)(y_stride - 1 - k);
    double sigma[3], lo[3], hi[3];
    for (int k = 0; k < d; ++k) { sigma[k] = 0.8 * g.spacing[k]; lo[k] = 0.5 * g.spacing[k]; hi[k] = 2.0 * g.spacing[k]; }
    std::vector<double> y(W * y_stride), adapt(W * row, 0.0), state(8, 0.0), out((W - 1) * cov_stride + T, -3.0);
    int64_t skipped = 0, emits = 0;
    for (int step = 0; step < 12; ++step) {
        for (int64_t w = 0; w < W; ++w)
            for (int k = 0; k < d; ++k)
                y[w * y_stride + columns[k]] = g.lower[k] + (0.11 * step + 0.6 * uniform(seed)) * g.shape[k] * g.spacing[k];     // drifts across the range
        if (step == 5) { y[(W - 1) * y_stride + columns[d - 1]] = INFINITY; ++skipped; }
        const int emit = step % 4 == 3;
        emits += emit;
        EXPECT(molann_selftest_metad_widths_f64(d, g.shape, g.lower, g.spacing, g.periodic, sigma, limits ? lo : nullptr, limits ? hi : nullptr, columns,
                                                y.data(), y_stride, nullptr, 0, 0, W, 1, window, emit, adapt.data(), state.data(),
                                                emit ? out.data() : nullptr, emit ? cov_stride : 0) == MOLANN_OK);
    }
    EXPECT(state[0] == (double)(12 * W - skipped) && state[1] == (double)emits && state[2] == (double)skipped);
    for (int64_t w = 0; w < W; ++w) {
        EXPECT(adapt[w * row] == (w == W - 1 ? 11.0 : 12.0));
        for (int k = 0; k < d; ++k) {
            const double m = adapt[w * row + 1 + k];
            EXPECT(std::isfinite(m) && (!g.periodic[k] || (m >= g.lower[k] && m < g.lower[k] + g.shape[k] * g.spacing[k])));
        }
        int at = 0;
        for (int i = 0; i < d; ++i)
            for (int j = i; j < d; ++j, ++at) {
                const double c = out[w * cov_stride + at];
                EXPECT(std::isfinite(c));
                if (i == j && limits) EXPECT(c >= lo[i] * lo[i] && c <= hi[i] * hi[i]);
            }
    }
    // GEOM: a metric of n_out = d + 1 outputs, sized exactly
    const int64_t n_out = d + 1;
    std::vector<double> metric(W * n_out * n_out);
    for (int64_t w = 0; w < W; ++w)
        for (int64_t i = 0; i < n_out; ++i)
            for (int64_t j = 0; j <= i; ++j)
                metric[(w * n_out + i) * n_out + j] = metric[(w * n_out + j) * n_out + i] = (i == j ? 2.0 : 0.5) * (0.5 + uniform(seed));
    int32_t cols[3];
    for (int k = 0; k < d; ++k) cols[k] = (int32_t)(n_out - 1 - k);
    EXPECT(molann_selftest_metad_widths_f64(d, g.shape, g.lower, g.spacing, g.periodic, sigma, limits ? lo : nullptr, limits ? hi : nullptr, cols, nullptr, 0,
                                            metric.data(), n_out * n_out, n_out, W, 2, 0, 1, nullptr, state.data(), out.data(), cov_stride) == MOLANN_OK);
    EXPECT(state[1] == (double)(emits + 1) && state[0] == (double)(12 * W - skipped));
    for (int64_t w = 0; w < W; ++w)
        if (!limits) EXPECT(out[w * cov_stride] == (sigma[0] * sigma[0]) * metric[(w * n_out + cols[0]) * n_out + cols[0]]);
}

static void refusals() {
    const Grid& g = GRIDS[2];
    const int64_t W = 3;
    std::vector<double> table(g.entries(), 0.0), y(W * 2, 0.1), V(W, 0.0), cov = {0.3, 0.1, 0.4, 0.3, 0.1, 0.4, 0.3, 0.1, 0.4}, state(8, 0.0), adapt(W * 6, 0.0),
        astate(8, 0.0), out(W * 3, 0.0), metric(W * 4, 1.0);
    double sigma[2] = {0.3, 0.4}, bad_sigma[2] = {0.3, -0.4}, neg[2] = {-0.1, 0.1}, small[2] = {0.1, 0.1}, big[2] = {0.2, 0.2};
    int32_t far[2] = {0, 2};
    double* odd = (double*)((char*)cov.data() + 4);
    auto dep = [&](double* t, int32_t d, const int64_t* shape, const int32_t* columns, const double* yy, int64_t ys, const double* c, int64_t cs, int64_t n,
                   double h0, double cut, double* st, int64_t cap) {
        return molann_selftest_metad_deposit_cov_f64(t, d, shape, g.lower, g.spacing, g.periodic, columns, yy, ys, V.data(), 1, c, cs, n, h0, 0.04, cut, st,
                                                     nullptr, cap);
    };
    double *t = table.data(), *st = state.data();
    const double *yy = y.data(), *c = cov.data();
    const int64_t bad_shape[2] = {3, 7};
    EXPECT(dep(nullptr, 2, g.shape, nullptr, yy, 2, c, 3, W, 1.2, INFINITY, st, 0) == MOLANN_E_NULL);
    EXPECT(dep(t, 2, g.shape, nullptr, yy, 2, nullptr, 3, W, 1.2, INFINITY, st, 0) == MOLANN_E_NULL);
    EXPECT(dep(t, 2, nullptr, nullptr, yy, 2, c, 3, W, 1.2, INFINITY, st, 0) == MOLANN_E_NULL);
    EXPECT(dep(t, 9, g.shape, nullptr, yy, 2, odd, 3, W, NAN, INFINITY, st, 0) == MOLANN_E_ALIGNMENT);
    EXPECT(dep(t, 9, g.shape, nullptr, yy, 2, c, 3, W, NAN, INFINITY, st, 0) == MOLANN_E_UNSUPPORTED);
    EXPECT(dep(t, 0, g.shape, nullptr, yy, 2, c, 3, W, 1.2, INFINITY, st, 0) == MOLANN_E_UNSUPPORTED);
    EXPECT(dep(t, 2, bad_shape, nullptr, yy, 2, c, 3, W, 1.2, INFINITY, st, 0) == MOLANN_E_DESC);
    EXPECT(dep(t, 2, g.shape, nullptr, yy, 2, c, 3, W, NAN, INFINITY, st, 0) == MOLANN_E_DESC);
    EXPECT(dep(t, 2, g.shape, nullptr, yy, 2, c, 3, W, 1.2, 0.0, st, 0) == MOLANN_E_DESC);
    EXPECT(dep(t, 2, g.shape, nullptr, yy, 2, c, 3, W, 1.2, NAN, st, 0) == MOLANN_E_DESC);
    EXPECT(dep(t, 2, g.shape, nullptr, yy, -2, c, 3, W, 1.2, INFINITY, st, 0) == MOLANN_E_DESC);
    EXPECT(dep(t, 2, g.shape, nullptr, yy, 1, c, 3, W, 1.2, INFINITY, st, 0) == MOLANN_E_DESC);
    EXPECT(dep(t, 2, g.shape, far, yy, 2, c, 3, W, 1.2, INFINITY, st, 0) == MOLANN_E_DESC);
    EXPECT(dep(t, 2, g.shape, nullptr, yy, 2, c, 2, W, 1.2, INFINITY, st, 0) == MOLANN_E_DESC);        // rows of cov would overlap
    EXPECT(dep(t, 2, g.shape, nullptr, yy, 2, c, -3, W, 1.2, INFINITY, st, 0) == MOLANN_E_DESC);
    EXPECT(dep(t, 2, g.shape, nullptr, yy, 2, c, 3, -1, 1.2, INFINITY, st, 0) == MOLANN_E_DESC);
    EXPECT(dep(t, 2, g.shape, nullptr, yy, 2, c, 3, W, 1.2, INFINITY, st, -1) == MOLANN_E_DESC);
    EXPECT(dep(nullptr, 2, nullptr, nullptr, nullptr, 2, nullptr, 3, 0, 1.2, INFINITY, nullptr, 0) == MOLANN_OK);
    for (double v : table) EXPECT(v == 0.0);
    for (double v : state) EXPECT(v == 0.0);
    EXPECT(dep(t, 2, g.shape, nullptr, yy, 2, c, 0, W, 1.2, INFINITY, st, 0) == MOLANN_OK && state[0] == 3.0);      // stride 0: one matrix for all

    auto wid = [&](int32_t d, const double* sg, const double* lo, const double* hi, const int32_t* columns, const double* yy2, int64_t ys, const double* m,
                   int64_t ms, int64_t ld, int64_t n, int32_t mode, int64_t window, int32_t emit, double* ad, double* as, double* o, int64_t cs) {
        return molann_selftest_metad_widths_f64(d, g.shape, g.lower, g.spacing, g.periodic, sg, lo, hi, columns, yy2, ys, m, ms, ld, n, mode, window, emit, ad, as,
                                                o, cs);
    };
    double *ad = adapt.data(), *as = astate.data(), *o = out.data();
    const double* m = metric.data();
    EXPECT(wid(2, sigma, nullptr, nullptr, nullptr, yy, 2, nullptr, 0, 0, W, 1, 5, 1, ad, nullptr, o, 3) == MOLANN_E_NULL);
    EXPECT(wid(2, sigma, nullptr, nullptr, nullptr, nullptr, 2, nullptr, 0, 0, W, 1, 5, 1, ad, as, o, 3) == MOLANN_E_NULL);
    EXPECT(wid(2, sigma, nullptr, nullptr, nullptr, yy, 2, nullptr, 0, 0, W, 1, 5, 1, nullptr, as, o, 3) == MOLANN_E_NULL);
    EXPECT(wid(2, sigma, nullptr, nullptr, nullptr, yy, 2, nullptr, 0, 0, W, 1, 5, 1, ad, as, nullptr, 3) == MOLANN_E_NULL);
    EXPECT(wid(2, sigma, nullptr, nullptr, nullptr, nullptr, 0, nullptr, 4, 2, W, 2, 0, 1, nullptr, as, o, 3) == MOLANN_E_NULL);
    EXPECT(wid(2, nullptr, nullptr, nullptr, nullptr, yy, 2, nullptr, 0, 0, W, 1, 5, 1, ad, as, o, 3) == MOLANN_E_NULL);
    EXPECT(wid(9, sigma, nullptr, nullptr, nullptr, yy, 2, nullptr, 0, 0, W, 7, 0, 1, ad, as, (double*)((char*)o + 4), 3) == MOLANN_E_ALIGNMENT);
    EXPECT(wid(9, sigma, nullptr, nullptr, nullptr, yy, 2, nullptr, 0, 0, W, 7, 0, 1, ad, as, o, 3) == MOLANN_E_UNSUPPORTED);
    EXPECT(wid(2, sigma, nullptr, nullptr, nullptr, yy, 2, nullptr, 0, 0, W, 7, 5, 1, ad, as, o, 3) == MOLANN_E_DESC);
    EXPECT(wid(2, bad_sigma, nullptr, nullptr, nullptr, yy, 2, nullptr, 0, 0, W, 1, 5, 1, ad, as, o, 3) == MOLANN_E_DESC);
    EXPECT(wid(2, sigma, neg, nullptr, nullptr, yy, 2, nullptr, 0, 0, W, 1, 5, 1, ad, as, o, 3) == MOLANN_E_DESC);
    EXPECT(wid(2, sigma, big, small, nullptr, yy, 2, nullptr, 0, 0, W, 1, 5, 1, ad, as, o, 3) == MOLANN_E_DESC);
    EXPECT(wid(2, sigma, nullptr, nullptr, nullptr, yy, 2, nullptr, 0, 0, W, 1, 0, 1, ad, as, o, 3) == MOLANN_E_DESC);
    EXPECT(wid(2, sigma, nullptr, nullptr, nullptr, yy, 1, nullptr, 0, 0, W, 1, 5, 1, ad, as, o, 3) == MOLANN_E_DESC);
    EXPECT(wid(2, sigma, nullptr, nullptr, far, yy, 2, nullptr, 0, 0, W, 1, 5, 1, ad, as, o, 3) == MOLANN_E_DESC);
    EXPECT(wid(2, sigma, nullptr, nullptr, nullptr, yy, 2, nullptr, 0, 0, W, 1, 5, 1, ad, as, o, 2) == MOLANN_E_DESC);       // rows of cov_out would overlap
    EXPECT(wid(2, sigma, nullptr, nullptr, nullptr, yy, 2, nullptr, 0, 0, W, 1, 5, 1, ad, as, o, 0) == MOLANN_E_DESC);
    EXPECT(wid(2, sigma, nullptr, nullptr, nullptr, nullptr, 0, m, 3, 2, W, 2, 0, 1, nullptr, as, o, 3) == MOLANN_E_DESC);   // a walker's metric is 2 x 2
    EXPECT(wid(2, sigma, nullptr, nullptr, far, nullptr, 0, m, 4, 2, W, 2, 0, 1, nullptr, as, o, 3) == MOLANN_E_DESC);
    EXPECT(wid(2, sigma, nullptr, nullptr, nullptr, yy, 2, nullptr, 0, 0, -1, 1, 5, 1, ad, as, o, 3) == MOLANN_E_DESC);
    EXPECT(wid(2, nullptr, nullptr, nullptr, nullptr, nullptr, 2, nullptr, 0, 0, 0, 1, 5, 1, nullptr, nullptr, nullptr, 3) == MOLANN_OK);
    for (double v : adapt) EXPECT(v == 0.0);
    for (double v : astate) EXPECT(v == 0.0);
    for (double v : out) EXPECT(v == 0.0);
    EXPECT(wid(2, sigma, nullptr, nullptr, nullptr, nullptr, 0, m, 4, 2, W, 2, 0, 1, nullptr, as, o, 3) == MOLANN_OK && astate[1] == 1.0);
    EXPECT(wid(2, sigma, small, big, nullptr, yy, 2, nullptr, 0, 0, W, 1, 5, 0, ad, as, nullptr, 0) == MOLANN_OK && astate[0] == 3.0);
}

int main() {
    uint64_t seed = 5;
    int deposits = 0, walks = 0;
    for (const Grid& g : GRIDS) {
        for (int64_t W : {(int64_t)1, (int64_t)2, (int64_t)9, (int64_t)65})
            for (double cutoff : {(double)INFINITY, 3.3}) {
                one_deposit(g, W, cutoff, 0, 1, 0, 0, 0, ++seed);
                one_deposit(g, W, cutoff, 3, 3, 4, W > 2 ? W - 2 : 1, 0, ++seed);        // strided inputs, a log shorter than the step
                deposits += 2;
                for (int spoil = 1; spoil <= 8; ++spoil, ++deposits) one_deposit(g, W, cutoff, 2, 2, 1, 3, spoil, ++seed);
            }
        for (int64_t W : {(int64_t)1, (int64_t)3, (int64_t)257})
            for (int64_t window : {(int64_t)1, (int64_t)5, (int64_t)50})
                for (int limits = 0; limits < 2; ++limits, ++walks) one_widths(g, W, window, limits ? 2 : 0, limits ? 3 : 0, limits != 0, ++seed);
        std::printf("d %d shape %lld %lld %lld: %d deposits, %d walks so far\n", g.d, (long long)g.shape[0], (long long)g.shape[1], (long long)g.shape[2],
                    deposits, walks);
    }
    refusals();
    std::printf(failures ? "FAILED: %d\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
