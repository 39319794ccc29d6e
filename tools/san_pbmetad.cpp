// san_pbmetad.cpp - the host twins of parallel-bias metadynamics, molann_selftest_pbmetad_f64 and molann_selftest_pbmetad_deposit_f64,
// under AddressSanitizer and UndefinedBehaviorSanitizer in a stand-alone program: host code only, no GPU, nothing preloaded.  Every
// buffer is sized exactly (heap vectors): the tables to their entries, y and V to their strides' last element, the energies to 2 + K, dy
// to d_out, the log to its capacity, so a read or a write past any of them is reported.  It runs a few hundred generated frames and
// deposits - every K, periodic and not, with and without a cutoff and walls, columns in reverse on a wider y, energies read in place, a
// log shorter than the step - and malformed ones: y and V that are not finite or huge, heights that overflow and underflow, and each
// refusal.  Build and run, from the repository root:
//
//   make -C molann_amd/csrc san
//   /opt/rocm/bin/hipcc -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       -Iinclude tools/san_pbmetad.cpp -Lmolann_amd/csrc -lmolann_hip_san -Wl,-rpath,$PWD/molann_amd/csrc -o tools/san_pbmetad
//   tools/san_pbmetad
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

static const int64_t SHAPE[8] = {4, 257, 1025, 5, 67, 513, 256, 300};
static const double KT = 2.494;

struct Axes {
    int32_t K;
    int64_t shape[8];
    double lower[8], spacing[8], sigma[8];
    int32_t periodic[8];
    int64_t entries() const {
        int64_t n = 0;
        for (int k = 0; k < K; ++k) n += shape[k];
        return n;
    }
};

static Axes axes(int K, int flip) {
    Axes a;
    a.K = K;
    for (int k = 0; k < 8; ++k) {
        a.shape[k] = SHAPE[(k + flip) % 8];
        a.lower[k] = -1.3 - 0.4 * k;
        a.spacing[k] = 0.37 + 0.11 * k;
        a.sigma[k] = 0.83 * a.spacing[k] * (1.0 + 0.27 * k);
        a.periodic[k] = (k + flip) % 2;
    }
    return a;
}

// the values a malformed input takes, by number
static double spoiled(int spoil) {
    switch (spoil) {
    case 1: return NAN;
    case 2: return INFINITY;
    case 3: return -INFINITY;
    case 4: return 1e308;
    case 5: return -1e308;
    default: return 5e-324;
    }
}

// frames on exactly sized buffers; `spoil` makes one chosen output of frame 1 malformed
static void frames(const Axes& a, int64_t d_out, bool walls, int spoil, uint64_t seed) {
    const int K = a.K;
    std::vector<int32_t> columns(K);
    for (int k = 0; k < K; ++k) columns[k] = (int32_t)(d_out - 1 - k);      // the last outputs, in reverse
    std::vector<double> table(a.entries()), center(d_out), kappa(d_out), flat(d_out);
    for (double& v : table) v = 10.0 * uniform(seed) - 5.0;
    for (int64_t k = 0; k < d_out; ++k) { center[k] = uniform(seed) - 0.5; kappa[k] = 3.0 * uniform(seed); flat[k] = 0.2 * uniform(seed); }
    molann_pbmetad_terms_f64 t = {};
    if (walls) { t.center = center.data(); t.kappa = kappa.data(); t.flat = flat.data(); }
    t.n_columns = K; t.columns = columns.data(); t.table = table.data();
    t.shape = a.shape; t.lower = a.lower; t.spacing = a.spacing; t.periodic = a.periodic; t.kT = KT;
    for (int f = 0; f < 6; ++f) {
        std::vector<double> y(d_out), energies(2 + K, -7.0), dy(d_out, -7.0);
        for (double& v : y) v = 6.0 * uniform(seed) - 3.0;
        for (int k = 0; k < K; ++k) y[columns[k]] = a.lower[k] + (1.8 * uniform(seed) - 0.4) * a.shape[k] * a.spacing[k];
        if (spoil && f == 1) y[columns[K / 2]] = spoiled(spoil);
        EXPECT(molann_selftest_pbmetad_f64(y.data(), (int)d_out, &t, energies.data(), dy.data()) == MOLANN_OK);
        const bool poisoned = spoil >= 1 && spoil <= 3 && f == 1;
        if (poisoned) EXPECT(std::isnan(energies[1]));
        if (f != 1 || spoil == 0 || spoil == 6) EXPECT(std::isfinite(energies[1]));      // a huge y may overflow the cell's index: NaN as well
        if (K == 1 && std::isfinite(energies[1])) EXPECT(energies[1] == energies[2]);
        if (!walls) EXPECT(energies[0] == 0.0);
    }
}

// one deposit with exactly sized, strided buffers; `spoil` makes walker 1's centre or bias malformed
static void one_deposit(const Axes& a, int64_t W, double cutoff, int64_t y_extra, int64_t v_extra, int64_t log_rows, int spoil, uint64_t seed) {
    const int K = a.K;
    const int64_t y_stride = K + y_extra, v_stride = K + v_extra;
    std::vector<int32_t> columns(K);
    for (int k = 0; k < K; ++k) columns[k] = (int32_t)(y_stride - 1 - k);
    std::vector<double> table(a.entries()), y((W - 1) * y_stride + y_stride), V((W - 1) * v_stride + K), state(8, 0.0), log(log_rows * 2 * K, -7.0);
    for (double& v : table) v = 10.0 * uniform(seed) - 5.0;
    for (double& v : y) v = 0.0;
    for (double& v : V) v = 0.0;
    for (int64_t w = 0; w < W; ++w)
        for (int k = 0; k < K; ++k) {
            y[w * y_stride + columns[k]] = a.lower[k] + (1.4 * uniform(seed) - 0.2) * a.shape[k] * a.spacing[k];
            V[w * v_stride + k] = 14.0 * uniform(seed) - 6.0;
        }
    int64_t bad = 0;
    if (spoil && W > 1) {
        bad = 1;
        switch (spoil) {
        case 1: y[1 * y_stride + columns[0]] = NAN; break;
        case 2: y[1 * y_stride + columns[K - 1]] = -INFINITY; break;
        case 3: V[1 * v_stride + K - 1] = NAN; break;
        case 4: V[1 * v_stride] = INFINITY; break;
        case 5: V[1 * v_stride] = -1e6; break;                                   // the height overflows
        case 6: V[1 * v_stride + K - 1] = 1e6; bad = 0; break;       // the height underflows to 0: a hill all the same
        default: y[1 * y_stride + columns[0]] = 1e300; bad = 0; break;           // a centre far away: finite, reaches nothing
        }
    }
    const std::vector<double> before = table;
    const int rc = molann_selftest_pbmetad_deposit_f64(table.data(), K, a.shape, a.lower, a.spacing, a.periodic, a.sigma, columns.data(), y.data(),
                                                       y_stride, V.data(), v_stride, W, 1.2, 1.0 / (KT * 9.0), KT, cutoff, state.data(),
                                                       log_rows ? log.data() : nullptr, log_rows);
    EXPECT(rc == MOLANN_OK);
    EXPECT(state[0] == (double)(W - bad) && state[1] == (double)bad && state[3] == 1.0);
    EXPECT(std::isfinite(state[2]) && state[2] >= 0.0);
    if (log_rows) EXPECT(state[4] == (double)(W - bad < log_rows ? W - bad : log_rows));
    for (double v : table) EXPECT(std::isfinite(v));
    if (W == 1 && bad == 0 && spoil == 0) {
        bool changed = false;
        for (size_t i = 0; i < table.size(); ++i) changed = changed || table[i] != before[i];
        EXPECT(changed);
    }
}

static void refusals() {
    const Axes a = axes(2, 0);
    std::vector<double> table(a.entries(), 0.0), y(6, 0.1), V(6, 0.0), state(8, 0.0), energies(4, -7.0), dy(3, -7.0);
    int32_t columns[2] = {2, 0};
    auto deposit = [&](int32_t K, const int64_t* shape, const double* sigma, const int32_t* cols, int64_t v_stride, double kT, double cutoff) {
        return molann_selftest_pbmetad_deposit_f64(table.data(), K, shape, a.lower, a.spacing, a.periodic, sigma, cols, y.data(), 3, V.data(), v_stride, 2,
                                                   1.2, 0.04, kT, cutoff, state.data(), nullptr, 0);
    };
    const int64_t small[2] = {4, 3};
    const double zero_sigma[2] = {0.3, 0.0};
    const int32_t twice[2] = {1, 1}, outside[2] = {3, 0};
    EXPECT(deposit(0, a.shape, a.sigma, columns, 3, KT, INFINITY) == MOLANN_E_UNSUPPORTED);
    EXPECT(deposit(9, a.shape, a.sigma, columns, 3, KT, INFINITY) == MOLANN_E_UNSUPPORTED);
    EXPECT(deposit(2, small, a.sigma, columns, 3, KT, INFINITY) == MOLANN_E_DESC);
    EXPECT(deposit(2, a.shape, zero_sigma, columns, 3, KT, INFINITY) == MOLANN_E_DESC);
    EXPECT(deposit(2, a.shape, a.sigma, columns, 3, 0.0, INFINITY) == MOLANN_E_DESC);
    EXPECT(deposit(2, a.shape, a.sigma, columns, 3, KT, NAN) == MOLANN_E_DESC);
    EXPECT(deposit(2, a.shape, a.sigma, columns, 1, KT, INFINITY) == MOLANN_E_DESC);
    EXPECT(deposit(2, a.shape, a.sigma, outside, 3, KT, INFINITY) == MOLANN_E_DESC);
    EXPECT(deposit(2, a.shape, a.sigma, twice, 3, KT, INFINITY) == MOLANN_E_INDEX);
    EXPECT(molann_selftest_pbmetad_deposit_f64(nullptr, 2, a.shape, a.lower, a.spacing, a.periodic, a.sigma, columns, y.data(), 3, V.data(), 3, 2, 1.2,
                                               0.04, KT, INFINITY, state.data(), nullptr, 0) == MOLANN_E_NULL);
    EXPECT(molann_selftest_pbmetad_deposit_f64(nullptr, 2, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 3, nullptr, 3, 0, 1.2, 0.04, KT,
                                               INFINITY, nullptr, nullptr, 0) == MOLANN_OK);
    for (double v : state) EXPECT(v == 0.0);
    for (double v : table) EXPECT(v == 0.0);
    molann_pbmetad_terms_f64 t = {};
    t.n_columns = 2; t.columns = columns; t.table = table.data(); t.shape = a.shape; t.lower = a.lower; t.spacing = a.spacing; t.kT = KT;
    EXPECT(molann_selftest_pbmetad_f64(y.data(), 3, &t, energies.data(), dy.data()) == MOLANN_OK);
    t.columns = outside;
    EXPECT(molann_selftest_pbmetad_f64(y.data(), 3, &t, energies.data(), dy.data()) == MOLANN_E_INDEX);
    t.columns = twice;
    EXPECT(molann_selftest_pbmetad_f64(y.data(), 3, &t, energies.data(), dy.data()) == MOLANN_E_INDEX);
    t.columns = columns; t.shape = small;
    EXPECT(molann_selftest_pbmetad_f64(y.data(), 3, &t, energies.data(), dy.data()) == MOLANN_E_DESC);
    t.shape = a.shape; t.kT = -1.0;
    EXPECT(molann_selftest_pbmetad_f64(y.data(), 3, &t, energies.data(), dy.data()) == MOLANN_E_DESC);
    t.kT = KT; t.n_columns = 9;
    EXPECT(molann_selftest_pbmetad_f64(y.data(), 3, &t, energies.data(), dy.data()) == MOLANN_E_UNSUPPORTED);
    t.n_columns = 2; t.table = nullptr;
    EXPECT(molann_selftest_pbmetad_f64(y.data(), 3, &t, energies.data(), dy.data()) == MOLANN_E_NULL);
    std::printf("refusals: done\n");
}

int main() {
    uint64_t seed = 12345;
    int n_frames = 0, n_deposits = 0;
    for (int K = 1; K <= 8; ++K)
        for (int flip = 0; flip < 2; ++flip)
            for (int walls = 0; walls < 2; ++walls)
                for (int spoil = 0; spoil <= 6; ++spoil) {
                    frames(axes(K, flip), K + (flip ? 2 : 0), walls != 0, spoil, seed += 7);
                    n_frames += 6;
                }
    std::printf("frames: %d\n", n_frames);
    const int64_t walkers[] = {1, 3, 8, 9, 64, 65, 257};
    for (int K = 1; K <= 8; ++K)
        for (int64_t W : walkers)
            for (int cut = 0; cut < 2; ++cut) {
                const int flip = (int)((K + W) % 2);
                one_deposit(axes(K, flip), W, cut ? 3.3 : INFINITY, flip ? 2 : 0, cut ? 3 : 0, (K + W) % 3 == 0 ? 0 : (W > 4 ? W - 3 : W + 2), 0, seed += 7);
                ++n_deposits;
            }
    for (int K = 1; K <= 8; K += 3)
        for (int spoil = 1; spoil <= 7; ++spoil)
            for (int64_t W : {2, 66}) {
                one_deposit(axes(K, 1), W, spoil % 2 ? 3.3 : INFINITY, 1, 2, W, spoil, seed += 7);
                ++n_deposits;
            }
    std::printf("deposits: %d\n", n_deposits);
    refusals();
    if (failures) {
        std::printf("%d failures\n", failures);
        return 1;
    }
    std::printf("ok\n");
    return 0;
}
