// san_opes_run_bias.cpp - the two host twins of an OPES run with walls and chosen outputs, molann_selftest_bias_opes_table_f64 and
// molann_selftest_opes_step_columns_f64, under AddressSanitizer and UndefinedBehaviorSanitizer in a stand-alone program: host code only,
// no GPU, nothing preloaded.  Every buffer is sized exactly (heap vectors), so a read or a write one element past a table row, past
// the chosen columns of y, past column 3 of the energies or past `capacity` rows is reported.  Build and run, from the repository root:
//
//   make -C molann_amd/csrc san
//   /opt/rocm/bin/hipcc -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       -Iinclude tools/san_opes_run_bias.cpp -Lmolann_amd/csrc -lmolann_hip_san -Wl,-rpath,$PWD/molann_amd/csrc -o tools/san_opes_run_bias
//   tools/san_opes_run_bias
//
// Prints one line per part and "ok"; any other end is a finding.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

static void bias_twin() {
    const int d_out = 8, width = 2;
    const int64_t capacity = 16;
    uint64_t seed = 7;
    std::vector<double> centers(capacity * width), sigma(capacity * width), heights(capacity), y(d_out), z(d_out), kappa(d_out), flat(d_out);
    std::vector<double> table(5 * 6), state(4), period(width, 0.0), energies(4), dy(d_out), energies2(4), dy2(d_out);
    for (double& v : centers) v = 2.0 * uniform(seed) - 1.0;
    for (double& v : sigma) v = 0.3 + uniform(seed);
    for (double& v : heights) v = 0.5 + uniform(seed);
    for (double& v : table) v = uniform(seed) - 0.5;
    for (int k = 0; k < d_out; ++k) { y[k] = 2.0 * uniform(seed) - 1.0; z[k] = 0.1 * k; kappa[k] = 1.0 + k; flat[k] = 0.2; }
    period[1] = 3.0;
    const int32_t columns[2] = {5, 2}, grid_columns[2] = {7, 0}, periodic[2] = {1, 0};
    const int64_t shape[2] = {5, 6};
    const double lower[2] = {-2.0, -2.0}, spacing[2] = {0.9, 0.8};
    molann_bias_terms_f64 t;
    std::memset(&t, 0, sizeof(t));
    t.center = z.data(); t.kappa = kappa.data(); t.flat = flat.data();
    t.n_grid_columns = 2; t.grid_columns = grid_columns; t.table = table.data(); t.shape = shape; t.lower = lower; t.spacing = spacing; t.periodic = periodic;
    molann_opes_table_term_f64 o;
    std::memset(&o, 0, sizeof(o));
    o.n_columns = width; o.columns = columns; o.centers = centers.data(); o.heights = heights.data(); o.sigma = sigma.data();
    o.capacity = capacity; o.state = state.data(); o.period = period.data(); o.scale = 0.9; o.epsilon = 1e-9; o.cutoff = 5.0;
    const double counts[] = {0.0, 1.0, 9.0, (double)capacity, capacity + 5.0, -1.0, std::nan("")};
    for (double count : counts) {
        state = {count, 12.5, 0.0, 0.0};
        EXPECT(molann_selftest_bias_opes_table_f64(y.data(), d_out, &t, &o, energies.data(), dy.data()) == MOLANN_OK);
        // the other twin, called with the n and the norm the state gives: the same doubles
        int64_t n = count >= 1.0 ? (int64_t)(count > capacity ? capacity : count) : 0;
        molann_opes_term_f64 by_value = {width, columns, centers.data(), heights.data(), n, sigma.data(), width, period.data(), 0.9,
                                         n ? 12.5 / (double)n : 1.0, 1e-9, 5.0};
        EXPECT(molann_selftest_bias_opes_f64(y.data(), d_out, &t, &by_value, energies2.data(), dy2.data()) == MOLANN_OK);
        EXPECT(std::memcmp(energies.data(), energies2.data(), 4 * sizeof(double)) == 0 && std::memcmp(dy.data(), dy2.data(), d_out * sizeof(double)) == 0);
        EXPECT(std::isfinite(energies[3]) && (n > 0 || energies[3] == 0.9 * std::log(1e-9)));
    }
    state = {3.0, 2.0, 0.0, 0.0};
    EXPECT(molann_selftest_bias_opes_table_f64(y.data(), d_out, nullptr, &o, energies.data(), dy.data()) == MOLANN_OK);     // no walls, no table
    o.columns = nullptr;                                                                                                     // identity columns
    EXPECT(molann_selftest_bias_opes_table_f64(y.data(), d_out, &t, &o, energies.data(), dy.data()) == MOLANN_OK);
    o.columns = columns;
    // refusals: nothing is read past what was checked
    o.capacity = 0;
    EXPECT(molann_selftest_bias_opes_table_f64(y.data(), d_out, &t, &o, energies.data(), dy.data()) == MOLANN_E_DESC);
    o.capacity = capacity; o.state = nullptr;
    EXPECT(molann_selftest_bias_opes_table_f64(y.data(), d_out, &t, &o, energies.data(), dy.data()) == MOLANN_E_NULL);
    o.state = state.data(); o.epsilon = 0.0;
    EXPECT(molann_selftest_bias_opes_table_f64(y.data(), d_out, &t, &o, energies.data(), dy.data()) == MOLANN_E_DESC);
    o.epsilon = 1e-9;
    const int32_t outside[2] = {5, 8};
    o.columns = outside;
    EXPECT(molann_selftest_bias_opes_table_f64(y.data(), d_out, &t, &o, energies.data(), dy.data()) == MOLANN_E_INDEX);
    o.columns = columns; t.n_hills_columns = 1;
    EXPECT(molann_selftest_bias_opes_table_f64(y.data(), d_out, &t, &o, energies.data(), dy.data()) == MOLANN_E_UNSUPPORTED);
    EXPECT(molann_selftest_bias_opes_table_f64(y.data(), d_out, &t, nullptr, energies.data(), dy.data()) == MOLANN_E_NULL);
    std::printf("bias twin: %d live counts, six refusals\n", (int)(sizeof(counts) / sizeof(counts[0])));
}

static void step_twin() {
    const int d = 2, n_out = 8, v_stride = 4;
    const int64_t capacity = 24, n_walkers = 20;
    uint64_t seed = 11;
    const int32_t columns[2] = {5, 2};
    for (int variant = 0; variant < 3; ++variant) {      // strided with columns; dense with identity columns; one walker
        const bool dense = variant == 1;
        const int64_t W = variant == 2 ? 1 : n_walkers, ys = dense ? d : n_out, vs = dense ? 1 : v_stride;
        std::vector<double> centers(capacity * d, 0.0), sigma(capacity * d, 0.0), heights(capacity, 0.0), state(4, 0.0), run(8, 0.0), period(d, 0.0);
        // the last walker's row ends with its last chosen column, its bias is the buffer's last element: nothing lies behind them
        std::vector<double> y(dense ? W * d : (W - 1) * n_out + 6), V(dense ? W : (W - 1) * v_stride + 1), sigma0(d, 0.3), sigma_min(d, 0.2);
        for (double& v : y) v = 4.0 * uniform(seed) - 2.0;
        for (double& v : V) v = -3.0 * uniform(seed);
        period[0] = 5.0;
        if (!dense && W > 3) { y[3 * n_out + 2] = std::nan(""); y[2 * n_out + 7] = std::nan(""); V[1 * v_stride] = INFINITY; }
        for (int step = 0; step < 3; ++step)           // the table fills: merges, appends, refusals at a full table
            EXPECT(molann_selftest_opes_step_columns_f64(centers.data(), sigma.data(), heights.data(), capacity, d, period.data(), state.data(), run.data(),
                                                         y.data(), ys, dense ? nullptr : columns, V.data(), vs, W, sigma0.data(), sigma_min.data(), 1.0, 1.0,
                                                         5.0, 0) == MOLANN_OK);
        EXPECT(state[0] >= 1.0 && state[0] <= (double)capacity && std::isfinite(state[1]) && std::isfinite(run[3]));
        EXPECT(run[0] + state[3] >= 3.0 * (variant == 0 ? W - 2 : W));
        if (variant == 0) EXPECT(run[0] == 3.0 * (W - 2));       // the NaN in a chosen column and the infinite bias refuse their walkers alone
        // refusals: a stride below d, a bias stride below 1, a column at y_stride, a repeated column - nothing enqueued, nothing written
        std::vector<double> before = state;
        const int32_t at_stride[2] = {5, (int32_t)ys}, twice[2] = {1, 1};
        EXPECT(molann_selftest_opes_step_columns_f64(centers.data(), sigma.data(), heights.data(), capacity, d, period.data(), state.data(), run.data(), y.data(),
                                                     1, nullptr, V.data(), vs, W, sigma0.data(), sigma_min.data(), 1.0, 1.0, 5.0, 0) == MOLANN_E_DESC);
        EXPECT(molann_selftest_opes_step_columns_f64(centers.data(), sigma.data(), heights.data(), capacity, d, period.data(), state.data(), run.data(), y.data(),
                                                     ys, nullptr, V.data(), 0, W, sigma0.data(), sigma_min.data(), 1.0, 1.0, 5.0, 0) == MOLANN_E_DESC);
        EXPECT(molann_selftest_opes_step_columns_f64(centers.data(), sigma.data(), heights.data(), capacity, d, period.data(), state.data(), run.data(), y.data(),
                                                     ys, at_stride, V.data(), vs, W, sigma0.data(), sigma_min.data(), 1.0, 1.0, 5.0, 0) == MOLANN_E_INDEX);
        EXPECT(molann_selftest_opes_step_columns_f64(centers.data(), sigma.data(), heights.data(), capacity, d, period.data(), state.data(), run.data(), y.data(),
                                                     ys, twice, V.data(), vs, W, sigma0.data(), sigma_min.data(), 1.0, 1.0, 5.0, 0) == MOLANN_E_INDEX);
        EXPECT(before == state);
        std::printf("step twin, variant %d: n %.0f merges %.0f refused %.0f counter %.0f\n", variant, state[0], state[2], state[3], run[0]);
    }
}

int main() {
    bias_twin();
    step_twin();
    std::printf(failures ? "FAILED: %d\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
