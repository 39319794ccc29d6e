// san_opes_adaptive.cpp - the host twin of the OPES step with adaptive widths and the explore variant,
// molann_selftest_opes_step_modes_f64, under AddressSanitizer and UndefinedBehaviorSanitizer in a stand-alone program: host code only,
// no GPU, nothing preloaded.  Every buffer is sized exactly (heap vectors), so a read or a write one element past a walker's row of
// adapt, past the chosen columns of y, past column 3 of the energies or past `capacity` rows is reported.  The call sequence is the
// host tests': observe, observe, deposit (skipped: 3 < 4), deposit (the first), then 30 times observe, deposit.  Build and run, from the
// repository root:
//
//   make -C molann_amd/csrc san
//   /opt/rocm/bin/hipcc -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       -Iinclude tools/san_opes_adaptive.cpp -Lmolann_amd/csrc -lmolann_hip_san -Wl,-rpath,$PWD/molann_amd/csrc -o tools/san_opes_adaptive
//   tools/san_opes_adaptive
//
// Prints one line per variant and "ok"; any other end is a finding.
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

enum { FIXED = 1, EXPLORE = 2, OBSERVE = 4 };

// one run of the sequence; strided: y is [W, 8] with columns (5, 2, ...) and V column 3 of [W, 4], both ending with the last element read
static void sequence(int d, int64_t W, bool strided, bool adaptive, int flags, bool with_min, uint64_t seed) {
    const int64_t capacity = 24, stride = 4;
    const int n_out = strided ? d + 6 : d, v_stride = strided ? 4 : 1;
    std::vector<int32_t> columns(d);
    for (int k = 0; k < d; ++k) columns[k] = strided ? (n_out - 1 - k) : k;       // descending: the first listed column is the row's last
    std::vector<double> centers(capacity * d, 0.0), sigma(capacity * d, 0.0), heights(capacity, 0.0), state(4, 0.0), run(8, 0.0), period(d, 0.0);
    std::vector<double> adapt(adaptive ? W * 3 * d : 0, 0.0), sigma0(d, 0.4), sigma_min(d, 0.03), pos(W * d);
    std::vector<double> y((W - 1) * n_out + (strided ? n_out : d)), V((W - 1) * v_stride + 1);
    period[0] = 2.0;
    for (double& v : pos) v = 0.8 + 0.1 * uniform(seed);
    int deposits = 0, observes = 0;
    for (int call = 0; call < 64; ++call) {
        const bool observe = call < 2 || (call >= 4 && call % 2 == 0);
        for (double& v : y) v = 1e300;                                              // what is not a chosen column is not looked at
        for (int64_t a = 0; a < W; ++a)
            for (int k = 0; k < d; ++k) {
                pos[a * d + k] += 0.16 * (uniform(seed) - 0.5) + (k == 0 ? 0.03 : 0.0);
                double v = pos[a * d + k];
                if (k == 0) v -= 2.0 * std::floor(v / 2.0 + 0.5);                   // wrapped into [-1, 1): the mean crosses the seam
                y[a * n_out + columns[k]] = v;
            }
        for (double& v : V) v = -3.0 * uniform(seed);
        if (call == 21) y[(W - 1) * n_out + columns[d - 1]] = std::nan("");
        if (call == 31) V[(W - 1) * v_stride] = INFINITY;
        if (observe && !adaptive) continue;
        const int code = molann_selftest_opes_step_modes_f64(centers.data(), sigma.data(), heights.data(), capacity, d, period.data(), state.data(),
                                                             run.data(), y.data(), n_out, strided ? columns.data() : nullptr,
                                                             observe ? y.data() : V.data(), observe ? 1 : v_stride, W, adaptive ? nullptr : sigma0.data(),
                                                             with_min ? sigma_min.data() : nullptr, adaptive ? adapt.data() : nullptr, 1.0, 10.0,
                                                             stride, 1.0, 5.0, flags | (observe ? OBSERVE : 0));
        EXPECT(code == MOLANN_OK);
        observes += observe ? 1 : 0;
        deposits += observe ? 0 : 1;
        if (adaptive) {
            EXPECT(run[6] == (double)(call + 1) && run[7] == (call >= 3 ? 1.0 : 0.0));
            if (call < 3) EXPECT(state[0] == 0.0 && state[1] == 0.0 && run[0] == 0.0);
        } else {
            EXPECT(run[6] == 0.0 && run[7] == 0.0);
        }
    }
    EXPECT(state[0] >= 1.0 && state[0] <= (double)capacity && std::isfinite(state[1]) && std::isfinite(run[3]) && std::isfinite(run[5]));
    EXPECT(run[0] == (double)((deposits - (adaptive ? 1 : 0)) * W - 2));          // the NaN output and the infinite bias refuse their walker alone
    for (double v : adapt) EXPECT(std::isfinite(v));
    // refusals write nothing
    std::vector<double> before = run;
    EXPECT(molann_selftest_opes_step_modes_f64(centers.data(), sigma.data(), heights.data(), capacity, d, period.data(), state.data(), run.data(), y.data(),
                                               n_out, nullptr, V.data(), v_stride, W, sigma0.data(), nullptr, nullptr, 1.0, 10.0, stride, 1.0, 5.0,
                                               OBSERVE) == MOLANN_E_DESC);
    EXPECT(molann_selftest_opes_step_modes_f64(centers.data(), sigma.data(), heights.data(), capacity, d, period.data(), state.data(), run.data(), y.data(),
                                               n_out, nullptr, V.data(), v_stride, W, sigma0.data(), nullptr, nullptr, 1.0, INFINITY, stride, 1.0, 5.0,
                                               EXPLORE) == MOLANN_E_DESC);
    if (adaptive)
        EXPECT(molann_selftest_opes_step_modes_f64(centers.data(), sigma.data(), heights.data(), capacity, d, period.data(), state.data(), run.data(),
                                                   y.data(), n_out, nullptr, V.data(), v_stride, W, nullptr, nullptr, adapt.data(), 1.0, 10.0, 1, 1.0, 5.0,
                                                   0) == MOLANN_E_DESC);
    EXPECT(before == run);
    std::printf("d %d W %d %s %s flags %d floor %d: n %.0f merges %.0f refused %.0f counter %.0f observations %.0f\n", d, (int)W,
                strided ? "strided" : "dense", adaptive ? "adaptive" : "given", flags, (int)with_min, state[0], state[2], state[3], run[0], run[6]);
}

int main() {
    uint64_t seed = 3;
    for (int d : {1, 2, 8})
        for (int64_t W : {(int64_t)1, (int64_t)3})
            for (int flags : {0, (int)FIXED, (int)EXPLORE, (int)(EXPLORE | FIXED)}) {
                sequence(d, W, d == 2, true, flags, flags != 0, ++seed);
                if (flags & EXPLORE) sequence(d, W, d != 2, false, flags, true, ++seed);     // the explore variant with given widths
            }
    sequence(2, 5, true, false, 0, true, ++seed);                                             // neither mode: the columns step's path
    std::printf(failures ? "FAILED: %d\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
