// san_metad_rct.cpp - the host twin of the metadynamics reweighting offset, molann_selftest_metad_rct_f64, under AddressSanitizer and
// UndefinedBehaviorSanitizer in a stand-alone program: host code only, no GPU, nothing preloaded.  Every buffer is sized exactly (heap
// vectors): the table to its n entries, partials to molann_metad_rct_chunks(n) rows of 4, rct and state to 8, so a read past a ragged last
// chunk or a row written past the chunks is reported.  It runs a ragged table, a one-entry table, tables around a chunk, entries that are
// not finite, the stride and each refusal.  Build and run, from the repository root:
//
//   make -C molann_amd/csrc san
//   /opt/rocm/bin/hipcc -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//       -Iinclude tools/san_metad_rct.cpp -Lmolann_amd/csrc -lmolann_hip_san -Wl,-rpath,$PWD/molann_amd/csrc -o tools/san_metad_rct
//   tools/san_metad_rct
//
// Prints one line per table and "ok"; any other end is a finding.
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

static const double KT = 2.494, INV_DT = 1.0 / (2.494 * 9.0);

// the offset in long double, whole table, no chunks
static double plain_offset(const std::vector<double>& v, double inv_dT) {
    long double M = v[0], s0 = 0, sV = 0;
    for (double x : v) M = x > M ? x : M;
    const long double a0 = 1.0L / KT + inv_dT, aV = inv_dT;
    for (double x : v) {
        s0 += std::exp(a0 * (x - M));
        sV += std::exp(aV * (x - M));
    }
    return (double)(M + KT * (std::log(s0) - std::log(sV)));
}

static void one_table(int64_t n, double inv_dT, uint64_t seed) {
    std::vector<double> table(n), rct(8, 0.0);
    for (double& v : table) v = 120.0 * uniform(seed) - 20.0;
    const int64_t rows = molann_metad_rct_chunks(n);
    EXPECT(rows == (n + 2047) / 2048);
    std::vector<double> partials(rows * 4, -1.0);
    EXPECT(molann_selftest_metad_rct_f64(table.data(), n, KT, inv_dT, nullptr, 1, partials.data(), rows, rct.data()) == MOLANN_OK);
    const double want = plain_offset(table, inv_dT);
    EXPECT(std::fabs(rct[0] - want) <= 1e-12 * (KT + std::fabs(rct[2])));
    EXPECT(rct[1] == 1.0 && rct[5] == 0.0 && rct[6] == 0.0 && rct[7] == 0.0);
    double count = 0.0;
    for (int64_t c = 0; c < rows; ++c) {
        EXPECT(partials[4 * c + 1] >= 1.0 && partials[4 * c + 2] >= 1.0 && partials[4 * c + 3] == 0.0);
        count += inv_dT == 0.0 ? partials[4 * c + 2] : 0.0;
    }
    EXPECT(inv_dT != 0.0 || count == (double)n);              // plain metadynamics: sV counts the entries, the ragged tail included

    // entries that are not finite, at both ends: counted, and nothing else read or written
    std::vector<double> holed = table;
    holed[0] = NAN;
    holed[n - 1] = n > 1 ? INFINITY : NAN;
    EXPECT(molann_selftest_metad_rct_f64(holed.data(), n, KT, inv_dT, nullptr, 1, partials.data(), rows, rct.data()) == MOLANN_OK);
    EXPECT(rct[6] == (n > 1 ? 2.0 : 1.0) && rct[1] == 2.0 && std::isnan(rct[0]) && std::isnan(rct[2]) && std::isnan(rct[3]) && std::isnan(rct[4]));

    // the stride: state[3] = 7 is off a stride of 3 and on a stride of 7
    std::vector<double> state = {3.0, 0.0, 1.0, 7.0, 0.0, 0.0, 0.0, 0.0}, before = rct, rows_before = partials;
    EXPECT(molann_selftest_metad_rct_f64(table.data(), n, KT, inv_dT, state.data(), 3, partials.data(), rows, rct.data()) == MOLANN_OK);
    EXPECT(rct[6] == before[6] && rct[1] == before[1] && partials == rows_before);
    EXPECT(molann_selftest_metad_rct_f64(table.data(), n, KT, inv_dT, state.data(), 7, partials.data(), rows, rct.data()) == MOLANN_OK);
    EXPECT(rct[1] == 3.0 && rct[5] == 7.0 && rct[6] == 0.0 && std::fabs(rct[0] - want) <= 1e-12 * (KT + std::fabs(rct[2])));
    for (double bits : {(double)NAN, -5.0, 1e300, (double)INFINITY}) {
        state[3] = bits;
        EXPECT(molann_selftest_metad_rct_f64(table.data(), n, KT, inv_dT, state.data(), 1, partials.data(), rows, rct.data()) == MOLANN_OK);
    }
    EXPECT(rct[1] == 7.0);

    // each refusal, in the entry's order; none writes
    before = rct;
    rows_before = partials;
    const double* t = table.data();
    double *p = partials.data(), *r = rct.data(), *s = state.data();
    const double* odd_t = (const double*)((const char*)t + 4);
    EXPECT(molann_selftest_metad_rct_f64(nullptr, n, KT, inv_dT, s, 1, p, rows, r) == MOLANN_E_NULL);
    EXPECT(molann_selftest_metad_rct_f64(t, n, KT, inv_dT, s, 1, nullptr, rows, r) == MOLANN_E_NULL);
    EXPECT(molann_selftest_metad_rct_f64(t, n, KT, inv_dT, s, 1, p, rows, nullptr) == MOLANN_E_NULL);
    EXPECT(molann_selftest_metad_rct_f64(odd_t, n, KT, inv_dT, s, 1, p, rows, r) == MOLANN_E_ALIGNMENT);
    EXPECT(molann_selftest_metad_rct_f64(t, n, KT, inv_dT, (const double*)((const char*)s + 4), 1, p, rows, r) == MOLANN_E_ALIGNMENT);
    EXPECT(molann_selftest_metad_rct_f64(t, n, KT, inv_dT, s, 1, (double*)((char*)p + 4), rows, r) == MOLANN_E_ALIGNMENT);
    EXPECT(molann_selftest_metad_rct_f64(t, n, KT, inv_dT, s, 1, p, rows, (double*)((char*)r + 4)) == MOLANN_E_ALIGNMENT);
    EXPECT(molann_selftest_metad_rct_f64(t, 0, KT, inv_dT, s, 1, p, rows, r) == MOLANN_E_DESC);
    EXPECT(molann_selftest_metad_rct_f64(t, (int64_t)1 << 31, KT, inv_dT, s, 1, p, rows, r) == MOLANN_E_DESC);
    EXPECT(molann_selftest_metad_rct_f64(t, n, 0.0, inv_dT, s, 1, p, rows, r) == MOLANN_E_DESC);
    EXPECT(molann_selftest_metad_rct_f64(t, n, NAN, inv_dT, s, 1, p, rows, r) == MOLANN_E_DESC);
    EXPECT(molann_selftest_metad_rct_f64(t, n, KT, -1.0, s, 1, p, rows, r) == MOLANN_E_DESC);
    EXPECT(molann_selftest_metad_rct_f64(t, n, KT, INFINITY, s, 1, p, rows, r) == MOLANN_E_DESC);
    EXPECT(molann_selftest_metad_rct_f64(t, n, KT, inv_dT, s, 0, p, rows, r) == MOLANN_E_DESC);
    EXPECT(molann_selftest_metad_rct_f64(t, n, KT, inv_dT, s, 1, p, rows - 1, r) == MOLANN_E_DESC);
    EXPECT(molann_selftest_metad_rct_f64(nullptr, 0, NAN, -1.0, (const double*)((const char*)s + 4), 0, p, 0, r) == MOLANN_E_NULL);
    EXPECT(molann_selftest_metad_rct_f64(odd_t, 0, NAN, -1.0, s, 0, p, 0, r) == MOLANN_E_ALIGNMENT);
    EXPECT(before == rct && rows_before == partials);
    std::printf("n %lld inv_dT %.4f: c %.15g (long double %.15g) max %.6g rows %lld\n", (long long)n, inv_dT, rct[0], want, rct[2], (long long)rows);
}

int main() {
    uint64_t seed = 5;
    for (int64_t n : {(int64_t)1, (int64_t)5, (int64_t)255, (int64_t)2047, (int64_t)2048, (int64_t)2049, (int64_t)4099, (int64_t)524289})
        for (double inv_dT : {INV_DT, 0.0}) one_table(n, inv_dT, ++seed);
    std::printf(failures ? "FAILED: %d\n" : "ok\n", failures);
    return failures ? 1 : 0;
}
