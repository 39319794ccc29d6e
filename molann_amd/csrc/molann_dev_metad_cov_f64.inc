// molann_dev_metad_cov_f64.inc - part of libmolann_hip.so, included by molann_kernels.hip after molann_dev_metad_rct_f64.inc.  Metadynamics
// hills with a full covariance matrix (adaptive Gaussians; the arithmetic and its proofs: molann_metad_cov.h): metad_widths_f64_kernel keeps
// every walker's running mean and covariance on the device (DIFF) or forms the covariance from the metric the caller passes (GEOM) and
// writes the step's covariances out; metad_deposit_cov_f64_kernel adds the step's correlated hills to the device-resident table
// (molann_metad_widths_f64 and molann_metad_deposit_cov_f64 launch them).  Out of scope: a frame kernel that fuses the bias with the metric;
// heights renormalised by the determinant; float32; tables of more than GRID_MAX_D axes.
namespace {

struct MetadWidthsArgs {
    double* adapt;                // [n_walkers, 1 + d + T] rows (n_a, mean, cov), DIFF; null for GEOM
    double* adapt_state;          // [8] = (observations, emits, skipped, 0...)
    double* cov_out;              // walker a's hill covariance: cov_out[a cov_stride + ...]; read only when emit
    const double* y;              // DIFF: y[a y_stride + col[k]]
    const double* metric;         // GEOM: metric[a metric_stride + col[i] metric_ld + col[j]]
    double lower[GRID_MAX_D];
    double P[GRID_MAX_D];
    double sigma[GRID_MAX_D], sigma_min[GRID_MAX_D], sigma_max[GRID_MAX_D];
    int col[GRID_MAX_D];
    long y_stride, metric_stride, metric_ld, cov_stride, n_walkers;
    double window, decay;
    int d, mode, emit;
};

// One walker's step of the widths call, one copy for the kernel's thread and the host twin's loop: 1 where a DIFF observation was skipped.
MOLANN_HD int metad_widths_walker_f64(const MetadWidthsArgs& a, long w) {
    double C[METAD_COV_MAX_T];
    int skipped = 0;
    if (a.mode == METAD_COV_DIFF) {
        double y[GRID_MAX_D] = {0., 0., 0.};
#pragma unroll
        for (int k = 0; k < GRID_MAX_D; ++k)
            if (k < a.d) y[k] = a.y[w * a.y_stride + a.col[k]];
        double* row = a.adapt + w * metad_cov_row(a.d);
        skipped = metad_cov_observe_f64(row, y, a.lower, a.P, a.d, a.decay) ? 0 : 1;
        if (!a.emit) return skipped;
        metad_cov_hill_diff_f64(row, a.sigma, a.d, a.window, C);
    } else {
        if (!a.emit) return 0;
        metad_cov_hill_geom_f64(a.metric + w * a.metric_stride, a.metric_ld, a.col, a.sigma, a.d, C);
    }
    metad_cov_limits_f64(C, a.sigma_min, a.sigma_max, a.d);
    metad_cov_store_f64(C, a.d, a.cov_out + w * a.cov_stride);
    return skipped;
}

// (observations, emits, skipped): counts in doubles, by one thread
MOLANN_HD void metad_widths_state_f64(const MetadWidthsArgs& a, long skipped) {
    if (a.mode == METAD_COV_DIFF) {
        a.adapt_state[0] = a.adapt_state[0] + (double)(a.n_walkers - skipped);
        a.adapt_state[2] = a.adapt_state[2] + (double)skipped;
    }
    if (a.emit) a.adapt_state[1] = a.adapt_state[1] + 1.0;
}

// =============================================================================================
// metad_widths_f64_kernel: one block, thread t takes the walkers t, t + 256, ...  A walker's row of adapt is read and written by that one
// thread, and nobody else reads it: the deposit takes the covariances from cov_out, which this launch writes and that one only reads, so
// no block of a deposit races this writer.  Thread 0 adds the step's counts to adapt_state.  Bounds: walkers to n_walkers.
// =============================================================================================
__global__ __launch_bounds__(256) void metad_widths_f64_kernel(const MetadWidthsArgs a) {
    long skipped = 0;
    for (long base = 0; base < a.n_walkers; base += 256) {
        const long w = base + threadIdx.x;
        const int s = w < a.n_walkers ? metad_widths_walker_f64(a, w) : 0;
        skipped += __syncthreads_count(s);
    }
    if (threadIdx.x == 0) metad_widths_state_f64(a, skipped);
}

struct MetadDepositCovArgs {
    double* table;
    double* state;                // [8] = (hills, refused, sum_heights, steps, logged, 0, 0, 0), as metad_deposit_f64_kernel's
    double* log;                  // [log_capacity, d + T + 1] or null
    const double* y;              // walker a's centre: y[a y_stride + col[k]]
    const double* V;              // walker a's bias: V[a v_stride]
    const double* cov;            // walker a's covariance, d's upper triangle: cov[a cov_stride + ...]
    long n[GRID_MAX_D];
    double lower[GRID_MAX_D];
    double h[GRID_MAX_D];
    double P[GRID_MAX_D];
    int col[GRID_MAX_D];
    long y_stride, v_stride, cov_stride, n_walkers, log_capacity;
    double height0, inv_dT, c2;
};

// =============================================================================================
// metad_deposit_cov_f64_kernel<D>: metad_deposit_f64_kernel's gather for hills that are not a product over the axes.  The same tiles
// (256; 16 x 16; 4 x 4 x 16), one thread per entry, the walkers through LDS metad_chunk(D) at a time, additions in walker order with no
// atomics, block 0's thread 0 the keeper of state and the log.  What differs:
//   A. thread j < chunk also loads walker j's covariance and factors it (metad_cov_factor_f64): a walker is valid when V, y and the height
//      are and the matrix is usable; any other is refused, changes no entry and is counted in state[1].  The reach test is per axis and
//      not summed (metad_cov_reach_f64, REACH in molann_metad_cov.h).  Height, centre, L and both flags go to LDS.
//   B. per reaching hill and per axis index of the tile one thread forms the wrapped delta_k (metad_axis_delta_f64) into LDS.
//   C. a thread reads its three deltas and the hill's L (broadcast), forms q by the forward substitution and, where q <= c2, adds
//      h exp(-(0.5 q)): one exp per entry and reaching hill, where the separable kernel has sum_k extent_k per hill and tile.
// Static LDS: 17 344 bytes (D = 1), 22 272 (D = 2), 18 176 (D = 3), well under the 64 KB default.  The keeper re-reads a walker's covariance
// from global memory for the log's row - the bits phase A loaded, since nobody writes cov during the launch.  Bounds: a tile's indices
// are clipped to the table's shape, the log's row to [0, log_capacity), walkers to n_walkers.  Every array of the arguments is indexed
// by constants (unrolled), so nothing goes to scratch: 76, 99 and 111 VGPRs for D = 1, 2, 3, no spill (78 for metad_widths_f64_kernel).
// =============================================================================================
template <int D>
__global__ __launch_bounds__(256) void metad_deposit_cov_f64_kernel(const MetadDepositCovArgs a) {
    constexpr int CH = metad_chunk(D), TS = metad_tile_slots(D);
    static_assert(CH <= METAD_TILE && METAD_TILE == 256, "thread j of the block stages walker j of a chunk");
    __shared__ double s_d[CH * TS], s_h[CH], s_y[CH][GRID_MAX_D], s_L[CH][METAD_COV_MAX_T];
    __shared__ int s_valid[CH], s_reach[CH];
    const int t = threadIdx.x;

    long i0[GRID_MAX_D] = {0, 0, 0}, i1[GRID_MAX_D] = {0, 0, 0}, idx[GRID_MAX_D] = {0, 0, 0};
    int loc[GRID_MAX_D] = {0, 0, 0};
    {
        unsigned b = blockIdx.x;    // fewer than 2^31 tiles: the host checks the table's size
        int r = t;
#pragma unroll
        for (int k = D - 1; k >= 0; --k) {
            const int T = metad_tile_extent(D, k);
            const unsigned tiles = (unsigned)((a.n[k] + T - 1) / T);
            const unsigned tk = b % tiles;
            b /= tiles;
            i0[k] = (long)tk * T;
            i1[k] = i0[k] + T - 1 < a.n[k] - 1 ? i0[k] + T - 1 : a.n[k] - 1;
            loc[k] = r % T;
            r /= T;
            idx[k] = i0[k] + loc[k];
        }
    }
    bool inside = true;
    long off = 0;
#pragma unroll
    for (int k = 0; k < D; ++k) {
        inside = inside && idx[k] <= i1[k];
        off = off * a.n[k] + idx[k];
    }
    int slot[GRID_MAX_D] = {0, 0, 0};
    {
        int base = 0;
#pragma unroll
        for (int k = 0; k < D; ++k) { slot[k] = base + loc[k]; base += metad_tile_extent(D, k); }
    }

    const bool keeper = blockIdx.x == 0 && t == 0;
    double hills = 0., refused = 0., sum_heights = 0.;
    long logged = 0;
    if (keeper) {
        hills = a.state[0]; refused = a.state[1]; sum_heights = a.state[2];
        logged = a.log ? opes_live_count_f64(a.state[4], a.log_capacity) : a.log_capacity;
    }

    double acc = 0.;
    bool loaded = false, touched = false;
    for (long base = 0; base < a.n_walkers; base += CH) {
        const int count = a.n_walkers - base < CH ? (int)(a.n_walkers - base) : CH;
        // A: the chunk's walkers
        int reach = 0;
        if (t < count) {
            const long w = base + t;
            const double V = a.V[w * a.v_stride];
            double y[GRID_MAX_D] = {0., 0., 0.};
#pragma unroll
            for (int k = 0; k < D; ++k) y[k] = a.y[w * a.y_stride + a.col[k]];
            double C[METAD_COV_MAX_T], L[METAD_COV_MAX_T];
            metad_cov_load_f64(a.cov + w * a.cov_stride, D, C);
            const bool usable = metad_cov_factor_f64(C, D, L);
            const double h = metad_height_f64(a.height0, V, a.inv_dT);
            const bool valid = metad_walker_valid_f64(V, y, h, D) && usable;
            reach = valid && metad_cov_reach_f64(i0, i1, y, a.lower, a.h, a.P, C, D, a.c2) ? 1 : 0;
            s_h[t] = h;
#pragma unroll
            for (int k = 0; k < D; ++k) s_y[t][k] = y[k];
#pragma unroll
            for (int k = 0; k < METAD_COV_MAX_T; ++k) s_L[t][k] = L[k];
            s_valid[t] = valid ? 1 : 0;
            s_reach[t] = reach;
        }
        const int any = __syncthreads_or(reach);
        if (blockIdx.x == 0) {
            if (keeper)
                for (int j = 0; j < count; ++j) {
                    double y[GRID_MAX_D] = {0., 0., 0.};
#pragma unroll
                    for (int k = 0; k < D; ++k) y[k] = s_y[j][k];
                    double C[METAD_COV_MAX_T];
                    metad_cov_load_f64(a.cov + (base + j) * a.cov_stride, D, C);
                    metad_cov_state_walker_f64(s_valid[j] != 0, s_h[j], y, C, D, a.log, a.log_capacity, hills, refused, sum_heights, logged);
                }
            if (!any) __syncthreads();    // the keeper has read the rows the next chunk overwrites
        }
        if (!any) continue;
        // B: the reaching hills' wrapped deltas along each axis of the tile
        for (int s = t; s < count * TS; s += METAD_TILE) {
            const int j = s / TS, r = s - j * TS;
            if (!s_reach[j]) continue;
            int lo = 0;
#pragma unroll
            for (int k = 0; k < D; ++k) {
                const int T = metad_tile_extent(D, k);
                if (r >= lo && r < lo + T && i0[k] + (r - lo) <= i1[k])
                    s_d[s] = metad_axis_delta_f64(i0[k] + (r - lo), s_y[j][k], a.lower[k], a.h[k], a.P[k]);
                lo += T;
            }
        }
        __syncthreads();
        // C: this thread's entry
        if (inside) {
            if (!loaded) { acc = a.table[off]; loaded = true; }
            for (int j = 0; j < count; ++j) {
                if (!s_reach[j]) continue;
                double delta[GRID_MAX_D] = {0., 0., 0.}, L[METAD_COV_MAX_T];
#pragma unroll
                for (int k = 0; k < D; ++k) delta[k] = s_d[j * TS + slot[k]];
#pragma unroll
                for (int k = 0; k < METAD_COV_MAX_T; ++k) L[k] = s_L[j][k];
                const double q = metad_cov_q_f64(delta, L, D);
                if (q <= a.c2) {
                    acc = acc + metad_cov_term_f64(s_h[j], q);
                    touched = true;
                }
            }
        }
        __syncthreads();    // the chunk's rows are free again
    }
    if (touched) a.table[off] = acc;
    if (keeper) {
        a.state[0] = hills; a.state[1] = refused; a.state[2] = sum_heights; a.state[3] = a.state[3] + 1.0;
        if (a.log) a.state[4] = (double)logged;
    }
}

} // namespace
