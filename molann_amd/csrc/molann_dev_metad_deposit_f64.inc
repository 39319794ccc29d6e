// molann_dev_metad_deposit_f64.inc - part of libmolann_hip.so, included by molann_kernels.hip after molann_dev_bias_opes_table_f64.inc.  The
// other half of a metadynamics run on a table, between the steps that molann_value_and_grid_f64 / molann_value_and_bias_f64 serve:
// metad_deposit_f64_kernel adds a step's hills to the device-resident table in place, with well-tempered heights formed from the bias
// those launches wrote (molann_metad_deposit_f64 launches it).  The reweighting offset c(t) is the next file's (molann_dev_metad_rct_f64.inc), queued after this
// launch.  Adaptive, correlated hills are molann_dev_metad_cov_f64.inc's.  Out of scope: float32; tables of more than GRID_MAX_D axes.
namespace {

struct MetadDepositArgs {
    double* table;
    double* state;                // [8] = (hills, refused, sum_heights, steps, logged, 0, 0, 0)
    double* log;                  // [log_capacity, 2 d + 1] or null
    const double* y;              // walker a's centre: y[a y_stride + col[k]]
    const double* V;              // walker a's bias: V[a v_stride]
    long n[GRID_MAX_D];           // the grid, as GridF64Args
    double lower[GRID_MAX_D];
    double h[GRID_MAX_D];
    double P[GRID_MAX_D];         // n h where the axis is periodic, else 0
    double sigma[GRID_MAX_D];
    int col[GRID_MAX_D];
    long y_stride, v_stride, n_walkers, log_capacity;
    double height0, inv_dT, c2;   // c2 = cutoff^2, +inf for none
};

// =============================================================================================
// metad_deposit_f64_kernel<D>: a GATHER.  Block b owns tile b of the table (metad_tile_extent(D, k) points along axis k, row-major over
// the tiles as over the table) and thread t one entry of it, so every entry is written by one thread, there are no atomics and the
// order of an entry's additions is the walkers' order, ((t + c_1) + c_2) + ..., whatever the launch geometry.  The walkers are an
// unbounded count and go through LDS metad_chunk(D) at a time:
//   A. thread j < chunk reads walker j's V and y (in place, by their strides), forms its height (metad_height_f64) and validity, and -
//      with a finite cutoff - whether the hill reaches this tile (metad_axis_reach_f64 per axis, summed); height, centre and both
//      flags go to LDS.  Every block re-forms the heights from V, which nobody writes: the same bits in every block, no hand-off.
//      __syncthreads_or: a chunk that does not reach the tile costs nothing more, and a tile no hill reaches returns without
//      reading or writing the table - the usual case by far with one walker on a table of millions of entries.
//   B. the Gaussian is a product over the axes: for each reaching hill and each of the tile's sum_k extent_k axis indices one thread
//      forms q_k and e_k = exp(-q_k / 2) (metad_axis_factor_f64) into LDS - sum_k extent_k exponentials per hill, not prod_k.
//   C. a thread adds the chunk's hills to its entry in order: q = sum_k q_k (3 LDS reads, broadcast along the tile's other axes), the
//      term h prod_k e_k where q <= c2 (metad_term_f64).  The entry is loaded before the first chunk that reaches the tile and stored
//      at the end if a term was added; an entry past the cutoff of every hill keeps its bits.
// Block 0's thread 0 also walks each chunk's LDS rows in order (metad_state_walker_f64: counts, the sum of heights, the log's rows)
// and stores state at the end; no other block reads state, and the host needs nothing of it to enqueue the next step.
// Bounds: a tile's indices are clipped to the table's shape, the log's row to [0, log_capacity), walkers to n_walkers.  Every array of
// the arguments is indexed by constants (unrolled), so nothing goes to scratch.
// =============================================================================================
template <int D>
__global__ __launch_bounds__(256) void metad_deposit_f64_kernel(const MetadDepositArgs a) {
    constexpr int CH = metad_chunk(D), TS = metad_tile_slots(D);
    static_assert(CH <= METAD_TILE && METAD_TILE == 256, "thread j of the block stages walker j of a chunk");
    __shared__ double s_q[CH * TS], s_e[CH * TS], s_h[CH], s_y[CH][GRID_MAX_D];
    __shared__ int s_valid[CH], s_reach[CH];
    const int t = threadIdx.x;

    // this block's tile and this thread's entry
    long i0[GRID_MAX_D], i1[GRID_MAX_D], idx[GRID_MAX_D];
    int loc[GRID_MAX_D];
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
    // where this thread's axis factors sit in a hill's TS slots
    int slot[GRID_MAX_D];
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
            const double h = metad_height_f64(a.height0, V, a.inv_dT);
            const bool valid = metad_walker_valid_f64(V, y, h, D);
            double qk[GRID_MAX_D] = {0., 0., 0.};
#pragma unroll
            for (int k = 0; k < D; ++k) qk[k] = metad_axis_reach_f64(i0[k], i1[k], y[k], a.lower[k], a.h[k], a.P[k], a.sigma[k]);
            reach = valid && metad_q_f64(qk, D) <= a.c2 ? 1 : 0;
            s_h[t] = h;
#pragma unroll
            for (int k = 0; k < D; ++k) s_y[t][k] = y[k];
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
                    metad_state_walker_f64(s_valid[j] != 0, s_h[j], y, a.sigma, D, a.log, a.log_capacity, hills, refused, sum_heights, logged);
                }
            if (!any) __syncthreads();    // the keeper has read the rows the next chunk overwrites
        }
        if (!any) continue;
        // B: the reaching hills' factors along each axis of the tile
        for (int s = t; s < count * TS; s += METAD_TILE) {
            const int j = s / TS, r = s - j * TS;
            if (!s_reach[j]) continue;
            int lo = 0;
#pragma unroll
            for (int k = 0; k < D; ++k) {
                const int T = metad_tile_extent(D, k);
                if (r >= lo && r < lo + T && i0[k] + (r - lo) <= i1[k]) {
                    const double dk = metad_axis_delta_f64(i0[k] + (r - lo), s_y[j][k], a.lower[k], a.h[k], a.P[k]);
                    double q, e;
                    metad_axis_factor_f64(dk, a.sigma[k], q, e);
                    s_q[s] = q;
                    s_e[s] = e;
                }
                lo += T;
            }
        }
        __syncthreads();
        // C: this thread's entry
        if (inside) {
            if (!loaded) { acc = a.table[off]; loaded = true; }
            for (int j = 0; j < count; ++j) {
                if (!s_reach[j]) continue;
                double q[GRID_MAX_D] = {0., 0., 0.}, e[GRID_MAX_D] = {1., 1., 1.};
#pragma unroll
                for (int k = 0; k < D; ++k) { q[k] = s_q[j * TS + slot[k]]; e[k] = s_e[j * TS + slot[k]]; }
                if (metad_q_f64(q, D) <= a.c2) {
                    acc = acc + metad_term_f64(s_h[j], e, D);
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
