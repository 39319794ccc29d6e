// molann_dev_pbmetad_deposit_f64.inc - part of libmolann_hip.so, included by molann_kernels.hip after molann_dev_pbmetad_f64.inc.  The
// other half of a parallel-bias metadynamics run, between the steps that molann_value_and_pbmetad_f64 serves: pbmetad_deposit_f64_kernel
// adds a step's hills to the K device-resident 1-D tables in place, every height weighted by its axis' share of the soft minimum and formed
// from the V_k that launch wrote (molann_pbmetad_deposit_f64 launches it).  metad_deposit_f64_kernel is not touched: its metad_* functions
// are called.  Out of scope: c(t); adaptive widths; per-axis heights or bias factors; float32.
namespace {

struct PbmetadDepositArgs {
    double* table;                    // the K tables back to back
    double* state;                    // [8] = (hills, refused, sum_heights, steps, logged, 0, 0, 0)
    double* log;                      // [log_capacity, 2 K] or null
    const double* y;                  // walker a's centre on axis k: y[a y_stride + col[k]]
    const double* V;                  // walker a's bias on axis k: V[a v_stride + k]
    long n[PBMETAD_MAX_K];
    long off[PBMETAD_MAX_K];          // where table k starts
    double lower[PBMETAD_MAX_K];
    double h[PBMETAD_MAX_K];
    double P[PBMETAD_MAX_K];          // n h where the axis is periodic, else 0
    double sigma[PBMETAD_MAX_K];
    int col[PBMETAD_MAX_K];
    int K;
    long y_stride, v_stride, n_walkers, log_capacity;
    double height0, inv_dT, kT, c2;   // c2 = cutoff^2, +inf for none
};

// tiles of METAD_TILE entries along an axis of n points
__host__ __device__ inline long pbmetad_axis_tiles(long n) { return (n + METAD_TILE - 1) / METAD_TILE; }

// =============================================================================================
// pbmetad_deposit_f64_kernel: a GATHER over all K tables in one launch of sum_k ceil(n_k / 256) blocks.  A block finds its (axis, tile) by
// walking the at most 8 tile counts of its arguments; thread t owns entry 256 tile + t of that axis, so every entry is written by one
// thread, there are no atomics and an entry's additions come in walker order, ((t + c_1) + c_2) + ..., whatever the launch geometry.  The
// walkers go through LDS PBMETAD_CHUNK at a time:
//   A. thread j < chunk reads walker j's K biases and K centres in place, by their strides, and forms the K heights and the validity
//      (pbmetad_walker_heights_f64) and whether the hill of THIS block's axis reaches this tile (pbmetad_axis_reaches_f64).  Every block
//      re-forms the heights from V, which nobody writes: the same bits in every block, no hand-off.  __syncthreads_or: a tile that no
//      hill reaches is neither read nor written.
//   B. a thread adds the chunk's reaching hills to its entry in order (pbmetad_entry_add_f64: metad_deposit_f64_kernel<1>'s arithmetic
//      per entry).  The entry is loaded before the first chunk that reaches the tile and stored at the end if a term was added; an entry
//      past the cutoff of every hill keeps its bits.
// Block 0's thread 0 also walks each chunk's LDS rows in order (pbmetad_state_walker_f64) and stores state at the end.
// Bounds: an entry's index is below n of its axis, its offset below sum_k n_k; the log's row lies in [0, log_capacity); walkers below
// n_walkers.  Every array of the arguments is indexed by constants (unrolled), so nothing goes to scratch.
// =============================================================================================
__global__ __launch_bounds__(256) void pbmetad_deposit_f64_kernel(const PbmetadDepositArgs a) {
    constexpr int CH = PBMETAD_CHUNK;
    static_assert(CH <= METAD_TILE && METAD_TILE == 256, "thread j of the block stages walker j of a chunk");
    __shared__ double s_h[CH][PBMETAD_MAX_K], s_y[CH][PBMETAD_MAX_K];
    __shared__ int s_valid[CH], s_reach[CH];
    const int t = threadIdx.x;

    // this block's axis and tile: the first axis whose tiles the block index falls into
    int axis = 0;
    long tile = 0, n = 4, off = 0;
    double lower = 0., h = 1., P = 0., sigma = 1.;
    {
        long b = blockIdx.x;
        bool found = false;
#pragma unroll
        for (int k = 0; k < PBMETAD_MAX_K; ++k) {
            const long tiles = k < a.K ? pbmetad_axis_tiles(a.n[k]) : 0;
            if (!found && b < tiles) {
                found = true;
                axis = k; tile = b; n = a.n[k]; off = a.off[k]; lower = a.lower[k]; h = a.h[k]; P = a.P[k]; sigma = a.sigma[k];
            }
            b -= tiles;
        }
        if (!found) return;    // a block past the last tile (the host launches none)
    }
    const long i0 = tile * METAD_TILE;
    const long i1 = i0 + METAD_TILE - 1 < n - 1 ? i0 + METAD_TILE - 1 : n - 1;
    const long idx = i0 + t;
    const bool inside = idx <= i1;

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
            double V[PBMETAD_MAX_K], y[PBMETAD_MAX_K], hk[PBMETAD_MAX_K];
#pragma unroll
            for (int k = 0; k < PBMETAD_MAX_K; ++k) {
                V[k] = k < a.K ? a.V[w * a.v_stride + k] : 0.;
                y[k] = k < a.K ? a.y[w * a.y_stride + a.col[k]] : 0.;
            }
            const bool valid = pbmetad_walker_heights_f64(V, y, a.K, a.height0, a.inv_dT, a.kT, hk);
            double mh = 0., my = 0.;
#pragma unroll
            for (int k = 0; k < PBMETAD_MAX_K; ++k) {
                s_h[t][k] = hk[k];
                s_y[t][k] = y[k];
                if (k == axis) { mh = hk[k]; my = y[k]; }
            }
            reach = valid && pbmetad_axis_reaches_f64(mh, i0, i1, my, lower, h, P, sigma, a.c2) ? 1 : 0;
            s_valid[t] = valid ? 1 : 0;
            s_reach[t] = reach;
        }
        const int any = __syncthreads_or(reach);
        if (keeper)
            for (int j = 0; j < count; ++j) {
                double y[PBMETAD_MAX_K], hk[PBMETAD_MAX_K];
#pragma unroll
                for (int k = 0; k < PBMETAD_MAX_K; ++k) { y[k] = s_y[j][k]; hk[k] = s_h[j][k]; }
                pbmetad_state_walker_f64(s_valid[j] != 0, hk, y, a.K, a.log, a.log_capacity, hills, refused, sum_heights, logged);
            }
        // B: this thread's entry
        if (any && inside) {
            if (!loaded) { acc = a.table[off + idx]; loaded = true; }
            for (int j = 0; j < count; ++j) {
                if (!s_reach[j]) continue;
                if (pbmetad_entry_add_f64(idx, s_h[j][axis], s_y[j][axis], lower, h, P, sigma, a.c2, acc)) touched = true;
            }
        }
        __syncthreads();    // the chunk's rows are free again (the keeper has read them too)
    }
    if (touched) a.table[off + idx] = acc;
    if (keeper) {
        a.state[0] = hills; a.state[1] = refused; a.state[2] = sum_heights; a.state[3] = a.state[3] + 1.0;
        if (a.log) a.state[4] = (double)logged;
    }
}

} // namespace
