// molann_dev_metad_rct_f64.inc - part of libmolann_hip.so, included by molann_kernels.hip after molann_dev_metad_deposit_f64.inc.  The
// reweighting offset c(t) of a metadynamics run (Tiwary-Parrinello; PLUMED's CALC_RCT / RCT_USTRIDE) from the device-resident table, so
// that a run's frames can be weighted by exp((V - c) / kT) without the table leaving the device: a deterministic reduction in two
// launches, a chain on the caller's stream (molann_metad_rct_f64 enqueues them).  No atomics, no ticket, no cooperative launch; the
// arithmetic and the order of every sum are molann_metad_rct.h's, which the host twin repeats.  Out of scope: a running acceleration
// factor; rbias written by the kernel; float32; a single-launch reduction.
namespace {

struct MetadRctArgs {
    const double* table;
    const double* state;          // MetadRun's [8], of which [3] = steps is read; null: update always
    double* partials;             // [chunks, 4] = (m_c, s0_c, sV_c, bad_c)
    double* rct;                  // [8] = (c, updates, M, a0 M + log S0, aV M + log SV, steps at the update, bad, 0)
    long n, chunks, stride;
    double kT, a0, aV;
};

// molann_metad_rct.h's TREE over the block's 256 values; every thread returns the result.  s_w: four doubles of LDS, free again on return.
template <class Op>
__device__ __forceinline__ double metad_rct_block_tree_f64(double x, double* s_w, Op op) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x = op(x, __shfl_down(x, off, 64));    // lane i < off: op(x_i, x_{i + off}); the others are not read again
    const int t = threadIdx.x;
    if ((t & 63) == 0) s_w[t >> 6] = x;
    __syncthreads();
    const double r = metad_rct_quad_f64(s_w[0], s_w[1], s_w[2], s_w[3], op);
    __syncthreads();
    return r;
}

// =============================================================================================
// metad_rct_partial_f64_kernel<<<min(chunks, METAD_RCT_MAX_BLOCKS), 256>>>: block b takes the chunks b, b + gridDim.x, ...; a chunk's row
// of partials depends on the chunk alone.  Per chunk a thread loads its 8 slots (entry 2048 c + 256 j + t: coalesced, each entry read
// once, a slot past n not read at all), and keeps them in registers through both passes: the chunk's maximum over the finite entries
// (thread, wave, four waves), then the two sums of exp(a (v - m_c)) in slot order and the tree.  Thread 0 stores the row.
// Off the stride (metad_rct_due_f64 on state[3], which the deposit queued before has incremented) every block returns at once.
// Bounds: g < n for every load; c < chunks <= the rows the host checked for every store.
// =============================================================================================
__global__ __launch_bounds__(256) void metad_rct_partial_f64_kernel(const MetadRctArgs a) {
    __shared__ double s_w[4];
    double steps;
    if (!metad_rct_due_f64(a.state, a.stride, steps)) return;
    const int t = threadIdx.x;
    for (long c = blockIdx.x; c < a.chunks; c += gridDim.x) {
        const long base = c * METAD_RCT_CHUNK + t;
        double v[METAD_RCT_SLOTS];
        bool live[METAD_RCT_SLOTS];
#pragma unroll
        for (int j = 0; j < METAD_RCT_SLOTS; ++j) {
            const long g = base + (long)j * METAD_RCT_THREADS;
            live[j] = g < a.n;
            v[j] = live[j] ? a.table[g] : 0.0;
        }
        int bad;
        const double tm = metad_rct_thread_max_f64(v, live, bad);
        const double m = metad_rct_block_tree_f64(tm, s_w, MetadRctMax());
        double s0, sV;
        metad_rct_thread_sums_f64(v, live, m, a.a0, a.aV, s0, sV);
        s0 = metad_rct_block_tree_f64(s0, s_w, MetadRctAdd());
        sV = metad_rct_block_tree_f64(sV, s_w, MetadRctAdd());
        const double nb = metad_rct_block_tree_f64((double)bad, s_w, MetadRctAdd());    // at most 2048: exact in any order
        if (t == 0) {
            double* p = a.partials + c * METAD_RCT_ROW;
            p[0] = m; p[1] = s0; p[2] = sV; p[3] = nb;
        }
    }
}

// =============================================================================================
// metad_rct_combine_f64_kernel<<<1, 256>>>: thread t walks the rows t, t + 256, ... twice, ascending: the table's maximum M, then the
// rows' sums moved to it, s_c exp(a (m_c - M)); both through the tree.  Thread 0 forms c and stores rct.  Off the stride it returns
// before reading a row, on the decision the partial launch took from the same state[3] (nothing in between writes it).
// =============================================================================================
__global__ __launch_bounds__(256) void metad_rct_combine_f64_kernel(const MetadRctArgs a) {
    __shared__ double s_w[4];
    double steps;
    if (!metad_rct_due_f64(a.state, a.stride, steps)) return;
    const int t = threadIdx.x;
    const double M = metad_rct_block_tree_f64(metad_rct_combine_max_f64(a.partials, a.chunks, t), s_w, MetadRctMax());
    double s0, sV, bad;
    metad_rct_combine_sums_f64(a.partials, a.chunks, t, M, a.a0, a.aV, s0, sV, bad);
    s0 = metad_rct_block_tree_f64(s0, s_w, MetadRctAdd());
    sV = metad_rct_block_tree_f64(sV, s_w, MetadRctAdd());
    bad = metad_rct_block_tree_f64(bad, s_w, MetadRctAdd());                             // below 2^31: exact in any order
    if (t == 0) metad_rct_final_f64(M, s0, sV, bad, a.kT, a.a0, a.aV, steps, a.rct);
}

} // namespace
