// molann_value_f64.inc - part of libmolann_hip.so, included by molann_kernels.hip after molann_hvp.inc.  The float64 calls that give the
// values and a derivative in one launch (see include/molann_hip.h): molann_value_and_vjp_f64 (forces, frames_value_vjp_f64_kernel of
// molann_dev_vjp_f64.inc), molann_value_and_jacobian_f64 (frames_value_jac_f64_kernel, molann_dev_jac_f64.inc),
// molann_value_and_metric_f64 (frames_value_metric_f64_kernel, molann_dev_metric_f64.inc), molann_value_and_restraint_f64
// (frames_value_restraint_f64_kernel, molann_dev_restraint_f64.inc), molann_value_and_hills_f64 (frames_value_hills_f64_kernel,
// molann_dev_hills_f64.inc), molann_value_and_grid_f64 (frames_value_grid_f64_kernel, molann_dev_grid_f64.inc),
// molann_value_and_bias_f64 (frames_value_bias_f64_kernel, molann_dev_bias_f64.inc), molann_value_and_opes_f64
// (frames_value_opes_f64_kernel, molann_dev_opes_f64.inc), molann_value_and_bias_opes_f64 (frames_value_bias_opes_f64_kernel,
// molann_dev_bias_opes_f64.inc), molann_value_and_opes_table_f64 (frames_value_opes_table_f64_kernel, molann_dev_opes_table_f64.inc) and
// molann_value_and_bias_opes_table_f64 (frames_value_bias_opes_table_f64_kernel, molann_dev_bias_opes_table_f64.inc).
// One argument front end, one launch and one dispatch over the lane group serve the eleven; an entry names its kernel, its pointers and
// its rows.
namespace {

constexpr size_t VJP64_LDS_DEFAULT = 65536;    // dynamic LDS a launch may ask for as it is
constexpr size_t VJP64_LDS_CU = 163840;        // the LDS of a gfx950 compute unit (one block of one wave may take all of it)
// the widest output the metric kernel's chunk pairs serve: d_out / JAC64_KC chunks, every pair of them a pass over the frame's atoms
constexpr int METRIC64_MAX_D_OUT = 64;
// the widest output the hills kernel serves: its cotangent sums are a register array of this size (hill_term_f64 of molann_math.h)
constexpr int HILLS64_MAX_D_OUT = HILLS_MAX_D;
// the widest output the grid kernel serves: the table has one axis per output (grid_axis_f64 of molann_math.h)
constexpr int GRID64_MAX_D_OUT = GRID_MAX_D;

enum F64Entry { F64_VJP, F64_JACOBIAN, F64_METRIC, F64_RESTRAINT, F64_HILLS, F64_GRID, F64_BIAS };

struct Vjp64Geom {
    int G, block;       // lanes per frame, threads per block
    size_t lds;         // dynamic LDS of a block, bytes
    bool ok;
};

// doubles of LDS per frame: the feature row, the hidden layers' pre-activations, two rows of the widest layer input
inline void vjp64_rows(const molann_plan* p, int& max_w, int& per_frame) {
    max_w = 0; per_frame = 0;
    if (p->n_layers <= 0) return;
    long z = 0;
    for (int l = 0; l < p->n_layers; ++l) {
        max_w = std::max(max_w, p->dims[l]);
        if (l > 0) z += p->dims[l];
    }
    const long total = (long)p->d_feat + z + 2l * max_w;
    per_frame = total > (1l << 28) ? (1 << 28) : (int)total;
}

// doubles of LDS per frame of the restraint: the forces' rows and the cotangent row of d_out, which it has with or without a head
inline void restraint64_rows(const molann_plan* p, int& max_w, int& per_frame) {
    vjp64_rows(p, max_w, per_frame);
    const long total = (long)per_frame + (p->n_layers > 0 ? p->dims[p->n_layers] : p->d_feat);
    per_frame = total > (1l << 28) ? (1 << 28) : (int)total;
}

// doubles of LDS per frame of the bias on chosen outputs: the restraint's rows and the selection row of BIAS_SEL, whatever terms a call has
inline void bias64_rows(const molann_plan* p, int& max_w, int& per_frame) {
    restraint64_rows(p, max_w, per_frame);
    const long total = (long)per_frame + BIAS_SEL;
    per_frame = total > (1l << 28) ? (1 << 28) : (int)total;
}

// doubles of LDS per frame of the Jacobian and the metric (whose accumulators of a chunk pair live in registers): with a head the
// feature row, the hidden layers' act'(z), two buffers of d_out rows of the widest layer input (the forward's two activation rows
// live in them first); with an alignment 12 per output (G_R and gsum, then G_H and cen)
inline void jac64_rows(const molann_plan* p, int& max_w, int& z_w, int& per_frame) {
    int vjp_rows;
    vjp64_rows(p, max_w, vjp_rows);
    const long d_out = p->n_layers > 0 ? p->dims[p->n_layers] : p->d_feat;
    long z = 0, total = 0;
    for (int l = 1; l < p->n_layers; ++l) z += p->dims[l];
    if (p->n_layers > 0) total = (long)p->d_feat + z + 2l * d_out * max_w;
    if (p->n_align > 0) total += 12l * d_out;
    z_w = (int)std::min(z, 1l << 28);
    per_frame = total > (1l << 28) ? (1 << 28) : (int)total;
}

// lanes per frame: the smallest group that covers the atoms, the items, the align atoms and the head's widest layer in one round
// (8/4/2 frames per wave), a whole wave from 33 on; fewer waves per block, then one wave per frame, where the rows ask for it
// (the rows are the entry's: the Jacobian sizes its own and steps down the same way)
inline Vjp64Geom vjp64_geometry_rows(const molann_plan* p, int max_w, int per_frame) {
    int work = std::max(std::max(p->n_inp, p->n_items), std::max(p->n_align, max_w));
    for (int l = 1; l <= p->n_layers; ++l) work = std::max(work, p->dims[l]);
    Vjp64Geom g;
    g.G = work <= 8 ? 8 : work <= 16 ? 16 : work <= 32 ? 32 : 64;
    const size_t bytes = (size_t)per_frame * sizeof(double);
    g.ok = p->n_items > 0 && bytes <= VJP64_LDS_CU;
    if ((size_t)(64 / g.G) * bytes > VJP64_LDS_DEFAULT) g.G = 64;
    int waves = 4;
    while (waves > 1 && (size_t)waves * (64 / g.G) * bytes > VJP64_LDS_DEFAULT) waves >>= 1;
    g.block = 64 * waves;
    g.lds = (size_t)(g.block / g.G) * bytes;
    return g;
}

// the kernel arguments' rows, by the struct that carries them
inline void f64_entry_rows(const molann_plan* p, VjpF64Args& a) { vjp64_rows(p, a.max_w, a.lds_per_frame); }
inline void f64_entry_rows(const molann_plan* p, JacF64Args& a) { jac64_rows(p, a.max_w, a.z_w, a.lds_per_frame); }
inline void f64_entry_rows(const molann_plan* p, RestraintF64Args& a) { restraint64_rows(p, a.max_w, a.lds_per_frame); }
inline void f64_entry_rows(const molann_plan* p, HillsF64Args& a) { restraint64_rows(p, a.max_w, a.lds_per_frame); }
inline void f64_entry_rows(const molann_plan* p, GridF64Args& a) { restraint64_rows(p, a.max_w, a.lds_per_frame); }
inline void f64_entry_rows(const molann_plan* p, BiasF64Args& a) { bias64_rows(p, a.max_w, a.lds_per_frame); }
inline void f64_entry_rows(const molann_plan* p, OpesF64Args& a) { restraint64_rows(p, a.max_w, a.lds_per_frame); }   // the hills' rows, geometry and cap: F64_HILLS
inline void f64_entry_rows(const molann_plan* p, BiasOpesF64Args& a) { bias64_rows(p, a.max_w, a.lds_per_frame); }   // the bias' rows and geometry: F64_BIAS
inline void f64_entry_rows(const molann_plan* p, BiasOpesTableF64Args& a) { bias64_rows(p, a.max_w, a.lds_per_frame); }   // as BiasOpesF64Args: F64_BIAS
inline void f64_entry_rows(const molann_plan* p, PbmetadF64Args& a) { bias64_rows(p, a.max_w, a.lds_per_frame); }   // the bias' rows and geometry: F64_BIAS
inline void f64_entry_rows(const molann_plan* p, OpesTableF64Args& a) { restraint64_rows(p, a.max_w, a.lds_per_frame); }   // as OpesF64Args: F64_HILLS

// geometry for this entry: the forces' rows, the restraint's (the hills' and the grid's too), the bias' or the Jacobian's, and the
// metric's, the hills' and the grid's caps on the outputs
inline Vjp64Geom f64_entry_geometry(const molann_plan* p, F64Entry entry) {
    int max_w, z_w, per_frame;
    if (entry == F64_VJP) vjp64_rows(p, max_w, per_frame);
    else if (entry == F64_RESTRAINT || entry == F64_HILLS || entry == F64_GRID) restraint64_rows(p, max_w, per_frame);
    else if (entry == F64_BIAS) bias64_rows(p, max_w, per_frame);
    else jac64_rows(p, max_w, z_w, per_frame);
    Vjp64Geom g = vjp64_geometry_rows(p, max_w, per_frame);
    const int d_out = p->n_layers > 0 ? p->dims[p->n_layers] : p->d_feat;
    if ((entry == F64_METRIC && d_out > METRIC64_MAX_D_OUT) || (entry == F64_HILLS && d_out > HILLS64_MAX_D_OUT) ||
        (entry == F64_GRID && d_out > GRID64_MAX_D_OUT))
        g.ok = false;
    return g;
}

template <class Args>
struct F64Call {    // what a launch takes besides the caller's pointers
    Vjp64Geom g;
    Args a;
    F64Mlp m;
};

// The argument front end of the entries, in this order: plan, n (MOLANN_OK at n == 0: the caller returns), the pointers that
// must be there (`required`), their and the `optional` ones' 8-byte alignment (a null optional pointer passes), items, the head's
// tensors layer by layer, geometry.  Nothing is dereferenced but W and b.
template <class Args>
int f64_entry_arguments(const molann_plan* p, F64Entry entry, int64_t n, std::initializer_list<const void*> required,
                        std::initializer_list<const void*> optional, const double* const* W, const double* const* b, F64Call<Args>& c) {
    if (!p) return MOLANN_E_NULL;
    if (n < 0) return MOLANN_E_DESC;
    if (n == 0) return MOLANN_OK;
    uintptr_t low_bits = 0;
    for (const void* ptr : optional) low_bits |= (uintptr_t)ptr;
    for (const void* ptr : required) {
        if (!ptr) return MOLANN_E_NULL;
        low_bits |= (uintptr_t)ptr;
    }
    if (low_bits & 7) return MOLANN_E_ALIGNMENT;
    if (p->n_items <= 0) return MOLANN_E_STAGE;
    F64Mlp& m = c.m;
    memset(&m, 0, sizeof(m));
    m.n_layers = p->n_layers; m.act = p->act;
    if (p->n_layers > 0) {
        if (!W || !b) return MOLANN_E_NULL;
        for (int i = 0; i <= p->n_layers; ++i) m.dims[i] = p->dims[i];
        for (int l = 0; l < p->n_layers; ++l) {
            if (!W[l] || !b[l]) return MOLANN_E_NULL;
            if ((((uintptr_t)W[l]) & 7) || (((uintptr_t)b[l]) & 7)) return MOLANN_E_ALIGNMENT;
            m.W[l] = W[l]; m.b[l] = b[l];
        }
    }
    c.g = f64_entry_geometry(p, entry);
    if (!c.g.ok) return MOLANN_E_UNSUPPORTED;
    Args& a = c.a;
    a.n_frames = (long)n;
    a.n_inp = p->n_inp; a.n_align = p->n_align; a.n_items = p->n_items; a.d_feat = p->d_feat;
    a.d_out = p->n_layers > 0 ? p->dims[p->n_layers] : p->d_feat;
    f64_entry_rows(p, a);
    m.max_w = a.max_w;
    return MOLANN_OK;
}

// The kernel's instance for a lane group (named in this order: it is the order of the instances in the code object), and its launch on
// the entry's own pointers (`lead`, the kernel's first arguments) and the plan's tables.  `what` completes the launch info.
#define F64_ENTRY_KERNEL(KERNEL, G) f64_entry_kernel(G, KERNEL<8>, KERNEL<16>, KERNEL<32>, KERNEL<64>)
template <class Kernel>
Kernel* f64_entry_kernel(int G, Kernel* k8, Kernel* k16, Kernel* k32, Kernel* k64) { return G == 8 ? k8 : G == 16 ? k16 : G == 32 ? k32 : k64; }

template <class Kernel, class Args, class... Lead>
int f64_entry_launch(Kernel* kernel, const char* name, const char* what, molann_plan* p, const F64Call<Args>& c, molann_stream_t stream, Lead... lead) {
    const Vjp64Geom& g = c.g;
    const int grid = grid_for(p, c.a.n_frames, g.block / g.G, 8);
    if (g.lds > VJP64_LDS_DEFAULT) {   // one wave, one frame, more than a launch may ask for by default: raise the kernel's limit
        const hipError_t e = hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(g.block), g.lds, (hipStream_t)stream, lead..., p->d_align_idx, p->d_ref64, p->d_items, p->d_hv_ptr,
                       p->d_hv_list, c.a, c.m);
    const int rc = (int)hipGetLastError();
    snprintf(p->last_info, sizeof(p->last_info), "%s (values + %s in one launch; %d lanes per frame) grid=%d block=%d lds=%d", name, what, g.G, grid,
             g.block, (int)g.lds);
    return rc;
}

// the grid of molann_value_and_grid_f64 from the caller's host arrays into the kernel's: false where an axis has fewer than 4 points, a
// spacing that is not finite and > 0 or a lower that is not finite, or where the table has 2^31 points or more
inline bool grid_geometry_f64(int d, const int64_t* shape, const double* lower, const double* spacing, const int32_t* periodic,
                              long (&n)[GRID_MAX_D], double (&lo)[GRID_MAX_D], double (&h)[GRID_MAX_D], int (&per)[GRID_MAX_D]) {
    int64_t points = 1;
    for (int k = 0; k < GRID_MAX_D; ++k) {
        n[k] = 4; lo[k] = 0.0; h[k] = 1.0; per[k] = 0;
        if (k >= d) continue;
        if (shape[k] < 4 || shape[k] >= (int64_t(1) << 31) || !(spacing[k] > 0.0) || !std::isfinite(spacing[k]) || !std::isfinite(lower[k])) return false;
        points *= shape[k];
        if (points >= (int64_t(1) << 31)) return false;
        n[k] = (long)shape[k]; lo[k] = lower[k]; h[k] = spacing[k]; per[k] = periodic && periodic[k] ? 1 : 0;
    }
    return true;
}

// one frame's hills on the host, through the functions the kernels call and in the order of one lane: returns V, dy[k < d] = dV/dy_k
inline double host_hills_f64(const double* y, int d, const double* centers, const double* heights, int64_t n_hills, const double* sigma,
                             int64_t sigma_stride, const double* period, double* dy) {
    double v = 0.;
    double acc[HILLS_MAX_D] = {0., 0., 0., 0., 0., 0., 0., 0.}, inv[HILLS_MAX_D] = {0., 0., 0., 0., 0., 0., 0., 0.};
    const bool shared = sigma_stride == 0;
    if (shared && n_hills > 0) hill_inverse_widths_f64(sigma, d, inv);
    for (int64_t h = 0; h < n_hills; ++h)
        v += hill_term_f64(y, centers + h * d, sigma + h * sigma_stride, inv, shared, period, heights[h], d, acc);
    if (dy)
        for (int k = 0; k < d; ++k) dy[k] = -acc[k];
    return v;
}

// one frame's OPES bias on the host, the same way: returns V, dy[k < d] = dV/dy_k
inline double host_opes_f64(const double* y, int d, const double* centers, const double* heights, int64_t n_kernels, const double* sigma,
                            int64_t sigma_stride, const double* period, double scale, double norm, double epsilon, double cutoff, double* dy) {
    double p = 0.;
    double acc[HILLS_MAX_D] = {0., 0., 0., 0., 0., 0., 0., 0.}, inv[HILLS_MAX_D] = {0., 0., 0., 0., 0., 0., 0., 0.}, cot[HILLS_MAX_D];
    if (n_kernels > 0) {
        const bool shared = sigma_stride == 0;
        if (shared) hill_inverse_widths_f64(sigma, d, inv);
        double c2, c0;
        opes_cutoff_f64(cutoff, c2, c0);
        for (int64_t h = 0; h < n_kernels; ++h)
            p += opes_term_f64(y, centers + h * d, sigma + h * sigma_stride, inv, shared, period, heights[h], c2, c0, d, acc);
    }
    const double v = opes_transform_f64(p, acc, scale, norm, epsilon, d, cot);
    if (dy)
        for (int k = 0; k < d; ++k) dy[k] = cot[k];
    return v;
}

// the four scalars of molann_value_and_opes_f64: scale finite; norm and epsilon finite and > 0; cutoff > 0, +inf for none (a NaN fails)
inline bool opes_scalars_f64(double scale, double norm, double epsilon, double cutoff) {
    return std::isfinite(scale) && std::isfinite(norm) && norm > 0.0 && std::isfinite(epsilon) && epsilon > 0.0 && cutoff > 0.0;
}
// the three of them that molann_value_and_opes_table_f64 takes by value (its norm is formed on the device), by the same rules
inline bool opes_table_scalars_f64(double scale, double epsilon, double cutoff) { return opes_scalars_f64(scale, 1.0, epsilon, cutoff); }

// one frame's OPES bias on the host from a table's state: n and norm as frames_value_opes_table_f64_kernel forms them, a row of widths
// per kernel
inline double host_opes_table_f64(const double* y, int d, const double* centers, const double* heights, const double* sigma, int64_t capacity,
                                  const double* state, const double* period, double scale, double epsilon, double cutoff, double* dy) {
    const long n = opes_live_count_f64(state[0], (long)capacity);
    const double norm = n > 0 ? opes_table_norm_f64(state[1], n) : 1.0;
    return host_opes_f64(y, d, centers, heights, n, sigma, d, period, scale, norm, epsilon, cutoff, dy);
}

// one frame's interpolation on the host, the same way: returns V, dy[k < d] = dV/dy_k; NaN for a grid grid_geometry_f64 refuses
inline double host_grid_f64(const double* y, int d, const double* table, const int64_t* shape, const double* lower, const double* spacing,
                            const int32_t* periodic, double* dy) {
    long n[GRID_MAX_D], idx[GRID_MAX_D][4] = {};
    double lo[GRID_MAX_D], h[GRID_MAX_D], a[GRID_MAX_D][4] = {}, b[GRID_MAX_D][4] = {};
    int per[GRID_MAX_D];
    if (!grid_geometry_f64(d, shape, lower, spacing, periodic, n, lo, h, per)) return (double)NAN;
    for (int k = 0; k < d; ++k) grid_axis_f64(y[k], n[k], lo[k], h[k], per[k] != 0, idx[k], a[k], b[k]);
    double v = 0.;
    double acc[GRID_MAX_D] = {0., 0., 0.};
    for (int p = 0; p < (1 << (2 * d)); ++p) {
        double term[GRID_MAX_D];
        v += grid_stencil_term_f64(p, d, table, n, idx, a, b, term);
        for (int k = 0; k < GRID_MAX_D; ++k) acc[k] += term[k];
    }
    if (dy)
        for (int k = 0; k < d; ++k) dy[k] = acc[k];
    return v;
}

// a column list of molann_value_and_bias_f64 against d_out, in the order of the refusals: an entry outside [0, d_out) or repeated
// (MOLANN_E_INDEX), more than `cap` entries (MOLANN_E_UNSUPPORTED), an identity list longer than d_out (MOLANN_E_INDEX); then the list is
// in `cols`
inline int bias_columns_f64(int32_t count, const int32_t* list, int cap, int d_out, int* cols) {
    if (list)
        for (int32_t j = 0; j < count; ++j) {
            if (list[j] < 0 || list[j] >= d_out) return MOLANN_E_INDEX;
            for (int32_t i = 0; i < j; ++i)
                if (list[i] == list[j]) return MOLANN_E_INDEX;
        }
    if (count > cap) return MOLANN_E_UNSUPPORTED;
    if (!list && count > d_out) return MOLANN_E_INDEX;
    for (int j = 0; j < cap; ++j) cols[j] = j < count ? (list ? list[j] : j) : 0;
    return MOLANN_OK;
}

// one frame of molann_value_and_bias_opes_f64 on the host once its scalars are accepted: the grid, the lists, then the terms in the
// kernel's order (the two host twins share it)
inline int host_bias_opes_frame_f64(const double* y, int d_out, const molann_bias_terms_f64* t, const molann_opes_term_f64* o, double* energies,
                                    double* dy) {
    const bool has_r = t && t->kappa, has_g = t && t->n_grid_columns > 0;
    int oc[HILLS_MAX_D], gc[GRID_MAX_D], per[GRID_MAX_D];
    long gn[GRID_MAX_D];
    double lo[GRID_MAX_D], gh[GRID_MAX_D];
    if (!grid_geometry_f64(has_g ? t->n_grid_columns : 0, has_g ? t->shape : nullptr, has_g ? t->lower : nullptr, has_g ? t->spacing : nullptr,
                           has_g ? t->periodic : nullptr, gn, lo, gh, per))
        return MOLANN_E_DESC;
    if (t && t->n_hills_columns != 0) return MOLANN_E_UNSUPPORTED;
    int rc = bias_columns_f64(o->n_columns, o->columns, HILLS_MAX_D, d_out, oc);
    if (rc == MOLANN_OK) rc = bias_columns_f64(has_g ? t->n_grid_columns : 0, has_g ? t->grid_columns : nullptr, GRID_MAX_D, d_out, gc);
    if (rc != MOLANN_OK) return rc;
    const int n_gc = has_g ? t->n_grid_columns : 0;
    double ysel[BIAS_SEL] = {}, dvo[HILLS_MAX_D] = {}, dg[GRID_MAX_D] = {};
    for (int j = 0; j < o->n_columns; ++j) ysel[j] = y[oc[j]];
    for (int j = 0; j < n_gc; ++j) ysel[HILLS_MAX_D + j] = y[gc[j]];
    double e = 0., vg = 0.;
    for (int k = 0; k < d_out; ++k) {
        dy[k] = 0.;
        if (has_r)
            e += restraint_term_f64(y[k], t->center[k], t->kappa[k], t->restraint_period ? t->restraint_period[k] : 0.0, t->flat ? t->flat[k] : 0.0,
                                    dy[k]);
    }
    const double vo = host_opes_f64(ysel, o->n_columns, o->centers, o->heights, o->n_kernels, o->sigma, o->sigma_stride, o->period, o->scale, o->norm,
                                    o->epsilon, o->cutoff, dvo);
    if (has_g) vg = host_grid_f64(ysel + HILLS_MAX_D, n_gc, t->table, t->shape, t->lower, t->spacing, t->periodic, dg);
    for (int j = 0; j < o->n_columns; ++j) dy[oc[j]] += dvo[j];
    for (int j = 0; j < n_gc; ++j) dy[gc[j]] += dg[j];
    energies[0] = e; energies[1] = 0.; energies[2] = vg; energies[3] = vo;
    return MOLANN_OK;
}

// the K axes of molann_value_and_pbmetad_f64 from the caller's host arrays into `a`, in the order of the refusals: K, the columns, each
// axis as grid_geometry_f64 has one, kT, the entries in all
struct PbmetadGeom {
    int K, col[PBMETAD_MAX_K], periodic[PBMETAD_MAX_K];
    long n[PBMETAD_MAX_K], off[PBMETAD_MAX_K];
    double lower[PBMETAD_MAX_K], h[PBMETAD_MAX_K];
};
inline int pbmetad_geometry_f64(const molann_pbmetad_terms_f64* t, int d_out, PbmetadGeom& g) {
    if (t->n_columns < 1) return MOLANN_E_DESC;
    if (t->n_columns > PBMETAD_MAX_K) return MOLANN_E_UNSUPPORTED;
    g.K = t->n_columns;
    const int rc = bias_columns_f64(g.K, t->columns, PBMETAD_MAX_K, d_out, g.col);
    if (rc != MOLANN_OK) return rc;
    int64_t entries = 0;
    for (int k = 0; k < PBMETAD_MAX_K; ++k) {
        g.n[k] = 4; g.off[k] = 0; g.lower[k] = 0.0; g.h[k] = 1.0; g.periodic[k] = 0;
        if (k >= g.K) continue;
        long n1[GRID_MAX_D];
        double lo1[GRID_MAX_D], h1[GRID_MAX_D];
        int per1[GRID_MAX_D];
        const int32_t periodic_k = t->periodic ? t->periodic[k] : 0;
        if (!grid_geometry_f64(1, t->shape + k, t->lower + k, t->spacing + k, &periodic_k, n1, lo1, h1, per1)) return MOLANN_E_DESC;
        g.n[k] = n1[0]; g.lower[k] = lo1[0]; g.h[k] = h1[0]; g.periodic[k] = per1[0];
    }
    if (!std::isfinite(t->kT) || !(t->kT > 0.0)) return MOLANN_E_DESC;
    for (int k = 0; k < g.K; ++k) {
        g.off[k] = (long)entries;
        entries += g.n[k];
        if (entries >= (int64_t(1) << 31)) return MOLANN_E_DESC;
    }
    return MOLANN_OK;
}

} // namespace

extern "C" {

int molann_plan_supports_value_and_vjp_f64(const molann_plan* p) {
    if (!p) return MOLANN_E_NULL;
    return f64_entry_geometry(p, F64_VJP).ok ? 1 : 0;
}

int molann_value_and_vjp_f64(molann_plan* p, const double* x, const double* grad_out, int64_t n, const double* const* W, const double* const* b,
                             double* out, double* grad_x, molann_stream_t stream) {
    F64Call<VjpF64Args> c;
    const int e = f64_entry_arguments(p, F64_VJP, n, {x, grad_out, out, grad_x}, {}, W, b, c);
    if (e != MOLANN_OK || n == 0) return e;
    return f64_entry_launch(F64_ENTRY_KERNEL(frames_value_vjp_f64_kernel, c.g.G), "frames_value_vjp_f64_kernel", "vjp", p, c, stream, x, grad_out, out,
                            grad_x);
}

int molann_plan_supports_value_and_jacobian_f64(const molann_plan* p) {
    if (!p) return MOLANN_E_NULL;
    return f64_entry_geometry(p, F64_JACOBIAN).ok ? 1 : 0;
}

int molann_value_and_jacobian_f64(molann_plan* p, const double* x, int64_t n, const double* const* W, const double* const* b, double* out, double* jac,
                                  molann_stream_t stream) {
    F64Call<JacF64Args> c;
    const int e = f64_entry_arguments(p, F64_JACOBIAN, n, {x, out, jac}, {}, W, b, c);
    if (e != MOLANN_OK || n == 0) return e;
    return f64_entry_launch(F64_ENTRY_KERNEL(frames_value_jac_f64_kernel, c.g.G), "frames_value_jac_f64_kernel", "Jacobian", p, c, stream, x, out, jac);
}

int molann_plan_supports_value_and_metric_f64(const molann_plan* p) {
    if (!p) return MOLANN_E_NULL;
    return f64_entry_geometry(p, F64_METRIC).ok ? 1 : 0;
}

int molann_value_and_metric_f64(molann_plan* p, const double* x, int64_t n, const double* const* W, const double* const* b, const double* atom_w,
                                double* out, double* metric, molann_stream_t stream) {
    F64Call<JacF64Args> c;
    const int e = f64_entry_arguments(p, F64_METRIC, n, {x, out, metric}, {atom_w}, W, b, c);
    if (e != MOLANN_OK || n == 0) return e;
    return f64_entry_launch(F64_ENTRY_KERNEL(frames_value_metric_f64_kernel, c.g.G), "frames_value_metric_f64_kernel", "metric", p, c, stream, x, out,
                            metric, atom_w);
}

int molann_plan_supports_value_and_restraint_f64(const molann_plan* p) {
    if (!p) return MOLANN_E_NULL;
    return f64_entry_geometry(p, F64_RESTRAINT).ok ? 1 : 0;
}

int molann_value_and_restraint_f64(molann_plan* p, const double* x, int64_t n, const double* const* W, const double* const* b, const double* center,
                                   int64_t center_stride, const double* kappa, const double* period, const double* flat, double* out, double* energy,
                                   double* grad_x, molann_stream_t stream) {
    F64Call<RestraintF64Args> c;
    const int e = f64_entry_arguments(p, F64_RESTRAINT, n, {x, center, kappa, out, energy, grad_x}, {period, flat}, W, b, c);
    if (e != MOLANN_OK || n == 0) return e;
    if (center_stride != 0 && center_stride != c.a.d_out) return MOLANN_E_DESC;
    c.a.center_stride = (long)center_stride;
    return f64_entry_launch(F64_ENTRY_KERNEL(frames_value_restraint_f64_kernel, c.g.G), "frames_value_restraint_f64_kernel", "restraint", p, c, stream,
                            x, center, kappa, period, flat, out, energy, grad_x);
}

int molann_plan_supports_value_and_hills_f64(const molann_plan* p) {
    if (!p) return MOLANN_E_NULL;
    return f64_entry_geometry(p, F64_HILLS).ok ? 1 : 0;
}

int molann_value_and_hills_f64(molann_plan* p, const double* x, int64_t n, const double* const* W, const double* const* b, const double* centers,
                               const double* heights, int64_t n_hills, const double* sigma, int64_t sigma_stride, const double* period, double* out,
                               double* bias, double* grad_x, molann_stream_t stream) {
    if (p && n_hills < 0) return MOLANN_E_DESC;
    F64Call<HillsF64Args> c;
    // The table - centres, heights and widths - is required where it has rows.  Without rows nothing of it is read, so its three
    // pointers are optional then; that includes sigma, because a [0, d_out] tensor of per-hill widths has no address.
    const int e = n_hills > 0 ? f64_entry_arguments(p, F64_HILLS, n, {x, centers, heights, sigma, out, bias, grad_x}, {period}, W, b, c)
                              : f64_entry_arguments(p, F64_HILLS, n, {x, out, bias, grad_x}, {centers, heights, sigma, period}, W, b, c);
    if (e != MOLANN_OK || n == 0) return e;
    if (sigma_stride != 0 && sigma_stride != c.a.d_out) return MOLANN_E_DESC;
    c.a.n_hills = (long)n_hills;
    c.a.sigma_stride = (long)sigma_stride;
    return f64_entry_launch(F64_ENTRY_KERNEL(frames_value_hills_f64_kernel, c.g.G), "frames_value_hills_f64_kernel", "hills", p, c, stream, x, centers,
                            heights, sigma, period, out, bias, grad_x);
}

int molann_plan_supports_value_and_opes_f64(const molann_plan* p) {
    if (!p) return MOLANN_E_NULL;
    return f64_entry_geometry(p, F64_HILLS).ok ? 1 : 0;
}

int molann_value_and_opes_f64(molann_plan* p, const double* x, int64_t n, const double* const* W, const double* const* b, const double* centers,
                              const double* heights, int64_t n_kernels, const double* sigma, int64_t sigma_stride, const double* period, double scale,
                              double norm, double epsilon, double cutoff, double* out, double* bias, double* grad_x, molann_stream_t stream) {
    if (p && n_kernels < 0) return MOLANN_E_DESC;
    F64Call<OpesF64Args> c;
    // the table is required where it has rows, as molann_value_and_hills_f64 has it
    const int e = n_kernels > 0 ? f64_entry_arguments(p, F64_HILLS, n, {x, centers, heights, sigma, out, bias, grad_x}, {period}, W, b, c)
                                : f64_entry_arguments(p, F64_HILLS, n, {x, out, bias, grad_x}, {centers, heights, sigma, period}, W, b, c);
    if (e != MOLANN_OK || n == 0) return e;
    if (sigma_stride != 0 && sigma_stride != c.a.d_out) return MOLANN_E_DESC;
    if (!opes_scalars_f64(scale, norm, epsilon, cutoff)) return MOLANN_E_DESC;
    c.a.n_kernels = (long)n_kernels;
    c.a.sigma_stride = (long)sigma_stride;
    c.a.scale = scale; c.a.norm = norm; c.a.epsilon = epsilon; c.a.cutoff = cutoff;
    return f64_entry_launch(F64_ENTRY_KERNEL(frames_value_opes_f64_kernel, c.g.G), "frames_value_opes_f64_kernel", "opes", p, c, stream, x, centers,
                            heights, sigma, period, out, bias, grad_x);
}

int molann_plan_supports_value_and_opes_table_f64(const molann_plan* p) { return molann_plan_supports_value_and_opes_f64(p); }

int molann_value_and_opes_table_f64(molann_plan* p, const double* x, int64_t n, const double* const* W, const double* const* b, const double* centers,
                                    const double* heights, const double* sigma, int64_t capacity, const double* state, const double* period,
                                    double scale, double epsilon, double cutoff, double* out, double* bias, double* grad_x, molann_stream_t stream) {
    F64Call<OpesTableF64Args> c;
    // the table has storage whatever its live count, which only the device knows: its three pointers and the state are required
    const int e = f64_entry_arguments(p, F64_HILLS, n, {x, centers, heights, sigma, state, out, bias, grad_x}, {period}, W, b, c);
    if (e != MOLANN_OK || n == 0) return e;
    if (capacity < 1) return MOLANN_E_DESC;
    if (!opes_table_scalars_f64(scale, epsilon, cutoff)) return MOLANN_E_DESC;
    c.a.capacity = (long)capacity;
    c.a.scale = scale; c.a.epsilon = epsilon; c.a.cutoff = cutoff;
    return f64_entry_launch(F64_ENTRY_KERNEL(frames_value_opes_table_f64_kernel, c.g.G), "frames_value_opes_table_f64_kernel", "opes from the table's state",
                            p, c, stream, x, centers, heights, sigma, state, period, out, bias, grad_x);
}

int molann_plan_supports_value_and_grid_f64(const molann_plan* p) {
    if (!p) return MOLANN_E_NULL;
    return f64_entry_geometry(p, F64_GRID).ok ? 1 : 0;
}

int molann_value_and_grid_f64(molann_plan* p, const double* x, int64_t n, const double* const* W, const double* const* b, const double* table,
                              const int64_t* shape, const double* lower, const double* spacing, const int32_t* periodic, double* out, double* bias,
                              double* grad_x, molann_stream_t stream) {
    F64Call<GridF64Args> c;
    const int e = f64_entry_arguments(p, F64_GRID, n, {x, table, out, bias, grad_x}, {}, W, b, c);
    if (e != MOLANN_OK || n == 0) return e;
    // the grid's geometry: host arrays of d_out entries, read now and carried by value
    if (!shape || !lower || !spacing) return MOLANN_E_NULL;
    if (!grid_geometry_f64(c.a.d_out, shape, lower, spacing, periodic, c.a.n, c.a.lower, c.a.h, c.a.periodic)) return MOLANN_E_DESC;
    return f64_entry_launch(F64_ENTRY_KERNEL(frames_value_grid_f64_kernel, c.g.G), "frames_value_grid_f64_kernel", "grid", p, c, stream, x, table, out,
                            bias, grad_x);
}

int molann_plan_supports_value_and_bias_f64(const molann_plan* p) {
    if (!p) return MOLANN_E_NULL;
    return f64_entry_geometry(p, F64_BIAS).ok ? 1 : 0;
}

int molann_value_and_bias_f64(molann_plan* p, const double* x, int64_t n, const double* const* W, const double* const* b,
                              const molann_bias_terms_f64* t, double* out, double* energies, double* grad_x, molann_stream_t stream) {
    if (p && !t) return MOLANN_E_NULL;
    // the host arrays of a present table are required pointers like the others: refused with them, before alignment (and, like them, not
    // looked at where n <= 0)
    if (p && n > 0 && t->n_grid_columns > 0 && (!t->shape || !t->lower || !t->spacing)) return MOLANN_E_NULL;
    F64Call<BiasF64Args> c;
    // A term that is absent has none of its pointers looked at (x stands in for them below); the hill table is required where it has rows,
    // as molann_value_and_hills_f64 has it.
    const bool has_r = t && t->kappa, has_h = t && t->n_hills_columns > 0, has_g = t && t->n_grid_columns > 0, rows = has_h && t->n_hills > 0;
    const int e = f64_entry_arguments(p, F64_BIAS, n,
                                      {x, out, energies, grad_x, has_r ? t->center : x, rows ? t->centers : x, rows ? t->heights : x,
                                       rows ? t->sigma : x, has_g ? t->table : x},
                                      {has_r ? t->restraint_period : nullptr, has_r ? t->flat : nullptr, has_h ? t->hills_period : nullptr,
                                       has_h && !rows ? t->centers : nullptr, has_h && !rows ? t->heights : nullptr,
                                       has_h && !rows ? t->sigma : nullptr},
                                      W, b, c);
    if (e != MOLANN_OK || n == 0) return e;
    if (!has_r && t->n_hills_columns == 0 && t->n_grid_columns == 0) return MOLANN_E_DESC;
    if (t->n_hills_columns < 0 || t->n_grid_columns < 0 || (has_h && t->n_hills < 0)) return MOLANN_E_DESC;
    BiasF64Args& a = c.a;
    if (has_r && t->center_stride != 0 && t->center_stride != a.d_out) return MOLANN_E_DESC;
    if (has_h && t->sigma_stride != 0 && t->sigma_stride != t->n_hills_columns) return MOLANN_E_DESC;
    if (!grid_geometry_f64(has_g ? t->n_grid_columns : 0, t->shape, t->lower, t->spacing, t->periodic, a.n, a.lower, a.h, a.periodic))
        return MOLANN_E_DESC;
    int rc = bias_columns_f64(t->n_hills_columns, t->hills_columns, HILLS_MAX_D, a.d_out, a.hc);
    if (rc == MOLANN_OK) rc = bias_columns_f64(t->n_grid_columns, t->grid_columns, GRID_MAX_D, a.d_out, a.gc);
    if (rc != MOLANN_OK) return rc;
    a.has_restraint = has_r ? 1 : 0;
    a.n_hc = t->n_hills_columns; a.n_gc = t->n_grid_columns;
    a.center_stride = has_r ? (long)t->center_stride : 0;
    a.n_hills = has_h ? (long)t->n_hills : 0;
    a.sigma_stride = has_h ? (long)t->sigma_stride : 0;
    const double* none = nullptr;
    return f64_entry_launch(F64_ENTRY_KERNEL(frames_value_bias_f64_kernel, c.g.G), "frames_value_bias_f64_kernel", "bias", p, c, stream, x,
                            has_r ? t->center : none, has_r ? t->kappa : none, has_r ? t->restraint_period : none, has_r ? t->flat : none,
                            rows ? t->centers : none, rows ? t->heights : none, rows ? t->sigma : none, has_h ? t->hills_period : none,
                            has_g ? t->table : none, out, energies, grad_x);
}

int molann_plan_supports_value_and_bias_opes_f64(const molann_plan* p) { return molann_plan_supports_value_and_bias_f64(p); }

int molann_value_and_bias_opes_f64(molann_plan* p, const double* x, int64_t n, const double* const* W, const double* const* b,
                                   const molann_bias_terms_f64* t, const molann_opes_term_f64* o, double* out, double* energies, double* grad_x,
                                   molann_stream_t stream) {
    if (p && !o) return MOLANN_E_NULL;
    // the host arrays of a present table are required pointers, as molann_value_and_bias_f64 has them
    if (p && n > 0 && t && t->n_grid_columns > 0 && (!t->shape || !t->lower || !t->spacing)) return MOLANN_E_NULL;
    F64Call<BiasOpesF64Args> c;
    // An absent restraint or table has none of its pointers looked at (x stands in for them below); the kernel table is required where it
    // has rows, as molann_value_and_opes_f64 has it.  The hills' pointers of `t` are never looked at: hills are refused below.
    const bool has_r = t && t->kappa, has_g = t && t->n_grid_columns > 0, rows = o && o->n_kernels > 0;
    const int e = f64_entry_arguments(p, F64_BIAS, n,
                                      {x, out, energies, grad_x, has_r ? t->center : x, rows ? o->centers : x, rows ? o->heights : x,
                                       rows ? o->sigma : x, has_g ? t->table : x},
                                      {has_r ? t->restraint_period : nullptr, has_r ? t->flat : nullptr, o ? o->period : nullptr,
                                       o && !rows ? o->centers : nullptr, o && !rows ? o->heights : nullptr, o && !rows ? o->sigma : nullptr},
                                      W, b, c);
    if (e != MOLANN_OK || n == 0) return e;
    BiasOpesF64Args& a = c.a;
    if (o->n_columns <= 0 || o->n_kernels < 0 || (t && t->n_grid_columns < 0)) return MOLANN_E_DESC;
    if (has_r && t->center_stride != 0 && t->center_stride != a.d_out) return MOLANN_E_DESC;
    if (o->sigma_stride != 0 && o->sigma_stride != o->n_columns) return MOLANN_E_DESC;
    if (!opes_scalars_f64(o->scale, o->norm, o->epsilon, o->cutoff)) return MOLANN_E_DESC;
    if (!grid_geometry_f64(has_g ? t->n_grid_columns : 0, has_g ? t->shape : nullptr, has_g ? t->lower : nullptr, has_g ? t->spacing : nullptr,
                           has_g ? t->periodic : nullptr, a.n, a.lower, a.h, a.periodic))
        return MOLANN_E_DESC;
    if (t && t->n_hills_columns != 0) return MOLANN_E_UNSUPPORTED;   // hills and OPES in one launch: out of scope
    int rc = bias_columns_f64(o->n_columns, o->columns, HILLS_MAX_D, a.d_out, a.oc);
    if (rc == MOLANN_OK) rc = bias_columns_f64(has_g ? t->n_grid_columns : 0, has_g ? t->grid_columns : nullptr, GRID_MAX_D, a.d_out, a.gc);
    if (rc != MOLANN_OK) return rc;
    a.has_restraint = has_r ? 1 : 0;
    a.n_oc = o->n_columns; a.n_gc = has_g ? t->n_grid_columns : 0;
    a.center_stride = has_r ? (long)t->center_stride : 0;
    a.n_kernels = (long)o->n_kernels;
    a.sigma_stride = (long)o->sigma_stride;
    a.scale = o->scale; a.norm = o->norm; a.epsilon = o->epsilon; a.cutoff = o->cutoff;
    const double* none = nullptr;
    return f64_entry_launch(F64_ENTRY_KERNEL(frames_value_bias_opes_f64_kernel, c.g.G), "frames_value_bias_opes_f64_kernel", "bias + opes", p, c, stream,
                            x, has_r ? t->center : none, has_r ? t->kappa : none, has_r ? t->restraint_period : none, has_r ? t->flat : none,
                            rows ? o->centers : none, rows ? o->heights : none, rows ? o->sigma : none, o->period, has_g ? t->table : none, out,
                            energies, grad_x);
}

int molann_plan_supports_value_and_bias_opes_table_f64(const molann_plan* p) { return molann_plan_supports_value_and_bias_f64(p); }

int molann_value_and_bias_opes_table_f64(molann_plan* p, const double* x, int64_t n, const double* const* W, const double* const* b,
                                         const molann_bias_terms_f64* t, const molann_opes_table_term_f64* o, double* out, double* energies,
                                         double* grad_x, molann_stream_t stream) {
    if (p && !o) return MOLANN_E_NULL;
    // the host arrays of a present table are required pointers, as molann_value_and_bias_f64 has them
    if (p && n > 0 && t && t->n_grid_columns > 0 && (!t->shape || !t->lower || !t->spacing)) return MOLANN_E_NULL;
    F64Call<BiasOpesTableF64Args> c;
    // An absent restraint or table has none of its pointers looked at (x stands in for them below).  The kernel table has storage whatever
    // its live count, which only the device knows: its three pointers and the state are required, as molann_value_and_opes_table_f64 has
    // them.  The hills' pointers of `t` are never looked at: hills are refused below.
    const bool has_r = t && t->kappa, has_g = t && t->n_grid_columns > 0;
    const int e = f64_entry_arguments(p, F64_BIAS, n,
                                      {x, out, energies, grad_x, has_r ? t->center : x, o ? o->centers : x, o ? o->heights : x, o ? o->sigma : x,
                                       o ? o->state : x, has_g ? t->table : x},
                                      {has_r ? t->kappa : nullptr, has_r ? t->restraint_period : nullptr, has_r ? t->flat : nullptr,
                                       o ? o->period : nullptr},      // kappa is there where the restraint is: its alignment is what is left to check
                                      W, b, c);
    if (e != MOLANN_OK || n == 0) return e;
    BiasOpesTableF64Args& a = c.a;
    if (o->n_columns <= 0 || (t && t->n_grid_columns < 0)) return MOLANN_E_DESC;
    if (has_r && t->center_stride != 0 && t->center_stride != a.d_out) return MOLANN_E_DESC;
    if (o->capacity < 1) return MOLANN_E_DESC;
    if (!opes_table_scalars_f64(o->scale, o->epsilon, o->cutoff)) return MOLANN_E_DESC;
    if (!grid_geometry_f64(has_g ? t->n_grid_columns : 0, has_g ? t->shape : nullptr, has_g ? t->lower : nullptr, has_g ? t->spacing : nullptr,
                           has_g ? t->periodic : nullptr, a.n, a.lower, a.h, a.periodic))
        return MOLANN_E_DESC;
    if (t && t->n_hills_columns != 0) return MOLANN_E_UNSUPPORTED;   // hills and OPES in one launch: out of scope
    int rc = bias_columns_f64(o->n_columns, o->columns, HILLS_MAX_D, a.d_out, a.oc);
    if (rc == MOLANN_OK) rc = bias_columns_f64(has_g ? t->n_grid_columns : 0, has_g ? t->grid_columns : nullptr, GRID_MAX_D, a.d_out, a.gc);
    if (rc != MOLANN_OK) return rc;
    a.has_restraint = has_r ? 1 : 0;
    a.n_oc = o->n_columns; a.n_gc = has_g ? t->n_grid_columns : 0;
    a.center_stride = has_r ? (long)t->center_stride : 0;
    a.capacity = (long)o->capacity;
    a.scale = o->scale; a.epsilon = o->epsilon; a.cutoff = o->cutoff;
    const double* none = nullptr;
    return f64_entry_launch(F64_ENTRY_KERNEL(frames_value_bias_opes_table_f64_kernel, c.g.G), "frames_value_bias_opes_table_f64_kernel",
                            "bias + opes from the table's state", p, c, stream, x, has_r ? t->center : none, has_r ? t->kappa : none,
                            has_r ? t->restraint_period : none, has_r ? t->flat : none, o->centers, o->heights, o->sigma, o->state, o->period,
                            has_g ? t->table : none, out, energies, grad_x);
}

int molann_plan_supports_value_and_pbmetad_f64(const molann_plan* p) { return molann_plan_supports_value_and_bias_f64(p); }

int molann_value_and_pbmetad_f64(molann_plan* p, const double* x, int64_t n, const double* const* W, const double* const* b,
                                 const molann_pbmetad_terms_f64* t, double* out, double* energies, int64_t energies_stride, double* grad_x,
                                 molann_stream_t stream) {
    if (p && !t) return MOLANN_E_NULL;
    // the host arrays of the tables are required pointers like the others: refused with them, before alignment (and, like them, not
    // looked at where n <= 0)
    if (p && n > 0 && (!t->shape || !t->lower || !t->spacing)) return MOLANN_E_NULL;
    F64Call<PbmetadF64Args> c;
    // an absent restraint has none of its pointers looked at (x stands in for its centre below)
    const bool has_r = t && t->kappa;
    const int e = f64_entry_arguments(p, F64_BIAS, n, {x, out, energies, grad_x, t ? t->table : x, has_r ? t->center : x},
                                      {has_r ? t->restraint_period : nullptr, has_r ? t->flat : nullptr}, W, b, c);
    if (e != MOLANN_OK || n == 0) return e;
    PbmetadF64Args& a = c.a;
    PbmetadGeom g;
    const int rc = pbmetad_geometry_f64(t, a.d_out, g);
    if (rc != MOLANN_OK) return rc;
    if (energies_stride < 2 + g.K) return MOLANN_E_DESC;
    if (has_r && t->center_stride != 0 && t->center_stride != a.d_out) return MOLANN_E_DESC;
    a.has_restraint = has_r ? 1 : 0;
    a.K = g.K;
    for (int k = 0; k < PBMETAD_MAX_K; ++k) {
        a.col[k] = g.col[k]; a.periodic[k] = g.periodic[k]; a.n[k] = g.n[k]; a.off[k] = g.off[k]; a.lower[k] = g.lower[k]; a.h[k] = g.h[k];
    }
    a.center_stride = has_r ? (long)t->center_stride : 0;
    a.e_stride = (long)energies_stride;
    a.kT = t->kT;
    const double* none = nullptr;
    return f64_entry_launch(F64_ENTRY_KERNEL(frames_value_pbmetad_f64_kernel, c.g.G), "frames_value_pbmetad_f64_kernel", "parallel bias", p, c, stream,
                            x, has_r ? t->center : none, has_r ? t->kappa : none, has_r ? t->restraint_period : none, has_r ? t->flat : none,
                            t->table, out, energies, grad_x);
}

double molann_selftest_act_derivative_f64(int act, double z) { return act_derivative_f64(act, z); }

double molann_selftest_restraint_f64(double y, double z, double kappa, double period, double flat, double* dy) {
    double cot;
    const double e = restraint_term_f64(y, z, kappa, period, flat, cot);
    if (dy) *dy = cot;
    return e;
}

double molann_selftest_hills_f64(const double* y, int d, const double* centers, const double* heights, int64_t n_hills, const double* sigma,
                                 int64_t sigma_stride, const double* period, double* dy) {
    if (!y || d < 1 || d > HILLS64_MAX_D_OUT || n_hills < 0 || (n_hills > 0 && (!centers || !heights || !sigma))) return (double)NAN;
    return host_hills_f64(y, d, centers, heights, n_hills, sigma, sigma_stride, period, dy);
}

double molann_selftest_opes_f64(const double* y, int d, const double* centers, const double* heights, int64_t n_kernels, const double* sigma,
                                int64_t sigma_stride, const double* period, double scale, double norm, double epsilon, double cutoff, double* dy) {
    if (!y || d < 1 || d > HILLS64_MAX_D_OUT || n_kernels < 0 || (n_kernels > 0 && (!centers || !heights || !sigma))) return (double)NAN;
    return host_opes_f64(y, d, centers, heights, n_kernels, sigma, sigma_stride, period, scale, norm, epsilon, cutoff, dy);
}

double molann_selftest_opes_table_f64(const double* y, int d, const double* centers, const double* heights, const double* sigma, int64_t capacity,
                                      const double* state, const double* period, double scale, double epsilon, double cutoff, double* dy) {
    if (!y || d < 1 || d > HILLS64_MAX_D_OUT || capacity < 1 || !centers || !heights || !sigma || !state) return (double)NAN;
    return host_opes_table_f64(y, d, centers, heights, sigma, capacity, state, period, scale, epsilon, cutoff, dy);
}

void molann_selftest_grid_axis_f64(double y, int64_t n, double lower, double spacing, int32_t periodic, int64_t idx[4], double w[4], double dw[4]) {
    long i4[4];
    double a4[4], b4[4];
    grid_axis_f64(y, (long)n, lower, spacing, periodic != 0, i4, a4, b4);
    for (int j = 0; j < 4; ++j) {
        if (idx) idx[j] = i4[j];
        if (w) w[j] = a4[j];
        if (dw) dw[j] = b4[j];
    }
}

double molann_selftest_grid_f64(const double* y, int d, const double* table, const int64_t* shape, const double* lower, const double* spacing,
                                const int32_t* periodic, double* dy) {
    if (!y || !table || !shape || !lower || !spacing || d < 1 || d > GRID64_MAX_D_OUT) return (double)NAN;
    return host_grid_f64(y, d, table, shape, lower, spacing, periodic, dy);
}

int molann_selftest_bias_f64(const double* y, int d_out, const molann_bias_terms_f64* t, double* energies, double* dy) {
    if (!y || !t || !energies || !dy) return MOLANN_E_NULL;
    const bool has_r = t->kappa, has_h = t->n_hills_columns > 0, has_g = t->n_grid_columns > 0;
    if (d_out < 1 || t->n_hills_columns < 0 || t->n_grid_columns < 0 || (!has_r && !has_h && !has_g) || (has_h && t->n_hills < 0)) return MOLANN_E_DESC;
    if ((has_r && !t->center) || (has_h && t->n_hills > 0 && (!t->centers || !t->heights || !t->sigma)) ||
        (has_g && (!t->table || !t->shape || !t->lower || !t->spacing)))
        return MOLANN_E_NULL;
    int hc[HILLS_MAX_D], gc[GRID_MAX_D], per[GRID_MAX_D];
    long gn[GRID_MAX_D];
    double lo[GRID_MAX_D], gh[GRID_MAX_D];
    if (has_h && t->sigma_stride != 0 && t->sigma_stride != t->n_hills_columns) return MOLANN_E_DESC;
    if (!grid_geometry_f64(has_g ? t->n_grid_columns : 0, t->shape, t->lower, t->spacing, t->periodic, gn, lo, gh, per)) return MOLANN_E_DESC;
    int rc = bias_columns_f64(t->n_hills_columns, t->hills_columns, HILLS_MAX_D, d_out, hc);
    if (rc == MOLANN_OK) rc = bias_columns_f64(t->n_grid_columns, t->grid_columns, GRID_MAX_D, d_out, gc);
    if (rc != MOLANN_OK) return rc;
    double ysel[BIAS_SEL] = {}, dh[HILLS_MAX_D] = {}, dg[GRID_MAX_D] = {};
    for (int j = 0; j < t->n_hills_columns; ++j) ysel[j] = y[hc[j]];
    for (int j = 0; j < t->n_grid_columns; ++j) ysel[HILLS_MAX_D + j] = y[gc[j]];
    double e = 0., vh = 0., vg = 0.;
    for (int k = 0; k < d_out; ++k) {
        dy[k] = 0.;
        if (has_r)
            e += restraint_term_f64(y[k], t->center[k], t->kappa[k], t->restraint_period ? t->restraint_period[k] : 0.0, t->flat ? t->flat[k] : 0.0,
                                    dy[k]);
    }
    if (has_h)
        vh = host_hills_f64(ysel, t->n_hills_columns, t->centers, t->heights, t->n_hills, t->sigma, t->sigma_stride, t->hills_period, dh);
    if (has_g) vg = host_grid_f64(ysel + HILLS_MAX_D, t->n_grid_columns, t->table, t->shape, t->lower, t->spacing, t->periodic, dg);
    for (int j = 0; j < t->n_hills_columns; ++j) dy[hc[j]] += dh[j];
    for (int j = 0; j < t->n_grid_columns; ++j) dy[gc[j]] += dg[j];
    energies[0] = e; energies[1] = vh; energies[2] = vg;
    return MOLANN_OK;
}

int molann_selftest_pbmetad_f64(const double* y, int d_out, const molann_pbmetad_terms_f64* t, double* energies, double* dy) {
    if (!y || !t || !energies || !dy) return MOLANN_E_NULL;
    const bool has_r = t->kappa;
    if (!t->table || !t->shape || !t->lower || !t->spacing || (has_r && !t->center)) return MOLANN_E_NULL;
    if (d_out < 1) return MOLANN_E_DESC;
    PbmetadGeom g;
    const int rc = pbmetad_geometry_f64(t, d_out, g);
    if (rc != MOLANN_OK) return rc;
    double e = 0.;
    for (int k = 0; k < d_out; ++k) {
        dy[k] = 0.;
        if (has_r)
            e += restraint_term_f64(y[k], t->center[k], t->kappa[k], t->restraint_period ? t->restraint_period[k] : 0.0, t->flat ? t->flat[k] : 0.0,
                                    dy[k]);
    }
    double V[PBMETAD_MAX_K] = {}, dV[PBMETAD_MAX_K] = {}, w[PBMETAD_MAX_K];
    for (int k = 0; k < g.K; ++k)
        pbmetad_axis_value_f64(y[g.col[k]], t->table + g.off[k], g.n[k], g.lower[k], g.h[k], g.periodic[k] != 0, V[k], dV[k]);
    const double vpb = pbmetad_softmin_f64(V, g.K, t->kT, w);
    for (int k = 0; k < g.K; ++k) dy[g.col[k]] = pbmetad_cotangent_f64(dy[g.col[k]], w[k], dV[k]);
    energies[0] = e; energies[1] = vpb;
    for (int k = 0; k < g.K; ++k) energies[2 + k] = V[k];
    return MOLANN_OK;
}

int molann_selftest_bias_opes_f64(const double* y, int d_out, const molann_bias_terms_f64* t, const molann_opes_term_f64* o, double* energies, double* dy) {
    if (!y || !o || !energies || !dy) return MOLANN_E_NULL;
    const bool has_r = t && t->kappa, has_g = t && t->n_grid_columns > 0;
    if ((has_r && !t->center) || (o->n_kernels > 0 && (!o->centers || !o->heights || !o->sigma)) ||
        (has_g && (!t->table || !t->shape || !t->lower || !t->spacing)))
        return MOLANN_E_NULL;
    if (d_out < 1 || o->n_columns <= 0 || o->n_kernels < 0 || (t && t->n_grid_columns < 0)) return MOLANN_E_DESC;
    if (o->sigma_stride != 0 && o->sigma_stride != o->n_columns) return MOLANN_E_DESC;
    if (!opes_scalars_f64(o->scale, o->norm, o->epsilon, o->cutoff)) return MOLANN_E_DESC;
    return host_bias_opes_frame_f64(y, d_out, t, o, energies, dy);
}

int molann_selftest_bias_opes_table_f64(const double* y, int d_out, const molann_bias_terms_f64* t, const molann_opes_table_term_f64* o,
                                        double* energies, double* dy) {
    if (!y || !o || !energies || !dy) return MOLANN_E_NULL;
    const bool has_r = t && t->kappa, has_g = t && t->n_grid_columns > 0;
    if ((has_r && !t->center) || !o->centers || !o->heights || !o->sigma || !o->state ||
        (has_g && (!t->table || !t->shape || !t->lower || !t->spacing)))
        return MOLANN_E_NULL;
    if (d_out < 1 || o->n_columns <= 0 || (t && t->n_grid_columns < 0)) return MOLANN_E_DESC;
    if (o->capacity < 1) return MOLANN_E_DESC;
    if (!opes_table_scalars_f64(o->scale, o->epsilon, o->cutoff)) return MOLANN_E_DESC;
    // n and norm as frames_value_bias_opes_table_f64_kernel forms them, a row of widths per kernel; the norm goes on as it comes
    const long n = opes_live_count_f64(o->state[0], (long)o->capacity);
    const double norm = n > 0 ? opes_table_norm_f64(o->state[1], n) : 1.0;
    const molann_opes_term_f64 term = {o->n_columns, o->columns, o->centers, o->heights, (int64_t)n, o->sigma, (int64_t)o->n_columns, o->period,
                                       o->scale, norm, o->epsilon, o->cutoff};
    return host_bias_opes_frame_f64(y, d_out, t, &term, energies, dy);
}

int molann_selftest_item_jacobian_f64(int type, int use_angle_value, const double* a, double* jac36) {
    if (!a || !jac36) return MOLANN_E_NULL;
    const int it = selftest_item_type(type, use_angle_value);
    if (it < 0) return MOLANN_E_FEATURE;
    const int w = item_width(it);
    for (int c = 0; c < 3; ++c) {
        V3d u[4] = {v3d(0., 0., 0.), v3d(0., 0., 0.), v3d(0., 0., 0.), v3d(0., 0., 0.)};
        if (c < w)
            item_unit_backward_f64(it, v3d(a[0], a[1], a[2]), v3d(a[3], a[4], a[5]), v3d(a[6], a[7], a[8]), v3d(a[9], a[10], a[11]), c, u);
        for (int j = 0; j < 4; ++j) { jac36[12 * c + 3 * j] = u[j].x; jac36[12 * c + 3 * j + 1] = u[j].y; jac36[12 * c + 3 * j + 2] = u[j].z; }
    }
    return w;
}

} // extern "C"
