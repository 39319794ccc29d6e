// molann_vjp_f64.inc - part of libmolann_hip.so, included by molann_kernels.hip after molann_hvp.inc.  Float64 values and forces in
// one launch: molann_value_and_vjp_f64 (see include/molann_hip.h) and its launch of frames_value_vjp_f64_kernel
// (molann_dev_vjp_f64.inc).
namespace {

constexpr size_t VJP64_LDS_DEFAULT = 65536;    // dynamic LDS a launch may ask for as it is
constexpr size_t VJP64_LDS_CU = 163840;        // the LDS of a gfx950 compute unit (one block of one wave may take all of it)

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

// lanes per frame: the smallest group that covers the atoms, the items, the align atoms and the head's widest layer in one round
// (8/4/2 frames per wave), a whole wave from 33 on; fewer waves per block, then one wave per frame, where the rows ask for it
// (the rows are the caller's: molann_jac_f64.inc sizes its own and steps down the same way)
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
inline Vjp64Geom vjp64_geometry(const molann_plan* p) {
    int max_w, per_frame;
    vjp64_rows(p, max_w, per_frame);
    return vjp64_geometry_rows(p, max_w, per_frame);
}

template <int G>
int launch_vjp64(const molann_plan* p, const Vjp64Geom& g, int grid, hipStream_t s, const double* x, const double* gout, double* out, double* gx,
                 const VjpF64Args& a, const F64Mlp& m) {
    if (g.lds > VJP64_LDS_DEFAULT) {   // one wave, one frame, more than a launch may ask for by default: raise the kernel's limit
        const hipError_t e = hipFuncSetAttribute((const void*)frames_value_vjp_f64_kernel<G>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL((frames_value_vjp_f64_kernel<G>), dim3(grid), dim3(g.block), g.lds, s, x, gout, out, gx, p->d_align_idx, p->d_ref64,
                       p->d_items, p->d_hv_ptr, p->d_hv_list, a, m);
    return (int)hipGetLastError();
}

} // namespace

extern "C" {

int molann_plan_supports_value_and_vjp_f64(const molann_plan* p) {
    if (!p) return MOLANN_E_NULL;
    return vjp64_geometry(p).ok ? 1 : 0;
}

int molann_value_and_vjp_f64(molann_plan* p, const double* x, const double* grad_out, int64_t n, const double* const* W, const double* const* b,
                             double* out, double* grad_x, molann_stream_t stream) {
    if (!p) return MOLANN_E_NULL;
    if (n < 0) return MOLANN_E_DESC;
    if (n == 0) return MOLANN_OK;
    if (!x || !grad_out || !out || !grad_x) return MOLANN_E_NULL;
    if ((((uintptr_t)x) & 7) || (((uintptr_t)grad_out) & 7) || (((uintptr_t)grad_x) & 7) || (((uintptr_t)out) & 7)) return MOLANN_E_ALIGNMENT;
    if (p->n_items <= 0) return MOLANN_E_STAGE;
    F64Mlp m;
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
    const Vjp64Geom g = vjp64_geometry(p);
    if (!g.ok) return MOLANN_E_UNSUPPORTED;
    VjpF64Args a;
    a.n_frames = (long)n;
    a.n_inp = p->n_inp; a.n_align = p->n_align; a.n_items = p->n_items; a.d_feat = p->d_feat;
    a.d_out = p->n_layers > 0 ? p->dims[p->n_layers] : p->d_feat;
    vjp64_rows(p, a.max_w, a.lds_per_frame);
    m.max_w = a.max_w;
    const int grid = grid_for(p, (long)n, g.block / g.G, 8);
    hipStream_t s = (hipStream_t)stream;
    int rc;
    switch (g.G) {
    case 8: rc = launch_vjp64<8>(p, g, grid, s, x, grad_out, out, grad_x, a, m); break;
    case 16: rc = launch_vjp64<16>(p, g, grid, s, x, grad_out, out, grad_x, a, m); break;
    case 32: rc = launch_vjp64<32>(p, g, grid, s, x, grad_out, out, grad_x, a, m); break;
    default: rc = launch_vjp64<64>(p, g, grid, s, x, grad_out, out, grad_x, a, m); break;
    }
    snprintf(p->last_info, sizeof(p->last_info), "frames_value_vjp_f64_kernel (values + vjp in one launch; %d lanes per frame) grid=%d block=%d lds=%d",
             g.G, grid, g.block, (int)g.lds);
    return rc;
}

double molann_selftest_act_derivative_f64(int act, double z) { return act_derivative_f64(act, z); }

} // extern "C"
