// molann_metric_f64.inc - part of libmolann_hip.so, included by molann_kernels.hip after molann_jac_f64.inc.  Float64 values and
// the metric tensor J W J^T in one launch: molann_value_and_metric_f64 (see include/molann_hip.h) and its launch of
// frames_value_metric_f64_kernel (molann_dev_metric_f64.inc).
namespace {

// the widest output the kernel's chunk pairs serve: d_out / JAC64_KC chunks, every pair of them a pass over the frame's atoms
constexpr int METRIC64_MAX_D_OUT = 64;

// The frame's LDS rows are the Jacobian kernel's (jac64_rows: the accumulators of a chunk pair live in registers), and so is the
// lane group; an output wider than METRIC64_MAX_D_OUT is refused.
inline Vjp64Geom metric64_geometry(const molann_plan* p) {
    Vjp64Geom g = jac64_geometry(p);
    const int d_out = p->n_layers > 0 ? p->dims[p->n_layers] : p->d_feat;
    if (d_out > METRIC64_MAX_D_OUT) g.ok = false;
    return g;
}

template <int G>
int launch_metric64(const molann_plan* p, const Vjp64Geom& g, int grid, hipStream_t s, const double* x, double* out, double* metric,
                    const double* atom_w, const JacF64Args& a, const F64Mlp& m) {
    if (g.lds > VJP64_LDS_DEFAULT) {   // one wave, one frame, more than a launch may ask for by default: raise the kernel's limit
        const hipError_t e = hipFuncSetAttribute((const void*)frames_value_metric_f64_kernel<G>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL((frames_value_metric_f64_kernel<G>), dim3(grid), dim3(g.block), g.lds, s, x, out, metric, atom_w, p->d_align_idx, p->d_ref64,
                       p->d_items, p->d_hv_ptr, p->d_hv_list, a, m);
    return (int)hipGetLastError();
}

} // namespace

extern "C" {

int molann_plan_supports_value_and_metric_f64(const molann_plan* p) {
    if (!p) return MOLANN_E_NULL;
    return metric64_geometry(p).ok ? 1 : 0;
}

int molann_value_and_metric_f64(molann_plan* p, const double* x, int64_t n, const double* const* W, const double* const* b, const double* atom_w,
                                double* out, double* metric, molann_stream_t stream) {
    if (!p) return MOLANN_E_NULL;
    if (n < 0) return MOLANN_E_DESC;
    if (n == 0) return MOLANN_OK;
    if (!x || !out || !metric) return MOLANN_E_NULL;
    if ((((uintptr_t)x) & 7) || (((uintptr_t)metric) & 7) || (((uintptr_t)out) & 7) || (((uintptr_t)atom_w) & 7)) return MOLANN_E_ALIGNMENT;
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
    const Vjp64Geom g = metric64_geometry(p);
    if (!g.ok) return MOLANN_E_UNSUPPORTED;
    JacF64Args a;
    a.n_frames = (long)n;
    a.n_inp = p->n_inp; a.n_align = p->n_align; a.n_items = p->n_items; a.d_feat = p->d_feat;
    a.d_out = p->n_layers > 0 ? p->dims[p->n_layers] : p->d_feat;
    jac64_rows(p, a.max_w, a.z_w, a.lds_per_frame);
    m.max_w = a.max_w;
    const int grid = grid_for(p, (long)n, g.block / g.G, 8);
    hipStream_t s = (hipStream_t)stream;
    int rc;
    switch (g.G) {
    case 8: rc = launch_metric64<8>(p, g, grid, s, x, out, metric, atom_w, a, m); break;
    case 16: rc = launch_metric64<16>(p, g, grid, s, x, out, metric, atom_w, a, m); break;
    case 32: rc = launch_metric64<32>(p, g, grid, s, x, out, metric, atom_w, a, m); break;
    default: rc = launch_metric64<64>(p, g, grid, s, x, out, metric, atom_w, a, m); break;
    }
    snprintf(p->last_info, sizeof(p->last_info), "frames_value_metric_f64_kernel (values + metric in one launch; %d lanes per frame) grid=%d block=%d lds=%d",
             g.G, grid, g.block, (int)g.lds);
    return rc;
}

} // extern "C"
