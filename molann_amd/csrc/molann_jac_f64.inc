// molann_jac_f64.inc - part of libmolann_hip.so, included by molann_kernels.hip after molann_vjp_f64.inc.  Float64 values and the
// full Jacobian in one launch: molann_value_and_jacobian_f64 (see include/molann_hip.h) and its launch of
// frames_value_jac_f64_kernel (molann_dev_jac_f64.inc).
namespace {

// doubles of LDS per frame: with a head the feature row, the hidden layers' act'(z), two buffers of d_out rows of the widest layer
// input (the forward's two activation rows live in them first); with an alignment 12 per output (G_R and gsum, then G_H and cen)
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

inline Vjp64Geom jac64_geometry(const molann_plan* p) {
    int max_w, z_w, per_frame;
    jac64_rows(p, max_w, z_w, per_frame);
    return vjp64_geometry_rows(p, max_w, per_frame);
}

template <int G>
int launch_jac64(const molann_plan* p, const Vjp64Geom& g, int grid, hipStream_t s, const double* x, double* out, double* jac, const JacF64Args& a,
                 const F64Mlp& m) {
    if (g.lds > VJP64_LDS_DEFAULT) {   // one wave, one frame, more than a launch may ask for by default: raise the kernel's limit
        const hipError_t e = hipFuncSetAttribute((const void*)frames_value_jac_f64_kernel<G>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)g.lds);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL((frames_value_jac_f64_kernel<G>), dim3(grid), dim3(g.block), g.lds, s, x, out, jac, p->d_align_idx, p->d_ref64, p->d_items,
                       p->d_hv_ptr, p->d_hv_list, a, m);
    return (int)hipGetLastError();
}

} // namespace

extern "C" {

int molann_plan_supports_value_and_jacobian_f64(const molann_plan* p) {
    if (!p) return MOLANN_E_NULL;
    return jac64_geometry(p).ok ? 1 : 0;
}

int molann_value_and_jacobian_f64(molann_plan* p, const double* x, int64_t n, const double* const* W, const double* const* b, double* out, double* jac,
                                  molann_stream_t stream) {
    if (!p) return MOLANN_E_NULL;
    if (n < 0) return MOLANN_E_DESC;
    if (n == 0) return MOLANN_OK;
    if (!x || !out || !jac) return MOLANN_E_NULL;
    if ((((uintptr_t)x) & 7) || (((uintptr_t)jac) & 7) || (((uintptr_t)out) & 7)) return MOLANN_E_ALIGNMENT;
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
    const Vjp64Geom g = jac64_geometry(p);
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
    case 8: rc = launch_jac64<8>(p, g, grid, s, x, out, jac, a, m); break;
    case 16: rc = launch_jac64<16>(p, g, grid, s, x, out, jac, a, m); break;
    case 32: rc = launch_jac64<32>(p, g, grid, s, x, out, jac, a, m); break;
    default: rc = launch_jac64<64>(p, g, grid, s, x, out, jac, a, m); break;
    }
    snprintf(p->last_info, sizeof(p->last_info), "frames_value_jac_f64_kernel (values + Jacobian in one launch; %d lanes per frame) grid=%d block=%d lds=%d",
             g.G, grid, g.block, (int)g.lds);
    return rc;
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
