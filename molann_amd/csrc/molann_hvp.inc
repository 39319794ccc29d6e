// molann_hvp.inc - part of libmolann_hip.so, included by molann_kernels.hip after molann_capi.inc.  The second-order entry point
// (molann_features_hvp_f64, see include/molann_hip.h) and its launch of frames_hvp_kernel (molann_dev_hvp.inc).
namespace {

// lanes per frame: the smallest group that covers the atoms, the items and - where the rotation is needed - the align atoms in
// one round (8/4/2 frames per wave), a whole wave from 33 on
inline int hvp_group(const molann_plan* p) {
    int work = std::max(p->n_inp, p->n_items);
    if (p->n_align > 0 && p->has_position_items) work = std::max(work, p->n_align);
    return work <= 8 ? 8 : work <= 16 ? 16 : work <= 32 ? 32 : 64;
}

} // namespace

extern "C" {

int molann_features_hvp_f64(const molann_plan* cp, const double* x, const double* g, const double* u, int64_t n, double* hx, double* hg,
                            molann_stream_t stream) {
    if (!cp) return MOLANN_E_NULL;
    molann_plan* p = const_cast<molann_plan*>(cp);
    if (p->n_items <= 0) return MOLANN_E_STAGE;
    if (n < 0) return MOLANN_E_DESC;
    if (n == 0) return MOLANN_OK;
    if (!x || !g || !u || !hx || !hg) return MOLANN_E_NULL;
    if ((((uintptr_t)x) & 7) || (((uintptr_t)g) & 7) || (((uintptr_t)u) & 7) || (((uintptr_t)hx) & 7) || (((uintptr_t)hg) & 7))
        return MOLANN_E_ALIGNMENT;
    HvpArgs a;
    a.n_frames = (long)n;
    a.n_inp = p->n_inp; a.n_align = p->n_align; a.n_items = p->n_items; a.out_cols = p->d_feat;
    a.rot = (p->n_align > 0 && p->has_position_items) ? 1 : 0;
    a.has_pos = p->has_position_items ? 1 : 0;
    const int G = hvp_group(p);
    const int frames_per_block = 4 * (64 / G);
    const int grid = grid_for(p, (long)n, frames_per_block, 8);
    hipStream_t s = (hipStream_t)stream;
    switch (G) {
    case 8: hipLaunchKernelGGL((frames_hvp_kernel<8>), dim3(grid), dim3(256), 0, s, x, g, u, hx, hg, p->d_align_idx, p->d_ref64, p->d_items, p->d_hv_ptr, p->d_hv_list, a); break;
    case 16: hipLaunchKernelGGL((frames_hvp_kernel<16>), dim3(grid), dim3(256), 0, s, x, g, u, hx, hg, p->d_align_idx, p->d_ref64, p->d_items, p->d_hv_ptr, p->d_hv_list, a); break;
    case 32: hipLaunchKernelGGL((frames_hvp_kernel<32>), dim3(grid), dim3(256), 0, s, x, g, u, hx, hg, p->d_align_idx, p->d_ref64, p->d_items, p->d_hv_ptr, p->d_hv_list, a); break;
    default: hipLaunchKernelGGL((frames_hvp_kernel<64>), dim3(grid), dim3(256), 0, s, x, g, u, hx, hg, p->d_align_idx, p->d_ref64, p->d_items, p->d_hv_ptr, p->d_hv_list, a); break;
    }
    snprintf(p->last_info, sizeof(p->last_info), "frames_hvp_f64_kernel (%d lanes per frame%s) grid=%d block=256", G,
             a.rot ? ", rotation tangent" : "", grid);
    return (int)hipGetLastError();
}

int molann_selftest_feature_backward_tangent_f64(int type, int use_angle_value, const double* a, const double* t, const double* g3,
                                                 const double* dg3, double* ga12, double* dga12) {
    if (!a || !t || !g3 || !dg3 || !ga12 || !dga12) return MOLANN_E_NULL;
    const int it = selftest_item_type(type, use_angle_value);
    if (it < 0) return MOLANN_E_FEATURE;
    const double g[3] = {g3[0], g3[1], g3[2]}, dg[3] = {dg3[0], dg3[1], dg3[2]};
    V3d ga[4], dga[4];
    for (int j = 0; j < 4; ++j) { ga[j] = v3d(0., 0., 0.); dga[j] = v3d(0., 0., 0.); }
    eval_item_backward_tangent_t<double>(it, v3d(a[0], a[1], a[2]), v3d(a[3], a[4], a[5]), v3d(a[6], a[7], a[8]), v3d(a[9], a[10], a[11]),
                                         v3d(t[0], t[1], t[2]), v3d(t[3], t[4], t[5]), v3d(t[6], t[7], t[8]), v3d(t[9], t[10], t[11]), g, dg,
                                         ga, dga);
    for (int j = 0; j < 4; ++j) {
        ga12[3 * j] = ga[j].x; ga12[3 * j + 1] = ga[j].y; ga12[3 * j + 2] = ga[j].z;
        dga12[3 * j] = dga[j].x; dga12[3 * j + 1] = dga[j].y; dga12[3 * j + 2] = dga[j].z;
    }
    return item_atoms(it);
}

int molann_selftest_kabsch_backward_tangent(const double* H9, const double* R9, const double* GR9, const double* dH9, const double* dR9,
                                            const double* dGR9, double* GH9, double* dGH9) {
    if (!H9 || !R9 || !GR9 || !dH9 || !dR9 || !dGR9 || !GH9 || !dGH9) return MOLANN_E_NULL;
    double h[9], r[9], gr[9], dh[9], dr[9], dgr[9], gh[9], dgh[9];
    for (int i = 0; i < 9; ++i) { h[i] = H9[i]; r[i] = R9[i]; gr[i] = GR9[i]; dh[i] = dH9[i]; dr[i] = dR9[i]; dgr[i] = dGR9[i]; }
    kabsch_rotation_backward_tangent_t<double>(h, r, gr, dh, dr, dgr, gh, dgh);
    for (int i = 0; i < 9; ++i) { GH9[i] = gh[i]; dGH9[i] = dgh[i]; }
    return MOLANN_OK;
}

} // extern "C"
