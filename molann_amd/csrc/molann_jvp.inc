// molann_jvp.inc - part of libmolann_hip.so, included by molann_kernels.hip after molann_capi.inc.  The forward-mode entry points
// (molann_features_jvp_f32 / _f64, see include/molann_hip.h) and their launches of frames_jvp_kernel (molann_dev_jvp.inc).
namespace {

// lanes per frame: the smallest group that covers the items - and the align atoms where the rotation is needed (position items)
// - in one round (8/4/2 frames per wave), a whole wave from 33 on
inline int jvp_group(const molann_plan* p) {
    const int work = (p->n_align > 0 && p->has_position_items) ? std::max(p->n_align, p->n_items) : p->n_items;
    return work <= 8 ? 8 : work <= 16 ? 16 : work <= 32 ? 32 : 64;
}

template <typename TI>
int launch_jvp(const molann_plan* cp, const TI* x, const TI* v, int64_t n, int n_tangents, TI* out, TI* tangent_out,
               hipStream_t stream) {
    if (!cp) return MOLANN_E_NULL;
    molann_plan* p = const_cast<molann_plan*>(cp);
    if (p->n_items <= 0) return MOLANN_E_STAGE;
    if (n < 0 || n_tangents < 1) return MOLANN_E_DESC;
    if (n == 0) return MOLANN_OK;
    if (!x || !v || !tangent_out) return MOLANN_E_NULL;
    if ((((uintptr_t)x) & 3) || (((uintptr_t)v) & 3) || (((uintptr_t)out) & 3) || (((uintptr_t)tangent_out) & 3)) return MOLANN_E_ALIGNMENT;
    JvpArgs a;
    a.n_frames = (long)n;
    a.v_tstride = (long)n * 3l * p->n_inp;
    a.f_tstride = (long)n * (long)p->d_feat;
    a.n_inp = p->n_inp; a.n_align = p->n_align; a.n_items = p->n_items; a.out_cols = p->d_feat;
    a.n_tangents = n_tangents;
    a.rot_tangent = (p->n_align > 0 && p->has_position_items) ? 1 : 0;
    const int G = jvp_group(p);
    const int frames_per_block = 4 * (64 / G);
    const int grid = grid_for(p, (long)n, frames_per_block, 8);
    const char* name = sizeof(TI) == 8 ? "frames_jvp_f64_kernel" : "frames_jvp_kernel";
    switch (G) {
    case 8: hipLaunchKernelGGL((frames_jvp_kernel<TI, 8>), dim3(grid), dim3(256), 0, stream, x, v, out, tangent_out, p->d_align_idx, p->d_ref64, p->d_items, a); break;
    case 16: hipLaunchKernelGGL((frames_jvp_kernel<TI, 16>), dim3(grid), dim3(256), 0, stream, x, v, out, tangent_out, p->d_align_idx, p->d_ref64, p->d_items, a); break;
    case 32: hipLaunchKernelGGL((frames_jvp_kernel<TI, 32>), dim3(grid), dim3(256), 0, stream, x, v, out, tangent_out, p->d_align_idx, p->d_ref64, p->d_items, a); break;
    default: hipLaunchKernelGGL((frames_jvp_kernel<TI, 64>), dim3(grid), dim3(256), 0, stream, x, v, out, tangent_out, p->d_align_idx, p->d_ref64, p->d_items, a); break;
    }
    snprintf(p->last_info, sizeof(p->last_info), "%s (%d lanes per frame, %d tangents%s) grid=%d block=256", name, G, n_tangents,
             a.rot_tangent ? ", rotation tangent" : "", grid);
    return (int)hipGetLastError();
}

} // namespace

extern "C" {

int molann_features_jvp_f32(const molann_plan* p, const float* x, const float* v, int64_t n_frames, int n_tangents, float* out,
                            float* tangent_out, molann_stream_t stream) {
    return launch_jvp<float>(p, x, v, n_frames, n_tangents, out, tangent_out, (hipStream_t)stream);
}

int molann_features_jvp_f64(const molann_plan* p, const double* x, const double* v, int64_t n_frames, int n_tangents, double* out,
                            double* tangent_out, molann_stream_t stream) {
    if (p && n_frames > 0 && ((((uintptr_t)x) & 7) || (((uintptr_t)v) & 7) || (((uintptr_t)out) & 7) || (((uintptr_t)tangent_out) & 7)))
        return MOLANN_E_ALIGNMENT;
    return launch_jvp<double>(p, x, v, n_frames, n_tangents, out, tangent_out, (hipStream_t)stream);
}

} // extern "C"
