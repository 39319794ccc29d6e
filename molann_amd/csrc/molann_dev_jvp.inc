// molann_dev_jvp.inc - part of libmolann_hip.so, included by molann_kernels.hip (one translation unit: the kernels' host stubs and the
// launches that use them must see each other).  The forward mode of the feature stage: features f and their tangents
// df = J(x) v for torch.autograd.forward_ad / torch.func.jvp / torch.func.jacfwd (molann_jvp.inc launches them).
namespace {

// =============================================================================================
// frames_jvp_kernel<TI, G>: x[N, n_inp, 3] and n_tangents tangents v[T, N, n_inp, 3] -> f[N, d_feat] (optional) and
// df[T, N, d_feat].  A group of G lanes per frame (G = 8/16/32: 8/4/2 frames per wave on small and mid-size frames, as
// frames_group_bwd_kernel; G = 64: one wave per frame on large frames, as frames_wave_bwd_gather_kernel), grid-stride.
// Everything per frame is computed in double whatever TI is - the centroid and covariance as group sums (butterflies of
// __shfl_xor inside the group: every lane ends with the same bits, no atomics, so the output is identical run to run), the
// rotation by kabsch_rotation_t<double>, the items by eval_item_tangent_t<double> - and rounded once on the store.  The
// tangents of a frame share its one read of x, its one rotation solve and its one f.
//
// Aligned coordinates are y = (p - c) R.  Bond / angle / dihedral items are invariant under rigid motion: their values
// and tangents are those of the INPUT coordinates (no R, no dR; the same numbers in exact arithmetic, as align_item_atoms
// argues for values).  Position items need dy = (dp - dc) R + (p - c) dR with dR = kabsch_rotation_tangent_t(H, R, dH),
// dH = sum_i (dp_i - dc) ref_i^T.  c, R and their tangents are computed only on plans that have position items and an
// alignment (a.rot_tangent); an aligned plan of invariant items reads neither the align atoms nor the reference.
// =============================================================================================
struct JvpArgs {
    long n_frames;
    long v_tstride, f_tstride; // elements between consecutive tangents of v and of df
    int n_inp, n_align, n_items, out_cols, n_tangents, rot_tangent;
};

template <int G>
__device__ __forceinline__ double group_sum(double v) {
#pragma unroll
    for (int m = G / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
    return v;
}

template <typename TI>
__device__ __forceinline__ V3d load_atom_d(const TI* __restrict__ xf, int k) {
    return v3d((double)xf[3 * k], (double)xf[3 * k + 1], (double)xf[3 * k + 2]);
}

template <typename TI, int G>
__global__ __launch_bounds__(256) void frames_jvp_kernel(const TI* __restrict__ x, const TI* __restrict__ v, TI* __restrict__ out,
                                                         TI* __restrict__ tout, const int* __restrict__ align_idx,
                                                         const double* __restrict__ ref64, const ItemDev* __restrict__ items, JvpArgs a) {
    static_assert(G == 8 || G == 16 || G == 32 || G == 64, "lane group of 8..64");
    const int lane = threadIdx.x & 63;
    const int gl = lane & (G - 1);
    const long per_block = (long)(blockDim.x >> 6) * (64 / G);
    const long frame_dw = 3l * a.n_inp;
    const bool has_align = a.n_align > 0;
    for (long f = (long)blockIdx.x * per_block + (threadIdx.x / G); f < a.n_frames; f += (long)gridDim.x * per_block) {
        const TI* xf = x + f * frame_dw;
        double R[9] = {1., 0., 0., 0., 1., 0., 0., 0., 1.};
        double h[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.};
        V3d c = v3d(0., 0., 0.);
        if (a.rot_tangent) {
            // (only position items depend on R: a plan of bond / angle / dihedral items solves nothing)
            // the float64 forward's formulas (frames_f64_kernel): centroid, then H = sum (p - c) ref^T and |p - c|^2
            double sx = 0., sy = 0., sz = 0.;
            for (int i = gl; i < a.n_align; i += G) { const V3d p = load_atom_d(xf, align_idx[i]); sx += p.x; sy += p.y; sz += p.z; }
            const double inv_a = 1.0 / (double)a.n_align;
            c = v3d(group_sum<G>(sx) * inv_a, group_sum<G>(sy) * inv_a, group_sum<G>(sz) * inv_a);
            double g = 0.;
            for (int i = gl; i < a.n_align; i += G) {
                const double rx = ref64[3 * i], ry = ref64[3 * i + 1], rz = ref64[3 * i + 2];
                const V3d p = load_atom_d(xf, align_idx[i]) - c;
                g = fma(p.x, p.x, fma(p.y, p.y, fma(p.z, p.z, g)));
                h[0] = fma(p.x, rx, h[0]); h[1] = fma(p.x, ry, h[1]); h[2] = fma(p.x, rz, h[2]);
                h[3] = fma(p.y, rx, h[3]); h[4] = fma(p.y, ry, h[4]); h[5] = fma(p.y, rz, h[5]);
                h[6] = fma(p.z, rx, h[6]); h[7] = fma(p.z, ry, h[7]); h[8] = fma(p.z, rz, h[8]);
            }
            g = group_sum<G>(g);
#pragma unroll
            for (int i = 0; i < 9; ++i) h[i] = group_sum<G>(h[i]);
            kabsch_rotation_t<double, double>(h, 0.5 * (g + ref64[3 * a.n_align + 3]) * 1.0001, R);
        }
        for (int t = 0; t < a.n_tangents; ++t) {
            const TI* vf = v + (long)t * a.v_tstride + f * frame_dw;
            TI* tf = tout + (long)t * a.f_tstride + f * (long)a.out_cols;
            double dR[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.};
            V3d dc = v3d(0., 0., 0.);
            if (a.rot_tangent) {
                // dc = mean of the align atoms' tangents; dH = sum dp ref^T - dc (sum ref)^T (the packed reference's sum is
                // not exactly zero in double, see frames_bwd_f64_kernel)
                double s[12] = {0., 0., 0., 0., 0., 0., 0., 0., 0., 0., 0., 0.};
                for (int i = gl; i < a.n_align; i += G) {
                    const double rx = ref64[3 * i], ry = ref64[3 * i + 1], rz = ref64[3 * i + 2];
                    const V3d d = load_atom_d(vf, align_idx[i]);
                    s[0] = fma(d.x, rx, s[0]); s[1] = fma(d.x, ry, s[1]); s[2] = fma(d.x, rz, s[2]);
                    s[3] = fma(d.y, rx, s[3]); s[4] = fma(d.y, ry, s[4]); s[5] = fma(d.y, rz, s[5]);
                    s[6] = fma(d.z, rx, s[6]); s[7] = fma(d.z, ry, s[7]); s[8] = fma(d.z, rz, s[8]);
                    s[9] += d.x; s[10] += d.y; s[11] += d.z;
                }
#pragma unroll
                for (int i = 0; i < 12; ++i) s[i] = group_sum<G>(s[i]);
                const double inv_a = 1.0 / (double)a.n_align;
                dc = v3d(s[9] * inv_a, s[10] * inv_a, s[11] * inv_a);
                const double srx = ref64[3 * a.n_align], sry = ref64[3 * a.n_align + 1], srz = ref64[3 * a.n_align + 2];
                double dh[9] = {s[0] - dc.x * srx, s[1] - dc.x * sry, s[2] - dc.x * srz,
                                s[3] - dc.y * srx, s[4] - dc.y * sry, s[5] - dc.y * srz,
                                s[6] - dc.z * srx, s[7] - dc.z * sry, s[8] - dc.z * srz};
                kabsch_rotation_tangent_t<double>(h, R, dh, dR);
            }
            for (int it = gl; it < a.n_items; it += G) {
                const ItemDev d = items[it];
                V3d p[4], dp[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) { p[j] = load_atom_d(xf, d.idx[j]); dp[j] = load_atom_d(vf, d.idx[j]); }
                if (d.type == IT_POSITION && has_align) {
                    const V3d q = p[0] - c;
                    const V3d y = rotate(q, R);
                    const V3d dq = dp[0] - dc;
                    const V3d rq = rotate(dq, R), dRq = rotate(q, dR);
                    p[0] = y;
                    dp[0] = v3d(rq.x + dRq.x, rq.y + dRq.y, rq.z + dRq.z);
                }
                double val[3], dval[3];
                const int w = eval_item_tangent_t<double>(d.type, p[0], p[1], p[2], p[3], dp[0], dp[1], dp[2], dp[3], val, dval);
                tf[d.col] = (TI)dval[0];
                if (w > 1) tf[d.col + 1] = (TI)dval[1];
                if (w > 2) tf[d.col + 2] = (TI)dval[2];
                if (t == 0 && out) {
                    TI* of = out + f * (long)a.out_cols;
                    of[d.col] = (TI)val[0];
                    if (w > 1) of[d.col + 1] = (TI)val[1];
                    if (w > 2) of[d.col + 2] = (TI)val[2];
                }
            }
        }
    }
}

} // namespace
