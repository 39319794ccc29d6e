// molann_dev_hvp.inc - part of libmolann_hip.so, included by molann_kernels.hip (one translation unit: the kernels' host stubs and the
// launches that use them must see each other).  The second order of the feature stage: the derivative of the float64 backward
// J(x)^T g along a direction u, for create_graph=True through the float64 features (molann_hvp.inc launches it).
namespace {

// =============================================================================================
// frames_hvp_kernel<G>: x[N, n_inp, 3], g[N, d_feat], u[N, n_inp, 3] -> hx[N, n_inp, 3] = d/dx <u, J(x)^T g>
// (= sum_k g_k Hess f_k(x) u) and hg[N, d_feat] = J(x) u, everything in double.  G lanes per frame (8/16/32: 8/4/2 frames per
// wave; 64: one wave per frame), grid-stride, as frames_jvp_kernel.  Per frame:
//   0. s = a power of two with |u| / s in [0.5, 1): the work runs on u / s and the stores multiply by s (exact), so a tiny or
//      huge u gives the same digits as a unit one - no underflow into subnormals in the products of tangents.
//   1. bond / angle / dihedral items (lanes): hg from eval_item_tangent_t (the JVP kernel's formulas) on the input coordinates.
//   2. (plans with position items and an alignment) c, H, R as frames_f64_kernel; dc, dH and dR = kabsch_rotation_tangent_t.
//   3. position items (lanes): hg; G_R += q g^T, dG_R += dq g^T (q = p - c), and the tangent of the centroid's share, sum dR g.
//   4. (rotation) group sums; G_H, dG_H = kabsch_rotation_backward_tangent_t(H, R, G_R; dH, dR, dG_R).
//   5. (rotation) atoms (lanes): a position item's slot adds dR g (the tangent of g_p = R g); an align slot i adds
//      dG_H ref_i - (sum dR g + dG_H sum ref) / n_align, the derivative of the backward's centring terms (sum ref is not
//      exactly zero in double, see frames_bwd_f64_kernel).  The row is stored.
//   6. atoms (lanes): a bond / angle / dihedral slot adds the tangent of eval_item_backward on the INPUT coordinates (these
//      items are invariant under rigid motion, so that is their whole Hessian; recomputed per atom of the item), to the row of
//      step 5, which the same lane wrote.
//   Steps 5 and 6 walk the plan-time list hv_ptr / hv_list (4 it + j: slot j of item it; -(i + 1): align slot i), so each atom
//   adds up its own terms in a fixed order and stores its row once: no atomics, the same bits on every run.  The order of the
//   steps keeps the rotation's state dead while the items' dual-number backward runs (no scratch, 244-248 VGPRs).
// =============================================================================================
struct HvpArgs {
    long n_frames;
    int n_inp, n_align, n_items, out_cols, rot, has_pos;
};

template <int G>
__device__ __forceinline__ double group_max(double v) {
#pragma unroll
    for (int m = G / 2; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, 64));
    return v;
}

// dG_H ref_i, G = a row-major 3x3 matrix
__device__ __forceinline__ V3d mat_ref(const double (&M)[9], double rx, double ry, double rz) {
    return v3d(fma(M[2], rz, fma(M[1], ry, M[0] * rx)), fma(M[5], rz, fma(M[4], ry, M[3] * rx)), fma(M[8], rz, fma(M[7], ry, M[6] * rx)));
}

template <int G>
__global__ __launch_bounds__(256) void frames_hvp_kernel(const double* __restrict__ x, const double* __restrict__ gin,
                                                         const double* __restrict__ u, double* __restrict__ hx, double* __restrict__ hg,
                                                         const int* __restrict__ align_idx, const double* __restrict__ ref64,
                                                         const ItemDev* __restrict__ items, const int* __restrict__ hv_ptr,
                                                         const int* __restrict__ hv_list, HvpArgs a) {
    static_assert(G == 8 || G == 16 || G == 32 || G == 64, "lane group of 8..64");
    const int lane = threadIdx.x & 63;
    const int gl = lane & (G - 1);
    const long per_block = (long)(blockDim.x >> 6) * (64 / G);
    const long frame_dw = 3l * a.n_inp;
    for (long f = (long)blockIdx.x * per_block + (threadIdx.x / G); f < a.n_frames; f += (long)gridDim.x * per_block) {
        const double* xf = x + f * frame_dw;
        const double* uf = u + f * frame_dw;
        const double* gf = gin + f * (long)a.out_cols;
        // ---- 0. the frame's scale: a power of two
        double um = 0.;
        for (long k = gl; k < frame_dw; k += G) um = fmax(um, fabs(uf[k]));
        um = group_max<G>(um);
        double su = 1., inv_su = 1.;
        if (um > 0. && um <= 1.7976931348623157e308) {
            // um = m 2^e, m in [0.5, 1) (a subnormal um takes e = -1022, the largest e = 1023: both scales stay finite)
            const int e = min((int)((__double_as_longlong(um) >> 52) & 0x7ff) - 1022, 1023);
            su = ldexp(1., e);
            inv_su = ldexp(1., -e);
        }
        double* hgf = hg + f * (long)a.out_cols;
        double* hxf = hx + f * frame_dw;
        // ---- 1. bond / angle / dihedral items (lanes): hg = J u on the input coordinates (nothing else is live yet)
        for (int it = gl; it < a.n_items; it += G) {
            const ItemDev d = items[it];
            if (d.type == IT_POSITION) continue;
            V3d p[4], dp[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) { p[j] = load_atom_d(xf, d.idx[j]); dp[j] = inv_su * load_atom_d(uf, d.idx[j]); }
            double fv[3], val[3];
            const int w = eval_item_tangent_t<double>(d.type, p[0], p[1], p[2], p[3], dp[0], dp[1], dp[2], dp[3], fv, val);
            hgf[d.col] = su * val[0];
            if (w > 1) hgf[d.col + 1] = su * val[1];
        }
        // ---- 2. (rotation) centre, covariance, rotation and their tangents
        double R[9] = {1., 0., 0., 0., 1., 0., 0., 0., 1.};
        double h[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.};
        double dR[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.};
        double dh[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.};
        V3d c = v3d(0., 0., 0.), dc = v3d(0., 0., 0.);
        if (a.rot) {
            double s[6] = {0., 0., 0., 0., 0., 0.};
            for (int i = gl; i < a.n_align; i += G) {
                const V3d p = load_atom_d(xf, align_idx[i]);
                s[0] += p.x; s[1] += p.y; s[2] += p.z;
            }
            const double inv_a = 1.0 / (double)a.n_align;
            c = v3d(group_sum<G>(s[0]) * inv_a, group_sum<G>(s[1]) * inv_a, group_sum<G>(s[2]) * inv_a);
            double g2 = 0.;
            for (int i = gl; i < a.n_align; i += G) {
                const double rx = ref64[3 * i], ry = ref64[3 * i + 1], rz = ref64[3 * i + 2];
                const int k = align_idx[i];
                const V3d p = load_atom_d(xf, k) - c;
                const V3d d = inv_su * load_atom_d(uf, k);
                g2 = fma(p.x, p.x, fma(p.y, p.y, fma(p.z, p.z, g2)));
                h[0] = fma(p.x, rx, h[0]); h[1] = fma(p.x, ry, h[1]); h[2] = fma(p.x, rz, h[2]);
                h[3] = fma(p.y, rx, h[3]); h[4] = fma(p.y, ry, h[4]); h[5] = fma(p.y, rz, h[5]);
                h[6] = fma(p.z, rx, h[6]); h[7] = fma(p.z, ry, h[7]); h[8] = fma(p.z, rz, h[8]);
                dh[0] = fma(d.x, rx, dh[0]); dh[1] = fma(d.x, ry, dh[1]); dh[2] = fma(d.x, rz, dh[2]);
                dh[3] = fma(d.y, rx, dh[3]); dh[4] = fma(d.y, ry, dh[4]); dh[5] = fma(d.y, rz, dh[5]);
                dh[6] = fma(d.z, rx, dh[6]); dh[7] = fma(d.z, ry, dh[7]); dh[8] = fma(d.z, rz, dh[8]);
                s[3] += d.x; s[4] += d.y; s[5] += d.z;
            }
            g2 = group_sum<G>(g2);
#pragma unroll
            for (int i = 0; i < 9; ++i) { h[i] = group_sum<G>(h[i]); dh[i] = group_sum<G>(dh[i]); }
            dc = v3d(group_sum<G>(s[3]) * inv_a, group_sum<G>(s[4]) * inv_a, group_sum<G>(s[5]) * inv_a);
            kabsch_rotation_t<double, double>(h, 0.5 * (g2 + ref64[3 * a.n_align + 3]) * 1.0001, R);
            // dH = sum du ref^T - dc (sum ref)^T
            const double srx = ref64[3 * a.n_align], sry = ref64[3 * a.n_align + 1], srz = ref64[3 * a.n_align + 2];
            dh[0] -= dc.x * srx; dh[1] -= dc.x * sry; dh[2] -= dc.x * srz;
            dh[3] -= dc.y * srx; dh[4] -= dc.y * sry; dh[5] -= dc.y * srz;
            dh[6] -= dc.z * srx; dh[7] -= dc.z * sry; dh[8] -= dc.z * srz;
            kabsch_rotation_tangent_t<double>(h, R, dh, dR);
        }
        // ---- 3. position items (lanes): hg, and what they give the rotation's backward
        double GR[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.}, dGR[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.};
        V3d dgs = v3d(0., 0., 0.);
        if (a.has_pos) {
            for (int it = gl; it < a.n_items; it += G) {
                const ItemDev d = items[it];
                if (d.type != IT_POSITION) continue;
                V3d dy = inv_su * load_atom_d(uf, d.idx[0]);
                if (a.rot) {
                    const V3d q = load_atom_d(xf, d.idx[0]) - c, dq = dy - dc;
                    dy = rotate(dq, R) + rotate(q, dR);
                    const double g0 = gf[d.col], g1 = gf[d.col + 1], g2 = gf[d.col + 2];
                    // y = q R: G_R += q g^T, and its tangent dq g^T; g_p = R g goes to the centroid: its tangent dR g
                    GR[0] = fma(q.x, g0, GR[0]); GR[1] = fma(q.x, g1, GR[1]); GR[2] = fma(q.x, g2, GR[2]);
                    GR[3] = fma(q.y, g0, GR[3]); GR[4] = fma(q.y, g1, GR[4]); GR[5] = fma(q.y, g2, GR[5]);
                    GR[6] = fma(q.z, g0, GR[6]); GR[7] = fma(q.z, g1, GR[7]); GR[8] = fma(q.z, g2, GR[8]);
                    dGR[0] = fma(dq.x, g0, dGR[0]); dGR[1] = fma(dq.x, g1, dGR[1]); dGR[2] = fma(dq.x, g2, dGR[2]);
                    dGR[3] = fma(dq.y, g0, dGR[3]); dGR[4] = fma(dq.y, g1, dGR[4]); dGR[5] = fma(dq.y, g2, dGR[5]);
                    dGR[6] = fma(dq.z, g0, dGR[6]); dGR[7] = fma(dq.z, g1, dGR[7]); dGR[8] = fma(dq.z, g2, dGR[8]);
                    dgs = dgs + mat_ref(dR, g0, g1, g2);
                }
                hgf[d.col] = su * dy.x;
                hgf[d.col + 1] = su * dy.y;
                hgf[d.col + 2] = su * dy.z;
            }
        }
        if (a.rot) {
            // ---- 4. the rotation's backward and its tangent; the centroid's share
#pragma unroll
            for (int i = 0; i < 9; ++i) { GR[i] = group_sum<G>(GR[i]); dGR[i] = group_sum<G>(dGR[i]); }
            dgs = v3d(group_sum<G>(dgs.x), group_sum<G>(dgs.y), group_sum<G>(dgs.z));
            double GH[9], dGH[9];
            kabsch_rotation_backward_tangent_t<double>(h, R, GR, dh, dR, dGR, GH, dGH);
            const double inv_a = 1.0 / (double)a.n_align;
            const double srx = ref64[3 * a.n_align], sry = ref64[3 * a.n_align + 1], srz = ref64[3 * a.n_align + 2];
            const V3d t = mat_ref(dGH, srx, sry, srz);
            const V3d dcen = v3d(inv_a * (dgs.x + t.x), inv_a * (dgs.y + t.y), inv_a * (dgs.z + t.z));
            // ---- 5. atoms (lanes): the rotation's terms in plan order - dR g per position item, dG_H ref_i - dcen per align slot
            for (int k = gl; k < a.n_inp; k += G) {
                V3d acc = v3d(0., 0., 0.);
                const int e1 = hv_ptr[k + 1];
                for (int e = hv_ptr[k]; e < e1; ++e) {
                    const int code = hv_list[e];
                    if (code < 0) {
                        const int i = -code - 1;
                        acc = acc + (mat_ref(dGH, ref64[3 * i], ref64[3 * i + 1], ref64[3 * i + 2]) - dcen);
                    } else {
                        const ItemDev d = items[code >> 2];
                        if (d.type == IT_POSITION) acc = acc + mat_ref(dR, gf[d.col], gf[d.col + 1], gf[d.col + 2]);
                    }
                }
                hxf[3 * k] = acc.x;
                hxf[3 * k + 1] = acc.y;
                hxf[3 * k + 2] = acc.z;
            }
        }
        // ---- 6. atoms (lanes): the bond / angle / dihedral slots in plan order, added to step 5's row (the same lane wrote it),
        // one store per row.  Every item's Hessian term is that of the input coordinates (they are invariant under rigid motion).
        for (int k = gl; k < a.n_inp; k += G) {
            V3d acc = a.rot ? v3d(hxf[3 * k], hxf[3 * k + 1], hxf[3 * k + 2]) : v3d(0., 0., 0.);
            const int e1 = hv_ptr[k + 1];
            for (int e = hv_ptr[k]; e < e1; ++e) {
                const int code = hv_list[e];
                if (code < 0) continue;
                const ItemDev d = items[code >> 2];
                if (d.type == IT_POSITION) continue;
                const int j = code & 3;
                V3d p[4], dp[4], ga[4], dga[4];
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    p[m] = load_atom_d(xf, d.idx[m]);
                    dp[m] = inv_su * load_atom_d(uf, d.idx[m]);
                    ga[m] = v3d(0., 0., 0.);
                    dga[m] = v3d(0., 0., 0.);
                }
                const double g3[3] = {gf[d.col], d.type == IT_DIHEDRAL_CS ? gf[d.col + 1] : 0.0, 0.0};
                const double dg3[3] = {0., 0., 0.};
                eval_item_backward_tangent_t<double>(d.type, p[0], p[1], p[2], p[3], dp[0], dp[1], dp[2], dp[3], g3, dg3, ga, dga);
                V3d t = dga[3];   // slot j (selects, not an indexed load: dga stays in registers)
                if (j == 2) t = dga[2];
                if (j == 1) t = dga[1];
                if (j == 0) t = dga[0];
                acc = acc + t;
            }
            hxf[3 * k] = su * acc.x;
            hxf[3 * k + 1] = su * acc.y;
            hxf[3 * k + 2] = su * acc.z;
        }
    }
}

} // namespace
