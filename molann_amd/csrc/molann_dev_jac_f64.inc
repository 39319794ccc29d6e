// molann_dev_jac_f64.inc - part of libmolann_hip.so, included by molann_kernels.hip after molann_dev_vjp_f64.inc, whose device
// functions it calls.  Float64 values and the full Jacobian dy/dx in one launch (molann_value_and_jacobian_f64 launches it).
namespace {

// =============================================================================================
// frames_value_jac_f64_kernel<G>: x[N, n_inp, 3] -> y[N, d_out] (frames_value_vjp_f64_kernel's, bit for bit) and
// jac[N, d_out, n_inp, 3], jac[f, k] = d y[f, k] / d x[f], everything in double.  G lanes per frame, grid-stride, as that kernel.
// Steps 1-3 (rotation, features, head forward) are its device functions, run once per frame; everything behind them is linear in
// the cotangent, so the d_out rows come from one pass.  The frame's LDS rows: feat[d_feat], z[sum of the hidden widths], two
// buffers of d_out * max_w (the head forward's two activation rows, then the head Jacobian's ping-pong), rot[d_out][12].
//   4. head Jacobian: z <- act'(z) in place, then one sweep from the last layer: D[k][i] = d y_k / d(input i of the layer), lanes
//      over the (k, i) pairs, j ascending.  The first layer's D is dF[k][:] = d y_k / d feat (the identity without a head).
//   5. (alignment) items (lanes): per output column c of the item (at most 3) the unit backward u_c[j], A_c = sum_j q_j u_c[j]^T
//      and s_c = sum_j u_c[j] R^T; per output k, G_R^k and gsum^k = sum_c dF[k][col + c] (A_c, s_c), group sums, into rot[k].
//      Then B = tr(S) I - S is inverted once (kabsch_rotation_backward_solve_t) and lanes over k turn rot[k] into (G_H^k, cen^k).
//   6. atoms (lanes), KC outputs at a time in registers: the atom walks hv_ptr / hv_list as the VJP kernel's step 6 - an item slot
//      evaluates the item's unit backward once per column and adds dF[k][col + c] u_c R^T to every k of the chunk, an align slot
//      adds G_H^k ref_i - cen^k - and stores its row of jac[f, k] once, zeros for untouched atoms.  No atomics, no zeroing pass,
//      a fixed summation order: the same bits on every run.
// The lanes of a frame exchange data through LDS only inside their own wave: lds_wave_sync() orders it, there is no block barrier.
// Steps 4 and 5 and one atom's rows of step 6 are the device functions below, shared with frames_value_metric_f64_kernel
// (molann_dev_metric_f64.inc).
// =============================================================================================
struct JacF64Args {
    long n_frames;
    int n_inp, n_align, n_items, d_feat, d_out;
    int max_w, z_w;            // the widest layer input, the sum of the hidden widths
    int lds_per_frame;         // in doubles
};

constexpr int JAC64_KC = 8;    // outputs an atom accumulates in registers per walk of its list

// d y_k / d feat[col]: the head Jacobian's row in LDS, the identity without a head
__device__ __forceinline__ double jac_df(const double* dF, int d_feat, int k, int col) { return dF ? dF[(long)k * d_feat + col] : (k == col ? 1.0 : 0.0); }

// ---- 4. head Jacobian: act'(z) in place, then the sweep from the last layer; returns dF (in buf0 or buf1)
template <int G>
__device__ __forceinline__ const double* frame_head_jacobian_f64(const F64Mlp& m, int d_out, int z_w, int gl, double* zrows, double* buf0, double* buf1) {
    for (int i = gl; i < z_w; i += G) zrows[i] = act_derivative_f64(m.act, zrows[i]);
    lds_wave_sync();
    const double* dz = zrows + z_w;   // past the last hidden layer's act'(z)
    const double* D = nullptr;
    double* Dn = buf0;
    for (int l = m.n_layers - 1; l >= 0; --l) {
        const int K = m.dims[l], J = m.dims[l + 1];
        const double* Wl = m.W[l];
        if (l > 0) dz -= K;
        const int total = d_out * K;
        for (int e = gl; e < total; e += G) {
            const int k = e / K, i = e - k * K;
            double acc;
            if (D) {
                acc = 0.;
                for (int j = 0; j < J; ++j) acc = fma(Wl[(long)j * K + i], D[k * J + j], acc);
            } else {
                acc = Wl[e];                    // the last layer: d y_k / d(its input i) = W[k][i]
            }
            Dn[e] = l > 0 ? acc * dz[i] : acc;
        }
        lds_wave_sync();
        D = Dn;
        Dn = Dn == buf0 ? buf1 : buf0;
    }
    return D;
}

// ---- 5. the rotation's backward of every output: rot[k] = (G_H^k, cen^k)
template <int G>
__device__ __forceinline__ void frame_rotation_backward_f64(const double* __restrict__ xf, const ItemDev* __restrict__ items,
                                                            const double* __restrict__ ref64, const JacF64Args& a, int gl, V3d c,
                                                            const double (&h)[9], const double (&R)[9], const double* dF, double* rot) {
    for (int base = 0; base < a.n_items; base += G) {
        const int it = base + gl;
        double A[3][12];
#pragma unroll
        for (int cc = 0; cc < 3; ++cc)
#pragma unroll
            for (int i = 0; i < 12; ++i) A[cc][i] = 0.;
        int col = 0, w = 0;
        if (it < a.n_items) {
            const ItemDev d = items[it];
            col = d.col;
            w = item_width(d.type);
            const int na = item_atoms(d.type);
            V3d q[4], y[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) { q[j] = load_atom_f64(xf, d.idx[j]) - c; y[j] = rotate(q[j], R); }
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) {
                if (cc < w) {
                    V3d u[4];
                    item_unit_backward_f64(d.type, y[0], y[1], y[2], y[3], cc, u);
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        if (j < na) { // y = q R :  G_R += q^T u ,  g_p = u R^T
                            const V3d g = u[j];
                            A[cc][0] = fma(q[j].x, g.x, A[cc][0]); A[cc][1] = fma(q[j].x, g.y, A[cc][1]); A[cc][2] = fma(q[j].x, g.z, A[cc][2]);
                            A[cc][3] = fma(q[j].y, g.x, A[cc][3]); A[cc][4] = fma(q[j].y, g.y, A[cc][4]); A[cc][5] = fma(q[j].y, g.z, A[cc][5]);
                            A[cc][6] = fma(q[j].z, g.x, A[cc][6]); A[cc][7] = fma(q[j].z, g.y, A[cc][7]); A[cc][8] = fma(q[j].z, g.z, A[cc][8]);
                            const V3d gp = rotate_back(g, R);
                            A[cc][9] += gp.x; A[cc][10] += gp.y; A[cc][11] += gp.z;
                        }
                    }
                }
            }
        }
        for (int k = 0; k < a.d_out; ++k) {
            const double w0 = w > 0 ? jac_df(dF, a.d_feat, k, col) : 0.0;
            const double w1 = w > 1 ? jac_df(dF, a.d_feat, k, col + 1) : 0.0;
            const double w2 = w > 2 ? jac_df(dF, a.d_feat, k, col + 2) : 0.0;
            double t[12];
#pragma unroll
            for (int i = 0; i < 12; ++i) t[i] = group_sum<G>(fma(w2, A[2][i], fma(w1, A[1][i], w0 * A[0][i])));
            if (gl == 0) {
                double* r = rot + 12 * k;
#pragma unroll
                for (int i = 0; i < 12; ++i) r[i] = base == 0 ? t[i] : r[i] + t[i];
            }
        }
    }
    lds_wave_sync();
    double Binv[7];
    kabsch_rotation_backward_solve_t<double, double>(h, R, Binv);
    const double inv_a = 1.0 / (double)a.n_align;
    const double srx = ref64[3 * a.n_align], sry = ref64[3 * a.n_align + 1], srz = ref64[3 * a.n_align + 2];
    for (int k = gl; k < a.d_out; k += G) {
        double* r = rot + 12 * k;
        double GR[9], GH[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) GR[i] = r[i];
        kabsch_rotation_backward_apply_t<double, double>(R, Binv, GR, GH);
        // H = sum_i (a_i - c) ref_i^T also depends on c through every p_i: - G_H (sum_j ref_j) / a per align atom
        const V3d t = mat_ref(GH, srx, sry, srz);
        const V3d cen = v3d(inv_a * (r[9] + t.x), inv_a * (r[10] + t.y), inv_a * (r[11] + t.z));
#pragma unroll
        for (int i = 0; i < 9; ++i) r[i] = GH[i];
        r[9] = cen.x; r[10] = cen.y; r[11] = cen.z;
    }
    lds_wave_sync();
}

// ---- 6. one atom's rows of the outputs k0 .. k0 + NK - 1 (those below d_out; the others stay zero): one walk of its entries
// e0 .. e1 - 1 of hv_list, the terms in plan order.  NK = JAC64_KC, or fewer where a caller has no registers for more.
template <int NK>
__device__ __forceinline__ void atom_rows_f64(const double* __restrict__ xf, const ItemDev* __restrict__ items, const double* __restrict__ ref64,
                                              const int* __restrict__ hv_list, int e0, int e1, int k0, int d_out, int d_feat, bool has_align, V3d c,
                                              const double (&R)[9], const double* dF, const double* rot, V3d (&acc)[NK]) {
#pragma unroll
    for (int kk = 0; kk < NK; ++kk) acc[kk] = v3d(0., 0., 0.);
    for (int e = e0; e < e1; ++e) {
        const int code = hv_list[e];
        if (code < 0) {
            const int i = -code - 1;
            const double rx = ref64[3 * i], ry = ref64[3 * i + 1], rz = ref64[3 * i + 2];
#pragma unroll
            for (int kk = 0; kk < NK; ++kk) {
                if (k0 + kk < d_out) {
                    const double* r = rot + 12 * (k0 + kk);
                    const double GH[9] = {r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8]};
                    acc[kk] = acc[kk] + (mat_ref(GH, rx, ry, rz) - v3d(r[9], r[10], r[11]));
                }
            }
        } else {
            const ItemDev d = items[code >> 2];
            const int j = code & 3;
            const int w = item_width(d.type);
            V3d y[4];
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                y[jj] = load_atom_f64(xf, d.idx[jj]);
                if (has_align) y[jj] = rotate(y[jj] - c, R);
            }
            V3d uc[3];
#pragma unroll
            for (int cc = 0; cc < 3; ++cc) {
                uc[cc] = v3d(0., 0., 0.);
                if (cc < w) {
                    V3d u[4];
                    item_unit_backward_f64(d.type, y[0], y[1], y[2], y[3], cc, u);
                    V3d t = u[3];   // slot j (selects, not an indexed load: u stays in registers)
                    if (j == 2) t = u[2];
                    if (j == 1) t = u[1];
                    if (j == 0) t = u[0];
                    uc[cc] = has_align ? rotate_back(t, R) : t;
                }
            }
#pragma unroll
            for (int kk = 0; kk < NK; ++kk) {
                if (k0 + kk < d_out) {
                    const int k = k0 + kk;
                    const double w0 = jac_df(dF, d_feat, k, d.col);
                    const double w1 = w > 1 ? jac_df(dF, d_feat, k, d.col + 1) : 0.0;
                    const double w2 = w > 2 ? jac_df(dF, d_feat, k, d.col + 2) : 0.0;
                    acc[kk] = acc[kk] + v3d(fma(w2, uc[2].x, fma(w1, uc[1].x, w0 * uc[0].x)), fma(w2, uc[2].y, fma(w1, uc[1].y, w0 * uc[0].y)),
                                            fma(w2, uc[2].z, fma(w1, uc[1].z, w0 * uc[0].z)));
                }
            }
        }
    }
}

template <int G>
__global__ __launch_bounds__(256) void frames_value_jac_f64_kernel(const double* __restrict__ x, double* __restrict__ out, double* __restrict__ jac,
                                                                   const int* __restrict__ align_idx, const double* __restrict__ ref64,
                                                                   const ItemDev* __restrict__ items, const int* __restrict__ hv_ptr,
                                                                   const int* __restrict__ hv_list, JacF64Args a, F64Mlp m) {
    static_assert(G == 8 || G == 16 || G == 32 || G == 64, "lane group of 8..64");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int gl = threadIdx.x & (G - 1);
    const int slot = threadIdx.x / G;
    const long per_block = blockDim.x / G;
    const long frame_dw = 3l * a.n_inp;
    const bool has_align = a.n_align > 0;
    const bool has_head = m.n_layers > 0;
    const int dbuf = a.d_out * a.max_w;
    double* feat = (double*)smem + (size_t)slot * a.lds_per_frame;
    double* zrows = feat + a.d_feat;
    double* buf0 = zrows + a.z_w;
    double* buf1 = buf0 + dbuf;
    double* rot = has_head ? buf1 + dbuf : feat;
    for (long f = (long)blockIdx.x * per_block + slot; f < a.n_frames; f += (long)gridDim.x * per_block) {
        const double* xf = x + f * frame_dw;
        double* of = out + f * (long)a.d_out;
        double* jf = jac + f * (long)a.d_out * frame_dw;
        // ---- 1-3. rotation, features, head forward: frames_value_vjp_f64_kernel's
        double R[9] = {1., 0., 0., 0., 1., 0., 0., 0., 1.};
        double h[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.};
        V3d c = v3d(0., 0., 0.);
        if (has_align) frame_rotation_f64<G>(xf, align_idx, ref64, a.n_align, gl, c, h, R);
        frame_features_f64<G>(xf, items, a.n_items, gl, has_align, c, R, has_head ? feat : of);
        const double* dF = nullptr;
        if (has_head) {
            lds_wave_sync();
            frame_head_forward_f64<G>(m, gl, feat, zrows, buf0, buf1, of);
            dF = frame_head_jacobian_f64<G>(m, a.d_out, a.z_w, gl, zrows, buf0, buf1);
        }
        if (has_align) frame_rotation_backward_f64<G>(xf, items, ref64, a, gl, c, h, R, dF, rot);
        // ---- 6. atoms (lanes): every row of every jac[f, k] once
        for (int atom = gl; atom < a.n_inp; atom += G) {
            const int e0 = hv_ptr[atom], e1 = hv_ptr[atom + 1];
            for (int k0 = 0; k0 < a.d_out; k0 += JAC64_KC) {
                V3d acc[JAC64_KC];
                atom_rows_f64(xf, items, ref64, hv_list, e0, e1, k0, a.d_out, a.d_feat, has_align, c, R, dF, rot, acc);
#pragma unroll
                for (int kk = 0; kk < JAC64_KC; ++kk) {
                    if (k0 + kk < a.d_out) {
                        double* row = jf + (long)(k0 + kk) * frame_dw + 3l * atom;
                        row[0] = acc[kk].x;
                        row[1] = acc[kk].y;
                        row[2] = acc[kk].z;
                    }
                }
            }
        }
        if (a.lds_per_frame > 0) lds_wave_sync();   // the next frame's rows are this frame's
    }
}

} // namespace
