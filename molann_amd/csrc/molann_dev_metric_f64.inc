// molann_dev_metric_f64.inc - part of libmolann_hip.so, included by molann_kernels.hip after molann_dev_jac_f64.inc, whose device
// functions it calls.  Float64 values and the metric tensor J W J^T in one launch (molann_value_and_metric_f64 launches it).
namespace {

// =============================================================================================
// frames_value_metric_f64_kernel<G>: x[N, n_inp, 3] -> y[N, d_out] (frames_value_jac_f64_kernel's, bit for bit) and
// metric[N, d_out, d_out], metric[f, k, l] = sum_a w_a grad_a y_k(x_f) . grad_a y_l(x_f), everything in double; atom_w holds the
// n_inp weights w_a, or is null for all ones (the same bits as a tensor of ones: the product with 1.0 is still made).
// G lanes per frame, grid-stride, the frame's LDS rows and steps 1-5 as frames_value_jac_f64_kernel (its device functions), then
//   6'. per block of output pairs - a chunk of JAC64_KC outputs with itself (k <= l: 36 pairs), then with every later strip of
//       METRIC64_KH outputs (8 x 2 pairs) - atoms (lanes): an atom in no item and no alignment set is skipped, a touched one
//       evaluates its rows g_k of the chunk (and g_l of the strip: atom_rows_f64, the Jacobian kernel's walk) and adds
//       w_a (g_k . g_l) to its own accumulators; after the atoms every accumulator is totalled
//       over the frame's lanes (group_sum's xor butterfly: every lane holds the same bits) and one lane stores metric[f, k, l] and
//       metric[f, l, k] from the same value.  d_out <= JAC64_KC is one block: one walk per atom, 36 accumulators.
// The Jacobian is never stored.  No atomics, no zeroing pass, a fixed summation order: the same bits on every run, and a metric
// that is symmetric bit for bit.
// =============================================================================================
// Outputs per strip off the diagonal.  The rows of a chunk, the accumulators and the walk's own registers are live together: with 8 x 8
// accumulators the kernel spills 184 bytes per lane to scratch, with 8 x 4 still 60-76, with 8 x 3 none at 254 of the 256 AGPRs, with
// 8 x 2 none at 238.
constexpr int METRIC64_KH = 2;

template <int G>
__global__ __launch_bounds__(256) void frames_value_metric_f64_kernel(const double* __restrict__ x, double* __restrict__ out,
                                                                      double* __restrict__ metric, const double* __restrict__ atom_w,
                                                                      const int* __restrict__ align_idx, const double* __restrict__ ref64,
                                                                      const ItemDev* __restrict__ items, const int* __restrict__ hv_ptr,
                                                                      const int* __restrict__ hv_list, JacF64Args a, F64Mlp m) {
    static_assert(G == 8 || G == 16 || G == 32 || G == 64, "lane group of 8..64");
    constexpr int KC = JAC64_KC, KH = METRIC64_KH;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int gl = threadIdx.x & (G - 1);
    const int slot = threadIdx.x / G;
    const long per_block = blockDim.x / G;
    const long frame_dw = 3l * a.n_inp;
    const bool has_align = a.n_align > 0;
    const bool has_head = m.n_layers > 0;
    const int dbuf = a.d_out * a.max_w;
    const int n_chunks = (a.d_out + KC - 1) / KC;
    double* feat = (double*)smem + (size_t)slot * a.lds_per_frame;
    double* zrows = feat + a.d_feat;
    double* buf0 = zrows + a.z_w;
    double* buf1 = buf0 + dbuf;
    double* rot = has_head ? buf1 + dbuf : feat;
    for (long f = (long)blockIdx.x * per_block + slot; f < a.n_frames; f += (long)gridDim.x * per_block) {
        const double* xf = x + f * frame_dw;
        double* of = out + f * (long)a.d_out;
        double* mf = metric + f * (long)a.d_out * a.d_out;
        // ---- 1-5. frames_value_jac_f64_kernel's
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
        // ---- 6'. the contraction over the atoms, a block of output pairs at a time
        for (int p = 0; p < n_chunks; ++p) {
            const int kp = p * KC;
            for (int kq = kp; kq < a.d_out; kq += kq == kp ? KC : KH) {
                const bool diag = kq == kp;
                double acc[KC][KC];   // a chunk with itself: [i][j >= i]; with a strip: [i][j < KH]
#pragma unroll
                for (int i = 0; i < KC; ++i)
#pragma unroll
                    for (int j = 0; j < KC; ++j) acc[i][j] = 0.;
                for (int atom = gl; atom < a.n_inp; atom += G) {
                    const int e0 = hv_ptr[atom], e1 = hv_ptr[atom + 1];
                    if (e0 == e1) continue;
                    const double wa = atom_w ? atom_w[atom] : 1.0;
                    V3d gp[KC];
                    atom_rows_f64(xf, items, ref64, hv_list, e0, e1, kp, a.d_out, a.d_feat, has_align, c, R, dF, rot, gp);
                    if (diag) {
#pragma unroll
                        for (int i = 0; i < KC; ++i)
#pragma unroll
                            for (int j = i; j < KC; ++j)
                                acc[i][j] = fma(wa, fma(gp[i].z, gp[j].z, fma(gp[i].y, gp[j].y, gp[i].x * gp[j].x)), acc[i][j]);
                    } else {
                        V3d gq[KH];
                        atom_rows_f64(xf, items, ref64, hv_list, e0, e1, kq, a.d_out, a.d_feat, has_align, c, R, dF, rot, gq);
#pragma unroll
                        for (int i = 0; i < KC; ++i)
#pragma unroll
                            for (int j = 0; j < KH; ++j)
                                acc[i][j] = fma(wa, fma(gp[i].z, gq[j].z, fma(gp[i].y, gq[j].y, gp[i].x * gq[j].x)), acc[i][j]);
                    }
                }
#pragma unroll
                for (int i = 0; i < KC; ++i) {
#pragma unroll
                    for (int j = 0; j < KC; ++j) {
                        const int k = kp + i, l = kq + j;
                        if ((diag ? j >= i : j < KH) && l < a.d_out) {   // k <= l < d_out: the same for every lane
                            const double t = group_sum<G>(acc[i][j]);
                            if (gl == ((i * KC + j) & (G - 1))) {
                                mf[(long)k * a.d_out + l] = t;
                                mf[(long)l * a.d_out + k] = t;
                            }
                        }
                    }
                }
            }
        }
        if (a.lds_per_frame > 0) lds_wave_sync();   // the next frame's rows are this frame's
    }
}

} // namespace
