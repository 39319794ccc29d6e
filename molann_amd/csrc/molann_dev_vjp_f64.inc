// molann_dev_vjp_f64.inc - part of libmolann_hip.so, included by molann_kernels.hip (one translation unit: the kernels' host stubs and the
// launches that use them must see each other).  Float64 values and forces in one launch (molann_value_and_vjp_f64 launches it).
namespace {

// =============================================================================================
// frames_value_vjp_f64_kernel<G>: x[N, n_inp, 3], grad_out[N, d_out] -> y[N, d_out] = the float64 forward (frames_f64_kernel's
// formulas, then mlp_f64_kernel's fma chains on the caller's torch.nn.Linear tensors) and gx[N, n_inp, 3] = J(x)^T grad_out,
// everything in double.  G lanes per frame (8/16/32: 8/4/2 frames per wave; 64: one wave per frame), grid-stride, as
// frames_hvp_kernel.  Per frame, in the frame's own LDS rows (feat[d_feat], z[sum of the hidden widths], two rows of max_w):
//   1. c, H, R of the alignment atoms (group sums, every lane solves the same rotation).
//   2. items (lanes): the features of the aligned coordinates -> feat (-> y where the plan has no head).
//   3. head forward: lane j computes units j, j + G, ... of a layer as one fma chain over W[j][:]; the hidden layers'
//      pre-activations stay in z, their activations ping-pong between the two rows; the last layer is stored as y.
//   4. head backward for x only (parameters are data): g = grad_out; per layer from the last, lane k sums dh[k] = sum_j W[j][k] g[j]
//      (j ascending: a fixed order, coalesced over k) and g'[k] = dh[k] act'(z[k]); the first layer's dh is dL/dfeat.
//   5. (alignment) items (lanes): G_R += q gy^T and the sum of g_p = gy R^T over every item atom; group sums;
//      G_H = kabsch_rotation_backward_t; the centroid's term with sum ref (frames_bwd_f64_kernel's formulas).
//   6. atoms (lanes): the plan-time list hv_ptr / hv_list (4 it + j: slot j of item it; -(i + 1): align slot i, frames_hvp_kernel's
//      tables) - a slot recomputes its item's backward and adds g_p, an align slot adds G_H ref_i - cen.  Every row of gx is
//      stored once, untouched atoms as zeros: no atomics, no zeroing pass, the same bits on every run.
// The lanes of a frame exchange data through LDS only inside their own wave: lds_wave_sync() orders it, there is no block barrier.
// Steps 1-3 are the device functions frame_rotation_f64 / frame_features_f64 / frame_head_forward_f64 below, shared with
// frames_value_jac_f64_kernel (molann_dev_jac_f64.inc); steps 4-6 are frame_head_backward_f64 / frame_rotation_vjp_f64 /
// frame_atoms_vjp_f64, shared with frame_value_term_loop_f64 at the end of this file: the loop of the value-and-bias kernels.
// =============================================================================================
struct VjpF64Args {
    long n_frames;
    int n_inp, n_align, n_items, d_feat, d_out;
    int max_w, lds_per_frame;   // in doubles; lds_per_frame = 0 without a head
};

__device__ __forceinline__ void lds_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// g_p = g R^T (the backward of y = q R for one atom)
__device__ __forceinline__ V3d rotate_back(V3d g, const double (&R)[9]) {
    return v3d(fma(g.z, R[2], fma(g.y, R[1], g.x * R[0])), fma(g.z, R[5], fma(g.y, R[4], g.x * R[3])), fma(g.z, R[8], fma(g.y, R[7], g.x * R[6])));
}

// the backward of item d for the cotangent row df: gy[0..3] on the aligned coordinates, q[0..3] = the centred input atoms
__device__ __forceinline__ void item_backward_f64(const ItemDev& d, const double* __restrict__ xf, const double* df, bool has_align, V3d c,
                                                  const double (&R)[9], V3d (&q)[4], V3d (&gy)[4]) {
    V3d y[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        q[j] = load_atom_f64(xf, d.idx[j]);
        if (has_align) q[j] = q[j] - c;
        y[j] = has_align ? rotate(q[j], R) : q[j];
        gy[j] = v3d(0., 0., 0.);
    }
    const int w = item_width(d.type);
    const double g3[3] = {df[d.col], w > 1 ? df[d.col + 1] : 0.0, w > 2 ? df[d.col + 2] : 0.0};
    eval_item_backward_f64(d.type, y[0], y[1], y[2], y[3], g3, gy[0], gy[1], gy[2], gy[3]);
}

// Steps 1-3 of a frame, shared with frames_value_jac_f64_kernel (molann_dev_jac_f64.inc): they do not depend on the cotangent.
// ---- 1. centroid, covariance, rotation (frames_f64_kernel's formulas)
template <int G>
__device__ __forceinline__ void frame_rotation_f64(const double* __restrict__ xf, const int* __restrict__ align_idx, const double* __restrict__ ref64,
                                                   int n_align, int gl, V3d& c, double (&h)[9], double (&R)[9]) {
    double sx = 0., sy = 0., sz = 0.;
    for (int i = gl; i < n_align; i += G) { const V3d p = load_atom_f64(xf, align_idx[i]); sx += p.x; sy += p.y; sz += p.z; }
    const double inv_a = 1.0 / (double)n_align;
    c = v3d(group_sum<G>(sx) * inv_a, group_sum<G>(sy) * inv_a, group_sum<G>(sz) * inv_a);
    double g = 0.;
    for (int i = gl; i < n_align; i += G) {
        const double rx = ref64[3 * i], ry = ref64[3 * i + 1], rz = ref64[3 * i + 2];
        const V3d p = load_atom_f64(xf, align_idx[i]) - c;
        g = fma(p.x, p.x, fma(p.y, p.y, fma(p.z, p.z, g)));
        h[0] = fma(p.x, rx, h[0]); h[1] = fma(p.x, ry, h[1]); h[2] = fma(p.x, rz, h[2]);
        h[3] = fma(p.y, rx, h[3]); h[4] = fma(p.y, ry, h[4]); h[5] = fma(p.y, rz, h[5]);
        h[6] = fma(p.z, rx, h[6]); h[7] = fma(p.z, ry, h[7]); h[8] = fma(p.z, rz, h[8]);
    }
    g = group_sum<G>(g);
#pragma unroll
    for (int i = 0; i < 9; ++i) h[i] = group_sum<G>(h[i]);
    kabsch_rotation_t<double, double>(h, 0.5 * (g + ref64[3 * n_align + 3]) * 1.0001, R);
}

// ---- 2. features (lanes over the items) into fdst: the frame's LDS row, or y where the plan has no head
template <int G>
__device__ __forceinline__ void frame_features_f64(const double* __restrict__ xf, const ItemDev* __restrict__ items, int n_items, int gl,
                                                   bool has_align, V3d c, const double (&R)[9], double* fdst) {
    for (int it = gl; it < n_items; it += G) {
        const ItemDev d = items[it];
        V3d p0 = load_atom_f64(xf, d.idx[0]), p1 = load_atom_f64(xf, d.idx[1]), p2 = load_atom_f64(xf, d.idx[2]), p3 = load_atom_f64(xf, d.idx[3]);
        if (has_align) { p0 = rotate(p0 - c, R); p1 = rotate(p1 - c, R); p2 = rotate(p2 - c, R); p3 = rotate(p3 - c, R); }
        double v[3];
        const int w = eval_item_f64(d.type, p0, p1, p2, p3, v);
        fdst[d.col] = v[0];
        if (w > 1) fdst[d.col + 1] = v[1];
        if (w > 2) fdst[d.col + 2] = v[2];
    }
}

// ---- 3. head forward: the hidden layers' pre-activations go to zrows, the last layer to of; returns the end of the pre-activations
template <int G>
__device__ __forceinline__ double* frame_head_forward_f64(const F64Mlp& m, int gl, const double* feat, double* zrows, double* row0, double* row1,
                                                          double* of) {
    const double* cur = feat;
    double* nxt = row0;
    double* zl = zrows;
    for (int l = 0; l < m.n_layers; ++l) {
        const int K = m.dims[l], J = m.dims[l + 1];
        const bool last = l + 1 == m.n_layers;
        const double* Wl = m.W[l];
        const double* bl = m.b[l];
        for (int j = gl; j < J; j += G) {
            const double* w = Wl + (long)j * K;
            double acc = bl[j];
            for (int k = 0; k < K; ++k) acc = fma(w[k], cur[k], acc);
            if (last) of[j] = acc;
            else { zl[j] = acc; nxt[j] = apply_activation_f64(m.act, acc); }
        }
        lds_wave_sync();
        if (!last) zl += J;
        cur = nxt;
        nxt = nxt == row0 ? row1 : row0;
    }
    return zl;
}

// Steps 4-6 of a frame, shared with frame_value_term_loop_f64 below: they take the cotangent row.
// ---- 4. head backward for x only: g is the cotangent, zl is past the last hidden layer's pre-activations; returns dL/dfeat
template <int G>
__device__ __forceinline__ const double* frame_head_backward_f64(const F64Mlp& m, int gl, const double* g, double* zl, double* row0, double* row1) {
    double* gn = row0;
    for (int l = m.n_layers - 1; l >= 0; --l) {
        const int K = m.dims[l], J = m.dims[l + 1];
        const double* Wl = m.W[l];
        if (l > 0) zl -= K;
        for (int k = gl; k < K; k += G) {
            double acc = 0.;
            for (int j = 0; j < J; ++j) acc = fma(Wl[(long)j * K + k], g[j], acc);
            gn[k] = l > 0 ? acc * act_derivative_f64(m.act, zl[k]) : acc;
        }
        lds_wave_sync();
        g = gn;
        gn = gn == row0 ? row1 : row0;
    }
    return g;
}

// ---- 5. what the items give the rotation's backward: G_H and the centroid's term for dL/dfeat = df
template <int G>
__device__ __forceinline__ void frame_rotation_vjp_f64(const double* __restrict__ xf, const double* __restrict__ ref64,
                                                       const ItemDev* __restrict__ items, int n_items, int n_align, int gl, const double* df, V3d c,
                                                       const double (&h)[9], const double (&R)[9], double (&GH)[9], V3d& cen) {
    double GR[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.};
    V3d gsum = v3d(0., 0., 0.);
    for (int it = gl; it < n_items; it += G) {
        const ItemDev d = items[it];
        V3d q[4], gy[4];
        item_backward_f64(d, xf, df, true, c, R, q, gy);
        const int na = item_atoms(d.type);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (j < na) { // y = q R :  G_R += q^T g ,  g_p = g R^T
                const V3d g = gy[j];
                GR[0] = fma(q[j].x, g.x, GR[0]); GR[1] = fma(q[j].x, g.y, GR[1]); GR[2] = fma(q[j].x, g.z, GR[2]);
                GR[3] = fma(q[j].y, g.x, GR[3]); GR[4] = fma(q[j].y, g.y, GR[4]); GR[5] = fma(q[j].y, g.z, GR[5]);
                GR[6] = fma(q[j].z, g.x, GR[6]); GR[7] = fma(q[j].z, g.y, GR[7]); GR[8] = fma(q[j].z, g.z, GR[8]);
                gsum = gsum + rotate_back(g, R);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 9; ++i) GR[i] = group_sum<G>(GR[i]);
    gsum = v3d(group_sum<G>(gsum.x), group_sum<G>(gsum.y), group_sum<G>(gsum.z));
    kabsch_rotation_backward_t<double, double>(h, R, GR, GH);
    // H = sum_i (a_i - c) ref_i^T also depends on c through every p_i: - G_H (sum_j ref_j) / a per align atom
    const double inv_a = 1.0 / (double)n_align;
    const V3d t = mat_ref(GH, ref64[3 * n_align], ref64[3 * n_align + 1], ref64[3 * n_align + 2]);
    cen = v3d(inv_a * (gsum.x + t.x), inv_a * (gsum.y + t.y), inv_a * (gsum.z + t.z));
}

// ---- 6. atoms (lanes): every row of gxf once, its terms in plan order
template <int G>
__device__ __forceinline__ void frame_atoms_vjp_f64(const double* __restrict__ xf, double* __restrict__ gxf, const double* __restrict__ ref64,
                                                    const ItemDev* __restrict__ items, const int* __restrict__ hv_ptr,
                                                    const int* __restrict__ hv_list, int n_inp, int gl, const double* df, bool has_align, V3d c,
                                                    const double (&R)[9], const double (&GH)[9], V3d cen) {
    for (int k = gl; k < n_inp; k += G) {
        V3d acc = v3d(0., 0., 0.);
        const int e1 = hv_ptr[k + 1];
        for (int e = hv_ptr[k]; e < e1; ++e) {
            const int code = hv_list[e];
            if (code < 0) {
                const int i = -code - 1;
                acc = acc + (mat_ref(GH, ref64[3 * i], ref64[3 * i + 1], ref64[3 * i + 2]) - cen);
            } else {
                const ItemDev d = items[code >> 2];
                const int j = code & 3;
                V3d q[4], gy[4];
                item_backward_f64(d, xf, df, has_align, c, R, q, gy);
                V3d t = gy[3];   // slot j (selects, not an indexed load: gy stays in registers)
                if (j == 2) t = gy[2];
                if (j == 1) t = gy[1];
                if (j == 0) t = gy[0];
                acc = acc + (has_align ? rotate_back(t, R) : t);
            }
        }
        gxf[3 * k] = acc.x;
        gxf[3 * k + 1] = acc.y;
        gxf[3 * k + 2] = acc.z;
    }
}

template <int G>
__global__ __launch_bounds__(256) void frames_value_vjp_f64_kernel(const double* __restrict__ x, const double* __restrict__ gout,
                                                                   double* __restrict__ out, double* __restrict__ gx,
                                                                   const int* __restrict__ align_idx, const double* __restrict__ ref64,
                                                                   const ItemDev* __restrict__ items, const int* __restrict__ hv_ptr,
                                                                   const int* __restrict__ hv_list, VjpF64Args a, F64Mlp m) {
    static_assert(G == 8 || G == 16 || G == 32 || G == 64, "lane group of 8..64");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int gl = threadIdx.x & (G - 1);
    const int slot = threadIdx.x / G;
    const long per_block = blockDim.x / G;
    const long frame_dw = 3l * a.n_inp;
    const bool has_align = a.n_align > 0;
    const bool has_head = m.n_layers > 0;
    double* feat = (double*)smem + (size_t)slot * a.lds_per_frame;
    double* zrows = feat + a.d_feat;
    double* row0 = zrows + (a.lds_per_frame - a.d_feat - 2 * a.max_w);
    double* row1 = row0 + a.max_w;
    for (long f = (long)blockIdx.x * per_block + slot; f < a.n_frames; f += (long)gridDim.x * per_block) {
        const double* xf = x + f * frame_dw;
        double* gxf = gx + f * frame_dw;
        const double* gf = gout + f * (long)a.d_out;
        double* of = out + f * (long)a.d_out;
        // ---- 1. centroid, covariance, rotation
        double R[9] = {1., 0., 0., 0., 1., 0., 0., 0., 1.};
        double h[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.};
        V3d c = v3d(0., 0., 0.);
        if (has_align) frame_rotation_f64<G>(xf, align_idx, ref64, a.n_align, gl, c, h, R);
        // ---- 2. features
        frame_features_f64<G>(xf, items, a.n_items, gl, has_align, c, R, has_head ? feat : of);
        const double* df = gf;     // dL/dfeat: the cotangent itself without a head
        if (has_head) {
            lds_wave_sync();
            // ---- 3. head forward
            double* zl = frame_head_forward_f64<G>(m, gl, feat, zrows, row0, row1, of);
            // ---- 4. head backward: zl is past the last hidden layer's pre-activations
            df = frame_head_backward_f64<G>(m, gl, gf, zl, row0, row1);
        }
        // ---- 5. what the items give the rotation's backward
        double GH[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.};
        V3d cen = v3d(0., 0., 0.);
        if (has_align) frame_rotation_vjp_f64<G>(xf, ref64, items, a.n_items, a.n_align, gl, df, c, h, R, GH, cen);
        // ---- 6. atoms (lanes): every row once, its terms in plan order
        frame_atoms_vjp_f64<G>(xf, gxf, ref64, items, hv_ptr, hv_list, a.n_inp, gl, df, has_align, c, R, GH, cen);
        if (has_head) lds_wave_sync();   // the next frame's rows are this frame's
    }
}

// =============================================================================================
// frame_value_term_loop_f64<G>: the frame loop of every "values + a term on them + forces in one launch" kernel
// on all of the model's outputs that runs as fast through it as written out: frames_value_{restraint,hills,opes,opes_table}_f64_kernel.
// (The grid kernel and the three bias kernels on chosen columns keep the same loop written out; DESIGN.md, "One frame loop for the
// value-and-bias kernels", has the figures.)  The cotangent of such a kernel
// depends on y, so it is formed where y is: lanes, grid-stride loop and steps as frames_value_vjp_f64_kernel, whose device functions do
// the work.  A frame's LDS rows are cot[d_out], then that kernel's where there is a head (none without one): lds_per_frame counts them.
//   1.-3. rotation, features, head forward.  The outputs - the last layer's with a head, the features without one - are written to
//      cot, not to y: a lane never reads y back from global memory.
//   term(f, gl, cot, of): reads y from cot, stores it to of (the frame's row of y) and its energies, and leaves the cotangent in
//      cot.  Between its last read of a word of cot by another lane and a store to that word it calls lds_wave_sync(); the loop syncs
//      after it.  Its sums have a fixed order, so the bits do not depend on N or on the frame's slot in its block.
//   4.-6. head backward, the rotation's backward and the per-atom gather on cot: with the same cotangent the bits of
//      frames_value_vjp_f64_kernel.
// block MUST be blockDim.x and nothing else: it decides which frames a slot runs.  It is a parameter only because the kernel has to read
// it: read in here, behind the inlining, it becomes a vector load of 16 bits and a wait on it at the head of every block (half a
// microsecond on a one-frame batch) where the kernel's own read is a scalar load among its arguments.
// =============================================================================================
template <int G, class Term>
__device__ __forceinline__ void frame_value_term_loop_f64(const double* __restrict__ x, double* __restrict__ out, double* __restrict__ gx,
                                                          const int* __restrict__ align_idx, const double* __restrict__ ref64,
                                                          const ItemDev* __restrict__ items, const int* __restrict__ hv_ptr,
                                                          const int* __restrict__ hv_list, const VjpF64Args& a, const F64Mlp& m,
                                                          unsigned block, Term term) {
    static_assert(G == 8 || G == 16 || G == 32 || G == 64, "lane group of 8..64");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int gl = threadIdx.x & (G - 1);
    const int slot = threadIdx.x / G;
    const long per_block = block / G;
    const long frame_dw = 3l * a.n_inp;
    const bool has_align = a.n_align > 0;
    const bool has_head = m.n_layers > 0;
    double* cot = (double*)smem + (size_t)slot * a.lds_per_frame;
    double* feat = cot + a.d_out;
    double* zrows = feat + a.d_feat;
    // row0 and row1 are the LAST 2 max_w doubles of a frame's rows, whatever lds_per_frame counts: a kernel whose rows hold more than this
    // loop uses (frames_value_pbmetad_f64_kernel on bias64_rows: BIAS_SEL more) finds its own words just below them, at
    // cot + lds_per_frame - 2 max_w - extra, above the hidden layers' rows.  Moving the two rows breaks that kernel.
    double* row0 = zrows + (a.lds_per_frame - a.d_out - a.d_feat - 2 * a.max_w);
    double* row1 = row0 + a.max_w;
    for (long f = (long)blockIdx.x * per_block + slot; f < a.n_frames; f += (long)gridDim.x * per_block) {
        const double* xf = x + f * frame_dw;
        double* gxf = gx + f * frame_dw;
        double* of = out + f * (long)a.d_out;
        // ---- 1. centroid, covariance, rotation
        double R[9] = {1., 0., 0., 0., 1., 0., 0., 0., 1.};
        double h[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.};
        V3d c = v3d(0., 0., 0.);
        if (has_align) frame_rotation_f64<G>(xf, align_idx, ref64, a.n_align, gl, c, h, R);
        // ---- 2. features
        frame_features_f64<G>(xf, items, a.n_items, gl, has_align, c, R, has_head ? feat : cot);
        lds_wave_sync();
        // ---- 3. head forward, its last layer into cot
        double* zl = zrows;
        if (has_head) zl = frame_head_forward_f64<G>(m, gl, feat, zrows, row0, row1, cot);
        // ---- the term on the outputs: y and the energies are stored, cot becomes the cotangent
        term(f, gl, cot, of);
        lds_wave_sync();
        // ---- 4. head backward
        const double* df = cot;     // dL/dfeat: the cotangent itself without a head
        if (has_head) df = frame_head_backward_f64<G>(m, gl, cot, zl, row0, row1);
        // ---- 5. what the items give the rotation's backward
        double GH[9] = {0., 0., 0., 0., 0., 0., 0., 0., 0.};
        V3d cen = v3d(0., 0., 0.);
        if (has_align) frame_rotation_vjp_f64<G>(xf, ref64, items, a.n_items, a.n_align, gl, df, c, h, R, GH, cen);
        // ---- 6. atoms (lanes): every row once, its terms in plan order
        frame_atoms_vjp_f64<G>(xf, gxf, ref64, items, hv_ptr, hv_list, a.n_inp, gl, df, has_align, c, R, GH, cen);
        lds_wave_sync();   // the next frame's rows are this frame's
    }
}

} // namespace
