// molann_host_create.inc - part of libmolann_hip.so, included by molann_kernels.hip (one translation unit: the kernels' host stubs and the
// launches that use them must see each other).  Host: what a plan will be (plan_choose: arithmetic on the description, no device),
// then its creation - device tables, streams and events, the kernels built at creation - and its one teardown.
namespace {

// activations the backward kernels differentiate; the same set is cheap enough for the MLP fused into a lane kernel
inline bool act_served(int act) {
    return act == MOLANN_ACT_TANH || act == MOLANN_ACT_RELU || act == MOLANN_ACT_SIGMOID || act == MOLANN_ACT_IDENTITY ||
           act == MOLANN_ACT_SILU || act == MOLANN_ACT_LEAKY_RELU;
}

// a head within the fused MLP's limits: fp32, <= 4 layers, every width <= 32, at most max_feat features, a served activation
inline bool head_is_small(const int* dims, int n_layers, int d_feat, int prec, int act, int max_feat = LANE_MLP_MAX_WIDTH) {
    if (n_layers <= 0 || n_layers > LANE_MLP_MAX_LAYERS || prec != MOLANN_MLP_F32 || d_feat > max_feat || !act_served(act)) return false;
    for (int l = 1; l <= n_layers; ++l)
        if (dims[l] > LANE_MLP_MAX_WIDTH) return false;
    return true;
}

// floats of the parameter-gradient buffer (torch layout: dW_l[J][K] then db_l[J], layer after layer)
inline int grad_params_count(const int* dims, int n_layers) {
    int n = 0;
    for (int l = 0; l < n_layers; ++l) n += dims[l + 1] * dims[l] + dims[l + 1];
    return n;
}

// The MFMA copy of the weights (pack_mfma_kernel): per layer Wp[Jp][Kp] in the MLP's precision, then bias[Jp] in fp32, 16-byte
// aligned.  Kp, Jp and the layer's offset in weight elements; returns the copy's bytes.  The backward kernels read the fp32 copy.
size_t mlp_layout(const int* dims, int n_layers, bool bf16, int* kp, int* jp, long* off) {
    const size_t es = bf16 ? 2 : 4;
    size_t bytes = 0;
    for (int l = 0; l < n_layers; ++l) {
        kp[l] = ceil_to(dims[l], bf16 ? 32 : 16);
        jp[l] = ceil_to(dims[l + 1], 16);
        off[l] = (long)(bytes / es);
        bytes += ((size_t)jp[l] * kp[l]) * es + (size_t)jp[l] * 4;
        bytes = (bytes + 15) & ~(size_t)15;
    }
    return bytes;
}
void set_layout(JitSpecBox& b, const int* kp, const int* jp, const long* off, int n_layers) {
    b.kp.assign(kp, kp + n_layers); b.jp.assign(jp, jp + n_layers); b.woff.assign(off, off + n_layers);
}

ChainGeom chain_geom(const int* dims, int n_layers, bool bf16) {
    ChainGeom g;
    memset(&g, 0, sizeof(g));
    g.nl = n_layers;
    g.bf16 = bf16 ? 1 : 0;
    for (int i = 0; n_layers > 0 && i <= n_layers; ++i) g.dims[i] = dims[i];
    return g;
}
// 16-frame blocks per wave of the chain kernel, an upper bound (plan creation steps down while the build spills): what the register
// file holds - resident stream: two waves per SIMD - and 0 where two LDS slabs of a streamed head do not fit
int chain_fb_bound(const ChainGeom& g) {
    int fb = 0;
    for (int f = 4; f >= 1 && fb == 0; --f)
        if (f * g.regs_per_fb() <= (chain_resident(g) ? 256 : 512)) fb = f;
    if (!chain_resident(g) && 2 * g.slab_max() * 1024 > 163840 - 1024) fb = 0;
    return fb;
}

// waves per block of molann_mlp_bwd: as many [unit][frame] scratch tiles as the LDS holds, eight at most; < 1: not served
inline int mlp_bwd_wpb(const std::vector<int>& dims, int act) {
    return (int)std::min<long>(8, (163840 - 64) / ((long)mlp_bwd_rows(dims, act) * 68 * 4));
}

// the dense frame tile of molann_lane_bwd (reused for the gradient rows)
inline void features_bwd_geometry(int n_inp, molann_plan::LaneGeom& g) { lane_geometry(g, 64 * n_inp * 12, 1); }

// Everything plan creation decides, computed from the description alone (hipRTC's presence and the MOLANN_NO_* switches are inputs).
struct PlanChoice {
    std::vector<ItemDev> items, items_slot, ring_items;   // atoms as frame indices / as slots / as positions in the ring's image
    std::vector<int> slots;                               // touched atoms in first-use order: align atoms, then the feature table's
    int d_feat, out_dim, cols_needed;
    bool has_position_items, align_is_prefix, regs_mode, nojit;
    bool small_mlp, wide_in_mlp, lane_spec_ok, jit_possible, fused_mlp, lane_mlp, jit_only, small_head, wide_fused, dense_positions;
    int family;
    molann_plan::LaneGeom geom[2], jit_geom;
    std::vector<int> ring_win, ring_align_pos, bw_atoms, bw_ptr, bw_list, bw_align, va_atoms, va_ptr, va_list, hv_ptr, hv_list, align_slot;
    int ring_nd, ring_nwin;
    int kp[MOLANN_MAX_LAYERS], jp[MOLANN_MAX_LAYERS];
    long moff[MOLANN_MAX_LAYERS];
    int mlp_ld[2], mlp_lds_per_wave;
    size_t lane_floats, mfma_bytes, chain_bytes, work_bytes;
    ChainGeom cg;
    int chain_fb, cbwd_waves, n_grad_params;
    long chain_stream_bytes, work_frames;
    JitSpec fwd, wide;      // the specialised lane kernel (lane_spec_ok), and with a wide head as its MLP stage (wide_fused)
    JitSpec align_out;      // AlignmentLayer.forward through the specialised kernel; no slots: not served
};

// the feature list as items, touched atoms as slots, the kernel family and where the MLP runs
void choose_family(const molann_plan_desc* d, PlanChoice& c) {
    c.d_feat = expand_items(d, c.items);
    c.out_dim = d->n_layers > 0 ? d->layer_dims[d->n_layers] : c.d_feat;
    const int n_items = (int)c.items.size();
    c.has_position_items = false;
    for (const ItemDev& it : c.items) c.has_position_items = c.has_position_items || it.type == IT_POSITION;
    c.small_mlp = head_is_small(d->layer_dims, d->n_layers, c.d_feat, d->mlp_precision, d->activation);
    // feature dims 33..64 in front of such an MLP: fused too, by the plan-specialised kernel only (16 k-steps in layer 0)
    c.wide_in_mlp = !c.small_mlp && head_is_small(d->layer_dims, d->n_layers, c.d_feat, d->mlp_precision, d->activation, 2 * LANE_MLP_MAX_WIDTH);
    c.cols_needed = std::max(1, c.small_mlp ? ceil_to(c.d_feat, 4) : c.d_feat);
    std::vector<int> slot_of(d->n_inp, -1);
    auto slot = [&](int atom) {
        if (slot_of[atom] < 0) { slot_of[atom] = (int)c.slots.size(); c.slots.push_back(atom); }
        return slot_of[atom];
    };
    c.align_is_prefix = true; // align atom i must be slot i (no repeated align atoms)
    for (int i = 0; i < d->n_align; ++i) c.align_is_prefix = c.align_is_prefix && (slot(d->align_idx[i]) == i);
    c.items_slot = c.items;
    for (auto& it : c.items_slot)
        for (int i = 0; i < 4; ++i) it.idx[i] = slot(it.idx[i]);
    const int n_slots = (int)c.slots.size();
    // (plan creation is setup time: MOLANN_NO_REGS / MOLANN_NO_JIT select the other generic modes here)
    c.regs_mode = n_items > 0 && n_items <= 64 && n_slots <= 16 && c.align_is_prefix && getenv("MOLANN_NO_REGS") == nullptr;
    memset(c.geom, 0, sizeof(c.geom));
    memset(&c.jit_geom, 0, sizeof(c.jit_geom));
    const bool lane_tables_fit = d->n_align <= 64 && (long)d->n_inp * 768 <= 65536;
    if (n_items > 0 && lane_tables_fit && c.cols_needed <= LANE_MAX_COLS) lane_geometry(c.geom[0], 64 * d->n_inp * 12, c.cols_needed);
    if (d->n_align > 0 && lane_tables_fit) features_bwd_geometry(d->n_inp, c.geom[1]);
    // The plan-specialised lane kernel stages only the touched 16-byte windows of a frame, so its tile does not grow
    // with n_inp: a plan that touches few atoms (<= 32) of a LARGE frame is a lane-per-frame plan too, as long as
    // hipRTC is there to build it (the ahead-of-time lane kernel needs the dense tile and cannot serve it).
    const char* nojit_env = getenv("MOLANN_NO_JIT");
    c.nojit = nojit_env && nojit_env[0] == '1';
    const bool head_in_lane = (c.small_mlp || c.wide_in_mlp) && d->n_features > 0;
    c.lane_spec_ok = n_items > 0 && n_items <= JIT_MAX_ITEMS && n_slots <= JIT_MAX_SLOTS && c.align_is_prefix;
    if (c.lane_spec_ok) {
        JitSpec& j = c.fwd;
        j.n_inp = d->n_inp; j.n_align = d->n_align; j.act = d->activation; j.d_feat = c.d_feat;
        j.n_layers = head_in_lane ? d->n_layers : 0;
        j.out_cols = head_in_lane ? c.out_dim : c.d_feat;
        j.slots = c.slots; j.items = c.items_slot;
        // compact tile: only the 16-byte windows of a frame that hold a touched atom go to LDS, so more waves fit
        j.win = compact_windows(c.slots, d->n_inp);
        if (head_in_lane) j.dims.assign(d->layer_dims, d->layer_dims + d->n_layers + 1);
        // its LDS geometry (compact tile + staging rows) must leave room for >= 4 waves per CU
        jit_geometry(j, c.jit_geom, head_in_lane ? c.d_feat : c.cols_needed, c.cols_needed);
    }
    c.jit_possible = c.lane_spec_ok && rtc_api()->ok && !c.nojit && c.cols_needed <= LANE_MAX_COLS && 3 * d->n_inp >= 4 && c.jit_geom.ok != 0;
    if (!c.jit_possible) memset(&c.jit_geom, 0, sizeof(c.jit_geom));
    const bool lane_by_jit_only = c.jit_possible && !c.geom[0].ok;
    const bool fused_by_jit_only = c.jit_possible && c.wide_in_mlp && d->n_features > 0;
    // the family names the kernel that serves the plan's main product (features if it has any)
    c.family = (n_items > 0 ? (c.geom[0].ok || lane_by_jit_only) : c.geom[1].ok) ? 0 : 1;
    c.fused_mlp = ((c.family == 0) && c.small_mlp && d->n_features > 0) || fused_by_jit_only;
    // a head within the fused MLP's limits behind a kernel that cannot fuse it (wave per frame), or called on its own
    // (molann_mlp_packed_f32): mlp_lane_kernel on the same weight fragments
    c.lane_mlp = c.small_mlp && !(getenv("MOLANN_NO_LANE_MLP") && getenv("MOLANN_NO_LANE_MLP")[0] == '1');
    c.jit_only = lane_by_jit_only || fused_by_jit_only;
}

// frames_ring_kernel tables (plans the lane kernels do not serve): windows, image positions
void choose_ring(const molann_plan_desc* d, PlanChoice& c) {
    c.ring_nd = c.ring_nwin = 0;
    if (!(c.family == 1 && !c.items.empty() && c.align_is_prefix)) return;
    const std::vector<int> win = compact_windows(c.slots, d->n_inp);
    static const int buckets[] = {1, 2, 3, 4, 6, 8, 10, 12, 14, 16, 18, 20, 22, 24, 26, 28, 30, 32};
    int nd = 0;
    for (int b : buckets)
        if (nd == 0 && (long)b * 64 >= (long)win.size()) nd = b;
    if (nd == 0) return;
    // dword position of the atom's x inside the image; its three dwords are contiguous there: either one
    // window holds all of them (always so for the window clamped to the frame's end, which may overlap its
    // predecessor), or the atom runs over the end of window k and window k + 1 starts right behind it
    auto pos_of = [&](int atom) {
        const int d0 = 3 * atom;
        for (size_t k = 0; k < win.size(); ++k)
            if (d0 >= win[k] && d0 + 2 < win[k] + 4) return (int)(4 * k) + d0 - win[k];
        for (size_t k = 0; k < win.size(); ++k)
            if (d0 >= win[k] && d0 < win[k] + 4) return (int)(4 * k) + d0 - win[k];
        return 0;
    };
    for (int w : win) c.ring_win.push_back(4 * w);
    for (int i = 0; i < d->n_align; ++i) c.ring_align_pos.push_back(pos_of(d->align_idx[i]));
    c.ring_items = c.items;
    for (auto& it : c.ring_items)
        for (int i = 0; i < 4; ++i) it.idx[i] = pos_of(it.idx[i]);
    c.ring_nd = nd;
    c.ring_nwin = (int)win.size();
}

// gather tables of the kernels that take frames the lane kernels do not, and of the second order
void choose_gather_tables(const molann_plan_desc* d, PlanChoice& c) {
    const std::vector<ItemDev>& items = c.items;
    // backward of large frames without atomics: who contributes to which touched atom
    if (!c.geom[0].ok && !items.empty()) {
        std::vector<std::vector<int>> contrib(d->n_inp);
        std::vector<int> al_of(d->n_inp, -1);
        std::vector<char> touched(d->n_inp, 0), seen(d->n_inp, 0);
        for (size_t it = 0; it < items.size(); ++it)
            for (int j = 0; j < item_atoms(items[it].type); ++j) { contrib[items[it].idx[j]].push_back((int)(4 * it + j)); touched[items[it].idx[j]] = 1; }
        for (int i = 0; i < d->n_align; ++i) { if (al_of[d->align_idx[i]] < 0) al_of[d->align_idx[i]] = i; touched[d->align_idx[i]] = 1; }
        bool repeated_align = false;
        for (int i = 0; i < d->n_align; ++i) { repeated_align = repeated_align || seen[d->align_idx[i]]; seen[d->align_idx[i]] = 1; }
        if (!repeated_align) {   // (an alignment set that names an atom twice keeps the atomics: the atom has two reference rows)
            c.bw_ptr.push_back(0);
            for (int a0 = 0; a0 < d->n_inp; ++a0)
                if (touched[a0]) {
                    c.bw_atoms.push_back(a0);
                    c.bw_align.push_back(al_of[a0]);
                    c.bw_list.insert(c.bw_list.end(), contrib[a0].begin(), contrib[a0].end());
                    c.bw_ptr.push_back((int)c.bw_list.size());
                }
        }
    }
    // values + vjp in one launch (molann_group_vjp.inc): the same lists for every alignment set, rows named twice included
    if (!c.geom[0].ok && !items.empty()) group_vjp_tables(d->n_inp, items, d->align_idx, d->n_align, c.va_atoms, c.va_ptr, c.va_list);
    // second order without atomics: every atom's item slots, then its align slots, in a fixed order (molann_hvp.inc)
    if (!items.empty()) hvp_tables(d->n_inp, items, d->align_idx, d->n_align, c.hv_ptr, c.hv_list);
    // AlignmentLayer.forward under autograd arrives as a feature plan with ONE position item per atom, in atom order: its
    // feature rows are the aligned frame, its backward the dense gradient of the alignment (frames_align_bwd_regs_kernel)
    c.dense_positions = false;
    if (d->n_align > 0 && d->n_layers == 0 && (int)items.size() == d->n_inp && !c.geom[0].ok) {
        bool dense = true, repeated = false;
        for (int i = 0; i < d->n_inp && dense; ++i) dense = items[i].type == IT_POSITION && items[i].idx[0] == i && items[i].col == 3 * i;
        c.align_slot.assign(d->n_inp, -1);
        for (int i = 0; i < d->n_align; ++i) { repeated = repeated || c.align_slot[d->align_idx[i]] >= 0; c.align_slot[d->align_idx[i]] = i; }
        c.dense_positions = dense && !repeated && getenv("MOLANN_NO_DENSE_ALIGN") == nullptr;
        if (!c.dense_positions) c.align_slot.clear();
    }
}

// the head outside a fused lane kernel: weight copies, the chain kernel's stream, the feature workspace, who serves its backward
void choose_head(const molann_plan_desc* d, PlanChoice& c) {
    const int nl = d->n_layers;
    const bool bf16 = d->mlp_precision == MOLANN_MLP_BF16;
    c.lane_floats = (c.fused_mlp || c.lane_mlp) ? (size_t)nl * (1024 + 512) + 1024 : 0;
    c.mfma_bytes = mlp_layout(d->layer_dims, nl, bf16, c.kp, c.jp, c.moff);
    c.mlp_ld[0] = c.mlp_ld[1] = c.mlp_lds_per_wave = 0;
    if (nl > 0) {
        // two activation buffers: [0] holds the inputs of even layers, [1] of odd layers (layer l writes what
        // layer l+1 reads).  Row strides: 16-byte multiples, off the power of two.
        int need[2] = {16, 16};
        for (int l = 0; l < nl; ++l) {
            need[l & 1] = std::max(need[l & 1], c.kp[l]);
            if (l + 1 < nl) need[(l + 1) & 1] = std::max(need[(l + 1) & 1], std::max(c.jp[l], c.kp[l + 1]));
        }
        for (int i = 0; i < 2; ++i) c.mlp_ld[i] = need[i] + (bf16 ? 8 : 4);
        c.mlp_lds_per_wave = 16 * (c.mlp_ld[0] + c.mlp_ld[1]) * (bf16 ? 2 : 4);
    }
    // wide MLP next to a gather kernel: the chain kernel's weight stream (molann_mlp_jit.inc), when its
    // two LDS slabs fit and at least one 16-frame block per wave fits the register file
    c.cg = chain_geom(d->layer_dims, nl, bf16);
    c.chain_fb = (nl > 0 && !c.fused_mlp) ? chain_fb_bound(c.cg) : 0;
    c.chain_stream_bytes = c.chain_fb > 0 ? c.cg.total_frags() * 1024 : 0;
    c.chain_bytes = c.chain_fb > 0 ? (size_t)c.chain_stream_bytes + (size_t)c.cg.bias_off(nl) * 4 : 0;
    c.work_frames = 0;
    c.work_bytes = 0;
    if (nl > 0 && d->n_features > 0 && !c.fused_mlp) {
        // feature chunk handed from the preprocessing kernel to the MLP kernel: sized to stay
        // resident in the 256 MiB Infinity Cache
        long wf = (64l << 20) / ((long)c.d_feat * 4);
        wf = std::max<long>(1024, std::min<long>(wf, 1l << 21)); // (narrow feature rows: few, large chunks - each costs ~6 host API calls, and a
                                                                  //  feature launch of 512 k frames takes 37 us where one of 1 M takes 46)
        wf &= ~63l;
        wf = std::max<long>(512, (wf / 2) & ~63l); // per half
        // Large frames: the feature rows are a few percent of the frame bytes, so letting them spill past the Infinity
        // Cache costs little, while a chunk that small leaves the MLP kernel (one block per CU, 64 FB frames per block
        // and step) a fraction of the chip: frames_ring_kernel holds every CU, the two kernels run one after the other,
        // and C5's MLP took 3.7 us per 1000 frames in 24 576-frame chunks against 1.2 on its own.  Up to 256 MiB per half.
        // (Round 3: for every wave-per-frame plan, not only those whose feature rows are a small part of the frame.  P2 - 166 atoms,
        // 126 features - ran 16 chunks of 66 560 frames per 1 M: 260 frames per CU and launch, both kernels all ramp and tail,
        // 1.64 ms; in 4 chunks 0.86 ms.)
        if (c.family == 1) wf = std::max<long>(wf, std::min<long>(1l << 18, ((256l << 20) / ((long)c.d_feat * 4)) & ~63l));
        c.work_frames = wf;
        c.work_bytes = 2 * (size_t)wf * c.d_feat * 4;
    }
    // a small head that no lane kernel fuses (wave-per-frame features): molann_mlp_bwd serves its backward
    c.small_head = c.lane_mlp && !c.fused_mlp && d->n_features > 0 && rtc_api()->ok;
    // backward of a wide fp32 head whose chain stream is resident (molann_chain_bwd.inc), built at its first use
    c.cbwd_waves = 0;
    if (c.chain_fb > 0 && chain_resident(c.cg) && !bf16 && !c.lane_mlp && rtc_api()->ok && !c.nojit && act_served(d->activation))
        c.cbwd_waves = chain_bwd_waves(std::vector<int>(c.kp, c.kp + nl), std::vector<int>(c.jp, c.jp + nl));
    // where one of the backward kernels serves the head, the parameter-gradient buffer has the head's layout
    const bool head_has_backward = (c.jit_possible && c.fused_mlp) || c.small_head || c.cbwd_waves > 0;
    c.n_grad_params = head_has_backward ? grad_params_count(d->layer_dims, nl) : 0;
}

// the lane kernel's description with the whole of a wide fp32 head as its MLP stage (molann_lane_jit.inc: WIDE_MLP)
JitSpec wide_lane_spec(const molann_plan_desc* d, const PlanChoice& c) {
    JitSpec j = c.fwd;
    j.n_layers = d->n_layers; j.out_cols = c.out_dim;
    j.dims.assign(d->layer_dims, d->layer_dims + d->n_layers + 1);
    j.wide_mlp = true; j.img_bytes = (int)(c.cg.total_frags() * 1024);
    return j;
}

void choose_side_kernels(const molann_plan_desc* d, PlanChoice& c) {
    // ---- the whole forward of a WIDE head in one lane kernel (round 3) ----------------------------------------------------
    // Hidden widths 33 .. ~128 behind a lane-per-frame preprocessing: features kernel + chain MLP kernel cost a launch, a
    // round trip of the features through the workspace and - the feature kernel holds every CU - no overlap.  Where the
    // chain's weight stream fits LDS beside a (shorter) ring, the specialised lane kernel runs the chain's arithmetic as its
    // MLP stage (molann_lane_jit.inc: WIDE_MLP).
    c.wide_fused = c.jit_possible && c.family == 0 && !c.fused_mlp && d->n_layers > 0 && d->n_features > 0 && d->mlp_precision != MOLANN_MLP_BF16 &&
                   c.chain_fb > 0 && chain_resident(c.cg) && c.chain_stream_bytes <= 112 * 1024 && c.d_feat <= LANE_MAX_COLS &&
                   getenv("MOLANN_NO_WIDE_FUSED") == nullptr;
    if (c.wide_fused) c.wide = wide_lane_spec(d, c);
    // ---- AlignmentLayer.forward through the specialised kernel: the aligned frame is the feature row of one position item per
    // atom, so molann_align_f32 is the loader / consumer kernel too (built at its first call).  Small frames only.
    if (!(d->n_align > 0 && d->n_inp <= JIT_MAX_SLOTS && 3 * d->n_inp <= LANE_MAX_COLS && 3 * d->n_inp >= 4 && rtc_api()->ok && !c.nojit)) return;
    JitSpec j;
    std::vector<int> seen(d->n_inp, 0);
    bool distinct = true;
    for (int i = 0; i < d->n_align; ++i) { distinct = distinct && !seen[d->align_idx[i]]; seen[d->align_idx[i]] = 1; j.slots.push_back(d->align_idx[i]); }
    for (int a = 0; a < d->n_inp; ++a) if (!seen[a]) j.slots.push_back(a);
    if (!distinct) return;
    for (int u = 0; u < d->n_inp; ++u) { ItemDev it = {IT_POSITION, 3 * j.slots[u], {u, u, u, u}, {0, 0}}; j.items.push_back(it); }
    j.n_inp = d->n_inp; j.n_align = d->n_align; j.act = 0; j.d_feat = 3 * d->n_inp; j.n_layers = 0; j.out_cols = 3 * d->n_inp;
    j.win = compact_windows(j.slots, d->n_inp);
    molann_plan::LaneGeom g;
    memset(&g, 0, sizeof(g));
    jit_geometry(j, g, j.d_feat, j.d_feat);
    if (g.ok) c.align_out = j;
}

// Fills the whole choice for any description validate_desc accepts, then says whether a plan may be made of it: E_DESC for a head
// whose input is not the feature row, E_UNSUPPORTED for one whose activations no wave's LDS holds.
int plan_choose(const molann_plan_desc* d, PlanChoice& c) {
    choose_family(d, c);
    choose_ring(d, c);
    choose_gather_tables(d, c);
    choose_head(d, c);
    choose_side_kernels(d, c);
    if (d->n_layers > 0 && d->n_features > 0 && d->layer_dims[0] != c.d_feat) return MOLANN_E_DESC;
    if (c.mlp_lds_per_wave > 163840) return MOLANN_E_UNSUPPORTED;
    return MOLANN_OK;
}

// The plan's device tables in one allocation: every table is recorded once (where its device pointer goes, its host data, its
// bytes), carved in that order at 256-byte steps, and uploaded where it has data.
struct BlobTables {
    struct Table { void* slot; const void* data; size_t bytes, off; };
    std::vector<Table> tables;
    size_t size = 0;
    // `slot` is the address of the plan's pointer to the table; `reserve`: bytes to keep where they exceed what is uploaded
    void add(void* slot, const void* data, size_t bytes, size_t reserve = 0) {
        tables.push_back({slot, data, bytes, size});
        size += (std::max<size_t>(1, std::max(bytes, reserve)) + 255) & ~(size_t)255;
    }
    hipError_t place(unsigned char* blob) const {   // (synchronous: plan creation is setup time)
        hipError_t e = hipSuccess;
        for (const Table& t : tables) {
            unsigned char* at = blob + t.off;
            memcpy(t.slot, &at, sizeof(at));
            if (e == hipSuccess && t.data && t.bytes > 0) e = hipMemcpy(at, t.data, t.bytes, hipMemcpyHostToDevice);
        }
        return e;
    }
};
size_t vec_bytes(const std::vector<int>& v) { return v.size() * sizeof(int); }
size_t vec_bytes(const std::vector<ItemDev>& v) { return v.size() * sizeof(ItemDev); }

// the reference in fp32 and fp64: [3 n_align] coordinates, centred here whatever the caller passes (pack_ref_kernel: the
// alignment does not depend on it), then the constants the kernels read behind them
void centred_ref(const molann_plan_desc* d, std::vector<float>& refc, std::vector<double>& refd) {
    refc.assign(3 * (size_t)d->n_align + 8, 0.f);
    refd.assign(3 * (size_t)d->n_align + 8, 0.);
    double mean[3] = {0, 0, 0}, s[4] = {0, 0, 0, 0};
    for (int i = 0; i < d->n_align; ++i)
        for (int c = 0; c < 3; ++c) mean[c] += d->ref_x[3 * i + c];
    for (int c = 0; c < 3; ++c) mean[c] /= (double)d->n_align;
    for (int i = 0; i < d->n_align; ++i) {
        for (int c = 0; c < 3; ++c) {
            const float r = (float)((double)d->ref_x[3 * i + c] - mean[c]);
            refc[3 * i + c] = r;
            refd[3 * i + c] = r;
            s[c] += r;
            s[3] += (double)r * r;
        }
    }
    float* c = refc.data() + 3 * (size_t)d->n_align;
    double* c64 = refd.data() + 3 * (size_t)d->n_align;
    for (int k = 0; k < 4; ++k) { c[k] = (float)s[k]; c64[k] = s[k]; }
    c[4] = 1.0f / (float)d->n_align;
    c[5] = (float)d->n_align;
    c64[4] = 1.0 / (double)d->n_align;
    c64[5] = (double)d->n_align;
}

// allocate the blob and fill its tables
int create_blob(molann_plan* p, const molann_plan_desc* d, const PlanChoice& c) {
    std::vector<float> refc;
    std::vector<double> refd;
    if (d->n_align > 0) centred_ref(d, refc, refd);
    const size_t n_ref = 3 * (size_t)d->n_align + 8;
    BlobTables t;
    t.add(&p->d_align_idx, d->align_idx, sizeof(int) * d->n_align);
    t.add(&p->d_ref, refc.data(), sizeof(float) * refc.size(), sizeof(float) * n_ref);
    t.add(&p->d_ref64, refd.data(), sizeof(double) * refd.size(), sizeof(double) * n_ref);
    t.add(&p->d_items, c.items.data(), vec_bytes(c.items));
    t.add(&p->d_items_slot, c.items_slot.data(), vec_bytes(c.items_slot));
    t.add(&p->d_slots, c.slots.data(), vec_bytes(c.slots));
    t.add(&p->d_ring_win, c.ring_win.data(), vec_bytes(c.ring_win));
    t.add(&p->d_ring_align_pos, c.ring_align_pos.data(), vec_bytes(c.ring_align_pos));
    t.add(&p->d_ring_items, c.ring_items.data(), vec_bytes(c.ring_items));
    t.add(&p->d_va_atoms, c.va_atoms.data(), vec_bytes(c.va_atoms));
    t.add(&p->d_va_ptr, c.va_ptr.data(), vec_bytes(c.va_ptr));
    t.add(&p->d_va_list, c.va_list.data(), vec_bytes(c.va_list));
    t.add(&p->d_hv_ptr, c.hv_ptr.data(), vec_bytes(c.hv_ptr));
    t.add(&p->d_hv_list, c.hv_list.data(), vec_bytes(c.hv_list));
    t.add(&p->d_align_slot, c.align_slot.data(), vec_bytes(c.align_slot));
    t.add(&p->d_bw_atoms, c.bw_atoms.data(), vec_bytes(c.bw_atoms));
    t.add(&p->d_bw_ptr, c.bw_ptr.data(), vec_bytes(c.bw_ptr));
    t.add(&p->d_bw_list, c.bw_list.data(), vec_bytes(c.bw_list));
    t.add(&p->d_bw_align, c.bw_align.data(), vec_bytes(c.bw_align));
    // written by the pack kernels (molann_plan_update_mlp) and by the forward
    t.add(&p->d_wlane, nullptr, 0, sizeof(float) * c.lane_floats);
    t.add(&p->d_wmfma, nullptr, 0, c.mfma_bytes);
    t.add(&p->d_wchain, nullptr, 0, c.chain_bytes);
    t.add(&p->d_work, nullptr, 0, c.work_bytes);
    HIP_TRY(hipMalloc((void**)&p->blob, t.size));
    return (int)t.place(p->blob);
}

// the side stream and the events of the unfused forward's two workspace halves
int create_streams(molann_plan* p) {
    HIP_TRY(hipStreamCreateWithFlags(&p->side, hipStreamNonBlocking));
    for (int h = 0; h < 2; ++h) {
        HIP_TRY(hipEventCreateWithFlags(&p->ev_feat[h], hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&p->ev_mlp[h], hipEventDisableTiming));
    }
    HIP_TRY(hipEventCreateWithFlags(&p->ev_done, hipEventDisableTiming));
    return MOLANN_OK;
}

// ---- plan-specialised lane kernel --------------------------------------------------------------
void build_lane_kernel(molann_plan* p, const PlanChoice& c) {
    JitSpec j = c.fwd;
    p->spec = new (std::nothrow) JitSpecBox();
    if (p->spec) {
        p->spec->j = j;
        set_layout(*p->spec, p->kp, p->jp, p->moff, j.n_layers);
    }
    BuiltKernel k;
    // no SLP vectorisation: hipcc otherwise packs a fifth of this straight-line fp32 code into v_pk_* pairs, which
    // buys ~1.2x on those operations at two waves per SIMD and pays for it with ~130 register moves per tile and 44
    // more registers (C3: 166 -> 122 VGPRs, 74 -> 70 us; tools/ab_flags.sh)
    if (build_kernel(jit_source(j), "molann_lane_jit", "-fno-slp-vectorize", "jit", k) && j.ncons > 10 && k.scratch > 0) {
        // Three or four layers of 32 units: the weight fragments do not fit the 128 registers of four waves per SIMD and the
        // build spills.  Ten consumers (three waves per SIMD, 168 registers) serve the stream as well as fourteen.
        JitSpec j3 = j;
        molann_plan::LaneGeom g3;
        memset(&g3, 0, sizeof(g3));
        jit_geometry(j3, g3, p->fused_mlp ? p->d_feat : c.cols_needed, c.cols_needed, 10);
        BuiltKernel k3;
        if (g3.ok && build_kernel(jit_source(j3), "molann_lane_jit", "-fno-slp-vectorize", "jit with ten consumers", k3)) {
            if (k3.scratch >= 0 && k3.scratch < k.scratch) {
                std::swap(k, k3);
                j = j3; p->jit_geom = g3;
                if (p->spec) p->spec->j = j;
            }
            k3.unload();
        }
    }
    if (k.fn) {
        p->jit_mod = k.mod; p->jit_fn = k.fn; p->jit_nl = j.n_layers; p->jit_waves = 2;
        p->jit_ncons = j.ncons; p->jit_nload = j.nload; p->jit_nslot = j.nslot; p->jit_bpc = j.bpc; p->jit_lds_block = j.lds_block;
        snprintf(p->jit_note, sizeof(p->jit_note), "jit: specialised kernel, %d+1 waves per block, %zu bytes", j.ncons, k.bytes);
    } else {
        snprintf(p->jit_note, sizeof(p->jit_note), "jit: unavailable (rc=%d), generic kernel", k.rc);
    }
}

// ---- plan-specialised wide MLP: most frames per wave (A-fragment reuse) that the register file holds without scratch
void build_chain_kernel(molann_plan* p, const PlanChoice& c) {
    int rc = -1;
    for (int fb = c.chain_fb; fb >= 1 && !p->chain_fn; --fb) {
        BuiltKernel k;
        const bool built = build_kernel(jit_source_chain(c.cg, p->act, fb), "molann_mlp_chain", nullptr, "chain jit", k);
        rc = k.rc;
        if (!built) break;
        if (k.scratch > 0 && fb > 1) { k.unload(); continue; }
        p->chain_mod = k.mod; p->chain_fn = k.fn; p->chain_fb = fb; p->chain_waves = chain_waves(c.cg); p->chain_nslab = chain_nslab(c.cg);
        snprintf(p->chain_note, sizeof(p->chain_note), "chain: specialised kernel, FB=%d, %zu bytes", fb, k.bytes);
    }
    if (!p->chain_fn) snprintf(p->chain_note, sizeof(p->chain_note), "chain: unavailable (rc=%d), mlp_mfma_kernel", rc);
}

// ---- the whole forward of a wide head in one lane kernel: eight consumers + two loaders where the ring still has four slots
void build_wide_kernel(molann_plan* p, const PlanChoice& c) {
    int first = 8;     // (measured, [6,64,64,8] at 1 M frames: 188 / 175 / 176 / 182 us with 6 / 8 / 10 / 14 consumers)
    if (const char* e = diag_env("MOLANN_DEBUG_WIDE_CONS")) first = std::max(1, std::min(14, atoi(e)));
    for (int wide_cons : {first, 6}) {       // six consumers + two loaders = two waves per SIMD: 256 registers for the wider heads
        if (p->wide_fn) break;
        JitSpec jw = c.wide;
        molann_plan::LaneGeom wg;
        memset(&wg, 0, sizeof(wg));
        jit_geometry(jw, wg, p->d_feat, c.cols_needed, wide_cons);
        if (!(wg.ok && jw.nslot >= 4)) continue;
        if (wide_cons == 6 && jw.ncons + jw.nload > 8) continue;
        BuiltKernel k;
        if (!build_kernel(jit_source(jw), "molann_lane_jit", "-fno-slp-vectorize", "wide fused forward", k)) continue;
        if (k.scratch != 0) {
            if (getenv("MOLANN_JIT_VERBOSE")) fprintf(stderr, "molann wide fused forward with %d consumers not used (scratch=%d)\n", jw.ncons, k.scratch);
            k.unload();
            continue;
        }
        p->wide_mod = k.mod; p->wide_fn = k.fn;
        p->wide_ncons = jw.ncons; p->wide_nload = jw.nload; p->wide_nslot = jw.nslot; p->wide_bpc = jw.bpc; p->wide_lds_block = jw.lds_block;
    }
}

// the plan's fields that are the choice's
void adopt_choice(molann_plan* p, const molann_plan_desc* d, const PlanChoice& c) {
    p->n_inp = d->n_inp;
    p->n_align = d->n_align;
    p->align_first = d->n_align > 0 ? d->align_idx[0] : 0;
    p->n_features = d->n_features;
    p->n_items = (int)c.items.size();
    p->has_position_items = c.has_position_items;
    p->d_feat = c.d_feat;
    p->use_angle_value = d->use_angle_value;
    p->n_layers = d->n_layers;
    p->act = d->activation;
    p->mlp_prec = d->mlp_precision;
    for (int i = 0; d->n_layers > 0 && i <= d->n_layers; ++i) p->dims[i] = d->layer_dims[i];
    p->out_dim = c.out_dim;
    p->n_slots = (int)c.slots.size();
    p->regs_mode = c.regs_mode;
    p->geom[0] = c.geom[0]; p->geom[1] = c.geom[1]; p->jit_geom = c.jit_geom;
    p->family = c.family; p->fused_mlp = c.fused_mlp; p->lane_mlp = c.lane_mlp; p->jit_only = c.jit_only;
    p->ring_nd = c.ring_nd; p->ring_nwin = c.ring_nwin;
    p->bw_touched = (int)c.bw_atoms.size(); p->bw_list_len = (int)c.bw_list.size();
    p->va_touched = (int)c.va_atoms.size(); p->va_list_len = (int)c.va_list.size();
    p->dense_positions = c.dense_positions;
    for (int l = 0; l < d->n_layers; ++l) { p->kp[l] = c.kp[l]; p->jp[l] = c.jp[l]; p->moff[l] = c.moff[l]; }
    p->mlp_ld[0] = c.mlp_ld[0]; p->mlp_ld[1] = c.mlp_ld[1]; p->mlp_lds_per_wave = c.mlp_lds_per_wave;
    p->chain_stream_bytes = c.chain_stream_bytes;
    p->work_frames = c.work_frames;
    p->cbwd_waves = c.cbwd_waves;
    p->n_grad_params = c.n_grad_params;
}

} // namespace

extern "C" {

int molann_plan_create(const molann_plan_desc* d, molann_plan** out_plan) {
    if (!out_plan) return MOLANN_E_NULL;
    *out_plan = nullptr;
    const int v = validate_desc(d);
    if (v != MOLANN_OK) return v;
    PlanChoice c;
    const int chosen = plan_choose(d, c);
    if (chosen != MOLANN_OK) return chosen;

    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, dev));
    molann_plan* p = new (std::nothrow) molann_plan();
    if (!p) return (int)hipErrorOutOfMemory;
    memset(p, 0, sizeof(*p));
    p->launch_mu = new std::mutex();
    p->jit_mu = new std::mutex();
    p->device = dev;
    p->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    adopt_choice(p, d, c);
    snprintf(p->last_info, sizeof(p->last_info), "(no launch yet)");
    snprintf(p->jit_note, sizeof(p->jit_note), "jit: not applicable");
    snprintf(p->chain_note, sizeof(p->chain_note), "chain: not applicable");

    // every failure from here on leaves through the one teardown
    int rc = MOLANN_OK;
    if (p->mlp_lds_per_wave > 65536) // a single wave's two activation buffers exceed the default 64 KiB cap
        rc = (int)hipFuncSetAttribute(p->mlp_prec == MOLANN_MLP_BF16 ? (const void*)mlp_mfma_kernel<true> : (const void*)mlp_mfma_kernel<false>,
                                      hipFuncAttributeMaxDynamicSharedMemorySize, 163840);
    if (rc == MOLANN_OK) rc = create_blob(p, d, c);
    if (rc == MOLANN_OK && p->work_frames > 0) rc = create_streams(p);
    if (rc == MOLANN_OK && c.jit_possible) build_lane_kernel(p, c);
    if (rc == MOLANN_OK && p->jit_only && !p->jit_fn) { // hipRTC is present but the build failed: no other lane kernel for this plan
        if (p->fused_mlp) rc = MOLANN_E_UNSUPPORTED;    // its MLP was planned into that kernel: nothing to fall back to
        p->jit_only = false;
        if (!p->geom[0].ok) p->family = 1; // features from the wave-per-frame kernel
    }
    if (rc != MOLANN_OK) {
        molann_plan_destroy(p);
        return rc;
    }
    if (!c.align_out.slots.empty() && (p->align_spec = new (std::nothrow) JitSpecBox())) p->align_spec->j = c.align_out;
    // a small head that no lane kernel fuses: its description for the MLP's backward kernel
    if (c.small_head && (p->mlp_spec = new (std::nothrow) JitSpecBox())) {
        JitSpec& mj = p->mlp_spec->j;
        mj.n_layers = d->n_layers; mj.act = d->activation; mj.d_feat = c.d_feat;
        mj.dims.assign(p->dims, p->dims + d->n_layers + 1);
        set_layout(*p->mlp_spec, p->kp, p->jp, p->moff, d->n_layers);
    }
    if (c.chain_fb > 0 && !c.nojit && !p->lane_mlp) build_chain_kernel(p, c);
    if (c.wide_fused && p->family == 0) build_wide_kernel(p, c);
    *out_plan = p;
    return MOLANN_OK;
}

// Also the way out of a creation that failed half-way: a plan without a blob has nothing queued on the device, and whatever
// stream, event or module it lacks is a null handle.
int molann_plan_destroy(molann_plan* p) {
    if (!p) return MOLANN_OK;
    if (p->blob) {
        // kernels of this plan may still be running or queued (`y = model(x); del model`): its code objects and device
        // memory go only when the device has drained.  Destroying a plan is setup-time work, like creating one.
        int cur = -1;
        const bool sw = hipGetDevice(&cur) == hipSuccess && cur != p->device && hipSetDevice(p->device) == hipSuccess;
        (void)hipDeviceSynchronize();
        if (sw) (void)hipSetDevice(cur);
    }
    for (hipModule_t m : {p->jit_mod, p->bwd_mod, p->mbwd_mod, p->cbwd_mod, p->rbwd_mod, p->vjp_mod, p->gvjp_mod, p->wide_mod, p->feat_mod,
                          p->train_mod, p->align_mod, p->chain_mod})
        if (m) (void)hipModuleUnload(m);
    delete p->align_spec;
    delete p->mlp_spec;
    delete p->spec;
    if (p->d_bwork) (void)hipFree(p->d_bwork);
    if (p->d_gpart) (void)hipFree(p->d_gpart);
    if (p->side) (void)hipStreamSynchronize(p->side);
    for (hipEvent_t e : {p->ev_bwork, p->ev_feat[0], p->ev_feat[1], p->ev_mlp[0], p->ev_mlp[1], p->ev_done})
        if (e) (void)hipEventDestroy(e);
    if (p->side) (void)hipStreamDestroy(p->side);
    delete p->launch_mu;
    delete p->jit_mu;
    const hipError_t e = p->blob ? hipFree(p->blob) : hipSuccess;
    delete p;
    return (int)e;
}

} // extern "C"
