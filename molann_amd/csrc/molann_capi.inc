// molann_capi.inc - part of libmolann_hip.so, included by molann_kernels.hip (one translation unit: the kernels' host stubs and the
// launches that use them must see each other).  The C ABI (include/molann_hip.h).
// =============================================================================================
// C ABI
// =============================================================================================
extern "C" {

int molann_abi_version(void) { return MOLANN_ABI_VERSION; }

const char* molann_build_kind(void) {
#ifdef MOLANN_DIAGNOSTICS
    return "diagnostics";
#else
    return "release";
#endif
}

const char* molann_error_string(int code) {
    switch (code) {
    case MOLANN_OK: return "ok";
    case MOLANN_E_NULL: return "required pointer is NULL";
    case MOLANN_E_DESC: return "inconsistent plan description";
    case MOLANN_E_INDEX: return "atom index outside [0, n_inp)";
    case MOLANN_E_FEATURE: return "unknown feature type or wrong atom count for its type";
    case MOLANN_E_STAGE: return "plan lacks the stage this call needs";
    case MOLANN_E_ALIGNMENT: return "pointer is not 4-byte aligned";
    case MOLANN_E_UNSUPPORTED: return "shape not covered by the gfx950 kernels";
    case MOLANN_E_NOT_PACKED: return "MLP weights were never packed (call molann_plan_update_mlp)";
    case MOLANN_E_DEVICE: return "no gfx950 device";
    default: return code > 0 ? hipGetErrorString((hipError_t)code) : "unknown error";
    }
}

int molann_plan_create(const molann_plan_desc* d, molann_plan** out_plan) {
    if (!out_plan) return MOLANN_E_NULL;
    *out_plan = nullptr;
    const int v = validate_desc(d);
    if (v != MOLANN_OK) return v;

    // ---- expand the feature list into items (column order = list order, ann.py:473) ------------
    std::vector<ItemDev> items;
    const int d_feat = expand_items(d, items);
    if (d->n_layers > 0 && d->n_features > 0 && d->layer_dims[0] != d_feat) return MOLANN_E_DESC;

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
    p->n_inp = d->n_inp;
    p->n_align = d->n_align;
    p->align_first = d->n_align > 0 ? d->align_idx[0] : 0;
    p->n_features = d->n_features;
    p->n_items = (int)items.size();
    for (const ItemDev& it : items) p->has_position_items = p->has_position_items || it.type == IT_POSITION;
    p->d_feat = d_feat;
    p->use_angle_value = d->use_angle_value;
    p->n_layers = d->n_layers;
    p->act = d->activation;
    p->mlp_prec = d->mlp_precision;
    if (d->n_layers > 0)
        for (int i = 0; i <= d->n_layers; ++i) p->dims[i] = d->layer_dims[i];
    p->out_dim = d->n_layers > 0 ? d->layer_dims[d->n_layers] : d_feat;

    // ---- kernel family and MLP placement -------------------------------------------------------
    int max_w = 0;
    for (int i = 1; i <= d->n_layers; ++i) max_w = std::max(max_w, d->layer_dims[i]);
    const bool cheap_act = d->activation != MOLANN_ACT_ELU && d->activation != MOLANN_ACT_SOFTPLUS &&
                           d->activation != MOLANN_ACT_GELU;
    const bool small_mlp = d->n_layers > 0 && d->n_layers <= LANE_MLP_MAX_LAYERS && max_w <= LANE_MLP_MAX_WIDTH &&
                           d_feat <= LANE_MLP_MAX_WIDTH && d->mlp_precision == MOLANN_MLP_F32 && cheap_act;
    // feature dims 33..64 in front of such an MLP: fused too, by the plan-specialised kernel only (16 k-steps in layer 0)
    const bool wide_in_mlp = !small_mlp && d->n_layers > 0 && d->n_layers <= LANE_MLP_MAX_LAYERS && max_w <= LANE_MLP_MAX_WIDTH &&
                             d_feat <= 2 * LANE_MLP_MAX_WIDTH && d->mlp_precision == MOLANN_MLP_F32 && cheap_act;
    const int cols_needed = std::max(1, small_mlp ? ceil_to(d_feat, 4) : d_feat);
    // touched atoms -> slots in first-use order: align atoms, then the feature table's atoms
    std::vector<int> slot_of(d->n_inp, -1), slots;
    auto slot = [&](int atom) {
        if (slot_of[atom] < 0) { slot_of[atom] = (int)slots.size(); slots.push_back(atom); }
        return slot_of[atom];
    };
    bool align_is_prefix = true; // align atom i must be slot i (no repeated align atoms)
    for (int i = 0; i < d->n_align; ++i) align_is_prefix = align_is_prefix && (slot(d->align_idx[i]) == i);
    std::vector<ItemDev> items_slot(items);
    for (auto& it : items_slot)
        for (int i = 0; i < 4; ++i) it.idx[i] = slot(it.idx[i]);
    p->n_slots = (int)slots.size();
    // (plan creation is setup time: MOLANN_NO_REGS / MOLANN_NO_JIT select the other generic modes here)
    p->regs_mode = p->n_items > 0 && p->n_items <= 64 && p->n_slots <= 16 && align_is_prefix &&
                   getenv("MOLANN_NO_REGS") == nullptr;
    memset(p->geom, 0, sizeof(p->geom));
    const bool lane_tables_fit = d->n_align <= 64 && (long)d->n_inp * 768 <= 65536;
    if (p->n_items > 0 && lane_tables_fit && cols_needed <= LANE_MAX_COLS)
        lane_geometry(p->geom[0], 64 * d->n_inp * 12, cols_needed);
    if (d->n_align > 0 && lane_tables_fit) lane_geometry(p->geom[1], 64 * d->n_inp * 12, 1);
    // The plan-specialised lane kernel stages only the touched 16-byte windows of a frame, so its tile does not grow
    // with n_inp: a plan that touches few atoms (<= 32) of a LARGE frame is a lane-per-frame plan too, as long as
    // hipRTC is there to build it (the ahead-of-time lane kernel needs the dense tile and cannot serve it).
    const char* nojit_env = getenv("MOLANN_NO_JIT");
    bool jit_possible = rtc_api()->ok && !(nojit_env && nojit_env[0] == '1') && p->n_items > 0 &&
                        p->n_items <= JIT_MAX_ITEMS && p->n_slots <= JIT_MAX_SLOTS && align_is_prefix &&
                        cols_needed <= LANE_MAX_COLS && 3 * d->n_inp >= 4;
    if (jit_possible) { // and its LDS geometry (compact tile + staging rows) must leave room for >= 4 waves per CU
        JitSpec probe;
        probe.win = compact_windows(slots, d->n_inp);
        molann_plan::LaneGeom pg;
        memset(&pg, 0, sizeof(pg));
        jit_geometry(probe, pg, ((small_mlp || wide_in_mlp) && d->n_features > 0) ? d_feat : cols_needed, cols_needed);
        jit_possible = pg.ok != 0;
    }
    const bool lane_by_jit_only = jit_possible && !p->geom[0].ok;
    const bool fused_by_jit_only = jit_possible && wide_in_mlp && d->n_features > 0;
    // the family names the kernel that serves the plan's main product (features if it has any)
    p->family = (p->n_items > 0 ? (p->geom[0].ok || lane_by_jit_only) : p->geom[1].ok) ? 0 : 1;
    p->fused_mlp = ((p->family == 0) && small_mlp && d->n_features > 0) || fused_by_jit_only;
    // a head within the fused MLP's limits behind a kernel that cannot fuse it (wave per frame), or called on its own
    // (molann_mlp_packed_f32): mlp_lane_kernel on the same weight fragments
    p->lane_mlp = small_mlp && !(getenv("MOLANN_NO_LANE_MLP") && getenv("MOLANN_NO_LANE_MLP")[0] == '1');
    p->jit_only = lane_by_jit_only || fused_by_jit_only;

    // ---- device blob ----------------------------------------------------------------------------
    size_t off = 0;
    auto carve = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_align = carve(sizeof(int) * std::max(1, d->n_align));
    const size_t o_ref = carve(sizeof(float) * (3 * (size_t)d->n_align + 8));
    const size_t o_ref64 = carve(sizeof(double) * (3 * (size_t)d->n_align + 8));
    const size_t o_items = carve(sizeof(ItemDev) * std::max<size_t>(1, items.size()));
    const size_t o_items_slot = carve(sizeof(ItemDev) * std::max<size_t>(1, items.size()));
    const size_t o_slots = carve(sizeof(int) * std::max<size_t>(1, slots.size()));
    // frames_ring_kernel tables (plans the lane kernels do not serve): windows, image positions
    std::vector<int> ring_win, ring_align_pos;
    std::vector<ItemDev> ring_items;
    p->ring_nd = 0;
    if (p->family == 1 && p->n_items > 0 && align_is_prefix) {
        const std::vector<int> win = compact_windows(slots, d->n_inp);
        static const int buckets[] = {1, 2, 3, 4, 6, 8, 10, 12, 14, 16, 18, 20, 22, 24, 26, 28, 30, 32};
        int nd = 0;
        for (int b : buckets)
            if (nd == 0 && (long)b * 64 >= (long)win.size()) nd = b;
        if (nd > 0) {
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
            for (int w : win) ring_win.push_back(4 * w);
            for (int i = 0; i < d->n_align; ++i) ring_align_pos.push_back(pos_of(d->align_idx[i]));
            ring_items = items;
            for (auto& it : ring_items)
                for (int i = 0; i < 4; ++i) it.idx[i] = pos_of(it.idx[i]);
            p->ring_nd = nd;
            p->ring_nwin = (int)win.size();
        }
    }
    const size_t o_ring_win = carve(sizeof(int) * std::max<size_t>(1, ring_win.size()));
    const size_t o_ring_apos = carve(sizeof(int) * std::max<size_t>(1, ring_align_pos.size()));
    const size_t o_ring_items = carve(sizeof(ItemDev) * std::max<size_t>(1, ring_items.size()));
    // backward of large frames without atomics: who contributes to which touched atom
    std::vector<int> bw_atoms, bw_ptr, bw_list, bw_align;
    if (!p->geom[0].ok && p->n_items > 0 && d->n_layers >= 0) {
        std::vector<std::vector<int>> contrib(d->n_inp);
        std::vector<int> al_of(d->n_inp, -1);
        std::vector<char> touched(d->n_inp, 0);
        for (size_t it = 0; it < items.size(); ++it)
            for (int j = 0; j < item_atoms(items[it].type); ++j) { contrib[items[it].idx[j]].push_back((int)(4 * it + j)); touched[items[it].idx[j]] = 1; }
        for (int i = 0; i < d->n_align; ++i) { if (al_of[d->align_idx[i]] < 0) al_of[d->align_idx[i]] = i; touched[d->align_idx[i]] = 1; }
        bool repeated_align = false;
        { std::vector<char> seen(d->n_inp, 0); for (int i = 0; i < d->n_align; ++i) { repeated_align = repeated_align || seen[d->align_idx[i]]; seen[d->align_idx[i]] = 1; } }
        if (!repeated_align) {   // (an alignment set that names an atom twice keeps the atomics: the atom has two reference rows)
            bw_ptr.push_back(0);
            for (int a0 = 0; a0 < d->n_inp; ++a0)
                if (touched[a0]) {
                    bw_atoms.push_back(a0);
                    bw_align.push_back(al_of[a0]);
                    bw_list.insert(bw_list.end(), contrib[a0].begin(), contrib[a0].end());
                    bw_ptr.push_back((int)bw_list.size());
                }
        }
    }
    p->bw_touched = (int)bw_atoms.size();
    p->bw_list_len = (int)bw_list.size();
    // values + vjp in one launch (molann_group_vjp.inc): the same lists for every alignment set, rows named twice included
    std::vector<int> va_atoms, va_ptr, va_list;
    if (!p->geom[0].ok && p->n_items > 0) group_vjp_tables(d->n_inp, items, d->align_idx, d->n_align, va_atoms, va_ptr, va_list);
    p->va_touched = (int)va_atoms.size();
    p->va_list_len = (int)va_list.size();
    const size_t o_va_atoms = carve(sizeof(int) * std::max<size_t>(1, va_atoms.size()));
    const size_t o_va_ptr = carve(sizeof(int) * std::max<size_t>(1, va_ptr.size()));
    const size_t o_va_list = carve(sizeof(int) * std::max<size_t>(1, va_list.size()));
    // second order without atomics: every atom's item slots, then its align slots, in a fixed order (molann_hvp.inc)
    std::vector<int> hv_ptr, hv_list;
    if (p->n_items > 0) hvp_tables(d->n_inp, items, d->align_idx, d->n_align, hv_ptr, hv_list);
    const size_t o_hv_ptr = carve(sizeof(int) * std::max<size_t>(1, hv_ptr.size()));
    const size_t o_hv_list = carve(sizeof(int) * std::max<size_t>(1, hv_list.size()));
    // AlignmentLayer.forward under autograd arrives as a feature plan with ONE position item per atom, in atom order: its
    // feature rows are the aligned frame, its backward the dense gradient of the alignment (frames_align_bwd_regs_kernel)
    std::vector<int> align_slot;
    p->dense_positions = false;
    if (d->n_align > 0 && d->n_layers == 0 && (int)items.size() == d->n_inp && !p->geom[0].ok) {
        bool dense = true, repeated = false;
        for (int i = 0; i < d->n_inp && dense; ++i) dense = items[i].type == IT_POSITION && items[i].idx[0] == i && items[i].col == 3 * i;
        align_slot.assign(d->n_inp, -1);
        for (int i = 0; i < d->n_align; ++i) { repeated = repeated || align_slot[d->align_idx[i]] >= 0; align_slot[d->align_idx[i]] = i; }
        p->dense_positions = dense && !repeated && getenv("MOLANN_NO_DENSE_ALIGN") == nullptr;
        if (!p->dense_positions) align_slot.clear();
    }
    const size_t o_align_slot = carve(sizeof(int) * std::max<size_t>(1, align_slot.size()));
    const size_t o_bw_atoms = carve(sizeof(int) * std::max<size_t>(1, bw_atoms.size()));
    const size_t o_bw_ptr = carve(sizeof(int) * std::max<size_t>(1, bw_ptr.size()));
    const size_t o_bw_list = carve(sizeof(int) * std::max<size_t>(1, bw_list.size()));
    const size_t o_bw_align = carve(sizeof(int) * std::max<size_t>(1, bw_align.size()));

    size_t lane_floats = 0;
    if (p->fused_mlp || p->lane_mlp) lane_floats = (size_t)d->n_layers * (1024 + 512) + 1024;
    const size_t o_wlane = carve(sizeof(float) * std::max<size_t>(1, lane_floats));
    size_t mfma_bytes = 0;
    const bool bf16 = d->mlp_precision == MOLANN_MLP_BF16;
    const int kgran = bf16 ? 32 : 16;
    int max_kp = 16;
    if (d->n_layers > 0) {
        const size_t es = bf16 ? 2 : 4;
        for (int l = 0; l < d->n_layers; ++l) {
            p->kp[l] = ceil_to(p->dims[l], kgran);
            p->jp[l] = ceil_to(p->dims[l + 1], 16);
            max_kp = std::max(max_kp, std::max(p->kp[l], p->jp[l]));
        }
        // the activations written by layer l (Jp columns) are read as layer l+1's Kp columns
        for (int l = 0; l + 1 < d->n_layers; ++l) max_kp = std::max(max_kp, p->kp[l + 1]);
        for (int l = 0; l < d->n_layers; ++l) {
            p->moff[l] = (long)(mfma_bytes / es);
            mfma_bytes += ((size_t)p->jp[l] * p->kp[l]) * es + (size_t)p->jp[l] * 4;
            mfma_bytes = (mfma_bytes + 15) & ~(size_t)15;
        }
        // two activation buffers: [0] holds the inputs of even layers, [1] of odd layers (layer l writes what
        // layer l+1 reads).  Row strides: 16-byte multiples, off the power of two.
        int need[2] = {16, 16};
        for (int l = 0; l < d->n_layers; ++l) {
            need[l & 1] = std::max(need[l & 1], p->kp[l]);
            if (l + 1 < d->n_layers) need[(l + 1) & 1] = std::max(need[(l + 1) & 1], std::max(p->jp[l], p->kp[l + 1]));
        }
        (void)max_kp;
        for (int i = 0; i < 2; ++i) p->mlp_ld[i] = need[i] + (bf16 ? 8 : 4);
        p->mlp_lds_per_wave = 16 * (p->mlp_ld[0] + p->mlp_ld[1]) * (int)es;
        if (p->mlp_lds_per_wave > 163840) { delete p; return MOLANN_E_UNSUPPORTED; }
        if (p->mlp_lds_per_wave > 65536) { // a single wave's two activation buffers exceed the default 64 KiB cap
            hipError_t ea = bf16 ? hipFuncSetAttribute((const void*)mlp_mfma_kernel<true>,
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, 163840)
                                 : hipFuncSetAttribute((const void*)mlp_mfma_kernel<false>,
                                                       hipFuncAttributeMaxDynamicSharedMemorySize, 163840);
            if (ea != hipSuccess) { delete p; return (int)ea; }
        }
    }
    const size_t o_wmfma = carve(std::max<size_t>(16, mfma_bytes));
    // wide bf16 MLP next to a gather kernel: the chain kernel's weight stream (molann_mlp_jit.inc), when its
    // two LDS slabs fit and at least one 16-frame block per wave fits the register file
    ChainGeom cg;
    memset(&cg, 0, sizeof(cg));
    size_t chain_bytes = 0;
    int chain_fb = 0;
    if (d->n_layers > 0 && !p->fused_mlp) {
        cg.nl = d->n_layers;
        cg.bf16 = bf16 ? 1 : 0;
        for (int i = 0; i <= d->n_layers; ++i) cg.dims[i] = p->dims[i];
        for (int fb = 4; fb >= 1 && chain_fb == 0; --fb) // upper bound; plan creation steps down while the build spills
            if (fb * cg.regs_per_fb() <= (chain_resident(cg) ? 256 : 512)) chain_fb = fb;     // resident: two waves per SIMD
        if (!chain_resident(cg) && 2 * cg.slab_max() * 1024 > 163840 - 1024) chain_fb = 0;
        if (chain_fb > 0) {
            p->chain_stream_bytes = cg.total_frags() * 1024;
            chain_bytes = (size_t)p->chain_stream_bytes + (size_t)cg.bias_off(cg.nl) * 4;
        }
    }
    const size_t o_wchain = carve(std::max<size_t>(16, chain_bytes));
    p->work_frames = 0;
    size_t work_bytes = 0;
    if (d->n_layers > 0 && d->n_features > 0 && !p->fused_mlp) {
        // feature chunk handed from the preprocessing kernel to the MLP kernel: sized to stay
        // resident in the 256 MiB Infinity Cache
        long wf = (64l << 20) / ((long)d_feat * 4);
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
        if (p->family == 1)
            wf = std::max<long>(wf, std::min<long>(1l << 18, ((256l << 20) / ((long)d_feat * 4)) & ~63l));
        p->work_frames = wf;
        work_bytes = 2 * (size_t)wf * d_feat * 4;
    }
    const size_t o_work = carve(std::max<size_t>(16, work_bytes));

    hipError_t e = hipMalloc((void**)&p->blob, off);
    if (e != hipSuccess) { delete p; return (int)e; }
    p->d_align_idx = (int*)(p->blob + o_align);
    p->d_ref = (float*)(p->blob + o_ref);
    p->d_ref64 = (double*)(p->blob + o_ref64);
    p->d_items = (ItemDev*)(p->blob + o_items);
    p->d_items_slot = (ItemDev*)(p->blob + o_items_slot);
    p->d_slots = (int*)(p->blob + o_slots);
    p->d_ring_win = (int*)(p->blob + o_ring_win);
    p->d_ring_align_pos = (int*)(p->blob + o_ring_apos);
    p->d_ring_items = (ItemDev*)(p->blob + o_ring_items);
    p->d_bw_atoms = (int*)(p->blob + o_bw_atoms); p->d_bw_ptr = (int*)(p->blob + o_bw_ptr);
    p->d_bw_list = (int*)(p->blob + o_bw_list); p->d_bw_align = (int*)(p->blob + o_bw_align);
    p->d_align_slot = (int*)(p->blob + o_align_slot);
    p->d_va_atoms = (int*)(p->blob + o_va_atoms); p->d_va_ptr = (int*)(p->blob + o_va_ptr); p->d_va_list = (int*)(p->blob + o_va_list);
    p->d_hv_ptr = (int*)(p->blob + o_hv_ptr); p->d_hv_list = (int*)(p->blob + o_hv_list);
    p->d_wlane = (float*)(p->blob + o_wlane);
    p->d_wmfma = (void*)(p->blob + o_wmfma);
    p->d_work = (float*)(p->blob + o_work);
    p->d_wchain = p->blob + o_wchain;

    // ---- upload (synchronous: plan creation is setup time) --------------------------------------
    if (d->n_align > 0) {
        std::vector<float> refc(3 * (size_t)d->n_align + 8, 0.f);
        std::vector<double> refd(3 * (size_t)d->n_align + 8, 0.);
        // centred here whatever the caller passes (pack_ref_kernel: the alignment does not depend on it)
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
        e = hipMemcpy(p->d_align_idx, d->align_idx, sizeof(int) * d->n_align, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(p->d_ref, refc.data(), sizeof(float) * refc.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(p->d_ref64, refd.data(), sizeof(double) * refd.size(), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess && !items.empty())
        e = hipMemcpy(p->d_items, items.data(), sizeof(ItemDev) * items.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess && !items.empty())
        e = hipMemcpy(p->d_items_slot, items_slot.data(), sizeof(ItemDev) * items.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess && !slots.empty())
        e = hipMemcpy(p->d_slots, slots.data(), sizeof(int) * slots.size(), hipMemcpyHostToDevice);
    if (e == hipSuccess && p->ring_nd > 0) {
        e = hipMemcpy(p->d_ring_win, ring_win.data(), sizeof(int) * ring_win.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess && !ring_align_pos.empty())
            e = hipMemcpy(p->d_ring_align_pos, ring_align_pos.data(), sizeof(int) * ring_align_pos.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(p->d_ring_items, ring_items.data(), sizeof(ItemDev) * ring_items.size(), hipMemcpyHostToDevice);
    }

    if (e == hipSuccess && p->bw_touched > 0) {
        e = hipMemcpy(p->d_bw_atoms, bw_atoms.data(), sizeof(int) * bw_atoms.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(p->d_bw_ptr, bw_ptr.data(), sizeof(int) * bw_ptr.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess && !bw_list.empty()) e = hipMemcpy(p->d_bw_list, bw_list.data(), sizeof(int) * bw_list.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess && !align_slot.empty()) e = hipMemcpy(p->d_align_slot, align_slot.data(), sizeof(int) * align_slot.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(p->d_bw_align, bw_align.data(), sizeof(int) * bw_align.size(), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess && p->va_touched > 0) {
        e = hipMemcpy(p->d_va_atoms, va_atoms.data(), sizeof(int) * va_atoms.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(p->d_va_ptr, va_ptr.data(), sizeof(int) * va_ptr.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(p->d_va_list, va_list.data(), sizeof(int) * va_list.size(), hipMemcpyHostToDevice);
    }
    if (e == hipSuccess && !hv_ptr.empty()) {
        e = hipMemcpy(p->d_hv_ptr, hv_ptr.data(), sizeof(int) * hv_ptr.size(), hipMemcpyHostToDevice);
        if (e == hipSuccess && !hv_list.empty()) e = hipMemcpy(p->d_hv_list, hv_list.data(), sizeof(int) * hv_list.size(), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) { (void)hipFree(p->blob); delete p; return (int)e; }
    snprintf(p->last_info, sizeof(p->last_info), "(no launch yet)");
    if (p->work_frames > 0) {
        e = hipStreamCreateWithFlags(&p->side, hipStreamNonBlocking);
        for (int h = 0; h < 2 && e == hipSuccess; ++h) {
            e = hipEventCreateWithFlags(&p->ev_feat[h], hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&p->ev_mlp[h], hipEventDisableTiming);
            if (e == hipSuccess && h == 0) e = hipEventCreateWithFlags(&p->ev_done, hipEventDisableTiming);
        }
        if (e != hipSuccess) { (void)hipFree(p->blob); delete p; return (int)e; }
    }
    // ---- plan-specialised lane kernel --------------------------------------------------------------
    snprintf(p->jit_note, sizeof(p->jit_note), "jit: not applicable");
    const char* nojit = nojit_env;
    if (jit_possible) {
        JitSpec j;
        j.n_inp = d->n_inp; j.n_align = d->n_align; j.act = d->activation; j.d_feat = d_feat;
        j.n_layers = p->fused_mlp ? d->n_layers : 0;
        j.out_cols = p->fused_mlp ? p->out_dim : d_feat;
        j.slots = slots; j.items = items_slot;
        // compact tile: only the 16-byte windows of a frame that hold a touched atom go to LDS, so more waves fit
        j.win = compact_windows(slots, d->n_inp);
        jit_geometry(j, p->jit_geom, p->fused_mlp ? d_feat : cols_needed, cols_needed);
        if (p->fused_mlp) j.dims.assign(p->dims, p->dims + d->n_layers + 1);
        p->spec = new (std::nothrow) JitSpecBox();
        if (p->spec) {
            p->spec->j = j;
            for (int l = 0; l < j.n_layers; ++l) { p->spec->kp.push_back(p->kp[l]); p->spec->jp.push_back(p->jp[l]); p->spec->woff.push_back(p->moff[l]); }
            p->n_grad_params = 0;
            for (int l = 0; l < j.n_layers; ++l) p->n_grad_params += p->dims[l + 1] * p->dims[l] + p->dims[l + 1];
        }
        int rc = -1;
        const bool frame_ok = p->jit_geom.ok && 3 * d->n_inp >= 4;
        if (frame_ok) {
            std::vector<char> code;
            std::string log;
            // no SLP vectorisation: hipcc otherwise packs a fifth of this straight-line fp32 code into v_pk_* pairs, which
            // buys ~1.2x on those operations at two waves per SIMD and pays for it with ~130 register moves per tile and 44
            // more registers (C3: 166 -> 122 VGPRs, 74 -> 70 us; tools/ab_flags.sh)
            rc = jit_compile(jit_source(j), code, log, "-fno-slp-vectorize");
            hipModule_t mod = nullptr;
            hipFunction_t fn = nullptr;
            bool loaded = rc == 0 && hipModuleLoadData(&mod, code.data()) == hipSuccess && hipModuleGetFunction(&fn, mod, "molann_lane_jit") == hipSuccess;
            int scratch = 0;
            if (loaded && j.ncons > 10 && hipFuncGetAttribute(&scratch, HIP_FUNC_ATTRIBUTE_LOCAL_SIZE_BYTES, fn) == hipSuccess && scratch > 0) {
                // Three or four layers of 32 units: the weight fragments do not fit the 128 registers of four waves per SIMD and the
                // build spills.  Ten consumers (three waves per SIMD, 168 registers) serve the stream as well as fourteen.
                JitSpec j3 = j;
                molann_plan::LaneGeom g3;
                memset(&g3, 0, sizeof(g3));
                jit_geometry(j3, g3, p->fused_mlp ? d_feat : cols_needed, cols_needed, 10);
                std::vector<char> code3;
                hipModule_t mod3 = nullptr;
                hipFunction_t fn3 = nullptr;
                int scratch3 = 0;
                if (g3.ok && jit_compile(jit_source(j3), code3, log, "-fno-slp-vectorize") == 0 && hipModuleLoadData(&mod3, code3.data()) == hipSuccess &&
                    hipModuleGetFunction(&fn3, mod3, "molann_lane_jit") == hipSuccess &&
                    hipFuncGetAttribute(&scratch3, HIP_FUNC_ATTRIBUTE_LOCAL_SIZE_BYTES, fn3) == hipSuccess && scratch3 < scratch) {
                    (void)hipModuleUnload(mod);
                    mod = mod3; fn = fn3; code.swap(code3);
                    j = j3; p->jit_geom = g3;
                    if (p->spec) p->spec->j = j;
                } else if (mod3) {
                    (void)hipModuleUnload(mod3);
                }
            }
            if (!loaded) {
                if (getenv("MOLANN_JIT_VERBOSE")) fprintf(stderr, "molann jit failed rc=%d\n%s\n", rc, log.c_str());
                if (mod) (void)hipModuleUnload(mod);
            } else {
                p->jit_mod = mod; p->jit_fn = fn; p->jit_nl = j.n_layers; p->jit_waves = 2;
                p->jit_ncons = j.ncons; p->jit_nload = j.nload; p->jit_nslot = j.nslot; p->jit_bpc = j.bpc; p->jit_lds_block = j.lds_block;
                snprintf(p->jit_note, sizeof(p->jit_note), "jit: specialised kernel, %d+1 waves per block, %zu bytes", j.ncons, code.size());
            }
        }
        if (!p->jit_fn) snprintf(p->jit_note, sizeof(p->jit_note), "jit: unavailable (rc=%d), generic kernel", rc);
    }
    if (p->jit_only && !p->jit_fn) { // hipRTC is present but the build failed: no other lane kernel for this plan
        if (p->fused_mlp) { // its MLP was planned into that kernel: nothing to fall back to
            molann_plan_destroy(p);
            return MOLANN_E_UNSUPPORTED;
        }
        p->jit_only = false;
        if (!p->geom[0].ok) p->family = 1; // features from the wave-per-frame kernel
    }
    // ---- AlignmentLayer.forward through the specialised kernel: the aligned frame is the feature row of one position item per
    // atom, so molann_align_f32 is the loader / consumer kernel too (built at its first call).  Small frames only.
    if (d->n_align > 0 && d->n_inp <= JIT_MAX_SLOTS && 3 * d->n_inp <= LANE_MAX_COLS && 3 * d->n_inp >= 4 && rtc_api()->ok &&
        !(nojit && nojit[0] == '1')) {
        JitSpec j;
        std::vector<int> seen(d->n_inp, 0);
        bool distinct = true;
        for (int i = 0; i < d->n_align; ++i) { distinct = distinct && !seen[d->align_idx[i]]; seen[d->align_idx[i]] = 1; j.slots.push_back(d->align_idx[i]); }
        for (int a = 0; a < d->n_inp; ++a) if (!seen[a]) j.slots.push_back(a);
        if (distinct) {
            for (int u = 0; u < d->n_inp; ++u) { ItemDev it = {IT_POSITION, 3 * j.slots[u], {u, u, u, u}, {0, 0}}; j.items.push_back(it); }
            j.n_inp = d->n_inp; j.n_align = d->n_align; j.act = 0; j.d_feat = 3 * d->n_inp; j.n_layers = 0; j.out_cols = 3 * d->n_inp;
            j.win = compact_windows(j.slots, d->n_inp);
            molann_plan::LaneGeom g;
            memset(&g, 0, sizeof(g));
            jit_geometry(j, g, j.d_feat, j.d_feat);
            if (g.ok && (p->align_spec = new (std::nothrow) JitSpecBox())) p->align_spec->j = j;
        }
    }
    // ---- a small head that no lane kernel fuses (wave-per-frame features): its description for the MLP's backward kernel
    if (p->lane_mlp && !p->fused_mlp && d->n_features > 0 && rtc_api()->ok && (p->mlp_spec = new (std::nothrow) JitSpecBox())) {
        JitSpec& mj = p->mlp_spec->j;
        mj.n_layers = d->n_layers; mj.act = d->activation; mj.d_feat = d_feat;
        mj.dims.assign(p->dims, p->dims + d->n_layers + 1);
        p->n_grad_params = 0;
        for (int l = 0; l < d->n_layers; ++l) {
            p->mlp_spec->kp.push_back(p->kp[l]); p->mlp_spec->jp.push_back(p->jp[l]); p->mlp_spec->woff.push_back(p->moff[l]);
            p->n_grad_params += p->dims[l + 1] * p->dims[l] + p->dims[l + 1];
        }
    }
    // ---- plan-specialised wide bf16 MLP ----------------------------------------------------------------
    snprintf(p->chain_note, sizeof(p->chain_note), "chain: not applicable");
    if (chain_fb > 0 && !(nojit && nojit[0] == '1') && !p->lane_mlp) {
        // most frames per wave (A-fragment reuse) that the register file holds without scratch
        int rc = -1;
        for (int fb = chain_fb; fb >= 1 && !p->chain_fn; --fb) {
            std::vector<char> code;
            std::string log;
            rc = jit_compile(jit_source_chain(cg, p->act, fb), code, log);
            hipModule_t mod = nullptr;
            hipFunction_t fn = nullptr;
            if (rc != 0 || hipModuleLoadData(&mod, code.data()) != hipSuccess ||
                hipModuleGetFunction(&fn, mod, "molann_mlp_chain") != hipSuccess) {
                if (getenv("MOLANN_JIT_VERBOSE")) fprintf(stderr, "molann chain jit failed rc=%d\n%s\n", rc, log.c_str());
                if (mod) (void)hipModuleUnload(mod);
                break;
            }
            int scratch = 0;
            (void)hipFuncGetAttribute(&scratch, HIP_FUNC_ATTRIBUTE_LOCAL_SIZE_BYTES, fn);
            if (scratch > 0 && fb > 1) { (void)hipModuleUnload(mod); continue; }
            p->chain_mod = mod; p->chain_fn = fn; p->chain_fb = fb; p->chain_waves = chain_waves(cg); p->chain_nslab = chain_nslab(cg);
            snprintf(p->chain_note, sizeof(p->chain_note), "chain: specialised kernel, FB=%d, %zu bytes", fb, code.size());
        }
        if (!p->chain_fn) snprintf(p->chain_note, sizeof(p->chain_note), "chain: unavailable (rc=%d), mlp_mfma_kernel", rc);
    }
    // ---- backward of a wide fp32 head whose chain stream is resident (molann_chain_bwd.inc), built at its first use: where it
    // serves the head, the parameter-gradient buffer has the head's layout (molann_mlp_backward_f32)
    if (chain_fb > 0 && chain_resident(cg) && !bf16 && !p->fused_mlp && !p->lane_mlp && rtc_api()->ok && !(nojit && nojit[0] == '1')) {
        const int act = d->activation;
        std::vector<int> kp(p->kp, p->kp + d->n_layers), jp(p->jp, p->jp + d->n_layers);
        if (act == 0 || act == 1 || act == 2 || act == 3 || act == 5 || act == 7) p->cbwd_waves = chain_bwd_waves(kp, jp);
        if (p->cbwd_waves > 0) {
            p->n_grad_params = 0;
            for (int l = 0; l < d->n_layers; ++l) p->n_grad_params += p->dims[l + 1] * p->dims[l] + p->dims[l + 1];
        }
    }
    // ---- the whole forward of a WIDE head in one lane kernel (round 3) ----------------------------------------------------
    // Hidden widths 33 .. ~128 behind a lane-per-frame preprocessing: features kernel + chain MLP kernel cost a launch, a
    // round trip of the features through the workspace and - the feature kernel holds every CU - no overlap.  Where the
    // chain's weight stream fits LDS beside a (shorter) ring, the specialised lane kernel runs the chain's arithmetic as its
    // MLP stage (molann_lane_jit.inc: WIDE_MLP).  Eight consumers + two loaders where the ring still has four slots.
    if (jit_possible && p->family == 0 && !p->fused_mlp && d->n_layers > 0 && d->n_features > 0 && !bf16 && chain_fb > 0 && chain_resident(cg) &&
        p->chain_stream_bytes <= 112 * 1024 && d_feat <= LANE_MAX_COLS && getenv("MOLANN_NO_WIDE_FUSED") == nullptr) {
        JitSpec j;
        j.n_inp = d->n_inp; j.n_align = d->n_align; j.act = d->activation; j.d_feat = d_feat;
        j.n_layers = d->n_layers; j.out_cols = p->out_dim;
        j.slots = slots; j.items = items_slot;
        j.win = compact_windows(slots, d->n_inp);
        j.dims.assign(p->dims, p->dims + d->n_layers + 1);
        j.wide_mlp = true; j.img_bytes = (int)p->chain_stream_bytes;
        int first = 8;     // (measured, [6,64,64,8] at 1 M frames: 188 / 175 / 176 / 182 us with 6 / 8 / 10 / 14 consumers)
        if (const char* e = diag_env("MOLANN_DEBUG_WIDE_CONS")) first = std::max(1, std::min(14, atoi(e)));
        for (int wide_cons : {first, 6}) {       // six consumers + two loaders = two waves per SIMD: 256 registers for the wider heads
            if (p->wide_fn) break;
            JitSpec jw = j;
            molann_plan::LaneGeom wg;
            memset(&wg, 0, sizeof(wg));
            jit_geometry(jw, wg, d_feat, cols_needed, wide_cons);
            if (!(wg.ok && jw.nslot >= 4)) continue;
            if (wide_cons == 6 && jw.ncons + jw.nload > 8) continue;
            std::vector<char> code;
            std::string log;
            hipModule_t mod = nullptr;
            hipFunction_t fn = nullptr;
            int scratch = 1;
            if (jit_compile(jit_source(jw), code, log, "-fno-slp-vectorize") == 0 && hipModuleLoadData(&mod, code.data()) == hipSuccess &&
                hipModuleGetFunction(&fn, mod, "molann_lane_jit") == hipSuccess &&
                hipFuncGetAttribute(&scratch, HIP_FUNC_ATTRIBUTE_LOCAL_SIZE_BYTES, fn) == hipSuccess && scratch == 0) {
                p->wide_mod = mod; p->wide_fn = fn;
                p->wide_ncons = jw.ncons; p->wide_nload = jw.nload; p->wide_nslot = jw.nslot; p->wide_bpc = jw.bpc; p->wide_lds_block = jw.lds_block;
            } else {
                if (getenv("MOLANN_JIT_VERBOSE")) fprintf(stderr, "molann wide fused forward with %d consumers not used (scratch=%d)\n%s\n", jw.ncons, scratch, log.c_str());
                if (mod) (void)hipModuleUnload(mod);
            }
        }
    }
    *out_plan = p;
    return MOLANN_OK;
}

int molann_plan_destroy(molann_plan* p) {
    if (!p) return MOLANN_OK;
    {   // kernels of this plan may still be running or queued (`y = model(x); del model`): its code objects and device
        // memory go only when the device has drained.  Destroying a plan is setup-time work, like creating one.
        int cur = -1;
        const bool sw = hipGetDevice(&cur) == hipSuccess && cur != p->device && hipSetDevice(p->device) == hipSuccess;
        (void)hipDeviceSynchronize();
        if (sw) (void)hipSetDevice(cur);
    }
    if (p->jit_mod) (void)hipModuleUnload(p->jit_mod);
    if (p->bwd_mod) (void)hipModuleUnload(p->bwd_mod);
    if (p->mbwd_mod) (void)hipModuleUnload(p->mbwd_mod);
    if (p->cbwd_mod) (void)hipModuleUnload(p->cbwd_mod);
    if (p->rbwd_mod) (void)hipModuleUnload(p->rbwd_mod);
    if (p->vjp_mod) (void)hipModuleUnload(p->vjp_mod);
    if (p->gvjp_mod) (void)hipModuleUnload(p->gvjp_mod);
    if (p->wide_mod) (void)hipModuleUnload(p->wide_mod);
    if (p->feat_mod) (void)hipModuleUnload(p->feat_mod);
    if (p->train_mod) (void)hipModuleUnload(p->train_mod);
    if (p->align_mod) (void)hipModuleUnload(p->align_mod);
    delete p->align_spec;
    delete p->mlp_spec;
    if (p->d_bwork) (void)hipFree(p->d_bwork);
    if (p->d_gpart) (void)hipFree(p->d_gpart);
    if (p->ev_bwork) (void)hipEventDestroy(p->ev_bwork);
    if (p->chain_mod) (void)hipModuleUnload(p->chain_mod);
    delete p->spec;
    if (p->side) {
        (void)hipStreamSynchronize(p->side);
        for (int h = 0; h < 2; ++h) { (void)hipEventDestroy(p->ev_feat[h]); (void)hipEventDestroy(p->ev_mlp[h]); }
        (void)hipEventDestroy(p->ev_done);
        (void)hipStreamDestroy(p->side);
    }
    delete p->launch_mu;
    delete p->jit_mu;
    hipError_t e = hipFree(p->blob);
    delete p;
    return (int)e;
}

int molann_plan_feature_dim(const molann_plan* p) { return p ? p->d_feat : MOLANN_E_NULL; }
int molann_plan_out_dim(const molann_plan* p) { return p ? p->out_dim : MOLANN_E_NULL; }
int molann_plan_kernel_family(const molann_plan* p) { return p ? p->family : MOLANN_E_NULL; }

int molann_plan_last_launch_info(const molann_plan* p, char* buf, int cap) {
    if (!p || !buf || cap <= 0) return MOLANN_E_NULL;
    snprintf(buf, (size_t)cap, "%s", p->last_info);
    return (int)strlen(buf);
}

int molann_plan_update_ref(molann_plan* p, const float* ref_x, molann_stream_t stream) {
    if (!p || !ref_x) return MOLANN_E_NULL;
    if (p->n_align <= 0) return MOLANN_E_STAGE;
    hipLaunchKernelGGL(pack_ref_kernel<float>, dim3(1), dim3(256), 0, (hipStream_t)stream, p->d_ref, p->d_ref64, ref_x, p->n_align);
    return (int)hipGetLastError();
}

int molann_plan_update_ref_f64(molann_plan* p, const double* ref_x, molann_stream_t stream) {
    if (!p || !ref_x) return MOLANN_E_NULL;
    if (p->n_align <= 0) return MOLANN_E_STAGE;
    hipLaunchKernelGGL(pack_ref_kernel<double>, dim3(1), dim3(256), 0, (hipStream_t)stream, p->d_ref, p->d_ref64, ref_x, p->n_align);
    return (int)hipGetLastError();
}

int molann_plan_update_mlp(molann_plan* p, const float* const* W, const float* const* b, molann_stream_t stream) {
    if (!p || !W || !b) return MOLANN_E_NULL;
    if (p->n_layers <= 0) return MOLANN_E_STAGE;
    PackArgs a;
    memset(&a, 0, sizeof(a));
    a.n_layers = p->n_layers;
    for (int i = 0; i <= p->n_layers; ++i) a.dims[i] = p->dims[i];
    for (int l = 0; l < p->n_layers; ++l) {
        if (!W[l] || !b[l]) return MOLANN_E_NULL;
        a.W[l] = W[l]; a.b[l] = b[l];
        a.kp[l] = p->kp[l]; a.jp[l] = p->jp[l]; a.moff[l] = p->moff[l];
    }
    a.fused = p->fused_mlp ? 1 : 0;
    a.bf16 = p->mlp_prec == MOLANN_MLP_BF16;
    if (p->fused_mlp || p->lane_mlp)
        hipLaunchKernelGGL(pack_lane_kernel, dim3(8), dim3(256), 0, (hipStream_t)stream, p->d_wlane, a);
    // the MFMA copy serves molann_mlp_packed_f32 and the unfused forward
    hipLaunchKernelGGL(pack_mfma_kernel, dim3(64, p->n_layers), dim3(256), 0, (hipStream_t)stream, p->d_wmfma, a);
    if (p->chain_fn || p->wide_fn) {
        ChainGeom g;
        memset(&g, 0, sizeof(g));
        g.nl = p->n_layers;
        g.bf16 = p->mlp_prec == MOLANN_MLP_BF16 ? 1 : 0;
        for (int i = 0; i <= p->n_layers; ++i) g.dims[i] = p->dims[i];
        ChainPackArgs c;
        memset(&c, 0, sizeof(c));
        c.n_layers = g.nl; c.npair = g.npair(); c.bf16 = g.bf16; c.stream_bytes = p->chain_stream_bytes;
        for (int i = 0; i <= g.nl; ++i) { c.dims[i] = g.dims[i]; c.bias_off[i] = g.bias_off(i); }
        for (int l = 0; l < g.nl; ++l) { c.W[l] = W[l]; c.b[l] = b[l]; }
        int start = 0;
        for (int q = 0; q < c.npair; ++q) {
            c.pair_start[q] = start; c.slab_frags[q] = g.slab_frags(q); c.ks_in[q] = g.ks(2 * q);
            start += g.nchunk(q) * g.slab_frags(q);
        }
        c.pair_start[c.npair] = start;
        hipLaunchKernelGGL(pack_chain_kernel, dim3(256), dim3(256), 0, (hipStream_t)stream, p->d_wchain, c);
    }
    const hipError_t e = hipGetLastError();
    if (e == hipSuccess) p->mlp_packed = true;
    return (int)e;
}

static int check_io(const void* x, const void* out, int64_t n) {
    if (n < 0) return MOLANN_E_DESC;
    if (n == 0) return MOLANN_OK;
    if (!x || !out) return MOLANN_E_NULL;
    if ((((uintptr_t)x) & 3) || (((uintptr_t)out) & 3)) return MOLANN_E_ALIGNMENT;
    return MOLANN_OK;
}

int molann_align_f32(const molann_plan* cp, const float* x, int64_t n, float* out_xyz, molann_stream_t stream) {
    if (!cp) return MOLANN_E_NULL;
    molann_plan* p = const_cast<molann_plan*>(cp);
    if (p->n_align <= 0) return MOLANN_E_STAGE;
    const int c = check_io(x, out_xyz, n);
    if (c != MOLANN_OK || n == 0) return c;
    if (p->align_spec && p->align_state >= 0 && (debug_env().ablate & ~(32 | 512)) == 0) {
        if (p->align_state == 0) {
            std::lock_guard<std::mutex> lock(*p->jit_mu);
            if (p->align_state == 0) {
                std::vector<char> code;
                std::string log;
                int st = -1;
                if (jit_compile(jit_source(p->align_spec->j), code, log, "-fno-slp-vectorize") == 0 && hipModuleLoadData(&p->align_mod, code.data()) == hipSuccess &&
                    hipModuleGetFunction(&p->align_fn, p->align_mod, "molann_lane_jit") == hipSuccess)
                    st = 1;
                else if (getenv("MOLANN_JIT_VERBOSE")) fprintf(stderr, "molann alignment jit failed\n%s\n", log.c_str());
                p->align_state = st;
            }
        }
        if (p->align_state == 1) {
            const JitSpec& j = p->align_spec->j;
            const long n_tiles = (n + 63) / 64;
            const int grid = grid_for(p, n_tiles, 1, j.bpc);
            struct { const float* x; float* out; const double* ref64; const float* wfrag; long n; int out_vec4, pad_;
                     unsigned long long* stamps; const float* ref32; float* feat; } ka = {x, out_xyz, p->d_ref64, nullptr, (long)n, 0, 0, nullptr, p->d_ref, nullptr};
            size_t ksz = sizeof(ka);
            void* cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &ka, HIP_LAUNCH_PARAM_BUFFER_SIZE, &ksz, HIP_LAUNCH_PARAM_END};
            const int block = 64 * (j.ncons + j.nload);
            const hipError_t le = hipModuleLaunchKernel(p->align_fn, grid, 1, 1, block, 1, 1, 0, (hipStream_t)stream, nullptr, cfg);
            snprintf(p->last_info, sizeof(p->last_info), "molann_lane_jit<align_out> (plan-specialised; %d consumer waves + %d loader, ring of %d tiles) grid=%d block=%d lds=%d",
                     j.ncons, j.nload, j.nslot, grid, block, j.lds_block);
            return (int)le;
        }
    }
    return launch_pre(p, x, n, out_xyz, 1, false, (hipStream_t)stream);
}

int molann_features_f32(const molann_plan* cp, const float* x, int64_t n, float* out, molann_stream_t stream) {
    if (!cp) return MOLANN_E_NULL;
    molann_plan* p = const_cast<molann_plan*>(cp);
    if (p->n_items <= 0) return MOLANN_E_STAGE;
    const int c = check_io(x, out, n);
    if (c != MOLANN_OK || n == 0) return c;
    return launch_pre(p, x, n, out, 0, false, (hipStream_t)stream);
}

int molann_mlp_packed_f32(const molann_plan* cp, const float* f, int64_t n, float* out, molann_stream_t stream) {
    if (!cp) return MOLANN_E_NULL;
    molann_plan* p = const_cast<molann_plan*>(cp);
    if (p->n_layers <= 0) return MOLANN_E_STAGE;
    if (!p->mlp_packed) return MOLANN_E_NOT_PACKED;
    const int c = check_io(f, out, n);
    if (c != MOLANN_OK || n == 0) return c;
    const int e = launch_mlp(p, f, n, p->dims[0], out, (hipStream_t)stream);
    snprintf(p->last_info, sizeof(p->last_info), "%s", p->mlp_info);
    return e;
}

int molann_forward_packed_f32(const molann_plan* cp, const float* x, int64_t n, float* out, molann_stream_t stream) {
    if (!cp) return MOLANN_E_NULL;
    molann_plan* p = const_cast<molann_plan*>(cp);
    if (p->n_layers <= 0 || p->n_items <= 0) return MOLANN_E_STAGE;
    if (!p->mlp_packed) return MOLANN_E_NOT_PACKED;
    const int c = check_io(x, out, n);
    if (c != MOLANN_OK || n == 0) return c;
    if (p->fused_mlp) return launch_pre(p, x, n, out, 0, true, (hipStream_t)stream);
    if (p->wide_fn && (debug_env().ablate == 0)) return launch_wide(p, x, (long)n, out, (hipStream_t)stream);
    // unfused: features of a chunk -> plan workspace (cache resident) -> MFMA MLP.  Two workspace halves:
    // the MLP of chunk i runs on the plan's side stream while this stream already gathers chunk i+1
    // (HBM-bound gather next to an MFMA/L2-bound kernel); events fork and join, so capture still works.
    char info[256];
    info[0] = 0;
    hipStream_t main = (hipStream_t)stream;
    std::lock_guard<std::mutex> lock(*p->launch_mu);
    if (p->have_done && p->last_stream != main) HIP_TRY(hipStreamWaitEvent(main, p->ev_done, 0)); // another stream used the workspace last
    int i = 0, rc = MOLANN_OK;
    bool mlp_recorded[2] = {false, false};
    if (n <= p->work_frames) {
        // one chunk: nothing to overlap, so both kernels go to the caller's stream back to back - handing the chunk to the side
        // stream and back costs two cross-stream waits (~15 us each on this stack: [6, 64, 64, 8] at 1 M frames 226 -> 196 us)
        rc = launch_pre(p, x, (long)n, p->d_work, 0, false, main);
        if (rc == MOLANN_OK) {
            snprintf(info, sizeof(info), "%s", p->last_info);
            rc = launch_mlp(p, p->d_work, (long)n, p->d_feat, out, main);
        }
        if (hipEventRecord(p->ev_done, main) == hipSuccess) { p->have_done = true; p->last_stream = main; }
        if (rc != MOLANN_OK) return rc;
        snprintf(p->last_info, sizeof(p->last_info), "%.130s || %.90s chunk=%ld", info, p->mlp_info, p->work_frames);
        return MOLANN_OK;
    }
    for (int64_t s = 0; s < n && rc == MOLANN_OK; s += p->work_frames, ++i) {
        const int h = i & 1;
        const long m = (long)std::min<int64_t>(p->work_frames, n - s);
        float* work = p->d_work + (size_t)h * p->work_frames * p->d_feat;
        if (i >= 2 && (rc = (int)hipStreamWaitEvent(main, p->ev_mlp[h], 0)) != 0) break; // this half is free again
        if ((rc = launch_pre(p, x + s * (long)p->n_inp * 3, m, work, 0, false, main)) != 0) break;
        if (s == 0) snprintf(info, sizeof(info), "%s", p->last_info);
        if ((rc = (int)hipEventRecord(p->ev_feat[h], main)) != 0) break;
        if ((rc = (int)hipStreamWaitEvent(p->side, p->ev_feat[h], 0)) != 0) break;
        rc = launch_mlp(p, work, m, p->d_feat, out + s * (long)p->out_dim, p->side);
        const int er = (int)hipEventRecord(p->ev_mlp[h], p->side); // also behind a failed launch: the join below needs it
        if (er == 0) mlp_recorded[h] = true;
        if (rc == 0) rc = er;
    }
    // join - on the error paths too: whatever reached the side stream is ordered before the caller's next work
    for (int h = 0; h < 2; ++h)
        if (mlp_recorded[h]) {
            const int er = (int)hipStreamWaitEvent(main, p->ev_mlp[h], 0);
            if (rc == 0) rc = er;
        }
    if (hipEventRecord(p->ev_done, main) == hipSuccess) { p->have_done = true; p->last_stream = main; }
    if (rc != MOLANN_OK) return rc;
    snprintf(p->last_info, sizeof(p->last_info), "%.130s || %.90s chunk=%ld", info, p->mlp_info, p->work_frames);
    return MOLANN_OK;
}

int molann_forward_f32(molann_plan* p, const float* x, int64_t n, const float* const* W, const float* const* b,
                       float* out, molann_stream_t stream) {
    const int e = molann_plan_update_mlp(p, W, b, stream);
    if (e != MOLANN_OK) return e;
    return molann_forward_packed_f32(p, x, n, out, stream);
}

// The fused forward that also keeps the features, for a backward that does not recompute them
int molann_forward_train_f32(molann_plan* p, const float* x, int64_t n, float* out, float* features, molann_stream_t stream) {
    if (!p) return MOLANN_E_NULL;
    if (p->n_layers <= 0 || p->n_items <= 0) return MOLANN_E_STAGE;
    if (!p->fused_mlp && !(p->family == 1 && p->lane_mlp)) return MOLANN_E_UNSUPPORTED;
    if (!p->mlp_packed) return MOLANN_E_NOT_PACKED;
    const int c = check_io(x, out, n);
    if (c != MOLANN_OK || n == 0) return c;
    if (!features) return MOLANN_E_NULL;
    if (((uintptr_t)features) & 3) return MOLANN_E_ALIGNMENT;
    if (!p->fused_mlp) { // a small head behind a wave-per-frame kernel: the features land where the caller keeps them, the head reads them there
        std::lock_guard<std::mutex> lock(*p->launch_mu);
        int rc = launch_pre(p, x, (long)n, features, 0, false, (hipStream_t)stream);
        char info[160];
        snprintf(info, sizeof(info), "%.159s", p->last_info);
        if (rc == MOLANN_OK) rc = launch_mlp(p, features, (long)n, p->d_feat, out, (hipStream_t)stream);
        if (rc == MOLANN_OK) snprintf(p->last_info, sizeof(p->last_info), "%.130s || %.90s", info, p->mlp_info);
        return rc;
    }
    return launch_pre(p, x, (long)n, out, 0, true, (hipStream_t)stream, features);
}


// ---- float64 entry points (the reference's modules follow x.dtype) -------------------------------------------------
static int check_io_f64(const void* x, const void* out, int64_t n) {
    if (n < 0) return MOLANN_E_DESC;
    if (n == 0) return MOLANN_OK;
    if (!x || !out) return MOLANN_E_NULL;
    if ((((uintptr_t)x) & 7) || (((uintptr_t)out) & 7)) return MOLANN_E_ALIGNMENT;
    return MOLANN_OK;
}

static int launch_f64(const molann_plan* p, const double* x, int64_t n, double* out, int mode, hipStream_t stream) {
    F64Args a;
    a.n_frames = n; a.n_inp = p->n_inp; a.n_align = p->n_align; a.n_items = p->n_items; a.out_cols = p->d_feat; a.mode = mode;
    const int grid = grid_for(p, n, 4, 8);
    hipLaunchKernelGGL(frames_f64_kernel, dim3(grid), dim3(256), 0, stream, x, out, p->d_align_idx, p->d_ref64, p->d_items, a);
    return (int)hipGetLastError();
}

int molann_align_f64(const molann_plan* p, const double* x, int64_t n, double* out_xyz, molann_stream_t stream) {
    if (!p) return MOLANN_E_NULL;
    if (p->n_align <= 0) return MOLANN_E_STAGE;
    const int c = check_io_f64(x, out_xyz, n);
    if (c != MOLANN_OK || n == 0) return c;
    snprintf(const_cast<molann_plan*>(p)->last_info, sizeof(p->last_info), "frames_f64_kernel (aligned coordinates)");
    return launch_f64(p, x, n, out_xyz, 1, (hipStream_t)stream);
}

int molann_features_f64(const molann_plan* p, const double* x, int64_t n, double* out, molann_stream_t stream) {
    if (!p) return MOLANN_E_NULL;
    if (p->n_items <= 0) return MOLANN_E_STAGE;
    const int c = check_io_f64(x, out, n);
    if (c != MOLANN_OK || n == 0) return c;
    snprintf(const_cast<molann_plan*>(p)->last_info, sizeof(p->last_info), "frames_f64_kernel (features)");
    return launch_f64(p, x, n, out, 0, (hipStream_t)stream);
}

// dL/dx of molann_features_f64 for the same x: grad_f[N, feature_dim] -> grad_x[N, n_inp, 3], everything in double
int molann_features_backward_f64(const molann_plan* p, const double* x, const double* grad_f, int64_t n, double* grad_x, molann_stream_t stream) {
    if (!p) return MOLANN_E_NULL;
    if (p->n_items <= 0) return MOLANN_E_STAGE;
    if (n < 0) return MOLANN_E_DESC;
    if (n == 0) return MOLANN_OK;
    if (!x || !grad_f || !grad_x) return MOLANN_E_NULL;
    if ((((uintptr_t)x) & 7) || (((uintptr_t)grad_f) & 7) || (((uintptr_t)grad_x) & 7)) return MOLANN_E_ALIGNMENT;
    F64Args a;
    a.n_frames = n; a.n_inp = p->n_inp; a.n_align = p->n_align; a.n_items = p->n_items; a.out_cols = p->d_feat; a.mode = 0;
    const int grid = grid_for(p, n, 4, 8);
    hipLaunchKernelGGL(frames_bwd_f64_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, grad_f, grad_x, p->d_align_idx, p->d_ref64, p->d_items, a);
    snprintf(const_cast<molann_plan*>(p)->last_info, sizeof(p->last_info), "frames_bwd_f64_kernel");
    return (int)hipGetLastError();
}

int molann_mlp_f64(const molann_plan* p, const double* f, int64_t n, const double* const* W, const double* const* b, double* out,
                   molann_stream_t stream) {
    if (!p || !W || !b) return MOLANN_E_NULL;
    if (p->n_layers <= 0) return MOLANN_E_STAGE;
    const int c = check_io_f64(f, out, n);
    if (c != MOLANN_OK || n == 0) return c;
    F64Mlp m;
    memset(&m, 0, sizeof(m));
    m.n_layers = p->n_layers; m.act = p->act;
    for (int i = 0; i <= p->n_layers; ++i) { m.dims[i] = p->dims[i]; m.max_w = std::max(m.max_w, p->dims[i]); }
    for (int l = 0; l < p->n_layers; ++l) {
        if (!W[l] || !b[l]) return MOLANN_E_NULL;
        m.W[l] = W[l]; m.b[l] = b[l];
    }
    const size_t lds = (size_t)4 * 2 * m.max_w * sizeof(double);
    if (lds > 65536) return MOLANN_E_UNSUPPORTED;
    const int grid = grid_for(p, n, 4, 8);
    hipLaunchKernelGGL(mlp_f64_kernel, dim3(grid), dim3(256), lds, (hipStream_t)stream, f, out, (long)n, m);
    return (int)hipGetLastError();
}

int molann_forward_f64(const molann_plan* p, const double* x, int64_t n, const double* const* W, const double* const* b,
                       double* features_work, double* out, molann_stream_t stream) {
    if (!p) return MOLANN_E_NULL;
    if (p->n_layers <= 0 || p->n_items <= 0) return MOLANN_E_STAGE;
    if (n > 0 && !features_work) return MOLANN_E_NULL;
    int e = molann_features_f64(p, x, n, features_work, stream);
    if (e != MOLANN_OK || n == 0) return e;
    e = molann_mlp_f64(p, features_work, n, W, b, out, stream);
    snprintf(const_cast<molann_plan*>(p)->last_info, sizeof(p->last_info), "frames_f64_kernel (features) + mlp_f64_kernel");
    return e;
}

int molann_plan_grad_params_size(const molann_plan* p) { return p ? p->n_grad_params : MOLANN_E_NULL; }

int molann_plan_supports_backward(const molann_plan* p) {
    if (!p) return MOLANN_E_NULL;
    if (!p->geom[0].ok) { // large frames: the features (frames_wave_bwd_kernel), and a head within the fused MLP's limits behind them
        if (p->n_items <= 0) return 0;
        if (p->n_layers == 0) return 1;
        const int act = p->act;
        return (p->mlp_spec && p->mbwd_state >= 0 && rtc_api()->ok && (act == 0 || act == 1 || act == 2 || act == 3 || act == 5 || act == 7)) ? 1 : 0;
    }
    if (!p->spec || p->n_items <= 0 || p->bwd_state < 0 || !rtc_api()->ok) return 0;
    if (p->n_layers > 0 && (!p->fused_mlp || p->d_feat > LANE_MLP_MAX_WIDTH || p->mbwd_state < 0)) return 0;
    const int act = p->act;
    if (p->n_layers > 0 && !(act == 0 || act == 1 || act == 2 || act == 3 || act == 5 || act == 7)) return 0;
    return 1;
}

namespace {
// ---- backward: lazily built kernels and workspaces --------------------------------------------------------------------
// The workspaces (parameter partial sums, recomputed features) belong to the plan and are shared by all streams: the
// enqueue is serialised by launch_mu and a caller on another stream first waits for the event recorded behind the
// previous backward (the protocol of the unfused forward).
struct BwdGuard {
    molann_plan* p;
    hipStream_t s;
    std::unique_lock<std::mutex> lock;
    int rc;
    BwdGuard(molann_plan* plan, hipStream_t stream) : p(plan), s(stream), lock(*plan->launch_mu), rc(0) {
        if (p->have_bwork && p->bwork_stream != s) rc = (int)hipStreamWaitEvent(s, p->ev_bwork, 0);
    }
    ~BwdGuard() {
        if (hipEventRecord(p->ev_bwork, s) == hipSuccess) { p->have_bwork = true; p->bwork_stream = s; }
    }
};

int ensure_bwd_event(molann_plan* p) { // jit_mu held
    if (!p->ev_bwork) HIP_TRY(hipEventCreateWithFlags(&p->ev_bwork, hipEventDisableTiming));
    return MOLANN_OK;
}

// the MLP's description for its backward kernel: the lane plan's own, or the one made for a small head behind a wave-per-frame kernel
const JitSpecBox* mlp_box(const molann_plan* p) { return (p->spec && p->spec->j.n_layers > 0) ? p->spec : p->mlp_spec; }

int ensure_mlp_bwd(molann_plan* p) {
    if (!mlp_box(p)) return MOLANN_E_UNSUPPORTED;
    if (p->mbwd_state == 0 || !p->d_gpart) {
        std::lock_guard<std::mutex> lock(*p->jit_mu);
        if (p->mbwd_state == 0) {
            const int rows = mlp_bwd_rows(mlp_box(p)->j.dims, p->act);
            const int wpb = (int)std::min<long>(8, (163840 - 64) / ((long)rows * 68 * 4));
            std::vector<char> code;
            std::string log;
            int rc = -1;
            if (wpb >= 1) rc = jit_compile(jit_source_mlp_bwd(*mlp_box(p), wpb), code, log);
            if (rc == 0 && hipModuleLoadData(&p->mbwd_mod, code.data()) == hipSuccess &&
                hipModuleGetFunction(&p->mbwd_fn, p->mbwd_mod, "molann_mlp_bwd") == hipSuccess) {
                p->mbwd_wpb = wpb;
                p->mbwd_state = 1;
            } else {
                p->mbwd_state = -1;
                if (getenv("MOLANN_JIT_VERBOSE")) fprintf(stderr, "molann mlp backward jit failed rc=%d\n%s\n", rc, log.c_str());
            }
        }
        if (p->mbwd_state == 1 && !p->d_gpart) {
            { const int er = ensure_bwd_event(p); if (er != MOLANN_OK) return er; }
            HIP_TRY(hipMalloc((void**)&p->d_gpart, (size_t)p->num_cus * std::max(1, p->n_grad_params) * 4));
        }
    }
    return p->mbwd_state == 1 ? MOLANN_OK : MOLANN_E_UNSUPPORTED;
}

int ensure_chain_bwd(molann_plan* p) {
    if (p->cbwd_waves <= 0) return MOLANN_E_UNSUPPORTED;
    if (p->cbwd_state == 0 || !p->d_gpart) {
        std::lock_guard<std::mutex> lock(*p->jit_mu);
        if (p->cbwd_state == 0) {
            const int nl = p->n_layers;
            std::vector<int> dims(p->dims, p->dims + nl + 1), kp(p->kp, p->kp + nl), jp(p->jp, p->jp + nl);
            std::vector<long> woff(p->moff, p->moff + nl);
            std::vector<char> code;
            std::string log;
            const int rc = jit_compile(jit_source_chain_bwd(dims, kp, jp, woff, p->act, p->cbwd_waves), code, log);
            if (rc == 0 && hipModuleLoadData(&p->cbwd_mod, code.data()) == hipSuccess &&
                hipModuleGetFunction(&p->cbwd_fn, p->cbwd_mod, "molann_chain_bwd") == hipSuccess) {
                p->cbwd_state = 1;
            } else {
                p->cbwd_state = -1;
                if (getenv("MOLANN_JIT_VERBOSE")) fprintf(stderr, "molann chain backward jit failed rc=%d\n%s\n", rc, log.c_str());
            }
        }
        if (p->cbwd_state == 1 && !p->d_gpart) {
            { const int er = ensure_bwd_event(p); if (er != MOLANN_OK) return er; }
            HIP_TRY(hipMalloc((void**)&p->d_gpart, (size_t)p->num_cus * std::max(1, p->n_grad_params) * 4));
        }
    }
    return p->cbwd_state == 1 ? MOLANN_OK : MOLANN_E_UNSUPPORTED;
}

int ensure_features_bwd(molann_plan* p, molann_plan::LaneGeom& g) {
    lane_geometry(g, 64 * p->n_inp * 12, 1); // the dense frame tile (reused for the gradient rows)
    if (!g.ok) return MOLANN_E_UNSUPPORTED;
    if (p->bwd_state == 0) {
        std::lock_guard<std::mutex> lock(*p->jit_mu);
        if (p->bwd_state == 0) {
            std::vector<char> code;
            std::string log;
            JitSpecBox b = *p->spec;
            b.j.wpb = g.wpb;
            const int rc = jit_compile(jit_source_bwd(b, g.lds_per_wave), code, log);
            if (rc == 0 && hipModuleLoadData(&p->bwd_mod, code.data()) == hipSuccess &&
                hipModuleGetFunction(&p->bwd_fn, p->bwd_mod, "molann_lane_bwd") == hipSuccess) {
                p->bwd_state = 1;
            } else {
                p->bwd_state = -1;
                if (getenv("MOLANN_JIT_VERBOSE")) fprintf(stderr, "molann backward jit failed rc=%d\n%s\n", rc, log.c_str());
            }
        }
    }
    return p->bwd_state == 1 ? MOLANN_OK : MOLANN_E_UNSUPPORTED;
}

// the one-pass backward of the plan (molann_bwd_ring.inc): built at the first backward; a build that does not fit the LDS or
// needs scratch memory (register spills) leaves the two-kernel path in charge
int ensure_ring_bwd(molann_plan* p) {
    if (p->rbwd_state == 0 || (p->rbwd_state == 1 && p->n_grad_params > 0 && !p->d_gpart)) {
        std::lock_guard<std::mutex> lock(*p->jit_mu);
        if (p->rbwd_state == 0) {
            int st = -1;
            JitSpecBox b = *p->spec;
            const char* off = getenv("MOLANN_NO_RING_BWD");
            if (!(off && off[0] == '1') && p->geom[0].ok && bwd_ring_geometry(b.j, p->n_grad_params)) {
                // The kernel lives at the edge of its 256 registers.  Without SLP vectorisation first (C3: 2267 vector instructions and
                // no scratch, against 2564 + 16 spilled registers with it); the default for the plans that spill without it.
                const std::string src = jit_source_bwd_ring(b);
                for (int attempt = 0; attempt < 2 && st != 1; ++attempt) {
                    std::vector<char> code;
                    std::string log;
                    const int rc = jit_compile(src, code, log, attempt == 0 ? "-fno-slp-vectorize" : nullptr);
                    int scratch = -1;
                    hipModule_t mod = nullptr;
                    hipFunction_t fn = nullptr;
                    if (rc == 0 && hipModuleLoadData(&mod, code.data()) == hipSuccess && hipModuleGetFunction(&fn, mod, "molann_bwd_ring") == hipSuccess &&
                        hipFuncGetAttribute(&scratch, HIP_FUNC_ATTRIBUTE_LOCAL_SIZE_BYTES, fn) == hipSuccess && scratch == 0) {
                        p->rbwd_mod = mod; p->rbwd_fn = fn;
                        p->rbwd_ncons = b.j.ncons; p->rbwd_nload = b.j.nload; p->rbwd_nslot = b.j.nslot; p->rbwd_lds = b.j.lds_block;
                        st = 1;
                    } else {
                        if (mod) (void)hipModuleUnload(mod);
                        if (getenv("MOLANN_JIT_VERBOSE")) fprintf(stderr, "molann one-pass backward, build %d not used (rc=%d, scratch=%d)\n%s\n", attempt, rc, scratch, log.c_str());
                    }
                }
            }
            p->rbwd_state = st;
        }
        if (p->rbwd_state == 1 && p->n_grad_params > 0 && !p->d_gpart) {
            { const int er = ensure_bwd_event(p); if (er != MOLANN_OK) return er; }
            HIP_TRY(hipMalloc((void**)&p->d_gpart, (size_t)p->num_cus * p->n_grad_params * 4));
        }
    }
    return p->rbwd_state == 1 ? MOLANN_OK : MOLANN_E_UNSUPPORTED;
}

// molann_bwd_ring (+ reduce_rows_kernel); with parameter gradients the caller holds the workspace (BwdGuard)
int launch_ring_bwd(molann_plan* p, const float* x, const float* grad_out, long n, float* grad_x, float* grad_params, hipStream_t stream,
                    float* values = nullptr) {
    const long n_tiles = (n + 63) / 64;
    const int grid = (int)std::max<long>(1, std::min<long>(p->num_cus, n_tiles));
    const bool params = grad_params && p->n_grad_params > 0;
    struct { const float* x; const float* gout; const double* ref64; const float* ref32; const float* wnat; float* gx; float* gp; long n; float* y; } ka =
        {x, grad_out, p->d_ref64, p->d_ref, (const float*)p->d_wmfma, grad_x, params ? p->d_gpart : nullptr, n, values};
    size_t ksz = sizeof(ka);
    void* cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &ka, HIP_LAUNCH_PARAM_BUFFER_SIZE, &ksz, HIP_LAUNCH_PARAM_END};
    const int block = 64 * (p->rbwd_ncons + p->rbwd_nload);
    const hipError_t le = hipModuleLaunchKernel(values ? p->vjp_fn : p->rbwd_fn, grid, 1, 1, block, 1, 1, 0, stream, nullptr, cfg);
    if (le != hipSuccess) return (int)le;
    if (params) {
        hipLaunchKernelGGL(reduce_rows_kernel, dim3((p->n_grad_params + 63) / 64), dim3(1024), 0, stream, p->d_gpart, grid, p->n_grad_params,
                           grad_params);
        HIP_TRY(hipGetLastError());
    }
    snprintf(p->last_info, sizeof(p->last_info), "molann_bwd_ring%s (plan-specialised; %d consumer waves + %d loader, ring of %d tiles) grid=%d block=%d lds=%d%s",
             values ? "<values>" : "", p->rbwd_ncons, p->rbwd_nload, p->rbwd_nslot, grid, block, p->rbwd_lds, params ? " + reduce_rows_kernel" : "");
    return MOLANN_OK;
}

// molann_lane_bwd: grad_f -> grad_x (no workspace)
int launch_features_bwd(molann_plan* p, const molann_plan::LaneGeom& g, const float* x, const float* grad_f, long n, float* grad_x,
                        hipStream_t stream) {
    const long n_tiles = (n + 63) / 64;
    int bpc = (int)(163840 / ((long)g.wpb * g.lds_per_wave));
    if (bpc < 1) bpc = 1;
    if (bpc * g.wpb > 8) bpc = std::max(1, 8 / g.wpb);
    const int grid = grid_for(p, n_tiles, g.wpb, bpc);
    struct { const float* x; const float* gf; const double* ref64; float* gx; long n; int x_wide; } ka =
        {x, grad_f, p->d_ref64, grad_x, n, (((uintptr_t)x) & 15) == 0 ? 1 : 0};
    size_t ksz = sizeof(ka);
    void* cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &ka, HIP_LAUNCH_PARAM_BUFFER_SIZE, &ksz, HIP_LAUNCH_PARAM_END};
    const hipError_t le = hipModuleLaunchKernel(p->bwd_fn, grid, 1, 1, 64 * g.wpb, 1, 1, (unsigned)((size_t)g.wpb * g.lds_per_wave), stream,
                                                nullptr, cfg);
    snprintf(p->last_info, sizeof(p->last_info), "molann_lane_bwd (plan-specialised) grid=%d block=%d", grid, 64 * g.wpb);
    return (int)le;
}

// molann_chain_bwd (+ reduce_rows_kernel when parameter gradients are wanted); the caller holds the workspace (BwdGuard).
// One block per CU at most (its weight copy fills the LDS), tiles of 16 WAVES frames handed out statically: the grid, and with it
// every block's partial sums, depend on n alone.
int launch_chain_bwd(molann_plan* p, const float* f, const float* grad_out, long n, float* grad_f, float* grad_params, hipStream_t stream) {
    const long n_tiles = (n + 16 * p->cbwd_waves - 1) / (16 * p->cbwd_waves);
    const int grid = (int)std::max<long>(1, std::min<long>(p->num_cus, n_tiles));
    struct { const float* f; const float* gout; const float* wnat; float* gf; float* gp; long n; } ka =
        {f, grad_out, (const float*)p->d_wmfma, grad_f, grad_params ? p->d_gpart : nullptr, n};
    size_t ksz = sizeof(ka);
    void* cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &ka, HIP_LAUNCH_PARAM_BUFFER_SIZE, &ksz, HIP_LAUNCH_PARAM_END};
    const hipError_t le = hipModuleLaunchKernel(p->cbwd_fn, grid, 1, 1, 64 * p->cbwd_waves, 1, 1, 0, stream, nullptr, cfg);
    if (le != hipSuccess) return (int)le;
    if (grad_params) {
        hipLaunchKernelGGL(reduce_rows_kernel, dim3((p->n_grad_params + 63) / 64), dim3(1024), 0, stream, p->d_gpart, grid, p->n_grad_params,
                           grad_params);
        HIP_TRY(hipGetLastError());
    }
    snprintf(p->last_info, sizeof(p->last_info), "molann_chain_bwd (plan-specialised) grid=%d block=%d%s", grid, 64 * p->cbwd_waves,
             grad_params ? " + reduce_rows_kernel" : "");
    return MOLANN_OK;
}

// molann_mlp_bwd (+ reduce_rows_kernel when parameter gradients are wanted); the caller holds the workspace (BwdGuard)
int launch_mlp_bwd(molann_plan* p, const float* f, const float* grad_out, long n, float* grad_f, float* grad_params, hipStream_t stream) {
    const long n_tiles = (n + 63) / 64;
    const int grid = (int)std::max<long>(1, std::min<long>(p->num_cus, (n_tiles + p->mbwd_wpb - 1) / p->mbwd_wpb)); // one block per CU
    struct { const float* f; const float* gout; const float* wnat; float* gf; float* gp; long n; } ka =
        {f, grad_out, (const float*)p->d_wmfma, grad_f, grad_params ? p->d_gpart : nullptr, n};
    size_t ksz = sizeof(ka);
    void* cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &ka, HIP_LAUNCH_PARAM_BUFFER_SIZE, &ksz, HIP_LAUNCH_PARAM_END};
    const hipError_t le = hipModuleLaunchKernel(p->mbwd_fn, grid, 1, 1, 64 * p->mbwd_wpb, 1, 1, 0, stream, nullptr, cfg);
    if (le != hipSuccess) return (int)le;
    if (grad_params) {
        hipLaunchKernelGGL(reduce_rows_kernel, dim3((p->n_grad_params + 63) / 64), dim3(1024), 0, stream, p->d_gpart, grid, p->n_grad_params,
                           grad_params);
        HIP_TRY(hipGetLastError());
    }
    snprintf(p->last_info, sizeof(p->last_info), "molann_mlp_bwd (plan-specialised) grid=%d block=%d%s", grid, 64 * p->mbwd_wpb,
             grad_params ? " + reduce_rows_kernel" : "");
    return MOLANN_OK;
}
} // namespace

// the backward's workspace (recomputed features and their gradients, two halves), allocated at the first backward that needs it
static int ensure_bwork(molann_plan* p) {
    if (!p->d_bwork) {
        std::lock_guard<std::mutex> lock(*p->jit_mu);
        if (!p->d_bwork) {
            long bf = std::min<long>(1l << 20, (64l << 20) / ((long)p->d_feat * 4)) & ~63l;
            bf = std::max<long>(bf, 4096);
            float* w = nullptr;
            HIP_TRY(hipMalloc((void**)&w, 2 * (size_t)bf * p->d_feat * 4));
            p->bwork_frames = bf;
            p->d_bwork = w;
        }
    }
    return MOLANN_OK;
}

// dL/dx of the features of LARGE frames (one wave per frame): grad_f[N, d_feat] -> grad_x[N, n_inp, 3]
static int launch_wave_bwd(molann_plan* p, const float* x, const float* grad_f, int64_t n, float* grad_x, hipStream_t stream) {
    if (!grad_x) return MOLANN_OK;
    if ((((uintptr_t)x) & 3) || (((uintptr_t)grad_f) & 3) || (((uintptr_t)grad_x) & 3)) return MOLANN_E_ALIGNMENT;
    PreArgs a;
    fill_pre_args(p, a, n, 0, p->d_feat, false, x, grad_x);
    // the aligned frame itself (one position item per atom): the dense gradient, cotangent and frame in registers
    if (p->dense_positions && p->n_inp <= 24 * 512) {
        AlignRegsArgs ra;
        memset(&ra, 0, sizeof(ra));
        ra.n_frames = n; ra.n_inp = p->n_inp; ra.n_align = p->n_align; ra.first_align = p->align_first;
        // the cotangent in registers (x passes through): as the forward, the fewest data waves with <= 24 atoms per thread
        int W = 1;
        while ((p->n_inp + 64 * W - 1) / (64 * W) > 24) W *= 2;
        const int units = ((p->n_inp + 64 * W - 1) / (64 * W) + 3) / 4;
        const void* fn = nullptr;
#define ALIGN_BWD_CASE(WW, UU) if (W == WW && units == UU) fn = (const void*)frames_align_bwd_regs_kernel<WW, UU>;
        ALIGN_BWD_CASE(1, 1) ALIGN_BWD_CASE(1, 2) ALIGN_BWD_CASE(1, 3) ALIGN_BWD_CASE(1, 4) ALIGN_BWD_CASE(1, 5) ALIGN_BWD_CASE(1, 6)
        ALIGN_BWD_CASE(2, 4) ALIGN_BWD_CASE(2, 5) ALIGN_BWD_CASE(2, 6) ALIGN_BWD_CASE(4, 4) ALIGN_BWD_CASE(4, 5) ALIGN_BWD_CASE(4, 6)
        ALIGN_BWD_CASE(8, 4) ALIGN_BWD_CASE(8, 5) ALIGN_BWD_CASE(8, 6)
#undef ALIGN_BWD_CASE
        if (fn) {
            int occ = 0;
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, 64 * (W + 2), 0) != hipSuccess || occ < 1) occ = 1;
            occ = std::min(occ, std::max(2, (int)(245760 / (24l * p->n_inp))));      // ~240 KB of frame + cotangent in flight per CU
            if (debug_env().wave_bpc > 0) occ = std::min(occ, debug_env().wave_bpc);
            const int grid = (int)std::min<long>(n, (long)p->num_cus * occ);
            void* kargs[] = {(void*)&x, (void*)&grad_f, (void*)&grad_x, (void*)&p->d_align_idx, (void*)&p->d_align_slot, (void*)&p->d_ref, (void*)&p->d_ref64, (void*)&ra};
            const hipError_t le = hipLaunchKernel(fn, dim3(grid), dim3(64 * (W + 2)), kargs, 0, stream);
            snprintf(p->last_info, sizeof(p->last_info), "frames_align_bwd_regs_kernel<W=%d,U=%d> (%d data waves + a forward and a backward solver wave, %d blocks per CU) grid=%d block=%d",
                     W, units, W, occ, grid, 64 * (W + 2));
            return le != hipSuccess ? (int)le : (int)hipGetLastError();
        }
    }
    const int per_wave = ((p->n_items * 48 + 15) / 16) * 16;   // g_y of every item's four atoms
    // mid-size frames with an alignment: B frames per wave and round (frames_group_bwd_kernel), the tables in LDS
    if (p->bw_touched > 0 && p->n_align > 0 && getenv("MOLANN_BWD_ATOMICS") == nullptr && getenv("MOLANN_NO_BWD_GROUP") == nullptr &&
        (p->n_inp <= 1024 || getenv("MOLANN_BWD_GROUP_ALL") != nullptr)) {
        const int wpb = 4;
        int nb = 8;
        while (nb > 1 && (long)nb * p->n_items > 256) nb /= 2;
        GroupBwdArgs gb;
        memset(&gb, 0, sizeof(gb));
        gb.n_touched = p->bw_touched; gb.n_list = p->bw_list_len; gb.gy_frame = 12 * p->n_items;
        size_t off = (size_t)ceil_to(8 * (3 * p->n_align + 8), 16);
        gb.off_ref32 = (int)off; off += (size_t)ceil_to(4 * (3 * p->n_align + 8), 16);
        gb.off_align = (int)off; off += (size_t)ceil_to(4 * p->n_align, 16);
        gb.off_items = (int)off; off += (size_t)32 * p->n_items;
        gb.off_bw_atoms = (int)off; off += (size_t)ceil_to(4 * p->bw_touched, 16);
        gb.off_bw_ptr = (int)off; off += (size_t)ceil_to(4 * (p->bw_touched + 1), 16);
        gb.off_bw_list = (int)off; off += (size_t)ceil_to(4 * p->bw_list_len, 16);
        gb.off_bw_align = (int)off; off += (size_t)ceil_to(4 * p->bw_touched, 16);
        gb.off_gy = (int)off; off += (size_t)wpb * nb * gb.gy_frame * 4;
        if (nb > 1 && off <= 65536) {
            const long n_rounds = (n + nb - 1) / nb;
            const int bpc = (int)std::max<size_t>(1, std::min<size_t>(8, 160 * 1024 / off));
            const int grid = grid_for(p, n_rounds, wpb, bpc);
#define LAUNCH_GROUP_BWD(BB) hipLaunchKernelGGL((frames_group_bwd_kernel<BB>), dim3(grid), dim3(64 * wpb), off, stream, x, grad_f, grad_x, p->d_align_idx, p->d_ref, \
                                            p->d_ref64, p->d_items, p->d_bw_atoms, p->d_bw_ptr, p->d_bw_list, p->d_bw_align, a, gb)
            if (nb == 8) LAUNCH_GROUP_BWD(8);
            else if (nb == 4) LAUNCH_GROUP_BWD(4);
            else LAUNCH_GROUP_BWD(2);
#undef LAUNCH_GROUP_BWD
            snprintf(p->last_info, sizeof(p->last_info), "frames_group_bwd_kernel<B=%d> (frames_wave_bwd on %d frames per wave and round) grid=%d block=%d lds=%zu",
                     nb, nb, grid, 64 * wpb, off);
            return (int)hipGetLastError();
        }
    }
    if (p->bw_touched > 0 && per_wave <= 65536 && getenv("MOLANN_BWD_ATOMICS") == nullptr) {
        const int wpb = std::max(1, std::min(4, 65536 / per_wave));
        const int bpc = std::max(1, std::min(8, 160 * 1024 / (wpb * per_wave)));
        const int grid = grid_for(p, n, wpb, bpc);
        BwGatherArgs b = {p->bw_touched, per_wave};
        hipLaunchKernelGGL(frames_wave_bwd_gather_kernel, dim3(grid), dim3(64 * wpb), (size_t)wpb * per_wave, stream, x, grad_f,
                           grad_x, p->d_align_idx, p->d_ref, p->d_ref64, p->d_items, p->d_bw_atoms, p->d_bw_ptr, p->d_bw_list, p->d_bw_align,
                           a, b);
        snprintf(p->last_info, sizeof(p->last_info), "frames_wave_bwd_gather_kernel grid=%d block=%d lds=%d", grid, 64 * wpb, wpb * per_wave);
        return (int)hipGetLastError();
    }
    const int wpb = 4;
    const int grid = grid_for(p, n, wpb, 8);
    hipLaunchKernelGGL(frames_wave_bwd_kernel, dim3(grid), dim3(64 * wpb), 0, stream, x, grad_f, grad_x,
                       p->d_align_idx, p->d_ref, p->d_ref64, p->d_items, a);
    snprintf(p->last_info, sizeof(p->last_info), "frames_wave_bwd_kernel grid=%d block=%d", grid, 64 * wpb);
    return (int)hipGetLastError();
}

// dL/dx and dL/d(parameters) of molann_forward_packed_f32 / molann_features_f32 for the same x.
int molann_backward_f32(molann_plan* p, const float* x, const float* grad_out, int64_t n, float* grad_x, float* grad_params,
                        molann_stream_t stream) {
    if (!p) return MOLANN_E_NULL;
    if (n < 0) return MOLANN_E_DESC;
    if (n == 0) return MOLANN_OK;
    if (!x || !grad_out) return MOLANN_E_NULL;
    if (!p->geom[0].ok && p->n_items > 0 && p->n_layers == 0) // large frames: one wave per frame, no parameters
        return launch_wave_bwd(p, x, grad_out, n, grad_x, (hipStream_t)stream);
    if (!p->geom[0].ok && p->n_items > 0) { // large frames, a small head: features (recomputed) -> MLP backward -> wave-per-frame backward
        if (!molann_plan_supports_backward(p)) return MOLANN_E_UNSUPPORTED;
        if (!p->mlp_packed) return MOLANN_E_NOT_PACKED;
        if ((((uintptr_t)x) & 3) || (((uintptr_t)grad_out) & 3) || (((uintptr_t)grad_x) & 3) || (((uintptr_t)grad_params) & 3)) return MOLANN_E_ALIGNMENT;
        if (!grad_x && !grad_params) return MOLANN_OK;
        int rc = ensure_mlp_bwd(p);
        if (rc != MOLANN_OK) return rc;
        if ((rc = ensure_bwork(p)) != MOLANN_OK) return rc;
        hipStream_t main = (hipStream_t)stream;
        BwdGuard guard(p, main);
        if (guard.rc != 0) return guard.rc;
        float* wf = p->d_bwork;
        float* wg = p->d_bwork + (size_t)p->bwork_frames * p->d_feat;
        char info[3][96];
        info[0][0] = info[1][0] = info[2][0] = 0;
        for (int64_t s = 0; s < n && rc == MOLANN_OK; s += p->bwork_frames) {
            const long m = (long)std::min<int64_t>(p->bwork_frames, n - s);
            const float* xs = x + s * (long)p->n_inp * 3;
            if ((rc = launch_pre(p, xs, m, wf, 0, false, main)) != 0) break;
            if (s == 0) snprintf(info[0], sizeof(info[0]), "%.95s", p->last_info);
            if ((rc = launch_mlp_bwd(p, wf, grad_out + s * (long)p->out_dim, m, grad_x ? wg : nullptr, grad_params, main)) != 0) break;
            if (s == 0) snprintf(info[1], sizeof(info[1]), "%.95s", p->last_info);
            if (grad_x && (rc = launch_wave_bwd(p, xs, wg, m, grad_x + s * (long)p->n_inp * 3, main)) != 0) break;
            if (s == 0 && grad_x) snprintf(info[2], sizeof(info[2]), "%.95s", p->last_info);
        }
        if (rc == MOLANN_OK)
            snprintf(p->last_info, sizeof(p->last_info), "%.72s || %.72s || %.72s || chunks of %ld frames", info[0], info[1], info[2], p->bwork_frames);
        return rc;
    }
    if (!p->spec || p->n_items <= 0) return MOLANN_E_UNSUPPORTED;
    if (p->n_layers == 0 || molann_plan_supports_backward(p)) { // one pass over x when the plan's kernel could be built
        if (p->n_layers > 0 && !p->mlp_packed) return MOLANN_E_NOT_PACKED;
        if ((((uintptr_t)x) & 3) || (((uintptr_t)grad_out) & 3) || (((uintptr_t)grad_x) & 3) || (((uintptr_t)grad_params) & 3)) return MOLANN_E_ALIGNMENT;
        if (!grad_x && !(grad_params && p->n_layers > 0)) return MOLANN_OK;
        const int er = ensure_ring_bwd(p);
        if (er == MOLANN_OK) {
            if (!(grad_params && p->n_grad_params > 0)) return launch_ring_bwd(p, x, grad_out, (long)n, grad_x, nullptr, (hipStream_t)stream);
            BwdGuard guard(p, (hipStream_t)stream);
            if (guard.rc != 0) return guard.rc;
            return launch_ring_bwd(p, x, grad_out, (long)n, grad_x, grad_params, (hipStream_t)stream);
        }
        if (er != MOLANN_E_UNSUPPORTED) return er;
    }
    if (p->n_layers == 0) return molann_features_backward_f32(p, x, grad_out, n, grad_x, stream);
    // plans with an MLP, nothing saved from the forward: features (recomputed) -> MLP backward -> preprocessing backward,
    // in chunks through the plan's backward workspace (allocated at the first call, like the kernels are compiled then)
    if (!molann_plan_supports_backward(p)) return MOLANN_E_UNSUPPORTED;
    if (!p->mlp_packed) return MOLANN_E_NOT_PACKED;
    if ((((uintptr_t)x) & 3) || (((uintptr_t)grad_out) & 3) || (((uintptr_t)grad_x) & 3) || (((uintptr_t)grad_params) & 3)) return MOLANN_E_ALIGNMENT;
    if (!grad_x && !grad_params) return MOLANN_OK;
    molann_plan::LaneGeom g;
    int rc = ensure_mlp_bwd(p);
    if (rc == MOLANN_OK && grad_x) rc = ensure_features_bwd(p, g);
    if (rc != MOLANN_OK) return rc;
    if ((rc = ensure_bwork(p)) != MOLANN_OK) return rc;
    hipStream_t main = (hipStream_t)stream;
    BwdGuard guard(p, main);
    if (guard.rc != 0) return guard.rc;
    float* wf = p->d_bwork;
    float* wg = p->d_bwork + (size_t)p->bwork_frames * p->d_feat;
    char info[3][96];
    info[0][0] = info[1][0] = info[2][0] = 0;
    for (int64_t s = 0; s < n && rc == MOLANN_OK; s += p->bwork_frames) {
        const long m = (long)std::min<int64_t>(p->bwork_frames, n - s);
        const float* xs = x + s * (long)p->n_inp * 3;
        if ((rc = launch_pre(p, xs, m, wf, 0, false, main)) != 0) break;
        if (s == 0) snprintf(info[0], sizeof(info[0]), "%.95s", p->last_info);
        if ((rc = launch_mlp_bwd(p, wf, grad_out + s * (long)p->out_dim, m, grad_x ? wg : nullptr, grad_params, main)) != 0) break;
        if (s == 0) snprintf(info[1], sizeof(info[1]), "%.95s", p->last_info);
        if (grad_x && (rc = launch_features_bwd(p, g, xs, wg, m, grad_x + s * (long)p->n_inp * 3, main)) != 0) break;
        if (s == 0 && grad_x) snprintf(info[2], sizeof(info[2]), "%.95s", p->last_info);
    }
    if (rc == MOLANN_OK)
        snprintf(p->last_info, sizeof(p->last_info), "%.72s || %.72s || %.72s || chunks of %ld frames", info[0], info[1], info[2], p->bwork_frames);
    return rc;
}

namespace {
// the one-pass backward's build that also stores the forward's outputs (molann_bwd_ring.inc, WITH_VALUES), built at the first use
int ensure_ring_vjp(molann_plan* p) {
    const int er = ensure_ring_bwd(p);       // the geometry is the one-pass backward's
    if (er != MOLANN_OK) return er;
    if (p->vjp_state == 0) {
        std::lock_guard<std::mutex> lock(*p->jit_mu);
        if (p->vjp_state == 0) {
            int st = -1;
            JitSpecBox b = *p->spec;
            if (bwd_ring_geometry(b.j, p->n_grad_params)) {
                b.j.with_values = true;
                const std::string src = jit_source_bwd_ring(b);
                for (int attempt = 0; attempt < 2 && st != 1; ++attempt) {   // (scratch is tolerated here: a latency path, not a throughput path)
                    std::vector<char> code;
                    std::string log;
                    hipModule_t mod = nullptr;
                    hipFunction_t fn = nullptr;
                    if (jit_compile(src, code, log, attempt == 0 ? "-fno-slp-vectorize" : nullptr) == 0 && hipModuleLoadData(&mod, code.data()) == hipSuccess &&
                        hipModuleGetFunction(&fn, mod, "molann_bwd_ring") == hipSuccess) {
                        p->vjp_mod = mod; p->vjp_fn = fn;
                        st = 1;
                    } else {
                        if (mod) (void)hipModuleUnload(mod);
                        if (getenv("MOLANN_JIT_VERBOSE")) fprintf(stderr, "molann value + vjp build %d failed\n%s\n", attempt, log.c_str());
                    }
                }
            }
            p->vjp_state = st;
        }
    }
    return p->vjp_state == 1 ? MOLANN_OK : MOLANN_E_UNSUPPORTED;
}

// Frames the lane kernels do not take (mid-size and large): molann_group_vjp.inc, for heads within the fused MLP's limits (every
// width and the feature dimension <= 32, <= 4 layers, fp32; tanh, ReLU, sigmoid, identity, SiLU, LeakyReLU - the fp32 MFMA
// copy of the weights is packed for every plan) and for features-only plans.  Built at the first use; E_UNSUPPORTED where the
// tables do not fit the LDS at B >= 2 or hipRTC is missing.
bool group_vjp_serves(const molann_plan* p) {
    if (p->geom[0].ok || p->n_items <= 0 || p->va_touched <= 0 || !rtc_api()->ok) return false;
    if (p->n_layers == 0) return true;
    const int act = p->act;
    if (p->mlp_prec != MOLANN_MLP_F32 || p->n_layers > LANE_MLP_MAX_LAYERS || p->d_feat > LANE_MLP_MAX_WIDTH) return false;
    for (int l = 1; l <= p->n_layers; ++l)
        if (p->dims[l] > LANE_MLP_MAX_WIDTH) return false;
    return act == 0 || act == 1 || act == 2 || act == 3 || act == 5 || act == 7;
}

int ensure_group_vjp(molann_plan* p) {
    if (!group_vjp_serves(p)) return MOLANN_E_UNSUPPORTED;
    if (p->gvjp_state == 0) {
        std::lock_guard<std::mutex> lock(*p->jit_mu);
        if (p->gvjp_state == 0) {
            int st = -1;
            const int nl = p->n_layers;
            std::vector<int> dims, kp, jp;
            std::vector<long> woff;
            if (nl > 0) {
                dims.assign(p->dims, p->dims + nl + 1); kp.assign(p->kp, p->kp + nl); jp.assign(p->jp, p->jp + nl); woff.assign(p->moff, p->moff + nl);
            }
            GroupVjpGeom g;
            if (group_vjp_geometry(dims, p->act, p->d_feat, p->n_align, p->n_items, p->va_touched, p->va_list_len, g)) {
                std::vector<char> code;
                std::string log;
                hipModule_t mod = nullptr;
                hipFunction_t fn = nullptr;
                const int rc = jit_compile(jit_source_group_vjp(dims, kp, jp, woff, p->act, p->d_feat, p->n_inp, p->n_align, p->n_items, p->va_touched,
                                                                p->va_list_len, g), code, log);
                if (rc == 0 && hipModuleLoadData(&mod, code.data()) == hipSuccess && hipModuleGetFunction(&fn, mod, "molann_group_vjp") == hipSuccess) {
                    // blocks per CU at the launch's block size: all WPB waves (batches of at most one tile per CU), or half of them
                    const int waves = g.wpb > 1 ? g.wpb / 2 : 1;
                    int occ = 0;
                    if (hipModuleOccupancyMaxActiveBlocksPerMultiprocessor(&occ, fn, 64 * waves, 0) != hipSuccess || occ < 1)
                        occ = std::max(1, std::min(163840 / g.lds, 32 / waves));
                    p->gvjp_mod = mod; p->gvjp_fn = fn;
                    p->gvjp_b = g.b; p->gvjp_wpb = g.wpb; p->gvjp_lds = g.lds; p->gvjp_bpc = occ;
                    st = 1;
                } else {
                    if (mod) (void)hipModuleUnload(mod);
                    if (getenv("MOLANN_JIT_VERBOSE")) fprintf(stderr, "molann group value + vjp build failed rc=%d\n%s\n", rc, log.c_str());
                }
            }
            p->gvjp_state = st;
        }
    }
    return p->gvjp_state == 1 ? MOLANN_OK : MOLANN_E_UNSUPPORTED;
}

// one block per 64-frame tile (tiles strided over the blocks): WPB waves per block while the batch has at most one tile per CU
// (latency: a round per wave), else half of them and as many blocks as the CUs hold.  No workspace, nothing but the enqueue.
int launch_group_vjp(molann_plan* p, const float* x, const float* grad_out, long n, float* out, float* grad_x, hipStream_t stream) {
    const long n_tiles = (n + 63) / 64;
    const bool wide = n_tiles <= p->num_cus || p->gvjp_wpb == 1;
    const int waves = wide ? p->gvjp_wpb : p->gvjp_wpb / 2;
    const int grid = (int)std::max<long>(1, std::min<long>((long)p->num_cus * (wide ? 1 : p->gvjp_bpc), n_tiles));
    struct { const float* x; const float* gout; const double* ref64; const float* ref32; const int* align; const int* items; const int* atoms;
             const int* ptr; const int* list; const float* wnat; float* out; float* gx; long n; } ka =
        {x, grad_out, p->d_ref64, p->d_ref, p->d_align_idx, (const int*)p->d_items, p->d_va_atoms, p->d_va_ptr, p->d_va_list,
         (const float*)p->d_wmfma, out, grad_x, n};
    size_t ksz = sizeof(ka);
    void* cfg[] = {HIP_LAUNCH_PARAM_BUFFER_POINTER, &ka, HIP_LAUNCH_PARAM_BUFFER_SIZE, &ksz, HIP_LAUNCH_PARAM_END};
    const hipError_t le = hipModuleLaunchKernel(p->gvjp_fn, grid, 1, 1, 64 * waves, 1, 1, 0, stream, nullptr, cfg);
    if (le != hipSuccess) return (int)le;
    snprintf(p->last_info, sizeof(p->last_info), "molann_group_vjp<B=%d> (values + vjp in one launch; %d waves per 64-frame tile) grid=%d block=%d lds=%d",
             p->gvjp_b, waves, grid, 64 * waves, p->gvjp_lds);
    return MOLANN_OK;
}
} // namespace

// The forward's outputs AND the vector-Jacobian product of a batch in ONE launch: the one-pass backward recomputes the forward per
// frame anyway, so a build of it that also stores the outputs (WITH_VALUES: one more product on the matrix cores, from the
// activations already in its scratch) returns both.  For callers that differentiate a small batch at every step with a cotangent
// they know up front - or want the Jacobian: a batch of d_out copies of a frame with the identity as cotangent (README.rst:49's
// use, a collective variable inside an MD engine).  Parameters are data here (no parameter gradients).  Plans the one-pass
// backward serves (molann_plan_backward_kind == 2), and frames the lane kernels do not take (molann_group_vjp.inc: the three
// launches of their backward as one); E_UNSUPPORTED otherwise.  The first call builds the kernel: outside a capture.
int molann_value_and_vjp_f32(molann_plan* p, const float* x, const float* grad_out, int64_t n, float* out, float* grad_x, molann_stream_t stream) {
    if (!p) return MOLANN_E_NULL;
    if (n < 0) return MOLANN_E_DESC;
    if (n == 0) return MOLANN_OK;
    if (!x || !grad_out || !out || !grad_x) return MOLANN_E_NULL;
    if ((((uintptr_t)x) & 3) || (((uintptr_t)grad_out) & 3) || (((uintptr_t)grad_x) & 3) || (((uintptr_t)out) & 3)) return MOLANN_E_ALIGNMENT;
    if (!p->geom[0].ok) {
        const int er = ensure_group_vjp(p);
        if (er != MOLANN_OK) return er;
        if (p->n_layers > 0 && !p->mlp_packed) return MOLANN_E_NOT_PACKED;
        return launch_group_vjp(p, x, grad_out, (long)n, out, grad_x, (hipStream_t)stream);
    }
    if (!p->spec || p->n_items <= 0) return MOLANN_E_UNSUPPORTED;
    if (p->n_layers > 0 && (!molann_plan_supports_backward(p) || !p->fused_mlp)) return MOLANN_E_UNSUPPORTED;
    if (p->n_layers > 0 && !p->mlp_packed) return MOLANN_E_NOT_PACKED;
    const int er = ensure_ring_vjp(p);
    if (er != MOLANN_OK) return er;
    return launch_ring_bwd(p, x, grad_out, (long)n, grad_x, nullptr, (hipStream_t)stream, out);
}

// 1 when molann_value_and_vjp_f32 serves the plan, 0 otherwise.  Builds the kernel it reports.
int molann_plan_supports_value_and_vjp(molann_plan* p) {
    if (!p) return MOLANN_E_NULL;
    if (!p->geom[0].ok) return ensure_group_vjp(p) == MOLANN_OK ? 1 : 0;
    if (!p->spec || p->n_items <= 0) return 0;
    if (p->n_layers > 0 && (!molann_plan_supports_backward(p) || !p->fused_mlp)) return 0;
    return ensure_ring_vjp(p) == MOLANN_OK ? 1 : 0;
}

// how molann_backward_f32 will serve this plan: 2 one pass over x (nothing worth saving from the forward), 1 two kernels
// (a caller that keeps the features of its forward saves their recompute), 0 not at all.  Builds the kernel it reports.
int molann_plan_backward_kind(molann_plan* p) {
    if (!p) return MOLANN_E_NULL;
    if (!molann_plan_supports_backward(p)) return 0;
    if (!p->geom[0].ok || !p->spec) return 1;
    return ensure_ring_bwd(p) == MOLANN_OK ? 2 : 1;
}

// dL/dx of molann_features_f32 for the same x: grad_f[N, feature_dim] -> grad_x[N, n_inp, 3]
int molann_features_backward_f32(molann_plan* p, const float* x, const float* grad_f, int64_t n, float* grad_x, molann_stream_t stream) {
    if (!p) return MOLANN_E_NULL;
    if (n < 0) return MOLANN_E_DESC;
    if (n == 0) return MOLANN_OK;
    if (!x || !grad_f) return MOLANN_E_NULL;
    if (!p->geom[0].ok) { // large frames: the wave-per-frame kernel
        if (p->n_items <= 0) return MOLANN_E_UNSUPPORTED;
        return launch_wave_bwd(p, x, grad_f, n, grad_x, (hipStream_t)stream);
    }
    if (!p->spec || p->n_items <= 0) return MOLANN_E_UNSUPPORTED;
    if (!grad_x) return MOLANN_OK;
    if ((((uintptr_t)x) & 3) || (((uintptr_t)grad_f) & 3) || (((uintptr_t)grad_x) & 3)) return MOLANN_E_ALIGNMENT;
    molann_plan::LaneGeom g;
    const int rc = ensure_features_bwd(p, g);
    if (rc != MOLANN_OK) return rc;
    return launch_features_bwd(p, g, x, grad_f, (long)n, grad_x, (hipStream_t)stream);
}

// 1 when molann_mlp_backward_f32 serves the plan's head: the fused family's kernel (molann_mlp_bwd.inc) or, for a wide fp32 head
// whose chain stream is resident, molann_chain_bwd.inc.  Builds the kernel it reports.
int molann_plan_supports_mlp_backward(molann_plan* p) {
    if (!p) return MOLANN_E_NULL;
    if (p->n_layers <= 0) return 0;
    if (mlp_box(p) && molann_plan_supports_backward(p)) return 1;
    return ensure_chain_bwd(p) == MOLANN_OK ? 1 : 0;
}

// dL/df and dL/d(parameters) of molann_mlp_packed_f32 for the same f (the fused family: every width <= 32; a wide fp32 head
// with a resident chain stream)
int molann_mlp_backward_f32(molann_plan* p, const float* f, const float* grad_out, int64_t n, float* grad_f, float* grad_params,
                            molann_stream_t stream) {
    if (!p) return MOLANN_E_NULL;
    if (n < 0) return MOLANN_E_DESC;
    if (n == 0) return MOLANN_OK;
    if (!f || !grad_out) return MOLANN_E_NULL;
    if (p->n_layers <= 0) return MOLANN_E_STAGE;
    const bool chain = !(mlp_box(p) && molann_plan_supports_backward(p));
    if (chain && p->cbwd_waves <= 0) return MOLANN_E_UNSUPPORTED;
    if (!p->mlp_packed) return MOLANN_E_NOT_PACKED;
    if ((((uintptr_t)f) & 3) || (((uintptr_t)grad_out) & 3) || (((uintptr_t)grad_f) & 3) || (((uintptr_t)grad_params) & 3)) return MOLANN_E_ALIGNMENT;
    if (!grad_f && !grad_params) return MOLANN_OK;
    if (chain) {
        const int rc = ensure_chain_bwd(p);
        if (rc != MOLANN_OK) return rc;
        if (!grad_params) return launch_chain_bwd(p, f, grad_out, (long)n, grad_f, nullptr, (hipStream_t)stream);
        BwdGuard guard(p, (hipStream_t)stream);
        if (guard.rc != 0) return guard.rc;
        return launch_chain_bwd(p, f, grad_out, (long)n, grad_f, grad_params, (hipStream_t)stream);
    }
    const int rc = ensure_mlp_bwd(p);
    if (rc != MOLANN_OK) return rc;
    if (!grad_params) return launch_mlp_bwd(p, f, grad_out, (long)n, grad_f, nullptr, (hipStream_t)stream); // no workspace involved
    BwdGuard guard(p, (hipStream_t)stream);
    if (guard.rc != 0) return guard.rc;
    return launch_mlp_bwd(p, f, grad_out, (long)n, grad_f, grad_params, (hipStream_t)stream);
}

// diagnostic / test hook: generate (and optionally compile, needs no GPU) the plan-specialised kernel
// source for a description.  Returns the source length, or a negative MOLANN_E_* / positive hiprtcResult.
int molann_debug_jit(const molann_plan_desc* d, int do_compile, char* buf, int cap) {
    const int v = validate_desc(d);
    if (v != MOLANN_OK) return v;
    if (do_compile & 512) { // values + vjp in one launch for frames the lane kernels do not take (molann_group_vjp.inc), as the plan would build it
        std::vector<ItemDev> items;
        const int d_feat = expand_items(d, items);
        if (items.empty()) return MOLANN_E_UNSUPPORTED;
        std::vector<int> dims, kp, jp;
        std::vector<long> woff;
        if (d->n_layers > 0) {   // the heads the plan's mlp_spec describes (the fused MLP's limits), with a served activation
            const int act = d->activation;
            if (d->mlp_precision != MOLANN_MLP_F32 || d->n_layers > LANE_MLP_MAX_LAYERS || d_feat > LANE_MLP_MAX_WIDTH) return MOLANN_E_UNSUPPORTED;
            if (!(act == 0 || act == 1 || act == 2 || act == 3 || act == 5 || act == 7)) return MOLANN_E_UNSUPPORTED;
            dims.assign(d->layer_dims, d->layer_dims + d->n_layers + 1);
            for (int v : dims) if (v > LANE_MLP_MAX_WIDTH) return MOLANN_E_UNSUPPORTED;
            long off = 0;
            for (int l = 0; l < d->n_layers; ++l) {   // the plan's fp32 MFMA copy: Wp[Jp][Kp] then bias[Jp], 16-byte aligned
                kp.push_back(ceil_to(dims[l], 16)); jp.push_back(ceil_to(dims[l + 1], 16)); woff.push_back(off);
                off += (long)jp.back() * kp.back() + jp.back();
                off = (off + 3) & ~3l;
            }
        }
        std::vector<int> atoms, ptr, list;
        group_vjp_tables(d->n_inp, items, d->align_idx, d->n_align, atoms, ptr, list);
        GroupVjpGeom g;
        if (!group_vjp_geometry(dims, d->activation, d_feat, d->n_align, (int)items.size(), (int)atoms.size(), (int)list.size(), g)) return MOLANN_E_UNSUPPORTED;
        const std::string src = jit_source_group_vjp(dims, kp, jp, woff, d->activation, d_feat, d->n_inp, d->n_align, (int)items.size(), (int)atoms.size(),
                                                     (int)list.size(), g);
        if (buf && cap > 0) snprintf(buf, (size_t)cap, "%s", src.c_str());
        if (do_compile & 1) {
            std::vector<char> code;
            std::string log;
            const int rc = jit_compile(src, code, log);
            if (rc != 0) {
                if (buf && cap > 0) snprintf(buf, (size_t)cap, "%s", log.c_str());
                return rc > 0 ? rc : MOLANN_E_UNSUPPORTED;
            }
        }
        return (int)src.size();
    }
    if (do_compile & 256) { // the backward of a wide fp32 head (molann_chain_bwd.inc), as plan creation would specialise it
        if (d->n_layers <= 0) return MOLANN_E_STAGE;
        if (d->mlp_precision != MOLANN_MLP_F32) return MOLANN_E_UNSUPPORTED;
        const int act = d->activation;
        if (!(act == 0 || act == 1 || act == 2 || act == 3 || act == 5 || act == 7)) return MOLANN_E_UNSUPPORTED;
        ChainGeom cg;
        memset(&cg, 0, sizeof(cg));
        cg.nl = d->n_layers;
        for (int i = 0; i <= d->n_layers; ++i) cg.dims[i] = d->layer_dims[i];
        if (!chain_resident(cg)) return MOLANN_E_UNSUPPORTED;
        std::vector<int> dims(d->layer_dims, d->layer_dims + d->n_layers + 1), kp, jp;
        std::vector<long> woff;
        long off = 0;
        for (int l = 0; l < d->n_layers; ++l) {   // the plan's fp32 MFMA copy: Wp[Jp][Kp] then bias[Jp], 16-byte aligned
            kp.push_back(ceil_to(dims[l], 16)); jp.push_back(ceil_to(dims[l + 1], 16)); woff.push_back(off);
            off += (long)jp.back() * kp.back() + jp.back();
            off = (off + 3) & ~3l;
        }
        const int waves = chain_bwd_waves(kp, jp);
        if (waves <= 0) return MOLANN_E_UNSUPPORTED;
        const std::string csrc = jit_source_chain_bwd(dims, kp, jp, woff, act, waves);
        if (buf && cap > 0) snprintf(buf, (size_t)cap, "%s", csrc.c_str());
        if (do_compile & 1) {
            std::vector<char> code;
            std::string log;
            const int rc = jit_compile(csrc, code, log);
            if (rc != 0) {
                if (buf && cap > 0) snprintf(buf, (size_t)cap, "%s", log.c_str());
                return rc > 0 ? rc : MOLANN_E_UNSUPPORTED;
            }
        }
        return (int)csrc.size();
    }
    if (do_compile & 4) { // the wide bf16 MLP kernel of the same plan (FB as plan creation would choose it)
        if (d->n_layers <= 0) return MOLANN_E_STAGE;
        ChainGeom cg;
        memset(&cg, 0, sizeof(cg));
        cg.nl = d->n_layers;
        cg.bf16 = d->mlp_precision == MOLANN_MLP_BF16 ? 1 : 0;
        for (int i = 0; i <= d->n_layers; ++i) cg.dims[i] = d->layer_dims[i];
        int fb = 0;
        for (int f = 4; f >= 1 && fb == 0; --f)
            if (f * cg.regs_per_fb() <= (chain_resident(cg) ? 256 : 400)) fb = f;
        if (fb == 0 || (!chain_resident(cg) && 2 * cg.slab_max() * 1024 > 163840 - 1024)) return MOLANN_E_UNSUPPORTED;
        const std::string csrc = jit_source_chain(cg, d->activation, fb);
        if (buf && cap > 0) snprintf(buf, (size_t)cap, "%s", csrc.c_str());
        if (do_compile & 1) {
            std::vector<char> code;
            std::string log;
            const int rc = jit_compile(csrc, code, log);
            if (rc != 0) {
                if (buf && cap > 0) snprintf(buf, (size_t)cap, "%s", log.c_str());
                return rc > 0 ? rc : MOLANN_E_UNSUPPORTED;
            }
        }
        return (int)csrc.size();
    }
    JitSpec j;
    std::vector<int> slot_of(d->n_inp, -1);
    auto slot = [&](int atom) {
        if (slot_of[atom] < 0) { slot_of[atom] = (int)j.slots.size(); j.slots.push_back(atom); }
        return slot_of[atom];
    };
    for (int i = 0; i < d->n_align; ++i)
        if (slot(d->align_idx[i]) != i) return MOLANN_E_UNSUPPORTED;
    int col = 0;
    for (int f = 0; f < d->n_features; ++f) {
        const int* idx = d->feat_idx + d->feat_ptr[f];
        const int cnt = d->feat_ptr[f + 1] - d->feat_ptr[f], t = d->feat_type[f];
        if (t == MOLANN_FEAT_POSITION) {
            for (int i = 0; i < cnt; ++i) { ItemDev it = {IT_POSITION, col, {slot(idx[i]), 0, 0, 0}, {0, 0}}; it.idx[1] = it.idx[2] = it.idx[3] = it.idx[0]; j.items.push_back(it); col += 3; }
        } else {
            ItemDev it;
            it.type = t == MOLANN_FEAT_ANGLE ? (d->use_angle_value ? IT_ANGLE_VAL : IT_ANGLE_COS)
                      : t == MOLANN_FEAT_BOND ? IT_BOND : (d->use_angle_value ? IT_DIHEDRAL_VAL : IT_DIHEDRAL_CS);
            it.col = col;
            for (int i = 0; i < 4; ++i) it.idx[i] = slot(idx[i < cnt ? i : 0]);
            it.pad[0] = it.pad[1] = 0;
            j.items.push_back(it);
            col += item_width(it.type);
        }
    }
    if (j.items.empty() || (int)j.items.size() > JIT_MAX_ITEMS || (int)j.slots.size() > JIT_MAX_SLOTS) return MOLANN_E_UNSUPPORTED;
    j.n_inp = d->n_inp; j.n_align = d->n_align; j.act = d->activation; j.d_feat = col;
    j.n_layers = d->n_layers; j.out_cols = d->n_layers > 0 ? d->layer_dims[d->n_layers] : col;
    if (d->n_layers > 0) j.dims.assign(d->layer_dims, d->layer_dims + d->n_layers + 1);
    molann_plan::LaneGeom g;
    j.win = compact_windows(j.slots, d->n_inp);
    if (do_compile & 128) { // the WIDE_MLP build (the whole forward of a wide head in the lane kernel)
        if (d->n_layers <= 0 || d->mlp_precision != MOLANN_MLP_F32) return MOLANN_E_STAGE;
        ChainGeom cg;
        memset(&cg, 0, sizeof(cg));
        cg.nl = d->n_layers; cg.bf16 = 0;
        for (int i = 0; i <= d->n_layers; ++i) cg.dims[i] = d->layer_dims[i];
        if (!chain_resident(cg) || cg.total_frags() * 1024 > 112 * 1024) return MOLANN_E_UNSUPPORTED;
        j.wide_mlp = true; j.img_bytes = (int)(cg.total_frags() * 1024);
    }
    jit_geometry(j, g, col, std::max(1, d->n_layers > 0 ? ceil_to(col, 4) : col), j.wide_mlp ? 8 : 14);
    if (!g.ok || 3 * d->n_inp < 4) return MOLANN_E_UNSUPPORTED;
    j.waves_per_eu = 2;
    j.save_feat = (do_compile & 32) != 0 && j.n_layers > 0;   // the feature-keeping twin of the fused forward
    std::string src = jit_source(j);
    if (do_compile & 2) { // the backward kernel of the same plan
        JitSpecBox b;
        b.j = j;
        long off = 0;
        for (int l = 0; l < j.n_layers; ++l) {
            const int kp = ceil_to(j.dims[l], 16), jp = ceil_to(j.dims[l + 1], 16);
            b.kp.push_back(kp); b.jp.push_back(jp); b.woff.push_back(off);
            off += (long)jp * kp + jp;
            off = (off + 3) & ~3l;
        }
        if (do_compile & 16) { // ... in one pass (molann_bwd_ring.inc)
            if (j.n_layers > 0)
                for (int v : j.dims) if (v > 32) return MOLANN_E_UNSUPPORTED;
            long np = 0;
            for (int l = 0; l < j.n_layers; ++l) np += (long)j.dims[l + 1] * j.dims[l] + j.dims[l + 1];
            if (!bwd_ring_geometry(b.j, (int)np)) return MOLANN_E_UNSUPPORTED;
            b.j.with_values = (do_compile & 64) != 0;          // ... the build that also stores the forward's outputs (molann_value_and_vjp_f32)
            src = jit_source_bwd_ring(b);
        } else if (do_compile & 8) { // ... its MLP half (molann_mlp_bwd.inc)
            if (j.n_layers <= 0) return MOLANN_E_STAGE;
            for (int v : j.dims) if (v > 32) return MOLANN_E_UNSUPPORTED;
            const int rows = mlp_bwd_rows(j.dims, j.act);
            const int wpb = (int)std::min<long>(8, (163840 - 64) / ((long)rows * 68 * 4));
            if (wpb < 1) return MOLANN_E_UNSUPPORTED;
            src = jit_source_mlp_bwd(b, wpb);
        } else {             // ... its preprocessing half (molann_lane_bwd.inc)
            molann_plan::LaneGeom gb;
            lane_geometry(gb, 64 * d->n_inp * 12, 1);
            b.j.wpb = gb.wpb;
            src = jit_source_bwd(b, gb.lds_per_wave);
        }
    }
    if (buf && cap > 0) snprintf(buf, (size_t)cap, "%s", src.c_str());
    if (do_compile & 1) {
        std::vector<char> code;
        std::string log;
        const int rc = jit_compile(src, code, log, (do_compile & 2) ? nullptr : "-fno-slp-vectorize");
        if (rc != 0) {
            if (buf && cap > 0) snprintf(buf, (size_t)cap, "%s", log.c_str());
            return rc > 0 ? rc : MOLANN_E_UNSUPPORTED;
        }
    }
    return (int)src.size();
}

// diagnostic: read and clear the phase-stamp sums (16 x u64; [0..5] consumer phases, [6] clock ratio, [7] = number of
// consumer waves that reported, [8..10] loader: waiting for a free slot / issuing DMA / waiting for a tile to land,
// [11] loader waves, [12] tiles issued)
int molann_debug_read_stamps(unsigned long long* out16) {
    if (!out16) return MOLANN_E_NULL;
    unsigned long long zero[16] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_stamps), sizeof(zero)));
    HIP_TRY(hipMemcpyToSymbol(HIP_SYMBOL(g_stamps), zero, sizeof(zero)));
    return MOLANN_OK;
}

// ---- self-test hooks: the same __host__ __device__ source, compiled for the host -------------
int molann_selftest_kabsch_rotation(const double* H9, double e0, float* R9) {
    if (!H9 || !R9) return MOLANN_E_NULL;
    double h[9];
    float r[9];
    for (int i = 0; i < 9; ++i) h[i] = H9[i];
    kabsch_rotation(h, e0, r);
    for (int i = 0; i < 9; ++i) R9[i] = r[i];
    return MOLANN_OK;
}

int molann_selftest_kabsch_rotation_f32(const float* H9, float e0, float* R9) {
    if (!H9 || !R9) return MOLANN_E_NULL;
    float h[9], r[9];
    for (int i = 0; i < 9; ++i) h[i] = H9[i];
    kabsch_rotation_f32(h, e0, r);
    for (int i = 0; i < 9; ++i) R9[i] = r[i];
    return MOLANN_OK;
}

int molann_selftest_feature(int type, int use_angle_value, const float* a, float* out3) {
    if (!a || !out3) return MOLANN_E_NULL;
    int it;
    if (type == MOLANN_FEAT_ANGLE) it = use_angle_value ? IT_ANGLE_VAL : IT_ANGLE_COS;
    else if (type == MOLANN_FEAT_BOND) it = IT_BOND;
    else if (type == MOLANN_FEAT_DIHEDRAL) it = use_angle_value ? IT_DIHEDRAL_VAL : IT_DIHEDRAL_CS;
    else if (type == MOLANN_FEAT_POSITION) it = IT_POSITION;
    else return MOLANN_E_FEATURE;
    float v[3] = {0.f, 0.f, 0.f};
    const int w = eval_item(it, v3(a[0], a[1], a[2]), v3(a[3], a[4], a[5]), v3(a[6], a[7], a[8]), v3(a[9], a[10], a[11]), v);
    for (int i = 0; i < w; ++i) out3[i] = v[i];
    return w;
}

float molann_selftest_activation(int act, float v) { return apply_activation(act, v); }

int molann_selftest_feature_backward(int type, int use_angle_value, const float* a, const float* g3, float* ga12) {
    if (!a || !g3 || !ga12) return MOLANN_E_NULL;
    int it;
    if (type == MOLANN_FEAT_ANGLE) it = use_angle_value ? IT_ANGLE_VAL : IT_ANGLE_COS;
    else if (type == MOLANN_FEAT_BOND) it = IT_BOND;
    else if (type == MOLANN_FEAT_DIHEDRAL) it = use_angle_value ? IT_DIHEDRAL_VAL : IT_DIHEDRAL_CS;
    else if (type == MOLANN_FEAT_POSITION) it = IT_POSITION;
    else return MOLANN_E_FEATURE;
    V3 g[4] = {v3(0, 0, 0), v3(0, 0, 0), v3(0, 0, 0), v3(0, 0, 0)};
    const float gg[3] = {g3[0], g3[1], g3[2]};
    eval_item_backward(it, v3(a[0], a[1], a[2]), v3(a[3], a[4], a[5]), v3(a[6], a[7], a[8]), v3(a[9], a[10], a[11]), gg, g[0],
                       g[1], g[2], g[3]);
    for (int i = 0; i < 4; ++i) { ga12[3 * i] = g[i].x; ga12[3 * i + 1] = g[i].y; ga12[3 * i + 2] = g[i].z; }
    return MOLANN_OK;
}

int molann_selftest_kabsch_backward(const double* H9, const float* R9, const float* GR9, float* GH9) {
    if (!H9 || !R9 || !GR9 || !GH9) return MOLANN_E_NULL;
    double h[9];
    float r[9], gr[9], gh[9];
    for (int i = 0; i < 9; ++i) { h[i] = H9[i]; r[i] = R9[i]; gr[i] = GR9[i]; }
    kabsch_rotation_backward(h, r, gr, gh);
    for (int i = 0; i < 9; ++i) GH9[i] = gh[i];
    return MOLANN_OK;
}

float molann_selftest_act_derivative(int act, float z) { return act_derivative(act, z, apply_activation(act, z)); }

static int selftest_item_type(int type, int use_angle_value) {
    if (type == MOLANN_FEAT_ANGLE) return use_angle_value ? IT_ANGLE_VAL : IT_ANGLE_COS;
    if (type == MOLANN_FEAT_BOND) return IT_BOND;
    if (type == MOLANN_FEAT_DIHEDRAL) return use_angle_value ? IT_DIHEDRAL_VAL : IT_DIHEDRAL_CS;
    if (type == MOLANN_FEAT_POSITION) return IT_POSITION;
    return -1;
}

int molann_selftest_feature_tangent_f32(int type, int use_angle_value, const float* a, const float* t, float* out3, float* dout3) {
    if (!a || !t || !out3 || !dout3) return MOLANN_E_NULL;
    const int it = selftest_item_type(type, use_angle_value);
    if (it < 0) return MOLANN_E_FEATURE;
    float v[3] = {0.f, 0.f, 0.f}, dv[3] = {0.f, 0.f, 0.f};
    const int w = eval_item_tangent(it, v3(a[0], a[1], a[2]), v3(a[3], a[4], a[5]), v3(a[6], a[7], a[8]), v3(a[9], a[10], a[11]),
                                    v3(t[0], t[1], t[2]), v3(t[3], t[4], t[5]), v3(t[6], t[7], t[8]), v3(t[9], t[10], t[11]), v, dv);
    for (int i = 0; i < w; ++i) { out3[i] = v[i]; dout3[i] = dv[i]; }
    return w;
}

int molann_selftest_feature_tangent_f64(int type, int use_angle_value, const double* a, const double* t, double* out3, double* dout3) {
    if (!a || !t || !out3 || !dout3) return MOLANN_E_NULL;
    const int it = selftest_item_type(type, use_angle_value);
    if (it < 0) return MOLANN_E_FEATURE;
    double v[3] = {0., 0., 0.}, dv[3] = {0., 0., 0.};
    const int w = eval_item_tangent_f64(it, v3d(a[0], a[1], a[2]), v3d(a[3], a[4], a[5]), v3d(a[6], a[7], a[8]), v3d(a[9], a[10], a[11]),
                                        v3d(t[0], t[1], t[2]), v3d(t[3], t[4], t[5]), v3d(t[6], t[7], t[8]), v3d(t[9], t[10], t[11]), v, dv);
    for (int i = 0; i < w; ++i) { out3[i] = v[i]; dout3[i] = dv[i]; }
    return w;
}

int molann_selftest_kabsch_rotation_f64(const double* H9, double e0, double* R9) {
    if (!H9 || !R9) return MOLANN_E_NULL;
    double h[9], r[9];
    for (int i = 0; i < 9; ++i) h[i] = H9[i];
    kabsch_rotation_t<double, double>(h, e0, r);
    for (int i = 0; i < 9; ++i) R9[i] = r[i];
    return MOLANN_OK;
}

int molann_selftest_kabsch_tangent(const double* H9, const double* R9, const double* dH9, double* dR9) {
    if (!H9 || !R9 || !dH9 || !dR9) return MOLANN_E_NULL;
    double h[9], r[9], dh[9], dr[9];
    for (int i = 0; i < 9; ++i) { h[i] = H9[i]; r[i] = R9[i]; dh[i] = dH9[i]; }
    kabsch_rotation_tangent_t<double>(h, r, dh, dr);
    for (int i = 0; i < 9; ++i) dR9[i] = dr[i];
    return MOLANN_OK;
}

int molann_selftest_kabsch_backward_f64(const double* H9, const double* R9, const double* GR9, double* GH9) {
    if (!H9 || !R9 || !GR9 || !GH9) return MOLANN_E_NULL;
    double h[9], r[9], gr[9], gh[9];
    for (int i = 0; i < 9; ++i) { h[i] = H9[i]; r[i] = R9[i]; gr[i] = GR9[i]; }
    kabsch_rotation_backward_t<double, double>(h, r, gr, gh);
    for (int i = 0; i < 9; ++i) GH9[i] = gh[i];
    return MOLANN_OK;
}

} // extern "C"
