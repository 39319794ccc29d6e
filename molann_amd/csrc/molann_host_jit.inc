// molann_host_jit.inc - part of libmolann_hip.so, included by molann_kernels.hip (one translation unit: the kernels' host stubs and the
// launches that use them must see each other).  Host: plan-time specialisation through hipRTC - source generation from the plan, compilation, the on-disk code-object cache.
namespace {

// ---------------------------------------------------------------------------------------------
// plan-time specialisation of the lane kernel (molann_lane_jit.inc) through hipRTC
// ---------------------------------------------------------------------------------------------
struct RtcApi {
    decltype(&hiprtcCreateProgram) create;
    decltype(&hiprtcCompileProgram) compile;
    decltype(&hiprtcGetCodeSize) code_size;
    decltype(&hiprtcGetCode) code;
    decltype(&hiprtcGetProgramLogSize) log_size;
    decltype(&hiprtcGetProgramLog) log;
    decltype(&hiprtcDestroyProgram) destroy;
    decltype(&hiprtcVersion) version;   // optional: part of the code-object cache's key
    bool ok;
};

const RtcApi* rtc_api() {
    static RtcApi api = [] {
        RtcApi a;
        memset(&a, 0, sizeof(a));
        void* h = dlopen("libhiprtc.so", RTLD_NOW | RTLD_LOCAL);
        if (!h) h = dlopen("libhiprtc.so.7", RTLD_NOW | RTLD_LOCAL);
        if (!h) h = dlopen("/opt/rocm/lib/libhiprtc.so", RTLD_NOW | RTLD_LOCAL);
        if (!h) return a;
        a.create = (decltype(a.create))dlsym(h, "hiprtcCreateProgram");
        a.compile = (decltype(a.compile))dlsym(h, "hiprtcCompileProgram");
        a.code_size = (decltype(a.code_size))dlsym(h, "hiprtcGetCodeSize");
        a.code = (decltype(a.code))dlsym(h, "hiprtcGetCode");
        a.log_size = (decltype(a.log_size))dlsym(h, "hiprtcGetProgramLogSize");
        a.log = (decltype(a.log))dlsym(h, "hiprtcGetProgramLog");
        a.destroy = (decltype(a.destroy))dlsym(h, "hiprtcDestroyProgram");
        a.version = (decltype(a.version))dlsym(h, "hiprtcVersion");
        a.ok = a.create && a.compile && a.code_size && a.code && a.log_size && a.log && a.destroy;
        return a;
    }();
    return &api;
}

std::string join_chunks(const char* const* chunks) {
    std::string s;
    for (int i = 0; chunks[i]; ++i) s += chunks[i];
    return s;
}

struct JitSpec { // what the specialised kernel is compiled for
    int n_inp, n_align, n_layers, act, d_feat, out_cols, wpb, lds_per_wave, fbuf_off;
    int waves_per_eu = 2;             // occupancy the backward kernel is compiled for (amdgpu_waves_per_eu)
    int nbuf = 1;
    bool save_feat = false;           // forward kernel: also writes the features (training; molann_forward_train_f32)
    bool with_values = false;         // one-pass backward kernel: also writes the forward's outputs (molann_value_and_vjp_f32)
    bool wide_mlp = false;            // forward kernel: hidden widths beyond 32 - the chain MLP's arithmetic on a weight stream resident at img_off
    int img_bytes = 0;                // ... its size
    bool frag_lds = false;            // one-pass backward: weight fragments in an LDS image at img_off instead of registers
    int img_off = 0;
    // forward kernel: loader / consumer block around a ring of tile slots (molann_lane_jit.inc)
    int nload = 1;                    // loaders per block
    int ncons = 0, nslot = 0, depth = 0, ring_off = 0, tile_stride = 0, fb_off = 0, fb_bytes = 0, lds_block = 0, bpc = 0;
    std::vector<int> win;             // compact staging: first dword of each 16-byte window copied per frame
    std::vector<int> slots;           // slot -> atom
    std::vector<ItemDev> items;       // atoms as slot indices
    std::vector<int> dims;
};

constexpr int JIT_MAX_ITEMS = 128, JIT_MAX_SLOTS = 32;
} // namespace
struct JitSpecBox { JitSpec j; std::vector<int> kp, jp; std::vector<long> woff; };
namespace {

// Compact staging (molann_lane_jit.inc): per frame only the 16-byte windows that hold a touched atom are copied
// to LDS.  Greedy cover of the touched dwords (LDS-DMA gathers from any dword-aligned address); an odd number of
// windows keeps the per-lane ds_read_b128 of the register fill conflict-free (frame stride = NW x 16 B).
std::vector<int> compact_windows(const std::vector<int>& slot_atoms, int n_inp) {
    const int frame_dw = 3 * n_inp;
    std::vector<char> used(frame_dw, 0);
    for (int a : slot_atoms)
        for (int c = 0; c < 3; ++c) used[3 * a + c] = 1;
    std::vector<int> win;
    for (int d = 0; d < frame_dw; ++d) {
        if (!used[d]) continue;
        if (!win.empty() && d < win.back() + 4) continue; // covered by the last window
        win.push_back(std::min(d, frame_dw - 4));      // never past the end of the frame (the last frame of x)
    }
    if (win.empty()) win.push_back(0);
    if (win.size() % 2 == 0) win.push_back(win.back());
    return win;
}

// LDS geometry of the specialised forward kernel: per block a header of hand-off words, a ring of NSLOT compact
// tiles and one feature staging buffer per consumer wave (the fused MLP reads only the real D_FEAT rows; padded k's
// are zeros in registers).  A block is NCONS consumers + 1 loader; blocks <= 64 KiB (the LDS-DMA destination offset
// is 16 bits).  Preference: 8 consumers per CU (two per SIMD: the arithmetic saturates the vector ALU there), then
// the deepest ring, then the fewest blocks (= loader waves).
void jit_geometry(JitSpec& j, molann_plan::LaneGeom& g, int staging_rows, int fallback_cols, int max_cons = 14) {
    const int tile = ceil_to(64 * 16 * (int)j.win.size(), 16);
    const int img = j.wide_mlp ? ceil_to(j.img_bytes, 1024) + 1024 : 0;   // WIDE_MLP: the resident weight stream behind the consumers' buffers (+ its alignment)
    const int fb = ceil_to(std::max(1, staging_rows) * FB_STRIDE * 4, 16);
    // One block per CU: 14 consumer waves + 2 loaders = four waves per SIMD (the kernel is built for <= 128 VGPRs).
    // Two loaders because a wave has at most 63 vector-memory operations in flight (vmcnt) = 63 KB of tiles, and
    // the loaded HBM latency (~4 us, tools/stamps.py) needs ~120 KB in flight per CU for 6 TB/s; the consumers beyond
    // two per SIMD add no vector-ALU rate but keep the SIMD issuing while others wait (LDS, MFMA results, a tile).
    j.bpc = 1;
    j.ncons = max_cons;
    j.nload = 2;
    const int header = 256;
    long nslot = 0;
    auto fit = [&]() {
        nslot = std::min<long>(16, (163840 / j.bpc - header - img - (long)j.ncons * fb) / tile);
        return nslot >= 2 * j.nload || (j.ncons == 1 && nslot >= 1);
    };
    while (!fit() && j.ncons > 1) { --j.ncons; if (j.ncons < 4) j.nload = 1; }   // large tiles: fewer consumers, down to one
    bool ok = fit();
    if (const char* e = diag_env("MOLANN_DEBUG_LC")) { // experiments: "blocks per CU,consumers,slots,loaders"
        int b = 0, c = 0, n = 0, ld = 1;
        if (sscanf(e, "%d,%d,%d,%d", &b, &c, &n, &ld) >= 3 && b >= 1 && c >= 1 && c <= 15 && n >= 1 && n <= 16 && ld >= 1 && ld <= 4 &&
            header + img + (long)n * tile + (long)c * fb <= 163840 / b) {
            j.bpc = b; j.ncons = c; nslot = n; j.nload = ld; ok = true;
        }
    }
    g.ok = ok ? 1 : 0;
    if (!g.ok) { lane_geometry(g, tile, fallback_cols); g.ok = 0; return; }
    j.nslot = (int)nslot;
    const int nw = (int)j.win.size();
    j.depth = std::min(6, 63 / std::max(1, nw));   // tiles a loader keeps in flight behind its newest published one: vmcnt <= 63
    j.depth = std::min(j.depth, std::max(0, j.nslot / j.nload - 1));
    if (const char* e = diag_env("MOLANN_DEBUG_LC_DEPTH")) j.depth = std::max(0, std::min(j.depth, atoi(e)));
    j.ring_off = header;
    j.tile_stride = tile;
    j.fb_off = header + j.nslot * tile;
    j.fb_bytes = fb;
    j.lds_block = j.fb_off + j.ncons * fb;
    if (j.wide_mlp) { j.img_off = ceil_to(j.lds_block, 1024); j.lds_block = j.img_off + img - 1024; }
    j.nbuf = 1;
    // (the fields of the older one-buffer-per-wave geometry stay filled: the backward kernel's preamble names them)
    g.wpb = std::min(4, j.ncons); g.lds_per_wave = tile + std::max(fb, 16); g.fbuf_off = tile;
    j.wpb = g.wpb; j.lds_per_wave = g.lds_per_wave; j.fbuf_off = g.fbuf_off;
}

std::string jit_preamble(const JitSpec& j);

std::string jit_source(const JitSpec& j) {
    std::string s = jit_preamble(j);
    s += "#line 1 \"molann_ring.inc\"\n";
    s += join_chunks(k_src_molann_ring_inc);
    if (j.wide_mlp) {
        s += "#define MOLANN_CHAIN_CORE_ONLY 1\n#line 1 \"molann_mlp_jit.inc\"\n";
        s += join_chunks(k_src_molann_mlp_jit_inc);
    }
    s += "#line 1 \"molann_lane_jit.inc\"\n";
    s += join_chunks(k_src_molann_lane_jit_inc);
    return s;
}

// wide bf16 MLP: layer widths, activation and frames per wave as constants
// the whole weight stream resident in LDS (molann_mlp_jit.inc: RESIDENT): no streaming, eight waves per block
inline bool chain_resident(const ChainGeom& g) { return g.total_frags() * 1024 <= 150 * 1024; }
inline int chain_waves(const ChainGeom& g) { return chain_resident(g) ? 8 : 4; }
// streaming: LDS slab buffers of the ring (NSLAB - 1 slabs in flight), as many as 160 KB less 2 KB hold, 2 to 4; resident: 1.
// The kernel takes this number from its preamble and the launch info reports it.
inline int chain_nslab(const ChainGeom& g) {
    if (chain_resident(g)) return 1;
    const int fit = (160 * 1024 - 2048) / (g.slab_max() * 1024);
    return fit >= 4 ? 4 : (fit >= 3 ? 3 : 2);
}

std::string jit_source_chain(const ChainGeom& g, int act, int fb) {
    std::string s = "// preamble generated from the plan\n";
    char t[160];
    snprintf(t, sizeof(t), "constexpr int NL = %d;\n", g.nl); s += t;
    s += "constexpr int DIMS[] = {";
    for (int i = 0; i <= g.nl; ++i) { snprintf(t, sizeof(t), "%s%d", i ? ", " : "", g.dims[i]); s += t; }
    s += "};\n";
    snprintf(t, sizeof(t), "constexpr int ACT = %d;\nconstexpr int FB = %d;\nconstexpr bool BF16 = %s;\n", act, fb, g.bf16 ? "true" : "false"); s += t;
    snprintf(t, sizeof(t), "constexpr bool RESIDENT = %s;\nconstexpr int WAVES = %d;\nconstexpr int NSLAB = %d;\n", chain_resident(g) ? "true" : "false",
             chain_waves(g), chain_nslab(g)); s += t;
    { const char* e = diag_env("MOLANN_DEBUG_CHAIN"); snprintf(t, sizeof(t), "constexpr int CHAIN_DIAG = %d;\n", e ? atoi(e) : 0); s += t; }   // diagnostics build: timing ablations (wrong results)
    s += "#line 1 \"molann_mlp_jit.inc\"\n";
    s += join_chunks(k_src_molann_mlp_jit_inc);
    return s;
}

// backward of the preprocessing: the forward preamble of the plan without its MLP
std::string jit_source_bwd(const JitSpecBox& b, int lds_per_wave) {
    JitSpec j = b.j;
    j.lds_per_wave = lds_per_wave;
    j.n_layers = 0;
    j.out_cols = j.d_feat;
    j.dims.clear();
    std::string s = jit_preamble(j);
    s += "#line 1 \"molann_lane_bwd.inc\"\n";
    s += join_chunks(k_src_molann_lane_bwd_inc);
    return s;
}

// rows of the [unit][frame] scratch of molann_mlp_bwd.inc (the kernel text computes the same number: n_rows())
int mlp_bwd_rows(const std::vector<int>& dims, int act) {
    const int nl = (int)dims.size() - 1;
    auto pad4 = [](int v) { return (v + 3) & ~3; };
    auto b16 = [](int v) { return (v + 15) >> 4; };
    auto act_row = [&](int l) { int r = 0; for (int i = 0; i < l; ++i) r += pad4(dims[i]); return r; };
    auto z_row = [&](int l) { int r = act_row(nl); for (int i = 0; i < l; ++i) r += pad4(dims[i + 1]); return r; };
    const int z_end = act == 5 ? z_row(nl - 1) : act_row(nl);
    auto d_row = [&](int l) { return l == nl - 1 ? z_end : act_row(l + 1); };
    int m = z_end + pad4(dims[nl]);
    for (int l = 0; l < nl; ++l) m = std::max(m, std::max(act_row(l) + 16 * b16(dims[l]), d_row(l) + 16 * b16(dims[l + 1])));
    return m;
}

// backward of the MLP: layer widths, activation, where the weights live (fp32 MFMA copy: Wp[Jp][Kp], bias[Jp]) and
// the layout of the parameter-gradient buffer (torch layout: dW[J][K] then db[J], layer after layer)
std::string jit_source_mlp_bwd(const JitSpecBox& b, int wpb) {
    const JitSpec& j = b.j;
    std::string s = "// preamble generated from the plan\n";
    char t[128];
    auto K = [&](const char* name, int v) { snprintf(t, sizeof(t), "constexpr int %s = %d;\n", name, v); s += t; };
    auto arr = [&](const char* name, const std::vector<long>& v) {
        s += std::string("constexpr int ") + name + "[] = {";
        for (size_t i = 0; i < v.size(); ++i) { snprintf(t, sizeof(t), "%s%ld", i ? ", " : "", v[i]); s += t; }
        s += "};\n";
    };
    K("NL", j.n_layers); K("ACT", j.act); K("WPB_M", wpb);
    std::vector<long> dims(j.dims.begin(), j.dims.end()), kp(b.kp.begin(), b.kp.end()), jp(b.jp.begin(), b.jp.end()), woff = b.woff, goff;
    long g = 0;
    for (int l = 0; l < j.n_layers; ++l) { goff.push_back(g); g += (long)j.dims[l + 1] * j.dims[l] + j.dims[l + 1]; }
    arr("DIMS", dims); arr("KP", kp); arr("JP", jp); arr("WOFF", woff); arr("GOFF", goff);
    K("N_PARAMS", (int)g);
    s += "constexpr bool FRAG_LDS = false;\n";   // this kernel's waves have the registers for their weight fragments
    s += "constexpr bool WITH_VALUES = false;\n";
    s += "#line 1 \"molann_mlp_tile.inc\"\n";
    s += join_chunks(k_src_molann_mlp_tile_inc);
    s += "#line 1 \"molann_mlp_bwd.inc\"\n";
    s += join_chunks(k_src_molann_mlp_bwd_inc);
    return s;
}

// backward of a wide fp32 head (molann_chain_bwd.inc): LDS floats of the kernel text's LDS_FLOATS - the weight copy at row
// stride Kp + 4 with its biases, and the block's [unit][frame] tile of 16 WAVES frames (row stride + 4)
long chain_bwd_lds_floats(const std::vector<int>& kp, const std::vector<int>& jp, int waves) {
    long w = 0;
    int rows = 0;
    for (size_t l = 0; l < kp.size(); ++l) { w += (long)jp[l] * (kp[l] + 4) + jp[l]; rows = std::max(rows, jp[l] + kp[l]); }
    return w + (long)rows * (16 * waves + 4);
}
// waves per block: four (a 64-frame tile) where weights and tile fit the CU's LDS, else fewer; 0 when not even one does
int chain_bwd_waves(const std::vector<int>& kp, const std::vector<int>& jp) {
    for (int w : {4, 2, 1})
        if (chain_bwd_lds_floats(kp, jp, w) * 4 <= 163840) return w;
    return 0;
}

std::string jit_source_chain_bwd(const std::vector<int>& dims, const std::vector<int>& kp, const std::vector<int>& jp,
                                 const std::vector<long>& woff, int act, int waves) {
    std::string s = "// preamble generated from the plan\n";
    char t[128];
    const int nl = (int)dims.size() - 1;
    auto K = [&](const char* name, long v) { snprintf(t, sizeof(t), "constexpr int %s = %ld;\n", name, v); s += t; };
    auto arr = [&](const char* name, const std::vector<long>& v) {
        s += std::string("constexpr int ") + name + "[] = {";
        for (size_t i = 0; i < v.size(); ++i) { snprintf(t, sizeof(t), "%s%ld", i ? ", " : "", v[i]); s += t; }
        s += "};\n";
    };
    K("NL", nl); K("ACT", act); K("WAVES", waves);
    std::vector<long> d(dims.begin(), dims.end()), k(kp.begin(), kp.end()), j(jp.begin(), jp.end()), goff;
    long g = 0;
    for (int l = 0; l < nl; ++l) { goff.push_back(g); g += (long)dims[l + 1] * dims[l] + dims[l + 1]; }
    arr("DIMS", d); arr("KP", k); arr("JP", j); arr("WOFF", woff); arr("GOFF", goff);
    K("N_PARAMS", g);
    s += "#line 1 \"molann_chain_bwd.inc\"\n";
    s += join_chunks(k_src_molann_chain_bwd_inc);
    return s;
}

// One-pass backward (molann_bwd_ring.inc): loaders + consumers around the ring of compact tiles; every consumer owns a
// buffer that is MLP scratch, gradient tile and parameter sums in turn.  Two waves per SIMD (256 VGPRs each).
// fragments of the weights the one-pass backward keeps per lane (molann_bwd_ring.inc: frag_ids())
int bwd_ring_frags(const JitSpec& j) {
    int n = 0;
    for (int l = 0; l < j.n_layers; ++l)
        for (int b = 0; b < 2; ++b) {
            for (int s = 0; s < 8; ++s) {
                if (l + 1 < j.n_layers && 16 * b < j.dims[l + 1] && 4 * s < j.dims[l]) ++n;
                if (16 * b < j.dims[l] && 4 * s < j.dims[l + 1]) ++n;
            }
            if (l + 1 < j.n_layers && 16 * b < j.dims[l + 1]) n += 4;
        }
    return n;
}

bool bwd_ring_geometry(JitSpec& j, int n_params) {
    const int tile = ceil_to(64 * 16 * (int)j.win.size(), 16);
    const int rows = j.n_layers > 0 ? mlp_bwd_rows(j.dims, j.act) : 0;
    const int cbuf = ceil_to(std::max(std::max(64 * 12 * j.n_inp, rows * 68 * 4), std::max(16, n_params * 4)), 16);
    const int header = 256;
    j.bpc = 1;
    // weight fragments: in registers up to the C3 class (a few dozen), beyond that in an LDS image shared by the block
    const int frags = bwd_ring_frags(j);
    j.frag_lds = frags > 40;
    const int img = j.frag_lds ? frags * 256 : 0;
    // With an MLP the consumers are bound by their SIMDs' issue cycles (matrix and vector instructions of a SIMD do not overlap:
    // C3 takes 114 us per 1 M frames without the gradient tile whether 4 or 7 consumers work on it), the stream needs one
    // loader, and the seventh consumer shortens the per-wave tail of the gradient tile (152 -> 145 us).
    int c0 = j.n_layers > 0 ? 7 : 6, ld0 = j.n_layers > 0 ? 1 : 2;
    if (const char* e = diag_env("MOLANN_DEBUG_BWD_LC")) { // experiments: "consumers,loaders"
        int c = 0, ld = 0;
        if (sscanf(e, "%d,%d", &c, &ld) == 2 && c >= 1 && c <= 14 && ld >= 1 && ld <= 4) { c0 = c; ld0 = ld; }
    }
    for (int ncons = c0; ncons >= 2; --ncons) {
        const int nload = ncons >= 4 ? ld0 : 1;
        const long nslot = std::min<long>(16, (163840 - header - img - (long)ncons * cbuf) / tile);
        if (nslot < 2 * nload) continue;
        j.ncons = ncons; j.nload = nload; j.nslot = (int)nslot;
        j.depth = std::min(6, 63 / std::max(1, (int)j.win.size()));
        j.depth = std::min(j.depth, std::max(0, j.nslot / j.nload - 1));
        j.ring_off = header;
        j.tile_stride = tile;
        j.fb_off = header + j.nslot * tile;
        j.fb_bytes = cbuf;
        j.img_off = j.fb_off + j.ncons * cbuf;
        j.lds_block = j.img_off + img;
        return true;
    }
    return false;
}

std::string jit_source_bwd_ring(const JitSpecBox& b) {
    const JitSpec& j = b.j;
    std::string s = jit_preamble(j);
    char t[128];
    auto arr = [&](const char* name, const std::vector<long>& v) {
        s += std::string("constexpr int ") + name + "[] = {";
        for (size_t i = 0; i < v.size(); ++i) { snprintf(t, sizeof(t), "%s%ld", i ? ", " : "", v[i]); s += t; }
        s += "};\n";
    };
    std::vector<long> kp(b.kp.begin(), b.kp.end()), jp(b.jp.begin(), b.jp.end()), woff = b.woff, goff;
    long g = 0;
    for (int l = 0; l < j.n_layers; ++l) { goff.push_back(g); g += (long)j.dims[l + 1] * j.dims[l] + j.dims[l + 1]; }
    if (kp.empty()) { kp.push_back(1); jp.push_back(1); woff.push_back(0); goff.push_back(0); }
    arr("KP", kp); arr("JP", jp); arr("WOFF", woff); arr("GOFF", goff);
    snprintf(t, sizeof(t), "constexpr int N_PARAMS = %ld;\n", g);
    s += t;
    s += "#line 1 \"molann_ring.inc\"\n";
    s += join_chunks(k_src_molann_ring_inc);
    s += "#line 1 \"molann_mlp_tile.inc\"\n";
    s += join_chunks(k_src_molann_mlp_tile_inc);
    s += "#line 1 \"molann_bwd_ring.inc\"\n";
    s += join_chunks(k_src_molann_bwd_ring_inc);
    return s;
}

// ---- values + vector-Jacobian product of frames the lane kernels do not take, in one launch (molann_group_vjp.inc) ----------
// The description's feature list as items (column order = list order, ann.py:473); returns the feature dimension.
int expand_items(const molann_plan_desc* d, std::vector<ItemDev>& items) {
    int col = 0;
    for (int f = 0; f < d->n_features; ++f) {
        const int* idx = d->feat_idx + d->feat_ptr[f];
        const int cnt = d->feat_ptr[f + 1] - d->feat_ptr[f];
        const int t = d->feat_type[f];
        if (t == MOLANN_FEAT_POSITION) {
            for (int i = 0; i < cnt; ++i) {
                ItemDev it = {IT_POSITION, col, {idx[i], idx[i], idx[i], idx[i]}, {0, 0}};
                items.push_back(it);
                col += 3;
            }
        } else {
            ItemDev it;
            it.type = t == MOLANN_FEAT_ANGLE ? (d->use_angle_value ? IT_ANGLE_VAL : IT_ANGLE_COS)
                      : t == MOLANN_FEAT_BOND ? IT_BOND
                                              : (d->use_angle_value ? IT_DIHEDRAL_VAL : IT_DIHEDRAL_CS);
            it.col = col;
            for (int i = 0; i < 4; ++i) it.idx[i] = idx[i < cnt ? i : 0];
            it.pad[0] = it.pad[1] = 0;
            items.push_back(it);
            col += item_width(it.type);
        }
    }
    return col;
}

// Touched atoms in atom order and, per atom (CSR: ptr / list), what its gradient gathers: entries >= 0 are the g_y slots
// 4 it + j of the item atoms it is, entries < 0 the alignment rows -1 - i it has (twice for an atom named twice).
void group_vjp_tables(int n_inp, const std::vector<ItemDev>& items, const int* align_idx, int n_align, std::vector<int>& atoms,
                      std::vector<int>& ptr, std::vector<int>& list) {
    std::vector<std::vector<int>> contrib(n_inp);
    for (size_t it = 0; it < items.size(); ++it)
        for (int j = 0; j < item_atoms(items[it].type); ++j) contrib[items[it].idx[j]].push_back((int)(4 * it + j));
    for (int i = 0; i < n_align; ++i) contrib[align_idx[i]].push_back(-1 - i);
    atoms.clear(); list.clear();
    ptr.assign(1, 0);
    for (int a = 0; a < n_inp; ++a)
        if (!contrib[a].empty()) {
            atoms.push_back(a);
            list.insert(list.end(), contrib[a].begin(), contrib[a].end());
            ptr.push_back((int)list.size());
        }
}

// LDS of one block (one 64-frame tile): the tables, the head's fragment image (heads of more than 40 fragments), the tile's
// [unit][frame] scratch, 64 frame states (H, R, c0, dl: 136 bytes) and a g_y buffer per wave and frame of a round.
// B frames per round as frames_group_bwd_kernel chooses them (<= 256 items per round), at least 2; eight waves per block where
// they fit 160 KiB, then fewer, then smaller rounds.
struct GroupVjpGeom { int b, wpb, s_rows, lds, off_ref32, off_align, off_items, off_atoms, off_ptr, off_list, off_img, off_s, off_st, off_gy; bool frag_lds; };
constexpr int GROUP_VJP_STATE_BYTES = 136;
bool group_vjp_geometry(const std::vector<int>& dims, int act, int d_feat, int n_align, int n_items, int n_touched, int n_list, GroupVjpGeom& g) {
    memset(&g, 0, sizeof(g));
    JitSpec j;
    j.n_layers = dims.empty() ? 0 : (int)dims.size() - 1;
    j.dims = dims;
    const int frags = bwd_ring_frags(j);
    g.frag_lds = frags > 40;      // (as molann_bwd_ring.inc: the fragments of up to the C3 class in registers)
    g.s_rows = std::max(j.n_layers > 0 ? mlp_bwd_rows(dims, act) : 0, d_feat);
    int b0 = 8;
    while (b0 > 2 && (long)b0 * n_items > 256) b0 /= 2;
    for (int b = b0; b >= 2; b /= 2)
        for (int w : {8, 4, 2, 1}) {
            long off = ceil_to(8 * (3 * n_align + 8), 16);
            g.off_ref32 = (int)off; off += ceil_to(4 * (3 * n_align + 8), 16);
            g.off_align = (int)off; off += ceil_to(4 * n_align, 16);
            g.off_items = (int)off; off += 32l * n_items;
            g.off_atoms = (int)off; off += ceil_to(4 * n_touched, 16);
            g.off_ptr = (int)off; off += ceil_to(4 * (n_touched + 1), 16);
            g.off_list = (int)off; off += ceil_to(4 * n_list, 16);
            g.off_img = (int)off; off += g.frag_lds ? (long)frags * 256 : 0;
            g.off_s = (int)off; off += (long)g.s_rows * 68 * 4;
            g.off_st = (int)off; off += 64l * GROUP_VJP_STATE_BYTES;
            g.off_gy = (int)off; off += (long)w * b * 48 * n_items;
            if (off <= 163840) { g.b = b; g.wpb = w; g.lds = (int)off; return true; }
        }
    return false;
}

std::string jit_source_group_vjp(const std::vector<int>& dims, const std::vector<int>& kp, const std::vector<int>& jp, const std::vector<long>& woff,
                                 int act, int d_feat, int n_inp, int n_align, int n_items, int n_touched, int n_list, const GroupVjpGeom& g) {
    std::string s = "// preamble generated from the plan\n";
    char t[128];
    const int nl = dims.empty() ? 0 : (int)dims.size() - 1;
    auto K = [&](const char* name, long v) { snprintf(t, sizeof(t), "constexpr int %s = %ld;\n", name, v); s += t; };
    auto arr = [&](const char* name, const std::vector<long>& v) {
        s += std::string("constexpr int ") + name + "[] = {";
        for (size_t i = 0; i < v.size(); ++i) { snprintf(t, sizeof(t), "%s%ld", i ? ", " : "", v[i]); s += t; }
        s += "};\n";
    };
    K("NL", nl); K("ACT", act);
    std::vector<long> d(dims.begin(), dims.end()), k(kp.begin(), kp.end()), jj(jp.begin(), jp.end()), wo = woff, goff;
    long np = 0;
    for (int l = 0; l < nl; ++l) { goff.push_back(np); np += (long)dims[l + 1] * dims[l] + dims[l + 1]; }
    if (nl == 0) { d = {d_feat, 1}; k = {1}; jj = {1}; wo = {0}; goff = {0}; }   // (the tile code names DIMS[1], KP[0], ...)
    arr("DIMS", d); arr("KP", k); arr("JP", jj); arr("WOFF", wo); arr("GOFF", goff);
    K("N_PARAMS", np);
    s += g.frag_lds ? "constexpr bool FRAG_LDS = true;\n" : "constexpr bool FRAG_LDS = false;\n";
    s += "constexpr bool WITH_VALUES = true;\n";
    K("B", g.b); K("WPB", g.wpb); K("N_ALIGN", n_align); K("N_ITEMS", n_items); K("D_FEAT", d_feat); K("FRAME_DW", 3l * n_inp);
    K("N_TOUCHED", n_touched); K("N_LIST", n_list); K("S_ROWS", g.s_rows); K("FRAME_STATE_BYTES", GROUP_VJP_STATE_BYTES);
    K("OFF_REF32", g.off_ref32); K("OFF_ALIGN", g.off_align); K("OFF_ITEMS", g.off_items); K("OFF_ATOMS", g.off_atoms);
    K("OFF_PTR", g.off_ptr); K("OFF_LIST", g.off_list); K("OFF_IMG", g.off_img); K("OFF_S", g.off_s); K("OFF_ST", g.off_st);
    K("OFF_GY", g.off_gy); K("LDS_BYTES", g.lds);
    s += "#line 1 \"molann_mlp_tile.inc\"\n";
    s += join_chunks(k_src_molann_mlp_tile_inc);
    s += "#line 1 \"molann_group_vjp.inc\"\n";
    s += join_chunks(k_src_molann_group_vjp_inc);
    return s;
}

std::string jit_preamble(const JitSpec& j) {
    std::string s = "// preamble generated from the plan\n";
    char b[256];
    auto K = [&](const char* name, int v) { snprintf(b, sizeof(b), "constexpr int %s = %d;\n", name, v); s += b; };
    K("N_INP", j.n_inp); K("N_ALIGN", j.n_align); K("N_SLOTS", (int)j.slots.size()); K("N_ITEMS", (int)j.items.size());
    K("NL", j.n_layers); K("ACT", j.act); K("D_FEAT", j.d_feat); K("OUT_COLS", j.out_cols); K("WPB", j.wpb);
    K("LDS_PER_WAVE", j.lds_per_wave); K("FBUF_OFF", j.fbuf_off);
    K("WAVES_PER_EU", j.waves_per_eu); K("NBUF", j.nbuf);
    K("NCONS", j.ncons); K("NLOAD", j.nload); K("LDS_BLOCK", j.lds_block); K("NSLOT", j.nslot); K("DEPTH", j.depth); K("RING_OFF", j.ring_off); K("TILE_STRIDE", j.tile_stride);
    K("FB_OFF", j.fb_off); K("FB_BYTES", j.fb_bytes);
    s += j.save_feat ? "constexpr bool SAVE_FEAT = true;\n" : "constexpr bool SAVE_FEAT = false;\n";
    s += j.with_values ? "constexpr bool WITH_VALUES = true;\n" : "constexpr bool WITH_VALUES = false;\n";
    s += j.wide_mlp ? "constexpr bool WIDE_MLP = true;\n" : "constexpr bool WIDE_MLP = false;\n";
    s += j.frag_lds ? "constexpr bool FRAG_LDS = true;\n" : "constexpr bool FRAG_LDS = false;\n";
    K("IMG_OFF", j.img_off);
    {   // waves per SIMD the forward kernel must fit (its register budget): every wave of the (NCONS + 1)-wave blocks
        // a CU is to hold - the loader waves carry the consumers' allocation
        const int waves = (j.ncons + j.nload) * std::max(1, j.bpc);
        K("WAVES_FWD", std::max(1, std::min(8, (waves + 3) / 4)));
    }
    {   // Opt-in, never used for a reported number: a plan whose items are all invariant under rigid motion produces the
        // same output with or without its alignment; MOLANN_ELIDE_INVARIANT_ALIGNMENT=1 (read at plan creation) drops
        // the (then dead) Kabsch from the specialised kernel.  Default: the alignment is computed, as the reference does.
        const char* e = diag_env("MOLANN_ELIDE_INVARIANT_ALIGNMENT");
        s += (e && e[0] == '1') ? "constexpr bool ELIDE_ALIGN = true;\n" : "constexpr bool ELIDE_ALIGN = false;\n";
    }
    {   // cache policy of the x stream's LDS-DMA: 2 = nt, the default (every frame is read once; round 3: C2 39.5 -> 36.5 us,
        // C3 66.4 -> 64.7 us per 1 M frames, tools/r03_ab.sh); experiments: 0 = default policy, 19 = sc0 sc1 nt
        const char* e = diag_env("MOLANN_DEBUG_DMA_AUX");
        K("DMA_AUX", e ? atoi(e) : 2);
    }
    {
        std::vector<int> win = j.win.empty() ? std::vector<int>(1, 0) : j.win;
        K("NWIN", (int)win.size());
        s += "constexpr int WIN_START[] = {";
        for (size_t i = 0; i < win.size(); ++i) { snprintf(b, sizeof(b), "%s%d", i ? ", " : "", win[i]); s += b; }
        s += "};\n";
    }
    s += (debug_env().ablate & 32) ? "constexpr bool STAMPS = true;\n" : "constexpr bool STAMPS = false;\n";
    // diagnostic (MOLANN_DEBUG_ABLATE bit 64): every wave stages its first tile only and recomputes it for all its
    // tiles - the kernel's compute time without the HBM stream
    s += (debug_env().ablate & 64) ? "constexpr bool NO_RESTAGE = true;\n" : "constexpr bool NO_RESTAGE = false;\n";
    // diagnostic (bit 128): the whole next tile's LDS-DMA right after the register fill instead of in slices
    s += (debug_env().ablate & 128) ? "constexpr bool DMA_EARLY = true;\n" : "constexpr bool DMA_EARLY = false;\n";
    // diagnostic (bit 256): every DMA re-reads the wave's first tile (L2-resident): the DMA mechanics without HBM
    s += (debug_env().ablate & 256) ? "constexpr bool SAME_TILE = true;\n" : "constexpr bool SAME_TILE = false;\n";
    // diagnostic (bit 512): the fused MLP's 16-byte output stores are (data-dependently) never executed
    s += (debug_env().ablate & 512) ? "constexpr bool NO_STORES = true;\n" : "constexpr bool NO_STORES = false;\n";
    // diagnostic (bit 2048): consumers hand every tile back as soon as it is in registers and compute nothing
    s += (debug_env().ablate & 2048) ? "constexpr bool NO_COMPUTE = true;\n" : "constexpr bool NO_COMPUTE = false;\n";
    { const char* e = diag_env("MOLANN_DEBUG_TILE_GROUP"); K("TILE_GROUP", e && atoi(e) > 0 ? atoi(e) : 1); } // adjacent tiles per block and turn (experiment)
    { const char* e = diag_env("MOLANN_DEBUG_STORE_GROUP"); K("STORE_GROUP", e && atoi(e) > 0 ? atoi(e) : 1); } // ... taken by ONE consumer, outputs stored as one burst (experiment; set TILE_GROUP to the same value; aligned 16-byte outputs only)
    { const char* e = diag_env("MOLANN_DEBUG_ST_POLICY"); K("ST_POLICY", e ? atoi(e) : 1); } // cache policy of the output stores (1 = nt)
    { const char* e = diag_env("MOLANN_DEBUG_SLEEP"); K("SLEEP_N", e ? atoi(e) : 0); }
    { const char* e = diag_env("MOLANN_DEBUG_SPIN"); K("SPIN_N", e ? atoi(e) : 0); }   // with NO_COMPUTE: 64 x N v_fma per tile // with NO_COMPUTE: idle ~8k cycles x N per tile
    auto A = [&](const char* name, const std::vector<int>& v) {
        s += std::string("constexpr int ") + name + "[] = {";
        for (size_t i = 0; i < v.size(); ++i) { snprintf(b, sizeof(b), "%s%d", i ? ", " : "", v[i]); s += b; }
        s += "};\n";
    };
    std::vector<int> used(j.slots.size(), 0), type, col;
    A("SLOT_ATOM", j.slots);
    s += "constexpr int ITEM_IDX[][4] = {";
    for (size_t i = 0; i < j.items.size(); ++i) {
        const ItemDev& it = j.items[i];
        const int na = item_atoms(it.type);
        for (int k = 0; k < na; ++k) used[it.idx[k]] = 1;
        type.push_back(it.type);
        col.push_back(it.col);
        snprintf(b, sizeof(b), "%s{%d, %d, %d, %d}", i ? ", " : "", it.idx[0], it.idx[1], it.idx[2], it.idx[3]);
        s += b;
    }
    s += "};\n";
    A("ITEM_TYPE", type); A("ITEM_COL", col); A("SLOT_USED", used);
    std::vector<int> dims = j.dims;
    if (dims.empty()) dims.push_back(j.d_feat);
    while (dims.size() < 2) dims.push_back(1); // the kernel text names DIMS[1] even when NL == 0 discards its use
    A("DIMS", dims);
    return s;
}

// compile to a gfx950 code object; returns 0 or a hiprtcResult, log filled on failure
int jit_compile(const std::string& src, std::vector<char>& code, std::string& log, const char* more_flags = nullptr) {
    const RtcApi* rtc = rtc_api();
    if (!rtc->ok) { log = "libhiprtc.so not found"; return -1; }
    const std::string math = join_chunks(k_src_molann_math_h);
    const char* hdr_src[] = {math.c_str()};
    const char* hdr_name[] = {"molann_math.h"};
    hiprtcProgram prog;
    hiprtcResult r = rtc->create(&prog, src.c_str(), "molann_lane_jit.hip", 1, hdr_src, hdr_name);
    if (r != HIPRTC_SUCCESS) { log = "hiprtcCreateProgram failed"; return (int)r; }
    std::vector<std::string> flags = {"--offload-arch=gfx950", "-O3", "-std=c++17"};
    if (more_flags && more_flags[0]) flags.push_back(more_flags);
    if (const char* extra = diag_env("MOLANN_JIT_EXTRA_FLAGS")) { // experiments: space-separated compiler flags
        std::string e(extra);
        size_t pos = 0;
        while (pos < e.size()) {
            const size_t sp = e.find(' ', pos);
            const std::string tok = e.substr(pos, sp == std::string::npos ? std::string::npos : sp - pos);
            if (!tok.empty()) flags.push_back(tok);
            if (sp == std::string::npos) break;
            pos = sp + 1;
        }
    }
    std::vector<const char*> opts;
    for (auto& f : flags) opts.push_back(f.c_str());
    // MOLANN_JIT_CACHE_DIR=<dir>: code objects kept on disk under a hash of everything they are made from (kernel text,
    // molann_math.h, flags, the hipRTC and HIP runtime versions), so a process that builds a plan another one has built
    // skips the compile (1.5-4 s per kernel).  Opt-in.  A cached file is [magic, format, blob length, FNV-1a of the blob]
    // + blob: anything that does not verify is deleted and rebuilt.  What is loaded from there runs on the GPU, so the
    // directory must belong to this user and be writable by nobody else - otherwise it is not used at all.
    std::string cache_file;
    auto fnv = [](const void* data, size_t n, unsigned long long h = 1469598103934665603ull) {
        const unsigned char* c = (const unsigned char*)data;
        for (size_t i = 0; i < n; ++i) { h ^= c[i]; h *= 1099511628211ull; }
        return h;
    };
    struct CacheHeader { char magic[8]; unsigned long long format, length, hash; };
    if (const char* dir = getenv("MOLANN_JIT_CACHE_DIR")) {
        struct stat st;
        const bool dir_ok = dir[0] && stat(dir, &st) == 0 && S_ISDIR(st.st_mode) && st.st_uid == geteuid() && (st.st_mode & (S_IWGRP | S_IWOTH)) == 0;
        if (dir[0] && !dir_ok && getenv("MOLANN_JIT_VERBOSE"))
            fprintf(stderr, "molann: MOLANN_JIT_CACHE_DIR=%s ignored (not a directory of this user, or writable by group / others)\n", dir);
        if (dir_ok) {
            unsigned long long h = 1469598103934665603ull;   // FNV-1a, 64 bit
            auto mix = [&](const std::string& t) { h = fnv(t.data(), t.size(), h); h ^= 0xff; h *= 1099511628211ull; };
            mix(src); mix(math);
            for (auto& f : flags) mix(f);
            int maj = 0, min = 0, rt = 0;
            if (rtc->version) (void)rtc->version(&maj, &min);
            (void)hipRuntimeGetVersion(&rt);
            char name[128];
            snprintf(name, sizeof(name), "/molann_%016llx_%zu_rtc%d.%d_hip%d.hsaco", h, src.size(), maj, min, rt);
            cache_file = std::string(dir) + name;
            if (FILE* f = fopen(cache_file.c_str(), "rb")) {
                std::vector<char> blob;
                char buf[1 << 16];
                size_t got;
                while ((got = fread(buf, 1, sizeof(buf), f)) > 0) blob.insert(blob.end(), buf, buf + got);
                fclose(f);
                CacheHeader hd;
                bool good = blob.size() > sizeof(hd) + 64;
                if (good) {
                    memcpy(&hd, blob.data(), sizeof(hd));
                    good = memcmp(hd.magic, "MOLANNCO", 8) == 0 && hd.format == 1 && hd.length == blob.size() - sizeof(hd) &&
                           memcmp(blob.data() + sizeof(hd), "\177ELF", 4) == 0 && hd.hash == fnv(blob.data() + sizeof(hd), blob.size() - sizeof(hd));
                }
                if (good) {
                    code.assign(blob.begin() + sizeof(hd), blob.end());
                    rtc->destroy(&prog);
                    return 0;
                }
                (void)remove(cache_file.c_str());   // truncated, corrupt or foreign: rebuilt below
            }
        }
    }
    r = rtc->compile(prog, (int)opts.size(), opts.data());
    size_t ls = 0;
    rtc->log_size(prog, &ls);
    if (ls > 1) { log.resize(ls); rtc->log(prog, &log[0]); }
    if (r == HIPRTC_SUCCESS) {
        size_t cs = 0;
        rtc->code_size(prog, &cs);
        code.resize(cs);
        rtc->code(prog, code.data());
        if (!cache_file.empty()) { // written under a temporary name and renamed: a reader never sees half a file
            const std::string tmp = cache_file + ".tmp" + std::to_string((long)getpid());
            if (FILE* f = fopen(tmp.c_str(), "wb")) {
                CacheHeader hd;
                memcpy(hd.magic, "MOLANNCO", 8);
                hd.format = 1; hd.length = code.size(); hd.hash = fnv(code.data(), code.size());
                const bool ok = fwrite(&hd, 1, sizeof(hd), f) == sizeof(hd) && fwrite(code.data(), 1, code.size(), f) == code.size();
                fclose(f);
                if (!ok || rename(tmp.c_str(), cache_file.c_str()) != 0) (void)remove(tmp.c_str());
            }
        }
    }
    rtc->destroy(&prog);
    return (int)r;
}

// One specialised kernel, ready to launch: compiled (or read from the code-object cache), loaded, its entry point resolved and its
// scratch bytes asked for (-1: the runtime does not say).  false: nothing stays loaded, rc is the compiler's (0 when the code
// object did not load), and MOLANN_JIT_VERBOSE prints what failed with the build log.  Which build a caller keeps is its own policy.
struct BuiltKernel {
    hipModule_t mod = nullptr;
    hipFunction_t fn = nullptr;
    int scratch = -1, rc = -1;
    size_t bytes = 0;      // of the code object
    void unload() { if (mod) (void)hipModuleUnload(mod); mod = nullptr; fn = nullptr; }
};
bool build_kernel(const std::string& src, const char* entry, const char* flags, const char* what, BuiltKernel& k) {
    std::vector<char> code;
    std::string log;
    k.rc = jit_compile(src, code, log, flags);
    k.bytes = code.size();
    if (k.rc == 0 && hipModuleLoadData(&k.mod, code.data()) == hipSuccess && hipModuleGetFunction(&k.fn, k.mod, entry) == hipSuccess) {
        if (hipFuncGetAttribute(&k.scratch, HIP_FUNC_ATTRIBUTE_LOCAL_SIZE_BYTES, k.fn) != hipSuccess) k.scratch = -1;
        return true;
    }
    k.unload();
    if (getenv("MOLANN_JIT_VERBOSE")) fprintf(stderr, "molann %s failed rc=%d\n%s\n", what, k.rc, log.c_str());
    return false;
}

} // namespace
