// molann_torch.cpp - the plans of libmolann_hip.so as TorchScript operators.
//
// The reference's own tests end every case with torch.jit.script(module).save(...) (test/test_molann.py:36,
// 46,62,75,101,114) and README.rst:49 ships models to MD engines that way.  A scripted module cannot call
// ctypes, so the same C ABI (include/molann_hip.h) is bound here a second time, as dispatcher operators a
// TorchScript graph can name:
//
//     molann::run(Tensor x, int[] desc, Tensor ref_x, Tensor[] weights, Tensor[] biases) -> Tensor
//     molann::run_backward(Tensor x, int[] desc, Tensor ref_x, Tensor[] weights, Tensor[] biases,
//                          Tensor grad_out, bool need_x, bool need_params) -> Tensor[]
//
// `desc` is everything the modules fix at construction time, as integers (layout below; written by
// molann_amd/script.py).  Plans are created on first use and cached per (desc, device); desc carries an
// instance id, so two models of the same architecture have plans (packed weights, workspaces) of their own.
// The live tensors (ref_x buffer, Linear parameters) are re-read whenever one of them is a different tensor
// OBJECT than the one packed last (identity through a weak reference to its TensorImpl: an address the
// allocator hands out again after a model was freed cannot pass for the old tensor), or its storage or version
// counter changed.  The one edit this cannot see is an in-place write through `.data` / under a detached alias
// (it bumps the alias's counter): molann::invalidate(desc, device) - `model.refresh_parameters()` in Python -
// or MOLANN_ALWAYS_REPACK=1 covers that.  Entries are evicted least-recently-used beyond
// MOLANN_PLAN_CACHE_SIZE (default 64) and by molann::release / molann::drop_plans.
// Only the HIP dispatch key is registered: a CPU tensor raises, there is no fallback.
// A libtorch host loads this library (dlopen / torch.ops.load_library) before torch::jit::load.
//
// desc: [0]=2 (layout version) [1]=kind (0 align, 1 features, 2 features+MLP) [2]=n_inp [3]=n_align
//       [4]=n_features [5]=use_angle_value [6]=n_layers [7]=activation [8]=mlp_precision [9]=instance id, then
//       align_idx[n_align], feat_type[n_features], feat_ptr[n_features+1], feat_idx[feat_ptr[n_features]],
//       layer_dims[n_layers+1] (only when n_layers > 0)

#include <torch/library.h>
#include <torch/csrc/autograd/custom_function.h>
#include <torch/csrc/autograd/autograd.h>
#include <ATen/ATen.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>

#include <cmath>
#include <cstdlib>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "molann_hip.h"

namespace {

enum { KIND_ALIGN = 0, KIND_FEATURES = 1, KIND_FORWARD = 2, DESC_LAYOUT = 2, DESC_HEAD = 10 };

// What was packed: the tensor OBJECT (a weak reference keeps the TensorImpl's address from being reused while we
// remember it, and says when the tensor is gone), its storage address and its version counter.
struct TensorKey {
    c10::weak_intrusive_ptr<c10::TensorImpl> impl{c10::weak_intrusive_ptr<c10::TensorImpl>(
        c10::intrusive_ptr<c10::TensorImpl, c10::UndefinedTensorImpl>())};
    const void* ptr = nullptr;
    int64_t version = -1;
    bool matches(const at::Tensor& t) const {
        return version >= 0 && !impl.expired() && impl._unsafe_get_target() == t.unsafeGetTensorImpl() && ptr == t.data_ptr() &&
               version == (int64_t)t._version();
    }
};

TensorKey key_of(const at::Tensor& t) {
    TensorKey k;
    k.impl = c10::weak_intrusive_ptr<c10::TensorImpl>(t.getIntrusivePtr());
    k.ptr = t.data_ptr();
    k.version = (int64_t)t._version();
    return k;
}

struct Entry {
    molann_plan* plan = nullptr;
    int kind = 0, n_inp = 0, n_align = 0, n_layers = 0, out_dim = 0, feature_dim = 0;
    TensorKey ref_key;
    std::vector<TensorKey> mlp_key;
    bool dirty = false; // molann::invalidate: repack at the next call whatever the keys say
    uint64_t last_use = 0;
    int pins = 0;  // captured HIP graphs that launch through this plan (molann::pin): never evicted while > 0 (guarded by g_cache_mu)
    std::mutex mu; // update_* + launch of one plan are one critical section
    ~Entry() {
        if (plan) molann_plan_destroy(plan);
    }
};

void check(int rc, const char* what) {
    TORCH_CHECK(rc == 0, what, " failed: ", molann_error_string(rc), " (", rc, ")");
}

struct Parsed {
    std::vector<int32_t> align_idx, feat_type, feat_ptr, feat_idx, layer_dims;
    molann_plan_desc d;
};

// the integer list -> molann_plan_desc (pointers into `p`)
void parse_desc(const std::vector<int64_t>& v, Parsed& p) {
    TORCH_CHECK(v.size() >= DESC_HEAD && v[0] == DESC_LAYOUT, "molann::run: unknown descriptor layout");
    const int64_t n_align = v[3], n_feat = v[4], n_layers = v[6];
    TORCH_CHECK(n_align >= 0 && n_feat >= 0 && n_layers >= 0 && n_layers <= MOLANN_MAX_LAYERS, "molann::run: bad descriptor counts");
    size_t pos = DESC_HEAD;
    auto take = [&](std::vector<int32_t>& out, int64_t n) {
        TORCH_CHECK(pos + (size_t)n <= v.size(), "molann::run: descriptor too short");
        out.assign(v.begin() + pos, v.begin() + pos + n);
        pos += (size_t)n;
    };
    take(p.align_idx, n_align);
    take(p.feat_type, n_feat);
    take(p.feat_ptr, n_feat > 0 ? n_feat + 1 : 0);
    take(p.feat_idx, n_feat > 0 ? p.feat_ptr.back() : 0);
    take(p.layer_dims, n_layers > 0 ? n_layers + 1 : 0);
    TORCH_CHECK(pos == v.size(), "molann::run: descriptor has trailing entries");
    molann_plan_desc& d = p.d;
    d = molann_plan_desc();
    d.abi_version = MOLANN_ABI_VERSION;
    d.n_inp = (int32_t)v[2];
    d.n_align = (int32_t)n_align;
    d.align_idx = p.align_idx.data();
    d.n_features = (int32_t)n_feat;
    d.feat_type = p.feat_type.data();
    d.feat_ptr = p.feat_ptr.data();
    d.feat_idx = p.feat_idx.data();
    d.use_angle_value = (int32_t)v[5];
    d.n_layers = (int32_t)n_layers;
    d.layer_dims = p.layer_dims.data();
    d.activation = (int32_t)v[7];
    d.mlp_precision = (int32_t)v[8];
}

typedef std::pair<std::vector<int64_t>, int> CacheKey;
std::mutex g_cache_mu;
std::map<CacheKey, std::shared_ptr<Entry>> g_cache;
uint64_t g_clock = 0;

size_t cache_capacity() {
    static const size_t cap = [] {
        const char* e = getenv("MOLANN_PLAN_CACHE_SIZE");
        const long v = e ? atol(e) : 64;
        return (size_t)(v < 1 ? 1 : v);
    }();
    return cap;
}

bool always_repack() {
    static const bool v = [] { const char* e = getenv("MOLANN_ALWAYS_REPACK"); return e && e[0] == '1'; }();
    return v;
}

// caller holds g_cache_mu.  An evicted entry that a running call still holds lives until that call returns
// (shared_ptr); its plan and device memory go with the last reference.
// Entries pinned by a captured graph are not candidates: a graph replay never passes through entry_for (its
// last_use does not move) and holds raw pointers into the plan's device memory and code objects.
void evict_lru_locked() {
    while (g_cache.size() > cache_capacity()) {
        auto victim = g_cache.end();
        for (auto it = g_cache.begin(); it != g_cache.end(); ++it)
            if (it->second->pins == 0 && (victim == g_cache.end() || it->second->last_use < victim->second->last_use)) victim = it;
        if (victim == g_cache.end()) return;   // everything left is pinned
        g_cache.erase(victim);
    }
}

// molann_plan_create reads two switches from the environment (MOLANN_NO_JIT, MOLANN_NO_REGS: which kernel
// family serves the plan); a plan built under other settings must not be handed out, so they are part of the key
int cache_device_key(int device) {
    const char* a = getenv("MOLANN_NO_JIT");
    const char* b = getenv("MOLANN_NO_REGS");
    return device | ((a && a[0] == '1') ? 1 << 16 : 0) | ((b && b[0] == '1') ? 1 << 17 : 0);
}

// plan for (desc, device of x); created with the current contents of ref_x
std::shared_ptr<Entry> entry_for(const std::vector<int64_t>& desc, const at::Tensor& x, const at::Tensor& ref_x) {
    const auto key = std::make_pair(desc, cache_device_key((int)x.get_device()));
    std::lock_guard<std::mutex> lock(g_cache_mu);
    auto it = g_cache.find(key);
    if (it != g_cache.end()) {
        it->second->last_use = ++g_clock;
        return it->second;
    }
    Parsed p;
    parse_desc(desc, p);
    at::Tensor ref_host;
    if (p.d.n_align > 0) {
        TORCH_CHECK(ref_x.numel() == 3 * (int64_t)p.d.n_align, "molann::run: ref_x must be [n_align, 3]");
        ref_host = ref_x.detach().to(at::kCPU, at::kFloat).contiguous();
        p.d.ref_x = ref_host.data_ptr<float>();
    }
    auto e = std::make_shared<Entry>();
    check(molann_plan_create(&p.d, &e->plan), "molann_plan_create");
    e->kind = (int)desc[1];
    e->n_inp = p.d.n_inp;
    e->n_align = p.d.n_align;
    e->n_layers = p.d.n_layers;
    e->out_dim = molann_plan_out_dim(e->plan);
    e->feature_dim = molann_plan_feature_dim(e->plan);
    e->last_use = ++g_clock;
    g_cache.emplace(key, e);
    evict_lru_locked();
    return e;
}

// AlignmentLayer on its own has no backward kernel; the same map written as alignment + one position item
// per atom does (molann_amd/ann.py does the same)
std::vector<int64_t> align_as_features(const std::vector<int64_t>& desc) {
    const int64_t n_inp = desc[2], n_align = desc[3];
    std::vector<int64_t> v(desc.begin(), desc.begin() + DESC_HEAD + n_align);
    v[1] = KIND_FEATURES;
    v[4] = 1; // one position feature over all atoms
    v.push_back(MOLANN_FEAT_POSITION);
    v.push_back(0);
    v.push_back(n_inp);
    for (int64_t i = 0; i < n_inp; ++i) v.push_back(i);
    return v;
}

at::Tensor device_f32(const at::Tensor& t, const at::Tensor& like, const char* name) {
    TORCH_CHECK(t.scalar_type() == at::kFloat, "molann::run: ", name, " must be float32, got ", t.scalar_type());
    TORCH_CHECK(t.device() == like.device(), "molann::run: ", name, " is on ", t.device(), " but x is on ", like.device());
    return t.contiguous();
}

// bring the plan's copies of the live tensors up to date (caller holds e.mu, device guard set)
void sync_live(Entry& e, const at::Tensor& x, const at::Tensor& ref_x, const std::vector<at::Tensor>& weights,
               const std::vector<at::Tensor>& biases, hipStream_t stream) {
    if (e.n_align > 0) {
        TORCH_CHECK(ref_x.scalar_type() == x.scalar_type(), "molann::run: expected ref_x and x to have the same dtype, but got ",
                    ref_x.scalar_type(), " and ", x.scalar_type());
        TORCH_CHECK(ref_x.device() == x.device(), "molann::run: ref_x is on ", ref_x.device(), " but x is on ", x.device());
        if (e.dirty || always_repack() || !e.ref_key.matches(ref_x)) {
            const at::Tensor r = ref_x.detach().contiguous();
            if (r.scalar_type() == at::kDouble) check(molann_plan_update_ref_f64(e.plan, r.data_ptr<double>(), stream), "molann_plan_update_ref_f64");
            else check(molann_plan_update_ref(e.plan, r.data_ptr<float>(), stream), "molann_plan_update_ref");
            e.ref_key = key_of(ref_x);
        }
    }
    if (x.scalar_type() == at::kDouble) { e.dirty = false; return; }   // float64: the Linear parameters are read as they are
    if (e.kind == KIND_FORWARD) {
        TORCH_CHECK((int)weights.size() == e.n_layers && (int)biases.size() == e.n_layers,
                    "molann::run: expected ", e.n_layers, " weight and bias tensors");
        bool changed = e.dirty || always_repack() || e.mlp_key.size() != 2 * (size_t)e.n_layers;
        for (int l = 0; !changed && l < e.n_layers; ++l)
            changed = !e.mlp_key[2 * l].matches(weights[l]) || !e.mlp_key[2 * l + 1].matches(biases[l]);
        if (changed) {
            std::vector<at::Tensor> hold;
            std::vector<const float*> W, B;
            for (int l = 0; l < e.n_layers; ++l) {
                hold.push_back(device_f32(weights[l].detach(), x, "weight"));
                W.push_back(hold.back().data_ptr<float>());
                hold.push_back(device_f32(biases[l].detach(), x, "bias"));
                B.push_back(hold.back().data_ptr<float>());
            }
            check(molann_plan_update_mlp(e.plan, W.data(), B.data(), stream), "molann_plan_update_mlp");
            e.mlp_key.clear();
            for (int l = 0; l < e.n_layers; ++l) { e.mlp_key.push_back(key_of(weights[l])); e.mlp_key.push_back(key_of(biases[l])); }
        }
    }
    e.dirty = false;
}

void check_x(const at::Tensor& x, const std::vector<int64_t>& desc) {
    TORCH_CHECK(desc.size() >= DESC_HEAD, "molann::run: bad descriptor");
    TORCH_CHECK(x.dim() == 3 && x.size(1) == desc[2] && x.size(2) == 3, "Input should be a 3d torch tensor, with sizes [*, ",
                desc[2], ", 3]. Actual sizes: ", x.sizes());
    TORCH_CHECK(x.scalar_type() == at::kFloat || x.scalar_type() == at::kDouble, "molann_amd kernels are float32 / float64; got ",
                x.scalar_type());
}

at::Tensor run_impl(const at::Tensor& x_in, const std::vector<int64_t>& desc, const at::Tensor& ref_x, const std::vector<at::Tensor>& weights,
                    const std::vector<at::Tensor>& biases);
// A description registered once (molann::register_desc) and named by a small integer afterwards: what the eager modules'
// inference calls use - converting the 30-odd integers of a description from a Python list at every call costs more
// than the launch's own bookkeeping.  Scripted modules keep the self-contained list form (molann::run).
std::mutex g_handle_mu;
std::vector<std::shared_ptr<const std::vector<int64_t>>> g_handles;

int64_t register_desc(std::vector<int64_t> desc) {
    TORCH_CHECK(desc.size() >= DESC_HEAD && desc[0] == DESC_LAYOUT, "molann::register_desc: unknown descriptor layout");
    std::lock_guard<std::mutex> lock(g_handle_mu);
    for (size_t i = 0; i < g_handles.size(); ++i)
        if (*g_handles[i] == desc) return (int64_t)i;
    g_handles.push_back(std::make_shared<const std::vector<int64_t>>(std::move(desc)));
    return (int64_t)g_handles.size() - 1;
}

// the description behind a handle (shared: a later register_desc may move the list)
std::shared_ptr<const std::vector<int64_t>> desc_of(int64_t handle, const char* op) {
    std::lock_guard<std::mutex> lock(g_handle_mu);
    TORCH_CHECK(handle >= 0 && (size_t)handle < g_handles.size(), op, ": unknown handle ", handle);
    return g_handles[(size_t)handle];
}

// The float64 Linear tensors of a forward plan as the float64 entry points take them, read as they are: `hold` keeps the contiguous
// tensors alive, W / B point into them.  Nothing for a plan without a head.
struct F64Linears {
    std::vector<at::Tensor> hold;
    std::vector<const double*> W, B;
};
void f64_linears(const char* op, const Entry& e, const at::Tensor& x, const std::vector<at::Tensor>& weights, const std::vector<at::Tensor>& biases,
                 F64Linears& lin, const char* hint = "") {
    if (e.kind != KIND_FORWARD) return;
    TORCH_CHECK((int)weights.size() == e.n_layers && (int)biases.size() == e.n_layers, op, ": expected ", e.n_layers, " weight and bias tensors");
    for (int l = 0; l < e.n_layers; ++l) {
        TORCH_CHECK(weights[l].scalar_type() == at::kDouble && biases[l].scalar_type() == at::kDouble && weights[l].device() == x.device() &&
                        biases[l].device() == x.device(),
                    op, ": ann_layers must be float64 on ", x.device(), " for a float64 input", hint);
        lin.hold.push_back(weights[l].detach().contiguous()); lin.W.push_back(lin.hold.back().data_ptr<double>());
        lin.hold.push_back(biases[l].detach().contiguous()); lin.B.push_back(lin.hold.back().data_ptr<double>());
    }
}

// The two outputs of a one-launch operator: the caller's `into` pair - x's dtype, contiguous, the element counts of the two shapes, on
// x's device - or fresh tensors of those shapes.  `names` ("(out, jac)") makes the refusals typed: any count but 0 and 2 is refused,
// a wrong dtype is a TypeError, the rest a ValueError.  Without it (value_and_vjp, which predates them) every fault is a plain Error
// and any other count means none.
std::pair<at::Tensor, at::Tensor> into_pair(const char* op, const std::vector<at::Tensor>& into, const at::Tensor& x, at::IntArrayRef shape0,
                                            at::IntArrayRef shape1, const char* names, const char* shapes) {
    if (names) TORCH_CHECK(into.empty() || into.size() == 2, op, ": `into` must be a pair of tensors ", names);
    if (into.size() != 2) return {at::empty(shape0, x.options()), at::empty(shape1, x.options())};
    const at::Tensor &a = into[0], &b = into[1];
    const bool dtype = a.scalar_type() == x.scalar_type() && b.scalar_type() == x.scalar_type();
    const bool rest = a.is_contiguous() && b.is_contiguous() && a.numel() == c10::multiply_integers(shape0) &&
                      b.numel() == c10::multiply_integers(shape1) && a.device() == x.device() && b.device() == x.device();
    if (names) {
        TORCH_CHECK_TYPE(dtype, op, ": `into` must be float64 like x");
        TORCH_CHECK_VALUE(rest, op, ": `into` must be contiguous ", shapes, " on x's device");
    } else
        TORCH_CHECK(dtype && rest, op, ": `into` must be contiguous ", shapes, " on x's device");
    return {a, b};
}

at::Tensor run_h_hip(const at::Tensor& x, int64_t handle, const at::Tensor& ref_x, std::vector<at::Tensor> weights, std::vector<at::Tensor> biases) {
    return run_impl(x, *desc_of(handle, "molann::run_h"), ref_x, weights, biases);
}

at::Tensor run_hip(const at::Tensor& x_in, std::vector<int64_t> desc, const at::Tensor& ref_x, std::vector<at::Tensor> weights,
                   std::vector<at::Tensor> biases) {
    return run_impl(x_in, desc, ref_x, weights, biases);
}
at::Tensor run_impl(const at::Tensor& x_in, const std::vector<int64_t>& desc, const at::Tensor& ref_x, const std::vector<at::Tensor>& weights,
                    const std::vector<at::Tensor>& biases) {
    check_x(x_in, desc);
    const at::Tensor x = x_in.contiguous();
    const c10::DeviceGuard guard(x.device());
    auto e = entry_for(desc, x, ref_x);
    const int64_t n = x.size(0);
    at::Tensor out = e->kind == KIND_ALIGN ? at::empty_like(x)
                                           : at::empty({n, e->kind == KIND_FORWARD ? e->out_dim : e->feature_dim}, x.options());
    if (n == 0) return out;
    hipStream_t stream = c10::hip::getCurrentHIPStream(x.get_device()).stream();
    std::lock_guard<std::mutex> lock(e->mu);
    sync_live(*e, x, ref_x, weights, biases, stream);
    if (x.scalar_type() == at::kDouble) { // `model.double()(x.double())`: the float64 entry points
        const double* xd = x.data_ptr<double>();
        double* od = out.data_ptr<double>();
        if (e->kind == KIND_ALIGN) check(molann_align_f64(e->plan, xd, n, od, stream), "molann_align_f64");
        else if (e->kind == KIND_FEATURES) check(molann_features_f64(e->plan, xd, n, od, stream), "molann_features_f64");
        else {
            F64Linears lin;
            f64_linears("molann::run", *e, x, weights, biases, lin);
            at::Tensor work = at::empty({n, e->feature_dim}, x.options());
            check(molann_forward_f64(e->plan, xd, n, lin.W.data(), lin.B.data(), work.data_ptr<double>(), od, stream), "molann_forward_f64");
        }
        return out;
    }
    const float* xp = x.data_ptr<float>();
    float* op = out.data_ptr<float>();
    if (e->kind == KIND_ALIGN) check(molann_align_f32(e->plan, xp, n, op, stream), "molann_align_f32");
    else if (e->kind == KIND_FEATURES) check(molann_features_f32(e->plan, xp, n, op, stream), "molann_features_f32");
    else check(molann_forward_packed_f32(e->plan, xp, n, op, stream), "molann_forward_packed_f32");
    return out;
}

// [grad_x or empty, flat parameter gradients (dW_l, db_l per layer) or empty]
std::vector<at::Tensor> run_backward_hip(const at::Tensor& x_in, std::vector<int64_t> desc, const at::Tensor& ref_x,
                                         std::vector<at::Tensor> weights, std::vector<at::Tensor> biases,
                                         const at::Tensor& grad_out, bool need_x, bool need_params) {
    check_x(x_in, desc);
    const at::Tensor x = x_in.contiguous();
    const c10::DeviceGuard guard(x.device());
    const bool align_only = desc[1] == KIND_ALIGN;
    auto e = entry_for(align_only ? align_as_features(desc) : desc, x, ref_x);
    TORCH_CHECK(x.scalar_type() == at::kDouble || molann_plan_supports_backward(e->plan) == 1,
                "no backward kernel for this plan (wide MLP / large frames / this activation): run it under torch.no_grad()");
    const int64_t n = x.size(0);
    const int64_t cols = e->kind == KIND_FORWARD ? e->out_dim : e->feature_dim;
    if (x.scalar_type() == at::kDouble) { // float64: the features' backward in double (the MLP of a float64 model is ATen's)
        TORCH_CHECK(e->kind != KIND_FORWARD && !need_params, "molann::run_backward: float64 gradients exist for the preprocessing only");
        at::Tensor g = grad_out.to(at::kDouble).reshape({n, cols}).contiguous();
        at::Tensor gx = need_x ? at::empty_like(x) : at::empty({0}, x.options());
        if (n == 0 || !need_x) return {gx, at::empty({0}, x.options())};
        hipStream_t stream = c10::hip::getCurrentHIPStream(x.get_device()).stream();
        std::lock_guard<std::mutex> lock(e->mu);
        sync_live(*e, x, ref_x, weights, biases, stream);
        check(molann_features_backward_f64(e->plan, x.data_ptr<double>(), g.data_ptr<double>(), n, gx.data_ptr<double>(), stream),
              "molann_features_backward_f64");
        return {gx, at::empty({0}, x.options())};
    }
    at::Tensor g = grad_out.to(at::kFloat).reshape({n, cols}).contiguous();
    at::Tensor gx = need_x ? at::empty_like(x) : at::empty({0}, x.options());
    at::Tensor gp = need_params ? at::zeros({molann_plan_grad_params_size(e->plan)}, x.options()) : at::empty({0}, x.options());
    if (n == 0) {
        if (need_x) gx.zero_();
        return {gx, gp};
    }
    hipStream_t stream = c10::hip::getCurrentHIPStream(x.get_device()).stream();
    std::lock_guard<std::mutex> lock(e->mu);
    sync_live(*e, x, ref_x, weights, biases, stream);
    check(molann_backward_f32(e->plan, x.data_ptr<float>(), g.data_ptr<float>(), n, need_x ? gx.data_ptr<float>() : nullptr,
                              need_params ? gp.data_ptr<float>() : nullptr, stream),
          "molann_backward_f32");
    return {gx, gp};
}

// {out, grad_x}: the forward's outputs and the vector-Jacobian product for grad_out in ONE launch (molann_value_and_vjp_f32: the
// one-pass backward that also stores the outputs; a float64 x: molann_value_and_vjp_f64 on the float64 Linear tensors).
// Parameters are data.  `into` (optional: {out, grad_x} of the right shapes) is written instead of fresh tensors - a caller at every MD step keeps its two buffers.
std::vector<at::Tensor> value_and_vjp_impl(const at::Tensor& x_in, const std::vector<int64_t>& desc, const at::Tensor& ref_x, const std::vector<at::Tensor>& weights,
                                           const std::vector<at::Tensor>& biases, const at::Tensor& grad_out, const std::vector<at::Tensor>& into);
std::vector<at::Tensor> value_and_vjp_hip(const at::Tensor& x_in, std::vector<int64_t> desc, const at::Tensor& ref_x, std::vector<at::Tensor> weights,
                                          std::vector<at::Tensor> biases, const at::Tensor& grad_out, std::vector<at::Tensor> into) {
    return value_and_vjp_impl(x_in, desc, ref_x, weights, biases, grad_out, into);
}
std::vector<at::Tensor> value_and_vjp_h_hip(const at::Tensor& x_in, int64_t handle, const at::Tensor& ref_x, std::vector<at::Tensor> weights,
                                            std::vector<at::Tensor> biases, const at::Tensor& grad_out, std::vector<at::Tensor> into) {
    return value_and_vjp_impl(x_in, *desc_of(handle, "molann::value_and_vjp_h"), ref_x, weights, biases, grad_out, into);
}
std::vector<at::Tensor> value_and_vjp_impl(const at::Tensor& x_in, const std::vector<int64_t>& desc, const at::Tensor& ref_x, const std::vector<at::Tensor>& weights,
                                           const std::vector<at::Tensor>& biases, const at::Tensor& grad_out, const std::vector<at::Tensor>& into) {
    check_x(x_in, desc);
    const bool f64 = x_in.scalar_type() == at::kDouble;   // `model.double()`: molann_value_and_vjp_f64, the Linear tensors read as they are
    const at::ScalarType st = x_in.scalar_type();
    const at::Tensor x = x_in.contiguous();
    const c10::DeviceGuard guard(x.device());
    const bool align_only = desc[1] == KIND_ALIGN;
    auto e = entry_for(align_only ? align_as_features(desc) : desc, x, ref_x);
    const int64_t n = x.size(0);
    const int64_t cols = e->kind == KIND_FORWARD ? e->out_dim : e->feature_dim;
    at::Tensor g = grad_out.scalar_type() == st && grad_out.is_contiguous() ? grad_out : grad_out.to(st).contiguous();
    TORCH_CHECK(g.numel() == n * cols && g.device() == x.device(), "molann::value_and_vjp: grad_out must be [", n, ", ", cols, "] on ", x.device());
    const auto [out, gx] = into_pair("molann::value_and_vjp", into, x, {n, cols}, x.sizes(), nullptr,
                                     f64 ? "float64 {[N, out_dim], [N, n_inp, 3]}" : "float32 {[N, out_dim], [N, n_inp, 3]}");
    F64Linears lin;
    if (f64) f64_linears("molann::value_and_vjp", *e, x, weights, biases, lin);
    if (n == 0) return {out, gx};
    hipStream_t stream = c10::hip::getCurrentHIPStream(x.get_device()).stream();
    std::lock_guard<std::mutex> lock(e->mu);
    sync_live(*e, x, ref_x, weights, biases, stream);
    if (f64) {
        check(molann_value_and_vjp_f64(e->plan, x.data_ptr<double>(), g.data_ptr<double>(), n, lin.W.data(), lin.B.data(), out.data_ptr<double>(),
                                       gx.data_ptr<double>(), stream),
              "molann_value_and_vjp_f64");
        return {out, gx};
    }
    check(molann_value_and_vjp_f32(e->plan, x.data_ptr<float>(), g.data_ptr<float>(), n, out.data_ptr<float>(), gx.data_ptr<float>(), stream),
          "molann_value_and_vjp_f32");
    return {out, gx};
}

// {out, jac}: the float64 forward's outputs and the full Jacobian jac[N, out_dim, n_inp, 3] = d out / d x in ONE launch
// (molann_value_and_jacobian_f64 on the float64 Linear tensors).  Parameters are data.  `into` as value_and_vjp's: {out, jac}.
std::vector<at::Tensor> value_and_jacobian_impl(const at::Tensor& x_in, const std::vector<int64_t>& desc, const at::Tensor& ref_x,
                                                const std::vector<at::Tensor>& weights, const std::vector<at::Tensor>& biases,
                                                const std::vector<at::Tensor>& into) {
    check_x(x_in, desc);
    TORCH_CHECK_TYPE(x_in.scalar_type() == at::kDouble, "molann::value_and_jacobian is float64: call model.double() and pass a float64 x (got ",
                     x_in.scalar_type(), ")");
    TORCH_CHECK(desc[1] == KIND_FORWARD || desc[1] == KIND_FEATURES, "molann::value_and_jacobian: a forward or a features description");
    const at::Tensor x = x_in.contiguous();
    const c10::DeviceGuard guard(x.device());
    auto e = entry_for(desc, x, ref_x);
    const int64_t n = x.size(0);
    const int64_t cols = e->kind == KIND_FORWARD ? e->out_dim : e->feature_dim;
    const auto [out, jac] = into_pair("molann::value_and_jacobian", into, x, {n, cols}, {n, cols, x.size(1), 3}, "(out, jac)",
                                      "{[N, out_dim], [N, out_dim, n_inp, 3]}");
    F64Linears lin;
    f64_linears("molann::value_and_jacobian", *e, x, weights, biases, lin, ": call .double()");
    std::lock_guard<std::mutex> lock(e->mu);
    TORCH_CHECK_NOT_IMPLEMENTED(molann_plan_supports_value_and_jacobian_f64(e->plan) == 1,
                                "molann::value_and_jacobian: one frame's rows exceed the LDS of a compute unit for this model; use value_and_vjp "
                                "on x.expand(d_out, ...) with torch.eye(d_out) as cotangent");
    if (n == 0) return {out, jac};
    hipStream_t stream = c10::hip::getCurrentHIPStream(x.get_device()).stream();
    sync_live(*e, x, ref_x, weights, biases, stream);
    check(molann_value_and_jacobian_f64(e->plan, x.data_ptr<double>(), n, lin.W.data(), lin.B.data(), out.data_ptr<double>(), jac.data_ptr<double>(),
                                        stream),
          "molann_value_and_jacobian_f64");
    return {out, jac};
}
std::vector<at::Tensor> value_and_jacobian_hip(const at::Tensor& x_in, std::vector<int64_t> desc, const at::Tensor& ref_x, std::vector<at::Tensor> weights,
                                               std::vector<at::Tensor> biases, std::vector<at::Tensor> into) {
    return value_and_jacobian_impl(x_in, desc, ref_x, weights, biases, into);
}
std::vector<at::Tensor> value_and_jacobian_h_hip(const at::Tensor& x_in, int64_t handle, const at::Tensor& ref_x, std::vector<at::Tensor> weights,
                                                 std::vector<at::Tensor> biases, std::vector<at::Tensor> into) {
    return value_and_jacobian_impl(x_in, *desc_of(handle, "molann::value_and_jacobian_h"), ref_x, weights, biases, into);
}

// {out, metric}: the float64 forward's outputs and the metric tensor metric[N, out_dim, out_dim] = sum_a atom_w[a] (d out_k / d x_a) .
// (d out_l / d x_a) in ONE launch (molann_value_and_metric_f64 on the float64 Linear tensors).  Parameters are data.  atom_w: n_inp
// float64 values on x's device, or none for all ones.  `into` as value_and_jacobian's: {out, metric}.
std::vector<at::Tensor> value_and_metric_impl(const at::Tensor& x_in, const std::vector<int64_t>& desc, const at::Tensor& ref_x,
                                              const std::vector<at::Tensor>& weights, const std::vector<at::Tensor>& biases,
                                              const c10::optional<at::Tensor>& atom_w_in, const std::vector<at::Tensor>& into) {
    check_x(x_in, desc);
    TORCH_CHECK_TYPE(x_in.scalar_type() == at::kDouble, "molann::value_and_metric is float64: call model.double() and pass a float64 x (got ",
                     x_in.scalar_type(), ")");
    TORCH_CHECK(desc[1] == KIND_FORWARD || desc[1] == KIND_FEATURES, "molann::value_and_metric: a forward or a features description");
    const at::Tensor x = x_in.contiguous();
    const c10::DeviceGuard guard(x.device());
    auto e = entry_for(desc, x, ref_x);
    const int64_t n = x.size(0);
    const int64_t cols = e->kind == KIND_FORWARD ? e->out_dim : e->feature_dim;
    at::Tensor atom_w;
    if (atom_w_in.has_value() && atom_w_in->defined()) {
        TORCH_CHECK_TYPE(atom_w_in->scalar_type() == at::kDouble, "molann::value_and_metric: `weights` must be float64 (got ", atom_w_in->scalar_type(), ")");
        TORCH_CHECK_VALUE(atom_w_in->numel() == x.size(1) && atom_w_in->device() == x.device(), "molann::value_and_metric: `weights` must hold ", x.size(1),
                          " values (one per atom) on ", x.device());
        atom_w = atom_w_in->detach().reshape({-1}).contiguous();
    }
    const auto [out, metric] = into_pair("molann::value_and_metric", into, x, {n, cols}, {n, cols, cols}, "(out, metric)",
                                         "{[N, out_dim], [N, out_dim, out_dim]}");
    F64Linears lin;
    f64_linears("molann::value_and_metric", *e, x, weights, biases, lin, ": call .double()");
    std::lock_guard<std::mutex> lock(e->mu);
    TORCH_CHECK_NOT_IMPLEMENTED(molann_plan_supports_value_and_metric_f64(e->plan) == 1,
                                "molann::value_and_metric: no single-launch kernel for this model (more than 64 outputs, or one frame's rows exceed "
                                "the LDS of a compute unit); use value_and_jacobian and torch.einsum(\"fkai,a,flai->fkl\", jac, w, jac)");
    if (n == 0) return {out, metric};
    hipStream_t stream = c10::hip::getCurrentHIPStream(x.get_device()).stream();
    sync_live(*e, x, ref_x, weights, biases, stream);
    check(molann_value_and_metric_f64(e->plan, x.data_ptr<double>(), n, lin.W.data(), lin.B.data(), atom_w.defined() ? atom_w.data_ptr<double>() : nullptr,
                                      out.data_ptr<double>(), metric.data_ptr<double>(), stream),
          "molann_value_and_metric_f64");
    return {out, metric};
}
std::vector<at::Tensor> value_and_metric_h_hip(const at::Tensor& x_in, int64_t handle, const at::Tensor& ref_x, std::vector<at::Tensor> weights,
                                               std::vector<at::Tensor> biases, const c10::optional<at::Tensor>& atom_w, std::vector<at::Tensor> into) {
    return value_and_metric_impl(x_in, *desc_of(handle, "molann::value_and_metric_h"), ref_x, weights, biases, atom_w, into);
}

// {out, energy, grad_x}: the float64 forward's outputs, the energy of a harmonic restraint on them, energy[N] = 1/2 sum_k kappa_k d_k^2 with
// d = out - center (wrapped where period > 0, cut where flat > 0), and its gradient grad_x[N, n_inp, 3] in ONE launch
// (molann_value_and_restraint_f64 on the float64 Linear tensors).  Parameters, centres and stiffnesses are data.  center: [out_dim] or
// [N, out_dim]; kappa, period, flat: [out_dim]; all float64 on x's device (the Python methods convert what is not).  `into`: none or
// {out, energy, grad_x}.
at::Tensor restraint_row(const char* what, const at::Tensor& t, const at::Tensor& x, int64_t cols, int64_t rows) {
    TORCH_CHECK_TYPE(t.scalar_type() == at::kDouble, "molann::value_and_restraint: `", what, "` must be float64 (got ", t.scalar_type(), ")");
    const bool row = t.dim() == 1 && t.size(0) == cols, per_frame = rows >= 0 && t.dim() == 2 && t.size(0) == rows && t.size(1) == cols;
    TORCH_CHECK_VALUE((row || per_frame) && t.device() == x.device(), "molann::value_and_restraint: `", what, "` must be [", cols,
                      rows >= 0 ? "] or [N, out_dim]" : "]", " on ", x.device());
    return t.detach().contiguous();
}
std::vector<at::Tensor> value_and_restraint_impl(const at::Tensor& x_in, const std::vector<int64_t>& desc, const at::Tensor& ref_x,
                                                 const std::vector<at::Tensor>& weights, const std::vector<at::Tensor>& biases,
                                                 const at::Tensor& center_in, const at::Tensor& kappa_in, const c10::optional<at::Tensor>& period_in,
                                                 const c10::optional<at::Tensor>& flat_in, const std::vector<at::Tensor>& into) {
    check_x(x_in, desc);
    TORCH_CHECK_TYPE(x_in.scalar_type() == at::kDouble, "molann::value_and_restraint is float64: call model.double() and pass a float64 x (got ",
                     x_in.scalar_type(), ")");
    TORCH_CHECK(desc[1] == KIND_FORWARD || desc[1] == KIND_FEATURES, "molann::value_and_restraint: a forward or a features description");
    const at::Tensor x = x_in.contiguous();
    const c10::DeviceGuard guard(x.device());
    auto e = entry_for(desc, x, ref_x);
    const int64_t n = x.size(0);
    const int64_t cols = e->kind == KIND_FORWARD ? e->out_dim : e->feature_dim;
    const at::Tensor center = restraint_row("center", center_in, x, cols, n), kappa = restraint_row("kappa", kappa_in, x, cols, -1);
    at::Tensor period, flat;
    if (period_in.has_value() && period_in->defined()) period = restraint_row("period", *period_in, x, cols, -1);
    if (flat_in.has_value() && flat_in->defined()) flat = restraint_row("flat", *flat_in, x, cols, -1);
    TORCH_CHECK(into.empty() || into.size() == 3, "molann::value_and_restraint: `into` must be a triple of tensors (out, energy, grad_x)");
    at::Tensor out, energy, gx;
    if (into.empty()) {
        out = at::empty({n, cols}, x.options()); energy = at::empty({n}, x.options()); gx = at::empty_like(x);
    } else {
        out = into[0]; energy = into[1]; gx = into[2];
        const int64_t counts[3] = {n * cols, n, x.numel()};
        for (int i = 0; i < 3; ++i) {
            TORCH_CHECK_TYPE(into[i].scalar_type() == at::kDouble, "molann::value_and_restraint: `into` must be float64 like x");
            TORCH_CHECK_VALUE(into[i].is_contiguous() && into[i].numel() == counts[i] && into[i].device() == x.device(),
                              "molann::value_and_restraint: `into` must be contiguous {[N, out_dim], [N], [N, n_inp, 3]} on x's device");
        }
    }
    F64Linears lin;
    f64_linears("molann::value_and_restraint", *e, x, weights, biases, lin, ": call .double()");
    std::lock_guard<std::mutex> lock(e->mu);
    TORCH_CHECK_NOT_IMPLEMENTED(molann_plan_supports_value_and_restraint_f64(e->plan) == 1,
                                "molann::value_and_restraint: one frame's rows exceed the LDS of a compute unit for this model; use run, form "
                                "kappa * d and the energy with torch, then value_and_vjp");
    if (n == 0) return {out, energy, gx};
    hipStream_t stream = c10::hip::getCurrentHIPStream(x.get_device()).stream();
    sync_live(*e, x, ref_x, weights, biases, stream);
    check(molann_value_and_restraint_f64(e->plan, x.data_ptr<double>(), n, lin.W.data(), lin.B.data(), center.data_ptr<double>(),
                                         center.dim() == 2 ? cols : 0, kappa.data_ptr<double>(), period.defined() ? period.data_ptr<double>() : nullptr,
                                         flat.defined() ? flat.data_ptr<double>() : nullptr, out.data_ptr<double>(), energy.data_ptr<double>(),
                                         gx.data_ptr<double>(), stream),
          "molann_value_and_restraint_f64");
    return {out, energy, gx};
}
std::vector<at::Tensor> value_and_restraint_hip(const at::Tensor& x_in, std::vector<int64_t> desc, const at::Tensor& ref_x, std::vector<at::Tensor> weights,
                                                std::vector<at::Tensor> biases, const at::Tensor& center, const at::Tensor& kappa,
                                                const c10::optional<at::Tensor>& period, const c10::optional<at::Tensor>& flat,
                                                std::vector<at::Tensor> into) {
    return value_and_restraint_impl(x_in, desc, ref_x, weights, biases, center, kappa, period, flat, into);
}
std::vector<at::Tensor> value_and_restraint_h_hip(const at::Tensor& x_in, int64_t handle, const at::Tensor& ref_x, std::vector<at::Tensor> weights,
                                                  std::vector<at::Tensor> biases, const at::Tensor& center, const at::Tensor& kappa,
                                                  const c10::optional<at::Tensor>& period, const c10::optional<at::Tensor>& flat,
                                                  std::vector<at::Tensor> into) {
    return value_and_restraint_impl(x_in, *desc_of(handle, "molann::value_and_restraint_h"), ref_x, weights, biases, center, kappa, period, flat, into);
}

// {out, bias, grad_x}: the float64 forward's outputs, a metadynamics bias on them, bias[N] = sum_h heights_h exp(-1/2 sum_k (d_hk / sigma_hk)^2)
// with d_h = out - centers_h (wrapped where period > 0), and its gradient grad_x[N, n_inp, 3] in ONE launch (molann_value_and_hills_f64 on
// the float64 Linear tensors).  Parameters and hills are data.  centers: [H, out_dim]; heights: [H]; sigma: [out_dim] or [H, out_dim];
// period: [out_dim]; all float64 on x's device (the Python methods convert what is not, and check sigma > 0).  H may be 0.  `into`: none
// or {out, bias, grad_x}.
at::Tensor hills_table(const char* what, const at::Tensor& t, const at::Tensor& x, bool ok, const char* shape) {
    TORCH_CHECK_TYPE(t.scalar_type() == at::kDouble, "molann::value_and_hills: `", what, "` must be float64 (got ", t.scalar_type(), ")");
    TORCH_CHECK_VALUE(ok && t.device() == x.device(), "molann::value_and_hills: `", what, "` must be ", shape, " on ", x.device());
    return t.detach().contiguous();
}
std::vector<at::Tensor> value_and_hills_impl(const at::Tensor& x_in, const std::vector<int64_t>& desc, const at::Tensor& ref_x,
                                             const std::vector<at::Tensor>& weights, const std::vector<at::Tensor>& biases,
                                             const at::Tensor& centers_in, const at::Tensor& heights_in, const at::Tensor& sigma_in,
                                             const c10::optional<at::Tensor>& period_in, const std::vector<at::Tensor>& into) {
    check_x(x_in, desc);
    TORCH_CHECK_TYPE(x_in.scalar_type() == at::kDouble, "molann::value_and_hills is float64: call model.double() and pass a float64 x (got ",
                     x_in.scalar_type(), ")");
    TORCH_CHECK(desc[1] == KIND_FORWARD || desc[1] == KIND_FEATURES, "molann::value_and_hills: a forward or a features description");
    const at::Tensor x = x_in.contiguous();
    const c10::DeviceGuard guard(x.device());
    auto e = entry_for(desc, x, ref_x);
    const int64_t n = x.size(0);
    const int64_t cols = e->kind == KIND_FORWARD ? e->out_dim : e->feature_dim;
    const at::Tensor centers = hills_table("centers", centers_in, x, centers_in.dim() == 2 && centers_in.size(1) == cols, "[H, out_dim]");
    const int64_t n_hills = centers.size(0);
    const at::Tensor heights = hills_table("heights", heights_in, x, heights_in.dim() == 1 && heights_in.size(0) == n_hills, "[H]");
    const bool per_hill = sigma_in.dim() == 2 && sigma_in.size(0) == n_hills && sigma_in.size(1) == cols;
    const at::Tensor sigma = hills_table("sigma", sigma_in, x, per_hill || (sigma_in.dim() == 1 && sigma_in.size(0) == cols), "[out_dim] or [H, out_dim]");
    at::Tensor period;
    if (period_in.has_value() && period_in->defined())
        period = hills_table("period", *period_in, x, period_in->dim() == 1 && period_in->size(0) == cols, "[out_dim]");
    TORCH_CHECK(into.empty() || into.size() == 3, "molann::value_and_hills: `into` must be a triple of tensors (out, bias, grad_x)");
    at::Tensor out, bias, gx;
    if (into.empty()) {
        out = at::empty({n, cols}, x.options()); bias = at::empty({n}, x.options()); gx = at::empty_like(x);
    } else {
        out = into[0]; bias = into[1]; gx = into[2];
        const int64_t counts[3] = {n * cols, n, x.numel()};
        for (int i = 0; i < 3; ++i) {
            TORCH_CHECK_TYPE(into[i].scalar_type() == at::kDouble, "molann::value_and_hills: `into` must be float64 like x");
            TORCH_CHECK_VALUE(into[i].is_contiguous() && into[i].numel() == counts[i] && into[i].device() == x.device(),
                              "molann::value_and_hills: `into` must be contiguous {[N, out_dim], [N], [N, n_inp, 3]} on x's device");
        }
    }
    F64Linears lin;
    f64_linears("molann::value_and_hills", *e, x, weights, biases, lin, ": call .double()");
    std::lock_guard<std::mutex> lock(e->mu);
    TORCH_CHECK_NOT_IMPLEMENTED(molann_plan_supports_value_and_hills_f64(e->plan) == 1,
                                "molann::value_and_hills: more than 8 outputs, or one frame's rows exceed the LDS of a compute unit for this model; "
                                "use run, form the hill sum and its derivative with torch, then value_and_vjp");
    if (n == 0) return {out, bias, gx};
    hipStream_t stream = c10::hip::getCurrentHIPStream(x.get_device()).stream();
    sync_live(*e, x, ref_x, weights, biases, stream);
    check(molann_value_and_hills_f64(e->plan, x.data_ptr<double>(), n, lin.W.data(), lin.B.data(), n_hills > 0 ? centers.data_ptr<double>() : nullptr,
                                     n_hills > 0 ? heights.data_ptr<double>() : nullptr, n_hills, sigma.data_ptr<double>(), per_hill ? cols : 0,
                                     period.defined() ? period.data_ptr<double>() : nullptr, out.data_ptr<double>(), bias.data_ptr<double>(),
                                     gx.data_ptr<double>(), stream),
          "molann_value_and_hills_f64");
    return {out, bias, gx};
}
std::vector<at::Tensor> value_and_hills_hip(const at::Tensor& x_in, std::vector<int64_t> desc, const at::Tensor& ref_x, std::vector<at::Tensor> weights,
                                            std::vector<at::Tensor> biases, const at::Tensor& centers, const at::Tensor& heights, const at::Tensor& sigma,
                                            const c10::optional<at::Tensor>& period, std::vector<at::Tensor> into) {
    return value_and_hills_impl(x_in, desc, ref_x, weights, biases, centers, heights, sigma, period, into);
}
std::vector<at::Tensor> value_and_hills_h_hip(const at::Tensor& x_in, int64_t handle, const at::Tensor& ref_x, std::vector<at::Tensor> weights,
                                              std::vector<at::Tensor> biases, const at::Tensor& centers, const at::Tensor& heights,
                                              const at::Tensor& sigma, const c10::optional<at::Tensor>& period, std::vector<at::Tensor> into) {
    return value_and_hills_impl(x_in, *desc_of(handle, "molann::value_and_hills_h"), ref_x, weights, biases, centers, heights, sigma, period, into);
}

// {out, bias, grad_x}: the float64 forward's outputs, an OPES bias on them, bias[N] = scale log(P / norm + epsilon) with P = sum_h heights_h
// (exp(-q_h / 2) - exp(-cutoff^2 / 2)) over the kernels with q_h = sum_k (d_hk / sigma_hk)^2 < cutoff^2, and its gradient grad_x[N, n_inp, 3]
// in ONE launch (molann_value_and_opes_f64 on the float64 Linear tensors).  The tensors as value_and_hills takes them; scale, norm, epsilon
// and cutoff (inf: none) are host values, checked here as the C entry checks them (the Python methods have checked them already).
at::Tensor opes_table(const char* what, const at::Tensor& t, const at::Tensor& x, bool ok, const char* shape) {
    TORCH_CHECK_TYPE(t.scalar_type() == at::kDouble, "molann::value_and_opes: `", what, "` must be float64 (got ", t.scalar_type(), ")");
    TORCH_CHECK_VALUE(ok && t.device() == x.device(), "molann::value_and_opes: `", what, "` must be ", shape, " on ", x.device());
    return t.detach().contiguous();
}
std::vector<at::Tensor> value_and_opes_impl(const at::Tensor& x_in, const std::vector<int64_t>& desc, const at::Tensor& ref_x,
                                            const std::vector<at::Tensor>& weights, const std::vector<at::Tensor>& biases,
                                            const at::Tensor& centers_in, const at::Tensor& heights_in, const at::Tensor& sigma_in,
                                            const c10::optional<at::Tensor>& period_in, double scale, double norm, double epsilon, double cutoff,
                                            const std::vector<at::Tensor>& into) {
    check_x(x_in, desc);
    TORCH_CHECK_TYPE(x_in.scalar_type() == at::kDouble, "molann::value_and_opes is float64: call model.double() and pass a float64 x (got ",
                     x_in.scalar_type(), ")");
    TORCH_CHECK(desc[1] == KIND_FORWARD || desc[1] == KIND_FEATURES, "molann::value_and_opes: a forward or a features description");
    TORCH_CHECK_VALUE(std::isfinite(scale) && std::isfinite(norm) && norm > 0.0 && std::isfinite(epsilon) && epsilon > 0.0 && cutoff > 0.0,
                      "molann::value_and_opes: `scale` must be finite, `norm` and `epsilon` finite and > 0, `cutoff` > 0 (inf: none); got ", scale,
                      ", ", norm, ", ", epsilon, ", ", cutoff);
    const at::Tensor x = x_in.contiguous();
    const c10::DeviceGuard guard(x.device());
    auto e = entry_for(desc, x, ref_x);
    const int64_t n = x.size(0);
    const int64_t cols = e->kind == KIND_FORWARD ? e->out_dim : e->feature_dim;
    const at::Tensor centers = opes_table("centers", centers_in, x, centers_in.dim() == 2 && centers_in.size(1) == cols, "[H, out_dim]");
    const int64_t n_kernels = centers.size(0);
    const at::Tensor heights = opes_table("heights", heights_in, x, heights_in.dim() == 1 && heights_in.size(0) == n_kernels, "[H]");
    const bool per_kernel = sigma_in.dim() == 2 && sigma_in.size(0) == n_kernels && sigma_in.size(1) == cols;
    const at::Tensor sigma = opes_table("sigma", sigma_in, x, per_kernel || (sigma_in.dim() == 1 && sigma_in.size(0) == cols), "[out_dim] or [H, out_dim]");
    at::Tensor period;
    if (period_in.has_value() && period_in->defined())
        period = opes_table("period", *period_in, x, period_in->dim() == 1 && period_in->size(0) == cols, "[out_dim]");
    TORCH_CHECK(into.empty() || into.size() == 3, "molann::value_and_opes: `into` must be a triple of tensors (out, bias, grad_x)");
    at::Tensor out, bias, gx;
    if (into.empty()) {
        out = at::empty({n, cols}, x.options()); bias = at::empty({n}, x.options()); gx = at::empty_like(x);
    } else {
        out = into[0]; bias = into[1]; gx = into[2];
        const int64_t counts[3] = {n * cols, n, x.numel()};
        for (int i = 0; i < 3; ++i) {
            TORCH_CHECK_TYPE(into[i].scalar_type() == at::kDouble, "molann::value_and_opes: `into` must be float64 like x");
            TORCH_CHECK_VALUE(into[i].is_contiguous() && into[i].numel() == counts[i] && into[i].device() == x.device(),
                              "molann::value_and_opes: `into` must be contiguous {[N, out_dim], [N], [N, n_inp, 3]} on x's device");
        }
    }
    F64Linears lin;
    f64_linears("molann::value_and_opes", *e, x, weights, biases, lin, ": call .double()");
    std::lock_guard<std::mutex> lock(e->mu);
    TORCH_CHECK_NOT_IMPLEMENTED(molann_plan_supports_value_and_opes_f64(e->plan) == 1,
                                "molann::value_and_opes: more than 8 outputs, or one frame's rows exceed the LDS of a compute unit for this model; "
                                "use run, form the kernel sum, its logarithm and its derivative with torch, then value_and_vjp");
    if (n == 0) return {out, bias, gx};
    hipStream_t stream = c10::hip::getCurrentHIPStream(x.get_device()).stream();
    sync_live(*e, x, ref_x, weights, biases, stream);
    check(molann_value_and_opes_f64(e->plan, x.data_ptr<double>(), n, lin.W.data(), lin.B.data(), n_kernels > 0 ? centers.data_ptr<double>() : nullptr,
                                    n_kernels > 0 ? heights.data_ptr<double>() : nullptr, n_kernels, sigma.data_ptr<double>(), per_kernel ? cols : 0,
                                    period.defined() ? period.data_ptr<double>() : nullptr, scale, norm, epsilon, cutoff, out.data_ptr<double>(),
                                    bias.data_ptr<double>(), gx.data_ptr<double>(), stream),
          "molann_value_and_opes_f64");
    return {out, bias, gx};
}
std::vector<at::Tensor> value_and_opes_hip(const at::Tensor& x_in, std::vector<int64_t> desc, const at::Tensor& ref_x, std::vector<at::Tensor> weights,
                                           std::vector<at::Tensor> biases, const at::Tensor& centers, const at::Tensor& heights, const at::Tensor& sigma,
                                           const c10::optional<at::Tensor>& period, double scale, double norm, double epsilon, double cutoff,
                                           std::vector<at::Tensor> into) {
    return value_and_opes_impl(x_in, desc, ref_x, weights, biases, centers, heights, sigma, period, scale, norm, epsilon, cutoff, into);
}
std::vector<at::Tensor> value_and_opes_h_hip(const at::Tensor& x_in, int64_t handle, const at::Tensor& ref_x, std::vector<at::Tensor> weights,
                                             std::vector<at::Tensor> biases, const at::Tensor& centers, const at::Tensor& heights,
                                             const at::Tensor& sigma, const c10::optional<at::Tensor>& period, double scale, double norm,
                                             double epsilon, double cutoff, std::vector<at::Tensor> into) {
    return value_and_opes_impl(x_in, *desc_of(handle, "molann::value_and_opes_h"), ref_x, weights, biases, centers, heights, sigma, period, scale, norm,
                               epsilon, cutoff, into);
}

// {out, bias, grad_x}: the float64 forward's outputs, a bias interpolated from `table` over them (cubic convolution on a regular grid: one
// axis of the table per output, point i of axis k at lower[k] + i spacing[k], periodic[k] wraps with period n_k spacing[k]) and its gradient
// grad_x[N, n_inp, 3] in ONE launch (molann_value_and_grid_f64 on the float64 Linear tensors).  Parameters and the table are data.  table:
// float64, contiguous, on x's device, out_dim <= 3 dimensions of at least 4 points; lower, spacing, periodic: out_dim host values (periodic
// may be empty: no axis is periodic).  `into`: none or {out, bias, grad_x}.
std::vector<at::Tensor> value_and_grid_impl(const at::Tensor& x_in, const std::vector<int64_t>& desc, const at::Tensor& ref_x,
                                            const std::vector<at::Tensor>& weights, const std::vector<at::Tensor>& biases, const at::Tensor& table,
                                            const std::vector<double>& lower, const std::vector<double>& spacing, const c10::List<bool>& periodic_in,
                                            const std::vector<at::Tensor>& into) {
    check_x(x_in, desc);
    TORCH_CHECK_TYPE(x_in.scalar_type() == at::kDouble, "molann::value_and_grid is float64: call model.double() and pass a float64 x (got ",
                     x_in.scalar_type(), ")");
    TORCH_CHECK(desc[1] == KIND_FORWARD || desc[1] == KIND_FEATURES, "molann::value_and_grid: a forward or a features description");
    const at::Tensor x = x_in.contiguous();
    const c10::DeviceGuard guard(x.device());
    auto e = entry_for(desc, x, ref_x);
    const int64_t n = x.size(0);
    const int64_t cols = e->kind == KIND_FORWARD ? e->out_dim : e->feature_dim;
    TORCH_CHECK_NOT_IMPLEMENTED(cols <= 3, "molann::value_and_grid: the one-launch kernel serves at most 3 outputs (got ", cols,
                                "); use run, interpolate the table and its derivative with torch, then value_and_vjp");
    TORCH_CHECK_TYPE(table.scalar_type() == at::kDouble, "molann::value_and_grid: `table` must be float64 (got ", table.scalar_type(), ")");
    TORCH_CHECK_VALUE(table.dim() == cols && table.is_contiguous() && table.device() == x.device(),
                      "molann::value_and_grid: `table` must be contiguous with one dimension per output (", cols, ") on ", x.device());
    TORCH_CHECK_VALUE((int64_t)lower.size() == cols && (int64_t)spacing.size() == cols && (periodic_in.size() == 0 || (int64_t)periodic_in.size() == cols),
                      "molann::value_and_grid: `lower`, `spacing` and `periodic` must hold one value per output (", cols, ")");
    int64_t shape[3] = {4, 4, 4};
    int32_t periodic[3] = {0, 0, 0};
    for (int64_t k = 0; k < cols; ++k) {
        shape[k] = table.size(k);
        TORCH_CHECK_VALUE(shape[k] >= 4, "molann::value_and_grid: every dimension of `table` must have at least 4 points (got ", shape[k], ")");
        TORCH_CHECK_VALUE(std::isfinite(spacing[k]) && spacing[k] > 0.0 && std::isfinite(lower[k]),
                          "molann::value_and_grid: `spacing` must be finite and > 0 and `lower` finite");
        periodic[k] = periodic_in.size() > 0 && periodic_in.get(k) ? 1 : 0;
    }
    TORCH_CHECK_VALUE(table.numel() < (int64_t(1) << 31), "molann::value_and_grid: `table` must hold fewer than 2^31 points");
    TORCH_CHECK(into.empty() || into.size() == 3, "molann::value_and_grid: `into` must be a triple of tensors (out, bias, grad_x)");
    at::Tensor out, bias, gx;
    if (into.empty()) {
        out = at::empty({n, cols}, x.options()); bias = at::empty({n}, x.options()); gx = at::empty_like(x);
    } else {
        out = into[0]; bias = into[1]; gx = into[2];
        const int64_t counts[3] = {n * cols, n, x.numel()};
        for (int i = 0; i < 3; ++i) {
            TORCH_CHECK_TYPE(into[i].scalar_type() == at::kDouble, "molann::value_and_grid: `into` must be float64 like x");
            TORCH_CHECK_VALUE(into[i].is_contiguous() && into[i].numel() == counts[i] && into[i].device() == x.device(),
                              "molann::value_and_grid: `into` must be contiguous {[N, out_dim], [N], [N, n_inp, 3]} on x's device");
        }
    }
    F64Linears lin;
    f64_linears("molann::value_and_grid", *e, x, weights, biases, lin, ": call .double()");
    std::lock_guard<std::mutex> lock(e->mu);
    TORCH_CHECK_NOT_IMPLEMENTED(molann_plan_supports_value_and_grid_f64(e->plan) == 1,
                                "molann::value_and_grid: one frame's rows exceed the LDS of a compute unit for this model; use run, interpolate "
                                "the table and its derivative with torch, then value_and_vjp");
    if (n == 0) return {out, bias, gx};
    hipStream_t stream = c10::hip::getCurrentHIPStream(x.get_device()).stream();
    sync_live(*e, x, ref_x, weights, biases, stream);
    check(molann_value_and_grid_f64(e->plan, x.data_ptr<double>(), n, lin.W.data(), lin.B.data(), table.data_ptr<double>(), shape, lower.data(),
                                    spacing.data(), periodic, out.data_ptr<double>(), bias.data_ptr<double>(), gx.data_ptr<double>(), stream),
          "molann_value_and_grid_f64");
    return {out, bias, gx};
}
std::vector<at::Tensor> value_and_grid_hip(const at::Tensor& x_in, std::vector<int64_t> desc, const at::Tensor& ref_x, std::vector<at::Tensor> weights,
                                           std::vector<at::Tensor> biases, const at::Tensor& table, std::vector<double> lower,
                                           std::vector<double> spacing, c10::List<bool> periodic, std::vector<at::Tensor> into) {
    return value_and_grid_impl(x_in, desc, ref_x, weights, biases, table, lower, spacing, periodic, into);
}
std::vector<at::Tensor> value_and_grid_h_hip(const at::Tensor& x_in, int64_t handle, const at::Tensor& ref_x, std::vector<at::Tensor> weights,
                                             std::vector<at::Tensor> biases, const at::Tensor& table, std::vector<double> lower,
                                             std::vector<double> spacing, c10::List<bool> periodic, std::vector<at::Tensor> into) {
    return value_and_grid_impl(x_in, *desc_of(handle, "molann::value_and_grid_h"), ref_x, weights, biases, table, lower, spacing, periodic, into);
}

// {out, energies, grad_x}: the float64 forward's outputs, up to three bias terms on chosen outputs - the restraint of value_and_restraint on all
// of them, the hills of value_and_hills on `hills_columns`, the table of value_and_grid on `grid_columns` - energies[N, 3] = (E_r, V_h, V_g)
// and the gradient of their sum grad_x[N, n_inp, 3] in ONE launch (molann_value_and_bias_f64 on the float64 Linear tensors).  A term is
// absent where `kappa` is none / a column list is empty; not all three.  The lists hold distinct output indices in any order; the hill
// table and the grid are laid out over them in the order of the list.  Tensors float64 on x's device (the Python methods convert what is
// not, and check sigma > 0); lower, spacing, periodic host values (periodic may be empty).  `into`: none or {out, energies, grad_x}.
at::Tensor bias_tensor(const char* what, const c10::optional<at::Tensor>& t, const at::Tensor& x, bool required) {
    if (!t.has_value() || !t->defined()) {
        TORCH_CHECK_VALUE(!required, "molann::value_and_bias: `", what, "` is required by a term that is present");
        return at::Tensor();
    }
    TORCH_CHECK_TYPE(t->scalar_type() == at::kDouble, "molann::value_and_bias: `", what, "` must be float64 (got ", t->scalar_type(), ")");
    TORCH_CHECK_VALUE(t->device() == x.device(), "molann::value_and_bias: `", what, "` must be on ", x.device());
    return t->detach().contiguous();
}
std::vector<int32_t> bias_columns(const char* what, const std::vector<int64_t>& columns, int64_t cap, int64_t cols) {
    std::vector<int32_t> list;
    for (size_t j = 0; j < columns.size(); ++j) {
        TORCH_CHECK_INDEX(columns[j] >= 0 && columns[j] < cols, "molann::value_and_bias: `", what, "` must lie in [0, ", cols, "); got ", columns[j]);
        for (size_t i = 0; i < j; ++i) TORCH_CHECK_INDEX(columns[i] != columns[j], "molann::value_and_bias: `", what, "` must be distinct");
        list.push_back((int32_t)columns[j]);
    }
    TORCH_CHECK_NOT_IMPLEMENTED((int64_t)columns.size() <= cap, "molann::value_and_bias: the one-launch kernel serves at most ", cap, " `", what,
                                "` (got ", columns.size(), "); use run, form the terms on the chosen columns with torch, then value_and_vjp");
    return list;
}
std::vector<at::Tensor> value_and_bias_impl(const at::Tensor& x_in, const std::vector<int64_t>& desc, const at::Tensor& ref_x,
                                            const std::vector<at::Tensor>& weights, const std::vector<at::Tensor>& biases,
                                            const c10::optional<at::Tensor>& center_in, const c10::optional<at::Tensor>& kappa_in,
                                            const c10::optional<at::Tensor>& rperiod_in, const c10::optional<at::Tensor>& flat_in,
                                            const std::vector<int64_t>& hills_columns, const c10::optional<at::Tensor>& centers_in,
                                            const c10::optional<at::Tensor>& heights_in, const c10::optional<at::Tensor>& sigma_in,
                                            const c10::optional<at::Tensor>& hperiod_in, const std::vector<int64_t>& grid_columns,
                                            const c10::optional<at::Tensor>& table_in, const std::vector<double>& lower,
                                            const std::vector<double>& spacing, const c10::List<bool>& periodic_in, const std::vector<at::Tensor>& into) {
    check_x(x_in, desc);
    TORCH_CHECK_TYPE(x_in.scalar_type() == at::kDouble, "molann::value_and_bias is float64: call model.double() and pass a float64 x (got ",
                     x_in.scalar_type(), ")");
    TORCH_CHECK(desc[1] == KIND_FORWARD || desc[1] == KIND_FEATURES, "molann::value_and_bias: a forward or a features description");
    const at::Tensor x = x_in.contiguous();
    const c10::DeviceGuard guard(x.device());
    auto e = entry_for(desc, x, ref_x);
    const int64_t n = x.size(0);
    const int64_t cols = e->kind == KIND_FORWARD ? e->out_dim : e->feature_dim;
    const bool has_r = kappa_in.has_value() && kappa_in->defined(), has_h = !hills_columns.empty(), has_g = !grid_columns.empty();
    TORCH_CHECK_VALUE(has_r || has_h || has_g, "molann::value_and_bias: at least one of the restraint, the hills and the table must be given");
    const std::vector<int32_t> hc = bias_columns("hills_columns", hills_columns, 8, cols), gc = bias_columns("grid_columns", grid_columns, 3, cols);
    const int64_t dh = (int64_t)hc.size(), dg = (int64_t)gc.size();
    molann_bias_terms_f64 t;
    memset(&t, 0, sizeof(t));
    at::Tensor center, kappa, rperiod, flat, centers, heights, sigma, hperiod, table;
    if (has_r) {
        center = bias_tensor("center", center_in, x, true); kappa = bias_tensor("kappa", kappa_in, x, true);
        rperiod = bias_tensor("restraint_period", rperiod_in, x, false); flat = bias_tensor("flat", flat_in, x, false);
        const bool per_frame = center.dim() == 2 && center.size(0) == n && center.size(1) == cols;
        TORCH_CHECK_VALUE(per_frame || (center.dim() == 1 && center.size(0) == cols), "molann::value_and_bias: `center` must be [", cols, "] or [N, out_dim]");
        TORCH_CHECK_VALUE(kappa.dim() == 1 && kappa.size(0) == cols && (!rperiod.defined() || (rperiod.dim() == 1 && rperiod.size(0) == cols)) &&
                              (!flat.defined() || (flat.dim() == 1 && flat.size(0) == cols)),
                          "molann::value_and_bias: `kappa`, `restraint_period` and `flat` must be [", cols, "]");
        t.center = center.data_ptr<double>(); t.center_stride = per_frame ? cols : 0; t.kappa = kappa.data_ptr<double>();
        t.restraint_period = rperiod.defined() ? rperiod.data_ptr<double>() : nullptr;
        t.flat = flat.defined() ? flat.data_ptr<double>() : nullptr;
    }
    if (has_h) {
        centers = bias_tensor("centers", centers_in, x, true); heights = bias_tensor("heights", heights_in, x, true);
        sigma = bias_tensor("sigma", sigma_in, x, true); hperiod = bias_tensor("hills_period", hperiod_in, x, false);
        TORCH_CHECK_VALUE(centers.dim() == 2 && centers.size(1) == dh, "molann::value_and_bias: `centers` must be [H, ", dh, "]");
        const int64_t n_hills = centers.size(0);
        const bool per_hill = sigma.dim() == 2 && sigma.size(0) == n_hills && sigma.size(1) == dh;
        TORCH_CHECK_VALUE(heights.dim() == 1 && heights.size(0) == n_hills && (per_hill || (sigma.dim() == 1 && sigma.size(0) == dh)) &&
                              (!hperiod.defined() || (hperiod.dim() == 1 && hperiod.size(0) == dh)),
                          "molann::value_and_bias: `heights` must be [H], `sigma` [", dh, "] or [H, ", dh, "], `hills_period` [", dh, "]");
        t.n_hills_columns = (int32_t)dh; t.hills_columns = hc.data(); t.n_hills = n_hills;
        t.centers = n_hills > 0 ? centers.data_ptr<double>() : nullptr; t.heights = n_hills > 0 ? heights.data_ptr<double>() : nullptr;
        t.sigma = n_hills > 0 ? sigma.data_ptr<double>() : nullptr; t.sigma_stride = per_hill ? dh : 0;
        t.hills_period = hperiod.defined() ? hperiod.data_ptr<double>() : nullptr;
    }
    int64_t shape[3] = {4, 4, 4};
    int32_t periodic[3] = {0, 0, 0};
    if (has_g) {
        table = bias_tensor("table", table_in, x, true);
        TORCH_CHECK_VALUE(table.dim() == dg && table_in->is_contiguous(), "molann::value_and_bias: `table` must be contiguous with one dimension per "
                          "grid column (", dg, ")");
        TORCH_CHECK_VALUE((int64_t)lower.size() == dg && (int64_t)spacing.size() == dg && (periodic_in.size() == 0 || (int64_t)periodic_in.size() == dg),
                          "molann::value_and_bias: `lower`, `spacing` and `periodic` must hold one value per grid column (", dg, ")");
        for (int64_t k = 0; k < dg; ++k) {
            shape[k] = table.size(k);
            TORCH_CHECK_VALUE(shape[k] >= 4, "molann::value_and_bias: every dimension of `table` must have at least 4 points (got ", shape[k], ")");
            TORCH_CHECK_VALUE(std::isfinite(spacing[k]) && spacing[k] > 0.0 && std::isfinite(lower[k]),
                              "molann::value_and_bias: `spacing` must be finite and > 0 and `lower` finite");
            periodic[k] = periodic_in.size() > 0 && periodic_in.get(k) ? 1 : 0;
        }
        TORCH_CHECK_VALUE(table.numel() < (int64_t(1) << 31), "molann::value_and_bias: `table` must hold fewer than 2^31 points");
        t.n_grid_columns = (int32_t)dg; t.grid_columns = gc.data(); t.table = table.data_ptr<double>();
        t.shape = shape; t.lower = lower.data(); t.spacing = spacing.data(); t.periodic = periodic;
    }
    TORCH_CHECK(into.empty() || into.size() == 3, "molann::value_and_bias: `into` must be a triple of tensors (out, energies, grad_x)");
    at::Tensor out, energies, gx;
    if (into.empty()) {
        out = at::empty({n, cols}, x.options()); energies = at::empty({n, 3}, x.options()); gx = at::empty_like(x);
    } else {
        out = into[0]; energies = into[1]; gx = into[2];
        const int64_t counts[3] = {n * cols, 3 * n, x.numel()};
        for (int i = 0; i < 3; ++i) {
            TORCH_CHECK_TYPE(into[i].scalar_type() == at::kDouble, "molann::value_and_bias: `into` must be float64 like x");
            TORCH_CHECK_VALUE(into[i].is_contiguous() && into[i].numel() == counts[i] && into[i].device() == x.device(),
                              "molann::value_and_bias: `into` must be contiguous {[N, out_dim], [N, 3], [N, n_inp, 3]} on x's device");
        }
    }
    F64Linears lin;
    f64_linears("molann::value_and_bias", *e, x, weights, biases, lin, ": call .double()");
    std::lock_guard<std::mutex> lock(e->mu);
    TORCH_CHECK_NOT_IMPLEMENTED(molann_plan_supports_value_and_bias_f64(e->plan) == 1,
                                "molann::value_and_bias: one frame's rows exceed the LDS of a compute unit for this model; use run, form the terms "
                                "on the chosen columns with torch, then value_and_vjp");
    if (n == 0) return {out, energies, gx};
    hipStream_t stream = c10::hip::getCurrentHIPStream(x.get_device()).stream();
    sync_live(*e, x, ref_x, weights, biases, stream);
    check(molann_value_and_bias_f64(e->plan, x.data_ptr<double>(), n, lin.W.data(), lin.B.data(), &t, out.data_ptr<double>(),
                                    energies.data_ptr<double>(), gx.data_ptr<double>(), stream),
          "molann_value_and_bias_f64");
    return {out, energies, gx};
}
#define MOLANN_BIAS_OP_PARAMS                                                                                                                        \
    const at::Tensor &ref_x, std::vector<at::Tensor> weights, std::vector<at::Tensor> biases, const c10::optional<at::Tensor>&center,                \
        const c10::optional<at::Tensor>&kappa, const c10::optional<at::Tensor>&rperiod, const c10::optional<at::Tensor>&flat,                        \
        std::vector<int64_t> hills_columns, const c10::optional<at::Tensor>&centers, const c10::optional<at::Tensor>&heights,                        \
        const c10::optional<at::Tensor>&sigma, const c10::optional<at::Tensor>&hperiod, std::vector<int64_t> grid_columns,                           \
        const c10::optional<at::Tensor>&table, std::vector<double> lower, std::vector<double> spacing, c10::List<bool> periodic,                     \
        std::vector<at::Tensor> into
#define MOLANN_BIAS_OP_ARGS                                                                                                                          \
    ref_x, weights, biases, center, kappa, rperiod, flat, hills_columns, centers, heights, sigma, hperiod, grid_columns, table, lower, spacing, periodic, into
std::vector<at::Tensor> value_and_bias_hip(const at::Tensor& x_in, std::vector<int64_t> desc, MOLANN_BIAS_OP_PARAMS) {
    return value_and_bias_impl(x_in, desc, MOLANN_BIAS_OP_ARGS);
}
std::vector<at::Tensor> value_and_bias_h_hip(const at::Tensor& x_in, int64_t handle, MOLANN_BIAS_OP_PARAMS) {
    return value_and_bias_impl(x_in, *desc_of(handle, "molann::value_and_bias_h"), MOLANN_BIAS_OP_ARGS);
}

// {out, energies, grad_x}: value_and_bias with an OPES term in the place of the hills - the restraint of value_and_restraint on all outputs, the
// kernel density of value_and_opes on `opes_columns` (required, at most 8), the table of value_and_grid on `grid_columns` - energies[N, 4] =
// (E_r, 0, V_g, V_o) and the gradient of their sum grad_x[N, n_inp, 3] in ONE launch (molann_value_and_bias_opes_f64 on the float64 Linear
// tensors).  The restraint is absent where `kappa` is none, the table where `grid_columns` is empty.  The kernel table is laid out over
// `opes_columns` in the order of the list; scale, norm, epsilon and cutoff (inf: none) are host values, checked here as the C entry checks
// them.  bias_tensor and bias_columns are value_and_bias': the Python method of both operators is value_and_bias.
std::vector<at::Tensor> value_and_bias_opes_impl(const at::Tensor& x_in, const std::vector<int64_t>& desc, const at::Tensor& ref_x,
                                                 const std::vector<at::Tensor>& weights, const std::vector<at::Tensor>& biases,
                                                 const c10::optional<at::Tensor>& center_in, const c10::optional<at::Tensor>& kappa_in,
                                                 const c10::optional<at::Tensor>& rperiod_in, const c10::optional<at::Tensor>& flat_in,
                                                 const std::vector<int64_t>& opes_columns, const at::Tensor& centers_in, const at::Tensor& heights_in,
                                                 const at::Tensor& sigma_in, const c10::optional<at::Tensor>& operiod_in, double scale, double norm,
                                                 double epsilon, double cutoff, const std::vector<int64_t>& grid_columns,
                                                 const c10::optional<at::Tensor>& table_in, const std::vector<double>& lower,
                                                 const std::vector<double>& spacing, const c10::List<bool>& periodic_in,
                                                 const std::vector<at::Tensor>& into) {
    check_x(x_in, desc);
    TORCH_CHECK_TYPE(x_in.scalar_type() == at::kDouble, "molann::value_and_bias_opes is float64: call model.double() and pass a float64 x (got ",
                     x_in.scalar_type(), ")");
    TORCH_CHECK(desc[1] == KIND_FORWARD || desc[1] == KIND_FEATURES, "molann::value_and_bias_opes: a forward or a features description");
    TORCH_CHECK_VALUE(std::isfinite(scale) && std::isfinite(norm) && norm > 0.0 && std::isfinite(epsilon) && epsilon > 0.0 && cutoff > 0.0,
                      "molann::value_and_bias_opes: `scale` must be finite, `norm` and `epsilon` finite and > 0, `cutoff` > 0 (inf: none); got ", scale,
                      ", ", norm, ", ", epsilon, ", ", cutoff);
    const at::Tensor x = x_in.contiguous();
    const c10::DeviceGuard guard(x.device());
    auto e = entry_for(desc, x, ref_x);
    const int64_t n = x.size(0);
    const int64_t cols = e->kind == KIND_FORWARD ? e->out_dim : e->feature_dim;
    const bool has_r = kappa_in.has_value() && kappa_in->defined(), has_g = !grid_columns.empty();
    TORCH_CHECK_VALUE(!opes_columns.empty(), "molann::value_and_bias_opes: `opes_columns` must name at least one output");
    const std::vector<int32_t> oc = bias_columns("opes_columns", opes_columns, 8, cols), gc = bias_columns("grid_columns", grid_columns, 3, cols);
    const int64_t dop = (int64_t)oc.size(), dg = (int64_t)gc.size();
    molann_bias_terms_f64 t;
    molann_opes_term_f64 o;
    memset(&t, 0, sizeof(t));
    memset(&o, 0, sizeof(o));
    at::Tensor center, kappa, rperiod, flat, table;
    if (has_r) {
        center = bias_tensor("center", center_in, x, true); kappa = bias_tensor("kappa", kappa_in, x, true);
        rperiod = bias_tensor("restraint_period", rperiod_in, x, false); flat = bias_tensor("flat", flat_in, x, false);
        const bool per_frame = center.dim() == 2 && center.size(0) == n && center.size(1) == cols;
        TORCH_CHECK_VALUE(per_frame || (center.dim() == 1 && center.size(0) == cols), "molann::value_and_bias_opes: `center` must be [", cols,
                          "] or [N, out_dim]");
        TORCH_CHECK_VALUE(kappa.dim() == 1 && kappa.size(0) == cols && (!rperiod.defined() || (rperiod.dim() == 1 && rperiod.size(0) == cols)) &&
                              (!flat.defined() || (flat.dim() == 1 && flat.size(0) == cols)),
                          "molann::value_and_bias_opes: `kappa`, `restraint_period` and `flat` must be [", cols, "]");
        t.center = center.data_ptr<double>(); t.center_stride = per_frame ? cols : 0; t.kappa = kappa.data_ptr<double>();
        t.restraint_period = rperiod.defined() ? rperiod.data_ptr<double>() : nullptr;
        t.flat = flat.defined() ? flat.data_ptr<double>() : nullptr;
    }
    const at::Tensor centers = opes_table("centers", centers_in, x, centers_in.dim() == 2 && centers_in.size(1) == dop, "[H, opes columns]");
    const int64_t n_kernels = centers.size(0);
    const at::Tensor heights = opes_table("heights", heights_in, x, heights_in.dim() == 1 && heights_in.size(0) == n_kernels, "[H]");
    const bool per_kernel = sigma_in.dim() == 2 && sigma_in.size(0) == n_kernels && sigma_in.size(1) == dop;
    const at::Tensor sigma = opes_table("sigma", sigma_in, x, per_kernel || (sigma_in.dim() == 1 && sigma_in.size(0) == dop),
                                        "[opes columns] or [H, opes columns]");
    at::Tensor operiod;
    if (operiod_in.has_value() && operiod_in->defined())
        operiod = opes_table("period", *operiod_in, x, operiod_in->dim() == 1 && operiod_in->size(0) == dop, "[opes columns]");
    o.n_columns = (int32_t)dop; o.columns = oc.data(); o.n_kernels = n_kernels;
    o.centers = n_kernels > 0 ? centers.data_ptr<double>() : nullptr; o.heights = n_kernels > 0 ? heights.data_ptr<double>() : nullptr;
    o.sigma = n_kernels > 0 ? sigma.data_ptr<double>() : nullptr; o.sigma_stride = per_kernel ? dop : 0;
    o.period = operiod.defined() ? operiod.data_ptr<double>() : nullptr;
    o.scale = scale; o.norm = norm; o.epsilon = epsilon; o.cutoff = cutoff;
    int64_t shape[3] = {4, 4, 4};
    int32_t periodic[3] = {0, 0, 0};
    if (has_g) {
        table = bias_tensor("table", table_in, x, true);
        TORCH_CHECK_VALUE(table.dim() == dg && table_in->is_contiguous(), "molann::value_and_bias_opes: `table` must be contiguous with one dimension per "
                          "grid column (", dg, ")");
        TORCH_CHECK_VALUE((int64_t)lower.size() == dg && (int64_t)spacing.size() == dg && (periodic_in.size() == 0 || (int64_t)periodic_in.size() == dg),
                          "molann::value_and_bias_opes: `lower`, `spacing` and `periodic` must hold one value per grid column (", dg, ")");
        for (int64_t k = 0; k < dg; ++k) {
            shape[k] = table.size(k);
            TORCH_CHECK_VALUE(shape[k] >= 4, "molann::value_and_bias_opes: every dimension of `table` must have at least 4 points (got ", shape[k], ")");
            TORCH_CHECK_VALUE(std::isfinite(spacing[k]) && spacing[k] > 0.0 && std::isfinite(lower[k]),
                              "molann::value_and_bias_opes: `spacing` must be finite and > 0 and `lower` finite");
            periodic[k] = periodic_in.size() > 0 && periodic_in.get(k) ? 1 : 0;
        }
        TORCH_CHECK_VALUE(table.numel() < (int64_t(1) << 31), "molann::value_and_bias_opes: `table` must hold fewer than 2^31 points");
        t.n_grid_columns = (int32_t)dg; t.grid_columns = gc.data(); t.table = table.data_ptr<double>();
        t.shape = shape; t.lower = lower.data(); t.spacing = spacing.data(); t.periodic = periodic;
    }
    TORCH_CHECK(into.empty() || into.size() == 3, "molann::value_and_bias_opes: `into` must be a triple of tensors (out, energies, grad_x)");
    at::Tensor out, energies, gx;
    if (into.empty()) {
        out = at::empty({n, cols}, x.options()); energies = at::empty({n, 4}, x.options()); gx = at::empty_like(x);
    } else {
        out = into[0]; energies = into[1]; gx = into[2];
        const int64_t counts[3] = {n * cols, 4 * n, x.numel()};
        for (int i = 0; i < 3; ++i) {
            TORCH_CHECK_TYPE(into[i].scalar_type() == at::kDouble, "molann::value_and_bias_opes: `into` must be float64 like x");
            TORCH_CHECK_VALUE(into[i].is_contiguous() && into[i].numel() == counts[i] && into[i].device() == x.device(),
                              "molann::value_and_bias_opes: `into` must be contiguous {[N, out_dim], [N, 4], [N, n_inp, 3]} on x's device");
        }
    }
    F64Linears lin;
    f64_linears("molann::value_and_bias_opes", *e, x, weights, biases, lin, ": call .double()");
    std::lock_guard<std::mutex> lock(e->mu);
    TORCH_CHECK_NOT_IMPLEMENTED(molann_plan_supports_value_and_bias_opes_f64(e->plan) == 1,
                                "molann::value_and_bias_opes: one frame's rows exceed the LDS of a compute unit for this model; use run, form the "
                                "terms on the chosen columns with torch, then value_and_vjp");
    if (n == 0) return {out, energies, gx};
    hipStream_t stream = c10::hip::getCurrentHIPStream(x.get_device()).stream();
    sync_live(*e, x, ref_x, weights, biases, stream);
    check(molann_value_and_bias_opes_f64(e->plan, x.data_ptr<double>(), n, lin.W.data(), lin.B.data(), &t, &o, out.data_ptr<double>(),
                                         energies.data_ptr<double>(), gx.data_ptr<double>(), stream),
          "molann_value_and_bias_opes_f64");
    return {out, energies, gx};
}
// The deposit step of an OPES run (molann_opes_deposit_f64): the new kernels are compressed into the caller's table in place and `state` =
// (n, S, merges, refused) is updated, in ONE launch on the current stream; nothing is read back.  The table: centers [cap, d], sigma [cap, d],
// heights [cap], state [4], contiguous float64 on one device (they are written: no copy is made); the new kernels: [W, d], [W, d], [W].
at::Tensor opes_tensor(const char* op, const char* what, const at::Tensor& t, const at::Tensor& like, bool ok, const char* shape, bool written) {
    TORCH_CHECK_TYPE(t.scalar_type() == at::kDouble, op, ": `", what, "` must be float64 (got ", t.scalar_type(), ")");
    TORCH_CHECK_VALUE(ok && t.device() == like.device(), op, ": `", what, "` must be ", shape, " on ", like.device());
    TORCH_CHECK_VALUE(!written || t.is_contiguous(), op, ": `", what, "` is written in place and must be contiguous");
    return written ? t : t.detach().contiguous();
}
void opes_deposit_hip(at::Tensor centers_in, at::Tensor sigma_in, at::Tensor heights_in, at::Tensor state_in, const c10::optional<at::Tensor>& period_in,
                      const at::Tensor& new_centers_in, const at::Tensor& new_sigma_in, const at::Tensor& new_heights_in, double threshold,
                      double cutoff) {
    const char* const op = "molann::opes_deposit";
    TORCH_CHECK_VALUE(centers_in.dim() == 2 && centers_in.size(0) >= 1 && centers_in.size(1) >= 1 && centers_in.size(1) <= 8,
                      "molann::opes_deposit: `centers` must be [capacity >= 1, 1 <= d <= 8]");
    TORCH_CHECK_VALUE(std::isfinite(threshold) && threshold >= 0.0 && cutoff > 0.0,
                      "molann::opes_deposit: `threshold` must be finite and >= 0, `cutoff` > 0 (inf: none); got ", threshold, ", ", cutoff);
    const int64_t cap = centers_in.size(0), d = centers_in.size(1);
    const at::Tensor centers = opes_tensor(op, "centers", centers_in, centers_in, true, "[capacity, d]", true);
    const at::Tensor sigma = opes_tensor(op, "sigma", sigma_in, centers, sigma_in.dim() == 2 && sigma_in.size(0) == cap && sigma_in.size(1) == d,
                                            "[capacity, d]", true);
    const at::Tensor heights = opes_tensor(op, "heights", heights_in, centers, heights_in.dim() == 1 && heights_in.size(0) == cap, "[capacity]", true);
    const at::Tensor state = opes_tensor(op, "state", state_in, centers, state_in.dim() == 1 && state_in.size(0) == 4, "[4]", true);
    at::Tensor period;
    if (period_in.has_value() && period_in->defined())
        period = opes_tensor(op, "period", *period_in, centers, period_in->dim() == 1 && period_in->size(0) == d, "[d]", false);
    const at::Tensor new_centers = opes_tensor(op, "new_centers", new_centers_in, centers, new_centers_in.dim() == 2 && new_centers_in.size(1) == d,
                                                  "[W, d]", false);
    const int64_t n_new = new_centers.size(0);
    const at::Tensor new_sigma = opes_tensor(op, "new_sigma", new_sigma_in, centers,
                                                new_sigma_in.dim() == 2 && new_sigma_in.size(0) == n_new && new_sigma_in.size(1) == d, "[W, d]", false);
    const at::Tensor new_heights = opes_tensor(op, "new_heights", new_heights_in, centers, new_heights_in.dim() == 1 && new_heights_in.size(0) == n_new,
                                                  "[W]", false);
    if (n_new == 0) return;
    const c10::DeviceGuard guard(centers.device());
    hipStream_t stream = c10::hip::getCurrentHIPStream(centers.get_device()).stream();
    check(molann_opes_deposit_f64(centers.data_ptr<double>(), sigma.data_ptr<double>(), heights.data_ptr<double>(), cap, (int32_t)d,
                                  period.defined() ? period.data_ptr<double>() : nullptr, state.data_ptr<double>(), new_centers.data_ptr<double>(),
                                  new_sigma.data_ptr<double>(), new_heights.data_ptr<double>(), n_new, threshold, cutoff, stream),
          "molann_opes_deposit_f64");
}

// {out, bias, grad_x}: value_and_opes on a table whose live count and normalisation the kernel reads from `state` [4] in device memory
// (molann_value_and_opes_table_f64): centers [capacity, out_dim], heights [capacity], sigma [capacity, out_dim] are the table's storage,
// contiguous float64 on x's device and read where they are (no copy: a later deposit writes them); scale, epsilon and cutoff (inf: none)
// are host values, checked here as the C entry checks them.  `into`: none or {out, bias, grad_x}.
std::vector<at::Tensor> value_and_opes_table_impl(const at::Tensor& x_in, const std::vector<int64_t>& desc, const at::Tensor& ref_x,
                                                  const std::vector<at::Tensor>& weights, const std::vector<at::Tensor>& biases,
                                                  const at::Tensor& centers_in, const at::Tensor& heights_in, const at::Tensor& sigma_in,
                                                  const at::Tensor& state_in, const c10::optional<at::Tensor>& period_in, double scale, double epsilon,
                                                  double cutoff, const std::vector<at::Tensor>& into) {
    const char* const op = "molann::value_and_opes_table";
    check_x(x_in, desc);
    TORCH_CHECK_TYPE(x_in.scalar_type() == at::kDouble, "molann::value_and_opes_table is float64: call model.double() and pass a float64 x (got ",
                     x_in.scalar_type(), ")");
    TORCH_CHECK(desc[1] == KIND_FORWARD || desc[1] == KIND_FEATURES, "molann::value_and_opes_table: a forward or a features description");
    TORCH_CHECK_VALUE(std::isfinite(scale) && std::isfinite(epsilon) && epsilon > 0.0 && cutoff > 0.0,
                      "molann::value_and_opes_table: `scale` must be finite, `epsilon` finite and > 0, `cutoff` > 0 (inf: none); got ", scale, ", ",
                      epsilon, ", ", cutoff);
    const at::Tensor x = x_in.contiguous();
    const c10::DeviceGuard guard(x.device());
    auto e = entry_for(desc, x, ref_x);
    const int64_t n = x.size(0);
    const int64_t cols = e->kind == KIND_FORWARD ? e->out_dim : e->feature_dim;
    TORCH_CHECK_VALUE(centers_in.dim() == 2 && centers_in.size(0) >= 1 && centers_in.size(1) == cols,
                      "molann::value_and_opes_table: `centers` must be [capacity >= 1, out_dim]");
    const int64_t cap = centers_in.size(0);
    // `written`: the table is read where it lives, so it must be contiguous as it is
    const at::Tensor centers = opes_tensor(op, "centers", centers_in, x, true, "[capacity, out_dim]", true);
    const at::Tensor heights = opes_tensor(op, "heights", heights_in, x, heights_in.dim() == 1 && heights_in.size(0) == cap, "[capacity]", true);
    const at::Tensor sigma = opes_tensor(op, "sigma", sigma_in, x, sigma_in.dim() == 2 && sigma_in.size(0) == cap && sigma_in.size(1) == cols,
                                         "[capacity, out_dim]", true);
    const at::Tensor state = opes_tensor(op, "state", state_in, x, state_in.dim() == 1 && state_in.size(0) == 4, "[4]", true);
    at::Tensor period;
    if (period_in.has_value() && period_in->defined())
        period = opes_tensor(op, "period", *period_in, x, period_in->dim() == 1 && period_in->size(0) == cols, "[out_dim]", false);
    TORCH_CHECK(into.empty() || into.size() == 3, "molann::value_and_opes_table: `into` must be a triple of tensors (out, bias, grad_x)");
    at::Tensor out, bias, gx;
    if (into.empty()) {
        out = at::empty({n, cols}, x.options()); bias = at::empty({n}, x.options()); gx = at::empty_like(x);
    } else {
        out = into[0]; bias = into[1]; gx = into[2];
        const int64_t counts[3] = {n * cols, n, x.numel()};
        for (int i = 0; i < 3; ++i) {
            TORCH_CHECK_TYPE(into[i].scalar_type() == at::kDouble, "molann::value_and_opes_table: `into` must be float64 like x");
            TORCH_CHECK_VALUE(into[i].is_contiguous() && into[i].numel() == counts[i] && into[i].device() == x.device(),
                              "molann::value_and_opes_table: `into` must be contiguous {[N, out_dim], [N], [N, n_inp, 3]} on x's device");
        }
    }
    F64Linears lin;
    f64_linears(op, *e, x, weights, biases, lin, ": call .double()");
    std::lock_guard<std::mutex> lock(e->mu);
    TORCH_CHECK_NOT_IMPLEMENTED(molann_plan_supports_value_and_opes_table_f64(e->plan) == 1,
                                "molann::value_and_opes_table: more than 8 outputs, or one frame's rows exceed the LDS of a compute unit for this "
                                "model; use run, form the kernel sum, its logarithm and its derivative with torch, then value_and_vjp");
    if (n == 0) return {out, bias, gx};
    hipStream_t stream = c10::hip::getCurrentHIPStream(x.get_device()).stream();
    sync_live(*e, x, ref_x, weights, biases, stream);
    check(molann_value_and_opes_table_f64(e->plan, x.data_ptr<double>(), n, lin.W.data(), lin.B.data(), centers.data_ptr<double>(),
                                          heights.data_ptr<double>(), sigma.data_ptr<double>(), cap, state.data_ptr<double>(),
                                          period.defined() ? period.data_ptr<double>() : nullptr, scale, epsilon, cutoff, out.data_ptr<double>(),
                                          bias.data_ptr<double>(), gx.data_ptr<double>(), stream),
          "molann_value_and_opes_table_f64");
    return {out, bias, gx};
}
std::vector<at::Tensor> value_and_opes_table_hip(const at::Tensor& x_in, std::vector<int64_t> desc, const at::Tensor& ref_x, std::vector<at::Tensor> weights,
                                                 std::vector<at::Tensor> biases, const at::Tensor& centers, const at::Tensor& heights,
                                                 const at::Tensor& sigma, const at::Tensor& state, const c10::optional<at::Tensor>& period, double scale,
                                                 double epsilon, double cutoff, std::vector<at::Tensor> into) {
    return value_and_opes_table_impl(x_in, desc, ref_x, weights, biases, centers, heights, sigma, state, period, scale, epsilon, cutoff, into);
}
std::vector<at::Tensor> value_and_opes_table_h_hip(const at::Tensor& x_in, int64_t handle, const at::Tensor& ref_x, std::vector<at::Tensor> weights,
                                                   std::vector<at::Tensor> biases, const at::Tensor& centers, const at::Tensor& heights,
                                                   const at::Tensor& sigma, const at::Tensor& state, const c10::optional<at::Tensor>& period,
                                                   double scale, double epsilon, double cutoff, std::vector<at::Tensor> into) {
    return value_and_opes_table_impl(x_in, *desc_of(handle, "molann::value_and_opes_table_h"), ref_x, weights, biases, centers, heights, sigma, state,
                                     period, scale, epsilon, cutoff, into);
}

// A whole OPES step after the bias launch (molann_opes_step_f64): this step's kernels are formed from y [W, d] and V [W] on the device and
// compressed into the caller's table in place; `state` [4] and `run` [8] = (counter, sum_w, sum_w2, neff, sigma_scale, rct, 0, 0) are
// updated, in ONE launch on the current stream; nothing is read back.  The table as opes_deposit takes it; sigma0 [d], sigma_min [d] or none.
void opes_step_hip(at::Tensor centers_in, at::Tensor sigma_in, at::Tensor heights_in, at::Tensor state_in, at::Tensor run_in,
                   const c10::optional<at::Tensor>& period_in, const at::Tensor& y_in, const at::Tensor& V_in, const at::Tensor& sigma0_in,
                   const c10::optional<at::Tensor>& sigma_min_in, double beta, double threshold, double cutoff, bool fixed_sigma) {
    const char* const op = "molann::opes_step";
    TORCH_CHECK_VALUE(centers_in.dim() == 2 && centers_in.size(0) >= 1 && centers_in.size(1) >= 1 && centers_in.size(1) <= 8,
                      "molann::opes_step: `centers` must be [capacity >= 1, 1 <= d <= 8]");
    TORCH_CHECK_VALUE(std::isfinite(beta) && beta > 0.0 && std::isfinite(threshold) && threshold >= 0.0 && cutoff > 0.0,
                      "molann::opes_step: `beta` must be finite and > 0, `threshold` finite and >= 0, `cutoff` > 0 (inf: none); got ", beta, ", ",
                      threshold, ", ", cutoff);
    const int64_t cap = centers_in.size(0), d = centers_in.size(1);
    const at::Tensor centers = opes_tensor(op, "centers", centers_in, centers_in, true, "[capacity, d]", true);
    const at::Tensor sigma = opes_tensor(op, "sigma", sigma_in, centers, sigma_in.dim() == 2 && sigma_in.size(0) == cap && sigma_in.size(1) == d,
                                         "[capacity, d]", true);
    const at::Tensor heights = opes_tensor(op, "heights", heights_in, centers, heights_in.dim() == 1 && heights_in.size(0) == cap, "[capacity]", true);
    const at::Tensor state = opes_tensor(op, "state", state_in, centers, state_in.dim() == 1 && state_in.size(0) == 4, "[4]", true);
    const at::Tensor run = opes_tensor(op, "run", run_in, centers, run_in.dim() == 1 && run_in.size(0) == 8, "[8]", true);
    at::Tensor period, sigma_min;
    if (period_in.has_value() && period_in->defined())
        period = opes_tensor(op, "period", *period_in, centers, period_in->dim() == 1 && period_in->size(0) == d, "[d]", false);
    const at::Tensor y = opes_tensor(op, "y", y_in, centers, y_in.dim() == 2 && y_in.size(1) == d, "[W, d]", false);
    const int64_t n_walkers = y.size(0);
    const at::Tensor V = opes_tensor(op, "V", V_in, centers, V_in.dim() == 1 && V_in.size(0) == n_walkers, "[W]", false);
    const at::Tensor sigma0 = opes_tensor(op, "sigma0", sigma0_in, centers, sigma0_in.dim() == 1 && sigma0_in.size(0) == d, "[d]", false);
    if (sigma_min_in.has_value() && sigma_min_in->defined())
        sigma_min = opes_tensor(op, "sigma_min", *sigma_min_in, centers, sigma_min_in->dim() == 1 && sigma_min_in->size(0) == d, "[d]", false);
    if (n_walkers == 0) return;
    const c10::DeviceGuard guard(centers.device());
    hipStream_t stream = c10::hip::getCurrentHIPStream(centers.get_device()).stream();
    check(molann_opes_step_f64(centers.data_ptr<double>(), sigma.data_ptr<double>(), heights.data_ptr<double>(), cap, (int32_t)d,
                               period.defined() ? period.data_ptr<double>() : nullptr, state.data_ptr<double>(), run.data_ptr<double>(),
                               y.data_ptr<double>(), V.data_ptr<double>(), n_walkers, sigma0.data_ptr<double>(),
                               sigma_min.defined() ? sigma_min.data_ptr<double>() : nullptr, beta, threshold, cutoff, fixed_sigma ? 1 : 0, stream),
          "molann_opes_step_f64");
}

// The deposit step of a metadynamics run on a table (molann_metad_deposit_f64): the hills of the walkers y [W, n_out] (centres in `columns`;
// empty: the first table.dim()) with biases V [W] - a column of a wider tensor is read where it is - are added to `table` in place with
// heights height0 exp(-V inv_dT), and `state` [8] and `log` ([capacity, 2 d + 1] or none) are updated, in ONE launch on the current stream;
// nothing is read back.  lower, spacing, sigma: one float per axis; periodic: one bool per axis or empty; the scalars are checked here as
// the C entry checks them.
void metad_step_hip(at::Tensor table_in, at::Tensor state_in, const c10::optional<at::Tensor>& log_in, std::vector<double> lower,
                    std::vector<double> spacing, c10::List<bool> periodic, std::vector<double> sigma, std::vector<int64_t> columns,
                    const at::Tensor& y_in, const at::Tensor& V_in, double height0, double inv_dT, double cutoff) {
    const char* const op = "molann::metad_step";
    TORCH_CHECK_VALUE(table_in.dim() >= 1 && table_in.dim() <= 3, "molann::metad_step: `table` must have 1 to 3 dimensions");
    const int64_t d = table_in.dim();
    TORCH_CHECK_VALUE((int64_t)lower.size() == d && (int64_t)spacing.size() == d && (int64_t)sigma.size() == d &&
                          (periodic.size() == 0 || (int64_t)periodic.size() == d) && (columns.empty() || (int64_t)columns.size() == d),
                      "molann::metad_step: `lower`, `spacing`, `sigma` must have one entry per axis of `table` (", d,
                      "), `periodic` and `columns` that many or none");
    TORCH_CHECK_VALUE(std::isfinite(height0) && height0 > 0.0 && std::isfinite(inv_dT) && inv_dT >= 0.0 && cutoff > 0.0,
                      "molann::metad_step: `height0` must be finite and > 0, `inv_dT` finite and >= 0, `cutoff` > 0 (inf: none); got ", height0, ", ",
                      inv_dT, ", ", cutoff);
    const at::Tensor table = opes_tensor(op, "table", table_in, table_in, true, "[n_0, ...]", true);
    const at::Tensor state = opes_tensor(op, "state", state_in, table, state_in.dim() == 1 && state_in.size(0) == 8, "[8]", true);
    at::Tensor log;
    if (log_in.has_value() && log_in->defined())
        log = opes_tensor(op, "log", *log_in, table, log_in->dim() == 2 && log_in->size(1) == 2 * d + 1, "[capacity, 2 d + 1]", true);
    int64_t widest = d - 1;
    for (int64_t c : columns) {
        TORCH_CHECK_INDEX(c >= 0, "molann::metad_step: `columns` holds output indices >= 0");
        widest = std::max(widest, c);
    }
    TORCH_CHECK_TYPE(y_in.scalar_type() == at::kDouble && V_in.scalar_type() == at::kDouble, "molann::metad_step: `y` and `V` must be float64");
    TORCH_CHECK_VALUE(y_in.dim() == 2 && y_in.size(1) > widest && y_in.device() == table.device(), "molann::metad_step: `y` must be [W, more than ",
                      widest, " columns] on ", table.device());
    const int64_t n_walkers = y_in.size(0);
    TORCH_CHECK_VALUE(V_in.dim() == 1 && V_in.size(0) == n_walkers && V_in.device() == table.device(), "molann::metad_step: `V` must be [W] on ",
                      table.device());
    // read where they are: a row stride for y, an element stride for V (energies[:, 2] of value_and_bias)
    const at::Tensor y = y_in.stride(1) == 1 || y_in.size(1) == 1 ? y_in.detach() : y_in.detach().contiguous();
    const at::Tensor V = V_in.detach();
    if (n_walkers == 0) return;
    int64_t shape[3] = {4, 4, 4};
    int32_t per[3] = {0, 0, 0}, cols[3] = {0, 1, 2};
    for (int64_t k = 0; k < d; ++k) {
        shape[k] = table.size(k);
        per[k] = periodic.size() > 0 && periodic.get(k) ? 1 : 0;
        if (!columns.empty()) cols[k] = (int32_t)columns[k];
    }
    const c10::DeviceGuard guard(table.device());
    hipStream_t stream = c10::hip::getCurrentHIPStream(table.get_device()).stream();
    check(molann_metad_deposit_f64(table.data_ptr<double>(), (int32_t)d, shape, lower.data(), spacing.data(), per, sigma.data(), cols,
                                   y.data_ptr<double>(), n_walkers > 1 ? y.stride(0) : y.size(1), V.data_ptr<double>(), n_walkers > 1 ? V.stride(0) : 1,
                                   n_walkers, height0, inv_dT, cutoff, state.data_ptr<double>(), log.defined() ? log.data_ptr<double>() : nullptr,
                                   log.defined() ? log.size(0) : 0, stream),
          "molann_metad_deposit_f64");
}

// The reweighting offset c(t) of a metadynamics run (molann_metad_rct_f64): `table` (any shape, contiguous, read flat and read only) is reduced
// through `partials` [at least molann_metad_rct_chunks(table.numel()), 4] into `rct` [8], in TWO launches on the current stream, a chain; nothing
// is read back.  `state` [8] or none: with a state the device skips the update unless state[3] is a multiple of `stride`.  The scalars are
// checked here as the C entry checks them.
void metad_rct_hip(const at::Tensor& table_in, const c10::optional<at::Tensor>& state_in, at::Tensor partials_in, at::Tensor rct_in, double kT,
                   double inv_dT, int64_t stride) {
    const char* const op = "molann::metad_rct";
    TORCH_CHECK_VALUE(table_in.numel() >= 1 && table_in.numel() < ((int64_t)1 << 31), "molann::metad_rct: `table` must hold 1 to 2^31 - 1 entries");
    TORCH_CHECK_VALUE(std::isfinite(kT) && kT > 0.0 && std::isfinite(inv_dT) && inv_dT >= 0.0 && stride >= 1,
                      "molann::metad_rct: `kT` must be finite and > 0, `inv_dT` finite and >= 0, `stride` >= 1; got ", kT, ", ", inv_dT, ", ", stride);
    TORCH_CHECK_VALUE(table_in.is_contiguous(), "molann::metad_rct: `table` is read where it is and must be contiguous");
    const at::Tensor table = opes_tensor(op, "table", table_in, table_in, true, "[n_0, ...]", false);
    const int64_t rows = molann_metad_rct_chunks(table.numel());
    at::Tensor state;
    if (state_in.has_value() && state_in->defined())
        state = opes_tensor(op, "state", *state_in, table, state_in->dim() == 1 && state_in->size(0) == 8, "[8]", true);
    const at::Tensor partials =
        opes_tensor(op, "partials", partials_in, table, partials_in.dim() == 2 && partials_in.size(0) >= rows && partials_in.size(1) == 4,
                    "[at least ceil(table.numel() / 2048), 4]", true);
    const at::Tensor rct = opes_tensor(op, "rct", rct_in, table, rct_in.dim() == 1 && rct_in.size(0) == 8, "[8]", true);
    const c10::DeviceGuard guard(table.device());
    hipStream_t stream = c10::hip::getCurrentHIPStream(table.get_device()).stream();
    check(molann_metad_rct_f64(table.data_ptr<double>(), table.numel(), kT, inv_dT, state.defined() ? state.data_ptr<double>() : nullptr, stride,
                               partials.data_ptr<double>(), partials.size(0), rct.data_ptr<double>(), stream),
          "molann_metad_rct_f64");
}

// {P} or {P, dP}: the kernel density of an OPES table at points [M, d] and, with `with_grad`, its derivative [M, d] in ONE launch
// (molann_opes_kernel_sum_f64).  The table as value_and_opes takes it.
std::vector<at::Tensor> opes_kernel_sum_hip(const at::Tensor& points_in, const at::Tensor& centers_in, const at::Tensor& heights_in,
                                            const at::Tensor& sigma_in, const c10::optional<at::Tensor>& period_in, double cutoff, bool with_grad) {
    const char* const op = "molann::opes_kernel_sum";
    TORCH_CHECK_TYPE(points_in.scalar_type() == at::kDouble, "molann::opes_kernel_sum: `points` must be float64 (got ", points_in.scalar_type(), ")");
    TORCH_CHECK_VALUE(points_in.dim() == 2 && points_in.size(1) >= 1 && points_in.size(1) <= 8, "molann::opes_kernel_sum: `points` must be [M, 1 <= d <= 8]");
    TORCH_CHECK_VALUE(cutoff > 0.0, "molann::opes_kernel_sum: `cutoff` must be > 0 (inf: none); got ", cutoff);
    const at::Tensor points = points_in.detach().contiguous();
    const int64_t m = points.size(0), d = points.size(1);
    const at::Tensor centers = opes_tensor(op, "centers", centers_in, points, centers_in.dim() == 2 && centers_in.size(1) == d, "[H, d]", false);
    const int64_t n_kernels = centers.size(0);
    const at::Tensor heights = opes_tensor(op, "heights", heights_in, points, heights_in.dim() == 1 && heights_in.size(0) == n_kernels, "[H]", false);
    const bool per_kernel = sigma_in.dim() == 2 && sigma_in.size(0) == n_kernels && sigma_in.size(1) == d;
    const at::Tensor sigma = opes_tensor(op, "sigma", sigma_in, points, per_kernel || (sigma_in.dim() == 1 && sigma_in.size(0) == d), "[d] or [H, d]", false);
    at::Tensor period;
    if (period_in.has_value() && period_in->defined()) period = opes_tensor(op, "period", *period_in, points, period_in->dim() == 1 && period_in->size(0) == d, "[d]", false);
    at::Tensor P = at::empty({m}, points.options()), dP;
    if (with_grad) dP = at::empty({m, d}, points.options());
    if (m > 0) {
        const c10::DeviceGuard guard(points.device());
        hipStream_t stream = c10::hip::getCurrentHIPStream(points.get_device()).stream();
        check(molann_opes_kernel_sum_f64(points.data_ptr<double>(), m, (int32_t)d, n_kernels > 0 ? centers.data_ptr<double>() : nullptr,
                                         n_kernels > 0 ? heights.data_ptr<double>() : nullptr, n_kernels, n_kernels > 0 ? sigma.data_ptr<double>() : nullptr,
                                         per_kernel ? d : 0, period.defined() ? period.data_ptr<double>() : nullptr, cutoff, P.data_ptr<double>(),
                                         with_grad ? dP.data_ptr<double>() : nullptr, stream),
              "molann_opes_kernel_sum_f64");
    }
    if (with_grad) return {P, dP};
    return {P};
}

#define MOLANN_BIAS_OPES_OP_PARAMS                                                                                                                   \
    const at::Tensor &ref_x, std::vector<at::Tensor> weights, std::vector<at::Tensor> biases, const c10::optional<at::Tensor>&center,                \
        const c10::optional<at::Tensor>&kappa, const c10::optional<at::Tensor>&rperiod, const c10::optional<at::Tensor>&flat,                        \
        std::vector<int64_t> opes_columns, const at::Tensor &centers, const at::Tensor &heights, const at::Tensor &sigma,                            \
        const c10::optional<at::Tensor>&operiod, double scale, double norm, double epsilon, double cutoff, std::vector<int64_t> grid_columns,        \
        const c10::optional<at::Tensor>&table, std::vector<double> lower, std::vector<double> spacing, c10::List<bool> periodic,                     \
        std::vector<at::Tensor> into
#define MOLANN_BIAS_OPES_OP_ARGS                                                                                                                     \
    ref_x, weights, biases, center, kappa, rperiod, flat, opes_columns, centers, heights, sigma, operiod, scale, norm, epsilon, cutoff, grid_columns, \
        table, lower, spacing, periodic, into
std::vector<at::Tensor> value_and_bias_opes_hip(const at::Tensor& x_in, std::vector<int64_t> desc, MOLANN_BIAS_OPES_OP_PARAMS) {
    return value_and_bias_opes_impl(x_in, desc, MOLANN_BIAS_OPES_OP_ARGS);
}
std::vector<at::Tensor> value_and_bias_opes_h_hip(const at::Tensor& x_in, int64_t handle, MOLANN_BIAS_OPES_OP_PARAMS) {
    return value_and_bias_opes_impl(x_in, *desc_of(handle, "molann::value_and_bias_opes_h"), MOLANN_BIAS_OPES_OP_ARGS);
}

// {out, energies, grad_x}: value_and_bias_opes on a kernel table whose live count and normalisation the kernel reads from `state` [4] in
// device memory (molann_value_and_bias_opes_table_f64): centers [capacity, opes columns], heights [capacity], sigma [capacity, opes columns]
// are the table's storage, checked as value_and_opes_table checks them - contiguous float64 on x's device and read where they are (no copy:
// a later step writes them); the restraint and the grid as value_and_bias_opes takes them; scale, epsilon and cutoff (inf: none) are host
// values, checked here as the C entry checks them.  `into`: none or {out, energies, grad_x}.
std::vector<at::Tensor> value_and_bias_opes_table_impl(const at::Tensor& x_in, const std::vector<int64_t>& desc, const at::Tensor& ref_x,
                                                       const std::vector<at::Tensor>& weights, const std::vector<at::Tensor>& biases,
                                                       const c10::optional<at::Tensor>& center_in, const c10::optional<at::Tensor>& kappa_in,
                                                       const c10::optional<at::Tensor>& rperiod_in, const c10::optional<at::Tensor>& flat_in,
                                                       const std::vector<int64_t>& opes_columns, const at::Tensor& centers_in,
                                                       const at::Tensor& heights_in, const at::Tensor& sigma_in, const at::Tensor& state_in,
                                                       const c10::optional<at::Tensor>& operiod_in, double scale, double epsilon, double cutoff,
                                                       const std::vector<int64_t>& grid_columns, const c10::optional<at::Tensor>& table_in,
                                                       const std::vector<double>& lower, const std::vector<double>& spacing,
                                                       const c10::List<bool>& periodic_in, const std::vector<at::Tensor>& into) {
    const char* const op = "molann::value_and_bias_opes_table";
    check_x(x_in, desc);
    TORCH_CHECK_TYPE(x_in.scalar_type() == at::kDouble, "molann::value_and_bias_opes_table is float64: call model.double() and pass a float64 x (got ",
                     x_in.scalar_type(), ")");
    TORCH_CHECK(desc[1] == KIND_FORWARD || desc[1] == KIND_FEATURES, "molann::value_and_bias_opes_table: a forward or a features description");
    TORCH_CHECK_VALUE(std::isfinite(scale) && std::isfinite(epsilon) && epsilon > 0.0 && cutoff > 0.0,
                      "molann::value_and_bias_opes_table: `scale` must be finite, `epsilon` finite and > 0, `cutoff` > 0 (inf: none); got ", scale, ", ",
                      epsilon, ", ", cutoff);
    const at::Tensor x = x_in.contiguous();
    const c10::DeviceGuard guard(x.device());
    auto e = entry_for(desc, x, ref_x);
    const int64_t n = x.size(0);
    const int64_t cols = e->kind == KIND_FORWARD ? e->out_dim : e->feature_dim;
    const bool has_r = kappa_in.has_value() && kappa_in->defined(), has_g = !grid_columns.empty();
    TORCH_CHECK_VALUE(!opes_columns.empty(), "molann::value_and_bias_opes_table: `opes_columns` must name at least one output");
    const std::vector<int32_t> oc = bias_columns("opes_columns", opes_columns, 8, cols), gc = bias_columns("grid_columns", grid_columns, 3, cols);
    const int64_t dop = (int64_t)oc.size(), dg = (int64_t)gc.size();
    molann_bias_terms_f64 t;
    molann_opes_table_term_f64 o;
    memset(&t, 0, sizeof(t));
    memset(&o, 0, sizeof(o));
    at::Tensor center, kappa, rperiod, flat, table;
    if (has_r) {
        center = bias_tensor("center", center_in, x, true); kappa = bias_tensor("kappa", kappa_in, x, true);
        rperiod = bias_tensor("restraint_period", rperiod_in, x, false); flat = bias_tensor("flat", flat_in, x, false);
        const bool per_frame = center.dim() == 2 && center.size(0) == n && center.size(1) == cols;
        TORCH_CHECK_VALUE(per_frame || (center.dim() == 1 && center.size(0) == cols), "molann::value_and_bias_opes_table: `center` must be [", cols,
                          "] or [N, out_dim]");
        TORCH_CHECK_VALUE(kappa.dim() == 1 && kappa.size(0) == cols && (!rperiod.defined() || (rperiod.dim() == 1 && rperiod.size(0) == cols)) &&
                              (!flat.defined() || (flat.dim() == 1 && flat.size(0) == cols)),
                          "molann::value_and_bias_opes_table: `kappa`, `restraint_period` and `flat` must be [", cols, "]");
        t.center = center.data_ptr<double>(); t.center_stride = per_frame ? cols : 0; t.kappa = kappa.data_ptr<double>();
        t.restraint_period = rperiod.defined() ? rperiod.data_ptr<double>() : nullptr;
        t.flat = flat.defined() ? flat.data_ptr<double>() : nullptr;
    }
    TORCH_CHECK_VALUE(centers_in.dim() == 2 && centers_in.size(0) >= 1 && centers_in.size(1) == dop,
                      "molann::value_and_bias_opes_table: `centers` must be [capacity >= 1, opes columns]");
    const int64_t cap = centers_in.size(0);
    // `written`: the table is read where it lives, so it must be contiguous as it is
    const at::Tensor centers = opes_tensor(op, "centers", centers_in, x, true, "[capacity, opes columns]", true);
    const at::Tensor heights = opes_tensor(op, "heights", heights_in, x, heights_in.dim() == 1 && heights_in.size(0) == cap, "[capacity]", true);
    const at::Tensor sigma = opes_tensor(op, "sigma", sigma_in, x, sigma_in.dim() == 2 && sigma_in.size(0) == cap && sigma_in.size(1) == dop,
                                         "[capacity, opes columns]", true);
    const at::Tensor state = opes_tensor(op, "state", state_in, x, state_in.dim() == 1 && state_in.size(0) == 4, "[4]", true);
    at::Tensor operiod;
    if (operiod_in.has_value() && operiod_in->defined())
        operiod = opes_tensor(op, "period", *operiod_in, x, operiod_in->dim() == 1 && operiod_in->size(0) == dop, "[opes columns]", false);
    o.n_columns = (int32_t)dop; o.columns = oc.data(); o.capacity = cap;
    o.centers = centers.data_ptr<double>(); o.heights = heights.data_ptr<double>(); o.sigma = sigma.data_ptr<double>();
    o.state = state.data_ptr<double>(); o.period = operiod.defined() ? operiod.data_ptr<double>() : nullptr;
    o.scale = scale; o.epsilon = epsilon; o.cutoff = cutoff;
    int64_t shape[3] = {4, 4, 4};
    int32_t periodic[3] = {0, 0, 0};
    if (has_g) {
        table = bias_tensor("table", table_in, x, true);
        TORCH_CHECK_VALUE(table.dim() == dg && table_in->is_contiguous(), "molann::value_and_bias_opes_table: `table` must be contiguous with one "
                          "dimension per grid column (", dg, ")");
        TORCH_CHECK_VALUE((int64_t)lower.size() == dg && (int64_t)spacing.size() == dg && (periodic_in.size() == 0 || (int64_t)periodic_in.size() == dg),
                          "molann::value_and_bias_opes_table: `lower`, `spacing` and `periodic` must hold one value per grid column (", dg, ")");
        for (int64_t k = 0; k < dg; ++k) {
            shape[k] = table.size(k);
            TORCH_CHECK_VALUE(shape[k] >= 4, "molann::value_and_bias_opes_table: every dimension of `table` must have at least 4 points (got ", shape[k],
                              ")");
            TORCH_CHECK_VALUE(std::isfinite(spacing[k]) && spacing[k] > 0.0 && std::isfinite(lower[k]),
                              "molann::value_and_bias_opes_table: `spacing` must be finite and > 0 and `lower` finite");
            periodic[k] = periodic_in.size() > 0 && periodic_in.get(k) ? 1 : 0;
        }
        TORCH_CHECK_VALUE(table.numel() < (int64_t(1) << 31), "molann::value_and_bias_opes_table: `table` must hold fewer than 2^31 points");
        t.n_grid_columns = (int32_t)dg; t.grid_columns = gc.data(); t.table = table.data_ptr<double>();
        t.shape = shape; t.lower = lower.data(); t.spacing = spacing.data(); t.periodic = periodic;
    }
    TORCH_CHECK(into.empty() || into.size() == 3, "molann::value_and_bias_opes_table: `into` must be a triple of tensors (out, energies, grad_x)");
    at::Tensor out, energies, gx;
    if (into.empty()) {
        out = at::empty({n, cols}, x.options()); energies = at::empty({n, 4}, x.options()); gx = at::empty_like(x);
    } else {
        out = into[0]; energies = into[1]; gx = into[2];
        const int64_t counts[3] = {n * cols, 4 * n, x.numel()};
        for (int i = 0; i < 3; ++i) {
            TORCH_CHECK_TYPE(into[i].scalar_type() == at::kDouble, "molann::value_and_bias_opes_table: `into` must be float64 like x");
            TORCH_CHECK_VALUE(into[i].is_contiguous() && into[i].numel() == counts[i] && into[i].device() == x.device(),
                              "molann::value_and_bias_opes_table: `into` must be contiguous {[N, out_dim], [N, 4], [N, n_inp, 3]} on x's device");
        }
    }
    F64Linears lin;
    f64_linears(op, *e, x, weights, biases, lin, ": call .double()");
    std::lock_guard<std::mutex> lock(e->mu);
    TORCH_CHECK_NOT_IMPLEMENTED(molann_plan_supports_value_and_bias_opes_table_f64(e->plan) == 1,
                                "molann::value_and_bias_opes_table: one frame's rows exceed the LDS of a compute unit for this model; use run, form "
                                "the terms on the chosen columns with torch, then value_and_vjp");
    if (n == 0) return {out, energies, gx};
    hipStream_t stream = c10::hip::getCurrentHIPStream(x.get_device()).stream();
    sync_live(*e, x, ref_x, weights, biases, stream);
    check(molann_value_and_bias_opes_table_f64(e->plan, x.data_ptr<double>(), n, lin.W.data(), lin.B.data(), &t, &o, out.data_ptr<double>(),
                                               energies.data_ptr<double>(), gx.data_ptr<double>(), stream),
          "molann_value_and_bias_opes_table_f64");
    return {out, energies, gx};
}
#define MOLANN_BIAS_OPES_TABLE_OP_PARAMS                                                                                                             \
    const at::Tensor &ref_x, std::vector<at::Tensor> weights, std::vector<at::Tensor> biases, const c10::optional<at::Tensor>&center,                \
        const c10::optional<at::Tensor>&kappa, const c10::optional<at::Tensor>&rperiod, const c10::optional<at::Tensor>&flat,                        \
        std::vector<int64_t> opes_columns, const at::Tensor &centers, const at::Tensor &heights, const at::Tensor &sigma, const at::Tensor &state,   \
        const c10::optional<at::Tensor>&operiod, double scale, double epsilon, double cutoff, std::vector<int64_t> grid_columns,                     \
        const c10::optional<at::Tensor>&table, std::vector<double> lower, std::vector<double> spacing, c10::List<bool> periodic,                     \
        std::vector<at::Tensor> into
#define MOLANN_BIAS_OPES_TABLE_OP_ARGS                                                                                                               \
    ref_x, weights, biases, center, kappa, rperiod, flat, opes_columns, centers, heights, sigma, state, operiod, scale, epsilon, cutoff,             \
        grid_columns, table, lower, spacing, periodic, into
std::vector<at::Tensor> value_and_bias_opes_table_hip(const at::Tensor& x_in, std::vector<int64_t> desc, MOLANN_BIAS_OPES_TABLE_OP_PARAMS) {
    return value_and_bias_opes_table_impl(x_in, desc, MOLANN_BIAS_OPES_TABLE_OP_ARGS);
}
std::vector<at::Tensor> value_and_bias_opes_table_h_hip(const at::Tensor& x_in, int64_t handle, MOLANN_BIAS_OPES_TABLE_OP_PARAMS) {
    return value_and_bias_opes_table_impl(x_in, *desc_of(handle, "molann::value_and_bias_opes_table_h"), MOLANN_BIAS_OPES_TABLE_OP_ARGS);
}

// {out, energies, grad_x}: values, a parallel-bias metadynamics bias on the outputs `columns` and an optional restraint on all outputs
// (molann_value_and_pbmetad_f64): `table` holds the K one-dimensional tables back to back, contiguous float64 on x's device and read
// where it is (no copy: a later deposit writes it); shape, lower, spacing, periodic and kT are host values.  energies [N, 2 + K] =
// (E_r, V_PB, V_0 ..).  `into`: none or {out, energies, grad_x}.
std::vector<at::Tensor> value_and_pbmetad_impl(const at::Tensor& x_in, const std::vector<int64_t>& desc, const at::Tensor& ref_x,
                                               const std::vector<at::Tensor>& weights, const std::vector<at::Tensor>& biases,
                                               const c10::optional<at::Tensor>& center_in, const c10::optional<at::Tensor>& kappa_in,
                                               const c10::optional<at::Tensor>& rperiod_in, const c10::optional<at::Tensor>& flat_in,
                                               const std::vector<int64_t>& columns, const at::Tensor& table_in, const std::vector<int64_t>& shape,
                                               const std::vector<double>& lower, const std::vector<double>& spacing, const c10::List<bool>& periodic_in,
                                               double kT, const std::vector<at::Tensor>& into) {
    const char* const op = "molann::value_and_pbmetad";
    check_x(x_in, desc);
    TORCH_CHECK_TYPE(x_in.scalar_type() == at::kDouble, "molann::value_and_pbmetad is float64: call model.double() and pass a float64 x (got ",
                     x_in.scalar_type(), ")");
    TORCH_CHECK(desc[1] == KIND_FORWARD || desc[1] == KIND_FEATURES, "molann::value_and_pbmetad: a forward or a features description");
    TORCH_CHECK_VALUE(std::isfinite(kT) && kT > 0.0, "molann::value_and_pbmetad: `kT` must be finite and > 0; got ", kT);
    const at::Tensor x = x_in.contiguous();
    const c10::DeviceGuard guard(x.device());
    auto e = entry_for(desc, x, ref_x);
    const int64_t n = x.size(0);
    const int64_t cols = e->kind == KIND_FORWARD ? e->out_dim : e->feature_dim;
    const bool has_r = kappa_in.has_value() && kappa_in->defined();
    TORCH_CHECK_VALUE(!columns.empty(), "molann::value_and_pbmetad: `columns` must name at least one output");
    const std::vector<int32_t> pc = bias_columns("columns", columns, 8, cols);
    const int64_t K = (int64_t)pc.size();
    molann_pbmetad_terms_f64 t;
    memset(&t, 0, sizeof(t));
    at::Tensor center, kappa, rperiod, flat;
    if (has_r) {
        center = bias_tensor("center", center_in, x, true); kappa = bias_tensor("kappa", kappa_in, x, true);
        rperiod = bias_tensor("restraint_period", rperiod_in, x, false); flat = bias_tensor("flat", flat_in, x, false);
        const bool per_frame = center.dim() == 2 && center.size(0) == n && center.size(1) == cols;
        TORCH_CHECK_VALUE(per_frame || (center.dim() == 1 && center.size(0) == cols), "molann::value_and_pbmetad: `center` must be [", cols,
                          "] or [N, out_dim]");
        TORCH_CHECK_VALUE(kappa.dim() == 1 && kappa.size(0) == cols && (!rperiod.defined() || (rperiod.dim() == 1 && rperiod.size(0) == cols)) &&
                              (!flat.defined() || (flat.dim() == 1 && flat.size(0) == cols)),
                          "molann::value_and_pbmetad: `kappa`, `restraint_period` and `flat` must be [", cols, "]");
        t.center = center.data_ptr<double>(); t.center_stride = per_frame ? cols : 0; t.kappa = kappa.data_ptr<double>();
        t.restraint_period = rperiod.defined() ? rperiod.data_ptr<double>() : nullptr;
        t.flat = flat.defined() ? flat.data_ptr<double>() : nullptr;
    }
    TORCH_CHECK_VALUE((int64_t)shape.size() == K && (int64_t)lower.size() == K && (int64_t)spacing.size() == K &&
                          (periodic_in.size() == 0 || (int64_t)periodic_in.size() == K),
                      "molann::value_and_pbmetad: `shape`, `lower`, `spacing` and `periodic` must hold one value per column (", K, ")");
    int32_t periodic[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int64_t entries = 0;
    for (int64_t k = 0; k < K; ++k) {
        TORCH_CHECK_VALUE(shape[k] >= 4 && shape[k] < (int64_t(1) << 31), "molann::value_and_pbmetad: every table must have at least 4 points (got ",
                          shape[k], ")");
        TORCH_CHECK_VALUE(std::isfinite(spacing[k]) && spacing[k] > 0.0 && std::isfinite(lower[k]),
                          "molann::value_and_pbmetad: `spacing` must be finite and > 0 and `lower` finite");
        periodic[k] = periodic_in.size() > 0 && periodic_in.get(k) ? 1 : 0;
        entries += shape[k];
    }
    TORCH_CHECK_VALUE(entries < (int64_t(1) << 31), "molann::value_and_pbmetad: the tables must hold fewer than 2^31 points");
    // `written`: the table is read where it lives, so it must be contiguous as it is
    const at::Tensor table = opes_tensor(op, "table", table_in, x, table_in.numel() == entries, "sum(shape) values", true);
    t.n_columns = (int32_t)K; t.columns = pc.data(); t.table = table.data_ptr<double>();
    t.shape = shape.data(); t.lower = lower.data(); t.spacing = spacing.data(); t.periodic = periodic; t.kT = kT;
    TORCH_CHECK(into.empty() || into.size() == 3, "molann::value_and_pbmetad: `into` must be a triple of tensors (out, energies, grad_x)");
    at::Tensor out, energies, gx;
    if (into.empty()) {
        out = at::empty({n, cols}, x.options()); energies = at::empty({n, 2 + K}, x.options()); gx = at::empty_like(x);
    } else {
        out = into[0]; energies = into[1]; gx = into[2];
        const int64_t counts[3] = {n * cols, (2 + K) * n, x.numel()};
        for (int i = 0; i < 3; ++i) {
            TORCH_CHECK_TYPE(into[i].scalar_type() == at::kDouble, "molann::value_and_pbmetad: `into` must be float64 like x");
            TORCH_CHECK_VALUE(into[i].is_contiguous() && into[i].numel() == counts[i] && into[i].device() == x.device(),
                              "molann::value_and_pbmetad: `into` must be contiguous {[N, out_dim], [N, 2 + K], [N, n_inp, 3]} on x's device");
        }
    }
    F64Linears lin;
    f64_linears(op, *e, x, weights, biases, lin, ": call .double()");
    std::lock_guard<std::mutex> lock(e->mu);
    TORCH_CHECK_NOT_IMPLEMENTED(molann_plan_supports_value_and_pbmetad_f64(e->plan) == 1,
                                "molann::value_and_pbmetad: one frame's rows exceed the LDS of a compute unit for this model; use run, form the "
                                "K interpolants and their soft minimum with torch, then value_and_vjp");
    if (n == 0) return {out, energies, gx};
    hipStream_t stream = c10::hip::getCurrentHIPStream(x.get_device()).stream();
    sync_live(*e, x, ref_x, weights, biases, stream);
    check(molann_value_and_pbmetad_f64(e->plan, x.data_ptr<double>(), n, lin.W.data(), lin.B.data(), &t, out.data_ptr<double>(),
                                       energies.data_ptr<double>(), 2 + K, gx.data_ptr<double>(), stream),
          "molann_value_and_pbmetad_f64");
    return {out, energies, gx};
}
#define MOLANN_PBMETAD_OP_PARAMS                                                                                                                     \
    const at::Tensor &ref_x, std::vector<at::Tensor> weights, std::vector<at::Tensor> biases, const c10::optional<at::Tensor>&center,                \
        const c10::optional<at::Tensor>&kappa, const c10::optional<at::Tensor>&rperiod, const c10::optional<at::Tensor>&flat,                        \
        std::vector<int64_t> columns, const at::Tensor &table, std::vector<int64_t> shape, std::vector<double> lower, std::vector<double> spacing,   \
        c10::List<bool> periodic, double kT, std::vector<at::Tensor> into
#define MOLANN_PBMETAD_OP_ARGS ref_x, weights, biases, center, kappa, rperiod, flat, columns, table, shape, lower, spacing, periodic, kT, into
std::vector<at::Tensor> value_and_pbmetad_hip(const at::Tensor& x_in, std::vector<int64_t> desc, MOLANN_PBMETAD_OP_PARAMS) {
    return value_and_pbmetad_impl(x_in, desc, MOLANN_PBMETAD_OP_ARGS);
}
std::vector<at::Tensor> value_and_pbmetad_h_hip(const at::Tensor& x_in, int64_t handle, MOLANN_PBMETAD_OP_PARAMS) {
    return value_and_pbmetad_impl(x_in, *desc_of(handle, "molann::value_and_pbmetad_h"), MOLANN_PBMETAD_OP_ARGS);
}

// The fused forward that also keeps the features: {out, features} - or {out, empty} where the plan has no such twin of its
// kernel (molann_plan_backward_kind != 1 ... != 2 plans recompute in molann_backward_f32).  float32 fused plans.
std::vector<at::Tensor> run_train_hip(const at::Tensor& x_in, std::vector<int64_t> desc, const at::Tensor& ref_x, std::vector<at::Tensor> weights,
                                      std::vector<at::Tensor> biases) {
    check_x(x_in, desc);
    TORCH_CHECK(desc[1] == KIND_FORWARD && x_in.scalar_type() == at::kFloat, "molann::run_train: float32 forward plans only");
    const at::Tensor x = x_in.contiguous();
    const c10::DeviceGuard guard(x.device());
    auto e = entry_for(desc, x, ref_x);
    const int64_t n = x.size(0);
    at::Tensor out = at::empty({n, e->out_dim}, x.options());
    at::Tensor feat = at::empty({n, e->feature_dim}, x.options());
    if (n == 0) return {out, feat};
    hipStream_t stream = c10::hip::getCurrentHIPStream(x.get_device()).stream();
    std::lock_guard<std::mutex> lock(e->mu);
    sync_live(*e, x, ref_x, weights, biases, stream);
    const int rc = molann_forward_train_f32(e->plan, x.data_ptr<float>(), n, out.data_ptr<float>(), feat.data_ptr<float>(), stream);
    if (rc == MOLANN_E_UNSUPPORTED) {
        check(molann_forward_packed_f32(e->plan, x.data_ptr<float>(), n, out.data_ptr<float>(), stream), "molann_forward_packed_f32");
        return {out, at::empty({0}, x.options())};
    }
    check(rc, "molann_forward_train_f32");
    return {out, feat};
}

// flat parameter gradients (dW_l, db_l per layer) of the MLP alone, from the features run_train kept
at::Tensor run_backward_mlp_hip(const at::Tensor& feat, std::vector<int64_t> desc, const at::Tensor& ref_x, std::vector<at::Tensor> weights,
                                std::vector<at::Tensor> biases, const at::Tensor& grad_out) {
    TORCH_CHECK(desc.size() >= DESC_HEAD && desc[1] == KIND_FORWARD && feat.dim() == 2 && feat.scalar_type() == at::kFloat, "molann::run_backward_mlp: bad arguments");
    const at::Tensor f = feat.contiguous();
    const c10::DeviceGuard guard(f.device());
    auto e = entry_for(desc, f, ref_x);
    const int64_t n = f.size(0);
    TORCH_CHECK(f.size(1) == e->feature_dim, "molann::run_backward_mlp: features are [*, ", e->feature_dim, "], got ", f.sizes());
    at::Tensor g = grad_out.to(at::kFloat).reshape({n, e->out_dim}).contiguous();
    at::Tensor gp = at::zeros({molann_plan_grad_params_size(e->plan)}, f.options());
    if (n == 0) return gp;
    hipStream_t stream = c10::hip::getCurrentHIPStream(f.get_device()).stream();
    std::lock_guard<std::mutex> lock(e->mu);
    // (the parameters were packed by the forward of this step; a step that changed them in between repacks here)
    sync_live(*e, f, ref_x, weights, biases, stream);
    check(molann_mlp_backward_f32(e->plan, f.data_ptr<float>(), g.data_ptr<float>(), n, nullptr, gp.data_ptr<float>(), stream),
          "molann_mlp_backward_f32");
    return gp;
}

// {grad_x, flat parameter gradients} from the features run_train kept, for plans whose backward is the launches on kept features
// (molann_plan_backward_kind == 1: wave-per-frame preprocessing with a small head): the MLP's backward, then the preprocessing's
std::vector<at::Tensor> run_backward_kept_hip(const at::Tensor& x_in, const at::Tensor& feat, std::vector<int64_t> desc, const at::Tensor& ref_x,
                                              std::vector<at::Tensor> weights, std::vector<at::Tensor> biases, const at::Tensor& grad_out,
                                              bool need_x, bool need_params) {
    check_x(x_in, desc);
    TORCH_CHECK(desc[1] == KIND_FORWARD && x_in.scalar_type() == at::kFloat && feat.dim() == 2 && feat.scalar_type() == at::kFloat,
                "molann::run_backward_kept: float32 forward plans only");
    const at::Tensor x = x_in.contiguous();
    const at::Tensor f = feat.contiguous();
    const c10::DeviceGuard guard(x.device());
    auto e = entry_for(desc, x, ref_x);
    const int64_t n = x.size(0);
    TORCH_CHECK(f.size(0) == n && f.size(1) == e->feature_dim, "molann::run_backward_kept: features are [", n, ", ", e->feature_dim, "], got ", f.sizes());
    at::Tensor g = grad_out.to(at::kFloat).reshape({n, e->out_dim}).contiguous();
    at::Tensor gx = need_x ? at::empty_like(x) : at::empty({0}, x.options());
    at::Tensor gp = need_params ? at::zeros({molann_plan_grad_params_size(e->plan)}, x.options()) : at::empty({0}, x.options());
    if (n == 0) {
        if (need_x) gx.zero_();
        return {gx, gp};
    }
    at::Tensor gf = need_x ? at::empty_like(f) : at::empty({0}, f.options());
    hipStream_t stream = c10::hip::getCurrentHIPStream(x.get_device()).stream();
    std::lock_guard<std::mutex> lock(e->mu);
    sync_live(*e, x, ref_x, weights, biases, stream);
    check(molann_mlp_backward_f32(e->plan, f.data_ptr<float>(), g.data_ptr<float>(), n, need_x ? gf.data_ptr<float>() : nullptr,
                                  need_params ? gp.data_ptr<float>() : nullptr, stream),
          "molann_mlp_backward_f32");
    if (need_x)
        check(molann_features_backward_f32(e->plan, x.data_ptr<float>(), gf.data_ptr<float>(), n, gx.data_ptr<float>(), stream),
              "molann_features_backward_f32");
    return {gx, gp};
}

// molann_plan_backward_kind of the plan of `desc` on x's device: 2 one pass over x, 1 launches on kept features, 0 none
int64_t backward_kind(const at::Tensor& x, std::vector<int64_t> desc, const at::Tensor& ref_x) {
    check_x(x, desc);
    TORCH_CHECK(x.is_cuda(), "molann::backward_kind: x must be a device tensor");
    const c10::DeviceGuard guard(x.device());
    auto e = entry_for(desc, x, ref_x);
    std::lock_guard<std::mutex> lock(e->mu);
    return molann_plan_backward_kind(e->plan);
}

// 1 if the plan of `desc` on x's device has backward kernels (molann_plan_supports_backward), else 0
int64_t supports_backward(const at::Tensor& x, std::vector<int64_t> desc, const at::Tensor& ref_x) {
    check_x(x, desc);
    TORCH_CHECK(x.is_cuda(), "molann::supports_backward: x must be a device tensor");
    const c10::DeviceGuard guard(x.device());
    return molann_plan_supports_backward(entry_for(desc, x, ref_x)->plan) == 1 ? 1 : 0;
}

// name + geometry of the kernels the plan of (desc, device) launched last ("" before its first launch)
std::string launch_info(std::vector<int64_t> desc, int64_t device) {
    std::shared_ptr<Entry> e;
    {
        std::lock_guard<std::mutex> lock(g_cache_mu);
        auto it = g_cache.find(std::make_pair(desc, cache_device_key((int)device)));
        if (it == g_cache.end()) return "";
        e = it->second;
    }
    char buf[256];
    buf[0] = 0;
    std::lock_guard<std::mutex> lock(e->mu);
    molann_plan_last_launch_info(e->plan, buf, (int)sizeof(buf));
    return buf;
}

// every cached plan derived from this description on this device (the plan itself, its features-only and
// alignment-as-features variants share the head up to the instance id)
template <typename F>
void for_plans_of(const std::vector<int64_t>& desc, int64_t device, F f) {
    std::lock_guard<std::mutex> lock(g_cache_mu);
    for (auto it = g_cache.begin(); it != g_cache.end();) {
        const std::vector<int64_t>& d = it->first.first;
        const bool same_dev = (it->first.second & 0xffff) == (int)device;
        const bool same_model = d.size() >= DESC_HEAD && desc.size() >= DESC_HEAD && d[9] == desc[9] && d[2] == desc[2] &&
                                (d == desc || desc[9] != 0);
        if (same_dev && same_model) it = f(it);
        else ++it;
    }
}

// the live tensors of this model were written in a way their version counters do not show (`.data`): repack
void invalidate(std::vector<int64_t> desc, int64_t device) {
    for_plans_of(desc, device, [](std::map<CacheKey, std::shared_ptr<Entry>>::iterator it) {
        std::lock_guard<std::mutex> lock(it->second->mu);
        it->second->dirty = true;
        return ++it;
    });
}

// the model is gone: give its plans (device blobs, workspaces, code objects) back - except those a captured graph still
// launches through (they go when the graph unpins them and the LRU gets to them)
void release(std::vector<int64_t> desc, int64_t device) {
    for_plans_of(desc, device, [](std::map<CacheKey, std::shared_ptr<Entry>>::iterator it) {
        return it->second->pins > 0 ? ++it : g_cache.erase(it);
    });
}

// A HIP graph captured through molann::run holds raw pointers to the plan's packed weights, reference and code objects:
// the plans of this model stay in the cache while pinned.  Returns how many plans were pinned / unpinned.
int64_t pin(std::vector<int64_t> desc, int64_t device) {
    int64_t n = 0;
    for_plans_of(desc, device, [&n](std::map<CacheKey, std::shared_ptr<Entry>>::iterator it) { ++it->second->pins; ++n; return ++it; });
    return n;
}
int64_t unpin(std::vector<int64_t> desc, int64_t device) {
    int64_t n = 0;
    for_plans_of(desc, device, [&n](std::map<CacheKey, std::shared_ptr<Entry>>::iterator it) {
        if (it->second->pins > 0) { --it->second->pins; ++n; }
        return ++it;
    });
    { std::lock_guard<std::mutex> lock(g_cache_mu); evict_lru_locked(); }
    return n;
}

int64_t drop_plans() {
    std::lock_guard<std::mutex> lock(g_cache_mu);
    const int64_t n = (int64_t)g_cache.size();
    g_cache.clear();
    return n;
}

int64_t cached_plans() {
    std::lock_guard<std::mutex> lock(g_cache_mu);
    return (int64_t)g_cache.size();
}

at::Tensor call_run(const at::Tensor& x, const std::vector<int64_t>& desc, const at::Tensor& ref_x,
                    const std::vector<at::Tensor>& weights, const std::vector<at::Tensor>& biases) {
    static auto op = c10::Dispatcher::singleton()
                         .findSchemaOrThrow("molann::run", "")
                         .typed<at::Tensor(const at::Tensor&, std::vector<int64_t>, const at::Tensor&, std::vector<at::Tensor>,
                                           std::vector<at::Tensor>)>();
    return op.call(x, desc, ref_x, weights, biases);
}

std::vector<at::Tensor> call_run_backward(const at::Tensor& x, const std::vector<int64_t>& desc, const at::Tensor& ref_x,
                                          const std::vector<at::Tensor>& weights, const std::vector<at::Tensor>& biases,
                                          const at::Tensor& grad_out, bool need_x, bool need_params) {
    static auto op = c10::Dispatcher::singleton()
                         .findSchemaOrThrow("molann::run_backward", "")
                         .typed<std::vector<at::Tensor>(const at::Tensor&, std::vector<int64_t>, const at::Tensor&,
                                                        std::vector<at::Tensor>, std::vector<at::Tensor>, const at::Tensor&, bool, bool)>();
    return op.call(x, desc, ref_x, weights, biases, grad_out, need_x, need_params);
}

std::vector<at::Tensor> call_run_train(const at::Tensor& x, const std::vector<int64_t>& desc, const at::Tensor& ref_x,
                                       const std::vector<at::Tensor>& weights, const std::vector<at::Tensor>& biases) {
    static auto op = c10::Dispatcher::singleton()
                         .findSchemaOrThrow("molann::run_train", "")
                         .typed<std::vector<at::Tensor>(const at::Tensor&, std::vector<int64_t>, const at::Tensor&, std::vector<at::Tensor>,
                                                        std::vector<at::Tensor>)>();
    return op.call(x, desc, ref_x, weights, biases);
}

at::Tensor call_run_backward_mlp(const at::Tensor& feat, const std::vector<int64_t>& desc, const at::Tensor& ref_x,
                                 const std::vector<at::Tensor>& weights, const std::vector<at::Tensor>& biases, const at::Tensor& grad_out) {
    static auto op = c10::Dispatcher::singleton()
                         .findSchemaOrThrow("molann::run_backward_mlp", "")
                         .typed<at::Tensor(const at::Tensor&, std::vector<int64_t>, const at::Tensor&, std::vector<at::Tensor>, std::vector<at::Tensor>,
                                           const at::Tensor&)>();
    return op.call(feat, desc, ref_x, weights, biases, grad_out);
}

std::vector<at::Tensor> call_run_backward_kept(const at::Tensor& x, const at::Tensor& feat, const std::vector<int64_t>& desc, const at::Tensor& ref_x,
                                               const std::vector<at::Tensor>& weights, const std::vector<at::Tensor>& biases, const at::Tensor& grad_out,
                                               bool need_x, bool need_params) {
    static auto op = c10::Dispatcher::singleton()
                         .findSchemaOrThrow("molann::run_backward_kept", "")
                         .typed<std::vector<at::Tensor>(const at::Tensor&, const at::Tensor&, std::vector<int64_t>, const at::Tensor&, std::vector<at::Tensor>,
                                                        std::vector<at::Tensor>, const at::Tensor&, bool, bool)>();
    return op.call(x, feat, desc, ref_x, weights, biases, grad_out, need_x, need_params);
}

std::vector<int64_t> features_only(const std::vector<int64_t>& desc);
at::Tensor activation(int64_t code, const at::Tensor& t);

// ---- create_graph=True (round 3) ---------------------------------------------------------------------------------------------
// The kernels' gradients carry no graph.  When a backward runs under an enabled grad mode (the caller wants to differentiate the
// gradients again: a loss on forces; the reference gets that from autograd through its SVD, ann.py:188-197) the gradient is
// rebuilt as a DIFFERENTIABLE composition: the float64 features as a node (Features64Fn) whose backward - J(x)^T g, the float64
// kernel - is itself a node (FeatBackward64Fn) with a backward of its own, and the MLP as ATen ops on the live parameters.
// FeatBackward64Fn's backward needs, for a cotangent v on J^T g, d/dx [v . J(x)^T g] and d/dg [..] = J(x) v: directional
// derivatives along v of the first-order kernel's output and of the features, both exact from one launch of
// molann_features_hvp_f64.  Central differences of the float64 kernels remain for a plan that kernel refuses (none does), per frame
// with h = 6e-6 / |v|_max: a move of 6e-6 in the coordinates' own unit, set by the length scale of the geometry (bonds, angles,
// dihedrals, the aligned set) and not by where the frame sits in the box (molann_amd/ann.py: _difference_points is the same step in
// Python and says why).
struct FeatBackward64Fn : public torch::autograd::Function<FeatBackward64Fn> {
    static at::Tensor forward(torch::autograd::AutogradContext* ctx, const at::Tensor& x, const at::Tensor& g, std::vector<int64_t> desc,
                              const at::Tensor& ref_x) {
        at::AutoDispatchBelowADInplaceOrView below;
        ctx->save_for_backward({x, g, ref_x});
        ctx->saved_data["desc"] = desc;
        return call_run_backward(x, desc, ref_x, {}, {}, g, true, false)[0];
    }
    static torch::autograd::variable_list backward(torch::autograd::AutogradContext* ctx, torch::autograd::variable_list grad_outputs) {
        TORCH_CHECK(!at::GradMode::is_enabled(), "molann::run: gradients of order three are not available (the double backward is first-order itself)");
        const auto saved = ctx->get_saved_variables();
        const at::Tensor &x = saved[0], &g = saved[1], &ref_x = saved[2];
        const std::vector<int64_t> desc = ctx->saved_data["desc"].toIntVector();
        at::AutoDispatchBelowADInplaceOrView below;
        const at::Tensor v = grad_outputs[0].to(at::kDouble).contiguous();
        {   // exact, one launch: molann_features_hvp_f64 on the plan of desc in this library's cache (as run_backward finds it)
            const at::Tensor xc = x.contiguous(), gc = g.contiguous();
            const c10::DeviceGuard guard(xc.device());
            auto e = entry_for(desc[1] == KIND_ALIGN ? align_as_features(desc) : desc, xc, ref_x);
            at::Tensor hx = at::empty_like(xc), hg = at::empty_like(gc);
            int rc = MOLANN_OK;
            if (xc.size(0) > 0) {
                hipStream_t stream = c10::hip::getCurrentHIPStream(xc.get_device()).stream();
                std::lock_guard<std::mutex> lock(e->mu);
                sync_live(*e, xc, ref_x, {}, {}, stream);
                rc = molann_features_hvp_f64(e->plan, xc.data_ptr<double>(), gc.data_ptr<double>(), v.data_ptr<double>(), xc.size(0),
                                             hx.data_ptr<double>(), hg.data_ptr<double>(), stream);
            }
            if (rc != MOLANN_E_UNSUPPORTED) {
                check(rc, "molann_features_hvp_f64");
                return {ctx->needs_input_grad(0) ? hx : at::Tensor(), ctx->needs_input_grad(1) ? hg : at::Tensor(), at::Tensor(), at::Tensor()};
            }
        }
        // (central differences: only for a plan the exact kernel refuses - there is none)
        const at::Tensor vmax = v.abs().amax({1, 2}, true);
        const at::Tensor h = at::where(vmax > 0, 6e-6 / vmax.clamp_min(1e-300), at::zeros_like(vmax));
        const at::Tensor inv = at::where(h > 0, 0.5 / h.clamp_min(1e-300), at::zeros_like(h));
        const at::Tensor xp = (x + h * v).contiguous(), xm = (x - h * v).contiguous();
        at::Tensor gx, gg;
        if (ctx->needs_input_grad(0))
            gx = (call_run_backward(xp, desc, ref_x, {}, {}, g, true, false)[0] - call_run_backward(xm, desc, ref_x, {}, {}, g, true, false)[0]) * inv;
        if (ctx->needs_input_grad(1))
            gg = (call_run(xp, desc, ref_x, {}, {}) - call_run(xm, desc, ref_x, {}, {})) * inv.view({-1, 1});
        return {gx, gg, at::Tensor(), at::Tensor()};
    }
};

struct Features64Fn : public torch::autograd::Function<Features64Fn> {
    static at::Tensor forward(torch::autograd::AutogradContext* ctx, const at::Tensor& x, std::vector<int64_t> desc, const at::Tensor& ref_x) {
        at::AutoDispatchBelowADInplaceOrView below;
        ctx->save_for_backward({x, ref_x});
        ctx->saved_data["desc"] = desc;
        return call_run(x, desc, ref_x, {}, {});
    }
    static torch::autograd::variable_list backward(torch::autograd::AutogradContext* ctx, torch::autograd::variable_list grad_outputs) {
        const auto saved = ctx->get_saved_variables();
        const std::vector<int64_t> desc = ctx->saved_data["desc"].toIntVector();
        const at::Tensor g = grad_outputs[0].to(at::kDouble).contiguous();
        if (at::GradMode::is_enabled()) return {FeatBackward64Fn::apply(saved[0], g, desc, saved[1]), at::Tensor(), at::Tensor()};
        at::AutoDispatchBelowADInplaceOrView below;
        return {call_run_backward(saved[0], desc, saved[1], {}, {}, g, true, false)[0], at::Tensor(), at::Tensor()};
    }
};

// the gradients of a RunFunction node as a differentiable composition: [x, ref_x, weights..., biases...]
torch::autograd::variable_list double_backward(const at::Tensor& x, const std::vector<int64_t>& desc, const at::Tensor& ref_x,
                                               const std::vector<at::Tensor>& weights, const std::vector<at::Tensor>& biases,
                                               const at::Tensor& grad_out, const std::vector<bool>& need) {
    const int64_t nl = (int64_t)weights.size();
    const std::vector<int64_t> fdesc = desc[1] == KIND_FORWARD ? features_only(desc) : (desc[1] == KIND_ALIGN ? align_as_features(desc) : desc);
    const at::Tensor ref64 = ref_x.numel() > 0 ? ref_x.detach().to(at::kDouble) : ref_x;
    at::Tensor h = Features64Fn::apply(x.to(at::kDouble), fdesc, ref64).to(x.scalar_type());
    if (desc[1] == KIND_ALIGN) h = h.view_as(x);
    if (desc[1] == KIND_FORWARD)
        for (int64_t l = 0; l < nl; ++l) {
            h = at::linear(h, weights[l], biases[l]);
            if (l + 1 < nl) h = activation(desc[7], h);
        }
    std::vector<at::Tensor> inputs;
    std::vector<int64_t> where;
    if (need[0]) { inputs.push_back(x); where.push_back(0); }
    for (int64_t l = 0; l < nl; ++l) if (need[2 + l]) { inputs.push_back(weights[l]); where.push_back(3 + l); }
    for (int64_t l = 0; l < nl; ++l) if (need[2 + nl + l]) { inputs.push_back(biases[l]); where.push_back(3 + nl + l); }
    torch::autograd::variable_list out(3 + 2 * nl);
    if (inputs.empty()) return out;
    const auto got = torch::autograd::grad({h}, inputs, {grad_out.to(h.scalar_type())}, /*retain_graph=*/true, /*create_graph=*/true, /*allow_unused=*/true);
    for (size_t i = 0; i < got.size(); ++i) out[where[i]] = got[i];
    return out;
}

// forward = one launch of the plan, nothing but the inputs saved; backward = molann_backward_f32, which
// recomputes the forward per frame (first-order only: the backward is not itself differentiable)
struct RunFunction : public torch::autograd::Function<RunFunction> {
    // apply() records one graph edge per at::Tensor / at::TensorList element and none for `desc`
    static at::Tensor forward(torch::autograd::AutogradContext* ctx, const at::Tensor& x, std::vector<int64_t> desc,
                              const at::Tensor& ref_x, at::TensorList weights, at::TensorList biases) {
        at::AutoDispatchBelowADInplaceOrView below;
        // What the backward will need is known here.  Gradients for x: molann_backward_f32 is one pass over x that
        // recomputes everything, nothing to keep.  Parameters only (x is data): the MLP's backward alone, on the features
        // this forward keeps - no second pass over x.
        at::Tensor out, feat;
        // (x wants a gradient too: kept features still pay where the backward is launches on them anyway - backward kind 1, a small
        // head behind the wave-per-frame kernels - instead of a recompute of the features inside molann_backward_f32)
        bool keep = desc.size() >= DESC_HEAD && desc[1] == KIND_FORWARD && x.scalar_type() == at::kFloat && x.is_cuda();
        if (keep && x.requires_grad()) keep = x.size(0) > 0 && backward_kind(x, desc, ref_x) == 1;
        if (keep) {
            std::vector<at::Tensor> r = call_run_train(x, desc, ref_x, weights.vec(), biases.vec());
            out = r[0];
            if (r[1].numel() > 0 || x.size(0) == 0) feat = r[1];
        } else {
            out = call_run(x, desc, ref_x, weights.vec(), biases.vec());
        }
        std::vector<at::Tensor> saved = {x, ref_x};
        for (auto& w : weights) saved.push_back(w);
        for (auto& b : biases) saved.push_back(b);
        if (feat.defined()) saved.push_back(feat);
        ctx->save_for_backward(saved);
        ctx->saved_data["desc"] = desc;
        ctx->saved_data["n_layers"] = (int64_t)weights.size();
        ctx->saved_data["kept_features"] = feat.defined();
        return out;
    }

    static torch::autograd::variable_list backward(torch::autograd::AutogradContext* ctx, torch::autograd::variable_list grad_outputs) {
        // grad mode is on inside a backward only under create_graph=True: the caller wants to differentiate these gradients
        // again.  molann_backward_f32 is a kernel, its result has no graph: the gradient is then rebuilt as a differentiable
        // composition (double_backward above).
        if (at::GradMode::is_enabled()) {
            const auto sv = ctx->get_saved_variables();
            const int64_t n = ctx->saved_data["n_layers"].toInt();
            std::vector<at::Tensor> w(sv.begin() + 2, sv.begin() + 2 + n), b(sv.begin() + 2 + n, sv.begin() + 2 + 2 * n);
            std::vector<bool> need(2 + 2 * n);
            for (int64_t i = 0; i < 2 + 2 * n; ++i) need[(size_t)i] = ctx->needs_input_grad((size_t)i);
            return double_backward(sv[0], ctx->saved_data["desc"].toIntVector(), sv[1], w, b, grad_outputs[0], need);
        }
        const auto saved = ctx->get_saved_variables();
        const std::vector<int64_t> desc = ctx->saved_data["desc"].toIntVector();
        const int64_t nl = ctx->saved_data["n_layers"].toInt();
        const at::Tensor& x = saved[0];
        const at::Tensor& ref_x = saved[1];
        std::vector<at::Tensor> weights(saved.begin() + 2, saved.begin() + 2 + nl), biases(saved.begin() + 2 + nl, saved.begin() + 2 + 2 * nl);
        // graph edges (tensors only): x, ref_x, weights..., biases...; returned list (all inputs): x, desc, ref_x, ...
        const bool need_x = ctx->needs_input_grad(0);
        bool need_p = false;
        for (int64_t i = 0; i < 2 * nl; ++i) need_p = need_p || ctx->needs_input_grad(2 + i);
        std::vector<at::Tensor> g;
        {
            at::AutoDispatchBelowADInplaceOrView below;
            if (ctx->saved_data["kept_features"].toBool() && !need_x) {
                g = {at::Tensor(), need_p ? call_run_backward_mlp(saved[2 + 2 * nl], desc, ref_x, weights, biases, grad_outputs[0]) : at::Tensor()};
            } else if (ctx->saved_data["kept_features"].toBool() && backward_kind(x, desc, ref_x) == 1) {
                g = call_run_backward_kept(x, saved[2 + 2 * nl], desc, ref_x, weights, biases, grad_outputs[0], need_x, need_p);
            } else {
                g = call_run_backward(x, desc, ref_x, weights, biases, grad_outputs[0], need_x, need_p);
            }
        }
        torch::autograd::variable_list out(3 + 2 * nl);
        if (need_x) out[0] = g[0];
        if (need_p) {
            int64_t off = 0;
            for (int64_t l = 0; l < nl; ++l) { // flat layout: dW_l[J][K] then db_l[J], layer after layer
                const int64_t nw = weights[l].numel(), nb = biases[l].numel();
                if (ctx->needs_input_grad(2 + l)) out[3 + l] = g[1].narrow(0, off, nw).view(weights[l].sizes());
                if (ctx->needs_input_grad(2 + nl + l)) out[3 + nl + l] = g[1].narrow(0, off + nw, nb).view(biases[l].sizes());
                off += nw + nb;
            }
        }
        return out;
    }
};

// The head of a forward plan whose backward is two nodes - the preprocessing's, then this one: a wide fp32 head that
// molann_mlp_backward_f32 serves (molann_plan_supports_mlp_backward) where molann_plan_supports_backward does not.  Forward
// molann_mlp_packed_f32 on the features, backward molann_mlp_backward_f32 on the same features; the parameters are repacked
// whenever the live tensors changed (sync_live), so an optimiser's in-place step is seen by the next forward.
at::Tensor activation(int64_t code, const at::Tensor& t);
struct HeadFunction : public torch::autograd::Function<HeadFunction> {
    static at::Tensor forward(torch::autograd::AutogradContext* ctx, const at::Tensor& feat, std::vector<int64_t> desc, const at::Tensor& ref_x,
                              at::TensorList weights, at::TensorList biases) {
        at::AutoDispatchBelowADInplaceOrView below;
        TORCH_CHECK(feat.dim() == 2 && feat.scalar_type() == at::kFloat && feat.is_cuda(), "molann::run_head: float32 device features [N, D] only");
        const at::Tensor f = feat.contiguous();
        const c10::DeviceGuard guard(f.device());
        auto e = entry_for(desc, f, ref_x);
        TORCH_CHECK(e->kind == KIND_FORWARD && f.size(1) == e->feature_dim, "molann::run_head: features are [*, ", e->feature_dim, "], got ", f.sizes());
        const int64_t n = f.size(0);
        at::Tensor out = at::empty({n, e->out_dim}, f.options());
        {
            hipStream_t stream = c10::hip::getCurrentHIPStream(f.get_device()).stream();
            std::lock_guard<std::mutex> lock(e->mu);
            sync_live(*e, f, ref_x, weights.vec(), biases.vec(), stream);
            if (n > 0) check(molann_mlp_packed_f32(e->plan, f.data_ptr<float>(), n, out.data_ptr<float>(), stream), "molann_mlp_packed_f32");
        }
        std::vector<at::Tensor> saved = {feat, ref_x};
        for (auto& w : weights) saved.push_back(w);
        for (auto& b : biases) saved.push_back(b);
        ctx->save_for_backward(saved);
        ctx->saved_data["desc"] = desc;
        ctx->saved_data["n_layers"] = (int64_t)weights.size();
        return out;
    }

    static torch::autograd::variable_list backward(torch::autograd::AutogradContext* ctx, torch::autograd::variable_list grad_outputs) {
        const auto sv = ctx->get_saved_variables();
        const std::vector<int64_t> desc = ctx->saved_data["desc"].toIntVector();
        const int64_t nl = ctx->saved_data["n_layers"].toInt();
        const at::Tensor& f = sv[0];
        const at::Tensor& ref_x = sv[1];
        std::vector<at::Tensor> weights(sv.begin() + 2, sv.begin() + 2 + nl), biases(sv.begin() + 2 + nl, sv.begin() + 2 + 2 * nl);
        // graph edges: feat, ref_x, weights..., biases...; returned list (all inputs): feat, desc, ref_x, weights..., biases...
        torch::autograd::variable_list out(3 + 2 * nl);
        const bool need_f = ctx->needs_input_grad(0);
        bool need_p = false;
        for (int64_t i = 0; i < 2 * nl; ++i) need_p = need_p || ctx->needs_input_grad(2 + i);
        if (at::GradMode::is_enabled()) {
            // create_graph=True: the head rebuilt as ATen ops on the live parameters (and the features with their own graph),
            // differentiated with a graph
            std::vector<at::Tensor> inputs;
            std::vector<size_t> slot;
            if (need_f) { inputs.push_back(f); slot.push_back(0); }
            for (int64_t l = 0; l < 2 * nl; ++l)
                if (ctx->needs_input_grad(2 + l)) { inputs.push_back(l < nl ? weights[l] : biases[l - nl]); slot.push_back(3 + l); }
            if (inputs.empty()) return out;
            at::Tensor h = f;
            for (int64_t l = 0; l < nl; ++l) {
                h = at::linear(h, weights[l], biases[l]);
                if (l + 1 < nl) h = activation(desc[7], h);
            }
            const auto g = torch::autograd::grad({h}, inputs, {grad_outputs[0]}, /*retain_graph=*/true, /*create_graph=*/true, /*allow_unused=*/true);
            for (size_t i = 0; i < g.size(); ++i) out[slot[i]] = g[i];
            return out;
        }
        if (!need_f && !need_p) return out;
        const at::Tensor fc = f.contiguous();
        const int64_t n = fc.size(0);
        const c10::DeviceGuard guard(fc.device());
        auto e = entry_for(desc, fc, ref_x);
        at::Tensor g = grad_outputs[0].to(at::kFloat).reshape({n, e->out_dim}).contiguous();
        at::Tensor gf = need_f ? at::empty_like(fc) : at::Tensor();
        at::Tensor gp = need_p ? at::zeros({molann_plan_grad_params_size(e->plan)}, fc.options()) : at::Tensor();
        if (n > 0) {
            hipStream_t stream = c10::hip::getCurrentHIPStream(fc.get_device()).stream();
            std::lock_guard<std::mutex> lock(e->mu);
            sync_live(*e, fc, ref_x, weights, biases, stream);
            check(molann_mlp_backward_f32(e->plan, fc.data_ptr<float>(), g.data_ptr<float>(), n, need_f ? gf.data_ptr<float>() : nullptr,
                                          need_p ? gp.data_ptr<float>() : nullptr, stream),
                  "molann_mlp_backward_f32");
        }
        if (need_f) out[0] = gf;
        if (need_p) {
            int64_t off = 0;
            for (int64_t l = 0; l < nl; ++l) { // flat layout: dW_l[J][K] then db_l[J], layer after layer
                const int64_t nw = weights[l].numel(), nb = biases[l].numel();
                if (ctx->needs_input_grad(2 + l)) out[3 + l] = gp.narrow(0, off, nw).view(weights[l].sizes());
                if (ctx->needs_input_grad(2 + nl + l)) out[3 + nl + l] = gp.narrow(0, off + nw, nb).view(biases[l].sizes());
                off += nw + nb;
            }
        }
        return out;
    }
};

// whether the head of `desc` runs as HeadFunction under autograd (float32 device input, a forward plan)
bool head_node(const std::vector<int64_t>& desc, const at::Tensor& x, const at::Tensor& ref_x) {
    const c10::DeviceGuard guard(x.device());
    auto e = entry_for(desc, x, ref_x);
    return molann_plan_supports_mlp_backward(e->plan) == 1;
}

// molann::run_head: the head node on features the caller computed (MolANN.forward: its preprocessing layer's output)
at::Tensor run_head(const at::Tensor& feat, std::vector<int64_t> desc, const at::Tensor& ref_x, std::vector<at::Tensor> weights,
                    std::vector<at::Tensor> biases) {
    TORCH_CHECK(desc.size() >= DESC_HEAD && desc[1] == KIND_FORWARD, "molann::run_head: a forward descriptor");
    return HeadFunction::apply(feat, desc, ref_x, at::TensorList(weights), at::TensorList(biases));
}

int64_t supports_mlp_backward(const at::Tensor& x, std::vector<int64_t> desc, const at::Tensor& ref_x) {
    TORCH_CHECK(x.is_cuda(), "molann::supports_mlp_backward: x must be a device tensor");
    return head_node(desc, x, ref_x) ? 1 : 0;
}

// the plan of `desc` without its MLP (what PreprocessingANN.forward launches)
std::vector<int64_t> features_only(const std::vector<int64_t>& desc) {
    const int64_t n_layers = desc[6];
    std::vector<int64_t> v(desc.begin(), desc.end() - (n_layers > 0 ? n_layers + 1 : 0));
    v[1] = KIND_FEATURES;
    v[6] = 0;
    return v;
}

at::Tensor activation(int64_t code, const at::Tensor& t) {
    switch (code) {
    case MOLANN_ACT_TANH: return at::tanh(t);
    case MOLANN_ACT_RELU: return at::relu(t);
    case MOLANN_ACT_SIGMOID: return at::sigmoid(t);
    case MOLANN_ACT_IDENTITY: return t;
    case MOLANN_ACT_ELU: return at::elu(t);
    case MOLANN_ACT_SILU: return at::silu(t);
    case MOLANN_ACT_SOFTPLUS: return at::softplus(t);
    case MOLANN_ACT_LEAKY_RELU: return at::leaky_relu(t, 0.01);
    case MOLANN_ACT_GELU: return at::gelu(t);
    default: TORCH_CHECK(false, "molann::run: unknown activation code ", code);
    }
}

// a forward-mode tangent (torch.autograd.forward_ad dual, torch.func.jvp / jacfwd: both at forward-AD level 0)
bool has_tangent(const at::Tensor& t) { return t.defined() && t._fw_grad(/*level=*/0).defined(); }

at::Tensor run_autograd(const at::Tensor& x, std::vector<int64_t> desc, const at::Tensor& ref_x, std::vector<at::Tensor> weights,
                        std::vector<at::Tensor> biases) {
    // molann::run has no forward-mode derivative: without this check a float64 dual went below autograd and came back as the
    // primal with no tangent, and a float32 one failed inside torch's C++ custom-Function machinery
    bool tangent = has_tangent(x) || has_tangent(ref_x);
    for (const auto& w : weights) tangent = tangent || has_tangent(w);
    for (const auto& b : biases) tangent = tangent || has_tangent(b);
    TORCH_CHECK(!tangent, "molann::run (a torch.jit.script'ed molann_amd module) has no forward-mode derivative: run "
                "torch.autograd.forward_ad / torch.func.jvp / jacfwd on the eager molann_amd module instead");
    if (x.scalar_type() == at::kDouble) {
        // float64 (`model.double()`): gradients for the preprocessing come from molann_features_backward_f64; the MLP of a
        // float64 model under grad mode is ATen's (its parameters are read as they are anyway)
        bool needs = at::GradMode::is_enabled() && x.requires_grad();
        for (const auto& w : weights) needs = needs || (at::GradMode::is_enabled() && w.requires_grad());
        for (const auto& b : biases) needs = needs || (at::GradMode::is_enabled() && b.requires_grad());
        if (!needs) {
            at::AutoDispatchBelowADInplaceOrView below;
            return call_run(x, desc, ref_x, weights, biases);
        }
        if (desc.size() >= DESC_HEAD && desc[1] == KIND_FORWARD) {
            at::Tensor h = call_run(x, features_only(desc), ref_x, {}, {});
            for (size_t l = 0; l < weights.size(); ++l) {
                h = at::linear(h, weights[l], biases[l]);
                if (l + 1 < weights.size()) h = activation(desc[7], h);
            }
            return h;
        }
        return RunFunction::apply(x, desc, ref_x, at::TensorList(weights), at::TensorList(biases));
    }
    // A fused plan without a backward kernel (MLP wider than 32, large frames, ELU / GELU / Softplus) that has to
    // record gradients: features and their gradient from the kernels (the plan without the MLP), the MLP as ATen
    // ops - the composition molann_amd/ann.py: MolANN.forward uses in the same situation.
    if (desc.size() >= DESC_HEAD && desc[1] == KIND_FORWARD && at::GradMode::is_enabled() && x.is_cuda()) {
        bool needs = x.requires_grad();
        for (const auto& w : weights) needs = needs || w.requires_grad();
        for (const auto& b : biases) needs = needs || b.requires_grad();
        if (needs) {
            check_x(x, desc);
            bool fused_backward;
            {
                const c10::DeviceGuard guard(x.device());
                fused_backward = molann_plan_supports_backward(entry_for(desc, x, ref_x)->plan) == 1;
            }
            if (!fused_backward && x.scalar_type() == at::kFloat && head_node(desc, x, ref_x)) {
                // the preprocessing's node (its HIP backward), then the head's (molann_chain_bwd)
                at::Tensor f = call_run(x, features_only(desc), ref_x, {}, {});
                return HeadFunction::apply(f, desc, ref_x, at::TensorList(weights), at::TensorList(biases));
            }
            if (!fused_backward) {
                at::Tensor h = call_run(x, features_only(desc), ref_x, {}, {});
                for (size_t l = 0; l < weights.size(); ++l) {
                    h = at::linear(h, weights[l], biases[l]);
                    if (l + 1 < weights.size()) h = activation(desc[7], h);
                }
                return h;
            }
        }
    }
    return RunFunction::apply(x, desc, ref_x, at::TensorList(weights), at::TensorList(biases));
}

} // namespace

TORCH_LIBRARY(molann, m) {
    m.def("run(Tensor x, int[] desc, Tensor ref_x, Tensor[] weights, Tensor[] biases) -> Tensor");
    m.def("run_backward(Tensor x, int[] desc, Tensor ref_x, Tensor[] weights, Tensor[] biases, Tensor grad_out, bool need_x, "
          "bool need_params) -> Tensor[]");
    m.def("run_train(Tensor x, int[] desc, Tensor ref_x, Tensor[] weights, Tensor[] biases) -> Tensor[]");
    m.def("run_backward_mlp(Tensor feat, int[] desc, Tensor ref_x, Tensor[] weights, Tensor[] biases, Tensor grad_out) -> Tensor");
    m.def("run_backward_kept(Tensor x, Tensor feat, int[] desc, Tensor ref_x, Tensor[] weights, Tensor[] biases, Tensor grad_out, bool need_x, "
          "bool need_params) -> Tensor[]");
    m.def("backward_kind(Tensor x, int[] desc, Tensor ref_x) -> int", backward_kind);
    m.def("register_desc(int[] desc) -> int", register_desc);
    m.def("run_h(Tensor x, int handle, Tensor ref_x, Tensor[] weights, Tensor[] biases) -> Tensor");
    m.def("value_and_vjp_h(Tensor x, int handle, Tensor ref_x, Tensor[] weights, Tensor[] biases, Tensor grad_out, Tensor[] into) -> Tensor[]");
    m.def("value_and_vjp(Tensor x, int[] desc, Tensor ref_x, Tensor[] weights, Tensor[] biases, Tensor grad_out, Tensor[] into) -> Tensor[]");
    m.def("value_and_jacobian_h(Tensor x, int handle, Tensor ref_x, Tensor[] weights, Tensor[] biases, Tensor[] into) -> Tensor[]");
    m.def("value_and_jacobian(Tensor x, int[] desc, Tensor ref_x, Tensor[] weights, Tensor[] biases, Tensor[] into) -> Tensor[]");
    m.def("value_and_metric_h(Tensor x, int handle, Tensor ref_x, Tensor[] weights, Tensor[] biases, Tensor? atom_w, Tensor[] into) -> Tensor[]");
    m.def("value_and_restraint_h(Tensor x, int handle, Tensor ref_x, Tensor[] weights, Tensor[] biases, Tensor center, Tensor kappa, Tensor? period, "
          "Tensor? flat, Tensor[] into) -> Tensor[]");
    m.def("value_and_restraint(Tensor x, int[] desc, Tensor ref_x, Tensor[] weights, Tensor[] biases, Tensor center, Tensor kappa, Tensor? period, "
          "Tensor? flat, Tensor[] into) -> Tensor[]");
    m.def("value_and_hills_h(Tensor x, int handle, Tensor ref_x, Tensor[] weights, Tensor[] biases, Tensor centers, Tensor heights, Tensor sigma, "
          "Tensor? period, Tensor[] into) -> Tensor[]");
    m.def("value_and_hills(Tensor x, int[] desc, Tensor ref_x, Tensor[] weights, Tensor[] biases, Tensor centers, Tensor heights, Tensor sigma, "
          "Tensor? period, Tensor[] into) -> Tensor[]");
    m.def("value_and_opes_h(Tensor x, int handle, Tensor ref_x, Tensor[] weights, Tensor[] biases, Tensor centers, Tensor heights, Tensor sigma, "
          "Tensor? period, float scale, float norm, float epsilon, float cutoff, Tensor[] into) -> Tensor[]");
    m.def("value_and_opes(Tensor x, int[] desc, Tensor ref_x, Tensor[] weights, Tensor[] biases, Tensor centers, Tensor heights, Tensor sigma, "
          "Tensor? period, float scale, float norm, float epsilon, float cutoff, Tensor[] into) -> Tensor[]");
    m.def("value_and_grid_h(Tensor x, int handle, Tensor ref_x, Tensor[] weights, Tensor[] biases, Tensor table, float[] lower, float[] spacing, "
          "bool[] periodic, Tensor[] into) -> Tensor[]");
    m.def("value_and_grid(Tensor x, int[] desc, Tensor ref_x, Tensor[] weights, Tensor[] biases, Tensor table, float[] lower, float[] spacing, "
          "bool[] periodic, Tensor[] into) -> Tensor[]");
    m.def("value_and_bias_h(Tensor x, int handle, Tensor ref_x, Tensor[] weights, Tensor[] biases, Tensor? center, Tensor? kappa, Tensor? restraint_period, "
          "Tensor? flat, int[] hills_columns, Tensor? centers, Tensor? heights, Tensor? sigma, Tensor? hills_period, int[] grid_columns, Tensor? table, "
          "float[] lower, float[] spacing, bool[] periodic, Tensor[] into) -> Tensor[]");
    m.def("value_and_bias(Tensor x, int[] desc, Tensor ref_x, Tensor[] weights, Tensor[] biases, Tensor? center, Tensor? kappa, Tensor? restraint_period, "
          "Tensor? flat, int[] hills_columns, Tensor? centers, Tensor? heights, Tensor? sigma, Tensor? hills_period, int[] grid_columns, Tensor? table, "
          "float[] lower, float[] spacing, bool[] periodic, Tensor[] into) -> Tensor[]");
    m.def("value_and_bias_opes_h(Tensor x, int handle, Tensor ref_x, Tensor[] weights, Tensor[] biases, Tensor? center, Tensor? kappa, Tensor? restraint_period, "
          "Tensor? flat, int[] opes_columns, Tensor centers, Tensor heights, Tensor sigma, Tensor? opes_period, float scale, float norm, float epsilon, "
          "float cutoff, int[] grid_columns, Tensor? table, float[] lower, float[] spacing, bool[] periodic, Tensor[] into) -> Tensor[]");
    m.def("value_and_bias_opes(Tensor x, int[] desc, Tensor ref_x, Tensor[] weights, Tensor[] biases, Tensor? center, Tensor? kappa, Tensor? restraint_period, "
          "Tensor? flat, int[] opes_columns, Tensor centers, Tensor heights, Tensor sigma, Tensor? opes_period, float scale, float norm, float epsilon, "
          "float cutoff, int[] grid_columns, Tensor? table, float[] lower, float[] spacing, bool[] periodic, Tensor[] into) -> Tensor[]");
    m.def("value_and_bias_opes_table_h(Tensor x, int handle, Tensor ref_x, Tensor[] weights, Tensor[] biases, Tensor? center, Tensor? kappa, "
          "Tensor? restraint_period, Tensor? flat, int[] opes_columns, Tensor centers, Tensor heights, Tensor sigma, Tensor state, Tensor? opes_period, "
          "float scale, float epsilon, float cutoff, int[] grid_columns, Tensor? table, float[] lower, float[] spacing, bool[] periodic, "
          "Tensor[] into) -> Tensor[]");
    m.def("value_and_bias_opes_table(Tensor x, int[] desc, Tensor ref_x, Tensor[] weights, Tensor[] biases, Tensor? center, Tensor? kappa, "
          "Tensor? restraint_period, Tensor? flat, int[] opes_columns, Tensor centers, Tensor heights, Tensor sigma, Tensor state, Tensor? opes_period, "
          "float scale, float epsilon, float cutoff, int[] grid_columns, Tensor? table, float[] lower, float[] spacing, bool[] periodic, "
          "Tensor[] into) -> Tensor[]");
    m.def("value_and_pbmetad_h(Tensor x, int handle, Tensor ref_x, Tensor[] weights, Tensor[] biases, Tensor? center, Tensor? kappa, "
          "Tensor? restraint_period, Tensor? flat, int[] columns, Tensor table, int[] shape, float[] lower, float[] spacing, bool[] periodic, float kT, "
          "Tensor[] into) -> Tensor[]");
    m.def("value_and_pbmetad(Tensor x, int[] desc, Tensor ref_x, Tensor[] weights, Tensor[] biases, Tensor? center, Tensor? kappa, "
          "Tensor? restraint_period, Tensor? flat, int[] columns, Tensor table, int[] shape, float[] lower, float[] spacing, bool[] periodic, float kT, "
          "Tensor[] into) -> Tensor[]");
    m.def("opes_deposit(Tensor(a!) centers, Tensor(b!) sigma, Tensor(c!) heights, Tensor(d!) state, Tensor? period, Tensor new_centers, "
          "Tensor new_sigma, Tensor new_heights, float threshold, float cutoff) -> ()");
    m.def("value_and_opes_table_h(Tensor x, int handle, Tensor ref_x, Tensor[] weights, Tensor[] biases, Tensor centers, Tensor heights, Tensor sigma, "
          "Tensor state, Tensor? period, float scale, float epsilon, float cutoff, Tensor[] into) -> Tensor[]");
    m.def("value_and_opes_table(Tensor x, int[] desc, Tensor ref_x, Tensor[] weights, Tensor[] biases, Tensor centers, Tensor heights, Tensor sigma, "
          "Tensor state, Tensor? period, float scale, float epsilon, float cutoff, Tensor[] into) -> Tensor[]");
    m.def("opes_step(Tensor(a!) centers, Tensor(b!) sigma, Tensor(c!) heights, Tensor(d!) state, Tensor(e!) run, Tensor? period, Tensor y, Tensor V, "
          "Tensor sigma0, Tensor? sigma_min, float beta, float threshold, float cutoff, bool fixed_sigma) -> ()");
    m.def("metad_step(Tensor(a!) table, Tensor(b!) state, Tensor(c!)? log, float[] lower, float[] spacing, bool[] periodic, float[] sigma, "
          "int[] columns, Tensor y, Tensor V, float height0, float inv_dT, float cutoff) -> ()");
    m.def("metad_rct(Tensor table, Tensor? state, Tensor(a!) partials, Tensor(b!) rct, float kT, float inv_dT, int stride) -> ()");
    m.def("opes_kernel_sum(Tensor points, Tensor centers, Tensor heights, Tensor sigma, Tensor? period, float cutoff, bool with_grad) -> Tensor[]");
    m.def("supports_backward(Tensor x, int[] desc, Tensor ref_x) -> int", supports_backward);
    m.def("supports_mlp_backward(Tensor x, int[] desc, Tensor ref_x) -> int", supports_mlp_backward);
    m.def("run_head(Tensor feat, int[] desc, Tensor ref_x, Tensor[] weights, Tensor[] biases) -> Tensor", run_head);
    m.def("launch_info(int[] desc, int device) -> str", launch_info);
    m.def("invalidate(int[] desc, int device) -> ()", invalidate);
    m.def("release(int[] desc, int device) -> ()", release);
    m.def("pin(int[] desc, int device) -> int", pin);
    m.def("unpin(int[] desc, int device) -> int", unpin);
    m.def("drop_plans() -> int", drop_plans);
    m.def("cached_plans() -> int", cached_plans);
}

TORCH_LIBRARY_IMPL(molann, CUDA, m) { // ROCm builds of torch name the HIP device "cuda"
    m.impl("run", run_hip);
    m.impl("run_backward", run_backward_hip);
    m.impl("run_train", run_train_hip);
    m.impl("run_backward_mlp", run_backward_mlp_hip);
    m.impl("run_backward_kept", run_backward_kept_hip);
    m.impl("value_and_vjp", value_and_vjp_hip);
    m.impl("run_h", run_h_hip);
    m.impl("value_and_vjp_h", value_and_vjp_h_hip);
    m.impl("value_and_jacobian", value_and_jacobian_hip);
    m.impl("value_and_jacobian_h", value_and_jacobian_h_hip);
    m.impl("value_and_metric_h", value_and_metric_h_hip);
    m.impl("value_and_restraint", value_and_restraint_hip);
    m.impl("value_and_restraint_h", value_and_restraint_h_hip);
    m.impl("value_and_hills", value_and_hills_hip);
    m.impl("value_and_hills_h", value_and_hills_h_hip);
    m.impl("value_and_opes", value_and_opes_hip);
    m.impl("value_and_opes_h", value_and_opes_h_hip);
    m.impl("value_and_grid", value_and_grid_hip);
    m.impl("value_and_grid_h", value_and_grid_h_hip);
    m.impl("value_and_bias", value_and_bias_hip);
    m.impl("value_and_bias_h", value_and_bias_h_hip);
    m.impl("value_and_bias_opes", value_and_bias_opes_hip);
    m.impl("value_and_bias_opes_h", value_and_bias_opes_h_hip);
    m.impl("value_and_bias_opes_table", value_and_bias_opes_table_hip);
    m.impl("value_and_bias_opes_table_h", value_and_bias_opes_table_h_hip);
    m.impl("value_and_pbmetad", value_and_pbmetad_hip);
    m.impl("value_and_pbmetad_h", value_and_pbmetad_h_hip);
    m.impl("opes_deposit", opes_deposit_hip);
    m.impl("value_and_opes_table", value_and_opes_table_hip);
    m.impl("value_and_opes_table_h", value_and_opes_table_h_hip);
    m.impl("opes_step", opes_step_hip);
    m.impl("metad_step", metad_step_hip);
    m.impl("metad_rct", metad_rct_hip);
    m.impl("opes_kernel_sum", opes_kernel_sum_hip);
}

TORCH_LIBRARY_IMPL(molann, Autograd, m) { m.impl("run", run_autograd); }
