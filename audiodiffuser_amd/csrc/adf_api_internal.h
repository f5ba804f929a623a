// Internals shared by the translation units behind the C ABI (include/audiodiffuser_amd.h): the handle, the per-(B, L) workspace
// ("plan"), the weight registry, the network walker, the sampler context.  Round 3 split of what was one 2,400-line adf_api.hip:
//   adf_api.hip            handle life cycle, weights, workspaces, the extern "C" entry points every network shares
//   adf_net_unet1d.hip     Unet1dNet: UNet1dBase (unet1d.py:771-816): adf_create, registry, the 1-D walker and its walk
//   adf_net_wavenet.hip    WavenetNet (declared in adf_net_wavenet.h): WaveNetNoise (wavenet.py:153-180): adf_wavenet_create, registry, walk
//   adf_net_adm.hip        AdmNet: ADM UNetModel (unet2d_oai.py:382-635): adf_adm_create, registry, walk
//   adf_net_unet2d.hip     Unet2dNet: Imagen-style UNet2dBase (unet2d.py:622-972), exact fp32: adf_unet2d_create, registry, walk
//   adf_net_dit.hip        DitNet: the adaLN-Zero transformer DiT (dit.py:278-429), exact fp32: adf_dit_create, registry, walk (kernels: adf_dit.h)
//   adf_net_dac.hip        DacNet: dac.py::Decoder, dac.py::Encoder and FineTuneAutoencoder.decode / .encode, exact fp32: adf_dac_create, adf_dac_forward, adf_dac_encode, the weight-norm fold (kernels: adf_dac.h)
//   adf_walk2d.h           what the two 2-D walks share: fine GroupNorm statistics, the conv launch, the conditioning prologue
//   adf_sampler.hip        denoise wrappers; the eleven sampler drivers (sampler_edm.py, stochastic_sampler_edm.py, sampler_rf.py), written on SamplerCtx's
//                          members (below), which own the split between the counting pass and the real pass; count_sampler, sampler_draws; the op
//                          loop behind the table form and the program form (run_ops, at the end of this header)
//   adf_bench_replay.hip   adf_bench_* instrumentation
// A handle owns one Net (below).  This header, adf_api.hip and adf_sampler.hip know a network only through that interface.
#pragma once
#include "../../include/audiodiffuser_amd.h"
#include "adf_gemm.h"
#include "adf_kernels.h"
#include "adf_wavenet.h"
#include "adf_conv2d.h"
#include "adf_unet2d.h"
#include "adf_transformer.h"
#include "adf_resblock_small.h"
#include "adf_resblock_split.h"
#include "adf_loss.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <map>
#include <memory>
#include <string>
#include <vector>


namespace adf_api {
using namespace adf;

extern std::string g_create_error;

struct ConvW {
    void* w = nullptr;
    void* wfrag = nullptr;   // transformer 1x1 weights (bf16): second copy in MFMA-fragment order (adf_transformer.h)
    float* bias = nullptr;
    int cout = 0, cin = 0, K = 0, n = 0, n_pad = 0, nchunk = 0, taps = 0, f = 0;
};

struct Slot {
    int kind = 0;  // 0 = fp32 copy, 1 = pack conv/linear, 2 = pack transposed conv
    void* dst = nullptr;
    void* frag = nullptr;    // also repacked to ConvW::wfrag after packing
    void* dst3 = nullptr; int n_pad3 = 0;   // kind 2: also packed in the 3-tap phase form (UpW::up3)
    float* rep = nullptr; int rep_n = 0;    // kind 0: also copied rep_n times back to back (the bias of that form)
    int64_t numel = 0;
    bool loaded = false;
    int cout = 0, cin = 0, K = 0, f = 0, n_offset = 0, n_pad = 0, nchunk = 0, taps = 0;
    int xmode = 0, xc0 = 0; float xscale = 1.0f;   // kind 6 (UNet2dBase): launch_u2d_weight_transform(mode, c0, scale) into `frag`, then packed
};

struct Act { void* p = nullptr; int C = 0, L = 0; double* stats = nullptr; };
struct TapRec { std::string name; void* p; int C, L; int f32 = 0; float scale = 1.0f; const double* stats = nullptr; };   // f32: an fp32 buffer whatever the storage mode; stats: the GroupNorm statistics reduced with it, if any
struct RbRec { std::string name; GemmArgs g1, g2; int cin, cout, L; };

struct Plan {
    int B = 0, L = 0;
    char* arena = nullptr; size_t arena_bytes = 0, arena_off = 0;
    char* stats = nullptr; size_t stats_bytes = 0, stats_off = 0;
    bool dry = false;
    std::vector<TapRec> taps;
    std::vector<RbRec> rbs;
    float *temb = nullptr, *film = nullptr, *coef = nullptr;
    // per sampler run: (c_in, c_noise, c_skip, c_out), sigma embedding and the FiLM projections of EVERY denoiser evaluation of
    // the run, computed by three launches at the head of the loop (sigma is uniform over the batch and the whole schedule is
    // known on the host) instead of three launches per evaluation
    float *coef_all = nullptr, *temb_all = nullptr, *film_all = nullptr;
    int pre_cap = 0;
    int pre_rows = 0;                                     // rows of coef_all the last sampler run filled (adf_debug_coef_rows)
    int den_rows = 0;                                     // rows of coef the last adf_denoise call filled, if that was the plan's last evaluation (else 0)
    // sampler state (fp32 [B][C][L] each)
    float* sb[10] = {nullptr};
    float* noise_stage = nullptr; float* out_stage = nullptr; float* inj_stage = nullptr; size_t inj_cap = 0;
    float* cfg_c = nullptr; float* cfg_n = nullptr;      // raw network outputs of the two CFG branches
    bool cfg_live = false;                               // both hold the two passes of the plan's last evaluation (adf_debug_tap_copy "cfg.cond" / "cfg.null")
    float* dyn_scale = nullptr;                          // [B] per-sample scales of the dynamic threshold
    double* loss_partial = nullptr;                      // [B][loss_chunks(C * L)] block sums of adf_diffusion_loss, allocated by the first loss call on this plan
    // captured sampler loops, most recently used first; at most kMaxGraphsPerPlan are kept (the oldest is destroyed)
    std::vector<std::pair<std::string, hipGraphExec_t>> graphs;
    std::vector<void*> allocs;                            // device memory owned by this plan (released when the plan is evicted)
    int64_t bytes = 0;
    unsigned long long last_use = 0;
    // timing replay buffers of adf_bench_resblock (rotating copies of one layer's operands), sized on first use
    char* bench_buf = nullptr; size_t bench_cap = 0;
    // WaveNetNoise: the layer launches of the last pass, for adf_bench_wavenet_layer
    WnIO wn_io; std::vector<WnLayerArgs> wn_layers;
};
constexpr size_t kMaxGraphsPerPlan = 8;
constexpr size_t kMaxPlans = 4;      // (B, L) workspaces kept per handle; the least recently used one is released beyond that

struct FwdIO {
    const float* x = nullptr; float* out = nullptr;
    const float* t = nullptr; int t_stride = 0; int nb = 0;
    const float* coef = nullptr; int coef_bstride = 0; const float* x_noisy = nullptr;
    int mode = 0;                                          // 0: raw network output; 1: clamp(c_skip x_noisy + c_out F, -1, 1); 2: the same unclipped (UNet2dBase, DiT)
    const float* film2 = nullptr; int film2_bstride = 0;   // class part of the FiLM projections (rows of adf_handle::cond_film)
    const float* film_pre = nullptr;                       // this evaluation's row of Plan::film_all: sigma embedding + FiLM already computed
    const float* temb_pre = nullptr;                       // this evaluation's row of Plan::temb_all (class-conditional ADM net: the FiLM rows are per sample)
    bool null_cond = false;                                // class-conditional ADM net: every sample takes the null class embedding (guidance branch)
    float* aux = nullptr;                                  // a second result of a net with its own entry point (adf_dac_encode: the KL term, one float)
    int variant = 0;                                       // which walk of a net that walks one (B, L) in more than one way (DAC autoencoder: 0 decode, 1 encode)
};

// What the shared plan, condition and sampler code reads of a network.  The create call fills it once; nothing else writes it.
struct NetDims {
    int in_channels = 0, out_channels = 0;
    int length_multiple = 1;            // the length argument L must be a multiple of this (UNet1dBase: its total down-sampling factor)
    int temb = 0;                       // width of the time embedding: a row of Plan::temb / temb_all
    int label_in = 0, num_classes = 0;  // LabelEmbedder: width of its embedding table, number of labels (0 = no class conditioning)
    int stat_groups = 1;                // GroupNorm groups per sample in one Walker::alloc_stats slab
};

// One network behind the C ABI: what the shared code asks of it.  One implementation per adf_net_*.hip.
struct Net {
    NetDims dims;
    // the class embedding is added to the time embedding before the FiLM projections, so the FiLM rows are per sample (UNetModel, unet2d_oai.py:621-623;
    // UNet2dBase, unet2d.py:902-908); false: the class columns are projected on their own into adf_handle::cond_film (UNet1dBase, unet1d.py:272)
    bool class_in_temb = false;
    bool unclipped_epilogue = false;    // the last kernel has the FwdIO mode 2 epilogue (UNet2dBase, DiT)
    // inputs are images [B][C][H][W]: adf_set_image_shape gives the shape behind the length argument L = H * W of the calls that follow
    bool image = false;
    int H = 0, W = 0;
    virtual ~Net() {}
    virtual int build_weights(adf_handle* h) = 0;                        // the registry, in state_dict order
    virtual int check_image(adf_handle* h, int L) { (void)h; (void)L; return 0; }      // image nets: (H, W) against L and the levels, before a plan
    virtual void weight_loaded() {}                                      // a tensor was (re)loaded ...
    virtual int prepare(adf_handle* h, hipStream_t s) { (void)h; (void)s; return 0; }   // ... and what that needs before the next pass
    virtual int forward(adf_handle* h, Plan* p, const FwdIO& io, hipStream_t s) = 0;
    // non-null: the net is no denoiser (the DAC decoder stack) -- why adf_net_forward, adf_denoise, the loss and the samplers refuse the handle
    virtual const char* own_entry() const { return nullptr; }
    // n rows of the time / sigma embedding ([n][dims.temb]) from t[i * t_stride]
    virtual const char* time_embed(const float* t, int t_stride, int n, float* temb, hipStream_t s) = 0;
};

}  // namespace adf_api

using namespace adf_api;      // (this header is private to the translation units behind the C ABI)

struct adf_handle {
    std::unique_ptr<Net> net;
    int device = 0;                     // the device that was current at adf_create: every entry point runs on it
    unsigned long long use_clock = 0;
    bool bf16 = false;
    bool x3 = false;                    // ADF_DTYPE_F32X3: storage and every non-GEMM kernel as fp32 (bf16 == false), GEMM operands split into bf16 hi + lo
    int gemm_dtype() const { return bf16 ? 1 : (x3 ? 2 : 0); }      // the `dtype` of launch_conv_gemm / launch_pack_weight
    int esz = 4, kc = 32;
    std::string err;
    std::vector<void*> allocs;
    int64_t bytes = 0;
    std::vector<std::string> names;
    std::map<std::string, Slot> slots;
    float *film_w = nullptr, *film_b = nullptr;      // every FiLM projection of the network, concatenated: [film_total][temb (+ cdim)], [film_total]
    int film_total = 0;
    // class conditioning (LabelEmbedder) and the state set by adf_set_condition
    float *lab_null = nullptr, *lab_emb = nullptr, *lab_lnw = nullptr, *lab_lnb = nullptr, *lab_w1 = nullptr, *lab_b1 = nullptr,
          *lab_w2 = nullptr, *lab_b2 = nullptr;
    int cdim = 0;                       // width of the class embedding (Registrar::label_embedder) or 0
    bool per_sample_film() const { return net->class_in_temb && cdim > 0; }      // FiLM rows differ per sample: projected inside each pass
    bool cond_on = false;
    int cond_B = 0;
    float cond_scale = 1.0f;
    Precond precond;                                     // which diffusion class's rows every evaluation uses (adf_set_preconditioning); sigma_data is filled per call
    Precond precond_for(float sigma_data) const { Precond pc = precond; pc.sigma_data = sigma_data; return pc; }
    // VDiffusion(for_edm=True) returns v_to_x0 as it is (diffusion.py:326), and ReFlow never clips in either mode (:388-418)
    bool unclipped() const { return precond.kind == ADF_PRECOND_KIND_V_EDM || precond.kind == ADF_PRECOND_KIND_RF || precond.kind == ADF_PRECOND_KIND_RF_EDM; }
    bool raw_output() const { return precond.kind == ADF_PRECOND_KIND_RF; }         // ReFlow(for_edm=False): the row is (1, t, 0, 1), the estimate is the network output
    float dyn_q = 0.0f;                                  // > 0: dynamic thresholding at this quantile instead of clamp(-1, 1) (adf_set_dynamic_threshold)
    long long* cond_classes = nullptr;  // [cond_B]
    float* cond_emb = nullptr;          // [cond_B + 1][cdim], last row = null embedding
    float* cond_film = nullptr;         // [cond_B + 1][film_total]: class part of every FiLM projection
    int cond_cap = 0;
    // (B, L, H): H = image height of an image net (W = L / H), the FwdIO::variant the plan was built for otherwise (0 but for a DAC autoencoder's encode) -- two image shapes with equal H * W must not share
    // a workspace: captured graphs and tap shapes carry the conv2d geometry
    std::map<std::tuple<int, int, int>, Plan*> plans;
    Plan* last_plan = nullptr;
    // graphs are captured and replayed on a library-owned stream (the caller's stream may be the legacy
    // default stream, which cannot be captured); it is fenced against the caller's stream with events
    hipStream_t gstream = nullptr;
    hipEvent_t ev_in = nullptr, ev_out = nullptr;
    adf_run_counters ctr{};             // what the device loop has done so far (adf_get_counters): lets a test tell it from a host-side loop
    int64_t loss_calls = 0;             // successful adf_diffusion_loss calls (adf_loss_calls; adf_run_counters must not grow at ABI version 7)
};

namespace adf_api {

inline int fail(adf_handle* h, const std::string& m) { h->err = m; return 1; }

// Makes the handle's device current for the duration of a C entry point (and restores the caller's afterwards): buffers,
// kernel attributes and launches of one handle all belong to the device it was created on, whatever is current in the caller.
struct DeviceScope {
    int prev = -1;
    bool ok = true;
    explicit DeviceScope(const adf_handle* h) {
        if (!h) return;
        int cur = -1;
        if (hipGetDevice(&cur) != hipSuccess) { ok = false; return; }
        if (cur != h->device) {
            if (hipSetDevice(h->device) != hipSuccess) { ok = false; return; }
            prev = cur;
        }
    }
    ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
};
#define ADF_ON_DEVICE(h)                                                            \
    DeviceScope adf_scope_(h);                                                      \
    if (!adf_scope_.ok) return fail(h, "could not make the handle's device current")

// device memory owned by the handle (weights, condition buffers) or, with `owner`, by one (B, L) plan
inline void* dalloc(adf_handle* h, size_t bytes, Plan* owner = nullptr) {
    void* p = nullptr;
    bytes = (bytes + 255) & ~(size_t)255;
    if (hipMalloc(&p, bytes) != hipSuccess) return nullptr;
    (void)hipMemset(p, 0, bytes);
    (owner ? owner->allocs : h->allocs).push_back(p);
    if (owner) owner->bytes += (int64_t)bytes;
    h->bytes += (int64_t)bytes;
    return p;
}
inline void dfree(adf_handle* h, void* ptr, size_t bytes, Plan* owner = nullptr) {
    if (!ptr) return;
    std::vector<void*>& v = owner ? owner->allocs : h->allocs;
    auto it = std::find(v.begin(), v.end(), ptr);
    if (it != v.end()) v.erase(it);
    bytes = (bytes + 255) & ~(size_t)255;
    if (owner) owner->bytes -= (int64_t)bytes;
    h->bytes -= (int64_t)bytes;
    (void)hipFree(ptr);
}
inline void drop_graphs(Plan* p) {
    for (auto& g : p->graphs) (void)hipGraphExecDestroy(g.second);
    p->graphs.clear();
}
// (the caller has synchronised the device if work of this plan may still be in flight)
inline void destroy_plan(adf_handle* h, Plan* p) {
    drop_graphs(p);
    for (void* q : p->allocs) (void)hipFree(q);
    h->bytes -= p->bytes;
    if (h->last_plan == p) h->last_plan = nullptr;
    delete p;
}
// ---- weight registry ---------------------------------------------------------------------------
struct Registrar {
    adf_handle* h;
    bool ok = true;
    float* reg_f32(const std::string& name, int64_t numel, float* dst = nullptr) {
        if (!dst) dst = (float*)dalloc(h, (size_t)numel * 4);
        if (!dst) { ok = false; return nullptr; }
        Slot s; s.kind = 0; s.dst = dst; s.numel = numel;
        h->names.push_back(name); h->slots[name] = s;
        return dst;
    }
    // Conv1d / Linear weight (cout, cin, K) packed as GEMM operand; several tensors may share one packed
    // buffer at different row offsets (fused qkv).
    void reg_pack(const std::string& name, ConvW& w, int cout, int cin, int K, int n_offset, int n_total, bool transposed, int f) {
        if (!w.w) {
            w.cin = cin; w.K = K; w.f = f;
            w.taps = transposed ? 2 : K;
            w.n = n_total; w.n_pad = round_up(n_total, 32);
            w.nchunk = ceil_div(cin, h->kc);
            // + kTapGroup slabs of 128 rows: the kernel's weight staging loads are unguarded (adf_gemm.h)
            w.w = dalloc(h, ((size_t)w.nchunk * w.taps * w.n_pad + (size_t)kTapGroup * (w.n_pad + 128)) * kRowBytes);
            if (!w.w) { ok = false; return; }
        }
        w.cout = cout;
        Slot s; s.kind = transposed ? 2 : 1; s.dst = w.w; s.numel = (int64_t)cout * cin * K;
        s.cout = cout; s.cin = cin; s.K = K; s.f = f; s.n_offset = n_offset; s.n_pad = w.n_pad; s.nchunk = w.nchunk; s.taps = w.taps;
        h->names.push_back(name); h->slots[name] = s;
    }
    void conv(const std::string& pre, ConvW& w, int cout, int cin, int K, bool bias) {
        reg_pack(pre + ".weight", w, cout, cin, K, 0, cout, false, 0);
        if (bias) w.bias = reg_f32(pre + ".bias", cout);
    }
    // LabelEmbedder(num_classes, width_in, width_out) (conditioner.py:64-90): sets the handle's lab_* tensors and cdim
    // (`module`: the attribute the network keeps it under -- DiT's is y_embedder)
    void label_embedder(int width_in, int width_out, int num_classes, const std::string& module = "label_conditioner") {
        h->cdim = width_out;
        h->lab_null = reg_f32(module + ".null_classes_emb", width_in);
        h->lab_emb = reg_f32(module + ".label_emb.weight", (int64_t)num_classes * width_in);
        h->lab_lnw = reg_f32(module + ".class_to_cond.0.weight", width_in);
        h->lab_lnb = reg_f32(module + ".class_to_cond.0.bias", width_in);
        h->lab_w1 = reg_f32(module + ".class_to_cond.1.weight", (int64_t)width_out * width_in);
        h->lab_b1 = reg_f32(module + ".class_to_cond.1.bias", width_out);
        h->lab_w2 = reg_f32(module + ".class_to_cond.3.weight", (int64_t)width_out * width_out);
        h->lab_b2 = reg_f32(module + ".class_to_cond.3.bias", width_out);
    }
};

// ---- per-(B, L) plan -----------------------------------------------------------------------------
// What every network's walk uses: the activation and statistics arenas of the plan, the tap list, the first error.
struct Walker {
    adf_handle* h;
    Plan* p;
    hipStream_t s;
    bool bad = false;

    // start of a pass: empty arenas and tap list; the statistics slab zeroed (the kernels accumulate into it)
    int begin() {
        p->arena_off = 0; p->stats_off = 0;
        p->taps.clear(); p->rbs.clear();
        if (!p->dry && p->stats_bytes && hipMemsetAsync(p->stats, 0, p->stats_bytes, s) != hipSuccess) return fail(h, "hipMemsetAsync(stats) failed");
        return 0;
    }
    void check(const char* e) { if (e && !bad) { bad = true; h->err = e; } }
    void* alloc(size_t bytes) {
        bytes = (bytes + 255) & ~(size_t)255;
        const size_t off = p->arena_off;
        p->arena_off += bytes;
        if (p->dry) return nullptr;
        if (p->arena_off > p->arena_bytes) { check("arena overflow"); return nullptr; }
        return p->arena + off;
    }
    double* alloc_stats() {
        const size_t bytes = ((size_t)p->B * h->net->dims.stat_groups * 2 * sizeof(double) + 255) & ~(size_t)255;
        const size_t off = p->stats_off;
        p->stats_off += bytes;
        if (p->dry) return (double*)(uintptr_t)(off + 256);  // non-null marker
        if (p->stats_off > p->stats_bytes) { check("stats arena overflow"); return nullptr; }
        return (double*)(p->stats + off);
    }
    Act new_act(int C, int L) { Act a; a.C = C; a.L = L; a.p = alloc((size_t)p->B * L * C * h->esz); return a; }
    void tap(const std::string& name, const Act& a) { p->taps.push_back({name, a.p, a.C, a.L, 0, 1.0f, a.stats}); }
    bool live() const { return !p->dry && !bad; }
};

// the head of every create call (null arguments, a HIP device exists) and, after its own argument checks, the tail: a handle on the current
// device with the storage mode of `dtype` that owns `net`, its registry built
int create_begin(const char* fn, const void* cfg, adf_handle** out);
int create_finish(const char* fn, int dtype, std::unique_ptr<Net> net, adf_handle** out);
int forward(adf_handle* h, Plan* p, const FwdIO& io, hipStream_t s);
// own_call: from the entry point of a net that is no denoiser (Net::own_entry); every other caller is refused on such a handle
// variant: FwdIO::variant of the walk the workspace is for (its dry pass and warm-up run with it); part of the plan's key
int get_plan(adf_handle* h, int B, int L, hipStream_t s, Plan** out, bool own_call = false, int variant = 0);
int cond_rows(adf_handle* h, int B, bool null_branch, FwdIO& io);
int ensure_cfg_buffers(adf_handle* h, Plan* p);
// How one evaluation ends.  noclip: the estimate is returned as it is -- VDiffusion(for_edm=True), ReFlow: no clamp, and dynamic_threshold is never read
// (diffusion.py:326, :388-418).  raw: the estimate IS the network output (row (c_in, t, 0, 1), ReFlow(for_edm=False)), so without guidance there is
// nothing to combine.  dyn: rescaled by the per-sample quantile instead of clamped.
struct EvalClip { bool noclip = false, raw = false, dyn = false; };
inline EvalClip handle_clip(const adf_handle* h) {
    EvalClip ec;
    ec.noclip = h->unclipped(); ec.raw = h->raw_output(); ec.dyn = h->dyn_q > 0.0f && !ec.noclip;
    return ec;
}
int denoise_io(adf_handle* h, Plan* p, FwdIO io, float* out, hipStream_t s);                        // ends as the handle is set (handle_clip)
int denoise_io(adf_handle* h, Plan* p, FwdIO io, float* out, const EvalClip& ec, hipStream_t s);
// Plan::dyn_scale, allocated where it is missing (outside graph capture, like ensure_cfg_buffers); `who` prefixes the message
int ensure_dyn_scale(adf_handle* h, Plan* p, const std::string& who = "");
// Evaluation k of a sampler run on x: it reads row k of Plan::coef_all and of temb_all / film_all, filled and embedded at the head of the run
inline FwdIO row_io(const adf_handle* h, const Plan* p, int k, const float* x) {
    FwdIO io;
    io.x = x; io.t = p->coef_all + (size_t)k * 4 + 1; io.t_stride = 4; io.nb = 1;
    io.coef = p->coef_all + (size_t)k * 4; io.coef_bstride = 0; io.x_noisy = x;
    if (h->per_sample_film()) io.temb_pre = p->temb_all + (size_t)k * h->net->dims.temb;
    else io.film_pre = p->film_all + (size_t)k * h->film_total;
    return io;
}
int denoise_scalar(adf_handle* h, Plan* p, const float* x, float sigma, float sigma_data, float* out, hipStream_t s);
// one evaluation with a sigma per sample (sigmas_dev [B] on the device): what adf_denoise enqueues, and the middle of adf_diffusion_loss
int denoise_rows(adf_handle* h, Plan* p, const float* x, const float* sigmas_dev, float sigma_data, float* out, hipStream_t s);

// One run of a sampler driver (adf_sampler.hip).  Every driver runs twice: a host-only counting pass (count_sampler: h == p == nullptr,
// serves adf_sampler_nfe and the per-run sigma table) and the real pass, which enqueues the launches.  The members below own that split:
// a driver takes its buffers from buf(), its draws from draw(), launches through start() / run() / finish() and refuses a schedule
// through reject(), and never asks which pass it is in.
struct SamplerCtx {
    adf_handle* h; Plan* p; const adf_sampler_desc* d; const float* sig; int nsig; hipStream_t s; long long n;
    int nfe = 0;
    bool count_only = false;
    std::vector<float>* collect = nullptr;     // counting pass: the sigma of every evaluation, in order
    bool precomputed = false;                  // real pass: evaluation k reads row k of Plan::coef_all / film_all
    int ck(const char* e) { if (e) { h->err = e; return 1; } return 0; }
    float* buf(int k) const { return count_only ? nullptr : p->sb[k]; }                 // state buffer k (fp32 [B][C][L])
    int reject(const std::string& msg) { return count_only ? 1 : fail(h, msg); }         // a schedule / descriptor the driver does not run
    // one launch of adf_kernels.h: every sampler launcher ends in (..., long long n, hipStream_t s)
    template <class F, class... A> int run(F launcher, A... args) { return count_only ? 0 : ck(launcher(args..., n, s)); }
    int start(float* x) { return count_only ? 0 : ck(launch_scale(x, p->noise_stage, sig[0], n, s)); }      // x = sigmas[0] * noise
    int finish(float* x, float** result) { *result = x; return run(launch_clamp, x); }                       // the loops that end in clamp(-1, 1)
    // draw k of the injected noise; the real pass refuses with `needs` when the caller passed none
    int draw(int k, const char* needs, const float** eps) {
        *eps = nullptr;
        if (count_only) return 0;
        if (!p->inj_stage) return fail(h, needs);
        *eps = p->inj_stage + (size_t)k * n;
        return 0;
    }
    int den(const float* x, float sigma, float* out) {
        const int k = nfe++;
        if (count_only) { if (collect) collect->push_back(sigma); return 0; }
        if (precomputed) return denoise_io(h, p, row_io(h, p, k, x), out, s);
        return denoise_scalar(h, p, x, sigma, d->sigma_data, out, s);
    }
    // DPMSampler.model_fn (sampler_edm.py:692-708): the denoised estimate, or with eps_pred the noise prediction (x - D) / sigma
    int model(const float* x, float sigma, float* out) {
        if (den(x, sigma, out)) return 1;
        if (d->eps_pred && !count_only) return ck(launch_eps(out, x, sigma, n, s));
        return 0;
    }
};
int run_sampler(SamplerCtx& c, float** result);
// the counting pass: NFE of this sampler on this schedule, or -1 where its driver rejects it; eval_sigmas: the sigma of every evaluation, in order
int count_sampler(const adf_sampler_desc* d, const float* sig, int nsig, std::vector<float>* eval_sigmas = nullptr);
// [B][C][L] draws of the injected noise the driver reads on this schedule (0: the sampler runs without injected_noise)
int sampler_draws(const adf_sampler_desc& d, const float* sig, int nsig);

// The op loop (adf_sampler.hip) behind the two public forms, adf_sampler_run_table and adf_sampler_run_program.  Each form has its refusal (why it cannot
// run, in the caller's argument names; "" when it can; host only) and its lowering to one OpList; the rows and the NFE of a run are read off the list,
// and run_ops enqueues it on the rows already in Plan::coef_all.  An op of the list is the public program op over a wider slot space: 0 .. 9 are
// Plan::sb[k], the range above them names the draws of Plan::inj_stage, which only a lowered table reads (program_refusal admits no such slot).
struct OpList { std::vector<adf_prog_op> ops; float x0_scale = 1.0f; int result_slot = 0; };
bool table_reads_eps(const adf_table_step& r);
std::string table_refusal(const adf_table_desc* d, const adf_table_step* st);
std::string program_refusal(const adf_prog_desc* d, const adf_prog_op* ops);
OpList lower_table(const adf_table_desc* d, const adf_table_step* st);
OpList lower_program(const adf_prog_desc* d, const adf_prog_op* ops);
std::vector<float> op_rows(const OpList& l);      // the (c_in, c_noise, c_skip, c_out) of the list's evaluations, in order
int run_ops(adf_handle* h, Plan* p, const OpList& l, long long n, hipStream_t s, float** result);

}  // namespace adf_api
