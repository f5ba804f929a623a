// C-ABI implementation (include/audiodiffuser_amd.h): weight registry keyed by the reference state_dict
// names, per-(B, L) workspace, and the sampler entry point (EDM Heun/churn, EDM-alpha, DPM-Solver multistep, ...) with
// whole-loop hipGraph capture.  The network a handle drives is its Net (adf_api_internal.h; one per adf_net_*.hip).
//
// Host logic mirrors (does not copy) the reference control flow:
//   Diffusion.denoise_fn      src/models/components/diffusion.py:32-63
//   EDMSampler / Alpha / DPM  src/models/components/sampler_edm.py:333-397, :251-300, :624-768
#include "adf_api_internal.h"

using namespace adf;
using namespace adf_api;

namespace adf_api {

std::string g_create_error;

int get_plan(adf_handle* h, int B, int L, hipStream_t s, Plan** out, bool own_call, int variant) {
    const NetDims& c = h->net->dims;
    if (const char* why = own_call ? nullptr : h->net->own_entry()) return fail(h, why);
    if (B < 1 || L < 1 || L % c.length_multiple) return fail(h, "length must be a positive multiple of the total down-sampling factor");
    if (adf_weights_missing(h)) return fail(h, "weights are not fully loaded");
    if (h->net->prepare(h, s) || h->net->check_image(h, L)) return 1;
    const std::tuple<int, int, int> pkey{B, L, h->net->image ? h->net->H : variant};
    auto it = h->plans.find(pkey);
    if (it != h->plans.end()) { *out = it->second; h->last_plan = it->second; it->second->last_use = ++h->use_clock; return 0; }
    Plan* p = new Plan();
    p->B = B; p->L = L;
    p->dry = true;
    FwdIO io;
    io.nb = B; io.variant = variant;
    if (forward(h, p, io, s)) { delete p; return 1; }
    // a long-running caller with varying batch sizes / lengths must not accumulate workspaces: release the least recently
    // used plan first (its graphs and buffers may still be referenced by queued work: drain the device before freeing)
    while (h->plans.size() >= kMaxPlans) {
        auto victim = h->plans.begin();
        for (auto i2 = h->plans.begin(); i2 != h->plans.end(); ++i2)
            if (i2->second->last_use < victim->second->last_use) victim = i2;
        (void)hipDeviceSynchronize();
        destroy_plan(h, victim->second);
        h->plans.erase(victim);
    }
    p->arena_bytes = p->arena_off; p->stats_bytes = p->stats_off;
    p->arena = (char*)dalloc(h, p->arena_bytes, p);
    p->stats = (char*)dalloc(h, p->stats_bytes ? p->stats_bytes : 256, p);
    const size_t wave = (size_t)B * c.out_channels * L;
    p->temb = (float*)dalloc(h, (size_t)B * c.temb * 4, p);
    p->film = (float*)dalloc(h, (size_t)B * h->film_total * 4, p);
    p->coef = (float*)dalloc(h, (size_t)B * 4 * 4, p);
    bool ok = p->arena && p->stats && p->temb && p->film && p->coef;
    for (int i = 0; i < 10; ++i) { p->sb[i] = (float*)dalloc(h, wave * 4, p); ok = ok && p->sb[i]; }
    // noise_stage serves as the sampler's noise ([B][out_channels][L]) AND as the network input of the warm-up below ([B][in_channels][L]): the larger
    const size_t wave_in = (size_t)B * std::max(c.in_channels, c.out_channels) * L;
    p->noise_stage = (float*)dalloc(h, wave_in * 4, p);
    p->out_stage = (float*)dalloc(h, wave * 4, p);
    ok = ok && p->noise_stage && p->out_stage;
    if (!ok) { destroy_plan(h, p); return fail(h, "device allocation failed for the workspace"); }
    p->dry = false;
    // eager warm-up (loads code objects, sets kernel attributes) so a later graph capture is clean
    io.x = p->noise_stage; io.out = p->out_stage; io.t = p->coef; io.t_stride = 1; io.nb = B; io.mode = 0;
    if (forward(h, p, io, s)) { destroy_plan(h, p); return 1; }
    if (hipStreamSynchronize(s) != hipSuccess) {
        destroy_plan(h, p);
        return fail(h, std::string("warm-up forward failed: ") + hipGetErrorString(hipGetLastError()));
    }
    h->plans[pkey] = p;
    h->last_plan = p;
    p->last_use = ++h->use_clock;
    *out = p;
    return 0;
}

int forward(adf_handle* h, Plan* p, const FwdIO& io, hipStream_t s) {
    if (!p->dry) ++h->ctr.net_passes;
    return h->net->forward(h, p, io, s);
}

int create_begin(const char* fn, const void* cfg, adf_handle** out) {
    if (!cfg || !out) { g_create_error = std::string(fn) + ": null argument"; return 1; }
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) { g_create_error = std::string(fn) + ": no HIP device available"; return 1; }
    return 0;
}

int create_finish(const char* fn, int dtype, std::unique_ptr<Net> net, adf_handle** out) {
    adf_handle* h = new adf_handle();
    if (hipGetDevice(&h->device) != hipSuccess) { g_create_error = std::string(fn) + ": hipGetDevice failed"; delete h; return 1; }
    h->bf16 = dtype == ADF_DTYPE_BF16;
    h->x3 = dtype == ADF_DTYPE_F32X3;               // fp32 storage (esz 4, 32 K elements per row) with split-bf16 GEMM operands
    h->esz = h->bf16 ? 2 : 4;
    h->kc = kRowBytes / h->esz;
    h->net = std::move(net);
    if (h->net->build_weights(h)) { g_create_error = h->err; adf_destroy(h); return 1; }
    *out = h;
    return 0;
}

// ---- what the three sampler entry points (adf_sampler_run, adf_sampler_run_table, adf_sampler_run_program) share ---------------------------------
// `floats` floats of injected noise copied into the plan's staging buffer, grown first where it is too small
static int stage_injected(adf_handle* h, Plan* p, const float* injected_noise, size_t floats, hipStream_t s) {
    if (p->inj_cap < floats) {
        if (p->inj_stage) {                      // captured graphs read the old staging buffer: drain and drop them with it
            (void)hipDeviceSynchronize();
            drop_graphs(p);
            dfree(h, p->inj_stage, p->inj_cap * 4, p);
            p->inj_stage = nullptr; p->inj_cap = 0;
        }
        p->inj_stage = (float*)dalloc(h, floats * 4, p);
        if (!p->inj_stage) return fail(h, "device allocation failed for injected noise");
        p->inj_cap = floats;
    }
    if (hipMemcpyAsync(p->inj_stage, injected_noise, floats * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return fail(h, "injected-noise copy failed");
    return 0;
}

// the buffers of the per-run table (Plan::coef_all / temb_all / film_all) for n_eval evaluations -- sized before any capture starts
static int reserve_eval_tables(adf_handle* h, Plan* p, int n_eval) {
    const NetDims& nd = h->net->dims;
    p->pre_rows = n_eval;
    p->den_rows = 0;
    if (n_eval <= p->pre_cap) return 0;
    if (p->pre_cap) {
        (void)hipDeviceSynchronize();
        drop_graphs(p);
        dfree(h, p->coef_all, (size_t)p->pre_cap * 4 * 4, p);
        dfree(h, p->temb_all, (size_t)p->pre_cap * nd.temb * 4, p);
        dfree(h, p->film_all, (size_t)p->pre_cap * h->film_total * 4, p);
        p->pre_cap = 0;
    }
    p->coef_all = (float*)dalloc(h, (size_t)n_eval * 4 * 4, p);
    p->temb_all = (float*)dalloc(h, (size_t)n_eval * nd.temb * 4, p);
    p->film_all = (float*)dalloc(h, (size_t)n_eval * h->film_total * 4, p);
    if (!p->coef_all || !p->temb_all || !p->film_all) return fail(h, "device allocation failed for the per-run sigma table");
    p->pre_cap = n_eval;
    return 0;
}

// sigma embeddings and FiLM projections of the n_eval rows already in Plan::coef_all, in two launches
static int embed_eval_tables(adf_handle* h, Plan* p, int n_eval, hipStream_t st) {
    const NetDims& nd = h->net->dims;
    if (const char* e = h->net->time_embed(p->coef_all + 1, 4, n_eval, p->temb_all, st)) return fail(h, e);
    if (h->per_sample_film()) return 0;                    // per-sample FiLM rows (time + class embedding): projected inside each pass
    if (const char* e = launch_film(p->temb_all, nd.temb, h->film_w, nd.temb + h->cdim, 0, h->film_b, p->film_all, n_eval, h->film_total, st))
        return fail(h, e);
    return 0;
}

// the handle state a captured loop depends on, appended to its cache key
static void append_handle_key(const adf_handle* h, std::string* key) {
    key->push_back(h->cond_on ? 'c' : 'u');                   // the guidance branch structure is part of the captured graph
    key->append((const char*)&h->cond_scale, sizeof(float));
    key->append((const char*)&h->dyn_q, sizeof(float));        // the clipping of every evaluation is part of the captured graph
    const Precond& pc = h->precond;                            // ... and so are the preconditioning formulas and their parameters
    const float pk[6] = {(float)pc.kind, pc.beta_min2, pc.two_beta_d, pc.beta_min, pc.beta_d, pc.m_minus_1};
    key->append((const char*)pk, sizeof(pk));
}

// One sampler run: enqueue(stream, &result) puts the whole loop on `stream` and names the buffer that holds the sample.  Eagerly on the caller's
// stream, or -- use_graph -- captured once per `key` on the handle's own stream and replayed; then the copy to `out` and the counters.
template <class Enqueue>
static int run_loop(adf_handle* h, Plan* p, bool use_graph, const std::string& key, Enqueue enqueue, float* out, long long n, int n_eval, hipStream_t s) {
    float* result = nullptr;
    if (!use_graph) {
        if (enqueue(s, &result)) return 1;
        if (hipMemcpyAsync(out, result, (size_t)n * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return fail(h, "result copy failed");
        ++h->ctr.sampler_runs; h->ctr.sampler_evals += n_eval;
        return 0;
    }
    if (!h->gstream) {
        if (hipStreamCreateWithFlags(&h->gstream, hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&h->ev_in, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&h->ev_out, hipEventDisableTiming) != hipSuccess)
            return fail(h, "could not create the graph stream / events");
    }
    hipStream_t gs = h->gstream;
    // inputs staged on the caller's stream must be visible to the graph stream
    if (hipEventRecord(h->ev_in, s) != hipSuccess || hipStreamWaitEvent(gs, h->ev_in, 0) != hipSuccess)
        return fail(h, "stream fence (in) failed");
    auto it = std::find_if(p->graphs.begin(), p->graphs.end(), [&](const std::pair<std::string, hipGraphExec_t>& g) { return g.first == key; });
    if (it != p->graphs.end() && it != p->graphs.begin()) {      // most recently used first
        std::rotate(p->graphs.begin(), it, it + 1);
        it = p->graphs.begin();
    }
    if (it == p->graphs.end()) {
        const hipError_t be = hipStreamBeginCapture(gs, hipStreamCaptureModeRelaxed);
        if (be != hipSuccess) return fail(h, std::string("hipStreamBeginCapture failed: ") + hipGetErrorString(be));
        int rc = enqueue(gs, &result);
        if (!rc && hipMemcpyAsync(p->out_stage, result, (size_t)n * 4, hipMemcpyDeviceToDevice, gs) != hipSuccess) { rc = 1; h->err = "result copy failed (capture)"; }
        hipGraph_t graph = nullptr;
        const hipError_t ee = hipStreamEndCapture(gs, &graph);
        if (rc) { if (graph) (void)hipGraphDestroy(graph); return 1; }
        if (ee != hipSuccess || !graph) return fail(h, std::string("hipStreamEndCapture failed: ") + hipGetErrorString(ee));
        hipGraphExec_t exec = nullptr;
        const hipError_t ie = hipGraphInstantiate(&exec, graph, nullptr, nullptr, 0);
        (void)hipGraphDestroy(graph);
        if (ie != hipSuccess) return fail(h, std::string("hipGraphInstantiate failed: ") + hipGetErrorString(ie));
        if (p->graphs.size() >= kMaxGraphsPerPlan) {               // every distinct (sampler, schedule, guidance) adds one: cap it
            if (hipStreamSynchronize(gs) != hipSuccess) { (void)hipGraphExecDestroy(exec); return fail(h, "graph stream sync failed"); }
            (void)hipGraphExecDestroy(p->graphs.back().second);
            p->graphs.pop_back();
        }
        p->graphs.insert(p->graphs.begin(), std::make_pair(key, exec));
        it = p->graphs.begin();
        ++h->ctr.graph_captures;
    }
    if (hipGraphLaunch(it->second, gs) != hipSuccess) return fail(h, "hipGraphLaunch failed");
    if (hipEventRecord(h->ev_out, gs) != hipSuccess || hipStreamWaitEvent(s, h->ev_out, 0) != hipSuccess)
        return fail(h, "stream fence (out) failed");
    if (hipMemcpyAsync(out, p->out_stage, (size_t)n * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return fail(h, "result copy failed");
    ++h->ctr.sampler_runs; ++h->ctr.graph_replays; h->ctr.sampler_evals += n_eval;
    return 0;
}

// Everything between an entry point's own refusals and the end of its run: the plan and what a run asks of the handle, the buffers an evaluation may
// need (all_buffers: whatever the handle may be set to; otherwise only what guidance, an unclipped estimate without the fused epilogue or the dynamic
// threshold needs as it is set now), the noise and the ndraws draws staged, the per-run tables sized -- all before any capture starts -- and run_loop
// around: upload(coef_all, stream) puts the n_eval rows into Plan::coef_all, they are embedded, body(plan, n, stream, &result) enqueues the rest.
// `who` prefixes the messages ("" for adf_sampler_run).  draws_refusal, where it is not empty, is reported once the handle and the noise have been
// seen to, which is where adf_sampler_run has always reported it.  `key` holds the entry point's own bytes; the handle's are appended here.
template <class Upload, class Body>
static int run_staged(adf_handle* h, const std::string& who, bool all_buffers, const float* noise, const float* injected_noise, int ndraws,
                      const std::string& draws_refusal, int n_eval, bool use_graph, std::string key, Upload upload, Body body, float* out, int B, int L,
                      hipStream_t s) {
    Plan* p;
    if (get_plan(h, B, L, s, &p)) return 1;
    const NetDims& nd = h->net->dims;
    const long long n = (long long)B * nd.out_channels * L;
    if (nd.in_channels != nd.out_channels)
        return fail(h, who.empty() ? "sampler needs in_channels == out_channels" : who + "the handle's network needs in_channels == out_channels");
    if (h->cdim > 0 && (!h->cond_on || h->cond_B != B))
        return fail(h, who + "class-conditional network: call adf_set_condition with the labels of this batch first");
    const bool guided = h->cdim > 0 && h->cond_scale != 1.0f;
    // unclipped estimate without a mode 2 epilogue: raw pass + combine (denoise_io); the raw kind (ReFlow(for_edm=False)) combines only under guidance
    const bool combined = h->unclipped() && !h->raw_output() && !h->net->unclipped_epilogue;
    const bool dyn = h->dyn_q > 0.0f;
    if ((all_buffers || guided || combined || dyn) && ensure_cfg_buffers(h, p)) return 1;
    if (dyn && ensure_dyn_scale(h, p, who)) return 1;
    if (hipMemcpyAsync(p->noise_stage, noise, (size_t)n * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return fail(h, who + "noise copy failed");
    if (!draws_refusal.empty()) return fail(h, draws_refusal);
    if (ndraws > 0 && stage_injected(h, p, injected_noise, (size_t)ndraws * n, s)) return 1;
    if (reserve_eval_tables(h, p, n_eval)) return 1;
    // head of the loop (inside the captured graph when there is one): coefficients, sigma embeddings and FiLM projections of all evaluations in
    // three launches
    auto enqueue = [&](hipStream_t st, float** result) -> int {
        if (n_eval > 0) {
            if (const char* e = upload(p->coef_all, st)) return fail(h, e);
            if (embed_eval_tables(h, p, n_eval, st)) return 1;
        }
        return body(p, n, st, result);
    };
    if (use_graph) append_handle_key(h, &key);
    return run_loop(h, p, use_graph, key, enqueue, out, n, n_eval, s);
}

// One run of a lowered op list (adf_sampler.hip): the rows are uploaded as the list gives them instead of being derived from sigmas, and an evaluation
// may end in any ADF_CLIP_* mode, so every buffer is allocated.
static int run_op_list(adf_handle* h, const std::string& who, const OpList& l, const float* noise, const float* injected_noise, int ndraws, bool use_graph,
                       const std::string& key, float* out, int B, int L, hipStream_t s) {
    const std::vector<float> rows = op_rows(l);
    const int n_eval = (int)(rows.size() / 4);
    return run_staged(h, who, true, noise, injected_noise, ndraws, "", n_eval, use_graph, key,
                      [&](float* coef_all, hipStream_t st) { return launch_coef_rows(rows.data(), n_eval, coef_all, st); },
                      [&](Plan* p, long long n, hipStream_t st, float** result) { return run_ops(h, p, l, n, st, result); }, out, B, L, s);
}

}  // namespace adf_api

// =====================================================================================================
// C ABI (adf_create, adf_wavenet_create, adf_adm_create, adf_unet2d_create: beside their networks, adf_net_*.hip)
// =====================================================================================================
extern "C" {

int adf_set_image_shape(adf_handle* h, int H, int W) {
    if (!h || !h->net->image) return h ? fail(h, "adf_set_image_shape: not a UNetModel / UNet2dBase handle") : 1;
    if (H < 1 || W < 1) return fail(h, "adf_set_image_shape: bad shape");
    h->net->H = H; h->net->W = W;
    return 0;
}

void adf_destroy(adf_handle* h) {
    if (!h) return;
    DeviceScope scope(h);
    for (auto& kv : h->plans) destroy_plan(h, kv.second);
    h->plans.clear();
    for (void* p : h->allocs) (void)hipFree(p);
    if (h->ev_in) (void)hipEventDestroy(h->ev_in);
    if (h->ev_out) (void)hipEventDestroy(h->ev_out);
    if (h->gstream) (void)hipStreamDestroy(h->gstream);
    delete h;
}

const char* adf_last_error(const adf_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int adf_num_weights(const adf_handle* h) { return (int)h->names.size(); }
const char* adf_weight_name(const adf_handle* h, int i) { return (i >= 0 && i < (int)h->names.size()) ? h->names[i].c_str() : nullptr; }
int64_t adf_weight_numel(const adf_handle* h, int i) {
    if (i < 0 || i >= (int)h->names.size()) return -1;
    return h->slots.at(h->names[i]).numel;
}

int adf_load_weight(adf_handle* h, const char* name, const float* dev, int64_t numel, void* stream) {
    ADF_ON_DEVICE(h);
    auto it = h->slots.find(name ? name : "");
    if (it == h->slots.end()) return fail(h, std::string("unexpected state_dict key: ") + (name ? name : "(null)"));
    Slot& sl = it->second;
    if (numel != sl.numel) return fail(h, std::string("size mismatch for ") + name + ": expected " + std::to_string(sl.numel) + " got " + std::to_string(numel));
    hipStream_t s = (hipStream_t)stream;
    if (sl.kind == 0) {
        if (hipMemcpyAsync(sl.dst, dev, (size_t)numel * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return fail(h, "hipMemcpyAsync failed");
        for (int p = 0; p < (sl.rep ? sl.rep_n : 0); ++p)
            if (hipMemcpyAsync(sl.rep + (size_t)p * numel, dev, (size_t)numel * 4, hipMemcpyDeviceToDevice, s) != hipSuccess) return fail(h, "hipMemcpyAsync failed");
    } else if (sl.kind == 5) {               // qkv bias with the legacy head-major rows -> q | k | v rows
        if (const char* e = launch_permute_qkv_rows(dev, (float*)sl.dst, sl.f, sl.cout / (3 * sl.f), 1, s)) return fail(h, e);
    } else if (sl.kind == 4) {               // qkv weight: permute the rows into a scratch copy, then pack that
        if (const char* e = launch_permute_qkv_rows(dev, (float*)sl.frag, sl.f, sl.cout / (3 * sl.f), sl.cin, s)) return fail(h, e);
        if (const char* e = launch_pack_weight((const float*)sl.frag, sl.dst, h->gemm_dtype(), 0, sl.cout, sl.cin, sl.K, 0, sl.n_offset, sl.n_pad, sl.nchunk, s))
            return fail(h, e);
    } else if (sl.kind == 6) {               // UNet2dBase: a load-time transform into an fp32 scratch copy (adf_unet2d.h), then the usual packing
        if (const char* e = launch_u2d_weight_transform(dev, (float*)sl.frag, sl.xmode, sl.cout, sl.cin, sl.K, sl.xc0, sl.xscale, s)) return fail(h, e);
        if (const char* e = launch_pack_weight((const float*)sl.frag, sl.dst, h->gemm_dtype(), 0, sl.cout, sl.cin, sl.K, 0, sl.n_offset, sl.n_pad, sl.nchunk, s))
            return fail(h, e);
    } else {
        const char* e = launch_pack_weight(dev, sl.dst, h->gemm_dtype(), sl.kind == 2 ? 1 : (sl.kind == 3 ? 2 : 0), sl.cout, sl.cin, sl.K, sl.f, sl.n_offset,
                                           sl.n_pad, sl.nchunk, s);
        if (e) return fail(h, e);
        if (sl.kind == 2 && sl.dst3) {
            e = launch_pack_weight(dev, sl.dst3, h->gemm_dtype(), 3, sl.cout, sl.cin, sl.K, sl.f, 0, sl.n_pad3, sl.nchunk, s);
            if (e) return fail(h, e);
        }
        if (sl.frag) {
            // rows of this tensor: cout (conv / linear) or f * cout phase-major rows (transposed conv)
            e = launch_repack_frag(sl.dst, sl.frag, sl.n_offset, sl.kind == 2 ? sl.f * sl.cout : sl.cout, sl.n_pad, sl.nchunk * sl.taps, s);
            if (e) return fail(h, e);
        }
    }
    sl.loaded = true;
    h->net->weight_loaded();
    return 0;
}

int adf_weights_missing(const adf_handle* h) {
    int m = 0;
    for (const auto& kv : h->slots) m += kv.second.loaded ? 0 : 1;
    return m;
}

int adf_net_forward(adf_handle* h, const float* x, const float* t, float* out, int B, int L, void* stream) {
    ADF_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    Plan* p;
    if (get_plan(h, B, L, s, &p)) return 1;
    FwdIO io;
    io.x = x; io.out = out; io.t = t; io.t_stride = 1; io.nb = B;
    p->cfg_live = false;
    if (cond_rows(h, B, false, io)) return 1;
    return forward(h, p, io, s);
}

int adf_set_condition(adf_handle* h, const int64_t* classes_dev, int B, int null_labels, float cond_scale, void* stream) {
    ADF_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    if (!classes_dev) { h->cond_on = false; h->cond_scale = 1.0f; return 0; }
    if (h->cdim == 0) return fail(h, "adf_set_condition: the network was built without class conditioning (num_classes = 0)");
    if (B < 1) return fail(h, "adf_set_condition: bad batch size");
    if (adf_weights_missing(h)) return fail(h, "weights are not fully loaded");
    if (B > h->cond_cap) {
        // graphs captured earlier hold the old buffer addresses; drain them before the buffers go
        (void)hipDeviceSynchronize();
        for (auto& kv : h->plans) drop_graphs(kv.second);
        dfree(h, h->cond_classes, (size_t)h->cond_cap * 8);
        dfree(h, h->cond_emb, (size_t)(h->cond_cap + 1) * h->cdim * 4);
        dfree(h, h->cond_film, (size_t)(h->cond_cap + 1) * h->film_total * 4);
        h->cond_cap = 0;
        h->cond_classes = (long long*)dalloc(h, (size_t)B * 8);
        h->cond_emb = (float*)dalloc(h, (size_t)(B + 1) * h->cdim * 4);
        h->cond_film = (float*)dalloc(h, (size_t)(B + 1) * h->film_total * 4);
        if (!h->cond_classes || !h->cond_emb || !h->cond_film) return fail(h, "device allocation failed for the class condition");
        h->cond_cap = B;
    }
    if (hipMemcpyAsync(h->cond_classes, classes_dev, (size_t)B * 8, hipMemcpyDeviceToDevice, s) != hipSuccess) return fail(h, "class label copy failed");
    const NetDims& c = h->net->dims;
    if (const char* e = launch_class_embed(h->cond_classes, c.num_classes, null_labels ? 1 : 0, h->lab_emb, h->lab_null, h->lab_lnw, h->lab_lnb,
                                           h->lab_w1, h->lab_b1, h->lab_w2, h->lab_b2, c.label_in, h->cdim, h->cond_emb, B + 1, s))
        return fail(h, e);
    // class part of every FiLM projection: columns [tdim, tdim + cdim) of the concatenated weight, no bias (it is in the time part)
    // (not where the embeddings are ADDED before the projections, Net::class_in_temb: nothing separates)
    if (!h->net->class_in_temb)
        if (const char* e = launch_film(h->cond_emb, h->cdim, h->film_w, c.temb + h->cdim, c.temb, nullptr, h->cond_film, B + 1,
                                        h->film_total, s))
            return fail(h, e);
    h->cond_on = true; h->cond_B = B; h->cond_scale = cond_scale;
    return 0;
}

int adf_set_dynamic_threshold(adf_handle* h, float quantile) {
    if (!h) return 1;
    if (!(quantile >= 0.0f) || quantile > 1.0f) return fail(h, "adf_set_dynamic_threshold: the quantile must be in [0, 1] (0 = clamp to [-1, 1])");
    h->dyn_q = quantile;
    return 0;
}

int adf_set_preconditioning(adf_handle* h, int kind, double beta_min, double beta_d, double M) {
    if (!h) return 1;
    Precond pc;
    switch (kind) {
        case ADF_PRECOND_EDM: pc.kind = ADF_PRECOND_KIND_EDM; break;
        case ADF_PRECOND_VE: pc.kind = ADF_PRECOND_KIND_VE; break;
        case ADF_PRECOND_V_EDM: pc.kind = ADF_PRECOND_KIND_V_EDM; break;
        case ADF_PRECOND_RF: pc.kind = ADF_PRECOND_KIND_RF; break;
        case ADF_PRECOND_RF_EDM: pc.kind = ADF_PRECOND_KIND_RF_EDM; break;
        case ADF_PRECOND_VP:
            if (!(beta_d != 0.0) || !std::isfinite(beta_min) || !std::isfinite(beta_d) || !std::isfinite(M))
                return fail(h, "adf_set_preconditioning: ADF_PRECOND_VP needs finite beta_min, beta_d != 0 and M");
            pc.kind = ADF_PRECOND_KIND_VP;
            // the reference forms these in Python doubles; torch rounds each scalar operand to fp32 (diffusion.py:159-160, :165)
            pc.beta_min2 = (float)(beta_min * beta_min); pc.two_beta_d = (float)(2.0 * beta_d);
            pc.beta_min = (float)beta_min; pc.beta_d = (float)beta_d; pc.m_minus_1 = (float)(M - 1.0);
            break;
        default: return fail(h, "adf_set_preconditioning: unknown kind (ADF_PRECOND_EDM, _VE, _VP, _V_EDM, _RF, _RF_EDM)");
    }
    h->precond = pc;
    return 0;
}

int adf_denoise(adf_handle* h, const float* x_noisy, const float* sigmas_dev, float sigma, float sigma_data, float* out, int B,
                int L, void* stream) {
    ADF_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    Plan* p;
    if (get_plan(h, B, L, s, &p)) return 1;
    ++h->ctr.denoise_calls;
    p->den_rows = sigmas_dev ? B : 1;                      // (adf_debug_coef_rows: the rows this call leaves in Plan::coef)
    if (!sigmas_dev) return denoise_scalar(h, p, x_noisy, sigma, sigma_data, out, s);
    return denoise_rows(h, p, x_noisy, sigmas_dev, sigma_data, out, s);
}

// Diffusion.forward / ReFlow.forward under no_grad (diffusion.py:65-97, :185-218, :420-442): mix, one denoiser evaluation, weighted squared error
// (adf_loss.h).  x_noisy and pred live in the first two sampler state buffers of the plan when the caller does not ask for them: a sampler run
// starts from its own noise, so nothing of theirs is carried between calls.
int adf_diffusion_loss(adf_handle* h, int kind, const float* x, const float* noise, const float* sigmas_dev, float sigma_data, float* losses,
                       float* x_noisy_out, float* pred_out, int B, int L, void* stream) {
    if (!h) return 1;
    ADF_ON_DEVICE(h);
    // adf_run_counters is left as it is, whatever the call enqueues (the network passes of the evaluation, a new plan's warm-up pass): adf_loss_calls is the loss's counter
    struct KeepCounters { adf_handle* h; adf_run_counters c; ~KeepCounters() { h->ctr = c; } } keep_counters{h, h->ctr};
    hipStream_t s = (hipStream_t)stream;
    if (kind != ADF_LOSS_X0_EDM && kind != ADF_LOSS_X0_INV_SIGMA2 && kind != ADF_LOSS_RF)
        return fail(h, "adf_diffusion_loss: unknown kind (ADF_LOSS_X0_EDM, _X0_INV_SIGMA2, _RF)");
    if (!x) return fail(h, "adf_diffusion_loss: x is null");
    if (!noise) return fail(h, "adf_diffusion_loss: noise is null");
    if (!sigmas_dev) return fail(h, "adf_diffusion_loss: sigmas_dev is null");
    if (!losses) return fail(h, "adf_diffusion_loss: losses is null");
    if (kind == ADF_LOSS_X0_EDM && !(sigma_data > 0.0f)) return fail(h, "adf_diffusion_loss: sigma_data must be positive for ADF_LOSS_X0_EDM");
    const NetDims& nd = h->net->dims;
    if (nd.in_channels != nd.out_channels) return fail(h, "adf_diffusion_loss: the loss needs in_channels == out_channels");
    if (B < 1 || L < 1) return fail(h, "adf_diffusion_loss: B and L must be positive");
    {   // the outputs must not overlap an input or each other: every kernel of the call reads x (and noise) after x_noisy and pred are written
        const size_t bytes = (size_t)B * nd.out_channels * L * sizeof(float);
        auto overlap = [bytes](const float* a, const float* b) {
            return a && b && (uintptr_t)a < (uintptr_t)b + bytes && (uintptr_t)b < (uintptr_t)a + bytes;
        };
        if (overlap(x_noisy_out, x) || overlap(x_noisy_out, noise)) return fail(h, "adf_diffusion_loss: x_noisy_out overlaps x or noise");
        if (overlap(pred_out, x) || overlap(pred_out, noise)) return fail(h, "adf_diffusion_loss: pred_out overlaps x or noise");
        if (overlap(pred_out, x_noisy_out)) return fail(h, "adf_diffusion_loss: pred_out overlaps x_noisy_out");
    }
    Plan* p;
    if (get_plan(h, B, L, s, &p)) return 1;
    const long long N = (long long)nd.out_channels * L;
    if (!p->loss_partial) {
        p->loss_partial = (double*)dalloc(h, (size_t)B * loss_chunks(N) * sizeof(double), p);
        if (!p->loss_partial) return fail(h, "adf_diffusion_loss: device allocation failed for the block sums");
    }
    float* xn = x_noisy_out ? x_noisy_out : p->sb[0];
    float* pred = pred_out ? pred_out : p->sb[1];
    const int rf = kind == ADF_LOSS_RF;
    if (const char* e = launch_loss_mix(xn, x, noise, sigmas_dev, rf, B, N, s)) return fail(h, e);
    if (denoise_rows(h, p, xn, sigmas_dev, sigma_data, pred, s)) return 1;
    if (const char* e = launch_loss_partial(p->loss_partial, pred, x, rf ? noise : nullptr, B, N, s)) return fail(h, e);
    if (const char* e = launch_loss_finalize(losses, p->loss_partial, sigmas_dev, kind, sigma_data, B, N, s)) return fail(h, e);
    ++h->loss_calls;
    return 0;
}

int64_t adf_loss_calls(const adf_handle* h) { return h ? h->loss_calls : 0; }

int adf_sampler_nfe(const adf_sampler_desc* desc, const float* sigmas_host, int n_sigmas) {
    return count_sampler(desc, sigmas_host, n_sigmas);
}

int adf_sampler_run(adf_handle* h, const adf_sampler_desc* desc, const float* sigmas_host, int n_sigmas, const float* noise,
                    const float* injected_noise, int n_injected, float* out, int B, int L, void* stream) {
    ADF_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    if (!desc || !sigmas_host || n_sigmas < 1) return fail(h, "adf_sampler_run: bad arguments");
    const int ndraws = sampler_draws(*desc, sigmas_host, n_sigmas);
    std::string draws_refusal;
    if (ndraws > 0 && !injected_noise)
        draws_refusal = desc->kind == ADF_SAMPLER_ADPM2 ? "ADPM2Sampler needs injected_noise (one pre-drawn randn_like tensor per step)"
                        : desc->kind == ADF_SAMPLER_ADPMPP2S ? "ADPMPP2SSampler needs injected_noise (one pre-drawn randn_like tensor per step with sigma_next > 0)"
                                                             : "a sampler with s_churn > 0 needs injected_noise (pre-drawn randn_like tensors)";
    else if (ndraws > 0 && n_injected < ndraws)      // the ABI carries the number of [B][C][L] draws behind the pointer: a short buffer is an error, not an over-read
        draws_refusal = "injected_noise holds " + std::to_string(n_injected) + " draws of [B][C][L], this sampler consumes " + std::to_string(ndraws);
    // the sigma of every denoiser evaluation of this run (host logic only)
    std::vector<float> eval_sigmas;
    if (count_sampler(desc, sigmas_host, n_sigmas, &eval_sigmas) < 0) eval_sigmas.clear();     // a schedule the sampler rejects: the real pass below reports why
    const int n_eval = (int)eval_sigmas.size();
    std::string key;
    if (desc->use_graph) {
        key.assign((const char*)desc, sizeof(*desc));
        key.append((const char*)sigmas_host, (size_t)n_sigmas * 4);
        key.push_back(injected_noise ? 'i' : 'n');
    }
    return run_staged(h, "", false, noise, injected_noise, ndraws, draws_refusal, n_eval, desc->use_graph != 0, key,
                      [&](float* coef_all, hipStream_t st) {
                          return launch_edm_coef_list(eval_sigmas.data(), n_eval, h->precond_for(desc->sigma_data), coef_all, st);
                      },
                      [&](Plan* p, long long n, hipStream_t st, float** result) {
                          SamplerCtx c{h, p, desc, sigmas_host, n_sigmas, st, n};
                          c.precomputed = n_eval > 0;
                          return run_sampler(c, result);
                      },
                      out, B, L, s);
}

// The two public forms of the op loop (adf_sampler.hip).  The same staging, per-run evaluation tables, capture cache and counters as adf_sampler_run.
// The table form: one record per step, lowered to ops; a record may read a draw.
int adf_sampler_run_table(adf_handle* h, const adf_table_desc* desc, const adf_table_step* steps, const float* noise, const float* injected_noise,
                          int n_injected, float* out, int B, int L, void* stream) {
    if (!h) return 1;
    ADF_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    const std::string why = table_refusal(desc, steps);
    if (!why.empty()) return fail(h, "adf_sampler_run_table: " + why);
    if (!noise) return fail(h, "adf_sampler_run_table: noise is null");
    if (!out) return fail(h, "adf_sampler_run_table: out is null");
    int ndraws = 0;                                           // draws of injected_noise the table reaches: 1 + the largest `draw` of a record that reads eps
    for (int i = 0; i < desc->num_steps; ++i) {
        if (!table_reads_eps(steps[i])) continue;
        if (!injected_noise) return fail(h, "adf_sampler_run_table: injected_noise is null and steps[" + std::to_string(i) + "] reads eps");
        if (steps[i].draw < 0 || steps[i].draw >= n_injected)
            return fail(h, "adf_sampler_run_table: steps[" + std::to_string(i) + "].draw = " + std::to_string(steps[i].draw) + " is outside the " +
                               std::to_string(n_injected) + " draws of injected_noise (n_injected)");
        ndraws = std::max(ndraws, steps[i].draw + 1);
    }
    std::string key;
    if (desc->use_graph) {
        key.assign("table");                                  // no adf_sampler_desc starts with these bytes (its first field is a kind below 11)
        key.append((const char*)desc, sizeof(*desc));
        key.append((const char*)steps, (size_t)desc->num_steps * sizeof(*steps));
    }
    return run_op_list(h, "adf_sampler_run_table: ", lower_table(desc, steps), noise, injected_noise, ndraws, desc->use_graph != 0, key, out, B, L, s);
}

int adf_sampler_table_nfe(const adf_table_desc* desc, const adf_table_step* steps) {
    if (!table_refusal(desc, steps).empty()) return -1;
    int nfe = 0;                                              // counted off the table: nobody has checked its draws, so it is not lowered
    for (int i = 0; i < desc->num_steps; ++i) nfe += steps[i].second ? 2 : 1;
    return nfe;
}

// The program form: a straight-line program over the plan's state buffers, which is the op list as it stands.  It reads no draws.
int adf_sampler_run_program(adf_handle* h, const adf_prog_desc* desc, const adf_prog_op* ops, const float* noise, float* out, int B, int L, void* stream) {
    if (!h) return 1;
    ADF_ON_DEVICE(h);
    hipStream_t s = (hipStream_t)stream;
    const std::string why = program_refusal(desc, ops);
    if (!why.empty()) return fail(h, "adf_sampler_run_program: " + why);
    if (!noise) return fail(h, "adf_sampler_run_program: noise is null");
    if (!out) return fail(h, "adf_sampler_run_program: out is null");
    std::string key;
    if (desc->use_graph) {
        key.assign("program");                                // no other key starts with these bytes ("table", or a sampler kind below 11)
        key.append((const char*)desc, sizeof(*desc));
        key.append((const char*)ops, (size_t)desc->num_ops * sizeof(*ops));
    }
    return run_op_list(h, "adf_sampler_run_program: ", lower_program(desc, ops), noise, nullptr, 0, desc->use_graph != 0, key, out, B, L, s);
}

int adf_sampler_program_nfe(const adf_prog_desc* desc, const adf_prog_op* ops) {
    if (!program_refusal(desc, ops).empty()) return -1;
    return (int)(op_rows(lower_program(desc, ops)).size() / 4);
}

int adf_abi_version(void) { return ADF_ABI_VERSION; }

int adf_get_counters(const adf_handle* h, adf_run_counters* out) {
    if (!h || !out) return 1;
    *out = h->ctr;
    return 0;
}

int adf_debug_dyn_threshold(adf_handle* h, float* x_dev, int B, long long per_sample, float quantile, void* stream) {
    ADF_ON_DEVICE(h);
    if (!x_dev || B < 1) return fail(h, "adf_debug_dyn_threshold: bad arguments");
    float* sc = (float*)dalloc(h, (size_t)B * 4);
    if (!sc) return fail(h, "device allocation failed");
    const char* e = launch_dyn_threshold(x_dev, B, per_sample, quantile, sc, (hipStream_t)stream);
    (void)hipStreamSynchronize((hipStream_t)stream);
    dfree(h, sc, (size_t)B * 4);
    return e ? fail(h, e) : 0;
}

int adf_debug_coef_rows(adf_handle* h, float* out_dev, int max_rows, int* n_rows, void* stream) {
    ADF_ON_DEVICE(h);
    if (!h->last_plan || (!h->last_plan->coef_all && !h->last_plan->den_rows)) return fail(h, "adf_debug_coef_rows: no sampler run or adf_denoise call yet");
    const Plan* p = h->last_plan;
    const int rows = p->den_rows ? p->den_rows : p->pre_rows;
    const float* src = p->den_rows ? p->coef : p->coef_all;
    if (n_rows) *n_rows = rows;
    const int n = std::min(max_rows, rows);
    if (n > 0 && out_dev && hipMemcpyAsync(out_dev, src, (size_t)n * 4 * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess)
        return fail(h, "adf_debug_coef_rows: copy failed");
    return 0;
}

int adf_debug_tap_count(adf_handle* h) { return h->last_plan ? (int)h->last_plan->taps.size() : 0; }
const char* adf_debug_tap_name(adf_handle* h, int i) {
    if (!h->last_plan || i < 0 || i >= (int)h->last_plan->taps.size()) return nullptr;
    return h->last_plan->taps[i].name.c_str();
}
int adf_debug_tap_shape(adf_handle* h, const char* name, int* C, int* L) {
    if (!h->last_plan) return fail(h, "no forward has run yet");
    // the label embedding of the last adf_set_condition: handle state, [cond_B][cdim] fp32 (the null row behind it is not part of the tap)
    if (h->cdim > 0 && h->cond_on && std::string(name) == "class_emb") { *C = h->cdim; *L = 1; return 0; }
    // the raw passes (labels, null labels) of the last evaluation, where it ran under guidance: fp32 [B][out_channels][L] as the combine kernel read them
    if (h->last_plan->cfg_live && (std::string(name) == "cfg.cond" || std::string(name) == "cfg.null")) {
        *C = h->net->dims.out_channels; *L = h->last_plan->L;
        return 0;
    }
    for (const auto& t : h->last_plan->taps)
        if (t.name == name) { *C = t.C; *L = t.L; return 0; }
    return fail(h, std::string("unknown tap ") + name);
}
int adf_debug_tap_copy(adf_handle* h, const char* name, float* out, void* stream) {
    ADF_ON_DEVICE(h);
    if (!h->last_plan) return fail(h, "no forward has run yet");
    if (h->cdim > 0 && h->cond_on && std::string(name) == "class_emb") {
        if (h->cond_B != h->last_plan->B) return fail(h, "adf_debug_tap_copy: class_emb belongs to another batch size than the last forward");
        if (hipMemcpyAsync(out, h->cond_emb, (size_t)h->cond_B * h->cdim * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess)
            return fail(h, "adf_debug_tap_copy: copy failed");
        return 0;
    }
    if (h->last_plan->cfg_live && (std::string(name) == "cfg.cond" || std::string(name) == "cfg.null")) {
        const Plan* p = h->last_plan;
        const size_t bytes = (size_t)p->B * h->net->dims.out_channels * p->L * 4;
        if (hipMemcpyAsync(out, std::string(name) == "cfg.cond" ? p->cfg_c : p->cfg_n, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream) != hipSuccess)
            return fail(h, "adf_debug_tap_copy: copy failed");
        return 0;
    }
    for (const auto& t : h->last_plan->taps)
        if (t.name == name) {
            const char* e = launch_nlc_to_ncl_f32(t.p, out, t.f32 ? 0 : h->bf16, h->last_plan->B, t.L, t.C, (hipStream_t)stream);
            if (!e && t.scale != 1.0f) e = launch_scale(out, out, t.scale, (long long)h->last_plan->B * t.L * t.C, (hipStream_t)stream);
            return e ? fail(h, e) : 0;
        }
    return fail(h, std::string("unknown tap ") + name);
}

int adf_debug_tap_stats(adf_handle* h, const char* name, double* out_host, int* groups, void* stream) {
    ADF_ON_DEVICE(h);
    if (!h->last_plan || h->last_plan->dry) return fail(h, "no forward has run yet");
    const int G = h->net->dims.stat_groups;
    for (const auto& t : h->last_plan->taps)
        if (t.name == name) {
            if (!t.stats) return fail(h, std::string("adf_debug_tap_stats: no statistics were reduced with ") + name);
            if (groups) *groups = G;
            if (!out_host) return 0;
            if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess ||
                hipMemcpy(out_host, t.stats, (size_t)h->last_plan->B * G * 2 * sizeof(double), hipMemcpyDeviceToHost) != hipSuccess)
                return fail(h, "adf_debug_tap_stats: copy failed");
            return 0;
        }
    return fail(h, std::string("unknown tap ") + name);
}

int64_t adf_device_bytes(const adf_handle* h) { return h->bytes; }

}  // extern "C"
