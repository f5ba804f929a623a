// DiT, the adaLN-Zero diffusion transformer, behind the C ABI (reference: src/models/backbones/dit.py:278-429): adf_dit_create, registry and the walk.
// Token-major fp32 activations [B][T][D]; kernels: adf_dit.h, attention: launch_attention (adf_kernels.h).  ADF_DTYPE_F32: exact fp32.
// ADF_DTYPE_F32X3: the four token linears of a block and its attention take the split-bf16 kernels (adf_dit_x3.hip); everything else is the fp32 path.
#include "adf_api_internal.h"
#include "adf_dit.h"

using namespace adf;
using namespace adf_api;

namespace adf_api {

// Linear weights stay the state dict's [N][K] rows (both GEMM operands are K-contiguous), padded with zero rows to whole 128-row tiles: the
// kernel's weight staging loads are unguarded (adf_dit.h).  to_q and to_kv share one [3 D][D] buffer; every adaLN_modulation of the net shares
// adf_handle::film_w / film_b ([(6 depth + 2) D][D]), so that one launch projects all of them.
// f32x3: a linear's weight is also kept as bf16 hi and lo planes of the padded shape (X3W), split from the fp32 buffer -- which stays the load target --
// before the first pass after a (re)load (DitNet::prepare).
struct X3W { unsigned short *hi = nullptr, *lo = nullptr; long long numel = 0; };
struct DitBlock {
    float *wqkv = nullptr, *wout = nullptr, *fc1w = nullptr, *fc1b = nullptr, *fc2w = nullptr, *fc2b = nullptr;
    X3W xqkv, xout, xfc1, xfc2;
    int mod_off = 0;
};

struct DitNet : Net {
    adf_dit_config cfg;
    int D = 0, T = 0, hid = 0, nout = 0;
    float *pos = nullptr, *pe_w = nullptr, *pe_b = nullptr, *t_w1 = nullptr, *t_b1 = nullptr, *t_w2 = nullptr, *t_b2 = nullptr;
    float *fin_w = nullptr, *fin_b = nullptr;
    int fin_mod_off = 0;
    bool block_taps = true;              // route switch ADF_DIT_TAPS (read at create): 0 = never keep the per-block taps, i.e. always the in-place residual stream
    // route switches of the f32x3 mode (read at create): ADF_DIT_X3_LINEAR=0 keeps dit_linear_kernel, ADF_DIT_X3_ATT=0 keeps launch_attention(.., 0, ..)
    bool x3_linear = false, x3_att = false;
    bool split_done = false;             // the hi / lo planes match the fp32 weights
    std::vector<DitBlock> blocks;

    DitNet() { class_in_temb = true; image = true; unclipped_epilogue = true; }
    int build_weights(adf_handle* h) override;
    void weight_loaded() override { split_done = false; }
    int prepare(adf_handle* h, hipStream_t s) override;
    int check_image(adf_handle* h, int L) override {
        if (H != cfg.input_h || W != cfg.input_w || (long long)H * W != L)
            return fail(h, "DiT: call adf_set_image_shape(H, W) with the net's input_size (" + std::to_string(cfg.input_h) + ", " +
                               std::to_string(cfg.input_w) + ") and H * W equal to the length argument first");
        return 0;
    }
    int forward(adf_handle* h, Plan* p, const FwdIO& io, hipStream_t s) override;
    // TimestepEmbedder(hidden_size, frequency_embedding_size = hidden_size): cos half first (conditioner.py:33-56) -- the embedding of the ADM net
    const char* time_embed(const float* t, int t_stride, int n, float* temb, hipStream_t s) override {
        return launch_adm_time_embed(t, t_stride, n, D, t_w1, t_b1, t_w2, t_b2, D, temb, s);
    }
};

int DitNet::build_weights(adf_handle* h) {
    Registrar R{h};
    const int depth = cfg.depth;
    h->film_total = (6 * depth + 2) * D;                     // a multiple of 128 rows: D is a multiple of 64 and 6 depth + 2 is even
    h->film_w = (float*)dalloc(h, (size_t)h->film_total * D * 4);
    h->film_b = (float*)dalloc(h, (size_t)h->film_total * 4);
    // to_context (context_dim = hidden_size, dit.py:232) is in the state dict and never read without text conditioning: one landing buffer for all blocks
    float* ctx = (float*)dalloc(h, (size_t)2 * D * D * 4);
    if (!h->film_w || !h->film_b || !ctx) return fail(h, "device allocation failed while building the weight registry");
    auto padded = [&](int n, int k) { float* q = (float*)dalloc(h, (size_t)round_up(n, kDitTileN) * k * 4); if (!q) R.ok = false; return q; };
    auto planes = [&](int n, int k) {
        X3W x;
        x.numel = (long long)round_up(n, kDitTileN) * k;
        x.hi = (unsigned short*)dalloc(h, (size_t)x.numel * 2); x.lo = (unsigned short*)dalloc(h, (size_t)x.numel * 2);
        if (!x.hi || !x.lo) R.ok = false;
        return x;
    };
    // nn.Module.state_dict order: the module's own parameter (pos_embed) before its children
    pos = R.reg_f32("pos_embed", (int64_t)T * D);
    pe_w = R.reg_f32("x_embedder.proj.weight", (int64_t)D * cfg.in_channels * cfg.patch_h * cfg.patch_w);
    pe_b = R.reg_f32("x_embedder.proj.bias", D);
    t_w1 = R.reg_f32("t_embedder.mlp.0.weight", (int64_t)D * D);
    t_b1 = R.reg_f32("t_embedder.mlp.0.bias", D);
    t_w2 = R.reg_f32("t_embedder.mlp.2.weight", (int64_t)D * D);
    t_b2 = R.reg_f32("t_embedder.mlp.2.bias", D);
    if (cfg.num_classes > 0) R.label_embedder(D, D, cfg.num_classes, "y_embedder");      // LabelEmbedder(num_classes, None, hidden, hidden), dit.py:313
    blocks.resize(depth);
    for (int i = 0; i < depth && R.ok; ++i) {
        DitBlock& b = blocks[i];
        const std::string pre = "blocks." + std::to_string(i);
        b.mod_off = 6 * D * i;
        b.wqkv = padded(3 * D, D); b.wout = padded(D, D); b.fc1w = padded(hid, D); b.fc2w = padded(D, hid);
        if (x3_linear) { b.xqkv = planes(3 * D, D); b.xout = planes(D, D); b.xfc1 = planes(hid, D); b.xfc2 = planes(D, hid); }
        if (!R.ok) break;
        R.reg_f32(pre + ".attn.to_q.weight", (int64_t)D * D, b.wqkv);
        R.reg_f32(pre + ".attn.to_kv.weight", (int64_t)2 * D * D, b.wqkv + (size_t)D * D);
        R.reg_f32(pre + ".attn.to_context.weight", (int64_t)2 * D * D, ctx);
        R.reg_f32(pre + ".attn.to_out.weight", (int64_t)D * D, b.wout);
        R.reg_f32(pre + ".mlp.fc1.weight", (int64_t)hid * D, b.fc1w);
        b.fc1b = R.reg_f32(pre + ".mlp.fc1.bias", hid);
        R.reg_f32(pre + ".mlp.fc2.weight", (int64_t)D * hid, b.fc2w);
        b.fc2b = R.reg_f32(pre + ".mlp.fc2.bias", D);
        R.reg_f32(pre + ".adaLN_modulation.1.weight", (int64_t)6 * D * D, h->film_w + (size_t)b.mod_off * D);
        R.reg_f32(pre + ".adaLN_modulation.1.bias", 6 * D, h->film_b + b.mod_off);
    }
    fin_mod_off = 6 * D * depth;
    fin_w = padded(nout, D);
    if (R.ok) {
        R.reg_f32("final_layer.linear.weight", (int64_t)nout * D, fin_w);
        fin_b = R.reg_f32("final_layer.linear.bias", nout);
        R.reg_f32("final_layer.adaLN_modulation.1.weight", (int64_t)2 * D * D, h->film_w + (size_t)fin_mod_off * D);
        R.reg_f32("final_layer.adaLN_modulation.1.bias", 2 * D, h->film_b + fin_mod_off);
    }
    return R.ok ? 0 : fail(h, "device allocation failed while building the weight registry");
}

// f32x3: the hi / lo planes of every block linear from the fp32 buffers (stream-ordered behind the loads)
int DitNet::prepare(adf_handle* h, hipStream_t s) {
    if (!x3_linear || split_done) return 0;
    for (const DitBlock& b : blocks) {
        const std::pair<const float*, const X3W*> ws[4] = {{b.wqkv, &b.xqkv}, {b.wout, &b.xout}, {b.fc1w, &b.xfc1}, {b.fc2w, &b.xfc2}};
        for (const auto& w : ws)
            if (const char* e = launch_dit_split_weight(w.first, w.second->hi, w.second->lo, w.second->numel, s)) return fail(h, e);
    }
    split_done = true;
    return 0;
}

// DiT.forward (dit.py:382-429); x / out are the reference's [B][C][H][W] fp32 (H = 1 for the [B][C][L] form)
int DitNet::forward(adf_handle* h, Plan* p, const FwdIO& io, hipStream_t s) {
    Walker W{h, p, s};
    if (W.begin()) return 1;
    const int B = p->B, M = B * T, depth = cfg.depth;
    auto falloc = [&](size_t n) { return (float*)W.alloc(n * 4); };
    auto linear = [&](const float* x, const float* w, const float* bias, float* y, int m, int n, int k, int epi, const float* res, const float* gate,
                      int gate_bs, float* pre = nullptr, const X3W* xw = nullptr) {
        if (!W.live()) return;
        DitLinearArgs a;
        a.x = x; a.w = w; a.bias = bias; a.y = y; a.M = m; a.N = n; a.K = k; a.epi = epi; a.res = res; a.gate = gate; a.gate_bstride = gate_bs; a.T = T; a.pre = pre;
        W.check(xw && x3_linear ? launch_dit_linear_x3(a, xw->hi, xw->lo, s) : launch_dit_linear(a, s));
    };
    // ---- c = t_embedder(t) (+ y_embedder(classes)), then every adaLN_modulation in one GEMM; an unconditional sampler run brings the rows of this
    // evaluation already projected (film_pre: Plan::film_all, filled at the head of the run)
    float* cbuf = falloc((size_t)B * D);
    float* scbuf = falloc((size_t)B * D);
    const float* mod = io.film_pre ? io.film_pre : p->film;
    int mod_bs = io.nb > 1 ? h->film_total : 0;
    if (h->cdim > 0 || !io.film_pre) {
        const bool labels = h->cdim > 0 && h->cond_on && h->cond_B == B && h->cond_emb;       // (not in a plan's warm-up pass before any adf_set_condition)
        const int rows = h->cdim > 0 ? B : io.nb;
        mod = p->film;
        mod_bs = rows > 1 ? h->film_total : 0;
        if (W.live()) {
            const float* te = io.temb_pre;
            int te_bs = 0;
            if (!te) {
                W.check(time_embed(io.t, io.t_stride, io.nb, p->temb, s));
                te = p->temb; te_bs = io.nb > 1 ? D : 0;
            }
            const float* ce = !labels ? nullptr : (io.null_cond ? h->cond_emb + (size_t)B * D : h->cond_emb);      // last row = the null embedding
            W.check(launch_dit_cond(cbuf, scbuf, te, te_bs, ce, io.null_cond ? 0 : D, rows, D, s));
        }
        linear(scbuf, h->film_w, h->film_b, p->film, rows, h->film_total, D, kDitEpiBias, nullptr, nullptr, 0);
        if (rows == B) W.tap("c", Act{cbuf, D, 1});
    }
    // ---- x = x_embedder(c_in x) + pos_embed
    float* x = falloc((size_t)M * D);
    if (W.live())
        W.check(launch_dit_patch_embed(io.x, io.coef, io.coef_bstride, pe_w, pe_b, pos, x, B, cfg.in_channels, cfg.input_h, cfg.input_w, cfg.patch_h,
                                       cfg.patch_w, D, s));
    W.tap("x_embedder", Act{x, D, T});
    float* xn = falloc((size_t)M * D);
    float* qkv = falloc((size_t)M * 3 * D);
    float* att = falloc((size_t)M * D);
    float* hb = falloc((size_t)M * hid);
    // the block outputs and both branches before their gates stay readable as taps while they fit 512 MiB; beyond that x is updated in place
    const bool keep = block_taps && (size_t)3 * depth * M * D * 4 <= ((size_t)512 << 20);
    float* xmid = keep ? falloc((size_t)M * D) : nullptr;
    float* xres = keep ? nullptr : falloc((size_t)M * D);      // in place from the first gated epilogue on; the x_embedder tap keeps its own buffer
    for (int i = 0; i < depth && !W.bad; ++i) {
        const DitBlock& b = blocks[i];
        const std::string bn = "blocks." + std::to_string(i);
        const float* m6 = mod + b.mod_off;          // shift_msa | scale_msa | gate_msa | shift_mlp | scale_mlp | gate_mlp (dit.py:251)
        if (W.live()) W.check(launch_dit_ln_modulate(x, xn, m6, m6 + D, mod_bs, M, T, D, s));
        linear(xn, b.wqkv, nullptr, qkv, M, 3 * D, D, kDitEpiBias, nullptr, nullptr, 0, nullptr, &b.xqkv);
        // Attention's plain branch (attention_utils.py:157-184): softmax(q k^T / sqrt(head dim)) v on q | k | v blocks
        if (W.live()) W.check(x3_att ? launch_dit_attention_x3(qkv, att, B, T, D, cfg.num_heads, s) : launch_attention(qkv, att, 0, B, T, D, cfg.num_heads, s));
        float* xm = keep ? xmid : xres;
        float* xo = keep ? falloc((size_t)M * D) : xres;
        float* ab = keep ? falloc((size_t)M * D) : nullptr;                 // the attention branch before its gate
        linear(att, b.wout, nullptr, xm, M, D, D, kDitEpiGate, x, m6 + 2 * D, mod_bs, ab, &b.xout);
        if (keep) W.tap(bn + ".attn", Act{ab, D, T});
        if (W.live()) W.check(launch_dit_ln_modulate(xm, xn, m6 + 3 * D, m6 + 4 * D, mod_bs, M, T, D, s));
        linear(xn, b.fc1w, b.fc1b, hb, M, hid, D, kDitEpiGelu, nullptr, nullptr, 0, nullptr, &b.xfc1);
        float* mb = keep ? falloc((size_t)M * D) : nullptr;
        linear(hb, b.fc2w, b.fc2b, xo, M, D, hid, kDitEpiGate, xm, m6 + 5 * D, mod_bs, mb, &b.xfc2);
        if (keep) W.tap(bn + ".mlp", Act{mb, D, T});
        x = xo;
        if (keep) W.tap(bn, Act{x, D, T});
    }
    // ---- FinalLayer (dit.py:271-275) and unpatchify with the denoiser epilogue
    const float* m2 = mod + fin_mod_off;
    float* lin = falloc((size_t)M * nout);
    if (W.live()) W.check(launch_dit_ln_modulate(x, xn, m2, m2 + D, mod_bs, M, T, D, s));
    linear(xn, fin_w, fin_b, lin, M, nout, D, kDitEpiBias, nullptr, nullptr, 0);
    W.tap("final_layer", Act{lin, nout, T});
    if (W.live())
        W.check(launch_dit_unpatchify(lin, io.out, B, cfg.in_channels, cfg.input_h, cfg.input_w, cfg.patch_h, cfg.patch_w, io.mode, io.x_noisy, io.coef,
                                      io.coef_bstride, s));
    return W.bad ? 1 : 0;
}

}  // namespace adf_api

extern "C" int adf_dit_create(const adf_dit_config* cfg, adf_handle** out) {
    if (create_begin("adf_dit_create", cfg, out)) return 1;
    const adf_dit_config& c = *cfg;
    auto bad = [&](const char* m) { g_create_error = std::string("adf_dit_create: ") + m; return 1; };
    if (c.dtype != ADF_DTYPE_F32 && c.dtype != ADF_DTYPE_F32X3) return bad("dtype must be ADF_DTYPE_F32 or ADF_DTYPE_F32X3 (no bf16-storage DiT)");
    if (c.input_h < 1 || c.input_w < 1 || c.patch_h < 1 || c.patch_w < 1 || c.input_h % c.patch_h || c.input_w % c.patch_w)
        return bad("input_size must be positive and divisible by patch_size");
    if (c.in_channels < 1 || (long long)c.in_channels * c.patch_h * c.patch_w < 4 || (long long)c.in_channels * c.patch_h * c.patch_w > 256)
        return bad("prod(patch_size) * in_channels must lie in [4, 256]");
    if (c.hidden_size < 64 || c.hidden_size % 64 || c.hidden_size > 1024) return bad("hidden_size must be a multiple of 64, at most 1024");
    if (c.num_heads < 1 || c.hidden_size % c.num_heads || (c.hidden_size / c.num_heads != 32 && c.hidden_size / c.num_heads != 64))
        return bad("num_heads must give a head dim (hidden_size / num_heads) of 32 or 64");
    if (c.mlp_hidden < 32 || c.mlp_hidden % 32 || c.mlp_hidden > 4096) return bad("mlp_hidden = int(hidden_size * mlp_ratio) must be a multiple of 32, at most 4096");
    if (c.depth < 1 || c.depth > 64) return bad("depth must lie in [1, 64]");
    if (c.num_classes < 0) return bad("num_classes must be >= 0");
    const long long tokens = (long long)(c.input_h / c.patch_h) * (c.input_w / c.patch_w);
    if (tokens > (1 << 20)) return bad("too many tokens");
    auto net = std::make_unique<DitNet>();
    net->cfg = c;
    net->block_taps = adf_route_switch("ADF_DIT_TAPS", 1) != 0;
    net->x3_linear = c.dtype == ADF_DTYPE_F32X3 && adf_route_switch("ADF_DIT_X3_LINEAR", 1) != 0;
    net->x3_att = c.dtype == ADF_DTYPE_F32X3 && adf_route_switch("ADF_DIT_X3_ATT", 1) != 0;
    net->D = c.hidden_size; net->T = (int)tokens; net->hid = c.mlp_hidden; net->nout = c.patch_h * c.patch_w * c.in_channels;
    NetDims& d = net->dims;
    d.in_channels = d.out_channels = c.in_channels;
    d.temb = c.hidden_size; d.label_in = c.hidden_size; d.num_classes = c.num_classes;
    return create_finish("adf_dit_create", c.dtype, std::move(net), out);
}
