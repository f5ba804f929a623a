// Imagen-style UNet2dBase behind the C ABI (reference: src/models/backbones/unet2d.py:622-972), exact fp32: adf_unet2d_create, registry and the block walk.
// The convs and linears go through launch_conv2d (launch_u2d_conv_small below 64 pixels per image), GroupNorm tables through
// launch_gn_finalize_fine; the layers the ADM net has no kernel for are in adf_unet2d.hip.
#include "adf_walk2d.h"

using namespace adf;
using namespace adf_api;

namespace adf_api {

// Imagen-style UNet2dBase (unet2d.py:622-972): the module tree of the memory-efficient layout as data
struct U2dRes {
    int cin = 0, cout = 0, skip_c = 0, film_off = 0;   // skip_c: channels of the (scaled) skip half of the input (up blocks), 0 otherwise
    float *g1w = nullptr, *g1b = nullptr, *g2w = nullptr, *g2b = nullptr;
    ConvW c1, c2, res;
    bool has_res = false, gca = false;
    int gca_hid = 0;
    float *gk_w = nullptr, *gk_b = nullptr, *gn0_w = nullptr, *gn0_b = nullptr, *gn2_w = nullptr, *gn2_b = nullptr;
};
struct U2dTrLayer { ConvW qkv, out, ff1, ff2; float *g0 = nullptr, *g3 = nullptr; };
struct U2dTr { int c = 0, hid = 0, heads = 0; std::vector<U2dTrLayer> layers; float* norm_g = nullptr; };
struct U2dLevel {
    int din = 0, dout = 0;
    ConvW down;                          // Downsample's 1x1 conv over unshuffled channels, packed as a 3x3 / stride-2 conv (slot kind 6)
    std::vector<U2dRes> down_rb, up_rb;  // [0] = the block without a gate (ds_block.1 / us_block.0), then the gated ones
    bool attn = false;
    U2dTr down_tr, up_tr;
    ConvW up;                            // PixelShuffleUpsample's 1x1 conv dout -> 4 din
};
struct Unet2dNet : Net {
    adf_unet2d_config cfg;
    int init_dim = 0, tcd = 0, fg = 4;
    int ce_off[5] = {0};
    float *ce_w[4] = {nullptr}, *ce_b[4] = {nullptr};
    float *fourier = nullptr, *t_w1 = nullptr, *t_b1 = nullptr, *t_w2 = nullptr, *t_b2 = nullptr;
    U2dRes init_rb, mid1, mid2, final_rb;
    U2dTr mid_tr;
    std::vector<U2dLevel> lv;
    float *out_w = nullptr, *out_b = nullptr;

    Unet2dNet() { class_in_temb = true; unclipped_epilogue = true; image = true; }
    int build_weights(adf_handle* h) override;
    int check_image(adf_handle* h, int L) override;
    int forward(adf_handle* h, Plan* p, const FwdIO& io, hipStream_t s) override;
    const char* time_embed(const float* t, int t_stride, int n, float* temb, hipStream_t s) override {
        return launch_u2d_time_embed(t, t_stride, n, fourier, cfg.learned_sinu_pos_emb_dim / 2, t_w1, t_b1, t_w2, t_b2, tcd, temb, s);
    }
};

int Unet2dNet::check_image(adf_handle* h, int L) {
    const int f = 1 << cfg.n_levels;
    if (H < 1 || W < 1 || (long long)H * W != L) return fail(h, "UNet2dBase: call adf_set_image_shape(H, W) with H * W equal to the length argument first");
    if (H % f || W % f) return fail(h, "UNet2dBase: H and W must be multiples of 2^levels");
    return 0;
}

// ---- registry: the registration order of UNet2dBase.__init__ (:679-876) ------------------------------------------------------------
int Unet2dNet::build_weights(adf_handle* h) {
    Unet2dNet& u = *this;
    const adf_unet2d_config& c = cfg;
    const int n = c.n_levels, tcd = u.tcd, cd = c.cond_dim;
    std::vector<int> dims{u.init_dim};
    for (int i = 0; i < n; ++i) dims.push_back(c.dim * c.dim_mults[i]);
    // pass 1: structure and FiLM row offsets (every resnet block has a time_mlp: Linear(tcd, 2 dout), :116-119)
    auto new_rb = [&](int cin, int cout, int skip_c, bool gca) {
        U2dRes r; r.cin = cin; r.cout = cout; r.skip_c = skip_c; r.has_res = cin != cout; r.gca = gca;
        r.gca_hid = std::max(3, cout / 2);
        r.film_off = h->film_total; h->film_total += 2 * cout;
        return r;
    };
    auto new_tr = [&](int ch, int depth, double ff_mult) {
        U2dTr t; t.c = ch; t.hid = (int)(ch * ff_mult); t.heads = c.attn_heads; t.layers.resize(depth);
        return t;
    };
    u.init_rb = new_rb(u.init_dim, u.init_dim, 0, true);
    u.lv.resize(n);
    for (int i = 0; i < n; ++i) {
        U2dLevel& L = u.lv[i];
        L.din = dims[i]; L.dout = dims[i + 1]; L.attn = c.layer_attns[i] != 0;
        L.down_rb.push_back(new_rb(L.dout, L.dout, 0, false));
        for (int j = 0; j < c.num_resnet_blocks; ++j) L.down_rb.push_back(new_rb(L.dout, L.dout, 0, true));
        if (L.attn) L.down_tr = new_tr(L.dout, c.layer_attns_depth, c.ff_mult);
    }
    const int mid = dims[n];
    u.mid1 = new_rb(mid, mid, 0, false);
    if (c.attend_at_middle) u.mid_tr = new_tr(mid, c.layer_mid_attns_depth, 2.0);
    u.mid2 = new_rb(mid, mid, 0, false);
    for (int i = 0; i < n; ++i) {
        U2dLevel& L = u.lv[n - 1 - i];                 // skip widths equal dout in the memory-efficient layout
        L.up_rb.push_back(new_rb(2 * L.dout, L.dout, L.dout, false));
        for (int j = 0; j < c.num_resnet_blocks; ++j) L.up_rb.push_back(new_rb(2 * L.dout, L.dout, L.dout, true));
        if (L.attn) L.up_tr = new_tr(L.dout, c.layer_attns_depth, c.ff_mult);
    }
    if (c.final_resnet_block) u.final_rb = new_rb(c.dim, c.dim, 0, true);
    {   // fine statistics group: gcd of every GroupNorm group size (incl. the concat inputs) and of the concat split, at most 4
        auto gcd = [](int x, int y) { while (y) { const int t = x % y; x = y; y = t; } return x; };
        const int G = c.resnet_groups;
        int g = 4;
        auto add = [&](const U2dRes& r) { g = gcd(g, r.cin / G); g = gcd(g, r.cout / G); if (r.skip_c) g = gcd(g, r.skip_c); };
        add(u.init_rb); add(u.mid1); add(u.mid2);
        if (c.final_resnet_block) add(u.final_rb);
        for (const U2dLevel& L : u.lv) { for (const U2dRes& r : L.down_rb) add(r); for (const U2dRes& r : L.up_rb) add(r); }
        u.fg = g < 1 ? 1 : g;
    }
    // pass 2: registry
    Registrar R{h};
    h->film_w = (float*)dalloc(h, (size_t)h->film_total * tcd * 4);
    h->film_b = (float*)dalloc(h, (size_t)h->film_total * 4);
    if (!h->film_w || !h->film_b) R.ok = false;
    auto unused = [&](const std::string& name, int64_t numel) { (void)R.reg_f32(name, numel); };     // in the state dict, never run (c = None)
    for (int i = 0; i < c.n_init_kernels; ++i) {           // CrossEmbedLayer (:261-282)
        const int k = c.init_kernel_sizes[i], ds = u.ce_off[i + 1] - u.ce_off[i];
        u.ce_w[i] = R.reg_f32("init_conv.convs." + std::to_string(i) + ".weight", (int64_t)ds * c.channels * k * k);
        u.ce_b[i] = R.reg_f32("init_conv.convs." + std::to_string(i) + ".bias", ds);
    }
    const int half = c.learned_sinu_pos_emb_dim / 2;
    u.fourier = R.reg_f32("to_time_hiddens.0.weights", half);
    u.t_w1 = R.reg_f32("to_time_hiddens.1.weight", (int64_t)tcd * (2 * half + 1));
    u.t_b1 = R.reg_f32("to_time_hiddens.1.bias", tcd);
    u.t_w2 = R.reg_f32("to_time_cond.0.weight", (int64_t)tcd * tcd);
    u.t_b2 = R.reg_f32("to_time_cond.0.bias", tcd);
    unused("to_time_tokens.0.weight", (int64_t)cd * c.num_time_tokens * tcd);
    unused("to_time_tokens.0.bias", (int64_t)cd * c.num_time_tokens);
    if (c.num_classes > 0) R.label_embedder(c.dim, 4 * c.dim, c.num_classes);      // LabelEmbedder(num_classes, dim, 4 dim) (:717-727, conditioner.py:65-90)
    // ResnetBlock.__init__ :106-144: time_mlp, cross_attn, block1, block2, gca, res_conv
    auto reg_rb = [&](const std::string& pre, U2dRes& r, bool cross) {
        R.reg_f32(pre + ".time_mlp.1.weight", (int64_t)2 * r.cout * tcd, h->film_w + (size_t)r.film_off * tcd);
        R.reg_f32(pre + ".time_mlp.1.bias", 2 * r.cout, h->film_b + r.film_off);
        if (cross) {
            unused(pre + ".cross_attn.to_q.weight", (int64_t)r.cout * r.cout);
            unused(pre + ".cross_attn.to_kv.weight", (int64_t)2 * r.cout * r.cout);
            unused(pre + ".cross_attn.to_context.weight", (int64_t)2 * r.cout * cd);
            unused(pre + ".cross_attn.to_out.weight", (int64_t)r.cout * r.cout);
        }
        r.g1w = R.reg_f32(pre + ".block1.groupnorm.weight", r.cin);
        r.g1b = R.reg_f32(pre + ".block1.groupnorm.bias", r.cin);
        R.conv(pre + ".block1.project", r.c1, r.cout, r.cin, 9, true);
        r.g2w = R.reg_f32(pre + ".block2.groupnorm.weight", r.cout);
        r.g2b = R.reg_f32(pre + ".block2.groupnorm.bias", r.cout);
        R.conv(pre + ".block2.project", r.c2, r.cout, r.cout, 9, true);
        if (r.gca) {
            r.gk_w = R.reg_f32(pre + ".gca.to_k.weight", r.cout);
            r.gk_b = R.reg_f32(pre + ".gca.to_k.bias", 1);
            r.gn0_w = R.reg_f32(pre + ".gca.net.0.weight", (int64_t)r.gca_hid * r.cout);
            r.gn0_b = R.reg_f32(pre + ".gca.net.0.bias", r.gca_hid);
            r.gn2_w = R.reg_f32(pre + ".gca.net.2.weight", (int64_t)r.cout * r.gca_hid);
            r.gn2_b = R.reg_f32(pre + ".gca.net.2.bias", r.cout);
        }
        if (r.has_res) {
            R.conv(pre + ".res_conv", r.res, r.cout, r.cin, 1, true);
            const float s = c.scale_skip_connection ? 0.70710678118654752440f : 1.0f;
            if (r.skip_c && s != 1.0f) {
                // the 2^-1/2 of the skip half of cat(x, skip * s) (:530-535) folded into the weight columns that read it
                Slot& sl = h->slots[pre + ".res_conv.weight"];
                sl.frag = dalloc(h, (size_t)r.cout * r.cin * 4);
                if (!sl.frag) R.ok = false;
                sl.kind = 6; sl.xmode = 1; sl.xc0 = r.cin - r.skip_c; sl.xscale = s;
            }
        }
    };
    // TransformerBlock.__init__ :198-217: to_q and to_kv share one packed [3C, C] operand (q | k | v rows, the layout of the attention kernels)
    auto reg_tr = [&](const std::string& pre, U2dTr& t, bool context) {
        for (size_t d = 0; d < t.layers.size(); ++d) {
            U2dTrLayer& Ly = t.layers[d];
            const std::string lp = pre + ".layers." + std::to_string(d);
            R.reg_pack(lp + ".0.to_q.weight", Ly.qkv, t.c, t.c, 1, 0, 3 * t.c, false, 0);
            R.reg_pack(lp + ".0.to_kv.weight", Ly.qkv, 2 * t.c, t.c, 1, t.c, 3 * t.c, false, 0);
            Ly.qkv.cout = 3 * t.c;
            if (context) unused(lp + ".0.to_context.weight", (int64_t)2 * t.c * cd);
            R.conv(lp + ".0.to_out", Ly.out, t.c, t.c, 1, false);
            Ly.g0 = R.reg_f32(lp + ".1.0.g", t.c);
            R.conv(lp + ".1.1", Ly.ff1, t.hid, t.c, 1, false);
            Ly.g3 = R.reg_f32(lp + ".1.3.g", t.hid);
            R.conv(lp + ".1.4", Ly.ff2, t.c, t.hid, 1, false);
        }
        t.norm_g = R.reg_f32(pre + ".norm.g", t.c);
    };
    reg_rb("init_resnet_block", u.init_rb, false);
    for (int i = 0; i < n; ++i) {
        U2dLevel& L = u.lv[i];
        const std::string pre = "downs." + std::to_string(i) + ".ds_block";
        // Downsample :57-64 (pixel unshuffle + 1x1 conv), packed as the equivalent 3x3 / stride-2 conv over the original channels
        R.reg_pack(pre + ".0.1.weight", L.down, L.dout, L.din, 9, 0, L.dout, false, 0);
        L.down.bias = R.reg_f32(pre + ".0.1.bias", L.dout);
        {
            Slot& sl = h->slots[pre + ".0.1.weight"];
            sl.numel = (int64_t)L.dout * L.din * 4;
            sl.frag = dalloc(h, (size_t)L.dout * L.din * 9 * 4);
            if (!sl.frag) R.ok = false;
            sl.kind = 6; sl.xmode = 0;
        }
        reg_rb(pre + ".1", L.down_rb[0], c.layer_cross_attns[i] != 0);
        for (int j = 0; j < c.num_resnet_blocks; ++j) reg_rb(pre + ".2." + std::to_string(j), L.down_rb[1 + j], false);
        if (L.attn) reg_tr(pre + ".3", L.down_tr, true);
    }
    reg_rb("mid_block.mid_block1", u.mid1, true);
    if (c.attend_at_middle) reg_tr("mid_block.mid_attn", u.mid_tr, false);
    reg_rb("mid_block.mid_block2", u.mid2, true);
    for (int i = 0; i < n; ++i) {
        const int li = n - 1 - i;
        U2dLevel& L = u.lv[li];
        const std::string pre = "ups." + std::to_string(i) + ".us_block";
        reg_rb(pre + ".0", L.up_rb[0], c.layer_cross_attns[li] != 0);
        for (int j = 0; j < c.num_resnet_blocks; ++j) reg_rb(pre + ".1." + std::to_string(j), L.up_rb[1 + j], false);
        if (L.attn) reg_tr(pre + ".2", L.up_tr, true);
        R.conv(pre + ".3.net.0", L.up, 4 * L.din, L.dout, 1, true);          // PixelShuffleUpsample :27-55
    }
    if (c.final_resnet_block) reg_rb("final_res_block", u.final_rb, false);
    u.out_w = R.reg_f32("final_conv.weight", (int64_t)c.channels_out * c.dim * 9);
    u.out_b = R.reg_f32("final_conv.bias", c.channels_out);
    return R.ok ? 0 : fail(h, "device allocation failed while building the weight registry");
}

// ---- UNet2dBase.forward (:879-972) for text_embeds = None, inj_channels = None, on channels-last fp32 activations --------------------
int Unet2dNet::forward(adf_handle* h, Plan* p, const FwdIO& io, hipStream_t s) {
    Unet2dNet& u = *this;
    const adf_unet2d_config& c = cfg;
    // the 2^-1/2 of the skip half of cat(x, skip * s) (:530-535) enters the GroupNorm table; images below 64 pixels take the small conv route
    Walk2d W{{h, p, s}, c.resnet_groups, fg, c.scale_skip_connection ? 0.70710678118654752440f : 1.0f, true, false};
    if (W.begin()) return 1;
    // conditioning (:898-908): t = to_time_cond(to_time_hiddens(c_noise)) (+ the label embedding), then every block's time_mlp (SiLU -> Linear)
    W.condition(io);
    const int B = p->B;
    const float* const film = W.film;
    // ResnetBlock.forward :147-168 (cond = None): block1, block2 with the time scale-shift, gca gate, residual
    auto resblock = [&](T2 x, const U2dRes& r, const std::string& name) -> T2 {
        if (x.t.C + x.t1.C != r.cin) { W.check("UNet2dBase: resnet block input width mismatch"); return x; }
        const float* ab1 = W.gn_table(x, r.g1w, r.g1b, nullptr);
        T2 h1 = W.conv(x, r.c1, ab1, 1, 0, nullptr, true);
        W.tap(name + ".h1", h1.t);
        const float* ab2 = W.gn_table(h1, r.g2w, r.g2b, film + r.film_off);
        const void* res = x.t.p;
        if (r.has_res) {
            T2 rr = W.conv(x, r.res, nullptr, 0, 0, nullptr, false);      // skip scale folded into its weight columns
            W.tap(name + ".res", rr.t);
            res = rr.t.p;
        } else if (x.t1.C) { W.check("UNet2dBase: identity residual over a concat"); return x; }
        if (!r.gca) {
            T2 y = W.conv(h1, r.c2, ab2, 1, 0, res, true);
            W.tap(name, y.t);
            return y;
        }
        T2 h2 = W.conv(h1, r.c2, ab2, 1, 0, nullptr, false);
        W.tap(name + ".h2", h2.t);
        const int L = h2.t.L, C = r.cout;
        float* part = (float*)W.alloc((size_t)B * u2d_gca_chunks(L) * (C + 2) * 4);
        float* gate = (float*)W.alloc((size_t)B * C * 4);
        T2 y; y.H = h2.H; y.W = h2.W; y.t = W.new_act(C, L); y.st = W.alloc_fine(C);
        if (W.live()) {
            W.check(launch_u2d_gca_pool((const float*)h2.t.p, r.gk_w, r.gk_b, B, L, C, part, s));
            W.check(launch_u2d_gca_gate(part, B, L, C, r.gca_hid, r.gn0_w, r.gn0_b, r.gn2_w, r.gn2_b, gate, s));
            W.check(launch_u2d_gate_residual((const float*)h2.t.p, gate, (const float*)res, (float*)y.t.p, B, L, C, y.st, fg, s));
        }
        W.tap(name, y.t);
        return y;
    };
    // TransformerBlock.forward :219-232 (no context): x = attn(norm(x)) + x (one shared norm), x = ff(x) + x; tokens = pixels (channels-last)
    auto transformer = [&](T2 x, const U2dTr& t, const std::string& name) -> T2 {
        const long long rows = (long long)B * x.t.L;
        for (size_t d = 0; d < t.layers.size() && !W.bad; ++d) {
            const U2dTrLayer& Ly = t.layers[d];
            const std::string ln = name + ".layers." + std::to_string(d);
            const bool last = d + 1 == t.layers.size();
            T2 xn = x; xn.st = nullptr; xn.t = W.new_act(t.c, x.t.L);
            if (W.live()) W.check(launch_ln_rows(x.t.p, xn.t.p, 0, rows, t.c, t.norm_g, nullptr, 1e-5f, s));
            T2 qkv = W.conv(xn, Ly.qkv, nullptr, 0, 0, nullptr, false);
            W.tap(ln + ".qkv", qkv.t);
            T2 att = xn; att.t = W.new_act(t.c, x.t.L);
            if (W.live())
                W.check(t.c / t.heads == 128 ? launch_u2d_attention_d128((const float*)qkv.t.p, (float*)att.t.p, B, x.t.L, t.c, t.heads, s)
                                             : launch_attention(qkv.t.p, att.t.p, 0, B, x.t.L, t.c, t.heads, s));
            W.tap(ln + ".att", att.t);
            T2 x1 = W.conv(att, Ly.out, nullptr, 0, 0, x.t.p, false);
            W.tap(ln + ".x1", x1.t);
            T2 n1 = x1; n1.t = W.new_act(t.c, x.t.L);
            if (W.live()) W.check(launch_ln_rows(x1.t.p, n1.t.p, 0, rows, t.c, Ly.g0, nullptr, 1e-5f, s));
            T2 f1 = W.conv(n1, Ly.ff1, nullptr, 0, 0, nullptr, false);
            T2 n2 = f1; n2.t = W.new_act(t.hid, x.t.L);
            if (W.live()) W.check(launch_u2d_gelu_ln_rows((const float*)f1.t.p, (float*)n2.t.p, rows, t.hid, Ly.g3, 1e-5f, s));
            x = W.conv(n2, Ly.ff2, nullptr, 0, 0, x1.t.p, last);
            W.tap(ln, x.t);
        }
        W.tap(name, x.t);
        return x;
    };
    // :890-892 initial convolution: CrossEmbedLayer with c_in fused, and the fine statistics init_resnet_block.block1 reads
    T2 x; x.H = H; x.W = this->W;
    x.t = W.new_act(u.init_dim, H * this->W);
    x.st = W.alloc_fine(u.init_dim);
    if (W.live()) {
        U2dCrossEmbedArgs ce;
        memset(&ce, 0, sizeof(ce));
        ce.x = io.x; ce.coef = io.coef; ce.coef_bstride = io.coef_bstride;
        ce.B = B; ce.cin = c.channels; ce.H = H; ce.W = this->W; ce.n = c.n_init_kernels;
        for (int i = 0; i < c.n_init_kernels; ++i) { ce.ks[i] = c.init_kernel_sizes[i]; ce.w[i] = u.ce_w[i]; ce.bias[i] = u.ce_b[i]; }
        for (int i = 0; i <= c.n_init_kernels; ++i) ce.off[i] = u.ce_off[i];
        ce.out = (float*)x.t.p; ce.stats = x.st; ce.fg = fg;
        W.check(launch_u2d_cross_embed(ce, s));
    }
    W.tap("init_conv", x.t);
    x = resblock(x, u.init_rb, "init_resnet_block");
    // :924-946 down path (DownsamplingBlock.forward :404-436, memory efficient: the downsample first)
    const int n = c.n_levels;
    std::vector<T2> hiddens;
    for (int i = 0; i < n && !W.bad; ++i) {
        const U2dLevel& L = u.lv[i];
        const std::string pre = "downs." + std::to_string(i);
        x = W.conv(x, L.down, nullptr, 0, 2, nullptr, true);
        W.tap(pre + ".down", x.t);
        x = resblock(x, L.down_rb[0], pre + ".1");
        for (int j = 0; j < c.num_resnet_blocks; ++j) {
            x = resblock(x, L.down_rb[1 + j], pre + ".2." + std::to_string(j));
            hiddens.push_back(x);
        }
        if (L.attn) x = transformer(x, L.down_tr, pre + ".3");
        hiddens.push_back(x);
        W.tap(pre, x.t);
    }
    // :948 (MiddleBlock.forward :461-469)
    x = resblock(x, u.mid1, "mid_block.mid_block1");
    if (c.attend_at_middle) x = transformer(x, u.mid_tr, "mid_block.mid_attn");
    x = resblock(x, u.mid2, "mid_block.mid_block2");
    W.tap("mid_block", x.t);
    // :950-958 up path (UpsamplingBlock.forward :524-538): cat(x, skip * 2^-1/2) per resnet block, the scale folded into the GroupNorm table and res_conv
    for (int i = 0; i < n && !W.bad; ++i) {
        const U2dLevel& L = u.lv[n - 1 - i];
        const std::string pre = "ups." + std::to_string(i);
        for (size_t j = 0; j < L.up_rb.size() && !W.bad; ++j) {
            const T2 sk = hiddens.back(); hiddens.pop_back();
            if (sk.H != x.H || sk.W != x.W) { W.check("UNet2dBase: skip shape mismatch"); break; }
            T2 cat = x;
            cat.t1 = sk.t; cat.st1 = sk.st;
            x = resblock(cat, L.up_rb[j], j == 0 ? pre + ".0" : pre + ".1." + std::to_string(j - 1));
        }
        if (L.attn) x = transformer(x, L.up_tr, pre + ".2");
        // PixelShuffleUpsample: 1x1 conv to 4 din, SiLU, pixel shuffle (statistics by the separate pass when the next GroupNorm asks)
        T2 pre_shuffle = W.conv(x, L.up, nullptr, 0, 0, nullptr, false);
        W.tap(pre + ".3.conv", pre_shuffle.t);
        T2 y; y.H = 2 * x.H; y.W = 2 * x.W; y.t = W.new_act(L.din, y.H * y.W);
        if (W.live()) W.check(launch_u2d_silu_shuffle((const float*)pre_shuffle.t.p, (float*)y.t.p, B, x.H, x.W, L.din, s));
        x = y;
        W.tap(pre, x.t);
    }
    if (!hiddens.empty() && !W.bad) W.check("UNet2dBase: unconsumed skip connections");
    if (c.final_resnet_block) x = resblock(x, u.final_rb, "final_res_block");
    // :972 final_conv (3x3, no norm, no activation) with the EDM epilogue
    if (W.live())
        W.check(launch_u2d_conv_out_raw((const float*)x.t.p, u.out_w, u.out_b, io.out, B, x.t.C, x.H, x.W, c.channels_out, io.mode, io.x_noisy, io.coef,
                                        io.coef_bstride, s));
    return W.bad ? 1 : 0;
}

}  // namespace adf_api

extern "C" int adf_unet2d_create(const adf_unet2d_config* cfg, adf_handle** out) {
    if (create_begin("adf_unet2d_create", cfg, out)) return 1;
    const adf_unet2d_config& c = *cfg;
    auto bad = [](const char* m) { g_create_error = std::string("adf_unet2d_create: ") + m; return 1; };
    if (c.dtype != ADF_DTYPE_F32) return bad("only the exact-fp32 mode (ADF_DTYPE_F32) is built for this net");
    if (c.n_levels < 1 || c.n_levels > ADF_U2D_MAX_LEVELS || c.num_resnet_blocks < 1) return bad("bad level / block counts");
    if (c.n_init_kernels < 1 || c.n_init_kernels > ADF_U2D_MAX_INIT_KERNELS) return bad("1 to 4 cross-embed kernel sizes");
    if (c.channels < 1 || c.channels_out < 1 || c.channels_out > 4) return bad("channels >= 1, 1 <= channels_out <= 4");
    if (c.dim % 32 || c.dim < 32 || c.dim > 1024 || c.cond_dim < 1 || c.cond_dim > 512 || c.resnet_groups < 1 || c.attn_heads < 1) return bad("bad widths");
    if (c.num_classes < 0 || (c.num_classes > 0 && (c.cond_dim != c.dim || c.dim > 512))) return bad("class conditioning needs cond_dim == dim <= 512");
    if (c.learned_sinu_pos_emb_dim < 2 || c.learned_sinu_pos_emb_dim % 2 || c.num_time_tokens < 1) return bad("bad time embedding widths");
    if (c.layer_attns_depth < 1 || c.layer_mid_attns_depth < 1 || !(c.ff_mult > 0.0)) return bad("bad transformer settings");
    for (int i = 0; i < c.n_levels; ++i) {
        const int w = c.dim * c.dim_mults[i];
        if (c.dim_mults[i] < 1 || w > 512 || w % c.resnet_groups) return bad("level widths must be at most 512 (a skip concat feeds a conv of at most 1024 channels) and multiples of resnet_groups");
        if (c.layer_attns[i] || c.attend_at_middle) {
            if (w % c.attn_heads) return bad("attention widths must divide into the heads");
        }
    }
    for (int i = 0; i < c.n_init_kernels; ++i)
        if (c.init_kernel_sizes[i] < 1 || !(c.init_kernel_sizes[i] & 1) || (i && c.init_kernel_sizes[i] < c.init_kernel_sizes[i - 1])) return bad("cross-embed kernel sizes must be odd and sorted");
    auto net = std::make_unique<Unet2dNet>();
    Unet2dNet& u = *net;
    u.cfg = c;
    u.init_dim = c.dim; u.tcd = 4 * c.cond_dim;
    // CrossEmbedLayer's split of init_dim over the sorted kernel sizes (:268-272): init_dim / 2, / 4, ..., the remainder to the largest
    for (int i = 0; i + 1 < c.n_init_kernels; ++i) u.ce_off[i + 1] = u.ce_off[i] + (c.dim >> (i + 1));
    u.ce_off[c.n_init_kernels] = c.dim;
    for (int i = 0; i < c.n_init_kernels; ++i)
        if (u.ce_off[i + 1] - u.ce_off[i] < 4 || (u.ce_off[i + 1] - u.ce_off[i]) % 4) return bad("every cross-embed slice must be a multiple of 4 channels");
    // (the label embedder's table has dim columns; with classes, cond_dim == dim was checked above)
    NetDims& d = u.dims;
    d.in_channels = c.channels; d.out_channels = c.channels_out;
    d.temb = u.tcd; d.label_in = c.dim; d.num_classes = c.num_classes; d.stat_groups = c.resnet_groups;
    return create_finish("adf_unet2d_create", c.dtype, std::move(net), out);
}
