// ADM-style UNetModel behind the C ABI (reference: src/models/backbones/unet2d_oai.py:382-635): adf_adm_create, registry and the block walk.
#include "adf_walk2d.h"

using namespace adf;
using namespace adf_api;

namespace adf_api {

// ADM-style 2-D U-Net (unet2d_oai.py:382-635): the module list of UNetModel.__init__ as data
struct AdmRes { int cin = 0, cout = 0, film_off = 0; float *g1w = nullptr, *g1b = nullptr, *g2w = nullptr, *g2b = nullptr; ConvW c1, c2, skip; bool has_skip = false;
                int updown = 0; };        // 1: ResBlock(up=True), 2: ResBlock(down=True) (resblock_updown, unet2d_oai.py:197-207, :249-254)
struct AdmAttn { int c = 0, heads = 0; float *gw = nullptr, *gb = nullptr; ConvW qkv, proj; float* qkv_tmp = nullptr; };
struct AdmLayer { int kind; int idx; };       // kind: 0 input conv, 1 ResBlock, 2 AttentionBlock, 3 Downsample (conv), 4 Upsample (conv), 5 average pool, 6 nearest x 2
struct AdmNet : Net {
    adf_adm_config cfg;
    std::vector<AdmRes> res;
    std::vector<AdmAttn> attn;
    std::vector<ConvW> resample;
    std::vector<std::vector<AdmLayer>> input_blocks, output_blocks;
    std::vector<AdmLayer> middle;
    std::vector<int> skip_ch;            // channels of the input-block outputs, in push order
    float *in_w = nullptr, *in_b = nullptr, *t_w1 = nullptr, *t_b1 = nullptr, *t_w2 = nullptr, *t_b2 = nullptr;
    float *out_gw = nullptr, *out_gb = nullptr, *out_w = nullptr, *out_b = nullptr;
    int input_ch = 0, final_ch = 0;
    int fg = 4;                          // channels per fine statistics group: gcd of every GroupNorm group size of the net (incl. the skip concats)

    AdmNet() { class_in_temb = true; image = true; }
    int build_weights(adf_handle* h) override;
    int check_image(adf_handle* h, int L) override;
    int forward(adf_handle* h, Plan* p, const FwdIO& io, hipStream_t s) override;
    const char* time_embed(const float* t, int t_stride, int n, float* temb, hipStream_t s) override {
        return launch_adm_time_embed(t, t_stride, n, cfg.model_channels, t_w1, t_b1, t_w2, t_b2, 4 * cfg.model_channels, temb, s);
    }
};

int AdmNet::check_image(adf_handle* h, int L) {
    int f = 1;
    for (int i = 1; i < cfg.n_mult; ++i) f *= 2;
    if (H < 1 || W < 1 || (long long)H * W != L) return fail(h, "UNetModel: call adf_set_image_shape(H, W) with H * W equal to the length argument first");
    if (H % f || W % f || ((H / f) * (W / f)) % 64)
        return fail(h, "UNetModel: H and W must be multiples of 2^(levels-1) and the coarsest level a multiple of 64 pixels");
    return 0;
}

// ---- ADM-style 2-D U-Net ---------------------------------------------------------------------------------------------
// The module list UNetModel.__init__ builds (unet2d_oai.py:467-594), registered in state_dict order.
int AdmNet::build_weights(adf_handle* h) {
    AdmNet& a = *this;
    const adf_adm_config& c = cfg;
    const int mc = c.model_channels, ted = 4 * mc;
    auto has_att = [&](int ds) { for (int i = 0; i < c.n_attention_ds; ++i) if (c.attention_ds[i] == ds) return true; return false; };
    auto heads_of = [&](int ch) { return c.num_head_channels == -1 ? c.num_heads : ch / c.num_head_channels; };
    // pass 1: structure
    auto new_res = [&](int cin, int cout) { AdmRes r; r.cin = cin; r.cout = cout; r.has_skip = cin != cout; r.film_off = h->film_total; h->film_total += (c.use_scale_shift_norm ? 2 : 1) * cout;
                                            a.res.push_back(r); return AdmLayer{1, (int)a.res.size() - 1}; };
    auto new_attn = [&](int ch) { AdmAttn t; t.c = ch; t.heads = heads_of(ch); a.attn.push_back(t); return AdmLayer{2, (int)a.attn.size() - 1}; };
    int ch = a.input_ch = c.channel_mult[0] * mc;
    a.input_blocks.push_back({AdmLayer{0, 0}});
    std::vector<int> chans{ch};
    int ds = 1;
    for (int level = 0; level < c.n_mult; ++level) {
        for (int k = 0; k < c.num_res_blocks; ++k) {
            std::vector<AdmLayer> ls{new_res(ch, c.channel_mult[level] * mc)};
            ch = c.channel_mult[level] * mc;
            if (has_att(ds)) ls.push_back(new_attn(ch));
            a.input_blocks.push_back(ls);
            chans.push_back(ch);
        }
        if (level != c.n_mult - 1) {
            if (c.resblock_updown) {                       // ResBlock(ch, ch, down=True) instead of Downsample (:515-528)
                AdmLayer l = new_res(ch, ch);
                a.res[l.idx].updown = 2;
                a.input_blocks.push_back({l});
            } else if (c.conv_resample) {
                a.resample.emplace_back();
                a.resample.back().cin = ch; a.resample.back().cout = ch;
                a.input_blocks.push_back({AdmLayer{3, (int)a.resample.size() - 1}});
            } else a.input_blocks.push_back({AdmLayer{5, 0}});
            chans.push_back(ch);
            ds *= 2;
        }
    }
    a.skip_ch = chans;
    a.middle = {new_res(ch, ch), new_attn(ch), new_res(ch, ch)};
    for (int level = c.n_mult - 1; level >= 0; --level) {
        for (int i = 0; i <= c.num_res_blocks; ++i) {
            const int ich = chans.back(); chans.pop_back();
            std::vector<AdmLayer> ls{new_res(ch + ich, mc * c.channel_mult[level])};
            ch = mc * c.channel_mult[level];
            if (has_att(ds)) ls.push_back(new_attn(ch));
            if (level && i == c.num_res_blocks) {
                if (c.resblock_updown) {                   // ResBlock(ch, ch, up=True) instead of Upsample (:575-588)
                    AdmLayer l = new_res(ch, ch);
                    a.res[l.idx].updown = 1;
                    ls.push_back(l);
                } else if (c.conv_resample) {
                    a.resample.emplace_back();
                    a.resample.back().cin = ch; a.resample.back().cout = ch;
                    ls.push_back(AdmLayer{4, (int)a.resample.size() - 1});
                } else ls.push_back(AdmLayer{6, 0});
                ds /= 2;
            }
            a.output_blocks.push_back(ls);
        }
    }
    a.final_ch = ch;
    if (a.final_ch != a.input_ch) return fail(h, "UNetModel: the last level's width must equal the first's (out conv, unet2d_oai.py:599)");
    {
        auto gcd = [](int x, int y) { while (y) { const int t = x % y; x = y; y = t; } return x; };
        int g = a.final_ch / 32;
        for (const AdmRes& r : a.res) { g = gcd(g, r.cin / 32); g = gcd(g, r.cout / 32); }
        for (const AdmAttn& t : a.attn) g = gcd(g, t.c / 32);
        for (int sc : a.skip_ch) g = gcd(g, sc);       // a concat splits at the skip's width
        // the largest power of two dividing g, at most 4: it must divide every group size (g) AND the 128-channel tile of the conv epilogue's
        // statistics (clamping g to 4 and stepping down to a divisor of 128 gave 2 for g = 3 and 4 for g = 5, 6, 7: widths 96, 160, 192, 224)
        a.fg = 1;
        while (a.fg < 4 && g > 0 && g % (2 * a.fg) == 0) a.fg *= 2;
    }
    // pass 2: registry, in the module's registration order
    Registrar R{h};
    h->film_w = (float*)dalloc(h, (size_t)h->film_total * ted * 4);
    h->film_b = (float*)dalloc(h, (size_t)h->film_total * 4);
    if (!h->film_w || !h->film_b) R.ok = false;
    a.t_w1 = R.reg_f32("time_embed.0.weight", (int64_t)ted * mc);
    a.t_b1 = R.reg_f32("time_embed.0.bias", ted);
    a.t_w2 = R.reg_f32("time_embed.2.weight", (int64_t)ted * ted);
    a.t_b2 = R.reg_f32("time_embed.2.bias", ted);
    // LabelEmbedder(num_classes, None, model_channels, 4 * model_channels), conditioner.py:64-90; unet2d_oai.py:461-468
    if (c.num_classes > 0) R.label_embedder(mc, ted, c.num_classes);
    auto reg_layer = [&](const AdmLayer& l, const std::string& pre) {
        if (l.kind == 0) {
            a.in_w = R.reg_f32(pre + ".weight", (int64_t)a.input_ch * c.in_channels * 9);
            a.in_b = R.reg_f32(pre + ".bias", a.input_ch);
        } else if (l.kind == 1) {
            AdmRes& r = a.res[l.idx];
            r.g1w = R.reg_f32(pre + ".in_layers.0.weight", r.cin);
            r.g1b = R.reg_f32(pre + ".in_layers.0.bias", r.cin);
            R.conv(pre + ".in_layers.2", r.c1, r.cout, r.cin, 9, true);
            const int ew = (c.use_scale_shift_norm ? 2 : 1) * r.cout;             // Linear(4 mc, 2 cout) or, additive conditioning, Linear(4 mc, cout) (:214-220)
            R.reg_f32(pre + ".emb_layers.1.weight", (int64_t)ew * ted, h->film_w + (size_t)r.film_off * ted);
            R.reg_f32(pre + ".emb_layers.1.bias", ew, h->film_b + r.film_off);
            r.g2w = R.reg_f32(pre + ".out_layers.0.weight", r.cout);
            r.g2b = R.reg_f32(pre + ".out_layers.0.bias", r.cout);
            R.conv(pre + ".out_layers.3", r.c2, r.cout, r.cout, 9, true);
            if (r.has_skip) R.conv(pre + ".skip_connection", r.skip, r.cout, r.cin, 1, true);
        } else if (l.kind == 2) {
            AdmAttn& t = a.attn[l.idx];
            t.gw = R.reg_f32(pre + ".norm.weight", t.c);
            t.gb = R.reg_f32(pre + ".norm.bias", t.c);
            R.conv(pre + ".qkv", t.qkv, 3 * t.c, t.c, 1, true);
            R.conv(pre + ".proj_out", t.proj, t.c, t.c, 1, true);
            if (!c.use_new_attention_order) {
                // QKVAttentionLegacy (:338-340) keeps each head's q | k | v rows together; the attention kernel reads q | k | v blocks:
                // the rows of the weight and of the bias are permuted once at load (slot kinds 4 / 5)
                t.qkv_tmp = (float*)dalloc(h, (size_t)3 * t.c * t.c * 4);
                if (!t.qkv_tmp) R.ok = false;
                Slot& sw = h->slots[pre + ".qkv.weight"]; sw.kind = 4; sw.frag = t.qkv_tmp; sw.f = t.heads;
                Slot& sb = h->slots[pre + ".qkv.bias"]; sb.kind = 5; sb.f = t.heads; sb.cout = 3 * t.c;
            }
        } else if (l.kind == 3 || l.kind == 4) {
            ConvW& w = a.resample[l.idx];
            R.conv(pre + (l.kind == 3 ? ".op" : ".conv"), w, w.cout, w.cin, 9, true);
        }                                                   // (5 / 6: AvgPool2d / nearest interpolation, no parameters)
    };
    for (size_t i = 0; i < a.input_blocks.size(); ++i)
        for (size_t j = 0; j < a.input_blocks[i].size(); ++j) reg_layer(a.input_blocks[i][j], "input_blocks." + std::to_string(i) + "." + std::to_string(j));
    for (size_t j = 0; j < a.middle.size(); ++j) reg_layer(a.middle[j], "middle_block." + std::to_string(j));
    for (size_t i = 0; i < a.output_blocks.size(); ++i)
        for (size_t j = 0; j < a.output_blocks[i].size(); ++j) reg_layer(a.output_blocks[i][j], "output_blocks." + std::to_string(i) + "." + std::to_string(j));
    a.out_gw = R.reg_f32("out.0.weight", a.final_ch);
    a.out_gb = R.reg_f32("out.0.bias", a.final_ch);
    a.out_w = R.reg_f32("out.2.weight", (int64_t)c.out_channels * a.input_ch * 9);
    a.out_b = R.reg_f32("out.2.bias", c.out_channels);
    return R.ok ? 0 : fail(h, "device allocation failed while building the weight registry");
}

// UNetModel.forward (unet2d_oai.py:603-634) on channels-last activations; x / out are the reference's [B][C][H][W] fp32
int AdmNet::forward(adf_handle* h, Plan* p, const FwdIO& io, hipStream_t s) {
    AdmNet& a = *this;
    const adf_adm_config& c = cfg;
    // GroupNorm32 (:10-21); no skip scale; every conv on the MFMA route; additive conditioning as a per-sample bias
    Walk2d W{{h, p, s}, 32, fg, 1.0f, false, true};
    if (W.begin()) return 1;
    W.condition(io);
    const int B = p->B;
    const float* const film = W.film;
    auto run = [&](const std::vector<AdmLayer>& ls, T2 x, const std::string& bname) -> T2 {
        int lj = -1;
        for (const AdmLayer& l : ls) {
            ++lj;
            const std::string ln = bname + "." + std::to_string(lj);
            if (W.bad) break;
            if (l.kind == 0) {
                T2 y; y.H = x.H; y.W = x.W; y.t = W.new_act(a.input_ch, x.H * x.W);
                y.st = W.alloc_fine(a.input_ch);   // here, so that the copy pushed on the skip stack carries them (the last output block reads them again)
                if (W.live()) W.check(launch_conv2d_in(io.x, a.in_w, a.in_b, y.t.p, h->bf16, B, c.in_channels, x.H, x.W, a.input_ch, io.coef, io.coef_bstride, y.st, fg, s));
                x = y;
                W.tap(ln, x.t);
            } else if (l.kind == 1) {                                  // ResBlock._forward, :248-272
                const AdmRes& r = a.res[l.idx];
                const float* ab1 = W.gn_table(x, r.g1w, r.g1b, nullptr);
                // scale-shift form (:262-267): the embedding enters the out_norm table; additive form (:268-270, h = out_norm(h + emb_out)): it is a
                // per-sample addend to conv1's bias, so that the stored tensor (and the statistics reduced from it) is h + emb_out
                const bool ss = c.use_scale_shift_norm != 0;
                const float* emb_b = ss ? nullptr : film + r.film_off;
                T2 hh;
                if (r.updown == 2) {
                    // ResBlock(down=True) (:249-254): h = in_conv(avg_pool(in_rest(x))), x = avg_pool(x).  The pooled activation and the pooled
                    // input are written once each (GroupNorm + SiLU fused into the first pool); conv1 then takes its input raw
                    if (x.t1.C) { W.check("ResBlock(down=True) on a skip concat"); break; }
                    T2 p1; p1.H = x.H / 2; p1.W = x.W / 2; p1.t = W.new_act(r.cin, p1.H * p1.W);
                    T2 p2 = p1; p2.t = W.new_act(r.cin, p1.H * p1.W);
                    if (W.live()) {
                        W.check(launch_avgpool2(x.t.p, ab1, 1, p1.t.p, h->bf16, B, x.H, x.W, r.cin, s));
                        W.check(launch_avgpool2(x.t.p, nullptr, 0, p2.t.p, h->bf16, B, x.H, x.W, r.cin, s));
                    }
                    hh = W.conv(p1, r.c1, nullptr, 0, 0, nullptr, true, emb_b);
                    x = p2;
                } else if (r.updown == 1) {
                    // ResBlock(up=True): h = in_conv(nearest x 2 (in_rest(x))) -- the upsampling is an index map of the conv's gather (mode 1),
                    // x = nearest x 2 (x) is written once (it is the block's residual)
                    if (x.t1.C) { W.check("ResBlock(up=True) on a skip concat"); break; }
                    hh = W.conv(x, r.c1, ab1, 1, 1, nullptr, true, emb_b);
                    T2 u2; u2.H = x.H * 2; u2.W = x.W * 2; u2.t = W.new_act(r.cin, u2.H * u2.W);
                    if (W.live()) W.check(launch_nearest_up2(x.t.p, u2.t.p, h->bf16, B, x.H, x.W, r.cin, s));
                    x = u2;
                } else hh = W.conv(x, r.c1, ab1, 1, 0, nullptr, true, emb_b);
                W.tap(ln + ".h1", hh.t);
                const float* ab2 = W.gn_table(hh, r.g2w, r.g2b, ss ? film + r.film_off : nullptr);
                const void* skip = x.t.p;
                if (r.has_skip) { T2 sk2 = W.conv(x, r.skip, nullptr, 0, 0, nullptr, false); W.tap(ln + ".skip", sk2.t); skip = sk2.t.p; }
                x = W.conv(hh, r.c2, ab2, 1, 0, skip, true);
                W.tap(ln, x.t);
            } else if (l.kind == 2) {                                   // AttentionBlock._forward, :316-322
                const AdmAttn& t = a.attn[l.idx];
                const float* ab = W.gn_table(x, t.gw, t.gb, nullptr);
                T2 xn; xn.H = x.H; xn.W = x.W; xn.t = W.new_act(t.c, x.t.L);
                if (W.live()) W.check(launch_gn_apply(x.t.p, nullptr, t.c, 0, x.t.L, B, ab, 0, xn.t.p, h->bf16, s));
                W.tap(ln + ".xn", xn.t);
                T2 qkv = W.conv(xn, t.qkv, nullptr, 0, 0, nullptr, false);
                W.tap(ln + ".qkv", qkv.t);         // q | k | v blocks (the rows were permuted at load for the legacy order)
                T2 att; att.H = x.H; att.W = x.W; att.t = W.new_act(t.c, x.t.L);
                // (split-bf16 mode: the MFMA form at head dim 32 and up to 1024 tokens, the exact kernel otherwise)
                if (W.live()) W.check(h->x3 ? launch_attention_x3(qkv.t.p, att.t.p, B, x.t.L, t.c, t.heads, s)
                                            : launch_attention(qkv.t.p, att.t.p, h->bf16, B, x.t.L, t.c, t.heads, s));
                W.tap(ln + ".att", att.t);
                x = W.conv(att, t.proj, nullptr, 0, 0, xn.t.p, true);    // the residual is the NORMALISED input (:318-322)
                W.tap(ln, x.t);
            } else if (l.kind == 5 || l.kind == 6) {                     // Downsample / Upsample without a conv (conv_resample=False, :122-125, :153-156)
                if (x.t1.C) { W.check("pooled resampling on a skip concat"); break; }
                T2 y; y.H = l.kind == 5 ? x.H / 2 : x.H * 2; y.W = l.kind == 5 ? x.W / 2 : x.W * 2;
                y.t = W.new_act(x.t.C, y.H * y.W);
                if (W.live()) W.check(l.kind == 5 ? launch_avgpool2(x.t.p, nullptr, 0, y.t.p, h->bf16, B, x.H, x.W, x.t.C, s)
                                                  : launch_nearest_up2(x.t.p, y.t.p, h->bf16, B, x.H, x.W, x.t.C, s));
                x = y;
                W.tap(ln, x.t);
            } else {
                x = W.conv(x, a.resample[l.idx], nullptr, 0, l.kind == 3 ? 2 : 1, nullptr, true);
                W.tap(ln, x.t);
            }
        }
        return x;
    };
    T2 x; x.H = H; x.W = this->W; x.t = Act{};
    std::vector<T2> hs;
    for (size_t i = 0; i < a.input_blocks.size() && !W.bad; ++i) {
        x = run(a.input_blocks[i], x, "input_blocks." + std::to_string(i));
        W.tap("input_blocks." + std::to_string(i), x.t);
        hs.push_back(x);
    }
    x = run(a.middle, x, "middle_block");
    W.tap("middle_block", x.t);
    for (size_t i = 0; i < a.output_blocks.size() && !W.bad; ++i) {
        const T2 sk = hs.back(); hs.pop_back();
        if (sk.H != x.H || sk.W != x.W) { W.check("UNetModel: skip shape mismatch"); break; }
        T2 cat = x;                                                    // [x ; skip] along channels, by reference
        cat.t1 = sk.t; cat.st1 = sk.st;
        x = run(a.output_blocks[i], cat, "output_blocks." + std::to_string(i));
        W.tap("output_blocks." + std::to_string(i), x.t);
    }
    const float* abo = W.gn_table(x, a.out_gw, a.out_gb, nullptr);
    if (W.live())
        W.check(launch_conv2d_out(x.t.p, abo, a.out_w, a.out_b, io.out, h->bf16, B, a.final_ch, x.H, x.W, c.out_channels, io.mode, io.x_noisy, io.coef,
                                  io.coef_bstride, s));
    return W.bad ? 1 : 0;
}

}  // namespace adf_api

extern "C" int adf_adm_create(const adf_adm_config* cfg, adf_handle** out) {
    if (create_begin("adf_adm_create", cfg, out)) return 1;
    const adf_adm_config& c = *cfg;
    const int kc = c.dtype == ADF_DTYPE_BF16 ? 64 : 32;
    if (c.dtype != ADF_DTYPE_F32 && c.dtype != ADF_DTYPE_BF16 && c.dtype != ADF_DTYPE_F32X3) { g_create_error = "adf_adm_create: bad dtype"; return 1; }
    if (c.n_mult < 1 || c.n_mult > ADF_ADM_MAX_LEVELS || c.num_res_blocks < 1 || c.n_attention_ds < 0 || c.n_attention_ds > ADF_ADM_MAX_LEVELS) { g_create_error = "adf_adm_create: bad level / block counts"; return 1; }
    if (c.model_channels < 32 || c.model_channels % 32 || c.model_channels % kc || c.model_channels > 256) { g_create_error = "adf_adm_create: model_channels must be a multiple of 32 (fp32, f32x3) / 64 (bf16), at most 256"; return 1; }
    if (c.in_channels < 1 || c.out_channels < 1 || c.out_channels > 4) { g_create_error = "adf_adm_create: in_channels >= 1, 1 <= out_channels <= 4"; return 1; }
    if (c.num_classes < 0) { g_create_error = "adf_adm_create: num_classes must be >= 0"; return 1; }
    for (int i = 0; i < c.n_mult; ++i) if (c.channel_mult[i] < 1) { g_create_error = "adf_adm_create: bad channel_mult"; return 1; }
    auto net = std::make_unique<AdmNet>();
    net->cfg = c;
    NetDims& d = net->dims;
    d.in_channels = c.in_channels; d.out_channels = c.out_channels;
    d.temb = 4 * c.model_channels; d.label_in = c.model_channels; d.num_classes = c.num_classes; d.stat_groups = 32;
    return create_finish("adf_adm_create", c.dtype, std::move(net), out);
}
