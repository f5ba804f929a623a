// UNet1dBase behind the C ABI: adf_create, the weight registry in the reference's state_dict order and the network walk that launches the
// fused kernels (reference: src/models/backbones/unet1d.py:771-816 UNet1d.forward, :441-468 / :542-566 Down / UpsampleBlock1d).
#include "adf_api_internal.h"

using namespace adf;
using namespace adf_api;

namespace adf_api {

struct ResW {
    int cin = 0, cout = 0, film_off = 0;
    float *g1w = nullptr, *g1b = nullptr, *g2w = nullptr, *g2b = nullptr;
    ConvW c1, c2, cr;
    bool has_res = false;
};
struct TrW {
    int c = 0, mid = 0;
    float *lnw = nullptr, *lnb = nullptr, *g0 = nullptr, *g3 = nullptr;
    ConvW qkv, proj, ff1, ff2;
};
struct DownW { ConvW down; std::vector<ResW> blocks; bool attn = false; TrW tr; int factor = 1, cin = 0, cout = 0; };
// up3: the same transposed conv as a 3-tap stride-1 conv with f * cout output columns (phase-major; [B][f L][cout] IS [B][L][f cout] in memory) -- the shape
// conv_gemm_rb_kernel<.., RAW> is written for; packed beside `up` when the factor is even and f * cout is 128 or 256 (bf16 mode)
struct UpW { std::vector<ResW> blocks; bool attn = false; TrW tr; ConvW up; ConvW up3; int factor = 1, cin = 0, cout = 0; bool nearest = false; };

struct Unet1dNet : Net {
    adf_net_config cfg;
    float *to_in_w = nullptr, *to_out_w = nullptr, *fourier = nullptr, *t_w1 = nullptr, *t_b1 = nullptr, *t_w2 = nullptr, *t_b2 = nullptr;
    std::vector<DownW> downs;
    ResW mid_pre, mid_post;
    TrW mid_tr;
    std::vector<UpW> ups;

    int build_weights(adf_handle* h) override;
    int forward(adf_handle* h, Plan* p, const FwdIO& io, hipStream_t s) override;
    const char* time_embed(const float* t, int t_stride, int n, float* temb, hipStream_t s) override {
        TimeEmbedArgs te;
        te.t = t; te.t_stride = t_stride; te.nb = n; te.ch = cfg.channels;
        te.fourier = fourier; te.w1 = t_w1; te.b1 = t_b1; te.w2 = t_w2; te.b2 = t_b2; te.temb = temb;
        return launch_time_embed(te, s);
    }
};

// the registry entries only this network has
struct Registrar1d : Registrar {
    // Strided Conv1d (kernel f*km + 1, stride f, pad f*(km/2)) folded to a stride-1 conv with km + 1 taps over
    // f*cin channels: the contiguous [L][cin] input is the same memory as [L/f][f*cin], so the fast stride-1 GEMM
    // kernels apply unchanged (the folded taps beyond the real kernel length are zero weights)
    void conv_folded(const std::string& pre, ConvW& w, int cout, int cin, int K, int f) {
        w.cin = f * cin; w.K = K; w.f = f;
        w.taps = (K - 1) / f + 1;
        w.n = cout; w.n_pad = round_up(cout, 32);
        w.nchunk = ceil_div(f * cin, h->kc);
        w.w = dalloc(h, ((size_t)w.nchunk * w.taps * w.n_pad + (size_t)kTapGroup * (w.n_pad + 128)) * kRowBytes);
        if (!w.w) { ok = false; return; }
        w.cout = cout;
        Slot s; s.kind = 3; s.dst = w.w; s.numel = (int64_t)cout * cin * K;
        s.cout = cout; s.cin = cin; s.K = K; s.f = f; s.n_offset = 0; s.n_pad = w.n_pad; s.nchunk = w.nchunk; s.taps = w.taps;
        h->names.push_back(pre + ".weight"); h->slots[pre + ".weight"] = s;
        w.bias = reg_f32(pre + ".bias", cout);
    }
    void resblock(const std::string& pre, ResW& r, int cin, int cout, int temb) {
        r.cin = cin; r.cout = cout;
        r.film_off = h->film_total;
        h->film_total += 2 * cout;
        // FiLM weights are registered later (one concatenated matrix), remember the order via names
        film_names.push_back({pre, r.film_off, 2 * cout});
        r.g1w = reg_f32(pre + ".block1.groupnorm.weight", cin);
        r.g1b = reg_f32(pre + ".block1.groupnorm.bias", cin);
        conv(pre + ".block1.project", r.c1, cout, cin, 3, true);
        r.g2w = reg_f32(pre + ".block2.groupnorm.weight", cout);
        r.g2b = reg_f32(pre + ".block2.groupnorm.bias", cout);
        conv(pre + ".block2.project", r.c2, cout, cout, 3, true);
        r.has_res = cin != cout;
        if (r.has_res) conv(pre + ".to_out", r.cr, cout, cin, 1, true);
        if (h->bf16 && (cout == 256 || cout == 128) && (cin == cout || cin == 2 * cout)) {   // fragment-major copies: adf_resblock_small.h, adf_gemm_tile.h
            const std::pair<const char*, ConvW*> m[] = {{".block1.project.weight", &r.c1}, {".block2.project.weight", &r.c2}, {".to_out.weight", &r.cr}};
            for (const auto& kv : m) {
                ConvW* w = kv.second;
                if (!w->w) continue;
                w->wfrag = dalloc(h, (size_t)w->nchunk * w->taps * w->n_pad * kRowBytes);
                if (!w->wfrag) { ok = false; return; }
                h->slots[pre + kv.first].frag = w->wfrag;
            }
        }
        (void)temb;
    }
    void transformer(const std::string& pre, TrW& t, int c, int mult) {
        t.c = c; t.mid = c * mult;
        t.lnw = reg_f32(pre + ".norm.weight", c);
        t.lnb = reg_f32(pre + ".norm.bias", c);
        reg_pack(pre + ".attention.to_q.weight", t.qkv, c, c, 1, 0, 3 * c, false, 0);
        reg_pack(pre + ".attention.to_kv.weight", t.qkv, 2 * c, c, 1, c, 3 * c, false, 0);
        t.qkv.cout = 3 * c;
        conv(pre + ".attention.to_out", t.proj, c, c, 1, false);
        t.g0 = reg_f32(pre + ".feed_forward.0.g", c);
        conv(pre + ".feed_forward.1", t.ff1, t.mid, c, 1, false);
        t.g3 = reg_f32(pre + ".feed_forward.3.g", t.mid);
        conv(pre + ".feed_forward.4", t.ff2, c, t.mid, 1, false);
        if (h->bf16) {
            for (ConvW* w : {&t.qkv, &t.proj, &t.ff1, &t.ff2}) {
                w->wfrag = dalloc(h, (size_t)w->nchunk * w->n_pad * kRowBytes);
                if (!w->wfrag) { ok = false; return; }
            }
            const std::pair<const char*, ConvW*> m[] = {{".attention.to_q.weight", &t.qkv}, {".attention.to_kv.weight", &t.qkv},
                                                       {".attention.to_out.weight", &t.proj}, {".feed_forward.1.weight", &t.ff1},
                                                       {".feed_forward.4.weight", &t.ff2}};
            for (const auto& kv : m) h->slots[pre + kv.first].frag = kv.second->wfrag;
        }
    }
    struct FilmName { std::string pre; int off, rows; };
    std::vector<FilmName> film_names;
};

// the 1-D walk's GEMM, resblock and transformer launches over the shared arenas
struct Walker1d : Walker {
    const adf_net_config& c;
    const float* film2 = nullptr;       // class part of the FiLM projections for this pass (FwdIO::film2)
    int film2_bstride = 0;
    const float* film = nullptr;        // time part: Plan::film, or the evaluation's row of Plan::film_all

    bool can_fuse_stats(int C) const {
        if (c.flags & ADF_FLAG_SEPARATE_GN_STATS) return false;
        const int G = c.resnet_groups;
        if (C % G) return false;
        const int gs = C / G;
        return (gs & (gs - 1)) == 0;
    }
    double* ensure_stats(Act& t) {
        if (!t.stats) {
            t.stats = alloc_stats();
            if (live()) check(launch_gn_stats(t.p, h->bf16, p->B, t.L, t.C, c.resnet_groups, t.stats, s));
        }
        return t.stats;
    }

    GemmArgs gemm_base(const Act& out, int lin, int mrows, const ConvW& w) {
        GemmArgs g;
        memset(&g, 0, sizeof(g));
        g.nseg = 1; g.B = p->B; g.lin = lin; g.mrows = mrows; g.n = w.n; g.n_pad = w.n_pad;
        g.bias0 = w.bias; g.bias_mod = w.n > 0 ? w.n : 1;
        g.out = out.p; g.out_rows = out.L; g.out_c = out.C;
        return g;
    }
    static GemmSeg seg_of(const Act& x, const Act* skip, const float* ab, float scale1, int act, int taps, int stride, int off0,
                          int step, const ConvW& w) {
        GemmSeg sg;
        memset(&sg, 0, sizeof(sg));
        sg.src0 = x.p; sg.c0 = x.C;
        sg.src1 = skip ? skip->p : nullptr; sg.c1 = skip ? skip->C : 0;
        sg.ab = ab; sg.scale1 = scale1; sg.act = act;
        sg.taps = taps; sg.stride = stride; sg.off0 = off0; sg.step = step;
        sg.w = w.w; sg.wfrag = w.wfrag; sg.nchunk = w.nchunk;
        return sg;
    }
    void run_gemm(GemmArgs& g, Act& out, bool want_stats) {
        const bool ask = want_stats && can_fuse_stats(out.C);      // also for the phase-scattered transposed convs
        if (ask) {
            out.stats = alloc_stats();
            g.stats = out.stats; g.stats_groups = c.resnet_groups;
        }
        if (live()) {
            bool fused = false;
            check(launch_conv_gemm(g, h->gemm_dtype(), s, &fused));
            // the launcher may decline (tile shape / group size): fill the same buffer with the separate pass
            if (ask && !fused) check(launch_gn_stats(out.p, h->bf16, p->B, out.L, out.C, c.resnet_groups, out.stats, s));
        }
    }

    Act linear(const Act& x, const ConvW& w, const void* res, int gelu, bool want_stats) {
        // a 1x1 op has no halo: run it over the flattened [B*L] rows as one long sample
        Act out = new_act(w.n, x.L);
        const int rows = p->B * x.L;
        GemmArgs g = gemm_base(out, rows, rows, w);
        g.B = 1; g.out_rows = rows;
        g.seg[0] = seg_of(x, nullptr, nullptr, 1.f, 0, 1, 1, 0, 1, w);
        g.res = res; g.gelu = gelu;
        run_gemm(g, out, false);
        (void)want_stats;   // per-sample statistics come from the separate pass (ensure_stats) when needed
        return out;
    }

    Act resblock(const std::string& name, Act& x, Act* skip, const ResW& r, int nb) {
        const int B = p->B, G = c.resnet_groups;
        const float sscale = c.use_skip_scale ? 0.70710678118654752440f : 1.0f;
        const int ctot = x.C + (skip ? skip->C : 0);
        if (ctot != r.cin) check("resblock: channel mismatch");
        double* s0 = ensure_stats(x);
        double* s1 = skip ? ensure_stats(*skip) : nullptr;
        static int short_max = -1;       // ADF_SHORT_LEVEL: longest level that materialises silu(GN(x)) for flat GEMM tiles
        if (short_max < 0) short_max = (int)adf_tuning("ADF_SHORT_LEVEL", 32);
        const bool short_level = x.L <= short_max && (x.L & (x.L - 1)) == 0;
        float* ab1 = (float*)alloc((size_t)B * ctot * 2 * 4);
        GnFinalizeArgs f1;
        memset(&f1, 0, sizeof(f1));
        f1.stats0 = s0; f1.stats1 = s1; f1.c0 = x.C; f1.c1 = skip ? skip->C : 0; f1.L = x.L; f1.G = G; f1.B = B;
        f1.scale1 = sscale; f1.eps = 1e-5f; f1.gamma = r.g1w; f1.beta = r.g1b; f1.film = nullptr; f1.ab = ab1;
        // short levels in bf16 mode: the whole resblock in one launch (adf_resblock_small.h); ADF_RB_FUSED=0 keeps the separate launches
        // (2 = four workgroups per sample in two launches when the batch leaves CUs idle, adf_resblock_split.h; 1 = always the one-launch kernel)
        static int rb_fused = -1;
        if (rb_fused < 0) rb_fused = adf_route_switch("ADF_RB_FUSED", 2);
        if (rb_fused && h->bf16 && (x.L == 16 || x.L == 64) && r.cout == 256 && x.C == 256 && (!skip || skip->C == 256) && G == 8 &&
            r.c1.wfrag && r.c2.wfrag && (!r.has_res || r.cr.wfrag) && r.c1.n_pad == 256 && !(c.flags & ADF_FLAG_SEPARATE_GN_STATS)) {
            Act y = new_act(r.cout, x.L);
            RbFusedArgs fa;
            memset(&fa, 0, sizeof(fa));
            fa.x = (const bf16_t*)x.p; fa.skip = skip ? (const bf16_t*)skip->p : nullptr; fa.out = (bf16_t*)y.p;
            fa.gn1 = f1;
            fa.gamma2 = r.g2w; fa.beta2 = r.g2b;
            fa.film = film + r.film_off; fa.film_bstride = nb == 1 ? 0 : h->film_total;
            if (film2) { fa.film2 = film2 + r.film_off; fa.film2_bstride = film2_bstride; }
            fa.w1 = r.c1.wfrag; fa.w2 = r.c2.wfrag; fa.wr = r.has_res ? r.cr.wfrag : nullptr;
            fa.b1 = r.c1.bias; fa.b2 = r.c2.bias; fa.br = r.has_res ? r.cr.bias : nullptr;
            fa.skip_scale = sscale; fa.eps = 1e-5f;
            y.stats = alloc_stats(); fa.stats = y.stats;
            if (rb_fused >= 2 && B * 4 <= 256) {
                Act hact = new_act(r.cout, x.L);
                RbSplitArgs sa;
                sa.f = fa; sa.hact = (bf16_t*)hact.p;
                if (live()) check(launch_resblock_split(sa, B, x.L, ctot, s));
            } else if (live()) check(launch_resblock_small(fa, B, x.L, ctot, s));
            RbRec rec{name, GemmArgs{}, GemmArgs{}, r.cin, r.cout, x.L};
            rec.g1.nseg = 0;                               // marks a fused block for adf_bench_resblock (keeps the block numbering)
            p->rbs.push_back(rec);
            tap(name, y);
            return y;
        }
        Act h1 = new_act(r.cout, x.L);
        GemmArgs g1 = gemm_base(h1, x.L, x.L, r.c1);
        if (short_level) {
            // short levels: one launch normalises + activates the (concatenated) input; the GEMM then takes raw tiles
            Act a1 = new_act(ctot, x.L);
            if (live()) check(launch_gn_norm_apply(x.p, skip ? skip->p : nullptr, f1, 1, a1.p, h->bf16, s));
            g1.seg[0] = seg_of(a1, nullptr, nullptr, 1.f, 0, 3, 1, -1, 1, r.c1);
        } else {
            g1.seg[0] = seg_of(x, skip, ab1, sscale, 1, 3, 1, -1, 1, r.c1);
            g1.seg[0].gn = f1;           // launch_conv_gemm derives the table (in the DMA kernel) or launches gn_finalize
        }
        run_gemm(g1, h1, true);
        tap(name + ".h1", h1);        // the block's stored intermediate (not there when the whole block is one launch)
        double* sh = ensure_stats(h1);
        float* ab2 = (float*)alloc((size_t)B * r.cout * 2 * 4);
        GnFinalizeArgs f2;
        memset(&f2, 0, sizeof(f2));
        f2.stats0 = sh; f2.c0 = r.cout; f2.L = x.L; f2.G = G; f2.B = B; f2.scale1 = 1.f; f2.eps = 1e-5f;
        f2.gamma = r.g2w; f2.beta = r.g2b;
        f2.film = film + r.film_off; f2.film_bstride = nb == 1 ? 0 : h->film_total; f2.ab = ab2;
        if (film2) { f2.film2 = film2 + r.film_off; f2.film2_bstride = film2_bstride; }
        Act y = new_act(r.cout, x.L);
        GemmArgs g2 = gemm_base(y, x.L, x.L, r.c2);
        if (short_level) {
            Act a2 = new_act(r.cout, x.L);
            if (live()) check(launch_gn_norm_apply(h1.p, nullptr, f2, 1, a2.p, h->bf16, s));
            g2.seg[0] = seg_of(a2, nullptr, nullptr, 1.f, 0, 3, 1, -1, 1, r.c2);
        } else {
            g2.seg[0] = seg_of(h1, nullptr, ab2, 1.f, 1, 3, 1, -1, 1, r.c2);
            g2.seg[0].gn = f2;
        }
        if (r.has_res) {
            g2.nseg = 2;
            g2.seg[1] = seg_of(x, skip, nullptr, sscale, 0, 1, 1, 0, 1, r.cr);
            g2.bias1 = r.cr.bias;
        } else {
            if (skip) check("resblock: identity residual with a skip input");
            g2.res = x.p;
        }
        run_gemm(g2, y, true);
        p->rbs.push_back({name, g1, g2, r.cin, r.cout, x.L});
        tap(name, y);
        return y;
    }

    Act transformer(const std::string& name, Act& x, const TrW& t) {
        const long long rows = (long long)p->B * x.L;
        // short levels in bf16 mode: the whole block in one launch (adf_transformer.h); ADF_TR_FUSED=0 keeps the nine launches
        static int tr_fused = -1;
        if (tr_fused < 0) tr_fused = adf_route_switch("ADF_TR_FUSED", 2);
        if (tr_fused && h->bf16 && t.c == 256 && t.mid == 512 && c.attention_heads == 8 && (x.L == 16 || x.L == 64) &&
            x.C == 256 && t.qkv.nchunk == 4 && t.ff2.nchunk == 8 && t.qkv.wfrag) {
            Act x2 = new_act(t.c, x.L);
            TrFusedArgs fa;
            memset(&fa, 0, sizeof(fa));
            fa.x = (const bf16_t*)x.p; fa.out = (bf16_t*)x2.p;
            fa.ln_w = t.lnw; fa.ln_b = t.lnb; fa.g0 = t.g0; fa.g3 = t.g3;
            fa.wqkv = t.qkv.wfrag; fa.wproj = t.proj.wfrag; fa.wff1 = t.ff1.wfrag; fa.wff2 = t.ff2.wfrag;
            fa.npad_qkv = t.qkv.n_pad; fa.npad_proj = t.proj.n_pad; fa.npad_ff1 = t.ff1.n_pad; fa.npad_ff2 = t.ff2.n_pad;
            fa.eps = 1e-5f;
            if (c.resnet_groups == 8 && !(c.flags & ADF_FLAG_SEPARATE_GN_STATS)) { x2.stats = alloc_stats(); fa.stats = x2.stats; }
            if (live()) check(launch_transformer_small(fa, p->B, x.L, s));
            tap(name, x2);
            return x2;
        }
        // longer samples (256 tokens): two fused launches around the attention kernel (ADF_TR_FUSED=1 keeps these unfused)
        if (tr_fused >= 2 && h->bf16 && t.c == 256 && t.mid == 512 && c.attention_heads == 8 && x.L % 64 == 0 && x.L > 64 &&
            x.C == 256 && t.qkv.nchunk == 4 && t.ff2.nchunk == 8 && t.qkv.wfrag && c.resnet_groups == 8 &&
            !(c.flags & ADF_FLAG_SEPARATE_GN_STATS)) {
            Act qkv = new_act(3 * t.c, x.L), att = new_act(t.c, x.L), x2 = new_act(t.c, x.L);
            TrFusedArgs fa;
            memset(&fa, 0, sizeof(fa));
            fa.x = (const bf16_t*)x.p; fa.out = (bf16_t*)x2.p; fa.qkv_out = (bf16_t*)qkv.p; fa.att = (const bf16_t*)att.p;
            fa.ln_w = t.lnw; fa.ln_b = t.lnb; fa.g0 = t.g0; fa.g3 = t.g3;
            fa.wqkv = t.qkv.wfrag; fa.wproj = t.proj.wfrag; fa.wff1 = t.ff1.wfrag; fa.wff2 = t.ff2.wfrag;
            fa.npad_qkv = t.qkv.n_pad; fa.npad_proj = t.proj.n_pad; fa.npad_ff1 = t.ff1.n_pad; fa.npad_ff2 = t.ff2.n_pad;
            fa.eps = 1e-5f;
            x2.stats = alloc_stats(); fa.stats = x2.stats;
            if (live()) {
                check(launch_transformer_tiles(fa, (int)rows, x.L, 1, s));
                check(launch_attention(qkv.p, att.p, h->bf16, p->B, x.L, t.c, c.attention_heads, s));
                check(launch_transformer_tiles(fa, (int)rows, x.L, 2, s));
            }
            tap(name + ".qkv", qkv);
            tap(name + ".att", att);
            tap(name, x2);
            return x2;
        }
        // the nine-launch path: every stored tensor of the block is a recorded activation (the parity tests hold each launch to
        // the oracle on its own; the fused kernels above are then held to this path)
        Act xn = new_act(t.c, x.L);
        if (live()) check(launch_ln_rows(x.p, xn.p, h->bf16, rows, t.c, t.lnw, t.lnb, 1e-5f, s));
        tap(name + ".ln", xn);
        Act qkv = linear(xn, t.qkv, nullptr, 0, false);
        tap(name + ".qkv", qkv);
        Act att = new_act(t.c, x.L);
        if (live()) check(h->x3 ? launch_attention_x3(qkv.p, att.p, p->B, x.L, t.c, c.attention_heads, s)
                                : launch_attention(qkv.p, att.p, h->bf16, p->B, x.L, t.c, c.attention_heads, s));
        tap(name + ".att", att);
        Act x1 = linear(att, t.proj, x.p, 0, false);
        tap(name + ".x1", x1);
        Act n1 = new_act(t.c, x.L);
        if (live()) check(launch_ln_rows(x1.p, n1.p, h->bf16, rows, t.c, t.g0, nullptr, 1e-5f, s));
        tap(name + ".n1", n1);
        Act f1 = linear(n1, t.ff1, nullptr, 1, false);
        tap(name + ".f1", f1);
        Act n2 = new_act(t.mid, x.L);
        if (live()) check(launch_ln_rows(f1.p, n2.p, h->bf16, rows, t.mid, t.g3, nullptr, 1e-5f, s));
        tap(name + ".n2", n2);
        Act x2 = linear(n2, t.ff2, x1.p, 0, true);
        tap(name, x2);
        return x2;
    }
};

int Unet1dNet::build_weights(adf_handle* h) {
    const adf_net_config& c = cfg;
    Registrar1d R{{h}};
    const int ch = c.channels, tdim = 4 * ch, n = c.num_layers;
    if (c.num_classes > 0) R.label_embedder(ch, tdim, c.num_classes);      // conditioner.py:64-90, registered before the U-Net
    const int temb = tdim + h->cdim;     // every FiLM Linear reads cat(time_embed, class_embed) (unet1d.py:272)
    to_in_w = R.reg_f32("unet.to_in.to_in.weight", (int64_t)c.num_filters * c.in_channels * c.window_length);
    to_out_w = R.reg_f32("unet.to_out.to_out.weight", (int64_t)c.num_filters * c.out_channels * c.window_length);
    fourier = R.reg_f32("unet.to_time.0.0.weights", ch / 2);
    t_w1 = R.reg_f32("unet.to_time.0.1.weight", (int64_t)tdim * (ch + 1));
    t_b1 = R.reg_f32("unet.to_time.0.1.bias", tdim);
    t_w2 = R.reg_f32("unet.to_time.2.weight", (int64_t)tdim * tdim);
    t_b2 = R.reg_f32("unet.to_time.2.bias", tdim);
    downs.resize(n);
    for (int i = 0; i < n; ++i) {
        DownW& d = downs[i];
        d.cin = ch * c.multipliers[i]; d.cout = ch * c.multipliers[i + 1]; d.factor = c.factors[i];
        const std::string pre = "unet.downsamples." + std::to_string(i);
        R.conv_folded(pre + ".downsample", d.down, d.cout, d.cin, d.factor * c.kernel_multiplier_downsample + 1, d.factor);
        d.blocks.resize(c.num_blocks[i]);
        for (int j = 0; j < c.num_blocks[i]; ++j) R.resblock(pre + ".blocks." + std::to_string(j), d.blocks[j], d.cout, d.cout, temb);
        d.attn = c.attentions[i] != 0;
        if (d.attn) R.transformer(pre + ".transformer", d.tr, d.cout, c.attention_multiplier);
    }
    const int cb = ch * c.multipliers[n];
    R.resblock("unet.bottleneck.pre_block", mid_pre, cb, cb, temb);
    if (c.use_attention_bottleneck) R.transformer("unet.bottleneck.transformer", mid_tr, cb, c.attention_multiplier);
    R.resblock("unet.bottleneck.post_block", mid_post, cb, cb, temb);
    ups.resize(n);
    for (int u = 0; u < n; ++u) {
        const int i = n - 1 - u;
        UpW& up = ups[u];
        up.cin = ch * c.multipliers[i + 1]; up.cout = ch * c.multipliers[i]; up.factor = c.factors[i];
        const std::string pre = "unet.upsamples." + std::to_string(u);
        const int nb = c.num_blocks[i] + (c.attentions[i] ? 1 : 0);
        up.blocks.resize(nb);
        for (int j = 0; j < nb; ++j) R.resblock(pre + ".blocks." + std::to_string(j), up.blocks[j], 2 * up.cin, up.cin, temb);
        up.attn = c.attentions[i] != 0;
        if (up.attn) R.transformer(pre + ".transformer", up.tr, up.cin, c.attention_multiplier);
        const int f = up.factor;
        if (c.flags & ADF_FLAG_NEAREST_UPSAMPLE) {          // nn.Sequential(Upsample(nearest), ReflectionPad1d(1), Conv1d(k = 3)): unet1d.py:236-246
            up.nearest = true;
            R.conv(pre + ".upsample.2", up.up, up.cout, up.cin, 3, true);
            continue;
        }
        R.reg_pack(pre + ".upsample.weight", up.up, up.cout, up.cin, 2 * f, 0, f * up.cout, true, f);
        if (h->bf16 && up.up.w && (up.cin == 128 || up.cin == 256) && (up.cout == 64 || up.cout == 128 || up.cout == 256) && (f == 2 || f == 4)) {
            up.up.wfrag = dalloc(h, (size_t)up.up.nchunk * up.up.taps * up.up.n_pad * kRowBytes);   // fragment-major copy: adf_gemm_up.h
            if (!up.up.wfrag) R.ok = false;
            else h->slots[pre + ".upsample.weight"].frag = up.up.wfrag;
        }
        up.up.bias = R.reg_f32(pre + ".upsample.bias", up.cout);
        // (f = 2 only: the packing is written for any even factor, but no configuration with f = 4 and f * cout <= 256 is in the tests)
        if ((h->bf16 || h->x3) && up.up.w && f == 2 && (f * up.cout == 128 || f * up.cout == 256) && up.cin % 128 == 0 && up.cout % 64 == 0) {
            ConvW& w3 = up.up3;
            w3.cin = up.cin; w3.K = 2 * f; w3.f = f; w3.taps = 3;
            w3.n = f * up.cout; w3.n_pad = w3.n; w3.cout = w3.n;
            w3.nchunk = ceil_div(up.cin, h->kc);
            w3.w = dalloc(h, ((size_t)w3.nchunk * 3 * w3.n_pad + (size_t)kTapGroup * (w3.n_pad + 128)) * kRowBytes);
            w3.bias = (float*)dalloc(h, (size_t)w3.n * 4);
            if (!w3.w || !w3.bias) R.ok = false;
            else {
                Slot& sw = h->slots[pre + ".upsample.weight"];
                sw.dst3 = w3.w; sw.n_pad3 = w3.n_pad;
                Slot& sb = h->slots[pre + ".upsample.bias"];
                sb.rep = w3.bias; sb.rep_n = f;
            }
        }
    }
    // one concatenated FiLM projection for all resblocks
    h->film_w = (float*)dalloc(h, (size_t)h->film_total * temb * 4);
    h->film_b = (float*)dalloc(h, (size_t)h->film_total * 4);
    if (!h->film_w || !h->film_b) R.ok = false;
    for (const auto& fn : R.film_names) {
        R.reg_f32(fn.pre + ".to_cond_embedding.1.weight", (int64_t)fn.rows * temb, h->film_w + (size_t)fn.off * temb);
        R.reg_f32(fn.pre + ".to_cond_embedding.1.bias", fn.rows, h->film_b + fn.off);
    }
    return R.ok ? 0 : fail(h, "device allocation failed while building the weight registry");
}

int Unet1dNet::forward(adf_handle* h, Plan* p, const FwdIO& io, hipStream_t s) {
    const adf_net_config& c = cfg;
    Walker1d W{{h, p, s}, c};
    W.film2 = io.film2; W.film2_bstride = io.film2_bstride;
    W.film = io.film_pre ? io.film_pre : p->film;
    if (W.begin()) return 1;
    const int B = p->B, L = p->L, n = c.num_layers;
    const int pad = c.window_length / 2 - c.stride / 2;
    const int tdim = 4 * c.channels;
    // sigma embedding + every resblock's FiLM projection (unless the sampler computed them for the whole run already)
    if (W.live() && !io.film_pre) {
        W.check(time_embed(io.t, io.t_stride, io.nb, p->temb, s));
        W.check(launch_film(p->temb, tdim, h->film_w, tdim + h->cdim, 0, h->film_b, p->film, io.nb, h->film_total, s));
    }
    Act x = W.new_act(c.num_filters, L / c.stride);
    if (W.live())
        W.check(launch_to_in(io.x, to_in_w, x.p, h->bf16, B, c.in_channels, L, c.num_filters, c.window_length, c.stride, pad,
                             io.coef, io.coef_bstride, s));
    W.tap("to_in", x);
    std::vector<std::vector<Act>> skips_list;
    for (int i = 0; i < n; ++i) {
        const DownW& d = downs[i];
        const int f = d.factor, km = c.kernel_multiplier_downsample;
        Act y = W.new_act(d.cout, x.L / f);
        // Downsample1d (unet1d.py:214-225) as a stride-1 conv over the row-folded view [L/f][f*C] (Registrar::conv_folded)
        if (x.L % f) return fail(h, "downsample: length not divisible by the factor");
        Act xv = x;
        xv.C = x.C * f; xv.L = x.L / f; xv.stats = nullptr;
        GemmArgs g = W.gemm_base(y, xv.L, y.L, d.down);
        g.seg[0] = Walker1d::seg_of(xv, nullptr, nullptr, 1.f, 0, km + 1, 1, -(km / 2), 1, d.down);
        g.seg[0].tap2_zero_c = folded_tap2_zero_from(d.down.K, f, x.C);
        W.run_gemm(g, y, true);
        W.tap("down" + std::to_string(i) + ".conv", y);
        x = y;
        std::vector<Act> skips;
        for (size_t j = 0; j < d.blocks.size(); ++j) {
            x = W.resblock("down" + std::to_string(i) + ".block" + std::to_string(j), x, nullptr, d.blocks[j], io.nb);
            skips.push_back(x);
        }
        if (d.attn) {
            x = W.transformer("down" + std::to_string(i) + ".attn", x, d.tr);
            skips.push_back(x);
        }
        skips_list.push_back(skips);
    }
    x = W.resblock("mid.pre", x, nullptr, mid_pre, io.nb);
    if (c.use_attention_bottleneck) x = W.transformer("mid.attn", x, mid_tr);
    x = W.resblock("mid.post", x, nullptr, mid_post, io.nb);
    for (int u = 0; u < n; ++u) {
        const UpW& up = ups[u];
        std::vector<Act>& skips = skips_list.back();
        for (size_t j = 0; j < up.blocks.size(); ++j) {
            if (skips.empty()) { W.check("upsample: skip stack underflow"); break; }
            Act sk = skips.back();
            skips.pop_back();
            x = W.resblock("up" + std::to_string(u) + ".block" + std::to_string(j), x, &sk, up.blocks[j], io.nb);
        }
        skips_list.pop_back();
        if (up.attn) x = W.transformer("up" + std::to_string(u) + ".attn", x, up.tr);
        const int f = up.factor;
        Act y = W.new_act(up.cout, x.L * f);
        bool done = false;
        if (up.nearest) {
            // the upsampled, reflection-padded rows are written once ([f L + 2][cin]: row i + 1 = x[i / f], rows 0 and f L + 1 the reflected ones), the
            // 3-tap conv then runs over them without padding (lin = mrows + 2, first tap at the output row)
            Act u0 = W.new_act(up.cin, x.L * f + 2);
            if (W.live()) W.check(launch_upsample_nearest_pad(x.p, u0.p, h->bf16, B, x.L, up.cin, f, s));
            GemmArgs g = W.gemm_base(y, x.L * f + 2, x.L * f, up.up);
            g.seg[0] = Walker1d::seg_of(u0, nullptr, nullptr, 1.f, 0, 3, 1, 0, 1, up.up);
            W.run_gemm(g, y, u + 1 < n);
            done = true;
        }
        if (up.up3.w) {
            // ConvTranspose1d(kernel 2 f, stride f, padding f / 2), f even, as a 3-tap conv over the INPUT rows with f * cout columns: column p * cout + co of
            // row j is output row f j + p -- the same bytes -- and uses x[j] (tap p + f / 2), x[j - 1] (tap p + 3 f / 2, p < f / 2) or x[j + 1] (tap p - f / 2,
            // p >= f / 2); the other third of the packed weights is zero.  No scatter, no L + 1-th row: the resblock conv kernel's raw form takes it.
            Act y3 = y;
            y3.C = f * up.cout; y3.L = x.L;
            GemmArgs g3 = W.gemm_base(y3, x.L, x.L, up.up3);
            g3.seg[0] = Walker1d::seg_of(x, nullptr, nullptr, 1.f, 0, 3, 1, -1, 1, up.up3);
            g3.phase_c = up.cout;
            // (the launcher's own decision, asked before the launch is built.  A statistics request does not change the answer: for a group size outside
            //  the 8 .. 64 channels the epilogue reduces the launcher drops the request and run_gemm runs the separate pass, as for every other route.)
            if (conv_gemm_phase_eligible(g3, h->gemm_dtype())) {
                W.run_gemm(g3, y, u + 1 < n);           // statistics over y's channels: the same bytes as y3
                done = true;
            }
        }
        if (!done) {
            GemmArgs g = W.gemm_base(y, x.L, x.L + 1, up.up);
            g.seg[0] = Walker1d::seg_of(x, nullptr, nullptr, 1.f, 0, 2, 1, 0, -1, up.up);
            g.bias_mod = up.cout;
            g.scatter_f = f; g.scatter_pad = f / 2 + f % 2;
            W.run_gemm(g, y, u + 1 < n);
        }
        W.tap("up" + std::to_string(u) + ".conv", y);
        x = y;
    }
    if (W.live())
        W.check(launch_to_out(x.p, to_out_w, io.out, h->gemm_dtype(), B, c.out_channels, x.L, c.num_filters, c.window_length, c.stride, pad,
                              io.mode, io.x_noisy, io.coef, io.coef_bstride, s));
    return W.bad ? 1 : 0;
}

}  // namespace adf_api

extern "C" int adf_create(const adf_net_config* cfg, adf_handle** out) {
    if (create_begin("adf_create", cfg, out)) return 1;
    const adf_net_config& c = *cfg;
    if (c.num_layers < 1 || c.num_layers > ADF_MAX_LAYERS) { g_create_error = "adf_create: bad num_layers"; return 1; }
    if (c.num_filters != c.channels * c.multipliers[0]) { g_create_error = "adf_create: num_filters must equal channels*multipliers[0]"; return 1; }
    if (c.channels % 2 || c.channels < 2) { g_create_error = "adf_create: channels must be even"; return 1; }
    if (c.dtype != ADF_DTYPE_F32 && c.dtype != ADF_DTYPE_BF16 && c.dtype != ADF_DTYPE_F32X3) { g_create_error = "adf_create: bad dtype"; return 1; }
    // (UNet1dConfig.validate_device restates the three checks below.)  The reference pads by window / 2 - stride / 2 (unet1d.py:584-591, :611-622): with a window
    // and a stride of different parity 2 pad != window - stride and its transposed conv returns L - 1 or L + 1 samples, where to_out writes L
    if (c.stride < 1) { g_create_error = "adf_create: unet.to_in / unet.to_out: stride must be at least 1"; return 1; }
    if (c.stride > c.window_length) { g_create_error = "adf_create: unet.to_in / unet.to_out: stride above window_length (negative padding)"; return 1; }
    if ((c.window_length - c.stride) % 2) { g_create_error = "adf_create: unet.to_in / unet.to_out: window_length and stride of different parity"; return 1; }
    auto net = std::make_unique<Unet1dNet>();
    net->cfg = c;
    NetDims& d = net->dims;
    d.in_channels = c.in_channels; d.out_channels = c.out_channels;
    d.length_multiple = c.stride;
    for (int i = 0; i < c.num_layers; ++i) d.length_multiple *= c.factors[i];
    d.temb = 4 * c.channels; d.label_in = c.channels; d.num_classes = c.num_classes; d.stat_groups = c.resnet_groups;
    return create_finish("adf_create", c.dtype, std::move(net), out);
}
