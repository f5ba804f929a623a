// What the walks of the two 2-D U-Nets (adf_net_adm.hip, adf_net_unet2d.hip) share: activations with FINE GroupNorm statistics, the GroupNorm
// table, the conv launch and the conditioning prologue.  The block walks themselves restate different reference modules and stay apart.
#pragma once
#include "adf_api_internal.h"

namespace adf_api {

// st: FINE GroupNorm statistics of the tensor ([B][C / fg][2]), when its producer reduced them; t1 / st1: the second source of a virtual
// concat (the skip of an output / up block: never materialised -- convs and the GroupNorm table read both sources)
struct T2 { Act t; int H = 0, W = 0; double* st = nullptr; Act t1; double* st1 = nullptr; };

struct Walk2d : Walker {
    int G;                  // GroupNorm groups
    int fg;                 // channels per fine statistics group: divides every GroupNorm group size of the net and every concat split
    float skip_scale;       // != 1: the skip half of a concat enters the GroupNorm table scaled (launch_u2d_gn_finalize_scaled)
    bool small_route;       // outputs that are no multiple of 64 pixels go to launch_u2d_conv_small (and reduce no statistics in the epilogue)
    bool sample_bias;       // convs may take a per-sample addend to the bias: rows of the FiLM projections (ResBlock's additive conditioning)
    const float* film = nullptr;        // the FiLM projections of this pass and their per-sample stride (condition())
    int film_bs = 0;

    // The time embedding (+ the class embedding, per sample) and every block's FiLM projection, unless the sampler computed them for the whole run.
    void condition(const FwdIO& io) {
        const int B = p->B, ted = h->net->dims.temb;
        film = io.film_pre ? io.film_pre : p->film;
        film_bs = io.nb > 1 ? h->film_total : 0;
        if (h->cdim > 0) {
            // class-conditional: emb[b] = time_embed(t) + label_conditioner(classes[b]) (unet2d_oai.py:619-623, unet2d.py:902-908), so every sample has
            // its own FiLM rows
            float* emb_b = (float*)alloc((size_t)B * ted * 4);
            film = p->film; film_bs = h->film_total;
            if (live()) {
                const float* te = io.temb_pre;
                int te_bs = 0;
                if (!te) {
                    check(h->net->time_embed(io.t, io.t_stride, io.nb, p->temb, s));
                    te = p->temb; te_bs = io.nb > 1 ? ted : 0;
                }
                const float* ce = io.null_cond ? h->cond_emb + (size_t)B * ted : h->cond_emb;       // last row = the null embedding
                check(launch_add_rows(emb_b, te, te_bs, ce, io.null_cond ? 0 : ted, B, ted, s));
                check(launch_film(emb_b, ted, h->film_w, ted, 0, h->film_b, p->film, B, h->film_total, s));
            }
        } else if (live() && !io.film_pre) {
            check(h->net->time_embed(io.t, io.t_stride, io.nb, p->temb, s));
            check(launch_film(p->temb, ted, h->film_w, ted, 0, h->film_b, p->film, io.nb, h->film_total, s));
        }
    }
    double* alloc_fine(int C) {
        const size_t bytes = ((size_t)p->B * (C / fg) * 2 * sizeof(double) + 255) & ~(size_t)255;
        const size_t off = p->stats_off;
        p->stats_off += bytes;
        if (p->dry) return (double*)(uintptr_t)(off + 256);
        if (p->stats_off > p->stats_bytes) { check("stats arena overflow"); return nullptr; }
        return (double*)(p->stats + off);
    }
    void ensure_stats(const Act& t, double*& st) {
        if (st) return;
        st = alloc_fine(t.C);
        if (live()) check(launch_gn_stats_any(t.p, h->bf16, p->B, t.L, t.C, t.C / fg, st, s));
    }
    // GroupNorm (+ the scale-shift of the embedding, `fl`) of a tensor (or a virtual concat) folded to the per-(sample, channel) table a conv prologue reads
    float* gn_table(T2& x, const float* gamma, const float* beta, const float* fl) {
        ensure_stats(x.t, x.st);
        if (x.t1.C) ensure_stats(x.t1, x.st1);
        const int ctot = x.t.C + x.t1.C;
        float* ab = (float*)alloc((size_t)p->B * ctot * 2 * 4);
        if (live()) {
            GnFineArgs g;
            memset(&g, 0, sizeof(g));
            g.stats0 = x.st; g.stats1 = x.st1; g.c0 = x.t.C; g.c1 = x.t1.C; g.L = x.t.L; g.G = G; g.B = p->B; g.fg = fg; g.eps = 1e-5f;
            g.gamma = gamma; g.beta = beta; g.film = fl; g.film_bstride = film_bs; g.ab = ab;
            check(x.t1.C && skip_scale != 1.0f ? launch_u2d_gn_finalize_scaled(g, skip_scale, s) : launch_gn_finalize_fine(g, s));
        }
        return ab;
    }
    // 3x3 / 1x1 conv or linear (mode 1: over the nearest x 2 upsampled input, 2: stride 2); `stats`: also reduce the fine GroupNorm statistics of the
    // output in the epilogue (where a GroupNorm reads this tensor next; by the separate pass of ensure_stats where the route has no such epilogue)
    T2 conv(const T2& x, const ConvW& w, const float* ab, int act, int mode, const void* res, bool stats, const float* bias_b = nullptr) {
        T2 y;
        y.H = mode == 1 ? x.H * 2 : (mode == 2 ? x.H / 2 : x.H);
        y.W = mode == 1 ? x.W * 2 : (mode == 2 ? x.W / 2 : x.W);
        y.t = new_act(w.cout, y.H * y.W);
        const bool tiled = !small_route || (y.H * y.W) % 64 == 0;
        if (stats && tiled && w.cout % fg == 0 && (w.cout <= 128 || w.cout % 128 == 0)) y.st = alloc_fine(w.cout);
        if (live()) {
            Conv2dArgs g;
            memset(&g, 0, sizeof(g));
            g.x = x.t.p; g.x1 = x.t1.C ? x.t1.p : nullptr; g.c0 = x.t.C;
            g.ab = ab; g.act = act; g.B = p->B; g.H = y.H; g.W = y.W; g.cin = x.t.C + x.t1.C; g.cout = w.cout; g.n_pad = w.n_pad;
            g.taps = w.taps; g.mode = mode; g.w = w.w; g.nchunk = w.nchunk; g.bias = w.bias; g.res = res; g.out = y.t.p;
            g.bias_b = bias_b; g.bias_bstride = sample_bias ? film_bs : 0;
            g.stats = y.st; g.stats_groups = w.cout / fg;
            check(tiled ? launch_conv2d(g, h->gemm_dtype(), s) : launch_u2d_conv_small(g, s));
        }
        return y;
    }
};

}  // namespace adf_api
