// The DAC stacks behind the C ABI: dac.py::Decoder (dac.py:108-137), dac.py::Encoder (dac.py:57-84) and both halves of FineTuneAutoencoder
// (dac_vae.py:11-77, encode with is_train=False), exact fp32: adf_dac_create, registry, the weight-norm fold, the walks, adf_dac_forward and
// adf_dac_encode.  Channels-last fp32 activations [B][L][C]; kernels: adf_dac.h.
#include "adf_api_internal.h"
#include "adf_dac.h"

using namespace adf;
using namespace adf_api;

namespace adf_api {

// One weight-normed conv: weight_g / weight_v / bias are the load targets; `packed` is w = g v / ||v|| in the layout of the kernel that reads it,
// rebuilt before the first pass after a (re)load of any tensor (DacNet::prepare).  alpha: the Snake in front of it (null: raw input).
struct DacConv {
    float *g = nullptr, *v = nullptr, *bias = nullptr, *alpha = nullptr, *scale = nullptr, *packed = nullptr;
    int cin = 0, cout = 0, taps = 1, dil = 1, stride = 0, down = 0, fold = kDacFoldConv;      // stride: transposed conv; down: strided conv
};
struct DacUnit { DacConv c7, c1; };                                     // ResidualUnit (dac.py:17-33)
struct DacStage { DacConv up; DacUnit unit[3]; int stride = 0; };       // DecoderBlock (dac.py:87-105); EncoderBlock (dac.py:36-54): `up` is its strided conv

constexpr int kDacWalkEncode = 1;      // FwdIO::variant of FineTuneAutoencoder.encode on an autoencoder handle (0: decode)

struct DacNet : Net {
    adf_dac_config cfg;
    bool stage_taps = true;              // route switch ADF_DAC_TAPS (read at create): 0 = never keep the per-unit taps, i.e. every unit's sum in place
    bool folded = false;                 // the packed weights match weight_g / weight_v
    DacConv first, last;                 // decoder: model.0 and the conv in front of tanh; encoder: block.0 and block.<n + 2>
    std::vector<DacStage> stages;
    std::vector<DacConv> ae;             // autoencoder: decoder_layers.{0, 2, 4, ..}
    std::vector<DacConv> enc;            // autoencoder: encoder_layers.{1, 3, 5, ..}
    DacConv btnk;                        // autoencoder: btnk_layer, a plain 1x1 conv to 2 latent_dim columns
    std::vector<DacConv*> all;

    int build_weights(adf_handle* h) override;
    void weight_loaded() override { folded = false; }
    int prepare(adf_handle* h, hipStream_t s) override;
    const char* own_entry() const override {
        if (cfg.kind == ADF_DAC_KIND_DECODER) return "this handle is a DAC decoder: adf_dac_forward is its only compute call (no network pass, denoiser or sampler)";
        if (cfg.kind == ADF_DAC_KIND_ENCODER) return "this handle is a DAC encoder: adf_dac_forward is its only compute call (no network pass, denoiser or sampler)";
        return "this handle is a DAC autoencoder: adf_dac_forward and adf_dac_encode are its compute calls (no network pass, denoiser or sampler)";
    }
    int walk_encoder(adf_handle* h, Plan* p, const FwdIO& io, hipStream_t s);
    int walk_encode(adf_handle* h, Plan* p, const FwdIO& io, hipStream_t s);
    int forward(adf_handle* h, Plan* p, const FwdIO& io, hipStream_t s) override;
    const char* time_embed(const float*, int, int, float*, hipStream_t) override { return "a DAC handle has no time embedding"; }
    // (encoder: -1 where a stage's input is shorter than its strided conv serves; *stage then names it)
    long long out_length(long long T, int* stage = nullptr) const {
        for (int i = 0; i < cfg.n_rates && cfg.kind == ADF_DAC_KIND_DECODER; ++i) T = (T - 1) * cfg.rates[i] - 2 * ((cfg.rates[i] + 1) / 2) + 2 * cfg.rates[i];
        for (int i = 0; i < cfg.n_rates && cfg.kind == ADF_DAC_KIND_ENCODER; ++i) {
            if (T < dac_down_min_length(cfg.rates[i])) { if (stage) *stage = i; return -1; }
            T = dac_down_length((int)T, cfg.rates[i]);
        }
        return T;
    }
};

int DacNet::build_weights(adf_handle* h) {
    Registrar R{h};
    h->film_total = 1;                   // (no FiLM: keeps the plan's shared buffers non-empty)
    // nn.utils.weight_norm: `weight` leaves the module and weight_g, weight_v join behind `bias`
    auto wn = [&](const std::string& pre, DacConv& c, int cin, int cout, int taps, int dil, int stride, int fold, float* alpha) {
        const bool down = fold == kDacFoldDown;                         // (`stride` is then the strided conv's)
        c.cin = cin; c.cout = cout; c.taps = taps; c.dil = dil; c.stride = down ? 0 : stride; c.down = down ? stride : 0; c.fold = fold; c.alpha = alpha;
        const int k = stride > 0 ? 2 * stride : taps;
        const int rows = stride > 0 && !down ? cin : cout;              // axis 0: the input channel of a ConvTranspose1d
        c.bias = R.reg_f32(pre + ".bias", cout);
        c.g = R.reg_f32(pre + ".weight_g", rows);
        c.v = R.reg_f32(pre + ".weight_v", (int64_t)cin * cout * k);
        c.scale = (float*)dalloc(h, (size_t)rows * 4);
        const long long pf = fold == kDacFoldOut ? 7LL * cin : (fold == kDacFoldIn ? 7LL * cout : (down ? dac_packed_floats(stride * cin, cout, 2, 0)
                                                                                                            : dac_packed_floats(cin, cout, taps, stride)));
        c.packed = (float*)dalloc(h, (size_t)pf * 4);
        if (!c.scale || !c.packed) R.ok = false;
        all.push_back(&c);
    };
    if (cfg.kind == ADF_DAC_KIND_AUTOENCODER) {
        const int n = cfg.n_widths;
        const int32_t* w = cfg.widths;
        // btnk_layer: a plain nn.Conv1d (no weight norm): packed with scale 1, its 2 latent_dim columns zero-padded to a multiple of 32
        btnk.cin = w[n - 1]; btnk.cout = 2 * cfg.input_channel; btnk.fold = kDacFoldPlain;
        btnk.v = R.reg_f32("btnk_layer.weight", (int64_t)btnk.cout * btnk.cin);
        btnk.bias = R.reg_f32("btnk_layer.bias", btnk.cout);
        btnk.scale = (float*)dalloc(h, 4);
        btnk.packed = (float*)dalloc(h, (size_t)dac_packed_floats(btnk.cin, btnk.cout, 1, 0) * 4);
        if (!btnk.scale || !btnk.packed) return fail(h, "device allocation failed while building the weight registry");
        all.push_back(&btnk);
        enc.resize(n - 1);                                              // (sized once: `all` keeps pointers into it)
        for (int i = 0; i + 1 < n && R.ok; ++i) {
            float* alpha = R.reg_f32("encoder_layers." + std::to_string(2 * i) + ".alpha", w[i]);
            wn("encoder_layers." + std::to_string(2 * i + 1), enc[i], w[i], w[i + 1], 3, 1, 0, kDacFoldConv, alpha);
        }
        ae.resize(n);
        wn("decoder_layers.0", ae[0], cfg.input_channel, w[n - 1], 3, 1, 0, kDacFoldConv, nullptr);
        for (int i = 1; i < n && R.ok; ++i) {
            float* alpha = R.reg_f32("decoder_layers." + std::to_string(2 * i - 1) + ".alpha", w[n - i]);
            wn("decoder_layers." + std::to_string(2 * i), ae[i], w[n - i], w[n - i - 1], 3, 1, 0, kDacFoldConv, alpha);
        }
        return R.ok ? 0 : fail(h, "device allocation failed while building the weight registry");
    }
    if (cfg.kind == ADF_DAC_KIND_ENCODER) {
        const int n = cfg.n_rates;
        const int dils[3] = {1, 3, 9};
        wn("block.0", first, 1, cfg.channels, 7, 1, 0, kDacFoldIn, nullptr);
        stages.resize(n);
        for (int i = 0; i < n && R.ok; ++i) {
            DacStage& st = stages[i];
            const int C = cfg.channels << i;
            const std::string pre = "block." + std::to_string(i + 1) + ".block.";
            st.stride = cfg.rates[i];
            for (int u = 0; u < 3 && R.ok; ++u) {
                const std::string up = pre + std::to_string(u) + ".block.";
                float* a0 = R.reg_f32(up + "0.alpha", C);
                wn(up + "1", st.unit[u].c7, C, C, 7, dils[u], 0, kDacFoldConv, a0);
                float* a2 = R.reg_f32(up + "2.alpha", C);
                wn(up + "3", st.unit[u].c1, C, C, 1, 1, 0, kDacFoldConv, a2);
            }
            float* alpha = R.reg_f32(pre + "3.alpha", C);
            wn(pre + "4", st.up, C, 2 * C, 2, 1, st.stride, kDacFoldDown, alpha);
        }
        if (R.ok) {
            float* alpha = R.reg_f32("block." + std::to_string(n + 1) + ".alpha", cfg.channels << n);
            wn("block." + std::to_string(n + 2), last, cfg.channels << n, cfg.d_out, 3, 1, 0, kDacFoldConv, alpha);
        }
        return R.ok ? 0 : fail(h, "device allocation failed while building the weight registry");
    }
    wn("model.0", first, cfg.input_channel, cfg.channels, 7, 1, 0, kDacFoldConv, nullptr);
    stages.resize(cfg.n_rates);
    for (int i = 0; i < cfg.n_rates && R.ok; ++i) {
        DacStage& st = stages[i];
        const int cin = cfg.channels >> i, cout = cfg.channels >> (i + 1);
        const std::string pre = "model." + std::to_string(i + 1) + ".block.";
        st.stride = cfg.rates[i];
        float* alpha = R.reg_f32(pre + "0.alpha", cin);
        wn(pre + "1", st.up, cin, cout, 2, 1, st.stride, kDacFoldConvT, alpha);
        const int dils[3] = {1, 3, 9};
        for (int u = 0; u < 3 && R.ok; ++u) {
            const std::string up = pre + std::to_string(u + 2) + ".block.";
            float* a0 = R.reg_f32(up + "0.alpha", cout);
            wn(up + "1", st.unit[u].c7, cout, cout, 7, dils[u], 0, kDacFoldConv, a0);
            float* a2 = R.reg_f32(up + "2.alpha", cout);
            wn(up + "3", st.unit[u].c1, cout, cout, 1, 1, 0, kDacFoldConv, a2);
        }
    }
    if (R.ok) {
        const int cl = cfg.channels >> cfg.n_rates;
        float* alpha = R.reg_f32("model." + std::to_string(cfg.n_rates + 1) + ".alpha", cl);
        wn("model." + std::to_string(cfg.n_rates + 2), last, cl, 1, 7, 1, 0, kDacFoldOut, alpha);
    }
    return R.ok ? 0 : fail(h, "device allocation failed while building the weight registry");
}

// the weight-norm fold of every conv from weight_g / weight_v (stream-ordered behind the loads)
int DacNet::prepare(adf_handle* h, hipStream_t s) {
    if (folded) return 0;
    for (const DacConv* c : all)
        if (const char* e = launch_dac_fold(c->fold, c->g, c->v, c->scale, c->packed, c->cin, c->cout, c->taps, c->down ? c->down : c->stride, s)) return fail(h, e);
    folded = true;
    return 0;
}

// What the three walks share: the plan's walker, an fp32 arena allocation and the one conv launch from a DacConv
struct DacWalk {
    Walker W;
    const int B;
    DacWalk(adf_handle* h, Plan* p, hipStream_t s) : W{h, p, s}, B(p->B) {}
    float* falloc(size_t n) { return (float*)W.alloc(n * 4); }
    void conv(const DacConv& c, const float* x, int L, float* y, const float* res) {
        if (!W.live()) return;
        DacConvArgs a;
        a.x = x; a.alpha = c.alpha; a.w = c.packed; a.bias = c.bias; a.res = res; a.y = y;
        a.B = B; a.Lin = L; a.Cin = c.cin; a.Cout = c.cout; a.taps = c.taps; a.dil = c.dil; a.stride = c.stride; a.down = c.down;
        W.check(launch_dac_conv(a, W.s));
    }
};

// Decoder.forward (dac.py:136-137) / FineTuneAutoencoder.decode (dac_vae.py:69-71); io.x is the reference's [B][C][T], io.out its [B][d_out][L_out]
// (decoder) or [B][1024][T] (autoencoder)
int DacNet::forward(adf_handle* h, Plan* p, const FwdIO& io, hipStream_t s) {
    if (cfg.kind == ADF_DAC_KIND_ENCODER) return walk_encoder(h, p, io, s);
    if (cfg.kind == ADF_DAC_KIND_AUTOENCODER && io.variant == kDacWalkEncode) return walk_encode(h, p, io, s);
    DacWalk K(h, p, s);
    Walker& W = K.W;
    if (W.begin()) return 1;
    const int B = p->B, T = p->L;
    float* x = K.falloc((size_t)B * T * cfg.input_channel);
    if (W.live()) W.check(launch_dac_transpose(io.x, x, B, cfg.input_channel, T, s));
    if (cfg.kind == ADF_DAC_KIND_AUTOENCODER) {
        for (size_t i = 0; i < ae.size() && !W.bad; ++i) {
            float* y = K.falloc((size_t)B * T * ae[i].cout);
            K.conv(ae[i], x, T, y, nullptr);
            W.tap("decoder_layers." + std::to_string(2 * i), Act{y, ae[i].cout, T});
            x = y;
        }
        if (W.live()) W.check(launch_dac_transpose(x, io.out, B, T, ae.back().cout, s));
        return W.bad ? 1 : 0;
    }
    // every unit's output stays readable as a tap while the taps fit 512 MiB; beyond that a unit adds into its input in place
    size_t tap_floats = 0;
    {
        long long L = T;
        for (int i = 0; i < cfg.n_rates; ++i) { L = dac_up_length((int)L, cfg.rates[i]); tap_floats += (size_t)4 * B * L * (cfg.channels >> (i + 1)); }
    }
    const bool keep = stage_taps && tap_floats * 4 <= ((size_t)512 << 20);
    int L = T;
    float* y = K.falloc((size_t)B * L * cfg.channels);
    K.conv(first, x, L, y, nullptr);
    W.tap("model.0", Act{y, cfg.channels, L});
    x = y;
    for (int i = 0; i < cfg.n_rates && !W.bad; ++i) {
        const DacStage& st = stages[i];
        const std::string name = "model." + std::to_string(i + 1);
        const int C = st.up.cout, Lo = dac_up_length(L, st.stride);
        y = K.falloc((size_t)B * Lo * C);
        K.conv(st.up, x, L, y, nullptr);
        if (keep) W.tap(name + ".block.1", Act{y, C, Lo});       // (in place, the first unit's sum lands in this buffer)
        x = y; L = Lo;
        float* t = K.falloc((size_t)B * L * C);
        for (int u = 0; u < 3; ++u) {
            K.conv(st.unit[u].c7, x, L, t, nullptr);
            y = keep ? K.falloc((size_t)B * L * C) : x;          // in place: the 1x1 conv reads t; each thread reads res[o] before it writes y[o]
            K.conv(st.unit[u].c1, t, L, y, x);
            if (keep) W.tap(name + ".block." + std::to_string(u + 2), Act{y, C, L});
            x = y;
        }
        W.tap(name, Act{x, C, L});
    }
    float* pre = keep ? K.falloc((size_t)B * L) : nullptr;
    if (W.live()) W.check(launch_dac_out(x, last.alpha, last.packed, last.bias, io.out, pre, B, L, last.cin, s));
    if (keep) W.tap("model." + std::to_string(cfg.n_rates + 2), Act{pre, 1, L});
    return W.bad ? 1 : 0;
}

// Encoder.forward (dac.py:83-84); io.x is the reference's [B][1][L], io.out its [B][d_latent][L_out]
int DacNet::walk_encoder(adf_handle* h, Plan* p, const FwdIO& io, hipStream_t s) {
    DacWalk K(h, p, s);
    Walker& W = K.W;
    if (W.begin()) return 1;
    const int B = p->B;
    const int n = cfg.n_rates;
    int L = p->L;
    // every unit's output stays readable as a tap while the taps fit 512 MiB; beyond that only a stage's first unit gets a buffer of its own (its input
    // is the tap of the block in front of it) and the other two add into it in place
    size_t tap_floats = 0;
    {
        long long Li = L;
        for (int i = 0; i < n; ++i) { tap_floats += (size_t)3 * B * Li * (cfg.channels << i); Li = Li < dac_down_min_length(cfg.rates[i]) ? 1 : dac_down_length((int)Li, cfg.rates[i]); }
    }
    const bool keep = stage_taps && tap_floats * 4 <= ((size_t)512 << 20);
    float* x = K.falloc((size_t)B * L * cfg.channels);
    if (W.live()) W.check(launch_dac_in(io.x, first.packed, first.bias, x, B, L, cfg.channels, s));
    W.tap("block.0", Act{x, cfg.channels, L});
    for (int i = 0; i < n && !W.bad; ++i) {
        const DacStage& st = stages[i];
        const std::string name = "block." + std::to_string(i + 1);
        const int C = cfg.channels << i;
        if (L < dac_down_min_length(st.stride)) { W.check("adf_dac_forward: L is too short for the strided conv of a stage"); break; }
        float* t = K.falloc((size_t)B * L * C);
        for (int u = 0; u < 3; ++u) {
            K.conv(st.unit[u].c7, x, L, t, nullptr);
            float* y = keep || u == 0 ? K.falloc((size_t)B * L * C) : x;      // in place: the 1x1 conv reads t; each thread reads res[o] before it writes y[o]
            K.conv(st.unit[u].c1, t, L, y, x);
            if (keep) W.tap(name + ".block." + std::to_string(u), Act{y, C, L});
            x = y;
        }
        const int Lo = dac_down_length(L, st.stride);
        float* y = K.falloc((size_t)B * Lo * 2 * C);
        K.conv(st.up, x, L, y, nullptr);
        W.tap(name, Act{y, 2 * C, Lo});
        x = y; L = Lo;
    }
    float* y = K.falloc((size_t)B * L * cfg.d_out);
    K.conv(last, x, L, y, nullptr);
    W.tap("block." + std::to_string(n + 2), Act{y, cfg.d_out, L});
    if (W.live()) W.check(launch_dac_transpose(y, io.out, B, L, cfg.d_out, s));
    return W.bad ? 1 : 0;
}

// FineTuneAutoencoder.encode(x, is_train=False) (dac_vae.py:50-67); io.x is [B][1024][T], io.out the mean [B][latent_dim][T], io.aux the KL term
// (one float; null in the warm-up pass: a float of the workspace)
int DacNet::walk_encode(adf_handle* h, Plan* p, const FwdIO& io, hipStream_t s) {
    DacWalk K(h, p, s);
    Walker& W = K.W;
    if (W.begin()) return 1;
    const int B = p->B;
    const int T = p->L, D = cfg.input_channel;
    float* x = K.falloc((size_t)B * T * cfg.widths[0]);
    if (W.live()) W.check(launch_dac_transpose(io.x, x, B, cfg.widths[0], T, s));
    for (size_t i = 0; i < enc.size() && !W.bad; ++i) {
        float* y = K.falloc((size_t)B * T * enc[i].cout);
        K.conv(enc[i], x, T, y, nullptr);
        W.tap("encoder_layers." + std::to_string(2 * i + 1), Act{y, enc[i].cout, T});
        x = y;
    }
    float* raw = K.falloc((size_t)B * T * 2 * D);
    K.conv(btnk, x, T, raw, nullptr);
    W.tap("btnk_layer", Act{raw, 2 * D, T});
    double* partial = (double*)W.alloc((size_t)B * dac_btnk_chunks((long long)D * T) * sizeof(double));
    float* kl = K.falloc(1);
    if (W.live()) W.check(launch_dac_btnk(raw, io.out, io.aux ? io.aux : kl, partial, B, T, D, cfg.d_out == ADF_DAC_BTNK_TANH, s));
    return W.bad ? 1 : 0;
}

}  // namespace adf_api

extern "C" int adf_dac_create(const adf_dac_config* cfg, adf_handle** out) {
    if (create_begin("adf_dac_create", cfg, out)) return 1;
    const adf_dac_config& c = *cfg;
    auto bad = [&](const char* m) { g_create_error = std::string("adf_dac_create: ") + m; return 1; };
    if (c.dtype != ADF_DTYPE_F32) return bad("dtype must be ADF_DTYPE_F32");
    if (c.kind != ADF_DAC_KIND_DECODER && c.kind != ADF_DAC_KIND_AUTOENCODER && c.kind != ADF_DAC_KIND_ENCODER)
        return bad("kind must be ADF_DAC_KIND_DECODER, ADF_DAC_KIND_AUTOENCODER or ADF_DAC_KIND_ENCODER");
    if (c.kind != ADF_DAC_KIND_ENCODER && (c.input_channel < 4 || c.input_channel % 4 || c.input_channel > 2048))
        return bad("input_channel (latent_dim) must be a multiple of 4 in [4, 2048]");
    auto net = std::make_unique<DacNet>();
    NetDims& d = net->dims;
    int in_channels = c.input_channel;
    if (c.kind == ADF_DAC_KIND_ENCODER) {
        if (c.input_channel != 1) return bad("input_channel must be 1 (the encoder reads a waveform)");
        if (c.n_rates < 1 || c.n_rates > ADF_DAC_MAX_RATES) return bad("1 to 6 strides");
        if (c.channels < 32 || c.channels % 32 || ((long long)c.channels << c.n_rates) > 8192) return bad("d_model must be a multiple of 32 with d_model * 2**n_strides <= 8192");
        if (c.d_out < 32 || c.d_out % 32 || c.d_out > 8192) return bad("d_latent must be a multiple of 32 in [32, 8192]");
        // the plan's staging buffers are sized [B][out_channels][L] and hold the [B][d_latent][L_out] result: a stride s maps a valid length L to at
        // most L / s (even s) or (L + 1) / s <= 1.5 L / s (odd s: L >= s - 1 >= 2)
        double f = (double)c.d_out;
        for (int i = 0; i < c.n_rates; ++i) {
            if (c.rates[i] < 2 || c.rates[i] > 16) return bad("every stride must lie in [2, 16]");
            f *= (c.rates[i] % 2 ? 1.5 : 1.0) / c.rates[i];
        }
        d.out_channels = std::max(1, (int)std::ceil(f));
    } else if (c.kind == ADF_DAC_KIND_DECODER) {
        if (c.n_rates < 1 || c.n_rates > ADF_DAC_MAX_RATES) return bad("1 to 6 rates");
        if (c.d_out != 1) return bad("d_out must be 1");
        if (c.channels < 1 || c.channels > 8192 || c.channels % (32 << c.n_rates)) return bad("every stage width channels / 2**i must be a multiple of 32");
        long long up = 1;
        for (int i = 0; i < c.n_rates; ++i) {
            if (c.rates[i] < 2 || c.rates[i] > 16) return bad("every rate must lie in [2, 16]");
            up *= c.rates[i];
        }
        d.out_channels = (int)up;        // (the plan's staging buffers are sized [B][out_channels][T]: at least the [B][1][L_out] result)
    } else {
        if (c.n_widths < 2 || c.n_widths > ADF_DAC_MAX_WIDTHS) return bad("intermediate_embedding_size must have 2 to 8 entries");
        if (c.widths[0] != 1024) return bad("intermediate_embedding_size[0] must be 1024 (the DAC embedding)");
        for (int i = 0; i < c.n_widths; ++i)
            if (c.widths[i] < 32 || c.widths[i] % 32 || c.widths[i] > 8192) return bad("every intermediate_embedding_size entry must be a multiple of 32");
        d.out_channels = std::max(c.widths[0], c.input_channel);      // (the plan's staging buffers hold decode's [B][1024][T] and encode's [B][latent_dim][T])
    }
    net->cfg = c;
    net->stage_taps = adf_route_switch("ADF_DAC_TAPS", 1) != 0;
    d.in_channels = in_channels;
    d.temb = 1;
    return create_finish("adf_dac_create", c.dtype, std::move(net), out);
}

extern "C" int adf_dac_forward(adf_handle* h, const float* in, int B, int T, float* out, void* stream) {
    if (!h) return 1;
    ADF_ON_DEVICE(h);
    if (!h->net->own_entry()) return fail(h, "adf_dac_forward: the handle is not a DAC handle (adf_dac_create)");
    if (!in || !out) return fail(h, "adf_dac_forward: null tensor");
    if (B < 1 || B > 65535 || T < 1) return fail(h, "adf_dac_forward: B in [1, 65535] and T >= 1");
    DacNet* net = static_cast<DacNet*>(h->net.get());
    if (net->cfg.kind == ADF_DAC_KIND_ENCODER) {
        int stage = 0;
        if (net->out_length(T, &stage) < 0)
            return fail(h, "adf_dac_forward: L = " + std::to_string(T) + " is too short: the strided conv of stage " + std::to_string(stage) + " (stride " +
                           std::to_string(net->cfg.rates[stage]) + ") needs at least " + std::to_string(dac_down_min_length(net->cfg.rates[stage])) + " positions");
        // the largest activation is the full-rate one behind the first conv ([B][L][d_model]; a stage halves or better the floats it is given)
        if (T > (1 << 30) || (long long)B * T * net->cfg.channels > (1LL << 33)) return fail(h, "adf_dac_forward: B * L too large");
    } else if (net->out_length(T) * std::max(B, 1) > (1LL << 30) || (long long)B * T * 8192 > (1LL << 33)) return fail(h, "adf_dac_forward: B * T too large");
    hipStream_t s = (hipStream_t)stream;
    Plan* p;
    if (get_plan(h, B, T, s, &p, true)) return 1;
    FwdIO io;
    io.x = in; io.out = out; io.nb = B;
    p->cfg_live = false;
    return forward(h, p, io, s);
}

extern "C" int adf_dac_encode(adf_handle* h, const float* in, int B, int T, float* mean_out, float* kl_out, void* stream) {
    if (!h) return 1;
    ADF_ON_DEVICE(h);
    if (!h->net->own_entry()) return fail(h, "adf_dac_encode: the handle is not a DAC handle (adf_dac_create)");
    DacNet* net = static_cast<DacNet*>(h->net.get());
    if (net->cfg.kind != ADF_DAC_KIND_AUTOENCODER) return fail(h, "adf_dac_encode: the handle is not an autoencoder (ADF_DAC_KIND_AUTOENCODER)");
    if (!in || !mean_out || !kl_out) return fail(h, "adf_dac_encode: null tensor");
    if (B < 1 || B > 65535 || T < 1) return fail(h, "adf_dac_encode: B in [1, 65535] and T >= 1");
    if ((long long)B * T * 8192 > (1LL << 33)) return fail(h, "adf_dac_encode: B * T too large");
    hipStream_t s = (hipStream_t)stream;
    Plan* p;
    if (get_plan(h, B, T, s, &p, true, kDacWalkEncode)) return 1;
    FwdIO io;
    io.x = in; io.out = mean_out; io.aux = kl_out; io.nb = B; io.variant = kDacWalkEncode;
    p->cfg_live = false;
    return forward(h, p, io, s);
}

extern "C" int64_t adf_dac_output_length(const adf_handle* h, int T) {
    if (!h || !h->net->own_entry() || T < 1) return -1;
    return static_cast<const DacNet*>(h->net.get())->out_length(T);
}
