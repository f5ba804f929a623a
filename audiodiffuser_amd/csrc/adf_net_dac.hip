// The DAC decoder stack behind the C ABI: dac.py::Decoder (dac.py:108-137) and the decode half of FineTuneAutoencoder (dac_vae.py:37-71), exact
// fp32: adf_dac_create, registry, the weight-norm fold, the walk and adf_dac_forward.  Channels-last fp32 activations [B][L][C]; kernels: adf_dac.h.
#include "adf_api_internal.h"
#include "adf_dac.h"

using namespace adf;
using namespace adf_api;

namespace adf_api {

// One weight-normed conv: weight_g / weight_v / bias are the load targets; `packed` is w = g v / ||v|| in the layout of the kernel that reads it,
// rebuilt before the first pass after a (re)load of any tensor (DacNet::prepare).  alpha: the Snake in front of it (null: raw input).
struct DacConv {
    float *g = nullptr, *v = nullptr, *bias = nullptr, *alpha = nullptr, *scale = nullptr, *packed = nullptr;
    int cin = 0, cout = 0, taps = 1, dil = 1, stride = 0, fold = kDacFoldConv;
};
struct DacUnit { DacConv c7, c1; };                                     // ResidualUnit (dac.py:17-33)
struct DacStage { DacConv up; DacUnit unit[3]; int stride = 0; };       // DecoderBlock (dac.py:87-105)

struct DacNet : Net {
    adf_dac_config cfg;
    bool stage_taps = true;              // route switch ADF_DAC_TAPS (read at create): 0 = never keep the per-unit taps, i.e. every unit's sum in place
    bool folded = false;                 // the packed weights match weight_g / weight_v
    DacConv first, last;                 // decoder: model.0 and the conv in front of tanh
    std::vector<DacStage> stages;
    std::vector<DacConv> ae;             // autoencoder: decoder_layers.{0, 2, 4, ..}
    std::vector<DacConv*> all;

    int build_weights(adf_handle* h) override;
    void weight_loaded() override { folded = false; }
    int prepare(adf_handle* h, hipStream_t s) override;
    const char* own_entry() const override { return "this handle is a DAC decoder: adf_dac_forward is its only compute call (no network pass, denoiser or sampler)"; }
    int forward(adf_handle* h, Plan* p, const FwdIO& io, hipStream_t s) override;
    const char* time_embed(const float*, int, int, float*, hipStream_t) override { return "a DAC handle has no time embedding"; }
    long long out_length(long long T) const {
        for (int i = 0; i < cfg.n_rates && cfg.kind == ADF_DAC_KIND_DECODER; ++i) T = (T - 1) * cfg.rates[i] - 2 * ((cfg.rates[i] + 1) / 2) + 2 * cfg.rates[i];
        return T;
    }
};

int DacNet::build_weights(adf_handle* h) {
    Registrar R{h};
    h->film_total = 1;                   // (no FiLM: keeps the plan's shared buffers non-empty)
    // nn.utils.weight_norm: `weight` leaves the module and weight_g, weight_v join behind `bias`
    auto wn = [&](const std::string& pre, DacConv& c, int cin, int cout, int taps, int dil, int stride, int fold, float* alpha) {
        c.cin = cin; c.cout = cout; c.taps = taps; c.dil = dil; c.stride = stride; c.fold = fold; c.alpha = alpha;
        const int k = stride > 0 ? 2 * stride : taps;
        const int rows = stride > 0 ? cin : cout;                       // axis 0: the input channel of a ConvTranspose1d
        c.bias = R.reg_f32(pre + ".bias", cout);
        c.g = R.reg_f32(pre + ".weight_g", rows);
        c.v = R.reg_f32(pre + ".weight_v", (int64_t)cin * cout * k);
        c.scale = (float*)dalloc(h, (size_t)rows * 4);
        c.packed = (float*)dalloc(h, (size_t)(fold == kDacFoldOut ? 7LL * cin : dac_packed_floats(cin, cout, taps, stride)) * 4);
        if (!c.scale || !c.packed) R.ok = false;
        all.push_back(&c);
    };
    if (cfg.kind == ADF_DAC_KIND_AUTOENCODER) {
        const int n = cfg.n_widths;
        const int32_t* w = cfg.widths;
        // btnk_layer and encoder_layers are in the state dict and never read by decode: one landing buffer each kind
        size_t big = (size_t)w[n - 1] * 2 * cfg.input_channel;
        for (int i = 0; i + 1 < n; ++i) big = std::max(big, (size_t)w[i] * w[i + 1] * 3);
        float* sink = (float*)dalloc(h, big * 4);
        if (!sink) return fail(h, "device allocation failed while building the weight registry");
        R.reg_f32("btnk_layer.weight", (int64_t)2 * cfg.input_channel * w[n - 1], sink);
        R.reg_f32("btnk_layer.bias", 2 * cfg.input_channel, sink);
        for (int i = 0; i + 1 < n; ++i) {
            const std::string cv = "encoder_layers." + std::to_string(2 * i + 1);
            R.reg_f32("encoder_layers." + std::to_string(2 * i) + ".alpha", w[i], sink);
            R.reg_f32(cv + ".bias", w[i + 1], sink);
            R.reg_f32(cv + ".weight_g", w[i + 1], sink);
            R.reg_f32(cv + ".weight_v", (int64_t)w[i + 1] * w[i] * 3, sink);
        }
        ae.resize(n);                                                   // (sized once: `all` keeps pointers into it)
        wn("decoder_layers.0", ae[0], cfg.input_channel, w[n - 1], 3, 1, 0, kDacFoldConv, nullptr);
        for (int i = 1; i < n && R.ok; ++i) {
            float* alpha = R.reg_f32("decoder_layers." + std::to_string(2 * i - 1) + ".alpha", w[n - i]);
            wn("decoder_layers." + std::to_string(2 * i), ae[i], w[n - i], w[n - i - 1], 3, 1, 0, kDacFoldConv, alpha);
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
        if (const char* e = launch_dac_fold(c->fold, c->g, c->v, c->scale, c->packed, c->cin, c->cout, c->taps, c->stride, s)) return fail(h, e);
    folded = true;
    return 0;
}

// Decoder.forward (dac.py:136-137) / FineTuneAutoencoder.decode (dac_vae.py:69-71); io.x is the reference's [B][C][T], io.out its [B][d_out][L_out]
// (decoder) or [B][1024][T] (autoencoder)
int DacNet::forward(adf_handle* h, Plan* p, const FwdIO& io, hipStream_t s) {
    Walker W{h, p, s};
    if (W.begin()) return 1;
    const int B = p->B, T = p->L;
    auto falloc = [&](size_t n) { return (float*)W.alloc(n * 4); };
    auto conv = [&](const DacConv& c, const float* x, int L, float* y, const float* res) {
        if (!W.live()) return;
        DacConvArgs a;
        a.x = x; a.alpha = c.alpha; a.w = c.packed; a.bias = c.bias; a.res = res; a.y = y;
        a.B = B; a.Lin = L; a.Cin = c.cin; a.Cout = c.cout; a.taps = c.taps; a.dil = c.dil; a.stride = c.stride;
        W.check(launch_dac_conv(a, s));
    };
    float* x = falloc((size_t)B * T * cfg.input_channel);
    if (W.live()) W.check(launch_dac_transpose(io.x, x, B, cfg.input_channel, T, s));
    if (cfg.kind == ADF_DAC_KIND_AUTOENCODER) {
        for (size_t i = 0; i < ae.size() && !W.bad; ++i) {
            float* y = falloc((size_t)B * T * ae[i].cout);
            conv(ae[i], x, T, y, nullptr);
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
    float* y = falloc((size_t)B * L * cfg.channels);
    conv(first, x, L, y, nullptr);
    W.tap("model.0", Act{y, cfg.channels, L});
    x = y;
    for (int i = 0; i < cfg.n_rates && !W.bad; ++i) {
        const DacStage& st = stages[i];
        const std::string name = "model." + std::to_string(i + 1);
        const int C = st.up.cout, Lo = dac_up_length(L, st.stride);
        y = falloc((size_t)B * Lo * C);
        conv(st.up, x, L, y, nullptr);
        if (keep) W.tap(name + ".block.1", Act{y, C, Lo});       // (in place, the first unit's sum lands in this buffer)
        x = y; L = Lo;
        float* t = falloc((size_t)B * L * C);
        for (int u = 0; u < 3; ++u) {
            conv(st.unit[u].c7, x, L, t, nullptr);
            y = keep ? falloc((size_t)B * L * C) : x;          // in place: the 1x1 conv reads t; each thread reads res[o] before it writes y[o]
            conv(st.unit[u].c1, t, L, y, x);
            if (keep) W.tap(name + ".block." + std::to_string(u + 2), Act{y, C, L});
            x = y;
        }
        W.tap(name, Act{x, C, L});
    }
    float* pre = keep ? falloc((size_t)B * L) : nullptr;
    if (W.live()) W.check(launch_dac_out(x, last.alpha, last.packed, last.bias, io.out, pre, B, L, last.cin, s));
    if (keep) W.tap("model." + std::to_string(cfg.n_rates + 2), Act{pre, 1, L});
    return W.bad ? 1 : 0;
}

}  // namespace adf_api

extern "C" int adf_dac_create(const adf_dac_config* cfg, adf_handle** out) {
    if (create_begin("adf_dac_create", cfg, out)) return 1;
    const adf_dac_config& c = *cfg;
    auto bad = [&](const char* m) { g_create_error = std::string("adf_dac_create: ") + m; return 1; };
    if (c.dtype != ADF_DTYPE_F32) return bad("dtype must be ADF_DTYPE_F32");
    if (c.kind != ADF_DAC_KIND_DECODER && c.kind != ADF_DAC_KIND_AUTOENCODER) return bad("kind must be ADF_DAC_KIND_DECODER or ADF_DAC_KIND_AUTOENCODER");
    if (c.input_channel < 4 || c.input_channel % 4 || c.input_channel > 2048) return bad("input_channel (latent_dim) must be a multiple of 4 in [4, 2048]");
    auto net = std::make_unique<DacNet>();
    NetDims& d = net->dims;
    if (c.kind == ADF_DAC_KIND_DECODER) {
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
        d.out_channels = c.widths[0];
    }
    net->cfg = c;
    net->stage_taps = adf_route_switch("ADF_DAC_TAPS", 1) != 0;
    d.in_channels = c.input_channel;
    d.temb = 1;
    return create_finish("adf_dac_create", c.dtype, std::move(net), out);
}

extern "C" int adf_dac_forward(adf_handle* h, const float* in, int B, int T, float* out, void* stream) {
    if (!h) return 1;
    ADF_ON_DEVICE(h);
    if (!h->net->own_entry()) return fail(h, "adf_dac_forward: the handle is not a DAC handle (adf_dac_create)");
    if (!in || !out) return fail(h, "adf_dac_forward: null tensor");
    if (B < 1 || B > 65535 || T < 1) return fail(h, "adf_dac_forward: B in [1, 65535] and T >= 1");
    const DacNet* net = static_cast<const DacNet*>(h->net.get());
    if (net->out_length(T) * std::max(B, 1) > (1LL << 30) || (long long)B * T * 8192 > (1LL << 33)) return fail(h, "adf_dac_forward: B * T too large");
    hipStream_t s = (hipStream_t)stream;
    Plan* p;
    if (get_plan(h, B, T, s, &p, true)) return 1;
    FwdIO io;
    io.x = in; io.out = out; io.nb = B;
    p->cfg_live = false;
    return forward(h, p, io, s);
}

extern "C" int64_t adf_dac_output_length(const adf_handle* h, int T) {
    if (!h || !h->net->own_entry() || T < 1) return -1;
    return static_cast<const DacNet*>(h->net.get())->out_length(T);
}
