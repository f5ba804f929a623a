// WavenetNet: the WaveNetNoise network object (adf_net_wavenet.hip), declared here because adf_bench_wavenet_layer (adf_bench_replay.hip) is
// instrumentation of this one network and reads its configuration.
#pragma once
#include "adf_api_internal.h"

namespace adf_api {

// WaveNetNoise (wavenet.py:153-180): a weight-normed conv keeps the state-dict tensors (bias, 0-dim g, v) in fp32 and a packed
// GEMM operand of the effective weight v * g / ||v||, rebuilt when a tensor was (re)loaded
struct WnConv {
    float *bias = nullptr, *g = nullptr, *v = nullptr;
    void* packed = nullptr;
    int cout = 0, cin = 0, K = 0;
};

struct WavenetNet : Net {
    adf_wavenet_config cfg;
    WnConv in, sp;
    std::vector<WnConv> dil, outp;
    float *fc1w = nullptr, *fc1b = nullptr, *fc2w = nullptr, *fc2b = nullptr, *out_w = nullptr, *out_b = nullptr;
    double* sumsq = nullptr;             // scratch of the norm reduction
    bool packed = false;

    int build_weights(adf_handle* h) override;
    void weight_loaded() override { packed = false; }      // the effective weights (v * g / ||v||) are rebuilt before the next pass
    int prepare(adf_handle* h, hipStream_t s) override;
    int forward(adf_handle* h, Plan* p, const FwdIO& io, hipStream_t s) override;
    const char* time_embed(const float* t, int t_stride, int n, float* temb, hipStream_t s) override {
        return launch_wn_step_embed(t, t_stride, n, fc1w, fc1b, fc2w, fc2b, cfg.dim_in, cfg.dim_mid, cfg.dim_out, temb, s);
    }
};

}  // namespace adf_api
