// Launchers of the kernels only the Imagen-style 2-D U-Net UNet2dBase needs (adf_unet2d.hip; reference: src/models/backbones/unet2d.py,
// attention_utils.py).  Same rules as adf_kernels.h: nullptr on success or a static error string; no allocation, synchronisation or copy,
// so every launcher is safe inside hipGraph capture.  Exact fp32 only: activations are channels-last fp32 [B][H*W][C].
#pragma once
#include "adf_common.h"
#include "adf_conv2d.h"

namespace adf {

// LearnedSinusoidalPosEmb (:66-81) -> Linear -> SiLU (to_time_hiddens :702-706) -> Linear (to_time_cond :708-710): t[b * t_stride] -> out[b][tcd].
// fourier: the `half` learned frequencies; w1 [tcd][2 half + 1], w2 [tcd][tcd].
const char* launch_u2d_time_embed(const float* t, int t_stride, int nb, const float* fourier, int half, const float* w1, const float* b1,
                                  const float* w2, const float* b2, int tcd, float* out, hipStream_t s);

// CrossEmbedLayer (:261-286) at stride 1 from the fp32 [B][cin][H][W] input with the EDM c_in (coef[b * coef_bstride], may be null) fused:
// kernel size ks[i] writes channels [off[i], off[i + 1]) of the channels-last output [B][H*W][off[n]].  stats (pre-zeroed [B][off[n] / fg][2]):
// the fine GroupNorm statistics (sum, sumsq over fg channels) of the stored output.  Every slice a multiple of 4 channels, fg in {1, 2, 4}.
struct U2dCrossEmbedArgs {
    const float* x; const float* coef; int coef_bstride;
    int B, cin, H, W, n;
    int ks[4], off[5];
    const float* w[4]; const float* bias[4];
    float* out; double* stats; int fg;
};
const char* launch_u2d_cross_embed(const U2dCrossEmbedArgs& a, hipStream_t s);

// Direct exact-fp32 convolution for images whose H * W is not a multiple of 64 pixels (launch_conv2d's tiles lie inside one image): the same
// Conv2dArgs and packed weights, modes 0 and 2, one or two sources, the GroupNorm table prologue, bias, per-sample bias addend and residual.
// Statistics are not reduced here (a.stats must be null).
const char* launch_u2d_conv_small(const Conv2dArgs& a, hipStream_t s);

// GroupNorm table of the virtual concat [x0 ; scale1 * x1] from the FINE statistics of the two UNSCALED sources (launch_gn_finalize_fine with the
// skip scale of UpsamplingBlock :530-535 folded in): statistics of source 1 enter as (scale1 sum, scale1^2 sumsq), and its table entries multiply
// the raw input, a = scale1 * gamma * rstd.
const char* launch_u2d_gn_finalize_scaled(const GnFineArgs& a, float scale1, hipStream_t s);

// GlobalContext (:173-195).  Pass 1: per sample and chunk of rows, the to_k logit of every pixel (1x1 conv to one channel), an online softmax
// over the chunk and the softmax-weighted channel sum: part[b][chunk] = (max, sum of exp, C weighted sums).  Pass 2: the chunks combined to the
// pooled vector, then 1x1 conv -> SiLU -> 1x1 conv -> sigmoid: gate[b][C].  C <= 1024, hid <= 1024.
int u2d_gca_chunks(int L);
const char* launch_u2d_gca_pool(const float* h, const float* wk, const float* bk, int B, int L, int C, float* part, hipStream_t s);
const char* launch_u2d_gca_gate(const float* part, int B, int L, int C, int hid, const float* w0, const float* b0, const float* w2,
                                const float* b2, float* gate, hipStream_t s);
// out = h * gate[b] + res (ResnetBlock :164-168) with the fine GroupNorm statistics of out (pre-zeroed [B][C / fg][2]; may be null)
const char* launch_u2d_gate_residual(const float* h, const float* gate, const float* res, float* out, int B, int L, int C, double* stats,
                                     int fg, hipStream_t s);

// PixelShuffleUpsample (:27-55) after its 1x1 conv: out[b][(2y + s1) * 2W + 2x + s2][c] = SiLU(in[b][y * W + x][4 c + 2 s1 + s2])
const char* launch_u2d_silu_shuffle(const float* in, float* out, int B, int H, int W, int C, hipStream_t s);

// FeedForward (attention_utils.py:186-194) middle: y = LayerNorm_g(GELU(x)) over the last dim (exact erf GELU, biased variance, gain only).
// C a multiple of 4, at most 1024: the widest row the net can hand it (the Linear behind it reads at most 1024 input channels).
const char* launch_u2d_gelu_ln_rows(const float* x, float* y, long long rows, int C, const float* g, float eps, hipStream_t s);

// Self-attention at head dim 128 (attention_utils.py:160-182) in exact fp32 on a fused [B][N][3C] q | k | v tensor -> out [B][N][C].
// Four lanes share a query (32 head dims each); key / value tiles are staged in LDS.  Any N >= 1.
const char* launch_u2d_attention_d128(const float* qkv, float* out, int B, int N, int C, int heads, hipStream_t s);

// final_conv (:972): 3x3 conv of the RAW channels-last input (no norm, no activation) to cout <= 4 channels, written as fp32 [B][cout][H][W],
// mode 1: clamp(c_skip * x_noisy + c_out * F, -1, 1) (the EDM epilogue of launch_conv2d_out)
const char* launch_u2d_conv_out_raw(const float* h, const float* w, const float* bias, float* out, int B, int cin, int H, int W, int cout,
                                    int mode, const float* x_noisy, const float* coef, int coef_bstride, hipStream_t s);

// Load-time weight transforms (fp32 -> fp32, then packed by launch_pack_weight):
//   mode 0: Downsample's 1x1 conv over pixel-unshuffled channels c * 4 + s1 * 2 + s2 (:57-64), src [cout][4 cin] -> a 3x3 weight
//           [cout][cin][9] whose taps (1 + s1, 1 + s2) carry it and whose other taps are zero: the same map as a 3x3 / stride-2 / pad-1 conv
//   mode 1: src [cout][cin][K] with input channels >= c0 scaled by `scale` (the skip scale folded into res_conv)
const char* launch_u2d_weight_transform(const float* src, float* dst, int mode, int cout, int cin, int K, int c0, float scale, hipStream_t s);

}  // namespace adf
