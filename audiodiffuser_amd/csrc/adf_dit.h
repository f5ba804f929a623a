// Kernels of the adaLN-Zero diffusion transformer (reference: src/models/backbones/dit.py:220-429), exact fp32 on token-major activations
// [B][T][D] (adf_dit.hip; the walk is adf_net_dit.hip).  Every launcher returns nullptr or a static string; none allocates, synchronises or copies,
// so all of them can be captured.
//
//   launch_dit_linear        Y[M][N] = epi(X[M][K] W[N][K]^T + b) on v_mfma_f32_32x32x2_f32: the q|k|v projection, to_out, fc1, fc2, the
//                            modulation GEMM of all blocks (M = B rows) and final_layer.linear.  Operands go through LDS in 128 x 16 tiles, two
//                            buffers; the weight is the state dict's [N][K] rows, concatenated and zero-padded to a multiple of 128 rows at load.
//   launch_dit_ln_modulate   LayerNorm(eps 1e-6, no affine, biased variance) (1 + scale[b]) + shift[b], one wave per row
//   launch_dit_patch_embed   PatchEmbed (conv with stride = kernel = patch) of c_in x, + bias + pos_embed
//   launch_dit_unpatchify    nhwpqc -> nchpwq scatter of final_layer.linear's rows with the three FwdIO epilogue modes
//   launch_dit_cond          c = time embedding (+ label embedding); SiLU(c), the input of every adaLN_modulation
//   launch_dit_linear_x3, launch_dit_attention_x3, launch_dit_split_weight
//                            the split-bf16 (f32x3) mode's token linear and key-tiled self-attention (below)
#pragma once
#include "adf_common.h"

namespace adf {

constexpr int kDitTileM = 128, kDitTileN = 128, kDitTileK = 16;
constexpr int kDitEpiBias = 0;      // acc + bias
constexpr int kDitEpiGelu = 1;      // nn.GELU(approximate="tanh") of acc + bias
constexpr int kDitEpiGate = 2;      // res + gate[row / T][n] (acc + bias)

struct DitLinearArgs {
    const float* x = nullptr;       // [M][K], 16-byte aligned
    const float* w = nullptr;       // [round_up(N, 128)][K]: rows from N on are zero
    const float* bias = nullptr;    // [N] or null
    float* y = nullptr;             // [M][N]
    int M = 0, N = 0, K = 0;        // K a multiple of 16
    int epi = kDitEpiBias;
    const float* res = nullptr;     // kDitEpiGate: [M][N]; may be y (every element is read and written by one thread)
    const float* gate = nullptr;    // kDitEpiGate: gate[b * gate_bstride + n], b = row / T
    int gate_bstride = 0, T = 1;
    float* pre = nullptr;           // kDitEpiGate: where given, acc + bias is also stored here ([M][N]: the branch before its gate, a debug tap)
};
const char* launch_dit_linear(const DitLinearArgs& a, hipStream_t s);

// ---- split-bf16 (f32x3) mode (adf_dit_x3.hip; the mode: adf_common.h) -- fp32 tensors in and out, matrix-core operands as bf16 hi + lo, three
// v_mfma_f32_32x32x16_bf16 per product (lo hi + hi lo + hi hi)
constexpr int kDitX3TileK = 32;
// fp32 [numel] -> bf16 hi and lo planes [numel]; numel a multiple of 4.  Run once per (re)load on the padded weight buffer: padding rows stay zero.
const char* launch_dit_split_weight(const float* w, unsigned short* hi, unsigned short* lo, long long numel, hipStream_t s);
// launch_dit_linear on split operands: a.w is not read, the weight comes as the planes [round_up(N, 128)][K] of launch_dit_split_weight; K a
// multiple of 32; the activation is split inside the kernel.  Same epilogues, same guards (res == y allowed).
const char* launch_dit_linear_x3(const DitLinearArgs& a, const unsigned short* w_hi, const unsigned short* w_lo, hipStream_t s);
// out[b][n][h D + :] = softmax(q k^T / sqrt(D)) v per (sample, head) on qkv rows [B N][3 C] (q | k | v blocks of C = heads D floats), head dim D 32
// or 64, any N >= 1: key tiles of 64 with an online softmax
const char* launch_dit_attention_x3(const float* qkv, float* out, int B, int N, int C, int heads, hipStream_t s);

// y[r][:] = (x[r][:] - mean) / sqrt(var + 1e-6) * (1 + scale[b][:]) + shift[b][:], b = r / T; shift / scale rows are mod_bstride floats apart.
// D a multiple of 4, at most 1024.
const char* launch_dit_ln_modulate(const float* x, float* y, const float* shift, const float* scale, int mod_bstride, int rows, int T, int D, hipStream_t s);

// out[b][t][d] = bias[d] + pos[t][d] + sum_{c,p,q} w[d][c][p][q] (c_in[b] x[b][c][gh p1 + p][gw p2 + q]), t = gh (W / p2) + gw.  coef: rows
// (c_in, ...) coef_bstride floats apart, or null.  C p1 p2 <= 256.
const char* launch_dit_patch_embed(const float* x, const float* coef, int coef_bstride, const float* w, const float* bias, const float* pos, float* out,
                                   int B, int C, int H, int W, int p1, int p2, int D, hipStream_t s);

// out[b][c][gh p1 + p][gw p2 + q] = epi(lin[b][gh (W / p2) + gw][(p p2 + q) C + c]); mode 0: F; 1: clamp(c_skip x_noisy + c_out F, -1, 1); 2: unclipped
const char* launch_dit_unpatchify(const float* lin, float* out, int B, int C, int H, int W, int p1, int p2, int mode, const float* x_noisy,
                                  const float* coef, int coef_bstride, hipStream_t s);

// c[r][:] = te[r * te_bstride + :] (+ ce[r * ce_bstride + :]); sc = SiLU(c).  ce may be null.
const char* launch_dit_cond(float* c, float* sc, const float* te, int te_bstride, const float* ce, int ce_bstride, int rows, int D, hipStream_t s);

}  // namespace adf
