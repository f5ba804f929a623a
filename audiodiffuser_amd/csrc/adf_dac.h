// Kernels of the DAC decoder and encoder stacks (reference: src/models/backbones/dac/dac.py:17-137, dac/layers.py:8-32, dac_vae.py:6-71), exact fp32 on
// channels-last activations [B][L][C] (adf_dac.hip; the walk is adf_net_dac.hip).  Every launcher returns nullptr or a static string; none
// allocates, synchronises or copies, so all of them can be captured.
//
//   launch_dac_conv          Snake -> Conv1d (k in {1, 3, 7}, dilation in {1, 3, 9}, "same" zero padding) -> + bias (-> + residual), and
//                            Snake -> ConvTranspose1d (kernel 2 s, stride s, padding ceil(s / 2)) -> + bias, as one implicit GEMM on
//                            v_mfma_f32_32x32x2_f32: M = positions of one sample, N = C_out (conv) or s C_out phase-major (transposed), K = taps x C_in;
//                            and Snake -> Conv1d (kernel 2 s, stride s, padding ceil(s / 2)) -> + bias, the encoder's down conv, as the same GEMM
//                            over frames of s C_in floats: M = output positions, N = C_out, K = 2 taps x s C_in
//   launch_dac_out           Snake -> Conv1d(C -> 1, k = 7, padding 3) -> tanh, written as the reference's [B][1][L]: a streaming kernel
//   launch_dac_in            Conv1d(1 -> C, k = 7, padding 3) straight from the reference's [B][1][L] to channels-last: a streaming kernel
//   launch_dac_btnk          the VAE bottleneck behind its 1x1 conv: mean (tanh), clamp of logvar, KL in a fixed order
//   launch_dac_transpose     [B][R][C] -> [B][C][R]: the [B][C][T] input to channels-last, and the autoencoder's result back
//   launch_dac_fold          weight norm folded and packed: w = g v / ||v|| (norm over all axes but 0) into the layout of the kernel that reads it
#pragma once
#include "adf_common.h"

namespace adf {

constexpr int kDacTileM = 128;      // positions of a workgroup's tile: four waves of 32 rows
constexpr int kDacTileN = 128;      // most outputs of a workgroup's tile: one to four 32-column MFMA tiles per wave, a divisor of N / 32 per launch
constexpr int kDacTileK = 32;       // input channels staged per step
constexpr int kDacMaxHalo = 27;     // (7 - 1) / 2 * 9
constexpr int kDacPitch = 33;       // LDS row pitch in floats: 32 rows of a fragment read land in 32 banks
constexpr int kDacOutTile = 256;    // positions of a workgroup of the output kernel

// Snake: x + sin^2(alpha x) / (alpha + 1e-9), alpha per channel (layers.py:18-23).  sinf, not the hardware sine: the bar is exact fp32.
struct DacConvArgs {
    const float* x = nullptr;       // [B][Lin][Cin], 16-byte aligned
    const float* alpha = nullptr;   // [Cin] or null: no Snake on the input
    const float* w = nullptr;       // packed by launch_dac_fold (kind kDacFoldConv / kDacFoldConvT)
    const float* bias = nullptr;    // [Cout]
    const float* res = nullptr;     // [B][Lin][Cout] or null: added in the epilogue (conv only)
    float* y = nullptr;             // [B][Lout][Cout]
    int B = 0, Lin = 0, Cin = 0, Cout = 0;      // Cin a multiple of 4, Cout of 32 (conv: any Cout >= 1, the packed weight zero-padded to 32 columns)
    int taps = 1, dil = 1;          // conv: taps in {1, 3, 7}, dilation in {1, 3, 9}
    int stride = 0;                 // > 0: the transposed conv of this stride (taps and dil are not read); Lout = (Lin - 1) s - 2 ceil(s / 2) + 2 s
    int down = 0;                   // > 0: the strided conv of this stride (kernel 2 s; Cin a multiple of 32; taps, dil, stride and res are not read); Lout = dac_down_length
};
const char* launch_dac_conv(const DacConvArgs& a, hipStream_t s);
inline int dac_up_length(int L, int s) { return (L - 1) * s - 2 * ((s + 1) / 2) + 2 * s; }
// Conv1d(kernel 2 s, stride s, padding p = ceil(s / 2)): floor((L + 2 p - 2 s) / s) + 1, i.e. L / s for even s and (L + 1) / s for odd s; L >= 2 s - 2 p
inline int dac_down_min_length(int s) { return 2 * s - 2 * ((s + 1) / 2); }
inline int dac_down_length(int L, int s) { return (L + 2 * ((s + 1) / 2) - 2 * s) / s + 1; }
// floats of the packed weight of a conv (stride 0; the down conv of stride s is one of 2 taps over s Cin) or a transposed conv
inline long long dac_packed_floats(int Cin, int Cout, int taps, int stride) {
    const long long kp = round_up(Cin, kDacTileK);
    return stride > 0 ? 2 * kp * (long long)stride * Cout : (long long)taps * kp * round_up(Cout, 32);
}

// out[b][0][l] = tanh(bias + sum_{t, c} w[t][c] snake(x[b][l + t - 3][c])); pre (or null): the sum before tanh, same layout.  C a multiple of 32.
const char* launch_dac_out(const float* x, const float* alpha, const float* w, const float* bias, float* out, float* pre, int B, int L, int C, hipStream_t s);

// y[b][l][c] = bias[c] + sum_t w[t][c] x[b][0][l + t - 3] (zero outside [0, L)); w packed by kDacFoldIn.  C a multiple of 4.
const char* launch_dac_in(const float* x, const float* w, const float* bias, float* y, int B, int L, int C, hipStream_t s);

// The bottleneck of FineTuneAutoencoder.encode (dac_vae.py:56-61) behind btnk_layer: raw is [B][T][2 D] channels-last; mean[b][c][t] = raw[b][t][c]
// (tanh of it with tanh_mean), logvar = clamp(raw[b][t][D + c], -30, 20), kl[0] = 0.5 / B sum_b sum_{c, t} (mean^2 + exp(logvar) - logvar - 1).
// The sum runs in a fixed order in double: block sums into partial[b][dac_btnk_chunks(D T)], then one block over every sample's chunks and the batch
// -- no atomics, so kl is bit-reproducible.  partial: B * dac_btnk_chunks(D * T) doubles of scratch.
constexpr int kDacBtnkChunk = 4096;
inline int dac_btnk_chunks(long long n) { return (int)((n + kDacBtnkChunk - 1) / kDacBtnkChunk); }
const char* launch_dac_btnk(const float* raw, float* mean, float* kl, double* partial, int B, int T, int D, int tanh_mean, hipStream_t s);

// out[b][c][r] = in[b][r][c]
const char* launch_dac_transpose(const float* in, float* out, int B, int R, int C, hipStream_t s);

constexpr int kDacFoldConv = 0;     // v [Cout][Cin][taps], g [Cout] -> the MFMA operand order of launch_dac_conv
constexpr int kDacFoldConvT = 1;    // v [Cin][Cout][2 s], g [Cin] (axis 0 of a ConvTranspose1d is the INPUT channel) -> phase-major operand, taps = 2
constexpr int kDacFoldOut = 2;      // v [1][C][7], g [1] -> [7][C]
constexpr int kDacFoldDown = 3;     // v [Cout][Cin][2 s], g [Cout] -> two taps over the frame index k = q Cin + c: W_t[k][co] = w[co][c][t s + q]
constexpr int kDacFoldIn = 4;       // v [C][1][7], g [C] -> [7][C] (Cin = 1, Cout = C)
constexpr int kDacFoldPlain = 5;    // v [Cout][Cin][1] of a plain nn.Conv1d (g is not read: scale 1) -> the conv operand, N zero-padded to a multiple of 32
// scale: scratch of one float per axis-0 row.  packed: dac_packed_floats (kinds 2 and 4: 7 C; kind 3: of (s Cin, Cout, 2, 0)) floats, all of them written
// (the K and N padding as zeros).
const char* launch_dac_fold(int kind, const float* g, const float* v, float* scale, float* packed, int Cin, int Cout, int taps, int stride, hipStream_t s);

}  // namespace adf
