// Kernels of the DAC decoder stack (reference: src/models/backbones/dac/dac.py:17-137, dac/layers.py:8-32, dac_vae.py:37-71), exact fp32 on
// channels-last activations [B][L][C] (adf_dac.hip; the walk is adf_net_dac.hip).  Every launcher returns nullptr or a static string; none
// allocates, synchronises or copies, so all of them can be captured.
//
//   launch_dac_conv          Snake -> Conv1d (k in {1, 3, 7}, dilation in {1, 3, 9}, "same" zero padding) -> + bias (-> + residual), and
//                            Snake -> ConvTranspose1d (kernel 2 s, stride s, padding ceil(s / 2)) -> + bias, as one implicit GEMM on
//                            v_mfma_f32_32x32x2_f32: M = positions of one sample, N = C_out (conv) or s C_out phase-major (transposed), K = taps x C_in
//   launch_dac_out           Snake -> Conv1d(C -> 1, k = 7, padding 3) -> tanh, written as the reference's [B][1][L]: a streaming kernel
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
    int B = 0, Lin = 0, Cin = 0, Cout = 0;      // Cin a multiple of 4, Cout of 32
    int taps = 1, dil = 1;          // conv: taps in {1, 3, 7}, dilation in {1, 3, 9}
    int stride = 0;                 // > 0: the transposed conv of this stride (taps and dil are not read); Lout = (Lin - 1) s - 2 ceil(s / 2) + 2 s
};
const char* launch_dac_conv(const DacConvArgs& a, hipStream_t s);
inline int dac_up_length(int L, int s) { return (L - 1) * s - 2 * ((s + 1) / 2) + 2 * s; }
// floats of the packed weight of a conv (stride 0) or a transposed conv
inline long long dac_packed_floats(int Cin, int Cout, int taps, int stride) {
    const long long kp = round_up(Cin, kDacTileK);
    return stride > 0 ? 2 * kp * (long long)stride * Cout : (long long)taps * kp * Cout;
}

// out[b][0][l] = tanh(bias + sum_{t, c} w[t][c] snake(x[b][l + t - 3][c])); pre (or null): the sum before tanh, same layout.  C a multiple of 32.
const char* launch_dac_out(const float* x, const float* alpha, const float* w, const float* bias, float* out, float* pre, int B, int L, int C, hipStream_t s);

// out[b][c][r] = in[b][r][c]
const char* launch_dac_transpose(const float* in, float* out, int B, int R, int C, hipStream_t s);

constexpr int kDacFoldConv = 0;     // v [Cout][Cin][taps], g [Cout] -> the MFMA operand order of launch_dac_conv
constexpr int kDacFoldConvT = 1;    // v [Cin][Cout][2 s], g [Cin] (axis 0 of a ConvTranspose1d is the INPUT channel) -> phase-major operand, taps = 2
constexpr int kDacFoldOut = 2;      // v [1][C][7], g [1] -> [7][C]
// scale: scratch of one float per axis-0 row.  packed: dac_packed_floats (kind 2: 7 C) floats, all of them written (the K padding as zeros).
const char* launch_dac_fold(int kind, const float* g, const float* v, float* scale, float* packed, int Cin, int Cout, int taps, int stride, hipStream_t s);

}  // namespace adf
