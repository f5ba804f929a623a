// The validation loss behind adf_diffusion_loss (Diffusion.forward, src/models/components/diffusion.py:65-97, :185-218; ReFlow.forward :420-442)
// around the denoiser: the noising of the clean input before it and the weighted per-sample mean squared error after it (adf_loss.hip; DESIGN.md
// section 14).  Both run on the rows of a [B][N] tensor, N = C * L elements per sample, whose pointers are only 4-byte aligned.
//
// Row geometry (shared by the mix and the partial kernel): row b starts at element b N, so with N % 4 != 0 its start is not 16-byte aligned even
// where the tensor is.  `phase` = (address / 4) % 4 of every pointer of the launch when they agree, else -1.  With a phase, row b has
//   head = min(N, (4 - (phase + b N) % 4) % 4) scalar elements, then nv = (N - head) / 4 aligned 16-byte vectors, then tail = N - head - 4 nv
// scalar elements; without one the whole row is "head" and goes element by element.  The grid is (chunks, B), chunks = ceil(N / kLossChunk):
// block (c, b) takes the vectors [c, c + 1) kLossChunk / 4 of row b (none, where the head shortened the body), block (0, b) also the head and
// the tail.  kLossChunk is a constant of the source, not of the device: the partial sums of a sample, and so its loss, do not depend on the CU count.
#pragma once
#include "adf_common.h"

namespace adf {

constexpr int kLossChunk = 4096;        // elements of a row per block: 256 threads x 4 vectors of 4 floats
constexpr int kLossThreads = 256;

// the loss kinds of include/audiodiffuser_amd.h (ADF_LOSS_*)
constexpr int kLossX0Edm = 0;           // w = (s^2 + sd^2) / (s sd)^2, d = pred - x
constexpr int kLossX0InvSigma2 = 1;     // w = 1 / s^2,                 d = pred - x
constexpr int kLossRf = 2;              // w = 1,                       d = (noise - x) - pred; the coefficient is the time t

inline int loss_chunks(long long N) { return (int)((N + kLossChunk - 1) / kLossChunk); }

// x_noisy[b][i] = fl(x + fl(s_b noise)) (rf == 0) or fl(fl(fl(1 - t_b) x) + fl(t_b noise)) (rf != 0): every operation rounded to fp32 on its own
const char* launch_loss_mix(float* x_noisy, const float* x, const float* noise, const float* coef_dev, int rf, int B, long long N, hipStream_t s);
// partial[b][c] (double, [B][loss_chunks(N)]) = the sum over block (c, b)'s elements of fl(d d), d = fl(pred - x), or with `noise`
// d = fl(fl(noise - x) - pred); accumulated in double per thread, combined in a fixed order: no atomics, the same bits on every run
const char* launch_loss_partial(double* partial, const float* pred, const float* x, const float* noise, int B, long long N, hipStream_t s);
// losses[b] = (float)(w(s_b) / N * sum_c partial[b][c]), the chunks summed in index order and w formed in double from the fp32 sigma
const char* launch_loss_finalize(float* losses, const double* partial, const float* sigmas_dev, int kind, float sigma_data, int B, long long N,
                                 hipStream_t s);

}  // namespace adf
