// WaveToSpec: reflect padding + STFT + spec_fwd of a waveform as ONE exact-fp32 MFMA GEMM (adf_stft.hip; DESIGN.md "WaveToSpec").
//
//   X_c[b, k, t] = sum_{m < Kp} A_c[k, m] xpad[b, t h + m]        A_0 = w cos s, A_1 = -w sin s (adf_stft_basis), zero columns for m >= n_fft
//   out[b, c, k, t] = X_c g factor,  g = |X|^(e - 1), 0 at |X| == 0
//
// M = the F bins (32-row tiles, MT of them), N = (frame t, sample b), K = Kp = n_fft rounded up to kStftKC.  The A operand is the basis,
// repacked once at plan creation into MFMA-fragment order so that a lane's four K steps are one 16-byte load straight from L2 (no LDS: the
// waves of a block split M and never share an A row).  A wave keeps a cosine and a sine accumulator tile for the same 32 bins x 32 frames and
// feeds both from one B fragment, so |X| and g are lane-local in the epilogue and a store instruction writes two rows of 32 consecutive frames.
//
// The B operand is the audio.  A block stages the padded samples its NTB frames touch, (NTB - 1) h + Kp of them (reflection applied while
// staging, zeros where neither the signal nor its one reflection reaches), ONCE, and frame t reads sample m at staged index i = t h + m.
// LDS layout: phase-major, index i = q h + p (p < h) lives at word p QP + q, QP = NTB + kStftQPad (odd).
//   reads:  a B fragment is 32 lanes with t = t0 .. t0 + 31 at one m (the other 32 lanes at m + 1 are the instruction's second lane group):
//           the 32 addresses are CONSECUTIVE words -> 32 distinct banks, 0 conflict cycles.  A linear stage would put them at stride h, a
//           multiple of 32 words: all 32 lanes on ONE bank of ds_read_b32's 32, 31 extra cycles per read (a one-word skew per 32 still leaves
//           h / 32-word strides: 4-way at h = 128, 8-way at 256).
//   writes: a lane group holds 32 consecutive i that start at a multiple of 32, so one q (h is a multiple of 32) and 32 consecutive p: stride
//           QP = 41 or 73 words, both 9 mod 32 and odd -> 32 distinct banks, 0 conflict cycles.
// q < NTB + D - 1 (Kp <= D h because h is a multiple of kStftKC), hence kStftQPad = 9 >= kIstftMaxD - 1 with QP odd for NTB = 32 and 64.
#pragma once
#include "adf_common.h"
#include "adf_istft.h"

namespace adf {

constexpr int kStftKC = 32;             // window positions per K-loop iteration (8 x 16-byte A loads per lane); n_fft is padded to a multiple of it
constexpr int kStftQPad = 9;            // see above

// g = r^(e - 1) from r2 = r^2; every mode gives 0 at r2 == 0
constexpr int kStftPowOne = 0;          // e == 1: g = 1
constexpr int kStftPowHalf = 1;         // e == 0.5: g = r2^(-1/4) = rsqrt(sqrt(r2))
constexpr int kStftPowFifth = 2;        // e == 0.2: g = r2^(-2/5): exp2(-0.4 log2 r2) on the transcendental unit, then one Newton step on g^-5 = r2^2
constexpr int kStftPowGeneral = 3;      // g = powf(r2, (e - 1) / 2)

struct StftArgs {
    const float* audio = nullptr;       // [B][L], rows 4-byte aligned
    float* spec = nullptr;              // [B][2][F][T]
    const f32x4_hw_t* apack = nullptr;  // [MT][NKI][2 components][4][64 lanes] x 4: element q of lane l = basis_c[32 mt + (l & 31)][32 it + 8 g + 2 q + (l >> 5)]
    int B = 0, L = 0, T = 0, F = 0, h = 0, half = 0;
    int MT = 0;                         // ceil(F / 32): 32-row M tiles (rows past F are zero in apack)
    int NKI = 0;                        // Kp / kStftKC: K-loop iterations
    int pmode = 0;                      // kStftPow*
    float pexp = 0.f;                   // (e - 1) / 2 (kStftPowGeneral)
    float factor = 1.f;                 // spec_factor
};

// frame tiles per block: with one or two bin tiles (n_fft <= 126) two waves of a block take a second frame tile instead of idling.  Not at
// h > 128, where the stage for 64 frames (h x 73 words) passes the 64 KiB of LDS a launch gets without asking for more.
inline int stft_wn(int F, int h) { return F <= 64 && h <= 128 ? 2 : 1; }

inline size_t stft_lds_bytes(int wn, int h) { return (size_t)h * (32 * wn + kStftQPad) * sizeof(float); }

hipError_t launch_stft(const StftArgs& a, hipStream_t s);

}  // namespace adf
