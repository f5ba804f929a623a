// SpecToWave: spec_back + inverse STFT of the sampled spectrogram as ONE exact-fp32 MFMA GEMM (adf_istft.hip; DESIGN.md "SpecToWave").
//
//   y[b, j h + n] = (1 / env) * sum_{d < D} [0 <= j - d < T] sum_k ( C[d h + n, k] Z_0[b, k, j - d] + S[d h + n, k] Z_1[b, k, j - d] )
//
// M = the h samples of a hop block, N = (hop block j, sample b), K = D * 2 * Fp (Fp = F rounded up to kIstftKC, zero basis columns).
// The A operand is the basis, repacked once at plan creation into MFMA-fragment order so that a lane's four K steps are one 16-byte load
// straight from L2 (no LDS: the waves of a block split M and never share an A row).  The B operand is the spectrogram after spec_back:
// a K chunk of kIstftKC bins x both components is staged once in LDS for frames j0 - (D - 1) .. j0 + NTB - 1, and segment d reads it shifted
// by D - 1 - d columns.
#pragma once
#include "adf_common.h"

namespace adf {

constexpr int kIstftKC = 32;            // frequency bins per staged K chunk (x 2 components); F is padded to a multiple of it
constexpr int kIstftMaxD = 8;           // ceil(n_fft / hop): the stage keeps 8 spare columns for the D - 1 earlier frames

// |Z| = r^(1/e): the factor g = r^(1/e - 1) that multiplies both components
constexpr int kIstftPowOne = 0;         // e == 1: g = 1
constexpr int kIstftPowTwo = 1;         // 1/e == 2: g = r
constexpr int kIstftPowFive = 2;        // 1/e == 5: g = (r^2)^2
constexpr int kIstftPowGeneral = 3;     // g = powf(r, 1/e - 1), 0 at r == 0

struct IstftArgs {
    const float* spec = nullptr;        // [B][2][F][T]
    float* audio = nullptr;             // [B][audio_len]
    const f32x4_hw_t* apack = nullptr;  // [D][MT][NCH][2 components][4][64 lanes] x 4: element q of lane l = basis_c[d h + 32 mt + (l & 31)][32 ch + 8 sg + 2 q + (l >> 5)]
    const float* wsq = nullptr;         // [D h]: w^2, zero past n_fft
    int B = 0, T = 0, F = 0, h = 0, D = 0, half = 0, audio_len = 0;
    int MT = 0;                         // h / 32: 32-row M tiles
    int NCH = 0;                        // Fp / kIstftKC: K chunks
    int jlo = 0, nj = 0;                // the hop blocks that hold kept samples: jlo .. jlo + nj - 1
    int pmode = 0;                      // kIstftPow*
    float pexp = 0.f;                   // 1/e - 1 (kIstftPowGeneral)
    float factor = 1.f;                 // spec_factor
};

// hop blocks per block: narrow hops give the waves of a block more hop blocks instead of more rows
inline int istft_wn(int h) { return h == 32 ? 4 : h == 64 ? 2 : 1; }

hipError_t launch_istft(const IstftArgs& a, hipStream_t s);

}  // namespace adf
