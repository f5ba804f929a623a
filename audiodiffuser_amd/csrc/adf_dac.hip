// Kernels of the DAC decoder and encoder stacks (adf_dac.h), exact fp32.
#include "adf_dac.h"

#define DAC_LAUNCH_CHECK(name) (hipGetLastError() == hipSuccess ? nullptr : name ": launch failed")

namespace adf {

typedef float dac_f32x16_t __attribute__((ext_vector_type(16)));
typedef float dac_f32x4_t __attribute__((ext_vector_type(4)));

// x + sin^2(alpha x) / (alpha + 1e-9) with inv = 1 / (alpha + 1e-9): at alpha = 0 the sine is 0 and the result is x, as in the reference
__device__ __forceinline__ float dac_snake(float x, float alpha, float inv) {
    const float sn = sinf(alpha * x);
    return x + inv * (sn * sn);
}

// =====================================================================================================
// Snake -> conv / transposed conv as an implicit GEMM on v_mfma_f32_32x32x2_f32
// =====================================================================================================
// A workgroup of four waves owns 128 positions x up to 128 outputs of ONE sample (grid.z = sample: a tile and its halo never see a neighbouring
// sample; rows outside [0, Lin) are staged as zeros, and snake(0) = 0).  Wave w owns rows 32 w .. 32 w + 31 and all of the tile's 32-column MFMA
// tiles (up to four accumulators).  Per step of 32 input channels the tile's rows with their halo are staged once into LDS -- Snake applied there, once
// per element, with the step's four alphas of a thread read once -- and every tap reads them at its row offset.  The B operand comes straight from the
// packed weight: launch_dac_fold lays it out so that the 64 lanes of one MFMA read 64 consecutive floats.
// The transposed conv (kernel 2 s, stride s, padding p = ceil(s / 2)) is the same GEMM with two taps at row offsets 0 and -1, N = s C_out columns
// (phase, c_out) and Lin + 1 rows: row m, phase f is output position m s + f - p (dropped outside [0, Lout)).
// The strided conv of the encoder (kernel 2 s, stride s, padding p = ceil(s / 2)) is the transposed conv's dual.  View the input as frames of s C_in
// floats that start at position -p: frame[j][q C_in + c] = x[j s - p + q][c].  Then out[m] = frame[m] W_0 + frame[m + 1] W_1: two taps at row offsets
// 0 and +1 over K = s C_in, N = C_out, Lout rows.  C_in is a multiple of 32, so a K step of 32 lies inside one input position q: the step stages 129
// frame rows of 32 floats each (row r is position (m0 + r) s - p + q, guarded per row), and Snake's alpha index is the channel k mod C_in.
// MODE: 0 the conv, 1 the transposed conv, 2 the strided conv.
// NJ: 32-column MFMA tiles per wave, the same for every workgroup of a launch (the launcher picks a divisor of N / 32), so the B loads and MFMAs of a step
// are straight-line code: a per-tile guard inside the step would put a branch between every load and its MFMA and expose each load's latency.
constexpr int kDacConv = 0, kDacUp = 1, kDacDown = 2;
template <int MODE, int NJ>
__global__ void __launch_bounds__(256) dac_conv_kernel(const DacConvArgs a, const int N, const int lo, const int hi, const int Mrows, const int Lout) {
    __shared__ float sA[(kDacTileM + 2 * kDacMaxHalo) * kDacPitch];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l31 = lane & 31, kh = lane >> 5;
    const int m0 = blockIdx.x * kDacTileM, n0 = blockIdx.y * (NJ * 32), b = blockIdx.z;
    const int NB = N >> 5, nb0 = n0 >> 5;
    constexpr bool UP = MODE == kDacUp, DOWN = MODE == kDacDown;
    const int nkc = DOWN ? a.down * a.Cin / kDacTileK : (a.Cin + kDacTileK - 1) / kDacTileK;
    const int rows = kDacTileM + hi - lo;
    const int ntap = UP || DOWN ? 2 : a.taps;
    const float* __restrict__ xb = a.x + (size_t)b * a.Lin * a.Cin;
    dac_f32x16_t acc[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[j][e] = 0.f;
    const int c4 = (tid & 7) * 4;
    for (int kc = 0; kc < nkc; ++kc) {
        if (kc) __syncthreads();
        const int q = DOWN ? kc * kDacTileK / a.Cin : 0;                     // down: the position inside the frame that this K step lies in
        const int ch = kc * kDacTileK - q * a.Cin + c4;
        const bool chv = ch < a.Cin;                 // Cin is a multiple of 4: a quad is inside or outside as a whole
        float al[4] = {0.f, 0.f, 0.f, 0.f}, inv[4] = {0.f, 0.f, 0.f, 0.f};
        if (a.alpha && chv) {
#pragma unroll
            for (int i = 0; i < 4; ++i) { al[i] = a.alpha[ch + i]; inv[i] = 1.0f / (al[i] + 1e-9f); }
        }
        for (int r = tid >> 3; r < rows; r += 32) {
            const int pos = DOWN ? (m0 + r) * a.down - (a.down + 1) / 2 + q : m0 + lo + r;
            dac_f32x4_t v = {0.f, 0.f, 0.f, 0.f};
            if (chv && pos >= 0 && pos < a.Lin) {
                v = *(const dac_f32x4_t*)(xb + (size_t)pos * a.Cin + ch);
                if (a.alpha) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) v[i] = dac_snake(v[i], al[i], inv[i]);
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) sA[r * kDacPitch + c4 + i] = v[i];
        }
        __syncthreads();
        for (int t = 0; t < ntap; ++t) {
            const int off = UP ? -t : (DOWN ? t : t * a.dil - hi);          // conv: hi = pad = (taps - 1) / 2 * dil
            const float* sa = sA + (wave * 32 + l31 + off - lo) * kDacPitch + kh;
            const float* __restrict__ wp = a.w + ((size_t)(t * nkc + kc) * 16 * NB + nb0) * 64 + lane;
#pragma unroll
            for (int k0 = 0; k0 < 16; k0 += 8) {
                float av[8], bv[8][NJ];
#pragma unroll
                for (int kk = 0; kk < 8; ++kk) {
                    av[kk] = sa[2 * (k0 + kk)];
#pragma unroll
                    for (int j = 0; j < NJ; ++j) bv[kk][j] = wp[((size_t)(k0 + kk) * NB + j) * 64];
                }
#pragma unroll
                for (int kk = 0; kk < 8; ++kk)
#pragma unroll
                    for (int j = 0; j < NJ; ++j) acc[j] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[kk], bv[kk][j], acc[j], 0, 0, 0);
            }
        }
    }
    // C/D map of the 32 x 32 MFMA: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int col = n0 + j * 32 + l31;
        const int phase = UP ? col / a.Cout : 0;
        const int co = UP ? col - phase * a.Cout : col;
        if (!UP && co >= a.Cout) continue;           // (a conv whose N is zero-padded to 32 columns: the bottleneck)
        const float bv = a.bias[co];
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = m0 + wave * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
            if (row >= Mrows) continue;
            if (UP) {
                const int jp = row * a.stride + phase - (a.stride + 1) / 2;
                if (jp < 0 || jp >= Lout) continue;
                a.y[((size_t)b * Lout + jp) * a.Cout + co] = acc[j][r] + bv;
            } else if (DOWN) {
                a.y[((size_t)b * Lout + row) * a.Cout + co] = acc[j][r] + bv;
            } else {
                const size_t o = ((size_t)b * a.Lin + row) * a.Cout + co;
                float v = acc[j][r] + bv;
                if (a.res) v += a.res[o];
                a.y[o] = v;
            }
        }
    }
}

const char* launch_dac_conv(const DacConvArgs& a, hipStream_t s) {
    if (!a.x || !a.w || !a.bias || !a.y) return "dac_conv: null operand";
    if (a.B < 1 || a.B > 65535 || a.Lin < 1) return "dac_conv: B in [1, 65535] and Lin >= 1";
    const bool up = a.stride > 0, down = a.down > 0;
    if (a.Cin < 4 || a.Cin % 4 || a.Cout < 1 || ((up || down) && a.Cout % 32)) return "dac_conv: Cin a multiple of 4, Cout a multiple of 32";
    if ((uintptr_t)a.x & 15) return "dac_conv: x must be 16-byte aligned";
    int lo, hi, N, M, Lout;
    if (down) {
        if (up) return "dac_conv: stride and down are exclusive";
        if (a.down < 2 || a.down > 16 || a.Cin % 32) return "dac_conv: down stride in [2, 16], Cin a multiple of 32";
        if (a.res) return "dac_conv: no residual on the strided conv";
        if (a.Lin < dac_down_min_length(a.down) || a.Lin > (1 << 30)) return "dac_conv: input too short or too long for the strided conv";
        lo = 0; hi = 1; N = a.Cout; Lout = dac_down_length(a.Lin, a.down); M = Lout;
    } else if (up) {
        if (a.stride < 2 || a.stride > 16) return "dac_conv: transposed stride in [2, 16]";
        if (a.res) return "dac_conv: no residual on the transposed conv";
        lo = -1; hi = 0; N = a.stride * a.Cout; M = a.Lin + 1; Lout = dac_up_length(a.Lin, a.stride);
        if ((long long)a.Lin * a.stride > (1 << 30)) return "dac_conv: output too long";
    } else {
        if (a.taps != 1 && a.taps != 3 && a.taps != 7) return "dac_conv: taps in {1, 3, 7}";
        if (a.dil != 1 && a.dil != 3 && a.dil != 9) return "dac_conv: dilation in {1, 3, 9}";
        hi = (a.taps - 1) / 2 * a.dil; lo = -hi; N = round_up(a.Cout, 32); M = a.Lin; Lout = a.Lin;
    }
    const long long mt = ((long long)M + kDacTileM - 1) / kDacTileM;
    const int NB = N / 32;
    const int nj = NB % 4 == 0 ? 4 : (NB % 3 == 0 ? 3 : (NB % 2 == 0 ? 2 : 1));      // every workgroup of the launch owns nj whole MFMA tiles
    const int nt = NB / nj;
    if (mt > 0x7fffffffLL || nt > 65535) return "dac_conv: grid too large";
    const dim3 grid((unsigned)mt, (unsigned)nt, (unsigned)a.B);
#define DAC_CONV_LAUNCH(UPV, NJV) hipLaunchKernelGGL((dac_conv_kernel<UPV, NJV>), grid, dim3(256), 0, s, a, N, lo, hi, M, Lout)
    if (up) { if (nj == 4) DAC_CONV_LAUNCH(kDacUp, 4); else if (nj == 3) DAC_CONV_LAUNCH(kDacUp, 3); else if (nj == 2) DAC_CONV_LAUNCH(kDacUp, 2); else DAC_CONV_LAUNCH(kDacUp, 1); }
    else if (down) { if (nj == 4) DAC_CONV_LAUNCH(kDacDown, 4); else if (nj == 3) DAC_CONV_LAUNCH(kDacDown, 3); else if (nj == 2) DAC_CONV_LAUNCH(kDacDown, 2); else DAC_CONV_LAUNCH(kDacDown, 1); }
    else { if (nj == 4) DAC_CONV_LAUNCH(kDacConv, 4); else if (nj == 3) DAC_CONV_LAUNCH(kDacConv, 3); else if (nj == 2) DAC_CONV_LAUNCH(kDacConv, 2); else DAC_CONV_LAUNCH(kDacConv, 1); }
#undef DAC_CONV_LAUNCH
    return DAC_LAUNCH_CHECK("dac_conv");
}

// =====================================================================================================
// Output: Snake -> Conv1d(C -> 1, k = 7) -> tanh.  One thread per position; the tile's rows (+ 3 each side) go through LDS 32 channels at a time
// with Snake applied there; the weight index is uniform over the workgroup.
// =====================================================================================================
__global__ void __launch_bounds__(kDacOutTile) dac_out_kernel(const float* __restrict__ x, const float* __restrict__ alpha, const float* __restrict__ w,
                                                              const float* __restrict__ bias, float* __restrict__ out, float* __restrict__ pre,
                                                              const int L, const int C) {
    __shared__ float sX[(kDacOutTile + 6) * kDacPitch];
    const int tid = threadIdx.x, b = blockIdx.y, l0 = blockIdx.x * kDacOutTile;
    const float* __restrict__ xb = x + (size_t)b * L * C;
    const int c4 = (tid & 7) * 4;
    float acc = 0.f;
    for (int c0 = 0; c0 < C; c0 += 32) {
        if (c0) __syncthreads();
        float al[4], inv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) { al[i] = alpha[c0 + c4 + i]; inv[i] = 1.0f / (al[i] + 1e-9f); }
        for (int r = tid >> 3; r < kDacOutTile + 6; r += kDacOutTile / 8) {
            const int pos = l0 - 3 + r;
            dac_f32x4_t v = {0.f, 0.f, 0.f, 0.f};
            if (pos >= 0 && pos < L) {
                v = *(const dac_f32x4_t*)(xb + (size_t)pos * C + c0 + c4);
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] = dac_snake(v[i], al[i], inv[i]);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) sX[r * kDacPitch + c4 + i] = v[i];
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 7; ++t) {
            const float* sx = sX + (tid + t) * kDacPitch;
            const float* __restrict__ wt = w + (size_t)t * C + c0;
#pragma unroll 8
            for (int c = 0; c < 32; ++c) acc = fmaf(sx[c], wt[c], acc);
        }
    }
    const int l = l0 + tid;
    if (l < L) {
        const float v = acc + bias[0];
        if (pre) pre[(size_t)b * L + l] = v;
        out[(size_t)b * L + l] = tanhf(v);
    }
}

const char* launch_dac_out(const float* x, const float* alpha, const float* w, const float* bias, float* out, float* pre, int B, int L, int C, hipStream_t s) {
    if (!x || !alpha || !w || !bias || !out) return "dac_out: null operand";
    if (B < 1 || B > 65535 || L < 1 || C < 32 || C % 32) return "dac_out: B in [1, 65535], L >= 1, C a multiple of 32";
    if ((uintptr_t)x & 15) return "dac_out: x must be 16-byte aligned";
    hipLaunchKernelGGL(dac_out_kernel, dim3((unsigned)ceil_div(L, kDacOutTile), (unsigned)B), dim3(kDacOutTile), 0, s, x, alpha, w, bias, out, pre, L, C);
    return DAC_LAUNCH_CHECK("dac_out");
}

// =====================================================================================================
// Input: Conv1d(1 -> C, k = 7, padding 3) from [B][1][L] to channels-last [B][L][C].  The mirror of dac_out_kernel: it reads one float per position and
// writes C, so it streams.  A workgroup owns kDacInTile positions (+ 3 each side in LDS); a thread keeps one channel quad's seven taps and bias in
// registers and walks the tile's positions, so the 64 lanes of a wave store consecutive quads of consecutive rows.
// =====================================================================================================
constexpr int kDacInTile = 256;
__global__ void __launch_bounds__(256) dac_in_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ bias,
                                                     float* __restrict__ y, const int L, const int C) {
    __shared__ float sX[kDacInTile + 6];
    const int tid = threadIdx.x, b = blockIdx.y, l0 = blockIdx.x * kDacInTile;
    const float* __restrict__ xb = x + (size_t)b * L;
    for (int r = tid; r < kDacInTile + 6; r += 256) {
        const int pos = l0 - 3 + r;
        sX[r] = pos >= 0 && pos < L ? xb[pos] : 0.f;
    }
    __syncthreads();
    const int nq = C >> 2, qw = nq < 256 ? nq : 256, rstep = 256 / qw;          // qw quads side by side, rstep rows per pass
    const int r0 = tid / qw;
    if (r0 >= rstep) return;
    const int nrow = L - l0 < kDacInTile ? L - l0 : kDacInTile;
    for (int qd = tid - r0 * qw; qd < nq; qd += qw) {
        dac_f32x4_t wt[7];
#pragma unroll
        for (int t = 0; t < 7; ++t) wt[t] = *(const dac_f32x4_t*)(w + (size_t)t * C + 4 * qd);
        const dac_f32x4_t bv = *(const dac_f32x4_t*)(bias + 4 * qd);
        for (int r = r0; r < nrow; r += rstep) {
            dac_f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int t = 0; t < 7; ++t) {
                const float xv = sX[r + t];
#pragma unroll
                for (int i = 0; i < 4; ++i) acc[i] = fmaf(xv, wt[t][i], acc[i]);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i] += bv[i];
            *(dac_f32x4_t*)(y + ((size_t)b * L + l0 + r) * C + 4 * qd) = acc;
        }
    }
}

const char* launch_dac_in(const float* x, const float* w, const float* bias, float* y, int B, int L, int C, hipStream_t s) {
    if (!x || !w || !bias || !y) return "dac_in: null operand";
    if (B < 1 || B > 65535 || L < 1 || C < 4 || C % 4) return "dac_in: B in [1, 65535], L >= 1, C a multiple of 4";
    if (((uintptr_t)w | (uintptr_t)bias | (uintptr_t)y) & 15) return "dac_in: w, bias and y must be 16-byte aligned";
    hipLaunchKernelGGL(dac_in_kernel, dim3((unsigned)ceil_div(L, kDacInTile), (unsigned)B), dim3(256), 0, s, x, w, bias, y, L, C);
    return DAC_LAUNCH_CHECK("dac_in");
}

// =====================================================================================================
// Bottleneck epilogue: mean (tanh), clamp of logvar, KL.  Element e = c T + t of a sample (the order of mean's [D][T]); block (chunk, b) owns
// kDacBtnkChunk consecutive elements, each thread a fixed subset of them in ascending order, then the block's tree: one double per block.  The second
// kernel adds every sample's chunks in ascending order, then the samples in ascending order, in one thread: the same sum on every run.
// =====================================================================================================
__global__ void __launch_bounds__(256) dac_btnk_kernel(const float* __restrict__ raw, float* __restrict__ mean, double* __restrict__ partial,
                                                       const int T, const int D, const int tanh_mean) {
    __shared__ double part[256];
    const int tid = threadIdx.x, b = blockIdx.y;
    const long long n = (long long)D * T, e0 = (long long)blockIdx.x * kDacBtnkChunk;
    const float* __restrict__ rb = raw + (size_t)b * T * 2 * D;
    double sum = 0.0;
    for (int i = tid; i < kDacBtnkChunk; i += 256) {
        const long long e = e0 + i;
        if (e >= n) break;
        const int c = (int)(e / T), t = (int)(e - (long long)c * T);
        float m = rb[(size_t)t * 2 * D + c];
        float lv = rb[(size_t)t * 2 * D + D + c];
        lv = fminf(fmaxf(lv, -30.0f), 20.0f);
        if (tanh_mean) m = tanhf(m);
        mean[(size_t)b * n + e] = m;
        sum += (double)m * (double)m + (double)expf(lv) - (double)lv - 1.0;
    }
    part[tid] = sum;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) part[tid] += part[tid + st];
        __syncthreads();
    }
    if (tid == 0) partial[(size_t)b * gridDim.x + blockIdx.x] = part[0];
}

__global__ void dac_btnk_sum_kernel(const double* __restrict__ partial, float* __restrict__ kl, const int B, const int chunks) {
    if (threadIdx.x || blockIdx.x) return;
    double total = 0.0;
    for (int b = 0; b < B; ++b) {
        double sb = 0.0;
        for (int i = 0; i < chunks; ++i) sb += partial[(size_t)b * chunks + i];
        total += sb;
    }
    kl[0] = (float)(0.5 * total / (double)B);
}

const char* launch_dac_btnk(const float* raw, float* mean, float* kl, double* partial, int B, int T, int D, int tanh_mean, hipStream_t s) {
    if (!raw || !mean || !kl || !partial) return "dac_btnk: null operand";
    if (B < 1 || B > 65535 || T < 1 || D < 1) return "dac_btnk: B in [1, 65535], T >= 1, latent_dim >= 1";
    const int chunks = dac_btnk_chunks((long long)D * T);
    hipLaunchKernelGGL(dac_btnk_kernel, dim3((unsigned)chunks, (unsigned)B), dim3(256), 0, s, raw, mean, partial, T, D, tanh_mean);
    if (hipGetLastError() != hipSuccess) return "dac_btnk: launch failed";
    hipLaunchKernelGGL(dac_btnk_sum_kernel, dim3(1), dim3(64), 0, s, (const double*)partial, kl, B, chunks);
    return DAC_LAUNCH_CHECK("dac_btnk");
}

// =====================================================================================================
// [B][R][C] -> [B][C][R] through a 32 x 32 LDS tile
// =====================================================================================================
__global__ void __launch_bounds__(256) dac_transpose_kernel(const float* __restrict__ in, float* __restrict__ out, const int R, const int C) {
    __shared__ float tile[32][33];
    const int b = blockIdx.z, r0 = blockIdx.y * 32, c0 = blockIdx.x * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const float* __restrict__ ib = in + (size_t)b * R * C;
    float* __restrict__ ob = out + (size_t)b * R * C;
    for (int i = ty; i < 32; i += 8)
        if (r0 + i < R && c0 + tx < C) tile[i][tx] = ib[(size_t)(r0 + i) * C + c0 + tx];
    __syncthreads();
    for (int i = ty; i < 32; i += 8)
        if (c0 + i < C && r0 + tx < R) ob[(size_t)(c0 + i) * R + r0 + tx] = tile[tx][i];
}

const char* launch_dac_transpose(const float* in, float* out, int B, int R, int C, hipStream_t s) {
    if (!in || !out) return "dac_transpose: null operand";
    if (B < 1 || B > 65535 || R < 1 || C < 1 || ceil_div(R, 32) > 65535) return "dac_transpose: shape out of range";
    hipLaunchKernelGGL(dac_transpose_kernel, dim3((unsigned)ceil_div(C, 32), (unsigned)ceil_div(R, 32), (unsigned)B), dim3(256), 0, s, in, out, R, C);
    return DAC_LAUNCH_CHECK("dac_transpose");
}

// =====================================================================================================
// Weight norm: scale[r] = g[r] / ||v[r]|| over a row of axis 0, then w = v scale packed for its kernel
// =====================================================================================================
__global__ void __launch_bounds__(256) dac_fold_scale_kernel(const float* __restrict__ g, const float* __restrict__ v, float* __restrict__ scale, const int n) {
    __shared__ double part[256];
    const int row = blockIdx.x, tid = threadIdx.x;
    const float* __restrict__ vr = v + (size_t)row * n;
    double sum = 0.0;
    for (int i = tid; i < n; i += 256) sum += (double)vr[i] * (double)vr[i];
    part[tid] = sum;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if (tid < st) part[tid] += part[tid + st];
        __syncthreads();
    }
    if (tid == 0) scale[row] = g[row] / (float)sqrt(part[0]);
}

__global__ void __launch_bounds__(256) dac_fold_pack_kernel(const int kind, const float* __restrict__ v, const float* __restrict__ scale,
                                                            float* __restrict__ packed, const long long total, const int Cin, const int Cout,
                                                            const int taps, const int stride) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    if (kind == kDacFoldOut) {                    // [7][C] from v [1][C][7]
        const int t = (int)(idx / Cin), c = (int)(idx % Cin);
        packed[idx] = v[(size_t)c * 7 + t] * scale[0];
        return;
    }
    if (kind == kDacFoldIn) {                     // [7][C] from v [C][1][7]
        const int t = (int)(idx / Cout), c = (int)(idx % Cout);
        packed[idx] = v[(size_t)c * 7 + t] * scale[c];
        return;
    }
    if (kind == kDacFoldDown || kind == kDacFoldPlain) {      // the conv layout below over K = s Cin (down) or with N padded and scale 1 (plain)
        const int K = kind == kDacFoldDown ? stride * Cin : Cin, NBp = (Cout + 31) >> 5, nk = (K + kDacTileK - 1) / kDacTileK;
        const int ln = (int)(idx & 63);
        long long u = idx >> 6;
        const int nbp = (int)(u % NBp); u /= NBp;
        const int kp = (int)(u & 15); u >>= 4;
        const int kcp = (int)(u % nk);
        const int tp = (int)(u / nk);
        const int kx = kcp * kDacTileK + 2 * kp + (ln >> 5), nx = nbp * 32 + (ln & 31);
        float o = 0.f;
        if (kx < K && nx < Cout) {
            if (kind == kDacFoldPlain) o = v[(size_t)nx * Cin + kx];
            else {
                const int q = kx / Cin, c = kx - q * Cin;
                o = v[((size_t)nx * Cin + c) * (2 * stride) + tp * stride + q] * scale[nx];
            }
        }
        packed[idx] = o;
        return;
    }
    // [tap][K step of 32][k pair][N / 32][lane]: k = 32 step + 2 pair + (lane >> 5), n = 32 block + (lane & 31)
    const int N = kind == kDacFoldConvT ? stride * Cout : Cout, NB = N >> 5, nkc = (Cin + kDacTileK - 1) / kDacTileK;
    const int lane = (int)(idx & 63);
    long long t = idx >> 6;
    const int nb = (int)(t % NB); t /= NB;
    const int kk = (int)(t & 15); t >>= 4;
    const int kc = (int)(t % nkc);
    const int tap = (int)(t / nkc);
    const int k = kc * kDacTileK + 2 * kk + (lane >> 5), n = nb * 32 + (lane & 31);
    float val = 0.f;
    if (k < Cin) {
        if (kind == kDacFoldConv) val = v[((size_t)n * Cin + k) * taps + tap] * scale[n];
        else {
            const int phase = n / Cout, co = n - phase * Cout;
            val = v[((size_t)k * Cout + co) * (2 * stride) + phase + tap * stride] * scale[k];
        }
    }
    packed[idx] = val;
}

const char* launch_dac_fold(int kind, const float* g, const float* v, float* scale, float* packed, int Cin, int Cout, int taps, int stride, hipStream_t s) {
    if ((!g && kind != kDacFoldPlain) || !v || !scale || !packed) return "dac_fold: null operand";
    if (kind < kDacFoldConv || kind > kDacFoldPlain) return "dac_fold: unknown kind";
    if (Cin < 1 || Cout < 1 || taps < 1) return "dac_fold: bad shape";
    int rows, n;
    long long total;
    if (kind == kDacFoldOut) { rows = 1; n = Cin * 7; total = (long long)7 * Cin; }
    else if (kind == kDacFoldIn) { if (Cin != 1) return "dac_fold: the input conv has one input channel"; rows = Cout; n = 7; total = (long long)7 * Cout; }
    else if (kind == kDacFoldDown) {
        if (Cout % 32 || Cin % 32 || stride < 2) return "dac_fold: down conv needs Cin and Cout multiples of 32, stride >= 2";
        rows = Cout; n = Cin * 2 * stride; total = dac_packed_floats(stride * Cin, Cout, 2, 0);
    }
    else if (kind == kDacFoldPlain) { rows = 0; n = 0; total = dac_packed_floats(Cin, Cout, 1, 0); }
    else if (kind == kDacFoldConv) { if (Cout % 32) return "dac_fold: Cout a multiple of 32"; rows = Cout; n = Cin * taps; total = dac_packed_floats(Cin, Cout, taps, 0); }
    else {
        if (Cout % 32 || stride < 1) return "dac_fold: Cout a multiple of 32, stride >= 1";
        rows = Cin; n = Cout * 2 * stride; total = dac_packed_floats(Cin, Cout, 2, stride);
    }
    if (rows) {
        hipLaunchKernelGGL(dac_fold_scale_kernel, dim3((unsigned)rows), dim3(256), 0, s, g, v, scale, n);
        if (hipGetLastError() != hipSuccess) return "dac_fold: launch failed";
    }
    const long long blocks = (total + 255) / 256;
    if (blocks > 0x7fffffffLL) return "dac_fold: weight too large";
    hipLaunchKernelGGL(dac_fold_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, s, kind, v, scale, packed, total, Cin, Cout, taps, stride);
    return DAC_LAUNCH_CHECK("dac_fold");
}

}  // namespace adf
