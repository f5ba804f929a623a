// Kernels of the Imagen-style 2-D U-Net UNet2dBase that the ADM net's launchers do not cover (declarations and contracts: adf_unet2d.h).
// Exact fp32 throughout; every store is a vector store.
#include "adf_unet2d.h"

#include <cmath>

namespace adf {

#define U2D_LAUNCH_CHECK(name) (hipGetLastError() == hipSuccess ? nullptr : "launch failed: " name)

__device__ __forceinline__ float silu_exact(float v) { return v / (1.0f + expf(-v)); }

// ------------------------------------------------------------------------------------------------ time conditioning
__global__ void __launch_bounds__(256) u2d_time_embed_kernel(const float* __restrict__ t, int t_stride, const float* __restrict__ fourier, int half,
                                                             const float* __restrict__ w1, const float* __restrict__ b1, const float* __restrict__ w2,
                                                             const float* __restrict__ b2, int tcd, float* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* const feat = (float*)smem;              // [2 half + 1]: t | sin | cos
    float* const hid = feat + 2 * half + 1;        // [tcd]
    const int b = blockIdx.x, nf = 2 * half + 1;
    const float tv = t[(size_t)b * t_stride];
    for (int i = threadIdx.x; i < nf; i += 256) {
        float v = tv;
        if (i > 0) {
            const int k = i <= half ? i - 1 : i - 1 - half;
            const float ang = tv * fourier[k] * 2.0f * 3.14159265358979323846f;
            v = i <= half ? sinf(ang) : cosf(ang);
        }
        feat[i] = v;
    }
    __syncthreads();
    for (int j = threadIdx.x; j < tcd; j += 256) {
        float acc = b1[j];
        for (int i = 0; i < nf; ++i) acc = fmaf(w1[(size_t)j * nf + i], feat[i], acc);
        hid[j] = silu_exact(acc);
    }
    __syncthreads();
    for (int j = threadIdx.x; j < tcd; j += 256) {
        float acc = b2[j];
        for (int i = 0; i < tcd; ++i) acc = fmaf(w2[(size_t)j * tcd + i], hid[i], acc);
        out[(size_t)b * tcd + j] = acc;
    }
}
const char* launch_u2d_time_embed(const float* t, int t_stride, int nb, const float* fourier, int half, const float* w1, const float* b1,
                                  const float* w2, const float* b2, int tcd, float* out, hipStream_t s) {
    const size_t lds = (size_t)(2 * half + 1 + tcd) * 4;
    if (half < 1 || tcd < 1 || lds > 64 * 1024) return "u2d_time_embed: unsupported widths";
    hipLaunchKernelGGL(u2d_time_embed_kernel, dim3(nb), dim3(256), lds, s, t, t_stride, fourier, half, w1, b1, w2, b2, tcd, out);
    return U2D_LAUNCH_CHECK("u2d_time_embed");
}

// ------------------------------------------------------------------------------------------------ block reduction helper
// Sums v[0..N) over the 256 threads of the workgroup; the result is valid in thread 0.  red: N * 4 floats of LDS.
template <int N>
__device__ __forceinline__ void block_sum256(float (&v)[N], float* red) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int i = 0; i < N; ++i) v[i] = wave_sum(v[i]);
    if (lane == 0)
#pragma unroll
        for (int i = 0; i < N; ++i) red[wave * N + i] = v[i];
    __syncthreads();
    if (threadIdx.x == 0)
#pragma unroll
        for (int i = 0; i < N; ++i) v[i] = red[i] + red[N + i] + red[2 * N + i] + red[3 * N + i];
}

// ------------------------------------------------------------------------------------------------ CrossEmbedLayer
// Workgroup = 256 consecutive pixels of one sample x 4 consecutive output channels (inside one kernel size's slice): the weights are uniform
// over the workgroup, the input reads run along image rows.  The 4 channels' sums over the workgroup's pixels go to the fine statistics.
__global__ void __launch_bounds__(256) u2d_cross_embed_kernel(const U2dCrossEmbedArgs a) {
    __shared__ float red[8 * 4];
    const int HW = a.H * a.W, b = blockIdx.z, co0 = blockIdx.y * 4;
    const int p = blockIdx.x * 256 + threadIdx.x;
    int si = 0;
    while (si + 1 < a.n && co0 >= a.off[si + 1]) ++si;
    const int k = a.ks[si], pad = (k - 1) / 2, cout = a.off[a.n];
    const float* const w = a.w[si] + (size_t)(co0 - a.off[si]) * a.cin * k * k;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    const bool live = p < HW;
    if (live) {
        const int y = p / a.W, x = p - y * a.W;
        for (int ci = 0; ci < a.cin; ++ci) {
            const float* const xp = a.x + ((size_t)b * a.cin + ci) * HW;
            for (int dy = 0; dy < k; ++dy) {
                const int iy = y + dy - pad;
                if (iy < 0 || iy >= a.H) continue;
                for (int dx = 0; dx < k; ++dx) {
                    const int ix = x + dx - pad;
                    if (ix < 0 || ix >= a.W) continue;
                    const float v = xp[iy * a.W + ix];
                    const size_t wi = ((size_t)ci * k + dy) * k + dx;
#pragma unroll
                    for (int j = 0; j < 4; ++j) acc[j] = fmaf(w[(size_t)j * a.cin * k * k + wi], v, acc[j]);
                }
            }
        }
    }
    // conv(c_in x) = c_in conv(x): the scaling applied once to the sums (CrossEmbedLayer has no norm in front)
    const float cin_s = a.coef ? a.coef[(size_t)b * a.coef_bstride] : 1.0f;
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = fmaf(acc[j], cin_s, a.bias[si][co0 - a.off[si] + j]);
    if (live) *(f32x4_hw_t*)(a.out + ((size_t)b * HW + p) * cout + co0) = f32x4_hw_t{o[0], o[1], o[2], o[3]};
    if (!a.stats) return;
    float st[8];
#pragma unroll
    for (int j = 0; j < 4; ++j) { st[j] = live ? o[j] : 0.f; st[4 + j] = live ? o[j] * o[j] : 0.f; }
    block_sum256<8>(st, red);
    if (threadIdx.x == 0) {
        for (int j0 = 0; j0 < 4; j0 += a.fg) {
            double s1 = 0.0, s2 = 0.0;
            for (int j = j0; j < j0 + a.fg; ++j) { s1 += (double)st[j]; s2 += (double)st[4 + j]; }
            double* const d = a.stats + ((size_t)b * (cout / a.fg) + (co0 + j0) / a.fg) * 2;
            atomicAdd(d, s1);
            atomicAdd(d + 1, s2);
        }
    }
}
const char* launch_u2d_cross_embed(const U2dCrossEmbedArgs& a, hipStream_t s) {
    if (a.n < 1 || a.n > 4 || a.cin < 1 || a.B < 1 || a.H < 1 || a.W < 1) return "u2d_cross_embed: bad arguments";
    for (int i = 0; i < a.n; ++i)
        if (a.ks[i] < 1 || !(a.ks[i] & 1) || a.off[i + 1] <= a.off[i] || (a.off[i + 1] - a.off[i]) % 4) return "u2d_cross_embed: kernel sizes must be odd, slices multiples of 4 channels";
    if (a.stats && (a.fg < 1 || 4 % a.fg)) return "u2d_cross_embed: the fine statistics group must divide 4";
    const long long HW = (long long)a.H * a.W;
    if (HW >= (1ll << 31) / 256) return "u2d_cross_embed: image too large";
    const dim3 grid((unsigned)((HW + 255) / 256), (unsigned)(a.off[a.n] / 4), (unsigned)a.B);
    hipLaunchKernelGGL(u2d_cross_embed_kernel, grid, dim3(256), 0, s, a);
    return U2D_LAUNCH_CHECK("u2d_cross_embed");
}

// ------------------------------------------------------------------------------------------------ direct conv (small images)
// One thread per (output pixel, output channel), output channels fastest.  Packed fp32 weight: [cin / 32][tap][n_pad][32].
__global__ void __launch_bounds__(256) u2d_conv_small_kernel(const Conv2dArgs a) {
    const int HW = a.H * a.W;
    const long long total = (long long)a.B * HW * a.cout;
    const int Hin = a.mode == 2 ? 2 * a.H : a.H, Win = a.mode == 2 ? 2 * a.W : a.W;
    const int c1 = a.cin - a.c0;
    const float* const x0 = (const float*)a.x;
    const float* const x1 = (const float*)a.x1;
    const float* const wp = (const float*)a.w;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int n = (int)(i % a.cout);
        const long long m = i / a.cout;
        const int b = (int)(m / HW), pix = (int)(m - (long long)b * HW);
        const int oy = pix / a.W, ox = pix - oy * a.W;
        float acc = 0.f;
        for (int t = 0; t < a.taps; ++t) {
            const int dy = a.taps == 9 ? t / 3 - 1 : 0, dx = a.taps == 9 ? t % 3 - 1 : 0;
            const int iy = (a.mode == 2 ? 2 * oy : oy) + dy, ix = (a.mode == 2 ? 2 * ox : ox) + dx;
            if (iy < 0 || iy >= Hin || ix < 0 || ix >= Win) continue;         // zero padding after the prologue
            const size_t ip = (size_t)b * Hin * Win + (size_t)iy * Win + ix;
            for (int ci = 0; ci < a.cin; ++ci) {
                float v = ci < a.c0 ? x0[ip * a.c0 + ci] : x1[ip * c1 + (ci - a.c0)];
                if (a.ab) {
                    const float* const abp = a.ab + ((size_t)b * a.cin + ci) * 2;
                    v = fmaf(v, abp[0], abp[1]);
                    if (a.act) v = silu_exact(v);
                }
                acc = fmaf(wp[(((size_t)(ci >> 5) * a.taps + t) * a.n_pad + n) * 32 + (ci & 31)], v, acc);
            }
        }
        float bias = a.bias ? a.bias[n] : 0.f;
        if (a.bias_b) bias += a.bias_b[(size_t)b * a.bias_bstride + n];
        float o = acc + bias;
        if (a.res) o += ((const float*)a.res)[m * a.cout + n];
        ((float*)a.out)[m * a.cout + n] = o;
    }
}
const char* launch_u2d_conv_small(const Conv2dArgs& a, hipStream_t s) {
    if (a.taps != 9 && a.taps != 1) return "u2d_conv_small: taps must be 9 or 1";
    if (a.mode != 0 && a.mode != 2) return "u2d_conv_small: modes 0 and 2 only";
    if (a.taps == 1 && a.mode != 0) return "u2d_conv_small: a 1x1 conv has no resampling mode";
    if (a.cin % 32 || a.c0 < 1 || a.c0 > a.cin || (a.c0 < a.cin) != (a.x1 != nullptr) || a.nchunk * 32 != a.cin) return "u2d_conv_small: bad input channels";
    if (a.stats) return "u2d_conv_small: statistics are reduced by a separate pass";
    const long long total = (long long)a.B * a.H * a.W * a.cout;
    const unsigned grid = (unsigned)((total + 255) / 256 > 16384 ? 16384 : (total + 255) / 256);
    hipLaunchKernelGGL(u2d_conv_small_kernel, dim3(grid), dim3(256), 0, s, a);
    return U2D_LAUNCH_CHECK("u2d_conv_small");
}

// ------------------------------------------------------------------------------------------------ GroupNorm table, scaled second source
__global__ void __launch_bounds__(256) u2d_gn_finalize_scaled_kernel(const GnFineArgs a, float scale1) {
    const int b = blockIdx.x, ctot = a.c0 + a.c1, gs = ctot / a.G;
    const double s1 = (double)scale1;
    for (int c = threadIdx.x; c < ctot; c += 256) {
        const int g = c / gs;
        double sum = 0.0, sq = 0.0;
        for (int k = g * gs / a.fg; k < (g + 1) * gs / a.fg; ++k) {
            if (k * a.fg < a.c0) {
                const double* st = a.stats0 + ((size_t)b * (a.c0 / a.fg) + k) * 2;
                sum += st[0]; sq += st[1];
            } else {
                const double* st = a.stats1 + ((size_t)b * (a.c1 / a.fg) + (k - a.c0 / a.fg)) * 2;
                sum += s1 * st[0]; sq += s1 * s1 * st[1];
            }
        }
        const double cnt = (double)a.L * (double)gs;
        const double mean = sum / cnt;
        double var = sq / cnt - mean * mean;
        var = var > 0.0 ? var : 0.0;
        const float rstd = (float)(1.0 / sqrt(var + (double)a.eps));
        float A = rstd * a.gamma[c];
        float Bc = a.beta[c] - (float)mean * A;
        if (a.film) {
            const float fs = a.film[(size_t)b * a.film_bstride + c] + 1.0f, fh = a.film[(size_t)b * a.film_bstride + ctot + c];
            A *= fs;
            Bc = fmaf(Bc, fs, fh);
        }
        if (c >= a.c0) A *= scale1;                 // the table multiplies the unscaled skip
        *(float2*)(a.ab + ((size_t)b * ctot + c) * 2) = make_float2(A, Bc);
    }
}
const char* launch_u2d_gn_finalize_scaled(const GnFineArgs& a, float scale1, hipStream_t s) {
    const int ctot = a.c0 + a.c1;
    if (a.fg < 1 || a.G < 1 || ctot % a.G || (ctot / a.G) % a.fg || a.c0 % a.fg || a.c1 % a.fg) return "u2d_gn_finalize_scaled: group size and source widths must be multiples of the fine group";
    hipLaunchKernelGGL(u2d_gn_finalize_scaled_kernel, dim3(a.B), dim3(256), 0, s, a, scale1);
    return U2D_LAUNCH_CHECK("u2d_gn_finalize_scaled");
}

// ------------------------------------------------------------------------------------------------ GlobalContext
// A wave walks rows; each lane holds up to 4 16-byte pieces of the row (C <= 1024).  Online softmax per wave, the four waves merged in LDS.
constexpr int kGcaRowsPerChunk = 512;
int u2d_gca_chunks(int L) { return (L + kGcaRowsPerChunk - 1) / kGcaRowsPerChunk; }

__global__ void __launch_bounds__(256) u2d_gca_pool_kernel(const float* __restrict__ h, const float* __restrict__ wk, const float* __restrict__ bk,
                                                           int L, int C, float* __restrict__ part) {
    __shared__ float wm[4], wl[4];
    __shared__ __attribute__((aligned(16))) float wacc[4][1024];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int b = blockIdx.y, chunk = blockIdx.x, nch = gridDim.x;
    const int cpr = C / 4;
    const int r0 = chunk * kGcaRowsPerChunk, r1 = r0 + kGcaRowsPerChunk < L ? r0 + kGcaRowsPerChunk : L;
    f32x4_hw_t kw[4], acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int cc = lane + 64 * i;
        kw[i] = cc < cpr ? *(const f32x4_hw_t*)(wk + cc * 4) : f32x4_hw_t{0.f, 0.f, 0.f, 0.f};
        acc[i] = f32x4_hw_t{0.f, 0.f, 0.f, 0.f};
    }
    const float kb = bk[0];
    float m = -INFINITY, l = 0.f;
    for (int r = r0 + wave; r < r1; r += 4) {
        const float* const row = h + ((size_t)b * L + r) * C;
        f32x4_hw_t v[4];
        float d = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int cc = lane + 64 * i;
            v[i] = cc < cpr ? *(const f32x4_hw_t*)(row + cc * 4) : f32x4_hw_t{0.f, 0.f, 0.f, 0.f};
            d = fmaf(v[i].x, kw[i].x, d); d = fmaf(v[i].y, kw[i].y, d); d = fmaf(v[i].z, kw[i].z, d); d = fmaf(v[i].w, kw[i].w, d);
        }
        const float logit = wave_sum(d) + kb;
        const float mn = fmaxf(m, logit);
        const float alpha = expf(m - mn), pw = expf(logit - mn);
        l = fmaf(l, alpha, pw);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i] = acc[i] * alpha + v[i] * pw;
        m = mn;
    }
    if (lane == 0) { wm[wave] = m; wl[wave] = l; }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int cc = lane + 64 * i;
        if (cc < cpr) *(f32x4_hw_t*)(&wacc[wave][cc * 4]) = acc[i];
    }
    __syncthreads();
    const float M = fmaxf(fmaxf(wm[0], wm[1]), fmaxf(wm[2], wm[3]));
    float sc[4];
#pragma unroll
    for (int w = 0; w < 4; ++w) sc[w] = wm[w] == -INFINITY ? 0.f : expf(wm[w] - M);      // (a wave without rows)
    float* const o = part + ((size_t)b * nch + chunk) * (C + 2);
    if (threadIdx.x == 0) *(float2*)o = make_float2(M, wl[0] * sc[0] + wl[1] * sc[1] + wl[2] * sc[2] + wl[3] * sc[3]);
    for (int c = threadIdx.x; c < C; c += 256) o[2 + c] = wacc[0][c] * sc[0] + wacc[1][c] * sc[1] + wacc[2][c] * sc[2] + wacc[3][c] * sc[3];
}
const char* launch_u2d_gca_pool(const float* h, const float* wk, const float* bk, int B, int L, int C, float* part, hipStream_t s) {
    if (C < 4 || C % 4 || C > 1024 || L < 1) return "u2d_gca_pool: C must be a multiple of 4, at most 1024";
    hipLaunchKernelGGL(u2d_gca_pool_kernel, dim3((unsigned)u2d_gca_chunks(L), (unsigned)B), dim3(256), 0, s, h, wk, bk, L, C, part);
    return U2D_LAUNCH_CHECK("u2d_gca_pool");
}

__global__ void __launch_bounds__(256) u2d_gca_gate_kernel(const float* __restrict__ part, int nch, int C, int hid, const float* __restrict__ w0,
                                                           const float* __restrict__ b0, const float* __restrict__ w2, const float* __restrict__ b2,
                                                           float* __restrict__ gate) {
    __shared__ float pooled[1024], hd[1024];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float* const pb = part + (size_t)b * nch * (C + 2);
    float M = -INFINITY;
    for (int k = 0; k < nch; ++k) M = fmaxf(M, pb[(size_t)k * (C + 2)]);
    float lsum = 0.f;
    for (int k = 0; k < nch; ++k) lsum += pb[(size_t)k * (C + 2) + 1] * expf(pb[(size_t)k * (C + 2)] - M);
    for (int c = threadIdx.x; c < C; c += 256) {
        float a = 0.f;
        for (int k = 0; k < nch; ++k) a = fmaf(pb[(size_t)k * (C + 2) + 2 + c], expf(pb[(size_t)k * (C + 2)] - M), a);
        pooled[c] = a / lsum;
    }
    __syncthreads();
    for (int j = wave; j < hid; j += 4) {             // net.0 (1x1 conv C -> hid) + SiLU: one wave per output
        float a = 0.f;
        for (int c = lane; c < C; c += 64) a = fmaf(w0[(size_t)j * C + c], pooled[c], a);
        a = wave_sum(a) + b0[j];
        if (lane == 0) hd[j] = silu_exact(a);
    }
    __syncthreads();
    for (int c = wave; c < C; c += 4) {               // net.2 (1x1 conv hid -> C) + sigmoid
        float a = 0.f;
        for (int j = lane; j < hid; j += 64) a = fmaf(w2[(size_t)c * hid + j], hd[j], a);
        a = wave_sum(a) + b2[c];
        if (lane == 0) gate[(size_t)b * C + c] = 1.0f / (1.0f + expf(-a));
    }
}
const char* launch_u2d_gca_gate(const float* part, int B, int L, int C, int hid, const float* w0, const float* b0, const float* w2,
                                const float* b2, float* gate, hipStream_t s) {
    if (C < 1 || C > 1024 || hid < 1 || hid > 1024) return "u2d_gca_gate: widths above 1024";
    hipLaunchKernelGGL(u2d_gca_gate_kernel, dim3((unsigned)B), dim3(256), 0, s, part, u2d_gca_chunks(L), C, hid, w0, b0, w2, b2, gate);
    return U2D_LAUNCH_CHECK("u2d_gca_gate");
}

// A thread keeps one 16-byte piece of the row (the same channels for every row it visits) and strides over rows; the statistics of the
// workgroup's rows are summed per channel in LDS, then per fine group into the fp64 buffer.
constexpr int kGateRows = 256;
__global__ void __launch_bounds__(256) u2d_gate_residual_kernel(const float* __restrict__ h, const float* __restrict__ gate, const float* __restrict__ res,
                                                                float* __restrict__ out, int L, int C, double* __restrict__ stats, int fg) {
    __shared__ float s1[1024], s2[1024];
    const int b = blockIdx.y, cpr = C / 4;
    const int step = 256 / cpr, cc = threadIdx.x % cpr, lr = threadIdx.x / cpr;
    const int r0 = blockIdx.x * kGateRows, r1 = r0 + kGateRows < L ? r0 + kGateRows : L;
    if (stats) {
        for (int i = threadIdx.x; i < C; i += 256) { s1[i] = 0.f; s2[i] = 0.f; }
        __syncthreads();
    }
    if (lr < step) {
        const f32x4_hw_t g = *(const f32x4_hw_t*)(gate + (size_t)b * C + cc * 4);
        f32x4_hw_t a1 = {0.f, 0.f, 0.f, 0.f}, a2 = {0.f, 0.f, 0.f, 0.f};
        for (int r = r0 + lr; r < r1; r += step) {
            const size_t o = ((size_t)b * L + r) * C + cc * 4;
            const f32x4_hw_t v = *(const f32x4_hw_t*)(h + o), rv = *(const f32x4_hw_t*)(res + o);
            f32x4_hw_t y;
            y.x = fmaf(v.x, g.x, rv.x); y.y = fmaf(v.y, g.y, rv.y); y.z = fmaf(v.z, g.z, rv.z); y.w = fmaf(v.w, g.w, rv.w);
            *(f32x4_hw_t*)(out + o) = y;
            a1 += y;
            a2 += y * y;
        }
        if (stats) {
            atomicAdd(&s1[cc * 4], a1.x); atomicAdd(&s1[cc * 4 + 1], a1.y); atomicAdd(&s1[cc * 4 + 2], a1.z); atomicAdd(&s1[cc * 4 + 3], a1.w);
            atomicAdd(&s2[cc * 4], a2.x); atomicAdd(&s2[cc * 4 + 1], a2.y); atomicAdd(&s2[cc * 4 + 2], a2.z); atomicAdd(&s2[cc * 4 + 3], a2.w);
        }
    }
    if (!stats) return;
    __syncthreads();
    for (int g = threadIdx.x; g < C / fg; g += 256) {
        double d1 = 0.0, d2 = 0.0;
        for (int c = g * fg; c < (g + 1) * fg; ++c) { d1 += (double)s1[c]; d2 += (double)s2[c]; }
        atomicAdd(&stats[((size_t)b * (C / fg) + g) * 2], d1);
        atomicAdd(&stats[((size_t)b * (C / fg) + g) * 2 + 1], d2);
    }
}
const char* launch_u2d_gate_residual(const float* h, const float* gate, const float* res, float* out, int B, int L, int C, double* stats,
                                     int fg, hipStream_t s) {
    if (C < 4 || C % 4 || C > 1024) return "u2d_gate_residual: C must be a multiple of 4, at most 1024";
    if (stats && (fg < 1 || C % fg)) return "u2d_gate_residual: the fine group must divide C";
    const dim3 grid((unsigned)((L + kGateRows - 1) / kGateRows), (unsigned)B);
    hipLaunchKernelGGL(u2d_gate_residual_kernel, grid, dim3(256), 0, s, h, gate, res, out, L, C, stats, fg);
    return U2D_LAUNCH_CHECK("u2d_gate_residual");
}

// ------------------------------------------------------------------------------------------------ PixelShuffle + SiLU
__global__ void __launch_bounds__(256) u2d_silu_shuffle_kernel(const float* __restrict__ in, float* __restrict__ out, int H, int W, int C, long long total) {
    const int cpr = C / 4, W2 = 2 * W;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        const int cc = (int)(i % cpr);
        long long r = i / cpr;
        const int ox = (int)(r % W2); r /= W2;
        const int oy = (int)(r % (2 * H));
        const long long b = r / (2 * H);
        const int sub = (oy & 1) * 2 + (ox & 1);
        const float* const src = in + ((size_t)b * H * W + (size_t)(oy >> 1) * W + (ox >> 1)) * (4 * C) + cc * 16 + sub;
        *(f32x4_hw_t*)(out + i * 4) = f32x4_hw_t{silu_exact(src[0]), silu_exact(src[4]), silu_exact(src[8]), silu_exact(src[12])};
    }
}
const char* launch_u2d_silu_shuffle(const float* in, float* out, int B, int H, int W, int C, hipStream_t s) {
    if (C % 4 || C < 4) return "u2d_silu_shuffle: C must be a multiple of 4";
    const long long total = (long long)B * 4 * H * W * (C / 4);
    const unsigned grid = (unsigned)((total + 255) / 256 > 65536 ? 65536 : (total + 255) / 256);
    hipLaunchKernelGGL(u2d_silu_shuffle_kernel, dim3(grid), dim3(256), 0, s, in, out, H, W, C, total);
    return U2D_LAUNCH_CHECK("u2d_silu_shuffle");
}

// ------------------------------------------------------------------------------------------------ LayerNorm_g(GELU(x))
// One wave per row, CPL 16-byte pieces per lane (C <= 256 CPL, CPL 1, 2 or 4); two passes over the register copy (mean, then centred squares)
template <int CPL>
__global__ void __launch_bounds__(256) u2d_gelu_ln_kernel(const float* __restrict__ x, float* __restrict__ y, long long rows, int C,
                                                          const float* __restrict__ g, float eps) {
    const int lane = threadIdx.x & 63;
    const long long r = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const int cpr = C / 4;
    f32x4_hw_t f[CPL];
    float sum = 0.f;
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        const int cc = lane + 64 * k;
        f[k] = f32x4_hw_t{0.f, 0.f, 0.f, 0.f};
        if (cc < cpr) {
            const f32x4_hw_t v = *(const f32x4_hw_t*)(x + r * C + cc * 4);
            f[k] = f32x4_hw_t{gelu_erf_f(v.x), gelu_erf_f(v.y), gelu_erf_f(v.z), gelu_erf_f(v.w)};
            sum += (f[k].x + f[k].y) + (f[k].z + f[k].w);
        }
    }
    const float mean = wave_sum(sum) / (float)C;
    float sq = 0.f;
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        if (lane + 64 * k < cpr) {
            const f32x4_hw_t d = f[k] - mean;
            sq += (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w);
        }
    }
    const float rstd = rsqrtf(wave_sum(sq) / (float)C + eps);
#pragma unroll
    for (int k = 0; k < CPL; ++k) {
        const int cc = lane + 64 * k;
        if (cc < cpr) {
            const f32x4_hw_t gg = *(const f32x4_hw_t*)(g + cc * 4);
            *(f32x4_hw_t*)(y + r * C + cc * 4) = (f[k] - mean) * rstd * gg;
        }
    }
}
const char* launch_u2d_gelu_ln_rows(const float* x, float* y, long long rows, int C, const float* g, float eps, hipStream_t s) {
    if (C % 4 || C < 4) return "u2d_gelu_ln_rows: C must be a multiple of 4";
    const unsigned grid = (unsigned)((rows + 3) / 4);
    const int cpr = C / 4;
    if (cpr <= 64) hipLaunchKernelGGL(u2d_gelu_ln_kernel<1>, dim3(grid), dim3(256), 0, s, x, y, rows, C, g, eps);
    else if (cpr <= 128) hipLaunchKernelGGL(u2d_gelu_ln_kernel<2>, dim3(grid), dim3(256), 0, s, x, y, rows, C, g, eps);
    else if (cpr <= 256) hipLaunchKernelGGL(u2d_gelu_ln_kernel<4>, dim3(grid), dim3(256), 0, s, x, y, rows, C, g, eps);
    else return "u2d_gelu_ln_rows: C above 1024";
    return U2D_LAUNCH_CHECK("u2d_gelu_ln_rows");
}

// ------------------------------------------------------------------------------------------------ attention, head dim 128
// Workgroup = 64 queries of one (sample, head) pair, four lanes per query: lane sub = lane & 3 holds the head dims {16 i + 4 sub + e} (i < 8,
// e < 4) of q and of the output accumulator, so the four lanes of a query read four consecutive 16-byte pieces of a K / V row in LDS.
// A dot product is the lane's 32-term partial + two xor exchanges.  Keys go in tiles of 32 (K and V of a tile: 32 KB of LDS); the scores of a
// tile stay in registers, one online-softmax rescale per tile.
constexpr int kAttKT = 32;
__global__ void __launch_bounds__(256) u2d_attention_d128_kernel(const float* __restrict__ qkv, float* __restrict__ out, int N, int C, int heads,
                                                                 float scale) {
    constexpr int D = 128;
    __shared__ __attribute__((aligned(16))) float ks[kAttKT][D], vs[kAttKT][D];
    const int tid = threadIdx.x, sub = tid & 3;
    const int qblocks = (N + 63) / 64;
    const int pair = blockIdx.x / qblocks, qb = blockIdx.x - pair * qblocks;
    const int b = pair / heads, hd = pair - b * heads;
    const int qi = qb * 64 + (tid >> 2);
    const bool qlive = qi < N;
    const size_t rs = (size_t)3 * C;
    const float* const base = qkv + (size_t)b * N * rs + (size_t)hd * D;
    f32x4_hw_t q[8], o[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        q[i] = qlive ? *(const f32x4_hw_t*)(base + (size_t)qi * rs + 16 * i + 4 * sub) : f32x4_hw_t{0.f, 0.f, 0.f, 0.f};
        o[i] = f32x4_hw_t{0.f, 0.f, 0.f, 0.f};
    }
    float m = -INFINITY, l = 0.f;
    for (int k0 = 0; k0 < N; k0 += kAttKT) {
        __syncthreads();
        for (int i = tid; i < kAttKT * D / 4; i += 256) {          // K and V rows of the tile (zero beyond N)
            const int kr = i / (D / 4), c4 = i - kr * (D / 4);
            const bool ok = k0 + kr < N;
            const float* const row = base + (size_t)(k0 + kr) * rs + c4 * 4;
            *(f32x4_hw_t*)(&ks[kr][c4 * 4]) = ok ? *(const f32x4_hw_t*)(row + C) : f32x4_hw_t{0.f, 0.f, 0.f, 0.f};
            *(f32x4_hw_t*)(&vs[kr][c4 * 4]) = ok ? *(const f32x4_hw_t*)(row + 2 * C) : f32x4_hw_t{0.f, 0.f, 0.f, 0.f};
        }
        __syncthreads();
        const int nk = N - k0 < kAttKT ? N - k0 : kAttKT;
        float sc[kAttKT];
        float tmax = -INFINITY;
#pragma unroll
        for (int j = 0; j < kAttKT; ++j) {
            float d = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const f32x4_hw_t kv = *(const f32x4_hw_t*)(&ks[j][16 * i + 4 * sub]);
                d = fmaf(q[i].x, kv.x, d); d = fmaf(q[i].y, kv.y, d); d = fmaf(q[i].z, kv.z, d); d = fmaf(q[i].w, kv.w, d);
            }
            d += __shfl_xor(d, 1, 64);
            d += __shfl_xor(d, 2, 64);
            sc[j] = j < nk ? d * scale : -INFINITY;
            tmax = fmaxf(tmax, sc[j]);
        }
        const float mn = fmaxf(m, tmax);
        const float alpha = expf(m - mn);
        l *= alpha;
#pragma unroll
        for (int i = 0; i < 8; ++i) o[i] *= alpha;
#pragma unroll
        for (int j = 0; j < kAttKT; ++j) {
            const float p = expf(sc[j] - mn);
            l += p;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const f32x4_hw_t vv = *(const f32x4_hw_t*)(&vs[j][16 * i + 4 * sub]);
                o[i].x = fmaf(p, vv.x, o[i].x); o[i].y = fmaf(p, vv.y, o[i].y); o[i].z = fmaf(p, vv.z, o[i].z); o[i].w = fmaf(p, vv.w, o[i].w);
            }
        }
        m = mn;
    }
    if (!qlive) return;
    const float inv = 1.0f / l;
    float* const orow = out + ((size_t)b * N + qi) * C + (size_t)hd * D;
#pragma unroll
    for (int i = 0; i < 8; ++i) *(f32x4_hw_t*)(orow + 16 * i + 4 * sub) = o[i] * inv;
}
const char* launch_u2d_attention_d128(const float* qkv, float* out, int B, int N, int C, int heads, hipStream_t s) {
    if (heads < 1 || C != 128 * heads || N < 1) return "u2d_attention_d128: head dim must be 128";
    const long long blocks = (long long)B * heads * ((N + 63) / 64);
    if (blocks > 0x7fffffffll) return "u2d_attention_d128: grid too large";
    hipLaunchKernelGGL(u2d_attention_d128_kernel, dim3((unsigned)blocks), dim3(256), 0, s, qkv, out, N, C, heads, 1.0f / sqrtf(128.0f));
    return U2D_LAUNCH_CHECK("u2d_attention_d128");
}

// ------------------------------------------------------------------------------------------------ final conv, raw input
// One thread per output pixel, all CO output channels; the weights ([co][tap][cin]) in LDS are read at one address per wave (broadcast).
// mode 0: out = F;  mode 1: out = clamp(c_skip x_noisy + c_out F, -1, 1);  mode 2: the same without the clamp.
template <int CO>
__global__ void __launch_bounds__(256) u2d_conv_out_raw_kernel(const float* __restrict__ hx, const float* __restrict__ w, const float* __restrict__ bias,
                                                               float* __restrict__ out, int B, int cin, int H, int W, int mode,
                                                               const float* __restrict__ x_noisy, const float* __restrict__ coef, int coef_bstride) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* const ws = (float*)smem;                    // [CO][9][cin]
    for (int i = threadIdx.x; i < CO * cin * 9; i += 256) {
        const int t = i % 9, ci = (i / 9) % cin, co = i / (9 * cin);
        ws[(co * 9 + t) * cin + ci] = w[i];
    }
    __syncthreads();
    const int HW = H * W, b = blockIdx.y;
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= HW) return;
    const int y = p / W, x = p - y * W;
    float acc[CO];
#pragma unroll
    for (int co = 0; co < CO; ++co) acc[co] = 0.f;
    for (int t = 0; t < 9; ++t) {
        const int iy = y + t / 3 - 1, ix = x + t % 3 - 1;
        if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
        const float* const row = hx + ((size_t)b * HW + (size_t)iy * W + ix) * cin;
        for (int c4 = 0; c4 < cin / 4; ++c4) {
            const f32x4_hw_t v = *(const f32x4_hw_t*)(row + c4 * 4);
#pragma unroll
            for (int co = 0; co < CO; ++co) {
                const f32x4_hw_t wv = *(const f32x4_hw_t*)(ws + (co * 9 + t) * cin + c4 * 4);
                acc[co] = fmaf(wv.x, v.x, acc[co]); acc[co] = fmaf(wv.y, v.y, acc[co]);
                acc[co] = fmaf(wv.z, v.z, acc[co]); acc[co] = fmaf(wv.w, v.w, acc[co]);
            }
        }
    }
#pragma unroll
    for (int co = 0; co < CO; ++co) {
        const float F = acc[co] + bias[co];
        const size_t o = ((size_t)b * CO + co) * HW + p;
        if (mode == 0) out[o] = F;
        else {
            const float c_skip = coef[(size_t)b * coef_bstride + 2], c_out = coef[(size_t)b * coef_bstride + 3];
            const float v = fmaf(c_out, F, c_skip * x_noisy[o]);
            out[o] = mode == 1 ? fminf(fmaxf(v, -1.0f), 1.0f) : v;        // mode 2: the unclipped estimate (VDiffusion(for_edm=True))
        }
    }
}
const char* launch_u2d_conv_out_raw(const float* h, const float* w, const float* bias, float* out, int B, int cin, int H, int W, int cout,
                                    int mode, const float* x_noisy, const float* coef, int coef_bstride, hipStream_t s) {
    if (cin % 4 || cin < 4) return "u2d_conv_out_raw: input channels must be a multiple of 4";
    const size_t lds = (size_t)cout * 9 * cin * 4;
    if (lds > 64 * 1024) return "u2d_conv_out_raw: the weights do not fit LDS";
    const dim3 grid((unsigned)((H * W + 255) / 256), (unsigned)B);
#define U2D_OUT(CO_) hipLaunchKernelGGL((u2d_conv_out_raw_kernel<CO_>), grid, dim3(256), lds, s, h, w, bias, out, B, cin, H, W, mode, x_noisy, coef, coef_bstride)
    switch (cout) {
        case 1: U2D_OUT(1); break;
        case 2: U2D_OUT(2); break;
        case 3: U2D_OUT(3); break;
        case 4: U2D_OUT(4); break;
        default: return "u2d_conv_out_raw: 1 to 4 output channels";
    }
#undef U2D_OUT
    return U2D_LAUNCH_CHECK("u2d_conv_out_raw");
}

// ------------------------------------------------------------------------------------------------ load-time weight transforms
__global__ void __launch_bounds__(256) u2d_weight_transform_kernel(const float* __restrict__ src, float* __restrict__ dst, int mode, int cout, int cin,
                                                                   int K, int c0, float scale, long long total) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
        if (mode == 0) {                               // dst [cout][cin][9]
            const int t = (int)(i % 9);
            const long long r = i / 9;
            const int c = (int)(r % cin), n = (int)(r / cin);
            const int ty = t / 3, tx = t % 3;
            dst[i] = (ty >= 1 && tx >= 1) ? src[((size_t)n * cin + c) * 4 + (ty - 1) * 2 + (tx - 1)] : 0.f;
        } else {                                       // dst [cout][cin][K]
            const int c = (int)((i / K) % cin);
            dst[i] = c >= c0 ? src[i] * scale : src[i];
        }
    }
}
const char* launch_u2d_weight_transform(const float* src, float* dst, int mode, int cout, int cin, int K, int c0, float scale, hipStream_t s) {
    if (mode != 0 && mode != 1) return "u2d_weight_transform: bad mode";
    const long long total = (long long)cout * cin * (mode == 0 ? 9 : K);
    const unsigned grid = (unsigned)((total + 255) / 256 > 4096 ? 4096 : (total + 255) / 256);
    hipLaunchKernelGGL(u2d_weight_transform_kernel, dim3(grid), dim3(256), 0, s, src, dst, mode, cout, cin, K, c0, scale, total);
    return U2D_LAUNCH_CHECK("u2d_weight_transform");
}

}  // namespace adf
