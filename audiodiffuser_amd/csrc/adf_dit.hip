// Kernels of the adaLN-Zero diffusion transformer (adf_dit.h), exact fp32.
#include "adf_dit.h"

#define DIT_LAUNCH_CHECK(name) (hipGetLastError() == hipSuccess ? nullptr : name ": launch failed")

namespace adf {

typedef float dit_f32x16_t __attribute__((ext_vector_type(16)));
typedef float dit_f32x4_t __attribute__((ext_vector_type(4)));

// =====================================================================================================
// Token linear: Y = epi(X W^T + b) on v_mfma_f32_32x32x2_f32
// =====================================================================================================
// A workgroup of four waves owns a 128 x 128 tile of Y; wave (wm, wn) owns 64 x 64 of it as 2 x 2 MFMA tiles.  Both operands are K-contiguous in
// memory, so X and W tiles are staged the same way: 128 rows x 16 floats, two 16-byte loads per thread, into LDS rows of kPitch = 20 floats (16
// consecutive rows then start in 16 different groups of four banks, so the 16-byte fragment reads below do not collide).  The tile of step k + 1 is
// loaded into registers before the MFMAs of step k and stored into the other LDS buffer after them: one barrier per step.
// An MFMA takes k = {lane >> 5} of its two-k slab; a lane reads four consecutive floats of its row (k = 4 (lane >> 5) + j of an 8-float chunk), so
// MFMA j of a chunk multiplies k = j (lower half-wave) and k = 4 + j (upper) -- the same pairing on both operands, i.e. a permutation of the k order.
constexpr int kDitPitch = 20;

__global__ void __launch_bounds__(256) dit_linear_kernel(const DitLinearArgs a) {
    __shared__ __attribute__((aligned(16))) float sA[2][kDitTileM * kDitPitch];
    __shared__ __attribute__((aligned(16))) float sB[2][kDitTileN * kDitPitch];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, kh = lane >> 5;
    const int m0 = blockIdx.y * kDitTileM, n0 = blockIdx.x * kDitTileN;
    const int K = a.K;
    // staging: float4 index tid + 256 i of the tile -> row (idx >> 2), floats 4 (idx & 3) ..; rows past M re-read row M - 1 (never stored)
    const float* ga[2];
    const float* gb[2];
    int so[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int idx = tid + 256 * i, row = idx >> 2, c4 = (idx & 3) * 4;
        const int mr = m0 + row < a.M ? m0 + row : a.M - 1;
        ga[i] = a.x + (size_t)mr * K + c4;
        gb[i] = a.w + (size_t)(n0 + row) * K + c4;          // the weight is padded to whole tiles
        so[i] = row * kDitPitch + c4;
    }
    dit_f32x16_t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][t][e] = 0.f;
    dit_f32x4_t ra[2], rb[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) { ra[i] = *(const dit_f32x4_t*)ga[i]; rb[i] = *(const dit_f32x4_t*)gb[i]; }
#pragma unroll
    for (int i = 0; i < 2; ++i) { *(dit_f32x4_t*)(&sA[0][so[i]]) = ra[i]; *(dit_f32x4_t*)(&sB[0][so[i]]) = rb[i]; }
    __syncthreads();
    const int nk = K / kDitTileK;
    const int fa = (wm * 64 + l31) * kDitPitch + kh * 4, fb = (wn * 64 + l31) * kDitPitch + kh * 4;
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        const bool more = kt + 1 < nk;
        if (more) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                ra[i] = *(const dit_f32x4_t*)(ga[i] + (size_t)(kt + 1) * kDitTileK);
                rb[i] = *(const dit_f32x4_t*)(gb[i] + (size_t)(kt + 1) * kDitTileK);
            }
        }
#pragma unroll
        for (int kc = 0; kc < 2; ++kc) {
            dit_f32x4_t va[2], vb[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                va[i] = *(const dit_f32x4_t*)(&sA[cur][fa + i * 32 * kDitPitch + kc * 8]);
                vb[i] = *(const dit_f32x4_t*)(&sB[cur][fb + i * 32 * kDitPitch + kc * 8]);
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int t = 0; t < 2; ++t) acc[i][t] = __builtin_amdgcn_mfma_f32_32x32x2f32(va[i][j], vb[t][j], acc[i][t], 0, 0, 0);
        }
        if (more) {
#pragma unroll
            for (int i = 0; i < 2; ++i) { *(dit_f32x4_t*)(&sA[cur ^ 1][so[i]]) = ra[i]; *(dit_f32x4_t*)(&sB[cur ^ 1][so[i]]) = rb[i]; }
        }
        __syncthreads();
    }
    // C/D map of the 32 x 32 MFMA: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int t = 0; t < 2; ++t) {
        const int col = n0 + wn * 64 + t * 32 + l31;
        if (col >= a.N) continue;
        const float bv = a.bias ? a.bias[col] : 0.f;
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = m0 + wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                if (row >= a.M) continue;
                float v = acc[i][t][r] + bv;
                const size_t o = (size_t)row * a.N + col;
                if (a.epi == kDitEpiGelu) {
                    // nn.GELU(approximate="tanh"): 0.5 v (1 + tanh(sqrt(2 / pi) (v + 0.044715 v^3)))
                    const float u = 0.7978845608028654f * (v + 0.044715f * v * v * v);
                    v = 0.5f * v * (1.0f + tanhf(u));
                } else if (a.epi == kDitEpiGate) {
                    const int b = row / a.T;
                    if (a.pre) a.pre[o] = v;
                    v = a.res[o] + a.gate[(size_t)b * a.gate_bstride + col] * v;
                }
                a.y[o] = v;
            }
        }
    }
}

const char* launch_dit_linear(const DitLinearArgs& a, hipStream_t s) {
    if (!a.x || !a.w || !a.y) return "dit_linear: null operand";
    if (a.M < 1 || a.N < 1 || a.K < kDitTileK || a.K % kDitTileK) return "dit_linear: M, N >= 1 and K a positive multiple of 16";
    if (a.epi != kDitEpiBias && a.epi != kDitEpiGelu && a.epi != kDitEpiGate) return "dit_linear: unknown epilogue";
    if (a.epi == kDitEpiGate && (!a.res || !a.gate || a.T < 1)) return "dit_linear: the gated epilogue needs res, gate and T";
    if (((uintptr_t)a.x | (uintptr_t)a.w) & 15) return "dit_linear: operands must be 16-byte aligned";
    const long long mt = ((long long)a.M + kDitTileM - 1) / kDitTileM;
    if (mt > 65535) return "dit_linear: too many rows";
    hipLaunchKernelGGL(dit_linear_kernel, dim3(ceil_div(a.N, kDitTileN), (unsigned)mt), dim3(256), 0, s, a);
    return DIT_LAUNCH_CHECK("dit_linear");
}

// =====================================================================================================
// LayerNorm + modulate: one wave per row, the row in registers (D <= 1024: at most four 16-byte chunks per lane)
// =====================================================================================================
__global__ void __launch_bounds__(256) dit_ln_modulate_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ shift,
                                                              const float* __restrict__ scale, int mod_bstride, int rows, int T, int D) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int nch = D >> 2;
    const float* xr = x + (size_t)row * D;
    dit_f32x4_t v[4];
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = lane + 64 * i;
        v[i] = c < nch ? *(const dit_f32x4_t*)(xr + 4 * c) : dit_f32x4_t{0.f, 0.f, 0.f, 0.f};
        sum += (v[i].x + v[i].y) + (v[i].z + v[i].w);
    }
    const float mean = wave_sum(sum) / (float)D;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        if (lane + 64 * i < nch) {
            const dit_f32x4_t d = v[i] - mean;
            sq += (d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w);
        }
    }
    const float rstd = 1.0f / sqrtf(wave_sum(sq) / (float)D + 1e-6f);
    const size_t mo = (size_t)(row / T) * mod_bstride;
    float* yr = y + (size_t)row * D;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = lane + 64 * i;
        if (c < nch) {
            const dit_f32x4_t sc = *(const dit_f32x4_t*)(scale + mo + 4 * c), sh = *(const dit_f32x4_t*)(shift + mo + 4 * c);
            *(dit_f32x4_t*)(yr + 4 * c) = (v[i] - mean) * rstd * (1.0f + sc) + sh;
        }
    }
}

const char* launch_dit_ln_modulate(const float* x, float* y, const float* shift, const float* scale, int mod_bstride, int rows, int T, int D,
                                   hipStream_t s) {
    if (!x || !y || !shift || !scale) return "dit_ln_modulate: null operand";
    if (rows < 1 || T < 1 || D < 4 || D % 4 || D > 1024 || mod_bstride % 4) return "dit_ln_modulate: D must be a multiple of 4, at most 1024";
    if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)shift | (uintptr_t)scale) & 15) return "dit_ln_modulate: operands must be 16-byte aligned";
    hipLaunchKernelGGL(dit_ln_modulate_kernel, dim3(ceil_div(rows, 4)), dim3(256), 0, s, x, y, shift, scale, mod_bstride, rows, T, D);
    return DIT_LAUNCH_CHECK("dit_ln_modulate");
}

// =====================================================================================================
// PatchEmbed (dit.py:96-120) + pos_embed (:403): eight tokens per workgroup, their patches in LDS, one output channel per thread
// =====================================================================================================
constexpr int kDitPatchTokens = 8;

__global__ void __launch_bounds__(256) dit_patch_embed_kernel(const float* __restrict__ x, const float* __restrict__ coef, int coef_bstride,
                                                              const float* __restrict__ w, const float* __restrict__ bias,
                                                              const float* __restrict__ pos, float* __restrict__ out, int B, int C, int H, int W,
                                                              int p1, int p2, int D) {
    __shared__ float patch[kDitPatchTokens][256];
    const int gw = W / p2, T = (H / p1) * gw, K = C * p1 * p2;
    const long long tok0 = (long long)blockIdx.x * kDitPatchTokens, ntok = (long long)B * T;
    for (int idx = threadIdx.x; idx < kDitPatchTokens * K; idx += 256) {
        const int j = idx / K, k = idx - j * K;
        const long long tg = tok0 + j;
        float v = 0.f;
        if (tg < ntok) {
            const int b = (int)(tg / T), t = (int)(tg - (long long)b * T);
            const int c = k / (p1 * p2), p = (k / p2) % p1, q = k % p2;
            const int yy = (t / gw) * p1 + p, xx = (t % gw) * p2 + q;
            v = x[(((size_t)b * C + c) * H + yy) * W + xx];
            if (coef) v *= coef[(size_t)b * coef_bstride];            // c_in x, rounded as the reference's tensor product is (diffusion.py:50)
        }
        patch[j][k] = v;
    }
    __syncthreads();
    for (int d = threadIdx.x; d < D; d += 256) {
        float acc[kDitPatchTokens];
#pragma unroll
        for (int j = 0; j < kDitPatchTokens; ++j) acc[j] = 0.f;
        const float* wr = w + (size_t)d * K;
        for (int k = 0; k < K; ++k) {
            const float wv = wr[k];
#pragma unroll
            for (int j = 0; j < kDitPatchTokens; ++j) acc[j] = fmaf(wv, patch[j][k], acc[j]);
        }
        const float bv = bias[d];
#pragma unroll
        for (int j = 0; j < kDitPatchTokens; ++j) {
            const long long tg = tok0 + j;
            if (tg < ntok) out[(size_t)tg * D + d] = (acc[j] + bv) + pos[(size_t)(tg % T) * D + d];
        }
    }
}

const char* launch_dit_patch_embed(const float* x, const float* coef, int coef_bstride, const float* w, const float* bias, const float* pos, float* out,
                                   int B, int C, int H, int W, int p1, int p2, int D, hipStream_t s) {
    if (!x || !w || !bias || !pos || !out) return "dit_patch_embed: null operand";
    if (B < 1 || C < 1 || p1 < 1 || p2 < 1 || H < p1 || W < p2 || H % p1 || W % p2 || D < 1) return "dit_patch_embed: bad shape";
    if ((long long)C * p1 * p2 > 256) return "dit_patch_embed: a patch holds at most 256 values";
    const long long ntok = (long long)B * (H / p1) * (W / p2);
    const long long blocks = (ntok + kDitPatchTokens - 1) / kDitPatchTokens;
    if (blocks > 0x7fffffffLL) return "dit_patch_embed: too many tokens";
    hipLaunchKernelGGL(dit_patch_embed_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, coef, coef_bstride, w, bias, pos, out, B, C, H, W, p1, p2, D);
    return DIT_LAUNCH_CHECK("dit_patch_embed");
}

// =====================================================================================================
// unpatchify (dit.py:366-380) with the denoiser epilogue (diffusion.py:57-61): one thread per output element
// =====================================================================================================
__global__ void __launch_bounds__(256) dit_unpatchify_kernel(const float* __restrict__ lin, float* __restrict__ out, int C, int H, int W, int p1, int p2,
                                                             int mode, const float* __restrict__ x_noisy, const float* __restrict__ coef,
                                                             int coef_bstride, long long total) {
    const int gw = W / p2, T = (H / p1) * gw, N = p1 * p2 * C;
    for (long long o = (long long)blockIdx.x * 256 + threadIdx.x; o < total; o += (long long)gridDim.x * 256) {
        const int xx = (int)(o % W);
        long long r = o / W;
        const int yy = (int)(r % H); r /= H;
        const int c = (int)(r % C);
        const long long b = r / C;
        const int t = (yy / p1) * gw + xx / p2, n = ((yy % p1) * p2 + xx % p2) * C + c;
        const float F = lin[((size_t)b * T + t) * N + n];
        if (mode == 0) out[o] = F;
        else {
            const float c_skip = coef[(size_t)b * coef_bstride + 2], c_out = coef[(size_t)b * coef_bstride + 3];
            const float v = fmaf(c_out, F, c_skip * x_noisy[o]);
            out[o] = mode == 1 ? fminf(fmaxf(v, -1.0f), 1.0f) : v;
        }
    }
}

const char* launch_dit_unpatchify(const float* lin, float* out, int B, int C, int H, int W, int p1, int p2, int mode, const float* x_noisy,
                                  const float* coef, int coef_bstride, hipStream_t s) {
    if (!lin || !out) return "dit_unpatchify: null operand";
    if (B < 1 || C < 1 || p1 < 1 || p2 < 1 || H < p1 || W < p2 || H % p1 || W % p2) return "dit_unpatchify: bad shape";
    if (mode < 0 || mode > 2) return "dit_unpatchify: unknown epilogue mode";
    if (mode != 0 && (!x_noisy || !coef)) return "dit_unpatchify: the denoiser epilogue needs x_noisy and coef";
    const long long total = (long long)B * C * H * W;
    const unsigned grid = (unsigned)((total + 255) / 256 > 16384 ? 16384 : (total + 255) / 256);
    hipLaunchKernelGGL(dit_unpatchify_kernel, dim3(grid), dim3(256), 0, s, lin, out, C, H, W, p1, p2, mode, x_noisy, coef, coef_bstride, total);
    return DIT_LAUNCH_CHECK("dit_unpatchify");
}

// =====================================================================================================
// c = t_embedder(t) (+ y_embedder(classes)) (dit.py:404-410) and SiLU(c), what every adaLN_modulation starts with (:243-246, :266-269)
// =====================================================================================================
__global__ void __launch_bounds__(256) dit_cond_kernel(float* __restrict__ c, float* __restrict__ sc, const float* __restrict__ te, int te_bs,
                                                       const float* __restrict__ ce, int ce_bs, int D) {
    const int r = blockIdx.y;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < D; i += gridDim.x * 256) {
        float v = te[(size_t)r * te_bs + i];
        if (ce) v += ce[(size_t)r * ce_bs + i];
        c[(size_t)r * D + i] = v;
        sc[(size_t)r * D + i] = v / (1.0f + expf(-v));
    }
}

const char* launch_dit_cond(float* c, float* sc, const float* te, int te_bstride, const float* ce, int ce_bstride, int rows, int D, hipStream_t s) {
    if (!c || !sc || !te) return "dit_cond: null operand";
    if (rows < 1 || rows > 65535 || D < 1) return "dit_cond: bad shape";
    hipLaunchKernelGGL(dit_cond_kernel, dim3(ceil_div(D, 256), rows), dim3(256), 0, s, c, sc, te, te_bstride, ce, ce_bstride, D);
    return DIT_LAUNCH_CHECK("dit_cond");
}

}  // namespace adf
