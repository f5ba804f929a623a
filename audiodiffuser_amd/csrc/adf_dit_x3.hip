// Kernels of the DiT's split-bf16 (f32x3) mode (adf_dit.h; the mode: adf_common.h): storage stays fp32, every matrix-core operand is hi = rn_bf16(x),
// lo = rn_bf16(x - hi), and a product is a_lo b_hi + a_hi b_lo + a_hi b_hi on v_mfma_f32_32x32x16_bf16 with fp32 accumulation.
#include "adf_dit.h"

#define DIT_LAUNCH_CHECK(name) (hipGetLastError() == hipSuccess ? nullptr : name ": launch failed")

namespace adf {

typedef float x3_f32x16_t __attribute__((ext_vector_type(16)));
typedef float x3_f32x2_t __attribute__((ext_vector_type(2)));
typedef __bf16 x3_bf16x8_t __attribute__((ext_vector_type(8)));

// =====================================================================================================
// Weight split: fp32 [rows][K] (rows padded to whole N tiles, the padding zero) -> bf16 hi and lo planes of the same shape
// =====================================================================================================
__global__ void __launch_bounds__(256) dit_split_weight_kernel(const float* __restrict__ w, unsigned short* __restrict__ hi, unsigned short* __restrict__ lo,
                                                               long long n4) {
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long long)gridDim.x * 256) {
        const f32x4_hw_t v = *(const f32x4_hw_t*)(w + 4 * i);
        const float f[4] = {v.x, v.y, v.z, v.w};
        u32x2_t h, l;
        split_bf16x4(f, h, l);
        *(u32x2_t*)(hi + 4 * i) = h;
        *(u32x2_t*)(lo + 4 * i) = l;
    }
}

const char* launch_dit_split_weight(const float* w, unsigned short* hi, unsigned short* lo, long long numel, hipStream_t s) {
    if (!w || !hi || !lo) return "dit_split_weight: null operand";
    if (numel < 4 || numel % 4) return "dit_split_weight: the element count must be a positive multiple of 4";
    if (((uintptr_t)w & 15) || (((uintptr_t)hi | (uintptr_t)lo) & 7)) return "dit_split_weight: misaligned operand";
    const long long n4 = numel / 4;
    const unsigned grid = (unsigned)((n4 + 255) / 256 > 8192 ? 8192 : (n4 + 255) / 256);
    hipLaunchKernelGGL(dit_split_weight_kernel, dim3(grid), dim3(256), 0, s, w, hi, lo, n4);
    return DIT_LAUNCH_CHECK("dit_split_weight");
}

// =====================================================================================================
// Token linear: Y = epi(X W^T + b), three bf16 MFMAs per product
// =====================================================================================================
// The tiling of dit_linear_kernel (adf_dit.hip): four waves own a 128 x 128 tile of Y, wave (wm, wn) 64 x 64 of it as 2 x 2 MFMA tiles, operands go
// through two LDS buffers with one barrier per K step.  A K step is 32: an LDS row holds its 32 hi parts (64 B), its 32 lo parts (64 B) and 16 B of
// padding (pitch 144 B = 36 banks: eight consecutive rows start in eight different groups of four banks, so the 16-byte fragment reads do not
// collide).  An activation is split ONCE, on its way from the staging registers into LDS; the weight arrives split (launch_dit_split_weight) and
// padded to whole tiles, so its staging loads are unguarded.  Rows past M re-read row M - 1 and are never stored.
// Fragment of MFMA step s (0, 1) of a K step: lane (l31, kh) reads k = 16 s + 8 kh .. + 7 of row l31 -- the same slice of both operands.
constexpr int kX3Pitch = 144;
constexpr int kX3Tile = 128 * kX3Pitch;                  // one operand tile
constexpr int kX3LinearLds = 4 * kX3Tile;                // A and B, two buffers each: 72 KB

__global__ void __launch_bounds__(256, 2) dit_linear_x3_kernel(const DitLinearArgs a, const unsigned short* __restrict__ wh,
                                                               const unsigned short* __restrict__ wl) {
    extern __shared__ __attribute__((aligned(16))) char x3_lin_smem[];
    char* const sA = x3_lin_smem;                        // [2][kX3Tile]
    char* const sB = x3_lin_smem + 2 * kX3Tile;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1, l31 = lane & 31, kh = lane >> 5;
    const int m0 = blockIdx.y * kDitTileM, n0 = blockIdx.x * kDitTileN;
    const int K = a.K;
    // staging, four 16-byte loads per thread and operand.  X: piece tid + 256 i -> row (idx >> 3), floats 4 (idx & 7) ..; W: pieces 0 .. 511 the hi
    // plane, 512 .. 1023 the lo plane, row ((idx & 511) >> 2), bf16 8 (idx & 3) ..
    const float* ga[4];
    const unsigned short* gb[4];
    int sa[4], sb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int idx = tid + 256 * i, row = idx >> 3, c = idx & 7;
        const int mr = m0 + row < a.M ? m0 + row : a.M - 1;
        ga[i] = a.x + (size_t)mr * K + c * 4;
        sa[i] = row * kX3Pitch + c * 8;
        const int plane = idx >> 9, wrow = (idx & 511) >> 2, wc = idx & 3;
        gb[i] = (plane ? wl : wh) + (size_t)(n0 + wrow) * K + wc * 8;
        sb[i] = wrow * kX3Pitch + plane * 64 + wc * 16;
    }
    x3_f32x16_t acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][t][e] = 0.f;
    f32x4_hw_t ra[4];
    u32x4_t rb[4];
    auto stage = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float f[4] = {ra[i].x, ra[i].y, ra[i].z, ra[i].w};
            u32x2_t hi, lo;
            split_bf16x4(f, hi, lo);
            *(u32x2_t*)(sA + buf * kX3Tile + sa[i]) = hi;
            *(u32x2_t*)(sA + buf * kX3Tile + sa[i] + 64) = lo;
            *(u32x4_t*)(sB + buf * kX3Tile + sb[i]) = rb[i];
        }
    };
#pragma unroll
    for (int i = 0; i < 4; ++i) { ra[i] = *(const f32x4_hw_t*)ga[i]; rb[i] = *(const u32x4_t*)gb[i]; }
    stage(0);
    __syncthreads();
    const int nk = K / kDitX3TileK;
    const int fa = (wm * 64 + l31) * kX3Pitch + kh * 16, fb = (wn * 64 + l31) * kX3Pitch + kh * 16;
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        const bool more = kt + 1 < nk;
        if (more) {
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                ra[i] = *(const f32x4_hw_t*)(ga[i] + (size_t)(kt + 1) * kDitX3TileK);
                rb[i] = *(const u32x4_t*)(gb[i] + (size_t)(kt + 1) * kDitX3TileK);
            }
        }
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            x3_bf16x8_t ah[2], al[2], bh[2], bl[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const char* pa = sA + cur * kX3Tile + fa + i * 32 * kX3Pitch + ks * 32;
                const char* pb = sB + cur * kX3Tile + fb + i * 32 * kX3Pitch + ks * 32;
                ah[i] = *(const x3_bf16x8_t*)pa; al[i] = *(const x3_bf16x8_t*)(pa + 64);
                bh[i] = *(const x3_bf16x8_t*)pb; bl[i] = *(const x3_bf16x8_t*)(pb + 64);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int t = 0; t < 2; ++t) {
                    acc[i][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[i], bh[t], acc[i][t], 0, 0, 0);
                    acc[i][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bl[t], acc[i][t], 0, 0, 0);
                    acc[i][t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[i], bh[t], acc[i][t], 0, 0, 0);
                }
        }
        if (more) stage(cur ^ 1);
        __syncthreads();
    }
    // the epilogues of dit_linear_kernel.  C/D map of the 32 x 32 MFMA: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
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

const char* launch_dit_linear_x3(const DitLinearArgs& a, const unsigned short* w_hi, const unsigned short* w_lo, hipStream_t s) {
    if (!a.x || !w_hi || !w_lo || !a.y) return "dit_linear_x3: null operand";
    if (a.M < 1 || a.N < 1 || a.K < kDitX3TileK || a.K % kDitX3TileK) return "dit_linear_x3: M, N >= 1 and K a positive multiple of 32";
    if (a.epi != kDitEpiBias && a.epi != kDitEpiGelu && a.epi != kDitEpiGate) return "dit_linear_x3: unknown epilogue";
    if (a.epi == kDitEpiGate && (!a.res || !a.gate || a.T < 1)) return "dit_linear_x3: the gated epilogue needs res, gate and T";
    if (((uintptr_t)a.x | (uintptr_t)w_hi | (uintptr_t)w_lo) & 15) return "dit_linear_x3: operands must be 16-byte aligned";
    const long long mt = ((long long)a.M + kDitTileM - 1) / kDitTileM;
    if (mt > 65535) return "dit_linear_x3: too many rows";
    if (!raise_lds_limit<kX3LinearLds, dit_linear_x3_kernel>()) return "dit_linear_x3: hipFuncSetAttribute failed";
    hipLaunchKernelGGL(dit_linear_x3_kernel, dim3(ceil_div(a.N, kDitTileN), (unsigned)mt), dim3(256), kX3LinearLds, s, a, w_hi, w_lo);
    return DIT_LAUNCH_CHECK("dit_linear_x3");
}

// =====================================================================================================
// Self-attention, key-tiled with an online softmax: head dim 32 or 64, any token count
// =====================================================================================================
// The plan of attention_x3_kernel (adf_kernels.hip) -- S^T = K Q^T with the query on the lane (lane-local softmax in the log2 domain), P^T split and
// reused as the B operand of O^T += V^T P^T -- over key tiles of 64 instead of a whole pair's V^T in LDS.  A workgroup of four waves owns 128 queries
// of one (sample, head) pair, 32 per wave, and walks the pair's keys: the K rows (kh / kl [key][D bf16], pitch 2 D + 16 B: conflict-free 16-byte
// reads with the key on the lane) and V^T (vth / vtl [d][64 keys], pitch 136 B) of a tile are split once while the workgroup stages them, and the
// loads of tile t + 1 are in flight while tile t is multiplied (two LDS stages, one barrier per tile).  Two adjacent keys go into V^T as one 4-byte
// store.  Keys past N in the last tile are staged from row N - 1 and get the score -inf (probability 0; every tile has at least one real key, so
// the running maximum is finite from the first tile on); queries past N run on row N - 1 and are not stored.
template <int D>
struct X3Att {
    static constexpr int KT = 64;                        // keys per tile
    static constexpr int KP = 2 * D + 16;                // bytes per K row (hi and lo arrays apart)
    static constexpr int VP = 2 * KT + 8;                // bytes per V^T row
    static constexpr int KBytes = KT * KP, VBytes = D * VP;
    static constexpr int Stage = 2 * KBytes + 2 * VBytes;
    static constexpr int Lds = 2 * Stage;                // D = 64: 70 KB; D = 32: 37 KB
    static constexpr int NK = D / 16;                    // K pieces (one key, four head dims) per thread and tile
    static constexpr int NV = D / 32;                    // V pieces (two keys, four head dims) per thread and tile
};

template <int D>
__global__ void __launch_bounds__(256, 2) dit_attention_x3_kernel(const float* __restrict__ qkv, float* __restrict__ out, int N, int C, int heads,
                                                                  int qgroups, float scale_log2e) {
    using L = X3Att<D>;
    constexpr int CPK = D / 4;                           // 16-byte chunks per key
    extern __shared__ __attribute__((aligned(16))) char x3_att_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;
    const int qg = blockIdx.x % qgroups, pair = blockIdx.x / qgroups;
    const int b = pair / heads, hd = pair - b * heads;
    const size_t rowstride = (size_t)3 * C;
    const float* base = qkv + (size_t)b * N * rowstride + (size_t)hd * D;
    const int ntiles = (N + L::KT - 1) / L::KT;
    const int query = (qg * 4 + wave) * 32 + r;
    const bool active = (qg * 4 + wave) * 32 < N;        // per wave
    const int qrow = query < N ? query : N - 1;

    f32x4_hw_t kreg[L::NK], vreg[L::NV][2];
    auto load_tile = [&](int kt) __attribute__((always_inline)) {
#pragma unroll
        for (int u = 0; u < L::NK; ++u) {
            const int idx = tid + 256 * u, key = kt * L::KT + idx / CPK, c = idx % CPK;
            kreg[u] = *(const f32x4_hw_t*)(base + (size_t)(key < N ? key : N - 1) * rowstride + C + c * 4);
        }
#pragma unroll
        for (int u = 0; u < L::NV; ++u) {
            const int idx = tid + 256 * u, key = kt * L::KT + 2 * (idx / CPK), c = idx % CPK;
            vreg[u][0] = *(const f32x4_hw_t*)(base + (size_t)(key < N ? key : N - 1) * rowstride + 2 * C + c * 4);
            vreg[u][1] = *(const f32x4_hw_t*)(base + (size_t)(key + 1 < N ? key + 1 : N - 1) * rowstride + 2 * C + c * 4);
        }
    };
    auto store_tile = [&](int stage) __attribute__((always_inline)) {
        char* kh = x3_att_smem + stage * L::Stage;
        char* kl = kh + L::KBytes;
        char* vth = kl + L::KBytes;
        char* vtl = vth + L::VBytes;
#pragma unroll
        for (int u = 0; u < L::NK; ++u) {
            const int idx = tid + 256 * u, key = idx / CPK, c = idx % CPK;
            const float f[4] = {kreg[u].x, kreg[u].y, kreg[u].z, kreg[u].w};
            u32x2_t hi, lo;
            split_bf16x4(f, hi, lo);
            *(u32x2_t*)(kh + key * L::KP + c * 8) = hi;
            *(u32x2_t*)(kl + key * L::KP + c * 8) = lo;
        }
#pragma unroll
        for (int u = 0; u < L::NV; ++u) {
            const int idx = tid + 256 * u, kp = idx / CPK, c = idx % CPK;
            const float f0[4] = {vreg[u][0].x, vreg[u][0].y, vreg[u][0].z, vreg[u][0].w};
            const float f1[4] = {vreg[u][1].x, vreg[u][1].y, vreg[u][1].z, vreg[u][1].w};
            u32x2_t h0, l0, h1, l1;
            split_bf16x4(f0, h0, l0);
            split_bf16x4(f1, h1, l1);
            // head dim 4 c + j of keys 2 kp (low half) and 2 kp + 1 (high half)
            const unsigned hw[4] = {(h0.x & 0xffffu) | (h1.x << 16), (h0.x >> 16) | (h1.x & 0xffff0000u), (h0.y & 0xffffu) | (h1.y << 16), (h0.y >> 16) | (h1.y & 0xffff0000u)};
            const unsigned lw[4] = {(l0.x & 0xffffu) | (l1.x << 16), (l0.x >> 16) | (l1.x & 0xffff0000u), (l0.y & 0xffffu) | (l1.y << 16), (l0.y >> 16) | (l1.y & 0xffff0000u)};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                *(unsigned*)(vth + (c * 4 + j) * L::VP + kp * 4) = hw[j];
                *(unsigned*)(vtl + (c * 4 + j) * L::VP + kp * 4) = lw[j];
            }
        }
    };

    load_tile(0);
    // Q^T fragments (B operand): head dims 16 ks + 8 hh .. + 7 of this lane's query
    x3_bf16x8_t qh[D / 16], ql[D / 16];
#pragma unroll
    for (int ks = 0; ks < D / 16; ++ks) {
        const float* qp = base + (size_t)qrow * rowstride + ks * 16 + hh * 8;
        const f32x4_hw_t a0 = *(const f32x4_hw_t*)qp, a1 = *(const f32x4_hw_t*)(qp + 4);
        const float f0[4] = {a0.x, a0.y, a0.z, a0.w}, f1[4] = {a1.x, a1.y, a1.z, a1.w};
        u32x2_t h0, l0, h1, l1;
        split_bf16x4(f0, h0, l0);
        split_bf16x4(f1, h1, l1);
        qh[ks] = __builtin_bit_cast(x3_bf16x8_t, u32x4_t{h0.x, h0.y, h1.x, h1.y});
        ql[ks] = __builtin_bit_cast(x3_bf16x8_t, u32x4_t{l0.x, l0.y, l1.x, l1.y});
    }
    store_tile(0);
    __syncthreads();

    x3_f32x16_t o[D / 32];
#pragma unroll
    for (int t = 0; t < D / 32; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[t][e] = 0.f;
    float m = -INFINITY, l = 0.f;                        // running maximum in the scaled log2 domain, running sum (this lane's half of the keys)
    for (int kt = 0; kt < ntiles; ++kt) {
        const int cur = kt & 1;
        const bool more = kt + 1 < ntiles;
        if (more) load_tile(kt + 1);
        if (active) {
            const char* kh = x3_att_smem + cur * L::Stage;
            const char* kl = kh + L::KBytes;
            const char* vth = kl + L::KBytes;
            const char* vtl = vth + L::VBytes;
            x3_f32x16_t st[2];
#pragma unroll
            for (int kk = 0; kk < 2; ++kk) {
#pragma unroll
                for (int e = 0; e < 16; ++e) st[kk][e] = 0.f;
#pragma unroll
                for (int ks = 0; ks < D / 16; ++ks) {
                    const x3_bf16x8_t fh = *(const x3_bf16x8_t*)(kh + (kk * 32 + r) * L::KP + (ks * 2 + hh) * 16);
                    const x3_bf16x8_t fl = *(const x3_bf16x8_t*)(kl + (kk * 32 + r) * L::KP + (ks * 2 + hh) * 16);
                    st[kk] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fl, qh[ks], st[kk], 0, 0, 0);
                    st[kk] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fh, ql[ks], st[kk], 0, 0, 0);
                    st[kk] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fh, qh[ks], st[kk], 0, 0, 0);
                }
            }
            // register e of subtile kk = key 64 kt + 32 kk + (e & 3) + 8 (e >> 2) + 4 hh
            if (!more && (N & (L::KT - 1))) {            // uniform: the partial key tile
#pragma unroll
                for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int key = kt * L::KT + kk * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
                        st[kk][e] = key < N ? st[kk][e] : -INFINITY;
                    }
            }
            float mt = st[0][0];
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int e = 0; e < 16; ++e) mt = fmaxf(mt, st[kk][e]);
            mt *= scale_log2e;                            // (the scale is positive)
            {
                const unsigned mu = __float_as_uint(mt);
                const auto sw = __builtin_amdgcn_permlane32_swap(mu, mu, false, false);
                mt = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
            }
            if (!__all(mt <= m)) {                        // some query's maximum grew: rescale (else alpha == 1 exactly)
                const float mn = fmaxf(m, mt);
                const float alpha = __builtin_amdgcn_exp2f(m - mn);
                l *= alpha;
#pragma unroll
                for (int t = 0; t < D / 32; ++t)
#pragma unroll
                    for (int e = 0; e < 16; ++e) o[t][e] *= alpha;
                m = mn;
            }
            float psum = 0.f;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const float pv = __builtin_amdgcn_exp2f(fmaf(st[kk][e], scale_log2e, -m));
                    st[kk][e] = pv;
                    psum += pv;
                }
            l += psum;
#pragma unroll
            for (int kk = 0; kk < 2; ++kk)
#pragma unroll
                for (int sgrp = 0; sgrp < 2; ++sgrp) {
                    float pf[8];
#pragma unroll
                    for (int j = 0; j < 8; ++j) pf[j] = st[kk][8 * sgrp + j];
                    u32x2_t h0, l0, h1, l1;
                    split_bf16x4(pf, h0, l0);
                    split_bf16x4(pf + 4, h1, l1);
                    const x3_bf16x8_t ph = __builtin_bit_cast(x3_bf16x8_t, u32x4_t{h0.x, h0.y, h1.x, h1.y});
                    const x3_bf16x8_t pl = __builtin_bit_cast(x3_bf16x8_t, u32x4_t{l0.x, l0.y, l1.x, l1.y});
                    // V^T fragments of this lane's head dim: elements j = 0 .. 3 = keys 16 s + 4 hh + j of the subtile, j = 4 .. 7 = keys 16 s + 8 + 4 hh + (j - 4)
                    const int ko = (kk * 32 + sgrp * 16) * 2 + hh * 8;
#pragma unroll
                    for (int t = 0; t < D / 32; ++t) {
                        const char* vh_row = vth + (t * 32 + r) * L::VP + ko;
                        const char* vl_row = vtl + (t * 32 + r) * L::VP + ko;
                        const u32x2_t a0 = *(const u32x2_t*)vh_row, a1 = *(const u32x2_t*)(vh_row + 16);
                        const u32x2_t b0 = *(const u32x2_t*)vl_row, b1 = *(const u32x2_t*)(vl_row + 16);
                        const x3_bf16x8_t vh = __builtin_bit_cast(x3_bf16x8_t, u32x4_t{a0.x, a0.y, a1.x, a1.y});
                        const x3_bf16x8_t vl = __builtin_bit_cast(x3_bf16x8_t, u32x4_t{b0.x, b0.y, b1.x, b1.y});
                        o[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vl, ph, o[t], 0, 0, 0);
                        o[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vh, pl, o[t], 0, 0, 0);
                        o[t] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vh, ph, o[t], 0, 0, 0);
                    }
                }
        }
        if (more) store_tile(cur ^ 1);
        __syncthreads();
    }
    if (!active) return;
    l += __shfl_xor(l, 32, 64);
    const float inv = 1.0f / l;
    if (query < N) {
        float* orow = out + ((size_t)b * N + query) * C + (size_t)hd * D;
#pragma unroll
        for (int t = 0; t < D / 32; ++t)
#pragma unroll
            for (int g = 0; g < 4; ++g)      // registers 4 g .. 4 g + 3 of tile t = head dims 32 t + 8 g + 4 hh .. + 3
                *(f32x4_hw_t*)(orow + t * 32 + 8 * g + 4 * hh) =
                    f32x4_hw_t{o[t][4 * g] * inv, o[t][4 * g + 1] * inv, o[t][4 * g + 2] * inv, o[t][4 * g + 3] * inv};
    }
}

const char* launch_dit_attention_x3(const float* qkv, float* out, int B, int N, int C, int heads, hipStream_t s) {
    if (!qkv || !out) return "dit_attention_x3: null operand";
    if (B < 1 || N < 1 || heads < 1 || C % heads) return "dit_attention_x3: bad shape";
    const int dh = C / heads;
    if (dh != 32 && dh != 64) return "dit_attention_x3: head dim must be 32 or 64";
    if (((uintptr_t)qkv | (uintptr_t)out) & 15) return "dit_attention_x3: operands must be 16-byte aligned";
    const int qgroups = ceil_div(ceil_div(N, 32), 4);
    const long long blocks = (long long)B * heads * qgroups;
    if (blocks > 0x7fffffffLL) return "dit_attention_x3: too many query tiles";
    const float sl2e = (float)(1.4426950408889634 / sqrt((double)dh));
    if (dh == 64) {
        if (!raise_lds_limit<X3Att<64>::Lds, dit_attention_x3_kernel<64>>()) return "dit_attention_x3: hipFuncSetAttribute failed";
        hipLaunchKernelGGL(dit_attention_x3_kernel<64>, dim3((unsigned)blocks), dim3(256), X3Att<64>::Lds, s, qkv, out, N, C, heads, qgroups, sl2e);
    } else {
        hipLaunchKernelGGL(dit_attention_x3_kernel<32>, dim3((unsigned)blocks), dim3(256), X3Att<32>::Lds, s, qkv, out, N, C, heads, qgroups, sl2e);
    }
    return DIT_LAUNCH_CHECK("dit_attention_x3");
}

}  // namespace adf
