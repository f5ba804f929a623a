// WaveToSpec (adf_stft.h): the kernel, the host basis, the plan and the adf_stft_* entry points of include/audiodiffuser_amd.h.
// Replaces, in front of the network, src/models/diffunet_complex_module.py:109-115 (torch.stft with center=True and reflect padding,
// spec_fwd of src/models/utils.py:8-19, cat of the real and the imaginary part).
#include "adf_stft.h"
#include "adf_spectral_host.h"

#include <cmath>
#include <string>
#include <vector>

namespace adf {

typedef __attribute__((ext_vector_type(16))) float st_f32x16_t;

// g = r^(e - 1) from r2 = r^2 (kStftPow*)
__device__ __forceinline__ float stft_gain(float r2, int pmode, float pexp) {
    if (pmode == kStftPowOne) return 1.f;
    if (!(r2 > 0.f)) return 0.f;
    if (pmode == kStftPowHalf) return rsqrtf(sqrtf(r2));
    if (pmode == kStftPowFifth && r2 > 1e-18f && r2 < 1e18f) {        // r2^2 and g^5 stay normal numbers inside this range
        float g = __builtin_amdgcn_exp2f(-0.4f * __builtin_amdgcn_logf(r2));
        const float c = r2 * r2, g2 = g * g;
        return fmaf(g * 0.2f, fmaf(-(c * g2 * g2), g, 1.f), g);    // g + g (1 - c g^5) / 5
    }
    return powf(r2, pexp);
}

// One block = 4 waves = WM bin tiles x WN frame tiles of 32 x 32; every wave owns a cosine and a sine accumulator tile over the whole K.
template <int WN>
__global__ __launch_bounds__(256) void stft_gemm_kernel(const StftArgs a) {
    constexpr int WM = 4 / WN;
    constexpr int NTB = 32 * WN;                  // frames per block
    constexpr int QP = NTB + kStftQPad;           // row pitch of the phase-major stage [h][QP]
    extern __shared__ float stage[];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;
    const int wm = wave % WM, wn = wave / WM;
    const int b = blockIdx.z;
    const int mt = blockIdx.y * WM + wm;
    const bool active = mt < a.MT;                // F = 129, 65, ...: the last bin group is not full
    const int t0 = blockIdx.x * NTB;
    const int h = a.h, NKI = a.NKI;

    // ---- A operand: 8 x 16 bytes per lane = the 32 MFMAs of one K iteration, prefetched one iteration ahead -------------------------------
    f32x4_hw_t a_cur[8], a_nxt[8];
    auto load_a = [&](f32x4_hw_t* dst, int it) {
        const f32x4_hw_t* p = a.apack + ((size_t)(mt * NKI + it) * 8) * 64 + lane;
#pragma unroll
        for (int g = 0; g < 8; ++g) dst[g] = p[g * 64];
    };
    if (active) load_a(a_cur, 0);

    // ---- B operand: the block's span of reflect-padded audio, global -> LDS, phase-major -------------------------------------------------
    {
        const int span = (NTB - 1) * h + NKI * kStftKC;
        const int first = t0 * h - a.half;                    // index into the row of the first staged sample (may lie before 0)
        const float* xb = a.audio + (size_t)b * a.L;
        for (int idx = tid; idx < span; idx += 256) {
            int j = first + idx;
            if (j < 0) j = -j;                                // L > n_fft / 2: one reflection brings every sample a kept frame reads inside
            else if (j >= a.L) j = 2 * (a.L - 1) - j;
            const float v = (j >= 0 && j < a.L) ? xb[j] : 0.f;    // past the reflection: only frames t >= T and basis columns m >= n_fft read it
            const int q = idx / h, p = idx - q * h;
            stage[p * QP + q] = v;
        }
    }
    __syncthreads();
    if (!active) return;                                      // no barrier below

    st_f32x16_t acc_c, acc_s;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc_c[e] = acc_s[e] = 0.f;

    // sample m = 32 it + 2 s + hh of frame t0 + 32 wn + r: h is a multiple of 32, so an iteration stays inside one q
    const float* sb = stage + hh * QP + wn * 32 + r;
    int pb = 0, qb = 0;
    for (int it = 0; it < NKI; ++it) {
        if (it + 1 < NKI) load_a(a_nxt, it + 1);
        const float* row = sb + pb * QP + qb;
#pragma unroll
        for (int sg = 0; sg < 4; ++sg) {
            const f32x4_hw_t ac = a_cur[sg], as = a_cur[4 + sg];
            const float b0 = row[(8 * sg) * QP], b1 = row[(8 * sg + 2) * QP], b2 = row[(8 * sg + 4) * QP], b3 = row[(8 * sg + 6) * QP];
            acc_c = __builtin_amdgcn_mfma_f32_32x32x2f32(ac.x, b0, acc_c, 0, 0, 0);
            acc_s = __builtin_amdgcn_mfma_f32_32x32x2f32(as.x, b0, acc_s, 0, 0, 0);
            acc_c = __builtin_amdgcn_mfma_f32_32x32x2f32(ac.y, b1, acc_c, 0, 0, 0);
            acc_s = __builtin_amdgcn_mfma_f32_32x32x2f32(as.y, b1, acc_s, 0, 0, 0);
            acc_c = __builtin_amdgcn_mfma_f32_32x32x2f32(ac.z, b2, acc_c, 0, 0, 0);
            acc_s = __builtin_amdgcn_mfma_f32_32x32x2f32(as.z, b2, acc_s, 0, 0, 0);
            acc_c = __builtin_amdgcn_mfma_f32_32x32x2f32(ac.w, b3, acc_c, 0, 0, 0);
            acc_s = __builtin_amdgcn_mfma_f32_32x32x2f32(as.w, b3, acc_s, 0, 0, 0);
        }
#pragma unroll
        for (int g = 0; g < 8; ++g) a_cur[g] = a_nxt[g];
        pb += kStftKC;
        if (pb == h) { pb = 0; ++qb; }
    }

    // ---- epilogue: spec_fwd on the lane's own (re, im) pairs; a store instruction writes 2 bins x 32 consecutive frames ------------------
    const int t = t0 + wn * 32 + r;
    if (t >= a.T) return;
    const size_t plane = (size_t)a.F * a.T;
    float* ob = a.spec + (size_t)b * 2 * plane + t;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int k = mt * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
        const float xr = acc_c[e], xi = acc_s[e];
        const float g = stft_gain(xr * xr + xi * xi, a.pmode, a.pexp) * a.factor;
        if (k < a.F) {
            ob[(size_t)k * a.T] = xr * g;
            ob[plane + (size_t)k * a.T] = xi * g;
        }
    }
}

hipError_t launch_stft(const StftArgs& a, hipStream_t s) {
    const int wn = stft_wn(a.F, a.h), wm = 4 / wn;
    const dim3 grid((a.T + 32 * wn - 1) / (32 * wn), (a.MT + wm - 1) / wm, a.B);
    const size_t lds = stft_lds_bytes(wn, a.h);
    if (wn == 2) hipLaunchKernelGGL(stft_gemm_kernel<2>, grid, dim3(256), lds, s, a);
    else hipLaunchKernelGGL(stft_gemm_kernel<1>, grid, dim3(256), lds, s, a);
    return hipGetLastError();
}

}  // namespace adf

// =====================================================================================================
// host: argument checks, the basis, the plan
// =====================================================================================================
struct adf_stft_plan {
    int device = 0;
    int n_fft = 0, h = 0, F = 0, MT = 0, NKI = 0;
    int pmode = 0;
    float pexp = 0.f, factor = 1.f;
    float* apack = nullptr;
};

namespace {

using adf_spectral::fail;

int stft_check(const char* fn, const adf_istft_config* cfg, const float* window) {
    if (adf_spectral::check_config(fn, cfg, "center=False, a transform without the reflect padding, is not built")) return 1;
    if (window) {
        bool any = false;
        for (int m = 0; m < cfg->n_fft; ++m) {
            if (!std::isfinite(window[m])) return fail(std::string(fn) + ": window: value " + std::to_string(m) + " is not finite");
            any = any || window[m] != 0.f;
        }
        if (!any) return fail(std::string(fn) + ": window: every value is zero");
    }
    return 0;
}

// basis [2][F][n_fft] (include/audiodiffuser_amd.h)
void stft_tables(const adf_istft_config& c, const float* window, float* basis) {
    const int N = c.n_fft, F = N / 2 + 1;
    const std::vector<double> w = adf_spectral::window_f64(c, window);
    const double s = c.normalized ? 1.0 / std::sqrt((double)N) : 1.0;
    float* Cb = basis;
    float* Sb = basis + (size_t)F * N;
    for (int k = 0; k < F; ++k)
        for (int m = 0; m < N; ++m) {
            const double ang = 2.0 * M_PI * (double)(((long long)m * k) % N) / N;      // the phase is reduced in integers
            Cb[(size_t)k * N + m] = (float)(w[m] * std::cos(ang) * s);
            Sb[(size_t)k * N + m] = (k == 0 || k == F - 1) ? 0.f : (float)(-w[m] * std::sin(ang) * s);
        }
}

}  // namespace

extern "C" {

int adf_stft_basis(const adf_istft_config* cfg, const float* window, float* basis) {
    if (stft_check("adf_stft_basis", cfg, window)) return 1;
    if (basis) stft_tables(*cfg, window, basis);
    return 0;
}

int adf_stft_create(const adf_istft_config* cfg, const float* window, adf_stft_plan** out) {
    if (!out) return fail("adf_stft_create: null argument");
    *out = nullptr;
    if (stft_check("adf_stft_create", cfg, window)) return 1;
    const adf_istft_config& c = *cfg;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return fail("adf_stft_create: no HIP device available");
    std::unique_ptr<adf_stft_plan> p(new adf_stft_plan());
    if (hipGetDevice(&p->device) != hipSuccess) return fail("adf_stft_create: hipGetDevice failed");
    const int N = c.n_fft, F = N / 2 + 1, KC = adf::kStftKC, MT = (F + 31) / 32, NKI = (N + KC - 1) / KC;
    p->n_fft = N; p->h = c.hop_length; p->F = F; p->MT = MT; p->NKI = NKI;
    const double e = c.spec_abs_exponent;
    p->pmode = e == 1.0 ? adf::kStftPowOne : std::fabs(e - 0.5) < 1e-12 ? adf::kStftPowHalf : std::fabs(e - 0.2) < 1e-12 ? adf::kStftPowFifth
             : adf::kStftPowGeneral;
    p->pexp = (float)(0.5 * (e - 1.0));
    p->factor = (float)c.spec_factor;

    std::vector<float> basis((size_t)2 * F * N);
    stft_tables(c, window, basis.data());
    // fragment order (StftArgs::apack); bins past F and window positions past n_fft are the zero rows and columns that pad M and K
    std::vector<float> pack((size_t)MT * NKI * 8 * 64 * 4);
    size_t o = 0;
    for (int mt = 0; mt < MT; ++mt)
        for (int it = 0; it < NKI; ++it)
            for (int comp = 0; comp < 2; ++comp)
                for (int sg = 0; sg < 4; ++sg)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int q = 0; q < 4; ++q) {
                            const int k = mt * 32 + (lane & 31);
                            const int m = it * KC + 8 * sg + 2 * q + (lane >> 5);
                            pack[o++] = (k < F && m < N) ? basis[((size_t)comp * F + k) * N + m] : 0.f;
                        }
    if (hipMalloc((void**)&p->apack, pack.size() * 4) != hipSuccess ||
        hipMemcpy(p->apack, pack.data(), pack.size() * 4, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        adf_stft_destroy(p.release());
        return fail("adf_stft_create: device allocation or copy of the basis failed");
    }
    *out = p.release();
    return 0;
}

int adf_stft_run(adf_stft_plan* plan, const float* audio, int B, int64_t L, float* spec, int T, void* stream) {
    if (!plan || !audio || !spec) return fail("adf_stft_run: null argument");
    if (B < 1 || B > 65535) return fail("adf_stft_run: B must be in [1, 65535]");
    const int half = plan->n_fft / 2;
    if (L <= half)
        return fail("adf_stft_run: audio: L must be greater than n_fft / 2 = " + std::to_string(half) + " (reflect padding), got " + std::to_string((long long)L));
    if (L >= (int64_t)1 << 30) return fail("adf_stft_run: L is too large (the kernel indexes a row in 32 bits)");
    const int64_t want = 1 + L / plan->h;
    if (T != want) return fail("adf_stft_run: T must be 1 + L / hop_length = " + std::to_string((long long)want));
    adf_spectral::DeviceScope scope(plan->device);
    if (!scope.ok) return fail("adf_stft_run: could not make the plan's device current");
    adf::StftArgs a;
    a.audio = audio; a.spec = spec; a.apack = (const adf::f32x4_hw_t*)plan->apack;
    a.B = B; a.L = (int)L; a.T = T; a.F = plan->F; a.h = plan->h; a.half = half;
    a.MT = plan->MT; a.NKI = plan->NKI;
    a.pmode = plan->pmode; a.pexp = plan->pexp; a.factor = plan->factor;
    const hipError_t e = adf::launch_stft(a, (hipStream_t)stream);
    if (e != hipSuccess) return fail(std::string("adf_stft_run: launch failed: ") + hipGetErrorString(e));
    return 0;
}

void adf_stft_destroy(adf_stft_plan* plan) {
    if (!plan) return;
    {
        adf_spectral::DeviceScope scope(plan->device);
        if (plan->apack) (void)hipFree(plan->apack);
    }
    delete plan;
}

}  // extern "C"
