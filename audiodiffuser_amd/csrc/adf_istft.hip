// SpecToWave (adf_istft.h): the kernel, the host tables, the plan and the adf_istft_* entry points of include/audiodiffuser_amd.h.
// Replaces, after the sampler, src/models/diffunet_complex_module.py:90-99 (permute + view_as_complex, spec_back of src/models/utils.py:22-28,
// torch.istft with center=True and length=None).
#include "adf_istft.h"
#include "adf_spectral_host.h"

#include <cmath>
#include <string>
#include <vector>

namespace adf {

typedef __attribute__((ext_vector_type(16))) float is_f32x16_t;

// One block = 4 waves = WM row tiles x WN hop-block tiles of 32 x 32; every wave owns one accumulator tile over the whole K.
template <int WN>
__global__ __launch_bounds__(256) void istft_gemm_kernel(const IstftArgs a) {
    constexpr int WM = 4 / WN;
    constexpr int NTB = 32 * WN;                  // hop blocks per block
    constexpr int TMB = 32 * WM;                  // samples of a hop block per block
    constexpr int KC = kIstftKC;
    constexpr int SW = NTB + kIstftMaxD;          // staged frames: j0 - (D - 1) .. ; row pitch of the stage
    constexpr int STAGE = 2 * KC * SW;            // floats of one stage buffer: [component][bin][frame]
    constexpr int NPAIR = KC * SW;                // (bin, frame) pairs of a chunk
    constexpr int PPT = (NPAIR + 255) / 256;      // pairs per thread
    constexpr int TP = TMB + 4;                   // row pitch of the epilogue tile [hop block][sample]
    static_assert(2 * STAGE >= NTB * TP, "the epilogue tile reuses the two stage buffers");
    __shared__ __attribute__((aligned(16))) float smem[2 * STAGE];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane & 31, hh = lane >> 5;
    const int wm = wave % WM, wn = wave / WM;
    const int b = blockIdx.z, mg = blockIdx.y;
    const int j0 = a.jlo + blockIdx.x * NTB;
    const int t0 = j0 - (a.D - 1);
    const int mt = mg * WM + wm;
    const bool active = mt < a.MT;                // h = 96, 160, ...: the last row group is not full
    const int D = a.D, NCH = a.NCH;

    // ---- B operand: global -> registers (raw), registers -> LDS with spec_back applied once per element ------------------
    float x0[PPT], x1[PPT];
    auto stage_load = [&](int ch) {
#pragma unroll
        for (int i = 0; i < PPT; ++i) {
            const int idx = tid + i * 256;
            const int kk = idx / SW, cc = idx - kk * SW;
            const int k = ch * KC + kk, t = t0 + cc;
            const bool ok = idx < NPAIR && k < a.F && t >= 0 && t < a.T;
            const size_t off = ((size_t)(b * 2) * a.F + k) * a.T + t;
            x0[i] = ok ? a.spec[off] : 0.f;
            x1[i] = ok ? a.spec[off + (size_t)a.F * a.T] : 0.f;
        }
    };
    auto stage_store = [&](int buf) {
        float* st = smem + buf * STAGE;
#pragma unroll
        for (int i = 0; i < PPT; ++i) {
            const int idx = tid + i * 256;
            if (idx < NPAIR) {
                const int kk = idx / SW, cc = idx - kk * SW;
                const float u0 = x0[i] / a.factor, u1 = x1[i] / a.factor;
                const float r2 = u0 * u0 + u1 * u1;
                float g = 1.f;
                if (a.pmode == kIstftPowTwo) g = sqrtf(r2);
                else if (a.pmode == kIstftPowFive) g = r2 * r2;
                else if (a.pmode == kIstftPowGeneral) g = r2 > 0.f ? powf(sqrtf(r2), a.pexp) : 0.f;
                st[kk * SW + cc] = g * u0;
                st[(KC + kk) * SW + cc] = g * u1;
            }
        }
    };

    // ---- A operand: 8 x 16 bytes per lane = the 32 MFMAs of one (segment, chunk), prefetched one item ahead ---------------
    f32x4_hw_t a_cur[8], a_nxt[8];
    auto load_a = [&](f32x4_hw_t* dst, int ch, int d) {
        const f32x4_hw_t* p = a.apack + ((((size_t)d * a.MT + mt) * NCH + ch) * 8) * 64 + lane;
#pragma unroll
        for (int g = 0; g < 8; ++g) dst[g] = p[g * 64];
    };

    is_f32x16_t acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;

    if (active) load_a(a_cur, 0, 0);
    stage_load(0);
    stage_store(0);
    __syncthreads();
    for (int ch = 0; ch < NCH; ++ch) {
        const bool more = ch + 1 < NCH;
        if (more) stage_load(ch + 1);
        const float* sbuf = smem + (ch & 1) * STAGE + wn * 32 + r + hh * SW;
        for (int d = 0; d < D; ++d) {
            const int nd = d + 1 < D ? d + 1 : 0;
            const int nch = d + 1 < D ? ch : ch + 1;
            if (active) {
                if (nch < NCH) load_a(a_nxt, nch, nd);
                const float* sb = sbuf + (D - 1 - d);     // frame j - d of hop block j = j0 + 32 wn + r
#pragma unroll
                for (int c = 0; c < 2; ++c)
#pragma unroll
                    for (int sg = 0; sg < 4; ++sg) {
                        const f32x4_hw_t av = a_cur[c * 4 + sg];
                        const float* row = sb + (c * KC + 8 * sg) * SW;
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, row[0], acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, row[2 * SW], acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, row[4 * SW], acc, 0, 0, 0);
                        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, row[6 * SW], acc, 0, 0, 0);
                    }
#pragma unroll
                for (int g = 0; g < 8; ++g) a_cur[g] = a_nxt[g];
            }
        }
        if (more) stage_store((ch + 1) & 1);
        __syncthreads();
    }

    // ---- epilogue 1: accumulators -> LDS tile [hop block][sample] (every wave is past the last stage read) ----------------
    float* tile = smem;
    if (active) {
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4_hw_t v = {acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]};
            *(f32x4_hw_t*)(tile + (wn * 32 + r) * TP + wm * 32 + 8 * g + 4 * hh) = v;
        }
    }
    __syncthreads();

    // ---- epilogue 2: window envelope, trim, 16-byte stores on the output's own alignment (scalar at the run's two ends) ---
    constexpr int GPR = TMB / 4 + 1;              // 16-byte groups an unaligned run of TMB samples can touch
    const int m0 = mg * TMB;
    const int len = min(TMB, a.h - m0);
    float* outb = a.audio + (size_t)b * a.audio_len;
    for (int idx = tid; idx < NTB * GPR; idx += 256) {
        const int jj = idx / GPR, gi = idx - jj * GPR;
        const int j = j0 + jj;
        if (j >= a.jlo + a.nj) continue;
        const int o_start = j * a.h + m0 - a.half;          // output index of the run's first sample (may lie before 0)
        const int lo = max(o_start, 0), hi = min(o_start + len, a.audio_len);
        if (lo >= hi) continue;
        const int base = ((lo >> 2) + gi) * 4;
        if (base >= hi) continue;
        float v[4];
        bool ok[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int o = base + e;
            ok[e] = o >= lo && o < hi;
            v[e] = 0.f;
            if (ok[e]) {
                const int nl = o - o_start;                 // sample within the block's rows
                const int n = m0 + nl;
                float env = 0.f;
                for (int d = 0; d < D; ++d) {
                    const int t = j - d;
                    if (t >= 0 && t < a.T) env += a.wsq[d * a.h + n];
                }
                v[e] = tile[jj * TP + nl] / env;
            }
        }
        if (ok[0] && ok[1] && ok[2] && ok[3]) {
            *(f32x4_hw_t*)(outb + base) = f32x4_hw_t{v[0], v[1], v[2], v[3]};
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if (ok[e]) outb[base + e] = v[e];
        }
    }
}

hipError_t launch_istft(const IstftArgs& a, hipStream_t s) {
    const int wn = istft_wn(a.h), wm = 4 / wn;
    const dim3 grid((a.nj + 32 * wn - 1) / (32 * wn), (a.MT + wm - 1) / wm, a.B);
    if (wn == 4) hipLaunchKernelGGL(istft_gemm_kernel<4>, grid, dim3(256), 0, s, a);
    else if (wn == 2) hipLaunchKernelGGL(istft_gemm_kernel<2>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(istft_gemm_kernel<1>, grid, dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace adf

// =====================================================================================================
// host: argument checks, the tables, the plan
// =====================================================================================================
struct adf_istft_plan {
    int device = 0;
    int n_fft = 0, h = 0, F = 0, Fp = 0, D = 0;
    int pmode = 0;
    float pexp = 0.f, factor = 1.f;
    float* apack = nullptr;
    float* wsq = nullptr;
};

namespace {

using adf_spectral::window_f64;
typedef adf_spectral::DeviceScope IstftDeviceScope;

int istft_fail(const std::string& m) { return adf_spectral::fail(m); }

int istft_check(const char* fn, const adf_istft_config* cfg, const float* window) {
    if (adf_spectral::check_config(fn, cfg, "with center=False a Hann window fails torch.istft's own envelope check")) return 1;
    const std::string f = std::string(fn) + ": ";
    const adf_istft_config& c = *cfg;
    // torch.istft's NOLA check: the overlap-added squared window over the kept samples.  Two frames (every kept sample of any T >= 2 is covered by
    // at least the pair of frames checked here, and squares only add) and the steady state.
    const std::vector<double> w = window_f64(c, window);
    const int N = c.n_fft, h = c.hop_length, D = (N + h - 1) / h;
    auto wsq = [&](int off) { return off >= 0 && off < N ? w[off] * w[off] : 0.0; };
    double worst = 1e300;
    for (int p = N / 2; p < N / 2 + h; ++p) worst = std::min(worst, wsq(p) + wsq(p - h));
    for (int n = 0; n < h; ++n) {
        double e = 0.0;
        for (int d = 0; d < D; ++d) e += wsq(d * h + n);
        worst = std::min(worst, e);
    }
    if (!(worst > 1e-11)) return istft_fail(f + "window: the overlap-added squared window falls to " + std::to_string(worst) + " inside the kept samples (must stay above 1e-11, torch.istft's NOLA check)");
    return 0;
}

// basis [2][D h][F] and wsq [D h] (include/audiodiffuser_amd.h); either may be null.
void istft_tables(const adf_istft_config& c, const float* window, float* basis, float* wsq) {
    const int N = c.n_fft, h = c.hop_length, F = N / 2 + 1, D = (N + h - 1) / h, M = D * h;
    const std::vector<double> w = window_f64(c, window);
    const double s = c.normalized ? std::sqrt((double)N) / N : 1.0 / N;
    if (wsq)
        for (int m = 0; m < M; ++m) wsq[m] = m < N ? (float)(w[m] * w[m]) : 0.f;
    if (!basis) return;
    float* C = basis;
    float* S = basis + (size_t)M * F;
    for (int m = 0; m < M; ++m)
        for (int k = 0; k < F; ++k) {
            float cv = 0.f, sv = 0.f;
            if (m < N) {
                const double ak = (k == 0 || k == F - 1) ? 1.0 : 2.0;
                const double ang = 2.0 * M_PI * (double)(((long long)m * k) % N) / N;      // the phase is reduced in integers
                cv = (float)(w[m] * ak * std::cos(ang) * s);
                sv = (k == 0 || k == F - 1) ? 0.f : (float)(-w[m] * ak * std::sin(ang) * s);
            }
            C[(size_t)m * F + k] = cv;
            S[(size_t)m * F + k] = sv;
        }
}

}  // namespace

extern "C" {

int adf_istft_basis(const adf_istft_config* cfg, const float* window, float* basis, float* wsq) {
    if (istft_check("adf_istft_basis", cfg, window)) return 1;
    istft_tables(*cfg, window, basis, wsq);
    return 0;
}

int adf_istft_create(const adf_istft_config* cfg, const float* window, adf_istft_plan** out) {
    if (!out) return istft_fail("adf_istft_create: null argument");
    *out = nullptr;
    if (istft_check("adf_istft_create", cfg, window)) return 1;
    const adf_istft_config& c = *cfg;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev < 1) return istft_fail("adf_istft_create: no HIP device available");
    std::unique_ptr<adf_istft_plan> p(new adf_istft_plan());
    if (hipGetDevice(&p->device) != hipSuccess) return istft_fail("adf_istft_create: hipGetDevice failed");
    const int N = c.n_fft, h = c.hop_length, F = N / 2 + 1, D = (N + h - 1) / h, M = D * h;
    const int KC = adf::kIstftKC, Fp = (F + KC - 1) / KC * KC, MT = h / 32, NCH = Fp / KC;
    p->n_fft = N; p->h = h; p->F = F; p->Fp = Fp; p->D = D;
    const double inv_e = 1.0 / c.spec_abs_exponent;
    p->pmode = c.spec_abs_exponent == 1.0 ? adf::kIstftPowOne : std::fabs(inv_e - 2.0) < 1e-12 ? adf::kIstftPowTwo
             : std::fabs(inv_e - 5.0) < 1e-12 ? adf::kIstftPowFive : adf::kIstftPowGeneral;
    p->pexp = (float)(inv_e - 1.0);
    p->factor = (float)c.spec_factor;

    std::vector<float> basis((size_t)2 * M * F), wsq(M);
    istft_tables(c, window, basis.data(), wsq.data());
    // fragment order (IstftArgs::apack); bins past F are the zero columns that pad K
    std::vector<float> pack((size_t)D * MT * NCH * 8 * 64 * 4);
    size_t o = 0;
    for (int d = 0; d < D; ++d)
        for (int mt = 0; mt < MT; ++mt)
            for (int ch = 0; ch < NCH; ++ch)
                for (int comp = 0; comp < 2; ++comp)
                    for (int sg = 0; sg < 4; ++sg)
                        for (int lane = 0; lane < 64; ++lane)
                            for (int q = 0; q < 4; ++q) {
                                const int m = d * h + mt * 32 + (lane & 31);
                                const int k = ch * KC + 8 * sg + 2 * q + (lane >> 5);
                                pack[o++] = k < F ? basis[((size_t)comp * M + m) * F + k] : 0.f;
                            }
    if (hipMalloc((void**)&p->apack, pack.size() * 4) != hipSuccess || hipMalloc((void**)&p->wsq, (size_t)M * 4) != hipSuccess ||
        hipMemcpy(p->apack, pack.data(), pack.size() * 4, hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(p->wsq, wsq.data(), (size_t)M * 4, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        adf_istft_destroy(p.release());
        return istft_fail("adf_istft_create: device allocation or copy of the basis tables failed");
    }
    *out = p.release();
    return 0;
}

int adf_istft_run(adf_istft_plan* plan, const float* spec, int B, int T, float* audio, int64_t audio_len, void* stream) {
    if (!plan || !spec || !audio) return istft_fail("adf_istft_run: null argument");
    if (B < 1 || B > 65535) return istft_fail("adf_istft_run: B must be in [1, 65535]");
    if (T < 2) return istft_fail("adf_istft_run: T must be at least 2 (center=True trims half a window at both ends)");
    const int64_t want = (int64_t)plan->h * (T - 1);
    if ((int64_t)plan->h * ((int64_t)T + plan->D) >= (int64_t)1 << 31) return istft_fail("adf_istft_run: T is too large");
    if (audio_len != want) return istft_fail("adf_istft_run: audio_len must be hop_length * (T - 1) = " + std::to_string(want));
    if ((uintptr_t)audio % 16) return istft_fail("adf_istft_run: audio must be 16-byte aligned");
    IstftDeviceScope scope(plan->device);
    if (!scope.ok) return istft_fail("adf_istft_run: could not make the plan's device current");
    adf::IstftArgs a;
    a.spec = spec; a.audio = audio;
    a.apack = (const adf::f32x4_hw_t*)plan->apack; a.wsq = plan->wsq;
    a.B = B; a.T = T; a.F = plan->F; a.h = plan->h; a.D = plan->D; a.half = plan->n_fft / 2; a.audio_len = (int)audio_len;
    a.MT = plan->h / 32; a.NCH = plan->Fp / adf::kIstftKC;
    a.jlo = a.half / a.h;
    a.nj = (a.half + a.audio_len - 1) / a.h - a.jlo + 1;
    a.pmode = plan->pmode; a.pexp = plan->pexp; a.factor = plan->factor;
    const hipError_t e = adf::launch_istft(a, (hipStream_t)stream);
    if (e != hipSuccess) return istft_fail(std::string("adf_istft_run: launch failed: ") + hipGetErrorString(e));
    return 0;
}

void adf_istft_destroy(adf_istft_plan* plan) {
    if (!plan) return;
    {
        IstftDeviceScope scope(plan->device);
        if (plan->apack) (void)hipFree(plan->apack);
        if (plan->wsq) (void)hipFree(plan->wsq);
    }
    delete plan;
}

}  // extern "C"
