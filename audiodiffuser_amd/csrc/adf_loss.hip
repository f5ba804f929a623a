// Kernels of adf_diffusion_loss (adf_loss.h): the noising in front of the denoiser and the weighted per-sample squared error behind it.
// Both are memory-bound passes over [B][N] rows that are only 4-byte aligned: 16-byte accesses on the aligned body of every row, scalar head
// and tail.  The reduction is the store-and-sum form (a double per block, then one sum per sample in index order): no atomics, so a loss
// repeats bit for bit, and the chunk length is a constant of the source, so it does not depend on the device either.
#include "adf_loss.h"

// Every fp32 operation below is rounded on its own, as the reference's separate tensor ops round.  hipcc's default is -ffp-contract=fast, and under
// it the __fmul_rn / __fadd_rn intrinsics are an ordinary product and sum that the back end fuses like any other (the mix compiled to v_pk_fma_f32):
// contraction is switched off for this file here, and again on its command line (build.py EXTRA_FLAGS), which also reaches inlined header code.
#pragma clang fp contract(off)

namespace adf {

#define ADF_LOSS_LAUNCH_CHECK(name) (hipGetLastError() == hipSuccess ? nullptr : name ": launch failed")

namespace {

constexpr int kVecPerChunk = kLossChunk / 4;
static_assert(kLossChunk == kLossThreads * 16, "a thread takes four 16-byte vectors of its block's chunk");

// the part of row b that block c walks (adf_loss.h "Row geometry")
struct RowPart {
    long long head, nv;     // scalar elements in front of the aligned body; 16-byte vectors of the body
    int tail;               // scalar elements behind it
    long long v0, v1;       // this block's vectors [v0, v1) of the body
    long long e0, e1;       // no common phase: this block's elements [e0, e1) of the row, one by one
};

__device__ __forceinline__ RowPart row_part(int phase, long long base, long long N, int c) {
    RowPart r{0, 0, 0, 0, 0, 0, 0};
    if (phase < 0) {
        r.e0 = (long long)c * kLossChunk;
        r.e1 = r.e0 + kLossChunk < N ? r.e0 + kLossChunk : N;
        return r;
    }
    const long long mis = (4 - (((long long)phase + base) & 3)) & 3;
    r.head = mis < N ? mis : N;
    r.nv = (N - r.head) >> 2;
    r.tail = (int)(N - r.head - 4 * r.nv);
    r.v0 = (long long)c * kVecPerChunk;
    r.v1 = r.v0 + kVecPerChunk < r.nv ? r.v0 + kVecPerChunk : r.nv;
    return r;
}

// index of the head / tail element thread t of block 0 takes, or -1: threads 0 .. head - 1 the head, threads 64 .. 64 + tail - 1 the tail
__device__ __forceinline__ long long edge_element(const RowPart& r, int c, int t) {
    if (c != 0) return -1;
    if (t < r.head) return t;
    if (t >= 64 && t - 64 < r.tail) return r.head + 4 * r.nv + (t - 64);
    return -1;
}

// every operation rounded to fp32 on its own, as the reference's separate tensor ops round (x + s * noise; (1 - t) * x + t * z1)
__device__ __forceinline__ float mix_1(float x, float z, float s, float one_minus, int rf) {
    const float sz = s * z;
    if (!rf) return x + sz;
    const float ax = one_minus * x;
    return ax + sz;
}

// fl(d d) of one element, widened: d = fl(pred - x), or for the velocity loss fl(fl(noise - x) - pred) (z1 - x - vtheta, left to right)
__device__ __forceinline__ double sq_1(float p, float x, float z, int rf) {
    const float d = rf ? (z - x) - p : p - x;
    const float sq = d * d;
    return (double)sq;
}

}  // namespace

__global__ void __launch_bounds__(kLossThreads) loss_mix_kernel(float* __restrict__ out, const float* __restrict__ x, const float* __restrict__ noise,
                                                                const float* __restrict__ coef, int rf, int phase, long long N) {
    const int c = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const long long base = (long long)b * N;
    const float s = coef[b];
    const float om = 1.0f - s;
    const RowPart r = row_part(phase, base, N, c);
    const float* xr = x + base;
    const float* zr = noise + base;
    float* orow = out + base;
    for (long long v = r.v0 + t; v < r.v1; v += kLossThreads) {
        const long long i = r.head + 4 * v;
        const float4 a = *reinterpret_cast<const float4*>(xr + i), z = *reinterpret_cast<const float4*>(zr + i);
        *reinterpret_cast<float4*>(orow + i) = make_float4(mix_1(a.x, z.x, s, om, rf), mix_1(a.y, z.y, s, om, rf), mix_1(a.z, z.z, s, om, rf),
                                                           mix_1(a.w, z.w, s, om, rf));
    }
    const long long e = edge_element(r, c, t);
    if (e >= 0) orow[e] = mix_1(xr[e], zr[e], s, om, rf);
    for (long long i = r.e0 + t; i < r.e1; i += kLossThreads) orow[i] = mix_1(xr[i], zr[i], s, om, rf);
}

__global__ void __launch_bounds__(kLossThreads) loss_partial_kernel(double* __restrict__ partial, const float* __restrict__ pred, const float* __restrict__ x,
                                                                    const float* __restrict__ noise, int phase, long long N) {
    const int c = blockIdx.x, b = blockIdx.y, t = threadIdx.x;
    const long long base = (long long)b * N;
    const int rf = noise != nullptr;
    const RowPart r = row_part(phase, base, N, c);
    const float* pr = pred + base;
    const float* xr = x + base;
    const float* zr = rf ? noise + base : xr;           // (read and ignored for the x0 kinds' scalar elements; never read as a vector there)
    double acc = 0.0;
    for (long long v = r.v0 + t; v < r.v1; v += kLossThreads) {
        const long long i = r.head + 4 * v;
        const float4 p = *reinterpret_cast<const float4*>(pr + i), a = *reinterpret_cast<const float4*>(xr + i);
        const float4 z = rf ? *reinterpret_cast<const float4*>(zr + i) : a;
        acc += sq_1(p.x, a.x, z.x, rf);
        acc += sq_1(p.y, a.y, z.y, rf);
        acc += sq_1(p.z, a.z, z.z, rf);
        acc += sq_1(p.w, a.w, z.w, rf);
    }
    const long long e = edge_element(r, c, t);
    if (e >= 0) acc += sq_1(pr[e], xr[e], zr[e], rf);
    for (long long i = r.e0 + t; i < r.e1; i += kLossThreads) acc += sq_1(pr[i], xr[i], zr[i], rf);
    // fixed order: the halving tree inside each wave, then the four waves in index order
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    __shared__ double wave_sum[kLossThreads / 64];
    if ((t & 63) == 0) wave_sum[t >> 6] = acc;
    __syncthreads();
    if (t == 0) {
        double sum = wave_sum[0];
        for (int w = 1; w < kLossThreads / 64; ++w) sum += wave_sum[w];
        partial[(long long)b * gridDim.x + c] = sum;
    }
}

__global__ void __launch_bounds__(64) loss_finalize_kernel(float* __restrict__ losses, const double* __restrict__ partial, const float* __restrict__ sigmas,
                                                           int kind, float sigma_data, int chunks, int B, long long N) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    double sum = 0.0;
    for (int c = 0; c < chunks; ++c) sum += partial[(long long)b * chunks + c];
    const double s = (double)sigmas[b], sd = (double)sigma_data;
    double w = 1.0;
    if (kind == kLossX0Edm) w = (s * s + sd * sd) / ((s * sd) * (s * sd));
    else if (kind == kLossX0InvSigma2) w = 1.0 / (s * s);
    losses[b] = (float)(w / (double)N * sum);
}

// (address / 4) % 4 of the pointers when they agree (null pointers aside), else -1
static int common_phase(const void* a, const void* b, const void* c) {
    int phase = -1;
    for (const void* p : {a, b, c}) {
        if (!p) continue;
        const int ph = (int)(((uintptr_t)p >> 2) & 3);
        if (phase >= 0 && ph != phase) return -1;
        phase = ph;
    }
    return phase;
}

static const char* loss_shape_error(int B, long long N) {
    if (B < 1 || B > 65535) return "loss: the batch size must be in [1, 65535]";
    if (N < 1 || N > ((long long)1 << 40)) return "loss: bad number of elements per sample";
    return nullptr;
}

const char* launch_loss_mix(float* x_noisy, const float* x, const float* noise, const float* coef_dev, int rf, int B, long long N, hipStream_t s) {
    if (const char* e = loss_shape_error(B, N)) return e;
    if (!x_noisy || !x || !noise || !coef_dev || x_noisy == x || x_noisy == noise) return "loss_mix: bad arguments (the output must not alias an input)";
    hipLaunchKernelGGL(loss_mix_kernel, dim3(loss_chunks(N), B), dim3(kLossThreads), 0, s, x_noisy, x, noise, coef_dev, rf, common_phase(x_noisy, x, noise), N);
    return ADF_LOSS_LAUNCH_CHECK("loss_mix");
}

const char* launch_loss_partial(double* partial, const float* pred, const float* x, const float* noise, int B, long long N, hipStream_t s) {
    if (const char* e = loss_shape_error(B, N)) return e;
    if (!partial || !pred || !x) return "loss_partial: bad arguments";
    hipLaunchKernelGGL(loss_partial_kernel, dim3(loss_chunks(N), B), dim3(kLossThreads), 0, s, partial, pred, x, noise, common_phase(pred, x, noise), N);
    return ADF_LOSS_LAUNCH_CHECK("loss_partial");
}

const char* launch_loss_finalize(float* losses, const double* partial, const float* sigmas_dev, int kind, float sigma_data, int B, long long N,
                                 hipStream_t s) {
    if (const char* e = loss_shape_error(B, N)) return e;
    if (!losses || !partial || !sigmas_dev || kind < kLossX0Edm || kind > kLossRf) return "loss_finalize: bad arguments";
    hipLaunchKernelGGL(loss_finalize_kernel, dim3((B + 63) / 64), dim3(64), 0, s, losses, partial, sigmas_dev, kind, sigma_data, loss_chunks(N), B, N);
    return ADF_LOSS_LAUNCH_CHECK("loss_finalize");
}

}  // namespace adf
