// Transposed convs of the up path (Upsample1d, unet1d.py:230-256: ConvTranspose1d k = 2f, stride f) in bf16 throughput mode,
// built like the fused short-level kernels: as a GEMM over the output blocks j = 0 .. L - 1 (block j = output rows j f .. j f + f - 1)
// with two taps and N = f * Cout columns, column n = phase * Cout + co.  A column of the upper phases (phase >= f/2) is output row
// j f + phase - f/2 and reads x[j] (tap 0) and x[j - 1] (tap 1); a column of the lower phases is output row j f + phase + f/2 and reads
// x[j + 1] (tap 0) and x[j] (tap 1): exactly L rows per column, none of them dead.  (As a GEMM over m = 0 .. L with output row m f + phase - f/2 -- the form the
// packed weights and GemmArgs::mrows = L + 1 still describe -- the lower phases sit one row further down, m = j + 1, and row 0 / row L
// are live for one half of the columns each; a wave's 32 columns lie in one phase, so the shift is uniform per wave and every stored
// element is the same MFMA sequence in both forms.)  A persistent 512-thread workgroup stages the raw input rows j0 - 1 .. j0 + TM of
// a tile into LDS once and keeps them for the column passes of that tile it owns, every wave owns 32 columns per pass and reads its
// weight fragments straight from a fragment-major copy in L2 (15 K steps ahead, A fragments one step ahead); the output of a pass
// goes through LDS and leaves as 16-byte stores; GroupNorm statistics by fp64 atomics.
// The plain / weight-stationary kernels ran these six launches at 260-325 TF/s (0.29 ms of a 3.2 ms network pass).
#pragma once
#include "adf_gemm.h"
#include <type_traits>

namespace adf {

#ifdef ADF_UP_TL
// diagnostic build only (tools/build_variant.sh uptl -DADF_UP_TL=256; tools/up_timeline.py): s_memtime stamps of every wave of workgroup 0
// and of one from the middle of the grid in the launch with lin == ADF_UP_TL -- per work item: start, tile staged (barrier passed), weight
// ring requested, K loop done, epilogue in LDS (barrier passed), stores issued, item done (barrier passed); s_memrealtime (100 MHz) at both ends.
constexpr int kUpTlItems = 4, kUpTlStamps = 7, kUpTlWave = 8 + kUpTlItems * kUpTlStamps;
extern __device__ unsigned long long adf_up_tl[2 * 8 * kUpTlWave];
#define ADF_UP_STAMP(k) do { if (tl_on && tl_item < kUpTlItems) tl[tl_item * kUpTlStamps + (k)] = __builtin_amdgcn_s_memtime(); } while (0)
#else
#define ADF_UP_STAMP(k) do { } while (0)
#endif

template <int CIN, int COUT, int F, int MTP>
struct UpCfg {
    static constexpr int N = F * COUT;
    static constexpr int PASSW = N >= 256 ? 256 : N;      // columns per pass
    static constexpr int NPASS = N / PASSW;
    static constexpr int WCOLS = PASSW / 32, WROWS = 8 / WCOLS;
    static constexpr int MT = MTP;                         // 32-row MFMA tiles per wave (1, 2 or 4)
    static constexpr int TM = 32 * MT * WROWS;             // output blocks j per tile
    static constexpr int XROWS = TM + 2;                   // staged input rows: j0 - 1 .. j0 + TM
    static constexpr int PX = CIN * 2 + 16, PO = PASSW * 2 + 16;
    static constexpr int kOfsO = XROWS * PX;
    static constexpr int kOfsB = kOfsO + TM * PO;          // bias [COUT] floats
    static constexpr int kLds = kOfsB + COUT * 4;
    static_assert(COUT % 32 == 0, "a wave's 32 columns lie in one phase");
};

// The tile height of a launch: B samples of L output blocks each, tiles of 32 * mt * wrows blocks (mt = 1, 2, 4), npass column passes per
// tile, one work item per (sample, tile, pass) on at most kUpGrid persistent workgroups.  Fewest rounds of kUpGrid workgroups first, then the
// fewest dead rows (rows of the last tile of a sample past L: they cost MFMAs and epilogue like live ones), then the taller tile (the
// weights are read once per item).
constexpr int kUpGrid = 256;
struct UpTilePlan { int mt, tile_rows, tiles_per_sample, dead_rows; long long items, rounds; };
inline UpTilePlan up_tile_plan(int B, int L, int wrows, int npass) {
    UpTilePlan best{};
    for (int mt = 1; mt <= 4; mt *= 2) {
        UpTilePlan c{};
        c.mt = mt;
        c.tile_rows = 32 * mt * wrows;
        c.tiles_per_sample = (L + c.tile_rows - 1) / c.tile_rows;
        c.dead_rows = c.tiles_per_sample * c.tile_rows - L;                    // per sample and pass
        c.items = (long long)B * c.tiles_per_sample * npass;
        c.rounds = (c.items + kUpGrid - 1) / kUpGrid;
        if (mt == 1 || c.rounds < best.rounds || (c.rounds == best.rounds && c.dead_rows <= best.dead_rows)) best = c;
    }
    return best;
}

// A work item is (sample, tile of j, column pass): the passes of a tile may go to different workgroups (each stages the few input
// rows), so that the short levels -- one tile per sample, 1 MB of weights -- still spread over all CUs; consecutive items of one
// workgroup that are passes of the same tile share its staged rows.
template <int CIN, int COUT, int F, int MTP>
__global__ void __launch_bounds__(512) conv_gemm_up_kernel(const GemmArgs a, int tiles_total, int tiles_per_sample) {
    typedef UpCfg<CIN, COUT, F, MTP> Cfg;
    constexpr int MT = Cfg::MT, TM = Cfg::TM, XROWS = Cfg::XROWS, PX = Cfg::PX, PO = Cfg::PO, PASSW = Cfg::PASSW, WCOLS = Cfg::WCOLS;
    constexpr int KS = (CIN / 64) * 2 * 4;                 // K steps of 16 channels: chunks x 2 taps x 4
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* const bufX = smem;                               // [TM + 2][PX]: input positions j0 - 1 .. j0 + TM (zeros outside the sample)
    char* const bufO = smem + Cfg::kOfsO;                  // [TM][PO]: one pass of output columns
    float* const bias = (float*)(smem + Cfg::kOfsB);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r = lane & 31, hh = lane >> 5;
    const int wc = wave % WCOLS, wr = wave / WCOLS;
    const int rowbase = wr * 32 * MT;
    const GemmSeg& sg = a.seg[0];
    const int L = a.lin;
    const bf16_t* const src = (const bf16_t*)sg.src0;
    for (int n = tid; n < COUT; n += 512) bias[n] = a.bias0 ? a.bias0[n] : 0.f;
    auto row_of = [&](int i, int e) __attribute__((always_inline)) -> int { return rowbase + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh; };

    const int nblk = (int)gridDim.x, bidx = (int)blockIdx.x;
#ifdef ADF_UP_TL
    const bool tl_on = L == (ADF_UP_TL) && (bidx == 0 || bidx == nblk / 2 + 3);
    unsigned long long tl[kUpTlItems * kUpTlStamps] = {};
    int tl_item = 0;
    const unsigned long long tl_real0 = tl_on ? __builtin_amdgcn_s_memrealtime() : 0ull;
#endif
    const int t_lo = (int)((long long)bidx * tiles_total / nblk), t_hi = (int)((long long)(bidx + 1) * tiles_total / nblk);
    int staged = -1;                                       // the tile in bufX
    for (int tt = t_lo; tt < t_hi; ++tt) {
        const int t = tt / Cfg::NPASS, pass = tt - t * Cfg::NPASS;
        const int b = t / tiles_per_sample, j0 = (t - b * tiles_per_sample) * TM;
        ADF_UP_STAMP(0);
        // (the barrier that ends an item has taken the previous pass out of bufX / bufO; another pass of the tile in bufX needs no staging)
        if (t != staged) {
            staged = t;
            constexpr int CPR = CIN / 8;
            // the pieces of a thread are loaded four at a time (unconditionally, rows outside the sample on a clamped address) before their LDS stores:
            // as load -> store per trip under a condition these were XROWS CPR / 512 serialised memory round trips per tile (four at a time: the
            // weight-fragment ring is live here, eight would spill)
            constexpr int XS = (XROWS * CPR + 511) / 512, XG = 4;
#pragma unroll
            for (int g0 = 0; g0 < XS; g0 += XG) {
                u32x4_t xs[XG];
#pragma unroll
                for (int k = 0; k < XG; ++k) {
                    const int idx = tid + (g0 + k) * 512;
                    const int row = idx < XROWS * CPR ? idx / CPR : 0, cc = idx % CPR;
                    const int p = j0 - 1 + row;
                    const int pc = p < 0 ? 0 : (p < L ? p : L - 1);
                    xs[k] = *(const u32x4_t*)(src + ((size_t)b * L + pc) * CIN + cc * 8);
                }
#pragma unroll
                for (int k = 0; k < XG; ++k) {
                    const int idx = tid + (g0 + k) * 512;
                    if (g0 + k >= XS || idx >= XROWS * CPR) continue;
                    const int row = idx / CPR, cc = idx % CPR;
                    const int p = j0 - 1 + row;
                    *(u32x4_t*)(bufX + row * PX + cc * 16) = (p >= 0 && p < L) ? xs[k] : u32x4_t{0u, 0u, 0u, 0u};
                }
            }
            __syncthreads();
        }
        ADF_UP_STAMP(1);
        {
            const int col = pass * PASSW + wc * 32 + r;     // this lane's column n
            // the wave's phase: the lower phases (sh = 1) read one staged row further down and store f/2 rows further down
            const int wphase = (pass * PASSW + wc * 32) / COUT;
            const int sh = wphase < F / 2 ? 1 : 0;
            f32x16_t acc[MT];
#pragma unroll
            for (int i = 0; i < MT; ++i)
#pragma unroll
                for (int e = 0; e < 16; ++e) acc[i][e] = 0.f;
            {
                const char* const wl = (const char*)sg.wfrag + ((size_t)hh * a.n_pad + col) * 16;
                auto wfrag = [&](int ks) __attribute__((always_inline)) -> bf16x8_t {
                    return __builtin_bit_cast(bf16x8_t, *(const u32x4_t*)(wl + (size_t)ks * 2 * a.n_pad * 16));
                };
                constexpr int DEPTH = 15 < KS ? 15 : KS, RING = DEPTH + 1;
                static_assert(RING % 2 == 0 && KS >= DEPTH, "ring");
                bf16x8_t wf[RING];
#pragma unroll
                for (int d = 0; d < DEPTH; ++d) wf[d] = wfrag(d);
                __builtin_amdgcn_sched_barrier(0);
                ADF_UP_STAMP(2);
                // K step ks = (chunk * 2 + tap) * 4 + q: tap t of block j reads x[j + sh - t] = staged row (j - j0) + 1 + sh - t
                auto afrag = [&](int ks, bf16x8_t (&af)[MT]) __attribute__((always_inline)) {
                    const int ct = ks >> 2, q = ks & 3;
                    const int chunk = ct >> 1, tap = ct & 1;
#pragma unroll
                    for (int i = 0; i < MT; ++i)
                        af[i] = *(const bf16x8_t*)(bufX + (rowbase + i * 32 + r + 1 + sh - tap) * PX + chunk * 128 + q * 32 + hh * 16);
                };
                bf16x8_t af[2][MT];
                afrag(0, af[0]);
#pragma unroll 1
                for (int kb = 0; kb < KS; kb += RING) {
#pragma unroll
                    for (int u = 0; u < RING; ++u) {
                        const int ks = kb + u;
                        if (ks < KS) {
                            if (ks + DEPTH < KS) wf[(u + DEPTH) % RING] = wfrag(ks + DEPTH);
                            if (ks + 1 < KS) afrag(ks + 1, af[(u + 1) & 1]);
                            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                            for (int i = 0; i < MT; ++i) acc[i] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[u & 1][i], wf[u], acc[i], 0, 0, 0);
                        }
                    }
                }
            }
            ADF_UP_STAMP(3);
            // epilogue of the pass: + bias, statistics over the blocks that exist, bf16 -> bufO
            {
                const int co = col - wphase * COUT;
                const float bv = bias[co];
                float s1 = 0.f, s2 = 0.f;
#pragma unroll
                for (int i = 0; i < MT; ++i)
#pragma unroll
                    for (int e = 0; e < 16; ++e) {
                        const int row = row_of(i, e);
                        const unsigned short qv = f32_to_bf16_hw(acc[i][e] + bv);
                        const float v = bf16_to_f32(qv);                 // statistics of the stored values (adf_common.h pack16_stored)
                        if (j0 + row < L) { s1 += v; s2 = fmaf(v, v, s2); }
                        *(unsigned short*)(bufO + row * PO + (wc * 32 + r) * 2) = qv;
                    }
                if (a.stats) {
                    constexpr int GS = COUT / 8;           // channels per group (8, 16 or 32): the wave's 32 columns hold 32 / GS groups
                    s1 += __shfl_xor(s1, 32, 64); s2 += __shfl_xor(s2, 32, 64);
#pragma unroll
                    for (int o = GS / 2; o > 0; o >>= 1) { s1 += __shfl_xor(s1, o, 64); s2 += __shfl_xor(s2, o, 64); }
                    if (lane < 32 && (lane % GS) == 0) {
                        double* sp = a.stats + ((size_t)b * 8 + co / GS) * 2;
                        atomicAdd(sp, (double)s1);
                        atomicAdd(sp + 1, (double)s2);
                    }
                }
            }
            __syncthreads();
            ADF_UP_STAMP(4);
            // blocks of the pass -> global: (j, local phase) -> output row, COUT channels = COUT / 8 chunks of 16 bytes
            {
                constexpr int PPP = PASSW / COUT;            // phases per pass
                constexpr int CPO = COUT / 8;
                bf16_t* const ob = (bf16_t*)a.out + (size_t)b * a.out_rows * COUT;
                const int live = L - j0 < TM ? L - j0 : TM;  // blocks of the tile inside the sample
                for (int idx = tid; idx < live * PPP * CPO; idx += 512) {
                    const int cc = idx % CPO, rp = idx / CPO;
                    const int pl = rp % PPP, row = rp / PPP;
                    const int phase = pass * PPP + pl;
                    const int orow = (j0 + row) * F + phase + (phase < F / 2 ? F / 2 : -(F / 2));
                    *(u32x4_t*)(ob + (size_t)orow * COUT + cc * 8) = *(const u32x4_t*)(bufO + row * PO + (pl * COUT + cc * 8) * 2);
                }
            }
            ADF_UP_STAMP(5);
            __syncthreads();
            ADF_UP_STAMP(6);
        }
#ifdef ADF_UP_TL
        ++tl_item;
#endif
    }
#ifdef ADF_UP_TL
    if (tl_on && lane == 0) {
        unsigned long long* const o = adf_up_tl + ((bidx == 0 ? 0 : 1) * 8 + wave) * kUpTlWave;
        o[0] = tl_real0; o[1] = __builtin_amdgcn_s_memrealtime(); o[2] = (unsigned long long)(t_hi - t_lo); o[3] = (unsigned long long)t_lo;
        for (int k = 0; k < kUpTlItems * kUpTlStamps; ++k) o[8 + k] = tl[k];
    }
#endif
}

}  // namespace adf
