// Tile-shape dispatch for the fused implicit-GEMM kernel (see adf_gemm.h).
#include "adf_gemm.h"
#include "adf_gemm_pp.h"
#include "adf_gemm_rb.h"
#include "adf_gemm_rbx3.h"
#include "adf_gemm_up.h"
#include "adf_kernels.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>


#ifdef ADF_RB_STAMP
namespace adf { __device__ unsigned long long adf_rb_stamps[8 * 16]; }
extern "C" int adf_debug_rb_stamps(unsigned long long* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(adf::adf_rb_stamps), sizeof(unsigned long long) * 8 * 16);
}
#endif

#ifdef ADF_RB_TL
namespace adf { __device__ unsigned adf_rb_tl[2 * 8 * 128]; }
extern "C" int adf_debug_rb_timeline(unsigned* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(adf::adf_rb_tl), sizeof(unsigned) * 2 * 8 * 128);
}
#endif

#ifdef ADF_UP_TL
namespace adf { __device__ unsigned long long adf_up_tl[2 * 8 * kUpTlWave]; }
extern "C" int adf_debug_up_timeline(unsigned long long* out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(adf::adf_up_tl), sizeof(unsigned long long) * 2 * 8 * adf::kUpTlWave);
}
#endif

namespace adf {

namespace {

// ---- the launch step of each kernel: grid arithmetic and the launch, no decision -----------------------------------------------------------------
template <typename T, int MT, int NT, int WM, int WN>
const char* launch_variant(const GemmArgs& a, hipStream_t stream) {
    constexpr int TM = 32 * MT * WM, TN = 32 * NT * WN, NTHR = 64 * WM * WN;
    constexpr int lds = gemm_lds_bytes<TM, TN>();
    if (!raise_lds_limit<lds, conv_gemm_kernel<T, MT, NT, WM, WN>>()) return "hipFuncSetAttribute(MaxDynamicSharedMemorySize) failed";
    const int tiles_n = (a.n_pad + TN - 1) / TN;
    const long long tiles_m = a.flat ? ((long long)a.B * a.mrows + TM - 1) / TM : (long long)((a.mrows + TM - 1) / TM) * a.B;
    const long long blocks = (long long)tiles_n * tiles_m;
    if (blocks <= 0 || blocks > 0x7fffffffLL) return "conv_gemm: bad grid";
    hipLaunchKernelGGL((conv_gemm_kernel<T, MT, NT, WM, WN>), dim3((unsigned)blocks), dim3(NTHR), lds, stream, a);
    return hipGetLastError() == hipSuccess ? nullptr : "conv_gemm: launch failed";
}

// Weight-stationary warp-specialised kernel (adf_gemm.h): persistent 512-thread blocks, one per CU.
int ws_lds_bytes(const GemmArgs& a, int tn) {
    long long wrows = 0;
    for (int s = 0; s < a.nseg; ++s) wrows += (long long)a.seg[s].nchunk * a.seg[s].taps * tn;
    const long long b = wrows * kLdsPitch + 2LL * kWsARows * kLdsPitch + kWsScratch;
    return b > 0x7fffffff ? 0x7fffffff : (int)b;
}

template <typename T, int NT, int WN>
const char* launch_ws_variant(const GemmArgs& a, hipStream_t stream) {
    constexpr int TN = NT * WN * 32;
    if (!raise_lds_limit<160 * 1024, conv_gemm_ws_kernel<T, NT, WN>>()) return "hipFuncSetAttribute(MaxDynamicSharedMemorySize, ws) failed";
    const int tiles_n = (a.n_pad + TN - 1) / TN;
    const long long tiles_m_total = (long long)((a.mrows + 127) / 128) * a.B;
    if (tiles_m_total <= 0 || tiles_m_total > 0x7fffffffLL) return "conv_gemm_ws: bad tile count";
    long long bpn = device_cus() / tiles_n;
    if (bpn < 1) bpn = 1;
    if (bpn > tiles_m_total) bpn = tiles_m_total;
    hipLaunchKernelGGL((conv_gemm_ws_kernel<T, NT, WN>), dim3((unsigned)(bpn * tiles_n)), dim3(512), (size_t)ws_lds_bytes(a, TN), stream, a, (int)tiles_m_total,
                       (int)bpn);
    return hipGetLastError() == hipSuccess ? nullptr : "conv_gemm_ws: launch failed";
}

// Transposed-conv kernel (adf_gemm_up.h): persistent 512-thread workgroups over tiles of the output blocks j = 0 .. L - 1 (a.lin of them per
// sample; a.mrows = L + 1 is the row count of the m-indexed form the route decision and the trace line speak of)
template <int CIN, int COUT, int F, int MTP>
const char* launch_up_mt(const GemmArgs& a, const UpTilePlan& tp, hipStream_t stream) {
    typedef UpCfg<CIN, COUT, F, MTP> Cfg;
    if (!raise_lds_limit<160 * 1024, conv_gemm_up_kernel<CIN, COUT, F, MTP>>()) return "hipFuncSetAttribute(MaxDynamicSharedMemorySize, up) failed";
    static_assert(Cfg::kLds <= 160 * 1024, "up kernel LDS budget");
    if (tp.tile_rows != Cfg::TM || tp.items <= 0 || tp.items > 0x7fffffffLL) return "conv_gemm_up: bad tile count";
    const long long grid = tp.items < kUpGrid ? tp.items : kUpGrid;
    hipLaunchKernelGGL((conv_gemm_up_kernel<CIN, COUT, F, MTP>), dim3((unsigned)grid), dim3(512), Cfg::kLds, stream, a, (int)tp.items, tp.tiles_per_sample);
    return hipGetLastError() == hipSuccess ? nullptr : "conv_gemm_up: launch failed";
}
// tile height: up_tile_plan (adf_gemm_up.h)
template <int CIN, int COUT, int F>
const char* launch_up(const GemmArgs& a, hipStream_t stream) {
    typedef UpCfg<CIN, COUT, F, 1> C1;
    if (a.lin < 1) return "conv_gemm_up: bad tile count";
    const UpTilePlan tp = up_tile_plan(a.B, a.lin, C1::WROWS, C1::NPASS);
    if (tp.mt == 1) return launch_up_mt<CIN, COUT, F, 1>(a, tp, stream);
    if (tp.mt == 2) return launch_up_mt<CIN, COUT, F, 2>(a, tp, stream);
    return launch_up_mt<CIN, COUT, F, 4>(a, tp, stream);
}

// Persistent LDS-DMA kernel (adf_gemm_pp.h): one 512-thread block per CU, block tile (128 MT) x 128.
template <int MT>
const char* launch_pp(const GemmArgs& a, hipStream_t stream) {
    if (!raise_lds_limit<kPpLds, conv_gemm_pp_kernel<MT>>()) return "hipFuncSetAttribute(MaxDynamicSharedMemorySize, pp) failed";
    constexpr int TM = 128 * MT;
    const int tiles_m = a.mrows / TM, tiles_n = a.n_pad / kPpTN;
    int tm_shift = 0;
    while ((1 << tm_shift) < tiles_m) ++tm_shift;
    const long long tiles_total = (long long)a.B * tiles_m * tiles_n;
    if (tiles_total <= 0 || tiles_total > (1 << 22)) return "conv_gemm_pp: bad tile count";
    const long long grid = tiles_total < device_cus() ? tiles_total : device_cus();
    hipLaunchKernelGGL(conv_gemm_pp_kernel<MT>, dim3((unsigned)grid), dim3(512), kPpLds, stream, a, (int)tiles_total, tm_shift, tiles_n);
    return hipGetLastError() == hipSuccess ? nullptr : "conv_gemm_pp: launch failed";
}

// can an epilogue reduce GroupNorm statistics over `channels` output channels in `groups` groups?  The group size has to be a power of two between
// `lo` and `hi` channels: what one thread stores at least, what one wave (or tile) covers at most -- each route has its own two bounds.
bool stats_groups_ok(int channels, int groups, int lo, int hi) {
    const int gs = groups > 0 ? channels / groups : 0;
    return gs > 0 && gs * groups == channels && (gs & (gs - 1)) == 0 && gs >= lo && gs <= hi;
}
bool pow2(int v) { return v > 0 && (v & (v - 1)) == 0; }

// What the two forms of the resblock conv kernel (adf_gemm_rb.h: bf16 rows, 64-channel K blocks; adf_gemm_rbx3.h: fp32 rows, 32-channel K blocks) share on the
// host: the shape checks, the tile shape, the K-block table of one tile and the argument head -- everything but the kernels themselves.
struct RbForm {
    int esz;            // bytes per stored element
    int blk_ch;         // channels of a K block (a 128-byte row)
    int max_blk;        // blocks of the argument table
    bool even_pairs;    // bf16 form: an even number of 64-channel blocks per tile (the ring parity of the first block of a tile is a compile-time constant)
    bool wide_n;        // bf16 form: a workgroup tile may span both 128-column halves of n = 256; the fp32 form has one 128-column N tile per workgroup tile
};
constexpr RbForm kRbBf16 = {2, 64, kRbMaxBlk, true, true}, kRbX3 = {4, 32, kRbx3MaxBlk, false, false};

// segment 0 of the resblock conv kernel: GroupNorm + SiLU with the table derived in the kernel, or raw (the folded down convs, the 3-tap form of a transposed conv)
bool rb_raw0(const GemmArgs& a) { return !a.seg[0].gn.gamma && !a.seg[0].ab && !a.seg[0].act && a.seg[0].c1 == 0; }

// false: not a shape the kernel is written for.  (Per-sample tiles only: the callers rule out flat tiles.  A GroupNorm on segment 1 is ignored by every route.)
bool rb_shape_ok(const GemmArgs& a, const RbForm& f, bool with_stats) {
    const GemmSeg& g0 = a.seg[0];
    if (a.scatter_f || a.gelu || a.mrows % 128 || a.lin != a.mrows || a.out_rows != a.mrows) return false;
    if (a.n != a.n_pad || a.out_c != a.n || (a.n != 128 && a.n != 256) || a.bias_mod != a.n) return false;
    if (!pow2(a.mrows / 128)) return false;
    const bool raw0 = rb_raw0(a);
    if (!raw0 && (!g0.gn.gamma || !g0.act)) return false;
    if (g0.taps != 3 || g0.off0 != -1 || g0.stride != 1 || g0.step != 1) return false;
    auto seg_ok = [&](int c0, int c1, int nb_before) {
        if (c0 % 64 || c1 % 64 || nb_before + (c0 + c1) / f.blk_ch > f.max_blk) return false;
        return !(f.even_pairs && ((c0 + c1) / 64) % 2);
    };
    if (!seg_ok(g0.c0, g0.c1, 0)) return false;
    if (!raw0 && g0.c0 + g0.c1 > kPpMaxCin) return false;
    if (!raw0) {
        // the kernel's table fill sums one or two stored (fine) statistics groups per GroupNorm group: one source, or two equal ones
        const GnFinalizeArgs& gn = g0.gn;
        if (gn.G < 1 || (gn.c0 + gn.c1) % gn.G || gn.c0 % gn.G || gn.c1 % gn.G) return false;
        const int gs = (gn.c0 + gn.c1) / gn.G;
        if (gn.c0 % gs) return false;                                       // a group must not straddle the two sources
        for (int cs : {gn.c0, gn.c1}) {
            if (cs == 0) continue;
            const int fg = cs / gn.G;
            if (gs != fg && gs != 2 * fg) return false;
        }
    }
    if (raw0 && (a.nseg > 1 || a.res)) return false;
    if (a.res && a.nseg > 1) return false;
    if (a.nseg > 1) {
        const GemmSeg& g1 = a.seg[1];
        if (g1.taps != 1 || g1.off0 != 0 || g1.stride != 1 || g1.step != 1 || g1.ab || g1.act) return false;
        if (!seg_ok(g1.c0, g1.c1, (g0.c0 + g0.c1) / f.blk_ch)) return false;
    }
    if (a.phase_c && (!raw0 || (a.phase_c & (a.phase_c - 1)) || a.phase_c < 64 || a.n % a.phase_c)) return false;
    // the channels the statistics are over: the phase_c channels of a 3-tap-form transposed conv, else all columns
    return !(with_stats && a.stats) || stats_groups_ok(a.phase_c ? a.phase_c : a.out_c, a.stats_groups, 8, 64);
}

// Tile shape.  n = 256 (bf16 form): one 256 x 256 tile per 256 rows (the activations are fetched and activated once) when that still gives
// every CU a tile, else two 256 x 128 tiles; when even those leave CUs idle (L = 256 at batch 64), 128-row tiles.  (128 x 256 tiles there --
// half as many thread blocks, each activation prepared once -- measured equal, 247.1 against 247.4 ms per step, and are not built.)
struct RbTiles { int tm, nh; long long total; };
// false: fewer tiles than `min_tiles` (CUs) even on 128-row tiles -- the other routes
bool rb_tiles(const GemmArgs& a, const RbForm& f, long long min_tiles, RbTiles& t) {
    t = RbTiles{256, 1, 0};
    auto at = [&](int tm) -> long long {       // thread-block tiles at tile height tm (0: the rows do not divide)
        if (a.mrows % tm || !pow2(a.mrows / tm)) return 0;
        const long long tiles_m = (long long)a.B * (a.mrows / tm);
        t.tm = tm;
        t.nh = (f.wide_n && a.n == 256 && tiles_m >= min_tiles) ? 2 : 1;
        return tiles_m * (a.n / (kPpTN * t.nh));
    };
    t.total = at(256);
    if (t.total < min_tiles) t.total = at(128);
    return t.total <= (1 << 22) && t.total >= min_tiles;
}

// the K-block table of one tile and the argument head, for a shape that rb_shape_ok and rb_tiles accepted.  zskip (bf16 form, raw launches): leave out the
// sub-steps whose weights are zero by construction -- RbHead::nb2 / phase2
template <typename ArgsT>
void rb_fill_args(const GemmArgs& a, const RbForm& f, const RbTiles& t, int zskip, ArgsT& r) {
    const GemmSeg& g0 = a.seg[0];
    memset(&r, 0, sizeof(r));
    int nb = 0;
    auto add_seg = [&](const void* s0, const void* s1, int c0, int c1, const void* w, int taps, bool table, float scale1) {
        for (int c = 0; c < c0 + c1; c += f.blk_ch, ++nb) {
            const bool from1 = c >= c0;
            RbBlk& e = r.blk[nb];
            e.src = (const char*)(from1 ? s1 : s0) + (size_t)(from1 ? c - c0 : c) * f.esz;
            e.pitch = (unsigned)(from1 ? c1 : c0) * (unsigned)f.esz;
            e.w = (const char*)w + (size_t)(c / f.blk_ch) * taps * a.n_pad * kRowBytes;
            e.tab = table ? c * 8 : -1;
            e.scale = from1 ? scale1 : 1.0f;
        }
    };
    add_seg(g0.src0, g0.src1, g0.c0, g0.c1, g0.w, 3, !rb_raw0(a), 1.0f);
    r.h.nb3 = nb;
    if (a.nseg > 1) add_seg(a.seg[1].src0, a.seg[1].src1, a.seg[1].c0, a.seg[1].c1, a.seg[1].w, 1, false, a.seg[1].scale1);
    r.h.res = a.nseg == 1 ? a.res : nullptr;                             // identity residual: added in the epilogue (fp32, before the rounding)
    r.h.nb1 = nb - r.h.nb3;
    if (zskip && rb_raw0(a)) {
        // folded strided conv: tap 2 is zero from folded channel tap2_zero_c on.  Two-tap blocks only behind an even number (the two-stage ring's parity) of at
        // least two (a tile starts with a three-tap block) three-tap blocks; else the table stays as it was
        const int z = g0.tap2_zero_c, nbz = z / f.blk_ch;
        if (!a.phase_c && z > 0 && z % f.blk_ch == 0 && nbz >= 2 && nbz % 2 == 0 && nbz < r.h.nb3) {
            r.h.nb2 = r.h.nb3 - nbz;
            r.h.nb3 = nbz;
        }
        // x2 transposed conv in its 3-tap form: the N halves are the phases
        if (a.phase_c && a.n == 2 * a.phase_c && t.nh == 2) r.h.phase2 = 1;
    }
    r.h.B = a.B; r.h.L = a.mrows;
    r.h.n = a.n;
    r.h.gn = g0.gn;
    r.h.bias0 = a.bias0; r.h.bias1 = a.bias1;
    r.h.out = a.out;
    if (a.stats) {
        r.h.stats = a.stats; r.h.stats_groups = a.stats_groups;
        r.h.stats_mod = a.phase_c;
    }
    r.h.tiles_n = a.n / (kPpTN * t.nh);
    while ((1 << r.h.tm_shift) < a.mrows / t.tm) ++r.h.tm_shift;
    r.h.tiles_total = (int)t.total;
}

// Resblock conv kernel (adf_gemm_rb.h): one 512-thread block per CU.
const char* launch_rb(const GemmArgs& a, long long min_tiles, int zskip, hipStream_t stream) {
    RbTiles t;
    RbArgs r;
    rb_tiles(a, kRbBf16, min_tiles, t);
    rb_fill_args(a, kRbBf16, t, zskip, r);
    if (r.h.nb2 && (r.h.nb3 < 2 || r.h.nb3 % 2 || r.h.nb1)) return "conv_gemm_rb: two-tap blocks need an even number >= 2 of three-tap blocks ahead of them";
    if (!raise_lds_limit<kRbLds, conv_gemm_rb_kernel<1, false, 2>, conv_gemm_rb_kernel<2, false, 2>, conv_gemm_rb_kernel<1, true, 2>, conv_gemm_rb_kernel<2, true, 2>,
                         conv_gemm_rb_kernel<1, false, 1>, conv_gemm_rb_kernel<2, false, 1>, conv_gemm_rb_kernel<1, true, 1>, conv_gemm_rb_kernel<2, true, 1>>())
        return "hipFuncSetAttribute(MaxDynamicSharedMemorySize, rb) failed";
    const long long grid = t.total < device_cus() ? t.total : device_cus();
    const bool raw0 = rb_raw0(a);
    auto go = [&](auto kern) { hipLaunchKernelGGL(kern, dim3((unsigned)grid), dim3(512), kRbLds, stream, r); };
    if (r.h.phase2) {
        if (!raise_lds_limit<kRbLds, conv_gemm_rb_kernel<2, true, 2, true>, conv_gemm_rb_kernel<2, true, 1, true>>())
            return "hipFuncSetAttribute(MaxDynamicSharedMemorySize, rb) failed";
        if (t.tm == 256) go(conv_gemm_rb_kernel<2, true, 2, true>);
        else go(conv_gemm_rb_kernel<2, true, 1, true>);
    } else if (t.tm == 256) {
        if (t.nh == 2 && raw0) go(conv_gemm_rb_kernel<2, true, 2>);
        else if (t.nh == 2) go(conv_gemm_rb_kernel<2, false, 2>);
        else if (raw0) go(conv_gemm_rb_kernel<1, true, 2>);
        else go(conv_gemm_rb_kernel<1, false, 2>);
    } else {
        if (t.nh == 2 && raw0) go(conv_gemm_rb_kernel<2, true, 1>);
        else if (t.nh == 2) go(conv_gemm_rb_kernel<2, false, 1>);
        else if (raw0) go(conv_gemm_rb_kernel<1, true, 1>);
        else go(conv_gemm_rb_kernel<1, false, 1>);
    }
    return hipGetLastError() == hipSuccess ? nullptr : "conv_gemm_rb: launch failed";
}

// Split-bf16 form of the resblock conv kernel (adf_gemm_rbx3.h): fp32 storage, 32-channel K blocks; the same shapes as launch_rb.
const char* launch_rbx3(const GemmArgs& a, long long min_tiles, hipStream_t stream) {
    RbTiles t;
    Rbx3Args r;
    rb_tiles(a, kRbX3, min_tiles, t);
    rb_fill_args(a, kRbX3, t, 0, r);
    if (!raise_lds_limit<kRbLds, conv_gemm_rbx3_kernel<2>, conv_gemm_rbx3_kernel<1>>()) return "hipFuncSetAttribute(MaxDynamicSharedMemorySize, rbx3) failed";
    const long long grid = t.total < device_cus() ? t.total : device_cus();
    if (t.tm == 256) hipLaunchKernelGGL(conv_gemm_rbx3_kernel<2>, dim3((unsigned)grid), dim3(512), kRbLds, stream, r);
    else hipLaunchKernelGGL(conv_gemm_rbx3_kernel<1>, dim3((unsigned)grid), dim3(512), kRbLds, stream, r);
    return hipGetLastError() == hipSuccess ? nullptr : "conv_gemm_rbx3: launch failed";
}

// shapes the pipelined kernel is written for (see the header of adf_gemm_pp.h); an identity residual counts as a
// second segment
bool pp_eligible(const GemmArgs& a, int tm) {
    if (a.scatter_f || a.mrows % tm || a.lin != a.mrows || a.out_rows != a.mrows) return false;
    if (a.n != a.n_pad || a.out_c != a.n || a.n_pad % kPpTN || a.n_pad > kPpMaxN) return false;
    if (!pow2(a.mrows / tm)) return false;
    if (a.res && a.nseg > 1) return false;
    int nb = a.res ? a.n / 64 : 0;
    for (int s = 0; s < a.nseg; ++s) {
        const GemmSeg& g = a.seg[s];
        if (g.stride != 1 || g.step != 1) return false;
        if (!((g.taps == 3 && g.off0 == -1) || (g.taps == 1 && g.off0 == 0))) return false;
        if (g.c0 % 64 || g.c1 % 64 || (g.ab && g.c0 + g.c1 > kPpMaxCin)) return false;   // the LDS affine table holds kPpMaxCin channels
        if (s == 1 && (g.ab || g.act)) return false;
        nb += (g.c0 + g.c1) / 64;
    }
    return nb >= 2;
}

// packed bf16 identity [n/64 chunks][1 tap][n rows][64 channels]: row r of chunk c holds 1.0 at channel r - 64 c
const void* pp_identity(int n, hipStream_t stream, const char** err) {
    static void* cache_dev[kMaxDevices][kPpMaxN / 64 + 1] = {};     // one copy per device (freed at process exit)
    void** cache = cache_dev[current_device()];
    const int idx = n / 64;
    if (cache[idx]) return cache[idx];
    const size_t elems = (size_t)(n / 64 + kTapGroup) * n * 64;     // over-allocated like every packed weight
    std::vector<uint16_t> hbuf(elems, 0);
    for (int r = 0; r < n; ++r) hbuf[((size_t)(r / 64) * n + r) * 64 + (r % 64)] = 0x3F80;
    void* d = nullptr;
    if (hipMalloc(&d, elems * 2) != hipSuccess) { *err = "conv_gemm_pp: hipMalloc(identity) failed"; return nullptr; }
    if (hipMemcpyAsync(d, hbuf.data(), elems * 2, hipMemcpyHostToDevice, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) {
        *err = "conv_gemm_pp: identity upload failed";
        return nullptr;
    }
    cache[idx] = d;
    return d;
}

template <typename T, int MT, int NT>
const char* launch_ksplit(const GemmArgs& a, hipStream_t stream) {
    constexpr int lds = 4 * ks_wave_lds(MT, NT);
    constexpr int TM = 32 * MT, TN = 32 * NT;
    if (!raise_lds_limit<lds, conv_gemm_ksplit_kernel<T, MT, NT>>()) return "hipFuncSetAttribute(MaxDynamicSharedMemorySize, ksplit) failed";
    const int tiles_n = (a.n_pad + TN - 1) / TN;
    const long long tiles_m = a.flat ? ((long long)a.B * a.mrows + TM - 1) / TM : (long long)((a.mrows + TM - 1) / TM) * a.B;
    const long long blocks = tiles_m * tiles_n;
    if (blocks <= 0 || blocks > 0x7fffffffLL) return "conv_gemm_ksplit: bad grid";
    hipLaunchKernelGGL((conv_gemm_ksplit_kernel<T, MT, NT>), dim3((unsigned)blocks), dim3(256), lds, stream, a);
    return hipGetLastError() == hipSuccess ? nullptr : "conv_gemm_ksplit: launch failed";
}

template <typename T>
const char* dispatch(const GemmArgs& a, int tm, int tn, hipStream_t s) {
    if (tm == 128 && tn == 128) return launch_variant<T, 2, 2, 2, 2>(a, s);
    if (tm == 128 && tn == 64) return launch_variant<T, 2, 1, 2, 2>(a, s);
    if (tm == 128 && tn == 32) return launch_variant<T, 1, 1, 4, 1>(a, s);
    if (tm == 64 && tn == 128) return launch_variant<T, 1, 2, 2, 2>(a, s);
    if (tm == 64 && tn == 64) return launch_variant<T, 1, 1, 2, 2>(a, s);
    if (tm == 64 && tn == 32) return launch_variant<T, 1, 1, 2, 1>(a, s);
    if (tm == 32 && tn == 128) return launch_variant<T, 1, 1, 1, 4>(a, s);
    if (tm == 32 && tn == 64) return launch_variant<T, 1, 1, 1, 2>(a, s);
    return launch_variant<T, 1, 1, 1, 1>(a, s);
}

// ---- the route decision ---------------------------------------------------------------------------------------------------------------------------
// Every switch and tuning value of the decision, read once per process.  Route switches come from the environment (the parity tests run both sides of
// each); tuning values are constants in the product build (adf_common.h).
struct GemmSwitches {
    int trace = adf_route_switch("ADF_GEMM_TRACE", 0);      // 1: print the kernel chosen for every launch (stderr)
    int up = adf_route_switch("ADF_GEMM_UP", 1);            // 0: the up-path transposed convs stay with the plain / weight-stationary kernels; 2: all four shapes
    int pp = adf_route_switch("ADF_GEMM_PP", 1);            // 0: off; 2: also identity-residual layers and >= 128 tiles (tests); 3: 256-row tiles only (A/B)
    int ws = adf_route_switch("ADF_GEMM_WS", 1);            // 0: off; 64: also 64-wide N tiles
    // fewest thread-block tiles for the resblock conv kernel's two forms (-1: the route is off).  ADF_GEMM_RB / ADF_GEMM_RBX3 = 0 leaves the layers to
    // the other routes (A/B; the tests compare the two), = 2 takes small batches too (tests)
    long long rb_min_tiles = min_tiles_of(adf_route_switch("ADF_GEMM_RB", 1));
    long long rbx3_min_tiles = min_tiles_of(adf_route_switch("ADF_GEMM_RBX3", 1));
    int rb_zskip = adf_route_switch("ADF_RB_ZSKIP", 1);     // 0: the raw launches of the resblock conv kernel run their structurally zero sub-steps too (A/B; the tests compare the two)
    int gn_in_kernel = (int)adf_tuning("ADF_GEMM_GN", 1);               // 0: always launch gn_finalize (A/B)
    int min_blocks = (int)adf_tuning("ADF_GEMM_MINBLOCKS", 512);        // the generic kernel's tiles shrink until the grid has this many blocks
    int ksplit = (int)adf_tuning("ADF_GEMM_KSPLIT", 1);                 // 0: off; 32: 32 x 32 tiles only
    long long ksplit_rows = adf_tuning("ADF_GEMM_KSPLIT_ROWS", 4096);   // largest B * rows the split-K kernel takes
    int ksplit_minit = (int)adf_tuning("ADF_GEMM_KSPLIT_MINIT", 4);     // fewest 64-channel K chunks (all segments) for which K is split over the waves
    long long ws_min_m = adf_tuning("ADF_GEMM_WS_MINM", 256);           // fewest 128-row tiles for the weight-stationary kernel
    static long long min_tiles_of(int sw) { return sw == 0 ? -1 : (sw >= 2 ? 32 : 256); }
};
const GemmSwitches& switches() {
    static const GemmSwitches s;
    return s;
}

enum class Route { refused, up, ksplit, rbx3, rb, pp, ws, plain };
const char* const kRouteName[] = {"", "up", "ksplit", "rbx3", "rb", "pp", "ws", "plain"};

// What launch_conv_gemm will do with one call; decide_conv_gemm fills it and launches nothing.
struct GemmPlan {
    Route route = Route::refused;
    const char* refusal = nullptr;      // route == refused: why
    int tm = 0, tn = 0;                 // tile height and width as the trace prints them (rb / rbx3: 256 x 128, the kernel's first choice; up: 64 x 256)
    int flat = 0, seg_rows = 0;         // GemmArgs::flat / seg_rows of the launch
    bool stats = false;                 // the requested statistics are reduced in the epilogue (else the caller runs the separate pass)
    bool stats_traced = false;          // the `stats=` of the trace line: `stats`, except that the rb / rbx3 lines of ordinary convs have always printed the
                                        // answer of the generic tile they did not take (tests and documents quote the lines)
    bool gn_in_kernel = false;          // a pending GroupNorm table of segment 0 is derived by the kernel (else gn_finalize is launched first)
    int up_cfg = 0;                     // up: 1 = 256 -> 256 x4, 2 = 256 -> 128 x2, 3 = 128 -> 128 x2, 4 = 128 -> 64 x2
    bool ident_seg = false;             // pp: the identity residual becomes a raw 1-tap K segment against the packed identity
};

// would the resblock conv kernel (the form of this dtype) take it: route on, shape, enough tiles?
bool rb_takes(const GemmArgs& a, bool x3, bool with_stats) {
    const long long min_tiles = x3 ? switches().rbx3_min_tiles : switches().rb_min_tiles;
    const RbForm& f = x3 ? kRbX3 : kRbBf16;
    RbTiles t;
    return min_tiles >= 0 && rb_shape_ok(a, f, with_stats) && rb_tiles(a, f, min_tiles, t);
}

GemmPlan decide_conv_gemm(const GemmArgs& a, int dtype) {
    // dtype: 0 = fp32 storage + exact-fp32 MFMA, 1 = bf16 storage, 2 = fp32 storage + split-bf16 operands (f32x3_t: the generic and split-K kernels only)
    const GemmSwitches& sw = switches();
    const bool dtype_bf16 = dtype == 1, x3 = dtype == 2;
    GemmPlan p;
    auto refuse = [&](const char* why) { p.refusal = why; return p; };
    auto take_rb = [&](bool stats) {
        p.route = x3 ? Route::rbx3 : Route::rb;
        p.tm = 256; p.tn = 128;
        p.stats = stats;
        p.gn_in_kernel = true;
        return p;
    };
    if (a.phase_c) {                 // only the resblock conv kernel's raw form knows the phase-major statistics
        // declined with a statistics request (group size), it is asked again without one and the caller runs the separate statistics pass: the one
        // place where a route is asked twice
        const char* const no = "conv_gemm: a 3-tap-form transposed conv that conv_gemm_rb_kernel does not take";
        if (dtype == 0 || a.flat) return refuse(no);
        const bool with_stats = a.stats && rb_takes(a, x3, true);
        if (!with_stats && !rb_takes(a, x3, false)) return refuse(no);
        p.stats_traced = with_stats;
        return take_rb(with_stats);
    }
    if (a.nseg < 1 || a.nseg > 2) return refuse("conv_gemm: nseg must be 1 or 2");
    if (a.n_pad % 32) return refuse("conv_gemm: n_pad must be a multiple of 32");
    const int epc = dtype_bf16 ? 8 : 4;
    if (a.n % epc || a.out_c % epc) return refuse("conv_gemm: output channels must be a multiple of a 16-byte chunk");
    const long long esz = dtype_bf16 ? 2 : 4;
    if ((long long)a.B * a.out_rows * a.out_c * esz >= (1LL << 32)) return refuse("conv_gemm: output tensor must be < 4 GiB");
    bool raw = true;
    for (int s = 0; s < a.nseg; ++s) {
        const GemmSeg& g = a.seg[s];
        if (g.c0 % epc || g.c1 % epc) return refuse("conv_gemm: channel counts must be multiples of a 16-byte chunk");
        if (g.step != 1 && g.step != -1) return refuse("conv_gemm: step must be +-1");
        if (g.taps < 1 || g.stride < 1) return refuse("conv_gemm: bad taps/stride");
        if (g.ab) raw = false;
        if ((long long)a.B * a.lin * (g.c0 > g.c1 ? g.c0 : g.c1) * esz >= (1LL << 32)) return refuse("conv_gemm: input tensor must be < 4 GiB");
    }
    // 1. The generic kernel's tile: every route below starts from it.  Per-sample tiles need (TM-1)*stride + taps staged rows; flat tiles (several whole
    // samples per tile, raw inputs only) need (TM/mrows) * ((mrows-1)*stride + taps).
    const bool can_flat = raw && !a.scatter_f && a.lin == a.mrows && (a.mrows & (a.mrows - 1)) == 0;
    int tm = 0, flat = 0;
    for (int cand = 128; cand >= 32 && !tm; cand >>= 1) {
        if (can_flat && a.mrows < cand) {
            bool fits = true;
            for (int s = 0; s < a.nseg; ++s)
                if ((cand / a.mrows) * ((a.mrows - 1) * a.seg[s].stride + a.seg[s].taps) > kARows) fits = false;
            if (fits) { tm = cand; flat = 1; continue; }
        }
        bool fits = true;
        for (int s = 0; s < a.nseg; ++s)
            if ((cand - 1) * a.seg[s].stride + a.seg[s].taps > kARows) fits = false;
        if (!fits) continue;
        if (cand > 32 && a.mrows <= cand / 2) continue;
        tm = cand;
    }
    if (!tm) return refuse("conv_gemm: no tile shape fits (stride/taps too large)");
    int tn = a.n_pad >= 128 ? 128 : (a.n_pad >= 64 ? 64 : 32);
    if (a.n_pad % tn && a.n_pad % 64 == 0) tn = 64;
    // keep the 256 CUs busy when the problem is small: prefer narrower N tiles, then shorter M tiles
    auto nblocks = [&](int tm_, int tn_) {
        const long long tmn = flat ? ((long long)a.B * a.mrows + tm_ - 1) / tm_ : (long long)((a.mrows + tm_ - 1) / tm_) * a.B;
        return tmn * ((a.n_pad + tn_ - 1) / tn_);
    };
    while (nblocks(tm, tn) < sw.min_blocks && tn > 32) tn >>= 1;
    while (nblocks(tm, tn) < sw.min_blocks && tm > 32) {
        tm >>= 1;
        if (flat && a.mrows >= tm) flat = 0;   // a tile now lies inside one sample again
    }
    p.route = Route::plain;
    p.tm = tm; p.tn = tn;
    p.flat = flat;
    p.seg_rows = flat ? a.mrows : tm;
    if (a.stats) {
        // the epilogue reduces statistics per thread-column and wave: see adf_gemm.h phase 2
        const int nthr = (tm == 64 && tn == 32) || (tm == 32 && tn == 64) ? 128 : ((tm == 32 && tn == 32) ? 64 : 256);
        const int rpk = nthr * epc / tn;
        p.stats = stats_groups_ok(a.out_c, a.stats_groups, epc, tn) && (!flat || a.mrows % rpk == 0);
    }
    p.stats_traced = p.stats;
    auto take = [&](Route r, int tm_, int tn_, bool stats) {
        p.route = r;
        p.tm = tm_; p.tn = tn_;
        p.stats = p.stats_traced = stats;
        return p;
    };
    // GroupNorm affine of segment 0 still to be derived from the statistics: the DMA kernels do it themselves (one launch less per GroupNorm: 4.7 us
    // each, 44 per network pass before), every other route gets gn_finalize launched first
    const GemmSeg& g0 = a.seg[0];
    const bool gn_pending = g0.gn.gamma != nullptr;
    {
        // 2. up: transposed convs of the up path in bf16 (adf_gemm_up.h)
        const int f = a.scatter_f, cout = a.out_c, cin = g0.c0;
        if (sw.up && dtype_bf16 && (f == 2 || f == 4) && a.nseg == 1 && g0.taps == 2 && g0.stride == 1 && g0.off0 == 0 && g0.step == -1 && !g0.ab &&
            !gn_pending && !g0.act && g0.scale1 == 1.0f && g0.wfrag && g0.c1 == 0 && a.n == f * cout && a.n == a.n_pad && a.mrows == a.lin + 1 &&
            a.out_rows == a.lin * f && a.scatter_pad == f / 2 && a.bias_mod == cout && !a.res && !a.gelu && !a.bias1 &&
            (!a.stats || a.stats_groups == 8)) {
            // measured (us per launch at batch 64, this kernel vs the plain / weight-stationary route): 256 -> 256 x4 at L = 16 / 64 / 256: 10.3 / 13.2 /
            // 32.7 (indexed by output block on 32- / 64- / 128-row tiles; 17.7 / 18.5 / 50.3 over m = 0 .. L on 128-row tiles: profiles/README.md) vs
            // 17 / 27 / 65; 256 -> 128 x2 at L = 1024: 47 vs 66; 128 -> 128 x2 at L = 2048 and 128 -> 64 x2 at L = 4096: 57 / 53 vs 57 / 53
            // (their tiles are bound by the per-CU HBM fetch rate, which this kernel does not overlap with the MFMAs): those two
            // stay on the old routes unless ADF_GEMM_UP=2
            if (cin == 256 && cout == 256 && f == 4) p.up_cfg = 1;
            else if (cin == 256 && cout == 128 && f == 2) p.up_cfg = 2;
            else if (sw.up >= 2 && cin == 128 && cout == 128 && f == 2) p.up_cfg = 3;
            else if (sw.up >= 2 && cin == 128 && cout == 64 && f == 2) p.up_cfg = 4;
            if (p.up_cfg) return take(Route::up, 64, 256, a.stats != nullptr);
        }
    }
    {
        // 3. ksplit: short levels (few rows, long K): intra-block split-K, 32 x 32 tiles, 4 waves x K/4 each
        int nit_total = 0;
        bool ks_ok = sw.ksplit && !a.scatter_f && (long long)a.B * a.mrows <= sw.ksplit_rows;
        const int ks_flat = (can_flat && a.mrows < 32 && 32 % a.mrows == 0) ? 1 : 0;
        const int ks_seg = ks_flat ? a.mrows : 32;
        if (!ks_flat && !raw && a.mrows < 32) ks_ok = false;     // per-sample tiles of a tiny sample: leave to the plain kernel
        for (int s = 0; s < a.nseg; ++s) {
            const GemmSeg& g = a.seg[s];
            if (g.stride != 1 || g.taps > kTapGroup) ks_ok = false;
            if ((32 / ks_seg) * ((ks_seg - 1) + g.taps) > ks_a_rows(1)) ks_ok = false;
            nit_total += g.nchunk;
        }
        if (ks_ok && nit_total >= sw.ksplit_minit) {
            // 64 x 64 tiles when they still give >= 128 blocks: every tile row re-reads all weights and every tile column
            // all activations (from L2), so the bytes a CU pulls halve against 32 x 32 (ADF_GEMM_KSPLIT=32 forces the small tile)
            const bool big = sw.ksplit != 32 && !ks_flat && a.mrows % 64 == 0 && a.n_pad % 64 == 0 &&
                             (long long)a.B * (a.mrows / 64) * (a.n_pad / 64) >= 128;
            const int tile = big ? 64 : 32;
            p.flat = ks_flat;
            p.seg_rows = big ? 64 : ks_seg;
            const int rows_per_wave = 64 / (tile / epc);
            return take(Route::ksplit, tile, tile, a.stats && stats_groups_ok(a.out_c, a.stats_groups, epc, tile) && p.seg_rows % rows_per_wave == 0);
        }
    }
    // 4. rb / rbx3: resblock convs (GroupNorm + SiLU prologue derived in the kernel) and raw 3-tap convs on 256-row tiles: adf_gemm_rb.h in bf16,
    // the same data path on 32-channel blocks of fp32 storage with split-bf16 products in adf_gemm_rbx3.h.  Asked once, with the statistics request.
    const bool rb_raw = !gn_pending && !g0.ab && !g0.act && a.nseg == 1 && !a.res && g0.taps == 3;
    if (dtype != 0 && !flat && ((gn_pending && sw.gn_in_kernel && !a.gn_ready) || rb_raw) && rb_takes(a, x3, true)) return take_rb(a.stats != nullptr);
    // 5. pp: large stride-1 bf16 layers on the persistent LDS-DMA 256 x 128 kernel (adf_gemm_pp.h).  Measured on MI355X (profiles/README.md): 12-20 %
    // faster than the routes below where it applies by default -- >= 256 tiles and no identity residual (those layers keep their weights resident in
    // the weight-stationary kernel, which wins).  The transformer's 1x1 projections (one 1-tap segment) measured equal to the plain kernel end to end
    // (388.6-393.9 vs 389.6-390.9 ms) and stay there.
    if (sw.pp && dtype_bf16 && !flat && tm == 128 && !(g0.taps == 1 && a.nseg == 1) && (sw.pp == 2 || !a.res)) {
        // tile height: 256 rows when that gives every CU a tile, else 128 rows (the L = 256 level at batch 64)
        const long long t256 = pp_eligible(a, 256) ? (long long)a.B * (a.mrows / 256) * (a.n_pad / kPpTN) : 0;
        const long long t128 = pp_eligible(a, 128) ? (long long)a.B * (a.mrows / 128) * (a.n_pad / kPpTN) : 0;
        const long long need = sw.pp >= 2 ? 128 : 256;
        const int ptm = t256 >= need ? 256 : ((t128 >= need && sw.pp != 3) ? 128 : 0);
        if (ptm) {
            p.ident_seg = a.res != nullptr;
            // (a GroupNorm group across the two sources -- an odd group count -- is derived by gn_finalize alone: adf_common.h gn_group_straddles)
            const int gn_gs = g0.gn.G > 0 ? (g0.gn.c0 + g0.gn.c1) / g0.gn.G : 0;
            p.gn_in_kernel = g0.taps == 3 && sw.gn_in_kernel && gn_gs > 0 && g0.gn.c0 % gn_gs == 0;
            return take(Route::pp, ptm, 128, a.stats && stats_groups_ok(a.out_c, a.stats_groups, 8, 64));
        }
    }
    {
        // 6. ws: large stride-1 layers on the weight-stationary persistent kernel when the weights of an N tile fit in LDS
        bool ws_ok = sw.ws && !x3 && !flat && tm == 128 && a.n_pad >= 64;
        for (int s = 0; s < a.nseg; ++s)
            if (a.seg[s].stride != 1 || 127 + a.seg[s].taps > kWsARows) ws_ok = false;
        const long long tiles_m_total = (long long)((a.mrows + 127) / 128) * a.B;
        if (ws_ok && tiles_m_total >= sw.ws_min_m) {
            // measured on MI355X: the weight-stationary kernel wins with 128-wide N tiles (Cin = Cout = 128 layers);
            // with 64-wide tiles (ADF_GEMM_WS=64 to force) the doubled activation staging loses to the plain kernel
            int wtn = 0;
            if (a.n_pad >= 128 && ws_lds_bytes(a, 128) <= 160 * 1024) wtn = 128;
            else if (sw.ws == 64 && ws_lds_bytes(a, 64) <= 160 * 1024) wtn = 64;
            // (wtn / 2: the columns owned by one consumer wave)
            if (wtn) return take(Route::ws, 128, wtn, a.stats && stats_groups_ok(a.out_c, a.stats_groups, epc, wtn / 2));
            // weights too large to stay resident (identity-residual 256 -> 256 layers): the plain kernel; a variant that streamed
            // the weights through an LDS-DMA ring beside the producer / consumer waves measured 1 % slower end to end
        }
    }
    return p;       // 7. plain: the generic kernel on the tile of step 1
}

}  // namespace

bool conv_gemm_phase_eligible(const GemmArgs& a, int dtype, bool* stats_fused) {
    const GemmPlan p = decide_conv_gemm(a, dtype);
    if (stats_fused) *stats_fused = p.stats;
    return a.phase_c && p.route != Route::refused;
}

// decide, settle the GroupNorm table, trace, launch the chosen kernel
const char* launch_conv_gemm(const GemmArgs& a_in, int dtype, hipStream_t stream, bool* stats_fused) {
    const GemmSwitches& sw = switches();
    const GemmPlan p = decide_conv_gemm(a_in, dtype);
    if (stats_fused) *stats_fused = p.stats;
    if (p.route == Route::refused) return p.refusal;
    GemmArgs a = a_in;
    a.flat = p.flat;
    a.seg_rows = p.seg_rows;
    if (!p.stats) a.stats = nullptr;
    if (a.nseg > 1) a.seg[1].gn.gamma = nullptr;
    if (p.ident_seg) {                     // identity residual = a raw 1-tap segment against the packed identity
        const char* err = nullptr;
        const void* ident = pp_identity(a.n, stream, &err);
        if (!ident) return err;
        GemmSeg& g = a.seg[1];
        g = GemmSeg{};
        g.src0 = a.res; g.src1 = nullptr; g.c0 = a.n; g.c1 = 0; g.ab = nullptr; g.scale1 = 1.0f; g.act = 0;
        g.taps = 1; g.stride = 1; g.off0 = 0; g.step = 1; g.w = ident; g.nchunk = a.n / 64;
        a.nseg = 2;
        a.res = nullptr;
    }
    if (a.seg[0].gn.gamma && !p.gn_in_kernel) {
        const char* err = a.gn_ready ? nullptr : launch_gn_finalize(a.seg[0].gn, stream);
        a.seg[0].gn.gamma = nullptr;
        if (err) return err;
    }
    if (sw.trace) {
        fprintf(stderr, "[adf gemm] %-6s B=%d lin=%d mrows=%d n=%d/%d nseg=%d seg0(c=%d+%d taps=%d stride=%d off0=%d step=%d ab=%d act=%d)", kRouteName[(int)p.route], a.B,
                a.lin, a.mrows, a.n, a.n_pad, a.nseg, a.seg[0].c0, a.seg[0].c1, a.seg[0].taps, a.seg[0].stride, a.seg[0].off0, a.seg[0].step, a.seg[0].ab != nullptr,
                a.seg[0].act);
        if (a.nseg > 1) fprintf(stderr, " seg1(c=%d+%d taps=%d ab=%d)", a.seg[1].c0, a.seg[1].c1, a.seg[1].taps, a.seg[1].ab != nullptr);
        fprintf(stderr, " res=%d gelu=%d scatter=%d out=%dx%d stats=%d flat=%d tile=%dx%d\n", a.res != nullptr, a.gelu, a.scatter_f, a.out_rows, a.out_c, p.stats_traced,
                a.flat, p.tm, p.tn);
    }
    switch (p.route) {
    case Route::up:
        if (p.up_cfg == 1) return launch_up<256, 256, 4>(a, stream);
        if (p.up_cfg == 2) return launch_up<256, 128, 2>(a, stream);
        if (p.up_cfg == 3) return launch_up<128, 128, 2>(a, stream);
        return launch_up<128, 64, 2>(a, stream);
    case Route::ksplit:
        if (p.tm == 64) return dtype == 1 ? launch_ksplit<bf16_t, 2, 2>(a, stream) : (dtype == 2 ? launch_ksplit<f32x3_t, 2, 2>(a, stream) : launch_ksplit<float, 2, 2>(a, stream));
        return dtype == 1 ? launch_ksplit<bf16_t, 1, 1>(a, stream) : (dtype == 2 ? launch_ksplit<f32x3_t, 1, 1>(a, stream) : launch_ksplit<float, 1, 1>(a, stream));
    case Route::rbx3: return launch_rbx3(a, sw.rbx3_min_tiles, stream);
    case Route::rb: return launch_rb(a, sw.rb_min_tiles, sw.rb_zskip, stream);
    case Route::pp: return p.tm == 256 ? launch_pp<2>(a, stream) : launch_pp<1>(a, stream);
    case Route::ws:
        if (p.tn == 128) return dtype == 1 ? launch_ws_variant<bf16_t, 2, 2>(a, stream) : launch_ws_variant<float, 2, 2>(a, stream);
        return dtype == 1 ? launch_ws_variant<bf16_t, 1, 2>(a, stream) : launch_ws_variant<float, 1, 2>(a, stream);
    default: return dtype == 1 ? dispatch<bf16_t>(a, p.tm, p.tn, stream) : (dtype == 2 ? dispatch<f32x3_t>(a, p.tm, p.tn, stream) : dispatch<float>(a, p.tm, p.tn, stream));
    }
}

}  // namespace adf

// include/audiodiffuser_amd.h: the K-block table launch_rb would build for a raw launch (host arithmetic only)
extern "C" int adf_debug_rb_block_plan(int K, int f, int C, int phase_c, int n, int B, int L, int min_tiles, int zskip, int* tile_rows, int* nh, int* nb3, int* nb2,
                                       int* phase2) {
    using namespace adf;
    if (B < 1 || L < 1 || C < 1 || f < 1 || (long long)B * L > 0x3fffffffLL) return 1;
    static const char dummy[16] = {};
    GemmArgs a;
    memset(&a, 0, sizeof(a));
    a.nseg = 1; a.B = B; a.lin = a.mrows = a.out_rows = L; a.n = a.n_pad = a.out_c = a.bias_mod = n;
    a.phase_c = phase_c;
    GemmSeg& g = a.seg[0];
    g.src0 = g.w = dummy;
    g.c0 = phase_c ? C : f * C;
    g.taps = 3; g.stride = 1; g.off0 = -1; g.step = 1;
    g.tap2_zero_c = phase_c ? 0 : folded_tap2_zero_from(K, f, C);
    RbTiles t;
    if (!rb_shape_ok(a, kRbBf16, false) || !rb_tiles(a, kRbBf16, min_tiles, t)) return 1;
    RbArgs r;
    rb_fill_args(a, kRbBf16, t, zskip, r);
    if (tile_rows) *tile_rows = t.tm;
    if (nh) *nh = t.nh;
    if (nb3) *nb3 = r.h.nb3;
    if (nb2) *nb2 = r.h.nb2;
    if (phase2) *phase2 = r.h.phase2;
    return 0;
}

// include/audiodiffuser_amd.h: the tile plan launch_up would take for one of the four shapes of the transposed-conv kernel (host arithmetic only)
extern "C" int adf_debug_up_tile_plan(int cin, int cout, int f, int B, int L, int* tile_rows, int* items, int* rounds, int* dead_rows) {
    using namespace adf;
    if (B < 1 || L < 1 || (long long)B * L > 0x3fffffffLL) return 1;
    UpTilePlan tp;
    if (cin == 256 && cout == 256 && f == 4) tp = up_tile_plan(B, L, UpCfg<256, 256, 4, 1>::WROWS, UpCfg<256, 256, 4, 1>::NPASS);
    else if (cin == 256 && cout == 128 && f == 2) tp = up_tile_plan(B, L, UpCfg<256, 128, 2, 1>::WROWS, UpCfg<256, 128, 2, 1>::NPASS);
    else if (cin == 128 && cout == 128 && f == 2) tp = up_tile_plan(B, L, UpCfg<128, 128, 2, 1>::WROWS, UpCfg<128, 128, 2, 1>::NPASS);
    else if (cin == 128 && cout == 64 && f == 2) tp = up_tile_plan(B, L, UpCfg<128, 64, 2, 1>::WROWS, UpCfg<128, 64, 2, 1>::NPASS);
    else return 1;
    if (tile_rows) *tile_rows = tp.tile_rows;
    if (items) *items = (int)tp.items;
    if (rounds) *rounds = (int)tp.rounds;
    if (dead_rows) *dead_rows = tp.dead_rows;
    return 0;
}
