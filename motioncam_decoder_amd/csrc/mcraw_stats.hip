// mcraw_stats.hip -- gfx950 kernels for per-frame statistics of uint16 mosaics resident in HBM (mcraw_stats_batch): per CFA
// position a histogram, the sample count, the saturated count, the sum of the unsaturated samples, min and max.
// The contract (integers only: bit-exact whatever the order of additions) is in include/mcraw_hip.h; DESIGN.md 17 has the design.
//
// A reduction, not a map.  A workgroup owns a run of consecutive tiles (ST_TW columns x ST_TH rows) of one frame's window.  The
// tile grid starts on an even row and an even column (on a multiple of 8 columns on the 16-byte path), so a lane's 8 columns of 2
// rows are 4 samples of each CFA position at fixed register places.  Histogram increments go to LDS: NC copies of the 4 x B
// counters (copy = lane % NC, copies staggered by 4 banks), 32-bit, so nothing can wrap.  Before a lane touches LDS it merges
// equal bins among its 4 samples of a position, and a wave whose 256 samples of a position all share one bin (flat or clipped
// content) adds 256 once.  min / max / saturated count / sum stay in registers until the workgroup ends.  At its end a
// workgroup adds the non-zero counters to the frame's record with global integer atomics: its write traffic is at most one
// record, whatever the number of pixels.  kstats_init writes the empty records first (unless MCRAW_STATS_ACCUMULATE).
//
// Test builds (build.MOSAIC_PATH_VARIANTS, tests/test_gpu_mosaic_paths.py; why each is valid: the head of mcraw_mosaic_paths.h):
//   MCRAW_PATHSM            the path census
//   MCRAW_FORCE_SLOWM       no wave takes stats_tile<BL, true>, and with it none the one-bin shortcut
//   MCRAW_STATS_MAXTILES=N  at most N tiles per workgroup
//   MCRAW_STAGE_FRAMES=N  the launch loop takes N frames at a time (mcraw_mosaic_paths.h: `frames2`)
#ifdef MCRAW_STAGE_FRAMES
#define LAUNCH_PIECE MCRAW_STAGE_FRAMES
#endif
#include "mcraw_host.h"
#ifdef MCRAW_PATHSM
#include "mcraw_mosaic_paths.h"
#endif
#include "mcraw_mosaic.h"

namespace mcraw {

constexpr int ST_T = 256;        // threads per workgroup
constexpr uint32_t ST_LX = 32u;  // lanes across a tile: 8 columns each
constexpr uint32_t ST_TW = 8u * ST_LX;
constexpr uint32_t ST_TH = 2u * (ST_T / ST_LX); // 2 rows per lane
// Tiles per workgroup at most: a lane's 32-bit sum of a position grows by at most 4 * 65535 per tile, 8192 * 4 * 65535 < 2^32.
#ifndef MCRAW_STATS_MAXTILES
#define MCRAW_STATS_MAXTILES 8192
#endif
constexpr uint32_t ST_MAXTILES = MCRAW_STATS_MAXTILES;
static_assert(ST_MAXTILES >= 1u && ST_MAXTILES <= 8192u, "a lane's 32-bit sums hold 8192 tiles at most");
#ifdef MCRAW_FORCE_SLOWM
constexpr bool ST_FULL_OK = false;
#else
constexpr bool ST_FULL_OK = true; // waves whose samples are all inside the window take stats_tile<BL, true>
#endif
constexpr uint32_t ST_WGS = 2048u; // workgroups a launch aims at (8 per CU)
constexpr uint32_t ST_NOBIN = 0xFFFFFFFFu;

// LDS copies of the histogram for B = 1 << BL bins: 8 up to 256 bins (33 KB at 256), then as many as 32 KB hold; 64 KB for 4096.
template <int BL>
struct StatsCfg {
    static constexpr uint32_t B = 1u << BL;
    static constexpr uint32_t NC = BL <= 8 ? 8u : BL >= 11 ? 1u : (8u >> (BL - 8));
    static constexpr uint32_t CS = 4u * B + (NC > 1u ? 4u : 0u); // dwords from copy to copy: bank of (copy, bin) = bin + 4 * copy
};

struct StatsArgs {
    const uint16_t *in;
    uint32_t *out; // the launch's first record
    size_t ipitch, ifstride;
    uint32_t recwords;       // dwords per record
    uint32_t xa, ya;         // origin of the tile grid: <= x0, y0, even
    uint32_t x0, x1, y0, y1; // the window: [x0, x1) x [y0, y1)
    uint32_t tilesX, tiles, tpc; // tiles across, in all, per workgroup
    uint32_t shift;
    uint32_t sat[4];
    uint32_t cnt[4]; // samples of the window by CFA position (geometry alone)
    uint32_t vec;    // every 8-column piece of the tile grid lies on the 16-byte grid
};

// The lane's part of tile t: p[a][k] = columns x + 2k (low half), x + 2k + 1 (high half) of row y + a; the returned mask has bit
// i for column x + i inside the window and bits 8, 9 for the two rows.  Only samples of the window are read.
__device__ __forceinline__ uint32_t stats_load(const StatsArgs &A, const uint16_t *fin, uint32_t t, uint32_t lx, uint32_t ly,
                                               uint32_t p[2][4])
{
    const uint32_t ty = t / A.tilesX, tx = t - ty * A.tilesX;
    const uint32_t x = A.xa + tx * ST_TW + 8u * lx, y = A.ya + ty * ST_TH + 2u * ly;
    const uint32_t lo = A.x0 > x ? min(A.x0 - x, 8u) : 0u, hi = A.x1 > x ? min(A.x1 - x, 8u) : 0u;
    const uint32_t cols = hi > lo ? ((1u << hi) - 1u) & ~((1u << lo) - 1u) : 0u;
    uint32_t m = cols;
#pragma unroll
    for (uint32_t a = 0; a < 2u; a++) {
        p[a][0] = p[a][1] = p[a][2] = p[a][3] = 0u;
        const uint32_t yy = y + a;
        MOS_PATH(MP_SS_ROW_OUT, cols == 0u || yy < A.y0 || yy >= A.y1);
        if (cols == 0u || yy < A.y0 || yy >= A.y1)
            continue;
        MOS_PATH(MP_SS_LD_EDGE, cols != 0xFFu);
        m |= 256u << a;
        const uint16_t *src = fin + static_cast<size_t>(yy) * A.ipitch + x;
        if (cols == 0xFFu) {
            load8(src, 8u, A.vec != 0u, p[a]);
        } else { // the window's left or right edge: element loads
#pragma unroll
            for (uint32_t i = 0; i < 8u; i++)
                if (cols >> i & 1u)
                    p[a][i >> 1] |= static_cast<uint32_t>(gptr<const uint16_t>(src)[i]) << (16u * (i & 1u));
        }
    }
    return (m & 0x300u) ? m : 0u;
}

struct StatsAcc {
    uint32_t nsat[4], sum[4]; // by CFA position
    uint32_t mn[2], mx[2];    // by row parity: (even column | odd column << 16)
};

// One lane's 16 samples.  FULL: all of them are inside the window, for every lane of the wave.
template <int BL, bool FULL>
__device__ __forceinline__ void stats_tile(const StatsArgs &A, const uint32_t p[2][4], uint32_t m, uint32_t *hc, StatsAcc &S)
{
    constexpr uint32_t B = StatsCfg<BL>::B;
#pragma unroll
    for (uint32_t a = 0; a < 2u; a++) {
        const bool row = FULL || (m >> (8u + a) & 1u);
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) { // min / max of both column parities at once; a sample outside is 65535 / 0
            const uint32_t off = FULL ? 0u
                                      : ((row && (m >> (2u * k) & 1u)) ? 0u : 0xFFFFu) |
                                            ((row && (m >> (2u * k + 1u) & 1u)) ? 0u : 0xFFFF0000u);
            S.mn[a] = pk_min(S.mn[a], p[a][k] | off);
            S.mx[a] = pk_max(S.mx[a], p[a][k] & ~off);
        }
#pragma unroll
        for (uint32_t par = 0; par < 2u; par++) {
            const uint32_t pos = 2u * a + par, sat = A.sat[pos];
            uint32_t b[4];
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++) {
                const uint32_t v = par ? p[a][k] >> 16 : p[a][k] & 0xFFFFu;
                const bool ok = FULL || (row && (m >> (2u * k + par) & 1u));
                const bool s = v >= sat;
                S.nsat[pos] += (ok && s) ? 1u : 0u;
                S.sum[pos] += (ok && !s) ? v : 0u;
                b[k] = ok ? min(v >> A.shift, B - 1u) : ST_NOBIN;
            }
            uint32_t *h = hc + pos * B;
            if (FULL) { // flat or clipped content: the wave's 256 samples of this position in one bin, one add
                const uint32_t first = __builtin_amdgcn_readfirstlane(b[0]);
                if (__all(b[0] == first && b[1] == first && b[2] == first && b[3] == first)) {
                    MOS_WAVE(MP_SS_ONEBIN, true);
                    if (__lane_id() == 0u)
                        atomicAdd(h + first, 4u * 64u);
                    continue;
                }
            }
            // equal bins of the lane merge before they reach LDS
            const uint32_t e01 = b[1] == b[0], e02 = b[2] == b[0], e03 = b[3] == b[0];
            const uint32_t e12 = b[2] == b[1], e13 = b[3] == b[1], e23 = b[3] == b[2];
            if (FULL || b[0] != ST_NOBIN)
                atomicAdd(h + b[0], 1u + e01 + e02 + e03);
            if (!e01 && (FULL || b[1] != ST_NOBIN))
                atomicAdd(h + b[1], 1u + e12 + e13);
            if (!e02 && !e12 && (FULL || b[2] != ST_NOBIN))
                atomicAdd(h + b[2], 1u + e23);
            if (!e03 && !e13 && !e23 && (FULL || b[3] != ST_NOBIN))
                atomicAdd(h + b[3], 1u);
        }
    }
}

template <int BL>
__global__ void __launch_bounds__(ST_T) kstats(const StatsArgs A)
{
    constexpr uint32_t B = StatsCfg<BL>::B, NC = StatsCfg<BL>::NC, CS = StatsCfg<BL>::CS;
    __shared__ uint32_t s_h[NC * CS];
    const uint32_t f = blockIdx.y, t0 = blockIdx.x * A.tpc, t1 = min(t0 + A.tpc, A.tiles);
    const uint32_t lx = threadIdx.x % ST_LX, ly = threadIdx.x / ST_LX;
    const uint16_t *fin = A.in + static_cast<size_t>(f) * A.ifstride;
    MOS_PATH(MP_WG, threadIdx.x == 0u);
    uint32_t cur[2][4], nxt[2][4];
    uint32_t curm = stats_load(A, fin, t0, lx, ly, cur), nxtm = 0u; // in flight while LDS is cleared
    for (uint32_t i = threadIdx.x; i < NC * CS; i += ST_T)
        s_h[i] = 0u;
    __syncthreads();
    uint32_t *hc = s_h + (threadIdx.x & (NC - 1u)) * CS;
    StatsAcc S;
#pragma unroll
    for (uint32_t i = 0; i < 4u; i++)
        S.nsat[i] = S.sum[i] = 0u;
    S.mn[0] = S.mn[1] = 0xFFFFFFFFu;
    S.mx[0] = S.mx[1] = 0u;
    for (uint32_t t = t0; t < t1; t++) {
        MOS_PATH(MP_SS_PREFETCH, threadIdx.x == 0u && t + 1u < t1);
        if (t + 1u < t1)
            nxtm = stats_load(A, fin, t + 1u, lx, ly, nxt); // the next tile's loads fly while this one is counted
        MOS_WAVE(MP_SS_FULL, ST_FULL_OK && __all(curm == 0x3FFu));
        MOS_WAVE(MP_SS_PARTIAL, !(ST_FULL_OK && __all(curm == 0x3FFu)) && __any(curm != 0u));
        MOS_WAVE(MP_SS_EMPTY, !__any(curm != 0u));
        if (ST_FULL_OK && __all(curm == 0x3FFu))
            stats_tile<BL, true>(A, cur, curm, hc, S);
        else if (__any(curm != 0u))
            stats_tile<BL, false>(A, cur, curm, hc, S);
#pragma unroll
        for (uint32_t a = 0; a < 2u; a++)
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++)
                cur[a][k] = nxt[a][k];
        curm = nxtm;
    }
    // the registers: reduce over the wave, then one lane adds to the record
    uint32_t *rec = A.out + static_cast<size_t>(f) * A.recwords;
    uint32_t *small = rec + 4u * B; // cnt[4], nsat[4], min[4], max[4], then uint64 sum[4]
#pragma unroll
    for (uint32_t pos = 0; pos < 4u; pos++) {
        uint32_t ns = S.nsat[pos];
        unsigned long long sm = S.sum[pos];
        uint32_t mn = (pos & 1u) ? S.mn[pos >> 1] >> 16 : S.mn[pos >> 1] & 0xFFFFu;
        uint32_t mx = (pos & 1u) ? S.mx[pos >> 1] >> 16 : S.mx[pos >> 1] & 0xFFFFu;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            ns += __shfl_xor(ns, d);
            sm += __shfl_xor(sm, d);
            mn = min(mn, static_cast<uint32_t>(__shfl_xor(mn, d)));
            mx = max(mx, static_cast<uint32_t>(__shfl_xor(mx, d)));
        }
        if (__lane_id() == 0u) {
            if (ns)
                atomicAdd(small + 4u + pos, ns);
            if (mn != 0xFFFFu)
                atomicMin(small + 8u + pos, mn);
            if (mx)
                atomicMax(small + 12u + pos, mx);
            if (sm)
                atomicAdd(reinterpret_cast<unsigned long long *>(small + 16u) + pos, sm);
        }
    }
    if (blockIdx.x == 0u && threadIdx.x < 4u && A.cnt[threadIdx.x])
        atomicAdd(small + threadIdx.x, A.cnt[threadIdx.x]);
    // the histogram: the copies' sum, the non-zero counters only
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < 4u * B; i += ST_T) {
        uint32_t s = 0u;
#pragma unroll
        for (uint32_t c = 0; c < NC; c++)
            s += s_h[c * CS + i];
        if (s)
            atomicAdd(rec + i, s);
    }
}

// Empty records: every counter 0, min 65535.
__global__ void __launch_bounds__(256) kstats_init(uint32_t *out, size_t words, uint32_t recwords, uint32_t B)
{
    const size_t step = static_cast<size_t>(gridDim.x) * blockDim.x;
    for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < words; i += step) {
        const uint32_t w = static_cast<uint32_t>(i % recwords);
        out[i] = (w >= 4u * B + 8u && w < 4u * B + 12u) ? 65535u : 0u;
    }
}

template <int BL>
static void stats_launch(const StatsArgs &A, dim3 grid, hipStream_t st)
{
    hipLaunchKernelGGL(kstats<BL>, grid, dim3(ST_T), 0, st, A);
}

// samples y in [lo, hi) with y & 1 == par
static uint32_t stats_parity(uint32_t lo, uint32_t hi, uint32_t par)
{
    return ((hi + 1u - par) >> 1) - ((lo + 1u - par) >> 1);
}

} // namespace mcraw

using namespace mcraw;

extern "C" size_t mcraw_stats_record_bytes(uint32_t bins_log2)
{
    return bins_log2 >= 6u && bins_log2 <= 12u ? (static_cast<size_t>(16) << bins_log2) + 96u : 0u;
}

extern "C" int mcraw_stats_batch(mcraw_ctx *c, const mcraw_stats *s, const uint16_t *in, size_t in_pitch, size_t in_frame_stride,
                                 int width, int height, int n, void *out, size_t out_bytes, void *stream)
{
    if (!c || !s || n < 0)
        return reject(__func__, "bad arguments");
    if (n == 0)
        return 0;
    if (!in || !out)
        return reject(__func__, "in or out missing");
    if (reinterpret_cast<uintptr_t>(in) & 1u)
        return reject(__func__, "in not aligned to uint16");
    if (reinterpret_cast<uintptr_t>(out) & 7u)
        return reject(__func__, "out not 8-byte aligned");
    const MosaicBatch I(in, in_pitch, in_frame_stride, static_cast<size_t>(n), width, height);
    if (const char *why = I.check())
        return reject(__func__, why);
    const size_t W = static_cast<size_t>(width), H = static_cast<size_t>(height);
    if (s->bins_log2 < 6u || s->bins_log2 > 12u)
        return reject(__func__, "bins_log2 must be 6 .. 12");
    if (s->shift > 15u)
        return reject(__func__, "shift must be 0 .. 15");
    if (s->w < 1u || s->h < 1u)
        return reject(__func__, "w and h must be at least 1");
    if (s->x0 >= W || s->w > W - s->x0 || s->y0 >= H || s->h > H - s->y0)
        return reject(__func__, "the window leaves the frame");
    if (s->flags & ~MCRAW_STATS_ACCUMULATE)
        return reject(__func__, "unknown flag");
    if (s->reserved != 0u)
        return reject(__func__, "reserved must be 0");
    const size_t rec = mcraw_stats_record_bytes(s->bins_log2), need = static_cast<size_t>(n) * rec;
    if (out_bytes < need)
        return reject(__func__, "out_bytes below n * mcraw_stats_record_bytes(bins_log2)");
    if (ranges_overlap(I.base, I.bytes(), reinterpret_cast<uintptr_t>(out), need))
        return reject(__func__, "out overlaps the input");

    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = stream_of(c, stream);
    const uint32_t B = 1u << s->bins_log2;
    StatsArgs A{};
    A.ipitch = in_pitch;
    A.ifstride = in_frame_stride;
    A.recwords = static_cast<uint32_t>(rec / 4u);
    A.vec = I.on_grid();
    A.x0 = s->x0, A.x1 = s->x0 + s->w, A.y0 = s->y0, A.y1 = s->y0 + s->h;
    A.xa = A.x0 & ~(A.vec ? 7u : 1u);
    A.ya = A.y0 & ~1u;
    A.tilesX = (A.x1 - A.xa + ST_TW - 1u) / ST_TW;
    A.tiles = A.tilesX * ((A.y1 - A.ya + ST_TH - 1u) / ST_TH);
    A.shift = s->shift;
    for (uint32_t p = 0; p < 4u; p++) {
        A.sat[p] = s->sat[p];
        A.cnt[p] = stats_parity(A.y0, A.y1, p >> 1) * stats_parity(A.x0, A.x1, p & 1u);
    }
    if (!(s->flags & MCRAW_STATS_ACCUMULATE)) {
        const size_t words = need / 4u;
        const uint32_t blocks = static_cast<uint32_t>(std::min<size_t>((words + 255u) / 256u, 4096u));
        hipLaunchKernelGGL(kstats_init, dim3(blocks), dim3(256), 0, st, static_cast<uint32_t *>(out), words, A.recwords, B);
        HIP_TRY(hipGetLastError());
    }
    for (int f0 = 0; f0 < n; f0 += LAUNCH_PIECE) {
        const int nf = std::min<int>(LAUNCH_PIECE, n - f0);
        // a workgroup's merge costs a pass over its LDS histogram: at least B / 64 tiles each, and ST_WGS workgroups if that leaves enough
        const uint32_t want = std::max(1u, ST_WGS / static_cast<uint32_t>(nf));
        A.tpc = std::min(ST_MAXTILES, std::max(std::max(1u, B / 64u), (A.tiles + want - 1u) / want));
        A.in = in + static_cast<size_t>(f0) * in_frame_stride;
        A.out = static_cast<uint32_t *>(out) + static_cast<size_t>(f0) * A.recwords;
        const dim3 grid((A.tiles + A.tpc - 1u) / A.tpc, static_cast<uint32_t>(nf));
        switch (s->bins_log2) {
        case 6: stats_launch<6>(A, grid, st); break;
        case 7: stats_launch<7>(A, grid, st); break;
        case 8: stats_launch<8>(A, grid, st); break;
        case 9: stats_launch<9>(A, grid, st); break;
        case 10: stats_launch<10>(A, grid, st); break;
        case 11: stats_launch<11>(A, grid, st); break;
        default: stats_launch<12>(A, grid, st); break;
        }
        HIP_TRY(hipGetLastError());
    }
    return 0;
}
