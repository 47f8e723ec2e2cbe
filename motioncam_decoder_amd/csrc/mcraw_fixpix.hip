// mcraw_fixpix.hip -- gfx950 kernels for uint16 mosaics resident in HBM -> uint16 mosaics with the defective (hot, dead, stuck)
// pixels taken out (mcraw_fixpix_batch).  The contract (integers only, bit-exact) is in include/mcraw_hip.h; DESIGN.md 18 has
// the design.
//
// The first mosaic-to-mosaic stencil here.  kfixpix: a workgroup owns a tile of FP_TW columns x FP_TH rows of one frame and
// stages it with a 2-row, 2-column halo in LDS as raw samples, 16-byte chunks on the frame's 8-column grid (krgb_mhc's
// staging); the halo holds what the contract's reflection names, so the stencil itself knows no edges.  Lane (lx, ly) then
// makes 8 columns of rows r and r + 2 per pass (4 LDS rows for 2 output rows).  Neighbouring columns are different CFA
// positions but share the stencil offsets, so the detector runs on the dwords as they lie in memory, two pixels at a time:
// packed min / max keep the two largest and the two smallest of the eight neighbours (3 operations per neighbour and
// direction).  Thresholds, the pair choice and the counters are needed only where a pixel lies outside [Lk, Hk]: they sit
// behind that predicate, and a wave without such a pixel skips them.  The counts stay in registers; a wave reduces them
// with shuffles and one lane adds them to the frame's record.  kfixpix_list, queued behind it, replaces the listed pixels:
// one thread per (entry, frame), eight searches, one element written.
//
// Test builds (build.MOSAIC_PATH_VARIANTS, tests/test_gpu_mosaic_paths.py; why each is valid: the head of mcraw_mosaic_paths.h):
//   MCRAW_PATHSM       the path census
//   MCRAW_FORCE_SLOWM  `cand` is true for every lane
//   MCRAW_POISON_M     s_t filled with 0xFFFF in front of staging
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

constexpr int FP_T = TILE_T;     // threads per workgroup
constexpr uint32_t FP_LX = 32u;  // lanes across a tile: 8 columns each
constexpr uint32_t FP_TW = TILE_W;
// Tile rows: 32 re-reads 36/32 of the rows (19.1 KB of LDS, 8 workgroups per CU), 16 re-reads 20/16 (10.6 KB).
// -DMCRAW_FIXPIX_TH=16 builds the other one; tools/bench_fixpix.py --alt-lib runs two builds side by side.
#ifndef MCRAW_FIXPIX_TH
#define MCRAW_FIXPIX_TH 32
#endif
constexpr uint32_t FP_TH = MCRAW_FIXPIX_TH;
static_assert(FP_TH == 16u || FP_TH == 32u, "a pass is 16 rows: 8 lane rows x 2 rows");
constexpr uint32_t FP_LW = TILE_LW;     // LDS row: 8 columns either side (2 used), so that chunks stay on the 8-grid
constexpr uint32_t FP_LH = FP_TH + 4u;  // 2 halo rows above and below
constexpr uint32_t FP_MAXLIST = 1u << 20;

// Which stores the full aligned pieces of the output rows use: `sc1 nt` streaming stores (store_stream16), as kshade and the
// decode kernels use for rows that are written once, or plain ones.  -DMCRAW_FIXPIX_FLIP_STORES builds the other one.
#ifdef MCRAW_FIXPIX_FLIP_STORES
constexpr bool FP_NT = false;
#else
constexpr bool FP_NT = true;
#endif

struct FixArgs {
    const uint16_t *in;
    uint16_t *out;
    const uint32_t *list;
    uint32_t *counts; // the launch's first record, or NULL
    size_t ipitch, ifstride, opitch, ofstride;
    uint32_t W, H, tilesX;
    uint32_t hot, cold, rank, rel, nlist;
    uint32_t black[4], abs_thr[4];
    uint32_t invec, outvec; // every 8-column piece of `in` / `out` lies on the 16-byte grid
};

// The contract's neighbour coordinate: c + d; outside [0, n): c - d; that outside too: c.
__device__ __forceinline__ int fix_neighbour(int c, int d, int n)
{
    const int a = c + d, b = c - d;
    return (a >= 0 && a < n) ? a : (b >= 0 && b < n) ? b : c;
}

// The frame coordinate whose sample the halo coordinate h (-2, -1, n, n + 1) stands for.  Each halo coordinate is read by
// one pixel only, c = h + 2 on the low side and c = h - 2 on the high side, so the reflection of the contract is a map of
// coordinates: h + 4 (= c + 2), or c itself where that leaves the frame too.  Coordinates no output reads are clamped.
__device__ __forceinline__ int fix_halo(int h, int n)
{
    if (h < 0)
        h = h + 4 < n ? h + 4 : h + 2;
    else if (h >= n)
        h = h - 4 >= 0 ? h - 4 : h - 2;
    return min(max(h, 0), n - 1);
}

// The lower-bound search of the contract, literally.
__device__ __forceinline__ bool fix_member(const uint32_t *list, uint32_t nlist, uint32_t key)
{
    uint32_t lo = 0u, hi = nlist;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (gptr<const uint32_t>(list)[mid] < key)
            lo = mid + 1u;
        else
            hi = mid;
    }
    return lo < nlist && gptr<const uint32_t>(list)[lo] == key;
}

// 0xFFFF in every half that is not 0 (v_pk_mul_lo_u16)
__device__ __forceinline__ uint32_t fix_pknz(uint32_t a)
{
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, pk_min(a, 0x00010001u)) * __builtin_bit_cast(u16x2, 0xFFFFFFFFu));
}

// One opposite pair for both halves: where |a - b| is strictly below `best`, `val` takes (a + b + 1) >> 1
// (= (a | b) - ((a ^ b) >> 1), which needs no 17th bit).
__device__ __forceinline__ void fix_pair(uint32_t a, uint32_t b, bool first, uint32_t &best, uint32_t &val)
{
    const uint32_t d = pk_absdiff(a, b);
    const uint32_t avg = pk_sub(a | b, ((a ^ b) >> 1) & 0x7FFF7FFFu);
    if (first) {
        best = d, val = avg;
        return;
    }
    const uint32_t m = pk_min(best, d), lt = fix_pknz(m ^ best);
    val = (avg & lt) | (val & ~lt);
    best = m;
}

template <bool NT>
__global__ void __launch_bounds__(FP_T) kfixpix(const FixArgs A)
{
    __shared__ __attribute__((aligned(16))) uint16_t s_t[FP_LH * FP_LW];
    const uint32_t tile = blockIdx.x, f = blockIdx.y;
    const uint32_t ty = tile / A.tilesX, tx = tile - ty * A.tilesX;
    const int W = static_cast<int>(A.W), H = static_cast<int>(A.H);
    const int x0 = static_cast<int>(tx * FP_TW), y0 = static_cast<int>(ty * FP_TH);
    const uint16_t *in = A.in + static_cast<size_t>(f) * A.ifstride;
    MOS_PATH(MP_WG, threadIdx.x == 0u);
#ifdef MCRAW_POISON_M
    poison_tile(s_t, FP_LH * FP_LW);
#endif
    stage_tile<FP_TH, 2, fix_halo>(s_t, in, A.ipitch, W, H, x0, y0, A.invec != 0u);
    __syncthreads();
    const uint32_t lx = threadIdx.x % FP_LX, ly = threadIdx.x / FP_LX;
    const uint32_t x = static_cast<uint32_t>(x0) + 8u * lx;
    const uint32_t n = x < A.W ? min(8u, A.W - x) : 0u;
    MOS_PATH(MP_IDLE_LANE, n == 0u);
    // the lane's rows all have the parity of ly (y0 is even): its counters are those of two CFA positions
    const uint32_t rowpar = ly & 1u;
    const uint32_t blk[2] = {A.black[2u * rowpar], A.black[2u * rowpar + 1u]};
    const uint32_t abt[2] = {A.abs_thr[2u * rowpar], A.abs_thr[2u * rowpar + 1u]};
    uint32_t nhot[2] = {0u, 0u}, ncold[2] = {0u, 0u};
    uint16_t *fout = A.out + static_cast<size_t>(f) * A.ofstride + x;
#pragma unroll 1
    for (uint32_t pass = 0; pass < FP_TH / 16u; pass++) {
        const uint32_t rb = 16u * pass + 4u * (ly >> 1) + rowpar; // the lane's rows of the tile: rb and rb + 2
        MOS_PATH(MP_ROW_CONT, n != 0u && static_cast<uint32_t>(y0) + rb >= A.H);
        MOS_PATH(MP_ROW_CONT, n != 0u && static_cast<uint32_t>(y0) + rb + 2u >= A.H);
        if (n == 0u || static_cast<uint32_t>(y0) + rb >= A.H)
            continue;
        // LDS rows rb, rb + 2, rb + 4, rb + 6 are frame rows y - 2, y, y + 2, y + 4; w[.][j]: columns x - 2 + 2j, x - 1 + 2j
        uint32_t w[4][6];
#pragma unroll
        for (uint32_t a = 0; a < 4u; a++) {
            const uint16_t *lrow = &s_t[(rb + 2u * a) * FP_LW + 8u * lx];
            const mcraw_u32x4 c0 = *reinterpret_cast<const mcraw_u32x4 *>(lrow);
            const mcraw_u32x4 c1 = *reinterpret_cast<const mcraw_u32x4 *>(lrow + 8);
            const uint32_t c2 = *reinterpret_cast<const uint32_t *>(lrow + 16);
            w[a][0] = c0[3], w[a][1] = c1[0], w[a][2] = c1[1], w[a][3] = c1[2], w[a][4] = c1[3], w[a][5] = c2;
        }
#pragma unroll
        for (uint32_t a = 0; a < 2u; a++) {
            const uint32_t y = static_cast<uint32_t>(y0) + rb + 2u * a;
            if (y >= A.H)
                continue;
            const uint32_t(&R0)[6] = w[a], (&R1)[6] = w[a + 1u], (&R2)[6] = w[a + 2u];
            uint32_t o[4], Hk[4], Lk[4];
            bool cand = false;
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++) {
                // the eight neighbours of both pixels of dword k: NW N NE W E SW S SE
                const uint32_t nb[8] = {R0[k], R0[k + 1u], R0[k + 2u], R1[k], R1[k + 2u], R2[k], R2[k + 1u], R2[k + 2u]};
                uint32_t h1 = nb[0], h2 = 0u, l1 = nb[0], l2 = 0xFFFFFFFFu;
#pragma unroll
                for (uint32_t j = 1; j < 8u; j++) {
                    const uint32_t th = pk_min(h1, nb[j]), tl = pk_max(l1, nb[j]);
                    h1 = pk_max(h1, nb[j]);
                    h2 = pk_max(h2, th);
                    l1 = pk_min(l1, nb[j]);
                    l2 = pk_min(l2, tl);
                }
                Hk[k] = A.rank == 2u ? h2 : h1;
                Lk[k] = A.rank == 2u ? l2 : l1;
                const uint32_t v = R1[k + 1u];
                o[k] = v;
                // a half of v above its Hk or below its Lk: v - min(v, Hk) and max(v, Lk) - v are not both 0.
                // (Behind a cropped row end, 2k >= n, the LDS chunks were never staged and v, Hk, Lk are whatever LDS held:
                // such a dword can only send the lane into the slow path below for nothing, where every test, count and
                // store is guarded by the column's place against n.)
                cand = cand || (pk_sub(v, pk_min(v, Hk[k])) | pk_sub(pk_max(v, Lk[k]), v)) != 0u;
            }
#ifdef MCRAW_FORCE_SLOWM
            cand = true;
#endif
            MOS_WAVE(MP_FP_WAVE_ANY, __any(cand));
            MOS_WAVE(MP_FP_WAVE_NONE, !__any(cand));
            MOS_PATH(MP_FP_CAND, cand);
            if (__any(cand)) {
                if (cand) {
#pragma unroll
                    for (uint32_t k = 0; k < 4u; k++) {
                        const uint32_t v = R1[k + 1u];
                        uint32_t flag = 0u; // 0xFFFF in the halves that are replaced
#pragma unroll
                        for (uint32_t h = 0; h < 2u; h++) {
                            if (2u * k + h >= n)
                                continue;
                            const uint32_t pv = half16(v, h), ph = half16(Hk[k], h), pl = half16(Lk[k], h);
                            // (every intermediate is below 2^32: at most 65535 * 65535, then 65535 + 2^24)
                            const bool hot = A.hot && pv > ph && pv - ph > abt[h] + (((ph > blk[h] ? ph - blk[h] : 0u) * A.rel) >> 8);
                            const bool cold = A.cold && pv < pl && pl - pv > abt[h] + (((pl > blk[h] ? pl - blk[h] : 0u) * A.rel) >> 8);
                            MOS_PATH(MP_FP_HOT, hot);
                            MOS_PATH(MP_FP_COLD, cold);
                            if (hot || cold) {
                                flag |= 0xFFFFu << (16u * h);
                                // a pixel that the search finds in the list is not counted
#ifdef MCRAW_PATHSM
                                // (the census counts the search's answer: one search, kept in a local; the product's own
                                // form below compiles to other code with such a local)
                                const bool listed = A.counts && A.nlist && fix_member(A.list, A.nlist, (y << 16) | (x + 2u * k + h));
                                MOS_PATH(MP_FP_LISTED, listed);
                                if (A.counts && !listed) {
#else
                                if (A.counts && !(A.nlist && fix_member(A.list, A.nlist, (y << 16) | (x + 2u * k + h)))) {
#endif
                                    nhot[h] += hot ? 1u : 0u;
                                    ncold[h] += cold ? 1u : 0u;
                                }
                            }
                        }
                        MOS_PATH(MP_FP_FLAG, flag != 0u);
                        if (flag) {
                            uint32_t best, val;
                            fix_pair(R1[k], R1[k + 2u], true, best, val);       // (W, E)
                            fix_pair(R0[k + 1u], R2[k + 1u], false, best, val); // (N, S)
                            fix_pair(R0[k], R2[k + 2u], false, best, val);      // (NW, SE)
                            fix_pair(R0[k + 2u], R2[k], false, best, val);      // (NE, SW)
                            o[k] = (val & flag) | (v & ~flag);
                        }
                    }
                }
            }
            store8<NT>(fout + static_cast<size_t>(y) * A.opitch, n, A.outvec != 0u, o);
        }
    }
    if (!A.counts)
        return;
    // lanes 0 .. 31 of a wave hold one row parity, lanes 32 .. 63 the other: reduce each half, then lane 0 adds all eight
    uint32_t c[4] = {nhot[0], nhot[1], ncold[0], ncold[1]};
#pragma unroll
    for (uint32_t i = 0; i < 4u; i++) {
#pragma unroll
        for (int d = 16; d >= 1; d >>= 1)
            c[i] += __shfl_xor(c[i], d);
    }
    uint32_t other[4];
#pragma unroll
    for (uint32_t i = 0; i < 4u; i++)
        other[i] = __shfl(c[i], 32);
    if (__lane_id() == 0u) { // (an even ly: this half is row parity 0, the other one row parity 1)
        uint32_t *rec = A.counts + static_cast<size_t>(f) * 8u;
#pragma unroll
        for (uint32_t i = 0; i < 4u; i++) { // i: hot / cold, column parity
            if (c[i])
                atomicAdd(rec + 4u * (i >> 1) + (i & 1u), c[i]);
            if (other[i])
                atomicAdd(rec + 4u * (i >> 1) + 2u + (i & 1u), other[i]);
        }
    }
}

// Empty records.
__global__ void __launch_bounds__(256) kfixpix_init(uint32_t *counts, size_t words)
{
    const size_t step = static_cast<size_t>(gridDim.x) * blockDim.x;
    for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < words; i += step)
        counts[i] = 0u;
}

// The static list: one thread per (entry, frame).  Reads `in`, writes one element of `out` (behind kfixpix on the stream).
__global__ void __launch_bounds__(256) kfixpix_list(const FixArgs A)
{
    const uint32_t e = blockIdx.x * 256u + threadIdx.x, f = blockIdx.y;
    MOS_PATH(MP_FL_WG, threadIdx.x == 0u);
    MOS_PATH(MP_FL_PAST, e >= A.nlist);
    if (e >= A.nlist)
        return;
    const uint32_t key = gptr<const uint32_t>(A.list)[e];
    const int x = static_cast<int>(key & 0xFFFFu), y = static_cast<int>(key >> 16);
    const int W = static_cast<int>(A.W), H = static_cast<int>(A.H);
    MOS_PATH(MP_FL_OUTSIDE, x >= W || y >= H);
    if (x >= W || y >= H)
        return;
    const int xs[3] = {fix_neighbour(x, -2, W), x, fix_neighbour(x, 2, W)};
    const int ys[3] = {fix_neighbour(y, -2, H), y, fix_neighbour(y, 2, H)};
    const uint16_t *in = A.in + static_cast<size_t>(f) * A.ifstride;
    // (row, column) of the pairs' members in the contract's order: (W,E), (N,S), (NW,SE), (NE,SW)
    const int pa[4][2] = {{1, 0}, {0, 1}, {0, 0}, {0, 2}}, pb[4][2] = {{1, 2}, {2, 1}, {2, 2}, {2, 0}};
    uint32_t best = 0xFFFFFFFFu, val = 0u;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const int ya = ys[pa[k][0]], xa = xs[pa[k][1]], yb = ys[pb[k][0]], xb = xs[pb[k][1]];
        if (fix_member(A.list, A.nlist, (static_cast<uint32_t>(ya) << 16) | static_cast<uint32_t>(xa)) ||
            fix_member(A.list, A.nlist, (static_cast<uint32_t>(yb) << 16) | static_cast<uint32_t>(xb)))
            continue;
        const uint32_t a = gptr<const uint16_t>(in)[static_cast<size_t>(ya) * A.ipitch + static_cast<size_t>(xa)];
        const uint32_t b = gptr<const uint16_t>(in)[static_cast<size_t>(yb) * A.ipitch + static_cast<size_t>(xb)];
        const uint32_t d = a > b ? a - b : b - a;
        if (d < best)
            best = d, val = (a + b + 1u) >> 1;
    }
    MOS_PATH(MP_FL_WRITTEN, best != 0xFFFFFFFFu);
    MOS_PATH(MP_FL_NOPAIR, best == 0xFFFFFFFFu);
    if (best != 0xFFFFFFFFu) // no eligible pair: the dynamic pass's result stands
        gptr<uint16_t>(A.out)[static_cast<size_t>(f) * A.ofstride + static_cast<size_t>(y) * A.opitch + static_cast<size_t>(x)] =
            static_cast<uint16_t>(val);
}

} // namespace mcraw

using namespace mcraw;

extern "C" int mcraw_fixpix_batch(mcraw_ctx *c, const mcraw_fixpix *p, const uint16_t *in, size_t in_pitch, size_t in_frame_stride,
                                  int width, int height, int n, uint16_t *out, size_t out_pitch, size_t out_frame_stride,
                                  void *stream)
{
    if (!c || !p || n < 0)
        return reject(__func__, "bad arguments");
    if (n == 0)
        return 0;
    if (!in || !out)
        return reject(__func__, "in or out missing");
    const MosaicBatch I(in, in_pitch, in_frame_stride, static_cast<size_t>(n), width, height);
    const MosaicBatch O(out, out_pitch, out_frame_stride, static_cast<size_t>(n), width, height);
    if (const char *why = check(I, O))
        return reject(__func__, why);
    if (p->rank != 1u && p->rank != 2u)
        return reject(__func__, "rank must be 1 or 2");
    if (p->rel_thr > 65535u)
        return reject(__func__, "rel_thr must be 0 .. 65535 (Q8)");
    if (p->flags & ~(MCRAW_FIXPIX_HOT | MCRAW_FIXPIX_COLD))
        return reject(__func__, "unknown flag");
    if (p->nlist > FP_MAXLIST)
        return reject(__func__, "nlist above 1 << 20");
    if (p->nlist > 0u && (!p->list || (reinterpret_cast<uintptr_t>(p->list) & 3u)))
        return reject(__func__, "list missing or not 4-byte aligned");
    if (reinterpret_cast<uintptr_t>(p->counts) & 3u)
        return reject(__func__, "counts not 4-byte aligned");
    if (p->reserved[0] != 0u || p->reserved[1] != 0u)
        return reject(__func__, "reserved must be 0");
    if (overlap(I, O))
        return reject(__func__, "in and out overlap (every pixel reads its neighbours: there is no in-place form)");
    if (p->counts) {
        const uintptr_t ca = reinterpret_cast<uintptr_t>(p->counts), cb = static_cast<size_t>(n) * 32u;
        if (ranges_overlap(ca, cb, I.base, I.bytes()) || ranges_overlap(ca, cb, O.base, O.bytes()))
            return reject(__func__, "counts overlaps the input or the output");
    }

    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = stream_of(c, stream);
    FixArgs A{};
    A.list = p->nlist ? p->list : nullptr;
    A.nlist = p->nlist;
    A.ipitch = in_pitch;
    A.ifstride = in_frame_stride;
    A.opitch = out_pitch;
    A.ofstride = out_frame_stride;
    A.W = static_cast<uint32_t>(width);
    A.H = static_cast<uint32_t>(height);
    A.tilesX = (A.W + FP_TW - 1u) / FP_TW;
    const uint32_t tilesY = (A.H + FP_TH - 1u) / FP_TH;
    A.hot = (p->flags & MCRAW_FIXPIX_HOT) ? 1u : 0u;
    A.cold = (p->flags & MCRAW_FIXPIX_COLD) ? 1u : 0u;
    A.rank = p->rank;
    A.rel = p->rel_thr;
    for (int i = 0; i < 4; i++) {
        A.black[i] = p->black[i];
        A.abs_thr[i] = p->abs_thr[i];
    }
    A.invec = I.on_grid();
    A.outvec = O.on_grid();
    if (p->counts) {
        const size_t words = static_cast<size_t>(n) * 8u;
        const uint32_t blocks = static_cast<uint32_t>(std::min<size_t>((words + 255u) / 256u, 4096u));
        hipLaunchKernelGGL(kfixpix_init, dim3(blocks), dim3(256), 0, st, p->counts, words);
        HIP_TRY(hipGetLastError());
    }
    for (int f0 = 0; f0 < n; f0 += LAUNCH_PIECE) {
        const int nf = std::min<int>(LAUNCH_PIECE, n - f0);
        A.in = in + static_cast<size_t>(f0) * in_frame_stride;
        A.out = out + static_cast<size_t>(f0) * out_frame_stride;
        A.counts = p->counts ? p->counts + static_cast<size_t>(f0) * 8u : nullptr;
        hipLaunchKernelGGL(FP_NT ? kfixpix<true> : kfixpix<false>, dim3(A.tilesX * tilesY, static_cast<uint32_t>(nf)), dim3(FP_T), 0, st, A);
        HIP_TRY(hipGetLastError());
        if (A.nlist) {
            hipLaunchKernelGGL(kfixpix_list, dim3((A.nlist + 255u) / 256u, static_cast<uint32_t>(nf)), dim3(256), 0, st, A);
            HIP_TRY(hipGetLastError());
        }
    }
    return 0;
}
