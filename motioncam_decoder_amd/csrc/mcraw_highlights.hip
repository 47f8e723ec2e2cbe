// mcraw_highlights.hip -- gfx950 kernels for uint16 mosaics resident in HBM -> uint16 mosaics with the clipped highlights clipped
// to a neutral level or rebuilt from their neighbours (mcraw_highlights_batch), and the records of the colour that the rebuild
// keeps (mcraw_highlights_measure_batch).  The contract (integers only, bit-exact) is in include/mcraw_hip.h; DESIGN.md 31 has
// the design.
//
// khl_apply (REBUILD) and khl_measure: a workgroup owns a tile of HL_TW columns x HL_TH rows of one frame and stages it with a
// halo of one row and one column in LDS as raw samples (kfixpix's staging; the halo holds what the contract's reflection names).
// Lane (lx, ly) makes 8 columns of the rows ly, ly + 8, ..: all of one row parity, so its samples are those of two CFA positions
// and their parameters sit in registers.  khl_apply tests its 8 samples packed, on the dwords as they lie, against sat - 1 of
// the row's two positions; the neighbours' rows, the white-balanced values, the reference, the 64-bit multiply and the select all
// sit behind that predicate, so a wave without a clipped sample reads one LDS row and stores it.  The four divisions sum / cnt
// are made by four threads per workgroup while the others stage.  khl_measure keeps two sums and two counts per lane, reduces
// them over the 32 lanes of a row parity with shuffles, then over the workgroup in LDS, and adds the non-zero ones to the record
// with global atomics (kstats' way).  khl_clip (CLIP) is one packed min per dword and needs no neighbours: it loads and stores directly, as kshade does.
//
// Test builds (build.MOSAIC_PATH_VARIANTS, tests/test_gpu_mosaic_paths.py; why each is valid: the head of mcraw_mosaic_paths.h):
//   MCRAW_PATHSM       the path census
//   MCRAW_FORCE_SLOWM  khl_apply's `clipped` is true for every lane
//   MCRAW_POISON_M     s_t filled with 0xFFFF in front of staging
//   MCRAW_STAGE_FRAMES=N  the launch loop takes N frames at a time (mcraw_mosaic_paths.h: `frames2`)
#ifdef MCRAW_STAGE_FRAMES
#define LAUNCH_PIECE MCRAW_STAGE_FRAMES
#endif
#include "mcraw_host.h"
#include "mcraw_highlights_args.h"
#ifdef MCRAW_PATHSM
#include "mcraw_mosaic_paths.h"
#endif
#include "mcraw_mosaic.h"

namespace mcraw {

constexpr int HL_T = TILE_T;     // threads per workgroup
constexpr uint32_t HL_LX = 32u;  // lanes across a tile: 8 columns each
constexpr uint32_t HL_TW = TILE_W;
// Tile rows: 32 re-reads 34/32 of the rows with 18.1 KB of LDS, which still lets 8 workgroups (all 32 waves) onto a CU.
constexpr uint32_t HL_TH = 32u;
constexpr uint32_t HL_PASS = HL_T / HL_LX; // rows per pass (8: even, so a lane's rows share their parity)
constexpr uint32_t HL_LW = TILE_LW;
constexpr uint32_t HL_LH = HL_TH + 2u; // one halo row above and below
constexpr uint32_t HL_CTH = 16u;       // khl_clip: two rows per lane
static_assert(HL_TH % HL_PASS == 0u && HL_PASS % 2u == 0u, "whole passes, and a lane's rows of one parity");

// Streaming stores (`sc1 nt`) for the full aligned pieces of the output rows, which are written once: as kfixpix and kshade.
constexpr bool HL_NT = true;

struct HlArgs {
    const uint16_t *in;
    uint16_t *out;
    void *rec; // the record of the launch's first frame, or NULL
    size_t ipitch, ifstride, opitch, ofstride;
    uint32_t W, H, tilesX;
    uint32_t perframe; // one record per frame (else record 0 for all)
    uint32_t gdiag;    // 1: the green positions are those whose column and row parity differ; 0: those where they agree
    uint32_t top;
    uint32_t black[4], gain[4], inv[4];
    // by row parity, (even column | odd column << 16):
    uint32_t satm1[2]; // sat - 1: a sample is clipped when it is above
    uint32_t lo[2];    // measure
    uint32_t cap[2];   // CLIP: min(cap, 65535)
    uint32_t invec, outvec; // every 8-column piece of `in` / `out` lies on the 16-byte grid
};

// The frame coordinate that h in -1 .. n stands for: -1 -> 1, n -> n - 2 (n >= 2).  Coordinates no output reads are clamped.
__device__ __forceinline__ int hl_halo(int h, int n)
{
    h = h < 0 ? -h : h;
    h = h >= n ? 2 * n - 2 - h : h;
    return min(max(h, 0), n - 1);
}

// (both factors below 2^16)
__device__ __forceinline__ uint32_t hl_wbd(uint32_t s, uint32_t black, uint32_t gain)
{
    return (mul24(s > black ? s - black : 0u, gain) + 2048u) >> 12;
}

// The lane's parameters: [0] its own rows' two positions, [1] those of the rows above and below; then by column parity.
struct HlLane {
    uint32_t blk[2][2], gn[2][2];
    uint32_t rp, gdiag;
};

__device__ __forceinline__ HlLane hl_lane(const HlArgs &A, uint32_t rp)
{
    HlLane P;
#pragma unroll
    for (uint32_t a = 0; a < 2u; a++)
#pragma unroll
        for (uint32_t c = 0; c < 2u; c++) {
            P.blk[a][c] = (rp ^ a) ? A.black[2u + c] : A.black[c];
            P.gn[a][c] = (rp ^ a) ? A.gain[2u + c] : A.gain[c];
        }
    P.rp = rp, P.gdiag = A.gdiag;
    return P;
}

// Three LDS rows around the lane's 8 columns: w[a][j] holds columns x - 2 + 2j and x - 1 + 2j of frame row y - 1 + a.
__device__ __forceinline__ void hl_rows(const uint16_t *s_t, uint32_t r, uint32_t lx, uint32_t w[3][6])
{
#pragma unroll
    for (uint32_t a = 0; a < 3u; a++) {
        const uint16_t *lrow = &s_t[(r + a) * HL_LW + 8u * lx];
        const mcraw_u32x4 c0 = *reinterpret_cast<const mcraw_u32x4 *>(lrow);
        const mcraw_u32x4 c1 = *reinterpret_cast<const mcraw_u32x4 *>(lrow + 8);
        const uint32_t c2 = *reinterpret_cast<const uint32_t *>(lrow + 16);
        w[a][0] = c0[3], w[a][1] = c1[0], w[a][2] = c1[1], w[a][3] = c1[2], w[a][4] = c1[3], w[a][5] = c2;
    }
}

// The sample of row a at column x + i (i: -1 .. 8, a compile-time constant wherever it is called)
__device__ __forceinline__ uint32_t hl_at(const uint32_t w[3][6], uint32_t a, int i)
{
    return half16(w[a][(i + 2) >> 1], static_cast<uint32_t>(i + 2) & 1u);
}

// The contract's reference at column x + i of the middle row.
__device__ __forceinline__ uint32_t hl_ref(const uint32_t w[3][6], int i, const HlLane &P)
{
    const uint32_t c = static_cast<uint32_t>(i) & 1u, o = c ^ 1u;
    const uint32_t Hm = (hl_wbd(hl_at(w, 1, i - 1), P.blk[0][o], P.gn[0][o]) + hl_wbd(hl_at(w, 1, i + 1), P.blk[0][o], P.gn[0][o]) + 1u) >> 1;
    const uint32_t Vm = (hl_wbd(hl_at(w, 0, i), P.blk[1][c], P.gn[1][c]) + hl_wbd(hl_at(w, 2, i), P.blk[1][c], P.gn[1][c]) + 1u) >> 1;
    const uint32_t hv = (Hm + Vm + 1u) >> 1;
    if ((c ^ P.rp) == P.gdiag) // a green position
        return hv;
    const uint32_t Dm = (hl_wbd(hl_at(w, 0, i - 1), P.blk[1][o], P.gn[1][o]) + hl_wbd(hl_at(w, 0, i + 1), P.blk[1][o], P.gn[1][o]) +
                         hl_wbd(hl_at(w, 2, i - 1), P.blk[1][o], P.gn[1][o]) + hl_wbd(hl_at(w, 2, i + 1), P.blk[1][o], P.gn[1][o]) + 2u) >> 2;
    return (hv + Dm + 1u) >> 1;
}

template <bool NT>
__global__ void __launch_bounds__(HL_T) khl_apply(const HlArgs A)
{
    __shared__ __attribute__((aligned(16))) uint16_t s_t[HL_LH * HL_LW];
    __shared__ int32_t s_ch[4];
    const uint32_t tile = blockIdx.x, f = blockIdx.y;
    const uint32_t ty = tile / A.tilesX, tx = tile - ty * A.tilesX;
    const int W = static_cast<int>(A.W), H = static_cast<int>(A.H);
    const int x0 = static_cast<int>(tx * HL_TW), y0 = static_cast<int>(ty * HL_TH);
    // the record's loads are in flight while the tile is staged
    long long sum = 0;
    uint32_t cnt = 0u;
    if (A.rec && threadIdx.x < 4u) {
        const char *rec = static_cast<const char *>(A.rec) + (A.perframe ? static_cast<size_t>(f) * HL_REC_BYTES : 0u);
        sum = gptr<const long long>(rec)[threadIdx.x];
        cnt = gptr<const uint32_t>(rec)[8u + threadIdx.x];
    }
    const uint16_t *in = A.in + static_cast<size_t>(f) * A.ifstride;
    MOS_PATH(MP_WG, threadIdx.x == 0u);
#ifdef MCRAW_POISON_M
    poison_tile(s_t, HL_LH * HL_LW);
#endif
    stage_tile<HL_TH, 1, hl_halo>(s_t, in, A.ipitch, W, H, x0, y0, A.invec != 0u);
    if (threadIdx.x < 4u) {
        long long c = cnt ? sum / static_cast<long long>(cnt) : 0;
        c = c < -HL_CHROMA_MAX ? -HL_CHROMA_MAX : c > HL_CHROMA_MAX ? HL_CHROMA_MAX : c;
        s_ch[threadIdx.x] = static_cast<int32_t>(c);
    }
    __syncthreads();
    const uint32_t lx = threadIdx.x % HL_LX, ly = threadIdx.x / HL_LX;
    const uint32_t x = static_cast<uint32_t>(x0) + 8u * lx;
    const uint32_t n = x < A.W ? min(8u, A.W - x) : 0u;
    const uint32_t rp = ly & 1u; // y0 and HL_PASS are even: every row of the lane has this parity
    const uint32_t satm1 = A.satm1[rp];
    MOS_PATH(MP_IDLE_LANE, n == 0u);
    uint16_t *fout = A.out + static_cast<size_t>(f) * A.ofstride + x;
#pragma unroll 1
    for (uint32_t pass = 0; pass < HL_TH / HL_PASS; pass++) {
        const uint32_t r = HL_PASS * pass + ly, y = static_cast<uint32_t>(y0) + r;
        MOS_PATH(MP_ROW_CONT, n != 0u && y >= A.H);
        if (n == 0u || y >= A.H)
            continue;
        const mcraw_u32x4 own = *reinterpret_cast<const mcraw_u32x4 *>(&s_t[(r + 1u) * HL_LW + 8u + 8u * lx]);
        uint32_t o[4] = {own[0], own[1], own[2], own[3]};
        // a half above sat - 1: s - min(s, sat - 1) is not 0.  (Behind a cropped row end the chunks were never staged and o is
        // whatever LDS held: that can only send the lane into the slow path for nothing, where every pixel is guarded by n.)
        bool clipped = false;
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++)
            clipped = clipped || pk_sub(o[k], pk_min(o[k], satm1)) != 0u;
#ifdef MCRAW_FORCE_SLOWM
        clipped = true;
#endif
        MOS_PATH(MP_HL_CLIPPED, clipped);
        MOS_PATH(MP_HL_UNCLIPPED, !clipped);
        if (clipped) {
            const HlLane P = hl_lane(A, rp);
            uint32_t w[3][6];
            hl_rows(s_t, r, lx, w);
#pragma unroll
            for (int i = 0; i < 8; i++) {
                const uint32_t c = static_cast<uint32_t>(i) & 1u;
                const uint32_t s = half16(o[i >> 1], c);
                if (static_cast<uint32_t>(i) >= n || s <= half16(satm1, c))
                    continue;
                const int32_t v = static_cast<int32_t>(hl_wbd(s, P.blk[0][c], P.gn[0][c]));
                const int32_t cand = static_cast<int32_t>(hl_ref(w, i, P)) + s_ch[2u * rp + c];
                MOS_PATH(MP_HL_LEFT, cand <= v);
                MOS_PATH(MP_HL_REBUILT, cand > v);
                if (cand <= v)
                    continue;
                // (cand <= 2^21 and inv <= 2^16: the product needs 64 bits, the result is below 2^26)
                const uint32_t inv = rp ? A.inv[2u + c] : A.inv[c];
                const uint32_t back = P.blk[0][c] + static_cast<uint32_t>((static_cast<uint64_t>(static_cast<uint32_t>(cand)) * inv + 2048u) >> 12);
                MOS_PATH(MP_HL_TOP, back > A.top);
                const uint32_t q = max(s, min(back, A.top));
                o[i >> 1] = c ? (o[i >> 1] & 0xFFFFu) | (q << 16) : (o[i >> 1] & 0xFFFF0000u) | q;
            }
        }
        store8<NT>(fout + static_cast<size_t>(y) * A.opitch, n, A.outvec != 0u, o);
    }
}

__global__ void __launch_bounds__(HL_T) khl_measure(const HlArgs A)
{
    __shared__ __attribute__((aligned(16))) uint16_t s_t[HL_LH * HL_LW];
    __shared__ unsigned long long s_sum[4]; // the workgroup's sums (two's complement) and counts by CFA position
    __shared__ uint32_t s_cnt[4];
    const uint32_t tile = blockIdx.x, f = blockIdx.y;
    const uint32_t ty = tile / A.tilesX, tx = tile - ty * A.tilesX;
    const int W = static_cast<int>(A.W), H = static_cast<int>(A.H);
    const int x0 = static_cast<int>(tx * HL_TW), y0 = static_cast<int>(ty * HL_TH);
    const uint16_t *in = A.in + static_cast<size_t>(f) * A.ifstride;
    if (threadIdx.x < 4u)
        s_sum[threadIdx.x] = 0ull, s_cnt[threadIdx.x] = 0u;
    MOS_PATH(MP_WG, threadIdx.x == 0u);
#ifdef MCRAW_POISON_M
    poison_tile(s_t, HL_LH * HL_LW);
#endif
    stage_tile<HL_TH, 1, hl_halo>(s_t, in, A.ipitch, W, H, x0, y0, A.invec != 0u);
    __syncthreads();
    const uint32_t lx = threadIdx.x % HL_LX, ly = threadIdx.x / HL_LX;
    const uint32_t x = static_cast<uint32_t>(x0) + 8u * lx;
    const uint32_t n = x < A.W ? min(8u, A.W - x) : 0u;
    const uint32_t rp = ly & 1u;
    MOS_PATH(MP_IDLE_LANE, n == 0u);
    const HlLane P = hl_lane(A, rp);
    // sat - 1 and lo of the lane's own rows [0] and of the rows above and below [1], by column parity
    uint32_t sm[2][2], lo[2];
#pragma unroll
    for (uint32_t c = 0; c < 2u; c++) {
        sm[0][c] = half16(A.satm1[rp], c);
        sm[1][c] = half16(A.satm1[rp ^ 1u], c);
        lo[c] = half16(A.lo[rp], c);
    }
    // a lane sees at most HL_TH / HL_PASS * 8 = 32 pixels of |v - ref| < 2^20: 32 bits hold its sums, and those of 32 lanes
    int32_t acc[2] = {0, 0};
    uint32_t cnt[2] = {0u, 0u};
#pragma unroll 1
    for (uint32_t pass = 0; pass < HL_TH / HL_PASS; pass++) {
        const uint32_t r = HL_PASS * pass + ly, y = static_cast<uint32_t>(y0) + r;
        MOS_PATH(MP_ROW_CONT, n != 0u && y >= A.H);
        if (n == 0u || y >= A.H)
            continue;
        uint32_t w[3][6];
        hl_rows(s_t, r, lx, w);
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const uint32_t c = static_cast<uint32_t>(i) & 1u, o = c ^ 1u;
            const uint32_t s = hl_at(w, 1, i);
            MOS_PATH(MP_HM_OWN, static_cast<uint32_t>(i) < n && (s < lo[c] || s > sm[0][c]));
            if (static_cast<uint32_t>(i) >= n || s < lo[c] || s > sm[0][c])
                continue;
            MOS_PATH(MP_HM_NEIGHBOUR,
                     hl_at(w, 1, i - 1) > sm[0][o] || hl_at(w, 1, i + 1) > sm[0][o] || hl_at(w, 0, i) > sm[1][c] || hl_at(w, 2, i) > sm[1][c] ||
                         hl_at(w, 0, i - 1) > sm[1][o] || hl_at(w, 0, i + 1) > sm[1][o] || hl_at(w, 2, i - 1) > sm[1][o] || hl_at(w, 2, i + 1) > sm[1][o]);
            if (hl_at(w, 1, i - 1) > sm[0][o] || hl_at(w, 1, i + 1) > sm[0][o] || hl_at(w, 0, i) > sm[1][c] || hl_at(w, 2, i) > sm[1][c] ||
                hl_at(w, 0, i - 1) > sm[1][o] || hl_at(w, 0, i + 1) > sm[1][o] || hl_at(w, 2, i - 1) > sm[1][o] || hl_at(w, 2, i + 1) > sm[1][o])
                continue;
            MOS_PATH(MP_HM_MEASURED, true);
            acc[c] += static_cast<int32_t>(hl_wbd(s, P.blk[0][c], P.gn[0][c])) - static_cast<int32_t>(hl_ref(w, i, P));
            cnt[c] += 1u;
        }
    }
    // lanes 0 .. 31 of a wave hold one row parity, lanes 32 .. 63 the other: reduce each half, its first lane adds its two to the
    // workgroup's in LDS (64 bits: eight halves of up to 2^30 each), and four threads add the non-zero ones to the record: 8 global
    // atomics per workgroup at most, all of a frame's on one line
#pragma unroll
    for (uint32_t c = 0; c < 2u; c++) {
#pragma unroll
        for (int d = 16; d >= 1; d >>= 1) {
            acc[c] += __shfl_xor(acc[c], d);
            cnt[c] += __shfl_xor(cnt[c], d);
        }
    }
    if ((__lane_id() & 31u) == 0u) {
#pragma unroll
        for (uint32_t c = 0; c < 2u; c++)
            if (cnt[c]) { // (two's complement: adding the sign-extended sum as unsigned is the signed addition)
                atomicAdd(&s_sum[2u * rp + c], static_cast<unsigned long long>(static_cast<long long>(acc[c])));
                atomicAdd(&s_cnt[2u * rp + c], cnt[c]);
            }
    }
    __syncthreads();
    if (threadIdx.x < 4u && s_cnt[threadIdx.x]) {
        char *rec = static_cast<char *>(A.rec) + (A.perframe ? static_cast<size_t>(f) * HL_REC_BYTES : 0u);
        atomicAdd(reinterpret_cast<unsigned long long *>(rec) + threadIdx.x, s_sum[threadIdx.x]);
        atomicAdd(reinterpret_cast<uint32_t *>(rec + 32) + threadIdx.x, s_cnt[threadIdx.x]);
    }
}

// Empty records.
__global__ void __launch_bounds__(256) khl_init(uint32_t *rec, size_t words)
{
    const size_t step = static_cast<size_t>(gridDim.x) * blockDim.x;
    for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < words; i += step)
        rec[i] = 0u;
}

// CLIP: every lane 8 columns of two rows, a 16-byte load and a 16-byte store each.
template <bool NT>
__global__ void __launch_bounds__(HL_T) khl_clip(const HlArgs A)
{
    const uint32_t tile = blockIdx.x, f = blockIdx.y;
    const uint32_t ty = tile / A.tilesX, tx = tile - ty * A.tilesX;
    const uint32_t lx = threadIdx.x % HL_LX, ly = threadIdx.x / HL_LX;
    const uint32_t x = tx * HL_TW + 8u * lx, y0 = ty * HL_CTH + ly;
    MOS_PATH(MP_WG, threadIdx.x == 0u);
    MOS_PATH(MP_IDLE_LANE, x >= A.W);
    if (x >= A.W)
        return;
    const uint32_t n = min(8u, A.W - x);
    const uint16_t *fin = A.in + static_cast<size_t>(f) * A.ifstride + x;
    uint16_t *fout = A.out + static_cast<size_t>(f) * A.ofstride + x;
    uint32_t p[2][4];
#pragma unroll
    for (uint32_t a = 0; a < 2u; a++) {
        const uint32_t y = y0 + a * HL_PASS;
        if (y < A.H)
            load8(fin + static_cast<size_t>(y) * A.ipitch, n, A.invec != 0u, p[a]);
    }
    const uint32_t cap = A.cap[y0 & 1u]; // (HL_PASS is even: both rows have this parity)
#pragma unroll
    for (uint32_t a = 0; a < 2u; a++) {
        const uint32_t y = y0 + a * HL_PASS;
        MOS_PATH(MP_ROW_CONT, y >= A.H);
        if (y >= A.H)
            continue;
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++)
            p[a][k] = pk_min(p[a][k], cap);
        store8<NT>(fout + static_cast<size_t>(y) * A.opitch, n, A.outvec != 0u, p[a]);
    }
}

// The struct and what the host derives from it, as the kernels take it.
static HlArgs hl_args(const mcraw_highlights &h, const MosaicBatch &I, const MosaicBatch *O)
{
    const HlDerived d = hl_derive(h);
    HlArgs A{};
    A.ipitch = I.pitch;
    A.ifstride = I.fstride;
    A.W = static_cast<uint32_t>(I.W);
    A.H = static_cast<uint32_t>(I.H);
    A.tilesX = (A.W + HL_TW - 1u) / HL_TW;
    A.perframe = h.nrec > 1u ? 1u : 0u;
    A.gdiag = h.cfa < 2u ? 1u : 0u;
    A.top = h.top;
    for (int p = 0; p < 4; p++) {
        A.black[p] = h.black[p];
        A.gain[p] = h.gain[p];
        A.inv[p] = d.inv[p];
    }
    for (int r = 0; r < 2; r++) {
        A.satm1[r] = (h.sat[2 * r] - 1u) | ((h.sat[2 * r + 1] - 1u) << 16);
        A.lo[r] = h.lo[2 * r] | (static_cast<uint32_t>(h.lo[2 * r + 1]) << 16);
        A.cap[r] = std::min(d.cap[2 * r], 65535u) | (std::min(d.cap[2 * r + 1], 65535u) << 16);
    }
    A.invec = I.on_grid();
    if (O) {
        A.opitch = O->pitch;
        A.ofstride = O->fstride;
        A.outvec = O->on_grid();
    }
    return A;
}

} // namespace mcraw

using namespace mcraw;

extern "C" int mcraw_highlights_measure_batch(mcraw_ctx *c, const mcraw_highlights *h, const uint16_t *in, size_t in_pitch,
                                              size_t in_frame_stride, int width, int height, int n, void *stream)
{
    if (!c || !h || n < 0)
        return reject(__func__, "bad arguments");
    if (n == 0)
        return 0;
    if (!in)
        return reject(__func__, "in missing");
    const MosaicBatch I(in, in_pitch, in_frame_stride, static_cast<size_t>(n), width, height);
    if (const char *why = hl_check_batches(I, nullptr))
        return reject(__func__, why);
    if (const char *why = hl_check(*h, static_cast<size_t>(n), true))
        return reject(__func__, why);
    if (hl_rec_overlaps(*h, I))
        return reject(__func__, "rec overlaps the input");

    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = stream_of(c, stream);
    HlArgs A = hl_args(*h, I, nullptr);
    const uint32_t tilesY = (A.H + HL_TH - 1u) / HL_TH;
    if (!(h->flags & MCRAW_HL_ACCUMULATE)) {
        const size_t words = static_cast<size_t>(h->nrec) * (HL_REC_BYTES / 4u);
        const uint32_t blocks = static_cast<uint32_t>(std::min<size_t>((words + 255u) / 256u, 4096u));
        hipLaunchKernelGGL(khl_init, dim3(blocks), dim3(256), 0, st, static_cast<uint32_t *>(h->rec), words);
        HIP_TRY(hipGetLastError());
    }
    for (int f0 = 0; f0 < n; f0 += LAUNCH_PIECE) {
        const int nf = std::min<int>(LAUNCH_PIECE, n - f0);
        A.in = in + static_cast<size_t>(f0) * in_frame_stride;
        A.rec = static_cast<char *>(h->rec) + (A.perframe ? static_cast<size_t>(f0) * HL_REC_BYTES : 0u);
        hipLaunchKernelGGL(khl_measure, dim3(A.tilesX * tilesY, static_cast<uint32_t>(nf)), dim3(HL_T), 0, st, A);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

extern "C" int mcraw_highlights_batch(mcraw_ctx *c, const mcraw_highlights *h, const uint16_t *in, size_t in_pitch, size_t in_frame_stride,
                                      int width, int height, int n, uint16_t *out, size_t out_pitch, size_t out_frame_stride,
                                      void *stream)
{
    if (!c || !h || n < 0)
        return reject(__func__, "bad arguments");
    if (n == 0)
        return 0;
    if (!in || !out)
        return reject(__func__, "in or out missing");
    const MosaicBatch I(in, in_pitch, in_frame_stride, static_cast<size_t>(n), width, height);
    const MosaicBatch O(out, out_pitch, out_frame_stride, static_cast<size_t>(n), width, height);
    if (const char *why = hl_check_batches(I, &O))
        return reject(__func__, why);
    if (const char *why = hl_check(*h, static_cast<size_t>(n), false))
        return reject(__func__, why);
    if (overlap(I, O))
        return reject(__func__, "in and out overlap (every pixel reads its neighbours: there is no in-place form)");
    if (hl_rec_overlaps(*h, I) || hl_rec_overlaps(*h, O))
        return reject(__func__, "rec overlaps the input or the output");

    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = stream_of(c, stream);
    HlArgs A = hl_args(*h, I, &O);
    const bool clip = h->mode == MCRAW_HL_CLIP;
    const uint32_t tilesY = (A.H + (clip ? HL_CTH : HL_TH) - 1u) / (clip ? HL_CTH : HL_TH);
    for (int f0 = 0; f0 < n; f0 += LAUNCH_PIECE) {
        const int nf = std::min<int>(LAUNCH_PIECE, n - f0);
        A.in = in + static_cast<size_t>(f0) * in_frame_stride;
        A.out = out + static_cast<size_t>(f0) * out_frame_stride;
        A.rec = h->nrec ? static_cast<char *>(h->rec) + (A.perframe ? static_cast<size_t>(f0) * HL_REC_BYTES : 0u) : nullptr;
        const dim3 grid(A.tilesX * tilesY, static_cast<uint32_t>(nf));
        if (clip)
            hipLaunchKernelGGL(khl_clip<HL_NT>, grid, dim3(HL_T), 0, st, A);
        else
            hipLaunchKernelGGL(khl_apply<HL_NT>, grid, dim3(HL_T), 0, st, A);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}
