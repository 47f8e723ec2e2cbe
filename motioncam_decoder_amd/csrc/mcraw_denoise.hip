// mcraw_denoise.hip -- gfx950 kernel for uint16 mosaics resident in HBM -> noise-adaptively smoothed uint16 mosaics
// (mcraw_denoise_batch).  The contract (integers only, bit-exact) is in include/mcraw_hip.h; DESIGN.md 19 has the design.
//
// kdenoise<RADIUS, NT>: a workgroup owns a tile of DN_TW columns x DN_TH rows of one frame and stages it with a halo of
// 2 * RADIUS rows and columns in LDS as raw samples, 16-byte chunks on the frame's 8-column grid (kfixpix's staging), and
// the frame's table behind it.  The halo holds what the contract's reflection names for the pixel at distance 2 (the two
// coordinates next to the frame) or 4 (the two beyond); the pixels 2 and 3 from an edge, whose distance-4 neighbour falls on
// a coordinate that belongs to the distance-2 reader, take their opposite distance-4 neighbour instead, which the rule
// makes the same sample.  Lane (lx, ly) makes 8 columns of rows ly, ly + 8, ...: for each of the 2R + 1 LDS
// rows it reads 8 + 4R samples and accumulates, for all 8 pixels, q = x * x, q * a and a over the 2R + 1 columns.  The
// centre counts as a neighbour of itself (x = 0, weight 256): that is the contract's 256 * c and 256.  |a - c| runs packed
// on the dwords as they lie in memory; every product has a factor below 2^24.
//
// Test builds (build.MOSAIC_PATH_VARIANTS, tests/test_gpu_mosaic_paths.py; why each is valid: the head of mcraw_mosaic_paths.h):
//   MCRAW_PATHSM      the path census, and the sweep of div_round at the end of this file
//   MCRAW_POISON_M    s_t filled with 0xFFFF in front of staging
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

constexpr int DN_T = TILE_T;     // threads per workgroup
constexpr uint32_t DN_LX = 32u;  // lanes across a tile: 8 columns each
constexpr uint32_t DN_LY = DN_T / DN_LX;
constexpr uint32_t DN_TW = TILE_W;
// Tile rows: 32 re-reads 40/32 of the rows at radius 2 (21.3 KB of LDS), 16 re-reads 24/16 (12.8 KB).
// -DMCRAW_DENOISE_TH=16 builds the other one; tools/bench_denoise.py --alt-lib runs two builds side by side.
#ifndef MCRAW_DENOISE_TH
#define MCRAW_DENOISE_TH 32
#endif
constexpr uint32_t DN_TH = MCRAW_DENOISE_TH;
static_assert(DN_TH == 16u || DN_TH == 32u, "the lanes' rows are DN_LY apart: the tile is a multiple of it");
constexpr uint32_t DN_LW = TILE_LW;     // LDS row: 8 columns either side (2 * RADIUS used), so that chunks stay on the 8-grid
constexpr uint32_t DN_CH = TILE_CH;     // 16-byte chunks per LDS row

// Which stores the full aligned pieces of the output rows use: `sc1 nt` streaming stores (store_stream16) or plain ones.
// -DMCRAW_DENOISE_FLIP_STORES builds the other one.
#ifdef MCRAW_DENOISE_FLIP_STORES
constexpr bool DN_NT = false;
#else
constexpr bool DN_NT = true;
#endif

struct DnArgs {
    const uint16_t *in;
    uint16_t *out;
    const uint16_t *lut; // the launch's first table
    size_t ipitch, ifstride, opitch, ofstride;
    uint32_t W, H, tilesX;
    uint32_t amount, L, shift, perframe;
    uint32_t invec, outvec; // every 8-column piece of `in` / `out` lies on the 16-byte grid
};

// The frame coordinate whose sample the halo coordinate h stands for.  h in {-2, -1} is read at distance 2 by c = h + 2, h in
// {-4, -3} at distance 4 by c = h + 4 (and mirrored on the high side): the contract's c - d, or c itself where that leaves
// the frame too.  (h in {-2, -1} is also where c = 2, 3 would look at distance 4: those pixels do not, see dn_swap.)
// Coordinates no output reads are clamped.
__device__ __forceinline__ int dn_halo(int h, int n)
{
    if (h < -2)
        h = h + 8 < n ? h + 8 : h + 4;
    else if (h < 0)
        h = h + 4 < n ? h + 4 : h + 2;
    else if (h >= n + 2)
        h = h - 8 >= 0 ? h - 8 : h - 4;
    else if (h >= n)
        h = h - 4 >= 0 ? h - 4 : h - 2;
    return min(max(h, 0), n - 1);
}

// Which way a pixel at coordinate c looks for its neighbours at distance 4.  c - 4 in {-2, -1} and c + 4 in {n, n + 1} are
// halo coordinates that hold the distance-2 reader's sample.  For such a c the contract's rule gives the neighbours at -4
// and at +4 the same coordinate (c - 4 is outside, so -4 means c + 4 or c, and +4 means c + 4 or, c - 4 being outside, c;
// likewise on the high side), so the pixel reads the other side: bit 0 = take +4 for -4, bit 1 = take -4 for +4, both = the
// pixel itself for both (n = 5, 6, 7: c = 2 of n = 5 has neither c - 4 nor c + 4 inside).
__device__ __forceinline__ uint32_t dn_swap(int c, int n)
{
    return ((c & ~1) == 2 ? 1u : 0u) | (static_cast<uint32_t>(c + 4 - n) < 2u ? 2u : 0u);
}

template <int RADIUS, bool NT>
__global__ void __launch_bounds__(DN_T) kdenoise(const DnArgs A)
{
    constexpr int HALO = 2 * RADIUS;
    constexpr uint32_t NP = 2u * RADIUS + 1u;       // neighbours per axis, the centre among them
    constexpr uint32_t NW = 4u + 2u * RADIUS;       // dwords of an LDS row that a lane reads: columns x - HALO .. x + 7 + HALO
    constexpr uint32_t LH = DN_TH + 2u * HALO;
    __shared__ __attribute__((aligned(16))) uint16_t s_t[LH * DN_LW];          // the tile and its halo
    extern __shared__ __attribute__((aligned(16))) uint16_t dn_lut[];          // the frame's table: 4 * L entries (the launch sizes it)
    const uint32_t tile = blockIdx.x, f = blockIdx.y;
    const uint32_t ty = tile / A.tilesX, tx = tile - ty * A.tilesX;
    const int W = static_cast<int>(A.W), H = static_cast<int>(A.H);
    const int x0 = static_cast<int>(tx * DN_TW), y0 = static_cast<int>(ty * DN_TH);
    const uint16_t *in = A.in + static_cast<size_t>(f) * A.ifstride;
    MOS_PATH(MP_WG, threadIdx.x == 0u);
#ifdef MCRAW_POISON_M
    poison_tile(s_t, LH * DN_LW);
#endif
    {
        const uint16_t *lut = A.lut + (A.perframe ? static_cast<size_t>(f) * 4u * A.L : 0u);
        for (uint32_t i = threadIdx.x; i < A.L / 2u; i += DN_T) // 4 * L * 2 bytes in 16-byte chunks (L >= 64)
            *reinterpret_cast<mcraw_u32x4 *>(&dn_lut[8u * i]) = *gptr<const mcraw_u32x4>(lut + 8u * i);
    }
    // (stage_tile of mcraw_mosaic.h, written out: as a call it measured slower in this kernel)
    for (uint32_t i = threadIdx.x; i < LH * DN_CH; i += DN_T) {
        const uint32_t r = i / DN_CH, q = i % DN_CH;
        const int yy = y0 - HALO + static_cast<int>(r), xs = x0 - 8 + 8 * static_cast<int>(q);
        MOS_PATH(MP_STG_SKIP, yy >= H + HALO || xs >= W + HALO);
        if (yy >= H + HALO || xs >= W + HALO) // no output of the frame reads it
            continue;
        MOS_STAGE(q != 0u && q != DN_CH - 1u, xs + 8 <= W, A.invec != 0u);
        const uint16_t *row = in + static_cast<size_t>(dn_halo(yy, H)) * A.ipitch;
        mcraw_u32x4 v;
        if (q != 0u && q != DN_CH - 1u && xs + 8 <= W) { // (xs >= 0 here) a full piece of the row
            v = load16(row + xs, A.invec != 0u);
        } else { // the halo columns (the last HALO of the first chunk, the first HALO of the last) and a cropped row end:
                 // element loads through the reflection
            const int e0 = q == 0u ? 8 - HALO : 0, e1 = q == DN_CH - 1u ? HALO : 8;
            uint32_t u[8];
#pragma unroll
            for (int e = 0; e < 8; e++)
                u[e] = (e >= e0 && e < e1 && xs + e < W + HALO) ? gptr<const uint16_t>(row)[dn_halo(xs + e, W)] : 0u;
            v = mcraw_u32x4{u[0] | (u[1] << 16), u[2] | (u[3] << 16), u[4] | (u[5] << 16), u[6] | (u[7] << 16)};
        }
        *reinterpret_cast<mcraw_u32x4 *>(&s_t[r * DN_LW + 8u * q]) = v;
    }
    __syncthreads();
    const uint32_t lx = threadIdx.x % DN_LX, ly = threadIdx.x / DN_LX;
    const uint32_t x = static_cast<uint32_t>(x0) + 8u * lx;
    const uint32_t n = x < A.W ? min(8u, A.W - x) : 0u;
    MOS_PATH(MP_IDLE_LANE, n == 0u);
    if (n == 0u)
        return;
    // the lane's rows all have the parity of ly (y0 and DN_LY are even): two of the table's four planes
    const uint16_t *plane[2] = {dn_lut + (2u * (ly & 1u)) * A.L, dn_lut + (2u * (ly & 1u) + 1u) * A.L};
    // radius 2: the halves of the lane's dwords whose distance-4 neighbours along the row are taken from the other side
    uint32_t mlo[4] = {0u, 0u, 0u, 0u}, mhi[4] = {0u, 0u, 0u, 0u};
    bool edgex = false;
    if (RADIUS == 2) {
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++)
#pragma unroll
            for (uint32_t h = 0; h < 2u; h++) {
                const uint32_t s = dn_swap(static_cast<int>(x + 2u * k + h), W);
                mlo[k] |= (s & 1u) ? 0xFFFFu << (16u * h) : 0u;
                mhi[k] |= (s & 2u) ? 0xFFFFu << (16u * h) : 0u;
                edgex = edgex || s != 0u;
            }
        MOS_PATH(MP_DN_EDGEX, edgex);
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++)
            MOS_PATH(MP_DN_BOTH, (mlo[k] & mhi[k]) != 0u);
    }
    uint16_t *fout = A.out + static_cast<size_t>(f) * A.ofstride + x;
    const uint32_t lmax = A.L - 1u;
#pragma unroll 1
    for (uint32_t rr = ly; rr < DN_TH; rr += DN_LY) {
        const uint32_t y = static_cast<uint32_t>(y0) + rr;
        MOS_PATH(MP_ROW_BREAK, y >= A.H);
        if (y >= A.H)
            break;
        const uint32_t sy = RADIUS == 2 ? dn_swap(static_cast<int>(y), H) : 0u;
        MOS_PATH(MP_DN_SY1, (sy & 1u) != 0u);
        MOS_PATH(MP_DN_SY2, (sy & 2u) != 0u);
        MOS_PATH(MP_DN_SY3, sy == 3u);
        const uint16_t *lane = &s_t[(rr + HALO) * DN_LW + 8u * lx + 8u - HALO]; // the pixel row, column x - HALO
        uint32_t c[4], rv[8];
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) {
            c[k] = *reinterpret_cast<const uint32_t *>(lane + HALO + 2u * k);
#pragma unroll
            for (uint32_t h = 0; h < 2u; h++)
                rv[2u * k + h] = plane[h][min(half16(c[k], h) >> A.shift, lmax)];
        }
        uint32_t sq[8], sqa[8], sa[8];
#pragma unroll
        for (uint32_t p = 0; p < 8u; p++)
            sq[p] = sqa[p] = sa[p] = 0u;
#pragma unroll 1
        for (uint32_t j = 0; j < NP; j++) {
            int dy = 2 * (static_cast<int>(j) - RADIUS);
            if (RADIUS == 2) { // the row at distance 4 that the halo cannot serve: the opposite one, or the pixel's own
                if (j == 0u && (sy & 1u))
                    dy = (sy & 2u) ? 0 : 4;
                if (j == NP - 1u && (sy & 2u))
                    dy = (sy & 1u) ? 0 : -4;
            }
            const uint16_t *lrow = lane + dy * static_cast<int>(DN_LW);
            uint32_t w[NW]; // w[i]: columns x - HALO + 2i, x - HALO + 2i + 1
            if (RADIUS == 2) {
                const mcraw_u32x2 a0 = *reinterpret_cast<const mcraw_u32x2 *>(lrow);
                const mcraw_u32x4 a1 = *reinterpret_cast<const mcraw_u32x4 *>(lrow + 4);
                const mcraw_u32x2 a2 = *reinterpret_cast<const mcraw_u32x2 *>(lrow + 12);
                const uint32_t t[8] = {a0[0], a0[1], a1[0], a1[1], a1[2], a1[3], a2[0], a2[1]};
#pragma unroll
                for (uint32_t i = 0; i < NW; i++)
                    w[i] = t[i];
            } else {
                const uint32_t a0 = *reinterpret_cast<const uint32_t *>(lrow);
                const mcraw_u32x4 a1 = *reinterpret_cast<const mcraw_u32x4 *>(lrow + 2);
                const uint32_t a2 = *reinterpret_cast<const uint32_t *>(lrow + 10);
                const uint32_t t[6] = {a0, a1[0], a1[1], a1[2], a1[3], a2};
#pragma unroll
                for (uint32_t i = 0; i < NW; i++)
                    w[i] = t[i];
            }
            uint32_t far[2][4]; // radius 2: the neighbours at -4 and +4 along the row
            if (RADIUS == 2) {
#pragma unroll
                for (uint32_t k = 0; k < 4u; k++)
                    far[0][k] = w[k], far[1][k] = w[k + 4u];
                if (edgex) {
#pragma unroll
                    for (uint32_t k = 0; k < 4u; k++) {
                        const uint32_t both = mlo[k] & mhi[k], own = w[k + 2u];
                        far[0][k] = (w[k] & ~mlo[k]) | (w[k + 4u] & mlo[k] & ~both) | (own & both);
                        far[1][k] = (w[k + 4u] & ~mhi[k]) | (w[k] & mhi[k] & ~both) | (own & both);
                    }
                }
            }
#pragma unroll
            for (uint32_t k = 0; k < 4u; k++) {
#pragma unroll
                for (uint32_t i = 0; i < NP; i++) {
                    const uint32_t a2 = (RADIUS == 2 && i == 0u) ? far[0][k] : (RADIUS == 2 && i == NP - 1u) ? far[1][k] : w[k + i];
                    const uint32_t d2 = pk_absdiff(a2, c[k]);
#pragma unroll
                    for (uint32_t h = 0; h < 2u; h++) {
                        const uint32_t p = 2u * k + h, a = half16(a2, h);
                        const uint32_t t = mul24(half16(d2, h), rv[p]) >> 8, xx = t < 16u ? t : 16u;
                        const uint32_t q = mul24(xx, xx);
                        sq[p] += q;
                        sqa[p] += mul24(q, a);
                        sa[p] += a;
                    }
                }
            }
        }
        uint32_t o[4];
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) {
            uint32_t res[2];
#pragma unroll
            for (uint32_t h = 0; h < 2u; h++) {
                const uint32_t p = 2u * k + h;
                // sum(w) = 256 * NP * NP - sum(q), sum(w * a) = 256 * sum(a) - sum(q * a), the centre (q = 0) among them
                const uint32_t den = 256u * NP * NP - sq[p], num = 256u * sa[p] - sqa[p];
                const int32_t cv = static_cast<int32_t>(half16(c[k], h));
                const int32_t m = static_cast<int32_t>(div_round(num + (den >> 1), den));
                res[h] = static_cast<uint32_t>(cv + (((m - cv) * static_cast<int32_t>(A.amount) + 128) >> 8));
            }
            o[k] = res[0] | (res[1] << 16);
        }
        store8<NT>(fout + static_cast<size_t>(y) * A.opitch, n, A.outvec != 0u, o);
    }
}

template <int RADIUS>
static void denoise_launch(const DnArgs &A, uint32_t tilesY, uint32_t nf, hipStream_t st)
{
    hipLaunchKernelGGL((DN_NT ? kdenoise<RADIUS, true> : kdenoise<RADIUS, false>), dim3(A.tilesX * tilesY, nf), dim3(DN_T), static_cast<size_t>(A.L) * 8u, st, A);
}

#ifdef MCRAW_PATHSM
// The sweep of div_round over the edges of its proven domain: workgroup b takes den = b + 1, its threads the quotients k =
// 0 .. 65536, each with n = k * den + {-1, 0, 1, den / 2, den - 1}; an n below 0 or from 2^30 on, or one whose quotient exceeds
// 65536, is passed over.  The device's own integer division is the reference.
struct DivSweep {
    unsigned long long evals, bad;
    uint32_t n, den, got, pad;
};

constexpr uint32_t DIV_MAXDEN = 6400u, DIV_MAXQ = 65536u;

__global__ void __launch_bounds__(256) kdiv_sweep(DivSweep *R)
{
    const uint32_t den = blockIdx.x + 1u;
    unsigned long long evals = 0ull;
    for (uint32_t k = threadIdx.x; k <= DIV_MAXQ; k += 256u) {
        const long long base = static_cast<long long>(k) * den;
        const long long off[5] = {-1, 0, 1, static_cast<long long>(den / 2u), static_cast<long long>(den) - 1};
#pragma unroll
        for (uint32_t i = 0; i < 5u; i++) {
            const long long nn = base + off[i];
            if (nn < 0 || nn >= (1ll << 30))
                continue;
            const uint32_t n = static_cast<uint32_t>(nn), want = n / den;
            if (want > DIV_MAXQ)
                continue;
            evals++;
            const uint32_t got = div_round(n, den);
            if (got != want && atomicAdd(&R->bad, 1ull) == 0ull)
                R->n = n, R->den = den, R->got = got;
        }
    }
    atomicAdd(&R->evals, evals);
}
#endif

} // namespace mcraw

using namespace mcraw;

#ifdef MCRAW_PATHSM
// The sweep on the current device: out[0 .. 8) = evaluations, mismatches, the first mismatch's n, den and result, and from this
// source's census div_round's calls, steps down and steps up (the census of this source starts over).
extern "C" int mcraw_diag_div_sweep(uint64_t *out)
{
    if (!out)
        return -1;
    mos_paths_read(nullptr, 0, 1);
    DivSweep *R = nullptr, h{};
    if (hipMalloc(&R, sizeof(DivSweep)) != hipSuccess || hipMemset(R, 0, sizeof(DivSweep)) != hipSuccess)
        return -1;
    hipLaunchKernelGGL(kdiv_sweep, dim3(DIV_MAXDEN), dim3(256), 0, nullptr, R);
    const bool ok = hipGetLastError() == hipSuccess && hipDeviceSynchronize() == hipSuccess &&
                    hipMemcpy(&h, R, sizeof(h), hipMemcpyDeviceToHost) == hipSuccess;
    (void)hipFree(R);
    if (!ok)
        return -1;
    uint64_t paths[MP_N] = {};
    mos_paths_read(paths, MP_N, 1);
    out[0] = h.evals, out[1] = h.bad, out[2] = h.n, out[3] = h.den, out[4] = h.got;
    out[5] = paths[MP_DIV_CALLS], out[6] = paths[MP_DIV_DOWN], out[7] = paths[MP_DIV_UP];
    return 0;
}
#endif

extern "C" int mcraw_denoise_batch(mcraw_ctx *c, const mcraw_denoise *d, const uint16_t *in, size_t in_pitch, size_t in_frame_stride,
                                   int width, int height, int n, uint16_t *out, size_t out_pitch, size_t out_frame_stride,
                                   void *stream)
{
    if (!c || !d || n < 0)
        return reject(__func__, "bad arguments");
    if (n == 0)
        return 0;
    if (!in || !out)
        return reject(__func__, "in or out missing");
    const MosaicBatch I(in, in_pitch, in_frame_stride, static_cast<size_t>(n), width, height);
    const MosaicBatch O(out, out_pitch, out_frame_stride, static_cast<size_t>(n), width, height);
    if (const char *why = check(I, O))
        return reject(__func__, why);
    if (d->radius != 1u && d->radius != 2u)
        return reject(__func__, "radius must be 1 or 2");
    if (d->amount < 1u || d->amount > 256u)
        return reject(__func__, "amount must be 1 .. 256");
    if (d->lut_log2 < 6u || d->lut_log2 > 10u)
        return reject(__func__, "lut_log2 must be 6 .. 10");
    if (d->shift > 15u)
        return reject(__func__, "shift must be 0 .. 15");
    if (d->nluts != 1u && d->nluts != static_cast<uint32_t>(n))
        return reject(__func__, "nluts must be 1 or n");
    if (d->reserved[0] != 0u || d->reserved[1] != 0u || d->reserved[2] != 0u)
        return reject(__func__, "reserved must be 0");
    if (!d->lut || (reinterpret_cast<uintptr_t>(d->lut) & 15u))
        return reject(__func__, "lut missing or not 16-byte aligned");
    if (overlap(I, O))
        return reject(__func__, "in and out overlap (every pixel reads its neighbours: there is no in-place form)");

    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = stream_of(c, stream);
    DnArgs A{};
    A.ipitch = in_pitch;
    A.ifstride = in_frame_stride;
    A.opitch = out_pitch;
    A.ofstride = out_frame_stride;
    A.W = static_cast<uint32_t>(width);
    A.H = static_cast<uint32_t>(height);
    A.tilesX = (A.W + DN_TW - 1u) / DN_TW;
    const uint32_t tilesY = (A.H + DN_TH - 1u) / DN_TH;
    A.amount = d->amount;
    A.L = 1u << d->lut_log2;
    A.shift = d->shift;
    A.perframe = d->nluts != 1u ? 1u : 0u;
    A.invec = I.on_grid();
    A.outvec = O.on_grid();
    for (int f0 = 0; f0 < n; f0 += LAUNCH_PIECE) {
        const int nf = std::min<int>(LAUNCH_PIECE, n - f0);
        A.in = in + static_cast<size_t>(f0) * in_frame_stride;
        A.out = out + static_cast<size_t>(f0) * out_frame_stride;
        A.lut = d->lut + (A.perframe ? static_cast<size_t>(f0) * 4u * A.L : 0u);
        if (d->radius == 2u)
            denoise_launch<2>(A, tilesY, static_cast<uint32_t>(nf), st);
        else
            denoise_launch<1>(A, tilesY, static_cast<uint32_t>(nf), st);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}
