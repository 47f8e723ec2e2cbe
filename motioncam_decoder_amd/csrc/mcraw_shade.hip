// mcraw_shade.hip -- gfx950 kernel for uint16 mosaics resident in HBM -> uint16 mosaics with a lens-shading gain map applied
// (mcraw_shade_batch).  The contract (integer arithmetic, bit-exact) is in include/mcraw_hip.h; DESIGN.md 16 has the design.
//
// A workgroup owns a tile of SH_TW columns x SH_TH rows of one frame.  First it writes the VERTICALLY interpolated gains of its
// rows into LDS: for each row, each column parity and each map column i its column span can touch, the pair
// (V[i] | V[min(i + 1, map_w - 1)] << 16) -- one multiply-add pair per value, done once per row and not once per pixel.  Then
// every lane makes 8 consecutive columns of two rows (a 16-byte load and a 16-byte store each): per pixel one ds_read_b32 (both
// horizontal neighbours), two 24-bit multiply-adds for G, the sample's multiply-add and the clamp.
// Every pixel reads only itself, so out == in (in place) is fine.
//
// Test builds (build.MOSAIC_PATH_VARIANTS, tests/test_gpu_mosaic_paths.py; why each is valid: the head of mcraw_mosaic_paths.h):
//   MCRAW_PATHSM  the path census; mcraw_diag_mosaic_paths below adds up the sources that include mcraw_mosaic_paths.h
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

constexpr int SH_T = 256;        // threads per workgroup
constexpr uint32_t SH_LX = 32u;  // lanes across a tile: 8 columns each
constexpr uint32_t SH_TW = 8u * SH_LX;
constexpr uint32_t SH_PASS = SH_T / SH_LX; // rows per pass (8)
constexpr uint32_t SH_NPASS = 2u;          // rows per lane: its loads are in flight together
constexpr uint32_t SH_TH = SH_PASS * SH_NPASS;
constexpr uint32_t SH_MAXM = 64u; // map_w, map_h <= 64

// Which stores the output rows use, out of place and in place (where the line was just read): `sc1 nt` streaming stores
// (store_stream16), as the decode kernels use for rows that are written once, or plain ones.
// -DMCRAW_SHADE_FLIP_STORES builds the other pair; tools/bench_shade.py --alt-lib runs the two builds side by side.
#ifdef MCRAW_SHADE_FLIP_STORES
constexpr bool SH_NT_OUT = false, SH_NT_INPLACE = false;
#else
constexpr bool SH_NT_OUT = true, SH_NT_INPLACE = true;
#endif

struct ShadeArgs {
    const uint16_t *in;
    uint16_t *out;
    const uint16_t *map; // (nmaps, 4, mh, mw)
    size_t ipitch, ifstride, opitch, ofstride;
    uint32_t W, H, mw, mh;
    uint32_t sx, sy;  // floor((map - 1) * 2^24 / (size - 1)), 0 for size 1
    uint32_t tilesX, tilesY;
    int top;
    int black[4];
    uint32_t permap; // one map per frame
    uint32_t f0;     // index of the launch's first frame in the batch (its map)
    uint32_t invec, outvec; // every 8-column piece of `in` / `out` lies on the 16-byte grid
};

template <bool NT>
__global__ void __launch_bounds__(SH_T) kshade(const ShadeArgs A)
{
    // s_v[row of the tile][column parity][map column - ilo]: V[i] | V[i1] << 16
    __shared__ uint32_t s_v[SH_TH][2][SH_MAXM];
    const uint32_t tile = blockIdx.x, f = blockIdx.y;
    const uint32_t ty = tile / A.tilesX, tx = tile - ty * A.tilesX;
    const uint32_t x0 = tx * SH_TW, y0 = ty * SH_TH;
    const uint32_t xlast = min(x0 + SH_TW, A.W) - 1u;
    // the lane's samples first: their loads are in flight while the gains below are made
    const uint32_t lx = threadIdx.x % SH_LX, ly = threadIdx.x / SH_LX;
    const uint32_t x = x0 + 8u * lx;
    const bool inside = x < A.W;
    const uint32_t n = inside ? min(8u, A.W - x) : 0u;
    const uint16_t *fin = A.in + static_cast<size_t>(f) * A.ifstride + x;
    uint16_t *fout = A.out + static_cast<size_t>(f) * A.ofstride + x;
    uint32_t p[SH_NPASS][4];
    MOS_PATH(MP_WG, threadIdx.x == 0u);
    MOS_PATH(MP_IDLE_LANE, !inside);
#pragma unroll
    for (uint32_t a = 0; a < SH_NPASS; a++) {
        const uint32_t y = y0 + ly + a * SH_PASS;
        MOS_PATH(MP_ROW_CONT, inside && y >= A.H);
        if (inside && y < A.H)
            load8(fin + static_cast<size_t>(y) * A.ipitch, n, A.invec != 0u, p[a]);
    }
    // (x <= W - 1 gives x * sx <= (mw - 1) << 24: every map column below is inside the map)
    const uint32_t ilo = (x0 * A.sx) >> 24, cnt = ((xlast * A.sx) >> 24) - ilo + 1u;
    const uint16_t *map = A.map + static_cast<size_t>(A.permap ? A.f0 + f : 0u) * 4u * A.mh * A.mw;
    for (uint32_t e = threadIdx.x; e < SH_TH * 2u * cnt; e += SH_T) {
        const uint32_t k = e % cnt, rp = e / cnt, px = rp & 1u, r = rp >> 1, y = y0 + r;
        if (y >= A.H)
            continue;
        const uint32_t uy = y * A.sy, j0 = uy >> 24, fy = (uy >> 12) & 4095u, j1 = min(j0 + 1u, A.mh - 1u);
        const uint32_t i0 = ilo + k, i1 = min(i0 + 1u, A.mw - 1u);
        const uint16_t *pl = map + static_cast<size_t>((y & 1u) * 2u + px) * A.mh * A.mw;
        const uint16_t *r0 = pl + j0 * A.mw, *r1 = pl + j1 * A.mw;
        const uint32_t g00 = r0[i0] & 0x7FFFu, g10 = r1[i0] & 0x7FFFu, g01 = r0[i1] & 0x7FFFu, g11 = r1[i1] & 0x7FFFu;
        const uint32_t v0 = (g00 * (4096u - fy) + g10 * fy + 2048u) >> 12;
        const uint32_t v1 = (g01 * (4096u - fy) + g11 * fy + 2048u) >> 12;
        s_v[r][px][k] = v0 | (v1 << 16);
    }
    __syncthreads();
    if (!inside)
        return;
    // the horizontal place of the lane's 8 columns: columns behind the row's end take the last column's (their results are
    // never stored), so no index leaves the row's entries
    // (ux by one multiply per lane and an add per column; it stays at or below (mw - 1) << 24 < 2^30)
    uint32_t idx[8], fx[8], ux = x * A.sx;
#pragma unroll
    for (uint32_t i = 0; i < 8u; i++) {
        idx[i] = (ux >> 24) - ilo;
        fx[i] = (ux >> 12) & 4095u;
        ux += x + i < xlast ? A.sx : 0u;
    }
#pragma unroll
    for (uint32_t a = 0; a < SH_NPASS; a++) {
        const uint32_t r = ly + a * SH_PASS, y = y0 + r;
        if (y >= A.H)
            continue;
        const int b0 = (y & 1u) ? A.black[2] : A.black[0], b1 = (y & 1u) ? A.black[3] : A.black[1];
        uint32_t o[4];
#pragma unroll
        for (uint32_t i = 0; i < 8u; i++) {
            const uint32_t v = s_v[r][i & 1u][idx[i]];
            // (every factor is below 2^24: the products are exact as 24-bit multiplies)
            const uint32_t G = (__umul24(v & 0xFFFFu, 4096u - fx[i]) + __umul24(v >> 16, fx[i]) + 2048u) >> 12;
            const int b = (i & 1u) ? b1 : b0;
            const int d = static_cast<int>((p[a][i >> 1] >> (16u * (i & 1u))) & 0xFFFFu) - b;
            const int c = b + ((__mul24(d, static_cast<int>(G)) + 2048) >> 12);
            const uint32_t q = static_cast<uint32_t>(min(max(c, 0), A.top));
            o[i >> 1] = (i & 1u) ? (o[i >> 1] | (q << 16)) : q;
        }
        store8<NT>(fout + static_cast<size_t>(y) * A.opitch, n, A.outvec != 0u, o);
    }
}

} // namespace mcraw

using namespace mcraw;

#ifdef MCRAW_PATHSM
// The census of the mosaic stages, in the order of MosPath, summed over the sources that have one (up to n counters; returns how
// many there are); `reset`: and start it over.
extern "C" int mcraw_diag_mosaic_paths(uint64_t *out, int n, int reset) { return census_sum<MosPath, MP_N>(out, n, reset); }
#endif

extern "C" int mcraw_shade_batch(mcraw_ctx *c, const mcraw_shade *s, const uint16_t *in, size_t in_pitch, size_t in_frame_stride,
                                 int width, int height, int n, uint16_t *out, size_t out_pitch, size_t out_frame_stride,
                                 void *stream)
{
    if (!c || !s || n < 0)
        return reject(__func__, "bad arguments");
    if (n == 0)
        return 0;
    if (!in || !out || !s->map)
        return reject(__func__, "in, out or map missing");
    const MosaicBatch I(in, in_pitch, in_frame_stride, static_cast<size_t>(n), width, height);
    const MosaicBatch O(out, out_pitch, out_frame_stride, static_cast<size_t>(n), width, height);
    if (const char *why = check(I, O))
        return reject(__func__, why);
    if (reinterpret_cast<uintptr_t>(s->map) & 15u)
        return reject(__func__, "map not 16-byte aligned");
    if (s->map_w < 1u || s->map_w > SH_MAXM || s->map_h < 1u || s->map_h > SH_MAXM)
        return reject(__func__, "map_w and map_h must be 1 .. 64");
    if (s->nmaps != 1u && s->nmaps != static_cast<uint32_t>(n))
        return reject(__func__, "nmaps must be 1 or n");
    if (s->top < 1u || s->top > 65535u)
        return reject(__func__, "top must be 1 .. 65535");
    if (s->reserved[0] != 0u || s->reserved[1] != 0u)
        return reject(__func__, "reserved must be 0");
    const bool inplace = in == out && in_pitch == out_pitch && (n == 1 || in_frame_stride == out_frame_stride);
    if (!inplace && overlap(I, O))
        return reject(__func__, "in and out overlap (in place needs out == in with the same pitch and frame stride)");

    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = stream_of(c, stream);
    ShadeArgs A{};
    A.map = s->map;
    A.ipitch = in_pitch;
    A.ifstride = in_frame_stride;
    A.opitch = out_pitch;
    A.ofstride = out_frame_stride;
    A.W = static_cast<uint32_t>(width);
    A.H = static_cast<uint32_t>(height);
    A.mw = s->map_w;
    A.mh = s->map_h;
    A.sx = width > 1 ? static_cast<uint32_t>((static_cast<uint64_t>(s->map_w - 1u) << 24) / (A.W - 1u)) : 0u;
    A.sy = height > 1 ? static_cast<uint32_t>((static_cast<uint64_t>(s->map_h - 1u) << 24) / (A.H - 1u)) : 0u;
    A.tilesX = (A.W + SH_TW - 1u) / SH_TW;
    A.tilesY = (A.H + SH_TH - 1u) / SH_TH;
    A.top = static_cast<int>(s->top);
    for (int i = 0; i < 4; i++)
        A.black[i] = s->black[i];
    A.permap = s->nmaps > 1u ? 1u : 0u;
    A.invec = I.on_grid();
    A.outvec = O.on_grid();
    const bool nt = inplace ? SH_NT_INPLACE : SH_NT_OUT;
    for (int f0 = 0; f0 < n; f0 += LAUNCH_PIECE) {
        const int nf = std::min<int>(LAUNCH_PIECE, n - f0);
        A.in = in + static_cast<size_t>(f0) * in_frame_stride;
        A.out = out + static_cast<size_t>(f0) * out_frame_stride;
        A.f0 = static_cast<uint32_t>(f0);
        const dim3 grid(A.tilesX * A.tilesY, static_cast<uint32_t>(nf));
        hipLaunchKernelGGL(nt ? kshade<true> : kshade<false>, grid, dim3(SH_T), 0, st, A);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}
