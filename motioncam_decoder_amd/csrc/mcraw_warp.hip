// mcraw_warp.hip -- gfx950 kernels for uint16 mosaics resident in HBM -> RGB sampled along one affine map per frame
// (mcraw_demosaic_warp_batch): the Malvar-He-Cutler estimates of krgb_mhc behind a 4 x 4 gather, linear or cubic, into the float,
// display and YUV families.  The contract and its weights: include/mcraw_hip.h; the checks, the phase tables, the position
// arithmetic and the plan, free of HIP: mcraw_warp_args.h; the numpy statement: tests/_warp_ref.py.  The colour stage and the
// stores are the siblings' (mcraw_rgb_dev.h), the host side of the launch theirs too (mcraw_rgb_launch.h); staging, phase A, the
// weights, the taps of a pixel and the store phase are shared with krgb_mesh (mcraw_warp_dev.h).
//
//   krgb_warp  one instance per (output kind, CFA), as the siblings
//
// A workgroup owns a tile of WARP_TW x WARP_TH output pixels.
//   stage   the raw samples under the bounding box of the tile's four corner positions, with the taps (-1 .. +2) and MHC's halo
//           of 2, reflected at the frame's edges, as 16-byte pieces on the frame's 8-column grid (s_raw, krgb_mhc's layout)
//   A       a lane takes 8 source columns on the 8-grid of one source row -- the row's parity is uniform in a wave, the columns'
//           is fixed by the slot, so the CFA role of every slot is known when the kernel is compiled (template S), as in
//           krgb_resample -- and writes the estimates e of the whole window to s_e, once per source pixel
//   gather  a lane takes 4 output columns of an output row -- every lane of the workgroup has its pixels, whatever the kind --:
//           per pixel the 4 x 4 taps over s_e, horizontally first; behind a barrier the tile's E takes the place of the
//           first estimates in s_e
//   store   a lane takes 8 output columns of an output row (the YUV kinds: of a row pair, carrying their 2x2 sums as
//           krgb_bin2y) out of the tile's E and calls the family's row store
// Every sum of taps is exact in two int32 accumulators: v = 256 vh + vl, A = sum w vh, B = sum w vl (the header's bounds),
// 24-bit multiplies (|w| < 2^13, |vh| < 2^15).  The phase table in use sits in LDS; the maps travel in the kernel arguments,
// beside the colours, in pieces of RGB_MAXF frames.
#ifdef MCRAW_PATHSR // (the test builds' switches: the head of mcraw_rgb.hip; the grid's cap comes from that source, below)
#define RGB_GATHER_FAMILY 0u
#include "mcraw_rgb_paths.h"
#endif
#include "mcraw_dev.h"
#include "mcraw_host.h"
#include "mcraw_rgb_args.h"
#include "mcraw_rgb_dev.h"
// The persistent grid's limit is mcraw_rgb.hip's: this unit does not name the cap's switch, and a build of that source with a
// capped grid (build.RGB_PATH_VARIANTS) caps this unit's grid too (tests/test_gpu_warp_paths.py).
namespace mcraw {
uint32_t rgb_grid_limit(uint32_t resident);
}
#define RGB_GRID_LIMIT(resident) ::mcraw::rgb_grid_limit(resident)
#include "mcraw_rgb_launch.h"
#include "mcraw_warp_args.h"
#include "mcraw_warp_dev.h"

namespace mcraw {

struct WarpGeo {
    int32_t m[RGB_MAXF][6]; // the maps of this launch's frames (permap), or one in m[0]
    uint32_t permap;
    uint32_t tilesX;
    uint32_t filter;
};

__device__ const WarpTable g_warp_cubic = warp_table(MCRAW_FILTER_CUBIC);

// One output pixel at position (Y, X): the 4 x 4 taps over the window's estimates (held from row pb, column eb of the frame on),
// horizontally first.  Whatever the position, the reads stay inside the array.
__device__ __forceinline__ void warp_pixel(const int32_t *s_e, const int16_t *s_w, int64_t Y, int64_t X, int32_t pb, int32_t eb,
                                           int32_t (&E)[3])
{
    int32_t wy[4], wx[4];
    warp_weights(s_w, static_cast<uint32_t>(Y) & 255u, wy);
    warp_weights(s_w, static_cast<uint32_t>(X) & 255u, wx);
    const int32_t r0 = min(max(static_cast<int32_t>(Y >> 8) - 1 - pb, 0), static_cast<int32_t>(WARP_EROWS) - 4);
    const int32_t c0 = min(max(static_cast<int32_t>(X >> 8) - 1 - eb, 0), static_cast<int32_t>(WARP_ECOLS) - 4);
    WARP_PATH(RPG_TAP_ROW_LO, static_cast<int32_t>(Y >> 8) - 1 - pb < 0);
    WARP_PATH(RPG_TAP_ROW_HI, static_cast<int32_t>(Y >> 8) - 1 - pb > static_cast<int32_t>(WARP_EROWS) - 4);
    WARP_PATH(RPG_TAP_COL_LO, static_cast<int32_t>(X >> 8) - 1 - eb < 0);
    WARP_PATH(RPG_TAP_COL_HI, static_cast<int32_t>(X >> 8) - 1 - eb > static_cast<int32_t>(WARP_ECOLS) - 4);
    warp_taps(s_e, wy, wx, r0, c0, E);
}

template <int PK, int S>
__global__ void __launch_bounds__(RGB_T) krgb_warp(const RgbArgs A, const WarpGeo G)
{
    constexpr bool LUT = has_lut(PK);
    __shared__ __attribute__((aligned(16))) uint16_t s_raw[WARP_RAWH * WARP_RAWW];
    __shared__ __attribute__((aligned(16))) int32_t s_e[3u * WARP_EROWS * WARP_ESTRIDE];
    __shared__ __attribute__((aligned(16))) int16_t s_w[256u * 4u];
    __shared__ __attribute__((aligned(16))) uint16_t s_lut[LUT ? DISP_LDS_MAX : 8u];
    uint32_t t = blockIdx.x;
    RGB_WALK_DECL;
    if constexpr (LUT)
        stage_lut(A, s_lut);
    for (uint32_t i = threadIdx.x; i < 256u; i += RGB_T) { // the phase table in use: four int16 per phase
        mcraw_u32x2 v;
        if (G.filter == MCRAW_FILTER_LINEAR)
            v = mcraw_u32x2{(16u * (256u - i)) << 16, 16u * i};
        else
            v = *reinterpret_cast<const mcraw_u32x2 *>(g_warp_cubic.w[i]);
        *reinterpret_cast<mcraw_u32x2 *>(&s_w[4u * i]) = v;
    }
    const int W = static_cast<int>(A.W), H = static_cast<int>(A.H);
    do {
        const uint32_t f = LUT ? t / A.units : blockIdx.y, u = LUT ? t % A.units : blockIdx.x;
        RGB_WALK(RF_WARP, f, LUT, A.lutg);
        const uint32_t tx = u % G.tilesX, ty = u / G.tilesX;
        const uint32_t k0 = tx * WARP_TW, k1 = min(k0 + WARP_TW, A.Wo) - 1u; // the tile's first and last column
        const uint32_t i0 = ty * WARP_TH, i1 = min(i0 + WARP_TH, A.Ho) - 1u; // ... and row
        const int32_t *m = G.m[G.permap ? f : 0u];
        const int32_t map[6] = {m[0], m[1], m[2], m[3], m[4], m[5]};
        // the estimates the tile needs: from row pb (even) and column eb (on the 8-grid) of the frame on, np row pairs and ne
        // pieces of 8 columns (tests/cpp/warp_args_check.cpp holds every tap of every tile against this window and the arrays)
        const WarpWin win = warp_window(map, i0, i1, k0, k1);
        const int32_t pb = win.pb, eb = win.eb;
        const uint32_t np = min(win.np, WARP_EROWS / 2u), ne = min(win.ne, WARP_ECOLS / 8u);
        const uint16_t *in = A.in + static_cast<size_t>(f) * A.fstride;
        __syncthreads(); // the LUT and the table are staged; the previous tile's LDS reads are done
#ifdef MCRAW_POISON_RGB
        // the raw window as the siblings'; an estimate of 0x5a5a5b lies above every value of phase A (< 2^22) and inside the taps'
        // bounds (|v >> 8| < 2^15): a stray read changes bytes and overflows nothing
        rgb_poison(s_raw, sizeof(s_raw), 0x5a5a5a5bu);
        rgb_poison(s_e, sizeof(s_e), 0x005a5a5bu);
        __syncthreads();
#endif
        WARP_UNIT(RPG_CUT_ROWS, np < win.np);
        WARP_UNIT(RPG_CUT_COLS, ne < win.ne);
        warp_stage(A, in, s_raw, pb, eb, np, ne, W, H); // raw rows pb - 2 .. pb + 2 np + 1, columns eb - 8 .. eb + 8 ne + 7
        __syncthreads();
        // A: rows of parity 0 in the first half of the workgroup, of parity 1 in the second (uniform in a wave)
        if (threadIdx.x < RGB_T / 2u) {
            for (uint32_t it = threadIdx.x; it < np * ne; it += RGB_T / 2u) {
                WARP_PATH(RPG_A_EVEN, true);
                warp_mhc_row<S, 0>(A, s_raw, s_e, it / ne, it % ne);
            }
        } else {
            for (uint32_t it = threadIdx.x - RGB_T / 2u; it < np * ne; it += RGB_T / 2u) {
                WARP_PATH(RPG_A_ODD, true);
                warp_mhc_row<S, 1>(A, s_raw, s_e, it / ne, it % ne);
            }
        }
        __syncthreads();
        // gather: a lane takes 4 output columns of one output row: every lane of the workgroup has its pixels
        {
            const uint32_t gr = threadIdx.x / (WARP_TW / 4u), gc = 4u * (threadIdx.x % (WARP_TW / 4u));
            const uint32_t j = i0 + gr, x = k0 + gc;
            int32_t E4[3][4] = {};
            WARP_PATH(RPG_PIX, j <= i1 && x <= k1);
            WARP_PATH(RPG_NOPIX, !(j <= i1 && x <= k1));
            if (j <= i1 && x <= k1) {
                const int64_t by = static_cast<int64_t>(map[0]) * j + static_cast<int64_t>(map[1]) * x + 128;
                const int64_t bx = static_cast<int64_t>(map[3]) * j + static_cast<int64_t>(map[4]) * x + 128;
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    int32_t e3[3];
                    warp_pixel(s_e, s_w, map[2] + ((by + static_cast<int64_t>(map[1]) * i) >> 8),
                               map[5] + ((bx + static_cast<int64_t>(map[4]) * i) >> 8), pb, eb, e3);
                    E4[0][i] = e3[0], E4[1][i] = e3[1], E4[2][i] = e3[2];
                }
            }
            __syncthreads(); // every tap is read: the tile's E takes the place of the first estimates
#pragma unroll
            for (uint32_t c = 0; c < 3u; c++)
                *reinterpret_cast<mcraw_u32x4 *>(&s_e[(c * WARP_TH + gr) * WARP_TW + gc]) =
                    mcraw_u32x4{static_cast<uint32_t>(E4[c][0]), static_cast<uint32_t>(E4[c][1]), static_cast<uint32_t>(E4[c][2]),
                                static_cast<uint32_t>(E4[c][3])};
            __syncthreads();
        }
        warp_store<PK>(A, s_e, s_lut, f, i0, i1, k0); // (8 output columns, output row or row pair) out of the tile's E
    } while (LUT && (t += gridDim.x) < A.units * A.nf);
}

struct WarpK {
    template <int PK, int S>
    static auto at() { return &krgb_warp<PK, S>; }
};

static int warp_launch(mcraw_ctx *c, const mcraw_rgb *p, const mcraw_warp *wp, const mcraw_display *d, const mcraw_yuv *yv,
                       const mcraw_rgb_color *colors, int ncolors, const int32_t *maps, const uint16_t *in, size_t in_pitch,
                       size_t in_frame_stride, int width, int height, int n, const WarpPlan &P, void *out, hipStream_t st)
{
    RgbArgs A = rgb_args(p, d, yv, in_pitch, in_frame_stride, width, height, ncolors);
    A.Wo = static_cast<uint32_t>(P.rgb.Wo);
    A.Ho = static_cast<uint32_t>(P.rgb.Ho);
    A.tilesX = P.tilesX;
    A.units = P.units;
    A.invec = P.rgb.invec;
    WarpGeo G{};
    G.permap = P.permap ? 1u : 0u;
    G.tilesX = P.tilesX;
    G.filter = wp->filter;
    const std::vector<RgbCol> cols = rgb_cols(p, colors, ncolors, 0.0625f);
    // pieces of RGB_MAXF frames where the maps or the colours are per frame: both travel in the kernel arguments
    const int piece = (P.permap || A.percol) ? RGB_MAXF : n;
    for (int f0 = 0; f0 < n; f0 += piece) {
        const int nf = std::min(piece, n - f0);
        std::memcpy(G.m, maps + (P.permap ? 6 * static_cast<size_t>(f0) : 0u), sizeof(int32_t) * 6u * static_cast<size_t>(P.permap ? nf : 1));
        const std::vector<RgbCol> pc = A.percol ? std::vector<RgbCol>(cols.begin() + f0, cols.begin() + f0 + nf) : cols;
        if (int rc = rgb_launch(c, rgb_pick<WarpK>(P.rgb), A, P.rgb, pc, in + static_cast<size_t>(f0) * in_frame_stride, nf,
                                static_cast<uint8_t *>(out) + static_cast<size_t>(f0) * P.rgb.out_frame, -1, st, G))
            return rc;
    }
    return 0;
}

} // namespace mcraw

using namespace mcraw;

extern "C" {

int mcraw_demosaic_warp_batch(mcraw_ctx *c, const mcraw_rgb *p, const mcraw_warp *wp, const mcraw_display *d, const mcraw_yuv *y,
                              const mcraw_rgb_color *colors, int ncolors, const int32_t *maps, int nmaps, const uint16_t *in,
                              size_t in_pitch, size_t in_frame_stride, int width, int height, int n, void *out, size_t out_bytes,
                              void *stream)
{
    WarpPlan P;
    const char *why = c ? warp_check(p, wp, d, y, colors, ncolors, maps, nmaps, in, in_pitch, in_frame_stride, width, height, n, out,
                                     out_bytes, P)
                        : "bad arguments";
    if (why)
        return reject("mcraw_demosaic_warp_batch", why);
    if (P.rgb.noop)
        return 0;
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    return warp_launch(c, p, wp, d, y, colors, ncolors, maps, in, in_pitch, in_frame_stride, width, height, n, P, out, stream_of(c, stream));
}

} // extern "C"
