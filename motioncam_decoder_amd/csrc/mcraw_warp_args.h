// mcraw_warp_args.h -- what mcraw_demosaic_warp_batch (include/mcraw_hip.h) decides about a call before anything is launched:
// accept, reject or no-op; the phase tables of its two filters, as compile-time constants; the position arithmetic of a map; and
// the plan of the launch: the workgroup's tile and the worst-case source window of a tile under the bounds on a map's linear
// part, from which the kernel's LDS arrays are sized.  No HIP in here, so that tests/cpp/warp_args_check.cpp can drive it on any
// machine.  The family's own rules (display / YUV struct, dtype, cfa, white, colours, `out`) are rgb_check's pieces
// (mcraw_rgb_args.h), run in scaled_check's order.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "mcraw_rgb_args.h"

namespace mcraw {

constexpr uint32_t WARP_TW = 32u;      // output columns of a workgroup's tile: 8 lanes of 4 columns gather, 4 lanes of 8 store
constexpr uint32_t WARP_TH = 32u;      // output rows of a tile
constexpr int32_t WARP_ONE = 65536;    // the linear part's unit
constexpr int32_t WARP_DEV = 16384;    // |ayy - 1|, |axx - 1|, |ayx|, |axy| at most (in 1/65536)
// A tile's positions span at most this many whole samples along either axis, first to last: the diagonal term over the tile's own
// axis, the off-diagonal term over the other, one for the two floors ((.. + 128) >> 8 and >> 8).
constexpr uint32_t warp_span(uint32_t own, uint32_t other)
{
    return static_cast<uint32_t>((static_cast<uint64_t>(WARP_ONE + WARP_DEV) * (own - 1u) + static_cast<uint64_t>(WARP_DEV) * (other - 1u)) >> 16) + 1u;
}
// LDS: rows of estimates of a tile (taps -1 .. +2 round the span, one row in front to start on an even row; even) and columns
// (likewise, up to 7 in front to start on the 8-grid; a multiple of 8)
constexpr uint32_t WARP_EROWS = (warp_span(WARP_TH, WARP_TW) + 1u + 3u + 1u + 1u) / 2u * 2u;
constexpr uint32_t WARP_ECOLS = (warp_span(WARP_TW, WARP_TH) + 1u + 3u + 7u + 7u) / 8u * 8u;
constexpr uint32_t WARP_ESTRIDE = WARP_ECOLS + 4u; // LDS: dwords of a row of estimates: rows start 4 banks apart
constexpr uint32_t WARP_RAWW = WARP_ECOLS + 16u;   // LDS: raw samples of a row: 8 either side of the estimates (2 used), as krgb_mhc
constexpr uint32_t WARP_RAWH = WARP_EROWS + 4u;    // 2 halo rows above and below
static_assert(WARP_EROWS == 52u && WARP_ECOLS == 64u, "the window of a 32 x 32 tile at the linear bounds");
static_assert(3u * WARP_TH * WARP_TW <= WARP_EROWS * WARP_ESTRIDE && WARP_TW % 8u == 0u,
              "the tile's E (3 channels, 16-byte pieces) takes the place of the first channel's estimates");
static_assert(3u * WARP_EROWS * WARP_ESTRIDE * 4u + WARP_RAWH * WARP_RAWW * 2u + 256u * 8u + 8192u <= 65536u,
              "estimates, raw window, phase table and an LDS-sized LUT fit a workgroup's 64 KiB");

// One table of 256 phases x 4 taps (at j = -1 .. 2 about the position's whole part), 4096 in all per phase.
struct WarpTable {
    int16_t w[256][4];
};

constexpr int64_t warp_floordiv(int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

// Catmull-Rom times 2 * 1024^3 at distance a / 1024 (mcraw_resample_args.h's res_f, cubic)
constexpr int64_t warp_cubic_f(int64_t a)
{
    if (a <= 1024)
        return 3 * a * a * a - 5 * 1024 * a * a + 2 * (int64_t{1} << 30);
    if (a < 2048)
        return -a * a * a + 5 * 1024 * a * a - 8 * 1024 * 1024 * a + 4 * (int64_t{1} << 30);
    return 0;
}

constexpr WarpTable warp_table(uint32_t filter)
{
    WarpTable T{};
    for (int p = 0; p < 256; p++) {
        if (filter == MCRAW_FILTER_LINEAR) {
            T.w[p][0] = 0, T.w[p][1] = static_cast<int16_t>(16 * (256 - p)), T.w[p][2] = static_cast<int16_t>(16 * p), T.w[p][3] = 0;
            continue;
        }
        int64_t f[4] = {}, F = 0, d[4] = {}, w[4] = {}, sum = 0;
        for (int j = 0; j < 4; j++) {
            const int64_t n = 256 * (j - 1) - p;
            d[j] = n < 0 ? -n : n;
            f[j] = warp_cubic_f(4 * d[j]);
            F += f[j];
        }
        for (int j = 0; j < 4; j++) {
            w[j] = warp_floordiv(4096 * f[j] + F / 2, F);
            sum += w[j];
        }
        // the residual: to the tap of smallest distance (j = 0: index 1; j = 1: index 2); half each where they are equally near
        const int64_t res = 4096 - sum;
        if (d[1] < d[2])
            w[1] += res;
        else if (d[2] < d[1])
            w[2] += res;
        else
            w[1] += res - res / 2, w[2] += res / 2;
        for (int j = 0; j < 4; j++)
            T.w[p][j] = static_cast<int16_t>(w[j]);
    }
    return T;
}

// The source position of output pixel (i, k) under map m = {ayy, ayx, ty, axy, axx, tx}, in 1/256 sample.
MCRAW_HD inline void warp_pos(const int32_t *m, uint32_t i, uint32_t k, int64_t &Y, int64_t &X)
{
    Y = m[2] + ((static_cast<int64_t>(m[0]) * i + static_cast<int64_t>(m[1]) * k + 128) >> 8);
    X = m[5] + ((static_cast<int64_t>(m[3]) * i + static_cast<int64_t>(m[4]) * k + 128) >> 8);
}

// The estimates that output rows i0 .. i1, columns k0 .. k1 read: from row pb (even) and column eb (on the 8-grid) of the frame
// on, np row pairs and ne pieces of 8 columns.  Y and X are monotone in i and in k, so the four corners bound every pixel.
struct WarpWin {
    int32_t pb, eb;
    uint32_t np, ne;
};
MCRAW_HD inline WarpWin warp_window(const int32_t *m, uint32_t i0, uint32_t i1, uint32_t k0, uint32_t k1)
{
    int64_t y[4], x[4];
    warp_pos(m, i0, k0, y[0], x[0]);
    warp_pos(m, i0, k1, y[1], x[1]);
    warp_pos(m, i1, k0, y[2], x[2]);
    warp_pos(m, i1, k1, y[3], x[3]);
    int64_t ylo = y[0], yhi = y[0], xlo = x[0], xhi = x[0];
    for (int c = 1; c < 4; c++) {
        ylo = y[c] < ylo ? y[c] : ylo, yhi = y[c] > yhi ? y[c] : yhi;
        xlo = x[c] < xlo ? x[c] : xlo, xhi = x[c] > xhi ? x[c] : xhi;
    }
    WarpWin w;
    w.pb = static_cast<int32_t>(((ylo >> 8) - 1) & ~int64_t{1});
    w.eb = static_cast<int32_t>(((xlo >> 8) - 1) & ~int64_t{7});
    w.np = static_cast<uint32_t>((((yhi >> 8) + 2 - w.pb) >> 1) + 1);
    w.ne = static_cast<uint32_t>((((xhi >> 8) + 2 - w.eb) >> 3) + 1);
    return w;
}

struct WarpPlan {
    RgbPlan rgb;               // noop, kind, shift, es, Wo, Ho, frame_samples, out_frame, invec (mhc, tilesX, units: unused)
    uint32_t tilesX = 0, tilesY = 0, units = 0;
    bool permap = false;       // a map per frame

    // Why `w` alone gives no geometry, or nullptr with the tiles filled.
    const char *geometry(const mcraw_warp *w)
    {
        if (w->reserved != 0u)
            return "reserved must be 0";
        if (w->filter != MCRAW_FILTER_LINEAR && w->filter != MCRAW_FILTER_CUBIC)
            return "unknown filter";
        if (w->out_w < 1u || w->out_h < 1u || w->out_w > 65536u || w->out_h > 65536u)
            return "out_w and out_h must be 1 .. 65536";
        rgb.Wo = w->out_w, rgb.Ho = w->out_h;
        tilesX = (w->out_w + WARP_TW - 1u) / WARP_TW;
        tilesY = (w->out_h + WARP_TH - 1u) / WARP_TH;
        units = tilesX * tilesY;
        return nullptr;
    }
};

// Why one map is none for a width x height frame onto Wo x Ho pixels, or nullptr.
inline const char *warp_map_check(const int32_t *m, int width, int height, uint32_t Wo, uint32_t Ho)
{
    const auto off = [](int32_t v, int32_t c) { return static_cast<int64_t>(v) - c > WARP_DEV || static_cast<int64_t>(v) - c < -WARP_DEV; };
    if (off(m[0], WARP_ONE) || off(m[4], WARP_ONE) || off(m[1], 0) || off(m[3], 0))
        return "the linear part is outside the stabilisation regime: |ayy - 65536|, |axx - 65536|, |ayx|, |axy| <= 16384";
    const uint32_t ci[4] = {0u, 0u, Ho - 1u, Ho - 1u}, ck[4] = {0u, Wo - 1u, 0u, Wo - 1u};
    for (int c = 0; c < 4; c++) {
        int64_t Y, X;
        warp_pos(m, ci[c], ck[c], Y, X);
        if (Y < 0 || Y > 256 * (static_cast<int64_t>(height) - 1) || X < 0 || X > 256 * (static_cast<int64_t>(width) - 1))
            return "a corner of the output leaves the frame: 0 <= Y <= 256 (height - 1) and 0 <= X <= 256 (width - 1)";
    }
    return nullptr;
}

// Why the call is rejected, or nullptr with `plan` filled (plan.rgb.noop: an empty batch, nothing else is set).  d: the display
// family, yv: the YUV family (never both); neither: the float family.  Addresses are only looked at as numbers; the maps are
// read (host memory).  A message about a map names its frame; it lives in a buffer of the calling thread.
inline const char *warp_check(const mcraw_rgb *p, const mcraw_warp *w, const mcraw_display *d, const mcraw_yuv *yv,
                              const mcraw_rgb_color *colors, int ncolors, const int32_t *maps, int nmaps, const uint16_t *in,
                              size_t in_pitch, size_t in_frame_stride, int width, int height, int n, const void *out, size_t out_bytes,
                              WarpPlan &plan)
{
    plan = WarpPlan{};
    if (!p || !w || !maps || n < 0)
        return "bad arguments";
    if (d && yv)
        return "a display stage and a YUV stage at once";
    if (n == 0) {
        plan.rgb.noop = true;
        return nullptr;
    }
    if (width < 8 || height < 8 || (width & 1) || (height & 1) || width > 65536 || height > 65536)
        return "width and height must be even, 8 .. 65536";
    const MosaicBatch I(in, in_pitch, in_frame_stride, static_cast<size_t>(n), width, height);
    if (const char *why = I.check())
        return why;
    if (p->algo != MCRAW_RGB_WARP)
        return "p->algo must be MCRAW_RGB_WARP";
    if (const char *why = rgb_check_stage(p, d, yv, colors, ncolors, n, plan.rgb))
        return why;
    if (const char *why = plan.geometry(w))
        return why;
    if (yv && ((plan.rgb.Ho | plan.rgb.Wo) & 1u))
        return "4:2:0 needs an even out_h and out_w";
    if (nmaps != 1 && nmaps != n)
        return "nmaps must be 1 or n";
    for (int f = 0; f < nmaps; f++)
        if (const char *why = warp_map_check(maps + 6 * static_cast<size_t>(f), width, height, w->out_w, w->out_h)) {
            static thread_local char msg[256];
            std::snprintf(msg, sizeof(msg), "the map of frame %d: %s", f, why);
            return msg;
        }
    if (const char *why = rgb_check_out(p, yv != nullptr, n, out, out_bytes, plan.rgb))
        return why;
    plan.permap = nmaps > 1;
    plan.rgb.invec = I.on_grid();
    return nullptr;
}

} // namespace mcraw
