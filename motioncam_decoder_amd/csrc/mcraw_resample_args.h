// mcraw_resample_args.h -- what mcraw_demosaic_resample_batch (include/mcraw_hip.h) decides about a call before anything is
// launched: accept, reject or no-op; on acceptance the plan of the launch (the workgroup's tile, its LDS arrays) and the layout
// of the caller's scratch; and the tap formula itself, as a plain function that the table kernel and the tests share.
// No HIP in here, so that tests/cpp/resample_args_check.cpp can drive it on any machine.  The family's own rules (display / YUV
// struct, dtype, cfa, white, colours, `out`) are rgb_check's pieces (mcraw_rgb_args.h), run in area_check's order: the sequence
// of the checks, the crop's rules and the scratch's layout are that header's window layer, shared with mcraw_area_args.h.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "mcraw_rgb_args.h"

namespace mcraw {

constexpr uint32_t RES_TAPS = 9u;     // taps of an output pixel along one axis, at most (cubic, ratio 2); linear: 5
constexpr uint32_t RES_TW = 64u;      // output columns of a workgroup's tile: 8 lanes of 8 columns side by side
constexpr uint32_t RES_LYMAX = 16u;   // row pairs of a tile, at most
constexpr uint32_t RES_TROWS = 32u;   // LDS: source rows of a tile whose horizontal sums t are kept (3 channels x RES_TSTRIDE dwords each)
constexpr uint32_t RES_TSTRIDE = 68u; // LDS: dwords of a row of t: the tile's 64 columns and 4 of padding (rows start 4 banks apart)
constexpr uint32_t RES_G = 4u;        // LDS: source row pairs whose MHC estimates are held at a time
constexpr uint32_t RES_ECOLS = 144u;  // LDS: source columns of the estimates (18 pieces of 8)
constexpr uint32_t RES_RAWW = RES_ECOLS + 16u; // LDS: raw samples of a row: 8 either side of the estimates (2 used), as krgb_mhc
constexpr size_t RES_SECTION = TAB_SECTION; // the tables of the scratch start on multiples of this

// One output column or row in the scratch: the first sample that carries weight, relative to the crop (negative in front of
// it), how many do, and the weights (4096 in all; those behind `nt` are 0).
struct ResampleTap {
    int32_t j0;
    uint16_t nt;
    int16_t w[RES_TAPS];
};
static_assert(sizeof(ResampleTap) == 24, "the scratch is laid out in entries of 24 bytes");

// n(k, j) of the contract: 2 O times the distance of crop sample j from output pixel k's position.
MCRAW_HD inline int64_t res_n(uint32_t k, int64_t j, uint32_t C, uint32_t O)
{
    return 2 * static_cast<int64_t>(O) * j - ((2 * static_cast<int64_t>(k) + 1) * C - static_cast<int64_t>(O));
}

// The raw kernel value f of the contract at distance |n| / D of the stretched unit.
MCRAW_HD inline int64_t res_f(int64_t n, int64_t D, uint32_t filter)
{
    const int64_t a = (1024 * (n < 0 ? -n : n) + D / 2) / D;
    if (filter == 0u)
        return a < 1024 ? 1024 - a : 0;
    if (a <= 1024)
        return 3 * a * a * a - 5 * 1024 * a * a + 2 * (int64_t{1} << 30);
    if (a < 2048)
        return -a * a * a + 5 * 1024 * a * a - 8 * 1024 * 1024 * a + 4 * (int64_t{1} << 30);
    return 0;
}

// The taps of output pixel k: C crop samples onto O pixels, ceil(C / 2) <= O <= 2 C.  The residual 4096 - sum w goes to the tap
// nearest to the pixel's position (smallest |n|); two taps equally near (the position lies half way between them, every tap has
// a mirror image, the residual is even) take half of it each.
MCRAW_HD inline void resample_taps(uint32_t k, uint32_t C, uint32_t O, uint32_t filter, ResampleTap &t)
{
    constexpr int CAND = 12;
    const int64_t D = 2 * static_cast<int64_t>(C > O ? C : O);
    const int64_t jc = floordiv((2 * static_cast<int64_t>(k) + 1) * C - static_cast<int64_t>(O), 2 * static_cast<int64_t>(O));
    int64_t f[CAND], F = 0;
    int first = -1, last = -1;
    for (int i = 0; i < CAND; i++) { // |j - u| < 2 r <= 4 and jc = floor(u): jc - 3 .. jc + 4 can carry weight
        f[i] = res_f(res_n(k, jc - 5 + i, C, O), D, filter);
        F += f[i];
        if (f[i] != 0) {
            if (first < 0)
                first = i;
            last = i;
        }
    }
    t.j0 = static_cast<int32_t>(jc - 5 + first);
    t.nt = static_cast<uint16_t>(last - first + 1);
    int64_t sum = 0, best = -1;
    int near0 = 0, near1 = -1;
    for (int i = 0; i < static_cast<int>(RES_TAPS); i++) {
        int64_t w = 0;
        if (first + i <= last) {
            w = floordiv(4096 * f[first + i] + F / 2, F);
            const int64_t n = res_n(k, jc - 5 + first + i, C, O), an = n < 0 ? -n : n;
            if (best < 0 || an < best)
                best = an, near0 = i, near1 = -1;
            else if (an == best)
                near1 = i;
        }
        t.w[i] = static_cast<int16_t>(w);
        sum += w;
    }
    const int64_t res = 4096 - sum;
    if (near1 < 0) {
        t.w[near0] = static_cast<int16_t>(t.w[near0] + res);
    } else {
        t.w[near0] = static_cast<int16_t>(t.w[near0] + (res - res / 2));
        t.w[near1] = static_cast<int16_t>(t.w[near1] + res / 2);
    }
}

// No pixel of the axis has more taps than this: the samples inside an open interval of 2 r (linear) or 4 r (cubic),
// r = max(1, C / O); one at equal sizes.
constexpr uint32_t res_tap_bound(uint32_t C, uint32_t O, uint32_t filter)
{
    const uint32_t reach = (filter ? 4u : 2u) * std::max(C, O) / O + 1u;
    return C == O ? 1u : std::min(reach, filter ? RES_TAPS : 5u);
}

// Samples between the first tap of a pixel and the last tap of the pixel m further on, at most (the cpp test sweeps it).
constexpr uint32_t res_span_bound(uint32_t m, uint32_t C, uint32_t O, uint32_t nt)
{
    return static_cast<uint32_t>((static_cast<uint64_t>(m) * C + O - 1u) / O) + 2u + nt;
}

struct ResamplePlan {
    RgbPlan rgb;               // noop, kind, shift, es, Wo, Ho, frame_samples, out_frame, invec (mhc, tilesX, units: unused)
    uint32_t ntx = 0, nty = 0; // res_tap_bound of the axes
    uint32_t ly = 0;           // row pairs of a tile: the most whose source rows fit RES_TROWS
    uint32_t ecols = 0;        // columns of estimates a tile needs, at most (a multiple of 8, <= RES_ECOLS)
    uint32_t erows = 0;        // rows of estimates a tile needs, at most (even, <= RES_TROWS)
    uint32_t tilesX = 0, bands = 0, units = 0; // column tiles; bands of ly row pairs; tilesX * bands
    size_t xtab = 0, ytab = 0, total = 0;      // byte offsets of the two tables in the scratch, and its size

    static constexpr uint32_t rows_of(uint32_t ly, uint32_t C, uint32_t O, uint32_t nt)
    {
        return (res_span_bound(2u * ly - 1u, C, O, nt) + 2u) / 2u * 2u; // from the even row at or in front of the first tap
    }

    // Why `r` alone gives no geometry, or nullptr with everything above filled.
    const char *geometry(const mcraw_resample *r)
    {
        if (r->reserved != 0u)
            return "reserved must be 0";
        if (r->filter != MCRAW_FILTER_LINEAR && r->filter != MCRAW_FILTER_CUBIC)
            return "unknown filter";
        if (const char *why = crop_check(r->x0, r->y0, r->cw, r->ch))
            return why;
        const uint32_t Wo = r->out_w, Ho = r->out_h;
        if (2u * Wo < r->cw || Wo > 2u * r->cw || 2u * Ho < r->ch || Ho > 2u * r->ch)
            return "the output must be 1/2 .. 2 of the crop: ceil(cw / 2) <= out_w <= 2 cw, likewise out_h";
        rgb.Wo = Wo, rgb.Ho = Ho;
        ntx = res_tap_bound(r->cw, Wo, r->filter), nty = res_tap_bound(r->ch, Ho, r->filter);
        ecols = (res_span_bound(RES_TW - 1u, r->cw, Wo, ntx) + 6u) / 8u * 8u + 8u;
        ly = RES_LYMAX;
        while (ly > 1u && (rows_of(ly, r->ch, Ho, nty) > RES_TROWS || ly / 2u >= (Ho + 1u) / 2u))
            ly /= 2u;
        erows = rows_of(ly, r->ch, Ho, nty);
        tilesX = (Wo + RES_TW - 1u) / RES_TW;
        bands = ((Ho + 1u) / 2u + ly - 1u) / ly;
        units = tilesX * bands;
        const TabLayout L = tab_layout(Wo, Ho, sizeof(ResampleTap));
        xtab = L.xtab, ytab = L.ytab, total = L.total;
        return nullptr;
    }
};
static_assert((res_span_bound(RES_TW - 1u, 2u, 1u, RES_TAPS) + 6u) / 8u * 8u + 8u <= RES_ECOLS, "a tile's estimates fit at the ratio limit");
static_assert(ResamplePlan::rows_of(1u, 2u, 1u, RES_TAPS) <= RES_TROWS, "one row pair fits at the ratio limit");

// Why the call is rejected, or nullptr with `plan` filled (plan.rgb.noop: an empty batch, nothing else is set).  d: the display
// family, yv: the YUV family (never both); neither: the float family.  Addresses are only looked at as numbers.
inline const char *resample_check(const mcraw_rgb *p, const mcraw_resample *r, const mcraw_display *d, const mcraw_yuv *yv,
                                  const mcraw_rgb_color *colors, int ncolors, const uint16_t *in, size_t in_pitch,
                                  size_t in_frame_stride, int width, int height, int n, const void *work, size_t work_bytes,
                                  const void *out, size_t out_bytes, ResamplePlan &plan)
{
    constexpr ScaledRules R{MCRAW_RGB_RESAMPLE, 8, "width and height must be even, 8 .. 65536", "p->algo must be MCRAW_RGB_RESAMPLE",
                            "work_bytes below mcraw_resample_work_bytes(r)"};
    const MosaicBatch I(in, in_pitch, in_frame_stride, static_cast<size_t>(n), width, height);
    const char *why = scaled_check(R, p, r, d, yv, colors, ncolors, I, n, work, work_bytes, out, out_bytes, plan);
    if (!why && !plan.rgb.noop)
        plan.rgb.invec = I.on_grid();
    return why;
}

} // namespace mcraw
