// mcraw_rgb_args.h -- what the three demosaic entry points (mcraw_demosaic_batch, _display_batch, _yuv_batch) decide about a
// call before anything is launched: accept, reject or no-op, and on acceptance the plan of the launch (output sizes, launch
// geometry, CFA role shift, kernel kind).  No HIP in here, so that tests/cpp/rgb_args_check.cpp can drive it on any machine.
// The input batch is a MosaicBatch (mcraw_mosaic_args.h): its base, alignment, pitch and frame-stride checks and its 16-byte
// grid are that header's.  At the end, the window layer: what the checks of the two scaled entry points (mcraw_area_args.h,
// mcraw_resample_args.h) share.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdlib>

#include "../../include/mcraw_hip.h"
#include "mcraw_mosaic_args.h"

namespace mcraw {

constexpr uint32_t RGB_T = 256;  // threads per workgroup
constexpr uint32_t MHC_TW = 256; // tile columns: 32 lanes x 8
constexpr uint32_t MHC_TH = 32;  // tile rows: 8 row pairs x 2 passes

// Output kinds.  The float kinds are mcraw_plan.h's PK_F32 / PK_F16 / PK_BF16 (mcraw_rgb.hip asserts that they agree).
constexpr int rgb_float_kind(uint32_t dtype) { return 31 + static_cast<int>(dtype); } // MCRAW_FLOAT_* -> PK_F32 / PK_F16 / PK_BF16
constexpr int PK_DISP8 = 48, PK_DISP16 = 49; // display: uint8 / uint16 through a transfer-curve LUT
// Y'CbCr 4:2:0: a Y plane, then interleaved (Cb, Cr) rows; uint8, or uint16 holding a 10-bit code << 6
constexpr int PK_NV12 = 50, PK_P010 = 51;
constexpr bool is_disp(int pk) { return pk == PK_DISP8 || pk == PK_DISP16; }
constexpr bool is_yuv(int pk) { return pk == PK_NV12 || pk == PK_P010; }
constexpr bool has_lut(int pk) { return is_disp(pk) || is_yuv(pk); } // persistent grid, LUT staged per workgroup
constexpr uint32_t out_es(int pk) { return pk == rgb_float_kind(MCRAW_FLOAT_F32) ? 4u : (pk == PK_DISP8 || pk == PK_NV12) ? 1u : 2u; }

// The launch of an accepted call.
struct RgbPlan {
    bool noop;            // an empty batch: nothing below is set, nothing is launched
    int kind;             // PK_*
    int shift;            // RGGB role of CFA position p: p ^ shift
    bool mhc;             // MCRAW_RGB_MHC, else BIN2 (or HA: `ha`)
    bool invec;           // every 8-column piece of every input row lies on the 16-byte grid
    size_t es, Wo, Ho;    // bytes per output sample; output size
    size_t frame_samples; // samples per frame: 3 planes, or a Y plane and half of one for the (Cb, Cr) rows
    size_t out_frame;     // bytes per output frame
    uint32_t tilesX;      // MHC: tiles per row band; BIN2: groups of 8 output columns per output row
    uint32_t units;       // per frame: tiles (MHC), or workgroups of 256 items (BIN2; YUV kinds: an item is a row pair)
    bool ha;              // MCRAW_RGB_HA (csrc/mcraw_ha.hip): MHC's output size and tiles, estimates in 1/32
};

inline bool finite_all(const float *v, int n)
{
    for (int i = 0; i < n; i++)
        if (!std::isfinite(v[i]))
            return false;
    return true;
}

// The pieces of rgb_check that mcraw_demosaic_area_batch's check (mcraw_area_args.h) runs as well, in rgb_check's order.
// rgb_check_stage: the display / YUV struct, dtype, cfa, flags, white and the colours; sets plan.kind.
inline const char *rgb_check_stage(const mcraw_rgb *p, const mcraw_display *d, const mcraw_yuv *yv, const mcraw_rgb_color *colors,
                                   int ncolors, int n, RgbPlan &plan)
{
    const uint16_t *lut = d ? d->lut : yv ? yv->lut : nullptr;
    const uint32_t lut_log2 = d ? d->lut_log2 : yv ? yv->lut_log2 : 0u;
    if (d || yv) {
        if (p->dtype != 0u || p->flags != 0u)
            return "p->dtype and p->flags must be 0 (the display / YUV stage decides the output)";
        if (lut_log2 < 8u || lut_log2 > 16u)
            return "lut_log2 must be 8 .. 16";
        if (!lut || (reinterpret_cast<uintptr_t>(lut) & 15u))
            return "lut missing or not 16-byte aligned";
    }
    if (d) {
        if (d->dtype != MCRAW_DISP_U8 && d->dtype != MCRAW_DISP_U16)
            return "unknown display dtype";
        if (d->layout != MCRAW_DISP_CHW && d->layout != MCRAW_DISP_HWC)
            return "unknown display layout";
        if (d->reserved != 0u)
            return "reserved must be 0";
        plan.kind = d->dtype == MCRAW_DISP_U8 ? PK_DISP8 : PK_DISP16;
    } else if (yv) {
        if (yv->format != MCRAW_YUV_NV12 && yv->format != MCRAW_YUV_P010)
            return "unknown YUV format";
        if (yv->reserved != 0u)
            return "reserved must be 0";
        if (yv->in_bits < 8u || yv->in_bits > 16u)
            return "in_bits must be 8 .. 16";
        if (yv->sh < 1u || yv->sh > 24u)
            return "sh must be 1 .. 24";
        const int32_t top = yv->format == MCRAW_YUV_NV12 ? 255 : 1023;
        if (yv->y_off < 0 || yv->y_off > top || yv->c_off < 0 || yv->c_off > top)
            return "y_off and c_off must be 0 .. 2^bits - 1";
        // no int32 sum can wrap: 4 * (2^in_bits - 1) * (|c0| + |c1| + |c2|) + 2^(sh + 1) < 2^31 for every row
        const int32_t *rows[3] = {yv->cy, yv->cb, yv->cr};
        for (const int32_t *r : rows) {
            const int64_t mag = std::llabs(static_cast<int64_t>(r[0])) + std::llabs(static_cast<int64_t>(r[1])) +
                                std::llabs(static_cast<int64_t>(r[2]));
            if (4 * ((int64_t{1} << yv->in_bits) - 1) * mag + (int64_t{1} << (yv->sh + 1u)) >= (int64_t{1} << 31))
                return "coefficients could overflow int32: 4 * (2^in_bits - 1) * (|c0| + |c1| + |c2|) + 2^(sh + 1) >= 2^31";
        }
        plan.kind = yv->format == MCRAW_YUV_NV12 ? PK_NV12 : PK_P010;
    } else {
        if (p->dtype != MCRAW_FLOAT_F32 && p->dtype != MCRAW_FLOAT_F16 && p->dtype != MCRAW_FLOAT_BF16)
            return "unknown dtype";
        plan.kind = rgb_float_kind(p->dtype);
    }
    if (p->cfa > MCRAW_CFA_GBRG)
        return "unknown cfa";
    if (p->flags & ~MCRAW_FLOAT_CLIP)
        return "unknown flag";
    const float bsum = static_cast<float>(static_cast<int>(p->black[0]) + p->black[1] + p->black[2] + p->black[3]);
    if (!std::isfinite(p->white) || !(p->white > 0.25f * bsum))
        return "white must be finite and above the mean black level";
    if (!colors || (ncolors != 1 && ncolors != n))
        return "ncolors must be 1 or n";
    for (int i = 0; i < ncolors; i++)
        if (!finite_all(colors[i].gain, 3) || !finite_all(colors[i].m, 9))
            return "non-finite gain or matrix entry";
    return nullptr;
}

// rgb_check_out: `out` against plan.kind, plan.Ho and plan.Wo; sets es, frame_samples, out_frame and the CFA's shift.
inline const char *rgb_check_out(const mcraw_rgb *p, bool yuv, int n, const void *out, size_t out_bytes, RgbPlan &plan)
{
    plan.es = out_es(plan.kind);
    plan.frame_samples = yuv ? plan.Ho * plan.Wo / 2u * 3u : 3u * plan.Ho * plan.Wo;
    if (out_bytes / plan.es / plan.frame_samples < static_cast<size_t>(n))
        return yuv ? "out_bytes below n * Ho * Wo * 3 / 2 * sample size" : "out_bytes below n * 3 * Ho * Wo * element size";
    if (!out || (reinterpret_cast<uintptr_t>(out) & (plan.es - 1u)))
        return "in / out missing or not aligned to their element size";
    plan.out_frame = plan.frame_samples * plan.es;
    constexpr int shift_of[4] = {0, 3, 1, 2}; // MCRAW_CFA_* -> role shift: RGGB 0, BGGR 3, GRBG 1, GBRG 2
    plan.shift = shift_of[p->cfa];
    return nullptr;
}

// Why the call is rejected, or nullptr with `plan` filled.  d: the display stage, yv: the YUV stage (never both); neither:
// the float entry.  Addresses are only looked at as numbers.
inline const char *rgb_check(const mcraw_rgb *p, const mcraw_display *d, const mcraw_yuv *yv, const mcraw_rgb_color *colors,
                             int ncolors, const uint16_t *in, size_t in_pitch, size_t in_frame_stride, int width, int height, int n,
                             const void *out, size_t out_bytes, RgbPlan &plan)
{
    plan = RgbPlan{};
    if (!p || n < 0)
        return "bad arguments";
    if (n == 0) {
        plan.noop = true;
        return nullptr;
    }
    if (width < 4 || height < 4 || (width & 1) || (height & 1) || width > 65536 || height > 65536)
        return "width and height must be even, 4 .. 65536";
    const MosaicBatch I(in, in_pitch, in_frame_stride, static_cast<size_t>(n), width, height);
    if (const char *why = I.check())
        return why;
    if (p->algo != MCRAW_RGB_MHC && p->algo != MCRAW_RGB_BIN2 && p->algo != MCRAW_RGB_HA)
        return "unknown algo";
    if (const char *why = rgb_check_stage(p, d, yv, colors, ncolors, n, plan))
        return why;
    plan.mhc = p->algo == MCRAW_RGB_MHC;
    plan.ha = p->algo == MCRAW_RGB_HA;
    const bool full = plan.mhc || plan.ha; // full resolution, in tiles of MHC_TW x MHC_TH
    plan.Wo = full ? static_cast<size_t>(width) : static_cast<size_t>(width) / 2u;
    plan.Ho = full ? static_cast<size_t>(height) : static_cast<size_t>(height) / 2u;
    if (yv && ((plan.Ho | plan.Wo) & 1u))
        return "4:2:0 needs an even Ho and Wo (BIN2: width and height multiples of 4)";
    if (const char *why = rgb_check_out(p, yv != nullptr, n, out, out_bytes, plan))
        return why;
    plan.invec = I.on_grid();
    if (full) {
        plan.tilesX = (static_cast<uint32_t>(width) + MHC_TW - 1u) / MHC_TW;
        plan.units = plan.tilesX * ((static_cast<uint32_t>(height) + MHC_TH - 1u) / MHC_TH);
    } else {
        plan.tilesX = static_cast<uint32_t>((plan.Wo + 7u) / 8u);
        // items: 8 output columns of an output row (YUV kinds: of an output row pair)
        plan.units = static_cast<uint32_t>((static_cast<size_t>(plan.tilesX) * (yv ? plan.Ho / 2u : plan.Ho) + RGB_T - 1u) / RGB_T);
    }
    return nullptr;
}

// ---- the window layer ---------------------------------------------------------------------------------------------------
//
// What the scaled entry points (mcraw_demosaic_area_batch: mcraw_area_args.h; mcraw_demosaic_resample_batch:
// mcraw_resample_args.h) share: both map a crop window (x0, y0, cw, ch) of the frame onto out_w x out_h pixels through two tables
// of taps in the caller's scratch.  A scaled stage brings its window struct, a plan with `rgb`, `total` and a geometry() for the
// struct's own rules (reserved fields, ratio, tiles), and its tap formula; the sequence of the checks is scaled_check's.
#if defined(__HIPCC__)
#define MCRAW_HD __host__ __device__
#else
#define MCRAW_HD
#endif

MCRAW_HD inline int64_t floordiv(int64_t a, int64_t b) // b > 0
{
    return a >= 0 ? a / b : -((-a + b - 1) / b);
}

constexpr size_t TAB_SECTION = 256u; // the tables of the scratch start on multiples of this

// The scratch of a scaled call: the taps of the Wo columns, then of the Ho rows, `tap` bytes each.
struct TabLayout {
    size_t xtab, ytab, total; // byte offsets of the two tables, and the size
};
inline TabLayout tab_layout(size_t Wo, size_t Ho, size_t tap)
{
    const auto up = [](size_t v) { return (v + TAB_SECTION - 1u) / TAB_SECTION * TAB_SECTION; };
    const size_t ytab = up(Wo * tap);
    return {0u, ytab, up(ytab + Ho * tap)};
}

// Why the window is none on its own (whether it fits the frame is scaled_check's question).
inline const char *crop_check(uint32_t x0, uint32_t y0, uint32_t cw, uint32_t ch)
{
    if ((x0 | y0 | cw | ch) & 1u)
        return "x0, y0, cw and ch must be even";
    if (cw < 2u || ch < 2u || cw > 65536u || ch > 65536u || x0 > 65536u || y0 > 65536u)
        return "the crop must be 2 .. 65536 wide and high";
    return nullptr;
}

// Where the two stages' checks differ: the algo code, the smallest frame, and the messages that name either.
struct ScaledRules {
    uint32_t algo;
    int min_side;
    const char *side_why, *algo_why, *work_why;
};

// Why the call is rejected, or nullptr with plan.rgb and the plan's geometry filled (plan.rgb.noop: an empty batch, nothing else
// is set); how the input is fetched (I.on_grid()) is left to the caller.  d: the display family, yv: the YUV family (never both);
// neither: the float family.  Addresses are only looked at as numbers.
template <class Win, class Plan>
inline const char *scaled_check(const ScaledRules &R, const mcraw_rgb *p, const Win *w, const mcraw_display *d, const mcraw_yuv *yv,
                                const mcraw_rgb_color *colors, int ncolors, const MosaicBatch &I, int n, const void *work,
                                size_t work_bytes, const void *out, size_t out_bytes, Plan &plan)
{
    plan = Plan{};
    if (!p || !w || n < 0)
        return "bad arguments";
    if (d && yv)
        return "a display stage and a YUV stage at once";
    if (n == 0) {
        plan.rgb.noop = true;
        return nullptr;
    }
    if (I.W < R.min_side || I.H < R.min_side || (I.W & 1) || (I.H & 1) || I.W > 65536 || I.H > 65536)
        return R.side_why;
    if (const char *why = I.check())
        return why;
    if (p->algo != R.algo)
        return R.algo_why;
    if (const char *why = rgb_check_stage(p, d, yv, colors, ncolors, n, plan.rgb))
        return why;
    if (const char *why = plan.geometry(w))
        return why;
    if (static_cast<uint64_t>(w->x0) + w->cw > static_cast<uint64_t>(I.W) || static_cast<uint64_t>(w->y0) + w->ch > static_cast<uint64_t>(I.H))
        return "the crop leaves the frame: x0 + cw > width or y0 + ch > height";
    if (yv && ((plan.rgb.Ho | plan.rgb.Wo) & 1u))
        return "4:2:0 needs an even out_h and out_w";
    if (const char *why = rgb_check_out(p, yv != nullptr, n, out, out_bytes, plan.rgb))
        return why;
    const uintptr_t k = reinterpret_cast<uintptr_t>(work);
    if (!k || (k & 15u))
        return "work missing or not 16-byte aligned";
    if (work_bytes < plan.total)
        return R.work_why;
    return nullptr;
}

} // namespace mcraw
