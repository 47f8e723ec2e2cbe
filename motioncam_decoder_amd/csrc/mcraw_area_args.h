// mcraw_area_args.h -- what mcraw_demosaic_area_batch (include/mcraw_hip.h) decides about a call before anything is launched:
// accept, reject or no-op; on acceptance the plan of the launch (the workgroup's tile, the LDS segment, the staging mode) and the
// layout of the caller's scratch; and the weight formula itself, as a plain function that the table kernel and the tests share.
// No HIP in here, so that tests/cpp/area_args_check.cpp can drive it on any machine.  The family's own rules (display / YUV
// struct, dtype, cfa, white, colours, `out`) are rgb_check's pieces (mcraw_rgb_args.h), run in rgb_check's order; the sequence
// of the checks, the crop's rules and the scratch's layout are that header's window layer, shared with mcraw_resample_args.h.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "mcraw_rgb_args.h"

namespace mcraw {

constexpr uint32_t AREA_TAPS = 17u;     // quads under an output pixel along one axis, at most (ratio <= 16)
constexpr uint32_t AREA_MAXRATIO = 16u; // Q <= 16 O
constexpr uint32_t AREA_TILE_Q = 2560u; // LDS: quad slots of a workgroup's tile (8 bytes each, 20 KiB)
constexpr uint32_t AREA_WXN = 4096u;    // LDS: horizontal weights of a workgroup's columns (uint16, 8 KiB)
constexpr uint32_t AREA_YN = 128u;      // LDS: (first quad row, taps) of a group's output rows; 2 per row pair, at most 64 row pairs
constexpr uint32_t AREA_BAND = 8u;      // groups of row pairs that a workgroup makes with one set of horizontal weights
constexpr size_t AREA_SECTION = TAB_SECTION; // the tables of the scratch start on multiples of this

// One output column or row in the scratch: the first quad under it, how many quads carry weight, and the weights (256 in
// all; those behind `nt` are 0).
struct AreaTap {
    uint32_t q0;
    uint16_t nt;
    uint16_t w[AREA_TAPS];
};
static_assert(sizeof(AreaTap) == 40, "the scratch is laid out in entries of 40 bytes");

// c(k, q) of the contract: the part of output pixel k's footprint [k Q / O, (k + 1) Q / O) that lies in front of quad q, in
// 1/256 of the footprint, rounded to nearest and clamped.  Q quads onto O pixels, O <= Q <= 16 O, Q <= 32768.
MCRAW_HD inline int32_t area_c(uint32_t k, uint32_t q, uint32_t Q, uint32_t O)
{
    const int64_t num = 256 * (static_cast<int64_t>(q) * O - static_cast<int64_t>(k) * Q) + static_cast<int64_t>(Q >> 1);
    const int64_t fl = floordiv(num, static_cast<int64_t>(Q));
    return static_cast<int32_t>(fl < 0 ? 0 : fl > 256 ? 256 : fl);
}

// The taps of output pixel k: w(k, q) = c(k, q + 1) - c(k, q) from q0 = floor(k Q / O) on.
MCRAW_HD inline void area_taps(uint32_t k, uint32_t Q, uint32_t O, AreaTap &t)
{
    t.q0 = static_cast<uint32_t>(static_cast<uint64_t>(k) * Q / O);
    t.nt = 0;
    int32_t c0 = area_c(k, t.q0, Q, O);
    for (uint32_t i = 0; i < AREA_TAPS; i++) {
        int32_t c1 = c0;
        if (t.q0 + i < Q)
            c1 = area_c(k, t.q0 + i + 1u, Q, O);
        t.w[i] = static_cast<uint16_t>(c1 - c0);
        if (c1 != c0)
            t.nt = static_cast<uint16_t>(i + 1u);
        c0 = c1;
    }
}

// No pixel of the axis has more taps than this: Q / O for a whole ratio, floor(Q / O) + 2 otherwise.
constexpr uint32_t area_tap_bound(uint32_t Q, uint32_t O) { return Q % O ? Q / O + 2u : Q / O; }

struct AreaPlan {
    RgbPlan rgb;              // noop, kind, shift, es, Wo, Ho, frame_samples, out_frame (mhc, invec, tilesX, units: unused)
    uint32_t Qw = 0, Qh = 0;  // quads of the crop
    uint32_t ntx = 0, nty = 0; // area_tap_bound of the axes
    uint32_t mode = 0;        // how a quad row is fetched: 2 = 16-byte pieces on the grid, 1 = aligned dwords, 0 = uint16 pairs
    // the workgroup: lx lanes side by side (8 output columns each) times ly row pairs, lx * ly <= 256
    uint32_t lx_log2 = 0, ly = 0;
    uint32_t seg = 0, segp = 0; // quads of a row pair's LDS segment; its slots (one pad slot behind every 8 quads)
    uint32_t nch = 0, nch_magic = 0; // 16-byte pieces per segment; ceil(2^32 / nch)
    uint32_t tilesX = 0, groups = 0, bands = 0, units = 0; // column tiles; groups of ly row pairs; bands of AREA_BAND groups; tilesX * bands
    size_t xtab = 0, ytab = 0, total = 0; // byte offsets of the two tables in the scratch, and its size

    // Why `a` alone gives no geometry, or nullptr with everything above (mode aside) filled.
    const char *geometry(const mcraw_area *a)
    {
        if (a->reserved[0] != 0u || a->reserved[1] != 0u)
            return "reserved must be 0";
        if (const char *why = crop_check(a->x0, a->y0, a->cw, a->ch))
            return why;
        Qw = a->cw / 2u, Qh = a->ch / 2u;
        const uint32_t Wo = a->out_w, Ho = a->out_h;
        if (Wo < 1u || Wo > Qw || Qw > static_cast<uint64_t>(AREA_MAXRATIO) * Wo || Ho < 1u || Ho > Qh ||
            Qh > static_cast<uint64_t>(AREA_MAXRATIO) * Ho)
            return "the output must be 1/16 .. 1 of the crop's quads: 1 <= out_w <= cw / 2 <= 16 out_w, likewise out_h";
        rgb.Wo = Wo, rgb.Ho = Ho;
        ntx = area_tap_bound(Qw, Wo), nty = area_tap_bound(Qh, Ho);
        const uint32_t cols8 = (Wo + 7u) / 8u, pairs = (Ho + 1u) / 2u;
        // the widest tile whose segment and weights fit, then as many row pairs as fit beside each other
        const auto seg_of = [&](uint32_t lx) { return ((8u * lx * Qw + Wo - 1u) / Wo + 1u + 7u + 3u + 3u) & ~3u; };
        const auto pad = [](uint32_t s) { return s + s / 8u + 1u; };
        uint32_t lx = 1u, l2 = 0u;
        while (lx < RGB_T && lx < cols8)
            lx *= 2u, l2++;
        while (lx > 1u && (pad(seg_of(lx)) > AREA_TILE_Q || 8u * lx * ntx > AREA_WXN))
            lx /= 2u, l2--;
        lx_log2 = l2;
        seg = seg_of(lx), segp = pad(seg);
        ly = std::min(RGB_T / lx, AREA_YN / 2u);
        while (ly > 1u && (ly * segp > AREA_TILE_Q || ly / 2u >= pairs))
            ly /= 2u;
        nch = seg / 4u;
        nch_magic = static_cast<uint32_t>(((uint64_t{1} << 32) + nch - 1u) / nch);
        tilesX = (cols8 + lx - 1u) / lx;
        groups = (pairs + ly - 1u) / ly;
        bands = (groups + AREA_BAND - 1u) / AREA_BAND;
        units = tilesX * bands;
        const TabLayout L = tab_layout(Wo, Ho, sizeof(AreaTap));
        xtab = L.xtab, ytab = L.ytab, total = L.total;
        return nullptr;
    }
};

// Why the call is rejected, or nullptr with `plan` filled (plan.rgb.noop: an empty batch, nothing else is set).  d: the display
// family, yv: the YUV family (never both); neither: the float family.  Addresses are only looked at as numbers.
inline const char *area_check(const mcraw_rgb *p, const mcraw_area *a, const mcraw_display *d, const mcraw_yuv *yv,
                              const mcraw_rgb_color *colors, int ncolors, const uint16_t *in, size_t in_pitch, size_t in_frame_stride,
                              int width, int height, int n, const void *work, size_t work_bytes, const void *out, size_t out_bytes,
                              AreaPlan &plan)
{
    constexpr ScaledRules R{MCRAW_RGB_AREA, 4, "width and height must be even, 4 .. 65536", "p->algo must be MCRAW_RGB_AREA",
                            "work_bytes below mcraw_area_work_bytes(a)"};
    const MosaicBatch I(in, in_pitch, in_frame_stride, static_cast<size_t>(n), width, height);
    const char *why = scaled_check(R, p, a, d, yv, colors, ncolors, I, n, work, work_bytes, out, out_bytes, plan);
    if (!why && !plan.rgb.noop)
        plan.mode = I.on_grid() ? 2u : ((I.base & 3u) == 0u && I.pitch % 2u == 0u && (I.frames == 1u || I.fstride % 2u == 0u)) ? 1u : 0u;
    return why;
}

} // namespace mcraw
