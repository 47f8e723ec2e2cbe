// mcraw_mesh_args.h -- what mcraw_demosaic_mesh_batch and mcraw_mesh_check (include/mcraw_hip.h) decide about a call before
// anything is launched: accept, reject or no-op; the position arithmetic of a mesh cell, in its 64-bit statement and in the 32-bit
// form the kernel uses where a cell allows it; a tile's source window from its four corner pixels, with the two clamps that make
// the result defined for every node content; and the plan of the launch.  The tile, the LDS arrays' sizes and the phase tables are
// the affine warp's (mcraw_warp_args.h).  No HIP in here, so that tests/cpp/mesh_args_check.cpp can drive it on any machine.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdio>

#include "mcraw_warp_args.h"

namespace mcraw {

static_assert(MCRAW_MESH_STEP == WARP_TW && MCRAW_MESH_STEP == WARP_TH && MCRAW_MESH_STEP == 32, "one node per corner of the warp's tile");
constexpr uint32_t MESH_NP = WARP_EROWS / 2u; // row pairs of estimates a tile may hold: the regime is np <= MESH_NP, ne <= MESH_NE
constexpr uint32_t MESH_NE = WARP_ECOLS / 8u; // pieces of 8 columns
constexpr int64_t MESH_NARROW = int64_t{1} << 21; // a cell whose nodes differ by less than this from the first: 32-bit sums

// The four nodes of a cell along one axis: (a, b), (a, b + 1), (a + 1, b), (a + 1, b + 1).
// The position of the cell's pixel (u, v), 0 <= u, v <= 31, before the clamp: the contract's 64-bit statement.
MCRAW_HD inline int64_t mesh_lerp64(const int32_t (&c)[4], uint32_t u, uint32_t v)
{
    const int64_t iu = 32 - static_cast<int64_t>(u), iv = 32 - static_cast<int64_t>(v);
    return (c[0] * (iu * iv) + c[1] * (iu * v) + c[2] * (u * iv) + c[3] * (static_cast<int64_t>(u) * v) + 512) >> 10;
}

// Whether the 32-bit form holds for the cell: with every |c[k] - c[0]| < 2^21 the sum below stays under 1024 (2^21 - 1) + 512 < 2^31.
MCRAW_HD inline bool mesh_narrow(const int32_t (&c)[4])
{
    bool ok = true;
    for (int k = 1; k < 4; k++) {
        const int64_t d = static_cast<int64_t>(c[k]) - c[0];
        ok = ok && d < MESH_NARROW && d > -MESH_NARROW;
    }
    return ok;
}

// The same position in 32 bits, relative to c[0] (1024 c[0] drops out of the shift).  A lane's pixels share u: l and r, the row's
// ends times 32, hoist out.  Only for a cell that mesh_narrow() accepts; equal to mesh_lerp64 there.
MCRAW_HD inline void mesh_row32(const int32_t (&c)[4], uint32_t u, int32_t &l, int32_t &r)
{
    const int32_t iu = 32 - static_cast<int32_t>(u), su = static_cast<int32_t>(u);
    l = (c[2] - c[0]) * su;
    r = (c[1] - c[0]) * iu + (c[3] - c[0]) * su;
}
MCRAW_HD inline int32_t mesh_lerp32(int32_t c0, int32_t l, int32_t r, uint32_t v)
{
    return c0 + ((l * (32 - static_cast<int32_t>(v)) + r * static_cast<int32_t>(v) + 512) >> 10);
}

MCRAW_HD inline int64_t mesh_clamp(int64_t v, int side) // side: height or width
{
    const int64_t top = 256 * (static_cast<int64_t>(side) - 1);
    return v < 0 ? 0 : v > top ? top : v;
}

MCRAW_HD inline int32_t mesh_clamp32(int32_t v, int side) // the same clamp for a position that is an int32 already (256 (65536 - 1) < 2^24)
{
    const int32_t top = 256 * (side - 1);
    return v < 0 ? 0 : v > top ? top : v;
}

// The estimates a tile reads: warp_window's formula over the clamped positions of the tile's four corner pixels (0 | u1, 0 | v1) of
// its cell, u1 and v1 the tile's last row and column.  A bilinear function takes its extremes over a rectangle at the corners, the
// floor and the clamp are monotone: the corners bound every pixel.  np and ne are what the positions ask for; the kernel holds
// min(np, MESH_NP) x min(ne, MESH_NE) and clamps the tap origins into that (mesh_tap_max).
MCRAW_HD inline WarpWin mesh_window(const int32_t (&cy)[4], const int32_t (&cx)[4], uint32_t u1, uint32_t v1, int width, int height)
{
    int64_t ylo = 0, yhi = 0, xlo = 0, xhi = 0;
    for (int c = 0; c < 4; c++) {
        const uint32_t u = (c & 2) ? u1 : 0u, v = (c & 1) ? v1 : 0u;
        const int64_t y = mesh_clamp(mesh_lerp64(cy, u, v), height), x = mesh_clamp(mesh_lerp64(cx, u, v), width);
        ylo = (c == 0 || y < ylo) ? y : ylo, yhi = (c == 0 || y > yhi) ? y : yhi;
        xlo = (c == 0 || x < xlo) ? x : xlo, xhi = (c == 0 || x > xhi) ? x : xhi;
    }
    WarpWin w;
    w.pb = static_cast<int32_t>(((ylo >> 8) - 1) & ~int64_t{1});
    w.eb = static_cast<int32_t>(((xlo >> 8) - 1) & ~int64_t{7});
    w.np = static_cast<uint32_t>((((yhi >> 8) + 2 - w.pb) >> 1) + 1);
    w.ne = static_cast<uint32_t>((((xhi >> 8) + 2 - w.eb) >> 3) + 1);
    return w;
}
MCRAW_HD inline bool mesh_in_regime(const WarpWin &w) { return w.np <= MESH_NP && w.ne <= MESH_NE; }
// The largest first tap row (column) relative to pb (eb) in a window of np' row pairs (ne' pieces).
MCRAW_HD inline int32_t mesh_tap_max_row(uint32_t np) { return 2 * static_cast<int32_t>(np < MESH_NP ? np : MESH_NP) - 4; }
MCRAW_HD inline int32_t mesh_tap_max_col(uint32_t ne) { return 8 * static_cast<int32_t>(ne < MESH_NE ? ne : MESH_NE) - 4; }

struct MeshPlan {
    RgbPlan rgb;               // noop, kind, shift, es, Wo, Ho, frame_samples, out_frame, invec (mhc, tilesX, units: unused)
    uint32_t tilesX = 0, tilesY = 0, units = 0;
    uint32_t Mx = 0, My = 0;   // nodes per row and rows of nodes of a mesh
    bool permesh = false;      // a mesh per frame

    // Why `m` alone gives no geometry, or nullptr with the tiles and the nodes filled.
    const char *geometry(const mcraw_mesh *m)
    {
        if (m->reserved != 0u)
            return "reserved must be 0";
        if (m->filter != MCRAW_FILTER_LINEAR && m->filter != MCRAW_FILTER_CUBIC)
            return "unknown filter";
        if (m->out_w < 1u || m->out_h < 1u || m->out_w > 65536u || m->out_h > 65536u)
            return "out_w and out_h must be 1 .. 65536";
        rgb.Wo = m->out_w, rgb.Ho = m->out_h;
        tilesX = (m->out_w + WARP_TW - 1u) / WARP_TW;
        tilesY = (m->out_h + WARP_TH - 1u) / WARP_TH;
        units = tilesX * tilesY;
        Mx = tilesX + 1u, My = tilesY + 1u;
        return nullptr;
    }
    size_t nodes() const { return static_cast<size_t>(My) * Mx; }
};

// The cell of tile (ty, tx) out of one mesh (My x Mx nodes of (Y, X)).
inline void mesh_cell(const int32_t *mesh, uint32_t Mx, uint32_t ty, uint32_t tx, int32_t (&cy)[4], int32_t (&cx)[4])
{
    for (int c = 0; c < 4; c++) {
        const int32_t *nd = mesh + 2u * ((static_cast<size_t>(ty) + static_cast<size_t>(c >> 1)) * Mx + tx + static_cast<size_t>(c & 1));
        cy[c] = nd[0], cx[c] = nd[1];
    }
}

// mcraw_mesh_check: why nmesh meshes in HOST memory are none for width x height frames, or nullptr.  The message names the first
// frame and tile whose window leaves the regime, or (flags & 1) where a corner pixel's unclamped position leaves the frame; it
// lives in a buffer of the calling thread.
inline const char *mesh_nodes_check(const mcraw_mesh *m, const int32_t *nodes, int nmesh, int width, int height, int flags)
{
    MeshPlan P;
    if (!m || !nodes)
        return "bad arguments";
    if (width < 8 || height < 8 || (width & 1) || (height & 1) || width > 65536 || height > 65536)
        return "width and height must be even, 8 .. 65536";
    if (const char *why = P.geometry(m))
        return why;
    if (nmesh < 1)
        return "nmesh must be at least 1";
    if (flags & ~1)
        return "unknown flag";
    static thread_local char msg[256];
    for (int f = 0; f < nmesh; f++) {
        const int32_t *mesh = nodes + 2u * P.nodes() * static_cast<size_t>(f);
        for (uint32_t ty = 0; ty < P.tilesY; ty++)
            for (uint32_t tx = 0; tx < P.tilesX; tx++) {
                int32_t cy[4], cx[4];
                mesh_cell(mesh, P.Mx, ty, tx, cy, cx);
                const uint32_t u1 = (m->out_h - ty * WARP_TH < WARP_TH ? m->out_h - ty * WARP_TH : WARP_TH) - 1u;
                const uint32_t v1 = (m->out_w - tx * WARP_TW < WARP_TW ? m->out_w - tx * WARP_TW : WARP_TW) - 1u;
                const WarpWin w = mesh_window(cy, cx, u1, v1, width, height);
                if (!mesh_in_regime(w)) {
                    std::snprintf(msg, sizeof(msg), "the mesh of frame %d: tile (%u, %u) reads %u row pairs x %u column pieces, above %u x %u", f,
                                  ty, tx, w.np, w.ne, MESH_NP, MESH_NE);
                    return msg;
                }
                for (int c = 0; (flags & 1) && c < 4; c++) {
                    const uint32_t u = (c & 2) ? u1 : 0u, v = (c & 1) ? v1 : 0u;
                    const int64_t y = mesh_lerp64(cy, u, v), x = mesh_lerp64(cx, u, v);
                    if (y != mesh_clamp(y, height) || x != mesh_clamp(x, width)) {
                        std::snprintf(msg, sizeof(msg), "the mesh of frame %d: a corner pixel of tile (%u, %u) leaves the frame: (%lld, %lld)", f, ty,
                                      tx, static_cast<long long>(y), static_cast<long long>(x));
                        return msg;
                    }
                }
            }
    }
    return nullptr;
}

// Why the call is rejected, or nullptr with `plan` filled (plan.rgb.noop: an empty batch, nothing else is set), in warp_check's
// order.  d: the display family, yv: the YUV family (never both); neither: the float family.  Addresses are only looked at as
// numbers: the nodes are DEVICE memory, and no node content is an error (the kernel's two clamps).
inline const char *mesh_check(const mcraw_rgb *p, const mcraw_mesh *m, const mcraw_display *d, const mcraw_yuv *yv,
                              const mcraw_rgb_color *colors, int ncolors, const int32_t *nodes, size_t nodes_bytes, int nmesh,
                              const uint16_t *in, size_t in_pitch, size_t in_frame_stride, int width, int height, int n, const void *out,
                              size_t out_bytes, MeshPlan &plan)
{
    plan = MeshPlan{};
    if (!p || !m || !nodes || n < 0)
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
    if (p->algo != MCRAW_RGB_MESH)
        return "p->algo must be MCRAW_RGB_MESH";
    if (const char *why = rgb_check_stage(p, d, yv, colors, ncolors, n, plan.rgb))
        return why;
    if (const char *why = plan.geometry(m))
        return why;
    if (yv && ((plan.rgb.Ho | plan.rgb.Wo) & 1u))
        return "4:2:0 needs an even out_h and out_w";
    if (nmesh != 1 && nmesh != n)
        return "nmesh must be 1 or n";
    if (reinterpret_cast<uintptr_t>(nodes) & 7u)
        return "nodes not 8-byte aligned";
    if (nodes_bytes / 8u / plan.nodes() < static_cast<size_t>(nmesh))
        return "nodes_bytes below nmesh * My * Mx * 8";
    if (const char *why = rgb_check_out(p, yv != nullptr, n, out, out_bytes, plan.rgb))
        return why;
    plan.permesh = nmesh > 1;
    plan.rgb.invec = I.on_grid();
    return nullptr;
}

} // namespace mcraw
