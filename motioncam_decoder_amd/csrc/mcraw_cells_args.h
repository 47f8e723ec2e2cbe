// mcraw_cells_args.h -- the geometry of the position field (include/mcraw_hip.h): the grid of cells that
// mcraw_align_cells_batch writes and mcraw_merge_cells_batch reads, the estimator's pyramid planes, the layout of its scratch
// and the checks on both calls' own arguments.  No HIP in here, so that tests/cpp/cells_args_check.cpp can drive it on any
// machine.  The batch of mosaics itself is checked by MosaicBatch.
#pragma once
#include <cstddef>
#include <cstdint>

#include "mcraw_mosaic_args.h"

namespace mcraw {

constexpr uint32_t CL_MAXLEVELS = 3u, CL_MAXRADIUS = 4u;
constexpr uint32_t CL_GRID_H = 32u, CL_GRID_W = 256u; // a cell is whole merge tiles of either build, and whole pixels of levels 0 .. 2
constexpr size_t CL_SECTION = 256u;                   // the sections of the scratch start on multiples of this

// The winner of one cell of one pair at one level: the displacement in that level's pixels (the centre included) and its SAD.
struct CellWin {
    int32_t dy, dx;
    uint64_t sad;
};

// The grid of cells over a frame.
struct CellGrid {
    uint32_t cell_h = 0, cell_w = 0, cells_y = 0, cells_x = 0;

    // Why these arguments give no grid, or nullptr.
    const char *make(int width, int height, uint32_t cell_h_, uint32_t cell_w_)
    {
        if (width < 1 || height < 1 || width > 65536 || height > 65536)
            return "width and height must be 1 .. 65536";
        if (cell_h_ == 0u || cell_h_ % CL_GRID_H != 0u || cell_h_ > 65536u)
            return "cell_h must be a multiple of 32 in 32 .. 65536";
        if (cell_w_ == 0u || cell_w_ % CL_GRID_W != 0u || cell_w_ > 65536u)
            return "cell_w must be a multiple of 256 in 256 .. 65536";
        cell_h = cell_h_, cell_w = cell_w_;
        cells_y = (static_cast<uint32_t>(height) + cell_h - 1u) / cell_h;
        cells_x = (static_cast<uint32_t>(width) + cell_w - 1u) / cell_w;
        return nullptr;
    }
    size_t cells() const { return static_cast<size_t>(cells_y) * cells_x; }
    size_t field_bytes(size_t n) const { return n * cells() * 4u; } // (n, cells_y, cells_x, 2) int16
};

struct CellsPlan {
    uint32_t levels = 0, radius = 0;
    CellGrid G;
    uint32_t h[CL_MAXLEVELS] = {}, w[CL_MAXLEVELS] = {}; // the planes' sizes (a plane may be empty: frames of 1 .. 15 samples)
    uint32_t pitch[CL_MAXLEVELS] = {};                   // elements from row to row: w rounded up to 8 (16-byte rows)
    size_t off[CL_MAXLEVELS] = {};                       // elements from a frame's pyramid to its level l
    size_t frame_elems = 0;                              // elements from pyramid to pyramid
    uint32_t acc0[CL_MAXLEVELS] = {};                    // index of level l's first sum among a cell's sums
    uint32_t nacc = 0;                                   // 64-bit sums per frame and cell: (2 radius + 1)^2 at the coarsest level, 9 below
    size_t pyr = 0, acc = 0, win = 0, total = 0;         // byte offsets of the three sections in the scratch, and its size

    static uint32_t cands(uint32_t r) { return (2u * r + 1u) * (2u * r + 1u); }

    // Why these arguments give no plan, or nullptr.
    const char *make(int width, int height, size_t n, uint32_t levels_, uint32_t radius_, uint32_t cell_h, uint32_t cell_w)
    {
        if (levels_ < 1u || levels_ > CL_MAXLEVELS)
            return "levels must be 1 .. 3";
        if (radius_ < 1u || radius_ > CL_MAXRADIUS)
            return "radius must be 1 .. 4";
        if (const char *why = G.make(width, height, cell_h, cell_w))
            return why;
        levels = levels_, radius = radius_;
        size_t o = 0;
        for (uint32_t l = 0; l < levels; l++) {
            h[l] = l ? h[l - 1u] / 2u : static_cast<uint32_t>(height) / 2u;
            w[l] = l ? w[l - 1u] / 2u : static_cast<uint32_t>(width) / 2u;
            pitch[l] = (w[l] + 7u) / 8u * 8u;
            off[l] = o;
            o += static_cast<size_t>(h[l]) * pitch[l];
        }
        frame_elems = o;
        nacc = 0;
        for (uint32_t l = levels; l-- > 0u;) { // coarsest first
            acc0[l] = nacc;
            nacc += l == levels - 1u ? cands(radius) : 9u;
        }
        const auto up = [](size_t v) { return (v + CL_SECTION - 1u) / CL_SECTION * CL_SECTION; };
        pyr = 0;
        acc = up(pyr + n * frame_elems * 2u);
        win = up(acc + n * G.cells() * nacc * 8u);
        total = up(win + n * G.cells() * CL_MAXLEVELS * sizeof(CellWin));
        return nullptr;
    }
};

// Why mcraw_align_cells_batch's own pointers cannot be used, or nullptr: the field pos (n, cells_y, cells_x, 2) int16, sad (n,
// cells_y, cells_x) uint64 or NULL, gpos (n, 2) int16 or NULL (read), work of work_bytes bytes, the input's extent I, a plan P
// made for the call.
inline const char *check_cells_ptrs(const MosaicBatch &I, const CellsPlan &P, size_t n, const void *pos, const void *sad, const void *gpos,
                                    const void *work, size_t work_bytes)
{
    const uintptr_t p = reinterpret_cast<uintptr_t>(pos), s = reinterpret_cast<uintptr_t>(sad), g = reinterpret_cast<uintptr_t>(gpos),
                    k = reinterpret_cast<uintptr_t>(work);
    if (!p || !k)
        return "pos or work missing";
    if ((p & 1u) || (g & 1u))
        return "pos or gpos not aligned to 2 bytes";
    if (s & 7u)
        return "sad not 8-byte aligned";
    if (k & 15u)
        return "work not 16-byte aligned";
    if (work_bytes < P.total)
        return "work_bytes below mcraw_align_cells_work_bytes(width, height, n, levels, radius, cell_h, cell_w)";
    const size_t np = P.G.field_bytes(n), ns = s ? n * P.G.cells() * 8u : 0u, ng = g ? n * 4u : 0u;
    if (ranges_overlap(I.base, I.bytes(), p, np) || (s && ranges_overlap(I.base, I.bytes(), s, ns)) ||
        ranges_overlap(I.base, I.bytes(), k, P.total))
        return "pos, sad or work overlaps the input";
    if (ranges_overlap(k, P.total, p, np) || (s && (ranges_overlap(k, P.total, s, ns) || ranges_overlap(p, np, s, ns))))
        return "pos, sad and work overlap one another";
    if (g && (ranges_overlap(g, ng, p, np) || (s && ranges_overlap(g, ng, s, ns)) || ranges_overlap(g, ng, k, P.total)))
        return "gpos overlaps pos, sad or work";
    return nullptr;
}

// Why mcraw_merge_cells_batch's field cannot be used, or nullptr: the grid the caller states against the frames' own, the field's
// address, and the field (n frames) against the output's extent O.
inline const char *check_merge_cells(const MosaicBatch &O, size_t n, int width, int height, uint32_t cell_h, uint32_t cell_w, uint32_t cells_y,
                                     uint32_t cells_x, uint32_t reserved, const void *field)
{
    CellGrid G;
    if (const char *why = G.make(width, height, cell_h, cell_w))
        return why;
    if (cells_y != G.cells_y || cells_x != G.cells_x)
        return "cells_y and cells_x must be ceil(height / cell_h) and ceil(width / cell_w)";
    if (reserved != 0u)
        return "the cells' reserved must be 0";
    const uintptr_t f = reinterpret_cast<uintptr_t>(field);
    if (!f)
        return "the cells' pos missing";
    if (f & 1u)
        return "the cells' pos not aligned to 2 bytes";
    if (ranges_overlap(O.base, O.bytes(), f, G.field_bytes(n)))
        return "the cells' pos overlaps the output";
    return nullptr;
}

} // namespace mcraw
