// mcraw_align_args.h -- the geometry of mcraw_align_batch (include/mcraw_hip.h): the pyramid's planes, the levels' bounds, the
// layout of the caller's scratch and the checks on the call's own arguments.  No HIP in here, so that
// tests/cpp/align_args_check.cpp can drive it on any machine.  The batch of mosaics itself is checked by MosaicBatch.
#pragma once
#include <cstddef>
#include <cstdint>

#include "mcraw_mosaic_args.h"

namespace mcraw {

constexpr uint32_t AL_MAXLEVELS = 6u, AL_MAXRADIUS = 8u;
constexpr size_t AL_SECTION = 256u; // the sections of the scratch start on multiples of this

// The winner of one pair at one level: the displacement in that level's pixels and its SAD.
struct AlignWin {
    int32_t dy, dx;
    uint64_t sad;
};

struct AlignPlan {
    uint32_t levels = 0, radius = 0;
    uint32_t h[AL_MAXLEVELS] = {}, w[AL_MAXLEVELS] = {}; // the planes' sizes
    uint32_t pitch[AL_MAXLEVELS] = {};                   // elements from row to row: w rounded up to 8 (16-byte rows)
    uint32_t B[AL_MAXLEVELS] = {};                       // the bound of the displacement = the margin of the window
    size_t off[AL_MAXLEVELS] = {};                       // elements from a frame's pyramid to its level l
    size_t frame_elems = 0;                              // elements from pyramid to pyramid
    uint32_t acc0[AL_MAXLEVELS] = {};                    // index of level l's first sum among a frame's sums
    uint32_t nacc = 0;                                   // 64-bit sums per frame: (2 radius + 1)^2 at the coarsest level, 9 below
    size_t pyr = 0, acc = 0, win = 0, total = 0;         // byte offsets of the three sections in the scratch, and its size

    static uint32_t cands(uint32_t r) { return (2u * r + 1u) * (2u * r + 1u); }

    // Why these arguments give no plan, or nullptr (width, height: 1 .. 65536, checked by the caller's MosaicBatch).
    const char *make(int width, int height, size_t n, uint32_t levels_, uint32_t radius_)
    {
        if (levels_ < 1u || levels_ > AL_MAXLEVELS)
            return "levels must be 1 .. 6";
        if (radius_ < 1u || radius_ > AL_MAXRADIUS)
            return "radius must be 1 .. 8";
        if (width < 1 || height < 1 || width > 65536 || height > 65536)
            return "width and height must be 1 .. 65536";
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
        B[levels - 1u] = radius;
        for (uint32_t l = levels - 1u; l-- > 0u;)
            B[l] = 2u * B[l + 1u] + 1u;
        for (uint32_t l = 0; l < levels; l++)
            if (h[l] < 2u * B[l] + 1u || w[l] < 2u * B[l] + 1u)
                return "the comparison window is empty at a level (h(l) - 2 B(l) < 1 or w(l) - 2 B(l) < 1): fewer levels, a "
                       "smaller radius or larger frames";
        nacc = 0;
        for (uint32_t l = levels; l-- > 0u;) { // coarsest first
            acc0[l] = nacc;
            nacc += l == levels - 1u ? cands(radius) : 9u;
        }
        const auto up = [](size_t v) { return (v + AL_SECTION - 1u) / AL_SECTION * AL_SECTION; };
        pyr = 0;
        acc = up(pyr + n * frame_elems * 2u);
        win = up(acc + n * nacc * 8u);
        total = up(win + n * AL_MAXLEVELS * sizeof(AlignWin));
        return nullptr;
    }
};

// Why the call's own pointers cannot be used, or nullptr: pos (n, 2) int16, sad n uint64 or NULL, work of work_bytes bytes, the
// input's extent I, a plan P made for the call.
inline const char *check_align_ptrs(const MosaicBatch &I, const AlignPlan &P, size_t n, const void *pos, const void *sad,
                                    const void *work, size_t work_bytes)
{
    const uintptr_t p = reinterpret_cast<uintptr_t>(pos), s = reinterpret_cast<uintptr_t>(sad), k = reinterpret_cast<uintptr_t>(work);
    if (!p || !k)
        return "pos or work missing";
    if (p & 1u)
        return "pos not aligned to 2 bytes";
    if (s & 7u)
        return "sad not 8-byte aligned";
    if (k & 15u)
        return "work not 16-byte aligned";
    if (work_bytes < P.total)
        return "work_bytes below mcraw_align_work_bytes(width, height, n, levels, radius)";
    const size_t np = n * 4u, ns = s ? n * 8u : 0u;
    if (ranges_overlap(I.base, I.bytes(), p, np) || (s && ranges_overlap(I.base, I.bytes(), s, ns)) ||
        ranges_overlap(I.base, I.bytes(), k, P.total))
        return "pos, sad or work overlaps the input";
    if (ranges_overlap(k, P.total, p, np) || (s && (ranges_overlap(k, P.total, s, ns) || ranges_overlap(p, np, s, ns))))
        return "pos, sad and work overlap one another";
    return nullptr;
}

} // namespace mcraw
