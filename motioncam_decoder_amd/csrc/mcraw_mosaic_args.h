// mcraw_mosaic_args.h -- one strided batch of uint16 mosaics as the mosaic stages' entry points are handed it (base, pitch and
// frame stride in elements, frames, width, height), and the checks on it that they share.  No HIP in here, so that
// tests/cpp/mosaic_args_check.cpp can drive it on any machine.  A stage's own arguments (its struct, its tables, an in-place
// form) are checked in its own unit.
#pragma once
#include <cstddef>
#include <cstdint>

namespace mcraw {

struct MosaicBatch {
    uintptr_t base;        // address of the first sample of the first frame
    size_t pitch, fstride; // elements from row to row, from frame to frame (the latter unused for one frame)
    size_t frames;         // at least 1
    int W, H;

    MosaicBatch(const void *p, size_t pitch_, size_t fstride_, size_t frames_, int width, int height)
        : base(reinterpret_cast<uintptr_t>(p)), pitch(pitch_), fstride(fstride_), frames(frames_), W(width), H(height)
    {
    }

    // Why the batch cannot be used, or nullptr.
    const char *check() const
    {
        if (!base)
            return "in or out missing";
        if (base & 1u)
            return "in / out not aligned to uint16";
        if (W < 1 || H < 1 || W > 65536 || H > 65536)
            return "width and height must be 1 .. 65536";
        if (pitch < static_cast<size_t>(W))
            return "pitch below width";
        if (frames > 1u && fstride < frame_extent())
            return "frame stride too small for the frames not to overlap";
        return nullptr;
    }

    // (the three below: of a batch that passed check())
    // elements from the first sample of a frame to behind its last one
    size_t frame_extent() const { return (static_cast<size_t>(H) - 1u) * pitch + static_cast<size_t>(W); }
    // elements from the first sample of the first frame to behind the last sample of the last one
    size_t extent() const { return (frames - 1u) * fstride + frame_extent(); }
    size_t bytes() const { return 2u * extent(); }
    // every 8-column piece of every row lies on the 16-byte grid
    bool on_grid() const { return (base & 15u) == 0u && pitch % 8u == 0u && (frames == 1u || fstride % 8u == 0u); }
};

// Why either of a stage's two batches cannot be used, or nullptr.
inline const char *check(const MosaicBatch &in, const MosaicBatch &out)
{
    const char *why = in.check();
    return why ? why : out.check();
}

// Do the byte ranges [a, a + na) and [b, b + nb) share a byte?
inline bool ranges_overlap(uintptr_t a, size_t na, uintptr_t b, size_t nb)
{
    return a < b + nb && b < a + na;
}

inline bool overlap(const MosaicBatch &a, const MosaicBatch &b)
{
    return ranges_overlap(a.base, a.bytes(), b.base, b.bytes());
}

} // namespace mcraw
