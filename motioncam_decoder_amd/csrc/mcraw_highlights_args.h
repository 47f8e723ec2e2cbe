// mcraw_highlights_args.h -- the host side of mcraw_highlights_batch / mcraw_highlights_measure_batch (include/mcraw_hip.h): the
// checks on the struct and on the records, and what the host derives from the struct for the kernels (inv, m, cap, the green
// positions of a cfa).  No HIP in here, so that tests/cpp/highlights_args_check.cpp can drive it on any machine.  The two batches
// of mosaics themselves are checked by MosaicBatch, but for the smallest size, which is 2 here.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/mcraw_hip.h"
#include "mcraw_mosaic_args.h"

namespace mcraw {

constexpr size_t HL_REC_BYTES = 64u;          // int64 sum[4]; uint32 cnt[4]; uint32 pad[4]
constexpr int32_t HL_CHROMA_MAX = 1 << 20;    // |chroma| is clamped to this

// The white-balanced value of a sample: d * gain + 2048 <= 65535 * 65535 + 2048 < 2^32, v <= 1048544 < 2^20.
inline uint32_t hl_wb(uint32_t s, uint32_t black, uint32_t gain)
{
    const uint32_t d = s > black ? s - black : 0u;
    return (d * gain + 2048u) >> 12;
}

// inv = ((1 << 24) + gain / 2) / gain: 65536 at gain 256, 256 at gain 65535.
inline uint32_t hl_inv(uint32_t gain)
{
    return ((1u << 24) + gain / 2u) / gain;
}

// A white-balanced value back at a position: black + ((v * inv + 2048) >> 12), the product in uint64 (v <= 2^21, inv <= 2^16).
inline uint32_t hl_back(uint32_t v, uint32_t black, uint32_t inv)
{
    return black + static_cast<uint32_t>((static_cast<uint64_t>(v) * inv + 2048u) >> 12);
}

// Is CFA position p green?  RGGB and BGGR: positions 1 and 2; GRBG and GBRG: 0 and 3.
inline bool hl_green(uint32_t cfa, uint32_t p)
{
    return (((p & 1u) ^ (p >> 1)) != 0u) == (cfa < 2u);
}

// What the kernels get beside the struct's own fields.
struct HlDerived {
    uint32_t inv[4];
    uint32_t m;      // the lowest white-balanced clip level
    uint32_t cap[4]; // CLIP: out = min(s, cap[p]); may be 65536 and above, where it changes nothing
};

inline HlDerived hl_derive(const mcraw_highlights &h)
{
    HlDerived d{};
    d.m = 0xFFFFFFFFu;
    for (int p = 0; p < 4; p++) {
        d.inv[p] = hl_inv(h.gain[p]);
        const uint32_t v = hl_wb(h.sat[p], h.black[p], h.gain[p]);
        d.m = v < d.m ? v : d.m;
    }
    for (int p = 0; p < 4; p++)
        d.cap[p] = hl_back(d.m, h.black[p], d.inv[p]);
    return d;
}

// Why the struct cannot be used for a batch of n frames, or nullptr.  measure: the records are written, so there must be some.
inline const char *hl_check(const mcraw_highlights &h, size_t n, bool measure)
{
    if (h.mode != MCRAW_HL_CLIP && h.mode != MCRAW_HL_REBUILD)
        return "unknown mode";
    if (h.cfa > 3u)
        return "unknown cfa";
    if (h.flags & ~MCRAW_HL_ACCUMULATE)
        return "unknown flag";
    if (h.top < 1u || h.top > 65535u)
        return "top must be 1 .. 65535";
    for (int p = 0; p < 4; p++) {
        if (h.gain[p] < 256u)
            return "gain must be 256 .. 65535 (Q4.12)";
        if (h.sat[p] <= h.black[p])
            return "sat must be above black";
    }
    if (measure ? (h.nrec != 1u && h.nrec != n) : (h.nrec != 0u && h.nrec != 1u && h.nrec != n))
        return measure ? "nrec must be 1 or n" : "nrec must be 0, 1 or n";
    if ((h.nrec > 0u) != (h.rec != nullptr))
        return "rec goes with nrec: NULL with 0, memory with 1 or n";
    if (reinterpret_cast<uintptr_t>(h.rec) & 7u)
        return "rec not 8-byte aligned";
    if (h.reserved != 0u)
        return "reserved must be 0";
    return nullptr;
}

// Why the batches cannot be used, or nullptr: MosaicBatch's checks, and no size of 1 (the reflection -1 -> 1 needs two).
inline const char *hl_check_batches(const MosaicBatch &in, const MosaicBatch *out)
{
    if (in.W < 2 || in.H < 2 || in.W > 65536 || in.H > 65536)
        return "width and height must be 2 .. 65536";
    return out ? check(in, *out) : in.check();
}

// Do the records share a byte with the batch?
inline bool hl_rec_overlaps(const mcraw_highlights &h, const MosaicBatch &b)
{
    return h.nrec > 0u && ranges_overlap(reinterpret_cast<uintptr_t>(h.rec), static_cast<size_t>(h.nrec) * HL_REC_BYTES, b.base, b.bytes());
}

} // namespace mcraw
