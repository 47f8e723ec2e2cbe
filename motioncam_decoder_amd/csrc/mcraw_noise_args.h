// mcraw_noise_args.h -- the host side of mcraw_noise_batch (include/mcraw_hip.h): the checks on the struct, the record's layout and
// its two bin formulas, and the launch plan: how a window's blocks are cut into strips, the strips dealt to workgroups and a
// strip's blocks to lanes.  The kernel (mcraw_noise.hip) takes the bins, the indices and the lane mapping from here, so what
// tests/cpp/noise_args_check.cpp drives on any machine is what the GPU runs.  No HIP in here but the two function attributes.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/mcraw_hip.h"
#include "mcraw_mosaic_args.h"

#ifndef MCRAW_HD
#if defined(__HIPCC__)
#define MCRAW_HD __host__ __device__
#else
#define MCRAW_HD
#endif
#endif

namespace mcraw {

constexpr uint32_t NS_BLK = 16u;                  // a block is 16 x 16 samples: an 8 x 8 plane of each CFA position
constexpr uint32_t NS_L = 32u, NS_V = 128u;       // level bins, energy bins
constexpr uint32_t NS_HIST = 4u * NS_L * NS_V;    // counters of hist[4][32][128]
constexpr uint32_t NS_RECWORDS = NS_HIST + 8u;    // ... then nblk[4], nrej[4]
constexpr size_t NS_REC_BYTES = 4u * NS_RECWORDS; // 65 568
constexpr int NS_T = 256;                         // threads per workgroup
constexpr uint32_t NS_SB = 64u;                   // blocks across a strip: 16 rows x 1024 columns
constexpr uint32_t NS_SL = 2u * NS_SB;            // lanes of a strip: one per (block, row parity)
constexpr uint32_t NS_HALVES = NS_T / NS_SL;      // strips a workgroup has under way at a time
constexpr uint32_t NS_WGS = 1024u;                // workgroups a launch aims at (two rounds of 2 per CU)
constexpr uint32_t NS_MINSTRIPS = 16u;            // a workgroup clears and flushes 64 KiB of LDS: at least 512 KiB of samples for it

// The energy bin of T: 0 below 16, then quarter octaves whose lower edges are 2^e * (1 + f / 4), the last one open.
MCRAW_HD inline uint32_t noise_energy_bin(uint64_t T)
{
    if (T < 16u)
        return 0u;
    const uint32_t e = 63u - static_cast<uint32_t>(__builtin_clzll(T)); // floor(log2 T) >= 4: T < 2^43 in the kernel, any uint64 here
    const uint32_t f = static_cast<uint32_t>(T >> (e - 2u)) & 3u, vb = 4u * (e - 4u) + f + 1u;
    return vb < NS_V - 1u ? vb : NS_V - 1u;
}

// The level bin of a plane whose 64 samples sum to s (< 2^22): its mean, shifted.
MCRAW_HD inline uint32_t noise_level_bin(uint32_t s, uint32_t shift)
{
    const uint32_t l = (s >> 6) >> shift;
    return l < NS_L - 1u ? l : NS_L - 1u;
}

// The counter of (position, level bin, energy bin) in a record and in the workgroup's LDS copy of it.
MCRAW_HD inline uint32_t noise_hist_index(uint32_t p, uint32_t l, uint32_t vb)
{
    return (p * NS_L + l) * NS_V + vb;
}

// Why the struct cannot be used on frames of W x H (which MosaicBatch::check() has passed), or nullptr.
inline const char *noise_check(const mcraw_noise &s, int W, int H)
{
    const uint32_t w = static_cast<uint32_t>(W), h = static_cast<uint32_t>(H);
    if (s.shift > 15u)
        return "shift must be 0 .. 15";
    if ((s.x0 | s.y0) & 1u)
        return "x0 and y0 must be even";
    if (s.w < NS_BLK || s.h < NS_BLK)
        return "w and h must be at least 16";
    if (s.x0 >= w || s.w > w - s.x0 || s.y0 >= h || s.h > h - s.y0)
        return "the window leaves the frame";
    if (s.flags & ~MCRAW_NOISE_ACCUMULATE)
        return "unknown flag";
    if (s.reserved != 0u)
        return "reserved must be 0";
    return nullptr;
}

// A window of w x h in whole blocks, in strips of 16 rows x at most NS_SB blocks (numbered row by row), and the strips in runs
// of spw consecutive ones, a run per workgroup.
struct NoisePlan {
    uint32_t bx, by;     // whole blocks across and down
    uint32_t stripsX;    // strips across
    uint32_t strips;     // in all
    uint32_t spw;        // strips per workgroup
    uint32_t wgs;        // workgroups per frame
};

// frames: those of the launch; maxstrips: the build's limit of strips per workgroup (at least 1).
inline NoisePlan noise_plan(uint32_t w, uint32_t h, uint32_t frames, uint32_t maxstrips)
{
    NoisePlan P{};
    P.bx = w / NS_BLK, P.by = h / NS_BLK;
    P.stripsX = (P.bx + NS_SB - 1u) / NS_SB;
    P.strips = P.stripsX * P.by; // at most 64 * 4096
    const uint32_t want = NS_WGS / frames > 1u ? NS_WGS / frames : 1u;
    uint32_t spw = (P.strips + want - 1u) / want;
    spw = spw > NS_MINSTRIPS ? spw : NS_MINSTRIPS;
    spw = spw < maxstrips ? spw : maxstrips;
    spw = spw < P.strips ? spw : P.strips;
    P.spw = spw > 1u ? spw : 1u;
    P.wgs = (P.strips + P.spw - 1u) / P.spw;
    return P;
}

// What lane `lane` (0 .. NS_SL - 1) of the half-workgroup that has strip `strip` reads: the rows y + 2r, r = 0 .. 7, columns
// x .. x + 15 relative to the window's origin -- the planes of positions 2 * rp and 2 * rp + 1 of one block.  A wave has one
// row parity, so the position's thresholds are uniform in it.
struct NoiseLane {
    bool active; // the strip has such a block
    uint32_t x, y, rp;
};

MCRAW_HD inline NoiseLane noise_lane(uint32_t bx, uint32_t stripsX, uint32_t strip, uint32_t lane)
{
    const uint32_t sy = strip / stripsX, sx = strip - sy * stripsX;
    const uint32_t blk = sx * NS_SB + (lane & (NS_SB - 1u)), rp = lane / NS_SB;
    return NoiseLane{blk < bx, blk * NS_BLK, sy * NS_BLK + rp, rp};
}

// The strip that half `half` (0 .. NS_HALVES - 1) of workgroup `wg` works on in its round `i`; >= the run's end: none.
MCRAW_HD inline uint32_t noise_strip(uint32_t wg, uint32_t spw, uint32_t i, uint32_t half)
{
    return wg * spw + i * NS_HALVES + half;
}

} // namespace mcraw
