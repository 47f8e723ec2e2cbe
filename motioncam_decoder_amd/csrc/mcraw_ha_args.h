// mcraw_ha_args.h -- the tile of krgb_ha (csrc/mcraw_ha.hip; MCRAW_RGB_HA, include/mcraw_hip.h): its two LDS arrays, the items
// of its three phases and every index they make.  No HIP in here, so that tests/cpp/ha_args_check.cpp can walk every item of every
// tile of a sweep of frame sizes and hold each index against the arrays, and each read against what the phase before wrote.
// Whether a call is accepted, and its plan (MHC's output size and tiles), is rgb_check's (mcraw_rgb_args.h).
#pragma once
#include "mcraw_rgb_args.h"

namespace mcraw {

// A workgroup of RGB_T threads owns MHC's tile, MHC_TW x MHC_TH pixels at (x0, y0) of a frame.
//   s_raw  the samples of the tile and 3 rows either side, columns x0 - 8 .. x0 + MHC_TW + 7 (3 used either side: 16-byte pieces on
//          the frame's 8-column grid), reflected at the frame's edges.  Row R is frame row y0 - 3 + R, column C frame column x0 - 8 + C.
//   s_g    the green plane at the R / B sites of the tile and its ring of one, int32 in 1/8 DN, at half density: row Q is frame row
//          y0 - 1 + Q, entry K the R / B site of that row in raw columns 2 K, 2 K + 1 (a row's R / B sites have one column parity).
constexpr uint32_t HA_RAWW = MHC_TW + 16u, HA_RAWH = MHC_TH + 6u; // 272 x 38 uint16: 20 672 bytes
constexpr uint32_t HA_RAWCH = HA_RAWW / 8u;                       // 16-byte pieces per raw row
constexpr uint32_t HA_GW = HA_RAWW / 2u, HA_GH = MHC_TH + 2u;     // 136 x 34 int32: 18 496 bytes
static_assert(HA_GW % 4u == 0u, "a lane's four entries of a g row are one 16-byte piece");

MCRAW_HD constexpr uint32_t ha_raw_idx(uint32_t R, uint32_t C) { return R * HA_RAWW + C; }
MCRAW_HD constexpr uint32_t ha_g_idx(uint32_t Q, uint32_t K) { return Q * HA_GW + K; }

// Column parity (of the frame, and of the raw window: x0 - 8 is even) of the R / B sites of a frame row of parity `ypar`, for the
// CFA role shift S: role = (ypar * 2 + xpar) ^ S is 0 or 3 where both bits agree.
MCRAW_HD constexpr uint32_t ha_rb_xpar(uint32_t ypar, uint32_t S) { return (ypar ^ (S >> 1) ^ S) & 1u; }

// Phase 1, stage: item i < HA_STAGE_ITEMS is piece q of raw row R: 8 samples to ha_raw_idx(R, 8 q).
constexpr uint32_t HA_STAGE_ITEMS = HA_RAWH * HA_RAWCH;

// Phase 2, green.  A main item is a pair of g rows and a piece of 8 tile columns: g rows 2 rp, 2 rp + 1 (frame rows of parity 1, 0:
// y0 is even), tile columns 8 q .. 8 q + 7.  It reads raw rows 2 rp .. 2 rp + 5 at columns 8 q .. 8 q + 17 (8 q + 6 .. 8 q + 17
// used) and writes the four entries 4 q + 4 .. 4 q + 7 of both g rows.  The ring's columns x0 - 1 and x0 + MHC_TW are the edge
// items': item e is g row e, where one of the two is an R / B site, by the row's parity: raw column 7 (entry 3) or
// MHC_TW + 8 (entry MHC_TW / 2 + 4); it reads raw rows e .. e + 4 of that column and columns - 2 .. + 2 of raw row e + 2.
constexpr uint32_t HA_G_PAIRS = HA_GH / 2u;                 // 17
constexpr uint32_t HA_G_MAIN = HA_G_PAIRS * (MHC_TW / 8u);  // 544 items: threads 0 .. 31 take three, the others two
constexpr uint32_t HA_G_EDGE = HA_GH;                       // 34 items
constexpr uint32_t HA_G_EDGE_T0 = 64u;                      // taken by threads 64 .. 97: a wave with two main items
static_assert(HA_G_EDGE_T0 + HA_G_EDGE <= RGB_T && HA_G_MAIN - 2u * RGB_T <= HA_G_EDGE_T0, "the edge items go to a wave with two main items");

MCRAW_HD constexpr uint32_t ha_edge_rawcol(uint32_t Q, uint32_t S) // g row Q is frame row y0 - 1 + Q: parity (Q + 1) & 1
{
    return ha_rb_xpar((Q + 1u) & 1u, S) ? 7u : MHC_TW + 8u;
}

// Phase 3, estimates: lane (lx, ly) makes tile columns 8 lx .. 8 lx + 7 of the tile's row pairs ly and ly + 8 (tile rows t, t + 1,
// t = 2 (ly + 8 pass)): raw rows t + 2 .. t + 5 at columns 8 lx + 6 .. 8 lx + 17 (8 lx + 7 .. 8 lx + 16 used), and of g rows
// t .. t + 3 the entries 4 lx + 4 .. 4 lx + 7 and, by the row's parity, 4 lx + 3 or 4 lx + 8.
MCRAW_HD constexpr uint32_t ha_g_extra(uint32_t xpar, uint32_t lx) { return xpar ? 4u * lx + 3u : 4u * lx + 8u; }

} // namespace mcraw
