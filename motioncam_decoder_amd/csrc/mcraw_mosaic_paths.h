// mcraw_mosaic_paths.h -- the path census of the mosaic stages kshade (csrc/mcraw_shade.hip), kstats (csrc/mcraw_stats.hip),
// kfixpix and kfixpix_list (csrc/mcraw_fixpix.hip), kdenoise<1|2> (csrc/mcraw_denoise.hip), kmerge<0|1> with global positions
// and with a cell field (csrc/mcraw_merge.hip) and khl_apply, khl_measure, khl_clip (csrc/mcraw_highlights.hip),
// for test builds only (tests/test_gpu_mosaic_paths.py, build.MOSAIC_PATH_VARIANTS).  A source that wants the census includes this
// header IN FRONT of mcraw_mosaic.h, under a -D switch that only the stage sources mention: the hooks of mcraw_mosaic.h (MOS_PATH,
// MOS_WAVE, MOS_STAGE, MOS_DIV) are empty unless defined, as RGB_PATH is in mcraw_rgb_dev.h, and this header names no switch, so a
// variant compiles the stage sources alone.  Including it is joining the family: mcraw_diag_mosaic_paths (mcraw_shade.hip) adds
// up the sources that did (mcraw_census.h, which also has the ways to count).
//
// Every counter but the two correction steps of div_round is fixed by geometry, by the alignment of the caller's buffers, by the
// parameters and by the samples: tests/_mosaic_paths_model.py predicts each one exactly.
//
// The builds (build.MOSAIC_PATH_VARIANTS; the -D names are spelled out there and in the sources), and why each is valid for every
// input:
//   census      the counters alone.  They add atomics on memory that no kernel reads: no output can depend on them.
//   slow        kfixpix's `cand` and khl_apply's `clipped` are true for every lane.  Both predicates only decide whether a lane enters
//               the general statement, in which every pixel is tested on its own (against Hk / Lk and the thresholds; against sat - 1)
//               and guarded by its place against n: a lane that enters it for nothing stores what it loaded.  kstats never takes
//               stats_tile<BL, true>, and so never its one-bin shortcut: stats_tile<BL, false> is the same statement with every
//               sample tested against the lane's mask, and a mask of all ones passes every one.
//               kmerge stages a member that weighs 0 for every pixel of the tile instead of passing it over: mg_stage writes 0
//               for what lies outside the moved frame, and every weight is guarded by rowv / colv / cenv, the pixel's place in
//               the valid region, which is empty inside such a tile: the member adds 0 to num and den.
//   poison      every LDS tile buffer (s_t of kfixpix, kdenoise, khl_apply, khl_measure; s_b of kmerge, and s_m again in front of
//               every member) is filled with 0xFFFF samples, and a barrier follows, in front of staging.  Staging writes every
//               chunk that an output of the frame reads (mg_stage writes every chunk there is), so only the chunks "that no
//               output reads" keep the poison.  0xFFFF is above any sat - 1, Hk or Lk: the value most likely to send a lane into
//               a slow path or to leak into a sum.
//   poisonslow  both.
//   pieces      kmerge launches 3 outputs at a time instead of up to 65535: A.first, A.out, A.nout and A.per are set per launch,
//               a window reaches into frames whose outputs other launches make (the input is never written), and 3 * tiles stays
//               below the 2^30 workgroups that the product's own bound keeps (a static_assert holds 1 .. 2048 against the 2^19
//               tiles of the largest frame).  kstats takes at most 2 tiles per workgroup instead of 8192: the bound only caps
//               how much a lane's 32-bit sums collect (8192 * 4 * 65535 < 2^32: fewer tiles collect less, the static_assert
//               allows 1 .. 8192); the host's floor of B / 64 tiles per workgroup is a cost heuristic that the cap may undercut:
//               every tile is still taken once, by grid = ceil(tiles / tpc) workgroups.
//   frames2     (build.MOSAIC_FRAMES2_FLAGS) the launch loops of kshade, kstats, kfixpix (+ kfixpix_list), kdenoise, khl_apply, khl_clip and khl_measure take 2
//               frames per launch instead of up to 65535 (LAUNCH_PIECE of mcraw_host.h): launches of 2 + 1 for the corpus' 3
//               frames.  The loops are written for any piece >= 1: every launch gets its first frame's input, output, record,
//               counts, table and map; kstats makes tiles per workgroup from the launch's frame count.
//   th16        the tile heights of 16 rows that kfixpix, kdenoise and kmerge already support
//               (their static_asserts allow 16 and 32; the
//               benchmarks build them): another split of the same rows into workgroups, lanes and passes.
#pragma once
#include "mcraw_census.h"

namespace mcraw {

enum MosPath {
    // walk: workgroups launched; lanes that have no column of the frame (n == 0), per thread; lanes that leave their rows at a row
    // past H (`break`: once per lane); lane rows past H that are passed over (`continue`: once per row)
    MP_WG, MP_IDLE_LANE, MP_ROW_BREAK, MP_ROW_CONT,
    // staging, per 16-byte chunk of the LDS tile: a full piece of a row as an aligned vector load / as one unaligned access; element
    // loads through the reflection for a halo chunk (the first and the last of an LDS row) / for a cropped row end; skipped as
    // "no output of the frame reads it"
    MP_STG_VEC, MP_STG_UNAL, MP_STG_HALO, MP_STG_CROP, MP_STG_SKIP,
    // direct loads (load8), per lane row: aligned vector / unaligned / elements
    MP_LD_VEC, MP_LD_UNAL, MP_LD_ELEM,
    // stores (store8), per lane row: aligned (streaming or plain) / one unaligned 16-byte store / cropped elements
    MP_ST_VEC, MP_ST_UNAL, MP_ST_ELEM,
    // kfixpix: waves (per pair of lane rows) with / without __any(cand); lane rows with cand; pixels hot / cold; flagged pixels
    // that the search finds in the list (looked for only with a counts record and a list); dwords with a flagged half
    MP_FP_WAVE_ANY, MP_FP_WAVE_NONE, MP_FP_CAND, MP_FP_HOT, MP_FP_COLD, MP_FP_LISTED, MP_FP_FLAG,
    // kfixpix_list: workgroups; threads past the list's end; entries outside the frame; entries written; entries without an
    // eligible pair
    MP_FL_WG, MP_FL_PAST, MP_FL_OUTSIDE, MP_FL_WRITTEN, MP_FL_NOPAIR,
    // kdenoise<2>: lanes with edgex; lane rows with sy & 1 / sy & 2 / both; dwords of a lane with `both` (W in {5, 6, 7})
    MP_DN_EDGEX, MP_DN_SY1, MP_DN_SY2, MP_DN_SY3, MP_DN_BOTH,
    // khl_apply: lane rows with / without clipped; pixels rebuilt / left as cand <= v / of the rebuilt ones limited by top
    MP_HL_CLIPPED, MP_HL_UNCLIPPED, MP_HL_REBUILT, MP_HL_LEFT, MP_HL_TOP,
    // khl_measure: pixels measured / rejected by their own level / rejected by a neighbour
    MP_HM_MEASURED, MP_HM_OWN, MP_HM_NEIGHBOUR,
    // kstats, per wave and tile: all samples inside the window (stats_tile<BL, true>) / some / none; the one-bin shortcut taken,
    // per wave, tile and CFA position; tiles prefetched (t + 1 < t1), per workgroup; lane rows loaded as elements at the
    // window's left or right edge; lane rows outside the window (no column of it, or a row above or below it)
    MP_SS_FULL, MP_SS_PARTIAL, MP_SS_EMPTY, MP_SS_ONEBIN, MP_SS_PREFETCH, MP_SS_LD_EDGE, MP_SS_ROW_OUT,
    // kmerge (plain and cell field): workgroups that return at once (the last XCD's short run); launches (pieces); mg_stage's
    // chunks staged as 0 because they lie outside the (moved) frame / of the inner chunks loaded as elements (MP_STG_CROP) those
    // that the frame's left edge cuts (a shift only); per workgroup the window's entries passed over as t == b /
    // skipped as "weighs 0 for the tile" / staged, and the staged ones by the form of their full pieces: aligned / unaligned
    // because of sx & 7 / unaligned because the input is off the 16-byte grid
    MP_MG_SHORT, MP_MG_LAUNCH, MP_MG_ZERO, MP_MG_CUT, MP_MG_SELF, MP_MG_ZEROW, MP_MG_STAGED, MP_MG_M_ALIGNED, MP_MG_M_SX, MP_MG_M_INVEC,
    // div_round: calls; corrections q - 1 (r < 0) and q + 1 (r >= den)
    MP_DIV_CALLS, MP_DIV_DOWN, MP_DIV_UP,
    MP_N
};

// (div_round's three are kept in MOS_STRIPES copies, by workgroup: the sweep of mcraw_denoise.hip calls it 2 * 10^9 times)
constexpr uint32_t MOS_STRIPES = 64u;
static __device__ unsigned long long g_mos_paths[MP_N + 3u * (MOS_STRIPES - 1u)];

// the active lanes for which `cond` holds (all active lanes of the wave call this together)
__device__ __forceinline__ void mos_path(uint32_t slot, bool cond) { census_count(&g_mos_paths[slot], cond); }

// one for the wave when `cond` (uniform over the active lanes) holds
__device__ __forceinline__ void mos_wave(uint32_t slot, bool cond) { census_wave(&g_mos_paths[slot], cond); }

// a staged chunk: `inner`: not the first or last chunk of the LDS row; `whole`: all 8 columns inside the row
__device__ __forceinline__ void mos_stage(bool inner, bool whole, bool vec)
{
    mos_path(MP_STG_VEC, inner && whole && vec);
    mos_path(MP_STG_UNAL, inner && whole && !vec);
    mos_path(MP_STG_HALO, !inner);
    mos_path(MP_STG_CROP, inner && !whole);
}

__device__ __forceinline__ void mos_div(int32_t r, uint32_t den)
{
    const uint32_t s = blockIdx.x & (MOS_STRIPES - 1u);
    const uint32_t base = s ? MP_N + 3u * (s - 1u) : MP_DIV_CALLS; // calls, down, up
    mos_path(base, true);
    mos_path(base + 1u, r < 0);
    mos_path(base + 2u, r >= static_cast<int32_t>(den));
}

// (div_round's stripes into MP_DIV_CALLS, MP_DIV_DOWN and MP_DIV_UP)
static void mos_fold_stripes(uint64_t *h)
{
    for (uint32_t s = 1; s < MOS_STRIPES; s++)
        for (uint32_t i = 0; i < 3u; i++)
            h[MP_DIV_CALLS + i] += h[MP_N + 3u * (s - 1u) + i];
}

// This source's counters added to out[0 .. n); `reset`: and start them over.  Defined, and joined, once per source (internal).
static void mos_paths_read(uint64_t *out, int n, int reset) { census_read<MP_N>(g_mos_paths, out, n, reset, true, mos_fold_stripes); }
static CensusJoin<MosPath> mos_paths_join(mos_paths_read);

} // namespace mcraw

#define MOS_PATH(slot, cond) ::mcraw::mos_path(::mcraw::slot, (cond))
#define MOS_WAVE(slot, cond) ::mcraw::mos_wave(::mcraw::slot, (cond))
#define MOS_STAGE(inner, whole, vec) ::mcraw::mos_stage((inner), (whole), (vec))
#define MOS_DIV(r, den) ::mcraw::mos_div((r), (den))
