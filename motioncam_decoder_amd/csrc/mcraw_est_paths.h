// mcraw_est_paths.h -- the path census of the estimators: kalign_pyr, kalign_down, kalign_zero, kalign_sad<0|1>, kalign_pick,
// kalign_final (csrc/mcraw_align.hip), kcells_zero, kcells_sad<0|1>, kcells_pick, kcells_final (csrc/mcraw_cells.hip) and knoise
// (csrc/mcraw_noise.hip), for test builds only (tests/test_gpu_est_paths.py, build.EST_PATH_VARIANTS).  A source that wants the
// census includes this header IN FRONT of its other headers, under a -D switch that only those three sources mention: the hooks
// (EST_PATH, EST_ADDN, EST_ONE of mcraw_align_pyr.h and mcraw_noise.hip; MOS_PATH of mcraw_mosaic.h, through which load8 counts its
// three forms) are empty unless defined, and this header names no switch, so a variant compiles the three sources alone.
// Including it is joining the family: mcraw_diag_est_paths (mcraw_align.hip) adds up the sources that did (mcraw_census.h, which
// also has the ways to count; EST_ADDN, rows a lane leaves: an atomic per lane).
//
// Every counter is fixed by geometry, by the alignment of the caller's buffers, by the parameters and by the
// samples -- none depends on LDS that nobody staged, every such read is masked --: tests/_est_paths_model.py predicts each exactly.
//
// The builds (build.EST_PATH_VARIANTS; the -D names are spelled out there and in the sources), and why each is valid for every
// input:
//   census      the counters alone.  They add atomics on memory that no kernel reads: no output can depend on them.
//   frames2     the launch loops of the three sources take 2 frames per launch instead of up to 65535 (LAUNCH_PIECE of
//               mcraw_host.h).  The loops are written for any piece >= 1: every launch gets its first frame's input, pyramid,
//               record and number; a frame's pair may lie in an earlier launch, whose pyramids and winners are complete by stream
//               order, and a level's launches all precede its kalign_pick (kcells_pick runs per launch, on that launch's frames).
//               knoise makes its plan per launch from the launch's frame count: another split of the same strips into workgroups.
//   slow        every wave of kalign_sad<1> and kcells_sad<1> takes al_refine<false>: al_refine<true> is the same statement with
//               every mask all ones, and that is what <false> computes for a lane with nx == ny == 4.  kcells_sad always adds with
//               atomics and kcells_zero always runs: a store of s_acc[i] is an add of it onto the zero that kcells_zero wrote.
//   poison      s_m and s_b of the four SAD kernels are filled with 0xFFFF samples, and a barrier follows, in front of staging.
//               Staging writes every dword that an unmasked pixel reads (al_stage: the whole tile and margin; cl_stage: the
//               piece's pixels and margin), so only masked reads see the poison.  0xFFFF gives the largest differences: the
//               value most likely to leak into a sum.
//   poisonslow  both.
//   strips1     knoise with at most one strip per workgroup (the static_assert allows any limit >= 1): as many workgroups as
//               strips flush into a frame's record, and half of every workgroup idles.
#pragma once
#include "mcraw_census.h"

namespace mcraw {

// The counters of one SAD kernel; kalign_sad<RT> has them at EP_AS + RT * SK_N, kcells_sad<RT> at EP_CS + RT * SK_N.
enum EstSad {
    // launches; workgroups; workgroups that return as b < 0; workgroups (with pixels) by (ob, om): 00, 01, 10, 11
    SK_LAUNCH, SK_WG, SK_NOPAIR, SK_OM0, SK_OM1, SK_OB1OM0, SK_OB1OM1,
    // staged dwords: one aligned load; al_stage: 0 as yy >= h, 0 as col >= pitch (and yy < h), loaded ones that hold a column
    // >= w; cl_stage: clamped elements at the left (col < 0), at the right (col + 1 >= w); staged rows clamped above, below
    SK_STG_LOAD, SK_STG_ZERO_Y, SK_STG_ZERO_COL, SK_STG_PAD, SK_STG_LEFT, SK_STG_RIGHT, SK_ROW_ABOVE, SK_ROW_BELOW,
    // waves in al_refine<true> / <false>; lanes without a pixel (nx == 0 or ny == 0); lanes that read LDS nobody staged (cells)
    SK_REF_FULL, SK_REF_MASK, SK_LANE_EMPTY, SK_UNSTAGED,
    // a wave's candidate sums added to s_acc / passed over as 0; the workgroup's: one 64-bit atomic / passed over as 0 / stored
    // (cells of one piece); workgroups whose piece has no pixels (cells)
    SK_WAVE_ADD, SK_WAVE_SKIP, SK_GLOB_ADD, SK_GLOB_SKIP, SK_STORE, SK_EMPTY,
    SK_N
};

enum EstPath {
    // load8 (the MOS_PATH hooks of mcraw_mosaic.h) of kalign_pyr: vector / unaligned / elements, then store8's three (never called)
    EP_PY_LD, EP_PY_LD_END = EP_PY_LD + 5,
    // kalign_pyr: workgroups; lanes that return (x >= W or y >= H); lane rows zero-filled (y + r >= H)
    EP_PY_WG, EP_PY_RET, EP_PY_ZERO_ROW,
    // G0 rows as an 8-byte vector / as elements / left by `break`; G1 rows as a dword / as one element / not stored (gx >= w1) /
    // left by `break`; G2 stored / not; lanes that return at levels < 2 / levels < 3
    EP_PY_G0_VEC, EP_PY_G0_ELEM, EP_PY_G0_LEFT, EP_PY_G1_DWORD, EP_PY_G1_ELEM, EP_PY_G1_NONE, EP_PY_G1_LEFT, EP_PY_G2_STORE, EP_PY_G2_NONE,
    EP_PY_RET_L2, EP_PY_RET_L3,
    // kalign_down: launches; threads past dh * dw.  kalign_zero, kcells_zero: launches
    EP_DN_LAUNCH, EP_DN_PAST, EP_AZ_LAUNCH, EP_CZ_LAUNCH,
    EP_AS, EP_AS_END = EP_AS + 2 * SK_N - 1,
    EP_CS, EP_CS_END = EP_CS + 2 * SK_N - 1,
    // kalign_pick: threads without a pair (t >= n or no base).  kalign_final: pieces of 256 in the chain scan; components clamped
    EP_AP_NOPAIR, EP_AF_PIECE, EP_AF_CLAMP,
    // kcells_pick: threads past `cells` or without a pair.  kcells_final: threads past `cells`; (cell, frame) without a pair;
    // components clamped
    EP_CP_NOPAIR, EP_CF_PAST, EP_CF_NOPAIR, EP_CF_CLAMP,
    // load8 of knoise
    EP_NS_LD, EP_NS_LD_END = EP_NS_LD + 5,
    // knoise: workgroups; lanes of an (iteration, half) passed over as t >= t1 / as !L.active; blocks read (a lane each: two
    // planes); planes rejected by sat / by lo but not sat / accepted; non-zero histogram counters flushed; register counters flushed
    EP_NS_WG, EP_NS_SKIP_T1, EP_NS_SKIP_INACTIVE, EP_NS_BLOCK, EP_NS_REJ_SAT, EP_NS_REJ_LO, EP_NS_ACCEPT, EP_NS_HIST_FLUSH, EP_NS_REG_FLUSH,
    EP_N
};

// what the MOS_PATH hooks of mcraw_mosaic.h name: offsets from the source's EST_LD_BASE.  Only load8 is called by these sources;
// store8 and the tile staging (MP_STG_SKIP) are not, and their counters stay 0.
enum EstLd { MP_LD_VEC, MP_LD_UNAL, MP_LD_ELEM, MP_ST_VEC, MP_ST_UNAL, MP_ST_ELEM, MP_STG_SKIP = MP_ST_ELEM };

static __device__ unsigned long long g_est_paths[EP_N];

// the active lanes for which `cond` holds (all active lanes of the wave call this together)
__device__ __forceinline__ void est_add(uint32_t index, bool cond) { census_count(&g_est_paths[index], cond); }

// n for every lane for which `cond` holds
__device__ __forceinline__ void est_addn(uint32_t index, bool cond, uint32_t n) { census_addn(&g_est_paths[index], cond, n); }

// This source's counters added to out[0 .. n); `reset`: and start them over.  Defined, and joined, once per source (internal).
static void est_paths_read(uint64_t *out, int n, int reset) { census_read<EP_N>(g_est_paths, out, n, reset, true); }
static CensusJoin<EstPath> est_paths_join(est_paths_read);

} // namespace mcraw

#define EST_PATH(slot, cond) ::mcraw::est_add((slot), (cond))
#define EST_ADDN(slot, cond, n) ::mcraw::est_addn((slot), (cond), (n))
// one for the workgroup when `cond` (uniform over it) holds
#define EST_ONE(slot, cond) ::mcraw::est_add((slot), threadIdx.x == 0u && (cond))
#define MOS_PATH(slot, cond) ::mcraw::est_add(EST_LD_BASE + ::mcraw::slot, (cond))
