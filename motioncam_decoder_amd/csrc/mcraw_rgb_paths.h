// mcraw_rgb_paths.h -- the path census of the demosaic kernels (krgb_mhc, krgb_bin2, krgb_bin2y: csrc/mcraw_rgb.hip; krgb_area:
// csrc/mcraw_area.hip; krgb_resample: csrc/mcraw_resample.hip; krgb_warp: csrc/mcraw_warp.hip; krgb_mesh: csrc/mcraw_mesh.hip;
// krgb_ha: csrc/mcraw_ha.hip), for test builds only (tests/test_gpu_rgb_paths.py, test_gpu_warp_paths.py, test_gpu_mesh_paths.py,
// test_gpu_ha_paths.py, build.RGB_PATH_VARIANTS).  A source that wants the census includes this header IN FRONT of mcraw_rgb_dev.h and mcraw_rgb_launch.h,
// under a -D switch of its own: the hooks of those headers (RGB_PATH, RGB_PATH_YUV, RGB_WALK, RGB_WALK_DECL) are empty unless
// defined, as MCRAW_STORE_PATH is in mcraw_dev.h (mcraw_warp_dev.h's WARP_PATH and WARP_UNIT likewise: a source of the two gather kernels
// defines RGB_GATHER_FAMILY, 0 krgb_warp or 1 krgb_mesh, in front of this header), and this header names no switch, so a variant
// compiles the six sources alone.
// Including it is joining the family: mcraw_diag_rgb_paths (mcraw_rgb.hip) adds up the sources that did (mcraw_census.h).
//
// Every counter is fixed by geometry, by the alignment of the caller's buffers and by the grid size: tests/_rgb_paths_model.py
// predicts each one exactly (the gather kernels' and krgb_ha's: tests/_gather_paths_model.py; krgb_ha's choices follow the content too).
#pragma once
#include "mcraw_census.h"

namespace mcraw {

enum RgbFamily { RF_MHC, RF_BIN2, RF_BIN2Y, RF_AREA, RF_RES, RF_WARP, RF_MESH, RF_HA, RF_N };

enum RgbPath {
    // per family (RP_WALK + 4 * family + ..): workgroups launched; units taken as a workgroup's first / as a later one; later units
    // whose frame differs from the workgroup's previous unit
    RP_WALK,
    RP_WG = 0, RP_FIRST, RP_LATER, RP_CROSS,
    RP_WALK_END = RP_WALK + 4 * RF_N,
    // units with the LUT in LDS / read from global memory (the kinds with a LUT)
    RP_LUT_LDS = RP_WALK_END, RP_LUT_GLOBAL,
    // idle work: MHC lanes past W; MHC lanes that leave a tile's passes at a row pair past H; BIN2 / bin2y items past Ho; area
    // lanes with !row_on, per group and row; resample phase-C lanes outside the tile
    RP_IDLE_MHC_LANE, RP_IDLE_MHC_ROWS, RP_IDLE_BIN2, RP_IDLE_AREA, RP_IDLE_RES,
    // loads: 16-byte staging pieces of MHC and resample, as one vector load / as 8 reflected elements; BIN2 and bin2y item rows
    // (bin2y: two per item) as vectors / as elements
    RP_LD_MHC_VEC, RP_LD_MHC_ELEM, RP_LD_RES_VEC, RP_LD_RES_ELEM, RP_LD_BIN2_VEC, RP_LD_BIN2_ELEM, RP_LD_BIN2Y_VEC, RP_LD_BIN2Y_ELEM,
    // krgb_area's pieces of 4 quads: two 16-byte loads / dwords / uint16 pairs; the dword and uint16 pieces with a zero-filled tail
    // (aq + 3 >= QW); pieces skipped by s >= nt
    RP_LD_AREA_M2, RP_LD_AREA_M1, RP_LD_AREA_M0, RP_LD_AREA_TAIL, RP_LD_AREA_SKIP,
    // stores, per 8-sample row piece and plane: whole on the grid / the cropped row end (n < 8) / whole off the grid
    RP_ST_F_FAST, RP_ST_F_CROP, RP_ST_F_OFF,          // the float kinds
    RP_ST_C8_FAST, RP_ST_C8_CROP, RP_ST_C8_OFF,       // display CHW uint8
    RP_ST_C16_FAST, RP_ST_C16_CROP, RP_ST_C16_OFF,    // display CHW uint16
    RP_ST_H8_16_8, RP_ST_H8_8_16, RP_ST_H8_ELEM,      // display HWC uint8 (per piece): 16 + 8 bytes / 8 + 16 / elements
    RP_ST_H16_FAST, RP_ST_H16_ELEM,                   // display HWC uint16 (per piece): 3 x 16 bytes / elements
    RP_ST_YL_FAST, RP_ST_YL_CROP, RP_ST_YL_OFF,       // YUV luma rows
    RP_ST_YC_FAST, RP_ST_YC_CROP, RP_ST_YC_OFF,       // YUV chroma rows
    // krgb_warp and krgb_mesh (RP_GATHER + RPG_N * (0 warp, 1 mesh) + ..): 16-byte staging pieces as one vector load / as 8 reflected
    // elements; phase-A items of even / odd rows; gather lanes with / without pixels; units whose window min() cut in rows / in
    // columns; pixels whose tap origin a clamp moved: row low, row high, column low, column high; the idle lanes of warp_store:
    // lyid past the tile's rows / else xo past Wo / else j0 past the tile's last row
    RP_GATHER,
    RPG_LD_VEC = 0, RPG_LD_ELEM, RPG_A_EVEN, RPG_A_ODD, RPG_PIX, RPG_NOPIX, RPG_CUT_ROWS, RPG_CUT_COLS,
    RPG_TAP_ROW_LO, RPG_TAP_ROW_HI, RPG_TAP_COL_LO, RPG_TAP_COL_HI, RPG_ST_IDLE_LY, RPG_ST_IDLE_X, RPG_ST_IDLE_ROW, RPG_N,
    RP_GATHER_END = RP_GATHER + 2 * RPG_N,
    // krgb_mesh: units whose cell is narrow in both axes (32-bit sums) / is not (mesh_lerp64); positions that the frame clamp moved:
    // Y to 0, Y to the last row, X to 0, X to the last column
    RP_MESH_NARROW = RP_GATHER_END, RP_MESH_WIDE, RP_MESH_Y_LO, RP_MESH_Y_HI, RP_MESH_X_LO, RP_MESH_X_HI,
    // krgb_ha: staging pieces as a vector / as elements; lanes that `continue` at x >= W; lane passes that `break` at y >= H; the
    // outcomes of ha_pick (Da < Db, Db < Da, equal) per call site: the main green items (every site computed), the ring's edge
    // items, the diagonal choice of the estimates (columns below n)
    RP_HA_LD_VEC, RP_HA_LD_ELEM, RP_HA_CONTINUE, RP_HA_BREAK,
    RP_HA_PICK,
    RP_HA_MAIN_A = RP_HA_PICK, RP_HA_MAIN_B, RP_HA_MAIN_EQ, RP_HA_EDGE_A, RP_HA_EDGE_B, RP_HA_EDGE_EQ, RP_HA_DIAG_A, RP_HA_DIAG_B, RP_HA_DIAG_EQ,
    RP_N
};

static __device__ unsigned long long g_rgb_paths[RP_N];

// the active lanes for which `cond` holds (all active lanes of the wave call this together)
__device__ __forceinline__ void rgb_path(uint32_t slot, bool cond) { census_count(&g_rgb_paths[slot], cond); }

// one for the workgroup when `cond`, which is uniform over it, holds
__device__ __forceinline__ void rgb_path_unit(uint32_t slot, bool cond)
{
    if (cond && threadIdx.x == 0u)
        atomicAdd(&g_rgb_paths[slot], 1ull);
}

// a call of ha_pick(.., Da, .., Db) at call site `site` (0 main, 1 edge, 2 diagonal) by the active lanes for which `on` holds
__device__ __forceinline__ void rgb_path_pick(uint32_t site, int Da, int Db, bool on)
{
    rgb_path(RP_HA_PICK + 3u * site, on && Da < Db);
    rgb_path(RP_HA_PICK + 3u * site + 1u, on && Db < Da);
    rgb_path(RP_HA_PICK + 3u * site + 2u, on && Da == Db);
}

// 8 samples of a YUV row at dst: slot (whole, on the grid of 8 es bytes), slot + 1 (n < 8), slot + 2 (whole, off the grid)
__device__ __forceinline__ void rgb_path_yuv(uint32_t slot, const void *dst, uint32_t n, uint32_t es)
{
    const bool on = (reinterpret_cast<uintptr_t>(dst) & (8u * es - 1u)) == 0u;
    rgb_path(slot, n == 8u && on);
    rgb_path(slot + 1u, n != 8u);
    rgb_path(slot + 2u, n == 8u && !on);
}

// A workgroup takes a unit of frame f (every thread calls this at the top of the unit; prev: ~0 in front of the first).
__device__ __forceinline__ void rgb_walk(uint32_t family, uint32_t f, bool lut, bool lutg, uint32_t &prev)
{
    if (threadIdx.x == 0u) {
        unsigned long long *w = &g_rgb_paths[RP_WALK + 4u * family];
        if (prev == 0xffffffffu) {
            atomicAdd(&w[RP_WG], 1ull);
            atomicAdd(&w[RP_FIRST], 1ull);
        } else {
            atomicAdd(&w[RP_LATER], 1ull);
            if (prev != f)
                atomicAdd(&w[RP_CROSS], 1ull);
        }
        if (lut)
            atomicAdd(&g_rgb_paths[lutg ? RP_LUT_GLOBAL : RP_LUT_LDS], 1ull);
    }
    prev = f;
}

// This source's counters added to out[0 .. n); `reset`: and start them over.  Defined, and joined, once per source (internal).
static void rgb_paths_read(uint64_t *out, int n, int reset) { census_read<RP_N>(g_rgb_paths, out, n, reset, true); }
static CensusJoin<RgbPath> rgb_paths_join(rgb_paths_read);

} // namespace mcraw

#define RGB_PATH(slot, cond) ::mcraw::rgb_path(::mcraw::slot, (cond))
#define RGB_PATH_YUV(slot, dst, n, es) ::mcraw::rgb_path_yuv(::mcraw::slot, (dst), (n), (es))
#define WARP_PATH(slot, cond) ::mcraw::rgb_path(::mcraw::RP_GATHER + ::mcraw::RPG_N * (RGB_GATHER_FAMILY) + ::mcraw::slot, (cond))
#define WARP_UNIT(slot, cond) ::mcraw::rgb_path_unit(::mcraw::RP_GATHER + ::mcraw::RPG_N * (RGB_GATHER_FAMILY) + ::mcraw::slot, (cond))
#define RGB_PATH_UNIT(slot, cond) ::mcraw::rgb_path_unit(::mcraw::slot, (cond))
#define HA_PICKS(site, Da, Db, on) ::mcraw::rgb_path_pick((site), (Da), (Db), (on))
#define RGB_WALK_DECL uint32_t rgb_walk_prev = 0xffffffffu
#define RGB_WALK(family, f, lut, lutg) ::mcraw::rgb_walk(::mcraw::family, (f), (lut), (lutg) != 0u, rgb_walk_prev)
