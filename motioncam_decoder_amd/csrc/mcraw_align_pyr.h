// mcraw_align_pyr.h -- what the two estimators share (mcraw_align.hip: one shift per frame; mcraw_cells.hip: one per cell): the
// grey pyramid, built by mcraw_align.hip's kalign_pyr / kalign_down through align_pyramid() below -- one set of kernels, one
// statement of the rounding --, the pair of a frame, and the nine candidates of a refinement level on two staged tiles.
#pragma once
#include "mcraw_host.h"
#include "mcraw_mosaic.h"
#include "mcraw_align_args.h"

// The hooks of the path census of the estimators (mcraw_est_paths.h, test builds only): empty unless a source defined them in
// front of this header.
#ifndef EST_PATH
#define EST_PATH(slot, cond)
#endif
#ifndef EST_ADDN
#define EST_ADDN(slot, cond, n)
#endif
#ifndef EST_ONE
#define EST_ONE(slot, cond)
#endif

namespace mcraw {

constexpr int AL_T = 256;        // threads per workgroup
constexpr uint32_t AL_TW = 128u; // the SAD kernels' tile: 32 lanes across with 4 pixels each,
constexpr uint32_t AL_TH = 32u;  //   8 lanes down with 4 rows each

// The planes of a frame's pyramid in the caller's scratch: AlignPlan's and CellsPlan's rule (h(l + 1) = h(l) / 2, rows of w
// rounded up to 8 elements, the levels back to back).
struct AlPyramid {
    uint32_t levels;
    uint32_t h[AL_MAXLEVELS], w[AL_MAXLEVELS], pitch[AL_MAXLEVELS];
    size_t off[AL_MAXLEVELS]; // elements from a frame's pyramid to its level l
    size_t frame_elems;       // elements from pyramid to pyramid
};

// Queues the pyramids of the n frames of I on st: pyr[f * frame_elems + off[l] + y * pitch[l] + x] = G(l)[f][y][x] of
// include/mcraw_hip.h.  A level without pixels is left out.  (mcraw_align.hip)
int align_pyramid(hipStream_t st, const MosaicBatch &I, const uint16_t *in, int n, const uint16_t black[4], const AlPyramid &G, uint16_t *pyr);

// The pair of frame t (0 .. n - 1): its base, or -1 for the frame that has none.
__device__ __forceinline__ int al_base(int t, int ref)
{
    return ref < 0 ? t - 1 : (t == ref ? -1 : ref);
}

// The pair of columns that starts at column c + o of dwords lo = (c, c + 1), hi = (c + 2, c + 3); o: 0 or 1
__device__ __forceinline__ uint32_t al_pair(uint32_t lo, uint32_t hi, uint32_t o)
{
    return o ? __builtin_amdgcn_alignbit(hi, lo, 16u) : lo;
}

// A lane's 4 x 4 pixels against the nine candidates of a refinement level: acc[3 * (ddy + 1) + (ddx + 1)].  sb, sm: the staged
// tiles (LD dwords per row); ob, om: which half of its first dword a row's first column is; nx, ny: the lane's columns and rows
// inside the window (FULL: 4 and 4 for every lane of the wave).  A pixel outside the window is 0 on both sides.
template <bool FULL>
__device__ __forceinline__ void al_refine(const uint32_t *sb, const uint32_t *sm, uint32_t LD, uint32_t lx, uint32_t ly, uint32_t ob,
                                          uint32_t om, uint32_t nx, uint32_t ny, uint32_t acc[9])
{
    uint32_t mk[4][2], bp[4][2];
#pragma unroll
    for (uint32_t i = 0; i < 4u; i++) {
        const uint32_t rowm = i < ny ? 0xFFFFFFFFu : 0u;
        mk[i][0] = FULL ? 0xFFFFFFFFu : rowm & ((nx > 0u ? 0xFFFFu : 0u) | (nx > 1u ? 0xFFFF0000u : 0u));
        mk[i][1] = FULL ? 0xFFFFFFFFu : rowm & ((nx > 2u ? 0xFFFFu : 0u) | (nx > 3u ? 0xFFFF0000u : 0u));
        const uint32_t *q = &sb[(4u * ly + i) * LD + 2u * lx];
        const uint32_t d0 = q[0], d1 = q[1], d2 = q[2];
        bp[i][0] = al_pair(d0, d1, ob) & mk[i][0];
        bp[i][1] = al_pair(d1, d2, ob) & mk[i][1];
    }
#pragma unroll
    for (uint32_t c = 0; c < 9u; c++)
        acc[c] = 0u;
#pragma unroll
    for (uint32_t rr = 0; rr < 6u; rr++) { // the member's rows 4 ly + rr: base row i meets it as ddy = rr - i - 1
        const uint32_t *q = &sm[(4u * ly + rr) * LD + 2u * lx];
        const uint32_t d0 = q[0], d1 = q[1], d2 = q[2], d3 = q[3];
        const uint32_t e1 = __builtin_amdgcn_alignbit(d1, d0, 16u), e3 = __builtin_amdgcn_alignbit(d2, d1, 16u),
                       e5 = __builtin_amdgcn_alignbit(d3, d2, 16u);
        // f[k]: the pair that starts k columns behind the member's column for the lane's first pixel and ddx = -1
        const uint32_t f[5] = {om ? e1 : d0, om ? d1 : e1, om ? e3 : d1, om ? d2 : e3, om ? e5 : d2};
#pragma unroll
        for (uint32_t i = 0; i < 4u; i++) {
            if (rr < i || rr > i + 2u)
                continue;
            const uint32_t ddy = rr - i; // + 1 already: 0 .. 2
#pragma unroll
            for (uint32_t ddx = 0; ddx < 3u; ddx++) { // + 1 already
                acc[3u * ddy + ddx] = __builtin_amdgcn_sad_u16(f[ddx] & mk[i][0], bp[i][0], acc[3u * ddy + ddx]);
                acc[3u * ddy + ddx] = __builtin_amdgcn_sad_u16(f[ddx + 2u] & mk[i][1], bp[i][1], acc[3u * ddy + ddx]);
            }
        }
    }
}

} // namespace mcraw
