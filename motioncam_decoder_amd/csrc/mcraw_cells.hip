// mcraw_cells.hip -- gfx950 kernels for uint16 mosaics resident in HBM -> a field of local shifts, one per cell of every frame
// (mcraw_align_cells_batch): what mcraw_merge_cells_batch takes as its cells' `pos`.  The contract (integers only, bit-exact) is
// in include/mcraw_hip.h; DESIGN.md 28 has the design.
//
// Everything is queued on the stream; no level waits for the host.  In the caller's scratch (mcraw_cells_args.h): per frame the
// pyramid's planes, per frame, cell and level the candidates' 64-bit sums, and the cells' winners by level.
//   align_pyramid     mcraw_align.hip's kalign_pyr (mcraw_align_pyr.h): the one pass over the mosaics, levels 0 .. 2.
//   kcells_zero       empties the sums of the levels at which a cell spans several workgroups.
//   kcells_sad<R>     one launch per level, coarsest first.  A workgroup takes a piece of AL_TW x AL_TH pixels of one cell of one
//                     pair and stages the base's piece and the member's, moved by the cell's centre -- uniform over the workgroup
//                     -- and wider by the candidates' margin, in LDS, no more of either than the cell has pixels there.  A
//                     coordinate outside the plane reads the plane's nearest pixel (the contract's clamp), so the staging knows
//                     the edges and the sums do not.  R = 1 (the refinement levels): kalign_sad's nine candidates in registers
//                     (al_refine).  R = 0 (the coarsest level, up to 9 x 9 candidates): a loop over the candidates.  The wave's
//                     sums are reduced across lanes, the waves' in LDS; a cell of one piece stores its sums, a cell of several
//                     adds each with one 64-bit atomic.
//   kcells_pick       a thread per (pair, cell): the winner at the level by the contract's key.
//   kcells_final      a thread per cell: the chain's running sum over n in int32 (or the anchor form), the clamp, pos and sad.
//
// Test builds (tests/test_gpu_est_paths.py, build.EST_PATH_VARIANTS; why each is valid: the head of mcraw_est_paths.h):
//   MCRAW_PATHSA        the path census (mcraw_diag_est_paths: mcraw_align.hip)
//   MCRAW_EST_FRAMES=N  the launch loop takes N frames at a time
//   MCRAW_FORCE_SLOWA   every wave of kcells_sad<1> takes al_refine<false>; every cell adds its sums with atomics, onto kcells_zero's zeros
//   MCRAW_POISON_A      s_m and s_b of kcells_sad hold 0xFFFF samples in front of staging
#ifdef MCRAW_PATHSA
#include "mcraw_est_paths.h"
#define EST_LD_BASE ::mcraw::EP_PY_LD // (load8 is not called in here)
#endif
#ifdef MCRAW_EST_FRAMES
#define LAUNCH_PIECE MCRAW_EST_FRAMES
#endif
#include "mcraw_align_pyr.h"
#include "mcraw_cells_args.h"

namespace mcraw {

#ifdef MCRAW_FORCE_SLOWA
constexpr bool CL_SLOW = true;
#else
constexpr bool CL_SLOW = false;
#endif

struct ClSadArgs {
    const uint16_t *pyr;     // frame 0's pyramid
    unsigned long long *acc; // frame 0's sums
    const CellWin *win;      // frame 0's winners
    const int16_t *gpos;     // (n, 2) or NULL
    size_t pstride, loff;    // elements from pyramid to pyramid, from a pyramid to the level
    uint32_t pitch, h, w;    // the level's plane
    uint32_t R;              // the candidates' radius: `radius` at the coarsest level, 1 below
    uint32_t level, top;     // top: the coarsest level (the centre comes from gpos)
    uint32_t nacc, acc0;     // sums per frame and cell; the level's first
    uint32_t ch, cw;         // a cell at this level, in pixels
    uint32_t cells_x, cells; // cells across, cells per frame
    uint32_t px, pieces;     // pieces across a cell, pieces per cell
    int32_t ref, t0;         // the launch's first frame
};

// The centre of pair (b, t) at the coarsest level `top`: (gpos[t] - gpos[b]) >> 1 >> top per component, arithmetic shifts.
__device__ __forceinline__ void cl_centre(const int16_t *gpos, int t, int b, uint32_t top, int &cy, int &cx)
{
    cy = cx = 0;
    if (gpos) {
        cy = ((static_cast<int>(gpos[2 * static_cast<size_t>(t)]) - static_cast<int>(gpos[2 * static_cast<size_t>(b)])) >> 1) >> top;
        cx = ((static_cast<int>(gpos[2 * static_cast<size_t>(t) + 1u]) - static_cast<int>(gpos[2 * static_cast<size_t>(b) + 1u])) >> 1) >> top;
    }
}

// rows x ndw dwords into s (LW elements per row): dword j of row r holds the plane's pixels (ys + r, xs + 2 j) and (ys + r,
// xs + 2 j + 1), each coordinate clamped into the plane (h, w >= 1).  xs is even, so a dword inside the plane is one aligned load.
// (SLOT: the census's, test builds only)
template <uint32_t SLOT>
__device__ __forceinline__ void cl_stage(uint32_t *s, uint32_t LW, const uint16_t *plane, uint32_t pitch, int h, int w, int ys, int xs,
                                         uint32_t rows, uint32_t ndw)
{
    for (uint32_t i = threadIdx.x; i < rows * ndw; i += AL_T) {
        const uint32_t r = i / ndw, j = i - r * ndw;
        const int yy = min(max(ys + static_cast<int>(r), 0), h - 1), col = xs + 2 * static_cast<int>(j);
        EST_PATH(SLOT + SK_STG_LOAD, col >= 0 && col + 1 < w);
        EST_PATH(SLOT + SK_STG_LEFT, col < 0);
        EST_PATH(SLOT + SK_STG_RIGHT, col >= 0 && col + 1 >= w);
        EST_PATH(SLOT + SK_ROW_ABOVE, j == 0u && ys + static_cast<int>(r) < 0);
        EST_PATH(SLOT + SK_ROW_BELOW, j == 0u && ys + static_cast<int>(r) > h - 1);
        const uint16_t *row = plane + static_cast<size_t>(yy) * pitch;
        uint32_t v;
        if (col >= 0 && col + 1 < w) {
            v = *gptr<const uint32_t>(row + col);
        } else {
            const uint32_t lo = gptr<const uint16_t>(row)[min(max(col, 0), w - 1)], hi = gptr<const uint16_t>(row)[min(max(col + 1, 0), w - 1)];
            v = lo | (hi << 16);
        }
        s[r * (LW / 2u) + j] = v;
    }
}

// RT == 1: the refinement levels, nine candidates in registers.  RT == 0: A.R up to CL_MAXRADIUS, a loop over the candidates.
template <int RT>
__global__ void __launch_bounds__(AL_T) kcells_sad(const ClSadArgs A)
{
    constexpr uint32_t RMAX = RT ? 1u : CL_MAXRADIUS;
    constexpr uint32_t LW = (AL_TW + 2u * RMAX + 2u + 7u) / 8u * 8u; // elements per LDS row
    constexpr uint32_t NC = (2u * RMAX + 1u) * (2u * RMAX + 1u);
    __shared__ __attribute__((aligned(16))) uint32_t s_m[(AL_TH + 2u * RMAX) * LW / 2u];
    __shared__ __attribute__((aligned(16))) uint32_t s_b[AL_TH * LW / 2u];
    __shared__ uint32_t s_acc[NC];
    const int t = A.t0 + static_cast<int>(blockIdx.y), b = al_base(t, A.ref);
#ifdef MCRAW_PATHSA
    constexpr uint32_t SLOT = EP_CS + RT * SK_N; // this instance's counters
#else
    constexpr uint32_t SLOT = 0u;
#endif
    EST_ONE(SLOT + SK_LAUNCH, blockIdx.x == 0u && blockIdx.y == 0u);
    EST_ONE(SLOT + SK_WG, true);
    EST_ONE(SLOT + SK_NOPAIR, b < 0);
    if (b < 0) // (uniform over the workgroup)
        return;
#ifdef MCRAW_POISON_A
    for (uint32_t i = threadIdx.x; i < sizeof(s_m) / 4u; i += AL_T)
        s_m[i] = 0xFFFFFFFFu;
    for (uint32_t i = threadIdx.x; i < sizeof(s_b) / 4u; i += AL_T)
        s_b[i] = 0xFFFFFFFFu;
    __syncthreads();
#endif
    const uint32_t R = RT ? 1u : A.R, ncand = (2u * R + 1u) * (2u * R + 1u);
    const uint32_t cell = blockIdx.x / A.pieces, piece = blockIdx.x - cell * A.pieces;
    const uint32_t ci = cell / A.cells_x, cj = cell - ci * A.cells_x;
    const uint32_t py = piece / A.px, pxi = piece - py * A.px;
    // the piece's origin and the end of the cell's pixels in the plane
    const uint32_t x0 = cj * A.cw + pxi * AL_TW, y0 = ci * A.ch + py * AL_TH;
    const uint32_t x1 = min((cj + 1u) * A.cw, A.w), y1 = min((ci + 1u) * A.ch, A.h);
    const size_t slot = static_cast<size_t>(t) * A.cells + cell;
    for (uint32_t i = threadIdx.x; i < ncand; i += AL_T)
        s_acc[i] = 0u;
    EST_ONE(SLOT + SK_EMPTY, !(x0 < x1 && y0 < y1));
    if (x0 < x1 && y0 < y1) { // (uniform) the piece has pixels: the plane is not empty
        int cy, cx;
        if (A.top) {
            cl_centre(A.gpos, t, b, A.level, cy, cx);
        } else {
            const CellWin wv = A.win[slot * CL_MAXLEVELS + A.level + 1u];
            cy = 2 * wv.dy, cx = 2 * wv.dx;
        }
        const int xm = static_cast<int>(x0) + cx - static_cast<int>(R), ym = static_cast<int>(y0) + cy - static_cast<int>(R);
        const uint32_t om = static_cast<uint32_t>(xm) & 1u; // x0 is even: the base's first column is the low half of its dword
        const uint16_t *pb = A.pyr + static_cast<size_t>(b) * A.pstride + A.loff, *pm = A.pyr + static_cast<size_t>(t) * A.pstride + A.loff;
        // only what the piece's pixels read is staged: a cell at a coarse level is a fraction of a piece.  The lanes without pixels
        // read LDS that nobody wrote, and mask it.
        const uint32_t nyp = min(AL_TH, y1 - y0), nxp = min(AL_TW, x1 - x0);
        EST_ONE(SLOT + SK_OM0 + om, true);
        cl_stage<SLOT>(s_b, LW, pb, A.pitch, static_cast<int>(A.h), static_cast<int>(A.w), static_cast<int>(y0), static_cast<int>(x0), nyp,
                 (nxp + 1u) / 2u);
        cl_stage<SLOT>(s_m, LW, pm, A.pitch, static_cast<int>(A.h), static_cast<int>(A.w), ym, xm & ~1, nyp + 2u * R, (nxp + 2u * R) / 2u + 1u);
        __syncthreads();
        const uint32_t lx = threadIdx.x % 32u, ly = threadIdx.x / 32u;
        const uint32_t px = x0 + 4u * lx, py4 = y0 + 4u * ly; // the lane's 4 x 4 pixels
        const uint32_t nx = px < x1 ? min(4u, x1 - px) : 0u, ny = py4 < y1 ? min(4u, y1 - py4) : 0u;
        EST_PATH(SLOT + SK_LANE_EMPTY, nx == 0u || ny == 0u);
        // a lane's reads against what was staged: s_b rows 4 ly .. 4 ly + 3, s_m rows .. 4 ly + 3 + 2 R; al_refine reads dwords
        // 2 lx .. 2 lx + 2 of s_b and .. 2 lx + 3 of s_m, the loop the elements 4 lx .. 4 lx + 3 of s_b and .. 4 lx + 3 + 2 R + om of s_m
        EST_PATH(SLOT + SK_UNSTAGED, 4u * ly + 3u >= nyp || (RT ? 2u * lx + 2u : 2u * lx + 1u) >= (nxp + 1u) / 2u ||
                                         (RT ? 2u * lx + 3u : (4u * lx + 3u + 2u * R + om) / 2u) >= (nxp + 2u * R) / 2u + 1u);
        if (RT) {
            uint32_t acc[9];
            EST_PATH(SLOT + SK_REF_FULL, __all(nx == 4u && ny == 4u) && !CL_SLOW && __lane_id() == 0u); // (every lane takes part in __all)
            EST_PATH(SLOT + SK_REF_MASK, !(__all(nx == 4u && ny == 4u) && !CL_SLOW) && __lane_id() == 0u);
            if (!CL_SLOW && __all(nx == 4u && ny == 4u)) // the cell's interior: no masks
                al_refine<true>(s_b, s_m, LW / 2u, lx, ly, 0u, om, nx, ny, acc);
            else
                al_refine<false>(s_b, s_m, LW / 2u, lx, ly, 0u, om, nx, ny, acc);
#pragma unroll
            for (uint32_t c = 0; c < 9u; c++) {
                uint32_t v = acc[c];
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1)
                    v += __shfl_xor(v, d);
                EST_PATH(SLOT + SK_WAVE_ADD, __lane_id() == 0u && v != 0u);
                EST_PATH(SLOT + SK_WAVE_SKIP, __lane_id() == 0u && v == 0u);
                if (__lane_id() == 0u && v)
                    atomicAdd(&s_acc[c], v);
            }
        } else {
            const uint16_t *sb = reinterpret_cast<const uint16_t *>(s_b), *sm = reinterpret_cast<const uint16_t *>(s_m);
            uint32_t bv[4][4];
#pragma unroll
            for (uint32_t i = 0; i < 4u; i++)
#pragma unroll
                for (uint32_t j = 0; j < 4u; j++)
                    bv[i][j] = sb[(4u * ly + i) * LW + 4u * lx + j];
            const uint32_t side = 2u * R + 1u;
#pragma unroll 1
            for (uint32_t c = 0; c < ncand; c++) {
                const uint32_t ddy = c / side, ddx = c - ddy * side; // + R already
                uint32_t v = 0u;
#pragma unroll
                for (uint32_t i = 0; i < 4u; i++)
#pragma unroll
                    for (uint32_t j = 0; j < 4u; j++) {
                        const uint32_t m = sm[(4u * ly + i + ddy) * LW + 4u * lx + j + ddx + om];
                        const uint32_t d = m > bv[i][j] ? m - bv[i][j] : bv[i][j] - m;
                        v += (i < ny && j < nx) ? d : 0u;
                    }
#pragma unroll
                for (int d = 32; d >= 1; d >>= 1)
                    v += __shfl_xor(v, d);
                EST_PATH(SLOT + SK_WAVE_ADD, __lane_id() == 0u && v != 0u);
                EST_PATH(SLOT + SK_WAVE_SKIP, __lane_id() == 0u && v == 0u);
                if (__lane_id() == 0u && v)
                    atomicAdd(&s_acc[c], v);
            }
        }
    }
    __syncthreads();
    unsigned long long *acc = A.acc + slot * A.nacc + A.acc0;
#ifdef MCRAW_PATHSA
    for (uint32_t i = threadIdx.x; i < ncand; i += AL_T) {
        EST_PATH(SLOT + SK_STORE, A.pieces == 1u && !CL_SLOW);
        EST_PATH(SLOT + SK_GLOB_ADD, !(A.pieces == 1u && !CL_SLOW) && s_acc[i] != 0u);
        EST_PATH(SLOT + SK_GLOB_SKIP, !(A.pieces == 1u && !CL_SLOW) && s_acc[i] == 0u);
    }
#endif
    if (A.pieces == 1u && !CL_SLOW) { // the cell is this workgroup's alone: a cell without pixels stores its zeros
        for (uint32_t i = threadIdx.x; i < ncand; i += AL_T)
            acc[i] = s_acc[i];
    } else {
        for (uint32_t i = threadIdx.x; i < ncand; i += AL_T)
            if (s_acc[i])
                atomicAdd(acc + i, static_cast<unsigned long long>(s_acc[i]));
    }
}

__global__ void __launch_bounds__(AL_T) kcells_zero(unsigned long long *p, size_t words)
{
    EST_ONE(EP_CZ_LAUNCH, blockIdx.x == 0u);
    const size_t step = static_cast<size_t>(gridDim.x) * AL_T;
    for (size_t i = static_cast<size_t>(blockIdx.x) * AL_T + threadIdx.x; i < words; i += step)
        p[i] = 0ull;
}

// The winner of every cell of every pair of the launch at one level: the smallest (SAD, ddy^2 + ddx^2, ddy, ddx).  The candidates
// are walked in the order of (ddy, ddx), so a later one wins only with a smaller (SAD, distance).
__global__ void __launch_bounds__(AL_T) kcells_pick(const unsigned long long *acc, CellWin *win, const int16_t *gpos, uint32_t nacc,
                                                    uint32_t acc0, uint32_t R, uint32_t level, uint32_t top, uint32_t cells, int t0, int ref)
{
    const uint32_t cell = blockIdx.x * AL_T + threadIdx.x;
    const int t = t0 + static_cast<int>(blockIdx.y), b = al_base(t, ref);
    EST_PATH(EP_CP_NOPAIR, cell >= cells || b < 0);
    if (cell >= cells || b < 0)
        return;
    const size_t slot = static_cast<size_t>(t) * cells + cell;
    CellWin *wv = win + slot * CL_MAXLEVELS;
    int cy, cx;
    if (top)
        cl_centre(gpos, t, b, level, cy, cx);
    else
        cy = 2 * wv[level + 1u].dy, cx = 2 * wv[level + 1u].dx;
    const unsigned long long *a = acc + slot * nacc + acc0;
    const int r = static_cast<int>(R);
    unsigned long long best = ~0ull;
    int bd = 0x7FFFFFFF, by = 0, bx = 0;
    for (int ddy = -r; ddy <= r; ddy++)
        for (int ddx = -r; ddx <= r; ddx++) {
            const unsigned long long s = a[(ddy + r) * (2 * r + 1) + (ddx + r)];
            const int d2 = ddy * ddy + ddx * ddx;
            if (s < best || (s == best && d2 < bd))
                best = s, bd = d2, by = ddy, bx = ddx;
        }
    wv[level].dy = cy + by;
    wv[level].dx = cx + bx;
    wv[level].sad = best;
}

// pos and sad from the level-0 winners, a thread per cell: the frames in order with a running sum (the chain), or every frame on
// its own (the anchor form).  n < 2: zeros, and the winners are not read.
__global__ void __launch_bounds__(AL_T) kcells_final(const CellWin *win, int16_t *pos, unsigned long long *sad, uint32_t cells, int n, int ref)
{
    const uint32_t cell = blockIdx.x * AL_T + threadIdx.x;
    EST_PATH(EP_CF_PAST, cell >= cells);
    if (cell >= cells)
        return;
    int sy = 0, sx = 0;
    for (int t = 0; t < n; t++) {
        const size_t slot = static_cast<size_t>(t) * cells + cell;
        int dy = 0, dx = 0;
        unsigned long long sv = 0ull;
        if (n > 1 && al_base(t, ref) >= 0) {
            const CellWin wv = win[slot * CL_MAXLEVELS];
            dy = 2 * wv.dy, dx = 2 * wv.dx, sv = wv.sad;
        }
        if (ref < 0)
            dy = sy += dy, dx = sx += dx;
        EST_PATH(EP_CF_NOPAIR, !(n > 1 && al_base(t, ref) >= 0));
        EST_PATH(EP_CF_CLAMP, dy < -32768 || dy > 32767);
        EST_PATH(EP_CF_CLAMP, dx < -32768 || dx > 32767);
        pos[2u * slot] = static_cast<int16_t>(max(-32768, min(32767, dy)));
        pos[2u * slot + 1u] = static_cast<int16_t>(max(-32768, min(32767, dx)));
        if (sad)
            sad[slot] = sv;
    }
}

} // namespace mcraw

using namespace mcraw;

extern "C" size_t mcraw_align_cells_work_bytes(int width, int height, int n, uint32_t levels, uint32_t radius, uint32_t cell_h, uint32_t cell_w)
{
    CellsPlan P;
    if (n < 1 || P.make(width, height, static_cast<size_t>(n), levels, radius, cell_h, cell_w))
        return 0u;
    return P.total;
}

static int mcraw_cells_launch(const mcraw_align_cells *a, const MosaicBatch &I, const CellsPlan &P, const uint16_t *in, int n, hipStream_t st)
{
    char *work = static_cast<char *>(a->work);
    uint16_t *pyr = reinterpret_cast<uint16_t *>(work + P.pyr);
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(work + P.acc);
    CellWin *win = reinterpret_cast<CellWin *>(work + P.win);
    const uint32_t cells = static_cast<uint32_t>(P.G.cells());
    if (n > 1) {
        uint32_t px[CL_MAXLEVELS], pieces[CL_MAXLEVELS];
        bool shared = false; // a cell spans several workgroups at some level
        for (uint32_t l = 0; l < P.levels; l++) {
            px[l] = ((P.G.cell_w >> (l + 1u)) + AL_TW - 1u) / AL_TW;
            pieces[l] = px[l] * (((P.G.cell_h >> (l + 1u)) + AL_TH - 1u) / AL_TH);
            shared = shared || pieces[l] != 1u || CL_SLOW;
        }
        if (shared) {
            const size_t words = static_cast<size_t>(n) * cells * P.nacc;
            hipLaunchKernelGGL(kcells_zero, dim3(static_cast<uint32_t>(std::min<size_t>((words + AL_T - 1u) / AL_T, 4096u))), dim3(AL_T), 0, st, acc, words);
            HIP_TRY(hipGetLastError());
        }
        AlPyramid G{};
        G.levels = P.levels, G.frame_elems = P.frame_elems;
        for (uint32_t l = 0; l < P.levels; l++)
            G.h[l] = P.h[l], G.w[l] = P.w[l], G.pitch[l] = P.pitch[l], G.off[l] = P.off[l];
        if (const int rc = align_pyramid(st, I, in, n, a->black, G, pyr))
            return rc;
        for (uint32_t l = P.levels; l-- > 0u;) { // coarsest first
            ClSadArgs S{};
            S.pyr = pyr, S.acc = acc, S.win = win, S.gpos = a->gpos;
            S.pstride = P.frame_elems, S.loff = P.off[l];
            S.pitch = P.pitch[l], S.h = P.h[l], S.w = P.w[l];
            S.top = l == P.levels - 1u ? 1u : 0u;
            S.R = S.top ? P.radius : 1u;
            S.level = l, S.nacc = P.nacc, S.acc0 = P.acc0[l];
            S.ch = P.G.cell_h >> (l + 1u), S.cw = P.G.cell_w >> (l + 1u);
            S.cells_x = P.G.cells_x, S.cells = cells;
            S.px = px[l], S.pieces = pieces[l];
            S.ref = a->ref;
            for (int f0 = 0; f0 < n; f0 += LAUNCH_PIECE) {
                S.t0 = f0;
                const uint32_t nf = static_cast<uint32_t>(std::min<int>(LAUNCH_PIECE, n - f0));
                const dim3 grid(cells * pieces[l], nf);
                if (S.top) // (the coarsest level takes the loop whatever its radius: one instance per role)
                    hipLaunchKernelGGL(kcells_sad<0>, grid, dim3(AL_T), 0, st, S);
                else
                    hipLaunchKernelGGL(kcells_sad<1>, grid, dim3(AL_T), 0, st, S);
                HIP_TRY(hipGetLastError());
                hipLaunchKernelGGL(kcells_pick, dim3((cells + AL_T - 1u) / AL_T, nf), dim3(AL_T), 0, st, acc, win, a->gpos, P.nacc, P.acc0[l], S.R, l,
                                   S.top, cells, f0, static_cast<int>(a->ref));
                HIP_TRY(hipGetLastError());
            }
        }
    }
    hipLaunchKernelGGL(kcells_final, dim3((cells + AL_T - 1u) / AL_T), dim3(AL_T), 0, st, win, a->pos, reinterpret_cast<unsigned long long *>(a->sad),
                       cells, n, static_cast<int>(a->ref));
    HIP_TRY(hipGetLastError());
    return 0;
}

extern "C" int mcraw_align_cells_batch(mcraw_ctx *c, const mcraw_align_cells *a, const uint16_t *in, size_t in_pitch, size_t in_frame_stride,
                                       int width, int height, int n, void *stream)
{
    if (!c || !a || n < 0)
        return reject(__func__, "bad arguments");
    if (n == 0)
        return 0;
    if (!in)
        return reject(__func__, "in missing");
    if (reinterpret_cast<uintptr_t>(in) & 1u)
        return reject(__func__, "in not aligned to uint16");
    const MosaicBatch I(in, in_pitch, in_frame_stride, static_cast<size_t>(n), width, height);
    if (const char *why = I.check())
        return reject(__func__, why);
    if (a->ref < -1 || a->ref >= n)
        return reject(__func__, "ref must be -1 (a chain) or 0 .. n - 1");
    if (a->reserved != 0u)
        return reject(__func__, "reserved must be 0");
    CellsPlan P;
    if (const char *why = P.make(width, height, static_cast<size_t>(n), a->levels, a->radius, a->cell_h, a->cell_w))
        return reject(__func__, why);
    if (const char *why = check_cells_ptrs(I, P, static_cast<size_t>(n), a->pos, a->sad, a->gpos, a->work, a->work_bytes))
        return reject(__func__, why);

    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    return mcraw_cells_launch(a, I, P, in, n, stream_of(c, stream));
}
