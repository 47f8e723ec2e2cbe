// mcraw_align.hip -- gfx950 kernels for uint16 mosaics resident in HBM -> one global shift per frame (mcraw_align_batch): what
// mcraw_merge_batch takes as `pos`.  The contract (integers only, bit-exact) is in include/mcraw_hip.h; DESIGN.md 23 has the design.
//
// Everything is queued on the stream; no level waits for the host.  In the caller's scratch (mcraw_align_args.h): per frame the
// pyramid's planes (rows of 16-byte multiples), per frame and level the candidates' 64-bit sums, and the levels' winners.
//   kalign_zero     empties the sums.
//   kalign_pyr      the one pass over the mosaics: a lane takes 8 columns of 8 rows (eight 16-byte loads in flight), subtracts the
//                   blacks with packed u16 operations and holds a 4 x 4 block of G0, the 2 x 2 block of G1 and the sample of G2
//                   under it in registers: levels 0 .. 2 leave in this pass, nothing goes through LDS.
//   kalign_down     one small launch per level from 3 on (1 / 64 of the grey plane and less).
//   kalign_sad<R>   one launch per level, coarsest first.  A workgroup takes AL_TW x AL_TH pixels of a pair's window and stages the
//                   base's tile and the member's tile, moved by the level's centre and wider by the candidates' margin, in LDS as
//                   dwords on the planes' even columns.  R = 1 (the refinement levels): a lane owns 4 x 4 pixels as pairs, reads
//                   six rows of the member once each and keeps the nine candidates' sums in registers (v_sad_u16: two differences
//                   and the add in one instruction).  R = 0 (the coarsest level, up to 17 x 17 candidates on a tiny plane): a loop
//                   over the candidates.  The wave's sums are reduced across lanes, the waves' in LDS, and a tile adds each
//                   candidate's 32-bit sum (4096 differences of at most 65535) to its 64-bit sum with one atomic.
//   kalign_pick     a pair's winner at the level by the contract's key; the next level's centre is twice it.
//   kalign_final    the chain's prefix sum over n in int32 (or the anchor form), the clamp, pos and sad.
// The pyramid's launches (align_pyramid), the pair rule and the nine-candidate refinement (al_refine) are shared with the cell-wise
// estimate, mcraw_cells.hip, through mcraw_align_pyr.h.
//
// Test builds (tests/test_gpu_est_paths.py, build.EST_PATH_VARIANTS; why each is valid: the head of mcraw_est_paths.h):
//   MCRAW_PATHSA        the path census; mcraw_diag_est_paths below adds up the sources that include mcraw_est_paths.h
//   MCRAW_EST_FRAMES=N  the launch loops take N frames at a time
//   MCRAW_FORCE_SLOWA   every wave of kalign_sad<1> takes al_refine<false>
//   MCRAW_POISON_A      s_m and s_b of kalign_sad hold 0xFFFF samples in front of staging
#ifdef MCRAW_PATHSA
#include "mcraw_est_paths.h"
#define EST_LD_BASE ::mcraw::EP_PY_LD
#endif
#ifdef MCRAW_EST_FRAMES
#define LAUNCH_PIECE MCRAW_EST_FRAMES
#endif
#include "mcraw_align_pyr.h"

namespace mcraw {

constexpr uint32_t AL_PW = 256u; // kalign_pyr's tile: 32 lanes across with 8 columns each,
constexpr uint32_t AL_PH = 64u;  //   8 lanes down with 8 rows each (kalign_sad's tile: AL_TW x AL_TH of mcraw_align_pyr.h)
// A build for timing the parts (tools/bench_align.py): the call stops after MCRAW_ALIGN_STOP of them -- the pyramid, then one per
// level, coarsest first -- and writes no positions.  Not the product.
#ifdef MCRAW_ALIGN_STOP
constexpr uint32_t AL_STOP = MCRAW_ALIGN_STOP;
#else
constexpr uint32_t AL_STOP = 0u;
#endif
#ifdef MCRAW_FORCE_SLOWA
constexpr bool AL_SLOW = true;
#else
constexpr bool AL_SLOW = false;
#endif

struct AlLevels { // a frame's pyramid
    uint32_t h[AL_MAXLEVELS], w[AL_MAXLEVELS], pitch[AL_MAXLEVELS];
    size_t off[AL_MAXLEVELS];
};

struct AlPyrArgs {
    const uint16_t *in; // the launch's first frame
    uint16_t *pyr;      // ... and its pyramid
    size_t ipitch, ifstride, pstride;
    uint32_t W, H, tilesX, levels, vec;
    uint32_t blk[2]; // black of (even column | odd column << 16) by row parity
    AlLevels L;
};

// One quad row of 8 columns: the 4 grey sums (before rounding) of rows a (even) and b (odd).
__device__ __forceinline__ void al_quads(const uint32_t a[4], const uint32_t b[4], uint32_t blk0, uint32_t blk1, uint32_t g[4])
{
#pragma unroll
    for (uint32_t k = 0; k < 4u; k++) {
        const uint32_t u = pk_sub(pk_max(a[k], blk0), blk0), v = pk_sub(pk_max(b[k], blk1), blk1); // max(s - black, 0), two at once
        g[k] = (u & 0xFFFFu) + (u >> 16) + (v & 0xFFFFu) + (v >> 16);
    }
}

__global__ void __launch_bounds__(AL_T) kalign_pyr(const AlPyrArgs A)
{
    const uint32_t f = blockIdx.y, ty = blockIdx.x / A.tilesX, tx = blockIdx.x - ty * A.tilesX;
    const uint32_t lx = threadIdx.x % 32u, ly = threadIdx.x / 32u;
    const uint32_t x = tx * AL_PW + 8u * lx, y = ty * AL_PH + 8u * ly; // the lane's 8 x 8 samples
    EST_ONE(EP_PY_WG, true);
    EST_PATH(EP_PY_RET, x >= A.W || y >= A.H);
    if (x >= A.W || y >= A.H)
        return;
    const uint16_t *src = A.in + static_cast<size_t>(f) * A.ifstride + static_cast<size_t>(y) * A.ipitch + x;
    const uint32_t nc = min(8u, A.W - x);
    uint32_t p[8][4];
#pragma unroll
    for (uint32_t r = 0; r < 8u; r++) {
        EST_PATH(EP_PY_ZERO_ROW, y + r >= A.H);
        if (y + r < A.H)
            load8(src + static_cast<size_t>(r) * A.ipitch, nc, A.vec != 0u, p[r]);
        else
            p[r][0] = p[r][1] = p[r][2] = p[r][3] = 0u;
    }
    uint16_t *pyr = A.pyr + static_cast<size_t>(f) * A.pstride;
    uint32_t g0[4][4]; // G0 rows y / 2 .. y / 2 + 3, columns x / 2 .. x / 2 + 3 (what lies outside the plane is never stored)
#pragma unroll
    for (uint32_t r = 0; r < 4u; r++) {
        al_quads(p[2u * r], p[2u * r + 1u], A.blk[0], A.blk[1], g0[r]);
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++)
            g0[r][k] = min((g0[r][k] + 2u) >> 2, 65535u);
    }
    {
        const uint32_t gx = x >> 1, gy = y >> 1, w0 = A.L.w[0], h0 = A.L.h[0];
        uint16_t *dst = pyr + A.L.off[0] + static_cast<size_t>(gy) * A.L.pitch[0] + gx; // 8-byte aligned: gx % 4 == 0, rows of 16 bytes
#pragma unroll
        for (uint32_t r = 0; r < 4u; r++) {
            EST_ADDN(EP_PY_G0_LEFT, gy + r >= h0, 4u - r);
            if (gy + r >= h0)
                break;
            EST_PATH(EP_PY_G0_VEC, gx + 4u <= w0);
            EST_PATH(EP_PY_G0_ELEM, gx + 4u > w0);
            uint16_t *d = dst + static_cast<size_t>(r) * A.L.pitch[0];
            if (gx + 4u <= w0) {
                typedef uint32_t u32x2 __attribute__((ext_vector_type(2)));
                *gptr<u32x2>(d) = u32x2{g0[r][0] | (g0[r][1] << 16), g0[r][2] | (g0[r][3] << 16)};
            } else {
#pragma unroll
                for (uint32_t k = 0; k < 4u; k++)
                    if (gx + k < w0)
                        gptr<uint16_t>(d)[k] = static_cast<uint16_t>(g0[r][k]);
            }
        }
    }
    EST_PATH(EP_PY_RET_L2, A.levels < 2u);
    if (A.levels < 2u)
        return;
    uint32_t g1[2][2];
#pragma unroll
    for (uint32_t r = 0; r < 2u; r++)
#pragma unroll
        for (uint32_t k = 0; k < 2u; k++)
            g1[r][k] = (g0[2u * r][2u * k] + g0[2u * r][2u * k + 1u] + g0[2u * r + 1u][2u * k] + g0[2u * r + 1u][2u * k + 1u] + 2u) >> 2;
    {
        const uint32_t gx = x >> 2, gy = y >> 2, w1 = A.L.w[1], h1 = A.L.h[1];
        uint16_t *dst = pyr + A.L.off[1] + static_cast<size_t>(gy) * A.L.pitch[1] + gx; // 4-byte aligned: gx % 2 == 0
#pragma unroll
        for (uint32_t r = 0; r < 2u; r++) {
            EST_ADDN(EP_PY_G1_LEFT, gy + r >= h1, 2u - r);
            if (gy + r >= h1)
                break;
            EST_PATH(EP_PY_G1_DWORD, gx + 2u <= w1);
            EST_PATH(EP_PY_G1_ELEM, gx + 2u > w1 && gx < w1);
            EST_PATH(EP_PY_G1_NONE, gx >= w1);
            uint16_t *d = dst + static_cast<size_t>(r) * A.L.pitch[1];
            if (gx + 2u <= w1)
                *gptr<uint32_t>(d) = g1[r][0] | (g1[r][1] << 16);
            else if (gx < w1)
                *gptr<uint16_t>(d) = static_cast<uint16_t>(g1[r][0]);
        }
    }
    EST_PATH(EP_PY_RET_L3, A.levels < 3u);
    if (A.levels < 3u)
        return;
    const uint32_t gx = x >> 3, gy = y >> 3;
    EST_PATH(EP_PY_G2_STORE, gx < A.L.w[2] && gy < A.L.h[2]);
    EST_PATH(EP_PY_G2_NONE, !(gx < A.L.w[2] && gy < A.L.h[2]));
    if (gx < A.L.w[2] && gy < A.L.h[2])
        gptr<uint16_t>(pyr + A.L.off[2] + static_cast<size_t>(gy) * A.L.pitch[2])[gx] =
            static_cast<uint16_t>((g1[0][0] + g1[0][1] + g1[1][0] + g1[1][1] + 2u) >> 2);
}

// G(l) -> G(l + 1) of every frame of the launch: a thread per sample.
__global__ void __launch_bounds__(AL_T) kalign_down(uint16_t *pyr, size_t pstride, size_t soff, uint32_t spitch, size_t doff, uint32_t dpitch,
                                                    uint32_t dh, uint32_t dw)
{
    const uint32_t i = blockIdx.x * AL_T + threadIdx.x;
    EST_ONE(EP_DN_LAUNCH, blockIdx.x == 0u && blockIdx.y == 0u);
    EST_PATH(EP_DN_PAST, i >= dh * dw);
    if (i >= dh * dw)
        return;
    const uint32_t y = i / dw, x = i - y * dw;
    uint16_t *fp = pyr + static_cast<size_t>(blockIdx.y) * pstride;
    const uint16_t *s = fp + soff + static_cast<size_t>(2u * y) * spitch + 2u * x; // an even column: a dword
    const uint32_t a = *gptr<const uint32_t>(s), b = *gptr<const uint32_t>(s + spitch);
    gptr<uint16_t>(fp + doff + static_cast<size_t>(y) * dpitch)[x] = static_cast<uint16_t>(((a & 0xFFFFu) + (a >> 16) + (b & 0xFFFFu) + (b >> 16) + 2u) >> 2);
}

__global__ void __launch_bounds__(AL_T) kalign_zero(unsigned long long *p, size_t words)
{
    EST_ONE(EP_AZ_LAUNCH, blockIdx.x == 0u);
    const size_t step = static_cast<size_t>(gridDim.x) * AL_T;
    for (size_t i = static_cast<size_t>(blockIdx.x) * AL_T + threadIdx.x; i < words; i += step)
        p[i] = 0ull;
}

struct AlSadArgs {
    const uint16_t *pyr; // frame 0's pyramid
    unsigned long long *acc; // frame 0's sums
    const AlignWin *win;     // frame 0's winners
    size_t pstride, loff;    // elements from pyramid to pyramid, from a pyramid to the level
    uint32_t pitch, h, w, B; // the level's plane and bound
    uint32_t R;              // the candidates' radius: `radius` at the coarsest level, 1 below
    uint32_t level, top;     // top: the coarsest level (the centre is (0, 0))
    uint32_t nacc, acc0;     // sums per frame; the level's first
    uint32_t tilesX;
    int32_t ref, t0;         // the launch's first frame
};

// rows x ndw dwords of the plane from row ys, even column xs on into s (LW elements per row); 0 below the plane.  The columns
// between w and pitch hold whatever the scratch held: no pixel of the window reads them.
// (SLOT, w: the census's, test builds only)
template <uint32_t SLOT>
__device__ __forceinline__ void al_stage(uint32_t *s, uint32_t LW, const uint16_t *plane, uint32_t pitch, uint32_t h, uint32_t w, uint32_t ys,
                                         uint32_t xs, uint32_t rows, uint32_t ndw)
{
    for (uint32_t i = threadIdx.x; i < rows * ndw; i += AL_T) {
        const uint32_t r = i / ndw, j = i - r * ndw, yy = ys + r, col = xs + 2u * j;
        EST_PATH(SLOT + SK_STG_LOAD, yy < h && col < pitch);
        EST_PATH(SLOT + SK_STG_ZERO_Y, yy >= h);
        EST_PATH(SLOT + SK_STG_ZERO_COL, yy < h && col >= pitch);
        EST_PATH(SLOT + SK_STG_PAD, yy < h && col < pitch && col + 1u >= w);
        uint32_t v = 0u;
        if (yy < h && col < pitch)
            v = *gptr<const uint32_t>(plane + static_cast<size_t>(yy) * pitch + col);
        s[r * (LW / 2u) + j] = v;
    }
}

// RT == 1: the refinement levels, nine candidates in registers.  RT == 0: A.R up to AL_MAXRADIUS, a loop over the candidates.
template <int RT>
__global__ void __launch_bounds__(AL_T) kalign_sad(const AlSadArgs A)
{
    constexpr uint32_t RMAX = RT ? 1u : AL_MAXRADIUS;
    constexpr uint32_t LW = (AL_TW + 2u * RMAX + 2u + 7u) / 8u * 8u; // elements per LDS row
    constexpr uint32_t NC = (2u * RMAX + 1u) * (2u * RMAX + 1u);
    __shared__ __attribute__((aligned(16))) uint32_t s_m[(AL_TH + 2u * RMAX) * LW / 2u];
    __shared__ __attribute__((aligned(16))) uint32_t s_b[AL_TH * LW / 2u];
    __shared__ uint32_t s_acc[NC];
    const int t = A.t0 + static_cast<int>(blockIdx.y), b = al_base(t, A.ref);
#ifdef MCRAW_PATHSA
    constexpr uint32_t SLOT = EP_AS + RT * SK_N; // this instance's counters
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
    int cy = 0, cx = 0;
    if (!A.top) {
        const AlignWin wv = A.win[static_cast<size_t>(t) * AL_MAXLEVELS + A.level + 1u];
        cy = 2 * wv.dy, cx = 2 * wv.dx; // |c| <= 2 B(l + 1) = B(l) - 1
    }
    const uint32_t ty = blockIdx.x / A.tilesX, tx = blockIdx.x - ty * A.tilesX;
    const uint32_t x0 = A.B + tx * AL_TW, y0 = A.B + ty * AL_TH, x1 = A.w - A.B, y1 = A.h - A.B; // the tile's origin, the window's end
    const uint32_t xm = static_cast<uint32_t>(static_cast<int>(x0) + cx) - R, ym = static_cast<uint32_t>(static_cast<int>(y0) + cy) - R; // >= 0
    const uint32_t om = xm & 1u, ob = x0 & 1u;
    const uint16_t *pb = A.pyr + static_cast<size_t>(b) * A.pstride + A.loff, *pm = A.pyr + static_cast<size_t>(t) * A.pstride + A.loff;
    for (uint32_t i = threadIdx.x; i < ncand; i += AL_T)
        s_acc[i] = 0u;
    EST_ONE(SLOT + SK_OM0 + 2u * ob + om, true);
    al_stage<SLOT>(s_b, LW, pb, A.pitch, A.h, A.w, y0, x0 & ~1u, AL_TH, AL_TW / 2u + 1u);
    al_stage<SLOT>(s_m, LW, pm, A.pitch, A.h, A.w, ym, xm & ~1u, AL_TH + 2u * R, AL_TW / 2u + R + 1u);
    __syncthreads();
    const uint32_t lx = threadIdx.x % 32u, ly = threadIdx.x / 32u;
    const uint32_t px = x0 + 4u * lx, py = y0 + 4u * ly; // the lane's 4 x 4 pixels
    const uint32_t nx = px < x1 ? min(4u, x1 - px) : 0u, ny = py < y1 ? min(4u, y1 - py) : 0u;
    EST_PATH(SLOT + SK_LANE_EMPTY, nx == 0u || ny == 0u);
    if (RT) {
        uint32_t acc[9];
        EST_PATH(SLOT + SK_REF_FULL, __all(nx == 4u && ny == 4u) && !AL_SLOW && __lane_id() == 0u); // (every lane takes part in __all)
        EST_PATH(SLOT + SK_REF_MASK, !(__all(nx == 4u && ny == 4u) && !AL_SLOW) && __lane_id() == 0u);
        if (!AL_SLOW && __all(nx == 4u && ny == 4u)) // the window's interior: no masks
            al_refine<true>(s_b, s_m, LW / 2u, lx, ly, ob, om, nx, ny, acc);
        else
            al_refine<false>(s_b, s_m, LW / 2u, lx, ly, ob, om, nx, ny, acc);
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
                bv[i][j] = sb[(4u * ly + i) * LW + 4u * lx + j + ob];
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
    __syncthreads();
    unsigned long long *acc = A.acc + static_cast<size_t>(t) * A.nacc + A.acc0;
#ifdef MCRAW_PATHSA
    for (uint32_t i = threadIdx.x; i < ncand; i += AL_T) {
        EST_PATH(SLOT + SK_GLOB_ADD, s_acc[i] != 0u);
        EST_PATH(SLOT + SK_GLOB_SKIP, s_acc[i] == 0u);
    }
#endif
    for (uint32_t i = threadIdx.x; i < ncand; i += AL_T)
        if (s_acc[i])
            atomicAdd(acc + i, static_cast<unsigned long long>(s_acc[i]));
}

// The winner of every pair of the launch at one level: the smallest (SAD, ddy^2 + ddx^2, ddy, ddx).  The candidates are walked in
// the order of (ddy, ddx), so a later one wins only with a smaller (SAD, distance).
__global__ void __launch_bounds__(AL_T) kalign_pick(const unsigned long long *acc, AlignWin *win, uint32_t nacc, uint32_t acc0, uint32_t R,
                                                    uint32_t level, uint32_t top, int n, int ref)
{
    const int t = static_cast<int>(blockIdx.x * AL_T + threadIdx.x);
    EST_PATH(EP_AP_NOPAIR, t >= n || al_base(t, ref) < 0);
    if (t >= n || al_base(t, ref) < 0)
        return;
    AlignWin *wv = win + static_cast<size_t>(t) * AL_MAXLEVELS;
    int cy = 0, cx = 0;
    if (!top)
        cy = 2 * wv[level + 1u].dy, cx = 2 * wv[level + 1u].dx;
    const unsigned long long *a = acc + static_cast<size_t>(t) * nacc + acc0;
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

// pos and sad from the level-0 winners: one workgroup walks the frames in pieces of AL_T with a running sum (the chain), or
// writes every frame on its own (the anchor form).
__global__ void __launch_bounds__(AL_T) kalign_final(const AlignWin *win, int16_t *pos, unsigned long long *sad, int n, int ref)
{
    __shared__ int s_y[AL_T], s_x[AL_T];
    int carry_y = 0, carry_x = 0;
    for (int t0 = 0; t0 < n; t0 += AL_T) {
        const int t = t0 + static_cast<int>(threadIdx.x);
        const bool paired = t < n && al_base(t, ref) >= 0;
        int dy = 0, dx = 0;
        unsigned long long sv = 0ull;
        if (paired) {
            const AlignWin wv = win[static_cast<size_t>(t) * AL_MAXLEVELS];
            dy = 2 * wv.dy, dx = 2 * wv.dx, sv = wv.sad;
        }
        EST_ONE(EP_AF_PIECE, ref < 0);
        if (ref < 0) { // inclusive scan of the piece (uniform: every thread takes part)
            s_y[threadIdx.x] = dy, s_x[threadIdx.x] = dx;
            __syncthreads();
            for (uint32_t d = 1; d < AL_T; d <<= 1) {
                const int ay = threadIdx.x >= d ? s_y[threadIdx.x - d] : 0, ax = threadIdx.x >= d ? s_x[threadIdx.x - d] : 0;
                __syncthreads();
                s_y[threadIdx.x] += ay, s_x[threadIdx.x] += ax;
                __syncthreads();
            }
            dy = carry_y + s_y[threadIdx.x], dx = carry_x + s_x[threadIdx.x];
            carry_y += s_y[AL_T - 1], carry_x += s_x[AL_T - 1];
            __syncthreads();
        }
        EST_PATH(EP_AF_CLAMP, t < n && (dy < -32768 || dy > 32767));
        EST_PATH(EP_AF_CLAMP, t < n && (dx < -32768 || dx > 32767));
        if (t < n) {
            pos[2 * static_cast<size_t>(t)] = static_cast<int16_t>(max(-32768, min(32767, dy)));
            pos[2 * static_cast<size_t>(t) + 1u] = static_cast<int16_t>(max(-32768, min(32767, dx)));
            if (sad)
                sad[t] = sv;
        }
    }
}

} // namespace mcraw

using namespace mcraw;

extern "C" size_t mcraw_align_work_bytes(int width, int height, int n, uint32_t levels, uint32_t radius)
{
    AlignPlan P;
    if (n < 1 || P.make(width, height, static_cast<size_t>(n), levels, radius))
        return 0u;
    return P.total;
}

// The census of the estimator sources that include mcraw_est_paths.h added up into out[0 .. n), and started over when `reset`; returns the number of
// counters, 0 in a build without the census (mcraw_est_paths.h).
extern "C" int mcraw_diag_est_paths(uint64_t *out, int n, int reset)
{
#ifdef MCRAW_PATHSA
    return census_sum<EstPath, EP_N>(out, n, reset);
#else
    (void)out, (void)n, (void)reset;
    return 0;
#endif
}

// The pyramids of the n frames (mcraw_align_pyr.h): the launch loop of the mosaic stages, grid.y frames at a time.
int mcraw::align_pyramid(hipStream_t st, const MosaicBatch &I, const uint16_t *in, int n, const uint16_t black[4], const AlPyramid &G, uint16_t *pyr)
{
    AlPyrArgs Y{};
    Y.ipitch = I.pitch, Y.ifstride = I.fstride, Y.pstride = G.frame_elems;
    Y.W = static_cast<uint32_t>(I.W), Y.H = static_cast<uint32_t>(I.H);
    Y.tilesX = (Y.W + AL_PW - 1u) / AL_PW;
    Y.levels = G.levels, Y.vec = I.on_grid();
    Y.blk[0] = black[0] | (static_cast<uint32_t>(black[1]) << 16);
    Y.blk[1] = black[2] | (static_cast<uint32_t>(black[3]) << 16);
    for (uint32_t l = 0; l < G.levels; l++)
        Y.L.h[l] = G.h[l], Y.L.w[l] = G.w[l], Y.L.pitch[l] = G.pitch[l], Y.L.off[l] = G.off[l];
    for (int f0 = 0; f0 < n; f0 += LAUNCH_PIECE) {
        const uint32_t nf = static_cast<uint32_t>(std::min<int>(LAUNCH_PIECE, n - f0));
        Y.in = in + static_cast<size_t>(f0) * I.fstride;
        Y.pyr = pyr + static_cast<size_t>(f0) * G.frame_elems;
        hipLaunchKernelGGL(kalign_pyr, dim3(Y.tilesX * ((Y.H + AL_PH - 1u) / AL_PH), nf), dim3(AL_T), 0, st, Y);
        HIP_TRY(hipGetLastError());
        for (uint32_t l = 3; l < G.levels; l++) {
            if (G.h[l] == 0u || G.w[l] == 0u)
                break;
            hipLaunchKernelGGL(kalign_down, dim3((G.h[l] * G.w[l] + AL_T - 1u) / AL_T, nf), dim3(AL_T), 0, st, Y.pyr, G.frame_elems, G.off[l - 1u],
                               G.pitch[l - 1u], G.off[l], G.pitch[l], G.h[l], G.w[l]);
            HIP_TRY(hipGetLastError());
        }
    }
    return 0;
}

static int mcraw_align_launch(mcraw_ctx *c, const mcraw_align *a, const MosaicBatch &I, const AlignPlan &P, const uint16_t *in, int n,
                              hipStream_t st)
{
    char *work = static_cast<char *>(a->work);
    uint16_t *pyr = reinterpret_cast<uint16_t *>(work + P.pyr);
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(work + P.acc);
    AlignWin *win = reinterpret_cast<AlignWin *>(work + P.win);
    if (n > 1) {
        const size_t words = static_cast<size_t>(n) * P.nacc;
        hipLaunchKernelGGL(kalign_zero, dim3(static_cast<uint32_t>(std::min<size_t>((words + AL_T - 1u) / AL_T, 4096u))), dim3(AL_T), 0, st, acc, words);
        HIP_TRY(hipGetLastError());
        AlPyramid G{};
        G.levels = P.levels, G.frame_elems = P.frame_elems;
        for (uint32_t l = 0; l < P.levels; l++)
            G.h[l] = P.h[l], G.w[l] = P.w[l], G.pitch[l] = P.pitch[l], G.off[l] = P.off[l];
        if (const int rc = align_pyramid(st, I, in, n, a->black, G, pyr))
            return rc;
        if (AL_STOP == 1u)
            return 0;
        for (uint32_t l = P.levels; l-- > 0u;) { // coarsest first
            AlSadArgs S{};
            S.pyr = pyr, S.acc = acc, S.win = win;
            S.pstride = P.frame_elems, S.loff = P.off[l];
            S.pitch = P.pitch[l], S.h = P.h[l], S.w = P.w[l], S.B = P.B[l];
            S.top = l == P.levels - 1u ? 1u : 0u;
            S.R = S.top ? P.radius : 1u;
            S.level = l, S.nacc = P.nacc, S.acc0 = P.acc0[l];
            S.tilesX = (S.w - 2u * S.B + AL_TW - 1u) / AL_TW;
            S.ref = a->ref;
            const uint32_t tiles = S.tilesX * ((S.h - 2u * S.B + AL_TH - 1u) / AL_TH);
            for (int f0 = 0; f0 < n; f0 += LAUNCH_PIECE) {
                S.t0 = f0;
                const dim3 grid(tiles, static_cast<uint32_t>(std::min<int>(LAUNCH_PIECE, n - f0)));
                if (S.R == 1u)
                    hipLaunchKernelGGL(kalign_sad<1>, grid, dim3(AL_T), 0, st, S);
                else
                    hipLaunchKernelGGL(kalign_sad<0>, grid, dim3(AL_T), 0, st, S);
                HIP_TRY(hipGetLastError());
            }
            hipLaunchKernelGGL(kalign_pick, dim3((static_cast<uint32_t>(n) + AL_T - 1u) / AL_T), dim3(AL_T), 0, st, acc, win, P.nacc, P.acc0[l], S.R, l,
                               S.top, n, static_cast<int>(a->ref));
            HIP_TRY(hipGetLastError());
            if (AL_STOP != 0u && P.levels - l + 1u >= AL_STOP)
                return 0;
        }
    }
    hipLaunchKernelGGL(kalign_final, dim3(1), dim3(AL_T), 0, st, win, a->pos, reinterpret_cast<unsigned long long *>(a->sad), n,
                       static_cast<int>(a->ref));
    HIP_TRY(hipGetLastError());
    (void)c;
    return 0;
}

extern "C" int mcraw_align_batch(mcraw_ctx *c, const mcraw_align *a, const uint16_t *in, size_t in_pitch, size_t in_frame_stride, int width,
                                 int height, int n, void *stream)
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
    AlignPlan P;
    if (const char *why = P.make(width, height, static_cast<size_t>(n), a->levels, a->radius))
        return reject(__func__, why);
    if (const char *why = check_align_ptrs(I, P, static_cast<size_t>(n), a->pos, a->sad, a->work, a->work_bytes))
        return reject(__func__, why);

    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    return mcraw_align_launch(c, a, I, P, in, n, stream_of(c, stream));
}
