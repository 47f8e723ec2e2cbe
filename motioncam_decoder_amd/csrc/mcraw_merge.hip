// mcraw_merge.hip -- gfx950 kernel for uint16 mosaics resident in HBM -> noise-adaptive temporal merges of them
// (mcraw_merge_batch).  The contract (integers only, bit-exact) is in include/mcraw_hip.h; DESIGN.md 20 has the design.
//
// kmerge<SUPPORT, NT>: a workgroup owns a tile of MG_TW columns x MG_TH rows of one output frame.  It stages the base frame's
// tile with a halo of one row and one column in LDS as raw samples, 16-byte chunks on the frame's 8-column grid (kfixpix's and
// kdenoise's staging), and the base frame's table behind it.  Then it walks the window's members: each member's tile, moved by
// the member's shift, is staged in a second LDS buffer on the BASE's grid (LDS column k holds the member's sample for base
// column k), so the lanes read both buffers at the same addresses.  A shift is even: a shifted piece of a row is 4-byte but
// not 16-byte aligned in memory, and is fetched with one unaligned 16-byte load.  Samples outside the frame are staged as 0.
// Lane (lx, ly) makes 8 columns of MG_RPL consecutive rows.  For support 1 it forms, row by row, the differences e = a - c of
// the 10 columns x - 1 .. x + 8 (0 outside the valid region: the frame intersected with the frame moved by the shift), their
// three-term sums along the row, and adds three such rows: s = boxV(member) - boxV(base) + (9 - nvalid) * e0, nvalid being a
// product of a row count and a column count because the region is a rectangle.  num and den stay in registers over the
// members.  Workgroups are numbered so that consecutive base frames of one tile run next to each other on one XCD: a member
// is fetched from HBM once and found in that XCD's L2 by the other bases that hold it in their windows.
// kmerge<SUPPORT, NT, true, MgCellArgs> (mcraw_merge_cells_batch): the same kernel, a tile reading its shifts from the cell of a
// position field that it lies in.
//
// Test builds (build.MOSAIC_PATH_VARIANTS, tests/test_gpu_mosaic_paths.py; why each is valid: the head of mcraw_mosaic_paths.h):
//   MCRAW_PATHSM         the path census
//   MCRAW_FORCE_SLOWM    a member that weighs 0 for the whole tile is staged like any other
//   MCRAW_POISON_M       s_b filled with 0xFFFF in front of the base's staging, s_m in front of every member's
//   MCRAW_MERGE_PIECE=N  N outputs per launch
#include "mcraw_host.h"
#ifdef MCRAW_PATHSM
#include "mcraw_mosaic_paths.h"
#endif
#include "mcraw_mosaic.h"
#include "mcraw_cells_args.h"

namespace mcraw {

constexpr int MG_T = 256;        // threads per workgroup
constexpr uint32_t MG_LX = 32u;  // lanes across a tile: 8 columns each
constexpr uint32_t MG_LY = MG_T / MG_LX;
constexpr uint32_t MG_TW = 8u * MG_LX;
// Tile rows: a lane makes MG_TH / MG_LY consecutive rows and needs the row above and the row below them.
#ifndef MCRAW_MERGE_TH
#define MCRAW_MERGE_TH 32
#endif
constexpr uint32_t MG_TH = MCRAW_MERGE_TH;
static_assert(MG_TH == 16u || MG_TH == 32u, "a lane's rows are consecutive: the tile is a multiple of MG_LY");
constexpr uint32_t MG_RPL = MG_TH / MG_LY; // rows per lane
constexpr uint32_t MG_LW = MG_TW + 16u;    // LDS row: 8 columns either side (1 used), so that chunks stay on the 8-grid
constexpr uint32_t MG_CH = MG_LW / 8u;     // 16-byte chunks per LDS row
constexpr uint32_t MG_LH = MG_TH + 2u;
constexpr uint32_t MG_XCDS = 8u;           // workgroups are dealt round-robin over the XCDs
#ifdef MCRAW_MERGE_PIECE
constexpr uint32_t MG_PIECE = MCRAW_MERGE_PIECE; // outputs per launch
static_assert(MG_PIECE >= 1u && MG_PIECE <= 2048u, "a frame has at most 2^19 tiles: tiles * outputs stays below 2^30 workgroups");
#else
constexpr uint32_t MG_PIECE = 0u; // as many as keep a launch below 2^30 workgroups
#endif
#ifdef MCRAW_FORCE_SLOWM
constexpr bool MG_SKIP_OK = false;
#else
constexpr bool MG_SKIP_OK = true; // a member that weighs 0 for every pixel of the tile is not staged
#endif

#ifdef MCRAW_MERGE_FLIP_STORES
constexpr bool MG_NT = false;
#else
constexpr bool MG_NT = true;
#endif

struct MgArgs {
    const uint16_t *in;  // frame 0 of the batch
    uint16_t *out;       // the launch's first output
    const uint16_t *lut; // table 0
    const int16_t *pos;  // (n, 2) as (y, x), or NULL
    size_t ipitch, ifstride, opitch, ofstride;
    uint32_t W, H, tilesX, tiles;
    uint32_t n, before, after, first; // first: the base of the launch's first output
    uint32_t nout, per;               // outputs of the launch; workgroups per XCD
    uint32_t amount, L, shift, perframe;
    uint32_t invec, outvec; // every 8-column piece of `in` / `out` lies on the 16-byte grid
};

// Stage rows y0 - 1 .. y0 + MG_TH, columns x0 - 8 .. x0 + MG_TW + 7 of `frm` moved by (sy, sx) into s: LDS column k of LDS row
// r holds frm[y0 - 1 + r + sy][x0 - 8 + k + sx], or 0 where that lies outside the frame.  Of the first and the last chunk only
// the column next to the tile is read by anyone.  aligned: the pieces lie on the 16-byte grid (invec and sx % 8 == 0).
__device__ __forceinline__ void mg_stage(uint16_t *s, const uint16_t *frm, size_t pitch, int W, int H, int y0, int x0, int sy, int sx,
                                         bool aligned)
{
    for (uint32_t i = threadIdx.x; i < MG_LH * MG_CH; i += MG_T) {
        const uint32_t r = i / MG_CH, q = i % MG_CH;
        const int yy = y0 - 1 + static_cast<int>(r) + sy, xs = x0 - 8 + 8 * static_cast<int>(q) + sx;
        mcraw_u32x4 v = {0u, 0u, 0u, 0u};
        MOS_PATH(MP_MG_ZERO, !(yy >= 0 && yy < H && xs + 8 > 0 && xs < W));
        if (yy >= 0 && yy < H && xs + 8 > 0 && xs < W) {
            MOS_STAGE(q != 0u && q != MG_CH - 1u, xs >= 0 && xs + 8 <= W, aligned);
            MOS_PATH(MP_MG_CUT, q != 0u && q != MG_CH - 1u && xs < 0);
            const uint16_t *row = frm + static_cast<size_t>(yy) * pitch;
            if (q != 0u && q != MG_CH - 1u && xs >= 0 && xs + 8 <= W) { // a full piece of the row
                v = load16(row + xs, aligned); // (not aligned: the base address, the pitch, or a shift that is no multiple of 8)
            } else { // the halo columns and the pieces that the frame's edge cuts: element loads
                const int e0 = q == 0u ? 7 : 0, e1 = q == MG_CH - 1u ? 1 : 8;
                uint32_t u[8];
#pragma unroll
                for (int e = 0; e < 8; e++)
                    u[e] = (e >= e0 && e < e1 && xs + e >= 0 && xs + e < W) ? gptr<const uint16_t>(row)[xs + e] : 0u;
                v = mcraw_u32x4{u[0] | (u[1] << 16), u[2] | (u[3] << 16), u[4] | (u[5] << 16), u[6] | (u[7] << 16)};
            }
        }
        *reinterpret_cast<mcraw_u32x4 *>(&s[r * MG_LW + 8u * q]) = v;
    }
}

// The 12 columns x - 2 .. x + 9 of an LDS row as 6 dwords (p: the row's column x - 2; 4-byte aligned, p + 2 16-byte aligned).
__device__ __forceinline__ void mg_row(const uint16_t *p, uint32_t w[6])
{
    const uint32_t a0 = *reinterpret_cast<const uint32_t *>(p);
    const mcraw_u32x4 a1 = *reinterpret_cast<const mcraw_u32x4 *>(p + 2);
    const uint32_t a2 = *reinterpret_cast<const uint32_t *>(p + 10);
    w[0] = a0, w[1] = a1[0], w[2] = a1[1], w[3] = a1[2], w[4] = a1[3], w[5] = a2;
}

// mcraw_merge_cells_batch: `pos` is a field (n, cells_y, cells_x, 2), and a tile reads the shifts of the cell it lies in.
struct MgCellArgs : MgArgs {
    uint32_t cell_h, cell_w, cells_x, cells; // a cell in samples (whole tiles); cells across, cells per frame
};

// FIELD changes only where by, bx, sy, sx are read: A.pos[(frame * cells + the tile's cell) * 2 ..] instead of A.pos[frame * 2 ..].
template <int SUPPORT, bool NT, bool FIELD = false, class ARGS = MgArgs>
__global__ void __launch_bounds__(MG_T) kmerge(const ARGS A)
{
    __shared__ __attribute__((aligned(16))) uint16_t s_b[MG_LH * MG_LW];      // the base's tile and its halo
    __shared__ __attribute__((aligned(16))) uint16_t s_m[MG_LH * MG_LW];      // one member's, moved by its shift
    extern __shared__ __attribute__((aligned(16))) uint16_t mg_lut[];         // the base's table: 4 * L entries (the launch sizes it)
    // consecutive workgroup ids go to consecutive XCDs: XCD k takes the k-th run of `per` (tile, output) pairs, outputs fastest
    const uint32_t l = (blockIdx.x % MG_XCDS) * A.per + blockIdx.x / MG_XCDS;
    MOS_PATH(MP_WG, threadIdx.x == 0u);
    MOS_PATH(MP_MG_LAUNCH, threadIdx.x == 0u && blockIdx.x == 0u);
    MOS_PATH(MP_MG_SHORT, threadIdx.x == 0u && l >= A.tiles * A.nout);
    if (l >= A.tiles * A.nout) // the last XCD's run may be short
        return;
    const uint32_t tile = l / A.nout, j = l - tile * A.nout;
    const uint32_t ty = tile / A.tilesX, tx = tile - ty * A.tilesX;
    const int W = static_cast<int>(A.W), H = static_cast<int>(A.H);
    const int x0 = static_cast<int>(tx * MG_TW), y0 = static_cast<int>(ty * MG_TH);
    const uint32_t b = A.first + j;
    {
        const uint16_t *lut = A.lut + (A.perframe ? static_cast<size_t>(b) * 4u * A.L : 0u);
        for (uint32_t i = threadIdx.x; i < A.L / 2u; i += MG_T) // 4 * L * 2 bytes in 16-byte chunks (L >= 64)
            *reinterpret_cast<mcraw_u32x4 *>(&mg_lut[8u * i]) = *gptr<const mcraw_u32x4>(lut + 8u * i);
    }
#ifdef MCRAW_POISON_M
    poison_tile(s_b, MG_LH * MG_LW);
#endif
    mg_stage(s_b, A.in + static_cast<size_t>(b) * A.ifstride, A.ipitch, W, H, y0, x0, 0, 0, A.invec != 0u);
    __syncthreads();
    const uint32_t lx = threadIdx.x % MG_LX, ly = threadIdx.x / MG_LX;
    const uint32_t x = static_cast<uint32_t>(x0) + 8u * lx;
    const uint32_t r0 = ly * MG_RPL; // the lane's first row in the tile; LDS row r0 is the row above it
    const uint16_t *lb = &s_b[r0 * MG_LW + 8u * lx + 6u], *lm = &s_m[r0 * MG_LW + 8u * lx + 6u]; // column x - 2
    const uint32_t lmax = A.L - 1u;
    uint32_t c[MG_RPL][4], rv[MG_RPL][4], num[MG_RPL][8], den[MG_RPL][8];
#pragma unroll
    for (uint32_t o = 0; o < MG_RPL; o++) {
        uint32_t w[6];
        mg_row(lb + (o + 1u) * MG_LW, w);
        const uint32_t yp = (static_cast<uint32_t>(y0) + r0 + o) & 1u;
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) {
            c[o][k] = w[k + 1u];
            uint32_t t[2];
#pragma unroll
            for (uint32_t h = 0; h < 2u; h++) {
                const uint32_t cv = half16(c[o][k], h);
                t[h] = mg_lut[(2u * yp + h) * A.L + min(cv >> A.shift, lmax)];
                num[o][2u * k + h] = cv << 8;
                den[o][2u * k + h] = 256u;
            }
            rv[o][k] = t[0] | (t[1] << 16);
        }
    }
    const uint32_t tlo = b > A.before ? b - A.before : 0u, thi = min(A.n - 1u, b + A.after);
    int by = 0, bx = 0;
    const int16_t *fpos = nullptr; // FIELD: the entry of the tile's cell in frame 0's field; frame f's is A.cells entries on
    if constexpr (FIELD) {
        fpos = A.pos + 2u * (static_cast<size_t>(static_cast<uint32_t>(y0) / A.cell_h) * A.cells_x + static_cast<uint32_t>(x0) / A.cell_w);
        by = fpos[2u * (static_cast<size_t>(b) * A.cells)];
        bx = fpos[2u * (static_cast<size_t>(b) * A.cells) + 1u];
    } else if (A.pos) {
        by = A.pos[2u * b];
        bx = A.pos[2u * b + 1u];
    }
#pragma unroll 1
    for (uint32_t t = tlo; t <= thi; t++) {
        MOS_PATH(MP_MG_SELF, threadIdx.x == 0u && t == b);
        if (t == b)
            continue;
        int sy = 0, sx = 0;
        if constexpr (FIELD) {
            sy = (static_cast<int>(fpos[2u * (static_cast<size_t>(t) * A.cells)]) - by) & ~1;
            sx = (static_cast<int>(fpos[2u * (static_cast<size_t>(t) * A.cells) + 1u]) - bx) & ~1;
        } else if (A.pos) {
            sy = (static_cast<int>(A.pos[2u * t]) - by) & ~1;
            sx = (static_cast<int>(A.pos[2u * t + 1u]) - bx) & ~1;
        }
        // the valid region in the base's coordinates: the frame intersected with the frame moved by the shift
        const int ry0 = max(0, -sy), ry1 = min(H, H - sy), rx0 = max(0, -sx), rx1 = min(W, W - sx);
        MOS_PATH(MP_MG_ZEROW, threadIdx.x == 0u && MG_SKIP_OK &&
                                  (ry0 >= ry1 || rx0 >= rx1 || ry1 <= y0 || ry0 >= y0 + static_cast<int>(MG_TH) || rx1 <= x0 ||
                                   rx0 >= x0 + static_cast<int>(MG_TW)));
        if (MG_SKIP_OK &&
            (ry0 >= ry1 || rx0 >= rx1 || ry1 <= y0 || ry0 >= y0 + static_cast<int>(MG_TH) || rx1 <= x0 || rx0 >= x0 + static_cast<int>(MG_TW)))
            continue; // the member weighs 0 for every pixel of the tile (uniform over the workgroup)
        MOS_PATH(MP_MG_STAGED, threadIdx.x == 0u);
        MOS_PATH(MP_MG_M_ALIGNED, threadIdx.x == 0u && A.invec != 0u && (sx & 7) == 0);
        MOS_PATH(MP_MG_M_SX, threadIdx.x == 0u && A.invec != 0u && (sx & 7) != 0);
        MOS_PATH(MP_MG_M_INVEC, threadIdx.x == 0u && A.invec == 0u);
        __syncthreads(); // everyone has read the member before
#ifdef MCRAW_POISON_M
        poison_tile(s_m, MG_LH * MG_LW);
#endif
        mg_stage(s_m, A.in + static_cast<size_t>(t) * A.ifstride, A.ipitch, W, H, y0, x0, sy, sx, A.invec != 0u && (sx & 7) == 0);
        __syncthreads();
        // columns x - 1 .. x + 8: bit i says that column x - 1 + i is in the region
        uint32_t colv = 0u;
#pragma unroll
        for (int i = 0; i < 10; i++) {
            const int col = static_cast<int>(x) - 1 + i;
            colv |= (col >= rx0 && col < rx1) ? 1u << i : 0u;
        }
        if (SUPPORT == 0) {
#pragma unroll
            for (uint32_t o = 0; o < MG_RPL; o++) {
                const int y = y0 + static_cast<int>(r0 + o);
                const bool rowv = y >= ry0 && y < ry1;
                uint32_t w[6];
                mg_row(lm + (o + 1u) * MG_LW, w);
#pragma unroll
                for (uint32_t p = 0; p < 8u; p++) {
                    const uint32_t a = half16(w[1u + (p >> 1)], p & 1u), cv = half16(c[o][p >> 1], p & 1u);
                    const uint32_t D = a > cv ? a - cv : cv - a;
                    const uint32_t xr = mul24(D, half16(rv[o][p >> 1], p & 1u)) >> 8, xx = xr < 16u ? xr : 16u;
                    const uint32_t wt = (rowv && ((colv >> (p + 1u)) & 1u)) ? 256u - mul24(xx, xx) : 0u;
                    num[o][p] += mul24(wt, a);
                    den[o][p] += wt;
                }
            }
        } else {
            int cnty[MG_RPL]; // rows of y - 1 .. y + 1 in the region
            uint32_t nvx[8];  // columns of x - 1 .. x + 1 in the region
#pragma unroll
            for (uint32_t p = 0; p < 8u; p++)
                nvx[p] = __builtin_popcount((colv >> p) & 7u);
            int hs[3][8], ec[2][8]; // the row sums of rows i - 2 .. i (i % 3); e of rows i - 1, i (i % 2)
            uint32_t am[2][4];      // the member's samples of rows i - 1, i
#pragma unroll
            for (uint32_t i = 0; i < MG_RPL + 2u; i++) { // LDS rows r0 + i: the rows y = y0 + r0 - 1 + i
                const int y = y0 + static_cast<int>(r0 + i) - 1;
                const bool rowv = y >= ry0 && y < ry1;
                uint32_t wb[6], wm[6];
                mg_row(lb + i * MG_LW, wb);
                mg_row(lm + i * MG_LW, wm);
                int e[10];
#pragma unroll
                for (uint32_t k = 0; k < 10u; k++) { // column x - 1 + k: half (k + 1) & 1 of dword (k + 1) >> 1
                    const int d = static_cast<int>(half16(wm[(k + 1u) >> 1], (k + 1u) & 1u)) - static_cast<int>(half16(wb[(k + 1u) >> 1], (k + 1u) & 1u));
                    e[k] = (rowv && ((colv >> k) & 1u)) ? d : 0;
                }
#pragma unroll
                for (uint32_t p = 0; p < 8u; p++) {
                    hs[i % 3u][p] = e[p] + e[p + 1u] + e[p + 2u];
                    ec[i & 1u][p] = e[p + 1u];
                }
#pragma unroll
                for (uint32_t k = 0; k < 4u; k++)
                    am[i & 1u][k] = wm[k + 1u];
                if (i < 2u)
                    continue;
                const uint32_t o = i - 2u; // the output row whose centre is row i - 1
                const int yc = y - 1;
                const bool cenv = yc >= ry0 && yc < ry1;
                cnty[o] = (yc - 1 >= ry0 && yc - 1 < ry1 ? 1 : 0) + (cenv ? 1 : 0) + (rowv ? 1 : 0);
#pragma unroll
                for (uint32_t p = 0; p < 8u; p++) {
                    const int e0 = ec[(i - 1u) & 1u][p];
                    const int s = hs[0][p] + hs[1][p] + hs[2][p] + (9 - cnty[o] * static_cast<int>(nvx[p])) * e0;
                    const uint32_t as = static_cast<uint32_t>(s < 0 ? -s : s) >> 3, ae = static_cast<uint32_t>(e0 < 0 ? -e0 : e0) >> 1;
                    const uint32_t D = max(min(as, 65535u), ae);
                    const uint32_t a = half16(am[(i - 1u) & 1u][p >> 1], p & 1u);
                    const uint32_t xr = mul24(D, half16(rv[o][p >> 1], p & 1u)) >> 8, xx = xr < 16u ? xr : 16u;
                    const uint32_t wt = (cenv && ((colv >> (p + 1u)) & 1u)) ? 256u - mul24(xx, xx) : 0u;
                    num[o][p] += mul24(wt, a);
                    den[o][p] += wt;
                }
            }
        }
    }
    const uint32_t n = x < A.W ? min(8u, A.W - x) : 0u;
    MOS_PATH(MP_IDLE_LANE, n == 0u);
    if (n == 0u)
        return;
    uint16_t *fout = A.out + static_cast<size_t>(j) * A.ofstride + x;
#pragma unroll
    for (uint32_t o = 0; o < MG_RPL; o++) {
        const uint32_t y = static_cast<uint32_t>(y0) + r0 + o;
        MOS_PATH(MP_ROW_BREAK, y >= A.H);
        if (y >= A.H)
            break;
        uint32_t res[4];
#pragma unroll
        for (uint32_t k = 0; k < 4u; k++) {
            uint32_t v[2];
#pragma unroll
            for (uint32_t h = 0; h < 2u; h++) {
                const uint32_t p = 2u * k + h;
                const int32_t cv = static_cast<int32_t>(half16(c[o][k], h));
                const int32_t m = static_cast<int32_t>(div_round(num[o][p] + (den[o][p] >> 1), den[o][p]));
                v[h] = static_cast<uint32_t>(cv + (((m - cv) * static_cast<int32_t>(A.amount) + 128) >> 8));
            }
            res[k] = v[0] | (v[1] << 16);
        }
        store8<NT>(fout + static_cast<size_t>(y) * A.opitch, n, A.outvec != 0u, res);
    }
}

static void merge_launch(const MgCellArgs &A, uint32_t support, hipStream_t st)
{
    const dim3 grid(A.per * MG_XCDS), block(MG_T);
    const size_t dyn = static_cast<size_t>(A.L) * 8u;
    if (support)
        hipLaunchKernelGGL((MG_NT ? kmerge<1, true, true, MgCellArgs> : kmerge<1, false, true, MgCellArgs>), grid, block, dyn, st, A);
    else
        hipLaunchKernelGGL((MG_NT ? kmerge<0, true, true, MgCellArgs> : kmerge<0, false, true, MgCellArgs>), grid, block, dyn, st, A);
}

static void merge_launch(const MgArgs &A, uint32_t support, hipStream_t st)
{
    const dim3 grid(A.per * MG_XCDS), block(MG_T);
    const size_t dyn = static_cast<size_t>(A.L) * 8u;
    if (support)
        hipLaunchKernelGGL((MG_NT ? kmerge<1, true> : kmerge<1, false>), grid, block, dyn, st, A);
    else
        hipLaunchKernelGGL((MG_NT ? kmerge<0, true> : kmerge<0, false>), grid, block, dyn, st, A);
}

} // namespace mcraw

using namespace mcraw;

// Both entry points: the checks on what they share, then the launches.  cells: NULL (mcraw_merge_batch), or the field's grid.
static int merge_entry(const char *fn, mcraw_ctx *c, const mcraw_merge *m, const mcraw_cells *cells, const uint16_t *in, size_t in_pitch,
                       size_t in_frame_stride, int width, int height, int n, uint16_t *out, size_t out_pitch, size_t out_frame_stride, void *stream)
{
    if (!c || !m || n < 0)
        return reject(fn, "bad arguments");
    if (n == 0 || m->count == 0u)
        return 0;
    if (!in || !out)
        return reject(fn, "in or out missing");
    if ((reinterpret_cast<uintptr_t>(in) & 1u) || (reinterpret_cast<uintptr_t>(out) & 1u) || (reinterpret_cast<uintptr_t>(m->pos) & 1u))
        return reject(fn, "in / out / pos not aligned to 2 bytes");
    const MosaicBatch I(in, in_pitch, in_frame_stride, static_cast<size_t>(n), width, height);
    const MosaicBatch O(out, out_pitch, out_frame_stride, static_cast<size_t>(m->count), width, height);
    if (const char *why = check(I, O))
        return reject(fn, why);
    if (m->before > 15u || m->after > 15u || m->before + m->after > 15u)
        return reject(fn, "before + after must be 0 .. 15");
    if (m->first > static_cast<uint32_t>(n) || m->count > static_cast<uint32_t>(n) - m->first)
        return reject(fn, "first + count must not exceed n");
    if (m->support > 1u)
        return reject(fn, "support must be 0 or 1");
    if (m->amount < 1u || m->amount > 256u)
        return reject(fn, "amount must be 1 .. 256");
    if (m->lut_log2 < 6u || m->lut_log2 > 10u)
        return reject(fn, "lut_log2 must be 6 .. 10");
    if (m->shift > 15u)
        return reject(fn, "shift must be 0 .. 15");
    if (m->nluts != 1u && m->nluts != static_cast<uint32_t>(n))
        return reject(fn, "nluts must be 1 or n");
    if (m->reserved != 0u)
        return reject(fn, "reserved must be 0");
    if (!m->lut || (reinterpret_cast<uintptr_t>(m->lut) & 15u))
        return reject(fn, "lut missing or not 16-byte aligned");
    if (overlap(I, O))
        return reject(fn, "in and out overlap (every output reads several frames: there is no in-place form)");
    if (cells) {
        if (m->pos)
            return reject(fn, "m->pos must be NULL: the positions are the cells'");
        if (const char *why = check_merge_cells(O, static_cast<size_t>(n), width, height, cells->cell_h, cells->cell_w, cells->cells_y,
                                                cells->cells_x, cells->reserved, cells->pos))
            return reject(fn, why);
    }

    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = stream_of(c, stream);
    MgCellArgs A{};
    A.in = in;
    A.lut = m->lut;
    A.pos = cells ? cells->pos : m->pos;
    A.ipitch = in_pitch;
    A.ifstride = in_frame_stride;
    A.opitch = out_pitch;
    A.ofstride = out_frame_stride;
    A.W = static_cast<uint32_t>(width);
    A.H = static_cast<uint32_t>(height);
    A.tilesX = (A.W + MG_TW - 1u) / MG_TW;
    A.tiles = A.tilesX * ((A.H + MG_TH - 1u) / MG_TH);
    A.n = static_cast<uint32_t>(n);
    A.before = m->before;
    A.after = m->after;
    A.amount = m->amount;
    A.L = 1u << m->lut_log2;
    A.shift = m->shift;
    A.perframe = m->nluts != 1u ? 1u : 0u;
    A.invec = I.on_grid();
    A.outvec = O.on_grid();
    if (cells) {
        A.cell_h = cells->cell_h, A.cell_w = cells->cell_w, A.cells_x = cells->cells_x;
        A.cells = cells->cells_y * cells->cells_x;
    }
    const uint32_t piece = MG_PIECE ? MG_PIECE : std::max(1u, std::min(65535u, 0x40000000u / A.tiles)); // outputs per launch: below 2^30 workgroups
    for (uint32_t j0 = 0; j0 < m->count; j0 += piece) {
        A.nout = std::min(piece, m->count - j0);
        A.first = m->first + j0;
        A.out = out + static_cast<size_t>(j0) * out_frame_stride;
        A.per = (A.tiles * A.nout + MG_XCDS - 1u) / MG_XCDS;
        if (cells)
            merge_launch(A, m->support, st);
        else
            merge_launch(static_cast<const MgArgs &>(A), m->support, st);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

extern "C" int mcraw_merge_batch(mcraw_ctx *c, const mcraw_merge *m, const uint16_t *in, size_t in_pitch, size_t in_frame_stride,
                                 int width, int height, int n, uint16_t *out, size_t out_pitch, size_t out_frame_stride,
                                 void *stream)
{
    return merge_entry(__func__, c, m, nullptr, in, in_pitch, in_frame_stride, width, height, n, out, out_pitch, out_frame_stride, stream);
}

extern "C" int mcraw_merge_cells_batch(mcraw_ctx *c, const mcraw_merge *m, const mcraw_cells *cells, const uint16_t *in, size_t in_pitch,
                                       size_t in_frame_stride, int width, int height, int n, uint16_t *out, size_t out_pitch,
                                       size_t out_frame_stride, void *stream)
{
    if (!cells)
        return reject(__func__, "cells missing");
    return merge_entry(__func__, c, m, cells, in, in_pitch, in_frame_stride, width, height, n, out, out_pitch, out_frame_stride, stream);
}
