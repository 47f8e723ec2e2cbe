// mcraw_rgb.hip -- gfx950 kernels for uint16 mosaics resident in HBM -> planar linear RGB (mcraw_demosaic_batch).
//
//   krgb_mhc   full resolution: Malvar-He-Cutler 5x5 gradient-corrected bilinear interpolation, in integers
//   krgb_bin2  half resolution: one output pixel per 2x2 CFA quad (R = r, G = mean(g1, g2), B = b)
//
// Both write (N, 3, Ho, Wo), channel-major per frame.  The arithmetic is the contract of include/mcraw_hip.h; the
// numpy statement of it is tests/_rgb_ref.py.  One instance per (dtype, CFA): the CFA decides at compile time which
// filter every lane slot runs.  CLIP is a wave-uniform run-time flag (v_med3_f32 under a uniform branch).
//
// The display kinds (PK_DISP8 / PK_DISP16, mcraw_demosaic_display_batch) share the integer estimates and the colour stage,
// then clamp, index a transfer-curve LUT and store uint8 / uint16, (N, 3, Ho, Wo) or (N, Ho, Wo, 3): layout and where the
// LUT is read from (LDS or global) are wave-uniform run-time flags.  Their grids are persistent (a grid-stride loop over
// tiles), so that each workgroup stages the LUT in LDS once; tests/_display_ref.py states the stage in numpy.
//
// The YUV kinds (PK_NV12 / PK_P010, mcraw_demosaic_yuv_batch) run the display stage up to the LUT entry, then an integer
// 3x3 matrix: a luma sample per pixel and, from the sums over each 2x2 block of output pixels, one (Cb, Cr) pair (4:2:0,
// chroma at the block's centre).  A lane owns whole 2x2 blocks (8 columns of a row pair), so nothing is exchanged.
// tests/_yuv_ref.py states the stage in numpy.
//
// The scaled siblings (krgb_area: mcraw_area.hip, krgb_resample: mcraw_resample.hip) share the device side through
// mcraw_rgb_dev.h and the host side of the launch through mcraw_rgb_launch.h.
//
// Test builds of the demosaic kernels (tests/test_gpu_rgb_paths.py, build.RGB_PATH_VARIANTS; none of this is in the product
// library).  MCRAW_PATHSR and MCRAW_POISON_RGB are read by this file, mcraw_area.hip, mcraw_resample.hip, mcraw_warp.hip,
// mcraw_mesh.hip and mcraw_ha.hip alone, MCRAW_RGB_GRID_CAP by the first three (the other three take rgb_grid_limit() below); the
// shared headers only have hooks that are empty unless defined in front of them.  Each switch chooses among ways that are right
// for EVERY input:
//   MCRAW_PATHSR            the path census (mcraw_rgb_paths.h; mcraw_diag_rgb_paths below adds up the sources that include it).
//   MCRAW_RGB_GRID_CAP=N    a persistent launch uses min(units x frames, N) workgroups, not min(units x frames, resident): the
//                           loop's condition makes any grid of 1 .. units x frames workgroups walk every unit exactly once.  The
//                           float kinds have no loop and are untouched.
//   MCRAW_POISON_RGB        a workgroup fills every LDS array it stages per unit with a non-zero pattern at the start of every
//                           unit, the first included, and syncs: a unit may read only what it staged itself, so a byte that
//                           changes proves a dependence on stale LDS.  s_lut, staged once per workgroup, is left alone (and
//                           s_w of krgb_warp and krgb_mesh).  The patterns: beside each rgb_poison().
#ifdef MCRAW_PATHSR
#include "mcraw_rgb_paths.h"
#endif
#ifdef MCRAW_RGB_GRID_CAP
#define RGB_GRID_LIMIT(resident) (static_cast<void>(resident), static_cast<uint32_t>(MCRAW_RGB_GRID_CAP))
#endif
#include "mcraw_dev.h"
#include "mcraw_host.h"
#include "mcraw_rgb_args.h"
#include "mcraw_rgb_dev.h"
#include "mcraw_rgb_launch.h"

namespace mcraw {

// ---- MHC --------------------------------------------------------------------------------------------------------------
//
// A workgroup owns a tile of 256 columns x 32 rows of one frame.  It stages the tile and a 2-pixel halo (reflected at the
// frame edges) in LDS as raw samples, 16-byte chunks on the frame's 8-column grid.  Lane (lx, ly) then makes 8 columns of
// row pairs ly and ly + 8: four CFA quads, so every filter choice is fixed per lane slot by the CFA (template S: the RGGB
// role of CFA position p is p ^ S).  The halo rows are read again by the tiles above and below (L2 / Infinity Cache).
// Float kinds: one tile per workgroup (blockIdx.x: tile, blockIdx.y: frame).  Display and YUV kinds: a persistent grid whose
// workgroups stage the LUT in LDS once and then take units t = blockIdx.x, + gridDim.x, ... (A.units tiles per frame, of
// the launch's A.nf frames); the loop runs once for the float kinds.
template <int PK, int S>
__global__ void __launch_bounds__(RGB_T) krgb_mhc(const RgbArgs A)
{
    constexpr bool DISP = has_lut(PK);
    __shared__ __attribute__((aligned(16))) uint16_t s_t[MHC_LH * MHC_LW];
    __shared__ __attribute__((aligned(16))) uint16_t s_lut[DISP ? DISP_LDS_MAX : 8u];
    uint32_t t = blockIdx.x;
    RGB_WALK_DECL;
    if constexpr (DISP)
        stage_lut(A, s_lut);
    do {
        if constexpr (DISP)
            __syncthreads(); // the LUT is staged; the previous tile's LDS reads are done
#ifdef MCRAW_POISON_RGB
        rgb_poison(s_t, sizeof(s_t), 0x5a5a5a5bu);
        __syncthreads();
#endif
        const uint32_t f = DISP ? t / A.units : blockIdx.y, u = DISP ? t % A.units : blockIdx.x;
        RGB_WALK(RF_MHC, f, DISP, A.lutg);
        const uint32_t tx = u % A.tilesX, ty = u / A.tilesX;
        const int W = static_cast<int>(A.W), H = static_cast<int>(A.H);
        const int x0 = static_cast<int>(tx * MHC_TW), y0 = static_cast<int>(ty * MHC_TH);
        const uint16_t *in = A.in + static_cast<size_t>(f) * A.fstride;
        for (uint32_t i = threadIdx.x; i < MHC_LH * MHC_CH; i += RGB_T) {
            const uint32_t r = i / MHC_CH, q = i % MHC_CH;
            const uint16_t *row = in + static_cast<size_t>(reflect101(y0 - 2 + static_cast<int>(r), H)) * A.pitch;
            const int xs = x0 - 8 + 8 * static_cast<int>(q);
            mcraw_u32x4 v;
            if (A.invec && xs >= 0 && xs + 8 <= W) {
                RGB_PATH(RP_LD_MHC_VEC, true);
                v = *gptr<const mcraw_u32x4>(row + xs);
            } else {
                RGB_PATH(RP_LD_MHC_ELEM, true);
                uint32_t u[8];
    #pragma unroll
                for (int e = 0; e < 8; e++)
                    u[e] = gptr<const uint16_t>(row)[reflect101(xs + e, W)];
                v = mcraw_u32x4{u[0] | (u[1] << 16), u[2] | (u[3] << 16), u[4] | (u[5] << 16), u[6] | (u[7] << 16)};
            }
            *reinterpret_cast<mcraw_u32x4 *>(&s_t[r * MHC_LW + 8u * q]) = v;
        }
        __syncthreads();
        const uint32_t lx = threadIdx.x & 31u, ly = threadIdx.x >> 5;
        const uint32_t x = static_cast<uint32_t>(x0) + 8u * lx;
        RGB_PATH(RP_IDLE_MHC_LANE, x >= A.W);
        if (x >= A.W)
            continue;
        const uint32_t n = min(8u, A.W - x);
        const RgbCol &col = A.col[A.percol ? f : 0u];
        uint8_t *fout = A.out + static_cast<size_t>(f) * 3u * A.Ho * A.Wo * out_es(PK) / (is_yuv(PK) ? 2u : 1u);
    #pragma unroll 1
        for (uint32_t pass = 0; pass < MHC_TH / 16u; pass++) {
            const uint32_t rp = ly + 8u * pass, y = static_cast<uint32_t>(y0) + 2u * rp;
            RGB_PATH(RP_IDLE_MHC_ROWS, y >= A.H);
            if (y >= A.H)
                break;
            // window: rows y-2 .. y+3, columns x-2 .. x+9, black subtracted: d[r][j] at image (y - 2 + r, x - 2 + j)
            int d[6][12];
    #pragma unroll
            for (int r = 0; r < 6; r++) {
                const uint16_t *lrow = &s_t[(2u * rp + static_cast<uint32_t>(r)) * MHC_LW + 8u * lx];
                const mcraw_u32x4 c0 = *reinterpret_cast<const mcraw_u32x4 *>(lrow);
                const mcraw_u32x4 c1 = *reinterpret_cast<const mcraw_u32x4 *>(lrow + 8);
                const uint32_t c2 = *reinterpret_cast<const uint32_t *>(lrow + 16);
                const uint32_t w[6] = {c0[3], c1[0], c1[1], c1[2], c1[3], c2};
    #pragma unroll
                for (int j = 0; j < 12; j++)
                    d[r][j] = static_cast<int>((w[j >> 1] >> (16u * (j & 1))) & 0xffffu) - A.black[(r & 1) * 2 + (j & 1)];
            }
            int SUM[3][4] = {}; // YUV kinds: the sums of P over the lane's four 2x2 blocks
    #pragma unroll
            for (int a = 0; a < 2; a++) {
                int E[3][8];
    #pragma unroll
                for (int b = 0; b < 8; b++) {
                    const int R = a + 2, J = b + 2;
                    const int C = d[R][J];
                    const int n1 = d[R - 1][J], s1 = d[R + 1][J], w1 = d[R][J - 1], e1 = d[R][J + 1];
                    const int v2 = d[R - 2][J] + d[R + 2][J], h2 = d[R][J - 2] + d[R][J + 2];
                    const int dg = (d[R - 1][J - 1] + d[R - 1][J + 1]) + (d[R + 1][J - 1] + d[R + 1][J + 1]);
                    const int role = (a * 2 + (b & 1)) ^ S;
                    const int nat = 16 * C;
                    if (role == 0 || role == 3) { // R or B site
                        const int g = 8 * C + 4 * ((n1 + s1) + (w1 + e1)) - 2 * (v2 + h2);
                        const int o = 12 * C + 4 * dg - 3 * (v2 + h2);
                        E[0][b] = role == 0 ? nat : o;
                        E[1][b] = g;
                        E[2][b] = role == 0 ? o : nat;
                    } else { // G site: role 1 has R left / right, role 2 has B left / right
                        const int hz = 10 * C + 8 * (w1 + e1) - 2 * h2 - 2 * dg + v2;
                        const int vt = 10 * C + 8 * (n1 + s1) - 2 * v2 - 2 * dg + h2;
                        E[0][b] = role == 1 ? hz : vt;
                        E[1][b] = nat;
                        E[2][b] = role == 1 ? vt : hz;
                    }
                }
                if (y + static_cast<uint32_t>(a) < A.H) {
                    if constexpr (is_yuv(PK)) // (H is even: a row pair always has both rows)
                        yuv_row8<PK>(A, col, s_lut, fout, y + static_cast<uint32_t>(a), x, n, a, E, SUM);
                    else if constexpr (is_disp(PK))
                        disp_store8<PK>(A, col, s_lut, fout, y + static_cast<uint32_t>(a), x, n, E);
                    else
                        rgb_store8<PK>(A, col, fout, y + static_cast<uint32_t>(a), x, n, E);
                }
            }
        }
    } while (DISP && (t += gridDim.x) < A.units * A.nf);
}

// ---- BIN2 -------------------------------------------------------------------------------------------------------------
//
// Lane = 8 consecutive output columns of one output row: 16 input columns of two input rows (two 16-byte loads per row
// where the rows allow it).
// Float kinds: item blockIdx.x * RGB_T + lane of frame blockIdx.y.  Display kinds: persistent, as krgb_mhc.
template <int PK, int S>
__global__ void __launch_bounds__(RGB_T) krgb_bin2(const RgbArgs A)
{
    constexpr bool DISP = is_disp(PK);
    __shared__ __attribute__((aligned(16))) uint16_t s_lut[DISP ? DISP_LDS_MAX : 8u];
    uint32_t t = blockIdx.x;
    RGB_WALK_DECL;
    if constexpr (DISP) {
        stage_lut(A, s_lut);
        __syncthreads();
    }
    do {
        const uint32_t f = DISP ? t / A.units : blockIdx.y, item = (DISP ? t % A.units : blockIdx.x) * RGB_T + threadIdx.x;
        RGB_WALK(RF_BIN2, f, DISP, A.lutg);
        const uint32_t yo = item / A.tilesX, xo = 8u * (item % A.tilesX);
        RGB_PATH(RP_IDLE_BIN2, yo >= A.Ho);
        if (yo >= A.Ho)
            continue;
        const uint32_t n = min(8u, A.Wo - xo);
        const uint16_t *row0 = A.in + static_cast<size_t>(f) * A.fstride + static_cast<size_t>(2u * yo) * A.pitch + 2u * xo;
        const uint16_t *row1 = row0 + A.pitch;
        uint32_t u[2][8]; // (even column | odd column << 16) of quad i, rows 0 and 1
        if (A.invec && n == 8u) {
            RGB_PATH(RP_LD_BIN2_VEC, true);
            const mcraw_u32x4 a0 = gptr<const mcraw_u32x4>(row0)[0], a1 = gptr<const mcraw_u32x4>(row0)[1];
            const mcraw_u32x4 b0 = gptr<const mcraw_u32x4>(row1)[0], b1 = gptr<const mcraw_u32x4>(row1)[1];
    #pragma unroll
            for (int i = 0; i < 4; i++) {
                u[0][i] = a0[i];
                u[0][4 + i] = a1[i];
                u[1][i] = b0[i];
                u[1][4 + i] = b1[i];
            }
        } else {
            RGB_PATH(RP_LD_BIN2_ELEM, true);
    #pragma unroll
            for (uint32_t i = 0; i < 8u; i++) {
                const uint32_t k = i < n ? 2u * i : 0u;
                u[0][i] = gptr<const uint16_t>(row0)[k] | (static_cast<uint32_t>(gptr<const uint16_t>(row0)[k + 1]) << 16);
                u[1][i] = gptr<const uint16_t>(row1)[k] | (static_cast<uint32_t>(gptr<const uint16_t>(row1)[k + 1]) << 16);
            }
        }
        int E[3][8];
    #pragma unroll
        for (int i = 0; i < 8; i++) {
            int q[4];
    #pragma unroll
            for (int p = 0; p < 4; p++)
                q[p] = static_cast<int>((u[p >> 1][i] >> (16u * (p & 1))) & 0xffffu) - A.black[p];
            E[0][i] = 2 * q[0 ^ S];
            E[1][i] = q[1 ^ S] + q[2 ^ S];
            E[2][i] = 2 * q[3 ^ S];
        }
        uint8_t *fout = A.out + static_cast<size_t>(f) * 3u * A.Ho * A.Wo * out_es(PK);
        if constexpr (is_disp(PK))
            disp_store8<PK>(A, A.col[A.percol ? f : 0u], s_lut, fout, yo, xo, n, E);
        else
            rgb_store8<PK>(A, A.col[A.percol ? f : 0u], fout, yo, xo, n, E);
    } while (DISP && (t += gridDim.x) < A.units * A.nf);
}

// The YUV kinds of BIN2: 4:2:0 needs two output rows, so a lane takes 8 output columns of an output row PAIR (four input
// rows), which holds its four 2x2 blocks.  A kernel of its own: the float and display instances of krgb_bin2 keep their
// code and registers.  Persistent, as the display kinds; A.units counts groups of 256 such items per frame.
template <int PK, int S>
__global__ void __launch_bounds__(RGB_T) krgb_bin2y(const RgbArgs A)
{
    static_assert(is_yuv(PK), "the YUV kinds only");
    constexpr uint32_t ROWS = 2u; // output rows per item
    __shared__ __attribute__((aligned(16))) uint16_t s_lut[DISP_LDS_MAX];
    uint32_t t = blockIdx.x;
    RGB_WALK_DECL;
    stage_lut(A, s_lut);
    __syncthreads();
    do {
        const uint32_t f = t / A.units, item = (t % A.units) * RGB_T + threadIdx.x;
        RGB_WALK(RF_BIN2Y, f, true, A.lutg);
        const uint32_t yo = item / A.tilesX * ROWS, xo = 8u * (item % A.tilesX);
        RGB_PATH(RP_IDLE_BIN2, yo >= A.Ho);
        if (yo >= A.Ho)
            continue;
        const uint32_t n = min(8u, A.Wo - xo);
        int SUM[3][4] = {}; // the sums of P over the lane's four 2x2 blocks
    #pragma unroll
        for (uint32_t a = 0; a < ROWS; a++) { // (krgb_bin2's load and quads, written out in both: DESIGN 22)
            const uint16_t *row0 = A.in + static_cast<size_t>(f) * A.fstride + static_cast<size_t>(2u * (yo + a)) * A.pitch + 2u * xo;
            const uint16_t *row1 = row0 + A.pitch;
            uint32_t u[2][8]; // (even column | odd column << 16) of quad i, rows 0 and 1
            if (A.invec && n == 8u) {
                RGB_PATH(RP_LD_BIN2Y_VEC, true);
                const mcraw_u32x4 a0 = gptr<const mcraw_u32x4>(row0)[0], a1 = gptr<const mcraw_u32x4>(row0)[1];
                const mcraw_u32x4 b0 = gptr<const mcraw_u32x4>(row1)[0], b1 = gptr<const mcraw_u32x4>(row1)[1];
    #pragma unroll
                for (int i = 0; i < 4; i++) {
                    u[0][i] = a0[i];
                    u[0][4 + i] = a1[i];
                    u[1][i] = b0[i];
                    u[1][4 + i] = b1[i];
                }
            } else {
                RGB_PATH(RP_LD_BIN2Y_ELEM, true);
    #pragma unroll
                for (uint32_t i = 0; i < 8u; i++) {
                    const uint32_t k = i < n ? 2u * i : 0u;
                    u[0][i] = gptr<const uint16_t>(row0)[k] | (static_cast<uint32_t>(gptr<const uint16_t>(row0)[k + 1]) << 16);
                    u[1][i] = gptr<const uint16_t>(row1)[k] | (static_cast<uint32_t>(gptr<const uint16_t>(row1)[k + 1]) << 16);
                }
            }
            int E[3][8];
    #pragma unroll
            for (int i = 0; i < 8; i++) {
                int q[4];
    #pragma unroll
                for (int p = 0; p < 4; p++)
                    q[p] = static_cast<int>((u[p >> 1][i] >> (16u * (p & 1))) & 0xffffu) - A.black[p];
                E[0][i] = 2 * q[0 ^ S];
                E[1][i] = q[1 ^ S] + q[2 ^ S];
                E[2][i] = 2 * q[3 ^ S];
            }
            uint8_t *fout = A.out + static_cast<size_t>(f) * 3u * A.Ho * A.Wo * out_es(PK) / ROWS;
            yuv_row8<PK>(A, A.col[A.percol ? f : 0u], s_lut, fout, yo + a, xo, n, static_cast<int>(a), E, SUM);
        }
    } while ((t += gridDim.x) < A.units * A.nf);
}

struct MhcK {
    template <int PK, int S>
    static auto at() { return &krgb_mhc<PK, S>; }
};

struct Bin2K { // (the YUV kinds have a kernel of their own)
    template <int PK, int S>
    static auto at()
    {
        if constexpr (is_yuv(PK))
            return &krgb_bin2y<PK, S>;
        else
            return &krgb_bin2<PK, S>;
    }
};

// krgb_ha's launches (csrc/mcraw_ha.hip)
int ha_launch(mcraw_ctx *c, const RgbArgs &A, const RgbPlan &P, const std::vector<RgbCol> &cols, const uint16_t *in, int n, void *out,
              hipStream_t st);

// The three entry points: rgb_check (mcraw_rgb_args.h) decides about the call and plans it -- `d` given: the display stage, `yv`:
// the YUV stage (never both) --, then the launches.
static int demosaic_launch(const char *fn, mcraw_ctx *c, const mcraw_rgb *p, const mcraw_display *d, const mcraw_yuv *yv,
                           const mcraw_rgb_color *colors, int ncolors, const uint16_t *in, size_t in_pitch,
                           size_t in_frame_stride, int width, int height, int n, void *out, size_t out_bytes, void *stream)
{
    RgbPlan P;
    const char *why = c ? rgb_check(p, d, yv, colors, ncolors, in, in_pitch, in_frame_stride, width, height, n, out, out_bytes, P)
                        : "bad arguments";
    if (why)
        return reject(fn, why);
    if (P.noop)
        return 0;

    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    RgbArgs A = rgb_args(p, d, yv, in_pitch, in_frame_stride, width, height, ncolors);
    A.Wo = static_cast<uint32_t>(P.Wo);
    A.Ho = static_cast<uint32_t>(P.Ho);
    A.tilesX = P.tilesX;
    A.units = P.units;
    A.invec = P.invec;
    if (P.ha) // the edge-directed demosaic: MHC's geometry, estimates in 1/32 (csrc/mcraw_ha.hip)
        return ha_launch(c, A, P, rgb_cols(p, colors, ncolors, 0.03125f), in, n, out, stream_of(c, stream));
    return rgb_launch(c, P.mhc ? rgb_pick<MhcK>(P) : rgb_pick<Bin2K>(P), A, P, rgb_cols(p, colors, ncolors, P.mhc ? 0.0625f : 0.5f), in, n,
                      out, P.mhc ? MCRAW_KRGB_MHC : MCRAW_KRGB_BIN2, stream_of(c, stream));
}

// What a persistent grid may hold, for a demosaic unit that names no switch of a test build (csrc/mcraw_warp.hip): this source's
// RGB_GRID_LIMIT, so that a build with a capped grid caps that unit's grid as well.
uint32_t rgb_grid_limit(uint32_t resident) { return RGB_GRID_LIMIT(resident); }

} // namespace mcraw

using namespace mcraw;

extern "C" {

#ifdef MCRAW_PATHSR
// The census of the demosaic kernels, in the order of RgbPath, summed over the three sources (up to n counters; returns how many
// there are); `reset`: and start it over.
int mcraw_diag_rgb_paths(uint64_t *out, int n, int reset) { return census_sum<RgbPath, RP_N>(out, n, reset); }
#endif

int mcraw_demosaic_batch(mcraw_ctx *c, const mcraw_rgb *p, const mcraw_rgb_color *colors, int ncolors, const uint16_t *in,
                         size_t in_pitch, size_t in_frame_stride, int width, int height, int n, void *out, size_t out_bytes,
                         void *stream)
{
    return demosaic_launch("mcraw_demosaic_batch", c, p, nullptr, nullptr, colors, ncolors, in, in_pitch, in_frame_stride, width, height,
                           n, out, out_bytes, stream);
}

int mcraw_demosaic_display_batch(mcraw_ctx *c, const mcraw_rgb *p, const mcraw_display *d, const mcraw_rgb_color *colors,
                                 int ncolors, const uint16_t *in, size_t in_pitch, size_t in_frame_stride, int width, int height,
                                 int n, void *out, size_t out_bytes, void *stream)
{
    if (!d)
        return reject("mcraw_demosaic_display_batch", "bad arguments");
    return demosaic_launch("mcraw_demosaic_display_batch", c, p, d, nullptr, colors, ncolors, in, in_pitch, in_frame_stride,
                           width, height, n, out, out_bytes, stream);
}

int mcraw_demosaic_yuv_batch(mcraw_ctx *c, const mcraw_rgb *p, const mcraw_yuv *y, const mcraw_rgb_color *colors, int ncolors,
                             const uint16_t *in, size_t in_pitch, size_t in_frame_stride, int width, int height, int n,
                             void *out, size_t out_bytes, void *stream)
{
    if (!y)
        return reject("mcraw_demosaic_yuv_batch", "bad arguments");
    return demosaic_launch("mcraw_demosaic_yuv_batch", c, p, nullptr, y, colors, ncolors, in, in_pitch, in_frame_stride, width,
                           height, n, out, out_bytes, stream);
}

} // extern "C"
