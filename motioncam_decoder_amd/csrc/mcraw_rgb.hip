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
//   krgb_area  any size from 1/16 of the crop's quads to all of them: the area average of the quads under a pixel's footprint
//              (mcraw_demosaic_area_batch, behind the three entry points below; tests/_area_ref.py states it in numpy)
#include "mcraw_dev.h"
#include "mcraw_host.h"
#include "mcraw_rgb_args.h"
#include "mcraw_rgb_dev.h"
#include "mcraw_area_args.h"

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
    if constexpr (DISP)
        stage_lut(A, s_lut);
    do {
        if constexpr (DISP)
            __syncthreads(); // the LUT is staged; the previous tile's LDS reads are done
        const uint32_t f = DISP ? t / A.units : blockIdx.y, u = DISP ? t % A.units : blockIdx.x;
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
                v = *gptr<const mcraw_u32x4>(row + xs);
            } else {
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
        if (x >= A.W)
            continue;
        const uint32_t n = min(8u, A.W - x);
        const RgbCol &col = A.col[A.percol ? f : 0u];
        uint8_t *fout = A.out + static_cast<size_t>(f) * 3u * A.Ho * A.Wo * out_es(PK) / (is_yuv(PK) ? 2u : 1u);
    #pragma unroll 1
        for (uint32_t pass = 0; pass < MHC_TH / 16u; pass++) {
            const uint32_t rp = ly + 8u * pass, y = static_cast<uint32_t>(y0) + 2u * rp;
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
    if constexpr (DISP) {
        stage_lut(A, s_lut);
        __syncthreads();
    }
    do {
        const uint32_t f = DISP ? t / A.units : blockIdx.y, item = (DISP ? t % A.units : blockIdx.x) * RGB_T + threadIdx.x;
        const uint32_t yo = item / A.tilesX, xo = 8u * (item % A.tilesX);
        if (yo >= A.Ho)
            continue;
        const uint32_t n = min(8u, A.Wo - xo);
        const uint16_t *row0 = A.in + static_cast<size_t>(f) * A.fstride + static_cast<size_t>(2u * yo) * A.pitch + 2u * xo;
        const uint16_t *row1 = row0 + A.pitch;
        uint32_t u[2][8]; // (even column | odd column << 16) of quad i, rows 0 and 1
        if (A.invec && n == 8u) {
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
    stage_lut(A, s_lut);
    __syncthreads();
    do {
        const uint32_t f = t / A.units, item = (t % A.units) * RGB_T + threadIdx.x;
        const uint32_t yo = item / A.tilesX * ROWS, xo = 8u * (item % A.tilesX);
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

typedef void (*RgbKernel)(const RgbArgs);

template <int PK>
static RgbKernel pick_kernel(bool mhc, int s)
{
    static const RgbKernel tile[4] = {krgb_mhc<PK, 0>, krgb_mhc<PK, 1>, krgb_mhc<PK, 2>, krgb_mhc<PK, 3>};
    if (mhc)
        return tile[s];
    if constexpr (is_yuv(PK)) {
        static const RgbKernel bin2[4] = {krgb_bin2y<PK, 0>, krgb_bin2y<PK, 1>, krgb_bin2y<PK, 2>, krgb_bin2y<PK, 3>};
        return bin2[s];
    } else {
        static const RgbKernel bin2[4] = {krgb_bin2<PK, 0>, krgb_bin2<PK, 1>, krgb_bin2<PK, 2>, krgb_bin2<PK, 3>};
        return bin2[s];
    }
}

static RgbKernel pick_kernel(const RgbPlan &P)
{
    switch (P.kind) {
    case PK_F32: return pick_kernel<PK_F32>(P.mhc, P.shift);
    case PK_F16: return pick_kernel<PK_F16>(P.mhc, P.shift);
    case PK_BF16: return pick_kernel<PK_BF16>(P.mhc, P.shift);
    case PK_DISP8: return pick_kernel<PK_DISP8>(P.mhc, P.shift);
    case PK_DISP16: return pick_kernel<PK_DISP16>(P.mhc, P.shift);
    case PK_NV12: return pick_kernel<PK_NV12>(P.mhc, P.shift);
    default: return pick_kernel<PK_P010>(P.mhc, P.shift);
    }
}

// Workgroups of a persistent display grid: what the device holds at once (compute units x resident workgroups of the
// instance), found once per (device, kernel).
static uint32_t resident_groups(int device, RgbKernel k)
{
    static std::mutex mu;
    static std::vector<std::pair<std::pair<int, RgbKernel>, uint32_t>> seen;
    std::lock_guard<std::mutex> lk(mu);
    for (const auto &e : seen)
        if (e.first.first == device && e.first.second == k)
            return e.second;
    int cus = 0, per = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0)
        cus = 256;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, reinterpret_cast<const void *>(k), RGB_T, 0) != hipSuccess || per <= 0)
        per = 2;
    const uint32_t g = static_cast<uint32_t>(cus) * static_cast<uint32_t>(per);
    seen.push_back({{device, k}, g});
    return g;
}

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
    hipStream_t st = stream ? static_cast<hipStream_t>(stream) : c->stream;
    // (the division is in f32, as every step of the host side of the contract)
    const float bsum = static_cast<float>(static_cast<int>(p->black[0]) + p->black[1] + p->black[2] + p->black[3]);
    const float inv = 1.0f / (p->white - 0.25f * bsum);
    const float scale = P.mhc ? 0.0625f : 0.5f;
    std::vector<RgbCol> cols(static_cast<size_t>(ncolors));
    for (int i = 0; i < ncolors; i++) {
        for (int k = 0; k < 3; k++)
            cols[static_cast<size_t>(i)].k[k] = (colors[i].gain[k] * inv) * scale;
        std::memcpy(cols[static_cast<size_t>(i)].m, colors[i].m, sizeof(float) * 9);
    }
    RgbKernel k = pick_kernel(P);
    RgbArgs A{};
    A.pitch = in_pitch;
    A.fstride = in_frame_stride;
    A.W = static_cast<uint32_t>(width);
    A.H = static_cast<uint32_t>(height);
    A.Wo = static_cast<uint32_t>(P.Wo);
    A.Ho = static_cast<uint32_t>(P.Ho);
    A.tilesX = P.tilesX;
    A.units = P.units;
    A.invec = P.invec;
    A.clip = (p->flags & MCRAW_FLOAT_CLIP) ? 1u : 0u;
    A.percol = ncolors > 1 ? 1u : 0u;
    if (d || yv) {
        A.lut = d ? d->lut : yv->lut;
        A.lutn = 1u << (d ? d->lut_log2 : yv->lut_log2);
        A.lutg = A.lutn > DISP_LDS_MAX ? 1u : 0u;
        A.hwc = d && d->layout == MCRAW_DISP_HWC ? 1u : 0u;
    }
    if (yv) {
        for (int i = 0; i < 3; i++) {
            A.ycf[i] = yv->cy[i];
            A.ycf[3 + i] = yv->cb[i];
            A.ycf[6 + i] = yv->cr[i];
        }
        A.ymask = (1u << yv->in_bits) - 1u;
        A.ysh = yv->sh;
        A.yoff = yv->y_off;
        A.coff = yv->c_off;
    }
    for (int i = 0; i < 4; i++)
        A.black[i] = p->black[i];
    const bool persistent = has_lut(P.kind);
    const uint32_t resident = persistent ? resident_groups(c->device, k) : 0u;
    const int kid = P.mhc ? MCRAW_KRGB_MHC : MCRAW_KRGB_BIN2;
    const int piece = A.percol ? RGB_MAXF : 65535;
    for (int f0 = 0; f0 < n; f0 += piece) {
        const int nf = std::min(piece, n - f0);
        A.in = in + static_cast<size_t>(f0) * in_frame_stride;
        A.out = static_cast<uint8_t *>(out) + static_cast<size_t>(f0) * P.out_frame;
        A.nf = static_cast<uint32_t>(nf);
        for (int i = 0; i < (A.percol ? nf : 1); i++)
            A.col[i] = cols[static_cast<size_t>(A.percol ? f0 + i : 0)];
        // display and YUV kinds: a persistent grid of at most what the device holds at once, over units x nf units of work
        const dim3 grid = persistent ? dim3(static_cast<uint32_t>(std::min<uint64_t>(static_cast<uint64_t>(P.units) * nf, resident)))
                            : dim3(P.units, static_cast<uint32_t>(nf));
        KTimer kt(c, kid, st);
        hipLaunchKernelGGL(k, grid, dim3(RGB_T), 0, st, A);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}


// ---- AREA -------------------------------------------------------------------------------------------------------------
//
// mcraw_demosaic_area_batch: an output pixel is the area average of the CFA quads under its footprint (the contract and its
// weights: include/mcraw_hip.h; the plan: mcraw_area_args.h; the numpy statement: tests/_area_ref.py).  karea_tab writes the
// per-column and per-row taps into the caller's scratch; krgb_area, queued behind it, reads them.
//
// A lane owns 8 consecutive output columns of an output row pair, as in krgb_bin2y, so one body feeds all three families.  A
// workgroup is lx lanes side by side times ly row pairs (the plan's choice: as wide as the LDS tile allows, then as high).  A
// unit of work is one column tile of AREA_BAND groups of ly row pairs: the horizontal weights of the tile's columns are staged
// in LDS once per unit (s_wx, [tap][column in lane][lane]: consecutive lanes read consecutive entries).  For each of a
// row's at most 17 quad rows the workgroup stages the span of quads under the tile, for each of its row pairs, in LDS (s_q:
// a quad is {row 0 dword, row 1 dword}; one pad slot behind every 8 quads, which spreads the lanes' strides of 8 * ratio
// quads over the banks), each lane forms t for its 8 columns from it and adds wy * t to its 24 sums.
// Horizontal sums run over the raw samples: the weights of a pixel add up to 256 exactly, so
// sum w (s - black) = sum w s - 256 black.
struct AreaGeo {
    const AreaTap *xt, *yt;
    uint32_t qx0, qy0; // the crop's origin in quads
    uint32_t QW;       // quads in a row of the frame
    uint32_t mode;     // AreaPlan::mode
    uint32_t lxl, ly, segp, nch, nchm;
    uint32_t ntx, nty;
    uint32_t tilesX, groups;
};

__global__ void __launch_bounds__(RGB_T) karea_tab(AreaTap *xt, AreaTap *yt, uint32_t Qw, uint32_t Ow, uint32_t Qh, uint32_t Oh)
{
    const uint32_t i = blockIdx.x * RGB_T + threadIdx.x;
    AreaTap t;
    if (i < Ow) {
        area_taps(i, Qw, Ow, t);
        xt[i] = t;
    } else if (i - Ow < Oh) {
        area_taps(i - Ow, Qh, Oh, t);
        yt[i - Ow] = t;
    }
}

template <int PK, int S>
__global__ void __launch_bounds__(RGB_T) krgb_area(const RgbArgs A, const AreaGeo G)
{
    constexpr bool LUT = has_lut(PK);
    __shared__ __attribute__((aligned(16))) mcraw_u32x2 s_q[AREA_TILE_Q];
    __shared__ uint16_t s_wx[AREA_WXN];
    __shared__ uint32_t s_y[AREA_YN];
    __shared__ __attribute__((aligned(16))) uint16_t s_lut[LUT ? DISP_LDS_MAX : 8u];
    uint32_t t = blockIdx.x;
    if constexpr (LUT)
        stage_lut(A, s_lut);
    const uint32_t lx = 1u << G.lxl, lxid = threadIdx.x & (lx - 1u), lyid = threadIdx.x >> G.lxl;
    const bool lane_on = lyid < G.ly;
    do {
        const uint32_t f = LUT ? t / A.units : blockIdx.y, u = LUT ? t % A.units : blockIdx.x;
        const uint32_t tx = u % G.tilesX, band = u / G.tilesX;
        const uint32_t k0 = (tx * 8u) << G.lxl, xo = k0 + 8u * lxid;
        const uint32_t n = xo < A.Wo ? min(8u, A.Wo - xo) : 0u;
        const uint32_t qb = (G.qx0 + G.xt[k0].q0) & ~7u; // the segment's first quad column in the frame: on the 32-byte grid
        const uint16_t *in = A.in + static_cast<size_t>(f) * A.fstride;
        __syncthreads(); // the LUT is staged; the previous unit's LDS reads are done
        for (uint32_t e = threadIdx.x; e < ((8u * G.ntx) << G.lxl); e += RGB_T) {
            const uint32_t tp = e >> (3u + G.lxl), cc = e & (8u * lx - 1u), k = k0 + cc;
            s_wx[((tp * 8u + (cc & 7u)) << G.lxl) + (cc >> 3)] = k < A.Wo ? gptr<const uint16_t>(G.xt[k].w)[tp] : uint16_t{0};
        }
        uint32_t qn[8]; // per column: first quad relative to qb | taps << 16
    #pragma unroll
        for (uint32_t i = 0; i < 8u; i++) {
            qn[i] = 0u;
            if (lane_on && i < n)
                qn[i] = (G.qx0 + G.xt[xo + i].q0 - qb) | (static_cast<uint32_t>(G.xt[xo + i].nt) << 16);
        }
        const RgbCol &col = A.col[A.percol ? f : 0u];
        uint8_t *fout = A.out + static_cast<size_t>(f) * 3u * A.Ho * A.Wo * out_es(PK) / (is_yuv(PK) ? 2u : 1u);
        const mcraw_u32x2 *tile = s_q + lyid * G.segp;
    #pragma unroll 1
        for (uint32_t g = 0; g < AREA_BAND; g++) {
            const uint32_t grp = band * AREA_BAND + g;
            if (grp >= G.groups)
                break;
            const uint32_t rp0 = grp * G.ly;
            __syncthreads(); // the previous group's reads of s_y are done
            for (uint32_t e = threadIdx.x; e < 2u * G.ly; e += RGB_T) {
                const uint32_t j = 2u * rp0 + e;
                s_y[e] = j < A.Ho ? (G.yt[j].q0 | (static_cast<uint32_t>(G.yt[j].nt) << 24)) : 0u;
            }
            int SUM[3][4] = {}; // YUV kinds: the sums of P over the lane's four 2x2 blocks
    #pragma unroll 1
            for (uint32_t a = 0; a < 2u; a++) {
                const uint32_t j = 2u * (rp0 + lyid) + a;
                const bool row_on = lane_on && n != 0u && j < A.Ho;
                int acc[3][8] = {};
    #pragma unroll 1
                for (uint32_t s = 0; s < G.nty; s++) {
                    const int wy = row_on ? static_cast<int>(gptr<const uint16_t>(G.yt[j].w)[s]) : 0;
                    __syncthreads(); // s_y is written; the previous step's reads of the tile are done
                    for (uint32_t c = threadIdx.x; c < G.ly * G.nch; c += RGB_T) {
                        const uint32_t lyc = __umulhi(c, G.nchm), ch = c - lyc * G.nch;
                        const uint32_t yy = s_y[2u * lyc + a];
                        if (s >= (yy >> 24))
                            continue;
                        const uint32_t qy = G.qy0 + (yy & 0xffffffu) + s, aq = qb + 4u * ch;
                        const uint16_t *row0 = in + static_cast<size_t>(2u * qy) * A.pitch + 2u * static_cast<size_t>(aq);
                        const uint16_t *row1 = row0 + A.pitch;
                        uint32_t r0[4], r1[4];
                        if (G.mode == 2u && aq + 4u <= G.QW) {
                            const mcraw_u32x4 v0 = *gptr<const mcraw_u32x4>(row0), v1 = *gptr<const mcraw_u32x4>(row1);
    #pragma unroll
                            for (int e = 0; e < 4; e++)
                                r0[e] = v0[e], r1[e] = v1[e];
                        } else {
    #pragma unroll
                            for (uint32_t e = 0; e < 4u; e++) {
                                r0[e] = r1[e] = 0u;
                                if (aq + e < G.QW) {
                                    if (G.mode != 0u) {
                                        r0[e] = gptr<const uint32_t>(row0)[e];
                                        r1[e] = gptr<const uint32_t>(row1)[e];
                                    } else {
                                        r0[e] = gptr<const uint16_t>(row0)[2u * e] | (static_cast<uint32_t>(gptr<const uint16_t>(row0)[2u * e + 1u]) << 16);
                                        r1[e] = gptr<const uint16_t>(row1)[2u * e] | (static_cast<uint32_t>(gptr<const uint16_t>(row1)[2u * e + 1u]) << 16);
                                    }
                                }
                            }
                        }
                        mcraw_u32x2 *dst = s_q + lyc * G.segp + 4u * ch + (ch >> 1); // (4 ch) + (4 ch >> 3): a piece never straddles a pad slot
    #pragma unroll
                        for (int e = 0; e < 4; e++)
                            dst[e] = mcraw_u32x2{r0[e], r1[e]};
                    }
                    __syncthreads();
                    if (wy == 0)
                        continue;
    #pragma unroll
                    for (uint32_t i = 0; i < 8u; i++) {
                        const uint32_t rel = qn[i] & 0xffffu, nt = qn[i] >> 16;
                        uint32_t h[4] = {0u, 0u, 0u, 0u}; // sum of w * sample, by CFA position
                        for (uint32_t tp = 0; tp < nt; tp++) {
                            const uint32_t idx = rel + tp;
                            const mcraw_u32x2 q = tile[idx + (idx >> 3)];
                            const uint32_t w = s_wx[((tp * 8u + i) << G.lxl) + lxid];
                            h[0] += __umul24(w, q[0] & 0xffffu);
                            h[1] += __umul24(w, q[0] >> 16);
                            h[2] += __umul24(w, q[1] & 0xffffu);
                            h[3] += __umul24(w, q[1] >> 16);
                        }
                        int d[4];
    #pragma unroll
                        for (int p = 0; p < 4; p++)
                            d[p] = static_cast<int>(h[p]) - 256 * A.black[p];
                        const int hc[3] = {2 * d[0 ^ S], d[1 ^ S] + d[2 ^ S], 2 * d[3 ^ S]};
    #pragma unroll
                        for (int c = 0; c < 3; c++)
                            acc[c][i] += __mul24(wy, (hc[c] + 8) >> 4);
                    }
                }
                if (!row_on)
                    continue;
                int E[3][8];
    #pragma unroll
                for (int c = 0; c < 3; c++)
    #pragma unroll
                    for (int i = 0; i < 8; i++)
                        E[c][i] = (acc[c][i] + 128) >> 8;
                if constexpr (is_yuv(PK)) // (Ho is even: a row pair always has both rows)
                    yuv_row8<PK>(A, col, s_lut, fout, j, xo, n, static_cast<int>(a), E, SUM);
                else if constexpr (is_disp(PK))
                    disp_store8<PK>(A, col, s_lut, fout, j, xo, n, E);
                else
                    rgb_store8<PK>(A, col, fout, j, xo, n, E);
            }
        }
    } while (LUT && (t += gridDim.x) < A.units * A.nf);
}

typedef void (*AreaKernel)(const RgbArgs, const AreaGeo);

template <int PK>
static AreaKernel pick_area(int s)
{
    static const AreaKernel k[4] = {krgb_area<PK, 0>, krgb_area<PK, 1>, krgb_area<PK, 2>, krgb_area<PK, 3>};
    return k[s];
}

static AreaKernel pick_area(const RgbPlan &P)
{
    switch (P.kind) {
    case PK_F32: return pick_area<PK_F32>(P.shift);
    case PK_F16: return pick_area<PK_F16>(P.shift);
    case PK_BF16: return pick_area<PK_BF16>(P.shift);
    case PK_DISP8: return pick_area<PK_DISP8>(P.shift);
    case PK_DISP16: return pick_area<PK_DISP16>(P.shift);
    case PK_NV12: return pick_area<PK_NV12>(P.shift);
    default: return pick_area<PK_P010>(P.shift);
    }
}

// Workgroups of a persistent area grid that the device holds at once, found once per (device, kernel), as resident_groups.
static uint32_t resident_area_groups(int device, AreaKernel k)
{
    static std::mutex mu;
    static std::vector<std::pair<std::pair<int, AreaKernel>, uint32_t>> seen;
    std::lock_guard<std::mutex> lk(mu);
    for (const auto &e : seen)
        if (e.first.first == device && e.first.second == k)
            return e.second;
    int cus = 0, per = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0)
        cus = 256;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, reinterpret_cast<const void *>(k), RGB_T, 0) != hipSuccess || per <= 0)
        per = 2;
    const uint32_t g = static_cast<uint32_t>(cus) * static_cast<uint32_t>(per);
    seen.push_back({{device, k}, g});
    return g;
}

static int area_launch(mcraw_ctx *c, const mcraw_rgb *p, const mcraw_area *a, const mcraw_display *d, const mcraw_yuv *yv,
                       const mcraw_rgb_color *colors, int ncolors, const uint16_t *in, size_t in_pitch, size_t in_frame_stride,
                       int width, int height, int n, void *work, const AreaPlan &P, void *out, hipStream_t st)
{
    // (the division is in f32, as every step of the host side of the contract)
    const float bsum = static_cast<float>(static_cast<int>(p->black[0]) + p->black[1] + p->black[2] + p->black[3]);
    const float inv = 1.0f / (p->white - 0.25f * bsum);
    std::vector<RgbCol> cols(static_cast<size_t>(ncolors));
    for (int i = 0; i < ncolors; i++) {
        for (int k = 0; k < 3; k++)
            cols[static_cast<size_t>(i)].k[k] = (colors[i].gain[k] * inv) * 0.03125f;
        std::memcpy(cols[static_cast<size_t>(i)].m, colors[i].m, sizeof(float) * 9);
    }
    AreaKernel k = pick_area(P.rgb);
    RgbArgs A{};
    A.pitch = in_pitch;
    A.fstride = in_frame_stride;
    A.W = static_cast<uint32_t>(width);
    A.H = static_cast<uint32_t>(height);
    A.Wo = static_cast<uint32_t>(P.rgb.Wo);
    A.Ho = static_cast<uint32_t>(P.rgb.Ho);
    A.tilesX = P.tilesX;
    A.units = P.units;
    A.invec = P.mode == 2u;
    A.clip = (p->flags & MCRAW_FLOAT_CLIP) ? 1u : 0u;
    A.percol = ncolors > 1 ? 1u : 0u;
    if (d || yv) {
        A.lut = d ? d->lut : yv->lut;
        A.lutn = 1u << (d ? d->lut_log2 : yv->lut_log2);
        A.lutg = A.lutn > DISP_LDS_MAX ? 1u : 0u;
        A.hwc = d && d->layout == MCRAW_DISP_HWC ? 1u : 0u;
    }
    if (yv) {
        for (int i = 0; i < 3; i++) {
            A.ycf[i] = yv->cy[i];
            A.ycf[3 + i] = yv->cb[i];
            A.ycf[6 + i] = yv->cr[i];
        }
        A.ymask = (1u << yv->in_bits) - 1u;
        A.ysh = yv->sh;
        A.yoff = yv->y_off;
        A.coff = yv->c_off;
    }
    for (int i = 0; i < 4; i++)
        A.black[i] = p->black[i];
    AreaGeo G{};
    G.xt = reinterpret_cast<const AreaTap *>(static_cast<const char *>(work) + P.xtab);
    G.yt = reinterpret_cast<const AreaTap *>(static_cast<const char *>(work) + P.ytab);
    G.qx0 = a->x0 / 2u, G.qy0 = a->y0 / 2u;
    G.QW = static_cast<uint32_t>(width) / 2u;
    G.mode = P.mode;
    G.lxl = P.lx_log2, G.ly = P.ly, G.segp = P.segp, G.nch = P.nch, G.nchm = P.nch_magic;
    G.ntx = P.ntx, G.nty = P.nty;
    G.tilesX = P.tilesX, G.groups = P.groups;
    hipLaunchKernelGGL(karea_tab, dim3((A.Wo + A.Ho + RGB_T - 1u) / RGB_T), dim3(RGB_T), 0, st, const_cast<AreaTap *>(G.xt),
                       const_cast<AreaTap *>(G.yt), P.Qw, A.Wo, P.Qh, A.Ho);
    HIP_TRY(hipGetLastError());
    const bool persistent = has_lut(P.rgb.kind);
    const uint32_t resident = persistent ? resident_area_groups(c->device, k) : 0u;
    const int piece = A.percol ? RGB_MAXF : 65535;
    for (int f0 = 0; f0 < n; f0 += piece) {
        const int nf = std::min(piece, n - f0);
        A.in = in + static_cast<size_t>(f0) * in_frame_stride;
        A.out = static_cast<uint8_t *>(out) + static_cast<size_t>(f0) * P.rgb.out_frame;
        A.nf = static_cast<uint32_t>(nf);
        for (int i = 0; i < (A.percol ? nf : 1); i++)
            A.col[i] = cols[static_cast<size_t>(A.percol ? f0 + i : 0)];
        const dim3 grid = persistent ? dim3(static_cast<uint32_t>(std::min<uint64_t>(static_cast<uint64_t>(P.units) * nf, resident)))
                                     : dim3(P.units, static_cast<uint32_t>(nf));
        hipLaunchKernelGGL(k, grid, dim3(RGB_T), 0, st, A, G);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

} // namespace mcraw

using namespace mcraw;

extern "C" {

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

size_t mcraw_area_work_bytes(const mcraw_area *a)
{
    AreaPlan P;
    if (!a || P.geometry(a))
        return 0u;
    return P.total;
}

int mcraw_demosaic_area_batch(mcraw_ctx *c, const mcraw_rgb *p, const mcraw_area *a, const mcraw_display *d, const mcraw_yuv *y,
                              const mcraw_rgb_color *colors, int ncolors, const uint16_t *in, size_t in_pitch, size_t in_frame_stride,
                              int width, int height, int n, void *work, size_t work_bytes, void *out, size_t out_bytes, void *stream)
{
    AreaPlan P;
    const char *why = c ? area_check(p, a, d, y, colors, ncolors, in, in_pitch, in_frame_stride, width, height, n, work, work_bytes, out,
                                     out_bytes, P)
                        : "bad arguments";
    if (why)
        return reject("mcraw_demosaic_area_batch", why);
    if (P.rgb.noop)
        return 0;
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    return area_launch(c, p, a, d, y, colors, ncolors, in, in_pitch, in_frame_stride, width, height, n, work, P, out, stream_of(c, stream));
}

} // extern "C"
