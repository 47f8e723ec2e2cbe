// mcraw_area.hip -- gfx950 kernels for uint16 mosaics resident in HBM -> RGB of any size from 1/16 of a crop window's quads to
// all of them (mcraw_demosaic_area_batch), into the float, display and YUV families.  The colour stage and the stores are the
// siblings' (mcraw_rgb_dev.h), the host side of the launch theirs too (mcraw_rgb_launch.h).
//
//   karea_tab  the taps of every output column and row, into the caller's scratch, queued in front
//   krgb_area  one instance per (output kind, CFA), as the siblings
#ifdef MCRAW_PATHSR // (the test builds' three switches: the head of mcraw_rgb.hip)
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
#include "mcraw_area_args.h"

namespace mcraw {

// An output pixel is the area average of the CFA quads under its footprint (the contract and its
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
    RGB_WALK_DECL;
    if constexpr (LUT)
        stage_lut(A, s_lut);
    const uint32_t lx = 1u << G.lxl, lxid = threadIdx.x & (lx - 1u), lyid = threadIdx.x >> G.lxl;
    const bool lane_on = lyid < G.ly;
    do {
        const uint32_t f = LUT ? t / A.units : blockIdx.y, u = LUT ? t % A.units : blockIdx.x;
        RGB_WALK(RF_AREA, f, LUT, A.lutg);
        const uint32_t tx = u % G.tilesX, band = u / G.tilesX;
        const uint32_t k0 = (tx * 8u) << G.lxl, xo = k0 + 8u * lxid;
        const uint32_t n = xo < A.Wo ? min(8u, A.Wo - xo) : 0u;
        const uint32_t qb = (G.qx0 + G.xt[k0].q0) & ~7u; // the segment's first quad column in the frame: on the 32-byte grid
        const uint16_t *in = A.in + static_cast<size_t>(f) * A.fstride;
        __syncthreads(); // the LUT is staged; the previous unit's LDS reads are done
#ifdef MCRAW_POISON_RGB
        rgb_poison(s_q, sizeof(s_q), 0x5a5a5a5bu);
        rgb_poison(s_wx, sizeof(s_wx), 0x5a5a5a5bu);
        rgb_poison(s_y, sizeof(s_y), 0x01000001u); // (one tap from quad row 1: a stale entry would still read inside the frame)
        __syncthreads();
#endif
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
                RGB_PATH(RP_IDLE_AREA, !row_on);
                int acc[3][8] = {};
    #pragma unroll 1
                for (uint32_t s = 0; s < G.nty; s++) {
                    const int wy = row_on ? static_cast<int>(gptr<const uint16_t>(G.yt[j].w)[s]) : 0;
                    __syncthreads(); // s_y is written; the previous step's reads of the tile are done
                    for (uint32_t c = threadIdx.x; c < G.ly * G.nch; c += RGB_T) {
                        const uint32_t lyc = __umulhi(c, G.nchm), ch = c - lyc * G.nch;
                        const uint32_t yy = s_y[2u * lyc + a];
                        RGB_PATH(RP_LD_AREA_SKIP, s >= (yy >> 24));
                        if (s >= (yy >> 24))
                            continue;
                        const uint32_t qy = G.qy0 + (yy & 0xffffffu) + s, aq = qb + 4u * ch;
                        const uint16_t *row0 = in + static_cast<size_t>(2u * qy) * A.pitch + 2u * static_cast<size_t>(aq);
                        const uint16_t *row1 = row0 + A.pitch;
                        uint32_t r0[4], r1[4];
                        if (G.mode == 2u && aq + 4u <= G.QW) {
                            RGB_PATH(RP_LD_AREA_M2, true);
                            const mcraw_u32x4 v0 = *gptr<const mcraw_u32x4>(row0), v1 = *gptr<const mcraw_u32x4>(row1);
    #pragma unroll
                            for (int e = 0; e < 4; e++)
                                r0[e] = v0[e], r1[e] = v1[e];
                        } else {
                            RGB_PATH(RP_LD_AREA_M1, G.mode != 0u);
                            RGB_PATH(RP_LD_AREA_M0, G.mode == 0u);
                            RGB_PATH(RP_LD_AREA_TAIL, aq + 3u >= G.QW);
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

struct AreaK {
    template <int PK, int S>
    static auto at() { return &krgb_area<PK, S>; }
};

static int area_launch(mcraw_ctx *c, const mcraw_rgb *p, const mcraw_area *a, const mcraw_display *d, const mcraw_yuv *yv,
                       const mcraw_rgb_color *colors, int ncolors, const uint16_t *in, size_t in_pitch, size_t in_frame_stride,
                       int width, int height, int n, void *work, const AreaPlan &P, void *out, hipStream_t st)
{
    RgbArgs A = rgb_args(p, d, yv, in_pitch, in_frame_stride, width, height, ncolors);
    A.Wo = static_cast<uint32_t>(P.rgb.Wo);
    A.Ho = static_cast<uint32_t>(P.rgb.Ho);
    A.tilesX = P.tilesX;
    A.units = P.units;
    A.invec = P.mode == 2u;
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
    return rgb_launch(c, rgb_pick<AreaK>(P.rgb), A, P.rgb, rgb_cols(p, colors, ncolors, 0.03125f), in, n, out, -1, st, G);
}

} // namespace mcraw

using namespace mcraw;

extern "C" {

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
