// mcraw_resample.hip -- gfx950 kernels for uint16 mosaics resident in HBM -> RGB of any size from half to twice a crop window
// (mcraw_demosaic_resample_batch): the Malvar-He-Cutler estimates of krgb_mhc behind a separable polyphase filter, linear or
// cubic, into the float, display and YUV families.  The contract and its weights: include/mcraw_hip.h; the checks, the plan
// and the tap formula, free of HIP: mcraw_resample_args.h; the numpy statement: tests/_resample_ref.py.  The colour stage and
// the stores are the siblings' (mcraw_rgb_dev.h), the host side of the launch theirs too (mcraw_rgb_launch.h).
//
//   kres_tab       the taps of every output column and row, into the caller's scratch, queued in front
//   krgb_resample  one instance per (output kind, CFA), as the siblings
//
// A workgroup owns a tile of 64 output columns x ly output row pairs (the plan's ly: as many as RES_TROWS source rows serve).
//   stage   the raw samples under the tile's taps, with MHC's halo of 2, reflected at the frame's edges, as 16-byte pieces on
//           the frame's 8-column grid (s_raw, krgb_mhc's layout); the tile's column taps (s_xt)
//   A       RES_G source row pairs at a time: a lane takes 8 source columns on the 8-grid of one source row -- the row's
//           parity is uniform in a wave, the columns' is fixed by the slot, so the CFA role of every slot is known when the
//           kernel is compiled (template S), as in krgb_mhc -- and writes the estimates e to s_e
//   B       a lane takes 4 output columns of one of those source rows: the horizontal taps over s_e, into s_t
//   C       a lane takes 8 output columns of an output row pair, as krgb_bin2y: the vertical taps over s_t, then the family's
//           row store (the YUV kinds carry their 2x2 sums over the pair)
// Every sum of taps is exact in two int32 accumulators: v = 256 vh + vl, A = sum w vh, B = sum w vl (the header's bounds),
// 24-bit multiplies (|w| < 2^13, |vh| < 2^15).
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
#include "mcraw_resample_args.h"

namespace mcraw {

struct ResGeo {
    const ResampleTap *xt, *yt;
    int32_t x0, y0;  // the crop's origin
    uint32_t ly;     // row pairs of a tile
    uint32_t tilesX; // column tiles
};

__global__ void __launch_bounds__(RGB_T) kres_tab(ResampleTap *xt, ResampleTap *yt, uint32_t Cw, uint32_t Ow, uint32_t Ch, uint32_t Oh,
                                                  uint32_t filter)
{
    const uint32_t i = blockIdx.x * RGB_T + threadIdx.x;
    ResampleTap t;
    if (i < Ow) {
        resample_taps(i, Cw, Ow, filter, t);
        xt[i] = t;
    } else if (i - Ow < Oh) {
        resample_taps(i - Ow, Ch, Oh, filter, t);
        yt[i - Ow] = t;
    }
}

// Phase A of one lane: the estimates of 8 columns of source row 2 rp + AR of the tile (AR: the row's parity) from the raw window
// in LDS: krgb_mhc's arithmetic, one row of it.
template <int S, int AR>
__device__ __forceinline__ void res_mhc_row(const RgbArgs &A, const uint16_t *s_raw, int32_t *s_e, uint32_t rp, uint32_t erow, uint32_t q)
{
    int d[5][12]; // rows 2 rp + AR - 2 .. + 2 of the estimates' grid, columns 8 q - 2 .. 8 q + 9
#pragma unroll
    for (int r = 0; r < 5; r++) {
        const uint16_t *lrow = &s_raw[(2u * rp + static_cast<uint32_t>(AR + r)) * RES_RAWW + 8u * q];
        const mcraw_u32x4 c0 = *reinterpret_cast<const mcraw_u32x4 *>(lrow);
        const mcraw_u32x4 c1 = *reinterpret_cast<const mcraw_u32x4 *>(lrow + 8);
        const uint32_t c2 = *reinterpret_cast<const uint32_t *>(lrow + 16);
        const uint32_t w[6] = {c0[3], c1[0], c1[1], c1[2], c1[3], c2};
#pragma unroll
        for (int j = 0; j < 12; j++)
            d[r][j] = static_cast<int>((w[j >> 1] >> (16u * (j & 1))) & 0xffffu) - A.black[((AR + r) & 1) * 2 + (j & 1)];
    }
    int E[3][8];
#pragma unroll
    for (int b = 0; b < 8; b++) {
        constexpr int R = 2;
        const int J = b + 2;
        const int C = d[R][J];
        const int n1 = d[R - 1][J], s1 = d[R + 1][J], w1 = d[R][J - 1], e1 = d[R][J + 1];
        const int v2 = d[R - 2][J] + d[R + 2][J], h2 = d[R][J - 2] + d[R][J + 2];
        const int dg = (d[R - 1][J - 1] + d[R - 1][J + 1]) + (d[R + 1][J - 1] + d[R + 1][J + 1]);
        const int role = (AR * 2 + (b & 1)) ^ S;
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
#pragma unroll
    for (uint32_t c = 0; c < 3u; c++) {
        int32_t *dst = &s_e[(c * 2u * RES_G + erow) * RES_ECOLS + 8u * q];
        *reinterpret_cast<mcraw_u32x4 *>(dst) = mcraw_u32x4{static_cast<uint32_t>(E[c][0]), static_cast<uint32_t>(E[c][1]),
                                                            static_cast<uint32_t>(E[c][2]), static_cast<uint32_t>(E[c][3])};
        *reinterpret_cast<mcraw_u32x4 *>(dst + 4) = mcraw_u32x4{static_cast<uint32_t>(E[c][4]), static_cast<uint32_t>(E[c][5]),
                                                                static_cast<uint32_t>(E[c][6]), static_cast<uint32_t>(E[c][7])};
    }
}

template <int PK, int S>
__global__ void __launch_bounds__(RGB_T) krgb_resample(const RgbArgs A, const ResGeo G)
{
    constexpr bool LUT = has_lut(PK);
    __shared__ __attribute__((aligned(16))) uint16_t s_raw[(RES_TROWS + 4u) * RES_RAWW];
    __shared__ __attribute__((aligned(16))) int32_t s_e[3u * 2u * RES_G * RES_ECOLS];
    __shared__ __attribute__((aligned(16))) int32_t s_t[3u * RES_TROWS * RES_TSTRIDE];
    __shared__ __attribute__((aligned(16))) ResampleTap s_xt[RES_TW];
    __shared__ __attribute__((aligned(16))) uint16_t s_lut[LUT ? DISP_LDS_MAX : 8u];
    uint32_t t = blockIdx.x;
    RGB_WALK_DECL;
    if constexpr (LUT)
        stage_lut(A, s_lut);
    const int W = static_cast<int>(A.W), H = static_cast<int>(A.H);
    do {
        const uint32_t f = LUT ? t / A.units : blockIdx.y, u = LUT ? t % A.units : blockIdx.x;
        RGB_WALK(RF_RES, f, LUT, A.lutg);
        const uint32_t tx = u % G.tilesX, band = u / G.tilesX;
        const uint32_t k0 = tx * RES_TW, k1 = min(k0 + RES_TW, A.Wo) - 1u;               // the tile's first and last column
        const uint32_t i0 = band * 2u * G.ly, i1 = min(i0 + 2u * G.ly, A.Ho) - 1u;        // ... and row
        // the estimates the tile needs: columns cf .. cl and rows rf .. rl of the frame (up to 3 outside it on every side);
        // held from column eb (on the 8-grid) and row pb (even) on: ne pieces of 8 columns, np row pairs
        // (the first tap of the first two pixels, the last tap of the last two: a pixel that sits on a sample has a single tap,
        // inside its neighbours' windows; tests/cpp/resample_args_check.cpp holds every tap of every tile against this window)
        const uint32_t k0b = min(k0 + 1u, k1), k1b = max(k1, k0 + 1u) - 1u, i0b = min(i0 + 1u, i1), i1b = max(i1, i0 + 1u) - 1u;
        const int cf = G.x0 + min(G.xt[k0].j0, G.xt[k0b].j0);
        const int cl = G.x0 + max(G.xt[k1].j0 + static_cast<int>(G.xt[k1].nt), G.xt[k1b].j0 + static_cast<int>(G.xt[k1b].nt)) - 1;
        const int rf = G.y0 + min(G.yt[i0].j0, G.yt[i0b].j0);
        const int rl = G.y0 + max(G.yt[i1].j0 + static_cast<int>(G.yt[i1].nt), G.yt[i1b].j0 + static_cast<int>(G.yt[i1b].nt)) - 1;
        const int eb = cf & ~7, pb = rf & ~1;
        const uint32_t ne = min(static_cast<uint32_t>((cl - eb) >> 3) + 1u, RES_ECOLS / 8u);
        const uint32_t np = min(static_cast<uint32_t>((rl - pb) >> 1) + 1u, RES_TROWS / 2u);
        const uint16_t *in = A.in + static_cast<size_t>(f) * A.fstride;
        __syncthreads(); // the LUT is staged; the previous tile's LDS reads are done
#ifdef MCRAW_POISON_RGB
        rgb_poison(s_raw, sizeof(s_raw), 0x5a5a5a5bu);
        rgb_poison(s_e, sizeof(s_e), 0x5a5a5a5bu);
        rgb_poison(s_t, sizeof(s_t), 0x5a5a5a5bu);
        rgb_poison(s_xt, sizeof(s_xt), 0x5a5a5a5bu);
        __syncthreads();
#endif
        // raw rows pb - 2 .. pb + 2 np + 1, columns eb - 8 .. eb + 8 ne + 7
        const uint32_t nch = ne + 2u;
        for (uint32_t i = threadIdx.x; i < (2u * np + 4u) * nch; i += RGB_T) {
            const uint32_t r = i / nch, q = i % nch;
            const uint16_t *row = in + static_cast<size_t>(reflect101(pb - 2 + static_cast<int>(r), H)) * A.pitch;
            const int xs = eb - 8 + 8 * static_cast<int>(q);
            mcraw_u32x4 v;
            if (A.invec && xs >= 0 && xs + 8 <= W) {
                RGB_PATH(RP_LD_RES_VEC, true);
                v = *gptr<const mcraw_u32x4>(row + xs);
            } else {
                RGB_PATH(RP_LD_RES_ELEM, true);
                uint32_t e[8];
#pragma unroll
                for (int k = 0; k < 8; k++)
                    e[k] = gptr<const uint16_t>(row)[reflect101(xs + k, W)];
                v = mcraw_u32x4{e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16)};
            }
            *reinterpret_cast<mcraw_u32x4 *>(&s_raw[r * RES_RAWW + 8u * q]) = v;
        }
        for (uint32_t i = threadIdx.x; i < RES_TW * (sizeof(ResampleTap) / 4u); i += RGB_T) { // as dwords; columns behind the row: no taps
            const uint32_t k = k0 + i / static_cast<uint32_t>(sizeof(ResampleTap) / 4u);
            reinterpret_cast<uint32_t *>(s_xt)[i] = k <= k1 ? gptr<const uint32_t>(G.xt + k0)[i] : 0u;
        }
#pragma unroll 1
        for (uint32_t c0 = 0; c0 < np; c0 += RES_G) {
            const uint32_t ga = min(RES_G, np - c0);
            __syncthreads(); // s_raw and s_xt are written; the previous round's reads of s_e are done
            // A: rows of parity 0 in the first half of the workgroup, of parity 1 in the second (uniform in a wave)
            if (threadIdx.x < RGB_T / 2u) {
                for (uint32_t it = threadIdx.x; it < ga * ne; it += RGB_T / 2u)
                    res_mhc_row<S, 0>(A, s_raw, s_e, c0 + it / ne, 2u * (it / ne), it % ne);
            } else {
                for (uint32_t it = threadIdx.x - RGB_T / 2u; it < ga * ne; it += RGB_T / 2u)
                    res_mhc_row<S, 1>(A, s_raw, s_e, c0 + it / ne, 2u * (it / ne) + 1u, it % ne);
            }
            __syncthreads();
            // B: (source row, 4 output columns)
            for (uint32_t it = threadIdx.x; it < 2u * ga * (RES_TW / 4u); it += RGB_T) {
                const uint32_t er = it / (RES_TW / 4u), cg = it % (RES_TW / 4u);
                int32_t tv[3][4];
#pragma unroll
                for (uint32_t i = 0; i < 4u; i++) {
                    const ResampleTap &tp = s_xt[4u * cg + i];
                    const uint32_t col = static_cast<uint32_t>(G.x0 + tp.j0 - eb), nt = tp.nt;
                    int32_t a[3] = {0, 0, 0}, b[3] = {0, 0, 0};
                    for (uint32_t s = 0; s < nt; s++) {
                        const int32_t w = tp.w[s];
#pragma unroll
                        for (uint32_t c = 0; c < 3u; c++) {
                            const int32_t v = s_e[(c * 2u * RES_G + er) * RES_ECOLS + min(col + s, RES_ECOLS - 1u)];
                            a[c] += __mul24(w, v >> 8);
                            b[c] += __mul24(w, v & 255);
                        }
                    }
#pragma unroll
                    for (int c = 0; c < 3; c++)
                        tv[c][i] = (a[c] + ((b[c] + 2048) >> 8)) >> 4;
                }
#pragma unroll
                for (uint32_t c = 0; c < 3u; c++)
                    *reinterpret_cast<mcraw_u32x4 *>(&s_t[(c * RES_TROWS + 2u * c0 + er) * RES_TSTRIDE + 4u * cg]) =
                        mcraw_u32x4{static_cast<uint32_t>(tv[c][0]), static_cast<uint32_t>(tv[c][1]), static_cast<uint32_t>(tv[c][2]),
                                    static_cast<uint32_t>(tv[c][3])};
            }
        }
        __syncthreads();
        // C: (8 output columns, output row pair)
        const uint32_t lxid = threadIdx.x & 7u, lyid = threadIdx.x >> 3;
        const uint32_t xo = k0 + 8u * lxid;
        RGB_PATH(RP_IDLE_RES, !(lyid < G.ly && xo < A.Wo && i0 + 2u * lyid <= i1));
        if (lyid < G.ly && xo < A.Wo && i0 + 2u * lyid <= i1) {
            const uint32_t n = min(8u, A.Wo - xo);
            const RgbCol &col = A.col[A.percol ? f : 0u];
            uint8_t *fout = A.out + static_cast<size_t>(f) * 3u * A.Ho * A.Wo * out_es(PK) / (is_yuv(PK) ? 2u : 1u);
            int SUM[3][4] = {}; // YUV kinds: the sums of P over the lane's four 2x2 blocks
#pragma unroll 1
            for (uint32_t a = 0; a < 2u; a++) {
                const uint32_t j = i0 + 2u * lyid + a;
                if (j > i1) // (the YUV kinds: Ho is even, a row pair always has both rows)
                    break;
                const ResampleTap *tp = &G.yt[j];
                const uint32_t row = static_cast<uint32_t>(G.y0 + tp->j0 - pb), nt = tp->nt;
                int32_t sa[3][8] = {}, sb[3][8] = {};
                for (uint32_t s = 0; s < nt; s++) {
                    const int32_t w = tp->w[s];
#pragma unroll
                    for (uint32_t c = 0; c < 3u; c++) {
                        const int32_t *src = &s_t[(c * RES_TROWS + min(row + s, RES_TROWS - 1u)) * RES_TSTRIDE + 8u * lxid];
                        const mcraw_u32x4 v0 = *reinterpret_cast<const mcraw_u32x4 *>(src);
                        const mcraw_u32x4 v1 = *reinterpret_cast<const mcraw_u32x4 *>(src + 4);
#pragma unroll
                        for (int i = 0; i < 8; i++) {
                            const int32_t v = static_cast<int32_t>(i < 4 ? v0[i] : v1[i - 4]);
                            sa[c][i] += __mul24(w, v >> 8);
                            sb[c][i] += __mul24(w, v & 255);
                        }
                    }
                }
                int E[3][8];
#pragma unroll
                for (int c = 0; c < 3; c++)
#pragma unroll
                    for (int i = 0; i < 8; i++)
                        E[c][i] = (sa[c][i] + ((sb[c][i] + 2048) >> 8)) >> 4;
                if constexpr (is_yuv(PK))
                    yuv_row8<PK>(A, col, s_lut, fout, j, xo, n, static_cast<int>(a), E, SUM);
                else if constexpr (is_disp(PK))
                    disp_store8<PK>(A, col, s_lut, fout, j, xo, n, E);
                else
                    rgb_store8<PK>(A, col, fout, j, xo, n, E);
            }
        }
    } while (LUT && (t += gridDim.x) < A.units * A.nf);
}

struct ResK {
    template <int PK, int S>
    static auto at() { return &krgb_resample<PK, S>; }
};

static int resample_launch(mcraw_ctx *c, const mcraw_rgb *p, const mcraw_resample *r, const mcraw_display *d, const mcraw_yuv *yv,
                           const mcraw_rgb_color *colors, int ncolors, const uint16_t *in, size_t in_pitch, size_t in_frame_stride,
                           int width, int height, int n, void *work, const ResamplePlan &P, void *out, hipStream_t st)
{
    RgbArgs A = rgb_args(p, d, yv, in_pitch, in_frame_stride, width, height, ncolors);
    A.Wo = static_cast<uint32_t>(P.rgb.Wo);
    A.Ho = static_cast<uint32_t>(P.rgb.Ho);
    A.tilesX = P.tilesX;
    A.units = P.units;
    A.invec = P.rgb.invec;
    ResGeo G{};
    G.xt = reinterpret_cast<const ResampleTap *>(static_cast<const char *>(work) + P.xtab);
    G.yt = reinterpret_cast<const ResampleTap *>(static_cast<const char *>(work) + P.ytab);
    G.x0 = static_cast<int32_t>(r->x0), G.y0 = static_cast<int32_t>(r->y0);
    G.ly = P.ly;
    G.tilesX = P.tilesX;
    hipLaunchKernelGGL(kres_tab, dim3((A.Wo + A.Ho + RGB_T - 1u) / RGB_T), dim3(RGB_T), 0, st, const_cast<ResampleTap *>(G.xt),
                       const_cast<ResampleTap *>(G.yt), r->cw, A.Wo, r->ch, A.Ho, r->filter);
    HIP_TRY(hipGetLastError());
    return rgb_launch(c, rgb_pick<ResK>(P.rgb), A, P.rgb, rgb_cols(p, colors, ncolors, 0.0625f), in, n, out, -1, st, G);
}

} // namespace mcraw

using namespace mcraw;

extern "C" {

size_t mcraw_resample_work_bytes(const mcraw_resample *r)
{
    ResamplePlan P;
    if (!r || P.geometry(r))
        return 0u;
    return P.total;
}

int mcraw_demosaic_resample_batch(mcraw_ctx *c, const mcraw_rgb *p, const mcraw_resample *r, const mcraw_display *d, const mcraw_yuv *y,
                                  const mcraw_rgb_color *colors, int ncolors, const uint16_t *in, size_t in_pitch,
                                  size_t in_frame_stride, int width, int height, int n, void *work, size_t work_bytes, void *out,
                                  size_t out_bytes, void *stream)
{
    ResamplePlan P;
    const char *why = c ? resample_check(p, r, d, y, colors, ncolors, in, in_pitch, in_frame_stride, width, height, n, work, work_bytes,
                                         out, out_bytes, P)
                        : "bad arguments";
    if (why)
        return reject("mcraw_demosaic_resample_batch", why);
    if (P.rgb.noop)
        return 0;
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    return resample_launch(c, p, r, d, y, colors, ncolors, in, in_pitch, in_frame_stride, width, height, n, work, P, out, stream_of(c, stream));
}

} // extern "C"
