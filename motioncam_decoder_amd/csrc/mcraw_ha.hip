// mcraw_ha.hip -- the gfx950 kernel of the edge-directed demosaic, MCRAW_RGB_HA: Hamilton-Adams adaptive colour-plane
// interpolation in integers, into the float, display and YUV families (mcraw_demosaic_batch, _display_batch, _yuv_batch: the entry
// points and rgb_check are mcraw_rgb.hip's and mcraw_rgb_args.h's; they hand an accepted call with plan.ha to ha_launch below).
// The contract: include/mcraw_hip.h; the numpy statement: tests/_ha_ref.py; the tile, its LDS arrays and every index, free of HIP:
// mcraw_ha_args.h.  The colour stage and the stores are the siblings' (mcraw_rgb_dev.h), the host side of the launch too
// (mcraw_rgb_launch.h).
//
//   krgb_ha  one instance per (output kind, CFA), as the siblings
//
// A workgroup owns MHC's tile of 256 x 32 pixels.
//   stage      the raw samples of the tile and 3 either side, reflected at the frame's edges, as 16-byte pieces on the frame's
//              8-column grid (s_raw, krgb_mhc's layout with two more rows)
//   green      the green plane g at the R / B sites of the tile and its ring of one, to s_g at half density (at a green site g is
//              8 d, which the next phase makes itself).  A lane takes 8 columns of a row pair, so that the CFA fixes the sites of
//              every slot when the kernel is compiled (template S), as in krgb_mhc; the ring's two columns are 34 single sites,
//              made one per lane from scalar LDS reads
//   estimates  behind a barrier, a lane takes 8 columns of the row pairs ly and ly + 8, as in krgb_mhc: the window of d (4 x 10)
//              and of g (4 x 5) from LDS, E[3][8] per row, and the family's row store
// Every three-way choice is a pair of selects: the lanes of a wave disagree on every edge.
// Float kinds: one tile per workgroup; display and YUV kinds: a persistent grid that stages the LUT once, as krgb_mhc.
#ifdef MCRAW_PATHSR // (the test builds' switches: the head of mcraw_rgb.hip; the grid's cap comes from that source, below)
#include "mcraw_rgb_paths.h"
#endif
#include "mcraw_dev.h"
#include "mcraw_host.h"
#include "mcraw_rgb_args.h"
#include "mcraw_rgb_dev.h"
// The persistent grid's limit is mcraw_rgb.hip's: this unit does not name the cap's switch, and a build of that source with a
// capped grid (build.RGB_PATH_VARIANTS) caps this unit's grid too (tests/test_gpu_ha_paths.py).
namespace mcraw {
uint32_t rgb_grid_limit(uint32_t resident);
}
#define RGB_GRID_LIMIT(resident) ::mcraw::rgb_grid_limit(resident)
#include "mcraw_ha_args.h"
#include "mcraw_rgb_launch.h"

namespace mcraw {

// 2 a where Da < Db, 2 b where Db < Da, a + b where they are equal
__device__ __forceinline__ int ha_pick(int a, int Da, int b, int Db)
{
    const int lo = Da < Db ? a : b; // (equal: b)
    const int hi = Db < Da ? b : a; // (equal: a)
    return lo + hi;
}

// g at an R / B site from d there (C), its axial neighbours at distance 1 (w1, e1, n1, s1) and 2 (w2, e2, n2, s2); SITE: the call
// site for the census (0 a main item, 1 an edge item)
template <int SITE>
__device__ __forceinline__ int ha_green(int C, int w1, int e1, int w2, int e2, int n1, int s1, int n2, int s2)
{
    const int ch = 2 * C - w2 - e2, cv = 2 * C - n2 - s2;
    const int gh = 2 * (w1 + e1) + ch, gv = 2 * (n1 + s1) + cv;
    const int DH = abs(w1 - e1) + abs(ch), DV = abs(n1 - s1) + abs(cv);
    HA_PICKS(SITE, DH, DV, true);
    return ha_pick(gh, DH, gv, DV);
}

template <int PK, int S>
__global__ void __launch_bounds__(RGB_T) krgb_ha(const RgbArgs A)
{
    constexpr bool LUT = has_lut(PK);
    __shared__ __attribute__((aligned(16))) uint16_t s_raw[HA_RAWH * HA_RAWW];
    __shared__ __attribute__((aligned(16))) int32_t s_g[HA_GH * HA_GW];
    __shared__ __attribute__((aligned(16))) uint16_t s_lut[LUT ? DISP_LDS_MAX : 8u];
    uint32_t t = blockIdx.x;
    RGB_WALK_DECL;
    if constexpr (LUT)
        stage_lut(A, s_lut);
    const int W = static_cast<int>(A.W), H = static_cast<int>(A.H);
    const int bk[4] = {A.black[0], A.black[1], A.black[2], A.black[3]};
    do {
        if constexpr (LUT)
            __syncthreads(); // the LUT is staged; the previous tile's LDS reads are done
#ifdef MCRAW_POISON_RGB
        // the raw window as the siblings'; a green value of 0x05a5a5a5 lies far above every value of ha_green (< 2^21), and the
        // estimates' sums over it (at most 8 of them) stay inside an int: a stray read changes bytes and overflows nothing
        rgb_poison(s_raw, sizeof(s_raw), 0x5a5a5a5bu);
        rgb_poison(s_g, sizeof(s_g), 0x05a5a5a5u);
        __syncthreads();
#endif
        const uint32_t f = LUT ? t / A.units : blockIdx.y, u = LUT ? t % A.units : blockIdx.x;
        RGB_WALK(RF_HA, f, LUT, A.lutg);
        const uint32_t tx = u % A.tilesX, ty = u / A.tilesX;
        const int x0 = static_cast<int>(tx * MHC_TW), y0 = static_cast<int>(ty * MHC_TH);
        const uint16_t *in = A.in + static_cast<size_t>(f) * A.fstride;
        // ---- stage: raw rows y0 - 3 .. y0 + 34, columns x0 - 8 .. x0 + 263
        for (uint32_t i = threadIdx.x; i < HA_STAGE_ITEMS; i += RGB_T) {
            const uint32_t r = i / HA_RAWCH, q = i % HA_RAWCH;
            const uint16_t *row = in + static_cast<size_t>(reflect101(y0 - 3 + static_cast<int>(r), H)) * A.pitch;
            const int xs = x0 - 8 + 8 * static_cast<int>(q);
            mcraw_u32x4 v;
            if (A.invec && xs >= 0 && xs + 8 <= W) {
                RGB_PATH(RP_HA_LD_VEC, true);
                v = *gptr<const mcraw_u32x4>(row + xs);
            } else {
                RGB_PATH(RP_HA_LD_ELEM, true);
                uint32_t e[8];
#pragma unroll
                for (int k = 0; k < 8; k++)
                    e[k] = gptr<const uint16_t>(row)[reflect101(xs + k, W)];
                v = mcraw_u32x4{e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16)};
            }
            *reinterpret_cast<mcraw_u32x4 *>(&s_raw[ha_raw_idx(r, 8u * q)]) = v;
        }
        __syncthreads();
        // ---- green, main items: g rows 2 rp and 2 rp + 1 (frame rows of parity 1 and 0), tile columns 8 q .. 8 q + 7
        for (uint32_t i = threadIdx.x; i < HA_G_MAIN; i += RGB_T) {
            const uint32_t rp = i / (MHC_TW / 8u), q = i % (MHC_TW / 8u);
            int d[6][12]; // raw rows 2 rp .. 2 rp + 5 (frame parity (r + 1) & 1), raw columns 8 q + 6 .. 8 q + 17
#pragma unroll
            for (int r = 0; r < 6; r++) {
                const uint16_t *lrow = &s_raw[ha_raw_idx(2u * rp + static_cast<uint32_t>(r), 8u * q)];
                const uint32_t c0 = *reinterpret_cast<const uint32_t *>(lrow + 6);
                const mcraw_u32x4 c1 = *reinterpret_cast<const mcraw_u32x4 *>(lrow + 8);
                const uint32_t c2 = *reinterpret_cast<const uint32_t *>(lrow + 16);
                const uint32_t w[6] = {c0, c1[0], c1[1], c1[2], c1[3], c2};
#pragma unroll
                for (int j = 0; j < 12; j++)
                    d[r][j] = static_cast<int>((w[j >> 1] >> (16u * (j & 1))) & 0xffffu) - bk[((r + 1) & 1) * 2 + (j & 1)];
            }
#pragma unroll
            for (int a = 0; a < 2; a++) {
                const int R = a + 2;
                const int xp = static_cast<int>(ha_rb_xpar(static_cast<uint32_t>((a + 1) & 1), S)); // the row's R / B columns
                uint32_t g[4];
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    const int J = 2 * k + xp + 2;
                    g[k] = static_cast<uint32_t>(ha_green<0>(d[R][J], d[R][J - 1], d[R][J + 1], d[R][J - 2], d[R][J + 2], d[R - 1][J],
                                                          d[R + 1][J], d[R - 2][J], d[R + 2][J]));
                }
                *reinterpret_cast<mcraw_u32x4 *>(&s_g[ha_g_idx(2u * rp + static_cast<uint32_t>(a), 4u * q + 4u)]) =
                    mcraw_u32x4{g[0], g[1], g[2], g[3]};
            }
        }
        // ---- green, edge items: the ring's column x0 - 1 or x0 + 256 of g row Q, whichever is an R / B site
        if (threadIdx.x - HA_G_EDGE_T0 < HA_G_EDGE) {
            const uint32_t Q = threadIdx.x - HA_G_EDGE_T0, C = ha_edge_rawcol(Q, S);
            const uint32_t yp = (Q + 1u) & 1u, xp = C & 1u; // the site's frame parities
            const int b_c = yp ? (xp ? bk[3] : bk[2]) : (xp ? bk[1] : bk[0]);   // the site and distance 2
            const int b_h = yp ? (xp ? bk[2] : bk[3]) : (xp ? bk[0] : bk[1]);   // left and right
            const int b_v = yp ? (xp ? bk[1] : bk[0]) : (xp ? bk[3] : bk[2]);   // above and below
            const auto at = [&](uint32_t dr, int dc) { return static_cast<int>(s_raw[ha_raw_idx(Q + dr, static_cast<uint32_t>(static_cast<int>(C) + dc))]); };
            s_g[ha_g_idx(Q, C >> 1)] = ha_green<1>(at(2, 0) - b_c, at(2, -1) - b_h, at(2, 1) - b_h, at(2, -2) - b_c, at(2, 2) - b_c,
                                                at(1, 0) - b_v, at(3, 0) - b_v, at(0, 0) - b_c, at(4, 0) - b_c);
        }
        __syncthreads();
        // ---- estimates
        const uint32_t lx = threadIdx.x & 31u, ly = threadIdx.x >> 5;
        const uint32_t x = static_cast<uint32_t>(x0) + 8u * lx;
        RGB_PATH(RP_HA_CONTINUE, x >= A.W);
        if (x >= A.W)
            continue;
        const uint32_t n = min(8u, A.W - x);
        const RgbCol &col = A.col[A.percol ? f : 0u];
        uint8_t *fout = A.out + static_cast<size_t>(f) * 3u * A.Ho * A.Wo * out_es(PK) / (is_yuv(PK) ? 2u : 1u);
#pragma unroll 1
        for (uint32_t pass = 0; pass < MHC_TH / 16u; pass++) {
            const uint32_t tr = 2u * (ly + 8u * pass), y = static_cast<uint32_t>(y0) + tr;
            RGB_PATH(RP_HA_BREAK, y >= A.H);
            if (y >= A.H)
                break;
            // d[r][j], G[r][j] at frame (y - 1 + r, x - 1 + j): frame parities (r + 1) & 1 and (j + 1) & 1
            int d[4][10], G[4][10];
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const uint16_t *lrow = &s_raw[ha_raw_idx(tr + 2u + static_cast<uint32_t>(r), 8u * lx)];
                const uint32_t c0 = *reinterpret_cast<const uint32_t *>(lrow + 6);
                const mcraw_u32x4 c1 = *reinterpret_cast<const mcraw_u32x4 *>(lrow + 8);
                const uint32_t c2 = *reinterpret_cast<const uint32_t *>(lrow + 16);
                const uint32_t w[6] = {c0, c1[0], c1[1], c1[2], c1[3], c2};
#pragma unroll
                for (int j = 0; j < 10; j++)
                    d[r][j] = static_cast<int>((w[(j + 1) >> 1] >> (16u * ((j + 1) & 1))) & 0xffffu) - bk[((r + 1) & 1) * 2 + ((j + 1) & 1)];
                const uint32_t xp = ha_rb_xpar(static_cast<uint32_t>((r + 1) & 1), S); // raw-column parity of the row's R / B sites
                const int32_t *grow = &s_g[ha_g_idx(tr + static_cast<uint32_t>(r), 0u)];
                const mcraw_u32x4 gv = *reinterpret_cast<const mcraw_u32x4 *>(grow + 4u * lx + 4u);
                const int32_t gx = grow[ha_g_extra(xp, lx)];
#pragma unroll
                for (int j = 0; j < 10; j++) {
                    if (((7 + j) & 1) != static_cast<int>(xp))
                        G[r][j] = 8 * d[r][j]; // a green site
                    else if (xp) // raw columns 7, 9 .. 15: j = 0 is the extra entry, j = 2 .. 8 the piece
                        G[r][j] = j == 0 ? gx : static_cast<int32_t>(gv[(j - 2) >> 1 & 3]);
                    else // raw columns 8 .. 14, 16: j = 1 .. 7 the piece, j = 9 the extra entry
                        G[r][j] = j == 9 ? gx : static_cast<int32_t>(gv[(j - 1) >> 1 & 3]);
                }
            }
            int SUM[3][4] = {}; // YUV kinds: the sums of P over the lane's four 2x2 blocks
#pragma unroll
            for (int a = 0; a < 2; a++) {
                int E[3][8];
#pragma unroll
                for (int b = 0; b < 8; b++) {
                    const int R = a + 1, J = b + 1;
                    const int C = d[R][J], g = G[R][J];
                    const int role = (a * 2 + (b & 1)) ^ S;
                    const int nat = 32 * C;
                    if (role == 0 || role == 3) { // R or B site: the other colour along the flatter diagonal
                        const int cN = 2 * g - G[R - 1][J - 1] - G[R + 1][J + 1], cP = 2 * g - G[R - 1][J + 1] - G[R + 1][J - 1];
                        const int nN = 8 * (d[R - 1][J - 1] + d[R + 1][J + 1]) + cN, nP = 8 * (d[R - 1][J + 1] + d[R + 1][J - 1]) + cP;
                        const int DN = 8 * abs(d[R - 1][J - 1] - d[R + 1][J + 1]) + abs(cN);
                        const int DP = 8 * abs(d[R - 1][J + 1] - d[R + 1][J - 1]) + abs(cP);
                        const int o = ha_pick(nN, DN, nP, DP);
                        HA_PICKS(2, DN, DP, static_cast<uint32_t>(b) < n);
                        E[0][b] = role == 0 ? nat : o;
                        E[1][b] = 4 * g;
                        E[2][b] = role == 0 ? o : nat;
                    } else { // G site: role 1 has R left / right, role 2 has B left / right
                        const int hz = 2 * (8 * (d[R][J - 1] + d[R][J + 1]) + (2 * g - G[R][J - 1] - G[R][J + 1]));
                        const int vt = 2 * (8 * (d[R - 1][J] + d[R + 1][J]) + (2 * g - G[R - 1][J] - G[R + 1][J]));
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
    } while (LUT && (t += gridDim.x) < A.units * A.nf);
}

struct HaK {
    template <int PK, int S>
    static auto at() { return &krgb_ha<PK, S>; }
};

// The launches of an accepted MCRAW_RGB_HA call (mcraw_rgb.hip's demosaic_launch, which holds the context's lock and has set the
// device): A as that function fills it for MHC.  No kernel id: no KTimer is made.
int ha_launch(mcraw_ctx *c, const RgbArgs &A, const RgbPlan &P, const std::vector<RgbCol> &cols, const uint16_t *in, int n, void *out,
              hipStream_t st)
{
    return rgb_launch(c, rgb_pick<HaK>(P), A, P, cols, in, n, out, -1, st);
}

} // namespace mcraw
