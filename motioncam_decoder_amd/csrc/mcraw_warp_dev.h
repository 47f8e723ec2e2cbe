// mcraw_warp_dev.h -- the device code that the kernels sampling the MHC image through a 4 x 4 gather share (krgb_warp:
// csrc/mcraw_warp.hip; krgb_mesh: csrc/mcraw_mesh.hip): staging of a tile's raw window, phase A of one lane, the weights of a phase,
// the taps of one pixel from a tap origin inside the window's estimates, and the store phase.  The LDS arrays' sizes are mcraw_warp_args.h's.
//
// Hooks of a test build's path census, empty unless defined in front of this header (mcraw_rgb_paths.h does, for the source that
// includes it under its switch; this header names none), as RGB_PATH of mcraw_rgb_dev.h:
//   WARP_PATH(slot, cond)   the active lanes for which `cond` holds take path `slot` of the including kernel's family
//   WARP_UNIT(slot, cond)   the workgroup's unit takes it (`cond` is uniform over the workgroup)
#pragma once
#ifndef WARP_PATH
#define WARP_PATH(slot, cond)
#define WARP_UNIT(slot, cond)
#endif
#include "mcraw_dev.h"
#include "mcraw_rgb_args.h"
#include "mcraw_rgb_dev.h"
#include "mcraw_warp_args.h"

namespace mcraw {

// Phase A of one lane: the estimates of 8 columns of source row 2 rp + AR of the window (AR: the row's parity) from the raw
// window in LDS: krgb_mhc's arithmetic, one row of it.
template <int S, int AR>
__device__ __forceinline__ void warp_mhc_row(const RgbArgs &A, const uint16_t *s_raw, int32_t *s_e, uint32_t rp, uint32_t q)
{
    int d[5][12]; // rows 2 rp + AR - 2 .. + 2 of the estimates' grid, columns 8 q - 2 .. 8 q + 9
#pragma unroll
    for (int r = 0; r < 5; r++) {
        const uint16_t *lrow = &s_raw[(2u * rp + static_cast<uint32_t>(AR + r)) * WARP_RAWW + 8u * q];
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
        int32_t *dst = &s_e[(c * WARP_EROWS + 2u * rp + static_cast<uint32_t>(AR)) * WARP_ESTRIDE + 8u * q];
        *reinterpret_cast<mcraw_u32x4 *>(dst) = mcraw_u32x4{static_cast<uint32_t>(E[c][0]), static_cast<uint32_t>(E[c][1]),
                                                            static_cast<uint32_t>(E[c][2]), static_cast<uint32_t>(E[c][3])};
        *reinterpret_cast<mcraw_u32x4 *>(dst + 4) = mcraw_u32x4{static_cast<uint32_t>(E[c][4]), static_cast<uint32_t>(E[c][5]),
                                                                static_cast<uint32_t>(E[c][6]), static_cast<uint32_t>(E[c][7])};
    }
}

// The four weights of phase p out of the table in LDS.
__device__ __forceinline__ void warp_weights(const int16_t *s_w, uint32_t p, int32_t (&w)[4])
{
    const mcraw_u32x2 v = *reinterpret_cast<const mcraw_u32x2 *>(&s_w[4u * p]);
    w[0] = static_cast<int32_t>(v[0] << 16) >> 16;
    w[1] = static_cast<int32_t>(v[0]) >> 16;
    w[2] = static_cast<int32_t>(v[1] << 16) >> 16;
    w[3] = static_cast<int32_t>(v[1]) >> 16;
}

// Staging: the raw samples under a tile's window -- rows pb - 2 .. pb + 2 np + 1, columns eb - 8 .. eb + 8 ne + 7 of frame `in`,
// reflected at the frame's edges (what lies further out than one reflection reaches is clamped into the row by reflect101 and
// read by no tap) -- as 16-byte pieces on the frame's 8-column grid.
__device__ __forceinline__ void warp_stage(const RgbArgs &A, const uint16_t *in, uint16_t *s_raw, int32_t pb, int32_t eb, uint32_t np, uint32_t ne,
                                           int W, int H)
{
    const uint32_t nch = ne + 2u;
    for (uint32_t i = threadIdx.x; i < (2u * np + 4u) * nch; i += RGB_T) {
        const uint32_t r = i / nch, q = i % nch;
        const uint16_t *row = in + static_cast<size_t>(reflect101(pb - 2 + static_cast<int>(r), H)) * A.pitch;
        const int xs = eb - 8 + 8 * static_cast<int>(q);
        mcraw_u32x4 v;
        if (A.invec && xs >= 0 && xs + 8 <= W) {
            WARP_PATH(RPG_LD_VEC, true);
            v = *gptr<const mcraw_u32x4>(row + xs);
        } else {
            WARP_PATH(RPG_LD_ELEM, true);
            uint32_t e[8];
#pragma unroll
            for (int k = 0; k < 8; k++)
                e[k] = gptr<const uint16_t>(row)[reflect101(xs + k, W)];
            v = mcraw_u32x4{e[0] | (e[1] << 16), e[2] | (e[3] << 16), e[4] | (e[5] << 16), e[6] | (e[7] << 16)};
        }
        *reinterpret_cast<mcraw_u32x4 *>(&s_raw[r * WARP_RAWW + 8u * q]) = v;
    }
}

// The store phase: a lane takes 8 output columns of an output row (the YUV kinds: of a row pair) of tile rows i0 .. i1 from
// column k0 on out of the tile's E in s_e and calls the family's row store for frame f.
template <int PK>
__device__ __forceinline__ void warp_store(const RgbArgs &A, const int32_t *s_e, const uint16_t *s_lut, uint32_t f, uint32_t i0, uint32_t i1,
                                           uint32_t k0)
{
    constexpr uint32_t ROWS = is_yuv(PK) ? 2u : 1u; // output rows of a lane
    const uint32_t lxid = threadIdx.x & (WARP_TW / 8u - 1u), lyid = threadIdx.x / (WARP_TW / 8u);
    const uint32_t xo = k0 + 8u * lxid, j0 = i0 + ROWS * lyid;
    WARP_PATH(RPG_ST_IDLE_LY, lyid >= WARP_TH / ROWS);
    WARP_PATH(RPG_ST_IDLE_X, lyid < WARP_TH / ROWS && xo >= A.Wo);
    WARP_PATH(RPG_ST_IDLE_ROW, lyid < WARP_TH / ROWS && xo < A.Wo && j0 > i1);
    if (lyid < WARP_TH / ROWS && xo < A.Wo && j0 <= i1) {
        const uint32_t n = min(8u, A.Wo - xo);
        const RgbCol &col = A.col[A.percol ? f : 0u];
        uint8_t *fout = A.out + static_cast<size_t>(f) * 3u * A.Ho * A.Wo * out_es(PK) / (is_yuv(PK) ? 2u : 1u);
        int SUM[3][4] = {}; // YUV kinds: the sums of P over the lane's four 2x2 blocks
#pragma unroll 1
        for (uint32_t a = 0; a < ROWS; a++) {
            const uint32_t j = j0 + a; // (the YUV kinds: Ho is even, a row pair always has both rows)
            int E[3][8];
#pragma unroll
            for (uint32_t c = 0; c < 3u; c++) {
                const int32_t *src = &s_e[(c * WARP_TH + (j - i0)) * WARP_TW + 8u * lxid];
                const mcraw_u32x4 v0 = *reinterpret_cast<const mcraw_u32x4 *>(src);
                const mcraw_u32x4 v1 = *reinterpret_cast<const mcraw_u32x4 *>(src + 4);
#pragma unroll
                for (int i = 0; i < 8; i++)
                    E[c][i] = static_cast<int32_t>(i < 4 ? v0[i] : v1[i - 4]);
            }
            if constexpr (is_yuv(PK))
                yuv_row8<PK>(A, col, s_lut, fout, j, xo, n, static_cast<int>(a), E, SUM);
            else if constexpr (is_disp(PK))
                disp_store8<PK>(A, col, s_lut, fout, j, xo, n, E);
            else
                rgb_store8<PK>(A, col, fout, j, xo, n, E);
        }
    }
}

// One output pixel: the 4 x 4 taps, weights wy and wx, over the window's estimates from row r0, column c0 of s_e on, horizontally
// first.  The caller keeps r0 + 3 and c0 + 3 inside the array.
__device__ __forceinline__ void warp_taps(const int32_t *s_e, const int32_t (&wy)[4], const int32_t (&wx)[4], int32_t r0, int32_t c0,
                                          int32_t (&E)[3])
{
#pragma unroll
    for (uint32_t c = 0; c < 3u; c++) {
        const int32_t *src = &s_e[(c * WARP_EROWS + static_cast<uint32_t>(r0)) * WARP_ESTRIDE + static_cast<uint32_t>(c0)];
        int32_t a2 = 0, b2 = 0;
#pragma unroll
        for (uint32_t r = 0; r < 4u; r++) {
            int32_t a = 0, b = 0;
#pragma unroll
            for (uint32_t j = 0; j < 4u; j++) {
                const int32_t v = src[r * WARP_ESTRIDE + j];
                a += __mul24(wx[j], v >> 8);
                b += __mul24(wx[j], v & 255);
            }
            const int32_t t = (a + ((b + 2048) >> 8)) >> 4;
            a2 += __mul24(wy[r], t >> 8);
            b2 += __mul24(wy[r], t & 255);
        }
        E[c] = (a2 + ((b2 + 2048) >> 8)) >> 4;
    }
}

} // namespace mcraw
