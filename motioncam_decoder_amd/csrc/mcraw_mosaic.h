// mcraw_mosaic.h -- device helpers that the mosaic stages share (mcraw_shade / stats / fixpix / denoise / merge / align .hip: uint16 mosaics
// resident in HBM in, lanes that make 8 consecutive columns as 4 dwords of (even column | odd column << 16)).  A unit's tile
// sizes and store policy reach these helpers as template arguments: no -D switch of a unit is read in here.
#pragma once
#include "mcraw_dev.h"

// The hooks of the path census of the stages (mcraw_mosaic_paths.h, test builds only): empty unless a source defined them in front
// of this header.
#ifndef MOS_PATH
#define MOS_PATH(slot, cond)
#endif
#ifndef MOS_WAVE
#define MOS_WAVE(slot, cond)
#endif
#ifndef MOS_STAGE
#define MOS_STAGE(inner, whole, vec)
#endif
#ifndef MOS_DIV
#define MOS_DIV(r, den)
#endif

namespace mcraw {

__device__ __forceinline__ uint32_t half16(uint32_t w, uint32_t h)
{
    return h ? w >> 16 : w & 0xFFFFu;
}

// v_mul_u32_u24: both factors below 2^24
__device__ __forceinline__ uint32_t mul24(uint32_t a, uint32_t b)
{
    return static_cast<uint32_t>(__umul24(a, b));
}

// n / den, exactly, for the rounding divides (num + (den >> 1)) / den of the weighted means.  The widest range any caller uses:
// n < 2^30, den <= 6400, quotient <= 65536 (a weighted mean of uint16 values plus the rounding half).  In float: n rounds with a
// relative error of 2^-24, den is exact, v_rcp_f32 is good to 1 ulp (2^-23) and the product rounds once more: the estimate is off
// by less than 65536 * 2^-21 = 1 / 32, so its integer part is the quotient or one beside it, and one step either way by the sign
// of the remainder makes it exact.  Outside that range the result is merely some number: nothing here traps or is
// undefined for any n and any den >= 1 (kdenoise and kmerge also call it for a lane's columns past the row end, whose sums come
// from samples that no output reads; their den is still 256 .. 6400, and the result is never stored).
__device__ __forceinline__ uint32_t div_round(uint32_t n, uint32_t den)
{
    uint32_t q = static_cast<uint32_t>(static_cast<float>(n) * __builtin_amdgcn_rcpf(static_cast<float>(den)));
    const int32_t r = static_cast<int32_t>(n - mul24(q, den)); // q <= 65537, den < 2^13: exact
    MOS_DIV(r, den);
    q = r < 0 ? q - 1u : q;
    q = r >= static_cast<int32_t>(den) ? q + 1u : q;
    return q;
}

// Two uint16 per dword, both halves at once (v_pk_min_u16, v_pk_max_u16, v_pk_sub_u16).
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ uint32_t pk_min(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_min(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}
__device__ __forceinline__ uint32_t pk_max(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}
__device__ __forceinline__ uint32_t pk_sub(uint32_t a, uint32_t b)
{
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(u16x2, a) - __builtin_bit_cast(u16x2, b));
}
__device__ __forceinline__ uint32_t pk_absdiff(uint32_t a, uint32_t b)
{
    return pk_sub(pk_max(a, b), pk_min(a, b));
}

// 16 bytes that are 2-byte aligned only: rows off the 16-byte grid are moved with one unaligned access
typedef uint32_t u32x4_unaligned __attribute__((ext_vector_type(4), aligned(2)));

// 8 consecutive samples from src as 4 dwords.  vec: src lies on the 16-byte grid.
__device__ __forceinline__ mcraw_u32x4 load16(const uint16_t *src, bool vec)
{
    if (vec)
        return *gptr<const mcraw_u32x4>(src);
    const u32x4_unaligned t = *gptr<const u32x4_unaligned>(src);
    return mcraw_u32x4{t[0], t[1], t[2], t[3]};
}

// 8 samples of columns x .. x + 7 (the first n exist) as (even column | odd column << 16) dwords.
__device__ __forceinline__ void load8(const uint16_t *src, uint32_t n, bool vec, uint32_t p[4])
{
    MOS_PATH(MP_LD_VEC, n == 8u && vec);
    MOS_PATH(MP_LD_UNAL, n == 8u && !vec);
    MOS_PATH(MP_LD_ELEM, n != 8u);
    if (n == 8u) {
        const mcraw_u32x4 v = load16(src, vec);
        p[0] = v[0], p[1] = v[1], p[2] = v[2], p[3] = v[3];
        return;
    }
#pragma unroll
    for (uint32_t i = 0; i < 4u; i++) { // the cropped end of a row: element loads
        const uint32_t lo = 2u * i < n ? gptr<const uint16_t>(src)[2u * i] : 0u;
        const uint32_t hi = 2u * i + 1u < n ? gptr<const uint16_t>(src)[2u * i + 1u] : 0u;
        p[i] = lo | (hi << 16);
    }
}

// The first n of 8 samples to dst.  NT: full pieces on the 16-byte grid go out as `sc1 nt` streaming stores (store_stream16), as
// the decode kernels use for rows that are written once.
template <bool NT>
__device__ __forceinline__ void store8(uint16_t *dst, uint32_t n, bool vec, const uint32_t p[4])
{
    MOS_PATH(MP_ST_VEC, n == 8u && vec);
    MOS_PATH(MP_ST_UNAL, n == 8u && !vec);
    MOS_PATH(MP_ST_ELEM, n != 8u);
    if (n == 8u) {
        if (vec) {
            const mcraw_u32x4 v = {p[0], p[1], p[2], p[3]};
            if (NT)
                store_stream16(dst, v);
            else
                *gptr<mcraw_u32x4>(dst) = v;
        } else { // rows off the 16-byte grid: one unaligned 16-byte store
            const u32x4_unaligned v = {p[0], p[1], p[2], p[3]};
            *gptr<u32x4_unaligned>(dst) = v;
        }
        return;
    }
#pragma unroll
    for (uint32_t i = 0; i < 8u; i++) // the cropped end of a row: element stores
        if (i < n)
            gptr<uint16_t>(dst)[i] = static_cast<uint16_t>(p[i >> 1] >> (16u * (i & 1u)));
}

// The stencil stages' tile: 256 threads, 32 lanes across with 8 columns each, and in LDS 8 columns either side of it so that
// the 16-byte chunks stay on the frame's 8-column grid.
constexpr int TILE_T = 256;
constexpr uint32_t TILE_W = 256u;
constexpr uint32_t TILE_LW = TILE_W + 16u; // samples per LDS row
constexpr uint32_t TILE_CH = TILE_LW / 8u; // 16-byte chunks per LDS row

// Stage the tile at (x0, y0) of a W x H frame with a halo of HALO (<= 8) rows and columns into s as raw samples: LDS row r, column
// k holds the sample for frame row y0 - HALO + r, column x0 - 8 + k.  MAP(h, n) names the frame coordinate whose sample a
// coordinate outside [0, n) stands for (the stage's reflection), so the stencil itself knows no edges.  Full pieces of a row are
// 16-byte loads (vec: they lie on the 16-byte grid); the halo columns (the last HALO of the first chunk, the first HALO of the
// last) and a cropped row end are element loads through MAP.  What no output of the frame reads is left as it is.
// (kfixpix stages with it.  kdenoise has the same loop written out: as a call it measured slower there)
template <uint32_t TH, int HALO, int (*MAP)(int, int)>
__device__ __forceinline__ void stage_tile(uint16_t *s, const uint16_t *in, size_t pitch, int W, int H, int x0, int y0, bool vec)
{
    constexpr uint32_t LH = TH + 2u * HALO;
    for (uint32_t i = threadIdx.x; i < LH * TILE_CH; i += TILE_T) {
        const uint32_t r = i / TILE_CH, q = i % TILE_CH;
        const int yy = y0 - HALO + static_cast<int>(r), xs = x0 - 8 + 8 * static_cast<int>(q);
        MOS_PATH(MP_STG_SKIP, yy >= H + HALO || xs >= W + HALO);
        if (yy >= H + HALO || xs >= W + HALO) // no output of the frame reads it
            continue;
        MOS_STAGE(q != 0u && q != TILE_CH - 1u, xs + 8 <= W, vec);
        const uint16_t *row = in + static_cast<size_t>(MAP(yy, H)) * pitch;
        mcraw_u32x4 v;
        if (q != 0u && q != TILE_CH - 1u && xs + 8 <= W) { // (xs >= 0 here) a full piece of the row
            v = load16(row + xs, vec);
        } else {
            const int e0 = q == 0u ? 8 - HALO : 0, e1 = q == TILE_CH - 1u ? HALO : 8;
            uint32_t u[8];
#pragma unroll
            for (int e = 0; e < 8; e++)
                u[e] = (e >= e0 && e < e1 && xs + e < W + HALO) ? gptr<const uint16_t>(row)[MAP(xs + e, W)] : 0u;
            v = mcraw_u32x4{u[0] | (u[1] << 16), u[2] | (u[3] << 16), u[4] | (u[5] << 16), u[6] | (u[7] << 16)};
        }
        *reinterpret_cast<mcraw_u32x4 *>(&s[r * TILE_LW + 8u * q]) = v;
    }
}

// `samples` (a multiple of 8) samples of an LDS tile buffer filled with 0xFFFF, and a barrier: what a test build puts in front
// of staging, so that the chunks that staging leaves as they are hold the most hostile value instead of what LDS held.
__device__ __forceinline__ void poison_tile(uint16_t *s, uint32_t samples)
{
    for (uint32_t i = threadIdx.x; i < samples / 8u; i += blockDim.x)
        *reinterpret_cast<mcraw_u32x4 *>(&s[8u * i]) = mcraw_u32x4{0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu};
    __syncthreads();
}

} // namespace mcraw
