// mcraw_rgb_dev.h -- the device code that every demosaic kernel shares (csrc/mcraw_rgb.hip: krgb_mhc, krgb_bin2;
// csrc/mcraw_area.hip: krgb_area; csrc/mcraw_resample.hip: krgb_resample): the kernel arguments, the colour stage and the stores
// of the float, display and YUV families, and the LUT staging.  Moved here from mcraw_rgb.hip as it stood:
// tools/rgb_resources.py --check holds every instance of those files to its committed figures.  The host side that the three
// files share: mcraw_rgb_launch.h.
#pragma once
#include "mcraw_dev.h"
#include "mcraw_host.h"
#include "mcraw_rgb_args.h"

// The hooks of the path census (csrc/mcraw_rgb_paths.h; tests/test_gpu_rgb_paths.py): empty unless a source defines them in front
// of this header, so that this header names no switch of a test build.
//   RGB_PATH(slot, cond)            the active lanes for which `cond` holds take path `slot`
//   RGB_PATH_YUV(slot, dst, n, es)  8 samples of a YUV row at dst: the form yuv_store8 takes
//   RGB_WALK_DECL, RGB_WALK(family, f, lut, lutg)   a workgroup takes a unit of frame f
//   RGB_PATH_UNIT(slot, cond)       the workgroup's unit takes path `slot` (`cond` is uniform over the workgroup)
//   HA_PICKS(site, Da, Db, on)      the active lanes for which `on` holds call ha_pick(.., Da, .., Db) at call site `site`
#ifndef RGB_PATH
#define RGB_PATH(slot, cond)
#define RGB_PATH_UNIT(slot, cond)
#define HA_PICKS(site, Da, Db, on)
#define RGB_PATH_YUV(slot, dst, n, es)
#define RGB_WALK_DECL
#define RGB_WALK(family, f, lut, lutg)
#endif

namespace mcraw {

static_assert(rgb_float_kind(MCRAW_FLOAT_F32) == PK_F32 && rgb_float_kind(MCRAW_FLOAT_F16) == PK_F16 &&
                  rgb_float_kind(MCRAW_FLOAT_BF16) == PK_BF16, "mcraw_rgb_args.h names the float kinds of mcraw_plan.h");

// per-frame colour as the kernels take it: k[c] = (gain[c] * inv) * scale, and the 3x3 matrix, row-major
struct RgbCol {
    float k[3];
    float m[9];
};
// Colours travel inside the kernel arguments, which the runtime copies when the launch is queued: two batches queued
// back to back, on one stream or on two, can never see each other's values.  A batch with per-frame colours is launched
// in pieces of RGB_MAXF frames.
constexpr int RGB_MAXF = 32;

struct RgbArgs {
    const uint16_t *in;
    uint8_t *out;
    uint64_t pitch, fstride; // input, in uint16 elements
    uint32_t W, H, Wo, Ho;
    uint32_t tilesX; // MHC: tiles per row band; BIN2: groups of 8 output columns per output row
    uint32_t invec;  // every input row starts on a 16-byte boundary: 16-byte loads
    uint32_t clip, percol;
    int32_t black[4];
    RgbCol col[RGB_MAXF];
    // display kinds only (behind the float kinds' fields, which keep their offsets)
    const uint16_t *lut; // the transfer-curve LUT (caller's device memory, 16-byte aligned)
    uint32_t lutn;       // LUT entries L (a power of two, 256 .. 65536)
    uint32_t lutg;       // the LUT is read from global memory (L > DISP_LDS_MAX) rather than staged in LDS
    uint32_t hwc;        // (n, Ho, Wo, 3) rather than (n, 3, Ho, Wo)
    uint32_t units, nf;  // tiles (MHC) or workgroups' items (BIN2) per frame; frames in this launch
    // YUV kinds only (behind everything else)
    int32_t ycf[9];      // cy, cb, cr
    uint32_t ymask, ysh; // (1 << in_bits) - 1; sh
    int32_t yoff, coff;
};

// (RGB_T threads per workgroup, tiles of MHC_TW x MHC_TH, the output kinds PK_*: mcraw_rgb_args.h)
constexpr uint32_t MHC_LW = MHC_TW + 16;    // LDS row: 8 columns either side (2 used), so that chunks stay on the 8-grid
constexpr uint32_t MHC_LH = MHC_TH + 4;     // 2 halo rows above and below
constexpr uint32_t MHC_CH = MHC_LW / 8u;    // 16-byte chunks per LDS row

constexpr uint32_t DISP_LDS_MAX = 4096; // LUTs up to this many entries (8 KiB) are staged in LDS

static __device__ __forceinline__ int reflect101(int i, int n)
{
    // -k -> k, n-1+k -> n-1-k (keeps the CFA parity for k <= 2); anything further (never used by an output) is clamped
    i = i < 0 ? -i : i;
    i = i > n - 1 ? 2 * (n - 1) - i : i;
    return min(max(i, 0), n - 1);
}

template <int PK>
__device__ __forceinline__ uint32_t bits16(float v)
{
    if (PK == PK_F16)
        return __builtin_bit_cast(uint16_t, static_cast<_Float16>(v));
    return __builtin_bit_cast(uint16_t, static_cast<__bf16>(v));
}

// The colour stage every output kind shares: E (3 channels x 8 pixels of one row) -> o_i = (m[3i] v0 + m[3i+1] v1) + m[3i+2] v2,
// v_c = (float)E_c * k[c], every product and sum rounded on its own (no FMA).
__device__ __forceinline__ void rgb_color8(const RgbCol &col, const int (&E)[3][8], float (&o)[3][8])
{
#pragma clang fp contract(off)
    float v[3][8];
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int i = 0; i < 8; i++)
            v[c][i] = static_cast<float>(E[c][i]) * col.k[c];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const float a = col.m[3 * r] * v[0][i], b = col.m[3 * r + 1] * v[1][i], c = col.m[3 * r + 2] * v[2][i];
            o[r][i] = (a + b) + c;
        }
}

// The float kinds: the colour stage, the optional clamp, then 8 consecutive elements of row y, column x, of each plane.
// `n`: elements of the 8 that exist.
template <int PK>
__device__ __forceinline__ void rgb_store8(const RgbArgs &A, const RgbCol &col, uint8_t *frame_out, uint32_t y, uint32_t x,
                                           uint32_t n, const int (&E)[3][8])
{
#pragma clang fp contract(off)
    constexpr uint32_t ES = PK == PK_F32 ? 4u : 2u;
    float o[3][8];
    rgb_color8(col, E, o);
    if (A.clip) {
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int i = 0; i < 8; i++)
                o[r][i] = __builtin_amdgcn_fmed3f(o[r][i], 0.0f, 1.0f);
    }
    const size_t plane = static_cast<size_t>(A.Ho) * A.Wo;
#pragma unroll
    for (int r = 0; r < 3; r++) {
        uint8_t *dst = frame_out + (r * plane + static_cast<size_t>(y) * A.Wo + x) * ES;
        uint32_t e[8];
        if (ES == 4u) {
#pragma unroll
            for (int i = 0; i < 8; i++)
                e[i] = __builtin_bit_cast(uint32_t, o[r][i]);
        } else {
#pragma unroll
            for (int i = 0; i < 4; i++)
                e[i] = bits16<PK>(o[r][2 * i]) | (bits16<PK>(o[r][2 * i + 1]) << 16);
        }
        if (n == 8u && (reinterpret_cast<uintptr_t>(dst) & 15u) == 0u) {
            // f16 / bf16: 16 bytes per lane, whole lines per instruction: streaming stores.  f32: each instruction covers half
            // of every 32-byte lane piece; streamed, those half lines reach HBM on their own (6x slower, measured): plain
            // stores, which L2 merges.
            RGB_PATH(RP_ST_F_FAST, true);
#pragma unroll
            for (uint32_t h = 0; h < ES / 2u; h++) {
                const mcraw_u32x4 w = {e[4 * h], e[4 * h + 1], e[4 * h + 2], e[4 * h + 3]};
                if (ES == 2u)
                    store_stream16(dst + 16u * h, w);
                else
                    *gptr<mcraw_u32x4>(dst + 16u * h) = w;
            }
        } else { // a cropped row end, or a row off the 16-byte grid
            RGB_PATH(RP_ST_F_CROP, n != 8u);
            RGB_PATH(RP_ST_F_OFF, n == 8u);
#pragma unroll
            for (uint32_t i = 0; i < 8u; i++)
                if (i < n) {
                    if (ES == 4u)
                        gptr<uint32_t>(dst)[i] = e[i];
                    else
                        gptr<uint16_t>(dst)[i] = static_cast<uint16_t>(e[i >> 1] >> (16u * (i & 1u)));
                }
        }
    }
}

// The display stage: the colour stage, then per sample c = o > 0 ? min(o, 1) : 0 (NaN -> 0), i = rint(c * (L - 1)) (one
// f32 multiply, RNE), q = lut[i] (the low byte for uint8).  The LUT is read from LDS (s_lut, staged by the kernel) or,
// for L > DISP_LDS_MAX, from global memory through L1 / L2.  Stores, plain (each instruction covers only part of the
// lines it touches in HWC):
//   CHW  u8: 8 B per plane (8-byte aligned); u16: 16 B per plane (16-byte aligned)
//   HWC  u8: 24 B per lane as 16 + 8 B, in whichever order keeps the 16-byte store 16-byte aligned (8-byte aligned rows);
//        u16: 48 B per lane as three 16-byte stores (16-byte aligned rows)
//   element stores for a cropped row end and for rows off those grids
// (disp_lookup8: everything up to the LUT entry q, which the YUV kinds share)
__device__ __forceinline__ void disp_lookup8(const RgbArgs &A, const RgbCol &col, const uint16_t *s_lut, const int (&E)[3][8],
                                             uint32_t (&q)[3][8])
{
#pragma clang fp contract(off)
    float o[3][8];
    rgb_color8(col, E, o);
    const float lf = static_cast<float>(A.lutn - 1u);
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int i = 0; i < 8; i++) {
            const float c = o[r][i] > 0.0f ? fminf(o[r][i], 1.0f) : 0.0f;
            q[r][i] = static_cast<uint32_t>(rintf(c * lf));
        }
    if (A.lutg) {
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int i = 0; i < 8; i++)
                q[r][i] = gptr<const uint16_t>(A.lut)[q[r][i]];
    } else {
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int i = 0; i < 8; i++)
                q[r][i] = s_lut[q[r][i]];
    }
}

template <int PK>
__device__ __forceinline__ void disp_store8(const RgbArgs &A, const RgbCol &col, const uint16_t *s_lut, uint8_t *frame_out,
                                            uint32_t y, uint32_t x, uint32_t n, const int (&E)[3][8])
{
    constexpr uint32_t ES = out_es(PK);
    uint32_t q[3][8];
    disp_lookup8(A, col, s_lut, E, q);
    if (ES == 1u) {
#pragma unroll
        for (int r = 0; r < 3; r++)
#pragma unroll
            for (int i = 0; i < 8; i++)
                q[r][i] &= 0xffu;
    }
    const bool full = n == 8u;
    if (A.hwc) {
        uint8_t *dst = frame_out + (static_cast<size_t>(y) * A.Wo + x) * 3u * ES;
        const uintptr_t a = reinterpret_cast<uintptr_t>(dst);
        if (ES == 1u) {
            uint32_t w[6] = {0, 0, 0, 0, 0, 0}; // byte j: pixel j / 3, channel j % 3
#pragma unroll
            for (int j = 0; j < 24; j++)
                w[j >> 2] |= q[j % 3][j / 3] << (8 * (j & 3));
            if (full && (a & 7u) == 0u) {
                if ((a & 8u) == 0u) {
                    RGB_PATH(RP_ST_H8_16_8, true);
                    *gptr<mcraw_u32x4>(dst) = mcraw_u32x4{w[0], w[1], w[2], w[3]};
                    *gptr<mcraw_u32x2>(dst + 16) = mcraw_u32x2{w[4], w[5]};
                } else {
                    RGB_PATH(RP_ST_H8_8_16, true);
                    *gptr<mcraw_u32x2>(dst) = mcraw_u32x2{w[0], w[1]};
                    *gptr<mcraw_u32x4>(dst + 8) = mcraw_u32x4{w[2], w[3], w[4], w[5]};
                }
            } else {
                RGB_PATH(RP_ST_H8_ELEM, true);
#pragma unroll
                for (uint32_t i = 0; i < 8u; i++)
                    if (i < n) {
#pragma unroll
                        for (uint32_t c = 0; c < 3u; c++)
                            gptr<uint8_t>(dst)[3u * i + c] = static_cast<uint8_t>(q[c][i]);
                    }
            }
        } else {
            uint32_t w[12]; // uint16 j: pixel j / 3, channel j % 3
#pragma unroll
            for (int k = 0; k < 12; k++)
                w[k] = q[(2 * k) % 3][(2 * k) / 3] | (q[(2 * k + 1) % 3][(2 * k + 1) / 3] << 16);
            if (full && (a & 15u) == 0u) {
                RGB_PATH(RP_ST_H16_FAST, true);
#pragma unroll
                for (int h = 0; h < 3; h++)
                    *gptr<mcraw_u32x4>(dst + 16 * h) = mcraw_u32x4{w[4 * h], w[4 * h + 1], w[4 * h + 2], w[4 * h + 3]};
            } else {
                RGB_PATH(RP_ST_H16_ELEM, true);
#pragma unroll
                for (uint32_t i = 0; i < 8u; i++)
                    if (i < n) {
#pragma unroll
                        for (uint32_t c = 0; c < 3u; c++)
                            gptr<uint16_t>(dst)[3u * i + c] = static_cast<uint16_t>(q[c][i]);
                    }
            }
        }
        return;
    }
    const size_t plane = static_cast<size_t>(A.Ho) * A.Wo;
#pragma unroll
    for (int r = 0; r < 3; r++) { // (yuv_store8 per plane, written out: calling it changes the schedule of 12 instances)
        uint8_t *dst = frame_out + (r * plane + static_cast<size_t>(y) * A.Wo + x) * ES;
        const uintptr_t a = reinterpret_cast<uintptr_t>(dst);
        if (ES == 1u) {
            const uint32_t w0 = q[r][0] | (q[r][1] << 8) | (q[r][2] << 16) | (q[r][3] << 24);
            const uint32_t w1 = q[r][4] | (q[r][5] << 8) | (q[r][6] << 16) | (q[r][7] << 24);
            if (full && (a & 7u) == 0u) {
                RGB_PATH(RP_ST_C8_FAST, true);
                *gptr<mcraw_u32x2>(dst) = mcraw_u32x2{w0, w1};
            } else {
                RGB_PATH(RP_ST_C8_CROP, !full);
                RGB_PATH(RP_ST_C8_OFF, full);
#pragma unroll
                for (uint32_t i = 0; i < 8u; i++)
                    if (i < n)
                        gptr<uint8_t>(dst)[i] = static_cast<uint8_t>(q[r][i]);
            }
        } else {
            if (full && (a & 15u) == 0u) {
                RGB_PATH(RP_ST_C16_FAST, true);
                *gptr<mcraw_u32x4>(dst) = mcraw_u32x4{q[r][0] | (q[r][1] << 16), q[r][2] | (q[r][3] << 16),
                                                      q[r][4] | (q[r][5] << 16), q[r][6] | (q[r][7] << 16)};
            } else {
                RGB_PATH(RP_ST_C16_CROP, !full);
                RGB_PATH(RP_ST_C16_OFF, full);
#pragma unroll
                for (uint32_t i = 0; i < 8u; i++)
                    if (i < n)
                        gptr<uint16_t>(dst)[i] = static_cast<uint16_t>(q[r][i]);
            }
        }
    }
}

// 8 consecutive samples (n of them exist) of one row of a YUV plane: one 8-byte (uint8) or 16-byte (uint16) store on
// natural alignment, element stores for a cropped row end or an address off that grid.
template <uint32_t ES>
__device__ __forceinline__ void yuv_store8(uint8_t *dst, uint32_t n, const uint32_t (&v)[8])
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(dst);
    if (ES == 1u) {
        if (n == 8u && (a & 7u) == 0u) {
            *gptr<mcraw_u32x2>(dst) = mcraw_u32x2{v[0] | (v[1] << 8) | (v[2] << 16) | (v[3] << 24),
                                                  v[4] | (v[5] << 8) | (v[6] << 16) | (v[7] << 24)};
        } else {
#pragma unroll
            for (uint32_t i = 0; i < 8u; i++)
                if (i < n)
                    gptr<uint8_t>(dst)[i] = static_cast<uint8_t>(v[i]);
        }
    } else {
        if (n == 8u && (a & 15u) == 0u) {
            *gptr<mcraw_u32x4>(dst) = mcraw_u32x4{v[0] | (v[1] << 16), v[2] | (v[3] << 16), v[4] | (v[5] << 16), v[6] | (v[7] << 16)};
        } else {
#pragma unroll
            for (uint32_t i = 0; i < 8u; i++)
                if (i < n)
                    gptr<uint16_t>(dst)[i] = static_cast<uint16_t>(v[i]);
        }
    }
}

// The YUV stage of row `a` (0 or 1) of a row pair: the display stage up to the LUT entry, P = entry & mask, then
//   Y = clamp(((cy . P + (1 << (sh - 1))) >> sh) + y_off, 0, top), stored at once;
// S (the sums of P over the lane's four 2x2 blocks) takes the row, and behind row 1
//   Cb, Cr = clamp(((c . S + (1 << (sh + 1))) >> (sh + 2)) + c_off, 0, top), stored as four (Cb, Cr) pairs.
// The host's overflow rule keeps every coefficient below 2^22 in magnitude and every sum inside int32; P < 2^16 and
// S < 2^18: the products are exact as 24-bit multiplies (v_mad_i32_i24, full rate; v_mul_lo_u32 is quarter rate).
template <int PK>
__device__ __forceinline__ void yuv_row8(const RgbArgs &A, const RgbCol &col, const uint16_t *s_lut, uint8_t *frame_out,
                                         uint32_t y, uint32_t x, uint32_t n, int a, const int (&E)[3][8], int (&S)[3][4])
{
    constexpr uint32_t ES = out_es(PK);
    constexpr int TOP = PK == PK_NV12 ? 255 : 1023, SHL = PK == PK_NV12 ? 0 : 6;
    uint32_t q[3][8];
    disp_lookup8(A, col, s_lut, E, q);
    int P[3][8];
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int i = 0; i < 8; i++)
            P[c][i] = static_cast<int>(q[c][i] & A.ymask);
    const int rnd = 1 << (A.ysh - 1u);
    uint32_t v[8];
#pragma unroll
    for (int i = 0; i < 8; i++) {
        const int s = __mul24(A.ycf[0], P[0][i]) + __mul24(A.ycf[1], P[1][i]) + __mul24(A.ycf[2], P[2][i]) + rnd;
        v[i] = static_cast<uint32_t>(min(max((s >> A.ysh) + A.yoff, 0), TOP)) << SHL;
    }
    RGB_PATH_YUV(RP_ST_YL_FAST, frame_out + (static_cast<size_t>(y) * A.Wo + x) * ES, n, ES);
    yuv_store8<ES>(frame_out + (static_cast<size_t>(y) * A.Wo + x) * ES, n, v);
#pragma unroll
    for (int c = 0; c < 3; c++)
#pragma unroll
        for (int k = 0; k < 4; k++)
            S[c][k] += P[c][2 * k] + P[c][2 * k + 1];
    if (a == 0)
        return;
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
        for (int r = 1; r < 3; r++) {
            const int s = __mul24(A.ycf[3 * r], S[0][k]) + __mul24(A.ycf[3 * r + 1], S[1][k]) + __mul24(A.ycf[3 * r + 2], S[2][k]) +
                          4 * rnd;
            v[2 * k + r - 1] = static_cast<uint32_t>(min(max((s >> (A.ysh + 2u)) + A.coff, 0), TOP)) << SHL;
        }
    RGB_PATH_YUV(RP_ST_YC_FAST, frame_out + ((static_cast<size_t>(A.Ho) + (y >> 1)) * A.Wo + x) * ES, n, ES);
    yuv_store8<ES>(frame_out + ((static_cast<size_t>(A.Ho) + (y >> 1)) * A.Wo + x) * ES, n, v);
}

// (test builds of the kernels) The workgroup fills an LDS array with `pattern`; the caller syncs.
__device__ __forceinline__ void rgb_poison(void *a, uint32_t bytes, uint32_t pattern)
{
    for (uint32_t i = threadIdx.x; i < bytes / 4u; i += RGB_T)
        static_cast<uint32_t *>(a)[i] = pattern;
}

// A display kernel's workgroup stages an LDS-sized LUT once, before its first tile (the caller syncs).
__device__ __forceinline__ void stage_lut(const RgbArgs &A, uint16_t *s_lut)
{
    if (A.lutg)
        return;
    for (uint32_t i = threadIdx.x; i < A.lutn / 8u; i += RGB_T)
        *reinterpret_cast<mcraw_u32x4 *>(&s_lut[8u * i]) = gptr<const mcraw_u32x4>(A.lut)[i];
}

} // namespace mcraw
