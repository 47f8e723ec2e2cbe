// mcraw_rgb.hip -- gfx950 kernels for uint16 mosaics resident in HBM -> planar linear RGB (mcraw_demosaic_batch).
//
//   krgb_mhc   full resolution: Malvar-He-Cutler 5x5 gradient-corrected bilinear interpolation, in integers
//   krgb_bin2  half resolution: one output pixel per 2x2 CFA quad (R = r, G = mean(g1, g2), B = b)
//
// Both write (N, 3, Ho, Wo), channel-major per frame.  The arithmetic is the contract of include/mcraw_hip.h; the
// numpy statement of it is tests/_rgb_ref.py.  One instance per (dtype, CFA): the CFA decides at compile time which
// filter every lane slot runs.  CLIP is a wave-uniform run-time flag (v_med3_f32 under a uniform branch).
#include <cmath>

#include "mcraw_dev.h"
#include "mcraw_host.h"

namespace mcraw {

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
};

constexpr uint32_t RGB_T = 256;             // threads per workgroup
constexpr uint32_t MHC_TW = 256;            // tile columns: 32 lanes x 8
constexpr uint32_t MHC_TH = 32;             // tile rows: 8 row pairs x 2 passes
constexpr uint32_t MHC_LW = MHC_TW + 16;    // LDS row: 8 columns either side (2 used), so that chunks stay on the 8-grid
constexpr uint32_t MHC_LH = MHC_TH + 4;     // 2 halo rows above and below
constexpr uint32_t MHC_CH = MHC_LW / 8u;    // 16-byte chunks per LDS row

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

// E (3 channels x 8 pixels of one row) -> o_i = (m[3i] v0 + m[3i+1] v1) + m[3i+2] v2, v_c = (float)E_c * k[c], every
// product and sum rounded on its own (no FMA), optional clamp, stored as 8 consecutive elements of row y, column x, of each
// plane.  `n`: elements of the 8 that exist.
template <int PK>
__device__ __forceinline__ void rgb_store8(const RgbArgs &A, const RgbCol &col, uint8_t *frame_out, uint32_t y, uint32_t x,
                                           uint32_t n, const int (&E)[3][8])
{
#pragma clang fp contract(off)
    constexpr uint32_t ES = PK == PK_F32 ? 4u : 2u;
    float v[3][8], o[3][8];
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
#pragma unroll
            for (uint32_t h = 0; h < ES / 2u; h++) {
                const mcraw_u32x4 w = {e[4 * h], e[4 * h + 1], e[4 * h + 2], e[4 * h + 3]};
                if (ES == 2u)
                    store_stream16(dst + 16u * h, w);
                else
                    *gptr<mcraw_u32x4>(dst + 16u * h) = w;
            }
        } else { // a cropped row end, or a row off the 16-byte grid
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

// ---- MHC --------------------------------------------------------------------------------------------------------------
//
// A workgroup owns a tile of 256 columns x 32 rows of one frame.  It stages the tile and a 2-pixel halo (reflected at the
// frame edges) in LDS as raw samples, 16-byte chunks on the frame's 8-column grid.  Lane (lx, ly) then makes 8 columns of
// row pairs ly and ly + 8: four CFA quads, so every filter choice is fixed per lane slot by the CFA (template S: the RGGB
// role of CFA position p is p ^ S).  The halo rows are read again by the tiles above and below (L2 / Infinity Cache).
template <int PK, int S>
__global__ void __launch_bounds__(RGB_T) krgb_mhc(const RgbArgs A)
{
    __shared__ __attribute__((aligned(16))) uint16_t s_t[MHC_LH * MHC_LW];
    const uint32_t f = blockIdx.y, tx = blockIdx.x % A.tilesX, ty = blockIdx.x / A.tilesX;
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
        return;
    const uint32_t n = min(8u, A.W - x);
    const RgbCol &col = A.col[A.percol ? f : 0u];
    uint8_t *fout = A.out + static_cast<size_t>(f) * 3u * A.Ho * A.Wo * (PK == PK_F32 ? 4u : 2u);
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
            if (y + static_cast<uint32_t>(a) < A.H)
                rgb_store8<PK>(A, col, fout, y + static_cast<uint32_t>(a), x, n, E);
        }
    }
}

// ---- BIN2 -------------------------------------------------------------------------------------------------------------
//
// Lane = 8 consecutive output columns of one output row: 16 input columns of two input rows (two 16-byte loads per row
// where the rows allow it).
template <int PK, int S>
__global__ void __launch_bounds__(RGB_T) krgb_bin2(const RgbArgs A)
{
    const uint32_t f = blockIdx.y, item = blockIdx.x * RGB_T + threadIdx.x;
    const uint32_t yo = item / A.tilesX, xo = 8u * (item % A.tilesX);
    if (yo >= A.Ho)
        return;
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
    uint8_t *fout = A.out + static_cast<size_t>(f) * 3u * A.Ho * A.Wo * (PK == PK_F32 ? 4u : 2u);
    rgb_store8<PK>(A, A.col[A.percol ? f : 0u], fout, yo, xo, n, E);
}

typedef void (*RgbKernel)(const RgbArgs);

template <int PK>
static RgbKernel pick_kernel(uint32_t algo, int s)
{
    static const RgbKernel mhc[4] = {krgb_mhc<PK, 0>, krgb_mhc<PK, 1>, krgb_mhc<PK, 2>, krgb_mhc<PK, 3>};
    static const RgbKernel bin2[4] = {krgb_bin2<PK, 0>, krgb_bin2<PK, 1>, krgb_bin2<PK, 2>, krgb_bin2<PK, 3>};
    return algo == MCRAW_RGB_MHC ? mhc[s] : bin2[s];
}

static int reject(const char *why)
{
    g_err = std::string("mcraw_demosaic_batch: ") + why;
    return -1;
}

static bool finite_all(const float *v, int n)
{
    for (int i = 0; i < n; i++)
        if (!std::isfinite(v[i]))
            return false;
    return true;
}

} // namespace mcraw

using namespace mcraw;

extern "C" {

int mcraw_demosaic_batch(mcraw_ctx *c, const mcraw_rgb *p, const mcraw_rgb_color *colors, int ncolors, const uint16_t *in,
                         size_t in_pitch, size_t in_frame_stride, int width, int height, int n, void *out, size_t out_bytes,
                         void *stream)
{
    if (!c || !p || n < 0)
        return reject("bad arguments");
    if (n == 0)
        return 0;
    if (width < 4 || height < 4 || (width & 1) || (height & 1) || width > 65536 || height > 65536)
        return reject("width and height must be even, 4 .. 65536");
    if (in_pitch < static_cast<size_t>(width))
        return reject("in_pitch below width");
    if (n > 1 && in_frame_stride < (static_cast<size_t>(height) - 1u) * in_pitch + static_cast<size_t>(width))
        return reject("in_frame_stride too small for the frames not to overlap");
    if (p->algo != MCRAW_RGB_MHC && p->algo != MCRAW_RGB_BIN2)
        return reject("unknown algo");
    if (p->dtype != MCRAW_FLOAT_F32 && p->dtype != MCRAW_FLOAT_F16 && p->dtype != MCRAW_FLOAT_BF16)
        return reject("unknown dtype");
    if (p->cfa > MCRAW_CFA_GBRG)
        return reject("unknown cfa");
    if (p->flags & ~MCRAW_FLOAT_CLIP)
        return reject("unknown flag");
    const float bsum = static_cast<float>(static_cast<int>(p->black[0]) + p->black[1] + p->black[2] + p->black[3]);
    if (!std::isfinite(p->white) || !(p->white > 0.25f * bsum))
        return reject("white must be finite and above the mean black level");
    if (!colors || (ncolors != 1 && ncolors != n))
        return reject("ncolors must be 1 or n");
    for (int i = 0; i < ncolors; i++)
        if (!finite_all(colors[i].gain, 3) || !finite_all(colors[i].m, 9))
            return reject("non-finite gain or matrix entry");
    const bool mhc = p->algo == MCRAW_RGB_MHC;
    const size_t es = p->dtype == MCRAW_FLOAT_F32 ? 4u : 2u;
    const size_t Wo = mhc ? static_cast<size_t>(width) : static_cast<size_t>(width) / 2u;
    const size_t Ho = mhc ? static_cast<size_t>(height) : static_cast<size_t>(height) / 2u;
    if (out_bytes / es / 3u / Ho / Wo < static_cast<size_t>(n))
        return reject("out_bytes below n * 3 * Ho * Wo * element size");
    if (!in || !out || (reinterpret_cast<uintptr_t>(in) & 1u) || (reinterpret_cast<uintptr_t>(out) & (es - 1u)))
        return reject("in / out missing or not aligned to their element size");

    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    hipStream_t st = stream ? static_cast<hipStream_t>(stream) : c->stream;
    // (the division is in f32, as every step of the host side of the contract)
    const float inv = 1.0f / (p->white - 0.25f * bsum);
    const float scale = mhc ? 0.0625f : 0.5f;
    std::vector<RgbCol> cols(static_cast<size_t>(ncolors));
    for (int i = 0; i < ncolors; i++) {
        for (int k = 0; k < 3; k++)
            cols[static_cast<size_t>(i)].k[k] = (colors[i].gain[k] * inv) * scale;
        std::memcpy(cols[static_cast<size_t>(i)].m, colors[i].m, sizeof(float) * 9);
    }
    static const int shift_of[4] = {0, 3, 1, 2}; // MCRAW_CFA_* -> role shift: RGGB 0, BGGR 3, GRBG 1, GBRG 2
    const int s = shift_of[p->cfa];
    RgbKernel k = p->dtype == MCRAW_FLOAT_F32 ? pick_kernel<PK_F32>(p->algo, s)
                  : p->dtype == MCRAW_FLOAT_F16 ? pick_kernel<PK_F16>(p->algo, s)
                                                : pick_kernel<PK_BF16>(p->algo, s);
    RgbArgs A{};
    A.pitch = in_pitch;
    A.fstride = in_frame_stride;
    A.W = static_cast<uint32_t>(width);
    A.H = static_cast<uint32_t>(height);
    A.Wo = static_cast<uint32_t>(Wo);
    A.Ho = static_cast<uint32_t>(Ho);
    A.invec = (reinterpret_cast<uintptr_t>(in) & 15u) == 0u && in_pitch % 8u == 0u && (n == 1 || in_frame_stride % 8u == 0u);
    A.clip = (p->flags & MCRAW_FLOAT_CLIP) ? 1u : 0u;
    A.percol = ncolors > 1 ? 1u : 0u;
    for (int i = 0; i < 4; i++)
        A.black[i] = p->black[i];
    uint32_t blocks;
    if (mhc) {
        A.tilesX = static_cast<uint32_t>((width + MHC_TW - 1) / MHC_TW);
        blocks = A.tilesX * static_cast<uint32_t>((height + MHC_TH - 1) / MHC_TH);
    } else {
        A.tilesX = static_cast<uint32_t>((Wo + 7u) / 8u);
        blocks = static_cast<uint32_t>((static_cast<size_t>(A.tilesX) * Ho + RGB_T - 1u) / RGB_T);
    }
    const int kid = mhc ? MCRAW_KRGB_MHC : MCRAW_KRGB_BIN2;
    const int piece = A.percol ? RGB_MAXF : 65535;
    const size_t out_frame = 3u * Ho * Wo * es;
    for (int f0 = 0; f0 < n; f0 += piece) {
        const int nf = std::min(piece, n - f0);
        A.in = in + static_cast<size_t>(f0) * in_frame_stride;
        A.out = static_cast<uint8_t *>(out) + static_cast<size_t>(f0) * out_frame;
        for (int i = 0; i < (A.percol ? nf : 1); i++)
            A.col[i] = cols[static_cast<size_t>(A.percol ? f0 + i : 0)];
        KTimer kt(c, kid, st);
        hipLaunchKernelGGL(k, dim3(blocks, static_cast<uint32_t>(nf)), dim3(RGB_T), 0, st, A);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

} // extern "C"
