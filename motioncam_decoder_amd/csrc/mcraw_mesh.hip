// mcraw_mesh.hip -- gfx950 kernels for uint16 mosaics resident in HBM -> RGB sampled along one displacement mesh per frame
// (mcraw_demosaic_mesh_batch): krgb_warp (csrc/mcraw_warp.hip) with the position of every pixel interpolated from the four nodes
// of its tile's cell, read from device memory, instead of an affine map in the kernel arguments.  The contract:
// include/mcraw_hip.h; the checks, the position arithmetic, the window and its clamps, free of HIP: mcraw_mesh_args.h; the numpy
// statement: tests/_mesh_ref.py.  Staging, phase A, the weights, the taps and the store phase are shared with krgb_warp (mcraw_warp_dev.h); the colour stage
// and the stores are the siblings' (mcraw_rgb_dev.h), the host side of the launch theirs too (mcraw_rgb_launch.h).
//
//   krgb_mesh  one instance per (output kind, CFA), as the siblings
//
// A workgroup owns a tile of WARP_TW x WARP_TH output pixels, which is one cell of the mesh.
//   nodes   the cell's four nodes, uniform over the workgroup; the window from the clamped positions of the tile's four corner
//           pixels, cut to the LDS arrays (np', ne')
//   stage, A, store   krgb_warp's
//   gather  a lane takes 4 output columns of an output row: they share u, so the row's two ends are formed once; the sums run in
//           32 bits relative to the first node where the cell allows it (mesh_narrow: every cell of the regime does), in 64 bits
//           otherwise -- both equal the contract's 64-bit statement (tests/cpp/mesh_args_check.cpp) --, then the per-pixel
//           clamp to the frame and the clamp of the tap origin into the window
// No node content can make a read leave the LDS arrays or the frame's reflection: the kernel depends on no validation.
#ifdef MCRAW_PATHSR // (the test builds' switches: the head of mcraw_rgb.hip; the grid's cap comes from that source, below)
#define RGB_GATHER_FAMILY 1u
#include "mcraw_rgb_paths.h"
#endif
#include "mcraw_dev.h"
#include "mcraw_host.h"
#include "mcraw_rgb_args.h"
#include "mcraw_rgb_dev.h"
// The persistent grid's limit is mcraw_rgb.hip's, as for krgb_warp: this unit does not name the cap's switch
// (tests/test_gpu_mesh_paths.py).
namespace mcraw {
uint32_t rgb_grid_limit(uint32_t resident);
}
#define RGB_GRID_LIMIT(resident) ::mcraw::rgb_grid_limit(resident)
#include "mcraw_rgb_launch.h"
#include "mcraw_mesh_args.h"
#include "mcraw_warp_dev.h"

namespace mcraw {

struct MeshGeo {
    const int32_t *nodes; // the mesh of this launch's first frame (permesh), or the batch's
    uint32_t permesh;
    uint32_t tilesX;
    uint32_t Mx;          // nodes per row of a mesh
    uint32_t stride;      // int32 per mesh: 2 My Mx
    uint32_t filter;
};

__device__ const WarpTable g_mesh_cubic = warp_table(MCRAW_FILTER_CUBIC);

template <int PK, int S>
__global__ void __launch_bounds__(RGB_T) krgb_mesh(const RgbArgs A, const MeshGeo G)
{
    constexpr bool LUT = has_lut(PK);
    __shared__ __attribute__((aligned(16))) uint16_t s_raw[WARP_RAWH * WARP_RAWW];
    __shared__ __attribute__((aligned(16))) int32_t s_e[3u * WARP_EROWS * WARP_ESTRIDE];
    __shared__ __attribute__((aligned(16))) int16_t s_w[256u * 4u];
    __shared__ __attribute__((aligned(16))) uint16_t s_lut[LUT ? DISP_LDS_MAX : 8u];
    uint32_t t = blockIdx.x;
    RGB_WALK_DECL;
    if constexpr (LUT)
        stage_lut(A, s_lut);
    for (uint32_t i = threadIdx.x; i < 256u; i += RGB_T) { // the phase table in use: four int16 per phase
        mcraw_u32x2 v;
        if (G.filter == MCRAW_FILTER_LINEAR)
            v = mcraw_u32x2{(16u * (256u - i)) << 16, 16u * i};
        else
            v = *reinterpret_cast<const mcraw_u32x2 *>(g_mesh_cubic.w[i]);
        *reinterpret_cast<mcraw_u32x2 *>(&s_w[4u * i]) = v;
    }
    const int W = static_cast<int>(A.W), H = static_cast<int>(A.H);
    do {
        const uint32_t f = LUT ? t / A.units : blockIdx.y, u = LUT ? t % A.units : blockIdx.x;
        RGB_WALK(RF_MESH, f, LUT, A.lutg);
        const uint32_t tx = u % G.tilesX, ty = u / G.tilesX;
        const uint32_t k0 = tx * WARP_TW, k1 = min(k0 + WARP_TW, A.Wo) - 1u; // the tile's first and last column
        const uint32_t i0 = ty * WARP_TH, i1 = min(i0 + WARP_TH, A.Ho) - 1u; // ... and row
        // the cell's nodes (00, 01, 10, 11): the same addresses in every lane
        const int32_t *nd = G.nodes + (G.permesh ? static_cast<size_t>(f) * G.stride : 0u) + 2u * (static_cast<size_t>(ty) * G.Mx + tx);
        typedef uint32_t u32x4_n __attribute__((ext_vector_type(4), aligned(8))); // two nodes: a mesh is 8-byte aligned
        const u32x4_n n0 = *gptr<const u32x4_n>(nd), n1 = *gptr<const u32x4_n>(nd + 2u * G.Mx);
        const int32_t cy[4] = {static_cast<int32_t>(n0[0]), static_cast<int32_t>(n0[2]), static_cast<int32_t>(n1[0]), static_cast<int32_t>(n1[2])};
        const int32_t cx[4] = {static_cast<int32_t>(n0[1]), static_cast<int32_t>(n0[3]), static_cast<int32_t>(n1[1]), static_cast<int32_t>(n1[3])};
        // the estimates the tile needs: from row pb (even) and column eb (on the 8-grid) of the frame on, np row pairs and ne
        // pieces of 8 columns, cut to the arrays (tests/cpp/mesh_args_check.cpp holds every index against them for any nodes)
        const WarpWin win = mesh_window(cy, cx, i1 - i0, k1 - k0, W, H);
        const int32_t pb = win.pb, eb = win.eb;
        const uint32_t np = min(win.np, MESH_NP), ne = min(win.ne, MESH_NE);
        const int32_t rmax = mesh_tap_max_row(win.np), cmax = mesh_tap_max_col(win.ne);
        const bool narrow = mesh_narrow(cy) && mesh_narrow(cx);
        RGB_PATH_UNIT(RP_MESH_NARROW, narrow);
        RGB_PATH_UNIT(RP_MESH_WIDE, !narrow);
        const uint16_t *in = A.in + static_cast<size_t>(f) * A.fstride;
        __syncthreads(); // the LUT and the table are staged; the previous tile's LDS reads are done
#ifdef MCRAW_POISON_RGB
        // the raw window as the siblings'; an estimate of 0x5a5a5b lies above every value of phase A (< 2^22) and inside the taps'
        // bounds (|v >> 8| < 2^15): a stray read changes bytes and overflows nothing
        rgb_poison(s_raw, sizeof(s_raw), 0x5a5a5a5bu);
        rgb_poison(s_e, sizeof(s_e), 0x005a5a5bu);
        __syncthreads();
#endif
        WARP_UNIT(RPG_CUT_ROWS, np < win.np);
        WARP_UNIT(RPG_CUT_COLS, ne < win.ne);
        warp_stage(A, in, s_raw, pb, eb, np, ne, W, H); // raw rows pb - 2 .. pb + 2 np + 1, columns eb - 8 .. eb + 8 ne + 7
        __syncthreads();
        // A: rows of parity 0 in the first half of the workgroup, of parity 1 in the second (uniform in a wave)
        if (threadIdx.x < RGB_T / 2u) {
            for (uint32_t it = threadIdx.x; it < np * ne; it += RGB_T / 2u) {
                WARP_PATH(RPG_A_EVEN, true);
                warp_mhc_row<S, 0>(A, s_raw, s_e, it / ne, it % ne);
            }
        } else {
            for (uint32_t it = threadIdx.x - RGB_T / 2u; it < np * ne; it += RGB_T / 2u) {
                WARP_PATH(RPG_A_ODD, true);
                warp_mhc_row<S, 1>(A, s_raw, s_e, it / ne, it % ne);
            }
        }
        __syncthreads();
        // gather: a lane takes 4 output columns of one output row: every lane of the workgroup has its pixels
        {
            const uint32_t gr = threadIdx.x / (WARP_TW / 4u), gc = 4u * (threadIdx.x % (WARP_TW / 4u));
            const uint32_t j = i0 + gr, x = k0 + gc;
            int32_t E4[3][4] = {};
            WARP_PATH(RPG_PIX, j <= i1 && x <= k1);
            WARP_PATH(RPG_NOPIX, !(j <= i1 && x <= k1));
            if (j <= i1 && x <= k1) {
                int32_t Ys[4], Xs[4]; // the lane's four positions: a uniform choice between the two forms of the same sum
                if (narrow) {
                    int32_t ly, ry, lx, rx;
                    mesh_row32(cy, gr, ly, ry);
                    mesh_row32(cx, gr, lx, rx);
#pragma unroll
                    for (uint32_t i = 0; i < 4u; i++) {
                        Ys[i] = mesh_clamp32(mesh_lerp32(cy[0], ly, ry, gc + i), H);
                        Xs[i] = mesh_clamp32(mesh_lerp32(cx[0], lx, rx, gc + i), W);
                        RGB_PATH(RP_MESH_Y_LO, mesh_lerp32(cy[0], ly, ry, gc + i) < 0);
                        RGB_PATH(RP_MESH_Y_HI, mesh_lerp32(cy[0], ly, ry, gc + i) > 256 * (H - 1));
                        RGB_PATH(RP_MESH_X_LO, mesh_lerp32(cx[0], lx, rx, gc + i) < 0);
                        RGB_PATH(RP_MESH_X_HI, mesh_lerp32(cx[0], lx, rx, gc + i) > 256 * (W - 1));
                    }
                } else {
#pragma unroll
                    for (uint32_t i = 0; i < 4u; i++) {
                        Ys[i] = static_cast<int32_t>(mesh_clamp(mesh_lerp64(cy, gr, gc + i), H));
                        Xs[i] = static_cast<int32_t>(mesh_clamp(mesh_lerp64(cx, gr, gc + i), W));
                        RGB_PATH(RP_MESH_Y_LO, mesh_lerp64(cy, gr, gc + i) < 0);
                        RGB_PATH(RP_MESH_Y_HI, mesh_lerp64(cy, gr, gc + i) > 256 * (static_cast<int64_t>(H) - 1));
                        RGB_PATH(RP_MESH_X_LO, mesh_lerp64(cx, gr, gc + i) < 0);
                        RGB_PATH(RP_MESH_X_HI, mesh_lerp64(cx, gr, gc + i) > 256 * (static_cast<int64_t>(W) - 1));
                    }
                }
#pragma unroll
                for (uint32_t i = 0; i < 4u; i++) {
                    const int32_t Y = Ys[i], X = Xs[i];
                    int32_t wy[4], wx[4], e3[3];
                    warp_weights(s_w, static_cast<uint32_t>(Y) & 255u, wy);
                    warp_weights(s_w, static_cast<uint32_t>(X) & 255u, wx);
                    warp_taps(s_e, wy, wx, min(max((Y >> 8) - 1 - pb, 0), rmax), min(max((X >> 8) - 1 - eb, 0), cmax), e3);
                    WARP_PATH(RPG_TAP_ROW_LO, (Y >> 8) - 1 - pb < 0);
                    WARP_PATH(RPG_TAP_ROW_HI, (Y >> 8) - 1 - pb > rmax);
                    WARP_PATH(RPG_TAP_COL_LO, (X >> 8) - 1 - eb < 0);
                    WARP_PATH(RPG_TAP_COL_HI, (X >> 8) - 1 - eb > cmax);
                    E4[0][i] = e3[0], E4[1][i] = e3[1], E4[2][i] = e3[2];
                }
            }
            __syncthreads(); // every tap is read: the tile's E takes the place of the first estimates
#pragma unroll
            for (uint32_t c = 0; c < 3u; c++)
                *reinterpret_cast<mcraw_u32x4 *>(&s_e[(c * WARP_TH + gr) * WARP_TW + gc]) =
                    mcraw_u32x4{static_cast<uint32_t>(E4[c][0]), static_cast<uint32_t>(E4[c][1]), static_cast<uint32_t>(E4[c][2]),
                                static_cast<uint32_t>(E4[c][3])};
            __syncthreads();
        }
        warp_store<PK>(A, s_e, s_lut, f, i0, i1, k0); // (8 output columns, output row or row pair) out of the tile's E
    } while (LUT && (t += gridDim.x) < A.units * A.nf);
}

struct MeshK {
    template <int PK, int S>
    static auto at() { return &krgb_mesh<PK, S>; }
};

static int mesh_launch(mcraw_ctx *c, const mcraw_rgb *p, const mcraw_mesh *mp, const mcraw_display *d, const mcraw_yuv *yv,
                       const mcraw_rgb_color *colors, int ncolors, const int32_t *nodes, const uint16_t *in, size_t in_pitch,
                       size_t in_frame_stride, int width, int height, int n, const MeshPlan &P, void *out, hipStream_t st)
{
    RgbArgs A = rgb_args(p, d, yv, in_pitch, in_frame_stride, width, height, ncolors);
    A.Wo = static_cast<uint32_t>(P.rgb.Wo);
    A.Ho = static_cast<uint32_t>(P.rgb.Ho);
    A.tilesX = P.tilesX;
    A.units = P.units;
    A.invec = P.rgb.invec;
    MeshGeo G{};
    G.permesh = P.permesh ? 1u : 0u;
    G.tilesX = P.tilesX;
    G.Mx = P.Mx;
    G.stride = static_cast<uint32_t>(2u * P.nodes());
    G.filter = mp->filter;
    const std::vector<RgbCol> cols = rgb_cols(p, colors, ncolors, 0.0625f);
    // the meshes stay where they are: pieces of RGB_MAXF frames only where the colours are per frame (they travel in the kernel
    // arguments), else of what one launch takes; a piece's first mesh goes with it
    const int piece = A.percol ? RGB_MAXF : LAUNCH_FRAMES;
    for (int f0 = 0; f0 < n; f0 += piece) {
        const int nf = std::min(piece, n - f0);
        G.nodes = nodes + (P.permesh ? static_cast<size_t>(f0) * G.stride : 0u);
        const std::vector<RgbCol> pc = A.percol ? std::vector<RgbCol>(cols.begin() + f0, cols.begin() + f0 + nf) : cols;
        if (int rc = rgb_launch(c, rgb_pick<MeshK>(P.rgb), A, P.rgb, pc, in + static_cast<size_t>(f0) * in_frame_stride, nf,
                                static_cast<uint8_t *>(out) + static_cast<size_t>(f0) * P.rgb.out_frame, -1, st, G))
            return rc;
    }
    return 0;
}

} // namespace mcraw

using namespace mcraw;

extern "C" {

size_t mcraw_mesh_nodes(const mcraw_mesh *m)
{
    MeshPlan P;
    if (!m || P.geometry(m))
        return 0u;
    return P.nodes();
}

int mcraw_mesh_check(const mcraw_mesh *m, const int32_t *nodes_host, int nmesh, int width, int height, int flags)
{
    if (const char *why = mesh_nodes_check(m, nodes_host, nmesh, width, height, flags))
        return reject("mcraw_mesh_check", why);
    return 0;
}

int mcraw_demosaic_mesh_batch(mcraw_ctx *c, const mcraw_rgb *p, const mcraw_mesh *m, const mcraw_display *d, const mcraw_yuv *y,
                              const mcraw_rgb_color *colors, int ncolors, const int32_t *nodes, size_t nodes_bytes, int nmesh,
                              const uint16_t *in, size_t in_pitch, size_t in_frame_stride, int width, int height, int n, void *out,
                              size_t out_bytes, void *stream)
{
    MeshPlan P;
    const char *why = c ? mesh_check(p, m, d, y, colors, ncolors, nodes, nodes_bytes, nmesh, in, in_pitch, in_frame_stride, width, height, n,
                                     out, out_bytes, P)
                        : "bad arguments";
    if (why)
        return reject("mcraw_demosaic_mesh_batch", why);
    if (P.rgb.noop)
        return 0;
    std::lock_guard<std::mutex> lk(c->mu);
    HIP_TRY(hipSetDevice(c->device));
    return mesh_launch(c, p, m, d, y, colors, ncolors, nodes, in, in_pitch, in_frame_stride, width, height, n, P, out, stream_of(c, stream));
}

} // extern "C"
