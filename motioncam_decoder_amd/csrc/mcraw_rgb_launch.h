// mcraw_rgb_launch.h -- the host side that every demosaic entry point shares (csrc/mcraw_rgb.hip: mhc and bin2;
// csrc/mcraw_area.hip; csrc/mcraw_resample.hip): the per-frame colours, the common part of the kernel arguments, the choice of a
// kernel's instance, the size of a persistent grid and the loop over the pieces of a batch.  An entry point keeps what is its
// own: the scale of its integer estimates, its geometry struct, the launch of its tap table and one call of rgb_launch.
#pragma once
#include <optional>

#include "mcraw_host.h"
#include "mcraw_rgb_args.h"
#include "mcraw_rgb_dev.h"

// The hook of the test builds that force a persistent grid's size (tests/test_gpu_rgb_paths.py): what the device holds at once,
// unless a source defines another limit in front of this header.  Any grid from 1 to units x frames workgroups walks every unit
// exactly once (the kernels' loop condition), so every limit >= 1 is valid for every input.
#ifndef RGB_GRID_LIMIT
#define RGB_GRID_LIMIT(resident) (resident)
#endif

namespace mcraw {

// k[c] = (gain[c] * inv) * scale per colour, `scale` undoing the weight of the kernel's integer estimates.
// (the division is in f32, as every step of the host side of the contract)
inline std::vector<RgbCol> rgb_cols(const mcraw_rgb *p, const mcraw_rgb_color *colors, int ncolors, float scale)
{
    const float bsum = static_cast<float>(static_cast<int>(p->black[0]) + p->black[1] + p->black[2] + p->black[3]);
    const float inv = 1.0f / (p->white - 0.25f * bsum);
    std::vector<RgbCol> cols(static_cast<size_t>(ncolors));
    for (int i = 0; i < ncolors; i++) {
        for (int k = 0; k < 3; k++)
            cols[static_cast<size_t>(i)].k[k] = (colors[i].gain[k] * inv) * scale;
        std::memcpy(cols[static_cast<size_t>(i)].m, colors[i].m, sizeof(float) * 9);
    }
    return cols;
}

// What every kernel's RgbArgs takes from the call itself; Wo, Ho, tilesX, units and invec are the caller's plan's, and in, out,
// nf and col are set per piece (rgb_launch).
inline RgbArgs rgb_args(const mcraw_rgb *p, const mcraw_display *d, const mcraw_yuv *yv, size_t in_pitch, size_t in_frame_stride,
                        int width, int height, int ncolors)
{
    RgbArgs A{};
    A.pitch = in_pitch;
    A.fstride = in_frame_stride;
    A.W = static_cast<uint32_t>(width);
    A.H = static_cast<uint32_t>(height);
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
    return A;
}

// The instance of a kernel template for the plan's output kind and CFA shift.  K names the template: K::at<PK, S>() is the
// address of its instance.
template <class K, int PK>
auto rgb_pick_shift(int s)
{
    static const decltype(K::template at<PK, 0>()) k[4] = {K::template at<PK, 0>(), K::template at<PK, 1>(), K::template at<PK, 2>(),
                                                          K::template at<PK, 3>()};
    return k[s];
}

template <class K>
auto rgb_pick(const RgbPlan &P)
{
    switch (P.kind) {
    case PK_F32: return rgb_pick_shift<K, PK_F32>(P.shift);
    case PK_F16: return rgb_pick_shift<K, PK_F16>(P.shift);
    case PK_BF16: return rgb_pick_shift<K, PK_BF16>(P.shift);
    case PK_DISP8: return rgb_pick_shift<K, PK_DISP8>(P.shift);
    case PK_DISP16: return rgb_pick_shift<K, PK_DISP16>(P.shift);
    case PK_NV12: return rgb_pick_shift<K, PK_NV12>(P.shift);
    default: return rgb_pick_shift<K, PK_P010>(P.shift);
    }
}

// Workgroups of a persistent grid: what the device holds at once (compute units x resident workgroups of the instance), found
// once per (device, kernel).
inline uint32_t resident_groups(int device, const void *kernel)
{
    static std::mutex mu;
    static std::vector<std::pair<std::pair<int, const void *>, uint32_t>> seen;
    std::lock_guard<std::mutex> lk(mu);
    for (const auto &e : seen)
        if (e.first.first == device && e.first.second == kernel)
            return e.second;
    int cus = 0, per = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0)
        cus = 256;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per, kernel, RGB_T, 0) != hipSuccess || per <= 0)
        per = 2;
    const uint32_t g = static_cast<uint32_t>(cus) * static_cast<uint32_t>(per);
    seen.push_back({{device, kernel}, g});
    return g;
}

// The launches of a batch of n frames, in pieces of RGB_MAXF frames where the colours are per frame (they travel in A).  The
// kinds with a LUT run a persistent grid of at most what the device holds at once, over A.units x nf units of work; the float
// kinds one workgroup per unit and frame.  kid: the kernel id whose KTimer brackets every launch, or -1: none is made.
// G: the kernel's second argument, if it has one.
template <class Kernel, class... Geo>
int rgb_launch(mcraw_ctx *c, Kernel k, RgbArgs A, const RgbPlan &P, const std::vector<RgbCol> &cols, const uint16_t *in, int n, void *out,
               int kid, hipStream_t st, const Geo &...G)
{
    const bool persistent = has_lut(P.kind);
    const uint32_t resident = persistent ? resident_groups(c->device, reinterpret_cast<const void *>(k)) : 0u;
    const int piece = A.percol ? RGB_MAXF : 65535;
    for (int f0 = 0; f0 < n; f0 += piece) {
        const int nf = std::min(piece, n - f0);
        A.in = in + static_cast<size_t>(f0) * A.fstride;
        A.out = static_cast<uint8_t *>(out) + static_cast<size_t>(f0) * P.out_frame;
        A.nf = static_cast<uint32_t>(nf);
        for (int i = 0; i < (A.percol ? nf : 1); i++)
            A.col[i] = cols[static_cast<size_t>(A.percol ? f0 + i : 0)];
        const dim3 grid = persistent ? dim3(static_cast<uint32_t>(std::min<uint64_t>(static_cast<uint64_t>(A.units) * nf, RGB_GRID_LIMIT(resident))))
                                     : dim3(A.units, static_cast<uint32_t>(nf));
        std::optional<KTimer> kt;
        if (kid >= 0)
            kt.emplace(c, kid, st);
        hipLaunchKernelGGL(k, grid, dim3(RGB_T), 0, st, A, G...);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

} // namespace mcraw
