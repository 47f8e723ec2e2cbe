// rgb_paths_plan.cpp -- the plans that the real headers (csrc/mcraw_rgb_args.h, mcraw_area_args.h, mcraw_resample_args.h: no HIP) make
// of the calls of tests/_rgb_paths_model.py's corpus, for tests/test_rgb_paths_model.py to compare with the model's own.  One call
// per line of standard input:
//   kernel(0 mhc, 1 bin2, 2 area, 3 resample) family(0 float, 1 display, 2 yuv) es n W H pitch fstride off_elems out_off y0 x0 ch cw Ho Wo filter
// and per call one line "key=value ..." of the plan, or "rejected: why".
#include <cstdio>
#include <cstring>

#include "mcraw_area_args.h"
#include "mcraw_resample_args.h"

using namespace mcraw;

int main()
{
    unsigned kernel, fam, es, n, W, H, off, out_off, y0, x0, ch, cw, Ho, Wo, filter;
    unsigned long pitch, fstride;
    while (std::scanf("%u %u %u %u %u %u %lu %lu %u %u %u %u %u %u %u %u %u", &kernel, &fam, &es, &n, &W, &H, &pitch, &fstride, &off, &out_off,
                      &y0, &x0, &ch, &cw, &Ho, &Wo, &filter) == 17) {
        mcraw_rgb p;
        mcraw_display d;
        mcraw_yuv y;
        std::memset(&p, 0, sizeof p);
        std::memset(&d, 0, sizeof d);
        std::memset(&y, 0, sizeof y);
        p.algo = kernel == 0 ? MCRAW_RGB_MHC : kernel == 1 ? MCRAW_RGB_BIN2 : kernel == 2 ? MCRAW_RGB_AREA : MCRAW_RGB_RESAMPLE;
        p.dtype = fam ? 0u : es == 4 ? MCRAW_FLOAT_F32 : MCRAW_FLOAT_F16;
        p.cfa = MCRAW_CFA_RGGB, p.white = 4095.0f;
        d.dtype = es == 1 ? MCRAW_DISP_U8 : MCRAW_DISP_U16, d.layout = MCRAW_DISP_HWC, d.lut_log2 = 12;
        d.lut = reinterpret_cast<const uint16_t *>(0x20000);
        y.format = es == 1 ? MCRAW_YUV_NV12 : MCRAW_YUV_P010, y.lut_log2 = 12, y.in_bits = 12, y.sh = 8, y.y_off = 16, y.c_off = 128;
        y.cy[0] = 47, y.cy[1] = 157, y.cy[2] = 16, y.cb[0] = -26, y.cb[1] = -86, y.cb[2] = 112, y.cr[0] = 112, y.cr[1] = -102, y.cr[2] = -10;
        y.lut = d.lut;
        static mcraw_rgb_color col[64];
        for (auto &k : col) {
            std::memset(&k, 0, sizeof k);
            k.gain[0] = k.gain[1] = k.gain[2] = 1.0f, k.m[0] = k.m[4] = k.m[8] = 1.0f;
        }
        const uint16_t *in = reinterpret_cast<const uint16_t *>(uintptr_t{0x100000} + 2u * off);
        const void *out = reinterpret_cast<const void *>(uintptr_t{0x40000000} + out_off), *work = reinterpret_cast<const void *>(uintptr_t{0x8000000});
        const size_t big = size_t{1} << 30;
        const mcraw_display *dp = fam == 1 ? &d : nullptr;
        const mcraw_yuv *yp = fam == 2 ? &y : nullptr;
        if (kernel < 2) {
            RgbPlan P;
            if (const char *why = rgb_check(&p, dp, yp, col, static_cast<int>(n), in, pitch, fstride, static_cast<int>(W), static_cast<int>(H),
                                            static_cast<int>(n), out, big, P)) {
                std::printf("rejected: %s\n", why);
                continue;
            }
            std::printf("Wo=%zu Ho=%zu tilesX=%u units=%u invec=%d out_frame=%zu\n", P.Wo, P.Ho, P.tilesX, P.units, P.invec ? 1 : 0, P.out_frame);
        } else if (kernel == 2) {
            mcraw_area a;
            std::memset(&a, 0, sizeof a);
            a.x0 = x0, a.y0 = y0, a.cw = cw, a.ch = ch, a.out_w = Wo, a.out_h = Ho;
            AreaPlan P;
            if (const char *why = area_check(&p, &a, dp, yp, col, static_cast<int>(n), in, pitch, fstride, static_cast<int>(W),
                                             static_cast<int>(H), static_cast<int>(n), work, big, out, big, P)) {
                std::printf("rejected: %s\n", why);
                continue;
            }
            std::printf("Wo=%zu Ho=%zu Qw=%u Qh=%u ntx=%u nty=%u mode=%u lx_log2=%u ly=%u seg=%u segp=%u nch=%u tilesX=%u groups=%u bands=%u "
                        "units=%u out_frame=%zu\n", P.rgb.Wo, P.rgb.Ho, P.Qw, P.Qh, P.ntx, P.nty, P.mode, P.lx_log2, P.ly, P.seg, P.segp, P.nch,
                        P.tilesX, P.groups, P.bands, P.units, P.rgb.out_frame);
        } else {
            mcraw_resample r;
            std::memset(&r, 0, sizeof r);
            r.x0 = x0, r.y0 = y0, r.cw = cw, r.ch = ch, r.out_w = Wo, r.out_h = Ho, r.filter = filter;
            ResamplePlan P;
            if (const char *why = resample_check(&p, &r, dp, yp, col, static_cast<int>(n), in, pitch, fstride, static_cast<int>(W),
                                                 static_cast<int>(H), static_cast<int>(n), work, big, out, big, P)) {
                std::printf("rejected: %s\n", why);
                continue;
            }
            std::printf("Wo=%zu Ho=%zu ntx=%u nty=%u ly=%u ecols=%u erows=%u tilesX=%u bands=%u units=%u invec=%d out_frame=%zu\n", P.rgb.Wo,
                        P.rgb.Ho, P.ntx, P.nty, P.ly, P.ecols, P.erows, P.tilesX, P.bands, P.units, P.rgb.invec ? 1 : 0, P.rgb.out_frame);
        }
    }
    return 0;
}
