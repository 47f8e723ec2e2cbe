// warp_args_check.cpp -- csrc/mcraw_warp_args.h on its own (no HIP: that this file compiles with a plain g++ is part of the test):
// the two phase tables against a transcription of the contract (include/mcraw_hip.h) -- 4096 in all, the mirror, the named
// phases, sum |w| and the smallest weight --; what mcraw_demosaic_warp_batch decides about a call, one defect at a time, and
// maps at and just beyond every bound against a transcription of the rules, with the frame named; and the plan's invariants over
// a sweep of maps at the bounds and seeded ones: the tiles cover the output, and every tap of every pixel of every tile, with
// MHC's halo, lies in the tile's planned window and the window in the workgroup's LDS arrays.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "mcraw_warp_args.h"

using namespace mcraw;

static long cases = 0, wrong = 0, accepted = 0, rejected = 0;

#define CHECK(cond)                                                                                                    \
    do {                                                                                                               \
        cases++;                                                                                                       \
        if (!(cond)) {                                                                                                 \
            wrong++;                                                                                                   \
            if (wrong < 20)                                                                                            \
                std::printf("line %d: %s\n", __LINE__, #cond);                                                         \
        }                                                                                                              \
    } while (0)

static constexpr WarpTable LIN = warp_table(MCRAW_FILTER_LINEAR), CUB = warp_table(MCRAW_FILTER_CUBIC); // compile-time constants
static_assert(CUB.w[0][1] == 4096 && CUB.w[128][0] == -256 && CUB.w[128][1] == 2304 && LIN.w[64][1] == 3072, "the tables are constant expressions");

static long long fdiv(long long a, long long b) { return a >= 0 ? a / b : -((-a + b - 1) / b); }

static void tables()
{
    long sabs = 0, wmin = 0;
    for (int p = 0; p < 256; p++) {
        // the contract, transcribed
        long long f[4], d[4], F = 0, w[4], sum = 0;
        for (int j = 0; j < 4; j++) {
            d[j] = std::llabs(256LL * (j - 1) - p);
            const long long a = 4 * d[j];
            f[j] = a <= 1024 ? 3 * a * a * a - 5 * 1024 * a * a + 2 * (1LL << 30)
                             : a < 2048 ? -a * a * a + 5 * 1024 * a * a - 8 * 1024 * 1024 * a + 4 * (1LL << 30) : 0;
            F += f[j];
        }
        CHECK(F == 2 * (1LL << 30));
        for (int j = 0; j < 4; j++)
            sum += w[j] = fdiv(4096 * f[j] + F / 2, F);
        const long long res = 4096 - sum;
        if (d[1] < d[2])
            w[1] += res;
        else if (d[2] < d[1])
            w[2] += res;
        else {
            CHECK(res % 2 == 0);
            w[1] += res - res / 2, w[2] += res / 2;
        }
        long s = 0, a = 0;
        for (int j = 0; j < 4; j++) {
            CHECK(CUB.w[p][j] == w[j]);
            CHECK(LIN.w[p][j] == (j == 1 ? 16 * (256 - p) : j == 2 ? 16 * p : 0));
            s += CUB.w[p][j], a += std::labs(CUB.w[p][j]);
            wmin = CUB.w[p][j] < wmin ? CUB.w[p][j] : wmin;
            if (p)
                CHECK(CUB.w[p][j] == CUB.w[256 - p][3 - j] && LIN.w[p][j] == LIN.w[256 - p][3 - j]); // w(p) mirrors w(256 - p)
        }
        CHECK(s == 4096);
        sabs = a > sabs ? a : sabs;
    }
    CHECK(CUB.w[0][0] == 0 && CUB.w[0][1] == 4096 && CUB.w[0][2] == 0 && CUB.w[0][3] == 0);
    CHECK(CUB.w[128][0] == -256 && CUB.w[128][1] == 2304 && CUB.w[128][2] == 2304 && CUB.w[128][3] == -256);
    CHECK(sabs <= 5120 && wmin == -303);
    std::printf("tables: max sum |w| %ld  min w %ld\n", sabs, wmin);
}

struct Call {
    mcraw_rgb p;
    mcraw_warp w;
    mcraw_display d;
    mcraw_yuv y;
    bool has_p = true, has_w = true, has_d = false, has_y = false, has_maps = true;
    mcraw_rgb_color col[3];
    int ncolors = 1;
    int32_t maps[3][6];
    int nmaps = 1;
    uintptr_t in = 0x10000, out = 0x4000000;
    size_t pitch = 64, fstride = 64 * 32, out_bytes = 1 << 22;
    int width = 64, height = 32, n = 2;
};

static Call good()
{
    Call c;
    std::memset(&c.p, 0, sizeof c.p);
    std::memset(&c.w, 0, sizeof c.w);
    std::memset(&c.d, 0, sizeof c.d);
    std::memset(&c.y, 0, sizeof c.y);
    c.p.algo = MCRAW_RGB_WARP, c.p.dtype = MCRAW_FLOAT_F32, c.p.cfa = MCRAW_CFA_GRBG, c.p.white = 4095.0f;
    c.w.out_w = 40, c.w.out_h = 20, c.w.filter = MCRAW_FILTER_CUBIC;
    c.d.dtype = MCRAW_DISP_U8, c.d.layout = MCRAW_DISP_HWC, c.d.lut_log2 = 12, c.d.lut = reinterpret_cast<const uint16_t *>(0x20000);
    c.y.format = MCRAW_YUV_NV12, c.y.lut_log2 = 12, c.y.in_bits = 8, c.y.sh = 8, c.y.y_off = 16, c.y.c_off = 128;
    c.y.cy[0] = 47, c.y.cy[1] = 157, c.y.cy[2] = 16, c.y.cb[0] = -26, c.y.cb[1] = -86, c.y.cb[2] = 112;
    c.y.cr[0] = 112, c.y.cr[1] = -102, c.y.cr[2] = -10, c.y.lut = reinterpret_cast<const uint16_t *>(0x20000);
    for (auto &k : c.col) {
        std::memset(&k, 0, sizeof k);
        k.gain[0] = k.gain[1] = k.gain[2] = 1.0f, k.m[0] = k.m[4] = k.m[8] = 1.0f;
    }
    for (auto &m : c.maps) {
        const int32_t id[6] = {65536, 0, 256 * 3, 0, 65536, 256 * 5};
        std::memcpy(m, id, sizeof id);
    }
    return c;
}

static const char *run(const Call &c, WarpPlan &P)
{
    const char *why = warp_check(c.has_p ? &c.p : nullptr, c.has_w ? &c.w : nullptr, c.has_d ? &c.d : nullptr, c.has_y ? &c.y : nullptr,
                                 c.col, c.ncolors, c.has_maps ? &c.maps[0][0] : nullptr, c.nmaps, reinterpret_cast<const uint16_t *>(c.in),
                                 c.pitch, c.fstride, c.width, c.height, c.n, reinterpret_cast<const void *>(c.out), c.out_bytes, P);
    (why ? rejected : accepted)++;
    return why;
}

template <class F>
static void defect(F f, const char *part = nullptr)
{
    Call c = good();
    f(c);
    WarpPlan P;
    const char *why = run(c, P);
    CHECK(why != nullptr);
    if (why && part)
        CHECK(std::strstr(why, part) != nullptr);
}

// the rules for one map, transcribed from the header
static bool map_rule(const int32_t *m, int W, int H, long Wo, long Ho)
{
    const long long dev[4] = {m[0] - 65536LL, m[4] - 65536LL, m[1], m[3]};
    for (long long v : dev)
        if (v > 16384 || v < -16384)
            return false;
    for (int c = 0; c < 4; c++) {
        const long long i = (c & 2) ? Ho - 1 : 0, k = (c & 1) ? Wo - 1 : 0;
        const long long Y = m[2] + fdiv(1LL * m[0] * i + 1LL * m[1] * k + 128, 256), X = m[5] + fdiv(1LL * m[3] * i + 1LL * m[4] * k + 128, 256);
        if (Y < 0 || Y > 256LL * (H - 1) || X < 0 || X > 256LL * (W - 1))
            return false;
    }
    return true;
}

static void decisions()
{
    WarpPlan P;
    Call g = good();
    CHECK(run(g, P) == nullptr && !P.rgb.noop && P.rgb.Wo == 40 && P.rgb.Ho == 20 && P.tilesX == 2 && P.tilesY == 1 && P.units == 2 && !P.permap);
    g.nmaps = 2;
    CHECK(run(g, P) == nullptr && P.permap);
    g = good(), g.n = 0, g.in = 0, g.out = 0, g.maps[0][2] = -1;
    CHECK(run(g, P) == nullptr && P.rgb.noop);
    g = good(), g.has_d = true, g.p.dtype = 0;
    CHECK(run(g, P) == nullptr && P.rgb.kind == PK_DISP8);
    g = good(), g.has_y = true, g.p.dtype = 0;
    CHECK(run(g, P) == nullptr && P.rgb.kind == PK_NV12);
    defect([](Call &c) { c.has_p = false; });
    defect([](Call &c) { c.has_w = false; });
    defect([](Call &c) { c.has_maps = false; });
    defect([](Call &c) { c.n = -1; });
    defect([](Call &c) { c.has_d = c.has_y = true, c.p.dtype = 0; }, "at once");
    defect([](Call &c) { c.width = 6; }, "8 .. 65536");
    defect([](Call &c) { c.height = 6; }, "8 .. 65536");
    defect([](Call &c) { c.width = 63; });
    defect([](Call &c) { c.in = 0; });
    defect([](Call &c) { c.in |= 1; });
    defect([](Call &c) { c.pitch = 62; });
    for (uint32_t a : {0u, 1u, 2u, 3u, 4u, 6u})
        defect([a](Call &c) { c.p.algo = a; }, "MCRAW_RGB_WARP");
    defect([](Call &c) { c.p.dtype = 9; });
    defect([](Call &c) { c.p.cfa = 4; });
    defect([](Call &c) { c.p.white = 0.0f; });
    defect([](Call &c) { c.ncolors = 3; });
    defect([](Call &c) { c.w.reserved = 1; }, "reserved");
    defect([](Call &c) { c.w.filter = 2; }, "filter");
    defect([](Call &c) { c.w.out_w = 0; }, "1 .. 65536");
    defect([](Call &c) { c.w.out_h = 65537; }, "1 .. 65536");
    defect([](Call &c) { c.has_y = true, c.p.dtype = 0, c.w.out_w = 39; }, "4:2:0");
    defect([](Call &c) { c.has_y = true, c.p.dtype = 0, c.w.out_h = 19; }, "4:2:0");
    defect([](Call &c) { c.nmaps = 0; }, "nmaps");
    defect([](Call &c) { c.nmaps = 3; }, "nmaps");
    defect([](Call &c) { c.out = 0; });
    defect([](Call &c) { c.out |= 2; });
    defect([](Call &c) { c.out_bytes = 2 * 3 * 20 * 40 * 4 - 1; });
    // maps at and just beyond every bound; the message names the frame of the first bad one
    const int at[] = {0, 1, 3, 4};
    for (int e : at)
        for (int sign : {-1, 1})
            for (int over : {0, 1}) {
                Call c = good();
                c.nmaps = 2, c.w.out_w = 8, c.w.out_h = 8; // small enough for every extreme linear part about the middle
                for (auto &m : c.maps)
                    m[2] = 256 * 12, m[5] = 256 * 28;
                c.maps[1][e] += sign * (16384 + over);
                const char *why = run(c, P);
                CHECK((why != nullptr) == (over == 1));
                CHECK(map_rule(c.maps[1], c.width, c.height, 8, 8) == (over == 0));
                if (why)
                    CHECK(std::strstr(why, "frame 1") && std::strstr(why, "linear part"));
            }
    std::mt19937 rng(7);
    for (int it = 0; it < 200000; it++) {
        Call c = good();
        c.nmaps = 2;
        c.w.out_w = 1 + rng() % 64, c.w.out_h = 1 + rng() % 32;
        for (auto &o : c.maps)
            o[2] = o[5] = 0; // the identity from the origin fits every size up to the frame's
        int32_t *m = c.maps[rng() & 1];
        const int bad = static_cast<int>(m - c.maps[0]) / 6;
        const auto pick = [&](int32_t centre) {
            switch (rng() % 4) {
            case 0: return centre;
            case 1: return centre + (rng() & 1 ? 16384 : -16384) + static_cast<int32_t>(rng() % 3) - 1;
            default: return centre + static_cast<int32_t>(rng() % 32771) - 16385;
            }
        };
        m[0] = pick(65536), m[1] = pick(0), m[3] = pick(0), m[4] = pick(65536);
        // the translation that puts the smallest corner about 0, or the largest about the frame's last sample, +- 1
        long long lo[2] = {0, 0}, hi[2] = {0, 0};
        for (int cnr = 0; cnr < 4; cnr++) {
            const long long i = (cnr & 2) ? c.w.out_h - 1 : 0, k = (cnr & 1) ? c.w.out_w - 1 : 0;
            const long long v[2] = {fdiv(1LL * m[0] * i + 1LL * m[1] * k + 128, 256), fdiv(1LL * m[3] * i + 1LL * m[4] * k + 128, 256)};
            for (int a = 0; a < 2; a++)
                lo[a] = v[a] < lo[a] ? v[a] : lo[a], hi[a] = v[a] > hi[a] ? v[a] : hi[a];
        }
        const long long side[2] = {256LL * (c.height - 1), 256LL * (c.width - 1)};
        for (int a = 0; a < 2; a++) {
            const long long nudge = static_cast<long long>(rng() % 3) - 1;
            m[a ? 5 : 2] = static_cast<int32_t>(rng() & 1 ? -lo[a] + nudge : side[a] - hi[a] + nudge);
        }
        const bool ok = map_rule(m, c.width, c.height, c.w.out_w, c.w.out_h);
        const char *why = run(c, P);
        CHECK((why == nullptr) == ok);
        if (why) {
            char name[32];
            std::snprintf(name, sizeof name, "frame %d", bad);
            CHECK(std::strstr(why, name) != nullptr);
        }
    }
}

// Every tap of every pixel of every tile inside the tile's window, the window inside the LDS arrays.
static void tile_sweep(const int32_t *m, uint32_t Wo, uint32_t Ho, int W, int H)
{
    const uint32_t tilesX = (Wo + WARP_TW - 1) / WARP_TW, tilesY = (Ho + WARP_TH - 1) / WARP_TH;
    CHECK(tilesX * WARP_TW >= Wo && tilesY * WARP_TH >= Ho);
    for (uint32_t ty = 0; ty < tilesY; ty++)
        for (uint32_t tx = 0; tx < tilesX; tx++) {
            const uint32_t k0 = tx * WARP_TW, k1 = std::min(k0 + WARP_TW, Wo) - 1, i0 = ty * WARP_TH, i1 = std::min(i0 + WARP_TH, Ho) - 1;
            const WarpWin w = warp_window(m, i0, i1, k0, k1);
            bool in = w.np >= 1 && w.ne >= 1 && w.np <= WARP_EROWS / 2 && w.ne <= WARP_ECOLS / 8 && !(w.pb & 1) && !(w.eb & 7);
            // the raw window: rows pb - 2 .. pb + 2 np + 1 (RAWH), columns eb - 8 .. eb + 8 ne + 7 (RAWW); phase A reads up to column
            // 8 (ne - 1) + 17 and row 2 (np - 1) + 1 + 4 of it
            in = in && 2 * w.np + 4 <= WARP_RAWH && 8 * (w.ne + 2) <= WARP_RAWW && 8 * (w.ne - 1) + 17 < 8 * (w.ne + 2);
            for (uint32_t i = i0; i <= i1 && in; i++)
                for (uint32_t k = k0; k <= k1; k++) {
                    int64_t Y, X;
                    warp_pos(m, i, k, Y, X);
                    const int64_t r0 = (Y >> 8) - 1 - w.pb, c0 = (X >> 8) - 1 - w.eb;
                    in = in && r0 >= 0 && r0 + 3 < 2 * static_cast<int64_t>(w.np) && c0 >= 0 && c0 + 3 < 8 * static_cast<int64_t>(w.ne);
                    in = in && r0 <= WARP_EROWS - 4 && c0 <= WARP_ECOLS - 4; // (the kernel's clamps change nothing)
                    in = in && Y >= 0 && Y <= 256LL * (H - 1) && X >= 0 && X <= 256LL * (W - 1); // the corners bound every pixel
                    // one reflection suffices for the taps with MHC's halo (the window's unused rim on the 8-grid may lie further out)
                    in = in && (Y >> 8) - 3 >= -(H - 1) && (Y >> 8) + 4 <= 2 * (H - 1) && (X >> 8) - 3 >= -(W - 1) && (X >> 8) + 4 <= 2 * (W - 1);
                }
            if (!in)
                std::printf("tile (%u, %u) of %u x %u onto %d x %d under {%d, %d, %d, %d, %d, %d}: window pb %d eb %d np %u ne %u\n", ty, tx, Ho, Wo, H,
                            W, m[0], m[1], m[2], m[3], m[4], m[5], w.pb, w.eb, w.np, w.ne);
            CHECK(in);
        }
}

static void plans()
{
    const int W = 328, H = 120;
    const int32_t ext[2] = {-16384, 16384};
    // every combination of the four extremes (and the identity on each), the window pushed into each corner of the frame
    for (int a = 0; a < 3; a++)
        for (int b = 0; b < 3; b++)
            for (int c = 0; c < 3; c++)
                for (int d = 0; d < 3; d++)
                    for (int cnr = 0; cnr < 4; cnr++)
                        for (uint32_t Wo : {70u, 33u}) {
                            const uint32_t Ho = Wo == 70u ? 40u : 65u;
                            int32_t m[6] = {65536 + (a < 2 ? ext[a] : 0), b < 2 ? ext[b] : 0, 0, c < 2 ? ext[c] : 0, 65536 + (d < 2 ? ext[d] : 0), 0};
                            long long lo[2] = {0, 0}, hi[2] = {0, 0};
                            for (int q = 0; q < 4; q++) {
                                int64_t Y, X;
                                warp_pos(m, (q & 2) ? Ho - 1 : 0, (q & 1) ? Wo - 1 : 0, Y, X);
                                lo[0] = Y < lo[0] ? Y : lo[0], hi[0] = Y > hi[0] ? Y : hi[0], lo[1] = X < lo[1] ? X : lo[1], hi[1] = X > hi[1] ? X : hi[1];
                            }
                            if (hi[0] - lo[0] > 256LL * (H - 1) || hi[1] - lo[1] > 256LL * (W - 1))
                                continue;
                            m[2] = static_cast<int32_t>((cnr & 2) ? 256LL * (H - 1) - hi[0] : -lo[0]);
                            m[5] = static_cast<int32_t>((cnr & 1) ? 256LL * (W - 1) - hi[1] : -lo[1]);
                            CHECK(warp_map_check(m, W, H, Wo, Ho) == nullptr);
                            tile_sweep(m, Wo, Ho, W, H);
                        }
    std::mt19937 rng(11);
    long swept = 0;
    for (int it = 0; it < 3000; it++) {
        const int w = 8 + 2 * static_cast<int>(rng() % 120), h = 8 + 2 * static_cast<int>(rng() % 60);
        const uint32_t Wo = 1 + rng() % 100, Ho = 1 + rng() % 70;
        int32_t m[6] = {65536 + static_cast<int32_t>(rng() % 32769) - 16384, static_cast<int32_t>(rng() % 32769) - 16384, 0,
                        static_cast<int32_t>(rng() % 32769) - 16384, 65536 + static_cast<int32_t>(rng() % 32769) - 16384, 0};
        m[2] = static_cast<int32_t>(rng() % (256 * h)) - 64, m[5] = static_cast<int32_t>(rng() % (256 * w)) - 64;
        if (warp_map_check(m, w, h, Wo, Ho))
            continue;
        swept++;
        tile_sweep(m, Wo, Ho, w, h);
    }
    CHECK(swept >= 100);
    std::printf("plans: %ld seeded maps swept\n", swept);
}

int main()
{
    static_assert(sizeof(mcraw_warp) == 16, "the header's layout");
    tables();
    decisions();
    plans();
    std::printf("accepted %ld rejected %ld\n", accepted, rejected);
    std::printf("cases %ld\n", cases);
    std::printf("wrong %ld\n", wrong);
    return wrong ? 1 : 0;
}
