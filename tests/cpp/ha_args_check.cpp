// ha_args_check.cpp -- csrc/mcraw_ha_args.h and rgb_check's part of MCRAW_RGB_HA on their own (no HIP: that this file compiles with
// a plain g++ is part of the test):
//   what the three classic entry points decide about a call with algo 6: over a sweep of frame sizes and the three families the
//   plan is MHC's but for the two flags, and every defect that MHC's call is rejected for rejects this one with the same words;
//   the tile of krgb_ha: for every tile of a sweep of frame sizes and the four CFA shifts, the items of the three phases as the
//   kernel decodes them -- every index inside the two LDS arrays, every raw piece staged exactly once, every entry of the green
//   plane written at most once and for the site (frame row, frame column) that the estimates' lanes later take it for, that site
//   an R / B site, and no entry read that the phase before did not write.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mcraw_ha_args.h"

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

struct Call {
    mcraw_rgb p{};
    mcraw_display d{};
    mcraw_yuv y{};
    mcraw_rgb_color col[3]{};
    int family = 0; // 0 float, 1 display, 2 YUV
    int ncolors = 1, width = 40, height = 24, n = 2;
    uintptr_t in = 0x100000, out = 0x200000;
    size_t pitch = 40, fstride = 40 * 24, out_bytes = size_t{1} << 30;
    bool null_p = false;

    explicit Call(int fam, uint32_t algo) : family(fam)
    {
        p.algo = algo;
        p.dtype = fam == 0 ? MCRAW_FLOAT_F32 : 0u;
        p.white = 4095.0f;
        for (auto &c : col) {
            c.gain[0] = c.gain[1] = c.gain[2] = 1.0f;
            c.m[0] = c.m[4] = c.m[8] = 1.0f;
        }
        d.dtype = MCRAW_DISP_U8, d.layout = MCRAW_DISP_HWC, d.lut_log2 = 12, d.lut = reinterpret_cast<const uint16_t *>(0x300000);
        y.format = MCRAW_YUV_NV12, y.lut_log2 = 12, y.in_bits = 11, y.sh = 14, y.y_off = 16, y.c_off = 128;
        y.cy[0] = 100, y.cy[1] = 300, y.cy[2] = 50, y.cb[0] = -50, y.cb[1] = -100, y.cb[2] = 150, y.cr[0] = 150, y.cr[1] = -120, y.cr[2] = -30;
        y.lut = reinterpret_cast<const uint16_t *>(0x300000);
    }
    const char *check(RgbPlan &P) const
    {
        return rgb_check(null_p ? nullptr : &p, family == 1 ? &d : nullptr, family == 2 ? &y : nullptr, col, ncolors,
                         reinterpret_cast<const uint16_t *>(in), pitch, fstride, width, height, n, reinterpret_cast<void *>(out), out_bytes, P);
    }
};

static void plans()
{
    const int sizes[] = {4, 6, 8, 30, 32, 34, 254, 256, 258, 510, 512, 514, 1000, 4032, 65536};
    for (int fam = 0; fam < 3; fam++)
        for (int w : sizes)
            for (int h : sizes) {
                if (static_cast<long long>(w) * h > (1LL << 26))
                    continue;
                Call a(fam, MCRAW_RGB_HA), b(fam, MCRAW_RGB_MHC);
                a.width = b.width = w, a.height = b.height = h;
                a.pitch = b.pitch = static_cast<size_t>(w), a.fstride = b.fstride = static_cast<size_t>(w) * h;
                a.out_bytes = b.out_bytes = ~size_t{0} >> 1;
                RgbPlan A, B;
                const char *wa = a.check(A), *wb = b.check(B);
                CHECK(!wa && !wb);
                if (wa || wb)
                    continue;
                accepted++;
                CHECK(A.ha && !A.mhc && B.mhc && !B.ha && !A.noop);
                CHECK(A.kind == B.kind && A.shift == B.shift && A.invec == B.invec && A.es == B.es && A.Wo == B.Wo && A.Ho == B.Ho);
                CHECK(A.frame_samples == B.frame_samples && A.out_frame == B.out_frame && A.tilesX == B.tilesX && A.units == B.units);
                CHECK(A.Wo == static_cast<size_t>(w) && A.Ho == static_cast<size_t>(h));
                CHECK(static_cast<uint64_t>(A.tilesX) * MHC_TW >= static_cast<uint64_t>(w) && (A.tilesX - 1u) * MHC_TW < static_cast<uint32_t>(w));
                CHECK(static_cast<uint64_t>(A.units / A.tilesX) * MHC_TH >= static_cast<uint64_t>(h) && A.units % A.tilesX == 0u);
            }
    // an empty batch is a no-op, whatever the algo says
    Call e(0, MCRAW_RGB_HA);
    e.n = 0;
    RgbPlan P;
    CHECK(!e.check(P) && P.noop);
    // the codes on either side stay unknown here
    for (uint32_t algo : {0u, 3u, 4u, 5u, 7u}) {
        Call u(0, algo);
        const char *why = u.check(P);
        CHECK(why && !std::strcmp(why, "unknown algo"));
    }
}

// Every defect that rejects MHC's call rejects this one, with the same words.
static void rejections()
{
    for (int fam = 0; fam < 3; fam++) {
        for (int defect = 0;; defect++) {
            Call a(fam, MCRAW_RGB_HA), b(fam, MCRAW_RGB_MHC);
            bool more = true;
            for (Call *c : {&a, &b}) {
                switch (defect) {
                case 0: c->null_p = true; break;
                case 1: c->n = -1; break;
                case 2: c->width = 2; break;
                case 3: c->height = 2; break;
                case 4: c->width = 41; break;
                case 5: c->height = 25; break;
                case 6: c->width = 65538, c->pitch = 65538; break;
                case 7: c->in = 0; break;
                case 8: c->in = 0x100001; break;
                case 9: c->pitch = 39; break;
                case 10: c->fstride = 40 * 24 - 1; break;
                case 11: c->p.dtype = 7; break;
                case 12: c->p.flags = 2; break;
                case 13: c->p.cfa = 4; break;
                case 14: c->p.white = 0.0f; break;
                case 15: c->p.white = NAN; break;
                case 16: c->p.black[0] = c->p.black[1] = c->p.black[2] = c->p.black[3] = 5000; break;
                case 17: c->ncolors = 0; break;
                case 18: c->ncolors = 3; break;
                case 19: c->col[0].gain[1] = INFINITY; break;
                case 20: c->col[0].m[5] = NAN; break;
                case 21: c->out = 0; break;
                case 22: c->out = fam == 0 ? 0x200002 : 0x200001; break; // (uint8 outputs have no alignment to miss)
                case 23: c->out_bytes = (fam == 0 ? 2u * 3u * 24u * 40u * 4u : fam == 1 ? 2u * 3u * 24u * 40u : 2u * 24u * 40u * 3u / 2u) - 1u; break;
                case 24: c->d.dtype = 3, c->y.format = 3; break;
                case 25: c->d.layout = 2, c->y.in_bits = 7; break;
                case 26: c->d.reserved = 1, c->y.reserved = 1; break;
                case 27: c->d.lut_log2 = 7, c->y.lut_log2 = 17; break;
                case 28: c->d.lut = nullptr, c->y.lut = nullptr; break;
                case 29: c->d.lut = c->y.lut = reinterpret_cast<const uint16_t *>(0x300008); break;
                case 30: c->y.sh = 25; break;
                case 31: c->y.y_off = 256; break;
                case 32: c->y.cb[1] = 1 << 21, c->y.in_bits = 16; break;
                case 33: c->p.dtype = MCRAW_FLOAT_F32, c->p.flags = fam ? 1u : 0u; break; // (the stage decides the output)
                default: more = false;
                }
            }
            if (!more)
                break;
            RgbPlan A, B;
            const char *wa = a.check(A), *wb = b.check(B);
            // (a defect of the other family's struct, or a uint8 `out` at an odd address, is none: then both calls are accepted)
            CHECK((wa == nullptr) == (wb == nullptr));
            if (wa && wb) {
                rejected++;
                CHECK(!std::strcmp(wa, wb) && std::strcmp(wa, "unknown algo") != 0);
            }
        }
    }
}

// ---- the tile

struct Site {
    int row, col; // tile coordinates of the site an entry of s_g was written for (the tile is rows 0 .. 31, columns 0 .. 255)
    bool set;
};

static void tile(uint32_t W, uint32_t H, uint32_t x0, uint32_t y0, uint32_t S)
{
    static std::vector<int> raw(HA_RAWH * HA_RAWW);
    static std::vector<Site> g(HA_GH * HA_GW);
    std::fill(raw.begin(), raw.end(), 0);
    std::fill(g.begin(), g.end(), Site{0, 0, false});
    const auto rawrd = [&](uint32_t R, uint32_t C) { // a raw sample that is read: inside the array and staged
        CHECK(R < HA_RAWH && C < HA_RAWW && ha_raw_idx(R, C) < raw.size() && raw[ha_raw_idx(R, C)] == 1);
    };
    // stage
    for (uint32_t tid = 0; tid < RGB_T; tid++)
        for (uint32_t i = tid; i < HA_STAGE_ITEMS; i += RGB_T) {
            const uint32_t r = i / HA_RAWCH, q = i % HA_RAWCH;
            for (uint32_t e = 0; e < 8u; e++) {
                const uint32_t idx = ha_raw_idx(r, 8u * q + e);
                CHECK(idx < raw.size());
                if (idx < raw.size())
                    raw[idx]++;
            }
        }
    for (int v : raw)
        CHECK(v == 1);
    // green
    const auto gwr = [&](uint32_t Q, uint32_t K, int row, int col) {
        const uint32_t idx = ha_g_idx(Q, K);
        CHECK(Q < HA_GH && K < HA_GW && idx < g.size() && !g[idx].set);
        // the site is an R / B site of the frame: role 0 or 3 (the ring's coordinates may be -1: parity as two's complement)
        const uint32_t role = (((static_cast<uint32_t>(static_cast<int>(y0) + row) & 1u) * 2u) | (static_cast<uint32_t>(static_cast<int>(x0) + col) & 1u)) ^ S;
        CHECK(role == 0u || role == 3u);
        if (idx < g.size())
            g[idx] = Site{row, col, true};
    };
    for (uint32_t tid = 0; tid < RGB_T; tid++) {
        for (uint32_t i = tid; i < HA_G_MAIN; i += RGB_T) {
            const uint32_t rp = i / (MHC_TW / 8u), q = i % (MHC_TW / 8u);
            for (uint32_t r = 0; r < 6u; r++) {
                rawrd(2u * rp + r, 8u * q + 6u), rawrd(2u * rp + r, 8u * q + 7u); // the 4-byte read
                for (uint32_t e = 8u; e < 18u; e++)
                    rawrd(2u * rp + r, 8u * q + e); // the 16-byte read and the 4-byte read behind it
            }
            for (uint32_t a = 0; a < 2u; a++) {
                const uint32_t xp = ha_rb_xpar((a + 1u) & 1u, S);
                for (uint32_t k = 0; k < 4u; k++) // g row 2 rp + a is tile row 2 rp + a - 1; raw column 8 q + 8 + b is tile column 8 q + b
                    gwr(2u * rp + a, 4u * q + 4u + k, static_cast<int>(2u * rp + a) - 1, static_cast<int>(8u * q + 2u * k + xp));
            }
        }
        if (tid - HA_G_EDGE_T0 < HA_G_EDGE) {
            const uint32_t Q = tid - HA_G_EDGE_T0, C = ha_edge_rawcol(Q, S);
            for (uint32_t dr = 0; dr < 5u; dr++)
                rawrd(Q + dr, C);
            for (int dc = -2; dc <= 2; dc++)
                rawrd(Q + 2u, static_cast<uint32_t>(static_cast<int>(C) + dc));
            gwr(Q, C >> 1, static_cast<int>(Q) - 1, static_cast<int>(C) - 8);
        }
    }
    // estimates: the lanes that have pixels
    for (uint32_t tid = 0; tid < RGB_T; tid++) {
        const uint32_t lx = tid & 31u, ly = tid >> 5;
        if (x0 + 8u * lx >= W)
            continue;
        for (uint32_t pass = 0; pass < MHC_TH / 16u; pass++) {
            const uint32_t tr = 2u * (ly + 8u * pass);
            if (y0 + tr >= H)
                break;
            for (uint32_t r = 0; r < 4u; r++) {
                for (uint32_t e = 6u; e < 18u; e++)
                    rawrd(tr + 2u + r, 8u * lx + e);
                // window row r is tile row tr - 1 + r, window column j tile column 8 lx - 1 + j
                const uint32_t xp = ha_rb_xpar((r + 1u) & 1u, S);
                for (int j = 0; j < 10; j++) {
                    if (((7 + j) & 1) != static_cast<int>(xp))
                        continue; // a green site
                    const uint32_t K = xp ? (j == 0 ? ha_g_extra(xp, lx) : 4u * lx + 4u + static_cast<uint32_t>((j - 2) >> 1))
                                          : (j == 9 ? ha_g_extra(xp, lx) : 4u * lx + 4u + static_cast<uint32_t>((j - 1) >> 1));
                    const uint32_t idx = ha_g_idx(tr + r, K);
                    CHECK(tr + r < HA_GH && K < HA_GW && idx < g.size());
                    if (idx < g.size())
                        CHECK(g[idx].set && g[idx].row == static_cast<int>(tr + r) - 1 && g[idx].col == static_cast<int>(8u * lx) - 1 + j);
                }
            }
        }
    }
}

int main()
{
    plans();
    rejections();
    std::printf("accepted %ld rejected %ld\n", accepted, rejected);
    long tiles = 0;
    const uint32_t sizes[] = {4, 6, 8, 10, 30, 32, 34, 250, 256, 258, 264, 300, 512, 520};
    for (uint32_t W : sizes)
        for (uint32_t H : sizes) {
            if (H > 300u)
                continue;
            for (uint32_t S = 0; S < 4u; S++)
                for (uint32_t y0 = 0; y0 < H; y0 += MHC_TH)
                    for (uint32_t x0 = 0; x0 < W; x0 += MHC_TW)
                        tile(W, H, x0, y0, S), tiles++;
        }
    std::printf("tiles %ld\n", tiles);
    std::printf("cases %ld\n", cases);
    std::printf("wrong %ld\n", wrong);
    return wrong ? 1 : 0;
}
