// area_args_check.cpp -- csrc/mcraw_area_args.h on its own (no HIP: that this file compiles with a plain g++ is part of the test):
// what mcraw_demosaic_area_batch decides with it about a call -- accept, reject or no-op -- against a transcription of the
// contract (include/mcraw_hip.h), one defect at a time and seeded tuples; the plan's invariants (the workgroup's tile covers the
// output, its LDS segment holds every tap of every column of every tile, the weights fit); the taps (256 in all, none behind the
// crop, no more than the bound); the layout of the scratch; and that rgb_check keeps turning algo 3 down.
#include <cstdio>
#include <cstring>
#include <random>

#include "mcraw_area_args.h"

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
    mcraw_rgb p;
    mcraw_area a;
    mcraw_display d;
    mcraw_yuv y;
    bool has_p = true, has_a = true, has_d = false, has_y = false;
    mcraw_rgb_color col[3];
    int ncolors = 1;
    uintptr_t in = 0x10000, out = 0x4000000, work = 0x8000000;
    size_t pitch = 64, fstride = 64 * 32, work_bytes = 1 << 20, out_bytes = 1 << 20;
    int width = 64, height = 32, n = 2;
};

static Call good()
{
    Call c;
    std::memset(&c.p, 0, sizeof c.p);
    std::memset(&c.a, 0, sizeof c.a);
    std::memset(&c.d, 0, sizeof c.d);
    std::memset(&c.y, 0, sizeof c.y);
    c.p.algo = MCRAW_RGB_AREA, c.p.dtype = MCRAW_FLOAT_F32, c.p.cfa = MCRAW_CFA_GRBG, c.p.white = 4095.0f;
    c.a.x0 = 4, c.a.y0 = 2, c.a.cw = 56, c.a.ch = 28, c.a.out_w = 10, c.a.out_h = 6;
    c.d.dtype = MCRAW_DISP_U8, c.d.layout = MCRAW_DISP_HWC, c.d.lut_log2 = 12, c.d.lut = reinterpret_cast<const uint16_t *>(0x20000);
    c.y.format = MCRAW_YUV_NV12, c.y.lut_log2 = 12, c.y.in_bits = 8, c.y.sh = 8, c.y.y_off = 16, c.y.c_off = 128;
    c.y.cy[0] = 47, c.y.cy[1] = 157, c.y.cy[2] = 16, c.y.cb[0] = -26, c.y.cb[1] = -86, c.y.cb[2] = 112;
    c.y.cr[0] = 112, c.y.cr[1] = -102, c.y.cr[2] = -10, c.y.lut = reinterpret_cast<const uint16_t *>(0x20000);
    for (auto &k : c.col) {
        std::memset(&k, 0, sizeof k);
        k.gain[0] = k.gain[1] = k.gain[2] = 1.0f, k.m[0] = k.m[4] = k.m[8] = 1.0f;
    }
    return c;
}

static const char *run(const Call &c, AreaPlan &P)
{
    return area_check(c.has_p ? &c.p : nullptr, c.has_a ? &c.a : nullptr, c.has_d ? &c.d : nullptr, c.has_y ? &c.y : nullptr, c.col,
                      c.ncolors, reinterpret_cast<const uint16_t *>(c.in), c.pitch, c.fstride, c.width, c.height, c.n,
                      reinterpret_cast<const void *>(c.work), c.work_bytes, reinterpret_cast<const void *>(c.out), c.out_bytes, P);
}

// The geometry rules of the contract, transcribed: 0 accept, 1 reject.
static int expect_geometry(const Call &c)
{
    const mcraw_area &a = c.a;
    if (a.reserved[0] || a.reserved[1])
        return 1;
    if ((a.x0 | a.y0 | a.cw | a.ch) & 1u)
        return 1;
    if (a.cw < 2 || a.ch < 2)
        return 1;
    if (static_cast<uint64_t>(a.x0) + a.cw > static_cast<uint64_t>(c.width) || static_cast<uint64_t>(a.y0) + a.ch > static_cast<uint64_t>(c.height))
        return 1;
    const uint64_t Qw = a.cw / 2, Qh = a.ch / 2;
    if (a.out_w < 1 || a.out_w > Qw || Qw > 16ull * a.out_w || a.out_h < 1 || a.out_h > Qh || Qh > 16ull * a.out_h)
        return 1;
    if (c.has_y && ((a.out_w | a.out_h) & 1u))
        return 1;
    const uint64_t es = c.has_d ? (c.d.dtype == MCRAW_DISP_U8 ? 1 : 2) : c.has_y ? (c.y.format == MCRAW_YUV_NV12 ? 1 : 2)
                                                                               : (c.p.dtype == MCRAW_FLOAT_F32 ? 4 : 2);
    const uint64_t frame = (c.has_y ? static_cast<uint64_t>(a.out_w) * a.out_h * 3 / 2 : 3ull * a.out_w * a.out_h) * es;
    if (c.out_bytes < frame * static_cast<uint64_t>(c.n))
        return 1;
    if (!c.out || (c.out & (es - 1)))
        return 1;
    if (!c.work || (c.work & 15u))
        return 1;
    return 0;
}

static void check_taps(uint32_t Q, uint32_t O)
{
    for (uint32_t k = 0; k < O; k += (O > 64 ? O / 37 + 1 : 1)) {
        AreaTap t;
        area_taps(k, Q, O, t);
        uint32_t sum = 0, last = 0;
        for (uint32_t i = 0; i < AREA_TAPS; i++) {
            sum += t.w[i];
            if (t.w[i])
                last = i + 1;
        }
        CHECK(sum == 256u && last == t.nt && t.nt >= 1u);
        CHECK(t.q0 == static_cast<uint32_t>(static_cast<uint64_t>(k) * Q / O) && t.q0 + t.nt <= Q);
        CHECK(t.nt <= area_tap_bound(Q, O) && area_tap_bound(Q, O) <= AREA_TAPS);
        CHECK(area_c(k, t.q0, Q, O) == 0 && area_c(k, t.q0 + t.nt, Q, O) == 256);
    }
}

// What the kernel relies on: every index it forms from the plan stays inside its LDS arrays, and the tiles cover the output.
static void check_plan(const Call &c, const AreaPlan &P)
{
    const uint32_t Wo = c.a.out_w, Ho = c.a.out_h, lx = 1u << P.lx_log2;
    CHECK(P.Qw == c.a.cw / 2 && P.Qh == c.a.ch / 2 && P.rgb.Wo == Wo && P.rgb.Ho == Ho);
    CHECK(P.ly >= 1u && lx * P.ly <= RGB_T && (P.ly & (P.ly - 1u)) == 0u);
    CHECK(P.ly * P.segp <= AREA_TILE_Q && 8u * lx * P.ntx <= AREA_WXN && 2u * P.ly <= AREA_YN);
    CHECK(P.seg % 4u == 0u && P.nch == P.seg / 4u && P.segp >= P.seg + (P.seg - 1u) / 8u + 1u);
    CHECK(static_cast<uint64_t>(P.tilesX) * lx * 8u >= Wo && static_cast<uint64_t>(P.tilesX - 1u) * lx * 8u < Wo);
    CHECK(static_cast<uint64_t>(P.groups) * P.ly * 2u >= Ho && static_cast<uint64_t>(P.groups - 1u) * P.ly * 2u < Ho);
    CHECK(P.bands == (P.groups + AREA_BAND - 1u) / AREA_BAND && P.units == P.tilesX * P.bands);
    CHECK(P.ntx == area_tap_bound(P.Qw, Wo) && P.nty == area_tap_bound(P.Qh, Ho));
    for (uint32_t cidx = 0; cidx < P.ly * P.nch; cidx += (P.ly * P.nch > 512u ? 97u : 1u)) { // the staging's division by nch
        const uint32_t q = static_cast<uint32_t>((static_cast<uint64_t>(cidx) * P.nch_magic) >> 32);
        CHECK(q == cidx / P.nch);
    }
    for (uint32_t tx = 0; tx < P.tilesX; tx++) { // every tap of every column of the tile lies in the segment
        const uint32_t k0 = tx * 8u * lx, k1 = std::min(Wo, k0 + 8u * lx);
        AreaTap t;
        area_taps(k0, P.Qw, Wo, t);
        const uint32_t qb = (c.a.x0 / 2u + t.q0) & ~7u;
        for (uint32_t k = k0; k < k1; k += (k1 - k0 > 64u && k + 40u < k1 ? 13u : 1u)) {
            area_taps(k, P.Qw, Wo, t);
            CHECK(c.a.x0 / 2u + t.q0 >= qb && c.a.x0 / 2u + t.q0 - qb + t.nt <= P.seg);
        }
        area_taps(k1 - 1u, P.Qw, Wo, t);
        CHECK(c.a.x0 / 2u + t.q0 - qb + t.nt <= P.seg);
    }
    // the scratch: two tables of 40-byte entries that do not overlap, sections on multiples of 256
    CHECK(P.xtab == 0u && P.ytab % AREA_SECTION == 0u && P.total % AREA_SECTION == 0u);
    CHECK(P.ytab >= static_cast<size_t>(Wo) * sizeof(AreaTap) && P.total >= P.ytab + static_cast<size_t>(Ho) * sizeof(AreaTap));
    CHECK(P.total < P.ytab + static_cast<size_t>(Ho) * sizeof(AreaTap) + AREA_SECTION);
}

static void decide(const Call &c, int want) // 0 accept, 1 reject, 2 no-op
{
    AreaPlan P;
    const char *why = run(c, P);
    const int got = why ? 1 : P.rgb.noop ? 2 : 0;
    CHECK(got == want);
    if (got != want && wrong < 20)
        std::printf("  want %d got %d (%s)\n", want, got, why ? why : "-");
    if (got == 0) {
        accepted++;
        check_plan(c, P);
    } else if (got == 1) {
        rejected++;
    }
}

int main()
{
    // the rules, one defect at a time
    decide(good(), 0);
    {
        Call c = good();
        c.n = 0;
        decide(c, 2);
        c.has_d = c.has_y = true; // (both stages are turned down in front of the no-op)
        decide(c, 1);
        c = good(), c.n = -1;
        decide(c, 1);
        c = good(), c.has_p = false;
        decide(c, 1);
        c = good(), c.has_a = false;
        decide(c, 1);
        c = good(), c.has_d = c.has_y = true, c.p.dtype = 0;
        decide(c, 1);
        for (uint32_t algo : {0u, 1u, 2u, 4u, 0xffffffffu}) {
            c = good(), c.p.algo = algo;
            decide(c, 1);
        }
        c = good(), c.has_d = true, c.p.dtype = 0, decide(c, 0);
        c = good(), c.has_y = true, c.p.dtype = 0, decide(c, 0);
        c = good(), c.has_d = true, decide(c, 1);                  // p->dtype must be 0 beside a stage
        c = good(), c.has_y = true, c.p.dtype = 0, c.a.out_w = 9, decide(c, 1); // 4:2:0 needs even sizes
        c = good(), c.has_y = true, c.p.dtype = 0, c.a.out_h = 5, decide(c, 1);
        c = good(), c.a.out_w = 9, c.a.out_h = 5, decide(c, 0);
        c = good(), c.a.x0 = 5, decide(c, 1);
        c = good(), c.a.y0 = 3, decide(c, 1);
        c = good(), c.a.cw = 55, decide(c, 1);
        c = good(), c.a.ch = 27, decide(c, 1);
        c = good(), c.a.cw = 0, decide(c, 1);
        c = good(), c.a.ch = 0, decide(c, 1);
        c = good(), c.a.x0 = 10, decide(c, 1);                     // 10 + 56 > 64
        c = good(), c.a.y0 = 6, decide(c, 1);
        c = good(), c.a.x0 = 8, c.a.y0 = 4, decide(c, 0);          // exactly to the edges
        c = good(), c.a.x0 = 0xfffffffeu, c.a.cw = 4, decide(c, 1); // (no wrap)
        c = good(), c.a.out_w = 29, decide(c, 1);                  // more pixels than quads
        c = good(), c.a.out_w = 28, decide(c, 0);
        c = good(), c.a.out_h = 15, decide(c, 1);
        c = good(), c.a.out_h = 14, decide(c, 0);
        c = good(), c.a.out_w = 1, decide(c, 1);                   // 28 quads onto 1 pixel
        c = good(), c.a.out_w = 2, decide(c, 0);                   // 14 per pixel
        c = good(), c.a.cw = 32, c.a.out_w = 1, decide(c, 0);      // the limit: 16
        c = good(), c.a.cw = 34, c.a.out_w = 1, decide(c, 1);
        c = good(), c.a.out_w = 0, decide(c, 1);
        c = good(), c.a.out_h = 0, decide(c, 1);
        c = good(), c.a.reserved[0] = 1, decide(c, 1);
        c = good(), c.a.reserved[1] = 1, decide(c, 1);
        c = good(), c.work = 0, decide(c, 1);
        c = good(), c.work += 8, decide(c, 1);
        {
            AreaPlan P;
            c = good();
            CHECK(P.geometry(&c.a) == nullptr);
            c.work_bytes = P.total, decide(c, 0);
            c.work_bytes = P.total - 1, decide(c, 1);
            c.work_bytes = 0, decide(c, 1);
        }
        c = good(), c.out_bytes = 2 * 3 * 10 * 6 * 4, decide(c, 0);
        c = good(), c.out_bytes = 2 * 3 * 10 * 6 * 4 - 1, decide(c, 1);
        c = good(), c.out = 0, decide(c, 1);
        c = good(), c.out += 2, decide(c, 1);
        c = good(), c.p.dtype = MCRAW_FLOAT_F16, c.out += 2, decide(c, 0);
        c = good(), c.in = 0, decide(c, 1);
        c = good(), c.in += 1, decide(c, 1);
        c = good(), c.width = 63, decide(c, 1);
        c = good(), c.height = 2, c.a.y0 = 0, c.a.ch = 2, c.a.out_h = 1, decide(c, 1);
        c = good(), c.pitch = 62, decide(c, 1);
        c = good(), c.fstride = 64 * 31, decide(c, 1);
        c = good(), c.ncolors = 3, decide(c, 1);
        c = good(), c.ncolors = 2, decide(c, 0);
        c = good(), c.p.cfa = 4, decide(c, 1);
        c = good(), c.p.dtype = 0, decide(c, 1);
        c = good(), c.p.flags = 2, decide(c, 1);
        c = good(), c.p.flags = MCRAW_FLOAT_CLIP, decide(c, 0);
        c = good(), c.p.white = 0.0f, decide(c, 1);
        c = good(), c.col[0].m[3] = 1.0f / 0.0f, decide(c, 1);
        c = good(), c.has_d = true, c.p.dtype = 0, c.d.lut_log2 = 7, decide(c, 1);
        c = good(), c.has_d = true, c.p.dtype = 0, c.d.reserved = 1, decide(c, 1);
        c = good(), c.has_d = true, c.p.dtype = 0, c.d.lut = nullptr, decide(c, 1);
        c = good(), c.has_y = true, c.p.dtype = 0, c.y.sh = 0, decide(c, 1);
        c = good(), c.has_y = true, c.p.dtype = 0, c.y.cy[0] = 1 << 30, decide(c, 1);
    }
    // the staging mode
    {
        AreaPlan P;
        Call c = good();
        CHECK(!run(c, P) && P.mode == 2u);
        c.pitch = 66;
        c.fstride = 66 * 32;
        CHECK(!run(c, P) && P.mode == 1u);
        c.in += 2;
        CHECK(!run(c, P) && P.mode == 0u);
        c = good(), c.fstride += 1;
        CHECK(!run(c, P) && P.mode == 0u);
        c.n = 1;
        CHECK(!run(c, P) && P.mode == 2u);
    }
    // rgb_check keeps turning algo 3 down, in front of everything that concerns the stage
    {
        Call c = good();
        RgbPlan R;
        const char *why = rgb_check(&c.p, nullptr, nullptr, c.col, 1, reinterpret_cast<const uint16_t *>(c.in), c.pitch, c.fstride, c.width,
                                    c.height, c.n, reinterpret_cast<const void *>(c.out), c.out_bytes, R);
        CHECK(why && !std::strcmp(why, "unknown algo"));
        c.p.dtype = 0;
        why = rgb_check(&c.p, &c.d, nullptr, c.col, 1, reinterpret_cast<const uint16_t *>(c.in), c.pitch, c.fstride, c.width, c.height, c.n,
                        reinterpret_cast<const void *>(c.out), c.out_bytes, R);
        CHECK(why && !std::strcmp(why, "unknown algo"));
        why = rgb_check(&c.p, nullptr, &c.y, c.col, 1, reinterpret_cast<const uint16_t *>(c.in), c.pitch, c.fstride, c.width, c.height, c.n,
                        reinterpret_cast<const void *>(c.out), c.out_bytes, R);
        CHECK(why && !std::strcmp(why, "unknown algo"));
        c.p.algo = MCRAW_RGB_BIN2, c.p.dtype = MCRAW_FLOAT_F32;
        CHECK(!rgb_check(&c.p, nullptr, nullptr, c.col, 1, reinterpret_cast<const uint16_t *>(c.in), c.pitch, c.fstride, c.width, c.height,
                         c.n, reinterpret_cast<const void *>(c.out), c.out_bytes, R) &&
              R.Wo == 32u && R.Ho == 16u && !R.mhc && R.es == 4u && R.shift == 1 && R.out_frame == 3u * 32u * 16u * 4u && R.invec);
    }
    // the taps
    for (uint32_t Q : {1u, 2u, 3u, 47u, 63u, 1920u, 2016u, 32768u})
        for (uint32_t O : {(Q + 15u) / 16u, (Q + 15u) / 16u + 1u, Q / 3u, Q * 10u / 21u, (Q + 1u) / 2u, Q - 1u, Q})
            if (O >= 1u && O <= Q && Q <= 16u * O)
                check_taps(Q, O);
    // seeded tuples: geometry, families, pointers
    std::mt19937_64 rng(12345);
    const auto pick = [&](uint32_t lo, uint32_t hi) { return lo + static_cast<uint32_t>(rng() % (hi - lo + 1u)); };
    for (int it = 0; it < 60000; it++) {
        Call c = good();
        const bool big = it % 8 == 0;
        c.width = static_cast<int>(2u * pick(2, big ? 32768 : 300));
        c.height = static_cast<int>(2u * pick(2, big ? 2000 : 200));
        c.n = static_cast<int>(pick(1, 3));
        c.pitch = static_cast<size_t>(c.width) + (rng() % 3 ? 0 : pick(0, 9));
        c.fstride = c.pitch * static_cast<size_t>(c.height) + pick(0, 5);
        c.a.cw = pick(0, static_cast<uint32_t>(c.width) + 2u);
        c.a.ch = pick(0, static_cast<uint32_t>(c.height) + 2u);
        if (rng() % 8) // mostly even, mostly inside
            c.a.cw &= ~1u, c.a.ch &= ~1u;
        c.a.x0 = c.a.cw <= static_cast<uint32_t>(c.width) ? pick(0, static_cast<uint32_t>(c.width) - c.a.cw + (rng() % 16 ? 0 : 2)) : 0;
        c.a.y0 = c.a.ch <= static_cast<uint32_t>(c.height) ? pick(0, static_cast<uint32_t>(c.height) - c.a.ch + (rng() % 16 ? 0 : 2)) : 0;
        if (rng() % 8)
            c.a.x0 &= ~1u, c.a.y0 &= ~1u;
        const uint32_t Qw = c.a.cw / 2u, Qh = c.a.ch / 2u;
        c.a.out_w = rng() % 6 ? pick((Qw + 15u) / 16u, Qw ? Qw : 1u) : pick(0, Qw + 3u);
        c.a.out_h = rng() % 6 ? pick((Qh + 15u) / 16u, Qh ? Qh : 1u) : pick(0, Qh + 3u);
        const int fam = static_cast<int>(rng() % 3);
        c.has_d = fam == 1, c.has_y = fam == 2;
        c.p.dtype = fam ? 0u : pick(1, 3);
        if (fam == 1)
            c.d.dtype = pick(1, 2);
        if (fam == 2)
            c.y.format = pick(1, 2);
        if (rng() % 32 == 0)
            c.a.reserved[rng() % 2] = 1;
        if (rng() % 32 == 0)
            c.work = rng() % 2 ? 0 : c.work + 4;
        if (rng() % 32 == 0)
            c.out = rng() % 2 ? 0 : c.out + 1;
        c.out_bytes = rng() % 16 ? (size_t{1} << 40) : pick(0, 4000);
        AreaPlan G;
        const bool geo_ok = G.geometry(&c.a) == nullptr;
        c.work_bytes = geo_ok && rng() % 16 == 0 ? G.total - 1u : size_t{1} << 30;
        int want = expect_geometry(c);
        if (!want && c.work_bytes < G.total)
            want = 1;
        decide(c, want);
    }
    std::printf("accepted %ld rejected %ld\ncases %ld\nwrong %ld\n", accepted, rejected, cases, wrong);
    return wrong ? 1 : 0;
}
