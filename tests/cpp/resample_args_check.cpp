// resample_args_check.cpp -- csrc/mcraw_resample_args.h on its own (no HIP: that this file compiles with a plain g++ is part of
// the test): the taps against a transcription of the contract (include/mcraw_hip.h) for every legal (C, O) with C <= 96 and both
// filters -- 4096 in all, no more than 5 / 9, the identity at O = C, pixel k mirrored by pixel O - 1 - k, no tap more than 4
// beyond the crop --; what mcraw_demosaic_resample_batch decides about a call, one defect at a time and seeded tuples; the plan's
// invariants (the tiles cover the output, every tap of every column and row of every tile lies in the workgroup's LDS arrays); the
// layout of the scratch; and that rgb_check and area_check keep turning algo 4 down.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "mcraw_area_args.h"
#include "mcraw_resample_args.h"

using namespace mcraw;

static long cases = 0, wrong = 0, accepted = 0, rejected = 0;
static long max_abs_w[2] = {0, 0};
static unsigned max_nt[2] = {0, 0};

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
    mcraw_resample r;
    mcraw_display d;
    mcraw_yuv y;
    bool has_p = true, has_r = true, has_d = false, has_y = false;
    mcraw_rgb_color col[3];
    int ncolors = 1;
    uintptr_t in = 0x10000, out = 0x4000000, work = 0x8000000;
    size_t pitch = 64, fstride = 64 * 32, work_bytes = 1 << 20, out_bytes = 1 << 22;
    int width = 64, height = 32, n = 2;
};

static Call good()
{
    Call c;
    std::memset(&c.p, 0, sizeof c.p);
    std::memset(&c.r, 0, sizeof c.r);
    std::memset(&c.d, 0, sizeof c.d);
    std::memset(&c.y, 0, sizeof c.y);
    c.p.algo = MCRAW_RGB_RESAMPLE, c.p.dtype = MCRAW_FLOAT_F32, c.p.cfa = MCRAW_CFA_GRBG, c.p.white = 4095.0f;
    c.r.x0 = 4, c.r.y0 = 2, c.r.cw = 56, c.r.ch = 28, c.r.out_w = 40, c.r.out_h = 30, c.r.filter = MCRAW_FILTER_CUBIC;
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

static const char *run(const Call &c, ResamplePlan &P)
{
    return resample_check(c.has_p ? &c.p : nullptr, c.has_r ? &c.r : nullptr, c.has_d ? &c.d : nullptr, c.has_y ? &c.y : nullptr, c.col,
                          c.ncolors, reinterpret_cast<const uint16_t *>(c.in), c.pitch, c.fstride, c.width, c.height, c.n,
                          reinterpret_cast<const void *>(c.work), c.work_bytes, reinterpret_cast<const void *>(c.out), c.out_bytes, P);
}

// The geometry rules of the contract, transcribed: 0 accept, 1 reject.
static int expect_geometry(const Call &c)
{
    const mcraw_resample &r = c.r;
    if (c.width < 8 || c.height < 8)
        return 1;
    if (r.reserved || r.filter > 1u)
        return 1;
    if ((r.x0 | r.y0 | r.cw | r.ch) & 1u)
        return 1;
    if (r.cw < 2 || r.ch < 2)
        return 1;
    if (static_cast<uint64_t>(r.x0) + r.cw > static_cast<uint64_t>(c.width) || static_cast<uint64_t>(r.y0) + r.ch > static_cast<uint64_t>(c.height))
        return 1;
    if ((r.cw + 1ull) / 2 > r.out_w || r.out_w > 2ull * r.cw || (r.ch + 1ull) / 2 > r.out_h || r.out_h > 2ull * r.ch)
        return 1;
    if (c.has_y && ((r.out_w | r.out_h) & 1u))
        return 1;
    const uint64_t es = c.has_d ? (c.d.dtype == MCRAW_DISP_U8 ? 1 : 2) : c.has_y ? (c.y.format == MCRAW_YUV_NV12 ? 1 : 2)
                                                                               : (c.p.dtype == MCRAW_FLOAT_F32 ? 4 : 2);
    const uint64_t frame = (c.has_y ? static_cast<uint64_t>(r.out_w) * r.out_h * 3 / 2 : 3ull * r.out_w * r.out_h) * es;
    if (c.out_bytes < frame * static_cast<uint64_t>(c.n))
        return 1;
    if (!c.out || (c.out & (es - 1)))
        return 1;
    if (!c.work || (c.work & 15u))
        return 1;
    return 0;
}

// The contract's weights of pixel k, written from the header's lines and not from resample_taps: over every j from -8 to C + 8.
static void contract_taps(long k, long C, long O, int filter, long long (&w)[256], long &jfirst, long &jlast)
{
    const long long D = 2 * std::max(C, O);
    long long f[256], F = 0;
    jfirst = 1 << 30, jlast = -(1 << 30);
    for (long j = -8; j < C + 8; j++) {
        const long long n = 2ll * O * j - ((2ll * k + 1) * C - O);
        const long long a = (1024 * std::llabs(n) + D / 2) / D;
        long long v;
        if (filter == 0)
            v = std::max(0ll, 1024 - a);
        else if (a <= 1024)
            v = 3 * a * a * a - 5 * 1024 * a * a + 2ll * 1024 * 1024 * 1024;
        else if (a < 2048)
            v = -a * a * a + 5 * 1024 * a * a - 8ll * 1024 * 1024 * a + 4ll * 1024 * 1024 * 1024;
        else
            v = 0;
        f[j + 8] = v;
        F += v;
        if (v != 0) {
            jfirst = std::min(jfirst, j);
            jlast = j;
        }
    }
    long long sum = 0, best = -1;
    long near[2] = {0, 0};
    int nnear = 0;
    for (long j = -8; j < C + 8; j++) {
        const long long num = 4096 * f[j + 8] + F / 2;
        w[j + 8] = num >= 0 ? num / F : -((-num + F - 1) / F);
        sum += w[j + 8];
        const long long an = std::llabs(2ll * O * j - ((2ll * k + 1) * C - O));
        if (best < 0 || an < best)
            best = an, near[0] = j, nnear = 1;
        else if (an == best)
            near[1] = j, nnear = 2;
    }
    const long long res = 4096 - sum;
    if (nnear == 1) {
        w[near[0] + 8] += res;
    } else {
        w[near[0] + 8] += res - res / 2;
        w[near[1] + 8] += res / 2;
    }
}

static void check_taps(uint32_t C, uint32_t O, uint32_t filter)
{
    const uint32_t cap = filter ? 9u : 5u;
    ResampleTap prev{};
    for (uint32_t k = 0; k < O; k++) {
        ResampleTap t, m;
        resample_taps(k, C, O, filter, t);
        resample_taps(O - 1u - k, C, O, filter, m);
        long sum = 0, sabs = 0;
        bool tail0 = true;
        for (uint32_t i = 0; i < RES_TAPS; i++) {
            sum += t.w[i];
            sabs += std::labs(t.w[i]);
            if (i >= t.nt && t.w[i] != 0)
                tail0 = false;
        }
        max_abs_w[filter] = std::max(max_abs_w[filter], sabs);
        max_nt[filter] = std::max<unsigned>(max_nt[filter], t.nt);
        CHECK(sum == 4096 && tail0 && t.nt >= 1u);
        CHECK(t.nt <= cap && t.nt <= res_tap_bound(C, O, filter));
        CHECK(t.j0 >= -4 && t.j0 + static_cast<int>(t.nt) - 1 <= static_cast<int>(C) + 3);
        if (C == O)
            CHECK(t.nt == 1u && t.j0 == static_cast<int>(k) && t.w[0] == 4096);
        // the mirror: tap i of pixel k is tap nt - 1 - i of pixel O - 1 - k, at sample C - 1 - j
        bool mir = m.nt == t.nt && m.j0 == static_cast<int>(C) - 1 - (t.j0 + static_cast<int>(t.nt) - 1);
        for (uint32_t i = 0; mir && i < t.nt; i++)
            mir = t.w[i] == m.w[t.nt - 1u - i];
        CHECK(mir);
        // neighbours' taps lie within the span bound (a pixel that sits on a sample has one tap, inside its neighbours' windows)
        if (k > 0)
            CHECK(static_cast<uint32_t>(std::max(t.j0 + t.nt, prev.j0 + prev.nt) - std::min(t.j0, prev.j0)) <=
                  res_span_bound(1u, C, O, res_tap_bound(C, O, filter)));
        prev = t;
        // the contract, transcribed
        long long w[256];
        long jf, jl;
        contract_taps(k, C, O, static_cast<int>(filter), w, jf, jl);
        bool same = jf == t.j0 && jl == t.j0 + static_cast<long>(t.nt) - 1;
        for (long j = -8; same && j < static_cast<long>(C) + 8; j++) {
            const long i = j - t.j0;
            same = w[j + 8] == (i >= 0 && i < static_cast<long>(t.nt) ? t.w[i] : 0);
        }
        CHECK(same);
    }
}

// What the kernel relies on: every index it forms stays inside its LDS arrays, and the tiles cover the output.
static void check_axis(uint32_t origin, uint32_t C, uint32_t O, uint32_t filter, uint32_t tile, uint32_t grid, uint32_t room)
{
    for (uint32_t k0 = 0; k0 < O; k0 += tile) {
        const uint32_t k1 = std::min(O, k0 + tile) - 1u;
        // as the kernel finds a tile's window: the first tap of its first two pixels, the last tap of its last two (a pixel that
        // sits on a sample has a single tap, which may start behind its right neighbour's and end in front of its left one's)
        ResampleTap a, a2, b, b2, t;
        resample_taps(k0, C, O, filter, a);
        resample_taps(std::min(k0 + 1u, k1), C, O, filter, a2);
        resample_taps(k1, C, O, filter, b);
        resample_taps(std::max(k1, k0 + 1u) - 1u, C, O, filter, b2);
        const int first = static_cast<int>(origin) + std::min(a.j0, a2.j0);
        const int last = static_cast<int>(origin) + std::max(b.j0 + static_cast<int>(b.nt), b2.j0 + static_cast<int>(b2.nt)) - 1;
        const int base = first & ~static_cast<int>(grid - 1u);
        CHECK(static_cast<uint32_t>(last - base) < room);
        for (uint32_t k = k0; k <= k1; k++) {
            resample_taps(k, C, O, filter, t);
            CHECK(static_cast<int>(origin) + t.j0 >= base && static_cast<uint32_t>(static_cast<int>(origin) + t.j0 + t.nt - 1 - base) < room);
        }
    }
}

static void check_plan(const Call &c, const ResamplePlan &P)
{
    const uint32_t Wo = c.r.out_w, Ho = c.r.out_h;
    CHECK(P.rgb.Wo == Wo && P.rgb.Ho == Ho);
    CHECK(P.ly >= 1u && P.ly <= RES_LYMAX && (P.ly & (P.ly - 1u)) == 0u && 8u * P.ly <= RGB_T);
    CHECK(P.ecols <= RES_ECOLS && P.ecols % 8u == 0u && P.erows <= RES_TROWS && P.erows % 2u == 0u);
    CHECK(P.ecols + 16u <= RES_RAWW && RES_TW + 4u <= RES_TSTRIDE);
    CHECK(static_cast<uint64_t>(P.tilesX) * RES_TW >= Wo && static_cast<uint64_t>(P.tilesX - 1u) * RES_TW < Wo);
    CHECK(static_cast<uint64_t>(P.bands) * P.ly * 2u >= Ho && static_cast<uint64_t>(P.bands - 1u) * P.ly * 2u < Ho);
    CHECK(P.units == P.tilesX * P.bands);
    CHECK(P.ntx == res_tap_bound(c.r.cw, Wo, c.r.filter) && P.nty == res_tap_bound(c.r.ch, Ho, c.r.filter));
    check_axis(c.r.x0, c.r.cw, Wo, c.r.filter, RES_TW, 8u, P.ecols);
    check_axis(c.r.y0, c.r.ch, Ho, c.r.filter, 2u * P.ly, 2u, P.erows);
    // the scratch: two tables of 24-byte entries that do not overlap, sections on multiples of 256
    CHECK(P.xtab == 0u && P.ytab % RES_SECTION == 0u && P.total % RES_SECTION == 0u);
    CHECK(P.ytab >= static_cast<size_t>(Wo) * sizeof(ResampleTap) && P.total >= P.ytab + static_cast<size_t>(Ho) * sizeof(ResampleTap));
    CHECK(P.total < P.ytab + static_cast<size_t>(Ho) * sizeof(ResampleTap) + RES_SECTION);
}

static void decide(const Call &c, int want) // 0 accept, 1 reject, 2 no-op
{
    ResamplePlan P;
    const char *why = run(c, P);
    const int got = why ? 1 : P.rgb.noop ? 2 : 0;
    CHECK(got == want);
    if (got == 0) {
        accepted++;
        check_plan(c, P);
    } else if (got == 1) {
        rejected++;
    }
}

int main()
{
    // the taps: every legal (C, O), C <= 96, both filters
    for (uint32_t filter = 0; filter < 2u; filter++)
        for (uint32_t C = 1; C <= 96u; C++)
            for (uint32_t O = (C + 1u) / 2u; O <= 2u * C; O++)
                check_taps(C, O, filter);
    CHECK(max_nt[0] <= 5u && max_nt[1] <= 9u);
    CHECK(max_abs_w[0] == 4096 && max_abs_w[1] >= 4096 && max_abs_w[1] <= 5600); // the header's bound on sum |w|
    std::printf("max taps %u %u  max sum |w| %ld %ld\n", max_nt[0], max_nt[1], max_abs_w[0], max_abs_w[1]);
    // large sizes: the 64-bit path
    for (uint32_t filter = 0; filter < 2u; filter++) {
        const uint32_t big[][2] = {{65536, 65536}, {65536, 32768}, {65536, 131072}, {4032, 3840}, {2268, 2160}, {3840, 2560}, {3456, 3840}};
        for (const auto &g : big)
            for (uint32_t k : {0u, 1u, g[1] / 2u, g[1] - 2u, g[1] - 1u}) {
                ResampleTap t;
                resample_taps(k, g[0], g[1], filter, t);
                long sum = 0;
                for (uint32_t i = 0; i < RES_TAPS; i++)
                    sum += t.w[i];
                CHECK(sum == 4096 && t.nt <= res_tap_bound(g[0], g[1], filter) && t.j0 >= -4 && t.j0 + static_cast<int>(t.nt) - 1 <= static_cast<int>(g[0]) + 3);
            }
    }

    // one defect at a time
    decide(good(), 0);
    {
        Call c = good();
        c.n = 0;
        decide(c, 2);
        c.has_r = false;
        decide(c, 1);
    }
#define BAD(stmt)                                                                                                      \
    do {                                                                                                               \
        Call c = good();                                                                                               \
        stmt;                                                                                                          \
        decide(c, 1);                                                                                                  \
    } while (0)
#define OK(stmt)                                                                                                       \
    do {                                                                                                               \
        Call c = good();                                                                                               \
        stmt;                                                                                                          \
        decide(c, 0);                                                                                                  \
    } while (0)
    BAD(c.has_p = false);
    BAD(c.has_r = false);
    BAD(c.n = -1);
    BAD(c.has_d = c.has_y = true; c.p.dtype = 0);
    for (uint32_t algo : {0u, 1u, 2u, 3u, 5u})
        BAD(c.p.algo = algo);
    BAD(c.r.reserved = 1);
    BAD(c.r.filter = 2);
    OK(c.r.filter = MCRAW_FILTER_LINEAR);
    BAD(c.r.x0 = 3);
    BAD(c.r.y0 = 1);
    BAD(c.r.cw = 55);
    BAD(c.r.ch = 27);
    BAD(c.r.cw = 0);
    BAD(c.r.ch = 0);
    BAD(c.r.x0 = 10);  // x0 + cw = 66 > 64
    BAD(c.r.y0 = 6);   // y0 + ch = 34 > 32
    BAD(c.r.out_w = 27);  // under cw / 2
    OK(c.r.out_w = 28);
    OK(c.r.out_w = 112);
    BAD(c.r.out_w = 113); // over 2 cw
    BAD(c.r.out_h = 13);
    OK(c.r.out_h = 14);
    OK(c.r.out_h = 56);
    BAD(c.r.out_h = 57);
    OK(c.r.out_w = 56; c.r.out_h = 28);
    BAD(c.width = 6; c.pitch = 8; c.r.x0 = 0; c.r.cw = 6; c.r.out_w = 6);  // frames under 8
    BAD(c.height = 6; c.r.y0 = 0; c.r.ch = 6; c.r.out_h = 6);
    OK(c.width = 8; c.height = 8; c.pitch = 8; c.fstride = 64; c.r.x0 = c.r.y0 = 0; c.r.cw = c.r.ch = 8; c.r.out_w = c.r.out_h = 9);
    BAD(c.width = 63);
    BAD(c.work = 0);
    BAD(c.work += 8);
    BAD(c.work_bytes = 0);
    BAD(c.out = 0);
    BAD(c.out += 2);
    BAD(c.out_bytes = 2 * 3 * 40 * 30 * 4 - 1);
    OK(c.out_bytes = 2 * 3 * 40 * 30 * 4);
    BAD(c.in = 0);
    BAD(c.in += 1);
    BAD(c.pitch = 62);
    BAD(c.ncolors = 3);
    BAD(c.p.dtype = 7);
    BAD(c.p.cfa = 4);
    BAD(c.p.flags = 2);
    BAD(c.p.white = 0.0f);
    OK(c.has_d = true; c.p.dtype = 0);
    BAD(c.has_d = true); // the display family decides the output: p->dtype must be 0
    BAD(c.has_d = true; c.p.dtype = 0; c.d.reserved = 1);
    BAD(c.has_d = true; c.p.dtype = 0; c.d.lut_log2 = 7);
    OK(c.has_y = true; c.p.dtype = 0);
    BAD(c.has_y = true; c.p.dtype = 0; c.r.out_w = 41);
    BAD(c.has_y = true; c.p.dtype = 0; c.r.out_h = 29);
    BAD(c.has_y = true; c.p.dtype = 0; c.y.in_bits = 7);
    { // work_bytes against the scratch layout
        Call c = good();
        ResamplePlan P;
        CHECK(run(c, P) == nullptr);
        CHECK(P.ytab == 1024u && P.total == 1024u + 768u); // 40 * 24 = 960 -> 1024; 30 * 24 = 720 -> 768
        c.work_bytes = P.total;
        decide(c, 0);
        c.work_bytes = P.total - 1u;
        decide(c, 1);
    }
    { // the siblings keep turning algo 4 down
        Call c = good();
        RgbPlan R;
        const char *why = rgb_check(&c.p, nullptr, nullptr, c.col, 1, reinterpret_cast<const uint16_t *>(c.in), c.pitch, c.fstride, c.width,
                                    c.height, c.n, reinterpret_cast<const void *>(c.out), c.out_bytes, R);
        CHECK(why && std::strcmp(why, "unknown algo") == 0);
        mcraw_area a;
        std::memset(&a, 0, sizeof a);
        a.cw = 56, a.ch = 28, a.out_w = 10, a.out_h = 6;
        AreaPlan AP;
        why = area_check(&c.p, &a, nullptr, nullptr, c.col, 1, reinterpret_cast<const uint16_t *>(c.in), c.pitch, c.fstride, c.width, c.height,
                         c.n, reinterpret_cast<const void *>(c.work), c.work_bytes, reinterpret_cast<const void *>(c.out), c.out_bytes, AP);
        CHECK(why && std::strcmp(why, "p->algo must be MCRAW_RGB_AREA") == 0);
    }
    { // the faults that the two scaled entry points share come out of one sequence: the same text from both
        const auto both = [&](const char *text, auto bend) { // bend(call, is it the area call): the fault, nullptr: none
            Call c[2] = {good(), good()};
            const char *why[2];
            for (int area = 0; area < 2; area++) {
                Call &k = c[area];
                k.p.algo = area ? MCRAW_RGB_AREA : MCRAW_RGB_RESAMPLE;
                k.width = k.height = 16, k.pitch = 16, k.fstride = 256, k.n = 1;
                k.r.x0 = k.r.y0 = 0, k.r.cw = k.r.ch = 16, k.r.out_w = k.r.out_h = 8;
                bend(k, area != 0);
            }
            ResamplePlan RP;
            why[0] = run(c[0], RP);
            const Call &k = c[1];
            mcraw_area a;
            std::memset(&a, 0, sizeof a);
            a.x0 = k.r.x0, a.y0 = k.r.y0, a.cw = k.r.cw, a.ch = k.r.ch, a.out_w = k.r.out_w, a.out_h = k.r.out_h;
            AreaPlan AP;
            why[1] = area_check(k.has_p ? &k.p : nullptr, k.has_r ? &a : nullptr, k.has_d ? &k.d : nullptr, k.has_y ? &k.y : nullptr, k.col,
                                k.ncolors, reinterpret_cast<const uint16_t *>(k.in), k.pitch, k.fstride, k.width, k.height, k.n,
                                reinterpret_cast<const void *>(k.work), k.work_bytes, reinterpret_cast<const void *>(k.out), k.out_bytes, AP);
            if (!text)
                CHECK(!why[0] && !why[1] && !RP.rgb.noop && !AP.rgb.noop);
            else
                CHECK(why[0] && why[1] && std::strcmp(why[0], why[1]) == 0 && std::strcmp(why[0], text) == 0);
        };
        both(nullptr, [](Call &, bool) {});
        both(nullptr, [](Call &k, bool) { k.has_y = true, k.p.dtype = 0; });
        both("bad arguments", [](Call &k, bool) { k.has_p = false; });
        both("a display stage and a YUV stage at once", [](Call &k, bool) { k.has_d = k.has_y = true, k.p.dtype = 0; });
        both("x0, y0, cw and ch must be even", [](Call &k, bool) { k.r.x0 = 1; });
        both("the crop must be 2 .. 65536 wide and high", [](Call &k, bool) { k.r.cw = 0; });
        both("the crop leaves the frame: x0 + cw > width or y0 + ch > height", [](Call &k, bool) { k.r.x0 = 2; });
        // (an odd out_w inside either's ratio rule: at most the crop's 8 quads for area, at least half the crop's 16 samples here)
        both("4:2:0 needs an even out_h and out_w", [](Call &k, bool area) { k.has_y = true, k.p.dtype = 0, k.r.out_w = area ? 7 : 9; });
        both("work missing or not 16-byte aligned", [](Call &k, bool) { k.work = 0; });
        both("work missing or not 16-byte aligned", [](Call &k, bool) { k.work += 8; });
    }

    // seeded tuples of geometry, family and pointers
    std::mt19937 rng(20261019u);
    const auto U = [&](uint32_t lo, uint32_t hi) { return lo + static_cast<uint32_t>(rng() % (hi - lo + 1u)); };
    for (int it = 0; it < 4000; it++) {
        Call c = good();
        c.width = static_cast<int>(2u * U(4, 200)), c.height = static_cast<int>(2u * U(4, 60));
        c.pitch = static_cast<size_t>(c.width) + 2u * U(0, 3), c.fstride = c.pitch * static_cast<size_t>(c.height);
        c.n = static_cast<int>(U(1, 3));
        c.r.cw = 2u * U(1, static_cast<uint32_t>(c.width) / 2u), c.r.ch = 2u * U(1, static_cast<uint32_t>(c.height) / 2u);
        c.r.x0 = 2u * U(0, (static_cast<uint32_t>(c.width) - c.r.cw) / 2u), c.r.y0 = 2u * U(0, (static_cast<uint32_t>(c.height) - c.r.ch) / 2u);
        c.r.out_w = U((c.r.cw + 1u) / 2u, 2u * c.r.cw), c.r.out_h = U((c.r.ch + 1u) / 2u, 2u * c.r.ch);
        c.r.filter = U(0, 1);
        const uint32_t fam = U(0, 2);
        c.has_d = fam == 1u, c.has_y = fam == 2u;
        if (fam)
            c.p.dtype = 0;
        switch (U(0, 9)) { // most tuples carry one defect
        case 0: c.r.out_w = c.r.cw / 2u - (c.r.cw >= 4u ? 1u : 0u); break;
        case 1: c.r.out_h = 2u * c.r.ch + 1u; break;
        case 2: c.r.x0 += static_cast<uint32_t>(c.width); break;
        case 3: c.r.cw += 1u; break;
        case 4: c.work += 4u * U(0, 3); break;
        case 5: c.out_bytes = U(0, 4000); break;
        case 6: c.r.reserved = U(0, 1); break;
        default: break;
        }
        decide(c, expect_geometry(c));
    }
    std::printf("accepted %ld rejected %ld\ncases %ld\nwrong %ld\n", accepted, rejected, cases, wrong);
    return wrong ? 1 : 0;
}
