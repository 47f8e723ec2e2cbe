// The host side of the noise measurement (csrc/mcraw_noise_args.h) without HIP: the struct's layout and checks, the two bin
// formulas at every edge, every index into the record (and into the kernel's LDS copy of it), and the launch plan: strips,
// workgroups, rounds, halves and lanes cover every whole block of the window exactly once and nothing outside it.
// Built by tests/test_noise_args.py under ASan and UBSan; prints "checks <n>" and "wrong <n>".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "mcraw_noise_args.h"

using namespace mcraw;

static long checks = 0, wrong = 0;

#define EXPECT(cond)                                                                                                   \
    do {                                                                                                               \
        checks++;                                                                                                      \
        if (!(cond)) {                                                                                                 \
            wrong++;                                                                                                   \
            if (wrong < 50)                                                                                            \
                std::printf("line %d: %s\n", __LINE__, #cond);                                                         \
        }                                                                                                              \
    } while (0)

static mcraw_noise good()
{
    mcraw_noise s;
    std::memset(&s, 0, sizeof s);
    s.shift = 7;
    s.x0 = 2, s.y0 = 4, s.w = 64, s.h = 32;
    for (int p = 0; p < 4; p++)
        s.sat[p] = 4095, s.lo[p] = 1;
    return s;
}

static bool says(const char *why, const char *part)
{
    return why && std::strstr(why, part);
}

// Every (block, row parity) of a w x h window exactly once, by the walk the kernel makes; no lane outside the window.
static void cover(uint32_t w, uint32_t h, uint32_t frames, uint32_t maxstrips)
{
    const NoisePlan P = noise_plan(w, h, frames, maxstrips);
    bool ok = P.bx == w / 16u && P.by == h / 16u && P.stripsX == (P.bx + 63u) / 64u && P.strips == P.stripsX * P.by;
    ok = ok && P.spw >= 1u && P.spw <= maxstrips && P.spw <= P.strips && P.wgs == (P.strips + P.spw - 1u) / P.spw;
    ok = ok && static_cast<uint64_t>(P.wgs) * P.spw >= P.strips && static_cast<uint64_t>(P.wgs - 1u) * P.spw < P.strips;
    ok = ok && (P.spw >= NS_MINSTRIPS || P.spw == maxstrips || P.spw == P.strips);
    std::vector<uint8_t> seen(static_cast<size_t>(P.bx) * P.by * 2u, 0);
    for (uint32_t wg = 0; wg < P.wgs && ok; wg++) {
        const uint32_t t0 = wg * P.spw, t1 = t0 + P.spw < P.strips ? t0 + P.spw : P.strips;
        for (uint32_t i = 0; noise_strip(wg, P.spw, i, 0u) < t1; i++)
            for (uint32_t half = 0; half < NS_HALVES; half++) {
                const uint32_t t = noise_strip(wg, P.spw, i, half);
                if (t >= t1)
                    continue;
                for (uint32_t lane = 0; lane < NS_SL; lane++) {
                    const NoiseLane L = noise_lane(P.bx, P.stripsX, t, lane);
                    if (!L.active)
                        continue;
                    ok = ok && L.rp == lane / 64u && L.x % 16u == 0u && L.x + 16u <= w && L.y % 16u == L.rp && L.y + 14u < h;
                    if (!ok)
                        break;
                    seen[(static_cast<size_t>(L.y / 16u) * P.bx + L.x / 16u) * 2u + L.rp]++;
                }
            }
    }
    for (uint8_t v : seen)
        ok = ok && v == 1u;
    EXPECT(ok);
    if (!ok && wrong < 50)
        std::printf("  cover(%u, %u, %u, %u)\n", w, h, frames, maxstrips);
}

int main()
{
    static_assert(sizeof(mcraw_noise) == 44, "struct mcraw_noise");
    static_assert(offsetof(mcraw_noise, x0) == 4 && offsetof(mcraw_noise, y0) == 8 && offsetof(mcraw_noise, w) == 12 &&
                      offsetof(mcraw_noise, h) == 16 && offsetof(mcraw_noise, sat) == 20 && offsetof(mcraw_noise, lo) == 28 &&
                      offsetof(mcraw_noise, flags) == 36 && offsetof(mcraw_noise, reserved) == 40,
                  "struct mcraw_noise");
    static_assert(NS_REC_BYTES == 65568u && NS_HIST == 16384u && NS_SL == 128u && NS_HALVES == 2u, "the record and the workgroup");

    // the energy bin: below 16, and both sides of every edge 2^e * (1 + f / 4)
    EXPECT(noise_energy_bin(0u) == 0u && noise_energy_bin(15u) == 0u && noise_energy_bin(16u) == 1u);
    for (uint32_t e = 4; e <= 62u; e++)
        for (uint32_t f = 0; f < 4u; f++) {
            const uint64_t edge = (1ull << e) + f * (1ull << (e - 2u));
            const uint32_t vb = 4u * (e - 4u) + f + 1u;
            EXPECT(noise_energy_bin(edge) == (vb < 127u ? vb : 127u));
            EXPECT(noise_energy_bin(edge - 1u) == (vb - 1u < 127u ? vb - 1u : 127u));
        }
    EXPECT(noise_energy_bin(96ull * 131070ull * 131070ull) == 127u && 96ull * 131070ull * 131070ull < (1ull << 43));
    EXPECT(noise_energy_bin(~0ull) == 127u);
    EXPECT(noise_energy_bin((1ull << 35) + (1ull << 34) - 1u) == 126u && noise_energy_bin((1ull << 35) + (1ull << 34)) == 127u);

    // the level bin and its clamp
    EXPECT(noise_level_bin(0u, 0u) == 0u && noise_level_bin(63u, 0u) == 0u && noise_level_bin(64u, 0u) == 1u);
    EXPECT(noise_level_bin(64u * 31u, 0u) == 31u && noise_level_bin(64u * 32u, 0u) == 31u && noise_level_bin(64u * 65535u, 0u) == 31u);
    EXPECT(noise_level_bin(64u * 4095u, 7u) == 31u && noise_level_bin(64u * 3967u, 7u) == 30u && noise_level_bin(64u * 65535u, 11u) == 31u);
    EXPECT(noise_level_bin(64u * 65535u, 15u) == 1u && noise_level_bin(64u * 32767u + 63u, 15u) == 0u);

    // every counter's index: the record's order, inside the 16384 counters, for every bin the two formulas can give
    {
        uint32_t next = 0;
        for (uint32_t p = 0; p < 4u; p++)
            for (uint32_t l = 0; l < NS_L; l++)
                for (uint32_t vb = 0; vb < NS_V; vb++)
                    EXPECT(noise_hist_index(p, l, vb) == next++);
        EXPECT(next == NS_HIST);
        bool in = true;
        for (uint32_t shift = 0; shift <= 15u; shift++)
            for (uint32_t s = 0; s <= 64u * 65535u; s += 4093u)
                for (uint32_t e = 0; e < 64u; e++)
                    in = in && noise_hist_index(3u, noise_level_bin(s, shift), noise_energy_bin((1ull << e) - 1u)) < NS_HIST;
        EXPECT(in);
    }

    // the struct's checks on a 100 x 60 frame
    {
        mcraw_noise s = good();
        EXPECT(noise_check(s, 100, 60) == nullptr);
        s = good(), s.shift = 15;
        EXPECT(noise_check(s, 100, 60) == nullptr);
        s = good(), s.shift = 16;
        EXPECT(says(noise_check(s, 100, 60), "shift"));
        s = good(), s.x0 = 3;
        EXPECT(says(noise_check(s, 100, 60), "even"));
        s = good(), s.y0 = 5;
        EXPECT(says(noise_check(s, 100, 60), "even"));
        s = good(), s.w = 15;
        EXPECT(says(noise_check(s, 100, 60), "at least 16"));
        s = good(), s.h = 15;
        EXPECT(says(noise_check(s, 100, 60), "at least 16"));
        s = good(), s.w = 16, s.h = 16;
        EXPECT(noise_check(s, 100, 60) == nullptr);
        s = good(), s.w = 98;
        EXPECT(noise_check(s, 100, 60) == nullptr);
        s = good(), s.w = 99;
        EXPECT(says(noise_check(s, 100, 60), "leaves"));
        s = good(), s.h = 56;
        EXPECT(noise_check(s, 100, 60) == nullptr);
        s = good(), s.h = 57;
        EXPECT(says(noise_check(s, 100, 60), "leaves"));
        s = good(), s.x0 = 100;
        EXPECT(says(noise_check(s, 100, 60), "leaves"));
        s = good(), s.x0 = 0xFFFFFFF0u, s.w = 32; // x0 + w wraps to 16
        EXPECT(says(noise_check(s, 100, 60), "leaves"));
        s = good(), s.y0 = 0xFFFFFFF0u, s.h = 32;
        EXPECT(says(noise_check(s, 100, 60), "leaves"));
        s = good(), s.w = 0xFFFFFFFFu;
        EXPECT(says(noise_check(s, 100, 60), "leaves"));
        s = good(), s.flags = MCRAW_NOISE_ACCUMULATE;
        EXPECT(noise_check(s, 100, 60) == nullptr);
        s = good(), s.flags = 2;
        EXPECT(says(noise_check(s, 100, 60), "flag"));
        s = good(), s.flags = 1u | 0x80000000u;
        EXPECT(says(noise_check(s, 100, 60), "flag"));
        s = good(), s.reserved = 1;
        EXPECT(says(noise_check(s, 100, 60), "reserved"));
        s = good(), s.x0 = 0, s.y0 = 0, s.w = 65536, s.h = 65536;
        EXPECT(noise_check(s, 65536, 65536) == nullptr);
        const NoisePlan P = noise_plan(65536, 65536, 1, 0x7FFFFFFFu); // the largest frame: 2^24 blocks
        EXPECT(P.bx == 4096u && P.by == 4096u && P.strips == 64u * 4096u && P.wgs == 1024u && P.spw == 256u);
    }

    // the plan: every width at the smallest and the largest height, every height at the widths about a strip's end
    const uint32_t widths[] = {16, 17, 31, 32, 1023, 1024, 1039, 1040, 2047, 2048, 2064, 4111, 4112};
    const uint32_t frames[] = {1, 35, 2000}, caps[] = {1, 3, 0x7FFFFFFFu};
    for (uint32_t f : frames)
        for (uint32_t cap : caps) {
            for (uint32_t w = 16; w <= 4112u; w++) {
                cover(w, 16, f, cap);
                cover(w, 80, f, cap);
            }
            for (uint32_t h = 16; h <= 80u; h++)
                for (uint32_t w : widths)
                    cover(w, h, f, cap);
        }
    // a UHD frame among 240, as the benchmark runs it, and one alone
    {
        const NoisePlan P = noise_plan(3840, 2160, 240, 0x7FFFFFFFu);
        EXPECT(P.stripsX == 4u && P.strips == 540u && P.spw == 135u && P.wgs == 4u);
        const NoisePlan Q = noise_plan(3840, 2160, 1, 0x7FFFFFFFu);
        EXPECT(Q.spw == 16u && Q.wgs == 34u);
        cover(3840, 2160, 240, 0x7FFFFFFFu);
        cover(3840, 2160, 1, 0x7FFFFFFFu);
    }

    std::printf("checks %ld\nwrong %ld\n", checks, wrong);
    return wrong ? 1 : 0;
}
