// The host side of the highlight stage (csrc/mcraw_highlights_args.h) without HIP: inv, m and cap at the extreme gains, the
// overflow bounds that the contract in include/mcraw_hip.h claims, the green positions, and every check on the struct, the sizes
// and the records.  Built by tests/test_highlights_args.py under ASan and UBSan; prints "checks <n>" and "wrong <n>".
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mcraw_highlights_args.h"

using namespace mcraw;

static long checks = 0, wrong = 0;

#define EXPECT(cond)                                                                                                   \
    do {                                                                                                               \
        checks++;                                                                                                      \
        if (!(cond)) {                                                                                                 \
            wrong++;                                                                                                   \
            std::printf("line %d: %s\n", __LINE__, #cond);                                                             \
        }                                                                                                              \
    } while (0)

static mcraw_highlights good(void *rec, uint32_t nrec)
{
    mcraw_highlights h;
    std::memset(&h, 0, sizeof h);
    h.mode = MCRAW_HL_REBUILD;
    h.cfa = MCRAW_CFA_RGGB;
    h.top = 65535u;
    const uint16_t gain[4] = {8192, 4096, 4096, 6554};
    for (int p = 0; p < 4; p++) {
        h.black[p] = 64;
        h.sat[p] = 4095;
        h.gain[p] = gain[p];
        h.lo[p] = 2079;
    }
    h.rec = rec;
    h.nrec = nrec;
    return h;
}

static bool says(const char *why, const char *part)
{
    return why && std::strstr(why, part);
}

int main()
{
    static_assert(sizeof(mcraw_highlights) == 64, "struct mcraw_highlights");
    static_assert(offsetof(mcraw_highlights, black) == 16 && offsetof(mcraw_highlights, sat) == 24 && offsetof(mcraw_highlights, gain) == 32 &&
                      offsetof(mcraw_highlights, lo) == 40 && offsetof(mcraw_highlights, rec) == 48 && offsetof(mcraw_highlights, nrec) == 56 &&
                      offsetof(mcraw_highlights, reserved) == 60,
                  "struct mcraw_highlights");

    // inv at the ends of the gain's range and around 1.0
    EXPECT(hl_inv(256u) == 65536u);
    EXPECT(hl_inv(65535u) == 256u);
    EXPECT(hl_inv(4096u) == 4096u);
    EXPECT(hl_inv(8192u) == 2048u);
    for (uint32_t g = 256u; g <= 65535u; g++) { // rounded to nearest: |inv * g - 2^24| <= g / 2, and 256 .. 65536
        const int64_t e = static_cast<int64_t>(hl_inv(g)) * g - (1 << 24);
        if (e > g / 2 || -e > g / 2 || hl_inv(g) < 256u || hl_inv(g) > 65536u)
            wrong++;
    }
    checks++;

    // the bounds the contract claims: d * gain + 2048 < 2^32, v < 2^20, and the largest product of the way back
    EXPECT(65535ull * 65535ull + 2048ull < (1ull << 32));
    EXPECT(hl_wb(65535u, 0u, 65535u) == 1048544u && hl_wb(65535u, 0u, 65535u) < (1u << 20));
    EXPECT(hl_wb(0u, 65535u, 65535u) == 0u && hl_wb(100u, 100u, 65535u) == 0u);
    EXPECT(hl_wb(4095u, 64u, 8192u) == 8062u && hl_wb(4095u, 64u, 6554u) == 6450u);
    const uint32_t candmax = (1u << 20) + static_cast<uint32_t>(HL_CHROMA_MAX); // ref < 2^20, chroma <= 2^20
    EXPECT(candmax <= (1u << 21));
    EXPECT(static_cast<uint64_t>(candmax) * 65536u + 2048u < (1ull << 38));
    EXPECT(hl_back(candmax, 65535u, 65536u) == 65535u + (1u << 25)); // fits uint32 with room to spare; min(.., top) follows
    EXPECT(hl_back(7256u, 64u, 4096u) == 7320u);

    // m and cap: the example of the header, then the extreme gains with sat = 65535
    {
        const mcraw_highlights h = good(nullptr, 0);
        const HlDerived d = hl_derive(h);
        EXPECT(d.m == 4031u);
        EXPECT(d.cap[0] == 2080u && d.cap[1] == 4095u && d.cap[2] == 4095u && d.cap[3] == 2583u);
        EXPECT(d.inv[0] == 2048u && d.inv[1] == 4096u && d.inv[3] == 2560u);
    }
    {
        mcraw_highlights h = good(nullptr, 0);
        for (int p = 0; p < 4; p++) {
            h.black[p] = 0;
            h.sat[p] = 65535;
            h.gain[p] = (p & 1) ? 65535 : 256;
        }
        const HlDerived d = hl_derive(h);
        EXPECT(d.inv[0] == 65536u && d.inv[1] == 256u);
        EXPECT(d.m == 4096u); // (65535 * 256 + 2048) >> 12: the low gain's clip level
        EXPECT(d.cap[0] == 65536u); // above every sample: min(s, cap) changes nothing, and the kernel packs min(cap, 65535)
        EXPECT(d.cap[1] == 256u);   // (4096 * 256 + 2048) >> 12
        for (int p = 0; p < 4; p++)
            h.gain[p] = 65535;
        const HlDerived e = hl_derive(h);
        EXPECT(e.m == 1048544u && e.cap[0] == 65534u && e.cap[3] == 65534u); // floor(1048544 * 256 / 4096 + 0.5) = floor(65534.5): one below sat
        for (int p = 0; p < 4; p++)
            h.gain[p] = 256;
        const HlDerived f = hl_derive(h);
        EXPECT(f.m == 4096u && f.cap[0] == 65536u && f.cap[2] == 65536u);
    }

    // green positions
    for (uint32_t cfa = 0; cfa < 4u; cfa++)
        for (uint32_t p = 0; p < 4u; p++)
            EXPECT(hl_green(cfa, p) == (cfa < 2u ? (p == 1u || p == 2u) : (p == 0u || p == 3u)));

    // the struct's checks
    alignas(64) static unsigned char mem[1 << 16];
    void *rec = mem + 4096;
    {
        EXPECT(hl_check(good(nullptr, 0), 3, false) == nullptr);
        EXPECT(hl_check(good(rec, 1), 3, false) == nullptr);
        EXPECT(hl_check(good(rec, 3), 3, false) == nullptr);
        EXPECT(hl_check(good(rec, 1), 3, true) == nullptr);
        EXPECT(hl_check(good(rec, 3), 3, true) == nullptr);
        EXPECT(hl_check(good(rec, 1), 1, true) == nullptr);
        mcraw_highlights h = good(rec, 3);
        h.mode = MCRAW_HL_CLIP, h.flags = MCRAW_HL_ACCUMULATE;
        EXPECT(hl_check(h, 3, false) == nullptr && hl_check(h, 3, true) == nullptr);
        h = good(rec, 3), h.mode = 2;
        EXPECT(says(hl_check(h, 3, false), "mode"));
        h = good(rec, 3), h.cfa = 4;
        EXPECT(says(hl_check(h, 3, false), "cfa"));
        h = good(rec, 3), h.flags = 2;
        EXPECT(says(hl_check(h, 3, true), "flag"));
        h = good(rec, 3), h.flags = 1u | 0x80000000u;
        EXPECT(says(hl_check(h, 3, true), "flag"));
        h = good(rec, 3), h.top = 0;
        EXPECT(says(hl_check(h, 3, false), "top"));
        h = good(rec, 3), h.top = 65536;
        EXPECT(says(hl_check(h, 3, false), "top"));
        for (int p = 0; p < 4; p++) {
            h = good(rec, 3), h.gain[p] = 255;
            EXPECT(says(hl_check(h, 3, false), "gain"));
            h = good(rec, 3), h.gain[p] = 256;
            EXPECT(hl_check(h, 3, false) == nullptr);
            h = good(rec, 3), h.sat[p] = h.black[p];
            EXPECT(says(hl_check(h, 3, false), "sat"));
            h = good(rec, 3), h.sat[p] = static_cast<uint16_t>(h.black[p] - 1);
            EXPECT(says(hl_check(h, 3, true), "sat"));
            h = good(rec, 3), h.sat[p] = static_cast<uint16_t>(h.black[p] + 1);
            EXPECT(hl_check(h, 3, false) == nullptr);
        }
        EXPECT(says(hl_check(good(rec, 2), 3, false), "nrec"));
        EXPECT(says(hl_check(good(rec, 4), 3, false), "nrec"));
        EXPECT(says(hl_check(good(nullptr, 0), 3, true), "nrec")); // measure writes records: there must be some
        EXPECT(says(hl_check(good(rec, 2), 3, true), "nrec"));
        EXPECT(says(hl_check(good(nullptr, 1), 3, false), "rec"));
        EXPECT(says(hl_check(good(nullptr, 3), 3, true), "rec"));
        EXPECT(says(hl_check(good(rec, 0), 3, false), "rec"));
        for (int off = 1; off < 8; off++)
            EXPECT(says(hl_check(good(mem + 4096 + off, 1), 3, false), "aligned"));
        h = good(rec, 3), h.reserved = 1;
        EXPECT(says(hl_check(h, 3, false), "reserved"));
    }

    // the sizes: 2 .. 65536, and what MosaicBatch asks
    {
        const uint16_t *in = reinterpret_cast<const uint16_t *>(mem + 8192), *out = reinterpret_cast<const uint16_t *>(mem + 16384);
        const int sizes[] = {-4, 0, 1, 2, 3, 65536, 65537};
        for (int w : sizes)
            for (int hh : sizes) {
                const MosaicBatch I(in, 70000, 0, 1, w, hh), O(out, 70000, 0, 1, w, hh);
                const bool ok = w >= 2 && w <= 65536 && hh >= 2 && hh <= 65536;
                EXPECT((hl_check_batches(I, &O) == nullptr) == ok);
                EXPECT((hl_check_batches(I, nullptr) == nullptr) == ok);
                if (!ok)
                    EXPECT(says(hl_check_batches(I, &O), "2 .. 65536"));
            }
        const MosaicBatch I(in, 24, 240, 2, 24, 10), O(out, 24, 240, 2, 24, 10);
        EXPECT(hl_check_batches(I, &O) == nullptr);
        EXPECT(says(hl_check_batches(MosaicBatch(nullptr, 24, 240, 2, 24, 10), &O), "missing"));
        EXPECT(hl_check_batches(I, nullptr) == nullptr);
        EXPECT(says(hl_check_batches(MosaicBatch(mem + 8193, 24, 240, 2, 24, 10), &O), "aligned"));
        const MosaicBatch Oodd(mem + 16385, 24, 240, 2, 24, 10);
        EXPECT(says(hl_check_batches(I, &Oodd), "aligned"));
        EXPECT(says(hl_check_batches(MosaicBatch(in, 23, 240, 2, 24, 10), &O), "pitch"));
        const MosaicBatch Opitch(out, 23, 240, 2, 24, 10), Ostride(out, 24, 239, 2, 24, 10);
        EXPECT(says(hl_check_batches(I, &Opitch), "pitch"));
        EXPECT(says(hl_check_batches(MosaicBatch(in, 24, 239, 2, 24, 10), &O), "stride"));
        EXPECT(says(hl_check_batches(I, &Ostride), "stride"));
        EXPECT(hl_check_batches(MosaicBatch(in, 24, 0, 1, 24, 10), nullptr) == nullptr); // one frame: the stride means nothing

        // records against the extents: I covers bytes [8192, 8192 + 960), records are 64 bytes each
        EXPECT(I.bytes() == 960u);
        EXPECT(!hl_rec_overlaps(good(nullptr, 0), I));
        EXPECT(!hl_rec_overlaps(good(mem + 8192 - 64, 1), I));
        EXPECT(hl_rec_overlaps(good(mem + 8192 - 64, 2), I));
        EXPECT(hl_rec_overlaps(good(mem + 8192 - 56, 1), I));
        EXPECT(hl_rec_overlaps(good(mem + 8192 + 952, 1), I));
        EXPECT(!hl_rec_overlaps(good(mem + 8192 + 960, 2), I));
        EXPECT(hl_rec_overlaps(good(mem + 8192 + 64, 1), I));
        EXPECT(overlap(I, MosaicBatch(mem + 8192 + 958, 24, 240, 2, 24, 10)) && !overlap(I, MosaicBatch(mem + 8192 + 960, 24, 240, 2, 24, 10)));
    }

    std::printf("checks %ld\nwrong %ld\n", checks, wrong);
    return wrong ? 1 : 0;
}
