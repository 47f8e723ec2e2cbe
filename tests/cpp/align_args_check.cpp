// align_args_check.cpp -- csrc/mcraw_align_args.h on its own (no HIP: that this file compiles with a plain g++ is part of the
// test): what mcraw_align_batch decides with it about a call -- accept or reject, the planes and bounds of the levels, where the
// three sections of the scratch lie -- against a transcription of the contract in include/mcraw_hip.h written without the
// header's helpers.  Addresses are numbers; nothing is read through them.  Prints "accepted A rejected R", "cases N" and
// "wrong N"; every failed check says where.  tests/test_align_args.py builds and runs it.
#include "mcraw_align_args.h"

#include <cstdio>
#include <random>

using namespace mcraw;

struct Call {
    int w, h;
    size_t n;
    unsigned levels, radius;
    uintptr_t in, pos, sad, work;
    size_t pitch, fstride, work_bytes;
};

static bool meet(uintptr_t a, size_t na, uintptr_t b, size_t nb)
{
    for (int k = 0; k < 2; k++) { // either range holds the other's first byte
        if (na && nb && a <= b && b - a < na)
            return true;
        std::swap(a, b), std::swap(na, nb);
    }
    return false;
}

// The contract, step by step: 0 accepted, -1 rejected.  need: the least the scratch has to hold (planes with rows of whole
// 16-byte pieces, 64-bit sums, winners), without the sections' padding.
static int contract(const Call &c, unsigned hh[6], unsigned ww[6], unsigned B[6], size_t *need)
{
    if (c.levels < 1 || c.levels > 6 || c.radius < 1 || c.radius > 8 || c.w < 1 || c.h < 1 || c.w > 65536 || c.h > 65536)
        return -1;
    unsigned h = c.h / 2, w = c.w / 2;
    size_t planes = 0;
    for (unsigned l = 0; l < c.levels; l++, h /= 2, w /= 2) {
        hh[l] = h, ww[l] = w;
        planes += static_cast<size_t>(h) * ((w + 7) / 8 * 8) * 2;
    }
    unsigned b = c.radius;
    for (int l = static_cast<int>(c.levels) - 1; l >= 0; l--, b = 2 * b + 1)
        B[l] = b;
    for (unsigned l = 0; l < c.levels; l++)
        if (static_cast<long>(hh[l]) - 2l * B[l] < 1 || static_cast<long>(ww[l]) - 2l * B[l] < 1)
            return -1;
    *need = c.n * (planes + 8 * ((2 * c.radius + 1) * (2 * c.radius + 1) + 9 * (c.levels - 1)) + 16 * c.levels);
    return 0;
}

static int wrong = 0;
#define CHECK(cond, c)                                                                                                               \
    do {                                                                                                                             \
        if (!(cond)) {                                                                                                               \
            wrong++;                                                                                                                 \
            std::printf("line %d: %s (w %d h %d n %zu levels %u radius %u)\n", __LINE__, #cond, (c).w, (c).h, (c).n, (c).levels, (c).radius); \
        }                                                                                                                            \
    } while (0)

int main()
{
    std::mt19937_64 rng(23);
    const int sizes[] = {1, 2, 5, 6, 7, 9, 24, 40, 72, 136, 260, 520, 1030, 2160, 3840, 65536, 65537, 0, -4};
    long cases = 0, acc = 0, rej = 0;
    for (int it = 0; it < 200000; it++) {
        Call c{};
        c.w = sizes[rng() % 19], c.h = sizes[rng() % 19];
        if (rng() % 4 == 0)
            c.w = 1 + static_cast<int>(rng() % 5000), c.h = 1 + static_cast<int>(rng() % 5000);
        c.n = 1 + rng() % (rng() % 8 ? 6 : 3000);
        c.levels = static_cast<unsigned>(rng() % 8), c.radius = static_cast<unsigned>(rng() % 10);
        if (rng() % 3)
            c.levels = 1 + c.levels % 4, c.radius = 1 + c.radius % 4;
        AlignPlan P;
        const char *why = P.make(c.w, c.h, c.n, c.levels, c.radius);
        unsigned hh[6] = {}, ww[6] = {}, B[6] = {};
        size_t need = 0;
        const int rc = contract(c, hh, ww, B, &need);
        cases++;
        CHECK((why != nullptr) == (rc != 0), c);
        if (why || rc) {
            rej++;
            continue;
        }
        for (unsigned l = 0; l < c.levels; l++) {
            CHECK(P.h[l] == hh[l] && P.w[l] == ww[l] && P.B[l] == B[l], c);
            CHECK(P.pitch[l] >= P.w[l] && P.pitch[l] % 8 == 0 && P.pitch[l] < P.w[l] + 8, c);
            CHECK(P.off[l] % 8 == 0 && P.off[l] + static_cast<size_t>(P.h[l]) * P.pitch[l] <= (l + 1 < c.levels ? P.off[l + 1] : P.frame_elems), c);
            CHECK(P.acc0[l] + (l + 1 == c.levels ? AlignPlan::cands(c.radius) : 9u) <= P.nacc, c);
            CHECK(l + 1 == c.levels ? P.acc0[l] == 0 : P.acc0[l] == P.acc0[l + 1] + (l + 2 == c.levels ? AlignPlan::cands(c.radius) : 9u), c);
        }
        // the sections follow one another inside `total`, each aligned, none cut short
        CHECK(P.pyr == 0 && P.acc % AL_SECTION == 0 && P.win % AL_SECTION == 0 && P.total % AL_SECTION == 0, c);
        CHECK(P.acc >= c.n * P.frame_elems * 2 && P.win >= P.acc + c.n * P.nacc * 8 && P.total >= P.win + c.n * 6 * sizeof(AlignWin), c);
        CHECK(P.total >= need && P.total <= need + c.n * (6 - c.levels) * 16 + 3 * AL_SECTION, c);
        // the pointers: a layout that is fine, then one defect at a time
        const uintptr_t base = 0x10000000u;
        const size_t pitch = static_cast<size_t>(c.w) + rng() % 3, fstride = static_cast<size_t>(c.h) * pitch + rng() % 9;
        const MosaicBatch I(reinterpret_cast<const void *>(base), pitch, fstride, c.n, c.w, c.h);
        CHECK(I.check() == nullptr, c);
        const uintptr_t after = (base + I.bytes() + 255) / 256 * 256;
        c.pos = after, c.sad = after + (c.n * 4 + 7) / 8 * 8, c.work = (c.sad + c.n * 8 + 15) / 16 * 16, c.work_bytes = P.total;
        const unsigned defect = static_cast<unsigned>(rng() % 14);
        bool bad = false;
        switch (defect) {
        case 1: c.pos = 0, bad = true; break;
        case 2: c.work = 0, bad = true; break;
        case 3: c.pos += 1, bad = true; break;
        case 4: c.sad += 4, bad = true; break;
        case 5: c.work += 8, bad = true; break;
        case 6: c.work_bytes -= 1, bad = true; break;
        case 7: c.pos = base + 2 * (rng() % I.extent()), bad = true; break;
        case 8: c.sad = (base + I.bytes() - 1) / 8 * 8, bad = true; break;
        case 9: c.work = base / 16 * 16 + 16 * (rng() % ((I.bytes() + 15) / 16)), bad = true; break;
        case 10: c.pos = c.work + 2 * (rng() % (P.total / 2)), bad = true; break;
        case 11: c.sad = c.work + 8 * (rng() % (P.total / 8)), bad = true; break;
        case 12: c.sad = c.pos + (c.n * 4 - 1) / 8 * 8, bad = true; break;
        case 13: c.sad = 0; break; // no sad: fine
        default: break;
        }
        const char *pw = check_align_ptrs(I, P, c.n, reinterpret_cast<const void *>(c.pos), reinterpret_cast<const void *>(c.sad),
                                          reinterpret_cast<const void *>(c.work), c.work_bytes);
        // the contract's list, by hand
        bool want = !c.pos || !c.work || (c.pos & 1) || (c.sad & 7) || (c.work & 15) || c.work_bytes < P.total;
        if (!want) {
            const size_t ns = c.sad ? c.n * 8 : 0;
            want = meet(base, I.bytes(), c.pos, c.n * 4) || meet(base, I.bytes(), c.sad, ns) || meet(base, I.bytes(), c.work, P.total) ||
                   meet(c.work, P.total, c.pos, c.n * 4) || meet(c.work, P.total, c.sad, ns) || meet(c.pos, c.n * 4, c.sad, ns);
        }
        cases++;
        CHECK((pw != nullptr) == want, c);
        CHECK(!bad || want, c); // (every defect above is one the contract names)
        (pw ? rej : acc)++;
    }
    std::printf("accepted %ld rejected %ld\ncases %ld\nwrong %d\n", acc, rej, cases, wrong);
    return wrong ? 1 : 0;
}
