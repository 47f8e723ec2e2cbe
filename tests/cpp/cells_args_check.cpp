// cells_args_check.cpp -- csrc/mcraw_cells_args.h on its own (no HIP: that this file compiles with a plain g++ is part of the
// test): what mcraw_align_cells_batch and mcraw_merge_cells_batch decide with it about a call -- accept or reject, the grid of
// cells, the planes of the levels, where the three sections of the scratch lie -- against a transcription of the contract in
// include/mcraw_hip.h written without the header's helpers.  Addresses are numbers; nothing is read through them.  Prints
// "accepted A rejected R", "cases N" and "wrong N"; every failed check says where.  tests/test_align_cells_abi.py builds and runs it.
#include "mcraw_cells_args.h"

#include <cstdio>
#include <random>

using namespace mcraw;

struct Call {
    int w, h;
    size_t n;
    unsigned levels, radius, ch, cw;
    uintptr_t pos, sad, gpos, work;
    size_t work_bytes;
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

// The contract, step by step: 0 accepted, -1 rejected.  need: the least the scratch has to hold (planes with rows of whole 16-byte
// pieces, 64-bit sums per cell, a winner per cell and level), without the sections' padding.
static int contract(const Call &c, unsigned hh[3], unsigned ww[3], unsigned *cy, unsigned *cx, size_t *need)
{
    if (c.levels < 1 || c.levels > 3 || c.radius < 1 || c.radius > 4 || c.w < 1 || c.h < 1 || c.w > 65536 || c.h > 65536)
        return -1;
    if (c.ch < 32 || c.ch % 32 || c.ch > 65536 || c.cw < 256 || c.cw % 256 || c.cw > 65536)
        return -1;
    *cy = (c.h + c.ch - 1) / c.ch, *cx = (c.w + c.cw - 1) / c.cw;
    size_t planes = 0;
    for (unsigned l = 0; l < c.levels; l++) {
        hh[l] = static_cast<unsigned>(c.h) >> (l + 1), ww[l] = static_cast<unsigned>(c.w) >> (l + 1);
        planes += static_cast<size_t>(hh[l]) * ((ww[l] + 7) / 8 * 8) * 2;
    }
    const size_t cells = static_cast<size_t>(*cy) * *cx;
    *need = c.n * (planes + cells * (8 * ((2 * c.radius + 1) * (2 * c.radius + 1) + 9 * (c.levels - 1)) + 16 * c.levels));
    return 0;
}

static int wrong = 0;
#define CHECK(cond, c)                                                                                                               \
    do {                                                                                                                             \
        if (!(cond)) {                                                                                                               \
            wrong++;                                                                                                                 \
            std::printf("line %d: %s (w %d h %d n %zu levels %u radius %u cell %u x %u)\n", __LINE__, #cond, (c).w, (c).h, (c).n, (c).levels, \
                        (c).radius, (c).ch, (c).cw);                                                                                 \
        }                                                                                                                            \
    } while (0)

int main()
{
    std::mt19937_64 rng(28);
    const int sizes[] = {1, 2, 8, 15, 16, 31, 32, 33, 100, 101, 130, 255, 256, 257, 600, 601, 1030, 2160, 3840, 65536, 65537, 0, -4};
    const unsigned chs[] = {32, 64, 96, 128, 2176, 65536, 0, 16, 48, 65568}, cws[] = {256, 512, 768, 3840, 65536, 0, 128, 384, 65792, 257};
    long cases = 0, acc = 0, rej = 0;
    for (int it = 0; it < 200000; it++) {
        Call c{};
        c.w = sizes[rng() % 23], c.h = sizes[rng() % 23];
        if (rng() % 4 == 0)
            c.w = 1 + static_cast<int>(rng() % 5000), c.h = 1 + static_cast<int>(rng() % 5000);
        c.n = 1 + rng() % (rng() % 8 ? 6 : 3000);
        c.levels = static_cast<unsigned>(rng() % 5), c.radius = static_cast<unsigned>(rng() % 6);
        c.ch = chs[rng() % 10], c.cw = cws[rng() % 10];
        if (rng() % 3)
            c.levels = 1 + c.levels % 3, c.radius = 1 + c.radius % 4, c.ch = chs[rng() % 6], c.cw = cws[rng() % 5];
        CellsPlan P;
        const char *why = P.make(c.w, c.h, c.n, c.levels, c.radius, c.ch, c.cw);
        unsigned hh[3] = {}, ww[3] = {}, cy = 0, cx = 0;
        size_t need = 0;
        const int rc = contract(c, hh, ww, &cy, &cx, &need);
        cases++;
        CHECK((why != nullptr) == (rc != 0), c);
        if (why || rc) {
            rej++;
            continue;
        }
        CHECK(P.G.cells_y == cy && P.G.cells_x == cx && P.G.cell_h == c.ch && P.G.cell_w == c.cw, c);
        CHECK(static_cast<size_t>(cy - 1) * c.ch < static_cast<size_t>(c.h) && static_cast<size_t>(cy) * c.ch >= static_cast<size_t>(c.h), c);
        CHECK(static_cast<size_t>(cx - 1) * c.cw < static_cast<size_t>(c.w) && static_cast<size_t>(cx) * c.cw >= static_cast<size_t>(c.w), c);
        for (unsigned l = 0; l < c.levels; l++) {
            CHECK(P.h[l] == hh[l] && P.w[l] == ww[l], c);
            CHECK(P.pitch[l] >= P.w[l] && P.pitch[l] % 8 == 0 && P.pitch[l] < P.w[l] + 8, c);
            CHECK(P.off[l] % 8 == 0 && P.off[l] + static_cast<size_t>(P.h[l]) * P.pitch[l] <= (l + 1 < c.levels ? P.off[l + 1] : P.frame_elems), c);
            CHECK(P.acc0[l] + (l + 1 == c.levels ? CellsPlan::cands(c.radius) : 9u) <= P.nacc, c);
            CHECK(l + 1 == c.levels ? P.acc0[l] == 0 : P.acc0[l] == P.acc0[l + 1] + (l + 2 == c.levels ? CellsPlan::cands(c.radius) : 9u), c);
            // a cell is whole pixels of the level, and the cells cover the plane
            CHECK((c.ch >> (l + 1)) << (l + 1) == c.ch && (c.cw >> (l + 1)) << (l + 1) == c.cw, c);
            CHECK(static_cast<size_t>(cy) * (c.ch >> (l + 1)) >= hh[l] && static_cast<size_t>(cx) * (c.cw >> (l + 1)) >= ww[l], c);
        }
        // the sections follow one another inside `total`, each aligned, none cut short, none overlapping another
        const size_t cells = static_cast<size_t>(cy) * cx;
        const size_t npyr = c.n * P.frame_elems * 2, nacc = c.n * cells * P.nacc * 8, nwin = c.n * cells * 3 * sizeof(CellWin);
        CHECK(P.pyr == 0 && P.acc % CL_SECTION == 0 && P.win % CL_SECTION == 0 && P.total % CL_SECTION == 0, c);
        CHECK(P.acc >= P.pyr + npyr && P.win >= P.acc + nacc && P.total >= P.win + nwin, c);
        CHECK(!meet(P.pyr, npyr, P.acc, nacc) && !meet(P.pyr, npyr, P.win, nwin) && !meet(P.acc, nacc, P.win, nwin), c);
        CHECK(P.total >= need && P.total <= need + c.n * cells * (3 - c.levels) * 16 + 3 * CL_SECTION, c);
        { // work_bytes grows with n, and a longer batch never needs less
            CellsPlan Q;
            CHECK(Q.make(c.w, c.h, c.n + 1, c.levels, c.radius, c.ch, c.cw) == nullptr && Q.total >= P.total, c);
            CellsPlan Q2;
            CHECK(Q2.make(c.w, c.h, 2 * c.n + 7, c.levels, c.radius, c.ch, c.cw) == nullptr && Q2.total > P.total, c);
        }
        // the pointers: a layout that is fine, then one defect at a time
        const uintptr_t base = 0x10000000u;
        const size_t pitch = static_cast<size_t>(c.w) + rng() % 3, fstride = static_cast<size_t>(c.h) * pitch + rng() % 9;
        const MosaicBatch I(reinterpret_cast<const void *>(base), pitch, fstride, c.n, c.w, c.h);
        CHECK(I.check() == nullptr, c);
        const size_t np = c.n * cells * 4, ns8 = c.n * cells * 8, ng = c.n * 4;
        const uintptr_t after = (base + I.bytes() + 255) / 256 * 256;
        c.gpos = after, c.pos = (c.gpos + ng + 7) / 8 * 8, c.sad = (c.pos + np + 7) / 8 * 8, c.work = (c.sad + ns8 + 15) / 16 * 16;
        c.work_bytes = P.total;
        const unsigned defect = static_cast<unsigned>(rng() % 20);
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
        case 12: c.sad = c.pos + (np - 1) / 8 * 8, bad = true; break;
        case 13: c.sad = 0; break;  // no sad: fine
        case 14: c.gpos = 0; break; // no gpos: fine
        case 15: c.gpos += 1, bad = true; break;
        case 16: c.gpos = c.pos + 2 * (rng() % (np / 2)), bad = true; break;
        case 17: c.gpos = c.work + 2 * (rng() % (P.total / 2)), bad = true; break;
        case 18: c.gpos = c.sad + 2 * (rng() % (ns8 / 2)), bad = true; break;
        case 19: c.gpos = base + 2 * (rng() % I.extent()); break; // gpos inside the input: both are only read
        default: break;
        }
        const char *pw = check_cells_ptrs(I, P, c.n, reinterpret_cast<const void *>(c.pos), reinterpret_cast<const void *>(c.sad),
                                          reinterpret_cast<const void *>(c.gpos), reinterpret_cast<const void *>(c.work), c.work_bytes);
        bool want = !c.pos || !c.work || (c.pos & 1) || (c.gpos & 1) || (c.sad & 7) || (c.work & 15) || c.work_bytes < P.total;
        if (!want) {
            const size_t ns = c.sad ? ns8 : 0, ngg = c.gpos ? ng : 0;
            want = meet(base, I.bytes(), c.pos, np) || meet(base, I.bytes(), c.sad, ns) || meet(base, I.bytes(), c.work, P.total) ||
                   meet(c.work, P.total, c.pos, np) || meet(c.work, P.total, c.sad, ns) || meet(c.pos, np, c.sad, ns) ||
                   meet(c.gpos, ngg, c.pos, np) || meet(c.gpos, ngg, c.sad, ns) || meet(c.gpos, ngg, c.work, P.total);
        }
        cases++;
        CHECK((pw != nullptr) == want, c);
        CHECK(!bad || want, c); // (every defect above is one the contract names)
        (pw ? rej : acc)++;
        // the merge's view of the same grid: the ceilings and nothing else, a field that is there, even, and off the output
        const MosaicBatch O(reinterpret_cast<const void *>(base), pitch, fstride, c.n, c.w, c.h);
        unsigned gy = cy, gx = cx, res = 0;
        uintptr_t f = after;
        const unsigned md = static_cast<unsigned>(rng() % 9);
        bool mbad = md >= 1 && md <= 7;
        switch (md) {
        case 1: gy += 1; break;
        case 2: gx -= 1; break;
        case 3: res = 1; break;
        case 4: f = 0; break;
        case 5: f += 1; break;
        case 6: f = base + 2 * (rng() % O.extent()); break;
        case 7: f = base - 2 * (1 + rng() % (np / 2 - 1)); break; // starts in front of the output and ends inside it
        default: break;
        }
        const char *mw = check_merge_cells(O, c.n, c.w, c.h, c.ch, c.cw, gy, gx, res, reinterpret_cast<const void *>(f));
        const bool mwant = gy != cy || gx != cx || res != 0 || !f || (f & 1) || meet(base, O.bytes(), f, np);
        cases++;
        CHECK((mw != nullptr) == mwant, c);
        CHECK(!mbad || mwant, c);
        CHECK(check_merge_cells(O, c.n, c.w, c.h, c.ch + 16, c.cw, gy, gx, 0, reinterpret_cast<const void *>(after)) != nullptr, c);
        CHECK(check_merge_cells(O, c.n, c.w, c.h, c.ch, c.cw + 128, gy, gx, 0, reinterpret_cast<const void *>(after)) != nullptr, c);
        (mw ? rej : acc)++;
    }
    std::printf("accepted %ld rejected %ld\ncases %ld\nwrong %d\n", acc, rej, cases, wrong);
    return wrong ? 1 : 0;
}
