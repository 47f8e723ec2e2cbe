// mosaic_args_check.cpp -- csrc/mcraw_mosaic_args.h on its own (no HIP: that this file compiles with a plain g++ is part of the
// test): what the five mosaic stages' entry points decide with it about the geometry of a call -- accept or reject, the extents
// of `in` and `out`, whether they lie on the 16-byte grid -- against transcriptions of the check sequences that each of
// mcraw_shade / stats / fixpix / denoise / merge .hip carried before the header existed (their geometry part: the stages'
// own struct fields are left out, but for merge's `count` and the bytes stats writes).  Addresses are numbers; nothing is read
// through them.  Prints "cases N" and "wrong N"; every failed check says where.  tests/test_mosaic_args.py builds and runs it.
#include "mcraw_mosaic_args.h"

#include <cstdio>
#include <random>

using mcraw::MosaicBatch;

struct Call {
    uintptr_t in, out;
    size_t ip, ifs, op, ofs; // pitches and frame strides
    int w, h, n;
    unsigned count; // merge: outputs
    size_t need;    // stats: bytes written at `out`
};

struct Verdict {
    int rc = 0;           // 0 accepted, -1 rejected
    bool launches = false; // accepted, and not the no-op of an empty batch: the four below are what the launch would use
    size_t in_ext = 0, out_ext = 0;
    bool invec = false, outvec = false;
};

static Verdict no() { Verdict v; v.rc = -1; return v; }
static Verdict noop() { return Verdict(); }
static Verdict yes(size_t in_ext, size_t out_ext, bool invec, bool outvec)
{
    Verdict v;
    v.launches = true, v.in_ext = in_ext, v.out_ext = out_ext, v.invec = invec, v.outvec = outvec;
    return v;
}

// ---- the sequences as they were, one per unit

static Verdict old_map_to_map(const Call &c, bool inplace_form) // shade (in place allowed), fixpix, denoise
{
    if (c.n < 0)
        return no();
    if (c.n == 0)
        return noop();
    if (!c.in || !c.out)
        return no();
    if ((c.in & 1u) || (c.out & 1u))
        return no();
    if (c.w < 1 || c.h < 1 || c.w > 65536 || c.h > 65536)
        return no();
    const size_t W = static_cast<size_t>(c.w), H = static_cast<size_t>(c.h);
    if (c.ip < W || c.op < W)
        return no();
    if (c.n > 1 && (c.ifs < (H - 1u) * c.ip + W || c.ofs < (H - 1u) * c.op + W))
        return no();
    const size_t in_ext = static_cast<size_t>(c.n - 1) * c.ifs + (H - 1u) * c.ip + W;
    const size_t out_ext = static_cast<size_t>(c.n - 1) * c.ofs + (H - 1u) * c.op + W;
    const bool inplace = inplace_form && c.in == c.out && c.ip == c.op && (c.n == 1 || c.ifs == c.ofs);
    const uintptr_t ia = c.in, oa = c.out;
    if (!inplace && ia < oa + 2u * out_ext && oa < ia + 2u * in_ext)
        return no();
    return yes(in_ext, out_ext, (ia & 15u) == 0u && c.ip % 8u == 0u && (c.n == 1 || c.ifs % 8u == 0u),
               (oa & 15u) == 0u && c.op % 8u == 0u && (c.n == 1 || c.ofs % 8u == 0u));
}

static Verdict old_shade(const Call &c) { return old_map_to_map(c, true); }
static Verdict old_fixpix(const Call &c) { return old_map_to_map(c, false); }
static Verdict old_denoise(const Call &c) { return old_map_to_map(c, false); }

static Verdict old_merge(const Call &c)
{
    if (c.n < 0)
        return no();
    if (c.n == 0 || c.count == 0u)
        return noop();
    if (!c.in || !c.out)
        return no();
    if ((c.in & 1u) || (c.out & 1u))
        return no();
    if (c.w < 1 || c.h < 1 || c.w > 65536 || c.h > 65536)
        return no();
    const size_t W = static_cast<size_t>(c.w), H = static_cast<size_t>(c.h);
    if (c.ip < W || c.op < W)
        return no();
    if ((c.n > 1 && c.ifs < (H - 1u) * c.ip + W) || (c.count > 1u && c.ofs < (H - 1u) * c.op + W))
        return no();
    if (c.count > static_cast<unsigned>(c.n)) // (first = 0: first + count must not exceed n)
        return no();
    const size_t in_ext = static_cast<size_t>(c.n - 1) * c.ifs + (H - 1u) * c.ip + W;
    const size_t out_ext = static_cast<size_t>(c.count - 1u) * c.ofs + (H - 1u) * c.op + W;
    const uintptr_t ia = c.in, oa = c.out;
    if (ia < oa + 2u * out_ext && oa < ia + 2u * in_ext)
        return no();
    return yes(in_ext, out_ext, (ia & 15u) == 0u && c.ip % 8u == 0u && (c.n == 1 || c.ifs % 8u == 0u),
               (oa & 15u) == 0u && c.op % 8u == 0u && (c.count == 1u || c.ofs % 8u == 0u));
}

static Verdict old_stats(const Call &c)
{
    if (c.n < 0)
        return no();
    if (c.n == 0)
        return noop();
    if (!c.in || !c.out)
        return no();
    if (c.in & 1u)
        return no();
    if (c.out & 7u)
        return no();
    if (c.w < 1 || c.h < 1 || c.w > 65536 || c.h > 65536)
        return no();
    const size_t W = static_cast<size_t>(c.w), H = static_cast<size_t>(c.h);
    if (c.ip < W)
        return no();
    if (c.n > 1 && c.ifs < (H - 1u) * c.ip + W)
        return no();
    const size_t in_ext = static_cast<size_t>(c.n - 1) * c.ifs + (H - 1u) * c.ip + W;
    const uintptr_t ia = c.in, oa = c.out;
    if (ia < oa + c.need && oa < ia + 2u * in_ext)
        return no();
    return yes(in_ext, 0u, (ia & 15u) == 0u && c.ip % 8u == 0u && (c.n == 1 || c.ifs % 8u == 0u), false);
}

// ---- the same decisions as the units make them now

static const void *ptr(uintptr_t a) { return reinterpret_cast<const void *>(a); }

static Verdict new_map_to_map(const Call &c, bool inplace_form)
{
    if (c.n < 0)
        return no();
    if (c.n == 0)
        return noop();
    if (!c.in || !c.out)
        return no();
    const MosaicBatch I(ptr(c.in), c.ip, c.ifs, static_cast<size_t>(c.n), c.w, c.h);
    const MosaicBatch O(ptr(c.out), c.op, c.ofs, static_cast<size_t>(c.n), c.w, c.h);
    if (mcraw::check(I, O))
        return no();
    const bool inplace = inplace_form && c.in == c.out && c.ip == c.op && (c.n == 1 || c.ifs == c.ofs);
    if (!inplace && mcraw::overlap(I, O))
        return no();
    return yes(I.extent(), O.extent(), I.on_grid(), O.on_grid());
}

static Verdict new_shade(const Call &c) { return new_map_to_map(c, true); }
static Verdict new_fixpix(const Call &c) { return new_map_to_map(c, false); }
static Verdict new_denoise(const Call &c) { return new_map_to_map(c, false); }

static Verdict new_merge(const Call &c)
{
    if (c.n < 0)
        return no();
    if (c.n == 0 || c.count == 0u)
        return noop();
    if (!c.in || !c.out)
        return no();
    if ((c.in & 1u) || (c.out & 1u))
        return no();
    const MosaicBatch I(ptr(c.in), c.ip, c.ifs, static_cast<size_t>(c.n), c.w, c.h);
    const MosaicBatch O(ptr(c.out), c.op, c.ofs, static_cast<size_t>(c.count), c.w, c.h);
    if (mcraw::check(I, O))
        return no();
    if (c.count > static_cast<unsigned>(c.n))
        return no();
    if (mcraw::overlap(I, O))
        return no();
    return yes(I.extent(), O.extent(), I.on_grid(), O.on_grid());
}

static Verdict new_stats(const Call &c)
{
    if (c.n < 0)
        return no();
    if (c.n == 0)
        return noop();
    if (!c.in || !c.out)
        return no();
    if (c.in & 1u)
        return no();
    if (c.out & 7u)
        return no();
    const MosaicBatch I(ptr(c.in), c.ip, c.ifs, static_cast<size_t>(c.n), c.w, c.h);
    if (I.check())
        return no();
    if (mcraw::ranges_overlap(I.base, I.bytes(), c.out, c.need))
        return no();
    return yes(I.extent(), 0u, I.on_grid(), false);
}

// ---- the comparison

static long cases = 0, accepted = 0, rejected = 0;
static int wrong = 0;

static void compare(const char *stage, const Call &c, const Verdict &a, const Verdict &b)
{
    const bool same = a.rc == b.rc && a.launches == b.launches &&
                      (!a.launches || (a.in_ext == b.in_ext && a.out_ext == b.out_ext && a.invec == b.invec && a.outvec == b.outvec));
    if (!same && wrong++ < 40)
        std::printf("%s: in %#zx pitch %zu stride %zu, out %#zx pitch %zu stride %zu, %d x %d, n %d count %u need %zu: was rc %d ext %zu / "
                    "%zu grid %d / %d, is rc %d ext %zu / %zu grid %d / %d\n",
                    stage, static_cast<size_t>(c.in), c.ip, c.ifs, static_cast<size_t>(c.out), c.op, c.ofs, c.w, c.h, c.n, c.count, c.need,
                    a.rc, a.in_ext, a.out_ext, a.invec, a.outvec, b.rc, b.in_ext, b.out_ext, b.invec, b.outvec);
}

static void one(const Call &c)
{
    cases++;
    const Verdict s = old_shade(c);
    (s.rc ? rejected : accepted)++;
    compare("shade", c, s, new_shade(c));
    compare("fixpix", c, old_fixpix(c), new_fixpix(c));
    compare("denoise", c, old_denoise(c), new_denoise(c));
    compare("merge", c, old_merge(c), new_merge(c));
    compare("stats", c, old_stats(c), new_stats(c));
}

// the smallest frame stride that check() lets pass for more than one frame (nonsense sizes: whatever the arithmetic gives)
static size_t min_stride(int w, int h, size_t pitch)
{
    return (static_cast<size_t>(h) - 1u) * pitch + static_cast<size_t>(w);
}

static const uintptr_t BASE = 0x7f0000000000u;   // (16-byte aligned)
static const uintptr_t FAR = BASE + (1ull << 40); // beyond every extent of the sizes below

// Every combination of the edge values: sizes, pitches around the width, frame strides around the minimum, 0 .. 2 frames,
// addresses odd / on the 2-byte grid / on the 16-byte grid; `out` far from `in`.
static void edge_grid()
{
    const int sizes[] = {1, 2, 7, 8, 9, 65536, 65537, 0, -4};
    const long dpitch[] = {-1, 0, 1, 8}, dstride[] = {-1, 0, 1};
    const uintptr_t offs[] = {1, 2, 0};
    for (int w : sizes)
        for (int h : sizes)
            for (long dp : dpitch)
                for (long ds : dstride)
                    for (int n = 0; n <= 2; n++)
                        for (uintptr_t io : offs)
                            for (long dq : dpitch)
                                for (long dt : dstride)
                                    for (uintptr_t oo : offs) {
                                        Call c{};
                                        c.w = w, c.h = h, c.n = n;
                                        c.in = BASE + io, c.out = FAR + oo;
                                        c.ip = static_cast<size_t>(static_cast<long>(w) + dp);
                                        c.op = static_cast<size_t>(static_cast<long>(w) + dq);
                                        c.ifs = min_stride(w, h, c.ip) + static_cast<size_t>(ds);
                                        c.ofs = min_stride(w, h, c.op) + static_cast<size_t>(dt);
                                        c.count = static_cast<unsigned>(n);
                                        c.need = 96u * static_cast<size_t>(n > 0 ? n : 0);
                                        one(c);
                                    }
    // pointers missing, n below 0, merge's count 0 and above n
    Call c{};
    c.w = 24, c.h = 10, c.n = 2, c.ip = c.op = 24, c.ifs = c.ofs = 240, c.in = BASE, c.out = FAR, c.count = 2, c.need = 192;
    Call d = c;
    d.in = 0, one(d);
    d = c, d.out = 0, one(d);
    d = c, d.n = -1, one(d);
    d = c, d.count = 0, d.out = 0, one(d);
    d = c, d.count = 3, one(d);
}

// The layouts of the GPU tests' rejections, and their neighbours that must pass: in place, `out` inside `in`, `out` ending inside
// `in`, the same base with another pitch or frame stride, ranges that touch, ranges that share one sample.
static void overlap_layouts()
{
    const int dims[][3] = {{24, 10, 2}, {24, 10, 1}, {1, 1, 1}, {7, 3, 2}, {8, 1, 2}, {41, 35, 2}};
    for (const auto &g : dims)
        for (size_t pad : {size_t(0), size_t(1), size_t(8)})
            for (size_t gap : {size_t(0), size_t(8), size_t(13)}) {
                Call c{};
                c.w = g[0], c.h = g[1], c.n = g[2];
                c.ip = c.op = static_cast<size_t>(c.w) + pad;
                c.ifs = c.ofs = min_stride(c.w, c.h, c.ip) + gap;
                c.in = BASE, c.count = static_cast<unsigned>(c.n);
                const size_t bytes = 2u * ((static_cast<size_t>(c.n) - 1u) * c.ifs + min_stride(c.w, c.h, c.ip));
                c.need = 96u * static_cast<size_t>(c.n);
                const long at[] = {0, 2, 16, 32, static_cast<long>(bytes) - 16, static_cast<long>(bytes) - 2, static_cast<long>(bytes),
                                   static_cast<long>(bytes) + 2, static_cast<long>(bytes) + 14, -2, -16, -static_cast<long>(bytes) + 2,
                                   -static_cast<long>(bytes), -static_cast<long>(bytes) - 2, -96, -192, -8, 8};
                for (long a : at) {
                    Call d = c;
                    d.out = static_cast<uintptr_t>(static_cast<long>(BASE) + a);
                    one(d);
                    d.op = c.op + 8u, d.ofs = min_stride(c.w, c.h, d.op) + gap, one(d); // another pitch
                    d = c, d.out = static_cast<uintptr_t>(static_cast<long>(BASE) + a), d.ofs = c.ofs + 8u, one(d); // another frame stride
                    d.count = 1, one(d);
                }
            }
}

// Seeded tuples: small frames close to each other in a small arena, every argument a little off as often as not.
static void seeded(unsigned seed, int rounds)
{
    std::mt19937 rng(seed);
    auto pick = [&](int lo, int hi) { return static_cast<int>(rng() % static_cast<unsigned>(hi - lo + 1)) + lo; };
    for (int i = 0; i < rounds; i++) {
        Call c{};
        c.w = pick(0, 40) ? pick(1, 48) : pick(-2, 0) + (pick(0, 1) ? 65537 : 0);
        c.h = pick(0, 40) ? pick(1, 12) : pick(-2, 0) + (pick(0, 1) ? 65537 : 0);
        c.n = pick(0, 30) ? pick(1, 4) : pick(-1, 0);
        c.count = static_cast<unsigned>(pick(0, 5));
        c.ip = static_cast<size_t>(c.w + (pick(0, 6) ? pick(0, 9) : -1));
        c.op = static_cast<size_t>(c.w + (pick(0, 6) ? pick(0, 9) : -1));
        c.ifs = min_stride(c.w, c.h, c.ip) + static_cast<size_t>(pick(0, 6) ? pick(0, 17) : -1);
        c.ofs = min_stride(c.w, c.h, c.op) + static_cast<size_t>(pick(0, 6) ? pick(0, 17) : -1);
        c.in = pick(0, 50) ? BASE + static_cast<uintptr_t>(pick(0, 3) ? 2 * pick(0, 4096) : 16 * pick(0, 512)) + (pick(0, 20) ? 0u : 1u) : 0u;
        c.out = pick(0, 50) ? BASE + static_cast<uintptr_t>(pick(0, 3) ? 2 * pick(0, 4096) : 16 * pick(0, 512)) + (pick(0, 20) ? 0u : 1u) : 0u;
        if (pick(0, 3) == 0)
            c.out = c.in, c.op = pick(0, 2) ? c.ip : c.op, c.ofs = pick(0, 2) ? c.ifs : c.ofs; // in place, or nearly
        c.need = static_cast<size_t>(pick(0, 4)) * 96u;
        one(c);
    }
}

int main()
{
    edge_grid();
    overlap_layouts();
    seeded(20240611u, 200000);
    std::printf("accepted %ld rejected %ld\n", accepted, rejected);
    std::printf("cases %ld\n", cases);
    std::printf("wrong %d\n", wrong);
    return wrong ? 1 : 0;
}
