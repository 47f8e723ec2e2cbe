// rgb_args_check.cpp -- csrc/mcraw_rgb_args.h on its own (no HIP: that this file compiles with a plain g++ is part of the test):
// what the three demosaic entry points decide with it about a call -- accept, no-op or reject, and on acceptance every field of
// the launch plan -- against a transcription of the check sequence and plan arithmetic that demosaic_launch in mcraw_rgb.hip
// carried before the header existed.  Message texts are not compared.  Addresses are numbers; nothing is read through them.
// Prints "accepted A rejected R", "cases N" and "wrong N"; every failed check says where.  tests/test_rgb_args.py builds and
// runs it.
#include "mcraw_rgb_args.h"

#include <cstdio>
#include <functional>
#include <limits>
#include <random>
#include <vector>

using mcraw::RgbPlan;

static const uintptr_t BASE = 0x7f0000000000u;    // (16-byte aligned)
static const uintptr_t FAR = BASE + (1ull << 40);  // the output, 16-byte aligned
static const uintptr_t LUT = BASE + (1ull << 41);  // the LUT, 16-byte aligned
static const float NaN = std::numeric_limits<float>::quiet_NaN(), Inf = std::numeric_limits<float>::infinity();

// A call as the sweeps describe it: pitch, frame stride and out_bytes relative to what the other fields need, resolved by one().
struct Call {
    int kind = 0; // 0: mcraw_demosaic_batch, 1: _display_batch (d), 2: _yuv_batch (yv)
    bool no_p = false, no_colors = false;
    mcraw_rgb p{};
    mcraw_display d{};
    mcraw_yuv y{};
    int w = 64, h = 16, n = 2;
    long dpitch = 0, dstride = 0, dbytes = 0; // pitch = w + dpitch, frame stride = minimum + dstride, out_bytes = need + dbytes
    uintptr_t in = BASE, out = FAR;
    int ncolors = -1;                 // -1: n
    int bad_at = -1, bad_what = 0;    // colour `bad_at` holds a NaN gain (0) or an inf matrix entry (1)
};

static Call good(int kind, uint32_t algo)
{
    Call c;
    c.kind = kind;
    c.p.algo = algo, c.p.dtype = kind == 0 ? MCRAW_FLOAT_F16 : 0u, c.p.flags = 0, c.p.cfa = MCRAW_CFA_RGGB;
    for (int i = 0; i < 4; i++)
        c.p.black[i] = 64;
    c.p.white = 4095.0f;
    c.d.dtype = MCRAW_DISP_U8, c.d.layout = MCRAW_DISP_HWC, c.d.lut_log2 = 12, c.d.reserved = 0;
    c.d.lut = reinterpret_cast<const uint16_t *>(LUT);
    c.y.format = MCRAW_YUV_NV12, c.y.lut_log2 = 12, c.y.in_bits = 12, c.y.sh = 14, c.y.y_off = 16, c.y.c_off = 128;
    const int32_t cy[3] = {2990, 9970, 1010}, cb[3] = {-1650, -5500, 7150}, cr[3] = {7150, -6500, -650};
    for (int i = 0; i < 3; i++)
        c.y.cy[i] = cy[i], c.y.cb[i] = cb[i], c.y.cr[i] = cr[i];
    c.y.reserved = 0, c.y.lut = reinterpret_cast<const uint16_t *>(LUT);
    return c;
}

struct Verdict {
    int rc = 0; // 0 accepted (or the no-op of an empty batch), -1 rejected
    bool launches = false;
    // of a launch
    size_t es = 0, Wo = 0, Ho = 0, frame_samples = 0, out_frame = 0;
    bool invec = false, mhc = false;
    uint32_t tilesX = 0, units = 0;
    int shift = 0, kind = 0;
};

static Verdict no() { Verdict v; v.rc = -1; return v; }

// ---- the sequence as demosaic_launch carried it (its context argument left out), with the figures its launch loop used

static bool old_finite_all(const float *v, int n)
{
    for (int i = 0; i < n; i++)
        if (!std::isfinite(v[i]))
            return false;
    return true;
}

static Verdict old_launch(const mcraw_rgb *p, const mcraw_display *d, const mcraw_yuv *yv, const mcraw_rgb_color *colors, int ncolors,
                          uintptr_t in, size_t in_pitch, size_t in_frame_stride, int width, int height, int n, uintptr_t out,
                          size_t out_bytes)
{
    if (!p || n < 0)
        return no();
    if (n == 0)
        return Verdict();
    if (width < 4 || height < 4 || (width & 1) || (height & 1) || width > 65536 || height > 65536)
        return no();
    if (in_pitch < static_cast<size_t>(width))
        return no();
    if (n > 1 && in_frame_stride < (static_cast<size_t>(height) - 1u) * in_pitch + static_cast<size_t>(width))
        return no();
    if (p->algo != MCRAW_RGB_MHC && p->algo != MCRAW_RGB_BIN2)
        return no();
    const uint16_t *lut = d ? d->lut : yv ? yv->lut : nullptr;
    const uint32_t lut_log2 = d ? d->lut_log2 : yv ? yv->lut_log2 : 0u;
    if (d || yv) {
        if (p->dtype != 0u || p->flags != 0u)
            return no();
        if (lut_log2 < 8u || lut_log2 > 16u)
            return no();
        if (!lut || (reinterpret_cast<uintptr_t>(lut) & 15u))
            return no();
    }
    if (d) {
        if (d->dtype != MCRAW_DISP_U8 && d->dtype != MCRAW_DISP_U16)
            return no();
        if (d->layout != MCRAW_DISP_CHW && d->layout != MCRAW_DISP_HWC)
            return no();
        if (d->reserved != 0u)
            return no();
    } else if (yv) {
        if (yv->format != MCRAW_YUV_NV12 && yv->format != MCRAW_YUV_P010)
            return no();
        if (yv->reserved != 0u)
            return no();
        if (yv->in_bits < 8u || yv->in_bits > 16u)
            return no();
        if (yv->sh < 1u || yv->sh > 24u)
            return no();
        const int32_t top = yv->format == MCRAW_YUV_NV12 ? 255 : 1023;
        if (yv->y_off < 0 || yv->y_off > top || yv->c_off < 0 || yv->c_off > top)
            return no();
        const int32_t *rows[3] = {yv->cy, yv->cb, yv->cr};
        for (const int32_t *r : rows) {
            const int64_t mag = std::llabs(static_cast<int64_t>(r[0])) + std::llabs(static_cast<int64_t>(r[1])) +
                                std::llabs(static_cast<int64_t>(r[2]));
            if (4 * ((int64_t{1} << yv->in_bits) - 1) * mag + (int64_t{1} << (yv->sh + 1u)) >= (int64_t{1} << 31))
                return no();
        }
    } else {
        if (p->dtype != MCRAW_FLOAT_F32 && p->dtype != MCRAW_FLOAT_F16 && p->dtype != MCRAW_FLOAT_BF16)
            return no();
    }
    if (p->cfa > MCRAW_CFA_GBRG)
        return no();
    if (p->flags & ~MCRAW_FLOAT_CLIP)
        return no();
    const float bsum = static_cast<float>(static_cast<int>(p->black[0]) + p->black[1] + p->black[2] + p->black[3]);
    if (!std::isfinite(p->white) || !(p->white > 0.25f * bsum))
        return no();
    if (!colors || (ncolors != 1 && ncolors != n))
        return no();
    for (int i = 0; i < ncolors; i++)
        if (!old_finite_all(colors[i].gain, 3) || !old_finite_all(colors[i].m, 9))
            return no();
    const bool mhc = p->algo == MCRAW_RGB_MHC;
    const size_t es = d ? (d->dtype == MCRAW_DISP_U8 ? 1u : 2u) : yv ? (yv->format == MCRAW_YUV_NV12 ? 1u : 2u)
                                                                      : p->dtype == MCRAW_FLOAT_F32 ? 4u : 2u;
    const size_t Wo = mhc ? static_cast<size_t>(width) : static_cast<size_t>(width) / 2u;
    const size_t Ho = mhc ? static_cast<size_t>(height) : static_cast<size_t>(height) / 2u;
    if (yv && ((Ho | Wo) & 1u))
        return no();
    const size_t frame_samples = yv ? Ho * Wo / 2u * 3u : 3u * Ho * Wo;
    if (out_bytes / es / frame_samples < static_cast<size_t>(n))
        return no();
    if (!in || !out || (in & 1u) || (out & (es - 1u)))
        return no();
    // (behind the lock) the kernel, the launch geometry, the bytes per output frame
    Verdict v;
    v.launches = true;
    static const int shift_of[4] = {0, 3, 1, 2};
    v.shift = shift_of[p->cfa];
    v.kind = yv ? (yv->format == MCRAW_YUV_NV12 ? 50 : 51) : d ? (d->dtype == MCRAW_DISP_U8 ? 48 : 49)
             : p->dtype == MCRAW_FLOAT_F32 ? 32 : p->dtype == MCRAW_FLOAT_F16 ? 33 : 34;
    v.mhc = mhc, v.es = es, v.Wo = Wo, v.Ho = Ho, v.frame_samples = frame_samples, v.out_frame = frame_samples * es;
    v.invec = (in & 15u) == 0u && in_pitch % 8u == 0u && (n == 1 || in_frame_stride % 8u == 0u);
    if (mhc) {
        v.tilesX = static_cast<uint32_t>((width + 256u - 1) / 256u);
        v.units = v.tilesX * static_cast<uint32_t>((height + 32u - 1) / 32u);
    } else {
        v.tilesX = static_cast<uint32_t>((Wo + 7u) / 8u);
        v.units = static_cast<uint32_t>((static_cast<size_t>(v.tilesX) * (yv ? Ho / 2u : Ho) + 256u - 1u) / 256u);
    }
    return v;
}

// ---- the same decision as the entry points make it now

static Verdict new_launch(const mcraw_rgb *p, const mcraw_display *d, const mcraw_yuv *yv, const mcraw_rgb_color *colors, int ncolors,
                          uintptr_t in, size_t in_pitch, size_t in_frame_stride, int width, int height, int n, uintptr_t out,
                          size_t out_bytes)
{
    RgbPlan P;
    if (mcraw::rgb_check(p, d, yv, colors, ncolors, reinterpret_cast<const uint16_t *>(in), in_pitch, in_frame_stride, width, height, n,
                         reinterpret_cast<const void *>(out), out_bytes, P))
        return no();
    Verdict v;
    if (P.noop)
        return v;
    v.launches = true;
    v.shift = P.shift, v.kind = P.kind, v.mhc = P.mhc, v.es = P.es, v.Wo = P.Wo, v.Ho = P.Ho, v.frame_samples = P.frame_samples;
    v.out_frame = P.out_frame, v.invec = P.invec, v.tilesX = P.tilesX, v.units = P.units;
    return v;
}

// ---- the comparison

static long cases = 0, accepted = 0, rejected = 0;
static int wrong = 0;

static size_t min_stride(int w, int h, size_t pitch) { return (static_cast<size_t>(h) - 1u) * pitch + static_cast<size_t>(w); }

// bytes the call's output needs (nonsense sizes: whatever the arithmetic gives)
static size_t need(const Call &c)
{
    const bool mhc = c.p.algo != MCRAW_RGB_BIN2;
    const size_t Wo = c.w < 0 ? 0u : mhc ? c.w : c.w / 2, Ho = c.h < 0 ? 0u : mhc ? c.h : c.h / 2;
    const size_t es = c.kind == 1 ? (c.d.dtype == MCRAW_DISP_U8 ? 1u : 2u) : c.kind == 2 ? (c.y.format == MCRAW_YUV_NV12 ? 1u : 2u)
                                                                                          : c.p.dtype == MCRAW_FLOAT_F32 ? 4u : 2u;
    return (c.kind == 2 ? Ho * Wo / 2u * 3u : 3u * Ho * Wo) * es * static_cast<size_t>(c.n > 0 ? c.n : 0);
}

static void one(const Call &c)
{
    static std::vector<mcraw_rgb_color> cols;
    cols.assign(64, mcraw_rgb_color{{2.0f, 1.0f, 1.5f}, {1.5f, -0.25f, -0.25f, -0.25f, 1.5f, -0.25f, -0.25f, -0.25f, 1.5f}});
    if (c.bad_at >= 0)
        (c.bad_what ? cols[c.bad_at].m[4] : cols[c.bad_at].gain[1]) = c.bad_what ? Inf : NaN;
    const size_t pitch = static_cast<size_t>(static_cast<long>(c.w) + c.dpitch);
    const size_t stride = min_stride(c.w, c.h, pitch) + static_cast<size_t>(c.dstride);
    const size_t bytes = need(c) + static_cast<size_t>(c.dbytes);
    const int nc = c.ncolors < 0 ? c.n : c.ncolors;
    const mcraw_rgb *p = c.no_p ? nullptr : &c.p;
    const mcraw_display *d = c.kind == 1 ? &c.d : nullptr;
    const mcraw_yuv *y = c.kind == 2 ? &c.y : nullptr;
    const mcraw_rgb_color *cl = c.no_colors ? nullptr : cols.data();
    const Verdict a = old_launch(p, d, y, cl, nc, c.in, pitch, stride, c.w, c.h, c.n, c.out, bytes);
    const Verdict b = new_launch(p, d, y, cl, nc, c.in, pitch, stride, c.w, c.h, c.n, c.out, bytes);
    cases++;
    (a.rc ? rejected : accepted)++;
    const bool same = a.rc == b.rc && a.launches == b.launches &&
                      (!a.launches || (a.es == b.es && a.Wo == b.Wo && a.Ho == b.Ho && a.frame_samples == b.frame_samples &&
                                       a.out_frame == b.out_frame && a.invec == b.invec && a.mhc == b.mhc && a.tilesX == b.tilesX &&
                                       a.units == b.units && a.shift == b.shift && a.kind == b.kind));
    if (!same && wrong++ < 40)
        std::printf("kind %d algo %u: %d x %d n %d pitch %zu stride %zu in %#zx out %#zx bytes %zu nc %d: was rc %d launch %d es %zu %zu x "
                    "%zu samples %zu frame %zu vec %d tiles %u units %u shift %d pk %d, is rc %d launch %d es %zu %zu x %zu samples %zu frame "
                    "%zu vec %d tiles %u units %u shift %d pk %d\n",
                    c.kind, c.p.algo, c.w, c.h, c.n, pitch, stride, static_cast<size_t>(c.in), static_cast<size_t>(c.out), bytes, nc, a.rc,
                    a.launches, a.es, a.Wo, a.Ho, a.frame_samples, a.out_frame, a.invec, a.tilesX, a.units, a.shift, a.kind, b.rc,
                    b.launches, b.es, b.Wo, b.Ho, b.frame_samples, b.out_frame, b.invec, b.tilesX, b.units, b.shift, b.kind);
}

// ---- the sweeps

typedef std::function<void(Call &)> Mut;

static const int SIZES[] = {-4, 0, 2, 4, 6, 14, 15, 16, 65536, 65538};
static const int EDGE = (2147483647 - 4) / (4 * 255); // the overflow rule's last accepted |c0| + |c1| + |c2| for in_bits 8, sh 1

// Every single change of a good call that the sweeps know: one value of one field each.
static std::vector<Mut> mutations()
{
    std::vector<Mut> m;
    for (int v : SIZES) {
        m.push_back([v](Call &c) { c.w = v; });
        m.push_back([v](Call &c) { c.h = v; });
    }
    for (long v : {-1L, 0L, 8L}) {
        m.push_back([v](Call &c) { c.dpitch = v; });
        m.push_back([v](Call &c) { c.dstride = v; });
    }
    for (int v : {-1, 0, 1, 2, 35})
        m.push_back([v](Call &c) { c.n = v; });
    for (uintptr_t v : {uintptr_t(0), BASE + 1, BASE + 2, BASE})
        m.push_back([v](Call &c) { c.in = v; });
    for (uintptr_t v : {uintptr_t(0), FAR, FAR + 1, FAR + 2, FAR + 4})
        m.push_back([v](Call &c) { c.out = v; });
    for (long v : {-1L, 0L, 1L})
        m.push_back([v](Call &c) { c.dbytes = v; });
    for (uint32_t v = 0; v <= 3; v++)
        m.push_back([v](Call &c) { c.p.algo = v; });
    for (uint32_t v = 0; v <= 4; v++)
        m.push_back([v](Call &c) { c.p.cfa = v; });
    for (uint32_t v = 0; v <= 4; v++) // the float dtypes, one below and one past; with a stage struct: p->dtype non-zero
        m.push_back([v](Call &c) { c.p.dtype = v; });
    for (uint32_t v = 0; v <= 2; v++)
        m.push_back([v](Call &c) { c.p.flags = v; });
    for (float v : {NaN, Inf, 64.0f, 64.5f})
        m.push_back([v](Call &c) { c.p.white = v; });
    for (int v : {0, 1, -1, 3})
        m.push_back([v](Call &c) { c.ncolors = v; });
    m.push_back([](Call &c) { c.no_colors = true; });
    m.push_back([](Call &c) { c.no_p = true; });
    for (int at : {0, 1, 34, 40})
        for (int what : {0, 1})
            m.push_back([at, what](Call &c) { c.bad_at = at, c.bad_what = what; });
    for (uint32_t v = 0; v <= 3; v++) {
        m.push_back([v](Call &c) { c.d.dtype = v; });
        m.push_back([v](Call &c) { c.y.format = v; });
    }
    for (uint32_t v = 0; v <= 2; v++)
        m.push_back([v](Call &c) { c.d.layout = v; });
    m.push_back([](Call &c) { c.d.reserved = 1; });
    m.push_back([](Call &c) { c.y.reserved = 1; });
    for (uintptr_t v : {uintptr_t(0), LUT + 8, LUT})
        m.push_back([v](Call &c) { c.d.lut = c.y.lut = reinterpret_cast<const uint16_t *>(v); });
    for (uint32_t v : {7u, 8u, 16u, 17u})
        m.push_back([v](Call &c) { c.d.lut_log2 = c.y.lut_log2 = v; });
    for (uint32_t v : {7u, 8u, 9u, 16u, 17u})
        m.push_back([v](Call &c) { c.y.in_bits = v; });
    for (uint32_t v : {0u, 1u, 24u, 25u})
        m.push_back([v](Call &c) { c.y.sh = v; });
    for (int fmt : {MCRAW_YUV_NV12, MCRAW_YUV_P010})
        for (int v : {-1, 0, fmt == MCRAW_YUV_NV12 ? 255 : 1023, fmt == MCRAW_YUV_NV12 ? 256 : 1024}) {
            m.push_back([fmt, v](Call &c) { c.y.format = fmt, c.y.y_off = v; });
            m.push_back([fmt, v](Call &c) { c.y.format = fmt, c.y.c_off = v; });
        }
    for (int row = 0; row < 3; row++)
        for (int v : {EDGE, EDGE + 1, -EDGE, -EDGE - 1})
            m.push_back([row, v](Call &c) {
                c.y.in_bits = 8, c.y.sh = 1;
                for (int r = 0; r < 3; r++) {
                    int32_t *q = r == 0 ? c.y.cy : r == 1 ? c.y.cb : c.y.cr;
                    q[0] = q[1] = q[2] = 0;
                    if (r == row)
                        q[1] = v;
                }
            });
    return m;
}

static const int KINDS[] = {0, 1, 2};
static const uint32_t ALGOS[] = {MCRAW_RGB_MHC, MCRAW_RGB_BIN2};

// every output type of every kind x algo: the good calls the sweeps start from
static std::vector<Call> bases()
{
    std::vector<Call> b;
    for (uint32_t algo : ALGOS) {
        for (uint32_t dt : {MCRAW_FLOAT_F32, MCRAW_FLOAT_F16, MCRAW_FLOAT_BF16}) {
            Call c = good(0, algo);
            c.p.dtype = dt, b.push_back(c);
        }
        for (uint32_t dt : {MCRAW_DISP_U8, MCRAW_DISP_U16})
            for (uint32_t lay : {MCRAW_DISP_CHW, MCRAW_DISP_HWC}) {
                Call c = good(1, algo);
                c.d.dtype = dt, c.d.layout = lay, b.push_back(c);
            }
        for (uint32_t f : {MCRAW_YUV_NV12, MCRAW_YUV_P010}) {
            Call c = good(2, algo);
            c.y.format = f, b.push_back(c);
        }
    }
    return b;
}

int main()
{
    const std::vector<Mut> muts = mutations();
    const std::vector<Call> base = bases();
    // one field at a time, from every good call; out_bytes around the need and `out` around its alignment for each of them
    for (const Call &b : base) {
        one(b);
        for (const Mut &m : muts) {
            Call c = b;
            m(c), one(c);
        }
        for (long db : {-1L, 0L, 1L})
            for (uintptr_t o : {FAR, FAR + 1, FAR + 2, FAR + 4}) {
                Call c = b;
                c.dbytes = db, c.out = o, one(c);
            }
    }
    // the geometry fields together
    for (int kind : KINDS)
        for (uint32_t algo : ALGOS)
            for (int w : SIZES)
                for (int h : SIZES)
                    for (long dp : {-1L, 0L, 8L})
                        for (long ds : {-1L, 0L, 8L})
                            for (int n : {-1, 0, 1, 2, 35})
                                for (uintptr_t in : {uintptr_t(0), BASE + 1, BASE + 2, BASE}) {
                                    Call c = good(kind, algo);
                                    c.w = w, c.h = h, c.dpitch = dp, c.dstride = ds, c.n = n, c.in = in, one(c);
                                }
    // 4:2:0 needs an even Ho and Wo: the sizes of the GPU test
    const int even[][2] = {{16, 6}, {14, 8}, {6, 4}, {1000, 6}, {16, 8}, {8, 4}};
    for (const auto &e : even)
        for (int kind : KINDS)
            for (uint32_t algo : ALGOS) {
                Call c = good(kind, algo);
                c.w = e[0], c.h = e[1], one(c);
            }
    // seeded tuples: zero to two changes of a good call
    std::mt19937 rng(20250301u);
    for (int i = 0; i < 200000; i++) {
        Call c = base[rng() % base.size()];
        for (unsigned k = rng() % 3u; k > 0; k--)
            muts[rng() % muts.size()](c);
        one(c);
    }
    std::printf("accepted %ld rejected %ld\n", accepted, rejected);
    std::printf("cases %ld\n", cases);
    std::printf("wrong %d\n", wrong);
    return wrong ? 1 : 0;
}
