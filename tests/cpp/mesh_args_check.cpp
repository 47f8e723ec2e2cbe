// mesh_args_check.cpp -- csrc/mcraw_mesh_args.h on its own (no HIP: that this file compiles with a plain g++ is part of the test):
// what mcraw_demosaic_mesh_batch decides about a call, one defect at a time; over a sweep of frame and output sizes, the meshes of
// the affine warp's 81 extreme linear parts and of seeded maps inside its bounds: every tile in the regime, the interpolated
// positions within 1/256 sample of warp_pos; and hostile meshes -- full-range random int32 nodes, folds, constant nodes --: for
// every tile the index arithmetic of krgb_mesh, transcribed: every staged row and column and every LDS index inside the arrays,
// every sample a tap can reach (MHC's halo included) within 4 of the frame, the tap clamp silent wherever the window is in the
// regime, and the 32-bit form of the interpolation equal to the 64-bit statement wherever the kernel uses it.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "mcraw_mesh_args.h"

using namespace mcraw;

static long cases = 0, wrong = 0, accepted = 0, rejected = 0, tiles_in = 0, tiles_out = 0, narrow_px = 0, wide_px = 0;

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
    mcraw_mesh m;
    mcraw_display d;
    mcraw_yuv y;
    bool has_p = true, has_m = true, has_d = false, has_y = false;
    mcraw_rgb_color col[3];
    int ncolors = 1;
    uintptr_t nodes = 0x800000;
    size_t nodes_bytes = 2 * 2 * 3 * 8;
    int nmesh = 2;
    uintptr_t in = 0x10000, out = 0x4000000;
    size_t pitch = 64, fstride = 64 * 32, out_bytes = 1 << 22;
    int width = 64, height = 32, n = 2;
};

static Call good()
{
    Call c;
    std::memset(&c.p, 0, sizeof c.p);
    std::memset(&c.m, 0, sizeof c.m);
    std::memset(&c.d, 0, sizeof c.d);
    std::memset(&c.y, 0, sizeof c.y);
    c.p.algo = MCRAW_RGB_MESH, c.p.dtype = MCRAW_FLOAT_F32, c.p.cfa = MCRAW_CFA_GRBG, c.p.white = 4095.0f;
    c.m.out_w = 40, c.m.out_h = 20, c.m.filter = MCRAW_FILTER_CUBIC;
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

static const char *run(const Call &c, MeshPlan &P)
{
    const char *why = mesh_check(c.has_p ? &c.p : nullptr, c.has_m ? &c.m : nullptr, c.has_d ? &c.d : nullptr, c.has_y ? &c.y : nullptr, c.col,
                                 c.ncolors, reinterpret_cast<const int32_t *>(c.nodes), c.nodes_bytes, c.nmesh, reinterpret_cast<const uint16_t *>(c.in),
                                 c.pitch, c.fstride, c.width, c.height, c.n, reinterpret_cast<const void *>(c.out), c.out_bytes, P);
    (why ? rejected : accepted)++;
    return why;
}

template <class F>
static void defect(F f, const char *part)
{
    Call c = good();
    f(c);
    MeshPlan P;
    const char *why = run(c, P);
    CHECK(why != nullptr);
    if (why)
        CHECK(std::strstr(why, part) != nullptr);
}

static void decisions()
{
    MeshPlan P;
    Call g = good();
    CHECK(run(g, P) == nullptr && !P.rgb.noop && P.rgb.Wo == 40 && P.rgb.Ho == 20 && P.tilesX == 2 && P.tilesY == 1 && P.units == 2 && P.Mx == 3 &&
          P.My == 2 && P.nodes() == 6 && P.permesh);
    g.nmesh = 1, g.nodes_bytes = 6 * 8;
    CHECK(run(g, P) == nullptr && !P.permesh);
    g = good(), g.n = 0, g.in = 0, g.out = 0, g.nmesh = 7;
    CHECK(run(g, P) == nullptr && P.rgb.noop);
    g = good(), g.has_d = true, g.p.dtype = 0;
    CHECK(run(g, P) == nullptr && P.rgb.kind == PK_DISP8);
    g = good(), g.has_y = true, g.p.dtype = 0;
    CHECK(run(g, P) == nullptr && P.rgb.kind == PK_NV12);
    defect([](Call &c) { c.has_p = false; }, "bad arguments");
    defect([](Call &c) { c.has_m = false; }, "bad arguments");
    defect([](Call &c) { c.nodes = 0; }, "bad arguments");
    defect([](Call &c) { c.n = -1; }, "bad arguments");
    defect([](Call &c) { c.has_d = c.has_y = true, c.p.dtype = 0; }, "at once");
    defect([](Call &c) { c.width = 6; }, "8 .. 65536");
    defect([](Call &c) { c.height = 31; }, "8 .. 65536");
    for (uint32_t a : {0u, 1u, 2u, 3u, 4u, 5u, 6u, 8u})
        defect([a](Call &c) { c.p.algo = a; }, "MCRAW_RGB_MESH");
    defect([](Call &c) { c.p.cfa = 4; }, "cfa");
    defect([](Call &c) { c.m.reserved = 1; }, "reserved");
    defect([](Call &c) { c.m.filter = 2; }, "filter");
    defect([](Call &c) { c.m.out_w = 0; }, "1 .. 65536");
    defect([](Call &c) { c.m.out_h = 65537; }, "1 .. 65536");
    defect([](Call &c) { c.has_y = true, c.p.dtype = 0, c.m.out_w = 39; }, "4:2:0");
    defect([](Call &c) { c.nmesh = 0; }, "nmesh");
    defect([](Call &c) { c.nmesh = 3; }, "nmesh");
    defect([](Call &c) { c.nodes |= 4; }, "8-byte");
    defect([](Call &c) { c.nodes_bytes -= 1; }, "nodes_bytes");
    defect([](Call &c) { c.out = 0; }, "out");
    defect([](Call &c) { c.out_bytes = 2 * 3 * 20 * 40 * 4 - 1; }, "out_bytes");
    mcraw_mesh big{};
    big.out_w = big.out_h = 65536, big.filter = MCRAW_FILTER_LINEAR;
    CHECK(P.geometry(&big) == nullptr && P.nodes() == 2049u * 2049u);
}

// csrc/mcraw_rgb_dev.h's reflect101, transcribed: -k -> k, n - 1 + k -> n - 1 - k, anything further clamped into 0 .. n - 1.
static int64_t reflect(int64_t i, int64_t n)
{
    i = i < 0 ? -i : i;
    i = i > n - 1 ? 2 * (n - 1) - i : i;
    return std::min(std::max<int64_t>(i, 0), n - 1);
}

// One tile through krgb_mesh's index arithmetic.  Returns whether its window is in the regime.
static bool tile(const int32_t *mesh, const MeshPlan &P, uint32_t ty, uint32_t tx, int W, int H)
{
    const uint32_t Wo = static_cast<uint32_t>(P.rgb.Wo), Ho = static_cast<uint32_t>(P.rgb.Ho);
    const uint32_t k0 = tx * WARP_TW, k1 = std::min(k0 + WARP_TW, Wo) - 1, i0 = ty * WARP_TH, i1 = std::min(i0 + WARP_TH, Ho) - 1;
    int32_t cy[4], cx[4];
    mesh_cell(mesh, P.Mx, ty, tx, cy, cx);
    const WarpWin win = mesh_window(cy, cx, i1 - i0, k1 - k0, W, H);
    const int64_t pb = win.pb, eb = win.eb;
    const uint32_t np = std::min(win.np, MESH_NP), ne = std::min(win.ne, MESH_NE);
    const int32_t rmax = mesh_tap_max_row(win.np), cmax = mesh_tap_max_col(win.ne);
    const bool regime = mesh_in_regime(win), narrow = mesh_narrow(cy) && mesh_narrow(cx);
    bool ok = win.np >= 1 && win.ne >= 1 && np >= 2 && ne >= 1 && !(pb & 1) && !(eb & 7) && rmax == 2 * static_cast<int32_t>(np) - 4 && rmax >= 0 &&
              cmax == 8 * static_cast<int32_t>(ne) - 4;
    // staging: rows r < 2 np + 4 of s_raw from frame row pb - 2 on, pieces q < ne + 2 from column eb - 8 on
    ok = ok && 2 * np + 4 <= WARP_RAWH && 8 * (ne + 2) <= WARP_RAWW;
    ok = ok && pb - 2 >= -4 && pb - 2 + (2 * np + 4) - 1 <= H - 1 + 4; // no staged row leaves the frame by more than 4
    // every staged sample is read at row reflect(pb - 2 + r), column reflect(eb - 8 + 8 q + k) of the frame: inside it for any nodes.
    // A column on the 8-grid's rim may lie up to 16 out, further than one reflection reaches; reflect101's last step clamps it into
    // the row, and no tap reaches it (below: the taps, halo included, stay within 4 of the frame, where one reflection is exact)
    for (int64_t r = 0; r < 2 * np + 4; r++) {
        const int64_t y = reflect(pb - 2 + r, H);
        ok = ok && y >= 0 && y <= H - 1;
    }
    for (int64_t c = 0; c < 8 * (ne + 2); c++) {
        const int64_t x = reflect(eb - 8 + c, W);
        ok = ok && x >= 0 && x <= W - 1 && eb - 8 + c >= -16 && eb - 8 + c <= W - 1 + 16;
    }
    // phase A: rp < np, q < ne reads raw rows 2 rp + AR + 0 .. 4, columns 8 q .. 8 q + 17, writes estimates row 2 rp + AR, columns 8 q .. + 7
    ok = ok && 2 * (np - 1) + 1 + 4 < 2 * np + 4 && 8 * (ne - 1) + 17 < 8 * (ne + 2) && 2 * np <= WARP_EROWS && 8 * ne <= WARP_ECOLS;
    for (uint32_t i = i0; i <= i1 && ok; i++) {
        int32_t ly = 0, ry = 0, lx = 0, rx = 0;
        if (narrow) {
            mesh_row32(cy, i - i0, ly, ry);
            mesh_row32(cx, i - i0, lx, rx);
        }
        for (uint32_t k = k0; k <= k1; k++) {
            const int64_t y64 = mesh_lerp64(cy, i - i0, k - k0), x64 = mesh_lerp64(cx, i - i0, k - k0);
            if (narrow) { // the form the kernel uses here
                ok = ok && mesh_lerp32(cy[0], ly, ry, k - k0) == y64 && mesh_lerp32(cx[0], lx, rx, k - k0) == x64;
                ok = ok && mesh_clamp32(static_cast<int32_t>(y64), H) == mesh_clamp(y64, H) && mesh_clamp32(static_cast<int32_t>(x64), W) == mesh_clamp(x64, W);
                narrow_px++;
            } else
                wide_px++;
            ok = ok && y64 >= INT32_MIN && y64 <= INT32_MAX && x64 >= INT32_MIN && x64 <= INT32_MAX;
            const int64_t Y = mesh_clamp(y64, H), X = mesh_clamp(x64, W);
            const int64_t ur = (Y >> 8) - 1 - pb, uc = (X >> 8) - 1 - eb;
            const int64_t r0 = std::min<int64_t>(std::max<int64_t>(ur, 0), rmax), c0 = std::min<int64_t>(std::max<int64_t>(uc, 0), cmax);
            ok = ok && ur >= 0 && uc >= 0;     // the corners bound every pixel from below, whatever the nodes
            if (regime)
                ok = ok && r0 == ur && c0 == uc; // ... and from above: in the regime the clamp never acts
            ok = ok && r0 + 3 < 2 * static_cast<int64_t>(np) && c0 + 3 < 8 * static_cast<int64_t>(ne);
            ok = ok && (2 * WARP_EROWS + static_cast<uint64_t>(r0) + 3) * WARP_ESTRIDE + static_cast<uint64_t>(c0) + 3 < 3u * WARP_EROWS * WARP_ESTRIDE;
            // the samples the taps reach, MHC's halo of 2 included: within 4 of the frame, one reflection suffices
            ok = ok && pb + r0 - 2 >= -4 && pb + r0 + 3 + 2 <= H - 1 + 4 && eb + c0 - 2 >= -4 && eb + c0 + 3 + 2 <= W - 1 + 4;
            ok = ok && 4 <= H - 1 && 4 <= W - 1;
        }
    }
    if (!ok)
        std::printf("tile (%u, %u) of %u x %u onto %d x %d: window pb %d eb %d np %u ne %u\n", ty, tx, Ho, Wo, H, W, win.pb, win.eb, win.np, win.ne);
    CHECK(ok);
    (regime ? tiles_in : tiles_out)++;
    return regime;
}

static bool sweep(const std::vector<int32_t> &mesh, const MeshPlan &P, int W, int H)
{
    bool all = true;
    for (uint32_t ty = 0; ty < P.tilesY; ty++)
        for (uint32_t tx = 0; tx < P.tilesX; tx++)
            all = tile(mesh.data(), P, ty, tx, W, H) && all;
    // mcraw_mesh_check's verdict is the sweep's
    mcraw_mesh m{};
    m.out_w = static_cast<uint32_t>(P.rgb.Wo), m.out_h = static_cast<uint32_t>(P.rgb.Ho), m.filter = MCRAW_FILTER_CUBIC;
    CHECK((mesh_nodes_check(&m, mesh.data(), 1, W, H, 0) == nullptr) == all);
    return all;
}

static MeshPlan plan_of(uint32_t Wo, uint32_t Ho)
{
    mcraw_mesh m{};
    m.out_w = Wo, m.out_h = Ho, m.filter = MCRAW_FILTER_CUBIC;
    MeshPlan P;
    CHECK(P.geometry(&m) == nullptr && P.tilesX * WARP_TW >= Wo && P.tilesY * WARP_TH >= Ho && P.Mx == P.tilesX + 1 && P.My == P.tilesY + 1);
    return P;
}

// The mesh of an affine map: warp_pos at the nodes.  Its positions: within 1/256 of warp_pos, equal under the identity linear part.
static void affine(const int32_t *m, uint32_t Wo, uint32_t Ho, int W, int H)
{
    const MeshPlan P = plan_of(Wo, Ho);
    std::vector<int32_t> mesh(2 * P.nodes());
    for (uint32_t a = 0; a < P.My; a++)
        for (uint32_t b = 0; b < P.Mx; b++) {
            int64_t Y, X;
            warp_pos(m, 32 * a, 32 * b, Y, X);
            mesh[2 * (a * P.Mx + b)] = static_cast<int32_t>(Y), mesh[2 * (a * P.Mx + b) + 1] = static_cast<int32_t>(X);
        }
    CHECK(sweep(mesh, P, W, H)); // every tile in the regime
    const bool ident = m[0] == 65536 && m[1] == 0 && m[3] == 0 && m[4] == 65536;
    int64_t worst = 0;
    for (uint32_t i = 0; i < Ho; i++)
        for (uint32_t k = 0; k < Wo; k++) {
            int32_t cy[4], cx[4];
            mesh_cell(mesh.data(), P.Mx, i >> 5, k >> 5, cy, cx);
            int64_t Y, X;
            warp_pos(m, i, k, Y, X);
            worst = std::max<int64_t>(worst, std::max<int64_t>(std::llabs(mesh_lerp64(cy, i & 31, k & 31) - Y), std::llabs(mesh_lerp64(cx, i & 31, k & 31) - X)));
        }
    CHECK(worst <= (ident ? 0 : 1));
}

static void affine_meshes()
{
    const int W = 328, H = 120;
    const int32_t ext[2] = {-16384, 16384};
    long swept = 0;
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
                                lo[0] = std::min<long long>(lo[0], Y), hi[0] = std::max<long long>(hi[0], Y);
                                lo[1] = std::min<long long>(lo[1], X), hi[1] = std::max<long long>(hi[1], X);
                            }
                            if (hi[0] - lo[0] > 256LL * (H - 1) || hi[1] - lo[1] > 256LL * (W - 1))
                                continue;
                            m[2] = static_cast<int32_t>((cnr & 2) ? 256LL * (H - 1) - hi[0] : -lo[0]);
                            m[5] = static_cast<int32_t>((cnr & 1) ? 256LL * (W - 1) - hi[1] : -lo[1]);
                            affine(m, Wo, Ho, W, H);
                            swept++;
                        }
    CHECK(swept >= 81 * 4);
    std::mt19937 rng(11);
    long seeded = 0;
    for (int it = 0; it < 3000; it++) {
        const int w = 8 + 2 * static_cast<int>(rng() % 120), h = 8 + 2 * static_cast<int>(rng() % 60);
        const uint32_t Wo = 1 + rng() % 100, Ho = 1 + rng() % 70;
        int32_t m[6] = {65536 + static_cast<int32_t>(rng() % 32769) - 16384, static_cast<int32_t>(rng() % 32769) - 16384, 0,
                        static_cast<int32_t>(rng() % 32769) - 16384, 65536 + static_cast<int32_t>(rng() % 32769) - 16384, 0};
        if (it % 5 == 0)
            m[0] = m[4] = 65536, m[1] = m[3] = 0;
        m[2] = static_cast<int32_t>(rng() % (256 * h)) - 64, m[5] = static_cast<int32_t>(rng() % (256 * w)) - 64;
        if (it % 2 && warp_map_check(m, w, h, Wo, Ho)) // (every other map may leave the frame: the clamp only shrinks a window)
            continue;
        seeded++;
        affine(m, Wo, Ho, w, h);
    }
    CHECK(seeded >= 1500);
    std::printf("affine meshes: %ld at the bounds, %ld seeded, every tile in the regime: %s\n", swept, seeded, tiles_out == 0 ? "yes" : "NO");
    CHECK(tiles_out == 0);
}

static void hostile_meshes()
{
    std::mt19937 rng(13);
    const long before_in = tiles_in;
    for (int it = 0; it < 1500; it++) {
        const int w = 8 + 2 * static_cast<int>(rng() % 150), h = 8 + 2 * static_cast<int>(rng() % 90);
        const uint32_t Wo = 1 + rng() % 130, Ho = 1 + rng() % 100;
        const MeshPlan P = plan_of(Wo, Ho);
        std::vector<int32_t> mesh(2 * P.nodes());
        const int kind = it % 6;
        const int32_t cst[2] = {static_cast<int32_t>(rng()), static_cast<int32_t>(rng())};
        for (size_t j = 0; j < mesh.size(); j++) {
            const int64_t side = 256LL * ((j & 1) ? w : h);
            switch (kind) {
            case 0: mesh[j] = static_cast<int32_t>(rng()); break;                                         // full-range int32
            case 1: mesh[j] = static_cast<int32_t>(static_cast<int64_t>(rng() % (3 * side)) - side); break; // about the frame: folds, huge tiles
            case 2: mesh[j] = cst[j & 1]; break;                                                          // constant, anywhere
            case 3: mesh[j] = static_cast<int32_t>(rng() % side); break;                                  // inside the frame, unordered
            case 4: mesh[j] = (rng() & 1) ? INT32_MAX : INT32_MIN; break;                                 // the extremes of the format
            default: mesh[j] = static_cast<int32_t>((static_cast<int64_t>(rng() % (1 << 22)) - (1 << 21)) * ((rng() & 3) ? 1 : 2)); // about the 32-bit form's limit
            }
        }
        sweep(mesh, P, w, h);
    }
    CHECK(narrow_px > 100000 && wide_px > 100000 && tiles_out > 1000 && tiles_in > before_in);
    std::printf("hostile meshes: %ld tiles outside the regime, %ld inside; %ld pixels through the 32-bit form, %ld through the 64-bit one\n", tiles_out,
                tiles_in - before_in, narrow_px, wide_px);
}

int main()
{
    static_assert(sizeof(mcraw_mesh) == 16, "the header's layout");
    static_assert(MESH_NP == 26 && MESH_NE == 8, "the header's np' and ne'");
    decisions();
    affine_meshes();
    hostile_meshes();
    std::printf("accepted %ld rejected %ld\n", accepted, rejected);
    std::printf("cases %ld\n", cases);
    std::printf("wrong %ld\n", wrong);
    return wrong ? 1 : 0;
}
