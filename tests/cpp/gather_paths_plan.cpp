// gather_paths_plan.cpp -- what the real headers (csrc/mcraw_warp_args.h, mcraw_mesh_args.h, mcraw_ha_args.h: no HIP) make of the
// tiles of tests/_gather_paths_model.py's corpus, for tests/test_gather_paths_model.py to compare with the model's own.  One query
// per line of standard input, one line of numbers per query:
//   w m0 .. m5 i0 i1 k0 k1            warp_window:  pb eb np ne
//   m cy0 .. cy3 cx0 .. cx3 u1 v1 W H mesh_window, mesh_narrow (Y, X), mesh_tap_max_row / _col, mesh_in_regime:  pb eb np ne ny nx rmax cmax regime
//   l c0 .. c3 u v side               mesh_lerp64, its clamp, and (a narrow cell) mesh_row32 / mesh_lerp32 / mesh_clamp32:  raw clamped raw32 clamped32
//   h                                 the constants of the three tiles, then ha_rb_xpar(ypar, S) and ha_edge_rawcol(Q, S) for every S
#include <cstdio>

#include "mcraw_ha_args.h"
#include "mcraw_mesh_args.h"

using namespace mcraw;

int main()
{
    char kind;
    while (std::scanf(" %c", &kind) == 1) {
        if (kind == 'w') {
            int32_t m[6];
            unsigned i0, i1, k0, k1;
            if (std::scanf("%d %d %d %d %d %d %u %u %u %u", &m[0], &m[1], &m[2], &m[3], &m[4], &m[5], &i0, &i1, &k0, &k1) != 10)
                return 2;
            const WarpWin w = warp_window(m, i0, i1, k0, k1);
            std::printf("%d %d %u %u\n", w.pb, w.eb, w.np, w.ne);
        } else if (kind == 'm') {
            int32_t cy[4], cx[4];
            unsigned u1, v1;
            int W, H;
            if (std::scanf("%d %d %d %d %d %d %d %d %u %u %d %d", &cy[0], &cy[1], &cy[2], &cy[3], &cx[0], &cx[1], &cx[2], &cx[3], &u1, &v1, &W, &H) != 12)
                return 2;
            const WarpWin w = mesh_window(cy, cx, u1, v1, W, H);
            std::printf("%d %d %u %u %d %d %d %d %d\n", w.pb, w.eb, w.np, w.ne, mesh_narrow(cy) ? 1 : 0, mesh_narrow(cx) ? 1 : 0, mesh_tap_max_row(w.np),
                        mesh_tap_max_col(w.ne), mesh_in_regime(w) ? 1 : 0);
        } else if (kind == 'l') {
            int32_t c[4];
            unsigned u, v;
            int side;
            if (std::scanf("%d %d %d %d %u %u %d", &c[0], &c[1], &c[2], &c[3], &u, &v, &side) != 7)
                return 2;
            const int64_t raw = mesh_lerp64(c, u, v);
            long long raw32 = raw, cl32 = mesh_clamp(raw, side);
            if (mesh_narrow(c)) {
                int32_t l, r;
                mesh_row32(c, u, l, r);
                raw32 = mesh_lerp32(c[0], l, r, v);
                cl32 = mesh_clamp32(static_cast<int32_t>(raw32), side);
            }
            std::printf("%lld %lld %lld %lld\n", static_cast<long long>(raw), static_cast<long long>(mesh_clamp(raw, side)), raw32, cl32);
        } else if (kind == 'h') {
            std::printf("%u %u %u %u %u %u %u %u %u %u %u %u %u %u %u", WARP_TW, WARP_TH, WARP_EROWS, WARP_ECOLS, MESH_NP, MESH_NE, MHC_TW, MHC_TH, HA_RAWW,
                        HA_RAWH, HA_RAWCH, HA_GH, HA_STAGE_ITEMS, HA_G_MAIN, HA_G_EDGE);
            for (uint32_t S = 0; S < 4u; S++) {
                std::printf(" %u %u", ha_rb_xpar(0u, S), ha_rb_xpar(1u, S));
                for (uint32_t Q = 0; Q < HA_GH; Q++)
                    std::printf(" %u", ha_edge_rawcol(Q, S));
            }
            std::printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}
