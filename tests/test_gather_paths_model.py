"""CPU: the model and corpus of tests/_gather_paths_model.py (what tests/test_gpu_warp_paths.py, test_gpu_mesh_paths.py and
test_gpu_ha_paths.py hold the path census of krgb_warp, krgb_mesh and krgb_ha against).

  * the model's windows, narrow flags, tap bounds, positions and tile constants are the real headers' (tests/cpp/gather_paths_plan.cpp
    prints what csrc/mcraw_warp_args.h, mcraw_mesh_args.h and mcraw_ha_args.h make of every tile of the corpus; host code only, a
    program of its own under ASan and UBSan), and its positions and choices are the numpy statements' (_warp_ref, _mesh_ref, _ha_ref);
  * the identities of a unit: staged pieces = (2 np + 4)(ne + 2) (krgb_ha: HA_STAGE_ITEMS), phase-A items = 2 np ne, gather lanes
    with pixels = the tile's rows x ceil(columns / 4), the outcomes of a ha_pick site add up to its sites, store pieces = the
    output's row pieces, and the walk counters as in tests/test_rgb_paths_model.py;
  * every new counter is driven above zero by the cases DRIVEN (or DRIVEN_CAPPED) names for it, or is in ARGUED_ZERO with its
    argument, and then zero over the whole corpus;
  * the corpus holds what it was made for."""
import os
import subprocess

import numpy as np
import pytest

import _gather_paths_model as G
import _ha_ref as HA
import _mesh_ref as MR
import _rgb_paths_model as T
import _warp_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "motioncam_decoder_amd", "csrc")
KERNELS = ("warp", "mesh", "ha")


def _tiles(S):
    P = G.plan(S)
    Ho, Wo = S["size"]
    for f in range(S["n"]):
        for u in range(P["units"]):
            ty, tx = u // P["tilesX"], u % P["tilesX"]
            i0, k0 = 32 * ty, 32 * tx
            yield f, ty, tx, i0, min(i0 + 32, Ho) - 1, k0, min(k0 + 32, Wo) - 1


def test_windows_are_the_headers(tmp_path):
    exe = str(tmp_path / "gather_paths_plan")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + CSRC, "-I" + os.path.join(ROOT, "include"), "-o", exe, os.path.join(ROOT, "tests", "cpp", "gather_paths_plan.cpp")], check=True)
    lines, want = ["h"], [None]
    rng = np.random.default_rng(7)
    for kernel in ("warp", "mesh"):
        for S in G.cases(kernel).values():
            geo = G.geometry(S)
            for f, ty, tx, i0, i1, k0, k1 in _tiles(S):
                (pb, eb, npp, nee), (ny, nx) = G.tile_window(S, geo, f, ty, tx)
                if kernel == "warp":
                    lines.append("w %s %d %d %d %d" % (" ".join(str(int(v)) for v in geo[f if len(geo) > 1 else 0]), i0, i1, k0, k1))
                    want.append([pb, eb, npp, nee])
                    continue
                cy, cx = G.mesh_cell(geo[f if len(geo) > 1 else 0], ty, tx)
                lines.append("m %s %s %d %d %d %d" % (" ".join(map(str, cy)), " ".join(map(str, cx)), i1 - i0, k1 - k0, S["W"], S["H"]))
                want.append([pb, eb, npp, nee, int(ny), int(nx), *G.mesh_tap_max(npp, nee), int(npp <= G.MESH_NP and nee <= G.MESH_NE)])
                for c, side in ((cy, S["H"]), (cx, S["W"])):  # positions: both forms of the sum equal the 64-bit statement
                    u, v = int(rng.integers(0, i1 - i0 + 1)), int(rng.integers(0, 32))
                    raw = G.mesh_lerp64(c, u, v)
                    lines.append("l %s %d %d %d" % (" ".join(map(str, c)), u, v, side))
                    want.append([raw, G.mesh_clamp(raw, side), raw, G.mesh_clamp(raw, side)])
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr.strip(), (r.stdout[-2000:], r.stderr[-3000:])
    out = [[int(v) for v in ln.split()] for ln in r.stdout.strip().splitlines()]
    assert len(out) == len(lines)
    head = [G.WARP_TW, G.WARP_TH, G.WARP_EROWS, G.WARP_ECOLS, G.MESH_NP, G.MESH_NE, G.MHC_TW, G.MHC_TH, G.HA_RAWW, G.HA_RAWH, G.HA_RAWCH, G.HA_GH,
            G.HA_STAGE_ITEMS, G.HA_G_MAIN, G.HA_G_EDGE]
    for Sh in range(4):
        head += [G.ha_rb_xpar(0, Sh), G.ha_rb_xpar(1, Sh)] + [G.ha_edge_rawcol(Q, Sh) for Q in range(G.HA_GH)]
    assert out[0] == head
    for ln, got, exp in zip(lines[1:], out[1:], want[1:]):
        assert got == exp, (ln, got, exp)
    assert sum(1 for ln in lines if ln[0] == "m") > 100 and sum(1 for ln in lines if ln[0] == "w") > 100


def test_positions_and_choices_are_the_numpy_statements():
    for S in G.cases("mesh").values():  # the windows and the per-pixel clamps of every real pixel, against _mesh_ref
        geo = G.geometry(S)
        for f in range(len(geo)):
            Y, X = MR.positions(geo[f], S["size"], S["H"], S["W"])
            pb, eb, npp, nee = MR.windows(Y, X)
            for _, ty, tx, i0, i1, k0, k1 in (t for t in _tiles(S) if t[0] == f):
                assert G.tile_window(S, geo, f, ty, tx)[0] == (pb[i0, k0], eb[i0, k0], npp[i0, k0], nee[i0, k0])
            Yr, Xr = MR.raw_positions(geo[f], S["size"])
            m = G.model("mesh", S["name"])
            if len(geo) == 1:  # (one mesh for the batch; no pixel past a tile's last column leaves the frame in these cases)
                assert m["mesh_y_lo"] == S["n"] * int((Yr < 0).sum()) == 0 and m["mesh_x_hi"] == 0
    for S in G.cases("warp").values():
        geo = G.geometry(S)
        for f, ty, tx, i0, i1, k0, k1 in _tiles(S):
            m = geo[f if len(geo) > 1 else 0]
            Y, X = W.positions(m, S["size"])
            assert G.warp_pos([int(v) for v in m], i1, k0) == (Y[i1, k0], X[i1, k0])
    for i in (-3, -1, 0, 5, 7, 8, 10):
        assert G.reflect101(i, 8) == np.pad(np.arange(8), 3, mode="reflect")[i + 3]
    assert G.reflect101(-9, 8) == 5 and G.reflect101(-20, 8) == 0 and G.reflect101(40, 8) == 0  # further out: folded twice, then clamped into the row
    S = next(iter(G.cases("ha").values()))
    for f in range(S["n"]):  # the banded image makes every choice occur, in every frame
        gw, dw = HA.ways(G.images(S["img"])[f], S["black"], "rggb")
        assert min(gw) >= 8 and min(dw) >= 8


@pytest.mark.parametrize("kernel", KERNELS)
def test_identities(kernel):
    for name, S in G.cases(kernel).items():
        P, m = G.plan(S), G.model(kernel, name)
        total = P["units"] * S["n"]
        assert m["wg_" + kernel] == m["first_" + kernel] == total and m["later_" + kernel] == 0  # (no cap, no resident limit)
        pieces = sum(v for k, v in m.items() if k.startswith("st_"))
        rowp = S["n"] * P["Ho"] * ((P["Wo"] + 7) // 8)
        if G.is_yuv(S):
            assert pieces == rowp + rowp // 2
        elif S["kind"][-3:] == "hwc":
            assert pieces == rowp
        else:
            assert pieces == 3 * rowp
        g1 = G.model(kernel, name, "grid1") if not G.is_float(S) else None
        if g1:
            nl = len(G.launches(S))
            assert g1["wg_" + kernel] == nl and g1["later_" + kernel] == total - nl and g1["cross_" + kernel] == S["n"] - nl
            assert {k: v for k, v in g1.items() if k.split("_")[0] not in T.WALK} == {k: v for k, v in m.items() if k.split("_")[0] not in T.WALK}
        if kernel == "ha":
            assert m["ha_ld_vec"] + m["ha_ld_elem"] == total * G.HA_STAGE_ITEMS
            assert m["ha_main_a"] + m["ha_main_b"] + m["ha_main_eq"] == total * 8 * G.HA_G_MAIN
            assert m["ha_edge_a"] + m["ha_edge_b"] + m["ha_edge_eq"] == total * G.HA_G_EDGE
            assert m["ha_diag_a"] + m["ha_diag_b"] + m["ha_diag_eq"] == S["n"] * S["H"] * S["W"] // 2  # the frame's R / B sites
            assert m["ha_continue"] == S["n"] * (P["units"] * 256 - P["Ho"] // 32 * 8 * ((S["W"] + 7) // 8) - (8 * ((S["W"] + 7) // 8) if S["H"] % 32 else 0))
            continue
        geo = G.geometry(S)
        staged = items = lanes = 0
        for f, ty, tx, i0, i1, k0, k1 in _tiles(S):
            (_, _, npp, nee), _ = G.tile_window(S, geo, f, ty, tx)
            npp, nee = min(npp, G.MESH_NP), min(nee, G.MESH_NE)
            staged += (2 * npp + 4) * (nee + 2)
            items += npp * nee
            lanes += (i1 - i0 + 1) * ((k1 - k0) // 4 + 1)
        assert m[kernel + "_ld_vec"] + m[kernel + "_ld_elem"] == staged
        assert m[kernel + "_a_even"] == m[kernel + "_a_odd"] == items
        assert m[kernel + "_pix"] == lanes and m[kernel + "_pix"] + m[kernel + "_nopix"] == total * 256
        assert 4 * lanes >= S["n"] * P["Ho"] * P["Wo"] > 4 * lanes - 3 * S["n"] * P["Ho"] * P["tilesX"]  # Ho x Wo x frames pixels, and the dropped ones
        rows = 2 if G.is_yuv(S) else 1
        busy = total * 256 - m[kernel + "_st_idle_ly"] - m[kernel + "_st_idle_x"] - m[kernel + "_st_idle_row"]
        assert busy == S["n"] * (P["Ho"] // rows) * ((P["Wo"] + 7) // 8)
        if kernel == "mesh":
            assert m["mesh_narrow"] + m["mesh_wide"] == total


def test_every_counter_is_driven_or_argued_zero():
    assert set(G.DRIVEN) == set(G.NEW) and set(G.ARGUED_ZERO) <= set(G.NEW) and set(G.DRIVEN_CAPPED) <= set(G.NEW)
    old = [k for k in T.PATHS if k not in G.NEW]
    assert old == [k for k in T.PATHS if T.DRIVEN[k] or T.DRIVEN_CAPPED.get(k)]  # the five older kernels' counters stay theirs
    for k in G.NEW:
        assert bool(G.DRIVEN[k] or G.DRIVEN_CAPPED.get(k)) != (k in G.ARGUED_ZERO), k
    for kernel in KERNELS:
        for name, S in G.cases(kernel).items():
            m = G.model(kernel, name)
            for k in T.PATHS:  # a case counts in its own kernel's counters, the LUT's place and the store forms alone
                mine = k in G.NEW and kernel in k.split("_") or k.startswith(("st_", "lut_"))
                assert mine or m[k] == 0, (name, k)
            for k, names in G.DRIVEN.items():
                assert m[k] > 0 or (kernel, name) not in names, (name, k)
            for k in G.ARGUED_ZERO:
                assert m[k] == 0, (name, k)
            for variant in ("grid1", "grid3"):
                for k, names in G.DRIVEN_CAPPED.items():
                    assert (kernel, name) not in names or G.model(kernel, name, variant)[k] > 0, (variant, name, k)


def test_corpus_holds_what_it_was_made_for():
    for kernel in KERNELS:
        C = list(G.cases(kernel).values())
        lut = [S for S in C if not G.is_float(S)]
        main = C[:8 if kernel == "ha" else 16]
        assert all(S["n"] == 3 and S["in_align"] == 0 and S["out_off"] == 0 and G.plan(S)["units"] == 6 for S in main)
        assert {S["cfa"] for S in main} == set(T.CFAS) and {S["kind"] for S in main} == {"u8hwc", "u16chw", "nv12", "p010"}
        assert {S["lutn"] for S in main} == {4096, 65536}
        assert {S["in_align"] for S in lut} == {0, 1, 2} and {S["out_off"] == 0 for S in lut} == {True, False}
        assert {S["kind"] for S in C if G.is_float(S)} == set(T.FLOAT_KINDS)
        many = [S for S in lut if S["n"] > T.RGB_MAXF]
        assert len(many) == 1 and G.launches(many[0]) == [32, 2] and G.plan(many[0])["units"] == 1
        assert all(G.plan(S)["units"] * S["n"] <= 40 and S["H"] * S["W"] <= 21000 for S in C)  # a few dozen units, a few thousand pixels
        if kernel == "ha":
            assert main[0]["H"] % 32 == 8 and main[0]["W"] % 256 == 8
            continue
        assert {S["filt"] for S in main} == {"linear", "cubic"} and main[0]["size"] == (40, 70)
        assert {S["geo"] for S in C} >= {"main", "edges", "tiny", "one"}
        tiny = [S for S in C if S["geo"] == "tiny"][0]
        assert (tiny["H"], tiny["W"], tiny["size"]) == (8, 8, (2, 2))
        edges = [S for S in C if S["geo"] == "edges" and S["n"] == 3][0]
        geo = G.geometry(edges)
        wins = [G.tile_window(edges, geo, f, ty, tx)[0] for f, ty, tx, *_ in _tiles(edges)]
        assert min(w[0] for w in wins) < 0 and min(w[1] for w in wins) < 0  # over the first row and the first column
        assert max(w[0] + 2 * w[2] for w in wins) > edges["H"] and max(w[1] + 8 * w[3] for w in wins) > edges["W"]  # ... the last ones
    wide = [S for S in G.cases("mesh").values() if S["geo"] == "wide"][0]
    geo = G.geometry(wide)
    flags = {G.tile_window(wide, geo, f, ty, tx)[1] for f, ty, tx, *_ in _tiles(wide)}
    assert (False, True) in flags and (True, False) in flags and (True, True) in flags
    assert not MR.in_regime(G.geometry(list(G.cases("mesh").values())[0])[2], (40, 70), 72, 136)  # the hostile mesh
