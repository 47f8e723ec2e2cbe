"""CPU: the model of the mosaic stages' path census (tests/_mosaic_paths_model.py) against itself, before any GPU time is spent on
it (tests/test_gpu_mosaic_paths.py): the identities that hold between its counters whatever the setting, that every counter of
DRIVEN is above zero in the settings named for it, what the forced variants must show, and the count of the div_round sweep."""
import os
import re

import numpy as np
import pytest

import _mosaic_paths_model as T

STAGED = {"fixpix": 2, "denoise": None, "hl_apply": 1, "hl_measure": 1}  # family -> halo (denoise: 2 * radius)


@pytest.fixture(scope="module")
def models():
    return {v: {name: T.model(name, v) for name in T.SETTINGS} for v in T.VARIANTS + T.EXTRA_VARIANTS}


def _pieces(S):
    return T.FRAMES * S["H"] * ((S["W"] + 7) // 8)


@pytest.mark.parametrize("variant", T.VARIANTS + T.EXTRA_VARIANTS)
def test_identities(models, variant):
    for name, S in T.SETTINGS.items():
        c, fam, H, W = models[variant][name], S["family"], S["H"], S["W"]
        assert sorted(k for k in c if not k.startswith("_")) == sorted(T.PATHS)
        assert all(c[k] >= 0 for k in T.PATHS) and c["div_down"] == c["div_up"] == 0, name
        tilesx = (W + 255) // 256
        if fam in ("merge", "merge_cells"):
            P = T.merge_plan(S, variant)
            LH, bases = P["TH"] + 2, range(S["first"], S["first"] + S["count"])
            before, after = T.MG_WINDOWS[S["window"]]
            units = P["tiles"] * S["count"]
            assert c["wg"] - c["mg_short"] == units and 0 <= c["mg_short"] < 8 * c["mg_launch"], name
            assert c["mg_launch"] == len(P["launches"]) == ((S["count"] + 2) // 3 if variant == "pieces" else 1), name
            # members staged + skipped + the base itself = the windows' sizes, per tile
            windows = sum(min(T.MG_FRAMES - 1, b + after) - max(0, b - before) + 1 for b in bases)
            assert c["mg_self"] == units and c["mg_self"] + c["mg_zerow"] + c["mg_staged"] == P["tiles"] * windows, name
            assert c["mg_m_aligned"] + c["mg_m_sx"] + c["mg_m_invec"] == c["mg_staged"], name
            assert c["mg_zerow"] == 0 or (variant not in ("slow", "poisonslow") and S["pos"] != "none"), name
            # every chunk of s_b and of every staged s_m is written: as a piece of the frame or as 0
            chunks = c["stg_vec"] + c["stg_unal"] + c["stg_halo"] + c["stg_crop"] + c["mg_zero"]
            assert chunks == (units + c["mg_staged"]) * LH * T.TILE_CH and c["stg_skip"] == 0 and c["mg_cut"] <= c["stg_crop"], name
            assert (c["stg_vec"] == 0) if not T.on_grid(S) else (c["stg_unal"] == 0 or c["mg_m_sx"] > 0), name
            stores = c["st_vec"] + c["st_unal"] + c["st_elem"]
            assert stores == S["count"] * H * ((W + 7) // 8) and c["div_calls"] == 8 * stores and c["row_cont"] == 0, name
            assert c["idle_lane"] % 8 == 0 and c["row_break"] <= units * 256 - c["idle_lane"], name
            assert c["st_elem"] == (S["count"] * H if W % 8 else 0), name
            continue
        if fam == "stats":
            P = T.stats_plan(S, variant)
            assert c["wg"] == T.FRAMES * P["wgs"] and c["wg"] + c["ss_prefetch"] == T.FRAMES * P["tiles"], name
            assert P["tpc"] <= (2 if variant == "pieces" else 64) and (P["wgs"] - 1) * P["tpc"] < P["tiles"] <= P["wgs"] * P["tpc"], name
            # per tile 4 waves, each full, partial or empty; per tile 512 lane rows, each loaded whole, at an edge, or outside
            assert c["ss_full"] + c["ss_partial"] + c["ss_empty"] == 4 * T.FRAMES * P["tiles"], name
            assert c["ld_vec"] + c["ld_unal"] + c["ss_ld_edge"] + c["ss_row_out"] == 512 * T.FRAMES * P["tiles"] and c["ld_elem"] == 0, name
            y0, x0, h, w = T.stats_roi(S)
            assert c["ld_vec"] + c["ld_unal"] + c["ss_ld_edge"] >= T.FRAMES * h * ((w + 7) // 8), name
            assert c["ss_onebin"] <= 4 * c["ss_full"] and (c["ss_onebin"] == 4 * c["ss_full"] or S["content"] == "noise"), name
            assert (c["ss_full"] == 0) if variant in ("slow", "poisonslow") else (c["ss_full"] > 0) == (w >= 256 + (x0 - P["xa"]) and h >= 4), name
            assert not any(c[k] for k in T.PATHS if k.startswith(("st_", "stg_", "row_", "idle"))), name
        elif fam in STAGED:
            TH = T.tile_heights(variant)[fam]
            halo = 2 * S["radius"] if fam == "denoise" else STAGED[fam]
            assert c["wg"] == T.FRAMES * tilesx * ((H + TH - 1) // TH), name
            # pieces staged + skipped = chunks
            staged = c["stg_vec"] + c["stg_unal"] + c["stg_halo"] + c["stg_crop"]
            assert staged + c["stg_skip"] == c["wg"] * (TH + 2 * halo) * T.TILE_CH, name
            # every sample of the frame and of its halo is staged once per tile row that holds it: at least the frame's own chunks
            assert staged >= T.FRAMES * H * ((W + 7) // 8), name
            assert (c["stg_vec"] == 0) if not T.on_grid(S) else (c["stg_unal"] == 0), name
            assert c["ld_vec"] + c["ld_unal"] + c["ld_elem"] == 0, name
            # lane rows: run (a store each, but khl_measure) + passed over, or left by a break
            stores = c["st_vec"] + c["st_unal"] + c["st_elem"]
            assert stores == (0 if fam == "hl_measure" else _pieces(S)), name
            if fam != "denoise":
                assert _pieces(S) + c["row_cont"] + c["idle_lane"] // 8 * TH == c["wg"] * TH * 32 and c["row_break"] == 0, name
            else:
                assert c["row_cont"] == 0 and c["div_calls"] == 8 * stores, name
                assert c["row_break"] <= c["wg"] * 256 - c["idle_lane"], name
        else:
            assert c["wg"] == T.FRAMES * tilesx * ((H + 15) // 16), name
            assert c["st_vec"] + c["st_unal"] + c["st_elem"] == _pieces(S), name
            assert (c["ld_vec"], c["ld_unal"], c["ld_elem"]) == (c["st_vec"], c["st_unal"], c["st_elem"]), name
            assert _pieces(S) + c["row_cont"] + c["idle_lane"] // 8 * 16 == c["wg"] * 16 * 32, name
            assert c["stg_vec"] + c["stg_unal"] + c["stg_halo"] + c["stg_crop"] + c["stg_skip"] == 0, name
        assert c["st_elem"] == (T.FRAMES * H if W % 8 and fam not in ("hl_measure", "stats") else 0), name
        assert fam == "stats" or not any(c[k] for k in T.PATHS if k.startswith("ss_")), name
        rng = c["_unstaged"]
        if fam == "fixpix":
            TH = T.tile_heights(variant)[fam]
            waves = T.FRAMES * tilesx * sum((min(TH, H - y0) + 1) // 2 for y0 in range(0, H, TH))
            assert c["fp_wave_any"] + c["fp_wave_none"] == waves, name
            assert rng.get("fp_wave_any", (0, 0))[1] == -rng.get("fp_wave_none", (0, 0))[0], name
            assert c["fp_wave_any"] <= c["fp_cand"] <= _pieces(S), name
            assert c["fp_flag"] <= c["fp_hot"] + c["fp_cold"] <= 2 * c["fp_flag"] and c["fp_listed"] <= c["fp_hot"] + c["fp_cold"], name
            lst = T.fix_list(name)
            if lst is None:
                assert c["fl_wg"] + c["fl_past"] + c["fl_outside"] + c["fl_written"] + c["fl_nopair"] + c["fp_listed"] == 0, name
            else:  # members written + without a pair + outside = the list, per frame
                assert c["fl_wg"] * 256 == c["fl_past"] + T.FRAMES * len(lst), name
                assert c["fl_outside"] + c["fl_written"] + c["fl_nopair"] == T.FRAMES * len(lst), name
        else:
            assert not any(c[k] for k in T.PATHS if k.startswith(("fp_", "fl_"))), name
        if fam == "hl_apply":
            assert c["hl_clipped"] + c["hl_unclipped"] == _pieces(S), name
            sat = T.HR.by_position(T.HL_SAT, H, W)
            assert c["hl_rebuilt"] + c["hl_left"] == int((T.images(name) >= sat).sum()) and c["hl_top"] <= c["hl_rebuilt"], name
        if fam == "hl_measure":
            assert c["hm_measured"] + c["hm_own"] + c["hm_neighbour"] == T.FRAMES * H * W, name
        if fam == "denoise" and S["radius"] == 2:
            assert c["dn_sy3"] <= min(c["dn_sy1"], c["dn_sy2"]) and (c["dn_both"] > 0) == (W in (5, 6, 7)) and (c["dn_sy3"] > 0) == (H in (5, 6, 7)), name
        elif fam != "denoise" or S["radius"] == 1:
            assert not any(c[k] for k in T.PATHS if k.startswith("dn_")), name
        # the ranges: none where LDS is poisoned or the predicate is forced, and only on the predicates' own counters
        assert set(rng) <= {"fp_cand", "fp_wave_any", "fp_wave_none", "hl_clipped", "hl_unclipped"}, name
        if variant not in ("census", "th16", "pieces", "frames2"):
            assert (not rng and c["_unstaged_rows"] == 0) or variant == "slow", name
        if variant in ("slow", "poisonslow"):
            assert not rng and c["fp_wave_none"] == 0 and c["hl_unclipped"] == 0, name


def test_driven(models):
    """Every counter but div_round's steps is driven, and above zero in the settings named for it (at its lowest, where it has a range)."""
    assert sorted(T.DRIVEN) == sorted(k for k in T.PATHS if k not in T.UNMODELLED)
    for k, names in T.DRIVEN.items():
        assert names, k
        for name in names:
            assert name in T.SETTINGS, (k, name)
            c = models["census"][name]
            assert c[k] + c["_unstaged"].get(k, (0, 0))[0] > 0, (k, name)


def test_unstaged_lanes_exist(models):
    """The corpus has lane rows whose `cand` reads chunks that staging leaves as they are (widths with a cropped row end of at most 6
    columns), and the poisoned builds decide every one of them."""
    rows = sum(c["_unstaged_rows"] for c in models["census"].values())
    assert rows > 0
    assert any(c["_unstaged"] for n, c in models["census"].items() if T.SETTINGS[n]["family"] == "fixpix")
    assert all(not c["_unstaged"] for c in models["poison"].values())


def test_variants_differ_where_they_should(models):
    name = "fixpix/35x520/grid/noise/counts=1/list=0/rank=2"
    assert models["th16"][name]["wg"] == T.FRAMES * 3 * 3 and models["census"][name]["wg"] == T.FRAMES * 3 * 2
    mg = "merge/35x520/grid/noise/count=5/first=1/perlut=0/pos=big/support=0/window=1"
    assert models["census"][mg]["mg_launch"] == 1 and models["pieces"][mg]["mg_launch"] == 2 and models["th16"][mg]["wg"] > models["census"][mg]["wg"]
    assert models["slow"][mg]["mg_staged"] == models["census"][mg]["mg_staged"] + models["census"][mg]["mg_zerow"] > models["census"][mg]["mg_staged"]
    st = "stats/35x520/grid/noise/bins=4096/roi=0"  # 9 tiles: one workgroup of the product, five of two tiles at most
    assert models["census"][st]["wg"] == T.FRAMES and models["pieces"][st]["wg"] == 5 * T.FRAMES and models["pieces"][st]["ss_prefetch"] == 4 * T.FRAMES
    for k in ("fp_hot", "fp_cold", "fp_flag", "st_vec", "st_elem"):
        assert len({models[v][name][k] for v in T.VARIANTS}) == 1, k
    flat = "fixpix/35x520/grid/flat/counts=1/list=0/rank=2"
    assert models["census"][flat]["fp_cand"] == 0 < models["slow"][flat]["fp_cand"] == 3 * 35 * 65


def test_frames2_counts_what_census_counts(models):
    """Two frames a launch change no counter: no stage counts its launches, and kstats' plan gives every launch the same tiles per
    workgroup (stats_plan asserts it)."""
    for name in T.SETTINGS:
        assert models["frames2"][name] == models["census"][name], name


def test_views():
    grid = {n: T.on_grid(S) for n, S in T.SETTINGS.items()}
    assert not any(g for n, g in grid.items() if T.SETTINGS[n]["view"] != "grid")
    # (a frame of one row has the pitch W: 1x1 is off the grid in every view)
    assert all(g == ((S["H"], S["W"]) != (1, 1)) for (n, g), S in zip(grid.items(), T.SETTINGS.values()) if S["view"] == "grid")


def test_counters_and_switches_of_the_sources():
    """PATHS is the header's enum, in its order; the variants' switches occur in the stage sources alone and in no header, so a
    variant compiles those sources and nothing else."""
    from motioncam_decoder_amd import build as B
    text = open(os.path.join(B.CSRC, "mcraw_mosaic_paths.h")).read()
    enum = text[text.index("enum MosPath {"):text.index("MP_N\n};")]
    enum = "\n".join(ln.split("//")[0] for ln in enum.splitlines())
    assert [m.lower() for m in re.findall(r"MP_([A-Z0-9_]+)", enum)] == T.PATHS
    assert tuple(B.MOSAIC_PATH_VARIANTS) == T.VARIANTS and all(v in B.TEST_VARIANTS for v in B.MOSAIC_PATH_VARIANTS.values())
    stage = {"mcraw_shade.hip", "mcraw_stats.hip", "mcraw_fixpix.hip", "mcraw_denoise.hip", "mcraw_merge.hip", "mcraw_highlights.hip"}
    assert T.EXTRA_VARIANTS == ("frames2",) and B.MOSAIC_FRAMES2_FLAGS in B.TEST_VARIANTS and B.MOSAIC_FRAMES2_FLAGS[0] == "-DMCRAW_PATHSM"
    names = {re.sub(r"^-D([A-Za-z0-9_]+).*$", r"\1", f) for flags in list(B.MOSAIC_PATH_VARIANTS.values()) + [B.MOSAIC_FRAMES2_FLAGS] for f in flags}
    for n in sorted(names):
        for f in B.HIP_HEADERS + B.HIP_SOURCES:
            if re.search(r"\b%s\b" % n, open(os.path.join(B.CSRC, f)).read()):
                assert f in stage, (n, f)
    assert all(f[0] == "-DMCRAW_PATHSM" for f in B.MOSAIC_PATH_VARIANTS.values())


def test_div_sweep_count():
    for den in (1, 2, 3, 7, 255, 256, 6399, 6400, 16383, 16384, 16385, 20000):
        assert T.div_sweep_count([den]) == T.div_sweep_count_plain(den), den
    total = T.div_sweep_count()
    assert 5 * 6400 * 65536 < total <= 5 * 6400 * 65537
