"""CPU: the model and corpus of tests/_tiles7_model.py (what tests/test_gpu_k7t_paths.py holds k7_tiles' path census against).

  * the model's view of every corpus frame -- bit widths and references parsed from the side streams, the payload unpacked block by
    block in numpy -- decodes to the oracle's pixels;
  * every counter of the census is driven above zero by the corpus in the settings named for it (DRIVEN), and DRIVEN names every counter;
  * every frame made to be not lean for one reason fails that reason ALONE in its setting, and the natural frames are lean throughout;
  * the corpus holds what it was made for: all 17 x 17 pairs of bit widths at both sibling positions, a full span at head 8, ...;
  * the five builds of build.K7T_PATH_VARIANTS compile and link (cross-compiled: no GPU needed), and only mcraw_type7.hip is
    compiled for them."""
import os

import numpy as np
import pytest

import _tiles7_model as T
from motioncam_decoder_amd import build as B


def test_model_decodes_to_the_oracles_pixels():
    for f, (ret, rows) in zip(T.corpus(), T.expectations()):
        got = T.decode_np(f["buf"], f["w"], f["h"])
        assert ret == got.size and np.array_equal(got, rows), f["name"]
        if "wrap" not in f["tags"]:
            assert np.array_equal(got, f["img"][:got.shape[0]]), f["name"]


def test_paths_and_driven_name_the_same_counters():
    assert sorted(T.DRIVEN) == sorted(T.PATHS) and len(set(T.PATHS)) == len(T.PATHS)
    for k, settings in T.DRIVEN.items():
        assert settings and all(s in T.SETTINGS for s in settings), k


@pytest.mark.parametrize("setting", list(T.SETTINGS))
def test_corpus_drives_every_counter(setting):
    m = T.model(setting)
    assert sorted(m) == sorted(T.PATHS)
    for k, settings in T.DRIVEN.items():
        if setting in settings:
            assert m[k] > 0, (setting, k, m)
    kind = T.stage_of(setting)[0]
    if kind not in (10, 12, 14):  # (only the strip instances decide about lean)
        assert all(m[k] == 0 for k in T.FAILS + ("lean", "notlean")), m
    if kind != 14:
        assert all(m[k] == 0 for k in ("st_merged_fwd", "st_merged_back", "decl_partial", "decl_notin")), m
    # every piece of every tile of a valid item goes exactly one way
    C = T.corpus()
    pieces = sum(T.parse(C[i]["buf"]).nblk // 4 * 32 for b in T.batches(setting) for i in b)
    assert sum(m[k] for k in ("drop_y", "drop_x", "st_aligned", "st_unaligned", "st_cropped", "st_merged_fwd", "st_merged_back")) == pieces
    assert sum(m["cls%d" % c] for c in range(10)) * 8 == pieces


def test_the_forcing_builds_move_the_counts_as_they_should():
    for setting in ("p14", "p14 black", "p12", "plain", "f16 planes clip"):
        m = T.model(setting)
        n = T.model(setting, "nolean")
        assert n["lean"] == 0 and n["notlean"] == m["lean"] + m["notlean"]
        s = T.model(setting, "slowstore")
        assert s["st_aligned"] == 0 and s["st_merged_fwd"] == s["st_merged_back"] == 0
        assert s["st_unaligned"] == m["st_aligned"] + m["st_unaligned"] + m["st_merged_fwd"] + m["st_merged_back"]
        g = T.model(setting, "nomerge")
        assert g["st_merged_fwd"] == g["st_merged_back"] == g["decl_partial"] == g["decl_notin"] == 0
        assert g["st_aligned"] == m["st_aligned"] + m["st_merged_fwd"] + m["st_merged_back"]


def test_each_lean_frame_fails_for_its_reason_alone():
    rep = T.alone_report()
    assert sorted(rep) == sorted(T.LEAN_ALONE)
    for name, (setting, reason) in T.LEAN_ALONE.items():
        c = rep[name]
        assert c[reason] > 0 and c["lean"] == 0 and c["notlean"] == c[reason], (name, c)  # (every item of the frame, for that reason)
        assert all(c[k] == 0 for k in T.FAILS if k != reason), (name, c)
    C = {f["name"]: f for f in T.corpus()}
    for name, settings in (("lean natural", ("p12", "p14")), ("lean natural above black", ("p12 black", "p10 black", "p14 black"))):
        for setting in settings:
            kind, black, planes = T.stage_of(setting)
            c = T.frame_census(C[name], kind, black, planes, 0, "census")
            assert c["lean"] == 2 and c["notlean"] == 0, (name, setting, c)


def test_corpus_holds_what_it_was_made_for():
    C = {f["name"]: f for f in T.corpus()}
    P = T.parse(C["pairs"]["buf"])
    tiles = P.bits.reshape(-1, 4)
    for pos in (0, 2):
        assert {(int(a), int(b)) for a, b in tiles[:, pos:pos + 2]} == {(a, b) for a in range(17) for b in range(17)}
    # residuals that use the width to the full, so a field mask one bit short shows
    assert all(int(P.res[i].max()) == (1 << int(b)) - 1 for i, b in enumerate(P.bits))
    c = T.frame_census(C["span full"], 0, None, False, 0, "census")
    assert c["span_full"] == 1 and c["head"] == 1
    c = T.frame_census(C["span empty"], 0, None, False, 0, "census")
    assert c["span_empty"] == 2 and c["cls0"] == 64
    c = T.frame_census(C["wrap"], 0, None, False, 0, "census")
    assert c["wrap_lanes"] > 0
    ret, rows = T.expectations()[[f["name"] for f in T.corpus()].index("wrap")]
    assert not np.array_equal(rows, C["wrap"]["img"])  # (the oracle wraps: the frame no longer is the image it was coded from)
    assert sorted(T.ngroups_planned(f["w"], f["h"]) for f in T.corpus() if "mixed" in f["tags"]) == [4, 4, 5]
    assert [len(m) for m, _ in T.size_classes([4, 5, 4])] == [3]
    # the merged store's neighbours: every number of tile columns from one to nine
    assert {T.parse(f["buf"]).tilesX for f in T.corpus()} >= set(range(1, 10))
    assert sum(f["w"] * f["h"] for f in T.corpus()) < 500000


@pytest.mark.parametrize("variant", list(B.K7T_PATH_VARIANTS))
def test_variant_compiles_and_links(variant, tmp_path, capfd):
    flags = B.K7T_PATH_VARIANTS[variant]
    assert flags in list(B.TEST_VARIANTS)
    out = B.build_variant(str(tmp_path / ("libmcraw_k7t_%s.so" % variant)), flags)
    assert os.path.getsize(out) > 0
    # the switches are known to mcraw_type7.hip alone: nothing else is compiled for a variant
    compiled = [ln for ln in capfd.readouterr().out.splitlines() if " -c " in ln]
    assert all(ln.endswith("mcraw_type7.hip") for ln in compiled), compiled
    import subprocess
    syms = subprocess.run(["nm", "-D", "--defined-only", out], capture_output=True, text=True, check=True).stdout
    assert "mcraw_diag_k7t_paths" in syms
