"""CPU: the model and corpus of tests/_rgb_paths_model.py (what tests/test_gpu_rgb_paths.py holds the demosaic kernels' path census
against).

  * the model's plans of every corpus call are the real headers' (tests/cpp/rgb_paths_plan.cpp prints what rgb_check, area_check and
    resample_check of csrc/*_args.h make of the same calls; host code only, under ASan and UBSan);
  * every counter of the census is driven above zero by the corpus in the settings named for it (DRIVEN, and DRIVEN_CAPPED for the
    counters that only a capped grid reaches), and the two name every counter;
  * the walk: any grid of 1 .. units x frames workgroups takes every unit exactly once; one workgroup crosses frames - 1 times;
  * the corpus holds what it was made for: per kernel two unit columns and rows, a unit count that 3 divides and one that it does
    not, every instance with a LUT, both LUT homes, the three input alignments, outputs on and off their grid;
  * the five builds of build.RGB_PATH_VARIANTS compile and link (cross-compiled: no GPU needed), only the six demosaic sources
    are compiled for them, and the switches' names occur in those sources alone: the census and the poison in all six, the grid's
    cap in the three older ones (krgb_warp, krgb_mesh and krgb_ha take their limit from mcraw_rgb.hip).
The counters of krgb_warp, krgb_mesh and krgb_ha, the tail of PATHS: tests/test_gather_paths_model.py."""
import os
import re
import subprocess

import pytest

import _rgb_paths_model as T
from motioncam_decoder_amd import build as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "motioncam_decoder_amd", "csrc")
THREE = ("mcraw_rgb.hip", "mcraw_area.hip", "mcraw_resample.hip")
SIX = THREE + ("mcraw_warp.hip", "mcraw_mesh.hip", "mcraw_ha.hip")
WHERE = {"MCRAW_PATHSR": SIX, "MCRAW_POISON_RGB": SIX, "MCRAW_RGB_GRID_CAP": THREE}


def test_plans_are_the_headers(tmp_path):
    exe = str(tmp_path / "rgb_paths_plan")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "cpp", "rgb_paths_plan.cpp")], check=True)
    names, lines = [], []
    for name, S in T.SETTINGS.items():
        y0, x0, ch, cw = S.get("crop", (0, 0, 0, 0))
        ho, wo = S.get("size", (0, 0))
        fam = 0 if T.is_float(S) else 2 if T.is_yuv(S) else 1
        lines.append(" ".join(str(v) for v in (("mhc", "bin2", "area", "resample").index(S["kernel"]), fam, T.ES[S["kind"]], S["n"], S["W"], S["H"],
                                               S["pitch"], S["fstride"], S["off"], S["out_off"], y0, x0, ch, cw, ho, wo,
                                               T.RS.FILTER_CODE[S.get("filt", "linear")])))
        names.append(name)
    r = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and not r.stderr.strip(), (r.stdout[-3000:], r.stderr[-3000:])
    out = r.stdout.strip().splitlines()
    assert len(out) == len(names)
    for name, ln in zip(names, out):
        assert not ln.startswith("rejected"), (name, ln)
        real = {k: int(v) for k, v in (kv.split("=") for kv in ln.split())}
        mine = dict(T.plan(T.SETTINGS[name]), out_frame=T.out_frame_bytes(T.SETTINGS[name]))
        assert set(mine) <= set(real), (name, sorted(set(mine) - set(real)))
        for k, v in mine.items():
            assert real[k] == v, (name, k, real[k], v)


def test_every_counter_is_driven():
    import _gather_paths_model as G
    assert set(T.DRIVEN) == set(T.PATHS) and set(T.DRIVEN_CAPPED) <= set(T.PATHS)
    for k in T.PATHS:  # (krgb_warp's, krgb_mesh's and krgb_ha's counters: their own corpus, or the argued-zero list)
        assert T.DRIVEN[k] or T.DRIVEN_CAPPED.get(k) or G.DRIVEN.get(k) or G.DRIVEN_CAPPED.get(k) or k in G.ARGUED_ZERO, "no setting drives " + k
        assert not (T.DRIVEN[k] or T.DRIVEN_CAPPED.get(k)) or k not in G.NEW
    for name in T.SETTINGS:
        m = T.model(name)
        for k, names in T.DRIVEN.items():
            assert m[k] > 0 or name not in names, (name, k)
        assert sum(m.values()) > 0
    for variant in ("grid1", "grid3"):
        for k, names in T.DRIVEN_CAPPED.items():
            for name in names:
                assert T.model(name, variant)[k] > 0, (variant, name, k)


def test_walk():
    for units, nf in ((1, 1), (4, 5), (9, 5), (1, 32), (6, 2)):
        total = units * nf
        for grid in range(1, total + 1):
            taken = sorted(t for b in range(grid) for t in range(b, total, grid))
            assert taken == list(range(total))
            first, later, cross = T.walk(units, nf, grid)
            assert first == grid and first + later == total and cross <= later
        assert T.walk(units, nf, 1) == (1, total - 1, nf - 1)
        assert T.walk(units, nf, total) == (total, 0, 0)


def test_corpus_holds_what_it_was_made_for():
    lut = [S for S in T.SETTINGS.values() if not T.is_float(S)]
    five = [S for S in lut if S["n"] == 5]
    kinds_of = {"bin2": ("u8", "u16"), "bin2y": ("nv12", "p010")}
    for fam in T.FAMILIES:
        mine = [S for S in five if T.family(S) == fam]
        units = {T.plan(S)["units"] for S in mine}
        assert any(u % 3 == 0 for u in units) and any(u % 3 for u in units), (fam, units)
        for S in mine:
            P = T.plan(S)
            assert P["units"] * S["n"] <= 300, "no batch needs more than a few hundred units"
            if fam in ("mhc", "area", "res"):
                assert P["tilesX"] >= 2 and P["units"] // P["tilesX"] >= 2, (fam, P)
            else:  # units are runs of 256 items in row-major order: more than one, over more than one row
                assert P["units"] >= 2 and P["tilesX"] < T.RGB_T
            # a partial last piece of 8 columns, a partial last unit column and a partial last unit row
            assert P["Wo"] % 8
            if fam == "mhc":
                assert S["W"] % T.MHC_TW and S["H"] % T.MHC_TH
            elif fam == "area":
                assert P["Wo"] % (8 << P["lx_log2"]) and P["groups"] % T.AREA_BAND and (P["Ho"] + 1) // 2 % P["ly"] == 0
            elif fam == "res":
                assert P["Wo"] % T.RES_TW and P["Ho"] % (2 * P["ly"])
            else:
                assert (P["tilesX"] * (P["Ho"] // 2 if fam == "bin2y" else P["Ho"])) % T.RGB_T
        seen = {(S["kind"].replace("hwc", "").replace("chw", ""), S["cfa"]) for S in mine}
        assert seen == {(k, c) for k in kinds_of.get(fam, ("u8", "u16", "nv12", "p010")) for c in T.CFAS}, fam
        assert {S["lutn"] for S in mine} == {4096, 65536} and {S["in_align"] for S in mine} == {0, 1, 2}
        assert {S["out_off"] == 0 for S in mine} == {True, False}
        assert fam == "bin2y" or {S["kind"][-3:] for S in mine if S["kind"][0] == "u"} == {"hwc", "chw"}
    assert {T.area_mode(S) for S in five if S["kernel"] == "area"} == {0, 1, 2}
    tiny = [S for S in lut if S["n"] > T.RGB_MAXF]
    assert len(tiny) == 1 and T.launches(tiny[0]) == [32, 2] and T.plan(tiny[0])["units"] == 1
    gain, m = T.colours(five[0])
    assert len({tuple(g) for g in gain}) == 5 and len({tuple(x.ravel()) for x in m}) == 5
    assert sum(S["n"] * S["H"] * S["W"] for S in {(S["n"], S["H"], S["W"]): S for S in T.SETTINGS.values()}.values()) < 8000000


def test_switch_names_stay_in_the_six_sources():
    names = sorted({re.sub(r"^-D([A-Za-z0-9_]+).*$", r"\1", f) for flags in B.RGB_PATH_VARIANTS.values() for f in flags})
    assert names == ["MCRAW_PATHSR", "MCRAW_POISON_RGB", "MCRAW_RGB_GRID_CAP"]
    for f in sorted(os.listdir(CSRC)):
        text = open(os.path.join(CSRC, f)).read()
        for n in names:
            assert bool(re.search(r"\b%s\b" % n, text)) == (f in WHERE[n]), (f, n)


@pytest.mark.parametrize("variant", list(B.RGB_PATH_VARIANTS))
def test_variant_compiles_and_links(variant, tmp_path, capfd):
    flags = B.RGB_PATH_VARIANTS[variant]
    assert flags in list(B.TEST_VARIANTS)
    out = B.build_variant(str(tmp_path / ("libmcraw_rgbp_%s.so" % variant)), flags)
    assert os.path.getsize(out) > 0
    # the switches are known to the six demosaic sources alone: nothing else is compiled for a variant
    compiled = [ln for ln in capfd.readouterr().out.splitlines() if " -c " in ln]
    assert all(ln.endswith(SIX) for ln in compiled), compiled
    syms = subprocess.run(["nm", "-D", "--defined-only", out], capture_output=True, text=True, check=True).stdout
    assert "mcraw_diag_rgb_paths" in syms
