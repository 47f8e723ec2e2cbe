"""GPU (-m gpu): every path of the mosaic-to-mosaic stages counted, the guarded ones forced, against the numpy statements and an
exact model; and div_round swept over the edges of its proven domain.

kshade, kstats, kfixpix + kfixpix_list, kdenoise<1|2>, kmerge<0|1> (global positions and a cell field), khl_apply, khl_measure and
khl_clip sit in front of every demosaic call of
a real pipeline.  Their own suites compare outputs bit for bit; nothing there shows which branch a test entered: the per-wave fast paths
(`__any(cand)`, `clipped`, kstats' stats_tile<BL, true> and its one-bin shortcut), the three forms of load8 / store8 / the staging pieces, the chunks that staging leaves as "whatever LDS
held" and that kfixpix then reads into `cand`, the distance-4 swaps of kdenoise<2> at frames of 5 .. 7 rows or columns.  Here seven
builds of the stage sources (build.MOSAIC_PATH_VARIANTS and build.MOSAIC_FRAMES2_FLAGS; why each is valid: the head of csrc/mcraw_mosaic_paths.h) run the corpus of
tests/_mosaic_paths_model.py in a child process each (tests/_mosaic_paths_child.py): 12 sizes from 1 x 1 to 35 x 520, each as three
views (on the 16-byte grid, a base 2 bytes off it, a pitch of W + 3) of input and output, contents that drive both sides of every
data-dependent branch, 3 frames per call (7 for the merge: windows (0, 0), (2, 2), (5, 0), positions none, multiples of 8, even,
larger than a tile, a cell field; both supports), 407 calls.  The child compares every call's whole output buffer with the numpy
statements; this module compares the census of every call with the model, EVERY counter, EXACTLY.

  every one          outputs; census == model(setting, variant), counter by counter.  Only `cand` / `clipped` of lane rows that read
                     unstaged LDS (the model says which, and how many) are held to the model's range instead, and only where LDS is
                     not poisoned; div_round's two steps are the chip's: down + up <= calls, calls exact
  census             every counter is above zero in the settings DRIVEN names for it; both steps of div_round occur
  slow, poisonslow   no wave of kfixpix without a candidate, no lane row of khl_apply unclipped, no wave of kstats in
                     stats_tile<BL, true> and none in its one-bin shortcut, no member of kmerge passed over as weighing 0; outputs as
                     the statements
  poison*            0xFFFF in every chunk that staging leaves: outputs as the statements, no range left in the model, and every
                     counter that has no range in `census` equals `census`'s
  pieces             kstats with at most 2 tiles per workgroup: more workgroups than the product's, prefetches in all of them;
                     kmerge with 3 outputs per launch: ceil(count / 3) > 1 launches in every call, windows across them
  th16               kfixpix, kdenoise and kmerge with tiles of 16 rows
  frames2            the launch loops of every stage but kmerge with 2 frames per launch (2 + 1 for the 3 frames of a call): outputs
                     as the statements, every counter as `census`'s
  sweep              div_round(n, den) == n / den for den 1 .. 6400, quotients 0 .. 65536, n = k * den + {-1, 0, 1, den / 2,
                     den - 1}: as many evaluations as the enumeration in Python counts, no mismatch, and both correction steps taken

A child that ends by a signal, at its time limit or without its result stops every further child, of this module and of every other (tests/_paths_harness.py): the remaining tests fail at
once.  Nothing is tried twice.

Measured on an MI355X, one run of the module (7 passed in 22.25 s).  Per variant: the child's own `seconds` (from its first line to
its result: 407 calls, their comparisons and census reads) / the whole test (the link of the variant, whose objects came with the
build; start of the child with its imports, child, the 407 models; the numpy statements' answers for the children are made once,
in 0.6 s, in front of `census`):
  census 0.85 / 3.09   slow 0.65 / 2.84   poison 0.65 / 3.26   poisonslow 0.65 / 3.14   pieces 0.67 / 2.95   th16 0.66 / 3.06
  sweep 0.05 / 2.59
`frames2` (test_mosaic_paths_frames2) was added later: its whole test 5.78 s in a run of this module.
CHILD_TIMEOUT is ten times the slowest whole test; it guards against a hang, not against performance.

The sweep on that chip: 2 097 177 599 evaluations, no mismatch; the step down (q - 1) taken by 516 137 076 of them, the step up
(q + 1) by 103 877 353: both corrections are live code, and one of them is needed for 30 % of the edges of the domain.  In the corpus
(3 867 984 calls of kdenoise and kmerge, among them lanes' columns past the row end, whose samples no output reads and in kdenoise
are what LDS held: the steps differ by one or two from build to build) 495 steps down and 288 up; at quotients below 900 (12-bit
content) only the step up occurs, at exact multiples of den: the `bright` settings are there for the other one."""
import json
import os

import numpy as np
import pytest

import _paths_harness as PH
from motioncam_decoder_amd import build as B

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "_mosaic_paths_child.py")
CHILD_TIMEOUT = 33  # seconds: ten times the slowest measured whole test (see above)



def make_npz(path):
    """What the numpy statements give for every setting: exp_<i> the mosaics, exp2_<i> the records."""
    import _denoise_ref as D
    import _fixpix_ref as FX
    import _highlights_ref as HR
    import _merge_cells_ref as MC
    import _merge_ref as MR
    import _mosaic_paths_model as T
    import _shade_ref as SR
    import _stats_ref as ST
    arrays = {}
    for i, (name, S) in enumerate(T.SETTINGS.items()):
        imgs, fam = T.images(name), S["family"]
        hl = (T.HL_SAT, T.HL_BLACK, T.HL_GAIN, HR.CFA[T.HL_CFA])
        if fam == "stats":
            exp = None
            arrays["exp2_%d" % i] = ST.record(ST.stats(imgs, S["bins"], T.ST_SHIFT[S["bins"]], T.ST_SAT, T.stats_roi(S) if S["roi"] else None))
        elif fam in ("merge", "merge_cells"):
            before, after = T.MG_WINDOWS[S["window"]]
            kw = dict(before=before, after=after, first=S["first"], count=S["count"], support=S["support"], amount=256)
            if fam == "merge":
                exp = MR.merge(imgs, T.merge_lut(name), T.DN_SHIFT, pos=T.merge_pos(name), **kw)
            else:
                exp = MC.merge(imgs, T.merge_lut(name), T.DN_SHIFT, T.merge_pos(name), T.MG_CELL, **kw)
        elif fam == "shade":
            exp = SR.shade_batch_ref(imgs, T.shade_map(name), T.SH_BLACK, T.SH_TOP)
        elif fam == "fixpix":
            exp, counts = FX.fixpix(imgs, FX.HOT | FX.COLD, S["rank"], int(np.rint(T.FP_REL * 256)), T.FP_BLACK, T.FP_ABS, T.fix_list(name))
            if S["counts"]:
                arrays["exp2_%d" % i] = counts
        elif fam == "denoise":
            exp = D.denoise(imgs, T.denoise_lut(name), T.DN_SHIFT, S["radius"], S["amount"])
        elif fam == "hl_apply":
            exp = HR.apply(imgs, HR.REBUILD, *hl, rec=T.hl_records(name) if S["rec"] else None, top=T.HL_TOP)
        elif fam == "hl_clip":
            exp = HR.apply(imgs, HR.CLIP, *hl, top=T.HL_TOP)
        else:
            exp = None
            arrays["exp2_%d" % i] = HR.raw(*HR.measure(imgs, T.HL_SAT, T.HL_BLACK, T.HL_GAIN, HR.CFA[T.HL_CFA], T.HL_LO))
        if exp is not None:
            arrays["exp_%d" % i] = np.asarray(exp, np.uint16)
    np.savez(path, **arrays)


@pytest.fixture(scope="module")
def corpus_npz(tmp_path_factory):
    """Computed once for the module."""
    path = str(tmp_path_factory.mktemp("mosaic_paths") / "corpus.npz")
    make_npz(path)
    return path


def _child(variant, corpus_npz, tmp_path_factory):
    """The result of `variant`'s child, which is run once whatever becomes of it (tests/_paths_harness.py)."""
    flags = B.MOSAIC_FRAMES2_FLAGS if variant == "frames2" else B.MOSAIC_PATH_VARIANTS["census" if variant == "sweep" else variant]
    judge = (lambda *a: None) if variant == "sweep" else PH.no_errors("outputs differ from the numpy statements")
    return PH.run_child(__name__, variant, CHILD, [corpus_npz, variant], flags, "libmcraw_mosp_%s.so" % variant, CHILD_TIMEOUT,
                       tmp_path_factory, judge)


def _seen(variant):
    """What `variant`'s child left, if it has run: its result or the failure."""
    return PH.outcome(__name__, variant)


def check(variant, res):
    """The census `res` of `variant`'s child against the model."""
    import _mosaic_paths_model as T
    assert res["paths"] == T.PATHS, "the child's counters are not the model's"
    assert list(res["census"]) == list(T.SETTINGS)
    total = dict.fromkeys(T.PATHS, 0)
    ranged = 0
    for name, row in res["census"].items():
        got, want = dict(zip(T.PATHS, row)), T.model(name, variant)
        print(variant, name, json.dumps({k: v for k, v in got.items() if v}), json.dumps(want["_unstaged"]))
        for k in T.PATHS:
            total[k] += got[k]
            if k in T.UNMODELLED:
                continue
            lo, hi = want["_unstaged"].get(k, (0, 0))
            assert want[k] + lo <= got[k] <= want[k] + hi, (variant, name, k, got[k], want[k], lo, hi)
        ranged += len(want["_unstaged"])
        assert got["div_down"] + got["div_up"] <= got["div_calls"], (variant, name)
        # what a range leaves open: a lane row is a candidate or not, a wave has one or not
        assert got["fp_wave_any"] + got["fp_wave_none"] == want["fp_wave_any"] + want["fp_wave_none"], (variant, name)
        assert got["hl_clipped"] + got["hl_unclipped"] == want["hl_clipped"] + want["hl_unclipped"], (variant, name)
        if variant == "census":
            for k, names in T.DRIVEN.items():
                assert got[k] > 0 or name not in names, (variant, name, k)
        if variant in ("poison", "poisonslow"):
            plain = _seen({"poison": "census", "poisonslow": "slow"}[variant])
            if isinstance(plain, dict):
                free = T.model(name, "census")["_unstaged"]
                for k, a, b in zip(T.PATHS, row, plain["census"][name]):
                    assert a == b or k in free or k in T.UNMODELLED, (variant, name, k, a, b)
    print(variant, "totals", json.dumps(total))
    if variant == "census":
        assert ranged > 0, "no lane row of the corpus reads unstaged LDS"
        assert total["div_down"] > 0 and total["div_up"] > 0, "a correction step of div_round never ran: %r" % (total,)
    else:
        assert variant in ("th16", "pieces", "slow", "frames2") or ranged == 0
    if variant == "pieces":  # more workgroups of kstats than the product's, each of two tiles at most; kmerge in launches of 3 outputs
        plain = _seen("census")
        for name, row in res["census"].items():
            S = T.SETTINGS[name]
            if S["family"] in ("merge", "merge_cells"):
                got = dict(zip(T.PATHS, row))
                assert got["mg_launch"] == (S["count"] + 2) // 3 > 1, (name, got["mg_launch"])
            if S["family"] == "stats":
                P, got = T.stats_plan(S, variant), dict(zip(T.PATHS, row))
                assert P["tpc"] <= 2 and got["wg"] == T.FRAMES * P["wgs"] and got["wg"] + got["ss_prefetch"] == T.FRAMES * P["tiles"], name
        assert total["ss_prefetch"] > 0 and (not isinstance(plain, dict) or total["wg"] > sum(r[0] for r in plain["census"].values()))
    if variant == "frames2" and isinstance(_seen("census"), dict):
        for name, row in res["census"].items():
            free = T.model(name, "census")["_unstaged"]
            for k, a, b in zip(T.PATHS, row, _seen("census")["census"][name]):
                assert a == b or k in free or k in T.UNMODELLED, (variant, name, k, a, b)
    if variant in ("slow", "poisonslow"):
        assert total["mg_zerow"] == 0 and total["mg_staged"] > 0
        assert total["ss_full"] == 0 and total["ss_onebin"] == 0 and total["ss_partial"] > 0
        assert total["fp_wave_none"] == 0 and total["hl_unclipped"] == 0 and total["fp_wave_any"] > 0 and total["hl_clipped"] > 0


@pytest.mark.parametrize("variant", list(B.MOSAIC_PATH_VARIANTS))
def test_mosaic_paths(variant, corpus_npz, tmp_path_factory):
    import _mosaic_paths_model as T
    assert tuple(B.MOSAIC_PATH_VARIANTS) == T.VARIANTS
    check(variant, _child(variant, corpus_npz, tmp_path_factory))


def test_mosaic_paths_frames2(corpus_npz, tmp_path_factory):
    """build.MOSAIC_FRAMES2_FLAGS: the same check as every other variant's."""
    import _mosaic_paths_model as T
    assert T.EXTRA_VARIANTS == ("frames2",)
    check("frames2", _child("frames2", corpus_npz, tmp_path_factory))


def test_div_round_sweep(tmp_path_factory):
    import _mosaic_paths_model as T
    res = _child("sweep", "sweep", tmp_path_factory)
    print("sweep", json.dumps(res))
    assert res["rc"] == 0
    assert res["bad"] == 0, "div_round(%d, %d) = %d, not %d (%d mismatches)" % (res["n"], res["den"], res["got"], res["n"] // max(res["den"], 1), res["bad"])
    assert res["evals"] == res["calls"] == T.div_sweep_count()
    assert res["down"] + res["up"] <= res["calls"]
    assert res["down"] > 0 and res["up"] > 0, "a correction step of div_round is dead code over the proven domain: %r" % (res,)
