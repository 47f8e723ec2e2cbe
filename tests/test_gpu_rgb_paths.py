"""GPU (-m gpu): the persistent loops of the demosaic kernels forced, and every path of theirs counted, against the numpy
statements and an exact model.

krgb_mhc, krgb_bin2, krgb_bin2y (csrc/mcraw_rgb.hip), krgb_area (csrc/mcraw_area.hip) and krgb_resample (csrc/mcraw_resample.hip)
run a persistent grid for every kind with a LUT: min(units x frames, what the device holds at once) workgroups, each walking
t = blockIdx.x, + gridDim.x, ...  The second and later trips of that loop -- the barrier at its top, the re-staging of the LDS
arrays, f, col and fout of another frame -- are all a real batch runs, and the machine, not the input, decides whether a test
reaches them: the other suites' shapes stay below the grid.  Here five builds of the same sources (build.RGB_PATH_VARIANTS: the
census, -DMCRAW_PATHSR, alone; a grid capped at 1 and at 3 workgroups; the LDS arrays poisoned in front of every unit, with the
product's grid and with one workgroup) run the corpus of tests/_rgb_paths_model.py in a child process each
(tests/_rgb_paths_child.py): every kernel x {u8 hwc, u8 chw, u16 hwc, u16 chw, nv12, p010} x the four CFAs as one call of 5 frames
with per-frame colours, inputs on and off the 16-byte and dword grids, outputs on and off theirs, LUTs in LDS and in global
memory, a batch of 34 frames that RGB_MAXF splits, and the float kinds (no loop: the variants without a cap only).  The child
compares every call's output byte for byte with the numpy statements (_rgb_ref, _display_ref, _yuv_ref, _area_ref, _resample_ref),
the guard bands around it included; this module compares the census of every call with the model, EVERY counter, EXACTLY.

  every one        pixels; census == model(setting, variant), counter by counter
  census           every counter is above zero in the settings DRIVEN names for it; the grid the census reports is 1 .. units x frames
  grid1            per launch one workgroup: later units = units x frames - 1, crossings = frames - 1
  grid3            the model's walk; with grid1: every instance with a LUT shows later units and frame crossings
  poison, poison1  pixels, and every count as in `census` / `grid1`

A child that ends by a signal, at its time limit or without its result stops every further child, of this module and of every other (tests/_paths_harness.py): the remaining variants fail at
once.  Nothing is tried twice.

Wall times on an MI355X: one run of the module (5 passed in 13.87 s) for the whole tests, one run of the five children for their
own.  Per variant: the child's own `seconds` (from its first line to its result: 109 calls, 97 under a cap, and their
comparisons) / the whole test (the link of the variant, whose three objects came
with the build; start of the child with its imports, child, the models; the corpus, the numpy statements' answers and the file for
the children are made once, in 0.5 s, in front of `census`):
  census 0.59 / 2.67   grid1 0.58 / 2.57   grid3 0.57 / 2.44   poison 0.49 / 2.56   poison1 0.54 / 2.58
CHILD_TIMEOUT is ten times the slowest whole test; it guards against a hang, not against performance."""
import json
import os

import numpy as np
import pytest

import _paths_harness as PH
import motioncam_decoder_amd as M
from motioncam_decoder_amd import build as B

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "_rgb_paths_child.py")
CHILD_TIMEOUT = 27  # seconds: ten times the slowest measured whole test (see above)



def make_npz(path):
    """The corpus: the images, the LUTs, the plan of the settings and the bytes that the numpy statements give for each."""
    import _area_ref as A
    import _resample_ref as RS
    import _rgb_ref as R
    import _rgb_paths_model as T
    import _yuv_ref as Y
    rng = np.random.default_rng(20261020)
    arrays = {"lut_4096": rng.integers(0, 65536, 4096, dtype=np.uint16), "lut_65536": rng.integers(0, 65536, 65536, dtype=np.uint16)}
    o_of = {}  # (kernel, geometry, cfa, n) -> the f32 values in front of the output stage, per frame
    plan = []
    for s, (name, S) in enumerate(T.SETTINGS.items()):
        n, H, W = S["n"], S["H"], S["W"]
        S = dict(S, img="img_%d_%d_%d" % (n, H, W), exp="exp_%d" % s)
        if S["img"] not in arrays:  # from below the black levels to above white: the clamps of the output stage take part
            arrays[S["img"]] = rng.integers(0, 5000, (n, H, W), dtype=np.uint16)
        imgs = arrays[S["img"]]
        gain, matrix = T.colours(S)
        key = (S["kernel"], S["img"], S["cfa"], str(S.get("crop")), str(S.get("size")), S.get("filt"))
        if key not in o_of:
            if S["kernel"] in ("mhc", "bin2"):
                o_of[key] = [R.rgb_values(imgs[i], S["kernel"], T.WHITE, T.BLACK, S["cfa"], gain[i], matrix[i], clip=False) for i in range(n)]
            elif S["kernel"] == "area":
                o_of[key] = [A.values(A.area_estimates(imgs[i], S["crop"], S["size"], T.BLACK, S["cfa"]), T.WHITE, T.BLACK, gain[i], matrix[i])
                             for i in range(n)]
            else:
                o_of[key] = [RS.values(RS.resample_estimates(imgs[i], S["crop"], S["size"], S["filt"], T.BLACK, S["cfa"]), T.WHITE, T.BLACK,
                                       gain[i], matrix[i]) for i in range(n)]
        o, kind = o_of[key], S["kind"]
        if T.is_float(S):
            frames = [A.float_bits(v, kind) for v in o]
        elif T.is_yuv(S):
            coef = M.yuv_matrix("bt709", "limited", Y.BITS[kind], T.IN_BITS)
            frames = [Y.yuv_from_o(v, arrays["lut_%d" % S["lutn"]], kind, coef, T.IN_BITS) for v in o]
        else:
            frames = [A.display_from_o(v, arrays["lut_%d" % S["lutn"]], kind[:-3], kind[-3:]) for v in o]
        exp = np.stack([np.ascontiguousarray(f) for f in frames])
        arrays[S["exp"]] = exp.view(np.uint8).reshape(-1)
        assert arrays[S["exp"]].size == n * T.out_frame_bytes(S), name
        plan.append(S)
    arrays["plan"] = np.array(json.dumps(plan))
    np.savez(path, **arrays)


@pytest.fixture(scope="module")
def corpus_npz(tmp_path_factory):
    """Computed once for the module."""
    path = str(tmp_path_factory.mktemp("rgb_paths") / "corpus.npz")
    make_npz(path)
    return path


def _child(variant, corpus_npz, tmp_path_factory):
    """The census of `variant`'s child, which is run once whatever becomes of it (tests/_paths_harness.py)."""
    return PH.run_child(__name__, variant, CHILD, [corpus_npz, variant], B.RGB_PATH_VARIANTS[variant], "libmcraw_rgbp_%s.so" % variant,
                       CHILD_TIMEOUT, tmp_path_factory, PH.no_errors("outputs differ from the numpy statements"))


def check(variant, res):
    """The census `res` of `variant`'s child against the model."""
    import _rgb_paths_model as T
    assert res["paths"] == T.PATHS, "the child's counters are not the model's"
    cap = T.VARIANT_CAP[variant]
    assert sorted(res["census"]) == sorted(n for n, S in T.SETTINGS.items() if T.runs(S, variant))
    for name, got in res["census"].items():
        S = T.SETTINGS[name]
        fam, units = T.family(S), T.plan(S)["units"]
        nfs = T.launches(S)
        total = sum(units * nf for nf in nfs)
        # the grid: under a cap the model's own; else what the census reports, which must be a grid that walks every unit once
        wg = got["wg_" + fam]
        if cap is None and not T.is_float(S):
            if len(nfs) == 1:
                assert 1 <= wg <= total, (variant, name, wg, total)
                want = T.model(name, variant, resident=wg)
            else:  # (the model takes every launch to fit the device; true of these tiny units on any device this runs on)
                want = T.model(name, variant)
        else:
            want = T.model(name, variant)
            assert wg == sum(T.grids(S, variant)), (variant, name, wg)
        print(variant, name, json.dumps({k: v for k, v in got.items() if v or want[k]}))
        # ---- every variant and setting: the model, exactly
        for k in T.PATHS:
            assert got[k] == want[k], (variant, name, k, got[k], want[k])
        assert got["first_" + fam] + got["later_" + fam] == total, (variant, name)
        # ---- what the variant is about
        if cap is None:
            for k, names in T.DRIVEN.items():
                assert got[k] > 0 or name not in names, (variant, name, k)
        else:
            for k, names in T.DRIVEN_CAPPED.items():
                assert got[k] > 0 or name not in names, (variant, name, k)
            if cap == 1:
                assert wg == len(nfs) and got["later_" + fam] == total - len(nfs) and got["cross_" + fam] == S["n"] - len(nfs), (name, got)
    # every instance with a LUT (kernel, output kind, CFA) ran, and under a cap looped and crossed frames (asserted above)
    seen = {(T.family(S), S["kind"].replace("hwc", "").replace("chw", ""), S["cfa"]) for n, S in T.SETTINGS.items()
            if n in res["census"] and not T.is_float(S)}
    kinds_of = {"bin2": ("u8", "u16"), "bin2y": ("nv12", "p010")}
    instances = {(f, k, c) for f in T.FAMILIES for k in kinds_of.get(f, ("u8", "u16", "nv12", "p010")) for c in T.CFAS}
    assert instances <= seen, sorted(instances - seen)
    if variant in T.PRODUCT_OF and isinstance(PH.outcome(__name__, T.PRODUCT_OF[variant]), dict):
        assert res["census"] == PH.outcome(__name__, T.PRODUCT_OF[variant])["census"], "the poisoned build's counts are not the plain build's"


@pytest.mark.parametrize("variant", list(B.RGB_PATH_VARIANTS))
def test_rgb_paths(variant, corpus_npz, tmp_path_factory):
    check(variant, _child(variant, corpus_npz, tmp_path_factory))
