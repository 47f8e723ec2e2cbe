"""What tests/test_gpu_warp_paths.py, test_gpu_mesh_paths.py and test_gpu_ha_paths.py share: the file for their children
(tests/_gather_paths_child.py) with the corpus of tests/_gather_paths_model.py and the bytes the numpy statements give, the run of a
variant's child, and the comparison of its census with the model.  A plain module: no fixture, no plugin."""
import json
import os

import numpy as np

import _gather_paths_model as G
import _paths_harness as PH
import _rgb_paths_model as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "_gather_paths_child.py")
CHILD_TIMEOUT = 60  # seconds: guards against a hang, not against performance (a child takes a few seconds)
LIBNAME = {"warp": "libmcraw_warpp_%s.so", "mesh": "libmcraw_meshp_%s.so", "ha": "libmcraw_hap_%s.so"}


def make_npz(path, kernel):
    """The corpus of `kernel`: the images, the maps or meshes, the colours, the LUTs, the plan of the cases and the bytes the numpy
    statement gives for each.  -> the number of cases."""
    import _display_ref as D
    import _ha_ref as HA
    import _mesh_ref as MR
    import _warp_ref as W
    import _yuv_ref as Y
    import motioncam_decoder_amd as M
    rng = np.random.default_rng(20261021)
    arrays = {"lut_4096": rng.integers(0, 65536, 4096, dtype=np.uint16), "lut_65536": rng.integers(0, 65536, 65536, dtype=np.uint16)}
    o_of, plan = {}, []
    for s, (name, S) in enumerate(G.cases(kernel).items()):
        n, kind = S["n"], S["kind"]
        S = dict(S, exp="exp_%d" % s, geokey="geo_%s_%d_%d_%d_%d" % (S["geo"], S["size"][0], S["size"][1], S["H"], n))
        imgs = arrays.setdefault(S["img"], G.images(S["img"]))
        gain, matrix = G.colours(n)
        arrays.setdefault("gain_%d" % n, gain), arrays.setdefault("matrix_%d" % n, matrix)
        geo = None if kernel == "ha" else arrays.setdefault(S["geokey"], G.geometry(S))
        key = (S["img"], S.get("geokey"), S["cfa"], S["filt"])
        if key not in o_of:  # the f32 values in front of the output stage, per frame
            if kernel == "ha":
                o_of[key] = [HA.rgb_values(imgs[i], S["white"], S["black"], S["cfa"], gain[i], matrix[i]) for i in range(n)]
            elif kernel == "warp":
                o_of[key] = [W.values(W.warp_estimates(imgs[i], geo[i if len(geo) > 1 else 0], S["size"], S["filt"], S["black"], S["cfa"]),
                                      S["white"], S["black"], gain[i], matrix[i]) for i in range(n)]
            else:
                o_of[key] = [MR.values(MR.mesh_estimates(imgs[i], geo[i if len(geo) > 1 else 0], S["size"], S["filt"], S["black"], S["cfa"]),
                                       S["white"], S["black"], gain[i], matrix[i]) for i in range(n)]
        o = o_of[key]
        if G.is_float(S):
            frames = [W.float_bits(v, kind) for v in o]
        elif G.is_yuv(S):
            coef = M.yuv_matrix("bt709", "limited", Y.BITS[kind], S["in_bits"])
            frames = [Y.yuv_from_o(v, arrays["lut_%d" % S["lutn"]], kind, coef, S["in_bits"]) for v in o]
        else:
            frames = [D.apply_lut(v, arrays["lut_%d" % S["lutn"]], kind[:-3]) for v in o]
            if kind[-3:] == "hwc":
                frames = [f.transpose(1, 2, 0) for f in frames]
        arrays[S["exp"]] = np.stack([np.ascontiguousarray(f) for f in frames]).view(np.uint8).reshape(-1)
        assert arrays[S["exp"]].size == n * G.out_frame_bytes(S), name
        plan.append(S)
    arrays["plan"] = np.array(json.dumps(plan))
    np.savez(path, **arrays)
    return len(plan)


def run_variant(module, kernel, variant, corpus_npz, tmp_path_factory):
    """The result of `variant`'s child for `module`, which is run once whatever becomes of it (tests/_paths_harness.py)."""
    from motioncam_decoder_amd import build as B
    ncases = sum(1 for S in G.cases(kernel).values() if G.runs(S, variant))
    return PH.run_child(module, variant, CHILD, [corpus_npz, kernel, variant], B.RGB_PATH_VARIANTS[variant], LIBNAME[kernel] % variant, CHILD_TIMEOUT,
                        tmp_path_factory, PH.no_errors("outputs differ from the numpy statement", lambda res: res["cases"] == ncases))


def check(module, kernel, variant, res):
    """The census `res` of `variant`'s child against the model: every counter of every case, exactly."""
    assert res["paths"] == T.PATHS, "the child's counters are not the model's"
    cap = T.VARIANT_CAP[variant]
    assert sorted(res["census"]) == sorted(n for n, S in G.cases(kernel).items() if G.runs(S, variant))
    for name, got in res["census"].items():
        S = G.cases(kernel)[name]
        units, nfs = G.plan(S)["units"], G.launches(S)
        total = sum(units * nf for nf in nfs)
        wg = got["wg_" + kernel]
        if cap is None and not G.is_float(S):  # the grid: what the census reports, which must be one that walks every unit once
            if len(nfs) == 1:
                assert 1 <= wg <= total, (variant, name, wg, total)
                want = G.model(kernel, name, variant, resident=wg)
            else:  # (the model takes every launch to fit the device: true of one-tile frames on any device this runs on)
                want = G.model(kernel, name, variant)
        else:
            want = G.model(kernel, name, variant)
            assert wg == sum(G.grids(S, variant)), (variant, name, wg)  # under a cap: min(units x frames, N) per launch
        print(variant, name, json.dumps({k: v for k, v in got.items() if v or want[k]}))
        for k in T.PATHS:
            assert got[k] == want[k], (variant, name, k, got[k], want[k])
        assert got["first_" + kernel] + got["later_" + kernel] == total, (variant, name)
        for k in G.ARGUED_ZERO:
            assert got[k] == 0, (variant, name, k)
        if cap is None:
            for k, names in G.DRIVEN.items():
                assert got[k] > 0 or (kernel, name) not in names, (variant, name, k)
        else:
            for k, names in G.DRIVEN_CAPPED.items():
                assert got[k] > 0 or (kernel, name) not in names, (variant, name, k)
            if cap == 1:
                assert wg == len(nfs) and got["later_" + kernel] == total - len(nfs) and got["cross_" + kernel] == S["n"] - len(nfs), (name, got)
    if variant in T.PRODUCT_OF and isinstance(PH.outcome(module, T.PRODUCT_OF[variant]), dict):
        assert res["census"] == PH.outcome(module, T.PRODUCT_OF[variant])["census"], "the poisoned build's counts are not the plain build's"
