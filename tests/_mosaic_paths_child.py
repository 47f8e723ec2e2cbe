"""Child process of tests/test_gpu_mosaic_paths.py:  python _mosaic_paths_child.py <corpus.npz> <variant>   or   ... sweep

Loads the build of the library that MCRAW_LIB_PATH names (one with the mosaic stages' census, build.MOSAIC_PATH_VARIANTS) and runs
every setting of tests/_mosaic_paths_model.py SETTINGS: one call of Context.shade / stats / fix_pixels / denoise / merge / highlights /
highlight_chroma each, on the setting's view of the input (offset, pitch and frame stride) into the same view of an output that
holds a sentinel everywhere else.  The whole output buffer -- guard bands, the gaps between rows and frames -- is compared with what
the parent worked out from the numpy statements (_shade_ref, _stats_ref, _fixpix_ref, _denoise_ref, _merge_ref, _merge_cells_ref, _highlights_ref); so are the
records of stats, the counts record of fix_pixels and the records of highlight_chroma, and the input must stay as it was.  The census is read, and started over, after
every call.  Prints one line  RESULT {json}.  Exit status 1 when something differs.

`sweep`: mcraw_diag_div_sweep alone, the sweep of div_round (csrc/mcraw_denoise.hip)."""
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import motioncam_decoder_amd as M  # noqa: E402
import _paths_harness as PH  # noqa: E402
import _mosaic_paths_model as T  # noqa: E402

GUARD, SENT = 2048, 0xA5A5
DEV = torch.device("cuda:0")


def dev16(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint16).view(np.int16)).to(DEV).view(torch.uint16)


def host16(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def sweep(lib):
    lib.mcraw_diag_div_sweep.restype = C.c_int
    lib.mcraw_diag_div_sweep.argtypes = [C.POINTER(C.c_uint64)]
    a = (C.c_uint64 * 8)()
    t0 = time.time()
    rc = lib.mcraw_diag_div_sweep(a)
    res = dict(zip(("evals", "bad", "n", "den", "got", "calls", "down", "up"), (int(v) for v in a)))
    res["rc"], res["seconds"] = rc, round(time.time() - t0, 2)
    print("RESULT " + json.dumps(res))
    return 0 if rc == 0 else 1


def main(npz, variant):
    t0 = time.time()
    lib = M.load()
    if npz == "sweep":
        torch.zeros(1, device=DEV)
        return sweep(lib)
    Z = np.load(npz)
    errors = []

    census = PH.census_reader(lib, "mcraw_diag_mosaic_paths", T.PATHS, as_dict=False)

    def run(ctx, i, name, S):
        H, W, fam = S["H"], S["W"], S["family"]
        off, pitch, fstride = T.view_geom(S)
        imgs = T.images(name)
        nin = T.nframes(S)                                          # frames in
        nout = S["count"] if fam in ("merge", "merge_cells") else nin  # and out
        ibuf = torch.zeros((off + nin * fstride + 16,), dtype=torch.int16, device=DEV)
        assert ibuf.data_ptr() % 16 == 0
        src = torch.as_strided(ibuf, (nin, H, W), (fstride, pitch, 1), off)
        src.copy_(torch.from_numpy(imgs.view(np.int16)).to(DEV))
        before = ibuf.clone()
        total = GUARD + off + nout * fstride + GUARD
        obuf = torch.full((total,), SENT - 65536, dtype=torch.int16, device=DEV)
        assert obuf.data_ptr() % 16 == 0 and GUARD % 8 == 0
        dst = torch.as_strided(obuf, (nout, H, W), (fstride, pitch, 1), GUARD + off).view(torch.uint16)
        src = src.view(torch.uint16)
        extra = None  # (what the call returns beside the mosaics, expected as exp2_<i>)
        torch.cuda.synchronize()
        if fam == "stats":
            r = ctx.stats(src, bins=S["bins"], shift=T.ST_SHIFT[S["bins"]], sat=T.ST_SAT, roi=T.stats_roi(S) if S["roi"] else None)
            extra = r.raw.cpu().numpy().astype(np.int64)
        elif fam in ("merge", "merge_cells"):
            wbefore, wafter = T.MG_WINDOWS[S["window"]]
            pos = T.merge_pos(name)
            ctx.merge(src, dev16(T.merge_lut(name)), T.DN_SHIFT, before=wbefore, after=wafter, first=S["first"], count=S["count"],
                      support=S["support"], amount=1.0, pos=None if pos is None else torch.from_numpy(pos).to(DEV), out=dst,
                      cell=T.MG_CELL if fam == "merge_cells" else None)
        elif fam == "shade":
            ctx.shade(src, dev16(T.shade_map(name)), black=T.SH_BLACK, top=T.SH_TOP, out=dst)
        elif fam == "fixpix":
            lst = T.fix_list(name)
            pixels = None if lst is None else torch.from_numpy(lst.view(np.int32)).to(DEV)
            r = ctx.fix_pixels(src, black=T.FP_BLACK, abs_thr=T.FP_ABS, rel_thr=T.FP_REL, rank=S["rank"], pixels=pixels,
                               counts=bool(S["counts"]), out=dst)
            if S["counts"]:
                extra = r[1].cpu().numpy().astype(np.int64)
        elif fam == "denoise":
            ctx.denoise(src, dev16(T.denoise_lut(name)), T.DN_SHIFT, radius=S["radius"], amount=S["amount"] / 256.0, out=dst)
        elif fam == "hl_measure":
            r = ctx.highlight_chroma(src, sat=T.HL_SAT, black=T.HL_BLACK, gain=T.HL_GAIN, cfa=T.HL_CFA, lo=T.HL_LO, scope="frame")
            extra = r.raw.cpu().numpy().astype(np.int64)
        else:
            rec = None
            if fam == "hl_apply" and S["rec"]:
                rec = torch.from_numpy(T.HR.raw(*T.hl_records(name))).to(DEV)
            ctx.highlights(src, sat=T.HL_SAT, black=T.HL_BLACK, gain=T.HL_GAIN, cfa=T.HL_CFA, lo=T.HL_LO, top=T.HL_TOP,
                           mode="clip" if fam == "hl_clip" else "rebuild", chroma=rec, out=dst)
        torch.cuda.synchronize()
        if not torch.equal(ibuf, before):
            errors.append("%s: the input was written" % name)
        want = np.full(total, SENT, np.uint16)
        if fam not in ("hl_measure", "stats"):
            np.lib.stride_tricks.as_strided(want[GUARD + off:], (nout, H, W), (2 * fstride, 2 * pitch, 2))[...] = Z["exp_%d" % i]
        got = obuf.cpu().numpy().view(np.uint16)
        if not np.array_equal(got, want):
            bad = np.nonzero(got != want)[0]
            errors.append("%s: %d samples of the output buffer differ, first at %d (the output starts at %d, pitch %d, frame stride %d)"
                          % (name, bad.size, int(bad[0]), GUARD + off, pitch, fstride))
        if extra is not None and not np.array_equal(extra, Z["exp2_%d" % i].astype(np.int64)):
            errors.append("%s: the record differs: %s, not %s" % (name, str(extra.tolist())[:300], str(Z["exp2_%d" % i].tolist())[:300]))

    res = {"paths": T.PATHS, "census": {}}
    ctx = M.Context(0)
    try:
        census()  # (start from zero)
        for i, (name, S) in enumerate(T.SETTINGS.items()):
            run(ctx, i, name, S)
            res["census"][name] = census()
    finally:
        ctx.close()
    return PH.finish(res, errors, t0)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else ""))
