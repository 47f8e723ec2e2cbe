#!/usr/bin/env python3
"""The resampling demosaic (mcraw_demosaic_resample_batch) on HBM-resident mosaics beside krgb_mhc of the same family on the same
input (the yardstick: at the crop's own size the stage computes what MHC computes, in two passes through LDS more), beside kshade out
of place, and beside the torch route (demosaic(algo="mhc", dtype="f16"), a slice, and torch.nn.functional.interpolate(mode="bicubic",
antialias=True) on it): ms per batch from events around the call on a torch stream, medians over the reps, algorithmic bytes (the
crop in + samples out) and the fraction of the 8 TB/s peak.  240 12-bit frames of noise; all forms of a geometry take turns rep by
rep in ONE process, in both orders.  Frame 0 of two resample forms of every geometry is checked against the numpy statement
(tests/_resample_ref.py) before anything is timed.  Appends to profiles/resample_bench.jsonl.  Needs a GPU.

    python tools/bench_resample.py [--reps 7] [--frames 240] [--geoms uhd_identity,43_uhd,uhd_1440p,uhd_zoom90] [--out PATH]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch

import _resample_ref as S
import _yuv_ref as Y
import motioncam_decoder_amd as M
from altlib import bench_images, bench_mosaics

PEAK = 8e12
WHITE, BLACK = 4095.0, (64, 64, 64, 64)
GAIN = (2.0, 1.0, 1.6)
MAT = np.array([[1.7, -0.5, -0.2], [-0.25, 1.4, -0.15], [0.05, -0.45, 1.4]], np.float32)
DISTINCT = 2
# name: (W, H, (Ho, Wo), crop or None for fit_crop's)
GEOMS = {"uhd_identity": (3840, 2160, (2160, 3840), (0, 0, 2160, 3840)),
         "43_uhd": (4032, 3024, (2160, 3840), None),
         "uhd_1440p": (3840, 2160, (1440, 2560), (0, 0, 2160, 3840)),
         "uhd_zoom90": (3840, 2160, (2160, 3840), (108, 192, 1944, 3456))}
KINDS = ("f16", "u8", "nv12")
ES = {"f16": 2, "u8": 1, "nv12": 1}


def samples(kind, ho, wo):
    return ho * wo * 3 // (2 if kind == "nv12" else 1)


def run(ctx, name, n, reps):
    dev = torch.device("cuda:0")
    W, H, size, crop = GEOMS[name]
    ho, wo = size
    crop = M.fit_crop(H, W, ho, wo, algo="resample") if crop is None else crop
    imgs = bench_images("noise", W, H, DISTINCT, np.random.default_rng(7))
    mos = bench_mosaics(dev, imgs, n)
    shaded = torch.empty_like(mos)
    gm = M.gain_map(np.ones((4, 13, 17)) * 1.25)
    dgm = torch.from_numpy(gm.view(np.int16)).to(dev).view(torch.uint16)
    out = torch.empty(n * 3 * max(W * H, wo * ho) * 2, dtype=torch.uint8, device=dev)  # room for the largest form (f16)
    stream = torch.cuda.Stream()
    kw = dict(white=WHITE, black=BLACK, gain=GAIN, matrix=MAT)

    def view(kind, h, w):
        t = out[: n * samples(kind, h, w) * ES[kind]]
        if kind == "f16":
            return t.view(torch.float16).view(n, 3, h, w)
        return t.view(n, h, w, 3) if kind == "u8" else t.view(n, h * 3 // 2, w)

    def demosaic(kind, algo, h, w, **extra):
        o = view(kind, h, w)
        if kind == "f16":
            return ctx.demosaic(mos, algo=algo, dtype="f16", out=o, **extra, **kw)
        if kind == "u8":
            return ctx.demosaic_display(mos, algo=algo, transfer="bt709", dtype=torch.uint8, layout="hwc", out=o, **extra, **kw)
        return ctx.demosaic_yuv(mos, algo=algo, fmt="nv12", transfer="bt709", out=o, **extra, **kw)

    def torch_route():
        y0, x0, ch, cw = crop
        full = ctx.demosaic(mos, algo="mhc", dtype="f16", out=view("f16", H, W), **kw)[:, :, y0:y0 + ch, x0:x0 + cw]
        if (ch, cw) == size:
            return full.contiguous()
        return torch.nn.functional.interpolate(full, size=size, mode="bicubic", antialias=True, align_corners=False)

    forms = {}
    for kind in KINDS:
        forms["resample_" + kind] = lambda kind=kind: demosaic(kind, "resample", ho, wo, size=size, crop=crop, filter="cubic")
        forms["mhc_" + kind] = lambda kind=kind: demosaic(kind, "mhc", H, W)
    forms["resample_f16_linear"] = lambda: demosaic("f16", "resample", ho, wo, size=size, crop=crop, filter="linear")
    forms["kshade"] = lambda: ctx.shade(mos, dgm, black=BLACK, out=shaded)
    forms["torch_mhc_f16_interpolate_bicubic"] = torch_route
    # bytes: what the form has to read and write at least
    crop_in = n * crop[2] * crop[3] * 2
    alg = {"kshade": 2 * n * W * H * 2, "torch_mhc_f16_interpolate_bicubic": crop_in + n * samples("f16", ho, wo) * 2,
           "resample_f16_linear": crop_in + n * samples("f16", ho, wo) * 2}
    for kind in KINDS:
        alg["resample_" + kind] = crop_in + n * samples(kind, ho, wo) * ES[kind]
        alg["mhc_" + kind] = n * W * H * 2 + n * samples(kind, H, W) * ES[kind]

    torch.cuda.synchronize()
    o = S.values(S.resample_estimates(imgs[0], crop, size, "cubic", BLACK, "rggb"), WHITE, BLACK, GAIN, MAT)  # the numpy statement of frame 0
    for f in forms:  # warm-up, and the correctness of frame 0 of two resample forms
        with torch.cuda.stream(stream):
            res = forms[f]()
        torch.cuda.synchronize()
        if f == "resample_f16":
            assert np.array_equal(res[0].view(torch.int16).cpu().numpy().view(np.uint16), S.float_bits(o, "f16")), (name, f)
        elif f == "resample_nv12":
            want = Y.yuv_from_o(o, M.transfer_lut("bt709", 4096, 12), "nv12", M.yuv_matrix("bt709", "limited", 8, 12), 12)
            assert np.array_equal(res[0].cpu().numpy(), want), (name, f)
        del res
    ms = {f: [] for f in forms}
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rep in range(reps):
        for f in (list(forms) if rep % 2 == 0 else list(forms)[::-1]):  # the forms take turns, in both orders
            with torch.cuda.stream(stream):
                a.record(stream)
                res = forms[f]()
                b.record(stream)
            torch.cuda.synchronize()
            del res
            ms[f].append(a.elapsed_time(b))
    ctx.synchronize()
    assert ctx.errors() == 0
    rows = []
    torch_ms = float(np.median(ms["torch_mhc_f16_interpolate_bicubic"]))
    for f in forms:
        med = float(np.median(ms[f]))
        r = {"geom": name, "form": f, "frames": n, "width": W, "height": H, "crop": list(crop), "size": list(size), "reps": reps,
             "batch_ms": round(med, 4), "batch_ms_min": round(min(ms[f]), 4), "batch_ms_max": round(max(ms[f]), 4),
             "alg_GB": round(alg[f] / 1e9, 3), "frac_peak_batch": round(alg[f] / (med * 1e-3) / PEAK, 3)}
        if f.startswith("resample_"):
            r["ratio_to_mhc"] = round(med / float(np.median(ms["mhc_" + f.split("_")[1]])), 3)
            r["ratio_to_torch_route"] = round(med / torch_ms, 3)
        rows.append(r)
    del mos, out, shaded
    torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--geoms", default=",".join(GEOMS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_resample.py needs a GPU")
    ctx = M.Context(0)
    with open(args.out, "a") as fh:
        for name in [g for g in args.geoms.split(",") if g]:
            for r in run(ctx, name, args.frames, max(3, args.reps)):
                line = json.dumps(r)
                print(line, flush=True)
                fh.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
