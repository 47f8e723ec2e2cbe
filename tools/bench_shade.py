#!/usr/bin/env python3
"""Lens-shading gain maps on HBM-resident mosaics (mcraw_shade_batch) beside krgb_bin2 f16 linear (the yardstick, measured in
the same run) and beside the same correction built from torch ops: ms per batch (events around the call on a torch stream),
algorithmic bytes (mosaic in + mosaic out for the shade forms) and the fraction of the 8 TB/s peak.  240 UHD 12-bit frames,
smooth (natural images) and noise content, a 17 x 13 map; all forms take turns rep by rep in ONE process.  Frame 0 of every
library form is checked against the numpy reference.  Also demosaic(algo="mhc", dtype=f16) with and without shading=.
Appends to profiles/shade_bench.jsonl.  Needs a GPU.

    python tools/bench_shade.py [--reps 15] [--frames 240] [--content smooth,noise] [--alt-lib PATH]

--alt-lib: another build of the library whose shade kernel uses the other store policy
(python -m motioncam_decoder_amd.build variant PATH -DMCRAW_SHADE_FLIP_STORES); its out-of-place and in-place forms take turns
with the others, in a context of its own.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch

import _libs as L
import _rgb_ref as R
import _shade_ref as S
import motioncam_decoder_amd as M
from altlib import AltLib

PEAK = 8e12
W, H = 3840, 2160
GH, GW = 13, 17
WHITE, BLACK, TOP = 4095.0, (64, 64, 64, 64), 65535
GAIN = (2.0, 1.0, 1.6)
MAT = np.array([[1.7, -0.5, -0.2], [-0.25, 1.4, -0.15], [0.05, -0.45, 1.4]], np.float32)
DISTINCT = 4
FORMS = ["shade_out", "shade_inplace", "shade_out_perframe", "bin2_f16", "torch_ops", "mhc_f16", "mhc_f16_shading"]
ALT_FORMS = ["shade_out_alt", "shade_inplace_alt"]


def float_gains(k=0):
    """A lens-like map: 1 in the centre, up to about 2 stops in the corners, each channel its own."""
    y, x = np.linspace(-1, 1, GH)[:, None], np.linspace(-1, 1, GW)[None, :]
    r2 = (x * x + y * y) / 2
    return np.stack([1.0 + (s + 0.01 * k - 1.0) * r2 for s in (3.6, 2.9, 2.95, 3.9)])


def torch_shade(mos, fg, black, top):
    """What a user writes without the kernel: per CFA position, the map upsampled to the frame with bilinear interpolation
    (corner points on corner pixels), multiply what is above the black level, round, clamp, back to uint16."""
    n, h, w = mos.shape
    out = torch.empty_like(mos)
    for p in range(4):
        py, px = p >> 1, p & 1
        g = torch.nn.functional.interpolate(fg[None, p:p + 1], size=(h, w), mode="bilinear", align_corners=True)[0, 0, py::2, px::2]
        x = mos[:, py::2, px::2].to(torch.float32)
        out[:, py::2, px::2] = torch.round((x - black[p]) * g + black[p]).clamp_(0, top).to(torch.uint16)
    return out


def run(ctx, alt, content, n, reps):
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    if content == "smooth":
        imgs = [L.natural_image_np(W, H, 12, 12.0, 100 + s) for s in range(DISTINCT)]
    else:
        imgs = [rng.integers(0, 4096, size=(H, W), dtype=np.uint16) for _ in range(DISTINCT)]
    mos = torch.empty((n, H, W), dtype=torch.uint16, device=dev)
    for i in range(n):
        mos.view(torch.int16)[i].copy_(torch.from_numpy(imgs[i % DISTINCT].view(np.int16)))
    work = mos.clone()  # the in-place forms run on this copy (its contents drift from rep to rep; the time does not depend on them)
    gm = M.gain_map(float_gains())
    gm_per = M.gain_map(np.stack([float_gains(i) for i in range(n)]))
    to_dev = lambda a: torch.from_numpy(a.view(np.int16)).to(dev).view(torch.uint16)
    dmap, dmap_per = to_dev(gm), to_dev(gm_per)
    fg = torch.from_numpy(float_gains().astype(np.float32)).to(dev)
    out16 = torch.empty((n, H, W), dtype=torch.uint16, device=dev)
    out_bin2 = torch.empty((n, 3, H // 2, W // 2), dtype=torch.float16, device=dev)
    out_mhc = torch.empty((n, 3, H, W), dtype=torch.float16, device=dev)
    stream = torch.cuda.Stream()
    kw = dict(white=WHITE, black=BLACK, gain=GAIN, matrix=MAT)
    forms = FORMS + (ALT_FORMS if alt else [])

    def call(f):
        if f == "shade_out":
            return ctx.shade(mos, dmap, black=BLACK, top=TOP, out=out16)
        if f == "shade_inplace":
            return ctx.shade(work, dmap, black=BLACK, top=TOP, out=work)
        if f == "shade_out_perframe":
            return ctx.shade(mos, dmap_per, black=BLACK, top=TOP, out=out16)
        if f == "bin2_f16":
            return ctx.demosaic(mos, algo="bin2", dtype="f16", out=out_bin2, **kw)
        if f == "torch_ops":
            return torch_shade(mos, fg, BLACK, TOP)
        if f == "mhc_f16":
            return ctx.demosaic(mos, algo="mhc", dtype="f16", out=out_mhc, **kw)
        if f == "mhc_f16_shading":
            return ctx.demosaic(mos, algo="mhc", dtype="f16", out=out_mhc, shading=dmap, **kw)
        if f == "shade_out_alt":
            return alt.shade(mos, dmap, out16, stream, GW, GH, TOP, BLACK)
        if f == "shade_inplace_alt":
            return alt.shade(work, dmap, work, stream, GW, GH, TOP, BLACK)
        raise KeyError(f)

    want0 = S.shade_ref(imgs[0], gm, BLACK, TOP)
    bits = lambda t: t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    torch.cuda.synchronize()
    for f in forms:  # correctness of frame 0 of every form, and warm-up
        work.copy_(mos)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            res = call(f)
        torch.cuda.synchronize()
        if f in ("shade_out", "shade_out_alt"):
            assert np.array_equal(bits(out16[0]), want0), f
        elif f in ("shade_inplace", "shade_inplace_alt"):
            assert np.array_equal(bits(work[0]), want0), f
        elif f == "shade_out_perframe":
            assert np.array_equal(bits(out16[1]), S.shade_ref(imgs[1 % DISTINCT], gm_per[1], BLACK, TOP)), f
        elif f == "bin2_f16":
            assert np.array_equal(bits(out_bin2[0]), R.ref_bits(imgs[0], "bin2", "f16", WHITE, black=BLACK, gain=GAIN, matrix=MAT)), f
        elif f == "torch_ops":
            # float weights on unquantised gains against the contract's integers: the gains differ by at most
            # 1.5 + Dy (1/4096 + (H-1)/2^24) + Dx (1/4096 + (W-1)/2^24) < 3 LSB of Q12 for this map (tests/test_shade_abi.py),
            # times a sample of at most 4095 over 4096, plus a rounding on each side: within 4 codes
            assert np.abs(bits(res[0]).astype(np.int32) - want0.astype(np.int32)).max() <= 4, f
        elif f == "mhc_f16":
            assert np.array_equal(bits(out_mhc[0]), R.ref_bits(imgs[0], "mhc", "f16", WHITE, black=BLACK, gain=GAIN, matrix=MAT)), f
        else:
            assert np.array_equal(bits(out_mhc[0]), R.ref_bits(want0, "mhc", "f16", WHITE, black=BLACK, gain=GAIN, matrix=MAT)), f
        del res
    ms = {f: [] for f in forms}
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(reps):
        for f in forms:  # the forms take turns
            with torch.cuda.stream(stream):
                a.record(stream)
                res = call(f)
                b.record(stream)
            torch.cuda.synchronize()
            del res
            ms[f].append(a.elapsed_time(b))
    ctx.synchronize()
    assert ctx.errors() == 0
    mosaic_bytes = n * W * H * 2
    alg = {"bin2_f16": mosaic_bytes + n * 3 * (H // 2) * (W // 2) * 2, "mhc_f16": mosaic_bytes + n * 3 * H * W * 2,
           "mhc_f16_shading": mosaic_bytes + n * 3 * H * W * 2}  # (with shading=: the bytes of the result, not of the extra pass)
    rows = []
    for f in forms:
        total = alg.get(f, 2 * mosaic_bytes)  # the shade forms and the torch route: mosaic in + mosaic out
        med = float(np.median(ms[f]))
        rows.append({"content": content, "form": f, "frames": n, "width": W, "height": H, "map": "%dx%d" % (GW, GH), "reps": reps,
                     "batch_ms": round(med, 4), "batch_ms_min": round(min(ms[f]), 4), "batch_ms_max": round(max(ms[f]), 4),
                     "alg_GB": round(total / 1e9, 3), "frac_peak_batch": round(total / (med * 1e-3) / PEAK, 3)})
    by = {r["form"]: r for r in rows}
    target = {"content": content, "form": "target", "shade_out_frac": by["shade_out"]["frac_peak_batch"],
              "bin2_f16_frac": by["bin2_f16"]["frac_peak_batch"],
              "met": by["shade_out"]["frac_peak_batch"] >= by["bin2_f16"]["frac_peak_batch"],
              "separate_pass_ms": round(by["mhc_f16_shading"]["batch_ms"] - by["mhc_f16"]["batch_ms"], 4)}
    rows.append(target)
    del mos, work, out16, out_bin2, out_mhc
    torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--content", default="smooth,noise")
    ap.add_argument("--alt-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shade_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_shade.py needs a GPU")
    ctx = M.Context(0)
    alt = AltLib(args.alt_lib) if args.alt_lib else None
    with open(args.out, "a") as fh:
        for content in [c for c in args.content.split(",") if c]:
            for r in run(ctx, alt, content, args.frames, max(3, args.reps)):
                line = json.dumps(r)
                print(line, flush=True)
                fh.write(line + "\n")
    if alt:
        alt.close()
    ctx.close()


if __name__ == "__main__":
    main()
