#!/usr/bin/env python3
"""Display-ready RGB (mcraw_demosaic_display_batch) on HBM-resident mosaics against the linear f16 demosaic and against the
same result built from torch ops: ms per batch (events around the call on a torch stream), the kernel's ms from the
library's event brackets, algorithmic bytes (mosaic in + output out; decode_display: compressed in + output out) and the
fraction of the 8 TB/s peak.  240 UHD 12-bit frames, smooth (natural images) and noise content; all forms take turns rep
by rep in ONE process.  Frame 0 of every form is checked against the numpy reference.  Appends to
profiles/display_bench.jsonl.

    python tools/bench_display.py [--reps 7] [--frames 240] [--content smooth,noise] [--alt-lib PATH]

--alt-lib: another build of the library (of another commit, say): its display forms (*_alt) take turns with the others, in a
context of its own, and are checked against the same reference.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch

import _display_ref as D
import _libs as L
import _rgb_ref as R
import motioncam_decoder_amd as M
from altlib import AltLib, bench_encoded, bench_images, bench_mosaics, turn_order

PEAK = 8e12
W, H = 3840, 2160
WHITE, BLACK = 4095.0, (64, 64, 64, 64)
GAIN = (2.0, 1.0, 1.6)
MAT = np.array([[1.7, -0.5, -0.2], [-0.25, 1.4, -0.15], [0.05, -0.45, 1.4]], np.float32)
DISTINCT = 4
# form: (kind, algo, out dtype, layout, LUT size); kind "linear" = demosaic f16 (the yardstick), "display" =
# demosaic_display, "decode" = decode_display, "torch" = demosaic f16 then sRGB, rounding and HWC as torch ops
FORMS = {
    "mhc_f16_chw_linear": ("linear", "mhc", "f16", "chw", 0),
    "mhc_u8_hwc_srgb4096": ("display", "mhc", "u8", "hwc", 4096),
    "mhc_u16_chw_lut65536": ("display", "mhc", "u16", "chw", 65536),
    "bin2_f16_chw_linear": ("linear", "bin2", "f16", "chw", 0),
    "bin2_u8_hwc_srgb4096": ("display", "bin2", "u8", "hwc", 4096),
    "decode_display_mhc_u8_hwc": ("decode", "mhc", "u8", "hwc", 4096),
    "torch_ops_mhc_u8_hwc": ("torch", "mhc", "u8", "hwc", 0),
}
ES = {"f16": 2, "u8": 1, "u16": 2}


def torch_srgb_u8_hwc(lin):
    """What a user writes after decode_rgb: clamp, sRGB OETF, x 255, round, (N, H, W, 3) contiguous uint8."""
    x = lin.float().clamp_(0.0, 1.0)
    y = torch.where(x <= 0.0031308, 12.92 * x, 1.055 * torch.pow(x, 1.0 / 2.4) - 0.055)
    return torch.round(y * 255.0).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def run(ctx, alt, content, n, reps):
    dev = torch.device("cuda:0")
    imgs = bench_images(content, W, H, DISTINCT, np.random.default_rng(7))
    mos = bench_mosaics(dev, imgs, n)
    forms = [f for f in FORMS if content == "smooth" or FORMS[f][0] != "decode"]
    if alt:  # (the alt library's display forms, each behind its counterpart)
        forms = [g for f in forms for g in ([f, f + "_alt"] if FORMS[f][0] == "display" else [f])]
    ins, inputs, inb = None, None, 0
    if any(FORMS[f.replace("_alt", "")][0] == "decode" for f in forms):
        ins, inputs, lens = bench_encoded(dev, imgs, n, L.encode7)
        inb = sum(lens)
    out = torch.empty(n * 3 * W * H * 2, dtype=torch.uint8, device=dev)  # room for the largest form (f16 / u16 MHC)
    stream = torch.cuda.Stream()
    lut16 = M.transfer_lut("srgb", 65536, 16)
    to_dev = lambda a: torch.from_numpy(a.view(np.int16)).to(dev).view(torch.uint16)
    alt_luts = {4096: to_dev(M.transfer_lut("srgb", 4096, 8)), 65536: to_dev(lut16)} if alt else None

    def out_view(f):
        kind, algo, dt, layout, _ = FORMS[f.replace("_alt", "")]
        ho, wo = (H, W) if algo == "mhc" else (H // 2, W // 2)
        shape = (n, ho, wo, 3) if layout == "hwc" else (n, 3, ho, wo)
        t = out[: n * 3 * ho * wo * ES[dt]]
        t = t.view(torch.float16) if dt == "f16" else t.view(torch.uint16) if dt == "u16" else t
        return t.view(shape)

    def call(f):
        kind, algo, dt, layout, size = FORMS[f.replace("_alt", "")]
        if f.endswith("_alt"):
            return alt.demosaic_display(mos, out_view(f), stream, algo, alt_luts[size], layout, WHITE, BLACK, GAIN, MAT)
        kw = dict(algo=algo, white=WHITE, black=BLACK, gain=GAIN, matrix=MAT)
        if kind == "linear":
            return ctx.demosaic(mos, dtype="f16", out=out_view(f), **kw)
        if kind == "torch":
            return torch_srgb_u8_hwc(ctx.demosaic(mos, dtype="f16", **kw))
        transfer = "srgb" if size == 4096 else lut16
        dkw = dict(transfer=transfer, lut_size=size, dtype=torch.uint8 if dt == "u8" else torch.uint16, layout=layout,
                   out=out_view(f), **kw)
        if kind == "display":
            return ctx.demosaic_display(mos, **dkw)
        return ctx.decode_display(inputs, W, H, 7, check=False, **dkw)

    torch.cuda.synchronize()
    for f in forms:  # correctness of frame 0 of every form, and warm-up
        kind, algo, dt, layout, size = FORMS[f.replace("_alt", "")]
        with torch.cuda.stream(stream):
            res = call(f)
        torch.cuda.synchronize()
        if kind == "linear":
            want = R.ref_bits(imgs[0], algo, "f16", WHITE, black=BLACK, gain=GAIN, matrix=MAT)
            assert np.array_equal(out_view(f)[0].cpu().numpy().view(np.uint16), want), f
        elif kind == "torch":
            del res
        else:
            lut = M.transfer_lut("srgb", 4096, 8) if size == 4096 else lut16
            want = D.display_ref(imgs[0], algo, WHITE, lut, dt, layout, BLACK, "rggb", GAIN, MAT)
            got = out_view(f)[0]
            got = got.view(torch.int16).cpu().numpy().view(np.uint16) if dt == "u16" else got.cpu().numpy()
            assert np.array_equal(got, want), f
    knames = ["krgb_mhc", "krgb_bin2", "k7_tiles"]
    ctx.profile(only=knames)
    if alt:
        alt.profile(knames[:2])
    for k in knames:
        ctx.kernel_ms(k, reset=True)
    ms = {f: [] for f in forms}
    km = {f: {} for f in forms}
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rep in range(reps):
        for f in turn_order(forms, rep):  # the forms take turns
            with torch.cuda.stream(stream):
                a.record(stream)
                res = call(f)
                b.record(stream)
            torch.cuda.synchronize()
            del res
            ms[f].append(a.elapsed_time(b))
            for k in knames:
                v, cnt = (alt if f.endswith("_alt") else ctx).kernel_ms(k, reset=True)
                if cnt:
                    km[f].setdefault(k, []).append(v)
    ctx.profile(enable=False)
    if alt:
        alt.profile(())
    ctx.synchronize()
    assert ctx.errors() == 0
    rows = []
    for f in forms:
        kind, algo, dt, layout, size = FORMS[f.replace("_alt", "")]
        ho, wo = (H, W) if algo == "mhc" else (H // 2, W // 2)
        outb = n * 3 * ho * wo * ES[dt]
        inbytes = inb if kind == "decode" else n * W * H * 2
        med = float(np.median(ms[f]))
        r = {"content": content, "form": f, "frames": n, "width": W, "height": H, "reps": reps, "lut": size,
             "batch_ms": round(med, 4), "batch_ms_min": round(min(ms[f]), 4), "batch_ms_max": round(max(ms[f]), 4),
             "alg_GB": round((inbytes + outb) / 1e9, 3), "frac_peak_batch": round((inbytes + outb) / (med * 1e-3) / PEAK, 3)}
        for k, v in km[f].items():
            kmed = float(np.median(v))
            r[k + "_ms"] = round(kmed, 4)
            if k.startswith("krgb"):
                kb = n * W * H * 2 + outb if kind != "torch" else n * W * H * 2 + n * 3 * ho * wo * 2
                r["frac_peak_" + k] = round(kb / (kmed * 1e-3) / PEAK, 3)
        rows.append(r)
    del mos, out
    torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--content", default="smooth,noise")
    ap.add_argument("--alt-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "display_bench.jsonl"))
    args = ap.parse_args()
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
