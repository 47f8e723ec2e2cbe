#!/usr/bin/env python3
"""NV12 / P010 output (mcraw_demosaic_yuv_batch) on HBM-resident mosaics beside the display-ready u8 HWC kernels (the
yardsticks, measured in the same run) and beside the same NV12 built from torch ops on demosaic_display's u8 CHW result:
ms per batch (events around the call on a torch stream), the kernel's ms from the library's event brackets
(Context.kernel_ms), algorithmic bytes (mosaic in + samples out) and the fraction of the 8 TB/s peak.  240 UHD 12-bit
frames, smooth (natural images) and noise content; all forms take turns rep by rep in ONE process.  Frame 0 of every
library form is checked against the numpy reference.  Appends to profiles/yuv_bench.jsonl.  Needs a GPU.

    python tools/bench_yuv.py [--reps 7] [--frames 240] [--content smooth,noise] [--alt-lib PATH]

--alt-lib: another build of the library (of another commit, say): its display and YUV forms (*_alt) take turns with the others,
in a context of its own, and are checked against the same reference.
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
import _yuv_ref as Y
import motioncam_decoder_amd as M
from altlib import AltLib, bench_images, bench_mosaics, turn_order

PEAK = 8e12
W, H = 3840, 2160
WHITE, BLACK = 4095.0, (64, 64, 64, 64)
GAIN = (2.0, 1.0, 1.6)
MAT = np.array([[1.7, -0.5, -0.2], [-0.25, 1.4, -0.15], [0.05, -0.45, 1.4]], np.float32)
DISTINCT = 4
# form: (kind, algo, format); kind "display" = demosaic_display u8 HWC (the yardsticks), "yuv" = demosaic_yuv, "torch" =
# demosaic_display u8 CHW, then matmul, avg_pool2d, round, clamp, interleave and cat as torch ops
FORMS = {
    "mhc_u8_hwc_display": ("display", "mhc", "u8"),
    "mhc_nv12": ("yuv", "mhc", "nv12"),
    "mhc_p010": ("yuv", "mhc", "p010"),
    "bin2_u8_hwc_display": ("display", "bin2", "u8"),
    "bin2_nv12": ("yuv", "bin2", "nv12"),
    "bin2_p010": ("yuv", "bin2", "p010"),
    "torch_ops_mhc_nv12": ("torch", "mhc", "nv12"),
}
IN_BITS = {"nv12": 12, "p010": 16}


def samples_out(kind, algo, fmt, n):
    ho, wo = (H, W) if algo == "mhc" else (H // 2, W // 2)
    return n * ho * wo * 3 if kind == "display" else n * ho * wo * 3 // 2 * (2 if fmt == "p010" else 1)


def torch_nv12(rgb):
    """What a user writes behind demosaic_display(layout="chw"): BT.709 limited-range matrix in f32, 2x2 average of the
    chroma, round, clamp, interleave Cb / Cr, and the planes behind each other: (N, H * 3 // 2, W) uint8."""
    n, _, h, w = rgb.shape
    kr, kb = 0.2126, 0.0722
    kg = 1.0 - kr - kb
    m = torch.tensor([[kr, kg, kb], [-kr / (2 * (1 - kb)), -kg / (2 * (1 - kb)), 0.5], [0.5, -kg / (2 * (1 - kr)), -kb / (2 * (1 - kr))]],
                     dtype=torch.float32, device=rgb.device)
    m = m * torch.tensor([[219.0], [224.0], [224.0]], device=rgb.device) / 255.0
    ycc = torch.matmul(m, rgb.float().reshape(n, 3, h * w)).reshape(n, 3, h, w)
    y = torch.round(ycc[:, 0] + 16.0).clamp_(0, 255).to(torch.uint8)
    c = torch.nn.functional.avg_pool2d(ycc[:, 1:], 2)
    c = torch.round(c + 128.0).clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).reshape(n, h // 2, w)
    return torch.cat([y, c], dim=1)


def run(ctx, alt, content, n, reps):
    dev = torch.device("cuda:0")
    imgs = bench_images(content, W, H, DISTINCT, np.random.default_rng(7))
    mos = bench_mosaics(dev, imgs, n)
    forms = list(FORMS)
    if alt:  # (the alt library's display and YUV forms, each behind its counterpart)
        forms = [g for f in forms for g in ([f, f + "_alt"] if FORMS[f][0] != "torch" else [f])]
    to_dev = lambda a: torch.from_numpy(a.view(np.int16)).to(dev).view(torch.uint16)
    alt_luts = {b: to_dev(M.transfer_lut("bt709", 4096, b)) for b in (8, 12, 16)} if alt else None
    out = torch.empty(n * 3 * W * H, dtype=torch.uint8, device=dev)  # room for the largest form (u8 HWC and P010, MHC)
    stream = torch.cuda.Stream()

    def out_view(f):
        kind, algo, fmt = FORMS[f.replace("_alt", "")]
        ho, wo = (H, W) if algo == "mhc" else (H // 2, W // 2)
        t = out[: samples_out(kind, algo, fmt, n)]
        if kind == "display":
            return t.view(n, ho, wo, 3)
        return (t.view(torch.uint16) if fmt == "p010" else t).view(n, ho * 3 // 2, wo)

    def call(f):
        kind, algo, fmt = FORMS[f.replace("_alt", "")]
        if f.endswith("_alt") and kind == "display":
            return alt.demosaic_display(mos, out_view(f), stream, algo, alt_luts[8], "hwc", WHITE, BLACK, GAIN, MAT)
        if f.endswith("_alt"):
            return alt.demosaic_yuv(mos, out_view(f), stream, algo, alt_luts[IN_BITS[fmt]], fmt, IN_BITS[fmt], WHITE, BLACK, GAIN, MAT)
        kw = dict(algo=algo, white=WHITE, black=BLACK, gain=GAIN, matrix=MAT)
        if kind == "display":
            return ctx.demosaic_display(mos, transfer="bt709", lut_size=4096, dtype=torch.uint8, layout="hwc", out=out_view(f), **kw)
        if kind == "torch":
            return torch_nv12(ctx.demosaic_display(mos, transfer="bt709", lut_size=4096, dtype=torch.uint8, layout="chw", **kw))
        return ctx.demosaic_yuv(mos, fmt=fmt, standard="bt709", range="limited", transfer="bt709", lut_size=4096, out=out_view(f), **kw)

    torch.cuda.synchronize()
    for f in forms:  # correctness of frame 0 of every library form, and warm-up
        kind, algo, fmt = FORMS[f.replace("_alt", "")]
        with torch.cuda.stream(stream):
            res = call(f)
        torch.cuda.synchronize()
        if kind == "display":
            want = D.display_ref(imgs[0], algo, WHITE, M.transfer_lut("bt709", 4096, 8), "u8", "hwc", BLACK, "rggb", GAIN, MAT)
            assert np.array_equal(out_view(f)[0].cpu().numpy(), want), f
        elif kind == "yuv":
            coef = M.yuv_matrix("bt709", "limited", Y.BITS[fmt], IN_BITS[fmt])
            want = Y.yuv_ref(imgs[0], algo, WHITE, M.transfer_lut("bt709", 4096, IN_BITS[fmt]), fmt, coef, IN_BITS[fmt], BLACK,
                             "rggb", GAIN, MAT)
            got = out_view(f)[0]
            got = got.view(torch.int16).cpu().numpy().view(np.uint16) if fmt == "p010" else got.cpu().numpy()
            assert np.array_equal(got, want), f
        else:  # the torch route rounds twice (to 8-bit R'G'B', then to codes): within 2 codes of the fused result
            coef = M.yuv_matrix("bt709", "limited", 8, 12)
            want = Y.yuv_ref(imgs[0], algo, WHITE, M.transfer_lut("bt709", 4096, 12), "nv12", coef, 12, BLACK, "rggb", GAIN, MAT)
            assert np.abs(res[0].cpu().numpy().astype(np.int32) - want.astype(np.int32)).max() <= 2, f
        del res
    knames = ["krgb_mhc", "krgb_bin2"]
    ctx.profile(only=knames)
    if alt:
        alt.profile(knames)
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
        kind, algo, fmt = FORMS[f.replace("_alt", "")]
        outb = samples_out("display" if kind == "torch" else kind, algo, fmt, n)  # (torch: what its kernel writes, u8 CHW)
        total = n * W * H * 2 + (samples_out("yuv", algo, fmt, n) if kind == "torch" else outb)
        med = float(np.median(ms[f]))
        r = {"content": content, "form": f, "frames": n, "width": W, "height": H, "reps": reps, "lut": 4096,
             "batch_ms": round(med, 4), "batch_ms_min": round(min(ms[f]), 4), "batch_ms_max": round(max(ms[f]), 4),
             "alg_GB": round(total / 1e9, 3), "frac_peak_batch": round(total / (med * 1e-3) / PEAK, 3)}
        for k, v in km[f].items():
            kmed = float(np.median(v))
            r[k + "_ms"] = round(kmed, 4)
            r["frac_peak_" + k] = round((n * W * H * 2 + outb) / (kmed * 1e-3) / PEAK, 3)
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "yuv_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_yuv.py needs a GPU")
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
