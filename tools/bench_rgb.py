#!/usr/bin/env python3
"""Demosaic to planar linear RGB (mcraw_demosaic_batch) on HBM-resident mosaics, and decode_rgb end to end against the
plain uint16 decode of the same frames: ms per batch (events around the call on a torch stream), the kernel's ms from the
library's event brackets, algorithmic bytes (mosaic in + RGB out; for decode_rgb: compressed in + RGB out) and the fraction
of the 8 TB/s peak.  All forms take turns rep by rep in ONE process on one set of buffers.  Frames 0 and 1 of every form
are checked against the numpy reference.  Also times an MHC written as torch ops (F.conv2d with the four 5x5 filters) on
the same mosaics: what a user would otherwise write.

    python tools/bench_rgb.py [--reps 9] [--only t7_uhd,t6_12mp] [--alt-lib PATH]

--alt-lib: another build of the library (of another commit, say): its demosaic forms (*_alt) take turns with the others, in a
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
import torch.nn.functional as F

import _libs as L
import _rgb_ref as R
import motioncam_decoder_amd as M
from altlib import AltLib, bench_encoded, bench_images, bench_mosaics, turn_order

PEAK = 8e12
WHITE, BLACK = 4095.0, (64, 64, 64, 64)
GAIN = (2.0, 1.0, 1.6)
MAT = np.array([[1.7, -0.5, -0.2], [-0.25, 1.4, -0.15], [0.05, -0.45, 1.4]], np.float32)
ES = {"f32": 4, "f16": 2, "bf16": 2}
# form: (kind, algo, dtype); kind "demosaic" = the kernel on resident mosaics, "decode_rgb" = decode + demosaic, "plain" =
# the uint16 decode alone
FORMS = {"mhc_f16": ("demosaic", "mhc", "f16"), "mhc_f32": ("demosaic", "mhc", "f32"), "bin2_f16": ("demosaic", "bin2", "f16"),
         "plain": ("plain", None, None), "decode_rgb_mhc_f16": ("decode_rgb", "mhc", "f16")}
WORKLOADS = {  # name: (type, frames, width, height, forms)
    "t7_uhd": (7, 240, 3840, 2160, ["mhc_f16", "mhc_f32", "bin2_f16", "plain", "decode_rgb_mhc_f16"]),
    "t6_12mp": (6, 32, 4000, 3000, ["plain", "decode_rgb_mhc_f16"]),
}
DISTINCT = 4
DECODE_KERNEL = {7: "k7_tiles", 6: "k6_decode"}


def torch_mhc(mos, black, out_dtype):
    """MHC as torch ops (RGGB): four 5x5 filters by F.conv2d on the reflected mosaic, picked per CFA site."""
    k = torch.zeros((4, 1, 5, 5), dtype=torch.float32, device=mos.device)
    g = [[0, 0, -1, 0, 0], [0, 0, 2, 0, 0], [-1, 2, 4, 2, -1], [0, 0, 2, 0, 0], [0, 0, -1, 0, 0]]
    hz = [[0, 0, .5, 0, 0], [0, -1, 0, -1, 0], [-1, 4, 5, 4, -1], [0, -1, 0, -1, 0], [0, 0, .5, 0, 0]]
    dg = [[0, 0, -1.5, 0, 0], [0, 2, 0, 2, 0], [-1.5, 0, 6, 0, -1.5], [0, 2, 0, 2, 0], [0, 0, -1.5, 0, 0]]
    k[0, 0] = torch.tensor(g)
    k[1, 0] = torch.tensor(hz)
    k[2, 0] = torch.tensor(hz).t()
    k[3, 0] = torch.tensor(dg)
    k /= 8
    x = (mos.view(torch.int16).to(torch.int32) & 0xFFFF).to(torch.float32).unsqueeze(1) - float(black)
    y = F.conv2d(F.pad(x, (2, 2, 2, 2), mode="reflect"), k)
    n, _, h, w = y.shape
    c = x[:, 0]
    gg, hh, vv, dd = y[:, 0], y[:, 1], y[:, 2], y[:, 3]
    er = (torch.arange(h, device=mos.device) % 2 == 0)[:, None]
    ec = (torch.arange(w, device=mos.device) % 2 == 0)[None, :]
    rs, bs = er & ec, ~er & ~ec
    g1, g2 = er & ~ec, ~er & ec
    r = torch.where(rs, c, torch.where(g1, hh, torch.where(g2, vv, dd)))
    gch = torch.where(rs | bs, gg, c)
    b = torch.where(bs, c, torch.where(g1, vv, torch.where(g2, hh, dd)))
    return torch.stack([r, gch, b], 1).to(out_dtype)


def run(ctx, alt, name, reps):
    typ, n, w, h, forms = WORKLOADS[name]
    if alt:  # (the alt library's demosaic forms, each behind its counterpart)
        forms = [g for f in forms for g in ([f, f + "_alt"] if FORMS[f][0] == "demosaic" else [f])]
    dev = torch.device("cuda:0")
    imgs = bench_images("smooth", w, h, DISTINCT, None)
    ins, inputs, lens = bench_encoded(dev, imgs, n, L.encode7 if typ == 7 else L.encode6)
    mos = bench_mosaics(dev, imgs, n)
    out = torch.empty(n * 3 * w * h * 4, dtype=torch.uint8, device=dev)  # room for the largest form (MHC f32)
    plain_frames = M.Context.make_frames([(inputs[i][0], lens[i], w, h, typ, mos.data_ptr() + i * w * h * 2, w * h)
                                          for i in range(n)])
    stream = torch.cuda.Stream()  # (not the null stream: the library takes NULL as its own stream)

    def out_view(f):
        _, algo, dt = FORMS[f.replace("_alt", "")]
        ho, wo = (h, w) if algo == "mhc" else (h // 2, w // 2)
        t = out[: n * 3 * ho * wo * ES[dt]].view({"f32": torch.float32, "f16": torch.float16}[dt])
        return t.view(n, 3, ho, wo)

    def call(f, check):
        kind, algo, dt = FORMS[f.replace("_alt", "")]
        if f.endswith("_alt"):
            return alt.demosaic(mos, out_view(f), stream, algo, dt, WHITE, BLACK, GAIN, MAT)
        if kind == "plain":
            return ctx.decode_batch(plain_frames, stream=stream.cuda_stream, want_status=check)
        kw = dict(algo=algo, dtype=dt, white=WHITE, black=BLACK, gain=GAIN, matrix=MAT, out=out_view(f))
        if kind == "demosaic":
            return ctx.demosaic(mos, **kw)
        return ctx.decode_rgb(inputs, w, h, typ, check=check, **kw)

    torch.cuda.synchronize()
    for f in forms:  # correctness of every form, and warm-up
        with torch.cuda.stream(stream):
            res = call(f, True)
        torch.cuda.synchronize()
        if FORMS[f.replace("_alt", "")][0] == "plain":
            assert all(s == 0 for s in res[1]), (f, res[1][:8])
            continue
        _, algo, dt = FORMS[f.replace("_alt", "")]
        for i in range(2):
            got = out_view(f)[i].cpu().numpy().view(np.uint32 if dt == "f32" else np.uint16)
            want = R.ref_bits(imgs[i % DISTINCT], algo, dt, WHITE, black=BLACK, gain=GAIN, matrix=MAT)
            assert np.array_equal(got, want), (name, f, i)
    knames = ["krgb_mhc", "krgb_bin2", DECODE_KERNEL[typ]]
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
                call(f, False)
                b.record(stream)
            torch.cuda.synchronize()
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
    # the yardstick: MHC as torch ops, on the first frames (its intermediates do not fit a whole batch comfortably)
    nt = min(n, 16)
    tms = []
    for r in range(max(3, reps // 3) + 1):
        a.record()
        y = torch_mhc(mos[:nt], BLACK[0], torch.float16)
        b.record()
        torch.cuda.synchronize()
        if r:
            tms.append(a.elapsed_time(b))
        del y
    torch_ms_frame = float(np.median(tms)) / nt
    res = []
    inb = sum(lens)
    base = float(np.median(ms["plain"])) if "plain" in ms else None
    for f in forms:
        kind, algo, dt = FORMS[f.replace("_alt", "")]
        med = float(np.median(ms[f]))
        if kind == "plain":
            outb, inbytes = n * w * h * 2, inb
        else:
            ho, wo = (h, w) if algo == "mhc" else (h // 2, w // 2)
            outb = n * 3 * ho * wo * ES[dt]
            inbytes = n * w * h * 2 if kind == "demosaic" else inb
        nbytes = inbytes + outb
        r = {"workload": name, "form": f, "frames": n, "width": w, "height": h, "reps": reps,
             "batch_ms": round(med, 4), "batch_ms_min": round(min(ms[f]), 4), "batch_ms_max": round(max(ms[f]), 4),
             "alg_GB": round(nbytes / 1e9, 3), "frac_peak_batch": round(nbytes / (med * 1e-3) / PEAK, 3)}
        for k, v in km[f].items():
            kmed = float(np.median(v))
            r[k + "_ms"] = round(kmed, 4)
            if k.startswith("krgb"):
                kb = n * w * h * 2 + outb
                r["frac_peak_" + k] = round(kb / (kmed * 1e-3) / PEAK, 3)
        if base is not None and kind != "demosaic":
            r["vs_plain"] = round(med / base, 4)
        if f == "mhc_f16":
            r["torch_ops_mhc_f16_ms_per_frame"] = round(torch_ms_frame, 4)
            r["torch_ops_mhc_f16_ms_batch_est"] = round(torch_ms_frame * n, 3)
        res.append(r)
    del ins, out, mos
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--only", default="")
    ap.add_argument("--alt-lib", default=None)
    args = ap.parse_args()
    names = [s for s in args.only.split(",") if s] or list(WORKLOADS)
    ctx = M.Context(0)
    alt = AltLib(args.alt_lib) if args.alt_lib else None
    for name in names:
        for r in run(ctx, alt, name, max(3, args.reps)):
            print(json.dumps(r), flush=True)
    if alt:
        alt.close()
    ctx.close()


if __name__ == "__main__":
    main()
