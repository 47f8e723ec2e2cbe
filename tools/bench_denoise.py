#!/usr/bin/env python3
"""Denoising on HBM-resident mosaics (mcraw_denoise_batch) beside kshade out of place and kfixpix (the yardsticks: the same
algorithmic bytes, mosaic in + mosaic out, measured in the same run) and beside the same filter built from torch ops: ms per
batch (events around the call on a torch stream), algorithmic bytes and the fraction of the 8 TB/s peak.  240 UHD 12-bit
frames; all forms take turns rep by rep in ONE process; medians.  The first and the last frame of every library form are
checked against the numpy reference.  Appends to profiles/denoise_bench.jsonl.  Needs a GPU.

    python tools/bench_denoise.py [--reps 15] [--frames 240] [--alt-lib PATH [--alt-lib PATH ...]]

Forms:
  dn_r2_natural    natural images, radius 2, one noise_lut table for the batch
  dn_r1_natural    the same at radius 1
  dn_r2_noise      noise of the profile's own sigma around a level (weights across their whole range), radius 2
  dn_r1_noise      the same at radius 1
  dn_r2_perframe   the noise form with one table per frame (nluts == n)
  shade_out        kshade out of place on the natural frames (17 x 13 map)
  fixpix           kfixpix on the natural frames with the detection test's thresholds (nothing flagged)
  torch_ops        the radius-2 filter from torch ops (24 shifted copies, a gather, a division) on --torch-frames frames, scaled
--alt-lib: another build of the library (python -m motioncam_decoder_amd.build variant PATH -DMCRAW_DENOISE_TH=16, or
-DMCRAW_DENOISE_FLIP_STORES); its dn_r2_natural, dn_r2_noise and dn_r1_noise forms take turns with the others, in a context of
its own.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch

import _denoise_ref as D
import _libs as L
import _shade_ref as S
import motioncam_decoder_amd as M
from altlib import AltLib

PEAK = 8e12
W, H = 3840, 2160
PROFILE = dict(S=2e-4, O=2e-6, black=64, white=4095)
BLACK, ABS, REL = (64,) * 4, (96,) * 4, 26
DISTINCT = 4
LEVEL = 800.0
FORMS = ["dn_r2_natural", "dn_r1_natural", "dn_r2_noise", "dn_r1_noise", "dn_r2_perframe", "shade_out", "fixpix", "torch_ops"]
ALT_FORMS = ["dn_r2_natural", "dn_r2_noise", "dn_r1_noise"]


def torch_denoise(mos, lut, shift, radius):
    """What a user writes without the kernel: (2R + 1)^2 - 1 shifted copies (reflected edges), a gather, a division.  Interior
    pixels agree with the contract; the 4R edge rows and columns use torch's reflection."""
    n, h, w = mos.shape
    P = 2 * radius
    c = mos.to(torch.int64)
    pad = torch.nn.functional.pad(mos.to(torch.float32)[:, None], (P, P, P, P), mode="reflect")[:, 0].to(torch.int64)
    yy = torch.arange(h, device=mos.device)[:, None] & 1
    xx = torch.arange(w, device=mos.device)[None, :] & 1
    r = lut.to(torch.int64)[(yy * 2 + xx)[None].expand(n, h, w), (c >> shift).clamp_(max=lut.shape[1] - 1)]
    num, den = 256 * c, torch.full_like(c, 256)
    for dy, dx in D.offsets(radius):
        a = pad[:, P + dy:P + dy + h, P + dx:P + dx + w]
        x = (((a - c).abs() * r) >> 8).clamp_(max=16)
        wgt = 256 - x * x
        num += wgt * a
        den += wgt
    return torch.div(num + (den >> 1), den, rounding_mode="floor").to(torch.uint16)


def run(ctx, alts, n, reps, torch_frames):
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    nat = [L.natural_image_np(W, H, 12, 12.0, 100 + s) for s in range(DISTINCT)]
    R = PROFILE["white"] - PROFILE["black"]
    sigma = np.sqrt(PROFILE["S"] * R * (LEVEL - PROFILE["black"]) + PROFILE["O"] * R * R)
    noi = [np.clip(np.rint(LEVEL + sigma * rng.standard_normal((H, W))), 0, 4095).astype(np.uint16) for _ in range(DISTINCT)]

    def batch(imgs):
        t = torch.empty((n, H, W), dtype=torch.uint16, device=dev)
        for i in range(n):
            t.view(torch.int16)[i].copy_(torch.from_numpy(imgs[i % DISTINCT].view(np.int16)))
        return t

    mos_nat, mos_noi = batch(nat), batch(noi)
    out16 = torch.empty((n, H, W), dtype=torch.uint16, device=dev)
    lut, shift = M.noise_lut(**PROFILE)
    ends = (0, n - 1)
    per_ends = {i: M.noise_lut(strength=2.0 + 2.0 * i / max(n - 1, 1), **PROFILE)[0] for i in ends}
    per = np.stack([per_ends[i] if i in per_ends else M.noise_lut(strength=2.0 + 2.0 * i / max(n - 1, 1), **PROFILE)[0] for i in range(n)])
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(dev).view(torch.uint16)
    dlut, dper = up(lut), up(per)
    y, x = np.linspace(-1, 1, 13)[:, None], np.linspace(-1, 1, 17)[None, :]
    gm = M.gain_map(np.stack([1.0 + (s - 1.0) * (x * x + y * y) / 2 for s in (3.6, 2.9, 2.95, 3.9)]))
    dmap = up(gm)
    stream = torch.cuda.Stream()
    alt_forms = [(f + "@" + a.name, f, a) for a in alts for f in ALT_FORMS]
    forms = FORMS + [name for name, _, _ in alt_forms]
    alt_of = {name: (f, a) for name, f, a in alt_forms}
    tf = max(1, min(torch_frames, n))

    def call(f):
        if f in alt_of:
            base, a = alt_of[f]
            return a.denoise(mos_nat if base.endswith("natural") else mos_noi, out16, stream, dlut, shift, 2 if "_r2_" in base else 1)
        if f in ("dn_r2_natural", "dn_r1_natural"):
            return ctx.denoise(mos_nat, dlut, shift, radius=2 if "_r2_" in f else 1, out=out16)
        if f in ("dn_r2_noise", "dn_r1_noise"):
            return ctx.denoise(mos_noi, dlut, shift, radius=2 if "_r2_" in f else 1, out=out16)
        if f == "dn_r2_perframe":
            return ctx.denoise(mos_noi, dper, shift, radius=2, out=out16)
        if f == "shade_out":
            return ctx.shade(mos_nat, dmap, black=BLACK, top=65535, out=out16)
        if f == "fixpix":
            return ctx.fix_pixels(mos_nat, black=BLACK, abs_thr=ABS, rel_thr=REL / 256.0, rank=2, out=out16)
        if f == "torch_ops":
            return torch_denoise(mos_noi[:tf], dlut, shift, 2)
        raise KeyError(f)

    bits = lambda t: t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    want = {}  # (content, radius, table) -> {frame: reference}

    def reference(f):
        base = alt_of[f][0] if f in alt_of else f
        if not base.startswith("dn_"):
            return None
        key = (base.split("_")[2], 2 if "_r2_" in base else 1)
        if key not in want:
            src = nat if key[0] == "natural" else noi
            want[key] = {i: D.denoise(src[i % DISTINCT][None], per_ends[i] if key[0] == "perframe" else lut, shift, key[1])[0] for i in ends}
        return want[key]

    torch.cuda.synchronize()
    for f in forms:  # correctness of the first and the last frame of every form, and warm-up
        out16.zero_()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            res = call(f)
        torch.cuda.synchronize()
        ref = reference(f)
        for i in ends:
            if ref is not None:
                assert np.array_equal(bits(out16[i]), ref[i]), (f, i)
            elif f == "shade_out":
                assert np.array_equal(bits(out16[i]), S.shade_ref(nat[i % DISTINCT], gm, BLACK, 65535)), (f, i)
        if f == "torch_ops":  # the interior agrees with the contract (torch's reflection differs near the edges)
            assert np.array_equal(bits(res[0])[8:-8, 8:-8], reference("dn_r2_noise")[0][8:-8, 8:-8]), f
        del res
        print("checked", f, flush=True)
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
            ms[f].append(a.elapsed_time(b) * (n / tf if f == "torch_ops" else 1.0))
    ctx.synchronize()
    assert ctx.errors() == 0
    total = 2 * n * W * H * 2  # mosaic in + mosaic out
    rows = []
    for f in forms:
        med = float(np.median(ms[f]))
        row = {"form": f, "frames": n, "width": W, "height": H, "reps": reps, "batch_ms": round(med, 4),
               "batch_ms_min": round(min(ms[f]), 4), "batch_ms_max": round(max(ms[f]), 4), "alg_GB": round(total / 1e9, 3),
               "frac_peak_batch": round(total / (med * 1e-3) / PEAK, 3)}
        if f == "torch_ops":
            row["measured_frames"] = tf
        rows.append(row)
    by = {r["form"]: r["batch_ms"] for r in rows}
    ratios = {"form": "ratios"}
    for f in forms:
        if f.startswith("dn_"):
            ratios[f + "_over_shade"] = round(by[f] / by["shade_out"], 3)
            ratios[f + "_over_fixpix"] = round(by[f] / by["fixpix"], 3)
        if f in alt_of:
            ratios[f + "_over_default"] = round(by[f] / by[alt_of[f][0]], 3)
    ratios["torch_over_r2_noise"] = round(by["torch_ops"] / by["dn_r2_noise"], 1)
    rows.append(ratios)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--torch-frames", type=int, default=2)
    ap.add_argument("--alt-lib", action="append", default=[])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "denoise_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_denoise.py needs a GPU")
    ctx = M.Context(0)
    alts = [AltLib(p) for p in args.alt_lib]
    with open(args.out, "a") as fh:
        for r in run(ctx, alts, args.frames, max(3, args.reps), args.torch_frames):
            if alts:
                r["alt_libs"] = [a.name for a in alts]
            line = json.dumps(r)
            print(line, flush=True)
            fh.write(line + "\n")
    for a in alts:
        a.close()
    ctx.close()


if __name__ == "__main__":
    main()
