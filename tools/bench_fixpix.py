#!/usr/bin/env python3
"""Defective pixels on HBM-resident mosaics (mcraw_fixpix_batch) beside kshade out of place (the yardstick: the same
algorithmic bytes, mosaic in + mosaic out, measured in the same run) and beside the same correction built from torch ops: ms
per batch (events around the call on a torch stream), algorithmic bytes and the fraction of the 8 TB/s peak.  240 UHD 12-bit
frames; all forms take turns rep by rep in ONE process; medians.  The first and the last frame of every library form are
checked against the numpy reference.  Appends to profiles/fixpix_bench.jsonl.  Needs a GPU.

    python tools/bench_fixpix.py [--reps 15] [--frames 240] [--alt-lib PATH]

Forms:
  fixpix_natural   natural images, the thresholds of the detection test (black 64, abs 96, rel 26/256): nothing is flagged
  fixpix_noise     uniform noise, all thresholds 0: the replacement path on about four pixels in nine
  fixpix_list      the natural form with a 4096-entry static list
  fixpix_counts    the natural form with the counts
  shade_out        kshade out of place on the natural frames (17 x 13 map)
  torch_ops        the dynamic pass from torch ops (eight shifted copies, sort) on --torch-frames frames, scaled to the batch
--alt-lib: another build of the library (python -m motioncam_decoder_amd.build variant PATH -DMCRAW_FIXPIX_TH=16, or
-DMCRAW_FIXPIX_FLIP_STORES); its natural and noise forms take turns with the others, in a context of its own.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch

import _fixpix_ref as F
import _libs as L
import _shade_ref as S
import motioncam_decoder_amd as M
from altlib import AltLib

PEAK = 8e12
W, H = 3840, 2160
BLACK, ABS, REL = (64,) * 4, (96,) * 4, 26
DISTINCT = 4
NLIST = 4096
FORMS = ["fixpix_natural", "fixpix_noise", "fixpix_list", "fixpix_counts", "shade_out", "torch_ops"]
ALT_FORMS = ["fixpix_natural_alt", "fixpix_noise_alt"]


def torch_fixpix(mos, black, abs_thr, rel, rank):
    """What a user writes without the kernel: eight shifted copies (reflected edges), a sort, the thresholds, the four pair
    means.  Interior pixels agree with the contract; the two edge rows and columns use torch's reflection."""
    n, h, w = mos.shape
    v = mos.to(torch.int32)
    pad = torch.nn.functional.pad(v.to(torch.float32)[:, None], (2, 2, 2, 2), mode="reflect")[:, 0].to(torch.int32)
    nb = [pad[:, 2 + dy:2 + dy + h, 2 + dx:2 + dx + w] for dy, dx in F.NEIGHBOURS]
    srt = torch.sort(torch.stack(nb), dim=0).values
    Hk, Lk = srt[8 - rank], srt[rank - 1]
    yy = torch.arange(h, device=mos.device)[:, None] & 1
    xx = torch.arange(w, device=mos.device)[None, :] & 1
    p = yy * 2 + xx
    b = torch.tensor(black, device=mos.device, dtype=torch.int32)[p]
    a = torch.tensor(abs_thr, device=mos.device, dtype=torch.int32)[p]
    thr = lambda m: a + (((m - b).clamp_(min=0).to(torch.int64) * rel) >> 8).to(torch.int32)
    flag = ((v > Hk) & (v - Hk > thr(Hk))) | ((v < Lk) & (Lk - v > thr(Lk)))
    best, val = None, None
    for i, j in F.PAIRS:
        d, m = (nb[i] - nb[j]).abs(), (nb[i] + nb[j] + 1) >> 1
        if best is None:
            best, val = d, m
        else:
            val = torch.where(d < best, m, val)
            best = torch.minimum(best, d)
    return torch.where(flag, val, v).to(torch.uint16)


def run(ctx, alt, n, reps, torch_frames):
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    nat = [L.natural_image_np(W, H, 12, 12.0, 100 + s) for s in range(DISTINCT)]
    noi = [L.uniform_image_np(W, H, 12, 200 + s) for s in range(DISTINCT)]

    def batch(imgs):
        t = torch.empty((n, H, W), dtype=torch.uint16, device=dev)
        for i in range(n):
            t.view(torch.int16)[i].copy_(torch.from_numpy(imgs[i % DISTINCT].view(np.int16)))
        return t

    mos_nat, mos_noi = batch(nat), batch(noi)
    out16 = torch.empty((n, H, W), dtype=torch.uint16, device=dev)
    lst = M.pack_pixels(np.stack([rng.integers(0, W, 2 * NLIST), rng.integers(0, H, 2 * NLIST)], axis=1))[:NLIST]
    dlist = torch.from_numpy(lst.view(np.int32)).to(dev)
    y, x = np.linspace(-1, 1, 13)[:, None], np.linspace(-1, 1, 17)[None, :]
    gm = M.gain_map(np.stack([1.0 + (s - 1.0) * (x * x + y * y) / 2 for s in (3.6, 2.9, 2.95, 3.9)]))
    dmap = torch.from_numpy(gm.view(np.int16)).to(dev).view(torch.uint16)
    stream = torch.cuda.Stream()
    nat_kw = dict(black=BLACK, abs_thr=ABS, rel_thr=REL / 256.0, rank=2)
    forms = FORMS + (ALT_FORMS if alt else [])
    tf = max(1, min(torch_frames, n))

    def call(f):
        if f == "fixpix_natural":
            return ctx.fix_pixels(mos_nat, out=out16, **nat_kw)
        if f == "fixpix_noise":
            return ctx.fix_pixels(mos_noi, abs_thr=0, rank=2, out=out16)
        if f == "fixpix_list":
            return ctx.fix_pixels(mos_nat, pixels=dlist, out=out16, **nat_kw)
        if f == "fixpix_counts":
            return ctx.fix_pixels(mos_nat, counts=True, out=out16, **nat_kw)
        if f == "shade_out":
            return ctx.shade(mos_nat, dmap, black=BLACK, top=65535, out=out16)
        if f == "torch_ops":
            return torch_fixpix(mos_nat[:tf], BLACK, ABS, REL, 2)
        if f == "fixpix_natural_alt":
            return alt.fix(mos_nat, out16, stream, BLACK, ABS, REL)
        if f == "fixpix_noise_alt":
            return alt.fix(mos_noi, out16, stream, (0,) * 4, (0,) * 4, 0)
        raise KeyError(f)

    bits = lambda t: t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    ends = (0, n - 1)
    want_nat = {i: F.fixpix(nat[i % DISTINCT][None], 3, 2, REL, BLACK, ABS) for i in ends}
    want_noi = {i: F.fixpix(noi[i % DISTINCT][None], 3, 2, 0) for i in ends}
    want_lst = {i: F.fixpix(nat[i % DISTINCT][None], 3, 2, REL, BLACK, ABS, lst) for i in ends}
    flagged = {"natural": int(want_nat[0][1].sum()), "noise": int(want_noi[0][1].sum())}
    torch.cuda.synchronize()
    for f in forms:  # correctness of the first and the last frame of every form, and warm-up
        out16.zero_()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            res = call(f)
        torch.cuda.synchronize()
        for i in ends:
            if f in ("fixpix_natural", "fixpix_natural_alt"):
                assert np.array_equal(bits(out16[i]), want_nat[i][0][0]), (f, i)
            elif f in ("fixpix_noise", "fixpix_noise_alt"):
                assert np.array_equal(bits(out16[i]), want_noi[i][0][0]), (f, i)
            elif f == "fixpix_list":
                assert np.array_equal(bits(out16[i]), want_lst[i][0][0]), (f, i)
            elif f == "fixpix_counts":
                assert np.array_equal(bits(out16[i]), want_nat[i][0][0]), (f, i)
                assert np.array_equal(res[1][i].cpu().numpy().view(np.uint32), want_nat[i][1][0]), (f, i)
            elif f == "shade_out":
                assert np.array_equal(bits(out16[i]), S.shade_ref(nat[i % DISTINCT], gm, BLACK, 65535)), (f, i)
        if f == "torch_ops":  # the interior agrees with the contract (torch's reflection differs in the two edge rows / columns)
            assert np.array_equal(bits(res[0])[2:-2, 2:-2], want_nat[0][0][0][2:-2, 2:-2]), f
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
    rows.append({"form": "ratios", "natural_over_shade": round(by["fixpix_natural"] / by["shade_out"], 3),
                 "noise_over_shade": round(by["fixpix_noise"] / by["shade_out"], 3),
                 "noise_over_natural": round(by["fixpix_noise"] / by["fixpix_natural"], 3),
                 "list_over_natural": round(by["fixpix_list"] / by["fixpix_natural"], 3),
                 "counts_over_natural": round(by["fixpix_counts"] / by["fixpix_natural"], 3),
                 "torch_over_natural": round(by["torch_ops"] / by["fixpix_natural"], 1),
                 "flagged_frame0": flagged})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--torch-frames", type=int, default=2)
    ap.add_argument("--alt-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fixpix_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_fixpix.py needs a GPU")
    ctx = M.Context(0)
    alt = AltLib(args.alt_lib) if args.alt_lib else None
    with open(args.out, "a") as fh:
        for r in run(ctx, alt, args.frames, max(3, args.reps), args.torch_frames):
            if alt:
                r["alt_lib"] = os.path.basename(args.alt_lib)
            line = json.dumps(r)
            print(line, flush=True)
            fh.write(line + "\n")
    if alt:
        alt.close()
    ctx.close()


if __name__ == "__main__":
    main()
