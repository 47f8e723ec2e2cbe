#!/usr/bin/env python3
"""Temporal merge on HBM-resident mosaics (mcraw_merge_batch) beside kshade out of place and kdenoise at radius 1 (measured in
the same run) and beside the same merge built from torch ops: ms per batch (events around the call on a torch stream), the
algorithmic bytes (every input frame read once, every output written once) and the fraction of the 8 TB/s peak.  240 UHD
12-bit frames; all forms take turns rep by rep in ONE process; medians.  Row bands of the first and the last output of every
library form are checked against the numpy reference.  Appends to profiles/merge_bench.jsonl.  Needs a GPU.

    python tools/bench_merge.py [--reps 15] [--frames 240] [--alt-lib PATH [--alt-lib PATH ...]] [--fetched-bytes FORM=BYTES ...]

Forms:
  mg_w5_s0_noise ... mg_w9_s1_natural        a sliding window of 5 or 9 frames (before = after = 2 or 4, count = n), support 0
                                             or 1, on static noise of the profile's own sigma or on a natural image that moves
                                             by (2, 6) pixels per frame
  ..._shift                                  the same with positions that follow that motion: shifts that are no multiples of 8
  mg_burst                                   the burst form: frames / 16 stacks of 16 frames onto their first (support 1)
  shade_out                                  kshade out of place on the natural frames (17 x 13 map)
  dn_r1                                      kdenoise at radius 1 on the noise frames
  torch_ops                                  the window-5, support-1 merge from torch ops on --torch-frames outputs, scaled
--alt-lib: another build of the library (python -m motioncam_decoder_amd.build variant PATH -DMCRAW_MERGE_TH=16, or
-DMCRAW_MERGE_FLIP_STORES); its mg_w5_s1_noise, mg_w9_s1_noise and mg_w5_s0_noise forms take turns with the others, in a context
of its own.  --fetched-bytes: the bytes a memory-side counter run of its own (one form per run) saw fetched for a form; the
row then carries their ratio to the algorithmic input bytes.
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
import _merge_ref as R
import _shade_ref as S
import motioncam_decoder_amd as M
from altlib import AltLib

PEAK = 8e12
W, H = 3840, 2160
PROFILE = dict(S=2e-4, O=2e-6, black=64, white=4095)
BLACK = (64,) * 4
DISTINCT = 8
LEVEL = 800.0
STEP = (2, 6)  # the natural image moves by this much per frame, modulo DISTINCT frames
BAND, MARGIN = 128, 32
MERGE_FORMS = ["mg_w%d_s%d_%s%s" % (w, s, c, sh) for sh in ("", "_shift") for c in ("noise", "natural") for w in (5, 9) for s in (0, 1)]
FORMS = MERGE_FORMS + ["mg_burst", "shade_out", "dn_r1", "torch_ops"]
ALT_FORMS = ["mg_w5_s1_noise", "mg_w9_s1_noise", "mg_w5_s0_noise"]


def torch_merge(mos, lut, shift, T, first, count):
    """What a user writes without the kernel (support 1, no shifts): per member a difference, a nine-term sum over shifted copies
    with the edge rule, a gather, and a division at the end."""
    n, h, w = mos.shape
    yy = torch.arange(h, device=mos.device)[:, None] & 1
    xx = torch.arange(w, device=mos.device)[None, :] & 1
    outs = []
    for b in range(first, first + count):
        c = mos[b].to(torch.int64)
        r = lut.to(torch.int64)[yy * 2 + xx, (c >> shift).clamp_(max=lut.shape[1] - 1)]
        num, den = 256 * c, torch.full_like(c, 256)
        ones = torch.nn.functional.pad(torch.ones_like(c), (1, 1, 1, 1))
        nv = sum(ones[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3))
        for t in range(max(0, b - T), min(n - 1, b + T) + 1):
            if t == b:
                continue
            a = mos[t].to(torch.int64)
            e0 = a - c
            e = torch.nn.functional.pad(e0, (1, 1, 1, 1))
            s = sum(e[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)) + (9 - nv) * e0
            D = torch.maximum((s.abs() >> 3).clamp_(max=65535), e0.abs() >> 1)
            x = ((D * r) >> 8).clamp_(max=16)
            wgt = 256 - x * x
            num += wgt * a
            den += wgt
        outs.append(torch.div(num + (den >> 1), den, rounding_mode="floor").to(torch.uint16))
    return torch.stack(outs)


def parse(form):
    """(window half, support, content, shifted) of a merge form's name."""
    p = form.split("@")[0].split("_")
    return (int(p[1][1:]) - 1) // 2, int(p[2][1:]), p[3], len(p) > 4


def run(ctx, alts, n, reps, torch_frames, fetched):
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    Rg = PROFILE["white"] - PROFILE["black"]
    sigma = np.sqrt(PROFILE["S"] * Rg * (LEVEL - PROFILE["black"]) + PROFILE["O"] * Rg * Rg)
    noi = [np.clip(np.rint(LEVEL + sigma * rng.standard_normal((H, W))), 0, 4095).astype(np.uint16) for _ in range(DISTINCT)]
    scene = L.natural_image_np(W, H, 12, 12.0, 100)
    nat = [np.roll(scene, (STEP[0] * k, STEP[1] * k), axis=(0, 1)) for k in range(DISTINCT)]
    src = {"noise": lambda i: noi[i % DISTINCT], "natural": lambda i: nat[i % DISTINCT]}
    pos = np.array([[STEP[0] * (i % DISTINCT), STEP[1] * (i % DISTINCT)] for i in range(n)])

    def batch(imgs):
        t = torch.empty((n, H, W), dtype=torch.uint16, device=dev)
        for i in range(n):
            t.view(torch.int16)[i].copy_(torch.from_numpy(imgs[i % DISTINCT].view(np.int16)))
        return t

    mos = {"noise": batch(noi), "natural": batch(nat)}
    out16 = torch.empty((n, H, W), dtype=torch.uint16, device=dev)
    lut, shift = M.noise_lut(**PROFILE)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(dev).view(torch.uint16)
    dlut = up(lut)
    dpos = torch.from_numpy(pos.astype(np.int16)).to(dev)
    y, x = np.linspace(-1, 1, 13)[:, None], np.linspace(-1, 1, 17)[None, :]
    gm = M.gain_map(np.stack([1.0 + (s - 1.0) * (x * x + y * y) / 2 for s in (3.6, 2.9, 2.95, 3.9)]))
    dmap = up(gm)
    stream = torch.cuda.Stream()
    alt_forms = [(f + "@" + a.name, f, a) for a in alts for f in ALT_FORMS]
    forms = FORMS + [name for name, _, _ in alt_forms]
    alt_of = {name: (f, a) for name, f, a in alt_forms}
    tf = max(1, min(torch_frames, n - 4))
    nb = n // 16

    def call(f):
        if f in alt_of:
            T, support, content, _ = parse(f)
            return alt_of[f][1].merge(mos[content], out16, stream, dlut, shift, T, support)
        if f.startswith("mg_w"):
            T, support, content, shifted = parse(f)
            return ctx.merge(mos[content], dlut, shift, before=T, after=T, support=support, pos=dpos if shifted else None, out=out16)
        if f == "mg_burst":
            return [ctx.stack(mos["noise"][16 * k:16 * k + 16], dlut, shift, out=out16[k]) for k in range(nb)]
        if f == "shade_out":
            return ctx.shade(mos["natural"], dmap, black=BLACK, top=65535, out=out16)
        if f == "dn_r1":
            return ctx.denoise(mos["noise"], dlut, shift, radius=1, out=out16)
        if f == "torch_ops":
            return torch_merge(mos["noise"][:tf + 4], dlut, shift, 2, 2, tf)
        raise KeyError(f)

    bits = lambda t: t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)

    def band_ok(got, want_of, rows):
        """Compare BAND rows at the top (rows = 0) or the bottom of an output with the reference made on a crop MARGIN rows taller
        (the rows next to the cut read members that the crop does not hold)."""
        if rows == 0:
            return np.array_equal(got[:BAND], want_of(slice(0, BAND + MARGIN))[:BAND])
        return np.array_equal(got[H - BAND:], want_of(slice(H - BAND - MARGIN, H))[MARGIN:])

    torch.cuda.synchronize()
    for f in forms:  # correctness of the first and the last output of every library form, and warm-up
        out16.zero_()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            res = call(f)
        torch.cuda.synchronize()
        if f.startswith("mg_w"):
            T, support, content, shifted = parse(f)
            for b in (0, n - 1):
                lo, hi = max(0, b - T), min(n - 1, b + T)
                got = bits(out16[b])
                for rows in (0, 1):
                    want_of = lambda sl: R.merge(np.stack([src[content](i)[sl] for i in range(lo, hi + 1)]), lut, shift, T, T, b - lo, 1,
                                                 support, 256, pos[lo:hi + 1] if shifted else None)[0]
                    assert band_ok(got, want_of, rows), (f, b, rows)
        elif f == "mg_burst":
            for k in (0, nb - 1):
                got = bits(out16[k])
                want_of = lambda sl: R.merge(np.stack([noi[i % DISTINCT][sl] for i in range(16 * k, 16 * k + 16)]), lut, shift, 0, 15, 0, 1)[0]
                assert band_ok(got, want_of, 0) and band_ok(got, want_of, 1), (f, k)
        elif f == "shade_out":
            assert np.array_equal(bits(out16[n - 1]), S.shade_ref(nat[(n - 1) % DISTINCT], gm, BLACK, 65535)), f
        elif f == "torch_ops":
            want_of = lambda sl: R.merge(np.stack([noi[i % DISTINCT][sl] for i in range(5)]), lut, shift, 2, 2, 2, 1)[0]
            assert band_ok(bits(res[0]), want_of, 0) and band_ok(bits(res[0]), want_of, 1), f
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
    frame = W * H * 2
    rows = []
    for f in forms:
        med = float(np.median(ms[f]))
        nin, nout = (16 * nb, nb) if f == "mg_burst" else (n, n)
        total = (nin + nout) * frame  # every input frame read once, every output written once
        row = {"form": f, "frames": n, "outputs": nout, "width": W, "height": H, "reps": reps, "batch_ms": round(med, 4),
               "batch_ms_min": round(min(ms[f]), 4), "batch_ms_max": round(max(ms[f]), 4), "alg_GB": round(total / 1e9, 3),
               "frac_peak_batch": round(total / (med * 1e-3) / PEAK, 3)}
        if f == "torch_ops":
            row["measured_outputs"] = tf
        if f in fetched:
            row["fetched_over_alg_input"] = round(fetched[f] / (nin * frame), 3)
        rows.append(row)
    by = {r["form"]: r["batch_ms"] for r in rows}
    ratios = {"form": "ratios"}
    for f in forms:
        if f.startswith("mg_w"):
            T = parse(f)[0]
            ratios[f + "_over_shade"] = round(by[f] / by["shade_out"], 3)
            ratios[f + "_over_shade_x_window"] = round(by[f] / (by["shade_out"] * (2 * T + 1)), 3)
            ratios[f + "_over_dn_r1"] = round(by[f] / by["dn_r1"], 3)
        if f in alt_of:
            ratios[f + "_over_default"] = round(by[f] / by[alt_of[f][0]], 3)
    ratios["torch_over_w5_s1_noise"] = round(by["torch_ops"] / by["mg_w5_s1_noise"], 1)
    rows.append(ratios)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--torch-frames", type=int, default=2)
    ap.add_argument("--alt-lib", action="append", default=[])
    ap.add_argument("--fetched-bytes", action="append", default=[])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_merge.py needs a GPU")
    if args.frames < 16:
        sys.exit("bench_merge.py: at least 16 frames (one burst)")
    fetched = {k: float(v) for k, v in (kv.split("=") for kv in args.fetched_bytes)}
    ctx = M.Context(0)
    alts = [AltLib(p) for p in args.alt_lib]
    with open(args.out, "a") as fh:
        for r in run(ctx, alts, args.frames, max(3, args.reps), args.torch_frames, fetched):
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
