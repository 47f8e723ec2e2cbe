#!/usr/bin/env python3
"""Per-frame statistics of HBM-resident mosaics (mcraw_stats_batch) beside kshade out of place (the neighbouring streaming
kernel, which moves twice the bytes; measured in the same run) and beside the same statistics built from torch ops (a cast
pass, a bincount of the shifted planes, masked sums and min / max per CFA position): ms per batch (events around the call on a
torch stream), bytes read and the fraction of the 8 TB/s peak.  240 UHD 12-bit frames of noise, smooth (natural images), flat
(one value) and half-clipped (the lower half at the white level) content; B = 256 and B = 4096 over the whole frame and
B = 256 over a centre window of a quarter of the frame; all forms take turns rep by rep in ONE process.  The first and the last
frame of every form are checked against the numpy reference.  Appends to profiles/stats_bench.jsonl.  Needs a GPU.

    python tools/bench_stats.py [--reps 15] [--frames 240] [--content noise,smooth,flat,halfclip] [--alt-lib PATH] [--out FILE]

--alt-lib: another build of the library (tools/altlib.py); its three stats forms (*_alt) join the turns.
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
import _stats_ref as S
import motioncam_decoder_amd as M
from altlib import AltLib

PEAK = 8e12
W, H = 3840, 2160
SAT = 4095
ROI = (H // 4, W // 4, H // 2, W // 2)
DISTINCT = 4
FORMS = ["stats_b256", "stats_b4096", "stats_b256_window", "kshade_out", "torch_ops_b256"]
ALT_FORMS = ["stats_b256_alt", "stats_b4096_alt", "stats_b256_window_alt"]


def frames(content, rng):
    if content == "noise":
        return [rng.integers(0, 4096, size=(H, W), dtype=np.uint16) for _ in range(DISTINCT)]
    if content == "smooth":
        return [L.natural_image_np(W, H, 12, 12.0, 100 + s) for s in range(DISTINCT)]
    if content == "flat":
        return [np.full((H, W), 1000 + s, np.uint16) for s in range(DISTINCT)]
    if content == "halfclip":
        out = []
        for s in range(DISTINCT):
            img = L.natural_image_np(W, H, 12, 12.0, 200 + s)
            img[H // 2:] = SAT
            out.append(img)
        return out
    raise KeyError(content)


def torch_stats(mos, bins, shift, sat):
    """What a user writes without the kernel, per CFA position: a cast pass, a bincount of the shifted plane (frames kept
    apart by an offset), masked sums, min / max."""
    n = mos.shape[0]
    res = []
    off = (torch.arange(n, device=mos.device, dtype=torch.int32) * bins)[:, None, None]
    for p in range(4):
        x = mos[:, p >> 1::2, p & 1::2].to(torch.int32)
        b = (x >> shift).clamp_(max=bins - 1) + off
        hist = torch.bincount(b.flatten(), minlength=n * bins).view(n, bins)
        m = x >= sat
        res.append((hist, m.sum(dim=(1, 2)), torch.where(m, 0, x).sum(dim=(1, 2), dtype=torch.int64), x.amin(dim=(1, 2)),
                    x.amax(dim=(1, 2))))
    return res


def run(ctx, alt, content, n, reps):
    dev = torch.device("cuda:0")
    imgs = frames(content, np.random.default_rng(7))
    mos = torch.empty((n, H, W), dtype=torch.uint16, device=dev)
    for i in range(n):
        mos.view(torch.int16)[i].copy_(torch.from_numpy(imgs[i % DISTINCT].view(np.int16)))
    out16 = torch.empty((n, H, W), dtype=torch.uint16, device=dev)
    unit = torch.from_numpy(np.full((4, 13, 17), 4096, np.uint16).view(np.int16)).to(dev).view(torch.uint16)
    recs = {256: torch.empty((n, 16 * 256 + 96), dtype=torch.uint8, device=dev),
            4096: torch.empty((n, 16 * 4096 + 96), dtype=torch.uint8, device=dev)}
    stream = torch.cuda.Stream()

    def call(f):
        if f == "stats_b256":
            return ctx.stats(mos, bins=256, shift=4, sat=SAT, out=recs[256])
        if f == "stats_b4096":
            return ctx.stats(mos, bins=4096, shift=0, sat=SAT, out=recs[4096])
        if f == "stats_b256_window":
            return ctx.stats(mos, bins=256, shift=4, sat=SAT, roi=ROI, out=recs[256])
        if f == "kshade_out":
            return ctx.shade(mos, unit, black=(64,) * 4, top=65535, out=out16)
        if f == "torch_ops_b256":
            return torch_stats(mos, 256, 4, SAT)
        if f == "stats_b256_alt":
            return alt.stats(mos, recs[256], stream, 256, 4, SAT)
        if f == "stats_b4096_alt":
            return alt.stats(mos, recs[4096], stream, 4096, 0, SAT)
        if f == "stats_b256_window_alt":
            return alt.stats(mos, recs[256], stream, 256, 4, SAT, ROI)
        raise KeyError(f)

    forms = FORMS + (ALT_FORMS if alt else [])

    last = (n - 1) % DISTINCT
    pair = np.stack([imgs[0], imgs[last]])
    torch.cuda.synchronize()
    for f in forms:  # correctness of the first and the last frame of every form, and warm-up
        with torch.cuda.stream(stream):
            res = call(f)
        torch.cuda.synchronize()
        if f.startswith("stats_"):
            bins, shift = (4096, 0) if f.startswith("stats_b4096") else (256, 4)
            want = S.record(S.stats(pair, bins, shift, (SAT,) * 4, ROI if "window" in f else None))
            got = res.raw.cpu().numpy()
            assert np.array_equal(got[0], want[0]) and np.array_equal(got[n - 1], want[1]), f
        elif f == "torch_ops_b256":
            want = S.stats(pair, 256, 4, (SAT,) * 4)
            for p, (hist, nsat, sm, mn, mx) in enumerate(res):
                for k, fr in ((0, 0), (1, n - 1)):
                    assert np.array_equal(hist[fr].cpu().numpy(), want["hist"][k, p]) and int(nsat[fr]) == want["nsat"][k, p]
                    assert int(sm[fr]) == want["sum"][k, p] and int(mn[fr]) == want["min"][k, p] and int(mx[fr]) == want["max"][k, p]
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
    read = {"stats_b256_window": mosaic_bytes // 4, "stats_b256_window_alt": mosaic_bytes // 4,
            "kshade_out": mosaic_bytes}  # (kshade writes as many again)
    rows = []
    for f in forms:
        med = float(np.median(ms[f]))
        rb = read.get(f, mosaic_bytes)
        moved = 2 * rb if f == "kshade_out" else rb
        rows.append({"content": content, "form": f, "frames": n, "width": W, "height": H, "reps": reps, "batch_ms": round(med, 4),
                     "batch_ms_min": round(min(ms[f]), 4), "batch_ms_max": round(max(ms[f]), 4), "read_GB": round(rb / 1e9, 3),
                     "moved_GB": round(moved / 1e9, 3), "frac_peak_batch": round(moved / (med * 1e-3) / PEAK, 3)})
    by = {r["form"]: r["batch_ms"] for r in rows}
    rows.append({"content": content, "form": "ratios", "b256_over_kshade": round(by["stats_b256"] / by["kshade_out"], 3),
                 "b4096_over_kshade": round(by["stats_b4096"] / by["kshade_out"], 3),
                 "torch_over_b256": round(by["torch_ops_b256"] / by["stats_b256"], 1)})
    del mos, out16, recs
    torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--content", default="noise,smooth,flat,halfclip")
    ap.add_argument("--alt-lib", default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stats_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_stats.py needs a GPU")
    ctx = M.Context(0)
    alt = AltLib(args.alt_lib) if args.alt_lib else None
    noise = {}
    with open(args.out, "a") as fh:
        for content in [c for c in args.content.split(",") if c]:
            rows = run(ctx, alt, content, args.frames, max(3, args.reps))
            by = {r["form"]: r.get("batch_ms") for r in rows}
            if content == "noise":
                noise = by
            elif noise:  # this content's cost as a ratio to noise, for each B
                rows.append({"content": content, "form": "over_noise", "b256": round(by["stats_b256"] / noise["stats_b256"], 3),
                             "b4096": round(by["stats_b4096"] / noise["stats_b4096"], 3)})
            for r in rows:
                if alt:
                    r["alt_lib"] = alt.name
                line = json.dumps(r)
                print(line, flush=True)
                fh.write(line + "\n")
    if alt:
        alt.close()
    ctx.close()


if __name__ == "__main__":
    main()
