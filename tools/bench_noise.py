#!/usr/bin/env python3
"""The noise measurement of HBM-resident mosaics (mcraw_noise_batch) beside kstats B = 256 (which reads the same bytes), beside
kshade out of place (the neighbouring streaming kernel, which moves twice the bytes) and beside the same records built from torch
ops (per CFA position the planes as int64, second differences, squares, block sums, the bin formulas, a bincount): ms per batch
(events around the call on a torch stream), bytes read and the fraction of the 8 TB/s peak.  240 UHD 12-bit frames of natural
(natural images under synthetic Poisson-Gaussian noise of variance 0.5 (x - black) + 4 DN^2), noise (uniform samples) and flat (one
value) content; all forms take turns rep by rep in ONE process.  The first and the last frame of every form are checked against
the numpy reference (tests/_noise_ref.py) first.  The `natural` rows also carry the profile that noise_fit recovers from the
batch's records.  Appends to profiles/noise_bench.jsonl.  Needs a GPU.

    python tools/bench_noise.py [--reps 15] [--torch-reps 3] [--frames 240] [--content natural,noise,flat] [--out FILE]

The torch form takes 0.2 s to seconds per batch (its bincount serialises on a flat frame), so it joins the first --torch-reps
turns only.

MCRAW_LIB_PATH names another build of the library for the whole run (its rows say so under "lib").
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
import _noise_ref as NR
import motioncam_decoder_amd as M

PEAK = 8e12
W, H = 3840, 2160
BLACK, SAT, SHIFT = 64, 4095, 7
PROFILE = (0.5, 4.0)
DISTINCT = 4
FORMS = ["noise", "stats_b256", "kshade_out", "torch_ops"]
CHUNK = 40  # frames per pass of the torch form (its int64 temporaries are four times the planes)


def frames(content, rng):
    if content == "natural":
        return [NR.noisy(L.natural_image_np(W, H, 12, 0.0, 100 + s).astype(np.float64), PROFILE[0], PROFILE[1], BLACK, rng, SAT)
                for s in range(DISTINCT)]
    if content == "noise":
        return [rng.integers(0, 4096, size=(H, W), dtype=np.uint16) for _ in range(DISTINCT)]
    if content == "flat":
        return [np.full((H, W), 1000 + s, np.uint16) for s in range(DISTINCT)]
    raise KeyError(content)


def torch_noise(mos, shift, sat, lo):
    """What a user writes without the kernel: (hist (N, 4, 32, 128), nblk (N, 4), nrej (N, 4)) as int64 tensors."""
    n, h, w = mos.shape
    by, bx = h // 16, w // 16
    hist = torch.zeros((n, 4, 32, 128), dtype=torch.int64, device=mos.device)
    nblk = torch.zeros((n, 4), dtype=torch.int64, device=mos.device)
    nrej = torch.zeros((n, 4), dtype=torch.int64, device=mos.device)
    for f0 in range(0, n, CHUNK):
        f1 = min(n, f0 + CHUNK)
        for p in range(4):
            b = mos[f0:f1, p >> 1:16 * by:2, p & 1:16 * bx:2].to(torch.int64).view(f1 - f0, by, 8, bx, 8)
            dh = b[..., :-2] - 2 * b[..., 1:-1] + b[..., 2:]
            dv = b[:, :, :-2] - 2 * b[:, :, 1:-1] + b[:, :, 2:]
            T = (dh * dh).sum(dim=(2, 4)) + (dv * dv).sum(dim=(2, 4))
            s = b.sum(dim=(2, 4))
            ok = (b.amax(dim=(2, 4)) < sat) & (b.amin(dim=(2, 4)) >= lo)
            e = torch.frexp(T.clamp(min=16).to(torch.float64))[1].to(torch.int64) - 1  # floor(log2 T): exact below 2^53
            vb = torch.where(T < 16, 0, (4 * (e - 4) + ((T.clamp(min=16) >> (e - 2)) & 3) + 1).clamp(max=127))
            lv = ((s >> 6) >> shift).clamp(max=31)
            fr = torch.arange(f1 - f0, device=mos.device)[:, None, None]
            idx = ((fr * 32 + lv) * 128 + vb).flatten()
            hist[f0:f1, p] = torch.bincount(idx, weights=ok.flatten().to(torch.float64), minlength=(f1 - f0) * 4096).to(torch.int64).view(-1, 32, 128)
            nblk[f0:f1, p] = ok.sum(dim=(1, 2))
            nrej[f0:f1, p] = (~ok).sum(dim=(1, 2))
    return hist, nblk, nrej


def run(ctx, content, n, reps, torch_reps):
    dev = torch.device("cuda:0")
    imgs = frames(content, np.random.default_rng(7))
    mos = torch.empty((n, H, W), dtype=torch.uint16, device=dev)
    for i in range(n):
        mos.view(torch.int16)[i].copy_(torch.from_numpy(imgs[i % DISTINCT].view(np.int16)))
    out16 = torch.empty((n, H, W), dtype=torch.uint16, device=dev)
    unit = torch.from_numpy(np.full((4, 13, 17), 4096, np.uint16).view(np.int16)).to(dev).view(torch.uint16)
    rec_noise = torch.empty((n, M.NOISE_RECORD_BYTES), dtype=torch.uint8, device=dev)
    rec_stats = torch.empty((n, 16 * 256 + 96), dtype=torch.uint8, device=dev)
    stream = torch.cuda.Stream()

    def call(f):
        if f == "noise":
            return ctx.noise_stats(mos, shift=SHIFT, sat=SAT, lo=1, out=rec_noise)
        if f == "stats_b256":
            return ctx.stats(mos, bins=256, shift=4, sat=SAT, out=rec_stats)
        if f == "kshade_out":
            return ctx.shade(mos, unit, black=(BLACK,) * 4, top=65535, out=out16)
        if f == "torch_ops":
            return torch_noise(mos, SHIFT, SAT, 1)
        raise KeyError(f)

    last = (n - 1) % DISTINCT
    pair = np.stack([imgs[0], imgs[last]])
    want = NR.noise_stats(pair, SHIFT, SAT, 1)
    fit = None
    torch.cuda.synchronize()
    for f in FORMS:  # correctness of the first and the last frame of every form, and warm-up
        with torch.cuda.stream(stream):
            res = call(f)
        torch.cuda.synchronize()
        if f == "noise":
            got, exp = res.raw.cpu().numpy(), NR.record(want)
            assert np.array_equal(got[0], exp[0]) and np.array_equal(got[n - 1], exp[1]), f
            if content == "natural":
                S, O = M.noise_fit(res, BLACK, SAT)
                R = SAT - BLACK
                fit = {"a_true": PROFILE[0], "b_true": PROFILE[1], "a_fit": [round(float(v) * R, 4) for v in S],
                       "b_fit": [round(float(v) * R * R, 3) for v in O]}
        elif f == "torch_ops":
            for k, fr in ((0, 0), (1, n - 1)):
                for name, t in zip(("hist", "nblk", "nrej"), res):
                    assert np.array_equal(t[fr].cpu().numpy(), want[name][k].astype(np.int64)), (f, name)
        del res
    ms = {f: [] for f in FORMS}
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rep in range(reps):
        for f in FORMS:  # the forms take turns
            if f == "torch_ops" and rep >= torch_reps:
                continue
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
    rows = []
    for f in FORMS:
        med = float(np.median(ms[f]))
        moved = 2 * mosaic_bytes if f == "kshade_out" else mosaic_bytes
        rows.append({"content": content, "form": f, "frames": n, "width": W, "height": H, "reps": len(ms[f]), "batch_ms": round(med, 4),
                     "batch_ms_min": round(min(ms[f]), 4), "batch_ms_max": round(max(ms[f]), 4), "read_GB": round(mosaic_bytes / 1e9, 3),
                     "moved_GB": round(moved / 1e9, 3), "frac_peak_batch": round(moved / (med * 1e-3) / PEAK, 3)})
    by = {r["form"]: r["batch_ms"] for r in rows}
    rows.append({"content": content, "form": "ratios", "noise_over_stats_b256": round(by["noise"] / by["stats_b256"], 3),
                 "noise_over_kshade": round(by["noise"] / by["kshade_out"], 3), "torch_over_noise": round(by["torch_ops"] / by["noise"], 1)})
    if fit:
        rows.append(dict({"content": content, "form": "fit"}, **fit))
    del mos, out16, rec_noise, rec_stats
    torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--torch-reps", type=int, default=3)
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--content", default="natural,noise,flat")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "noise_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_noise.py needs a GPU")
    ctx = M.Context(0)
    with open(args.out, "a") as fh:
        for content in [c for c in args.content.split(",") if c]:
            for r in run(ctx, content, args.frames, max(3, args.reps), max(1, args.torch_reps)):
                if os.environ.get("MCRAW_LIB_PATH"):
                    r["lib"] = os.path.basename(os.environ["MCRAW_LIB_PATH"])
                line = json.dumps(r)
                print(line, flush=True)
                fh.write(line + "\n")
                fh.flush()
    ctx.close()


if __name__ == "__main__":
    main()
