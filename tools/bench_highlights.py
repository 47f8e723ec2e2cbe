#!/usr/bin/env python3
"""Highlight reconstruction on HBM-resident mosaics (mcraw_highlights_batch, mcraw_highlights_measure_batch) beside kshade out of
place and kfixpix (the yardsticks: the same algorithmic bytes, mosaic in + mosaic out, measured in the same run) and beside the
same arithmetic built from torch ops: ms per batch (events around the call on a torch stream), algorithmic bytes and the
fraction of the 8 TB/s peak.  240 UHD 12-bit natural frames; how much of them is clipped is set by `sat` (above every sample,
at the 95th percentile, at the median); all forms take turns rep by rep in ONE process; medians.  The first and the last frame
of every library form are checked against the numpy statement first.  Appends to profiles/highlights_bench.jsonl.  Needs a GPU.

    python tools/bench_highlights.py [--reps 15] [--frames 240]

Forms:
  rebuild_0        apply, REBUILD with the records of a measure call, nothing clipped: the copy-only path
  rebuild_5        the same with about 5 % of the samples clipped
  rebuild_50       the same with about 50 % clipped
  clip             apply, CLIP (sat at the 95th percentile)
  measure          the measure call alone, one record per frame (sat at the 95th percentile)
  chained          measure and apply back to back (highlights(chroma="frame"), about 5 % clipped)
  shade_out        kshade out of place (17 x 13 map)
  fixpix           kfixpix with the thresholds of its detection test (nothing flagged)
  torch_ops        REBUILD with chroma 0 from torch ops on --torch-frames frames, scaled to the batch
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
import _highlights_ref as HL
import _libs as L
import _shade_ref as S
import motioncam_decoder_amd as M

PEAK = 8e12
W, H = 3840, 2160
BLACK, GAIN, CFA = (64,) * 4, (2.0, 1.0, 1.6), "rggb"
DISTINCT = 4
FORMS = ["rebuild_0", "rebuild_5", "rebuild_50", "clip", "measure", "chained", "shade_out", "fixpix", "torch_ops"]


def torch_rebuild(mos, sat, black, gain, top):
    """What a user writes without the kernel: REBUILD with chroma 0 from shifted copies (torch's reflect padding is the
    contract's reflection), RGGB."""
    n, h, w = mos.shape
    dev = mos.device
    p = (torch.arange(h, device=dev)[:, None] & 1) * 2 + (torch.arange(w, device=dev)[None, :] & 1)
    by = lambda vals: torch.tensor([int(v) for v in vals], device=dev, dtype=torch.int64)[p]
    s = mos.to(torch.int64)
    v = ((s - by(black)).clamp_(min=0) * by(gain) + 2048) >> 12
    pad = torch.nn.functional.pad(v.to(torch.float64)[:, None], (1, 1, 1, 1), mode="reflect")[:, 0].to(torch.int64)
    nb = lambda dy, dx: pad[:, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w]
    Hm, Vm = (nb(0, -1) + nb(0, 1) + 1) >> 1, (nb(-1, 0) + nb(1, 0) + 1) >> 1
    Dm = (nb(-1, -1) + nb(-1, 1) + nb(1, -1) + nb(1, 1) + 2) >> 2
    hv = (Hm + Vm + 1) >> 1
    ref = torch.where((p == 1) | (p == 2), hv, (hv + Dm + 1) >> 1)
    back = by(black) + ((ref * by(HL.inv(gain)) + 2048) >> 12)
    new = torch.maximum(s, back.clamp_(max=top))
    return torch.where((s >= by(sat)) & (ref > v), new, s).to(torch.uint16)


def run(ctx, n, reps, torch_frames):
    dev = torch.device("cuda:0")
    nat = [L.natural_image_np(W, H, 12, 12.0, 100 + s) for s in range(DISTINCT)]
    mos = torch.empty((n, H, W), dtype=torch.uint16, device=dev)
    for i in range(n):
        mos.view(torch.int16)[i].copy_(torch.from_numpy(nat[i % DISTINCT].view(np.int16)))
    out16 = torch.empty((n, H, W), dtype=torch.uint16, device=dev)
    gq = M.highlight_gains(GAIN, CFA)
    sats = {"0": 4095, "5": int(np.percentile(nat[0], 95)), "50": int(np.percentile(nat[0], 50))}
    share = {k: round(float(np.mean([(a >= s).mean() for a in nat])), 4) for k, s in sats.items()}
    y, x = np.linspace(-1, 1, 13)[:, None], np.linspace(-1, 1, 17)[None, :]
    gm = M.gain_map(np.stack([1.0 + (s - 1.0) * (x * x + y * y) / 2 for s in (3.6, 2.9, 2.95, 3.9)]))
    dmap = torch.from_numpy(gm.view(np.int16)).to(dev).view(torch.uint16)
    stream = torch.cuda.Stream()
    kw = lambda k: dict(sat=sats[k], black=BLACK, gain=GAIN, cfa=CFA)
    recs = {k: ctx.highlight_chroma(mos, **kw(k)) for k in sats}
    tf = max(1, min(torch_frames, n))
    torch.cuda.synchronize()

    def call(f):
        if f.startswith("rebuild_"):
            return ctx.highlights(mos, chroma=recs[f[8:]], out=out16, **kw(f[8:]))
        if f == "clip":
            return ctx.highlights(mos, mode="clip", out=out16, **kw("5"))
        if f == "measure":
            return ctx.highlight_chroma(mos, **kw("5"))
        if f == "chained":
            return ctx.highlights(mos, chroma="frame", out=out16, **kw("5"))
        if f == "shade_out":
            return ctx.shade(mos, dmap, black=BLACK, top=65535, out=out16)
        if f == "fixpix":
            return ctx.fix_pixels(mos, black=BLACK, abs_thr=(96,) * 4, rel_thr=26 / 256.0, rank=2, out=out16)
        if f == "torch_ops":
            return torch_rebuild(mos[:tf], (sats["5"],) * 4, BLACK, gq, 65535)
        raise KeyError(f)

    bits = lambda t: t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)
    ends = (0, n - 1)
    four = lambda v: (v,) * 4
    wrec = {(k, i): HL.measure(nat[i % DISTINCT][None], four(sats[k]), BLACK, gq, 0, HL.default_lo(four(sats[k]), BLACK)) for k in sats for i in ends}
    for f in FORMS:  # correctness of the first and the last frame of every form, and warm-up
        out16.zero_()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            res = call(f)
        torch.cuda.synchronize()
        for i in ends:
            img = nat[i % DISTINCT]
            if f.startswith("rebuild_") or f == "chained":
                k = "5" if f == "chained" else f[8:]
                assert np.array_equal(bits(out16[i]), HL.apply(img[None], HL.REBUILD, four(sats[k]), BLACK, gq, 0, wrec[k, i])[0]), (f, i)
            elif f == "clip":
                assert np.array_equal(bits(out16[i]), HL.apply(img[None], HL.CLIP, four(sats["5"]), BLACK, gq, 0)[0]), (f, i)
            elif f == "measure":
                assert np.array_equal(res.raw[i:i + 1].cpu().numpy(), HL.raw(*wrec["5", i])), (f, i)
            elif f == "shade_out":
                assert np.array_equal(bits(out16[i]), S.shade_ref(img, gm, BLACK, 65535)), (f, i)
            elif f == "fixpix":
                assert np.array_equal(bits(out16[i]), F.fixpix(img[None], 3, 2, 26, BLACK, (96,) * 4)[0][0]), (f, i)
        if f == "torch_ops":
            assert np.array_equal(bits(res[0]), HL.apply(nat[0][None], HL.REBUILD, four(sats["5"]), BLACK, gq, 0, None)[0]), f
        del res
    ms = {f: [] for f in FORMS}
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(reps):
        for f in FORMS:  # the forms take turns
            with torch.cuda.stream(stream):
                a.record(stream)
                res = call(f)
                b.record(stream)
            torch.cuda.synchronize()
            del res
            ms[f].append(a.elapsed_time(b) * (n / tf if f == "torch_ops" else 1.0))
    ctx.synchronize()
    assert ctx.errors() == 0
    frame = n * W * H * 2
    rows = []
    for f in FORMS:
        med = float(np.median(ms[f]))
        total = frame if f == "measure" else 3 * frame if f == "chained" else 2 * frame  # mosaic in (+ mosaic out)
        row = {"form": f, "frames": n, "width": W, "height": H, "reps": reps, "batch_ms": round(med, 4),
               "batch_ms_min": round(min(ms[f]), 4), "batch_ms_max": round(max(ms[f]), 4), "alg_GB": round(total / 1e9, 3),
               "frac_peak_batch": round(total / (med * 1e-3) / PEAK, 3)}
        if f == "torch_ops":
            row["measured_frames"] = tf
        rows.append(row)
    by = {r["form"]: r["batch_ms"] for r in rows}
    rows.append({"form": "ratios", "rebuild_0_over_fixpix": round(by["rebuild_0"] / by["fixpix"], 3),
                 "rebuild_0_over_shade": round(by["rebuild_0"] / by["shade_out"], 3),
                 "rebuild_5_over_rebuild_0": round(by["rebuild_5"] / by["rebuild_0"], 3),
                 "rebuild_50_over_rebuild_0": round(by["rebuild_50"] / by["rebuild_0"], 3),
                 "clip_over_shade": round(by["clip"] / by["shade_out"], 3),
                 "measure_over_shade": round(by["measure"] / by["shade_out"], 3),
                 "chained_over_parts": round(by["chained"] / (by["measure"] + by["rebuild_5"]), 3),
                 "torch_over_rebuild_5": round(by["torch_ops"] / by["rebuild_5"], 1),
                 "sat": sats, "clipped_share": share})
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--torch-frames", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "highlights_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_highlights.py needs a GPU")
    ctx = M.Context(0)
    with open(args.out, "a") as fh:
        for r in run(ctx, args.frames, max(3, args.reps), args.torch_frames):
            line = json.dumps(r)
            print(line, flush=True)
            fh.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
