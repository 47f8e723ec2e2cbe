#!/usr/bin/env python3
"""The shift estimate on HBM-resident mosaics (mcraw_align_batch) beside kshade out of place (measured in the same run) and
beside the same estimate built from torch ops: ms per batch (events around the call on a torch stream), the algorithmic bytes
(every mosaic read once, every pyramid level written once and read once per pair it belongs to) and the fraction of the 8 TB/s
peak.  240 UHD 12-bit frames, a chain at levels 4, radius 4; all forms take turns rep by rep in ONE process; medians.  The
first and the last pair's pos and sad are checked against the numpy reference before anything is timed.  Appends to
profiles/align_bench.jsonl.  Needs a GPU.

    python tools/bench_align.py [--reps 15] [--frames 240] [--stop-lib K=PATH ...]

Forms:
  align_natural, align_noise     the chain on a natural image that moves by (2, 6) samples per frame, and on static noise
  align_stopK                    --stop-lib K=PATH: a build that stops after K parts (python -m motioncam_decoder_amd.build variant
                                 PATH -DMCRAW_ALIGN_STOP=K: 1 = the pyramid pass, 1 + j = j levels of the search, coarsest first),
                                 on the natural frames, in a context of its own; the parts' times are the differences
  shade_out                      kshade out of place on the natural frames (17 x 13 map): the yardstick of one pass
  torch_ops                      the same estimate from torch ops on --torch-pairs pairs, scaled to the batch's pairs
  mg_w5_s1_natural, ..._pos      merge, window 5, support 1, on the natural frames without positions and with the stage's
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch

import _align_ref as R
import _libs as L
import motioncam_decoder_amd as M
from altlib import AltLib, bench_mosaics

PEAK = 8e12
W, H = 3840, 2160
PROFILE = dict(S=2e-4, O=2e-6, black=64, white=4095)
BLACK = (64,) * 4
LEVELS, RADIUS = 4, 4
DISTINCT = 8
LEVEL = 800.0
STEP = (2, 6)  # the natural image moves by this much per frame, modulo DISTINCT frames


def torch_align(mos, black, levels, radius):
    """What a user writes without the kernels: grey planes and the pyramid from strided sums, per level and candidate a shifted
    abs().sum(), the winner fetched by the host (a chain; returns the pairs' d as a list)."""
    n, h, w = mos.shape
    bl = torch.tensor(black, device=mos.device, dtype=torch.int64).reshape(1, 2, 1, 2)
    g = (mos[:, :h // 2 * 2, :w // 2 * 2].to(torch.int64).reshape(n, h // 2, 2, w // 2, 2) - bl).clamp_(min=0)
    pyr = [((g.sum(dim=(2, 4)) + 2) >> 2).clamp_(max=65535)]
    for _ in range(levels - 1):
        p = pyr[-1]
        hh, ww = p.shape[1] // 2, p.shape[2] // 2
        pyr.append((p[:, :2 * hh, :2 * ww].reshape(n, hh, 2, ww, 2).sum(dim=(2, 4)) + 2) >> 2)
    B = R.bounds(levels, radius)
    out = []
    for t in range(1, n):
        cy = cx = 0
        for l in range(levels - 1, -1, -1):
            rad = radius if l == levels - 1 else 1
            hh, ww = pyr[l].shape[1:]
            base = pyr[l][t - 1, B[l]:hh - B[l], B[l]:ww - B[l]]
            sads = torch.stack([(pyr[l][t, B[l] + cy + dy:hh - B[l] + cy + dy, B[l] + cx + dx:ww - B[l] + cx + dx] - base).abs().sum()
                                for dy in range(-rad, rad + 1) for dx in range(-rad, rad + 1)]).cpu().tolist()
            key = min((s, dy * dy + dx * dx, dy, dx) for s, (dy, dx) in
                      zip(sads, ((dy, dx) for dy in range(-rad, rad + 1) for dx in range(-rad, rad + 1))))
            cy, cx = cy + key[2], cx + key[3]
            if l:
                cy, cx = 2 * cy, 2 * cx
        out.append((cy, cx))
    return out


def alg_bytes(n, levels):
    """(mosaic bytes read, pyramid bytes written, pyramid bytes read by the pairs of a chain)."""
    planes = sum(((H // 2) >> l) * ((W // 2) >> l) * 2 for l in range(levels))
    return n * W * H * 2, n * planes, 2 * (n - 1) * planes


def run(ctx, stops, n, reps, torch_pairs):
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    Rg = PROFILE["white"] - PROFILE["black"]
    sigma = np.sqrt(PROFILE["S"] * Rg * (LEVEL - PROFILE["black"]) + PROFILE["O"] * Rg * Rg)
    noi = [np.clip(np.rint(LEVEL + sigma * rng.standard_normal((H, W))), 0, 4095).astype(np.uint16) for _ in range(DISTINCT)]
    scene = L.natural_image_np(W, H, 12, 12.0, 100)
    nat = [np.roll(scene, (STEP[0] * k, STEP[1] * k), axis=(0, 1)) for k in range(DISTINCT)]
    imgs = {"natural": nat, "noise": noi}
    mos = {k: bench_mosaics(dev, v, n) for k, v in imgs.items()}
    out16 = torch.empty((n, H, W), dtype=torch.uint16, device=dev)
    lut, shift = M.noise_lut(**PROFILE)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(dev).view(torch.uint16)
    dlut = up(lut)
    y, x = np.linspace(-1, 1, 13)[:, None], np.linspace(-1, 1, 17)[None, :]
    dmap = up(M.gain_map(np.stack([1.0 + (s - 1.0) * (x * x + y * y) / 2 for s in (3.6, 2.9, 2.95, 3.9)])))
    stream = torch.cuda.Stream()
    kw = dict(black=BLACK, levels=LEVELS, radius=RADIUS)
    work = torch.empty((int(M.load().mcraw_align_work_bytes(W, H, n, LEVELS, RADIUS)),), dtype=torch.uint8, device=dev)
    spos = torch.empty((n, 2), dtype=torch.int16, device=dev)
    tp = max(1, min(torch_pairs, n - 1))

    # the first and the last pair against the numpy reference, before anything is timed
    found = {}
    for content in ("natural", "noise"):
        with torch.cuda.stream(stream):
            pos, sad = ctx.align(mos[content], sad=True, **kw)
        torch.cuda.synchronize()
        pos, sad = pos.cpu().numpy().astype(np.int64), sad.cpu().numpy()
        for t in (1, n - 1):
            want_pos, want_sad = R.align(np.stack([imgs[content][(t - 1) % DISTINCT], imgs[content][t % DISTINCT]]), BLACK, LEVELS, RADIUS)
            assert np.array_equal(pos[t] - pos[t - 1], want_pos[1]) and sad[t] == want_sad[1], (content, t, pos[t] - pos[t - 1], want_pos[1])
        found[content] = pos
        print("checked align_%s" % content, flush=True)
    follows = np.array_equal(found["natural"], np.array([[STEP[0] * (i % DISTINCT), STEP[1] * (i % DISTINCT)] for i in range(n)]))
    assert follows, "the natural frames' motion was not recovered"
    got = torch_align(mos["natural"][:tp + 1], BLACK, LEVELS, RADIUS)
    assert [list(2 * np.array(d)) for d in got] == [list(found["natural"][t] - found["natural"][t - 1]) for t in range(1, tp + 1)]
    print("checked torch_ops", flush=True)
    dpos = torch.from_numpy(found["natural"].astype(np.int16)).to(dev)

    forms = ["align_natural", "align_noise"] + ["align_stop%d" % k for k, _ in stops] + ["shade_out", "torch_ops", "mg_w5_s1_natural",
                                                                                       "mg_w5_s1_natural_pos"]
    stop_of = {"align_stop%d" % k: a for k, a in stops}

    def call(f):
        if f in stop_of:
            return stop_of[f].align(mos["natural"], spos, work, stream, LEVELS, RADIUS, BLACK)
        if f.startswith("align_"):
            return ctx.align(mos[f[6:]], **kw)
        if f == "shade_out":
            return ctx.shade(mos["natural"], dmap, black=BLACK, top=65535, out=out16)
        if f == "torch_ops":
            return torch_align(mos["natural"][:tp + 1], BLACK, LEVELS, RADIUS)
        if f.startswith("mg_w5"):
            return ctx.merge(mos["natural"], dlut, shift, before=2, after=2, support=1, pos=dpos if f.endswith("_pos") else None, out=out16)
        raise KeyError(f)

    for f in forms:  # warm-up
        with torch.cuda.stream(stream):
            res = call(f)
        torch.cuda.synchronize()
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
            ms[f].append(a.elapsed_time(b) * ((n - 1) / tp if f == "torch_ops" else 1.0))
    ctx.synchronize()
    assert ctx.errors() == 0
    frame = W * H * 2
    rd, wr, prd = alg_bytes(n, LEVELS)
    rows = []
    for f in forms:
        med = float(np.median(ms[f]))
        if f == "align_stop1":
            total = rd + wr
        elif f.startswith("align_") or f == "torch_ops":
            total = rd + wr + prd
        else:
            total = 2 * n * frame  # every input frame read once, every output written once
        row = {"form": f, "frames": n, "width": W, "height": H, "levels": LEVELS, "radius": RADIUS, "reps": reps, "batch_ms": round(med, 4),
               "batch_ms_min": round(min(ms[f]), 4), "batch_ms_max": round(max(ms[f]), 4), "alg_GB": round(total / 1e9, 3),
               "frac_peak_batch": round(total / (med * 1e-3) / PEAK, 3)}
        if f == "torch_ops":
            row["measured_pairs"] = tp
        rows.append(row)
    by = {r["form"]: r["batch_ms"] for r in rows}
    ratios = {"form": "ratios", "alg_mosaic_GB": round(rd / 1e9, 3), "alg_pyramid_written_GB": round(wr / 1e9, 3),
              "alg_pyramid_read_GB": round(prd / 1e9, 3), "natural_motion_recovered": bool(follows)}
    for f in ("align_natural", "align_noise"):
        ratios[f + "_over_shade"] = round(by[f] / by["shade_out"], 3)
        ratios["torch_over_" + f] = round(by["torch_ops"] / by[f], 1)
    prev = 0.0
    for k, _ in stops:  # the parts' times: the differences of the builds that stop early
        name = "pyramid" if k == 1 else "level_%d" % (LEVELS + 1 - k)
        ratios[name + "_ms"] = round(by["align_stop%d" % k] - prev, 4)
        if k == 1:
            ratios["pyramid_over_shade"] = round(by["align_stop1"] / by["shade_out"], 3)
        prev = by["align_stop%d" % k]
    if stops:
        ratios["rest_ms"] = round(by["align_natural"] - prev, 4)
    ratios["merge_pos_over_merge"] = round(by["mg_w5_s1_natural_pos"] / by["mg_w5_s1_natural"], 3)
    ratios["align_over_merge_pos"] = round(by["align_natural"] / by["mg_w5_s1_natural_pos"], 3)
    rows.append(ratios)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--torch-pairs", type=int, default=2)
    ap.add_argument("--stop-lib", action="append", default=[], help="K=PATH: a build with -DMCRAW_ALIGN_STOP=K")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_align.py needs a GPU")
    if args.frames < 3:
        sys.exit("bench_align.py: at least 3 frames")
    ctx = M.Context(0)
    stops = sorted((int(k), AltLib(p)) for k, p in (kp.split("=", 1) for kp in args.stop_lib))
    with open(args.out, "a") as fh:
        for r in run(ctx, stops, args.frames, max(3, args.reps), args.torch_pairs):
            if stops:
                r["stop_libs"] = [a.name for _, a in stops]
            line = json.dumps(r)
            print(line, flush=True)
            fh.write(line + "\n")
    for _, a in stops:
        a.close()
    ctx.close()


if __name__ == "__main__":
    main()
