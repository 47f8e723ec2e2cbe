#!/usr/bin/env python3
"""The position field on HBM-resident mosaics (mcraw_align_cells_batch, mcraw_merge_cells_batch) beside the global estimate
(mcraw_align_batch), kshade out of place and the merge with one position per frame, all measured in the same run: ms per batch
(events around the call on a torch stream), the algorithmic bytes and the fraction of the 8 TB/s peak.  240 UHD 12-bit frames, a
chain, cell (64, 256), levels 3, radius 2 about align()'s result; all forms take turns rep by rep in ONE process; medians, and
the merges' min - max.  The first and the last pair's field and sad are checked against the numpy statement before anything is
timed.  Appends to profiles/align_cells_bench.jsonl.  Needs a GPU.

    python tools/bench_align_cells.py [--reps 15] [--frames 240]

Forms:
  cells_natural, cells_noise     the field on a natural image that rolls by half a degree per frame, forth over 3.5 degrees and back
                                 again, so every pair of the chain is half a degree apart (about align()'s positions), and on
                                 static noise (about none)
  align_natural                  the global estimate on the rolling frames (levels 4, radius 4)
  shade_out                      kshade out of place on the rolling frames (17 x 13 map): the yardstick of one pass
  mg_w5_s1_pos, mg_w5_s1_field   merge, window 5, support 1, on the rolling frames with align()'s positions and with the field
  mg_w5_s1_constfield            the same merge through the field's entry point with align()'s positions repeated in every cell: the
                                 shifts of mg_w5_s1_pos, read per tile, which splits the field's cost into the reads and the shifts
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch

import _align_cells_ref as CR
import _libs as L
import motioncam_decoder_amd as M
from altlib import bench_mosaics

PEAK = 8e12
W, H = 3840, 2160
PROFILE = dict(S=2e-4, O=2e-6, black=64, white=4095)
BLACK = (64,) * 4
CELL, LEVELS, RADIUS = (64, 256), 3, 2
GLEVELS, GRADIUS = 4, 4
DISTINCT = 8
LEVEL = 800.0
ROLL = 0.5  # degrees per frame: DISTINCT angles, walked forth and back


def rolled(scene, deg):
    """The mosaic rotated by `deg` about its centre, a quad at a time (nearest quad, clamped): a sample keeps its CFA position."""
    h, w = scene.shape[0] // 2, scene.shape[1] // 2
    a = np.deg2rad(deg)
    y, x = np.arange(h)[:, None] - (h - 1) / 2, np.arange(w)[None, :] - (w - 1) / 2
    sy = np.clip(np.rint(np.cos(a) * y - np.sin(a) * x + (h - 1) / 2), 0, h - 1).astype(np.int64)
    sx = np.clip(np.rint(np.sin(a) * y + np.cos(a) * x + (w - 1) / 2), 0, w - 1).astype(np.int64)
    out = np.empty_like(scene)
    for r in (0, 1):
        for c in (0, 1):
            out[r::2, c::2] = scene[2 * sy + r, 2 * sx + c]
    return out


def alg_bytes(n):
    """(mosaic bytes read, pyramid bytes written, pyramid bytes read by the pairs of a chain: base and member once per level)."""
    planes = sum((H >> (l + 1)) * (W >> (l + 1)) * 2 for l in range(LEVELS))
    return n * W * H * 2, n * planes, 2 * (n - 1) * planes


def run(ctx, n, reps):
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(7)
    Rg = PROFILE["white"] - PROFILE["black"]
    sigma = np.sqrt(PROFILE["S"] * Rg * (LEVEL - PROFILE["black"]) + PROFILE["O"] * Rg * Rg)
    noi = [np.clip(np.rint(LEVEL + sigma * rng.standard_normal((H, W))), 0, 4095).astype(np.uint16) for _ in range(DISTINCT)]
    scene = L.natural_image_np(W, H, 12, 12.0, 100)
    nat = [rolled(scene, ROLL * k) for k in range(DISTINCT)]
    nat = nat + nat[-2:0:-1]  # 0, 0.5 .. 3.5, 3.0 .. 0.5 degrees and round again: no pair is further apart than ROLL
    imgs = {"natural": nat, "noise": noi}
    mos = {k: bench_mosaics(dev, v, n) for k, v in imgs.items()}
    out16 = torch.empty((n, H, W), dtype=torch.uint16, device=dev)
    lut, shift = M.noise_lut(**PROFILE)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int16)).to(dev).view(torch.uint16)
    dlut = up(lut)
    y, x = np.linspace(-1, 1, 13)[:, None], np.linspace(-1, 1, 17)[None, :]
    dmap = up(M.gain_map(np.stack([1.0 + (s - 1.0) * (x * x + y * y) / 2 for s in (3.6, 2.9, 2.95, 3.9)])))
    stream = torch.cuda.Stream()
    kw = dict(black=BLACK, cell=CELL, levels=LEVELS, radius=RADIUS)

    # the first and the last pair against the numpy statement, before anything is timed
    with torch.cuda.stream(stream):
        gpos = ctx.align(mos["natural"], black=BLACK, levels=GLEVELS, radius=GRADIUS)
    torch.cuda.synchronize()
    centres = {"natural": gpos, "noise": None}
    fields = {}
    for content in ("natural", "noise"):
        with torch.cuda.stream(stream):
            pos, sad = ctx.align_cells(mos[content], pos=centres[content], sad=True, **kw)
        torch.cuda.synchronize()
        fields[content] = pos
        p, s = pos.cpu().numpy().astype(np.int64), sad.cpu().numpy()
        g = None if centres[content] is None else centres[content].cpu().numpy()
        for t in (1, n - 1):
            pair = np.stack([imgs[content][(t - 1) % len(imgs[content])], imgs[content][t % len(imgs[content])]])
            want_pos, want_sad = CR.align_cells(pair, BLACK, CELL, LEVELS, RADIUS, -1, None if g is None else g[t - 1:t + 1])
            assert np.array_equal(p[t] - p[t - 1], want_pos[1]) and np.array_equal(s[t], want_sad[1].astype(np.int64)), (content, t)
        print("checked cells_%s" % content, flush=True)
    step = (fields["natural"][1].cpu().numpy().astype(np.int64) - fields["natural"][0].cpu().numpy())  # (Cy, Cx, 2): frame 1 against frame 0
    spread = [int(step[..., k].max() - step[..., k].min()) for k in (0, 1)]

    steps = np.diff(fields["natural"].cpu().numpy().astype(np.int64), axis=0)  # every pair of the chain against its centre (reported)
    resid = steps - np.diff(gpos.cpu().numpy().astype(np.int64), axis=0)[:, None, None, :]
    cy, cx = M.cell_grid(H, W, CELL)
    constfield = gpos[:, None, None, :].expand(n, cy, cx, 2).contiguous()
    forms = ["cells_natural", "cells_noise", "align_natural", "shade_out", "mg_w5_s1_pos", "mg_w5_s1_field", "mg_w5_s1_constfield"]

    def call(f):
        if f.startswith("cells_"):
            return ctx.align_cells(mos[f[6:]], pos=centres[f[6:]], **kw)
        if f == "align_natural":
            return ctx.align(mos["natural"], black=BLACK, levels=GLEVELS, radius=GRADIUS)
        if f == "shade_out":
            return ctx.shade(mos["natural"], dmap, black=BLACK, top=65535, out=out16)
        if f == "mg_w5_s1_pos":
            return ctx.merge(mos["natural"], dlut, shift, before=2, after=2, support=1, pos=gpos, out=out16)
        if f == "mg_w5_s1_field":
            return ctx.merge(mos["natural"], dlut, shift, before=2, after=2, support=1, pos=fields["natural"], cell=CELL, out=out16)
        if f == "mg_w5_s1_constfield":
            return ctx.merge(mos["natural"], dlut, shift, before=2, after=2, support=1, pos=constfield, cell=CELL, out=out16)
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
            ms[f].append(a.elapsed_time(b))
    ctx.synchronize()
    assert ctx.errors() == 0
    frame = W * H * 2
    rd, wr, prd = alg_bytes(n)
    rows = []
    for f in forms:
        med = float(np.median(ms[f]))
        if f.startswith("cells_"):
            total = rd + wr + prd
        elif f == "align_natural":
            planes = sum(((H // 2) >> l) * ((W // 2) >> l) * 2 for l in range(GLEVELS))
            total = rd + n * planes + 2 * (n - 1) * planes
        else:
            total = 2 * n * frame  # every input frame read once, every output written once
        rows.append({"form": f, "frames": n, "width": W, "height": H, "cell": list(CELL), "levels": LEVELS, "radius": RADIUS, "reps": reps,
                     "batch_ms": round(med, 4), "batch_ms_min": round(min(ms[f]), 4), "batch_ms_max": round(max(ms[f]), 4),
                     "alg_GB": round(total / 1e9, 3), "frac_peak_batch": round(total / (med * 1e-3) / PEAK, 3)})
    by = {r["form"]: r for r in rows}
    ratios = {"form": "ratios", "alg_mosaic_GB": round(rd / 1e9, 3), "alg_pyramid_written_GB": round(wr / 1e9, 3),
              "alg_pyramid_read_GB": round(prd / 1e9, 3), "field_spread_frame1_yx": spread}
    for f in ("cells_natural", "cells_noise"):
        ratios[f + "_over_align"] = round(by[f]["batch_ms"] / by["align_natural"]["batch_ms"], 3)
        ratios[f + "_over_shade"] = round(by[f]["batch_ms"] / by["shade_out"]["batch_ms"], 3)
    ratios["merge_field_over_merge_pos"] = round(by["mg_w5_s1_field"]["batch_ms"] / by["mg_w5_s1_pos"]["batch_ms"], 3)
    ratios["merge_constfield_over_merge_pos"] = round(by["mg_w5_s1_constfield"]["batch_ms"] / by["mg_w5_s1_pos"]["batch_ms"], 3)
    ratios["field_step_residual_max"], ratios["search_reach"] = int(np.abs(resid).max()), 2 * ((RADIUS + 1) * 2 ** (LEVELS - 1) - 1)
    for f in ("mg_w5_s1_pos", "mg_w5_s1_field", "mg_w5_s1_constfield"):
        ratios[f + "_min_max_ms"] = [by[f]["batch_ms_min"], by[f]["batch_ms_max"]]
    rows.append(ratios)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_cells_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_align_cells.py needs a GPU")
    if args.frames < 3:
        sys.exit("bench_align_cells.py: at least 3 frames")
    ctx = M.Context(0)
    with open(args.out, "a") as fh:
        for r in run(ctx, args.frames, max(3, args.reps)):
            line = json.dumps(r)
            print(line, flush=True)
            fh.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
