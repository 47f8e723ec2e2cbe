#!/usr/bin/env python3
"""The affine warp of the demosaic (mcraw_demosaic_warp_batch) on HBM-resident mosaics: 240 UHD frames onto 3456 x 1944, the
90 % stabilisation window, with the identity map (the window centred) and with a roll of half a degree per frame about the
frame's centre, forth over 3.5 degrees and back, as tools/bench_align_cells.py rolls its scene.  Forms: f16 cubic, f16 linear,
u8 HWC and NV12, each under both sets of maps.  Beside them krgb_resample on the 90 % crop at its own size (what the window cost
before it could move by fractions or roll), krgb_mhc of the whole frame, kshade out of place (the yardstick of one pass), and the
torch route: demosaic(algo="mhc", dtype="f16"), then affine_grid + grid_sample(mode="bicubic") with the same roll.  ms per batch
from events around the call on a torch stream, medians over the reps, algorithmic bytes (the window's samples in + samples out)
and the fraction of the 8 TB/s peak; all forms take turns rep by rep in ONE process, in both orders.  Frame 0 and a rolled frame
of two forms are checked against the numpy statement (tests/_warp_ref.py) before anything is timed.  Appends to
profiles/warp_bench.jsonl.  Needs a GPU.

    python tools/bench_warp.py [--reps 7] [--frames 240] [--out PATH]
"""
import argparse
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch

import _warp_ref as WR
import _yuv_ref as Y
import motioncam_decoder_amd as M
from altlib import bench_images, bench_mosaics

PEAK = 8e12
WHITE, BLACK = 4095.0, (64, 64, 64, 64)
GAIN = (2.0, 1.0, 1.6)
MAT = np.array([[1.7, -0.5, -0.2], [-0.25, 1.4, -0.15], [0.05, -0.45, 1.4]], np.float32)
DISTINCT = 2
W, H, SIZE = 3840, 2160, (1944, 3456)
CROP = (108, 192, 1944, 3456)
ROLL, STEPS = 0.5, 8  # degrees per frame; angles 0 .. 3.5, walked forth and back
KINDS = ("f16", "u8", "nv12")
ES = {"f16": 2, "u8": 1, "nv12": 1}


def samples(kind, ho, wo):
    return ho * wo * 3 // (2 if kind == "nv12" else 1)


def roll_maps(n):
    """(identity maps (1, 6), roll maps (n, 6)): the centred window, and the same window rolled about the frame's centre."""
    oy, ox = (H - SIZE[0]) // 2, (W - SIZE[1]) // 2
    cy, cx = (H - 1) / 2.0, (W - 1) / 2.0
    cyc = list(range(STEPS)) + list(range(STEPS - 2, 0, -1))
    A = np.zeros((n, 2, 3))
    for t in range(n):
        a = math.radians(ROLL * cyc[t % len(cyc)])
        c, s = math.cos(a), math.sin(a)
        A[t] = [[c, -s, cy + c * (oy - cy) - s * (ox - cx)], [s, c, cx + s * (oy - cy) + c * (ox - cx)]]
    return np.array([[65536, 0, 256 * oy, 0, 65536, 256 * ox]], dtype=np.int32), M.quantize_affine(A), A


def run(ctx, n, reps):
    dev = torch.device("cuda:0")
    ho, wo = SIZE
    imgs = bench_images("noise", W, H, DISTINCT, np.random.default_rng(7))
    mos = bench_mosaics(dev, imgs, n)
    shaded = torch.empty_like(mos)
    gm = M.gain_map(np.ones((4, 13, 17)) * 1.25)
    dgm = torch.from_numpy(gm.view(np.int16)).to(dev).view(torch.uint16)
    out = torch.empty(n * 3 * W * H * 2, dtype=torch.uint8, device=dev)  # room for the largest form (f16, the whole frame)
    stream = torch.cuda.Stream()
    kw = dict(white=WHITE, black=BLACK, gain=GAIN, matrix=MAT)
    ident, roll, A = roll_maps(n)
    for m in roll:
        assert WR.map_ok(m, SIZE, H, W)
    # the torch route's grid: normalised coordinates of the rolled window's pixels in the whole frame (align_corners=True: -1 and
    # 1 are the centres of the first and last sample)
    theta = torch.zeros((n, 2, 3), dtype=torch.float32)
    oy, ox = (H - ho) // 2, (W - wo) // 2
    for t in range(n):
        # output pixel (i, k), normalised u = 2 k / (wo - 1) - 1, v = 2 i / (ho - 1) - 1 -> source (x, y), normalised likewise
        ayy, ayx, ty, axy, axx, tx = A[t, 0, 0], A[t, 0, 1], A[t, 0, 2], A[t, 1, 0], A[t, 1, 1], A[t, 1, 2]
        sy, sx = (ho - 1) / 2.0, (wo - 1) / 2.0
        # y = ty + ayy i + ayx k with i = sy (v + 1), k = sx (u + 1); yn = 2 y / (H - 1) - 1
        theta[t, 0] = torch.tensor([2 * axx * sx / (W - 1), 2 * axy * sy / (W - 1), 2 * (tx + axy * sy + axx * sx) / (W - 1) - 1])
        theta[t, 1] = torch.tensor([2 * ayx * sx / (H - 1), 2 * ayy * sy / (H - 1), 2 * (ty + ayy * sy + ayx * sx) / (H - 1) - 1])
    theta = theta.to(dev).to(torch.float16)

    def view(kind, h, w):
        t = out[: n * samples(kind, h, w) * ES[kind]]
        if kind == "f16":
            return t.view(torch.float16).view(n, 3, h, w)
        return t.view(n, h, w, 3) if kind == "u8" else t.view(n, h * 3 // 2, w)

    def demosaic(kind, algo, h, w, **extra):
        o = view(kind, h, w)
        if kind == "f16":
            return ctx.demosaic(mos, algo=algo, dtype="f16", out=o, **extra, **kw)
        if kind == "u8":
            return ctx.demosaic_display(mos, algo=algo, transfer="bt709", dtype=torch.uint8, layout="hwc", out=o, **extra, **kw)
        return ctx.demosaic_yuv(mos, algo=algo, fmt="nv12", transfer="bt709", out=o, **extra, **kw)

    def torch_route():
        full = ctx.demosaic(mos, algo="mhc", dtype="f16", out=view("f16", H, W), **kw)
        grid = torch.nn.functional.affine_grid(theta, (n, 3, ho, wo), align_corners=True)
        return torch.nn.functional.grid_sample(full, grid, mode="bicubic", padding_mode="reflection", align_corners=True)

    forms = {}
    for kind in KINDS:
        forms["warp_%s_identity" % kind] = lambda kind=kind: demosaic(kind, "warp", ho, wo, size=SIZE, affine=ident, filter="cubic")
        forms["warp_%s_roll" % kind] = lambda kind=kind: demosaic(kind, "warp", ho, wo, size=SIZE, affine=roll, filter="cubic")
    forms["warp_f16_linear_identity"] = lambda: demosaic("f16", "warp", ho, wo, size=SIZE, affine=ident, filter="linear")
    forms["warp_f16_linear_roll"] = lambda: demosaic("f16", "warp", ho, wo, size=SIZE, affine=roll, filter="linear")
    forms["resample_f16_crop90"] = lambda: demosaic("f16", "resample", ho, wo, size=SIZE, crop=CROP, filter="cubic")
    forms["mhc_f16"] = lambda: demosaic("f16", "mhc", H, W)
    forms["kshade"] = lambda: ctx.shade(mos, dgm, black=BLACK, out=shaded)
    forms["torch_mhc_f16_grid_sample_bicubic_roll"] = torch_route
    win_in = n * ho * wo * 2
    alg = {"kshade": 2 * n * W * H * 2, "mhc_f16": n * W * H * 2 + n * samples("f16", H, W) * 2}
    for f in forms:
        if f not in alg:
            kind = "u8" if "_u8" in f else "nv12" if "_nv12" in f else "f16"
            alg[f] = win_in + n * samples(kind, ho, wo) * ES[kind]

    torch.cuda.synchronize()
    t1 = 3  # a rolled frame: 1.5 degrees
    o0 = WR.values(WR.warp_estimates(imgs[0], ident[0], SIZE, "cubic", BLACK, "rggb"), WHITE, BLACK, GAIN, MAT)
    o1 = WR.values(WR.warp_estimates(imgs[t1 % DISTINCT], roll[t1], SIZE, "cubic", BLACK, "rggb"), WHITE, BLACK, GAIN, MAT)
    for f in forms:  # warm-up, and the correctness of two frames of two forms
        with torch.cuda.stream(stream):
            res = forms[f]()
        torch.cuda.synchronize()
        if f == "warp_f16_identity":
            assert np.array_equal(res[0].view(torch.int16).cpu().numpy().view(np.uint16), WR.float_bits(o0, "f16")), f
        elif f == "warp_nv12_roll":
            want = Y.yuv_from_o(o1, M.transfer_lut("bt709", 4096, 12), "nv12", M.yuv_matrix("bt709", "limited", 8, 12), 12)
            assert np.array_equal(res[t1].cpu().numpy(), want), f
        del res
    ms = {f: [] for f in forms}
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for rep in range(reps):
        for f in (list(forms) if rep % 2 == 0 else list(forms)[::-1]):  # the forms take turns, in both orders
            with torch.cuda.stream(stream):
                a.record(stream)
                res = forms[f]()
                b.record(stream)
            torch.cuda.synchronize()
            del res
            ms[f].append(a.elapsed_time(b))
    ctx.synchronize()
    assert ctx.errors() == 0
    rows = []
    torch_ms = float(np.median(ms["torch_mhc_f16_grid_sample_bicubic_roll"]))
    res_ms = float(np.median(ms["resample_f16_crop90"]))
    for f in forms:
        med = float(np.median(ms[f]))
        r = {"form": f, "frames": n, "width": W, "height": H, "size": list(SIZE), "reps": reps, "batch_ms": round(med, 4),
             "batch_ms_min": round(min(ms[f]), 4), "batch_ms_max": round(max(ms[f]), 4), "alg_GB": round(alg[f] / 1e9, 3),
             "frac_peak_batch": round(alg[f] / (med * 1e-3) / PEAK, 3)}
        if f.startswith("warp_"):
            r["ratio_to_resample_f16"] = round(med / res_ms, 3)
            r["ratio_to_torch_route"] = round(med / torch_ms, 3)
            if f.endswith("_roll"):
                r["roll_over_identity"] = round(med / float(np.median(ms[f[:-5] + "_identity"])), 3)
        rows.append(r)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "warp_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_warp.py needs a GPU")
    ctx = M.Context(0)
    with open(args.out, "a") as fh:
        for r in run(ctx, args.frames, max(3, args.reps)):
            line = json.dumps(r)
            print(line, flush=True)
            fh.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
