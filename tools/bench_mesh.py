#!/usr/bin/env python3
"""The mesh warp of the demosaic (mcraw_demosaic_mesh_batch) on HBM-resident mosaics: 240 UHD frames onto 3456 x 1944, the 90 %
window.  Forms: f16 cubic, u8 HWC and NV12, each under three mesh contents: affine_mesh of the identity (one mesh for the batch),
affine_mesh of tools/bench_warp.py's roll (one mesh per frame), and one barrel distortion_mesh for the batch.  Beside them, from
the same run: krgb_warp under the same identity and roll maps (the yardstick: on the same maps the mesh reads the same samples
and does the same taps, plus four node loads per tile and the per-pixel interpolation), krgb_mhc of the whole frame and kshade out
of place.  ms per batch from events around the call on a torch stream, medians over the reps; all forms take turns rep by rep in
ONE process, in both orders.  Every mesh row carries its ratio to krgb_warp on the same maps and whether that ratio lies inside
krgb_warp's own min .. max spread; nothing is asserted about it.  Two frames of two forms are checked against the numpy statement
(tests/_mesh_ref.py) before anything is timed.  Appends to profiles/mesh_bench.jsonl.  Needs a GPU.

    python tools/bench_mesh.py [--reps 7] [--frames 240] [--out PATH]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]
import numpy as np
import torch

import _mesh_ref as MR
import _yuv_ref as Y
import motioncam_decoder_amd as M
from altlib import bench_images, bench_mosaics
from bench_warp import BLACK, DISTINCT, ES, GAIN, H, KINDS, MAT, PEAK, SIZE, W, WHITE, roll_maps, samples

BARREL = dict(radial=(1.0, -0.12, 0.02, 0.0), tangential=(0.001, -0.001))


def run(ctx, n, reps):
    dev = torch.device("cuda:0")
    ho, wo = SIZE
    imgs = bench_images("noise", W, H, DISTINCT, np.random.default_rng(7))
    mos = bench_mosaics(dev, imgs, n)
    shaded = torch.empty_like(mos)
    dgm = torch.from_numpy(M.gain_map(np.ones((4, 13, 17)) * 1.25).view(np.int16)).to(dev).view(torch.uint16)
    out = torch.empty(n * 3 * W * H * 2, dtype=torch.uint8, device=dev)  # room for the largest form (f16, the whole frame)
    stream = torch.cuda.Stream()
    kw = dict(white=WHITE, black=BLACK, gain=GAIN, matrix=MAT)
    ident, roll, _ = roll_maps(n)
    barrel = M.distortion_mesh(H, W, SIZE, **BARREL)
    host = {"identity": M.affine_mesh(ident, SIZE), "roll": M.affine_mesh(roll, SIZE), "barrel": barrel[None]}
    for name, m in host.items():
        M.mesh_check(m, H, W, SIZE, inside=True)  # in the regime and inside the frame: neither clamp acts
    meshes = {name: torch.from_numpy(m).to(dev) for name, m in host.items()}  # resident: the calls take them in place
    maps = {"identity": ident, "roll": roll}

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

    forms = {}
    for kind in KINDS:
        for name in meshes:
            forms["mesh_%s_%s" % (kind, name)] = lambda kind=kind, name=name: demosaic(kind, "mesh", ho, wo, size=SIZE, mesh=meshes[name], filter="cubic")
        for name in maps:
            forms["warp_%s_%s" % (kind, name)] = lambda kind=kind, name=name: demosaic(kind, "warp", ho, wo, size=SIZE, affine=maps[name], filter="cubic")
    forms["mhc_f16"] = lambda: demosaic("f16", "mhc", H, W)
    forms["kshade"] = lambda: ctx.shade(mos, dgm, black=BLACK, out=shaded)
    win_in = n * ho * wo * 2
    alg = {"kshade": 2 * n * W * H * 2, "mhc_f16": n * W * H * 2 + n * samples("f16", H, W) * 2}
    for f in forms:
        if f not in alg:
            kind = f.split("_")[1]
            alg[f] = win_in + n * samples(kind, ho, wo) * ES[kind]

    torch.cuda.synchronize()
    t1 = 3  # a rolled frame: 1.5 degrees
    o0 = MR.values(MR.mesh_estimates(imgs[0], barrel, SIZE, "cubic", BLACK, "rggb"), WHITE, BLACK, GAIN, MAT)
    o1 = MR.values(MR.mesh_estimates(imgs[t1 % DISTINCT], host["roll"][t1], SIZE, "cubic", BLACK, "rggb"), WHITE, BLACK, GAIN, MAT)
    for f in forms:  # warm-up, and the correctness of two frames of two forms
        with torch.cuda.stream(stream):
            res = forms[f]()
        torch.cuda.synchronize()
        if f == "mesh_f16_barrel":
            assert np.array_equal(res[0].view(torch.int16).cpu().numpy().view(np.uint16), MR.float_bits(o0, "f16")), f
        elif f == "mesh_nv12_roll":
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
    for f in forms:
        med = float(np.median(ms[f]))
        r = {"form": f, "frames": n, "width": W, "height": H, "size": list(SIZE), "reps": reps, "batch_ms": round(med, 4),
             "batch_ms_min": round(min(ms[f]), 4), "batch_ms_max": round(max(ms[f]), 4), "alg_GB": round(alg[f] / 1e9, 3),
             "frac_peak_batch": round(alg[f] / (med * 1e-3) / PEAK, 3)}
        if f.startswith("mesh_"):
            _, kind, name = f.split("_")
            yard = ms["warp_%s_%s" % (kind, "roll" if name == "barrel" else name)]  # (the barrel has no affine twin: against the roll)
            ymed = float(np.median(yard))
            r["yardstick"] = "warp_%s_%s" % (kind, "roll" if name == "barrel" else name)
            r["ratio_to_warp"] = round(med / ymed, 3)
            r["warp_spread"] = [round(min(yard) / ymed, 3), round(max(yard) / ymed, 3)]
            r["inside_warp_spread"] = bool(min(yard) <= med <= max(yard))
        rows.append(r)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_mesh.py needs a GPU")
    ctx = M.Context(0)
    with open(args.out, "a") as fh:
        for r in run(ctx, args.frames, max(3, args.reps)):
            line = json.dumps(r)
            print(line, flush=True)
            fh.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
