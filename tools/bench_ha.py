#!/usr/bin/env python3
"""The edge-directed demosaic (MCRAW_RGB_HA, algo="ha") on HBM-resident mosaics: 240 UHD frames as f16 CHW, u8 HWC sRGB (L = 4096)
and NV12, on a natural scene ("smooth") and on noise -- the direction choice is data-dependent, so content may matter.  Beside
every form krgb_mhc of the same family on the same input, and once kshade out of place (the yardstick of one pass) and the same
algorithm built from torch ops (int32 tensors, in chunks of 8 frames; f16 CHW on the natural scene).  ms per batch from events
around the call on a torch stream, medians over the reps, algorithmic bytes (samples in + samples out) and the fraction of the
8 TB/s peak; all forms take turns rep by rep in ONE process, in both orders.  Two frames of two forms are checked against the numpy
statement (tests/_ha_ref.py) before anything is timed.  Appends to profiles/ha_bench.jsonl.  Needs a GPU.

    python tools/bench_ha.py [--reps 7] [--frames 240] [--out PATH]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch

import _ha_ref as HA
import motioncam_decoder_amd as M
from altlib import bench_images, bench_mosaics

PEAK = 8e12
WHITE, BLACK = 4095.0, (64, 64, 64, 64)
GAIN = (2.0, 1.0, 1.6)
MAT = np.array([[1.7, -0.5, -0.2], [-0.25, 1.4, -0.15], [0.05, -0.45, 1.4]], np.float32)
DISTINCT = 2
W, H = 3840, 2160
KINDS = ("f16", "u8", "nv12")
ES = {"f16": 2, "u8": 1, "nv12": 1}
CONTENTS = ("smooth", "noise")
CHUNK = 8  # frames per pass of the torch route: its intermediates are int32 planes of the whole chunk


def samples(kind):
    return H * W * 3 // (2 if kind == "nv12" else 1)


def _pad3(d):
    """101-reflection by 3 samples along the last two axes (torch's reflect padding takes no integer tensors)."""
    d = torch.cat([d[:, 1:4].flip(1), d, d[:, -4:-1].flip(1)], dim=1)
    return torch.cat([d[:, :, 1:4].flip(2), d, d[:, :, -4:-1].flip(2)], dim=2)


def torch_ha_f16(mos, out):
    """algo="ha" (RGGB, equal black levels) of the (m, H, W) uint16 tensor mos from torch ops, into out (m, 3, H, W) f16."""
    m, h, w = mos.shape
    dev = mos.device
    P = _pad3(mos.view(torch.int16).to(torch.int32) - BLACK[0])
    yy = torch.arange(-1, h + 1, device=dev)[:, None] & 1
    xx = torch.arange(-1, w + 1, device=dev)[None, :] & 1
    rb_ring = yy == xx  # RGGB: R and B where both parities agree

    def at(dy, dx):  # on the frame and its ring of one
        return P[:, 2 + dy:4 + dy + h, 2 + dx:4 + dx + w]

    C = at(0, 0)
    ch, cv = 2 * C - at(0, -2) - at(0, 2), 2 * C - at(-2, 0) - at(2, 0)
    gh, gv = 2 * (at(0, -1) + at(0, 1)) + ch, 2 * (at(-1, 0) + at(1, 0)) + cv
    DH, DV = (at(0, -1) - at(0, 1)).abs() + ch.abs(), (at(-1, 0) - at(1, 0)).abs() + cv.abs()
    g = torch.where(rb_ring, torch.where(DH < DV, 2 * gh, torch.where(DV < DH, 2 * gv, gh + gv)), 8 * C)
    del ch, cv, gh, gv, DH, DV

    def dat(dy, dx):
        return P[:, 3 + dy:3 + dy + h, 3 + dx:3 + dx + w]

    def gat(dy, dx):
        return g[:, 1 + dy:1 + dy + h, 1 + dx:1 + dx + w]

    G = gat(0, 0)

    def pair(a, b):
        c = 2 * G - gat(*a) - gat(*b)
        return 8 * (dat(*a) + dat(*b)) + c, 8 * (dat(*a) - dat(*b)).abs() + c.abs()

    hz, vt = 2 * pair((0, -1), (0, 1))[0], 2 * pair((-1, 0), (1, 0))[0]
    nN, DN = pair((-1, -1), (1, 1))
    nP, DP = pair((-1, 1), (1, -1))
    diag = torch.where(DN < DP, 2 * nN, torch.where(DP < DN, 2 * nP, nN + nP))
    del nN, DN, nP, DP
    nat = 32 * dat(0, 0)
    ry = (torch.arange(h, device=dev)[:, None] & 1).expand(h, w)
    rx = (torch.arange(w, device=dev)[None, :] & 1).expand(h, w)
    role = ry * 2 + rx
    E = [torch.where(role == 0, nat, torch.where(role == 3, diag, torch.where(role == 1, hz, vt))),
         torch.where((role == 0) | (role == 3), 4 * G, nat),
         torch.where(role == 3, nat, torch.where(role == 0, diag, torch.where(role == 1, vt, hz)))]
    k = HA.scales(WHITE, BLACK, GAIN)
    v = [E[c].to(torch.float32) * float(k[c]) for c in range(3)]
    for i in range(3):
        out[:, i] = ((float(MAT[i, 0]) * v[0] + float(MAT[i, 1]) * v[1]) + float(MAT[i, 2]) * v[2]).to(torch.float16)
    return out


def run(ctx, n, reps):
    dev = torch.device("cuda:0")
    imgs = {c: bench_images(c, W, H, DISTINCT, np.random.default_rng(7)) for c in CONTENTS}
    mos = {c: bench_mosaics(dev, imgs[c], n) for c in CONTENTS}
    shaded = torch.empty_like(mos["noise"])
    gm = M.gain_map(np.ones((4, 13, 17)) * 1.25)
    dgm = torch.from_numpy(gm.view(np.int16)).to(dev).view(torch.uint16)
    out = torch.empty(n * 3 * W * H * 2, dtype=torch.uint8, device=dev)  # room for the largest form (f16)
    stream = torch.cuda.Stream()
    kw = dict(white=WHITE, black=BLACK, gain=GAIN, matrix=MAT)

    def view(kind):
        t = out[: n * samples(kind) * ES[kind]]
        if kind == "f16":
            return t.view(torch.float16).view(n, 3, H, W)
        return t.view(n, H, W, 3) if kind == "u8" else t.view(n, H * 3 // 2, W)

    def demosaic(kind, algo, content):
        o = view(kind)
        if kind == "f16":
            return ctx.demosaic(mos[content], algo=algo, dtype="f16", out=o, **kw)
        if kind == "u8":
            return ctx.demosaic_display(mos[content], algo=algo, transfer="srgb", lut_size=4096, dtype=torch.uint8, layout="hwc", out=o, **kw)
        return ctx.demosaic_yuv(mos[content], algo=algo, fmt="nv12", transfer="bt709", out=o, **kw)

    def torch_route():
        o = view("f16")
        for f0 in range(0, n, CHUNK):
            torch_ha_f16(mos["smooth"][f0:f0 + CHUNK], o[f0:f0 + CHUNK])
        return o

    forms = {}
    for content in CONTENTS:
        for kind in KINDS:
            for algo in ("ha", "mhc"):
                forms["%s_%s_%s" % (algo, kind, content)] = lambda kind=kind, algo=algo, content=content: demosaic(kind, algo, content)
    forms["kshade"] = lambda: ctx.shade(mos["noise"], dgm, black=BLACK, out=shaded)
    forms["torch_ha_f16_smooth"] = torch_route
    alg = {f: n * W * H * 2 + n * samples(f.split("_")[1]) * ES[f.split("_")[1]] for f in forms if f[:3] in ("ha_", "mhc")}
    alg["kshade"] = 2 * n * W * H * 2
    alg["torch_ha_f16_smooth"] = alg["ha_f16_smooth"]

    torch.cuda.synchronize()
    o0 = HA.rgb_values(imgs["smooth"][0], WHITE, BLACK, "rggb", GAIN, MAT)
    o1 = HA.rgb_values(imgs["noise"][1 % DISTINCT], WHITE, BLACK, "rggb", GAIN, MAT)
    torch_equal = None
    for f in forms:  # warm-up, and the correctness of two frames of two forms
        with torch.cuda.stream(stream):
            res = forms[f]()
        torch.cuda.synchronize()
        if f == "ha_f16_smooth":
            with np.errstate(over="ignore"):
                assert np.array_equal(res[0].view(torch.int16).cpu().numpy().view(np.uint16), o0.astype(np.float16).view(np.uint16)), f
        elif f == "ha_nv12_noise":
            import _yuv_ref as Y
            want = Y.yuv_from_o(o1, M.transfer_lut("bt709", 4096, 12), "nv12", M.yuv_matrix("bt709", "limited", 8, 12), 12)
            assert np.array_equal(res[1].cpu().numpy(), want), f
        elif f == "torch_ha_f16_smooth":  # (reported, not asserted: the torch route is a yardstick, not the product)
            with np.errstate(over="ignore"):
                torch_equal = bool(np.array_equal(res[0].view(torch.int16).cpu().numpy().view(np.uint16), o0.astype(np.float16).view(np.uint16)))
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
    med = {f: float(np.median(ms[f])) for f in forms}
    for f in forms:
        r = {"form": f, "frames": n, "width": W, "height": H, "reps": reps, "batch_ms": round(med[f], 4),
             "batch_ms_min": round(min(ms[f]), 4), "batch_ms_max": round(max(ms[f]), 4), "alg_GB": round(alg[f] / 1e9, 3),
             "frac_peak_batch": round(alg[f] / (med[f] * 1e-3) / PEAK, 3)}
        if f.startswith("ha_"):
            r["ratio_to_mhc"] = round(med[f] / med["mhc_" + f[3:]], 3)
            r["ratio_to_kshade"] = round(med[f] / med["kshade"], 3)
            if f == "ha_f16_smooth":
                r["ratio_to_torch_route"] = round(med[f] / med["torch_ha_f16_smooth"], 4)
        if f == "torch_ha_f16_smooth":
            r["equals_numpy_statement"] = torch_equal
        rows.append(r)
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--frames", type=int, default=240)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ha_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_ha.py needs a GPU")
    ctx = M.Context(0)
    with open(args.out, "a") as fh:
        for r in run(ctx, args.frames, max(3, args.reps)):
            line = json.dumps(r)
            print(line, flush=True)
            fh.write(line + "\n")
    ctx.close()


if __name__ == "__main__":
    main()
