#!/usr/bin/env python3
"""Decode into normalised float tensors (mcraw_ctx_set_float_out) on HBM-resident frames, against the plain uint16
decode of the same buffers: ms per batch (events around the call on a torch stream), each kernel's ms from the
library's event brackets, algorithmic bytes (input bytes + output bytes) and the fraction of the 8 TB/s peak.  All
numbers come from ONE process and one set of buffers, the forms taking turns rep by rep (fresh processes differ by a
few per cent on these kernels).  Frames 0 and 1 of every form are checked against the numpy reference.

    python tools/bench_float.py [--reps 9] [--only t7_uhd,t6_12mp]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import numpy as np
import torch

import _float_ref as R
import _libs as L
import motioncam_decoder_amd as M

PEAK = 8e12
WHITE, BLACK = 4095.0, (64, 64, 64, 64)
# form: (dtype, layout, clip); None = the plain uint16 mosaic
FORMS = {"plain": None, "f16_planes": ("f16", "planes", False), "bf16_planes": ("bf16", "planes", False),
         "f32_planes": ("f32", "planes", False), "f16_mosaic": ("f16", "mosaic", False), "f16_planes_clip": ("f16", "planes", True)}
WORKLOADS = {  # name: (type, frames, width, height, forms)
    "t7_uhd": (7, 240, 3840, 2160, list(FORMS)),
    "t6_12mp": (6, 32, 4000, 3000, ["plain", "f16_planes"]),
}
DISTINCT = 4
KERNEL = {7: "k7_tiles", 6: "k6_decode"}


def run(ctx, name, reps):
    typ, n, w, h, forms = WORKLOADS[name]
    dev = torch.device("cuda:0")
    imgs = [L.natural_image_np(w, h, 12, 12.0, 100 + s) for s in range(DISTINCT)]
    bufs = [L.encode7(im) if typ == 7 else L.encode6(im) for im in imgs]
    stride = max(len(b) for b in bufs) + 256
    ins = torch.zeros((n, stride), dtype=torch.uint8, device=dev)
    lens = []
    for i in range(n):
        b = bufs[i % DISTINCT]
        ins[i, :len(b)].copy_(torch.from_numpy(b))
        lens.append(len(b))
    out = torch.empty(n * w * h * 4, dtype=torch.uint8, device=dev)  # room for the largest form (f32)
    stream = torch.cuda.Stream()  # (not the null stream: the library takes NULL as its own stream)
    frames, obytes = {}, {}
    for f in forms:
        fb = w * h * (4 if f != "plain" and FORMS[f][0] == "f32" else 2)
        obytes[f] = fb * n
        frames[f] = M.Context.make_frames([(ins[i].data_ptr(), lens[i], w, h, typ, out.data_ptr() + i * fb, fb // 2) for i in range(n)])

    def stage(f):
        if FORMS[f] is None:
            ctx.set_post()
        else:
            d, lay, clip = FORMS[f]
            ctx.set_float_out(d, WHITE, layout=lay, black=BLACK, clip=clip, plane=M.cfa_planes("rggb"))

    torch.cuda.synchronize()
    for f in forms:  # correctness of every form, and warm-up
        stage(f)
        written, status = ctx.decode_batch(frames[f])
        assert all(s == 0 for s in status), (f, status[:8])
        fb = obytes[f] // n
        for i in range(2):
            got = out[i * fb:(i + 1) * fb].cpu().numpy()
            if FORMS[f] is None:
                want = imgs[i % DISTINCT].view(np.uint8).ravel()
            else:
                d, lay, clip = FORMS[f]
                want = R.ref_bytes(imgs[i % DISTINCT], d, WHITE, lay, BLACK, clip, M.cfa_planes("rggb"))
            assert np.array_equal(got, want), (name, f, i)
    kname = KERNEL[typ]
    ctx.profile(only=[kname])
    ctx.kernel_ms(kname, reset=True)
    ms = {f: [] for f in forms}
    km = {f: [] for f in forms}
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(reps):
        for f in forms:  # the forms take turns
            stage(f)
            a.record(stream)
            ctx.decode_batch(frames[f], stream=stream.cuda_stream, want_status=False)
            b.record(stream)
            torch.cuda.synchronize()
            ms[f].append(a.elapsed_time(b))
            km[f].append(ctx.kernel_ms(kname, reset=True)[0])
    ctx.profile(enable=False)
    ctx.set_post()
    ctx.synchronize()
    assert ctx.errors() == 0
    res = []
    inb = sum(lens)
    base = float(np.median(ms["plain"]))
    for f in forms:
        med, kmed = float(np.median(ms[f])), float(np.median(km[f]))
        nbytes = inb + obytes[f]
        res.append({"workload": name, "form": f, "frames": n, "width": w, "height": h, "reps": reps,
                    "batch_ms": round(med, 4), "batch_ms_min": round(min(ms[f]), 4), "batch_ms_max": round(max(ms[f]), 4),
                    kname + "_ms": round(kmed, 4), "vs_plain": round(med / base, 4),
                    "alg_GB": round(nbytes / 1e9, 3), "in_GB": round(inb / 1e9, 3), "out_GB": round(obytes[f] / 1e9, 3),
                    "frac_peak_batch": round(nbytes / (med * 1e-3) / PEAK, 3),
                    "frac_peak_kernel": round(nbytes / (kmed * 1e-3) / PEAK, 3)})
    del ins, out
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    names = [s for s in args.only.split(",") if s] or list(WORKLOADS)
    ctx = M.Context(0)
    for name in names:
        for r in run(ctx, name, max(3, args.reps)):
            print(json.dumps(r), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
