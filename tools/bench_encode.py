#!/usr/bin/env python3
"""The type-7 encoder on HBM-resident mosaics (mcraw_encode_batch, MCRAW_MEM_DEVICE): for each workload, ms per batch
(both launches, events around the call), each kernel's time from the library's event brackets, algorithmic bytes
(input 2 w h + bytes written) and the fraction of the 8 TB/s peak they make; median and spread over REPS batches in one
process.  Every frame of the first batch is checked against the synthesiser's encoder.

    python tools/bench_encode.py [--reps 7] [--only uhd_nat12,uhd_uni16,8k_nat12]
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
import motioncam_decoder_amd as M

PEAK = 8e12
WORKLOADS = {  # name: (frames, width, height, image maker)
    "uhd_nat12": (240, 3840, 2160, lambda w, h, s: L.natural_image_np(w, h, 12, 12.0, s)),
    "uhd_uni16": (240, 3840, 2160, lambda w, h, s: L.uniform_image_np(w, h, 16, s)),
    "8k_nat12": (120, 7680, 4320, lambda w, h, s: L.natural_image_np(w, h, 12, 12.0, s)),
}
DISTINCT = 4  # distinct images per workload (each frame still has buffers of its own)


def run(ctx, name, reps):
    n, w, h, make = WORKLOADS[name]
    dev = torch.device("cuda:0")
    base = [make(w, h, 100 + s) for s in range(DISTINCT)]
    want = [L.encode7(b) for b in base]
    ins = torch.empty((n, h, w), dtype=torch.int16, device=dev)
    for i in range(n):
        ins[i].copy_(torch.from_numpy(base[i % DISTINCT].view(np.int16)))
    cap = M.encode_bound7(w, h)
    out = torch.zeros((n, cap), dtype=torch.uint8, device=dev)
    frames = M.Context.make_enc_frames([(ins[i].data_ptr(), w, h, out[i].data_ptr(), cap) for i in range(n)])
    torch.cuda.synchronize()
    written, status = ctx.encode_batch(frames)
    assert all(s == 0 for s in status), status[:8]
    for i in range(n):
        assert written[i] == len(want[i % DISTINCT]), (i, written[i])
    for i in range(min(n, 2 * DISTINCT)):
        assert np.array_equal(out[i, :written[i]].cpu().numpy(), want[i % DISTINCT]), i
    nbytes = 2 * w * h * n + sum(written)
    ctx.profile(only=["k7e_payload", "k7e_side"])
    ctx.kernel_ms("k7e_payload", reset=True)
    ctx.kernel_ms("k7e_side", reset=True)
    ms, kp, ks = [], [], []
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream = torch.cuda.Stream()  # (not the null stream: the library takes NULL as its own stream)
    for _ in range(reps):
        a.record(stream)
        ctx.encode_batch(frames, stream=stream.cuda_stream, want_status=False)
        b.record(stream)
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
        kp.append(ctx.kernel_ms("k7e_payload", reset=True)[0])
        ks.append(ctx.kernel_ms("k7e_side", reset=True)[0])
    ctx.profile(enable=False)
    med = float(np.median(ms))
    res = {"workload": name, "frames": n, "width": w, "height": h, "reps": reps,
           "batch_ms": round(med, 4), "batch_ms_min": round(min(ms), 4), "batch_ms_max": round(max(ms), 4),
           "k7e_payload_ms": round(float(np.median(kp)), 4), "k7e_side_ms": round(float(np.median(ks)), 4),
           "alg_GB": round(nbytes / 1e9, 3), "out_GB": round(sum(written) / 1e9, 3),
           "frac_peak_batch": round(nbytes / (med * 1e-3) / PEAK, 3),
           "frac_peak_payload": round((2 * w * h * n + sum(written)) / (float(np.median(kp)) * 1e-3) / PEAK, 3)}
    del ins, out
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--only", default="")
    args = ap.parse_args()
    names = [s for s in args.only.split(",") if s] or list(WORKLOADS)
    ctx = M.Context(0)
    for name in names:
        print(json.dumps(run(ctx, name, max(5, args.reps))), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
