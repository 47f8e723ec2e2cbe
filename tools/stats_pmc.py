#!/usr/bin/env python3
"""The statistics kernel under hardware counters: launches kstats once per form (B = 256 and B = 4096 on noise, smooth, flat
and half-clipped UHD frames) so that a counter run sees one dispatch per form, in this order.  Run it under the profiler, in a
run of its own (counters and tracing do not mix):

    rocprofv3 --pmc SQ_LDS_BANK_CONFLICT SQ_LDS_ADDR_CONFLICT SQ_ACTIVE_INST_LDS SQ_WAIT_INST_LDS \\
        -d DIR -o stats --output-format csv -- python tools/stats_pmc.py [--frames 24]

With --summarize FILE it prints the counters of the kstats dispatches of such a run's counter_collection.csv, summed per
dispatch, in launch order.  Needs a GPU (without --summarize).
"""
import argparse
import csv
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tools")]

ORDER = [(c, b) for c in ("noise", "smooth", "flat", "halfclip") for b in (256, 4096)]


def summarize(path):
    rows = {}
    for r in csv.DictReader(open(path)):
        if "kstats" not in r["Kernel_Name"] or "kstats_init" in r["Kernel_Name"]:
            continue
        d = rows.setdefault(int(r["Dispatch_Id"]), {})
        d[r["Counter_Name"]] = d.get(r["Counter_Name"], 0.0) + float(r["Counter_Value"])
    for (content, bins), (disp, d) in zip(ORDER, sorted(rows.items())):
        print("%-9s B=%-5d dispatch %-4d %s" % (content, bins, disp, "  ".join("%s=%.4g" % kv for kv in sorted(d.items()))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=24)
    ap.add_argument("--summarize", default=None)
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize)
    import numpy as np
    import torch
    import bench_stats as BS
    import motioncam_decoder_amd as M
    ctx = M.Context(0)
    dev = torch.device("cuda:0")
    for content in ("noise", "smooth", "flat", "halfclip"):
        imgs = BS.frames(content, np.random.default_rng(7))
        mos = torch.empty((args.frames, BS.H, BS.W), dtype=torch.uint16, device=dev)
        for i in range(args.frames):
            mos.view(torch.int16)[i].copy_(torch.from_numpy(imgs[i % BS.DISTINCT].view(np.int16)))
        for bins, shift in ((256, 4), (4096, 0)):
            ctx.stats(mos, bins=bins, shift=shift, sat=BS.SAT)
            torch.cuda.synchronize()
    ctx.close()


if __name__ == "__main__":
    main()
