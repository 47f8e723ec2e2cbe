"""Child process of tests/test_gpu_noise.py::test_one_strip_per_workgroup:  python _noise_strip_child.py

Loads the build of the library that MCRAW_LIB_PATH names (build.NOISE_STRIP_FLAGS: knoise with one strip per workgroup) and runs
three calls of Context.noise_stats whose frames have 6, 34 and 6 strips: that many workgroups add their LDS counters to one frame's
record.  Every call's records, with the sentinels around them, are compared with the numpy statement (_noise_ref).  Prints one line
RESULT {json}.  Exit status 1 when something differs."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import motioncam_decoder_amd as M  # noqa: E402
import _noise_ref as NR  # noqa: E402
import _paths_harness as PH  # noqa: E402

DEV = torch.device("cuda:0")
GUARD, SENT = 4096, 0xA5
CALLS = ((2, 48, 1040), (1, 272, 1040), (3, 96, 272))  # frames, H, W


def main():
    t0, errors, strips = time.time(), [], []
    ctx = M.Context(0)
    try:
        for k, (n, H, W) in enumerate(CALLS):
            rng = np.random.default_rng(40 + k)
            yy, xx = np.mgrid[0:H, 0:W]
            img = (xx * 3 + yy * 5)[None] + np.rint(rng.standard_normal((n, H, W)) * rng.integers(1, 50, size=(n, 1, 1))).astype(np.int64)
            img = np.clip(img + 100, 0, 4095).astype(np.uint16)
            strips.append((H // 16) * ((W // 16 + 63) // 64))
            t = torch.from_numpy(img.view(np.int16)).to(DEV).view(torch.uint16)
            buf = torch.full((GUARD + n * NR.REC_BYTES + GUARD,), SENT, dtype=torch.uint8, device=DEV)
            out = buf[GUARD:GUARD + n * NR.REC_BYTES].view(n, NR.REC_BYTES)
            ctx.noise_stats(t, shift=7, sat=4095, lo=1, out=out)
            torch.cuda.synchronize()
            host = buf.cpu().numpy()
            if not ((host[:GUARD] == SENT).all() and (host[-GUARD:] == SENT).all()):
                errors.append("call %d: written outside the records" % k)
            want = NR.record(NR.noise_stats(img, 7, 4095, 1))
            if not np.array_equal(host[GUARD:-GUARD].reshape(n, NR.REC_BYTES), want):
                errors.append("call %d: the records differ from the numpy statement" % k)
    finally:
        ctx.close()
    return PH.finish({"calls": len(CALLS), "strips": strips}, errors, t0)


if __name__ == "__main__":
    sys.exit(main())
