"""Child process of tests/test_gpu_k6_paths.py:  python _k6_paths_child.py <corpus.npz>

Loads the build of the library that MCRAW_LIB_PATH names (one with -DMCRAW_PATHS6), decodes the legacy corpus of the .npz as one
batch, frame by frame and as one batch in reversed order, the frames of 16 and more segments once more as a batch of their own,
and a few frames through the fused stages of k6_decode<POST> (12-bit strips, f16 planes); compares every frame with what the
parent worked out (the oracle's pixels and return value, the fuzz suite's status rule) and prints the path census of each part
as one line  RESULT {json}.  Exit status 1 when a frame differs."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import motioncam_decoder_amd as M  # noqa: E402
import _paths_harness as PH  # noqa: E402

# the order of Path6 in csrc/mcraw_type6.hip
PATHS = ["segments", "careful", "repaired", "front0", "latefront", "nofront", "maps", "lb_scalar", "lb_vector", "lb_handed",
         "noted", "coop", "noncoop", "waves", "waves_pair", "waves_multi", "lost"]


def main(npz):
    t0 = time.time()
    Z = np.load(npz)
    meta = Z["meta"]  # per frame: w, h, ret, segments
    n = len(meta)
    bufs = [Z["buf%d" % i] for i in range(n)]
    want = [Z["out%d" % i] for i in range(n)]
    dev = torch.device("cuda:0")
    lib = M.load()
    ctx = M.Context(0)
    tin = [torch.from_numpy(b).to(dev) for b in bufs]
    errors = []

    census = PH.census_reader(lib, "mcraw_diag_k6_paths", PATHS)

    def decode(order, how):
        outs = [torch.zeros(int(meta[i][0]) * int(meta[i][1]) * 2, dtype=torch.uint8, device=dev) for i in order]
        torch.cuda.synchronize()
        frames = M.Context.make_frames([(tin[i].data_ptr(), tin[i].numel(), int(meta[i][0]), int(meta[i][1]), 6, o.data_ptr(),
                                         int(meta[i][0]) * int(meta[i][1])) for i, o in zip(order, outs)])
        written, status = ctx.decode_batch(frames)
        torch.cuda.synchronize()
        for i, o, wr, st in zip(order, outs, written, status):
            w, h, ret = int(meta[i][0]), int(meta[i][1]), int(meta[i][2])
            if ret == 0:
                if st == 0 or wr != 0:
                    errors.append("%s: frame %d must fail: status %#x written %d" % (how, i, st, wr))
                continue
            if st != 0 or wr != ret:
                errors.append("%s: frame %d: status %#x written %d, want 0 and %d" % (how, i, st, wr, ret))
                continue
            rows = ret // w  # (a frame coded shorter than `height` leaves the rows below untouched)
            got = o.cpu().numpy().view(np.uint16).reshape(h, w)
            if not np.array_equal(got[:rows], want[i][:rows]):
                bad = np.argwhere(got[:rows] != want[i][:rows])
                errors.append("%s: frame %d %dx%d: %d pixels differ, first at %s" % (how, i, w, h, len(bad), bad[0].tolist()))

    census()  # (start from zero)
    decode(list(range(n)), "one batch")
    for i in range(n):
        decode([i], "alone")
    decode(list(range(n))[::-1], "reversed batch")
    res = {"plain": census()}
    decode([i for i in range(n) if int(meta[i][3]) >= 16], "frames of 16 and more segments")
    res["big"] = census()

    # the fused stages share the unpack loop: 12-bit strips and f16 planes of a few frames
    sub = [int(i) for i in Z["post_frames"]]
    black, white, plane = [int(v) for v in Z["post_black"]], float(Z["post_white"]), [int(v) for v in Z["post_plane"]]

    def staged(what, nbytes_of):
        outs = [torch.full((nbytes_of(i) + 64,), 0xA5, dtype=torch.uint8, device=dev) for i in sub]
        torch.cuda.synchronize()
        frames = M.Context.make_frames([(tin[i].data_ptr(), tin[i].numel(), int(meta[i][0]), int(meta[i][1]), 6, o.data_ptr(),
                                         (nbytes_of(i) + 1) // 2) for i, o in zip(sub, outs)])
        written, status = ctx.decode_batch(frames)
        torch.cuda.synchronize()
        for i, o, wr, st in zip(sub, outs, written, status):
            ref = Z["%s%d" % (what, i)].ravel()
            a = o.cpu().numpy()
            if st != 0 or wr != int(meta[i][2]):
                errors.append("%s: frame %d: status %#x written %d" % (what, i, st, wr))
            elif not np.array_equal(a[:ref.size], ref):
                errors.append("%s: frame %d: %d bytes differ, first at %d" % (what, i, int((a[:ref.size] != ref).sum()), int(np.flatnonzero(a[:ref.size] != ref)[0])))
            elif not (a[ref.size:] == 0xA5).all():
                errors.append("%s: frame %d: wrote behind the output" % (what, i))

    ctx.set_post(black=black, bits=12)
    try:
        staged("strip", lambda i: Z["strip%d" % i].size)
    finally:
        ctx.set_post()
    ctx.set_float_out("f16", white, layout="planes", black=tuple(black), clip=False, plane=plane)
    try:
        staged("planes", lambda i: Z["planes%d" % i].size)
    finally:
        ctx.set_post()
    res["post"] = census()
    ctx.close()
    return PH.finish(res, errors, t0)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
