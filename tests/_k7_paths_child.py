"""Child process of tests/test_gpu_k7_paths.py:  python _k7_paths_child.py <corpus.npz>

Loads the build of the library that MCRAW_LIB_PATH names (one with -DMCRAW_PATHS7) and decodes the side-stream corpus of the .npz
under each setting of SETTINGS -- the library's own choice and one workgroup per stream pinned: one batch, frame by frame,
reversed batch; every stream in parts (MCRAW_SIDE_SPLIT 2,2 / 4,4 / 3,2 with the last part's count pinned on -- the library would
turn it off for a batch of this many workgroups --, 3,2 also with MCRAW_SIDE_LASTC=0): one batch --
with a context of its own per setting (the environment is read when a context is made; one context at a time).  Every frame is
compared with what the parent worked out (the oracle's pixels and return value, the fuzz suite's status rule); the rows below a
frame coded shorter than asked and a guard band behind every output must stay as they were filled.  Prints the path census of
each setting as one line  RESULT {json}.  Exit status 1 when a frame differs."""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import motioncam_decoder_amd as M  # noqa: E402
import _paths_harness as PH  # noqa: E402

# the order of Path7 in csrc/mcraw_type7.hip
PATHS = ["streams", "rejected", "records", "units", "units_full", "piece_steps", "units_dead", "skipped_units", "dead", "run_passes",
         "run_passes64", "segw_switch", "segw_pieces", "segw_repaired", "segw_rounds2", "segw_resumed", "parts", "part_empty",
         "counted", "spec", "ho_mute", "ho_over", "ho_pass", "ho_last", "ho_hit", "ho_miss", "ho_mute_work", "ho_mute_part1", "lastc_replayed", "replay_units",
         "replay_pieceflag", "replay_tail", "told_late", "items_behind_part0", "truncated_by_tiles"]
# name, environment, orders: "three" = one batch, frame by frame, reversed batch
SETTINGS = [("default", {}, "three"), ("one", {"MCRAW_SIDE_SPLIT": "1,1"}, "three"), ("2,2", {"MCRAW_SIDE_SPLIT": "2,2", "MCRAW_SIDE_LASTC": "1"}, "batch"),
            ("4,4", {"MCRAW_SIDE_SPLIT": "4,4", "MCRAW_SIDE_LASTC": "1"}, "batch"), ("3,2", {"MCRAW_SIDE_SPLIT": "3,2", "MCRAW_SIDE_LASTC": "1"}, "batch"),
            ("3,2 lastc0", {"MCRAW_SIDE_SPLIT": "3,2", "MCRAW_SIDE_LASTC": "0"}, "batch")]
GUARD, FILL = 4096, 0xA5


def main(npz):
    t0 = time.time()
    Z = np.load(npz)
    meta = Z["meta"]  # per frame: w, h, ret
    n = len(meta)
    dev = torch.device("cuda:0")
    lib = M.load()
    tin = [torch.from_numpy(Z["buf%d" % i]).to(dev) for i in range(n)]
    want = []
    for i in range(n):
        a = torch.from_numpy(Z["out%d" % i].view(np.int16).copy()).to(dev)  # the oracle's rows, or one value per tile of 64 x 4 pixels
        if bool(Z["tiled%d" % i]):
            a = a.repeat_interleave(4, 0).repeat_interleave(64, 1)
        want.append(a.reshape(-1))
    errors = []

    census = PH.census_reader(lib, "mcraw_diag_k7_paths", PATHS)

    def decode(ctx, order, how):
        outs = [torch.full((int(meta[i][0]) * int(meta[i][1]) * 2 + GUARD,), FILL, dtype=torch.uint8, device=dev) for i in order]
        torch.cuda.synchronize()
        frames = M.Context.make_frames([(tin[i].data_ptr(), tin[i].numel(), int(meta[i][0]), int(meta[i][1]), 7, o.data_ptr(),
                                         int(meta[i][0]) * int(meta[i][1])) for i, o in zip(order, outs)])
        written, status = ctx.decode_batch(frames)
        torch.cuda.synchronize()
        for i, o, wr, st in zip(order, outs, written, status):
            w, h, ret = int(meta[i][0]), int(meta[i][1]), int(meta[i][2])
            if ret == 0:
                if st == 0 or wr != 0:
                    errors.append("%s: frame %d must fail: status %#x written %d" % (how, i, st, wr))
                if not bool((o[w * h * 2:] == FILL).all()):
                    errors.append("%s: frame %d: wrote behind the output" % (how, i))
                continue
            if st != 0 or wr != ret:
                errors.append("%s: frame %d: status %#x written %d, want 0 and %d" % (how, i, st, wr, ret))
                continue
            nb = ret // w * w * 2  # (a frame coded shorter than `height` leaves the rows below untouched)
            if not torch.equal(o[:nb].view(torch.int16), want[i]):
                bad = torch.nonzero(o[:nb].view(torch.int16) != want[i]).ravel()
                errors.append("%s: frame %d %dx%d: %d pixels differ, first at (%d, %d)" % (how, i, w, h, bad.numel(), int(bad[0]) // w, int(bad[0]) % w))
            if not bool((o[nb:] == FILL).all()):
                errors.append("%s: frame %d: wrote below its rows or behind the output" % (how, i))

    res = {}
    for name, env, orders in SETTINGS:
        for k in ("MCRAW_SIDE_SPLIT", "MCRAW_SIDE_LASTC"):
            os.environ.pop(k, None)
        os.environ.update(env)
        ctx = M.Context(0)
        try:
            census()  # (start from zero)
            decode(ctx, list(range(n)), name + ": one batch")
            if orders == "three":
                for i in range(n):
                    decode(ctx, [i], name + ": alone")
                decode(ctx, list(range(n))[::-1], name + ": reversed batch")
            res[name] = census()
        finally:
            ctx.close()
    return PH.finish(res, errors, t0)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
