"""Child process of tests/test_gpu_k7t_paths.py:  python _k7t_paths_child.py <corpus.npz>

Loads the build of the library that MCRAW_LIB_PATH names (one with -DMCRAW_PATHST) and decodes the corpus of the .npz under each
setting of its plan (tests/_tiles7_model.py SETTINGS: the plain mosaic, the uint16 and strip stages with and without black levels,
the float rows and planes, outputs off their grid, MCRAW_XCD_CHUNK, MCRAW_SIDE_SPLIT) with a context of its own per setting (the
environment is read when a context is made; one context at a time): every frame alone, the mixed frames as one batch.  Every
frame's output is compared byte for byte with what the parent worked out from the oracle; the bytes in front of an output that
does not start on the allocation, the rows below a frame coded shorter than asked and a guard band behind every output must stay
as they were filled.  Prints the census of each setting as one line  RESULT {json}.  Exit status 1 when a frame differs."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
import motioncam_decoder_amd as M  # noqa: E402
import _paths_harness as PH  # noqa: E402

# the order of PathT in csrc/mcraw_type7.hip
PATHS = (["waves", "invalid", "short", "tiles_skipped", "span_empty", "span_full", "head", "wg_remap", "wg_chunked"]
         + ["cls%d" % c for c in range(10)]
         + ["pair_diff", "wrap_lanes", "lean", "notlean", "fail_bits", "fail_ref", "fail_top", "fail_wrap",
            "drop_y", "drop_x", "st_aligned", "st_unaligned", "st_cropped", "st_merged_fwd", "st_merged_back",
            "decl_partial", "decl_notin"])
ENV_KEYS = ("MCRAW_XCD_CHUNK", "MCRAW_SIDE_SPLIT", "MCRAW_SIDE_LASTC")
GUARD, FILL = 4096, 0xA5


def main(npz):
    t0 = time.time()
    Z = np.load(npz)
    plan = json.loads(str(Z["plan"]))
    meta = Z["meta"]  # per frame: w, h, ret
    dev = torch.device("cuda:0")
    lib = M.load()
    tin = [torch.from_numpy(Z["buf%d" % i]).to(dev) for i in range(len(meta))]
    errors = []

    census = PH.census_reader(lib, "mcraw_diag_k7t_paths", PATHS)

    def decode(ctx, s, S, order):
        off = int(S["off"])
        want = [torch.from_numpy(Z["exp_%d_%d" % (s, i)]).to(dev) for i in order]
        alloc = [int(S["alloc"][str(i)]) for i in order]
        outs = [torch.full((off + a + GUARD,), FILL, dtype=torch.uint8, device=dev) for a in alloc]
        assert all(o.data_ptr() % 16 == 0 for o in outs)
        torch.cuda.synchronize()
        frames = M.Context.make_frames([(tin[i].data_ptr(), tin[i].numel(), int(meta[i][0]), int(meta[i][1]), 7, o.data_ptr() + off, (a + 1) // 2)
                                        for i, o, a in zip(order, outs, alloc)])
        written, status = ctx.decode_batch(frames)
        torch.cuda.synchronize()
        for i, o, wt, wr, st in zip(order, outs, want, written, status):
            how = "%s: frame %d %dx%d" % (S["name"], i, int(meta[i][0]), int(meta[i][1]))
            if st != 0 or wr != int(meta[i][2]):
                errors.append("%s: status %#x written %d, want 0 and %d" % (how, st, wr, int(meta[i][2])))
                continue
            got = o[off:off + wt.numel()]
            if not torch.equal(got, wt):
                bad = torch.nonzero(got != wt).ravel()
                errors.append("%s: %d bytes differ, first at %d" % (how, bad.numel(), int(bad[0])))
            if not bool((o[:off] == FILL).all()) or not bool((o[off + wt.numel():] == FILL).all()):
                errors.append("%s: wrote in front of the output, below its rows or behind it" % how)

    res = {"paths": PATHS}
    for s, S in enumerate(plan):
        for k in ENV_KEYS:
            os.environ.pop(k, None)
        os.environ.update(S["env"])
        ctx = M.Context(0)
        try:
            if S["stage"] and S["stage"][0] == "post":
                ctx.set_post(**S["stage"][1])
            elif S["stage"]:
                ctx.set_float_out(**S["stage"][1])
            census()  # (start from zero)
            for order in S["batches"]:
                decode(ctx, s, S, order)
            res[S["name"]] = census()
        finally:
            ctx.close()
    return PH.finish(res, errors, t0)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
