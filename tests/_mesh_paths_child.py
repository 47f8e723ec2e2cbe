"""Child process of tests/test_gpu_mesh_paths.py:  python _mesh_paths_child.py <corpus.npz>

Loads the build of the library that MCRAW_LIB_PATH names (one of build.RGB_PATH_VARIANTS with a capped grid: grid1, grid3) and runs every case
of the .npz's plan through Context.demosaic_display / demosaic_yuv with algo="mesh": 3 frames with per-frame meshes (a CUDA
tensor, used in place) and colours over 2 x 3 tiles each.  Every call's output is compared byte for byte with what the parent worked out from the numpy statement; the
guard bands in front of and behind it must stay as they were filled.  Prints one line  RESULT {json}.  Exit status 1 when a byte
differs."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import motioncam_decoder_amd as M  # noqa: E402
import _paths_harness as PH  # noqa: E402

GUARD, FILL = 4096, 0xA5


def main(npz):
    t0 = time.time()
    Z = np.load(npz)
    plan = json.loads(str(Z["plan"]))
    dev = torch.device("cuda:0")
    ctx = M.Context(0)
    imgs = torch.from_numpy(Z["imgs"].view(np.int16)).to(dev).view(torch.uint16)
    meshes = torch.from_numpy(Z["meshes"]).to(dev)
    errors = []
    for S in plan:
        lut = torch.from_numpy(Z["lut_%d" % S["lutn"]].view(np.int16)).to(dev).view(torch.uint16)
        exp = Z[S["exp"]]
        yuv = S["kind"] in ("nv12", "p010")
        td = torch.uint8 if S["kind"] in ("u8", "nv12") else torch.uint16
        ho, wo = S["size"]
        n = imgs.shape[0]
        shape = (n, ho * 3 // 2, wo) if yuv else ((n, ho, wo, 3) if S["layout"] == "hwc" else (n, 3, ho, wo))
        buf = torch.full((exp.size + 2 * GUARD,), FILL, dtype=torch.uint8, device=dev)
        out = buf[GUARD:GUARD + exp.size].view(td).view(shape)
        kw = dict(algo="mesh", size=(ho, wo), mesh=meshes, filter=S["filt"], white=S["white"], black=tuple(S["black"]), cfa=S["cfa"],
                  gain=Z["gain"], matrix=Z["matrix"], transfer=lut, out=out)
        if yuv:
            ctx.demosaic_yuv(imgs, fmt=S["kind"], in_bits=S["in_bits"], **kw)
        else:
            ctx.demosaic_display(imgs, dtype=td, layout=S["layout"], **kw)
        torch.cuda.synchronize()
        host = buf.cpu().numpy()
        if not ((host[:GUARD] == FILL).all() and (host[GUARD + exp.size:] == FILL).all()):
            errors.append("%s: wrote outside out" % S["name"])
        bad = np.flatnonzero(host[GUARD:GUARD + exp.size] != exp)
        if bad.size:
            errors.append("%s: %d bytes differ, the first at %d" % (S["name"], bad.size, int(bad[0])))
    ctx.close()
    return PH.finish({"cases": len(plan)}, errors, t0)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
