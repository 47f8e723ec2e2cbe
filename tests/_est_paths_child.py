"""Child process of tests/test_gpu_est_paths.py:  python _est_paths_child.py <corpus.npz> <variant>

Loads the build of the library that MCRAW_LIB_PATH names (one with the estimators' census, build.EST_PATH_VARIANTS) and runs every
setting of tests/_est_paths_model.py SETTINGS through the raw ABI, on the setting's view of the input (offset, pitch and frame
stride): mcraw_align_batch and mcraw_align_cells_batch twice each, with a scratch that this script filled with 0xFF bytes and then
with 0x00 bytes -- the columns between w and pitch of the pyramid's planes, the sums that no kernel zeroes, the winners of the
pairless frames --, mcraw_noise_batch once or twice into records that held 0xA5 bytes (the second call accumulates).  pos, sad and
the records are compared with what the parent worked out from the numpy statements, the two fills' results with each other, and the
input must stay as it was.  The census is read, and started over, after every call of align and cells and after a setting of
noise.  Prints one line  RESULT {json}.  Exit status 1 when something differs."""
import ctypes as C
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import motioncam_decoder_amd as M  # noqa: E402
import _paths_harness as PH  # noqa: E402
import _est_paths_model as T  # noqa: E402

DEV = torch.device("cuda:0")
FILLS = (0xFF, 0x00)


def main(npz, variant):
    t0 = time.time()
    lib = M.load()
    Z = np.load(npz)
    errors = []

    census = PH.census_reader(lib, "mcraw_diag_est_paths", T.PATHS, as_dict=False)

    def run(ctx, i, name, S):
        H, W, n, fam = S["H"], S["W"], S["n"], S["family"]
        off, pitch, fstride = T.view_geom(S)
        ibuf = torch.zeros((off + n * fstride + 16,), dtype=torch.int16, device=DEV)
        assert ibuf.data_ptr() % 16 == 0
        torch.as_strided(ibuf, (n, H, W), (fstride, pitch, 1), off).copy_(torch.from_numpy(T.images(name).view(np.int16)).to(DEV))
        before = ibuf.clone()
        src = C.c_void_p(ibuf.data_ptr() + 2 * off)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        out = []
        if fam == "noise":
            rec = torch.full((n, M.NOISE_RECORD_BYTES), 0xA5, dtype=torch.uint8, device=DEV)
            s = M.Noise()
            s.shift, (s.y0, s.x0, s.h, s.w), s.reserved = T.NS_SHIFT, S["roi"], 0
            for p in range(4):
                s.sat[p], s.lo[p] = T.NS_SAT[p], T.NS_LO[p]
            for call in range(S["calls"]):
                s.flags = M.NOISE_ACCUMULATE if call else 0
                rc = lib.mcraw_noise_batch(ctx._h, C.byref(s), src, pitch, fstride, W, H, n, C.c_void_p(rec.data_ptr()), rec.numel(), stream)
                assert rc == 0, (name, lib.mcraw_last_error())
            torch.cuda.synchronize()
            if not np.array_equal(rec.cpu().numpy(), Z["rec_%d" % i]):
                errors.append("%s: the records differ" % name)
            out.append(census())
        else:
            cells = fam == "cells"
            if cells:
                cy, cx = M.cell_grid(H, W, S["cell"])
                g = T.centres(name)
                gpos = None if g is None else torch.from_numpy(np.ascontiguousarray(g, dtype=np.int16)).to(DEV)
                need = lib.mcraw_align_cells_work_bytes(W, H, n, S["levels"], S["radius"], *S["cell"])
                a = M.AlignCells()
                a.cell_h, a.cell_w = S["cell"]
                a.gpos = None if gpos is None else gpos.data_ptr()
                shape = (n, cy, cx)
            else:
                need = lib.mcraw_align_work_bytes(W, H, n, S["levels"], S["radius"])
                a = M.Align()
                shape = (n,)
            assert need > 0, name
            a.levels, a.radius, a.ref, a.reserved = S["levels"], S["radius"], S["ref"], 0
            for p in range(4):
                a.black[p] = T.black(S)[p]
            first = None
            for fill in FILLS:
                work = torch.full((need,), fill, dtype=torch.uint8, device=DEV)
                pos = torch.full(shape + (2,), 0x5A5A, dtype=torch.int16, device=DEV)
                sad = torch.full(shape, 0x5A5A5A5A, dtype=torch.int64, device=DEV)
                a.pos, a.sad, a.work, a.work_bytes = pos.data_ptr(), sad.data_ptr(), work.data_ptr(), need
                fn = lib.mcraw_align_cells_batch if cells else lib.mcraw_align_batch
                rc = fn(ctx._h, C.byref(a), src, pitch, fstride, W, H, n, stream)
                assert rc == 0, (name, lib.mcraw_last_error())
                torch.cuda.synchronize()
                got = (pos.cpu().numpy(), sad.cpu().numpy().view(np.uint64))
                if not np.array_equal(got[0], Z["pos_%d" % i]):
                    bad = np.argwhere(got[0] != Z["pos_%d" % i])
                    errors.append("%s, scratch of 0x%02X: %d positions differ, first at %s: %s, not %s"
                                  % (name, fill, len(bad), bad[0].tolist(), got[0][tuple(bad[0])], Z["pos_%d" % i][tuple(bad[0])]))
                if not np.array_equal(got[1], Z["sad_%d" % i]):
                    bad = np.argwhere(got[1] != Z["sad_%d" % i])
                    errors.append("%s, scratch of 0x%02X: %d sums differ, first at %s: %s, not %s"
                                  % (name, fill, len(bad), bad[0].tolist(), got[1][tuple(bad[0])], Z["sad_%d" % i][tuple(bad[0])]))
                if first is not None and not (np.array_equal(first[0], got[0]) and np.array_equal(first[1], got[1])):
                    errors.append("%s: the results depend on what the scratch held" % name)
                first = got
                out.append(census())
        if not torch.equal(ibuf, before):
            errors.append("%s: the input was written" % name)
        return out

    res = {"paths": T.PATHS, "census": {}}
    ctx = M.Context(0)
    try:
        census()  # (start from zero)
        for i, (name, S) in enumerate(T.SETTINGS.items()):
            res["census"][name] = run(ctx, i, name, S)
    finally:
        ctx.close()
    return PH.finish(res, errors, t0)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else ""))
