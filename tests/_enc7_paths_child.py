"""Child process of tests/test_gpu_enc7_paths.py:  python _enc7_paths_child.py <variant>

Loads the build of the library that MCRAW_LIB_PATH names (one with -DMCRAW_PATHSE) and encodes the batches that
tests/_enc7_model.py plans for the variant, in order, on one context: device-resident with a len_out word per frame, or in
MCRAW_MEM_HOST.  Every frame is compared with synthlib.encode7 byte for byte -- written, status, len_out, and every byte behind
the frame still as it was filled -- and every good result is decoded back on the device to its input.  A frame the host rejects
must leave its buffer untouched.  A frame whose look-back the `lost` build fails must come back with MCRAW_E_DEVICE and nothing
counted, its buffer untouched outside the payload of the segments in front of the lost one (in host memory: untouched).  Prints
the path census of each batch as one line  RESULT {json}.  Exit status 1 when a frame differs."""
import os
import sys
import time

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), HERE]
import _enc7_model as E  # noqa: E402
import _libs as L  # noqa: E402
import motioncam_decoder_amd as M  # noqa: E402
import _paths_harness as PH  # noqa: E402

GUARD, FILL, UNSET = 64, 0xA5, 0x7777777777777777


def main(variant):
    t0 = time.time()
    dev = torch.device("cuda:0")
    lib = M.load()
    errors, want, tin = [], {}, {}

    census = PH.census_reader(lib, "mcraw_diag_k7e_paths", E.PATHS)

    def expect(f):
        if f["name"] not in want:
            want[f["name"]] = L.encode7(f["img"])
            tin[f["name"]] = torch.from_numpy(f["img"]).to(dev)
        return want[f["name"]]

    def check(how, f, i, lost, got, wr, st, ln):
        """got: the frame's whole buffer (bound + GUARD bytes) as numpy."""
        what = "%s: frame %d (%s)" % (how, i, f["name"])
        if ln != wr:
            errors.append("%s: len_out %d, written %d" % (what, ln, wr))
        if f["bad"]:
            if st != f["bad"] or wr != 0 or not (got == FILL).all():
                errors.append("%s: status %#x written %d, want %#x and 0 and an untouched buffer" % (what, st, wr, f["bad"]))
            return False
        w = expect(f)
        if lost and i == 0:
            lo, hi = E.model_of(f["img"]).failed_range()
            if st != E.E_DEVICE or wr != 0:
                errors.append("%s: status %#x written %d, want MCRAW_E_DEVICE and 0" % (what, st, wr))
            if not ((got[:lo] == FILL).all() and (got[hi:] == FILL).all()):
                errors.append("%s: a failed frame touched bytes outside [%d, %d)" % (what, lo, hi))
            if not np.array_equal(got[lo:hi], w[lo:hi]):
                errors.append("%s: the payload in front of the lost segment differs" % what)
            return False
        if st != 0 or wr != len(w):
            errors.append("%s: status %#x written %d, want 0 and %d" % (what, st, wr, len(w)))
            return False
        if not np.array_equal(got[:wr], w):
            bad = np.nonzero(got[:wr] != w)[0]
            errors.append("%s: %d bytes differ, first at %d" % (what, bad.size, bad[0]))
        if not (got[wr:] == FILL).all():
            errors.append("%s: bytes written behind the frame" % what)
        return True

    def caps(batch):
        """(width, height, bound, capacity) of every frame as it is given to the library."""
        out = []
        for f in batch:
            h, w = f["img"].shape
            bound = M.encode_bound7(w, h)
            out.append((0 if f["bad"] == E.E_ARGS else w, h, bound, bound - 1 if f["bad"] == E.E_CAPACITY else bound))
        return out

    def run_device(ctx, how, batch, lost):
        for f in batch:
            expect(f)
        geo = caps(batch)
        outs = [torch.full((bound + GUARD,), FILL, dtype=torch.uint8, device=dev) for _, _, bound, _ in geo]
        lens = torch.full((len(batch),), UNSET, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        descs = [(tin[f["name"]].data_ptr(), w, h, o.data_ptr(), cap, lens.data_ptr() + 8 * i)
                 for i, (f, o, (w, h, _, cap)) in enumerate(zip(batch, outs, geo))]
        written, status = ctx.encode_batch(M.Context.make_enc_frames(descs), mem=M.MEM_DEVICE)
        torch.cuda.synchronize()
        ln = [int(v) for v in lens.cpu().numpy()]
        good = [i for i, (f, o) in enumerate(zip(batch, outs)) if check(how, f, i, lost, o.cpu().numpy(), written[i], status[i], ln[i])]
        # the results go straight back into mcraw_decode_batch
        back = [torch.zeros(batch[i]["img"].size * 2, dtype=torch.uint8, device=dev) for i in good]
        if good:
            dd = [(outs[i].data_ptr(), written[i], batch[i]["w"], batch[i]["h"], 7, b.data_ptr(), batch[i]["img"].size) for i, b in zip(good, back)]
            dw, ds = ctx.decode_batch(M.Context.make_frames(dd), mem=M.MEM_DEVICE)
            torch.cuda.synchronize()
            for i, b, w2, s2 in zip(good, back, dw, ds):
                if s2 != 0 or w2 != batch[i]["img"].size or not torch.equal(b.view(torch.int16), tin[batch[i]["name"]].view(torch.int16).reshape(-1)):
                    errors.append("%s: frame %d (%s) does not decode back to its input: status %#x written %d" % (how, i, batch[i]["name"], s2, w2))

    def run_host(ctx, how, batch, lost):
        geo = caps(batch)
        outs = [np.full(bound + GUARD, FILL, dtype=np.uint8) for _, _, bound, _ in geo]
        lens = np.full(len(batch), UNSET, dtype=np.uint64)
        descs = [(f["img"].ctypes.data, w, h, o.ctypes.data, cap, lens.ctypes.data + 8 * i)
                 for i, (f, o, (w, h, _, cap)) in enumerate(zip(batch, outs, geo))]
        written, status = ctx.encode_batch(M.Context.make_enc_frames(descs), mem=M.MEM_HOST)
        for i, (f, o) in enumerate(zip(batch, outs)):
            if lost and i == 0:  # nothing of a failed frame is copied back
                if status[i] != E.E_DEVICE or written[i] != 0 or int(lens[i]) != 0 or not (o == FILL).all():
                    errors.append("%s: frame 0: status %#x written %d len_out %d, want MCRAW_E_DEVICE, 0, 0 and an untouched buffer"
                                  % (how, status[i], written[i], int(lens[i])))
            else:
                check(how, f, i, False, o, written[i], status[i], int(lens[i]))

    res = {"batches": []}
    ctx = M.Context(0)
    try:
        census()  # (start from zero)
        for name, batch, host, lost in E.plan(variant):
            (run_host if host else run_device)(ctx, name, batch, lost)
            res["batches"].append(census())
    finally:
        ctx.close()
    res["nerrors"] = len(errors)
    return PH.finish(res, errors, t0)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
