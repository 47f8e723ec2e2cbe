"""Child process of tests/test_gpu_rgb_paths.py:  python _rgb_paths_child.py <corpus.npz> <variant>

Loads the build of the library that MCRAW_LIB_PATH names (one with -DMCRAW_PATHSR) and runs every setting of the .npz's plan
(tests/_rgb_paths_model.py SETTINGS) that the variant runs: one call of demosaic / demosaic_display / demosaic_yuv each, on a
strided view of the input (offset, pitch and frame stride are the setting's) into an output that starts `out_off` bytes behind a
16-byte boundary.  Every call's output is compared byte for byte with what the parent worked out from the numpy statements; the
guard bands in front of and behind it must stay as they were filled.  The scaled kernels are called through the C ABI itself
(scaled_call), with a scratch of this script's: what lies behind its work_bytes must stay as filled too.  Prints the census of
each setting as one line  RESULT {json}.  Exit status 1 when a byte differs."""
import ctypes as C
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
import _rgb_paths_model as T  # noqa: E402

GUARD, FILL = 4096, 0xA5
TD = {"u8hwc": torch.uint8, "u8chw": torch.uint8, "u16hwc": torch.uint16, "u16chw": torch.uint16, "nv12": torch.uint8, "p010": torch.uint16,
      "f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}


def scaled_call(ctx, lib, S, view, out, lut, gain, matrix, errors):
    """mcraw_demosaic_area_batch / _resample_batch as Context._demosaic_call makes the call, with a guarded scratch."""
    struct, work_symbol, batch_symbol, _ = M._SCALED[S["kernel"]]
    a = struct()
    a.y0, a.x0, a.ch, a.cw = S["crop"]
    a.out_h, a.out_w = S["size"]
    if S["kernel"] == "resample":
        a.filter = T.RS.FILTER_CODE[S["filt"]]
    need = int(getattr(lib, work_symbol)(C.byref(a)))
    assert need > 0 and need % 16 == 0
    work = torch.full((need + GUARD,), FILL, dtype=torch.uint8, device=out.device)
    d = y = None
    code = 0
    if T.is_float(S):
        code = M._float_code(S["kind"])
    elif T.is_yuv(S):
        fcode, bits, _ = M._YUV_FORMATS[S["kind"]]
        cy, cb, cr, sh, y_off, c_off = M.yuv_matrix("bt709", "limited", bits, T.IN_BITS)
        yv = M.Yuv()
        yv.format, yv.lut_log2, yv.in_bits, yv.sh, yv.y_off, yv.c_off = fcode, int(lut.numel()).bit_length() - 1, T.IN_BITS, sh, y_off, c_off
        for i in (0, 1, 2):
            yv.cy[i], yv.cb[i], yv.cr[i] = cy[i], cb[i], cr[i]
        yv.reserved, yv.lut = 0, lut.data_ptr()
        y = C.byref(yv)
    else:
        dd = M.Display()
        dd.dtype, dd.layout = (M.DISP_U8 if S["kind"][:2] == "u8" else M.DISP_U16), M._DISP_LAYOUTS[S["kind"][-3:]]
        dd.lut_log2, dd.reserved, dd.lut = int(lut.numel()).bit_length() - 1, 0, lut.data_ptr()
        d = C.byref(dd)
    cols, nc = M._rgb_colors(gain, matrix, S["n"], "scaled_call")
    prm = M._rgb_params(S["kernel"], code, 0, S["cfa"], T.WHITE, T.BLACK)
    torch.cuda.synchronize()
    src = ctx._strided("scaled_call", "the mosaic", view, S["H"], S["W"])
    ctx._call(torch, out.device, batch_symbol, (view, out, work), C.byref(prm), C.byref(a), d, y, cols, nc, *src, S["W"], S["H"], S["n"],
              C.c_void_p(work.data_ptr()), need, C.c_void_p(out.data_ptr()), out.numel() * out.element_size())
    torch.cuda.synchronize()
    if not bool((work[need:] == FILL).all()):
        errors.append("%s: wrote behind work_bytes of the scratch" % S["name"])


def main(npz, variant):
    t0 = time.time()
    Z = np.load(npz)
    plan = json.loads(str(Z["plan"]))
    dev = torch.device("cuda:0")
    lib = M.load()
    luts = {n: torch.from_numpy(Z["lut_%d" % n].view(np.int16)).to(dev).view(torch.uint16) for n in (4096, 65536)}
    errors = []

    census = PH.census_reader(lib, "mcraw_diag_rgb_paths", T.PATHS)

    def run(ctx, S):
        n, H, W, kind = S["n"], S["H"], S["W"], S["kind"]
        buf = torch.zeros((S["off"] + n * S["fstride"] + 16,), dtype=torch.int16, device=dev)
        assert buf.data_ptr() % 16 == 0
        view = torch.as_strided(buf, (n, H, W), (S["fstride"], S["pitch"], 1), S["off"])
        view.copy_(torch.from_numpy(Z[S["img"]].view(np.int16)).to(dev))
        view = view.view(torch.uint16)
        want = torch.from_numpy(Z[S["exp"]]).to(dev)
        raw = torch.full((GUARD + S["out_off"] + want.numel() + GUARD,), FILL, dtype=torch.uint8, device=dev)
        assert raw.data_ptr() % 16 == 0
        lo, hi = GUARD + S["out_off"], GUARD + S["out_off"] + want.numel()
        P = T.plan(S)
        ho, wo = P["Ho"], P["Wo"]
        shape = {"hwc": (n, ho, wo, 3), "chw": (n, 3, ho, wo)}[kind[-3:]] if kind[0] == "u" else \
            (n, ho * 3 // 2, wo) if T.is_yuv(S) else (n, 3, ho, wo)
        out = raw[lo:hi].view(TD[kind]).view(shape)
        gain, matrix = T.colours(S)
        kw = dict(algo=S["kernel"], white=T.WHITE, black=T.BLACK, cfa=S["cfa"], gain=gain, matrix=matrix, out=out)
        torch.cuda.synchronize()
        if S["kernel"] in ("area", "resample"):
            scaled_call(ctx, lib, S, view, out, None if T.is_float(S) else luts[S["lutn"]], gain, matrix, errors)
        elif T.is_float(S):
            ctx.demosaic(view, dtype=kind, **kw)
        elif T.is_yuv(S):
            ctx.demosaic_yuv(view, fmt=kind, transfer=luts[S["lutn"]], in_bits=T.IN_BITS, **kw)
        else:
            ctx.demosaic_display(view, dtype=TD[kind], layout=kind[-3:], transfer=luts[S["lutn"]], **kw)
        torch.cuda.synchronize()
        got = raw[lo:hi]
        if not torch.equal(got, want):
            bad = torch.nonzero(got != want).ravel()
            per = want.numel() // n
            errors.append("%s: %d bytes differ, first at %d (frame %d)" % (S["name"], bad.numel(), int(bad[0]), int(bad[0]) // per))
        if not bool((raw[:lo] == FILL).all()) or not bool((raw[hi:] == FILL).all()):
            errors.append("%s: wrote in front of the output or behind it" % S["name"])

    res = {"paths": T.PATHS, "census": {}}
    ctx = M.Context(0)
    try:
        census()  # (start from zero)
        for S in plan:
            if not T.runs(S, variant):
                continue
            run(ctx, S)
            res["census"][S["name"]] = census()
    finally:
        ctx.close()
    return PH.finish(res, errors, t0)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
