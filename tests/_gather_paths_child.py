"""Child process of tests/test_gpu_warp_paths.py, test_gpu_mesh_paths.py and test_gpu_ha_paths.py:
    python _gather_paths_child.py <corpus.npz> <kernel: warp | mesh | ha> <variant>

Loads the build of the library that MCRAW_LIB_PATH names (one of build.RGB_PATH_VARIANTS) and runs every case of the .npz's plan
(tests/_gather_paths_model.py cases(kernel)) that the variant runs: one call of demosaic / demosaic_display / demosaic_yuv each with
algo = the kernel, on a strided view of the input (offset, pitch and frame stride are the case's) into an output that starts
`out_off` bytes behind a 16-byte boundary.  Every call's output is compared byte for byte with what the parent worked out from the
numpy statement; the guard bands in front of and behind it must stay as they were filled.  Prints the census of each case as one
line  RESULT {json}.  Exit status 1 when a byte differs."""
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


def main(npz, kernel, variant):
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
        ho, wo = S["size"]
        yuv, flt = kind in ("nv12", "p010"), kind in T.FLOAT_KINDS
        shape = (n, ho * 3 // 2, wo) if yuv else (n, ho, wo, 3) if kind[-3:] == "hwc" else (n, 3, ho, wo)
        out = raw[lo:hi].view(TD[kind]).view(shape)
        kw = dict(algo=kernel, white=S["white"], black=tuple(S["black"]), cfa=S["cfa"], gain=Z["gain_%d" % n], matrix=Z["matrix_%d" % n], out=out)
        if kernel == "warp":
            kw.update(size=(ho, wo), affine=Z[S["geokey"]], filter=S["filt"])
        elif kernel == "mesh":  # a device tensor is taken as it is: no node content is an error
            kw.update(size=(ho, wo), mesh=torch.from_numpy(Z[S["geokey"]]).to(dev), filter=S["filt"])
        torch.cuda.synchronize()
        if flt:
            ctx.demosaic(view, dtype=kind, **kw)
        elif yuv:
            ctx.demosaic_yuv(view, fmt=kind, transfer=luts[S["lutn"]], in_bits=S["in_bits"], **kw)
        else:
            ctx.demosaic_display(view, dtype=TD[kind], layout=kind[-3:], transfer=luts[S["lutn"]], **kw)
        torch.cuda.synchronize()
        got = raw[lo:hi]
        if not torch.equal(got, want):
            bad = torch.nonzero(got != want).ravel()
            errors.append("%s: %d bytes differ, first at %d (frame %d)" % (S["name"], bad.numel(), int(bad[0]), int(bad[0]) // (want.numel() // n)))
        if not bool((raw[:lo] == FILL).all()) or not bool((raw[hi:] == FILL).all()):
            errors.append("%s: wrote in front of the output or behind it" % S["name"])

    res = {"paths": T.PATHS, "census": {}, "cases": 0}
    ctx = M.Context(0)
    try:
        census()  # (start from zero)
        for S in plan:
            if S["kind"] in T.FLOAT_KINDS and T.VARIANT_CAP[variant] is not None:
                continue  # the float kinds have no loop to force
            run(ctx, S)
            res["census"][S["name"]] = census()
            res["cases"] += 1
    finally:
        ctx.close()
    return PH.finish(res, errors, t0)


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:4]))
