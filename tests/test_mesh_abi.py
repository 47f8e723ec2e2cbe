"""The mesh warp of the demosaic (mcraw_demosaic_mesh_batch, mcraw_mesh_nodes, mcraw_mesh_check) without a GPU: the ABI's symbols,
macros and struct, every rejection driven through the library with its exact message (a rejected call touches neither the context
nor the device, and the nodes are only an address), mcraw_mesh_check's verdicts and messages, and code 7 in the older entry
points."""
import ctypes as C
import os
import re

import numpy as np

import _mesh_ref as MR
import motioncam_decoder_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYM = "mcraw_demosaic_mesh_batch"


def _hdr():
    return open(os.path.join(ROOT, "include", "mcraw_hip.h")).read()


def test_mesh_symbols_macros_and_struct():
    hdr = _hdr()
    lib = M.load()
    for sym in (SYM, "mcraw_mesh_nodes", "mcraw_mesh_check"):
        assert re.search(r"\b%s\s*\(" % sym, hdr) and sym in M.ABI_SYMBOLS and hasattr(lib, sym), sym
    assert re.search(r"#define MCRAW_RGB_MESH\s+7\b", hdr) and M.RGB_MESH == 7
    assert re.search(r"#define MCRAW_MESH_STEP\s+32\b", hdr) and M.MESH_STEP == 32
    assert re.search(r"#define MCRAW_K_COUNT\s+11\b", hdr)  # no kernel id of its own
    for name in ("Mesh", "RGB_MESH", "MESH_STEP", "mesh_grid", "affine_mesh", "distortion_mesh", "stabilize_mesh", "mesh_check"):
        assert name in M.__all__
    assert hdr.index("} mcraw_warp;") < hdr.index("sampled along one displacement mesh per frame") < hdr.index("} mcraw_mesh;")  # behind the warp block
    block = hdr[hdr.index("sampled along one displacement mesh per frame"):hdr.index("} mcraw_mesh;")]
    for line in ("Yr = (Y00 (32-u)(32-v) + Y01 (32-u) v + Y10 u (32-v) + Y11 u v + 512) >> 10", "Y = min(max(Yr, 0), 256 (height - 1))",
                 "np' = min(np, 26)", "ne' = min(ne, 8)", "[pb, pb + 2 np' - 4]", "[eb, eb + 8 ne' - 4]", "k[c] = (gain[c] * inv) * 0.0625f",
                 "DEVICE memory", "ANY node content"):
        assert line in block, line
    names = ("out_w", "out_h", "filter", "reserved")
    assert C.sizeof(M.Mesh) == 16 and [getattr(M.Mesh, f).offset for f in names] == [0, 4, 8, 12]
    m = re.search(r"\}\s*mcraw_mesh;\s*/\*\s*sizeof (\d+); out_h (\d+), filter (\d+), reserved (\d+)", hdr)
    assert m and [int(v) for v in m.groups()] == [16, 4, 8, 12]


def _mesh(out_w=70, out_h=40, filt=1, reserved=0):
    m = M.Mesh()
    m.out_w, m.out_h, m.filter, m.reserved = out_w, out_h, filt, reserved
    return m


def test_mesh_nodes():
    lib = M.load()
    for (ho, wo) in ((40, 70), (1, 1), (32, 32), (33, 64), (65536, 65536)):
        assert lib.mcraw_mesh_nodes(C.byref(_mesh(wo, ho))) == int(np.prod(M.mesh_grid(ho, wo))) == int(np.prod(MR.grid((ho, wo))))
    assert lib.mcraw_mesh_nodes(None) == 0
    for bad in (_mesh(out_w=0), _mesh(out_h=65537), _mesh(filt=2), _mesh(reserved=1)):
        assert lib.mcraw_mesh_nodes(C.byref(bad)) == 0


class _Call:
    """One call of the entry point with every argument good unless replaced.  The context is a dummy block that a rejected call
    (and an empty batch) never looks into; addresses are only looked at as numbers."""

    def __init__(self):
        self.ctx = C.create_string_buffer(4096)
        self.lib = M.load()

    def __call__(self, **kw):
        a = dict(ctx=C.addressof(self.ctx), algo=7, dtype=1, flags=0, cfa=0, white=4095.0, out_w=70, out_h=40, filter=1, reserved=0,
                 d=None, y=None, ncolors=1, nodes=0x400000, nodes_bytes=2 * 3 * 4 * 8, nmesh=2, inp=0x100000, pitch=136, fstride=136 * 72,
                 width=136, height=72, n=2, out=0x200000, out_bytes=1 << 24, prm=True, mp=True, gain=(1.0, 1.0, 1.0))
        a.update(kw)
        p = M.RgbParams()
        p.algo, p.dtype, p.flags, p.cfa, p.white = a["algo"], a["dtype"], a["flags"], a["cfa"], a["white"]
        m = _mesh(a["out_w"], a["out_h"], a["filter"], a["reserved"])
        cols = (M.RgbColor * max(a["ncolors"], 1))()
        for c in cols:
            for i in range(3):
                c.gain[i] = a["gain"][i]
                c.m[4 * i] = 1.0
        rc = getattr(self.lib, SYM)(a["ctx"], C.byref(p) if a["prm"] else None, C.byref(m) if a["mp"] else None,
                                    C.byref(a["d"]) if a["d"] is not None else None, C.byref(a["y"]) if a["y"] is not None else None,
                                    cols, a["ncolors"], C.c_void_p(a["nodes"]), a["nodes_bytes"], a["nmesh"], C.c_void_p(a["inp"]),
                                    a["pitch"], a["fstride"], a["width"], a["height"], a["n"], C.c_void_p(a["out"]), a["out_bytes"], None)
        return rc, self.lib.mcraw_last_error().decode()


def _display(lut=0x300000):
    d = M.Display()
    d.dtype, d.layout, d.lut_log2, d.reserved, d.lut = M.DISP_U8, M.DISP_HWC, 12, 0, lut
    return d


def _yuv(lut=0x300000):
    cy, cb, cr, sh, y_off, c_off = M.yuv_matrix("bt709", "limited", 8, 11)
    y = M.Yuv()
    y.format, y.lut_log2, y.in_bits, y.sh, y.y_off, y.c_off, y.reserved, y.lut = M.YUV_NV12, 12, 11, sh, y_off, c_off, 0, lut
    for i in range(3):
        y.cy[i], y.cb[i], y.cr[i] = cy[i], cb[i], cr[i]
    return y


def test_every_rejection_through_the_library():
    call = _Call()
    bad = [(dict(ctx=None), "bad arguments"), (dict(prm=False), "bad arguments"), (dict(mp=False), "bad arguments"),
           (dict(nodes=0), "bad arguments"), (dict(n=-1), "bad arguments"),
           (dict(d=_display(), y=_yuv(), dtype=0), "a display stage and a YUV stage at once"),
           (dict(width=6), "width and height must be even, 8 .. 65536"), (dict(height=6), "width and height must be even, 8 .. 65536"),
           (dict(width=137, pitch=140), "width and height must be even, 8 .. 65536"), (dict(height=73), "width and height must be even, 8 .. 65536"),
           (dict(width=65538, pitch=65538), "width and height must be even, 8 .. 65536"),
           (dict(algo=1), "p->algo must be MCRAW_RGB_MESH"), (dict(algo=5), "p->algo must be MCRAW_RGB_MESH"),
           (dict(algo=6), "p->algo must be MCRAW_RGB_MESH"), (dict(algo=8), "p->algo must be MCRAW_RGB_MESH"),
           (dict(dtype=7), "unknown dtype"), (dict(flags=2), "unknown flag"), (dict(cfa=4), "unknown cfa"),
           (dict(white=0.0), "white must be finite and above the mean black level"),
           (dict(white=float("nan")), "white must be finite and above the mean black level"),
           (dict(ncolors=0), "ncolors must be 1 or n"), (dict(ncolors=3), "ncolors must be 1 or n"),
           (dict(gain=(float("inf"), 1.0, 1.0)), "non-finite gain or matrix entry"),
           (dict(d=_display(), dtype=1), "p->dtype and p->flags must be 0 (the display / YUV stage decides the output)"),
           (dict(d=_display(lut=0), dtype=0), "lut missing or not 16-byte aligned"),
           (dict(d=_display(lut=0x300008), dtype=0), "lut missing or not 16-byte aligned"),
           (dict(reserved=1), "reserved must be 0"), (dict(filter=2), "unknown filter"),
           (dict(out_w=0), "out_w and out_h must be 1 .. 65536"), (dict(out_h=0), "out_w and out_h must be 1 .. 65536"),
           (dict(out_w=65537), "out_w and out_h must be 1 .. 65536"), (dict(out_h=65537), "out_w and out_h must be 1 .. 65536"),
           (dict(y=_yuv(), dtype=0, out_w=69), "4:2:0 needs an even out_h and out_w"),
           (dict(y=_yuv(), dtype=0, out_h=39), "4:2:0 needs an even out_h and out_w"),
           (dict(nmesh=0), "nmesh must be 1 or n"), (dict(nmesh=3), "nmesh must be 1 or n"), (dict(nmesh=-1), "nmesh must be 1 or n"),
           (dict(nodes=0x400004), "nodes not 8-byte aligned"),
           (dict(nodes_bytes=2 * 3 * 4 * 8 - 1), "nodes_bytes below nmesh * My * Mx * 8"),
           (dict(nmesh=1, nodes_bytes=3 * 4 * 8 - 1), "nodes_bytes below nmesh * My * Mx * 8"),
           (dict(out=0), "in / out missing or not aligned to their element size"),
           (dict(out=0x200002), "in / out missing or not aligned to their element size"),
           (dict(out_bytes=2 * 3 * 40 * 70 * 4 - 1), "out_bytes below n * 3 * Ho * Wo * element size")]
    for kw, why in bad:
        rc, msg = call(**kw)
        assert rc < 0 and msg == SYM + ": " + why, (kw, rc, msg)
    for kw in (dict(inp=0), dict(inp=0x100001), dict(pitch=135), dict(fstride=136 * 72 - 1)):  # the mosaic batch's own messages
        rc, msg = call(**kw)
        assert rc < 0 and msg.startswith(SYM + ": "), (kw, rc, msg)
    # warp_check's order: the frame in front of the algo, the algo in front of the stage, the geometry in front of the nodes
    assert call(width=6, algo=1)[1].endswith("8 .. 65536") and call(algo=1, dtype=7)[1].endswith("MCRAW_RGB_MESH")
    assert call(reserved=1, nmesh=3)[1].endswith("reserved must be 0") and call(nmesh=3, out=0)[1].endswith("nmesh must be 1 or n")
    # an empty batch is a no-op whatever else is wrong with it; one mesh for the batch needs half the bytes
    assert call(n=0, out=0, inp=0, nmesh=5)[0] == 0
    # the older entry points keep their own messages for code 7
    lib = M.load()
    p = M.RgbParams()
    p.algo, p.dtype, p.white = 7, 1, 4095.0
    col = (M.RgbColor * 1)()
    for i in range(3):
        col[0].gain[i] = 1.0
    ctx, inp, out = C.addressof(call.ctx), C.c_void_p(0x100000), C.c_void_p(0x200000)
    assert lib.mcraw_demosaic_batch(ctx, C.byref(p), col, 1, inp, 40, 960, 40, 24, 1, out, 1 << 24, None) < 0
    assert lib.mcraw_last_error().decode() == "mcraw_demosaic_batch: unknown algo"
    p.dtype = 0
    d, y = _display(), _yuv()
    assert lib.mcraw_demosaic_display_batch(ctx, C.byref(p), C.byref(d), col, 1, inp, 40, 960, 40, 24, 1, out, 1 << 24, None) < 0
    assert lib.mcraw_last_error().decode() == "mcraw_demosaic_display_batch: unknown algo"
    assert lib.mcraw_demosaic_yuv_batch(ctx, C.byref(p), C.byref(y), col, 1, inp, 40, 960, 40, 24, 1, out, 1 << 24, None) < 0
    assert lib.mcraw_last_error().decode() == "mcraw_demosaic_yuv_batch: unknown algo"
    p.dtype = 1
    w = M.Warp()
    w.out_w, w.out_h, w.filter = 16, 12, 1
    maps = (C.c_int32 * 6)(65536, 0, 0, 0, 65536, 0)
    assert lib.mcraw_demosaic_warp_batch(ctx, C.byref(p), C.byref(w), None, None, col, 1, maps, 1, inp, 40, 960, 40, 24, 1, out, 1 << 24, None) < 0
    assert lib.mcraw_last_error().decode() == "mcraw_demosaic_warp_batch: p->algo must be MCRAW_RGB_WARP"
    a = M.Area()
    a.cw, a.ch, a.out_w, a.out_h = 40, 24, 20, 12
    work = C.c_void_p(0x500000)
    assert lib.mcraw_demosaic_area_batch(ctx, C.byref(p), C.byref(a), None, None, col, 1, inp, 40, 960, 40, 24, 1, work, 1 << 20, out, 1 << 24, None) < 0
    assert lib.mcraw_last_error().decode() == "mcraw_demosaic_area_batch: p->algo must be MCRAW_RGB_AREA"
    r = M.Resample()
    r.cw, r.ch, r.out_w, r.out_h, r.filter = 40, 24, 40, 24, 1
    assert lib.mcraw_demosaic_resample_batch(ctx, C.byref(p), C.byref(r), None, None, col, 1, inp, 40, 960, 40, 24, 1, work, 1 << 20, out, 1 << 24, None) < 0
    assert lib.mcraw_last_error().decode() == "mcraw_demosaic_resample_batch: p->algo must be MCRAW_RGB_RESAMPLE"


def _check(mesh, size, height, width, flags=0, nmesh=None):
    lib = M.load()
    a = np.ascontiguousarray(np.asarray(mesh, dtype=np.int32).reshape((-1,) + MR.grid(size) + (2,)))
    rc = lib.mcraw_mesh_check(C.byref(_mesh(size[1], size[0])), a.ctypes.data_as(C.POINTER(C.c_int32)), a.shape[0] if nmesh is None else nmesh,
                              width, height, flags)
    return rc, lib.mcraw_last_error().decode()


def test_mesh_check_verdicts_and_messages():
    H, Wd, size = 120, 328, (40, 70)
    good = MR.translation_mesh(size, 3, 5)
    assert _check(good, size, H, Wd)[0] == 0 and _check(good, size, H, Wd, 1)[0] == 0
    ext = M.affine_mesh([[81920, 16384, 0, -16384, 81920, 256 * 12]], size)[0]  # the affine warp's extreme linear part: still the regime
    assert MR.in_regime(ext, size, H, Wd) and _check(ext, size, H, Wd)[0] == 0
    # a tile 132 samples across: tile (0, 1) of frame 1 leaves the regime, and the statement agrees
    wide = good.copy()
    wide[:, 2:, 1] += 256 * 100
    assert not MR.in_regime(wide, size, H, Wd)
    rc, msg = _check(np.stack([good, wide]), size, H, Wd)
    assert rc < 0 and msg.startswith("mcraw_mesh_check: the mesh of frame 1: tile (0, 1) reads ") and msg.endswith("above 26 x 8"), msg
    tall = good.copy()
    tall[2, :, 0] += 256 * 200   # rows 32 .. 39 of the output spread over 7 + 7 * 200 / 32 source rows
    assert not MR.in_regime(tall, size, H, Wd)
    rc, msg = _check(np.stack([tall, wide]), size, H, Wd)
    assert rc < 0 and "frame 0: tile (1, 0) reads" in msg, msg
    # nodes outside the frame: fine for the regime (the clamp), named with flags & 1
    out = MR.translation_mesh(size, -2, 5)
    assert _check(out, size, H, Wd)[0] == 0
    rc, msg = _check(out, size, H, Wd, 1)
    assert rc < 0 and msg == "mcraw_mesh_check: the mesh of frame 0: a corner pixel of tile (0, 0) leaves the frame: (-512, 1280)", msg
    far = MR.translation_mesh(size, 3, 260)  # the last column of the last tile: pixel 69 reads 329 > 327
    rc, msg = _check(far, size, H, Wd, 1)
    assert rc < 0 and "tile (0, 2) leaves the frame" in msg, msg
    # a node behind the last partial tile may lie anywhere as long as the tile's own pixels stay put
    virt = good.astype(np.int64)
    virt[2, :, 0] = 2 * virt[1, :, 0] - virt[0, :, 0]   # (the same slope: rows 32 .. 39 read where they did)
    assert _check(virt.astype(np.int32), size, H, Wd, 1)[0] == 0
    for kw, why in ((dict(height=6), "width and height must be even, 8 .. 65536"), (dict(nmesh=0), "nmesh must be at least 1"), (dict(flags=2), "unknown flag")):
        rc, msg = _check(good, size, kw.get("height", H), Wd, kw.get("flags", 0), kw.get("nmesh"))
        assert rc < 0 and msg == "mcraw_mesh_check: " + why, msg
    lib = M.load()
    assert lib.mcraw_mesh_check(None, None, 1, Wd, H, 0) < 0 and lib.mcraw_last_error().decode() == "mcraw_mesh_check: bad arguments"
