"""The edge-directed demosaic (MCRAW_RGB_HA, algo="ha") without a GPU: the ABI's macro and the contract's text, the code object,
what the three classic entry points decide about algo 6 driven through the library (a rejected call touches neither the context
nor the device), the three scaled entry points' answer to 6, the Python layer's names, and the stand-alone C++ check of the
plan and of the kernel's LDS indices (tests/cpp/ha_args_check.cpp), plain and under ASan and UBSan."""
import ctypes as C
import os
import re
import subprocess

import pytest

import motioncam_decoder_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "motioncam_decoder_amd", "csrc")
ENTRIES = ("mcraw_demosaic_batch", "mcraw_demosaic_display_batch", "mcraw_demosaic_yuv_batch")


def _hdr():
    return open(os.path.join(ROOT, "include", "mcraw_hip.h")).read()


def test_macro_contract_and_names():
    hdr = _hdr()
    assert re.search(r"#define MCRAW_RGB_HA\s+6\b", hdr) and M.RGB_HA == 6 and "RGB_HA" in M.__all__
    assert M._RGB_ALGOS["ha"] == 6 and "ha" not in M._SCALED
    assert re.search(r"#define MCRAW_K_COUNT\s+11\b", hdr)  # no kernel id of its own
    block = hdr[hdr.index("the edge-directed demosaic: MCRAW_RGB_HA"):hdr.index("#define MCRAW_RGB_HA")]
    for line in ("ch = 2 C - d[y][x-2] - d[y][x+2]", "gh = 2 (d[y][x-1] + d[y][x+1]) + ch", "DH = |d[y][x-1] - d[y][x+1]| + |ch|",
                 "g  = 2 gh if DH < DV, 2 gv if DV < DH, gh + gv if they are equal", "E_G = 4 g", "n(a, b) = 8 (d_a + d_b) + (2 g - g_a - g_b)",
                 "D(a, b) = 8 |d_a - d_b| + |2 g - g_a - g_b|", "2 n(N) if D(N) < D(P), 2 n(P) if D(P) < D(N), n(N) + n(P) if equal",
                 "|g| <= 16 * 65535", "10 485 600 < 2^24", "k[c] = (gain[c] * inv) * 0.03125f", "up to 3 samples"):
        assert line in block, line


def test_code_object_has_the_kernel():
    assert b"krgb_ha" in open(M.lib_path(), "rb").read()


# ---- through the library: a call that is rejected is decided from the arguments alone

def _display(lut=0x300000, **kw):
    d = M.Display()
    d.dtype, d.layout, d.lut_log2, d.reserved, d.lut = M.DISP_U8, M.DISP_HWC, 12, 0, lut
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _yuv(lut=0x300000, **kw):
    cy, cb, cr, sh, y_off, c_off = M.yuv_matrix("bt709", "limited", 8, 11)
    y = M.Yuv()
    y.format, y.lut_log2, y.in_bits, y.sh, y.y_off, y.c_off, y.reserved, y.lut = M.YUV_NV12, 12, 11, sh, y_off, c_off, 0, lut
    for i in range(3):
        y.cy[i], y.cb[i], y.cr[i] = cy[i], cb[i], cr[i]
    for k, v in kw.items():
        setattr(y, k, v)
    return y


class _Call:
    """One call of a classic entry point (family 0: float, 1: display, 2: YUV) with every argument good unless replaced.  The
    context is a dummy block that a rejected call (and an empty batch) never looks into; addresses are only looked at as numbers."""

    def __init__(self, family):
        self.ctx = C.create_string_buffer(4096)
        self.lib = M.load()
        self.family = family

    def __call__(self, **kw):
        a = dict(ctx=C.addressof(self.ctx), algo=6, dtype=1 if self.family == 0 else 0, flags=0, cfa=0, white=4095.0, black=(0, 0, 0, 0),
                 stage=(None, _display(), _yuv())[self.family], ncolors=1, inp=0x100000, pitch=40, fstride=40 * 24, width=40, height=24,
                 n=2, out=0x200000, out_bytes=1 << 24, prm=True, gain=(1.0, 1.0, 1.0))
        a.update(kw)
        p = M.RgbParams()
        p.algo, p.dtype, p.flags, p.cfa, p.white = a["algo"], a["dtype"], a["flags"], a["cfa"], a["white"]
        for i in range(4):
            p.black[i] = a["black"][i]
        cols = (M.RgbColor * max(a["ncolors"], 1))()
        for c in cols:
            for i in range(3):
                c.gain[i] = a["gain"][i]
                c.m[4 * i] = 1.0
        structs = [C.byref(p) if a["prm"] else None]
        if self.family:
            structs.append(C.byref(a["stage"]) if a["stage"] is not None else None)
        rc = getattr(self.lib, ENTRIES[self.family])(a["ctx"], *structs, cols, a["ncolors"], C.c_void_p(a["inp"]), a["pitch"], a["fstride"],
                                                      a["width"], a["height"], a["n"], C.c_void_p(a["out"]), a["out_bytes"], None)
        return rc, self.lib.mcraw_last_error().decode()


LAST = "in / out missing or not aligned to their element size"  # rgb_check's last question, behind the algo, the stage and the sizes


@pytest.mark.parametrize("family", (0, 1, 2))
def test_the_classic_entry_points_accept_6_up_to_the_device(family):
    """Nothing here may reach the device (the context is a dummy): a call that is good but for what rgb_check asks last -- `out` -- is
    turned down with that question's words, so every check in front of it, the algo's among them, has passed; one step earlier the
    size of `out` is asked; and an empty batch is a no-op."""
    call = _Call(family)
    need = {0: 2 * 3 * 24 * 40 * 4, 1: 2 * 3 * 24 * 40, 2: 2 * 24 * 40 * 3 // 2}[family]
    for algo in (1, 6):  # MHC's geometry: full resolution
        rc, msg = call(algo=algo, out=0)
        assert rc < 0 and msg == ENTRIES[family] + ": " + LAST, (algo, msg)
        rc, msg = call(algo=algo, out=0, out_bytes=need)
        assert rc < 0 and msg == ENTRIES[family] + ": " + LAST, (algo, msg)
        rc, msg = call(algo=algo, out_bytes=need - 1)
        assert rc < 0 and "out_bytes below" in msg, (algo, msg)
    rc, msg = call(algo=2, out=0, out_bytes=need // 4)  # (BIN2's is a quarter: 6 is not taken for it)
    assert rc < 0 and msg.endswith(LAST)
    rc, msg = call(algo=6, out_bytes=need // 4)
    assert rc < 0 and "out_bytes below" in msg
    assert call(n=0, out=0, inp=0)[0] == 0
    for algo in (0, 3, 4, 5, 7):
        rc, msg = call(algo=algo)
        assert rc < 0 and msg == ENTRIES[family] + ": unknown algo", (algo, msg)


@pytest.mark.parametrize("family", (0, 1, 2))
def test_every_rejection_of_mhc_is_hit_with_6(family):
    call = _Call(family)
    bad = [dict(ctx=None), dict(prm=False), dict(n=-1), dict(width=2), dict(height=2), dict(width=41), dict(height=25),
           dict(width=65538, pitch=65538), dict(inp=0), dict(inp=0x100001), dict(pitch=39), dict(fstride=40 * 24 - 1),
           dict(dtype=7), dict(flags=2), dict(cfa=4), dict(white=0.0), dict(white=float("nan")), dict(white=float("inf")),
           dict(black=(5000, 5000, 5000, 5000)), dict(ncolors=0), dict(ncolors=3), dict(gain=(float("inf"), 1.0, 1.0)),
           dict(gain=(1.0, float("nan"), 1.0)), dict(out=0), dict(out_bytes=100)]
    if family == 0:
        bad += [dict(dtype=0), dict(out=0x200002)]
    else:
        bad += [dict(stage=None), dict(dtype=1), dict(flags=1)]
    if family == 1:
        bad += [dict(stage=_display(dtype=3)), dict(stage=_display(layout=2)), dict(stage=_display(reserved=1)), dict(stage=_display(lut_log2=7)),
                dict(stage=_display(lut_log2=17)), dict(stage=_display(lut=0)), dict(stage=_display(lut=0x300008)),
                dict(stage=_display(dtype=M.DISP_U16), out=0x200001)]
    if family == 2:
        bad += [dict(stage=_yuv(format=3)), dict(stage=_yuv(reserved=1)), dict(stage=_yuv(lut_log2=7)), dict(stage=_yuv(lut=0)),
                dict(stage=_yuv(lut=0x300008)), dict(stage=_yuv(in_bits=7)), dict(stage=_yuv(in_bits=17)), dict(stage=_yuv(sh=0)),
                dict(stage=_yuv(sh=25)), dict(stage=_yuv(y_off=256)), dict(stage=_yuv(c_off=-1)),
                dict(stage=_yuv(format=M.YUV_P010), out=0x200001)]
        over = _yuv(in_bits=16)
        over.cb[1] = 1 << 21  # 4 * 65535 * 2^21 is far beyond 2^31: the overflow rule
        bad.append(dict(stage=over))
    for kw in bad:
        rc1, msg1 = call(algo=1, **kw)
        rc6, msg6 = call(algo=6, **kw)
        assert rc1 < 0 and rc6 < 0 and msg1 == msg6 and msg6.startswith(ENTRIES[family] + ": ") and "unknown algo" not in msg6, (kw, msg1, msg6)


def test_the_scaled_entry_points_answer_6_as_before():
    lib = M.load()
    ctx = C.create_string_buffer(4096)
    p = M.RgbParams()
    p.algo, p.dtype, p.white = 6, 1, 4095.0
    col = (M.RgbColor * 1)()
    for i in range(3):
        col[0].gain[i] = 1.0
        col[0].m[4 * i] = 1.0
    a = M.Area()
    a.x0, a.y0, a.cw, a.ch, a.out_w, a.out_h = 0, 0, 40, 24, 20, 12
    work = int(lib.mcraw_area_work_bytes(C.byref(a)))
    assert work > 0
    rc = lib.mcraw_demosaic_area_batch(C.addressof(ctx), C.byref(p), C.byref(a), None, None, col, 1, C.c_void_p(0x100000), 40, 960, 40, 24, 1,
                                       C.c_void_p(0x400000), work, C.c_void_p(0x200000), 1 << 24, None)
    assert rc < 0 and lib.mcraw_last_error().decode() == "mcraw_demosaic_area_batch: p->algo must be MCRAW_RGB_AREA"
    r = M.Resample()
    r.x0, r.y0, r.cw, r.ch, r.out_w, r.out_h, r.filter = 0, 0, 40, 24, 30, 18, 1
    work = int(lib.mcraw_resample_work_bytes(C.byref(r)))
    assert work > 0
    rc = lib.mcraw_demosaic_resample_batch(C.addressof(ctx), C.byref(p), C.byref(r), None, None, col, 1, C.c_void_p(0x100000), 40, 960, 40, 24,
                                           1, C.c_void_p(0x400000), work, C.c_void_p(0x200000), 1 << 24, None)
    assert rc < 0 and lib.mcraw_last_error().decode() == "mcraw_demosaic_resample_batch: p->algo must be MCRAW_RGB_RESAMPLE"
    w = M.Warp()
    w.out_w, w.out_h, w.filter, w.reserved = 16, 12, 1, 0
    maps = (C.c_int32 * 6)(65536, 0, 0, 0, 65536, 0)
    rc = lib.mcraw_demosaic_warp_batch(C.addressof(ctx), C.byref(p), C.byref(w), None, None, col, 1, maps, 1, C.c_void_p(0x100000), 40, 960,
                                       40, 24, 1, C.c_void_p(0x200000), 1 << 24, None)
    assert rc < 0 and lib.mcraw_last_error().decode() == "mcraw_demosaic_warp_batch: p->algo must be MCRAW_RGB_WARP"


def test_python_names():
    with pytest.raises(ValueError, match="'ha'"):
        M.fit_crop(24, 40, 12, 20, algo="ha")  # a scaled algo it is not
    assert "ha" in M.Context.demosaic.__doc__ and "Hamilton-Adams" in M.Context.demosaic.__doc__


@pytest.mark.parametrize("flags", (["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]),
                         ids=("plain", "asan_ubsan"))
def test_ha_args_without_hip(tmp_path, flags):
    """rgb_check's answers to algo 6 (MHC's plan over a sweep of sizes and families; MHC's rejections, word for word) and krgb_ha's
    tile (mcraw_ha_args.h): every LDS index of every item of every tile of a sweep of frame sizes inside the arrays, every entry of
    the green plane written once, for an R / B site, and read for that very site.  A stand-alone host program, once plain and once
    under ASan and UBSan."""
    exe = str(tmp_path / "ha_args_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I" + CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "ha_args_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr.strip(), (r.stdout[-3000:], r.stderr[-3000:])
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "wrong 0", r.stdout[-3000:]
    assert int(re.match(r"cases (\d+)", lines[-2]).group(1)) >= 1000000, lines[-2]
    assert int(re.match(r"tiles (\d+)", lines[-3]).group(1)) >= 1000, lines[-3]
    acc, rej = (int(v) for v in re.match(r"accepted (\d+) rejected (\d+)", lines[-4]).groups())
    assert acc >= 300 and rej >= 60, lines[-4]
