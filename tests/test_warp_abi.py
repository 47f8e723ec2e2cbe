"""The affine warp of the demosaic (mcraw_demosaic_warp_batch) without a GPU: the ABI's symbol, macro and struct, every rejection
driven through the library (a rejected call touches neither the context nor the device), the numpy statement of the contract
(_warp_ref) against a scalar one written straight from the header, the properties the contract names (the phase tables, whole-
sample translations, flat frames), the int32 formulation the kernel uses against the exact sums at the extreme inputs, and the
distance from a float64 warp with the unquantised kernel at the unquantised positions."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _resample_ref as S
import _rgb_ref as R
import _warp_ref as W
import motioncam_decoder_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFAS = ("rggb", "bggr", "grbg", "gbrg")
FILTERS = ("linear", "cubic")
SYM = "mcraw_demosaic_warp_batch"
ID = W.IDENTITY


def _hdr():
    return open(os.path.join(ROOT, "include", "mcraw_hip.h")).read()


def test_warp_symbol_exported_and_listed():
    hdr = _hdr()
    lib = M.load()
    assert re.search(r"\b%s\s*\(" % SYM, hdr) and SYM in M.ABI_SYMBOLS and hasattr(lib, SYM)
    assert re.search(r"#define MCRAW_RGB_WARP\s+5\b", hdr) and M.RGB_WARP == 5
    assert re.search(r"#define MCRAW_K_COUNT\s+11\b", hdr)  # no kernel id of its own
    for name in ("Warp", "RGB_WARP", "quantize_affine", "fit_affine", "stabilize"):
        assert name in M.__all__
    assert hdr.index("} mcraw_resample;") < hdr.index("sampled along one affine map per frame")  # behind the resample block
    block = hdr[hdr.index("sampled along one affine map per frame"):hdr.index("} mcraw_warp;")]
    for line in ("Y = ty + ((ayy i + ayx k + 128) >> 8)", "X = tx + ((axy i + axx k + 128) >> 8)", "iy = Y >> 8,  py = Y & 255",
                 "w(p) = (0, 16 (256 - p), 16 p, 0)", "a = 4 |256 j - p|", "w(128) = (-256, 2304, 2304, -256)",
                 "t_c(r, k) = (sum_j w(px)[j] e_c(r, ix - 1 + j) + 2048) >> 12", "E_c(i, k) = (sum_j w(py)[j] t_c(iy - 1 + j, k) + 2048) >> 12",
                 "k[c] = (gain[c] * inv) * 0.0625f", "e_c(reflect101(y, height), reflect101(x, width))", "aliases"):
        assert line in block, line


def test_warp_struct_layout():
    names = ("out_w", "out_h", "filter", "reserved")
    assert C.sizeof(M.Warp) == 16
    assert [getattr(M.Warp, f).offset for f in names] == [0, 4, 8, 12]
    m = re.search(r"\}\s*mcraw_warp;\s*/\*\s*sizeof (\d+); out_h (\d+), filter (\d+), reserved (\d+)", _hdr())
    assert m and [int(v) for v in m.groups()] == [16, 4, 8, 12]


# ---- rejections, through the library: a rejected call is decided from the arguments alone

class _Call:
    """One call of the entry point with every argument good unless replaced.  The context is a dummy block that a rejected call
    (and an empty batch) never looks into; addresses are only looked at as numbers."""

    def __init__(self):
        self.ctx = C.create_string_buffer(4096)
        self.lib = M.load()

    def __call__(self, **kw):
        a = dict(ctx=C.addressof(self.ctx), algo=5, dtype=1, flags=0, cfa=0, white=4095.0, out_w=16, out_h=12, filter=1, reserved=0,
                 d=None, y=None, ncolors=1, maps=[ID], nmaps=None, inp=0x100000, pitch=40, fstride=40 * 24, width=40, height=24, n=2,
                 out=0x200000, out_bytes=1 << 24, prm=True, wp=True, gain=(1.0, 1.0, 1.0))
        a.update(kw)
        p = M.RgbParams()
        p.algo, p.dtype, p.flags, p.cfa, p.white = a["algo"], a["dtype"], a["flags"], a["cfa"], a["white"]
        w = M.Warp()
        w.out_w, w.out_h, w.filter, w.reserved = a["out_w"], a["out_h"], a["filter"], a["reserved"]
        cols = (M.RgbColor * max(a["ncolors"], 1))()
        for c in cols:
            for i in range(3):
                c.gain[i] = a["gain"][i]
                c.m[4 * i] = 1.0
        maps = None
        if a["maps"] is not None:
            flat = np.ascontiguousarray(np.asarray(a["maps"], dtype=np.int32).reshape(-1, 6))
            maps = flat.ctypes.data_as(C.POINTER(C.c_int32))
        nmaps = (0 if a["maps"] is None else len(a["maps"])) if a["nmaps"] is None else a["nmaps"]
        rc = getattr(self.lib, SYM)(a["ctx"], C.byref(p) if a["prm"] else None, C.byref(w) if a["wp"] else None,
                                    C.byref(a["d"]) if a["d"] is not None else None, C.byref(a["y"]) if a["y"] is not None else None,
                                    cols, a["ncolors"], maps, nmaps, C.c_void_p(a["inp"]), a["pitch"], a["fstride"], a["width"],
                                    a["height"], a["n"], C.c_void_p(a["out"]), a["out_bytes"], None)
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


def _m(ayy=65536, ayx=0, ty=0, axy=0, axx=65536, tx=0):
    return (ayy, ayx, ty, axy, axx, tx)


def test_every_rejection_through_the_library():
    call = _Call()
    # 16 x 12 onto a 40 x 24 frame: the identity may move by 0 .. 256 * 12 rows and 0 .. 256 * 24 columns
    bad = [dict(ctx=None), dict(prm=False), dict(wp=False), dict(maps=None, nmaps=1), dict(n=-1), dict(d=_display(), y=_yuv(), dtype=0),
           dict(algo=1), dict(algo=4), dict(algo=6), dict(dtype=7), dict(flags=2), dict(cfa=4), dict(white=0.0), dict(white=float("nan")),
           dict(ncolors=0), dict(ncolors=3), dict(gain=(float("inf"), 1.0, 1.0)),
           dict(width=6), dict(height=6), dict(width=41), dict(height=25), dict(width=65538, pitch=65538),
           dict(inp=0), dict(inp=0x100001), dict(pitch=39), dict(fstride=40 * 24 - 1),
           dict(reserved=1), dict(filter=2), dict(out_w=0), dict(out_h=0), dict(out_w=65537), dict(out_h=65537),
           dict(y=_yuv(), dtype=0, out_w=15), dict(y=_yuv(), dtype=0, out_h=11), dict(d=_display(), dtype=1), dict(d=_display(lut=0), dtype=0),
           dict(d=_display(lut=0x300008), dtype=0),
           dict(nmaps=0), dict(maps=[ID] * 3), dict(maps=[ID] * 2, nmaps=3),
           dict(out=0), dict(out=0x200002), dict(out_bytes=2 * 3 * 12 * 16 * 4 - 1)]
    for kw in bad:
        rc, msg = call(**kw)
        assert rc < 0 and msg.startswith(SYM + ": "), (kw, rc, msg)
    # the maps: each bound of the linear part, each corner, each side; the message names the frame of the first bad map
    lin = [_m(ayy=65536 + 16385), _m(ayy=65536 - 16385), _m(axx=65536 + 16385), _m(axx=65536 - 16385), _m(ayx=16385), _m(ayx=-16385),
           _m(axy=16385), _m(axy=-16385), _m(ayy=-65536)]
    corner = [_m(ty=-1), _m(tx=-1), _m(ty=256 * 12 + 1), _m(tx=256 * 24 + 1),
              _m(ayx=-16384, ty=0),                    # (0, Wo - 1) rises above the frame
              _m(axy=-16384, tx=0),                    # (Ho - 1, 0) leaves on the left
              _m(ayx=16384, ty=256 * 12 - 959),        # (Ho - 1, Wo - 1) sinks below it: 15 * 64 = 960
              _m(ayy=81920, ty=256 * 9 + 65)]          # 11 * 320 = 3520 > 256 * 23 - (256 * 9 + 65)
    for m in lin + corner:
        assert not W.map_ok(m, (12, 16), 24, 40), m  # (the statement's rule: no good map ever reaches the dummy context)
        for frame in (0, 1):
            maps = [ID, ID]
            maps[frame] = m
            rc, msg = call(maps=maps)
            assert rc < 0 and msg.startswith(SYM + ": ") and ("frame %d" % frame) in msg, (m, frame, msg)
        rc, msg = call(maps=[m])
        assert rc < 0 and "frame 0" in msg, (m, msg)
        rc, msg = call(maps=[m, m])
        assert rc < 0 and "frame 0" in msg and "frame 1" not in msg, (m, msg)
    # the neighbours of every bound above are decided by the same code; an empty batch is a no-op whatever else is wrong with it
    rc, msg = call(n=0, maps=[_m(ty=-1)], out=0, inp=0)
    assert rc == 0
    # the siblings keep rejecting algo 5
    lib = M.load()
    p = M.RgbParams()
    p.algo, p.dtype, p.white = 5, 1, 4095.0
    col = (M.RgbColor * 1)()
    assert lib.mcraw_demosaic_batch(C.addressof(call.ctx), C.byref(p), col, 1, C.c_void_p(0x100000), 40, 960, 40, 24, 1,
                                    C.c_void_p(0x200000), 1 << 24, None) < 0
    assert "unknown algo" in lib.mcraw_last_error().decode()


# ---- the statement

def _reflect(i, n):
    i = -i if i < 0 else i
    return 2 * (n - 1) - i if i > n - 1 else i


def _scalar_table(p, filt):
    if filt == "linear":
        return [0, 16 * (256 - p), 16 * p, 0]
    f, d = [], []
    for j in (-1, 0, 1, 2):
        a = 4 * abs(256 * j - p)
        d.append(abs(256 * j - p))
        f.append(3 * a ** 3 - 5 * 1024 * a ** 2 + 2 * 1024 ** 3 if a <= 1024 else
                 -a ** 3 + 5 * 1024 * a ** 2 - 8 * 1024 ** 2 * a + 4 * 1024 ** 3 if a < 2048 else 0)
    F = sum(f)
    w = [(4096 * v + F // 2) // F for v in f]
    res = 4096 - sum(w)
    near = [j for j in range(4) if d[j] == min(d)]
    if len(near) == 1:
        w[near[0]] += res
    else:
        w[near[0]] += res - res // 2
        w[near[1]] += res // 2
    return w


def _scalar(img, m, size, filt, black, cfa):
    """The header's statement, one output pixel at a time, in Python integers."""
    H, Wd = img.shape
    e = R.mhc_estimates(img, black, cfa)
    ayy, ayx, ty, axy, axx, tx = m
    out = np.zeros((3,) + size, dtype=np.int64)
    for i in range(size[0]):
        for k in range(size[1]):
            Y = ty + ((ayy * i + ayx * k + 128) >> 8)
            X = tx + ((axy * i + axx * k + 128) >> 8)
            wy, wx = _scalar_table(Y & 255, filt), _scalar_table(X & 255, filt)
            for c in range(3):
                t = [(sum(wx[j] * int(e[c, _reflect((Y >> 8) - 1 + r, H), _reflect((X >> 8) - 1 + j, Wd)]) for j in range(4)) + 2048) >> 12
                     for r in range(4)]
                out[c, i, k] = (sum(wy[r] * t[r] for r in range(4)) + 2048) >> 12
    return out


MAPS_16x24 = (  # onto (9, 13) of a 16 x 24 frame
    _m(ty=256 * 3 + 77, tx=256 * 5 + 201), _m(ayy=81920, axx=49152, ty=0, tx=256 * 10), _m(ayx=16384, axy=-16384, ty=0, tx=256 * 3),
    _m(ayy=60000, ayx=-9000, ty=256 * 5, axy=12000, axx=70000, tx=13), _m(ty=256 * 7, tx=256 * 11), _m(ty=0, tx=0))


@pytest.mark.parametrize("filt", FILTERS)
def test_numpy_statement_equals_the_scalar_one(filt):
    rng = np.random.default_rng(11)
    img = rng.integers(0, 4096, size=(16, 24)).astype(np.uint16)
    black = (60, 64, 61, 70)
    for m in MAPS_16x24:
        for cfa in ("rggb", "gbrg"):
            assert np.array_equal(W.warp_estimates(img, m, (9, 13), filt, black, cfa), _scalar(img, m, (9, 13), filt, black, cfa)), (m, cfa)


def test_table_properties():
    lin, cub = W.table("linear"), W.table("cubic")
    for p in range(256):
        assert list(cub[p]) == _scalar_table(p, "cubic") and list(lin[p]) == _scalar_table(p, "linear")
    d = np.abs(256 * np.arange(-1, 3)[None, :] - np.arange(256)[:, None])
    assert (S.kernel_f(4 * d, "cubic").sum(axis=1) == 2 * 1024 ** 3).all()  # F is the same for every phase
    for T in (lin, cub):
        assert (T.sum(axis=1) == 4096).all()
        assert np.array_equal(T[1:], T[:0:-1, ::-1])  # w(p) mirrors w(256 - p)
        assert list(T[0]) == [0, 4096, 0, 0]
    assert np.abs(cub).sum(axis=1).max() <= 5120 and np.abs(lin).sum(axis=1).max() == 4096
    assert cub.min() == -303 and cub.max() <= 4096 and lin.min() == 0
    assert list(cub[128]) == [-256, 2304, 2304, -256] and list(lin[128]) == [0, 2048, 2048, 0]


def test_whole_sample_translations_equal_mhc_cut():
    rng = np.random.default_rng(12)
    img = rng.integers(0, 4096, size=(16, 24)).astype(np.uint16)
    black = (60, 61, 62, 63)
    for cfa in CFAS:
        e = R.mhc_estimates(img, black, cfa)
        for (a, b), size in (((0, 0), (16, 24)), ((3, 5), (10, 16)), ((6, 0), (10, 8)), ((1, 7), (15, 17))):
            m = _m(ty=256 * a, tx=256 * b)
            for filt in FILTERS:
                assert np.array_equal(W.warp_estimates(img, m, size, filt, black, cfa), e[:, a:a + size[0], b:b + size[1]]), (cfa, a, b, filt)
                want = R.ref_bits(img, "mhc", "f32", 4095.0, black=black, cfa=cfa, gain=(1.7, 1.0, 1.4))[:, a:a + size[0], b:b + size[1]]
                assert np.array_equal(W.warp_ref(img, m, size, "f32", 4095.0, filt, black, cfa, (1.7, 1.0, 1.4)), want)


def test_flat_frames_stay_flat_and_greys_neutral():
    img = np.full((16, 24), 1234, dtype=np.uint16)
    grey = np.zeros((16, 24), dtype=np.uint16)
    for p, b in enumerate((60, 70, 80, 90)):
        grey[p >> 1::2, p & 1::2] = 1000 + b
    for filt in FILTERS:
        for m in MAPS_16x24:
            assert (W.warp_estimates(img, m, (9, 13), filt, (64, 64, 64, 64), "grbg") == 16 * (1234 - 64)).all(), (filt, m)
            assert (W.warp_estimates(grey, m, (9, 13), filt, (60, 70, 80, 90), "bggr") == 16000).all(), (filt, m)


def test_int32_formulation_is_exact_at_the_extremes():
    """The kernel's sums: v = 256 vh + vl, A = sum w vh and B = sum w vl in int32, (A + ((B + 2048) >> 8)) >> 4.  At samples
    alternating 0 / 65535 under blacks 65535 / 0 -- the largest |e| the format allows -- they equal the int64 sums (warp_from_e
    asserts that no accumulator leaves int32), and the bounds that follow from the table's sum |w| hold."""
    sw = int(np.abs(W.table("cubic")).sum(axis=1).max())
    yy, xx = np.mgrid[0:20, 0:28]
    worst = 0
    maps = (_m(ty=256 * 2 + 128, tx=256 * 3 + 128), _m(ayy=81920, ayx=-16384, ty=256 * 4, axy=16384, axx=49152, tx=1),
            _m(ayy=49152, ayx=16384, ty=0, axy=-16384, axx=81920, tx=256 * 4 + 37), _m(ty=77, tx=256 * 11 + 255))
    for phase, black in ((0, (65535, 0, 0, 65535)), (1, (0, 65535, 65535, 0)), (0, (0, 65535, 0, 65535)), (1, (65535, 65535, 0, 0))):
        img = (((yy + xx + phase) & 1) * 65535).astype(np.uint16)
        for cfa in ("rggb", "grbg"):
            e = R.mhc_estimates(img, black, cfa)
            worst = max(worst, int(np.abs(e).max()))
            for m in maps:
                for filt in FILTERS:
                    assert np.array_equal(W.warp_from_e(e, m, (12, 16), filt), W.warp_from_e(e, m, (12, 16), filt, split=True)), (m, filt)
    assert worst <= 40 * 65535 < 1 << 22
    emax = 40 * 65535
    tmax = (sw * emax + 2048) >> 12
    Emax = (sw * tmax + 2048) >> 12
    assert tmax < 1 << 23 and Emax < 1 << 24
    assert sw * ((tmax >> 8) + 1) < 1 << 31 and sw * 255 + 2048 < 1 << 31  # A and B of both passes fit int32
    assert sw < 1 << 13 and (tmax >> 8) + 1 < 1 << 23  # ... and their factors fit 24-bit multiplies
    assert sw * emax >= 1 << 31  # (a plain int32 sum would not: the reason for the split)


def _k(x, filt):
    x = np.abs(x)
    if filt == "linear":
        return np.maximum(0.0, 1.0 - x)
    return np.where(x <= 1, 1.5 * x ** 3 - 2.5 * x ** 2 + 1, np.where(x < 2, -0.5 * x ** 3 + 2.5 * x ** 2 - 4 * x + 2, 0.0))


def _dk(x, filt):
    """The kernel's derivative."""
    s, x = np.sign(x), np.abs(x)
    if filt == "linear":
        return np.where(x < 1, -s, 0.0)
    return s * np.where(x <= 1, 4.5 * x ** 2 - 5 * x, np.where(x < 2, -1.5 * x ** 2 + 5 * x - 4, 0.0))


@pytest.mark.parametrize("filt", FILTERS)
def test_close_to_a_float64_warp_with_the_unquantised_kernel(filt):
    """E against Ef, the float64 kernel at the unquantised positions y* = ty / 256 + (ayy i + ayx k) / 65536 (x* likewise), in 1/16
    DN.  Three terms, as for the resample, none of them chosen:
      the table     dw R S + dw R S: dw the largest sum_j |w / 4096 - kernel| of a phase, R half the range of e (the weights add
                    up to 1 in both tables), S the largest sum |w| / 4096, which carries the horizontal pass's error through the
                    vertical one;
      the roundings S / 2 + 1 / 2;
      the position  Y rounds 256 y* to the nearest integer: at most 1/512 sample off along each axis.  The interpolant's slope
                    along x is sum_j c_j(p) (e[j + 1] - e[j]) with c_j(p) = -sum_{m <= j} k'(p - m) (summation by parts, sum k' = 0),
                    so at most D1 gx, D1 = max_p sum_j |c_j(p)| and gx the largest |e(y, x + 1) - e(y, x)| of the padded frame; the
                    other axis's taps weigh it by at most Sf = max_p sum |kernel|: (D1 Sf gx + D1 Sf gy) / 512."""
    rng = np.random.default_rng(13)
    yy, xx = np.mgrid[0:40, 0:56]
    img = (1000 + 2 * xx + 3 * yy + rng.integers(-20, 21, size=(40, 56))).astype(np.uint16)
    black = (64, 64, 64, 64)
    e = R.mhc_estimates(img, black, "rggb")
    P = np.pad(e, ((0, 0), (W.REACH,) * 2, (W.REACH,) * 2), mode="reflect").astype(np.float64)
    Rh = (e.max() - e.min()) / 2.0
    gy, gx = np.abs(np.diff(P, axis=1)).max(), np.abs(np.diff(P, axis=2)).max()
    taps = np.arange(-1, 3, dtype=np.float64)
    ph = np.arange(256)[:, None] / 256.0
    T = W.table(filt) / 4096.0
    dw = np.abs(T - _k(ph - taps[None, :], filt)).sum(axis=1).max()
    Si = np.abs(T).sum(axis=1).max()
    fine = np.linspace(0.0, 1.0, 4097)[:, None]
    Sf = np.abs(_k(fine - taps[None, :], filt)).sum(axis=1).max()
    D1 = np.abs(-np.cumsum(_dk(fine - taps[None, :], filt), axis=1)[:, :3]).sum(axis=1).max()
    assert dw < 0.01 and 1.0 <= D1 <= 1.5 and 1.0 <= Sf <= 1.25 + 1e-12
    size = (21, 27)
    for m in (_m(ty=256 * 3 + 77, tx=256 * 5 + 201), _m(ayy=66000, ayx=-1700, ty=256 * 8, axy=1700, axx=66000, tx=256 * 3 + 9),
              _m(ayy=81920, ayx=16384, ty=0, axy=-16384, axx=81920, tx=256 * 6), _m(ayy=49152, ayx=-16384, ty=256 * 9, axy=16384, axx=49152, tx=31)):
        i = np.arange(size[0], dtype=np.float64)[:, None]
        k = np.arange(size[1], dtype=np.float64)[None, :]
        ys = m[2] / 256.0 + (m[0] * i + m[1] * k) / 65536.0
        xs = m[5] / 256.0 + (m[3] * i + m[4] * k) / 65536.0
        Y, X = W.positions(m, size)
        assert np.abs(Y / 256.0 - ys).max() <= 1 / 512 + 1e-12 and np.abs(X / 256.0 - xs).max() <= 1 / 512 + 1e-12
        # the float warp's taps sit about the integer statement's whole parts (the kernel is 0 beyond them, or reaches one sample
        # further where the rounding crossed a sample: five taps cover both)
        iy, ix = Y >> 8, X >> 8
        Ef = np.zeros((3,) + size)
        for r in range(-2, 4):
            for j in range(-2, 4):
                wgt = _k(ys - (iy + r), filt) * _k(xs - (ix + j), filt)
                rr = np.clip(iy + r + W.REACH, 0, P.shape[1] - 1)
                cc = np.clip(ix + j + W.REACH, 0, P.shape[2] - 1)
                assert (wgt[(iy + r + W.REACH != rr) | (ix + j + W.REACH != cc)] == 0).all()
                Ef += wgt[None] * P[:, rr, cc]
        E = W.warp_estimates(img, m, size, filt, black, "rggb")
        tol = 2 * dw * Rh * Si + 0.5 * Si + 0.5 + (D1 * Sf * gx + D1 * Sf * gy) / 512.0
        err = np.abs(E - Ef).max()
        print("%s %r: max |E - E_float| %.2f, tolerance %.2f (dw %.5f R %.0f D1 %.3f gx %.0f gy %.0f)" % (filt, m, err, tol, dw, Rh, D1, gx, gy))
        assert err <= tol, (m, err, tol)
