"""Y'CbCr 4:2:0 output (mcraw_demosaic_yuv_batch) without a GPU: the ABI's symbol, macros and struct, yuv_matrix, and
properties of the numpy reference of the stage (_yuv_ref)."""
import ctypes as C
import os
import re
import zlib

import numpy as np
import pytest

import _display_ref as D
import _rgb_ref as R
import _yuv_ref as Y
import motioncam_decoder_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}
COMBOS = [(s, r, b, i) for s in KR_KB for r in ("limited", "full") for b in (8, 10) for i in (8, 10, 12, 14, 16)]


def test_yuv_symbol_macros_exported_and_listed():
    hdr = open(os.path.join(ROOT, "include", "mcraw_hip.h")).read()
    assert re.search(r"\bmcraw_demosaic_yuv_batch\s*\(", hdr)
    assert "mcraw_demosaic_yuv_batch" in M.ABI_SYMBOLS
    assert hasattr(M.load(), "mcraw_demosaic_yuv_batch")
    for macro, v in (("MCRAW_YUV_NV12", 1), ("MCRAW_YUV_P010", 2), ("MCRAW_K_COUNT", 11)):
        assert re.search(r"#define %s\s+%du?\b" % (macro, v), hdr), macro
    assert (M.YUV_NV12, M.YUV_P010) == (1, 2)
    assert M.RGB_KERNELS == {"krgb_mhc": 9, "krgb_bin2": 10}


def test_yuv_struct_layout():
    assert C.sizeof(M.Yuv) == 72
    names = ("format", "lut_log2", "in_bits", "sh", "y_off", "c_off", "cy", "cb", "cr", "reserved", "lut")
    assert [getattr(M.Yuv, f).offset for f in names] == [0, 4, 8, 12, 16, 20, 24, 36, 48, 60, 64]
    hdr = open(os.path.join(ROOT, "include", "mcraw_hip.h")).read()
    assert "sizeof 72; y_off 16, c_off 20, cy 24, cb 36, cr 48, reserved 60, lut 64" in hdr


def _ranges(rng_name, bits):
    """(luma span, chroma span, y_off, c_off, code of white) of a range."""
    if rng_name == "limited":
        return 219 << (bits - 8), 224 << (bits - 8), 16 << (bits - 8), 128 << (bits - 8), 235 << (bits - 8)
    return (1 << bits) - 1, (1 << bits) - 1, 0, 1 << (bits - 1), (1 << bits) - 1


@pytest.mark.parametrize("standard,rng_name,bits,in_bits", COMBOS)
def test_yuv_matrix_exactness(standard, rng_name, bits, in_bits):
    cy, cb, cr, sh, y_off, c_off = M.yuv_matrix(standard, rng_name, bits, in_bits)
    assert all(isinstance(v, int) for v in cy + cb + cr + (sh, y_off, c_off))
    luma, chroma, yo, co, white = _ranges(rng_name, bits)
    top_in = (1 << in_bits) - 1
    assert (y_off, c_off) == (yo, co)
    assert sum(cb) == 0 and sum(cr) == 0
    assert sum(cy) == int(np.rint(luma * 2.0 ** sh / top_in))
    assert 1 <= sh <= 24 and Y.rule_ok((cy, cb, cr), sh, in_bits)
    # the largest sh the rule admits: the same real matrix one step finer breaks it
    assert not Y.rule_ok(([2 * c for c in cy], [2 * c for c in cb], [2 * c for c in cr]), sh + 1, in_bits) or sh == 24
    # the derived error bound of the coefficients needs 2^sh >= 4 * (2^in_bits - 1)
    assert (1 << sh) >= 4 * top_in
    # every grey level is exactly neutral; black and white land on the ends of the range
    g = np.repeat(np.arange(top_in + 1, dtype=np.int64), 2)  # one 2x2 block per level
    P = np.broadcast_to(g[None, None, :], (3, 2, g.size))
    Yc, Cb, Cr = Y.yuv_codes(P, cy, cb, cr, sh, y_off, c_off, bits)
    assert (Cb == c_off).all() and (Cr == c_off).all()
    assert Yc[0, 0] == y_off and Yc[0, -1] == white
    assert (np.diff(Yc[0]) >= 0).all()


@pytest.mark.parametrize("standard,rng_name,bits,in_bits", COMBOS)
def test_yuv_matrix_within_one_code_of_float64(standard, rng_name, bits, in_bits):
    """0.5 from the final rounding plus at most (0.5 + 0.5 + 1) * (2^in_bits - 1) / 2^sh <= 0.5 from the coefficients
    (two rounded entries and the corrected G entry)."""
    cy, cb, cr, sh, y_off, c_off = M.yuv_matrix(standard, rng_name, bits, in_bits)
    rng = np.random.default_rng(zlib.crc32(("%s%s%d%d" % (standard, rng_name, bits, in_bits)).encode()))
    n = 200000
    P = rng.integers(0, 1 << in_bits, size=(3, 2, 2 * n), dtype=np.int64)  # n 2x2 blocks, 4 n triples
    Yc, Cb, Cr = Y.yuv_codes(P, cy, cb, cr, sh, y_off, c_off, bits)
    kr, kb = KR_KB[standard]
    kg = 1.0 - kr - kb
    luma, chroma, _, _, _ = _ranges(rng_name, bits)
    x = P.astype(np.float64) / ((1 << in_bits) - 1)
    yf = kr * x[0] + kg * x[1] + kb * x[2]
    top = (1 << bits) - 1
    assert np.abs(Yc - np.clip(yf * luma + y_off, 0, top)).max() <= 1.0
    xb = (x[:, 0::2, 0::2] + x[:, 0::2, 1::2] + x[:, 1::2, 0::2] + x[:, 1::2, 1::2]) / 4.0
    yb = kr * xb[0] + kg * xb[1] + kb * xb[2]
    cbf = (xb[2] - yb) / (2.0 * (1.0 - kb)) * chroma + c_off
    crf = (xb[0] - yb) / (2.0 * (1.0 - kr)) * chroma + c_off
    assert np.abs(Cb - np.clip(cbf, 0, top)).max() <= 1.0
    assert np.abs(Cr - np.clip(crf, 0, top)).max() <= 1.0


@pytest.mark.parametrize("kw", [dict(standard="bt470"), dict(standard=None), dict(standard=709), dict(range="video"),
                                dict(range=None), dict(bits=12), dict(bits=9), dict(bits=True), dict(in_bits=7),
                                dict(in_bits=17), dict(in_bits=8.5), dict(in_bits="12")])
def test_yuv_matrix_rejects(kw):
    args = dict(standard="bt709", range="limited", bits=8, in_bits=8)
    args.update(kw)
    with pytest.raises(ValueError):
        M.yuv_matrix(**args)


def test_yuv_matrix_defaults_and_case():
    assert M.yuv_matrix() == M.yuv_matrix("bt709", "limited", 8, 8)
    assert M.yuv_matrix("BT601") == M.yuv_matrix("bt601")


def test_reference_layout_and_p010_shift():
    rng = np.random.default_rng(5)
    h, w = 6, 8
    Yc = rng.integers(0, 1024, size=(h, w))
    Cb = rng.integers(0, 1024, size=(h // 2, w // 2))
    Cr = rng.integers(0, 1024, size=(h // 2, w // 2))
    f = Y.pack(Yc, Cb, Cr, "p010")
    assert f.dtype == np.uint16 and f.shape == (9, 8)
    assert np.array_equal(f[:h], Yc << 6)
    assert np.array_equal(f[h:].reshape(h // 2, w // 2, 2)[..., 0], Cb << 6)
    assert np.array_equal(f[h:].reshape(h // 2, w // 2, 2)[..., 1], Cr << 6)
    assert (f & 63 == 0).all()
    f8 = Y.pack(Yc & 255, Cb & 255, Cr & 255, "nv12")
    assert f8.dtype == np.uint8 and f8.shape == (9, 8) and f8.tobytes()[:w] == (Yc[0] & 255).astype(np.uint8).tobytes()
    # the chroma bytes of a frame, as a raw video reader sees them: Cb0 Cr0 Cb1 Cr1 ...
    assert list(f8.ravel()[h * w: h * w + 4]) == [Cb[0, 0] & 255, Cr[0, 0] & 255, Cb[0, 1] & 255, Cr[0, 1] & 255]


def test_reference_identity_lut_by_hand():
    """BIN2 on a constant-quad mosaic, identity LUT of 256 entries, in_bits 8, coefficients small enough to do on paper."""
    img = np.zeros((4, 4), np.uint16)
    img[0::2, 0::2], img[0::2, 1::2], img[1::2, 0::2], img[1::2, 1::2] = 255, 102, 102, 51  # R, G, G, B
    img[2:, 2:] = 0  # the fourth output pixel is black
    lut = np.arange(256, dtype=np.uint16)
    o = R.rgb_values(img, "bin2", 255.0)
    assert np.array_equal(D.lut_index(o, 256), np.array([[[255, 255], [255, 0]], [[102, 102], [102, 0]], [[51, 51], [51, 0]]]))
    coef = ((1, 2, 1), (-1, -1, 2), (2, -1, -1), 2, 16, 128)  # sh = 2: Y = (R + 2 G + B + 2) >> 2, + 16
    f = Y.yuv_ref(img, "bin2", 255.0, lut, "nv12", coef, 8)
    assert f.shape == (3, 2)
    yy = ((255 + 204 + 51 + 2) >> 2) + 16  # 144
    assert f[:2].tolist() == [[yy, yy], [yy, 16]]
    # S = 3 x (255, 102, 51); Cb = ((-765 - 306 + 306 + 8) >> 4) + 128 = (-757 >> 4) + 128 = -48 + 128; floor, not truncation
    assert f[2].tolist() == [80, ((1530 - 306 - 153 + 8) >> 4) + 128]
    # in_bits masks the entry: with in_bits 8 a LUT holding 0x1234 counts as 0x34
    f2 = Y.yuv_from_o(np.ones((3, 2, 2), np.float32), np.full(256, 0x1234, np.uint16), "p010", coef, 8)
    assert f2[0, 0] == min(((4 * 0x34 + 2) >> 2) + 16, 1023) << 6 and f2[2].tolist() == [128 << 6, 128 << 6]


def test_reference_asserts_on_int32_wrap():
    big = ((1 << 22, 1 << 22, 1 << 22), (0, 0, 0), (0, 0, 0), 1, 0, 0)
    assert not Y.rule_ok(big[:3], 1, 16)
    with pytest.raises(AssertionError):
        Y.yuv_codes(np.full((3, 2, 2), 65535), *big, 8)


def test_yuv_planes_views():
    import torch
    t = torch.arange(2 * 6 * 4, dtype=torch.int32).reshape(2, 6, 4)
    yv, c = M.yuv_planes(t, 4)
    assert tuple(yv.shape) == (2, 4, 4) and tuple(c.shape) == (2, 2, 2, 2)
    assert yv.data_ptr() == t.data_ptr() and c.data_ptr() == t[0, 4:].data_ptr()
    assert c[1, 1, 0].tolist() == [t[1, 5, 0].item(), t[1, 5, 1].item()]
    y1, c1 = M.yuv_planes(t[0], 4)
    assert tuple(y1.shape) == (4, 4) and tuple(c1.shape) == (2, 2, 2)
    with pytest.raises(ValueError):
        M.yuv_planes(t, 6)
