"""Display-ready RGB (mcraw_demosaic_display_batch) without a GPU: the ABI's symbol, macros and struct, transfer_lut, and
properties of the numpy reference of the stage (_display_ref)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _display_ref as D
import _rgb_ref as R
import motioncam_decoder_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_display_symbol_macros_exported_and_listed():
    hdr = open(os.path.join(ROOT, "include", "mcraw_hip.h")).read()
    assert re.search(r"\bmcraw_demosaic_display_batch\s*\(", hdr)
    assert "mcraw_demosaic_display_batch" in M.ABI_SYMBOLS
    assert hasattr(M.load(), "mcraw_demosaic_display_batch")
    for macro, v in (("MCRAW_DISP_U8", 1), ("MCRAW_DISP_U16", 2), ("MCRAW_DISP_CHW", 0), ("MCRAW_DISP_HWC", 1),
                     ("MCRAW_K_COUNT", 11)):
        assert re.search(r"#define %s\s+%du?\b" % (macro, v), hdr), macro
    assert (M.DISP_U8, M.DISP_U16, M.DISP_CHW, M.DISP_HWC) == (1, 2, 0, 1)
    assert M.RGB_KERNELS == {"krgb_mhc": 9, "krgb_bin2": 10}


def test_display_struct_layout():
    assert C.sizeof(M.Display) == 24
    assert [getattr(M.Display, f).offset for f in ("dtype", "layout", "lut_log2", "reserved", "lut")] == [0, 4, 8, 12, 16]


@pytest.mark.parametrize("curve", ("linear", "srgb", "bt709", 2.2, 1.0, lambda x: x * x))
@pytest.mark.parametrize("bits", (8, 10, 12, 16))
@pytest.mark.parametrize("size", (256, 4096, 65536))
def test_transfer_lut_endpoints_monotonic_range(curve, bits, size):
    lut = M.transfer_lut(curve, size, bits)
    assert lut.dtype == np.uint16 and lut.shape == (size,)
    top = (1 << bits) - 1
    assert lut[0] == 0 and lut[-1] == top
    assert (np.diff(lut.astype(np.int64)) >= 0).all()
    assert int(lut.max()) <= top


def test_transfer_lut_curves():
    size = 65536
    x = np.arange(size) / (size - 1)
    lin = M.transfer_lut("linear", size, 16)
    assert np.array_equal(lin, np.arange(size, dtype=np.uint16))
    s = M.transfer_lut("srgb", size, 16).astype(np.float64) / 65535
    lo, hi = x <= 0.0031308, x > 0.0031308
    assert np.abs(s[lo] - 12.92 * x[lo]).max() <= 0.5 / 65535 + 1e-12
    assert np.abs(s[hi] - (1.055 * x[hi] ** (1 / 2.4) - 0.055)).max() <= 0.5 / 65535 + 1e-12
    b = M.transfer_lut("bt709", size, 16).astype(np.float64) / 65535
    lo, hi = x < 0.018, x >= 0.018
    assert np.abs(b[lo] - 4.5 * x[lo]).max() <= 0.5 / 65535 + 1e-12
    assert np.abs(b[hi] - (1.099 * x[hi] ** 0.45 - 0.099)).max() <= 0.5 / 65535 + 1e-12
    # the two pieces meet at the breakpoint: no step there beyond the slope of the linear piece (12.92 codes per entry)
    k = int(np.searchsorted(x, 0.0031308, side="right"))
    s16 = M.transfer_lut("srgb", size, 16).astype(np.int64)
    assert s16[k] - s16[k - 1] <= 14 and s16[k - 1] - s16[k - 2] <= 14
    g = M.transfer_lut(2.2, 4096, 8)
    assert np.array_equal(g, np.rint((np.arange(4096) / 4095) ** (1 / 2.2) * 255).astype(np.uint16))
    assert np.array_equal(M.transfer_lut(lambda v: v, 256, 8), np.arange(256, dtype=np.uint16))
    assert M.transfer_lut("SRGB", 256, 8)[128] == M.transfer_lut("srgb", 256, 8)[128]


@pytest.mark.parametrize("kw", [dict(size=255), dict(size=128), dict(size=3000), dict(size=131072), dict(bits=9),
                                dict(bits=0), dict(bits=32), dict(curve="pq"), dict(curve=0.0), dict(curve=-2.0),
                                dict(curve=lambda v: v[:3]), dict(curve=lambda v: v * np.nan)])
def test_transfer_lut_rejects(kw):
    args = dict(curve="srgb", size=4096, bits=8)
    args.update(kw)
    with pytest.raises(ValueError):
        M.transfer_lut(**args)


def test_lut_index_rules():
    L = 4096
    o = np.array([np.nan, -np.inf, -1.0, -0.0, 0.0, 1e-30, 0.5 / 4095, 1.5 / 4095, 0.5, 1.0, 1.0000001, 7.0, np.inf],
                 np.float32)
    i = D.lut_index(o, L)
    assert i.dtype == np.uint32
    assert list(i[:6]) == [0, 0, 0, 0, 0, 0]
    # ties of the f32 product go to even: 0.5 -> 0, 1.5 -> 2 (when the product is exact)
    p = (np.float32(o[6]) * np.float32(L - 1))
    assert i[6] == np.rint(p)
    assert list(i[9:]) == [L - 1] * 4
    assert i[8] == np.rint(np.float32(0.5) * np.float32(L - 1))  # 2047.5 -> 2048
    assert i[8] == 2048


def test_reference_identity_lut_and_layouts():
    rng = np.random.default_rng(2)
    img = rng.integers(0, 4096, size=(12, 16), dtype=np.uint16)
    ident = np.arange(65536, dtype=np.uint16)
    o = R.rgb_values(img, "mhc", 4095.0, gain=(1.5, 1.0, 1.2))
    q = D.display_ref(img, "mhc", 4095.0, ident, "u16", "chw", gain=(1.5, 1.0, 1.2))
    assert np.array_equal(q, D.lut_index(o, 65536).astype(np.uint16))
    hwc = D.display_ref(img, "mhc", 4095.0, ident, "u16", "hwc", gain=(1.5, 1.0, 1.2))
    assert hwc.shape == (12, 16, 3) and np.array_equal(hwc, q.transpose(1, 2, 0))
    # uint8 keeps the low byte of each entry
    lut = (np.arange(4096, dtype=np.uint16) * 37) & 0xFFFF
    u8 = D.display_ref(img, "bin2", 4095.0, lut, "u8", "chw")
    o2 = R.rgb_values(img, "bin2", 4095.0)
    assert u8.dtype == np.uint8 and np.array_equal(u8, (lut[D.lut_index(o2, 4096)] & 0xFF).astype(np.uint8))


def test_reference_srgb_close_to_float64():
    rng = np.random.default_rng(4)
    o = rng.uniform(-0.1, 1.1, size=(3, 64, 64)).astype(np.float32)
    got = D.apply_lut(o, M.transfer_lut("srgb", 4096, 8), "u8").astype(np.float64)
    x = np.clip(o.astype(np.float64), 0, 1)
    want = np.where(x <= 0.0031308, 12.92 * x, 1.055 * x ** (1 / 2.4) - 0.055) * 255
    assert np.abs(got - want).max() <= 1.0 + 1e-9
