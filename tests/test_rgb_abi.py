"""Demosaic to linear RGB (mcraw_demosaic_batch) without a GPU: the ABI's symbol, macros and structs, properties of the
numpy reference of the arithmetic (_rgb_ref), and rgb_color."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _rgb_ref as R
import motioncam_decoder_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFAS = ("rggb", "bggr", "grbg", "gbrg")


def test_demosaic_symbol_macros_exported_and_listed():
    hdr = open(os.path.join(ROOT, "include", "mcraw_hip.h")).read()
    assert re.search(r"\bmcraw_demosaic_batch\s*\(", hdr)
    assert "mcraw_demosaic_batch" in M.ABI_SYMBOLS
    assert hasattr(M.load(), "mcraw_demosaic_batch")
    for macro, v in (("MCRAW_RGB_MHC", 1), ("MCRAW_RGB_BIN2", 2), ("MCRAW_CFA_RGGB", 0), ("MCRAW_CFA_BGGR", 1),
                     ("MCRAW_CFA_GRBG", 2), ("MCRAW_CFA_GBRG", 3), ("MCRAW_KRGB_MHC", 9), ("MCRAW_KRGB_BIN2", 10),
                     ("MCRAW_K_COUNT", 11)):
        assert re.search(r"#define %s\s+%du?\b" % (macro, v), hdr), macro
    assert M.RGB_KERNELS == {"krgb_mhc": 9, "krgb_bin2": 10}
    for cfa, code in R.CFA_CODE.items():
        assert re.search(r"#define MCRAW_CFA_%s\s+%d\b" % (cfa.upper(), code), hdr)


def test_code_object_has_rgb_kernels():
    raw = open(M.lib_path(), "rb").read()
    for k in (b"krgb_mhc", b"krgb_bin2"):
        assert k in raw, k


def test_struct_layouts():
    assert C.sizeof(M.RgbParams) == 28 and C.sizeof(M.RgbColor) == 48
    assert M.RgbParams.cfa.offset == 12 and M.RgbParams.black.offset == 16 and M.RgbParams.white.offset == 24
    assert M.RgbColor.gain.offset == 0 and M.RgbColor.m.offset == 12


@pytest.mark.parametrize("cfa", CFAS)
@pytest.mark.parametrize("algo", ("mhc", "bin2"))
def test_flat_mosaic_gives_equal_estimates(algo, cfa):
    # every filter sums to 16 (MHC) or 2 (BIN2): a flat mosaic above black gives the same E in every channel, borders included
    black = (60, 64, 66, 70)
    img = np.empty((10, 12), np.uint16)
    for p in range(4):
        img[(p >> 1)::2, (p & 1)::2] = 1000 + black[p]
    E = R.estimates(img, algo, black, cfa)
    scale = 16 if algo == "mhc" else 2
    assert (E == 1000 * scale).all()


def _mosaic_of(rgb, cfa):
    """Sample an RGB image (3, h, w) on the CFA."""
    h, w = rgb.shape[1:]
    s = R.SHIFT[cfa]
    role = ((np.arange(h)[:, None] & 1) * 2 + (np.arange(w)[None, :] & 1)) ^ s
    chan = np.choose(role, [0, 1, 1, 2])
    return np.take_along_axis(rgb, chan[None], 0)[0]


@pytest.mark.parametrize("cfa", CFAS)
def test_mhc_exact_on_linear_gradients(cfa):
    # on a linear ramp every MHC filter is exact: E = 16 x the true value away from the border (a wrong coefficient breaks it)
    h, w = 16, 20
    y, x = np.mgrid[0:h, 0:w]
    rgb = np.stack([500 + 13 * x + 7 * y, 800 + 5 * x + 11 * y, 300 + 17 * x + 3 * y]).astype(np.int64)
    E = R.mhc_estimates(_mosaic_of(rgb, cfa).astype(np.uint16), (0, 0, 0, 0), cfa)
    assert np.array_equal(E[:, 2:-2, 2:-2], 16 * rgb[:, 2:-2, 2:-2])


def test_mirror_in_x_and_y():
    rng = np.random.default_rng(3)
    img = rng.integers(0, 4096, size=(12, 14), dtype=np.uint16)
    E = R.mhc_estimates(img, (0, 0, 0, 0), "rggb")
    # mirrored in x, an even width moves column 0 (R) to an odd column: the CFA becomes grbg
    Ex = R.mhc_estimates(img[:, ::-1], (0, 0, 0, 0), "grbg")
    assert np.array_equal(Ex, E[:, :, ::-1])
    Ey = R.mhc_estimates(img[::-1, :], (0, 0, 0, 0), "gbrg")
    assert np.array_equal(Ey, E[:, ::-1, :])


@pytest.mark.parametrize("cfa", CFAS)
def test_bin2_of_a_quad(cfa):
    black = (10, 20, 30, 40)
    img = np.array([[110, 220], [330, 440]], np.uint16)
    d = [100, 200, 300, 400]
    s = R.SHIFT[cfa]
    o = R.rgb_values(img, "bin2", 1000.0, black, cfa)
    inv = np.float32(1.0) / (np.float32(1000.0) - np.float32(25.0))
    want = [d[0 ^ s], (d[1 ^ s] + d[2 ^ s]) / 2, d[3 ^ s]]
    assert np.allclose(o[:, 0, 0], np.array(want, np.float32) * inv, rtol=1e-6, atol=0)
    assert R.bin2_estimates(img, black, cfa)[:, 0, 0].tolist() == [2 * d[0 ^ s], d[1 ^ s] + d[2 ^ s], 2 * d[3 ^ s]]


def test_reference_float_stage_order():
    # o = (m0 v0 + m1 v1) + m2 v2 in f32, products rounded, with k = (gain * inv) * 1/16
    img = np.full((4, 4), 1000, np.uint16)
    m = np.array([[0.1, 0.2, 0.3], [1.0, 0.0, 0.0], [-0.5, 1.5, 0.25]], np.float32)
    g = np.array([2.0, 1.0, 1.5], np.float32)
    o = R.rgb_values(img, "mhc", 4095.0, (0, 0, 0, 0), "rggb", g, m)
    inv = np.float32(1.0) / np.float32(4095.0)
    v = [np.float32(16000) * ((g[c] * inv) * np.float32(0.0625)) for c in range(3)]
    for i in range(3):
        assert o[i, 1, 1] == (m[i, 0] * v[0] + m[i, 1] * v[1]) + m[i, 2] * v[2]


def test_rgb_color_camera_is_identity():
    g, m = M.rgb_color({}, {"asShotNeutral": [0.5, 1.0, 0.8]}, space="camera")
    assert g.dtype == np.float32 and m.dtype == np.float32
    assert np.array_equal(m, np.eye(3, dtype=np.float32))
    assert np.array_equal(g, np.array([2.0, 1.0, 1.25], np.float32))
    g, m = M.rgb_color({}, None, space="camera")
    assert np.array_equal(g, np.ones(3, np.float32))


def test_rgb_color_neutral_maps_to_grey():
    # a forward matrix whose rows sum to the D50 white: a camera-neutral sample (after white balance) is grey in sRGB
    d50 = np.array([0.96422, 1.0, 0.82521])
    fm = np.array([[0.6, 0.25, 0.0], [0.2, 0.75, 0.05], [0.0, 0.05, 0.0]])
    fm[:, 2] = d50 - fm[:, :2].sum(1)
    neutral = np.array([0.45, 1.0, 0.7])
    g, m = M.rgb_color({"forwardMatrix1": fm.ravel().tolist()}, {"asShotNeutral": neutral.tolist()}, space="srgb")
    o = m.astype(np.float64) @ (g.astype(np.float64) * neutral)
    assert np.abs(o - o.mean()).max() < 1e-6 and abs(o.mean() - 1.0) < 1e-6
    _, mx = M.rgb_color({"forwardMatrix1": fm.ravel().tolist()}, None, space="xyz")
    assert np.array_equal(mx, fm.astype(np.float32))


def test_rgb_color_missing_keys_raise():
    with pytest.raises(ValueError):
        M.rgb_color({}, None, space="srgb")
    with pytest.raises(ValueError):
        M.rgb_color({"forwardMatrix1": [0] * 9}, None, space="xyz")
    with pytest.raises(ValueError):
        M.rgb_color({"forwardMatrix1": [1, 0, 0, 0, 1, 0, 0, 0, 1]}, None, space="lab")
