"""The area downscale (mcraw_demosaic_area_batch) without a GPU: the ABI's symbols, macros and struct, the numpy statement of the
contract (_area_ref) against a scalar one written straight from the header, the properties the contract names (weights, identity
at one quad per pixel, flat frames, the int32 bounds, the distance from the exact area average), and fit_crop."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import _area_ref as A
import _rgb_ref as R
import motioncam_decoder_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFAS = ("rggb", "bggr", "grbg", "gbrg")


def _hdr():
    return open(os.path.join(ROOT, "include", "mcraw_hip.h")).read()


def test_area_symbols_exported_and_listed():
    hdr = _hdr()
    lib = M.load()
    for sym in ("mcraw_demosaic_area_batch", "mcraw_area_work_bytes"):
        assert re.search(r"\b%s\s*\(" % sym, hdr), sym
        assert sym in M.ABI_SYMBOLS and hasattr(lib, sym), sym
    assert re.search(r"#define MCRAW_RGB_AREA\s+3\b", hdr) and M.RGB_AREA == 3
    assert re.search(r"#define MCRAW_K_COUNT\s+11\b", hdr)
    for name in ("fit_crop", "Area", "RGB_AREA"):
        assert name in M.__all__
    block = hdr[hdr.index("any output size"):hdr.index("} mcraw_area;")]
    for line in ("c(k, q)    = clamp(floor((256 * (q * O - k * Q) + (Q >> 1)) / Q), 0, 256)", "w(k, q)    = c(k, q + 1) - c(k, q)",
                 "t_c(qy, k) = (h_c + 8) >> 4", "E_c(j, k)  = (v_c + 128) >> 8", "k[c] = (gain[c] * inv) * 0.03125f",
                 "1 <= out_w <= Qw <= 16 out_w", "out of scope"):
        assert line in block, line


def test_area_struct_layout():
    names = ("x0", "y0", "cw", "ch", "out_w", "out_h", "reserved")
    assert C.sizeof(M.Area) == 32
    assert [getattr(M.Area, f).offset for f in names] == [0, 4, 8, 12, 16, 20, 24]
    m = re.search(r"\}\s*mcraw_area;\s*/\*\s*sizeof (\d+); y0 (\d+), cw (\d+), ch (\d+), out_w (\d+), out_h (\d+), reserved (\d+)", _hdr())
    assert m and [int(v) for v in m.groups()] == [32, 4, 8, 12, 16, 20, 24]


def _area(cw, ch, ow, oh, x0=0, y0=0, reserved=(0, 0)):
    a = M.Area()
    a.x0, a.y0, a.cw, a.ch, a.out_w, a.out_h = x0, y0, cw, ch, ow, oh
    a.reserved[0], a.reserved[1] = reserved
    return a


def test_work_bytes():
    wb = M.load().mcraw_area_work_bytes
    assert wb(None) == 0
    # a table per axis: the first quad, the taps and 17 weights per output column and row
    assert wb(_area(4032, 2268, 1920, 1080)) >= (1920 + 1080) * (4 + 2 + 17 * 2)
    assert wb(_area(2, 2, 1, 1)) > 0 and wb(_area(64, 64, 2, 2)) > 0
    for bad in (_area(3, 2, 1, 1), _area(2, 2, 1, 1, x0=1), _area(2, 2, 1, 1, y0=1), _area(0, 2, 1, 1), _area(2, 0, 1, 1),
                _area(2, 2, 0, 1), _area(2, 2, 1, 0), _area(2, 2, 2, 1), _area(2, 2, 1, 2), _area(66, 64, 2, 2), _area(64, 66, 2, 2),
                _area(2, 2, 1, 1, reserved=(1, 0)), _area(2, 2, 1, 1, reserved=(0, 1))):
        assert wb(bad) == 0, [getattr(bad, f) for f in ("x0", "y0", "cw", "ch", "out_w", "out_h")]


def _scalar(img, crop, size, black, cfa):
    """The header's statement, one output pixel at a time, in Python integers."""
    y0, x0, h, w = crop
    ho, wo = size
    Qh, Qw = h // 2, w // 2
    s = R.SHIFT[cfa]

    def c(k, q, Q, O):
        return min(max((256 * (q * O - k * Q) + (Q >> 1)) // Q, 0), 256)

    def e(qy, qx):
        d = [int(img[y0 + 2 * qy + (p >> 1), x0 + 2 * qx + (p & 1)]) - int(black[p]) for p in range(4)]
        return (2 * d[0 ^ s], d[1 ^ s] + d[2 ^ s], 2 * d[3 ^ s])

    E = np.zeros((3, ho, wo), dtype=np.int64)
    for j in range(ho):
        for k in range(wo):
            v = [0, 0, 0]
            for qy in range(j * Qh // ho, Qh):
                wy = c(j, qy + 1, Qh, ho) - c(j, qy, Qh, ho)
                if wy == 0:
                    break
                hsum = [0, 0, 0]
                for qx in range(k * Qw // wo, Qw):
                    wx = c(k, qx + 1, Qw, wo) - c(k, qx, Qw, wo)
                    if wx == 0:
                        break
                    for ch, ev in enumerate(e(qy, qx)):
                        hsum[ch] += wx * ev
                for ch in range(3):
                    v[ch] += wy * ((hsum[ch] + 8) >> 4)
            for ch in range(3):
                E[ch, j, k] = (v[ch] + 128) >> 8
    return E


def test_numpy_statement_equals_scalar_restatement():
    rng = np.random.default_rng(1)
    for (h, w), crop, size, cfa in (((12, 20), (0, 0, 12, 20), (3, 4), "rggb"), ((12, 20), (2, 4, 10, 14), (2, 3), "bggr"),
                                    ((36, 52), (2, 6, 30, 42), (6, 10), "grbg"), ((40, 70), (0, 0, 34, 66), (1, 3), "gbrg"),
                                    ((8, 8), (0, 0, 8, 8), (4, 4), "grbg")):
        img = rng.integers(0, 1 << 16, size=(h, w), dtype=np.uint16)
        black = tuple(int(b) for b in rng.integers(0, 1 << 16, size=4))
        assert np.array_equal(A.area_estimates(img, crop, size, black, cfa), _scalar(img, crop, size, black, cfa)), (crop, size)


def _legal_sizes(Q):
    lo, hi = -(-Q // 16), Q
    return sorted({lo, hi, min(hi, lo + 1), max(lo, hi - 1), (lo + hi) // 2, max(lo, min(hi, Q * 10 // 21)), max(lo, min(hi, Q // 3))})


@pytest.mark.parametrize("Q", (1, 2, 3, 47, 63, 1920, 2016, 32768))
def test_weights_sum_sign_and_taps(Q):
    for O in _legal_sizes(Q):
        q0, w = A.weights(Q, O)  # (asserts that there is no 18th tap)
        assert (w.sum(axis=1) == 256).all() and (w >= 0).all(), (Q, O)
        last = np.where(w > 0, np.arange(A.TAPS)[None, :], -1).max(axis=1)
        assert (q0 + last < Q).all(), (Q, O)  # no tap behind the crop
        assert (last + 1 <= (Q // O if Q % O == 0 else Q // O + 2)).all(), (Q, O)  # the plan's bound on the taps
        # the overlap of the footprint with each quad, rounded cumulatively: each cumulative sum is within 1/2 of the exact one
        for k in (0, O // 2, O - 1):
            for t in range(A.TAPS + 1):
                exact = min(max(Fraction(256 * ((int(q0[k]) + t) * O - k * Q), Q), 0), 256)
                assert abs(int(w[k, :t].sum()) - exact) <= Fraction(1, 2), (Q, O, k, t)


@pytest.mark.parametrize("cfa", CFAS)
def test_one_quad_per_pixel_is_bin2_times_16(cfa):
    rng = np.random.default_rng(2)
    img = rng.integers(0, 1 << 16, size=(16, 24), dtype=np.uint16)
    black = (3, 65535, 100, 0)
    for crop in ((0, 0, 16, 24), (2, 4, 12, 18)):
        y0, x0, h, w = crop
        want = R.bin2_estimates(img[y0:y0 + h, x0:x0 + w], black, cfa) * 16
        assert np.array_equal(A.area_estimates(img, crop, (h // 2, w // 2), black, cfa), want)


def test_flat_frames_stay_flat_at_every_legal_size():
    black = (60, 64, 68, 72)
    img = np.zeros((12, 20), dtype=np.uint16)
    for p in range(4):
        img[(p >> 1)::2, (p & 1)::2] = black[p] + 1000  # d = 1000 at every position
    for ho in range(1, 7):
        for wo in range(1, 11):
            assert (A.area_estimates(img, (0, 0, 12, 20), (ho, wo), black) == 32 * 1000).all(), (ho, wo)


def test_int32_bounds_at_the_extremes():
    for fill, black in ((65535, (0, 0, 0, 0)), (0, (65535,) * 4)):
        img = np.full((94, 126), fill, dtype=np.uint16)
        for size in ((3, 4), (47, 63), (6, 8), (13, 10)):
            E = A.area_estimates(img, (0, 0, 94, 126), size, black)  # (area_from_e asserts the bounds of h, v and E)
            assert (E == (32 * 65535 if fill else -32 * 65535)).all()  # flat: E = 32 d


def _exact_average(e, size):
    """The float64 area average of the binned image e (Qh, Qw) over every output pixel's footprint."""
    def overlap(Q, O):
        m = np.zeros((O, Q))
        for k in range(O):
            lo, hi = k * Q / O, (k + 1) * Q / O
            for q in range(int(lo), min(Q, int(np.ceil(hi)))):
                m[k, q] = max(0.0, min(hi, q + 1) - max(lo, q)) * O / Q
        return m
    return overlap(e.shape[0], size[0]) @ e.astype(np.float64) @ overlap(e.shape[1], size[1]).T


def test_close_to_the_exact_area_average():
    """|E / 32 - exact| <= (taps_x + taps_y) / 256 * (max - min of e) / 2 + 3/32 DN: each cumulative rounding is off by at most
    1/512 of the footprint."""
    rng = np.random.default_rng(5)
    worst = 0.0
    for (h, w), size in (((36, 52), (6, 10)), ((94, 126), (3, 4)), ((64, 64), (2, 2)), ((48, 80), (24, 40)), ((50, 84), (12, 20)),
                         ((50, 84), (5, 9))):
        img = rng.integers(0, 1 << 12, size=(h, w), dtype=np.uint16)
        e = R.bin2_estimates(img, (0, 0, 0, 0), "rggb")
        E = A.area_from_e(e, size)
        tx = int((A.weights(w // 2, size[1])[1] > 0).sum(axis=1).max())
        ty = int((A.weights(h // 2, size[0])[1] > 0).sum(axis=1).max())
        for c in range(3):
            bound = (tx + ty) / 256.0 * (float(e[c].max()) - float(e[c].min())) / 2.0 / 2.0 + 3.0 / 32.0  # (e is in half DN)
            err = np.abs(E[c] / 32.0 - _exact_average(e[c], size) / 2.0).max()
            worst = max(worst, err / bound)
            assert err <= bound, (h, w, size, c, err, bound)
    assert worst > 0.0


def test_fit_crop():
    assert M.fit_crop(3024, 4032, 1080, 1920) == (378, 0, 2268, 4032)
    assert M.fit_crop(2160, 3840, 1080, 1920) == (0, 0, 2160, 3840)
    assert M.fit_crop(3000, 4000, 720, 1280) == (374, 0, 2250, 4000) == A.fit_crop(3000, 4000, 720, 1280)
    assert M.fit_crop(4032, 3024, 540, 960) == (1166, 0, 1700, 3024)  # a portrait frame: the width binds
    assert M.fit_crop(1000, 4000, 500, 500) == (0, 1500, 1000, 1000)                    # the height binds
    for (h, w, ho, wo) in ((3024, 4032, 1080, 1920), (2160, 3840, 270, 480), (1234, 5678, 100, 300), (481, 641, 60, 80)):
        y0, x0, ch, cw = M.fit_crop(h, w, ho, wo)
        assert (y0, x0, ch, cw) == A.fit_crop(h, w, ho, wo)
        assert not (y0 | x0 | ch | cw) & 1 and y0 + ch <= h and x0 + cw <= w
        assert ch + 2 > h - 1 or cw + 2 > w - 1  # the largest: one axis is used up
        assert abs((h - ch) - 2 * y0) <= 2 and abs((w - cw) - 2 * x0) <= 2  # centred
        assert M.load().mcraw_area_work_bytes(_area(cw, ch, wo, ho, x0, y0)) > 0
    for bad in ((100, 100, 100, 100), (100, 100, 51, 50), (4000, 4000, 100, 100), (100, 100, 1, 60), (0, 100, 10, 10),
                (100, 100, 0, 10), (100.5, 100, 10, 10), (100, 100, 10, True)):
        with pytest.raises(ValueError):
            M.fit_crop(*bad)
