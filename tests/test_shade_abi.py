"""Lens-shading gain maps (mcraw_shade_batch) without a GPU: the ABI's symbol and struct, properties of the numpy statement
of the arithmetic (_shade_ref) for every geometry and map size the GPU tests use, and the host helpers gain_map /
shading_map."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _shade_ref as S
import motioncam_decoder_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (H, W) and (gh, gw): the cases of tests/test_gpu_shade.py
GEOMS = ((16, 64), (34, 520), (70, 1002), (2160, 3840), (35, 41), (1, 64), (33, 1), (71, 1001))
MAPS = ((1, 1), (2, 2), (13, 17), (64, 64), (3, 64))
CASES = [(g, m) for g in GEOMS for m in MAPS]


def _rand_map(rng, gh, gw):
    return rng.integers(0, 1 << 16, size=(4, gh, gw), dtype=np.uint16)


def _vignette(gh, gw, strength=(1.9, 1.4, 1.45, 2.3)):
    """Unquantised gains of a lens-like map: 1 in the centre, rising with the squared radius, per channel."""
    y = np.linspace(-1, 1, gh)[:, None] if gh > 1 else np.zeros((1, 1))
    x = np.linspace(-1, 1, gw)[None, :] if gw > 1 else np.zeros((1, 1))
    r2 = (x * x + y * y) / 2
    return np.stack([1.0 + (s - 1.0) * r2 + 0.03 * x * (i - 1.5) for i, s in enumerate(strength)])


def test_shade_symbol_exported_and_listed():
    hdr = open(os.path.join(ROOT, "include", "mcraw_hip.h")).read()
    assert re.search(r"\bmcraw_shade_batch\s*\(", hdr)
    assert "mcraw_shade_batch" in M.ABI_SYMBOLS
    assert hasattr(M.load(), "mcraw_shade_batch")
    assert re.search(r"#define MCRAW_K_COUNT\s+11\b", hdr)
    assert M.RGB_KERNELS == {"krgb_mhc": 9, "krgb_bin2": 10}


def test_shade_struct_layout():
    assert C.sizeof(M.Shade) == 40
    names = ("map_w", "map_h", "nmaps", "top", "black", "reserved", "map")
    assert [getattr(M.Shade, f).offset for f in names] == [0, 4, 8, 12, 16, 24, 32]
    hdr = open(os.path.join(ROOT, "include", "mcraw_hip.h")).read()
    m = re.search(r"\}\s*mcraw_shade;\s*/\*\s*sizeof (\d+); black (\d+), reserved (\d+), map (\d+)", hdr)
    assert m and [int(v) for v in m.groups()] == [C.sizeof(M.Shade), M.Shade.black.offset, M.Shade.reserved.offset,
                                                  M.Shade.map.offset]


@pytest.mark.parametrize("geom,mp", CASES)
def test_unit_map_is_the_identity(geom, mp):
    (H, W), (gh, gw) = geom, mp
    rng = np.random.default_rng(H * 131 + W + gh * 7 + gw)
    img = rng.integers(0, 1 << 16, size=(H, W), dtype=np.uint16)
    unit = np.full((4, gh, gw), 4096, np.uint16)
    for black in ((0, 0, 0, 0), (64, 65, 1000, 65535)):
        assert np.array_equal(S.shade_ref(img, unit, black), img)
    # ... and the black level of the output is the black level of the input, whatever the gain
    flat = np.empty((H, W), np.uint16)
    black = (64, 80, 96, 112)
    for p in range(4):
        flat[p >> 1::2, p & 1::2] = black[p]
    assert np.array_equal(S.shade_ref(flat, _rand_map(rng, gh, gw), black), flat)


@pytest.mark.parametrize("geom,mp", CASES)
def test_bit15_ignored_extremes_monotone_top(geom, mp):
    (H, W), (gh, gw) = geom, mp
    rng = np.random.default_rng(H * 17 + W * 3 + gh * 64 + gw)
    gm = _rand_map(rng, gh, gw)
    img = rng.integers(0, 1 << 16, size=(H, W), dtype=np.uint16)
    black = tuple(int(b) for b in rng.integers(0, 5000, size=4))
    G, _ = S.gains(H, W, gm)
    want = S.apply(img, G, black)
    assert np.array_equal(S.shade_ref(img, gm ^ 0x8000, black), want)
    assert np.array_equal(S.shade_ref(img, gm & 0x7FFF, black), want)
    # the extreme products stay below 2^31: the largest sample over black 0 and the smallest under black 65535, largest gain
    Gtop, peak = S.gains(H, W, np.full((4, gh, gw), 0xFFFF, np.uint16))
    assert (Gtop == 32767).all() and peak < 1 << 31
    hi, peak_hi = S.apply(np.full((H, W), 65535, np.uint16), Gtop, (0, 0, 0, 0), with_peak=True)
    lo, peak_lo = S.apply(np.zeros((H, W), np.uint16), Gtop, (65535,) * 4, with_peak=True)
    assert max(peak_hi, peak_lo) < 1 << 31
    assert (hi == 65535).all() and (lo == 0).all()
    # monotone in the sample, at every pixel's own gain
    ladder = np.sort(rng.integers(0, 1 << 16, size=9 if H * W < 1 << 20 else 4, dtype=np.uint16))
    prev = None
    for v in ladder:
        cur = S.apply(np.full((H, W), v, np.uint16), G, black).astype(np.int64)
        assert prev is None or (cur >= prev).all()
        prev = cur
    # top saturates, and only saturates
    for top in (1, 1023, 4095, 65534):
        got = S.apply(img, G, black, top)
        assert int(got.max()) <= top and np.array_equal(got, np.minimum(want, top))


@pytest.mark.parametrize("geom,mp", CASES)
def test_gain_close_to_float64_bilinear(geom, mp):
    """G against float64 bilinear interpolation of the unquantised gains, in LSB of Q12.  The bound is derived: three
    roundings of at most 0.5 (the entry, V, G); a weight that is truncated to 12 bits (1/4096 of a cell) and taken from a
    floored step (at most (size - 1) / 2^24 of a cell by the last pixel), each times the largest difference between
    neighbouring map entries in its direction."""
    (H, W), (gh, gw) = geom, mp
    rng = np.random.default_rng(gh * 100 + gw)
    for fg in (_vignette(gh, gw), rng.uniform(0.0, 7.99, size=(4, gh, gw))):
        gm = M.gain_map(fg, order="cfa")
        q = gm.astype(np.int64)
        Dy = int(np.abs(np.diff(q, axis=1)).max()) if gh > 1 else 0
        Dx = int(np.abs(np.diff(q, axis=2)).max()) if gw > 1 else 0
        bound = 1.5 + Dy * (1 / 4096 + (H - 1) / 2 ** 24) + Dx * (1 / 4096 + (W - 1) / 2 ** 24)
        G, _ = S.gains(H, W, gm)
        err = np.abs(G - S.float_gains(H, W, fg) * 4096.0).max()
        print("H %d W %d map %dx%d: max error %.4f LSB, bound %.4f" % (H, W, gh, gw, err, bound))
        assert err <= bound


@pytest.mark.parametrize("cfa", ("rggb", "bggr", "grbg", "gbrg"))
def test_gain_map_permutation_and_rounding(cfa):
    rng = np.random.default_rng(5)
    g = rng.uniform(0, 7.9, size=(3, 4, 5, 7))
    q = M.gain_map(g, cfa)
    assert q.dtype == np.uint16 and q.shape == g.shape and q.flags["C_CONTIGUOUS"]
    planes = M.cfa_planes(cfa)
    for p in range(4):  # CFA position p holds the plane that cfa_planes puts there: R, G (R row), G (B row), B = 0..3
        assert np.array_equal(q[:, p], np.rint(g[:, planes[p]] * 4096).astype(np.uint16))
    assert np.array_equal(M.gain_map(g[0], cfa), q[0])
    assert np.array_equal(M.gain_map(g, cfa, order="cfa"), np.rint(g * 4096).astype(np.uint16))
    # rint: ties to even, and the ends of the range
    e = M.gain_map(np.array([0.5 / 4096, 1.5 / 4096, 1.0, 0.0, 32767 / 4096, 32767.49 / 4096] + [1.0] * 6).reshape(4, 1, 3))
    assert list(e.ravel()[:6]) == [0, 2, 4096, 0, 32767, 32767]


@pytest.mark.parametrize("bad", (np.nan, np.inf, -0.001, 32767.5 / 4096, 8.0))
def test_gain_map_rejects(bad):
    g = np.ones((4, 3, 3))
    g[2, 1, 1] = bad
    with pytest.raises(ValueError):
        M.gain_map(g)
    with pytest.raises(ValueError):
        M.gain_map(np.ones((3, 3, 3)))
    with pytest.raises(ValueError):
        M.gain_map(np.ones((4, 3, 3)), "xyzw")
    with pytest.raises(ValueError):
        M.gain_map(np.ones((4, 3, 3)), order="bayer")


def test_shading_map_layouts_and_absent_keys():
    rng = np.random.default_rng(9)
    gh, gw = 13, 17
    g = rng.uniform(1.0, 3.0, size=(4, gh, gw))
    flat = {"lensShadingMap": [pl.ravel().tolist() for pl in g], "lensShadingMapWidth": gw, "lensShadingMapHeight": gh}
    rows = {"lensShadingMap": [pl.tolist() for pl in g], "lensShadingMapWidth": gw, "lensShadingMapHeight": gh}
    bare = {"lensShadingMap": [pl.tolist() for pl in g]}
    for cfa in ("rggb", "gbrg"):
        want = M.gain_map(g, cfa)
        for meta in (flat, rows, bare):
            got = M.shading_map(meta, cfa)
            assert got.dtype == np.uint16 and np.array_equal(got, want)
    assert M.shading_map({}, "rggb") is None
    assert M.shading_map({"asShotNeutral": [0.5, 1, 0.6]}, "rggb") is None
    assert M.shading_map(None, "rggb") is None
    with pytest.raises(ValueError):  # flat planes without their size
        M.shading_map({"lensShadingMap": flat["lensShadingMap"]}, "rggb")
    with pytest.raises(ValueError):
        M.shading_map(dict(flat, lensShadingMapWidth=gw + 1), "rggb")
    with pytest.raises(ValueError):
        M.shading_map({"lensShadingMap": flat["lensShadingMap"][:3], "lensShadingMapWidth": gw, "lensShadingMapHeight": gh})
