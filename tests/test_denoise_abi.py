"""Denoising of mosaics (mcraw_denoise_batch) without a GPU: the ABI's symbol and struct, the numpy statement of the contract
(_denoise_ref) against a scalar one written straight from the header, the neighbour rule, properties of the statement on every
geometry the GPU tests use, the host helper noise_lut, and what the filter does to noise of the model's own sigma."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _denoise_ref as D
import motioncam_decoder_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (H, W): the cases of tests/test_gpu_denoise.py
GEOMS = ((1, 1), (2, 2), (3, 5), (4, 9), (5, 4), (8, 8), (9, 9), (1, 64), (33, 1), (16, 64), (35, 41), (34, 520), (70, 1002),
         (2160, 3840))
SMALL = tuple(g for g in GEOMS if g[0] * g[1] <= 35 * 41)


def _content(rng, H, W, kind):
    if kind == "full":
        return rng.integers(0, 1 << 16, size=(H, W), dtype=np.uint16)
    if kind == "ties":
        return (rng.integers(0, 1 << 12, size=(H, W), dtype=np.uint16) >> 6 << 6).astype(np.uint16)
    return np.clip(np.rint(800 + 30 * rng.standard_normal((H, W))), 0, 65535).astype(np.uint16)  # "noise"


def test_denoise_symbol_exported_and_listed():
    hdr = open(os.path.join(ROOT, "include", "mcraw_hip.h")).read()
    lib = M.load()
    assert re.search(r"\bmcraw_denoise_batch\s*\(", hdr)
    assert "mcraw_denoise_batch" in M.ABI_SYMBOLS
    assert hasattr(lib, "mcraw_denoise_batch")
    assert re.search(r"#define MCRAW_K_COUNT\s+11\b", hdr)
    assert M.RGB_KERNELS == {"krgb_mhc": 9, "krgb_bin2": 10}
    assert "Denoise" in M.__all__ and "noise_lut" in M.__all__
    # the arithmetic is stated in the header as the kernel and the reference follow it
    for line in ("x = min((|a - c| * r) >> 8, 16)", "w = 256 - x * x", "m   = (num + (den >> 1)) / den",
                 "out = c + (((m - c) * amount + 128) >> 8)"):
        assert line in hdr, line


def test_denoise_struct_layout():
    assert C.sizeof(M.Denoise) == 40
    names = ("radius", "amount", "lut_log2", "shift", "nluts", "reserved", "lut")
    assert [getattr(M.Denoise, f).offset for f in names] == [0, 4, 8, 12, 16, 20, 32]
    hdr = open(os.path.join(ROOT, "include", "mcraw_hip.h")).read()
    m = re.search(r"\}\s*mcraw_denoise;\s*/\*\s*sizeof (\d+); amount (\d+), lut_log2 (\d+), shift (\d+), nluts (\d+), reserved (\d+), "
                  r"lut (\d+)", hdr)
    assert m and [int(v) for v in m.groups()] == [C.sizeof(M.Denoise)] + [getattr(M.Denoise, f).offset for f in names[1:]]


def test_neighbour_rule():
    for size in range(1, 10):
        for c in range(size):
            for d in (-4, -2, 2, 4):
                a, b = c + d, c - d
                want = a if 0 <= a < size else b if 0 <= b < size else c
                assert int(D.neighbour(c, d, size)) == want
    assert len(D.offsets(1)) == 8 and len(D.offsets(2)) == 24
    assert set(D.offsets(1)) == {(dy, dx) for dy in (-2, 0, 2) for dx in (-2, 0, 2)} - {(0, 0)}
    assert set(D.offsets(2)) == {(dy, dx) for dy in (-4, -2, 0, 2, 4) for dx in (-4, -2, 0, 2, 4)} - {(0, 0)}


def _scalar(img, lut, shift, radius, amount):
    """The header's per-pixel statement, one pixel at a time, in Python integers."""
    H, W = img.shape
    L = lut.shape[1]

    def nb(c, d, size):
        if 0 <= c + d < size:
            return c + d
        if 0 <= c - d < size:
            return c - d
        return c

    steps = range(-2 * radius, 2 * radius + 1, 2)
    out = np.empty((H, W), np.uint16)
    for y in range(H):
        for x in range(W):
            c = int(img[y, x])
            r = int(lut[(y & 1) * 2 + (x & 1)][min(c >> shift, L - 1)])
            num, den = 256 * c, 256
            for dy in steps:
                for dx in steps:
                    if dy == 0 and dx == 0:
                        continue
                    a = int(img[nb(y, dy, H) if dy else y, nb(x, dx, W) if dx else x])
                    xx = min((abs(a - c) * r) >> 8, 16)
                    w = 256 - xx * xx
                    num += w * a
                    den += w
            m = (num + (den >> 1)) // den
            out[y, x] = c + (((m - c) * amount + 128) >> 8)
    return out


@pytest.mark.parametrize("geom", SMALL)
def test_numpy_statement_equals_the_scalar_one(geom):
    H, W = geom
    rng = np.random.default_rng(H * 4099 + W)
    lut, shift = M.noise_lut(2e-4, 2e-6, 64, 4095, entries=64)
    rnd = rng.integers(0, 1 << 16, size=(4, 256), dtype=np.uint16)
    for kind, table, sh in (("noise", lut, shift), ("ties", rnd >> 4, 4), ("full", rnd >> 9, 8)):
        img = _content(rng, H, W, kind)
        for radius in (1, 2):
            for amount in (1, 128, 256):
                want = _scalar(img, table, sh, radius, amount)
                assert np.array_equal(D.denoise(img[None], table, sh, radius, amount)[0], want), (kind, radius, amount)


def _box_mean(img, radius):
    """The rounded mean of the pixel and its reflected neighbours, written on its own: one gathered copy per offset, summed."""
    H, W = img.shape
    P = 2 * radius
    acc = img.astype(np.int64).copy()
    yy, xx = np.arange(H), np.arange(W)
    for dy in range(-P, P + 1, 2):
        for dx in range(-P, P + 1, 2):
            if dy == 0 and dx == 0:
                continue
            ry = np.array([y + dy if 0 <= y + dy < H else y - dy if 0 <= y - dy < H else y for y in yy])
            rx = np.array([x + dx if 0 <= x + dx < W else x - dx if 0 <= x - dx < W else x for x in xx])
            acc += img[ry[:, None], rx[None, :]]
    k = (2 * radius + 1) ** 2
    return (acc + k // 2) // k


@pytest.mark.parametrize("geom", GEOMS)
def test_properties_of_the_statement(geom):
    H, W = geom
    big = H * W > 1 << 20  # the large frame: one content, radius 2, m computed twice in all (the rule knows no size)
    rng = np.random.default_rng(H * 131 + W)
    ident = np.full((4, 256), 65535, np.uint16)
    zero = np.zeros((4, 64), np.uint16)
    rnd = rng.integers(0, 1 << 16, size=(4, 1024), dtype=np.uint16)
    lut, shift = M.noise_lut(2e-4, 2e-6, 64, 4095)
    for kind in ("noise",) if big else ("full", "ties", "noise"):
        img = _content(rng, H, W, kind)
        c = img.astype(np.int64)
        for radius in (2,) if big else (1, 2):
            # an all-0 table is the reflected box mean; an all-65535 table is the identity
            assert np.array_equal(D.mean(img, zero, 10, radius), _box_mean(img, radius))
            if not big:
                assert np.array_equal(D.denoise(img[None], ident, 8, radius)[0], img)
            # amount 256 returns m; every amount lies between c and m
            tab, sh = (lut, shift) if kind == "noise" else (rnd >> 6, 6)
            m = D.mean(img, tab, sh, radius)
            assert np.array_equal(D.blend(c, m, 256), m)
            for amount in (1, 2, 77, 128, 255):
                o = D.blend(c, m, amount)
                assert (np.minimum(c, m) <= o).all() and (o <= np.maximum(c, m)).all()
                assert big or np.array_equal(D.denoise(img[None], tab, sh, radius, amount)[0], o)
            if kind == "noise":
                assert (m != c).any() or (H <= 2 and W <= 2)  # the filter is at work (every neighbour of a 2 x 2 frame is the pixel)
    if big:
        return
    # a flat frame comes back unchanged under any table
    flat = np.full((1, H, W), 1234, np.uint16)
    for tab, sh in ((ident, 8), (zero, 10), (rnd, 6)):
        assert np.array_equal(D.denoise(flat, tab, sh, 2, 256), flat)
        assert np.array_equal(D.denoise(flat, tab, sh, 1, 200), flat)


def test_noise_lut():
    lut, shift = M.noise_lut(2e-4, 2e-6, 64, 4095)
    assert lut.shape == (4, 256) and lut.dtype == np.uint16 and shift == 4  # 4095 >> 4 = 255 < 256, 4095 >> 3 = 511
    assert (lut[0] == lut[1]).all() and (lut[0] == lut[3]).all()
    # by hand: entry 0, m = 8 < black: var = O R^2 = 2e-6 * 4031^2 = 32.497922, sigma 5.70069, 4096 / (3 * 5.70069) = 239.50
    R = 4031.0
    assert lut[0, 0] == int(np.rint(4096 / (3 * np.sqrt(2e-6 * R * R))))
    # entry 100: m = 1608, var = 2e-4 * 4031 * 1544 + 32.497922 = 1277.270722, sigma 35.7389, entry rint(38.2029) = 38
    assert lut[0, 100] == 38
    assert lut[0, 255] == int(np.rint(4096 / (3 * np.sqrt(2e-4 * R * (4088 - 64) + 2e-6 * R * R))))
    assert (np.diff(lut[0].astype(np.int64)) <= 0).all()  # the cut-off grows with the level
    # the shift is the smallest with (top >> shift) < entries
    for top, entries, want in ((4095, 256, 4), (4095, 1024, 2), (4095, 64, 6), (1023, 1024, 0), (65535, 64, 10), (16383, 512, 5),
                               (255, 256, 0), (256, 256, 1)):
        l2, s2 = M.noise_lut(1e-4, 1e-6, 0, 4095 if top < 4095 else top, entries=entries, top=top)
        assert s2 == want and l2.shape == (4, entries), (top, entries, s2)
    assert M.noise_lut(2e-4, 2e-6, 64, 4095, top=65535)[1] == 8
    # per-position arguments
    S, O, black = (1e-4, 2e-4, 3e-4, 4e-4), (1e-6, 2e-6, 3e-6, 4e-6), (60, 62, 64, 66)
    lut4, sh4 = M.noise_lut(S, O, black, 1023, strength=2.5, entries=128)
    assert sh4 == 3
    for p in range(4):
        one, _ = M.noise_lut(S[p], O[p], black[p], 1023, strength=2.5, entries=128)
        assert np.array_equal(lut4[p], one[0])
        i = 77
        m = (i << 3) + 4
        Rp = 1023 - black[p]
        var = S[p] * Rp * max(m - black[p], 0) + O[p] * Rp * Rp
        assert lut4[p, i] == int(np.clip(np.rint(4096 / (2.5 * np.sqrt(var))), 1, 65535))
    assert len({lut4[p].tobytes() for p in range(4)}) == 4
    # strength scales the cut-off; a zero variance gives 65535; entries clip at 1
    a, _ = M.noise_lut(2e-4, 2e-6, 64, 4095, strength=1.5)
    assert abs(int(a[0, 100]) - 2 * int(lut[0, 100])) <= 1
    z, _ = M.noise_lut(1e-4, 0.0, 64, 4095)
    assert (z[:, :4] == 65535).all() and z[0, 4] < 65535  # m = 8 .. 56 below black, then 72
    assert (M.noise_lut(0.0, 0.0, 0, 4095)[0] == 65535).all()
    assert M.noise_lut(10.0, 10.0, 0, 65535, strength=100.0)[0].min() == 1
    for kw in (dict(entries=100), dict(entries=32), dict(entries=2048), dict(white=64), dict(white=10), dict(S=-1e-4),
               dict(O=-1e-6), dict(strength=0.0), dict(strength=-1.0), dict(S=(1e-4, 1e-4, -1e-4, 1e-4)), dict(black=(64, 64, 5000, 64)),
               dict(S=(1e-4, 1e-4)), dict(black=(1, 2, 3))):
        args = dict(S=2e-4, O=2e-6, black=64, white=4095)
        args.update(kw)
        with pytest.raises(ValueError):
            M.noise_lut(**args)


def _noisy(rng, clean, S, O, black, white):
    R = white - black
    sigma = np.sqrt(S * R * np.maximum(clean - black, 0) + O * R * R)
    return np.clip(np.rint(clean + sigma * rng.standard_normal(clean.shape)), 0, 65535).astype(np.uint16)


def test_what_the_filter_does_to_noise_of_the_models_sigma():
    S, O, black, white = 2e-4, 2e-6, 64, 4095
    lut, shift = M.noise_lut(S, O, black, white, strength=3.0, entries=256)
    assert shift == 4
    rng = np.random.default_rng(5)
    for level in (100, 400, 2000):
        img = _noisy(rng, np.full((128, 128), float(level)), S, O, black, white)
        for radius, bound in ((2, 0.45), (1, 0.6)):
            out = D.denoise(img[None], lut, shift, radius, 256)[0]
            ratio = out.std() / img.std()
            moved = out.mean() - img.mean()
            print("level %d radius %d: std ratio %.3f, mean moved %+.3f DN" % (level, radius, ratio, moved))
            assert ratio < bound, (level, radius, ratio)
            assert abs(moved) < 0.5, (level, radius, moved)
    # a vertical step from 400 to 1600: the edge stays where it is and as high as it is
    clean = np.full((128, 128), 400.0)
    clean[:, 64:] = 1600.0
    img = _noisy(rng, clean, S, O, black, white)
    out = D.denoise(img[None], lut, shift, 2, 256)[0]
    cols = out.mean(axis=0)
    worst = max(np.abs(cols[:64] - 400).max(), np.abs(cols[64:] - 1600).max())
    print("step: column means within %.2f DN of the clean levels" % worst)
    assert worst < 6, worst
