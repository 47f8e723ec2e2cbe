"""Temporal merge of mosaics (mcraw_merge_batch) without a GPU: the ABI's symbol and struct, the numpy statement of the contract
(_merge_ref) against a scalar one written straight from the header, the consequences the contract names, the shift rule, and
what the filter does to noise of the model's own sigma, to a moving object and to an isolated outlier."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _merge_ref as R
import motioncam_decoder_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = ((1, 1), (2, 2), (3, 5), (5, 4), (9, 9), (1, 64), (33, 1), (35, 41))  # (H, W): the small cases of tests/test_gpu_merge.py
PROFILE = dict(S=2e-4, O=2e-6, black=64, white=4095)


def _hdr():
    return open(os.path.join(ROOT, "include", "mcraw_hip.h")).read()


def test_merge_symbol_exported_and_listed():
    hdr = _hdr()
    lib = M.load()
    assert re.search(r"\bmcraw_merge_batch\s*\(", hdr)
    assert "mcraw_merge_batch" in M.ABI_SYMBOLS
    assert hasattr(lib, "mcraw_merge_batch")
    assert re.search(r"#define MCRAW_K_COUNT\s+11\b", hdr)
    assert M.RGB_KERNELS == {"krgb_mhc": 9, "krgb_bin2": 10}
    assert "Merge" in M.__all__
    block = hdr[hdr.index("temporally merged uint16 mosaics"):hdr.index("} mcraw_merge;")]
    # the arithmetic is stated in the header as the kernel and the reference follow it
    for line in ("sy = (pos[t].y - pos[b].y) & ~1", "D = |e0|", "D = max(min(|s| >> 3, 65535), |e0| >> 1)",
                 "r   = lut[f][p][min(c >> shift, L - 1)]", "x = min((D * r) >> 8, 16)", "w = 256 - x * x",
                 "num = 256 * c + sum(w * a)", "den = 256 + sum(w)", "m   = (num + (den >> 1)) / den",
                 "out = c + (((m - c) * amount + 128) >> 8)"):
        assert line in block, line


def test_merge_struct_layout():
    names = ("before", "after", "first", "count", "support", "amount", "lut_log2", "shift", "nluts", "reserved", "lut", "pos")
    assert C.sizeof(M.Merge) == 56
    assert [getattr(M.Merge, f).offset for f in names] == [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 48]
    m = re.search(r"\}\s*mcraw_merge;\s*/\*\s*sizeof (\d+); after (\d+), first (\d+), count (\d+), support (\d+), amount (\d+), "
                  r"lut_log2 (\d+), shift (\d+), nluts (\d+), reserved (\d+), lut (\d+), pos (\d+)", _hdr())
    assert m and [int(v) for v in m.groups()] == [56, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 48]


def _scalar(imgs, lut, shift, before, after, first, count, support, amount, pos):
    """The header's per-pixel statement, one pixel at a time, in Python integers."""
    n, H, W = imgs.shape
    out = np.empty((count, H, W), np.uint16)
    for j in range(count):
        b = first + j
        tab = lut if lut.ndim == 2 else lut[b]
        L = tab.shape[1]
        for y in range(H):
            for x in range(W):
                c = int(imgs[b, y, x])
                r = int(tab[(y & 1) * 2 + (x & 1)][min(c >> shift, L - 1)])
                num, den = 256 * c, 256
                for t in range(max(0, b - before), min(n - 1, b + after) + 1):
                    if t == b:
                        continue
                    sy = sx = 0
                    if pos is not None:
                        sy, sx = (int(pos[t][0]) - int(pos[b][0])) & ~1, (int(pos[t][1]) - int(pos[b][1])) & ~1
                    if not (0 <= y + sy < H and 0 <= x + sx < W):
                        continue  # the member weighs 0
                    a = int(imgs[t, y + sy, x + sx])
                    e0 = a - c
                    if support == 0:
                        D = abs(e0)
                    else:
                        s = 0
                        for dy in (-1, 0, 1):
                            for dx in (-1, 0, 1):
                                by, bx = y + dy, x + dx
                                if 0 <= by < H and 0 <= bx < W and 0 <= by + sy < H and 0 <= bx + sx < W:
                                    s += int(imgs[t, by + sy, bx + sx]) - int(imgs[b, by, bx])
                                else:
                                    s += e0
                        D = max(min(abs(s) >> 3, 65535), abs(e0) >> 1)
                    xx = min((D * r) >> 8, 16)
                    w = 256 - xx * xx
                    num += w * a
                    den += w
                m = (num + (den >> 1)) // den
                out[j, y, x] = c + (((m - c) * amount + 128) >> 8)
    return out


def _content(rng, n, H, W, kind):
    if kind == "full":
        return rng.integers(0, 1 << 16, size=(n, H, W), dtype=np.uint16)
    if kind == "ties":
        return (rng.integers(0, 1 << 12, size=(n, H, W), dtype=np.uint16) >> 6 << 6).astype(np.uint16)
    return np.clip(np.rint(800 + 30 * rng.standard_normal((n, H, W))), 0, 65535).astype(np.uint16)  # "noise"


@pytest.mark.parametrize("geom", SMALL)
def test_numpy_statement_equals_the_scalar_one(geom):
    H, W = geom
    rng = np.random.default_rng(H * 4099 + W)
    lut, shift = M.noise_lut(entries=64, **PROFILE)
    rnd = rng.integers(0, 1 << 16, size=(6, 4, 256), dtype=np.uint16)
    big = H * W > 600
    for kind, table, sh in (("noise", lut, shift), ("ties", rnd[0] >> 4, 4), ("full", rnd >> 9, 8)):
        for n, before, after, first, count in ((1, 2, 2, 0, 1), (6, 2, 2, 0, 6), (6, 0, 5, 0, 1), (5, 5, 0, 2, 3), (4, 0, 0, 1, 2)):
            if big and (n, before) not in ((6, 2), (5, 5)):
                continue
            imgs = _content(rng, n, H, W, kind)
            tab = table if table.ndim == 2 else table[:n]
            far = np.zeros((n, 2), np.int64)
            far[1::2] = (2 * H + 1, -2 * W - 1)
            for pos in (None, rng.integers(-6, 7, size=(n, 2)), far):
                for support in (0, 1):
                    amount = (1, 128, 256)[(support + n) % 3]
                    want = _scalar(imgs, tab, sh, before, after, first, count, support, amount, pos)
                    got = R.merge(imgs, tab, sh, before, after, first, count, support, amount, pos)
                    assert np.array_equal(got, want), (kind, n, before, after, first, count, support, pos)


def test_shift_rule():
    for d, want in ((0, 0), (1, 0), (2, 2), (3, 2), (-1, -2), (-2, -2), (-3, -4), (-5, -6), (7, 6), (65535, 65534), (-65535, -65536)):
        pos = np.array([[0, 0], [d, -d]], np.int64)
        assert R.shift_of(pos, 1, 0) == (want, (-d) & ~1), d
    pos16 = np.array([[32767, -32768], [-32768, 32767]], np.int16)  # the difference is taken in int32, not in int16
    assert R.shift_of(pos16, 1, 0) == (-65536, 65534) and R.shift_of(pos16, 0, 1) == (65534, -65536)
    assert R.shift_of(None, 3, 1) == (0, 0)
    assert R.window(0, 6, 2, 2) == [1, 2] and R.window(5, 6, 2, 2) == [3, 4] and R.window(3, 6, 5, 0) == [0, 1, 2]
    assert R.window(2, 6, 0, 0) == [] and R.window(0, 1, 7, 8) == []
    # a sample keeps its CFA position: a member that equals the base moved by an odd offset is read at the even one
    rng = np.random.default_rng(2)
    img = rng.integers(0, 4096, size=(12, 14), dtype=np.uint16)
    a, inside, D = R.measure(img, img, *R.shift_of(np.array([[0, 0], [3, -3]]), 1, 0), 0)
    assert np.array_equal(a[:10, 4:], img[2:, :10]) and inside[:10, 4:].all() and not inside[10:].any() and not inside[:, :4].any()


@pytest.mark.parametrize("geom", SMALL)
def test_consequences_of_the_contract(geom):
    H, W = geom
    rng = np.random.default_rng(H * 131 + W)
    n = 6
    ident = np.full((4, 256), 65535, np.uint16)
    zero = np.zeros((4, 64), np.uint16)
    rnd = rng.integers(0, 1 << 16, size=(4, 1024), dtype=np.uint16)
    lut, shift = M.noise_lut(**PROFILE)
    pos = rng.integers(-6, 7, size=(n, 2))
    far = np.arange(n)[:, None] * np.array([[2 * H + 1, 2 * W + 1]])
    for kind in ("full", "ties", "noise"):
        imgs = _content(rng, n, H, W, kind)
        for support in (0, 1):
            # the identity: a table of all 65535, an empty window, shifts that leave the frame
            if support == 0 or kind != "noise":  # (support 1 and samples that differ by exactly 1: see the test below)
                for p in (None, pos):
                    assert np.array_equal(R.merge(imgs, ident, 8, 2, 2, support=support, pos=p), imgs)
            assert np.array_equal(R.merge(imgs, rnd >> 6, 6, 0, 0, support=support, pos=pos), imgs)
            assert np.array_equal(R.merge(imgs, zero, 10, 2, 3, support=support, pos=far), imgs)
            # a table of all 0 with no shifts is the rounded mean of the window
            for before, after in ((2, 2), (0, 5), (5, 0)):
                got = R.merge(imgs, zero, 10, before, after, support=support)
                for b in range(n):
                    lo, hi = max(0, b - before), min(n - 1, b + after)
                    k = hi - lo + 1
                    assert np.array_equal(got[b], (imgs[lo:hi + 1].astype(np.int64).sum(axis=0) + k // 2) // k)
            # out lies between c and m; amount 256 gives m
            tab, sh = (lut, shift) if kind == "noise" else (rnd >> 6, 6)
            for b in (0, 3):
                c = imgs[b].astype(np.int64)
                m = R.mean(imgs, b, tab, sh, 2, 2, support, pos)
                assert np.array_equal(R.blend(c, m, 256), m)
                for amount in (1, 77, 255):
                    o = R.blend(c, m, amount)
                    assert (np.minimum(c, m) <= o).all() and (o <= np.maximum(c, m)).all()
                    assert np.array_equal(R.merge(imgs, tab, sh, 2, 2, b, 1, support, amount, pos)[0], o)


def test_identity_table_and_differences_of_one():
    """Under the all-65535 table a member's sample counts only where D is 0.  With support 0 that sample equals the base pixel.
    With support 1, D = 0 also admits e0 = +-1 under a 3x3 sum below 8: a sample one above the base pixel then lifts the
    rounded mean by one (the header says so); content whose samples differ by 0 or by 2 and more comes back bit for bit."""
    base = np.full((1, 3, 3), 500, np.uint16)
    up, down = base.copy(), base.copy()
    up[0, 1, 1], down[0, 1, 1] = 501, 499
    ident = np.full((4, 64), 65535, np.uint16)
    for other, want in ((up, 501), (down, 500)):
        imgs = np.concatenate([base, other])
        assert np.array_equal(R.merge(imgs, ident, 10, 0, 1, 0, 1, support=0), base)
        got = R.merge(imgs, ident, 10, 0, 1, 0, 1, support=1)
        assert got[0, 1, 1] == want and (np.delete(got.reshape(-1), 4) == 500).all()


def _noisy(rng, clean):
    S, O, black, white = PROFILE["S"], PROFILE["O"], PROFILE["black"], PROFILE["white"]
    Rg = white - black
    sigma = np.sqrt(S * Rg * np.maximum(clean - black, 0) + O * Rg * Rg)
    return np.clip(np.rint(clean + sigma * rng.standard_normal(clean.shape)), 0, 65535).astype(np.uint16)


def _sigma(level):
    Rg = PROFILE["white"] - PROFILE["black"]
    return float(np.sqrt(PROFILE["S"] * Rg * (level - PROFILE["black"]) + PROFILE["O"] * Rg * Rg))


# What the committed statement gives for the committed seed on 96 x 96 patches (standard deviation out / in):
# (support, window) -> levels 100, 400, 2000.  The ideal is 1 / sqrt(window): 0.447 and 0.333.
EXPECTED = {
    (1, 5): (0.452, 0.452, 0.454),
    (1, 9): (0.345, 0.341, 0.339),
    (0, 5): (0.582, 0.580, 0.582),
    (0, 9): (0.481, 0.474, 0.475),
}


def test_what_the_filter_does_to_noise_of_the_models_sigma():
    lut, shift = M.noise_lut(strength=3.0, entries=256, **PROFILE)
    assert shift == 4
    rng = np.random.default_rng(5)
    side = 96  # the standard error of the output's mean: at most 0.46 * 40 / 96 = 0.19 DN (level 2000), below a quarter DN
    for li, level in enumerate((100, 400, 2000)):
        assert 0.5 * _sigma(level) / side < 0.25
        imgs = _noisy(rng, np.full((9, side, side), float(level)))
        for support in (1, 0):
            for T in (2, 4):
                out = R.merge(imgs, lut, shift, T, T, 4, 1, support, 256)[0]
                ratio = out.std() / imgs[4].std()
                moved = out.mean() - level
                print("level %d support %d window %d: std ratio %.3f, mean %+.3f DN off the level" % (level, support, 2 * T + 1, ratio, moved))
                assert ratio <= EXPECTED[(support, 2 * T + 1)][li] + 0.03, (level, support, T, ratio)
                if support == 1 and T == 2:
                    assert ratio < 0.5, (level, ratio)
                assert abs(moved) < 1.0, (level, support, T, moved)


def test_a_moving_square_is_not_smeared():
    """A 16-pixel square moving 8 pixels per frame over 5 frames, merged onto the middle frame: the robust merge is no worse
    than the noisy base frame itself, where the plain mean of the window (the all-0 table) leaves most of the square's height."""
    rng = np.random.default_rng(6)
    n, H, W = 5, 64, 96
    clean = np.full((n, H, W), 400.0)
    for t in range(n):
        clean[t, 24:40, 20 + 8 * t:36 + 8 * t] = 1350.0
    imgs = _noisy(rng, clean)
    lut, shift = M.noise_lut(strength=3.0, **PROFILE)
    robust = R.merge(imgs, lut, shift, 2, 2, 2, 1, 1, 256)[0].astype(np.int64)
    plain = R.merge(imgs, np.zeros((4, 64), np.uint16), 10, 2, 2, 2, 1, 1, 256)[0].astype(np.int64)
    err_in = np.abs(imgs[2].astype(np.int64) - clean[2]).max()
    err_robust, err_plain = np.abs(robust - clean[2]).max(), np.abs(plain - clean[2]).max()
    print("max error: input %d, robust merge %d, plain mean %d" % (err_in, err_robust, err_plain))
    assert err_robust <= err_in + 1
    assert err_robust < err_plain / 2


def test_an_isolated_outlier_in_a_member_does_not_leak():
    """The leak is what the outlier itself adds to the result at its pixel: the merge of the window that holds it against the
    merge of the same window without that member (the other members' measures do not depend on it)."""
    rng = np.random.default_rng(7)
    lut, shift = M.noise_lut(strength=3.0, **PROFILE)
    for level in (100, 400, 2000):
        sigma = _sigma(level)
        hit = _noisy(rng, np.full((5, 33, 33), float(level)))
        ys, xs = np.meshgrid(np.arange(4, 30, 6), np.arange(4, 30, 6), indexing="ij")  # isolated: 6 apart, in one member
        hit[3, ys, xs] = np.rint(level + 12 * sigma).astype(np.uint16)
        for support in (1, 0):
            got = R.merge(hit, lut, shift, 2, 2, 2, 1, support, 256)[0].astype(np.int64)
            without = R.merge(hit[[0, 1, 2, 4]], lut, shift, 2, 1, 2, 1, support, 256)[0].astype(np.int64)
            leak = np.abs(got - without)[ys, xs].max() / sigma
            print("level %d support %d: a +12 sigma pixel in one member moves the result by %.3f sigma" % (level, support, leak))
            assert leak < 0.1, (level, support, leak)
