"""Per-frame mosaic statistics (mcraw_stats_batch) without a GPU: the ABI's symbols and struct, properties of the numpy
statement of the contract (_stats_ref) on every geometry the GPU tests use, and the host helpers stats_white_balance /
stats_percentile / stats_clipped on closed-form inputs."""
import ctypes as C
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import _stats_ref as S
import motioncam_decoder_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (H, W): the cases of tests/test_gpu_stats.py
GEOMS = ((2, 2), (1, 64), (33, 1), (35, 41), (34, 520), (70, 1002), (71, 1001), (1080, 1920))


def _frames(geom, n=2):
    H, W = geom
    rng = np.random.default_rng(H * 4099 + W)
    return rng.integers(0, 1 << 16, size=(n, H, W), dtype=np.uint16)


def _windows(H, W):
    """The full frame, windows at odd offsets, and the thin ones."""
    ws = [(0, 0, H, W), (H // 2, W // 2, 1, 1), (H - 1, 0, 1, W), (0, W - 1, H, 1)]
    if H > 2 and W > 2:
        ws += [(1, 1, H - 2, W - 2), (1, 0, H - 1, W), (0, 1, H, W - 2)]
    return ws


def test_stats_symbols_exported_and_listed():
    hdr = open(os.path.join(ROOT, "include", "mcraw_hip.h")).read()
    lib = M.load()
    for name in ("mcraw_stats_batch", "mcraw_stats_record_bytes"):
        assert re.search(r"\b%s\s*\(" % name, hdr)
        assert name in M.ABI_SYMBOLS
        assert hasattr(lib, name)
    assert re.search(r"#define MCRAW_STATS_ACCUMULATE\s+1u\b", hdr) and M.STATS_ACCUMULATE == 1
    assert re.search(r"#define MCRAW_K_COUNT\s+11\b", hdr)
    assert M.RGB_KERNELS == {"krgb_mhc": 9, "krgb_bin2": 10}


def test_stats_struct_layout():
    assert C.sizeof(M.Stats) == 40
    names = ("bins_log2", "shift", "x0", "y0", "w", "h", "sat", "flags", "reserved")
    assert [getattr(M.Stats, f).offset for f in names] == [0, 4, 8, 12, 16, 20, 24, 32, 36]
    hdr = open(os.path.join(ROOT, "include", "mcraw_hip.h")).read()
    m = re.search(r"\}\s*mcraw_stats;\s*/\*\s*sizeof (\d+); x0 (\d+), sat (\d+), flags (\d+), reserved (\d+)", hdr)
    assert m and [int(v) for v in m.groups()] == [C.sizeof(M.Stats), M.Stats.x0.offset, M.Stats.sat.offset,
                                                  M.Stats.flags.offset, M.Stats.reserved.offset]


def test_record_bytes():
    lib = M.load()
    for bl in range(0, 20):
        want = 16 * (1 << bl) + 96 if 6 <= bl <= 12 else 0
        assert lib.mcraw_stats_record_bytes(bl) == want
        if want:
            assert S.record_bytes(1 << bl) == want
    assert lib.mcraw_stats_record_bytes(0xFFFFFFFF) == 0


@pytest.mark.parametrize("geom", GEOMS)
def test_reference_counts_and_parity(geom):
    H, W = geom
    imgs = _frames(geom)
    for k, roi in enumerate(_windows(H, W)):
        y0, x0, h, w = roi
        bins, shift = ((64, 10), (256, 8), (4096, 0), (256, 4))[k % 4]
        sat = (65535, 40000, 0, 1000)
        st = S.stats(imgs, bins, shift, sat, roi)
        assert np.array_equal(st["hist"].sum(axis=2), st["cnt"])
        assert (st["cnt"].sum(axis=1) == w * h).all()
        assert (st["nsat"] <= st["cnt"]).all() and np.array_equal(st["nsat"][:, 2], st["cnt"][:, 2])  # sat 0: all of them
        assert (st["sum"][:, 2] == 0).all()
        win = imgs[:, y0:y0 + h, x0:x0 + w]
        for p in range(4):
            # the window's samples of FRAME parity p: a window at an odd offset keeps the frame's positions
            sub = win[:, ((p >> 1) - y0) & 1::2, ((p & 1) - x0) & 1::2]
            assert (st["cnt"][:, p] == sub.shape[1] * sub.shape[2]).all()
            if sub.shape[1] * sub.shape[2] == 0:  # the empty-position convention
                assert (st["min"][:, p] == 65535).all() and (st["max"][:, p] == 0).all()
                assert (st["hist"][:, p] == 0).all() and (st["sum"][:, p] == 0).all() and (st["nsat"][:, p] == 0).all()
                continue
            flat = sub.reshape(len(imgs), -1).astype(np.int64)
            assert np.array_equal(st["min"][:, p], flat.min(axis=1)) and np.array_equal(st["max"][:, p], flat.max(axis=1))
            assert np.array_equal(st["nsat"][:, p], (flat >= sat[p]).sum(axis=1))
            assert np.array_equal(st["sum"][:, p].astype(np.int64), np.where(flat >= sat[p], 0, flat).sum(axis=1))
            assert (st["hist"][:, p, -1] == (flat >> shift >= bins - 1).sum(axis=1)).all()  # the last bin absorbs the rest
        raw = S.record(st)
        assert raw.shape == (len(imgs), S.record_bytes(bins)) and raw.dtype == np.uint8
        back = S.parse(raw, bins)
        assert all(np.array_equal(back[f], st[f]) for f in st)


@pytest.mark.parametrize("geom", GEOMS)
def test_reference_windows_that_tile_a_frame_accumulate_to_it(geom):
    H, W = geom
    imgs = _frames(geom)
    args = (256, 8, (65535, 30000, 65000, 12))
    whole = S.stats(imgs, *args)
    splits = []
    if W > 1:
        cut = W // 2 | 1 if W > 2 else 1  # an odd cut: the second window starts on an odd column
        splits.append(((0, 0, H, cut), (0, cut, H, W - cut)))
    if H > 1:
        cut = H // 2 | 1 if H > 2 else 1
        splits.append(((0, 0, cut, W), (cut, 0, H - cut, W)))
    for a, b in splits:
        acc = S.stats(imgs, *args, roi=b, into=S.stats(imgs, *args, roi=a))
        assert all(np.array_equal(acc[f], whole[f]) for f in whole), (a, b)
        assert np.array_equal(S.record(acc), S.record(whole))


def _closed_form(r, g, b, black, H=8, W=12, cfa="rggb"):
    """A frame whose channels sit at r, g, b above the per-position black levels."""
    plane = M.cfa_planes(cfa)
    img = np.empty((H, W), np.uint16)
    for p in range(4):
        img[p >> 1::2, p & 1::2] = black[p] + (r, g, g, b)[plane[p]]
    return img[None]


@pytest.mark.parametrize("cfa", ("rggb", "bggr", "grbg", "gbrg"))
def test_white_balance_closed_form(cfa):
    black = (64, 65, 66, 67)
    st = S.stats(_closed_form(4000, 2000, 1000, black, cfa=cfa), 256, 8)
    g = M.stats_white_balance(S.helper_input(st, 256, 8), black=black, cfa=cfa)
    assert g.shape == (1, 3) and g.dtype == np.float64
    assert np.allclose(g[0], (0.5, 1.0, 2.0), rtol=1e-12, atol=0)
    # a single record drops N
    one = {k: v[0] for k, v in st.items()}
    assert np.array_equal(M.stats_white_balance(S.helper_input(one, 256, 8), black=black, cfa=cfa), g[0])
    # usable as gain= of the demosaic methods
    assert M.rgb_color is not None and np.asarray(g[0], np.float32).shape == (3,)


def test_white_balance_pools_greens_by_count_and_falls_back():
    # an odd-sized window: the two green positions have different counts; the pooled mean weighs them by count
    img = np.zeros((1, 3, 5), np.uint16)
    img[0, 0::2, 0::2], img[0, 0::2, 1::2], img[0, 1::2, 0::2], img[0, 1::2, 1::2] = 1000, 300, 600, 250
    st = S.stats(img, 64, 10)
    assert st["cnt"][0].tolist() == [6, 4, 3, 2]
    g = M.stats_white_balance(S.helper_input(st, 64, 10))
    green = (4 * 300 + 3 * 600) / 7.0
    assert np.allclose(g[0], (green / 1000, 1.0, green / 250), rtol=1e-12, atol=0)
    # a saturated red channel has no unsaturated sample: gain 1; blue is still measured
    st = S.stats(_closed_form(5000, 2000, 1000, (0, 0, 0, 0)), 256, 8, sat=(5000, 65535, 65535, 65535))
    assert st["nsat"][0].tolist() == [24, 0, 0, 0] and st["sum"][0, 0] == 0
    g = M.stats_white_balance(S.helper_input(st, 256, 8))
    assert g[0].tolist() == [1.0, 1.0, 2.0]
    # a channel at or below black: gain 1
    st = S.stats(_closed_form(0, 2000, 1000, (100, 100, 100, 100)), 256, 8)
    assert M.stats_white_balance(S.helper_input(st, 256, 8), black=(100, 100, 100, 100))[0].tolist() == [1.0, 1.0, 2.0]
    # no usable green: nothing to refer to
    st = S.stats(_closed_form(500, 2000, 1000, (0, 0, 0, 0)), 256, 8, sat=(65535, 2000, 2000, 65535))
    assert M.stats_white_balance(S.helper_input(st, 256, 8))[0].tolist() == [1.0, 1.0, 1.0]
    assert np.array_equal(M.stats_clipped(S.helper_input(st, 256, 8)), [[0.0, 1.0, 1.0, 0.0]])


def test_percentile_edges():
    # 4 x 4: position p holds four samples of values 16 * (4 * p + i), shift 4 -> bins 0 .. 15, one sample each
    img = np.zeros((1, 4, 4), np.uint16)
    for p in range(4):
        img[0, p >> 1::2, p & 1::2] = (16 * (4 * p + np.arange(4))).reshape(2, 2)
    shift, bins = 4, 64
    h = S.helper_input(S.stats(img, bins, shift), bins, shift)
    total = 16
    edge = lambda b: min(((b + 1) << shift) - 1, 65535)
    assert M.stats_percentile(h, 0).tolist() == [edge(0)]
    assert M.stats_percentile(h, Fraction(1, total)).tolist() == [edge(0)]
    assert M.stats_percentile(h, Fraction(2, total)).tolist() == [edge(1)]
    assert M.stats_percentile(h, 0.5).tolist() == [edge(7)]
    assert M.stats_percentile(h, 1).tolist() == [edge(15)]
    assert M.stats_percentile(h, 0.5, pool=False).tolist() == [[edge(1), edge(5), edge(9), edge(13)]]
    assert M.stats_percentile(h, 1.0, pool=False).tolist() == [[edge(3), edge(7), edge(11), edge(15)]]
    assert M.stats_percentile(h, 0, pool=False).tolist() == [[edge(0)] * 4]
    # the upper edge saturates at 65535 when the last bin absorbs the overflow
    top = np.full((1, 2, 2), 65535, np.uint16)
    for bins, shift in ((64, 10), (64, 8), (4096, 4), (256, 15)):
        h = S.helper_input(S.stats(top, bins, shift), bins, shift)
        assert M.stats_percentile(h, 1).tolist() == [min((bins << shift) - 1, 65535)]
    with pytest.raises(ValueError):
        M.stats_percentile(h, 1.5)


def test_clipped_fraction():
    img = np.zeros((2, 4, 6), np.uint16)
    img[1, 0, 0] = img[1, 0, 2] = 4095
    img[1, 1, 1] = 5000
    st = S.stats(img, 64, 6, sat=(4095,) * 4)
    c = M.stats_clipped(S.helper_input(st, 64, 6))
    assert c.shape == (2, 4) and np.array_equal(c, [[0, 0, 0, 0], [2 / 6, 0, 0, 1 / 6]])


def test_frame_stats_views_of_reference_bytes():
    """FrameStats' views address the record as the header lays it out (here over host bytes)."""
    torch = pytest.importorskip("torch")
    imgs = _frames((35, 41), n=3)
    for bins, shift in ((64, 10), (4096, 4)):
        st = S.stats(imgs, bins, shift, (60000, 65535, 100, 0), (3, 5, 30, 31))
        fs = M.FrameStats(torch.from_numpy(S.record(st).copy()), bins, shift)
        for f in ("hist", "cnt", "nsat", "min", "max", "sum"):
            assert np.array_equal(getattr(fs, f).numpy().astype(np.int64), st[f].astype(np.int64)), f
        assert tuple(fs.hist.shape) == (3, 4, bins) and fs.hist.dtype == torch.int32 and fs.sum.dtype == torch.int64
        assert np.array_equal(M.stats_white_balance(fs), M.stats_white_balance(S.helper_input(st, bins, shift)))
        one = M.FrameStats(torch.from_numpy(S.record(st)[1].copy()), bins, shift)
        assert tuple(one.hist.shape) == (4, bins) and tuple(one.sum.shape) == (4,)
        assert M.stats_percentile(one, 0.5) == M.stats_percentile(fs, 0.5)[1]
