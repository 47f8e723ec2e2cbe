"""Defective pixels of mosaics (mcraw_fixpix_batch) without a GPU: the ABI's symbol and struct, properties of the numpy
statement of the contract (_fixpix_ref) on every geometry the GPU tests use, that statement against a scalar one written
straight from the header, the detection of injected defects in a natural image, and the host helper pack_pixels."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _fixpix_ref as F
import _libs as L
import motioncam_decoder_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (H, W): the cases of tests/test_gpu_fixpix.py
GEOMS = ((1, 1), (2, 2), (3, 5), (1, 64), (33, 1), (16, 64), (35, 41), (34, 520), (70, 1002), (2160, 3840))
SMALL = tuple(g for g in GEOMS if g[0] * g[1] <= 35 * 41)


def _pack(pix):
    """(y, x) pairs -> packed entries, in the order given."""
    return np.array([(y << 16) | x for y, x in pix], dtype=np.uint32)


def _detectable(c, size):
    """A pixel whose neighbours along this axis are not itself."""
    return int(F.neighbour(c, 2, size)) != c


def _spots(H, W):
    """Corners, edge middles and the centre."""
    return sorted({(y, x) for y in (0, H // 2, H - 1) for x in (0, W // 2, W - 1)})


def test_fixpix_symbol_exported_and_listed():
    hdr = open(os.path.join(ROOT, "include", "mcraw_hip.h")).read()
    lib = M.load()
    assert re.search(r"\bmcraw_fixpix_batch\s*\(", hdr)
    assert "mcraw_fixpix_batch" in M.ABI_SYMBOLS
    assert hasattr(lib, "mcraw_fixpix_batch")
    assert re.search(r"#define MCRAW_FIXPIX_HOT\s+1u\b", hdr) and M.FIXPIX_HOT == 1 == F.HOT
    assert re.search(r"#define MCRAW_FIXPIX_COLD\s+2u\b", hdr) and M.FIXPIX_COLD == 2 == F.COLD
    assert re.search(r"#define MCRAW_K_COUNT\s+11\b", hdr)
    assert M.RGB_KERNELS == {"krgb_mhc": 9, "krgb_bin2": 10}
    # the search is stated in the header as the kernels and the reference follow it
    assert "list[mid] < key ? lo = mid + 1 : hi = mid" in hdr and "member = lo < nlist && list[lo] == key" in hdr


def test_fixpix_struct_layout():
    assert C.sizeof(M.FixPix) == 56
    names = ("flags", "rank", "rel_thr", "nlist", "black", "abs_thr", "list", "counts", "reserved")
    assert [getattr(M.FixPix, f).offset for f in names] == [0, 4, 8, 12, 16, 24, 32, 40, 48]
    hdr = open(os.path.join(ROOT, "include", "mcraw_hip.h")).read()
    m = re.search(r"\}\s*mcraw_fixpix;\s*/\*\s*sizeof (\d+); rank (\d+), rel_thr (\d+), nlist (\d+), black (\d+), abs_thr (\d+), "
                  r"list (\d+), counts (\d+), reserved (\d+)", hdr)
    assert m and [int(v) for v in m.groups()] == [C.sizeof(M.FixPix)] + [getattr(M.FixPix, f).offset for f in names[1:]]


def test_neighbour_rule():
    for size in (1, 2, 3, 4, 5, 9):
        for c in range(size):
            for d in (-2, 2):
                a, b = c + d, c - d
                want = a if 0 <= a < size else b if 0 <= b < size else c
                assert int(F.neighbour(c, d, size)) == want
    assert F.NEIGHBOURS == ((-2, -2), (-2, 0), (-2, 2), (0, -2), (0, 2), (2, -2), (2, 0), (2, 2))
    assert [(F.NEIGHBOURS[a], F.NEIGHBOURS[b]) for a, b in F.PAIRS] == [((0, -2), (0, 2)), ((-2, 0), (2, 0)), ((-2, -2), (2, 2)),
                                                                          ((-2, 2), (2, -2))]


@pytest.mark.parametrize("geom", GEOMS)
def test_flags_off_without_a_list_is_the_identity(geom):
    H, W = geom
    img = np.random.default_rng(H * 4099 + W).integers(0, 1 << 16, size=(1, H, W), dtype=np.uint16)
    out, counts = F.fixpix(img, 0, 2, 300, (1, 2, 3, 4), (0, 0, 0, 0))
    assert np.array_equal(out, img) and not counts.any()


@pytest.mark.parametrize("geom", GEOMS)
def test_one_defect_in_a_flat_frame_is_restored_and_counted(geom):
    H, W = geom
    black, abs_thr, rel = (64, 64, 64, 64), (96, 97, 98, 99), 26
    flat = 1000
    big = H * W > 1 << 20  # the large frame: two corners and the centre, the first check alone (the rule knows no size)
    for rank in (1, 2):
        for (y, x) in ((0, 0), (H // 2, W // 2), (H - 1, W - 1)) if big else _spots(H, W):
            thr = abs_thr[(y & 1) * 2 + (x & 1)] + (((flat - 64) * rel) >> 8)
            for sign, bit, row in ((1, F.HOT, 0), (-1, F.COLD, 1)):
                img = np.full((1, H, W), flat, np.uint16)
                img[0, y, x] = flat + sign * (thr + 1)
                out, counts = F.fixpix(img, F.HOT | F.COLD, rank, rel, black, abs_thr)
                want = np.zeros((2, 4), np.uint32)
                if _detectable(y, H) and _detectable(x, W):
                    assert (out == flat).all(), (rank, y, x, sign)
                    want[row, (y & 1) * 2 + (x & 1)] = 1
                else:  # the centre is among its own neighbours: defined behaviour
                    assert np.array_equal(out, img), (rank, y, x, sign)
                assert np.array_equal(counts[0], want), (rank, y, x, sign)
                if big:
                    continue
                # the other flag alone does not see it
                out, counts = F.fixpix(img, bit ^ (F.HOT | F.COLD), rank, rel, black, abs_thr)
                assert np.array_equal(out, img) and not counts.any()
                # moved by exactly thr: kept
                img[0, y, x] = flat + sign * thr
                out, counts = F.fixpix(img, F.HOT | F.COLD, rank, rel, black, abs_thr)
                assert np.array_equal(out, img) and not counts.any()


@pytest.mark.parametrize("geom", GEOMS)
def test_two_adjacent_defects_need_rank_2(geom):
    H, W = geom
    for dy, dx in ((0, 2), (2, 0), (2, 2)):
        y, x = H // 2, W // 2
        # both pixels with eight distinct neighbours
        if min(y, x) < 2 or y + dy + 2 >= H or x + dx + 2 >= W:
            continue
        img = np.full((1, H, W), 500, np.uint16)
        img[0, y, x] = img[0, y + dy, x + dx] = 3000
        out, counts = F.fixpix(img, F.HOT, 2, 0, (0,) * 4, (100,) * 4)
        assert (out == 500).all() and counts.sum() == 2
        out, counts = F.fixpix(img, F.HOT, 1, 0, (0,) * 4, (100,) * 4)
        assert np.array_equal(out, img) and not counts.any()
    # a line one pixel wide is kept at either rank
    if H >= 5 and W >= 5:
        img = np.full((1, H, W), 500, np.uint16)
        img[0, H // 2, :] = 3000
        for rank in (1, 2):
            out, counts = F.fixpix(img, F.HOT | F.COLD, rank, 0, (0,) * 4, (100,) * 4)
            assert np.array_equal(out, img) and not counts.any()


@pytest.mark.parametrize("geom", GEOMS)
def test_list_properties(geom):
    H, W = geom
    rng = np.random.default_rng(H * 31 + W)
    img = rng.integers(0, 1 << 16, size=(1, H, W), dtype=np.uint16)
    args = (F.HOT | F.COLD, 2, 40, (10, 20, 30, 40), (500, 600, 700, 800))
    plain, pcounts = F.fixpix(img, *args)
    # a listed pixel whose eight neighbours are all listed is left as the dynamic pass made it
    y, x = H // 2, W // 2
    ring = {(int(F.neighbour(y, dy, H)) if dy else y, int(F.neighbour(x, dx, W)) if dx else x) for dy, dx in F.NEIGHBOURS}
    ring.discard((y, x))
    out, _ = F.fixpix(img, *args, lst=_pack(sorted(ring | {(y, x)})))
    assert out[0, y, x] == plain[0, y, x]
    # a listed corner takes the (W, E) reflection: both members are the pixel two to the right, a difference of 0
    out, counts = F.fixpix(img, *args, lst=_pack([(0, 0)]))
    if W > 2:
        assert out[0, 0, 0] == img[0, 0, 2]
    else:  # W and E are the corner itself, which is listed; the vertical pair if there is one, else nothing
        assert out[0, 0, 0] == (img[0, 2, 0] if H > 2 else plain[0, 0, 0])
    changed = np.argwhere(out != plain)
    assert all(tuple(c[1:]) == (0, 0) for c in changed)
    # entries outside the frame are skipped
    outside = [(H, 0), (0, W), (H, W), (65535, 65535), (H + 7, W // 2), (H // 2, 65535)]
    outside = [(a, b) for a, b in outside if a <= 65535 and b <= 65535]
    out, counts = F.fixpix(img, *args, lst=_pack(sorted(outside)))
    assert np.array_equal(out, plain) and np.array_equal(counts, pcounts)
    inside = [(H - 1, W - 1)]
    a, _ = F.fixpix(img, *args, lst=_pack(sorted(inside + outside)))
    b, _ = F.fixpix(img, *args, lst=_pack(inside))
    assert np.array_equal(a, b)
    # listed pixels are not counted
    fy, fx = np.nonzero(plain[0] != img[0])
    if len(fy):
        out, counts = F.fixpix(img, *args, lst=_pack([(int(fy[0]), int(fx[0]))]))
        assert counts.sum() == pcounts.sum() - 1


def _scalar_member(lst, key):
    lo, hi = 0, len(lst)
    while lo < hi:
        mid = (lo + hi) >> 1
        if lst[mid] < key:
            lo = mid + 1
        else:
            hi = mid
    return lo < len(lst) and lst[lo] == key


def _scalar(img, flags, rank, rel, black, abs_thr, lst):
    """The header, pixel by pixel, in plain Python."""
    H, W = img.shape
    v = img.astype(int).tolist()
    lst = [int(e) for e in lst]
    out = [row[:] for row in v]
    counts = [[0] * 4, [0] * 4]

    def nbs(y, x):
        res = []
        for dy, dx in ((-2, -2), (-2, 0), (-2, 2), (0, -2), (0, 2), (2, -2), (2, 0), (2, 2)):
            yy, xx = y, x
            if dy:
                yy = y + dy if 0 <= y + dy < H else y - dy if 0 <= y - dy < H else y
            if dx:
                xx = x + dx if 0 <= x + dx < W else x - dx if 0 <= x - dx < W else x
            res.append((yy, xx))
        return res

    def choose(cands):
        best = None
        for a, b in cands:
            if best is None or abs(a - b) < best[0]:
                best = (abs(a - b), (a + b + 1) >> 1)
        return None if best is None else best[1]

    order = ((3, 4), (1, 6), (0, 7), (2, 5))
    for y in range(H):
        for x in range(W):
            p = (y & 1) * 2 + (x & 1)
            nb = nbs(y, x)
            vals = sorted(v[a][b] for a, b in nb)
            Hk, Lk = vals[8 - rank], vals[rank - 1]
            thr = lambda m: abs_thr[p] + ((max(m - black[p], 0) * rel) >> 8)
            hot = bool(flags & 1) and v[y][x] > Hk and v[y][x] - Hk > thr(Hk)
            cold = bool(flags & 2) and v[y][x] < Lk and Lk - v[y][x] > thr(Lk)
            if hot or cold:
                out[y][x] = choose([(v[nb[a][0]][nb[a][1]], v[nb[b][0]][nb[b][1]]) for a, b in order])
                if not _scalar_member(lst, (y << 16) | x):
                    counts[1 if cold else 0][p] += 1
    for e in lst:
        y, x = e >> 16, e & 0xFFFF
        if x >= W or y >= H:
            continue
        nb = nbs(y, x)
        free = [not _scalar_member(lst, (a << 16) | b) for a, b in nb]
        r = choose([(v[nb[a][0]][nb[a][1]], v[nb[b][0]][nb[b][1]]) for a, b in order if free[a] and free[b]])
        if r is not None:
            out[y][x] = r
    return np.array(out, np.uint16), np.array(counts, np.uint32)


@pytest.mark.parametrize("geom", SMALL)
def test_reference_equals_the_scalar_statement(geom):
    H, W = geom
    rng = np.random.default_rng(H * 977 + W)
    for k in range(4):
        img = rng.integers(0, 1 << (16 if k & 1 else 10), size=(H, W), dtype=np.uint16)
        flags, rank = (3, 1, 2, 3)[k], 1 + (k & 1)
        rel, black, abs_thr = (0, 26, 65535, 300)[k], ((0,) * 4, (64, 65, 66, 67), (0, 1, 2, 3), (60000, 5, 9, 100))[k], \
            ((0,) * 4, (96, 97, 98, 99), (0,) * 4, (7, 6, 5, 4))[k]
        K = max(1, H * W // 6)
        pix = np.stack([rng.integers(0, H + 2, K), rng.integers(0, W + 2, K)], axis=1)  # some outside, some twice
        for lst in (np.zeros(0, np.uint32), np.sort(_pack(pix.tolist())), _pack(pix.tolist())):  # none, ascending, unsorted
            got, gc = F.fixpix(img[None], flags, rank, rel, black, abs_thr, lst)
            want, wc = _scalar(img, flags, rank, rel, black, abs_thr, lst)
            assert np.array_equal(got[0], want), (k, len(lst))
            assert np.array_equal(gc[0], wc), (k, len(lst))


def test_unsorted_list_gives_what_the_stated_search_gives():
    rng = np.random.default_rng(5)
    lst = rng.integers(0, 64, size=37).astype(np.uint32)  # not ascending, with duplicates
    keys = np.arange(0, 70)
    got = F.member(lst, keys)
    want = [_scalar_member([int(e) for e in lst], int(k)) for k in keys]
    assert got.tolist() == want
    assert got.sum() < len(set(lst.tolist()))  # the search misses entries that are there: still one defined result
    srt = np.sort(lst)
    assert F.member(srt, keys).tolist() == [int(k) in set(lst.tolist()) for k in keys]
    assert not F.member(np.zeros(0, np.uint32), keys).any()


def test_extreme_products_stay_below_2_to_32():
    img = np.zeros((1, 9, 9), np.uint16)
    img[0, ::2, ::2] = 65535
    img[0, 4, 4] = 0
    peak = []
    out, counts = F.fixpix(img, F.HOT | F.COLD, 1, 65535, (0,) * 4, (65535,) * 4, peak=peak)
    assert max(peak) == 65535 * 65535 < 1 << 32 and 65535 + ((65535 * 65535) >> 8) < 1 << 32
    assert np.array_equal(out, img)  # 65535 below its neighbours is within such a threshold
    out, counts = F.fixpix(img, F.COLD, 1, 0, (0,) * 4, (65534,) * 4)
    assert out[0, 4, 4] == 65535 and counts[0, 1, 0] == 1 and counts.sum() == 1


def test_flagged_share_on_noise():
    """All thresholds 0: a pixel is flagged when it is above the rank-th largest or below the rank-th smallest of nine
    exchangeable values, 2 / 9 at rank 1 and 4 / 9 at rank 2 but for ties and the reflected edges."""
    img = L.uniform_image_np(1002, 70, 12, 3)[None]
    for rank, share in ((1, 2 / 9), (2, 4 / 9)):
        out, counts = F.fixpix(img, F.HOT | F.COLD, rank, 0, (0,) * 4, (0,) * 4)
        got = counts.sum() / img.size
        assert abs(got - share) <= 0.02, (rank, got)
        assert counts.sum() >= (out != img).sum()


def test_injected_defects_in_a_natural_image_are_found_and_nothing_else():
    W, H, sigma = 1002, 70, 12.0
    clean = L.natural_image_np(W, H, 12, sigma, 7)
    black, abs_thr, rel = (64,) * 4, (96,) * 4, 26
    ys, xs = np.arange(3, H - 3, 7), np.arange(3, W - 3, 9)
    yy, xx = np.meshgrid(ys, xs, indexing="ij")
    assert yy.size == 1110
    bad = clean.astype(np.int64)
    bad[yy, xx] = np.clip(bad[yy, xx] + np.where((yy + xx) & 1, 600, -600), 0, 4095)
    bad = bad.astype(np.uint16)
    assert (np.abs(bad[yy, xx].astype(int) - clean[yy, xx].astype(int)) >= 400).all()
    mask = np.zeros((H, W), bool)
    mask[yy, xx] = True
    # a replacement is the mean of two clean samples 2 pixels either side of the defect: against the clean sample there the
    # smooth field's second difference is below 1474 * (2 / 211 + 2 / 173) ** 2 / 2 < 1, the noise is (na + nb) / 2 - n0
    # with a deviation of sigma * sqrt(1.5), and each rounding adds at most 1: 6 deviations and 2
    bound = int(6 * sigma * np.sqrt(1.5) + 2)
    assert bound == 90
    for rank in (1, 2):
        out, counts = F.fixpix(bad[None], F.HOT | F.COLD, rank, rel, black, abs_thr)
        assert (out[0][mask] != bad[mask]).all(), rank          # every injected pixel is replaced
        assert np.array_equal(out[0][~mask], bad[~mask]), rank  # no other pixel changes
        assert counts.sum() == 1110
        err = np.abs(out[0][mask].astype(int) - clean[mask].astype(int)).max()
        assert err <= bound, (rank, err)
        same, c0 = F.fixpix(clean[None], F.HOT | F.COLD, rank, rel, black, abs_thr)
        assert np.array_equal(same[0], clean) and not c0.any(), rank  # the clean image changes nowhere


def test_pack_pixels():
    got = M.pack_pixels(np.array([[5, 1], [3, 1], [5, 1], [0, 0], [65535, 65535], [7, 0]]))
    assert got.dtype == np.uint32 and got.flags["C_CONTIGUOUS"]
    assert got.tolist() == [0, 7, (1 << 16) | 3, (1 << 16) | 5, 0xFFFFFFFF]  # y << 16 | x, ascending, the duplicate gone
    assert M.pack_pixels([(2, 3)]).tolist() == [(3 << 16) | 2]
    assert M.pack_pixels(np.zeros((0, 2), np.int64)).tolist() == [] and M.pack_pixels([]).tolist() == []
    for a in (np.zeros((3, 3), np.int32), np.zeros(4, np.int32), np.zeros((2, 2, 2), np.int32)):
        with pytest.raises(ValueError):
            M.pack_pixels(a)
    with pytest.raises(ValueError):
        M.pack_pixels(np.array([[1.0, 2.0]]))
    with pytest.raises(ValueError):
        M.pack_pixels(np.array([[-1, 2]]))
    with pytest.raises(ValueError):
        M.pack_pixels(np.array([[1, 65536]]))
    many = np.stack(np.meshgrid(np.arange(1025), np.arange(1024)), axis=-1).reshape(-1, 2)
    with pytest.raises(ValueError):
        M.pack_pixels(many)  # 1025 * 1024 pixels: above 1 << 20
    assert M.pack_pixels(many[:1 << 20]).size == 1 << 20
    # what the list means to the reference: the packed pixels are the listed ones
    lst = M.pack_pixels(np.array([[2, 1], [0, 0]]))
    assert F.member(lst, np.array([(1 << 16) | 2, 0, 1])).tolist() == [True, True, False]
