"""CPU: the numpy statement of the noise measurement's contract (tests/_noise_ref.py) against a scalar reading of
include/mcraw_hip.h, and the properties the contract claims: the energy bins at every edge, the largest T, T = 0 on a linear ramp,
the level bin's clamp, rejection by sat and lo, and that nothing outside the window's whole blocks is read."""
import numpy as np
import pytest

import _noise_ref as NR
import motioncam_decoder_amd as M


def _scalar(frames, shift, sat, lo, roi=None):
    """The contract, sample by sample, with Python integers."""
    n, H, W = frames.shape
    y0, x0, h, w = (0, 0, H, W) if roi is None else roi
    hist, nblk, nrej = np.zeros((n, 4, 32, 128), np.uint32), np.zeros((n, 4), np.uint32), np.zeros((n, 4), np.uint32)
    for f in range(n):
        for j in range(h // 16):
            for i in range(w // 16):
                for p in range(4):
                    b = [[int(frames[f, y0 + 16 * j + 2 * r + (p >> 1), x0 + 16 * i + 2 * c + (p & 1)]) for c in range(8)] for r in range(8)]
                    s = sum(sum(row) for row in b)
                    T = sum((b[r][c - 1] - 2 * b[r][c] + b[r][c + 1]) ** 2 for r in range(8) for c in range(1, 7))
                    T += sum((b[r - 1][c] - 2 * b[r][c] + b[r + 1][c]) ** 2 for r in range(1, 7) for c in range(8))
                    if any(v >= sat[p] or v < lo[p] for row in b for v in row):
                        nrej[f, p] += 1
                        continue
                    if T < 16:
                        vb = 0
                    else:
                        e = T.bit_length() - 1
                        vb = min(4 * (e - 4) + ((T >> (e - 2)) & 3) + 1, 127)
                    hist[f, p, min((s >> 6) >> shift, 31), vb] += 1
                    nblk[f, p] += 1
    return dict(hist=hist, nblk=nblk, nrej=nrej)


def _equal(a, b):
    return all(np.array_equal(a[k], b[k]) for k in ("hist", "nblk", "nrej"))


@pytest.mark.parametrize("seed", (0, 1))
def test_statement_equals_the_scalar_reading(seed):
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 1 << 16, size=(2, 48, 80), dtype=np.uint16)
    frames[1] = 800 + (frames[1] >> 10)  # a quiet 10-bit frame next to a 16-bit one: low and high energy bins
    sat, lo = (65535, 60000, 865, 65000), (0, 100, 1, 801)
    for shift, roi in ((11, None), (5, None), (7, (2, 6, 45, 70))):
        got, want = NR.noise_stats(frames, shift, sat, lo, roi), _scalar(frames, shift, sat, lo, roi)
        assert _equal(got, want), (shift, roi)
        assert int(got["nblk"].sum()) > 0 and int(got["nrej"].sum()) > 0
    rec = NR.record(NR.noise_stats(frames, 11, sat, lo))
    assert rec.shape == (2, 65568) and rec.dtype == np.uint8
    assert np.array_equal(rec.view("<u4")[:, 16384:16388], NR.noise_stats(frames, 11, sat, lo)["nblk"])


def test_energy_bins_at_every_edge():
    lib = M.load()
    assert [int(v) for v in NR.energy_bin([0, 15, 16])] == [0, 0, 1]
    for e in range(4, 43):
        for f in range(4):
            edge, vb = NR.edge(e, f), 4 * (e - 4) + f + 1
            assert edge == 2 ** e * (4 + f) // 4
            got = [int(v) for v in NR.energy_bin([edge - 1, edge])]
            assert got == [min(vb - 1, 127), min(vb, 127)], (e, f, got)
            # the library's exported formula (the kernel's) and the one noise_fit simulates with agree
            assert [lib.mcraw_noise_energy_bin(edge - 1), lib.mcraw_noise_energy_bin(edge)] == got
            assert [int(v) for v in M._noise_energy_bin(np.array([edge - 1, edge]))] == got
            if 1 <= vb <= 127:
                assert M._noise_edge(vb) == float(edge)


def test_largest_energy_and_a_linear_ramp():
    r, c = np.mgrid[0:8, 0:8]
    worst = (((r + c) & 1) * 65535).astype(np.int64)
    s, T = NR.sums(worst[None])
    assert int(T[0]) == 96 * (2 * 65535) ** 2 < 2 ** 43 and int(NR.energy_bin(T)[0]) == 127 and int(s[0]) == 32 * 65535 < 2 ** 22
    assert int(M._noise_energy(worst[None])[0]) == int(T[0])
    for ramp in (100 + 7 * r + 13 * c, 65535 - 4681 * r - 4681 * c, 5 * c, np.full((8, 8), 4095)):
        assert int(NR.sums(ramp[None].astype(np.int64))[1][0]) == 0
    # as frames: the alternating extreme in every plane lands in the last energy bin, a ramp over the frame in the first
    yy, xx = np.mgrid[0:32, 0:48]
    ext = ((((yy >> 1) + (xx >> 1)) & 1) * 65534).astype(np.uint16)[None]
    d = NR.noise_stats(ext, 11)
    assert int(d["hist"][..., 127].sum()) == 4 * 6 == int(d["nblk"].sum())
    d = NR.noise_stats((3 * yy + 5 * xx + 17).astype(np.uint16)[None], 4)
    assert int(d["hist"][..., 0].sum()) == 4 * 6


def test_level_bin_clamp():
    for value, shift, want in ((4095, 7, 31), (3967, 7, 30), (4096, 7, 31), (65535, 7, 31), (65535, 11, 31), (65535, 15, 1), (127, 7, 0),
                               (128, 7, 1), (31, 0, 31), (32, 0, 31), (30, 0, 30)):
        d = NR.noise_stats(np.full((1, 16, 16), value, np.uint16), shift, sat=65536)
        assert (d["hist"][0, :, want, 0] == 1).all() and int(d["hist"].sum()) == 4, (value, shift)
    # the mean's fraction is dropped: 63 samples of 128 and one of 127 sum to 64 * 128 - 1
    img = np.full((1, 16, 16), 128, np.uint16)
    img[0, 0, 0] = 127
    d = NR.noise_stats(img, 7)
    assert int(d["hist"][0, 0, 0].sum()) == 1 and int(d["hist"][0, 1:, 1].sum()) == 3


def test_rejection_by_sat_and_lo():
    rng = np.random.default_rng(2)
    img = rng.integers(200, 300, size=(1, 32, 32), dtype=np.uint16)
    assert int(NR.noise_stats(img, 4)["nrej"].sum()) == 0
    img[0, 16 + 5, 2] = 1000   # block (1, 0), position 2
    img[0, 2, 16 + 9] = 150    # block (0, 1), position 1
    d = NR.noise_stats(img, 4, sat=1000, lo=151)
    assert d["nrej"].tolist() == [[0, 1, 1, 0]] and d["nblk"].tolist() == [[4, 3, 3, 4]]
    d = NR.noise_stats(img, 4, sat=1001, lo=150)  # sat is the first rejected value, lo the first accepted one
    assert int(d["nrej"].sum()) == 0
    d = NR.noise_stats(img, 4, sat=(1001, 1001, 0, 1001), lo=0)  # sat = 0 rejects everything of its position
    assert d["nrej"].tolist() == [[0, 0, 4, 0]] and int(d["hist"][0, 2].sum()) == 0
    d = NR.noise_stats(img, 4, sat=65535, lo=(0, 0, 0, 65535))
    assert d["nrej"].tolist() == [[0, 0, 0, 4]]


def test_partial_blocks_are_not_read():
    rng = np.random.default_rng(3)
    H, W, roi = 60, 90, (4, 6, 50, 75)  # 3 x 4 whole blocks; 2 rows and 11 columns of the window belong to none
    img = rng.integers(0, 4096, size=(2, H, W), dtype=np.uint16)
    want = NR.noise_stats(img, 7, 4095, 1, roi)
    poisoned = np.full_like(img, 65535)
    poisoned[:, 4:4 + 48, 6:6 + 64] = img[:, 4:4 + 48, 6:6 + 64]
    got = NR.noise_stats(poisoned, 7, 4095, 1, roi)
    assert _equal(got, want) and _equal(got, _scalar(poisoned, 7, (4095,) * 4, (1,) * 4, roi))
    assert int((want["nblk"] + want["nrej"]).sum()) == 2 * 4 * 12
