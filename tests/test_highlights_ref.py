"""Highlight reconstruction (mcraw_highlights_batch / mcraw_highlights_measure_batch) without a GPU: the numpy statement of the
contract (_highlights_ref) against a scalar one written straight from the header, its properties, the defect it cures shown
through the display statement, how well it rebuilds a grey ramp and a coloured patch, and the Python helpers."""
import numpy as np
import pytest

import _display_ref as D
import _highlights_ref as HL
import motioncam_decoder_amd as M

GEOMS = ((2, 2), (2, 3), (3, 2), (5, 7), (12, 10))
# the issue's example: every colour of a real camera-to-sRGB matrix has negative off-diagonal terms
BLACK, WHITE, GAIN = 64, 4095, (2.0, 1.0, 1.6)
MATRIX = np.array([[1.6, -0.4, -0.2], [-0.2, 1.4, -0.2], [0.0, -0.5, 1.5]], np.float32)


def _scalar(img, mode, sat, black, gain, cfa, rec, top, lo):
    """The header, pixel by pixel, in plain Python: (out, sum[4], cnt[4]) of one frame; rec: (sum[4], cnt[4]) or None."""
    H, W = img.shape
    s = img.astype(int).tolist()
    inv = [((1 << 24) + g // 2) // g for g in gain]
    pos = lambda y, x: (y & 1) * 2 + (x & 1)
    refl = lambda c, n: 1 if c == -1 else n - 2 if c == n else c

    def v(y, x):
        q = pos(y, x)
        return (max(s[y][x] - black[q], 0) * gain[q] + 2048) >> 12

    def ref(y, x):
        nb = lambda dy, dx: v(refl(y + dy, H), refl(x + dx, W))
        Hm = (nb(0, -1) + nb(0, 1) + 1) >> 1
        Vm = (nb(-1, 0) + nb(1, 0) + 1) >> 1
        Dm = (nb(-1, -1) + nb(-1, 1) + nb(1, -1) + nb(1, 1) + 2) >> 2
        green = pos(y, x) in ((1, 2) if cfa < 2 else (0, 3))
        return (Hm + Vm + 1) >> 1 if green else (((Hm + Vm + 1) >> 1) + Dm + 1) >> 1

    m = min(((sat[p] - black[p]) * gain[p] + 2048) >> 12 for p in range(4))
    cap = [black[p] + ((m * inv[p] + 2048) >> 12) for p in range(4)]
    chroma = [0] * 4
    if rec is not None:
        for p in range(4):
            sm, c = int(rec[0][p]), int(rec[1][p])
            q = 0 if c == 0 else (abs(sm) // c if sm >= 0 else -(abs(sm) // c))  # C's division truncates towards zero
            chroma[p] = min(max(q, -(1 << 20)), 1 << 20)
    out = [row[:] for row in s]
    sums, cnts = [0] * 4, [0] * 4
    for y in range(H):
        for x in range(W):
            p = pos(y, x)
            if lo[p] <= s[y][x] < sat[p] and all(
                    s[refl(y + dy, H)][refl(x + dx, W)] < sat[pos(refl(y + dy, H), refl(x + dx, W))]
                    for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dy or dx):
                sums[p] += v(y, x) - ref(y, x)
                cnts[p] += 1
            if mode == HL.CLIP:
                out[y][x] = min(s[y][x], cap[p])
            elif s[y][x] >= sat[p]:
                cand = ref(y, x) + chroma[p]
                if cand > v(y, x):
                    out[y][x] = max(s[y][x], min(black[p] + ((cand * inv[p] + 2048) >> 12), top))
    return np.array(out, np.uint16), sums, cnts


def _content(rng, H, W, sat, third=True):
    """Random samples, about a third of them at or above their sat."""
    satm = HL.by_position(sat, H, W)
    img = np.minimum(rng.integers(0, 4000, size=(H, W)), satm - 1)
    if third:
        img = np.where(rng.random((H, W)) < 1 / 3, satm + rng.integers(0, 3, size=(H, W)) * 50, img)
    return np.clip(img, 0, 65535).astype(np.uint16)


@pytest.mark.parametrize("geom", GEOMS)
@pytest.mark.parametrize("cfa", (0, 1, 2, 3))
def test_reference_equals_the_scalar_statement(geom, cfa):
    H, W = geom
    rng = np.random.default_rng(H * 101 + W * 7 + cfa)
    for k in range(6):
        gain = [int(g) for g in rng.integers(256, 65536, size=4)] if k else [256, 65535, 4096, 8192]
        black = [int(b) for b in rng.integers(0, 300, size=4)]
        sat = [int(b) + int(d) for b, d in zip(black, rng.integers(1, 3700, size=4))]
        lo = HL.default_lo(sat, black) if k & 1 else [int(b) for b in black]
        top = (65535, 4500, 1, 20000)[k % 4]
        img = _content(rng, H, W, sat)
        rec = None if k == 0 else (rng.integers(-4000, 4000, size=(1, 4)) * (1 if k < 4 else 1 << 30), rng.integers(0, 3, size=(1, 4)).astype(np.uint32))
        sums, cnts = HL.measure(img[None], sat, black, gain, cfa, lo)
        for mode in (HL.REBUILD, HL.CLIP):
            got = HL.apply(img[None], mode, sat, black, gain, cfa, rec, top)[0]
            want, ws, wc = _scalar(img, mode, sat, black, gain, cfa, None if rec is None else (rec[0][0], rec[1][0]), top, lo)
            assert np.array_equal(got, want), (k, mode)
            assert sums[0].tolist() == ws and cnts[0].tolist() == wc, (k, mode)


def test_records_layout_and_division():
    sums = np.array([[-7, 7, -(1 << 62), 5]], np.int64)
    cnts = np.array([[2, 2, 3, 0]], np.uint32)
    assert HL.chroma(sums, cnts).tolist() == [[-3, 3, -(1 << 20), 0]]  # towards zero, clamped, 0 without a count
    r = HL.raw(sums, cnts)
    assert r.shape == (1, 8) and r.dtype == np.int64 and r[0, :4].tolist() == sums[0].tolist()
    assert r[0, 4] == 2 | (2 << 32) and r[0, 5] == 3 and r[0, 6] == 0 and r[0, 7] == 0


@pytest.mark.parametrize("geom", GEOMS + ((33, 41),))
def test_rebuild_properties(geom):
    H, W = geom
    rng = np.random.default_rng(H + 1000 * W)
    sat, black, gain = [3000, 3100, 2900, 3050], [60, 64, 68, 72], M.highlight_gains(GAIN, "grbg")
    img = _content(rng, 3 * H, W, sat).reshape(3, H, W)
    rec = HL.measure(img, sat, black, gain, 2, HL.default_lo(sat, black))
    for r in (None, rec, (np.full((1, 4), 1 << 40), np.ones((1, 4), np.uint32)), (np.full((1, 4), -(1 << 40)), np.ones((1, 4), np.uint32))):
        out = HL.apply(img, HL.REBUILD, sat, black, gain, 2, r, 65535)
        assert (out >= img).all()  # no sample is lowered
        unclipped = img < HL.by_position(sat, H, W)
        assert np.array_equal(out[unclipped], img[unclipped])  # unclipped samples never change
        assert (HL.apply(img, HL.REBUILD, sat, black, gain, 2, r, 3500) <= np.maximum(img, 3500)).all()  # top cuts what is written
    clean = _content(rng, H, W, sat, third=False)[None]
    assert (clean < HL.by_position(sat, H, W)).all()
    assert np.array_equal(HL.apply(clean, HL.REBUILD, sat, black, gain, 2, (np.full((1, 4), 1 << 40), np.ones((1, 4), np.uint32))), clean)


@pytest.mark.parametrize("geom", GEOMS + ((33, 41),))
def test_clip_properties(geom):
    H, W = geom
    rng = np.random.default_rng(H * 3 + W)
    sat, black = [3000, 3100, 2900, 3050], [60, 64, 68, 72]
    for cfa in ("rggb", "gbrg"):
        gain = M.highlight_gains((1.9, 1.0, 1.45), cfa)
        img = _content(rng, H, W, sat)[None]
        out = HL.apply(img, HL.CLIP, sat, black, gain, HL.CFA[cfa])
        assert (out <= img).all()  # no sample is raised
        m, cap = HL.caps(sat, black, gain)
        vs = [((sat[p] - black[p]) * gain[p] + 2048) >> 12 for p in range(4)]
        p = vs.index(m)  # the position that attains m keeps every sample below sat
        below = img[0, p >> 1::2, p & 1::2] < sat[p]
        assert np.array_equal(out[0, p >> 1::2, p & 1::2][below], img[0, p >> 1::2, p & 1::2][below])
        # ... and a blown frame comes out neutral: every position at the same white-balanced level, but for the roundings
        blown = HL.by_position(sat, H, W).astype(np.uint16)[None]
        v = HL.wb(HL.apply(blown, HL.CLIP, sat, black, gain, HL.CFA[cfa]), black, gain)
        assert int(v.max()) - int(v.min()) <= 1 + max(gain) // 4096 and abs(int(v.min()) - m) <= 1 + max(gain) // 4096


def test_measure_properties():
    rng = np.random.default_rng(8)
    H, W = 12, 10
    sat, black, gain = [3000] * 4, [64] * 4, [8192, 4096, 4096, 6554]
    lo = HL.default_lo(sat, black)
    blown = np.full((1, H, W), 3000, np.uint16)
    s, c = HL.measure(blown, sat, black, gain, 0, lo)
    assert not c.any() and not s.any()  # nothing takes part on a blown frame
    a, b = _content(rng, H, W, sat)[None], _content(rng, H, W, sat)[None]
    ra, rb = HL.measure(a, sat, black, gain, 0, lo), HL.measure(b, sat, black, gain, 0, lo)
    both = HL.measure(b, sat, black, gain, 0, lo, into=ra)  # accumulating two frames into one record: the sum of their records
    assert np.array_equal(both[0], ra[0] + rb[0]) and np.array_equal(both[1], ra[1] + rb[1])
    one = HL.measure(np.concatenate([a, b]), sat, black, gain, 0, lo, nrec=1)
    assert np.array_equal(one[0], both[0]) and np.array_equal(one[1], both[1])
    per = HL.measure(np.concatenate([a, b]), sat, black, gain, 0, lo)
    assert np.array_equal(per[0], np.concatenate([ra[0], rb[0]])) and np.array_equal(per[1], np.concatenate([ra[1], rb[1]]))
    # a single clipped sample takes itself and its eight neighbours out
    flat = np.full((1, H, W), 2000, np.uint16)
    full = HL.measure(flat, sat, black, gain, 0, lo)[1].sum()
    flat[0, 5, 5] = 3000
    assert full == H * W and HL.measure(flat, sat, black, gain, 0, lo)[1].sum() == H * W - 9


def _display(img):
    lut = M.transfer_lut("srgb", 4096, 8)
    return D.display_ref(img, "mhc", float(WHITE), lut, "u8", "hwc", (BLACK,) * 4, "rggb", GAIN, MATRIX)


def test_the_motivating_case():
    """A blown frame turns magenta in the colour stage; behind either mode it is white."""
    img = np.full((16, 16), WHITE, np.uint16)
    raw = _display(img)
    assert (raw == np.array([255, 215, 255], np.uint8)).all()
    assert int(raw[0, 0, 1]) < int(raw[0, 0, 0])  # G < R: the defect
    gain = M.highlight_gains(GAIN, "rggb")
    assert gain == [8192, 4096, 4096, 6554]
    reb = HL.apply(img[None], HL.REBUILD, [WHITE] * 4, [BLACK] * 4, gain, 0, None)[0]
    assert sorted(set(reb.ravel().tolist())) == [4095, 7320]
    assert (reb[0::2, 0::2] == 4095).all() and (reb[1::2, 1::2] == 4095).all() and (reb[0::2, 1::2] == 7320).all() and (reb[1::2, 0::2] == 7320).all()
    assert (_display(reb) == 255).all()
    assert HL.caps([WHITE] * 4, [BLACK] * 4, gain) == (4031, [2080, 4095, 4095, 2583])
    clp = HL.apply(img[None], HL.CLIP, [WHITE] * 4, [BLACK] * 4, gain, 0)[0]
    assert (_display(clp) == 255).all()


def _sensor(wbv, gain, black=BLACK, white=WHITE):
    """What a sensor that clips at `white` records of white-balanced values (H, W) at RGGB positions: (recorded, unclipped truth)."""
    H, W = wbv.shape
    truth = np.rint(black + wbv * 4096.0 / HL.by_position(gain, H, W)).astype(np.int64)
    return np.minimum(truth, white).astype(np.uint16), truth


def test_grey_ramp():
    """Condition 1: the largest error of the rebuilt samples is below one column step of the ramp (the reference is a mean of
    neighbours one column away, plus the roundings); measured here: 31 levels against a step of 63.6.  Condition 2: the
    chroma measured on grey is 0 at every position; measured here: sums of 0, -96, -128, -96 over 0, 480, 512, 192 samples."""
    H, W = 64, 96
    gain = M.highlight_gains(GAIN, "rggb")
    ramp = np.tile(1.5 * (WHITE - BLACK) * np.arange(W) / (W - 1), (H, 1))
    img, truth = _sensor(ramp, gain)
    clipped = img >= WHITE
    assert clipped[0::2, 1::2].any() and not clipped[0::2, 0::2].any() and not clipped[1::2, 1::2].any()  # only green clips
    sat, black = [WHITE] * 4, [BLACK] * 4
    rec = HL.measure(img[None], sat, black, gain, 0, HL.default_lo(sat, black))
    ch = HL.chroma(*rec)
    print("grey ramp: sums", rec[0].tolist(), "counts", rec[1].tolist(), "chroma", ch.tolist())
    out = HL.apply(img[None], HL.REBUILD, sat, black, gain, 0, rec)[0]
    err = int(np.abs(out.astype(np.int64) - truth)[clipped].max())
    step = 1.5 * (WHITE - BLACK) / (W - 1)
    print("grey ramp: largest error %d, one column step %.1f" % (err, step))
    assert err < step
    assert not ch.any()


def test_coloured_patch():
    """A patch of one colour, half below and half above green's clip level: the colour measured on the unclipped half makes
    the rebuilt half better than the neighbours' mean alone, which is better than nothing.  Largest error over the clipped
    samples, in raw levels (DESIGN.md 31 has the three values)."""
    H, W = 64, 96
    gain = M.highlight_gains(GAIN, "rggb")
    level = np.where(np.arange(W) < W // 2, 0.9, 1.4) * (WHITE - BLACK)
    # white-balanced (1.2, 1.0, 0.7) at the RGGB positions
    colour = np.where(HL.by_position((0, 1, 1, 0), H, W) == 1, 1.0, np.where(HL.by_position((1, 0, 0, 0), H, W) == 1, 1.2, 0.7))
    img, truth = _sensor(colour * level[None, :], gain)
    clipped = img >= WHITE
    assert clipped.any() and not clipped[:, :W // 2].any()
    sat, black = [WHITE] * 4, [BLACK] * 4
    rec = HL.measure(img[None], sat, black, gain, 0, HL.default_lo(sat, black))
    errs = []
    for out in (HL.apply(img[None], HL.REBUILD, sat, black, gain, 0, rec)[0], HL.apply(img[None], HL.REBUILD, sat, black, gain, 0, None)[0], img):
        errs.append(int(np.abs(out.astype(np.int64) - truth)[clipped].max()))
    print("coloured patch: measured chroma %d, zero chroma %d, untreated %d" % tuple(errs))
    assert errs[0] < errs[1] < errs[2]


def test_highlight_gains():
    assert M.highlight_gains((2.0, 1.0, 1.6), "rggb") == [8192, 4096, 4096, 6554]
    assert M.highlight_gains((2.0, 1.0, 1.6), "bggr") == [6554, 4096, 4096, 8192]
    assert M.highlight_gains((2.0, 1.0, 1.6), "grbg") == [4096, 8192, 6554, 4096]
    assert M.highlight_gains((2.0, 1.0, 1.6), "GBRG") == [4096, 6554, 8192, 4096]
    assert M.highlight_gains((1 / 16, 16.0, 1.0)) == [256, 65535, 65535, 4096]
    assert M.highlight_gains(np.array([0.5 / 4096 + 1.0, 1.5 / 4096 + 1.0, 1.0]))[:2] == [4096, 4098]  # rint: ties to even
    for bad in ((1.0, 1.0), (1.0, 1.0, 1.0, 1.0), (0.06, 1, 1), (1, 16.01, 1), (1, 1, float("nan")), (1, float("inf"), 1), (-1, 1, 1)):
        with pytest.raises(ValueError):
            M.highlight_gains(bad)
    with pytest.raises(ValueError):
        M.highlight_gains((1, 1, 1), "xyzw")
    for cfa in ("rggb", "bggr", "grbg", "gbrg"):  # green where the library puts it
        g = M.highlight_gains((2.0, 1.0, 3.0), cfa)
        assert [g[p] == 4096 for p in range(4)] == [HL.green(HL.CFA[cfa], p) for p in range(4)]


def test_keyword_defaults_and_errors():
    kw = M._hl_kwargs("demosaic", {}, 4095.0, (64,) * 4, "grbg", (2.0, 1.0, 1.6))
    assert kw == dict(gain=(2.0, 1.0, 1.6), sat=4095, black=(64,) * 4, cfa="grbg")
    kw = M._hl_kwargs("demosaic", dict(mode="clip", sat=(4000,) * 4, gain=(1.5, 1, 1.5), black=(0,) * 4, cfa="rggb", top=5000, lo=100, chroma=None),
                      4095.0, (64,) * 4, "grbg", np.ones((2, 3)))
    assert kw["sat"] == (4000,) * 4 and kw["gain"] == (1.5, 1, 1.5) and kw["black"] == (0,) * 4 and kw["cfa"] == "rggb" and kw["chroma"] is None
    assert M._hl_kwargs("demosaic", {}, 1023, (0,) * 4, "rggb", None)["gain"] == (1.0, 1.0, 1.0)
    with pytest.raises(ValueError, match="one gain for the batch"):
        M._hl_kwargs("decode_yuv", {}, 4095.0, (64,) * 4, "rggb", np.ones((2, 3)))
    with pytest.raises(ValueError, match="no key 'out'"):
        M._hl_kwargs("demosaic", dict(out=None), 4095.0, (64,) * 4, "rggb", None)
    with pytest.raises(ValueError, match="no key 'strength'"):
        M._hl_kwargs("demosaic", dict(strength=1), 4095.0, (64,) * 4, "rggb", None)
    with pytest.raises(ValueError, match="dict"):
        M._hl_kwargs("demosaic", True, 4095.0, (64,) * 4, "rggb", None)
    with pytest.raises(ValueError, match="integer 'sat'"):
        M._hl_kwargs("demosaic", {}, 4095.5, (64,) * 4, "rggb", None)
    # the struct that the methods build
    s = M._hl_struct("highlights", 4095, 64, (2.0, 1.0, 1.6), "rggb", None, 65535, "rebuild")
    assert (s.mode, s.cfa, s.flags, s.top, s.nrec, s.reserved) == (M.HL_REBUILD, 0, 0, 65535, 0, 0) and not s.rec
    assert list(s.sat) == [4095] * 4 and list(s.black) == [64] * 4 and list(s.gain) == [8192, 4096, 4096, 6554]
    assert list(s.lo) == [64 + 4031 // 2] * 4
    s = M._hl_struct("highlights", (4000, 4001, 4002, 4003), (1, 2, 3, 4), (300, 400, 500, 65535), "gbrg", (9, 8, 7, 6), 1, "clip")
    assert (s.mode, s.cfa, s.top) == (M.HL_CLIP, 3, 1) and list(s.gain) == [300, 400, 500, 65535] and list(s.lo) == [9, 8, 7, 6]
    for bad in (dict(sat=64), dict(sat=(1, 2, 3)), dict(sat=4095.5), dict(sat=70000), dict(black=(64, 64)), dict(gain=None), dict(gain=(1, 1)),
                dict(gain=(255, 4096, 4096, 4096)), dict(gain=(0.01, 1, 1)), dict(cfa="rgbg"), dict(lo=(1, 2)), dict(lo=-1), dict(top=0),
                dict(top=65536), dict(top=1.5), dict(mode="inpaint")):
        a = dict(sat=4095, black=64, gain=(2.0, 1.0, 1.6), cfa="rggb", lo=None, top=65535, mode="rebuild")
        a.update(bad)
        with pytest.raises(ValueError):
            M._hl_struct("highlights", **a)
    for name in ("demosaic", "demosaic_display", "demosaic_yuv", "decode_rgb", "decode_display", "decode_yuv"):
        assert "highlights" in getattr(M.Context, name).__code__.co_varnames
    assert "highlights" not in M.Context.decode_merge.__code__.co_varnames[:M.Context.decode_merge.__code__.co_argcount + M.Context.decode_merge.__code__.co_kwonlyargcount]
