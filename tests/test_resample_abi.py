"""The resampling demosaic (mcraw_demosaic_resample_batch) without a GPU: the ABI's symbols, macros and struct, the numpy
statement of the contract (_resample_ref) against a scalar one written straight from the header, the properties the contract names
(weights, identity at the crop's own size, flat frames), the int32 formulation the kernel uses against the exact sums at the
extreme inputs, and the distance from a float64 resampling with the unquantised kernel."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import _resample_ref as S
import _rgb_ref as R
import motioncam_decoder_amd as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFAS = ("rggb", "bggr", "grbg", "gbrg")
FILTERS = ("linear", "cubic")


def _hdr():
    return open(os.path.join(ROOT, "include", "mcraw_hip.h")).read()


def test_resample_symbols_exported_and_listed():
    hdr = _hdr()
    lib = M.load()
    for sym in ("mcraw_demosaic_resample_batch", "mcraw_resample_work_bytes"):
        assert re.search(r"\b%s\s*\(" % sym, hdr), sym
        assert sym in M.ABI_SYMBOLS and hasattr(lib, sym), sym
    assert re.search(r"#define MCRAW_RGB_RESAMPLE\s+4\b", hdr) and M.RGB_RESAMPLE == 4
    assert re.search(r"#define MCRAW_FILTER_LINEAR\s+0\b", hdr) and M.FILTER_LINEAR == 0
    assert re.search(r"#define MCRAW_FILTER_CUBIC\s+1\b", hdr) and M.FILTER_CUBIC == 1
    assert re.search(r"#define MCRAW_K_COUNT\s+11\b", hdr)
    for name in ("Resample", "RGB_RESAMPLE", "FILTER_LINEAR", "FILTER_CUBIC"):
        assert name in M.__all__
    assert hdr.index("} mcraw_area;") < hdr.index("half to twice a crop window")  # behind the area section, which stays as it was
    block = hdr[hdr.index("half to twice a crop window"):hdr.index("} mcraw_resample;")]
    for line in ("D = 2 max(C, O);  n(k, j) = 2 O j - ((2 k + 1) C - O);  a = floor((1024 |n| + D / 2) / D)",
                 "linear: f = max(0, 1024 - a)", "f = 3 a^3 - 5 * 1024 a^2 + 2 * 1024^3",
                 "f = -a^3 + 5 * 1024 a^2 - 8 * 1024^2 a + 4 * 1024^3", "w(k, j) = floor((4096 f + F / 2) / F)",
                 "added to the tap of smallest |n|", "t_c(y, k) = (sum_j wx(k, j) e_c(y, x0 + j) + 2048) >> 12",
                 "E_c(i, k) = (sum_j wy(i, j) t_c(y0 + j, k) + 2048) >> 12", "|E| < 2^24", "k[c] = (gain[c] * inv) * 0.0625f",
                 "e_c(reflect101(y, height), reflect101(x, width))", "(256 A + B + 2048) >> 12 == (A + ((B + 2048) >> 8)) >> 4",
                 "ceil(cw / 2) <= out_w <= 2 cw"):
        assert line in block, line


def test_resample_struct_layout():
    names = ("x0", "y0", "cw", "ch", "out_w", "out_h", "filter", "reserved")
    assert C.sizeof(M.Resample) == 32
    assert [getattr(M.Resample, f).offset for f in names] == [0, 4, 8, 12, 16, 20, 24, 28]
    m = re.search(r"\}\s*mcraw_resample;\s*/\*\s*sizeof (\d+); y0 (\d+), cw (\d+), ch (\d+), out_w (\d+), out_h (\d+), filter (\d+), "
                  r"reserved (\d+)", _hdr())
    assert m and [int(v) for v in m.groups()] == [32, 4, 8, 12, 16, 20, 24, 28]


def _res(cw, ch, ow, oh, x0=0, y0=0, filt=1, reserved=0):
    r = M.Resample()
    r.x0, r.y0, r.cw, r.ch, r.out_w, r.out_h, r.filter, r.reserved = x0, y0, cw, ch, ow, oh, filt, reserved
    return r


def test_work_bytes():
    wb = M.load().mcraw_resample_work_bytes
    assert wb(None) == 0
    # a table per axis: the first sample, the taps and 9 weights per output column and row
    assert wb(_res(4032, 2268, 3840, 2160)) >= (3840 + 2160) * (4 + 2 + 9 * 2)
    assert wb(_res(2, 2, 1, 1)) > 0 and wb(_res(2, 2, 4, 4)) > 0 and wb(_res(64, 64, 32, 128, filt=0)) > 0
    for bad in (_res(3, 2, 2, 2), _res(2, 2, 1, 1, x0=1), _res(2, 2, 1, 1, y0=1), _res(0, 2, 1, 1), _res(2, 0, 1, 1),
                _res(2, 2, 0, 1), _res(2, 2, 1, 0), _res(2, 2, 5, 1), _res(2, 2, 1, 5), _res(66, 64, 32, 64), _res(64, 66, 64, 32),
                _res(2, 2, 1, 1, reserved=1), _res(2, 2, 1, 1, filt=2)):
        assert wb(bad) == 0, [getattr(bad, f) for f in ("x0", "y0", "cw", "ch", "out_w", "out_h", "filter", "reserved")]


def _scalar_taps(k, Cn, O, filt):
    """The header's weights of pixel k, in Python integers: {j: w}."""
    D = 2 * max(Cn, O)
    f = {}
    for j in range(-8, Cn + 8):
        n = 2 * O * j - ((2 * k + 1) * Cn - O)
        a = (1024 * abs(n) + D // 2) // D
        if filt == "linear":
            v = max(0, 1024 - a)
        elif a <= 1024:
            v = 3 * a ** 3 - 5 * 1024 * a ** 2 + 2 * 1024 ** 3
        elif a < 2048:
            v = -a ** 3 + 5 * 1024 * a ** 2 - 8 * 1024 ** 2 * a + 4 * 1024 ** 3
        else:
            v = 0
        f[j] = (v, abs(n))
    F = sum(v for v, _ in f.values())
    w = {j: (4096 * v + F // 2) // F for j, (v, _) in f.items()}
    res = 4096 - sum(w.values())
    best = min(an for _, an in f.values())
    near = [j for j, (_, an) in f.items() if an == best]
    if len(near) == 1:
        w[near[0]] += res
    else:
        w[near[0]] += res - res // 2
        w[near[1]] += res // 2
    return {j: v for j, v in w.items() if v or f[j][0]}


def _reflect(i, n):
    i = -i if i < 0 else i
    return 2 * (n - 1) - i if i > n - 1 else i


def _scalar(img, crop, size, filt, black, cfa):
    """The header's statement, one output pixel at a time, in Python integers."""
    y0, x0, h, w = crop
    ho, wo = size
    H, W = img.shape
    e = R.mhc_estimates(img, black, cfa)
    xt = [_scalar_taps(k, w, wo, filt) for k in range(wo)]
    yt = [_scalar_taps(i, h, ho, filt) for i in range(ho)]
    rows = sorted({y0 + j for t in yt for j in t})
    out = np.zeros((3, ho, wo), dtype=np.int64)
    for c in range(3):
        t = {y: [(sum(wt * int(e[c, _reflect(y, H), _reflect(x0 + j, W)]) for j, wt in xt[k].items()) + 2048) >> 12 for k in range(wo)]
             for y in rows}
        for i in range(ho):
            for k in range(wo):
                out[c, i, k] = (sum(wt * t[y0 + j][k] for j, wt in yt[i].items()) + 2048) >> 12
    return out


@pytest.mark.parametrize("filt", FILTERS)
def test_numpy_statement_equals_the_scalar_one(filt):
    rng = np.random.default_rng(11)
    img = rng.integers(0, 4096, size=(12, 16)).astype(np.uint16)
    black = (60, 64, 61, 70)
    for crop, size in (((2, 2, 8, 10), (7, 13)), ((0, 0, 12, 16), (6, 8)), ((4, 6, 8, 10), (16, 20)), ((0, 6, 6, 10), (6, 10)),
                       ((0, 0, 12, 16), (11, 17))):
        for cfa in ("rggb", "gbrg"):
            assert np.array_equal(S.resample_estimates(img, crop, size, filt, black, cfa), _scalar(img, crop, size, filt, black, cfa)), \
                (crop, size, cfa)


@pytest.fixture(scope="module")
def sweep():
    """Per filter: the largest sum |w| and the largest tap count over every legal (C, O) with C <= 96, with the weights' own
    properties asserted on the way."""
    out = {}
    for filt in FILTERS:
        sabs, taps = 0, 0
        for Cn in range(1, 97):
            for O in range((Cn + 1) // 2, 2 * Cn + 1):
                j0, nt, w = S.weights(Cn, O, filt)
                assert (w.sum(axis=1) == 4096).all(), (filt, Cn, O)
                assert j0.min() >= -4 and (j0 + nt - 1).max() <= Cn + 3
                # pixel O - 1 - k mirrors pixel k
                assert np.array_equal(nt, nt[::-1]) and np.array_equal(j0[::-1], Cn - 1 - (j0 + nt - 1)), (filt, Cn, O)
                idx = nt[:, None] - 1 - np.arange(9)[None, :]
                rev = np.where(idx >= 0, np.take_along_axis(w[::-1], np.clip(idx, 0, 8), axis=1), 0)
                assert np.array_equal(w, rev), (filt, Cn, O)
                if O == Cn:
                    assert (nt == 1).all() and np.array_equal(j0, np.arange(O)) and (w[:, 0] == 4096).all()
                sabs, taps = max(sabs, int(np.abs(w).sum(axis=1).max())), max(taps, int(nt.max()))
        out[filt] = (sabs, taps)
    return out


def test_weight_properties(sweep):
    assert sweep["linear"][1] <= 5 and sweep["cubic"][1] <= 9
    assert sweep["linear"][0] == 4096  # no negative weight
    assert 4096 < sweep["cubic"][0] <= 5600  # the header's bound on sum |w|


def test_identity_equals_mhc_of_the_crop():
    rng = np.random.default_rng(12)
    img = rng.integers(0, 4096, size=(16, 24)).astype(np.uint16)
    black = (60, 61, 62, 63)
    for cfa in CFAS:
        e = R.mhc_estimates(img, black, cfa)
        for crop in ((0, 0, 16, 24), (2, 4, 10, 16), (6, 0, 10, 8)):
            y0, x0, h, w = crop
            for filt in FILTERS:
                assert np.array_equal(S.resample_estimates(img, crop, (h, w), filt, black, cfa), e[:, y0:y0 + h, x0:x0 + w]), (cfa, crop, filt)
                want = R.ref_bits(img, "mhc", "f32", 4095.0, black=black, cfa=cfa, gain=(1.7, 1.0, 1.4))[:, y0:y0 + h, x0:x0 + w]
                assert np.array_equal(S.resample_ref(img, crop, (h, w), "f32", 4095.0, filt, black, cfa, (1.7, 1.0, 1.4)), want)


def test_flat_frames_stay_flat_at_every_legal_size():
    img = np.full((12, 14), 1234, dtype=np.uint16)
    black = (64, 64, 64, 64)
    crop = (2, 4, 6, 8)
    for filt in FILTERS:
        for ho in range(3, 13):
            for wo in range(4, 17):
                E = S.resample_estimates(img, crop, (ho, wo), filt, black, "grbg")
                assert (E == 16 * (1234 - 64)).all(), (filt, ho, wo)
    # greys stay neutral: equal channels in, equal channels out, whatever the black levels of the four positions
    grey = np.zeros((12, 14), dtype=np.uint16)
    for p, b in enumerate((60, 70, 80, 90)):
        grey[p >> 1::2, p & 1::2] = 1000 + b
    E = S.resample_estimates(grey, crop, (5, 11), "cubic", (60, 70, 80, 90), "bggr")
    assert (E == 16000).all()


def test_int32_formulation_is_exact_at_the_extremes(sweep):
    """The kernel's sums: v = 256 vh + vl, A = sum w vh and B = sum w vl in int32, (A + ((B + 2048) >> 8)) >> 4.  At samples
    alternating 0 / 65535 under blacks 65535 / 0 -- the largest |e| the format allows -- they equal the int64 sums, and the bounds
    that follow from the measured sum |w| hold."""
    sw = sweep["cubic"][0]
    yy, xx = np.mgrid[0:20, 0:28]
    worst = 0
    for phase, black in ((0, (65535, 0, 0, 65535)), (1, (0, 65535, 65535, 0)), (0, (0, 65535, 0, 65535)), (1, (65535, 65535, 0, 0))):
        img = (((yy + xx + phase) & 1) * 65535).astype(np.uint16)
        for cfa in ("rggb", "grbg"):
            e = R.mhc_estimates(img, black, cfa)
            worst = max(worst, int(np.abs(e).max()))
            for crop, size in (((2, 2, 16, 24), (9, 13)), ((0, 0, 20, 28), (37, 55)), ((2, 4, 14, 20), (10, 19))):
                for filt in FILTERS:
                    y0, x0, h, w = crop
                    P = np.pad(e, ((0, 0), (S.REACH,) * 2, (S.REACH,) * 2), mode="reflect")
                    t64 = S.filter_axis(P, x0, w, size[1], filt, 2)
                    t32 = _split_axis(P, x0, w, size[1], filt, 2)
                    assert np.array_equal(t64, t32)
                    E64 = S.filter_axis(t64, y0, h, size[0], filt, 1)
                    assert np.array_equal(E64, _split_axis(t64, y0, h, size[0], filt, 1))
                    assert np.abs(t64).max() < 1 << 23 and np.abs(E64).max() < 1 << 24
    # the bounds, from the measured sum |w| and the largest |e| of the format (40 * 65535: MHC's largest sum of |coefficients|)
    assert worst <= 40 * 65535 < 1 << 22
    emax = 40 * 65535
    tmax = (sw * emax + 2048) >> 12
    Emax = (sw * tmax + 2048) >> 12
    assert tmax < 1 << 23 and Emax < 1 << 24
    assert sw * ((tmax >> 8) + 1) < 1 << 31 and sw * 255 + 2048 < 1 << 31  # A and B of both passes fit int32
    assert sw < 1 << 13 and (tmax >> 8) + 1 < 1 << 23  # ... and their factors fit 24-bit multiplies
    assert sw * emax >= 1 << 31  # (a plain int32 sum would not: the reason for the split)


def _split_axis(e, origin, Cn, O, filt, axis):
    """filter_axis in the kernel's arithmetic: two int32 accumulators per sum (numpy wraps int32 silently: an overflow shows as
    a difference from the int64 sums)."""
    e = np.moveaxis(np.asarray(e), axis, -1)
    assert np.abs(e).max() < 1 << 31
    e = e.astype(np.int32)
    j0, nt, w = S.weights(Cn, O, filt)
    w = w.astype(np.int32)
    a = np.zeros(e.shape[:-1] + (O,), dtype=np.int32)
    b = np.zeros_like(a)
    with np.errstate(over="ignore"):
        for t in range(9):
            idx = np.where(t < nt, origin + S.REACH + j0 + t, 0)
            v = e[..., idx]
            a += w[:, t] * (v >> 8)
            b += w[:, t] * (v & 255)
        out = (a + ((b + np.int32(2048)) >> 8)) >> 4
    assert out.dtype == np.int32
    return np.moveaxis(out.astype(np.int64), -1, axis)


def _float_kernel(x, filt):
    x = np.abs(x)
    if filt == "linear":
        return np.maximum(0.0, 1.0 - x)
    return np.where(x <= 1, 1.5 * x ** 3 - 2.5 * x ** 2 + 1, np.where(x < 2, -0.5 * x ** 3 + 2.5 * x ** 2 - 4 * x + 2, 0.0))


def _float_weights(Cn, O, filt):
    """(O, C + 2 REACH) float64: the unquantised kernel at the exact distances, normalised per pixel; column j + REACH is sample j."""
    k = np.arange(O, dtype=np.float64)[:, None]
    j = np.arange(-S.REACH, Cn + S.REACH, dtype=np.float64)[None, :]
    u = (k + 0.5) * Cn / O - 0.5
    f = _float_kernel((j - u) / max(1.0, Cn / O), filt)
    return f / f.sum(axis=1, keepdims=True)


def _int_weights(Cn, O, filt):
    j0, nt, w = S.weights(Cn, O, filt)
    full = np.zeros((O, Cn + 2 * S.REACH))
    for k in range(O):
        full[k, j0[k] + S.REACH:j0[k] + S.REACH + nt[k]] = w[k, :nt[k]] / 4096.0
    return full


@pytest.mark.parametrize("filt", FILTERS)
def test_close_to_a_float64_resampling_with_the_unquantised_kernel(filt):
    """|E - E_float| <= dx R Sy + dy R Sx + (Sy / 2 + 1 / 2): dx, dy the largest sum_j |w / 4096 - w_float| of a pixel of either axis
    (the table's deviation from the kernel), R half the range of e over the frame (the weights of a pixel add up to 1 in both tables,
    so only e's distance from the middle of its range counts; t strays from it by at most R Sx), Sx and Sy the largest sum |w| / 4096
    of the axes (Sy carries the horizontal pass's error and its rounding of 1/2 through the vertical pass), 1/2 the second rounding.
    In 1/16 DN."""
    rng = np.random.default_rng(13)
    yy, xx = np.mgrid[0:40, 0:56]
    img = (1000 + 2 * xx + 3 * yy + rng.integers(-20, 21, size=(40, 56))).astype(np.uint16)
    black = (64, 64, 64, 64)
    e = R.mhc_estimates(img, black, "rggb")
    P = np.pad(e, ((0, 0), (S.REACH,) * 2, (S.REACH,) * 2), mode="reflect").astype(np.float64)
    Rh = (e.max() - e.min()) / 2.0
    for crop, size in (((4, 6, 30, 40), (21, 27)), ((4, 6, 30, 40), (43, 61)), ((0, 0, 40, 56), (20, 28)), ((2, 2, 36, 50), (72, 100)),
                       ((0, 0, 40, 56), (38, 53))):
        y0, x0, h, w = crop
        fx, fy = _float_weights(w, size[1], filt), _float_weights(h, size[0], filt)
        ix, iy = _int_weights(w, size[1], filt), _int_weights(h, size[0], filt)
        dx, dy = np.abs(ix - fx).sum(axis=1).max(), np.abs(iy - fy).sum(axis=1).max()
        sx, sy = np.abs(ix).sum(axis=1).max(), np.abs(iy).sum(axis=1).max()
        assert dx < 0.01 and dy < 0.01  # the table is the kernel to within its 1/1024 and 1/4096 steps
        tf = np.einsum("cyx,kx->cyk", P[:, :, x0:x0 + w + 2 * S.REACH], fx)
        Ef = np.einsum("cyk,iy->cik", tf[:, y0:y0 + h + 2 * S.REACH], fy)
        E = S.resample_estimates(img, crop, size, filt, black, "rggb")
        tol = dx * Rh * sy + dy * Rh * sx + 0.5 * sy + 0.5
        err = np.abs(E - Ef).max()
        print("%s %r -> %r: max |E - E_float| %.2f, tolerance %.2f (dx %.5f dy %.5f R %.0f)" % (filt, crop, size, err, tol, dx, dy, Rh))
        assert err <= tol, (crop, size, err, tol)
