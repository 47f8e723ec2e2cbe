"""numpy statement of the affine warp of the demosaic (mcraw_demosaic_warp_batch, include/mcraw_hip.h), bit-exact.

A map is six integers {ayy, ayx, ty, axy, axx, tx}: the linear part in 1/65536, the translation in 1/256 sample.  Output pixel
(i, k) reads, in 1/256 sample (int64, arithmetic shifts):
    Y = ty + ((ayy i + ayx k + 128) >> 8)      iy = Y >> 8,  py = Y & 255
    X = tx + ((axy i + axx k + 128) >> 8)      ix = X >> 8,  px = X & 255
One table of 256 phases x 4 taps (j = -1 .. 2 about iy or ix) serves both axes:
    linear w(p) = (0, 16 (256 - p), 16 p, 0)
    cubic  a = 4 |256 j - p|, f = _resample_ref.kernel_f(a, "cubic"), F = sum f, w = (4096 f + F // 2) // F; the residual
           4096 - sum w goes to the tap of smallest distance, half each to two equally near
e: _rgb_ref.mhc_estimates of the WHOLE frame (1/16 DN), reflected 101-style beyond its edges.
    t(r, k) = (sum_j w(px)[j] e(r, ix - 1 + j) + 2048) >> 12       r = iy - 1 .. iy + 2
    E(i, k) = (sum_j w(py)[j] t(iy - 1 + j, k) + 2048) >> 12
Behind E the colour stage, the LUT and the Y'CbCr matrix are _rgb_ref's, _display_ref's and _yuv_ref's, with MHC's k[c]."""
import functools

import numpy as np

import _resample_ref as RS
import _rgb_ref as R

FILTER_CODE = RS.FILTER_CODE
REACH = 2        # taps leave the frame by at most this many samples (the corners lie inside it)
ONE, DEV = 65536, 16384
IDENTITY = (65536, 0, 0, 0, 65536, 0)


@functools.lru_cache(maxsize=None)
def table(filt):
    """(256, 4) int64: the weights of every phase."""
    p = np.arange(256, dtype=np.int64)
    if filt == "linear":
        return np.stack([0 * p, 16 * (256 - p), 16 * p, 0 * p], axis=1)
    assert filt == "cubic"
    d = np.abs(256 * np.arange(-1, 3, dtype=np.int64)[None, :] - p[:, None])      # (256, 4)
    f = RS.kernel_f(4 * d, "cubic")
    F = f.sum(axis=1, keepdims=True)
    w = (4096 * f + F // 2) // F
    res = 4096 - w.sum(axis=1)
    near = d == d.min(axis=1, keepdims=True)
    cnt = near.sum(axis=1)
    assert ((cnt == 1) | (cnt == 2)).all() and (res[cnt == 2] % 2 == 0).all()
    half = np.where(cnt == 2, res // 2, 0)
    rows = np.arange(256)
    w[rows, near.argmax(axis=1)] += res - half
    w[rows, 3 - near[:, ::-1].argmax(axis=1)] += half
    return w


def positions(m, size):
    """(Y, X) int64 (Ho, Wo) each: the source positions of the output pixels under map m, in 1/256 sample."""
    ayy, ayx, ty, axy, axx, tx = (int(v) for v in m)
    i = np.arange(size[0], dtype=np.int64)[:, None]
    k = np.arange(size[1], dtype=np.int64)[None, :]
    return ty + ((ayy * i + ayx * k + 128) >> 8), tx + ((axy * i + axx * k + 128) >> 8)


def map_ok(m, size, height, width):
    """The contract's rules for one map: the linear part's bounds and the four corners inside the frame."""
    m = [int(v) for v in m]
    if max(abs(m[0] - ONE), abs(m[4] - ONE), abs(m[1]), abs(m[3])) > DEV:
        return False
    Y, X = positions(m, size)
    cy, cx = Y[[0, 0, -1, -1], [0, -1, 0, -1]], X[[0, 0, -1, -1], [0, -1, 0, -1]]
    return bool(cy.min() >= 0 and cy.max() <= 256 * (height - 1) and cx.min() >= 0 and cx.max() <= 256 * (width - 1))


def warp_from_e(e, m, size, filt="cubic", split=False):
    """e (3, H, W) integers, MHC's estimates of the whole frame -> E (3, Ho, Wo) int64.  split: the sums in two int32
    accumulators over v = 256 vh + vl, as the kernel forms them (asserted to stay inside int32), instead of int64 sums."""
    e = np.asarray(e, dtype=np.int64)
    H, W = e.shape[1:]
    assert min(H, W) >= 8 and map_ok(m, size, H, W), "a map outside the contract"
    assert np.abs(e).max() < 1 << 22
    P = np.pad(e, ((0, 0), (REACH, REACH), (REACH, REACH)), mode="reflect")
    Y, X = positions(m, size)
    assert Y.min() >= 0 and Y.max() <= 256 * (H - 1) and X.min() >= 0 and X.max() <= 256 * (W - 1), "the corners bound every pixel"
    T = table(filt)
    wy, wx = T[Y & 255], T[X & 255]                     # (Ho, Wo, 4)
    iy, ix = (Y >> 8) + REACH - 1, (X >> 8) + REACH - 1  # the first tap, in P

    def dot(w, v):  # sum_j w[..., j] v[j]; -> (sum + 2048) >> 12
        if not split:
            return (sum(w[..., j] * v[j] for j in range(4)) + 2048) >> 12
        a = sum(w[..., j] * (v[j] >> 8) for j in range(4))
        b = sum(w[..., j] * (v[j] & 255) for j in range(4))
        assert np.abs(a).max() < 1 << 31 and np.abs(b).max() < 1 << 31
        return (a + ((b + 2048) >> 8)) >> 4

    E = np.zeros((3,) + tuple(size), dtype=np.int64)
    for c in range(3):
        t = [dot(wx, [P[c][iy + r, ix + j] for j in range(4)]) for r in range(4)]
        assert max(np.abs(v).max() for v in t) < 1 << 23
        E[c] = dot(wy, t)
    assert np.abs(E).max() < 1 << 24
    return E


def warp_estimates(img, m, size, filt="cubic", black=(0, 0, 0, 0), cfa="rggb"):
    """E (3, Ho, Wo) int64 in units of 1/16."""
    return warp_from_e(R.mhc_estimates(np.asarray(img), black, cfa), m, size, filt)


values = RS.values
float_bits = RS.float_bits
display_from_o = RS.display_from_o
yuv_from_o = RS.yuv_from_o


def warp_ref(img, m, size, dtype, white, filt="cubic", black=(0, 0, 0, 0), cfa="rggb", gain=(1, 1, 1), matrix=None, clip=False):
    return float_bits(values(warp_estimates(img, m, size, filt, black, cfa), white, black, gain, matrix, clip), dtype)


def warp_display_ref(img, m, size, white, lut, dtype="u8", layout="hwc", filt="cubic", black=(0, 0, 0, 0), cfa="rggb",
                     gain=(1, 1, 1), matrix=None):
    return display_from_o(values(warp_estimates(img, m, size, filt, black, cfa), white, black, gain, matrix), lut, dtype, layout)


def warp_yuv_ref(img, m, size, white, lut, fmt, coef, in_bits, filt="cubic", black=(0, 0, 0, 0), cfa="rggb", gain=(1, 1, 1),
                 matrix=None):
    return yuv_from_o(values(warp_estimates(img, m, size, filt, black, cfa), white, black, gain, matrix), lut, fmt, coef, in_bits)
