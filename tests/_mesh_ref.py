"""numpy statement of the mesh warp of the demosaic (mcraw_demosaic_mesh_batch, include/mcraw_hip.h), bit-exact.

A mesh is (My, Mx, 2) int32 nodes (Y, X), My = ceil(Ho / 32) + 1, Mx = ceil(Wo / 32) + 1: node (a, b) is the source position of
output pixel (32 a, 32 b) in 1/256 sample.  Output pixel (i, k), a = i >> 5, u = i & 31, b = k >> 5, v = k & 31 (int64):
    Yr = (Y00 (32-u)(32-v) + Y01 (32-u) v + Y10 u (32-v) + Y11 u v + 512) >> 10      Y = min(max(Yr, 0), 256 (height - 1))
and X likewise with the width.  The window of a tile from the clamped positions of its four corner pixels (warp_window's formula),
np' = min(np, 26), ne' = min(ne, 8); a pixel's first tap row iy - 1 is clamped to [pb, pb + 2 np' - 4], its first tap column to
[eb, eb + 8 ne' - 4].  From there on the table and the gather are _warp_ref's, over position arrays."""
import numpy as np

import _rgb_ref as R
import _warp_ref as W

STEP = 32
NP, NE = 26, 8   # WARP_EROWS / 2, WARP_ECOLS / 8
REACH = 2        # the tap origins are clamped into the window, which leaves the frame by at most 2 rows and columns of estimates
FILTER_CODE = W.FILTER_CODE
table = W.table
values, float_bits, display_from_o, yuv_from_o = W.values, W.float_bits, W.display_from_o, W.yuv_from_o


def grid(size):
    return (size[0] + STEP - 1) // STEP + 1, (size[1] + STEP - 1) // STEP + 1


def raw_positions(mesh, size):
    """(Yr, Xr) int64 (Ho, Wo): the interpolated positions before the clamp."""
    mesh = np.asarray(mesh)
    assert mesh.dtype == np.int32 and mesh.shape == grid(size) + (2,), (mesh.dtype, mesh.shape)
    m = mesh.astype(np.int64)
    i = np.arange(size[0], dtype=np.int64)
    k = np.arange(size[1], dtype=np.int64)
    a, u = (i >> 5)[:, None], (i & 31)[:, None]
    b, v = (k >> 5)[None, :], (k & 31)[None, :]
    out = []
    for c in (0, 1):
        n = m[:, :, c]
        s = n[a, b] * ((32 - u) * (32 - v)) + n[a, b + 1] * ((32 - u) * v) + n[a + 1, b] * (u * (32 - v)) + n[a + 1, b + 1] * (u * v)
        out.append((s + 512) >> 10)
    return out[0], out[1]


def positions(mesh, size, height, width):
    """(Y, X) int64 (Ho, Wo): the clamped positions."""
    Yr, Xr = raw_positions(mesh, size)
    return np.clip(Yr, 0, 256 * (height - 1)), np.clip(Xr, 0, 256 * (width - 1))


def windows(Y, X):
    """Per pixel, its tile's (pb, eb, np, ne) (int64 arrays (Ho, Wo)): from the tile's four corner pixels."""
    Ho, Wo = Y.shape
    pb, eb, npp, nee = (np.zeros((Ho, Wo), dtype=np.int64) for _ in range(4))
    for i0 in range(0, Ho, STEP):
        for k0 in range(0, Wo, STEP):
            i1, k1 = min(i0 + STEP, Ho) - 1, min(k0 + STEP, Wo) - 1
            cy, cx = Y[[i0, i0, i1, i1], [k0, k1, k0, k1]], X[[i0, i0, i1, i1], [k0, k1, k0, k1]]
            p = ((int(cy.min()) >> 8) - 1) & ~1
            e = ((int(cx.min()) >> 8) - 1) & ~7
            sl = (slice(i0, i1 + 1), slice(k0, k1 + 1))
            pb[sl], eb[sl] = p, e
            npp[sl] = (((int(cy.max()) >> 8) + 2 - p) >> 1) + 1
            nee[sl] = (((int(cx.max()) >> 8) + 2 - e) >> 3) + 1
    return pb, eb, npp, nee


def in_regime(mesh, size, height, width):
    Y, X = positions(mesh, size, height, width)
    _, _, npp, nee = windows(Y, X)
    return bool(npp.max() <= NP and nee.max() <= NE)


def tap_origins(mesh, size, height, width):
    """(Y, X, r, c): the clamped positions and the first tap row and column of every pixel, with both clamps."""
    Y, X = positions(mesh, size, height, width)
    pb, eb, npp, nee = windows(Y, X)
    r = np.clip((Y >> 8) - 1, pb, pb + 2 * np.minimum(npp, NP) - 4)
    c = np.clip((X >> 8) - 1, eb, eb + 8 * np.minimum(nee, NE) - 4)
    return Y, X, r, c


def gather(e, Y, X, r, c, filt="cubic"):
    """e (3, H, W) integers -> E (3, Ho, Wo) int64: _warp_ref's gather with the phases of (Y, X) and the taps from (r, c) on."""
    e = np.asarray(e, dtype=np.int64)
    assert np.abs(e).max() < 1 << 22
    P = np.pad(e, ((0, 0), (REACH, REACH), (REACH, REACH)), mode="reflect")
    H, Wd = e.shape[1:]
    assert r.min() >= -REACH and r.max() + 3 <= H - 1 + REACH and c.min() >= -REACH and c.max() + 3 <= Wd - 1 + REACH
    T = table(filt)
    wy, wx = T[Y & 255], T[X & 255]
    iy, ix = r + REACH, c + REACH

    def dot(w, v):
        return (sum(w[..., j] * v[j] for j in range(4)) + 2048) >> 12

    E = np.zeros((3,) + Y.shape, dtype=np.int64)
    for ch in range(3):
        t = [dot(wx, [P[ch][iy + rr, ix + j] for j in range(4)]) for rr in range(4)]
        E[ch] = dot(wy, t)
    return E


def mesh_from_e(e, mesh, size, filt="cubic"):
    H, Wd = np.asarray(e).shape[1:]
    return gather(e, *tap_origins(mesh, size, H, Wd), filt)


def mesh_estimates(img, mesh, size, filt="cubic", black=(0, 0, 0, 0), cfa="rggb"):
    """E (3, Ho, Wo) int64 in units of 1/16."""
    return mesh_from_e(R.mhc_estimates(np.asarray(img), black, cfa), mesh, size, filt)


def translation_mesh(size, ty, tx):
    """Nodes 256 (32 a + ty, 32 b + tx), ty and tx in samples (fractions of 1/256 allowed)."""
    my, mx = grid(size)
    a = np.arange(my, dtype=np.int64)[:, None]
    b = np.arange(mx, dtype=np.int64)[None, :]
    return np.stack([256 * 32 * a + int(round(256 * ty)) + 0 * b, 256 * 32 * b + int(round(256 * tx)) + 0 * a], axis=-1).astype(np.int32)


def mesh_ref(img, mesh, size, dtype, white, filt="cubic", black=(0, 0, 0, 0), cfa="rggb", gain=(1, 1, 1), matrix=None, clip=False):
    return float_bits(values(mesh_estimates(img, mesh, size, filt, black, cfa), white, black, gain, matrix, clip), dtype)


def mesh_display_ref(img, mesh, size, white, lut, dtype="u8", layout="hwc", filt="cubic", black=(0, 0, 0, 0), cfa="rggb",
                     gain=(1, 1, 1), matrix=None):
    return display_from_o(values(mesh_estimates(img, mesh, size, filt, black, cfa), white, black, gain, matrix), lut, dtype, layout)


def mesh_yuv_ref(img, mesh, size, white, lut, fmt, coef, in_bits, filt="cubic", black=(0, 0, 0, 0), cfa="rggb", gain=(1, 1, 1),
                 matrix=None):
    return yuv_from_o(values(mesh_estimates(img, mesh, size, filt, black, cfa), white, black, gain, matrix), lut, fmt, coef, in_bits)
