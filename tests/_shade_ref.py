"""numpy statement of mcraw_shade_batch's contract (include/mcraw_hip.h): a lens-shading gain map, four planes of Q3.12
entries by CFA position, bilinearly interpolated in integers (vertical first, every stage rounds) and applied to what a
sample holds above its black level.  int64 throughout: the bounds the contract states are checked, not relied on."""
import numpy as np


def steps(W, H, gw, gh):
    """(sx, sy): the 8.24 step per pixel column / row, floored; 0 for a size of 1."""
    sx = ((gw - 1) << 24) // (W - 1) if W > 1 else 0
    sy = ((gh - 1) << 24) // (H - 1) if H > 1 else 0
    return sx, sy


def gains(H, W, gmap):
    """G (H, W) int64 of the contract for a map (4, gh, gw) uint16; also returns the largest |intermediate sum| seen."""
    gmap = np.asarray(gmap)
    assert gmap.ndim == 3 and gmap.shape[0] == 4 and gmap.dtype == np.uint16
    gh, gw = gmap.shape[1:]
    assert 1 <= gh <= 64 and 1 <= gw <= 64
    g = (gmap & 0x7FFF).astype(np.int64)
    sx, sy = steps(W, H, gw, gh)
    ux = np.arange(W, dtype=np.int64) * sx
    uy = np.arange(H, dtype=np.int64) * sy
    assert ux.max() < 1 << 30 and uy.max() < 1 << 30
    i0, fx = ux >> 24, (ux >> 12) & 4095
    j0, fy = uy >> 24, (uy >> 12) & 4095
    i1, j1 = np.minimum(i0 + 1, gw - 1), np.minimum(j0 + 1, gh - 1)
    assert i0.max() <= gw - 1 and j0.max() <= gh - 1
    p = (np.arange(H)[:, None] & 1) * 2 + (np.arange(W)[None, :] & 1)
    J0, J1, FY = j0[:, None], j1[:, None], fy[:, None]
    I0, I1, FX = i0[None, :], i1[None, :], fx[None, :]
    s0 = g[p, J0, I0] * (4096 - FY) + g[p, J1, I0] * FY + 2048
    s1 = g[p, J0, I1] * (4096 - FY) + g[p, J1, I1] * FY + 2048
    V0, V1 = s0 >> 12, s1 >> 12
    s2 = V0 * (4096 - FX) + V1 * FX + 2048
    G = s2 >> 12
    assert G.min() >= 0 and G.max() <= 32767
    return G, int(max(s0.max(), s1.max(), s2.max()))


def apply(img, G, black=(0, 0, 0, 0), top=65535, with_peak=False):
    """The sample stage alone: the uint16 (H, W) result for one mosaic and per-pixel gains G (H, W) as gains() gives them."""
    img = np.asarray(img)
    assert img.ndim == 2 and img.dtype == np.uint16 and 1 <= top <= 65535 and G.shape == img.shape
    H, W = img.shape
    p = (np.arange(H)[:, None] & 1) * 2 + (np.arange(W)[None, :] & 1)
    b = np.asarray(black, dtype=np.int64)[p]
    d = img.astype(np.int64) - b
    prod = d * G + 2048
    c = b + (prod >> 12)  # numpy's >> on a signed integer is arithmetic: floor
    out = np.clip(c, 0, top).astype(np.uint16)
    return (out, int(np.abs(prod).max())) if with_peak else out


def shade_ref(img, gmap, black=(0, 0, 0, 0), top=65535, with_peak=False):
    """The uint16 (H, W) result for one mosaic and one map (4, gh, gw)."""
    G, peak = gains(np.shape(img)[0], np.shape(img)[1], gmap)
    res = apply(img, G, black, top, with_peak)
    return (res[0], max(res[1], peak)) if with_peak else res


def shade_batch_ref(imgs, gmaps, black=(0, 0, 0, 0), top=65535):
    """(N, H, W) for maps (4, gh, gw) (all frames) or (N, 4, gh, gw) (per frame)."""
    imgs, gmaps = np.asarray(imgs), np.asarray(gmaps)
    return np.stack([shade_ref(imgs[i], gmaps if gmaps.ndim == 3 else gmaps[i], black, top) for i in range(imgs.shape[0])])


def float_gains(H, W, fg):
    """float64 bilinear interpolation (H, W) of unquantised gains (4, gh, gw): map point (j, i) on pixel
    (j * (H - 1) / (gh - 1), i * (W - 1) / (gw - 1))."""
    fg = np.asarray(fg, dtype=np.float64)
    gh, gw = fg.shape[1:]
    u = np.arange(W, dtype=np.float64) * ((gw - 1) / (W - 1) if W > 1 else 0.0)
    v = np.arange(H, dtype=np.float64) * ((gh - 1) / (H - 1) if H > 1 else 0.0)
    i0 = np.minimum(np.floor(u).astype(np.int64), gw - 1)
    j0 = np.minimum(np.floor(v).astype(np.int64), gh - 1)
    i1, j1 = np.minimum(i0 + 1, gw - 1), np.minimum(j0 + 1, gh - 1)
    fx, fy = (u - i0)[None, :], (v - j0)[:, None]
    p = (np.arange(H)[:, None] & 1) * 2 + (np.arange(W)[None, :] & 1)
    J0, J1, I0, I1 = j0[:, None], j1[:, None], i0[None, :], i1[None, :]
    a = fg[p, J0, I0] * (1 - fy) + fg[p, J1, I0] * fy
    b = fg[p, J0, I1] * (1 - fy) + fg[p, J1, I1] * fy
    return a * (1 - fx) + b * fx
