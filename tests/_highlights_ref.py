"""The numpy statement of mcraw_highlights_measure_batch and mcraw_highlights_batch (include/mcraw_hip.h): integers only, so the
kernels must agree with it bit for bit.  Arguments by CFA position p = (y & 1) * 2 + (x & 1) are sequences of four."""
import numpy as np

CLIP, REBUILD = 0, 1
CHROMA_MAX = 1 << 20
CFA = {"rggb": 0, "bggr": 1, "grbg": 2, "gbrg": 3}


def inv(gain):
    return [((1 << 24) + int(g) // 2) // int(g) for g in gain]


def green(cfa, p):
    """Is CFA position p green for the cfa code?"""
    return (((p & 1) ^ (p >> 1)) != 0) == (cfa < 2)


def by_position(vals, H, W):
    """(H, W) int64: vals[p] at every pixel of position p."""
    a = np.empty((H, W), np.int64)
    for p in range(4):
        a[p >> 1::2, p & 1::2] = int(vals[p])
    return a


def wb(img, black, gain):
    """The white-balanced values of (..., H, W) samples, int64."""
    H, W = img.shape[-2:]
    d = np.maximum(img.astype(np.int64) - by_position(black, H, W), 0)
    return (d * by_position(gain, H, W) + 2048) >> 12


def _nb(a):
    """The eight neighbours of every element of (..., H, W) under the reflection -1 -> 1, n -> n - 2, keyed by (dy, dx)."""
    pad = [(0, 0)] * (a.ndim - 2) + [(1, 1), (1, 1)]
    p = np.pad(a, pad, mode="reflect")
    H, W = a.shape[-2:]
    return {(dy, dx): p[..., 1 + dy:1 + dy + H, 1 + dx:1 + dx + W] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dy or dx}


def reference(v, cfa):
    """ref at every pixel from the white-balanced values v (..., H, W)."""
    H, W = v.shape[-2:]
    n = _nb(v)
    Hm = (n[0, -1] + n[0, 1] + 1) >> 1
    Vm = (n[-1, 0] + n[1, 0] + 1) >> 1
    Dm = (n[-1, -1] + n[-1, 1] + n[1, -1] + n[1, 1] + 2) >> 2
    hv = (Hm + Vm + 1) >> 1
    g = by_position([1 if green(cfa, p) else 0 for p in range(4)], H, W).astype(bool)
    return np.where(g, hv, (hv + Dm + 1) >> 1)


def measure(imgs, sat, black, gain, cfa, lo, nrec=None, into=None):
    """The records of a batch (N, H, W): (sum int64 (R, 4), cnt uint32 (R, 4)), R = nrec (N by default, or 1).  into: records
    (sum, cnt) to add to (MCRAW_HL_ACCUMULATE)."""
    imgs = np.asarray(imgs)
    N, H, W = imgs.shape
    nrec = N if nrec is None else nrec
    assert nrec in (1, N)
    s = imgs.astype(np.int64)
    satm, lom = by_position(sat, H, W), by_position(lo, H, W)
    below = s < satm
    ok = (s >= lom) & below
    for m in _nb(below).values():
        ok &= m
    v = wb(imgs, black, gain)
    diff = np.where(ok, v - reference(v, cfa), 0)
    sums = np.zeros((nrec, 4), np.int64) if into is None else into[0].astype(np.int64).copy()
    cnts = np.zeros((nrec, 4), np.int64) if into is None else into[1].astype(np.int64).copy()
    for f in range(N):
        r = f if nrec == N and N > 1 else 0
        for p in range(4):
            sums[r, p] += int(diff[f, p >> 1::2, p & 1::2].sum())
            cnts[r, p] += int(ok[f, p >> 1::2, p & 1::2].sum())
    return sums, (cnts & 0xFFFFFFFF).astype(np.uint32)


def raw(sums, cnts):
    """The records as the library lays them out: int64 (R, 8)."""
    R = sums.shape[0]
    a = np.zeros((R, 64), np.uint8)
    a[:, :32] = np.ascontiguousarray(sums, dtype=np.int64).view(np.uint8).reshape(R, 32)
    a[:, 32:48] = np.ascontiguousarray(cnts, dtype=np.uint32).view(np.uint8).reshape(R, 16)
    return a.view(np.int64).reshape(R, 8)


def chroma(sums, cnts):
    """sum / cnt as C divides int64 (towards zero), 0 without a count, clamped to -2^20 .. 2^20: int64 (R, 4)."""
    out = np.zeros(sums.shape, np.int64)
    for idx in np.ndindex(*sums.shape):
        s, c = int(sums[idx]), int(cnts[idx])
        q = 0 if c == 0 else (abs(s) // c) * (1 if s >= 0 else -1)
        out[idx] = min(max(q, -CHROMA_MAX), CHROMA_MAX)
    return out


def caps(sat, black, gain):
    """(m, cap[4]) of MCRAW_HL_CLIP."""
    m = min(((int(sat[p]) - int(black[p])) * int(gain[p]) + 2048) >> 12 for p in range(4))
    iv = inv(gain)
    return m, [int(black[p]) + ((m * iv[p] + 2048) >> 12) for p in range(4)]


def apply(imgs, mode, sat, black, gain, cfa, rec=None, top=65535):
    """The output of mcraw_highlights_batch for a batch (N, H, W): uint16.  rec: None (chroma 0) or (sum, cnt) of 1 or N records."""
    imgs = np.asarray(imgs)
    N, H, W = imgs.shape
    s = imgs.astype(np.int64)
    if mode == CLIP:
        return np.minimum(s, by_position(caps(sat, black, gain)[1], H, W)).astype(np.uint16)
    v = wb(imgs, black, gain)
    ch = np.zeros((N, H, W), np.int64)
    if rec is not None:
        c = chroma(*rec)
        for f in range(N):
            ch[f] = by_position(c[f if c.shape[0] > 1 else 0], H, W)
    cand = reference(v, cfa) + ch
    blk = by_position(black, H, W)
    back = blk + ((np.maximum(cand, 0) * by_position(inv(gain), H, W) + 2048) >> 12)
    new = np.maximum(s, np.minimum(back, int(top)))
    take = (s >= by_position(sat, H, W)) & (cand > v)
    return np.where(take, new, s).astype(np.uint16)


def default_lo(sat, black):
    return [int(b) + (int(s) - int(b)) // 2 for s, b in zip(sat, black)]
