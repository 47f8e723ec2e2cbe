"""The contract of mcraw_noise_batch (include/mcraw_hip.h) in numpy, integers only: what the GPU records must equal byte for byte.
Also the scenes and the noise model of the recovery tests (tests/test_noise_fit.py, tools/bench_noise.py)."""
import numpy as np

L, V = 32, 128
REC_BYTES = 4 * (4 * L * V + 8)


def energy_bin(T):
    """vb of T (integers below 2^63, any shape), with Python integers: 0 below 16, else e = floor(log2 T),
    f = (T >> (e - 2)) & 3, min(4 * (e - 4) + f + 1, 127)."""
    def one(t):
        t = int(t)
        if t < 16:
            return 0
        e = t.bit_length() - 1
        return min(4 * (e - 4) + ((t >> (e - 2)) & 3) + 1, V - 1)
    return np.vectorize(one, otypes=[np.int64])(np.asarray(T, dtype=object))


def edge(e, f):
    """The lower edge 2^e * (1 + f / 4) of the quarter-octave bin 4 * (e - 4) + f + 1, an integer for e >= 4."""
    return (1 << e) + f * (1 << (e - 2))


def planes(frames, roi=None):
    """(N, by, bx, 4, 8, 8) int64: the 8 x 8 planes by CFA position of the whole 16 x 16 blocks of the window
    roi = (y0, x0, h, w) (the whole frame unless given) of frames (N, H, W)."""
    f = np.asarray(frames)
    n, H, W = f.shape
    y0, x0, h, w = (0, 0, H, W) if roi is None else roi
    assert y0 % 2 == 0 and x0 % 2 == 0 and h >= 16 and w >= 16 and y0 + h <= H and x0 + w <= W
    by, bx = h // 16, w // 16
    win = f[:, y0:y0 + 16 * by, x0:x0 + 16 * bx].astype(np.int64)
    out = np.empty((n, by, bx, 4, 8, 8), np.int64)
    for p in range(4):
        pl = win[:, p >> 1::2, p & 1::2]  # (n, 8 by, 8 bx)
        out[:, :, :, p] = pl.reshape(n, by, 8, bx, 8).transpose(0, 1, 3, 2, 4)
    return out


def sums(b):
    """(s, T) of planes (..., 8, 8) int64."""
    dh = b[..., :, :-2] - 2 * b[..., :, 1:-1] + b[..., :, 2:]
    dv = b[..., :-2, :] - 2 * b[..., 1:-1, :] + b[..., 2:, :]
    return b.sum((-1, -2)), (dh * dh).sum((-1, -2)) + (dv * dv).sum((-1, -2))


def noise_stats(frames, shift, sat=65535, lo=0, roi=None):
    """dict(hist (N, 4, 32, 128), nblk (N, 4), nrej (N, 4)) uint32 of frames (N, H, W) uint16; sat, lo: one level or four."""
    sat = np.broadcast_to(np.asarray(sat, np.int64), (4,))
    lo = np.broadcast_to(np.asarray(lo, np.int64), (4,))
    b = planes(frames, roi)
    n = b.shape[0]
    s, T = sums(b)                                   # (n, by, bx, 4)
    rej = (b.max((-1, -2)) >= sat) | (b.min((-1, -2)) < lo)
    lv = np.minimum((s >> 6) >> shift, L - 1)
    vb = energy_bin(T)
    hist, nblk, nrej = np.zeros((n, 4, L, V), np.int64), np.zeros((n, 4), np.int64), np.zeros((n, 4), np.int64)
    for p in range(4):
        for f in range(n):
            ok = ~rej[f, :, :, p]
            np.add.at(hist[f, p], (lv[f, :, :, p][ok], vb[f, :, :, p][ok]), 1)
            nblk[f, p], nrej[f, p] = ok.sum(), (~ok).sum()
    return dict(hist=hist.astype(np.uint32), nblk=nblk.astype(np.uint32), nrej=nrej.astype(np.uint32))


def record(d):
    """The records' bytes (N, 65568) uint8: uint32 hist[4][32][128]; uint32 nblk[4]; uint32 nrej[4]."""
    n = d["hist"].shape[0]
    words = np.concatenate([d["hist"].reshape(n, -1), d["nblk"], d["nrej"]], axis=1).astype("<u4")
    return np.ascontiguousarray(words).view(np.uint8).reshape(n, REC_BYTES)


def add(a, b):
    return {k: (a[k].astype(np.uint64) + b[k]).astype(np.uint32) for k in ("hist", "nblk", "nrej")}


# ---- scenes of the recovery tests: clean images in DN above nothing (they include the black level), 12 bits

SCENES = ("ramp", "halftex", "checker", "natural")


def scene(name, H=1088, W=1920, black=64):
    """A clean (H, W) float64 image: a horizontal ramp; the ramp with the lower half strongly textured; the ramp under a
    checker of 400 DN whose edges cross 74 % of the blocks; a smooth scene with textured regions and steps of 200 DN."""
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    ramp = black + (xx / W) * 3600
    if name == "ramp":
        return ramp
    if name == "halftex":
        return ramp + 150 * np.sin(xx / 3.1) * np.sin(yy / 4.3) * (yy > H / 2)
    if name == "checker":
        return ramp + 400 * (((xx // 37) + (yy // 29)) % 2)
    if name == "natural":
        return black + np.clip(1800 + 1500 * np.sin(xx / 301.) * np.cos(yy / 177.)
                               + 300 * np.sin(xx / 11.) * np.sin(yy / 13.) * (np.sin(xx / 97.) > 0)
                               + 200 * ((xx // 64 + yy // 48) % 2), 0, 3900)
    raise ValueError(name)


def noisy(clean, a, b, black, rng, white=4095):
    """clean + Gaussian noise of variance a * max(clean - black, 0) + b DN^2, rounded and clipped to 0 .. white, uint16."""
    var = a * np.maximum(clean - black, 0) + b
    return np.clip(np.rint(clean + rng.standard_normal(clean.shape) * np.sqrt(var)), 0, white).astype(np.uint16)
