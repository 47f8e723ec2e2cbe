"""Inputs of the alignment tests (test_align_abi.py, test_gpu_align.py): crops of one textured scene at known even offsets."""
import numpy as np

import _align_ref as R


def _blur(a, k):
    """The k x k box mean, valid part."""
    c = np.cumsum(np.cumsum(np.pad(a, ((1, 0), (1, 0))), axis=0), axis=1)
    return (c[k:, k:] - c[:-k, k:] - c[k:, :-k] + c[:-k, :-k]) / (k * k)


def scene_frames(seed, H, W, levels, radius, k, n=5, noise=8.0, step=None):
    """(frames (n, H, W) uint16, offsets (n, 2)): crops of one textured scene (a box-blurred uniform field, scaled to 3000 DN
    over black 64, plus Gaussian noise) at even offsets whose steps are uniform in -2 B(0) .. 2 B(0)."""
    rng = np.random.default_rng(seed)
    B0 = R.bounds(levels, radius)[0]
    steps = 2 * rng.integers(-B0, B0 + 1, size=(n - 1, 2)) if step is None else np.tile(np.asarray(step), (n - 1, 1))
    off = np.concatenate([np.zeros((1, 2), np.int64), np.cumsum(steps, axis=0)])
    off -= off.min(axis=0)
    sh, sw = H + int(off[:, 0].max()), W + int(off[:, 1].max())
    f = _blur(rng.random((sh + k - 1, sw + k - 1)), k)
    scene = 64.0 + 3000.0 * (f - f.min()) / (f.max() - f.min())
    frames = np.stack([scene[oy:oy + H, ox:ox + W] for oy, ox in off])
    if noise:
        frames = frames + noise * rng.standard_normal(frames.shape)
    return np.clip(np.rint(frames), 0, 65535).astype(np.uint16), off


def clamp_frames(n):
    """n frames of 40 x 40 cut from a noise-free strip that moves 16 samples per frame: d(t | t - 1) = (0, -8) at levels 1,
    radius 8, so pos[t].x = -16 t until it is clamped (from frame 2048 on)."""
    return scene_frames(77, 40, 40, 1, 8, 9, n, noise=0.0, step=(0, 16))
