"""Inputs of the position-field tests (test_align_cells_abi.py, test_gpu_align_cells.py, test_gpu_merge_cells.py): frames whose
left and right halves are cut from one textured scene at different known even offsets, so the seam lies where the caller puts it."""
import numpy as np

from _align_scenes import _blur


def halves_frames(seed, H, W, k, n=4, reach=8, noise=0.0, seam=None):
    """(frames (n, H, W) uint16, off (n, 2, 2)): columns 0 .. seam - 1 of frame t show the scene at offset off[t, 0], the columns
    from seam (default W // 2) on at off[t, 1]; the steps of either half are even, uniform in -reach .. reach and never equal in
    both halves.  The scene is a k x k box-blurred uniform field scaled to 3000 DN over black 64, plus Gaussian noise."""
    rng = np.random.default_rng(seed)
    seam = W // 2 if seam is None else seam
    steps = np.zeros((n - 1, 2, 2), np.int64)
    for t in range(n - 1):
        while True:
            steps[t] = 2 * rng.integers(-(reach // 2), reach // 2 + 1, size=(2, 2))
            if (steps[t, 0] != steps[t, 1]).any():
                break
    off = np.concatenate([np.zeros((1, 2, 2), np.int64), np.cumsum(steps, axis=0)])
    off -= off.min(axis=(0, 1))
    sh, sw = H + int(off[..., 0].max()), W + int(off[..., 1].max())
    f = _blur(rng.random((sh + k - 1, sw + k - 1)), k)
    scene = 64.0 + 3000.0 * (f - f.min()) / (f.max() - f.min())
    frames = np.empty((n, H, W))
    for t in range(n):
        (ly, lx), (ry, rx) = off[t]
        frames[t, :, :seam] = scene[ly:ly + H, lx:lx + seam]
        frames[t, :, seam:] = scene[ry:ry + H, rx + seam:rx + W]
    if noise:
        frames = frames + noise * rng.standard_normal(frames.shape)
    return np.clip(np.rint(frames), 0, 65535).astype(np.uint16), off


def halves_field(off, cells_y, cells_x, seam_cell):
    """The chain's field (n, cells_y, cells_x, 2) that the halves' offsets give: the cell columns below seam_cell follow the left
    half, the others the right one (pos[t] - pos[t - 1] = off[t - 1] - off[t], pos[0] = 0)."""
    n = len(off)
    pos = off[:1] - off  # (n, 2 halves, 2)
    out = np.empty((n, cells_y, cells_x, 2), np.int64)
    out[:, :, :seam_cell] = pos[:, None, None, 0]
    out[:, :, seam_cell:] = pos[:, None, None, 1]
    return out
