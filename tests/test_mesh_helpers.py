"""The host-side helpers of algo="mesh" (mesh_grid, affine_mesh, distortion_mesh, stabilize_mesh, mesh_check): no GPU."""
import numpy as np
import pytest

import _mesh_ref as MR
import motioncam_decoder_amd as M


def test_mesh_grid():
    assert M.mesh_grid(1, 1) == (2, 2) and M.mesh_grid(32, 32) == (2, 2) and M.mesh_grid(33, 64) == (3, 3)
    assert M.mesh_grid(40, 70) == (3, 4) == MR.grid((40, 70)) and M.mesh_grid(1944, 3456) == (62, 109) and M.mesh_grid(65536, 65536) == (2049, 2049)
    for bad in ((0, 5), (5, 65537), (2.5, 4), (True, 4)):
        with pytest.raises(ValueError):
            M.mesh_grid(*bad)


def test_affine_mesh_shapes_and_nodes():
    size = (40, 70)
    m = np.array([[70000, -9000, 256 * 14, 12000, 60000, 775], [65536, 0, 3, 0, 65536, 9]], dtype=np.int32)
    mesh = M.affine_mesh(m, size)
    assert mesh.shape == (2, 3, 4, 2) and mesh.dtype == np.int32 and mesh.flags["C_CONTIGUOUS"]
    for f in range(2):
        for a in range(3):
            for b in range(4):
                i, k = 32 * a, 32 * b
                assert mesh[f, a, b, 0] == m[f, 2] + ((int(m[f, 0]) * i + int(m[f, 1]) * k + 128) >> 8)
                assert mesh[f, a, b, 1] == m[f, 5] + ((int(m[f, 3]) * i + int(m[f, 4]) * k + 128) >> 8)
    assert M.affine_mesh(m[0], size).shape == (1, 3, 4, 2)
    f = M.affine_mesh(np.array([[1.0, 0.0, 2.5], [0.0, 1.0, 3.25]]), size)  # float maps are quantised first
    assert np.array_equal(f, M.affine_mesh([65536, 0, 640, 0, 65536, 832], size))


def test_distortion_mesh_without_distortion_is_the_centred_window():
    for (h, w), size in (((72, 136), (40, 70)), ((3024, 4032), (1944, 3456)), ((37, 51), (36, 51))):
        oy, ox = (h - size[0]) // 2, (w - size[1]) // 2
        want = M.affine_mesh([65536, 0, 256 * oy, 0, 65536, 256 * ox], size)[0]
        for center in ((0.5, 0.5), (0.3, 0.81)):
            assert np.array_equal(M.distortion_mesh(h, w, size, radial=(1, 0, 0, 0), center=center), want), (h, w, center)
    # with stabilise maps in front: their positions, one mesh per map
    maps = np.array([[65536, 0, 256 * 3 + 7, 0, 65536, 256 * 5], [65536, 0, 11, 0, 65536, 256 * 9 + 200]], dtype=np.int32)
    got = M.distortion_mesh(72, 136, (40, 70), affine=maps)
    assert got.shape == (2, 3, 4, 2) and np.array_equal(got, M.affine_mesh(maps, (40, 70)))
    assert M.distortion_mesh(72, 136, (40, 70), affine=maps[0]).shape == (3, 4, 2)


def test_distortion_mesh_model():
    """Against the DNG formula written out per node in Python floats."""
    import math
    h, w, size = 120, 200, (100, 170)
    k, kt, (cx, cy) = (0.98, -0.07, 0.02, -0.004), (0.003, -0.002), (0.48, 0.53)
    mesh = M.distortion_mesh(h, w, size, radial=k, tangential=kt, center=(cx, cy))
    px, py = cx * (w - 1), cy * (h - 1)
    m = max(math.hypot(px - x, py - y) for x in (0, w - 1) for y in (0, h - 1))
    for a in range(mesh.shape[0]):
        for b in range(mesh.shape[1]):
            dy, dx = (32 * a + (h - size[0]) // 2 - py) / m, (32 * b + (w - size[1]) // 2 - px) / m
            r2 = dx * dx + dy * dy
            f = k[0] + k[1] * r2 + k[2] * r2 ** 2 + k[3] * r2 ** 3
            sx = px + m * (f * dx + 2 * kt[0] * dx * dy + kt[1] * (r2 + 2 * dx * dx))
            sy = py + m * (f * dy + kt[0] * (r2 + 2 * dy * dy) + 2 * kt[1] * dx * dy)
            assert abs(int(mesh[a, b, 0]) - 256 * sy) <= 0.5 + 1e-6 and abs(int(mesh[a, b, 1]) - 256 * sx) <= 0.5 + 1e-6


def test_stabilize_mesh_of_an_affine_field():
    """A field that is exactly affine: bilinear interpolation between the cell centres and the linear continuation reproduce it, so
    the nodes are 256 (q + D(q)) rounded once (1/2 unit of 1/256 sample).  affine_mesh(stabilize(fit_affine(field))) carries the
    linear part's quantisation, 2^-17 per coefficient times the node's coordinates, the translation's (1/2 unit) and warp_pos's
    rounding (1/2 unit): in all 1.5 + 256 (i + k) 2^-17 units at node (i, k), beside the least-squares fit's float error."""
    h, w, cell, size = 256, 1024, (64, 256), (200, 900)
    cy, cx = M.cell_grid(h, w, cell)
    yc = (np.arange(cy) * 64 + 32.0)[:, None]
    xc = (np.arange(cx) * 256 + 128.0)[None, :]
    n = 4
    rng = np.random.default_rng(3)
    lin = rng.uniform(-0.01, 0.01, size=(n, 2, 2))
    tr = rng.uniform(-3, 3, size=(n, 2))
    field = np.stack([np.stack([lin[t, c, 0] * yc + lin[t, c, 1] * xc + tr[t, c] for c in range(2)], axis=-1) for t in range(n)])
    for window in (0, 1):
        got = M.stabilize_mesh(field, h, w, cell, size, window=window)
        want = M.affine_mesh(M.stabilize(M.fit_affine(field, h, w, cell), h, w, size, window=window, limit=False), size)
        assert got.shape == want.shape == (n,) + M.mesh_grid(*size) + (2,)
        i = 32.0 * np.arange(got.shape[1])[:, None, None]
        k = 32.0 * np.arange(got.shape[2])[None, :, None]
        bound = 1.5 + 256.0 * (i + k) / 131072.0 + 1e-3
        err = np.abs(got.astype(np.int64) - want)
        print("window %d: max node difference %d units of 1/256, bound %.2f .. %.2f" % (window, err.max(), bound.min(), bound.max()))
        assert (err <= bound[None]).all()
    # one cell along an axis: constant there
    one = M.stabilize_mesh(np.full((1, 1, 1, 2), 1.5), 64, 256, cell, (40, 70))
    assert np.array_equal(one[0], MR.translation_mesh((40, 70), 12 + 1.5, 93 + 1.5))


def test_value_errors():
    size = (40, 70)
    good = MR.translation_mesh(size, 2, 4)
    with pytest.raises(ValueError):
        M.affine_mesh(np.zeros((3, 5), np.int32), size)
    with pytest.raises(ValueError):
        M.affine_mesh([65536, 0, 0, 0, 65536, 0], (0, 70))
    with pytest.raises(ValueError):
        M.affine_mesh([65536, 0, 0, 0, 65536, 0], 40)
    with pytest.raises(ValueError):
        M.affine_mesh([2 ** 31 - 1, 0, 2 ** 31 - 1, 0, 65536, 0], (65536, 70))  # a node leaves int32
    with pytest.raises(ValueError):
        M.distortion_mesh(72, 136, size, radial=(1, 0, 0))
    with pytest.raises(ValueError):
        M.distortion_mesh(72, 136, size, tangential=(0,))
    with pytest.raises(ValueError):
        M.distortion_mesh(72, 136, size, center="x")
    with pytest.raises(ValueError):
        M.distortion_mesh(72, 136, size, radial=(float("nan"), 0, 0, 0))
    with pytest.raises(ValueError):
        M.distortion_mesh(72, 136, size, radial=(1e9, 0, 0, 0))
    with pytest.raises(ValueError):
        M.distortion_mesh(72, 136, size, affine=np.zeros((2, 5), np.int32))
    field = np.zeros((2, 2, 1, 2))
    with pytest.raises(ValueError):
        M.stabilize_mesh(field, 128, 256, (64, 256), (200, 70))  # larger than the frame
    with pytest.raises(ValueError):
        M.stabilize_mesh(field[:, :1], 128, 256, (64, 256), size)  # not the cell grid
    with pytest.raises(ValueError):
        M.stabilize_mesh(field, 128, 256, (64, 256), size, window=-1)
    with pytest.raises(ValueError):
        M.stabilize_mesh(field, 128, 256, (60, 256), size)  # cell_grid's own rule
    torn = field.copy()
    torn[1, 1, 0, 0] = 90.0   # the lower cells 90 samples further down than the upper ones: 64 output rows read 154
    with pytest.raises(ValueError, match=r"stabilize_mesh: mcraw_mesh_check: the mesh of frame 1: tile \("):
        M.stabilize_mesh(torn, 128, 256, (64, 256), (100, 70))
    assert M.stabilize_mesh(torn, 128, 256, (64, 256), (100, 70), limit=False).shape == (2, 5, 4, 2)
    M.mesh_check(good, 72, 136, size)
    M.mesh_check(np.stack([good, good]), 72, 136, size, inside=True)
    for bad in (good.astype(np.int64), good[:2], good[None, None], np.zeros((0, 3, 4, 2), np.int32)):
        with pytest.raises(ValueError, match="mesh_check: mesh must be int32"):
            M.mesh_check(bad, 72, 136, size)
    with pytest.raises(ValueError, match="leaves the frame"):
        M.mesh_check(MR.translation_mesh(size, -1, 4), 72, 136, size, inside=True)
    with pytest.raises(ValueError, match="width and height must be even"):
        M.mesh_check(good, 71, 136, size)
    wide = good.copy()
    wide[:, 1:, 1] += 256 * 100
    with pytest.raises(ValueError, match=r"tile \(0, 0\) reads"):
        M.mesh_check(wide, 120, 328, size)
