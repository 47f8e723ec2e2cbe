"""The host helpers in front of algo="warp" (quantize_affine, fit_affine, stabilize), without a GPU: numpy float64 against their
definitions, and a round trip through the numpy statements of the cell-wise alignment and of the warp."""
import numpy as np
import pytest

import _align_cells_ref as AC
import _warp_ref as W
import motioncam_decoder_amd as M


def test_quantize_affine_rounds_half_up():
    a = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]])
    assert M.quantize_affine(a).tolist() == list(W.IDENTITY) and M.quantize_affine(a).dtype == np.int32
    h = 0.5 / 65536
    a = np.array([[1 + h, -h, 1.5 / 256], [h, 1 - h, -1.5 / 256]])  # exact halves: floor(v + 0.5), not round-to-even, not truncation
    assert M.quantize_affine(a).tolist() == [65537, 0, 2, 1, 65536, -1]
    a = np.array([[[0.99, 0.01, 3.3], [-0.01, 1.2, -7.7]]] * 3)
    q = M.quantize_affine(a)
    assert q.shape == (3, 6) and q[1].tolist() == [int(np.floor(0.99 * 65536 + 0.5)), int(np.floor(0.01 * 65536 + 0.5)),
                                                  int(np.floor(3.3 * 256 + 0.5)), int(np.floor(-0.01 * 65536 + 0.5)),
                                                  int(np.floor(1.2 * 65536 + 0.5)), int(np.floor(-7.7 * 256 + 0.5))]
    for bad in (np.zeros((3, 2)), np.zeros((2, 2, 2, 3)), np.full((2, 3), np.nan), np.full((2, 3), 1e6)):
        with pytest.raises(ValueError):
            M.quantize_affine(bad)


def test_fit_affine_recovers_an_exact_field():
    cell = (64, 256)
    cy, cx = 6, 5
    h, w = cy * 64, cx * 256
    assert M.cell_grid(h, w, cell) == (cy, cx)
    i, j = np.mgrid[0:cy, 0:cx]
    field = np.zeros((3, cy, cx, 2), dtype=np.int16)
    field[1, :, :, 0], field[1, :, :, 1] = 2 * (j - 2), -2 * (i - 3)     # dy = 2 (j - j0), dx = -2 (i - i0): a roll
    field[2, :, :, 0], field[2, :, :, 1] = 4 * i + 2 * j - 6, 2 * j + 8  # zoom, shear and a shift
    D = M.fit_affine(field, h, w, cell)
    assert D.shape == (3, 2, 3) and D.dtype == np.float64
    want = np.zeros((3, 2, 3))
    # j = (x - 128) / 256, i = (y - 32) / 64
    want[1] = [[0.0, 2 / 256, 2 * (-128 / 256 - 2)], [-2 / 64, 0.0, -2 * (-32 / 64 - 3)]]
    want[2] = [[4 / 64, 2 / 256, 4 * (-32 / 64) + 2 * (-128 / 256) - 6], [0.0, 2 / 256, 2 * (-128 / 256) + 8]]
    assert np.abs(D - want).max() <= 1e-9
    # a single shift per frame: no linear part
    pos = np.array([[0, 0], [4, -6], [-2, 8]], dtype=np.int16)
    D = M.fit_affine(pos, h, w)
    assert D.shape == (3, 2, 3) and (D[:, :, :2] == 0).all() and np.array_equal(D[:, :, 2], pos.astype(np.float64))
    for bad in (dict(pos=field, cell=None), dict(pos=field[:, :5], cell=cell), dict(pos=np.zeros((3, 3)), cell=None), dict(pos=pos, cell=cell)):
        with pytest.raises(ValueError):
            M.fit_affine(bad["pos"], h, w, bad["cell"])


def test_stabilize_pure_translation_and_limit():
    h, w, size = 96, 512, (80, 480)
    pos = np.array([[0, 0], [4, -6], [-2, 8], [9, 17]], dtype=np.float64)
    D = M.fit_affine(pos, h, w)
    maps = M.stabilize(D, h, w, size, limit=False)
    assert maps.dtype == np.int32 and maps.shape == (4, 6)
    assert np.array_equal(maps[:, [0, 1, 3, 4]], np.tile([65536, 0, 0, 65536], (4, 1)))  # the identity linear part
    assert np.array_equal(maps[:, 2], 256 * (pos[:, 0] + 8)) and np.array_equal(maps[:, 5], 256 * (pos[:, 1] + 16))  # pos + the centring offset
    # window: what stays is the running mean
    sm = M.stabilize(D, h, w, size, window=1, limit=False)
    mean = np.array([pos[max(0, t - 1):t + 2].mean(axis=0) for t in range(4)])
    assert np.array_equal(sm[:, 2], np.floor((pos[:, 0] - mean[:, 0] + 8) * 256 + 0.5)) and np.array_equal(sm[:, 5], np.floor((pos[:, 1] - mean[:, 1] + 16) * 256 + 0.5))
    # limit: the corners stay inside, the frames that were inside stay as they were
    lim = M.stabilize(D, h, w, size)
    for t in range(4):
        assert W.map_ok(lim[t], size, h, w)
        assert W.map_ok(maps[t], size, h, w) == np.array_equal(lim[t], maps[t])
    assert not W.map_ok(maps[3], size, h, w) and lim[3].tolist() == [65536, 0, 256 * 16, 0, 65536, 256 * 32]
    # with roll: the translation is clamped, the linear part stays
    roll = np.zeros((2, 2, 3))
    roll[1] = [[0.0, 0.02, -30.0], [-0.02, 0.0, 40.0]]
    lim = M.stabilize(roll, h, w, (64, 400))
    free = M.stabilize(roll, h, w, (64, 400), limit=False)
    assert W.map_ok(lim[1], (64, 400), h, w) and not W.map_ok(free[1], (64, 400), h, w)
    assert np.array_equal(lim[1, [0, 1, 3, 4]], free[1, [0, 1, 3, 4]]) and np.array_equal(lim[0], free[0])
    # no translation can hold the corners inside / a linear part beyond the library's bounds
    with pytest.raises(ValueError):
        M.stabilize(roll * 5, h, w, (94, 500))  # 0.1 * 499 columns lift the rows by more than the 2 to spare
    big = np.zeros((1, 2, 3))
    big[0, 0, 0] = 0.3
    with pytest.raises(ValueError):
        M.stabilize(big, h, w, (32, 32))
    with pytest.raises(ValueError):
        M.stabilize(roll, h, w, (97, 512))
    assert M.stabilize(big, h, w, (32, 32), limit=False)[0, 0] == int(np.floor(1.3 * 65536 + 0.5))


def _grey_e(img):
    return np.repeat(16 * np.asarray(img, dtype=np.int64)[None], 3, axis=0)


def _sample(img, m, size):
    """A grey image through the statement's sampling (warp_from_e on 16 x the image in every channel), rounded back to DN."""
    return ((W.warp_from_e(_grey_e(img), m, size, "cubic")[1] + 8) >> 4).astype(np.uint16)


TEXTURE = ((300.0, 2 * np.pi / 40, 2 * np.pi / 90, 0.3), (250.0, -2 * np.pi / 64, 2 * np.pi / 48, 1.1), (200.0, 2 * np.pi / 110, -2 * np.pi / 36, 2.0))


def test_round_trip_align_cells_fit_stabilize_warp():
    """Noise-free 96 x 512 frames: a base of three plane waves, f = 2000 + sum A sin(a y + b x + phi), sampled along known rolls by
    the statement; _align_cells_ref against frame 0, fit_affine, stabilize, and the statement again bring every frame back onto
    frame 0's window.  Nothing below is a chosen number.

    The position term, from the field's even quantisation.  A cell's entry is an even number of samples: the even number
    nearest to the cell's true displacement is at most 1 sample off per axis (asserted for every cell; the search finds it on
    this texture).  The least-squares fit is linear in the entries, so at position q its error is at most L(q), the absolute row
    sum of the fit's prediction matrix a(q)^T (A^T A)^-1 A^T over the cell centres, times that 1; the four corners of the output
    window bound it (asserted: the fit's error at the corners against the known maps).  The map's own quantisation adds 1/128
    sample (1/512 for the translation, 1/512 for the linear part at the far corner, both axes' terms).  A position error of d
    samples per axis moves the read position in the base by at most m d, m the largest absolute row sum of the frames' linear
    parts, and the base's slopes gy = sum A |a| and gx = sum A |b| turn that into DN:  m (L + 1/128) (gy + gx).
    The sampling term, twice (base -> frame, frame -> output).  Catmull-Rom reproduces quadratics, so against the function itself
    a sampling errs by the Taylor remainder, at most C3 (M3y + M3x) S m^3 with C3 = max_p sum_j |w_j(p)| |j - p|^3 / 6 from the
    table, M3y = sum A |a|^3, M3x = sum A |b|^3 and S = max_p sum |w| / 4096 for the other axis's pass; the position's own
    quantisation of 1/512 sample per axis, (gy + gx) m / 512; and 1 DN for the roundings (two of 1/16 DN inside, one to whole DN).
    The second sampling also carries the first one's error through its taps: times S.  tol = position + (1 + S) sampling.
    Measured here: every entry within 0.90 sample of the truth, L = 2.00 at the worst corner and a fit error of 0.93 sample
    there; a sampling term of 1.7 DN; stabilised frames within 101, 77 and 43 DN of frame 0's window under a tolerance of 354 DN;
    unstabilised they differ from it by 902, 1033 and 605 DN."""
    H, Wd, cell = 96, 512, (32, 256)
    yy, xx = np.mgrid[0:160, 0:640].astype(np.float64)
    base = np.round(2000.0 + sum(A * np.sin(a * yy + b * xx + ph) for A, a, b, ph in TEXTURE)).astype(np.uint16)
    gy, gx = sum(A * abs(a) for A, a, b, _ in TEXTURE), sum(A * abs(b) for A, a, b, _ in TEXTURE)
    m3y, m3x = sum(A * abs(a) ** 3 for A, a, b, _ in TEXTURE), sum(A * abs(b) ** 3 for A, a, b, _ in TEXTURE)
    # frame t reads the base at M_t q + c_t: frame 0 the centred window, the others rolled and shifted about it
    fm = np.array([[[1.0, 0.0, 32.0], [0.0, 1.0, 64.0]],
                   [[1.0, 0.012, 31.0], [-0.012, 1.0, 75.0]],
                   [[1.0, -0.016, 44.0], [0.016, 1.0, 55.0]],
                   [[1.004, 0.008, 27.0], [-0.008, 1.004, 70.0]]])
    fmaps = M.quantize_affine(fm)
    frames = np.stack([_sample(base, m, (H, Wd)) for m in fmaps])
    pos = AC.align_cells(frames, cell=cell, levels=3, radius=2, ref=0)[0]
    cy, cx = M.cell_grid(H, Wd, cell)
    assert pos.shape == (4, cy, cx, 2) and (pos[0] == 0).all() and (pos % 2 == 0).all()
    # the true displacement: in[t][q + d] looks like in[0][q], so M_t (q + d) + c_t = q + c_0
    ci, cj = np.mgrid[0:cy, 0:cx]
    centres = np.stack([ci * cell[0] + cell[0] / 2.0, cj * cell[1] + cell[1] / 2.0], axis=-1).reshape(-1, 2)

    def true_d(t, q):
        A = fmaps[t].astype(np.float64)
        Mt = np.array([[A[0], A[1]], [A[3], A[4]]]) / 65536.0
        ct = np.array([A[2], A[5]]) / 256.0
        return np.linalg.solve(Mt, (q + np.array([32.0, 64.0]) - ct).T).T - q

    worst_entry = max(np.abs(pos[t].reshape(-1, 2) - true_d(t, centres)).max() for t in range(1, 4))
    print("largest |entry - true displacement at the cell's centre|: %.3f samples" % worst_entry)
    assert worst_entry <= 1.0
    D = M.fit_affine(pos, H, Wd, cell)
    size = (64, 448)
    off = np.array([(H - size[0]) // 2, (Wd - size[1]) // 2], dtype=np.float64)
    corners = np.array([[0, 0], [0, size[1] - 1], [size[0] - 1, 0], [size[0] - 1, size[1] - 1]], dtype=np.float64) + off
    A = np.concatenate([centres, np.ones((cy * cx, 1))], axis=1)
    L = np.abs(np.concatenate([corners, np.ones((4, 1))], axis=1) @ np.linalg.pinv(A)).sum(axis=1).max()
    fit_err = max(np.abs(corners @ D[t, :, :2].T + D[t, :, 2] - true_d(t, corners)).max() for t in range(1, 4))
    print("prediction matrix: largest absolute row sum at a corner %.3f; largest fit error at a corner %.3f samples" % (L, fit_err))
    assert fit_err <= L * 1.0 + 1e-9
    maps = M.stabilize(D, H, Wd, size)
    assert all(W.map_ok(m, size, H, Wd) for m in maps) and maps[0].tolist() == [65536, 0, 256 * 16, 0, 65536, 256 * 32]
    outs = [_sample(frames[t], maps[t], size).astype(np.int64) for t in range(4)]
    T = W.table("cubic") / 4096.0
    ph = np.arange(256)[:, None] / 256.0
    C3 = (np.abs(T) * np.abs(np.arange(-1, 3)[None, :] - ph) ** 3).sum(axis=1).max() / 6.0
    S = np.abs(T).sum(axis=1).max()
    m = max(np.abs(fm[:, :, :2]).sum(axis=2).max(), max(np.abs(maps[:, [0, 1]]).sum(axis=1).max(), np.abs(maps[:, [3, 4]]).sum(axis=1).max()) / 65536.0)
    sampling = C3 * (m3y + m3x) * S * m ** 3 + (gy + gx) * m / 512.0 + 1.0
    tol = m * (L + 1 / 128) * (gy + gx) + (1 + S) * sampling
    plain = [frames[t][16:80, 32:480].astype(np.int64) for t in range(4)]
    assert np.array_equal(outs[0], plain[0])
    for t in range(1, 4):
        err, before = np.abs(outs[t] - outs[0]).max(), np.abs(plain[t] - plain[0]).max()
        print("frame %d: stabilised |out - out0| max %d DN (tolerance %.1f: position %.1f, sampling %.2f); unstabilised %d DN"
              % (t, err, tol, tol - (1 + S) * sampling, sampling, before))
        assert err <= tol < before
