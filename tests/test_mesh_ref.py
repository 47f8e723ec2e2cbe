"""The numpy statement of the mesh warp (_mesh_ref) without a GPU: against a scalar one written straight from the header, the
properties the contract names (whole-sample translations are "mhc" cut, identity-linear-part meshes are the affine warp, flat frames,
neutral greys), affine_mesh against the affine warp's positions, and a distortion_mesh warp against a float64 evaluation of the
lens model."""
import numpy as np
import pytest

import _mesh_ref as MR
import _rgb_ref as R
import _warp_ref as W
import motioncam_decoder_amd as M

CFAS = ("rggb", "bggr", "grbg", "gbrg")
FILTERS = ("linear", "cubic")


def _reflect(i, n):
    i = -i if i < 0 else i
    return 2 * (n - 1) - i if i > n - 1 else i


def _scalar(e, mesh, size, filt):
    """The header's statement, one output pixel at a time, in Python integers."""
    _, H, Wd = e.shape
    T = W.table(filt)
    node = lambda a, b, c: int(mesh[a, b, c])

    def pos(i, k, c, side):
        a, u, b, v = i >> 5, i & 31, k >> 5, k & 31
        s = node(a, b, c) * (32 - u) * (32 - v) + node(a, b + 1, c) * (32 - u) * v + node(a + 1, b, c) * u * (32 - v) + node(a + 1, b + 1, c) * u * v
        return min(max((s + 512) >> 10, 0), 256 * (side - 1))

    out = np.zeros((3,) + size, dtype=np.int64)
    for i in range(size[0]):
        for k in range(size[1]):
            i0, k0 = i & ~31, k & ~31
            i1, k1 = min(i0 + 32, size[0]) - 1, min(k0 + 32, size[1]) - 1
            ys = [pos(ii, kk, 0, H) for ii in (i0, i1) for kk in (k0, k1)]
            xs = [pos(ii, kk, 1, Wd) for ii in (i0, i1) for kk in (k0, k1)]
            pb, eb = ((min(ys) >> 8) - 1) & ~1, ((min(xs) >> 8) - 1) & ~7
            npp, nee = min((((max(ys) >> 8) + 2 - pb) >> 1) + 1, 26), min((((max(xs) >> 8) + 2 - eb) >> 3) + 1, 8)
            Y, X = pos(i, k, 0, H), pos(i, k, 1, Wd)
            r = min(max((Y >> 8) - 1, pb), pb + 2 * npp - 4)
            c = min(max((X >> 8) - 1, eb), eb + 8 * nee - 4)
            wy, wx = [int(v) for v in T[Y & 255]], [int(v) for v in T[X & 255]]
            for ch in range(3):
                t = [(sum(wx[j] * int(e[ch, _reflect(r + rr, H), _reflect(c + j, Wd)]) for j in range(4)) + 2048) >> 12 for rr in range(4)]
                out[ch, i, k] = (sum(wy[rr] * t[rr] for rr in range(4)) + 2048) >> 12
    return out


def _hostile(size, H, Wd, seed):
    """A mesh with a tile far outside the regime and nodes outside the frame: both clamps act."""
    rng = np.random.default_rng(seed)
    mesh = MR.translation_mesh(size, 2, 3)
    mesh[0, 0] = (-256 * 9, -256 * 20)
    mesh[1, 1] = (256 * (H + 30), 256 * (Wd + 40))
    mesh[-1, -1] = rng.integers(-2 ** 31, 2 ** 31, 2)
    return mesh


@pytest.mark.parametrize("filt", FILTERS)
def test_numpy_statement_equals_the_scalar_one(filt):
    rng = np.random.default_rng(21)
    H, Wd, size = 80, 136, (37, 45)
    e = R.mhc_estimates(rng.integers(0, 4096, size=(H, Wd)).astype(np.uint16), (60, 64, 61, 70), "grbg")
    smooth = M.affine_mesh([70000, -9000, 256 * 14, 12000, 60000, 256 * 3 + 7], size)[0]
    hostile = _hostile(size, H, Wd, 5)
    assert MR.in_regime(smooth, size, H, Wd) and not MR.in_regime(hostile, size, H, Wd)
    Y, X, r, c = MR.tap_origins(hostile, size, H, Wd)
    Yr, Xr = MR.raw_positions(hostile, size)
    assert (Yr != Y).any() and (Xr != X).any() and ((Y >> 8) - 1 != r).any() and ((X >> 8) - 1 != c).any()  # every clamp acts
    for mesh in (smooth, hostile, MR.translation_mesh(size, 0.5, 90.25)):
        assert np.array_equal(MR.mesh_from_e(e, mesh, size, filt), _scalar(e, mesh, size, filt))


def test_whole_sample_translations_equal_mhc_cut():
    rng = np.random.default_rng(22)
    img = rng.integers(0, 4096, size=(48, 72)).astype(np.uint16)
    black = (60, 61, 62, 63)
    for cfa in CFAS:
        e = R.mhc_estimates(img, black, cfa)
        for (a, b), size in (((0, 0), (48, 72)), ((3, 5), (40, 66)), ((7, 0), (33, 8))):
            mesh = MR.translation_mesh(size, a, b)
            for filt in FILTERS:
                assert np.array_equal(MR.mesh_estimates(img, mesh, size, filt, black, cfa), e[:, a:a + size[0], b:b + size[1]]), (cfa, a, b, filt)
            want = R.ref_bits(img, "mhc", "f32", 4095.0, black=black, cfa=cfa, gain=(1.7, 1.0, 1.4))[:, a:a + size[0], b:b + size[1]]
            assert np.array_equal(MR.mesh_ref(img, mesh, size, "f32", 4095.0, "cubic", black, cfa, (1.7, 1.0, 1.4)), want)


def test_identity_linear_part_equals_the_affine_warp():
    rng = np.random.default_rng(23)
    img = rng.integers(0, 4096, size=(48, 72)).astype(np.uint16)
    e = R.mhc_estimates(img, (64, 64, 64, 64), "rggb")
    size = (37, 45)
    for ty, tx in ((0, 0), (77, 256 * 5 + 201), (256 * 10 + 255, 1), (256 * 11, 256 * 27)):
        m = (65536, 0, ty, 0, 65536, tx)
        mesh = M.affine_mesh(m, size)[0]
        Y, X = MR.positions(mesh, size, 48, 72)
        Yw, Xw = W.positions(m, size)
        assert np.array_equal(Y, Yw) and np.array_equal(X, Xw)
        for filt in FILTERS:
            assert np.array_equal(MR.mesh_from_e(e, mesh, size, filt), W.warp_from_e(e, m, size, filt)), (m, filt)


def test_flat_frames_stay_flat_and_greys_neutral():
    H, Wd, size = 48, 72, (37, 45)
    img = np.full((H, Wd), 1234, dtype=np.uint16)
    grey = np.zeros((H, Wd), dtype=np.uint16)
    for p, b in enumerate((60, 70, 80, 90)):
        grey[p >> 1::2, p & 1::2] = 1000 + b
    meshes = (M.affine_mesh([60000, -9000, 256 * 9, 12000, 70000, 13], size)[0], _hostile(size, H, Wd, 6),
              M.distortion_mesh(H, Wd, size, radial=(1.0, -0.08, 0.01, 0.0)))
    for filt in FILTERS:
        for mesh in meshes:
            assert (MR.mesh_estimates(img, mesh, size, filt, (64, 64, 64, 64), "grbg") == 16 * (1234 - 64)).all()
            assert (MR.mesh_estimates(grey, mesh, size, filt, (60, 70, 80, 90), "bggr") == 16000).all()


def test_affine_mesh_is_within_a_step_of_the_affine_positions():
    """Bilinear interpolation of an affine function is the function; the nodes carry warp_pos's rounding (1/512 sample) and the
    interpolation rounds once more (1/512): at most 1/256 sample, and nothing where the linear part is the identity."""
    rng = np.random.default_rng(24)
    size = (70, 100)
    worst = 0
    for it in range(200):
        lin = 65536 * np.array([1, 0, 0, 1]) + rng.integers(-16384, 16385, 4) * (it % 3 != 0)
        m = (int(lin[0]), int(lin[1]), int(rng.integers(0, 4096)), int(lin[2]), int(lin[3]), int(rng.integers(0, 4096)))
        mesh = M.affine_mesh(m, size)[0]
        Yr, Xr = MR.raw_positions(mesh, size)
        Yw, Xw = W.positions(m, size)
        d = max(int(np.abs(Yr - Yw).max()), int(np.abs(Xr - Xw).max()))
        worst = max(worst, d)
        assert d <= 1, (m, d)
        if it % 3 == 0:
            assert d == 0
    assert worst == 1


def test_distortion_mesh_warp_against_the_float64_model():
    """A linear image g = gy y + gx x + g0 behind the linear filter: the table interpolates it exactly at the quantised position, so
    E / 16 = g(Y / 256, X / 256) up to the two roundings (1/16 DN in all).  The position is off the model's by at most
        d = h^2 / 8 * (max |s_ii| + max |s_kk|) + 1/512 + 1/512        (bilinear interpolation over a cell of h = 32 output pixels,
                                                                        the nodes' rounding, the interpolation's rounding)
    per axis.  With d = (q - c) / m, |d| <= 1 and F = (k0 + k1 r^2 + k2 r^4) dy: F_yy = k1 6 dy + k2 (8 dy^3 + 12 r^2 dy),
    F_xx = k1 2 dy + k2 (8 dx^2 dy + 4 r^2 dy), so |s_ii| + |s_kk| <= (8 |k1| + 32 |k2|) / m.  Nothing here is fitted."""
    H, Wd, size = 200, 296, (150, 230)
    k = (1.0, -0.06, 0.015, 0.0)
    mesh = M.distortion_mesh(H, Wd, size, radial=k)
    Yr, Xr = MR.raw_positions(mesh, size)
    assert Yr.min() >= 0 and Yr.max() <= 256 * (H - 1) and Xr.min() >= 0 and Xr.max() <= 256 * (Wd - 1) and MR.in_regime(mesh, size, H, Wd)
    py, px = 0.5 * (H - 1), 0.5 * (Wd - 1)
    m = np.hypot(py, px)
    qy = np.arange(size[0], dtype=np.float64)[:, None] + (H - size[0]) // 2
    qx = np.arange(size[1], dtype=np.float64)[None, :] + (Wd - size[1]) // 2
    dy, dx = (qy - py) / m, (qx - px) / m
    r2 = dx * dx + dy * dy
    f = k[0] + k[1] * r2 + k[2] * r2 * r2
    sy, sx = py + m * f * dy, px + m * f * dx
    delta = 32.0 ** 2 / 8.0 * (8 * abs(k[1]) + 32 * abs(k[2])) / m + 1.0 / 256
    perr = max(np.abs(Yr / 256.0 - sy).max(), np.abs(Xr / 256.0 - sx).max())
    print("position: max error %.5f sample, bound %.5f" % (perr, delta))
    assert perr <= delta
    gy, gx, g0 = 3.0, -2.0, 2000.0
    yy, xx = np.mgrid[0:H, 0:Wd]
    e = np.broadcast_to((16 * (gy * yy + gx * xx + g0)).astype(np.int64), (3, H, Wd))
    E = MR.mesh_from_e(e, mesh, size, "linear")
    err = np.abs(E / 16.0 - (gy * sy + gx * sx + g0)).max()
    tol = (abs(gy) + abs(gx)) * delta + 1.0 / 16
    print("image: max error %.4f DN, bound %.4f" % (err, tol))
    assert err <= tol
