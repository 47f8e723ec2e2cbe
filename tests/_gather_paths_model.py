"""The corpus and the exact model of the path census of krgb_warp (csrc/mcraw_warp.hip), krgb_mesh (csrc/mcraw_mesh.hip) and krgb_ha
(csrc/mcraw_ha.hip): tests/test_gpu_warp_paths.py, test_gpu_mesh_paths.py, test_gpu_ha_paths.py and tests/test_gather_paths_model.py.

The counters are the tail of RgbPath (csrc/mcraw_rgb_paths.h; PATHS is tests/_rgb_paths_model.py's, one order for the family).  All
of this is integer arithmetic: warp_window, mesh_lerp64, mesh_narrow, mesh_clamp, mesh_window, mesh_tap_max_* and reflect101 as
the headers state them (tests/cpp/gather_paths_plan.cpp prints the headers' own values for the CPU test), the staging of a tile,
the lane-to-pixel maps of phase A, the gather and the store phase, krgb_ha's tile with its green items.  Every counter is
predicted exactly.  krgb_ha's choices follow the samples: the model evaluates ha_green's two gradients at every site a tile
computes -- the ring, and the sites a partial tile computes outside the frame from reflected samples --, and takes the diagonal
choice of the frame's own R / B sites from _ha_ref.

A gather lane holds 4 columns and computes all 4 whenever its first lies in the tile: in a tile whose width 4 does not divide,
up to 3 positions past the tile's last column are evaluated, gathered and dropped by the store phase.  They are counted as the
kernel counts them (pixel-wise counters run over 4 x the lanes with pixels).

cases(kernel): the corpus.  The first 16 (krgb_ha: 8) are the cases the three modules always ran -- 3 frames of 2 x 3 tiles with
per-frame maps / meshes and colours, the four kinds with a LUT x the four CFAs x both filters, LUTs of 4096 and 65536 entries --;
behind them what the census asked for: the input with its pitch off the 16-byte grid and with its base one sample off, the output
one sample behind its grid, windows over each of the four frame edges, the 8 x 8 mosaic onto 2 x 2, a mesh with a cell that is
not narrow in Y and one not narrow in X, 34 one-tile frames (a launch takes RGB_MAXF = 32), and the float kinds (no loop: the
variants without a grid cap only)."""
import functools

import numpy as np

import _ha_ref as HA
import _mesh_ref as MR
import _rgb_paths_model as T
import _rgb_ref as R
import _warp_ref as W

PATHS, VARIANT_CAP, PRODUCT_OF, ES, RGB_T, RGB_MAXF = T.PATHS, T.VARIANT_CAP, T.PRODUCT_OF, T.ES, T.RGB_T, T.RGB_MAXF
WARP_TW = WARP_TH = 32
WARP_EROWS, WARP_ECOLS = 52, 64
MESH_NP, MESH_NE, MESH_NARROW = WARP_EROWS // 2, WARP_ECOLS // 8, 1 << 21
MHC_TW, MHC_TH = T.MHC_TW, T.MHC_TH
HA_RAWW, HA_RAWH = MHC_TW + 16, MHC_TH + 6
HA_RAWCH, HA_GH = HA_RAWW // 8, MHC_TH + 2
HA_STAGE_ITEMS, HA_G_MAIN, HA_G_EDGE = HA_RAWH * HA_RAWCH, HA_GH // 2 * (MHC_TW // 8), HA_GH
POISON = {"s_raw": 0x5a5a5a5b, "s_e": 0x005a5a5b, "s_g": 0x05a5a5a5}  # what the poisoned builds fill in (the sources say why)
CFAS = T.CFAS
IN_BITS = 11

# ---- the corpus

SIZE, FRAME, N = (40, 70), (72, 136), 3           # 2 x 3 tiles of 32 x 32; the last lane of a row holds 6 of its 8 columns
HA_FRAME = (40, 520)                              # 2 x 3 tiles of 256 x 32: the last row 8 high, the last column 8 wide
GW = dict(white=4095.0, black=(60, 61, 62, 63))   # krgb_warp and krgb_mesh
HW = dict(white=3.5, black=(3, 1, 2, 3))          # krgb_ha


def _case(kernel, kind, cfa, lutn, geo, filt=None, size=None, frame=None, n=N, in_align=0, out_off=0, tag=""):
    frame = frame or (HA_FRAME if kernel == "ha" else FRAME)
    size = frame if kernel == "ha" else (size or SIZE)
    S = dict(kernel=kernel, kind=kind, cfa=cfa, lutn=lutn, geo=geo, filt=filt, size=tuple(size), H=frame[0], W=frame[1], n=n,
             in_align=in_align, out_off=out_off, in_bits=IN_BITS, **(HW if kernel == "ha" else GW))
    S["name"] = "-".join(str(v) for v in (kernel, kind, cfa, filt or "ha", lutn, geo, "i%d" % in_align, "o%d" % out_off, "n%d" % n) if v != "") + tag
    S["off"], S["pitch"], S["fstride"] = T._layout(S["W"], S["H"], n, in_align)
    S["img"] = "img_%s_%d_%d_%d" % ("ha" if kernel == "ha" else "g", n, S["H"], S["W"])
    return S


@functools.lru_cache(maxsize=None)
def cases(kernel):
    out = []
    kinds = ("u8hwc", "u16chw", "nv12", "p010")
    for c, cfa in enumerate(("rggb", "bggr", "grbg", "gbrg")):
        for k, kind in enumerate(kinds):
            if kernel == "ha":
                if (c + k) % 2 == 0:  # two kinds per CFA: every kind with two CFAs
                    out.append(_case("ha", kind, cfa, 65536 if (c + k) % 4 == 2 else 4096, ""))
            else:
                out.append(_case(kernel, kind, cfa, 65536 if (c + k) % 4 == 1 else 4096, "main", "linear" if (c + k) % 4 == 3 else "cubic"))
    if kernel == "ha":
        out += [_case("ha", "u8chw", "grbg", 4096, "", in_align=1, out_off=1), _case("ha", "p010", "rggb", 4096, "", in_align=2),
                _case("ha", "u16hwc", "bggr", 65536, "", in_align=1, out_off=2), _case("ha", "nv12", "gbrg", 4096, "", out_off=1),
                _case("ha", "u8chw", "rggb", 4096, "", frame=(8, 16), n=34)]
        out += [_case("ha", kind, CFAS[i], 0, "", n=2, in_align=i, out_off=ES[kind] * (i % 2)) for i, kind in enumerate(T.FLOAT_KINDS)]
    else:
        out += [_case(kernel, "u8chw", "grbg", 4096, "main", "cubic", in_align=1, out_off=1),
                _case(kernel, "p010", "rggb", 4096, "main", "linear", in_align=2),
                _case(kernel, "u16hwc", "bggr", 65536, "main", "cubic", in_align=1, out_off=2),
                _case(kernel, "nv12", "gbrg", 4096, "main", "cubic", out_off=1),
                _case(kernel, "u16chw", "rggb", 4096, "edges", "cubic"),
                _case(kernel, "u8hwc", "gbrg", 4096, "edges", "linear", n=2, in_align=1),
                _case(kernel, "nv12", "bggr", 4096, "tiny", "cubic", size=(2, 2), frame=(8, 8), n=2),
                _case(kernel, "u8chw", "grbg", 4096, "one", "cubic", size=(6, 10), frame=(8, 16), n=34)]
        if kernel == "mesh":
            out += [_case("mesh", "u16chw", "grbg", 4096, "wide", "cubic"), _case("mesh", "nv12", "rggb", 65536, "wide", "linear", in_align=2)]
        out += [_case(kernel, kind, CFAS[i], 0, "main", "cubic", n=2, in_align=i, out_off=ES[kind] * (i % 2)) for i, kind in enumerate(T.FLOAT_KINDS)]
    assert len({S["name"] for S in out}) == len(out)
    return {S["name"]: S for S in out}


def is_float(S):
    return S["kind"] in T.FLOAT_KINDS


def is_yuv(S):
    return S["kind"] in ("nv12", "p010")


def runs(S, variant):
    """Whether `variant`'s child runs the case: the float kinds have no loop to force."""
    return not is_float(S) or VARIANT_CAP[variant] is None


def colours(n):
    gain = np.stack([np.array([1.5 + 0.1 * (i % 5), 1.0, 1.9 - 0.2 * (i % 4)], np.float32) for i in range(n)])
    base = np.array([[1.7, -0.5, -0.2], [-0.25, 1.4, -0.15], [0.05, -0.45, 1.4]], np.float32)
    return gain, np.stack([base * np.float32(1.0 - 0.03 * (i % 7)) for i in range(n)])


@functools.lru_cache(maxsize=None)
def images(key):
    """The mosaics of a case's S["img"]: (n, H, W) uint16."""
    kind, n, H, Wd = key.split("_")[1:]
    n, H, Wd = int(n), int(H), int(Wd)
    if kind == "g":  # from below the black levels to above white
        return np.random.default_rng([20261021, n, H, Wd]).integers(0, 5000, (n, H, Wd), dtype=np.uint16)
    # krgb_ha: every way of both choices in every frame: 2-bit noise, with stripes both ways and 16-bit noise in bands of columns
    rng = np.random.default_rng([20261022, n, H, Wd])
    yy, xx = np.mgrid[0:H, 0:Wd]
    imgs = rng.integers(0, 4, (n, H, Wd)).astype(np.uint16)
    b = lambda lo, hi: slice(lo * Wd // 520, hi * Wd // 520)
    imgs[:, :, b(96, 160)] = rng.integers(0, 1 << 16, imgs[:, :, b(96, 160)].shape)
    imgs[:, :, b(224, 288)] = ((xx[:, b(224, 288)] & 1) * 65535).astype(np.uint16)
    imgs[:, :, b(400, 464)] = ((yy[:, b(400, 464)] & 1) * 65535).astype(np.uint16)
    return imgs


@functools.lru_cache(maxsize=None)
def maps(geo, size, frame, n):
    """krgb_warp: int32 (nmaps, 6), a map per frame (geo "one": one map for the batch)."""
    H, Wd = frame
    if geo == "main":  # at the bounds of the linear part, the output spread over the frame
        lins = ((65536 + 9000, 12000, -12000, 65536 + 9000), (65536 - 11000, -14000, 14000, 65536 - 11000), (65536, 3000, 5000, 65536 + 16384))
        out = []
        for i, lin in enumerate(lins[:n]):
            m = [lin[0], lin[1], 0, lin[2], lin[3], 0]
            Yp, Xp = W.positions(m, size)
            m[2] = -int(Yp.min()) + (256 * (H - 1) - int(Yp.max() - Yp.min())) * (i + 1) // 4
            m[5] = -int(Xp.min()) + (256 * (Wd - 1) - int(Xp.max() - Xp.min())) * (3 - i) // 4
            out.append(m)
    elif geo == "one":
        out = [[65536, 0, 256 + 77, 0, 65536, 512 + 130]]
    else:  # "edges", "tiny": translations into the frame's first corner and into its last: the windows reach over all four edges
        out = [[65536, 0, 0, 0, 65536, 0], [65536, 0, 256 * (H - size[0]), 0, 65536, 256 * (Wd - size[1])]]
        if n == 3:  # Y falls by 1/4 sample per column: (0, 69), the last tile's last pixel, reads row 1 + 10/256, the dropped (0, 71) row 0
            out.append([65536, -16384, 64 * (size[1] - 1) + 256 + 10, 0, 65536, 256])
    assert all(W.map_ok(m, size, H, Wd) for m in out)
    return np.asarray(out, dtype=np.int32)


@functools.lru_cache(maxsize=None)
def meshes(geo, size, frame, n):
    """krgb_mesh: int32 (nmesh, My, Mx, 2), a mesh per frame (geo "one": one for the batch)."""
    import motioncam_decoder_amd as M
    H, Wd = frame
    if geo in ("main", "wide"):
        m = [65536 - 11000, -14000, 0, 14000, 65536 - 11000, 0]
        Yp, Xp = W.positions(m, size)
        m[2], m[5] = -int(Yp.min()) + 300, -int(Xp.min()) + 500
        assert W.map_ok(m, size, H, Wd)
        hostile = MR.translation_mesh(size, 4, 6)  # outside the regime, nodes outside the frame
        hostile[:, 1:, 1] += 256 * 88
        hostile[0, :, 0] -= 256 * 9
        out = [M.affine_mesh(m, size)[0], M.distortion_mesh(H, Wd, size, radial=(1.0, -0.3, 0.05, 0.0)), hostile][:n]
        assert MR.in_regime(out[0], size, H, Wd) and MR.in_regime(out[1], size, H, Wd) and (n < 3 or not MR.in_regime(out[2], size, H, Wd))
        if geo == "wide":  # frame 0: the first cell is not narrow in Y; frame 1: the last cell is not narrow in X (nodes 2^22 away)
            out = [np.array(v) for v in out]
            out[0][0, 0, 0] -= 1 << 22
            out[1][-1, -1, 1] += 1 << 22
            out[2][1, 0, 0] += 1 << 22  # (and the hostile mesh leaves the frame through its other two sides: tile row 0 spans every row)
            out[2][0, -1, 1] -= 1 << 22
    elif geo == "one":
        out = [MR.translation_mesh(size, 1.3, 2.5)]
    else:
        out = [MR.translation_mesh(size, 0, 0), MR.translation_mesh(size, H - size[0], Wd - size[1]), MR.translation_mesh(size, 7.5, 7.25)][:n]
        if n == 3:  # folded: X falls by a sample per column over the last tile column; its last pixel (k = 69) reads column 66.25,
            out[2][:, -1, 1] = out[2][:, -2, 1] - 256 * 32  # the dropped k = 71 column 64.25, whose first tap lies left of eb = 64
    return np.stack(out).astype(np.int32)


def geometry(S):
    args = (S["geo"], S["size"], (S["H"], S["W"]), S["n"])
    return maps(*args) if S["kernel"] == "warp" else meshes(*args)


# ---- the headers' arithmetic (csrc/mcraw_rgb_dev.h, mcraw_warp_args.h, mcraw_mesh_args.h)

def reflect101(i, n):
    i = -i if i < 0 else i
    i = 2 * (n - 1) - i if i > n - 1 else i
    return min(max(i, 0), n - 1)


def _win(ys, xs):
    pb, eb = ((min(ys) >> 8) - 1) & ~1, ((min(xs) >> 8) - 1) & ~7
    return pb, eb, (((max(ys) >> 8) + 2 - pb) >> 1) + 1, (((max(xs) >> 8) + 2 - eb) >> 3) + 1


def warp_pos(m, i, k):
    return m[2] + ((m[0] * i + m[1] * k + 128) >> 8), m[5] + ((m[3] * i + m[4] * k + 128) >> 8)


def warp_window(m, i0, i1, k0, k1):
    p = [warp_pos(m, i, k) for i in (i0, i1) for k in (k0, k1)]
    return _win([y for y, _ in p], [x for _, x in p])


def mesh_lerp64(c, u, v):
    return (c[0] * (32 - u) * (32 - v) + c[1] * (32 - u) * v + c[2] * u * (32 - v) + c[3] * u * v + 512) >> 10


def mesh_narrow(c):
    return all(-MESH_NARROW < c[k] - c[0] < MESH_NARROW for k in (1, 2, 3))


def mesh_clamp(v, side):
    return min(max(v, 0), 256 * (side - 1))


def mesh_window(cy, cx, u1, v1, width, height):
    return _win([mesh_clamp(mesh_lerp64(cy, u, v), height) for u in (0, u1) for v in (0, v1)],
                [mesh_clamp(mesh_lerp64(cx, u, v), width) for u in (0, u1) for v in (0, v1)])


def mesh_tap_max(npp, nee):
    return 2 * min(npp, MESH_NP) - 4, 8 * min(nee, MESH_NE) - 4


def mesh_cell(mesh, ty, tx):
    c = [mesh[ty + (k >> 1)][tx + (k & 1)] for k in range(4)]
    return [int(v[0]) for v in c], [int(v[1]) for v in c]


# ---- the plan and the walk

def plan(S):
    if S["kernel"] == "ha":
        tilesX = (S["W"] + MHC_TW - 1) // MHC_TW
        return dict(Wo=S["W"], Ho=S["H"], tilesX=tilesX, units=tilesX * ((S["H"] + MHC_TH - 1) // MHC_TH), invec=int(T.on_grid(S)))
    Ho, Wo = S["size"]
    tilesX = (Wo + WARP_TW - 1) // WARP_TW
    return dict(Wo=Wo, Ho=Ho, tilesX=tilesX, units=tilesX * ((Ho + WARP_TH - 1) // WARP_TH), invec=int(T.on_grid(S)))


def out_frame_bytes(S):
    P = plan(S)
    return (P["Ho"] * P["Wo"] * 3 // 2 if is_yuv(S) else 3 * P["Ho"] * P["Wo"]) * ES[S["kind"]]


def launches(S):
    """Frames per launch: the colours are per frame in every case, so a batch goes in pieces of RGB_MAXF frames."""
    return [min(RGB_MAXF, S["n"] - f0) for f0 in range(0, S["n"], RGB_MAXF)]


def grids(S, variant, resident=None):
    units, cap = plan(S)["units"], VARIANT_CAP[variant]
    if is_float(S):
        return [units * nf for nf in launches(S)]
    lim = cap if cap is not None else resident if resident is not None else 1 << 30
    return [min(units * nf, lim) for nf in launches(S)]


# ---- krgb_warp and krgb_mesh: one unit

def tile_window(S, geo, f, ty, tx):
    """(pb, eb, np, ne) as warp_window / mesh_window give them, before the cut; and krgb_mesh's (narrow in Y, narrow in X)."""
    Ho, Wo = S["size"]
    i0, k0 = ty * WARP_TH, tx * WARP_TW
    i1, k1 = min(i0 + WARP_TH, Ho) - 1, min(k0 + WARP_TW, Wo) - 1
    if S["kernel"] == "warp":
        return warp_window([int(v) for v in geo[f if len(geo) > 1 else 0]], i0, i1, k0, k1), (True, True)
    cy, cx = mesh_cell(geo[f if len(geo) > 1 else 0], ty, tx)
    return mesh_window(cy, cx, i1 - i0, k1 - k0, S["W"], S["H"]), (mesh_narrow(cy), mesh_narrow(cx))


def _gather_unit(S, P, geo, f, u, c):
    fam, H, Wd = S["kernel"], S["H"], S["W"]
    Ho, Wo = S["size"]
    tx, ty = u % P["tilesX"], u // P["tilesX"]
    i0, k0 = ty * WARP_TH, tx * WARP_TW
    i1, k1 = min(i0 + WARP_TH, Ho) - 1, min(k0 + WARP_TW, Wo) - 1
    (pb, eb, wnp, wne), (ny, nx) = tile_window(S, geo, f, ty, tx)
    npp, nee = min(wnp, WARP_EROWS // 2), min(wne, WARP_ECOLS // 8)
    c[fam + "_cut_rows"] += npp < wnp
    c[fam + "_cut_cols"] += nee < wne
    for q in range(nee + 2):  # staging
        xs = eb - 8 + 8 * q
        c[fam + ("_ld_vec" if P["invec"] and xs >= 0 and xs + 8 <= Wd else "_ld_elem")] += 2 * npp + 4
    c[fam + "_a_even"] += npp * nee
    c[fam + "_a_odd"] += npp * nee
    if fam == "warp":
        m = [int(v) for v in geo[f if len(geo) > 1 else 0]]
        rmax, cmax = WARP_EROWS - 4, WARP_ECOLS - 4
    else:
        cy, cx = mesh_cell(geo[f if len(geo) > 1 else 0], ty, tx)
        rmax, cmax = mesh_tap_max(wnp, wne)
        c["mesh_narrow" if ny and nx else "mesh_wide"] += 1
    for t in range(RGB_T):  # the gather: a lane takes 4 columns of one row, all 4 of them when the first is in the tile
        gr, gc = t // (WARP_TW // 4), 4 * (t % (WARP_TW // 4))
        j, x = i0 + gr, k0 + gc
        if not (j <= i1 and x <= k1):
            c[fam + "_nopix"] += 1
            continue
        c[fam + "_pix"] += 1
        for i in range(4):
            if fam == "warp":
                by, bx = m[0] * j + m[1] * x + 128, m[3] * j + m[4] * x + 128
                Y, X = m[2] + ((by + m[1] * i) >> 8), m[5] + ((bx + m[4] * i) >> 8)
            else:
                yr, xr = mesh_lerp64(cy, gr, gc + i), mesh_lerp64(cx, gr, gc + i)
                c["mesh_y_lo"] += yr < 0
                c["mesh_y_hi"] += yr > 256 * (H - 1)
                c["mesh_x_lo"] += xr < 0
                c["mesh_x_hi"] += xr > 256 * (Wd - 1)
                Y, X = mesh_clamp(yr, H), mesh_clamp(xr, Wd)
            r, cc = (Y >> 8) - 1 - pb, (X >> 8) - 1 - eb
            c[fam + "_tap_row_lo"] += r < 0
            c[fam + "_tap_row_hi"] += r > rmax
            c[fam + "_tap_col_lo"] += cc < 0
            c[fam + "_tap_col_hi"] += cc > cmax
    rows = 2 if is_yuv(S) else 1
    for t in range(RGB_T):  # the store phase: a lane takes 8 columns of a row (YUV: of a row pair)
        lxid, lyid = t % (WARP_TW // 8), t // (WARP_TW // 8)
        if lyid >= WARP_TH // rows:
            c[fam + "_st_idle_ly"] += 1
        elif k0 + 8 * lxid >= Wo:
            c[fam + "_st_idle_x"] += 1
        elif i0 + rows * lyid > i1:
            c[fam + "_st_idle_row"] += 1


# ---- krgb_ha: one unit

def ha_rb_xpar(ypar, Sh):
    return (ypar ^ (Sh >> 1) ^ Sh) & 1


def ha_edge_rawcol(Q, Sh):
    return 7 if ha_rb_xpar((Q + 1) & 1, Sh) else MHC_TW + 8


def _ha_unit(S, P, img, u, c):
    H, Wd, Sh = S["H"], S["W"], R.SHIFT[S["cfa"]]
    x0, y0 = u % P["tilesX"] * MHC_TW, u // P["tilesX"] * MHC_TH
    for q in range(HA_RAWCH):
        xs = x0 - 8 + 8 * q
        c["ha_ld_vec" if P["invec"] and xs >= 0 and xs + 8 <= Wd else "ha_ld_elem"] += HA_RAWH
    # the raw window as staged, black subtracted by the frame parity of raw row R (y0 - 3 + R) and raw column C (x0 - 8 + C)
    rr = np.array([reflect101(y0 - 3 + r, H) for r in range(HA_RAWH)])
    cc = np.array([reflect101(x0 - 8 + k, Wd) for k in range(HA_RAWW)])
    bk = np.array(S["black"], dtype=np.int64)
    Rr, Cc = np.mgrid[0:HA_RAWH, 0:HA_RAWW]
    d = img[rr][:, cc].astype(np.int64) - bk[((Rr + 1) & 1) * 2 + (Cc & 1)]
    # ha_green's gradients at g row Q (raw row Q + 2), raw column C, for every Q and C = 2 .. HA_RAWW - 3
    at = lambda dr, dc: d[2 + dr:2 + dr + HA_GH, 2 + dc:HA_RAWW - 2 + dc]
    DH = np.abs(at(0, -1) - at(0, 1)) + np.abs(2 * at(0, 0) - at(0, -2) - at(0, 2))
    DV = np.abs(at(-1, 0) - at(1, 0)) + np.abs(2 * at(0, 0) - at(-2, 0) - at(2, 0))
    Q, C = np.mgrid[0:HA_GH, 2:HA_RAWW - 2]
    xp = np.array([ha_rb_xpar((q + 1) & 1, Sh) for q in range(HA_GH)])[:, None]
    main = (C >= 8) & (C < MHC_TW + 8) & ((C & 1) == xp)  # the main items run over every tile column, whatever the frame's width
    edge = C == np.array([ha_edge_rawcol(q, Sh) for q in range(HA_GH)])[:, None]
    assert int(main.sum()) == 8 * HA_G_MAIN and int(edge.sum()) == HA_G_EDGE
    for site, m in (("main", main), ("edge", edge)):
        c["ha_%s_a" % site] += int((m & (DH < DV)).sum())
        c["ha_%s_b" % site] += int((m & (DV < DH)).sum())
        c["ha_%s_eq" % site] += int((m & (DH == DV)).sum())
    for lx in range(32):  # the estimates
        if x0 + 8 * lx >= Wd:
            c["ha_continue"] += 8
            continue
        for ly in range(8):
            for ps in range(MHC_TH // 16):
                if y0 + 2 * (ly + 8 * ps) >= H:
                    c["ha_break"] += 1
                    break


@functools.lru_cache(maxsize=None)
def _ha_frame(img_key, f, cfa, black):
    """The diagonal choice at the R / B sites of frame f: the estimates count the columns below n of the rows below H, which is the frame."""
    return HA.ways(images(img_key)[f], black, cfa)[1]


# ---- the census of a call

@functools.lru_cache(maxsize=None)
def _model(kernel, name, variant, resident):
    S = cases(kernel)[name]
    P = plan(S)
    c = dict.fromkeys(PATHS, 0)
    for nf, grid in zip(launches(S), grids(S, variant, resident)):
        total = P["units"] * nf
        if is_float(S):
            first, later, cross = total, 0, 0
        else:
            first, later, cross = T.walk(P["units"], nf, grid)
            c["lut_global" if S["lutn"] > 4096 else "lut_lds"] += total
        for k, v in zip(T.WALK, (grid, first, later, cross)):
            c["%s_%s" % (k, kernel)] += v
    geo = None if kernel == "ha" else geometry(S)
    for f in range(S["n"]):
        for u in range(P["units"]):
            if kernel == "ha":
                _ha_unit(S, P, images(S["img"])[f], u, c)
            else:
                _gather_unit(S, P, geo, f, u, c)
        if kernel == "ha":
            for k, v in zip(("a", "b", "eq"), _ha_frame(S["img"], f, S["cfa"], tuple(S["black"]))):
                c["ha_diag_" + k] += v
    T.stores_of(c, S["kind"], P["Wo"], P["Ho"], S["n"], S["out_off"], out_frame_bytes(S))
    return c


def model(kernel, name, variant="census", resident=None):
    """The census of case `name` of `kernel` in the build `variant`."""
    return dict(_model(kernel, name, variant, resident))


# ---- which cases must drive which counter (variants `census` and `poison`), by the corpus' own attributes, and the counters
# that no accepted call can reach

NEW = [k for k in PATHS if k.split("_")[0] in ("warp", "mesh", "ha") or k.split("_")[-1] in ("warp", "mesh", "ha")]

# krgb_warp, for every call that warp_check accepts (the GPU tests assert these stay at zero):
ARGUED_ZERO = {
    "warp_cut_rows": "a map inside the linear bounds spans at most warp_span(32, 32) samples over a tile: WARP_EROWS is sized from it (the header's static_assert), so np <= 26",
    "warp_cut_cols": "likewise ne <= 8: WARP_ECOLS is warp_span(32, 32) + 1 + 3 + 7 rounded up to the 8-grid",
    "warp_tap_row_hi": "a tile's pixels, and the up to 3 positions a lane evaluates past a partial tile's last column, lie inside a full tile's span from the window's first row: the origin stays <= 2 np - 4 <= 48",
    "warp_tap_col_hi": "likewise in columns: the origin stays <= 8 ne - 4 <= 60",
    "warp_tap_col_lo": "axx >= 49152 > 0: X grows with the column, so no position of a row lies left of its first, which the window holds",
}


def _driven():
    D = {k: [] for k in NEW}
    for kernel in ("warp", "mesh", "ha"):
        for name, S in cases(kernel).items():
            add = lambda *ks: [D[k].append((kernel, name)) for k in ks]
            add("wg_" + kernel, "first_" + kernel)
            grid_in = S["in_align"] == 0
            if kernel == "ha":
                add("ha_ld_elem", "ha_continue", "ha_main_a", "ha_main_b", "ha_main_eq", "ha_edge_a", "ha_edge_b", "ha_edge_eq", "ha_diag_a", "ha_diag_b", "ha_diag_eq")
                if S["H"] % 32:
                    add("ha_break")
                if grid_in:
                    add("ha_ld_vec")
                continue
            add(kernel + "_a_even", kernel + "_a_odd", kernel + "_pix", kernel + "_st_idle_ly")
            if grid_in and S["geo"] in ("main", "wide"):
                add(kernel + "_ld_vec")
            if not grid_in or S["geo"] in ("edges", "tiny"):
                add(kernel + "_ld_elem")
            if S["size"][0] % 32 or S["size"][1] % 32:
                add(kernel + "_nopix")
            if S["size"][1] % 32 and S["size"][1] % 32 <= 24:
                add(kernel + "_st_idle_x")
            if S["size"][0] % 32:
                add(kernel + "_st_idle_row")
            if kernel == "mesh":
                add("mesh_narrow")
                if S["geo"] == "wide":
                    add("mesh_wide", "mesh_cut_rows", "mesh_tap_row_hi", "mesh_y_hi", "mesh_x_lo")
                if S["geo"] in ("main", "wide") and S["n"] == 3:  # the hostile mesh: outside the regime, nodes outside the frame
                    add("mesh_cut_cols", "mesh_y_lo", "mesh_x_hi", "mesh_tap_col_hi")
                if S["geo"] == "main":  # the affine mesh: Y falls along a row, as in krgb_warp's case below
                    add("mesh_tap_row_lo")
                if S["geo"] == "edges" and S["n"] == 3:  # the folded mesh: a position past the tile's last column lies left of the window
                    add("mesh_tap_col_lo")
            elif S["geo"] == "edges" and S["n"] == 3:  # a position past the last tile's last column lies above the window
                add("warp_tap_row_lo")
    return D


DRIVEN = _driven()
# under a grid cap (of at most 3 workgroups) every call with a LUT and a launch of more than 3 units also has later units and frame crossings
DRIVEN_CAPPED = {"%s_%s" % (k, f): [(f, n) for n, S in cases(f).items() if not is_float(S) and plan(S)["units"] * max(launches(S)) > 3]
                 for f in ("warp", "mesh", "ha") for k in ("later", "cross")}
