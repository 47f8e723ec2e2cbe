"""The corpus and the exact model of the estimators' path census (csrc/mcraw_est_paths.h; tests/test_est_paths_model.py on the CPU,
tests/test_gpu_est_paths.py and tests/_est_paths_child.py on the GPU).

model(name, variant) predicts every counter of one setting -- one call of mcraw_align_batch or mcraw_align_cells_batch, or one or
two of mcraw_noise_batch -- from the geometry, the view, the parameters, the samples, the per-level winners and the per-wave,
per-tile and per-candidate sums.  It replays the statements' search (_align_ref.pair, _align_cells_ref.pair_cell) level by level
and keeps what they throw away; answers() checks that the replay ends where the statements end.  No counter depends on LDS that
nobody staged (every such read is masked), so there is no range and no list of unmodelled counters."""
import functools

import numpy as np

import _align_cells_ref as CR
import _align_ref as R
import _align_scenes as SC
import _cells_scenes as CS
import _noise_ref as NR

N = 5                  # frames per call: launches of 2, 2, 1 in the `frames2` build
LONG_N = 2056          # ... and of the one chain that is clamped
VIEWS = ("grid", "off", "pitch")
VARIANTS = ("census", "frames2", "slow", "poison", "poisonslow", "strips1")
BLACK = (64, 60, 66, 64)
AL_T, AL_TW, AL_TH, AL_PW, AL_PH = 256, 128, 32, 256, 64
LAUNCH_FRAMES = 65535
NS_SB, NS_WGS, NS_MINSTRIPS, NS_MAXSTRIPS = 64, 1024, 16, 0x7FFFFFFF
NS_SAT, NS_LO, NS_SHIFT = (3900, 4000, 4000, 3950), (50, 40, 60, 50), 7

SK = ("launch", "wg", "nopair", "om0", "om1", "ob1om0", "ob1om1", "stg_load", "stg_zero_y", "stg_zero_col", "stg_pad", "stg_left",
      "stg_right", "row_above", "row_below", "ref_full", "ref_mask", "lane_empty", "unstaged", "wave_add", "wave_skip", "glob_add",
      "glob_skip", "store", "empty")
_LD = ("ld_vec", "ld_unal", "ld_elem", "st_vec", "st_unal", "st_elem")
PATHS = (["py_" + k for k in _LD]
         + ["py_wg", "py_ret", "py_zero_row", "py_g0_vec", "py_g0_elem", "py_g0_left", "py_g1_dword", "py_g1_elem", "py_g1_none",
            "py_g1_left", "py_g2_store", "py_g2_none", "py_ret_l2", "py_ret_l3", "dn_launch", "dn_past", "az_launch", "cz_launch"]
         + ["%s%d_%s" % (f, rt, k) for f in ("as", "cs") for rt in (0, 1) for k in SK]
         + ["ap_nopair", "af_piece", "af_clamp", "cp_nopair", "cf_past", "cf_nopair", "cf_clamp"]
         + ["ns_" + k for k in _LD]
         + ["ns_wg", "ns_skip_t1", "ns_skip_inactive", "ns_block", "ns_rej_sat", "ns_rej_lo", "ns_accept", "ns_hist_flush", "ns_reg_flush"])
# what no input can drive: store8 is not called by these sources and knoise reads whole blocks; al_stage has no clamps and cl_stage
# no zeros; only kcells_sad stores or meets an empty piece; the candidate loops have no al_refine.  And the parities: a cell starts
# on an even column (ob = 0); a refinement level's centre is twice a winner, so even, its radius is 1 and B(l) = 2 B(l + 1) + 1 is
# odd: kalign_sad<1> sees (ob, om) = (1, 0) only -- a coarsest level of radius 1 too: B = 1, centre 0 -- and kcells_sad<1> om = 1 only;
# kalign_sad<0> starts its member tile at column tx * 128 (om = 0) with ob = radius & 1.
NEVER = (["py_st_vec", "py_st_unal", "py_st_elem", "ns_st_vec", "ns_st_unal", "ns_st_elem", "ns_ld_elem"]
         + ["as%d_%s" % (rt, k) for rt in (0, 1) for k in ("stg_left", "stg_right", "row_above", "row_below", "unstaged", "store", "empty")]
         + ["cs%d_%s" % (rt, k) for rt in (0, 1) for k in ("ob1om0", "ob1om1", "stg_zero_y", "stg_zero_col", "stg_pad")]
         + ["as0_ref_full", "as0_ref_mask", "cs0_ref_full", "cs0_ref_mask"]
         + ["as1_om0", "as1_om1", "as1_ob1om1", "as0_om1", "as0_ob1om1", "cs1_om0"])


# ---------------------------------------------------------------------------------------------------------------- corpus

def _settings():
    S = {}

    def add(name, **kw):
        assert name not in S
        kw.setdefault("n", N)
        S[name] = kw

    # align, mosaics (H, W), levels, radius.  (The window of 56 x 72 is empty at level 0 with levels = 4: 64 x 72 is the smallest
    # frame of that width that the contract takes with a kalign_down level.  44 x 44 with radius 3 is here for ob = 1 in the
    # candidate loop: B = 3 is odd.)
    shapes = ((6, 6, 1, 1), (7, 9, 1, 1), (20, 300, 1, 1), (80, 40, 1, 2), (70, 270, 3, 1), (64, 72, 4, 1), (70, 74, 1, 8), (44, 44, 1, 3))
    for H, W, levels, radius in shapes:
        for ref in (-1, 2):
            for view in VIEWS:
                add("align_%dx%d_%s_%s" % (H, W, view, "chain" if ref < 0 else "anchor"), family="align", H=H, W=W, levels=levels,
                    radius=radius, ref=ref, view=view, content="scene", seed=len(S))
        for content in ("noise", "flat", "same"):
            add("align_%dx%d_%s" % (H, W, content), family="align", H=H, W=W, levels=levels, radius=radius, ref=-1, view="grid",
                content=content, seed=len(S))
    add("align_long", family="align", H=40, W=40, levels=1, radius=8, ref=-1, view="grid", content="long", seed=0, n=LONG_N)
    # cells: (H, W), cell; (levels, radius, centres, ref), the views in turn
    combos = ((3, 1, "none", -1), (2, 4, "hand", 2), (1, 4, "align", -1), (1, 1, "hand", 2), (3, 4, "hand", -1), (2, 1, "align", 2))
    k = 0
    for H, W, cell in ((6, 16, (32, 256)), (8, 16, (32, 256)), (101, 601, (32, 256)), (130, 1030, (64, 512)), (32, 256, (32, 256))):
        for levels, radius, centres, ref in combos:
            add("cells_%dx%d_l%dr%d_%s_%s_%s" % (H, W, levels, radius, centres, "chain" if ref < 0 else "anchor", VIEWS[k % 3]),
                family="cells", H=H, W=W, cell=cell, levels=levels, radius=radius, centres=centres, ref=ref, view=VIEWS[k % 3],
                content="halves", seed=len(S))
            k += 1
        for content in ("flat", "same"):
            add("cells_%dx%d_%s" % (H, W, content), family="cells", H=H, W=W, cell=cell, levels=2, radius=1, centres="none", ref=-1,
                view="grid", content=content, seed=len(S))
    # noise: the frame, the window (y0, x0, h, w)
    for tag, H, W, roi in (("one", 40, 40, (4, 8, 16, 16)), ("strip65", 20, 1048, (2, 0, 16, 1040)), ("odd", 40, 72, (2, 2, 33, 50)),
                           ("rows", 300, 40, (0, 8, 290, 24))):
        for view in VIEWS:
            add("noise_%s_%s" % (tag, view), family="noise", H=H, W=W, roi=roi, view=view, content="kinds", seed=len(S), calls=1)
    add("noise_strip65_twice", family="noise", H=20, W=1048, roi=(2, 0, 16, 1040), view="grid", content="kinds", seed=len(S), calls=2)
    return S


SETTINGS = _settings()


def view_geom(S):
    """(offset, pitch, frame stride) of the setting's input, in samples from a 16-byte boundary."""
    H, W = S["H"], S["W"]
    pitch = W + 3 if S["view"] == "pitch" else (W + 7) // 8 * 8
    return (1 if S["view"] == "off" else 0), pitch, H * pitch


def on_grid(S):
    off, pitch, fstride = view_geom(S)
    return off % 8 == 0 and pitch % 8 == 0 and fstride % 8 == 0


def black(S):
    return (0, 0, 0, 0) if S["content"] == "noise" else BLACK


@functools.lru_cache(maxsize=None)
def images(name):
    """(n, H, W) uint16 of a setting."""
    S = SETTINGS[name]
    H, W, n, content = S["H"], S["W"], S["n"], S["content"]
    rng = np.random.default_rng(20261021 + S["seed"])
    if content == "scene":  # steps of both parities in the grey plane
        return SC.scene_frames(S["seed"], H, W, S["levels"], S["radius"], 9, n=n)[0]
    if content == "long":
        return SC.clamp_frames(n)[0]
    if content == "halves":
        return CS.halves_frames(S["seed"], H, W, 9, n=n, reach=8, noise=8.0, seam=min(256, W // 2))[0]
    if content == "noise":
        return rng.integers(0, 1 << 16, (n, H, W), dtype=np.uint16)
    if content == "flat":
        return np.full((n, H, W), 1000, np.uint16)
    if content == "same":
        return np.repeat(rng.integers(64, 4096, (1, H, W), dtype=np.uint16), n, axis=0)
    assert content == "kinds"
    # 12-bit noise between lo and sat; block k of frame f is of kind (k + f) % 4: accepted, a sample >= sat in every position's
    # plane, a sample < lo in every one, both
    f = rng.integers(100, 3000, (n, H, W), dtype=np.uint16)
    y0, x0, h, w = S["roi"]
    for t in range(n):
        for by in range(h // 16):
            for bx in range(w // 16):
                kind = (by * (w // 16) + bx + t) % 4
                yy, xx = y0 + 16 * by, x0 + 16 * bx
                if kind & 1:
                    f[t, yy + 4:yy + 6, xx + 6:xx + 8] = 4090
                if kind & 2:
                    f[t, yy + 8:yy + 10, xx + 2:xx + 4] = 7
    return f


def hand(S):
    """Centres with odd and negative components, steps larger than the frame, and a last step that the clamp cuts."""
    H, W = S["H"], S["W"]
    return np.array([[0, 0], [5, -7], [-2 * H - 101, 9], [3, 2 * W + 33], [32767, -32768]], np.int16)


@functools.lru_cache(maxsize=None)
def centres(name):
    S = SETTINGS[name]
    if S["centres"] == "none":
        return None
    if S["centres"] == "hand":
        return hand(S)
    return R.align(images(name), BLACK, 1, 1)[0]


# ---------------------------------------------------------------------------------------------------------------- the model

def _ceil(a, b):
    return -(-a // b)


def _launches(n, variant):
    """The frames of every launch of a launch loop."""
    piece = 2 if variant == "frames2" else LAUNCH_FRAMES
    return [min(piece, n - f0) for f0 in range(0, n, piece)]


def _planes(H, W, levels):
    h, w = [H // 2], [W // 2]
    for _ in range(levels - 1):
        h.append(h[-1] // 2), w.append(w[-1] // 2)
    return h, w


def _blocks(D, rh, rw):
    """Sums of D (..., hh, ww) over blocks of rh x rw from its origin: (..., ceil(hh / rh), ceil(ww / rw))."""
    D = np.add.reduceat(D, np.arange(0, D.shape[-2], rh), axis=-2)
    return np.add.reduceat(D, np.arange(0, D.shape[-1], rw), axis=-1)


def _pyramid(c, S, variant):
    """kalign_pyr and kalign_down for the n frames (align_pyramid)."""
    H, W, levels, n = S["H"], S["W"], S["levels"], S["n"]
    h, w = _planes(H, W, levels)
    vec = on_grid(S)
    xs, ys = np.arange(0, _ceil(W, AL_PW) * AL_PW, 8), np.arange(0, _ceil(H, AL_PH) * AL_PH, 8)
    X, Y = xs[xs < W], ys[ys < H]
    c["py_wg"] += n * _ceil(W, AL_PW) * _ceil(H, AL_PH)
    c["py_ret"] += n * (len(xs) * len(ys) - len(X) * len(Y))
    zero = int(np.maximum(Y + 8 - H, 0).sum())
    c["py_zero_row"] += n * zero * len(X)
    rows = 8 * len(Y) - zero  # loaded rows per lane column
    full = int((W - X >= 8).sum())
    c["py_ld_vec" if vec else "py_ld_unal"] += n * rows * full
    c["py_ld_elem"] += n * rows * (len(X) - full)
    # G0
    r0 = np.clip(h[0] - Y // 2, 0, 4)  # rows stored per lane row
    c["py_g0_left"] += n * int((4 - r0).sum()) * len(X)
    nv = int((X // 2 + 4 <= w[0]).sum())
    c["py_g0_vec"] += n * int(r0.sum()) * nv
    c["py_g0_elem"] += n * int(r0.sum()) * (len(X) - nv)
    if levels < 2:
        c["py_ret_l2"] += n * len(X) * len(Y)
        return
    r1 = np.clip(h[1] - Y // 4, 0, 2)
    c["py_g1_left"] += n * int((2 - r1).sum()) * len(X)
    gx = X // 4
    c["py_g1_dword"] += n * int(r1.sum()) * int((gx + 2 <= w[1]).sum())
    c["py_g1_elem"] += n * int(r1.sum()) * int(((gx + 2 > w[1]) & (gx < w[1])).sum())
    c["py_g1_none"] += n * int(r1.sum()) * int((gx >= w[1]).sum())
    if levels < 3:
        c["py_ret_l3"] += n * len(X) * len(Y)
        return
    st = int((X // 8 < w[2]).sum()) * int((Y // 8 < h[2]).sum())
    c["py_g2_store"] += n * st
    c["py_g2_none"] += n * (len(X) * len(Y) - st)
    for nf in _launches(n, variant):
        for l in range(3, levels):
            if h[l] == 0 or w[l] == 0:
                break
            c["dn_launch"] += 1
            c["dn_past"] += nf * (_ceil(h[l] * w[l], AL_T) * AL_T - h[l] * w[l])


def _base(t, ref):
    return t - 1 if ref < 0 else (-1 if t == ref else ref)


def _key(s, Rr):
    return min((int(s[dy + Rr, dx + Rr]), dy * dy + dx * dx, dy, dx) for dy in range(-Rr, Rr + 1) for dx in range(-Rr, Rr + 1))


def _al_stage(c, pre, h, pitch, w, ys, xs, rows, ndw):
    yok = int((ys + np.arange(rows) < h).sum())
    cols = xs + 2 * np.arange(ndw)
    c[pre + "stg_load"] += yok * int((cols < pitch).sum())
    c[pre + "stg_zero_y"] += (rows - yok) * ndw
    c[pre + "stg_zero_col"] += yok * int((cols >= pitch).sum())
    c[pre + "stg_pad"] += yok * int(((cols < pitch) & (cols + 1 >= w)).sum())


def _waves(c, pre, D, wgs, ncand, atomics=True):
    """A launch's candidate sums D (ncand.., hh, ww) from the first workgroup's origin: per wave (8 rows x 128 columns), per tile."""
    wave = _blocks(D, 8, AL_TW)
    c[pre + "wave_add"] += int((wave != 0).sum())
    c[pre + "wave_skip"] += 4 * ncand * wgs - int((wave != 0).sum())
    if atomics:
        tile = _blocks(D, AL_TH, AL_TW)
        c[pre + "glob_add"] += int((tile != 0).sum())
        c[pre + "glob_skip"] += ncand * wgs - int((tile != 0).sum())


def _align(c, S, variant, frames):
    """mcraw_align_batch: (d (n, 2) in level-0 pixels, sad (n,))."""
    H, W, levels, radius, ref, n = S["H"], S["W"], S["levels"], S["radius"], S["ref"], S["n"]
    slow = variant in ("slow", "poisonslow")
    h, w = _planes(H, W, levels)
    B = R.bounds(levels, radius)
    pyr = [R.pyramid(f, black(S), levels) for f in frames]
    c["az_launch"] += 1
    _pyramid(c, S, variant)
    pairs = [(t, _base(t, ref)) for t in range(n) if _base(t, ref) >= 0]
    centre = {t: (0, 0) for t, _ in pairs}
    sad = np.zeros(n, np.uint64)
    for l in range(levels - 1, -1, -1):
        top = l == levels - 1
        Rr = radius if top else 1
        rt = 0 if Rr != 1 else 1  # (a coarsest level of radius 1 takes the register form)
        pre = "as%d_" % rt
        ncand, pitch = (2 * Rr + 1) ** 2, (w[l] + 7) // 8 * 8
        hh, ww = h[l] - 2 * B[l], w[l] - 2 * B[l]
        tx, ty = _ceil(ww, AL_TW), _ceil(hh, AL_TH)
        c[pre + "launch"] += len(_launches(n, variant))
        c[pre + "wg"] += n * tx * ty
        c[pre + "nopair"] += (n - len(pairs)) * tx * ty
        c["ap_nopair"] += _ceil(n, AL_T) * AL_T - len(pairs)
        for t, b in pairs:
            cy, cx = centre[t]
            gb, gt = pyr[b][l], pyr[t][l]
            base = gb[B[l]:h[l] - B[l], B[l]:w[l] - B[l]]
            v = np.lib.stride_tricks.sliding_window_view(gt, base.shape)[B[l] + cy - Rr:B[l] + cy + Rr + 1, B[l] + cx - Rr:B[l] + cx + Rr + 1]
            D = np.abs(v - base)
            assert D.shape[:2] == (2 * Rr + 1, 2 * Rr + 1)
            for j in range(ty):
                for i in range(tx):
                    x0, y0, x1, y1 = B[l] + i * AL_TW, B[l] + j * AL_TH, w[l] - B[l], h[l] - B[l]
                    xm, ym = x0 + cx - Rr, y0 + cy - Rr
                    assert xm >= 0 and ym >= 0
                    c[pre + ("om0", "om1", "ob1om0", "ob1om1")[2 * (x0 & 1) + (xm & 1)]] += 1
                    _al_stage(c, pre, h[l], pitch, w[l], y0, x0 & ~1, AL_TH, AL_TW // 2 + 1)
                    _al_stage(c, pre, h[l], pitch, w[l], ym, xm & ~1, AL_TH + 2 * Rr, AL_TW // 2 + Rr + 1)
                    c[pre + "lane_empty"] += AL_T - _ceil(min(AL_TW, x1 - x0), 4) * _ceil(min(AL_TH, y1 - y0), 4)
                    if rt:
                        full = 0 if slow or x0 + AL_TW > x1 else sum(1 for k in range(4) if y0 + 8 * k + 8 <= y1)
                        c[pre + "ref_full"] += full
                        c[pre + "ref_mask"] += 4 - full
            _waves(c, pre, D, tx * ty, ncand)
            key = _key(D.sum(axis=(2, 3)), Rr)
            cy, cx = cy + key[2], cx + key[3]
            sad[t] = key[0]
            centre[t] = (2 * cy, 2 * cx) if l else (cy, cx)
    d = np.zeros((n, 2), np.int64)
    for t, _ in pairs:
        d[t] = centre[t]
    c["af_piece"] += _ceil(n, AL_T) if ref < 0 else 0
    step = 2 * d
    pos = np.cumsum(step, axis=0) if ref < 0 else step
    c["af_clamp"] += int(((pos < -32768) | (pos > 32767)).sum())
    return R.positions(d, ref), sad


def _cl_stage(c, pre, h, w, ys, xs, rows, ndw):
    cols = xs + 2 * np.arange(ndw)
    c[pre + "stg_load"] += rows * int(((cols >= 0) & (cols + 1 < w)).sum())
    c[pre + "stg_left"] += rows * int((cols < 0).sum())
    c[pre + "stg_right"] += rows * int(((cols >= 0) & (cols + 1 >= w)).sum())
    yy = ys + np.arange(rows)
    c[pre + "row_above"] += int((yy < 0).sum())
    c[pre + "row_below"] += int((yy > h - 1).sum())


_LX, _LY = np.arange(AL_T) % 32, np.arange(AL_T) // 32


def _cells(c, S, variant, frames, gpos):
    """mcraw_align_cells_batch: (pos (n, Cy, Cx, 2), sad (n, Cy, Cx))."""
    H, W, levels, radius, ref, n, cell = S["H"], S["W"], S["levels"], S["radius"], S["ref"], S["n"], S["cell"]
    slow = variant in ("slow", "poisonslow")
    h, w = _planes(H, W, levels)
    Cy, Cx = CR.grid(H, W, cell)
    cells = Cy * Cx
    pyr = [R.pyramid(f, black(S), levels) for f in frames]
    geo = [(cell[0] >> (l + 1), cell[1] >> (l + 1)) for l in range(levels)]
    npieces = [_ceil(cw, AL_TW) * _ceil(ch, AL_TH) for ch, cw in geo]
    if slow or any(p != 1 for p in npieces):
        c["cz_launch"] += 1
    _pyramid(c, S, variant)
    pairs = [(t, _base(t, ref)) for t in range(n) if _base(t, ref) >= 0]
    centre = {(t, i, j): CR.centre(gpos, t, b, levels) for t, b in pairs for i in range(Cy) for j in range(Cx)}
    sad = np.zeros((n, Cy, Cx), np.uint64)
    for l in range(levels - 1, -1, -1):
        top = l == levels - 1
        Rr = radius if top else 1
        rt = 0 if top else 1  # (the coarsest level takes the loop whatever its radius)
        pre = "cs%d_" % rt
        ncand = (2 * Rr + 1) ** 2
        ch, cw = geo[l]
        px, py = _ceil(cw, AL_TW), _ceil(ch, AL_TH)
        store = npieces[l] == 1 and not slow
        c[pre + "launch"] += len(_launches(n, variant))
        c[pre + "wg"] += n * cells * npieces[l]
        c[pre + "nopair"] += (n - len(pairs)) * cells * npieces[l]
        c["cp_nopair"] += n * _ceil(cells, AL_T) * AL_T - len(pairs) * cells
        for t, b in pairs:
            gb, gt = pyr[b][l], pyr[t][l]
            for i in range(Cy):
                for j in range(Cx):
                    cy, cx = centre[t, i, j]
                    r0, r1, c0, c1 = CR.cell_pixels(i, j, cell, l, h[l], w[l])
                    assert (r0, c0) == (i * ch, j * cw)
                    withpix = 0
                    for pj in range(py):
                        for pi in range(px):
                            x0, y0 = c0 + pi * AL_TW, r0 + pj * AL_TH
                            if not (x0 < c1 and y0 < r1):
                                c[pre + "empty"] += 1
                                continue
                            withpix += 1
                            xm, ym = x0 + cx - Rr, y0 + cy - Rr
                            om = xm & 1
                            c[pre + ("om0", "om1")[om]] += 1
                            nyp, nxp = min(AL_TH, r1 - y0), min(AL_TW, c1 - x0)
                            _cl_stage(c, pre, h[l], w[l], y0, x0, nyp, (nxp + 1) // 2)
                            _cl_stage(c, pre, h[l], w[l], ym, xm & ~1, nyp + 2 * Rr, (nxp + 2 * Rr) // 2 + 1)
                            c[pre + "lane_empty"] += AL_T - _ceil(nxp, 4) * _ceil(nyp, 4)
                            un = (4 * _LY + 3 >= nyp) | ((2 * _LX + 2 if rt else 2 * _LX + 1) >= (nxp + 1) // 2) | \
                                ((2 * _LX + 3 if rt else (4 * _LX + 3 + 2 * Rr + om) // 2) >= (nxp + 2 * Rr) // 2 + 1)
                            c[pre + "unstaged"] += int(un.sum())
                            if rt:
                                full = 0 if slow or nxp < AL_TW else sum(1 for k in range(4) if 8 * k + 8 <= nyp)
                                c[pre + "ref_full"] += full
                                c[pre + "ref_mask"] += 4 - full
                    if store:
                        c[pre + "store"] += ncand * npieces[l]
                    if r0 >= r1 or c0 >= c1:
                        s = np.zeros((2 * Rr + 1, 2 * Rr + 1), np.int64)
                        if not store:
                            c[pre + "glob_skip"] += ncand * npieces[l]
                    else:
                        ys, xs = np.arange(r0, r1), np.arange(c0, c1)
                        D = np.empty((2 * Rr + 1, 2 * Rr + 1, r1 - r0, c1 - c0), np.int64)
                        for a, dy in enumerate(range(cy - Rr, cy + Rr + 1)):
                            rows = gt[np.clip(ys + dy, 0, h[l] - 1)]
                            for e, dx in enumerate(range(cx - Rr, cx + Rr + 1)):
                                D[a, e] = np.abs(rows[:, np.clip(xs + dx, 0, w[l] - 1)] - gb[r0:r1, c0:c1])
                        _waves(c, pre, D, withpix, ncand, atomics=not store)
                        if not store:
                            c[pre + "glob_skip"] += ncand * (npieces[l] - withpix)
                        s = D.sum(axis=(2, 3))
                    key = _key(s, Rr)
                    cy, cx = cy + key[2], cx + key[3]
                    sad[t, i, j] = key[0]
                    centre[t, i, j] = (2 * cy, 2 * cx) if l else (cy, cx)
    d = np.zeros((n, Cy, Cx, 2), np.int64)
    for (t, i, j), v in centre.items():
        d[t, i, j] = v
    c["cf_past"] += _ceil(cells, AL_T) * AL_T - cells
    c["cf_nopair"] += (n - len(pairs)) * cells
    pos = np.cumsum(2 * d, axis=0) if ref < 0 else 2 * d
    c["cf_clamp"] += int(((pos < -32768) | (pos > 32767)).sum())
    return CR.positions(d, ref), sad


def noise_plan(w, h, frames, maxstrips):
    """noise_plan of csrc/mcraw_noise_args.h."""
    bx, by = w // 16, h // 16
    sx = _ceil(bx, NS_SB)
    strips = sx * by
    want = max(NS_WGS // frames, 1)
    spw = max(min(max(_ceil(strips, want), NS_MINSTRIPS), maxstrips, strips), 1)
    return dict(bx=bx, by=by, stripsX=sx, strips=strips, spw=spw, wgs=_ceil(strips, spw))


def _noise(c, S, variant, frames):
    """mcraw_noise_batch, S["calls"] times into the same records: the records' bytes."""
    n, (y0, x0, rh, rw) = S["n"], S["roi"]
    vec = on_grid(S) and x0 % 8 == 0
    b = NR.planes(frames, S["roi"])
    s, T = NR.sums(b)
    sat, lo = np.asarray(NS_SAT), np.asarray(NS_LO)
    rsat = b.max((-1, -2)) >= sat                      # (n, by, bx, 4)
    rlo = ~rsat & (b.min((-1, -2)) < lo)
    ok = ~rsat & ~rlo
    bins = (np.arange(4) * NR.L + np.minimum((s >> 6) >> NS_SHIFT, NR.L - 1)) * NR.V + NR.energy_bin(T)
    for _ in range(S["calls"]):
        f0 = 0
        for nf in _launches(n, variant):
            P = noise_plan(rw, rh, nf, 1 if variant == "strips1" else NS_MAXSTRIPS)
            for f in range(f0, f0 + nf):
                c["ns_wg"] += P["wgs"]
                for wg in range(P["wgs"]):
                    t0 = wg * P["spw"]
                    t1 = min(t0 + P["spw"], P["strips"])
                    seen = set()
                    regs = np.zeros((2, 4, 2), np.int64)  # half, position, accepted | rejected
                    i = 0
                    while t0 + 2 * i < t1:
                        for half in (0, 1):
                            t = t0 + 2 * i + half
                            if t >= t1:
                                c["ns_skip_t1"] += 2 * NS_SB
                                continue
                            sy, sx = divmod(t, P["stripsX"])
                            nb = min(NS_SB, P["bx"] - sx * NS_SB)
                            c["ns_skip_inactive"] += 2 * (NS_SB - nb)
                            c["ns_block"] += 2 * nb
                            c["ns_ld_vec" if vec else "ns_ld_unal"] += 2 * nb * 16
                            sl = (f, sy, slice(sx * NS_SB, sx * NS_SB + nb))
                            c["ns_rej_sat"] += int(rsat[sl].sum())
                            c["ns_rej_lo"] += int(rlo[sl].sum())
                            c["ns_accept"] += int(ok[sl].sum())
                            seen.update(bins[sl][ok[sl]].tolist())
                            regs[half, :, 0] += ok[sl].sum(axis=0)
                            regs[half, :, 1] += (~ok[sl]).sum(axis=0)
                        i += 1
                    c["ns_hist_flush"] += len(seen)
                    c["ns_reg_flush"] += int((regs != 0).sum())
            f0 += nf
    d = NR.noise_stats(frames, NS_SHIFT, NS_SAT, NS_LO, S["roi"])
    for _ in range(S["calls"] - 1):
        d = NR.add(d, NR.noise_stats(frames, NS_SHIFT, NS_SAT, NS_LO, S["roi"]))
    return NR.record(d)


@functools.lru_cache(maxsize=None)
def _run(name, variant):
    S = SETTINGS[name]
    c = dict.fromkeys(PATHS, 0)
    frames = images(name)
    if S["family"] == "align":
        out = _align(c, S, variant, frames)
    elif S["family"] == "cells":
        out = _cells(c, S, variant, frames, centres(name))
    else:
        out = (_noise(c, S, variant, frames),)
    return c, out


def _twin(variant):
    """The build whose census `variant`'s equals: poison changes no counter, strips1 none outside knoise, frames2 none in it ..."""
    return {"poison": "census", "poisonslow": "slow"}.get(variant, variant)


def model(name, variant="census"):
    """Every counter of setting `name` in build `variant`: a dict by PATHS."""
    fam = SETTINGS[name]["family"]
    v = _twin(variant)
    if fam == "noise":
        v = v if v in ("frames2", "strips1") else "census"
    else:
        v = v if v in ("frames2", "slow") else "census"
    return dict(_run(name, v)[0])


def answers(name):
    """What the replay ends in: (pos, sad) of align and cells, (records,) of noise."""
    return _run(name, "census")[1]


def statement(name):
    """The same from the numpy statements alone."""
    S = SETTINGS[name]
    if S["family"] == "align":
        return R.align(images(name), black(S), S["levels"], S["radius"], S["ref"])
    if S["family"] == "cells":
        return CR.align_cells(images(name), black(S), S["cell"], S["levels"], S["radius"], S["ref"], centres(name))
    return (answers(name)[0],)  # (_noise builds the records from _noise_ref.noise_stats itself)


# ---------------------------------------------------------------------------------------------------------------- DRIVEN

def _names(pred):
    return tuple(k for k, S in SETTINGS.items() if pred(S))


def _al(H, W, **kw):
    return lambda S: S["family"] == "align" and (S["H"], S["W"]) == (H, W) and all(S[k] == v for k, v in kw.items())


def _cl(H, W, **kw):
    return lambda S: S["family"] == "cells" and (S["H"], S["W"]) == (H, W) and all(S[k] == v for k, v in kw.items())


def _fam(f, **kw):
    return lambda S: S["family"] == f and all(S.get(k) == v for k, v in kw.items())


def _driven():
    """Per counter the settings in which it must be above zero (`census`), each from the geometry that the corpus was cut for."""
    D = {}
    D["py_ld_vec"] = _names(lambda S: S["family"] != "noise" and S["view"] == "grid" and S["W"] >= 8)
    D["py_ld_unal"] = _names(lambda S: S["family"] != "noise" and S["view"] != "grid" and S["W"] >= 8)
    D["py_ld_elem"] = _names(lambda S: S["family"] != "noise" and S["W"] % 8 != 0)
    D["py_wg"] = _names(lambda S: S["family"] != "noise")
    D["py_g0_left"] = _names(lambda S: S["family"] != "noise" and S["H"] % 8 != 0)
    D["py_ret"] = _names(lambda S: S["family"] != "noise" and (S["W"] % 256 != 0 or S["H"] % 64 != 0))
    D["py_zero_row"] = _names(lambda S: S["family"] != "noise" and S["H"] % 8 != 0)
    D["py_g0_vec"] = _names(lambda S: S["family"] != "noise" and S["W"] >= 8)
    D["py_g0_elem"] = _names(lambda S: S["family"] != "noise" and S["W"] % 8 != 0)
    D["py_g1_dword"] = _names(_al(70, 270)) + _names(_al(64, 72))
    D["py_g1_left"] = _names(_al(70, 270))   # h1 = 17: the lanes at y = 64 have gy = 16
    D["py_g1_elem"] = _names(_al(70, 270))   # w1 = 67: the lane at x = 264 has gx = 66
    D["py_g1_none"] = _names(_cl(101, 601, levels=3))  # w1 = 150: the lane at x = 600 has gx = 150
    D["py_g2_store"] = _names(_al(70, 270))
    D["py_g2_none"] = _names(_al(70, 270))   # h2 = 8: the lanes at y = 64 have gy = 8
    D["py_ret_l2"] = _names(lambda S: S["family"] != "noise" and S["levels"] == 1)
    D["py_ret_l3"] = _names(lambda S: S["family"] != "noise" and S["levels"] == 2)
    D["dn_launch"] = D["dn_past"] = _names(_al(64, 72))
    D["az_launch"] = _names(_fam("align"))
    D["cz_launch"] = _names(_cl(130, 1030))
    D["ap_nopair"] = D["as1_launch"] = D["as1_wg"] = D["as1_nopair"] = _names(_al(70, 270))
    D["af_piece"] = _names(_fam("align", ref=-1))
    D["af_clamp"] = ("align_long",)
    for k in ("launch", "wg", "nopair", "stg_load", "wave_add", "glob_add", "lane_empty"):
        D["as0_" + k] = _names(_al(70, 74, content="scene"))
        D["as1_" + k] = _names(_al(70, 270, content="scene"))
        D["cs0_" + k] = _names(_cl(101, 601, content="halves"))
        D["cs1_" + k] = _names(_cl(130, 1030, content="halves", levels=3))
    D["cs1_glob_add"] = _names(_cl(130, 1030, content="halves", levels=3))
    D["cs0_glob_add"] = _names(_cl(130, 1030, content="halves", levels=1))
    D["as1_ref_full"] = _names(_al(20, 300))  # the first tile across: 8 rows, one full wave
    D["as1_ref_mask"] = _names(_al(20, 300))
    D["cs1_ref_full"] = D["cs1_ref_mask"] = _names(_cl(130, 1030, levels=2)) + _names(_cl(130, 1030, levels=3))
    D["as0_stg_zero_y"] = D["as0_stg_zero_col"] = D["as0_stg_pad"] = _names(_al(70, 74))
    D["as1_stg_zero_y"] = D["as1_stg_zero_col"] = D["as1_stg_pad"] = _names(_al(20, 300))
    for k in ("wave_skip", "glob_skip"):
        D["as0_" + k] = _names(_al(70, 74, content="flat"))
        D["as1_" + k] = _names(_al(70, 270, content="flat"))
    D["cs0_wave_skip"] = D["cs1_wave_skip"] = _names(_cl(130, 1030, content="flat"))
    D["cs0_glob_skip"] = _names(_cl(130, 1030, levels=1))  # (pieces past the frame's edge)
    D["cs1_glob_skip"] = _names(_cl(130, 1030, content="flat"))
    D["cs0_store"] = _names(_cl(32, 256))
    D["cs1_store"] = _names(_cl(32, 256, levels=3))
    D["cs0_empty"] = _names(_cl(6, 16, levels=3)) + _names(_cl(130, 1030, levels=1))
    D["cs1_empty"] = _names(_cl(130, 1030, levels=3))
    D["cs0_unstaged"] = _names(_cl(101, 601))
    D["cs1_unstaged"] = _names(_cl(101, 601, levels=3))
    for k in ("stg_left", "stg_right", "row_above", "row_below"):  # the chain's hand-made centres point every way
        D["cs0_" + k] = _names(lambda S: S["family"] == "cells" and S["centres"] == "hand" and S["ref"] < 0 and S["H"] >= 8)
    D["cp_nopair"] = D["cf_past"] = D["cf_nopair"] = _names(_fam("cells"))
    D["cf_clamp"] = _names(_fam("cells", centres="hand", ref=2, levels=1))
    D["ns_ld_vec"] = _names(lambda S: S["family"] == "noise" and S["view"] == "grid" and S["roi"][1] % 8 == 0)
    D["ns_ld_unal"] = _names(lambda S: S["family"] == "noise" and (S["view"] != "grid" or S["roi"][1] % 8 != 0))
    D["ns_wg"] = D["ns_block"] = D["ns_rej_sat"] = D["ns_rej_lo"] = D["ns_accept"] = D["ns_hist_flush"] = D["ns_reg_flush"] = _names(_fam("noise"))
    D["ns_skip_t1"] = _names(lambda S: S["family"] == "noise" and (S["roi"][2] // 16) * _ceil(S["roi"][3] // 16, NS_SB) % 2 == 1)
    D["ns_skip_inactive"] = _names(lambda S: S["family"] == "noise" and (S["roi"][3] // 16) % NS_SB != 0)
    D["as1_ob1om0"] = _names(_al(70, 270))
    D["as0_om0"] = _names(_al(70, 74)) + _names(_al(80, 40))
    D["as0_ob1om0"] = _names(_al(44, 44))
    D["cs1_om1"] = _names(_cl(101, 601, levels=3))
    return D


DRIVEN = _driven()
# above zero in one of the settings named, by the samples: the clamps of a refinement level's margin at the frame's four edges, and
# an odd first column of the member's tile at the coarsest level of cells (the centres' parity)
DRIVEN_ANY = {k: _names(_cl(101, 601, levels=3)) + _names(_cl(130, 1030, levels=3)) for k in ("cs1_stg_left", "cs1_stg_right", "cs1_row_above", "cs1_row_below")}
DRIVEN_ANY["cs0_om0"] = DRIVEN_ANY["cs0_om1"] = _names(_fam("cells", centres="hand"))
