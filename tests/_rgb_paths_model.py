"""The corpus and the exact model of the demosaic kernels' path census (tests/test_gpu_rgb_paths.py, tests/test_rgb_paths_model.py).

krgb_mhc, krgb_bin2, krgb_bin2y (csrc/mcraw_rgb.hip), krgb_area (csrc/mcraw_area.hip) and krgb_resample (csrc/mcraw_resample.hip)
count what they do in a build with the census (csrc/mcraw_rgb_paths.h: RgbPath).  Nothing they do depends on content or timing:
every counter follows from the geometry of the call, the alignment of its buffers and the size of the grid.  This module states
the plans of the calls (rgb_check, AreaPlan, ResamplePlan of the csrc/*_args.h headers; tests/cpp/rgb_paths_plan.cpp prints the
headers' own for tests/test_rgb_paths_model.py), the walk of a persistent grid's workgroups over the units, and the load, store
and idle rules, as plain Python.  model(setting, variant) is the census of one call.

The corpus (SETTINGS): every kernel x {u8 hwc, u8 chw, u16 hwc, u16 chw, nv12, p010} x the four CFAs, one call of 5 frames with
per-frame colours each.  Per kernel two shapes -- each with at least two unit columns and two unit rows, a partial last column and
row; one with a unit count that 3 divides and one that it does not --, and over the settings every combination that selects a
path: the input on the 16-byte grid / with a pitch off it / with a base off the dword grid, the output on its grid / one sample off
it, a LUT of 4096 entries (LDS) / 65536 (global).  krgb_bin2 also takes a batch of 34 tiny frames, which a launch's RGB_MAXF = 32
colours split in two.  The float kinds have no loop: they run under the variants without a grid cap only."""
import functools

import numpy as np

import _area_ref as A
import _resample_ref as RS

RGB_T, MHC_TW, MHC_TH, RGB_MAXF = 256, 256, 32, 32
AREA_TILE_Q, AREA_WXN, AREA_YN, AREA_BAND, AREA_MAXRATIO = 2560, 4096, 128, 8, 16
RES_TW, RES_LYMAX, RES_TROWS, RES_ECOLS, RES_TAPS = 64, 16, 32, 144, 9

# the order of RgbPath in csrc/mcraw_rgb_paths.h
FAMILIES = ("mhc", "bin2", "bin2y", "area", "res")
GATHER_FAMILIES = ("warp", "mesh")  # krgb_warp, krgb_mesh and krgb_ha: their corpus and model are tests/_gather_paths_model.py's
WALK_FAMILIES = FAMILIES + GATHER_FAMILIES + ("ha",)
WALK = ("wg", "first", "later", "cross")
GATHER = ("ld_vec", "ld_elem", "a_even", "a_odd", "pix", "nopix", "cut_rows", "cut_cols", "tap_row_lo", "tap_row_hi", "tap_col_lo", "tap_col_hi",
          "st_idle_ly", "st_idle_x", "st_idle_row")
PATHS = (["%s_%s" % (w, f) for f in WALK_FAMILIES for w in WALK]
         + ["lut_lds", "lut_global", "idle_mhc_lane", "idle_mhc_rows", "idle_bin2", "idle_area", "idle_res",
            "ld_mhc_vec", "ld_mhc_elem", "ld_res_vec", "ld_res_elem", "ld_bin2_vec", "ld_bin2_elem", "ld_bin2y_vec", "ld_bin2y_elem",
            "ld_area_m2", "ld_area_m1", "ld_area_m0", "ld_area_tail", "ld_area_skip",
            "st_f_fast", "st_f_crop", "st_f_off", "st_c8_fast", "st_c8_crop", "st_c8_off", "st_c16_fast", "st_c16_crop", "st_c16_off",
            "st_h8_16_8", "st_h8_8_16", "st_h8_elem", "st_h16_fast", "st_h16_elem",
            "st_yl_fast", "st_yl_crop", "st_yl_off", "st_yc_fast", "st_yc_crop", "st_yc_off"]
         + ["%s_%s" % (f, g) for f in GATHER_FAMILIES for g in GATHER]
         + ["mesh_narrow", "mesh_wide", "mesh_y_lo", "mesh_y_hi", "mesh_x_lo", "mesh_x_hi", "ha_ld_vec", "ha_ld_elem", "ha_continue", "ha_break"]
         + ["ha_%s_%s" % (s, o) for s in ("main", "edge", "diag") for o in ("a", "b", "eq")])

VARIANT_CAP = {"census": None, "grid1": 1, "grid3": 3, "poison": None, "poison1": 1}
PRODUCT_OF = {"poison": "census", "poison1": "grid1"}  # the variants whose counts are another's

CFAS = ("rggb", "bggr", "grbg", "gbrg")
LUT_KINDS = ("u8hwc", "u8chw", "u16hwc", "u16chw", "nv12", "p010")
FLOAT_KINDS = ("f32", "f16", "bf16")
ES = {"u8hwc": 1, "u8chw": 1, "u16hwc": 2, "u16chw": 2, "nv12": 1, "p010": 2, "f32": 4, "f16": 2, "bf16": 2}
IN_BITS = 12
WHITE, BLACK = 4095.0, (64, 60, 66, 62)

# Per kernel two shapes.  mhc: (W, H); bin2: (W, H), and for the YUV kinds (W and H multiples of 4) the second pair; the scaled
# kernels: the frame, the crop (y0, x0, h, w) and the output size (Ho, Wo), at a fractional ratio with an offset crop.  krgb_area's
# crop ends at the frame's right edge, whose quad count 4 does not divide: the last piece of a row has a zero-filled tail.
SHAPES = {
    "mhc": [dict(W=516, H=70), dict(W=258, H=34)],                                  # 3 x 3 tiles (4 columns, 6 rows left); 2 x 2
    "bin2": [dict(W=520, H=70, yuv=(520, 72)), dict(W=520, H=92, yuv=(520, 100))],  # 5 and 6 units; bin2y: 3 and 4
    "area": [dict(W=2438, H=120, crop=(4, 18, 102, 2420), size=(22, 524)),          # 2 column tiles x 2 bands
             dict(W=2438, H=190, crop=(6, 18, 176, 2420), size=(38, 524))],         # 2 x 3
    "resample": [dict(W=220, H=60, crop=(6, 4, 38, 192), size=(30, 148), filt="cubic"),
                 dict(W=220, H=60, crop=(4, 4, 28, 110), size=(22, 84), filt="linear")],
}
TINY = dict(W=16, H=8, n=34)  # one unit per frame


def _layout(W, H, n, in_align):
    """(offset, pitch, frame stride) of the input in uint16 elements from a 16-byte aligned allocation: 0 on the 16-byte grid;
    1 the pitch off it (even: dwords stay aligned); 2 the base one sample behind the allocation."""
    up = (W + 7) // 8 * 8 + 8
    if in_align == 1:
        pitch = W + 2 if (W + 2) % 8 else W + 4
        return 0, pitch, pitch * H + 2
    return (1 if in_align == 2 else 0), up, up * H + 8


def _setting(kernel, kind, cfa, shape, in_align, out_off, lutn, n=5, **over):
    S = dict(SHAPES[kernel][shape], kernel=kernel, kind=kind, cfa=cfa, shape=shape, in_align=in_align, out_off=out_off, lutn=lutn, n=n)
    S.update(over)
    if kernel == "bin2" and kind in ("nv12", "p010"):
        S["W"], S["H"] = S["yuv"]
    S.pop("yuv", None)
    S["name"] = "%s-%s-%s-s%d-i%d-o%d-l%d-n%d" % (kernel, kind, cfa, shape, in_align, out_off, lutn, S["n"])
    S["off"], S["pitch"], S["fstride"] = _layout(S["W"], S["H"], S["n"], in_align)
    return S


def _settings():
    out = []
    for kernel in SHAPES:
        for ki, kind in enumerate(LUT_KINDS):
            for ci, cfa in enumerate(CFAS):
                shape = (ci + ki) % 2
                lutn = 65536 if ((ci >> 1) + ki) % 2 else 4096
                in_align = (ci + ki // 2) % 3
                out_off = ES[kind] * ((ci + (ki >> 1) + (ci >> 1)) % 2)
                out.append(_setting(kernel, kind, cfa, shape, in_align, out_off, lutn))
        for ki, kind in enumerate(FLOAT_KINDS):
            out.append(_setting(kernel, kind, CFAS[ki], ki % 2, ki % 3, ES[kind] * (ki % 2), 0, n=2))
    out.append(_setting("bin2", "u8chw", "grbg", 0, 0, 0, 4096, n=TINY["n"], W=TINY["W"], H=TINY["H"]))
    return {S["name"]: S for S in out}


SETTINGS = _settings()


def is_float(S):
    return S["kind"] in FLOAT_KINDS


def is_yuv(S):
    return S["kind"] in ("nv12", "p010")


def family(S):
    return {"mhc": "mhc", "bin2": "bin2y" if is_yuv(S) else "bin2", "area": "area", "resample": "res"}[S["kernel"]]


def runs(S, variant):
    """Whether `variant`'s child runs the setting: the float kinds have no loop to force."""
    return not is_float(S) or VARIANT_CAP[variant] is None


def colours(S):
    """Per-frame gains (n, 3) and matrices (n, 3, 3), f32, that differ visibly from frame to frame."""
    i = np.arange(S["n"], dtype=np.float32)
    gain = np.stack([1.2 + 0.17 * (i % 7), np.ones_like(i), 1.9 - 0.13 * (i % 5)], axis=1).astype(np.float32)
    base = np.array([[1.6, -0.4, -0.2], [-0.3, 1.5, -0.2], [0.05, -0.55, 1.5]], dtype=np.float32)
    m = np.stack([base * np.float32(1.0 - 0.06 * (k % 6)) + np.float32(0.02 * (k % 4)) for k in range(S["n"])]).astype(np.float32)
    return gain, m


# ---- the plans (csrc/mcraw_rgb_args.h, mcraw_area_args.h, mcraw_resample_args.h)

def on_grid(S):
    return S["off"] % 8 == 0 and S["pitch"] % 8 == 0 and (S["n"] == 1 or S["fstride"] % 8 == 0)


def area_mode(S):
    if on_grid(S):
        return 2
    return 1 if S["off"] % 2 == 0 and S["pitch"] % 2 == 0 and (S["n"] == 1 or S["fstride"] % 2 == 0) else 0


def rgb_plan(S):
    W, H = S["W"], S["H"]
    if S["kernel"] == "mhc":
        tilesX = (W + MHC_TW - 1) // MHC_TW
        return dict(Wo=W, Ho=H, tilesX=tilesX, units=tilesX * ((H + MHC_TH - 1) // MHC_TH), invec=int(on_grid(S)))
    Wo, Ho = W // 2, H // 2
    tilesX = (Wo + 7) // 8
    return dict(Wo=Wo, Ho=Ho, tilesX=tilesX, units=(tilesX * (Ho // 2 if is_yuv(S) else Ho) + RGB_T - 1) // RGB_T, invec=int(on_grid(S)))


def area_plan(S):
    (y0, x0, ch, cw), (Ho, Wo) = S["crop"], S["size"]
    Qw, Qh = cw // 2, ch // 2
    assert 1 <= Wo <= Qw <= AREA_MAXRATIO * Wo and 1 <= Ho <= Qh <= AREA_MAXRATIO * Ho
    bound = lambda Q, O: Q // O + 2 if Q % O else Q // O
    ntx, nty = bound(Qw, Wo), bound(Qh, Ho)
    cols8, pairs = (Wo + 7) // 8, (Ho + 1) // 2
    seg_of = lambda lx: ((8 * lx * Qw + Wo - 1) // Wo + 1 + 7 + 3 + 3) & ~3
    pad = lambda s: s + s // 8 + 1
    lx, l2 = 1, 0
    while lx < RGB_T and lx < cols8:
        lx, l2 = lx * 2, l2 + 1
    while lx > 1 and (pad(seg_of(lx)) > AREA_TILE_Q or 8 * lx * ntx > AREA_WXN):
        lx, l2 = lx // 2, l2 - 1
    seg = seg_of(lx)
    segp = pad(seg)
    ly = min(RGB_T // lx, AREA_YN // 2)
    while ly > 1 and (ly * segp > AREA_TILE_Q or ly // 2 >= pairs):
        ly //= 2
    tilesX, groups = (cols8 + lx - 1) // lx, (pairs + ly - 1) // ly
    bands = (groups + AREA_BAND - 1) // AREA_BAND
    return dict(Wo=Wo, Ho=Ho, Qw=Qw, Qh=Qh, ntx=ntx, nty=nty, mode=area_mode(S), lx_log2=l2, ly=ly, seg=seg, segp=segp, nch=seg // 4,
                tilesX=tilesX, groups=groups, bands=bands, units=tilesX * bands)


def resample_plan(S):
    (y0, x0, ch, cw), (Ho, Wo) = S["crop"], S["size"]
    filt = RS.FILTER_CODE[S["filt"]]
    assert 2 * Wo >= cw and Wo <= 2 * cw and 2 * Ho >= ch and Ho <= 2 * ch

    def tap_bound(C, O):
        reach = (4 if filt else 2) * max(C, O) // O + 1
        return 1 if C == O else min(reach, RES_TAPS if filt else 5)
    span = lambda m, C, O, nt: (m * C + O - 1) // O + 2 + nt
    rows_of = lambda ly, C, O, nt: (span(2 * ly - 1, C, O, nt) + 2) // 2 * 2
    ntx, nty = tap_bound(cw, Wo), tap_bound(ch, Ho)
    ecols = (span(RES_TW - 1, cw, Wo, ntx) + 6) // 8 * 8 + 8
    ly = RES_LYMAX
    while ly > 1 and (rows_of(ly, ch, Ho, nty) > RES_TROWS or ly // 2 >= (Ho + 1) // 2):
        ly //= 2
    tilesX = (Wo + RES_TW - 1) // RES_TW
    bands = ((Ho + 1) // 2 + ly - 1) // ly
    return dict(Wo=Wo, Ho=Ho, ntx=ntx, nty=nty, ly=ly, ecols=ecols, erows=rows_of(ly, ch, Ho, nty), tilesX=tilesX, bands=bands,
                units=tilesX * bands, invec=int(on_grid(S)))


def plan(S):
    return {"mhc": rgb_plan, "bin2": rgb_plan, "area": area_plan, "resample": resample_plan}[S["kernel"]](S)


def out_frame_bytes(S):
    P = plan(S)
    return (P["Ho"] * P["Wo"] * 3 // 2 if is_yuv(S) else 3 * P["Ho"] * P["Wo"]) * ES[S["kind"]]


# ---- the walk

def launches(S):
    """Frames per launch: the colours are per frame, so a batch goes in pieces of RGB_MAXF frames."""
    return [min(RGB_MAXF, S["n"] - f0) for f0 in range(0, S["n"], RGB_MAXF)]


def walk(units, nf, grid):
    """(first, later, crossings) of a persistent launch: workgroup b takes t = b, b + grid, .. < units * nf; unit t is of frame
    t // units."""
    total = units * nf
    assert 1 <= grid <= total
    first = later = cross = 0
    for b in range(grid):
        prev = None
        for t in range(b, total, grid):
            f = t // units
            if prev is None:
                first += 1
            else:
                later += 1
                cross += f != prev
            prev = f
    return first, later, cross


def grids(S, variant, resident=None):
    """The grid of every launch.  Under a cap: min(units * nf, cap).  Else min(units * nf, resident): `resident` is what the census
    reports for a call of one launch; a call of several launches is taken to fit the device (the test asserts it)."""
    units, cap = plan(S)["units"], VARIANT_CAP[variant]
    if is_float(S):
        return [units * nf for nf in launches(S)]
    lim = cap if cap is not None else resident if resident is not None else 1 << 30
    return [min(units * nf, lim) for nf in launches(S)]


# ---- loads and idle work, per unit

def _mhc_unit(S, P, u, c):
    W, H = S["W"], S["H"]
    x0, y0 = u % P["tilesX"] * MHC_TW, u // P["tilesX"] * MHC_TH
    for q in range((MHC_TW + 16) // 8):
        xs = x0 - 8 + 8 * q
        c["ld_mhc_vec" if P["invec"] and xs >= 0 and xs + 8 <= W else "ld_mhc_elem"] += MHC_TH + 4
    for lx in range(32):
        if x0 + 8 * lx >= W:
            c["idle_mhc_lane"] += 8
            continue
        for ly in range(8):
            for ps in range(MHC_TH // 16):
                if y0 + 2 * (ly + 8 * ps) >= H:
                    c["idle_mhc_rows"] += 1
                    break


def _bin2_unit(S, P, u, c):
    yuv = is_yuv(S)
    for item in range(u * RGB_T, (u + 1) * RGB_T):
        yo, xo = item // P["tilesX"] * (2 if yuv else 1), 8 * (item % P["tilesX"])
        if yo >= P["Ho"]:
            c["idle_bin2"] += 1
            continue
        vec = P["invec"] and min(8, P["Wo"] - xo) == 8
        c[("ld_bin2y_" if yuv else "ld_bin2_") + ("vec" if vec else "elem")] += 2 if yuv else 1


@functools.lru_cache(maxsize=None)
def _area_taps(Q, O):
    q0, w = A.weights(Q, O)
    nt = np.where(w != 0, np.arange(A.TAPS)[None, :] + 1, 0).max(axis=1)
    return q0, nt


def _area_unit(S, P, u, c):
    (y0, x0, ch, cw), Wo, Ho = S["crop"], P["Wo"], P["Ho"]
    QW, lx, ly, nch = S["W"] // 2, 1 << P["lx_log2"], P["ly"], P["nch"]
    xq0, _ = _area_taps(P["Qw"], Wo)
    _, ynt = _area_taps(P["Qh"], Ho)
    tx, band = u % P["tilesX"], u // P["tilesX"]
    k0 = tx * 8 * lx
    qb = (x0 // 2 + int(xq0[k0])) & ~7
    cols_on = sum(1 for l in range(lx) if k0 + 8 * l < Wo)
    piece = {"ld_area_m2": 0, "ld_area_m1": 0, "ld_area_m0": 0, "ld_area_tail": 0}
    for chk in range(nch):
        aq = qb + 4 * chk
        if P["mode"] == 2 and aq + 4 <= QW:
            piece["ld_area_m2"] += 1
        else:
            piece["ld_area_m1" if P["mode"] else "ld_area_m0"] += 1
            piece["ld_area_tail"] += aq + 3 >= QW
    for g in range(AREA_BAND):
        grp = band * AREA_BAND + g
        if grp >= P["groups"]:
            break
        for a in range(2):
            rows = [2 * (grp * ly + l) + a for l in range(ly)]
            c["idle_area"] += RGB_T - cols_on * sum(1 for j in rows if j < Ho)
            for j in rows:
                live = min(int(ynt[j]), P["nty"]) if j < Ho else 0
                c["ld_area_skip"] += nch * (P["nty"] - live)
                for k, v in piece.items():
                    c[k] += v * live


@functools.lru_cache(maxsize=None)
def _res_taps(C, O, filt):
    j0, nt, _ = RS.weights(C, O, filt)
    return j0, nt


def _res_unit(S, P, u, c):
    (y0, x0, ch, cw), Wo, Ho, W = S["crop"], P["Wo"], P["Ho"], S["W"]
    xj, xn = _res_taps(cw, Wo, S["filt"])
    yj, yn = _res_taps(ch, Ho, S["filt"])
    tx, band = u % P["tilesX"], u // P["tilesX"]
    k0 = tx * RES_TW
    k1 = min(k0 + RES_TW, Wo) - 1
    i0 = band * 2 * P["ly"]
    i1 = min(i0 + 2 * P["ly"], Ho) - 1
    k0b, k1b, i0b, i1b = min(k0 + 1, k1), max(k1, k0 + 1) - 1, min(i0 + 1, i1), max(i1, i0 + 1) - 1
    cf = x0 + min(int(xj[k0]), int(xj[k0b]))
    cl = x0 + max(int(xj[k1] + xn[k1]), int(xj[k1b] + xn[k1b])) - 1
    rf = y0 + min(int(yj[i0]), int(yj[i0b]))
    rl = y0 + max(int(yj[i1] + yn[i1]), int(yj[i1b] + yn[i1b])) - 1
    eb, pb = cf & ~7, rf & ~1
    ne, npairs = min(((cl - eb) >> 3) + 1, RES_ECOLS // 8), min(((rl - pb) >> 1) + 1, RES_TROWS // 2)
    for q in range(ne + 2):
        xs = eb - 8 + 8 * q
        c["ld_res_vec" if P["invec"] and xs >= 0 and xs + 8 <= W else "ld_res_elem"] += 2 * npairs + 4
    on = sum(1 for lxid in range(8) for lyid in range(32) if lyid < P["ly"] and k0 + 8 * lxid < Wo and i0 + 2 * lyid <= i1)
    c["idle_res"] += RGB_T - on


_UNIT = {"mhc": _mhc_unit, "bin2": _bin2_unit, "area": _area_unit, "resample": _res_unit}


# ---- stores

def _forms(c, keys, addr, n, align):
    full = n == 8
    on = addr % align == 0
    c[keys[0]] += int((full & on).sum())
    c[keys[1]] += int((~full).sum())
    c[keys[2]] += int((full & ~on).sum())


def stores(S, c):
    """Every 8-sample piece of every output row is stored once, whichever kernel and walk: the form follows from its address (the
    output starts out_off bytes behind a 16-byte boundary) and from n, the samples of the 8 that exist."""
    P = plan(S)
    stores_of(c, S["kind"], P["Wo"], P["Ho"], S["n"], S["out_off"], out_frame_bytes(S))


def stores_of(c, kind, Wo, Ho, nframes, out_off, frame_bytes):
    """stores() for any kernel: nframes frames of Ho x Wo of `kind`, frame_bytes apart, from out_off bytes behind a 16-byte boundary."""
    es, yuv, flt = ES[kind], kind in ("nv12", "p010"), kind in FLOAT_KINDS
    y, x = np.meshgrid(np.arange(Ho, dtype=np.int64), np.arange(0, Wo, 8, dtype=np.int64), indexing="ij")
    n = np.minimum(8, Wo - x)
    for f in range(nframes):
        base = out_off + f * frame_bytes
        if yuv:
            _forms(c, ("st_yl_fast", "st_yl_crop", "st_yl_off"), base + (y * Wo + x) * es, n, 8 * es)
            odd = (y & 1) == 1
            _forms(c, ("st_yc_fast", "st_yc_crop", "st_yc_off"), (base + ((Ho + (y >> 1)) * Wo + x) * es)[odd], n[odd], 8 * es)
        elif kind in ("u8hwc", "u16hwc"):
            a = base + (y * Wo + x) * 3 * es
            fast = (n == 8) & (a % (8 * es) == 0)
            if es == 1:
                c["st_h8_16_8"] += int((fast & ((a & 8) == 0)).sum())
                c["st_h8_8_16"] += int((fast & ((a & 8) != 0)).sum())
                c["st_h8_elem"] += int((~fast).sum())
            else:
                c["st_h16_fast"] += int(fast.sum())
                c["st_h16_elem"] += int((~fast).sum())
        else:
            pre = "st_f" if flt else "st_c8" if es == 1 else "st_c16"
            align = 16 if flt else 8 * es
            for r in range(3):
                _forms(c, (pre + "_fast", pre + "_crop", pre + "_off"), base + (r * Ho * Wo + y * Wo + x) * es, n, align)


# ---- the census of a call

@functools.lru_cache(maxsize=None)
def _model(name, variant, resident):
    S = SETTINGS[name]
    P, fam = plan(S), family(S)
    c = dict.fromkeys(PATHS, 0)
    for nf, grid in zip(launches(S), grids(S, variant, resident)):
        total = P["units"] * nf
        if is_float(S):
            first, later, cross = total, 0, 0
        else:
            first, later, cross = walk(P["units"], nf, grid)
            c["lut_global" if S["lutn"] > 4096 else "lut_lds"] += total
        for k, v in zip(WALK, (grid, first, later, cross)):
            c["%s_%s" % (k, fam)] += v
    per_frame = dict.fromkeys(PATHS, 0)
    for u in range(P["units"]):
        _UNIT[S["kernel"]](S, P, u, per_frame)
    for k, v in per_frame.items():
        c[k] += v * S["n"]
    stores(S, c)
    return c


def model(name, variant="census", resident=None):
    """The census of setting `name` in the build `variant`."""
    return dict(_model(name, variant, resident))


# ---- which settings must drive which counter (the product's way: variants `census` and `poison`), by the corpus' own attributes

def _driven():
    D = {k: [] for k in PATHS}
    for name, S in SETTINGS.items():
        fam, kind, es = family(S), S["kind"], ES[S["kind"]]
        on_out = S["out_off"] == 0
        for k in ("wg", "first"):
            D["%s_%s" % (k, fam)].append(name)
        if not is_float(S):
            D["lut_global" if S["lutn"] > 4096 else "lut_lds"].append(name)
        grid_in = S["in_align"] == 0
        if S["kernel"] == "mhc":
            D["idle_mhc_lane"].append(name), D["idle_mhc_rows"].append(name), D["ld_mhc_elem"].append(name)
            if grid_in:
                D["ld_mhc_vec"].append(name)
        elif S["kernel"] == "bin2":
            D["idle_bin2"].append(name)
            if S["W"] != TINY["W"]:
                D["ld_%s_elem" % fam].append(name)  # (the partial last column)
            if grid_in:
                D["ld_%s_vec" % fam].append(name)
        elif S["kernel"] == "area":
            D["idle_area"].append(name), D["ld_area_skip"].append(name)
            D["ld_area_m%d" % area_mode(S)].append(name)
            D["ld_area_tail"].append(name)
            if grid_in:
                D["ld_area_m1"].append(name)  # (the piece with the tail)
        else:
            D["idle_res"].append(name), D["ld_res_elem"].append(name)
            if grid_in:
                D["ld_res_vec"].append(name)
        if is_yuv(S):
            for p in ("st_yl", "st_yc"):
                D[p + "_crop"].append(name)
                D[p + ("_fast" if on_out else "_off")].append(name)
        elif kind == "u8hwc":
            D["st_h8_elem"].append(name)
            if on_out:
                D["st_h8_16_8"].append(name), D["st_h8_8_16"].append(name)
        elif kind == "u16hwc":
            D["st_h16_elem"].append(name)
            if on_out:
                D["st_h16_fast"].append(name)
        else:
            pre = "st_f" if is_float(S) else "st_c8" if es == 1 else "st_c16"
            if S["W"] != TINY["W"]:
                D[pre + "_crop"].append(name)
            D[pre + ("_fast" if on_out else "_off")].append(name)
    return D


DRIVEN = _driven()
# under a grid cap every call with a LUT also has later units and frame crossings
DRIVEN_CAPPED = {"%s_%s" % (k, f): [n for n, S in SETTINGS.items() if family(S) == f and not is_float(S)] for f in FAMILIES for k in ("later", "cross")}
