"""The corpus of tests/test_gpu_mosaic_paths.py and the exact model of the path census of the mosaic stages
(csrc/mcraw_mosaic_paths.h): kshade, kstats, kmerge<0|1> (plain and cell field), kfixpix + kfixpix_list, kdenoise<1|2>, khl_apply, khl_measure, khl_clip.

SETTINGS names every call of the corpus: the family, the size (H, W), the view of the input and of the output (`grid`: contiguous
on the 16-byte grid; `off`: a base 2 bytes off it; `pitch`: a pitch of W + 3 samples), the content and the parameters.  The
contents are made here, from a seed per setting, because the data-path counters depend on them.

model(name, variant) gives every counter of PATHS for that call: the walk, the staging pieces, the direct loads and the stores
from the geometry and the views alone; the data-path counters from the samples -- the model stages every LDS tile as the kernel
does (stage(): which chunks are vector pieces, element pieces through the stage's reflection, or left as they are) and evaluates
the kernels' predicates on it with the kernels' lane-to-pixel map.  A chunk that staging leaves as it is holds 0xFFFF in the
`poison` builds; in the others it holds what LDS held, and a lane row whose predicate (`cand` of kfixpix, `clipped` of khl_apply)
reads such a chunk without being decided by the samples it does know is left out of the exact comparison of those predicates'
counters: model()["_unstaged"] maps each such counter to (lowest, highest) it can be, and to how many lane rows that is owed.
No other counter has such a range.  div_round's two correction steps are the chip's (v_rcp_f32): the model gives its calls."""
import functools

import numpy as np

import _fixpix_ref as FX
import _highlights_ref as HR

PATHS = ["wg", "idle_lane", "row_break", "row_cont",
         "stg_vec", "stg_unal", "stg_halo", "stg_crop", "stg_skip",
         "ld_vec", "ld_unal", "ld_elem",
         "st_vec", "st_unal", "st_elem",
         "fp_wave_any", "fp_wave_none", "fp_cand", "fp_hot", "fp_cold", "fp_listed", "fp_flag",
         "fl_wg", "fl_past", "fl_outside", "fl_written", "fl_nopair",
         "dn_edgex", "dn_sy1", "dn_sy2", "dn_sy3", "dn_both",
         "hl_clipped", "hl_unclipped", "hl_rebuilt", "hl_left", "hl_top",
         "hm_measured", "hm_own", "hm_neighbour",
         "ss_full", "ss_partial", "ss_empty", "ss_onebin", "ss_prefetch", "ss_ld_edge", "ss_row_out",
         "mg_short", "mg_launch", "mg_zero", "mg_cut", "mg_self", "mg_zerow", "mg_staged", "mg_m_aligned", "mg_m_sx", "mg_m_invec",
         "div_calls", "div_down", "div_up"]
UNMODELLED = ("div_down", "div_up")
VARIANTS = ("census", "slow", "poison", "poisonslow", "pieces", "th16")  # build.MOSAIC_PATH_VARIANTS
EXTRA_VARIANTS = ("frames2",)                                             # build.MOSAIC_FRAMES2_FLAGS
FRAMES = 3
MG_FRAMES = 7  # frames of a merge call
MG_WINDOWS = ((0, 0), (2, 2), (5, 0))  # (before, after)
MG_CELL = (32, 256)
SIZES = ((1, 1), (2, 2), (5, 4), (7, 6), (6, 7), (9, 9), (33, 1), (1, 64), (17, 255), (31, 257), (34, 264), (35, 520))  # (H, W)
VIEWS = ("grid", "off", "pitch")
TILE_W, TILE_LW, TILE_CH = 256, 272, 34
POISON = 0xFFFF

# fixpix
FP_BLACK, FP_ABS, FP_REL = (64, 60, 66, 64), (48, 40, 44, 48), 0.25
# denoise
DN_SHIFT, DN_L = 4, 256
# highlights
HL_SAT, HL_BLACK, HL_GAIN, HL_CFA, HL_TOP = (3900, 4000, 4000, 3950), (64, 60, 66, 64), (8192, 4096, 4096, 6144), "rggb", 5000
HL_LO = HR.default_lo(HL_SAT, HL_BLACK)
# shade
SH_BLACK, SH_TOP = (64, 60, 66, 64), 4095
# stats: bins -> shift; a workgroup takes at most ST_MAXTILES tiles (2 in the `pieces` build), a launch aims at ST_WGS workgroups
ST_SAT, ST_SHIFT, ST_MAXTILES, ST_WGS = (3900, 4000, 4000, 3950), {64: 6, 4096: 0}, 8192, 2048


def _settings():
    S = {}

    def add(family, H, W, view, content, **kw):
        name = "/".join([family, "%dx%d" % (H, W), view, content] + ["%s=%s" % (k, kw[k]) for k in sorted(kw)])
        S[name] = dict(kw, name=name, family=family, H=H, W=W, view=view, content=content, seed=len(S) + 1)

    for i, (H, W) in enumerate(SIZES):
        for j, view in enumerate(VIEWS):
            add("shade", H, W, view, "noise", permap=(i + j) & 1)
            add("stats", H, W, view, "noise", bins=(64, 4096)[(i + j) & 1], roi=0)
            if H >= 17 and W >= 17:  # a window that cuts tiles on all four sides, at an odd offset
                add("stats", H, W, view, "noise", bins=(4096, 64)[(i + j) & 1], roi=1)
            # rank, the counts record and the list change with the view; `planted` has both row ends of every kind
            add("fixpix", H, W, view, "noise", rank=1 + (i + j) % 2, counts=int(view != "pitch"), list=0)
            add("fixpix", H, W, view, "planted", rank=2 - (i + j) % 2, counts=int(view != "off"), list=1)
            for radius in (1, 2):
                add("denoise", H, W, view, "noise", radius=radius, amount=(256, 77)[(i + j) & 1], perlut=(i + j + radius) & 1)
            if H >= 2 and W >= 2:
                add("hl_apply", H, W, view, "patch", rec=(i + j) & 1)
                add("hl_measure", H, W, view, "patch")
                add("hl_clip", H, W, view, "patch")
            k = i + j
            add("merge", H, W, view, "noise", window=k % 3, support=k & 1, pos=("none", "m8", "even")[(k // 2) % 3], first=0, count=MG_FRAMES,
                perlut=k & 1)
            if (H, W) in ((9, 9), (31, 257), (34, 264), (35, 520)):
                add("merge_cells", H, W, view, "noise", window=1 + (k & 1), support=(k + 1) & 1, pos="cells", first=0, count=MG_FRAMES, perlut=0)
            if (H, W) == (35, 520):  # shifts larger than a tile: some tiles pass members over; a launch that starts at base 1
                for support in (0, 1):
                    add("merge", H, W, view, "noise", window=1, support=support, pos="big", first=1, count=5, perlut=0)
                add("merge", H, W, view, "noise", window=2, support=j & 1, pos="m8", first=0, count=MG_FRAMES, perlut=1)
                add("merge", H, W, view, "noise", window=1, support=(j + 1) & 1, pos="even", first=0, count=MG_FRAMES, perlut=0)
        if H * W >= 64:
            add("fixpix", H, W, "grid", "flat", rank=2, counts=1, list=0)
        if H * W >= 4096:  # quotients near 60000: div_round's float estimate is off by up to 0.01 there, and steps down as well as up
            for radius in (1, 2):
                add("denoise", H, W, "grid", "bright", radius=radius, amount=256, perlut=0)
        if H >= 2 and W >= 64:
            for content in ("flatlow", "flatsat"):
                add("stats", H, W, "grid", content, bins=(64, 4096)[i & 1], roi=0)
                add("hl_apply", H, W, "grid", content, rec=0)
                add("hl_measure", H, W, "grid", content)
    return S


SETTINGS = _settings()

# counter -> the settings in which it must be above zero in the `census` build (tests/test_mosaic_paths_model.py checks that the
# model says so, before any GPU time is spent)
DRIVEN = {
    "wg": ["shade/1x1/grid/noise/permap=0", "hl_clip/35x520/pitch/patch", "stats/35x520/pitch/noise/bins=4096/roi=0"],
    "idle_lane": ["shade/1x1/grid/noise/permap=0", "fixpix/35x520/grid/noise/counts=1/list=0/rank=2", "hl_clip/2x2/grid/patch"],
    "row_break": ["denoise/35x520/grid/noise/amount=77/perlut=0/radius=1", "denoise/1x1/off/noise/amount=77/perlut=1/radius=2"],
    "row_cont": ["shade/17x255/grid/noise/permap=0", "fixpix/35x520/grid/noise/counts=1/list=0/rank=2", "hl_apply/35x520/off/patch/rec=0",
                 "hl_measure/35x520/grid/patch", "hl_clip/35x520/grid/patch"],
    "stg_vec": ["fixpix/34x264/grid/noise/counts=1/list=0/rank=1", "denoise/35x520/grid/noise/amount=77/perlut=0/radius=1",
                "hl_apply/34x264/grid/patch/rec=0", "hl_measure/34x264/grid/patch"],
    "stg_unal": ["fixpix/34x264/off/noise/counts=1/list=0/rank=2", "fixpix/34x264/pitch/noise/counts=0/list=0/rank=1",
                 "denoise/35x520/off/noise/amount=256/perlut=1/radius=1", "hl_apply/34x264/pitch/patch/rec=0", "hl_measure/34x264/off/patch"],
    "stg_halo": ["fixpix/1x1/grid/noise/counts=1/list=0/rank=1", "denoise/2x2/grid/noise/amount=77/perlut=1/radius=2", "hl_apply/2x2/grid/patch/rec=1"],
    "stg_crop": ["fixpix/17x255/grid/noise/counts=1/list=0/rank=1", "denoise/31x257/grid/noise/amount=77/perlut=1/radius=2",
                 "hl_apply/31x257/grid/patch/rec=1", "hl_measure/9x9/grid/patch"],
    "stg_skip": ["fixpix/1x1/grid/noise/counts=1/list=0/rank=1", "denoise/35x520/grid/noise/amount=77/perlut=1/radius=2",
                 "hl_apply/35x520/grid/patch/rec=1", "hl_measure/2x2/grid/patch"],
    "ld_vec": ["shade/34x264/grid/noise/permap=0", "hl_clip/34x264/grid/patch", "stats/34x264/grid/noise/bins=64/roi=0"],
    "ld_unal": ["stats/34x264/off/noise/bins=4096/roi=0", "shade/34x264/off/noise/permap=1", "shade/34x264/pitch/noise/permap=0", "hl_clip/34x264/off/patch", "hl_clip/34x264/pitch/patch"],
    "ld_elem": ["shade/1x1/grid/noise/permap=0", "shade/31x257/grid/noise/permap=1", "hl_clip/17x255/grid/patch"],
    "st_vec": ["shade/34x264/grid/noise/permap=0", "fixpix/34x264/grid/noise/counts=1/list=0/rank=1",
               "denoise/34x264/grid/noise/amount=256/perlut=1/radius=1", "hl_apply/34x264/grid/patch/rec=0", "hl_clip/34x264/grid/patch"],
    "st_unal": ["shade/34x264/off/noise/permap=1", "fixpix/34x264/pitch/noise/counts=0/list=0/rank=1",
                "denoise/34x264/off/noise/amount=77/perlut=0/radius=1", "hl_apply/34x264/pitch/patch/rec=0", "hl_clip/34x264/off/patch"],
    "st_elem": ["shade/5x4/grid/noise/permap=0", "fixpix/17x255/grid/noise/counts=1/list=0/rank=1",
                "denoise/31x257/grid/noise/amount=77/perlut=1/radius=2", "hl_apply/6x7/grid/patch/rec=0", "hl_clip/9x9/grid/patch"],
    "fp_wave_any": ["fixpix/35x520/grid/noise/counts=1/list=0/rank=2", "fixpix/35x520/grid/planted/counts=1/list=1/rank=1"],
    "fp_wave_none": ["fixpix/35x520/grid/flat/counts=1/list=0/rank=2", "fixpix/35x520/grid/planted/counts=1/list=1/rank=1"],
    "fp_cand": ["fixpix/9x9/pitch/planted/counts=1/list=1/rank=1", "fixpix/35x520/grid/planted/counts=1/list=1/rank=1"],
    "fp_hot": ["fixpix/35x520/grid/planted/counts=1/list=1/rank=1", "fixpix/35x520/grid/noise/counts=1/list=0/rank=2"],
    "fp_cold": ["fixpix/35x520/grid/planted/counts=1/list=1/rank=1", "fixpix/35x520/grid/noise/counts=1/list=0/rank=2"],
    "fp_listed": ["fixpix/35x520/grid/planted/counts=1/list=1/rank=1", "fixpix/17x255/pitch/planted/counts=1/list=1/rank=2"],
    "fp_flag": ["fixpix/35x520/grid/planted/counts=1/list=1/rank=1"],
    "fl_wg": ["fixpix/35x520/grid/planted/counts=1/list=1/rank=1"],
    "fl_past": ["fixpix/35x520/grid/planted/counts=1/list=1/rank=1"],
    "fl_outside": ["fixpix/35x520/grid/planted/counts=1/list=1/rank=1", "fixpix/1x1/grid/planted/counts=1/list=1/rank=2"],
    "fl_written": ["fixpix/35x520/grid/planted/counts=1/list=1/rank=1"],
    "fl_nopair": ["fixpix/1x1/grid/planted/counts=1/list=1/rank=2"],
    "dn_edgex": ["denoise/1x1/grid/noise/amount=256/perlut=0/radius=2", "denoise/35x520/grid/noise/amount=77/perlut=1/radius=2"],
    "dn_sy1": ["denoise/35x520/grid/noise/amount=77/perlut=1/radius=2", "denoise/7x6/grid/noise/amount=77/perlut=1/radius=2"],
    "dn_sy2": ["denoise/35x520/grid/noise/amount=77/perlut=1/radius=2", "denoise/7x6/grid/noise/amount=77/perlut=1/radius=2"],
    "dn_sy3": ["denoise/7x6/grid/noise/amount=77/perlut=1/radius=2", "denoise/6x7/grid/noise/amount=256/perlut=0/radius=2"],
    "dn_both": ["denoise/7x6/grid/noise/amount=77/perlut=1/radius=2", "denoise/6x7/grid/noise/amount=256/perlut=0/radius=2"],
    "hl_clipped": ["hl_apply/35x520/grid/patch/rec=1", "hl_apply/35x520/grid/flatsat/rec=0"],
    "hl_unclipped": ["hl_apply/35x520/grid/patch/rec=1", "hl_apply/35x520/grid/flatlow/rec=0"],
    "hl_rebuilt": ["hl_apply/35x520/grid/patch/rec=1", "hl_apply/35x520/off/patch/rec=0"],
    "hl_left": ["hl_apply/35x520/grid/patch/rec=1", "hl_apply/35x520/grid/flatsat/rec=0"],
    "hl_top": ["hl_apply/35x520/grid/patch/rec=1"],
    "hm_measured": ["hl_measure/35x520/grid/patch", "hl_measure/17x255/off/patch"],
    "hm_own": ["hl_measure/35x520/grid/patch", "hl_measure/35x520/grid/flatsat", "hl_measure/35x520/grid/flatlow"],
    "hm_neighbour": ["hl_measure/35x520/grid/patch"],
    "ss_full": ["stats/34x264/grid/noise/bins=64/roi=0", "stats/35x520/off/noise/bins=64/roi=0", "stats/35x520/grid/noise/bins=64/roi=1"],
    "ss_partial": ["stats/1x1/grid/noise/bins=64/roi=0", "stats/35x520/grid/noise/bins=64/roi=1"],
    "ss_empty": ["stats/1x1/grid/noise/bins=64/roi=0", "stats/35x520/grid/noise/bins=4096/roi=0"],
    "ss_onebin": ["stats/35x520/grid/flatlow/bins=4096/roi=0", "stats/35x520/grid/flatsat/bins=4096/roi=0", "stats/34x264/grid/flatlow/bins=64/roi=0"],
    "ss_prefetch": ["stats/35x520/grid/noise/bins=4096/roi=0", "stats/35x520/grid/flatlow/bins=4096/roi=0"],
    "ss_ld_edge": ["stats/1x1/grid/noise/bins=64/roi=0", "stats/35x520/grid/noise/bins=64/roi=1", "stats/31x257/off/noise/bins=64/roi=0"],
    "ss_row_out": ["stats/1x1/grid/noise/bins=64/roi=0", "stats/35x520/grid/noise/bins=64/roi=1"],
    "mg_short": ["merge/1x1/grid/noise/count=7/first=0/perlut=0/pos=none/support=0/window=0"],
    "mg_launch": ["merge/1x1/grid/noise/count=7/first=0/perlut=0/pos=none/support=0/window=0"],
    "mg_zero": ["merge/1x1/grid/noise/count=7/first=0/perlut=0/pos=none/support=0/window=0",
                "merge/35x520/grid/noise/count=5/first=1/perlut=0/pos=big/support=1/window=1"],
    "mg_cut": ["merge/35x520/grid/noise/count=5/first=1/perlut=0/pos=big/support=0/window=1",
               "merge/35x520/grid/noise/count=7/first=0/perlut=0/pos=even/support=1/window=1"],
    "mg_self": ["merge/1x1/grid/noise/count=7/first=0/perlut=0/pos=none/support=0/window=0",
                "merge_cells/35x520/grid/noise/count=7/first=0/perlut=0/pos=cells/support=0/window=2"],
    "mg_zerow": ["merge/35x520/grid/noise/count=5/first=1/perlut=0/pos=big/support=0/window=1",
                 "merge/35x520/off/noise/count=5/first=1/perlut=0/pos=big/support=1/window=1",
                 "merge_cells/35x520/grid/noise/count=7/first=0/perlut=0/pos=cells/support=0/window=2"],
    "mg_staged": ["merge/35x520/grid/noise/count=5/first=1/perlut=0/pos=big/support=0/window=1",
                  "merge_cells/35x520/pitch/noise/count=7/first=0/perlut=0/pos=cells/support=0/window=2"],
    "mg_m_aligned": ["merge/35x520/grid/noise/count=7/first=0/perlut=1/pos=m8/support=0/window=2",
                     "merge_cells/35x520/grid/noise/count=7/first=0/perlut=0/pos=cells/support=0/window=2"],
    "mg_m_sx": ["merge/35x520/grid/noise/count=7/first=0/perlut=0/pos=even/support=1/window=1",
                "merge/35x520/grid/noise/count=5/first=1/perlut=0/pos=big/support=0/window=1",
                "merge_cells/35x520/grid/noise/count=7/first=0/perlut=0/pos=cells/support=0/window=2"],
    "mg_m_invec": ["merge/35x520/off/noise/count=7/first=0/perlut=1/pos=m8/support=1/window=2",
                   "merge/35x520/pitch/noise/count=7/first=0/perlut=0/pos=even/support=1/window=1"],
    "div_calls": ["denoise/1x1/grid/noise/amount=256/perlut=1/radius=1", "denoise/35x520/pitch/noise/amount=77/perlut=1/radius=2"],
}


# ---------------------------------------------------------------------------------------------------------------- views
def view_geom(S):
    """(offset, pitch, frame stride) of the setting's input and output buffers, in samples from a 16-byte boundary."""
    H, W = S["H"], S["W"]
    pitch = W + 3 if S["view"] == "pitch" else (W + 7) // 8 * 8
    return (1 if S["view"] == "off" else 0), pitch, H * pitch


def on_grid(S):
    """MosaicBatch::on_grid() for what Context._strided makes of the view: a frame of one row has the pitch W."""
    off, pitch, fstride = view_geom(S)
    pitch = pitch if S["H"] > 1 else S["W"]
    return off % 8 == 0 and pitch % 8 == 0 and fstride % 8 == 0


# ---------------------------------------------------------------------------------------------------------------- contents
@functools.lru_cache(maxsize=None)
def images(name):
    """(FRAMES, H, W) uint16 of a setting."""
    S = SETTINGS[name]
    H, W, content = S["H"], S["W"], S["content"]
    rng = np.random.default_rng(20261021 + S["seed"])
    shape = (FRAMES, H, W)
    if S["family"] in ("merge", "merge_cells"):  # a scene, and noise per frame that the table's cut-offs spread over all weights
        scene = 800 + 60 * rng.standard_normal((1, H, W))
        return np.clip(np.rint(scene + 20 * rng.standard_normal((MG_FRAMES, H, W))), 0, 65535).astype(np.uint16)
    if S["family"] == "denoise":  # differences that the table's cut-offs spread over all weights
        return np.clip(np.rint((60000 if content == "bright" else 800) + 20 * rng.standard_normal(shape)), 0, 65535).astype(np.uint16)
    if content == "noise":
        return rng.integers(0, 4096, shape, dtype=np.uint16)
    if content == "flat":
        return np.full(shape, 1000, np.uint16)
    if content == "flatlow":
        return np.full(shape, 1000, np.uint16)
    if content == "flatsat":
        return np.full(shape, 4095, np.uint16)
    if content == "planted":  # noise well below the thresholds, with hot and cold pixels: many candidates, few of them flagged
        a = np.clip(np.rint(1000 + 8 * rng.standard_normal(shape)), 0, 65535).astype(np.uint16)
        k = max(1, H * W // 40)
        for f in range(FRAMES):
            ys, xs = planted_at(name)
            a[f, ys[0::2], xs[0::2]] = 4000 + f
            a[f, ys[1::2], xs[1::2]] = 0
            extra = rng.integers(0, H * W, k)  # and some of the frame's own
            a[f].reshape(-1)[extra] = rng.integers(0, 4096, k, dtype=np.uint16)
        return a
    if content == "patch":  # noise below the clip levels, a blown patch, and a patch clipped in one colour only
        a = rng.integers(200, 3800, shape, dtype=np.uint16)
        a[:, H // 4:H // 2 + 1, W // 4:W // 2 + 1] = 4095
        ys, xs = np.meshgrid(np.arange(H // 2, H), np.arange(W // 2, W), indexing="ij")
        red = ((ys & 1) == 0) & ((xs & 1) == 0)
        a[:, ys[red], xs[red]] = 4095
        if H * W >= 64:  # isolated clipped samples among unclipped ones
            k = H * W // 50
            a.reshape(FRAMES, -1)[:, rng.integers(0, H * W, k)] = 4050
        return a
    raise KeyError(content)


@functools.lru_cache(maxsize=None)
def planted_at(name):
    S = SETTINGS[name]
    H, W = S["H"], S["W"]
    rng = np.random.default_rng(977 + S["seed"])
    k = max(2, H * W // 50)
    at = rng.choice(H * W, size=min(k, H * W), replace=False)
    return at // W, at % W


@functools.lru_cache(maxsize=None)
def fix_list(name):
    """The static list of a `planted` setting, packed y << 16 | x and ascending: half of the planted pixels, some others, pairs
    of neighbours (so that pairs lose their eligibility) and one entry outside the frame."""
    S = SETTINGS[name]
    if not S.get("list"):
        return None
    H, W = S["H"], S["W"]
    rng = np.random.default_rng(31 + S["seed"])
    ys, xs = planted_at(name)
    keys = [(int(y) << 16) | int(x) for y, x in zip(ys[::2], xs[::2])]
    for _ in range(max(1, H * W // 200)):
        y, x = int(rng.integers(0, H)), int(rng.integers(0, W))
        keys += [(y << 16) | x, (y << 16) | min(x + 2, W - 1), (min(y + 2, H - 1) << 16) | x]
    keys.append((H << 16) | 0)
    return np.unique(np.array(keys, np.uint32))


@functools.lru_cache(maxsize=None)
def denoise_lut(name):
    S = SETTINGS[name]
    rng = np.random.default_rng(555 + S["seed"])
    return rng.integers(64, 400, ((FRAMES, 4, DN_L) if S["perlut"] else (4, DN_L)), dtype=np.uint16)


@functools.lru_cache(maxsize=None)
def shade_map(name):
    S = SETTINGS[name]
    rng = np.random.default_rng(333 + S["seed"])
    return rng.integers(2048, 12288, ((FRAMES, 4, 3, 5) if S["permap"] else (4, 3, 5)), dtype=np.uint16)


@functools.lru_cache(maxsize=None)
def hl_records(name):
    """(sum, cnt) per frame that an hl_apply setting with rec=1 is given: what the statement measures on its own images."""
    return HR.measure(images(name), HL_SAT, HL_BLACK, HL_GAIN, HR.CFA[HL_CFA], HL_LO)


# ---------------------------------------------------------------------------------------------------------------- staging
def nframes(S):
    return MG_FRAMES if S["family"] in ("merge", "merge_cells") else FRAMES


@functools.lru_cache(maxsize=None)
def merge_pos(name):
    """The positions of a merge setting: None, (n, 2) int16 as (y, x), or for merge_cells the field (n, Cy, Cx, 2)."""
    S = SETTINGS[name]
    rng = np.random.default_rng(4242 + S["seed"])
    kind = S["pos"]
    if kind == "none":
        return None
    if kind == "m8":
        return (8 * rng.integers(-3, 4, (MG_FRAMES, 2))).astype(np.int16)
    if kind == "even":  # odd positions among them: the low bit of a difference is dropped
        return rng.integers(-9, 10, (MG_FRAMES, 2)).astype(np.int16)
    if kind == "big":   # 150 columns and 20 rows a frame: a window of 2 reaches 300 columns and 40 rows
        return np.stack([20 * np.arange(MG_FRAMES), 150 * np.arange(MG_FRAMES)], axis=1).astype(np.int16)
    cy, cx = (S["H"] + MG_CELL[0] - 1) // MG_CELL[0], (S["W"] + MG_CELL[1] - 1) // MG_CELL[1]
    f = rng.integers(-9, 10, (MG_FRAMES, cy, cx, 2))
    f[:, -1, -1, 1] += 600 * np.arange(MG_FRAMES)  # the last cell moves out of the frame: its tiles pass every member over
    f[:, 0, 0, :] = 8 * rng.integers(-2, 3, (MG_FRAMES, 2))
    return f.astype(np.int16)


@functools.lru_cache(maxsize=None)
def merge_lut(name):
    S = SETTINGS[name]
    rng = np.random.default_rng(777 + S["seed"])
    return rng.integers(64, 400, ((MG_FRAMES, 4, DN_L) if S["perlut"] else (4, DN_L)), dtype=np.uint16)


def fix_halo(h, n):
    h = np.where(h < 0, np.where(h + 4 < n, h + 4, h + 2), np.where(h >= n, np.where(h - 4 >= 0, h - 4, h - 2), h))
    return np.clip(h, 0, n - 1)


def dn_halo(h, n):
    out = np.where(h < -2, np.where(h + 8 < n, h + 8, h + 4),
                   np.where(h < 0, np.where(h + 4 < n, h + 4, h + 2),
                            np.where(h >= n + 2, np.where(h - 8 >= 0, h - 8, h - 4),
                                     np.where(h >= n, np.where(h - 4 >= 0, h - 4, h - 2), h))))
    return np.clip(out, 0, n - 1)


def hl_halo(h, n):
    h = np.where(h < 0, -h, h)
    h = np.where(h >= n, 2 * n - 2 - h, h)
    return np.clip(h, 0, n - 1)


def dn_swap(c, n):
    c = np.asarray(c, np.int64)
    return ((c & ~1) == 2).astype(np.int64) | (2 * ((c + 4 - n >= 0) & (c + 4 - n < 2)).astype(np.int64))


def stage_plan(H, W, x0, y0, TH, HALO, MAP):
    """What stage_tile does for the tile at (x0, y0), by LDS row r and LDS column k: rowskip (LH,), per chunk colskip / full /
    halo / crop (TILE_CH,), and per column: the frame column it holds (srcx), `zero` (an element the chunk fills with 0)."""
    LH = TH + 2 * HALO
    yy = y0 - HALO + np.arange(LH)
    rowskip = yy >= H + HALO
    q = np.arange(TILE_CH)
    xs = x0 - 8 + 8 * q
    colskip = xs >= W + HALO
    inner = (q != 0) & (q != TILE_CH - 1)
    full = inner & (xs + 8 <= W)
    k = np.arange(TILE_LW)
    e, xc, qk = k % 8, x0 - 8 + k, k // 8
    e0 = np.where(qk == 0, 8 - HALO, 0)
    e1 = np.where(qk == TILE_CH - 1, HALO, 8)
    valid = full[qk] | ((e >= e0) & (e < e1) & (xc < W + HALO))
    srcx = np.where(full[qk], np.clip(xc, 0, W - 1), MAP(xc, W))
    return dict(LH=LH, rowskip=rowskip, colskip=colskip, full=full, halo=~inner, crop=inner & ~full, srcy=MAP(yy, H),
                srcx=srcx, zero=~valid, colskip_k=colskip[qk])


def stage(img, P, poison):
    """(lds (LH, TILE_LW) int64, known (LH, TILE_LW) bool) after staging one frame's tile by plan P."""
    lds = img[P["srcy"][:, None], P["srcx"][None, :]].astype(np.int64)
    lds[:, P["zero"]] = 0
    left = P["rowskip"][:, None] | P["colskip_k"][None, :]
    lds[left] = POISON
    known = np.ones(lds.shape, bool) if poison else ~left
    return lds, known


def stage_counts(c, P, vec, frames):
    staged = (~P["rowskip"]).sum()
    cols = ~P["colskip"]
    nfull = int((P["full"] & cols).sum())
    c["stg_vec" if vec else "stg_unal"] += frames * staged * nfull
    c["stg_halo"] += frames * staged * int((P["halo"] & cols).sum())
    c["stg_crop"] += frames * staged * int((P["crop"] & cols).sum())
    c["stg_skip"] += frames * (P["LH"] * TILE_CH - staged * int(cols.sum()))


def lanes_of(W, x0):
    """n of the tile's 32 lanes."""
    return np.clip(W - (x0 + 8 * np.arange(32)), 0, 8)


def store_counts(c, n, rows, vec, frames, what="st"):
    """`rows` rows of the lanes with n columns each."""
    whole = int((n == 8).sum())
    c[what + ("_vec" if vec else "_unal")] += frames * rows * whole
    c[what + "_elem"] += frames * rows * int(((n > 0) & (n < 8)).sum())


def tile_heights(variant):
    th = 16 if variant == "th16" else 32
    return {"fixpix": th, "denoise": th, "hl_apply": 32, "hl_measure": 32}


# ---------------------------------------------------------------------------------------------------------------- the model
def model(name, variant="census"):
    assert variant in VARIANTS + EXTRA_VARIANTS
    S = SETTINGS[name]
    c = dict.fromkeys(PATHS, 0)
    c["_unstaged"] = {}
    c["_unstaged_rows"] = 0
    {"merge": _merge, "merge_cells": _merge, "stats": _stats, "shade": _shade, "hl_clip": _hl_clip, "fixpix": _fixpix, "denoise": _denoise, "hl_apply": _hl_apply, "hl_measure": _hl_measure}[S["family"]](
        c, S, variant)
    for k in PATHS:
        c[k] = int(c[k])
    return c


def _direct(c, S, TH, loads):
    """kshade and khl_clip: tiles of TILE_W x TH (16), every lane two rows 8 apart, load8 and store8."""
    H, W = S["H"], S["W"]
    vec = on_grid(S)
    for y0 in range(0, H, TH):
        for x0 in range(0, W, TILE_W):
            c["wg"] += FRAMES
            n = lanes_of(W, x0)
            inside = int((n > 0).sum())
            c["idle_lane"] += FRAMES * 8 * (32 - inside)
            rows = min(TH, H - y0)
            c["row_cont"] += FRAMES * (TH - rows) * inside
            store_counts(c, n, rows, vec, FRAMES)
            if loads:
                store_counts(c, n, rows, vec, FRAMES, "ld")


def _shade(c, S, variant):
    _direct(c, S, 16, True)


def _hl_clip(c, S, variant):
    _direct(c, S, 16, True)


def stats_roi(S):
    """(y0, x0, h, w) of the setting's window."""
    H, W = S["H"], S["W"]
    return (3, 5, H - 7, W - 9) if S["roi"] else (0, 0, H, W)


def stats_plan(S, variant="census"):
    """The host side of mcraw_stats_batch: the tile grid's origin, its tiles, tiles per workgroup and workgroups per frame."""
    vec = on_grid(S)
    y0, x0, h, w = stats_roi(S)
    xa, ya = x0 & ~(7 if vec else 1), y0 & ~1
    tilesx = (x0 + w - xa + 255) // 256
    tiles = tilesx * ((y0 + h - ya + 15) // 16)
    # the plan takes the launch's frame count: 3 in one launch, 2 and 1 in the `frames2` build.  It is the only place where that
    # build's census could differ from `census`'s, and with the corpus' few tiles it does not: every launch gets the same tpc.
    tpcs = set()
    for nf in ((2, 1) if variant == "frames2" else (FRAMES,)):
        want = max(1, ST_WGS // nf)
        tpcs.add(min(2 if variant == "pieces" else ST_MAXTILES, max(max(1, S["bins"] // 64), (tiles + want - 1) // want)))
    assert len(tpcs) == 1
    tpc = tpcs.pop()
    return dict(vec=vec, xa=xa, ya=ya, tilesx=tilesx, tiles=tiles, tpc=tpc, wgs=(tiles + tpc - 1) // tpc)


def _stats(c, S, variant):
    P = stats_plan(S, variant)
    y0, x0, h, w = stats_roi(S)
    x1, y1 = x0 + w, y0 + h
    slow = variant in ("slow", "poisonslow")
    imgs, B, shift = images(S["name"]), S["bins"], ST_SHIFT[S["bins"]]
    c["wg"] += FRAMES * P["wgs"]
    c["ss_prefetch"] += FRAMES * (P["tiles"] - P["wgs"])  # every tile of a workgroup but its first
    for t in range(P["tiles"]):
        ty, tx = divmod(t, P["tilesx"])
        x = P["xa"] + tx * 256 + 8 * np.arange(32)
        lo, hi = np.clip(x0 - x, 0, 8), np.clip(x1 - x, 0, 8)
        some, whole = hi > lo, (lo == 0) & (hi == 8)
        y = P["ya"] + ty * 16 + np.arange(16)
        rin = (y >= y0) & (y < y1)
        nrows = int(rin.sum())
        c["ld_vec" if P["vec"] else "ld_unal"] += FRAMES * nrows * int(whole.sum())
        c["ss_ld_edge"] += FRAMES * nrows * int((some & ~whole).sum())
        c["ss_row_out"] += FRAMES * (16 * 32 - nrows * int(some.sum()))
        for wv in range(4):  # a wave: rows 4 wv .. 4 wv + 3 of the tile, all 32 lanes
            r = rin[4 * wv:4 * wv + 4]
            full = bool(whole.all() and r.all())
            if full and not slow:
                c["ss_full"] += FRAMES
                for a in (0, 1):
                    for par in (0, 1):  # the wave's 256 samples of position 2 a + par
                        v = imgs[:, y[4 * wv + a:4 * wv + 4:2]][:, :, x[0] + par:x[0] + 256:2].astype(np.int64)
                        b = np.minimum(v >> shift, B - 1).reshape(FRAMES, -1)
                        c["ss_onebin"] += int((b == b[:, :1]).all(axis=1).sum())
            elif some.any() and r.any():
                c["ss_partial"] += FRAMES
            else:
                c["ss_empty"] += FRAMES


def merge_plan(S, variant="census"):
    """The host side of mcraw_merge_batch: tile rows, tiles, and (first base, outputs, workgroups) of every launch."""
    H, W = S["H"], S["W"]
    TH = 16 if variant == "th16" else 32
    tilesx = (W + 255) // 256
    tiles = tilesx * ((H + TH - 1) // TH)
    piece = 3 if variant == "pieces" else max(1, min(65535, 0x40000000 // tiles))
    launches = []
    for j0 in range(0, S["count"], piece):
        nout = min(piece, S["count"] - j0)
        launches.append((S["first"] + j0, nout, 8 * ((tiles * nout + 7) // 8)))
    return dict(TH=TH, tilesx=tilesx, tiles=tiles, launches=launches)


def merge_shift(S, pos, t, b, y0, x0):
    """(sy, sx) of member t against base b for the tile at (y0, x0)."""
    if pos is None:
        return 0, 0
    p = pos.astype(np.int64)
    if S["family"] == "merge_cells":
        p = p[:, y0 // MG_CELL[0], x0 // MG_CELL[1]]
    return int(p[t, 0] - p[b, 0]) & ~1, int(p[t, 1] - p[b, 1]) & ~1


def _mg_stage(c, H, W, TH, y0, x0, sy, sx, aligned):
    """mg_stage's chunks: every one is written."""
    yy = y0 - 1 + np.arange(TH + 2) + sy
    q = np.arange(TILE_CH)
    xs = x0 - 8 + 8 * q + sx
    rows = int(((yy >= 0) & (yy < H)).sum())
    cols = (xs + 8 > 0) & (xs < W)
    inner = (q != 0) & (q != TILE_CH - 1)
    whole = (xs >= 0) & (xs + 8 <= W)
    c["stg_vec" if aligned else "stg_unal"] += rows * int((cols & inner & whole).sum())
    c["stg_halo"] += rows * int((cols & ~inner).sum())
    c["stg_crop"] += rows * int((cols & inner & ~whole).sum())
    c["mg_cut"] += rows * int((cols & inner & (xs < 0)).sum())
    c["mg_zero"] += (TH + 2) * TILE_CH - rows * int(cols.sum())


def _merge(c, S, variant):
    H, W, n = S["H"], S["W"], MG_FRAMES
    P = merge_plan(S, variant)
    TH, vec = P["TH"], on_grid(S)
    slow = variant in ("slow", "poisonslow")
    before, after = MG_WINDOWS[S["window"]]
    pos = merge_pos(S["name"])
    rpl = TH // 8
    for first, nout, wgs in P["launches"]:
        c["wg"] += wgs
        c["mg_launch"] += 1
        c["mg_short"] += wgs - P["tiles"] * nout
        for b in range(first, first + nout):
            for y0 in range(0, H, TH):
                for x0 in range(0, W, TILE_W):
                    _mg_stage(c, H, W, TH, y0, x0, 0, 0, vec)
                    for t in range(max(0, b - before), min(n - 1, b + after) + 1):
                        if t == b:
                            c["mg_self"] += 1
                            continue
                        sy, sx = merge_shift(S, pos, t, b, y0, x0)
                        ry0, ry1, rx0, rx1 = max(0, -sy), min(H, H - sy), max(0, -sx), min(W, W - sx)
                        if not slow and (ry0 >= ry1 or rx0 >= rx1 or ry1 <= y0 or ry0 >= y0 + TH or rx1 <= x0 or rx0 >= x0 + TILE_W):
                            c["mg_zerow"] += 1
                            continue
                        c["mg_staged"] += 1
                        c["mg_m_aligned" if vec and sx % 8 == 0 else "mg_m_sx" if vec else "mg_m_invec"] += 1
                        _mg_stage(c, H, W, TH, y0, x0, sy, sx, vec and sx % 8 == 0)
                    ln = lanes_of(W, x0)
                    inside = int((ln > 0).sum())
                    c["idle_lane"] += 8 * (32 - inside)
                    rows = min(TH, H - y0)
                    # lane (lx, ly) takes rows ly * rpl .. ly * rpl + rpl - 1 and leaves at the first one past H
                    c["row_break"] += inside * int((np.arange(8) * rpl + rpl - 1 >= H - y0).sum())
                    store_counts(c, ln, rows, vec, 1)
                    c["div_calls"] += 8 * rows * inside


def _tiles(c, S, TH, HALO, MAP):
    """The walk, the staging and the stores of a stencil stage; yields (x0, y0, plan, n of the lanes, rows of the tile inside)."""
    H, W = S["H"], S["W"]
    vec = on_grid(S)
    for y0 in range(0, H, TH):
        for x0 in range(0, W, TILE_W):
            c["wg"] += FRAMES
            P = stage_plan(H, W, x0, y0, TH, HALO, MAP)
            stage_counts(c, P, vec, FRAMES)
            n = lanes_of(W, x0)
            c["idle_lane"] += FRAMES * 8 * int((n == 0).sum())
            yield x0, y0, P, n, min(TH, H - y0)


def _lane_any(pix, TH):
    """(TH, 256) per pixel -> (TH, 32) per lane row: any of its 8 columns."""
    return pix.reshape(TH, 32, 8).any(axis=2)


def _range(c, key, lo, hi):
    c[key] += lo
    if hi != lo:
        a, b = c["_unstaged"].get(key, (0, 0))
        c["_unstaged"][key] = (a, b + hi - lo)


def _fixpix(c, S, variant):
    name = S["name"]
    H, W = S["H"], S["W"]
    TH = tile_heights(variant)["fixpix"]
    slow, poison = variant in ("slow", "poisonslow"), variant in ("poison", "poisonslow")
    imgs = images(name)
    lst = fix_list(name)
    for x0, y0, P, n, rows in _tiles(c, S, TH, 2, fix_halo):
        inside = n > 0
        c["row_cont"] += FRAMES * (TH - rows) * int(inside.sum())
        store_counts(c, n, rows, on_grid(S), FRAMES)
        active = (np.arange(TH) < rows)[:, None] & inside[None, :]  # (TH, 32) lane rows that run
        for f in range(FRAMES):
            lds, known = stage(imgs[f], P, poison)
            v = lds[2:2 + TH, 8:264]
            nb = [lds[2 + dy:2 + dy + TH, 8 + dx:264 + dx] for dy, dx in FX.NEIGHBOURS]
            kn = known[2:2 + TH, 8:264].copy()
            for dy, dx in FX.NEIGHBOURS:
                kn &= known[2 + dy:2 + dy + TH, 8 + dx:264 + dx]
            Hk, Lk = FX.rank_values(nb, S["rank"])
            candpix = (v > Hk) | (v < Lk)
            if slow:
                sure, maybe = active.copy(), np.zeros_like(active)
            else:
                sure = _lane_any(candpix & kn, TH) & active
                maybe = _lane_any(~kn, TH) & active & ~sure
            c["_unstaged_rows"] += int(maybe.sum())
            _range(c, "fp_cand", int(sure.sum()), int(sure.sum() + maybe.sum()))
            # a wave: the 32 lanes of tile rows 2j and 2j + 1
            wact = active.reshape(TH // 2, 64).any(axis=1)
            wsure = sure.reshape(TH // 2, 64).any(axis=1)
            wmaybe = maybe.reshape(TH // 2, 64).any(axis=1) & ~wsure
            _range(c, "fp_wave_any", int(wsure.sum()), int(wsure.sum() + wmaybe.sum()))
            c["fp_wave_none"] += int(wact.sum() - wsure.sum())
            if wmaybe.any():
                a, b = c["_unstaged"].get("fp_wave_none", (0, 0))
                c["_unstaged"]["fp_wave_none"] = (a - int(wmaybe.sum()), b)
    flags = FX.HOT | FX.COLD
    for f in range(FRAMES):
        _, hot, cold = FX.dynamic(imgs[f], flags, S["rank"], int(np.rint(FP_REL * 256)), FP_BLACK, FP_ABS)
        c["fp_hot"] += int(hot.sum())
        c["fp_cold"] += int(cold.sum())
        fl = hot | cold
        if S["counts"] and lst is not None:
            fy, fx = np.nonzero(fl)
            c["fp_listed"] += int(FX.member(lst, (fy.astype(np.int64) << 16) | fx).sum())
        pad = np.zeros((H, (W + 1) // 2 * 2), bool)
        pad[:, :W] = fl
        c["fp_flag"] += int(pad.reshape(H, -1, 2).any(axis=2).sum())
    if lst is not None:
        ly, lx = (lst >> 16).astype(np.int64), (lst & 0xFFFF).astype(np.int64)
        keep = (lx < W) & (ly < H)
        ly, lx = ly[keep], lx[keep]
        ny = np.stack([FX.neighbour(ly, dy, H) if dy else ly for dy, _ in FX.NEIGHBOURS])
        nx = np.stack([FX.neighbour(lx, dx, W) if dx else lx for _, dx in FX.NEIGHBOURS])
        free = ~FX.member(lst, (ny << 16) | nx)
        ok = np.stack([free[a] & free[b] for a, b in FX.PAIRS]).any(axis=0)
        wgs = (len(lst) + 255) // 256
        c["fl_wg"] += FRAMES * wgs
        c["fl_past"] += FRAMES * (wgs * 256 - len(lst))
        c["fl_outside"] += FRAMES * int((~keep).sum())
        c["fl_written"] += FRAMES * int(ok.sum())
        c["fl_nopair"] += FRAMES * int((~ok).sum())


def _denoise(c, S, variant):
    H, W, R = S["H"], S["W"], S["radius"]
    TH = tile_heights(variant)["denoise"]
    for x0, y0, P, n, rows in _tiles(c, S, TH, 2 * R, dn_halo):
        inside = int((n > 0).sum())
        # a lane (lx, ly) takes rows ly, ly + 8, .. and leaves at the first one past H: those whose last row is
        c["row_break"] += FRAMES * inside * int((np.arange(8) + TH - 8 >= H - y0).sum())
        store_counts(c, n, rows, on_grid(S), FRAMES)
        c["div_calls"] += FRAMES * 8 * rows * inside
        if R == 2:
            x = x0 + 8 * np.arange(32)
            sw = dn_swap(x[:, None] + np.arange(8)[None, :], W)  # (32, 8): all 8 columns, whatever n is
            run = n > 0
            c["dn_edgex"] += FRAMES * 8 * int(((sw != 0).any(axis=1) & run).sum())
            c["dn_both"] += FRAMES * 8 * int(((sw == 3).reshape(32, 4, 2).any(axis=2) & run[:, None]).sum())
            sy = dn_swap(y0 + np.arange(rows), H)
            c["dn_sy1"] += FRAMES * inside * int(((sy & 1) != 0).sum())
            c["dn_sy2"] += FRAMES * inside * int(((sy & 2) != 0).sum())
            c["dn_sy3"] += FRAMES * inside * int((sy == 3).sum())


def _hl_common(c, S, TH):
    for x0, y0, P, n, rows in _tiles(c, S, TH, 1, hl_halo):
        inside = n > 0
        c["row_cont"] += FRAMES * (TH - rows) * int(inside.sum())
        yield x0, y0, P, n, rows, (np.arange(TH) < rows)[:, None] & inside[None, :]


def _hl_apply(c, S, variant):
    name = S["name"]
    H, W = S["H"], S["W"]
    slow, poison = variant in ("slow", "poisonslow"), variant in ("poison", "poisonslow")
    imgs = images(name)
    satm = HR.by_position(HL_SAT, 32, 256)  # (the tile starts on an even row and column)
    for x0, y0, P, n, rows, active in _hl_common(c, S, 32):
        store_counts(c, n, rows, on_grid(S), FRAMES)
        for f in range(FRAMES):
            lds, known = stage(imgs[f], P, poison)
            own, kn = lds[1:33, 8:264], known[1:33, 8:264]
            pix = own >= satm
            if slow:
                sure, maybe = active.copy(), np.zeros_like(active)
            else:
                sure = _lane_any(pix & kn, 32) & active
                maybe = _lane_any(~kn, 32) & active & ~sure
            c["_unstaged_rows"] += int(maybe.sum())
            _range(c, "hl_clipped", int(sure.sum()), int(sure.sum() + maybe.sum()))
            c["hl_unclipped"] += int(active.sum() - sure.sum())
            if maybe.any():
                a, b = c["_unstaged"].get("hl_unclipped", (0, 0))
                c["_unstaged"]["hl_unclipped"] = (a - int(maybe.sum()), b)
    # the pixels: every clipped one of the frame enters the slow path
    s = imgs.astype(np.int64)
    v = HR.wb(imgs, HL_BLACK, HL_GAIN)
    ch = np.zeros(s.shape, np.int64)
    if S["rec"]:
        cc = HR.chroma(*hl_records(name))
        for f in range(FRAMES):
            ch[f] = HR.by_position(cc[f], H, W)
    cand = HR.reference(v, HR.CFA[HL_CFA]) + ch
    clipped = s >= HR.by_position(HL_SAT, H, W)
    take = clipped & (cand > v)
    back = HR.by_position(HL_BLACK, H, W) + ((np.maximum(cand, 0) * HR.by_position(HR.inv(HL_GAIN), H, W) + 2048) >> 12)
    c["hl_rebuilt"] += int(take.sum())
    c["hl_left"] += int((clipped & ~take).sum())
    c["hl_top"] += int((take & (back > HL_TOP)).sum())


def _hl_measure(c, S, variant):
    imgs = images(S["name"])
    H, W = S["H"], S["W"]
    for _ in _hl_common(c, S, 32):
        pass
    s = imgs.astype(np.int64)
    below = s < HR.by_position(HL_SAT, H, W)
    own = (s >= HR.by_position(HL_LO, H, W)) & below
    ok = own.copy()
    for m in HR._nb(below).values():
        ok &= m
    c["hm_own"] += int((~own).sum())
    c["hm_neighbour"] += int((own & ~ok).sum())
    c["hm_measured"] += int(ok.sum())


# ---------------------------------------------------------------------------------------------------------------- the sweep
DIV_MAXDEN, DIV_MAXQ, DIV_MAXN = 6400, 65536, 1 << 30


def div_sweep_count(dens=range(1, DIV_MAXDEN + 1)):
    """How many (n, den) the sweep of div_round evaluates: for every den and every quotient k in 0 .. 65536 the five n =
    k * den + {-1, 0, 1, den // 2, den - 1} with 0 <= n < 2^30 and n // den <= 65536 (equal n count as often as they occur).
    n grows with k, so for each den and offset the k that pass are a run."""
    total = 0
    for den in dens:
        for o in (-1, 0, 1, den // 2, den - 1):
            k0 = -(o // den) if o < 0 else 0                     # k * den + o >= 0
            k1 = min(DIV_MAXQ, (DIV_MAXN - 1 - o) // den)         # k * den + o < 2^30
            k1 = min(k1, DIV_MAXQ - (o // den))                   # (k * den + o) // den = k + o // den <= 65536
            total += max(0, k1 - k0 + 1)
    return total


def div_sweep_count_plain(den):
    """The same for one den, by enumeration."""
    k = np.arange(DIV_MAXQ + 1, dtype=np.int64)
    n = np.stack([k * den + o for o in (-1, 0, 1, den // 2, den - 1)])
    return int(((n >= 0) & (n < DIV_MAXN) & (n // den <= DIV_MAXQ)).sum())
