"""GPU (-m gpu): the persistent loop of krgb_ha (csrc/mcraw_ha.hip) forced.

The kinds with a LUT run a persistent grid: min(units x frames, what the device holds at once) workgroups, each walking
t = blockIdx.x, + gridDim.x, ...  The second and later trips of that loop -- the barrier at its top, in front of a stage that
overwrites what the estimates of the trip before read, and the tile, the colours and the output frame of another unit -- are all a
real batch runs, and the machine, not the input, decides whether a test reaches them: the shapes of test_gpu_ha.py stay below the
grid.  Here the builds of build.RGB_PATH_VARIANTS with the grid capped at 1 and at 3 workgroups (the RGB_GRID_LIMIT hook of
csrc/mcraw_rgb_launch.h, which krgb_ha's unit takes from csrc/mcraw_rgb.hip: it names no switch of its own) run 3 frames of 6 tiles
each with per-frame colours in a fresh child process each (tests/_ha_paths_child.py): the four kinds with a LUT, every CFA, LUTs in
LDS and in global memory.  With one workgroup every unit behind the first is a later trip, 17 of them, 2 of which cross into
another frame; with three a workgroup's successive units skip columns, rows and frames.  The child compares every call's output
byte for byte with the numpy statement (_ha_ref), the guard bands around it included.

A child that ends by a signal, at its time limit or without its result stops every further child, of this module and of every other (tests/_paths_harness.py): the remaining variants fail at
once.  Nothing is tried twice."""
import json
import os

import numpy as np
import pytest

import _paths_harness as PH
import motioncam_decoder_amd as M
from motioncam_decoder_amd import build as B

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "_ha_paths_child.py")
CHILD_TIMEOUT = 60  # seconds: guards against a hang, not against performance (a child takes a few seconds)
VARIANTS = ("grid1", "grid3")
H, WD, N = 40, 520, 3  # 2 x 3 tiles: the last tile row 8 rows high, the last tile column 8 columns wide
WHITE, BLACK, IN_BITS = 3.5, (3, 1, 2, 3), 11


def make_npz(path):
    """The corpus: the images, the colours, the LUTs, the plan of the cases and the bytes the numpy statement gives."""
    import _display_ref as D
    import _ha_ref as HA
    import _yuv_ref as Y
    rng = np.random.default_rng(20261022)
    yy, xx = np.mgrid[0:H, 0:WD]
    # every way of both choices in every frame: 2-bit noise, with stripes both ways and 16-bit noise in bands of columns
    imgs = rng.integers(0, 4, (N, H, WD)).astype(np.uint16)
    imgs[:, :, 96:160] = rng.integers(0, 1 << 16, (N, H, 64))
    imgs[:, :, 224:288] = ((xx[:, 224:288] & 1) * 65535).astype(np.uint16)
    imgs[:, :, 400:464] = ((yy[:, 400:464] & 1) * 65535).astype(np.uint16)
    for i in range(N):
        gw, dw = HA.ways(imgs[i], BLACK, "rggb")
        assert min(gw) >= 8 and min(dw) >= 8
    gain = np.stack([np.array([1.5 + 0.1 * i, 1.0, 1.9 - 0.2 * i], np.float32) for i in range(N)])
    base = np.array([[1.7, -0.5, -0.2], [-0.25, 1.4, -0.15], [0.05, -0.45, 1.4]], np.float32)
    matrix = np.stack([base * np.float32(1.0 - 0.03 * i) for i in range(N)])
    arrays = {"imgs": imgs, "gain": gain, "matrix": matrix, "lut_4096": rng.integers(0, 65536, 4096, dtype=np.uint16),
              "lut_65536": rng.integers(0, 65536, 65536, dtype=np.uint16)}
    plan = []
    kinds = (("u8", "hwc"), ("u16", "chw"), ("nv12", None), ("p010", None))
    for c, cfa in enumerate(("rggb", "bggr", "grbg", "gbrg")):
        o = [HA.rgb_values(imgs[i], WHITE, BLACK, cfa, gain[i], matrix[i]) for i in range(N)]
        for k, (kind, layout) in enumerate(kinds):
            if (c + k) % 2:
                continue  # two kinds per CFA: every kind with two CFAs
            lutn = 65536 if (c + k) % 4 == 2 else 4096
            S = dict(name="%s_%s_%d" % (kind, cfa, lutn), kind=kind, layout=layout, cfa=cfa, lutn=lutn, white=WHITE, black=BLACK,
                     in_bits=IN_BITS, exp="exp_%d_%d" % (c, k))
            lut = arrays["lut_%d" % lutn]
            if layout is None:
                coef = M.yuv_matrix("bt709", "limited", Y.BITS[kind], IN_BITS)
                frames = [Y.yuv_from_o(v, lut, kind, coef, IN_BITS) for v in o]
            else:
                frames = [D.apply_lut(v, lut, kind) for v in o]
                if layout == "hwc":
                    frames = [f.transpose(1, 2, 0) for f in frames]
            arrays[S["exp"]] = np.stack([np.ascontiguousarray(f) for f in frames]).view(np.uint8).reshape(-1)
            plan.append(S)
    arrays["plan"] = np.array(json.dumps(plan))
    np.savez(path, **arrays)
    return len(plan)


@pytest.fixture(scope="module")
def corpus_npz(tmp_path_factory):
    """Computed once for the module."""
    path = str(tmp_path_factory.mktemp("ha_paths") / "corpus.npz")
    assert make_npz(path) == 8
    return path


@pytest.mark.parametrize("variant", VARIANTS)
def test_ha_persistent_loop(variant, corpus_npz, tmp_path_factory):
    assert (H + 31) // 32 * ((WD + 255) // 256) >= 6 and N >= 3  # at least 6 tiles x 3 frames
    PH.run_child(__name__, variant, CHILD, [corpus_npz], B.RGB_PATH_VARIANTS[variant], "libmcraw_hap_%s.so" % variant, CHILD_TIMEOUT, tmp_path_factory,
                 PH.no_errors("outputs differ from the numpy statement", lambda res: res["cases"] == 8))
