"""GPU (-m gpu): the persistent loop of krgb_mesh (csrc/mcraw_mesh.hip) forced.

The kinds with a LUT run a persistent grid: min(units x frames, what the device holds at once) workgroups, each walking
t = blockIdx.x, + gridDim.x, ...  The second and later trips of that loop -- the barrier at its top, the cell's nodes, the window, the
colours and the output frame of another unit -- are all a real batch runs, and the machine, not the input, decides whether a
test reaches them: the shapes of test_gpu_mesh.py stay below the grid.  Here the builds of build.RGB_PATH_VARIANTS with the grid
capped at 1 and at 3 workgroups (the RGB_GRID_LIMIT hook of csrc/mcraw_rgb_launch.h, which krgb_mesh's unit takes from
csrc/mcraw_rgb.hip: it names no switch of its own) run 3 frames of 6 tiles each with per-frame meshes and colours in a fresh child
process each (tests/_mesh_paths_child.py): the four kinds with a LUT, every CFA, both filters, LUTs in LDS and in global memory.  With one
workgroup every unit behind the first is a later trip, 17 of them, 2 of which cross into another frame; with three a workgroup's
successive units skip columns, rows and frames.  The child compares every call's output byte for byte with the numpy statement
(_mesh_ref), the guard bands around it included.

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
CHILD = os.path.join(ROOT, "tests", "_mesh_paths_child.py")
CHILD_TIMEOUT = 60  # seconds: guards against a hang, not against performance (a child takes a few seconds)
VARIANTS = ("grid1", "grid3")
SIZE, H, WD, N = (40, 70), 72, 136, 3  # 2 x 3 tiles; the last lane of a row holds 6 of its 8 columns
WHITE, BLACK, IN_BITS = 4095.0, (60, 61, 62, 63), 11


def make_npz(path):
    """The corpus: the images, the meshes, the colours, the LUTs, the plan of the cases and the bytes the numpy statement gives.  The
    meshes: affine_mesh of an extreme map, a barrel, and one with a tile outside the regime and nodes outside the frame."""
    import _mesh_ref as MR
    import _warp_ref as W
    import _yuv_ref as Y
    rng = np.random.default_rng(20261021)
    imgs = rng.integers(0, 5000, (N, H, WD), dtype=np.uint16)  # from below the black levels to above white
    lin = (65536 - 11000, -14000, 14000, 65536 - 11000)
    m = [lin[0], lin[1], 0, lin[2], lin[3], 0]
    Yp, Xp = W.positions(m, SIZE)
    m[2], m[5] = -int(Yp.min()) + 300, -int(Xp.min()) + 500
    assert W.map_ok(m, SIZE, H, WD)
    hostile = MR.translation_mesh(SIZE, 4, 6)
    hostile[:, 1:, 1] += 256 * 88
    hostile[0, :, 0] -= 256 * 9
    meshes = np.stack([M.affine_mesh(m, SIZE)[0], M.distortion_mesh(H, WD, SIZE, radial=(1.0, -0.3, 0.05, 0.0)), hostile])
    assert MR.in_regime(meshes[0], SIZE, H, WD) and MR.in_regime(meshes[1], SIZE, H, WD) and not MR.in_regime(meshes[2], SIZE, H, WD)
    gain = np.stack([np.array([1.5 + 0.1 * i, 1.0, 1.9 - 0.2 * i], np.float32) for i in range(N)])
    base = np.array([[1.7, -0.5, -0.2], [-0.25, 1.4, -0.15], [0.05, -0.45, 1.4]], np.float32)
    matrix = np.stack([base * np.float32(1.0 - 0.03 * i) for i in range(N)])
    arrays = {"imgs": imgs, "meshes": meshes, "gain": gain, "matrix": matrix,
              "lut_4096": rng.integers(0, 65536, 4096, dtype=np.uint16), "lut_65536": rng.integers(0, 65536, 65536, dtype=np.uint16)}
    plan = []
    o_of = {}
    kinds = (("u8", "hwc"), ("u16", "chw"), ("nv12", None), ("p010", None))
    for c, cfa in enumerate(("rggb", "bggr", "grbg", "gbrg")):
        for k, (kind, layout) in enumerate(kinds):
            filt = "linear" if (c + k) % 4 == 3 else "cubic"
            lutn = 65536 if (c + k) % 4 == 1 else 4096
            S = dict(name="%s_%s_%s" % (kind, cfa, filt), kind=kind, layout=layout, cfa=cfa, filt=filt, lutn=lutn, size=SIZE, white=WHITE,
                     black=BLACK, in_bits=IN_BITS, exp="exp_%d_%d" % (c, k))
            if (cfa, filt) not in o_of:
                o_of[cfa, filt] = [MR.values(MR.mesh_estimates(imgs[i], meshes[i], SIZE, filt, BLACK, cfa), WHITE, BLACK, gain[i], matrix[i]) for i in range(N)]
            o = o_of[cfa, filt]
            lut = arrays["lut_%d" % lutn]
            if layout is None:
                coef = M.yuv_matrix("bt709", "limited", Y.BITS[kind], IN_BITS)
                frames = [MR.yuv_from_o(v, lut, kind, coef, IN_BITS) for v in o]
            else:
                frames = [MR.display_from_o(v, lut, kind, layout) for v in o]
            arrays[S["exp"]] = np.stack([np.ascontiguousarray(f) for f in frames]).view(np.uint8).reshape(-1)
            plan.append(S)
    arrays["plan"] = np.array(json.dumps(plan))
    np.savez(path, **arrays)
    return len(plan)


@pytest.fixture(scope="module")
def corpus_npz(tmp_path_factory):
    """Computed once for the module."""
    path = str(tmp_path_factory.mktemp("mesh_paths") / "corpus.npz")
    assert make_npz(path) == 16
    return path


@pytest.mark.parametrize("variant", VARIANTS)
def test_mesh_persistent_loop(variant, corpus_npz, tmp_path_factory):
    assert (SIZE[0] + 31) // 32 * ((SIZE[1] + 31) // 32) >= 5 and N >= 3  # at least 5 tiles x 3 frames
    PH.run_child(__name__, variant, CHILD, [corpus_npz], B.RGB_PATH_VARIANTS[variant], "libmcraw_meshp_%s.so" % variant, CHILD_TIMEOUT, tmp_path_factory,
                 PH.no_errors("outputs differ from the numpy statement", lambda res: res["cases"] == 16))
