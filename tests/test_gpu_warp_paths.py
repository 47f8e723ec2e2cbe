"""GPU (-m gpu): the persistent loop of krgb_warp (csrc/mcraw_warp.hip) forced, its LDS poisoned and every path of it counted, against
the numpy statement and an exact model.

The kinds with a LUT run a persistent grid: min(units x frames, what the device holds at once) workgroups, each walking
t = blockIdx.x, + gridDim.x, ...  The second and later trips of that loop -- the barrier at its top, the window, the map, the
colours and the output frame of another unit -- are all a real batch runs, and the machine, not the input, decides whether a
test reaches them: the shapes of test_gpu_warp.py stay below the grid.  Here the five builds of build.RGB_PATH_VARIANTS (the census,
-DMCRAW_PATHSR, alone; the grid capped at 1 and at 3 workgroups through the RGB_GRID_LIMIT hook of csrc/mcraw_rgb_launch.h, which
krgb_warp's unit takes from csrc/mcraw_rgb.hip; s_raw and s_e filled with a pattern in front of every unit, with the product's grid and
with one workgroup) run the corpus of tests/_gather_paths_model.py in a fresh child process each (tests/_gather_paths_child.py):
first the cases this module always ran -- 3 frames of 6 tiles each with per-frame maps and colours, the four kinds with a LUT,
every CFA, both filters, LUTs in LDS and in global memory --, then the input with its pitch off the 16-byte grid and with its base one sample
off, outputs one sample behind their grid, maps whose windows reach over each of the four frame edges, the 8 x 8
mosaic onto 2 x 2, a map that sends a dropped position above the window, 34 one-tile frames that RGB_MAXF splits into 32 + 2, and the float kinds (no loop:
under `census` and `poison` only).  With one workgroup every unit behind the first is a later trip, 17 of them in a case of 3
frames, 2 of which cross into another frame; with three a workgroup's successive units skip columns, rows and frames.

  every one        every output byte and guard byte equals the numpy statement (_warp_ref); census == model(case, variant), EVERY
                   counter, EXACTLY; the counters that no accepted call can reach (ARGUED_ZERO) are zero
  census           every counter is above zero in the cases DRIVEN names for it; the grid the census reports is 1 .. units x frames
  grid1, grid3     the grid is min(units x frames, N) per launch; every case with a LUT shows later units and frame crossings
  poison, poison1  bytes, and every count as in `census` / `grid1`

A child that ends by a signal, at its time limit or without its result stops every further child, of this module and of every other (tests/_paths_harness.py): the remaining variants fail at
once.  Nothing is tried twice.

Wall times on an MI355X (one run of the whole GPU suite; a child's own `seconds` from a run of the children alone): a child
0.26 .. 0.51 s for its 24 or 27 calls and their comparisons; a whole test, in seconds
(the link of the variant, whose six objects came with the build, the start of the child with its imports, the child, the models):
census 2.39, grid1 2.41, poison 2.34, poison1 2.58, grid3 below 2.26.
The parent commit's two tests of this module, run beside them, took less than 2.26 s each (they did not reach that run's 80 slowest).
CHILD_TIMEOUT guards against a hang, not against performance."""
import pytest

import _gather_paths_model as G
import _gather_paths_parent as GP
from motioncam_decoder_amd import build as B

pytestmark = pytest.mark.gpu
KERNEL = "warp"
CHILD_TIMEOUT = GP.CHILD_TIMEOUT  # 60 seconds: guards against a hang, not against performance


@pytest.fixture(scope="module")
def corpus_npz(tmp_path_factory):
    """Computed once for the module."""
    path = str(tmp_path_factory.mktemp("warp_paths") / "corpus.npz")
    assert GP.make_npz(path, KERNEL) == len(G.cases(KERNEL)) >= 16
    return path


@pytest.mark.parametrize("variant", list(B.RGB_PATH_VARIANTS))
def test_warp_persistent_loop(variant, corpus_npz, tmp_path_factory):
    main = list(G.cases(KERNEL).values())[:16]  # the cases this module always ran: at least 5 tiles x 3 frames, every one with a LUT
    assert all(G.plan(S)["units"] >= 5 and S["n"] >= 3 and not G.is_float(S) and S["in_align"] == 0 == S["out_off"] for S in main)
    GP.check(__name__, KERNEL, variant, GP.run_variant(__name__, KERNEL, variant, corpus_npz, tmp_path_factory))
