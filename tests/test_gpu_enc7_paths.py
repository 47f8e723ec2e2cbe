"""GPU (-m gpu): every path of the type-7 encoder's two kernels, forced and counted, against the synthesiser and a model.

Which way a workgroup of k7e_payload or k7e_side goes (csrc/mcraw_encode7.hip) is decided by the frame's content and geometry --
loads at the right edge and below the frame, block classes, record classes, the 12-bit ref clamp, chunks of records -- and by
timing: whether the prefetched guess was the ticket, and what a look-back finds published.  A failed look-back, the frame that
comes back with MCRAW_E_DEVICE and the epoch's wrap never happen by themselves.  tests/test_gpu_encode.py compares bytes on
contents chosen for other reasons; here six builds of the same sources -- the product's code with the path census
(-DMCRAW_PATHSE), and five that also force or inject one thing each (build.ENC7_PATH_VARIANTS; every switch is valid for every
input, see the kernel source) -- encode the corpus of tests/_enc7_model.py in a child process each (tests/_enc7_paths_child.py:
all frames as one batch, reversed, every frame alone, big / 1 x 1 / big, rejected frames among good ones, all on one context,
and once in host memory).  The child compares every frame with synthlib.encode7 byte for byte and decodes it back; this module
compares each batch's census with what the model and the switch determine -- exact counts where content or the switch decides,
bounds where timing does:

  every one  all content-driven counters are the model's, per batch; live + idle workgroups = n * smax; hit + refetched = live;
             the look-backs add at least one word each and at most the segments in front; the bound check behind the look-back
             never hits; no look-back gives up or meets a failure (but `lost`)
  census     every content-driven counter that an input can reach is above zero somewhere
  refetch    refetched = live, hit = 0
  aggonly    words = the sum of nseg (nseg - 1) / 2 exactly; windows >= the sum over segments of ceil(seg / 64)
  slow       polls > 0
  wrap       five batches on one context, byte-exact (the child); the third runs at epoch 1
  lost       at odd epochs frame 0 (1024 x 1028, 65 segments) fails as the child checks, gave up + met a failure = nseg - 4 with
             one to four give-ups and nseg - 8 failures met at least (the build makes the segments from 8 on wait for segment 4's
             give-up, so that LB_FAIL is read as well as written), every other frame is byte-exact; at even epochs on the same workspace every frame is
             byte-exact and nothing gives up

Two things differ from a plain reading of the plan, both because the kernel has it so: refs_clamped is counted in k7e_payload,
where `rmn > 4095` is evaluated (k7e_side only sees the clamped ref); and in a launch that `lost` fails, the fewest words are
those of the frames that do not fail plus the two look-backs in front of the lost segment -- one that gives up may have added
none.

A child that ends by a signal, at its time limit or without its result stops every further child, of this module and of every other (tests/_paths_harness.py): the remaining variants fail at
once.  Nothing is tried twice.

Wall times on an MI355X, one run of the module (the six tests: 16.0 s).  Per variant: the child's own `seconds` (from its first line
to its result: 85 encode and 84 decode calls and their comparisons; 5 and 4 for `lost`, 5 and 5 for `wrap`) / the whole test (link
of the variant, start of the child with its imports, child, the model):
  census 0.56 / 2.99   refetch 0.42 / 2.51   aggonly 0.39 / 2.67   slow 0.43 / 2.67   lost 0.40 / 2.66   wrap 0.34 / 2.49
The child process is what the time limit is on; it is no slower than the test around it, 2.99 s at the most.  CHILD_TIMEOUT is
ten times that.  What timing decided in that run, summed over a child's batches: in `census` 150 guesses hit and 1341 were
fetched again, 9870 polls; `slow` polled 644034 times (64 x s_sleep 127 in front of every eighth segment's first word; no
look-back gave up); in each of the three failing launches of `lost` 4 look-backs gave up (segments 4..7, 4096 polls each) and 57
met LB_FAIL."""
import json
import os

import pytest

import _enc7_model as E
import _paths_harness as PH
from motioncam_decoder_amd import build as B

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD = os.path.join(ROOT, "tests", "_enc7_paths_child.py")
CHILD_TIMEOUT = 30  # seconds: ten times the slowest measured whole test (see above)



def _judge(variant, res, returncode):
    print(variant, "errors", res["nerrors"])
    for (name, _, _, _), c in zip(E.plan(variant), res["batches"]):
        print(variant, name, json.dumps({k: v for k, v in c.items() if v}))
    PH.no_errors("frames differ from the synthesiser")(variant, res, returncode)


def _child(variant, tmp_path_factory):
    """The census of `variant`'s child, which is run once whatever becomes of it (tests/_paths_harness.py)."""
    return PH.run_child(__name__, variant, CHILD, [variant], B.ENC7_PATH_VARIANTS[variant], "libmcraw_k7e_%s.so" % variant, CHILD_TIMEOUT,
                       tmp_path_factory, _judge)


def check(variant, res):
    plan = E.plan(variant)
    assert len(res["batches"]) == len(plan)
    total = dict.fromkeys(E.PATHS, 0)
    for (name, batch, _, lost), c in zip(plan, res["batches"]):
        for k, v in c.items():
            total[k] += v
        # ---- every variant and batch
        T = E.census(batch, lost=lost)
        for k in E.CONTENT:
            assert c[k] == T[k], (name, k, c[k], T[k])
        smax, _ = E.strides(batch)
        assert c["live"] + c["idle"] == len(batch) * smax, (name, c)
        assert c["hit"] + c["refetched"] == c["live"], (name, c)
        lo, hi = E.word_bounds(batch, lost=lost)
        assert lo <= c["words"] <= hi, (name, c["words"], lo, hi)
        assert c["never"] == 0, (name, c)
        if not lost:
            assert c["gave_up"] == 0 and c["met_fail"] == 0, (name, c)
        assert c["windows"] >= c["lookbacks"] - c["gave_up"], (name, c)
        # ---- what the variant is about
        nsegs = [E.geometry(f["w"], f["h"])["nseg"] for f in batch if not f["bad"]]
        if variant == "refetch":
            assert c["refetched"] == c["live"] and c["hit"] == 0, (name, c)
        elif variant == "aggonly":
            assert c["words"] == sum(n * (n - 1) // 2 for n in nsegs), (name, c["words"])
            assert c["windows"] >= E.windows_aggonly(batch), (name, c["windows"], E.windows_aggonly(batch))
        elif variant == "lost" and lost:
            assert batch[0]["name"] == "nat12 1024x1028" and nsegs[0] == 65
            assert c["gave_up"] + c["met_fail"] == nsegs[0] - 4 and c["gave_up"] >= 1, (name, c)
            # (segments 8.. start their look-back when segment 4 has given up: its LB_FAIL, or one behind it, is in their first window)
            assert c["met_fail"] >= nsegs[0] - 8 and c["gave_up"] <= 4, (name, c)
    if variant == "census":
        for k in E.CONTENT:
            assert (total[k] > 0) == (k not in E.UNREACHABLE + ("side_fail",)), (k, total[k])  # (a failed look-back: `lost` alone)
    elif variant == "aggonly":
        third = dict(E.batches())["seq big"]
        assert E.windows_aggonly(third) >= 129 + 65 + 1  # (the 130-segment frame reads second and third windows)
    elif variant == "slow":
        assert total["polls"] > 0, total
    elif variant == "wrap":
        assert len(plan) == 5 and B.ENC7_PATH_VARIANTS["wrap"][-1] == "-DMCRAW_EPOCH0E=0xFFFFFFFDu"  # epochs ..FE, ..FF, 1, 2, 3
    elif variant == "lost":
        assert [lost for _, _, _, lost in plan] == [True, False, True, False, True]
        assert total["side_fail"] > 0 and total["gave_up"] >= 3


@pytest.mark.parametrize("variant", list(B.ENC7_PATH_VARIANTS))
def test_k7e_paths(variant, tmp_path_factory):
    check(variant, _child(variant, tmp_path_factory))
