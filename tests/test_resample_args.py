"""CPU: what mcraw_demosaic_resample_batch decides about a call (csrc/mcraw_resample_args.h: accept / reject / no-op, the plan of
the launch, the taps, the layout of the scratch) is plain C++ and needs neither a GPU nor HIP.  tests/cpp/resample_args_check.cpp
includes that header (and the area one, for the siblings' answer to algo 4) and compares its decisions against a transcription of
the contract."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "motioncam_decoder_amd", "csrc")


@pytest.mark.parametrize("flags", (["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]),
                         ids=("plain", "asan_ubsan"))
def test_resample_args_without_hip(tmp_path, flags):
    """The taps of every legal (C, O) with C <= 96 and both filters against the contract (4096 in all, at most 5 / 9, the identity,
    the mirror, the reach), every rule one defect at a time, the scratch layout, rgb_check's and area_check's answer to algo 4, and
    4000 seeded tuples of geometry, family and pointers; for every accepted call the plan's invariants (the tiles cover the output,
    every tap of every column and row of every tile lies in the workgroup's LDS arrays).  A stand-alone host program, once plain and
    once under ASan and UBSan."""
    exe = str(tmp_path / "resample_args_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I" + CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "resample_args_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr.strip(), (r.stdout[-3000:], r.stderr[-3000:])
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "wrong 0", r.stdout[-3000:]
    assert int(re.match(r"cases (\d+)", lines[-2]).group(1)) >= 1000000, lines[-2]
    acc, rej = (int(v) for v in re.match(r"accepted (\d+) rejected (\d+)", lines[-3]).groups())
    assert acc >= 1000 and rej >= 1000, lines[-3]  # (both decisions are exercised)
    nl, nc, sl, sc = (int(v) for v in re.match(r"max taps (\d+) (\d+)  max sum \|w\| (\d+) (\d+)", lines[-4]).groups())
    assert nl <= 5 and nc <= 9 and sl == 4096 and 4096 < sc <= 5600, lines[-4]
