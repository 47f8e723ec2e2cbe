"""CPU: what mcraw_demosaic_area_batch decides about a call (csrc/mcraw_area_args.h: accept / reject / no-op, the plan of the
launch, the taps, the layout of the scratch) is plain C++ and needs neither a GPU nor HIP.  tests/cpp/area_args_check.cpp
includes that header alone and compares its decisions against a transcription of the contract."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "motioncam_decoder_amd", "csrc")


def test_area_args_without_hip(tmp_path):
    """Every rule one defect at a time, the staging modes, rgb_check's answer to algo 3, the taps of eight crop sizes, and 60 000
    seeded tuples of geometry, family and pointers; for every accepted call the plan's invariants (the tiles cover the output, every
    tap of every column lies in its LDS segment, the weights fit).  Host code only, under ASan and UBSan."""
    exe = str(tmp_path / "area_args_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "cpp", "area_args_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr.strip(), (r.stdout[-3000:], r.stderr[-3000:])
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "wrong 0", r.stdout[-3000:]
    assert int(re.match(r"cases (\d+)", lines[-2]).group(1)) >= 100000, lines[-2]
    acc, rej = (int(v) for v in re.match(r"accepted (\d+) rejected (\d+)", lines[-3]).groups())
    assert acc >= 1000 and rej >= 1000, lines[-3]  # (both decisions are exercised)
