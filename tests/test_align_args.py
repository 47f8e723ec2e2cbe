"""CPU: the geometry of mcraw_align_batch (csrc/mcraw_align_args.h: the pyramid's planes, the levels' bounds, the empty-window
rule, the layout of the scratch, the checks on pos / sad / work) is plain C++ and needs neither a GPU nor HIP.
tests/cpp/align_args_check.cpp includes that header alone and compares what the entry point decides with it against a
transcription of the contract."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "motioncam_decoder_amd", "csrc")


def test_align_args_without_hip(tmp_path):
    """Accept / reject for levels 0 .. 7, radius 0 .. 9 and sizes from 0 to 65537 (the empty-window rule at every level), the
    planes, bounds and sections of accepted plans, and one defect at a time in pos / sad / work (missing, misaligned, too small,
    inside the input, inside one another); 200 000 seeded tuples.  Host code only, under ASan and UBSan."""
    exe = str(tmp_path / "align_args_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + CSRC, "-o", exe, os.path.join(ROOT, "tests", "cpp", "align_args_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr.strip(), (r.stdout[-3000:], r.stderr[-3000:])
    lines = r.stdout.strip().splitlines()
    assert lines[-1] == "wrong 0", r.stdout[-3000:]
    assert int(re.match(r"cases (\d+)", lines[-2]).group(1)) >= 1000, lines[-2]
    acc, rej = (int(v) for v in re.match(r"accepted (\d+) rejected (\d+)", lines[-3]).groups())
    assert acc >= 1000 and rej >= 1000, lines[-3]  # (both decisions are exercised)
