"""CPU: what mcraw_demosaic_mesh_batch and mcraw_mesh_check decide about a call, the position arithmetic of a mesh cell and a tile's
window with its clamps (csrc/mcraw_mesh_args.h) are plain C++ and need neither a GPU nor HIP.  tests/cpp/mesh_args_check.cpp includes
that header and holds the kernel's index arithmetic, transcribed, against the LDS arrays and the frame for meshes of every kind."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "motioncam_decoder_amd", "csrc")


@pytest.mark.parametrize("flags", (["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]),
                         ids=("plain", "asan_ubsan"))
def test_mesh_args_without_hip(tmp_path, flags):
    """Every rule one defect at a time; over a sweep of frame and output sizes the meshes of the affine warp's 81 extreme linear
    parts in every corner of the frame and of seeded maps inside its bounds: every tile in the regime (reported), positions within
    1/256 sample of the affine warp's and equal under the identity; hostile meshes (full-range random int32 nodes, folds, constant
    nodes, the format's extremes, cells about the 32-bit form's limit): every staged row, every LDS index and every sample a tap
    reaches inside the arrays and within 4 samples of the frame, the tap clamp silent in the regime, the 32-bit interpolation equal
    to the 64-bit statement wherever the kernel uses it, and mcraw_mesh_check's verdict the sweep's.  A stand-alone host program,
    once plain and once under ASan and UBSan."""
    exe = str(tmp_path / "mesh_args_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I" + CSRC, "-o", exe,
                    os.path.join(ROOT, "tests", "cpp", "mesh_args_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and not r.stderr.strip(), (r.stdout[-3000:], r.stderr[-3000:])
    lines = r.stdout.strip().splitlines()
    print(r.stdout)
    assert lines[-1] == "wrong 0", r.stdout[-3000:]
    assert int(re.match(r"cases (\d+)", lines[-2]).group(1)) >= 10000, lines[-2]
    acc, rej = (int(v) for v in re.match(r"accepted (\d+) rejected (\d+)", lines[-3]).groups())
    assert acc >= 5 and rej >= 25, lines[-3]
    m = re.match(r"affine meshes: (\d+) at the bounds, (\d+) seeded, every tile in the regime: (\w+)", lines[0])
    assert m and int(m.group(1)) >= 324 and int(m.group(2)) >= 1500 and m.group(3) == "yes", lines[0]
    m = re.match(r"hostile meshes: (\d+) tiles outside the regime, (\d+) inside; (\d+) pixels through the 32-bit form, (\d+) through the 64-bit one", lines[1])
    assert m and min(int(v) for v in m.groups()) > 1000, lines[1]
