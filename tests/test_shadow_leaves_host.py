"""CPU check of the light-dead leaves of the flat leaf table (tests/cpp/xshadow_leaves_check.cpp),
built from the product's host scene builder and the launch's own mask function."""
import os
import re
import shutil
import subprocess

import pytest

import oracle_util as U

CSRC = os.path.join(U.ROOT, "2019global_amd", "csrc")
SRCS = [os.path.join(U.ROOT, "tests", "cpp", "xshadow_leaves_check.cpp"), os.path.join(CSRC, "gi_build.cpp"),
        os.path.join(CSRC, "gi_bvh.cpp")]
FLAGS = ["-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I" + CSRC, "-I" + os.path.join(U.ROOT, "include")]


def _scenes(tmp_path):
    out = []
    for name in ("cornell", "zoo"):
        p = tmp_path / (name + ".scn")
        p.write_text(U.scenes().named_scene(name).to_scn())
        out.append(str(p))
    return out


def test_dead_leaves_never_occlude(tmp_path):
    """Classification: the Cornell box under its own light has exactly the five walls and the two block
    bottoms dead; with the light above the ceiling the ceiling stays live; at 0.5 and 0.999 delta from the
    ceiling it is live, at 1.001 and 2 delta dead; a far camera, the `full` argument and a NaN light keep every
    leaf; the every-entity scene and the ground scenes mark a leaf only where the rule holds.  Rays: over more
    than a million shadow rays from computed hit points, weighted toward the edges of two walls, the corners
    and the blocks' contact with the floor, for lights down to 1.001 delta from one, two and three walls, no
    record of a dead leaf answers the exact test inside (MX_TMIN, ldist).  Zero mismatches."""
    exe = str(tmp_path / "xshadow")
    subprocess.run(["g++", "-O2", *FLAGS, "-o", exe, *SRCS], check=True)
    out = subprocess.run([exe, "60000", *_scenes(tmp_path)], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout
    last = out.stdout.strip().splitlines()[-1]
    m = re.match(r"rays (\d+) mismatches 0$", last)
    assert m and int(m.group(1)) >= 1_000_000, last
    share = re.search(r"within 1e-6 of two planes: ([0-9.]+) %", out.stdout)
    assert share and float(share.group(1)) >= 10.0   # the weighting toward the edges took


def test_dead_leaves_under_sanitizers(tmp_path):
    """The same stand-alone program (host code only) built with AddressSanitizer and
    UndefinedBehaviorSanitizer: no report, 0 mismatches."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "xshadow_san")
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", *FLAGS, "-o", exe, *SRCS], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe, "3000", *_scenes(tmp_path)], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]
    assert "mismatches 0" in out.stdout.strip().splitlines()[-1]
