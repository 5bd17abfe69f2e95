"""CPU checks of the flat leaf table and the flat leaf query (tests/cpp/xflat_check.cpp), built from
the product's host scene builder."""
import os
import shutil
import subprocess

import pytest

import oracle_util as U

CSRC = os.path.join(U.ROOT, "2019global_amd", "csrc")
SRCS = [os.path.join(U.ROOT, "tests", "cpp", "xflat_check.cpp"), os.path.join(CSRC, "gi_build.cpp"),
        os.path.join(CSRC, "gi_bvh.cpp")]
FLAGS = ["-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I" + CSRC, "-I" + os.path.join(U.ROOT, "include")]


def _cornell(tmp_path):
    scn = tmp_path / "cornell.scn"
    scn.write_text(U.scenes().cornell_scene().to_scn())
    return str(scn)


def test_flat_leaf_table_and_query(tmp_path):
    """The table holds every leaf child of the wide tree once with the node's own box floats, offset,
    count and plane group, and the flat query (phase A over the table, phase B per ray; restated in
    the checker) returns brute force's closest hit (t, primitive) and any-hit answer: the Cornell box,
    soups of 1, GI_XFLAT_MAX and GI_XFLAT_MAX + 1 leaves (the last keeps the tree), tilted coplanar
    quads and scenes with spheres; random and axis-parallel rays and rays leaving hit points with the
    own-plane skip down to just above the scene's bound."""
    exe = str(tmp_path / "xflat")
    subprocess.run(["g++", "-O2", *FLAGS, "-o", exe, *SRCS], check=True)
    out = subprocess.run([exe, "4000", _cornell(tmp_path)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout
    assert "mismatches 0" in out.stdout.strip().splitlines()[-1], out.stdout
    assert "scene 6:" in out.stdout and "scene 2:" in out.stdout


def test_flat_leaf_checker_under_sanitizers(tmp_path):
    """The same program (host code only, stand-alone) built with AddressSanitizer +
    UndefinedBehaviorSanitizer: no report, 0 mismatches."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "xflat_san")
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", *FLAGS, "-o", exe, *SRCS], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe, "600", _cornell(tmp_path)], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]
    assert "mismatches 0" in out.stdout.strip().splitlines()[-1]
