"""CPU model of the flat leaf query's Phase A and Phase B as gi_wf.hip wf_flat has them since round 8
(tests/cpp/xflat_phase_a_check.cpp), built from the product's host scene builder."""
import os
import shutil
import subprocess

import pytest

import oracle_util as U

CSRC = os.path.join(U.ROOT, "2019global_amd", "csrc")
SRCS = [os.path.join(U.ROOT, "tests", "cpp", "xflat_phase_a_check.cpp"), os.path.join(CSRC, "gi_build.cpp"),
        os.path.join(CSRC, "gi_bvh.cpp")]
FLAGS = ["-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I" + CSRC, "-I" + os.path.join(U.ROOT, "include")]


def _cornell(tmp_path):
    scn = tmp_path / "cornell.scn"
    scn.write_text(U.scenes().cornell_scene().to_scn())
    return str(scn)


def test_phase_a_model_equals_brute_force(tmp_path):
    """Hit bits shifted into the mask, the nearest candidate carried as a key (entry distance with the
    leaf index in its low five bits), the early exit on the second key's floor, the any hit's candidate
    taken from the mask: (t, primitive) and the any-hit boolean equal brute force on leaf tables of 1,
    4, 5, 31, 32 leaves and the Cornell box's 17, over random and axis-parallel rays, origins inside a
    box, rays whose two nearest entry distances are equal or within 32 ulp (both classes must occur on
    the Cornell box), rays leaving surfaces on both sides of the own-plane bound, and queries without a
    ray.  Zero mismatches."""
    exe = str(tmp_path / "xflat_a")
    subprocess.run(["g++", "-O2", *FLAGS, "-o", exe, *SRCS], check=True)
    out = subprocess.run([exe, "3000", _cornell(tmp_path)], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout
    assert "mismatches 0" in out.stdout.strip().splitlines()[-1], out.stdout
    assert all(f"scene {i}:" in out.stdout for i in range(6))


def test_phase_a_model_under_sanitizers(tmp_path):
    """The same stand-alone program (host code only) built with AddressSanitizer and
    UndefinedBehaviorSanitizer: no report, 0 mismatches."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = str(tmp_path / "xflat_a_san")
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", *FLAGS, "-o", exe, *SRCS], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe, "400", _cornell(tmp_path)], capture_output=True, text=True, env=env, timeout=600)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]
    assert "mismatches 0" in out.stdout.strip().splitlines()[-1]
