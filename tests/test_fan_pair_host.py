"""CPU checks of the fan-pair decision of the flat leaf query (csrc/gi_fan_pair.h, the very functions the
builder and gi_wf.hip wf_flat call; tests/cpp/xfan_pair_check.cpp) and of the builder's marking, built from
the product's host scene builder."""
import os
import re
import shutil
import subprocess

import pytest

import oracle_util as U
from x_scenes import coincident_quads, with_sphere

CSRC = os.path.join(U.ROOT, "2019global_amd", "csrc")
SRCS = [os.path.join(U.ROOT, "tests", "cpp", "xfan_pair_check.cpp"), os.path.join(CSRC, "gi_build.cpp"),
        os.path.join(CSRC, "gi_bvh.cpp")]
FLAGS = ["-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I" + CSRC, "-I" + os.path.join(U.ROOT, "include")]


def _scn(tmp_path, name, sc):
    p = tmp_path / (name + ".scn")
    p.write_text(sc.to_scn())
    return str(p)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("xfan") / "xfan")
    subprocess.run(["g++", "-O2", *FLAGS, "-o", out, *SRCS], check=True)
    return out


def _last(out):
    m = re.search(r"rays (\d+) undecided ([0-9.]+) random rays (\d+) undecided ([0-9.]+) mismatches (\d+)",
                  out.stdout.strip().splitlines()[-1])
    assert m, out.stdout[-2000:]
    return int(m.group(1)), float(m.group(2)), int(m.group(3)), float(m.group(4)), int(m.group(5))


def test_fan_pair_decision_equals_two_exact_tests(exe, tmp_path):
    """fan_pair_choice plus one exact test on the record it names (both where it is undecided) against two
    plain exact tests, (t of record 0, t of record 1) bit for bit: the Cornell box's 17 leaves as the
    builder marks them, rotated planar rectangles and convex quads, quads bent to just inside the builder's
    tolerance and near-slivers just inside its bound; the pairs the builder must refuse are each refused
    (the program fails otherwise).  Rays: random; at the diagonal and 0, 1, 2, 32 ulp off it per coordinate;
    corners and edges; |d . n| across the det margin and det = 0; origins in the plane; NaN directions.
    0 mismatches, and at least 99 % of the random rays decided (0.003 % undecided as measured here)."""
    out = subprocess.run([exe, "3000", _scn(tmp_path, "cornell", U.scenes().cornell_scene())], capture_output=True,
                         text=True, timeout=600)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-3000:]
    rays, share, rnd, rnd_share, bad = _last(out)
    print(f"undecided: {share:.6f} of {rays} rays, {rnd_share:.6f} of the {rnd} random rays")
    assert bad == 0
    assert rnd >= 17 * 3000 and rnd_share <= 0.01
    assert share > 0.0   # the diagonal and grazing classes do come out undecided


def test_fan_pair_check_under_sanitizers(tmp_path):
    """The same stand-alone program (host code only) built with AddressSanitizer and
    UndefinedBehaviorSanitizer: no report, 0 mismatches."""
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    san = str(tmp_path / "xfan_san")
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", *FLAGS, "-o", san, *SRCS], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([san, "300", _scn(tmp_path, "cornell", U.scenes().cornell_scene())], capture_output=True,
                         text=True, env=env, timeout=600)
    assert out.returncode == 0, (out.stdout[-2000:], out.stderr[-2000:])
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]
    assert _last(out)[4] == 0


def test_builder_marks_fan_pair_leaves(exe, tmp_path):
    """The builder's marking per scene: the Cornell box has 17 of 17 fan-pair leaves and the property; its
    mirror variant and the box with a sphere have the 17 and one sphere leaf (no property); the two
    coincident quads share one leaf of four records (none)."""
    S = U.scenes()
    cases = [("cornell", S.cornell_scene(), 17, 17, 1), ("cornell_mirror", S.named_scene("cornell_mirror"), 18, 17, 0),
             ("cornell_sphere", with_sphere()[0], 18, 17, 0), ("coincident_quads", coincident_quads()[0], 1, 0, 0)]
    out = subprocess.run([exe, "info", *[_scn(tmp_path, n, sc) for n, sc, *_ in cases]], capture_output=True, text=True,
                         timeout=600)
    assert out.returncode == 0, out.stdout[-2000:]
    got = re.findall(r"info \S+: leaves (\d+) fan (\d+) all (\d+) flat_ok 1", out.stdout)
    assert [tuple(map(int, g)) for g in got] == [c[2:] for c in cases], out.stdout
