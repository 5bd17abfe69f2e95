"""The checker-texel filter on the CPU: 2019global_amd/csrc/gi_math.h tri_tex_class / tri_texel_fast -- the
functions the device's shading helper x_texel calls -- driven by tests/cpp/tex_class_check.cpp against the
exact code (tri_texcoord + texel) on the frames and point classes that program's header lists."""
import os
import re
import subprocess

import oracle_util as U

CSRC = os.path.join(U.ROOT, "2019global_amd", "csrc")
SRC = os.path.join(U.ROOT, "tests", "cpp", "tex_class_check.cpp")
FLAGS = ["-std=c++17", "-Wall", "-Wextra", "-pthread", "-ffp-contract=off", "-I" + CSRC, "-I" + os.path.join(U.ROOT, "include")]
FRAMES = ["red wall a", "red wall b", "green wall a", "back wall a", "short block top b", "tall block side a",
          "long thin", "tiny unit", "degenerate"]


def _check(out, min_points):
    lines = out.stdout.strip().splitlines()
    assert out.returncode == 0, out.stdout[-3000:]
    assert lines[-1] == "failures 0", out.stdout[-3000:]
    for name in FRAMES:
        m = [re.fullmatch(rf"frame {name}: points (\d+) answered (\d+) wrong 0", ln) for ln in lines]
        m = [x for x in m if x]
        assert len(m) == 1, (name, out.stdout[-3000:])
        assert int(m[0].group(1)) >= min_points, (name, m[0].group(0))
    share = re.search(r"wall fallback share ([0-9.]+) of (\d+) uniform points", out.stdout)
    return float(share.group(1)), int(share.group(2))


def test_tex_class_exact_and_decides(tmp_path):
    """At least 10 M points per frame (uniform, pattern boundaries -/+ 0..4 ulp for both coordinates, the
    p1 -> p2 edge and its extension, P == p1, far outside): the filter never gives another colour than the
    exact code.  On uniform points of the Cornell box's coloured walls it decides at least 99% (a filter
    that never answers would be exact and save nothing)."""
    exe = str(tmp_path / "tex_class")
    subprocess.run(["g++", "-O2", *FLAGS, "-o", exe, SRC], check=True)
    out = subprocess.run([exe, "4"], capture_output=True, text=True, timeout=600)
    print(out.stdout)
    share, n = _check(out, 10_000_000)
    assert n >= 10_000_000
    assert share <= 0.01, share


def test_tex_class_under_sanitizers(tmp_path):
    """The same stand-alone program (host code only) built with AddressSanitizer and
    UndefinedBehaviorSanitizer, a quarter of the points: no report, 0 failures."""
    exe = str(tmp_path / "tex_class_san")
    subprocess.run(["g++", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                    "-fno-omit-frame-pointer", *FLAGS, "-o", exe, SRC], check=True)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    out = subprocess.run([exe, "1"], capture_output=True, text=True, env=env, timeout=600)
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr, out.stderr[-2000:]
    _check(out, 2_000_000)
