"""CPU checks of the flat leaf query's packed Phase A (tests/cpp/xflat_pk_check.cpp): the two-stage form of the
plane distances equals child_hit's select form, and the device's leaf table is the host's, permuted."""
import os
import re
import subprocess

import pytest

import oracle_util as U
from x_scenes import placed_scene, soup

CSRC = os.path.join(U.ROOT, "2019global_amd", "csrc")
SRCS = [os.path.join(U.ROOT, "tests", "cpp", "xflat_pk_check.cpp"), os.path.join(CSRC, "gi_build.cpp"),
        os.path.join(CSRC, "gi_bvh.cpp")]
FLAGS = ["-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-pthread", "-I" + CSRC, "-I" + os.path.join(U.ROOT, "include")]
CLASSES = ("octants", "zero_dir", "zero_org", "on_plane", "large", "thin", "tiny")
CASES = 10_000_000


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("xflat_pk") / "xflat_pk_check")
    subprocess.run(["g++", "-O2", *FLAGS, "-o", exe, *SRCS], check=True)
    return exe


def test_two_stage_form_equals_select_form(checker):
    """10 M generated cases per class (all octants; one and two zero direction components of either sign; origin
    components +-0; origins on box planes; coordinates up to GI_X_COORD_MAX; boxes of 0 to 4 ulp; subnormals):
    near, far and max(near, 0) of every axis, tn, tf and the decision tn <= tf are equal between the two forms,
    +0 and -0 counting as equal.  The sign-of-zero differences are printed."""
    out = subprocess.run([checker, "identity", str(CASES)], capture_output=True, text=True, timeout=900)
    print(out.stdout)
    assert out.returncode == 0, out.stdout[-3000:]
    lines = out.stdout.strip().splitlines()
    for name in CLASSES:
        m = [re.match(r"%s\s+cases (\d+) mismatches (\d+) zero_sign (\d+)$" % name, ln) for ln in lines]
        m = [x for x in m if x]
        assert len(m) == 1 and int(m[0].group(1)) >= CASES and int(m[0].group(2)) == 0, (name, out.stdout[-3000:])
    m = re.match(r"cases (\d+) mismatches 0 zero_sign (\d+)$", lines[-1])
    assert m and int(m.group(1)) >= CASES * len(CLASSES), lines[-1]


def test_device_table_is_the_host_table_permuted(checker, tmp_path):
    """The Cornell box, soups of 1, 5 and 32 single-triangle leaves and the Cornell box scaled by 2^10 and moved
    by (8192, -4096, 2048): the table the upload copies is HostScene::xflat word for word in the device's order,
    and off, cnt, group and fan decode to the host's values."""
    S = U.scenes()
    cases = [("cornell", S.named_scene("cornell"), {}, 17)]
    for n in (1, 5, 32):
        sc, env = soup(n)
        cases.append(("soup%d" % n, sc, env, n))
    for p in ("x2^10", "off2^13"):
        sc, env = placed_scene("cornell", p)
        cases.append(("cornell_" + re.sub(r"\W", "_", p), sc, env, 17))
    for name, sc, env, leaves in cases:
        scn = tmp_path / (name + ".scn")
        scn.write_text(sc.to_scn())
        out = subprocess.run([checker, "table", str(scn)], capture_output=True, text=True, env=dict(os.environ, **env), timeout=300)
        assert out.returncode == 0, (name, out.stdout[-2000:])
        m = re.search(r": leaves (\d+) mismatches 0$", out.stdout.strip().splitlines()[-1])
        assert m and int(m.group(1)) == leaves, (name, out.stdout[-2000:])
