"""CPU: Mode X scenes at other scales and away from the origin (x_scenes.placed, PLACEMENTS).

The placed ray sets meet, on the oracle alone, the conditions the device test
(tests/test_gpu_x_placed.py) relies on: the class conditions of test_x_query_oracle.py's
test_ray_sets_cover_their_classes, and the oracle's BVH equal to its brute force on every ray -- met by
the choice of inputs (x_scenes.FAR_MOVED_IN), never by leaving rays out.  The base sets are unchanged by
the generators' new frame argument (their hashes are pinned here).  The CPU restatements of the kernels'
traversal, flat query, fan pairs and light-dead leaves (tests/cpp/xaccel_check.cpp, xflat_check.cpp,
xflat_phase_a_check.cpp, xfan_pair_check.cpp, xshadow_leaves_check.cpp), built from the product's host
builder, run on the placed .scn files with rays drawn from the placed scene's own bounds: 0 mismatches at
every placement inside the fp32 box tests' limit (gi_scene.h GI_X_COORD_MAX), and the missed hits the
limit is there for one power of two beyond it."""
import hashlib
import os
import re
import subprocess

import numpy as np
import pytest

import oracle_util as U
import x_rays as R
from x_scenes import (FAR_MOVED_IN, INSIDE, PLACED_CASES, PLACEMENTS, QUERY_SCENES, X_COORD_MAX, placed, placed_scene,
                      placed_set, query_set)

S = U.scenes()
CSRC = os.path.join(U.ROOT, "2019global_amd", "csrc")
FLAGS = ["-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I" + CSRC, "-I" + os.path.join(U.ROOT, "include")]
BUILDER = [os.path.join(CSRC, "gi_build.cpp"), os.path.join(CSRC, "gi_bvh.cpp")]
CORNELL_FAMILY = ("cornell", "cornell_sphere", "grazing_tilted")   # (the shadow-share condition's scenes, as SHADOW_SCENES)

# sha256 (16 hex digits) of every base set's records, taken before the generators learnt of frames
BASE_SET_SHA = {
    "coincident": "e51f8e21d1e99853", "cornell": "8b94fd6056766d53", "cornell_mirror": "ba84c98d290ec1bf",
    "cornell_sphere": "3f5eee367bbb9383", "corner3_octree": "10b1f237d77f2f9d", "empty": "6ed2dcf3813d44d6",
    "grazing_floor": "48b758c12829f58e", "grazing_tilted": "1380c84b610b4087", "one_triangle": "ed0b96009b1c0570",
    "soup1000": "7c5808ede719abf4", "soup_max": "4f0d266a45faac0c", "soup_max_plus_1": "5090d7fe33e52487",
    "soup_xcnode": "06e1cb1bb640d004", "three_record_leaves": "ce07d9167b5cd345", "zoo": "35baff6feca6158c",
}


def test_placed_maps_every_point_and_refuses_other_kinds():
    base = S.cornell_scene()
    base.imp_sphere((4.0, 0.5, -1.0), 1.2, (0.8, 0.8, 0.3))
    s, off = 2.0 ** 10, np.array([8192.0, -4096.0, 2048.0])
    p = placed(base, s, off)
    assert p.name != base.name and p.focal == base.focal and len(p.entities) == len(base.entities)
    for a, b in ((p.cam_pos, base.cam_pos), (p.cam_look, base.cam_look), (p.light, base.light)):
        assert (np.array(a) == s * np.array(b) + off).all()
    for e, f in zip(p.entities, base.entities):
        assert e.kind == f.kind and e.material is f.material
        if e.kind == S.IMP_TRIANGLE:
            assert (np.array(e.args).reshape(3, 3) == s * np.array(f.args).reshape(3, 3) + off).all()
        else:
            assert (np.array(e.args[:3]) == s * np.array(f.args[:3]) + off).all()
            assert e.args[3] == s * f.args[3] and e.args[4:] == f.args[4:]
    # power-of-two scales and dyadic offsets keep the Cornell box exact: mapping back returns it
    back = placed(p, 1.0 / s, -off / s)
    assert [e.args for e in back.entities] == [e.args for e in base.entities]
    assert base.entities[0].args[0] == S.cornell_scene().entities[0].args[0]   # (the base is not modified)
    with pytest.raises(ValueError):
        placed(S.named_scene("zoo"), 2.0, (0.0, 0.0, 0.0))


def test_limit_placements_straddle_the_limit():
    """at_limit is the largest power-of-two scale at which the Cornell box's padded fp32 bounds stay within
    GI_X_COORD_MAX, beyond_limit the next; the limit itself is FLT_MAX / (1e30f (1 + 2^-23)) rounded down."""
    exact = float(np.finfo(np.float32).max) / (float(np.float32(1e30)) * (1.0 + 2.0 ** -23))
    assert 0.99 * exact <= X_COORD_MAX <= exact
    s_in, s_out = PLACEMENTS["at_limit"][0], PLACEMENTS["beyond_limit"][0]
    assert s_out == 2.0 * s_in and np.log2(s_in) == int(np.log2(s_in))
    reach = 10.0 * (1.0 + 1e-5)
    assert float(np.nextafter(np.float32(reach * s_in), np.float32(np.inf))) <= X_COORD_MAX < reach * s_out


@pytest.mark.parametrize("name", sorted(QUERY_SCENES))
def test_base_sets_are_unchanged(name):
    assert hashlib.sha256(query_set(name)[2]["recs"].tobytes()).hexdigest()[:16] == BASE_SET_SHA[name]


@pytest.mark.parametrize("base,placement", PLACED_CASES, ids=["%s/%s" % c for c in PLACED_CASES])
def test_placed_sets_meet_their_conditions(base, placement):
    """Per placed set, judged on the oracle: the oracle's BVH equals its brute force on every ray (so
    the reference is well-defined there); 1024 + 37 rays; at least 20 % hop-1 hits (75 % in the Cornell
    family) and 10 % misses; every hop-1 class the geometry allows, every hop-2 and light class among the
    hits of an all-triangle scene; in the Cornell family each shadow answer on at least 12 % of the hits
    and at least 170 hop-1 ties (x_rays.PLACED_SHARE gives edge_axis two shares of a placed set for it); the
    direction edge cases are what they say (both zeros, components that underflow in fp32); the far classes
    start 32 E and 1e3 E from the world origin, beyond the 16 E of ray_org32 -- but for the sets of
    FAR_MOVED_IN, whose both classes start at 32 E."""
    sc, _, rs, ref, frame = placed_set(base, placement)
    U.oracle_accel(1)
    try:
        bvh = U.oracle_x_query(sc.to_scn(), rs["recs"])
    finally:
        U.oracle_accel(-1)
    for k in ("prim1", "occl", "prim2"):
        assert (bvh[k] == ref[k]).all(), (k, int((bvh[k] != ref[k]).sum()), sorted({R.H1[c] for c in rs["h1"][bvh[k] != ref[k]]}))
    for k in ("t1", "t2"):
        assert U.bits_equal(bvh[k], ref[k]).all(), k
    n = len(rs["h1"])
    assert n == 1024 + 37 and n % 64 != 0
    hit = ref["prim1"] >= 0
    family = base in CORNELL_FAMILY
    assert hit.mean() >= (0.75 if family else 0.20) and (~hit).mean() >= 0.10, hit.mean()
    assert np.isposinf(ref["t1"][~hit]).all()
    g = R.Geo(sc, frame)
    want = set(R.H1) - (set() if g.shared else {"shared_edge"}) - (set() if g.shared_axis else {"edge_axis"})
    assert want <= {R.H1[c] for c in np.unique(rs["h1"])}
    if len(g.tris) == len(sc.entities):
        assert {R.H2[c] for c in np.unique(rs["h2"][hit])} == set(R.H2)
        assert {R.LIGHTS[c] for c in np.unique(rs["light"][hit])} == set(R.LIGHTS)
    assert (rs["h2"][~hit] == -1).all() and (rs["h2"][hit] >= 0).all()
    if family:
        oc = ref["occl"][hit]
        assert (oc == 1).mean() >= 0.12 and (oc == 0).mean() >= 0.12, (oc == 1).mean()
        assert (ref["nties1"] >= 2).sum() >= 170, int((ref["nties1"] >= 2).sum())
    d = rs["recs"][:, 3:6]
    for cls, zeros in (("axis1", 1), ("axis2", 2)):
        sel = rs["h1"] == R.H1.index(cls)
        assert ((d[sel] == 0.0).sum(1) == zeros).all()
        assert np.signbit(d[sel][d[sel] == 0.0]).any() and (~np.signbit(d[sel][d[sel] == 0.0])).any()
    for cls, tiny in (("tiny_1e-20", 1e-20), ("tiny_1e-45", 1e-45)):
        sel = rs["h1"] == R.H1.index(cls)
        small = np.abs(d[sel]) <= 1e6 * tiny   # (renormalised after the component was set)
        assert (small.sum(1) >= 1).all() and (d[sel][small] != 0.0).all()
        if tiny < 1e-38:   # below fp32's normal range: the cast underflows
            assert (np.abs(d[sel][small]).astype(np.float32) < 1.2e-38).all()
    # the far classes: distances from the world origin in E, both beyond x_far_r = 16 E
    E = g.ext
    o = rs["recs"][:, 0:3]
    for cls, f in frame.far.items():
        r = np.sqrt((o[rs["h1"] == R.H1.index(cls)] ** 2).sum(1))
        assert np.allclose(r, f * E, rtol=1e-12) and f >= 32.0
    assert (frame.far["far_1e6"] == 32.0) == ((base, placement) in FAR_MOVED_IN)
    assert (np.abs(o[R.near(rs)]).max(1) <= 2.5 * E).all()


def test_placed_sets_hold_hop2_ties():
    n2 = sum(int((placed_set(b, p)[3]["nties2"] >= 2).sum()) for b, p in PLACED_CASES if b in CORNELL_FAMILY)
    assert n2 >= 50, n2


# ---- the CPU restatements on placed scenes -----------------------------------------------------------
@pytest.fixture(scope="module")
def checkers(tmp_path_factory):
    d = tmp_path_factory.mktemp("xplaced")
    exes, jobs = {}, []
    for name in ("xaccel_check", "xfan_pair_check", "xflat_check", "xflat_phase_a_check", "xshadow_leaves_check"):
        exes[name] = str(d / name)
        jobs.append(subprocess.Popen(["g++", *FLAGS, "-o", exes[name], os.path.join(U.ROOT, "tests", "cpp", name + ".cpp"), *BUILDER]))
    for j in jobs:
        assert j.wait(timeout=900) == 0
    return exes


def _scn(tmp_path, base, placement):
    p = tmp_path / ("%s_%s.scn" % (base, re.sub(r"\W", "_", placement)))
    p.write_text(placed_scene(base, placement)[0].to_scn())
    return str(p)


XACCEL_ENVS = ({}, {"GI_XLEAF_MAX": "1"}, {"GI_XACCEL": "octree"})


@pytest.mark.parametrize("placement", INSIDE)
def test_xaccel_check_on_placed_scenes(checkers, tmp_path, placement):
    """The kernels' stackless walk, restated on the host, equals brute force on the placed Cornell box,
    the box with a sphere and the box with the tilted quads -- over the BVH, single-primitive leaves and
    the SAT octree, with rays drawn from the placed scene's own bounds -- and the scene is inside the
    fp32 limit.  Prints the wide-node visits per ray (a CPU restatement's count, not a device timing)."""
    for base in CORNELL_FAMILY:
        scn = _scn(tmp_path, base, placement)
        for env in XACCEL_ENVS:
            out = subprocess.run([checkers["xaccel_check"], "2000", scn], capture_output=True, text=True,
                                 env=dict(os.environ, **env), timeout=600)
            assert out.returncode == 0, (base, env, out.stdout[-2000:])
            assert re.search(r"rays \d+ mismatches 0 ", out.stdout) and ": inside the fp32" in out.stdout, out.stdout[-2000:]
            m = re.search(r"bound ([0-9.e+-]+) \+ ([0-9.e+-]+) \|cam\|.*\n.*\n.*per ray: ([0-9.]+) node visits", out.stdout)
            print(f"{base}/{placement} {env}: skip bound {m.group(1)} + {m.group(2)} |cam|, {m.group(3)} wide-node visits per ray")


@pytest.mark.parametrize("placement", INSIDE)
def test_flat_query_checkers_on_placed_scenes(checkers, tmp_path, placement):
    """The flat leaf query restated on the host (xflat_check; xflat_phase_a_check, which models triangles
    only: the box and the box with the tilted quads, 17 and 21 leaves) and the light-dead leaves' claim
    (xshadow_leaves_check: no record of a dead leaf occludes) on the placed scenes, each with rays drawn
    from the placed scene's own bounds: 0 mismatches."""
    scn = {b: _scn(tmp_path, b, placement) for b in CORNELL_FAMILY}
    runs = [["xflat_check", "2000", scn[b], "only"] for b in CORNELL_FAMILY]
    runs += [["xflat_phase_a_check", "2000", scn["cornell"], "only", "17"], ["xflat_phase_a_check", "2000", scn["grazing_tilted"], "only", "21"]]
    runs += [["xshadow_leaves_check", "4000", "scenes", *scn.values()]]
    for name, *args in runs:
        out = subprocess.run([checkers[name], *args], capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, (name, args, out.stdout[-2000:])
        m = re.match(r"rays (\d+) mismatches 0$", out.stdout.strip().splitlines()[-1])
        assert m and int(m.group(1)) >= 8000, (name, args, out.stdout[-2000:])


def test_xaccel_check_beyond_the_limit_misses_hits(checkers, tmp_path):
    """One power of two beyond the limit the restated walk misses hits brute force finds (axis-parallel
    rays that start inside the scene: the slab test's o * iv overflows, gi_dev.h inv_dir) -- the reason
    gi_scene_create refuses such a scene.  The checker says the scene is beyond the limit."""
    out = subprocess.run([checkers["xaccel_check"], "2000", _scn(tmp_path, "cornell", "beyond_limit")], capture_output=True,
                         text=True, timeout=600)
    m = re.search(r"rays (\d+) mismatches (\d+) ", out.stdout)
    assert m, out.stdout[-2000:]
    print(f"beyond_limit: {m.group(2)} of {m.group(1)} rays mismatch")
    assert out.returncode == 1 and int(m.group(2)) > 0
    assert ": BEYOND the fp32" in out.stdout


def test_fan_pair_leaves_at_every_placement(checkers, tmp_path):
    """The builder marks all 17 leaves of the Cornell box as fan pairs at every placement inside the limit
    (and the 17 beside the sphere's leaf, and beside the tilted quads' leaves)."""
    cases = [(b, p) for p in INSIDE for b in CORNELL_FAMILY]
    scns = [_scn(tmp_path, b, p) for b, p in cases]
    for b in CORNELL_FAMILY:   # ... and the scenes where they are today: the leaf counts every placement must keep
        scns.append(str(tmp_path / (b + ".scn")))
        open(scns[-1], "w").write(QUERY_SCENES[b][0]()[0].to_scn())
    out = subprocess.run([checkers["xfan_pair_check"], "info", *scns], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:]
    got = [tuple(map(int, g)) for g in re.findall(r"info \S+: leaves (\d+) fan (\d+) all (\d+) flat_ok (\d+)", out.stdout)]
    assert len(got) == len(scns), out.stdout
    unplaced = dict(zip(CORNELL_FAMILY, got[len(cases):]))
    assert unplaced["cornell"] == (17, 17, 1, 1) and unplaced["cornell_sphere"] == (18, 17, 0, 1), unplaced
    assert unplaced["grazing_tilted"][1:] == (17, 0, 1), unplaced
    for (b, p), g in zip(cases, got):
        assert g == unplaced[b], (b, p, g, unplaced[b])


@pytest.mark.parametrize("placement", INSIDE)
def test_fan_pair_decision_on_placed_cornell(checkers, tmp_path, placement):
    """The fan-pair decision plus one exact test against two exact tests (xfan_pair_check; its rays are built
    from the pairs themselves) on the placed Cornell box's 17 leaves: 0 mismatches."""
    out = subprocess.run([checkers["xfan_pair_check"], "1000", _scn(tmp_path, "cornell", placement)], capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:]
    assert "(cornell 17)" in out.stdout and re.search(r" mismatches 0$", out.stdout.strip().splitlines()[-1]), out.stdout[-1000:]
