"""GPU: the Mode X device queries ray by ray (gi_kat_x_query) against the oracle's brute force, and
Mode X frames from cameras inside, on and far from the geometry.

The hook runs one path segment's three queries -- closest hit, shadow any-hit from the hit point,
closest hit of the next ray -- per ray, in the kernel variant the segment form (k_seg) runs for the
scene, so a wrong (t, primitive) cannot hide behind shading.  The rays (tests/x_rays.py) sit where
the queries' arithmetic has edges; the reference is gio_x_query with brute force.  No tolerance and
no excluded rays: primitives and shadow answers equal, t bit for bit, a miss is (-1, +inf)."""
import numpy as np
import pytest

import oracle_util as U
import x_rays as R
from x_scenes import QUERY_SCENES, STANDIN_SKIP_COS, XFLAT_MAX, query_set, with_env, with_sphere

pytestmark = pytest.mark.gpu

gi = U.pkg()
S = U.scenes()
TREE, HBM = gi.KAT_X_TREE, gi.KAT_X_HBM

# case -> (scene, flags, the variant's properties the case is there for, LDS-resident, bytes per node)
FLAT_W4 = ("cornell", "grazing_floor", "grazing_tilted", "soup_max", "three_record_leaves", "coincident", "one_triangle",
           "empty")
FLAT_OTHER = ("cornell_mirror", "cornell_sphere")   # an ImpSphere each: not triangles only, 3 waves per SIMD
CASES = {}
for _n in FLAT_W4:
    CASES[_n + "/flat"] = (_n, 0, dict(LDS=True, W4=True, TRI=True, FLAT=True), 1, 256)
    CASES[_n + "/tree"] = (_n, TREE, dict(LDS=True, W4=True, SH=True, TRI=True, FLAT=False), 1, 256)
for _n in FLAT_OTHER:
    CASES[_n + "/flat"] = (_n, 0, dict(LDS=True, W4=False, TRI=False, FLAT=True), 1, 256)
    CASES[_n + "/tree"] = (_n, TREE, dict(LDS=True, W4=False, SH=True, TRI=False, FLAT=False), 1, 256)
CASES["soup_max_plus_1/tree"] = ("soup_max_plus_1", 0, dict(LDS=True, SH=True, FLAT=False), 1, 256)
CASES["corner3_octree/deep_tree"] = ("corner3_octree", 0, dict(LDS=True, SH=False, FLAT=False), 1, 256)
CASES["soup1000/hbm"] = ("soup1000", 0, dict(LDS=False, TRI=True, CN=False, FLAT=False), 0, 256)
CASES["zoo/hbm"] = ("zoo", 0, dict(LDS=False, TRI=False, CN=False, FLAT=False), 0, 256)
CASES["cornell/hbm"] = ("cornell", HBM, dict(LDS=False, TRI=True, CN=False, FLAT=False), 1, 256)
CASES["soup_xcnode/hbm_quantised"] = ("soup_xcnode", 0, dict(LDS=False, TRI=True, CN=True, FLAT=False), 0, 128)
assert {c[0] for c in CASES.values()} == set(QUERY_SCENES)

OUTS = ("prim1", "t1", "occl", "skip_s", "prim2", "t2", "skip2")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    return torch


_devs = {}


def dev_of(name):
    if name not in _devs:
        sc, env = QUERY_SCENES[name][0]()
        _devs[name] = (sc, with_env(env, lambda: gi.DeviceScene.from_scene(sc)))
    return _devs[name]


def device_skip_cos(d, cam_pos):
    return d.kat_x_query(np.array([[0.0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0]]), cam_pos)["skip_cos"]


def device_set(name):
    """The scene's ray set, its hop-2 directions placed around the device's skip_cos for the scene's
    own camera, with the brute-force reference (built once per scene)."""
    sc, d = dev_of(name)
    return query_set(name, device_skip_cos(d, sc.cam_pos))


def first_difference(rs, ref, out, sel):
    """The first ray of a call on which the device and the reference differ: index, classes, values."""
    idx = np.flatnonzero(sel)
    for k in ("prim1", "t1", "occl", "prim2", "t2"):
        a, b = out[k], ref[k][sel]
        ne = ~U.bits_equal(a, b) if a.dtype == np.float64 else a != b
        if ne.any():
            j = int(np.flatnonzero(ne)[0])
            i = int(idx[j])
            return (f"{int(ne.sum())} of {len(a)} rays differ in {k}; first: ray {i} class {R.H1[rs['h1'][i]]} / "
                    f"{R.H2[rs['h2'][i]] if rs['h2'][i] >= 0 else '-'} / {R.LIGHTS[rs['light'][i]] if rs['light'][i] >= 0 else '-'}: "
                    f"device prim1 {out['prim1'][j]} t1 {out['t1'][j]!r} occl {out['occl'][j]} prim2 {out['prim2'][j]} "
                    f"t2 {out['t2'][j]!r} skip {out['skip_s'][j]}/{out['skip2'][j]}, reference prim1 {ref['prim1'][i]} "
                    f"t1 {ref['t1'][i]!r} occl {ref['occl'][i]} prim2 {ref['prim2'][i]} t2 {ref['t2'][i]!r}; "
                    f"record {rs['recs'][i].tolist()}")
    return None


def check_variant(case):
    name, flags, want, lds, node_bytes = CASES[case]
    sc, d = dev_of(name)
    var, info = d.kat_x_variant(flags), d.info()
    assert {k: var[k] for k in want} == want, (case, var)
    assert info["x_lds_resident"] == lds and info["x_node_bytes"] == node_bytes, (case, info)
    return sc, d, flags


CAMS = ("own", (0.0, 0.0, 0.0), (600.0, -1000.0, 300.0))


@pytest.mark.parametrize("case", sorted(CASES))
def test_x_query_device_equals_brute_force(torch_cuda, case):
    """Every near ray of the scene's set through the case's kernel variant: prim1, prim2 and occl equal
    the oracle's brute force and t1, t2 are bit-equal.  The variant is asserted first
    (gi_kat_x_variant, x_lds_resident, x_node_bytes), so each of k_seg's variants is shown to have run:
    the flat query (4 and 3 waves per SIMD), the LDS tree walk with one-word and two-word level masks,
    the HBM walk over wide and over quantised nodes.  Three camera positions (the own-plane skip's
    bound depends on it): the scene's own, the origin and one of magnitude 1e3."""
    sc, d, flags = check_variant(case)
    _, _, rs, ref = device_set(CASES[case][0])
    sel = R.near(rs)
    assert sel.sum() % 64 != 0
    for cam in CAMS:
        cam = sc.cam_pos if cam == "own" else cam
        out = d.kat_x_query(rs["recs"][sel], cam, flags)
        bad = first_difference(rs, ref, out, sel)
        assert bad is None, f"{case} cam {cam}: {bad}"
        miss = out["prim1"] < 0
        assert np.isposinf(out["t1"][miss]).all() and np.isposinf(out["t2"][out["prim2"] < 0]).all()


@pytest.mark.parametrize("far", sorted(R.FAR))
def test_x_query_far_origins_equal_brute_force(torch_cuda, far):
    """The rays that start 1e3 and 1e6 scene extents out, aimed at inner points and (every other ray)
    exactly at vertices of the triangles, through every case's variant, with a camera as far out: the
    same equalities.

    This test found the queries' box tests not conservative for such rays: they ran on the fp32 cast
    of the origin (three roundings of about 2^-24 |o| against a padding of 1e-5 extents: good to about
    50 extents), and on the MI355X the device missed hits the brute force finds, or returned a farther
    hit or the higher primitive of a tie -- from 1e3 extents in 17 of the 26 cases (1 to 9 rays of 70
    to 275 each, the ones aimed at vertices), from 1e6 in 22 of 26 (19 of 275 on the Cornell box, 47
    of 139 on soup1000, 35 of 70 over quantised nodes).  Since then a launch whose camera is more than
    16 extents out runs the fp32 tests from a point of the ray near the scene (gi_dev.h ray_org32;
    the fp64 tests keep the ray as given), and both classes hold in every case."""
    bad, total = [], 0
    for case in sorted(CASES):
        sc, d, flags = check_variant(case)
        _, _, rs, ref = device_set(CASES[case][0])
        sel, cam = R.far_call(rs, far, R.Geo(sc).ext)
        assert sel.sum() % 64 != 0 and sel.sum() > 0
        out = d.kat_x_query(rs["recs"][sel], cam, flags)
        total += int(sel.sum())
        msg = first_difference(rs, ref, out, sel)
        if msg is not None:
            bad.append(f"{case}: {msg}")
    print(f"{far}: {len(bad)} of {len(CASES)} cases differ over {total} rays")
    for b in bad:
        print("  " + b[:400])
    assert not bad, f"{len(bad)} of {len(CASES)} cases differ; " + " | ".join(b[:160] for b in bad)


@pytest.mark.parametrize("name", FLAT_W4 + FLAT_OTHER)
def test_x_query_flat_and_tree_identical_and_frames_take_flat(torch_cuda, name):
    """The flat leaf query and the forced tree walk of one scene return identical arrays, the reported
    skips included; and a frame of the scene really runs the flat kernel the hook ran: the segment
    form, whose node count is the table's 256-byte units per query (the stats rule of
    tests/test_gpu_flat_leaves.py; at most GI_XFLAT_MAX leaves of 32 bytes)."""
    sc, d = dev_of(name)
    _, _, rs, _ = device_set(name)
    recs = rs["recs"][R.near(rs)]
    a = d.kat_x_query(recs, sc.cam_pos, 0)
    b = d.kat_x_query(recs, sc.cam_pos, TREE)
    for k in OUTS:
        assert (a[k] == b[k]).all() if a[k].dtype != np.float64 else U.bits_equal(a[k], b[k]).all(), (name, k)
    assert a["skip_cos"] == b["skip_cos"]
    w, h, spp, depth = 32, 32, 2, 3
    assert d.x_form(spp=spp, depth=depth) == "k_seg" and d.kat_x_variant(0)["FLAT"]
    torch = torch_cuda
    st = torch.zeros(gi.STATS_N, dtype=torch.int64, device="cuda")
    buf = torch.zeros(w * h * 3, dtype=torch.float64, device="cuda")
    d.render_device(gi.Camera(sc.cam_pos, sc.cam_look, sc.focal), sc.light, w, h, buf.data_ptr(), mode=gi.MODE_X, spp=spp,
                    depth=depth, seed=7, stats_ptr=st.data_ptr())
    torch.cuda.synchronize()
    st = st.cpu().numpy()
    queries = int(st[gi.STAT_RAYS]) - int(st[gi.STAT_X_RESOLVED])
    if name == "empty":
        assert int(st[gi.STAT_NODES]) == 0
    else:
        assert queries > 0 and int(st[gi.STAT_NODES]) % queries == 0
        assert 1 <= int(st[gi.STAT_NODES]) // queries <= (XFLAT_MAX * 32 + 255) // 256


def test_x_query_skip_bound_is_straddled_on_cornell(torch_cuda):
    """The hop-2 directions u + c n with c a multiple of skip_cos and the lights almost in the hit's
    plane sit on both sides of the own-plane skip's bound: the device reports at least 100 skipped and
    100 unskipped rays among them, for the next ray (skip2) and for the shadow ray (skip_s).  The
    stand-in the CPU tests build their sets around lies within a factor of 10 of the device's bound."""
    sc, d = dev_of("cornell")
    skip_cos = device_skip_cos(d, sc.cam_pos)
    assert STANDIN_SKIP_COS / 10 <= skip_cos <= STANDIN_SKIP_COS * 10, skip_cos
    _, _, rs, ref = device_set("cornell")
    near = R.near(rs)   # (the far rays belong with a camera as far out)
    rs = {k: v[near] for k, v in rs.items()}
    ref = {k: v[near] for k, v in ref.items()}
    out = d.kat_x_query(rs["recs"], sc.cam_pos, 0)
    assert out["skip_cos"] == skip_cos
    near_bound = np.isin(rs["h2"], [j for j, c in enumerate(R.H2_C) if c[1] != 0.0])
    assert (out["skip2"][near_bound] < 254).sum() >= 100 and (out["skip2"][near_bound] == 254).sum() >= 100
    above = np.isin(rs["h2"], [j for j, c in enumerate(R.H2_C) if abs(c[1]) > 1.0 or abs(c[2]) == 0.5])
    below = np.isin(rs["h2"], [j for j, c in enumerate(R.H2_C) if abs(c[1]) < 1.0 and abs(c[2]) < 0.5])
    assert (out["skip2"][above] < 254).all() and (out["skip2"][below] == 254).all()   # (the box: every triangle in a group)
    hit = ref["prim1"] >= 0
    graze = rs["light"] == R.LIGHTS.index("graze_plane")
    assert (out["skip_s"][graze] == 254).sum() >= 100 and (out["skip_s"][hit & ~graze] < 254).sum() >= 100
    assert (out["skip_s"][~hit] == 254).all() and (out["skip2"][~hit] == 254).all()


def test_x_query_one_ray_and_none(torch_cuda):
    """A call with a single ray (63 lanes of its wave without one) and a call with none."""
    sc, d = dev_of("cornell")
    _, _, rs, ref = device_set("cornell")
    i = int(np.flatnonzero(R.near(rs) & (ref["prim1"] >= 0) & (ref["prim2"] >= 0))[0])
    for flags in (0, TREE, HBM):
        out = d.kat_x_query(rs["recs"][i:i + 1], sc.cam_pos, flags)
        assert out["prim1"][0] == ref["prim1"][i] and out["prim2"][0] == ref["prim2"][i] and out["occl"][0] == ref["occl"][i]
        assert U.bits_equal(out["t1"], ref["t1"][i:i + 1]).all() and U.bits_equal(out["t2"], ref["t2"][i:i + 1]).all()
    none = d.kat_x_query(np.zeros((0, 12)), sc.cam_pos, 0)
    assert len(none["prim1"]) == 0 and none["skip_cos"] is None


# ---- camera placement at frame level ---------------------------------------------------------------
W = H = 24
F45 = W * 1e-4   # the pixel pitch is 2e-4: the frame spans about +-45 degrees
# (position, look-at, focal, sealed): the box is x in [0, 10], y and z in [-5, 5], open toward -x
CAMERAS = {
    "centre+x": ((5.0, 0.0, 0.0), (6.0, 0.0, 0.0), F45, False),
    # toward the open side only rays beyond 45 degrees meet a wall: half the focal length, +-63 degrees
    "centre-x": ((5.0, 0.0, 0.0), (4.0, 0.0, 0.0), F45 / 2, False),
    "centre+y": ((5.0, 0.0, 0.0), (5.0, 1.0, 0.0), F45, False),
    "centre-y": ((5.0, 0.0, 0.0), (5.0, -1.0, 0.0), F45, False),
    "centre_oblique_a": ((5.0, 0.0, 0.0), (6.0, 1.0, 0.5), F45, False),
    "centre_oblique_b": ((5.0, 0.0, 0.0), (5.7, -1.0, -0.7), F45, False),
    "on_wall_plane": ((4.0, 5.0, 1.0), (6.0, -5.0, -1.0), F45, False),
    "inside_tall_block": ((7.75, 1.75, -2.0), (9.0, 2.0, -1.5), F45, True),
    "outside_corner": ((-0.1, -5.1, -5.1), (10.0, 5.0, 5.0), F45, False),
    "far_1e3": ((-1000.0, 0.0, 0.0), (5.0, 0.0, 0.0), W * 0.02, False),   # the box's +-5 at distance 1000 fills the frame
}
CAM_SCENES = {"cornell": lambda: S.named_scene("cornell"), "cornell_mirror": lambda: S.named_scene("cornell_mirror"),
              "cornell_sphere": lambda: with_sphere()[0]}
_cam_devs = {}


@pytest.mark.parametrize("cam", sorted(CAMERAS))
@pytest.mark.parametrize("scene", sorted(CAM_SCENES))
def test_mode_x_camera_placements_bit_exact(torch_cuda, scene, cam):
    """Mode X frames (24 x 24, 2 spp, depth 4) from cameras at the box centre looking along the axes
    and obliquely, exactly on a wall plane, sealed inside the tall block, just outside a corner and
    1e3 units away: fp64 radiance bit for bit and the same RGB888 as the oracle, and as many rays
    traced (GI_STAT_RAYS against the oracle's per-pixel counts).  k_x_classify's root-box and frustum
    shortcuts and the own-plane skip's bound depend on the camera position.  Each frame sees geometry
    in at least 30 % of its pixels (all of them from inside the block), judged on the oracle."""
    pos, look, focal, sealed = CAMERAS[cam]
    sc = CAM_SCENES[scene]()
    sc.cam_pos, sc.cam_look, sc.focal = pos, look, focal
    if scene not in _cam_devs:
        _cam_devs[scene] = gi.DeviceScene.from_scene(sc)
    d = _cam_devs[scene]
    spp, depth, seed = 2, 4, 11
    o = U.oracle_render(sc.to_scn(), W, H, mode=1, spp=spp, depth=depth, seed=seed)
    seen = (o["hit"] >= 0).mean()
    assert seen == 1.0 if sealed else seen >= 0.30, (cam, seen)
    torch = torch_cuda
    st = torch.zeros(gi.STATS_N, dtype=torch.int64, device="cuda")
    buf = torch.zeros(W * H * 3, dtype=torch.float64, device="cuda")
    buf8 = torch.zeros(W * H * 3, dtype=torch.uint8, device="cuda")
    d.render_device(gi.Camera(pos, look, focal), sc.light, W, H, buf.data_ptr(), buf8.data_ptr(), mode=gi.MODE_X, spp=spp,
                    depth=depth, seed=seed, stats_ptr=st.data_ptr())
    torch.cuda.synchronize()
    rgb, rgb8 = buf.cpu().numpy().reshape(-1, 3), buf8.cpu().numpy().reshape(-1, 3)
    same = U.bits_equal(rgb, o["rgb"]).all(1)
    assert same.all(), f"{scene} {cam}: {int((~same).sum())} of {same.size} pixels differ, first {int(np.flatnonzero(~same)[0])}"
    assert (rgb8 == o["q"]).all()
    assert int(st.cpu().numpy()[gi.STAT_RAYS]) == int(o["ncand"].sum())


# ---- k_mode_x forced onto small scenes -----------------------------------------------------------------
# k_mode_x reads every scene from global memory, so forcing it (GI_FLAG_X_MEGA) onto a scene that k_seg
# stages in LDS runs the instantiation a large scene of the same properties would: STATS x HELP x CN x
# SH x TR.  scene -> the properties of the device scene that pick the instantiation (None: not asserted).
MEGA_W, MEGA_H, MEGA_SPP, MEGA_DEPTH, MEGA_SEED = 48, 40, 3, 5, 2019
MEGA_SCENES = {
    "corner3_octree": dict(SH=False, TRI=True, CN=False),   # 12 levels: the two-word level masks
    "cornell_sphere": dict(SH=True, TRI=False, CN=False),   # a sphere: the general shading and primitive test
    "one_triangle": dict(SH=True, TRI=True, CN=False),
    "empty": None,                                          # no primitive: every pixel 0, nothing hangs
    "soup_xcnode": dict(SH=None, TRI=True, CN=True),        # quantised nodes
}
_mega_ref = {}


def mega_reference(name):
    """The oracle's frame of a scene (its own camera), computed once and shared by the two tests."""
    if name not in _mega_ref:
        sc = QUERY_SCENES[name][0]()[0]
        o = U.oracle_render(sc.to_scn(), MEGA_W, MEGA_H, mode=1, spp=MEGA_SPP, depth=MEGA_DEPTH, seed=MEGA_SEED)
        for a in o.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _mega_ref[name] = o
    return _mega_ref[name]


@pytest.mark.parametrize("name", sorted(MEGA_SCENES))
def test_forced_k_mode_x_on_small_scenes_bit_exact(torch_cuda, name):
    """GI_FLAG_X_MEGA on scenes k_seg would run (LDS-resident ones, and a small quantised soup): the 48 x
    40 frame at 3 spp, depth 5 equals the oracle's bit for bit, RGB888 included -- launches this small
    take the shadow-ray handoff build.  The scenes cover the instantiation axes: a 12-level tree (SH
    off), a sphere (TR off), quantised nodes (CN on), one triangle, and the empty scene (all 0)."""
    sc, d = dev_of(name)
    want = MEGA_SCENES[name]
    if want is not None:   # the scene still has the properties the case is there for
        var, info = d.kat_x_variant(0 if want["CN"] else TREE), d.info()
        assert info["x_node_bytes"] == (128 if want["CN"] else 256), info
        assert var["CN"] == want["CN"] and var["TRI"] == want["TRI"], var
        assert want["SH"] is None or var["SH"] == want["SH"], var
    assert d.x_form(spp=MEGA_SPP, depth=MEGA_DEPTH, flags=gi.FLAG_X_MEGA) == "k_mode_x"
    o = mega_reference(name)
    rgb, rgb8 = d.render(gi.Camera(sc.cam_pos, sc.cam_look, sc.focal), sc.light, MEGA_W, MEGA_H, mode=gi.MODE_X,
                         spp=MEGA_SPP, depth=MEGA_DEPTH, seed=MEGA_SEED, flags=gi.FLAG_X_MEGA)
    same = U.bits_equal(rgb.reshape(-1, 3), o["rgb"]).all(1)
    assert same.all(), f"{name}: {int((~same).sum())} of {same.size} pixels differ, first {int(np.flatnonzero(~same)[0])}"
    assert (rgb8.reshape(-1, 3) == o["q"]).all()
    if name == "empty":
        assert not rgb.any() and not rgb8.any()
    else:
        assert (o["hit"] >= 0).mean() >= 0.30, name   # the frame sees the scene


def test_forced_k_mode_x_on_small_scenes_without_handoff(torch_cuda, tmp_path):
    """The same frames from the builds without the shadow-ray handoff (GI_X_HELP=0, read once per
    process: a child process renders all the scenes): equal to the oracle's bit for bit."""
    import os
    import subprocess
    import sys
    out = tmp_path / "mega_nohelp.npz"
    code = ("import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r); import oracle_util as U; "
            "from x_scenes import QUERY_SCENES, with_env; gi = U.pkg(); res = {}\n"
            "for name in %r:\n"
            "    sc, env = QUERY_SCENES[name][0](); d = with_env(env, lambda: gi.DeviceScene.from_scene(sc))\n"
            "    res[name] = d.render(gi.Camera(sc.cam_pos, sc.cam_look, sc.focal), sc.light, %d, %d, mode=gi.MODE_X, "
            "spp=%d, depth=%d, seed=%d, flags=gi.FLAG_X_MEGA)[0]\n"
            "np.savez(%r, **res)") % (U.ROOT, os.path.join(U.ROOT, "tests"), tuple(sorted(MEGA_SCENES)), MEGA_W, MEGA_H,
                                      MEGA_SPP, MEGA_DEPTH, MEGA_SEED, str(out))
    subprocess.run([sys.executable, "-c", code], check=True, timeout=300, env=dict(os.environ, GI_X_HELP="0"))
    got = np.load(out)
    for name in sorted(MEGA_SCENES):
        same = U.bits_equal(got[name].reshape(-1, 3), mega_reference(name)["rgb"]).all(1)
        assert same.all(), f"{name}: {int((~same).sum())} of {same.size} pixels differ, first {int(np.flatnonzero(~same)[0])}"
