"""GPU: Mode X on scenes at other scales and away from the origin (x_scenes.PLACEMENTS): the device
queries ray by ray, the batched ray queries, frames and feature buffers, each against the oracle on
the placed scene itself.  No tolerance and no excluded rays: primitives and shadow answers equal, t bit
for bit, a miss is (-1, +inf); fp64 radiance bit for bit.

Almost every derived bound of the Mode X path scales with max |coordinate| -- the box padding, the
own-plane skip's bound, the light-dead bound, the far-origin radius, the clamp of the reciprocal
direction -- and every other test keeps that magnitude near 10.  The placements reach the builder's
extent floor (2^-10), a skip bound near 0.3 (2^10), no shortcut left at all (2^20), a padding as large
as the scene (offset 2^20), and both sides of the fp32 box tests' coordinate limit (gi_scene.h
GI_X_COORD_MAX): just inside it everything holds, just outside gi_scene_create refuses the scene.  What
each placement is there for is asserted on the device (skip_cos, dead leaves, fan leaves against the
host builder's values), so a placement cannot silently stop exercising it."""
import os
import re
import subprocess

import numpy as np
import pytest

import aov_frames as A
import cast_rays as C
import oracle_util as U
import x_rays as R
from x_scenes import INSIDE, PLACED_CASES, PLACEMENTS, X_COORD_MAX, placed_scene, placed_set, with_env

pytestmark = pytest.mark.gpu

gi = U.pkg()
S = U.scenes()
TREE, HBM = gi.KAT_X_TREE, gi.KAT_X_HBM
FAMILY = ("cornell", "cornell_sphere", "grazing_tilted")

# base scene -> [(flags, the variant's properties)], LDS-resident, bytes per node (tests/test_gpu_x_query.py CASES)
VARIANTS = {
    "cornell": ([(0, dict(LDS=True, W4=True, TRI=True, FLAT=True)), (TREE, dict(LDS=True, W4=True, SH=True, TRI=True, FLAT=False))], 1, 256),
    "grazing_tilted": ([(0, dict(LDS=True, W4=True, TRI=True, FLAT=True)), (TREE, dict(LDS=True, W4=True, SH=True, TRI=True, FLAT=False))], 1, 256),
    "cornell_sphere": ([(0, dict(LDS=True, W4=False, TRI=False, FLAT=True)), (TREE, dict(LDS=True, W4=False, SH=True, TRI=False, FLAT=False))], 1, 256),
    "corner3_octree": ([(0, dict(LDS=True, SH=False, FLAT=False))], 1, 256),
    "soup1000": ([(0, dict(LDS=False, TRI=True, CN=False, FLAT=False))], 0, 256),
    "soup_xcnode": ([(0, dict(LDS=False, TRI=True, CN=True, FLAT=False))], 0, 128),
}
IDS = ["%s/%s" % c for c in PLACED_CASES]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    return torch


_devs = {}


def dev_of(base, placement):
    if (base, placement) not in _devs:
        sc, env = placed_scene(base, placement)
        _devs[base, placement] = (sc, with_env(env, lambda: gi.DeviceScene.from_scene(sc)))
    return _devs[base, placement]


def device_skip_cos(d, cam_pos):
    return d.kat_x_query(np.array([[0.0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0]]), cam_pos)["skip_cos"]


_well_defined = set()


def device_set(base, placement):
    """The placed set with its hop-2 directions around the device's skip_cos for the scene's own camera.
    Hop 1 is the set tests/test_x_placed_host.py checks; hop 2 and the lights differ with skip_cos, so the
    condition that the reference is well-defined -- the oracle's BVH equal to its brute force on every ray
    -- is checked again on the set that really runs (once per set)."""
    sc, d = dev_of(base, placement)
    out = placed_set(base, placement, device_skip_cos(d, sc.cam_pos))
    if (base, placement) not in _well_defined:
        _, _, rs, ref, _ = out
        U.oracle_accel(1)
        try:
            bvh = U.oracle_x_query(sc.to_scn(), rs["recs"])
        finally:
            U.oracle_accel(-1)
        for k in ("prim1", "occl", "prim2", "t1", "t2"):
            assert U.bits_equal(bvh[k].astype(np.float64), ref[k].astype(np.float64)).all(), (base, placement, k)
        _well_defined.add((base, placement))
    return out


def check_variants(base, placement):
    cases, lds, node_bytes = VARIANTS[base]
    sc, d = dev_of(base, placement)
    info = d.info()
    assert info["x_lds_resident"] == lds and info["x_node_bytes"] == node_bytes, (base, placement, info)
    for flags, want in cases:
        var = d.kat_x_variant(flags)
        assert {k: var[k] for k in want} == want, (base, placement, flags, var)
    return sc, d, [f for f, _ in cases]


def first_difference(rs, ref, out, sel):
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


# ---- the device queries ray by ray ------------------------------------------------------------------------
@pytest.mark.parametrize("base,placement", PLACED_CASES, ids=IDS)
def test_x_query_placed_equals_brute_force(torch_cuda, base, placement):
    """gi_kat_x_query over the placed set, the variant asserted first (flat and forced tree walk where
    the scene is flat): the near rays with the placed own camera and with a camera at the world origin,
    then the two far classes (32 E and 1e3 E from the world origin: gi_dev.h ray_org32 runs) with a camera
    as far out."""
    sc, d, flagses = check_variants(base, placement)
    _, _, rs, ref, frame = device_set(base, placement)
    E = R.Geo(sc, frame).ext
    near = R.near(rs)
    calls = [(near, sc.cam_pos), (near, (0.0, 0.0, 0.0))] + [R.far_call(rs, far, E, frame) for far in sorted(R.FAR)]
    for flags in flagses:
        for sel, cam in calls:
            assert sel.sum() % 64 != 0 and sel.sum() > 0
            out = d.kat_x_query(rs["recs"][sel], cam, flags)
            bad = first_difference(rs, ref, out, sel)
            assert bad is None, f"{base}/{placement} flags {flags} cam {cam}: {bad}"
            miss = out["prim1"] < 0
            assert np.isposinf(out["t1"][miss]).all() and np.isposinf(out["t2"][out["prim2"] < 0]).all()


def test_x_query_placed_hbm_walk(torch_cuda):
    """The HBM walk forced onto the Cornell box at offset 2^13 (KAT_X_HBM): the same equalities."""
    sc, d = dev_of("cornell", "off2^13")
    var = d.kat_x_variant(HBM)
    assert {k: var[k] for k in ("LDS", "TRI", "CN", "FLAT")} == dict(LDS=False, TRI=True, CN=False, FLAT=False), var
    _, _, rs, ref, frame = device_set("cornell", "off2^13")
    sel = R.near(rs)
    for cam in (sc.cam_pos, (0.0, 0.0, 0.0)):
        bad = first_difference(rs, ref, d.kat_x_query(rs["recs"][sel], cam, HBM), sel)
        assert bad is None, bad


# ---- the batched ray queries -------------------------------------------------------------------------------
def _rays(o, d, tmax):
    rays = np.zeros((len(o), C.RAY_DOUBLES))
    rays[:, 0:3], rays[:, 3:6], rays[:, 6] = o, d, tmax
    return np.ascontiguousarray(rays)


def _assert_cast(what, d, rays, prim, t, cls):
    hit = (prim >= 0) & (t < rays[:, 6])   # (the interval is open)
    exp = dict(rays=rays, prim=np.where(hit, prim, -1).astype(np.int32), t=np.where(hit, t, np.inf), occl=hit.astype(np.int32),
               cls=np.asarray(cls))
    out = d.intersect(rays, want=("t", "prim"))
    bad = C.first_difference(exp, {"prim": out["prim"], "t": out["t"]})
    assert bad is None, f"{what}: {bad[:800]}"
    bad = C.first_difference(exp, {"occl": d.occluded(rays)})
    assert bad is None, f"{what}: {bad[:800]}"


@pytest.mark.parametrize("base,placement", PLACED_CASES, ids=IDS)
def test_intersect_and_occluded_placed(torch_cuda, base, placement):
    """gi_intersect and gi_occluded over hop 1 of the placed set, the near rays and both far classes in one
    call (the far-origin rule per lane)."""
    sc, d, _ = check_variants(base, placement)
    _, _, rs, ref, _ = device_set(base, placement)
    recs = rs["recs"]
    assert len(recs) % 64 != 0
    _assert_cast(f"{base}/{placement}", d, _rays(recs[:, 0:3], recs[:, 3:6], np.inf), ref["prim1"], ref["t1"],
                 [R.H1[c] for c in rs["h1"]])


@pytest.mark.parametrize("placement", ["off2^13", "x2^20"])
@pytest.mark.parametrize("base", ["cornell", "soup1000"])
def test_tmax_classes_placed(torch_cuda, base, placement):
    """The tmax classes of tests/cast_rays.py (inf, t1, nextafter(t1), t1 / 2, 2 t1, 1e-7, 0, -1 on hits; inf,
    1e3 on misses) over the placed set's hop 1: a hit exactly when t1 < tmax."""
    sc, d, _ = check_variants(base, placement)
    _, _, rs, ref, _ = device_set(base, placement)
    prim, t = ref["prim1"], ref["t1"]
    hit = prim >= 0
    k = np.zeros(len(prim), np.int64)
    k[hit] = np.arange(hit.sum()) % len(C.TMAX_HIT)
    k[~hit] = len(C.TMAX_HIT) + np.arange((~hit).sum()) % len(C.TMAX_MISS)
    tmax = np.zeros(len(prim))
    for j, (_, f) in enumerate(C.TMAX_HIT):
        tmax[k == j] = f(t[k == j])
    for j, (_, v) in enumerate(C.TMAX_MISS):
        tmax[k == len(C.TMAX_HIT) + j] = v
    assert set(np.unique(k)) == set(range(len(C.TMAX_CLASSES)))
    cls = [C.TMAX_CLASSES[a] + " / " + R.H1[b] for a, b in zip(k, rs["h1"])]
    _assert_cast(f"{base}/{placement} tmax", d, _rays(rs["recs"][:, 0:3], rs["recs"][:, 3:6], tmax), prim, t, cls)


# ---- frames and feature buffers ----------------------------------------------------------------------------
W = H = 24
SPP, DEPTH, SEED = 2, 4, 11
FORMS = (("default", 0), ("mega", gi.FLAG_X_MEGA), ("all_leaves", gi.FLAG_X_ALL_LEAVES))


def _check_frames(torch, what, sc, d):
    o = U.oracle_render(sc.to_scn(), W, H, mode=1, spp=SPP, depth=DEPTH, seed=SEED)
    seen = (o["hit"] >= 0).mean()
    assert seen >= 0.30, (what, seen)
    cam = gi.Camera(sc.cam_pos, sc.cam_look, sc.focal)
    for form, flags in FORMS:
        st = torch.zeros(gi.STATS_N, dtype=torch.int64, device="cuda")
        buf = torch.zeros(W * H * 3, dtype=torch.float64, device="cuda")
        buf8 = torch.zeros(W * H * 3, dtype=torch.uint8, device="cuda")
        d.render_device(cam, sc.light, W, H, buf.data_ptr(), buf8.data_ptr(), mode=gi.MODE_X, spp=SPP, depth=DEPTH, seed=SEED,
                        stats_ptr=st.data_ptr(), flags=flags)
        torch.cuda.synchronize()
        rgb, rgb8 = buf.cpu().numpy().reshape(-1, 3), buf8.cpu().numpy().reshape(-1, 3)
        same = U.bits_equal(rgb, o["rgb"]).all(1)
        assert same.all(), f"{what} {form}: {int((~same).sum())} of {same.size} pixels differ, first {int(np.flatnonzero(~same)[0])}"
        assert (rgb8 == o["q"]).all(), (what, form)
        assert int(st.cpu().numpy()[gi.STAT_RAYS]) == int(o["ncand"].sum()), (what, form)
    ref = A._reference(sc, W, H)   # the oracle's first hits of the frame's pixel rays
    aov = d.render_aov(cam, W, H, want=("t", "prim"))
    assert (aov["prim"].reshape(-1) == ref["prim"]).all(), what
    assert U.bits_equal(aov["t"].reshape(-1), ref["t"]).all(), what
    assert (ref["prim"] >= 0).mean() >= 0.30


@pytest.mark.parametrize("placement", INSIDE)
@pytest.mark.parametrize("base", FAMILY)
def test_frames_placed_bit_exact(torch_cuda, base, placement):
    """24 x 24, 2 spp, depth 4 from the placed own camera, as k_seg runs it, as k_mode_x (GI_FLAG_X_MEGA) and
    with every leaf's shadow test (GI_FLAG_X_ALL_LEAVES): fp64 radiance bit for bit, RGB888 equal,
    GI_STAT_RAYS the oracle's ncand sum, at least 30 % of the pixels seeing geometry (judged on the
    oracle); and gi_render_aov's t / prim are the oracle's first hits of the same frame."""
    sc, d = dev_of(base, placement)
    _check_frames(torch_cuda, f"{base}/{placement}", sc, d)


def test_at_limit_axis_camera_just_inside_the_far_radius(torch_cuda):
    """The Cornell box just inside the coordinate limit, seen along +x from just under 16 extents out (the
    farthest origin the fp32 box tests take as given; beyond it ray_org32 moves them): the frame's centre
    ray (pixel 12, 12 of 24) is exactly (1, 0, 0) from y = z = 0, axis-parallel on two axes with the
    origin inside both slabs.  Frames, feature buffers and the near rays of the set with this camera."""
    sc0, d = dev_of("cornell", "at_limit")
    s = PLACEMENTS["at_limit"][0]
    sc, _ = placed_scene("cornell", "at_limit")
    sc.cam_pos, sc.cam_look, sc.focal = (-15.9 * 10.0 * s, 0.0, 0.0), (5.0 * s, 0.0, 0.0), 0.1
    assert 16.0 * 10.0 * s > abs(sc.cam_pos[0]) > 15.0 * 10.0 * s
    rays = A.rays_np(sc, W, H)
    assert (rays[12 * W + 12, 3:6] == (1.0, 0.0, 0.0)).all()
    _check_frames(torch_cuda, "cornell/at_limit axis camera", sc, d)
    _, _, rs, ref, _ = device_set("cornell", "at_limit")
    sel = R.near(rs)
    for flags in (0, TREE):
        bad = first_difference(rs, ref, d.kat_x_query(rs["recs"][sel], sc.cam_pos, flags), sel)
        assert bad is None, bad


# ---- the limit -----------------------------------------------------------------------------------------------
def test_beyond_the_limit_scene_creation_refuses(torch_cuda):
    """One power of two beyond the limit gi_scene_create returns GI_ERR_SCENE with a message that names the
    limit -- before anything is uploaded or launched, so no render, ray query, feature buffer, adaptive
    pass or test hook can be asked of such a scene -- while the scene just inside it is made."""
    for base in FAMILY:
        sc, env = placed_scene(base, "beyond_limit")
        with pytest.raises(gi.GIError) as e:
            with_env(env, lambda: gi.DeviceScene.from_scene(sc))
        msg = str(e.value)
        assert "(-3)" in msg and "%.9g" % X_COORD_MAX in msg, msg   # GI_ERR_SCENE
        assert gi.lib().gi_last_error().decode() != "" and "beyond the supported range" in msg
    assert dev_of("cornell", "at_limit")[1].info()["x_prims"] == 34


# ---- the shortcuts a placement is there for are really taken, or really off ------------------------------------
@pytest.fixture(scope="module")
def host_info(tmp_path_factory):
    """What the host builder derives per placed scene (tests/cpp/xplaced_info.cpp over the product's builder)."""
    d = tmp_path_factory.mktemp("xplaced_info")
    exe = str(d / "xplaced_info")
    csrc = os.path.join(U.ROOT, "2019global_amd", "csrc")
    subprocess.run(["g++", "-O1", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I" + csrc, "-I" + os.path.join(U.ROOT, "include"),
                    "-o", exe, os.path.join(U.ROOT, "tests", "cpp", "xplaced_info.cpp"), os.path.join(csrc, "gi_build.cpp"),
                    os.path.join(csrc, "gi_bvh.cpp")], check=True, timeout=600)
    info = {}
    for base in FAMILY:
        for placement in INSIDE:
            sc, env = placed_scene(base, placement)
            p = d / "s.scn"
            p.write_text(sc.to_scn())
            out = subprocess.run([exe, str(p)], capture_output=True, text=True, env=dict(os.environ, **env), timeout=600).stdout
            m = re.search(r"skip_cos (\S+) dead_c \S+ nodes \d+ leaves (\d+) flat_ok 1 fan (\d+) boundary (\w+) live (\w+)", out)
            assert m, out
            info[base, placement] = (float(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4), 16), int(m.group(5), 16))
    return info


# placement -> the own-plane skip can happen (skip_cos <= 1), leaves of the Cornell box the own light leaves dead
EXPECT = {"x2^-10": (True, 7), "x2^10": (True, 0), "x2^20": (False, 0), "off2^13": (True, 0), "off2^20": (False, 0),
          "x2^-10_off2^7": (True, 0), "at_limit": (False, 0)}


@pytest.mark.parametrize("placement", INSIDE)
def test_shortcuts_per_placement_match_the_host_builder(torch_cuda, host_info, placement):
    """Per placement and scene of the Cornell family the device scene's skip_cos (own camera), flat and fan
    leaf counts and gi_scene_shadow_leaves masks (own light and camera) are the host builder's; the skip
    bound is on the side of 1 the placement is there for (above 1 at 2^20, at offset 2^20 and at the
    limit: no own-plane skip is ever taken), the Cornell box keeps its 17 fan leaves and seven boundary
    leaves everywhere, and its dead leaves are as many as expected: all seven at 2^-10, none elsewhere
    (the light-dead bound grows with max |coordinate|)."""
    for base in FAMILY:
        sc, d = dev_of(base, placement)
        skip_cos, leaves, fan, bnd, live = host_info[base, placement]
        got = device_skip_cos(d, sc.cam_pos)
        info = d.info()
        dbnd, dlive = d.shadow_leaves(sc.light, sc.cam_pos)
        dead = bin(dbnd & ~dlive).count("1")
        print(f"{base}/{placement}: device skip_cos {got:.6g}, dead leaves {dead} of {bin(dbnd).count('1')} boundary, "
              f"fan leaves {info['x_fan_leaves']} of {info['x_flat_leaves']}")
        assert abs(got - skip_cos) <= 1e-12 * skip_cos, (base, got, skip_cos)
        assert (info["x_flat_leaves"], info["x_fan_leaves"]) == (leaves, fan) and fan == 17, (base, info)
        assert (dbnd, dlive & ((1 << leaves) - 1)) == (bnd, live), (base, hex(dbnd), hex(dlive), hex(bnd), hex(live))
        can_skip, n_dead = EXPECT[placement]
        assert (got <= 1.0) == can_skip, (base, got)
        if base == "cornell":
            assert bin(dbnd).count("1") == 7 and dead == n_dead, (hex(dbnd), hex(dlive))
