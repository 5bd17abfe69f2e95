"""GPU (gfx950): Mode R away from Scene's default camera.  Every other Mode R test renders from
(-10, 0, 0) looking at (1, 0, 0), where each pixel ray's x component is positive and dominant and all
geometry lies in front of a camera far outside it.  Here the placements of tests/r_cameras.py -- every
sign pattern of the ray direction, steep (sheared) views, cameras inside the geometry and on its
planes, geometry behind the camera (the reference's tests have no t > 0), cameras 1e3 and 1e5 units out
-- in 40 x 28 frames with a ragged last tile row, against the CPU oracle, which
tests/test_mode_r_cameras_host.py pins to the compiled reference at these very placements:

  (a) DeviceScene.render against the oracle (and the reference's golden) on every pixel, at
      test_gpu_parity.py's Mode R bar: 1e-5 relative per channel, RGB888 exact, NaN in the same places;
  (b) the four routes -- k_mode_r, the flat phases, k_mode_r_batch, the flat phases with no pool --
      bit-identical, each in a child process (the knobs are read once per process);
  (c) GI_FLAG_R_DFS bit-identical to the default;
  (d) three packed shards after unshard, and bands of 8 rows, equal the whole frame;
  (e) gi_trace_ray on pixels chosen on the oracle: hit entity and (u, v) exact, colour at the bar.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_util as U
import r_cameras as RC
from test_gpu_parity import assert_rel   # the project's Mode R bar

pytestmark = pytest.mark.gpu

gi = U.pkg()
W, H = RC.W, RC.H
FRAME_IDS = [f"{s}/{n}" for s, n in RC.FRAMES]


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    return torch


_dev, _frames = {}, {}


def dev_scene(scene):
    if scene not in _dev:
        _dev[scene] = gi.DeviceScene.from_scene(RC.base_scene(scene))
    return _dev[scene]


def cam_light(scene, name):
    sc = RC.scene_at(scene, name)
    return gi.Camera(sc.cam_pos, sc.cam_look, sc.focal), sc.light


def dev_frame(scene, name):
    """The placement's frame by this process's default route, rendered once: (fp64, RGB888), read-only."""
    if (scene, name) not in _frames:
        cam, light = cam_light(scene, name)
        rgb, rgb8 = dev_scene(scene).render(cam, light, W, H)
        rgb.setflags(write=False)
        rgb8.setflags(write=False)
        _frames[(scene, name)] = (rgb, rgb8)
    return _frames[(scene, name)]


def _against(rgb, rgb8, ref, what):
    g, g8 = rgb.reshape(-1, 3), rgb8.reshape(-1, 3)
    assert (np.isnan(g) == np.isnan(ref["rgb"])).all(), f"{what}: NaN in other places"
    assert_rel(g, ref["rgb"], what)
    diff = (g8 != ref["q"]).any(1)
    assert not diff.any(), f"{what}: {int(diff.sum())} RGB888 pixels differ (first: pixel {int(np.nonzero(diff)[0][0])}, " \
                           f"255 c = {255 * ref['rgb'][diff][0]}, device {g8[diff][0]}, reference {ref['q'][diff][0]})"
    return U.bits_equal(g, ref["rgb"]).all(1).mean()


# ---- (a) frames ------------------------------------------------------------------------------------
@pytest.mark.parametrize("scene,name", RC.FRAMES, ids=FRAME_IDS)
def test_mode_r_camera_frame_vs_oracle(torch_cuda, scene, name):
    rgb, rgb8 = dev_frame(scene, name)
    o = RC.oracle_frame(scene, name)
    exact = _against(rgb, rgb8, o, f"{scene}/{name} vs the oracle")
    g = RC.load_golden(scene)
    if g is not None:
        _against(rgb, rgb8, g[name], f"{scene}/{name} vs the reference's golden")
    hit = o["hit"] >= 0
    print(f"{scene}/{name}: seen {hit.mean():.3f}, {len(np.unique(o['hit'][hit]))} entities, "
          f"{exact * 100:.3f}% pixels bit-identical to the oracle")


def test_default_routes(torch_cuda):
    """What the frames above ran: k_mode_r for the small scenes, the flat phases for the 4100-triangle soup."""
    for scene in RC.SCENES:
        assert dev_scene(scene).r_kernel() == ("k_rf_walk" if scene == "soup4100" else "k_mode_r"), scene


# ---- (b) routes ------------------------------------------------------------------------------------
ROUTES = {   # tag: (environment, gi_scene_r_kernel of a scene whose octree split)
    "k_mode_r": ({"GI_R_FLAT": "0"}, "k_mode_r"),
    "flat": ({"GI_R_FLAT": "1"}, "k_rf_walk"),
    "batch": ({"GI_R_FLAT": "2"}, "k_mode_r_batch"),
    "flat_no_pool": ({"GI_R_FLAT": "1", "GI_RF_PER_SLOT": "0"}, "k_rf_walk"),
}


@pytest.mark.parametrize("route", list(ROUTES))
def test_mode_r_camera_routes_bit_identical(torch_cuda, tmp_path, route):
    """Every placement's frame by each Mode R kernel, forced in a child process, equals this process's
    default route's bit for bit (fp64 and RGB888), so all routes agree with one another.  With no pool
    (GI_RF_PER_SLOT=0) a tile keeps its own 512 candidate pairs: at some soup placement some but not
    all of the frame's tiles overflow to k_mode_r_batch (GI_STAT_R_OVF_TILES)."""
    env, kernel = ROUTES[route]
    out = tmp_path / (route + ".npz")
    subprocess.run([sys.executable, os.path.join(U.ROOT, "tests", "r_cameras.py"), "render", str(out)], check=True,
                   timeout=240, env=dict(os.environ, **env))
    z = np.load(out)
    for scene in RC.SCENES:
        split = dev_scene(scene).info()["n_nodes"] > 1   # (an octree that never split is one leaf: always k_mode_r)
        assert str(z[scene + "/kernel"]) == (kernel if split else "k_mode_r"), scene
    for scene, name in RC.FRAMES:
        rgb, rgb8 = dev_frame(scene, name)
        assert U.bits_equal(rgb, z[f"{scene}/{name}"]).all(), f"{route}: {scene}/{name}"
        assert (rgb8 == z[f"{scene}/{name}/q"]).all(), f"{route}: {scene}/{name} RGB888"
    tiles = gi.shard_tiles(W, H, 1)
    ovf = {f"{s}/{n}": int(z[f"{s}/{n}/stats"][gi.STAT_R_OVF_TILES]) for s, n in RC.FRAMES if s in RC.SOUPS}
    pairs = {f"{s}/{n}": int(z[f"{s}/{n}/stats"][gi.STAT_R_PAIRS]) for s, n in RC.FRAMES if s in RC.SOUPS}
    print(route, "overflowed tiles of", tiles, ovf)
    if route == "flat":
        assert all(v > 0 for v in pairs.values())
    if route == "flat_no_pool":
        assert 0 < ovf["soup4100/" + RC.OVERFLOW_PLACEMENT] < tiles
    if kernel != "k_rf_walk":
        assert all(v == 0 for v in pairs.values())


def test_soup4100_default_route_counts_pairs(torch_cuda):
    """The 4100-triangle soup at default settings runs the flat phases: GI_STAT_R_PAIRS > 0 at every
    placement, and the stats launch renders the same frame."""
    torch = torch_cuda
    d = dev_scene("soup4100")
    assert d.r_kernel() == "k_rf_walk"
    for name, *_ in RC.CAMERAS["soup4100"]:
        cam, light = cam_light("soup4100", name)
        st = torch.zeros(gi.STATS_N, dtype=torch.int64, device="cuda")
        buf = torch.zeros(W * H * 3, dtype=torch.float64, device="cuda")
        d.render_device(cam, light, W, H, buf.data_ptr(), stats_ptr=st.data_ptr())
        torch.cuda.synchronize()
        s = st.cpu().numpy()
        assert s[gi.STAT_R_PAIRS] > 0 and s[gi.STAT_PIXELS] == W * H, name
        assert U.bits_equal(buf.cpu().numpy(), dev_frame("soup4100", name)[0].reshape(-1)).all(), name


# ---- (c) GI_FLAG_R_DFS -------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", RC.SCENES)
def test_mode_r_camera_frames_equal_reverse_dfs(torch_cuda, scene):
    """The reference order walked in full (GI_FLAG_R_DFS, in-process) gives the default's frame bit for bit."""
    d = dev_scene(scene)
    assert d.r_kernel(flags=gi.FLAG_R_DFS) == "k_mode_r"
    for name, *_ in RC.CAMERAS[scene]:
        cam, light = cam_light(scene, name)
        rgb, rgb8 = d.render(cam, light, W, H, flags=gi.FLAG_R_DFS)
        ref, ref8 = dev_frame(scene, name)
        same = U.bits_equal(rgb, ref).all(2)
        assert same.all(), f"{scene}/{name}: {int((~same).sum())} pixels differ from the reverse DFS"
        assert (rgb8 == ref8).all(), f"{scene}/{name} RGB888"


# ---- (d) shards and bands ------------------------------------------------------------------------------
@pytest.mark.parametrize("scene", RC.SCENES)
def test_mode_r_camera_shards_and_bands_equal_whole_frame(torch_cuda, scene):
    torch = torch_cuda
    d = dev_scene(scene)
    n = 3
    per = gi.shard_tiles(W, H, n) * gi.TILE * gi.TILE * 3
    for name in RC.SHARD_PLACEMENTS[scene]:
        cam, light = cam_light(scene, name)
        ref, ref8 = dev_frame(scene, name)
        packed = torch.zeros(n * per, dtype=torch.float64, device="cuda")
        packed8 = torch.zeros(n * per, dtype=torch.uint8, device="cuda")
        for r in range(n):
            d.render_device(cam, light, W, H, packed.data_ptr() + r * per * 8, packed8.data_ptr() + r * per,
                            shard_count=n, shard_index=r)
        out = torch.zeros(H * W * 3, dtype=torch.float64, device="cuda")
        out8 = torch.zeros(H * W * 3, dtype=torch.uint8, device="cuda")
        gi.unshard_device(W, H, n, packed.data_ptr(), packed8.data_ptr(), out.data_ptr(), out8.data_ptr())
        torch.cuda.synchronize()
        assert U.bits_equal(out.cpu().numpy(), ref.reshape(-1)).all(), f"{scene}/{name}: 3 shards"
        assert (out8.cpu().numpy() == ref8.reshape(-1)).all(), f"{scene}/{name}: 3 shards RGB888"
        b, b8 = d.render(cam, light, W, H, band_rows=8)
        assert U.bits_equal(b, ref).all() and (b8 == ref8).all(), f"{scene}/{name}: bands of 8 rows"


# ---- (e) gi_trace_ray --------------------------------------------------------------------------------------
def trace_pixels(o):
    """The pixels of a frame to trace, chosen on the oracle: one hit of every entity seen, up to 16 misses,
    the four corners and the centre, up to 16 hits behind the camera."""
    hit = o["hit"]
    px = [0, W - 1, (H - 1) * W, H * W - 1, (H // 2) * W + W // 2]
    px += [int(np.nonzero(hit == e)[0][0]) for e in np.unique(hit[hit >= 0])]
    for sel in (np.nonzero(hit < 0)[0], np.nonzero((hit >= 0) & (o["t"] < 0))[0]):
        px += [int(sel[k]) for k in np.unique(np.linspace(0, len(sel) - 1, min(16, len(sel))).astype(int))] if len(sel) else []
    return sorted(set(px))


@pytest.mark.parametrize("scene,name", RC.FRAMES, ids=FRAME_IDS)
def test_trace_ray_matches_oracle_pixels(torch_cuda, scene, name):
    """gi_trace_ray with a pixel's UNNORMALISED primary direction (numpy, glm's operation order) is that
    pixel of the oracle's frame: entity and (u, v) exactly, the colour within 1e-5 relative; a miss is
    entity -1 and colour 0.  One call per ray."""
    o = RC.oracle_frame(scene, name)
    sc = RC.scene_at(scene, name)
    d = dev_scene(scene)
    px = trace_pixels(o)
    assert (o["hit"][px] < 0).any() or (o["hit"] >= 0).all()
    got_e, got_uv, got_rgb = [], [], []
    for p in px:
        h, rgb = d.trace_ray(sc.cam_pos, tuple(o["dirs"][p]), sc.light)
        got_e.append(h.entity)
        got_uv.append((h.u, h.v))
        got_rgb.append(rgb)
    got_e, got_uv, got_rgb = np.array(got_e), np.array(got_uv), np.array(got_rgb)
    bad = np.nonzero(got_e != o["hit"][px])[0]
    assert not len(bad), f"{scene}/{name}: pixel {px[bad[0]]} entity {got_e[bad[0]]}, the oracle's {o['hit'][px[bad[0]]]}"
    hit = got_e >= 0
    assert (got_uv[hit] == o["uv"][px][hit]).all(), f"{scene}/{name}: (u, v)"
    assert (got_uv[~hit] == 0).all() and (got_rgb[~hit] == 0).all(), f"{scene}/{name}: a miss is not black"
    assert_rel(got_rgb[hit], o["rgb"][px][hit], f"{scene}/{name} trace_ray colour")
