"""GPU (gfx950): the HIP path through the C-ABI against (a) the golden vectors of the COMPILED
REFERENCE (Mode R) and (b) the CPU oracle on the same seeded inputs (Mode R and Mode X).

Tolerances (north_star: per-pixel error <= 1e-5 relative per channel):
  * Mode R radiance: |gpu - ref| <= 1e-5 * max(|ref|, 1e-300) per channel.  Everything except the
    device's f64 acos/sin/cos/pow is the reference's exact op sequence, so most pixels are
    bit-identical; the count is reported.  RGB888 (Image::setPixel) must match exactly.
  * Mode X radiance: bit-identical to the oracle (only correctly rounded ops, no contraction).
"""
import json
import os
import re
import glob

import numpy as np
import pytest

import oracle_util as U
from x_scenes import grazing_scene as _grazing_scene   # (shared with the flat-leaf and query tests)

pytestmark = pytest.mark.gpu

gi = U.pkg()
S = U.scenes()
GOLD = U.GOLDEN
REL = 1e-5


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    return torch


def _scene(name):
    return S.named_scene(name)


_dev_cache = {}


def dev_scene(name):
    if name not in _dev_cache:
        _dev_cache[name] = gi.DeviceScene.from_scene(_scene(name))
    return _dev_cache[name]


def cam_of(sc):
    return gi.Camera(sc.cam_pos, sc.cam_look, sc.focal)


def assert_rel(gpu, ref, what):
    gpu = np.asarray(gpu, np.float64)
    ref = np.asarray(ref, np.float64)
    err = np.abs(gpu - ref)
    tol = REL * np.maximum(np.abs(ref), 1e-300)
    bad = ~(err <= tol)
    same_nan = np.isnan(gpu) & np.isnan(ref)
    bad &= ~same_nan
    assert not bad.any(), f"{what}: {int(bad.sum())} channels beyond {REL} relative; max rel err " \
                          f"{float(np.nanmax(err / np.maximum(np.abs(ref), 1e-300)))}"


def texel_ub_mask(hit, uv):
    f = np.fmod(uv[:, 0], 32) * 32 + np.fmod(uv[:, 1], 32)
    return (hit >= 0) & ((f < 0) | (f >= 1024))


FRAMES = sorted(os.path.basename(p)[:-4] for p in glob.glob(os.path.join(GOLD, "*.npz"))
                if re.search(r"_\d+x\d+", os.path.basename(p)))


@pytest.mark.parametrize("name", FRAMES)
def test_mode_r_vs_reference_golden(torch_cuda, name):
    z = np.load(os.path.join(GOLD, name + ".npz"))
    meta = json.loads(str(z["meta"]))
    sc = _scene(meta["scene"])
    assert sc.digest() == meta["scene_sha256"]
    w, h = meta["w"], meta["h"]
    rgb, rgb8 = dev_scene(meta["scene"]).render(cam_of(sc), sc.light, w, h)
    g = rgb[z["y"], z["x"]]
    g8 = rgb8[z["y"], z["x"]]
    ok = ~texel_ub_mask(z["hit"], z["uv"])   # texture reads outside the array: reference UB, no claim
    assert int((~ok).sum()) == (154 if name == "only_expsphere_96x96" else 0), "texel-UB pixel count"
    assert_rel(g[ok], z["rgb"][ok], name)
    assert (g8 == z["q"])[ok].all(), f"{name}: {(g8 != z['q'])[ok].any(1).sum()} RGB888 pixels differ"
    if "run_q" in z.files:   # RayTracer::run's own frame
        assert (rgb8 == z["run_q"])[ok.reshape(h, w)].all()
    exact = U.bits_equal(g, z["rgb"]).all(1).mean()
    print(f"{name}: {exact * 100:.3f}% pixels bit-identical to the reference")


@pytest.mark.parametrize("scene", ["cornell", "soup100000"])
def test_mode_r_whole_frame_vs_reference(torch_cuda, scene):
    """R-C3 (Cornell) and R-C4 (the 100k soup) at 1920x1080, EVERY pixel against the compiled
    reference (tests/golden/whole_<scene>_1920x1080.json, make_golden.py `whole`): the RGB888 frame
    (Image::setPixel, image.h:14-16) hashes equal row by row and as a whole -- the exact bar -- and
    each row's fp64 radiance sums per channel agree within 1e-5 relative, its NaN count exactly."""
    g = json.load(open(os.path.join(GOLD, f"whole_{scene}_1920x1080.json")))
    sc = _scene(scene)
    assert sc.digest() == g["scene_sha256"]
    rgb, rgb8 = dev_scene(scene).render(cam_of(sc), sc.light, g["w"], g["h"])
    d = U.whole_frame_digest(rgb, rgb8)
    bad = [y for y in range(g["h"]) if d["row_rgb8_sha256"][y] != g["row_rgb8_sha256"][y]]
    assert not bad, f"{scene}: RGB888 rows differ from the reference: {bad[:10]} ({len(bad)} rows)"
    assert d["rgb8_sha256"] == g["rgb8_sha256"]
    assert d["row_nan"] == g["row_nan"]
    assert_rel(np.array(d["row_sum"]), np.array(g["row_sum"]), f"{scene} row sums")


@pytest.mark.parametrize("scene,w,h", [("zoo", 160, 160), ("only_expsphere", 96, 96), ("only_expcone", 96, 96)])
def test_mode_r_entities_vs_oracle_all_pixels(torch_cuda, scene, w, h):
    """Every pixel, including those whose texel the reference reads out of bounds: the device and
    the oracle both wrap the flat texel index (texture UB), so they must agree."""
    sc = _scene(scene)
    o = U.oracle_render(sc.to_scn(), w, h)
    rgb, rgb8 = dev_scene(scene).render(cam_of(sc), sc.light, w, h)
    assert_rel(rgb.reshape(-1, 3), o["rgb"], scene)
    assert (rgb8.reshape(-1, 3) == o["q"]).all()


def test_mode_r_random_scene_vs_oracle(torch_cuda):
    rng = np.random.default_rng(5)
    s = S.Scene(entities=[])
    for _ in range(8):
        s.imp_sphere(tuple(rng.uniform(-4, 8, 3)), float(rng.uniform(0.5, 3)), tuple(rng.integers(0, 2, 3)))
    for _ in range(60):
        c = rng.uniform(-3, 9, 3)
        v = c + rng.uniform(-2, 2, (3, 3))
        s.imp_triangle(tuple(v[0]), tuple(v[1]), tuple(v[2]), tuple(rng.integers(0, 2, 3)))
    s.exp_quad((1.0, 0.5, -0.5), 3, 2, 0.7, (1, 1, 0))
    w, h = 160, 120
    o = U.oracle_render(s.to_scn(), w, h)
    d = gi.DeviceScene.from_scene(s)
    info = d.info()
    assert info["n_nodes"] > 1   # the octree splits: node tests are exercised
    rgb, rgb8 = d.render(cam_of(s), s.light, w, h)
    assert_rel(rgb.reshape(-1, 3), o["rgb"], "random scene")
    assert (rgb8.reshape(-1, 3) == o["q"]).all()


def test_scene_info_matches_reference_tree(torch_cuda):
    for name in ("cornell", "soup1000", "soup100000", "zoo"):
        st = json.load(open(os.path.join(GOLD, f"tree_{name}.json")))
        info = dev_scene(name).info()
        assert (info["n_nodes"], info["n_leaves"], info["max_depth"], info["n_reachable"]) == \
               (st["n_nodes"], st["n_leaves"], st["max_depth"], st["n_reachable"])


def test_trace_ray_matches_frame(torch_cuda):
    sc = S.cornell_scene()
    z = np.load(os.path.join(GOLD, "cornell_128x128.npz"))
    d = dev_scene("cornell")
    # camera ray of pixel (x, y) exactly as raytracer.h:41 builds it
    c = cam_of(sc)
    pos, up, fwd = np.array(c.pos), np.array(c.up), np.array(c.forward)
    for k in range(0, len(z["x"]), 997):
        x, y = int(z["x"][k]), int(z["y"][k])
        left = np.cross(up, fwd)
        left = left * (1.0 / np.sqrt((left[0] * left[0] + left[1] * left[1]) + left[2] * left[2]))
        # only used as a spot check: the kernel normalises; compare hit entity and colour
        w = 128
        tl = (((pos + c.focalDist * fwd) + ((left * w) * 0.5) * 0.0002) + ((up * w) * 0.5) * 0.0002) - pos
        dirv = (tl - (left * x) * 0.0002) - (up * y) * 0.0002
        hit, rgb = d.trace_ray(c.pos, tuple(dirv), sc.light)
        assert hit.entity == z["hit"][k]
        assert_rel(rgb, z["rgb"][k], f"trace_ray px {x},{y}")


def test_progressive_bands_equal_whole_frame(torch_cuda):
    sc = S.cornell_scene()
    d = dev_scene("cornell")
    a, a8 = d.render(cam_of(sc), sc.light, 200, 136)
    b, b8 = d.render(cam_of(sc), sc.light, 200, 136, band_rows=16)
    assert U.bits_equal(a, b).all() and (a8 == b8).all()
    for spp in (2, 11):   # spp > 1: per-sample radiance rows + in-order reduce, per band
        ax, _ = d.render(cam_of(sc), sc.light, 64, 40, mode=gi.MODE_X, spp=spp, depth=3, seed=9)
        bx, _ = d.render(cam_of(sc), sc.light, 64, 40, mode=gi.MODE_X, spp=spp, depth=3, seed=9, band_rows=8)
        assert U.bits_equal(ax, bx).all()


def _mirror_variants():
    tri = S.cornell_scene()             # triangles only: the 4-wave LDS kernel
    tri.name = "cornell_mirror_tris"
    for e in tri.entities[10:22]:       # short block: half mirror
        e.material.reflectivity = 0.5
    for e in tri.entities[22:34]:       # tall block: mirror
        e.material.reflectivity = 1.0
    soup = S.soup_scene(1000)           # HBM-resident records
    for i, e in enumerate(soup.entities):
        if i % 3 == 0:   # (the soup's entities share one Material object)
            e.material = S.Material((1.0, 1.0, 1.0), reflectivity=0.7)
    return {"cornell_mirror": S.named_scene("cornell_mirror"), "cornell_mirror_tris": tri, "soup1000_mirror": soup}


@pytest.mark.parametrize("name,w,h,spp,depth", [("cornell_mirror", 48, 40, 4, 6), ("cornell_mirror_tris", 40, 40, 3, 8),
                                                 ("soup1000_mirror", 40, 40, 2, 8)])
def test_mode_x_mirror_bounces_bit_exact(torch_cuda, name, w, h, spp, depth):
    """Material reflectivity (Mode X mirror spawn): GPU frames equal the oracle bit for bit,
    and the mirrors change the frame (against the same scene with reflectivity 0)."""
    sc = _mirror_variants()[name]
    o = U.oracle_render(sc.to_scn(), w, h, mode=1, spp=spp, depth=depth, seed=77)
    d = gi.DeviceScene.from_scene(sc)
    rgb, rgb8 = d.render(cam_of(sc), sc.light, w, h, mode=gi.MODE_X, spp=spp, depth=depth, seed=77)
    same = U.bits_equal(rgb.reshape(-1, 3), o["rgb"]).all(1)
    assert same.all(), f"{(~same).sum()} of {same.size} pixels differ from the oracle"
    assert (rgb8.reshape(-1, 3) == o["q"]).all()
    if name.startswith("soup"):
        return   # the white soup's lit pixels saturate at 1 either way
    for e in sc.entities:
        if e.material is not None:
            e.material.reflectivity = 0.0
    plain, _ = gi.DeviceScene.from_scene(sc).render(cam_of(sc), sc.light, w, h, mode=gi.MODE_X, spp=spp, depth=depth,
                                                      seed=77)
    assert not U.bits_equal(plain, rgb).all()


def test_reflectivity_out_of_range_is_a_scene_error(torch_cuda):
    sc = S.cornell_scene()
    sc.entities[0].material.reflectivity = 1.5
    with pytest.raises(gi.GIError, match="-3"):
        gi.DeviceScene.from_scene(sc)


def test_band_pipeline_outputs_and_callbacks(torch_cuda):
    """gi_render's two-slot band pipeline: caller-owned outputs (either one alone), band callbacks
    in row order with the final rows, slot buffers grown between calls, device path equality."""
    import torch
    sc = S.cornell_scene()
    d = dev_scene("cornell")
    cam = cam_of(sc)
    w, h = 96, 75   # ragged last band
    a, a8 = d.render(cam, sc.light, w, h, mode=gi.MODE_X, spp=3, depth=4, seed=5)
    dr = torch.empty(w * h * 3, dtype=torch.float64, device="cuda")
    dr8 = torch.empty(w * h * 3, dtype=torch.uint8, device="cuda")
    d.render_device(cam, sc.light, w, h, dr.data_ptr(), dr8.data_ptr(), mode=gi.MODE_X, spp=3, depth=4, seed=5)
    torch.cuda.synchronize()
    assert U.bits_equal(a.reshape(-1), dr.cpu().numpy()).all() and (a8.reshape(-1) == dr8.cpu().numpy()).all()
    seen = []

    def cb(user, y0, rows, p8, p):
        got8 = np.ctypeslib.as_array(p8, shape=(rows * w * 3,)).copy()
        got = np.ctypeslib.as_array(p, shape=(rows * w * 3,)).copy()
        seen.append((y0, rows, got, got8))

    for band in (8, 16, 24, 0):
        only8 = np.zeros((h, w, 3), np.uint8)
        seen.clear()
        _, r8 = d.render(cam, sc.light, w, h, mode=gi.MODE_X, spp=3, depth=4, seed=5, band_rows=band,
                         out=(None, only8), callback=cb)
        assert r8 is only8 and (only8 == a8).all()
        step = band if band else 80
        assert [s[0] for s in seen] == list(range(0, h, step))
        assert sum(s[1] for s in seen) == h
        for y0, rows, got, got8 in seen:   # callbacks see the final rows (fp64 staged without a caller buffer)
            assert U.bits_equal(got, a[y0:y0 + rows].reshape(-1)).all()
            assert (got8 == a8[y0:y0 + rows].reshape(-1)).all()
        onlyf = np.zeros((h, w, 3), np.float64)
        rf, _ = d.render(cam, sc.light, w, h, mode=gi.MODE_X, spp=3, depth=4, seed=5, band_rows=band, out=(onlyf, None))
        assert rf is onlyf and U.bits_equal(onlyf, a).all()
    big, big8 = d.render(cam, sc.light, 3 * w, 2 * h, band_rows=40)   # slots grow (Mode R)
    whole, whole8 = d.render(cam, sc.light, 3 * w, 2 * h)
    assert U.bits_equal(big, whole).all() and (big8 == whole8).all()


def test_cancel_mid_frame_keeps_delivered_bands(torch_cuda):
    import ctypes
    sc = S.cornell_scene()
    d = dev_scene("cornell")
    cam = cam_of(sc)
    full, full8 = d.render(cam, sc.light, 64, 64)
    flag = ctypes.c_int(0)
    got = []

    def cb(user, y0, rows, p8, p):
        got.append(y0)
        flag.value = 1   # cancel after the first delivered band
    part8 = np.zeros((64, 64, 3), np.uint8)
    with pytest.raises(gi.GIError, match="-4"):
        d.render(cam, sc.light, 64, 64, band_rows=8, cancel=flag, callback=cb, out=(None, part8))
    assert got == [0]
    assert (part8[:8] == full8[:8]).all()
    again, again8 = d.render(cam, sc.light, 64, 64)   # the scene is usable after a cancelled call
    assert U.bits_equal(again, full).all() and (again8 == full8).all()


def test_cancel_before_start(torch_cuda):
    import ctypes
    sc = S.cornell_scene()
    with pytest.raises(gi.GIError, match="-4"):
        dev_scene("cornell").render(cam_of(sc), sc.light, 64, 64, cancel=ctypes.c_int(1))


def test_raytracer_api_matches_run_golden(torch_cuda):
    z = np.load(os.path.join(GOLD, "main_200x200.npz"))
    sc = S.main_scene()
    cam = gi.Camera(sc.cam_pos, sc.cam_look, sc.focal)
    rt = gi.RayTracer(cam, sc.light)
    tree = gi.Octree(sc.octree_min, sc.octree_max)
    tree.push_back(gi.ExpQuad((0.0, 0.0, 0.0), 2, 3, 90.0 * np.pi / 180.0, (1, 2, 3)))
    tree.push_back(gi.ImpSphere((3.0, 4.0, 4.0), 2, (1, 0, 0)))
    tree.push_back(gi.ImpSphere((4.0, -4.0, 4.0), 2, (0, 0, 1)))
    rt.setScene(tree)
    rt.start()
    rt.run(200, 200)
    img = rt.getImage()
    assert img.width() == 200 and img.height() == 200
    assert (img.rgb8 == z["run_q"]).all()


@pytest.mark.parametrize("scene,w,h,spp,depth", [("cornell", 48, 40, 4, 4), ("main", 40, 40, 2, 3),
                                                  ("sphere", 32, 32, 3, 2), ("soup1000", 40, 40, 2, 8),
                                                  ("zoo", 48, 48, 2, 4), ("only_expcone", 32, 32, 2, 3),
                                                  ("only_expsphere", 32, 32, 2, 3), ("only_exprectangle", 32, 32, 1, 2),
                                                  ("only_expcube", 32, 32, 1, 2), ("only_expbox", 32, 32, 1, 2)])
def test_mode_x_bit_exact_vs_oracle(torch_cuda, scene, w, h, spp, depth):
    sc = _scene(scene)
    o = U.oracle_render(sc.to_scn(), w, h, mode=1, spp=spp, depth=depth, seed=2019)
    rgb, rgb8 = dev_scene(scene).render(cam_of(sc), sc.light, w, h, mode=gi.MODE_X, spp=spp, depth=depth, seed=2019)
    same = U.bits_equal(rgb.reshape(-1, 3), o["rgb"]).all(1)
    assert same.all(), f"{(~same).sum()} of {same.size} pixels differ from the oracle"
    assert (rgb8.reshape(-1, 3) == o["q"]).all()


@pytest.mark.parametrize("scene,w,h,spp,depth", [("cornell", 24, 20, 8, 3), ("cornell", 24, 20, 9, 3),
                                                  ("cornell", 21, 13, 17, 4), ("cornell", 16, 16, 64, 8),
                                                  ("zoo", 20, 12, 12, 3), ("soup1000", 16, 16, 24, 5)])
def test_mode_x_spp_runs_bit_exact(torch_cuda, scene, w, h, spp, depth):
    """spp > 1: a pixel's samples are split into runs of k (separate work units on the device, each
    sample's radiance stored and summed in sample order by k_x_reduce); odd spp included."""
    sc = _scene(scene)
    o = U.oracle_render(sc.to_scn(), w, h, mode=1, spp=spp, depth=depth, seed=41)
    rgb, rgb8 = dev_scene(scene).render(cam_of(sc), sc.light, w, h, mode=gi.MODE_X, spp=spp, depth=depth, seed=41)
    same = U.bits_equal(rgb.reshape(-1, 3), o["rgb"]).all(1)
    assert same.all(), f"{(~same).sum()} of {same.size} pixels differ from the oracle"
    assert (rgb8.reshape(-1, 3) == o["q"]).all()


@pytest.mark.parametrize("scene,w,h,spp,depth", [("cornell", 512, 512, 1, 4),          # BASELINE configs[1] (C2)
                                                  ("cornell_mirror", 256, 256, 4, 8)])
def test_mode_x_whole_frame_bit_exact(torch_cuda, scene, w, h, spp, depth):
    """Every pixel of a whole frame against the oracle (C2 is the bench's C2 workload)."""
    sc = _scene(scene)
    o = U.oracle_render(sc.to_scn(), w, h, mode=1, spp=spp, depth=depth, seed=2019, threads=16)
    rgb, rgb8 = dev_scene(scene).render(cam_of(sc), sc.light, w, h, mode=gi.MODE_X, spp=spp, depth=depth, seed=2019)
    same = U.bits_equal(rgb.reshape(-1, 3), o["rgb"]).all(1)
    assert same.all(), f"{(~same).sum()} of {same.size} pixels differ from the oracle"
    assert (rgb8.reshape(-1, 3) == o["q"]).all()
    assert (o["hit"] >= 0).mean() > 0.5


def test_mode_x_multi_sample_units_bit_exact(torch_cuda, tmp_path):
    """GI_X_MAX_RUN=8 (k-sample work units, read once per process: a child process renders) gives
    the same frame bit for bit as the default one-sample units and as the oracle."""
    import subprocess
    import sys
    sc = S.cornell_scene()
    # 512 x 512 x 96 spp: ~90 listed samples per lane of the resident grid, so k = 8 is chosen
    w, h, kw = 512, 512, dict(spp=96, depth=3, seed=11)
    out = tmp_path / "k8.npy"
    code = ("import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r); import oracle_util as U; "
            "gi = U.pkg(); S = U.scenes(); sc = S.cornell_scene(); "
            "d = gi.DeviceScene.from_scene(sc); "
            "rgb, _ = d.render(gi.Camera(sc.cam_pos, sc.cam_look, sc.focal), sc.light, %d, %d, mode=gi.MODE_X, "
            "spp=%d, depth=%d, seed=%d); np.save(%r, rgb)") % (U.ROOT, os.path.join(U.ROOT, "tests"), w, h,
                                                                kw["spp"], kw["depth"], kw["seed"], str(out))
    subprocess.run([sys.executable, "-c", code], check=True, timeout=120, env=dict(os.environ, GI_X_MAX_RUN="8"))
    k8 = np.load(out)
    k1, _ = dev_scene("cornell").render(cam_of(sc), sc.light, w, h, mode=gi.MODE_X, **kw)
    assert U.bits_equal(k8, k1).all()
    win = (240, 300, 264, 316)
    o = U.oracle_render(sc.to_scn(), w, h, mode=1, window=win, **kw)
    assert (o["hit"] >= 0).all()
    assert U.bits_equal(k1[win[1]:win[3], win[0]:win[2]].reshape(-1, 3), o["rgb"]).all()


def _check_rows(sc, f, f8, w, h, spp, depth, seed, row0=0, stride=1, what=""):
    """The device frame's full-width rows row0 + k*stride against the oracle (gio_time_rows, 16 host
    threads: the GPU box's CPU share), bit for bit in fp64 and RGB888; names the first differing rows."""
    o = U.oracle_time_rows(sc.to_scn(), w, h, spp, depth, seed, row0, stride, h, threads=16, pixels=True)
    g, g8 = f[o["rows"]], f8[o["rows"]]
    same = U.bits_equal(g, o["rgb"]).all(2)
    bad = [o["rows"][i] for i in np.nonzero(~same.all(1))[0]]
    assert not bad, f"{what}: {int((~same).sum())} pixels in {len(bad)} rows differ from the oracle (rows {bad[:8]})"
    assert (g8 == o["q"]).all(), f"{what}: RGB888"
    return o


def test_mode_x_c3_config_whole_frame_and_shards(torch_cuda):
    """The bench's own workload: C3 = Cornell 1920x1080, depth 8, 64 spp (single-sample work units by
    default, GI_X_MAX_RUN = 1, for the whole frame and for an 8-way shard of it).  EVERY pixel against
    the oracle bit for bit (round 5 compared three windows, 768 pixels), and the
    8-shard frame against the whole frame bit for bit."""
    torch = torch_cuda
    sc = S.cornell_scene()
    d = dev_scene("cornell")
    w, h, kw = 1920, 1080, dict(mode=gi.MODE_X, spp=64, depth=8, seed=2019)
    full = torch.zeros(w * h * 3, dtype=torch.float64, device="cuda")
    full8 = torch.zeros(w * h * 3, dtype=torch.uint8, device="cuda")
    d.render_device(cam_of(sc), sc.light, w, h, full.data_ptr(), full8.data_ptr(), **kw)
    torch.cuda.synchronize()
    f = full.cpu().numpy().reshape(h, w, 3)
    f8 = full8.cpu().numpy().reshape(h, w, 3)
    o = _check_rows(sc, f, f8, w, h, 64, 8, 2019, what="C3 whole frame")
    assert o["pixels"] == w * h and o["rays"] > 100_000_000
    n = 8
    per = gi.shard_tiles(w, h, n) * gi.TILE * gi.TILE * 3
    packed = torch.zeros(n * per, dtype=torch.float64, device="cuda")
    packed8 = torch.zeros(n * per, dtype=torch.uint8, device="cuda")
    for r in range(n):
        d.render_device(cam_of(sc), sc.light, w, h, packed.data_ptr() + r * per * 8, packed8.data_ptr() + r * per,
                        shard_count=n, shard_index=r, **kw)
    out = torch.zeros_like(full)
    out8 = torch.zeros_like(full8)
    gi.unshard_device(w, h, n, packed.data_ptr(), packed8.data_ptr(), out.data_ptr(), out8.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int64), full.view(torch.int64))
    assert torch.equal(out8, full8)


def test_mode_x_cornell_window_full_depth(torch_cuda):
    # C3 frame (1920x1080, depth 8) on a window, 2 spp: parity at the config's geometry
    sc = S.cornell_scene()
    win = (900, 880, 940, 920)
    o = U.oracle_render(sc.to_scn(), 1920, 1080, mode=1, spp=2, depth=8, seed=1, window=win)
    rgb, _ = dev_scene("cornell").render(cam_of(sc), sc.light, 1920, 1080, mode=gi.MODE_X, spp=2, depth=8, seed=1)
    g = rgb[win[1]:win[3], win[0]:win[2]].reshape(-1, 3)
    assert U.bits_equal(g, o["rgb"]).all()
    assert (o["hit"] >= 0).mean() > 0.5


@pytest.mark.parametrize("n", [2, 3, 8])
@pytest.mark.parametrize("mode,spp,scene", [(gi.MODE_R, 1, "cornell"), (gi.MODE_X, 2, "cornell"),
                                            (gi.MODE_X, 19, "cornell"), (gi.MODE_X, 5, "cornell_mirror")])
def test_sharded_render_equals_single(torch_cuda, n, mode, spp, scene):
    torch = torch_cuda
    sc = _scene(scene)
    d = dev_scene(scene)
    w, h = 203, 117
    kw = dict(mode=mode, spp=spp, depth=4, seed=3) if mode == gi.MODE_X else {}
    full = torch.zeros(h * w * 3, dtype=torch.float64, device="cuda")
    full8 = torch.zeros(h * w * 3, dtype=torch.uint8, device="cuda")
    d.render_device(cam_of(sc), sc.light, w, h, full.data_ptr(), full8.data_ptr(), **kw)
    per = gi.shard_tiles(w, h, n) * gi.TILE * gi.TILE * 3
    packed = torch.zeros(n * per, dtype=torch.float64, device="cuda")
    packed8 = torch.zeros(n * per, dtype=torch.uint8, device="cuda")
    for r in range(n):
        d.render_device(cam_of(sc), sc.light, w, h, packed.data_ptr() + r * per * 8, packed8.data_ptr() + r * per,
                        shard_count=n, shard_index=r, **kw)
    out = torch.zeros_like(full)
    out8 = torch.zeros_like(full8)
    gi.unshard_device(w, h, n, packed.data_ptr(), packed8.data_ptr(), out.data_ptr(), out8.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int64), full.view(torch.int64))
    assert torch.equal(out8, full8)


def test_stats_counters(torch_cuda):
    torch = torch_cuda
    sc = S.cornell_scene()
    d = dev_scene("cornell")
    w, h = 128, 128
    st = torch.zeros(gi.STATS_N, dtype=torch.int64, device="cuda")
    buf = torch.zeros(w * h * 3, dtype=torch.float64, device="cuda")
    d.render_device(cam_of(sc), sc.light, w, h, buf.data_ptr(), stats_ptr=st.data_ptr())
    torch.cuda.synchronize()
    s = st.cpu().numpy()
    assert s[gi.STAT_RAYS] == w * h and s[gi.STAT_PIXELS] == w * h
    z = np.load(os.path.join(GOLD, "cornell_128x128.npz"))
    # reverse-DFS first hit never tests more nodes than the reference's full DFS
    assert 0 < s[gi.STAT_NODES] <= int(z["nnode"].sum())


def test_kernel_timer_ring(torch_cuda):
    # GI_FLAG_TIME (bench's kernel_ms): more timed frames than the 64-pair event ring, the average
    # covers every one, never exceeds the whole render call, and the timed frame is the same frame
    torch = torch_cuda
    sc = S.cornell_scene()
    d = dev_scene("cornell")
    w, h = 96, 64
    kw = dict(mode=gi.MODE_X, spp=4, depth=3, seed=5)
    ref = torch.zeros(w * h * 3, dtype=torch.float64, device="cuda")
    d.render_device(cam_of(sc), sc.light, w, h, ref.data_ptr(), **kw)
    buf = torch.zeros_like(ref)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    n = 70
    e0.record()
    for _ in range(n):
        d.render_device(cam_of(sc), sc.light, w, h, buf.data_ptr(), flags=gi.FLAG_TIME, **kw)
    e1.record()
    ms, cnt = d.kernel_ms()
    torch.cuda.synchronize()
    assert cnt == n
    assert 0.0 < ms <= e0.elapsed_time(e1) / n * 1.05
    assert torch.equal(buf.view(torch.int64), ref.view(torch.int64))
    with pytest.raises(gi.GIError):   # read resets: nothing timed since
        d.kernel_ms()
    d.render_device(cam_of(sc), sc.light, w, h, buf.data_ptr(), flags=gi.FLAG_TIME)   # Mode R
    ms_r, cnt_r = d.kernel_ms()
    assert cnt_r == 1 and ms_r > 0.0


def test_soup100k_full_frame_properties(torch_cuda):
    # C4 at full 1920x1080: the golden window sample above pins values; here the whole frame is
    # rendered and checked for size-independent properties: sharding invariance and determinism.
    torch = torch_cuda
    sc = S.soup_scene(100000)
    d = dev_scene("soup100000")
    w, h = 1920, 1080
    a = torch.zeros(w * h * 3, dtype=torch.float64, device="cuda")
    b = torch.zeros_like(a)
    d.render_device(cam_of(sc), sc.light, w, h, a.data_ptr())
    d.render_device(cam_of(sc), sc.light, w, h, b.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(a.view(torch.int64), b.view(torch.int64))
    assert float(a.max()) <= 1.0 and float(a.min()) >= 0.0


def test_unshard_matches_host_layout(torch_cuda):
    torch = torch_cuda
    from importlib import import_module
    SH = import_module("2019global_amd.shard")
    sc = S.cornell_scene()
    d = dev_scene("cornell")
    w, h, n = 77, 50, 3
    full = torch.zeros(h * w * 3, dtype=torch.float64, device="cuda")
    d.render_device(cam_of(sc), sc.light, w, h, full.data_ptr())
    per = gi.shard_tiles(w, h, n) * 64 * 3
    f = None
    for r in range(n):
        pk = torch.zeros(per, dtype=torch.float64, device="cuda")
        d.render_device(cam_of(sc), sc.light, w, h, pk.data_ptr(), shard_count=n, shard_index=r)
        torch.cuda.synchronize()
        f = full.cpu().numpy().reshape(-1, 3)
        pp = SH.packed_pixels(w, h, n, r)
        got = pk.cpu().numpy().reshape(-1, 3)
        assert U.bits_equal(got[pp >= 0], f[pp[pp >= 0]]).all()
        assert (got[pp < 0] == 0).all()


def test_gpu_run_loads_library_built_from_this_tree(torch_cuda):
    """Provenance on the GPU box: the libgi.so this GPU process loaded was compiled from
    the sources in the tree it runs from (gi_build_id == build.py source_hash)."""
    from importlib import import_module
    assert gi.build_id() == import_module("2019global_amd.build").source_hash()


def test_expbox_node_test_kat_on_device(torch_cuda):
    z = np.load(os.path.join(GOLD, "boxes.npz"))
    got = gi.kat_expbox(z["recs"])
    assert (got == z["hit"]).all(), f"{(got != z['hit']).sum()} node tests differ from the reference"


def test_cpp_dropin_raytracer_matches_reference_run(torch_cuda, tmp_path):
    """The reference app's own classes + include/gi_dropin/raytracer.h (built by integration/Makefile
    where the reference tree exists) give RayTracer::run's frame of the main.cpp scene."""
    import subprocess
    exe = U.dropin_demo()
    out = tmp_path / "f.rgb"
    env = dict(os.environ, QT_QPA_PLATFORM="offscreen")
    subprocess.run([exe, "200", "200", str(out)], check=True, env=env, timeout=120)
    got = np.frombuffer(out.read_bytes(), np.uint8).reshape(200, 200, 3)
    z = np.load(os.path.join(GOLD, "main_200x200.npz"))
    assert (got == z["run_q"]).all()
    # every entity class of entities.h through the drop-in (zoo scene, RayTracer::run's frame)
    subprocess.run([exe, "160", "160", str(out), "zoo"], check=True, env=env, timeout=120)
    got = np.frombuffer(out.read_bytes(), np.uint8).reshape(160, 160, 3)
    z = np.load(os.path.join(GOLD, "zoo_160x160.npz"))
    assert (got == z["run_q"]).all()


@pytest.mark.parametrize("band_env", [{}, {"GI_DEVICES": "0,0"}])
def test_cpp_dropin_raytracer_mode_x_opt_in(torch_cuda, tmp_path, band_env):
    """the north_star integrator through the reference's own boundary.  The
    reference app's classes build the Cornell box (dropin_demo `scn:`), and the drop-in
    RayTracer::run -- opted in by GI_MODE=X / GI_SPP / GI_DEPTH / GI_SEED, read once by its
    constructor -- renders it in Mode X, band by band through Image::setPixel: its fp64 radiance
    equals the oracle's pixel_mode_x bit for bit and its Image is that radiance's RGB888.  Without the
    opt-in the same binary renders the reference's Mode R frame (the default is unchanged).  Also
    over two tile shards (GI_DEVICES=0,0: gi_multi)."""
    import subprocess
    exe = U.dropin_demo()
    sc = S.cornell_scene()
    scn = tmp_path / "c.scn"
    scn.write_text(sc.to_scn())
    w, h, spp, depth, seed = 72, 56, 4, 5, 11
    env = dict(os.environ, QT_QPA_PLATFORM="offscreen", GI_MODE="X", GI_SPP=str(spp), GI_DEPTH=str(depth),
               GI_SEED=str(seed), **band_env)
    out, out8 = tmp_path / "f.f64", tmp_path / "f.rgb"
    subprocess.run([exe, str(w), str(h), str(out), f"scn:{scn}", "rad"], check=True, env=env, timeout=120)
    subprocess.run([exe, str(w), str(h), str(out8), f"scn:{scn}"], check=True, env=env, timeout=120)
    got = np.frombuffer(out.read_bytes(), np.float64).reshape(-1, 3)
    got8 = np.frombuffer(out8.read_bytes(), np.uint8).reshape(-1, 3)
    o = U.oracle_render(sc.to_scn(), w, h, mode=1, spp=spp, depth=depth, seed=seed)
    assert U.bits_equal(got, o["rgb"]).all()
    assert (got8 == o["q"]).all()
    assert (got8 != 0).any()
    # default: the reference's integrator (Mode R) through the same binary
    env_r = {k: v for k, v in env.items() if k not in ("GI_MODE", "GI_SPP", "GI_DEPTH", "GI_SEED")}
    subprocess.run([exe, str(w), str(h), str(out), f"scn:{scn}", "rad"], check=True, env=env_r, timeout=120)
    o_r = U.oracle_render(sc.to_scn(), w, h)
    got_r = np.frombuffer(out.read_bytes(), np.float64).reshape(-1, 3)
    err = np.abs(got_r - o_r["rgb"]) / np.maximum(np.abs(o_r["rgb"]), 1e-300)
    assert float(err.max()) <= 1e-5


def test_cpp_dropin_progressive_passes(torch_cuda, tmp_path):
    """SURVEY §5 (checkpoint/resume: progressive spp): the drop-in RayTracer::run renders a Mode X
    frame's spp in passes (GI_PASS=2 of 8 samples) and delivers each pass's running estimate through
    Image::setPixel.  Stopped after the first pass (stop() from the pass callback, as a Viewer resize
    does), the image holds that pass -- exactly the 2-sample frame of the oracle; run to the end, the
    frame is the 8-sample oracle frame bit for bit, after 4 passes."""
    import subprocess
    exe = U.dropin_demo()
    sc = S.cornell_scene()
    scn = tmp_path / "c.scn"
    scn.write_text(sc.to_scn())
    w, h, spp, depth, seed = 72, 56, 8, 5, 11
    env = dict(os.environ, QT_QPA_PLATFORM="offscreen", GI_MODE="X", GI_SPP=str(spp), GI_DEPTH=str(depth),
               GI_SEED=str(seed), GI_PASS="2")
    out = tmp_path / "f.f64"
    for stop_after, samples, passes in ((1, 2, 1), (0, 8, 4)):
        e = dict(env, DEMO_STOP_AFTER=str(stop_after)) if stop_after else env
        r = subprocess.run([exe, str(w), str(h), str(out), f"scn:{scn}", "rad"], check=True, env=e, timeout=120,
                           capture_output=True, text=True)
        assert f"passes {passes}" in r.stderr, r.stderr
        got = np.frombuffer(out.read_bytes(), np.float64).reshape(-1, 3)
        o = U.oracle_render(sc.to_scn(), w, h, mode=1, spp=samples, depth=depth, seed=seed)
        assert U.bits_equal(got, o["rgb"]).all(), (stop_after, samples)


@pytest.mark.parametrize("name,w,h,spp,depth,passes", [("cornell", 64, 48, 8, 5, (0, 2, 3, 8)),
                                                       ("soup1000", 48, 40, 6, 8, (0, 4, 6)),
                                                       ("zoo", 40, 32, 4, 4, (0, 1, 4))])
def test_mode_x_progressive_passes(torch_cuda, name, w, h, spp, depth, passes):
    """Progressive Mode X passes (gi_opts sample_begin / sample_end, ABI 10): after the pass ending at
    sample e the frame is the e-sample frame bit for bit (jitter and paths do not depend on spp; e > 1),
    and the last pass's frame equals the one-shot spp frame and the oracle's; the three Mode X forms
    alike.  A pass out of order, or after another render of the scene, is refused."""
    sc = _scene(name)
    d = dev_scene(name)
    kw = dict(mode=gi.MODE_X, spp=spp, depth=depth, seed=5)
    for fl in (0, gi.FLAG_X_MEGA, gi.FLAG_X_WF, gi.FLAG_X_SEG):
        for b, e in zip(passes[:-1], passes[1:]):
            rgb, rgb8 = d.render(cam_of(sc), sc.light, w, h, flags=fl, samples=(b, e), **kw)
            if e > 1:
                ref, ref8 = d.render(cam_of(sc), sc.light, w, h, mode=gi.MODE_X, spp=e, depth=depth, seed=5, flags=fl)
                assert U.bits_equal(rgb, ref).all() and (rgb8 == ref8).all(), (name, fl, b, e)
            if e == spp:
                o = U.oracle_render(sc.to_scn(), w, h, mode=1, spp=spp, depth=depth, seed=5)
                assert U.bits_equal(rgb.reshape(-1, 3), o["rgb"]).all(), (name, fl)
            if e > 1 and e < spp:   # (the reference render above ended the progressive frame: resume it)
                d.render(cam_of(sc), sc.light, w, h, flags=fl, samples=(0, e), **kw)
    with pytest.raises(gi.GIError):   # out of order: a frame starts at sample 0
        d.render(cam_of(sc), sc.light, w, h, samples=(passes[1], passes[2]), **kw)
    d.render(cam_of(sc), sc.light, w, h, samples=(0, passes[1]), **kw)
    d.render(cam_of(sc), sc.light, w, h, **kw)   # another render ends the progressive frame
    with pytest.raises(gi.GIError):
        d.render(cam_of(sc), sc.light, w, h, samples=(passes[1], passes[2]), **kw)


@pytest.mark.parametrize("scene,w,h,spp,depth", [("cornell", 37, 29, 3, 5), ("zoo", 45, 19, 2, 4),
                                                  ("main", 13, 61, 1, 3)])
def test_mode_x_ragged_frames_bit_exact(torch_cuda, scene, w, h, spp, depth):
    """Frame sizes that are not multiples of the 8x8 tile: partial tiles, padding slots."""
    sc = _scene(scene)
    o = U.oracle_render(sc.to_scn(), w, h, mode=1, spp=spp, depth=depth, seed=77)
    rgb, rgb8 = dev_scene(scene).render(cam_of(sc), sc.light, w, h, mode=gi.MODE_X, spp=spp, depth=depth, seed=77)
    assert U.bits_equal(rgb.reshape(-1, 3), o["rgb"]).all()
    assert (rgb8.reshape(-1, 3) == o["q"]).all()


@pytest.mark.parametrize("spp", [4, 12])
def test_mode_x_ray_count_equals_oracle(torch_cuda, spp):
    """The bench's rays/frame (GI_FLAG_STATS) is the frame's ray count as the oracle traces it ray by
    ray -- including primary rays the device resolves by its root-box and pixel-frustum tests."""
    torch = torch_cuda
    sc = S.cornell_scene()
    w, h, depth = 96, 64, 6
    o = U.oracle_render(sc.to_scn(), w, h, mode=1, spp=spp, depth=depth, seed=5)
    st = torch.zeros(gi.STATS_N, dtype=torch.int64, device="cuda")
    buf = torch.zeros(w * h * 3, dtype=torch.float64, device="cuda")
    dev_scene("cornell").render_device(cam_of(sc), sc.light, w, h, buf.data_ptr(), stats_ptr=st.data_ptr(),
                                       mode=gi.MODE_X, spp=spp, depth=depth, seed=5)
    torch.cuda.synchronize()
    s = st.cpu().numpy()
    assert int(s[gi.STAT_RAYS]) == int(o["ncand"].sum())
    assert int(s[gi.STAT_PIXELS]) == w * h
    assert U.bits_equal(buf.cpu().numpy().reshape(-1, 3), o["rgb"]).all()


@pytest.mark.parametrize("mode", [0, 1])
def test_empty_scene_and_single_pixel(torch_cuda, mode):
    s = S.Scene(entities=[])
    d = gi.DeviceScene.from_scene(s)
    for w, h in ((1, 1), (9, 3)):
        rgb, rgb8 = d.render(cam_of(s), s.light, w, h, mode=mode, spp=2 if mode else 1, depth=3)
        assert (rgb == 0).all() and (rgb8 == 0).all()


def test_degenerate_triangles_match_oracle(torch_cuda):
    """Zero-area (collinear and repeated-vertex) triangles among ordinary ones, both modes."""
    s = S.Scene(entities=[])
    s.imp_triangle((2.0, -1.0, -1.0), (2.0, 1.0, 1.0), (2.0, 3.0, 3.0), (1, 0, 0))    # collinear
    s.imp_triangle((3.0, 0.5, 0.5), (3.0, 0.5, 0.5), (3.0, -2.0, 1.0), (0, 1, 0))     # repeated vertex
    s.imp_triangle((4.0, -3.0, -3.0), (4.0, 3.0, -3.0), (4.0, 0.0, 3.0), (1, 1, 0))
    s.imp_sphere((6.0, 1.0, 1.0), 1.5, (0, 0, 1))
    d = gi.DeviceScene.from_scene(s)
    w, h = 40, 24
    o = U.oracle_render(s.to_scn(), w, h)
    rgb, rgb8 = d.render(cam_of(s), s.light, w, h)
    assert_rel(rgb.reshape(-1, 3), o["rgb"], "mode R degenerate")
    assert (rgb8.reshape(-1, 3) == o["q"]).all()
    ox = U.oracle_render(s.to_scn(), w, h, mode=1, spp=2, depth=4, seed=9)
    rgb, _ = d.render(cam_of(s), s.light, w, h, mode=gi.MODE_X, spp=2, depth=4, seed=9)
    assert U.bits_equal(rgb.reshape(-1, 3), ox["rgb"]).all()


@pytest.mark.parametrize("scene,w,h", [("main", 200, 200), ("cornell", 256, 160), ("zoo", 160, 160),
                                       ("soup1000", 192, 128), ("sphere", 96, 96), ("only_expbox", 96, 96),
                                       ("only_exprectangle", 96, 96), ("only_expcone", 96, 96)])
def test_mode_r_candidate_reconstruction_equals_reverse_dfs(torch_cuda, scene, w, h):
    """Mode R's default traversal (candidate reconstruction from the line BVH) against the reference
    order walked in full (GI_FLAG_R_DFS): the same frame bit for bit, fp64 and RGB888."""
    torch = torch_cuda
    sc = _scene(scene)
    d = dev_scene(scene)
    out = []
    for flags in (0, gi.FLAG_R_DFS):
        a = torch.zeros(w * h * 3, dtype=torch.float64, device="cuda")
        a8 = torch.zeros(w * h * 3, dtype=torch.uint8, device="cuda")
        d.render_device(cam_of(sc), sc.light, w, h, a.data_ptr(), a8.data_ptr(), flags=flags)
        out.append((a, a8))
    torch.cuda.synchronize()
    assert torch.equal(out[0][0].view(torch.int64), out[1][0].view(torch.int64))
    assert torch.equal(out[0][1], out[1][1])


def test_mode_r_soup100k_frame_equals_reverse_dfs(torch_cuda):
    """C4's scene in Mode R (100k triangles, 59% of them lost by the reference octree): the whole
    1920x1080 frame by candidate reconstruction equals the full reverse-DFS frame bit for bit."""
    torch = torch_cuda
    sc = S.soup_scene(100000)
    d = dev_scene("soup100000")
    w, h = 1920, 1080
    out = []
    for flags in (0, gi.FLAG_R_DFS):
        a = torch.zeros(w * h * 3, dtype=torch.float64, device="cuda")
        d.render_device(cam_of(sc), sc.light, w, h, a.data_ptr(), flags=flags)
        out.append(a)
    torch.cuda.synchronize()
    assert torch.equal(out[0].view(torch.int64), out[1].view(torch.int64))


def _render_frame_device(torch, scene, w, h, **kw):
    sc = _scene(scene)
    d = dev_scene(scene)
    rgb = torch.zeros(w * h * 3, dtype=torch.float64, device="cuda")
    rgb8 = torch.zeros(w * h * 3, dtype=torch.uint8, device="cuda")
    d.render_device(cam_of(sc), sc.light, w, h, rgb.data_ptr(), rgb8.data_ptr(), **kw)
    torch.cuda.synchronize()
    return rgb, rgb8


def _check_windows(sc, frame, frame8, w, h, wins, spp, depth, seed, min_hit=None):
    """Device frame windows against the oracle, bit for bit (fp64 and RGB888)."""
    hits = 0
    for win in wins:
        o = U.oracle_render(sc.to_scn(), w, h, mode=1, spp=spp, depth=depth, seed=seed, window=win, threads=16)
        g = frame[win[1]:win[3], win[0]:win[2]].reshape(-1, 3)
        g8 = frame8[win[1]:win[3], win[0]:win[2]].reshape(-1, 3)
        same = U.bits_equal(g, o["rgb"]).all(1)
        assert same.all(), f"window {win}: {(~same).sum()} of {same.size} pixels differ from the oracle"
        assert (g8 == o["q"]).all(), f"window {win}: RGB888"
        hits += int((o["hit"] >= 0).sum())
    if min_hit is not None:
        assert hits >= min_hit
    return hits


def test_mode_x_c4_config_whole_frame(torch_cuda):
    """BASELINE configs[3] (C4): the 100k-triangle soup at 1920x1080, depth 8, Mode X, whole frame on
    the device; EVERY pixel against the oracle bit for bit, plus a window at the
    soup's centre (the frame's longest paths: pixel (960, 960) looks along +x through the soup's core,
    raytracer.h:26-30 with A.12) that must hold hits."""
    torch = torch_cuda
    sc = S.soup_scene(100000)
    w, h, kw = 1920, 1080, dict(mode=gi.MODE_X, spp=1, depth=8, seed=2019)
    rgb, rgb8 = _render_frame_device(torch, "soup100000", w, h, **kw)
    f = rgb.cpu().numpy().reshape(h, w, 3)
    f8 = rgb8.cpu().numpy().reshape(h, w, 3)
    _check_rows(sc, f, f8, w, h, 1, 8, 2019, what="C4 whole frame")
    _check_windows(sc, f, f8, w, h, ((952, 952, 968, 968),), 1, 8, 2019, min_hit=200)
    assert float(f.max()) <= 1.0 and float(f.min()) >= 0.0


def test_mode_x_c5_config_rows_and_8_shards(torch_cuda):
    """BASELINE configs[4] (C5): the 100k soup at 3840x2160, depth 8, 256 spp -- the whole frame on
    one device, every 16th row against the oracle bit for bit, and the 8-way tile-sharded frame (the
    config's 8-GPU split, rendered shard by shard here) equal to the single frame bit for bit."""
    torch = torch_cuda
    sc = S.soup_scene(100000)
    d = dev_scene("soup100000")
    w, h, kw = 3840, 2160, dict(mode=gi.MODE_X, spp=256, depth=8, seed=2019)
    full, full8 = _render_frame_device(torch, "soup100000", w, h, **kw)
    f = full.cpu().numpy().reshape(h, w, 3)
    f8 = full8.cpu().numpy().reshape(h, w, 3)
    # every 16th full-width row (135 rows = 518,400 pixels x 256 spp; rows 1908 and 1924 cross the
    # soup's core), bit for bit against the oracle (round 5 compared 256 pixels)
    _check_rows(sc, f, f8, w, h, 256, 8, 2019, row0=4, stride=16, what="C5 strided rows")
    _check_windows(sc, f, f8, w, h, ((1916, 1916, 1924, 1924),), 256, 8, 2019, min_hit=50)
    n = 8
    per = gi.shard_tiles(w, h, n) * gi.TILE * gi.TILE * 3
    packed = torch.zeros(n * per, dtype=torch.float64, device="cuda")
    packed8 = torch.zeros(n * per, dtype=torch.uint8, device="cuda")
    for r in range(n):
        d.render_device(cam_of(sc), sc.light, w, h, packed.data_ptr() + r * per * 8, packed8.data_ptr() + r * per,
                        shard_count=n, shard_index=r, **kw)
    out = torch.zeros_like(full)
    out8 = torch.zeros_like(full8)
    gi.unshard_device(w, h, n, packed.data_ptr(), packed8.data_ptr(), out.data_ptr(), out8.data_ptr())
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int64), full.view(torch.int64))
    assert torch.equal(out8, full8)


@pytest.mark.parametrize("spec_pow", [5.5, 0.25, 100.0, 64.0])
def test_mode_x_non_integer_specular_power(torch_cuda, spec_pow):
    """Material::specular_power is any double (material.h:29): Mode X's mx_pow (exp/ln series for a
    non-integer or > 64 power) is bit-identical between the device and the oracle."""
    import dataclasses
    s = S.cornell_scene()
    changed = 0
    for e in s.entities:
        if e.material is not None:
            e.material = dataclasses.replace(e.material, specular_power=spec_pow)
            changed += 1
    assert changed > 0
    d = gi.DeviceScene.from_scene(s)
    w, h = 48, 40
    o = U.oracle_render(s.to_scn(), w, h, mode=1, spp=2, depth=4, seed=3)
    rgb, rgb8 = d.render(cam_of(s), s.light, w, h, mode=gi.MODE_X, spp=2, depth=4, seed=3)
    assert U.bits_equal(rgb.reshape(-1, 3), o["rgb"]).all()
    assert (rgb8.reshape(-1, 3) == o["q"]).all()


# ---- several GPUs through the C-ABI (gi_multi_*) -------------------------------------------------
@pytest.mark.parametrize("devices", [[0], [0, 0], [0, 0, 0]])
def test_multi_render_equals_single_device(torch_cuda, devices):
    """gi_multi_render (tile shards over the listed devices, gathered to devices[0]) against
    gi_render on one device, bit for bit: Mode R with progressive bands, Mode X with spp > 1.  On a
    one-GPU box the shards share device 0 (the RCCL route is tested separately, below)."""
    sc = S.cornell_scene()
    single = dev_scene("cornell")
    m = gi.MultiScene.from_scene(sc, devices)
    assert m.info() == {"shards": len(devices), "devices": 1, "rccl": False}
    w, h = 203, 117
    for kw in (dict(mode=gi.MODE_R, band_rows=24), dict(mode=gi.MODE_X, spp=3, depth=4, seed=9)):
        a, a8 = single.render(cam_of(sc), sc.light, w, h, **kw)
        b, b8 = m.render(cam_of(sc), sc.light, w, h, **kw)
        assert U.bits_equal(a, b).all(), kw
        assert (a8 == b8).all(), kw
    m.close()


def test_multi_render_through_rccl(torch_cuda, tmp_path):
    """The RCCL gather itself (ncclCommInitAll + a group of ncclSend/ncclRecv, rccl.h:236, 700-725):
    GI_MULTI_RCCL=1 routes every shard through RCCL even on one device (rank 0 sends to itself), in
    a child process with its own time limit.  The frame equals the one-device frame bit for bit."""
    import subprocess
    import sys
    sc = S.cornell_scene()
    w, h = 160, 96
    out = tmp_path / "m.npy"
    code = ("import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r); import oracle_util as U; "
            "gi = U.pkg(); S = U.scenes(); sc = S.cornell_scene(); "
            "m = gi.MultiScene.from_scene(sc, [0, 0]); info = m.info(); assert info['rccl'], info; "
            "rgb, rgb8 = m.render(gi.Camera(sc.cam_pos, sc.cam_look, sc.focal), sc.light, %d, %d, mode=gi.MODE_X, "
            "spp=2, depth=3, seed=4, band_rows=48); np.save(%r, rgb); m.close(); print('rccl ok', info)"
            ) % (U.ROOT, os.path.join(U.ROOT, "tests"), w, h, str(out))
    r = subprocess.run([sys.executable, "-c", code], timeout=180, capture_output=True, text=True,
                       env=dict(os.environ, GI_MULTI_RCCL="1", NCCL_DEBUG="WARN"))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    got = np.load(out)
    ref, _ = dev_scene("cornell").render(cam_of(sc), sc.light, w, h, mode=gi.MODE_X, spp=2, depth=3, seed=4)
    assert U.bits_equal(got, ref).all()


def test_cpp_dropin_multi_device_matches_reference_run(torch_cuda, tmp_path):
    """The drop-in RayTracer with GI_DEVICES=0,0 (two tile shards through gi_multi) still gives
    RayTracer::run's frame of the main.cpp scene."""
    import subprocess
    exe = U.dropin_demo()
    out = tmp_path / "f.rgb"
    env = dict(os.environ, QT_QPA_PLATFORM="offscreen", GI_DEVICES="0,0")
    subprocess.run([exe, "200", "200", str(out)], check=True, env=env, timeout=120)
    got = np.frombuffer(out.read_bytes(), np.uint8).reshape(200, 200, 3)
    z = np.load(os.path.join(GOLD, "main_200x200.npz"))
    assert (got == z["run_q"]).all()


def test_renders_on_two_streams_are_ordered(torch_cuda):
    """One scene, a Mode X gi_render_device on a side stream immediately followed by gi_render on
    the scene's own stream (they share the scene's work list): the library orders them, both frames
    are right (per-scene launches ordered by an event)."""
    torch = torch_cuda
    sc = S.cornell_scene()
    d = gi.DeviceScene.from_scene(sc)
    w, h, kw = 160, 120, dict(mode=gi.MODE_X, spp=4, depth=4, seed=21)
    ref, _ = d.render(cam_of(sc), sc.light, w, h, **kw)
    side = torch.cuda.Stream()
    buf = torch.zeros(w * h * 3, dtype=torch.float64, device="cuda")
    for _ in range(3):
        d.render_device(cam_of(sc), sc.light, w, h, buf.data_ptr(), stream=side.cuda_stream, **kw)
        host, _ = d.render(cam_of(sc), sc.light, w, h, mode=gi.MODE_X, spp=2, depth=3, seed=5)
    side.synchronize()
    assert U.bits_equal(buf.cpu().numpy().reshape(h, w, 3), ref).all()
    o = U.oracle_render(sc.to_scn(), w, h, mode=1, spp=2, depth=3, seed=5)
    assert U.bits_equal(host.reshape(-1, 3), o["rgb"]).all()


def test_python_raytracer_sees_push_back_after_first_run(torch_cuda):
    """RayTracer.run reads the live octree (raytracer.h:45): an entity pushed after the first run
    appears in the next frame (the scene is re-uploaded when Octree.generation changes)."""
    sc = S.main_scene()
    rt = gi.RayTracer(gi.Camera(sc.cam_pos, sc.cam_look, sc.focal), sc.light)
    tree = gi.Octree(sc.octree_min, sc.octree_max)
    tree.push_back(gi.ImpSphere((5.0, 0.0, 0.0), 1, (1, 0, 0)))
    rt.setScene(tree)
    rt.start()
    rt.run(64, 64)
    a = rt.getImage().rgb8.copy()
    assert a.any()
    tree.push_back(gi.ImpSphere((2.0, 0.3, 0.3), 0.3, (0, 0, 1)))
    rt.start()
    rt.run(64, 64)
    b = rt.getImage().rgb8
    assert (a != b).any()
    s2 = S.Scene(entities=[])
    s2.imp_sphere((5.0, 0.0, 0.0), 1, (1, 0, 0))
    s2.imp_sphere((2.0, 0.3, 0.3), 0.3, (0, 0, 1))
    o = U.oracle_render(s2.to_scn(), 64, 64)
    assert (b.reshape(-1, 3) == o["q"]).all()


@pytest.mark.parametrize("name", sorted(U.ANCHOR))
def test_reduced_mode_x_anchored_to_reference_on_device(torch_cuda, name):
    """the DEVICE's Mode X stages tied to the compiled reference's frames where
    the semantics coincide -- depth 1, 1 spp, no shadow rays (GI_FLAG_X_NO_SHADOW).  The device frame
    equals the oracle's reduced frame bit for bit, and against the reference fixture the excluded
    pixels are exactly the counted classes of oracle_util.ANCHOR (A.1/A.6 entity choice, texel
    edges, fp32 sphere roots); every other pixel is within 1e-5 relative per channel."""
    z = np.load(os.path.join(GOLD, name + ".npz"))
    meta = json.loads(str(z["meta"]))
    sc = _scene(meta["scene"])
    w, h = meta["w"], meta["h"]
    rgb, _ = dev_scene(meta["scene"]).render(cam_of(sc), sc.light, w, h, mode=gi.MODE_X, spp=1, depth=1,
                                             flags=gi.FLAG_X_NO_SHADOW)
    g = rgb[z["y"], z["x"]]
    xs, ys = z["x"], z["y"]
    x0, x1, y0, y1 = int(xs.min()), int(xs.max()) + 1, int(ys.min()), int(ys.max()) + 1
    U.oracle_no_shadow(True)
    try:
        o = U.oracle_render(sc.to_scn(), w, h, mode=1, spp=1, depth=1, window=(x0, y0, x1, y1))
    finally:
        U.oracle_no_shadow(False)
    i = (ys - y0) * (x1 - x0) + (xs - x0)
    assert U.bits_equal(g, o["rgb"][i]).all(), "device reduced Mode X differs from the oracle's"
    ent, tex, far, exact, far_max = U.anchor_counts(g, o["hit"][i], o["uv"][i], z)
    assert (ent, tex, far, exact) == U.ANCHOR[name]
    assert far_max <= U.ANCHOR_ABS
    print(f"{name}: {exact} of {len(xs)} pixels bit-identical to the reference")


def test_mode_x_shadow_handoff_frame_identical(torch_cuda, tmp_path):
    """Shadow rays handed to idle lanes (GI_X_HELP, chosen for small launches of k_mode_x such as the
    whole C4 frame) change the schedule only: the frame equals the one rendered without the handoff
    (GI_X_HELP=0, read once per process: a child process renders) bit for bit, for the C4 workload
    and for the 1k soup at 4 spp (whose tree is small enough for k_seg by default: k_mode_x is forced
    in both processes, so that the two handoff builds are what is compared)."""
    import subprocess
    import sys
    cases = (("soup100000", 1920, 1080, 1, 8, 0), ("soup1000", 320, 240, 4, 6, gi.FLAG_X_MEGA))
    out = tmp_path / "nohelp.npz"
    code = ("import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r); import oracle_util as U; "
            "gi = U.pkg(); S = U.scenes(); res = {}\n"
            "for name, w, h, spp, depth, flags in %r:\n"
            "    sc = S.named_scene(name); d = gi.DeviceScene.from_scene(sc)\n"
            "    res[name] = d.render(gi.Camera(sc.cam_pos, sc.cam_look, sc.focal), sc.light, w, h, mode=gi.MODE_X, "
            "spp=spp, depth=depth, seed=2019, flags=flags)[0]\n"
            "np.savez(%r, **res)") % (U.ROOT, os.path.join(U.ROOT, "tests"), cases, str(out))
    subprocess.run([sys.executable, "-c", code], check=True, timeout=300, env=dict(os.environ, GI_X_HELP="0"))
    ref = np.load(out)
    for name, w, h, spp, depth, flags in cases:
        sc = _scene(name)
        rgb, _ = dev_scene(name).render(cam_of(sc), sc.light, w, h, mode=gi.MODE_X, spp=spp, depth=depth, seed=2019,
                                        flags=flags)
        assert U.bits_equal(rgb, ref[name]).all(), name


@pytest.mark.parametrize("kernel", ["1", "2"])
def test_mode_r_large_scene_kernels_on_small_scenes(torch_cuda, tmp_path, kernel):
    """The Mode R kernels for scenes of more than 4096 entities -- the flat phases (GI_R_FLAT=1) and
    the 8-lanes-per-pixel fallback k_mode_r_batch over the whole frame (GI_R_FLAT=2), forced onto the
    small scenes (read once per process: a child process renders) -- give the same frames bit for
    bit as k_mode_r's one lane per pixel: spheres (tested by every ray), all entity classes, and the
    sharded packed layout."""
    import subprocess
    import sys
    cases = (("main", 200, 200, 1), ("zoo", 160, 160, 1), ("cornell", 128, 128, 1), ("soup1000", 160, 160, 3))
    out = tmp_path / "split.npz"
    code = ("import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r); import oracle_util as U; "
            "import torch; gi = U.pkg(); S = U.scenes(); res = {}\n"
            "for name, w, h, n in %r:\n"
            "    sc = S.named_scene(name); d = gi.DeviceScene.from_scene(sc)\n"
            "    cam = gi.Camera(sc.cam_pos, sc.cam_look, sc.focal)\n"
            "    res[name] = d.render(cam, sc.light, w, h)[0]\n"
            "    if n > 1:\n"
            "        per = gi.shard_tiles(w, h, n) * gi.TILE * gi.TILE * 3\n"
            "        p = torch.zeros(n * per, dtype=torch.float64, device='cuda')\n"
            "        for r in range(n): d.render_device(cam, sc.light, w, h, p.data_ptr() + r * per * 8, 0, shard_count=n, shard_index=r)\n"
            "        torch.cuda.synchronize(); res[name + '_packed'] = p.cpu().numpy()\n"
            "np.savez(%r, **res)") % (U.ROOT, os.path.join(U.ROOT, "tests"), cases, str(out))
    subprocess.run([sys.executable, "-c", code], check=True, timeout=300, env=dict(os.environ, GI_R_FLAT=kernel))
    ref = np.load(out)
    torch = torch_cuda
    for name, w, h, n in cases:
        sc = _scene(name)
        d = dev_scene(name)
        rgb, _ = d.render(cam_of(sc), sc.light, w, h)
        assert U.bits_equal(rgb, ref[name]).all(), name
        if n > 1:
            per = gi.shard_tiles(w, h, n) * gi.TILE * gi.TILE * 3
            p = torch.zeros(n * per, dtype=torch.float64, device="cuda")
            for r in range(n):
                d.render_device(cam_of(sc), sc.light, w, h, p.data_ptr() + r * per * 8, 0, shard_count=n, shard_index=r)
            torch.cuda.synchronize()
            assert U.bits_equal(p.cpu().numpy(), ref[name + "_packed"]).all(), name + " packed"


@pytest.mark.parametrize("group", ["1", "4"])
def test_mode_r_reach_lane_groups_bit_exact(torch_cuda, tmp_path, group):
    """k_rf_reach with one lane per hit (GI_RF_GROUP=1) or four (GI_RF_GROUP=4: the 12 ExpBox faces of
    a node test split over the hit's lanes, OR-ed by a ballot), forced in a child process on launches
    the default gives to the other: the 100k soup's whole 1080p frame (266 k hits, default 1) and its
    8 shards (~33 k hits each, default 4), and the one-tile-column strip -- bit for bit the frames of
    the default choice."""
    import subprocess
    import sys
    w, h, n = 1920, 1080, 8
    strip = tmp_path / "strip.scn"
    strip.write_text(_strip_scene(size=0.3).to_scn())
    out = tmp_path / "groups.npz"
    code = ("import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r); import oracle_util as U; "
            "import torch; gi = U.pkg(); S = U.scenes(); res = {}\n"
            "sc = S.named_scene('soup100000'); d = gi.DeviceScene.from_scene(sc)\n"
            "cam = gi.Camera(sc.cam_pos, sc.cam_look, sc.focal)\n"
            "res['full'] = d.render(cam, sc.light, %d, %d)[0]\n"
            "per = gi.shard_tiles(%d, %d, %d) * gi.TILE * gi.TILE * 3\n"
            "p = torch.zeros(%d * per, dtype=torch.float64, device='cuda')\n"
            "for r in range(%d): d.render_device(cam, sc.light, %d, %d, p.data_ptr() + r * per * 8, 0, shard_count=%d, shard_index=r)\n"
            "torch.cuda.synchronize(); res['packed'] = p.cpu().numpy()\n"
            "st = S.parse_scn(open(%r).read()); ds = gi.DeviceScene.from_scene(st)\n"
            "res['strip'] = ds.render(gi.Camera(st.cam_pos, st.cam_look, st.focal), st.light, 2048, 1088)[0]\n"
            "np.savez(%r, **res)") % (U.ROOT, os.path.join(U.ROOT, "tests"), w, h, w, h, n, n, n, w, h, n, str(strip), str(out))
    subprocess.run([sys.executable, "-c", code], check=True, timeout=300, env=dict(os.environ, GI_RF_GROUP=group))
    ref = np.load(out)
    torch = torch_cuda
    sc = _scene("soup100000")
    d = dev_scene("soup100000")
    assert d.r_kernel() == "k_rf_walk"
    rgb, _ = d.render(cam_of(sc), sc.light, w, h)
    assert U.bits_equal(rgb, ref["full"]).all(), "whole frame"
    per = gi.shard_tiles(w, h, n) * gi.TILE * gi.TILE * 3
    p = torch.zeros(n * per, dtype=torch.float64, device="cuda")
    for r in range(n):
        d.render_device(cam_of(sc), sc.light, w, h, p.data_ptr() + r * per * 8, 0, shard_count=n, shard_index=r)
    torch.cuda.synchronize()
    assert U.bits_equal(p.cpu().numpy(), ref["packed"]).all(), "8 shards"
    st = _strip_scene(size=0.3)
    ds = gi.DeviceScene.from_scene(st)
    rs, _ = ds.render(cam_of(st), st.light, 2048, 1088)
    assert U.bits_equal(rs, ref["strip"]).all(), "strip"


@pytest.mark.parametrize("light_mode", ["floor", "tilted"])
def test_mode_x_own_plane_skip_grazing_light(torch_cuda, light_mode):
    """The own-plane leaf skip (gi_build.cpp assign_plane_groups) with the light almost in a
    surface's plane: the shadow rays leaving that surface graze it, fall below the skip's incidence
    bound and are traced in full; every other ray may skip its own plane.  Mode X frames (k_seg, the
    default form for this LDS-resident scene) bit for bit equal the oracle's, which never skips."""
    sc = _grazing_scene(light_mode)
    d = gi.DeviceScene.from_scene(sc)
    assert d.x_form(spp=4, depth=6) == "k_seg"
    w, h, spp, depth = 96, 64, 4, 6
    rgb, _ = d.render(cam_of(sc), sc.light, w, h, mode=gi.MODE_X, spp=spp, depth=depth, seed=3)
    o = U.oracle_render(sc.to_scn(), w, h, mode=1, spp=spp, depth=depth, seed=3)
    same = U.bits_equal(rgb.reshape(-1, 3), o["rgb"]).all(1)
    assert same.all(), f"{int((~same).sum())} of {same.size} pixels differ"
    assert (o["rgb"] > 0).any()


@pytest.mark.parametrize("accel", [{"GI_XACCEL": "octree"}, {"GI_XLEAF_MAX": "1"}, {"GI_XSBVH": "1"}])
def test_mode_x_other_acceleration_structures_bit_exact(torch_cuda, accel):
    """Mode X over the SAT octree (GI_XACCEL=octree: up to 12 levels, so the kernel keeps its two-word
    level masks), over a BVH of single-primitive leaves (GI_XLEAF_MAX=1) and over the spatial-split
    BVH forced onto these small scenes (GI_XSBVH=1: triangles cut by planes, a primitive in several
    leaves; the 100k soup uses it by default), all read when the scene is built: frames equal the
    oracle's bit for bit -- the result does not depend on the acceleration structure."""
    old = {k: os.environ.get(k) for k in accel}
    os.environ.update(accel)
    try:
        devs = {name: gi.DeviceScene.from_scene(_scene(name)) for name in ("cornell", "soup1000")}
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    for name, (w, h, spp, depth) in (("cornell", (48, 40, 3, 5)), ("soup1000", (64, 48, 2, 8))):
        sc = _scene(name)
        rgb, _ = devs[name].render(cam_of(sc), sc.light, w, h, mode=gi.MODE_X, spp=spp, depth=depth, seed=7)
        o = U.oracle_render(sc.to_scn(), w, h, mode=1, spp=spp, depth=depth, seed=7)
        assert U.bits_equal(rgb.reshape(-1, 3), o["rgb"]).all(), (name, accel)


@pytest.mark.parametrize("name,w,h,spp,depth,shard", [
    ("cornell", 96, 80, 16, 8, (1, 0)), ("cornell_mirror", 64, 48, 4, 8, (3, 1)), ("zoo", 64, 48, 2, 4, (1, 0)),
    ("main", 80, 60, 3, 5, (1, 0)), ("soup1000", 64, 64, 2, 8, (2, 1)), ("sphere", 40, 40, 5, 3, (1, 0))])
def test_mode_x_forms_bit_identical(torch_cuda, name, w, h, spp, depth, shard):
    """The three Mode X forms -- the persistent path-state kernel (k_mode_x), the wavefront form (one
    k_wf_bounce launch per bounce over ballot-compacted path queues) and the segment-synchronous form
    (k_seg) -- run the same per-path operations, so every frame is bit-identical across them and to
    the oracle (LDS- and HBM-resident scenes, mirrors, spheres, a packed shard; gi_scene_x_form names
    the form each flag selects)."""
    sc = _scene(name)
    d = dev_scene(name)
    kw = dict(mode=gi.MODE_X, spp=spp, depth=depth, seed=7)
    frames = {}
    for form, fl in (("k_mode_x", gi.FLAG_X_MEGA), ("k_wf_bounce", gi.FLAG_X_WF), ("k_seg", gi.FLAG_X_SEG)):
        assert d.x_form(gi.MODE_X, spp, depth, flags=fl) == form
        if shard[0] == 1:
            frames[form] = d.render(cam_of(sc), sc.light, w, h, flags=fl, **kw)
        else:
            torch = torch_cuda
            n = gi.shard_tiles(w, h, shard[0]) * 64 * 3
            buf = torch.zeros(n, dtype=torch.float64, device="cuda")
            buf8 = torch.zeros(n, dtype=torch.uint8, device="cuda")
            d.render_device(cam_of(sc), sc.light, w, h, buf.data_ptr(), buf8.data_ptr(), shard_count=shard[0],
                            shard_index=shard[1], flags=fl, **kw)
            torch.cuda.synchronize()
            frames[form] = (buf.cpu().numpy(), buf8.cpu().numpy())
    for form in ("k_wf_bounce", "k_seg"):
        assert U.bits_equal(frames[form][0], frames["k_mode_x"][0]).all(), form
        assert (frames[form][1] == frames["k_mode_x"][1]).all(), form
    if shard[0] == 1:
        o = U.oracle_render(sc.to_scn(), w, h, mode=1, spp=spp, depth=depth, seed=7)
        assert U.bits_equal(frames["k_seg"][0].reshape(-1, 3), o["rgb"]).all()


def test_mode_r_kernels_frame_identical(torch_cuda, tmp_path):
    """The Mode R kernels for large scenes render the whole R-C4 frame (the 100k soup, 1920x1080) and
    a 2-way sharded, packed 480x270 frame of it bit for bit alike: the flat phases (default), the
    fallback k_mode_r_batch over the whole frame (GI_R_FLAT=2), and the flat phases with no pool
    (GI_RF_PER_SLOT=0: every tile with more than its own 512 candidate pairs overflows and only those
    tiles are rendered by k_mode_r_batch -- counted in GI_STAT_R_OVF_TILES, some but not all).  Read
    once per process: child processes render."""
    import subprocess
    import sys
    code = ("import sys, numpy as np, torch; sys.path.insert(0, %r); sys.path.insert(0, %r); import oracle_util as U; "
            "gi = U.pkg(); S = U.scenes(); res = {}\n"
            "sc = S.named_scene('soup100000'); d = gi.DeviceScene.from_scene(sc)\n"
            "cam = gi.Camera(sc.cam_pos, sc.cam_look, sc.focal)\n"
            "res['c4'] = d.render(cam, sc.light, 1920, 1080)[0]\n"
            "st = torch.zeros(gi.STATS_N, dtype=torch.int64, device='cuda')\n"
            "buf = torch.zeros(1920 * 1080 * 3, dtype=torch.float64, device='cuda')\n"
            "d.render_device(cam, sc.light, 1920, 1080, buf.data_ptr(), 0, stats_ptr=st.data_ptr())\n"
            "torch.cuda.synchronize(); res['stats'] = st.cpu().numpy(); res['c4_stats'] = buf.cpu().numpy()\n"
            "per = gi.shard_tiles(480, 270, 2) * gi.TILE * gi.TILE * 3\n"
            "p = torch.zeros(2 * per, dtype=torch.float64, device='cuda')\n"
            "for r in range(2): d.render_device(cam, sc.light, 480, 270, p.data_ptr() + r * per * 8, 0, shard_count=2, shard_index=r)\n"
            "torch.cuda.synchronize(); res['packed'] = p.cpu().numpy()\n"
            "np.savez(sys.argv[1], **res)") % (U.ROOT, os.path.join(U.ROOT, "tests"))
    frames = {}
    for tag, env in (("flat", {}), ("batch", {"GI_R_FLAT": "2"}), ("flat_overflow", {"GI_RF_PER_SLOT": "0"})):
        out = tmp_path / (tag + ".npz")
        subprocess.run([sys.executable, "-c", code, str(out)], check=True, timeout=300, env=dict(os.environ, **env))
        frames[tag] = dict(np.load(out))
    torch = torch_cuda
    sc = _scene("soup100000")
    d = dev_scene("soup100000")
    rgb, _ = d.render(cam_of(sc), sc.light, 1920, 1080)
    per = gi.shard_tiles(480, 270, 2) * gi.TILE * gi.TILE * 3
    p = torch.zeros(2 * per, dtype=torch.float64, device="cuda")
    for r in range(2):
        d.render_device(cam_of(sc), sc.light, 480, 270, p.data_ptr() + r * per * 8, 0, shard_count=2, shard_index=r)
    torch.cuda.synchronize()
    for tag, f in frames.items():
        assert U.bits_equal(rgb, f["c4"]).all(), tag
        assert U.bits_equal(rgb.reshape(-1), f["c4_stats"]).all(), tag + " (stats launch)"
        assert U.bits_equal(p.cpu().numpy(), f["packed"]).all(), tag + " packed"
    tiles = gi.shard_tiles(1920, 1080, 1)
    assert frames["flat"]["stats"][gi.STAT_R_OVF_TILES] == 0
    assert 0 < frames["flat_overflow"]["stats"][gi.STAT_R_OVF_TILES] < tiles
    assert frames["flat"]["stats"][gi.STAT_R_PAIRS] > 0
    print("R-C4 pairs", int(frames["flat"]["stats"][gi.STAT_R_PAIRS]), "overflowed tiles without a pool",
          int(frames["flat_overflow"]["stats"][gi.STAT_R_OVF_TILES]), "of", tiles)


def _strip_scene(n=5000, seed=6, size=0.03):
    """n small triangles in a thin vertical strip that a 2048-wide frame sees in ONE 8-pixel tile
    column (tiles X, X + 256, X + 512, ... at 256 tiles per row): k_rf_reach's chunks of 64 hits then
    hold tiles whose indices differ by multiples of 256, the case that broke round 5's memo tag
    (ADVICE r05, high)."""
    rng = np.random.default_rng(seed)
    s = S.Scene(entities=[], name="strip")
    # pixel column x looks at y = 20.48 - 0.02 x on the plane x = 0 (raytracer.h:26-30, 41-43 at
    # w = 2048): tile column 128 covers y in (-0.14, 0.02]; rows reach z in [-1.28, 20.48]
    c = np.stack([rng.uniform(-2.0, 2.0, n), rng.uniform(-0.13, 0.01, n), rng.uniform(-1.0, 20.0, n)], 1)
    for k in range(n):
        v = c[k] + rng.uniform(-size, size, (3, 3))
        s.imp_triangle(tuple(v[0]), tuple(v[1]), tuple(v[2]), tuple(rng.integers(0, 2, 3)))
    return s


@pytest.mark.parametrize("size", [0.03, 0.3])
def test_mode_r_flat_reach_sparse_tile_column(torch_cuda, tmp_path, size):
    """Mode R's flat phases (the default above 4096 entities) on a scene hit only in one tile column of
    a 2048-wide frame: every pixel equals k_mode_r's (GI_R_FLAT=0, a child process) bit for bit and the
    strip's pixels equal the oracle's (within 1e-5 relative, RGB888 exact).  The reach phase's node-test
    memo must never hand one tile's result to a tile 256 (or any multiple) further on."""
    import subprocess
    import sys
    sc = _strip_scene(size=size)   # (0.3: triangles over several tile columns and octree leaves)
    w, h = 2048, 1088
    d = gi.DeviceScene.from_scene(sc)
    assert d.r_kernel() == "k_rf_walk"
    rgb, rgb8 = d.render(cam_of(sc), sc.light, w, h)
    scn = tmp_path / "strip.scn"
    scn.write_text(sc.to_scn())
    out = tmp_path / "r0.npy"
    code = ("import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r); import oracle_util as U; "
            "gi = U.pkg(); S = U.scenes(); sc = S.parse_scn(open(%r).read()); d = gi.DeviceScene.from_scene(sc); "
            "np.save(%r, d.render(gi.Camera(sc.cam_pos, sc.cam_look, sc.focal), sc.light, %d, %d)[0])"
            ) % (U.ROOT, os.path.join(U.ROOT, "tests"), str(scn), str(out), w, h)
    subprocess.run([sys.executable, "-c", code], check=True, timeout=300, env=dict(os.environ, GI_R_FLAT="0"))
    ref = np.load(out)
    same = U.bits_equal(rgb, ref).all(2)
    assert same.all(), f"{int((~same).sum())} pixels differ from k_mode_r (rows {np.nonzero(~same.all(1))[0][:8]})"
    win = (1016, 0, 1040, h)
    o = U.oracle_render(sc.to_scn(), w, h, window=win, threads=16)
    g = rgb[:, win[0]:win[2]].reshape(-1, 3)
    assert (o["hit"] >= 0).sum() > 1000
    assert_rel(g, o["rgb"], "strip window")
    assert (rgb8[:, win[0]:win[2]].reshape(-1, 3) == o["q"]).all()
