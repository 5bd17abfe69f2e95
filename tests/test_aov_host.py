"""CPU: the feature buffers' host side (gi_render_aov, gi_camera_rays) -- the frames and references of
tests/aov_frames.py judged on the oracle alone, the Python wrappers' argument checks, and the C-ABI's
declarations.  No device."""
import os
import re

import numpy as np
import pytest

import aov_frames as A
import oracle_util as U

gi = U.pkg()
NEW = ("gi_render_aov_device", "gi_render_aov", "gi_camera_rays_device", "gi_camera_rays")


@pytest.mark.parametrize("key", sorted(A.FRAMES))
def test_frames_hold_hits_and_misses(key):
    """Every frame the device tests use, judged on gio_render: at least 5 % of its pixels hit and at least
    10 % missed, and at least 40 pixels of each (the empty scene: all missed)."""
    r = A.reference(key)
    hit = r["hit"] >= 0
    n = len(hit)
    _, _, w, h, _ = A.FRAMES[key]
    assert n == w * h
    if (w, h) != (64, 40):   # edge tiles and a partial last wave (the 64 x 40 frames: whole tiles and waves)
        assert w % 8 and h % 8 and n % 64
    if key == "empty":
        assert not hit.any()
        return
    print(key, "hit share %.3f (%d of %d)" % (hit.mean(), hit.sum(), n))
    assert hit.sum() >= max(40, 0.05 * n) and (~hit).sum() >= max(40, 0.10 * n), (key, int(hit.sum()), n)
    # the brute force agrees on which pixels hit, and a miss is (-1, +inf)
    assert ((r["prim"] >= 0) == hit).all()
    assert np.isposinf(r["t"][~hit]).all() and (r["prim"][~hit] == -1).all() and (r["uv"][~hit] == 0).all()


def test_far_camera_is_beyond_the_far_origin_rule():
    """The far frame's camera is more than x_far_r = 16 scene extents out (the Cornell box: extent 10)."""
    sc, _, _, _ = A.frame_scene("cornell/far")
    assert max(abs(c) for c in sc.cam_pos) > 16 * 10.0 * 2


@pytest.mark.parametrize("key", ["cornell/0.01", "cornell_sphere/0.004"])
def test_numpy_camera_reproduces_the_oracles_primary_hits(key):
    """The numpy restatement of the camera (the rays' reference): run through gio_x_query, hop 1 hits the
    entity gio_render reports on every pixel.  Scenes of ImpTriangles and ImpSpheres: primitive i is entity i."""
    sc, _, w, h = A.frame_scene(key)
    S = U.scenes()
    assert all(e.kind in (S.IMP_TRIANGLE, S.IMP_SPHERE) for e in sc.entities)
    r = A.reference(key)
    assert (r["prim"] == r["hit"]).all(), int((r["prim"] != r["hit"]).sum())
    assert (r["hit"] >= 0).any() and (r["hit"] < 0).any()
    rays = r["rays"]
    assert rays.shape == (w * h, 8) and np.isposinf(rays[:, 6]).all() and (rays[:, 7] == 0).all()
    assert (rays[:, 0:3] == np.array(sc.cam_pos)).all()
    assert (np.abs(np.sqrt((rays[:, 3:6] ** 2).sum(1)) - 1.0) <= 1e-9).all()   # (the project's NTOL for geometric checks)
    # a window's rays are the same rectangle of the whole frame's
    win = A.rays_np(sc, w, h, A.ODD_WINDOW)
    assert U.bits_equal(win, A.window_of(rays, w, h, A.ODD_WINDOW).reshape(-1, 8)).all()


@pytest.mark.parametrize("name", A.ALBEDO_SCENES)
def test_albedo_reference_is_the_oracles_frame(name):
    """With every material of shader (1, 0, 0) the oracle's depth-1 frame is min(texel(colour, u, v), 1)
    restated in numpy from the oracle's own hit and uv, bit for bit, and 0 on misses."""
    r = A.albedo_reference(name)
    hit = r["hit"] >= 0
    n = len(hit)   # (the frames' cap: these frames run on the device too)
    assert hit.sum() >= max(40, 0.05 * n) and (~hit).sum() >= max(40, 0.10 * n), (name, int(hit.sum()), n)
    assert U.bits_equal(np.minimum(r["albedo"], 1.0), r["rgb"]).all()
    assert (r["rgb"][~hit] == 0.0).all() and (r["albedo"][~hit] == 0.0).all()
    tx = r["albedo"][hit]
    assert len(np.unique(tx, axis=0)) >= 2   # the checker's white and at least one colour


def test_header_declares_the_feature_buffers_and_exports_list_them():
    hdr = open(os.path.join(U.ROOT, "include", "gi.h")).read()
    for f in NEW:
        assert re.search(r"^int %s\(" % f, hdr, re.M), f
        assert f in gi.EXPORTS
    assert re.search(r"^int gi_render_aov_device\(gi_scene\* scene, const gi_camera\* cam, const gi_aov_frame\* frame, "
                     r"const gi_aov\* d_out,\s+void\* stream\);", hdr, re.M)
    assert re.search(r"^int gi_camera_rays\(const gi_camera\* cam, const gi_aov_frame\* frame, double\* rays\);", hdr, re.M)
    assert "typedef struct gi_aov_frame { int32_t w, h, x0, y0, x1, y1; } gi_aov_frame;" in hdr
    assert ("typedef struct gi_aov { double* t; double* normal; double* albedo; int32_t* prim; int32_t* entity; "
            "int32_t* uv; } gi_aov;") in hdr
    assert int(re.search(r"#define GI_ABI_VERSION (\d+)", hdr).group(1)) == gi.ABI_VERSION >= 13
    # the ctypes mirrors have the header's layout
    assert [f for f, _ in gi.Aov._fields_] == list(gi.AOV_OUTPUTS) == ["t", "normal", "albedo", "prim", "entity", "uv"]
    assert [f for f, _ in gi.AovFrame._fields_] == ["w", "h", "x0", "y0", "x1", "y1"]


def test_wrappers_check_want_and_window_without_the_library(monkeypatch):
    """render_aov / render_aov_device / camera_rays / camera_rays_device check want, the frame and the
    window in Python and raise ValueError before the library is touched (here: lib() would fail the test)."""
    cam = gi.Camera((-10.0, 0.0, 0.0), (1.0, 0.0, 0.0), 0.01)   # (gi_camera_init: host code)

    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(gi, "lib", no_lib)
    d = gi.DeviceScene.__new__(gi.DeviceScene)   # no scene: the checks come first
    for want in ((), ("t", "t"), ("colour",), ("t", "depth"), ("uv", "prim", "uv")):
        with pytest.raises(ValueError):
            d.render_aov(cam, 37, 21, want=want)
    bad_windows = [(0, 0, 38, 21), (0, 0, 37, 22), (-1, 0, 37, 21), (0, -1, 37, 21), (30, 3, 5, 20), (5, 20, 30, 3),
                   (0, 0, 37), (0, 0, 37, 21, 1), (0.0, 0, 37, 21)]
    for win in bad_windows:
        with pytest.raises(ValueError):
            d.render_aov(cam, 37, 21, window=win)
        with pytest.raises(ValueError):
            d.render_aov_device(cam, 37, 21, window=win, d_t=1024)
        with pytest.raises(ValueError):
            gi.camera_rays(cam, 37, 21, window=win)
        with pytest.raises(ValueError):
            gi.camera_rays_device(cam, 37, 21, 1024, window=win)
    for w, h in ((0, 21), (37, 0), (-3, 21), (37.0, 21)):
        with pytest.raises(ValueError):
            d.render_aov(cam, w, h)
        with pytest.raises(ValueError):
            gi.camera_rays(cam, w, h)
    f = gi._aov_frame(37, 21, A.ODD_WINDOW)   # a good window passes the same check
    assert (f.w, f.h, f.x0, f.y0, f.x1, f.y1) == (37, 21) + A.ODD_WINDOW
