"""GPU: first-hit feature buffers (gi_render_aov*) and camera rays (gi_camera_rays*) against the oracle.

k_aov (gi_wf.hip) runs in the kernel variant a Mode X render of the scene runs; the frames and their
references are tests/aov_frames.py's, judged on the CPU by tests/test_aov_host.py.  Everything is exact:
entity and uv equal gio_render's, prim equals gio_x_query's brute force, t, albedo, ray records and (against
gi_intersect) normals compare bit for bit; a miss is (-1, -1, +inf, 0, 0, (0, 0)).  Only the geometric
checks of the normal carry a bound, the project's NTOL = 1e-9 (tests/test_gpu_cast.py)."""
import copy
import ctypes

import numpy as np
import pytest

import aov_frames as A
import cast_rays as C
import oracle_util as U
import x_rays as R
from x_scenes import with_env

pytestmark = pytest.mark.gpu

gi = U.pkg()
S = U.scenes()
NTOL = 1e-9
PLANES = {"t": 1, "normal": 3, "albedo": 3, "prim": 1, "entity": 1, "uv": 2}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    return torch


_devs = {}


def dev_of(name, albedo=False):
    """The device scene of a base scene (a frame's focal and camera do not enter it), built once."""
    key = (name, albedo)
    if key not in _devs:
        sc, env = (A.albedo_scene(name)[:2] if albedo else A.base_scene(name))
        _devs[key] = with_env(env, lambda: gi.DeviceScene.from_scene(sc))
    return _devs[key]


def check_variant(name):
    """The scene's kernel variant, asserted as tests/test_gpu_cast.py check_variant does (main: printed)."""
    d = dev_of(name)
    var, info = d.kat_x_variant(0), d.info()
    if name not in C.VARIANTS:
        print(name, var, info["x_lds_resident"], info["x_node_bytes"])
        return d
    want, lds, node_bytes = C.VARIANTS[name]
    assert {k: var[k] for k in want} == want, (name, var)
    assert info["x_lds_resident"] == lds and info["x_node_bytes"] == node_bytes, (name, info)
    return d


def cam_of(sc):
    return gi.Camera(sc.cam_pos, sc.cam_look, sc.focal)


def flat(out):
    """A render_aov result as planes (rows * cols[, k]), the references' layout."""
    return {k: v.reshape((-1,) + v.shape[2:]) for k, v in out.items()}


def assert_frame(what, ref, out):
    """Every plane of a whole-window result against the oracle's reference."""
    hit = ref["hit"] >= 0
    bad = {k: int((out[k] != ref[r]).sum()) for k, r in (("entity", "hit"), ("prim", "prim")) if (out[k] != ref[r]).any()}
    if (out["uv"] != ref["uv"]).any():
        bad["uv"] = int((out["uv"] != ref["uv"]).any(1).sum())
    if not U.bits_equal(out["t"], ref["t"]).all():
        bad["t"] = int((~U.bits_equal(out["t"], ref["t"])).sum())
    if bad:
        print(what, "pixels that differ:", bad)
    assert not bad, (what, bad)
    miss = ~hit
    assert (out["entity"][miss] == -1).all() and (out["prim"][miss] == -1).all() and np.isposinf(out["t"][miss]).all()
    assert (out["normal"][miss] == 0.0).all() and (out["albedo"][miss] == 0.0).all() and (out["uv"][miss] == 0).all()
    assert (out["entity"][hit] >= 0).all() and np.isfinite(out["t"][hit]).all()
    n = out["normal"][hit]
    assert (np.abs(np.sqrt((n * n).sum(1)) - 1.0) <= NTOL).all()
    assert ((n * ref["rays"][hit, 3:6]).sum(1) <= 0.0).all()


# ---- 1. rays ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("key", ["cornell/0.004", "cornell/0.01", "cornell/far", "main"])
def test_camera_rays_equal_the_numpy_camera(torch_cuda, key):
    """camera_rays equals the numpy restatement of the oracle's camera bit for bit, whole frame and the odd
    window; tmax = +inf, reserved = 0; the device form on a non-default stream equals the host form."""
    torch = torch_cuda
    sc, _, w, h = A.frame_scene(key)
    cam = cam_of(sc)
    ref = A.reference(key)["rays"]
    rays = gi.camera_rays(cam, w, h)
    assert rays.shape == (w * h, gi.RAY_DOUBLES) and rays.dtype == np.float64
    ne = ~U.bits_equal(rays, ref)
    assert not ne.any(), (key, int(ne.any(1).sum()), rays[ne.any(1)][:2], ref[ne.any(1)][:2])
    assert np.isposinf(rays[:, 6]).all() and (rays[:, 7].view(np.int64) == 0).all()
    win = A.ODD_WINDOW if (w, h) == (37, 21) else (5, 3, 62, 39)
    rw = gi.camera_rays(cam, w, h, window=win)
    assert U.bits_equal(rw, A.rays_np(sc, w, h, win)).all()
    n, pad = len(rw), 8
    buf = torch.full(((n + pad) * gi.RAY_DOUBLES,), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    assert st.cuda_stream != 0 and buf.data_ptr() % 16 == 0
    gi.camera_rays_device(cam, w, h, buf.data_ptr(), window=win, stream=st.cuda_stream)
    st.synchronize()
    got = buf.cpu().numpy().reshape(n + pad, gi.RAY_DOUBLES)
    assert U.bits_equal(got[:n], rw).all() and (got[n:] == -7.0).all()


# ---- 2. against the oracle, per scene ---------------------------------------------------------------
@pytest.mark.parametrize("key", sorted(A.FRAMES))
def test_feature_buffers_equal_the_oracle(torch_cuda, key):
    """The scene's variant first; then entity and uv equal gio_render's hit and uv on every pixel, prim and t
    (bit for bit) gio_x_query's brute force on the frame's rays, and a miss is (-1, -1, +inf, 0, 0, (0, 0))."""
    name = A.FRAMES[key][0]
    d = check_variant(name)
    sc, _, w, h = A.frame_scene(key)
    ref = A.reference(key)
    res = d.render_aov(cam_of(sc), w, h)
    assert list(res) == list(gi.AOV_OUTPUTS)
    for k, c in PLANES.items():
        assert res[k].shape == ((h, w) if c == 1 else (h, w, c)), (k, res[k].shape)
        assert res[k].dtype == (np.int32 if k in ("prim", "entity", "uv") else np.float64)
    out = flat(res)
    assert_frame(key, ref, out)
    hit = ref["hit"] >= 0
    if name == "empty":
        assert not hit.any() and (out["prim"] == -1).all()
    if name == "main":   # an ExpQuad (two triangles), two ImpSpheres
        assert (out["entity"] == np.array([-1, 0, 0, 1, 2])[out["prim"] + 1]).all()
    if name == "zoo":
        assert len(np.unique(out["entity"][hit])) >= 8
    if name == "coincident":   # two primitives at every hit's t: the lower index
        assert set(np.unique(out["prim"][hit])) <= {0, 1}


# ---- 3. albedo ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", A.ALBEDO_SCENES)
def test_albedo_is_the_colour_mode_x_shades_with(torch_cuda, name):
    """Materials of shader (1, 0, 0): min(albedo, 1) equals the oracle's depth-1 frame bit for bit, and albedo
    itself the numpy texel of the oracle's hit, uv and the colours."""
    check_variant(name)   # (materials do not enter the variant: the geometry's)
    d = dev_of(name, albedo=True)
    sc, _, w, h = A.albedo_scene(name)
    ref = A.albedo_reference(name)
    out = flat(d.render_aov(cam_of(sc), w, h))
    assert_frame("albedo " + name, ref, out)
    assert U.bits_equal(np.minimum(out["albedo"], 1.0), ref["rgb"]).all()
    assert U.bits_equal(out["albedo"], ref["albedo"]).all()
    # and the render itself: the depth-1 Mode X frame is that colour
    rgb, _ = d.render(cam_of(sc), sc.light, w, h, mode=gi.MODE_X, spp=1, depth=1)
    assert U.bits_equal(rgb.reshape(-1, 3), np.minimum(out["albedo"], 1.0)).all()


# ---- 4. against the existing queries ------------------------------------------------------------------
def _unit(v):
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


@pytest.mark.parametrize("key", ["cornell/0.004", "cornell_sphere/0.01", "one_triangle", "coincident", "soup1000",
                                 "zoo", "soup_xcnode", "corner3_octree", "cornell/far"])
def test_feature_buffers_equal_intersect_over_camera_rays(torch_cuda, key):
    """gi_intersect over camera_rays of the same frame: the same t (bits), prim, entity and normal (bits).
    Scenes of ImpTriangles and ImpSpheres: the normals pass the geometric checks of
    tests/test_gpu_cast.py test_attributes_of_triangle_and_sphere_scenes within NTOL."""
    name = A.FRAMES[key][0]
    d = check_variant(name)
    sc, _, w, h = A.frame_scene(key)
    cam = cam_of(sc)
    out = flat(d.render_aov(cam, w, h, want=("t", "prim", "entity", "normal")))
    rays = gi.camera_rays(cam, w, h)
    q = d.intersect(rays)
    assert (out["prim"] == q["prim"]).all() and (out["entity"] == q["entity"]).all()
    assert U.bits_equal(out["t"], q["t"]).all() and U.bits_equal(out["normal"], q["normal"]).all()
    hit = out["prim"] >= 0
    assert hit.sum() >= 40 and (~hit).sum() >= 40
    if not all(e.kind in (S.IMP_TRIANGLE, S.IMP_SPHERE) for e in sc.entities):
        return
    assert (out["entity"] == out["prim"]).all()
    o, dr, n, prim = rays[hit, 0:3], rays[hit, 3:6], out["normal"][hit], out["prim"][hit]
    assert (np.abs(np.sqrt((n * n).sum(1)) - 1.0) <= NTOL).all()
    assert ((n * _unit(dr)).sum(1) <= 0.0).all()
    tri = R.Geo(sc).ptri[prim]
    fl = ~np.isnan(tri).any((1, 2))
    e1, e2 = _unit(tri[fl, 1] - tri[fl, 0]), _unit(tri[fl, 2] - tri[fl, 0])
    assert (np.abs((n[fl] * e1).sum(1)) <= NTOL).all() and (np.abs((n[fl] * e2).sum(1)) <= NTOL).all()
    if (~fl).any():
        c = np.array([sc.entities[p].args[:3] for p in prim[~fl]])
        P = C.hop2_points(o[~fl], dr[~fl], out["t"][hit][~fl])
        assert (np.sqrt((np.cross(n[~fl], _unit(P - c)) ** 2).sum(1)) <= NTOL).all()
    assert (~fl).any() == (name == "cornell_sphere")


# ---- 5. windows and sizes -----------------------------------------------------------------------------
def test_windows_equal_the_rectangle_of_the_whole_frame(torch_cuda):
    """The odd window and a one-pixel window (picking) equal the same rectangle cut from the whole frame."""
    for key in ("cornell_sphere/0.004", "zoo", "soup1000"):
        d = check_variant(A.FRAMES[key][0])
        sc, _, w, h = A.frame_scene(key)
        cam = cam_of(sc)
        whole = d.render_aov(cam, w, h)
        hit = np.argwhere(whole["prim"] >= 0)
        py, px = (int(v) for v in hit[len(hit) // 2])
        for win in (A.ODD_WINDOW, (px, py, px + 1, py + 1), (0, 0, 1, 1), (w - 1, h - 1, w, h), (0, 7, w, 8), (8, 0, 9, h)):
            x0, y0, x1, y1 = win
            part = d.render_aov(cam, w, h, window=win)
            for k in gi.AOV_OUTPUTS:
                a, b = part[k], whole[k][y0:y1, x0:x1]
                assert a.shape == b.shape, (key, win, k)
                assert (U.bits_equal(a, b) if a.dtype == np.float64 else a == b).all(), (key, win, k)
        pick = d.render_aov(cam, w, h, window=(px, py, px + 1, py + 1), want=("entity", "t"))
        assert pick["entity"].shape == (1, 1) and pick["entity"][0, 0] == A.reference(key)["hit"][py * w + px] >= 0


@pytest.mark.parametrize("w,h", [(1, 1), (3, 2), (65, 1), (1, 65)])
def test_tiny_frames(torch_cuda, w, h):
    """Frames of one pixel, less than a tile, and one row / column of 65: a partial wave, edge tiles only."""
    d = check_variant("cornell")
    sc = copy.deepcopy(A.base_scene("cornell")[0])
    sc.focal = 0.02   # (the frame's vertical offset grows with w: at this focal every one of these frames has hits)
    ref = A._reference(sc, w, h)
    assert (ref["hit"] >= 0).any()
    cam = cam_of(sc)
    assert_frame(f"{w} x {h}", ref, flat(d.render_aov(cam, w, h)))
    assert U.bits_equal(gi.camera_rays(cam, w, h), ref["rays"]).all()


@pytest.mark.parametrize("name", ["cornell", "corner3_octree", "soup1000"])
def test_more_pixels_than_resident_lanes(torch_cuda, name):
    """1031 x 517 = 533027 pixels (the device holds at most 256 CUs x 2048 lanes = 2^19): every wave's loop
    over its batches runs more than once.  cornell: LDS, flat; corner3_octree: LDS, tree; soup1000: HBM."""
    d = check_variant(name)
    sc = copy.deepcopy(A.base_scene(name)[0])
    sc.focal = 0.1
    w, h = 1031, 517
    ref = A._reference(sc, w, h)
    assert (ref["hit"] >= 0).sum() > 1000 and (ref["hit"] < 0).sum() > 1000
    assert_frame(f"{name} {w} x {h}", ref, flat(d.render_aov(cam_of(sc), w, h)))


def test_want_subsets_write_only_what_was_asked(torch_cuda):
    """Host form: the dict holds exactly want, in its order.  Device form: guard values in the planes that
    were not asked for, and past the window's end of those that were, stay untouched."""
    torch = torch_cuda
    key = "cornell_sphere/0.004"
    d = check_variant(A.FRAMES[key][0])
    sc, _, w, h = A.frame_scene(key)
    cam = cam_of(sc)
    whole = d.render_aov(cam, w, h)
    for want in (("t",), ("uv",), ("albedo", "prim"), ("entity", "normal", "t")):
        part = d.render_aov(cam, w, h, want=want)
        assert list(part) == list(want)
        for k in want:
            assert (U.bits_equal(part[k], whole[k]) if part[k].dtype == np.float64 else part[k] == whole[k]).all(), (want, k)
    n, pad = w * h, 64

    def fresh():
        return {k: torch.full(((n + pad) * c,), -7.0 if k in ("t", "normal", "albedo") else -777,
                              dtype=torch.float64 if k in ("t", "normal", "albedo") else torch.int32, device="cuda")
                for k, c in PLANES.items()}
    for want in (("t",), ("uv", "albedo"), ("prim", "entity", "normal"), gi.AOV_OUTPUTS):
        b = fresh()
        torch.cuda.synchronize()
        d.render_aov_device(cam, w, h, **{"d_" + k: b[k].data_ptr() for k in want})
        torch.cuda.synchronize()
        for k, c in PLANES.items():
            a = b[k].cpu().numpy()
            guard = -7.0 if a.dtype == np.float64 else -777
            if k in want:
                exp = whole[k].reshape(-1)
                assert (U.bits_equal(a[:n * c], exp) if a.dtype == np.float64 else a[:n * c] == exp).all(), (want, k)
                assert (a[n * c:] == guard).all(), (want, k)
            else:
                assert (a == guard).all(), (want, k)


# ---- 6. device form and state -------------------------------------------------------------------------
def test_device_form_on_a_stream_equals_the_host_form(torch_cuda):
    """render_aov_device into torch tensors on a side stream, whole frame and the odd window, on a flat LDS
    scene and an HBM scene."""
    torch = torch_cuda
    for key in ("cornell/0.004", "zoo"):
        d = check_variant(A.FRAMES[key][0])
        sc, _, w, h = A.frame_scene(key)
        cam = cam_of(sc)
        for win in (None, A.ODD_WINDOW):
            host = d.render_aov(cam, w, h, window=win)
            n = host["t"].size
            b = {k: torch.zeros((n * c,), dtype=torch.float64 if k in ("t", "normal", "albedo") else torch.int32, device="cuda")
                 for k, c in PLANES.items()}
            torch.cuda.synchronize()
            st = torch.cuda.Stream()
            assert st.cuda_stream != 0
            d.render_aov_device(cam, w, h, window=win, stream=st.cuda_stream, **{"d_" + k: v.data_ptr() for k, v in b.items()})
            st.synchronize()
            for k in gi.AOV_OUTPUTS:
                a, e = b[k].cpu().numpy(), host[k].reshape(-1)
                assert (U.bits_equal(a, e) if a.dtype == np.float64 else a == e).all(), (key, win, k)


def test_feature_buffers_share_no_state_with_renders(torch_cuda):
    """An AOV call between two progressive passes does not end the progressive frame: the final pass equals
    the one-shot frame bit for bit; calls before and after a whole render return identical planes."""
    key = "cornell/0.01"
    d = check_variant("cornell")
    sc, _, w, h = A.frame_scene(key)
    cam = cam_of(sc)
    kw = dict(mode=gi.MODE_X, spp=4, depth=3, seed=5)
    before = d.render_aov(cam, w, h)
    one_shot, one_shot8 = d.render(cam, sc.light, 32, 32, **kw)
    after = d.render_aov(cam, w, h)
    d.render(cam, sc.light, 32, 32, samples=(0, 2), **kw)
    between = d.render_aov(cam, w, h)
    rays = gi.camera_rays(cam, w, h)
    rgb, rgb8 = d.render(cam, sc.light, 32, 32, samples=(2, 4), **kw)
    assert U.bits_equal(rgb, one_shot).all() and (rgb8 == one_shot8).all()
    assert U.bits_equal(rays, A.reference(key)["rays"]).all()
    for other in (after, between):
        for k in before:
            assert (U.bits_equal(before[k], other[k]) if before[k].dtype == np.float64 else before[k] == other[k]).all(), k
    assert_frame(key, A.reference(key), flat(between))


# ---- 7. argument errors -------------------------------------------------------------------------------
def test_argument_errors(torch_cuda):
    """Every GI_ERR_ARG case of gi.h, with a message and before anything is launched; the empty window
    returns GI_OK and writes nothing."""
    torch = torch_cuda
    d = check_variant("cornell")
    sc, _, w, h = A.frame_scene("cornell/0.004")
    cam = cam_of(sc)
    L = gi.lib()
    n = w * h
    t = np.full(n, -7.0)
    rays = np.full((n, gi.RAY_DOUBLES), -7.0)
    dt = torch.full((n,), -7.0, dtype=torch.float64, device="cuda")
    dr = torch.full((n * gi.RAY_DOUBLES + 2,), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    dp = ctypes.POINTER(ctypes.c_double)

    def frame(*v):
        return gi.AovFrame(*v)
    good = frame(w, h, 0, 0, w, h)
    host_out = gi.Aov(t=t.ctypes.data)
    dev_out = gi.Aov(t=dt.data_ptr())
    cp, gp = ctypes.byref(cam._c), ctypes.byref(good)

    def refused(rc):
        assert rc == -1 and len(L.gi_last_error()) > 0, (rc, L.gi_last_error())
    # null scene, camera, frame, output struct
    refused(L.gi_render_aov(None, cp, gp, ctypes.byref(host_out)))
    refused(L.gi_render_aov(d._h, None, gp, ctypes.byref(host_out)))
    refused(L.gi_render_aov(d._h, cp, None, ctypes.byref(host_out)))
    refused(L.gi_render_aov(d._h, cp, gp, None))
    refused(L.gi_render_aov_device(None, cp, gp, ctypes.byref(dev_out), None))
    refused(L.gi_render_aov_device(d._h, None, gp, ctypes.byref(dev_out), None))
    refused(L.gi_render_aov_device(d._h, cp, None, ctypes.byref(dev_out), None))
    refused(L.gi_render_aov_device(d._h, cp, gp, None, None))
    refused(L.gi_camera_rays(None, gp, rays.ctypes.data_as(dp)))
    refused(L.gi_camera_rays(cp, None, rays.ctypes.data_as(dp)))
    refused(L.gi_camera_rays(cp, gp, None))
    refused(L.gi_camera_rays_device(None, gp, dr.data_ptr(), None))
    refused(L.gi_camera_rays_device(cp, None, dr.data_ptr(), None))
    refused(L.gi_camera_rays_device(cp, gp, None, None))
    # every output null
    refused(L.gi_render_aov(d._h, cp, gp, ctypes.byref(gi.Aov())))
    refused(L.gi_render_aov_device(d._h, cp, gp, ctypes.byref(gi.Aov()), None))
    with pytest.raises(gi.GIError, match=r"\(-1\)"):
        d.render_aov_device(cam, w, h)
    # a misaligned ray buffer
    assert dr.data_ptr() % 16 == 0
    refused(L.gi_camera_rays_device(cp, gp, dr.data_ptr() + 8, None))
    # frame sizes and windows
    bad = [frame(0, h, 0, 0, 0, h), frame(w, 0, 0, 0, w, 0), frame(-1, h, 0, 0, 1, h), frame(w, -5, 0, 0, w, 1),
           frame(w, h, 0, 0, w + 1, h), frame(w, h, 0, 0, w, h + 1), frame(w, h, -1, 0, w, h), frame(w, h, 0, -1, w, h),
           frame(w, h, 30, 3, 5, 20), frame(w, h, 5, 20, 30, 3)]
    for f in bad:
        fp = ctypes.byref(f)
        refused(L.gi_render_aov(d._h, cp, fp, ctypes.byref(host_out)))
        refused(L.gi_render_aov_device(d._h, cp, fp, ctypes.byref(dev_out), None))
        refused(L.gi_camera_rays(cp, fp, rays.ctypes.data_as(dp)))
        refused(L.gi_camera_rays_device(cp, fp, dr.data_ptr(), None))
    # a non-finite camera field
    for field, i in (("pos", 0), ("pos", 2), ("up", 1), ("forward", 0), ("focal", None)):
        for v in (np.nan, np.inf, -np.inf):
            c2 = gi.CameraDesc.from_buffer_copy(cam._c)
            if i is None:
                setattr(c2, field, v)
            else:
                getattr(c2, field)[i] = v
            refused(L.gi_render_aov(d._h, ctypes.byref(c2), gp, ctypes.byref(host_out)))
            refused(L.gi_render_aov_device(d._h, ctypes.byref(c2), gp, ctypes.byref(dev_out), None))
            refused(L.gi_camera_rays(ctypes.byref(c2), gp, rays.ctypes.data_as(dp)))
            refused(L.gi_camera_rays_device(ctypes.byref(c2), gp, dr.data_ptr(), None))
    # the empty window: GI_OK, nothing launched, nothing written
    for f in (frame(w, h, 5, 3, 5, 20), frame(w, h, 5, 3, 30, 3), frame(w, h, w, h, w, h), frame(w, h, 0, 0, 0, 0)):
        fp = ctypes.byref(f)
        assert L.gi_render_aov(d._h, cp, fp, ctypes.byref(host_out)) == 0
        assert L.gi_render_aov_device(d._h, cp, fp, ctypes.byref(dev_out), None) == 0
        assert L.gi_camera_rays(cp, fp, rays.ctypes.data_as(dp)) == 0
        assert L.gi_camera_rays_device(cp, fp, dr.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert (t == -7.0).all() and (rays == -7.0).all()
    assert (dt.cpu().numpy() == -7.0).all() and (dr.cpu().numpy() == -7.0).all()
    e = d.render_aov(cam, w, h, window=(5, 3, 5, 20))
    assert e["t"].shape == (17, 0) and e["normal"].shape == (17, 0, 3) and e["uv"].shape == (17, 0, 2)
    assert gi.camera_rays(cam, w, h, window=(5, 3, 30, 3)).shape == (0, gi.RAY_DOUBLES)
