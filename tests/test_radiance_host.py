"""CPU: the host side of the radiance query, the sample rays and the resolve (gi_radiance*, gi_sample_rays*,
gi_resolve_samples*) -- the numpy references of tests/radiance_ref.py against gi_math.h compiled by g++, the
C-ABI's declarations and refusals, the Python wrappers' argument checks, and the lens geometry.  No device: every
call here returns before one is touched.  Nothing carries a tolerance but the lens geometry's 1e-12 (relative)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import aov_frames as A
import oracle_util as U
import radiance_ref as RR

gi = U.pkg()
NEW = ("gi_radiance_device", "gi_radiance", "gi_sample_rays_device", "gi_sample_rays", "gi_resolve_samples_device",
       "gi_resolve_samples")
CAM = dict(pos=(-10.0, 0.5, 0.25), look=(1.0, 0.0, 0.0), focal=0.01)


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _f64(bits):
    return np.asarray(bits, np.uint64).view(np.float64)


def test_numpy_random_numbers_equal_gi_math_h(tmp_path):
    """mx_key, mx_u01k and mx_disk of tests/radiance_ref.py against gi_math.h (tests/cpp/sample_rays_check.cpp), bit
    for bit: random inputs, the jitter's and the lens's bounce indices, the disk's octant boundaries (|a| == |b|,
    a == 0, b == 0, the centre), u = 0 and u just below 1."""
    exe = str(tmp_path / "src")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-I" + os.path.join(U.ROOT, "2019global_amd", "csrc"),
                    "-o", exe, os.path.join(U.ROOT, "tests", "cpp", "sample_rays_check.cpp")], check=True)
    rng = np.random.default_rng(2019)
    seeds = rng.integers(0, 2 ** 64, 200, dtype=np.uint64)
    streams = np.concatenate([rng.integers(0, 2 ** 64, 100, dtype=np.uint64), np.arange(100, dtype=np.uint64)])
    keys = rng.integers(0, 2 ** 64, 400, dtype=np.uint64)
    smp = rng.integers(0, 2 ** 32, 400, dtype=np.uint64)
    smp[:8] = [0, 1, 2, 3, 4, 7, 2 ** 32 - 1, 2 ** 31]
    bnc = rng.integers(0, 2 ** 16, 400, dtype=np.uint64)
    bnc[:6] = [0, 1, 0xFFFF, 0xFFFE, 0xFFFD, 3]
    dim = rng.integers(0, 5, 400, dtype=np.uint64)
    below1 = np.nextafter(1.0, 0.0)
    edge = [0.0, below1, 0.5, 0.25, 0.75, np.nextafter(0.5, 0.0), np.nextafter(0.5, 1.0), 2.0 ** -53, 0.125, 0.875]
    u = np.array([(a, b) for a in edge for b in edge] + [(t, t) for t in rng.random(50)] + [(t, 1.0 - t) for t in rng.random(50)]
                 + [tuple(p) for p in rng.random((600, 2))])
    assert ((u >= 0) & (u < 1)).all()
    a, b = 2.0 * u[:, 0] - 1.0, 2.0 * u[:, 1] - 1.0
    assert (np.abs(a) == np.abs(b)).sum() >= 60 and ((a == 0) & (b == 0)).sum() == 1 and (a == 0).sum() > 1 and (b == 0).sum() > 1
    lines = [f"k {s:x} {t:x}" for s, t in zip(seeds, streams)]
    lines += [f"u {k:x} {s:x} {q:x} {m:x}" for k, s, q, m in zip(keys, smp, bnc, dim)]
    lines += [f"d {p:x} {q:x}" for p, q in zip(_bits(u[:, 0]), _bits(u[:, 1]))]
    inp = tmp_path / "in.txt"
    inp.write_text("\n".join(lines) + "\n")
    out = subprocess.run([exe, str(inp)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    got = out.stdout.split("\n")
    gk = np.array([int(x, 16) for x in got[:200]], np.uint64)
    gu = np.array([int(x, 16) for x in got[200:600]], np.uint64)
    gd = np.array([[int(x, 16) for x in ln.split()] for ln in got[600:600 + len(u)]], np.uint64)
    assert (RR.mx_key(seeds, streams) == gk).all()
    un = RR.mx_u01k(keys, smp, bnc, dim)
    assert (_bits(un) == gu).all() and ((un >= 0) & (un < 1)).all()
    dx, dy, r2 = RR.mx_disk(u[:, 0], u[:, 1])
    for k, v in enumerate((dx, dy, r2)):
        ne = _bits(v) != gd[:, k]
        assert not ne.any(), (k, u[ne][:4], v[ne][:4], _f64(gd[ne, k])[:4])
    assert (r2 <= 1.0).all() and np.isfinite(dx).all() and np.isfinite(dy).all()


def test_header_declares_the_calls_and_exports_list_them():
    hdr = open(os.path.join(U.ROOT, "include", "gi.h")).read()
    for f in NEW:
        assert re.search(r"^int %s\(" % f, hdr, re.M), f
        assert f in gi.EXPORTS
    assert int(re.search(r"#define GI_ABI_VERSION (\d+)", hdr).group(1)) == gi.ABI_VERSION == 21
    assert "typedef struct gi_path_id { uint64_t stream; uint32_t sample; uint32_t reserved; } gi_path_id;" in hdr
    assert "typedef struct gi_radiance_params { int32_t depth; uint32_t flags; uint64_t seed; } gi_radiance_params;" in hdr
    assert "#define GI_SAMPLE_JITTER 1u" in hdr and gi.SAMPLE_JITTER == 1
    assert ctypes.sizeof(gi.PathId) == 16 == gi.PATH_ID_DTYPE.itemsize
    assert ctypes.sizeof(gi.RadianceParams) == 16 and ctypes.sizeof(gi.SampleParams) == 40
    assert [f for f, _ in gi.SampleParams._fields_] == ["seed", "sample_begin", "sample_end", "flags", "reserved", "aperture", "focus"]
    for n in ("sample_rays", "sample_rays_device", "resolve_samples", "resolve_samples_device", "PathId", "RadianceParams",
              "SampleParams"):
        assert n in gi.__all__ and hasattr(gi, n)
    assert hasattr(gi.DeviceScene, "radiance") and hasattr(gi.DeviceScene, "radiance_device")
    for part in ("Mode R", "shards and gi_multi", "drop-in headers", "GI_FLAG_STATS / GI_FLAG_TIME", "tmax on", "adaptive stopping",
                 "gi_frame_moments does not see these rows"):
        assert part in hdr[hdr.index("radiance along caller-supplied rays"):], part


def test_the_library_exports_the_calls():
    L = gi.lib()
    assert L.gi_abi_version() == 21
    for f in NEW:
        assert getattr(L, f) is not None


def _refused(rc):
    assert rc == -1 and len(gi.lib().gi_last_error()) > 0
    return gi.lib().gi_last_error().decode()


def test_radiance_refusals_come_before_the_scene():
    """Every GI_ERR_ARG case of gi_radiance*, on both forms, with a NULL scene: the message names the argument, so
    the refusal came before the scene (and so before any device) was looked at; a call whose other arguments are
    good is refused for the scene."""
    L = gi.lib()
    rays, rgb, ids = np.zeros((4, 8)), np.full((4, 3), -7.0), np.zeros(4, gi.PATH_ID_DTYPE)
    light = (ctypes.c_double * 3)(0.0, 0.0, 3.0)
    dp = ctypes.POINTER(ctypes.c_double)
    R, G, I = rays.ctypes.data, rgb.ctypes.data, ids.ctypes.data
    assert R % 16 == 0 and I % 8 == 0
    good = gi.RadianceParams(4, 0, 1)

    def both(n, r, i, li, p, g):
        m1 = _refused(L.gi_radiance(None, n, ctypes.cast(r, dp), i, li, p, ctypes.cast(g, dp)))
        m2 = _refused(L.gi_radiance_device(None, n, r, i, li, p, g, None))
        assert m1 == m2
        return m1
    assert "null scene" in both(4, R, I, light, ctypes.byref(good), G)
    assert "null scene" in both(4, R, None, light, ctypes.byref(good), G)
    assert "null scene" in both(0, R, I, light, ctypes.byref(good), G)
    for n in (-1, 2 ** 32):
        assert "null scene" not in both(n, R, I, light, ctypes.byref(good), G)
    for r, li, p, g in ((None, light, ctypes.byref(good), G), (R, None, ctypes.byref(good), G), (R, light, None, G),
                        (R, light, ctypes.byref(good), None)):
        assert "null rays, light, params or output" in both(4, r, I, li, p, g)
    for depth in (0, -1, 65535, 2 ** 31 - 1):
        assert "depth" in both(4, R, I, light, ctypes.byref(gi.RadianceParams(depth, 0, 1)), G)
    assert "null scene" in both(4, R, I, light, ctypes.byref(gi.RadianceParams(65534, gi.FLAG_X_NO_SHADOW, 1)), G)
    for fl in (gi.FLAG_STATS, gi.FLAG_TIME, gi.FLAG_X_SEG, gi.FLAG_X_NO_SHADOW | gi.FLAG_STATS, 1 << 31):
        assert "flag" in both(4, R, I, light, ctypes.byref(gi.RadianceParams(4, fl, 1)), G)
    assert "16-byte" in _refused(L.gi_radiance_device(None, 3, R + 8, I, light, ctypes.byref(good), G, None))
    assert "8-byte" in _refused(L.gi_radiance_device(None, 3, R, I + 4, light, ctypes.byref(good), G, None))
    assert (rgb == -7.0).all()


def _cam():
    return gi.Camera(CAM["pos"], CAM["look"], CAM["focal"])


def test_sample_rays_refusals_and_empty_calls():
    """Every GI_ERR_ARG case of gi_sample_rays*, on both forms; an empty window and an empty sample range return
    GI_OK and write nothing.  None of these calls reaches a device."""
    L = gi.lib()
    cam = _cam()
    w, h = 37, 21
    rays, ids = np.full((w * h * 2, 8), -7.0), np.zeros(w * h * 2, gi.PATH_ID_DTYPE)
    R, I = rays.ctypes.data, ids.ctypes.data
    fr = gi.AovFrame(w, h, 0, 0, w, h)

    def P(**kw):
        d = dict(seed=1, sample_begin=0, sample_end=2, flags=gi.SAMPLE_JITTER, reserved=0, aperture=0.0, focus=1.0)
        d.update(kw)
        return gi.SampleParams(*[d[f] for f, _ in gi.SampleParams._fields_])

    def both(c, f, p, r, i):
        m1 = _refused(L.gi_sample_rays(c, f, p, r, i))
        m2 = _refused(L.gi_sample_rays_device(c, f, p, r, i, None))
        assert m1 == m2
        return m1
    C, F = ctypes.byref(cam._c), ctypes.byref(fr)
    both(None, F, ctypes.byref(P()), R, I)
    both(C, None, ctypes.byref(P()), R, I)
    both(C, F, None, R, I)
    for f in (gi.AovFrame(w, h, 0, 0, w + 1, h), gi.AovFrame(w, h, -1, 0, w, h), gi.AovFrame(w, h, 30, 3, 5, 20),
              gi.AovFrame(0, h, 0, 0, 0, h), gi.AovFrame(w, -2, 0, 0, w, 1)):
        both(C, ctypes.byref(f), ctypes.byref(P()), R, I)
    bad_cam = gi.CameraDesc.from_buffer_copy(cam._c)
    bad_cam.pos[1] = float("nan")
    assert "camera" in both(ctypes.byref(bad_cam), F, ctypes.byref(P()), R, I)
    for kw in (dict(sample_begin=-1), dict(sample_begin=3, sample_end=2)):
        assert "sample_begin" in both(C, F, ctypes.byref(P(**kw)), R, I)
    for ap in (-1e-9, float("inf"), float("nan"), -float("inf")):
        assert "aperture" in both(C, F, ctypes.byref(P(aperture=ap)), R, I)
    for fo in (0.0, -1.0, float("inf"), float("nan")):
        assert "focus" in both(C, F, ctypes.byref(P(aperture=0.1, focus=fo)), R, I)
    assert "flag" in both(C, F, ctypes.byref(P(flags=2)), R, I)
    assert "flag" in both(C, F, ctypes.byref(P(flags=gi.SAMPLE_JITTER | 4)), R, I)
    assert "reserved" in both(C, F, ctypes.byref(P(reserved=1)), R, I)
    assert "null" in both(C, F, ctypes.byref(P()), None, None)
    big = gi.AovFrame(2 ** 16, 2 ** 16, 0, 0, 2 ** 16, 2 ** 16)
    assert "records" in both(C, ctypes.byref(big), ctypes.byref(P()), R, I)
    assert "16-byte" in _refused(L.gi_sample_rays_device(C, F, ctypes.byref(P()), R + 8, I, None))
    assert "8-byte" in _refused(L.gi_sample_rays_device(C, F, ctypes.byref(P()), R, I + 4, None))
    # a focus is not judged without a lens
    for f, p in ((gi.AovFrame(w, h, 5, 3, 5, 20), P()), (gi.AovFrame(w, h, 5, 3, 30, 3), P()), (fr, P(sample_begin=2, sample_end=2)),
                 (fr, P(sample_begin=0, sample_end=0, focus=float("nan")))):
        assert L.gi_sample_rays(C, ctypes.byref(f), ctypes.byref(p), R, I) == 0
        assert L.gi_sample_rays_device(C, ctypes.byref(f), ctypes.byref(p), R, I, None) == 0
    assert (rays == -7.0).all() and (ids["stream"] == 0).all()
    r, i = gi.sample_rays(cam, w, h, samples=(3, 3))
    assert r.shape == (0, 8) and i.shape == (0,)
    r, i = gi.sample_rays(cam, w, h, samples=2, window=(5, 3, 5, 20))
    assert r.shape == (0, 8) and i.shape == (0,)


def test_resolve_refusals_and_empty_calls():
    L = gi.lib()
    rows, rgb, rgb8 = np.full((5, 3, 3), 0.5), np.full((5, 3), -7.0), np.full((5, 3), 9, np.uint8)
    dp = ctypes.POINTER(ctypes.c_double)
    W, G, Q = rows.ctypes.data, rgb.ctypes.data, rgb8.ctypes.data

    def both(n, ns, r, g, q):
        m1 = _refused(L.gi_resolve_samples(n, ns, ctypes.cast(r, dp), g, q))
        m2 = _refused(L.gi_resolve_samples_device(n, ns, r, g, q, None))
        assert m1 == m2
        return m1
    assert "ns" in both(5, 0, W, G, Q)
    assert "ns" in both(5, -3, W, G, Q)
    both(-1, 3, W, G, Q)
    assert "null" in both(5, 3, W, None, None)
    assert "null rows" in both(5, 3, None, G, Q)
    assert "rows' buffer" in both(5, 3, W, W, Q)
    assert "rows' buffer" in both(5, 3, W, W, None)
    assert L.gi_resolve_samples(0, 3, ctypes.cast(W, dp), G, Q) == 0 and L.gi_resolve_samples_device(0, 3, W, G, Q, None) == 0
    assert L.gi_resolve_samples(0, 3, None, G, None) == 0
    assert (rgb == -7.0).all() and (rgb8 == 9).all() and (rows == 0.5).all()
    out = gi.resolve_samples(np.zeros((0, 4, 3)))
    assert out["rgb"].shape == (0, 3) and out["rgb8"].shape == (0, 3) and out["rgb8"].dtype == np.uint8


def test_wrappers_check_their_arguments_without_the_library(monkeypatch):
    """radiance, sample_rays* and resolve_samples* check shapes, dtypes, layouts, the window and the sample range in
    Python and raise ValueError before the library is touched (here: lib() would fail the test)."""
    cam = _cam()   # (gi_camera_init: host code)

    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(gi, "lib", no_lib)
    d = gi.DeviceScene.__new__(gi.DeviceScene)   # no scene: the checks come first
    good = np.zeros((5, gi.RAY_DOUBLES))
    for a in (np.zeros((5, 6)), np.zeros(8), good.astype(np.float32), np.zeros((5, 16))[:, ::2], np.asfortranarray(good), good.tolist()):
        with pytest.raises(ValueError):
            d.radiance(a, (0, 0, 1), 4)
    for ids in (np.zeros(4, gi.PATH_ID_DTYPE), np.zeros((5, 1), gi.PATH_ID_DTYPE), np.zeros(5, np.uint64), np.zeros((5, 2), np.uint64),
                np.zeros(10, gi.PATH_ID_DTYPE)[::2], [0] * 5):
        with pytest.raises(ValueError):
            d.radiance(good, (0, 0, 1), 4, ids=ids)
    for win in ((0, 0, 38, 21), (-1, 0, 37, 21), (30, 3, 5, 20), (0, 0, 37), (0.0, 0, 37, 21)):
        with pytest.raises(ValueError):
            gi.sample_rays(cam, 37, 21, window=win)
        with pytest.raises(ValueError):
            gi.sample_rays_device(cam, 37, 21, 1024, 2048, window=win)
    for smp in (-1, (2, 1), (-1, 2), (0, 1, 2), 2.0, (0, 2.0), True, 2 ** 31):
        with pytest.raises(ValueError):
            gi.sample_rays(cam, 37, 21, samples=smp)
        with pytest.raises(ValueError):
            gi.sample_rays_device(cam, 37, 21, 1024, 2048, samples=smp)
    for rows in (np.zeros((5, 3)), np.zeros((5, 2, 4)), np.zeros((5, 0, 3)), np.zeros((5, 2, 3), np.float32), np.zeros((5, 2, 6))[:, :, ::2],
                 np.zeros((5, 2, 3)).tolist()):
        with pytest.raises(ValueError):
            gi.resolve_samples(rows)
    for want in ((), ("rgb", "rgb"), ("mean",)):
        with pytest.raises(ValueError):
            gi.resolve_samples(np.zeros((5, 2, 3)), want=want)


def test_pinhole_sample_rays_restate_the_camera_rays_and_the_jitter():
    """sample_rays_np without a lens: the ids are (y w + x, s); without jitter d is the pixel direction whose
    normalisation is aov_frames.rays_np's d, bit for bit; with jitter d moves by less than a pixel and differs
    between samples; o is the camera position throughout."""
    sc, _, w, h = A.frame_scene("cornell/0.004")
    win = A.ODD_WINDOW
    x0, y0, x1, y1 = win
    rays, ids = RR.sample_rays_np(sc, w, h, win, 7, 0, 1, False, 0.0, 1.0)
    ref = A.rays_np(sc, w, h, win)
    assert U.bits_equal(A._norm(rays[:, 3:6]), ref[:, 3:6]).all() and U.bits_equal(rays[:, 0:3], ref[:, 0:3]).all()
    yy, xx = np.mgrid[y0:y1, x0:x1]
    assert (ids["stream"] == (yy * w + xx).reshape(-1)).all() and (ids["sample"] == 0).all() and (ids["reserved"] == 0).all()
    jr, jid = RR.sample_rays_np(sc, w, h, win, 7, 2, 5, True, 0.0, 1.0)
    assert jr.shape == (len(rays) * 3, 8) and (jid["sample"].reshape(-1, 3) == [2, 3, 4]).all()
    assert (jid["stream"].reshape(-1, 3) == ids["stream"][:, None]).all()
    assert np.isposinf(jr[:, 6]).all() and (jr[:, 7] == 0).all() and U.bits_equal(jr[:, 0:3], np.repeat(rays[:, 0:3], 3, 0)).all()
    step = np.abs(jr[:, 3:6].reshape(-1, 3, 3) - rays[:, None, 3:6]).max()
    assert 0 < step <= 2 * A.RES
    assert not U.bits_equal(jr[0::3, 3:6], jr[1::3, 3:6]).all(-1).any()


@pytest.mark.parametrize("aperture,focus", [(0.05, 3.0), (0.5, 11.0), (1e-3, 0.02)])
def test_lens_geometry(aperture, focus):
    """With aperture > 0 every ray of a pixel sample passes within 1e-12 (relative to the focus distance) of its
    focus point F, F lies at `focus` along forward from the camera, the origins lie on the lens disk (in the plane
    of the renders' left and up vectors, within `aperture` of its centre) and fill it, and the pinhole ray passes through F."""
    sc, _, w, h = A.frame_scene("cornell/0.01")
    sc.cam_pos = (-10.0, 0.5, 0.25)
    pos, f, up, left, tl = RR.camera_frame(sc, w)
    rays, ids, F = RR.sample_rays_np(sc, w, h, A.ODD_WINDOW, 3, 1, 4, True, aperture, focus, with_focus=True)
    pin, _ = RR.sample_rays_np(sc, w, h, A.ODD_WINDOW, 3, 1, 4, True, 0.0, focus)
    o, d = rays[:, 0:3], rays[:, 3:6]
    tol = 1e-12 * focus
    assert (np.abs((F - pos) @ f - focus) <= tol).all()
    # the point of the ray nearest F
    t = ((F - o) * d).sum(1) / (d * d).sum(1)
    assert (np.sqrt((((o + t[:, None] * d) - F) ** 2).sum(1)) <= tol).all()
    assert (np.abs(t - 1.0) <= 1e-12).all()   # d = F - o: F is the ray's point at t = 1
    dp = A._norm(pin[:, 3:6])
    tp = ((F - pos) * dp).sum(1)
    assert (np.sqrt((((pos + tp[:, None] * dp) - F) ** 2).sum(1)) <= tol).all()
    off = o - pos
    assert (np.abs(off @ np.cross(left, up)) <= 1e-12 * aperture).all()   # (up is the world's: not forward's normal plane)
    assert abs(left @ up) <= 1e-15
    rad = np.sqrt((off * off).sum(1))
    assert (rad <= aperture * (1 + 1e-12)).all() and rad.max() > 0.9 * aperture and rad.min() < 0.2 * aperture
    assert (ids["sample"].reshape(-1, 3) == [1, 2, 3]).all()
    assert (off @ left > 0).any() and (off @ left < 0).any() and (off @ up > 0).any() and (off @ up < 0).any()


def test_resolve_np_is_the_sequential_sum():
    rng = np.random.default_rng(5)
    rows = rng.random((40, 5, 3)) * 1.5
    want = np.zeros((40, 3))
    for i in range(40):
        for c in range(3):
            s = 0.0
            for k in range(5):
                s = s + rows[i, k, c]
            m = s / 5.0
            want[i, c] = m if m < 1.0 else 1.0
    got = RR.resolve_np(rows)
    assert U.bits_equal(got, want).all() and (got == 1.0).any() and (got < 1.0).any()
    assert U.bits_equal(RR.resolve_np(rows[:, :1]), np.where(rows[:, 0] < 1.0, rows[:, 0], 1.0)).all()
    assert (RR.quantize_np(np.array([[0.0, 1.0, 0.999]])) == [[0, 255, 254]]).all()
