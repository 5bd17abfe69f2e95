"""GPU: the denoiser (gi_denoise*; gi_denoise.hip k_dn_prep, k_dn_level) against its numpy restatement
(tests/denoise_ref.py, judged on the CPU by tests/test_denoise_host.py).  Everything compares bit for bit
(U.bits_equal): there is no tolerance anywhere in this file."""
import ctypes
import itertools

import numpy as np
import pytest

import aov_frames as A
import denoise_ref as D
import oracle_util as U
from x_scenes import with_env

pytestmark = pytest.mark.gpu

gi = U.pkg()
INF = float("inf")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    return torch


def syn_cam():
    return gi.Camera(D.SYN_CAM.cam_pos, D.SYN_CAM.cam_look, D.SYN_CAM.focal)


def device_dirs(cam, w, h, window):
    """(rows, cols, 3): the window's ray directions from the device's own camera rays."""
    x0, y0, x1, y1 = window if window is not None else (0, 0, w, h)
    return gi.camera_rays(cam, w, h, window=window)[:, 3:6].reshape(y1 - y0, x1 - x0, 3)


# levels 1..5 with and without the albedo stop; at 3 levels every combination of the stops and the normal power
CONFIGS = [dict(levels=k, albedo_stop=st, sigma_c=0.25, sigma_p=0.01, normal_pow_log2=5) for k in (1, 2, 3, 4, 5) for st in (True, False)] + \
          [dict(levels=3, albedo_stop=st, sigma_c=sc, sigma_p=sp, normal_pow_log2=k)
           for st, sc, sp, k in itertools.product((True, False), (0.1, INF), (0.02, INF), (0, 5))]
# (w, h, window): whole frames -- 131 x 67 crosses the 64 x 4 workgroup tiles in both directions at every step, at
# step 16 many pixels keep the centre tap alone -- and windows of one pixel, one column, one row, and the odd window
SHAPES = [(37, 21, None), (64, 40, None), (131, 67, None), (37, 21, (11, 7, 12, 8)), (64, 40, (63, 9, 64, 32)),
          (64, 40, (3, 39, 26, 40)), (37, 21, A.ODD_WINDOW), (131, 67, (1, 2, 130, 66))]


@pytest.mark.parametrize("w,h,window", SHAPES)
def test_synthetic_frames_equal_the_reference(torch_cuda, w, h, window):
    """Seeded synthetic planes: out_rgb and out_rgb8 of the host form equal the restatement run with the
    device's own camera rays (absolute pixels of the window), for every configuration."""
    cam = syn_cam()
    x0, y0, x1, y1 = window if window is not None else (0, 0, w, h)
    rows, cols = y1 - y0, x1 - x0
    if window in ((11, 7, 12, 8), (63, 9, 64, 32), (3, 39, 26, 40)):
        assert (rows, cols) in ((1, 1), (23, 1), (1, 23))
    s = D.synthetic(rows, cols, seed=w * 1000 + rows, holes=0.15 if rows * cols > 1 else 0.0)
    dirs = device_dirs(cam, w, h, window)
    assert U.bits_equal(dirs, D.dirs_np(D.SYN_CAM, w, h, window)).all()
    for cfg in CONFIGS:
        ref, ref8 = D.denoise_np(D.SYN_CAM.cam_pos, dirs, s["rgb"], s["t"], s["normal"], s["albedo"], **cfg)
        alb = s["albedo"] if cfg["albedo_stop"] else None
        out = gi.denoise(cam, w, h, s["rgb"], s["t"], s["normal"], alb, window=window, **cfg)
        assert out["rgb"].shape == (rows, cols, 3) and out["rgb8"].shape == (rows, cols, 3) and out["rgb8"].dtype == np.uint8
        ne = ~U.bits_equal(out["rgb"], ref)
        assert not ne.any(), (cfg, int(ne.any(-1).sum()), out["rgb"][ne.any(-1)][:2], ref[ne.any(-1)][:2])
        assert (out["rgb8"] == ref8).all(), cfg
    if rows * cols > 500:   # the filter did something: most valid pixels changed at the defaults
        valid = s["t"] < INF
        out = gi.denoise(cam, w, h, s["rgb"], s["t"], s["normal"], s["albedo"], window=window)["rgb"]
        assert (~U.bits_equal(out[valid], s["rgb"][valid])).any(-1).mean() > 0.5
        assert U.bits_equal(out[~valid], s["rgb"][~valid]).all()


def test_levels_up_to_eight_and_every_normal_power(torch_cuda):
    """levels 6..8 (steps 32..128: beyond a 64 x 40 frame only the centre tap is left) and normal_pow_log2 0..7."""
    cam = syn_cam()
    w, h = 64, 40
    s = D.synthetic(h, w, seed=11)
    dirs = device_dirs(cam, w, h, None)
    for cfg in [dict(levels=k, normal_pow_log2=2) for k in (6, 7, 8)] + [dict(levels=2, normal_pow_log2=k) for k in range(8)]:
        ref, ref8 = D.denoise_np(D.SYN_CAM.cam_pos, dirs, s["rgb"], s["t"], s["normal"], s["albedo"], **cfg)
        out = gi.denoise(cam, w, h, s["rgb"], s["t"], s["normal"], s["albedo"], **cfg)
        assert U.bits_equal(out["rgb"], ref).all() and (out["rgb8"] == ref8).all(), cfg


def test_a_tall_frame_crosses_the_band_deal(torch_cuda):
    """23 x 1100: one tile column of 275 tiles -- the direct-gather levels (steps 4 and up) deal their tiles to the
    XCDs in spans of 8 bands x 16 tile rows = 128 tiles here, so two whole spans are dealt and 19 tiles keep their
    order; 70 x 540 has two tile columns (spans of 256 tiles: one whole span and 14 tiles)."""
    cam = syn_cam()
    for w, h in ((23, 1100), (70, 540)):
        s = D.synthetic(h, w, seed=h)
        dirs = device_dirs(cam, w, h, None)
        for cfg in (dict(levels=4, albedo_stop=True), dict(levels=5, albedo_stop=False, sigma_p=INF)):
            ref, ref8 = D.denoise_np(D.SYN_CAM.cam_pos, dirs, s["rgb"], s["t"], s["normal"], s["albedo"], **cfg)
            out = gi.denoise(cam, w, h, s["rgb"], s["t"], s["normal"], s["albedo"] if cfg["albedo_stop"] else None, **cfg)
            ne = ~U.bits_equal(out["rgb"], ref)
            assert not ne.any(), (w, h, cfg, int(ne.any(-1).sum()))
            assert (out["rgb8"] == ref8).all()


def test_an_all_invalid_frame_comes_back_unchanged(torch_cuda):
    cam = syn_cam()
    w, h = 37, 21
    s = D.synthetic(h, w, seed=2)
    t = np.full((h, w), INF)
    for stop in (True, False):
        out = gi.denoise(cam, w, h, s["rgb"], t, np.zeros((h, w, 3)), s["albedo"], levels=5, albedo_stop=stop)
        assert U.bits_equal(out["rgb"], s["rgb"]).all()
        assert (out["rgb8"] == np.trunc(255 * s["rgb"]).astype(np.uint8)).all()


def test_want_subsets(torch_cuda):
    """One output alone (the other pointer null) equals the same output of the full call."""
    cam = syn_cam()
    w, h = 37, 21
    s = D.synthetic(h, w, seed=4)
    both = gi.denoise(cam, w, h, s["rgb"], s["t"], s["normal"], s["albedo"])
    for levels in (1, 3):
        both = gi.denoise(cam, w, h, s["rgb"], s["t"], s["normal"], s["albedo"], levels=levels)
        a = gi.denoise(cam, w, h, s["rgb"], s["t"], s["normal"], s["albedo"], levels=levels, want=("rgb",))
        b = gi.denoise(cam, w, h, s["rgb"], s["t"], s["normal"], s["albedo"], levels=levels, want=("rgb8",))
        assert list(a) == ["rgb"] and list(b) == ["rgb8"]
        assert U.bits_equal(a["rgb"], both["rgb"]).all() and (b["rgb8"] == both["rgb8"]).all()


# ---- end to end -----------------------------------------------------------------------------------------
_devs = {}


def dev_of(name):
    if name not in _devs:
        sc, env = A.base_scene(name)
        _devs[name] = with_env(env, lambda: gi.DeviceScene.from_scene(sc))
    return _devs[name]


@pytest.mark.parametrize("key", ["cornell/0.01", "zoo"])
def test_render_aov_and_denoise_on_one_stream(torch_cuda, key):
    """render_device (Mode X, 4 spp, depth 4), render_aov_device and denoise_device on one non-default stream:
    the outputs equal the restatement run on the device's own planes and gi.camera_rays, out_rgb8 is
    trunc(255 out_rgb), the guarded tails of the outputs and of the scratch stay untouched, the inputs are not
    written, and the host form equals the device form."""
    torch = torch_cuda
    d = dev_of(A.FRAMES[key][0])
    sc, _, w, h = A.frame_scene(key)
    cam = gi.Camera(sc.cam_pos, sc.cam_look, sc.focal)
    n, pad = w * h, 64
    f64 = dict(dtype=torch.float64, device="cuda")
    rgb, t = torch.full((n * 3 + pad,), -7.0, **f64), torch.full((n + pad,), -7.0, **f64)
    nrm, alb = torch.full((n * 3 + pad,), -7.0, **f64), torch.full((n * 3 + pad,), -7.0, **f64)
    out, out8 = torch.full((n * 3 + pad,), -7.0, **f64), torch.full((n * 3 + pad,), 77, dtype=torch.uint8, device="cuda")
    kw = dict(levels=4, sigma_c=0.25, sigma_p=0.01, normal_pow_log2=5, albedo_stop=True)
    nbytes = gi.denoise_scratch_bytes(w, h, **kw)
    scratch = torch.full((nbytes + pad,), 77, dtype=torch.uint8, device="cuda")
    assert scratch.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    assert st.cuda_stream != 0
    d.render_device(cam, sc.light, w, h, rgb.data_ptr(), stream=st.cuda_stream, mode=gi.MODE_X, spp=4, depth=4, seed=1)
    d.render_aov_device(cam, w, h, d_t=t.data_ptr(), d_normal=nrm.data_ptr(), d_albedo=alb.data_ptr(), stream=st.cuda_stream)
    gi.denoise_device(cam, w, h, rgb.data_ptr(), t.data_ptr(), nrm.data_ptr(), alb.data_ptr(), scratch.data_ptr(), nbytes,
                      d_out_rgb=out.data_ptr(), d_out_rgb8=out8.data_ptr(), stream=st.cuda_stream, **kw)
    st.synchronize()
    h_rgb, h_t, h_n, h_a = (x.cpu().numpy() for x in (rgb, t, nrm, alb))
    h_out, h_out8, h_scr = out.cpu().numpy(), out8.cpu().numpy(), scratch.cpu().numpy()
    for a, m in ((h_rgb, 3 * n), (h_t, n), (h_n, 3 * n), (h_a, 3 * n), (h_out, 3 * n)):
        assert (a[m:] == -7.0).all()
    assert (h_out8[3 * n:] == 77).all() and (h_scr[nbytes:] == 77).all()
    frame, tt = h_rgb[:3 * n].reshape(h, w, 3), h_t[:n].reshape(h, w)
    nn, aa = h_n[:3 * n].reshape(h, w, 3), h_a[:3 * n].reshape(h, w, 3)
    one_shot, _ = d.render(cam, sc.light, w, h, mode=gi.MODE_X, spp=4, depth=4, seed=1)
    assert U.bits_equal(frame, one_shot).all()   # (the denoiser left its input alone)
    valid = tt < INF
    assert valid.sum() >= 40 and (~valid).sum() >= 40
    ref, ref8 = D.denoise_np(sc.cam_pos, device_dirs(cam, w, h, None), frame, tt, nn, aa, **kw)
    got = h_out[:3 * n].reshape(h, w, 3)
    ne = ~U.bits_equal(got, ref)
    assert not ne.any(), (key, int(ne.any(-1).sum()))
    got8 = h_out8[:3 * n].reshape(h, w, 3)
    assert (got8 == ref8).all() and (got8 == np.trunc(255 * got).astype(np.uint8)).all()
    assert (~U.bits_equal(got[valid], frame[valid])).any(-1).mean() > 0.5
    host = gi.denoise(cam, w, h, frame, tt, nn, aa, **kw)
    assert U.bits_equal(host["rgb"], got).all() and (host["rgb8"] == got8).all()
    # without the albedo stop the albedo plane may be null
    kw2 = dict(kw, albedo_stop=False, levels=2)
    gi.denoise_device(cam, w, h, rgb.data_ptr(), t.data_ptr(), nrm.data_ptr(), 0, scratch.data_ptr(), nbytes,
                      d_out_rgb=out.data_ptr(), stream=st.cuda_stream, **kw2)
    st.synchronize()
    ref, _ = D.denoise_np(sc.cam_pos, device_dirs(cam, w, h, None), frame, tt, nn, None, **kw2)
    assert U.bits_equal(out.cpu().numpy()[:3 * n].reshape(h, w, 3), ref).all()
    assert (out8.cpu().numpy() == h_out8).all()   # (a null out_rgb8 is not written)


def test_denoise_between_progressive_passes_leaves_the_frame_alone(torch_cuda):
    """A denoise of the first pass between two progressive passes: the final pass equals the one-shot frame."""
    key = "cornell/0.01"
    d = dev_of("cornell")
    sc, _, w, h = A.frame_scene(key)
    cam = gi.Camera(sc.cam_pos, sc.cam_look, sc.focal)
    kw = dict(mode=gi.MODE_X, spp=4, depth=4, seed=1)
    one_shot, one_shot8 = d.render(cam, sc.light, w, h, **kw)
    aov = d.render_aov(cam, w, h, want=("t", "normal", "albedo"))
    first, _ = d.render(cam, sc.light, w, h, samples=(0, 2), **kw)
    first = first.copy()
    pre = gi.denoise(cam, w, h, first, aov["t"], aov["normal"], aov["albedo"], sigma_c=0.5 / np.sqrt(2.0))
    rgb, rgb8 = d.render(cam, sc.light, w, h, samples=(2, 4), **kw)
    assert U.bits_equal(rgb, one_shot).all() and (rgb8 == one_shot8).all()
    ref, ref8 = D.denoise_np(sc.cam_pos, device_dirs(cam, w, h, None), first, aov["t"], aov["normal"], aov["albedo"],
                             sigma_c=0.5 / np.sqrt(2.0))
    assert U.bits_equal(pre["rgb"], ref).all() and (pre["rgb8"] == ref8).all()


# ---- argument errors ------------------------------------------------------------------------------------
def test_argument_errors(torch_cuda):
    """Every GI_ERR_ARG case of gi.h, with a message and before anything is launched; the empty window returns
    GI_OK and writes nothing."""
    torch = torch_cuda
    cam = syn_cam()
    w, h = 37, 21
    n = w * h
    L = gi.lib()
    s = D.synthetic(h, w, seed=6)
    o_rgb, o_rgb8 = np.full((h, w, 3), -7.0), np.full((h, w, 3), 77, np.uint8)
    f64 = dict(dtype=torch.float64, device="cuda")
    d_in = {k: torch.tensor(s[k].reshape(-1), **f64) for k in ("rgb", "t", "normal", "albedo")}
    d_out, d_out8 = torch.full((3 * n,), -7.0, **f64), torch.full((3 * n,), 77, dtype=torch.uint8, device="cuda")
    nbytes = gi.denoise_scratch_bytes(w, h)
    d_scr = torch.full((nbytes + 16,), 77, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert d_scr.data_ptr() % 16 == 0

    good_f, good_p = gi.AovFrame(w, h, 0, 0, w, h), gi.DenoiseParams(4, 5, 1, 0, 0.25, 0.01)

    def host_io(**kw):
        v = dict(rgb=s["rgb"].ctypes.data, t=s["t"].ctypes.data, normal=s["normal"].ctypes.data, albedo=s["albedo"].ctypes.data,
                 out_rgb=o_rgb.ctypes.data, out_rgb8=o_rgb8.ctypes.data)
        v.update(kw)
        return gi.DenoiseIO(**v)

    def dev_io(**kw):
        v = dict(rgb=d_in["rgb"].data_ptr(), t=d_in["t"].data_ptr(), normal=d_in["normal"].data_ptr(),
                 albedo=d_in["albedo"].data_ptr(), out_rgb=d_out.data_ptr(), out_rgb8=d_out8.data_ptr())
        v.update(kw)
        return gi.DenoiseIO(**v)

    def ref(x):
        return ctypes.byref(x) if x is not None else None

    def both(c=cam._c, f=good_f, p=good_p, io_kw=None, io_null=False):
        """(host status, device status) of one argument set."""
        hio, dio = (None, None) if io_null else (host_io(**(io_kw or {})), dev_io(**(io_kw or {})))
        return (L.gi_denoise(ref(c), ref(f), ref(p), ref(hio)),
                L.gi_denoise_device(ref(c), ref(f), ref(p), ref(dio), d_scr.data_ptr(), nbytes, None))

    def refused(rcs):
        for rc in (rcs if isinstance(rcs, tuple) else (rcs,)):
            assert rc == -1 and len(L.gi_last_error()) > 0, (rcs, L.gi_last_error())
    # null cam, frame, p, io
    refused(both(c=None))
    refused(both(f=None))
    refused(both(p=None))
    refused(both(io_null=True))
    # null rgb, t, normal; both outputs null; albedo null with the stop; out_rgb == rgb
    for k in ("rgb", "t", "normal"):
        refused(both(io_kw={k: None}))
    refused(both(io_kw=dict(out_rgb=None, out_rgb8=None)))
    refused(both(io_kw=dict(albedo=None)))
    refused(L.gi_denoise(ref(cam._c), ref(good_f), ref(good_p), ref(host_io(out_rgb=s["rgb"].ctypes.data))))
    refused(L.gi_denoise_device(ref(cam._c), ref(good_f), ref(good_p), ref(dev_io(out_rgb=d_in["rgb"].data_ptr())),
                                d_scr.data_ptr(), nbytes, None))
    # parameters out of range or NaN
    for p in (gi.DenoiseParams(0, 5, 1, 0, 0.25, 0.01), gi.DenoiseParams(9, 5, 1, 0, 0.25, 0.01), gi.DenoiseParams(4, -1, 1, 0, 0.25, 0.01),
              gi.DenoiseParams(4, 8, 1, 0, 0.25, 0.01), gi.DenoiseParams(4, 5, 2, 0, 0.25, 0.01), gi.DenoiseParams(4, 5, 3, 0, 0.25, 0.01),
              gi.DenoiseParams(4, 5, 1, 1, 0.25, 0.01), gi.DenoiseParams(4, 5, 1, 0, 0.0, 0.01), gi.DenoiseParams(4, 5, 1, 0, -0.25, 0.01),
              gi.DenoiseParams(4, 5, 1, 0, np.nan, 0.01), gi.DenoiseParams(4, 5, 1, 0, 0.25, 0.0), gi.DenoiseParams(4, 5, 1, 0, 0.25, -INF),
              gi.DenoiseParams(4, 5, 1, 0, 0.25, np.nan)):
        refused(both(p=p))
    # frame sizes and windows, as gi_render_aov judges them
    for f in (gi.AovFrame(0, h, 0, 0, 0, h), gi.AovFrame(w, 0, 0, 0, w, 0), gi.AovFrame(-1, h, 0, 0, 1, h), gi.AovFrame(w, h, 0, 0, w + 1, h),
              gi.AovFrame(w, h, 0, 0, w, h + 1), gi.AovFrame(w, h, -1, 0, w, h), gi.AovFrame(w, h, 0, -1, w, h),
              gi.AovFrame(w, h, 30, 3, 5, 20), gi.AovFrame(w, h, 5, 20, 30, 3)):
        refused(both(f=f))
    # a non-finite camera field
    for field, i in (("pos", 0), ("up", 1), ("forward", 2), ("focal", None)):
        for v in (np.nan, np.inf, -np.inf):
            c2 = gi.CameraDesc.from_buffer_copy(cam._c)
            if i is None:
                setattr(c2, field, v)
            else:
                getattr(c2, field)[i] = v
            refused(both(c=c2))
    # the scratch: too small, null, misaligned
    dio = dev_io()
    args = (ref(cam._c), ref(good_f), ref(good_p), ref(dio))
    refused(L.gi_denoise_device(*args, d_scr.data_ptr(), nbytes - 1, None))
    refused(L.gi_denoise_device(*args, d_scr.data_ptr(), 0, None))
    refused(L.gi_denoise_device(*args, d_scr.data_ptr(), -5, None))
    refused(L.gi_denoise_device(*args, None, nbytes, None))
    refused(L.gi_denoise_device(*args, d_scr.data_ptr() + 8, nbytes, None))
    with pytest.raises(gi.GIError, match=r"\(-1\)"):
        gi.denoise_device(cam, w, h, d_in["rgb"].data_ptr(), d_in["t"].data_ptr(), d_in["normal"].data_ptr(), d_in["albedo"].data_ptr(),
                          d_scr.data_ptr(), nbytes)   # both outputs null
    # the empty window: GI_OK, nothing launched, nothing written (no scratch needed)
    for f in (gi.AovFrame(w, h, 5, 3, 5, 20), gi.AovFrame(w, h, 5, 3, 30, 3), gi.AovFrame(w, h, w, h, w, h)):
        assert both(f=f) == (0, 0)
        assert L.gi_denoise_device(ref(cam._c), ref(f), ref(good_p), ref(dio), None, 0, None) == 0
    torch.cuda.synchronize()
    assert (o_rgb == -7.0).all() and (o_rgb8 == 77).all()
    assert (d_out.cpu().numpy() == -7.0).all() and (d_out8.cpu().numpy() == 77).all() and (d_scr.cpu().numpy() == 77).all()
    for k in d_in:
        assert U.bits_equal(d_in[k].cpu().numpy(), s[k].reshape(-1)).all()
    e = gi.denoise(cam, w, h, np.zeros((17, 0, 3)), np.zeros((17, 0)), np.zeros((17, 0, 3)), np.zeros((17, 0, 3)), window=(5, 3, 5, 20))
    assert e["rgb"].shape == (17, 0, 3) and e["rgb8"].shape == (17, 0, 3)
    # and a good call after all of that still works
    assert both() == (0, 0)
    torch.cuda.synchronize()
    r, r8 = D.denoise_np(D.SYN_CAM.cam_pos, device_dirs(cam, w, h, None), s["rgb"], s["t"], s["normal"], s["albedo"])
    assert U.bits_equal(o_rgb, r).all() and (o_rgb8 == r8).all()
    assert U.bits_equal(d_out.cpu().numpy().reshape(h, w, 3), r).all() and (d_out8.cpu().numpy().reshape(h, w, 3) == r8).all()
