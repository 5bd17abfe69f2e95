"""GPU: the sample moments of the retained Mode X frame (gi_frame_samples_info, gi_frame_moments*; gi_kernels.hip
k_x_moments, k_x_moments_fill) against the CPU oracle's frames and the numpy restatement (tests/moments_ref.py).
Everything compares bit for bit (U.bits_equal): there is no tolerance anywhere in this file."""
import numpy as np
import pytest

import aov_frames as A
import moments_ref as M
import oracle_util as U
from x_scenes import with_env

pytestmark = pytest.mark.gpu

gi = U.pkg()
DEPTH, SEED = 4, 1
SPPS = (2, 3, 8)
FORMS = {"default": 0, "mega": gi.FLAG_X_MEGA, "wf": gi.FLAG_X_WF, "seg": gi.FLAG_X_SEG}
# (frame key, w, h): cornell/0.01 at 37 x 21 has background pixels; zoo is read from HBM (not staged in LDS)
CASES = {"cornell": ("cornell/0.01", 37, 21), "zoo": ("zoo", 37, 21)}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    return torch


_devs, _oracle = {}, {}


def setup(case):
    """(device scene, scene, camera, w, h) of a case; the device scene is built once."""
    key, w, h = CASES[case]
    sc, env, _, _ = A.frame_scene(key)
    if case not in _devs:
        _devs[case] = with_env(env, lambda: gi.DeviceScene.from_scene(sc))
    return _devs[case], sc, gi.Camera(sc.cam_pos, sc.cam_look, sc.focal), w, h


def oracle_frame(case, w, h, k):
    """The oracle's Mode X frame of spp = k as (h, w, 3); computed once, read-only."""
    if (case, w, h, k) not in _oracle:
        sc = A.frame_scene(CASES[case][0])[0]
        f = U.oracle_render(sc.to_scn(), w, h, mode=1, spp=k, depth=DEPTH, seed=SEED)["rgb"].reshape(h, w, 3)
        f.setflags(write=False)
        _oracle[(case, w, h, k)] = f
    return _oracle[(case, w, h, k)]


def check_frame(case, d, w, h, n, rgb, m):
    """Every bit-for-bit property of a whole frame's moments m (mean, var, samples) after n samples."""
    s = m["samples"]
    assert s.shape == (h, w, n, 3) and m["mean"].shape == m["var"].shape == (h, w, 3)
    run = M.running_frames_np(s)
    for k in range(2, n + 1):   # the rows are the oracle's samples: every prefix sums to the oracle's frame
        ne = ~U.bits_equal(run[k], oracle_frame(case, w, h, k))
        assert not ne.any(), (case, n, k, int(ne.any(-1).sum()))
    mean, var = M.moments_np(s)
    assert U.bits_equal(m["mean"], mean).all() and U.bits_equal(m["var"], var).all()
    assert U.bits_equal(np.where(m["mean"] < 1.0, m["mean"], 1.0), rgb).all()
    return (s == 0).all((-1, -2))   # the pixels without a row (or whose every sample is black)


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("case", list(CASES))
def test_rows_mean_and_variance_of_every_form(torch_cuda, case, form):
    d, sc, cam, w, h = setup(case)
    if case == "zoo":
        assert d.info()["x_lds_resident"] == 0
    for spp in SPPS:
        rgb, _ = d.render(cam, sc.light, w, h, mode=gi.MODE_X, spp=spp, depth=DEPTH, seed=SEED, flags=FORMS[form])
        assert d.frame_samples_info() == dict(w=w, h=h, n=spp, spp=spp)
        m = d.frame_moments(w, h, want=("mean", "var", "samples"))
        zero = check_frame(case, d, w, h, spp, rgb, m)
        # unlisted pixels are +0 in every output, sign included
        z = np.zeros(1)
        assert U.bits_equal(m["mean"][zero], z).all() and U.bits_equal(m["var"][zero], z).all()
        assert (~zero).sum() >= 100   # (the frames with many unlisted pixels: test_a_frame_of_several_blocks)
        # each output alone equals the same output of the full call
        for k in gi.MOMENTS_OUTPUTS:
            one = d.frame_moments(w, h, want=(k,))
            assert list(one) == [k] and U.bits_equal(one[k], m[k]).all()
    assert (m["var"] > 0).any()


def test_a_frame_of_several_blocks(torch_cuda):
    """131 x 67: 8777 pixels, more than one workgroup of every kernel and no multiple of a tile or a wave."""
    d, sc, cam, _, _ = setup("cornell")
    w, h, spp = 131, 67, 3
    rgb, _ = d.render(cam, sc.light, w, h, mode=gi.MODE_X, spp=spp, depth=DEPTH, seed=SEED)
    m = d.frame_moments(w, h, want=("mean", "var", "samples"))
    zero = check_frame("cornell", d, w, h, spp, rgb, m)
    assert zero.sum() >= 1000 and (~zero).sum() >= 1000
    assert (m["mean"][zero] == 0).all() and (m["var"][zero] == 0).all()


def test_windows_equal_the_slices_of_the_whole_frame(torch_cuda):
    d, sc, cam, w, h = setup("cornell")
    d.render(cam, sc.light, w, h, mode=gi.MODE_X, spp=3, depth=DEPTH, seed=SEED)
    full = d.frame_moments(w, h, want=("mean", "var", "samples"))
    for win in (A.ODD_WINDOW, (17, 11, 18, 12), (3, 20, 26, 21), (36, 0, 37, 21), (0, 0, w, h)):
        x0, y0, x1, y1 = win
        part = d.frame_moments(w, h, window=win, want=("mean", "var", "samples"))
        for k in gi.MOMENTS_OUTPUTS:
            assert part[k].shape[:2] == (y1 - y0, x1 - x0)
            assert U.bits_equal(part[k], full[k][y0:y1, x0:x1]).all(), (win, k)
    e = d.frame_moments(w, h, window=(5, 3, 5, 20))   # an empty window: GI_OK, nothing written
    assert e["mean"].shape == (17, 0, 3)


@pytest.mark.parametrize("form", ["default", "mega"])
def test_progressive_passes(torch_cuda, form):
    """Passes (0, 2), (2, 3), (3, 8) of an 8-spp frame with a moments call after each: n follows the passes, each
    result is the one-shot frame's first n samples, and the calls do not end the progressive frame."""
    d, sc, cam, w, h = setup("cornell")
    kw = dict(mode=gi.MODE_X, spp=8, depth=DEPTH, seed=SEED, flags=FORMS[form])
    one_shot, one_shot8 = d.render(cam, sc.light, w, h, **kw)
    full = d.frame_moments(w, h, want=("samples",))["samples"]
    for b, e in ((0, 2), (2, 3), (3, 8)):
        rgb, rgb8 = d.render(cam, sc.light, w, h, samples=(b, e), **kw)
        assert d.frame_samples_info() == dict(w=w, h=h, n=e, spp=8)
        m = d.frame_moments(w, h, want=("mean", "var", "samples"))
        assert U.bits_equal(m["samples"], full[:, :, :e]).all()
        check_frame("cornell", d, w, h, e, rgb, m)
    assert U.bits_equal(rgb, one_shot).all() and (rgb8 == one_shot8).all()


def test_device_form_on_other_streams_is_ordered_with_the_renders(torch_cuda):
    """render_device on one stream, frame_moments_device on another with no host synchronisation between them, then
    the scene's next render (another seed, which overwrites the rows) on the first stream: the moments are the
    first frame's, equal to the host form, and the guarded tails of the outputs stay untouched."""
    torch = torch_cuda
    d, sc, cam, w, h = setup("cornell")
    n, spp, pad = w * h, 8, 64
    kw = dict(mode=gi.MODE_X, spp=spp, depth=DEPTH)
    d.render(cam, sc.light, w, h, seed=SEED, **kw)
    host = d.frame_moments(w, h, want=("mean", "var", "samples"))
    f64 = dict(dtype=torch.float64, device="cuda")
    rgb, rgb2 = torch.full((3 * n,), -7.0, **f64), torch.full((3 * n,), -7.0, **f64)
    mean, var = torch.full((3 * n + pad,), -7.0, **f64), torch.full((3 * n + pad,), -7.0, **f64)
    smp = torch.full((3 * n * spp + pad,), -7.0, **f64)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    assert s1.cuda_stream != 0 and s2.cuda_stream != 0
    d.render_device(cam, sc.light, w, h, rgb.data_ptr(), stream=s1.cuda_stream, seed=SEED, **kw)
    d.frame_moments_device(w, h, d_mean=mean.data_ptr(), d_var=var.data_ptr(), d_samples=smp.data_ptr(), stream=s2.cuda_stream)
    d.render_device(cam, sc.light, w, h, rgb2.data_ptr(), stream=s1.cuda_stream, seed=SEED + 1, **kw)
    torch.cuda.synchronize()
    for a, m, k in ((mean, 3 * n, "mean"), (var, 3 * n, "var"), (smp, 3 * n * spp, "samples")):
        a = a.cpu().numpy()
        assert (a[m:] == -7.0).all()
        assert U.bits_equal(a[:m], host[k].reshape(-1)).all(), k
    assert not U.bits_equal(rgb.cpu().numpy(), rgb2.cpu().numpy()).all()
    # a window and one output alone on a stream
    x0, y0, x1, y1 = A.ODD_WINDOW
    m = (x1 - x0) * (y1 - y0)
    d.render_device(cam, sc.light, w, h, rgb.data_ptr(), stream=s1.cuda_stream, seed=SEED, **kw)
    var.fill_(-7.0)
    torch.cuda.synchronize()
    d.frame_moments_device(w, h, window=A.ODD_WINDOW, d_var=var.data_ptr(), stream=s2.cuda_stream)
    torch.cuda.synchronize()
    a = var.cpu().numpy()
    assert (a[3 * m:] == -7.0).all() and U.bits_equal(a[:3 * m].reshape(y1 - y0, x1 - x0, 3), host["var"][y0:y1, x0:x1]).all()
    assert (mean.cpu().numpy()[:3 * n] == host["mean"].reshape(-1)).all()   # (a null output is not written)


def test_refusals(torch_cuda):
    """GI_ERR_ARG, with a message: a fresh scene; after a Mode R render, spp = 1, two shards, a banded gi_render, a
    pass (0, 1); a frame of another size; null arguments; and a good call after all of that."""
    import ctypes
    torch = torch_cuda
    L = gi.lib()
    sc, env, _, _ = A.frame_scene("cornell/0.01")
    w, h = 37, 21
    cam = gi.Camera(sc.cam_pos, sc.cam_look, sc.focal)
    d = with_env(env, lambda: gi.DeviceScene.from_scene(sc))
    kw = dict(mode=gi.MODE_X, depth=DEPTH, seed=SEED)

    def refused():
        with pytest.raises(gi.GIError, match=r"\(-1\)"):
            d.frame_samples_info()
        with pytest.raises(gi.GIError, match=r"\(-1\)"):
            d.frame_moments(w, h)
        assert len(L.gi_last_error()) > 0

    def good():
        d.render(cam, sc.light, w, h, spp=3, **kw)
        assert d.frame_samples_info()["n"] == 3
        return d.frame_moments(w, h)
    refused()                                              # a fresh scene
    first = good()
    d.render(cam, sc.light, w, h, mode=gi.MODE_R)
    refused()
    good()
    d.render(cam, sc.light, w, h, spp=1, **kw)
    refused()
    good()
    buf = torch.zeros(int(L.gi_shard_tiles(w, h, 2)) * 64 * 3, dtype=torch.float64, device="cuda")
    d.render_device(cam, sc.light, w, h, buf.data_ptr(), spp=3, shard_count=2, shard_index=0, **kw)
    torch.cuda.synchronize()
    refused()
    good()
    d.render(cam, sc.light, w, h, spp=3, band_rows=8, **kw)
    refused()
    good()
    d.render(cam, sc.light, w, h, spp=3, samples=(0, 1), **kw)
    assert d.frame_samples_info()["n"] == 1                # retained, but one sample has no variance
    with pytest.raises(gi.GIError, match=r"\(-1\)"):
        d.frame_moments(w, h)
    d.render(cam, sc.light, w, h, spp=3, samples=(1, 3), **kw)   # (the refused call did not end the frame)
    assert U.bits_equal(d.frame_moments(w, h)["mean"], first["mean"]).all()
    with pytest.raises(gi.GIError, match=r"\(-1\)"):
        d.render(cam, sc.light, w, h, spp=0, **kw)         # a refused render ends the retained frame
    refused()
    good()
    for fw, fh in ((w + 1, h), (w, h - 1), (64, 40)):      # a frame of another size
        with pytest.raises(gi.GIError, match=r"\(-1\)"):
            d.frame_moments(fw, fh)
    # null struct, null frame, every output null; bad windows as gi_render_aov judges them
    fr, out = gi.AovFrame(w, h, 0, 0, w, h), np.zeros((h, w, 3))
    m = gi.Moments(out.ctypes.data, None, None)
    assert L.gi_frame_moments(d._h, None, ctypes.byref(m)) == -1
    assert L.gi_frame_moments(d._h, ctypes.byref(fr), None) == -1
    assert L.gi_frame_moments_device(d._h, ctypes.byref(fr), None, None) == -1
    assert L.gi_frame_moments(d._h, ctypes.byref(fr), ctypes.byref(gi.Moments(None, None, None))) == -1
    assert L.gi_frame_moments_device(d._h, ctypes.byref(fr), ctypes.byref(gi.Moments(None, None, None)), None) == -1
    for f in (gi.AovFrame(w, h, 0, 0, w + 1, h), gi.AovFrame(w, h, -1, 0, w, h), gi.AovFrame(w, h, 30, 3, 5, 20)):
        assert L.gi_frame_moments(d._h, ctypes.byref(f), ctypes.byref(m)) == -1 and len(L.gi_last_error()) > 0
    assert (out == 0).all()
    assert L.gi_frame_moments(d._h, ctypes.byref(fr), ctypes.byref(m)) == 0
    assert U.bits_equal(out, first["mean"]).all()
    d.close()
