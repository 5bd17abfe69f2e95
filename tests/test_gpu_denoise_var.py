"""GPU: the variance-guided denoiser (gi_denoise_var*; gi_denoise.hip k_dnv_g, k_dnv_level) against its numpy
restatement (tests/denoise_var_ref.py, judged on the CPU by tests/test_denoise_var_host.py), and end to end behind
the sample moments.  The comparisons with the restatement are bit for bit (U.bits_equal): no tolerance; the end
to end test asserts the project's quality condition."""
import itertools

import numpy as np
import pytest

import aov_frames as A
import denoise_ref as D
import denoise_var_ref as DV
import oracle_util as U
from test_gpu_denoise import SHAPES, dev_of, device_dirs, syn_cam

pytestmark = pytest.mark.gpu

gi = U.pkg()
INF = float("inf")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    return torch


# levels 1..5 with and without the albedo stop; at 3 levels every combination of the stops and the normal power
CONFIGS = [dict(levels=k, albedo_stop=st, sigma_v=1.0, sigma_p=0.02, var_floor=1e-6, normal_pow_log2=5) for k in (1, 2, 3, 4, 5)
           for st in (True, False)] + \
          [dict(levels=3, albedo_stop=st, sigma_v=sv, sigma_p=sp, var_floor=1e-4, normal_pow_log2=k)
           for st, sv, sp, k in itertools.product((True, False), (1.0, INF), (0.02, INF), (0, 5))]


def compare(cam, w, h, window, s, var, dirs, cfg, want=gi.DENOISE_VAR_OUTPUTS):
    cfg = dict(dict(sigma_v=1.0, var_floor=1e-6), **cfg)   # (both sides get every stop explicitly)
    ref, refv, ref8 = DV.denoise_var_np(D.SYN_CAM.cam_pos, dirs, s["rgb"], var, s["t"], s["normal"], s["albedo"], **cfg)
    out = gi.denoise_var(cam, w, h, s["rgb"], var, s["t"], s["normal"], s["albedo"] if cfg.get("albedo_stop", True) else None,
                         window=window, want=want, **cfg)
    assert list(out) == list(want)
    for k, r in (("rgb", ref), ("var", refv)):
        if k in want:
            ne = ~U.bits_equal(out[k], r)
            assert not ne.any(), (cfg, k, int(ne.any(-1).sum()), out[k][ne.any(-1)][:2], r[ne.any(-1)][:2])
    if "rgb8" in want:
        assert out["rgb8"].dtype == np.uint8 and (out["rgb8"] == ref8).all(), cfg
    return out


@pytest.mark.parametrize("w,h,window", SHAPES)
def test_synthetic_frames_equal_the_reference(torch_cuda, w, h, window):
    """Seeded synthetic planes and a seeded non-negative variance with regions of exact zeros: out_rgb, out_var and
    out_rgb8 of the host form equal the restatement run with the device's own camera rays, for every configuration."""
    cam = syn_cam()
    x0, y0, x1, y1 = window if window is not None else (0, 0, w, h)
    rows, cols = y1 - y0, x1 - x0
    s = D.synthetic(rows, cols, seed=w * 1000 + rows, holes=0.15 if rows * cols > 1 else 0.0)
    var = DV.synthetic_var(rows, cols, seed=w + rows)
    if rows * cols > 500:
        assert (var == 0).all(-1).mean() > 0.2 and (var > 0).all(-1).mean() > 0.4
    dirs = device_dirs(cam, w, h, window)
    for cfg in CONFIGS:
        out = compare(cam, w, h, window, s, var, dirs, cfg)
    if rows * cols > 500:   # the filter did something, and left the invalid pixels alone
        valid = s["t"] < INF
        assert (~U.bits_equal(out["rgb"][valid], s["rgb"][valid])).any(-1).mean() > 0.5
        assert U.bits_equal(out["rgb"][~valid], s["rgb"][~valid]).all() and U.bits_equal(out["var"][~valid], var[~valid]).all()


def test_levels_up_to_eight(torch_cuda):
    cam = syn_cam()
    w, h = 64, 40
    s, var = D.synthetic(h, w, seed=11), DV.synthetic_var(h, w, seed=11)
    dirs = device_dirs(cam, w, h, None)
    for k in (6, 7, 8):
        compare(cam, w, h, None, s, var, dirs, dict(levels=k, normal_pow_log2=2, sigma_v=2.0))


def test_a_tall_frame_crosses_the_band_deal(torch_cuda):
    """23 x 1100 and 70 x 540: the level kernels deal their tiles to the XCDs in spans (test_gpu_denoise.py)."""
    cam = syn_cam()
    for w, h in ((23, 1100), (70, 540)):
        s, var = D.synthetic(h, w, seed=h), DV.synthetic_var(h, w, seed=h)
        dirs = device_dirs(cam, w, h, None)
        for cfg in (dict(levels=4, albedo_stop=True, sigma_v=1.0), dict(levels=5, albedo_stop=False, sigma_p=INF, sigma_v=2.0)):
            compare(cam, w, h, None, s, var, dirs, cfg)


def test_an_all_invalid_frame_comes_back_unchanged(torch_cuda):
    cam = syn_cam()
    w, h = 37, 21
    s, var = D.synthetic(h, w, seed=2), DV.synthetic_var(h, w, seed=2)
    t = np.full((h, w), INF)
    for stop in (True, False):
        out = gi.denoise_var(cam, w, h, s["rgb"], var, t, np.zeros((h, w, 3)), s["albedo"], levels=5, albedo_stop=stop)
        assert U.bits_equal(out["rgb"], s["rgb"]).all() and U.bits_equal(out["var"], var).all()
        assert (out["rgb8"] == np.trunc(255 * s["rgb"]).astype(np.uint8)).all()


def test_want_subsets(torch_cuda):
    """Every non-empty selection of the outputs (the other pointers null) equals the same outputs of the full call."""
    cam = syn_cam()
    w, h = 37, 21
    s, var = D.synthetic(h, w, seed=4), DV.synthetic_var(h, w, seed=4)
    dirs = device_dirs(cam, w, h, None)
    for levels in (1, 3):
        for r in (1, 2):
            for want in itertools.combinations(gi.DENOISE_VAR_OUTPUTS, r):
                compare(cam, w, h, None, s, var, dirs, dict(levels=levels, sigma_v=1.0), want=want)


@pytest.mark.parametrize("w,h", [(37, 21), (64, 40)])
def test_one_level_equals_gi_denoise_at_the_same_stop(torch_cuda, w, h):
    """var = 1/16, sigma_v = 1, var_floor = 1/16: sigma2 = 1/4 at every valid pixel, so one level is gi_denoise's
    level at sigma_c = 0.5 -- the two device filters agree bit for bit."""
    cam = syn_cam()
    s = D.synthetic(h, w, seed=w)
    var = np.full((h, w, 3), 0.0625)
    for stop in (True, False):
        a = gi.denoise_var(cam, w, h, s["rgb"], var, s["t"], s["normal"], s["albedo"], levels=1, sigma_v=1.0, var_floor=0.0625,
                           albedo_stop=stop)
        b = gi.denoise(cam, w, h, s["rgb"], s["t"], s["normal"], s["albedo"], levels=1, sigma_c=0.5, albedo_stop=stop)
        assert U.bits_equal(a["rgb"], b["rgb"]).all() and (a["rgb8"] == b["rgb8"]).all()


def test_device_form_on_a_stream(torch_cuda):
    """denoise_var_device on a non-default stream equals the host form; guarded tails of the outputs and of the
    scratch stay untouched and the inputs are not written."""
    torch = torch_cuda
    cam = syn_cam()
    w, h, pad = 64, 40, 64
    n = w * h
    s, var = D.synthetic(h, w, seed=8), DV.synthetic_var(h, w, seed=8)
    kw = dict(levels=4, sigma_v=2.0, sigma_p=0.01, var_floor=1e-6, normal_pow_log2=5, albedo_stop=True)
    host = gi.denoise_var(cam, w, h, s["rgb"], var, s["t"], s["normal"], s["albedo"], **kw)
    f64 = dict(dtype=torch.float64, device="cuda")
    ins = {k: torch.tensor(a.reshape(-1), **f64) for k, a in (("rgb", s["rgb"]), ("var", var), ("t", s["t"]), ("normal", s["normal"]),
                                                              ("albedo", s["albedo"]))}
    out, ov = torch.full((3 * n + pad,), -7.0, **f64), torch.full((3 * n + pad,), -7.0, **f64)
    out8 = torch.full((3 * n + pad,), 77, dtype=torch.uint8, device="cuda")
    nbytes = gi.denoise_var_scratch_bytes(w, h, **kw)
    scratch = torch.full((nbytes + pad,), 77, dtype=torch.uint8, device="cuda")
    assert scratch.data_ptr() % 16 == 0
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    gi.denoise_var_device(cam, w, h, ins["rgb"].data_ptr(), ins["var"].data_ptr(), ins["t"].data_ptr(), ins["normal"].data_ptr(),
                          ins["albedo"].data_ptr(), scratch.data_ptr(), nbytes, d_out_rgb=out.data_ptr(), d_out_var=ov.data_ptr(),
                          d_out_rgb8=out8.data_ptr(), stream=st.cuda_stream, **kw)
    st.synchronize()
    o, v, o8 = out.cpu().numpy(), ov.cpu().numpy(), out8.cpu().numpy()
    assert (o[3 * n:] == -7.0).all() and (v[3 * n:] == -7.0).all() and (o8[3 * n:] == 77).all()
    assert (scratch.cpu().numpy()[nbytes:] == 77).all()
    assert U.bits_equal(o[:3 * n], host["rgb"].reshape(-1)).all() and U.bits_equal(v[:3 * n], host["var"].reshape(-1)).all()
    assert (o8[:3 * n] == host["rgb8"].reshape(-1)).all()
    for k, a in (("rgb", s["rgb"]), ("var", var), ("t", s["t"])):
        assert U.bits_equal(ins[k].cpu().numpy(), a.reshape(-1)).all()
    # bad arguments of the device form: too little scratch, every output null, out_var == var
    with pytest.raises(gi.GIError, match=r"\(-1\)"):
        gi.denoise_var_device(cam, w, h, ins["rgb"].data_ptr(), ins["var"].data_ptr(), ins["t"].data_ptr(), ins["normal"].data_ptr(),
                              ins["albedo"].data_ptr(), scratch.data_ptr(), nbytes - 1, d_out_rgb=out.data_ptr(), **kw)
    with pytest.raises(gi.GIError, match=r"\(-1\)"):
        gi.denoise_var_device(cam, w, h, ins["rgb"].data_ptr(), ins["var"].data_ptr(), ins["t"].data_ptr(), ins["normal"].data_ptr(),
                              ins["albedo"].data_ptr(), scratch.data_ptr(), nbytes, **kw)
    with pytest.raises(gi.GIError, match=r"\(-1\)"):
        gi.denoise_var_device(cam, w, h, ins["rgb"].data_ptr(), ins["var"].data_ptr(), ins["t"].data_ptr(), ins["normal"].data_ptr(),
                              ins["albedo"].data_ptr(), scratch.data_ptr(), nbytes, d_out_var=ins["var"].data_ptr(), **kw)
    with pytest.raises(gi.GIError, match=r"\(-1\)"):
        gi.denoise_var(cam, w, h, s["rgb"], var, s["t"], s["normal"], s["albedo"], var_floor=INF)


def test_end_to_end_lowers_the_error_of_the_first_passes(torch_cuda):
    """Cornell 64 x 40, depth 4, seed 1 at n = 4, 16, 64 samples: render, frame_moments, render_aov, denoise_var at
    the default sigma_v and var_floor, against the device's own 2048-spp frame of seed 7 (the oracle's, bit for
    bit: test_gpu_parity).  The filtered mean squared error is at most 0.9 x the unfiltered one; gi_denoise at
    sigma_c = 0.5 / sqrt(n) is printed beside it."""
    d = dev_of("cornell")
    sc, _, w, h = A.frame_scene("cornell/0.01")
    cam = gi.Camera(sc.cam_pos, sc.cam_look, sc.focal)
    ref, _ = d.render(cam, sc.light, w, h, mode=gi.MODE_X, spp=2048, depth=4, seed=7)
    ref = ref.copy()
    aov = d.render_aov(cam, w, h, want=("t", "normal", "albedo"))
    for n in (4, 16, 64):
        noisy, _ = d.render(cam, sc.light, w, h, mode=gi.MODE_X, spp=n, depth=4, seed=1)
        m = d.frame_moments(w, h)
        assert U.bits_equal(np.where(m["mean"] < 1.0, m["mean"], 1.0), noisy).all()
        out = gi.denoise_var(cam, w, h, m["mean"], m["var"], aov["t"], aov["normal"], aov["albedo"], want=("rgb",))["rgb"]
        fixed = gi.denoise(cam, w, h, noisy, aov["t"], aov["normal"], aov["albedo"], sigma_c=0.5 / np.sqrt(n), want=("rgb",))["rgb"]
        raw, flt, fx = (((a - ref) ** 2).mean() for a in (noisy, out, fixed))
        print("n %d: mse %.3e -> variance-guided %.3e (%.2f x), gi_denoise %.3e (%.2f x)" % (n, raw, flt, flt / raw, fx, fx / raw))
        assert flt <= 0.9 * raw, (n, flt / raw)
