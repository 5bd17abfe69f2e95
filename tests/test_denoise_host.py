"""CPU: the denoiser's host side (gi_denoise*) -- the C-ABI's declarations, gi_denoise_scratch_bytes (host code,
no device), the numpy restatement's own properties, and the filter's quality on the oracle's Cornell frames.
No device."""
import ctypes
import os
import re

import numpy as np
import pytest

import denoise_ref as D
import oracle_util as U

gi = U.pkg()
NEW = ("gi_denoise_scratch_bytes", "gi_denoise_device", "gi_denoise")


def test_header_declares_the_denoiser_and_exports_list_it():
    hdr = open(os.path.join(U.ROOT, "include", "gi.h")).read()
    for f in NEW:
        assert re.search(r"^(int|int64_t) %s\(" % f, hdr, re.M), f
        assert f in gi.EXPORTS
    assert re.search(r"^int64_t gi_denoise_scratch_bytes\(const gi_aov_frame\* frame, const gi_denoise_params\* p\);", hdr, re.M)
    assert re.search(r"^int gi_denoise_device\(const gi_camera\* cam, const gi_aov_frame\* frame, const gi_denoise_params\* p,\s+"
                     r"const gi_denoise_io\* d_io, void\* d_scratch, int64_t scratch_bytes, void\* stream\);", hdr, re.M)
    assert re.search(r"^int gi_denoise\(const gi_camera\* cam, const gi_aov_frame\* frame, const gi_denoise_params\* p, "
                     r"const gi_denoise_io\* io\);", hdr, re.M)
    assert "#define GI_DENOISE_ALBEDO_STOP 1u" in hdr and gi.DENOISE_ALBEDO_STOP == 1
    assert int(re.search(r"#define GI_ABI_VERSION (\d+)", hdr).group(1)) == gi.ABI_VERSION >= 17
    # the ctypes mirrors have the header's layout
    assert [f for f, _ in gi.DenoiseParams._fields_] == ["levels", "normal_pow_log2", "flags", "reserved", "sigma_c", "sigma_p"]
    assert ctypes.sizeof(gi.DenoiseParams) == 32 and gi.DenoiseParams.sigma_c.offset == 16
    assert [f for f, _ in gi.DenoiseIO._fields_] == ["rgb", "t", "normal", "albedo", "out_rgb", "out_rgb8"]
    for f in ("denoise", "denoise_scratch_bytes", "denoise_device", "DenoiseParams"):
        assert f in gi.__all__ and hasattr(gi, f)


def test_scratch_bytes_checks_its_arguments_and_grows_with_the_window():
    L = gi.lib()

    def call(frame, p):
        return L.gi_denoise_scratch_bytes(ctypes.byref(frame) if frame is not None else None,
                                          ctypes.byref(p) if p is not None else None)
    good_f, good_p = gi.AovFrame(37, 21, 0, 0, 37, 21), gi.DenoiseParams(4, 5, 1, 0, 0.25, 0.01)
    n = call(good_f, good_p)
    assert n > 0 and n % 16 == 0
    assert n == gi.denoise_scratch_bytes(37, 21)
    # bad arguments: a negative status (GI_ERR_ARG) and a message
    bad_p = [gi.DenoiseParams(0, 5, 1, 0, 0.25, 0.01), gi.DenoiseParams(9, 5, 1, 0, 0.25, 0.01), gi.DenoiseParams(-1, 5, 1, 0, 0.25, 0.01),
             gi.DenoiseParams(4, -1, 1, 0, 0.25, 0.01), gi.DenoiseParams(4, 8, 1, 0, 0.25, 0.01), gi.DenoiseParams(4, 5, 2, 0, 0.25, 0.01),
             gi.DenoiseParams(4, 5, 1, 1, 0.25, 0.01), gi.DenoiseParams(4, 5, 1, 0, 0.0, 0.01), gi.DenoiseParams(4, 5, 1, 0, -1.0, 0.01),
             gi.DenoiseParams(4, 5, 1, 0, np.nan, 0.01), gi.DenoiseParams(4, 5, 1, 0, 0.25, 0.0), gi.DenoiseParams(4, 5, 1, 0, 0.25, np.nan),
             gi.DenoiseParams(4, 5, 1, 0, 0.25, -np.inf)]
    for p in bad_p:
        assert call(good_f, p) == -1 and len(L.gi_last_error()) > 0
    bad_f = [gi.AovFrame(0, 21, 0, 0, 0, 21), gi.AovFrame(37, -1, 0, 0, 37, 1), gi.AovFrame(37, 21, 0, 0, 38, 21),
             gi.AovFrame(37, 21, -1, 0, 37, 21), gi.AovFrame(37, 21, 30, 3, 5, 20), gi.AovFrame(37, 21, 0, 0, 37, 22)]
    for f in bad_f:
        assert call(f, good_p) == -1 and len(L.gi_last_error()) > 0
    assert call(None, good_p) == -1 and call(good_f, None) == -1
    with pytest.raises(gi.GIError, match=r"\(-1\)"):
        gi.denoise_scratch_bytes(37, 21, levels=0)
    # +inf sigmas are allowed; an empty window needs nothing
    assert call(good_f, gi.DenoiseParams(4, 5, 1, 0, np.inf, np.inf)) == n
    assert gi.denoise_scratch_bytes(37, 21, window=(5, 3, 5, 20)) == 0
    # grows with the window, with the albedo stop and up to the third level (two colour planes ping-pong)
    sizes = [gi.denoise_scratch_bytes(w, h) for w, h in ((1, 1), (23, 1), (37, 21), (64, 40), (131, 67), (1920, 1080))]
    assert sizes == sorted(set(sizes))
    assert gi.denoise_scratch_bytes(64, 40, window=(8, 8, 40, 24)) < gi.denoise_scratch_bytes(64, 40)
    assert gi.denoise_scratch_bytes(64, 40, albedo_stop=False) < gi.denoise_scratch_bytes(64, 40)
    by_levels = [gi.denoise_scratch_bytes(64, 40, levels=k) for k in range(1, 9)]
    assert by_levels[0] < by_levels[1] < by_levels[2] and len(set(by_levels[2:])) == 1
    # at least what the definition needs: a guide record (position, normal, scale: 7 doubles) per pixel
    assert by_levels[0] >= 64 * 40 * 7 * 8


def test_wrappers_check_shapes_without_the_library(monkeypatch):
    cam = gi.Camera(D.SYN_CAM.cam_pos, D.SYN_CAM.cam_look, D.SYN_CAM.focal)
    s = D.synthetic(21, 37, 1)

    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(gi, "lib", no_lib)
    with pytest.raises(ValueError):
        gi.denoise(cam, 37, 21, s["rgb"], s["t"], s["normal"])   # the albedo stop without albedo
    with pytest.raises(ValueError):
        gi.denoise(cam, 37, 21, s["rgb"][:, :30], s["t"], s["normal"], s["albedo"])
    with pytest.raises(ValueError):
        gi.denoise(cam, 37, 21, s["rgb"], s["t"], s["normal"], s["albedo"], window=(0, 0, 38, 21))
    for want in ((), ("rgb", "rgb"), ("t",)):
        with pytest.raises(ValueError):
            gi.denoise(cam, 37, 21, s["rgb"], s["t"], s["normal"], s["albedo"], want=want)
    with pytest.raises(ValueError):
        gi.denoise_device(cam, 37, 21, 1024, 1024, 1024, 1024, 1024, 1 << 20, d_out_rgb=2048, window=(5, 20, 30, 3))
    with pytest.raises(ValueError):
        gi.denoise_scratch_bytes(0, 21)


def _syn(rows, cols, seed, **kw):
    s = D.synthetic(rows, cols, seed)
    dirs = D.dirs_np(D.SYN_CAM, cols, rows)
    return s, D.denoise_np(D.SYN_CAM.cam_pos, dirs, s["rgb"], s["t"], s["normal"], s["albedo"], **kw)


def test_reference_passes_invalid_pixels_through():
    """Invalid pixels (t = +inf) come back unchanged at every level and change nothing as taps: an all-invalid
    frame is the input; valid pixels do change; the 8-bit output is trunc(255 c)."""
    s, (out, out8, steps) = _syn(21, 37, 3, levels=3, all_levels=True)
    hole = ~(s["t"] < np.inf)
    assert hole.sum() >= 40 and (~hole).sum() >= 400
    for c in steps + [out]:
        assert U.bits_equal(c[hole], s["rgb"][hole]).all()
    assert (~U.bits_equal(out[~hole], s["rgb"][~hole])).any(1).mean() > 0.5   # (a pixel of the random-normal blocks keeps its centre tap alone)
    assert (out8 == np.trunc(255 * out).astype(np.uint8)).all()
    # the holes' own colours do not enter: another colour there, the same valid pixels
    rgb2 = s["rgb"].copy()
    rgb2[hole] = 0.5
    out2, _ = D.denoise_np(D.SYN_CAM.cam_pos, D.dirs_np(D.SYN_CAM, 37, 21), rgb2, s["t"], s["normal"], s["albedo"], levels=3)
    assert U.bits_equal(out2[~hole], out[~hole]).all()
    t = np.full((21, 37), np.inf)
    out3, _ = D.denoise_np(D.SYN_CAM.cam_pos, D.dirs_np(D.SYN_CAM, 37, 21), s["rgb"], t, np.zeros((21, 37, 3)), s["albedo"])
    assert U.bits_equal(out3, s["rgb"]).all()


def test_reference_keeps_an_image_that_equals_its_albedo():
    """With the albedo stop every tap of a pixel has the pixel's albedo: an image whose colour is its {0, 1}^3
    albedo comes back bit for bit (sum_c = sum_w or 0 per channel); without the stop it is blurred."""
    s = D.synthetic(40, 64, 5)
    dirs = D.dirs_np(D.SYN_CAM, 64, 40)
    assert set(np.unique(s["albedo"])) == {0.0, 1.0} and len(np.unique(s["albedo"].reshape(-1, 3), axis=0)) == 4
    kw = dict(levels=5, sigma_c=np.inf, sigma_p=np.inf, normal_pow_log2=0)
    out, out8 = D.denoise_np(D.SYN_CAM.cam_pos, dirs, s["albedo"], s["t"], s["normal"], s["albedo"], albedo_stop=True, **kw)
    assert U.bits_equal(out, s["albedo"]).all() and (out8 == 255 * s["albedo"]).all()
    out, _ = D.denoise_np(D.SYN_CAM.cam_pos, dirs, s["albedo"], s["t"], s["normal"], s["albedo"], albedo_stop=False, **kw)
    valid = s["t"] < np.inf
    assert (~U.bits_equal(out[valid], s["albedo"][valid])).any(1).mean() > 0.5


def test_filter_lowers_the_error_of_the_cornell_frames():
    """The quality condition: frame cornell/0.01 (64 x 40), depth 4, noisy frames of seed 1 at 1, 2, 4, 16 and 64
    spp against 2048 spp of seed 7; guides from the oracle (normals from the triangles); 4 levels, sigma_c =
    0.5 / sqrt(spp), the other parameters the defaults.  The filtered mean squared error is at most 0.9 x the
    unfiltered one."""
    g = D.cornell_guides()
    ref = D.cornell_frame(2048, 7)
    for spp in (1, 2, 4, 16, 64):
        noisy = D.cornell_frame(spp, 1)
        out, _ = D.denoise_np(g["sc"].cam_pos, g["dirs"], noisy, g["t"], g["normal"], g["albedo"], levels=4,
                              sigma_c=0.5 / np.sqrt(spp), sigma_p=0.01, normal_pow_log2=5, albedo_stop=True)
        raw, flt = ((noisy - ref) ** 2).mean(), ((out - ref) ** 2).mean()
        print("spp %d: mse %.3e -> %.3e (%.2f x)" % (spp, raw, flt, flt / raw))
        assert flt <= 0.9 * raw, (spp, flt / raw)
