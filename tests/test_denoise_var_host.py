"""CPU: the variance-guided denoiser's host side (gi_denoise_var*) -- the C-ABI's declarations,
gi_denoise_var_scratch_bytes (host code, no device), the numpy restatement's own properties
(tests/denoise_var_ref.py), its tie to the fixed-sigma filter, and its quality on a heteroscedastic synthetic.
No device."""
import ctypes
import os
import re

import numpy as np
import pytest

import denoise_ref as D
import denoise_var_ref as DV
import moments_ref as M
import oracle_util as U

gi = U.pkg()
NEW = ("gi_denoise_var_scratch_bytes", "gi_denoise_var_device", "gi_denoise_var")
INF = float("inf")


def test_header_declares_the_filter_and_exports_list_it():
    hdr = open(os.path.join(U.ROOT, "include", "gi.h")).read()
    for f in NEW:
        assert re.search(r"^(int|int64_t) %s\(" % f, hdr, re.M), f
        assert f in gi.EXPORTS
    assert re.search(r"^int64_t gi_denoise_var_scratch_bytes\(const gi_aov_frame\* frame, const gi_denoise_var_params\* p\);", hdr, re.M)
    assert re.search(r"^int gi_denoise_var_device\(const gi_camera\* cam, const gi_aov_frame\* frame, const gi_denoise_var_params\* p,\s+"
                     r"const gi_denoise_var_io\* d_io, void\* d_scratch, int64_t scratch_bytes, void\* stream\);", hdr, re.M)
    assert re.search(r"^int gi_denoise_var\(const gi_camera\* cam, const gi_aov_frame\* frame, const gi_denoise_var_params\* p,\s+"
                     r"const gi_denoise_var_io\* io\);", hdr, re.M)
    assert int(re.search(r"#define GI_ABI_VERSION (\d+)", hdr).group(1)) == gi.ABI_VERSION >= 18
    # the ctypes mirrors have the header's layout: the fields of the two structs in the header's order
    for name, cls in (("gi_denoise_var_params", gi.DenoiseVarParams), ("gi_denoise_var_io", gi.DenoiseVarIO)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        fields = [re.search(r"(\w+)$", d.strip()).group(1) for d in body.split(";") if d.strip()]
        assert fields == [f for f, _ in cls._fields_], name
    assert ctypes.sizeof(gi.DenoiseVarParams) == 40 and gi.DenoiseVarParams.sigma_v.offset == 16
    assert gi.DenoiseVarParams.var_floor.offset == 32 and ctypes.sizeof(gi.DenoiseVarIO) == 64
    # gi_denoise's structs are as they were
    assert ctypes.sizeof(gi.DenoiseParams) == 32 and ctypes.sizeof(gi.DenoiseIO) == 48
    for f in ("denoise_var", "denoise_var_scratch_bytes", "denoise_var_device", "DenoiseVarParams"):
        assert f in gi.__all__ and hasattr(gi, f)
    assert gi.DENOISE_VAR_SIGMA_V > 0 and 0 < gi.DENOISE_VAR_FLOOR < INF


def test_scratch_bytes_checks_its_arguments_and_grows_with_the_window():
    L = gi.lib()

    def call(frame, p):
        return L.gi_denoise_var_scratch_bytes(ctypes.byref(frame) if frame is not None else None,
                                              ctypes.byref(p) if p is not None else None)
    P = gi.DenoiseVarParams
    good_f, good_p = gi.AovFrame(37, 21, 0, 0, 37, 21), P(4, 5, 1, 0, 2.0, 0.01, 1e-6)
    n = call(good_f, good_p)
    assert n > 0 and n % 16 == 0
    assert n == gi.denoise_var_scratch_bytes(37, 21, sigma_v=2.0)
    bad_p = [P(0, 5, 1, 0, 2.0, 0.01, 1e-6), P(9, 5, 1, 0, 2.0, 0.01, 1e-6), P(-1, 5, 1, 0, 2.0, 0.01, 1e-6),
             P(4, -1, 1, 0, 2.0, 0.01, 1e-6), P(4, 8, 1, 0, 2.0, 0.01, 1e-6), P(4, 5, 2, 0, 2.0, 0.01, 1e-6),
             P(4, 5, 1, 1, 2.0, 0.01, 1e-6), P(4, 5, 1, 0, 0.0, 0.01, 1e-6), P(4, 5, 1, 0, -1.0, 0.01, 1e-6),
             P(4, 5, 1, 0, np.nan, 0.01, 1e-6), P(4, 5, 1, 0, 2.0, 0.0, 1e-6), P(4, 5, 1, 0, 2.0, np.nan, 1e-6),
             P(4, 5, 1, 0, 2.0, -np.inf, 1e-6),
             P(4, 5, 1, 0, 2.0, 0.01, 0.0), P(4, 5, 1, 0, 2.0, 0.01, -1e-6), P(4, 5, 1, 0, 2.0, 0.01, np.inf),
             P(4, 5, 1, 0, 2.0, 0.01, np.nan)]
    for p in bad_p:
        assert call(good_f, p) == -1 and len(L.gi_last_error()) > 0
    bad_f = [gi.AovFrame(0, 21, 0, 0, 0, 21), gi.AovFrame(37, -1, 0, 0, 37, 1), gi.AovFrame(37, 21, 0, 0, 38, 21),
             gi.AovFrame(37, 21, -1, 0, 37, 21), gi.AovFrame(37, 21, 30, 3, 5, 20), gi.AovFrame(37, 21, 0, 0, 37, 22)]
    for f in bad_f:
        assert call(f, good_p) == -1 and len(L.gi_last_error()) > 0
    assert call(None, good_p) == -1 and call(good_f, None) == -1
    with pytest.raises(gi.GIError, match=r"\(-1\)"):
        gi.denoise_var_scratch_bytes(37, 21, var_floor=0.0)
    # +inf sigmas are allowed; an empty window needs nothing
    assert call(good_f, P(4, 5, 1, 0, np.inf, np.inf, 1e-6)) == n
    assert gi.denoise_var_scratch_bytes(37, 21, window=(5, 3, 5, 20)) == 0
    # monotone in the window, and never below gi_denoise's for the same frame and levels
    frames = ((1, 1), (23, 1), (37, 21), (64, 40), (131, 67), (1920, 1080))
    sizes = [gi.denoise_var_scratch_bytes(w, h) for w, h in frames]
    assert sizes == sorted(set(sizes))
    assert gi.denoise_var_scratch_bytes(64, 40, window=(8, 8, 40, 24)) < gi.denoise_var_scratch_bytes(64, 40)
    for w, h in frames:
        for k in range(1, 9):
            for stop in (True, False):
                assert gi.denoise_var_scratch_bytes(w, h, levels=k, albedo_stop=stop) >= gi.denoise_scratch_bytes(w, h, levels=k, albedo_stop=stop)
    # the variance planes ping-pong beside the colour planes: three doubles more per pixel and plane
    by_levels = [gi.denoise_var_scratch_bytes(64, 40, levels=k) - gi.denoise_scratch_bytes(64, 40, levels=k) for k in range(1, 9)]
    assert by_levels[0] >= 0 and by_levels[1] - by_levels[0] >= 64 * 40 * 24 and by_levels[2] - by_levels[1] >= 64 * 40 * 24
    assert len(set(by_levels[2:])) == 1


def test_wrappers_check_shapes_without_the_library(monkeypatch):
    cam = gi.Camera(D.SYN_CAM.cam_pos, D.SYN_CAM.cam_look, D.SYN_CAM.focal)
    s = D.synthetic(21, 37, 1)
    v = DV.synthetic_var(21, 37, 1)

    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(gi, "lib", no_lib)
    with pytest.raises(ValueError):
        gi.denoise_var(cam, 37, 21, s["rgb"], v, s["t"], s["normal"])   # the albedo stop without albedo
    with pytest.raises(ValueError):
        gi.denoise_var(cam, 37, 21, s["rgb"], v[:, :30], s["t"], s["normal"], s["albedo"])
    with pytest.raises(ValueError):
        gi.denoise_var(cam, 37, 21, s["rgb"][:, :30], v, s["t"], s["normal"], s["albedo"])
    with pytest.raises(ValueError):
        gi.denoise_var(cam, 37, 21, s["rgb"], v, s["t"], s["normal"], s["albedo"], window=(0, 0, 38, 21))
    for want in ((), ("rgb", "rgb"), ("t",)):
        with pytest.raises(ValueError):
            gi.denoise_var(cam, 37, 21, s["rgb"], v, s["t"], s["normal"], s["albedo"], want=want)
    with pytest.raises(ValueError):
        gi.denoise_var_device(cam, 37, 21, 1024, 1024, 1024, 1024, 1024, 1024, 1 << 20, d_out_rgb=2048, window=(5, 20, 30, 3))
    with pytest.raises(ValueError):
        gi.denoise_var_scratch_bytes(0, 21)


def _run(s, var, rows, cols, **kw):
    return DV.denoise_var_np(D.SYN_CAM.cam_pos, D.dirs_np(D.SYN_CAM, cols, rows), s["rgb"], var, s["t"], s["normal"], s["albedo"], **kw)


def test_reference_passes_invalid_pixels_through():
    """Invalid pixels keep their colour and variance at every level, and neither enters a valid pixel."""
    s, var = D.synthetic(21, 37, 3), DV.synthetic_var(21, 37, 3)
    out, ov, out8, cs, Vs, _ = _run(s, var, 21, 37, levels=3, sigma_v=1.0, all_levels=True)
    hole = ~(s["t"] < np.inf)
    assert hole.sum() >= 40 and (~hole).sum() >= 400
    for c, V in zip(cs + [out], Vs + [ov]):
        assert U.bits_equal(c[hole], s["rgb"][hole]).all() and U.bits_equal(V[hole], var[hole]).all()
    assert (~U.bits_equal(out[~hole], s["rgb"][~hole])).any(1).mean() > 0.5
    assert (out8 == np.trunc(255 * out).astype(np.uint8)).all()
    s2, var2 = dict(s), var.copy()
    s2["rgb"] = s["rgb"].copy()
    s2["rgb"][hole] = 0.5
    var2[hole] = np.nan
    out2, ov2, _ = _run(s2, var2, 21, 37, levels=3, sigma_v=1.0)
    assert U.bits_equal(out2[~hole], out[~hole]).all() and U.bits_equal(ov2[~hole], ov[~hole]).all()


def test_reference_zero_variance_stays_zero_without_the_colour_stop():
    s = D.synthetic(21, 37, 4)
    valid = s["t"] < np.inf
    for levels in (1, 3, 5):
        out, ov, _ = _run(s, np.zeros((21, 37, 3)), 21, 37, levels=levels, sigma_v=INF)
        assert (ov[valid] == 0).all() and np.isfinite(out[valid]).all()
        # and the colour is the fixed filter's without its colour stop
        ref, _ = D.denoise_np(D.SYN_CAM.cam_pos, D.dirs_np(D.SYN_CAM, 37, 21), s["rgb"], s["t"], s["normal"], s["albedo"],
                              levels=levels, sigma_c=INF)
        assert U.bits_equal(out, ref).all()


@pytest.mark.parametrize("rows,cols,seed", [(21, 37, 6), (40, 64, 7)])
def test_one_level_equals_the_fixed_filter_at_the_same_stop(rows, cols, seed):
    """var = 1/16 in every channel, sigma_v = 1, var_floor = 1/16: g_p = 3/16 exactly (small integers over 256),
    so sigma2_p = 1/4 exactly and one level is denoise_np's level at sigma_c = 0.5, bit for bit."""
    s = D.synthetic(rows, cols, seed)
    var = np.full((rows, cols, 3), 0.0625)
    valid = s["t"] < np.inf
    for stop in (True, False):
        out, ov, out8, _, _, gs = _run(s, var, rows, cols, levels=1, sigma_v=1.0, var_floor=0.0625, albedo_stop=stop, all_levels=True)
        assert (gs[0][valid] == 0.1875).all()
        assert (1.0 * 1.0 * gs[0][valid] + 0.0625 == 0.25).all()
        ref, ref8 = D.denoise_np(D.SYN_CAM.cam_pos, D.dirs_np(D.SYN_CAM, cols, rows), s["rgb"], s["t"], s["normal"], s["albedo"],
                                 levels=1, sigma_c=0.5, albedo_stop=stop)
        assert U.bits_equal(out, ref).all() and (out8 == ref8).all()
        assert (ov[valid] <= 0.0625).all() and (ov[valid] > 0).all()   # sum w^2 <= (sum w)^2


def test_variance_propagation_of_a_flat_region():
    """No stops and constant inputs: every level's weights are the H x H of the taps that exist, so an interior
    pixel's variance falls by sum(k^2) / sum(k)^2 per level."""
    rows, cols = 21, 37
    s = D.synthetic(rows, cols, 9, holes=0.0)
    s["normal"][:] = (1.0, 0.0, 0.0)
    s["rgb"][:] = 0.5
    var = np.full((rows, cols, 3), 0.25)
    _, ov, _ = DV.denoise_var_np(D.SYN_CAM.cam_pos, D.dirs_np(D.SYN_CAM, cols, rows), s["rgb"], var, s["t"], s["normal"], None,
                                 levels=1, sigma_v=INF, sigma_p=INF, normal_pow_log2=0, albedo_stop=False)
    k2 = sum((a * b) ** 2 for a in D.H for b in D.H)
    assert np.allclose(ov[2:-2, 2:-2], 0.25 * k2, rtol=1e-14)


def test_filter_lowers_the_error_of_a_heteroscedastic_frame():
    """Clean signal: the oracle's 2048-spp Cornell frame (64 x 40, depth 4, seed 7).  Noise: 8 seeded samples per
    pixel whose standard deviation is 0.02 in the left half of the frame and 0.3 in the right half.  Moments from
    moments_ref; 4 levels at the default sigma_v and var_floor.  The filtered mean squared error is at most
    0.9 x the unfiltered one (the project's condition); the fixed-sigma_c filter's figure is printed beside it."""
    g = D.cornell_guides()
    clean = D.cornell_frame(2048, 7)
    h, w, n = g["h"], g["w"], 8
    rng = np.random.default_rng(20)
    sd = np.where(np.arange(w) < w // 2, 0.02, 0.3)[None, :, None, None]
    samples = clean[:, :, None, :] + sd * rng.normal(size=(h, w, n, 3))
    mean, var = M.moments_np(samples)
    out, ov, _ = DV.denoise_var_np(g["sc"].cam_pos, g["dirs"], mean, var, g["t"], g["normal"], g["albedo"], levels=4,
                                   sigma_v=gi.DENOISE_VAR_SIGMA_V, var_floor=gi.DENOISE_VAR_FLOOR)
    fixed, _ = D.denoise_np(g["sc"].cam_pos, g["dirs"], mean, g["t"], g["normal"], g["albedo"], levels=4, sigma_c=0.5 / np.sqrt(n))
    valid = g["t"] < np.inf
    raw, flt, fx = (((a - clean) ** 2).mean() for a in (mean, out, fixed))
    print("n %d: mse %.3e -> variance-guided %.3e (%.2f x), fixed sigma_c %.3e (%.2f x)" % (n, raw, flt, flt / raw, fx, fx / raw))
    for name, cols in (("left (sd 0.02)", slice(0, w // 2)), ("right (sd 0.3)", slice(w // 2, w))):
        r, f, x = (((a[:, cols] - clean[:, cols]) ** 2).mean() for a in (mean, out, fixed))
        print("  %s: mse %.3e -> variance-guided %.3e, fixed sigma_c %.3e" % (name, r, f, x))
    assert flt <= 0.9 * raw, flt / raw
    assert (ov[valid] <= var[valid].max()).all()
