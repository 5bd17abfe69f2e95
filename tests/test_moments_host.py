"""CPU: the sample moments' host side (gi_frame_samples_info, gi_frame_moments*) -- the C-ABI's declarations, the
ctypes mirrors, the wrappers' own checks, and the numpy restatement's properties (tests/moments_ref.py).  No device."""
import ctypes
import os
import re

import numpy as np
import pytest

import moments_ref as M
import oracle_util as U

gi = U.pkg()
NEW = ("gi_frame_samples_info", "gi_frame_moments_device", "gi_frame_moments")


def test_header_declares_the_moments_and_exports_list_them():
    hdr = open(os.path.join(U.ROOT, "include", "gi.h")).read()
    for f in NEW:
        assert re.search(r"^int %s\(" % f, hdr, re.M), f
        assert f in gi.EXPORTS
    assert re.search(r"^typedef struct gi_moments \{ double\* mean; double\* var; double\* samples; \} gi_moments;", hdr, re.M)
    assert re.search(r"^int gi_frame_samples_info\(gi_scene\* scene, int32_t\* w, int32_t\* h, int32_t\* n, int32_t\* spp\);", hdr, re.M)
    assert re.search(r"^int gi_frame_moments_device\(gi_scene\* scene, const gi_aov_frame\* frame, const gi_moments\* d_out, "
                     r"void\* stream\);", hdr, re.M)
    assert re.search(r"^int gi_frame_moments\(gi_scene\* scene, const gi_aov_frame\* frame, const gi_moments\* out\);", hdr, re.M)
    assert int(re.search(r"#define GI_ABI_VERSION (\d+)", hdr).group(1)) == gi.ABI_VERSION >= 18
    assert [f for f, _ in gi.Moments._fields_] == ["mean", "var", "samples"] == list(gi.MOMENTS_OUTPUTS)
    assert ctypes.sizeof(gi.Moments) == 24
    assert "MOMENTS_OUTPUTS" in gi.__all__
    for f in ("frame_samples_info", "frame_moments", "frame_moments_device"):
        assert callable(getattr(gi.DeviceScene, f))


def test_library_exports_the_symbols():
    L = gi.lib()
    for f in NEW:
        assert getattr(L, f) is not None
    # a null scene is refused by each, with a message, before any device is touched
    fr, m = gi.AovFrame(37, 21, 0, 0, 37, 21), gi.Moments(None, None, None)
    assert L.gi_frame_samples_info(None, None, None, None, None) == -1 and len(L.gi_last_error()) > 0
    assert L.gi_frame_moments(None, ctypes.byref(fr), ctypes.byref(m)) == -1
    assert L.gi_frame_moments_device(None, ctypes.byref(fr), ctypes.byref(m), None) == -1


def test_wrappers_check_their_arguments_without_the_library(monkeypatch):
    d = object.__new__(gi.DeviceScene)   # (no scene: the checks come first)

    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(gi, "lib", no_lib)
    for want in ((), ("mean", "mean"), ("rgb",)):
        with pytest.raises(ValueError):
            d.frame_moments(37, 21, want=want)
    with pytest.raises(ValueError):
        d.frame_moments(37, 21, window=(0, 0, 38, 21))
    with pytest.raises(ValueError):
        d.frame_moments(0, 21)
    with pytest.raises(ValueError):
        d.frame_moments_device(37, 21, window=(5, 20, 30, 3), d_mean=1024)


def test_reference_moments():
    """The restatement against exact small cases and numpy's own two-pass variance."""
    x = np.array([[[1.0, 2.0, 0.0], [3.0, 2.0, 0.0]]])          # one pixel, two samples
    mean, var = M.moments_np(x)
    assert U.bits_equal(mean, np.array([[2.0, 2.0, 0.0]])).all()
    assert U.bits_equal(var, np.array([[1.0, 0.0, 0.0]])).all()   # ((1 + 1) / 1) / 2
    g = np.random.default_rng(5)
    for n in (2, 3, 8, 17):
        s = g.random((4, 5, n, 3)) * 3.0
        s[0, 0] = 0.0           # an unlisted pixel: +0 mean and variance
        mean, var = M.moments_np(s)
        assert mean.shape == var.shape == (4, 5, 3)
        assert np.allclose(mean, s.mean(2), rtol=1e-14) and np.allclose(var, s.var(2, ddof=1) / n, rtol=1e-12)
        assert (mean[0, 0] == 0).all() and (var[0, 0] == 0).all() and not np.signbit(mean[0, 0]).any()
        assert (var >= 0).all()
        run = M.running_frames_np(s)
        assert sorted(run) == list(range(2, n + 1))
        assert U.bits_equal(run[n], np.where(mean < 1.0, mean, 1.0)).all()
        m2, _ = M.moments_np(s[:, :, :2])
        assert U.bits_equal(run[2], np.where(m2 < 1.0, m2, 1.0)).all()
    # the sum is sequential from +0 in sample order: a case where another order rounds differently
    x = np.array([[[1e16, 0, 0], [1.0, 0, 0], [1.0, 0, 0], [-1e16, 0, 0]]])
    assert M.moments_np(x)[0][0, 0] == 0.0 and M.moments_np(x[:, ::-1])[0][0, 0] == 0.0
    x = np.array([[[1.0, 0, 0], [1e16, 0, 0], [-1e16, 0, 0], [1.0, 0, 0]]])
    assert M.moments_np(x)[0][0, 0] == 0.25
