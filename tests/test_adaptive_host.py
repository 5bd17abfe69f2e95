"""CPU: adaptive sampling's host side (gi_render_adaptive*, gi_adaptive_info) -- the C-ABI's declarations, the ctypes
mirrors, the wrappers' own checks, and known answers of the numpy restatement (tests/adaptive_ref.py).  No device."""
import ctypes
import os
import re

import numpy as np
import pytest

import adaptive_ref as R
import moments_ref as M
import oracle_util as U

gi = U.pkg()
NEW = ("gi_render_adaptive_device", "gi_render_adaptive", "gi_adaptive_info")
INF = float("inf")


def test_header_declares_the_interface_and_exports_list_it():
    hdr = open(os.path.join(U.ROOT, "include", "gi.h")).read()
    for f in NEW:
        assert re.search(r"^int %s\(" % f, hdr, re.M), f
        assert f in gi.EXPORTS
    assert int(re.search(r"#define GI_ABI_VERSION (\d+)", hdr).group(1)) == gi.ABI_VERSION == 21
    assert gi.lib().gi_abi_version() == 21
    assert re.search(r"^#define GI_ADAPTIVE_RELATIVE 1u", hdr, re.M) and gi.ADAPTIVE_RELATIVE == 1
    assert re.search(r"^int gi_adaptive_info\(gi_scene\* scene, int32_t\* w, int32_t\* h, int32_t\* samples_done, int64_t\* active\);",
                     hdr, re.M)
    # what is not provided is said in the header
    sec = hdr[hdr.index("adaptive sampling: stop converged pixels"):hdr.index("typedef struct gi_adaptive_params")]
    for word in ("gi_multi", "banded gi_render", "drop-in", "passes of one sample", "Mode R", "ONE-PASS"):
        assert word in sec, word
    import importlib
    B = importlib.import_module(gi.__name__ + ".build")
    assert "gi_adapt.hip" in B.DEV_SRCS and gi.build_id() == B.source_hash()
    for f in ("render_adaptive", "render_adaptive_device", "adaptive_info"):
        assert callable(getattr(gi.DeviceScene, f))
    for k in ("AdaptiveParams", "AdaptiveOut", "ADAPTIVE_RELATIVE", "ADAPTIVE_OUTPUTS"):
        assert k in gi.__all__


def _c_fields(hdr, name):
    """[(type, field)] of `typedef struct name { ... } name;` in the header, comments dropped."""
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), hdr, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    return [(t.strip(), f) for t, f in re.findall(r"([\w ]+?\*?)\s*(\w+);", body)]


def test_ctypes_layouts_are_the_headers():
    hdr = open(os.path.join(U.ROOT, "include", "gi.h")).read()
    ctype = {"int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "double": ctypes.c_double}
    p = _c_fields(hdr, "gi_adaptive_params")
    assert [f for _, f in p] == [f for f, _ in gi.AdaptiveParams._fields_] == ["min_samples", "flags", "tol", "y_floor"]
    assert [ctype[t] for t, _ in p] == [t for _, t in gi.AdaptiveParams._fields_]
    assert ctypes.sizeof(gi.AdaptiveParams) == 24 and gi.AdaptiveParams.tol.offset == 8 and gi.AdaptiveParams.y_floor.offset == 16
    o = _c_fields(hdr, "gi_adaptive_out")
    assert [f for _, f in o] == [f for f, _ in gi.AdaptiveOut._fields_] == list(gi.ADAPTIVE_OUTPUTS) == ["rgb", "rgb8", "mean", "var", "n"]
    assert [t for t, _ in o] == ["double*", "uint8_t*", "double*", "double*", "int32_t*"]
    assert all(t is ctypes.c_void_p for _, t in gi.AdaptiveOut._fields_) and ctypes.sizeof(gi.AdaptiveOut) == 40


def test_library_exports_the_symbols():
    L = gi.lib()
    for f in NEW:
        assert getattr(L, f) is not None
    # a null scene is refused by each, with a message, before any device is touched
    o, p, a = gi.Opts(), gi.AdaptiveParams(2, 0, 1.0, 0.0), gi.AdaptiveOut()
    cam, light = gi.Camera((0, 0, 1)), (ctypes.c_double * 3)(0, 0, 0)
    assert L.gi_render_adaptive(None, ctypes.byref(cam._c), light, 8, 8, ctypes.byref(o), ctypes.byref(p), ctypes.byref(a)) == -1
    assert len(L.gi_last_error()) > 0
    assert L.gi_render_adaptive_device(None, ctypes.byref(cam._c), light, 8, 8, ctypes.byref(o), ctypes.byref(p), ctypes.byref(a), None) == -1
    assert L.gi_adaptive_info(None, None, None, None, None) == -1


def test_wrapper_checks_want_without_the_library(monkeypatch):
    d = object.__new__(gi.DeviceScene)
    cam = gi.Camera((0, 0, 1))

    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(gi, "lib", no_lib)
    for want in ((), ("n", "n"), ("samples",)):
        with pytest.raises(ValueError):
            d.render_adaptive(cam, (0, 0, 0), 8, 8, (0, 4), 16, want=want)


PASSES = [(0, 4), (4, 8), (8, 16)]


def test_exact_integer_samples_equal_the_two_pass_variance():
    """Integer-valued samples and n a power of two: every sum, product and quotient of the rule is exact, so the
    one-pass var is the two-pass value of tests/moments_ref.py bit for bit, after every pass."""
    g = np.random.default_rng(11)
    x = g.integers(0, 9, size=(5, 7, 16, 3)).astype(np.float64)
    res = R.adaptive_np(x, PASSES, 16, tol=5e-324)
    for (b, e), r in zip(PASSES, res):
        mean, var = M.moments_np(x[..., :e, :])
        # (only pixels of zero variance stop early with the smallest tol; the others carry n = e)
        live = r["n"] == e
        assert live.sum() >= 30
        assert U.bits_equal(r["mean"][live], mean[live]).all() and U.bits_equal(r["var"][live], var[live]).all()
        assert U.bits_equal(r["rgb"], np.where(r["mean"] < 1.0, r["mean"], 1.0)).all()
    assert (res[-1]["n"] == 16).all() and not res[-1]["active"].any()
    # one pixel by hand: samples 1, 3 (twice), S1 = 8, S2 = 20, n = 4: m = 2, v = ((20 - 16) / 3) / 4 = 1/3
    one = np.zeros((1, 4, 3))
    one[0, :, 0] = [1, 3, 1, 3]
    r = R.adaptive_np(one, [(0, 4)], 8, tol=0.5)[0]
    assert r["mean"][0, 0] == 2.0 and r["var"][0, 0] == (4.0 / 3.0) / 4.0 and r["n"][0] == 4 and r["active"][0]
    assert r["rgb"][0, 0] == 1.0 and tuple(r["rgb8"][0]) == (255, 0, 0)
    assert not R.adaptive_np(one, [(0, 4)], 8, tol=0.6)[0]["active"][0]   # 1/3 <= 0.36


def test_tol_inf_stops_everything_at_the_first_judged_pass():
    g = np.random.default_rng(12)
    x = g.random((6, 16, 3)) * 4.0
    res = R.adaptive_np(x, PASSES, 16, tol=INF, min_samples=2)
    assert all((r["n"] == 4).all() and not r["active"].any() for r in res)
    for k in ("mean", "var", "rgb", "rgb8"):
        assert U.bits_equal(res[0][k], res[2][k]).all()
    assert U.bits_equal(res[0]["rgb"], M.running_frames_np(x)[4]).all()
    # no pixel is judged before it has min_samples
    res = R.adaptive_np(x, PASSES, 16, tol=INF, min_samples=5)
    assert res[0]["active"].all() and (res[1]["n"] == 8).all() and not res[1]["active"].any()


def test_nan_never_stops_early_and_zeros_stop_at_once():
    x = np.zeros((3, 16, 3))
    x[0, 1, 2] = np.nan          # pixel 0: a NaN sample
    x[1, :, :] = 0.25            # pixel 1: constant
    res = R.adaptive_np(x, PASSES, 16, tol=INF)   # pixel 2: zeros
    assert [int(r["n"][0]) for r in res] == [4, 8, 16] and [bool(r["active"][0]) for r in res] == [True, True, False]
    assert np.isnan(res[2]["mean"][0, 2]) and np.isnan(res[2]["rgb"][0, 2]) and tuple(res[2]["rgb8"][0]) == (0, 0, 0)
    res = R.adaptive_np(x, PASSES, 16, tol=5e-324, resolved=np.array([False, False, True]))
    assert (res[2]["n"][1:] == 4).all()
    z = np.zeros(1)
    for k in ("mean", "var", "rgb"):
        assert U.bits_equal(res[2][k][2], z).all()   # +0, sign included
    assert res[2]["var"][1, 0] == 0.0 and res[2]["mean"][1, 0] == 0.25


def test_relative_at_and_below_the_floor():
    # two pixels of the same variance, v = 1/12 per channel (samples 0, 1, 0, 1 scaled): err = 3 v
    x = np.zeros((2, 4, 3))
    x[0] = np.array([0.0, 1.0, 0.0, 1.0])[:, None] * 0.5 + 8.0    # bright: y = 3 * 8.25
    x[1] = np.array([0.0, 1.0, 0.0, 1.0])[:, None] * 0.5          # dim:    y = 3 * 0.25 = 0.75
    a = R.adaptive_np(x, [(0, 4)], 8, tol=0.1)[0]
    assert U.bits_equal(a["var"][0], a["var"][1]).all() and a["active"].all()     # absolute: err = 1/16 > 0.01
    err = float((a["var"][1, 0] + a["var"][1, 1]) + a["var"][1, 2])
    assert err == 0.0625
    r = R.adaptive_np(x, [(0, 4)], 8, tol=0.1, relative=True, y_floor=0.5)[0]
    assert not r["active"][0] and r["active"][1]      # thr = 0.01 y^2: 6.1 for the bright pixel, 0.0056 for the dim
    # at and below the floor: f = y_floor where y <= y_floor, so the dim pixel stops iff err <= (tol y_floor)^2
    assert R.adaptive_np(x, [(0, 4)], 8, tol=0.1, relative=True, y_floor=0.75)[0]["active"][1]       # y == floor: 0.005625
    assert not R.adaptive_np(x, [(0, 4)], 8, tol=0.1, relative=True, y_floor=2.5)[0]["active"][1]    # (0.25)^2 = 0.0625 <= itself
    assert R.adaptive_np(x, [(0, 4)], 8, tol=0.1, relative=True, y_floor=2.4)[0]["active"][1]        # 0.0576 < 0.0625
