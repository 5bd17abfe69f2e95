"""GPU: adaptive sampling (gi_render_adaptive*, gi_adaptive_info; gi_adapt.hip k_x_adapt_init / _fill / _fold around
the render kernels) against the CPU oracle's frames and the numpy restatement of the rule (tests/adaptive_ref.py).
Everything compares bit for bit (U.bits_equal): there is no tolerance anywhere in this file.

Frames: 16 spp at depth 4 in the passes (0, 4), (4, 8), (8, 16).  A pixel that stopped after n_p samples is the
oracle's frame of spp = n_p at that pixel; every plane after every pass is the restatement applied to the per-sample
rows of the plain 16-spp render of the same seed (gi_frame_moments' samples plane)."""
import copy
import ctypes

import numpy as np
import pytest

import adaptive_ref as R
import aov_frames as A
import oracle_util as U
from x_scenes import with_env

pytestmark = pytest.mark.gpu

gi = U.pkg()
SPP, DEPTH, SEED = 16, 4, 1
PASSES = ((0, 4), (4, 8), (8, 16))
FORMS = {"default": 0, "mega": gi.FLAG_X_MEGA, "wf": gi.FLAG_X_WF, "seg": gi.FLAG_X_SEG}
PLANES = gi.ADAPTIVE_OUTPUTS
DENORMAL, INF = 5e-324, float("inf")
# name -> (frame key of tests/aov_frames.py, w, h, camera position or None: the frame's).  cornell is staged in LDS and
# answers its queries from the flat leaf table; zoo is read from HBM.  big: 8777 pixels, several workgroups of every
# kernel here, and a listed count that is no multiple of 64.  far: the camera 40 units out, most pixels resolved by
# the classify pass and fewer than 64 listed (less than one wave of k_x_adapt_fold).  inside: the camera inside the box
# (from (2, 0, 0) toward (10, 2, -2), focal 0.05), every pixel listed and none of constant radiance over its first
# samples (the frames seen from outside list pixels around the box whose every sample is black, and some whose
# samples are all the saturated (1, 1, 1): exactly zero variance, so even the smallest tol stops them).
FRAMES = {"cornell": ("cornell/0.01", 64, 40, None), "zoo": ("zoo", 37, 21, None), "big": ("cornell/0.01", 131, 67, None),
          "far": ("cornell/0.004", 37, 21, (-40.0, 0.0, 0.0)), "inside": ("cornell/0.004", 37, 21, (2.0, 0.0, 0.0))}
INSIDE_LOOK, INSIDE_FOCAL = (10.0, 2.0, -2.0), 0.05
# The tolerance of the decision tests, chosen once per frame from the device's own samples (the samples plane of
# gi_frame_moments of the plain 16-spp render, seed 1): the value of a coarse sweep (0.01, 0.02, 0.03, 0.04, 0.05, 0.06,
# 0.08, 0.1, 0.15) at which the restatement leaves the traced pixels most evenly split between n = 4, 8 and 16 --
# cornell 22 / 23 / 55 %, big 23 / 22 / 55 %, zoo 55 / 14 / 31 %; decision_ref asserts the split.  far and inside
# (no share is asserted of them): between the medians of sqrt(err) after 4 and after 8 samples on far, 0.32 and 0.23;
# on inside that stops 691 pixels after 4 samples and the other 86 after 8.
TOL = {"cornell": 0.15, "zoo": 0.08, "big": 0.15, "far": 0.3, "inside": 0.3}
KW = dict(spp=SPP, depth=DEPTH, seed=SEED)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    return torch


_devs, _cache = {}, {}


def scene_of(frame):
    key, w, h, pos = FRAMES[frame]
    sc, env, _, _ = A.frame_scene(key)
    if pos is not None:
        sc = copy.deepcopy(sc)
        sc.cam_pos = pos
    if frame == "inside":
        sc.cam_look, sc.focal = INSIDE_LOOK, INSIDE_FOCAL
    return sc, env, w, h


def setup(frame, fresh=False):
    """(device scene, scene, camera, w, h) of a frame; the device scene is built once unless fresh."""
    sc, env, w, h = scene_of(frame)
    if fresh:
        d = with_env(env, lambda: gi.DeviceScene.from_scene(sc))
    else:
        if frame not in _devs:
            _devs[frame] = with_env(env, lambda: gi.DeviceScene.from_scene(sc))
        d = _devs[frame]
    return d, sc, gi.Camera(sc.cam_pos, sc.cam_look, sc.focal), w, h


def frozen(key, make):
    if key not in _cache:
        v = make()
        for a in (v.values() if isinstance(v, dict) else v if isinstance(v, (list, tuple)) else [v]):
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = v
    return _cache[key]


def oracle_frame(frame, k):
    """The oracle's Mode X frame of spp = k as (h, w, 3); computed once, read-only."""
    sc, _, w, h = scene_of(frame)
    return frozen(("oracle", frame, k),
                  lambda: U.oracle_render(sc.to_scn(), w, h, mode=1, spp=k, depth=DEPTH, seed=SEED)["rgb"].reshape(h, w, 3))


def plain(frame):
    """The plain 16-spp render of the frame: {"rgb", "rgb8", "samples" (h, w, 16, 3), "listed" (the work list's length)};
    computed once, read-only."""
    def make():
        d, sc, cam, w, h = setup(frame)
        rgb, rgb8 = d.render(cam, sc.light, w, h, mode=gi.MODE_X, **KW)
        smp = d.frame_moments(w, h, want=("samples",))["samples"]
        # nobody is judged in a first pass that ends below min_samples: what is active after it is the work list
        d.render_adaptive(cam, sc.light, w, h, (0, 4), tol=1.0, min_samples=5, want=("n",), **KW)
        return dict(rgb=rgb, rgb8=rgb8, samples=smp, listed=d.adaptive_info()["active"])
    return frozen(("plain", frame), make)


def ref(frame, tol, min_samples, relative=False, y_floor=0.0):
    """The restatement's result per pass for the frame's device samples; computed once, read-only."""
    def make():
        out = R.adaptive_np(plain(frame)["samples"], PASSES, SPP, tol, min_samples, relative, y_floor)
        for r in out:
            for a in r.values():
                a.setflags(write=False)
        return out
    return frozen(("ref", frame, tol, min_samples, relative, y_floor), make)


def decision_ref(frame):
    """ref() at the frame's TOL, with the condition on the inputs: each of 4, 8 and 16 is held by at least 5 % of the
    listed pixels (n = 4 counted over the pixels with a non-zero sample only: a resolved pixel also ends at 4), so the
    test can pass neither with nothing stopping nor with everything stopping."""
    r = ref(frame, TOL[frame], 4)
    p = plain(frame)
    n, traced = r[-1]["n"], p["samples"].any((-1, -2))
    for k in (4, 8, 16):
        assert ((n == k) & traced).sum() >= 0.05 * p["listed"], (frame, k, int(((n == k) & traced).sum()), p["listed"])
    return r


def run(d, sc, cam, w, h, tol, min_samples=4, flags=0, passes=PASSES, between=None, **kw):
    """The passes through the host form; every plane and the active count after each."""
    out = []
    for b, e in passes:
        o = d.render_adaptive(cam, sc.light, w, h, (b, e), tol=tol, min_samples=min_samples, flags=flags, want=PLANES, **KW, **kw)
        info = d.adaptive_info()
        assert (info["w"], info["h"], info["samples_done"]) == (w, h, e)
        o["active"] = info["active"]
        out.append(o)
        if between:
            between(e)
    return out


def same(o, r):
    """The planes of one pass against the restatement's."""
    for k in ("mean", "var", "rgb"):
        ne = ~U.bits_equal(o[k], r[k])
        assert not ne.any(), (k, int(ne.any(-1).sum()))
    assert (o["n"] == r["n"]).all() and (o["rgb8"] == r["rgb8"]).all()
    # the active count is the list's: the resolved pixels, which the restatement carries until they are judged, are
    # never in it -- they have all stopped once a pass has been judged (n >= min_samples, known by a stopped pixel)
    if not r["active"].all():
        assert o["active"] == int(r["active"].sum())


def test_frames_are_what_they_are_meant_to_be(torch_cuda):
    assert setup("cornell")[0].info()["x_lds_resident"] == 1 and setup("cornell")[0].kat_x_variant()["FLAT"]
    assert setup("zoo")[0].info()["x_lds_resident"] == 0
    far, big = plain("far"), plain("big")
    assert 0 < far["listed"] < 64 and far["listed"] < 0.1 * 37 * 21
    assert big["listed"] > 4 * 256 and big["listed"] % 64 != 0
    assert plain("inside")["listed"] == 37 * 21


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("frame", ["cornell", "zoo"])
def test_stopped_pixels_are_the_oracles_frames(torch_cuda, frame, form):
    """After every pass, every pixel with n_p samples is the oracle's frame of spp = n_p at that pixel."""
    d, sc, cam, w, h = setup(frame)
    decision_ref(frame)
    outs = run(d, sc, cam, w, h, TOL[frame], flags=FORMS[form])
    for (b, e), o in zip(PASSES, outs):
        assert set(np.unique(o["n"])) <= {k for _, k in PASSES if k <= e}
        for k in (4, 8, 16):
            m = o["n"] == k
            ne = ~U.bits_equal(o["rgb"][m], oracle_frame(frame, k)[m])
            assert not ne.any(), (frame, form, e, k, int(ne.any(-1).sum()))
    assert set(np.unique(outs[-1]["n"])) == {4, 8, 16} and outs[-1]["active"] == 0


@pytest.mark.parametrize("frame", ["big", "far"])
def test_oracle_on_the_large_and_the_far_frame(torch_cuda, frame):
    d, sc, cam, w, h = setup(frame)
    o = run(d, sc, cam, w, h, TOL[frame])[-1]
    for k in (4, 8, 16):
        m = o["n"] == k
        assert U.bits_equal(o["rgb"][m], oracle_frame(frame, k)[m]).all(), (frame, k)
    assert (o["n"] >= 4).all()


@pytest.mark.parametrize("frame", list(FRAMES))
def test_decisions_equal_the_restatement(torch_cuda, frame):
    """n, mean, var, rgb, rgb8 and the active count after each pass, absolute and relative."""
    d, sc, cam, w, h = setup(frame)
    # (far: too few pixels for the shares; inside serves the ends of the range)
    r = decision_ref(frame) if frame not in ("far", "inside") else ref(frame, TOL[frame], 4)
    for o, q in zip(run(d, sc, cam, w, h, TOL[frame]), r):
        same(o, q)
    y_floor = 0.05
    r = ref(frame, 2.0 * TOL[frame], 8, True, y_floor)
    outs = run(d, sc, cam, w, h, 2.0 * TOL[frame], min_samples=8, relative=True, y_floor=y_floor)
    for o, q in zip(outs, r):
        same(o, q)
    assert outs[0]["active"] == plain(frame)["listed"]    # nobody is judged before min_samples
    z = np.zeros(1)                                        # resolved pixels: +0 in every plane, sign included
    res = ~plain(frame)["samples"].any((-1, -2)) & (outs[-1]["n"] == 8)
    for k in ("mean", "var", "rgb"):
        assert U.bits_equal(outs[-1][k][res], z).all()


@pytest.mark.parametrize("form", list(FORMS))
def test_smallest_tol_is_the_plain_frame(torch_cuda, form):
    """tol = 5e-324, min_samples = 2: only pixels of exactly zero variance stop early, and the final frame is the plain
    16-spp frame bit for bit.  The condition on the inputs: a pixel whose samples are constant up to a pass's end
    delivers that value at 16 samples too (cornell, inside; on zoo some pixels' first 4 jittered rays all miss and a later
    one hits: such a pixel stops with zero variance by the rule, so there the pixels that ran to 16 are compared)."""
    for frame in ("cornell", "inside", "zoo"):
        d, sc, cam, w, h = setup(frame)
        p, r = plain(frame), ref(frame, DENORMAL, 2)
        outs = run(d, sc, cam, w, h, DENORMAL, min_samples=2, flags=FORMS[form])
        for o, q in zip(outs, r):
            same(o, q)
        o, x = outs[-1], p["samples"]
        early = o["n"] < 16
        assert (o["var"][early] == 0).all() and (~early).sum() >= 100
        if frame != "zoo":
            # stated on the inputs through the restatement: the pixels it stops early keep their value to the end
            const = (x[:, :, :4] == x[:, :, :1]).all((-1, -2))
            assert (const | ~early).all() and U.bits_equal(r[-1]["rgb"], p["rgb"]).all(), frame
            early = np.zeros_like(early)
        assert U.bits_equal(o["rgb"][~early], p["rgb"][~early]).all() and (o["rgb8"][~early] == p["rgb8"][~early]).all()


def test_infinite_tol_is_the_four_sample_frame(torch_cuda):
    for frame in ("cornell", "far"):
        d, sc, cam, w, h = setup(frame)
        outs = run(d, sc, cam, w, h, INF, min_samples=2)
        rgb4, rgb4_8 = d.render(cam, sc.light, w, h, mode=gi.MODE_X, spp=4, depth=DEPTH, seed=SEED)
        for o in outs:   # everything stops at the first pass; the two further passes change no plane
            assert o["active"] == 0 and (o["n"] == 4).all()
            assert U.bits_equal(o["rgb"], rgb4).all() and (o["rgb8"] == rgb4_8).all()
            for k in ("mean", "var"):
                assert U.bits_equal(o[k], outs[0][k]).all()
        assert U.bits_equal(outs[0]["rgb"], oracle_frame(frame, 4)).all()


def device_planes(torch, w, h, pad=64):
    n = w * h
    f64 = dict(dtype=torch.float64, device="cuda")
    return {"rgb": torch.full((3 * n + pad,), -7.0, **f64), "mean": torch.full((3 * n + pad,), -7.0, **f64),
            "var": torch.full((3 * n + pad,), -7.0, **f64), "rgb8": torch.full((3 * n + pad,), 77, dtype=torch.uint8, device="cuda"),
            "n": torch.full((n + pad,), -7, dtype=torch.int32, device="cuda")}


def planes_np(t, w, h):
    """The planes as the host form shapes them, after checking the guarded tails."""
    n, out = w * h, {}
    for k, a in t.items():
        a = a.cpu().numpy()
        m = n if k == "n" else 3 * n
        assert (a[m:] == (77 if k == "rgb8" else -7)).all(), k
        out[k] = a[:m].reshape((h, w) if k == "n" else (h, w, 3))
    return out


@pytest.mark.parametrize("frame", ["cornell", "big"])
def test_passes_queued_without_a_host_read(torch_cuda, frame):
    """All passes queued on a side stream, each into its own planes with guarded tails, no host read in between:
    identical to the pass-by-pass run on that stream and to the host form."""
    torch = torch_cuda
    d, sc, cam, w, h = setup(frame)
    r = decision_ref(frame)
    host = run(d, sc, cam, w, h, TOL[frame])
    s1 = torch.cuda.Stream()
    assert s1.cuda_stream != 0

    def passes(sync):
        sets = [device_planes(torch, w, h) for _ in PASSES]
        torch.cuda.synchronize()
        for (b, e), t in zip(PASSES, sets):
            d.render_adaptive_device(cam, sc.light, w, h, (b, e), tol=TOL[frame], min_samples=4, stream=s1.cuda_stream,
                                     **{"d_" + k: a.data_ptr() for k, a in t.items()}, **KW)
            if sync:
                torch.cuda.synchronize()
                assert d.adaptive_info()["samples_done"] == e
        torch.cuda.synchronize()
        return [planes_np(t, w, h) for t in sets]
    queued, stepped = passes(False), passes(True)
    assert d.adaptive_info()["active"] == 0
    for q, s, o, ref_pass in zip(queued, stepped, host, r):
        for k in PLANES:
            assert U.bits_equal(q[k], s[k]).all() and U.bits_equal(q[k], o[k]).all(), k
        assert (q["n"] == ref_pass["n"]).all()
    # one plane alone: the others are not written
    t = device_planes(torch, w, h)
    torch.cuda.synchronize()
    d.render_adaptive_device(cam, sc.light, w, h, (0, 4), tol=TOL[frame], min_samples=4, stream=s1.cuda_stream, d_n=t["n"].data_ptr(), **KW)
    torch.cuda.synchronize()
    assert (t["n"].cpu().numpy()[:w * h].reshape(h, w) == host[0]["n"]).all()
    assert all((t[k] == (77 if k == "rgb8" else -7)).all().item() for k in ("rgb", "rgb8", "mean", "var"))


def test_scene_state(torch_cuda):
    """frame_moments after an adaptive pass is refused; the queries, the AOVs and the denoiser between passes leave the
    frame intact; a plain render after an adaptive frame equals itself from a fresh scene."""
    torch = torch_cuda
    frame = "cornell"
    d, sc, cam, w, h = setup(frame)
    r = decision_ref(frame)
    n = w * h
    f64 = dict(dtype=torch.float64, device="cuda")
    rays = torch.from_numpy(gi.camera_rays(cam, w, h).reshape(-1)).cuda()
    t, nrm, alb = torch.zeros(n, **f64), torch.zeros(3 * n, **f64), torch.zeros(3 * n, **f64)
    prim = torch.zeros(n, dtype=torch.int32, device="cuda")
    mean, var, out = torch.zeros(3 * n, **f64), torch.zeros(3 * n, **f64), torch.zeros(3 * n, **f64)
    scratch = torch.zeros(gi.denoise_var_scratch_bytes(w, h) // 8 + 2, **f64)

    def between(e):
        with pytest.raises(gi.GIError, match=r"\(-1\)"):
            d.frame_moments(w, h)
        with pytest.raises(gi.GIError, match=r"\(-1\)"):
            d.frame_samples_info()
        d.intersect_device(n, rays.data_ptr(), d_t=t.data_ptr(), d_prim=prim.data_ptr())
        d.render_aov_device(cam, w, h, d_t=t.data_ptr(), d_normal=nrm.data_ptr(), d_albedo=alb.data_ptr())
        mean.copy_(torch.from_numpy(outs_so_far[-1]["mean"].reshape(-1)))
        var.copy_(torch.from_numpy(outs_so_far[-1]["var"].reshape(-1)))
        gi.denoise_var_device(cam, w, h, mean.data_ptr(), var.data_ptr(), t.data_ptr(), nrm.data_ptr(), alb.data_ptr(),
                              scratch.data_ptr(), scratch.numel() * 8, d_out_rgb=out.data_ptr())
        torch.cuda.synchronize()
        assert np.isfinite(out.cpu().numpy()).all()
    outs_so_far = []
    for b, e in PASSES:
        o = d.render_adaptive(cam, sc.light, w, h, (b, e), tol=TOL[frame], min_samples=4, want=PLANES, **KW)
        o["active"] = d.adaptive_info()["active"]
        outs_so_far.append(o)
        between(e)
    for o, q in zip(outs_so_far, r):
        same(o, q)
    # a plain render after the adaptive frame, and the same render of a fresh scene
    rgb, rgb8 = d.render(cam, sc.light, w, h, mode=gi.MODE_X, spp=3, depth=DEPTH, seed=SEED + 1)
    with pytest.raises(gi.GIError, match=r"\(-1\)"):
        d.adaptive_info()
    f = setup(frame, fresh=True)[0]
    rgb_f, rgb8_f = f.render(cam, sc.light, w, h, mode=gi.MODE_X, spp=3, depth=DEPTH, seed=SEED + 1)
    f.close()
    assert U.bits_equal(rgb, rgb_f).all() and (rgb8 == rgb8_f).all()
    assert d.frame_samples_info()["n"] == 3


def test_rays_traced(torch_cuda):
    """GI_STAT_RAYS over the adaptive frame: below the plain 16-spp frame's when pixels stopped early, equal to it
    with the smallest tol on a frame where that stops no traced pixel."""
    torch = torch_cuda
    frame = "inside"
    d, sc, cam, w, h = setup(frame)
    p = plain(frame)
    stats = torch.zeros(gi.STATS_N, dtype=torch.int64, device="cuda")
    buf = torch.zeros(3 * w * h, dtype=torch.float64, device="cuda")

    def rays(go):
        stats.zero_()
        torch.cuda.synchronize()
        go()
        torch.cuda.synchronize()
        return int(stats[gi.STAT_RAYS].item())
    whole = rays(lambda: d.render_device(cam, sc.light, w, h, buf.data_ptr(), mode=gi.MODE_X, stats_ptr=stats.data_ptr(), **KW))

    def adaptive(tol, ms):
        for b, e in PASSES:
            d.render_adaptive_device(cam, sc.light, w, h, (b, e), tol=tol, min_samples=ms, stats_ptr=stats.data_ptr(),
                                     d_rgb=buf.data_ptr(), **KW)
    assert (ref(frame, TOL[frame], 4)[-1]["n"] < 16).sum() >= 20    # (the condition on the inputs: pixels stop early)
    some = rays(lambda: adaptive(TOL[frame], 4))
    assert 0 < some < whole
    # the condition on the inputs: with the smallest tol every listed pixel runs to 16
    assert int((ref(frame, DENORMAL, 2)[-1]["n"] == 16).sum()) == p["listed"]
    assert rays(lambda: adaptive(DENORMAL, 2)) == whole
    assert U.bits_equal(buf.cpu().numpy().reshape(h, w, 3), p["rgb"]).all()


def test_refusals(torch_cuda):
    """GI_ERR_ARG, with a message, and a good frame after all of it."""
    L = gi.lib()
    frame = "far"
    d, sc, cam, w, h = setup(frame, fresh=True)
    light = (ctypes.c_double * 3)(*sc.light)
    n_plane = np.zeros((h, w), np.int32)
    out = gi.AdaptiveOut(None, None, None, None, n_plane.ctypes.data)

    def call(o=None, p=None, a=out, c=cam, li=light, ww=w, hh=h, scene=d):
        o = gi.DeviceScene.opts(gi.MODE_X, SPP, DEPTH, SEED, samples=(0, 4)) if o is None else o
        p = gi.AdaptiveParams(4, 0, 0.05, 0.0) if p is None else p
        return L.gi_render_adaptive(scene._h if scene else None, ctypes.byref(c._c) if c else None, li, ww, hh,
                                    ctypes.byref(o) if o is not False else None, ctypes.byref(p) if p is not False else None,
                                    ctypes.byref(a) if a else None)

    def opts(samples=(0, 4), spp=SPP, mode=gi.MODE_X, seed=SEED, **kw):
        return gi.DeviceScene.opts(mode, spp, DEPTH, seed, samples=samples, **kw)
    assert call() == 0
    for bad in (dict(scene=None), dict(c=None), dict(li=None), dict(o=False), dict(p=False), dict(a=None),
                dict(a=gi.AdaptiveOut(None, None, None, None, None)), dict(ww=0), dict(hh=-1)):
        assert call(**bad) == -1 and len(L.gi_last_error()) > 0, bad
    nan = float("nan")
    for p in (gi.AdaptiveParams(1, 0, 0.05, 0.0), gi.AdaptiveParams(0, 0, 0.05, 0.0), gi.AdaptiveParams(4, 0, nan, 0.0),
              gi.AdaptiveParams(4, 0, 0.0, 0.0), gi.AdaptiveParams(4, 0, -1.0, 0.0), gi.AdaptiveParams(4, 1, 0.05, 0.0),
              gi.AdaptiveParams(4, 1, 0.05, -1.0), gi.AdaptiveParams(4, 1, 0.05, nan), gi.AdaptiveParams(4, 1, 0.05, INF),
              gi.AdaptiveParams(4, 2, 0.05, 0.1), gi.AdaptiveParams(4, 0x80000000, 0.05, 0.1)):
        assert call(p=p) == -1 and len(L.gi_last_error()) > 0, (p.min_samples, p.flags, p.tol, p.y_floor)
    assert call(p=gi.AdaptiveParams(2, 0, INF, nan)) == 0          # +inf is allowed; y_floor is not read without RELATIVE
    for o in (opts((0, 1)), opts((3, 4)), opts((0, 17)), opts((0, 0)), opts((4, 2)), opts((-2, 2)), opts(mode=gi.MODE_R),
              opts(shard_count=2), opts(shard_count=2, shard_index=1), opts((0, 4), spp=1)):
        assert call(o=o) == -1 and len(L.gi_last_error()) > 0, (o.sample_begin, o.sample_end, o.mode, o.shard_count)
    # out of order, and a changed frame mid-way
    kw = dict(tol=0.05, min_samples=4, want=("n",))
    with pytest.raises(gi.GIError, match=r"\(-1\)"):
        d.render_adaptive(cam, sc.light, w, h, (4, 8), **KW, **kw)             # no first pass (the refusals ended it)
    changes = [dict(seed=SEED + 1), dict(depth=DEPTH + 1), dict(spp=SPP + 1), dict(tol=0.06), dict(min_samples=5),
               dict(relative=True, y_floor=0.1), dict(flags=gi.FLAG_X_NO_SHADOW), dict(cam=gi.Camera((-41.0, 0.0, 0.0), sc.cam_look, sc.focal)),
               dict(light=(5.0, 0.0, 4.0)), dict(w=w + 1), dict(samples=(5, 8)), dict(samples=(0 + 2, 8))]
    for ch in changes:
        a = dict(KW, **kw)
        a.update({k: v for k, v in ch.items() if k not in ("cam", "light", "w", "samples")})
        d.render_adaptive(cam, sc.light, w, h, (0, 4), **KW, **kw)
        with pytest.raises(gi.GIError, match=r"\(-1\)"):
            d.render_adaptive(ch.get("cam", cam), ch.get("light", sc.light), ch.get("w", w), h, ch.get("samples", (4, 8)), **a)
        with pytest.raises(gi.GIError, match=r"\(-1\)"):                     # the refused pass ended the frame
            d.render_adaptive(cam, sc.light, w, h, (4, 8), **KW, **kw)
    # a plain progressive pass cannot continue an adaptive frame, nor the reverse; another render ends the frame
    d.render_adaptive(cam, sc.light, w, h, (0, 4), **KW, **kw)
    with pytest.raises(gi.GIError, match=r"\(-1\)"):
        d.render(cam, sc.light, w, h, mode=gi.MODE_X, samples=(4, 8), **KW)
    d.render(cam, sc.light, w, h, mode=gi.MODE_X, samples=(0, 4), **KW)
    with pytest.raises(gi.GIError, match=r"\(-1\)"):
        d.render_adaptive(cam, sc.light, w, h, (4, 8), **KW, **kw)
    d.render_adaptive(cam, sc.light, w, h, (0, 4), **KW, **kw)
    d.render(cam, sc.light, w, h, mode=gi.MODE_R)
    with pytest.raises(gi.GIError, match=r"\(-1\)"):
        d.render_adaptive(cam, sc.light, w, h, (4, 8), **KW, **kw)
    # a finished frame cannot be continued either; STATS and TIME may differ between passes
    for o, q in zip(run(d, sc, cam, w, h, TOL[frame]), ref(frame, TOL[frame], 4)):
        same(o, q)
    with pytest.raises(gi.GIError, match=r"\(-1\)"):
        d.render_adaptive(cam, sc.light, w, h, (16, 18), spp=18, depth=DEPTH, seed=SEED, **kw)
    d.render_adaptive(cam, sc.light, w, h, (0, 4), **KW, **kw)
    o = d.render_adaptive(cam, sc.light, w, h, (4, 8), flags=gi.FLAG_TIME, **KW, **kw)
    assert (o["n"] == ref(frame, 0.05, 4)[1]["n"]).all() and d.kernel_ms()[1] == 1
    d.close()
