"""GPU: the temporal accumulation (gi_temporal*; gi_temporal.hip k_temporal) against its numpy restatement
(tests/temporal_ref.py, judged on the CPU by tests/test_temporal_host.py), and in the device-resident chain of a preview
loop.  Everything compares bit for bit (U.bits_equal): there is no tolerance anywhere in this file."""
import ctypes
import itertools

import numpy as np
import pytest

import aov_frames as A
import oracle_util as U
import temporal_ref as T
from test_gpu_denoise import SHAPES, dev_of

pytestmark = pytest.mark.gpu

gi = U.pkg()
INF = float("inf")


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    return torch


def gcam(sc):
    return gi.Camera(sc.cam_pos, sc.cam_look, sc.focal)


# every combination of the stops at the default blend, then every combination of the blend's parameters at the default
# stops; with and without the variance in turn
CONFIGS = [dict(prim_stop=ps, cos_min=cm, sigma_p=sp, max_history=32, alpha_min=0.0)
           for ps, cm, sp in itertools.product((True, False), (-1.0, 0.9, 1.0), (0.01, INF))] + \
          [dict(prim_stop=True, cos_min=0.9, sigma_p=0.01, max_history=mh, alpha_min=am) for mh, am in itertools.product((1, 4, 32), (0.0, 0.2, 1.0))]
DEFAULTS = dict(prim_stop=True, cos_min=0.9, sigma_p=0.01, max_history=32, alpha_min=0.0)


def compare(cam, prev, sc, psc, w, h, window, cur, hist, cfg, carry=True, want=None):
    """gi.temporal against temporal_np on the same planes; returns (device outputs, reference)."""
    if not carry:
        cur = {k: a for k, a in cur.items() if k != "var"}
    want = want or (gi.TEMPORAL_OUTPUTS if carry else ("rgb", "len"))
    ref = T.temporal_np(sc, psc, w, h, cur, hist, window=window, **cfg)
    out = gi.temporal(cam, prev if hist is not None else None, w, h, cur, hist, window=window, want=want, **cfg)
    assert list(out) == list(want)
    for k in want:
        if k == "len":
            assert out[k].dtype == np.int32 and (out[k] == ref[k]).all(), (cfg, k, int((out[k] != ref[k]).sum()))
        else:
            ne = ~U.bits_equal(out[k], ref[k]).all(-1)
            assert not ne.any(), (cfg, k, int(ne.sum()), out[k][ne][:2], ref[k][ne][:2])
    return out, ref


@pytest.mark.parametrize("w,h,window", SHAPES)
def test_synthetic_pairs_equal_the_reference(torch_cuda, w, h, window):
    """Every camera pair of temporal_ref.PAIRS on seeded planes with holes and len in 0..40: out.rgb, out.var and out.len
    of the host form equal the restatement, for every configuration and for no history.  On the larger shapes the
    reference alone is first asked whether the pair is what its table entry says -- accepted pixels, reset pixels or
    both -- so that a degenerate input does not pass silently; "in_plane" and "far" must reach coordinates beyond an int."""
    x0, y0, x1, y1 = window if window is not None else (0, 0, w, h)
    rows, cols = y1 - y0, x1 - x0
    for name, (psc, kind) in T.PAIRS.items():
        sc, _, cur, hist = T.synthetic_pair(name, w, h, window, seed=w * 1000 + rows)
        cam, prev = gcam(sc), gcam(psc)
        for c, s in ((cam, sc), (prev, psc)):   # the numpy camera is the device's
            assert U.bits_equal(gi.camera_rays(c, w, h, window=window)[:, 3:6], A.rays_np(s, w, h, window)[:, 3:6]).all(), name
        if rows * cols > 2000:
            r = T.temporal_np(sc, psc, w, h, cur, hist, window=window, **DEFAULTS)
            acc, rst = T.counts(r, cur)
            assert (acc >= 20) == (kind != "reset") and (acc == 0) == (kind == "reset") and (rst >= 20 or kind == "accepted"), (name, acc, rst)
            valid = cur["t"] < INF
            if name == "far":
                assert np.abs(r["xs"][valid]).min() > 2.0 ** 31
            if name == "in_plane":
                assert (valid & ~(np.abs(r["xs"]) < 2.0 ** 31)).sum() >= 500
        for k, cfg in enumerate(CONFIGS):
            compare(cam, prev, sc, psc, w, h, window, cur, hist, cfg, carry=k % 2 == 0)
    sc, psc, cur, hist = T.synthetic_pair("pixels", w, h, window, seed=5)
    cam = gcam(sc)
    for carry in (True, False):
        out, _ = compare(cam, None, sc, None, w, h, window, cur, None, DEFAULTS, carry=carry)
        assert (out["len"] == (cur["t"] < INF)).all() and U.bits_equal(out["rgb"], cur["rgb"]).all()


def test_garbage_lengths_and_prims_are_only_compared(torch_cuda):
    """hist.len and the prim planes hold extreme values: they are compared and min'ed, never an index, and
    min(len_h + 1, max_history) does not overflow."""
    w, h = 64, 40
    sc, psc, cur, hist = T.synthetic_pair("subpixel", w, h, seed=9)
    g = np.random.default_rng(3)
    hist = dict(hist, len=g.choice(np.array([-2 ** 31, -1, 0, 1, 2 ** 31 - 2, 2 ** 31 - 1], np.int64), size=(h, w)).astype(np.int32))
    big = g.choice(np.array([-2 ** 31, 2 ** 31 - 1, 7], np.int64), size=(h, w)).astype(np.int32)
    cur, hist = dict(cur, prim=big), dict(hist, prim=big)
    for mh in (1, 32, 2 ** 31 - 1):
        out, ref = compare(gcam(sc), gcam(psc), sc, psc, w, h, None, cur, hist, dict(DEFAULTS, max_history=mh))
        assert (ref["taps"] > 0).sum() >= 200 and out["len"].max() <= mh and out["len"].min() >= 0


def test_want_subsets(torch_cuda):
    """Every non-empty selection of the outputs (the other pointers null) equals the same outputs of the full call."""
    w, h = 37, 21
    sc, psc, cur, hist = T.synthetic_pair("pixels", w, h, seed=4)
    for r in (1, 2):
        for want in itertools.combinations(gi.TEMPORAL_OUTPUTS, r):
            compare(gcam(sc), gcam(psc), sc, psc, w, h, None, cur, hist, DEFAULTS, carry="var" in want, want=want)


def _dev_frame(torch, d, pad=0, fill=None):
    """Device copies of a dict of planes (flat, with `pad` guard elements); returns (tensors, pointers)."""
    ts = {}
    for k, a in d.items():
        a = np.ascontiguousarray(a).reshape(-1)
        t = torch.empty(a.size + pad, dtype=torch.int32 if a.dtype == np.int32 else torch.float64, device="cuda")
        t[:a.size] = torch.from_numpy(a)
        if pad:
            t[a.size:] = fill
        ts[k] = t
    return ts, {k: t.data_ptr() for k, t in ts.items()}


def test_device_form_on_a_stream(torch_cuda):
    """temporal_device on a non-default stream equals the host form; the guarded tails of the outputs stay untouched,
    the inputs are not written, a null output is not written; then the GI_ERR_ARG cases with device planes -- outputs
    that alias an input, missing planes -- and the empty window, which returns GI_OK and writes nothing."""
    torch = torch_cuda
    w, h, pad = 64, 40, 64
    n = w * h
    sc, psc, cur, hist = T.synthetic_pair("pixels", w, h, seed=8)
    cam, prev = gcam(sc), gcam(psc)
    kw = dict(DEFAULTS, max_history=8, alpha_min=0.1)
    host = gi.temporal(cam, prev, w, h, cur, hist, **kw)
    tc, pc = _dev_frame(torch, cur)
    th, ph = _dev_frame(torch, hist)
    f64 = dict(dtype=torch.float64, device="cuda")
    o_rgb, o_var = torch.full((3 * n + pad,), -7.0, **f64), torch.full((3 * n + pad,), -7.0, **f64)
    o_len = torch.full((n + pad,), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    assert st.cuda_stream != 0
    gi.temporal_device(cam, prev, w, h, pc, ph, d_out_rgb=o_rgb.data_ptr(), d_out_var=o_var.data_ptr(), d_out_len=o_len.data_ptr(),
                       stream=st.cuda_stream, **kw)
    st.synchronize()
    r, v, ln = o_rgb.cpu().numpy(), o_var.cpu().numpy(), o_len.cpu().numpy()
    assert (r[3 * n:] == -7.0).all() and (v[3 * n:] == -7.0).all() and (ln[n:] == -7).all()
    assert U.bits_equal(r[:3 * n], host["rgb"].reshape(-1)).all() and U.bits_equal(v[:3 * n], host["var"].reshape(-1)).all()
    assert (ln[:n] == host["len"].reshape(-1)).all()
    assert (host["len"] > 1).sum() >= 100 and (host["len"] == 1).sum() >= 20 and (host["len"] == 0).sum() >= 20
    for ts, d in ((tc, cur), (th, hist)):
        for k, a in d.items():
            assert (ts[k].cpu().numpy() == a.reshape(-1)).all() or U.bits_equal(ts[k].cpu().numpy(), a.reshape(-1)).all(), k
    # without the variance and the prim stop those planes may be null; a null output is not written
    o_rgb.fill_(-7.0)
    kw2 = dict(kw, prim_stop=False)
    lean = ("rgb", "t", "normal")
    gi.temporal_device(cam, prev, w, h, {k: pc[k] for k in lean}, {k: ph[k] for k in lean + ("len",)}, d_out_rgb=o_rgb.data_ptr(),
                       stream=st.cuda_stream, **kw2)
    st.synchronize()
    host2 = gi.temporal(cam, prev, w, h, {k: cur[k] for k in lean}, {k: hist[k] for k in lean + ("len",)}, want=("rgb",), **kw2)
    assert U.bits_equal(o_rgb.cpu().numpy()[:3 * n], host2["rgb"].reshape(-1)).all()
    assert U.bits_equal(o_var.cpu().numpy(), v).all() and (o_len.cpu().numpy() == ln).all()

    # ---- argument errors with device planes ----
    L = gi.lib()
    P, good_f = gi.TemporalParams, gi.AovFrame(w, h, 0, 0, w, h)

    def call(cur_kw=None, hist_kw=None, out_kw=None, f=good_f, p=P(32, 1, 0.0, 0.9, 0.01), no_hist=False):
        fc = gi.TemporalFrame(**{k: a for k, a in dict(pc, **(cur_kw or {})).items() if a})
        fh = gi.TemporalFrame(**{k: a for k, a in dict(ph, **(hist_kw or {})).items() if a})
        fo = gi.TemporalOut(**{k: a for k, a in dict(dict(rgb=o_rgb.data_ptr(), var=o_var.data_ptr(), len=o_len.data_ptr()), **(out_kw or {})).items() if a})
        return L.gi_temporal_device(ctypes.byref(cam._c), ctypes.byref(prev._c), ctypes.byref(f), ctypes.byref(p), ctypes.byref(fc),
                                    None if no_hist else ctypes.byref(fh), ctypes.byref(fo), st.cuda_stream)

    def refused(rc):
        assert rc == -1 and len(L.gi_last_error()) > 0, (rc, L.gi_last_error())
    o_rgb.fill_(-7.0)
    torch.cuda.synchronize()
    for k in ("rgb", "var", "t", "normal"):
        refused(call(out_kw={"rgb": pc[k]})), refused(call(out_kw={"var": ph[k]})), refused(call(out_kw={"rgb": ph[k]}))
    for k in ("prim",):
        refused(call(out_kw={"len": pc[k]})), refused(call(out_kw={"len": ph[k]}))
    refused(call(out_kw={"len": ph["len"]}))
    for k in ("rgb", "t", "normal", "prim", "var"):
        refused(call(cur_kw={k: 0})), refused(call(hist_kw={k: 0}))
    refused(call(hist_kw={"len": 0})), refused(call(out_kw=dict(rgb=0, var=0, len=0)))
    refused(call(cur_kw={"var": 0}, no_hist=True)), refused(call(cur_kw={"prim": 0}, no_hist=True))
    refused(call(p=P(0, 1, 0.0, 0.9, 0.01))), refused(call(p=P(32, 1, 0.0, 0.9, np.nan))), refused(call(f=gi.AovFrame(w, h, 0, 0, w + 1, h)))
    with pytest.raises(gi.GIError, match=r"\(-1\)"):
        gi.temporal_device(cam, None, w, h, pc, ph, d_out_rgb=o_rgb.data_ptr())
    with pytest.raises(gi.GIError, match=r"\(-1\)"):
        gi.temporal(cam, prev, w, h, cur, hist, sigma_p=0.0)
    # the empty window: GI_OK, nothing launched, nothing written (the refused calls wrote nothing either)
    assert call(f=gi.AovFrame(w, h, 5, 3, 5, 20)) == 0 and call(f=gi.AovFrame(w, h, 5, 3, 30, 3), no_hist=True) == 0
    st.synchronize()
    torch.cuda.synchronize()
    assert (o_rgb.cpu().numpy() == -7.0).all() and U.bits_equal(o_var.cpu().numpy(), v).all() and (o_len.cpu().numpy() == ln).all()
    e = gi.temporal(cam, prev, w, h, {k: a[3:3, 5:30] for k, a in cur.items()}, {k: a[3:3, 5:30] for k, a in hist.items()}, window=(5, 3, 30, 3))
    assert e["rgb"].shape == (0, 25, 3) and e["len"].shape == (0, 25)


def test_a_preview_loop_stays_on_the_device(torch_cuda):
    """Three frames of the Cornell box at 64 x 40, 4 spp, depth 4, a camera that moves and a new seed per frame, all
    device-resident on one non-default stream: render_device, frame_moments_device, render_aov_device, temporal_device
    (two history sets swapped), denoise_var_device.  Every frame's accumulated and filtered planes equal the same chain
    through the host forms bit for bit, and the temporal output equals temporal_np fed with the device's own inputs."""
    torch = torch_cuda
    d = dev_of("cornell")
    base, _, w, h = A.frame_scene("cornell/0.01")
    n = w * h
    f64 = dict(dtype=torch.float64, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    frame_rgb = torch.zeros(3 * n, **f64)
    alb = torch.zeros(3 * n, **f64)

    def plane_set():
        return dict(rgb=torch.zeros(3 * n, **f64), var=torch.zeros(3 * n, **f64), t=torch.zeros(n, **f64), normal=torch.zeros(3 * n, **f64),
                    prim=torch.zeros(n, **i32), len=torch.zeros(n, **i32))
    mom = dict(rgb=torch.zeros(3 * n, **f64), var=torch.zeros(3 * n, **f64))   # this frame's mean and variance
    sets = [plane_set(), plane_set()]   # history sets: accumulated rgb, var, len and the frame's own t, normal, prim
    out_rgb, out_var = torch.zeros(3 * n, **f64), torch.zeros(3 * n, **f64)
    dkw = dict(levels=3, sigma_v=gi.DENOISE_VAR_SIGMA_V, sigma_p=0.01, var_floor=gi.DENOISE_VAR_FLOOR, normal_pow_log2=5, albedo_stop=True)
    nbytes = gi.denoise_var_scratch_bytes(w, h, **dkw)
    scratch = torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    s = st.cuda_stream
    ptr = lambda t: t.data_ptr()   # noqa: E731
    prev_cam, prev_sc, h_hist = None, None, None
    for k in range(3):
        sc = T.moved(base, (0.0, 0.15 * k, 0.05 * k))
        cam = gi.Camera(sc.cam_pos, sc.cam_look, sc.focal)
        new, old = sets[k & 1], sets[(k & 1) ^ 1]
        # ---- the device chain ----
        d.render_device(cam, base.light, w, h, ptr(frame_rgb), stream=s, mode=gi.MODE_X, spp=4, depth=4, seed=1 + k)
        d.frame_moments_device(w, h, d_mean=ptr(mom["rgb"]), d_var=ptr(mom["var"]), stream=s)
        d.render_aov_device(cam, w, h, d_t=ptr(new["t"]), d_normal=ptr(new["normal"]), d_albedo=ptr(alb), d_prim=ptr(new["prim"]), stream=s)
        d_cur = dict(rgb=ptr(mom["rgb"]), var=ptr(mom["var"]), t=ptr(new["t"]), normal=ptr(new["normal"]), prim=ptr(new["prim"]))
        gi.temporal_device(cam, prev_cam, w, h, d_cur, {q: ptr(a) for q, a in old.items()} if k else None, d_out_rgb=ptr(new["rgb"]),
                           d_out_var=ptr(new["var"]), d_out_len=ptr(new["len"]), stream=s)
        gi.denoise_var_device(cam, w, h, ptr(new["rgb"]), ptr(new["var"]), ptr(new["t"]), ptr(new["normal"]), ptr(alb), ptr(scratch), nbytes,
                              d_out_rgb=ptr(out_rgb), d_out_var=ptr(out_var), stream=s, **dkw)
        st.synchronize()
        dev = {q: a.cpu().numpy() for q, a in new.items()}
        dev_cur = dict(rgb=mom["rgb"].cpu().numpy().reshape(h, w, 3), var=mom["var"].cpu().numpy().reshape(h, w, 3),
                       t=dev["t"].reshape(h, w), normal=dev["normal"].reshape(h, w, 3), prim=dev["prim"].reshape(h, w))
        # ---- the same chain through the host forms ----
        d.render(cam, base.light, w, h, mode=gi.MODE_X, spp=4, depth=4, seed=1 + k)
        m = d.frame_moments(w, h)
        aov = d.render_aov(cam, w, h, want=("t", "normal", "albedo", "prim"))
        h_cur = dict(rgb=m["mean"], var=m["var"], t=aov["t"], normal=aov["normal"], prim=aov["prim"])
        for q in h_cur:
            assert (h_cur[q] == dev_cur[q]).all() if q == "prim" else U.bits_equal(h_cur[q], dev_cur[q]).all(), (k, q)
        acc = gi.temporal(cam, prev_cam, w, h, h_cur, h_hist)
        flt = gi.denoise_var(cam, w, h, acc["rgb"], acc["var"], aov["t"], aov["normal"], aov["albedo"], want=("rgb", "var"), **dkw)
        assert U.bits_equal(dev["rgb"], acc["rgb"].reshape(-1)).all() and U.bits_equal(dev["var"], acc["var"].reshape(-1)).all(), k
        assert (dev["len"] == acc["len"].reshape(-1)).all(), k
        assert U.bits_equal(out_rgb.cpu().numpy(), flt["rgb"].reshape(-1)).all() and U.bits_equal(out_var.cpu().numpy(), flt["var"].reshape(-1)).all(), k
        # ---- and the restatement on the device's own inputs ----
        ref = T.temporal_np(sc, prev_sc, w, h, dev_cur, h_hist)
        assert U.bits_equal(ref["rgb"], acc["rgb"]).all() and U.bits_equal(ref["var"], acc["var"]).all() and (ref["len"] == acc["len"]).all(), k
        valid = aov["t"] < INF
        if k:
            assert (acc["len"][valid] == k + 1).mean() > 0.8 and (acc["len"][valid] == 1).sum() >= 1 and (acc["len"][~valid] == 0).all()
            assert (~U.bits_equal(acc["rgb"], m["mean"]).all(-1))[acc["len"] > 1].mean() > 0.9
        h_hist = dict(h_cur, rgb=acc["rgb"], var=acc["var"], len=acc["len"])
        prev_cam, prev_sc = cam, sc
