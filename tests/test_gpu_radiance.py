"""GPU: the radiance query, the sample rays and the resolve (gi_radiance*, gi_sample_rays*, gi_resolve_samples*;
gi_wf.hip k_rad, gi_sample.hip) against the renders' own per-sample rows, the CPU oracle's frames and the numpy
restatement (tests/radiance_ref.py).  Everything compares bit for bit (U.bits_equal): there is no tolerance
anywhere in this file.

The frames are small (64 x 40 and below) and chosen on the CPU so that paths do bounce: check_inputs asserts for
every frame that the oracle's first hits cover at least 30 % of its pixels and that its depth-4 frame differs from
its depth-1 frame on at least 10 % of those.  Where the frame tests/aov_frames.py has for a scene does not (the
soups and the stacks: a path that leaves a triangle meets nothing), the variant is covered by a frame that does:
the scene's own from another camera or focal length, or the Cornell box built so that it runs that variant."""
import copy
import ctypes
import os

import numpy as np
import pytest

import aov_frames as A
import oracle_util as U
import radiance_ref as RR
from x_scenes import QUERY_SCENES, with_env

pytestmark = pytest.mark.gpu

gi = U.pkg()
S = U.scenes()
SEED = 1
GUARD = -7.0


def _query_scene(name, focal, pos=None, look=None):
    def make():
        sc, env = QUERY_SCENES[name][0]()
        sc = copy.deepcopy(sc)
        sc.focal = focal
        if pos is not None:
            sc.cam_pos, sc.cam_look = pos, look
        return sc, env
    return make


def _frame(key):
    return lambda: A.frame_scene(key)[:2]


def _cornell_single_leaves():
    """The Cornell box with one triangle per leaf: 34 leaves, more than the flat table holds -- the tree walk over
    the scene staged in LDS."""
    sc = S.cornell_scene()
    sc.focal = 0.004
    return sc, {"GI_XLEAF_MAX": "1"}


def _cornell_in_soup():
    """The Cornell box with the 1000-triangle soup inside it: too large for LDS, triangles only -- the wide nodes
    in HBM."""
    sc = S.cornell_scene()
    sc.focal = 0.004
    sc.entities.extend(copy.deepcopy(S.named_scene("soup1000").entities))
    return sc, {}


# case -> (builder of (scene, env), w, h, window or None, the variant gi_kat_x_variant must report, x_lds_resident)
CASES = {
    "cornell": (_frame("cornell/0.01"), 64, 40, None, dict(LDS=True, W4=True, TRI=True, FLAT=True), 1),
    "cornell_sphere": (_frame("cornell_sphere/0.004"), 37, 21, None, dict(LDS=True, W4=False, TRI=False, FLAT=True), 1),
    "cornell_mirror": (_query_scene("cornell_mirror", 0.004), 37, 21, None, dict(LDS=True, FLAT=True), 1),
    "lds_tree": (_cornell_single_leaves, 37, 21, None, dict(LDS=True, SH=True, FLAT=False), 1),
    "lds_deep_tree": (_query_scene("corner3_octree", 0.02, (12.0, 0.0, 3.0), (4.1, 0.3, -0.7)), 37, 21, None,
                      dict(LDS=True, SH=False, FLAT=False), 1),
    "hbm_tri": (_cornell_in_soup, 37, 21, None, dict(LDS=False, TRI=True, CN=False, FLAT=False), 0),
    "hbm_zoo": (_frame("zoo"), 37, 21, None, dict(LDS=False, TRI=False, CN=False, FLAT=False), 0),
    "hbm_quantised": (_query_scene("soup_xcnode", 0.006), 37, 21, (9, 5, 28, 16), dict(LDS=False, TRI=True, CN=True, FLAT=False), 0),
}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    return torch


_devs, _oracle = {}, {}


def setup(case):
    """(device scene, scene, camera, w, h, window) of a case; built once, its variant asserted when it is built."""
    make, w, h, win, variant, lds = CASES[case]
    if case not in _devs:
        sc, env = make()
        d = with_env(env, lambda: gi.DeviceScene.from_scene(sc))
        var, info = d.kat_x_variant(0), d.info()
        assert {k: var[k] for k in variant} == variant, (case, var)
        assert info["x_lds_resident"] == lds, (case, info)
        _devs[case] = (d, sc)
    d, sc = _devs[case]
    return d, sc, gi.Camera(sc.cam_pos, sc.cam_look, sc.focal), w, h, win if win is not None else (0, 0, w, h)


def oracle_frame(case, depth, k, no_shadow=False, sc=None, tag=None):
    """The oracle's Mode X frame of spp = k over the case's window, (pixels, 3); computed once, read-only."""
    key = (case, depth, k, no_shadow, tag)
    if key not in _oracle:
        _, w, h, win, _, _ = CASES[case]
        sc = sc if sc is not None else _devs[case][1]
        U.oracle_no_shadow(no_shadow)
        try:
            o = U.oracle_render(sc.to_scn(), w, h, mode=1, spp=k, depth=depth, seed=SEED, window=win)
        finally:
            U.oracle_no_shadow(False)
        for a in o.values():
            a.setflags(write=False)
        _oracle[key] = o
    return _oracle[key]


def check_inputs(case):
    """The frame exercises the paths: first hits on at least 30 % of its pixels, and the depth-4 frame differs from
    the depth-1 frame on at least 10 % of those."""
    o1, o4 = oracle_frame(case, 1, 1), oracle_frame(case, 4, 1)
    hit = o1["hit"] >= 0
    bounced = hit & ~U.bits_equal(o1["rgb"], o4["rgb"]).all(1)
    assert hit.sum() >= 0.3 * len(hit), (case, int(hit.sum()), len(hit))
    assert bounced.sum() >= 0.1 * hit.sum(), (case, int(bounced.sum()), int(hit.sum()))


class Dev:
    """Device buffers of one radiance pipeline over n records, each with a guarded tail."""
    PAD = 64

    def __init__(self, torch, n, n_pix=0):
        f64 = dict(dtype=torch.float64, device="cuda")
        self.torch, self.n, self.n_pix = torch, n, n_pix
        self.rays = torch.full((8 * n + self.PAD,), GUARD, **f64)
        self.ids = torch.full((2 * n + self.PAD,), -7, dtype=torch.int64, device="cuda")
        self.rows = torch.full((3 * n + self.PAD,), GUARD, **f64)
        self.rgb = torch.full((3 * n_pix + self.PAD,), GUARD, **f64)
        self.rgb8 = torch.full((3 * n_pix + self.PAD,), 99, dtype=torch.uint8, device="cuda")
        assert self.rays.data_ptr() % 16 == 0

    def put(self, rays, ids):
        t = self.torch
        self.rays[:8 * self.n] = t.from_numpy(np.ascontiguousarray(rays).reshape(-1)).cuda()
        self.ids[:2 * self.n] = t.from_numpy(np.ascontiguousarray(ids).view(np.int64).reshape(-1)).cuda()

    def get(self):
        """(rays, ids, rows) as numpy; the guards behind each are asserted untouched."""
        self.torch.cuda.synchronize()
        r, i, o = self.rays.cpu().numpy(), self.ids.cpu().numpy(), self.rows.cpu().numpy()
        n = self.n
        assert (r[8 * n:] == GUARD).all() and (i[2 * n:] == -7).all() and (o[3 * n:] == GUARD).all()
        return r[:8 * n].reshape(n, 8), i[:2 * n].copy().view(gi.PATH_ID_DTYPE).reshape(n), o[:3 * n].reshape(n, 3)

    def pixels(self):
        self.torch.cuda.synchronize()
        a, b = self.rgb.cpu().numpy(), self.rgb8.cpu().numpy()
        m = 3 * self.n_pix
        assert (a[m:] == GUARD).all() and (b[m:] == 99).all()
        return a[:m].reshape(-1, 3), b[:m].reshape(-1, 3)


def radiance_rows(torch, d, sc, rays, ids, depth, flags=0, seed=SEED):
    """radiance_device over host records: (n, 3)."""
    b = Dev(torch, len(rays))
    b.put(rays, ids)
    d.radiance_device(len(rays), b.rays.data_ptr(), b.rows.data_ptr(), sc.light, depth, d_ids=b.ids.data_ptr(), seed=seed, flags=flags)
    return b.get()[2].copy()


def render_rows(torch, d, cam, sc, w, h, win, spp, depth, flags=0):
    """A plain render_device of the frame: (its rows over the window (pixels, spp, 3), rgb, rgb8 over the window)."""
    rgb = torch.full((3 * w * h,), GUARD, dtype=torch.float64, device="cuda")
    rgb8 = torch.full((3 * w * h,), 99, dtype=torch.uint8, device="cuda")
    d.render_device(cam, sc.light, w, h, rgb.data_ptr(), rgb8.data_ptr(), mode=gi.MODE_X, spp=spp, depth=depth, seed=SEED, flags=flags)
    torch.cuda.synchronize()
    rows = d.frame_moments(w, h, window=win, want=("samples",))["samples"] if spp > 1 else None
    return (None if rows is None else rows.reshape(-1, spp, 3), A.window_of(rgb.cpu().numpy().reshape(-1, 3), w, h, win).reshape(-1, 3),
            A.window_of(rgb8.cpu().numpy().reshape(-1, 3), w, h, win).reshape(-1, 3))


def pipeline(torch, d, cam, sc, w, h, win, s0, s1, depth, jitter, flags=0, aperture=0.0, focus=1.0):
    """sample_rays_device -> radiance_device -> resolve_samples_device on one stream, nothing read between them:
    (rays, ids, rows (pixels, ns, 3), rgb, rgb8)."""
    x0, y0, x1, y1 = win
    n_pix, ns = (x1 - x0) * (y1 - y0), s1 - s0
    b = Dev(torch, n_pix * ns, n_pix)
    st = torch.cuda.Stream()
    q = st.cuda_stream
    torch.cuda.synchronize()
    gi.sample_rays_device(cam, w, h, b.rays.data_ptr(), b.ids.data_ptr(), samples=(s0, s1), window=win, seed=SEED, jitter=jitter,
                          aperture=aperture, focus=focus, stream=q)
    d.radiance_device(b.n, b.rays.data_ptr(), b.rows.data_ptr(), sc.light, depth, d_ids=b.ids.data_ptr(), seed=SEED, flags=flags, stream=q)
    gi.resolve_samples_device(n_pix, ns, b.rows.data_ptr(), b.rgb.data_ptr(), b.rgb8.data_ptr(), stream=q)
    rays, ids, rows = b.get()
    rgb, rgb8 = b.pixels()
    return rays, ids, rows.reshape(n_pix, ns, 3), rgb, rgb8


def assert_records(got_rays, got_ids, exp_rays, exp_ids):
    assert U.bits_equal(got_rays, exp_rays).all(), int((~U.bits_equal(got_rays, exp_rays)).any(1).sum())
    for f in ("stream", "sample", "reserved"):
        assert (got_ids[f] == exp_ids[f]).all(), f


def prefix_frames(rows):
    """{k: resolve_np of the first k samples} for k = 2 .. ns."""
    return {k: RR.resolve_np(rows[:, :k]) for k in range(2, rows.shape[1] + 1)}


# ---- 1. the render's rows ------------------------------------------------------------------------------------
@pytest.mark.parametrize("depth", [1, 4])
@pytest.mark.parametrize("case", list(CASES))
def test_rows_are_the_renders_rows(torch_cuda, case, depth):
    """Every variant, depth 1 and 4.  For spp in {2, 5}: the sample rays are the numpy restatement's; radiance over
    them is the samples plane of a plain render of the frame; every prefix resolves to the oracle's frame of that
    spp; resolve_samples gives the render's rgb and rgb8.  spp = 1: no jitter, sample 0, the 1-spp frame.  (The
    oracle's frames bound the time: the 31089-triangle soup costs about a second per frame whatever its size.)"""
    torch = torch_cuda
    d, sc, cam, w, h, win = setup(case)
    check_inputs(case)
    for depth in (depth,):
        for spp in (2, 5):
            rays, ids, rows, rgb, rgb8 = pipeline(torch, d, cam, sc, w, h, win, 0, spp, depth, True)
            assert_records(rays, ids, *RR.sample_rays_np(sc, w, h, win, SEED, 0, spp, True, 0.0, 1.0))
            r_rows, r_rgb, r_rgb8 = render_rows(torch, d, cam, sc, w, h, win, spp, depth)
            ne = ~U.bits_equal(rows, r_rows)
            assert not ne.any(), (case, depth, spp, int(ne.any((1, 2)).sum()), rows[ne][:3], r_rows[ne][:3])
            for k, f in prefix_frames(rows).items():
                ne = ~U.bits_equal(f, oracle_frame(case, depth, k)["rgb"])
                assert not ne.any(), (case, depth, spp, k, int(ne.any(1).sum()))
            assert U.bits_equal(rgb, r_rgb).all() and (rgb8 == r_rgb8).all()
            assert U.bits_equal(rgb, RR.resolve_np(rows)).all() and (rgb8 == RR.quantize_np(rgb)).all()
        rays, ids, rows, rgb, rgb8 = pipeline(torch, d, cam, sc, w, h, win, 0, 1, depth, False)
        assert_records(rays, ids, *RR.sample_rays_np(sc, w, h, win, SEED, 0, 1, False, 0.0, 1.0))
        _, r_rgb, r_rgb8 = render_rows(torch, d, cam, sc, w, h, win, 1, depth)
        o = oracle_frame(case, depth, 1)
        assert U.bits_equal(rgb, o["rgb"]).all() and U.bits_equal(rgb, r_rgb).all() and (rgb8 == r_rgb8).all() and (rgb8 == o["q"]).all()
        assert U.bits_equal(np.where(rows[:, 0] < 1.0, rows[:, 0], 1.0), rgb).all()
    assert (rows > 0).any()


def test_mirror_scene_has_mirrors_and_no_shadow_rows(torch_cuda):
    """The mirror case's materials reflect (mat_reflectivity > 0), so its paths take the dim-4 choice; and with
    GI_FLAG_X_NO_SHADOW the rows are those of a render with the flag and of the oracle without shadow rays, and
    differ from the shadowed rows."""
    torch = torch_cuda
    d, sc, cam, w, h, win = setup("cornell_mirror")
    assert any(e.material is not None and e.material.reflectivity > 0 for e in sc.entities)
    for case in ("cornell_mirror", "cornell"):
        d, sc, cam, w, h, win = setup(case)
        rays, ids, rows, rgb, rgb8 = pipeline(torch, d, cam, sc, w, h, win, 0, 3, 4, True, flags=gi.FLAG_X_NO_SHADOW)
        r_rows, r_rgb, r_rgb8 = render_rows(torch, d, cam, sc, w, h, win, 3, 4, flags=gi.FLAG_X_NO_SHADOW)
        assert U.bits_equal(rows, r_rows).all() and U.bits_equal(rgb, r_rgb).all() and (rgb8 == r_rgb8).all()
        for k, f in prefix_frames(rows).items():
            assert U.bits_equal(f, oracle_frame(case, 4, k, no_shadow=True)["rgb"]).all(), (case, k)
        lit = pipeline(torch, d, cam, sc, w, h, win, 0, 3, 4, True)[2]
        assert not U.bits_equal(rows, lit).all()


# ---- 2. origins mixed in one call ----------------------------------------------------------------------------
def _cameras():
    """The Cornell box (extent 10) from its own camera, from inside the box, and from 1e3 and 1e6 extents out,
    the focal length grown with the distance so that the box stays in the frame."""
    out = []
    for tag, pos, look, focal in (("default", (-10.0, 0.0, 0.0), (1.0, 0.0, 0.0), 0.004),
                                  ("inside", (4.0, 1.0, -1.0), (10.0, -2.0, 1.0), 0.004),
                                  ("far_1e3", (-1e4, 300.0, 200.0), (5.0, 0.0, 0.0), 4.0),
                                  ("far_1e6", (-1e7, -2e5, 3e5), (5.0, 0.0, 0.0), 4000.0)):
        sc = S.cornell_scene()
        sc.cam_pos, sc.cam_look, sc.focal = pos, look, focal
        out.append((tag, sc))
    return out


def test_origins_mixed_in_one_call(torch_cuda):
    """Four cameras' records concatenated and permuted (seed 2019), so that the lanes of a wave carry near and far
    origins and different streams: every record's row is the row it has in its own camera's batch, and each
    camera's prefixes resolve to the oracle's frames from that camera."""
    torch = torch_cuda
    d, _, _, _, _, _ = setup("cornell")
    w, h, spp, depth = 37, 21, 3, 4
    own, recs, idl = [], [], []
    for tag, sc in _cameras():
        cam = gi.Camera(sc.cam_pos, sc.cam_look, sc.focal)
        rays, ids, rows, _, _ = pipeline(torch, d, cam, sc, w, h, (0, 0, w, h), 0, spp, depth, True)
        assert_records(rays, ids, *RR.sample_rays_np(sc, w, h, None, SEED, 0, spp, True, 0.0, 1.0))
        hits = 0
        for k, f in prefix_frames(rows).items():
            o = U.oracle_render(sc.to_scn(), w, h, mode=1, spp=k, depth=depth, seed=SEED)
            assert U.bits_equal(f, o["rgb"]).all(), (tag, k)
            hits = int((o["hit"] >= 0).sum())
        assert hits >= 100, (tag, hits)
        own.append(rows.reshape(-1, 3))
        recs.append(rays)
        idl.append(ids)
    rays, ids, exp = np.concatenate(recs), np.concatenate(idl), np.concatenate(own)
    p = np.random.default_rng(2019).permutation(len(rays))
    far = np.abs(rays[p, 0]) > 1e3
    waves = [far[k:k + 64] for k in range(0, len(p) - 63, 64)]
    assert sum(1 for v in waves if v.any() and not v.all()) >= len(waves) // 2
    got = radiance_rows(torch, d, S.cornell_scene(), np.ascontiguousarray(rays[p]), np.ascontiguousarray(ids[p]), depth)
    ne = ~U.bits_equal(got, exp[p])
    assert not ne.any(), (int(ne.any(1).sum()), rays[p][ne.any(1)][:2])


# ---- 3. schedule ---------------------------------------------------------------------------------------------
def _records(n):
    """n records of the Cornell case's jittered frame (64 x 40, 5 samples: 12800), drawn by a seeded permutation."""
    sc = _devs["cornell"][1]
    rays, ids = RR.sample_rays_np(sc, 64, 40, None, SEED, 0, 5, True, 0.0, 1.0)
    p = np.random.default_rng(7).permutation(len(rays))[:n]
    return np.ascontiguousarray(rays[p]), np.ascontiguousarray(ids[p])


def _in_batches(torch, d, sc, rays, ids, depth, m=64):
    return np.concatenate([radiance_rows(torch, d, sc, rays[k:k + m], ids[k:k + m], depth) for k in range(0, len(rays), m)])


def test_counts_that_are_no_multiple_of_a_wave_and_malformed_records(torch_cuda):
    """n = 1, and n = 64 * 9 + 37 with malformed records -- a NaN in o, an infinite d, a zero d -- between good
    ones: they yield (0, 0, 0), every other row is what the record has alone in batches of 64 without them, and
    the guard behind the output stays untouched (Dev.get)."""
    torch = torch_cuda
    d, sc, _, _, _, _ = setup("cornell")
    rays, ids = _records(64 * 9 + 37)
    clean = _in_batches(torch, d, sc, rays, ids, 4)
    assert (clean != 0).any(1).sum() >= 200
    one = radiance_rows(torch, d, sc, rays[5:6], ids[5:6], 4)
    assert U.bits_equal(one, clean[5:6]).all()
    bad = rays.copy()
    k_nan, k_inf, k_zero = np.arange(3, len(rays), 11), np.arange(7, len(rays), 13), np.arange(1, len(rays), 17)
    bad[k_nan, 1] = np.nan
    bad[k_inf, 4] = np.inf
    bad[k_zero, 3:6] = 0.0
    bad[::5, 6] = np.nan     # tmax and reserved are ignored, whatever they hold
    bad[::3, 7] = -1.0
    mal = np.zeros(len(rays), bool)
    mal[np.concatenate([k_nan, k_inf, k_zero])] = True
    got = radiance_rows(torch, d, sc, bad, ids, 4)
    assert U.bits_equal(got[mal], np.zeros(1)).all()
    assert U.bits_equal(got[~mal], clean[~mal]).all()
    assert (clean[mal] != 0).any()   # (they would have carried radiance)


def test_refill_across_a_run_boundary(torch_cuda):
    """GI_RAD_MAX_GRID=1 (read at every launch) makes the launch one workgroup: W = 4 waves, and wave w owns the
    runs w, w + 4, ... of 64 records -- with n = 64 * 4 * 3 + 17, three or four each.  That a refill crosses a run
    boundary is known from the records: five of the first 64 are malformed, so wave 0's first refill round hands
    its 64 lanes run 0, five of them resolve at once (no path), and the second round of the same loop iteration
    finds run 0 used up and gives those five lanes the first five records of run 4 -- lanes of one wave then carry
    records of two runs, and every later refill of the wave begins inside a run.  Results equal those of the same
    records in batches of 64 in a launch without the knob."""
    torch = torch_cuda
    d, sc, _, _, _, _ = setup("cornell")
    n = 64 * 4 * 3 + 17
    rays, ids = _records(n)
    rays[[2, 11, 23, 40, 63], 0] = np.nan
    ref = _in_batches(torch, d, sc, rays, ids, 4)
    assert "GI_RAD_MAX_GRID" not in os.environ
    os.environ["GI_RAD_MAX_GRID"] = "1"
    try:
        got = radiance_rows(torch, d, sc, rays, ids, 4)
    finally:
        del os.environ["GI_RAD_MAX_GRID"]
    ne = ~U.bits_equal(got, ref)
    assert not ne.any(), (int(ne.any(1).sum()), np.flatnonzero(ne.any(1))[:8])
    assert (got != 0).any(1).sum() >= 300 and U.bits_equal(got[[2, 11, 23, 40, 63]], np.zeros(1)).all()
    # a batch large enough that waves of a full grid take several runs too, against its own batches of 4096
    big_r, big_i = np.tile(rays, (400, 1)), np.tile(ids, 400)
    whole = radiance_rows(torch, d, sc, big_r, big_i, 4)
    assert U.bits_equal(whole.reshape(400, n, 3), ref[None]).all()


def test_zero_records_and_null_ids(torch_cuda):
    """n == 0 returns GI_OK on both forms and writes nothing; NULL ids mean stream = i, sample = 0."""
    torch = torch_cuda
    d, sc, _, _, _, _ = setup("cornell")
    b = Dev(torch, 4)
    d.radiance_device(0, b.rays.data_ptr(), b.rows.data_ptr(), sc.light, 4, d_ids=b.ids.data_ptr())
    assert (b.get()[2] == GUARD).all()
    assert d.radiance(np.zeros((0, 8)), sc.light, 4).shape == (0, 3)
    rays, _ = _records(100)
    ids = np.zeros(100, gi.PATH_ID_DTYPE)
    ids["stream"] = np.arange(100)
    assert U.bits_equal(d.radiance(rays, sc.light, 4, seed=SEED), d.radiance(rays, sc.light, 4, ids=ids, seed=SEED)).all()


# ---- 4. state ------------------------------------------------------------------------------------------------
def test_a_call_between_passes_ends_no_frame(torch_cuda):
    """radiance_device between two progressive passes and between two adaptive passes: the final frames are those
    without the call, bit for bit, and frame_samples_info is what it was before the call."""
    torch = torch_cuda
    d, sc, cam, w, h, win = setup("cornell")
    rays, ids = _records(1000)
    kw = dict(mode=gi.MODE_X, spp=4, depth=4, seed=SEED)

    def progressive(call):
        d.render(cam, sc.light, w, h, samples=(0, 2), **kw)
        info = d.frame_samples_info()
        if call:
            rows = radiance_rows(torch, d, sc, rays, ids, 4)
            assert (rows != 0).any() and d.frame_samples_info() == info
        return d.render(cam, sc.light, w, h, samples=(2, 4), **kw)

    a, b = progressive(False), progressive(True)
    assert U.bits_equal(a[0], b[0]).all() and (a[1] == b[1]).all()
    assert U.bits_equal(a[0], d.render(cam, sc.light, w, h, **kw)[0]).all()
    info = d.frame_samples_info()
    radiance_rows(torch, d, sc, rays, ids, 4)
    assert d.frame_samples_info() == info == dict(w=w, h=h, n=4, spp=4)

    def adaptive(call):
        akw = dict(spp=8, depth=4, seed=SEED, tol=0.01, min_samples=2, want=("rgb", "n", "mean", "var"))
        d.render_adaptive(cam, sc.light, w, h, (0, 4), **akw)
        info = d.adaptive_info()
        if call:
            radiance_rows(torch, d, sc, rays, ids, 4)
            assert d.adaptive_info() == info
        return d.render_adaptive(cam, sc.light, w, h, (4, 8), **akw)

    a, b = adaptive(False), adaptive(True)
    for k in a:
        assert U.bits_equal(a[k].astype(np.float64), b[k].astype(np.float64)).all(), k
    assert (a["n"] < 8).any() and (a["n"] == 8).any()


# ---- 5. lens -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("win,samples", [(A.ODD_WINDOW, (0, 3)), ((17, 11, 18, 12), (2, 5)), ((0, 0, 37, 21), (1, 2))])
def test_lens_rays_and_their_radiance(torch_cuda, win, samples):
    """aperture > 0 on an odd window, a 1 x 1 window and with sample_begin > 0: the device's rays are the numpy
    restatement's bit for bit, their rows are radiance of the numpy rays, the host forms equal the device forms, and
    the resolved frame differs from the pinhole frame."""
    torch = torch_cuda
    d, sc, cam, w, h, _ = setup("cornell_sphere")
    ap, focus, depth = 0.4, 12.0, 4
    s0, s1 = samples
    rays, ids, rows, rgb, rgb8 = pipeline(torch, d, cam, sc, w, h, win, s0, s1, depth, True, aperture=ap, focus=focus)
    e_rays, e_ids = RR.sample_rays_np(sc, w, h, win, SEED, s0, s1, True, ap, focus)
    assert_records(rays, ids, e_rays, e_ids)
    assert not U.bits_equal(rays[:, 0:3], np.array(sc.cam_pos)).all(1).any()
    assert U.bits_equal(rows.reshape(-1, 3), radiance_rows(torch, d, sc, e_rays, e_ids, depth)).all()
    h_rays, h_ids = gi.sample_rays(cam, w, h, samples=samples, window=win, seed=SEED, jitter=True, aperture=ap, focus=focus)
    assert_records(h_rays, h_ids, e_rays, e_ids)
    assert U.bits_equal(d.radiance(h_rays, sc.light, depth, ids=h_ids, seed=SEED), rows.reshape(-1, 3)).all()
    host = gi.resolve_samples(rows)
    assert U.bits_equal(host["rgb"], rgb).all() and (host["rgb8"] == rgb8).all()
    assert U.bits_equal(rgb, RR.resolve_np(rows)).all() and (rgb8 == RR.quantize_np(rgb)).all()
    pin = pipeline(torch, d, cam, sc, w, h, win, s0, s1, depth, True)
    if len(rgb) > 1:
        assert not U.bits_equal(pin[3], rgb).all() and (rgb > 0).any()
    assert not U.bits_equal(pin[0][:, 3:6], rays[:, 3:6]).all()
    # only one output of each call
    b = Dev(torch, len(rays), len(rgb))
    gi.sample_rays_device(cam, w, h, b.rays.data_ptr(), 0, samples=samples, window=win, seed=SEED, aperture=ap, focus=focus)
    b.rows[:rows.size] = torch.from_numpy(rows.reshape(-1)).cuda()
    gi.resolve_samples_device(len(rgb), s1 - s0, b.rows.data_ptr(), 0, b.rgb8.data_ptr())
    r2, i2, _ = b.get()
    assert U.bits_equal(r2, e_rays).all() and (i2.view(np.int64) == -7).all()
    assert (b.pixels()[0] == GUARD).all() and (b.pixels()[1] == rgb8).all()
