"""GPU checks of the shading helper x_texel (gi_dev.h; DESIGN.md §5 "The checker texel"): an fp32 filter decides
the checker's colour of a triangle's hit point where it is sure, the exact texture-coordinate code decides the
rest, and a wave runs the exact code only if some lane asks for it.  Results must not change:
  * the known-answer hook (gi_kat_x_texel) in helper mode against its exact mode, bit for bit, on the point
    classes of tests/cpp/tex_class_check.cpp, in waves with no, one and only unsure lanes;
  * frames through k_seg itself against the CPU oracle, with the ring of primary rays and with GI_SEG_RING=0
    (read once per process: a child process), and against render_aov's albedo plane, which k_aov computes
    with the exact code."""
import copy
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_util as U

pytestmark = pytest.mark.gpu

gi = U.pkg()
S = U.scenes()

SEED = 2019
NS = (1, 63, 64, 65, 200)
RED = (2, 3)   # the Cornell box's red wall (scenes.py cornell_scene: entities in push order)


# ---- points ---------------------------------------------------------------------------------------------------
def _frame(e):
    """p1, p2 - p1, p3 - p1, unit_v, unit_h of an ImpTriangle (gi_build.cpp's constants, in numpy)."""
    p1, p2, p3 = (np.array(e.args[3 * k:3 * k + 3]) for k in range(3))
    p21, p31, p32 = p2 - p1, p3 - p1, p3 - p2
    return p1, p21, p31, np.linalg.norm(0.5 * (p21 + p31)) / 160.0, np.linalg.norm(0.5 * (-p32 - p31)) / 160.0


def _basis(p21, p31):
    a1 = p21 / np.linalg.norm(p21)
    n = np.cross(p21, p31)
    n /= np.linalg.norm(n)
    return a1, np.cross(n, a1), n


def uniform_points(e, n, rng):
    p1, p21, p31, _, _ = _frame(e)
    s, t = rng.random(n), rng.random(n)
    f = s + t > 1.0
    s[f], t[f] = 1.0 - s[f], 1.0 - t[f]
    return p1 + s[:, None] * p21 + t[:, None] * p31


def boundary_points(e, n, rng, ulps=True):
    """Points whose exact u (even rows; odd rows: v) is 32 k + {0, 17}, the distance from p1 scaled by
    1 -/+ j 2^-52, j = 0 .. 4 (ulps=False: j = 0)."""
    p1, p21, p31, uv, uh = _frame(e)
    a1, a2, _ = _basis(p21, p31)
    size = max(np.linalg.norm(p21), np.linalg.norm(p31))
    for_v = np.arange(n) % 2 == 1
    unit = np.where(for_v, uh, uv)
    cells = np.floor(rng.random(n) * (size / unit) / 32.0)
    B = 32.0 * cells + np.where(rng.random(n) < 0.5, 17.0, 0.0)
    B[B == 0.0] = 17.0   # (coordinate 0 is P == p1: its own class below)
    th = (0.05 + 0.9 * rng.random(n)) * np.pi
    j = rng.integers(-4, 5, n) if ulps else np.zeros(n)
    ln = np.where(for_v, B * unit, B * unit / np.sin(th)) * (1.0 + j * 2.0 ** -52)
    return p1 + (ln * np.cos(th))[:, None] * a1 + (ln * np.sin(th))[:, None] * a2


def edge_points(e, n, rng):
    p1, p21, p31, _, _ = _frame(e)
    _, a2, nn = _basis(p21, p31)
    size = max(np.linalg.norm(p21), np.linalg.norm(p31))
    t = 5.0 * rng.random(n) - 2.0
    off = rng.choice([0.0, 1e-17, 1e-16, 1e-15, 1e-13, 1e-11, 1e-8, 1e-6], n) * size * rng.choice([-1.0, 1.0], n)
    return p1 + t[:, None] * p21 + off[:, None] * np.where((rng.random(n) < 0.5)[:, None], a2, nn)


def far_points(e, n, rng):
    p1 = _frame(e)[0]
    return p1 + rng.choice([1e1, 1e3, 1e5, 1e6, 1e8, 1e30, 1e300], n)[:, None] * (2.0 * rng.random((n, 3)) - 1.0)


def class_points(e, n, rng):
    """n points of every class on one triangle, and P == p1."""
    return np.concatenate([uniform_points(e, n, rng), boundary_points(e, n, rng), edge_points(e, n, rng),
                           far_points(e, n, rng), _frame(e)[0][None, :]])


# ---- the hook -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cornell():
    sc = S.cornell_scene()
    return sc, gi.DeviceScene.from_scene(sc)


@pytest.fixture(scope="module")
def pools(cornell):
    """Red-wall points the device's filter decides (uniform points, how == 1) and points it leaves to the exact
    code (points on pattern boundaries, how == 2), 256 of each: a point's `how` depends on the point alone."""
    sc, d = cornell
    rng = np.random.default_rng(SEED)
    ents = np.repeat(RED, 2048)
    uni = np.concatenate([uniform_points(sc.entities[k], 2048, rng) for k in RED])
    bnd = np.concatenate([boundary_points(sc.entities[k], 2048, rng, ulps=False) for k in RED])
    how_u, how_b = d.kat_x_texel(ents, uni)[1], d.kat_x_texel(ents, bnd)[1]
    print("uniform: decided %d of %d; boundary: left to the exact code %d of %d" %
          ((how_u == 1).sum(), len(how_u), (how_b == 2).sum(), len(how_b)))
    assert (how_u == 1).sum() >= 256 and (how_b == 2).sum() >= 256
    sure = (ents[how_u == 1][:256], uni[how_u == 1][:256])
    unsure = (ents[how_b == 2][:256], bnd[how_b == 2][:256])
    return sure, unsure


def _both(d, ents, pts):
    tex, how = d.kat_x_texel(ents, pts)
    ref, how_ref = d.kat_x_texel(ents, pts, exact=True)
    assert (how_ref == 2).all()
    assert U.bits_equal(tex, ref).all(), np.flatnonzero(~U.bits_equal(tex, ref).all(1))[:8]
    return tex, how


@pytest.mark.parametrize("n", NS)
def test_hook_wave_shapes(cornell, pools, n):
    """n = 1, 63, 64, 65, 200 records (the lanes past n run the helper without a point): waves in which no
    lane is unsure (the wave skips the exact code), exactly one is (the exact code runs for that lane alone),
    all are; the texels equal the exact mode's bit for bit and every lane reports what decided it."""
    _, d = cornell
    (se, sp), (ue, up) = pools
    _, how = _both(d, se[:n], sp[:n])
    assert (how == 1).all()
    for at in sorted({0, n // 2, n - 1}):
        ents, pts = se[:n].copy(), sp[:n].copy()
        ents[at], pts[at] = ue[at], up[at]
        _, how = _both(d, ents, pts)
        want = np.ones(n, np.int32)
        want[at] = 2
        assert (how == want).all()
    _, how = _both(d, ue[:n], up[:n])
    assert (how == 2).all()


@pytest.mark.parametrize("n", NS)
def test_hook_white_entities_never_ask(cornell, n):
    """Boundary points (-/+ 0..4 ulp) on white entities -- the back wall, the floor, a block face: the colour
    decides, no lane asks for the exact code, and the texel is the exact mode's (1, 1, 1)."""
    sc, d = cornell
    rng = np.random.default_rng(SEED + n)
    ents = np.resize(np.array([0, 1, 6, 7, 12, 25]), n)
    pts = np.concatenate([boundary_points(sc.entities[k], 1, rng) for k in ents])
    tex, how = _both(d, ents, pts)
    assert (how == 0).all() and (tex == 1.0).all()


def test_hook_cornell_point_classes_and_decided_share(cornell):
    """Every point class on the red and green walls (the filter works) and on two white triangles; on uniform
    red-wall points the filter decides at least 99%."""
    sc, d = cornell
    rng = np.random.default_rng(SEED)
    for k in (2, 3, 4, 5, 0, 20):
        pts = class_points(sc.entities[k], 1000, rng)
        _, how = _both(d, np.full(len(pts), k), pts)
        print("entity", k, "how 0/1/2:", [(how == v).sum() for v in (0, 1, 2)])
        assert ((how == 0).all() if k in (0, 20) else (how != 0).all())
    ents = np.repeat(RED, 10000)
    pts = np.concatenate([uniform_points(sc.entities[k], 10000, rng) for k in RED])
    _, how = _both(d, ents, pts)
    share = (how == 1).mean()
    print("decided share on uniform red-wall points: %.5f" % share)
    assert share >= 0.99


def mixed_tri_scene():
    """The kinds of the TRI kernels in one scene: an ExpCube, an ExpQuad, a red and a white ImpTriangle."""
    s = S.Scene(name="mixed_tri")
    s.exp_cube((0.0, 0.0, 0.0), 2, 2, 2, (1, 0, 0))
    s.exp_quad((0.0, 3.0, 0.0), 2, 3, 90.0 * np.pi / 180.0, (1, 2, 3))
    s.imp_triangle((0.0, 3.0, 2.0), (3.0, 3.0, -4.0), (3.0, -3.0, -4.0), (1, 0, 0))
    s.imp_triangle((4.0, -3.0, 2.0), (4.0, 3.0, 2.0), (4.0, 0.0, 4.0), (1, 1, 1))
    return s


def _kinds_check(sc, tri_kernels):
    """Points around every entity of the scene, and waves that mix the entities: equal to the exact mode; the
    other kinds always ask for the exact code, the triangles are filtered in the TRI kernels only."""
    d = gi.DeviceScene.from_scene(sc)
    assert d.kat_x_variant()["TRI"] == tri_kernels
    rng = np.random.default_rng(SEED)
    tri = [k for k, e in enumerate(sc.entities) if e.kind == S.IMP_TRIANGLE]
    assert tri and len(tri) < len(sc.entities)
    for k, e in enumerate(sc.entities):
        if k in tri:
            pts = class_points(e, 1000, rng)
        else:
            pts = np.array(e.args[:3]) + np.concatenate([6.0 * rng.random((300, 3)) - 3.0, np.zeros((1, 3))])
        _, how = _both(d, np.full(len(pts), k), pts)
        print(sc.name, "entity", k, "how 0/1/2:", [int((how == v).sum()) for v in (0, 1, 2)])
        if k not in tri or not tri_kernels:
            assert (how == 2).all(), k
        elif e.material.color == (1.0, 1.0, 1.0):
            assert (how == 0).all(), k
        else:
            assert (how == 1).sum() > 500 and (how == 2).sum() > 0 and (how != 0).all(), k
    for n in NS:   # waves that mix the kinds
        ents = rng.integers(0, len(sc.entities), n)
        _, how = _both(d, ents, uniform_points(sc.entities[tri[0]], n, rng))
        assert (how[~np.isin(ents, tri)] == 2).all()


def test_hook_other_kinds_in_the_tri_kernels():
    """ExpCube and ExpQuad beside triangles in a scene of the TRI kernels: they take the exact code, in waves
    of their own and mixed with filtered and white triangles."""
    _kinds_check(mixed_tri_scene(), True)


def test_hook_zoo_runs_the_exact_code():
    """The zoo scene (every entity kind; the non-TRI kernels, which keep the exact code for every lane, its
    ImpTriangle included): the helper mode is the exact mode."""
    _kinds_check(S.zoo_scene(), False)


def test_hook_refuses_bad_arguments(cornell):
    sc, d = cornell
    for ent in (-1, len(sc.entities), 0.5, float("nan")):
        with pytest.raises(gi.GIError):
            d.kat_x_texel([ent], np.zeros((1, 3)))
    tex, how = d.kat_x_texel([], np.zeros((0, 3)))
    assert tex.shape == (0, 3) and how.shape == (0,)


# ---- frames through k_seg ---------------------------------------------------------------------------------------
W, H = 64, 48


def checker_wall():
    """Two triangles with a red material, slanted across the view, the pattern's cells a few pixels wide:
    many boundaries in the frame."""
    s = S.Scene(name="checker_wall", light=(-4.0, 3.0, 6.0))
    s.imp_triangle((6.0, -9.0, -7.0), (3.0, 9.0, -7.0), (3.0, 9.0, 7.0), (1.0, 0.0, 0.0))
    s.imp_triangle((6.0, -9.0, -7.0), (3.0, 9.0, 7.0), (6.0, -9.0, 7.0), (1.0, 0.0, 0.0))
    s.focal = 0.009   # (the wall fills most of the 64 x 48 view)
    return s


def frame_scene(name, depth):
    """depth 1: every material's shader (1, 0, 0) (the frame is then min(texel, 1)); depth 3: the scene's own."""
    sc = S.cornell_scene() if name == "cornell" else checker_wall()
    if name == "cornell":
        sc.focal = 0.009
    if depth == 1:
        sc = copy.deepcopy(sc)
        for e in sc.entities:
            e.material = S.Material(e.material.color, (1.0, 0.0, 0.0))
    return sc


FRAME_CASES = [(name, spp, depth) for name in ("cornell", "checker_wall") for spp in (1, 4) for depth in (1, 3)]


def _key(case):
    return "%s_%d_%d" % case


def render_frames(out):
    """(Also the child process's entry point.)"""
    res = {}
    for case in FRAME_CASES:
        name, spp, depth = case
        sc = frame_scene(name, depth)
        d = gi.DeviceScene.from_scene(sc)
        cam = gi.Camera(sc.cam_pos, sc.cam_look, sc.focal)
        rgb, rgb8 = d.render(cam, sc.light, W, H, mode=gi.MODE_X, spp=spp, depth=depth, seed=SEED)
        res[_key(case) + "/rgb"], res[_key(case) + "/rgb8"] = rgb.reshape(-1, 3), rgb8.reshape(-1, 3)
        res[_key(case) + "/form"] = np.array([int(d.x_form(spp=spp, depth=depth) == "k_seg"), int(d.seg_ring(spp=spp, depth=depth))])
        if spp == 1 and depth == 1:
            res[_key(case) + "/albedo"] = d.render_aov(cam, W, H, want=("albedo",))["albedo"].reshape(-1, 3)
    if out:
        np.savez(out, **res)
    return res


@pytest.fixture(scope="module")
def frames(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("tex_class") / "direct.npz")
    code = ("import sys; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_tex_class as T; "
            "T.render_frames(%r)") % (U.ROOT, os.path.join(U.ROOT, "tests"), out)
    p = subprocess.Popen([sys.executable, "-c", code], env=dict(os.environ, GI_SEG_RING="0"))
    try:
        ring = render_frames(None)
        rc = p.wait(timeout=300)
    finally:
        if p.poll() is None:
            p.kill()
        p.wait()
    assert rc == 0
    return ring, dict(np.load(out).items())


@pytest.fixture(scope="module")
def oracle_frames():
    return {case: U.oracle_render(frame_scene(case[0], case[2]).to_scn(), W, H, mode=1, spp=case[1], depth=case[2], seed=SEED)
            for case in FRAME_CASES}


@pytest.mark.parametrize("case", FRAME_CASES, ids=_key)
def test_frames_equal_the_oracle(frames, oracle_frames, case):
    """64 x 48, spp 1 and 4, depth 1 and 3, k_seg with the ring and with GI_SEG_RING=0: fp64 radiance bit for
    bit and the same RGB888 as the CPU oracle.  The checker wall's frame shows many pattern boundaries."""
    o = oracle_frames[case]
    for res, ring in zip(frames, (1, 0)):
        assert res[_key(case) + "/form"].tolist() == [1, ring]
        same = U.bits_equal(res[_key(case) + "/rgb"], o["rgb"]).all(1)
        assert same.all(), f"{case} ring {ring}: {int((~same).sum())} of {same.size} pixels differ"
        assert (res[_key(case) + "/rgb8"] == o["q"]).all()
    if case[0] == "checker_wall" and case[1:] == (1, 1):
        img = o["rgb"].reshape(H, W, 3)
        changes = int((img[:, 1:] != img[:, :-1]).any(2).sum() + (img[1:] != img[:-1]).any(2).sum())
        print("checker wall: colour changes between neighbouring pixels:", changes)
        assert changes >= 300


@pytest.mark.parametrize("name", ["cornell", "checker_wall"])
def test_depth1_frame_is_the_albedo_plane(frames, name):
    """Shader (1, 0, 0), depth 1, one sample (the pixel's own ray): k_seg's frame -- the helper -- equals
    render_aov's albedo plane clamped to 1 -- k_aov, the exact code -- bit for bit."""
    for res in frames:
        k = _key((name, 1, 1))
        alb = res[k + "/albedo"]
        assert U.bits_equal(np.minimum(alb, 1.0), res[k + "/rgb"]).all()
        assert len(np.unique(alb, axis=0)) >= 3   # background, white, a colour
