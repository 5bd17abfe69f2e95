"""GPU: the flat leaf query with Phase A's plane distances taken by two packed fmas per axis (gi_wf.hip
flat_pk_inner / flat_pk_outer on the device's leaf record, XFlatLeafDev) -- ray by ray against the oracle's
brute force, and one Cornell frame.

The rays are built for what the two-stage form turns on, the sign of each reciprocal direction component: from
the camera and from the scene's centre into every octant, along each axis in both directions, with one
component zero (+0 and -0: the clamped reciprocals of either sign), and from the hit points of all of these
(the record's second direction cycles through the same classes).  Leaf tables of 1, 5 and 32 leaves and the
Cornell box's 17; calls of 1, 64 and 65 rays.  No tolerance: primitives and shadow answers equal, t bit for
bit; the frame's radiance bit for bit."""
import itertools

import numpy as np
import pytest

import oracle_util as U
import x_rays as R
from x_scenes import soup, with_env

pytestmark = pytest.mark.gpu

gi = U.pkg()
S = U.scenes()

SCENES = ("cornell", "1", "5", "32")
COUNTS = (1, 64, 65)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    return torch


def class_dirs(rng):
    """(directions, class names): every octant three times with random magnitudes, the six axis directions, and
    every (zero axis, zero sign, signs of the other two) combination."""
    d, c = [], []
    for sx, sy, sz in itertools.product((1.0, -1.0), repeat=3):
        for _ in range(3):
            d.append(np.array([sx, sy, sz]) * (0.05 + rng.random(3)))
            c.append("octant")
    for k in range(3):
        for s in (1.0, -1.0):
            v = np.zeros(3)
            v[k] = s
            v[(k + 1) % 3] = 0.0 if s > 0 else -0.0
            v[(k + 2) % 3] = -0.0 if s > 0 else 0.0
            d.append(v)
            c.append("axis")
    for k in range(3):
        for z, sa, sb in itertools.product((0.0, -0.0), (1.0, -1.0), (1.0, -1.0)):
            v = np.array([sa, sb, 1.0]) * (0.05 + rng.random(3))
            v = np.roll(np.array([v[0], v[1], z]), k + 1)
            d.append(v)
            c.append("zero1")
    d = np.array(d)
    n = np.sqrt((d * d).sum(1, keepdims=True))
    return d / n, c   # (a zero component keeps its sign)


def build_rays(sc):
    """Records (n, 12): o, d, light, d2.  Origins: the camera, the centre of the scene's bounds and a point
    inside its bounds off every vertex plane, then points in front of the geometry; d and d2 over class_dirs
    (d2 shifted, so each class leaves hit points of every other)."""
    rng = np.random.default_rng(14)
    g = R.Geo(sc)
    lo, hi, centre = g.lo, g.hi, g.centre
    origins = [np.asarray(sc.cam_pos, np.float64), centre, lo + (hi - lo) * np.array([0.31, 0.57, 0.43])]
    dirs, cls = class_dirs(rng)
    recs, names = [], []
    for oi, o in enumerate(origins):
        for j in range(len(dirs)):
            d = dirs[j]
            if oi == 0 and cls[j] == "octant":   # from the camera: the octant's signs, aimed into the scene where they allow
                aim = lo + rng.random(3) * (hi - lo) - o
                d = np.where(np.sign(aim) == np.sign(d), aim, d * np.abs(aim).max())
                d = d / np.sqrt((d * d).sum())
            recs.append(np.concatenate([o, d, np.asarray(sc.light, np.float64), dirs[(j * 7 + 5 * oi + 3) % len(dirs)]]))
            names.append(cls[j])
    # every direction again, three times, from 1 to 3 units in front of a point of the geometry: rays of each class
    # that hit, and so hit points that rays of each class leave
    for rep in range(3):
        for j in range(len(dirs)):
            if len(g.tris):
                t = g.tris[rng.integers(0, len(g.tris))]
                b = rng.dirichlet((1.0, 1.0, 1.0))
                p = (t * b[:, None]).sum(0)
            else:
                p = lo + rng.random(3) * (hi - lo)
            o = p - dirs[j] * (1.0 + 2.0 * rng.random())
            recs.append(np.concatenate([o, dirs[j], np.asarray(sc.light, np.float64), dirs[(j * 11 + 13 * rep + 1) % len(dirs)]]))
            names.append(cls[j])
    return np.ascontiguousarray(np.array(recs)), names


_cases = {}


def query_case(name):
    """(scene, device scene, records, brute-force reference), built once per scene and left unchanged."""
    if name not in _cases:
        sc, env = (S.named_scene("cornell"), {}) if name == "cornell" else soup(int(name))
        d = with_env(env, lambda: gi.DeviceScene.from_scene(sc))
        recs, names = build_rays(sc)
        U.oracle_accel(0)   # brute force
        try:
            ref = U.oracle_x_query(sc.to_scn(), recs)
        finally:
            U.oracle_accel(-1)
        for a in [recs] + list(ref.values()):
            a.setflags(write=False)
        _cases[name] = (sc, d, recs, ref, names)
    return _cases[name]


@pytest.mark.parametrize("name", SCENES)
def test_packed_phase_a_query_equals_brute_force(torch_cuda, name):
    """gi_kat_x_query in the flat variant on the Cornell box and soups of 1, 5 and 32 single-triangle leaves:
    the whole set in one call and windows of 1, 64 and 65 rays from different parts of it.  prim1, occl and
    prim2 equal brute force; t1 and t2 are bit-equal."""
    sc, d, recs, ref, names = query_case(name)
    var = d.kat_x_variant(0)
    assert var["FLAT"] and var["LDS"], var
    assert {"octant", "axis", "zero1"} <= set(names)
    n_all = len(recs)
    assert n_all >= 6 * (24 + 6 + 24)
    calls = [(0, n_all)] + [((j * 37 + 11) % (n_all - n + 1), n) for j, n in enumerate(COUNTS)]
    hits = hits2 = 0
    for lo, n in calls:
        out = d.kat_x_query(recs[lo:lo + n], sc.cam_pos, 0)
        for k in ("prim1", "occl", "prim2"):
            ne = out[k] != ref[k][lo:lo + n]
            assert not ne.any(), f"{name}, {n} rays from {lo}: {k} differs at ray {lo + int(np.flatnonzero(ne)[0])} ({names[lo + int(np.flatnonzero(ne)[0])]})"
        for k in ("t1", "t2"):
            ne = ~U.bits_equal(out[k], ref[k][lo:lo + n])
            assert not ne.any(), f"{name}, {n} rays from {lo}: {k} differs at ray {lo + int(np.flatnonzero(ne)[0])} ({names[lo + int(np.flatnonzero(ne)[0])]})"
        hits += int((out["prim1"] >= 0).sum())
        hits2 += int((out["prim2"] >= 0).sum())
    assert hits > 0, name   # the calls see the scene
    if name == "cornell":   # a closed box: every ray from inside hits, and so does every ray that leaves a hit point
        assert hits2 > 0


def test_packed_phase_a_cornell_frame_bit_exact(torch_cuda):
    """The Cornell box at 64 x 48, 4 spp, depth 8 through k_seg's flat variant: fp64 radiance bit for bit and the
    same RGB888 as the CPU oracle."""
    torch = torch_cuda
    sc = S.named_scene("cornell")
    d = gi.DeviceScene.from_scene(sc)
    w, h, spp, depth, seed = 64, 48, 4, 8, 14
    assert d.x_form(spp=spp, depth=depth) == "k_seg" and d.kat_x_variant(0)["FLAT"]
    buf = torch.zeros(w * h * 3, dtype=torch.float64, device="cuda")
    buf8 = torch.zeros(w * h * 3, dtype=torch.uint8, device="cuda")
    d.render_device(gi.Camera(sc.cam_pos, sc.cam_look, sc.focal), sc.light, w, h, buf.data_ptr(), buf8.data_ptr(), mode=gi.MODE_X,
                    spp=spp, depth=depth, seed=seed)
    torch.cuda.synchronize()
    o = U.oracle_render(sc.to_scn(), w, h, mode=1, spp=spp, depth=depth, seed=seed)
    same = U.bits_equal(buf.cpu().numpy().reshape(-1, 3), o["rgb"]).all(1)
    assert same.all(), f"{int((~same).sum())} of {same.size} pixels differ, first {int(np.flatnonzero(~same)[0])}"
    assert (buf8.cpu().numpy().reshape(-1, 3) == o["q"]).all()
