"""GPU checks of the fan-pair decision in the flat leaf query's phase B (gi_wf.hip wf_flat, csrc/gi_fan_pair.h):
where every leaf of a scene's table is the two halves of one planar convex quad, a lane runs one exact test
per leaf, chosen by the first record's first step, and both only where that leaves it undecided.  Answers must
not change: ray by ray against the oracle's brute force, with the decision (the default) and with GI_X_FAN=0
(both tests always; read once per process: one child process), and a frame both ways against the oracle."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_util as U
import x_rays as R
from x_scenes import STANDIN_SKIP_COS, tri_scene

pytestmark = pytest.mark.gpu

gi = U.pkg()
S = U.scenes()
FRAME = (48, 48, 4, 8, 2019)   # w, h, spp, depth, seed


def _quads(bend):
    """Four planar quads off the axes, apart from each other: two rectangles turned about one axis and two
    parallelograms tilted in all three.  (Their diagonal a-c spans the quad's bounding box, so the two
    triangles' boxes are the quad's and the builder's SAH keeps each quad as one leaf of two records.)
    bend: the last vertex of each lifted off its plane by that many units."""
    frames = (((np.cos(0.7), np.sin(0.7), 0.0), (0.0, 0.0, 1.0)), ((0.0, np.cos(0.4), np.sin(0.4)), (1.0, 0.0, 0.0)),
              ((1.0, 2.0, 0.5), (0.5, 1.0, 3.0)), ((2.0, 0.3, 1.0), (0.2, 1.5, 0.1)))
    tris = []
    for i, c in enumerate(((3.0, -2.5, -2.5), (4.0, 2.5, -2.0), (5.0, -2.0, 2.5), (6.0, 2.5, 2.5))):
        u, v = R.unit(np.array(frames[i][0])), R.unit(np.array(frames[i][1]))
        n = R.unit(np.cross(u, v))
        c = np.array(c)
        q = [c - 1.2 * u - 0.9 * v, c + 1.2 * u - 0.9 * v, c + 1.2 * u + 0.9 * v, c - 1.2 * u + 0.9 * v + bend * n]
        col = (0.9 - 0.2 * i, 0.3 + 0.2 * i, 0.5)
        tris.append(((tuple(q[0]), tuple(q[1]), tuple(q[2])), col))
        tris.append(((tuple(q[0]), tuple(q[2]), tuple(q[3])), col))
    return tris


def rotated_quads():
    return tri_scene(_quads(0.0), "rotated_quads")


def bent_quads():
    """The same quads bent by 1e-6 along the diagonal: two-record leaves the builder must refuse."""
    return tri_scene(_quads(1e-6), "bent_quads")


# scene -> (builder, leaves, fan-pair leaves)
SCENES = {"cornell": (lambda: S.named_scene("cornell"), 17, 17), "rotated_quads": (rotated_quads, 4, 4),
          "bent_quads": (bent_quads, 4, 0)}


def _ulps(x, n):
    for _ in range(abs(n)):
        x = np.nextafter(x, np.inf if n > 0 else -np.inf)
    return x


def extra_rays(sc, seed):
    """Rays at the edges of the decision, per quad (a, b, c, d) of the scene (consecutive triangle pairs):
    aimed at points of the diagonal a-c and 0, +-1, +-2, +-32 ulp off them in each coordinate; through the
    four corners; grazing the plane (|d . n| = 2^-j across the det margin) and in it.  Records (o, d, light,
    d2): the next ray leaves the hit point along the diagonal, in the plane."""
    g = R.Geo(sc)
    rng = np.random.default_rng(seed)
    tri = g.ptri[~np.isnan(g.ptri).any((1, 2))]
    recs = []
    for k in range(0, len(tri) - 1, 2):
        a, b, c, d = tri[k][0], tri[k][1], tri[k][2], tri[k + 1][2]
        n = R.unit(np.cross(b - a, c - a))
        diag = R.unit(c - a)

        def origin():
            o = g.lo + rng.random(3) * (g.hi - g.lo)
            return o if abs(np.dot(o - a, n)) > 1e-3 else o + 0.5 * n

        def add(o, to):
            recs.append(np.concatenate([o, R.unit(to - o), np.asarray(sc.light, np.float64), diag]))

        for s in (0.0, 0.25, 0.5, 0.75, 1.0, rng.random()):
            p, o = a + s * (c - a), origin()
            for off in (0, 1, -1, 2, -2, 32, -32):
                for ax in range(3):
                    t = p.copy()
                    t[ax] = _ulps(t[ax], off)
                    add(o, t)
        for p in (a, b, c, d):
            add(origin(), p)
        for j in range(8, 64, 4):
            for sg in (1.0, -1.0):
                w = R.unit((b - a) * rng.normal() + (d - a) * rng.normal())
                dr = w + sg * 2.0 ** -j * n
                tgt = a + 0.5 * rng.random() * (b - a) + 0.5 * rng.random() * (d - a)
                add(tgt - 3.0 * dr, tgt)
        add(a - 0.5 * (c - a), c)   # in the plane, along the diagonal
    return np.array(recs)


_sets = {}


def query_set(name):
    """(scene, records, brute-force reference): tests/x_rays.py's set of the scene plus extra_rays, built
    once and left unchanged."""
    if name not in _sets:
        sc = SCENES[name][0]()
        scn = sc.to_scn()
        U.oracle_accel(0)
        try:
            rs = R.ray_set(sc, 2048 + 37, STANDIN_SKIP_COS, 2019, lambda recs: U.oracle_x_query(scn, recs))
            recs = np.concatenate([rs["recs"][R.near(rs)], extra_rays(sc, 7)])
            ref = U.oracle_x_query(scn, recs)
        finally:
            U.oracle_accel(-1)
        assert len(recs) <= 1 << 16 and len(recs) % 64 != 0
        for a in [recs] + list(ref.values()):
            a.setflags(write=False)
        _sets[name] = (sc, recs, ref)
    return _sets[name]


def run_all():
    """Every scene's query answers and the Cornell frame with its stats, in this process."""
    import torch
    res = {}
    for name in SCENES:
        sc, recs, _ = query_set(name)
        d = gi.DeviceScene.from_scene(sc)
        info, var = d.info(), d.kat_x_variant(0)
        assert (info["x_flat_leaves"], info["x_fan_leaves"]) == SCENES[name][1:], (name, info)
        assert var["TRI"] and var["FLAT"] and var["LDS"], (name, var)
        out = d.kat_x_query(recs, sc.cam_pos, 0)
        for k in ("prim1", "t1", "occl", "prim2", "t2"):
            res[f"{name}/{k}"] = out[k]
        if name == "cornell":
            w, h, spp, depth, seed = FRAME
            st = torch.zeros(gi.STATS_N, dtype=torch.int64, device="cuda")
            buf = torch.zeros(w * h * 3, dtype=torch.float64, device="cuda")
            assert d.x_form(spp=spp, depth=depth) == "k_seg"
            d.render_device(gi.Camera(sc.cam_pos, sc.cam_look, sc.focal), sc.light, w, h, buf.data_ptr(), mode=gi.MODE_X,
                            spp=spp, depth=depth, seed=seed, stats_ptr=st.data_ptr())
            torch.cuda.synchronize()
            res["frame"], res["stats"] = buf.cpu().numpy().reshape(-1, 3), st.cpu().numpy()
    return res


@pytest.fixture(scope="module")
def both_ways(tmp_path_factory):
    """run_all() here (the decision, unless the suite itself runs under GI_X_FAN=0) and in a child process
    with GI_X_FAN=0."""
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    out = tmp_path_factory.mktemp("fan") / "two_tests.npz"
    code = ("import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r); import test_gpu_fan_pair as T; "
            "np.savez(%r, **T.run_all())") % (U.ROOT, os.path.join(U.ROOT, "tests"), str(out))
    child = subprocess.Popen([sys.executable, "-c", code], env=dict(os.environ, GI_X_FAN="0"))
    try:
        here = run_all()
        assert child.wait(timeout=300) == 0
    finally:
        if child.poll() is None:
            child.kill()
            child.wait()
    return here, {k: v for k, v in np.load(out).items()}


@pytest.mark.parametrize("name", sorted(SCENES))
def test_fan_pair_queries_equal_brute_force_both_ways(both_ways, name):
    """prim1, t1, occl, prim2, t2 of every ray equal the oracle's brute force bit for bit, with the decision
    and with GI_X_FAN=0: on the Cornell box (17 of 17 fan-pair leaves), on four planar quads off the axes
    (4 of 4) and on the same quads bent by 1e-6, which the builder refuses (0 of 4: both tests always)."""
    _, recs, ref = query_set(name)
    for way, res in zip(("decision", "GI_X_FAN=0"), both_ways):
        for k in ("prim1", "t1", "occl", "prim2", "t2"):
            a, b = res[f"{name}/{k}"], ref[k]
            ne = ~U.bits_equal(a, b) if a.dtype == np.float64 else a != b
            assert not ne.any(), (f"{name} {way}: {int(ne.sum())} of {len(a)} rays differ in {k}; first: ray "
                                  f"{int(np.flatnonzero(ne)[0])} device {a[ne][0]!r} reference {b[ne][0]!r} record "
                                  f"{recs[int(np.flatnonzero(ne)[0])].tolist()}")
    assert (ref["prim1"] >= 0).mean() > 0.3 and (ref["prim2"] >= 0).any()
    if name == "cornell":   # (the separate quads rarely shadow each other)
        assert (ref["occl"] != 0).any()


def test_fan_pair_frame_identical_both_ways_and_to_oracle(both_ways):
    """A 48 x 48, 4 spp, depth 8 Cornell frame through k_seg: fp64 radiance byte-identical with the decision
    and with GI_X_FAN=0 and equal to the oracle's; rays traced and records decided (GI_STAT_RAYS,
    GI_STAT_PRIMS) equal both ways -- a leaf counts two records however many tests ran."""
    here, off = both_ways
    w, h, spp, depth, seed = FRAME
    o = U.oracle_render(S.named_scene("cornell").to_scn(), w, h, mode=1, spp=spp, depth=depth, seed=seed)
    assert here["frame"].tobytes() == off["frame"].tobytes()
    assert U.bits_equal(here["frame"], o["rgb"]).all() and (o["rgb"] > 0).any()
    for k in (gi.STAT_RAYS, gi.STAT_PRIMS):
        assert int(here["stats"][k]) == int(off["stats"][k]) > 0
    assert int(here["stats"][gi.STAT_RAYS]) == int(o["ncand"].sum())
