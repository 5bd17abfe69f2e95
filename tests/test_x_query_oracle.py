"""CPU: the oracle's ray-level Mode X queries (gio_x_query) and the ray sets of tests/x_rays.py.
The brute force and the oracle's own BVH answer every ray alike; hop 1 equals gio_render's primary
hit; and the sets really hold what the device test (tests/test_gpu_x_query.py) relies on -- hits and
misses, ties, both shadow answers and every ray class -- judged on the oracle alone."""
import numpy as np
import pytest

import oracle_util as U
import x_rays as R
from x_scenes import QUERY_SCENES, SHADOW_SCENES, TIE_SCENES, query_set

S = U.scenes()


@pytest.mark.parametrize("name", sorted(QUERY_SCENES))
def test_x_query_bvh_equals_brute_force(name):
    """gio_x_query over the scene's whole ray set with the oracle's BVH forced equals the brute force:
    primitives, shadow answers, and t bit for bit (the tie counts are brute force either way)."""
    sc, _, rs, ref = query_set(name)
    U.oracle_accel(1)
    try:
        bvh = U.oracle_x_query(sc.to_scn(), rs["recs"])
    finally:
        U.oracle_accel(-1)
    for k in ("prim1", "occl", "prim2"):
        assert (bvh[k] == ref[k]).all(), (name, k, int((bvh[k] != ref[k]).sum()))
    for k in ("t1", "t2"):
        assert U.bits_equal(bvh[k], ref[k]).all(), (name, k)
    miss = ref["prim1"] < 0
    assert np.isposinf(ref["t1"][miss]).all() and (ref["occl"][miss] == -1).all() and (ref["prim2"][miss] == -1).all()
    assert np.isposinf(ref["t2"][ref["prim2"] < 0]).all()


def test_x_query_hop1_equals_render_primary_hit():
    """Hop 1 of rays built as a frame's primary rays (the oracle's camera, restated in numpy) hits the
    entity gio_render reports per pixel: Cornell box, 32 x 32, one sample, depth 1."""
    sc = S.named_scene("cornell")
    w = h = 32

    def norm(v):
        return v * (1.0 / np.sqrt(v[..., 0:1] * v[..., 0:1] + v[..., 1:2] * v[..., 1:2] + v[..., 2:3] * v[..., 2:3]))

    pos, up = np.array(sc.cam_pos), np.array([0.0, 0.0, 1.0])
    fwd = norm(np.array(sc.cam_look) - pos)
    left = norm(np.cross(up, fwd))
    top_left = (((pos + sc.focal * fwd) + ((left * float(w)) * 0.5) * 0.0002) + ((up * float(w)) * 0.5) * 0.0002) - pos
    y, x = np.mgrid[0:h, 0:w]
    x, y = x.reshape(-1, 1).astype(float), y.reshape(-1, 1).astype(float)
    d = norm((top_left - (left * x) * 0.0002) - (up * y) * 0.0002)
    recs = np.concatenate([np.tile(pos, (w * h, 1)), d, np.tile(sc.light, (w * h, 1)), d], 1)
    q = U.oracle_x_query(sc.to_scn(), recs)
    o = U.oracle_render(sc.to_scn(), w, h, mode=1, spp=1, depth=1)
    assert (q["prim1"] == o["hit"]).all()   # (the box is ImpTriangles only: primitive i is entity i)
    assert (o["hit"] >= 0).sum() > w * h // 2


@pytest.mark.parametrize("name", sorted(QUERY_SCENES))
def test_ray_sets_cover_their_classes(name):
    """Each scene's set, judged on the oracle: at least 20 % hop-1 hits and 10 % misses; every hop-1
    class present that the scene's geometry allows, every hop-2 and light class present among the
    hits; in the scenes that can shadow, at least 10 % of the hits lit and 10 % shadowed."""
    sc, _, rs, ref = query_set(name)
    n = len(rs["h1"])
    assert n % 64 != 0
    hit = ref["prim1"] >= 0
    if name == "empty":
        assert not hit.any()
        return
    assert hit.mean() >= 0.20 and (~hit).mean() >= 0.10, (name, hit.mean())
    g = R.Geo(sc)
    want = set(R.H1)
    if not len(g.tris):
        want -= {"at_vertex"}
    if not g.shared:
        want -= {"shared_edge"}
    if not g.shared_axis:
        want -= {"edge_axis"}
    if not g.boxes:
        want -= {"in_box"}
    have = {R.H1[c] for c in np.unique(rs["h1"])}
    assert want <= have, (name, sorted(want - have))
    flat = len(g.tris) == len(sc.entities)   # every primitive a known triangle: all classes apply
    if flat:
        assert {R.H2[c] for c in np.unique(rs["h2"][hit])} == set(R.H2), name
        assert {R.LIGHTS[c] for c in np.unique(rs["light"][hit])} == set(R.LIGHTS), name
    assert (rs["h2"][~hit] == -1).all() and (rs["h2"][hit] >= 0).all()
    if name in SHADOW_SCENES:
        oc = ref["occl"][hit]
        assert (oc == 1).mean() >= 0.10 and (oc == 0).mean() >= 0.10, (name, (oc == 1).mean())
    # the direction edge cases are what they say
    d = rs["recs"][:, 3:6]
    for cls, zeros in (("axis1", 1), ("axis2", 2)):
        sel = rs["h1"] == R.H1.index(cls)
        assert ((d[sel] == 0.0).sum(1) == zeros).all()
        assert np.signbit(d[sel][d[sel] == 0.0]).any() and (~np.signbit(d[sel][d[sel] == 0.0])).any()
    for cls, tiny in (("tiny_1e-20", 1e-20), ("tiny_1e-45", 1e-45)):
        sel = rs["h1"] == R.H1.index(cls)
        small = np.abs(d[sel]) <= 1e6 * tiny   # (renormalised after the component was set)
        assert (small.sum(1) >= 1).all() and (d[sel][small] != 0.0).all()
        if tiny < 1e-38:   # below fp32's normal range: the cast underflows (1e-20 stays normal: a reciprocal of 1e20)
            assert (np.abs(d[sel][small]).astype(np.float32) < 1.2e-38).all()


def test_ray_sets_hold_ties_and_both_shadow_answers():
    """Summed over the scenes with shared edges or coincident quads: at least 50 rays whose hop-1 hit
    has two or more primitives at the best t, and at least 50 such hop-2 hits; over all scenes at
    least 10 % of the hits lit and 10 % shadowed."""
    n1 = n2 = 0
    for name in TIE_SCENES:
        ref = query_set(name)[3]
        n1 += int((ref["nties1"] >= 2).sum())
        n2 += int((ref["nties2"] >= 2).sum())
    assert n1 >= 50 and n2 >= 50, (n1, n2)
    oc = np.concatenate([query_set(name)[3]["occl"] for name in QUERY_SCENES])
    oc = oc[oc >= 0]
    assert (oc == 1).mean() >= 0.10 and (oc == 0).mean() >= 0.10


def test_x_query_single_ray_and_none():
    sc = S.named_scene("cornell")
    rec = np.array([[-10.0, 0.0, 0.0, 1.0, 0.0, 0.0, 5.0, 0.0, 4.5, -1.0, 0.0, 0.0]])
    q = U.oracle_x_query(sc.to_scn(), rec)
    assert q["prim1"][0] in (0, 1) and q["t1"][0] == 20.0 and q["prim2"][0] == -1 and np.isposinf(q["t2"][0])
    assert len(U.oracle_x_query(sc.to_scn(), np.zeros((0, 12)))["prim1"]) == 0
