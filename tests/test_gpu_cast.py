"""GPU: the batched ray queries (gi_intersect, gi_occluded and their device variants) against the
oracle's brute force.

The queries run k_cast (gi_wf.hip) in the kernel variant a Mode X render of the scene runs, over the
ray sets of tests/x_rays.py as tests/cast_rays.py arranges them: near and far origins mixed in one
call, second hops from the hit points, tmax on and around the closest hit.  No tolerance on t, the
primitive or the occlusion answer: primitives equal, t bit for bit, a miss is (-1, +inf) with entity
-1 and a zero normal.  Only the geometric checks of the normal carry a bound (1e-9 at unit scale:
about 1e6 ulp, while a wrong primitive, sign or length is an error of order 1)."""
import ctypes

import numpy as np
import pytest

import cast_rays as C
import oracle_util as U
import x_rays as R
from x_scenes import QUERY_SCENES, with_env

pytestmark = pytest.mark.gpu

gi = U.pkg()
S = U.scenes()
NTOL = 1e-9


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    return torch


_devs = {}


def dev_of(name):
    if name not in _devs:
        sc, env = QUERY_SCENES[name][0]()
        _devs[name] = (sc, with_env(env, lambda: gi.DeviceScene.from_scene(sc)))
    return _devs[name]


def check_variant(name):
    want, lds, node_bytes = C.VARIANTS[name]
    sc, d = dev_of(name)
    var, info = d.kat_x_variant(0), d.info()
    assert {k: var[k] for k in want} == want, (name, var)
    assert info["x_lds_resident"] == lds and info["x_node_bytes"] == node_bytes, (name, info)
    return sc, d


def assert_closest(name, what, exp, out):
    """Every output of an intersect call: t and prim as expected; a miss carries entity -1 and a zero normal."""
    bad = C.first_difference(exp, {k: out[k] for k in ("prim", "t") if k in out})
    if bad is not None:
        print(f"{name} {what}: {bad}")
    assert bad is None, f"{name} {what}: {bad[:600]}"
    if "t" in out:
        assert U.bits_equal(out["t"], exp["t"]).all()
    miss = exp["prim"] < 0
    if "t" in out:
        assert np.isposinf(out["t"][miss]).all()
    if "entity" in out:
        assert (out["entity"][miss] == -1).all() and (out["entity"][~miss] >= 0).all()
    if "normal" in out:
        assert (out["normal"][miss] == 0.0).all()


def assert_occluded(name, what, exp, occl):
    bad = C.first_difference(exp, {"occl": occl})
    if bad is not None:
        print(f"{name} {what}: {bad}")
    assert bad is None, f"{name} {what}: {bad[:600]}"


@pytest.mark.parametrize("name", sorted(QUERY_SCENES))
def test_intersect_both_hops_equal_brute_force(torch_cuda, name):
    """Every variant: the scene's variant is asserted first (gi_kat_x_variant with flags 0, x_lds_resident,
    x_node_bytes), then hop 1 (near rays and rays from 1e3 and 1e6 extents out in one call: the far-origin
    rule per lane) and hop 2 (from the hit points, no skip)."""
    sc, d = check_variant(name)
    for what, exp in (("hop 1", C.hop1(name)), ("hop 2", C.hop2(name))):
        if len(exp["prim"]) == 0:   # (the empty scene has no second hop)
            assert name == "empty" and what == "hop 2"
            continue
        assert len(exp["prim"]) % 64 != 0 or what == "hop 2"
        assert_closest(name, what, exp, d.intersect(exp["rays"]))
        assert_occluded(name, what, exp, d.occluded(exp["rays"]))


@pytest.mark.parametrize("name", sorted(QUERY_SCENES))
def test_tmax_is_an_open_upper_end(torch_cuda, name):
    """tmax = inf, t1, nextafter(t1), t1 / 2, 2 t1, 1e-7, 0, -1 on hits and inf, 1e3 on misses: the closest
    hit is (prim1, t1) exactly when t1 < tmax, and occluded says the same."""
    sc, d = check_variant(name)
    exp = C.tmax_classes(name)
    assert_closest(name, "tmax", exp, d.intersect(exp["rays"]))
    assert_occluded(name, "tmax", exp, d.occluded(exp["rays"]))


def _unit(v):
    return v / np.sqrt((v * v).sum(-1, keepdims=True))


@pytest.mark.parametrize("name", ["cornell", "cornell_sphere", "one_triangle", "coincident", "soup1000"])
def test_attributes_of_triangle_and_sphere_scenes(torch_cuda, name):
    """Scenes of ImpTriangle and ImpSphere only: entity == prim; a triangle's normal is the unit normal of
    its plane, a sphere's is parallel to P - c; both face the ray."""
    sc, d = check_variant(name)
    assert all(e.kind in (S.IMP_TRIANGLE, S.IMP_SPHERE) for e in sc.entities)
    exp = C.hop1(name)
    out = d.intersect(exp["rays"])
    assert_closest(name, "attributes", exp, out)
    hit = exp["prim"] >= 0
    assert hit.sum() > 100 or name == "one_triangle"
    assert (out["entity"] == out["prim"]).all()
    o, dr, n = exp["rays"][hit, 0:3], exp["rays"][hit, 3:6], out["normal"][hit]
    prim = out["prim"][hit]
    assert (np.abs(np.sqrt((n * n).sum(1)) - 1.0) <= NTOL).all()
    assert ((n * _unit(dr)).sum(1) <= 0.0).all()
    ptri = R.Geo(sc).ptri
    assert len(ptri) == len(sc.entities)
    tri = ptri[prim]
    flat = ~np.isnan(tri).any((1, 2))
    e1, e2 = _unit(tri[flat, 1] - tri[flat, 0]), _unit(tri[flat, 2] - tri[flat, 0])
    assert (np.abs((n[flat] * e1).sum(1)) <= NTOL).all() and (np.abs((n[flat] * e2).sum(1)) <= NTOL).all()
    if (~flat).any():
        c = np.array([sc.entities[p].args[:3] for p in prim[~flat]])
        P = C.hop2_points(o[~flat], dr[~flat], out["t"][hit][~flat])
        rad = _unit(P - c)
        assert (np.sqrt((np.cross(n[~flat], rad) ** 2).sum(1)) <= NTOL).all()
    assert (~flat).any() == (name == "cornell_sphere")


def test_attributes_of_meshed_entities(torch_cuda):
    """main (an ExpQuad, two ImpSpheres): primitives 0 and 1 are the quad's triangles, entity 0; 2 and 3 the
    spheres, entities 1 and 2.  zoo (every entity kind): the observed primitive -> entity map is
    single-valued, non-decreasing and within the scene's entities."""
    sc = S.named_scene("main")
    d = gi.DeviceScene.from_scene(sc)
    o, dr, _ = R.hop1(sc, 1024 + 37, 2019)
    rays = np.zeros((len(o), gi.RAY_DOUBLES))
    rays[:, 0:3], rays[:, 3:6], rays[:, 6] = o, dr, np.inf
    out = d.intersect(rays, want=("prim", "entity"))
    seen = {int(p): int(e) for p, e in zip(out["prim"], out["entity"])}
    assert seen == {-1: -1, 0: 0, 1: 0, 2: 1, 3: 2}, seen
    assert (out["entity"] == np.array([-1, 0, 0, 1, 2])[out["prim"] + 1]).all()

    scz, dz = check_variant("zoo")
    exp = C.hop1("zoo")
    out = dz.intersect(exp["rays"], want=("prim", "entity"))
    assert (out["prim"] == exp["prim"]).all()
    hit = out["prim"] >= 0
    pairs = np.unique(np.stack([out["prim"][hit], out["entity"][hit]], 1), axis=0)
    assert len(pairs) == len(np.unique(pairs[:, 0])) > 50        # single-valued
    assert (np.diff(pairs[:, 1]) >= 0).all()                     # non-decreasing in the primitive
    n_ent = dz.info()["n_entities"]
    assert n_ent == len(scz.entities) and pairs[:, 1].min() >= 0 and pairs[:, 1].max() < n_ent
    assert len(np.unique(pairs[:, 1])) >= 4


@pytest.mark.parametrize("name", ["cornell", "soup1000"])
def test_more_rays_than_resident_lanes(torch_cuda, name):
    """2^20 + 37 rays (the device holds at most 256 CUs x 2048 lanes = 2^19): every wave's loop over its
    batches runs more than once, whatever the occupancy.  cornell: LDS, flat; soup1000: HBM."""
    sc, d = check_variant(name)
    exp = C.drawn(C.tmax_classes(name), 2 ** 20 + 37, 7)
    out = d.intersect(exp["rays"], want=("t", "prim"))
    assert_closest(name, "2^20 + 37 rays", exp, out)
    assert_occluded(name, "2^20 + 37 rays", exp, d.occluded(exp["rays"]))


def test_small_and_odd_calls(torch_cuda):
    sc, d = check_variant("cornell")
    exp = C.hop1("cornell")
    none = d.intersect(np.zeros((0, gi.RAY_DOUBLES)))
    assert [none[k].shape for k in ("t", "prim", "entity", "normal")] == [(0,), (0,), (0,), (0, 3)]
    assert d.occluded(np.zeros((0, gi.RAY_DOUBLES))).shape == (0,)
    i = int(np.flatnonzero(exp["prim"] >= 0)[0])
    one = {k: v[i:i + 1] for k, v in exp.items()}
    assert_closest("cornell", "one ray", one, d.intersect(np.ascontiguousarray(exp["rays"][i:i + 1])))
    assert d.occluded(np.ascontiguousarray(exp["rays"][i:i + 1]))[0] == 1
    only_t = d.intersect(exp["rays"], want=("t",))
    only_p = d.intersect(exp["rays"], want=("prim",))
    assert list(only_t) == ["t"] and list(only_p) == ["prim"]
    assert_closest("cornell", "t alone", exp, only_t)
    assert_closest("cornell", "prim alone", exp, only_p)


def test_malformed_rays_miss_and_leave_their_wave_alone(torch_cuda):
    """NaN and inf in o and d, a zero d and a NaN tmax, every third ray of the call, among good rays: the
    malformed rays miss, the good ones keep their exact answers.  Two scenes: the flat query, whose first
    phase runs uniformly over the wave, and the HBM tree walk."""
    bad_rows = []
    for k in range(6):
        for v in (np.nan, np.inf, -np.inf):
            bad_rows.append((k, v))
    for name in ("cornell", "soup1000"):
        sc, d = check_variant(name)
        src = C.hop1(name)
        rays = src["rays"].copy()
        prim, t, occl = src["prim"].copy(), src["t"].copy(), src["occl"].copy()
        mal = np.flatnonzero(np.arange(len(rays)) % 3 == 1)
        for j, i in enumerate(mal):
            kind = j % (len(bad_rows) + 2)
            if kind < len(bad_rows):
                rays[i, bad_rows[kind][0]] = bad_rows[kind][1]
            elif kind == len(bad_rows):
                rays[i, 3:6] = (0.0, -0.0, 0.0)
            else:
                rays[i, 6] = np.nan
        prim[mal], t[mal], occl[mal] = -1, np.inf, 0
        exp = dict(rays=rays, prim=prim, t=t, occl=occl, cls=src["cls"])
        assert (prim >= 0).sum() > 100
        out = d.intersect(rays)
        assert_closest(name, "malformed rays", exp, out)
        assert_occluded(name, "malformed rays", exp, d.occluded(rays))


def test_device_variant_on_a_stream(torch_cuda):
    """Torch tensors on a non-default stream, outputs 64 elements longer than the call and pre-filled:
    the host variant's results, the tails untouched, and no normal written where none is asked for."""
    torch = torch_cuda
    sc, d = check_variant("cornell")
    exp = C.tmax_classes("cornell")
    host = d.intersect(exp["rays"])
    host_occl = d.occluded(exp["rays"])
    n, pad = len(exp["prim"]), 64
    rays = torch.from_numpy(exp["rays"].copy()).cuda()

    def fresh():
        return dict(t=torch.full((n + pad,), -7.0, dtype=torch.float64, device="cuda"),
                    prim=torch.full((n + pad,), -777, dtype=torch.int32, device="cuda"),
                    entity=torch.full((n + pad,), -777, dtype=torch.int32, device="cuda"),
                    normal=torch.full((3 * (n + pad),), -7.0, dtype=torch.float64, device="cuda"),
                    occl=torch.full((n + pad,), -777, dtype=torch.int32, device="cuda"))
    a, b = fresh(), fresh()
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    assert st.cuda_stream != 0
    d.intersect_device(n, rays.data_ptr(), a["t"].data_ptr(), a["prim"].data_ptr(), a["entity"].data_ptr(),
                       a["normal"].data_ptr(), stream=st.cuda_stream)
    d.occluded_device(n, rays.data_ptr(), a["occl"].data_ptr(), stream=st.cuda_stream)
    d.intersect_device(n, rays.data_ptr(), b["t"].data_ptr(), b["prim"].data_ptr(), b["entity"].data_ptr(), 0,
                       stream=st.cuda_stream)
    st.synchronize()
    a = {k: v.cpu().numpy() for k, v in a.items()}
    b = {k: v.cpu().numpy() for k, v in b.items()}
    for r in (a, b):
        assert U.bits_equal(r["t"][:n], host["t"]).all() and (r["prim"][:n] == host["prim"]).all()
        assert (r["entity"][:n] == host["entity"]).all()
        assert (r["t"][n:] == -7.0).all() and (r["prim"][n:] == -777).all() and (r["entity"][n:] == -777).all()
    assert U.bits_equal(a["normal"][:3 * n].reshape(n, 3), host["normal"]).all() and (a["normal"][3 * n:] == -7.0).all()
    assert (a["occl"][:n] == host_occl).all() and (a["occl"][n:] == -777).all()
    assert (b["normal"] == -7.0).all() and (b["occl"] == -777).all()


def test_queries_share_no_state_with_renders(torch_cuda):
    """A query between two progressive passes does not end the progressive frame, and the frame equals the
    one-shot frame bit for bit; a query before and one after a whole render return identical arrays."""
    sc, d = check_variant("cornell")
    exp = C.hop1("cornell")
    cam = gi.Camera(sc.cam_pos, sc.cam_look, sc.focal)
    kw = dict(mode=gi.MODE_X, spp=4, depth=3, seed=5)
    before = d.intersect(exp["rays"])
    before_occl = d.occluded(exp["rays"])
    one_shot, one_shot8 = d.render(cam, sc.light, 32, 32, **kw)
    after = d.intersect(exp["rays"])
    for k in before:
        assert U.bits_equal(before[k], after[k]).all() if before[k].dtype == np.float64 else (before[k] == after[k]).all(), k
    d.render(cam, sc.light, 32, 32, samples=(0, 2), **kw)
    between = d.intersect(exp["rays"])
    assert (d.occluded(exp["rays"]) == before_occl).all()
    rgb, rgb8 = d.render(cam, sc.light, 32, 32, samples=(2, 4), **kw)
    assert U.bits_equal(rgb, one_shot).all() and (rgb8 == one_shot8).all()
    assert_closest("cornell", "between passes", exp, between)


def test_argument_errors(torch_cuda):
    """Negative n, NULL rays with n > 0 and every output NULL: GI_ERR_ARG with a message, before anything
    is launched (no call here hands the device a pointer it cannot read)."""
    sc, d = check_variant("cornell")
    L = gi.lib()
    dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    rays = np.ascontiguousarray(C.hop1("cornell")["rays"][:4])
    t, occl = np.zeros(4), np.zeros(4, np.int32)
    pr, pt, po = rays.ctypes.data_as(dp), t.ctypes.data_as(dp), occl.ctypes.data_as(ip)

    def refused(rc):
        assert rc == -1 and len(L.gi_last_error()) > 0, (rc, L.gi_last_error())
    refused(L.gi_intersect(d._h, -1, pr, pt, None, None, None))
    refused(L.gi_intersect(d._h, 4, None, pt, None, None, None))
    refused(L.gi_intersect(d._h, 4, pr, None, None, None, None))
    refused(L.gi_occluded(d._h, -1, pr, po))
    refused(L.gi_occluded(d._h, 4, None, po))
    refused(L.gi_occluded(d._h, 4, pr, None))
    refused(L.gi_intersect_device(d._h, -1, None, None, None, None, None, None))
    refused(L.gi_intersect_device(d._h, 4, None, None, None, None, None, None))
    refused(L.gi_occluded_device(d._h, -1, None, None, None))
    refused(L.gi_occluded_device(d._h, 4, None, None, None))
    torch = torch_cuda
    dr = torch.from_numpy(rays.copy()).cuda()
    refused(L.gi_intersect_device(d._h, 4, dr.data_ptr(), None, None, None, None, None))   # every output NULL
    with pytest.raises(gi.GIError, match=r"\(-1\)"):
        d.intersect_device(4, dr.data_ptr())
    assert (t == 0).all() and (occl == 0).all()
    assert L.gi_intersect(d._h, 0, None, pt, None, None, None) == 0   # n == 0: nothing to do
