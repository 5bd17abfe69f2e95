"""CPU: the batched ray queries' host side (gi_intersect, gi_occluded) -- the test inputs built by
tests/cast_rays.py against the oracle alone, the Python wrappers' argument checks, and the C-ABI's
declarations.  No device."""
import os
import re

import numpy as np
import pytest

import cast_rays as C
import oracle_util as U
from x_scenes import query_set

gi = U.pkg()
NEW = ("gi_intersect", "gi_occluded", "gi_intersect_device", "gi_occluded_device")


@pytest.mark.parametrize("name", ["cornell", "cornell_sphere", "soup1000", "zoo"])
def test_hop2_rays_reproduce_the_oracles_second_hop(name):
    """The hop-2 rays (P, d2), with P = o + t1 d formed in numpy by a multiply and an add, are the rays
    the oracle's own second hop traces: run as the first hop of new records, the brute force returns
    exactly (prim2, t2) of the original records."""
    sc, _, rs, ref = query_set(name)
    h2 = C.hop2(name)
    assert len(h2["prim"]) == int((ref["prim1"] >= 0).sum()) > 0
    n = len(h2["prim"])
    recs = np.concatenate([h2["rays"][:, 0:6], np.zeros((n, 3)), np.tile([1.0, 0.0, 0.0], (n, 1))], 1)
    U.oracle_accel(0)
    try:
        again = U.oracle_x_query(sc.to_scn(), recs)
    finally:
        U.oracle_accel(-1)
    i = h2["index"]
    assert (again["prim1"] == ref["prim2"][i]).all(), int((again["prim1"] != ref["prim2"][i]).sum())
    assert U.bits_equal(again["t1"], ref["t2"][i]).all()
    assert (h2["prim"] == ref["prim2"][i]).all() and U.bits_equal(h2["t"], ref["t2"][i]).all()
    assert (ref["prim2"][i] >= 0).any() and (ref["prim2"][i] < 0).any()


def test_hop1_mixes_near_and_far_origins_in_one_call():
    sc, _, rs, ref = query_set("cornell")
    h1 = C.hop1("cornell")
    assert (np.sort(h1["index"]) == np.arange(len(ref["prim1"]))).all()
    assert (h1["prim"] == ref["prim1"][h1["index"]]).all() and U.bits_equal(h1["t"], ref["t1"][h1["index"]]).all()
    far = np.array([c.startswith("far_") for c in h1["cls"]])
    per_wave = [far[k:k + 64] for k in range(0, len(far) - 63, 64)]
    mixed = sum(1 for w in per_wave if w.any() and not w.all())
    assert mixed >= len(per_wave) // 2, f"{mixed} of {len(per_wave)} waves hold near and far origins"
    assert np.isnan(h1["rays"][1::2, 7]).all() and (h1["rays"][0::2, 7] == 0).all()   # (the reserved field)


def test_tmax_classes_of_cornell_are_populated():
    """Every tmax class has at least 50 rays and both occlusion answers make up at least 10 % of the
    expected values (they hold by construction: three of the eight hit classes keep the hit)."""
    tm = C.tmax_classes("cornell")
    counts = {c: int((tm["tclass"] == j).sum()) for j, c in enumerate(C.TMAX_CLASSES)}
    assert min(counts.values()) >= 50, f"rays per tmax class: {counts}"
    n, ones = len(tm["occl"]), int(tm["occl"].sum())
    assert ones >= 0.1 * n and n - ones >= 0.1 * n, f"occluded {ones} of {n} rays, not occluded {n - ones}"
    assert ((tm["prim"] >= 0) == (tm["occl"] == 1)).all()
    # the open upper end, to the bit: tmax = t1 loses the hit, the next double keeps it
    at, nxt = tm["tclass"] == C.TMAX_CLASSES.index("t1"), tm["tclass"] == C.TMAX_CLASSES.index("nextafter(t1)")
    assert (tm["occl"][at] == 0).all() and (tm["occl"][nxt] == 1).all()
    assert (tm["rays"][nxt, 6] > tm["t"][nxt]).all() and np.isinf(tm["t"][at]).all()


def test_wrappers_reject_malformed_arrays_without_the_library(monkeypatch):
    """DeviceScene.intersect / occluded check shape, dtype and layout in Python and raise ValueError
    before the library is touched (here: lib() would fail the test)."""
    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(gi, "lib", no_lib)
    d = gi.DeviceScene.__new__(gi.DeviceScene)   # no scene: the checks come first
    good = np.zeros((5, gi.RAY_DOUBLES))
    bad = {"shape (n, 6)": np.zeros((5, 6)), "one dimension": np.zeros(8), "three dimensions": np.zeros((2, 5, 8)),
           "float32": good.astype(np.float32), "int64": good.astype(np.int64),
           "non-contiguous rows": np.zeros((5, 16))[:, ::2], "Fortran order": np.asfortranarray(good),
           "a list": good.tolist()}
    assert bad["non-contiguous rows"].shape == good.shape and bad["Fortran order"].shape == good.shape
    for what, a in bad.items():
        with pytest.raises(ValueError):
            d.intersect(a)
        with pytest.raises(ValueError):
            d.occluded(a)
    for want in ((), ("t", "t"), ("colour",)):
        with pytest.raises(ValueError):
            d.intersect(good, want=want)
    assert gi.RAY_DOUBLES == 8


def test_header_declares_the_queries_and_exports_list_them():
    hdr = open(os.path.join(U.ROOT, "include", "gi.h")).read()
    for f in NEW:
        assert re.search(r"^int %s\(gi_scene\* scene, int64_t n, const double\* " % f, hdr, re.M), f
        assert f in gi.EXPORTS
    assert "#define GI_RAY_DOUBLES 8" in hdr
    assert int(re.search(r"#define GI_ABI_VERSION (\d+)", hdr).group(1)) == gi.ABI_VERSION >= 12
