"""GPU (gfx950): Mode R's primitive tests on the device, record by record, against the COMPILED REFERENCE.

gi_kat_r_prims runs the functions the Mode R kernels call -- tri_hit(const TriRec&) on the builder's record,
sphere_hit, box_hit and the grouped node test r_box_test<4> (4 lanes per record, a ballot) -- over the
adversarial records of tests/r_prims_cases.py.  The assertions are those of tests/test_r_prims_host.py with the
hook's output in place of the host checker's: the generator's sha256 equals the fixture's, the oracle reproduces
the fixture (tests/golden/adv_<kind>.npz: the reference's answers as digests), and the device equals the oracle
on every case -- hit exactly, P and N bit for bit, nothing excluded, no tolerance.  One launch per test.

gi_kat_r_entities runs every ray of tests/golden/rays_<scene>.npz against every entity through the kernels'
ent_hit: hit equal and P, N bit for bit with the reference's recorded answers for every (ray, entity)."""
import os

import numpy as np
import pytest

import oracle_util as U

pytestmark = pytest.mark.gpu

gi = U.pkg()
S = U.scenes()

KIND = {"tris": gi.KAT_R_TRI, "spheres": gi.KAT_R_SPHERE, "boxes": gi.KAT_R_BOX}


@pytest.mark.parametrize("kind", ["tris", "spheres", "boxes"])
def test_device_primitives_equal_the_reference(kind):
    e = U.prims_expected(kind)   # the generator is the fixture's; the oracle reproduces the fixture
    got = gi.kat_r_prims(KIND[kind], e["recs"])
    U.assert_prims_equal(kind, "gi_kat_r_prims", got["hit"], got["pn"])


def test_grouped_node_test_equals_the_plain_one():
    e = U.prims_expected("boxes")
    plain = gi.kat_r_prims(gi.KAT_R_BOX, e["recs"])["hit"]
    grouped = gi.kat_r_prims(gi.KAT_R_BOX4, e["recs"])["hit"]
    U.assert_prims_equal("boxes", "r_box_test<4>", grouped)
    bad = np.flatnonzero(plain != grouped)
    assert bad.size == 0, f"grouped != plain on {bad.size} records; first {bad[0]}: {e['recs'][bad[0]].tolist()}"


def mixed_prefix(kind, n):
    """n records drawn evenly across the whole case list (every class), in a fixed order."""
    e = U.prims_expected(kind)
    idx = (np.arange(n, dtype=np.int64) * e["recs"].shape[0]) // max(n, 1)
    return e, idx


@pytest.mark.parametrize("n", [0, 1, 3, 63, 64, 65, 257])
def test_partial_waves(n):
    """Record counts that leave partial waves and partial lane groups: the grouped node test's 4 lanes per
    record must all be active in the last wave too.  The leading n cases and n cases spread over all classes."""
    for kind, k in (("boxes", gi.KAT_R_BOX4), ("boxes", gi.KAT_R_BOX), ("tris", gi.KAT_R_TRI), ("spheres", gi.KAT_R_SPHERE)):
        e = U.prims_expected(kind)
        got = gi.kat_r_prims(k, e["recs"][:n])
        U.assert_prims_equal(kind, f"gi_kat_r_prims kind {k}, first {n}", got["hit"], got["pn"], n=n)
        _, idx = mixed_prefix(kind, n)
        got = gi.kat_r_prims(k, e["recs"][idx])
        assert ((got["hit"] != 0) == (e["hit"][idx] != 0)).all(), (kind, k, n)
        if got["pn"] is not None:
            assert U.bits_equal(got["pn"], e["pn"][idx]).all(), (kind, k, n)


@pytest.mark.parametrize("scene", ["main", "cornell", "zoo"])
def test_entity_tests_equal_the_reference(scene):
    z = np.load(os.path.join(U.GOLDEN, f"rays_{scene}.npz"))
    sc = S.named_scene(scene)
    dev = gi.DeviceScene.from_scene(sc)
    got = dev.kat_r_entities(z["rays"])
    assert got["hit"].shape == z["hit"].shape
    bad = np.argwhere((got["hit"] != z["hit"]) | ~U.bits_equal(got["pn"], z["pn"]).all(2))
    assert bad.shape[0] == 0, (f"{scene}: {bad.shape[0]} (ray, entity) pairs differ from the reference; first: ray {bad[0][0]} "
                               f"{z['rays'][bad[0][0]].tolist()} entity {bad[0][1]} got {got['hit'][tuple(bad[0])]} "
                               f"{got['pn'][tuple(bad[0])].tolist()} reference {z['hit'][tuple(bad[0])]} {z['pn'][tuple(bad[0])].tolist()}")
