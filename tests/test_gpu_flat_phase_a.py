"""GPU: the flat leaf query's Phase A as it is since round 8 -- hit bits shifted into the candidate mask
(leaf k at bit n - 1 - k), the nearest candidate carried as a key (entry distance with the leaf index in
its low five bits), the any hit's candidate taken from the mask after the loop -- ray by ray against
the oracle's brute force, and a whole Cornell frame with more units than resident lanes.

Leaf tables of 1, 4, 5, 31 and 32 leaves cover the four-record loop's remainders (1, 0, 1, 3, 0) and the
mask's top bit; ray counts of 1, 63, 64, 65 and 257 cover a lone lane, a wave one short, full, one
over (a second wave with one ray) and a second workgroup.  No tolerance: primitives and shadow
answers equal, t bit for bit."""
import numpy as np
import pytest

import oracle_util as U
import x_rays as R
from x_scenes import soup, with_env

pytestmark = pytest.mark.gpu

gi = U.pkg()
S = U.scenes()

LEAVES = (1, 4, 5, 31, 32)
COUNTS = (1, 63, 64, 65, 257)
N_RAYS = 512 + 37


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    return torch


_sets = {}


def query_case(name):
    """(scene, device scene, near rays' records, brute-force reference over them), built once per scene."""
    if name not in _sets:
        sc, env = (S.named_scene("cornell"), {}) if name == "cornell" else soup(int(name))
        d = with_env(env, lambda: gi.DeviceScene.from_scene(sc))
        skip_cos = d.kat_x_query(np.array([[0.0, 0, 0, 1, 0, 0, 0, 0, 0, 1, 0, 0]]), sc.cam_pos)["skip_cos"]
        scn = sc.to_scn()
        U.oracle_accel(0)   # brute force
        try:
            rs = R.ray_set(sc, N_RAYS, skip_cos, 2019, lambda recs: U.oracle_x_query(scn, recs))
            recs = np.ascontiguousarray(rs["recs"][R.near(rs)])
            ref = U.oracle_x_query(scn, recs)
        finally:
            U.oracle_accel(-1)
        for a in [recs] + list(ref.values()):
            a.setflags(write=False)
        _sets[name] = (sc, d, recs, ref)
    return _sets[name]


@pytest.mark.parametrize("name", [str(n) for n in LEAVES] + ["cornell"])
def test_phase_a_query_kat_equals_brute_force(torch_cuda, name):
    """gi_kat_x_query in the flat variant over soups of 1, 4, 5, 31 and 32 single-triangle leaves and the
    Cornell box, in calls of 1, 63, 64, 65 and 257 rays taken from different parts of the scene's set:
    prim1, occl, prim2 equal brute force and t1, t2 are bit-equal."""
    sc, d, recs, ref = query_case(name)
    var = d.kat_x_variant(0)
    assert var["FLAT"] and var["LDS"], var
    assert len(recs) >= 257 + 65
    hits = 0
    for j, n in enumerate(COUNTS):
        lo = (j * 61) % (len(recs) - n + 1)
        out = d.kat_x_query(recs[lo:lo + n], sc.cam_pos, 0)
        for k in ("prim1", "occl", "prim2"):
            ne = out[k] != ref[k][lo:lo + n]
            assert not ne.any(), f"{name} leaves, {n} rays from {lo}: {k} differs at ray {lo + int(np.flatnonzero(ne)[0])}"
        for k in ("t1", "t2"):
            ne = ~U.bits_equal(out[k], ref[k][lo:lo + n])
            assert not ne.any(), f"{name} leaves, {n} rays from {lo}: {k} differs at ray {lo + int(np.flatnonzero(ne)[0])}"
        hits += int((out["prim1"] >= 0).sum())
    assert hits > 0, name   # the calls see the scene


def test_phase_a_whole_frame_with_refills_bit_exact(torch_cuda):
    """The Cornell box at 160 x 120, 32 spp, depth 8: 614,400 units, more than the lanes of five resident
    workgroups per CU, so every resident wave takes work and refills.  fp64 radiance bit for bit and the
    same RGB888 as the CPU oracle; the form is k_seg in the flat variant."""
    torch = torch_cuda
    sc = S.named_scene("cornell")
    d = gi.DeviceScene.from_scene(sc)
    w, h, spp, depth, seed = 160, 120, 32, 8, 2019
    assert w * h * spp > 5 * 256 * 256
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
    assert (o["hit"] >= 0).mean() >= 0.30
