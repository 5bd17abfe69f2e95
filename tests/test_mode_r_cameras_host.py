"""CPU: Mode R away from Scene's default camera.  The placements of tests/r_cameras.py on the oracle
against the COMPILED REFERENCE's frames (tests/golden/rcam_<scene>.npz, make_golden.py `cameras`; live
where oracle/_ref exists), bit for bit as test_oracle_golden.py's default-camera frames are, and the
conditions the placements were chosen under -- so the oracle is a sound reference for the device at
these placements (tests/test_gpu_mode_r_cameras.py)."""
import numpy as np
import pytest

import oracle_util as U
import r_cameras as RC

GOLDEN_SCENES = [s for s in RC.SCENES if RC.load_golden(s) is not None]


def _same_as_reference(o, r, what):
    """The keys of test_mode_r_bit_exact_vs_reference_golden (and ncand), on every pixel."""
    assert not np.isnan(r["rgb"]).any(), f"{what}: NaN pixels in the reference"
    assert not RC.texel_ub_mask(r["hit"], r["uv"]).any(), f"{what}: texel-UB pixels in the reference"
    assert U.bits_equal(o["rgb"], r["rgb"]).all(), f"{what}: fp64 radiance differs from the reference"
    assert (o["hit"] == r["hit"]).all(), what
    assert (o["uv"] == r["uv"]).all(), what
    assert (o["ncand"] == r["ncand"]).all(), what
    assert (o["nnode"] == r["nnode"]).all(), what
    assert (o["q"] == r["q"]).all(), what


def test_goldens_present():
    """Every scene but the 4100-triangle soup has its fixture (that one only if it is small enough)."""
    assert set(RC.SCENES) - set(GOLDEN_SCENES) <= {"soup4100"}


@pytest.mark.parametrize("scene", GOLDEN_SCENES)
def test_mode_r_cameras_bit_exact_vs_reference_golden(scene):
    g = RC.load_golden(scene)
    assert g["meta"]["scene_sha256"] == RC.base_scene(scene).digest(), "scene generator drifted from the fixture"
    assert g["meta"]["placements"] == [p[0] for p in RC.CAMERAS[scene]], "the table drifted from the fixture"
    for name, pos, look, focal in RC.CAMERAS[scene]:
        z = g[name]
        assert tuple(z["pos"]) == pos and tuple(z["look"]) == look and float(z["focal"]) == focal, name
        _same_as_reference(RC.oracle_frame(scene, name), z, f"{scene}/{name}")


@pytest.mark.skipif(not U.have_ref(), reason="compiled reference only in the build container")
@pytest.mark.parametrize("scene", RC.SCENES)
def test_mode_r_cameras_live_vs_reference(scene):
    for name, *_ in RC.CAMERAS[scene]:
        r = U.ref_render(RC.scene_at(scene, name).to_scn(), RC.W, RC.H)
        _same_as_reference(RC.oracle_frame(scene, name), r, f"{scene}/{name}")


@pytest.mark.parametrize("scene", RC.SCENES)
def test_placement_conditions(scene):
    """What the placements are for (r_cameras.py), on the oracle: the seen share, the soups' entity
    counts, all eight sign patterns of the centre pixel's direction, a frame seen through the backward
    half-line alone, no NaN and no texel-UB pixel; and the kinds of view every scene has."""
    names = [p[0] for p in RC.CAMERAS[scene]]
    assert len(names) == len(set(names)) >= 6
    patterns, behind_only = set(), []
    for name in names:
        o = RC.oracle_frame(scene, name)
        hit = o["hit"] >= 0
        seen = hit.mean()
        ents = len(np.unique(o["hit"][hit]))
        print(f"{scene}/{name}: seen {seen:.3f}, {ents} entities, max ncand {int(o['ncand'].max())}")
        assert np.isfinite(o["dirs"]).all()
        assert seen >= (0.45 if scene == "cornell" else 0.05), name
        if scene in RC.SOUPS:
            assert ents >= 50, name
        assert not np.isnan(o["rgb"]).any() and not RC.texel_ub_mask(o["hit"], o["uv"]).any(), name
        patterns.add(RC.sign_pattern(o["dirs"][(RC.H // 2) * RC.W + RC.W // 2]))
        if (o["t"][hit] < 0).all():
            behind_only.append(name)
    assert patterns == set(range(8)), f"sign patterns of the centre pixel: {sorted(patterns)}"
    assert "behind" in behind_only
    if scene != "cornell":   # (cornell's table: centre-x, centre+y / -y, oblique_*, steep_down, far_*, and the camera is inside)
        for kind in ("minus_x", "plus_y", "minus_y", "oct_mpm", "steep_down", "steep_up", "inside", "behind", "far_1e3"):
            assert kind in names, kind
    # the exact-zero direction components of the axis views
    for name, axis in (("centre-x", 0), ("centre+y", 1), ("centre-y", 1)) if scene == "cornell" else \
            (("minus_x", 0), ("plus_y", 1), ("minus_y", 1)):
        _, pos, look, _ = RC.placement(scene, name)
        d = np.array(look) - np.array(pos)
        assert d[axis] != 0 and (np.delete(d, axis) == 0).all(), name


def test_scene_copies_leave_the_default_scene_alone():
    sc = RC.scene_at("cornell", "behind")
    assert (sc.cam_pos, sc.cam_look, sc.focal) == ((25.0, 0.5, 0.25), (26.0, 0.5, 0.3), 5 * RC.F)
    assert RC.base_scene("cornell").cam_pos == (-10.0, 0.0, 0.0)
    assert U.scenes().named_scene("cornell").digest() == RC.base_scene("cornell").digest()


def test_soup4100_is_a_flat_phase_scene_with_overflowing_tiles():
    """The 4100-triangle soup is over the 4096-entity switch to the flat phases, and at
    OVERFLOW_PLACEMENT some but not all tiles must overflow with GI_RF_PER_SLOT=0
    (test_gpu_mode_r_cameras.py's route test counts them).  A lower bound of a tile's candidate pairs:
    the device queues every entity of a line-BVH leaf whose box the pixel's line crosses, the leaf's box
    holds its entities' own (gi_bvh.cpp build_rcand: the box of the sphere about the centroid, radius
    1.01 x the farthest vertex's distance), and only entities that appear in some octree leaf are in
    the BVH -- so the lines' crossings of those entities' boxes, counted here, are among the pairs.
    Tiles over 512 by this count overflow for certain; the tiles far under it (measured on the
    device: its pairs exceed this count by a few per cent) keep the count below the frame's tiles."""
    sc = RC.scene_at("soup4100", RC.OVERFLOW_PLACEMENT)
    assert len(sc.entities) > 4096
    o = RC.oracle_frame("soup4100", RC.OVERFLOW_PLACEMENT)
    leaves = [l.split() for l in U.oracle_tree(sc.to_scn()).splitlines() if l.startswith("node")]
    appear = sorted({int(e) for l in leaves if l[3] == "1" for e in l[11:]})
    v = np.array([sc.entities[e].args for e in appear]).reshape(-1, 3, 3)
    c = v.mean(1)
    r = np.sqrt(((v - c[:, None]) ** 2).sum(2).max(1) * 1.0201)
    lo, hi, pos = c - r[:, None], c + r[:, None], np.array(sc.cam_pos)
    iv = 1.0 / o["dirs"]   # (no zero component at this placement)
    t0, t1 = (lo[None] - pos) * iv[:, None, :], (hi[None] - pos) * iv[:, None, :]
    n = (np.minimum(t0, t1).max(2) <= np.maximum(t0, t1).min(2)).sum(1).reshape(RC.H, RC.W)
    per_tile = [int(n[y:y + 8, x:x + 8].sum()) for y in range(0, RC.H, 8) for x in range(0, RC.W, 8)]
    print("lower bound of the pairs per tile:", per_tile)
    assert sum(p > 512 for p in per_tile) >= 2 and sum(p < 256 for p in per_tile) >= 2, per_tile
