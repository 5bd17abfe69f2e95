"""GPU checks of the flat leaf query (gi_wf.hip wf_flat): scenes staged in LDS with at most
GI_XFLAT_MAX leaves answer k_seg's closest-hit and shadow queries from the leaf table instead of
walking the tree.  Frames must not change: against the tree walk (GI_X_FLAT=0, a child process) and
against the oracle at the edges of eligibility."""
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_util as U
from x_scenes import (XFLAT_MAX, coincident_quads, empty as _empty, grazing_scene as _grazing_scene,
                      one_triangle as _one_triangle, soup as _soup, three_record_leaves as _three_record_leaves,
                      with_env as _with_env, with_sphere as _with_sphere)

pytestmark = pytest.mark.gpu

gi = U.pkg()
S = U.scenes()


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    return torch


def cam_of(sc):
    return gi.Camera(sc.cam_pos, sc.cam_look, sc.focal)


def _tree_cases():
    return [("cornell", S.named_scene("cornell"), 64, 48, 4, 8),
            ("cornell_mirror", S.named_scene("cornell_mirror"), 48, 40, 4, 6),
            ("grazing_floor", _grazing_scene("floor"), 96, 64, 4, 6),
            ("grazing_tilted", _grazing_scene("tilted"), 96, 64, 4, 6)]


@pytest.fixture(scope="module")
def tree_frames(torch_cuda, tmp_path_factory):
    """The cases' frames rendered with GI_X_FLAT=0 (read once per process: one child process)."""
    tmp = tmp_path_factory.mktemp("flat")
    cases = []
    for name, sc, w, h, spp, depth in _tree_cases():
        p = tmp / (name + ".scn")
        p.write_text(sc.to_scn())
        cases.append((name, str(p), w, h, spp, depth))
    out = tmp / "tree.npz"
    code = ("import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r); import oracle_util as U; "
            "gi = U.pkg(); S = U.scenes(); res = {}\n"
            "for name, path, w, h, spp, depth in %r:\n"
            "    sc = S.parse_scn(open(path).read()); d = gi.DeviceScene.from_scene(sc)\n"
            "    assert d.x_form(spp=spp, depth=depth) == 'k_seg'\n"
            "    rgb, rgb8 = d.render(gi.Camera(sc.cam_pos, sc.cam_look, sc.focal), sc.light, w, h, mode=gi.MODE_X, "
            "spp=spp, depth=depth, seed=2019)\n"
            "    res[name] = rgb; res[name + '_8'] = rgb8\n"
            "np.savez(%r, **res)") % (U.ROOT, os.path.join(U.ROOT, "tests"), cases, str(out))
    subprocess.run([sys.executable, "-c", code], check=True, timeout=300, env=dict(os.environ, GI_X_FLAT="0"))
    return {k: v for k, v in np.load(out).items()}, {c[0]: c[1] for c in cases}


@pytest.mark.parametrize("case", [c[0] for c in _tree_cases()])
def test_flat_query_frame_equals_tree_walk(torch_cuda, tree_frames, case):
    """k_seg with the flat leaf query (the default for these LDS-resident scenes) against k_seg walking
    the tree (GI_X_FLAT=0): fp64 radiance bit for bit and the same RGB888, on the Cornell box, its
    mirror variant and the grazing-light scenes (the own-plane skip at and below its bound)."""
    ref, paths = tree_frames
    name, _, w, h, spp, depth = next(c for c in _tree_cases() if c[0] == case)
    sc = S.parse_scn(open(paths[name]).read())   # the very scene text the child process rendered
    d = gi.DeviceScene.from_scene(sc)
    assert d.x_form(spp=spp, depth=depth) == "k_seg"
    rgb, rgb8 = d.render(cam_of(sc), sc.light, w, h, mode=gi.MODE_X, spp=spp, depth=depth, seed=2019)
    assert U.bits_equal(rgb, ref[name]).all(), name
    assert (rgb8 == ref[name + "_8"]).all(), name
    assert (rgb > 0).any()


def _render_stats(torch, d, sc, w, h, spp, depth, seed):
    st = torch.zeros(gi.STATS_N, dtype=torch.int64, device="cuda")
    buf = torch.zeros(w * h * 3, dtype=torch.float64, device="cuda")
    d.render_device(cam_of(sc), sc.light, w, h, buf.data_ptr(), mode=gi.MODE_X, spp=spp, depth=depth, seed=seed,
                    stats_ptr=st.data_ptr())
    torch.cuda.synchronize()
    return buf.cpu().numpy().reshape(-1, 3), st.cpu().numpy()


EDGE = {"one_triangle": (_one_triangle, 1), "empty": (_empty, 0),
        "soup_max": (lambda: _soup(XFLAT_MAX), XFLAT_MAX), "soup_max_plus_1": (lambda: _soup(XFLAT_MAX + 1), None),
        "three_record_leaves": (_three_record_leaves, 4), "sphere": (_with_sphere, 18)}


@pytest.mark.parametrize("case", sorted(EDGE))
def test_flat_query_edges_bit_exact_to_oracle(torch_cuda, case):
    """Frames at the edges of eligibility equal the oracle's bit for bit: one triangle, the empty scene,
    soups of exactly GI_XFLAT_MAX leaves (flat) and one more (the tree walk), leaves of three records
    (the pair loop's odd tail) and a scene with a sphere (the non-triangle kernels).  Which query ran
    is read from the stats: the flat query counts the 256-byte units of the table per query
    (GI_STAT_NODES = units x (rays - samples resolved without traversal)), the tree walk its visits of
    interior nodes."""
    make, leaves = EDGE[case]
    sc, env = make()
    d = _with_env(env, lambda: gi.DeviceScene.from_scene(sc))
    w, h, spp, depth, seed = 32, 32, 2, 3, 7
    assert d.x_form(spp=spp, depth=depth) == "k_seg"
    rgb, st = _render_stats(torch_cuda, d, sc, w, h, spp, depth, seed)
    o = U.oracle_render(sc.to_scn(), w, h, mode=1, spp=spp, depth=depth, seed=seed)
    same = U.bits_equal(rgb, o["rgb"]).all(1)
    assert same.all(), f"{case}: {int((~same).sum())} of {same.size} pixels differ"
    queries = int(st[gi.STAT_RAYS]) - int(st[gi.STAT_X_RESOLVED])
    if case != "empty":
        assert (o["rgb"] > 0).any() and queries > 0
    if leaves is not None:
        units = (leaves * 32 + 255) // 256
        assert int(st[gi.STAT_NODES]) == units * queries, (case, st[gi.STAT_NODES], units, queries)
    else:   # one leaf too many: the tree walk (its node count is no multiple of the table's units per query)
        units = ((XFLAT_MAX + 1) * 32 + 255) // 256
        assert int(st[gi.STAT_NODES]) != units * queries, (case, st[gi.STAT_NODES], units, queries)
        assert int(st[gi.STAT_NODES]) > 0


def test_flat_query_equal_t_tie_break(torch_cuda):
    """Two coincident quads (every triangle duplicated, in another colour): each hit has two primitives
    at the same t, and the frame equals the oracle's, which keeps the smaller primitive index."""
    sc, _ = coincident_quads()
    d = gi.DeviceScene.from_scene(sc)
    w, h, spp, depth, seed = 24, 24, 2, 3, 7
    assert d.x_form(spp=spp, depth=depth) == "k_seg"
    rgb, st = _render_stats(torch_cuda, d, sc, w, h, spp, depth, seed)
    o = U.oracle_render(sc.to_scn(), w, h, mode=1, spp=spp, depth=depth, seed=seed)
    assert U.bits_equal(rgb, o["rgb"]).all()
    assert (o["rgb"] > 0).any()
    queries = int(st[gi.STAT_RAYS]) - int(st[gi.STAT_X_RESOLVED])
    assert int(st[gi.STAT_NODES]) == queries > 0   # the flat query: one unit of table per query
