"""GPU checks of the light-dead leaves of the flat leaf query (gi_wf.hip wf_flat): a launch's
shadow queries leave out the boundary leaves its light cannot be occluded by.  Frames must not change:
every case is rendered with the launch's own mask and with GI_FLAG_X_ALL_LEAVES, compared bit for bit, and
both against the oracle."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

import oracle_util as U
from x_scenes import XFLAT_MAX, tri_scene, with_env, with_sphere

pytestmark = pytest.mark.gpu

gi = U.pkg()
S = U.scenes()
SEED = 2019


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "gpu tests need a device"
    return torch


def cam_of(sc):
    return gi.Camera(sc.cam_pos, sc.cam_look, sc.focal)


def _render(torch, d, sc, w, h, spp, depth, flags):
    st = torch.zeros(gi.STATS_N, dtype=torch.int64, device="cuda")
    buf = torch.zeros(w * h * 3, dtype=torch.float64, device="cuda")
    buf8 = torch.zeros(w * h * 3, dtype=torch.uint8, device="cuda")
    d.render_device(cam_of(sc), sc.light, w, h, buf.data_ptr(), buf8.data_ptr(), mode=gi.MODE_X, spp=spp, depth=depth,
                    seed=SEED, stats_ptr=st.data_ptr(), flags=flags | gi.FLAG_STATS)
    torch.cuda.synchronize()
    return buf.cpu().numpy().reshape(-1, 3), buf8.cpu().numpy().reshape(-1, 3), st.cpu().numpy()


def _check(torch, sc, w, h, spp, depth, flags=0, env=None, form="k_seg"):
    """The frame with the launch's own mask and with every leaf: equal bit for bit (fp64 and RGB888), both equal
    to the oracle's; the same rays, resolved samples and pixels; no more exact tests with the mask.  Returns
    (device scene, exact tests with the mask, with every leaf)."""
    d = with_env(env or {}, lambda: gi.DeviceScene.from_scene(sc))
    assert d.x_form(spp=spp, depth=depth, flags=flags) == form
    a, a8, sa = _render(torch, d, sc, w, h, spp, depth, flags)
    b, b8, sb = _render(torch, d, sc, w, h, spp, depth, flags | gi.FLAG_X_ALL_LEAVES)
    assert U.bits_equal(a, b).all() and (a8 == b8).all()
    o = U.oracle_render(sc.to_scn(), w, h, mode=1, spp=spp, depth=depth, seed=SEED)
    assert U.bits_equal(a, o["rgb"]).all() and U.bits_equal(b, o["rgb"]).all()
    assert (a8 == o["q"]).all()
    assert (o["rgb"] > 0).any()
    for k in (gi.STAT_RAYS, gi.STAT_X_RESOLVED, gi.STAT_PIXELS, gi.STAT_NODES):
        assert sa[k] == sb[k], k
    assert sa[gi.STAT_PRIMS] <= sb[gi.STAT_PRIMS]
    return d, int(sa[gi.STAT_PRIMS]), int(sb[gi.STAT_PRIMS])


def _cornell(light=None, **kw):
    sc = S.cornell_scene()
    if light is not None:
        sc.light = tuple(float(v) for v in light)
    for k, v in kw.items():
        setattr(sc, k, v)
    return sc


def _ceiling_delta(d, cam_pos):
    """The least distance below the Cornell box's ceiling (z = 5) at which a light over the room's middle leaves
    the ceiling's leaf dead, bisected on the accessor; and that leaf's bit."""
    _, far = d.shadow_leaves((5.0, 0.0, 4.0), cam_pos)
    _, on = d.shadow_leaves((5.0, 0.0, 5.0), cam_pos)
    bit = on & ~far
    assert bit != 0 and bit & (bit - 1) == 0   # one leaf comes alive as the light reaches the ceiling
    lo, hi = 0.0, 1.0
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        if d.shadow_leaves((5.0, 0.0, 5.0 - mid), cam_pos)[1] & bit:
            lo = mid
        else:
            hi = mid
    return hi, bit


def test_cornell_own_light(torch_cuda):
    """The Cornell box under its own light: seven of the 17 leaves are boundary leaves (five walls, two block
    bottoms) and all seven are dead; the frame is the full table's and the oracle's, with fewer exact tests (the
    shadow rays that start inside a neighbouring wall's padded box no longer test that wall)."""
    sc = _cornell()
    d, pa, pb = _check(torch_cuda, sc, 96, 64, 4, 4)
    bnd, live = d.shadow_leaves(sc.light, sc.cam_pos)
    assert bin(bnd).count("1") == 7 and live == ((1 << 17) - 1) & ~bnd
    assert pa < pb


def test_cornell_light_at_the_bound(torch_cuda):
    """Lights just inside and just outside the bound delta below the ceiling: the accessor's masks differ in
    the ceiling's leaf alone, delta is of the order the derivation gives (1e-3 .. 0.5, against the own light's
    0.5), and both frames are the full table's and the oracle's."""
    d0 = gi.DeviceScene.from_scene(_cornell())
    cam = _cornell().cam_pos
    delta, bit = _ceiling_delta(d0, cam)
    print("delta below the ceiling:", delta)
    assert 1e-3 < delta < 0.5
    masks = []
    for f in (0.99, 1.01):
        sc = _cornell((5.0, 0.0, 5.0 - f * delta))
        d, _, _ = _check(torch_cuda, sc, 64, 48, 2, 3)
        masks.append(d.shadow_leaves(sc.light, sc.cam_pos)[1])
    assert masks[0] ^ masks[1] == bit and masks[0] & bit


def test_cornell_light_on_a_wall_plane(torch_cuda):
    """A light exactly in the ceiling's plane: that leaf is visited; the frame is the full table's and the oracle's."""
    sc = _cornell((5.0, 0.0, 5.0))
    d, _, _ = _check(torch_cuda, sc, 64, 48, 2, 3)
    bnd, live = d.shadow_leaves(sc.light, sc.cam_pos)
    assert bin(bnd & ~live).count("1") == 6


def test_cornell_light_outside_the_room(torch_cuda):
    """A light above the ceiling: the ceiling stays live and occludes -- the frame is the oracle's, in which the
    room's surfaces get no direct light."""
    sc = _cornell((5.0, 0.0, 7.0))
    d, _, _ = _check(torch_cuda, sc, 64, 48, 2, 3)
    bnd, live = d.shadow_leaves(sc.light, sc.cam_pos)
    assert bin(bnd & ~live).count("1") == 6 and bin(bnd & live).count("1") == 1
    lit = _cornell()
    o_dark = U.oracle_render(sc.to_scn(), 64, 48, mode=1, spp=2, depth=3, seed=SEED)["rgb"]
    o_lit = U.oracle_render(lit.to_scn(), 64, 48, mode=1, spp=2, depth=3, seed=SEED)["rgb"]
    assert o_dark.sum() < 0.5 * o_lit.sum()


def test_camera_into_a_floor_corner(torch_cuda):
    """Every primary ray ends near the corner of the floor, the back wall and a side wall: shadow rays leave
    points next to three dead leaves."""
    sc = _cornell(cam_pos=(1.0, 0.0, 0.0), cam_look=(10.0, -5.0, -5.0), focal=0.05)
    _check(torch_cuda, sc, 64, 48, 4, 4)


def test_walls_only_scene_has_no_live_leaf(torch_cuda):
    """The five walls alone: every leaf is a boundary leaf, every shadow query visits none."""
    sc = _cornell()
    sc.entities = sc.entities[:10]
    sc.name = "walls"
    d, pa, pb = _check(torch_cuda, sc, 64, 48, 2, 4)
    bnd, live = d.shadow_leaves(sc.light, sc.cam_pos)
    n = d.info()["x_flat_leaves"]
    assert bnd == (1 << n) - 1 and live == 0


def _polyhedron():
    """XFLAT_MAX triangles in tangent planes of a sphere, one per leaf (GI_XLEAF_MAX=1): every leaf is a
    boundary leaf, and a light outside the sphere leaves the faces it looks at from behind live."""
    c, r = np.array([5.0, 0.0, 0.0]), 3.0
    tris, dirs = [], []
    for j in range(XFLAT_MAX):
        z = 1.0 - 2.0 * (j + 0.5) / XFLAT_MAX
        ph = j * math.pi * (3.0 - math.sqrt(5.0))
        u = np.array([math.sqrt(1.0 - z * z) * math.cos(ph), math.sqrt(1.0 - z * z) * math.sin(ph), z])
        a = np.cross(u, [0.0, 0.0, 1.0] if abs(u[2]) < 0.9 else [1.0, 0.0, 0.0])
        a /= np.linalg.norm(a)
        b = np.cross(u, a)
        p = c + r * u
        v = [p + 0.5 * (math.cos(t) * a + math.sin(t) * b) for t in (0.3, 0.3 + 2.1, 0.3 + 4.2)]
        tris.append((tuple(tuple(float(x) for x in q) for q in v), (0.3 + 0.02 * j, 0.9 - 0.02 * j, 0.5)))
        dirs.append(u)
    return tri_scene(tris, "polyhedron"), {"GI_XLEAF_MAX": "1"}, c, dirs


def test_full_table_with_first_and_last_leaf_dead(torch_cuda):
    """A table of GI_XFLAT_MAX leaves whose first and last leaves are dead and some between them live, with
    gaps: the candidate mask's shifts before a visited leaf and after the last one."""
    sc, env, c, dirs = _polyhedron()
    d0 = with_env(env, lambda: gi.DeviceScene.from_scene(sc))
    top = 1 << (XFLAT_MAX - 1)
    best = None
    for u in dirs:
        L = tuple(float(x) for x in c + 6.0 * u)
        bnd, live = d0.shadow_leaves(L, sc.cam_pos)
        assert bnd == (1 << XFLAT_MAX) - 1
        if live and not live & 1 and not live & top and (best is None or bin(live).count("1") > bin(best[1]).count("1")):
            best = (L, live)
    assert best is not None and bin(best[1]).count("1") >= 2
    sc.light = best[0]
    _check(torch_cuda, sc, 96, 64, 2, 3, env=env)


def test_box_with_a_sphere(torch_cuda):
    """The Cornell box with a sphere (the kernels of mixed scenes, a table that is not all fan pairs): the walls stay
    boundary leaves, the sphere's box lies on their inner side."""
    sc, env = with_sphere()
    d, pa, pb = _check(torch_cuda, sc, 64, 48, 2, 3, env=env)
    bnd, live = d.shadow_leaves(sc.light, sc.cam_pos)
    assert bin(bnd).count("1") == 7 and bnd & live == 0


def test_wavefront_form(torch_cuda):
    """k_wf_bounce (GI_FLAG_X_WF) passes the same mask to x_segment: at the frame size of test_cornell_own_light
    its exact tests fall as k_seg's do (the few shadow rays that start inside a neighbouring wall's padded box)."""
    _, pa, pb = _check(torch_cuda, _cornell(), 96, 64, 4, 4, flags=gi.FLAG_X_WF, form="k_wf_bounce")
    assert pa < pb


def test_far_camera_keeps_every_leaf(torch_cuda):
    """A camera farther out than 16 scene extents: the mask is full (the bound does not budget the rounding of
    its hit points), the frame the oracle's."""
    sc = _cornell(cam_pos=(-200.0, 0.0, 0.0), focal=0.2)
    d, pa, pb = _check(torch_cuda, sc, 48, 40, 2, 3)
    bnd, live = d.shadow_leaves(sc.light, sc.cam_pos)
    assert bin(bnd).count("1") == 7 and live == (1 << 17) - 1
    assert pa == pb


def test_ring_off(torch_cuda, tmp_path):
    """k_seg without its ring (GI_SEG_RING=0, read once per process: a child process) with the mask and with
    every leaf: both the frame this process renders with the ring."""
    sc = _cornell()
    scn = tmp_path / "cornell.scn"
    scn.write_text(sc.to_scn())
    out = tmp_path / "direct.npz"
    code = ("import sys, numpy as np; sys.path.insert(0, %r); sys.path.insert(0, %r); import oracle_util as U; "
            "gi = U.pkg(); S = U.scenes(); sc = S.parse_scn(open(%r).read()); d = gi.DeviceScene.from_scene(sc)\n"
            "assert d.x_form(spp=2, depth=3) == 'k_seg' and not d.seg_ring(spp=2, depth=3)\n"
            "cam = gi.Camera(sc.cam_pos, sc.cam_look, sc.focal)\n"
            "a = d.render(cam, sc.light, 64, 48, mode=gi.MODE_X, spp=2, depth=3, seed=%d)[0]\n"
            "b = d.render(cam, sc.light, 64, 48, mode=gi.MODE_X, spp=2, depth=3, seed=%d, flags=gi.FLAG_X_ALL_LEAVES)[0]\n"
            "np.savez(%r, a=a, b=b)") % (U.ROOT, os.path.join(U.ROOT, "tests"), str(scn), SEED, SEED, str(out))
    subprocess.run([sys.executable, "-c", code], check=True, timeout=300, env=dict(os.environ, GI_SEG_RING="0"))
    r = np.load(out)
    d = gi.DeviceScene.from_scene(sc)
    rgb, _, _ = _render(torch_cuda, d, sc, 64, 48, 2, 3, 0)
    assert U.bits_equal(r["a"].reshape(-1, 3), rgb).all() and U.bits_equal(r["b"].reshape(-1, 3), rgb).all()
