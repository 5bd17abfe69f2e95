"""Scene builders shared by the Mode X GPU tests (flat leaf query, ray-level query KAT, parity): small
scenes at the edges of the flat leaf table's eligibility and the grazing-light scenes.  Pure host
code (no device).  A builder returns (scene, env): env holds the builder knobs (read when the device
scene is created) the case needs."""
import os
import re

import numpy as np

import oracle_util as U

S = U.scenes()
XFLAT_MAX = int(re.search(r"#define GI_XFLAT_MAX (\d+)",
                          open(os.path.join(U.ROOT, "2019global_amd", "csrc", "gi_scene.h")).read()).group(1))


def with_env(env, make):
    """make() with the environment variables of env set (the scene builder reads its knobs there)."""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return make()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def tri_scene(tris, name):
    s = S.Scene()
    s.name = name
    for t, col in tris:
        s.imp_triangle(*t, col)
    return s


def one_triangle():
    return tri_scene([(((2.0, -3.0, -3.0), (2.0, 4.0, -2.0), (3.0, 0.0, 4.0)), (0.9, 0.6, 0.2))], "one_triangle"), {}


def empty():
    s = S.Scene()
    s.name = "empty"
    return s, {}


def soup(n):
    # single-primitive leaves (GI_XLEAF_MAX=1, read when the scene is built): n triangles, n leaves --
    # rows of eight small tilted triangles in front of the camera
    tris = []
    for i in range(n):
        x, y, z = 3.0 + 0.1 * (i % 3), -3.5 + (i % 8), -2.0 + (i // 8)
        tris.append((((x, y - 0.4, z - 0.4), (x, y + 0.4, z - 0.4), (x + 0.2, y, z + 0.4)),
                     (0.2 + 0.1 * (i % 8), 0.9 - 0.1 * (i % 7), 0.5)))
    return tri_scene(tris, "soup%d" % n), {"GI_XLEAF_MAX": "1"}


def three_record_leaves():
    # four stacks of three parallel triangles: a stack's boxes coincide, so the builder keeps each as one
    # leaf of three records (the pair loop's odd tail)
    tris = []
    # (close to the view axis: a 32 x 32 frame sees about +-0.4 around it at this distance)
    for i, (y, z) in enumerate(((-0.3, -0.3), (0.3, -0.3), (-0.3, 0.3), (0.3, 0.3))):
        for j in range(3):
            x = 3.0 + 2.0 * i + 0.01 * j
            tris.append((((x, y - 0.3, z - 0.3), (x, y + 0.3, z - 0.3), (x, y, z + 0.3)),
                         (0.3 + 0.3 * j, 0.9 - 0.3 * j, 0.5)))
    return tri_scene(tris, "stacks"), {}


def with_sphere():
    s = S.cornell_scene()
    s.name = "cornell_sphere"
    s.imp_sphere((4.0, 0.5, -1.0), 1.2, (0.8, 0.8, 0.3))
    return s, {}


def coincident_quads():
    """Two coincident quads (every triangle duplicated, in another colour): each hit has two primitives
    at the same t."""
    q = [(3.0, -3.0, -3.0), (3.0, 3.0, -3.0), (3.5, 3.0, 3.0), (3.5, -3.0, 3.0)]
    tris = []
    for col in ((0.9, 0.2, 0.2), (0.2, 0.9, 0.2)):
        tris.append(((q[0], q[1], q[2]), col))
        tris.append(((q[0], q[2], q[3]), col))
    return tri_scene(tris, "coincident"), {}


def corner3_octree():
    """Three large triangles meeting in one vertex, over the SAT octree with leaves of at most two
    (GI_XACCEL=octree, GI_XLEAF_MAX=2): the cell that holds the vertex holds all three at every level,
    so the tree reaches the builder's 12 levels (the tree walk's two-word level masks) while the scene
    stays small enough for LDS (23 wide nodes, 75 leaf records).  The Cornell box over the octree is
    as deep, but its 2014 leaf records do not fit."""
    c = (4.1, 0.3, -0.7)
    tris = [((c, (7.3, 3.1, -0.2), (7.9, -2.7, 0.4)), (0.9, 0.4, 0.3)),
            ((c, (3.7, 3.3, 2.9), (4.6, -2.2, 3.4)), (0.3, 0.9, 0.4)),
            ((c, (1.2, -0.4, -3.6), (6.8, 0.9, -3.9)), (0.3, 0.4, 0.9))]
    return tri_scene(tris, "corner3"), {"GI_XACCEL": "octree", "GI_XLEAF_MAX": "2"}


def grazing_scene(light_mode: str):
    """The Cornell box plus two tilted quads (coplanar pairs on oblique planes), with the light put
    almost into a surface's plane: "floor" 1e-9 above the floor (z = -5), "tilted" 1e-9 off the first
    tilted quad's plane.  Shadow rays from that surface then leave it at an incidence ~1e-10, far
    below the own-plane skip's bound, and must be traced unskipped."""
    s = S.cornell_scene()
    s.name = "grazing_" + light_mode
    rng = np.random.default_rng(11)
    centres = [np.array([4.0, 1.5, 0.5]), np.array([3.0, -2.0, 2.5])]
    planes = []
    for c in centres:
        u = rng.normal(size=3); u /= np.linalg.norm(u)
        v = np.cross(u, rng.normal(size=3)); v /= np.linalg.norm(v)
        q = [c - u - v, c + u - v, c + u + v, c - u + v]
        s.imp_triangle(tuple(q[0]), tuple(q[1]), tuple(q[2]), (1, 1, 1))
        s.imp_triangle(tuple(q[0]), tuple(q[2]), tuple(q[3]), (1, 1, 1))
        planes.append((c, np.cross(u, v)))
    if light_mode == "floor":
        s.light = (5.0, 0.5, -5.0 + 1e-9)
    else:
        c, n = planes[0]
        w = np.cross(n, [0.0, 0.0, 1.0]); w /= np.linalg.norm(w)
        s.light = tuple(c + 1.7 * w + 1e-9 * n)
    return s


# ---- the ray-level query tests' scenes (tests/test_x_query_oracle.py, tests/test_gpu_x_query.py) -------
# The smallest soup_scene(n) the device traverses through quantised nodes (XCNode): gi_capi.cpp takes
# them when the XWNode tree exceeds 2 MB, 8192 nodes of 256 bytes; the host builder gives
# soup_scene(31088) exactly 8192 wide nodes and soup_scene(31089) 8194 (bisected over n on the CPU with
# tests/cpp/xaccel_check.cpp, which prints the node count of a scene file).
XCNODE_SOUP_N = 31089
# Stand-in for the device's skip_cos (the own-plane skip's bound on |d . n|) where no device is at
# hand.  The host builder's bound for the Cornell box is 3.03e-4 + 5.37e-6 max|cam| (printed by
# tests/cpp/xaccel_check.cpp), 3.6e-4 for its own camera at (-10, 0, 0) -- not the 1e-9 first assumed
# for it, which lies five orders of magnitude below.  The GPU test checks the stand-in against the
# device's value for the Cornell box to within a factor of 10.
STANDIN_SKIP_COS = 3.6e-4


def _named(name):
    return lambda: (S.named_scene(name), {})


# name -> (builder, rays): ray counts are no multiple of the wave's 64 lanes
QUERY_SCENES = {
    "cornell": (_named("cornell"), 4096 + 37),
    "cornell_mirror": (_named("cornell_mirror"), 2048 + 37),
    "grazing_floor": (lambda: (grazing_scene("floor"), {}), 2048 + 37),
    "grazing_tilted": (lambda: (grazing_scene("tilted"), {}), 2048 + 37),
    "soup_max": (lambda: soup(XFLAT_MAX), 2048 + 37),
    "soup_max_plus_1": (lambda: soup(XFLAT_MAX + 1), 2048 + 37),
    "three_record_leaves": (three_record_leaves, 2048 + 37),
    "coincident": (coincident_quads, 2048 + 37),
    "one_triangle": (one_triangle, 1024 + 37),
    "empty": (empty, 256 + 37),
    "cornell_sphere": (with_sphere, 2048 + 37),
    "corner3_octree": (corner3_octree, 1024 + 37),
    "soup1000": (_named("soup1000"), 2048 + 37),
    "zoo": (_named("zoo"), 2048 + 37),
    "soup_xcnode": (_named("soup%d" % XCNODE_SOUP_N), 1024 + 37),
}
# scenes whose triangles share edges or coincide (the tie counts are summed over these)
TIE_SCENES = ("cornell", "cornell_mirror", "grazing_floor", "grazing_tilted", "coincident", "cornell_sphere",
              "corner3_octree")
# scenes in which a surface point can be shadowed by other geometry often enough to ask for 10 % of
# each shadow answer; a single plane (one_triangle, coincident) never shadows its own points, and in the
# sparse soups and stacks a shadow ray rarely meets a second triangle
SHADOW_SCENES = ("cornell", "cornell_mirror", "grazing_floor", "grazing_tilted", "cornell_sphere")

_sets = {}


def query_set(name, skip_cos=STANDIN_SKIP_COS):
    """(scene, env, ray set, brute-force reference) of a query scene, built once per (scene, skip_cos)
    and shared by the tests; nothing of it is modified afterwards."""
    import x_rays as R
    key = (name, skip_cos)
    if key not in _sets:
        make, n = QUERY_SCENES[name]
        sc, env = make()
        scn = sc.to_scn()
        U.oracle_accel(0)
        try:
            rs = R.ray_set(sc, n, skip_cos, 2019, lambda recs: U.oracle_x_query(scn, recs))
            ref = U.oracle_x_query(scn, rs["recs"])
        finally:
            U.oracle_accel(-1)
        for a in list(rs.values()) + list(ref.values()):
            a.setflags(write=False)
        _sets[key] = (sc, env, rs, ref)
    return _sets[key]
