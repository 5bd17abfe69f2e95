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


# ---- scenes at other scales and away from the origin (tests/test_x_placed_host.py, tests/test_gpu_x_placed.py) ----
# The largest |bound| of a Mode X structure gi_scene_create accepts (gi_scene.h; gi_dev.h inv_dir derives it)
X_COORD_MAX = float(re.search(r"constexpr double GI_X_COORD_MAX = ([0-9.e+]+);",
                              open(os.path.join(U.ROOT, "2019global_amd", "csrc", "gi_scene.h")).read()).group(1))


def placed(scene, s, off, name=None):
    """A copy of a scene of ImpTriangles and ImpSpheres under x -> s x + off: every vertex, sphere centre,
    the camera's position and look-at point, the light and the octree bounds mapped, sphere radii times
    s, the focal length and the materials as they are.  Other entity kinds are refused."""
    off = np.asarray(off, np.float64)
    s = float(s)

    def m(p):
        return tuple(float(v) for v in s * np.asarray(p, np.float64) + off)

    out = S.Scene(octree_min=m(scene.octree_min), octree_max=m(scene.octree_max), cam_pos=m(scene.cam_pos),
                  cam_look=m(scene.cam_look), focal=scene.focal, light=m(scene.light), entities=[],
                  name=name or "%s@%gx+(%g,%g,%g)" % (scene.name, s, *off))
    for e in scene.entities:
        if e.kind == S.IMP_TRIANGLE:
            args = m(e.args[0:3]) + m(e.args[3:6]) + m(e.args[6:9])
        elif e.kind == S.IMP_SPHERE:
            args = m(e.args[0:3]) + (e.args[3] * s,) + tuple(e.args[4:])
        else:
            raise ValueError("placed(): entity kind %d is neither an ImpTriangle nor an ImpSphere" % e.kind)
        out.entities.append(S.Entity(e.kind, args, e.material))
    return out


def _limit_scale():
    """The largest power-of-two scale at which the Cornell box's structure (max |coordinate| 10, padded
    by 1e-5 of it and rounded outward to fp32) stays within X_COORD_MAX."""
    k = 0
    while float(np.nextafter(np.float32(10.0 * (1.0 + 1e-5) * 2.0 ** (k + 1)), np.float32(np.inf))) <= X_COORD_MAX:
        k += 1
    return 2.0 ** k


# name -> (s, off): power-of-two scales and dyadic offsets, so the Cornell box's coordinates stay exact
PLACEMENTS = {
    "x2^-10": (2.0 ** -10, (0.0, 0.0, 0.0)),            # the max(1, ...) floor of the builder's extent
    "x2^10": (2.0 ** 10, (0.0, 0.0, 0.0)),              # an own-plane skip bound near 0.3
    "x2^20": (2.0 ** 20, (0.0, 0.0, 0.0)),              # the bound above 1, no dead leaf: no shortcut left
    "off2^13": (1.0, (8192.0, -4096.0, 2048.0)),
    "off2^20": (1.0, (2.0 ** 20, 2.0 ** 20, -2.0 ** 20)),   # padding as large as the scene
    "x2^-10_off2^7": (2.0 ** -10, (128.0, 128.0, -128.0)),  # a small scene 1e4 of its size from the origin
    "at_limit": (_limit_scale(), (0.0, 0.0, 0.0)),      # just inside the fp32 box tests' limit (2^25)
    "beyond_limit": (2.0 * _limit_scale(), (0.0, 0.0, 0.0)),   # just outside: gi_scene_create refuses it
}
INSIDE = tuple(p for p in PLACEMENTS if p != "beyond_limit")
PLACED_N = 1024 + 37   # rays per placed set
# the base scenes placed everywhere, and the one whose build is slow at two placements only
PLACED_BASES = ("cornell", "cornell_sphere", "grazing_tilted", "corner3_octree", "soup1000")
PLACED_CASES = [(b, p) for b in PLACED_BASES for p in INSIDE] + [("soup_xcnode", "off2^13"), ("soup_xcnode", "x2^20")]
# Sets whose farther class (far_1e6, 1e3 E from the world origin by default) starts 32 E out like the
# nearer one, because at 1e3 E the oracle's BVH and its brute force disagree on the sphere (phantom
# roots of the quadratic, x_rays.Frame): found by tests/test_x_placed_host.py, which checks every set.
# At 1e3 E brute force answers the sphere where the BVH does not on 8 of the first set's 66 far_1e6 rays and on 1 of
# the second's.
FAR_MOVED_IN = (("cornell_sphere", "off2^20"), ("cornell_sphere", "x2^-10_off2^7"))


def placed_scene(base, placement):
    """(scene, env) of a base query scene at a placement."""
    sc, env = QUERY_SCENES[base][0]()
    s, off = PLACEMENTS[placement]
    return placed(sc, s, off, "%s@%s" % (sc.name, placement)), env


def placed_frame(base, placement):
    import x_rays as R
    s, off = PLACEMENTS[placement]
    far = dict(R.PLACED_FAR)
    if (base, placement) in FAR_MOVED_IN:
        far["far_1e6"] = far["far_1e3"]
    return R.Frame(s, off, far, R.PLACED_SHARE)


def placed_skip_standin(sc):
    """Stand-in for the device's skip_cos of a placed scene: every term of the builder's bound but tau
    grows with E = max |coordinate|, so the base stand-in (E = 10) times E / 10, E floored at 1."""
    import x_rays as R
    return STANDIN_SKIP_COS * max(1.0, R.Geo(sc).ext) / 10.0


def placed_set(base, placement, skip_cos=None):
    """(scene, env, ray set, brute-force reference, frame) of a base scene at a placement, as query_set:
    built once per (scene, placement, skip_cos), read-only afterwards."""
    import x_rays as R
    sc, env = placed_scene(base, placement)
    if skip_cos is None:
        skip_cos = placed_skip_standin(sc)
    key = (base, placement, skip_cos)
    if key not in _sets:
        frame = placed_frame(base, placement)
        scn = sc.to_scn()
        U.oracle_accel(0)
        try:
            rs = R.ray_set(sc, PLACED_N, skip_cos, 2019, lambda recs: U.oracle_x_query(scn, recs), frame)
            ref = U.oracle_x_query(scn, rs["recs"])
        finally:
            U.oracle_accel(-1)
        for a in list(rs.values()) + list(ref.values()):
            a.setflags(write=False)
        _sets[key] = (sc, env, rs, ref, frame)
    return _sets[key]


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
