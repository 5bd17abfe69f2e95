"""Frames and expected answers of the feature-buffer tests (gi_render_aov, gi_camera_rays), judged on the
oracle alone.  Host code only (numpy, the CPU oracle); a helper, not a test.

A frame is (scene, focal, w, h[, camera position]): small, no multiple of 8 or 64 in either direction,
with hits and misses.  Its reference, built once and read-only:
  rays        the pixel rays restated in numpy with glm's operation order (the oracle's camera);
  hit, uv     gio_render's primary hit entity and texture coordinate per pixel (mode 1, 1 spp, depth 1);
  rgb         that frame's radiance (the albedo tests: materials of shader (1, 0, 0));
  prim, t     gio_x_query's brute-force closest hit of the rays (the oracle's BVH for the 31089-triangle soup).
Nothing here carries a tolerance.
"""
import copy

import numpy as np

import oracle_util as U
from x_scenes import QUERY_SCENES

S = U.scenes()
RAY_DOUBLES = 8
RES = 0.0002   # the reference's pixel pitch (raytracer.h:28-29)

# key -> (scene, focal, w, h, camera position or None: the scene's)
FRAMES = {
    "cornell/0.004": ("cornell", 0.004, 37, 21, None),
    "cornell/0.01": ("cornell", 0.01, 64, 40, None),
    "cornell_sphere/0.004": ("cornell_sphere", 0.004, 37, 21, None),
    "cornell_sphere/0.01": ("cornell_sphere", 0.01, 64, 40, None),
    "soup_max_plus_1": ("soup_max_plus_1", 0.01, 37, 21, None),
    "corner3_octree": ("corner3_octree", 0.01, 37, 21, None),
    "soup1000": ("soup1000", 0.01, 37, 21, None),
    "soup_xcnode": ("soup_xcnode", 0.004, 37, 21, None),
    "zoo": ("zoo", 0.01, 37, 21, None),
    "one_triangle": ("one_triangle", 0.01, 37, 21, None),
    "coincident": ("coincident", 0.01, 37, 21, None),
    "three_record_leaves": ("three_record_leaves", 0.1, 37, 21, None),
    "main": ("main", 0.01, 37, 21, None),
    "empty": ("empty", 0.01, 37, 21, None),
    # more than x_far_r = 16 extents out: the launch-uniform far-camera rule
    "cornell/far": ("cornell", 0.5, 37, 21, (-1000.0, 0.0, 0.0)),
}
ODD_WINDOW = (5, 3, 30, 20)   # x 5..30, y 3..20 of a 37 x 21 frame
# the albedo frames: every entity's material set to shader (1, 0, 0), colours from {0, 1}^3
ALBEDO_SCENES = ("cornell", "zoo", "cornell_sphere")
ALBEDO_FOCAL = {"cornell": 0.004, "zoo": 0.01, "cornell_sphere": 0.004}   # (the table's focal of each at 37 x 21)
ALBEDO_COLOURS = [(1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (1.0, 1.0, 0.0), (0.0, 0.0, 1.0), (0.0, 1.0, 1.0)]
ALBEDO_FRAME = (37, 21)

_cache = {}


def _frozen(key, make):
    if key not in _cache:
        out = make()
        for a in out.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def base_scene(name):
    """(scene, env) of a frame's scene: the ray-level query tests' builders, and main."""
    if name in QUERY_SCENES:
        return QUERY_SCENES[name][0]()
    return S.named_scene(name), {}


def frame_scene(key):
    """(scene with the frame's focal and camera, env, w, h)."""
    name, focal, w, h, pos = FRAMES[key]
    sc, env = base_scene(name)
    sc = copy.deepcopy(sc)
    sc.focal = focal
    if pos is not None:
        sc.cam_pos = pos
    return sc, env, w, h


def albedo_scene(name):
    """(scene, env, w, h): every entity's material replaced by one of shader (1, 0, 0) -- ambient x 1,
    diffuse x 0, specular x 0 -- so the depth-1 frame is min(texel, 1) exactly."""
    sc, env = base_scene(name)
    sc = copy.deepcopy(sc)
    sc.focal = ALBEDO_FOCAL[name]
    for k, e in enumerate(sc.entities):
        e.material = S.Material(ALBEDO_COLOURS[k % len(ALBEDO_COLOURS)], (1.0, 0.0, 0.0))
    return sc, env, ALBEDO_FRAME[0], ALBEDO_FRAME[1]


def _norm(v):
    """glm::normalize: v * (1 / sqrt(dot(v, v))), the dot summed as (x x + y y) + z z."""
    return v * (1.0 / np.sqrt((v[..., 0:1] * v[..., 0:1] + v[..., 1:2] * v[..., 1:2]) + v[..., 2:3] * v[..., 2:3]))


def rays_np(sc, w, h, window=None):
    """The window's pixel rays as (rows * cols, 8) records, row-major: raytracer.h:26-30, 41-43 in fp64 with
    glm's operation order (tests/test_capi.py _primary_dirs), normalised as the oracle's Ray does."""
    x0, y0, x1, y1 = window if window is not None else (0, 0, w, h)
    pos = np.array(sc.cam_pos, np.float64)
    f = _norm(np.array(sc.cam_look, np.float64) - pos)
    up = np.array([0.0, 0.0, 1.0])
    left = _norm(np.array([up[1] * f[2] - f[1] * up[2], up[2] * f[0] - f[2] * up[0], up[0] * f[1] - f[0] * up[1]]))
    tl = (((pos + sc.focal * f) + ((left * float(w)) * 0.5) * RES) + ((up * float(w)) * 0.5) * RES) - pos
    y, x = np.mgrid[y0:y1, x0:x1]
    x, y = x.reshape(-1, 1).astype(np.float64), y.reshape(-1, 1).astype(np.float64)
    d = _norm((tl - (left * x) * RES) - (up * y) * RES)
    rays = np.zeros((len(d), RAY_DOUBLES))
    rays[:, 0:3], rays[:, 3:6], rays[:, 6] = pos, d, np.inf
    return np.ascontiguousarray(rays)


def texel_np(col, u, v):
    """Material's 32 x 32 checker (gi_math.h texel) of colours col (n, 3) at (u, v): white, or the truncated colour."""
    u, v = u.astype(np.int64), v.astype(np.int64)
    f = np.fmod(u, 32) * 32 + np.fmod(v, 32)
    f = np.where((f < 0) | (f >= 1024), np.fmod(np.fmod(f, 1024) + 1024, 1024), f)
    i, j = f >> 5, f & 31
    white = ((i <= 16) & (j <= 16)) | ((i > 16) & (j > 16))
    return np.where(white[:, None], 1.0, np.trunc(col))


def _x_query(sc, rays, bvh):
    n = len(rays)
    recs = np.concatenate([rays[:, 0:6], np.tile(np.array(sc.light, np.float64), (n, 1)), rays[:, 3:6]], 1)
    U.oracle_accel(1 if bvh else 0)
    try:
        return U.oracle_x_query(sc.to_scn(), recs)
    finally:
        U.oracle_accel(-1)


def _reference(sc, w, h, bvh=False):
    o = U.oracle_render(sc.to_scn(), w, h, mode=1, spp=1, depth=1)
    rays = rays_np(sc, w, h)
    q = _x_query(sc, rays, bvh)
    return dict(rays=rays, hit=o["hit"], uv=o["uv"], rgb=o["rgb"], prim=q["prim1"], t=q["t1"])


def reference(key):
    """The frame's reference planes, each (h * w[, k]) row-major."""
    def make():
        sc, _, w, h = frame_scene(key)
        return _reference(sc, w, h, bvh=FRAMES[key][0] == "soup_xcnode")
    return _frozen(("frame", key), make)


def albedo_reference(name):
    """As reference() for the albedo scene, with `albedo`: the numpy texel of the oracle's own hit and uv
    and the entities' colours ((0, 0, 0) on misses)."""
    def make():
        sc, _, w, h = albedo_scene(name)
        r = _reference(sc, w, h)
        hit = r["hit"] >= 0
        col = np.array([sc.entities[k].material.color for k in r["hit"][hit]], np.float64).reshape(-1, 3)
        alb = np.zeros((w * h, 3))
        alb[hit] = texel_np(col, r["uv"][hit, 0], r["uv"][hit, 1])
        r["albedo"] = alb
        return r
    return _frozen(("albedo", name), make)


def window_of(a, w, h, window):
    """The window's rectangle of a whole-frame plane (h * w[, k]) as (rows, cols[, k])."""
    x0, y0, x1, y1 = window
    return np.ascontiguousarray(a.reshape((h, w) + a.shape[1:])[y0:y1, x0:x1])
