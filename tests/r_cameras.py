"""Camera placements of the Mode R tests away from Scene's default camera ((-10, 0, 0) looking at
(1, 0, 0)), the scene copies that carry them, and their references on the CPU oracle.  Host code only
(numpy, the CPU oracle); a helper, not a test.

Every frame is W x H = 40 x 28: five tile columns and three and a half tile rows, so the last tile row
is ragged.  A placement is (name, position, look-at, focal).  The reference's camera keeps
up = (0, 0, 1) and never makes it orthogonal to forward (camera.h:8-10), so a camera that looks up or
down has a sheared image plane; a forward parallel to up gives left = normalize(0) and NaN rays, and
no placement here has one.  The reference's intersection tests carry no t > 0: the
geometry BEHIND a camera is rendered, point-mirrored, and the `behind` placements see nothing else.

What the placements are chosen for (tests/test_mode_r_cameras_host.py asserts it on the oracle):
  * every cornell frame sees geometry in >= 45 % of its pixels, every other frame in >= 5 %;
  * every soup frame shows >= 50 distinct entities;
  * per scene, each of the 8 sign patterns of the centre pixel's direction occurs (the device's slab
    tests choose near / far planes and the sign of the tau widening by them);
  * per scene, at least one frame whose hits all lie on the backward half-line;
  * no frame has a NaN or a texel-UB pixel in the reference.
"""
import copy
import json
import os
import sys

import numpy as np

import oracle_util as U

if U.ROOT not in sys.path:   # (run as a script by the route tests' child processes: the package's directory)
    sys.path.insert(0, U.ROOT)
S = U.scenes()
W, H = 40, 28
F = W * 1e-4     # focal of a 90 degree wide frame at the reference's pixel pitch of 0.0002
RES = 0.0002     # raytracer.h:28-29

# The Cornell box is x in [0, 10], y and z in [-5, 5], open toward -x.
CORNELL = [
    ("centre+x", (5, 0, 0), (6, 0, 0), F),
    ("centre-x", (5, 0, 0), (4, 0, 0), F / 2),
    ("centre+y", (5, 0, 0), (5, 1, 0), F),
    ("centre-y", (5, 0, 0), (5, -1, 0), F),
    ("oblique_a", (5, 0, 0), (6, 1, 0.5), F),
    ("oblique_b", (5, 0, 0), (5.7, -1, -0.7), F),
    ("on_wall_plane", (4, 5, 1), (6, -5, -1), F),
    ("outside_corner", (-0.1, -5.1, -5.1), (10, 5, 5), F),
    ("behind", (25, 0.5, 0.25), (26, 0.5, 0.3), 5 * F),
    ("steep_down", (3, 0.5, 30), (3.5, 0.6, 0), 6 * F),
    ("far_1e3", (-1000, 0, 0), (5, 0, 0), 200 * F),
    ("far_1e5", (-1e5, 3e4, 2e4), (3, 0, 0), 2e4 * F),
    # the sign patterns with d.x < 0 that the twelve above leave out, from the box's far corners
    ("corner_mmm", (9, 4, 4), (0, -5, -5), F),
    ("corner_mpm", (9, -4, 4), (0, 5, -5), F),
    ("corner_mmp", (9, 4, -4), (0, -5, 5), F),
]


def _around(c, r, fm=1.0):
    """The placements every scene gets, around its geometry's centre c at distance r with focal fm * F:
    the axis views (exact zeros in the direction), the eight oblique octants, steep views down and up,
    a camera past the geometry that looks away from it, and one 1000 units out."""
    c = np.array(c, np.float64)
    f = fm * F
    out = [("minus_x", c + (r, 0, 0), c, f), ("plus_y", c - (0, r, 0), c, f), ("minus_y", c + (0, r, 0), c, f)]
    for sx in (1, -1):
        for sy in (1, -1):
            for sz in (1, -1):
                name = "oct_" + "".join("p" if s > 0 else "m" for s in (sx, sy, sz))
                out.append((name, c - r * np.array([0.8 * sx, 0.55 * sy, 0.45 * sz]), c, f))
    out.append(("steep_down", c + (0.25 * r, 0.1 * r, 1.1 * r), c, f))
    out.append(("steep_up", c + (-0.2 * r, 0.15 * r, -1.1 * r), c, f))
    p = c + 2.5 * r * np.array([1.0, 0.05, 0.02])
    out.append(("behind", p, p + (1, 0, 0.05), 3 * f))
    out.append(("far_1e3", c + 1000 * np.array([-1.0, 0.3, 0.2]), c, 1000.0 / r * f))
    return [(n, tuple(float(v) for v in p), tuple(float(v) for v in l), float(f)) for n, p, l, f in out]


# The reference octree keeps about a third of the 1000-triangle soup reachable, so a line through the
# whole cloud meets a triangle in about one pixel of 25 whatever the zoom: these placements of the same
# kinds as _around's are the best of a seeded random search on the oracle for the seen share and the
# entity count (>= 5 %, >= 50), rounded to two decimals.
SOUP1000 = [
    ("minus_x", (18.34, 0.17, -1.21), (4.37, 0.17, -1.21), 0.009405),
    ("plus_y", (3.3, -10.34, 0.16), (3.3, 1.85, 0.16), 0.01341),
    ("minus_y", (5.05, 9.31, -0.43), (5.05, -0.96, -0.43), 0.00821),
    ("oct_ppp", (0.88, -3.5, -10.92), (6.72, 1.17, -0.45), 0.01031),
    ("oct_ppm", (-1.05, -10.23, 6.22), (3.82, -0.79, -0.15), 0.01518),
    ("oct_pmp", (-1.68, 5.0, -5.59), (4.61, 1.29, -0.38), 0.007858),
    ("oct_pmm", (-2.11, 6.53, 8.4), (4.51, -0.9, -1.05), 0.01536),
    ("oct_mpp", (14.26, -5.5, -7.6), (6.63, 0.7, -1.53), 0.01007),
    ("oct_mpm", (12.78, -6.63, 5.13), (4.18, 1.89, -0.06), 0.01712),
    ("oct_mmp", (13.75, 10.1, -6.77), (5.05, 1.01, -1.29), 0.01789),
    ("oct_mmm", (9.49, 7.75, 5.92), (4.01, 1.28, -1.22), 0.00827),
    ("steep_down", (11.05, -3.3, 14.32), (5.02, 0.21, 1.98), 0.01471),
    ("steep_up", (6.99, 6.25, -12.5), (3.2, 1.29, 0.78), 0.009782),
    ("behind", (-9.82, 7.27, 7.05), (-10.64, 7.67, 7.45), 0.02052),
    ("far_1e3", (-996.63, -342.08, 35.7), (3.37, -1.5, -1.22), 1.53),
    ("inside", (3.52, -0.12, 0.78), (2.41, -2.48, 1.79), 0.004306),
]

CAMERAS = {
    "cornell": [(n, tuple(map(float, p)), tuple(map(float, l)), float(f)) for n, p, l, f in CORNELL],
    # every entity kind in the scene, but the reference's octree keeps only the ExpRectangle and the ExpBox
    # reachable (entities 6 and 7, as in the default camera's golden): the views circle those two; `inside`: in
    # the ExpSphere at (-2, 0, 0), which no ray's candidate list holds
    "zoo": _around((2, 0, -2.5), 8) + [("inside", (-2.0, 0.3, 0.2), (1.0, 0.5, 0.0), F)],
    # an ExpQuad at the origin and two ImpSpheres (the r_always list); `inside`: in the sphere at (3, 4, 4)
    "main": _around((2.5, 0, 3), 9) + [("inside", (3.0, 4.0, 4.5), (0.0, 0.0, 0.0), F)],
    "soup1000": SOUP1000,
    # just over the 4096 entities from which the flat phases (k_rf_walk) are the default route; `tele_diag`
    # is a narrow view along a diagonal of the soup's cube (see OVERFLOW_PLACEMENT)
    "soup4100": _around((5, 0, 0), 11, 2.0) + [("inside", (5.0, 0.1, 0.2), (9.0, 3.0, -2.0), 0.6 * F),
                                               ("tele_diag", (23.52, -14.67, 18.39), (5.11, 1.31, -1.12), 0.1202),
                                               # tau = 1e-5 (max|pos| + extent) is 0.1 here, half a triangle's box
                                               ("far_1e4", (-1e4 + 5, 3e3, 2e3), (5.0, 0.0, 0.0), 1e4 / 11 * 2 * F)],
    # the box (2, 4, -5) .. (4, 6, -3); `inside`: within it; `on_face`: on the plane of its face y = 4
    "only_expbox": _around((3, 5, -4), 2.6) + [("inside", (3.0, 5.0, -4.0), (4.0, 6.5, -3.2), F),
                                               ("on_face", (1.0, 4.0, -4.5), (4.0, 6.0, -3.5), F)],
}
SCENES = tuple(CAMERAS)
FRAMES = [(scene, p[0]) for scene in SCENES for p in CAMERAS[scene]]
SOUPS = ("soup1000", "soup4100")
# The soup4100 frame whose tiles split under GI_RF_PER_SLOT=0 (no pool: a tile keeps the 512 candidate
# pairs it owns).  A pair is an (entity, pixel) whose line crosses the entity's bounding box, about 3 to 10
# a pixel through this soup however the camera stands, so only tiles whose 64 lines all run the cube's
# long way collect more than 512: found by a seeded search on the host's lower bound of the pairs
# (test_mode_r_cameras_host.py restates it), which puts four tiles over 512 and others under 150.
OVERFLOW_PLACEMENT = "tele_diag"
# (d) of the GPU tests: one oblique and one behind placement per scene
SHARD_PLACEMENTS = {scene: (("oblique_b" if scene == "cornell" else "oct_mpm"), "behind") for scene in SCENES}

_cache = {}


def placement(scene, name):
    for p in CAMERAS[scene]:
        if p[0] == name:
            return p
    raise KeyError((scene, name))


def base_scene(scene):
    if ("scene", scene) not in _cache:
        _cache[("scene", scene)] = S.named_scene(scene)
    return _cache[("scene", scene)]


def scene_at(scene, name):
    """A copy of the scene with the placement's cam_pos, cam_look and focal."""
    _, pos, look, focal = placement(scene, name)
    sc = copy.copy(base_scene(scene))   # (the entities are shared: nothing here changes them)
    sc.cam_pos, sc.cam_look, sc.focal = pos, look, focal
    return sc


def _norm(v):
    """glm::normalize: v * (1 / sqrt(dot(v, v))), the dot summed as (x x + y y) + z z."""
    return v * (1.0 / np.sqrt((v[..., 0:1] * v[..., 0:1] + v[..., 1:2] * v[..., 1:2]) + v[..., 2:3] * v[..., 2:3]))


def primary_dirs(sc, w=W, h=H):
    """The pixels' UNNORMALISED primary directions (h * w, 3), row-major: raytracer.h:26-30, 41-43 in fp64
    with glm's operation order (tests/aov_frames.py rays_np before its normalisation)."""
    pos = np.array(sc.cam_pos, np.float64)
    f = _norm(np.array(sc.cam_look, np.float64) - pos)
    up = np.array([0.0, 0.0, 1.0])
    left = _norm(np.array([up[1] * f[2] - f[1] * up[2], up[2] * f[0] - f[2] * up[0], up[0] * f[1] - f[0] * up[1]]))
    tl = (((pos + sc.focal * f) + ((left * float(w)) * 0.5) * RES) + ((up * float(w)) * 0.5) * RES) - pos
    y, x = np.mgrid[0:h, 0:w]
    x, y = x.reshape(-1, 1).astype(np.float64), y.reshape(-1, 1).astype(np.float64)
    return (tl - (left * x) * RES) - (up * y) * RES


def sign_pattern(d):
    """The sign bits of a direction's components, as the device's iv_signs reads them: bit a set when
    component a is negative."""
    return int(np.signbit(d[0])) | int(np.signbit(d[1])) << 1 | int(np.signbit(d[2])) << 2


def texel_ub_mask(hit, uv):
    """Pixels whose texture lookup reads outside the reference's 32 x 32 array (tests/test_oracle_golden.py)."""
    f = np.fmod(uv[:, 0], 32) * 32 + np.fmod(uv[:, 1], 32)
    return (hit >= 0) & ((f < 0) | (f >= 1024))


def _hit_t(sc, dirs, hit):
    """Per pixel, the ray parameter of the oracle's hit point along the pixel's normalised direction
    (NaN on a miss): negative when the hit lies behind the camera.  gio_rays over the hit pixels'
    rays in chunks, the hit entity's point picked from each."""
    t = np.full(len(hit), np.nan)
    idx = np.nonzero(hit >= 0)[0]
    pos = np.array(sc.cam_pos, np.float64)
    scn = sc.to_scn()
    n_ent = len(sc.entities)
    for k in range(0, len(idx), 128):
        ii = idx[k:k + 128]
        rays = np.concatenate([np.tile(pos, (len(ii), 1)), dirs[ii]], axis=1)
        pn = U.oracle_rays(scn, rays, n_ent)["pn"]
        P = pn[np.arange(len(ii)), hit[ii], 0:3]
        dn = _norm(dirs[ii])
        t[ii] = ((P - pos) * dn).sum(1)
        # an ImpSphere's point is o + min|root| * d / d.x (the oracle's sphere_intersect): not on the
        # sphere where the sign differs.  From outside, both roots of its line have the sign of the
        # closest approach's parameter; from inside there is one on each side (0: neither)
        for j, e in enumerate(hit[ii]):
            ent = sc.entities[e]
            if ent.kind == S.IMP_SPHERE:
                oc = np.array(ent.args[0:3]) - pos
                t[ii[j]] = float(oc @ dn[j]) if float(oc @ oc) > ent.args[3] ** 2 else 0.0
    return t


def oracle_frame(scene, name):
    """The placement's Mode R frame on the CPU oracle, computed once and read-only: gio_render's rgb,
    hit, uv, ncand, nnode, q, plus `dirs` (primary_dirs) and `t` (the hit's ray parameter, NaN on a miss)."""
    key = ("frame", scene, name)
    if key not in _cache:
        sc = scene_at(scene, name)
        o = U.oracle_render(sc.to_scn(), W, H, threads=16)
        o["dirs"] = primary_dirs(sc)
        o["t"] = _hit_t(sc, o["dirs"], o["hit"])
        for a in o.values():
            a.setflags(write=False)
        _cache[key] = o
    return _cache[key]


def golden_path(scene):
    return os.path.join(U.GOLDEN, f"rcam_{scene}.npz")


def load_golden(scene):
    """{placement: dict of the reference's arrays} of tests/golden/rcam_<scene>.npz (make_golden.py
    `cameras`), or None where the fixture is not committed (make_golden.py keeps a file over its size
    limit out)."""
    key = ("golden", scene)
    if key not in _cache:
        if not os.path.exists(golden_path(scene)):
            _cache[key] = None
        else:
            z = np.load(golden_path(scene))
            meta = json.loads(str(z["meta"]))
            out = {"meta": meta}
            for k, name in enumerate(meta["placements"]):
                out[name] = {f: z[f][k] for f in ("pos", "look", "focal", "rgb", "hit", "uv", "ncand", "nnode", "q")}
            _cache[key] = out
    return _cache[key]


def render_all(out_path):
    """Every placement's Mode R frame on the device with this process's settings (the GI_R_FLAT /
    GI_RF_PER_SLOT knobs are read once per process: the route tests run this in child processes), saved
    as an .npz: "<scene>/<name>" the fp64 frame, "<scene>/<name>/q" its RGB888, "<scene>/<name>/stats" the
    GI_FLAG_STATS counters of a second launch of the soups' frames (whose frame must equal the first),
    "<scene>/kernel" gi_scene_r_kernel's name."""
    import torch
    gi = U.pkg()
    res = {}
    for scene in SCENES:
        d = gi.DeviceScene.from_scene(base_scene(scene))
        res[scene + "/kernel"] = np.array(d.r_kernel())
        for name, *_ in CAMERAS[scene]:
            sc = scene_at(scene, name)
            cam = gi.Camera(sc.cam_pos, sc.cam_look, sc.focal)
            rgb, rgb8 = d.render(cam, sc.light, W, H)
            res[f"{scene}/{name}"], res[f"{scene}/{name}/q"] = rgb, rgb8
            if scene in SOUPS:
                st = torch.zeros(gi.STATS_N, dtype=torch.int64, device="cuda")
                buf = torch.zeros(W * H * 3, dtype=torch.float64, device="cuda")
                d.render_device(cam, sc.light, W, H, buf.data_ptr(), stats_ptr=st.data_ptr())
                torch.cuda.synchronize()
                assert U.bits_equal(buf.cpu().numpy(), rgb.reshape(-1)).all(), f"{scene}/{name}: the stats launch's frame"
                res[f"{scene}/{name}/stats"] = st.cpu().numpy()
    np.savez(out_path, **res)


if __name__ == "__main__":
    if len(sys.argv) != 3 or sys.argv[1] != "render":
        sys.exit("usage: r_cameras.py render OUT.npz")
    render_all(sys.argv[2])
