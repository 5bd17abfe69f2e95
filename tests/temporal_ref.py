"""The temporal accumulation's reference (gi.h "temporal accumulation"): reproject, test, blend restated in numpy
with the header's operation order -- fp64, no contraction, dots as (x x' + y y') + z z', crosses one subtraction of
two products per component, the four taps summed one after the other, j outer, i inner -- so it is exact bit for
bit; the camera vectors are those of the numpy camera aov_frames.rays_np uses.  And builders of synthetic previous
and current planes: a small analytic world seen from two cameras, so that reprojected taps are accepted where the
cameras see the same surface and rejected where they do not.  Host code only (numpy, the CPU oracle for the Cornell
guides); a helper, not a test.  Nothing here carries a tolerance.
"""
import copy
import types

import numpy as np

import aov_frames as A
import denoise_ref as D
import denoise_var_ref as DV

INF = np.inf
OUTPUTS = ("rgb", "var", "len")


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def _cross(a, b):
    """gi_math.h cross: (a.y b.z - b.y a.z, a.z b.x - b.z a.x, a.x b.y - b.x a.y)."""
    return np.stack([a[..., 1] * b[..., 2] - b[..., 1] * a[..., 2], a[..., 2] * b[..., 0] - b[..., 2] * a[..., 0],
                     a[..., 0] * b[..., 1] - b[..., 0] * a[..., 1]], -1)


def cam_np(sc, w):
    """(pos, left, up, top_left) of gi_capi.cpp make_cam(cam, w) for the scene-like camera sc (cam_pos, cam_look,
    focal): aov_frames.rays_np's own lines."""
    pos = np.array(sc.cam_pos, np.float64)
    f = A._norm(np.array(sc.cam_look, np.float64) - pos)
    up = np.array([0.0, 0.0, 1.0])
    left = A._norm(np.array([up[1] * f[2] - f[1] * up[2], up[2] * f[0] - f[2] * up[0], up[0] * f[1] - f[0] * up[1]]))
    tl = (((pos + sc.focal * f) + ((left * float(w)) * 0.5) * A.RES) + ((up * float(w)) * 0.5) * A.RES) - pos
    return pos, left, up, tl


def temporal_np(cam, prev, w, h, cur, hist=None, window=None, max_history=32, alpha_min=0.0, cos_min=0.9, sigma_p=0.01,
                prim_stop=True):
    """The operation over the window (None: the whole frame) of a w x h frame.  cam, prev: scene-like cameras (prev may
    be None without hist); cur, hist: dicts of planes over the window as gi.temporal takes them (cur["var"] may be
    missing: no variance is carried, "var" comes back None).  Returns dict(rgb, var, len) and, for the tests' own
    assertions, xs, ys (x', y' per pixel; NaN where none was formed), seen (history exists) and taps (accepted taps)."""
    x0, y0, x1, y1 = window if window is not None else (0, 0, w, h)
    rows, cols = y1 - y0, x1 - x0
    c = np.array(cur["rgb"], np.float64).reshape(rows, cols, 3)
    carry = cur.get("var") is not None
    V = np.array(cur["var"], np.float64).reshape(rows, cols, 3) if carry else np.zeros((rows, cols, 3))
    t = np.asarray(cur["t"], np.float64).reshape(rows, cols)
    valid = t < INF
    res = dict(rgb=c.copy(), var=V.copy() if carry else None, len=np.where(valid, 1, 0).astype(np.int32),
               xs=np.full((rows, cols), np.nan), ys=np.full((rows, cols), np.nan), seen=np.zeros((rows, cols), bool),
               taps=np.zeros((rows, cols), np.int32))
    if hist is None or rows * cols == 0:
        return res
    n = np.asarray(cur["normal"], np.float64).reshape(rows, cols, 3)
    pos, _, _, _ = cam_np(cam, w)
    ppos, pleft, pup, ptl = cam_np(prev, w)
    dirs = D.dirs_np(cam, w, h, window)
    pdirs = D.dirs_np(prev, w, h, window)
    ht = np.asarray(hist["t"], np.float64).reshape(rows, cols)
    hn = np.asarray(hist["normal"], np.float64).reshape(rows, cols, 3)
    hc = np.asarray(hist["rgb"], np.float64).reshape(rows, cols, 3)
    hV = np.asarray(hist["var"], np.float64).reshape(rows, cols, 3) if carry else np.zeros((rows, cols, 3))
    hlen = np.asarray(hist["len"], np.int32).reshape(rows, cols).astype(np.int64)
    with np.errstate(all="ignore"):
        P = pos + t[..., None] * dirs
        Pq_plane = ppos + ht[..., None] * pdirs
        Av, Bv, T = pleft * A.RES, pup * A.RES, ptl
        N = _cross(Av, Bv)
        det = _dot(T, N)
        v = P - ppos
        den = _dot(v, N)
        xs = -_dot(v, _cross(Bv, T)) / den
        ys = -_dot(v, _cross(T, Av)) / den
        fx, fy = np.floor(xs), np.floor(ys)
        seen = valid & (den * det > 0.0) & np.isfinite(xs) & np.isfinite(ys) & (fx >= x0 - 1.0) & (fx <= x1 - 1.0) & \
            (fy >= y0 - 1.0) & (fy <= y1 - 1.0)
        qx0 = np.where(seen, fx, float(x0)).astype(np.int64) - x0
        qy0 = np.where(seen, fy, float(y0)).astype(np.int64) - y0
        wx, wy = xs - fx, ys - fy
        sp = sigma_p * t
        sum_b = np.zeros((rows, cols))
        sum_c, sum_V = np.zeros((rows, cols, 3)), np.zeros((rows, cols, 3))
        len_h = np.full((rows, cols), 2 ** 31 - 1, np.int64)
        taps = np.zeros((rows, cols), np.int32)
        for j in (0, 1):
            for i in (0, 1):
                qx, qy = qx0 + i, qy0 + j
                use = seen & (qx >= 0) & (qx < cols) & (qy >= 0) & (qy < rows)
                qx, qy = np.where(use, qx, 0), np.where(use, qy, 0)
                b = (wx if i else 1.0 - wx) * (wy if j else 1.0 - wy)
                use = use & (b > 0.0) & (ht[qy, qx] < INF) & (hlen[qy, qx] >= 1)
                if prim_stop:
                    use = use & (np.asarray(hist["prim"]).reshape(rows, cols)[qy, qx] == np.asarray(cur["prim"]).reshape(rows, cols))
                use = use & (_dot(n, hn[qy, qx]) >= cos_min) & (np.abs(_dot(n, Pq_plane[qy, qx] - P)) <= sp)
                sum_b = np.where(use, sum_b + b, sum_b)
                sum_c = np.where(use[..., None], sum_c + b[..., None] * hc[qy, qx], sum_c)
                sum_V = np.where(use[..., None], sum_V + b[..., None] * hV[qy, qx], sum_V)
                len_h = np.where(use, np.minimum(len_h, hlen[qy, qx]), len_h)
                taps += use
        acc = taps > 0
        ln = np.where(len_h >= max_history, max_history, len_h + 1)
        inv = 1.0 / ln.astype(np.float64)
        a = np.where(inv > alpha_min, inv, alpha_min)[..., None]
        na = 1.0 - a
        res["rgb"] = np.where(acc[..., None], (na * (sum_c / sum_b[..., None])) + (a * c), c)
        if carry:
            res["var"] = np.where(acc[..., None], ((na * na) * (sum_V / sum_b[..., None])) + ((a * a) * V), V)
        res["len"] = np.where(acc, ln, res["len"]).astype(np.int32)
    res.update(xs=np.where(valid, xs, np.nan), ys=np.where(valid, ys, np.nan), seen=seen, taps=taps)
    return res


# ---- synthetic planes -------------------------------------------------------------------------------------
# The world: the wall x = X_WALL with cells of CELL[0] x CELL[1] in (y, z); the cells of kind 0 and 3 are recessed to
# x = X_DEEP.  A cell's kind gives its normal (kind 4: a random normal per pixel, which no cos_min above ~0 accepts),
# the cell itself is the primitive.  Seen from denoise_ref.SYN_CAM the wall is 5 away and a pixel 0.1 wide.
X_WALL, X_DEEP, CELL = -5.0, -4.5, (0.9, 0.7)


def camera(pos=D.SYN_CAM.cam_pos, look=D.SYN_CAM.cam_look, focal=D.SYN_CAM.focal):
    return types.SimpleNamespace(cam_pos=tuple(pos), cam_look=tuple(look), focal=focal)


def moved(cam, d):
    """cam translated by d, looking the same way (its lookAt moves along)."""
    return camera(np.add(cam.cam_pos, d), np.add(cam.cam_look, d), cam.focal)


# the camera pairs of the tests: name -> previous camera (the current one is SYN_CAM), and whether accepted pixels,
# reset pixels, or both must occur in the reference at the default parameters
SYN = camera()
PAIRS = {
    "identical": (SYN, "accepted"),
    "subpixel": (moved(SYN, (0.0, 0.031, -0.017)), "both"),                   # a pixel is 0.1 wide at the wall
    "pixels": (moved(SYN, (0.0, 0.37, 0.21)), "both"),
    "towards": (moved(SYN, (0.6, 0.0, 0.0)), "both"),
    "rotated": (camera(look=(1.0, 0.6, 0.5)), "both"),
    "behind": (moved(SYN, (10.0, 0.0, 0.0)), "reset"),                        # at x = 0: the wall lies behind it
    # in the wall's own plane, looking along +x exactly: den of a wall point is rounding noise, x' and y' are huge,
    # infinite or NaN -- rejected before any conversion to int -- while the recessed cell in front of it reprojects
    "in_plane": (camera((X_WALL, 0.5, 0.25), (X_WALL + 1.0, 0.5, 0.25)), "both"),
    # 1e9 to the side, looking along +x exactly: x' of every point is about 1e10, beyond an int
    "far": (camera((-10.0, 1e9, 0.25), (-9.0, 1e9, 0.25)), "reset"),
}


def world_planes(cam, w, h, window=None, seed=0, holes=0.12, jitter=0.002, with_len=False):
    """What cam sees of the world, over the window: dict(rgb, var, t, normal, prim[, len]); rgb in [0, 1], var >= 0
    with exact zeros (denoise_var_ref.synthetic_var), t jittered by a relative `jitter`, +inf holes, len in 0..40."""
    x0, y0, x1, y1 = window if window is not None else (0, 0, w, h)
    rows, cols = y1 - y0, x1 - x0
    g = np.random.default_rng(seed)
    d = D.dirs_np(cam, w, h, window)
    pos = np.array(cam.cam_pos, np.float64)
    with np.errstate(all="ignore"):
        td = (X_DEEP - pos[0]) / d[..., 0]
        cy, cz = np.floor((pos[1] + td * d[..., 1]) / CELL[0]), np.floor((pos[2] + td * d[..., 2]) / CELL[1])
        kind = np.mod(cy + 2.0 * cz, 5.0)
        kind = np.where(np.isfinite(kind), kind, 0.0).astype(np.int64)
        t = (np.where((kind == 0) | (kind == 3), X_DEEP, X_WALL) - pos[0]) / d[..., 0]
        t = t * (1.0 + jitter * g.normal(size=(rows, cols)))
        t = np.where((d[..., 0] > 0) & (t >= 0) & np.isfinite(t), t, INF)
    t[g.random((rows, cols)) < holes] = INF
    n = np.stack([-np.ones((rows, cols)), 0.1 * kind, 0.05 * kind], -1) + 0.02 * g.normal(size=(rows, cols, 3))
    n = np.where((kind == 4)[..., None], g.normal(size=(rows, cols, 3)), n)
    n = n / np.sqrt(_dot(n, n))[..., None]
    n[~(t < INF)] = 0.0
    prim = np.where(t < INF, np.clip(cy, -1000, 1000) * 4096 + np.clip(cz, -1000, 1000), -1).astype(np.int32)
    out = dict(rgb=g.random((rows, cols, 3)), var=DV.synthetic_var(rows, cols, seed + 1), t=t, normal=n, prim=prim)
    if with_len:
        out["len"] = g.integers(0, 41, size=(rows, cols)).astype(np.int32)
    return {k: np.ascontiguousarray(a) for k, a in out.items()}


def synthetic_pair(name, w, h, window=None, seed=0):
    """(current camera, previous camera, cur, hist) of the camera pair `name`.  The history is what the previous camera
    sees of the world -- for "behind" and "far", which see nothing of it, what the current camera sees (valid planes
    that only the geometry of the reprojection rejects).  "in_plane": no jitter on the current t, so that the wall's
    points lie in the previous camera's plane to rounding."""
    prev = PAIRS[name][0]
    cur = world_planes(SYN, w, h, window, seed=seed, jitter=0.0 if name == "in_plane" else 0.002)
    hist = world_planes(SYN if name in ("behind", "far") else prev, w, h, window, seed=seed + 7, with_len=True)
    return SYN, prev, cur, hist


def counts(r, cur):
    """(accepted, reset) valid pixels of a temporal_np result."""
    valid = cur["t"] < INF
    return int((valid & (r["taps"] > 0)).sum()), int((valid & (r["taps"] == 0)).sum())


# ---- the Cornell box under a moving camera (the oracle's guides) ---------------------------------------------
def cornell_at(offset):
    """cornell_guides of frame cornell/0.01 with the camera translated by `offset` (its lookAt moves along):
    dict(sc, w, h, t, normal, prim) from the oracle alone, as denoise_ref.cornell_guides builds them."""
    import x_rays as R
    sc, _, w, h = A.frame_scene("cornell/0.01")
    sc = copy.deepcopy(sc)
    sc.cam_pos = tuple(np.add(sc.cam_pos, offset))
    sc.cam_look = tuple(np.add(sc.cam_look, offset))
    r = A._reference(sc, w, h)
    hit = r["prim"] >= 0
    d = r["rays"][:, 3:6]
    tri = R.Geo(sc).ptri[r["prim"][hit]]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    n = n / np.sqrt(_dot(n, n))[:, None]
    n = np.where((_dot(d[hit], n) < 0)[:, None], n, -n)
    nrm = np.zeros((w * h, 3))
    nrm[hit] = n
    return dict(sc=sc, w=w, h=h, t=np.ascontiguousarray(r["t"].reshape(h, w)), normal=nrm.reshape(h, w, 3),
                prim=np.ascontiguousarray(r["prim"].reshape(h, w).astype(np.int32)))
