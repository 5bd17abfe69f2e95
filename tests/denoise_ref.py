"""The denoiser's reference (gi.h "denoiser"): the edge-avoiding a-trous filter restated in numpy with the
header's operation order -- fp64, no contraction, dots as (x x' + y y') + z z', the 25 taps summed one after
the other, dy outer, dx inner -- so it is exact bit for bit; and builders of synthetic inputs.  Host code only
(numpy, the CPU oracle for the Cornell guides); a helper, not a test.  Nothing here carries a tolerance.
"""
import types

import numpy as np

import aov_frames as A
import oracle_util as U

H = (0.0625, 0.25, 0.375, 0.25, 0.0625)
COLOURS = np.array([(1.0, 1.0, 1.0), (1.0, 0.0, 0.0), (0.0, 1.0, 0.0), (0.0, 0.0, 1.0)])
# the camera of the synthetic inputs (scene-like: what aov_frames.rays_np and gi.Camera read)
SYN_CAM = types.SimpleNamespace(cam_pos=(-10.0, 0.5, 0.25), cam_look=(1.0, 0.0, 0.0), focal=0.01)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def quantize_np(c):
    """gi_math.h quantize of (..., 3) colours: (int)(255 c) per channel; a channel outside 0..255: black."""
    q = np.trunc(255 * c)
    ok = ((q >= 0) & (q <= 255)).all(-1, keepdims=True)
    return np.where(ok, q, 0.0).astype(np.uint8)


def denoise_np(pos, dirs, rgb, t, normal, albedo=None, levels=4, sigma_c=0.25, sigma_p=0.01, normal_pow_log2=5,
               albedo_stop=True, all_levels=False):
    """The filter over a (rows, cols) window: pos (3,) the camera position, dirs (rows, cols, 3) the pixels'
    normalised primary directions (gi.camera_rays' d), rgb / normal / albedo (rows, cols, 3), t (rows, cols).
    Returns (out_rgb, out_rgb8); all_levels: also the list of c^1 .. c^levels before the final min."""
    rows, cols = t.shape
    pos = np.asarray(pos, np.float64)
    valid = t < np.inf
    with np.errstate(all="ignore"):
        tt = np.where(valid, t, 0.0)
        P = pos + tt[..., None] * dirs
        sp = sigma_p * tt
        y, x = np.mgrid[0:rows, 0:cols]
        c = np.array(rgb, np.float64)
        steps = []
        for i in range(levels):
            s = 1 << i
            sg = np.ldexp(np.float64(sigma_c), -i)
            sigma2 = sg * sg
            sum_w = np.zeros((rows, cols))
            sum_c = np.zeros((rows, cols, 3))
            for dy in range(-2, 3):
                for dx in range(-2, 3):
                    qy, qx = y + s * dy, x + s * dx
                    use = (qy >= 0) & (qy < rows) & (qx >= 0) & (qx < cols)
                    qy, qx = np.where(use, qy, y), np.where(use, qx, x)
                    use = use & valid[qy, qx]
                    if albedo_stop:
                        use = use & (albedo[qy, qx] == albedo).all(-1)
                    k = H[dx + 2] * H[dy + 2]
                    wn = _dot(normal, normal[qy, qx])
                    wn = np.where(wn > 0.0, wn, 0.0)
                    for _ in range(normal_pow_log2):
                        wn = wn * wn
                    wp = 1.0 - np.abs(_dot(normal, P[qy, qx] - P)) / sp
                    wp = np.where(wp > 0.0, wp, 0.0)
                    cq = c[qy, qx]
                    e = c - cq
                    wc = 1.0 / (1.0 + _dot(e, e) / sigma2)
                    wt = ((k * wn) * wp) * wc
                    sum_w = np.where(use, sum_w + wt, sum_w)
                    sum_c = np.where(use[..., None], sum_c + wt[..., None] * cq, sum_c)
            c = np.where(valid[..., None], sum_c / sum_w[..., None], c)
            steps.append(c)
        out = np.where(c < 1.0, c, 1.0)
    res = (out, quantize_np(out))
    return res + (steps,) if all_levels else res


def dirs_np(sc, w, h, window=None):
    """(rows, cols, 3): the window's normalised primary directions by the numpy camera (aov_frames.rays_np)."""
    x0, y0, x1, y1 = window if window is not None else (0, 0, w, h)
    return np.ascontiguousarray(A.rays_np(sc, w, h, window)[:, 3:6].reshape(y1 - y0, x1 - x0, 3))


def synthetic(rows, cols, seed, holes=0.15):
    """Seeded planes of a (rows, cols) window: unit normals (blocks of three palette normals slightly perturbed,
    the rest random), t around 5 with +inf holes, albedo drawn from four colours in blocks, rgb in [0, 1]."""
    g = np.random.default_rng(seed)
    y, x = np.mgrid[0:rows, 0:cols]
    block = (y // 5 + x // 7) % 4
    palette = np.array([(1.0, 0.0, 0.0), (0.0, 0.6, 0.8), (-0.6, 0.0, 0.8)])
    n = g.normal(size=(rows, cols, 3))
    pal = block < 3
    n[pal] = palette[block[pal]] + 0.02 * g.normal(size=(int(pal.sum()), 3))
    n = n / np.sqrt(_dot(n, n))[..., None]
    t = 5.0 + 0.02 * g.random((rows, cols)) + 0.5 * ((y // 9 + x // 11) % 2)
    t[g.random((rows, cols)) < holes] = np.inf
    albedo = COLOURS[((y // 4 + x // 6) % 4 + (g.random((rows, cols)) < 0.1)) % 4]
    rgb = g.random((rows, cols, 3))
    n[~(t < np.inf)] = 0.0
    return dict(rgb=np.ascontiguousarray(rgb), t=np.ascontiguousarray(t), normal=np.ascontiguousarray(n),
                albedo=np.ascontiguousarray(albedo))


_cornell = {}


def cornell_guides():
    """The guides of frame cornell/0.01 (64 x 40) from the oracle alone: t and the hit primitive of
    aov_frames.reference, the facing normals from the triangles, the albedo as the numpy texel of the oracle's
    hit and uv.  Built once, read-only.  Returns dict(sc, w, h, dirs, t, normal, albedo)."""
    if not _cornell:
        import x_rays as R
        key = "cornell/0.01"
        sc, _, w, h = A.frame_scene(key)
        r = A.reference(key)
        hit = r["prim"] >= 0
        d = r["rays"][:, 3:6]
        tri = R.Geo(sc).ptri[r["prim"][hit]]
        n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
        n = n / np.sqrt(_dot(n, n))[:, None]
        n = np.where((_dot(d[hit], n) < 0)[:, None], n, -n)
        nrm = np.zeros((w * h, 3))
        nrm[hit] = n
        col = np.array([sc.entities[k].material.color for k in r["hit"][hit]], np.float64).reshape(-1, 3)
        alb = np.zeros((w * h, 3))
        alb[hit] = A.texel_np(col, r["uv"][hit, 0], r["uv"][hit, 1])
        out = dict(dirs=d.reshape(h, w, 3), t=r["t"].reshape(h, w), normal=nrm.reshape(h, w, 3), albedo=alb.reshape(h, w, 3))
        for a in out.values():
            a.setflags(write=False)
        out.update(sc=sc, w=w, h=h)
        _cornell.update(out)
    return _cornell


def cornell_frame(spp, seed, depth=4):
    """The oracle's Mode X frame of cornell/0.01 as (h, w, 3)."""
    g = cornell_guides()
    return U.oracle_render(g["sc"].to_scn(), g["w"], g["h"], mode=1, spp=spp, depth=depth, seed=seed)["rgb"].reshape(g["h"], g["w"], 3)
