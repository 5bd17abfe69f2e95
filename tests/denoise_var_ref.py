"""The variance-guided denoiser's reference (gi.h "variance-guided denoiser"): the filter restated in numpy with
the header's operation order, on denoise_ref's pieces -- so it is exact bit for bit; and a seeded variance plane
for synthetic inputs.  Host code only; a helper, not a test.  Nothing here carries a tolerance.
"""
import numpy as np

from denoise_ref import H, _dot, quantize_np, dirs_np, synthetic   # noqa: F401  (dirs_np, synthetic: for the tests)

G = (0.25, 0.5, 0.25)


def prefilter_np(V, valid):
    """g (rows, cols): per valid pixel the G x G weighted mean of v = (V.r + V.g) + V.b over its valid 3 x 3
    neighbours inside the window, dy outer, dx inner; 0 at invalid pixels (not used)."""
    rows, cols = valid.shape
    y, x = np.mgrid[0:rows, 0:cols]
    v = (V[..., 0] + V[..., 1]) + V[..., 2]
    sum_k, sum_v = np.zeros((rows, cols)), np.zeros((rows, cols))
    for dy in range(-1, 2):
        for dx in range(-1, 2):
            qy, qx = y + dy, x + dx
            use = (qy >= 0) & (qy < rows) & (qx >= 0) & (qx < cols)
            qy, qx = np.where(use, qy, y), np.where(use, qx, x)
            use = use & valid[qy, qx]
            k = G[dx + 1] * G[dy + 1]
            sum_k = np.where(use, sum_k + k, sum_k)
            sum_v = np.where(use, sum_v + k * v[qy, qx], sum_v)
    with np.errstate(all="ignore"):
        return np.where(valid, sum_v / sum_k, 0.0)


def denoise_var_np(pos, dirs, rgb, var, t, normal, albedo=None, levels=4, sigma_v=1.0, sigma_p=0.01, var_floor=1e-6,
                   normal_pow_log2=5, albedo_stop=True, all_levels=False):
    """The filter over a (rows, cols) window: denoise_ref.denoise_np's arguments plus var (rows, cols, 3).
    Returns (out_rgb, out_var, out_rgb8); all_levels: also the lists of c^1 .. c^levels (before the final min),
    V^1 .. V^levels and g of every level."""
    rows, cols = t.shape
    pos = np.asarray(pos, np.float64)
    valid = t < np.inf
    sv2 = np.float64(sigma_v) * np.float64(sigma_v)
    with np.errstate(all="ignore"):
        tt = np.where(valid, t, 0.0)
        P = pos + tt[..., None] * dirs
        sp = sigma_p * tt
        y, x = np.mgrid[0:rows, 0:cols]
        c = np.array(rgb, np.float64)
        V = np.array(var, np.float64)
        cs, Vs, gs = [], [], []
        for i in range(levels):
            s = 1 << i
            g = prefilter_np(V, valid)
            sigma2 = sv2 * g + np.float64(var_floor) if sv2 < np.inf else np.full((rows, cols), np.inf)
            sum_w = np.zeros((rows, cols))
            sum_c = np.zeros((rows, cols, 3))
            sum_V = np.zeros((rows, cols, 3))
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
                    sum_V = np.where(use[..., None], sum_V + (wt * wt)[..., None] * V[qy, qx], sum_V)
            c = np.where(valid[..., None], sum_c / sum_w[..., None], c)
            V = np.where(valid[..., None], sum_V / (sum_w * sum_w)[..., None], V)
            cs.append(c)
            Vs.append(V)
            gs.append(g)
        out = np.where(c < 1.0, c, 1.0)
    res = (out, V, quantize_np(out))
    return res + (cs, Vs, gs) if all_levels else res


def synthetic_var(rows, cols, seed):
    """A seeded non-negative variance plane (rows, cols, 3): magnitudes over four decades, with blocks of exact
    zeros (every third 6 x 8 block) and scattered single zeros."""
    g = np.random.default_rng(seed + 77)
    y, x = np.mgrid[0:rows, 0:cols]
    v = 10.0 ** g.uniform(-6.0, -2.0, (rows, cols, 3))
    v[((y // 6 + x // 8) % 3 == 0)] = 0.0
    v[g.random((rows, cols)) < 0.05] = 0.0
    return np.ascontiguousarray(v)
