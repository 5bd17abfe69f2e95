"""The radiance query's references (gi.h "radiance"): the Mode X random numbers, the sample rays and the resolve,
restated in numpy with the header's operation order -- the integer hash on uint64, everything else fp64 with one
rounding per operation -- so they are exact bit for bit.  Host code only; a helper, not a test.  Nothing here
carries a tolerance.
"""
import numpy as np

import aov_frames as A
import oracle_util as U

gi = U.pkg()
M64 = np.uint64
JITTER_BOUNCE, LENS_BOUNCE = 0xFFFF, 0xFFFE   # the bounce indices of the pixel jitter and the lens (gi.h)


def _u64(v):
    return np.asarray(v).astype(np.uint64)


def mix64(z):
    """gi_math.h mix64 (splitmix64's finaliser) on uint64 arrays; the products wrap modulo 2^64."""
    z = _u64(z)
    with np.errstate(over="ignore"):
        z = (z ^ (z >> M64(30))) * M64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> M64(27))) * M64(0x94D049BB133111EB)
    return z ^ (z >> M64(31))


def mx_key(seed, stream):
    with np.errstate(over="ignore"):
        return mix64(_u64(seed) + M64(0x9E3779B97F4A7C15) * (_u64(stream) + M64(1)))


def mx_u01k(key, sample, bounce, dim):
    """gi_math.h mx_u01k: a uniform in [0, 1) with 53 bits, exact in fp64."""
    w = (_u64(sample) << M64(32)) | ((_u64(bounce) & M64(0xFFFF)) << M64(16)) | (_u64(dim) & M64(0xFFFF))
    k = mix64(_u64(key) ^ w)
    return (k >> M64(11)).astype(np.float64) * 2.0 ** -53


_S = [float.fromhex(h) for h in ("-0x1.5555555555555p-3", "0x1.1111111111111p-7", "-0x1.a01a01a01a01ap-13", "0x1.71de3a556c734p-19",
                                 "-0x1.ae64567f544e4p-26", "0x1.6124613a86d09p-33", "-0x1.ae7f3e733b81fp-41", "0x1.952c77030ad4ap-49")]
_C = [float.fromhex(h) for h in ("-0x1.0000000000000p-1", "0x1.5555555555555p-5", "-0x1.6c16c16c16c17p-10", "0x1.a01a01a01a01ap-16",
                                 "-0x1.27e4fb7789f5cp-22", "0x1.1eed8eff8d898p-29", "-0x1.93974a8c07c9dp-37", "0x1.ae7f3e733b81fp-45")]


def mx_sincos_q(p):
    z = p * p
    ps, pc = np.full_like(p, _S[7]), np.full_like(p, _C[7])
    for k in range(6, -1, -1):
        ps = ps * z + _S[k]
        pc = pc * z + _C[k]
    return p + p * (z * ps), 1.0 + z * pc


def mx_disk(u1, u2):
    """gi_math.h mx_disk, operation for operation: (dx, dy, r2) of the concentric map of (u1, u2)."""
    u1, u2 = np.asarray(u1, np.float64), np.asarray(u2, np.float64)
    a, b = 2.0 * u1 - 1.0, 2.0 * u2 - 1.0
    qpi = float.fromhex("0x1.921fb54442d18p-1")
    ax = np.where(a < 0, -a, a) > np.where(b < 0, -b, b)
    r, num = np.where(ax, a, b), np.where(ax, b, a)
    with np.errstate(invalid="ignore", divide="ignore"):
        q = num / r
        sn, cs = mx_sincos_q(qpi * q)
        zero = (a == 0.0) & (b == 0.0)
        dx = np.where(zero, 0.0, r * np.where(ax, cs, sn))
        dy = np.where(zero, 0.0, r * np.where(ax, sn, cs))
        r2 = np.where(zero, 0.0, r * r)
    return dx, dy, r2


def _dot(a, b):
    return (a[..., 0:1] * b[..., 0:1] + a[..., 1:2] * b[..., 1:2]) + a[..., 2:3] * b[..., 2:3]


def camera_frame(sc, w):
    """(pos, forward, up, left, top_left) of a scene's camera for frames w wide: aov_frames.rays_np's lines."""
    pos = np.array(sc.cam_pos, np.float64)
    f = A._norm(np.array(sc.cam_look, np.float64) - pos)
    up = np.array([0.0, 0.0, 1.0])
    left = A._norm(np.array([up[1] * f[2] - f[1] * up[2], up[2] * f[0] - f[2] * up[0], up[0] * f[1] - f[0] * up[1]]))
    tl = (((pos + sc.focal * f) + ((left * float(w)) * 0.5) * A.RES) + ((up * float(w)) * 0.5) * A.RES) - pos
    return pos, f, up, left, tl


def sample_rays_np(sc, w, h, window, seed, s0, s1, jitter, aperture, focus, with_focus=False):
    """gi_sample_rays in numpy: (rays (n, 8), ids (n,) PATH_ID_DTYPE) of the window's pixels (row-major) and
    their samples [s0, s1), n = pixels * (s1 - s0); with_focus: also the focus points F (n, 3) (aperture > 0)."""
    x0, y0, x1, y1 = window if window is not None else (0, 0, w, h)
    pos, f, up, left, tl = camera_frame(sc, w)
    ns = s1 - s0
    y, x = np.mgrid[y0:y1, x0:x1]
    x, y = np.repeat(x.reshape(-1), ns), np.repeat(y.reshape(-1), ns)
    s = np.tile(np.arange(s0, s1), (x1 - x0) * (y1 - y0))
    stream = _u64(y) * M64(w) + _u64(x)
    key = mx_key(seed, stream)
    fx, fy = x.astype(np.float64).reshape(-1, 1), y.astype(np.float64).reshape(-1, 1)
    if jitter:
        fx = fx + mx_u01k(key, s, JITTER_BOUNCE, 0).reshape(-1, 1)
        fy = fy + mx_u01k(key, s, JITTER_BOUNCE, 1).reshape(-1, 1)
    d0 = (tl - (left * fx) * A.RES) - (up * fy) * A.RES
    n = len(s)
    o, d, F = np.tile(pos, (n, 1)), d0, None
    if aperture > 0:
        lx, ly, _ = mx_disk(mx_u01k(key, s, LENS_BOUNCE, 0), mx_u01k(key, s, LENS_BOUNCE, 1))
        F = pos + d0 * (focus / _dot(d0, f.reshape(1, 3)))
        o = (pos + left * (aperture * lx).reshape(-1, 1)) + up * (aperture * ly).reshape(-1, 1)
        d = F - o
    rays = np.zeros((n, gi.RAY_DOUBLES))
    rays[:, 0:3], rays[:, 3:6], rays[:, 6] = o, d, np.inf
    ids = np.zeros(n, gi.PATH_ID_DTYPE)
    ids["stream"], ids["sample"] = stream, s
    out = (np.ascontiguousarray(rays), ids)
    return out + (F,) if with_focus else out


def resolve_np(rows):
    """gi_resolve_samples in numpy: rows (n_pix, ns, 3) -> min(mean, 1) with the sum sequential in sample order
    from +0 (np.sum is pairwise: not the render's order)."""
    x = np.asarray(rows, np.float64)
    s = np.zeros((x.shape[0], 3))
    for k in range(x.shape[1]):
        s = s + x[:, k, :]
    m = s / np.float64(x.shape[1])
    return np.where(m < 1.0, m, 1.0)


def quantize_np(rgb):
    """gi_math.h quantize for channels in [0, 1]: trunc(255 c)."""
    return np.trunc(255 * np.asarray(rgb, np.float64)).astype(np.uint8)
