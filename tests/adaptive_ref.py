"""The adaptive sampling reference (gi.h "adaptive sampling"): the rule that stops pixels between the passes of a
Mode X frame, restated in numpy with the header's operation order -- fp64, S1 and S2 sequential in sample order from
+0 with one multiply then one add per sample, the one-pass variance of the mean clamped at 0 -- so it is exact bit
for bit.  Host code only; a helper, not a test.  Nothing here carries a tolerance.
"""
import numpy as np


def quantize_np(rgb):
    """gi_math.h quantize: (int)(255 c) per channel by truncation; a pixel with a channel outside 0..255 (NaN
    included) is (0, 0, 0)."""
    with np.errstate(invalid="ignore"):
        v = 255.0 * np.asarray(rgb, np.float64)
        ok = ((v > -1.0) & (v < 256.0)).all(-1, keepdims=True)
        q = np.where(ok, np.trunc(np.where(ok, v, 0.0)), 0.0)
    return q.astype(np.uint8)


def adaptive_np(samples, passes, spp, tol, min_samples=2, relative=False, y_floor=0.0, resolved=None):
    """samples (..., spp', 3) float64 with spp' >= the last pass's end: every pixel's radiance rows, whether traced
    or not.  passes: [(begin, end), ...] from 0, contiguous, each of >= 2 samples, end <= spp.  resolved (...) bool:
    the pixels the classify pass resolved without traversal (their rows are +0); None: none.
    Returns one dict per pass: n (...) int32, mean, var, rgb (..., 3) float64, rgb8 uint8 and active (...) bool (the
    pixels still traced after the pass)."""
    x = np.asarray(samples, np.float64)
    shape = x.shape[:-2]
    assert x.shape[-1] == 3 and min_samples >= 2 and tol > 0
    s1, s2 = np.zeros(shape + (3,)), np.zeros(shape + (3,))
    n = np.zeros(shape, np.int32)
    active = np.ones(shape, bool)
    if resolved is not None:
        assert not x[resolved].any()
    out, at = [], 0
    for b, e in passes:
        assert b == at and e - b >= 2 and e <= spp and e <= x.shape[-2]
        at = e
        a3 = active[..., None]
        for k in range(b, e):
            xs = x[..., k, :]
            s1 = np.where(a3, s1 + xs, s1)
            s2 = np.where(a3, s2 + xs * xs, s2)
        n = np.where(active, np.int32(e), n)
        with np.errstate(all="ignore"):
            dn = n.astype(np.float64)[..., None]
            m = s1 / dn
            v = ((s2 - s1 * m) / (dn - 1.0)) / dn
            v = np.where((v > 0) | np.isnan(v), v, 0.0)   # (a NaN stays: it must not stop the pixel)
            err = (v[..., 0] + v[..., 1]) + v[..., 2]
            thr = np.full(shape, np.float64(tol) * np.float64(tol))
            if relative:
                y = (m[..., 0] + m[..., 1]) + m[..., 2]
                f = np.where(y > y_floor, y, np.float64(y_floor))
                thr = thr * (f * f)
            stop = ((e >= min_samples) & (err <= thr)) | (e == spp)
        active = active & ~stop
        rgb = np.where(1.0 < m, 1.0, m)   # smin(m, 1): a NaN stays
        out.append(dict(n=n.copy(), mean=m, var=v, rgb=rgb, rgb8=quantize_np(rgb), active=active.copy()))
    return out
