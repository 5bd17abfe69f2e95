"""The sample moments' reference (gi.h "sample moments"): mean and variance of the mean of a samples array,
restated in numpy with the header's operation order -- fp64, sums sequential in sample order from +0, the
variance two-pass with one multiply then one add per sample -- so it is exact bit for bit.  Host code only; a
helper, not a test.  Nothing here carries a tolerance.
"""
import numpy as np


def moments_np(samples):
    """samples (..., n, 3) float64, n >= 2 -> (mean, var), each (..., 3): mean = (((+0 + x_0) + x_1) + ...) / n;
    var = ((sum of (x_s - mean)^2 in sample order from +0) / (n - 1)) / n, the sample variance of the mean."""
    x = np.asarray(samples, np.float64)
    n = x.shape[-2]
    assert n >= 2 and x.shape[-1] == 3
    s = np.zeros(x.shape[:-2] + (3,))
    for k in range(n):
        s = s + x[..., k, :]
    mean = s / np.float64(n)
    m2 = np.zeros_like(s)
    for k in range(n):
        d = x[..., k, :] - mean
        m2 = m2 + d * d
    return mean, (m2 / np.float64(n - 1)) / np.float64(n)


def running_frames_np(samples):
    """{k: min(sum of the first k samples / k, 1)} for k = 2 .. n: the delivered frame of spp = k."""
    x = np.asarray(samples, np.float64)
    s = np.zeros(x.shape[:-2] + (3,))
    out = {}
    for k in range(x.shape[-2]):
        s = s + x[..., k, :]
        if k >= 1:
            m = s / np.float64(k + 1)
            out[k + 1] = np.where(m < 1.0, m, 1.0)
    return out
