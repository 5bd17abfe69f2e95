"""Adversarial inputs for Mode R's primitive tests (a helper, not a test): (triangle, ray), (box, ray) and
(sphere, ray) records aimed at the shortcuts of gi_math.h -- the bounding-sphere prefilter, tri_accept's two
early exits, tri_hit_corners' parallel test, the 4-lane face split and sphere_hit's fp32/fp64 mix.

cases(kind) -> (recs, names, cls): the float64 record array, the class names and each record's class index.
    tris     15 doubles  p1 p2 p3 o dir
    boxes    12 doubles  min max o dir
    spheres  10 doubles  pos radius o dir
`dir` is not normalised (every consumer normalises it as the reference's Ray constructor does).

Deterministic without numpy.random: every uniform is (k >> 11) * 2**-53 of a splitmix64 counter hash, the
counter stream keyed by the class name.  tests/golden/adv_*.npz store the sha256 of the record bytes
(digest()), so a drift of this generator fails the tests instead of silently changing their inputs.  Only + - *
/ sqrt, conversions and comparisons (powers of ten come from a table of literals), all correctly rounded, so the
records do not depend on the platform's libm."""
from __future__ import annotations

import hashlib

import numpy as np

KINDS = ("tris", "boxes", "spheres")
WIDTH = {"tris": 15, "boxes": 12, "spheres": 10}
_GOLD = np.uint64(0x9E3779B97F4A7C15)


def _mix(z):
    z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return z ^ (z >> np.uint64(31))


class Stream:
    """Counter-based uniforms: value i of the stream `name` is splitmix64(key(name) + GOLD * (i + 1))."""

    def __init__(self, name: str):
        self.key = np.uint64(int.from_bytes(hashlib.sha256(name.encode()).digest()[:8], "little"))
        self.ctr = 0

    def u(self, *shape):   # [0, 1)
        n = int(np.prod(shape)) if shape else 1
        idx = np.arange(self.ctr + 1, self.ctr + 1 + n, dtype=np.uint64)
        self.ctr += n
        with np.errstate(over="ignore"):
            k = _mix(self.key + _GOLD * idx)
        r = (k >> np.uint64(11)).astype(np.float64) * 2.0 ** -53
        return r.reshape(shape) if shape else r[0]

    def s(self, *shape):   # [-1, 1)
        return 2.0 * self.u(*shape) - 1.0

    def sign(self, *shape):
        return np.where(self.u(*shape) < 0.5, -1.0, 1.0)

    def pick(self, m, *shape):   # integers in [0, m)
        return np.minimum((self.u(*shape) * m).astype(np.int64), m - 1)

    def pow10(self, lo: int, hi: int, *shape):
        """About log-uniform over [10**lo, 10**hi): an exact table power of ten times a factor in [1, 10)."""
        e = self.pick(hi - lo, *shape) + lo
        table = np.array([float("1e%d" % k) for k in range(lo, hi)])
        return table[e - lo] * (1.0 + 9.0 * self.u(*shape) ** 2)


# ---- glm's vector operations in its operation order (numpy, rows of 3) --------------------------------------

def dot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def cross(x, y):
    return np.stack([x[:, 1] * y[:, 2] - y[:, 1] * x[:, 2], x[:, 2] * y[:, 0] - y[:, 2] * x[:, 0],
                     x[:, 0] * y[:, 1] - y[:, 0] * x[:, 1]], axis=1)


def normalize(v):
    with np.errstate(all="ignore"):
        return v * (1.0 / np.sqrt(dot(v, v)))[:, None]


def col(x):
    return np.asarray(x, np.float64)[:, None]


def realised_metric(p1, p2, p3, o, draw):
    """Steering only (never an expected value): max(|d1 - d2|^2, |d2 - d3|^2) of ImpTriangle::intersect's
    acceptance test at the point its fp32 solve lands on, evaluated with numpy's float32 / float64."""
    f = np.float32
    with np.errstate(all="ignore"):
        d = normalize(draw)
        e1, e2 = (p2 - p1).astype(f), (p3 - p1).astype(f)
        pos = 0.5 * (0.5 * (p1 + p2) + p3)
        m = (-d).astype(f)
        m00, m01, m02 = e1[:, 0], e2[:, 0], m[:, 0]
        m10, m11, m12 = e1[:, 1], e2[:, 1], m[:, 1]
        m20, m21, m22 = e1[:, 2], e2[:, 2], m[:, 2]
        det = m00 * (m11 * m22 - m21 * m12) - m10 * (m01 * m22 - m21 * m02) + m20 * (m01 * m12 - m11 * m02)
        ood = f(1.0) / det
        i20, i21, i22 = (m10 * m21 - m20 * m11) * ood, (-(m00 * m21 - m20 * m01)) * ood, (m00 * m11 - m10 * m01) * ood
        r = (o - pos).astype(f)
        solz = i20 * r[:, 0] + i21 * r[:, 1] + i22 * r[:, 2]
        pt = o + solz.astype(np.float64)[:, None] * d
        d1, d2, d3 = (normalize(cross(a - pt, b - pt)) for a, b in ((p1, p2), (p2, p3), (p3, p1)))
        q1, q2 = d1 - d2, d2 - d3
        return np.maximum(dot(q1, q1), dot(q2, q2))


# ---- triangles ---------------------------------------------------------------------------------------------

def _tri(st, n, sc):
    sc = col(sc)
    return st.s(n, 3) * sc, st.s(n, 3) * sc, st.s(n, 3) * sc


def _bary(st, n):
    a = st.u(n)
    return col(a), col(st.u(n) * (1.0 - a))


def _inside(st, p1, p2, p3):
    a, b = _bary(st, len(p1))
    return p1 + (p2 - p1) * a + (p3 - p1) * b


def _mixed_target(st, p1, p2, p3, sc):
    """A quarter each: inside, on the p1-p2 edge, within 1e-3 of that edge, anywhere."""
    n = len(p1)
    a, _ = _bary(st, n)
    edge = p1 + (p2 - p1) * a
    near = edge + st.s(n, 3) * col(sc) * 1e-3
    any_ = st.s(n, 3) * col(sc) * 2.0
    ins = _inside(st, p1, p2, p3)
    k = col(np.arange(n) % 4)
    return np.where(k == 0, ins, np.where(k == 1, edge, np.where(k == 2, near, any_)))


def _rec_tri(p1, p2, p3, o, d):
    return np.concatenate([p1, p2, p3, o, d], axis=1)


def _t_generic(name, n, target, sliver=None, mirror=False):
    st = Stream("tri/" + name)
    sc = st.pow10(-3, 3, n)
    p1, p2, p3 = _tri(st, n, sc)
    if sliver is not None:
        p2 = p1 + (p2 - p1) * sliver
    if mirror:
        p3 = -p3   # ExpRectangle's p4 = -p3 (the spurious faces of an ExpBox)
    o = st.s(n, 3) * col(sc) * 20.0
    if target == "inside":
        tgt = _inside(st, p1, p2, p3)
    elif target == "edge":
        tgt = p1 + (p2 - p1) * _bary(st, n)[0]
    elif target == "near_edge":
        a, b = _bary(st, n)
        off = cross(p2 - p1, p3 - p1) * (0.02 * col(st.s(n)) * (a + b) * (1.0 - a - b) / col(sc))
        plane = p1 + (p2 - p1) * a + (p3 - p1) * b + off       # just off the plane: the acceptance angle's edge
        edge = p1 + (p2 - p1) * a + st.s(n, 3) * col(sc) * col(st.pow10(-6, -2, n))
        tgt = np.where(col(np.arange(n) % 4) == 0, plane, edge)
    elif target == "anywhere":
        tgt = st.s(n, 3) * col(sc) * 2.0
    else:
        tgt = _mixed_target(st, p1, p2, p3, sc)
    return _rec_tri(p1, p2, p3, o, tgt - o)


def _t_scale(name, n, scale):
    st = Stream("tri/" + name)
    sc = np.full(n, scale) * (1.0 + 9.0 * st.u(n))   # (1e-20 .. 1e-19: fp32 cofactors and determinants around 1e-39)
    p1, p2, p3 = _tri(st, n, sc)
    o = st.s(n, 3) * col(sc) * 20.0
    return _rec_tri(p1, p2, p3, o, _mixed_target(st, p1, p2, p3, sc) - o)


def _t_overflow(n):
    """Magnitudes at which a squared length, an fp32 cast or a sub-triangle cross product leaves its range."""
    st = Stream("tri/overflow")
    k = np.arange(n) % 6
    big = st.pow10(76, 79, n)
    # 0: everything past fp32's range; 1: fp32 cofactor products at its edge, the origin as far as an fp32 holds;
    # 2: a triangle far from the origin with edges of a few ulps; 3: a small triangle seen from 1e77; 4: fp32 edges
    # whose products overflow; 5: an ordinary view of a triangle with edges around 1e18 (the largest finite
    # sub-triangle cross products)
    huge = st.pow10(17, 20, n)
    edge = np.select([k == 0, k == 1, k == 2, k == 3, k == 4], [big, huge, st.pow10(60, 64, n), st.pow10(-2, 2, n),
                                                               st.pow10(28, 32, n)], huge)
    base = np.select([k == 2], [big], 0.0)
    odist = np.select([k == 0, k == 1, k == 2, k == 3, k == 4], [big, st.pow10(36, 39, n), big, big, st.pow10(36, 39, n)], huge * 20.0)
    p1, p2, p3 = _tri(st, n, edge)
    shift = st.s(n, 3) * col(base)
    p1, p2, p3 = p1 + shift, p2 + shift, p3 + shift
    o = shift + st.s(n, 3) * col(odist)
    tgt = np.where(col(np.arange(n) // 6 % 2) == 0, _inside(st, p1, p2, p3), shift + st.s(n, 3) * col(edge) * 2.0)
    return _rec_tri(p1, p2, p3, o, tgt - o)


def _t_near_parallel(n):
    """Rays in the triangle's plane plus 1e-17 .. 1e-9 of its normal (and exactly in-plane ones), from origins in
    or near the plane: the fp32 determinant is rounding noise, the parallel test within a few ulps of 0."""
    st = Stream("tri/near_parallel")
    sc = st.pow10(-3, 3, n)
    p1, p2, p3 = _tri(st, n, sc)
    nrm = normalize(cross(p2 - p1, p3 - p1))
    a, b = _bary(st, n)
    spread = col(np.where(np.arange(n) % 3 == 0, 3.0, 1.0))       # a third of the origins up to 3x outside
    o = p1 + (p2 - p1) * (0.5 + (a - 0.5) * spread) + (p3 - p1) * (0.5 + (b - 0.5) * spread)
    o = o + nrm * col(sc) * col(np.where(np.arange(n) % 5 == 0, st.s(n) * 1e-9, 0.0))
    tgt = _inside(st, p1, p2, p3)
    flat = tgt - o
    flat = flat - nrm * col(dot(flat, nrm))
    eps = st.sign(n) * st.pow10(-17, -9, n) * np.where(np.arange(n) % 7 == 0, 0.0, 1.0)
    d = flat + nrm * col(eps * np.sqrt(dot(flat, flat)))
    return _rec_tri(p1, p2, p3, o, d)


def _t_fp32_parallel(n):
    """dot(n, d) != 0 in fp64 while the fp32 determinant is 0 or a subnormal: a triangle in a coordinate plane
    through the origin and a ray whose component along that plane's axis is below fp32's normal range."""
    st = Stream("tri/fp32_parallel")
    ax = np.arange(n) % 3
    sc = 0.5 + 1.5 * st.u(n)
    q1, q2, q3 = (st.s(n, 2) * col(sc) for _ in range(3))
    a, b = _bary(st, n)
    inside = q1 + (q2 - q1) * a + (q3 - q1) * b
    tgt = np.where(col(np.arange(n) // 3 % 3) == 2, st.s(n, 2) * col(sc) * 1.5, inside)
    oq = st.s(n, 2) * col(sc) * 6.0
    run = tgt - oq
    length = np.sqrt(run[:, 0] ** 2 + run[:, 1] ** 2)
    area2 = np.abs((q2 - q1)[:, 0] * (q3 - q1)[:, 1] - (q2 - q1)[:, 1] * (q3 - q1)[:, 0])
    # the determinant is the axis component of d times area2: [3e-39, 1.1e-38] keeps 1 / det finite; a third of
    # the cases go below fp32's smallest subnormal (the determinant is exactly 0)
    delta = np.where(np.arange(n) // 9 % 3 == 2, st.pow10(-60, -46, n), (3e-39 + 8e-39 * st.u(n)) / area2) * st.sign(n)
    lift = length * delta

    def embed(q, z):
        out = np.zeros((n, 3))
        for k in range(3):
            m = ax == k
            out[m, k] = z[m]
            out[m, (k + 1) % 3] = q[m, 0]
            out[m, (k + 2) % 3] = q[m, 1]
        return out

    zero = np.zeros(n)
    return _rec_tri(embed(q1, zero), embed(q2, zero), embed(q3, zero), embed(oq, -lift), embed(run, lift))


def _t_behind(n):
    st = Stream("tri/behind")
    sc = st.pow10(-3, 3, n)
    p1, p2, p3 = _tri(st, n, sc)
    tgt = _mixed_target(st, p1, p2, p3, sc)
    o = tgt + st.s(n, 3) * col(sc) * 20.0
    return _rec_tri(p1, p2, p3, o, o - tgt)   # the triangle lies behind the origin: no t > 0 test in the reference


def _t_axis(n):
    """Axis-parallel triangles and rays: direction components that are exactly 0."""
    st = Stream("tri/axis")
    sc = st.pow10(-3, 3, n)
    p1, p2, p3 = _tri(st, n, sc)
    ax = np.arange(n) % 3
    rows = np.arange(n)
    h = st.s(n) * sc
    for p in (p1, p2, p3):
        p[rows, ax] = h                                 # the triangle lies in the plane x_ax = h
    tgt = _mixed_target(st, p1, p2, p3, sc)
    tgt[rows, ax] = np.where(np.arange(n) % 4 == 2, tgt[rows, ax], h)
    kind = np.arange(n) // 3 % 3                        # 0: along the plane's axis; 1: another axis (in-plane); 2: one zero
    dax = np.where(kind == 0, ax, (ax + 1 + np.arange(n) // 9 % 2) % 3)
    d = np.zeros((n, 3))
    d[rows, dax] = st.sign(n)
    gen = st.s(n, 3)
    gen[rows, (ax + 1) % 3] = 0.0
    d = np.where(col(kind) == 2, gen, d)
    o = tgt - d * col(sc) * col(1.0 + 19.0 * st.u(n))
    return _rec_tri(p1, p2, p3, o, d)


def _t_band(n):
    """The acceptance test's 1e-3 threshold.  The reference's point is where its fp32 solve lands: on the
    triangle's plane up to a height of ~1e-7 of the ray's length, so the sub-triangle normals spread by 1e-3
    only within ~1e-5 of an edge.  The target's distance from the p1-p2 edge (inwards, in the plane) and its
    height above the plane are scaled together by a factor found per case: a bisection on realised_metric()
    -- steering only -- between a factor whose case is accepted and one whose case is not, ended where the two
    differ by 1e-6 relative; one of the two ends is kept.  The solve's rounding moves with the factor, so the
    kept metric scatters around 1e-3 instead of sitting in tri_accept's 1e-9 band."""
    st = Stream("tri/band")
    sc = st.pow10(-2, 2, n)
    p1, p2, p3 = _tri(st, n, sc)
    e1, e2 = p2 - p1, p3 - p1
    nrm = normalize(cross(e1, e2))
    inward = normalize(cross(nrm, e1))
    inward = inward * col(np.where(dot(inward, e2) < 0, -1.0, 1.0))
    base = p1 + e1 * col(0.2 + 0.6 * st.u(n))
    o = base + (nrm * col(st.sign(n) * (0.2 + st.u(n))) + st.s(n, 3) * 0.5) * col(sc) * 10.0
    tilt = col(st.s(n) * 0.05)

    def rays(fac):
        tgt = base + (inward + nrm * tilt) * col(fac * sc)
        return tgt - o

    thr = 1.0e-3
    lo, hi = np.full(n, 1e-9), np.full(n, 0.05)          # lo: rejected (next to the edge), hi: accepted
    ok = (realised_metric(p1, p2, p3, o, rays(lo)) >= thr) & (realised_metric(p1, p2, p3, o, rays(hi)) < thr)
    for _ in range(60):
        mid = np.sqrt(lo * hi)
        acc = realised_metric(p1, p2, p3, o, rays(mid)) < thr
        hi = np.where(acc, mid, hi)
        lo = np.where(acc, lo, mid)
        if (hi <= lo * (1.0 + 1e-6)).all():
            break
    fac = np.where(st.u(n) < 0.5, lo, hi)
    fac = np.where(ok, fac, 1e-5)
    return _rec_tri(p1, p2, p3, o, rays(fac))


TRI_CLASSES = [
    ("inside", lambda: _t_generic("inside", 12000, "inside")),
    ("edge", lambda: _t_generic("edge", 12000, "edge")),
    ("near_edge", lambda: _t_generic("near_edge", 26000, "near_edge")),
    ("sliver_1e-3", lambda: _t_generic("sliver_1e-3", 12000, "mixed", sliver=1e-3)),
    ("sliver_1e-9", lambda: _t_generic("sliver_1e-9", 12000, "mixed", sliver=1e-9)),
    ("anywhere", lambda: _t_generic("anywhere", 12000, "anywhere")),
    ("mirror", lambda: _t_generic("mirror", 12000, "mixed", mirror=True)),
    ("near_parallel", lambda: _t_near_parallel(28000)),
    ("scale_1e-20", lambda: _t_scale("scale_1e-20", 12000, 1e-20)),
    ("scale_1e8", lambda: _t_scale("scale_1e8", 12000, 1e8)),
    ("overflow", lambda: _t_overflow(12000)),
    ("fp32_parallel", lambda: _t_fp32_parallel(24000)),
    ("behind", lambda: _t_behind(12000)),
    ("axis", lambda: _t_axis(12000)),
    ("band", lambda: _t_band(30000)),
]


# ---- boxes -------------------------------------------------------------------------------------------------

def _rec_box(mn, mx, o, d):
    return np.concatenate([mn, mx, o, d], axis=1)


def _box(st, n, sc):
    c = st.s(n, 3) * col(sc * np.where(np.arange(n) % 2 == 1, 0.5, 4.0))
    hw = (st.s(n, 3) + 1.01) * col(sc * 0.25)
    return c, hw


def _b_generic(name, n, mode, lo=-2, hi=2):
    st = Stream("box/" + name)
    sc = st.pow10(lo, hi, n)
    c, hw = _box(st, n, sc)
    o = st.s(n, 3) * col(sc) * 10.0
    if mode == "through":
        tgt = c + hw * st.s(n, 3)
    elif mode == "mirror":
        tgt = -c + hw * st.s(n, 3)   # the spurious faces pass through the box's mirror image
    else:                            # near: 1, 2 or 3 coordinates within 1 +- 0.05 of a face, an edge or a corner
        f = st.s(n, 3)
        edge = st.sign(n, 3) * (0.95 + 0.1 * st.u(n, 3))
        m = np.arange(n) % 3 + 1
        first = st.pick(3, n)
        for k in range(3):
            on = ((np.arange(3)[None, :] - col(first)) % 3 < col(m))[:, k]
            f[:, k] = np.where(on, edge[:, k], f[:, k])
        tgt = c + hw * f
    return _rec_box(c - hw, c + hw, o, tgt - o)


def _b_octree(name, n, inside):
    """Cells of an octree over [-20, 20]^3 (levels 1 .. 7), seen from inside or from outside the root."""
    st = Stream("box/" + name)
    lvl = st.pick(7, n) + 1
    size = 40.0 / 2.0 ** lvl
    cell = np.floor(st.u(n, 3) * col(2.0 ** lvl))
    mn = -20.0 + cell * col(size)
    mx = mn + col(size)
    if inside:
        o = st.s(n, 3) * 19.0
    else:
        o = st.s(n, 3) * 30.0
        k = st.pick(3, n)
        o[np.arange(n), k] = st.sign(n) * (21.0 + 40.0 * st.u(n))
    tgt = mn + col(size) * (st.u(n, 3) * np.where(col(np.arange(n) % 2) == 0, 1.0, 3.0) - np.where(col(np.arange(n) % 2) == 0, 0.0, 1.0))
    return _rec_box(mn, mx, o, tgt - o)


def _b_axis_face(n):
    """Axis-parallel rays lying in a face's plane (or a hair off it)."""
    st = Stream("box/axis_face")
    sc = st.pow10(-2, 2, n)
    c, hw = _box(st, n, sc)
    mn, mx = c - hw, c + hw
    rows = np.arange(n)
    fax = rows % 3
    dax = (fax + 1 + rows // 3 % 2) % 3
    o = c + hw * st.s(n, 3) * 1.2
    o[rows, fax] = np.where(st.u(n) < 0.5, mn[rows, fax], mx[rows, fax]) * np.where(rows % 5 == 0, 1.0 + 1e-15, 1.0)
    d = np.zeros((n, 3))
    d[rows, dax] = st.sign(n)
    o = o - d * col(sc) * col(10.0 * st.u(n))
    return _rec_box(mn, mx, o, d)


BOX_CLASSES = [
    ("through", lambda: _b_generic("through", 8000, "through")),
    ("near_face", lambda: _b_generic("near_face", 16000, "near")),
    ("mirror", lambda: _b_generic("mirror", 8000, "mirror")),
    ("octree_inside", lambda: _b_octree("octree_inside", 8000, True)),
    ("octree_outside", lambda: _b_octree("octree_outside", 8000, False)),
    ("axis_face", lambda: _b_axis_face(6000)),
    ("scales", lambda: _b_generic("scales", 10000, "near", lo=-3, hi=8)),
]


# ---- spheres -----------------------------------------------------------------------------------------------

def _rec_sph(pos, r, o, d):
    return np.concatenate([pos, col(r), o, d], axis=1)


def _f32(x):
    return np.asarray(x, np.float64).astype(np.float32).astype(np.float64)


def _s_axis(name, n, zero_axes):
    """Aimed at the sphere (two thirds through it); the listed direction components are exactly 0."""
    st = Stream("sph/" + name)
    pos = st.s(n, 3) * 5.0
    r = _f32(st.pow10(-1, 1, n))
    d = st.s(n, 3)
    tgt = pos + st.s(n, 3) * col(r) * col(np.where(np.arange(n) % 3 == 2, 1.6, 0.57))
    o = tgt - d * col(r) * col(2.0 + 20.0 * st.u(n))
    for k in zero_axes:
        d[:, k] = 0.0
        o[:, k] = tgt[:, k]
    if zero_axes == (0, 1, 2):
        o = pos + st.s(n, 3) * col(r) * 2.0
    return _rec_sph(pos, r, o, d)


def _s_tangent(n):
    """Closest approach r (1 + delta), |delta| up to 4e-7: the discriminant within a few fp32 ulps of 0."""
    st = Stream("sph/tangent")
    pos = st.s(n, 3) * 5.0
    r = _f32(st.pow10(-1, 2, n))
    w = normalize(st.s(n, 3))
    d = normalize(cross(w, st.s(n, 3)))
    delta = st.s(n) * 4e-7
    q = pos + w * col(r * (1.0 + delta))
    o = q - d * col(r) * col(st.pow10(-1, 2, n))
    return _rec_sph(pos, r, o, d * col(st.pow10(-2, 2, n)))


def _s_from(name, n, dist, nonfp32=False, behind=False):
    """Origins `dist` radii from the centre (0: anywhere inside, 1: on the surface)."""
    st = Stream("sph/" + name)
    pos = st.s(n, 3) * 5.0
    r = st.pow10(-1, 1, n)
    if not nonfp32:
        r = _f32(r)
    u = normalize(st.s(n, 3))
    if dist == 0:
        o = pos + u * col(r * st.u(n))
    else:
        o = pos + u * col(r * dist)
    tgt = pos + st.s(n, 3) * col(r) * col(np.where(np.arange(n) % 3 == 2, 1.6, 0.57))
    d = (o - tgt) if behind else (tgt - o)
    return _rec_sph(pos, r, o, d)


SPHERE_CLASSES = [
    ("dx", lambda: _s_axis("dx", 6000, ())),
    ("dx0", lambda: _s_axis("dx0", 6000, (0,))),
    ("dxy0", lambda: _s_axis("dxy0", 6000, (0, 1))),
    ("zero_d", lambda: _s_axis("zero_d", 1000, (0, 1, 2))),
    ("tangent", lambda: _s_tangent(16000)),
    ("inside", lambda: _s_from("inside", 5000, 0)),
    ("surface", lambda: _s_from("surface", 5000, 1)),
    ("far_1e3", lambda: _s_from("far_1e3", 5000, 1e3)),
    ("far_1e6", lambda: _s_from("far_1e6", 5000, 1e6)),
    ("behind", lambda: _s_from("behind", 5000, 4.0, behind=True)),
    ("radius_not_fp32", lambda: _s_from("radius_not_fp32", 5000, 5.0, nonfp32=True)),
]

_CLASSES = {"tris": TRI_CLASSES, "boxes": BOX_CLASSES, "spheres": SPHERE_CLASSES}
_cache: dict = {}


def cases(kind: str):
    """(recs (n, width) float64, class names, class index per record (n,) int32); computed once per process."""
    if kind not in _cache:
        parts, cls = [], []
        for k, (_, make) in enumerate(_CLASSES[kind]):
            with np.errstate(all="ignore"):
                a = np.ascontiguousarray(make(), np.float64)
            assert a.shape[1] == WIDTH[kind]
            parts.append(a)
            cls.append(np.full(a.shape[0], k, np.int32))
        recs = np.ascontiguousarray(np.concatenate(parts))
        recs.setflags(write=False)
        _cache[kind] = (recs, [name for name, _ in _CLASSES[kind]], np.concatenate(cls))
    return _cache[kind]


def digest(recs: np.ndarray) -> str:
    return hashlib.sha256(np.ascontiguousarray(recs, "<f8").tobytes()).hexdigest()
