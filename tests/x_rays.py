"""Seeded ray sets for the ray-level Mode X query tests (pure numpy; no device, no oracle).

A record is 12 doubles, o[3], d[3], light[3], d2[3]: the ray of a path segment, the point light its
hit point is shaded from, and the direction the path leaves the hit point in (gi_kat_x_query on the
device, gio_x_query in the oracle).  Rays are built from the scene's own vertices and bounds so that
they sit on the edges of the queries' arithmetic: box planes, shared edges, vertices, zero and
underflowing direction components, origins inside leaf boxes and far outside the scene, and
directions around the own-plane skip's bound on |d . n|.

Two steps, because hop 2 starts at hop 1's hit point: hop1() makes origins and directions by class;
complete() takes the reference's hop-1 answer (primitive, t) and adds each ray's light and d2 by
class.  Every class is a name in H1 / H2 / LIGHTS; the tests count rays per class.
"""
import numpy as np

import oracle_util as U

S = U.scenes()

H1 = ("rand_in", "rand_out", "axis1", "axis2", "centre", "in_box", "at_vertex", "shared_edge", "edge_axis",
      "bounds_edge_mid", "tiny_1e-20", "tiny_1e-45", "away", "far_1e3", "far_1e6")
# u + c n for c = k * skip_cos (the "sc" classes) or an absolute c; then random hemispheres and the reverse ray
H2_C = (("c0", 0.0, 0.0), ("c+1e-12", 0.0, 1e-12), ("c-1e-12", 0.0, -1e-12), ("c+0.5sc", 0.5, 0.0), ("c-0.5sc", -0.5, 0.0),
        ("c+sc(1-1e-3)", 1.0 - 1e-3, 0.0), ("c-sc(1-1e-3)", -(1.0 - 1e-3), 0.0), ("c+sc(1+1e-3)", 1.0 + 1e-3, 0.0),
        ("c-sc(1+1e-3)", -(1.0 + 1e-3), 0.0), ("c+2sc", 2.0, 0.0), ("c-2sc", -2.0, 0.0), ("c+0.5", 0.0, 0.5),
        ("c-0.5", 0.0, -0.5))
H2 = tuple(c[0] for c in H2_C) + ("hemi_front", "hemi_back", "reverse")
LIGHTS = ("scene", "inside", "graze_plane", "behind", "near_1e-7", "far_1e6")
FAR = {"far_1e3": 1e3, "far_1e6": 1e6}


class Frame:
    """The frame a set's generators work in: the scene's coordinates are x -> s x + off of a base scene's
    (x_scenes.placed).  Lengths that are absolute in the base frame are multiplied by s, the Cornell
    blocks' boxes are mapped, and `far` gives the far classes' distances.  The base frame (s = 1, no
    offset) measures them in extents from the scene's centre, FAR; a placed frame in E = max
    |coordinate| of the placed scene from the WORLD origin, 32 E and 1e3 E by default -- both beyond
    the 16 E from which the device tests a ray from a point near the scene (gi_dev.h ray_org32), and
    near enough for a sphere's quadratic: from 1e6 extents beyond a scene that itself lies 2^20 from
    the origin a unit sphere's discriminant b^2 - c2 is rounding alone (phantom hits of brute force).
    `share` gives a hop-1 class that many equal shares of the set instead of one: the placed sets hold
    1061 rays, a quarter of the base Cornell set, and edge_axis -- whose every ray meets two triangles
    at one t -- takes two shares there, so that a placed set of the Cornell family still holds at least
    170 ties."""

    def __init__(self, s=1.0, off=(0.0, 0.0, 0.0), far=None, share=None):
        self.s, self.off = float(s), np.asarray(off, np.float64)
        self.placed = far is not None
        self.far = dict(far) if far is not None else dict(FAR)
        self.share = dict(share or {})

    def map(self, p):
        return self.s * np.asarray(p, np.float64) + self.off


BASE = Frame()
PLACED_FAR = {"far_1e3": 32.0, "far_1e6": 1e3}
PLACED_SHARE = {"edge_axis": 2}


def unit(v):
    v = np.asarray(v, np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = v / np.sqrt((v * v).sum(-1, keepdims=True))
    bad = ~np.isfinite(r).all(-1)
    r[bad] = (1.0, 0.0, 0.0)
    return r


class Geo:
    """What the generators need of a scene: per Mode X primitive its triangle (NaN rows: a sphere, or a
    primitive of a meshed entity, whose index this module does not derive), the bounds, the pool of
    vertex and bound coordinates per axis, shared edges and boxes to start rays inside."""

    def __init__(self, sc, frame=BASE):
        tri, known = [], True
        pts = []
        for e in sc.entities:
            if e.kind == S.IMP_TRIANGLE:
                t = np.array(e.args[:9]).reshape(3, 3)
                pts.append(t)
                if known:
                    tri.append(t)
            elif e.kind == S.IMP_SPHERE:
                c, r = np.array(e.args[:3]), float(np.float32(e.args[3]))
                pts.append(np.array([c - r, c + r, c]))
                if known:
                    tri.append(np.full((3, 3), np.nan))
            else:   # a meshed entity: several primitives; the ones after it stay unnumbered
                known = False
                c = np.array(e.args[:3])
                pts.append(np.array([c - 3.0, c + 3.0, c]))
        self.ptri = np.array(tri).reshape(-1, 3, 3)
        self.tris = self.ptri[~np.isnan(self.ptri).any((1, 2))] if len(tri) else np.zeros((0, 3, 3))
        allp = np.concatenate(pts).reshape(-1, 3) if pts else np.array([[-1.0, -1.0, -1.0], [1.0, 1.0, 1.0]])
        self.lo, self.hi = allp.min(0), allp.max(0)
        self.hi = np.where(self.hi > self.lo, self.hi, self.lo + 1.0)
        self.centre = 0.5 * (self.lo + self.hi)
        self.half = 0.5 * (self.hi - self.lo)
        self.ext = float(np.abs(np.concatenate([self.lo, self.hi])).max())
        vs = self.tris.reshape(-1, 3) if len(self.tris) else allp
        self.coords = [np.unique(np.concatenate([vs[:, k], [self.lo[k], self.hi[k]]])) for k in range(3)]
        # shared edges: two triangles with two vertices in common; `axis` when both lie in one axis plane
        edges = {}
        for i, t in enumerate(self.tris):
            for a, b in ((0, 1), (1, 2), (2, 0)):
                key = tuple(sorted((tuple(t[a]), tuple(t[b]))))
                edges.setdefault(key, []).append(i)
        self.shared, self.shared_axis = [], []
        for (a, b), ts in edges.items():
            if len(ts) < 2:
                continue
            a, b = np.array(a), np.array(b)
            self.shared.append((a, b))
            flat = [k for k in range(3) if all((self.tris[i][:, k] == a[k]).all() for i in ts[:2])]
            if flat:
                self.shared_axis.append((a, b, flat[0]))
        name = getattr(sc, "name", "")
        if name.startswith("cornell") or name.startswith("grazing"):   # the Cornell box's two blocks
            self.boxes = [(frame.map([5.0, -3.5, -5.0]), frame.map([7.5, -1.0, -2.0])),
                          (frame.map([6.5, 0.5, -5.0]), frame.map([9.0, 3.0, 0.5]))]
        else:   # triangles' own boxes: origins inside leaf boxes
            self.boxes = [(t.min(0), t.max(0)) for t in self.tris[:: max(1, len(self.tris) // 64)]]


def hop1(sc, n, seed, frame=BASE):
    """n rays (o, d unit, class index into H1).  Classes a scene cannot have (no triangles, no shared
    edge) give their share to the random classes."""
    g = Geo(sc, frame)
    rng = np.random.default_rng(seed)
    per = max(1, n // (len(H1) + sum(v - 1 for v in frame.share.values())))
    o_all, d_all, c_all = [], [], []

    def inside(m):
        return g.lo + rng.random((m, 3)) * (g.hi - g.lo)

    def outside(m):   # within 1.5 half-extents of the centre, beyond the bounds on one axis at least
        p = g.centre + (2.0 * rng.random((m, 3)) - 1.0) * g.half
        k = rng.integers(0, 3, m)
        s = np.where(rng.random(m) < 0.5, -1.0, 1.0)
        p[np.arange(m), k] = g.centre[k] + s * g.half[k] * (1.05 + 0.45 * rng.random(m))
        return p

    def target(m):   # a point of the geometry: on a random triangle, else anywhere inside the bounds
        if not len(g.tris):
            return inside(m)
        t = g.tris[rng.integers(0, len(g.tris), m)]
        b = rng.dirichlet((1.0, 1.0, 1.0), m)
        return (t * b[:, :, None]).sum(1)

    def anywhere(m):
        return np.where((rng.random(m) < 0.5)[:, None], inside(m), outside(m))

    def on_planes(m):   # every coordinate copied from a vertex coordinate or a bound
        return np.stack([rng.choice(g.coords[k], m) for k in range(3)], 1)

    def zeros(m):   # +0.0 and -0.0 alternately
        return np.where(np.arange(m) % 2 == 0, 0.0, -0.0)

    def emit(name, o, d):
        o_all.append(np.asarray(o, np.float64))
        d_all.append(np.asarray(d, np.float64))
        c_all.append(np.full(len(o), H1.index(name)))

    have_tri, m = len(g.tris) > 0, per
    o = outside(m)
    emit("rand_out", o, np.where((rng.random(m) < 0.5)[:, None], unit(target(m) - o), unit(rng.normal(size=(m, 3)))))
    d = unit(rng.normal(size=(m, 3)))
    d[np.arange(m), rng.integers(0, 3, m)] = zeros(m)
    emit("axis1", on_planes(m), unit(d))   # (unit() keeps a zero component's sign)
    d = np.stack([zeros(m), zeros(m)[::-1], zeros(m)], 1)
    d[np.arange(m), rng.integers(0, 3, m)] = np.where(rng.random(m) < 0.5, -1.0, 1.0)
    emit("axis2", on_planes(m), d)
    d = unit(rng.normal(size=(m, 3)))
    d[: m // 3] = np.eye(3)[rng.integers(0, 3, m // 3)] * np.where(rng.random(m // 3) < 0.5, -1.0, 1.0)[:, None]
    d[m // 3: 2 * (m // 3)] = unit(target(m // 3) - g.centre)
    emit("centre", np.tile(g.centre, (m, 1)), d)
    if g.boxes:
        bi = rng.integers(0, len(g.boxes), m)
        lo, hi = np.array([g.boxes[i][0] for i in bi]), np.array([g.boxes[i][1] for i in bi])
        emit("in_box", lo + rng.random((m, 3)) * (hi - lo), unit(rng.normal(size=(m, 3))))
    if have_tri:
        o = anywhere(m)
        emit("at_vertex", o, unit(g.tris.reshape(-1, 3)[rng.integers(0, 3 * len(g.tris), m)] - o))
    if g.shared:
        o = anywhere(m)
        ei = rng.integers(0, len(g.shared), m)
        a, b = np.array([g.shared[i][0] for i in ei]), np.array([g.shared[i][1] for i in ei])
        emit("shared_edge", o, unit(a + rng.random((m, 1)) * (b - a) - o))
    if g.shared_axis:
        # exactly through a point k/32 along a shared edge of two triangles in an axis plane, along that
        # axis from 1, 2 or 4 units off the plane: every operation of the exact tests is exact for
        # vertices with few mantissa bits, so both triangles are hit at one t
        m = per * frame.share.get("edge_axis", 1)
        ei = rng.integers(0, len(g.shared_axis), m)
        a, b = np.array([g.shared_axis[i][0] for i in ei]), np.array([g.shared_axis[i][1] for i in ei])
        ax = np.array([g.shared_axis[i][2] for i in ei])
        p = a + (rng.integers(1, 32, m) / 32.0)[:, None] * (b - a)
        sgn = np.where(p[np.arange(m), ax] > g.centre[ax], -1.0, 1.0)   # start on the scene's side of the plane
        off = np.zeros((m, 3))
        off[np.arange(m), ax] = sgn * rng.choice([1.0, 2.0, 4.0], m) * frame.s
        d = np.zeros((m, 3))
        d[np.arange(m), ax] = -sgn
        emit("edge_axis", p + off, d)
        m = per
    mids = []
    for k in range(3):   # the bounds' 12 edge midpoints
        for u in (g.lo, g.hi):
            for v in (g.lo, g.hi):
                q = g.centre.copy()
                q[(k + 1) % 3], q[(k + 2) % 3] = u[(k + 1) % 3], v[(k + 2) % 3]
                mids.append(q)
    o = anywhere(m)
    emit("bounds_edge_mid", o, unit(np.array(mids)[rng.integers(0, 12, m)] - o))
    for name, tiny in (("tiny_1e-20", 1e-20), ("tiny_1e-45", 1e-45)):
        d = unit(rng.normal(size=(m, 3)))
        k = rng.integers(0, 3, m)
        d[np.arange(m), k] = np.where(rng.random(m) < 0.5, -tiny, tiny)
        two = rng.random(m) < 0.3
        d[two, (k[two] + 1) % 3] = tiny
        emit(name, anywhere(m), unit(d))
    o = outside(m)
    emit("away", o, unit(o - g.centre))
    for name, f in frame.far.items():   # aimed at points of triangles and, every other ray, exactly at a vertex
        o = (0.0 if frame.placed else g.centre) + unit(rng.normal(size=(m, 3))) * (f * g.ext)
        aim = target(m)
        if have_tri:
            aim[::2] = g.tris.reshape(-1, 3)[rng.integers(0, 3 * len(g.tris), len(aim[::2]))]
        emit(name, o, unit(aim - o))
    rest = max(0, n - sum(len(x) for x in o_all))
    o = inside(rest)
    emit("rand_in", o, np.where((rng.random(rest) < 0.5)[:, None], unit(target(rest) - o), unit(rng.normal(size=(rest, 3)))))
    o, d, c = np.concatenate(o_all), np.concatenate(d_all), np.concatenate(c_all)
    order = rng.permutation(len(o))   # classes mixed within every wave
    return o[order], d[order], c[order]


def complete(sc, o, d, prim1, t1, skip_cos, seed, frame=BASE):
    """The records (n, 12) and each ray's H2 and LIGHTS class index (-1: no hop-1 hit, the fields are
    filler).  prim1, t1: the reference's hop-1 answer.  Hits on a primitive without a known triangle
    get random directions and lights that need no normal."""
    g = Geo(sc, frame)
    rng = np.random.default_rng(seed + 1)
    n = len(o)
    hit = prim1 >= 0
    with np.errstate(invalid="ignore"):
        P = np.where(hit[:, None], o + np.where(hit, t1, 0.0)[:, None] * d, o)
    tri = np.full((n, 3, 3), np.nan)
    ok = hit & (prim1 < len(g.ptri))
    tri[ok] = g.ptri[prim1[ok]]
    flat = ~np.isnan(tri).any((1, 2))   # a known triangle was hit
    e1, e2 = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0]
    with np.errstate(invalid="ignore"):
        nrm, tan = unit(np.cross(e1, e2)), unit(e1)
    nrm[~flat], tan[~flat] = unit(rng.normal(size=(n, 3)))[~flat], unit(rng.normal(size=(n, 3)))[~flat]
    front = np.where(((d * nrm).sum(1) < 0)[:, None], nrm, -nrm)   # the normal facing the incoming ray

    h2 = np.where(hit, rng.integers(0, len(H2), n), -1)
    h2 = np.where(hit & ~flat, H2.index("hemi_front") + (h2 % 2), h2)
    d2 = np.tile([1.0, 0.0, 0.0], (n, 1))
    for j, (_, k_sc, c_abs) in enumerate(H2_C):
        c = k_sc * skip_cos + c_abs
        d2[h2 == j] = unit(tan + c * nrm)[h2 == j]
    rnd = unit(rng.normal(size=(n, 3)))
    side = np.sign((rnd * front).sum(1))[:, None]
    d2[h2 == H2.index("hemi_front")] = (rnd * np.where(side == 0, 1.0, side))[h2 == H2.index("hemi_front")]
    d2[h2 == H2.index("hemi_back")] = (-rnd * np.where(side == 0, 1.0, side))[h2 == H2.index("hemi_back")]
    d2[h2 == H2.index("reverse")] = (-d)[h2 == H2.index("reverse")]

    lc = np.where(hit, rng.integers(0, len(LIGHTS), n), -1)
    lc = np.where(hit & ~flat & np.isin(lc, [LIGHTS.index("graze_plane"), LIGHTS.index("behind")]),
                  LIGHTS.index("inside"), lc)
    light = np.tile(np.asarray(sc.light, np.float64), (n, 1))
    ins = g.lo + rng.random((n, 3)) * (g.hi - g.lo)
    w = unit(np.cross(nrm, unit(rng.normal(size=(n, 3)))))   # a tangent: the light almost in the hit's plane
    s = frame.s   # (the light offsets are lengths of the base frame)
    cand = {"inside": ins, "graze_plane": P + (1.7 * s) * w + (1e-9 * s) * front, "behind": P - (2.0 * s) * front,
            "near_1e-7": P + (1e-7 * s) * rnd, "far_1e6": P + (1e6 * s) * unit(rng.normal(size=(n, 3)))}
    for name, v in cand.items():
        sel = lc == LIGHTS.index(name)
        light[sel] = v[sel]
    return np.concatenate([o, d, light, d2], 1), h2, lc


def ray_set(sc, n, skip_cos, seed, trace, frame=BASE):
    """The scene's whole set: dict(recs, h1, h2, light) -- trace(recs) -> dict with prim1 and t1 is the
    reference's query (hop 1 is traced once, with filler lights and directions, to place hop 2)."""
    o, d, h1 = hop1(sc, n, seed, frame)
    filler = np.concatenate([o, d, np.zeros_like(o), np.tile([1.0, 0.0, 0.0], (len(o), 1))], 1)
    r = trace(filler)
    recs, h2, lc = complete(sc, o, d, r["prim1"], r["t1"], skip_cos, seed, frame)
    return dict(recs=recs, h1=h1, h2=h2, light=lc)


def near(rs):
    """The rays that start within 2.5 extents of the origin (every class but the far ones)."""
    return ~np.isin(rs["h1"], [H1.index(k) for k in FAR])


def far_call(rs, name, ext, frame=BASE):
    """(selector, cam_pos) of a far class's call.  The own-plane skip's bound is derived for ray
    origins no farther out than the camera (skip_cos grows with max|cam.pos|, gi_build.cpp
    assign_plane_groups), so the rays that start 1e3 and 1e6 extents out run in calls of their own
    with a camera position of that magnitude; the near rays (rounding of the size of the scene's own
    coordinates, which the bound's 4 E term and its factor of 2000 cover) run with any camera."""
    return rs["h1"] == H1.index(name), (0.0, -2.0 * frame.far[name] * ext, 0.0)
