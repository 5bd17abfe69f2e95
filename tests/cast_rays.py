"""Inputs and expected answers of the batched ray query tests (gi_intersect, gi_occluded), built from
the ray-level query sets (tests/x_rays.py, tests/x_scenes.py).  Host code only (numpy); a helper, not a test.

The reference is always the oracle's brute force (gio_x_query through x_scenes.query_set): prim1, t1
of a record are the closest hit of its ray (o, d), prim2, t2 the closest hit of (P, d2) from the hit
point P = o + t1 d -- neither with an own-plane skip.  Nothing here carries a tolerance: t, the
primitive and the occlusion answer are compared exactly.

A ray of the public interface is 8 doubles: o[3], d[3], tmax, reserved.  Every builder returns a dict:
rays (n, 8), prim (n,), t (n,), occl (n,) -- the expected closest hit (a miss: -1, +inf) and any-hit
answer -- and cls (n,), each ray's class name for failure messages.  The arrays are read-only.
"""
import numpy as np

import oracle_util as U
import x_rays as R
from x_scenes import QUERY_SCENES, query_set

PERM_SEED = 2019
RAY_DOUBLES = U.pkg().RAY_DOUBLES   # the interface's record: o[3], d[3], tmax, reserved

# the kernel variant a scene's queries run (gi_kat_x_variant with flags 0), whether Mode X stages the
# scene in LDS and the bytes of its traversal node
FLAT_W4 = ("cornell", "grazing_floor", "grazing_tilted", "soup_max", "three_record_leaves", "coincident", "one_triangle",
           "empty")
FLAT_OTHER = ("cornell_mirror", "cornell_sphere")   # an ImpSphere each: not triangles only, 3 waves per SIMD
VARIANTS = {}
for _n in FLAT_W4:
    VARIANTS[_n] = (dict(LDS=True, W4=True, TRI=True, FLAT=True), 1, 256)
for _n in FLAT_OTHER:
    VARIANTS[_n] = (dict(LDS=True, W4=False, TRI=False, FLAT=True), 1, 256)
VARIANTS["soup_max_plus_1"] = (dict(LDS=True, SH=True, FLAT=False), 1, 256)
VARIANTS["corner3_octree"] = (dict(LDS=True, SH=False, FLAT=False), 1, 256)
VARIANTS["soup1000"] = (dict(LDS=False, TRI=True, CN=False, FLAT=False), 0, 256)
VARIANTS["zoo"] = (dict(LDS=False, TRI=False, CN=False, FLAT=False), 0, 256)
VARIANTS["soup_xcnode"] = (dict(LDS=False, TRI=True, CN=True, FLAT=False), 0, 128)
assert set(VARIANTS) == set(QUERY_SCENES)

# tmax of a ray whose closest hit is at t1, and of a ray that hits nothing
TMAX_HIT = (("inf", lambda t: np.full_like(t, np.inf)), ("t1", lambda t: t.copy()),
            ("nextafter(t1)", lambda t: np.nextafter(t, np.inf)), ("0.5*t1", lambda t: 0.5 * t), ("2*t1", lambda t: 2.0 * t),
            ("1e-7", lambda t: np.full_like(t, 1e-7)), ("0.0", lambda t: np.zeros_like(t)), ("-1.0", lambda t: np.full_like(t, -1.0)))
TMAX_MISS = (("miss/inf", np.inf), ("miss/1e3", 1e3))
TMAX_CLASSES = tuple(c[0] for c in TMAX_HIT) + tuple(c[0] for c in TMAX_MISS)

_cache = {}


def _frozen(key, make):
    if key not in _cache:
        out = make()
        for a in out.values():
            a.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def _pack(o, d, tmax, prim, t, cls):
    n = len(o)
    rays = np.zeros((n, RAY_DOUBLES))
    rays[:, 0:3], rays[:, 3:6], rays[:, 6] = o, d, tmax
    rays[1::2, 7] = np.nan   # the reserved field is ignored, whatever it holds
    hit = (prim >= 0) & (t < tmax)   # the interval is open: tmax == t is a miss
    return dict(rays=np.ascontiguousarray(rays), prim=np.where(hit, prim, -1).astype(np.int32),
                t=np.where(hit, t, np.inf), occl=hit.astype(np.int32), cls=np.asarray(cls))


def hop1(name):
    """(o, d) of every record, tmax = inf: the near rays and the far classes (1e3 and 1e6 extents out)
    mixed in one call by a fixed seeded permutation, so a wave holds both.  Expected: (prim1, t1)."""
    def make():
        _, _, rs, ref = query_set(name)
        p = np.random.default_rng(PERM_SEED).permutation(len(rs["recs"]))
        recs = rs["recs"][p]
        out = _pack(recs[:, 0:3], recs[:, 3:6], np.inf, ref["prim1"][p], ref["t1"][p], [R.H1[c] for c in rs["h1"][p]])
        out["index"] = p   # the record of the set each ray comes from
        return out
    return _frozen(("hop1", name), make)


def hop2_points(o, d, t1):
    """The hit points P = o + t1 d as the oracle forms them: a multiply, then an add (no fused operation)."""
    m = t1[:, None] * d
    return o + m


def hop2(name):
    """Where hop 1 hits: the ray (P, d2) from the hit point, tmax = inf.  Expected: (prim2, t2)."""
    def make():
        _, _, rs, ref = query_set(name)
        sel = np.flatnonzero(ref["prim1"] >= 0)
        recs = rs["recs"][sel]
        P = hop2_points(recs[:, 0:3], recs[:, 3:6], ref["t1"][sel])
        cls = [R.H1[a] + " -> " + R.H2[b] for a, b in zip(rs["h1"][sel], rs["h2"][sel])]
        out = _pack(P, recs[:, 9:12], np.inf, ref["prim2"][sel], ref["t2"][sel], cls)
        out["index"] = sel
        return out
    return _frozen(("hop2", name), make)


def tmax_classes(name):
    """Hop 1's rays with a finite or degenerate tmax: the hits take TMAX_HIT's classes in turn, the misses
    TMAX_MISS's.  Expected closest hit: (prim1, t1) when t1 < tmax, else a miss; occlusion: t1 < tmax."""
    def make():
        h = hop1(name)
        prim, t = h["prim"], h["t"]
        n = len(prim)
        hit = prim >= 0
        k = np.zeros(n, np.int64)
        k[hit] = np.arange(hit.sum()) % len(TMAX_HIT)
        k[~hit] = len(TMAX_HIT) + np.arange((~hit).sum()) % len(TMAX_MISS)
        tmax = np.zeros(n)
        with np.errstate(invalid="ignore"):
            for j, (_, f) in enumerate(TMAX_HIT):
                tmax[k == j] = f(t[k == j])
        for j, (_, v) in enumerate(TMAX_MISS):
            tmax[k == len(TMAX_HIT) + j] = v
        cls = [TMAX_CLASSES[a] + " / " + b for a, b in zip(k, h["cls"])]
        out = _pack(h["rays"][:, 0:3], h["rays"][:, 3:6], tmax, prim, t, cls)
        out["tclass"] = k
        out["index"] = h["index"].copy()
        return out
    return _frozen(("tmax", name), make)


def drawn(src, n, seed):
    """n rays of a built set drawn by a seeded index permutation, with the expected answers of the same
    indices (more rays than a device holds lanes: every wave's loop runs more than once)."""
    idx = np.random.default_rng(seed).permutation(n) % len(src["prim"])
    return dict(rays=np.ascontiguousarray(src["rays"][idx]), prim=src["prim"][idx], t=src["t"][idx], occl=src["occl"][idx],
                cls=src["cls"][idx])


def first_difference(exp, got):
    """None, or a message naming the first ray on which an answer differs from the expected one, with
    its class.  got: any of t, prim, occl (arrays as the device returned them)."""
    for k, a in got.items():
        b = exp[k]
        ne = (a.view(np.uint64) != np.ascontiguousarray(b).view(np.uint64)) if a.dtype == np.float64 else a != b
        if ne.any():
            i = int(np.flatnonzero(ne)[0])
            return (f"{int(ne.sum())} of {len(a)} rays differ in {k}; first: ray {i} class {exp['cls'][i]}: device "
                    + ", ".join(f"{q} {got[q][i]!r}" for q in got) + "; expected "
                    + ", ".join(f"{q} {exp[q][i]!r}" for q in got) + f"; ray {exp['rays'][i].tolist()}")
    return None
