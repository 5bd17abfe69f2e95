"""Helpers shared by the tests: load the CPU oracle (oracle/_build/libgi_oracle.so), run the
compiled reference harness (oracle/_ref/ref_harness, only where /root/reference was present at
build time), and read/write golden fixtures.  Test infrastructure only."""
from __future__ import annotations

import ctypes
import hashlib
import importlib
import os
import struct
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_SO = os.path.join(ROOT, "oracle", "_build", "libgi_oracle.so")
REF_HARNESS = os.path.join(ROOT, "oracle", "_ref", "ref_harness")
REF_RUN = os.path.join(ROOT, "oracle", "_ref", "ref_run")
GOLDEN = os.path.join(ROOT, "tests", "golden")


def pkg():
    """The product package (its directory name starts with a digit, so import by string)."""
    return importlib.import_module("2019global_amd")


def scenes():
    return importlib.import_module("2019global_amd.scenes")


_oracle = None


def oracle():
    global _oracle
    if _oracle is None:
        if not os.path.exists(ORACLE_SO):
            subprocess.run(["make", "-C", os.path.join(ROOT, "oracle"), "oracle"], check=True,
                           stdout=subprocess.DEVNULL)
        lib = ctypes.CDLL(ORACLE_SO)
        i32p = ctypes.POINTER(ctypes.c_int32)
        f64p = ctypes.POINTER(ctypes.c_double)
        lib.gio_render.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                   ctypes.c_int, ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                   ctypes.c_int, ctypes.c_int, f64p, i32p, i32p, i32p, i32p,
                                   ctypes.POINTER(ctypes.c_uint8)]
        lib.gio_tree.argtypes = [ctypes.c_char_p, ctypes.c_char_p, ctypes.c_long]
        lib.gio_tree.restype = ctypes.c_long
        lib.gio_rays.argtypes = [ctypes.c_char_p, ctypes.c_int, f64p, i32p, f64p, i32p]
        lib.gio_boxes.argtypes = [ctypes.c_int, f64p, i32p]
        lib.gio_prims.argtypes = [ctypes.c_int, ctypes.c_int, f64p, i32p, f64p]
        lib.gio_last_error.restype = ctypes.c_char_p
        lib.gio_set_accel.argtypes = [ctypes.c_int]
        lib.gio_set_no_shadow.argtypes = [ctypes.c_int]
        lib.gio_time_rows.argtypes = [ctypes.c_char_p, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                      ctypes.c_uint64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, f64p,
                                      f64p, ctypes.POINTER(ctypes.c_uint8)]
        lib.gio_x_query.argtypes = [ctypes.c_char_p, ctypes.c_int, f64p, i32p, f64p, i32p, i32p, f64p, i32p, i32p]
        _oracle = lib
    return _oracle


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def oracle_render(scn: str, w: int, h: int, mode: int = 0, spp: int = 1, depth: int = 1, seed: int = 0,
                  window=None, threads: int = 0) -> dict:
    x0, y0, x1, y1 = window if window is not None else (0, 0, w, h)
    n = (x1 - x0) * (y1 - y0)
    out = dict(rgb=np.zeros((n, 3)), hit=np.zeros(n, np.int32), uv=np.zeros((n, 2), np.int32),
               ncand=np.zeros(n, np.int32), nnode=np.zeros(n, np.int32), q=np.zeros((n, 3), np.uint8))
    lib = oracle()
    rc = lib.gio_render(scn.encode(), w, h, mode, spp, depth, seed, x0, y0, x1, y1, threads,
                        _p(out["rgb"], ctypes.c_double), _p(out["hit"], ctypes.c_int32),
                        _p(out["uv"], ctypes.c_int32), _p(out["ncand"], ctypes.c_int32),
                        _p(out["nnode"], ctypes.c_int32), _p(out["q"], ctypes.c_uint8))
    if rc != 0:
        raise RuntimeError(f"gio_render failed ({rc}): {lib.gio_last_error().decode()}")
    return out


def oracle_time_rows(scn: str, w: int, h: int, spp: int, depth: int, seed: int, row0: int, stride: int, n_rows: int,
                     threads: int = 0, pixels: bool = False) -> dict:
    """Mode X over the full-width rows row0 + k*stride (bench.py's cpu_baseline; the whole-frame and
    strided-row parity tests): rays traced, primary samples resolved by the scene-box test (not
    traced), pixels, radiance sum; with pixels=True also the rows' pixels as gio_render writes them
    ("rows": the row indices, "rgb": (rows, w, 3) fp64, "q": (rows, w, 3) RGB888)."""
    rows = [row0 + k * stride for k in range(n_rows) if row0 + k * stride < h]
    out = np.zeros(4)
    rgb = np.zeros((len(rows), w, 3)) if pixels else None
    q = np.zeros((len(rows), w, 3), np.uint8) if pixels else None
    lib = oracle()
    rc = lib.gio_time_rows(scn.encode(), w, h, spp, depth, seed, row0, stride, n_rows, threads, _p(out, ctypes.c_double),
                           _p(rgb, ctypes.c_double) if pixels else None, _p(q, ctypes.c_uint8) if pixels else None)
    if rc != 0:
        raise RuntimeError(f"gio_time_rows failed ({rc}): {lib.gio_last_error().decode()}")
    r = {"rays": int(out[0]), "resolved": int(out[1]), "pixels": int(out[2]), "sum": float(out[3])}
    if pixels:
        r.update(rows=rows, rgb=rgb, q=q)
    return r


def oracle_no_shadow(on: bool) -> None:
    """Mode X without shadow rays (the oracle side of GI_FLAG_X_NO_SHADOW)."""
    oracle().gio_set_no_shadow(1 if on else 0)


def oracle_accel(mode: int) -> None:
    """Mode X queries: -1 default (BVH above 256 primitives), 0 brute force, 1 BVH."""
    oracle().gio_set_accel(mode)


def oracle_x_query(scn: str, recs: np.ndarray) -> dict:
    """Ray-level Mode X queries (gio_x_query) over records (o, d, light, d2) of 12 doubles: prim1, t1,
    occl, prim2, t2 and the tie counts nties1, nties2.  oracle_accel() chooses brute force or the BVH."""
    recs = np.ascontiguousarray(recs, np.float64).reshape(-1, 12)
    n = recs.shape[0]
    out = dict(prim1=np.zeros(n, np.int32), t1=np.zeros(n), occl=np.zeros(n, np.int32), prim2=np.zeros(n, np.int32),
               t2=np.zeros(n), nties1=np.zeros(n, np.int32), nties2=np.zeros(n, np.int32))
    lib = oracle()
    rc = lib.gio_x_query(scn.encode(), n, _p(recs, ctypes.c_double), _p(out["prim1"], ctypes.c_int32),
                         _p(out["t1"], ctypes.c_double), _p(out["occl"], ctypes.c_int32),
                         _p(out["prim2"], ctypes.c_int32), _p(out["t2"], ctypes.c_double),
                         _p(out["nties1"], ctypes.c_int32), _p(out["nties2"], ctypes.c_int32))
    if rc != 0:
        raise RuntimeError(f"gio_x_query failed ({rc}): {lib.gio_last_error().decode()}")
    return out


def oracle_tree(scn: str) -> str:
    lib = oracle()
    n = lib.gio_tree(scn.encode(), None, 0)
    buf = ctypes.create_string_buffer(n + 1)
    lib.gio_tree(scn.encode(), buf, n + 1)
    return buf.value.decode()


def oracle_rays(scn: str, rays: np.ndarray, n_ent: int) -> dict:
    rays = np.ascontiguousarray(rays, np.float64)
    n = rays.shape[0]
    hit = np.zeros((n, n_ent), np.int32)
    pn = np.zeros((n, n_ent, 6))
    uv = np.zeros((n, n_ent, 2), np.int32)
    rc = oracle().gio_rays(scn.encode(), n, _p(rays, ctypes.c_double), _p(hit, ctypes.c_int32),
                           _p(pn, ctypes.c_double), _p(uv, ctypes.c_int32))
    assert rc == 0
    return dict(hit=hit, pn=pn, uv=uv)


def oracle_boxes(recs: np.ndarray) -> np.ndarray:
    recs = np.ascontiguousarray(recs, np.float64)
    out = np.zeros(recs.shape[0], np.int32)
    assert oracle().gio_boxes(recs.shape[0], _p(recs, ctypes.c_double), _p(out, ctypes.c_int32)) == 0
    return out


PRIM_KINDS = {"tris": (0, 15), "spheres": (1, 10), "boxes": (2, 12)}   # kind -> (gio_prims kind, record width)


def oracle_prims(kind: str, recs: np.ndarray) -> dict:
    """The oracle's own primitive routines over r_prims_cases records (gio_prims): hit (n,) int32 and
    pn (n, 6) = P, N, zeros on a miss and for boxes."""
    k, width = PRIM_KINDS[kind]
    recs = np.ascontiguousarray(recs, np.float64).reshape(-1, width)
    n = recs.shape[0]
    hit = np.zeros(n, np.int32)
    pn = np.zeros((n, 6))
    rc = oracle().gio_prims(k, n, _p(recs, ctypes.c_double), _p(hit, ctypes.c_int32), _p(pn, ctypes.c_double) if k < 2 else None)
    assert rc == 0, rc
    return dict(hit=hit, pn=pn)


PRIM_BLOCK, PRIM_SAMPLES = 512, 64


def prims_summary(hit: np.ndarray, pn: np.ndarray, cls: np.ndarray, n_classes: int) -> dict:
    """What tests/golden/adv_*.npz keep of a primitive run (make_golden.py `adversarial`): the packed hit
    bits, the hit count per class, the sha256 of the P|N bit patterns of every block of PRIM_BLOCK cases
    (misses contribute their zeros) and P, N in full for the first PRIM_SAMPLES hits of every class."""
    hit = np.ascontiguousarray(hit, np.int32)
    pn = np.ascontiguousarray(pn, "<f8").reshape(-1, 6)
    n = hit.shape[0]
    blocks = np.array([np.frombuffer(hashlib.sha256(pn[b:b + PRIM_BLOCK].tobytes()).digest(), np.uint8)
                       for b in range(0, n, PRIM_BLOCK)])
    idx = np.concatenate([np.flatnonzero((cls == k) & (hit != 0))[:PRIM_SAMPLES] for k in range(n_classes)])
    return dict(hit_bits=np.packbits(hit != 0), class_hits=np.array([int(hit[cls == k].sum()) for k in range(n_classes)], np.int64),
                block_sha256=blocks, sample_index=idx.astype(np.int64), sample_pn=pn[idx].view("<u8"))


_prims_expected: dict = {}


def prims_expected(kind: str) -> dict:
    """The adversarial records of `kind` with the oracle's per-case answers, after the two checks that make
    them the compiled reference's: the generator's sha256 equals the fixture's, and the oracle's summary equals
    the fixture's (hit bits, per-class hit counts, every block digest, the stored P, N samples).  Computed once
    per process; the arrays are read-only."""
    if kind not in _prims_expected:
        import r_prims_cases as C
        z = np.load(os.path.join(GOLDEN, f"adv_{kind}.npz"))
        recs, names, cls = C.cases(kind)
        assert C.digest(recs) == str(z["inputs_sha256"]), f"{kind}: r_prims_cases no longer generates the fixture's records"
        assert names == [str(x) for x in z["class_names"]]
        assert [int((cls == k).sum()) for k in range(len(names))] == z["class_counts"].tolist()
        o = oracle_prims(kind, recs)
        s = prims_summary(o["hit"], o["pn"], cls, len(names))
        ref_hit = np.unpackbits(z["hit_bits"])[:recs.shape[0]]
        bad = np.flatnonzero(ref_hit != (o["hit"] != 0))
        assert bad.size == 0, (f"{kind}: the oracle's hit differs from the reference's on {bad.size} cases; first: case {bad[0]} "
                               f"class {names[cls[bad[0]]]} record {recs[bad[0]].tolist()} reference {ref_hit[bad[0]]} oracle {o['hit'][bad[0]]}")
        assert s["class_hits"].tolist() == z["class_hits"].tolist()
        blk = np.flatnonzero((s["block_sha256"] != z["block_sha256"]).any(1))
        assert blk.size == 0, f"{kind}: the oracle's P|N differ from the reference's in {blk.size} blocks of {PRIM_BLOCK}; first block {blk[:1]}"
        assert (s["sample_index"] == z["sample_index"]).all() and (s["sample_pn"] == z["sample_pn"]).all()
        for a in (o["hit"], o["pn"]):
            a.setflags(write=False)
        _prims_expected[kind] = dict(recs=recs, names=names, cls=cls, hit=o["hit"], pn=o["pn"])
    return _prims_expected[kind]


def assert_prims_equal(kind: str, what: str, hit: np.ndarray, pn=None, n=None) -> None:
    """`hit` (and `pn`, bit for bit) of the first n adversarial cases equal the oracle's on every case: nothing
    excluded, no tolerance.  A failure names the first differing case."""
    e = prims_expected(kind)
    n = e["recs"].shape[0] if n is None else n
    hit = np.asarray(hit).reshape(-1)
    assert hit.shape[0] == n
    bad = (hit != 0) != (e["hit"][:n] != 0)
    if pn is not None:
        bad |= ~bits_equal(np.asarray(pn).reshape(n, 6), e["pn"][:n]).all(1)
    idx = np.flatnonzero(bad)
    if idx.size:
        i = int(idx[0])
        per = {e["names"][k]: int((e["cls"][idx] == k).sum()) for k in sorted(set(e["cls"][idx].tolist()))}
        raise AssertionError(f"{kind} / {what}: {idx.size} of {n} cases differ from the oracle, by class {per}; first: case {i} class "
                             f"{e['names'][e['cls'][i]]} record {e['recs'][i].tolist()} got hit {int(hit[i])} pn "
                             f"{None if pn is None else np.asarray(pn).reshape(n, 6)[i].tolist()} expected hit {int(e['hit'][i])} pn {e['pn'][i].tolist()}")


# ---- compiled reference (oracle/_ref) -------------------------------------------------------

def have_ref() -> bool:
    return os.path.exists(REF_HARNESS)


def ref_render(scn: str, w: int, h: int, window=None, stride: int = 1) -> dict:
    with tempfile.TemporaryDirectory() as td:
        sp = os.path.join(td, "s.scn")
        op = os.path.join(td, "o.bin")
        open(sp, "w").write(scn)
        args = [REF_HARNESS, "render", sp, str(w), str(h), op]
        if window is not None or stride != 1:
            x0, y0, x1, y1 = window if window is not None else (0, 0, w, h)
            args += [str(x0), str(y0), str(x1), str(y1), str(stride)]
        subprocess.run(args, check=True, stdout=subprocess.DEVNULL)   # ExpRectangle prints (entities.h:362)
        return read_ref_render(open(op, "rb").read())


def read_ref_render(b: bytes) -> dict:
    assert b[:6] == b"GIREF1"
    w, h, n, _ = struct.unpack("<4i", b[8:24])
    off = 24

    def take(dtype, count):
        nonlocal off
        a = np.frombuffer(b, dtype=dtype, count=count, offset=off)
        off += a.nbytes
        return a.copy()

    xs = take(np.int32, n)
    ys = take(np.int32, n)
    rgb = take(np.float64, 3 * n).reshape(n, 3)
    hit = take(np.int32, n)
    uv = take(np.int32, 2 * n).reshape(n, 2)
    ncand = take(np.int32, n)
    nnode = take(np.int32, n)
    q = take(np.uint8, 3 * n).reshape(n, 3)
    return dict(w=w, h=h, x=xs, y=ys, rgb=rgb, hit=hit, uv=uv, ncand=ncand, nnode=nnode, q=q)


def ref_tree(scn: str) -> str:
    with tempfile.TemporaryDirectory() as td:
        sp = os.path.join(td, "s.scn")
        open(sp, "w").write(scn)
        return subprocess.run([REF_HARNESS, "tree", sp], check=True, capture_output=True, text=True).stdout


def ref_rays(scn: str, rays: np.ndarray, n_ent: int) -> dict:
    with tempfile.TemporaryDirectory() as td:
        sp, rp, op = (os.path.join(td, f) for f in ("s.scn", "r.bin", "o.bin"))
        open(sp, "w").write(scn)
        with open(rp, "wb") as f:
            f.write(struct.pack("<i", rays.shape[0]))
            f.write(np.ascontiguousarray(rays, "<f8").tobytes())
        subprocess.run([REF_HARNESS, "rays", sp, rp, op], check=True, stdout=subprocess.DEVNULL)
        rec = np.dtype([("hit", "<i4"), ("pn", "<f8", 6), ("uv", "<i4", 2)])
        a = np.frombuffer(open(op, "rb").read(), dtype=rec).reshape(rays.shape[0], n_ent)
        return dict(hit=a["hit"].copy(), pn=a["pn"].copy(), uv=a["uv"].copy())


def ref_boxes(recs: np.ndarray) -> np.ndarray:
    with tempfile.TemporaryDirectory() as td:
        rp, op = os.path.join(td, "r.bin"), os.path.join(td, "o.bin")
        with open(rp, "wb") as f:
            f.write(struct.pack("<i", recs.shape[0]))
            f.write(np.ascontiguousarray(recs, "<f8").tobytes())
        subprocess.run([REF_HARNESS, "boxes", rp, op], check=True)
        return np.frombuffer(open(op, "rb").read(), dtype="<i4").copy()


def _ref_prims(mode: str, recs: np.ndarray) -> dict:
    with tempfile.TemporaryDirectory() as td:
        rp, op = os.path.join(td, "r.bin"), os.path.join(td, "o.bin")
        with open(rp, "wb") as f:
            f.write(struct.pack("<i", recs.shape[0]))
            f.write(np.ascontiguousarray(recs, "<f8").tobytes())
        subprocess.run([REF_HARNESS, mode, rp, op], check=True)
        a = np.fromfile(op, dtype=np.dtype([("hit", "<i4"), ("pn", "<f8", 6)]))
        assert a.shape[0] == recs.shape[0]
        return dict(hit=a["hit"].copy(), pn=a["pn"].copy())


def ref_tris(recs: np.ndarray) -> dict:
    """ImpTriangle::intersect over records p1 p2 p3 o dir (15 doubles): hit, pn = P, N (zeros on a miss)."""
    return _ref_prims("tris", np.asarray(recs).reshape(-1, 15))


def ref_spheres(recs: np.ndarray) -> dict:
    """ImpSphere::intersect over records pos radius o dir (10 doubles): hit, pn = P, N (zeros on a miss)."""
    return _ref_prims("spheres", np.asarray(recs).reshape(-1, 10))


def dropin_demo() -> str:
    """integration/_build/dropin_demo (the reference app's classes + the C++ drop-in headers; built by
    integration/Makefile where the reference tree exists).  Skips when it was never built; FAILS when
    it was built against a gi.h of another GI_ABI_VERSION than the tree's (a stale build travelled
    with the snapshot: it would refuse every render)."""
    import pytest
    import re
    exe = os.path.join(ROOT, "integration", "_build", "dropin_demo")
    if not os.path.exists(exe):
        pytest.skip("integration/_build/dropin_demo not built (needs the reference tree)")
    want = re.search(r"#define GI_ABI_VERSION (\d+)", open(os.path.join(ROOT, "include", "gi.h")).read()).group(1)
    got = subprocess.run([exe, "--abi"], capture_output=True, text=True, timeout=60).stdout.strip()
    assert got == want, f"stale {exe}: built against GI_ABI_VERSION {got!r}, the tree's gi.h has {want} (rebuild: make -C integration)"
    return exe


def whole_frame_digest(rgb: np.ndarray, q: np.ndarray) -> dict:
    """Digests of a whole frame (tests/golden/whole_*.json, make_golden.py `whole`): rgb (h, w, 3) fp64
    radiance, q (h, w, 3) RGB888.  The sha256 of the RGB888 frame and of each of its rows (the exact
    bar), and per row the fp64 channel sums over its non-NaN pixels and its NaN count (compared within
    1e-5 relative: the device's acos / sin / pow may differ from libm by an ulp)."""
    h = q.shape[0]
    nan = np.isnan(rgb).any(axis=2)
    sums = np.where(nan[:, :, None], 0.0, rgb).sum(axis=1)   # (h, 3)
    return dict(rgb8_sha256=hashlib.sha256(np.ascontiguousarray(q).tobytes()).hexdigest(),
                row_rgb8_sha256=[hashlib.sha256(np.ascontiguousarray(q[y]).tobytes()).hexdigest()[:16] for y in range(h)],
                row_sum=sums.tolist(), row_nan=nan.sum(axis=1).astype(int).tolist())


def bits_equal(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Elementwise bit equality of float64 arrays (NaN == NaN when the payload matches)."""
    return np.ascontiguousarray(a, np.float64).view(np.int64) == np.ascontiguousarray(b, np.float64).view(np.int64)


# ---- reduced Mode X against the reference --------------------------------
# Mode X at depth 1, 1 spp, without shadow rays (GI_FLAG_X_NO_SHADOW) is the reference's own
# per-pixel shading (raytracer.h:41-84, material.h:48-62) with three semantic differences, each of
# which is a class of excluded pixels, counted exactly per fixture:
#   ent  - a different entity: the reference keeps the LAST hitting candidate of Octree::intersect's
#          list and loses entities the octree drops (A.6); Mode X takes the closest hit
#          over all entities;
#   tex  - same entity, different texel (u, v): the reference's hit point differs in rounding (fp32
#          sphere root, A.2; glm's inverse for triangles, A.3) and its acos is libm's, so the x86 int()
#          truncation of the texture coordinate (A.9) can land on the other side of a texel edge;
#   far  - same entity and texel, but beyond 1e-5 relative in some channel: only scenes with
#          ImpSpheres (the reference's fp32 root moves the hit point by ~1e-7 relative, A.2) or an
#          ExpCone (float height and radius in its constructor, entities.h:823); always within ANCHOR_ABS.
# Every other pixel must be within 1e-5 relative per channel of the reference's radiance (the
# north_star tolerance); `exact` counts the bit-identical ones.  ExpBox frames (and the zoo, which
# has one) are left out: ExpBox::intersect keeps the LAST face hit, not the nearest
# (entities.h:421-437, min_dist_square reset per face), so its point and normal differ by design.
# The fixtures' pixel sets are the goldens' own (tests/golden/*.npz).
ANCHOR_ABS = 3e-5
ANCHOR = {   # fixture: (ent, tex, far, exact) -- pinned from the oracle (the device is bit-identical)
    "sphere_256x256": (0, 2, 2308, 36706),
    "cornell_128x128": (7673, 4, 0, 4583),
    "cornell_512x512_s61": (2398, 0, 0, 497),
    "cornell_1920x1080_s509": (179, 0, 0, 3745),
    "main_200x200": (297, 1813, 122, 25122),
    "soup1000_160x160": (658, 1, 0, 24087),
    "soup100000_1920x1080_win700-600-1220-1080_s29": (4191, 1, 0, 3517),
    "only_exprectangle_96x96": (79, 0, 0, 4625),
    "only_expcone_96x96": (96, 2, 8, 2315),
    "only_expcube_96x96": (96, 231, 0, 0),
}


def anchor_counts(rgb, hit, uv, z):
    """(ent, tex, far, exact, max |error| over `far`) of a reduced Mode X frame at the fixture's
    pixels: `hit`/`uv` are Mode X's primary hit entity and texel (the oracle's), `z` the fixture."""
    rgb = np.asarray(rgb, np.float64)
    same_ent = hit == z["hit"]
    same = same_ent & (uv == z["uv"]).all(1)
    err = np.abs(rgb - z["rgb"])
    within = (err <= 1e-5 * np.maximum(np.abs(z["rgb"]), 1e-300)).all(1)
    far = same & ~within
    exact = same & bits_equal(rgb, z["rgb"]).all(1)
    return (int((~same_ent).sum()), int((same_ent & ~same).sum()), int(far.sum()), int(exact.sum()),
            float(err[far].max()) if far.any() else 0.0)
