// xshadow_leaves_check.cpp — CPU check of the light-dead leaves of the flat leaf table over
// libgi's own host scene builder and the launch's own mask (gi_build.cpp mark_boundary_leaves /
// shadow_leaves_of, gi_scene.h x_shadow_live), compiled here by g++.
//
//  * classification.  The Cornell box (argv[2]) with its own light: exactly the leaves of the five walls and of
//    the two block bottoms are dead.  A light above the ceiling: the ceiling's leaf stays live.  A light at
//    0.5 delta from a wall: that wall live; at 2 delta: dead.  A far camera, or the `full` argument: every
//    leaf.  The every-entity scene (argv[3]) and scenes of tilted quads and spheres: a leaf is marked only
//    where every primitive, sampled on its surface, lies on the marked side of the leaf's plane.
//  * rays.  For every light the claim of the rule itself: no record of a dead leaf answers the kernel's
//    exact test (x_prim_t) of a shadow ray inside (MX_TMIN, ldist) -- so the any hit over the live leaves'
//    records is the any hit over all records, with or without the own-plane skip.  Shadow rays leave hit
//    points computed as the device computes them, P = o + t d of a closest hit, toward the light as
//    x_hit_frame builds them.  On the Cornell box most primary rays aim at points 1e-12 to 1e-3 from the
//    wall-wall edges, the room's corners and the blocks' contact with the floor; the lights include ones at
//    1.001 delta from a wall and from two walls at once.  The share of shadow rays that start within 1e-6 of
//    two planes is printed.
//   xshadow_leaves_check <rays per light> <cornell.scn> <zoo.scn>
//   xshadow_leaves_check <rays per light> scenes a.scn ...   (the generic check alone per file, from the file's camera
//                                                            under the file's light, around the scene's own bounds)
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "gi.h"
#include "gi_scene.h"

using namespace gi;

static uint64_t g_rng = 0x2019;
static double urand() {
    g_rng += 0x9E3779B97F4A7C15ULL;
    uint64_t z = g_rng;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    z ^= z >> 31;
    return (double)(z >> 11) * 0x1.0p-53;
}

static double prim_t(const XHot& p, V3 o, V3 d, double tmin) {   // the kernel's x_prim_t
    if (p.kind == 0) {
        const V3 e1 = ld3(p.b), e2 = ld3(p.c);
        const V3 pv = fcross(d, e2);
        const double det = fdot(e1, pv);
        if (det == 0.0) return INFINITY;
        const V3 tv = o - ld3(p.a);
        const double un = fdot(tv, pv);
        if (det > 0.0 ? (un < 0.0 || un > det) : (un > 0.0 || un < det)) return INFINITY;
        const V3 qv = fcross(tv, e1);
        const double vn = fdot(d, qv);
        const double uvn = un + vn;
        if (det > 0.0 ? (vn < 0.0 || uvn > det) : (vn > 0.0 || uvn < det)) return INFINITY;
        const double t = fdot(e2, qv) / det;
        return (t > tmin) ? t : INFINITY;
    }
    const V3 oc = o - ld3(p.a);
    const double b = fdot(oc, d);
    const double r = p.b[0];
    const double c2 = gfma(-r, r, fdot(oc, oc));
    const double disc = gfma(b, b, -c2);
    if (disc < 0.0) return INFINITY;
    const double sq = std::sqrt(disc);
    double t = -b - sq;
    if (t > tmin) return t;
    t = -b + sq;
    return (t > tmin) ? t : INFINITY;
}
static XHot hot_of(const XPrim& p, int i) {
    XHot h;
    for (int k = 0; k < 3; ++k) { h.a[k] = p.a[k]; h.b[k] = p.b[k]; h.c[k] = p.c[k]; }
    h.prim = i;
    h.kind = p.kind;
    return h;
}

struct SceneFile {
    std::vector<gi_entity_desc> ents;
    double light[3] = {0, 0, 0}, cam[3] = {-10, 0, 0};
};
static bool read_scn(const char* path, SceneFile& sf) {
    static const struct { const char* kw; int kind; } kinds[] = {
        {"impsphere", GI_IMP_SPHERE}, {"imptriangle", GI_IMP_TRIANGLE}, {"expquad", GI_EXP_QUAD}, {"expsphere", GI_EXP_SPHERE},
        {"expcube", GI_EXP_CUBE}, {"expcone", GI_EXP_CONE}, {"exprectangle", GI_EXP_RECTANGLE}, {"expbox", GI_EXP_BOX}};
    std::ifstream f(path);
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream is(line);
        std::string kw;
        is >> kw;
        std::vector<double> v;
        double x;
        while (is >> x) v.push_back(x);
        if (kw == "light" && v.size() >= 3) { for (int k = 0; k < 3; ++k) sf.light[k] = v[k]; continue; }
        if (kw == "camera" && v.size() >= 3) { for (int k = 0; k < 3; ++k) sf.cam[k] = v[k]; continue; }
        gi_entity_desc e{};
        for (const auto& kd : kinds)
            if (kw == kd.kw) e.kind = kd.kind;
        if (e.kind == 0) continue;
        for (size_t k = 0; k < v.size() && k < 11; ++k) e.args[k] = v[k];
        sf.ents.push_back(e);
    }
    return !sf.ents.empty();
}
static bool build(std::vector<gi_entity_desc>& ents, HostScene& hs) {
    gi_scene_desc sd{};
    for (int k = 0; k < 3; ++k) { sd.octree_min[k] = -20; sd.octree_max[k] = 20; }
    sd.n_entities = (int32_t)ents.size();
    sd.entities = ents.data();
    std::string err;
    if (!build_host_scene(sd, hs, err)) { std::printf("build failed: %s\n", err.c_str()); return false; }
    return true;
}
static gi_entity_desc tri(V3 a, V3 b, V3 c) {
    gi_entity_desc e{};
    e.kind = GI_IMP_TRIANGLE;
    const double v[9] = {a.x, a.y, a.z, b.x, b.y, b.z, c.x, c.y, c.z};
    for (int k = 0; k < 9; ++k) e.args[k] = v[k];
    return e;
}

// the launch's far-camera radius as gi_capi.cpp sets DevScene::x_far_r: 16 x the root boxes' largest |coordinate|
static double far_r_of(const HostScene& hs) {
    double m = 0.0;
    for (const XFlatLeaf& f : hs.xflat)
        for (int k = 0; k < 3; ++k) m = std::max(m, (double)std::max(std::fabs(f.lo[k]), std::fabs(f.hi[k])));
    return 16.0 * m;
}
static uint32_t live_of(const HostScene& hs, const double* L, const double* cam, bool full = false) {
    const XShadowLeaves sl = shadow_leaves_of(hs);
    return x_shadow_live(sl, L, cam, far_r_of(hs), full) & sl.table_mask();
}

// the rule, independently: every primitive, sampled on its surface, on the marked side of leaf k's plane
static bool sides_hold(const HostScene& hs, int k) {
    const XLeafPlane& r = hs.xflat_plane[(size_t)k];
    const V3 n = v3(r.n[0], r.n[1], r.n[2]);
    for (const XPrim& p : hs.xprims)
        for (int s = 0; s < 64; ++s) {
            V3 x;
            if (p.kind == 0) {
                double a = s < 3 ? (s == 1) : urand(), b = s < 3 ? (s == 2) : urand();
                if (a + b > 1) { a = 1 - a; b = 1 - b; }
                x = ld3(p.a) + ld3(p.b) * a + ld3(p.c) * b;
            } else {
                const V3 u = s == 0 ? n : s == 1 ? -n : normalize(v3(urand() - 0.5, urand() - 0.5, urand() - 0.5));
                x = ld3(p.a) + u * p.b[0];
            }
            const double h = dot(n, x) - r.c;
            if ((r.sides & 1) && h < -1e-9) return false;
            if ((r.sides & 2) && h > 1e-9) return false;
        }
    return true;
}

struct RayStats { long rays = 0, edge = 0, bad = 0, dead_tests = 0; };
// shadow rays from the hit point of the primary ray o -> tgt toward L: no record of a dead leaf answers inside
// (MX_TMIN, ldist); the any hit over the live leaves equals the any hit over all
static void shadow_check(const HostScene& hs, uint32_t live, V3 o, V3 tgt, V3 L, RayStats& st) {
    if (sq3(tgt - o) == 0.0) return;
    const V3 d = normalize(tgt - o);
    double tb = INFINITY;
    for (size_t i = 0; i < hs.xprims.size(); ++i) tb = std::min(tb, prim_t(hot_of(hs.xprims[i], (int)i), o, d, 1e-7));
    if (!std::isfinite(tb)) return;
    const V3 P = o + tb * d;   // x_hit_frame
    const V3 lv = L - P;
    const double ldist = gsqrt(dot(lv, lv));
    const V3 Ld = normalize(lv);
    bool any_all = false, any_live = false;
    for (size_t k = 0; k < hs.xflat.size(); ++k) {
        const XFlatLeaf& lf = hs.xflat[k];
        const bool lv_k = (live >> k) & 1u;
        for (int j = 0; j < lf.cnt; ++j) {
            const bool hit = prim_t(hs.xhot[(size_t)lf.off + j], P, Ld, 1e-7) < ldist;
            any_all = any_all || hit;
            any_live = any_live || (hit && lv_k);
            if (!lv_k) {
                ++st.dead_tests;
                if (hit && ++st.bad < 5)
                    std::printf("dead leaf %zu record %d occludes: P (%.17g %.17g %.17g) L (%.17g %.17g %.17g)\n", k, j, P.x, P.y, P.z, L.x, L.y, L.z);
            }
        }
    }
    if (any_all != any_live) ++st.bad;
    int near = 0;
    for (const HostScene::XPlane& pl : hs.x_planes) near += std::fabs(dot(v3(pl.n[0], pl.n[1], pl.n[2]), P) - pl.c) < 1e-6;
    ++st.rays;
    st.edge += near >= 2;
}

static V3 rand_in(const double* lo, const double* hi) {
    return v3(lo[0] + urand() * (hi[0] - lo[0]), lo[1] + urand() * (hi[1] - lo[1]), lo[2] + urand() * (hi[2] - lo[2]));
}
static double tiny() { return std::pow(10.0, -12.0 + 9.0 * urand()); }   // 1e-12 .. 1e-3

// the Cornell box: a primary target 1e-12 to 1e-3 inside the room from a wall-wall edge, a corner, or a block's
// contact with the floor; else anywhere
static V3 cornell_target(int r) {
    const double lo[3] = {0, -5, -5}, hi[3] = {10, 5, 5};
    V3 t = rand_in(lo, hi);
    const int cls = r % 8;
    if (cls == 7) return t;
    if (cls <= 3) {   // an edge of two walls (x = 10, y = +-5, z = +-5), or with cls 3 a corner of three
        const int pick = (int)(urand() * 8);
        const double y = (pick & 1) ? 5 - tiny() : -5 + tiny(), z = (pick & 2) ? 5 - tiny() : -5 + tiny(), x = 10 - tiny();
        if (cls == 0) { t.y = y; t.z = z; }
        if (cls == 1) { t.x = x; t.y = y; }
        if (cls == 2) { t.x = x; t.z = z; }
        if (cls == 3) { t.x = x; t.y = y; t.z = z; }
        return t;
    }
    // the floor beside a block's side, or the side just above the floor
    const double bl[2][4] = {{5.0, -3.5, 7.5, -1.0}, {6.5, 0.5, 9.0, 3.0}};
    const double* b = bl[(int)(urand() * 2)];
    const int side = (int)(urand() * 4);
    const bool on_floor = cls <= 5;
    const double e = tiny();
    t.x = b[0] + urand() * (b[2] - b[0]);
    t.y = b[1] + urand() * (b[3] - b[1]);
    t.z = on_floor ? -5.0 : -5.0 + e;
    if (side == 0) t.x = b[0] - (on_floor ? e : 0.0);
    if (side == 1) t.x = b[2] + (on_floor ? e : 0.0);
    if (side == 2) t.y = b[1] - (on_floor ? e : 0.0);
    if (side == 3) t.y = b[3] + (on_floor ? e : 0.0);
    return t;
}

static int popc(uint32_t v) { return __builtin_popcount(v); }

static int check_cornell(const SceneFile& sf, HostScene& hs, int nrays, RayStats& total) {
    const XShadowLeaves sl = shadow_leaves_of(hs);
    const int n = (int)hs.xflat.size();
    if (!hs.x_flat_ok || sl.n != n) { std::printf("cornell: the table does not fit\n"); return 1; }
    // the leaves that lie in a wall's plane: the five walls and the two block bottoms (in the floor's plane)
    uint32_t walls = 0, ceiling = 0;
    for (int k = 0; k < n; ++k) {
        bool in_wall = true, in_ceiling = true;
        for (int j = 0; j < hs.xflat[k].cnt; ++j) {
            const XHot& h = hs.xhot[(size_t)hs.xflat[k].off + j];
            bool rec = false, rec_c = true;
            for (int pl = 0; pl < 5; ++pl) {   // x = 10, y = 5, y = -5, z = -5, z = 5
                const int ax = pl == 0 ? 0 : pl <= 2 ? 1 : 2;
                const double c = pl == 0 ? 10 : (pl == 1 || pl == 4) ? 5 : -5;
                const bool on = h.a[ax] == c && h.b[ax] == 0.0 && h.c[ax] == 0.0;
                rec = rec || on;
                if (pl == 4) rec_c = on;
            }
            in_wall = in_wall && rec;
            in_ceiling = in_ceiling && rec_c;
        }
        if (in_wall) walls |= 1u << k;
        if (in_ceiling) ceiling |= 1u << k;
    }
    const uint32_t tm = sl.table_mask();
    if (popc(walls) != 7 || popc(ceiling) != 1) { std::printf("cornell: %d wall leaves, %d ceiling leaves\n", popc(walls), popc(ceiling)); return 1; }
    if (sl.boundary_mask() != walls) { std::printf("cornell: boundary mask %08x, walls %08x\n", sl.boundary_mask(), walls); return 1; }
    const uint32_t own = live_of(hs, sf.light, sf.cam);
    if (own != (tm & ~walls)) { std::printf("cornell: own light live %08x, want %08x\n", own, tm & ~walls); return 1; }
    const double outside[3] = {5, 0, 7};
    const uint32_t out_live = live_of(hs, outside, sf.cam);
    if (!(out_live & ceiling) || popc(tm & ~out_live) != 6) { std::printf("cornell: light above the ceiling: live %08x\n", out_live); return 1; }
    const double far_cam[3] = {-1000, 0, 0};
    if (live_of(hs, sf.light, far_cam) != tm || live_of(hs, sf.light, sf.cam, true) != tm) { std::printf("cornell: far camera / full: mask not full\n"); return 1; }
    const double nan_l[3] = {NAN, 0, 0};
    if (live_of(hs, nan_l, sf.cam) != tm) { std::printf("cornell: NaN light: mask not full\n"); return 1; }
    // lights at f delta from the ceiling, over the room's middle: live below delta, dead from it
    std::vector<V3> lights = {v3(sf.light[0], sf.light[1], sf.light[2]), v3(5, 0, 7), v3(-3, 1, 0)};
    const double fs[] = {0.5, 0.999, 1.001, 2.0};
    for (double f : fs) {
        double L[3] = {5, 0, 4};
        for (int it = 0; it < 3; ++it) L[2] = 5.0 - f * sl.delta(L);
        const bool dead = !(live_of(hs, L, sf.cam) & ceiling), want = (5.0 - L[2]) >= sl.delta(L);
        std::printf("cornell: light %.4g delta (%.6g) below the ceiling: ceiling %s\n", f, 5.0 - L[2], dead ? "dead" : "live");
        if (dead != want || dead != (f > 1.0)) { std::printf("cornell: wrong\n"); return 1; }
        lights.push_back(v3(L[0], L[1], L[2]));
    }
    // just above delta from one wall, from two (an edge) and from three (a corner)
    for (int c = 0; c < 12; ++c) {
        double L[3] = {1 + 8 * urand(), -4 + 8 * urand(), -4 + 8 * urand()};
        for (int it = 0; it < 3; ++it) {
            const double dl = 1.001 * sl.delta(L);
            const int m = c < 5 ? 1 << c : c < 9 ? 3 << (c - 5) : 7 << (c - 9);   // bits: x = 10, y = 5, y = -5, z = -5, z = 5
            if (m & 1) L[0] = 10 - dl;
            if (m & 2) L[1] = 5 - dl;
            else if (m & 4) L[1] = -5 + dl;
            if (m & 8) L[2] = -5 + dl;
            else if (m & 16) L[2] = 5 - dl;
        }
        if (live_of(hs, L, sf.cam) != (tm & ~walls)) { std::printf("cornell: light just above delta: a wall is live\n"); return 1; }
        lights.push_back(v3(L[0], L[1], L[2]));
    }
    std::printf("cornell: %d leaves, boundary %08x, delta(own light) %.4g, %zu lights\n", n, walls, sl.delta(sf.light), lights.size());
    for (const V3& L : lights) {
        const double Ld[3] = {L.x, L.y, L.z};
        const uint32_t live = live_of(hs, Ld, sf.cam);
        RayStats st;
        for (int r = 0; r < nrays; ++r) {
            const double lo[3] = {0, -5, -5}, hi[3] = {10, 5, 5};
            const V3 o = (r % 3 == 0) ? v3(sf.cam[0], sf.cam[1], sf.cam[2]) : rand_in(lo, hi);
            shadow_check(hs, live, o, cornell_target(r), L, st);
        }
        total.rays += st.rays; total.edge += st.edge; total.bad += st.bad; total.dead_tests += st.dead_tests;
        if (st.bad) std::printf("cornell: light (%.6g %.6g %.6g): %ld mismatches\n", L.x, L.y, L.z, st.bad);
    }
    return 0;
}

// any scene: marked leaves obey the rule; rays from random and camera origins toward random targets and
// toward points just off the marked planes, lights on either side of them
// file_cam: the camera of a .scn file given by itself (`scenes` mode) -- origins, targets and lights are then drawn
// around the scene's own bounds, not around the world origin, so a scene moved away from it is sampled alike
static int check_generic(const char* name, HostScene& hs, const double* light, int nrays, RayStats& total, const double* file_cam = nullptr) {
    const int n = (int)hs.xflat.size();
    if (hs.xflat_plane.size() != hs.xflat.size()) { std::printf("%s: xflat_plane has another length\n", name); return 1; }
    const XShadowLeaves sl = shadow_leaves_of(hs);
    int marked = 0;
    for (int k = 0; k < n; ++k)
        if (hs.xflat_plane[(size_t)k].sides) {
            ++marked;
            if (hs.xflat[(size_t)k].group == 255 || !sides_hold(hs, k)) { std::printf("%s: leaf %d marked against the rule\n", name, k); return 1; }
        }
    if (!hs.x_flat_ok) {
        if (sl.n != 0 || marked) { std::printf("%s: marks without the flat query\n", name); return 1; }
        std::printf("%s: %d leaves, not eligible, no marks\n", name, n);
        return 0;
    }
    const double E = std::max(1.0, hs.x_ext);
    double cam[3] = {-10, 0, 0}, c[3] = {0, 0, 0}, h[3] = {E, E, E};   // the region: centre and half size
    if (file_cam) {
        for (int k = 0; k < 3; ++k) {
            double lo = INFINITY, hi = -INFINITY;
            for (const XFlatLeaf& f : hs.xflat) { lo = std::min(lo, (double)f.lo[k]); hi = std::max(hi, (double)f.hi[k]); }
            cam[k] = file_cam[k];
            c[k] = 0.5 * (lo + hi);
            h[k] = 0.5 * (hi - lo);
        }
    }
    std::vector<V3> lights = {v3(light[0], light[1], light[2])};
    for (int i = 0; i < 6; ++i)
        lights.push_back(v3((2 * urand() - 1) * 1.5 * h[0] + c[0], (2 * urand() - 1) * 1.5 * h[1] + c[1], (2 * urand() - 1) * 1.5 * h[2] + c[2]));
    long dead_sum = 0;
    RayStats st;
    for (const V3& L : lights) {
        const double Ld[3] = {L.x, L.y, L.z};
        const uint32_t live = live_of(hs, Ld, cam);
        dead_sum += n - popc(live);
        for (int r = 0; r < nrays; ++r) {
            const V3 o = (r % 3 == 0) ? v3(cam[0], cam[1], cam[2])
                                      : v3((2 * urand() - 1) * h[0] + c[0], (2 * urand() - 1) * h[1] + c[1], (2 * urand() - 1) * h[2] + c[2]);
            V3 tgt = v3((2 * urand() - 1) * h[0] + c[0], (2 * urand() - 1) * h[1] + c[1], (2 * urand() - 1) * h[2] + c[2]);
            if (r % 2 == 0 && !hs.xprims.empty()) {   // a point of a primitive, moved by 1e-12 .. 1e-3
                const XPrim& p = hs.xprims[(size_t)(urand() * hs.xprims.size()) % hs.xprims.size()];
                double a = urand(), b = urand();
                if (a + b > 1) { a = 1 - a; b = 1 - b; }
                if (r % 4 == 0) a = tiny(), b = tiny();
                tgt = p.kind == 0 ? ld3(p.a) + ld3(p.b) * a + ld3(p.c) * b : ld3(p.a) + normalize(v3(urand() - 0.5, urand() - 0.5, urand() - 0.5)) * p.b[0];
                tgt = tgt + v3(urand() - 0.5, urand() - 0.5, urand() - 0.5) * tiny();
            }
            shadow_check(hs, live, o, tgt, L, st);
        }
    }
    total.rays += st.rays; total.edge += st.edge; total.bad += st.bad; total.dead_tests += st.dead_tests;
    std::printf("%s: %zu prims, %d leaves, %d boundary leaves, %ld dead over %zu lights, %ld rays, mismatches %ld\n", name, hs.xprims.size(), n, marked,
                dead_sum, lights.size(), st.rays, st.bad);
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 4) { std::printf("usage: xshadow_leaves_check <rays per light> <cornell.scn> <zoo.scn> | <rays per light> scenes a.scn ...\n"); return 2; }
    const int nrays = std::atoi(argv[1]);
    RayStats total;
    if (std::string(argv[2]) == "scenes") {   // the generic check alone, per file, from the file's camera under the file's light
        for (int i = 3; i < argc; ++i) {
            SceneFile sf;
            HostScene hs;
            if (!read_scn(argv[i], sf) || !build(sf.ents, hs)) return 2;
            if (check_generic(argv[i], hs, sf.light, nrays, total, sf.cam)) return 1;
        }
        std::printf("rays %ld mismatches %ld\n", total.rays, total.bad);
        return total.bad == 0 ? 0 : 1;
    }
    {
        SceneFile sf;
        HostScene hs;
        if (!read_scn(argv[2], sf) || !build(sf.ents, hs)) return 2;
        if (check_cornell(sf, hs, nrays, total)) return 1;
        if (check_generic("cornell", hs, sf.light, nrays / 8, total)) return 1;
    }
    {
        SceneFile sf;
        HostScene hs;
        if (!read_scn(argv[3], sf) || !build(sf.ents, hs)) return 2;
        if (check_generic("every entity", hs, sf.light, nrays / 4, total)) return 1;
    }
    {   // a ground quad under two spheres and a tilted triangle; the same with a triangle dipping below the ground
        for (int dip = 0; dip < 2; ++dip) {
            std::vector<gi_entity_desc> ents;
            ents.push_back(tri(v3(-4, -4, -1), v3(4, -4, -1), v3(4, 4, -1)));
            ents.push_back(tri(v3(-4, -4, -1), v3(4, 4, -1), v3(-4, 4, -1)));
            for (int i = 0; i < 2; ++i) {
                gi_entity_desc e{};
                e.kind = GI_IMP_SPHERE;
                e.args[0] = 2.0 * i - 1; e.args[1] = 1.0 - i; e.args[2] = i ? 0.5 : 0.0; e.args[3] = i ? 1.5 : 1.0;   // the first touches the ground
                ents.push_back(e);
            }
            ents.push_back(tri(v3(2, 2, dip ? -1.0 - 1e-9 : -1.0), v3(3, 2, 1), v3(2, 3, 2)));
            HostScene hs;
            if (!build(ents, hs)) return 2;
            int marked = 0;
            for (const XLeafPlane& r : hs.xflat_plane) marked += r.sides != 0;
            if ((marked != 0) == (dip != 0)) { std::printf("ground scene %d: %d boundary leaves\n", dip, marked); return 1; }
            const double light[3] = {0.5, -0.5, 3};
            if (check_generic(dip ? "ground, dipping triangle" : "ground", hs, light, nrays / 4, total)) return 1;
        }
    }
    std::printf("dead-leaf record tests %ld; rays from within 1e-6 of two planes: %.1f %%\n", total.dead_tests,
                100.0 * (double)total.edge / (double)std::max(1l, total.rays));
    std::printf("rays %ld mismatches %ld\n", total.rays, total.bad);
    return total.bad == 0 ? 0 : 1;
}
