// xflat_check.cpp — CPU check of the flat leaf table and the flat leaf query (gi_wf.hip wf_flat) over
// libgi's own host scene builder (gi_build.cpp + gi_bvh.cpp, compiled here by g++).
//
//  * table: every leaf child of every wide node appears exactly once, in node order then child
//    order, its box floats bit-equal to the node's, with the node's offset, count and plane group;
//    HostScene::x_flat_ok holds exactly for tables of at most GI_XFLAT_MAX leaves (of <= 255 records,
//    offsets below 2^16);
//  * query: wf_flat restated step for step -- phase A over the whole table (child_hit's arithmetic,
//    the own-plane group left out, nearest candidate and second smallest entry distance kept), phase
//    B per ray (nearest candidate first, the cut at the second entry distance, the others re-tested
//    against the best t; any hit: from the highest candidate down) -- returns brute force's closest
//    hit (t, primitive) and any-hit answer.
//  Scenes: the Cornell box (argv[2], a .scn file), soups of exactly 1, GI_XFLAT_MAX and
//  GI_XFLAT_MAX + 1 leaves, tilted coplanar quads, scenes with spheres.  Rays: random, axis-parallel,
//  and rays leaving computed hit points with the own-plane skip at incidences down to just above the
//  scene's bound (xaccel_check.cpp check_plane_skip's classes).
//   xflat_check <n_rays> [scene.scn [only]]   (rays of the file's scene from its own bounds, x_region.h;
//                                              only: the file's scene alone)
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
#include "x_region.h"   // where the rays start and aim: the scene's own bounds

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
static float up32(double v) {
    float f = (float)v;
    if ((double)f < v) f = std::nextafter(f, INFINITY);
    return f;
}
struct F3 { float x, y, z; };
static float inv_clamp(float v) { return std::fmin(std::fmax(1.0f / v, -1e30f), 1e30f); }

// the kernel's box test of a table record: plane distances fma(b, iv, -(o * iv)), near / far planes by
// the reciprocal's sign; tn is the entry distance
static bool flat_box(const XFlatLeaf& r, F3 no, F3 ivf, float tmax, float& tn) {
    const bool sx = std::signbit(ivf.x), sy = std::signbit(ivf.y), sz = std::signbit(ivf.z);
    const float ax = std::fmaf(r.lo[0], ivf.x, no.x), bx = std::fmaf(r.hi[0], ivf.x, no.x);
    const float ay = std::fmaf(r.lo[1], ivf.y, no.y), by = std::fmaf(r.hi[1], ivf.y, no.y);
    const float az = std::fmaf(r.lo[2], ivf.z, no.z), bz = std::fmaf(r.hi[2], ivf.z, no.z);
    tn = std::fmax(std::fmax(sx ? bx : ax, sy ? by : ay), std::fmax(sz ? bz : az, 0.0f));
    const float tf = std::fmin(std::fmin(sx ? ax : bx, sy ? ay : by), std::fmin(sz ? az : bz, tmax));
    return tn <= tf;
}
static float med3(float a, float b, float c) { return std::fmax(std::fmin(a, b), std::fmin(std::fmax(a, b), c)); }

static long g_iters = 0, g_cands = 0, g_queries = 0;
// wf_flat; skip: the ray's own plane group (254: none)
static int flat_query(const HostScene& s, V3 o, V3 d, bool any, double tmax, double& t_out, int skip) {
    const F3 of = {(float)o.x, (float)o.y, (float)o.z};
    const F3 ivf = {inv_clamp((float)d.x), inv_clamp((float)d.y), inv_clamp((float)d.z)};
    const F3 no = {-(of.x * ivf.x), -(of.y * ivf.y), -(of.z * ivf.z)};
    double tb = tmax;
    float tbf = up32(tmax);
    int best = -1;
    const int n = (int)s.xflat.size();
    uint32_t m = 0;
    int k1 = -1;
    float tn1 = INFINITY, tn2 = INFINITY;
    for (int k = 0; k < n; ++k) {   // phase A
        float tn;
        const bool hit = flat_box(s.xflat[k], no, ivf, tbf, tn) && (int)s.xflat[k].group != skip;
        if (hit) m |= 1u << k;
        if (any) {
            if (hit) k1 = k;
        } else {
            const float th = hit ? tn : INFINITY;
            if (th < tn1) k1 = k;
            tn2 = med3(tn1, tn2, th);
            tn1 = std::fmin(tn1, th);
        }
    }
    ++g_queries;
    g_cands += __builtin_popcount(m);
    bool go = m != 0;
    int k = k1;
    if (go) m &= ~(1u << k);
    while (go) {   // phase B
        ++g_iters;
        const XFlatLeaf& lf = s.xflat[k];
        for (int j = 0; j < lf.cnt; ++j) {
            const XHot& h = s.xhot[lf.off + j];
            const double t = prim_t(h, o, d, 1e-7);
            if (any) {
                if (t < tmax) { best = h.prim; break; }
            } else if (t < tb || (t == tb && h.prim < best)) {
                tb = t;
                best = h.prim;
                tbf = up32(tb);
            }
        }
        go = false;
        if (any) {
            if (best < 0 && m != 0) {
                k = 31 - __builtin_clz(m);
                m &= ~(1u << k);
                go = true;
            }
        } else {
            if (tn2 > tbf) m = 0;
            while (m != 0) {
                k = __builtin_ctz(m);
                m &= m - 1;
                float tn;
                if (flat_box(s.xflat[k], no, ivf, tbf, tn)) { go = true; break; }
            }
        }
    }
    t_out = any ? INFINITY : tb;
    return best;
}

static int brute(const HostScene& s, V3 o, V3 d, bool shadow, double tmax, double& tbest) {
    tbest = INFINITY;
    int best = -1;
    for (size_t i = 0; i < s.xprims.size(); ++i) {
        const double t = prim_t(hot_of(s.xprims[i], (int)i), o, d, 1e-7);
        if (shadow) {
            if (t < tmax) return (int)i;
        } else if (t < tbest) {
            tbest = t;
            best = (int)i;
        }
    }
    return best;
}

// the table against the wide nodes
static int check_table(const HostScene& s) {
    size_t k = 0;
    bool fits = true;
    for (const XWNode& w : s.xwnodes) {
        const uint8_t* g = reinterpret_cast<const uint8_t*>(w.pad);
        for (int c = 0; c < 8; ++c) {
            if (w.child[c] >= 0 || w.child[c] == XEMPTY) continue;
            if (k >= s.xflat.size()) { std::printf("table: leaf missing\n"); return 1; }
            const XFlatLeaf& f = s.xflat[k++];
            for (int a = 0; a < 3; ++a)
                if (std::memcmp(&f.lo[a], &w.lo[a][c], 4) != 0 || std::memcmp(&f.hi[a], &w.hi[a][c], 4) != 0) {
                    std::printf("table: box floats differ\n");
                    return 1;
                }
            if (f.off != ~w.child[c] || f.cnt != w.cnt[c] || f.group != g[c]) { std::printf("table: fields differ\n"); return 1; }
            fits = fits && f.cnt <= 255 && f.off < 65536;
        }
    }
    if (k != s.xflat.size()) { std::printf("table: %zu records for %zu leaves\n", s.xflat.size(), k); return 1; }
    // (each leaf once: the records' xhot ranges are disjoint and cover xhot)
    std::vector<int> seen(s.xhot.size(), 0);
    for (const XFlatLeaf& f : s.xflat)
        for (int j = 0; j < f.cnt; ++j) {
            if ((size_t)(f.off + j) >= seen.size() || seen[f.off + j]++) { std::printf("table: record ranges overlap\n"); return 1; }
        }
    for (int v : seen)
        if (!v) { std::printf("table: leaf record not covered\n"); return 1; }
    if (s.x_flat_ok != (fits && s.xflat.size() <= (size_t)GI_XFLAT_MAX)) { std::printf("table: x_flat_ok wrong\n"); return 1; }
    return 0;
}

static gi_entity_desc tri(const double* v) {
    gi_entity_desc e{};
    e.kind = GI_IMP_TRIANGLE;
    for (int k = 0; k < 9; ++k) e.args[k] = v[k];
    return e;
}
static gi_entity_desc sphere() {
    gi_entity_desc e{};
    e.kind = GI_IMP_SPHERE;
    e.args[0] = urand() * 10; e.args[1] = urand() * 10 - 5; e.args[2] = urand() * 10 - 5; e.args[3] = 0.3 + urand();
    return e;
}
static void add_soup(std::vector<gi_entity_desc>& ents, int ntri, double sz) {
    for (int i = 0; i < ntri; ++i) {
        double c[3] = {urand() * 10, urand() * 10 - 5, urand() * 10 - 5}, v[9];
        for (int k = 0; k < 9; ++k) v[k] = c[k % 3] + sz * (2 * urand() - 1);
        ents.push_back(tri(v));
    }
}
static void add_quads(std::vector<gi_entity_desc>& ents, int nq) {   // tilted quads: two triangles in one plane each
    for (int i = 0; i < nq; ++i) {
        const V3 c = v3(urand() * 10, urand() * 10 - 5, urand() * 10 - 5);
        const V3 u = normalize(v3(urand() - 0.5, urand() - 0.5, urand() - 0.5));
        const V3 w = normalize(cross(u, v3(urand() - 0.5, urand() - 0.5, urand() - 0.5)));
        const double su = 0.3 + urand(), sw = 0.3 + urand();
        const V3 q[4] = {c - u * su - w * sw, c + u * su - w * sw, c + u * su + w * sw, c - u * su + w * sw};
        const double v1[9] = {q[0].x, q[0].y, q[0].z, q[1].x, q[1].y, q[1].z, q[2].x, q[2].y, q[2].z};
        const double v2[9] = {q[0].x, q[0].y, q[0].z, q[2].x, q[2].y, q[2].z, q[3].x, q[3].y, q[3].z};
        ents.push_back(tri(v1));
        ents.push_back(tri(v2));
    }
}
static bool read_scn(const char* path, std::vector<gi_entity_desc>& ents) {
    std::ifstream f(path);
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream is(line);
        std::string kw;
        is >> kw;
        std::vector<double> v;
        double x;
        while (is >> x) v.push_back(x);
        gi_entity_desc e{};
        if (kw == "imptriangle") e.kind = GI_IMP_TRIANGLE;
        else if (kw == "impsphere") e.kind = GI_IMP_SPHERE;
        else continue;
        for (size_t k = 0; k < v.size() && k < 11; ++k) e.args[k] = v[k];
        ents.push_back(e);
    }
    return !ents.empty();
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
// a soup whose table has exactly `leaves` records (triangle counts tried upward, fresh soups)
static bool soup_with_leaves(int leaves, std::vector<gi_entity_desc>& ents, HostScene& hs) {
    for (int attempt = 0; attempt < 4000; ++attempt) {
        ents.clear();
        add_soup(ents, leaves == 1 ? 1 : leaves + attempt % (3 * leaves + 1), 0.6);
        hs = HostScene();
        if (!build(ents, hs)) return false;
        if ((int)hs.xflat.size() == leaves) return true;
    }
    std::printf("no soup of %d leaves found\n", leaves);
    return false;
}

static bool same(bool shadow, int a, int b, double t1, double t2) {
    return shadow ? ((a >= 0) == (b >= 0)) : (a == b && (t1 == t2 || (std::isinf(t1) && std::isinf(t2))));
}
// random and axis-parallel rays
static long check_rays(const HostScene& hs, const Region& rg, int nrays, long& total) {
    long bad = 0;
    for (int r = 0; r < nrays; ++r) {
        V3 o = (r % 2 == 0) ? rg.cam : rg.point(urand);
        V3 tgt = rg.point(urand);
        if (r % 7 == 0) tgt.y = o.y;                    // one axis-parallel component
        if (r % 21 == 0) tgt.z = o.z;                   // two
        if (r % 63 == 0) { o = rg.cam_yz(tgt); }         // along +x
        if (sq3(tgt - o) == 0.0) continue;
        const V3 d = normalize(tgt - o);
        const bool shadow = (r % 3) == 0;
        const double tmax = shadow ? rg.shadow_tmax(urand) : INFINITY;
        double t1, t2;
        const int a = flat_query(hs, o, d, shadow, tmax, t1, 254);
        const int b = brute(hs, o, d, shadow, tmax, t2);
        ++total;
        if (!same(shadow, a, b, t1, t2) && ++bad < 5) std::printf("ray mismatch: got %d want %d (t %.17g %.17g)\n", a, b, t1, t2);
    }
    return bad;
}
// rays leaving computed hit points, the origin's plane group skipped when the incidence clears the bound
static long check_plane_skip(const HostScene& hs, const Region& rg, int nrays, long& skipped, long& total) {
    long bad = 0;
    const int np = (int)hs.xprims.size();
    if (np == 0) return 0;
    for (int r = 0; r < nrays; ++r) {
        const int i = (int)(urand() * np) % np;
        const XPrim& x = hs.xprims[i];
        if (x.kind != 0 || x.pad[0] == 255) continue;
        const V3 o = (r % 4 == 0) ? rg.cam : rg.point(urand);
        double a = urand(), b = urand();
        if (a + b > 1) { a = 1 - a; b = 1 - b; }
        const V3 tgt = ld3(x.a) + ld3(x.b) * a + ld3(x.c) * b;
        const V3 d = normalize(tgt - o);
        const double t = prim_t(hot_of(x, i), o, d, 1e-7);
        if (!std::isfinite(t)) continue;
        const V3 P = o + t * d;   // as x_segment computes the hit point
        const V3 n = ld3(x.n);
        const double cmin = hs.x_skip_a * std::max(std::fabs(o.x), std::max(std::fabs(o.y), std::fabs(o.z))) + hs.x_skip_b;
        V3 d2;
        double tmax = INFINITY;
        const int kind = r % 5;
        if (kind == 0) {   // shadow ray toward a random point
            const V3 L = rg.point(urand);
            tmax = std::sqrt(sq3(L - P));
            d2 = normalize(L - P);
        } else {           // incidence c: random tangent direction tilted to |d . n| = c, either side
            const double c = kind == 1 ? urand() : kind == 2 ? cmin * (1.0 + 3.0 * urand()) : kind == 3 ? cmin * (1.0 + 1e-3 * urand()) : cmin * 0.5;
            V3 tg = cross(n, v3(urand() - 0.5, urand() - 0.5, urand() - 0.5));
            if (sq3(tg) == 0.0) continue;
            tg = normalize(tg);
            const double sg = urand() < 0.5 ? -1.0 : 1.0;
            d2 = normalize(tg * std::sqrt(std::max(0.0, 1.0 - c * c)) + n * (sg * c));
        }
        const bool shadow = kind == 0;
        const int skip = std::fabs(dot(d2, n)) >= cmin ? x.pad[0] : 254;
        double t1, t2;
        const int p1 = flat_query(hs, P, d2, shadow, tmax, t1, skip);
        const int p2 = brute(hs, P, d2, shadow, tmax, t2);
        ++total;
        skipped += skip != 254;
        if (!same(shadow, p1, p2, t1, t2) && ++bad < 5)
            std::printf("plane skip mismatch: prim %d kind %d skip %d got %d want %d (t %.17g %.17g)\n", i, kind, skip, p1, p2, t1, t2);
    }
    return bad;
}

int main(int argc, char** argv) {
    const int nrays = argc > 1 ? std::atoi(argv[1]) : 20000;
    long mism = 0, total = 0;
    // scenes: 0 one leaf, 1 GI_XFLAT_MAX leaves, 2 one more (table only: the scene keeps the tree),
    // 3 tilted coplanar quads, 4 quads and spheres, 5 soup and spheres, 6 the .scn file
    const bool only = argc > 3 && std::string(argv[3]) == "only";   // the .scn file alone
    for (int scene = only ? 6 : 0; scene < (argc > 2 ? 7 : 6); ++scene) {
        std::vector<gi_entity_desc> ents;
        HostScene hs;
        Region rg;
        if (scene <= 2) {
            if (!soup_with_leaves(scene == 0 ? 1 : GI_XFLAT_MAX + scene - 1, ents, hs)) return 2;
        } else {
            if (scene == 3) add_quads(ents, 14);
            if (scene == 4) { add_quads(ents, 8); for (int i = 0; i < 5; ++i) ents.push_back(sphere()); }
            if (scene == 5) { add_soup(ents, 18, 0.6); for (int i = 0; i < 6; ++i) ents.push_back(sphere()); }
            if (scene == 6 && !read_scn(argv[2], ents)) return 2;
            if (scene == 6) rg = region_of(ents, rg);
            if (!build(ents, hs)) return 2;
        }
        if (check_table(hs)) return 1;
        const size_t leaves = hs.xflat.size();
        if (scene == 2) {
            if (hs.x_flat_ok) { std::printf("scene 2: %zu leaves flagged as fitting\n", leaves); return 1; }
            std::printf("scene 2: %zu leaves, table checked, not eligible\n", leaves);
            continue;
        }
        if (!hs.x_flat_ok) { std::printf("scene %d: %zu leaves, not eligible\n", scene, leaves); return 1; }
        const long q0 = g_queries, i0 = g_iters, c0 = g_cands;
        long t0 = 0, skipped = 0, tot = 0;
        const long b1 = check_rays(hs, rg, nrays, t0);
        const long b2 = check_plane_skip(hs, rg, 4 * nrays, skipped, tot);
        mism += b1 + b2;
        total += t0 + tot;
        std::printf("scene %d: %zu prims, %zu leaves; %ld rays + %ld from hit points (%ld skipping, bound %.3g + %.3g |cam|);"
                    " per query %.2f candidates, %.2f exact-test iterations; mismatches %ld\n",
                    scene, hs.xprims.size(), leaves, t0, tot, skipped, hs.x_skip_b, hs.x_skip_a,
                    (double)(g_cands - c0) / (double)std::max(1l, g_queries - q0),
                    (double)(g_iters - i0) / (double)std::max(1l, g_queries - q0), b1 + b2);
    }
    std::printf("rays %ld mismatches %ld\n", total, mism);
    return mism == 0 ? 0 : 1;
}
