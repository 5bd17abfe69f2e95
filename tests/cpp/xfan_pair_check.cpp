// xfan_pair_check.cpp — the fan-pair decision of the flat leaf query (csrc/gi_fan_pair.h: the functions
// the builder and the kernel call, compiled here by g++) against two plain exact tests per pair.
//
//  For a fan pair (r0, r1) and a ray: fan_pair_choice(r0, o, d) names the record to run (or both); the
//  chosen record's t comes from x_prim_t's branch-free form restated here, the other record counts as
//  infinity.  Checked: (t of r0, t of r1) equal the plain Moller-Trumbore restatement's on both records,
//  bit for bit, for every ray.
//  Pairs: the Cornell box's 17 leaves (argv[2], through libgi's own host builder, which must mark all 17),
//  rotated planar rectangles and convex quads, quads bent to just inside the builder's parallel tolerance,
//  near-slivers just inside its sliver bound; and pairs the builder must refuse, each asserted refused:
//  folded, records in reverse order, one triangle wound backwards, slivers, non-convex, bent beyond the
//  tolerance, another first vertex, a sphere record.
//  Rays per pair: seeded random rays; rays aimed at points of the diagonal and 0, +-1, +-2, +-32 ulp off
//  them in each coordinate and in all three; rays through the four corners, through points of the edges and
//  along the edges; directions whose |d . n| straddles the det margin (in-plane tangents lifted by 2^-j),
//  det = 0 included; origins on the quad's plane; NaN and infinite directions.
//  Reported: the undecided share, over all rays and over the random rays alone (at most 1 % there).
//   xfan_pair_check <n_random_rays_per_pair> cornell.scn
//   xfan_pair_check info a.scn ...      (prints each scene's leaves and fan-pair leaves)
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
#include "gi_fan_pair.h"
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
static double srand1() { return 2.0 * urand() - 1.0; }

// the plain restatement (early returns, ||): the reference
static double prim_t(const XHot& p, V3 o, V3 d, double tmin) {
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
// x_prim_t<true> as gi_dev.h has it (one block, | and &): what the kernel runs on the chosen record
static double prim_t_dev(const XHot& p, V3 o, V3 d, double tmin) {
    const V3 e1 = ld3(p.b), e2 = ld3(p.c), v0 = ld3(p.a);
    const V3 pv = fcross(d, e2);
    const double det = fdot(e1, pv);
    const V3 tv = o - v0;
    const double un = fdot(tv, pv);
    const V3 qv = fcross(tv, e1);
    const double vn = fdot(d, qv);
    const double uvn = un + vn;
    const bool pos = det > 0.0;
    const bool miss = (det == 0.0) | (pos & ((un < 0.0) | (un > det) | (vn < 0.0) | (uvn > det))) |
                      (!pos & ((un > 0.0) | (un < det) | (vn > 0.0) | (uvn < det)));
    const double t = fdot(e2, qv) / det;
    return (!miss & (t > tmin)) ? t : INFINITY;
}

struct Pair { XHot r0, r1; };
static Pair make_pair(V3 a, V3 b, V3 c, V3 d) {   // the quad (a, b, c, d) as triangles (a, b, c), (a, c, d)
    Pair p{};
    st3(p.r0.a, a); st3(p.r0.b, b - a); st3(p.r0.c, c - a);
    st3(p.r1.a, a); st3(p.r1.b, c - a); st3(p.r1.c, d - a);
    p.r0.prim = 0; p.r1.prim = 1;
    p.r0.kind = p.r1.kind = 0;
    return p;
}
static double ulps(double x, int n) {
    for (int i = 0; i < (n < 0 ? -n : n); ++i) x = std::nextafter(x, n < 0 ? -INFINITY : INFINITY);
    return x;
}
static bool same_bits(double a, double b) { return mx_f64_to_bits(a) == mx_f64_to_bits(b); }

struct Tally {
    long rays = 0, both = 0, t1 = 0, t2 = 0, bad = 0;
    long rnd = 0, rnd_both = 0;                 // the seeded random rays alone
    long un0 = 0, det0 = 0, hits = 0, nan = 0;  // classes that must occur
};
static Tally g;

static void check(const Pair& p, V3 o, V3 d, bool random_class = false) {
    const double tmin = 1e-7;
    const double wa = prim_t(p.r0, o, d, tmin), wq = prim_t(p.r1, o, d, tmin);
    const int ch = fan_pair_choice(p.r0, o, d);
    const double ga = ch == FAN_T2 ? INFINITY : prim_t_dev(p.r0, o, d, tmin);
    const double gq = ch == FAN_T1 ? INFINITY : prim_t_dev(p.r1, o, d, tmin);
    ++g.rays;
    (ch == FAN_BOTH ? g.both : ch == FAN_T1 ? g.t1 : g.t2) += 1;
    if (random_class) { ++g.rnd; g.rnd_both += ch == FAN_BOTH; }
    if (std::isfinite(wa) || std::isfinite(wq)) ++g.hits;
    // the decision's own inputs, for the classes: un = 0 and det = 0 must not be decided for T1
    const V3 pv = fcross(d, ld3(p.r0.c));
    const double det = fdot(ld3(p.r0.b), pv), un = fdot(o - ld3(p.r0.a), pv);
    if (un == 0.0) { ++g.un0; if (ch == FAN_T1) { std::printf("un = 0 decided for T1\n"); ++g.bad; } }
    if (det == 0.0) { ++g.det0; if (ch == FAN_T1) { std::printf("det = 0 decided for T1\n"); ++g.bad; } }
    // (a NaN may still send the lane to T2 alone: by T1's own predicate, which x_prim_t evaluates the same)
    if (det != det || un != un) { ++g.nan; if (ch == FAN_T1) { std::printf("NaN decided for T1\n"); ++g.bad; } }
    if (!same_bits(wa, ga) || !same_bits(wq, gq)) {
        ++g.bad;
        if (g.bad < 20)
            std::printf("mismatch (choice %d): t0 %.17g want %.17g, t1 %.17g want %.17g; o %.17g %.17g %.17g d %.17g %.17g %.17g\n", ch,
                        ga, wa, gq, wq, o.x, o.y, o.z, d.x, d.y, d.z);
    }
}

static V3 rand_unit() {
    for (;;) {
        const V3 v = v3(srand1(), srand1(), srand1());
        const double q = sq3(v);
        if (q > 1e-4 && q <= 1.0) return normalize(v);
    }
}
static V3 comp_set(V3 v, int k, double x) { if (k == 0) v.x = x; else if (k == 1) v.y = x; else v.z = x; return v; }
static double comp(V3 v, int k) { return k == 0 ? v.x : k == 1 ? v.y : v.z; }

// the ray classes on one accepted pair
static void check_pair(const Pair& p, int nrand) {
    const V3 a = ld3(p.r0.a), e1 = ld3(p.r0.b), D = ld3(p.r0.c), e2 = ld3(p.r1.c);
    const V3 q[4] = {a, a + e1, a + D, a + e2};
    const double ext = fan_n1(e1) + fan_n1(D) + fan_n1(e2);
    const V3 n = normalize(cross(e1, D));
    auto origin = [&]() { return a + D * 0.5 + v3(srand1(), srand1(), srand1()) * (2.0 * ext); };
    // 1. seeded random rays toward points of the quad's neighbourhood
    for (int r = 0; r < nrand; ++r) {
        const V3 o = origin();
        const V3 tgt = a + e1 * (1.4 * urand() - 0.2) + e2 * (1.4 * urand() - 0.2) + D * (0.4 * urand() - 0.2);
        const V3 d = tgt - o;
        check(p, o, (r & 1) ? normalize(d) : d, true);
    }
    // 2. the diagonal: points a + s D, exact and 0, +-1, +-2, +-32 ulp off in each coordinate and in all
    const int offs[7] = {0, 1, -1, 2, -2, 32, -32};
    const double ss[7] = {0.0, 0.25, 0.5, 0.75, 1.0, urand(), urand()};
    for (double s : ss)
        for (int rep = 0; rep < 3; ++rep) {
            const V3 pt = a + D * s, o = origin();
            for (int off : offs)
                for (int k = 0; k < 4; ++k) {
                    V3 t = pt;
                    if (k < 3) t = comp_set(t, k, ulps(comp(t, k), off));
                    else t = v3(ulps(t.x, off), ulps(t.y, off), ulps(t.z, off));
                    check(p, o, t - o);
                    check(p, o, normalize(t - o));
                    V3 o2 = k < 3 ? comp_set(o, k, ulps(comp(o, k), off)) : o;
                    check(p, o2, pt - o);
                }
            // a ray in the plane spanned by the origin and the diagonal, built from the record itself:
            // o = a + (something along n and D), d along D's plane -- un is a cancelling triple product
            check(p, a + n * (0.5 * ext), (a + D * s) - (a + n * (0.5 * ext)));
        }
    // 3. corners, points of the edges, rays along the edges
    for (int c = 0; c < 4; ++c) {
        const V3 o = origin(), p0 = q[c], p1 = q[(c + 1) & 3];
        check(p, o, p0 - o);
        check(p, o, normalize(p0 - o));
        for (double s : {0.125, 0.5, 0.875}) check(p, o, (p0 + (p1 - p0) * s) - o);
        check(p, p0 - (p1 - p0) * 0.5, p1 - p0);               // along the edge, from outside
        check(p, p0 + (p1 - p0) * 0.25, p0 - p1);              // along the edge, from inside
        check(p, p0 - (p1 - p0) * 0.5 + n * (1e-9 * ext), p1 - p0);
    }
    check(p, a - D * 0.5, D);   // along the diagonal
    check(p, a + D * 0.5, -D);
    // 4. |d . n| across the det margin: an in-plane tangent lifted by +-2^-j, aimed at points of the quad
    for (int j = 4; j <= 70; j += 2)
        for (int rep = 0; rep < 2; ++rep) {
            const V3 w = normalize(e1 * srand1() + e2 * srand1());
            const double eps = std::ldexp(rep ? -1.0 : 1.0, -j);
            const V3 d = w + n * eps;
            const V3 tgt = a + e1 * urand() * 0.5 + e2 * urand() * 0.5;
            check(p, tgt - d * ext, d);
            check(p, tgt - d * ext, d * 3.0);
        }
    for (int rep = 0; rep < 4; ++rep) {   // det = 0: directions in the plane (exactly, where the quad is axis-aligned)
        const V3 w = rep < 2 ? e1 : e2;
        check(p, a + e1 * 0.3 + e2 * 0.3 + n * (rep & 1 ? 0.0 : 0.1 * ext), w);
    }
    // 5. origins on the quad's plane
    for (int r = 0; r < 16; ++r) {
        const V3 o = a + e1 * (1.5 * urand() - 0.25) + e2 * (1.5 * urand() - 0.25);
        check(p, o, rand_unit());
        check(p, o, (r & 1) ? n : -n);
        check(p, o, normalize(e1 * srand1() + e2 * srand1()));
    }
    // 6. NaN and infinite directions and origins
    const double nanv = std::nan("");
    check(p, origin(), v3(nanv, 1.0, 0.0));
    check(p, origin(), v3(nanv, nanv, nanv));
    check(p, origin(), v3(INFINITY, 0.0, 1.0));
    check(p, v3(nanv, 0.0, 0.0), rand_unit());
    check(p, origin(), v3(0.0, 0.0, 0.0));
}

static bool read_scn(const char* path, std::vector<gi_entity_desc>& ents) {
    std::ifstream f(path);
    std::string line;
    while (std::getline(f, line)) {
        std::istringstream is(line);
        std::string kw;
        is >> kw;
        const int kind = kw == "imptriangle" ? GI_IMP_TRIANGLE : kw == "impsphere" ? GI_IMP_SPHERE : 0;
        if (!kind) continue;
        gi_entity_desc e{};
        e.kind = kind;
        double x;
        for (int k = 0; k < 11 && (is >> x); ++k) e.args[k] = x;
        ents.push_back(e);
    }
    return !ents.empty();
}
static bool build(const char* path, HostScene& hs) {
    std::vector<gi_entity_desc> ents;
    if (!read_scn(path, ents)) { std::printf("%s: no entities\n", path); return false; }
    gi_scene_desc sd{};
    for (int k = 0; k < 3; ++k) { sd.octree_min[k] = -20; sd.octree_max[k] = 20; }
    sd.n_entities = (int32_t)ents.size();
    sd.entities = ents.data();
    std::string err;
    if (!build_host_scene(sd, hs, err)) { std::printf("build failed: %s\n", err.c_str()); return false; }
    return true;
}

static long g_refuse_bad = 0;
static void must_refuse(const char* what, const Pair& p) {
    if (fan_pair_ok(p.r0, p.r1)) { std::printf("accepted a pair it must refuse: %s\n", what); ++g_refuse_bad; }
}
static Pair must_accept(const char* what, const Pair& p) {
    if (!fan_pair_ok(p.r0, p.r1)) { std::printf("refused a fan pair: %s\n", what); ++g_refuse_bad; }
    return p;
}
// a rotation from three random angles
static void frame(V3& u, V3& v, V3& w) {
    u = rand_unit();
    v = normalize(cross(u, rand_unit()));
    w = cross(u, v);
}

int main(int argc, char** argv) {
    if (argc >= 3 && std::string(argv[1]) == "info") {
        for (int i = 2; i < argc; ++i) {
            HostScene hs;
            if (!build(argv[i], hs)) return 2;
            std::printf("info %s: leaves %zu fan %d all %d flat_ok %d\n", argv[i], hs.xflat.size(), hs.n_fan_leaves, (int)hs.x_fan_all,
                        (int)hs.x_flat_ok);
        }
        return 0;
    }
    if (argc < 3) { std::printf("usage: xfan_pair_check <n_rays> cornell.scn | info a.scn ...\n"); return 2; }
    const int nrand = std::atoi(argv[1]);
    std::vector<Pair> pairs;
    {   // the Cornell box: 17 leaves, every one a fan pair by the builder's own marking
        HostScene hs;
        if (!build(argv[2], hs)) return 2;
        if (hs.xflat.size() != 17 || hs.n_fan_leaves != 17 || !hs.x_fan_all) {
            std::printf("cornell: %zu leaves, %d fan pairs\n", hs.xflat.size(), hs.n_fan_leaves);
            return 1;
        }
        for (const XFlatLeaf& f : hs.xflat) pairs.push_back(Pair{hs.xhot[(size_t)f.off], hs.xhot[(size_t)f.off + 1]});
    }
    const size_t n_cornell = pairs.size();
    for (int i = 0; i < 12; ++i) {   // rotated planar rectangles and convex quads, at several scales and offsets
        V3 u, v, w;
        frame(u, v, w);
        const double sc = std::ldexp(1.0, (i % 4) * 3 - 3);
        const V3 c = v3(srand1(), srand1(), srand1()) * (i < 6 ? 5.0 : 500.0);
        if (i & 1) pairs.push_back(must_accept("rotated rectangle", make_pair(c - u * sc - v * (2 * sc), c + u * sc - v * (2 * sc), c + u * sc + v * (2 * sc), c - u * sc + v * (2 * sc))));
        else pairs.push_back(must_accept("rotated convex quad", make_pair(c, c + u * (sc * (1 + urand())), c + u * (sc * (1.5 + urand())) + v * (sc * (1.5 + urand())), c + v * (sc * (1 + urand())))));
    }
    const double T = kFanParTol;
    for (int i = 0; i < 4; ++i) {   // the unit square with d lifted by h: |n1 x n2| / (|n1|1 |n2|1) = h / (1 + 2 h)
        const double s = std::ldexp(1.0, 2 * i - 2), h = (i & 1 ? 0.9 : 0.5) * T;
        const V3 o = v3(3.0 * i, -1.0, 0.5 * i);
        pairs.push_back(must_accept("bent to inside the tolerance", make_pair(o, o + v3(s, 0, 0), o + v3(s, s, 0), o + v3(0, s, (i & 2 ? h : -h) * s))));
        must_refuse("bent to twice the tolerance", make_pair(o, o + v3(s, 0, 0), o + v3(s, s, 0), o + v3(0, s, 2.5 * T * s)));
    }
    for (int i = 0; i < 3; ++i) {   // parallelograms of angle phi: |n|1 / (|e1|1 |D|1) ~ sin(phi) / 2
        V3 u, v, w;
        frame(u, v, w);
        if (i == 0) { u = v3(1, 0, 0); v = v3(0, 1, 0); }
        // (|n|1 >= 3 sn; |e1|1 |D|1 = 2 (3.5 + 1.5 sn) on the axes and at most 36.4 in any frame)
        const double sn = (i == 0 ? 2.6 : 13.0) * kFanSliver, cs = std::sqrt(1 - sn * sn);
        const V3 b = u * 2.0, d = (u * cs + v * sn) * 1.5, c0 = v3(1, 2, 3);
        pairs.push_back(must_accept("near-sliver inside the bound", make_pair(c0, c0 + b, c0 + b + d, c0 + d)));
        const double s2 = 0.5 * kFanSliver, c2 = std::sqrt(1 - s2 * s2);
        const V3 d2 = (u * c2 + v * s2) * 1.5;
        must_refuse("sliver", make_pair(c0, c0 + b, c0 + b + d2, c0 + d2));
    }
    {   // refused pairs
        const V3 a = v3(0, 0, 0), b = v3(2, 0, 0), c = v3(2, 2, 0), d = v3(0, 2, 0);
        const Pair ok = must_accept("square", make_pair(a, b, c, d));
        must_refuse("records in reverse order", Pair{ok.r1, ok.r0});
        must_refuse("folded (d on b's side of the diagonal)", make_pair(a, b, c, v3(1.5, 0.5, 0)));
        must_refuse("folded along the diagonal (d above b)", make_pair(a, b, c, v3(2, 0, 1e-3)));
        Pair wound = ok;   // (a, c, b), (a, c, d): the first triangle wound backwards
        st3(wound.r0.b, c - a); st3(wound.r0.c, b - a);
        must_refuse("first triangle wound backwards", wound);
        must_refuse("non-convex at c", make_pair(a, b, v3(0.5, 0.5, 0), d));
        must_refuse("non-convex at a", make_pair(v3(1.5, 1.5, 0), b, v3(2.5, 2.5, 0), d));
        must_refuse("collinear b, c, d", make_pair(a, v3(2, 0, 0), v3(1, 1, 0), v3(0, 2, 0)));
        must_refuse("zero-area triangle", make_pair(a, b, v3(4, 0, 0), d));
        must_refuse("not planar", make_pair(a, b, c, v3(0, 2, 1e-6)));
        Pair other = ok;
        other.r1.a[0] = ulps(other.r1.a[0], 1);
        must_refuse("another first vertex (1 ulp)", other);
        other = ok;
        other.r1.b[1] = ulps(other.r1.b[1], 1);
        must_refuse("another diagonal (1 ulp)", other);
        other = ok;
        other.r1.kind = 1;
        must_refuse("a sphere record", other);
        other = ok;
        other.r0.c[2] = std::nan("");
        other.r1.b[2] = other.r0.c[2];
        must_refuse("NaN", other);
    }
    if (g_refuse_bad) { std::printf("builder predicate: %ld wrong\n", g_refuse_bad); return 1; }
    for (size_t i = 0; i < pairs.size(); ++i) check_pair(pairs[i], nrand);
    const double share = (double)g.both / (double)g.rays, rshare = (double)g.rnd_both / (double)(g.rnd ? g.rnd : 1);
    std::printf("pairs %zu (cornell %zu); T1 %ld T2 %ld both %ld; hits %ld; un = 0: %ld, det = 0: %ld, NaN: %ld\n", pairs.size(), n_cornell,
                g.t1, g.t2, g.both, g.hits, g.un0, g.det0, g.nan);
    if (g.un0 == 0 || g.det0 == 0 || g.nan == 0 || g.hits == 0 || g.t1 == 0 || g.t2 == 0 || g.both == 0) {
        std::printf("a ray class is empty\n");
        return 1;
    }
    std::printf("rays %ld undecided %.6f random rays %ld undecided %.6f mismatches %ld\n", g.rays, share, g.rnd, rshare, g.bad);
    if (rshare > 0.01) { std::printf("more than 1%% of the random rays undecided\n"); return 1; }
    return g.bad == 0 ? 0 : 1;
}
