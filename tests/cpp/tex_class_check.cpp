// CPU check of the checker-texel filter (2019global_amd/csrc/gi_math.h tri_tex_class / tri_texel_fast:
// the functions the shading helper x_texel calls on the device, here with IEEE division, sqrt and floor).
// For every point: texel(colour, exact u, exact v) -- tri_texcoord, the exact code -- against the
// helper's logic: tri_texel_fast's colour where it answers, the exact code where it does not (equal by
// construction, so only an answer can be wrong).  A wrong answer is a failure.
//
// Frames: Cornell-box wall triangles (red wall both halves, green wall, back wall) and block faces (short
// block top, tall block side), a long thin triangle, a small triangle with a tiny unit (coordinates reach
// 1e5), a degenerate one (p3 - p1 = -(p2 - p1): zero median, unit_v = 0).  Every point runs with a
// non-white colour (the filter decides), every 16th also with white (the colour decides).
// Points per frame (argv[1] x 2.5 M; 4 gives 10 M):
//   40%  uniform in the triangle
//   10%  uniform in the triangle's plane, three triangle sizes around it
//   30%  pattern boundaries: a point whose exact u (half of them: v) is 32 k + {0, 17}, its distance from
//        p1 scaled by 1 -/+ j 2^-52, j = 0 .. 4 (the rounding of the point itself adds a few ulp of noise)
//   10%  the p1 -> p2 edge and its extension (t in [-2, 3]) with relative offsets 0, 1e-17 .. 1e-6 off it
//   10%  far outside: p1 + a random direction x 10^k, k = 1 .. 8 and 30, 300; P == p1 and its neighbours
// Prints one line per frame, the share of uniform points on the coloured walls that the filter leaves
// to the exact code, and "failures N" last; exit status 1 when N > 0.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

#include "gi_math.h"

namespace {
using namespace gi;

uint64_t mix(uint64_t x) {
    x ^= x >> 30; x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27; x *= 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}
struct Rng {
    uint64_t s;
    uint64_t next() { return mix(s += 0x9E3779B97F4A7C15ull); }
    double u01() { return (double)(next() >> 11) * 0x1.0p-53; }
};

struct Frame {
    const char* name;
    V3 p1, p2, p3;
    bool wall;       // counts toward the coloured walls' fallback share
    // the entity record's frame as gi_build.cpp computes it: qv0 = p1, qv1 = p2 - p1, qv2 = (|p21|, unit_v, unit_h)
    double qv0[3] = {}, qv1[3] = {}, qv2[3] = {};
    V3 p21 = {};
    double unit_v = 0, unit_h = 0;
    unsigned long long points = 0, answered = 0, wrong = 0, uni = 0, uni_left = 0;
};

void derive(Frame& f) {
    const V3 p21 = f.p2 - f.p1, p31 = f.p3 - f.p1, p32 = f.p3 - f.p2;
    f.p21 = p21;
    f.unit_v = gsqrt(sq3(0.5 * (p21 + p31))) / 160.0;
    f.unit_h = gsqrt(sq3(0.5 * ((-p32) + (-p31)))) / 160.0;
    st3(f.qv0, f.p1);
    st3(f.qv1, p21);
    f.qv2[0] = gsqrt(sq3(p21)); f.qv2[1] = f.unit_v; f.qv2[2] = f.unit_h;
}

bool same(V3 a, V3 b) { return std::memcmp(&a, &b, sizeof a) == 0; }

// one point, one colour: true when the filter (or the colour) answered
bool check(Frame& f, V3 color, V3 P) {
    int32_t x, y;
    tri_texcoord(f.qv0, f.qv1, f.qv2, P, x, y);
    const V3 want = texel(color, x, y);
    bool white;
    const bool fast = tri_texel_fast(color, f.p1, f.p21, f.unit_v, f.unit_h, P, white);
    ++f.points;
    if (fast) {
        const V3 tc = texel_pick(color, white);
        ++f.answered;
        if (!same(tc, want)) {
            if (f.wrong < 5)
                std::printf("  WRONG %s P (%a, %a, %a) exact (%d, %d) want %g %g %g got %g %g %g\n", f.name, P.x, P.y, P.z,
                            x, y, want.x, want.y, want.z, tc.x, tc.y, tc.z);
            ++f.wrong;
        }
    }
    return fast;
}

void run(Frame& f, unsigned long long n, uint64_t seed) {
    Rng r{seed};
    const V3 colours[2] = {v3(1.0, 0.25, 0.0), v3(0.0, 1.9, 0.0)};   // truncate to (1,0,0) and (0,1,0)
    const V3 white = v3(1.0, 1.5, 1.999);                              // truncates to (1,1,1)
    const V3 e1v = f.p2 - f.p1, e2v = f.p3 - f.p1;
    // an orthonormal basis of the plane (any plane through the edge for the degenerate frame)
    V3 a1 = normalize(e1v), nn = cross(e1v, e2v);
    if (!(dot(nn, nn) > 0.0)) nn = cross(e1v, std::fabs(a1.x) < 0.9 ? v3(1, 0, 0) : v3(0, 1, 0));
    nn = normalize(nn);
    const V3 a2 = cross(nn, a1);
    const double size = smax(gsqrt(sq3(e1v)), gsqrt(sq3(e2v)));
    unsigned long long k = 0;
    auto one = [&](V3 P, bool uniform) {
        const bool fast = check(f, colours[k & 1], P);
        if (uniform) { ++f.uni; f.uni_left += fast ? 0 : 1; }
        if ((k & 15) == 0) {
            if (!check(f, white, P)) { ++f.wrong; std::printf("  WRONG %s: a white entity asked for the exact code\n", f.name); }
        }
        ++k;
    };
    for (unsigned long long i = 0; i < n * 4 / 10; ++i) {   // uniform in the triangle
        double s = r.u01(), t = r.u01();
        if (s + t > 1.0) { s = 1.0 - s; t = 1.0 - t; }
        one(f.p1 + (s * e1v + t * e2v), true);
    }
    for (unsigned long long i = 0; i < n / 10; ++i)        // around it, in its plane
        one(f.p1 + ((6.0 * r.u01() - 3.0) * size) * a1 + ((6.0 * r.u01() - 3.0) * size) * a2, false);
    for (unsigned long long i = 0; i < n * 3 / 10; ++i) {   // pattern boundaries
        const bool for_v = (i & 1) != 0;
        const double unit = for_v ? f.unit_h : f.unit_v;
        const double reach = 3.0 * size / (unit > 0.0 ? unit : 1.0);   // coordinates the plane points above take
        const double cells = std::floor(r.u01() * smin(reach, 1.0e6) / 32.0);
        const double B = 32.0 * cells + ((r.next() & 1) ? 17.0 : 0.0);
        const double th = (0.001 + 0.998 * r.u01()) * 3.14159265358979;
        const double sn = std::sin(th);
        const int j = (int)(r.next() % 9) - 4;
        const double len = (for_v ? B * unit : B * unit / sn) * (1.0 + (double)j * 0x1.0p-52);
        one(f.p1 + (len * std::cos(th)) * a1 + (len * sn) * a2, false);
    }
    const double offs[8] = {0.0, 1e-17, 1e-16, 1e-15, 1e-13, 1e-11, 1e-8, 1e-6};
    for (unsigned long long i = 0; i < n / 10; ++i) {      // the p1 -> p2 edge and its extension
        const double t = 5.0 * r.u01() - 2.0;
        const double off = offs[r.next() & 7] * size * ((r.next() & 1) ? 1.0 : -1.0);
        one(f.p1 + t * e1v + off * ((r.next() & 1) ? a2 : nn), false);
    }
    const double far_k[10] = {1e1, 1e2, 1e3, 1e4, 1e5, 1e6, 1e7, 1e8, 1e30, 1e300};
    for (unsigned long long i = 0; i < n / 10; ++i) {      // far outside, any direction
        const V3 dir = v3(2.0 * r.u01() - 1.0, 2.0 * r.u01() - 1.0, 2.0 * r.u01() - 1.0);
        one(f.p1 + (far_k[r.next() % 10] * size) * dir, false);
    }
    one(f.p1, false);                                       // P == p1 and its neighbours
    for (int d = 0; d < 3; ++d)
        for (int sgn = -1; sgn <= 1; sgn += 2) {
            V3 P = f.p1;
            double* c = d == 0 ? &P.x : d == 1 ? &P.y : &P.z;
            *c = std::nextafter(*c, sgn * INFINITY);
            one(P, false);
        }
}

}  // namespace

int main(int argc, char** argv) {
    const unsigned long long scale = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 4;
    const unsigned long long n = scale * 2500000ull;
    std::vector<Frame> fr = {
        {"red wall a", v3(0, 5, -5), v3(10, 5, -5), v3(10, 5, 5), true},
        {"red wall b", v3(0, 5, -5), v3(10, 5, 5), v3(0, 5, 5), true},
        {"green wall a", v3(0, -5, -5), v3(10, -5, -5), v3(10, -5, 5), true},
        {"back wall a", v3(10, -5, -5), v3(10, 5, -5), v3(10, 5, 5), false},
        {"short block top b", v3(5.0, -3.5, -2.0), v3(7.5, -1.0, -2.0), v3(5.0, -1.0, -2.0), false},
        {"tall block side a", v3(6.5, 0.5, -5.0), v3(6.5, 3.0, -5.0), v3(6.5, 3.0, 0.5), false},
        {"long thin", v3(-3.0, 2.0, 1.0), v3(97.0, 2.5, 1.25), v3(47.0, 2.26, 1.13), false},
        {"tiny unit", v3(1.0, 2.0, 3.0), v3(1.001, 2.0, 3.0), v3(1.0, 2.001, 3.0005), false},
        {"degenerate", v3(0.5, 0.25, 0.0), v3(1.5, 0.5, 0.0), v3(-0.5, 0.0, 0.0), false},
    };
    for (Frame& f : fr) derive(f);
    std::vector<std::thread> th;
    for (size_t i = 0; i < fr.size(); ++i) th.emplace_back(run, std::ref(fr[i]), n, 0x1234ull + 977ull * i);
    for (std::thread& t : th) t.join();
    unsigned long long failures = 0, uni = 0, left = 0;
    for (const Frame& f : fr) {
        std::printf("frame %s: points %llu answered %llu wrong %llu\n", f.name, f.points, f.answered, f.wrong);
        failures += f.wrong;
        if (f.wall) { uni += f.uni; left += f.uni_left; }
    }
    std::printf("wall fallback share %.6f of %llu uniform points\n", uni ? (double)left / (double)uni : 1.0, uni);
    std::printf("failures %llu\n", failures);
    return failures ? 1 : 0;
}
