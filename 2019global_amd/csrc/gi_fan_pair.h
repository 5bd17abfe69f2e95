// gi_fan_pair.h — fan-pair leaves of the flat leaf query (gi_wf.hip wf_flat, TRI kernels): which of a
// leaf's two triangles a ray can hit, decided from the first step of the first triangle's exact test.
// Host and device: the builder (gi_build.cpp build_xflat) marks the leaves with fan_pair_ok, the kernel
// calls fan_pair_choice, and tests/cpp/xfan_pair_check.cpp drives the same two functions on the CPU.
//
// A fan pair is the two halves of one planar convex quad (a, b, c, d) cut along its diagonal a-c:
//   T1 = (v0 = a, e1 = b - a, e2 = D),  T2 = (v0 = a, e1 = D, e2 = d - a),  D = c - a,
// with v0 and D the same bits in both records.  x_prim_t (gi_dev.h) computes for T1
//   tv = o - v0,  pv1 = fcross(d, D),  det1 = fdot(e1, pv1),  un1 = fdot(tv, pv1)
// and for T2  vn2 = fdot(d, fcross(tv, D)): in exact arithmetic vn2 = -un1 (the same triple product,
// two of its vectors exchanged), and det2 = -d . n2 has the sign of det1 = -d . n1 because the normals
// n1 = e1 x D and n2 = D x e2' point the same way.  So when un1 has det1's sign and both are clear of
// rounding, vn2 has the wrong sign for det2 and x_prim_t(T2) returns infinity: T2 need not be run.
// When un1 has the wrong sign for det1, x_prim_t(T1) returns infinity by its own test (no margin: the
// values are T1's own), and only T2 is run.  The margins: DESIGN.md §5 "Fan-pair leaves".
#ifndef GI_FAN_PAIR_H_
#define GI_FAN_PAIR_H_

#include "gi_math.h"
#include "gi_scene.h"

namespace gi {

// The builder's bounds (fan_pair_ok).  With n1, n2 the two unnormalised normals and |.|1 the 1-norm:
//  parallel: every component of n1 x n2 is at most kFanParTol |n1|1 |n2|1 in magnitude, and n1 . n2 > 0;
//  no sliver: |n|1 >= kFanSliver |e1|1 |e2|1 for both triangles (|e1 x e2|1 <= |e1|1 |e2|1 always).
constexpr double kFanParTol = 0x1.0p-44;
constexpr double kFanSliver = 0x1.0p-6;
// The decision's margin, relative to the 1-norm product of a triple product's three vectors (rounding:
// 5 u of that product, u = 2^-53), and its absolute floor (underflow in the products).
constexpr double kFanMargin = 0x1.0p-24;
constexpr double kFanFloor = 0x1.0p-960;

enum FanChoice : int { FAN_T1 = 0, FAN_T2 = 1, FAN_BOTH = 2 };

GI_HD double fan_abs(double x) { return __builtin_fabs(x); }
GI_HD double fan_n1(V3 v) { return fan_abs(v.x) + fan_abs(v.y) + fan_abs(v.z); }
GI_HD bool fan_same_bits(const double* p, const double* q) {
    return mx_f64_to_bits(p[0]) == mx_f64_to_bits(q[0]) && mx_f64_to_bits(p[1]) == mx_f64_to_bits(q[1]) &&
           mx_f64_to_bits(p[2]) == mx_f64_to_bits(q[2]);
}

// The records r0, r1 of a two-record leaf are a fan pair.
GI_HD bool fan_pair_ok(const XHot& r0, const XHot& r1) {
    if (r0.kind != 0 || r1.kind != 0) return false;
    if (!fan_same_bits(r0.a, r1.a) || !fan_same_bits(r0.c, r1.b)) return false;
    const V3 e1 = ld3(r0.b), D = ld3(r0.c), e2 = ld3(r1.c);
    const V3 n1 = cross(e1, D), n2 = cross(D, e2);
    const double s1 = fan_n1(n1), s2 = fan_n1(n2);
    // (written so that a NaN or an infinity anywhere refuses the pair)
    if (!(s1 >= kFanSliver * (fan_n1(e1) * fan_n1(D))) || !(s2 >= kFanSliver * (fan_n1(D) * fan_n1(e2)))) return false;
    if (!(s1 > 0.0) || !(s2 > 0.0) || !(s1 * s2 < INFINITY)) return false;
    if (!(dot(n1, n2) > 0.0)) return false;   // folded along the diagonal
    const V3 x = cross(n1, n2);
    const double tol = kFanParTol * (s1 * s2);
    if (!(fan_abs(x.x) <= tol) || !(fan_abs(x.y) <= tol) || !(fan_abs(x.z) <= tol)) return false;
    // convex: the other diagonal's triangles (b, c, d) and (d, a, b) turn the same way
    const V3 nb = cross(D - e1, e2 - e1), nd = cross(e1, e2);
    return dot(nb, n1) > 0.0 && dot(nd, n1) > 0.0;
}

// Which record of a fan pair whose first record is r0 the ray (o, d) can hit: FAN_T1 / FAN_T2 (the other
// record's x_prim_t<true> is infinity), or FAN_BOTH (undecided: run both).  tv, pv, det and un are
// x_prim_t's own operations on r0.
GI_HD int fan_pair_choice(const XHot& r0, V3 o, V3 d) {
    const V3 e1 = ld3(r0.b), D = ld3(r0.c), v0 = ld3(r0.a);
    const V3 pv = fcross(d, D);
    const double det = fdot(e1, pv);
    const V3 tv = o - v0;
    const double un = fdot(tv, pv);
    const bool pos = det > 0.0;
    const bool t1_miss = (pos & (un < 0.0)) | (!pos & (un > 0.0));
    // (the direction's factor first: the same for every leaf of a query)
    const double k = (kFanMargin * fan_n1(d)) * fan_n1(D);
    const bool sure = (fan_abs(un) > gfma(k, fan_n1(tv), kFanFloor)) & (fan_abs(det) > gfma(k, fan_n1(e1), kFanFloor));
    return t1_miss ? FAN_T2 : (sure ? FAN_T1 : FAN_BOTH);
}

}  // namespace gi

#endif  // GI_FAN_PAIR_H_
