// xflat_pk_check.cpp — CPU checks of the flat leaf query's packed Phase A (gi_wf.hip flat_pk_inner /
// flat_pk_outer; DESIGN.md §5 "Two-stage slab distances").  Host code only, stand-alone.
//
//   xflat_pk_check identity <cases per class>
//     The two-stage form of a box's plane distances against child_hit's select form, both with fmaf and no
//     contraction, over generated rays and boxes.  Per axis, with a = fma(lo, iv, no), b = fma(hi, iv, no):
//       select:     near = iv < 0 ? b : a,                       far = iv < 0 ? a : b
//       two-stage:  near = fma(hi, ivn, fma(lo, ivp, no)),       far = fma(lo, ivn, fma(hi, ivp, no))
//     with ivp = iv < 0 ? +0 : iv and ivn = iv < 0 ? iv : +0 (the sign bit decides, gi_dev.h iv_signs).  iv and no
//     are made as the device makes them (inv_dir's clamp to +-1e30, neg_oiv).  Compared per case: near and far
//     of every axis, max(near, 0) of every axis, the entry distance tn and the decision tn <= min(far, tmax).
//     Values must be equal; +0 and -0 count as equal and their differences are counted.  Classes:
//       octants   all eight sign combinations of the direction, moderate coordinates
//       zero_dir  one or two direction components zero, +0 and -0: the clamped reciprocals of either sign
//       zero_org  one to three origin components +0 or -0
//       on_plane  one to three origin components exactly on a plane of the box
//       large     coordinates up to GI_X_COORD_MAX, every other ray with zero direction components: the products
//                 with the clamped reciprocal that overflow (gi_dev.h inv_dir's comment)
//       thin      boxes zero to four ulp thick on every axis, at magnitudes from 1e-3 to 1e8
//       tiny      coordinates and direction components down to fp32's subnormals
//     Prints one line per class and "cases <n> mismatches <m> zero_sign <z>" last; exit status 1 on a mismatch.
//
//   xflat_pk_check table scene.scn [...]
//     For each scene file (imptriangle / impsphere lines; the builder's knobs from the environment): the device's
//     leaf table (gi_build.cpp xflat_device_table) is HostScene::xflat word for word in the order lo.x, hi.x,
//     lo.y, hi.y, lo.z, hi.z, off, (cnt | group << 16 | fan << 24), and those words decode to the host's off, cnt,
//     group and fan.  Prints "<file>: leaves <n> mismatches <m>" per scene; exit status 1 on a mismatch.
#include <atomic>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <thread>
#include <vector>

#include "gi.h"
#include "gi_scene.h"

using namespace gi;

namespace {

struct Rng {   // splitmix64
    uint64_t s;
    uint64_t next() {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    double u01() { return (double)(next() >> 11) * (1.0 / 9007199254740992.0); }
    double sym() { return 2.0 * u01() - 1.0; }
    unsigned below(unsigned n) { return (unsigned)(next() % n); }
    // magnitude log-uniform in [lo, hi], random sign
    double logmag(double lo, double hi) { return (next() & 1 ? -1.0 : 1.0) * std::exp(std::log(lo) + u01() * (std::log(hi) - std::log(lo))); }
};

inline uint32_t bits(float x) {
    uint32_t u;
    std::memcpy(&u, &x, 4);
    return u;
}
inline float clamp_iv(float r) { return r < -1e30f ? -1e30f : r > 1e30f ? 1e30f : r; }   // (inv_dir: never NaN here)
// equal as values (+0 == -0; NaN only with NaN)
inline bool same(float a, float b) { return a == b || (a != a && b != b); }
inline bool zero_sign_differs(float a, float b) { return a == 0.0f && b == 0.0f && bits(a) != bits(b); }

struct Case {
    float o[3], d[3], lo[3], hi[3], tmax;
};

struct Tally {
    uint64_t cases = 0, mismatches = 0, zero_sign = 0;
    Case first{};
    bool have_first = false;
};

void check(const Case& c, Tally& t) {
    float nearS[3], farS[3], nearT[3], farT[3];
    for (int k = 0; k < 3; ++k) {
        const float iv = clamp_iv(1.0f / c.d[k]);
        const float no = -(c.o[k] * iv);
        const bool neg = (bits(iv) >> 31) != 0;
        const float a = fmaf(c.lo[k], iv, no), b = fmaf(c.hi[k], iv, no);
        nearS[k] = neg ? b : a;
        farS[k] = neg ? a : b;
        const float ivp = neg ? 0.0f : iv, ivn = neg ? iv : 0.0f;
        nearT[k] = fmaf(c.hi[k], ivn, fmaf(c.lo[k], ivp, no));
        farT[k] = fmaf(c.lo[k], ivn, fmaf(c.hi[k], ivp, no));
    }
    bool ok = true;
    for (int k = 0; k < 3; ++k) {
        ok = ok && same(nearS[k], nearT[k]) && same(farS[k], farT[k]) && same(fmaxf(nearS[k], 0.0f), fmaxf(nearT[k], 0.0f));
        t.zero_sign += zero_sign_differs(nearS[k], nearT[k]) + zero_sign_differs(farS[k], farT[k]);
    }
    const float tnS = fmaxf(fmaxf(nearS[0], nearS[1]), fmaxf(nearS[2], 0.0f));
    const float tfS = fminf(fminf(farS[0], farS[1]), fminf(farS[2], c.tmax));
    const float tnT = fmaxf(fmaxf(nearT[0], nearT[1]), fmaxf(nearT[2], 0.0f));
    const float tfT = fminf(fminf(farT[0], farT[1]), fminf(farT[2], c.tmax));
    ok = ok && same(tnS, tnT) && same(tfS, tfT) && ((tnS <= tfS) == (tnT <= tfT));
    ++t.cases;
    if (!ok) {
        ++t.mismatches;
        if (!t.have_first) { t.first = c; t.have_first = true; }
    }
}

void unit3(double* v) {
    const double n = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (n > 0.0 && std::isfinite(n)) for (int k = 0; k < 3; ++k) v[k] /= n;   // (a zero keeps its sign)
}
float next_up_by(float x, int ulps) {
    for (int i = 0; i < ulps; ++i) x = std::nextafterf(x, INFINITY);
    return x;
}
// a box around / beside a point, sides up to `size`, clamped to +-lim
void box_near(Rng& r, const double* p, double size, double lim, Case& c) {
    for (int k = 0; k < 3; ++k) {
        const double a = p[k] + size * r.sym(), b = a + size * r.u01();
        c.lo[k] = (float)std::fmax(-lim, std::fmin(lim, a));
        c.hi[k] = (float)std::fmax(-lim, std::fmin(lim, b));
        if (c.hi[k] < c.lo[k]) c.hi[k] = c.lo[k];
    }
}
float pick_tmax(Rng& r, double scale) {
    const unsigned m = r.below(4);
    return m == 0 ? INFINITY : m == 1 ? 0.0f : (float)(scale * 4.0 * r.u01() * r.u01());
}

enum Class { OCTANTS, ZERO_DIR, ZERO_ORG, ON_PLANE, LARGE, THIN, TINY, N_CLASSES };
const char* const kClassNames[N_CLASSES] = {"octants", "zero_dir", "zero_org", "on_plane", "large", "thin", "tiny"};

void zero_some_dirs(Rng& r, uint64_t i, double* d) {
    // one zero (three places x two signs), then two zeros (three places x four sign pairs): by the case index
    const unsigned v = (unsigned)(i % 18);
    const double z[2] = {0.0, -0.0};
    if (v < 6) d[v % 3] = z[v / 3];
    else {
        const unsigned w = v - 6, keep = w % 3, s = w / 3;
        d[(keep + 1) % 3] = z[s & 1];
        d[(keep + 2) % 3] = z[s >> 1];
    }
    (void)r;
}

Case make(Class cl, Rng& r, uint64_t i) {
    Case c{};
    double o[3], d[3];
    for (int k = 0; k < 3; ++k) { o[k] = 10.0 * r.sym(); d[k] = 0.02 + r.u01(); }
    const unsigned oct = (unsigned)(i & 7);
    for (int k = 0; k < 3; ++k) if (oct >> k & 1) d[k] = -d[k];
    double scale = 10.0;
    switch (cl) {
        case OCTANTS:
            unit3(d);
            box_near(r, o, 6.0, GI_X_COORD_MAX, c);
            break;
        case ZERO_DIR:
            zero_some_dirs(r, i >> 3, d);
            unit3(d);
            box_near(r, o, 6.0, GI_X_COORD_MAX, c);
            break;
        case ZERO_ORG: {
            unit3(d);
            const unsigned m = 1 + r.below(7);   // which components, not none
            for (int k = 0; k < 3; ++k) if (m >> k & 1) o[k] = (r.next() & 1) ? 0.0 : -0.0;
            if (i & 8) zero_some_dirs(r, i >> 4, d);
            box_near(r, o, 6.0, GI_X_COORD_MAX, c);
            break;
        }
        case ON_PLANE: {
            unit3(d);
            if (i & 8) zero_some_dirs(r, i >> 4, d);
            box_near(r, o, 6.0, GI_X_COORD_MAX, c);
            const unsigned m = 1 + r.below(7);
            for (int k = 0; k < 3; ++k) if (m >> k & 1) o[k] = (r.next() & 1) ? c.lo[k] : c.hi[k];
            break;
        }
        case LARGE: {
            scale = std::fabs(r.logmag(1e3, GI_X_COORD_MAX));
            for (int k = 0; k < 3; ++k) o[k] = (r.next() & 3) ? scale * r.sym() : (r.next() & 1 ? GI_X_COORD_MAX : -GI_X_COORD_MAX);
            if (i & 8) zero_some_dirs(r, i >> 4, d);
            unit3(d);
            box_near(r, o, scale * (r.next() & 1 ? 1.0 : 1e-4), GI_X_COORD_MAX, c);
            if ((i & 48) == 48)   // the origin inside the box on the axes of zero direction: the case the limit is for
                for (int k = 0; k < 3; ++k) o[k] = 0.5 * ((double)c.lo[k] + (double)c.hi[k]);
            break;
        }
        case THIN: {
            scale = std::fabs(r.logmag(1e-3, 1e8));
            for (int k = 0; k < 3; ++k) o[k] = scale * r.sym();
            if (i & 8) zero_some_dirs(r, i >> 4, d);
            unit3(d);
            for (int k = 0; k < 3; ++k) {
                c.lo[k] = (float)(scale * r.sym());
                c.hi[k] = next_up_by(c.lo[k], (int)r.below(5));
            }
            if (i & 16) for (int k = 0; k < 3; ++k) if (r.next() & 1) o[k] = c.lo[k];
            break;
        }
        default: {   // TINY
            scale = std::fabs(r.logmag(1e-44, 1e-3));
            for (int k = 0; k < 3; ++k) o[k] = scale * r.sym();
            for (int k = 0; k < 3; ++k) if (r.below(3) == 0) d[k] = r.logmag(1e-45, 1e-3);
            unit3(d);
            box_near(r, o, scale, GI_X_COORD_MAX, c);
            break;
        }
    }
    for (int k = 0; k < 3; ++k) { c.o[k] = (float)o[k]; c.d[k] = (float)d[k]; }
    c.tmax = pick_tmax(r, scale);
    return c;
}

int run_identity(uint64_t n) {
    Tally tally[N_CLASSES];
    std::vector<std::thread> th;
    for (int cl = 0; cl < N_CLASSES; ++cl)
        th.emplace_back([cl, n, &tally] {
            Rng r{0x2019ull * 1000003ull + (uint64_t)cl};
            Tally t;   // (the thread's own: the array's elements share cache lines)
            for (uint64_t i = 0; i < n; ++i) check(make((Class)cl, r, i), t);
            tally[cl] = t;
        });
    for (std::thread& t : th) t.join();
    Tally sum;
    for (int cl = 0; cl < N_CLASSES; ++cl) {
        const Tally& t = tally[cl];
        std::printf("%-9s cases %llu mismatches %llu zero_sign %llu\n", kClassNames[cl], (unsigned long long)t.cases,
                    (unsigned long long)t.mismatches, (unsigned long long)t.zero_sign);
        if (t.have_first) {
            const Case& c = t.first;
            std::printf("  first: o %.9g %.9g %.9g d %.9g %.9g %.9g lo %.9g %.9g %.9g hi %.9g %.9g %.9g tmax %.9g\n", c.o[0], c.o[1], c.o[2],
                        c.d[0], c.d[1], c.d[2], c.lo[0], c.lo[1], c.lo[2], c.hi[0], c.hi[1], c.hi[2], c.tmax);
        }
        sum.cases += t.cases;
        sum.mismatches += t.mismatches;
        sum.zero_sign += t.zero_sign;
    }
    std::printf("cases %llu mismatches %llu zero_sign %llu\n", (unsigned long long)sum.cases, (unsigned long long)sum.mismatches,
                (unsigned long long)sum.zero_sign);
    return sum.mismatches ? 1 : 0;
}

bool read_scn(const char* path, std::vector<gi_entity_desc>& ents) {
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

int run_table(const char* path) {
    std::vector<gi_entity_desc> ents;
    if (!read_scn(path, ents)) { std::printf("%s: no entities\n", path); return 1; }
    gi_scene_desc sd{};
    double lo = INFINITY, hi = -INFINITY;
    for (const gi_entity_desc& e : ents)
        for (int k = 0; k < (e.kind == GI_IMP_TRIANGLE ? 9 : 3); ++k) { lo = std::fmin(lo, e.args[k]); hi = std::fmax(hi, e.args[k]); }
    const double pad = 0.5 * (hi - lo) + 4.0 * std::fmax(1.0, std::fmax(std::fabs(lo), std::fabs(hi)) * 1e-6);
    for (int k = 0; k < 3; ++k) { sd.octree_min[k] = lo - pad; sd.octree_max[k] = hi + pad; }
    sd.n_entities = (int32_t)ents.size();
    sd.entities = ents.data();
    HostScene hs;
    std::string err;
    if (!build_host_scene(sd, hs, err)) { std::printf("%s: build failed: %s\n", path, err.c_str()); return 1; }
    const std::vector<XFlatLeafDev> dev = xflat_device_table(hs);
    static const int kFrom[8] = {0, 3, 1, 4, 2, 5, 6, 7};   // device word j is host word kFrom[j]
    uint64_t bad = dev.size() == hs.xflat.size() ? 0 : 1;
    for (size_t i = 0; i < dev.size() && i < hs.xflat.size(); ++i) {
        uint32_t h[8], w[8];
        std::memcpy(h, &hs.xflat[i], 32);
        std::memcpy(w, &dev[i], 32);
        const XFlatLeaf& f = hs.xflat[i];
        bool ok = true;
        for (int j = 0; j < 8; ++j) ok = ok && w[j] == h[kFrom[j]];
        // as the kernel decodes them (gi_wf.hip step, flat_pack, wf_stage)
        ok = ok && (int32_t)w[6] == f.off && (w[7] & 0xFFFFu) == f.cnt && ((w[7] >> 16) & 0xFFu) == f.group && (w[7] >> 24) == f.fan;
        ok = ok && dev[i].off == f.off && dev[i].cnt == f.cnt && dev[i].group == f.group && dev[i].fan == f.fan;
        for (int k = 0; k < 3; ++k) ok = ok && bits(dev[i].lohi[k][0]) == bits(f.lo[k]) && bits(dev[i].lohi[k][1]) == bits(f.hi[k]);
        bad += ok ? 0 : 1;
    }
    std::printf("%s: leaves %zu mismatches %llu\n", path, hs.xflat.size(), (unsigned long long)bad);
    return bad ? 1 : 0;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc >= 3 && std::strcmp(argv[1], "identity") == 0) return run_identity(std::strtoull(argv[2], nullptr, 10));
    if (argc >= 3 && std::strcmp(argv[1], "table") == 0) {
        int rc = 0;
        for (int i = 2; i < argc; ++i) rc |= run_table(argv[i]);
        return rc;
    }
    std::printf("usage: xflat_pk_check identity <cases per class> | table scene.scn [...]\n");
    return 2;
}
