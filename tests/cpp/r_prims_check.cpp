// The product's host-compiled primitive tests (gi_math.h) over a record file of tests/r_prims_cases.py:
//   r_prims_check tris|boxes|spheres <in> <out>
// in:  int32 n, then n records of 15 (p1 p2 p3 o dir), 12 (min max o dir) or 10 (pos radius o dir) doubles;
//      dir is normalised here as the reference's Ray constructor does.
// out: per record int32 hit, int32 hit2, double P[3], N[3] (P and N start as zeros):
//   tris     hit = make_tri + tri_hit(TriRec) (the entity path), hit2 = tri_hit_corners (the node-test path,
//            the same triangle without its stored normal)
//   boxes    hit = box_hit, hit2 = the OR of the four box_hit_part parts; P, N stay zeros
//   spheres  hit = hit2 = sphere_hit with the radius narrowed to float as REnt stores it
// tests/test_r_prims_host.py compares every record with the oracle; this program only computes.
#include "gi_math.h"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace gi;

#pragma pack(push, 1)
struct Out {
    int32_t hit, hit2;
    double pn[6];
};
#pragma pack(pop)

int main(int argc, char** argv) {
    if (argc < 4) { fprintf(stderr, "usage: r_prims_check tris|boxes|spheres <in> <out>\n"); return 2; }
    const int kind = !strcmp(argv[1], "tris") ? 0 : !strcmp(argv[1], "spheres") ? 1 : !strcmp(argv[1], "boxes") ? 2 : -1;
    if (kind < 0) { fprintf(stderr, "unknown kind %s\n", argv[1]); return 2; }
    const size_t width = kind == 0 ? 15 : kind == 1 ? 10 : 12;
    FILE* f = fopen(argv[2], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[2]); return 1; }
    int32_t n = 0;
    if (fread(&n, 4, 1, f) != 1 || n < 0) { fprintf(stderr, "bad header\n"); return 1; }
    std::vector<double> recs((size_t)n * width);
    if (fread(recs.data(), 8, recs.size(), f) != recs.size()) { fprintf(stderr, "short file\n"); return 1; }
    fclose(f);
    std::vector<Out> out((size_t)n);
    for (int i = 0; i < n; ++i) {
        const double* q = &recs[width * (size_t)i];
        V3 P = v3(0, 0, 0), N = v3(0, 0, 0);
        Out& r = out[(size_t)i];
        if (kind == 0) {
            const V3 p1 = v3(q[0], q[1], q[2]), p2 = v3(q[3], q[4], q[5]), p3 = v3(q[6], q[7], q[8]);
            const V3 o = v3(q[9], q[10], q[11]), d = normalize(v3(q[12], q[13], q[14]));
            TriRec t;
            make_tri(p1, p2, p3, t);
            r.hit = tri_hit(t, o, d, P, N) ? 1 : 0;
            r.hit2 = tri_hit_corners(p1, p2, p3, o, d) ? 1 : 0;
        } else if (kind == 1) {
            r.hit = sphere_hit(v3(q[0], q[1], q[2]), (float)q[3], v3(q[4], q[5], q[6]), normalize(v3(q[7], q[8], q[9])), P, N) ? 1 : 0;
            r.hit2 = r.hit;
        } else {
            const V3 mn = v3(q[0], q[1], q[2]), mx = v3(q[3], q[4], q[5]), o = v3(q[6], q[7], q[8]);
            const V3 d = normalize(v3(q[9], q[10], q[11]));
            r.hit = box_hit(mn, mx, o, d) ? 1 : 0;
            r.hit2 = (box_hit_part(mn, mx, o, d, 0) || box_hit_part(mn, mx, o, d, 1) || box_hit_part(mn, mx, o, d, 2) ||
                      box_hit_part(mn, mx, o, d, 3)) ? 1 : 0;
        }
        r.pn[0] = P.x; r.pn[1] = P.y; r.pn[2] = P.z; r.pn[3] = N.x; r.pn[4] = N.y; r.pn[5] = N.z;
    }
    FILE* o = fopen(argv[3], "wb");
    if (!o) { fprintf(stderr, "cannot write %s\n", argv[3]); return 1; }
    const bool ok = fwrite(out.data(), sizeof(Out), out.size(), o) == out.size();
    fclose(o);
    printf("%s records %d\n", argv[1], (int)n);
    return ok ? 0 : 1;
}
