// x_region.h — where the Mode X checkers' rays start and aim (xaccel_check, xflat_check,
// xflat_phase_a_check).  The checker passes its own generator of uniform numbers in [0, 1).
//
// The scene's bounds widened by a tenth of their size on every side (point()), a camera one size before
// them on x, shadow rays 0.3 to 1.3 sizes long.  The built-in scenes' nominal bounds are
// [0, 10] x [-5, 5]^2 -- the region [-1, 11] x [-6, 6]^2 and the camera at (-10, 0, 0) the checkers
// always used -- and a .scn file gives its own (region_of), so a scene scaled or moved is sampled in
// the same proportions.  For the Cornell box where it is today both are the same numbers, bit for bit.
#pragma once
#include <cmath>
#include <vector>

#include "gi.h"
#include "gi_math.h"

struct Region {
    gi::V3 b = gi::v3(-1, -6, -6), w = gi::v3(12, 12, 12), cam = gi::v3(-10, 0, 0);
    double size = 10;
    double oct_lo[3] = {-20, -20, -20}, oct_hi[3] = {20, 20, 20};   // the .scn file's octree line
    gi::V3 point(double (*rnd)()) const { return gi::v3(rnd() * w.x + b.x, rnd() * w.y + b.y, rnd() * w.z + b.z); }
    gi::V3 cam_yz(gi::V3 p) const { return gi::v3(cam.x, p.y, p.z); }   // on the camera's x, looking along +x at p
    double shadow_tmax(double (*rnd)()) const { return 0.3 * size + size * rnd(); }
};
// the region of entities of ImpTriangles and ImpSpheres; `file` carries the octree bounds read with them
static inline Region region_of(const std::vector<gi_entity_desc>& ents, const Region& file) {
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (const gi_entity_desc& e : ents)
        for (int k = 0; k < 3; ++k) {
            if (e.kind == GI_IMP_SPHERE) {
                lo[k] = std::fmin(lo[k], e.args[k] - e.args[3]);
                hi[k] = std::fmax(hi[k], e.args[k] + e.args[3]);
            } else {
                for (int v = 0; v < 3; ++v) {
                    lo[k] = std::fmin(lo[k], e.args[3 * v + k]);
                    hi[k] = std::fmax(hi[k], e.args[3 * v + k]);
                }
            }
        }
    Region r = file;
    const gi::V3 l = gi::v3(lo[0], lo[1], lo[2]), s = gi::v3(hi[0] - lo[0], hi[1] - lo[1], hi[2] - lo[2]);
    r.b = gi::v3(l.x - 0.1 * s.x, l.y - 0.1 * s.y, l.z - 0.1 * s.z);
    r.w = gi::v3(1.2 * s.x, 1.2 * s.y, 1.2 * s.z);
    r.cam = gi::v3(l.x - s.x, l.y + 0.5 * s.y, l.z + 0.5 * s.z);
    r.size = std::fmax(s.x, std::fmax(s.y, s.z));
    return r;
}
