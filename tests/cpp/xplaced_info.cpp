// xplaced_info.cpp — what libgi's host builder (gi_build.cpp + gi_bvh.cpp, compiled here by g++) derives
// for a scene from the magnitude of its coordinates, one line per .scn file (octree / camera / light /
// impsphere / imptriangle lines): the structure's reach against the fp32 box tests' limit, the own-plane
// skip's bound a |cam| + b for the file's camera, the light-dead bound, the flat table's leaves, its fan
// pairs, and the boundary and live masks of the file's light as a launch from the file's camera gets them
// (gi_scene.h x_shadow_live with the far radius gi_capi.cpp sets).  The device tests compare a device
// scene's accessors with these.
//   xplaced_info a.scn ...
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "gi.h"
#include "gi_scene.h"

using namespace gi;

int main(int argc, char** argv) {
    for (int i = 1; i < argc; ++i) {
        std::vector<gi_entity_desc> ents;
        double oct[6] = {-20, -20, -20, 20, 20, 20}, cam[3] = {-10, 0, 0}, light[3] = {0, 0, 0};
        std::ifstream f(argv[i]);
        std::string line;
        while (std::getline(f, line)) {
            std::istringstream is(line);
            std::string kw;
            is >> kw;
            std::vector<double> v;
            double x;
            while (is >> x) v.push_back(x);
            if (kw == "octree" && v.size() == 6) for (int k = 0; k < 6; ++k) oct[k] = v[k];
            if (kw == "camera" && v.size() >= 3) for (int k = 0; k < 3; ++k) cam[k] = v[k];
            if (kw == "light" && v.size() >= 3) for (int k = 0; k < 3; ++k) light[k] = v[k];
            gi_entity_desc e{};
            if (kw == "imptriangle") e.kind = GI_IMP_TRIANGLE;
            else if (kw == "impsphere") e.kind = GI_IMP_SPHERE;
            else continue;
            for (size_t k = 0; k < v.size() && k < 11; ++k) e.args[k] = v[k];
            ents.push_back(e);
        }
        gi_scene_desc sd{};
        for (int k = 0; k < 3; ++k) { sd.octree_min[k] = oct[k]; sd.octree_max[k] = oct[3 + k]; }
        sd.n_entities = (int32_t)ents.size();
        sd.entities = ents.data();
        HostScene hs;
        std::string err;
        if (!build_host_scene(sd, hs, err)) { std::printf("build failed: %s\n", err.c_str()); return 2; }
        const double reach = x_coord_reach(hs);
        const double cm = std::fmax(std::fabs(cam[0]), std::fmax(std::fabs(cam[1]), std::fabs(cam[2])));
        const XShadowLeaves sl = shadow_leaves_of(hs);
        const uint32_t live = x_shadow_live(sl, light, cam, 16.0 * (double)(float)reach, false) & sl.table_mask();
        std::printf("info %s: reach %.17g inside %d skip_a %.17g skip_b %.17g skip_cos %.17g dead_c %.17g nodes %zu leaves %zu "
                    "flat_ok %d fan %d boundary %08x live %08x\n", argv[i], reach, (int)(reach <= GI_X_COORD_MAX), hs.x_skip_a,
                    hs.x_skip_b, hs.x_skip_a * cm + hs.x_skip_b, hs.x_dead_c, hs.xwnodes.size(), hs.xflat.size(), (int)hs.x_flat_ok,
                    hs.n_fan_leaves, sl.boundary_mask(), live);
    }
    return 0;
}
