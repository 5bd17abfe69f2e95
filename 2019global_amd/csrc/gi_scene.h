// gi_scene.h — device-resident scene layout (HBM) and the host-side builder interface.
//
// Mode R keeps the reference octree exactly (octree.h:12-163, including SURVEY A.4-A.6, A.14):
//   RNode[]   64 B/node: AABB (fp64) + child0 / parent / leaf list range.  Children of a node are
//             8 consecutive records in octant order 0..7 (octree.h:94-108).
//   leaf_ents int32 entity indices, each leaf's list in push order.
//   REnt[]    entity records (kind, material, sphere/quad parameters) + TriRec[] triangles.
// Mode X uses its own tight octree over primitives (XWNode[] traversal nodes, XHot[] leaf records,
// XPrim[] shading records).
#pragma once
#include <stdint.h>
#include <string>
#include <type_traits>
#include <vector>

#include "gi.h"
#include "gi_math.h"

namespace gi {

// camera basis and frame corner of raytracer.h:26-30: made on the host (gi_capi.cpp make_cam), passed to
// the kernels by value
struct CamDev {
    V3 pos, up, left, top_left;
    double rx, ry;
};

enum EntKind : int32_t { K_IMP_SPHERE = 1, K_IMP_TRIANGLE = 2, K_EXP_QUAD = 3, K_EXP_SPHERE = 4, K_EXP_CUBE = 5,
                         K_EXP_CONE = 6, K_EXP_RECTANGLE = 7, K_EXP_BOX = 8 };

struct RNode {             // 64 bytes
    double mn[3], mx[3];
    int32_t child0;        // -1: leaf
    int32_t parent;        // -1: root
    int32_t ent_off;       // leaves: offset into leaf_ents
    int32_t ent_cnt;       // size of the node's _entities (interior: only emptiness is used, octree.h:140)
};
static_assert(sizeof(RNode) == 64, "RNode layout");

// Mode R reachability records (the flat reach phase and the candidate walks, round 5): a leaf's root
// path laid out as consecutive node records, so a walk down it streams one record after another (the
// next load issued before the current exact node test) instead of chasing rpath[i] -> rnodes[...].
struct RPathRec {          // 64 bytes: the node's box, its id (memo key) and emptiness
    double mn[3], mx[3];
    int32_t node;
    int32_t ent_cnt;
    int32_t pad[2];
};
static_assert(sizeof(RPathRec) == 64, "RPathRec layout");
struct RApp {              // 16 bytes: one appearance of an entity, by decreasing rank
    int64_t rank;          // (leaf's rank in the reference's DFS order << 32) | position
    int32_t p0, p1;        // its leaf's root path: rpath_rec[p0 .. p1), top-down
};
static_assert(sizeof(RApp) == 16, "RApp layout");

struct REnt {              // 208 bytes
    int32_t kind, tri_first, tri_count, pad0;
    double pos[3];         // ImpSphere / ExpSphere / ExpCone centre, ExpQuad / ExpCube pos
    float radius, width, length, alpha;
    double qv0[3], qv1[3], qv2[3];   // texture frames: ExpQuad vertices[0], [1] (entities.h:634-635);
                                     // ExpCube vertices[0] (:772); ExpRectangle p1, p3, p4 (:346-350)
    double color[3], shader[3];
    double spec_pow;
    float height, pad1;    // ExpCube / ExpCone height
    double sin_theta;      // ExpCone: sin(cone_theta), cone_theta = float atan(radius/height) (:950-953)
    double refl;           // Mode X mirror-reflection probability (gi_entity_desc::mat_reflectivity)
};
static_assert(sizeof(REnt) == 208, "REnt layout");

// Mode X primitive: triangle (v0, e1, e2, n) or sphere (c, r)
struct XPrim {             // 112 bytes
    double a[3];           // triangle v0 | sphere centre
    double b[3];           // triangle e1 | sphere (r, 0, 0)
    double c[3];           // triangle e2
    double n[3];           // triangle geometric normal normalize(cross(e1,e2))
    int32_t kind;          // 0 triangle, 1 sphere
    int32_t ent;
    int32_t pad[2];        // pad[0]: plane group (gi_build.cpp assign_plane_groups; 255 none)
};
static_assert(sizeof(XPrim) == 112, "XPrim layout");

struct XNode {             // 64 bytes
    double mn[3], mx[3];   // conservative AABB of the cell
    int32_t child_base;    // interior: index of the first existing child (children contiguous)
    int32_t child_mask;    // interior: bit c set if octant c exists; 0 for a leaf
    int32_t prim_off;      // leaf: range in xprim_idx
    int32_t prim_cnt;
};
static_assert(sizeof(XNode) == 64, "XNode layout");

// Mode X traversal node: the 8 children of one octree cell, each child's tight box in fp32
// rounded outward and padded (conservative culling; the fp64 primitive tests decide hits).
constexpr int32_t XEMPTY = (int32_t)0x80000000;
struct XWNode {            // 256 bytes, 2 cache lines
    float lo[3][8];        // child box minima, SoA over the 8 octants
    float hi[3][8];
    int32_t child[8];      // >= 0: wide node; < 0 (not XEMPTY): leaf = ~(offset into xhot[]); XEMPTY: none
    int32_t parent;        // wide node of the parent cell, -1 at the root (stackless traversal)
    uint16_t cnt[8];       // leaf children: number of xhot records
    int32_t exists;        // bit c set iff child[c] != XEMPTY (branch-free culling)
    int32_t pad[2];        // byte c: plane group of leaf child c, 255 none (Mode X scene nodes)
};
static_assert(sizeof(XWNode) == 256, "XWNode layout");
// The same node quantised into one 128-byte cache line (HBM-resident scenes, k_mode_x): child c's
// box on axis a is lo = fma(qlo[a][c], 2^ex[a], org[a]), hi = fma(qhi[a][c], 2^ex[a], org[a]) in
// fp32, with the 8-bit q chosen on the host -- by the device's own fused arithmetic -- so that the
// decoded box contains XWNode's padded box (culling stays conservative).  Children, counts and
// parent as in XWNode (counts <= 255; a scene with a larger leaf keeps XWNode).
struct XCNode {            // 128 bytes
    float org[3];
    int8_t ex[3];
    uint8_t exists;        // bit c set iff child[c] != XEMPTY
    uint8_t qlo[3][8];
    uint8_t qhi[3][8];     // bytes 0..63: what the slab tests read (four 16-byte loads)
    int32_t child[8];
    uint8_t cnt[8];
    int32_t parent;
    int32_t pad[5];
};
static_assert(sizeof(XCNode) == 128, "XCNode layout");
// Encodes w as XCNode (the decode above contains every child's box); false if a count exceeds 255.
bool encode_xcnodes(const std::vector<XWNode>& w, std::vector<XCNode>& out);

// Leaf primitive records, duplicated per leaf reference and stored contiguously per leaf, so a
// leaf costs one dependent load level: exactly what Moller-Trumbore / the sphere test read.
struct XHot {              // 80 bytes
    double a[3], b[3], c[3];   // triangle v0, e1, e2 | sphere centre, (r, 0, 0)
    int32_t prim;          // global primitive index (tie-break, shading record)
    int32_t kind;          // 0 triangle, 1 sphere
};
static_assert(sizeof(XHot) == 80, "XHot layout");
// fp32 prefilter record parallel to xhot[]: the primitive's AABB rounded outward and padded, so a
// ray that misses it cannot hit the primitive; the 80-B fp64 record is fetched only otherwise.
struct XBox {              // 32 bytes
    float lo[3], hi[3];
    int32_t pad[2];
};
static_assert(sizeof(XBox) == 32, "XBox layout");
struct XLeaf {
    int32_t off, cnt;      // host build only: range in xprim_idx
};
// Flat leaf table (build_xflat; gi_wf.hip wf_flat): one record per leaf child of the wide tree, in
// node order then child order.  lo / hi are the very floats of the child's XWNode box, so the
// proof that those padded boxes are conservative covers the table too.
#ifndef GI_XFLAT_MAX
#define GI_XFLAT_MAX 32    // most leaves of a scene that answers its queries from the table
#endif
static_assert(GI_XFLAT_MAX >= 1 && GI_XFLAT_MAX <= 32, "the candidate mask is one 32-bit word");
struct XFlatLeaf {         // 32 bytes
    float lo[3], hi[3];
    int32_t off;           // the leaf's first record in xhot[]
    uint16_t cnt;          // its records
    uint8_t group;         // its plane group (byte c of XWNode::pad; 255 none)
    uint8_t fan;           // 1: its two records are a fan pair (gi_fan_pair.h fan_pair_ok); host-side only
};
static_assert(sizeof(XFlatLeaf) == 32, "XFlatLeaf layout");
// The table as the device reads it (DevScene::xflat; xflat_device_table): the same eight words with each
// axis's two planes side by side, so that a scalar register pair (lo_a, hi_a) is one operand of wf_flat's
// packed plane distances (DESIGN.md §5 "Two-stage slab distances").  Words 6 and 7 stay where they were.
struct XFlatLeafDev {      // 32 bytes
    float lohi[3][2];      // [axis][0: lo, 1: hi]
    int32_t off;
    uint16_t cnt;
    uint8_t group;
    uint8_t fan;
};
static_assert(sizeof(XFlatLeafDev) == 32, "XFlatLeafDev layout");
// A leaf of the flat table as a boundary of the scene (gi_build.cpp mark_boundary_leaves; DESIGN.md §5
// "light-dead leaves"): every record of the leaf lies in the plane n . x = c (one plane group), and every
// primitive of the scene on the closed side(s) named by `sides`.  A shadow ray toward a light that lies on
// such a side, at least XShadowLeaves::delta from the plane, cannot be occluded by the leaf.
struct XLeafPlane {
    double n[3], c;
    int32_t sides;         // bit 0: the scene lies in n . x - c >= -tau; bit 1: in n . x - c <= tau; 0: no boundary leaf
    int32_t pad;
};
// The boundary leaves of a scene's table and the bound of the light-dead rule, as a launch reads them.
struct XShadowLeaves {
    int32_t n = 0;               // leaves of the table (0: the rule does not apply; every mask is full)
    XLeafPlane pl[GI_XFLAT_MAX] = {};
    double dead_c = INFINITY;    // delta(L) = dead_c * ldist_max(L)
    double ext = 0.0;            // E: the largest |coordinate| of a primitive
    // the least distance of the light from a boundary leaf's plane at which the leaf is dead: dead_c times a
    // bound on the length of a shadow ray toward L (both ends within E of the origin, or L farther out)
    double delta(const double* L) const {
        const double lm = std::fmax(std::fabs(L[0]), std::fmax(std::fabs(L[1]), std::fabs(L[2])));
        return dead_c * (1.7320508075688774 * (lm + ext));
    }
    uint32_t table_mask() const { return n >= 32 ? ~0u : (1u << n) - 1u; }
    uint32_t boundary_mask() const {
        uint32_t b = 0;
        for (int k = 0; k < n; ++k) b |= pl[k].sides ? 1u << k : 0u;
        return b;
    }
    // bit k: leaf k can occlude a shadow ray toward L (a NaN anywhere keeps the leaf)
    uint32_t live_mask(const double* L) const {
        const double dl = delta(L);
        uint32_t live = table_mask();
        for (int k = 0; k < n; ++k) {
            const double s = (pl[k].n[0] * L[0] + pl[k].n[1] * L[1] + pl[k].n[2] * L[2]) - pl[k].c;
            if (((pl[k].sides & 1) && s >= dl) || ((pl[k].sides & 2) && -s >= dl)) live &= ~(1u << k);
        }
        return live;
    }
};

struct HostScene {
    // Mode R
    std::vector<RNode> rnodes;
    std::vector<int32_t> leaf_ents;
    std::vector<REnt> ents;
    std::vector<TriRec> tris;
    int32_t max_depth = 0, n_leaves = 0, n_reachable = 0, n_dropped = 0;
    // Mode X
    std::vector<XNode> xnodes;
    std::vector<XWNode> xwnodes;
    std::vector<XCNode> xcnodes;     // xwnodes quantised (encode_xcnodes), for HBM-resident scenes
    std::vector<XLeaf> xleaves;
    std::vector<int32_t> xprim_idx;
    std::vector<XHot> xhot;
    std::vector<XBox> xbox;
    std::vector<XPrim> xprims;
    int32_t x_max_depth = 0;
    // Mode R candidate reconstruction (gi_bvh.cpp build_rcand; DESIGN.md §5 k_mode_r)
    std::vector<int32_t> app_off;    // per entity (n_ents + 1): its appearances in leaf lists
    std::vector<int32_t> app_leaf;   //   leaf node of each appearance, by decreasing rank
    std::vector<int64_t> app_rank;   //   (leaf's rank in the reference's DFS order << 32) | position
    std::vector<int32_t> rpath_off;  // per node (n_rnodes + 1): its path below the root, top-down
    std::vector<int32_t> rpath;      //   (filled for leaves; the leaf itself is the last entry)
    std::vector<RPathRec> rpath_rec; // rpath's node records, in the same order (the device reads these)
    std::vector<RApp> app_rec;       // app_rank / app_leaf as (rank, path range) records (device)
    std::vector<XWNode> rc_nodes;    // line BVH over the non-sphere entities that appear in a leaf
    std::vector<int32_t> rc_ent;     //   entity of each leaf record
    std::vector<int64_t> rc_maxkey;  //   per node slot (8 per node): the highest app_rank under it;
                                     //   a node's slots are in decreasing order of it
    std::vector<int32_t> r_always;   // ImpSpheres that appear in a leaf (tested by every ray)
    std::vector<int32_t> r_leaf_of_rank;   // leaf node of each DFS rank (app_rank >> 32)
    double rc_ext = 0;               // max |coordinate| of the line BVH's boxes
    int32_t x_handle8 = 6;   // Mode X handler threshold (eighths), chosen by the builder
    int32_t x_flags = 0;     // Mode X schedule flags (DevScene::x_flags), chosen by the builder
    double x_est_nodes = 0, x_est_prims = 0;   // SAH estimates per random ray through the root
    bool x_spatial = false;  // the Mode X BVH was built with spatial splits (a primitive in several leaves)
    double x_skip_a = 0.0, x_skip_b = 2.0;   // own-plane leaf skip: |d . n| >= a * max|cam| + b (gi_build.cpp)
    std::vector<XFlatLeaf> xflat;    // the wide tree's leaf children (build_xflat)
    bool x_flat_ok = false;          // xflat fits the flat query: <= GI_XFLAT_MAX leaves of <= 255 records each,
                                     // offsets below 2^16 (wf_flat packs offset, index and count in a word)
    int32_t n_fan_leaves = 0;        // leaves of xflat that are fan pairs (XFlatLeaf::fan)
    bool x_fan_all = false;          // every leaf of xflat is one (and there is a leaf): wf_flat's TRI kernels run
                                     // one exact test per leaf where the first step decides (DevScene::x_fan)
    struct XPlane { double n[3], c; };
    std::vector<XPlane> x_planes;    // the plane groups' planes, by group id (assign_plane_groups)
    double x_tau = 0.0, x_ext = 0.0; // their measured coplanarity tolerance; E, the largest |coordinate| of a primitive
    std::vector<XLeafPlane> xflat_plane;   // per leaf of xflat: its boundary record (mark_boundary_leaves)
    double x_dead_c = INFINITY;      // the light-dead rule's bound per unit of shadow-ray length (XShadowLeaves::dead_c)
};
// Builds every host structure of a scene from its description (gi_build.cpp); false: err says why.
bool build_host_scene(const gi_scene_desc& desc, HostScene& hs, std::string& err);
// The largest |bound| of a Mode X structure's fp32 boxes (padding included) the box tests are exact
// about: FLT_MAX / (1e30f (1 + 2^-23)) = 3.40282e8, rounded down (gi_dev.h inv_dir derives it).
// gi_scene_create refuses a scene beyond it.
constexpr double GI_X_COORD_MAX = 3.4e8;
// The largest |bound| of hs's fp32 child boxes: the root node's (a child's box lies inside its parent's,
// both padded alike); 0 without a primitive.
inline double x_coord_reach(const HostScene& hs) {
    double m = 0.0;
    if (!hs.xwnodes.empty())
        for (int c = 0; c < 8; ++c)
            if (hs.xwnodes[0].child[c] != XEMPTY)
                for (int k = 0; k < 3; ++k)
                    m = std::fmax(m, std::fmax(std::fabs((double)hs.xwnodes[0].lo[k][c]), std::fabs((double)hs.xwnodes[0].hi[k][c])));
    return m;
}
// A lower bound of it known before the build: the largest |coordinate| of the ImpTriangles' vertices and the
// ImpSpheres' extents (other kinds and NaNs add nothing: the built structure decides those).
inline double x_desc_reach(const gi_scene_desc& desc) {
    double m = 0.0;
    for (int32_t i = 0; desc.entities && i < desc.n_entities; ++i) {
        const gi_entity_desc& e = desc.entities[i];
        const int n = e.kind == GI_IMP_TRIANGLE ? 9 : e.kind == GI_IMP_SPHERE ? 3 : 0;
        const double r = e.kind == GI_IMP_SPHERE ? std::fabs(e.args[3]) : 0.0;
        for (int k = 0; k < n; ++k) {
            const double v = std::fabs(e.args[k]) + r;
            if (v > m) m = v;
        }
    }
    return m;
}
// Fills hs.xflat / x_flat_ok from hs.xwnodes (after assign_plane_groups: the group bytes are copied).
void build_xflat(HostScene& hs);
// hs.xflat in the device's word order (XFlatLeafDev), record for record: what the scene upload copies.
std::vector<XFlatLeafDev> xflat_device_table(const HostScene& hs);
// Fills hs.xflat_plane / x_dead_c from xflat, the plane groups and the primitives (build_xflat calls it).
void mark_boundary_leaves(HostScene& hs);
// The launch's copy of them (empty unless the table fits the flat query).
XShadowLeaves shadow_leaves_of(const HostScene& hs);
// The 32-bit mask of table leaves a launch's shadow queries visit (the kernels' shadow_live argument; all ones: every leaf, the
// dense loop): full when the rule does not apply to the launch -- the flat query is not the scene's, no shadow
// rays, the test flag, or a far camera (max |cam| above far_r: the hit points of its primary rays carry the
// camera's rounding, which the bound does not budget).
inline uint32_t x_shadow_live(const XShadowLeaves& sl, const double* light, const double* cam_pos, double far_r, bool full) {
    const double cm = std::fmax(std::fabs(cam_pos[0]), std::fmax(std::fabs(cam_pos[1]), std::fabs(cam_pos[2])));
    if (full || sl.n == 0 || !(cm <= far_r)) return ~0u;
    const uint32_t live = sl.live_mask(light);
    return live == sl.table_mask() ? ~0u : live;
}

// Sets XWNode::exists from the child references (both Mode X builders call it last).
inline void finalize_xwnodes(std::vector<XWNode>& w) {
    for (XWNode& n : w) {
        n.exists = 0;
        for (int c = 0; c < 8; ++c)
            if (n.child[c] != XEMPTY) n.exists |= 1 << c;
    }
}

// Mode X 8-wide BVH over the primitives (gi_bvh.cpp); bounds: 6 doubles (min xyz, max xyz) each.
// geometric: the prims hold their geometry (Mode X), so large scenes may use spatial splits; the
// Mode R line BVH passes boxes only.
void build_xbvh(const std::vector<XPrim>& prims, const std::vector<double>& bounds, int leaf_max, HostScene& hs,
                bool geometric = false);
// Mode R candidate reconstruction structures (HostScene app_* / rpath* / rc_* / r_always) from the
// reference octree (rnodes, leaf_ents) and the entities' triangles.
void build_rcand(HostScene& hs);

// Device view passed to kernels by value.
struct DevScene {
    const RNode* rnodes;
    const int32_t* leaf_ents;
    const REnt* ents;
    const TriRec* tris;
    const XWNode* xwnodes;
    const XCNode* xcnodes;   // quantised copy of xwnodes (null: the scene keeps XWNode everywhere)
    const XHot* xhot;
    const XBox* xbox;
    const XPrim* xprims;
    unsigned* work;        // 16 device counters (persistent-kernel tile queue), reset per launch
    int32_t n_rnodes, n_ents, n_xwnodes, n_xprims;
    int32_t x_max_depth;
    int32_t x_handle8;     // Mode X shading-handler threshold, eighths of the live lanes (set at upload)
    int32_t x_flags;       // Mode X schedule flags (XFlag): XF_INLINE_SHADOW or 0
    int32_t n_xhot;
    int32_t x_lds_bytes;   // > 0: xwnodes + xhot fit in LDS and are staged there by each workgroup
    int32_t x_waves4;      // LDS-resident scene with light shading: gi_wf.hip's kernels at 4 waves per SIMD
    int32_t x_tri_only;    // every primitive a triangle, every entity ImpTriangle / ExpQuad / ExpCube /
                           // ExpBox (the 4-wave kinds): k_mode_x's TRI specialisation
    int32_t r_tri_only;    // every entity an ImpTriangle: the Mode R kernels' TRI specialisation
    float root_lo[3], root_hi[3];   // Mode X: union of the root's fp32 child boxes (conservative)
    double x_skip_a, x_skip_b;      // Mode X own-plane leaf skip bound (HostScene, gi_build.cpp)
    // Mode R candidate reconstruction (HostScene fields of the same names)
    const int32_t* app_off;
    const RApp* app_rec;
    const RPathRec* rpath_rec;
    const XWNode* rc_nodes;
    const int32_t* rc_ent;
    const int64_t* rc_maxkey;
    const int32_t* r_always;
    const int32_t* r_leaf_of_rank;
    int32_t n_r_always;
    float rc_ext;
    // Mode X flat leaf table (HostScene::xflat in the device's word order), read through the constant cache at
    // wave-uniform addresses
    const XFlatLeafDev* xflat;
    int32_t n_xflat;
    int32_t x_flat;        // 1: the scene is staged in LDS and its table fits (k_seg / k_wf_bounce use wf_flat)
    float x_far_r;         // 16 x max |coordinate| of root_lo / root_hi (inf: no primitive): rays that start
                           // farther out run their fp32 box tests from a point near the scene (gi_dev.h ray_org32)
    int32_t x_fan;         // 1: x_flat and every leaf of the table is a fan pair (HostScene::x_fan_all), unless
                           // GI_X_FAN=0: wf_flat<., true> runs one exact test per leaf where gi_fan_pair.h decides
};
// (x_fan fills what was tail padding: the kernels' argument layouts are those of the struct without it)
static_assert(sizeof(DevScene) == 264, "DevScene layout");

// HIP events bracketing the dominant kernel of renders issued with GI_FLAG_TIME (owned by the
// scene handle, created on first use): a ring of kRing pairs, so frames stay asynchronous; a pair
// about to be reused is folded into the running sum first (it ended kRing frames ago).
struct KTimer {
    static constexpr int kRing = 64;
    void* ev0[kRing] = {};   // hipEvent_t
    void* ev1[kRing] = {};
    long long recorded = 0;  // pairs recorded since the last read
    double sum_ms = 0.0;     // folded pairs
    long long folded = 0;
};

// Mode X per-launch work buffers, owned by the scene handle (gi_capi.cpp) and grown on demand:
// the list of pixel slots left after the background test and, for spp > 1, every listed pixel's
// per-sample radiance (summed in sample order by k_x_reduce).
struct XScratch {
    unsigned* list = nullptr;   // cap entries
    double* part = nullptr;     // cap * spp * 3 doubles
    long long cap = 0;          // pixel slots the buffers hold
    int spp = 0;                // samples per pixel the part buffer was sized for
    // wavefront Mode X (gi_wf.hip): two path queues of wcap entries (SoA: 12 fp64 fields + a
    // (list index, sample) pair = 104 B per entry) and 2 device counters per bounce
    double* wq[2] = {nullptr, nullptr};
    unsigned* wid[2] = {nullptr, nullptr};
    unsigned* wcnt = nullptr;
    long long wcap = 0;
    // flat Mode R (gi_mode_r.hip k_rf_*): candidate pairs, one word each -- every tile's own region
    // of GI_RF_S0, then the pool of rf_pages pages of GI_RF_PAGE (rf_pairs holds both); per tile its
    // pool page ids (GI_RF_KMAX), its pairs / hits and its first chunk of hits; per pixel slot the best
    // rank + 1 and the primary direction; the counters (pool pages taken, overflowed tiles) and the
    // overflowed tiles' list; the segment offsets and hit counts.  Sized for rf_slots pixel slots.
    unsigned* rf_pairs = nullptr;
    unsigned* rf_pt = nullptr;
    unsigned long long* rf_best = nullptr;
    double* rf_dir = nullptr;
    unsigned* rf_cnt = nullptr;
    unsigned* rf_ovf = nullptr;
    unsigned* rf_rcnt = nullptr;
    unsigned* rf_soff = nullptr;    // per tile + 1: its first segment of pairs (k_rf_hit's unit)
    unsigned* rf_shc = nullptr;     // per segment: its hits
    unsigned* rf_sreg = nullptr;    // per segment: its tile
    unsigned* rf_hoff = nullptr;    // per segment + 1: the hits before it (k_rf_reach's chunks of 64)
    unsigned rf_pages = 0;
    long long rf_slots = 0;
    size_t rf_bytes = 0;
    long long rf_failed = 0;   // pixel slots for which the allocation failed (0: none): not retried for
                               // that many or more; such frames render through k_mode_r_batch
    // adaptive sampling (gi_adapt.hip): the second of the two ping-pong lists of active pixel slots (the first is
    // `list`, which the classify pass fills), their two device counts (ad_cnt[q]: entries of list q) and the
    // per-slot state -- S1[3], S2[3] (ad_sum, 6 doubles per slot) and n with its flags (ad_n) -- for ad_cap
    // slots.  A pass's rows go to `part`, as [active index][k][3] for its k samples.
    unsigned* ad_list = nullptr;
    unsigned* ad_cnt = nullptr;
    double* ad_sum = nullptr;
    int32_t* ad_n = nullptr;
    long long ad_cap = 0;
};

// The Mode X kernels' xflags argument: the scene's schedule flags (DevScene::x_flags) and the launch's.
enum XFlag : int {
    XF_INLINE_SHADOW = 1 << 0,   // k_mode_x continues paths from shadow rays in traversal (the builder's choice)
    XF_NO_SHADOW = 1 << 2,       // GI_FLAG_X_NO_SHADOW (tests): no shadow rays, every light visible
    XF_HANDOFF = 1 << 3,         // the shadow-ray handoff is allowed (GI_X_HELP; used by the HELP builds)
    XF_SPREAD = 1 << 4,          // spread work groups (launches that run the handoff build)
    XF_PIXEL_MAJOR = 1 << 5,     // pixel-major work blocks
    XF_NO_FLAT = 1 << 6,         // GI_X_FLAT=0: gi_wf.hip's forms walk the tree although the flat leaf table applies
    XF_SEG_RING = 1 << 7,        // k_seg refills from its per-wave ring of prepared primary rays (XLaunchCfg::seg_ring)
    XF_RUN_SHIFT = 8, XF_RUN_MASK = 7,   // bits 8-10: log2 of the maximum run length (GI_X_MAX_RUN)
};

// The run-time choices that pick an instantiation of gi_wf.hip's kernels (k_seg, k_wf_bounce, k_cast, the
// query KAT) besides the scene's own properties.  k_mode_x reads neither field: it traverses every scene
// in global memory (gi_kernels.hip x_dispatch).
struct XVariant {
    bool lds = false;    // the scene is staged in LDS (DevScene::x_lds_bytes > 0)
    bool w4 = false;     // ... and its shading is light: 4 waves per SIMD (DevScene::x_waves4)
};
// An instantiation of gi_wf.hip's kernels as a type: what wf_dispatch hands to its callers.
template <bool STATS, bool LDS, bool W4, bool SH, bool TRI, bool CN, bool FLAT>
struct XTag {
    static constexpr bool stats = STATS, lds = LDS, w4 = W4, sh = SH, tri = TRI, cn = CN, flat = FLAT;
};
// f(std::bool_constant<b>...) for run-time booleans b...
template <bool... Bs, typename F>
void with_bools(F&& f) {
    f(std::integral_constant<bool, Bs>{}...);
}
template <bool... Bs, typename F, typename... R>
void with_bools(F&& f, bool b, R... r) {
    if (b) with_bools<Bs..., true>(f, r...);
    else with_bools<Bs..., false>(f, r...);
}

// Mode X form of a launch (x_form_choice; the values are gi_scene_x_form's, part of the ABI): the
// persistent path-state kernel (k_mode_x), the wavefront form (k_wf_bounce once per bounce over compacted
// queues), the segment-synchronous form (k_seg).
enum XForm : int { XFORM_MEGA = 0, XFORM_WF = 1, XFORM_SEG = 2 };
// Mode R kernel of a launch (r_kernel_choice; the values are gi_scene_r_kernel's, part of the ABI): k_mode_r
// (one lane per pixel), the flat phases (k_rf_*), k_mode_r_batch for the whole frame.
enum RKernel : int { RK_PIXEL = 0, RK_FLAT = 1, RK_BATCH = 2 };
// gi_wf.hip's kernels whose occupancy is queried per scene (wf_occupancy): k_wf_bounce, k_seg, k_seg with
// its per-wave ring, k_cast closest hit and any hit, k_aov, k_rad.
enum WfKernel { WK_BOUNCE, WK_SEG, WK_SEG_RING, WK_CAST, WK_OCCL, WK_AOV, WK_RAD, WK_COUNT };

// Mode X launch configuration, computed once per scene when it is created (gi_capi.cpp, on the
// scene's device): kernel variant, dynamic LDS bytes and the resident persistent grids.
struct XLaunchCfg {
    XVariant var;            // gi_wf.hip's kernels: their variant
    size_t lds_bytes = 0;    // k_mode_x: dynamic LDS per workgroup (level stack and handoff slots, any scene)
    int resident = 1;        //   and its resident 256-thread workgroups on the device (occupancy x CUs)
    size_t wf_lds_bytes = 0; // gi_wf.hip's kernels (k_wf_bounce, k_cast, k_aov, the query KAT): dynamic LDS per workgroup
    size_t wf_tree_lds_bytes = 0;   //   the same for the tree walk where the flat query is the default (the KAT's flag)
    int wf_grid[WK_COUNT] = {};     //   and each kernel's resident workgroups (WK_SEG_RING: with the ring's LDS)
    XShadowLeaves shadow;    // the scene's boundary leaves (gi_capi.cpp fills it from the host scene)
    bool seg_ring = false;   // k_seg refills from its per-wave ring: its LDS does not lower k_seg's resident workgroups
    size_t seg_lds_bytes = 0;//   k_seg's dynamic LDS: wf_lds_bytes, and the ring's bytes with seg_ring
};

// One call of the public ray queries (gi_intersect*, gi_occluded*; gi_wf.hip k_cast): device pointers.
struct CastIO {
    const double* rays;   // n records of 8 doubles (o[3], d[3], tmax, reserved), 16-byte aligned
    long long n;
    double* t;            // closest hit: distance, primitive, entity, facing unit normal (3 per ray);
    int32_t* prim;        //   a null pointer: that output is not written
    int32_t* ent;
    double* nrm;
    int32_t* occl;        // any hit: 1 / 0
};

// One call of the radiance query (gi_radiance*; gi_wf.hip k_rad): device pointers.
struct RadIO {
    const double* rays;     // n records of 8 doubles (o[3], d[3], tmax, reserved), 16-byte aligned
    const uint64_t* ids;    // n gi_path_id records as two words each (stream; sample | reserved << 32), or null
    long long n;            // < 2^32 (the path slot's record index, gi_capi.cpp)
    double* rgb;            // n x 3: the paths' radiance
    V3 light;
    uint64_t seed;
    int depth;
    int no_shadow;          // GI_FLAG_X_NO_SHADOW
};

// One call of the feature buffers (gi_render_aov*; gi_wf.hip k_aov): the window [x0, x0 + cols) x
// [y0, y0 + rows) of the frame and its output planes, device pointers, row-major over the window;
// a null pointer: that plane is not written.
struct AovIO {
    int x0, y0, cols, rows;
    double* t;            // distance from the camera position (+inf: no hit)
    double* nrm;          // facing unit normal (3 per pixel)
    double* alb;          // the hit's texel (3 per pixel)
    int32_t* prim;        // Mode X primitive, entity (-1: no hit)
    int32_t* ent;
    int32_t* uv;          // texture coordinate (2 per pixel)
};

}  // namespace gi
