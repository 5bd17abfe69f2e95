// gi_mode_r.hip — gfx950 (CDNA4) kernels of Mode R, the reference's per-pixel radiance path.
//
// Work decomposition: 8x8 pixel tiles dealt round-robin over shard ranks (tile t belongs to rank
// t % shard_count), so the same kernels serve 1 GPU and N-GPU tile sharding; four waves per
// 256-thread workgroup, one wave64 per tile (lane = pixel).
//
// Mode R (reference semantics):
//   The reference builds the full candidate list of Octree::intersect (octree.h:132-155, DFS over
//   children 0..7, ExpBox node test) and keeps the LAST candidate whose intersect() succeeds
//   (raytracer.h:53-74, A.1).  The kernel reconstructs that answer from the entities the ray's line
//   passes near (a line BVH), their exact tests and the reachability of their leaves (the same
//   node tests on those leaves' root paths only): trace_mode_r_cand.  The reference-order walk --
//   the last hit in DFS order is the first hit in reverse DFS order, children 7..0, leaf lists
//   backwards, first success -- stays available (trace_mode_r, GI_FLAG_R_DFS); both give the same
//   frame bit for bit.  Same primitive math (gi_math.h) as the reference.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (bit-level parity needs no FMA
// contraction; f64 div/sqrt are correctly rounded on gfx950).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>

#include "gi.h"
#include "gi_dev.h"
#include "gi_launch.h"
#include "gi_scene.h"

namespace gi {

namespace {

// ---------------------------------------------------------------------------------------------
// Mode R device pieces
// ---------------------------------------------------------------------------------------------
// TRI: every entity of the scene is an ImpTriangle (DevScene::r_tri_only; the other kinds' code and
// registers drop out of the Mode R kernels)
template <bool TRI = false>
__device__ bool ent_hit(const DevScene& sc, const REnt& e, V3 o, V3 d, V3& P, V3& N, uint32_t& nprim) {
    if (TRI) {
        ++nprim;
        return tri_hit(sc.tris[e.tri_first], o, d, P, N);
    }
    if (e.kind == K_IMP_SPHERE) {
        ++nprim;
        return sphere_hit(ld3(e.pos), e.radius, o, d, P, N);
    }
    if (e.kind == K_IMP_TRIANGLE) {
        ++nprim;
        return tri_hit(sc.tris[e.tri_first], o, d, P, N);
    }
    if (e.kind == K_EXP_RECTANGLE) {   // entities.h:326-336: t1, else t2
        nprim += 1;
        if (tri_hit(sc.tris[e.tri_first], o, d, P, N)) return true;
        nprim += 1;
        return tri_hit(sc.tris[e.tri_first + 1], o, d, P, N);
    }
    if (e.kind == K_EXP_BOX) {   // entities.h:415-440: every face; the LAST hitting face's point wins
        bool any = false;
        for (int f = 0; f < 6; ++f) {
            V3 p, n;
            ++nprim;
            bool h = tri_hit(sc.tris[e.tri_first + 2 * f], o, d, p, n);
            if (!h) {
                ++nprim;
                h = tri_hit(sc.tris[e.tri_first + 2 * f + 1], o, d, p, n);
            }
            if (h) {
                if (sq3(p - o) < DBL_MAX) { P = p; N = n; }
                any = true;
            }
        }
        return any;
    }
    // ExpQuad / ExpSphere / ExpCube / ExpCone ::intersect (entities.h:596-620, 514-536, 736-760,
    // 906-930): nearest by <= over the triangles (ties -> later); outputs overwritten on a miss
    bool flag = false;
    double md = DBL_MAX;
    V3 mi = v3(DBL_MAX, DBL_MAX, DBL_MAX), cn = v3(0, 0, 0);
    for (int t = 0; t < e.tri_count; ++t) {
        V3 p, n;
        ++nprim;
        if (tri_hit(sc.tris[e.tri_first + t], o, d, p, n)) {
            const double dd = sq3(p - o);
            if (dd <= md) { mi = p; cn = n; md = dd; }
            flag = true;
        }
    }
    P = mi;
    N = cn;
    return flag;
}

// getTextureCoord (entities.h:108-130, 277-303, 630-641) with the device's f64 acos/sin/cos
template <bool TRI = false>
__device__ void tex_coord(const DevScene& sc, const REnt& e, V3 ip, int32_t& x, int32_t& y) {
    if (!TRI && e.kind == K_IMP_SPHERE) {
        const double r = e.radius;
        const double unit_v = 2.0 * REF_PI * r / 320.0;
        const V3 to = ip - ld3(e.pos);
        const double cos_vert = dot(to, v3(0, 0, r)) / (r * r);
        const double ang = acos(cos_vert);
        y = x86_trunc((r * ang) / unit_v);
        const double small_r = r * sin(ang);
        const double cos_hori = dot(v3(to.x, to.y, 0), v3(0, small_r, 0)) / (small_r * small_r);
        const double unit_h = 2.0 * REF_PI * small_r / 320.0;
        x = x86_trunc(small_r * acos(cos_hori) / unit_h);
    } else if (TRI || e.kind == K_IMP_TRIANGLE) {   // per-triangle constants precomputed by the builder
        const V3 p1 = ld3(e.qv0), p21 = ld3(e.qv1), i1 = ip - p1;
        const double i1l = gsqrt(sq3(i1));
        const double theta = acos(dot(p21, i1) / (e.qv2[0] * i1l));
        const double ixl = i1l * sin(theta);
        y = x86_trunc(i1l / e.qv2[2]);
        x = x86_trunc(ixl / e.qv2[1]);
    } else if (e.kind == K_EXP_QUAD) {
        const double uv = (double)e.width / 160.0, uh = (double)e.length / 160.0;
        const V3 rv = ld3(e.qv0) - ld3(e.qv1);
        const V3 i1 = ip - ld3(e.qv1);
        const double i1l = gsqrt(sq3(i1));
        const double theta = acos(dot(i1, rv) / ((double)e.width * i1l));
        y = x86_trunc(i1l * sin(theta) / uh);
        x = x86_trunc(i1l * cos(theta) / uv);
    } else if (e.kind == K_EXP_SPHERE) {   // entities.h:549-571 (latitude measured from the equator)
        const double r = e.radius;
        const double unit_v = 2.0 * REF_PI * r / 320.0;
        const V3 to = ip - ld3(e.pos);
        const double ang = acos(dot(to, v3(0, 0, r)) / (r * r));
        y = x86_trunc((0.5 * REF_PI * r - r * ang) / unit_v);
        const double small_r = r * sin(ang);
        const double cos_hori = dot(v3(to.x, to.y, 0), v3(0, small_r, 0)) / (small_r * small_r);
        const double unit_h = 2.0 * REF_PI * small_r / 320.0;
        x = x86_trunc(small_r * acos(cos_hori) / unit_h);
    } else if (e.kind == K_EXP_CUBE) {     // entities.h:769-811
        const double uv = (double)e.width / 160.0, uh = (double)e.length / 160.0;
        const V3 i1 = ip - ld3(e.qv0);
        const double l = gsqrt(sq3(i1));
        const double theta = acos(dot(i1, v3(0, (double)e.width, 0)) / ((double)e.width * l));
        y = x86_trunc(l * sin(theta) / uh);
        x = x86_trunc(l * cos(theta) / uv);
    } else if (e.kind == K_EXP_CONE) {     // entities.h:942-961
        const double R = e.radius, H = e.height;
        const double unit_h = gsqrt(R * R + H * H) / 320.0;
        const V3 pos = ld3(e.pos);
        const double ylen = gsqrt(sq3(ip - pos));
        y = x86_trunc(ylen / unit_h);
        const V3 center = v3((float)pos.x, (float)pos.y, (float)ip.z);   // glm::vec3
        const double rp = ylen * e.sin_theta;
        const V3 left = v3(0, (float)rp, 0);                              // glm::vec3
        const V3 ic = ip - center;
        const double unit_v = 2.0 * REF_PI * rp / 320.0;
        double alpha = acos(dot(ic, left) / (rp * rp));
        if (alpha > REF_PI / 4.0) alpha = acos(dot(ic, -left) / (rp * rp));
        x = x86_trunc(rp * alpha / unit_v);
    } else if (e.kind == K_EXP_RECTANGLE) {   // entities.h:346-365 (acos of an angle, as written)
        const V3 p1 = ld3(e.qv0), p31 = ld3(e.qv1) - p1, p41 = ld3(e.qv2) - p1;
        const double width = gsqrt(sq3(p41)), length = gsqrt(sq3(p31));
        const V3 i1 = ip - p1;
        const double l = gsqrt(sq3(i1));
        const double ct = acos(dot(i1, p31) / (length * l));
        x = x86_trunc(l * sin(acos(ct)) / (length / 64.0));
        y = x86_trunc(l * ct / (width / 64.0));
    } else {   // ExpBox: (0, 0) (entities.h:448-451)
        x = 0;
        y = 0;
    }
}

// Material::blinn_phong_texture (material.h:48-62)
__device__ V3 shade_ref(const REnt& e, V3 dir, V3 light, V3 ip, V3 n, int32_t u, int32_t v) {
    const V3 tc = texel(ld3(e.color), u, v);
    const V3 tdc = tc * 0.5;
    const V3 la = tc * e.shader[0];
    const V3 ld = (smax(0.0, dot(n, normalize(light - ip))) * tdc) * e.shader[1];
    const V3 bis = normalize(normalize(-dir) + normalize(light - ip));
    const double p = pow(smax(0.0, dot(n, bis)), e.spec_pow);
    const V3 ls = (p * v3(1, 1, 1)) * e.shader[2];
    const V3 out = (la + ld) + ls;
    return v3(smin(out.x, 1.0), smin(out.y, 1.0), smin(out.z, 1.0));
}

struct RResult {
    int32_t ent;
    V3 P, N;
};

// scan one leaf list backwards; true when the last hitting candidate of this leaf is found
__device__ bool scan_leaf_rev(const DevScene& sc, const RNode& nd, V3 o, V3 d, RResult& r, uint32_t& nprim) {
    for (int k = nd.ent_cnt - 1; k >= 0; --k) {
        const int32_t e = sc.leaf_ents[nd.ent_off + k];
        V3 P, N;
        if (ent_hit(sc, sc.ents[e], o, d, P, N, nprim)) {
            if (sq3(P - o) < DBL_MAX) {   // raytracer.h:63-65 with min_dist_square == DBL_MAX
                r.ent = e;
                r.P = P;
                r.N = N;
                return true;
            }
        }
    }
    return false;
}

// Last hitting candidate of Octree::intersect's list = first hit of the reverse DFS.
__device__ void trace_mode_r(const DevScene& sc, V3 o, V3 d, RResult& r, uint32_t& nnode, uint32_t& nprim) {
    r.ent = -1;
    const RNode* nodes = sc.rnodes;
    const RNode root = nodes[0];
    if (root.child0 < 0) {
        scan_leaf_rev(sc, root, o, d, r, nprim);
        return;
    }
    int parent = 0, parent_child0 = root.child0, slot = 7;
    for (;;) {
        if (slot < 0) {
            if (parent == 0) return;
            const int pp = nodes[parent].parent;
            const int pc0 = nodes[pp].child0;
            slot = parent - pc0 - 1;
            parent = pp;
            parent_child0 = pc0;
            continue;
        }
        const int c = parent_child0 + slot;
        const RNode nd = nodes[c];
        if (nd.ent_cnt == 0) { --slot; continue; }   // octree.h:140
        ++nnode;
        if (!box_hit(ld3(nd.mn), ld3(nd.mx), o, d)) { --slot; continue; }
        if (nd.child0 < 0) {
            if (scan_leaf_rev(sc, nd, o, d, r, nprim)) return;
            --slot;
            continue;
        }
        parent = c;
        parent_child0 = nd.child0;
        slot = 7;
    }
}

// ---------------------------------------------------------------------------------------------
// Mode R, candidate reconstruction (gi_bvh.cpp build_rcand).  The reference keeps the LAST hitting
// candidate of Octree::intersect's list; a candidate's list position is (its leaf's rank in the
// static DFS order, its index in the leaf's list), and a leaf is in the list iff every node of its
// root path is non-empty and passes the exact ExpBox node test.  So: collect the entities whose
// boxes the ray's LINE crosses (no t > 0 in the reference's tests, A.2/A.3) from a line BVH, test
// each exactly (ent_hit), and keep the hitting entity whose latest reachable appearance is latest
// (reachability = the same node tests, on that leaf's path only).  Same answer as the reference's
// full DFS, with node tests only on the paths of hitting entities.
// ---------------------------------------------------------------------------------------------
// the 8 children of a line-BVH node against the whole line o + t d (t real), boxes widened by tau
__device__ __forceinline__ uint32_t children_mask_line(const XWNode* nd, F3 of, F3 ivf, float tau) {
    const float4* b = reinterpret_cast<const float4*>(nd);
    // near / far planes by the sign of the (clamped) reciprocal, as in the Mode X node tests: the
    // distance ((b -+ tau) - o) * iv is monotone in b, so no per-child min / max; the planes' quads
    // are addressed directly (lo of axis a at quad 2a, hi at 6 + 2a)
    const int sm = iv_signs(ivf);
    const int ex = nd->exists;
    float4 q[12];   // near[3][8] then far[3][8]
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const int nq = ((sm >> a) & 1) ? 6 + 2 * a : 2 * a, fq = ((sm >> a) & 1) ? 2 * a : 6 + 2 * a;
        q[2 * a] = b[nq];
        q[2 * a + 1] = b[nq + 1];
        q[6 + 2 * a] = b[fq];
        q[6 + 2 * a + 1] = b[fq + 1];
    }
    const float* v = reinterpret_cast<const float*>(q);
    const float sx = (sm & 1) ? tau : -tau, sy = (sm & 2) ? tau : -tau, sz = (sm & 4) ? tau : -tau;
    uint32_t m = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const float tn = fmaxf(fmaxf(((v[c] + sx) - of.x) * ivf.x, ((v[8 + c] + sy) - of.y) * ivf.y),
                               ((v[16 + c] + sz) - of.z) * ivf.z);
        const float tf = fminf(fminf(((v[24 + c] - sx) - of.x) * ivf.x, ((v[32 + c] - sy) - of.y) * ivf.y),
                               ((v[40 + c] - sz) - of.z) * ivf.z);
        m |= (uint32_t)((tn <= tf) & ((ex >> c) & 1)) << c;
    }
    return m;
}

// The same 8 tests spread over the NSUB (>= 8) lanes of a pixel group that walk one line
// (k_mode_r_batch's top two levels): lane sub tests child sub & 7 only -- its six bounds are one float
// each, and the group's 8 lanes read 8 consecutive floats of each plane array -- and a ballot gathers
// the mask, the same in every lane.  Per child the arithmetic is children_mask_line's, so the mask is
// identical.
template <int NSUB>
__device__ __forceinline__ uint32_t children_mask_line_coop(const XWNode* nd, F3 of, F3 ivf, float tau, int sub) {
    const int c = sub & 7;
    const int sm = iv_signs(ivf);
    const float nx = (sm & 1) ? nd->hi[0][c] : nd->lo[0][c], fx = (sm & 1) ? nd->lo[0][c] : nd->hi[0][c];
    const float ny = (sm & 2) ? nd->hi[1][c] : nd->lo[1][c], fy = (sm & 2) ? nd->lo[1][c] : nd->hi[1][c];
    const float nz = (sm & 4) ? nd->hi[2][c] : nd->lo[2][c], fz = (sm & 4) ? nd->lo[2][c] : nd->hi[2][c];
    const float sx = (sm & 1) ? tau : -tau, sy = (sm & 2) ? tau : -tau, sz = (sm & 4) ? tau : -tau;
    const float tn = fmaxf(fmaxf(((nx + sx) - of.x) * ivf.x, ((ny + sy) - of.y) * ivf.y), ((nz + sz) - of.z) * ivf.z);
    const float tf = fminf(fminf(((fx - sx) - of.x) * ivf.x, ((fy - sy) - of.y) * ivf.y), ((fz - sz) - of.z) * ivf.z);
    const bool hit = (tn <= tf) & ((nd->exists >> c) & 1);
    const unsigned long long b = __ballot(hit);
    const int base = (int)(threadIdx.x & 63) & ~(NSUB - 1);
    return (uint32_t)((b >> base) & 0xFFull);
}

// Per-ray memo of node-test results (k_mode_r_batch, k_rf_reach): the candidates' root paths share their upper
// levels -- every path starts at the root -- and an exact ExpBox node test is ~12 fp32/fp64 triangle
// solves, so a ray that walks many appearances' paths would repeat the same tests.  Direct-mapped,
// RMEMO entries per ray in LDS, shared by the NSUB lanes of the pixel (one ray, so a result found
// by any of them holds for all); an entry is (node << 1) | passed, -1 when empty.  A lost or stale
// slot only costs a recomputation: the answer never depends on the memo.
#ifndef GI_R_MEMO
#define GI_R_MEMO 64   // entries per ray (power of two); 0 disables the memo
#endif
struct RMemo {
    int* e;        // GI_R_MEMO entries of this ray, or nullptr
    int tag = 0;   // k_rf_reach: (the lane's run of equal tiles in its chunk) << 1 -- a row serves the same
                   // pixel slot of the chunk's tiles, and the memo is cleared at every chunk
};
__device__ __forceinline__ int r_memo_slot(int node) { return (int)(((unsigned)node * 2654435761u) >> 26) & (GI_R_MEMO - 1); }

// is the leaf whose root path is rpath_rec[p0 .. p1) in the ray's candidate list?  (octree.h:139-150
// on that path, top-down: every node non-empty and hit by the exact ExpBox test.)  The path's node
// records are consecutive, so the next one is loaded before the current one's test -- the walk waits
// on one load round trip per path, not two per node (rpath[i], then rnodes[rpath[i]]).
struct RPathR {
    union {
        int4 q[4];
        RPathRec r;
    };
};
__device__ __forceinline__ RPathR load_rpath(const RPathRec* p) {
    const int4* s = reinterpret_cast<const int4*>(p);
    RPathR r;
#pragma unroll
    for (int i = 0; i < 4; ++i) r.q[i] = s[i];
    return r;
}
// G > 1 (k_rf_reach's lane groups): G consecutive lanes hold the same ray and walk the same path in
// step; each tests its part of the 12 ExpBox faces (box_hit_part) and a ballot ORs the group's parts,
// so every decision below is the group's and its lanes never diverge.  Needs the group's lanes active.
template <int G>
__device__ __forceinline__ bool r_box_test(V3 mn, V3 mx, V3 o, V3 d) {
    if constexpr (G == 1) {
        return box_hit(mn, mx, o, d);
    } else {
        static_assert(G == 4, "box_hit_part splits the faces over 4 lanes");
        const int lane = (int)(threadIdx.x & 63);
        const unsigned long long b = __ballot(box_hit_part(mn, mx, o, d, lane & 3));
        return ((b >> (lane & ~3)) & 0xFull) != 0;
    }
}
template <int G = 1>
__device__ __forceinline__ bool r_path_reachable(const DevScene& sc, int p0, int p1, V3 o, V3 d, uint32_t& nnode,
                                                 RMemo memo = RMemo{nullptr}) {
    if (p0 >= p1) return true;
    RPathR cur = load_rpath(sc.rpath_rec + p0);
    for (int i = p0; i < p1; ++i) {
        const RPathR nd = cur;
        if (i + 1 < p1) cur = load_rpath(sc.rpath_rec + i + 1);
        if (nd.r.ent_cnt == 0) return false;   // octree.h:140
        const int ni = nd.r.node;
        if (GI_R_MEMO > 0 && memo.e) {
            int* slot = memo.e + r_memo_slot(ni);
            const int m = *slot;   // (a group's lanes read it in one instruction: the same value)
            const int key = (ni << 9) | memo.tag;   // (the scenes using a memo have < 2^22 nodes)
            if ((m & ~1) == key) {
                if (!(m & 1)) return false;
                continue;
            }
            ++nnode;
            const bool ok = r_box_test<G>(ld3(nd.r.mn), ld3(nd.r.mx), o, d);
            *slot = key | (ok ? 1 : 0);
            if (!ok) return false;
            continue;
        }
        ++nnode;
        if (!r_box_test<G>(ld3(nd.r.mn), ld3(nd.r.mx), o, d)) return false;
    }
    return true;
}

// entity e as a candidate: exact test, then its latest reachable appearance against the best so far
template <bool TRI = false>
__device__ __forceinline__ void r_consider(const DevScene& sc, int e, V3 o, V3 d, long long& best, RResult& r,
                                           uint32_t& nnode, uint32_t& nprim, RMemo memo = RMemo{nullptr}) {
    const int a0 = sc.app_off[e], a1 = sc.app_off[e + 1];
    if (a0 == a1 || sc.app_rec[a0].rank <= best) return;
    V3 P, N;
    if (!ent_hit<TRI>(sc, sc.ents[e], o, d, P, N, nprim) || !(sq3(P - o) < DBL_MAX)) return;   // raytracer.h:58-65
    for (int i = a0; i < a1; ++i) {
        const RApp ap = sc.app_rec[i];
        const long long rk = ap.rank;
        if (rk <= best) return;
        if (r_path_reachable(sc, ap.p0, ap.p1, o, d, nnode, memo)) {
            best = rk;
            r.ent = e;
            r.P = P;
            r.N = N;
            return;
        }
    }
}

__device__ __forceinline__ void trace_mode_r_cand(const DevScene& sc, V3 o, V3 d, float tau, RResult& r, uint32_t& nnode,
                                  uint32_t& nprim) {
    r.ent = -1;
    long long best = -1;
    for (int i = 0; i < sc.n_r_always; ++i) r_consider(sc, sc.r_always[i], o, d, best, r, nnode, nprim);
    const XWNode* W = sc.rc_nodes;
    const F3 of = f3((float)o.x, (float)o.y, (float)o.z);
    const F3 ivf = inv_dir(d);   // clamped to +-1e30: finite plane distances, near / far by sign
    uint64_t mlo = 0, mhi = 0;
    int node = 0, level = 0;
    const uint32_t rm = children_mask_line(W, of, ivf, tau);
    lvl_set(mlo, mhi, 0, rm);
    bool going = rm != 0;
    while (going) {   // stackless: 8-bit "children left" mask per level, parent pointers
        const uint32_t msk = lvl_get(mlo, mhi, level);
        const int c = __builtin_ctz(msk);
        lvl_set(mlo, mhi, level, msk & (msk - 1));
        const XWNode* nd = W + node;
        const int ch = nd->child[c];
        if (sc.rc_maxkey[node * 8 + c] <= best) {   // rank order: no better candidate here or after
            lvl_set(mlo, mhi, level, 0);
        } else if (ch < 0) {
            const int cnt = nd->cnt[c];
            for (int j = 0; j < cnt; ++j) r_consider(sc, sc.rc_ent[~ch + j], o, d, best, r, nnode, nprim);
        } else {
            const uint32_t cm = children_mask_line(W + ch, of, ivf, tau);
            if (cm) {
                node = ch;
                ++level;
                lvl_set(mlo, mhi, level, cm);
            }
        }
        uint32_t rest = lvl_get(mlo, mhi, level);
        while (rest == 0 && level > 0) {
            --level;
            node = level == 0 ? 0 : W[node].parent;
            rest = lvl_get(mlo, mhi, level);
        }
        going = rest != 0;
    }
}

// Mode R for large scenes (more than 4096 entities).  A one-lane-per-pixel walk (k_mode_r) spends
// the 100k soup's frame on a few pixels' serial work -- their lines cross ~100 entity boxes -- so
// these scenes run the flat phases below (k_rf_*), chip-wide and dense, and k_mode_r_batch renders
// the tiles whose candidates do not fit the flat phases' buffers.  Both answer as trace_mode_r_cand:
// the hitting candidate of highest reachable list rank (A.1), bit for bit.

// maximum over the NSUB lanes of a pixel group
template <int NSUB>
__device__ __forceinline__ long long group_max(long long v) {
#pragma unroll
    for (int off = 1; off < NSUB; off <<= 1) {
        const long long u = __shfl_xor(v, off);
        v = u > v ? u : v;
    }
    return v;
}

// the pixel from a group's candidates: the lowest sub-lane holding the group's highest rank (ranks are
// unique: one lane at most) shades it; none: black
template <int NSUB, bool TRI>
__device__ __forceinline__ void r_group_write(const DevScene& sc, V3 d, V3 light, const RResult& r, long long mine,
                                              int sub, long long idx, double* rgb, uint8_t* rgb8) {
    const long long gmax = group_max<NSUB>(mine);
    const unsigned long long m_win = __ballot(mine == gmax);
    const int base = (int)(threadIdx.x & 63) & ~(NSUB - 1);
    const unsigned long long gm = NSUB >= 64 ? ~0ull : ((1ull << (NSUB & 63)) - 1);
    const bool writer = gmax < 0 ? sub == 0 : (int)(threadIdx.x & 63) == base + __builtin_ctzll((m_win >> base) & gm);
    if (writer) {
        double c0 = 0, c1 = 0, c2 = 0;
        if (gmax >= 0) {
            const REnt& e = sc.ents[r.ent];
            int32_t u, v;
            tex_coord<TRI>(sc, e, r.P, u, v);
            const V3 col = shade_ref(e, d, light, r.P, r.N, u, v);
            c0 = col.x; c1 = col.y; c2 = col.z;
        }
        if (rgb) { rgb[3 * idx] = c0; rgb[3 * idx + 1] = c1; rgb[3 * idx + 2] = c2; }
        if (rgb8) quantize(c0, c1, c2, rgb8 + 3 * idx);
    }
}

// a candidate considered by one lane of the group: on a better reachable hit, the group's best rank
// (LDS, atomic max) is raised
template <bool TRI>
__device__ __forceinline__ void r_group_consider(const DevScene& sc, int e, V3 o, V3 d, unsigned long long* gb, long long& best,
                                                 long long& mine, RResult& r, uint32_t& nnode, uint32_t& nprim, RMemo memo) {
    const long long before = best;
    r_consider<TRI>(sc, e, o, d, best, r, nnode, nprim, memo);
    if (best != before) {
        mine = best;
        atomicMax(gb, (unsigned long long)(best + 1));
    }
}
// the items of a pixel's walk: the root's hit slots, an interior one replaced by its own hit slots
// (cooperative node tests), in rank order -- (node << 3) | slot, at most 64; written by sub-lane 0
template <int NSUB>
__device__ __forceinline__ int r_items(const XWNode* W, F3 of, F3 ivf, float tau, int sub, int* items) {
    int n = 0;
    uint32_t rm = children_mask_line_coop<NSUB>(W, of, ivf, tau, sub);
    while (rm) {
        const int c = __builtin_ctz(rm);
        rm &= rm - 1;
        const int ch = W[0].child[c];
        if (ch < 0) {
            if (sub == 0) items[n] = c;
            ++n;
        } else {
            uint32_t cm = children_mask_line_coop<NSUB>(W + ch, of, ivf, tau, sub);
            while (cm) {
                const int c2 = __builtin_ctz(cm);
                cm &= cm - 1;
                if (sub == 0) items[n] = (ch << 3) | c2;
                ++n;
            }
        }
    }
    __builtin_amdgcn_wave_barrier();
    return n;
}

// Mode R in rounds, 8 lanes per pixel (k_mode_r_batch; the flat phases' fallback).  The group walks
// the line BVH's top two levels together into <= 64 items in rank order; every lane then alternates a
// walk phase of at most GI_R_BATCH_STEPS node steps over the items it takes from the group's LDS
// counter, which only queues the entities of the leaves it meets (those whose highest rank beats the
// group's best) in the lane's LDS segment, and a test phase in which the pixel's 8 lanes share the
// group's queued candidates (compacted, candidate j by lane j mod 8) -- the exact tests of a wave's 8
// pixels in one dense block.  Pruning only skips slots whose bound is <= a rank found, and every
// candidate is considered by one lane, so the answer is the highest reachable hitting rank.
// Work items are 32 pixel slots (one per 8-lane group of the workgroup): the whole frame
// (tiles == nullptr) or both halves of each of the *n_tiles listed tiles.
#ifndef GI_R_BATCH_STEPS
#define GI_R_BATCH_STEPS 16   // node steps a lane's walk takes per round (R-C4: 2 4.04, 4 3.56, 8 3.41,
                             // 16 3.19, 32 3.33 ms)
#endif
#ifndef GI_R_BATCH_SEG
#define GI_R_BATCH_SEG 8     // candidates a lane queues per round (4 and 16: equal or slower)
#endif
template <bool STATS, bool TRI>
__global__ __launch_bounds__(256) void k_mode_r_batch(DevScene sc, CamDev cam, V3 light, TileMap m, double* rgb,
                                                      uint8_t* rgb8, unsigned long long* stats, float tau,
                                                      const unsigned* tiles, const unsigned* n_tiles) {
    constexpr int NSUB = 8, SEG = GI_R_BATCH_SEG;   // lanes per pixel; queued candidates per lane and round
    const int sub = (int)(threadIdx.x % NSUB), grp = threadIdx.x / NSUB;
    __shared__ int s_memo[GI_R_MEMO > 0 ? (256 / NSUB) * GI_R_MEMO : 1];
    __shared__ unsigned long long s_best[256 / NSUB];   // the group's best rank + 1 (0: none)
    __shared__ int s_item[256 / NSUB][64];              // (node << 3) | slot, in rank order
    __shared__ unsigned s_next[256 / NSUB];             // the group's next item
    __shared__ int s_seg[256 / NSUB][NSUB * SEG];       // each lane's queued candidates (SEG slots)
    __shared__ int s_cand[256 / NSUB][NSUB * SEG];      // the group's candidates of the round, compacted
    // (memo keys are node << 9: scenes of 2^22 nodes or more run without the memo)
    RMemo memo{(GI_R_MEMO > 0 && sc.n_rnodes < (1 << 22)) ? s_memo + grp * GI_R_MEMO : nullptr};
    const long long n_items = tiles ? 2ll * (long long)*n_tiles : (m.n_local * (kTile * kTile) + 31) / 32;
    uint32_t nnode = 0, nprim = 0, npx = 0;
    for (long long item = blockIdx.x; item < n_items; item += gridDim.x) {   // uniform over the workgroup
        const long long ps = (tiles ? (long long)tiles[item >> 1] * 64 + (item & 1) * 32 : item * 32) + grp;
        if (memo.e)
            for (int k = sub; k < GI_R_MEMO; k += NSUB) memo.e[k] = -1;
        if (sub == 0) {
            s_best[grp] = 0ull;
            s_next[grp] = 0u;
        }
        __builtin_amdgcn_wave_barrier();
        const long long lt = ps >> 6;
        long long idx = -1;
        int x = 0, y = 0;
        const bool ok = lt < m.n_local && slot_pixel(m, lt, (int)(ps & 63), idx, x, y);
        y += m.y0;
        if (ok) {
            if (sub == 0) ++npx;
            const V3 o = cam.pos;
            const V3 d = normalize(primary_dir(cam, (double)x, (double)y));
            unsigned long long* gb = s_best + grp;
            RResult r;
            r.ent = -1;
            long long best = -1, mine = -1;
            for (int i = sub; i < sc.n_r_always; i += NSUB) r_group_consider<TRI>(sc, sc.r_always[i], o, d, gb, best, mine, r, nnode, nprim, memo);
            const XWNode* W = sc.rc_nodes;
            const F3 of = f3((float)o.x, (float)o.y, (float)o.z);
            const F3 ivf = inv_dir(d);
            const int n = r_items<NSUB>(W, of, ivf, tau, sub, s_item[grp]);
            int* seg = s_seg[grp] + sub * SEG;
            int* cand = s_cand[grp];
            // the lane's walk: (root, node, level, masks) while walking; a leaf's entities [pcur, pend)
            // still to queue; done once the group's items are all taken
            bool walking = false, done = false;
            int root = 0, node = 0, level = 0, pcur = 0, pend = 0;
            uint64_t mlo = 0, mhi = 0;
            for (;;) {
                // ---- walk phase: queue up to SEG candidates within GI_R_BATCH_STEPS node steps
                int nq = 0, steps = 0;
                while (nq < SEG) {
                    best = max(best, (long long)*(volatile unsigned long long*)gb - 1);
                    if (pcur < pend) {   // the current leaf's entities: those that can still win
                        const int e = sc.rc_ent[pcur++];
                        const int a0 = sc.app_off[e];
                        if (a0 != sc.app_off[e + 1] && sc.app_rec[a0].rank > best) seg[nq++] = e;
                        continue;
                    }
                    if (steps >= GI_R_BATCH_STEPS || done) break;
                    ++steps;
                    if (!walking) {      // the group's next item
                        const int i = (int)atomicAdd(s_next + grp, 1u);
                        if (i >= n) {
                            done = true;
                            break;
                        }
                        const int it = s_item[grp][i];
                        const int in = it >> 3, ic = it & 7;
                        if (sc.rc_maxkey[in * 8 + ic] <= best) continue;
                        const int ch = W[in].child[ic];
                        if (ch < 0) {
                            pcur = ~ch;
                            pend = ~ch + W[in].cnt[ic];
                        } else {
                            ++nnode;
                            const uint32_t cm = children_mask_line(W + ch, of, ivf, tau);
                            if (cm) {
                                root = node = ch;
                                level = 0;
                                mlo = mhi = 0;
                                lvl_set(mlo, mhi, 0, cm);
                                walking = true;
                            }
                        }
                        continue;
                    }
                    // one step of the item's subtree walk (stackless, rank order)
                    const uint32_t msk = lvl_get(mlo, mhi, level);
                    const int c = __builtin_ctz(msk);
                    lvl_set(mlo, mhi, level, msk & (msk - 1));
                    const XWNode* nd = W + node;
                    const int ch = nd->child[c];
                    if (sc.rc_maxkey[node * 8 + c] <= best) {
                        lvl_set(mlo, mhi, level, 0);
                    } else if (ch < 0) {
                        pcur = ~ch;
                        pend = ~ch + nd->cnt[c];
                    } else {
                        ++nnode;
                        const uint32_t cm = children_mask_line(W + ch, of, ivf, tau);
                        if (cm) {
                            node = ch;
                            ++level;
                            lvl_set(mlo, mhi, level, cm);
                        }
                    }
                    uint32_t rest = lvl_get(mlo, mhi, level);
                    while (rest == 0 && level > 0) {
                        --level;
                        node = level == 0 ? root : W[node].parent;
                        rest = lvl_get(mlo, mhi, level);
                    }
                    walking = rest != 0;
                }
                // ---- the group's queue, compacted (inclusive prefix of the lanes' counts)
                int incl = nq;
#pragma unroll
                for (int off = 1; off < NSUB; off <<= 1) {
                    const int t = __shfl_up(incl, off, NSUB);
                    if (sub >= off) incl += t;
                }
                const int total = __shfl(incl, NSUB - 1, NSUB);
                for (int k = 0; k < nq; ++k) cand[incl - nq + k] = seg[k];
                __builtin_amdgcn_wave_barrier();
                // ---- test phase: candidate j by lane j mod 8
                for (int j = sub; j < total; j += NSUB) {
                    best = max(best, (long long)*(volatile unsigned long long*)gb - 1);
                    r_group_consider<TRI>(sc, cand[j], o, d, gb, best, mine, r, nnode, nprim, memo);
                }
                __builtin_amdgcn_wave_barrier();
                // the wave leaves the loop once none of its lanes has anything left (groups stay in step)
                if (__ballot(!(done && !walking && pcur >= pend)) == 0) break;
            }
            r_group_write<NSUB, TRI>(sc, d, light, r, mine, sub, idx, rgb, rgb8);
        } else if (sub == 0 && idx >= 0 && m.shard_count > 1) {   // padding slot of a packed tile
            if (rgb) { rgb[3 * idx] = 0; rgb[3 * idx + 1] = 0; rgb[3 * idx + 2] = 0; }
            if (rgb8) { rgb8[3 * idx] = 0; rgb8[3 * idx + 1] = 0; rgb8[3 * idx + 2] = 0; }
        }
        __builtin_amdgcn_wave_barrier();   // the group's LDS state is reset for the next item
    }
    if (STATS) wave_add_stats(stats, npx, nnode, nprim, npx);
}

// Flat Mode R (VERDICT r03's chip-wide phases; the default for large scenes).  k_rf_walk: one lane per
// pixel slot walks the whole line BVH (no rank pruning) and stores a (slot, entity) pair for every
// entity of every leaf its line crosses; k_rf_hit: ent_hit over the pairs, the hitting ones kept;
// k_rf_scan + k_rf_reach: per hitting pair, the entity's appearances latest first against the pixel's
// best rank so far (atomic max), the first reachable one raising it; k_rf_shade: per pixel, the
// entity of the best rank (r_leaf_of_rank) tested again for its hit point and normal, shaded.  The
// answer -- the highest reachable hitting rank -- is k_mode_r's.
// Storage, no device-wide append counter (a first version appended every wave's pairs through one:
// the atomics serialised, k_rf_hit waited 95% of its cycles): the walk's wave for tile t owns tile
// t's region -- GI_RF_S0 pairs of its own, then pool pages of GI_RF_PAGE pairs taken with one atomic
// per page run (only tiles with many candidates take any), at most GI_RF_KMAX; rcnt[t] its pairs.  A
// pair is one word, (slot in the tile << 26) | entity.  k_rf_hit compacts a region's hitting pairs in
// place; persistent waves take regions in turn.  A tile that needs more pages than it may take, or
// finds the pool empty, is marked overflowed (rcnt = kRfOvf) and listed; the other phases skip it and
// k_mode_r_batch, launched behind them over that list, renders exactly those tiles.
#ifndef GI_RF_BUF
#define GI_RF_BUF 16   // k_rf_walk: pairs a lane buffers in LDS before the wave flushes
#endif
#define GI_RF_S0 512u     // pairs of a tile's own region (8 per pixel slot)
#define GI_RF_PAGE 512u   // pairs per pool page
#define GI_RF_KMAX 64u    // pool pages a tile may take (so at most 33,280 pairs per tile)
constexpr unsigned kRfOvf = 0xFFFFFFFFu;
constexpr unsigned kRfEntMask = (1u << 26) - 1u;   // scenes of more entities run k_mode_r_batch
struct RFlat {
    unsigned* pairs;            // n_regions x GI_RF_S0: each tile's own region
    unsigned* pool;             // n_pages x GI_RF_PAGE
    unsigned* pt;               // per tile: GI_RF_KMAX pool page ids (those taken)
    unsigned long long* best;   // per pixel slot: best rank + 1
    unsigned* cnt;              // [0] pool pages taken, [1] overflowed tiles
    unsigned* ovf;              // the overflowed tiles (cnt[1] of them)
    unsigned* rcnt;             // per tile: pairs, or kRfOvf
    unsigned* soff;             // per tile: its first segment of GI_RF_SEG pairs (k_rf_scan); [n_regions]: the total
    unsigned* shc;              // per segment: its hitting pairs (compacted to the segment's start)
    unsigned* sreg;             // per segment: its region
    unsigned* hoff;             // per segment: the hits before it (k_rf_scan); [segments]: the total
    double* dir;                // per pixel slot: its primary direction (k_rf_walk writes, the others read)
    unsigned n_pages;
};
__device__ __forceinline__ V3 rf_dir(const RFlat& f, unsigned slot) {
    const double* q = f.dir + 3 * (size_t)slot;
    return v3(q[0], q[1], q[2]);
}
// the page index (0 .. GI_RF_KMAX-1) holding pair i of a region beyond its own GI_RF_S0 (0 below)
__device__ __forceinline__ int rf_page(unsigned i) {
    return i < GI_RF_S0 ? 0 : (int)min((i - GI_RF_S0) / GI_RF_PAGE, GI_RF_KMAX - 1u);
}
// pair i of region r; pg: the id of its pool page (rf_page(i)-th of the region's pages)
__device__ __forceinline__ unsigned* rf_pair(const RFlat& f, long long r, unsigned i, unsigned pg) {
    return i < GI_RF_S0 ? f.pairs + (size_t)r * GI_RF_S0 + i : f.pool + (size_t)pg * GI_RF_PAGE + (i - GI_RF_S0) % GI_RF_PAGE;
}
// lane k: the id of region r's k-th pool page (only regions beyond their own pairs have any)
__device__ __forceinline__ unsigned rf_pages_of(const RFlat& f, long long r, unsigned n, int lane) {
    return (n > GI_RF_S0 && (unsigned)lane < GI_RF_KMAX) ? f.pt[(size_t)r * GI_RF_KMAX + lane] : 0u;
}
// k_rf_walk: a wave per tile walks the line BVH ONCE for all 64 of its pixels' lines.  The lines
// of a tile's pixels lie in the convex cone (apex at the camera) over the tile's 4 corner directions
// -- the primary direction is affine in the pixel coordinates (raytracer.h:41-43) -- so a node box
// that misses both nappes of that cone (a necessary-condition test against its 4 side planes, in
// fp64, the box widened by 2 tau) holds no pixel's candidate.  The wave pops up to 8 nodes per round
// from its LDS stack and tests their 64 children together, one per lane; hit interior children are
// pushed, hit leaf slots are then tested by every lane against its own line with the per-line slab
// test of the per-pixel walk (box_hit_line: children_mask_line's arithmetic), and a passing lane queues the
// slot's entities.  Since a node's box contains its children's, the pairs are exactly those of a
// per-pixel walk; a tile's loads are the same for all its lanes (broadcasts) instead of 64
// divergent walks.  A stack that would exceed GI_RF_STK marks the tile overflowed (k_mode_r_batch).
#define GI_RF_STK 512u   // traversal stack entries per wave (tile)
// one existing child's box (lo xyz, hi xyz) against the line: children_mask_line's arithmetic
__device__ __forceinline__ bool box_hit_line(const float* b, F3 of, F3 ivf, float tau) {
    const int sm = iv_signs(ivf);
    const float nx = (sm & 1) ? b[3] : b[0], fx = (sm & 1) ? b[0] : b[3];
    const float ny = (sm & 2) ? b[4] : b[1], fy = (sm & 2) ? b[1] : b[4];
    const float nz = (sm & 4) ? b[5] : b[2], fz = (sm & 4) ? b[2] : b[5];
    const float sx = (sm & 1) ? tau : -tau, sy = (sm & 2) ? tau : -tau, sz = (sm & 4) ? tau : -tau;
    const float tn = fmaxf(fmaxf(((nx + sx) - of.x) * ivf.x, ((ny + sy) - of.y) * ivf.y), ((nz + sz) - of.z) * ivf.z);
    const float tf = fminf(fminf(((fx - sx) - of.x) * ivf.x, ((fy - sy) - of.y) * ivf.y), ((fz - sz) - of.z) * ivf.z);
    return tn <= tf;
}
// may some line of the tile's double cone (side-plane normals n[4], through the camera c) meet the
// box [lo - wd, hi + wd]?  Forward nappe: every side plane has part of the box on its inner side;
// backward nappe: every side plane has part of it on its outer side.  Conservative (margin eps).
__device__ __forceinline__ bool box_meets_cone(const float* lo, const float* hi, double wd, V3 c, const V3* n) {
    const double l[3] = {(double)lo[0] - wd - c.x, (double)lo[1] - wd - c.y, (double)lo[2] - wd - c.z};
    const double h[3] = {(double)hi[0] + wd - c.x, (double)hi[1] + wd - c.y, (double)hi[2] + wd - c.z};
    const double ext = fmax(fmax(fabs(l[0]), fabs(h[0])), fmax(fmax(fabs(l[1]), fabs(h[1])), fmax(fabs(l[2]), fabs(h[2]))));
    bool fwd = true, bwd = true;
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        const double nn[3] = {n[a].x, n[a].y, n[a].z};
        double mx = 0.0, mn = 0.0, an = 0.0;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const double u = nn[k] * l[k], v = nn[k] * h[k];
            mx += fmax(u, v);
            mn += fmin(u, v);
            an += fabs(nn[k]);
        }
        const double eps = 1e-9 * an * ext;
        fwd = fwd && mx >= -eps;
        bwd = bwd && mn <= eps;
    }
    return fwd || bwd;
}
template <bool STATS>
__global__ __launch_bounds__(256) void k_rf_walk(DevScene sc, CamDev cam, TileMap m, float tau, RFlat f,
                                                 unsigned long long* stats) {
    __shared__ int s_buf[256][GI_RF_BUF];
    __shared__ unsigned s_pt[4][GI_RF_KMAX];   // the wave's pool pages
    __shared__ int s_stk[4][GI_RF_STK];        // the tile's traversal stack (line-BVH nodes)
    __shared__ int s_leaf[4][64];              // a round's hit leaf slots: (node << 3) | slot
    __shared__ float s_lb[4][64][6];           //   their boxes (lo xyz, hi xyz)
    __shared__ int s_le[4][64][6];             //   their first entity, count and first 4 entity ids
    const long long slot = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long region = slot >> 6;
    const int lane = threadIdx.x & 63;
    int* buf = s_buf[threadIdx.x];
    unsigned* pt = s_pt[threadIdx.x >> 6];
    int* stk = s_stk[threadIdx.x >> 6];
    int* leaves = s_leaf[threadIdx.x >> 6];
    float (*lb)[6] = s_lb[threadIdx.x >> 6];
    int (*le)[6] = s_le[threadIdx.x >> 6];
    long long idx = -1;
    int x = 0, y = 0;
    const bool in = slot < m.n_local * 64;
    const bool ok = in && slot_pixel(m, slot >> 6, (int)(slot & 63), idx, x, y);
    if (in) f.best[slot] = 0ull;
    if (__ballot(in) == 0) return;   // (a wave is one tile: all of it beyond the shard's tiles)
    uint32_t nnode = 0;
    const XWNode* W = sc.rc_nodes;
    int nb = 0;
    unsigned fill = 0, npg = 0;   // the wave's pairs and pool pages so far (the same in every lane)
    bool ovf = false;
    const unsigned tag = (unsigned)(slot & 63) << 26;
    const F3 of = f3((float)cam.pos.x, (float)cam.pos.y, (float)cam.pos.z);
    F3 ivf = f3(1, 1, 1);
    if (ok) {
        const V3 d = normalize(primary_dir(cam, (double)x, (double)(y + m.y0)));
        double* qd = f.dir + 3 * slot;
        qd[0] = d.x; qd[1] = d.y; qd[2] = d.z;
        ivf = inv_dir(d);
    }
    // flush the wave's buffers into its region (pool pages taken as needed: one atomic)
    auto flush = [&]() {
        int incl = nb;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const int t = __shfl_up(incl, off);
            if (lane >= off) incl += t;
        }
        const unsigned tot = (unsigned)__shfl(incl, 63);
        const unsigned end = fill + tot;
        const unsigned need = end > GI_RF_S0 ? (end - GI_RF_S0 + GI_RF_PAGE - 1) / GI_RF_PAGE : 0u;
        if (need > npg && !ovf) {
            unsigned b = 0;
            if (lane == 0 && need <= GI_RF_KMAX) b = atomicAdd(f.cnt, need - npg);
            b = __shfl(b, 0);
            if (need > GI_RF_KMAX || b + (need - npg) > f.n_pages) {
                ovf = true;   // (pages taken past the pool's end are simply unused)
            } else {
                if ((unsigned)lane >= npg && (unsigned)lane < need) {
                    pt[lane] = b + (unsigned)lane - npg;
                    f.pt[(size_t)region * GI_RF_KMAX + lane] = b + (unsigned)lane - npg;
                }
                npg = need;
                __builtin_amdgcn_wave_barrier();
            }
        }
        if (!ovf) {
            for (int k = 0; k < nb; ++k) {
                const unsigned j = fill + (unsigned)(incl - nb + k);
                *rf_pair(f, region, j, pt[rf_page(j)]) = (unsigned)buf[k];
            }
        }
        fill = end;
        nb = 0;
    };
    // every ray's ImpSpheres (build_rcand keeps them out of the line BVH)
    for (int k = 0; k < sc.n_r_always; ++k) {
        if (__ballot(nb >= (int)GI_RF_BUF) != 0) flush();
        if (ok) buf[nb++] = (int)(tag | (unsigned)sc.r_always[k]);
    }
    // the tile's cone: corner directions from its pixels' extents (uniform)
    int x0 = ok ? x : INT_MAX, x1 = ok ? x : INT_MIN, y0 = ok ? y : INT_MAX, y1 = ok ? y : INT_MIN;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        x0 = min(x0, __shfl_xor(x0, off));
        x1 = max(x1, __shfl_xor(x1, off));
        y0 = min(y0, __shfl_xor(y0, off));
        y1 = max(y1, __shfl_xor(y1, off));
    }
    int sp = 0;   // stack entries (uniform)
    V3 n[4];
    if (x0 <= x1) {
        const V3 da = primary_dir(cam, (double)x0, (double)(y0 + m.y0)), db = primary_dir(cam, (double)x1, (double)(y0 + m.y0));
        const V3 dc = primary_dir(cam, (double)x1, (double)(y1 + m.y0)), dd = primary_dir(cam, (double)x0, (double)(y1 + m.y0));
        const V3 mid = ((da + db) + (dc + dd)) * 0.25;
        n[0] = cross(da, db);
        n[1] = cross(db, dc);
        n[2] = cross(dc, dd);
        n[3] = cross(dd, da);
#pragma unroll
        for (int a = 0; a < 4; ++a)
            if (dot(n[a], mid) < 0) n[a] = -n[a];
        if (lane == 0) stk[0] = 0;   // the root
        sp = 1;
        __builtin_amdgcn_wave_barrier();
    }
    const double wd = 2.0 * (double)tau;
    const V3 cp = cam.pos;
    while (sp > 0 && !ovf) {
        // ---- up to 8 nodes from the stack, their 64 children one per lane
        const int nt = min(sp, 8);
        const int j = lane >> 3, c = lane & 7;
        int ch = 0;
        bool hit = false;
        if (j < nt) {
            const int nd_i = stk[sp - 1 - j];
            const XWNode* nd = W + nd_i;
            if ((nd->exists >> c) & 1) {
                const float lo[3] = {nd->lo[0][c], nd->lo[1][c], nd->lo[2][c]};
                const float hi[3] = {nd->hi[0][c], nd->hi[1][c], nd->hi[2][c]};
                hit = box_meets_cone(lo, hi, wd, cp, n);
                ch = nd->child[c];
                if (hit && ch < 0) ch = ~((nd_i << 3) | c);   // a leaf slot: (node << 3) | slot, negated
            }
            if (c == 0) ++nnode;
        }
        __builtin_amdgcn_wave_barrier();
        sp -= nt;
        const unsigned long long m_in = __ballot(hit && ch >= 0), m_lf = __ballot(hit && ch < 0);
        const int n_in = __popcll(m_in), n_lf = __popcll(m_lf);
        if ((unsigned)(sp + n_in) > GI_RF_STK) {
            ovf = true;
            break;
        }
        if (hit && ch >= 0) stk[sp + __popcll(m_in & ((1ull << lane) - 1))] = ch;
        if (hit && ch < 0) leaves[__popcll(m_lf & ((1ull << lane) - 1))] = ~ch;
        sp += n_in;
        __builtin_amdgcn_wave_barrier();
        // ---- the round's leaf slots against every lane's own line.  Their records are fetched first,
        // lane j those of slot j, into LDS (one memory round trip for the round instead of one per
        // slot); then every slot is tested by every lane from LDS
        if (lane < n_lf) {
            const int it = leaves[lane];
            const XWNode* nd = W + (it >> 3);
            const int sl = it & 7;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                lb[lane][a] = nd->lo[a][sl];
                lb[lane][3 + a] = nd->hi[a][sl];
            }
            const int e0 = ~nd->child[sl], cnt = nd->cnt[sl];
            le[lane][0] = e0;
            le[lane][1] = cnt;
#pragma unroll
            for (int k = 0; k < 4; ++k) le[lane][2 + k] = k < cnt ? sc.rc_ent[e0 + k] : 0;
        }
        __builtin_amdgcn_wave_barrier();
        for (int i = 0; i < n_lf; ++i) {
            const bool pass = ok && box_hit_line(lb[i], of, ivf, tau);
            const int e0 = le[i][0], cnt = le[i][1];   // (uniform: one leaf for the wave)
            for (int k0 = 0; k0 < cnt; k0 += (int)GI_RF_BUF / 2) {
                const int kk = min(cnt - k0, (int)GI_RF_BUF / 2);
                if (__ballot(nb + kk > (int)GI_RF_BUF) != 0) flush();
                if (pass)
                    for (int k = 0; k < kk; ++k) {
                        const int q = k0 + k;
                        buf[nb++] = (int)(tag | (unsigned)(q < 4 ? le[i][2 + q] : sc.rc_ent[e0 + q]));
                    }
            }
        }
        __builtin_amdgcn_wave_barrier();
    }
    flush();
    if (in && lane == 0) {
        f.rcnt[region] = ovf ? kRfOvf : fill;
        if (ovf) f.ovf[atomicAdd(f.cnt + 1, 1u)] = (unsigned)region;
    }
    if (STATS) {
        wave_add_stats(stats, 0, nnode, 0, 0);
        if (in && lane == 0) {
            atomicAdd(stats + GI_STAT_R_PAIRS, (unsigned long long)fill);
            if (ovf) atomicAdd(stats + GI_STAT_R_OVF_TILES, 1ull);
        }
    }
}
// the last index k in [0, n) with off[k] <= v (off ascending from off[0] = 0)
__device__ __forceinline__ long long rf_find(const unsigned* off, long long n, long long v) {
    long long lo = 0, hi = n - 1;
    while (lo < hi) {
        const long long mid = (lo + hi + 1) >> 1;
        if ((long long)off[mid] <= v) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
// The pairs' exact entity tests, per segment of GI_RF_SEG pairs of a region (k_rf_scan numbers them),
// its hitting pairs compacted to the segment's start.  Persistent waves take segments in turn, so the
// thousands of pairs of a soup-core tile are tested by many waves at once, not by one in sequence.
#ifndef GI_RF_SEG
#define GI_RF_SEG 512u   // pairs per segment (8 chunks of 64)
#endif
template <bool STATS, bool TRI>
__global__ __launch_bounds__(64) void k_rf_hit(DevScene sc, CamDev cam, TileMap m, RFlat f, unsigned long long* stats) {
    const int lane = threadIdx.x & 63;
    const long long n_regions = m.n_local;
    const long long gw = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_w = ((long long)gridDim.x * blockDim.x) >> 6;
    const long long n_seg = f.soff[n_regions];
    uint32_t nprim = 0;
    long long cur = -1;
    unsigned pg = 0, n = 0;
    for (long long sg = gw; sg < n_seg; sg += n_w) {
        const long long r = rf_find(f.soff, n_regions, sg);
        if (r != cur) {
            n = f.rcnt[r];   // (overflowed tiles have no segment)
            pg = rf_pages_of(f, r, n, lane);
            cur = r;
        }
        const unsigned p0 = (unsigned)(sg - (long long)f.soff[r]) * GI_RF_SEG, p1 = min(n, p0 + GI_RF_SEG);
        unsigned kept = 0;
        for (unsigned i0 = p0; i0 < p1; i0 += 64) {
            const unsigned i = i0 + lane;
            const unsigned pin = __shfl(pg, rf_page(i));
            bool hit = false;
            unsigned pr = 0;
            if (i < p1) {
                pr = *rf_pair(f, r, i, pin);
                const unsigned slot = (unsigned)r * 64u + (pr >> 26);
                const V3 d = rf_dir(f, slot);
                V3 P, N;
                hit = ent_hit<TRI>(sc, sc.ents[pr & kRfEntMask], cam.pos, d, P, N, nprim) && sq3(P - cam.pos) < DBL_MAX;   // raytracer.h:58-65
            }
            const unsigned long long mh = __ballot(hit);
            const unsigned k = p0 + kept + (unsigned)__popcll(mh & ((1ull << lane) - 1));
            const unsigned pout = __shfl(pg, rf_page(k));
            if (hit) *rf_pair(f, r, k, pout) = pr;   // at or before its own position, already read
            kept += (unsigned)__popcll(mh);
        }
        if (lane == 0) {
            f.shc[sg] = kept;
            f.sreg[sg] = (unsigned)r;
        }
    }
    if (STATS) wave_add_stats(stats, 0, 0, nprim, 0);
}
// out[k] = sum of ceil(in[j] / div) over j < k, out[n] = the total (in[j] == kRfOvf counts 0); n from
// the device (n_dev) or the host.  One workgroup: tiles of 8192 entries, a coalesced load of their
// counts into LDS, 8 consecutive ones per thread, wave prefix sums by shuffles, the 16 wave totals, a
// coalesced store (the first version -- 32 strided entries per thread -- took ~50 us for the 32,400
// tiles of a 1080p frame; this one ~15 us).
__global__ __launch_bounds__(1024) void k_rf_scan(const unsigned* in, unsigned* out, const unsigned* n_dev, long long n_host,
                                                 unsigned div) {
    __shared__ unsigned s_v[8192];
    __shared__ unsigned s_w[16];
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const long long n = n_dev ? (long long)*n_dev : n_host;
    unsigned carry = 0;
    for (long long base = 0; base < n; base += 8192) {
        for (int k = t; k < 8192; k += 1024) {
            const long long r = base + k;
            const unsigned v = r < n ? in[r] : 0u;
            s_v[k] = v == kRfOvf ? 0u : (v + div - 1u) / div;
        }
        __syncthreads();
        unsigned v[8], sum = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            v[k] = s_v[8 * t + k];
            sum += v[k];
        }
        unsigned incl = sum;   // inclusive prefix over the wave's lanes
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const unsigned u = __shfl_up(incl, off);
            if (lane >= off) incl += u;
        }
        if (lane == 63) s_w[wv] = incl;
        __syncthreads();
        unsigned before = carry, tot = 0;
#pragma unroll
        for (int w = 0; w < 16; ++w) {
            before += w < wv ? s_w[w] : 0u;
            tot += s_w[w];
        }
        unsigned run = before + incl - sum;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            s_v[8 * t + k] = run;
            run += v[k];
        }
        __syncthreads();
        for (int k = t; k < 8192; k += 1024) {
            const long long r = base + k;
            if (r < n) out[r] = s_v[k];
        }
        carry += tot;
        __syncthreads();
    }
    if (t == 0) out[n] = carry;
}
// per hitting pair: its entity's latest reachable appearance that beats the pixel's best rank.
// Persistent waves take chunks of 64 / G consecutive hits of the whole frame in turn (hoff numbers
// them across the segments, so chunks are full; a chunk's first segment by a binary search, each
// hit's from there), so the hits of a soup-core tile are shared by many waves.  G lanes per hit (G =
// 4: each tests 3 of a node's 12 ExpBox faces, r_box_test): a wave's node-test step runs the union
// of its lanes' face tests, which with 64 hits of mixed outcomes is nearly all 12 whether or not a
// face accepts early, so splitting the faces shortens every hit's chain of tests about G-fold for
// the same instructions per hit -- what a sparse launch (an eighth of R-C4: ~500 chunks of 64 on a
// chip of 2,560 wave slots) waits on.  One wave per workgroup: its LDS holds a node-test memo
// (RMemo, GI_R_MEMO entries) per pixel slot of a tile, cleared at every chunk and each entry tagged
// with its hit's run of equal tiles in the chunk, so hits of different tiles never read each
// other's results.
template <bool STATS, int G>
__device__ __forceinline__ void rf_reach_chunks(const DevScene& sc, const CamDev& cam, const RFlat& f, unsigned long long* stats,
                                                int* s_memo, long long n_seg, long long n_hits) {
    constexpr int H = 64 / G;   // hits per chunk
    const int lane = threadIdx.x & 63;
    const int hl = lane / G;   // this lane's hit in the chunk; lane % G its part of the face tests
    const long long gw = ((long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, n_w = ((long long)gridDim.x * blockDim.x) >> 6;
    const bool use_memo = GI_R_MEMO > 0 && sc.n_rnodes < (1 << 22);
    uint32_t nnode = 0;
    // (chunks from a device counter instead, as waves free up: R-C4 0.80 -> 0.88 ms)
    for (long long c = gw; H * c < n_hits; c += n_w) {
        const long long i = H * c + hl;
        long long sg = rf_find(f.hoff, n_seg, H * c);   // the chunk's first segment (uniform)
        long long r = -1;
        if (i < n_hits) {
            while (sg + 1 < n_seg && (long long)f.hoff[sg + 1] <= i) ++sg;   // this hit's
            r = f.sreg[sg];
        }
        // the memo is the chunk's: cleared here (each lane a row), its entries tagged with the hit's
        // run of equal tiles in the chunk (<= 64 runs, so the tag fits its 8 bits).  Two hits share a
        // tag only if they hold the same tile, hence with the same row the same pixel: no entry is
        // ever read for another ray (a tag of the tile's low bits alone let tiles r and r + 256 of
        // one chunk, or of the wave's earlier chunks, read each other's results)
        const long long r_prev = __shfl(r, lane >= G ? lane - G : 0);
        const unsigned long long runs = __ballot(lane % G == 0 && r >= 0 && (hl == 0 || r != r_prev));
        const int run_ord = __popcll(runs & ((2ull << lane) - 1)) - 1;
        if (use_memo) {
            int4* row = reinterpret_cast<int4*>(s_memo + lane * GI_R_MEMO);
            for (int k = 0; k < GI_R_MEMO / 4; ++k) row[k] = make_int4(-1, -1, -1, -1);   // (matches no key)
        }
        __builtin_amdgcn_wave_barrier();
        if (r >= 0) {   // (every value below is the hit's: a group's lanes stay together)
            const unsigned p = (unsigned)(sg - (long long)f.soff[r]) * GI_RF_SEG + (unsigned)(i - (long long)f.hoff[sg]);
            const unsigned pg = p < GI_RF_S0 ? 0u : f.pt[(size_t)r * GI_RF_KMAX + rf_page(p)];
            const unsigned pr = *rf_pair(f, r, p, pg);
            const unsigned slot = (unsigned)r * 64u + (pr >> 26);
            const int e = (int)(pr & kRfEntMask);
            const RMemo memo{use_memo ? s_memo + (pr >> 26) * GI_R_MEMO : nullptr, run_ord << 1};
            const V3 d = rf_dir(f, slot);
            const int a1 = sc.app_off[e + 1];
            for (int a = sc.app_off[e]; a < a1; ++a) {
                const RApp ap = sc.app_rec[a];
                const long long rk = ap.rank;
                long long bst = (long long)*(volatile unsigned long long*)(f.best + slot) - 1;
                if (G > 1) bst = __shfl(bst, lane & ~(G - 1));   // one reading for the group (others raise it)
                if (rk <= bst) break;
                if (r_path_reachable<G>(sc, ap.p0, ap.p1, cam.pos, d, nnode, memo)) {
                    if (lane % G == 0) atomicMax(f.best + slot, (unsigned long long)(rk + 1));
                    break;
                }
            }
        }
    }
    if (STATS) wave_add_stats(stats, 0, lane % G == 0 ? nnode : 0u, 0, 0);   // (node tests per hit, not per lane)
}
// G = 4 for launches of at most kRfGroupHits hits (<= 2,560 chunks of 16: one per resident wave of
// the chip, 10 per CU by the memo's LDS), else G = 1.  R-C4 (266 k hits) and its half and quarter
// shares run faster at G = 1 (whole frame 0.67 against 0.89 ms: where the chip is full, the early
// face exits of the single-lane test save more than the shorter chains); an eighth (33 k hits)
// at G = 4 (rank 0 / 7: 0.33 / 0.37 -> 0.30 / 0.31 ms).  group: 0 chooses, 1 or 4 forces (tests).
constexpr long long kRfGroupHits = 40960;
template <bool STATS>
__global__ __launch_bounds__(64) void k_rf_reach(DevScene sc, CamDev cam, TileMap m, RFlat f, unsigned long long* stats, int group) {
    __shared__ __attribute__((aligned(16))) int s_memo[GI_R_MEMO > 0 ? 64 * GI_R_MEMO : 4];
    const long long n_seg = f.soff[m.n_local], n_hits = f.hoff[n_seg];
    if (group == 4 || (group == 0 && n_hits <= kRfGroupHits)) rf_reach_chunks<STATS, 4>(sc, cam, f, stats, s_memo, n_seg, n_hits);
    else rf_reach_chunks<STATS, 1>(sc, cam, f, stats, s_memo, n_seg, n_hits);
}
// per pixel: the best rank's entity, shaded (overflowed tiles: left to k_mode_r_batch)
template <bool STATS, bool TRI>
__global__ __launch_bounds__(256) void k_rf_shade(DevScene sc, CamDev cam, V3 light, TileMap m, double* rgb, uint8_t* rgb8,
                                                  RFlat f, unsigned long long* stats) {
    const long long slot = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (slot < m.n_local * 64 && f.rcnt[slot >> 6] == kRfOvf) return;   // (uniform: a wave is one tile)
    long long idx = -1;
    int x = 0, y = 0;
    const bool ok = slot < m.n_local * 64 && slot_pixel(m, slot >> 6, (int)(slot & 63), idx, x, y);
    uint32_t nprim = 0;
    if (ok) {
        const V3 d = rf_dir(f, (unsigned)slot);
        const long long b = (long long)f.best[slot] - 1;
        double c0 = 0, c1 = 0, c2 = 0;
        if (b >= 0) {
            const int leaf = sc.r_leaf_of_rank[b >> 32];
            const REnt& e = sc.ents[sc.leaf_ents[sc.rnodes[leaf].ent_off + (int)(b & 0xFFFFFFFFll)]];
            V3 P, N;
            ent_hit<TRI>(sc, e, cam.pos, d, P, N, nprim);
            int32_t u, v;
            tex_coord<TRI>(sc, e, P, u, v);
            const V3 col = shade_ref(e, d, light, P, N, u, v);
            c0 = col.x; c1 = col.y; c2 = col.z;
        }
        if (rgb) { rgb[3 * idx] = c0; rgb[3 * idx + 1] = c1; rgb[3 * idx + 2] = c2; }
        if (rgb8) quantize(c0, c1, c2, rgb8 + 3 * idx);
    } else if (idx >= 0 && m.shard_count > 1) {   // padding slot of a packed tile
        if (rgb) { rgb[3 * idx] = 0; rgb[3 * idx + 1] = 0; rgb[3 * idx + 2] = 0; }
        if (rgb8) { rgb8[3 * idx] = 0; rgb8[3 * idx + 1] = 0; rgb8[3 * idx + 2] = 0; }
    }
    if (STATS) wave_add_stats(stats, ok ? 1 : 0, 0, nprim, ok ? 1 : 0);
}

template <bool STATS>
__global__ __launch_bounds__(256) void k_mode_r(DevScene sc, CamDev cam, V3 light, TileMap m, double* rgb,
                                                 uint8_t* rgb8, unsigned long long* stats, float tau, int dfs) {
    long long idx = -1;
    int x = 0, y = 0;
    const long long lt = (long long)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    const bool ok = lane_pixel(m, lt, idx, x, y);
    y += m.y0;
    uint32_t nnode = 0, nprim = 0;
    if (ok) {
        const V3 o = cam.pos;
        const V3 d = normalize(primary_dir(cam, (double)x, (double)y));   // Ray ctor (ray.h:6)
        RResult r;
        if (dfs) trace_mode_r(sc, o, d, r, nnode, nprim);   // the reference's list order, reversed (A/B)
        else trace_mode_r_cand(sc, o, d, tau, r, nnode, nprim);
        double c0 = 0, c1 = 0, c2 = 0;
        if (r.ent >= 0) {
            const REnt e = sc.ents[r.ent];
            int32_t u, v;
            tex_coord(sc, e, r.P, u, v);
            const V3 col = shade_ref(e, d, light, r.P, r.N, u, v);
            c0 = col.x; c1 = col.y; c2 = col.z;
        }
        if (rgb) { rgb[3 * idx] = c0; rgb[3 * idx + 1] = c1; rgb[3 * idx + 2] = c2; }
        if (rgb8) quantize(c0, c1, c2, rgb8 + 3 * idx);
    } else if (idx >= 0 && m.shard_count > 1) {   // padding lanes of a packed tile
        if (rgb) { rgb[3 * idx] = 0; rgb[3 * idx + 1] = 0; rgb[3 * idx + 2] = 0; }
        if (rgb8) { rgb8[3 * idx] = 0; rgb8[3 * idx + 1] = 0; rgb8[3 * idx + 2] = 0; }
    }
    if (STATS && lt < m.n_local) wave_add_stats(stats, ok ? 1 : 0, nnode, nprim, ok ? 1 : 0);
}

__global__ __launch_bounds__(256) void k_box_kat(int n, const double* recs, int32_t* out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double* q = recs + 12 * (size_t)i;
    out[i] = box_hit(v3(q[0], q[1], q[2]), v3(q[3], q[4], q[5]), v3(q[6], q[7], q[8]),
                     normalize(v3(q[9], q[10], q[11]))) ? 1 : 0;
}

// Primitive-level known-answer kernels (gi_kat_r_prims): one record per lane through the functions the
// Mode R kernels call, the direction normalised as k_box_kat does.  kind 0: tri_hit(const TriRec&) on the
// host-built record (15 doubles p1 p2 p3 o dir); 1: sphere_hit (10 doubles pos radius o dir, the radius
// narrowed to float as REnt stores it); 2: box_hit (12 doubles, k_box_kat's record).  pn (P, N; zeros on
// a miss) is written for kinds 0 and 1.
__global__ __launch_bounds__(256) void k_r_prims_kat(int kind, int n, const double* recs, const TriRec* tris,
                                                     int32_t* hit, double* pn) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    V3 P = v3(0, 0, 0), N = v3(0, 0, 0);
    bool h;
    if (kind == 0) {
        const double* q = recs + 15 * (size_t)i;
        h = tri_hit(tris[i], v3(q[9], q[10], q[11]), normalize(v3(q[12], q[13], q[14])), P, N);
    } else if (kind == 1) {
        const double* q = recs + 10 * (size_t)i;
        h = sphere_hit(v3(q[0], q[1], q[2]), (float)q[3], v3(q[4], q[5], q[6]), normalize(v3(q[7], q[8], q[9])), P, N);
    } else {
        const double* q = recs + 12 * (size_t)i;
        h = box_hit(v3(q[0], q[1], q[2]), v3(q[3], q[4], q[5]), v3(q[6], q[7], q[8]), normalize(v3(q[9], q[10], q[11])));
    }
    hit[i] = h ? 1 : 0;
    if (kind <= 1) {
        double* w = pn + 6 * (size_t)i;
        w[0] = P.x; w[1] = P.y; w[2] = P.z; w[3] = N.x; w[4] = N.y; w[5] = N.z;
    }
}
// kind 3: k_rf_reach's grouped node test itself -- record i is held by the 4 consecutive lanes 4i .. 4i + 3
// (a group lies inside one wave, and its lanes leave or stay together).
__global__ __launch_bounds__(256) void k_r_box4_kat(int n, const double* recs, int32_t* hit) {
    const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long i = t >> 2;
    if (i >= n) return;
    const double* q = recs + 12 * (size_t)i;
    const bool h = r_box_test<4>(v3(q[0], q[1], q[2]), v3(q[3], q[4], q[5]), v3(q[6], q[7], q[8]),
                                 normalize(v3(q[9], q[10], q[11])));
    if ((t & 3) == 0) hit[i] = h ? 1 : 0;
}
// gi_kat_r_entities: every ray (o, dir normalised here) against every entity through ent_hit, one pair
// per lane; P and N start as zeros and are stored as ent_hit leaves them.
template <bool TRI>
__global__ __launch_bounds__(256) void k_r_entities_kat(DevScene sc, int n, const double* rays, int32_t* hit, double* pn) {
    const long long j = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= (long long)n * sc.n_ents) return;
    const long long i = j / sc.n_ents;
    const int k = (int)(j - i * sc.n_ents);
    const double* q = rays + 6 * (size_t)i;
    V3 P = v3(0, 0, 0), N = v3(0, 0, 0);
    uint32_t nprim = 0;
    const bool h = ent_hit<TRI>(sc, sc.ents[k], v3(q[0], q[1], q[2]), normalize(v3(q[3], q[4], q[5])), P, N, nprim);
    hit[j] = h ? 1 : 0;
    double* w = pn + 6 * (size_t)j;
    w[0] = P.x; w[1] = P.y; w[2] = P.z; w[3] = N.x; w[4] = N.y; w[5] = N.z;
}

__global__ __launch_bounds__(64) void k_trace_ray(DevScene sc, V3 o, V3 d, V3 light, int32_t* out_i, double* out_d) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    RResult r;
    uint32_t nn = 0, np = 0;
    const double reach = fmax(fabs(o.x), fmax(fabs(o.y), fabs(o.z))) + (double)sc.rc_ext;
    trace_mode_r_cand(sc, o, d, (float)(1e-5 * reach + 1e-30), r, nn, np);
    out_i[0] = r.ent;
    out_i[1] = out_i[2] = 0;
    for (int k = 0; k < 9; ++k) out_d[k] = 0;
    if (r.ent >= 0) {
        const REnt e = sc.ents[r.ent];
        int32_t u, v;
        tex_coord(sc, e, r.P, u, v);
        const V3 col = shade_ref(e, d, light, r.P, r.N, u, v);
        out_i[1] = u; out_i[2] = v;
        out_d[0] = r.P.x; out_d[1] = r.P.y; out_d[2] = r.P.z;
        out_d[3] = r.N.x; out_d[4] = r.N.y; out_d[5] = r.N.z;
        out_d[6] = col.x; out_d[7] = col.y; out_d[8] = col.z;
    }
}

}  // namespace

unsigned rf_own_pairs() { return GI_RF_S0; }
unsigned rf_page_pairs() { return GI_RF_PAGE; }
unsigned rf_max_pages() { return GI_RF_KMAX; }
unsigned rf_seg_pairs() { return GI_RF_SEG; }
// Mode R kernel of a launch (RKernel): k_mode_r for small scenes, the reverse-DFS flag and an octree that
// never split; the flat phases for scenes of more than 4096 entities (their overflowed tiles through
// k_mode_r_batch); k_mode_r_batch for the whole frame with GI_R_FLAT=2 (tests) and for scenes of 2^26
// entities or more, beyond the flat phases' one-word pairs
RKernel r_kernel_choice(const DevScene& sc, const gi_opts& o) {
    if (o.mode != GI_MODE_R || (o.flags & GI_FLAG_R_DFS) || sc.n_rnodes <= 1) return RK_PIXEL;
    const XEnv& env = x_env();
    const bool large = env.r_flat >= 0 ? env.r_flat != 0 : sc.n_ents > 4096;
    if (!large) return RK_PIXEL;
    return (env.r_flat == 2 || (unsigned)sc.n_ents > kRfEntMask) ? RK_BATCH : RK_FLAT;
}

hipError_t launch_mode_r(const DevScene& sc, const CamDev& cam, V3 light, int w, int h, int y0, const gi_opts& o,
                         double* rgb, uint8_t* rgb8, const XScratch& xs, hipStream_t stream, hipEvent_t ev_begin,
                         hipEvent_t ev_end) {
    const TileMap m = make_map(w, h, o.shard_count, o.shard_index, y0);   // (launch_render's: TileMap is local to a unit)
    const dim3 grid((unsigned)((m.n_local + kWavesPerBlock - 1) / kWavesPerBlock)), block(64 * kWavesPerBlock);
    unsigned long long* st = reinterpret_cast<unsigned long long*>(o.stats);
    const bool stats = (o.flags & GI_FLAG_STATS) && st;
    // line-BVH widening: the prefilter's 1e-12|oc|^2 slack (<= 1e-6 |oc|) and fp32 slab rounding
    const double reach = std::max(std::fabs(cam.pos.x), std::max(std::fabs(cam.pos.y), std::fabs(cam.pos.z))) + (double)sc.rc_ext;
    const float tau = (float)(1e-5 * reach + 1e-30);
    // an octree that never split is one leaf: its list scanned backwards (first success) is
    // already the least work
    const int dfs = ((o.flags & GI_FLAG_R_DFS) || sc.n_rnodes <= 1) ? 1 : 0;
    const RKernel rk = r_kernel_choice(sc, o);
    const bool tri = sc.r_tri_only != 0;   // ImpTriangle-only scenes: the other entity kinds' code dropped
    if (ev_begin) (void)hipEventRecord(ev_begin, stream);
    if (rk == RK_FLAT && xs.rf_pairs && xs.rf_slots >= m.n_local * (kTile * kTile)) {   // flat phases
        const RFlat f{xs.rf_pairs, xs.rf_pairs + (size_t)(xs.rf_slots / 64) * GI_RF_S0, xs.rf_pt, xs.rf_best, xs.rf_cnt,
                      xs.rf_ovf, xs.rf_rcnt, xs.rf_soff, xs.rf_shc, xs.rf_sreg, xs.rf_hoff, xs.rf_dir, xs.rf_pages};
        const dim3 pgrid((unsigned)((m.n_local * (kTile * kTile) + 255) / 256)), fgrid(4096);
        hipError_t e1 = hipMemsetAsync(xs.rf_cnt, 0, 2 * sizeof(unsigned), stream);
        if (e1 != hipSuccess) return e1;
        // the overflowed tiles' fallback: half a tile per workgroup item, a grid that returns at once
        // when the list is empty
        const dim3 bgrid((unsigned)std::min<long long>(2 * m.n_local, 2048));
        const dim3 hgrid(16384);   // k_rf_hit: persistent waves (one per workgroup) over the segments
        const int rgroup = x_env().rf_group;
        with_bools([&](auto S, auto T) {
            hipLaunchKernelGGL(k_rf_walk<S.value>, pgrid, block, 0, stream, sc, cam, m, tau, f, st);
            hipLaunchKernelGGL(k_rf_scan, dim3(1), dim3(1024), 0, stream, f.rcnt, f.soff, nullptr, m.n_local, GI_RF_SEG);
            hipLaunchKernelGGL((k_rf_hit<S.value, T.value>), hgrid, dim3(64), 0, stream, sc, cam, m, f, st);
            hipLaunchKernelGGL(k_rf_scan, dim3(1), dim3(1024), 0, stream, f.shc, f.hoff, f.soff + m.n_local, 0ll, 1u);
            hipLaunchKernelGGL(k_rf_reach<S.value>, dim3(4 * fgrid.x), dim3(64), 0, stream, sc, cam, m, f, st, rgroup);
            hipLaunchKernelGGL((k_rf_shade<S.value, T.value>), pgrid, block, 0, stream, sc, cam, light, m, rgb, rgb8, f, st);
            hipLaunchKernelGGL((k_mode_r_batch<S.value, T.value>), bgrid, block, 0, stream, sc, cam, light, m, rgb, rgb8, st, tau,
                               (const unsigned*)xs.rf_ovf, (const unsigned*)(xs.rf_cnt + 1));
        }, stats, tri);
    } else if (rk != RK_PIXEL) {   // k_mode_r_batch over the whole frame
        const dim3 sgrid((unsigned)((m.n_local * (kTile * kTile) + 31) / 32));
        with_bools([&](auto S, auto T) {
            hipLaunchKernelGGL((k_mode_r_batch<S.value, T.value>), sgrid, block, 0, stream, sc, cam, light, m, rgb, rgb8, st, tau, nullptr, nullptr);
        }, stats, tri);
    } else {
        with_bools([&](auto S) { hipLaunchKernelGGL(k_mode_r<S.value>, grid, block, 0, stream, sc, cam, light, m, rgb, rgb8, st, tau, dfs); },
                   stats);
    }
    if (ev_end) (void)hipEventRecord(ev_end, stream);
    return hipSuccess;
}

hipError_t launch_box_kat(int n, const double* recs, int32_t* out, hipStream_t stream) {
    if (n > 0) hipLaunchKernelGGL(k_box_kat, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, n, recs, out);
    return hipGetLastError();
}

hipError_t launch_r_prims_kat(int kind, int n, const double* recs, const TriRec* tris, int32_t* hit, double* pn,
                              hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    if (kind == 3)
        hipLaunchKernelGGL(k_r_box4_kat, dim3((unsigned)((4ll * n + 255) / 256)), dim3(256), 0, stream, n, recs, hit);
    else
        hipLaunchKernelGGL(k_r_prims_kat, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, kind, n, recs, tris, hit, pn);
    return hipGetLastError();
}

hipError_t launch_r_entities_kat(const DevScene& sc, int n, const double* rays, int32_t* hit, double* pn, hipStream_t stream) {
    const long long pairs = (long long)n * sc.n_ents;
    if (pairs <= 0) return hipSuccess;
    const dim3 grid((unsigned)((pairs + 255) / 256));
    if (sc.r_tri_only)
        hipLaunchKernelGGL(k_r_entities_kat<true>, grid, dim3(256), 0, stream, sc, n, rays, hit, pn);
    else
        hipLaunchKernelGGL(k_r_entities_kat<false>, grid, dim3(256), 0, stream, sc, n, rays, hit, pn);
    return hipGetLastError();
}

hipError_t launch_trace_ray(const DevScene& sc, V3 o, V3 d, V3 light, int32_t* out_i, double* out_d, hipStream_t stream) {
    hipLaunchKernelGGL(k_trace_ray, dim3(1), dim3(64), 0, stream, sc, o, d, light, out_i, out_d);
    return hipGetLastError();
}

}  // namespace gi
