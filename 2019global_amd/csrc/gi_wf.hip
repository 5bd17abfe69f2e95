// gi_wf.hip — Mode X in wavefront form (WF): one kernel launch per bounce over a compacted queue of
// live paths, instead of the persistent path-state machine of k_mode_x (gi_kernels.hip).
//
// Per bounce b every lane of a wave runs the same sequence on one path (the per-pixel
// body raytracer.h:41-84 extended by the build-defined integrator, DESIGN.md "Mode X"):
//   closest-hit traversal -> hit point, light direction -> shadow any-hit traversal -> shading
//   (texture, Blinn-Phong with the shadow answer) -> L += T * local -> next direction (mirror /
//   cosine-weighted) -> the path is appended to the next bounce's queue, or its radiance stored.
// The queue is compacted with one ballot + prefix count + one atomic per wave (paths that end drop
// out), so bounce b + 1 launches over exactly the live paths.  Bounce 0 enumerates the work list's
// (pixel, sample) units directly (no queue: a primary ray is regenerated from its unit).  Path
// records are SoA in HBM (o, d, L, T in fp64 + (list index, sample): 104 B); a frame whose units
// exceed a queue's capacity runs in chunks of units, each chunk depth launches.
//
// Results: every path runs exactly the oracle's operations (oracle/gi_oracle.cpp sample_mode_x);
// the closest hit is the minimum of (t, primitive index) whatever the traversal order, and the
// per-sample radiance rows are summed in sample order by k_x_reduce as for k_mode_x -- so frames
// are bit-identical to k_mode_x's and the oracle's (tests/test_gpu_parity.py).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <mutex>
#include <type_traits>

#include "gi.h"
#include "gi_dev.h"
#include "gi_fan_pair.h"
#include "gi_launch.h"
#include "gi_scene.h"
#include "gi_seg_ring.h"

namespace gi {
namespace {

constexpr long long kWfTile = 8;   // pixel tiles are 8 x 8 (GI_TILE)

#ifndef GI_WF_MIN_WAVES_LDS
#define GI_WF_MIN_WAVES_LDS 4   // LDS-resident scenes, light shading (<= 128 VGPRs)
#endif
#ifndef GI_WF_MIN_WAVES
#define GI_WF_MIN_WAVES 3       // other scenes
#endif
#ifndef GI_WF_TAKE
#define GI_WF_TAKE 16   // most 64-entry batches a wave takes per atomic on the queue's counter
#endif
// a path's L and T wait out the two traversals in a per-lane LDS slot (column layout, 6 x 256 fp64 per
// workgroup) instead of VGPRs: the 4-wave kernel stays within 128 VGPRs.  k_seg also keeps the path's
// RNG key and its output index and sample there (fields 6, 7), read where they are used: carried in
// VGPRs across the traversals they were spilled to scratch (136 -> 56 B per lane).  The path's bounce
// index rides in the high bits of k_seg's own-plane register (kSegPlaneBits).
// LDS-resident scenes test leaf records two at a time (PAIR: two interleaved fp64 chains) and their
// node slab tests issue the 12 loads at once (round 5: C3 4.90 -> 4.81 ms against axis by axis)
constexpr size_t kWfSlotBytes = 8 * 256 * sizeof(double);
// k_seg's per-wave ring of prepared primary rays, behind the path slots of launches that
// carry it: five planes (d.x, d.y, d.z, key, idx | smp << 32) of 64 x 8 B per wave
constexpr int kSegRingPlanes = 5;
constexpr size_t kSegRingBytes = 4 * kSegRingPlanes * kSegBatch * sizeof(uint64_t);
// k_seg's plane register: the own-plane skip of the lane's next ray in the low bits, the path's bounce
// index (< 2^16, gi_capi.cpp) above them
constexpr int kSegPlaneBits = 8, kSegPlaneMask = (1 << kSegPlaneBits) - 1;

// a path's identity where the shading needs it: RNG key, sample, bounce
struct PathId {
    uint64_t key;
    unsigned smp;
    int b;
};
__device__ __forceinline__ void slot_put_u64(double* pl, int f, uint64_t v) { reinterpret_cast<uint64_t*>(pl)[f * 256] = v; }
__device__ __forceinline__ uint64_t slot_get_u64(const double* pl, int f) { return reinterpret_cast<const uint64_t*>(pl)[f * 256]; }

// one queue of path records: field f (o.xyz, d.xyz, L.xyz, T.xyz) of entry j at r[f * cap + j]
struct WFQ {
    double* r;
    uint2* id;   // (work-list index, sample)
    long long cap;
};

// Closest hit (ANY = false: the (t, primitive) minimum over t > MX_TMIN) or any hit before tmax
// (ANY: a shadow ray; true on the first primitive found) of the ray o + t d through the 8-wide BVH.
// Stackless: 8-bit "children left" mask per level (SH: one 64-bit word, trees of <= 8 levels);
// climbing by parent pointers (LDS-resident scenes) or the per-lane level stack nst (HBM).
// PAIR: leaf records two at a time (two interleaved fp64 chains; LDS records); otherwise records
// fetched one ahead of their test.  LDS-resident scenes (!NST), closest hit: a popped child is
// re-tested against the current best t (its box is a ds_read away).
template <bool ANY, bool PAIR, bool AXIS, bool SH, bool TRI, bool NST, typename NodeP, typename HotP>
__device__ __forceinline__ int wf_trace(float far_r, NodeP W, HotP H, V3 o, V3 d, double tmax, bool act, int* nst, double& t_out,
                                        uint32_t& nnode, uint32_t& nprim, uint32_t& nsteps, int skip = 254) {
    // the own-plane skip (XWNode scenes; gi_build.cpp assign_plane_groups): leaves of group skip are
    // never entered -- their exact tests would all find t below MX_TMIN for this ray
    constexpr bool kSkip = std::is_same<NodeP, const XWNode*>::value;
    const F3 of = ray_org32(o, d, far_r);
    const F3 ivf = inv_dir(d);
    const int dmask = (d.x < 0 ? 1 : 0) | (d.y < 0 ? 2 : 0) | (d.z < 0 ? 4 : 0);
    double tb = tmax;
    float tbf = up32(tmax);
    int best = -1;
    uint64_t mlo = 0, mhi = 0;
    int node = 0, level = 0;
    bool raying = false;
    if (act) {
        uint32_t rm;
        if constexpr (kSkip) rm = children_mask<AXIS, true>(W, of, ivf, tbf, dmask, skip);
        else rm = children_mask<AXIS>(W, of, ivf, tbf, dmask);
        lvl_set<SH>(mlo, mhi, 0, rm);
        raying = rm != 0;
    }
    while (raying) {
        ++nsteps;
        const auto* nd = W + node;
        const uint32_t msk = lvl_get<SH>(mlo, mhi, level);
        const int kc = __builtin_ctz(msk);   // next child in front-to-back order
        lvl_set<SH>(mlo, mhi, level, msk & (msk - 1));
        const int c = kc ^ dmask;
        bool keep = true;
        if (!ANY && !NST && best >= 0) {   // (LDS scenes) re-cull against the current best t
            keep = child_hit(nd, c, of, ivf, tbf);
        }
        const int ch = nd->child[c];
        if (keep) {
            if (ch < 0) {   // leaf: the fp64 primitive tests decide
                const int cnt = nd->cnt[c];
                const auto* hp = H + ~ch;
                if constexpr (PAIR) {
                    for (int j = 0; j < cnt; j += 2) {
                        const bool two = j + 1 < cnt;
                        const XHotR r0 = load_hot(hp + j), r1 = load_hot(hp + (two ? j + 1 : j));
                        const double ta = x_prim_t<TRI>(r0.h, o, d, MX_TMIN);
                        const double tq = two ? x_prim_t<TRI>(r1.h, o, d, MX_TMIN) : INFINITY;
                        nprim += two ? 2 : 1;
                        if (ANY) {
                            if ((ta < tmax) | (tq < tmax)) {
                                best = ta < tmax ? r0.h.prim : r1.h.prim;
                                break;
                            }
                        } else {   // (selects, not branches: | and & do not short-circuit)
                            const bool ua = (ta < tb) | ((ta == tb) & (r0.h.prim < best));
                            tb = ua ? ta : tb;
                            best = ua ? r0.h.prim : best;
                            const bool uq = (tq < tb) | ((tq == tb) & (r1.h.prim < best));
                            tb = uq ? tq : tb;
                            best = uq ? r1.h.prim : best;
                            tbf = up32(tb);
                        }
                    }
                } else {
                    XHotR cur = load_hot(hp);
                    for (int j = 0; j < cnt; ++j) {
                        const XHotR rec = cur;
                        if (j + 1 < cnt) cur = load_hot(hp + j + 1);
                        ++nprim;
                        const double t = x_prim_t<TRI>(rec.h, o, d, MX_TMIN);
                        if (ANY) {
                            if (t < tmax) { best = rec.h.prim; break; }
                        } else {
                            const bool u = (t < tb) | ((t == tb) & (rec.h.prim < best));
                            tb = u ? t : tb;
                            best = u ? rec.h.prim : best;
                            tbf = u ? up32(t) : tbf;
                        }
                    }
                }
            } else {        // interior: descend if any of its children is hit (fp32 slabs)
                ++nnode;
                uint32_t cm;
                if constexpr (kSkip) cm = children_mask<AXIS, true>(W + ch, of, ivf, tbf, dmask, skip);
                else cm = children_mask<AXIS>(W + ch, of, ivf, tbf, dmask);
                if (cm) {
                    node = ch;
                    ++level;
                    lvl_set<SH>(mlo, mhi, level, cm);
                    if (NST) nst[level * 256] = ch;
                }
            }
        }
        if (ANY && best >= 0) break;
        uint32_t rest = lvl_get<SH>(mlo, mhi, level);
        if (rest == 0 && level > 0) {   // climb to the nearest level with children left
            if constexpr (NST) {
                const uint64_t lm = level >= 8 ? mlo : mlo & ((1ull << (8 * level)) - 1);
                const uint64_t hm = level <= 8 ? 0ull : mhi & ((1ull << (8 * (level - 8))) - 1);
                level = hm ? 8 + (63 - __clzll((long long)hm)) / 8 : lm ? (63 - __clzll((long long)lm)) / 8 : 0;
                rest = lvl_get<SH>(mlo, mhi, level);
                node = level == 0 ? 0 : nst[level * 256];
            } else {
                do {
                    --level;
                    node = level == 0 ? 0 : W[node].parent;   // the root is node 0: no load
                    rest = lvl_get<SH>(mlo, mhi, level);
                } while (rest == 0 && level > 0);
            }
        }
        raying = rest != 0;
    }
    t_out = tb;
    return best;
}

// The flat leaf query (scenes staged in LDS with at most GI_XFLAT_MAX leaves): the same
// answer as wf_trace without the tree walk.
//  Phase A, uniform over the wave: every record of the leaf table (DevScene::xflat) is read at a
//    wave-uniform address -- through the constant cache, so its eight words are scalar operands -- and
//    its box tested for every lane with child_hit's arithmetic against [0, tmax]; leaves of the ray's
//    own plane group are dropped as children_mask<AXIS, true> drops them.  Every leaf shifts its hit
//    bit into the lane's candidate mask.  Closest hit: the two smallest keys of the candidates are kept,
//    a key being the entry distance with the leaf index in its low five bits -- so the nearest
//    candidate travels with its distance, to within 31 ulp.  Nothing else is carried per leaf.
//  Phase B, per lane: the PAIR leaf block of wf_trace on one candidate per iteration, its (offset,
//    count) read per lane from the table.  Closest hit: the smallest key's leaf first; a lane whose best
//    t lies in front of the second key's floor is finished (no other box reaches it); otherwise the
//    remaining candidates in bit order, each re-tested against the current best t (a per-lane read of
//    its record) before its exact tests.  Any hit: candidates from the lowest bit up (the highest leaf
//    first) until one is hit.
//  The keys round entry distances, which only orders the candidates; the one decision taken on a key,
//    the early exit, compares a value that is not above any remaining candidate's true entry distance.
// Exactness: the closest hit is the (t, primitive) minimum over all primitives whatever the order,
// a leaf is left out only by the conservative box test or the own-plane rule the tree walk uses,
// and the shadow answer is a boolean.
// STATS: nnode counts the 256-byte units of the table a query reads, nsteps Phase B's iterations.
constexpr size_t kFlatPkBytes = GI_XFLAT_MAX * sizeof(uint32_t);   // the leaves' candidate words in LDS (wf_stage)
typedef uint32_t u32x8 __attribute__((ext_vector_type(8)));
// record k's eight words from the constant address space: a scalar load at a uniform address (a copy
// of the table staged in LDS and read by broadcast measured 2.5% slower on the Cornell box, round 8)
__device__ __forceinline__ u32x8 flat_rec_uniform(const XFlatLeafDev* tab, int k) {
    return *(const __attribute__((address_space(4))) u32x8*)(uintptr_t)(tab + k);
}
// (offset, index, count) of a candidate in one word: offset < 2^16, count <= 255 (HostScene::x_flat_ok)
__device__ __forceinline__ uint32_t flat_pack(uint32_t off, int k, uint32_t w7) { return off | ((uint32_t)k << 16) | ((w7 & 0xFFu) << 24); }
// Phase A's per-leaf bookkeeping, one instruction each.  The compiler has no single-instruction form for
// either from C++ (it selects a 0/1 select + shift-or, and an and + or), hence the two asm lines.
//  flat_shift_in: m + m + (the lane's bit of the wave mask hm) -- an add with carry-in.
//  flat_key: the entry distance's bits with the low five replaced by the leaf index k (uniform, < 32).
__device__ __forceinline__ uint32_t flat_shift_in(uint32_t m, unsigned long long hm) {
    uint32_t r;
    asm("v_addc_co_u32 %0, vcc, %1, %1, %2" : "=v"(r) : "v"(m), "s"(hm) : "vcc");
    return r;
}
__device__ __forceinline__ int flat_key(float tn, int k) {
    int r;
    asm("v_bfi_b32 %0, 31, %1, %2" : "=v"(r) : "s"(k), "v"(tn));
    return r;
}
// the middle of three (selected as one v_med3_i32)
__device__ __forceinline__ int flat_med3(int a, int b, int c) { return max(min(a, b), min(max(a, b), c)); }
// a key without its index bits: not above the entry distance it was made from
__device__ __forceinline__ float flat_key_floor(int e) { return __int_as_float(e & ~31); }
// (offset, index, count) of leaf k, read per lane from the words wf_stage packed into LDS (the flat query
// runs on scenes staged in LDS only): an LDS read where a read of the table record in global memory put
// a cache round trip on every query's path (C3 3.31 -> 3.29 ms, round 8)
__device__ __forceinline__ uint32_t flat_pk_of(const uint32_t* pkw, int k) { return pkw[k]; }
// Phase A's plane distances, two packed fmas per axis (DESIGN.md §5 "Two-stage slab distances").  With ivp the
// reciprocal where it is positive and +0 otherwise, and ivn the reciprocal where it is negative and +0 otherwise,
//   near = fma(hi, ivn, fma(lo, ivp, no)),  far = fma(lo, ivn, fma(hi, ivp, no))
// are child_hit's near / far distances without a select: for a positive reciprocal the inner fma is the plane's
// distance and the outer adds hi x 0 (or lo x 0) to it; for a negative one the inner fma is 0 + no = no exactly and
// the outer is child_hit's fma.  The reciprocals are finite and not zero (inv_dir) and the boxes finite, so no
// 0 x inf arises, and an inner overflow stays the same infinity; only the sign of an exact zero can differ, which
// no comparison sees.
//  flat_pk_inner: (fma(lo, ivp, no), fma(hi, ivp, no)) from lh = (lo, hi), iv = (ivp, ivn) and half H of nn.
//  flat_pk_outer: (near, far) from the same lh with its halves swapped, ivn, and the inner pair.
// lh is a scalar register pair: two neighbouring words of a record read at a uniform address (XFlatLeafDev).
typedef float f32x2 __attribute__((ext_vector_type(2)));
template <int H>
__device__ __forceinline__ f32x2 flat_pk_inner(f32x2 lh, f32x2 iv, f32x2 nn) {
    f32x2 r;
    if constexpr (H == 0) asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel_hi:[1,0,0]" : "=v"(r) : "s"(lh), "v"(iv), "v"(nn));
    else asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[0,0,1] op_sel_hi:[1,0,1]" : "=v"(r) : "s"(lh), "v"(iv), "v"(nn));
    return r;
}
__device__ __forceinline__ f32x2 flat_pk_outer(f32x2 lh, f32x2 iv, f32x2 in) {
    f32x2 r;
    asm("v_pk_fma_f32 %0, %1, %2, %3 op_sel:[1,1,0] op_sel_hi:[0,1,1]" : "=v"(r) : "s"(lh), "v"(iv), "v"(in));
    return r;
}
// The interval of a box from its three (near, far) pairs: tn = max(near x, near y, max(near z, 0)) and
// tf = min(far x, far y, min(far z, tend)), child_hit's.  As instructions because the compiler does not know that a
// result of the asm lines above is canonical and would quiet each one before its minimum or maximum (a
// v_max_f32 x, x per operand); an fma returns no signalling NaN, and tend is canonical where it is made.
__device__ __forceinline__ float flat_tn(f32x2 px, f32x2 py, f32x2 pz) {
    float t, r;
    asm("v_max_f32 %0, 0, %1" : "=v"(t) : "v"(pz.x));
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(px.x), "v"(py.x), "v"(t));
    return r;
}
__device__ __forceinline__ float flat_tf(f32x2 px, f32x2 py, f32x2 pz, float tend) {
    float t, r;
    asm("v_min_f32 %0, %1, %2" : "=v"(t) : "v"(pz.y), "v"(tend));
    asm("v_min3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(px.y), "v"(py.y), "v"(t));
    return r;
}
// (ivp, ivn) of one reciprocal, by its sign bit as iv_signs takes it
__device__ __forceinline__ f32x2 flat_iv_pair(float iv) {
    const bool neg = (int)__float_as_uint(iv) < 0;
    f32x2 r = {neg ? 0.0f : iv, neg ? iv : 0.0f};
    return r;
}
// the query's operands of the two forms: per axis (ivp, ivn); (no.x, no.y) and (no.z, the interval's end: the
// pair's other half is not an operand of the fmas, so the bound the far distances are cut at rides in it)
struct FlatPk {
    f32x2 ix, iy, iz, nxy, nzt;
};
__device__ __forceinline__ FlatPk flat_pk_of_ray(F3 no, F3 ivf, float tend) {
    FlatPk q;
    q.ix = flat_iv_pair(ivf.x);
    q.iy = flat_iv_pair(ivf.y);
    q.iz = flat_iv_pair(ivf.z);
    q.nxy = f32x2{no.x, no.y};
    q.nzt = f32x2{no.z, tend};
    return q;
}
// child_hit on a table record read per lane: the select form, whose distances are Phase A's (above).  The record is
// the lane's own, so the choice of near and far is made on the planes; the two-stage form here needs the three
// (ivp, ivn) pairs beside Phase B's fp64 tests and put k_wf_bounce into scratch (DESIGN.md §9 "Round 14").
__device__ __forceinline__ bool flat_hit(const XFlatLeafDev* r, F3 no, F3 ivf, float tmax, uint32_t& pk, int k) {
    const int4* q = reinterpret_cast<const int4*>(r);
    const int4 a = q[0], b = q[1];
    const float lx = __int_as_float(a.x), hx = __int_as_float(a.y), ly = __int_as_float(a.z);
    const float hy = __int_as_float(a.w), lz = __int_as_float(b.x), hz = __int_as_float(b.y);
    const int sm = iv_signs(ivf);
    const float nx = (sm & 1) ? hx : lx, fx = (sm & 1) ? lx : hx;
    const float ny = (sm & 2) ? hy : ly, fy = (sm & 2) ? ly : hy;
    const float nz = (sm & 4) ? hz : lz, fz = (sm & 4) ? lz : hz;
    const float tn = fmaxf(fmaxf(__builtin_fmaf(nx, ivf.x, no.x), __builtin_fmaf(ny, ivf.y, no.y)),
                           fmaxf(__builtin_fmaf(nz, ivf.z, no.z), 0.0f));
    const float tf = fminf(fminf(__builtin_fmaf(fx, ivf.x, no.x), __builtin_fmaf(fy, ivf.y, no.y)),
                           fminf(__builtin_fmaf(fz, ivf.z, no.z), tmax));
    pk = flat_pack((uint32_t)b.z, k, (uint32_t)b.w);
    return tn <= tf;
}
// fan (launch-uniform, DevScene::x_fan; the TRI kernels): every leaf is a fan pair, phase B runs one exact test per
// leaf where the first record's first step decides (gi_fan_pair.h) -- the same (t, primitive) as with both
template <bool ANY, bool TRI>
__device__ __forceinline__ int wf_flat(float far_r, const XFlatLeafDev* tab, const uint32_t* pkw, int n, const XHot* H, V3 o, V3 d, double tmax, bool act,
                                       double& t_out, uint32_t& nnode, uint32_t& nprim, uint32_t& nsteps, int skip, bool fan, uint32_t live) {
    const F3 of = ray_org32(o, d, far_r);
    const F3 ivf = inv_dir(d);
    const F3 no = neg_oiv(of, ivf);
    double tb = tmax;
    float tbf = up32(tmax);
    int best = -1;
    // ---- phase A (a lane without a ray: an empty interval, no candidates)
    // (canonical here, once: the minimum it enters would otherwise quiet it again for every leaf)
    const float tfa = __builtin_canonicalizef(act ? tbf : -1.0f);
    const FlatPk pq = flat_pk_of_ray(no, ivf, tfa);
    // m: the hit bits shifted in, so leaf k ends at bit n - 1 - k.  Closest hit: e1 <= e2, the two
    // smallest candidate keys -- the entry distance's bits (tn >= 0: ordered as integers; -0 sorts first,
    // which is its place) with the low five overwritten by the leaf index, so min / med3 carry the
    // candidate along.  A key lies within 31 ulp of its tn on either side; flat_key_floor(key) <= tn.
    constexpr int kNone = 0x7F800000;   // +inf: no candidate
    uint32_t m = 0, pk = 0;
    int e1 = kNone, e2 = kNone;
    auto step = [&](const u32x8 w, int k) {
        // (lo, hi) of each axis: a scalar register pair of the record as loaded
        const f32x2 lhx = {__uint_as_float(w[0]), __uint_as_float(w[1])}, lhy = {__uint_as_float(w[2]), __uint_as_float(w[3])};
        const f32x2 lhz = {__uint_as_float(w[4]), __uint_as_float(w[5])};
        // (near, far) per axis: child_hit's values by two packed fmas, no select (flat_pk_inner)
        const f32x2 px = flat_pk_outer(lhx, pq.ix, flat_pk_inner<0>(lhx, pq.ix, pq.nxy));
        const f32x2 py = flat_pk_outer(lhy, pq.iy, flat_pk_inner<1>(lhy, pq.iy, pq.nxy));
        const f32x2 pz = flat_pk_outer(lhz, pq.iz, flat_pk_inner<0>(lhz, pq.iz, pq.nzt));
        const float tn = flat_tn(px, py, pz), tf = flat_tf(px, py, pz, pq.nzt.y);
        const bool in = tn <= tf, other = (int)((w[7] >> 16) & 0xFFu) != skip;
        // (the two compares' wave masks, so that their conjunction is the add's carry-in as it stands)
        m = flat_shift_in(m, __builtin_amdgcn_ballot_w64(in) & __builtin_amdgcn_ballot_w64(other));
        if (!ANY) {
            const int key = flat_key(tn, k);   // (outside the select: asm is not speculated)
            const int eh = (in & other) ? key : kNone;
            e2 = flat_med3(e1, e2, eh);   // (e1 <= e2: the middle is the second smallest)
            e1 = min(e1, eh);
        }
    };
    // four records at a time, written out: the wave masks of step() are convergent operations, which the
    // compiler does not unroll around when the trip count is a run-time value
    // live (launch-uniform; the any hit of a path's shadow ray, x_segment): bit k clear -- leaf k cannot occlude
    // this launch's light (gi_build.cpp mark_boundary_leaves) and is not read.  The set bits are visited in
    // order, up to four records per round so that their scalar loads stay batched; before a leaf that follows
    // g skipped ones the candidate mask moves up by g, and by the trailing gap at the end, so leaf k ends at
    // bit n - 1 - k as in the dense loop.  All ones (every other caller, as a constant): the dense loop alone.
    int k0 = 0;
    if (ANY && live != ~0u) {
        uint32_t rem = live & (n >= 32 ? ~0u : (1u << n) - 1u);
        int prev = -1;
        auto sstep = [&](const u32x8 w, int k) {
            m <<= (k - prev - 1) & 31;   // (m is 0 before the first visited leaf)
            step(w, k);
            prev = k;
        };
        while (rem != 0) {
            const int ka = __builtin_ctz(rem);
            rem &= rem - 1;
            const int kb = rem ? __builtin_ctz(rem) : -1;
            rem &= rem - 1;
            const int kc = rem ? __builtin_ctz(rem) : -1;
            rem &= rem - 1;
            const int kd = rem ? __builtin_ctz(rem) : -1;
            rem &= rem - 1;
            const u32x8 w0 = flat_rec_uniform(tab, ka), w1 = flat_rec_uniform(tab, kb < 0 ? ka : kb);
            const u32x8 w2 = flat_rec_uniform(tab, kc < 0 ? ka : kc), w3 = flat_rec_uniform(tab, kd < 0 ? ka : kd);
            sstep(w0, ka);
            if (kb >= 0) sstep(w1, kb);
            if (kc >= 0) sstep(w2, kc);
            if (kd >= 0) sstep(w3, kd);
        }
        m <<= (n - 1 - prev) & 31;
        k0 = n;
    }
    for (; k0 + 4 <= n; k0 += 4) {
        const u32x8 w0 = flat_rec_uniform(tab, k0), w1 = flat_rec_uniform(tab, k0 + 1);
        const u32x8 w2 = flat_rec_uniform(tab, k0 + 2), w3 = flat_rec_uniform(tab, k0 + 3);
        step(w0, k0);
        step(w1, k0 + 1);
        step(w2, k0 + 2);
        step(w3, k0 + 3);
    }
#pragma unroll 1
    for (int k = k0; k < n; ++k) step(flat_rec_uniform(tab, k), k);
    if (act) nnode += (uint32_t)((n * (int)sizeof(XFlatLeafDev) + 255) / 256);
    // ---- phase B
    bool go = m != 0;
    if (go) {   // the first candidate: any hit, the lowest bit (the highest leaf, the order of the table's
                // unshifted mask: on the Cornell box it finds an occluder a quarter of an iteration sooner
                // than the reverse); closest hit, the smallest key's leaf (a candidate that begins at
                // infinity has no key: without a keyed one, the lowest bit)
        const int bit = (ANY || e1 == kNone) ? __builtin_ctz(m) : n - 1 - (e1 & 31);
        m &= ~(1u << bit);
        pk = flat_pk_of(pkw, n - 1 - bit);
    }
    while (go) {
        ++nsteps;
        const int cnt = (int)(pk >> 24);
        const XHot* hp = H + (pk & 0xFFFFu);
        if (TRI && fan) {
            // every leaf a fan pair (gi_fan_pair.h): the first record's tv, pv, det and un say which of the
            // two a ray can hit, and the lane runs that one's exact test; the other's is infinity.  Lanes the
            // margins leave undecided (rays through the diagonal, grazing rays) run the other record too.
            const XHotR r0 = load_hot(hp);
            const int ch = fan_pair_choice(r0.h, o, d);
            // (the chosen record read again at the lane's address: assembling it from r0 and the second
            // record's e2 by selects was measured and is slower, C3 2.830-2.841 against 2.821-2.827 ms)
            const XHotR rc = load_hot(hp + (ch == FAN_T2 ? 1 : 0));
            const double ta = x_prim_t<TRI>(rc.h, o, d, MX_TMIN);
            double tq = INFINITY;
            int pq = rc.h.prim;
            if (__builtin_amdgcn_ballot_w64(ch == FAN_BOTH) != 0) {
                if (ch == FAN_BOTH) {
                    const XHotR r1 = load_hot(hp + 1);
                    tq = x_prim_t<TRI>(r1.h, o, d, MX_TMIN);
                    pq = r1.h.prim;
                }
            }
            nprim += 2;   // (records decided)
            if (ANY) {
                if ((ta < tmax) | (tq < tmax)) best = ta < tmax ? rc.h.prim : pq;
            } else {
                const bool ua = (ta < tb) | ((ta == tb) & (rc.h.prim < best));
                tb = ua ? ta : tb;
                best = ua ? rc.h.prim : best;
                const bool uq = (tq < tb) | ((tq == tb) & (pq < best));
                tb = uq ? tq : tb;
                best = uq ? pq : best;
                tbf = up32(tb);
            }
        } else
        for (int j = 0; j < cnt; j += 2) {
            const bool two = j + 1 < cnt;
            const XHotR r0 = load_hot(hp + j), r1 = load_hot(hp + (two ? j + 1 : j));
            const double ta = x_prim_t<TRI>(r0.h, o, d, MX_TMIN);
            const double tq = two ? x_prim_t<TRI>(r1.h, o, d, MX_TMIN) : INFINITY;
            nprim += two ? 2 : 1;
            if (ANY) {
                if ((ta < tmax) | (tq < tmax)) {
                    best = ta < tmax ? r0.h.prim : r1.h.prim;
                    break;
                }
            } else {   // (selects, not branches: | and & do not short-circuit)
                const bool ua = (ta < tb) | ((ta == tb) & (r0.h.prim < best));
                tb = ua ? ta : tb;
                best = ua ? r0.h.prim : best;
                const bool uq = (tq < tb) | ((tq == tb) & (r1.h.prim < best));
                tb = uq ? tq : tb;
                best = uq ? r1.h.prim : best;
                tbf = up32(tb);
            }
        }
        go = false;
        if (ANY) {
            if (best < 0 && m != 0) {
                const int bit = __builtin_ctz(m);
                m &= m - 1;
                pk = flat_pk_of(pkw, n - 1 - bit);
                go = true;
            }
        } else {
            // every other candidate's key is at least e2, so its box begins at flat_key_floor(e2) or
            // later: behind the best t
            if (flat_key_floor(e2) > tbf) m = 0;
            while (m != 0) {
                const int bit = 31 - __builtin_clz(m);   // (the lowest leaf first, as the unshifted mask went)
                m &= ~(1u << bit);
                const int k = n - 1 - bit;
                if (flat_hit(tab + k, no, ivf, tbf, pk, k)) {
                    go = true;
                    break;
                }
            }
        }
    }
    t_out = tb;
    return best;
}

struct WFArgs {
    const unsigned* list;      // k_x_classify's work list (pixel slots, tile order)
    const unsigned* n_list;    // its length (device)
    double* part;              // per-sample radiance rows (spp > 1)
    unsigned* take;            // this bounce's input entries handed out (device counter)
    const unsigned* n_in;      // this bounce's input length (bounce > 0: the previous bounce's n_out)
    unsigned* n_out;           // entries appended to qout
    unsigned long long u0, u1; // bounce 0: the chunk's units [u0, u1) of n_list * ns
    unsigned s0, ns;           // the launch's samples [s0, s0 + ns) of the spp (0, spp; or a progressive pass)
};

// The scene views of a bounce / segment kernel.  LDS (sc.x_lds_bytes > 0): the workgroup stages the
// traversal records (wide nodes, leaf records) and the shading records (primitives, entities) at the
// start of its dynamic LDS, so neither the traversal nor the shading issues a global load; then the
// per-lane path slots.
// HBM-resident scenes: the per-lane level stack (16 x 256 ints), then the path slots.
struct WFView {
    const XWNode* LW = nullptr;
    const XHot* LH = nullptr;
    const XPrim* XP = nullptr;
    const REnt* EN = nullptr;
    const XFlatLeafDev* FT = nullptr;   // the flat leaf table phase A reads
    const uint32_t* FP = nullptr;    // FLAT: per leaf its (offset, index, count) word, in LDS (flat_pk_of)
    int* nst = nullptr;
    double* pl = nullptr;   // this lane's L (fields 0-2) and T (3-5), pl[f * 256]
};
template <bool LDS, bool FLAT = false>
__device__ __forceinline__ WFView wf_stage(const DevScene& sc, int4* lds) {
    WFView v;
    v.XP = sc.xprims;
    v.EN = sc.ents;
    v.FT = sc.xflat;
    if constexpr (LDS) {
        // (FLAT: no kernel's flat query reads the wide nodes -- not staged, not counted by wf_lds_bytes)
        const int nw = FLAT ? 0 : sc.n_xwnodes * (int)(sizeof(XWNode) / sizeof(int4));
        const int nh = sc.n_xhot * (int)(sizeof(XHot) / sizeof(int4));
        const int np = sc.n_xprims * (int)(sizeof(XPrim) / sizeof(int4));
        const int ne = sc.n_ents * (int)(sizeof(REnt) / sizeof(int4));
        const int4* gw = reinterpret_cast<const int4*>(sc.xwnodes);
        const int4* gh = reinterpret_cast<const int4*>(sc.xhot);
        const int4* gp = reinterpret_cast<const int4*>(sc.xprims);
        const int4* ge = reinterpret_cast<const int4*>(sc.ents);
        for (int i = threadIdx.x; i < nw; i += blockDim.x) lds[i] = gw[i];
        for (int i = threadIdx.x; i < nh; i += blockDim.x) lds[nw + i] = gh[i];
        for (int i = threadIdx.x; i < np; i += blockDim.x) lds[nw + nh + i] = gp[i];
        for (int i = threadIdx.x; i < ne; i += blockDim.x) lds[nw + nh + np + i] = ge[i];
        // FLAT: the leaves' candidate words behind the entities (kFlatPkBytes, counted by wf_lds_bytes)
        constexpr int nk = FLAT ? (int)(kFlatPkBytes / sizeof(int4)) : 0;
        if constexpr (FLAT) {
            uint32_t* pkw = reinterpret_cast<uint32_t*>(lds + nw + nh + np + ne);
            for (int i = threadIdx.x; i < sc.n_xflat; i += blockDim.x) pkw[i] = flat_pack((uint32_t)sc.xflat[i].off, i, (uint32_t)sc.xflat[i].cnt);
            v.FP = pkw;
        }
        __syncthreads();
        if constexpr (!FLAT) v.LW = reinterpret_cast<const XWNode*>(lds);
        v.LH = reinterpret_cast<const XHot*>(lds + nw);
        v.XP = reinterpret_cast<const XPrim*>(lds + nw + nh);
        v.EN = reinterpret_cast<const REnt*>(lds + nw + nh + np);
        v.pl = reinterpret_cast<double*>(lds + nw + nh + np + ne + nk) + threadIdx.x;
    } else {
        v.nst = reinterpret_cast<int*>(lds) + threadIdx.x;   // 16 levels x 256 lanes
        v.pl = reinterpret_cast<double*>(reinterpret_cast<int*>(lds) + 16 * 256) + threadIdx.x;
    }
    return v;
}

// The unit (work-list index li, sample smp) of a pixel's sample: its pixel, RNG key and primary
// direction (the reference's corner ray, jittered for spp > 1).  idx: the output slot (the
// per-sample radiance row for spp > 1, else the pixel).
__device__ __forceinline__ V3 wf_primary(const CamDev& cam, const TileMap& m, unsigned ps, int spp, uint64_t seed,
                                         unsigned li, unsigned smp, long long& idx, uint64_t& key) {
    int x = 0, y = 0;   // ps: the work list's entry li (the pixel slot)
    slot_pixel(m, (long long)(ps >> 6), (int)(ps & 63), idx, x, y);
    y += m.y0;
    if (spp > 1) idx = (long long)li;
    key = mx_key(seed, (uint64_t)y * (uint64_t)m.w + (uint64_t)x);
    double jx = 0.0, jy = 0.0;
    if (spp > 1) {
        jx = mx_u01k(key, smp, 0xFFFF, 0);
        jy = mx_u01k(key, smp, 0xFFFF, 1);
    }
    return primary_dir(cam, (double)x + jx, (double)y + jy);
}
// conservative fp32 test of the scene's root box on the unnormalised primary direction: a miss adds
// exactly +0 (the oracle traces it and adds L = 0)
__device__ __forceinline__ bool wf_primary_misses(const DevScene& sc, const CamDev& cam, V3 d0) {
    const F3 iv0 = f3(__builtin_amdgcn_rcpf((float)d0.x), __builtin_amdgcn_rcpf((float)d0.y), __builtin_amdgcn_rcpf((float)d0.z));
    return !root_hit(sc, ray_org32(cam.pos, d0, ray_far_r(sc, cam.pos)), iv0);   // (a far camera: tested from near the scene)
}
// the path's radiance once it ends: its per-sample row (spp > 1; k_x_reduce adds a pixel's rows in
// sample order) or, with one sample, the pixel: min((0 + L) / 1, 1), the reduce pass's operations
__device__ __forceinline__ void wf_store(double* part, double* rgb, uint8_t* rgb8, int spp, long long idx, unsigned smp, V3 L) {
    if (spp > 1) {
        double* q = part + 3 * ((size_t)idx * (size_t)spp + (size_t)smp);
        q[0] = L.x; q[1] = L.y; q[2] = L.z;
    } else {
        const double c0 = smin((0.0 + L.x) / 1.0, 1.0), c1 = smin((0.0 + L.y) / 1.0, 1.0), c2 = smin((0.0 + L.z) / 1.0, 1.0);
        if (rgb) { rgb[3 * idx] = c0; rgb[3 * idx + 1] = c1; rgb[3 * idx + 2] = c2; }
        if (rgb8) quantize(c0, c1, c2, rgb8 + 3 * idx);
    }
}

// One path segment, bounce b (every lane of the wave runs the same sequence): closest hit -> hit
// point and light direction -> shadow any-hit -> texture and Blinn-Phong with the shadow answer ->
// L += T * local -> the next direction (mirror with probability refl, else T *= texel / 2 and a
// cosine-weighted direction).  The oracle's operations (sample_mode_x).  In: o, d and (in the lane's
// path slot) the path's L and T.  Out: true when the path continues (o, d set to its next ray; L, T in
// registers and in the slot); false when it ends (L final).
// STATS: the wave's traversal-loop iterations (closest, shadow) and the lanes' own steps, summed into
// ws (lane 0) -- the divergence profile of a segment
struct WFSegStats {
    uint64_t it_c = 0, ln_c = 0, it_s = 0, ln_s = 0, segs = 0, live = 0, iters = 0;
    uint64_t cyc_c = 0, cyc_s = 0, cyc_sh = 0, cyc_ref = 0, cyc_all = 0;   // wave clock cycles per phase
};
__device__ __forceinline__ void wf_wave_steps(uint32_t n, uint64_t& it, uint64_t& ln) {
    uint32_t mx = n, sm = n;
    for (int off = 32; off > 0; off >>= 1) {
        mx = max(mx, (uint32_t)__shfl_xor(mx, off));
        sm += __shfl_xor(sm, off);
    }
    if ((threadIdx.x & 63) == 0) { it += mx; ln += sm; }
}
// A segment's query in the kernel variant's form -- the flat leaf table, or the tree walk over the nodes
// staged in LDS, the quantised nodes or the wide nodes in HBM: the one place that chooses.  ANY: the
// shadow any-hit before tmax, else the closest hit.  skip: the ray's own plane group (254: none; the
// quantised nodes carry no groups).
template <bool ANY, bool LDS, bool SH, bool TRI, bool CN, bool FLAT>
__device__ __forceinline__ int x_query(const DevScene& sc, const WFView& v, float far_r, const V3& o, const V3& d, double tmax,
                                       bool act, double& t_out, uint32_t& nnode, uint32_t& nprim, uint32_t& st_steps, int skip,
                                       uint32_t live = ~0u) {
    if constexpr (FLAT) return wf_flat<ANY, TRI>(far_r, v.FT, v.FP, sc.n_xflat, v.LH, o, d, tmax, act, t_out, nnode, nprim, st_steps, skip, sc.x_fan != 0, live);
    else if constexpr (LDS) return wf_trace<ANY, true, false, SH, TRI, false>(far_r, v.LW, v.LH, o, d, tmax, act, v.nst, t_out, nnode, nprim, st_steps, skip);
    else if constexpr (CN) return wf_trace<ANY, false, false, SH, TRI, true>(far_r, sc.xcnodes, sc.xhot, o, d, tmax, act, v.nst, t_out, nnode, nprim, st_steps);
    else return wf_trace<ANY, false, false, SH, TRI, true>(far_r, sc.xwnodes, sc.xhot, o, d, tmax, act, v.nst, t_out, nnode, nprim, st_steps, skip);
}
// The own-plane skip of a ray that leaves a surface of plane group pg (254: none) and normal pn along
// dir: the group, when the ray is steep enough that the exact tests of the group's primitives would
// all find t below MX_TMIN (gi_build.cpp assign_plane_groups; skip_cos: gi_dev.h x_skip_cos), else 254.
__device__ __forceinline__ int x_own_plane(int pg, const V3& pn, const V3& dir, double skip_cos) {
    return (pg < 254 && fabs(dot(dir, pn)) >= skip_cos) ? pg : 254;
}
// The frame of a closest hit (prim best at t along o + t d): the point P, the direction Ld and distance
// ldist to the point light, the primitive's plane group pg and normal pn -- the shadow ray and the
// next ray leave that plane.  Without a hit: P = o and values that skip nothing.
struct XHitFrame { V3 P, Ld, pn; double ldist; int pg; };
__device__ __forceinline__ XHitFrame x_hit_frame(const WFView& v, const V3& light, const V3& o, const V3& d, bool hit, int best, double t) {
    XHitFrame h{o, v3(0, 0, 1), v3(0, 0, 1), 0.0, 254};
    if (hit) {
        h.P = o + t * d;
        const V3 lv = light - h.P;
        h.ldist = gsqrt(dot(lv, lv));
        h.Ld = normalize(lv);
        const XPrim& px = v.XP[best];
        h.pg = px.pad[0] < 254 ? px.pad[0] : 254;
        h.pn = ld3(px.n);
    }
    return h;
}

template <bool STATS, bool LDS, bool SH, bool TRI, bool CN, bool FLAT, typename KeyF>
__device__ __forceinline__ bool x_segment(const DevScene& sc, const WFView& v, const V3& light, int depth, bool no_shadow, bool act,
                                          const KeyF& id_of, V3& o, V3& d, V3& L, V3& T,
                                          uint32_t& nnode, uint32_t& nprim, uint32_t& nrays, WFSegStats& ws,
                                          double skip_cos = 2.0, int* splane = nullptr, float far_r = INFINITY, uint32_t live = ~0u) {
    uint32_t st_steps = 0;
    uint64_t c0 = STATS ? clock64() : 0;
    bool occl = false;
    // ---- closest hit
    double tbest = INFINITY;
    // the own-plane skip of this ray (k_seg carries it from the previous segment; 254: none).  Only the
    // low kSegPlaneBits of *splane are the plane: k_seg keeps its bounce index above them.  (Unpacking
    // the plane in k_seg around this call instead was compiled: k_seg<false,true,true,false,true,false,
    // false,false> then takes 84 B of scratch against 68 B, above the 76 B it had before the ring)
    const int skip_c = splane ? (*splane & kSegPlaneMask) : 254;
    const int best = x_query<false, LDS, SH, TRI, CN, FLAT>(sc, v, far_r, o, d, INFINITY, act, tbest, nnode, nprim, st_steps, skip_c);
    if (act) ++nrays;
    if (STATS) {
        wf_wave_steps(st_steps, ws.it_c, ws.ln_c);
        st_steps = 0;
        const uint64_t c1 = clock64();
        ws.cyc_c += c1 - c0;
        c0 = c1;
    }
    const bool hit = act && best >= 0;
    // ---- the hit point and its shadow ray toward the point light
    const XHitFrame h = x_hit_frame(v, light, o, d, hit, best, tbest);
    const V3 &P = h.P, &Ld = h.Ld;
    if (!no_shadow) {
        double tdummy;
        const int skip_s = x_own_plane(h.pg, h.pn, Ld, skip_cos);
        occl = x_query<true, LDS, SH, TRI, CN, FLAT>(sc, v, INFINITY, P, Ld, h.ldist, hit, tdummy, nnode, nprim, st_steps, skip_s, live) >= 0;
        if (STATS) wf_wave_steps(st_steps, ws.it_s, ws.ln_s);
    }
    if (STATS) {
        const uint64_t c1 = clock64();
        ws.cyc_s += c1 - c0;
        c0 = c1;
    }
    {   // every lane: a lane without a path never uses them, so L and T are dead during
        L = v3(v.pl[0], v.pl[256], v.pl[512]);      // the traversals (conditioned on act, the register copies
        T = v3(v.pl[768], v.pl[1024], v.pl[1280]);  // stayed live for inactive lanes and were spilled)
    }
    // ---- shading (local = ambient, + diffuse + specular when lit)
    bool cont = false;
    if (hit) {
        ++nrays;   // the shadow ray
        const XPrim& p = v.XP[best];   // the facing normal (after the shadow ray: fewer live values)
        V3 N = (TRI || p.kind == 0) ? ld3(p.n) : normalize(P - ld3(p.a));
        N = dot(d, N) < 0 ? N : -N;
        const REnt& e = v.EN[p.ent];
        const V3 tc = x_texel<TRI>(sc, e, P);
        const V3 la = tc * e.shader[0];
        V3 loc = la;
        if (!occl) {
            const V3 ldf = (smax(0.0, dot(N, Ld)) * (tc * 0.5)) * e.shader[1];
            const V3 bis = normalize(normalize(-d) + Ld);
            const double spw = mx_pow(smax(0.0, dot(N, bis)), e.spec_pow);
            const V3 ls = v3(spw, spw, spw) * e.shader[2];
            loc = (la + ldf) + ls;
        }
        L = L + vmul(T, v3(smin(loc.x, 1.0), smin(loc.y, 1.0), smin(loc.z, 1.0)));
        const PathId id = id_of();   // (k_seg: from the lane's slot)
        const uint64_t key = id.key;
        const unsigned smp = id.smp;
        const int b = id.b;
        if (b != depth - 1) {
            if (e.refl > 0.0 && mx_u01k(key, smp, b, 4) < e.refl) {   // mirror: T unchanged
                d = normalize(d - N * (2.0 * dot(d, N)));
                cont = true;
            } else {
                T = vmul(T, tc * 0.5);
                if (!((T.x == 0.0) & (T.y == 0.0) & (T.z == 0.0))) {
                    double sx, sy, r2;   // concentric disk + Malley
                    mx_disk(mx_u01k(key, smp, b, 2), mx_u01k(key, smp, b, 3), sx, sy, r2);
                    const double sz = gsqrt(1.0 - r2);
                    const double sg = N.z >= 0.0 ? 1.0 : -1.0;   // Duff et al. 2017 basis
                    const double aa = -1.0 / (sg + N.z);
                    const double bb = N.x * N.y * aa;
                    const V3 bt1 = v3(1.0 + sg * N.x * N.x * aa, sg * bb, -sg * N.x);
                    const V3 bt2 = v3(bb, sg + N.y * N.y * aa, -N.y);
                    d = normalize((bt1 * sx + bt2 * sy) + N * sz);
                    cont = true;
                }
            }
            o = P;
        }
        if (cont) {
            v.pl[0] = L.x; v.pl[256] = L.y; v.pl[512] = L.z;
            v.pl[768] = T.x; v.pl[1024] = T.y; v.pl[1280] = T.z;
            if (splane) *splane = (*splane & ~kSegPlaneMask) | x_own_plane(h.pg, h.pn, d, skip_cos);
        }
    }
    if (STATS) ws.cyc_sh += clock64() - c0;
    return cont;
}

// One bounce of every live path (the wavefront form).  Persistent grid: each wave takes GI_WF_TAKE
// batches of 64 queue entries per atomic until the queue is exhausted.
template <bool STATS, bool LDS, bool W4, bool SH, bool TRI, bool CN, bool FLAT>
__global__ __launch_bounds__(256, (LDS && W4) ? GI_WF_MIN_WAVES_LDS : GI_WF_MIN_WAVES) void k_wf_bounce(
    DevScene sc, CamDev cam, V3 light, TileMap m, int spp, int depth, uint64_t seed, int b, double* rgb, uint8_t* rgb8,
    unsigned long long* stats, WFArgs a, WFQ qin, WFQ qout, int xflags, uint32_t shadow_live) {
    // the bounce's input length: bounce 0, the chunk's units of the work list; else the queue
    unsigned n_in;
    if (b == 0) {
        const unsigned long long tot = (unsigned long long)*a.n_list * (unsigned long long)a.ns;
        n_in = (unsigned)(min(tot, a.u1) > a.u0 ? min(tot, a.u1) - a.u0 : 0ull);
    } else {
        n_in = *a.n_in;
    }
    if (*(volatile unsigned*)a.take >= n_in) return;   // nothing left (before staging the scene)
    extern __shared__ int4 lds_dyn[];
    const WFView v = wf_stage<LDS, FLAT>(sc, lds_dyn);
    const bool no_shadow = (xflags & XF_NO_SHADOW) != 0;
    const int lane = threadIdx.x & 63;
    uint32_t nnode = 0, nprim = 0, nrays = 0, nres = 0, npx = 0;
    const long long qc = qin.cap, oc = qout.cap;
    // batches per atomic: up to GI_WF_TAKE, fewer when the queue has fewer than about 8 runs per
    // resident wave (small queues: every wave gets work)
    const unsigned take = (unsigned)max(1u, min((unsigned)GI_WF_TAKE, n_in / (64u * 8u * (gridDim.x * (blockDim.x >> 6)))));
    unsigned base = 0, left = 0;   // the wave's current run of take x 64 entries
    for (;;) {
        if (left == 0) {
            if (lane == 0) base = atomicAdd(a.take, 64u * take);
            base = __shfl(base, 0);
            left = take;
        }
        if (base >= n_in) break;
        const unsigned j = base + (unsigned)lane;
        base += 64u;
        --left;
        bool act = j < n_in;
        unsigned li = 0, smp = 0;
        V3 o = cam.pos, d = v3(1, 0, 0), L = v3(0, 0, 0), T = v3(1, 1, 1);
        long long idx = -1;
        uint64_t key = 0;
        if (act) {
            if (b == 0) {
                const unsigned long long u = a.u0 + j;
                if (u < (1ull << 32)) {   // 32-bit division where it suffices
                    li = (unsigned)u / a.ns;
                    smp = a.s0 + ((unsigned)u - li * a.ns);
                } else {
                    li = (unsigned)(u / (unsigned long long)a.ns);
                    smp = a.s0 + (unsigned)(u - (unsigned long long)li * (unsigned long long)a.ns);
                }
            } else {
                const uint2 id = qin.id[j];
                li = id.x;
                smp = id.y;
                const double* r = qin.r + j;
                o = v3(r[0], r[qc], r[2 * qc]);
                d = v3(r[3 * qc], r[4 * qc], r[5 * qc]);
                L = v3(r[6 * qc], r[7 * qc], r[8 * qc]);
                T = v3(r[9 * qc], r[10 * qc], r[11 * qc]);
            }
            const V3 d0 = wf_primary(cam, m, a.list[li], spp, seed, li, smp, idx, key);
            if (b == 0) {   // the unit's primary ray
                if (smp == 0) ++npx;
                if (wf_primary_misses(sc, cam, d0)) {
                    ++nrays;
                    ++nres;
                    act = false;
                    wf_store(a.part, rgb, rgb8, spp, idx, smp, v3(0, 0, 0));
                } else {
                    d = normalize(d0);
                }
            }
            v.pl[0] = L.x; v.pl[256] = L.y; v.pl[512] = L.z;
            v.pl[768] = T.x; v.pl[1024] = T.y; v.pl[1280] = T.z;
        }
        WFSegStats ws;
        // (the queue carries no plane: the closest ray is not skipped here, the shadow ray is)
        const double skip_cos = x_skip_cos(sc, cam.pos);
        const float far_r = ray_far_r(sc, cam.pos);   // (far cameras: gi_dev.h ray_org32)
        int splane = 254;
        const bool cont = x_segment<false, LDS, SH, TRI, CN, FLAT>(sc, v, light, depth, no_shadow, act, [&] { return PathId{key, smp, b}; }, o, d, L, T,
                                                             nnode, nprim, nrays, ws, skip_cos, &splane, far_r, shadow_live);
        // ---- live paths to the next bounce's queue: one atomic per wave, entries in lane order
        const unsigned long long mc = __ballot(cont);
        if (mc) {
            const int leader = __ffsll((long long)mc) - 1;
            unsigned ob = 0;
            if (lane == leader) ob = atomicAdd(a.n_out, (unsigned)__popcll(mc));
            ob = __shfl(ob, leader);
            if (cont) {
                const unsigned k = ob + (unsigned)__popcll(mc & ((1ull << lane) - 1));
                qout.id[k] = make_uint2(li, smp);
                double* r = qout.r + k;
                r[0] = o.x; r[oc] = o.y; r[2 * oc] = o.z;
                r[3 * oc] = d.x; r[4 * oc] = d.y; r[5 * oc] = d.z;
                r[6 * oc] = L.x; r[7 * oc] = L.y; r[8 * oc] = L.z;
                r[9 * oc] = T.x; r[10 * oc] = T.y; r[11 * oc] = T.z;
            }
        }
        if (act && !cont) wf_store(a.part, rgb, rgb8, spp, idx, smp, L);
    }
    if (STATS) {
        wave_add_stats(stats, nrays, nnode, nprim, npx);
        uint64_t r = nres;
        for (int off = 32; off > 0; off >>= 1) r += __shfl_xor(r, off);
        if (lane == 0 && r) atomicAdd(stats + GI_STAT_X_RESOLVED, (unsigned long long)r);
    }
}

// The segment-synchronous form (SEG): one persistent kernel in which every loop iteration is one
// whole path segment (x_segment) for every lane of the wave -- the wavefront form's uniform per-lane
// sequence, with the path state kept in registers / the lane's LDS slot instead of HBM queues, and
// no launch per bounce.  A lane whose path ends takes the next (pixel, sample) unit at the top of
// the next iteration (units handed out from the wave's run, one atomic per run);
// primary rays that miss the scene's root box are resolved there, up to GI_SEG_BURST per lane.
#ifndef GI_SEG_BURST
#define GI_SEG_BURST 16
#endif
#ifndef GI_SEG_TAKE
#define GI_SEG_TAKE 2       // k_seg: most batches of 64 units per run (one atomic per run)
#endif
#ifndef GI_SEG_TAKE_TRI
#define GI_SEG_TAKE_TRI 1   // the same for LDS-resident triangle-only scenes (the Cornell box)
#endif
// Unit u of a k_seg launch, made: its work-list entry and sample, its primary ray (wf_primary), the
// root-box pretest (wf_primary_misses).  A miss is resolved here -- its zero row stored -- and false
// returned; else what a lane needs to trace the unit's path: d = normalize(d0), the RNG key and the word
// of slot field 7 (idx | smp << 32; idx < 2^32: work-list index or pixel).  Both refill paths of k_seg
// call it: the one statement of a unit's ray.  The STATS counters count where a unit is made.
struct SegRay {
    V3 d;
    uint64_t key, is;
};
__device__ __forceinline__ bool seg_make_unit(const DevScene& sc, const CamDev& cam, const TileMap& m, const WFArgs& a, int spp,
                                              uint64_t seed, double* rgb, uint8_t* rgb8, unsigned long long u, SegRay& r,
                                              uint32_t& nrays, uint32_t& nres, uint32_t& npx) {
    unsigned li, smp;
    if (u < (1ull << 32)) {   // 32-bit division where it suffices
        li = (unsigned)u / a.ns;
        smp = a.s0 + ((unsigned)u - li * a.ns);
    } else {
        li = (unsigned)(u / (unsigned long long)a.ns);
        smp = a.s0 + (unsigned)(u - (unsigned long long)li * (unsigned long long)a.ns);
    }
    const unsigned ps = a.list[li];   // (prefetching a run's entries into lanes: +3%, round 4)
    long long idx = -1;
    const V3 d0 = wf_primary(cam, m, ps, spp, seed, li, smp, idx, r.key);
    if (smp == 0) ++npx;
    if (wf_primary_misses(sc, cam, d0)) {
        ++nrays;
        ++nres;
        wf_store(a.part, rgb, rgb8, spp, idx, smp, v3(0, 0, 0));
        return false;
    }
    r.d = normalize(d0);
    r.is = (uint64_t)(uint32_t)idx | ((uint64_t)smp << 32);
    return true;
}
// this lane's rank among the lanes of a wave mask: the mask's bits below the lane (mbcnt: no lane mask
// held in two VGPRs -- every k_seg variant came out two VGPRs lower)
__device__ __forceinline__ unsigned seg_rank(unsigned long long mask) {
    return __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
}
// a 64-bit value of lane 0 as a wave-uniform one (scalar registers)
__device__ __forceinline__ unsigned long long seg_uniform64(unsigned long long v) {
    const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32));
    return ((unsigned long long)hi << 32) | lo;
}

// RING (launches with XF_SEG_RING: the host's choice per scene, gi_kernels.hip x_launch_config): lanes
// without a path take prepared primary rays from the wave's ring, generated a batch of 64 units at a
// time by all 64 lanes.  Without it they make their units themselves, under the need
// mask.  The launch's dynamic LDS carries kSegRingBytes behind the path slots only with RING.  (A
// template parameter: as a run-time choice in one kernel the Cornell box's variant took 12 B of scratch.)
// shadow_live: the table leaves the launch's shadow queries visit (gi_scene.h x_shadow_live; all ones: every
// leaf).  The last argument, in the four bytes behind xflags that were padding: as a field of WFArgs it moved
// the arguments behind it, and the kernels without the flat query compiled to other instructions.
template <bool STATS, bool LDS, bool W4, bool SH, bool TRI, bool CN, bool FLAT, bool RING>
__global__ __launch_bounds__(256, (LDS && W4) ? GI_WF_MIN_WAVES_LDS : GI_WF_MIN_WAVES) void k_seg(
    DevScene sc, CamDev cam, V3 light, TileMap m, int spp, int depth, uint64_t seed, double* rgb, uint8_t* rgb8,
    unsigned long long* stats, WFArgs a, int xflags, uint32_t shadow_live) {
    extern __shared__ int4 lds_dyn[];
    const WFView v = wf_stage<LDS, FLAT>(sc, lds_dyn);
    const bool no_shadow = (xflags & XF_NO_SHADOW) != 0;
    const int lane = threadIdx.x & 63;
    const unsigned long long total = (unsigned long long)*a.n_list * (unsigned long long)a.ns;
    // run length: up to GI_SEG_TAKE batches of 64 units per atomic (background-heavy frames burn units
    // fast: longer runs, fewer atomics on the one counter), fewer when the launch has less than about
    // 8 runs per resident wave (small launches: every wave gets work).  Round 5, after the spill fix
    // (profiles/r05_ab.txt): 4 -> 2 batches gives C3 5.09 -> 4.95 ms and X-zoo 4.35-4.43 -> 4.17-4.19,
    // X-main and the 1k soup unchanged; 1 batch gives C3 4.89-4.90 but X-main 0.38 -> 0.69 and X-zoo
    // 4.67 (their frames are background-heavy or shading-heavy), so 1 only for LDS-resident
    // triangle-only scenes.  Guided self-scheduling -- run sizes from a relaxed read of the counter --
    // measured 1.2-2.6x slower (the read waits behind the atomics on that L2 line).
    constexpr long long kTake = (LDS && TRI) ? GI_SEG_TAKE_TRI : GI_SEG_TAKE;
    const unsigned long long n_waves = (unsigned long long)gridDim.x * (blockDim.x >> 6);
    const unsigned long long run = 64ull * (unsigned long long)max(1ll, min(kTake, (long long)(total / (64ull * 8ull * n_waves))));
    uint32_t nnode = 0, nprim = 0, nrays = 0, nres = 0, npx = 0;
    SegUnits su;         // the wave's units and its ring's fill (gi_seg_ring.h; uniform)
    bool live = false;   // this lane carries a path
    V3 o = cam.pos, d = v3(1, 0, 0), L = v3(0, 0, 0), T = v3(1, 1, 1);
    int splane = 254;   // the own-plane skip of the lane's next ray (254: none; primary rays) | bounce << kSegPlaneBits
    // the wave's ring: plane f of entry j at rq[f * 64 + j] (behind the workgroup's path slots)
    uint64_t* const rq = reinterpret_cast<uint64_t*>(v.pl - threadIdx.x + kWfSlotBytes / sizeof(double)) +
                         (threadIdx.x >> 6) * (kSegRingPlanes * kSegBatch);
    // a lane's path begins: the ray and the slot of bounce 0
    auto begin_path = [&](const V3& dir, uint64_t key, uint64_t is) {
        live = true;
        o = cam.pos;
        d = dir;
        splane = 254;
        L = v3(0, 0, 0);
        T = v3(1, 1, 1);
        v.pl[0] = 0.0; v.pl[256] = 0.0; v.pl[512] = 0.0;
        v.pl[768] = 1.0; v.pl[1024] = 1.0; v.pl[1280] = 1.0;
        slot_put_u64(v.pl, 6, key);
        slot_put_u64(v.pl, 7, is);
    };
    // (gi_build.cpp assign_plane_groups: the bound on |d . n| above which a surface's own plane is skipped)
    const double skip_cos = x_skip_cos(sc, cam.pos);
    const float far_r = ray_far_r(sc, cam.pos);   // (far cameras: gi_dev.h ray_org32)
    WFSegStats ws;
    const uint64_t t_begin = STATS ? clock64() : 0;
    for (;;) {
        if (STATS && lane == 0) ++ws.iters;
        const uint64_t t_ref = STATS ? clock64() : 0;
        // ---- lanes without a path take units (primary rays; background samples resolved here)
        for (int burst = 0; burst < GI_SEG_BURST; ++burst) {
            const unsigned long long m_need = __ballot(!live);
            if (m_need == 0 || su.done()) break;
            const unsigned rank = seg_rank(m_need);
            const unsigned n_need = (unsigned)__popcll(m_need);
            if constexpr (RING) {
                if (su.wants_batch(n_need)) {   // the ring is empty: all 64 lanes make the run's next batch
                    if (su.wants_run()) {
                        unsigned long long nb = 0;
                        if (lane == 0) nb = atomicAdd(reinterpret_cast<unsigned long long*>(a.take), run);
                        su.give_run(seg_uniform64(nb), run, total);
                    }
                    unsigned long long first = 0;
                    const unsigned n_batch = su.take_batch(first);
                    if (n_batch != 0) {
                        // (the ring is the wave's own: no workgroup barrier, whose waves are in different
                        // iterations.  The wave's lanes run in lockstep and its LDS operations complete in
                        // order; the fences keep the compiler from moving the ring's writes over the
                        // earlier pops' reads, and the pops' reads over the writes)
                        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                        SegRay r{};
                        bool hit = false;
                        if ((unsigned)lane < n_batch) hit = seg_make_unit(sc, cam, m, a, spp, seed, rgb, rgb8, first + (unsigned)lane, r, nrays, nres, npx);
                        const unsigned long long m_hit = __ballot(hit);
                        if (hit) {   // entries in lane order of the hits: j < 64
                            uint64_t* e = rq + seg_rank(m_hit);
                            e[0] = (uint64_t)__double_as_longlong(r.d.x);
                            e[kSegBatch] = (uint64_t)__double_as_longlong(r.d.y);
                            e[2 * kSegBatch] = (uint64_t)__double_as_longlong(r.d.z);
                            e[3 * kSegBatch] = r.key;
                            e[4 * kSegBatch] = r.is;
                        }
                        su.push((unsigned)__popcll(m_hit));
                        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                        __builtin_amdgcn_wave_barrier();
                    }
                }
                // lanes without a path take entries by their rank among such lanes
                unsigned first_e = 0;
                const unsigned k = su.pop(n_need, first_e);
                if (!live && rank < k) {   // first_e + rank < 64: the popped entries were pushed
                    const uint64_t* e = rq + (first_e + rank);
                    begin_path(v3(__longlong_as_double((long long)e[0]), __longlong_as_double((long long)e[kSegBatch]),
                                  __longlong_as_double((long long)e[2 * kSegBatch])),
                               e[3 * kSegBatch], e[4 * kSegBatch]);
                }
                continue;
            }
            // ---- the direct path: the lanes make their own units, under the need mask
            unsigned long long u = ~0ull;
            const unsigned long long avail = su.cur_end - su.cur;
            if (n_need > avail && !su.exhausted) {   // a new run of units for the lanes beyond it
                unsigned long long nb = 0;
                if (lane == 0) nb = atomicAdd(reinterpret_cast<unsigned long long*>(a.take), run);
                nb = seg_uniform64(nb);
                if (nb >= total) {
                    su.exhausted = true;
                    if (!live && rank < avail) u = su.cur + rank;
                    su.cur = su.cur_end;
                } else {
                    const unsigned long long ne = min(total, nb + run);
                    if (!live) {
                        if (rank < avail) u = su.cur + rank;
                        else if (nb + (rank - avail) < ne) u = nb + (rank - avail);
                    }
                    su.cur = min(ne, nb + (n_need - avail));
                    su.cur_end = ne;
                    if (ne == total) su.exhausted = true;
                }
            } else {
                if (!live && rank < avail) u = su.cur + rank;
                su.cur += min((unsigned long long)n_need, avail);
            }
            if (!live && u != ~0ull) {
                SegRay r{};
                if (seg_make_unit(sc, cam, m, a, spp, seed, rgb, rgb8, u, r, nrays, nres, npx)) begin_path(r.d, r.key, r.is);
            }
        }
        if (STATS) ws.cyc_ref += clock64() - t_ref;
        if (__ballot(live) == 0) {
            if (su.done()) break;
            continue;
        }
        // ---- one segment of every live path
        if (STATS) {
            const unsigned long long ml = __ballot(live);
            if (lane == 0) { ++ws.segs; ws.live += __popcll(ml); }
        }
        const bool cont = x_segment<STATS, LDS, SH, TRI, CN, FLAT>(
            sc, v, light, depth, no_shadow, live,
            [&] { return PathId{slot_get_u64(v.pl, 6), (unsigned)(slot_get_u64(v.pl, 7) >> 32), splane >> kSegPlaneBits}; },
            o, d, L, T, nnode, nprim, nrays, ws, skip_cos, &splane, far_r, shadow_live);
        if (live) {
            if (cont) {
                splane += 1 << kSegPlaneBits;   // the next bounce
            } else {
                const uint64_t is = slot_get_u64(v.pl, 7);
                wf_store(a.part, rgb, rgb8, spp, (long long)(uint32_t)is, (unsigned)(is >> 32), L);
                live = false;
            }
        }
    }
    if (STATS && lane == 0) {   // the segment divergence profile (bench "schedule")
        atomicAdd(stats + GI_STAT_X_ITERS, (unsigned long long)ws.iters);
        atomicAdd(stats + GI_STAT_X_HANDLE, (unsigned long long)ws.segs);
        atomicAdd(stats + GI_STAT_X_HLANES, (unsigned long long)ws.live);
        atomicAdd(stats + GI_STAT_X_IT_LEAF, (unsigned long long)ws.it_c);
        atomicAdd(stats + GI_STAT_X_LN_LEAF, (unsigned long long)ws.ln_c);
        atomicAdd(stats + GI_STAT_X_IT_NODE, (unsigned long long)ws.it_s);
        atomicAdd(stats + GI_STAT_X_LN_NODE, (unsigned long long)ws.ln_s);
        atomicAdd(stats + GI_STAT_X_CYC_TRAV, (unsigned long long)(ws.cyc_c + ws.cyc_s));
        atomicAdd(stats + GI_STAT_X_IT_RS, (unsigned long long)ws.cyc_c);   // (k_seg: closest-trace cycles)
        atomicAdd(stats + GI_STAT_X_CYC_HIT, (unsigned long long)ws.cyc_sh);
        atomicAdd(stats + GI_STAT_X_CYC_NEXT, (unsigned long long)ws.cyc_ref);
        atomicAdd(stats + GI_STAT_X_CYC_ALL, (unsigned long long)(clock64() - t_begin));
    }
    if (STATS) {
        wave_add_stats(stats, nrays, nnode, nprim, npx);
        uint64_t r = nres;
        for (int off = 32; off > 0; off >>= 1) r += __shfl_xor(r, off);
        if (lane == 0 && r) atomicAdd(stats + GI_STAT_X_RESOLVED, (unsigned long long)r);
    }
}

// Known-answer hook (gi_kat_x_query; tests): the three queries of one path segment, one ray per
// lane, through x_segment's own helpers (x_query, x_hit_frame, x_own_plane, x_skip_cos) and k_seg's
// staging, so a test sees the (t, primitive) answers themselves.  Record i: o, d, light, d2 (12 doubles).
// The closest hit of (o, d) without a skip; from its point P the any-hit query toward the light and the
// closest hit of (P, d2), each with the own-plane skip.  Lanes past n run the queries
// without a ray.  oi[5 i ..]: prim1, occl (-1 without a hit), skip_s, prim2, skip2; od[2 i ..]:
// t1, t2; od[2 n]: the launch's skip_cos.
template <bool LDS, bool W4, bool SH, bool TRI, bool CN, bool FLAT>
__global__ __launch_bounds__(256, (LDS && W4) ? GI_WF_MIN_WAVES_LDS : GI_WF_MIN_WAVES) void k_x_query_kat(
    DevScene sc, V3 cam_pos, int n, const double* recs, int32_t* oi, double* od) {
    extern __shared__ int4 lds_dyn[];
    const WFView v = wf_stage<LDS, FLAT>(sc, lds_dyn);
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool act = i < (long long)n;
    const double skip_cos = x_skip_cos(sc, cam_pos);
    const float far_r = ray_far_r(sc, cam_pos);   // (as k_seg: gi_dev.h ray_org32)
    V3 o = v3(0, 0, 0), d = v3(1, 0, 0), light = v3(0, 0, 0), d2 = v3(1, 0, 0);
    if (act) {
        const double* q = recs + 12 * i;
        o = v3(q[0], q[1], q[2]);
        d = v3(q[3], q[4], q[5]);
        light = v3(q[6], q[7], q[8]);
        d2 = v3(q[9], q[10], q[11]);
    }
    uint32_t nnode = 0, nprim = 0, st_steps = 0;
    // ---- closest hit (a primary ray: no skip)
    double t1 = INFINITY;
    const int p1 = x_query<false, LDS, SH, TRI, CN, FLAT>(sc, v, far_r, o, d, INFINITY, act, t1, nnode, nprim, st_steps, 254);
    const bool hit = act && p1 >= 0;
    const XHitFrame h = x_hit_frame(v, light, o, d, hit, p1, t1);
    // ---- shadow any-hit
    double tdummy;
    const int skip_s = x_own_plane(h.pg, h.pn, h.Ld, skip_cos);
    const int sb = x_query<true, LDS, SH, TRI, CN, FLAT>(sc, v, INFINITY, h.P, h.Ld, h.ldist, hit, tdummy, nnode, nprim, st_steps, skip_s);
    // ---- the next segment's closest hit, leaving the surface along d2
    const int skip2 = x_own_plane(h.pg, h.pn, d2, skip_cos);
    double t2 = INFINITY;
    const int p2 = x_query<false, LDS, SH, TRI, CN, FLAT>(sc, v, far_r, h.P, d2, INFINITY, hit, t2, nnode, nprim, st_steps, skip2);
    if (act) {
        oi[5 * i] = p1 >= 0 ? p1 : -1;
        oi[5 * i + 1] = hit ? (sb >= 0 ? 1 : 0) : -1;
        oi[5 * i + 2] = skip_s;
        oi[5 * i + 3] = (hit && p2 >= 0) ? p2 : -1;
        oi[5 * i + 4] = skip2;
        od[2 * i] = p1 >= 0 ? t1 : INFINITY;
        od[2 * i + 1] = (hit && p2 >= 0) ? t2 : INFINITY;
    }
    if (i == 0) od[2 * (long long)n] = skip_cos;
}

// Known-answer hook (gi_kat_x_texel; tests): the texel x_segment shades a hit with, one (entity, point)
// per lane.  Record i: the entity index (a double holding an integer in [0, n_ents), checked by the
// host) and the point (4 doubles).  mode 0: x_texel, the helper x_segment calls; mode 1: the exact code
// it stands for (x_texcoord + texel).  Lanes past n run the helper without a point (entity 0, the
// origin).  od[3 i ..]: the texel; oi[i]: x_texel's `how` (mode 1: 2).  The entity records are read from
// global memory (the helper is the same code wherever they lie).
template <bool TRI>
__global__ __launch_bounds__(256) void k_x_texel_kat(DevScene sc, int n, int mode, const double* recs, int32_t* oi, double* od) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool act = i < (long long)n;
    int ent = 0;
    V3 P = v3(0, 0, 0);
    if (act) {
        const double* q = recs + 4 * i;
        ent = (int)q[0];
        P = v3(q[1], q[2], q[3]);
    }
    const REnt& e = sc.ents[ent];
    int how = 2;
    V3 tc;
    if (mode == 0) {
        tc = x_texel<TRI>(sc, e, P, &how);
    } else {
        int32_t tu, tv;
        x_texcoord<TRI>(sc, e, P, tu, tv);
        tc = texel(ld3(e.color), tu, tv);
    }
    if (act) {
        od[3 * i] = tc.x; od[3 * i + 1] = tc.y; od[3 * i + 2] = tc.z;
        oi[i] = how;
    }
}

// The public ray queries (gi_intersect*, gi_occluded*; DESIGN.md §5 "Ray queries"): the closest hit
// (ANY = false: the (t, primitive) minimum over t in (MX_TMIN, tmax), with the primitive's entity and
// the facing unit normal) or any hit (ANY: 1 / 0) of n caller-supplied rays, through x_query in the
// variant a k_seg launch on the scene runs, the scene staged once per workgroup as k_seg stages it.
// Persistent grid, static schedule: wave w of the launch's W waves takes the batches of 64 rays
// w, w + W, ... -- no device counter, so concurrent calls share nothing, and nothing of the scene's
// render scratch (work list, counters, per-sample rows) is read or written.
//  skip: none (254).  A caller's ray leaves no known surface, so no plane group may be left out.
//  far_r: the scene's x_far_r always.  Origins are the caller's, so the choice in ray_org32 between
//    the origin and a point of the ray near the scene is made per lane here (divergent where a wave
//    mixes near and far origins) instead of once per launch.  With a finite tmax the rule stays
//    conservative for the reason it is with the best t: a far ray's box distances count from the
//    shifted point o + t0 d (t0 > 0) while tmax, like the best t it initialises in wf_trace and
//    wf_flat (tb, tbf, phase A's tfa), counts from o.  A box that begins at s from the shifted point
//    begins at s + t0 from o, so the exact bound from the shifted point would be tmax - t0; testing
//    s against tmax itself only keeps more boxes, and wf_flat's early exit (e2's floor > tbf) drops its
//    other candidates only when they begin beyond tmax + t0.  The fp64 primitive tests take o, d and
//    tmax as given, and compare t < tmax strictly (a first hit at t == tmax finds best = -1, which
//    no primitive index is below): the interval is open at both ends.
//  Malformed rays (a non-finite component of o or d, a zero d, a NaN tmax) and rays whose tmax is
//    not above MX_TMIN run as lanes without a ray, on a harmless stand-in ray: a miss, and no NaN
//    reaches a comparison that other lanes' control flow shares.
// Resources (hipcc -S, gfx950): DESIGN.md §9 "Ray queries".
template <bool ANY, bool LDS, bool W4, bool SH, bool TRI, bool CN, bool FLAT>
__global__ __launch_bounds__(256, (LDS && W4) ? GI_WF_MIN_WAVES_LDS : GI_WF_MIN_WAVES) void k_cast(DevScene sc, CastIO io) {
    extern __shared__ int4 lds_dyn[];
    const WFView v = wf_stage<LDS, FLAT>(sc, lds_dyn);
    const int lane = threadIdx.x & 63;
    const long long stride = 64ll * (long long)gridDim.x * (long long)(blockDim.x >> 6);
    for (long long base = 64ll * ((long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)); base < io.n; base += stride) {
        const long long i = base + lane;
        const bool in = i < io.n;
        V3 o = v3(0, 0, 0), d = v3(1, 0, 0);
        double tmax = INFINITY;
        bool act = false;
        if (in) {   // the 64-byte record in four 16-byte loads
            const double2* q = reinterpret_cast<const double2*>(io.rays) + 4 * i;
            const double2 q0 = q[0], q1 = q[1], q2 = q[2], q3 = q[3];
            const V3 ro = v3(q0.x, q0.y, q1.x), rd = v3(q1.y, q2.x, q2.y);
            const bool fin = __builtin_isfinite(ro.x) & __builtin_isfinite(ro.y) & __builtin_isfinite(ro.z) &
                             __builtin_isfinite(rd.x) & __builtin_isfinite(rd.y) & __builtin_isfinite(rd.z);
            const bool nz = (rd.x != 0.0) | (rd.y != 0.0) | (rd.z != 0.0);
            act = fin & nz & (q3.x > MX_TMIN);   // (false for a NaN tmax; q3.y is reserved)
            if (act) {
                o = ro;
                d = rd;
                tmax = q3.x;
            }
        }
        uint32_t nnode = 0, nprim = 0, nsteps = 0;
        double tb = INFINITY;
        const int best = x_query<ANY, LDS, SH, TRI, CN, FLAT>(sc, v, sc.x_far_r, o, d, tmax, act, tb, nnode, nprim, nsteps, 254);
        const bool hit = act && best >= 0;
        if constexpr (ANY) {
            if (in) io.occl[i] = hit ? 1 : 0;
        } else {
            if (in) {
                if (io.t) io.t[i] = hit ? tb : INFINITY;
                if (io.prim) io.prim[i] = hit ? best : -1;
                if (io.ent || io.nrm) {
                    int ent = -1;
                    V3 N = v3(0, 0, 0);
                    if (hit) {   // x_segment's facing normal
                        const XPrim& p = v.XP[best];
                        ent = p.ent;
                        const V3 P = o + tb * d;
                        N = (TRI || p.kind == 0) ? ld3(p.n) : normalize(P - ld3(p.a));
                        N = dot(d, N) < 0 ? N : -N;
                    }
                    if (io.ent) io.ent[i] = ent;
                    if (io.nrm) {
                        double* q = io.nrm + 3 * i;
                        q[0] = N.x; q[1] = N.y; q[2] = N.z;
                    }
                }
            }
        }
    }
}

// The radiance query (gi_radiance*; DESIGN.md §5 "Radiance query"): what radiance arrives along n
// caller-supplied rays.  Every record is one path sample: x_segment from its first ray on, in the variant a
// k_seg launch on the scene runs and with the scene staged as k_seg stages it, so a record that restates a
// render's jittered primary ray (gi_sample_rays*) gets that render's per-sample row bit for bit.  The path
// state sits where k_seg keeps it: L and T in the lane's slot fields 0-5, the RNG key in field 6, the record
// index and the sample in field 7 (idx | smp << 32, idx < 2^32: gi_capi.cpp), the own-plane skip and the bounce
// index in the plane register.
// Schedule: a persistent grid that refills without a device counter.  Wave w of the launch's W waves owns the
// runs w, w + W, ... of kRadRun records.  Each loop iteration is k_seg's direct path minus its atomic: lanes
// without a path take the next records of the wave's current run by their rank among such lanes (up to
// GI_SEG_BURST rounds: records that resolve at once leave their lanes free), then every live lane runs one
// segment, and a lane whose path ended stores L at its record index.  cur, cur_end and next are wave-uniform,
// and so is every branch of the loop; it ends when the wave has neither a live lane nor a record left.  The
// call reads the scene's immutable records and its own arguments only, as k_cast.
// What k_seg decides once per launch from its camera is decided per path here, origins being the caller's:
//  far_r: the scene's x_far_r always, ray_org32 chooses per lane (k_cast's rule and reasons); bounce rays start
//    inside the scene and take the near branch, shadow rays pass INFINITY inside x_segment.
//  the root pretest: wf_primary_misses from the record's o and unnormalised d; a miss stores exact +0.
//  skip_cos: x_skip_cos of the record's own o.  assign_plane_groups (gi_build.cpp) uses the camera only as the
//    bound |o| on the origin of the ray whose hit point P the next ray leaves: P's rounding is ~u (|o| + |P| +
//    ...), and every later origin is a hit point, within the scene's extent E that x_skip_b covers.  The
//    record's max |o| is that bound for the path's first hit and is kept, larger than needed, for its later ones.
//  shadow_live: all ones (x_shadow_live returns the full mask where the host cannot bound the origins).
// Malformed records (a non-finite component of o or d, a zero d) are screened as k_cast screens them: no path,
// (0, 0, 0) stored, no NaN reaches a comparison that other lanes' control flow shares.
// Resources (hipcc -S, gfx950): DESIGN.md §9 "Radiance query".
#ifndef GI_RAD_RUN
#define GI_RAD_RUN 64   // records per run of k_rad's static schedule
#endif
constexpr long long kRadRun = GI_RAD_RUN;
template <bool LDS, bool W4, bool SH, bool TRI, bool CN, bool FLAT>
__global__ __launch_bounds__(256, (LDS && W4) ? GI_WF_MIN_WAVES_LDS : GI_WF_MIN_WAVES) void k_rad(DevScene sc, RadIO io) {
    extern __shared__ int4 lds_dyn[];
    const WFView v = wf_stage<LDS, FLAT>(sc, lds_dyn);
    const bool no_shadow = io.no_shadow != 0;
    const long long hop = kRadRun * (long long)gridDim.x * (long long)(blockDim.x >> 6);
    // the wave's runs: records [cur, cur_end) of the current one, the next one begins at `next` (uniform)
    long long next = kRadRun * ((long long)blockIdx.x * (blockDim.x >> 6) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)));
    long long cur = 0, cur_end = 0;
    bool live = false;   // this lane carries a path
    V3 o = v3(0, 0, 0), d = v3(1, 0, 0), L = v3(0, 0, 0), T = v3(1, 1, 1);
    int splane = 254;        // the own-plane skip of the lane's next ray | bounce << kSegPlaneBits, as k_seg's
    double skip_cos = 2.0;   // the path's bound on |d . n| (above)
    uint32_t nnode = 0, nprim = 0, nrays = 0;
    WFSegStats ws;
    for (;;) {
        // ---- lanes without a path take records
        for (int burst = 0; burst < GI_SEG_BURST; ++burst) {
            const unsigned long long m_need = __ballot(!live);
            if (m_need == 0) break;
            if (cur == cur_end) {   // the run is used up: the wave's next one
                if (next >= io.n) break;
                cur = next;
                cur_end = min(io.n, next + kRadRun);
                next += hop;
            }
            const unsigned rank = seg_rank(m_need);
            const unsigned avail = (unsigned)(cur_end - cur), n_need = (unsigned)__popcll(m_need);
            const long long i = cur + (long long)rank;
            const bool take = !live && rank < avail;
            cur += (long long)min(n_need, avail);
            if (take) {   // i < cur_end <= n; the 64-byte record in three 16-byte loads (tmax, reserved: not read)
                const double2* q = reinterpret_cast<const double2*>(io.rays) + 4 * i;
                const double2 q0 = q[0], q1 = q[1], q2 = q[2];
                const V3 ro = v3(q0.x, q0.y, q1.x), rd = v3(q1.y, q2.x, q2.y);
                const bool fin = __builtin_isfinite(ro.x) & __builtin_isfinite(ro.y) & __builtin_isfinite(ro.z) &
                                 __builtin_isfinite(rd.x) & __builtin_isfinite(rd.y) & __builtin_isfinite(rd.z);
                const bool nz = (rd.x != 0.0) | (rd.y != 0.0) | (rd.z != 0.0);
                CamDev at{};   // (wf_primary_misses reads the position only)
                at.pos = ro;
                if (fin && nz && !wf_primary_misses(sc, at, rd)) {
                    uint64_t stream = (uint64_t)i, smp = 0;
                    if (io.ids) {
                        stream = io.ids[2 * i];
                        smp = io.ids[2 * i + 1] & 0xFFFFFFFFull;
                    }
                    live = true;
                    o = ro;
                    d = normalize(rd);
                    splane = 254;
                    skip_cos = x_skip_cos(sc, ro);
                    v.pl[0] = 0.0; v.pl[256] = 0.0; v.pl[512] = 0.0;
                    v.pl[768] = 1.0; v.pl[1024] = 1.0; v.pl[1280] = 1.0;
                    slot_put_u64(v.pl, 6, mx_key(io.seed, stream));
                    slot_put_u64(v.pl, 7, (uint64_t)(uint32_t)i | (smp << 32));
                } else {
                    double* r = io.rgb + 3 * i;
                    r[0] = 0.0; r[1] = 0.0; r[2] = 0.0;
                }
            }
        }
        if (__ballot(live) == 0) {
            if (cur == cur_end && next >= io.n) break;
            continue;
        }
        // ---- one segment of every live path
        const bool cont = x_segment<false, LDS, SH, TRI, CN, FLAT>(
            sc, v, io.light, io.depth, no_shadow, live,
            [&] { return PathId{slot_get_u64(v.pl, 6), (unsigned)(slot_get_u64(v.pl, 7) >> 32), splane >> kSegPlaneBits}; },
            o, d, L, T, nnode, nprim, nrays, ws, skip_cos, &splane, sc.x_far_r, ~0u);
        if (live) {
            if (cont) {
                splane += 1 << kSegPlaneBits;   // the next bounce
            } else {
                double* r = io.rgb + 3 * (long long)(uint32_t)slot_get_u64(v.pl, 7);
                r[0] = L.x; r[1] = L.y; r[2] = L.z;
                live = false;
            }
        }
    }
}

// Lane-to-pixel mapping of the feature-buffer kernels: batch b (64 lanes) of a cols x rows window takes
// the 64 consecutive window pixels 64 b .. 64 b + 63 in row order, so every plane store of a wave is one
// contiguous run (512 B of t, 1536 B of normals, ...).  The alternative, 8 x 8 tiles as the renders map
// their lanes (more coherent rays, stores in row pieces of 8 pixels), was built and measured on the
// MI355X on a 2048 x 2048 frame, t / prim / entity / normal (DESIGN.md §9 "Feature buffers";
// profiles/aov_rate.jsonl): the Cornell box 0.095-0.098 ms by rows, 0.094-0.095 by tiles (ranges
// overlap); soup100000 0.713 by rows against 0.739 ms.  Rows stayed, the tile mapping was removed.
__host__ __device__ inline long long aov_batches(int cols, int rows) { return ((long long)cols * (long long)rows + 63) / 64; }
// window pixel (px, py) of a lane; false: the lane has no pixel.  The division in 32 bits where it
// suffices (a frame holds at most 2^34 pixels, gi_capi.cpp check_aov_frame)
__device__ __forceinline__ bool aov_pixel(int cols, int rows, long long b, int lane, int& px, int& py) {
    const long long i = 64 * b + lane;
    if (i < (1ll << 32)) {
        const unsigned q = (unsigned)i / (unsigned)cols;
        py = (int)q;
        px = (int)((unsigned)i - q * (unsigned)cols);
    } else {
        const long long q = i / (long long)cols;
        py = (int)q;
        px = (int)(i - q * (long long)cols);
    }
    return i < (long long)cols * (long long)rows;
}

// First-hit feature buffers (gi_render_aov*; DESIGN.md §5 "Feature buffers"): what each pixel of the
// window [x0, x0 + cols) x [y0, y0 + rows) of a frame shows.  One lane per pixel; the pixel's ray is
// the primary ray of a 1-spp Mode X frame by k_seg's own steps -- o = cam.pos, d =
// normalize(primary_dir(x, y)) without jitter, the root pretest (wf_primary_misses: a miss), the
// launch-uniform far-camera rule (ray_far_r), no skip group -- and its closest hit x_query's in the
// variant a k_seg launch on the scene runs, the scene staged as k_seg stages it.  The hit's facing
// normal, entity, texture coordinate and texel are x_segment's.  Outputs are row-major planes over the
// window (64-bit indices); a null plane is not written.  Persistent grid, static schedule (as k_cast):
// no device counter, none of the scene's render scratch is read or written.
// Resources (hipcc -S, gfx950): DESIGN.md §9 "Feature buffers".
template <bool LDS, bool W4, bool SH, bool TRI, bool CN, bool FLAT>
__global__ __launch_bounds__(256, (LDS && W4) ? GI_WF_MIN_WAVES_LDS : GI_WF_MIN_WAVES) void k_aov(DevScene sc, CamDev cam, AovIO io) {
    extern __shared__ int4 lds_dyn[];
    const WFView v = wf_stage<LDS, FLAT>(sc, lds_dyn);
    const int lane = threadIdx.x & 63;
    const float far_r = ray_far_r(sc, cam.pos);   // (far cameras: gi_dev.h ray_org32)
    const long long n_batches = aov_batches(io.cols, io.rows);
    const long long stride = (long long)gridDim.x * (long long)(blockDim.x >> 6);
    const bool want_tex = io.alb || io.uv;
    for (long long b = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); b < n_batches; b += stride) {
        int px = 0, py = 0;
        const bool in = aov_pixel(io.cols, io.rows, b, lane, px, py);
        const V3 o = cam.pos;
        V3 d = v3(1, 0, 0);
        bool act = false;
        if (in) {
            const V3 d0 = primary_dir(cam, (double)(io.x0 + px), (double)(io.y0 + py));
            if (!wf_primary_misses(sc, cam, d0)) {
                act = true;
                d = normalize(d0);
            }
        }
        uint32_t nnode = 0, nprim = 0, nsteps = 0;
        double tb = INFINITY;
        const int best = x_query<false, LDS, SH, TRI, CN, FLAT>(sc, v, far_r, o, d, INFINITY, act, tb, nnode, nprim, nsteps, 254);
        const bool hit = act && best >= 0;
        if (in) {
            const long long i = (long long)py * (long long)io.cols + (long long)px;
            int ent = -1, tu = 0, tv = 0;
            V3 N = v3(0, 0, 0), tc = v3(0, 0, 0);
            if (hit) {   // x_segment's facing normal, texture coordinate and texel
                const XPrim& p = v.XP[best];
                ent = p.ent;
                const V3 P = o + tb * d;
                N = (TRI || p.kind == 0) ? ld3(p.n) : normalize(P - ld3(p.a));
                N = dot(d, N) < 0 ? N : -N;
                if (want_tex) {
                    const REnt& e = v.EN[p.ent];
                    x_texcoord<TRI>(sc, e, P, tu, tv);
                    tc = texel(ld3(e.color), tu, tv);
                }
            }
            if (io.t) io.t[i] = hit ? tb : INFINITY;
            if (io.prim) io.prim[i] = hit ? best : -1;
            if (io.ent) io.ent[i] = ent;
            if (io.nrm) {
                double* q = io.nrm + 3 * i;
                q[0] = N.x; q[1] = N.y; q[2] = N.z;
            }
            if (io.alb) {
                double* q = io.alb + 3 * i;
                q[0] = tc.x; q[1] = tc.y; q[2] = tc.z;
            }
            if (io.uv) {   // (two 4-byte stores: the caller's plane need not be 8-byte aligned)
                int32_t* q = io.uv + 2 * i;
                q[0] = tu; q[1] = tv;
            }
        }
    }
}

// The window's pixel rays as records of the ray queries (gi_camera_rays*): o = cam.pos, d = k_aov's
// normalize(primary_dir(x, y)) bit for bit, tmax = +inf, reserved = 0; row-major over the window,
// one lane per pixel, a 64-byte record in four 16-byte stores.  No scene.
__global__ __launch_bounds__(256) void k_cam_rays(CamDev cam, int x0, int y0, int cols, int rows, double* rays) {
    const long long n_batches = aov_batches(cols, rows);
    const long long stride = (long long)gridDim.x * (long long)(blockDim.x >> 6);
    const int lane = threadIdx.x & 63;
    for (long long b = (long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6); b < n_batches; b += stride) {
        int px = 0, py = 0;
        if (!aov_pixel(cols, rows, b, lane, px, py)) continue;
        const V3 d = normalize(primary_dir(cam, (double)(x0 + px), (double)(y0 + py)));
        double2* q = reinterpret_cast<double2*>(rays) + 4 * (64 * b + lane);
        q[0] = make_double2(cam.pos.x, cam.pos.y);
        q[1] = make_double2(cam.pos.z, d.x);
        q[2] = make_double2(d.y, d.z);
        q[3] = make_double2(INFINITY, 0.0);
    }
}

}  // namespace

// dynamic LDS of the bounce kernel and its kin: the per-lane path slots behind the level stack (lds false:
// the HBM-resident variants) or behind the staged scene's records (entity records included: read from
// global memory by the shading instead, C3 4.65 -> 4.69 ms, and 5 waves per SIMD with them there, 96 VGPRs
// and 120 B of scratch, 4.79 ms; profiles/r06_ab.txt) and, where the flat leaf table applies, its per-leaf
// candidate words.  flat: the launch runs the flat kernels, which do not stage the wide nodes (wf_stage)
constexpr size_t kWfStackBytes = 16 * 256 * sizeof(int);
size_t wf_lds_bytes(const DevScene& sc, bool lds, bool flat) {
    const size_t nodes = (flat && sc.x_flat) ? (size_t)sc.n_xwnodes * sizeof(XWNode) : 0;
    return (lds ? (size_t)sc.x_lds_bytes - nodes + (sc.x_flat ? kFlatPkBytes : 0) : kWfStackBytes) + kWfSlotBytes;
}
// dynamic LDS of a k_seg launch that runs the ring (XF_SEG_RING), beyond the other kernels' bytes
size_t wf_seg_ring_bytes() { return kSegRingBytes; }

// The kernel variant for a scene: f(XTag) (c.var: XLaunchCfg::var; c.flat: the flat leaf query, LDS-resident
// scenes whose table applies -- DevScene::x_flat -- unless GI_X_FLAT=0).  TRI of an LDS-resident scene is
// its W4 (light shading); HBM-resident scenes run SH = false.
namespace {
template <typename F>
void wf_dispatch(const DevScene& sc, const XKernelCfg& c, bool stats, F&& f) {
    const XVariant var = c.var;
    if (var.lds && c.flat && sc.x_flat)   // (SH only shapes the tree walk's level masks: one flat kernel per W4)
        with_bools([&](auto S, auto W) { f(XTag<S.value, true, W.value, true, W.value, false, true>{}); }, stats, var.w4);
    else if (var.lds)
        with_bools([&](auto S, auto W, auto H) { f(XTag<S.value, true, W.value, H.value, W.value, false, false>{}); },
                   stats, var.w4, sc.x_max_depth <= 7);
    else
        with_bools([&](auto S, auto T, auto C) { f(XTag<S.value, false, false, false, T.value, C.value, false>{}); },
                   stats, sc.x_tri_only != 0, sc.xcnodes != nullptr);
}
template <bool RING, typename V>
constexpr auto seg_kernel(V) { return &k_seg<V::stats, V::lds, V::w4, V::sh, V::tri, V::cn, V::flat, RING>; }
template <typename V>
constexpr auto bounce_kernel(V) { return &k_wf_bounce<V::stats, V::lds, V::w4, V::sh, V::tri, V::cn, V::flat>; }

template <bool ANY, typename V>
constexpr auto cast_kernel(V) { return &k_cast<ANY, V::lds, V::w4, V::sh, V::tri, V::cn, V::flat>; }

template <typename V>
constexpr auto aov_kernel(V) { return &k_aov<V::lds, V::w4, V::sh, V::tri, V::cn, V::flat>; }

template <typename V>
constexpr auto rad_kernel(V) { return &k_rad<V::lds, V::w4, V::sh, V::tri, V::cn, V::flat>; }
}  // namespace

XKernelCfg x_query_cfg(const XLaunchCfg& xc, int flags, WfKernel k) {
    const bool hbm = (flags & 2) != 0 && xc.var.lds;
    const bool flat = x_env().flat && (flags & 1) == 0;
    return XKernelCfg{hbm ? XVariant{} : xc.var, flat,
                      hbm ? kWfStackBytes + kWfSlotBytes : flat ? xc.wf_lds_bytes : xc.wf_tree_lds_bytes, xc.wf_grid[k]};
}

// resident workgroups per CU of kernel k in this scene's variant, with c.lds_bytes of dynamic LDS
hipError_t wf_occupancy(const DevScene& sc, WfKernel k, const XKernelCfg& c, int* per_cu) {
    hipError_t e = hipSuccess;
    wf_dispatch(sc, c, false, [&](auto V) {
        const void* f = nullptr;
        switch (k) {
            case WK_BOUNCE: f = reinterpret_cast<const void*>(bounce_kernel(V)); break;
            case WK_SEG: f = reinterpret_cast<const void*>(seg_kernel<false>(V)); break;
            case WK_SEG_RING: f = reinterpret_cast<const void*>(seg_kernel<true>(V)); break;
            case WK_CAST: f = reinterpret_cast<const void*>(cast_kernel<false>(V)); break;
            case WK_OCCL: f = reinterpret_cast<const void*>(cast_kernel<true>(V)); break;
            case WK_AOV: f = reinterpret_cast<const void*>(aov_kernel(V)); break;
            case WK_RAD: f = reinterpret_cast<const void*>(rad_kernel(V)); break;
            case WK_COUNT: break;
        }
        e = f ? hipOccupancyMaxActiveBlocksPerMultiprocessor(per_cu, f, 256, c.lds_bytes) : hipErrorInvalidValue;
    });
    return e;
}

// The Mode X pass after k_x_classify and before k_x_reduce in the wavefront forms.
//  XFORM_WF (wavefront): per chunk of units (the queue capacity; chunks for the launch's every pixel
//    slot, those past the work list's end return at once on the device) `depth` bounce launches;
//    counters: 2 per bounce (take, n_out), zeroed per chunk.
//  XFORM_SEG (segment-synchronous): one persistent launch; counter: a 64-bit unit count at xs.wcnt.
// c.flat is the launch's choice (xflags without XF_NO_FLAT).
hipError_t launch_wf(const DevScene& sc, const XKernelCfg& c, XForm form, const CamDev& cam, V3 light, int w, int h, int y0,
                     const gi_opts& o, double* rgb, uint8_t* rgb8, const XScratch& xs, const unsigned* n_list_dev,
                     unsigned long long* stats, int xflags, uint32_t live, hipStream_t stream, hipEvent_t ev_begin, hipEvent_t ev_end) {
    const TileMap m = make_map(w, h, o.shard_count, o.shard_index, y0);
    const int depth = o.depth;
    const int s0 = o.sample_end > 0 ? o.sample_begin : 0, s1 = o.sample_end > 0 ? o.sample_end : o.spp;
    const dim3 grid((unsigned)std::max(1, c.resident)), block(256);
    hipError_t e = hipSuccess;
    WFArgs a{};   // (the fields of a bounce stay zero in k_seg's)
    a.list = xs.list;
    a.n_list = n_list_dev;
    a.part = xs.part;
    a.s0 = (unsigned)s0;
    a.ns = (unsigned)(s1 - s0);
    if (form == XFORM_SEG) {   // (the unit counter xs.wcnt[0..1] was zeroed by k_x_classify)
        a.take = xs.wcnt;
        if (ev_begin) (void)hipEventRecord(ev_begin, stream);
        wf_dispatch(sc, c, stats != nullptr, [&](auto V) {
            if (xflags & XF_SEG_RING)   // (c.lds_bytes then holds the ring's: XLaunchCfg::seg_lds_bytes)
                hipLaunchKernelGGL(seg_kernel<true>(V), grid, block, c.lds_bytes, stream, sc, cam, light, m, o.spp, depth, o.seed, rgb, rgb8, stats, a, xflags, live);
            else
                hipLaunchKernelGGL(seg_kernel<false>(V), grid, block, c.lds_bytes, stream, sc, cam, light, m, o.spp, depth, o.seed, rgb, rgb8, stats, a, xflags, live);
        });
        if (ev_end) (void)hipEventRecord(ev_end, stream);
        return hipGetLastError();
    }
    // chunks for every pixel slot of the launch listed (the list's length stays on the device: no host
    // synchronisation, so the form can be captured in a graph); a chunk beyond the listed units' end
    // finds no input on the device and its bounce kernels return at once
    const unsigned long long units = (unsigned long long)m.n_local * (unsigned long long)(kWfTile * kWfTile) *
                                     (unsigned long long)(s1 - s0);
    if (ev_begin) (void)hipEventRecord(ev_begin, stream);
    for (unsigned long long u0 = 0; u0 < units; u0 += (unsigned long long)xs.wcap) {
        e = hipMemsetAsync(xs.wcnt, 0, 2 * (size_t)depth * sizeof(unsigned), stream);
        if (e != hipSuccess) return e;
        for (int b = 0; b < depth; ++b) {
            a.take = xs.wcnt + 2 * b;
            a.n_in = b > 0 ? xs.wcnt + 2 * (b - 1) + 1 : nullptr;
            a.n_out = xs.wcnt + 2 * b + 1;
            a.u0 = u0;
            a.u1 = std::min(units, u0 + (unsigned long long)xs.wcap);
            WFQ qin, qout;
            qin.cap = qout.cap = xs.wcap;
            qin.r = xs.wq[(b + 1) & 1];
            qin.id = reinterpret_cast<uint2*>(xs.wid[(b + 1) & 1]);
            qout.r = xs.wq[b & 1];
            qout.id = reinterpret_cast<uint2*>(xs.wid[b & 1]);
            wf_dispatch(sc, c, stats != nullptr, [&](auto V) {
                hipLaunchKernelGGL(bounce_kernel(V), grid, block, c.lds_bytes, stream, sc, cam, light, m, o.spp, depth, o.seed, b, rgb, rgb8, stats, a, qin, qout, xflags, live);
            });
        }
    }
    if (ev_end) (void)hipEventRecord(ev_end, stream);
    return hipGetLastError();
}

// gi_kat_x_query's launch: k_seg's variant for the scene (wf_dispatch), one ray per lane
hipError_t launch_x_query_kat(const DevScene& sc, const XKernelCfg& c, V3 cam_pos, int n, const double* recs, int32_t* oi,
                              double* od, hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    const dim3 grid((unsigned)(((long long)n + 255) / 256)), block(256);
    wf_dispatch(sc, c, false, [&](auto V) {
        using T = decltype(V);
        hipLaunchKernelGGL((k_x_query_kat<T::lds, T::w4, T::sh, T::tri, T::cn, T::flat>), grid, block, c.lds_bytes, stream, sc, cam_pos, n, recs, oi, od);
    });
    return hipGetLastError();
}

// gi_kat_x_texel's launch: TRI as k_seg's variant for the scene has it (wf_dispatch), one record per lane
hipError_t launch_x_texel_kat(const DevScene& sc, XVariant var, int n, int mode, const double* recs, int32_t* oi, double* od,
                              hipStream_t stream) {
    if (n <= 0) return hipSuccess;
    const dim3 grid((unsigned)(((long long)n + 255) / 256)), block(256);
    wf_dispatch(sc, XKernelCfg{var, false, 0, 0}, false, [&](auto V) {
        using T = decltype(V);
        hipLaunchKernelGGL((k_x_texel_kat<T::tri>), grid, block, 0, stream, sc, n, mode, recs, oi, od);
    });
    return hipGetLastError();
}

// The ray queries' launch: k_seg's variant for the scene (wf_dispatch) over a persistent grid of at most
// c.resident workgroups (wf_occupancy WK_CAST / WK_OCCL), fewer when the rays need fewer.  Asynchronous on
// `stream`; no allocation, no copy, no synchronisation.
hipError_t launch_cast(const DevScene& sc, const XKernelCfg& c, bool any, const CastIO& io, hipStream_t stream) {
    if (io.n <= 0) return hipSuccess;
    const long long want = (io.n + 255) / 256;
    const dim3 grid((unsigned)std::max<long long>(1, std::min<long long>(want, c.resident))), block(256);
    wf_dispatch(sc, c, false, [&](auto V) {
        if (any) hipLaunchKernelGGL(cast_kernel<true>(V), grid, block, c.lds_bytes, stream, sc, io);
        else hipLaunchKernelGGL(cast_kernel<false>(V), grid, block, c.lds_bytes, stream, sc, io);
    });
    return hipGetLastError();
}

// The feature buffers' launch: k_aov in k_seg's variant for the scene (wf_dispatch) over a persistent grid
// of at most c.resident workgroups (wf_occupancy WK_AOV), fewer when the window needs fewer.
// Asynchronous on `stream`; no allocation, no copy, no synchronisation.
hipError_t launch_aov(const DevScene& sc, const XKernelCfg& c, const CamDev& cam, const AovIO& io, hipStream_t stream) {
    if (io.cols <= 0 || io.rows <= 0) return hipSuccess;
    const long long want = (aov_batches(io.cols, io.rows) + 3) / 4;   // four waves (batches) per workgroup
    const dim3 grid((unsigned)std::max<long long>(1, std::min<long long>(want, c.resident))), block(256);
    wf_dispatch(sc, c, false, [&](auto V) {
        hipLaunchKernelGGL(aov_kernel(V), grid, block, c.lds_bytes, stream, sc, cam, io);
    });
    return hipGetLastError();
}

// The radiance query's launch: k_rad in k_seg's variant for the scene (wf_dispatch) over a persistent grid of at
// most c.resident workgroups (wf_occupancy WK_RAD), fewer when the records need fewer: a wave per run.
// GI_RAD_MAX_GRID (a TEST hook, read at every launch so that one process can set and clear it): at most that
// many workgroups, so that a small batch gives every wave several runs.  Asynchronous on `stream`; no
// allocation, no copy, no synchronisation.
hipError_t launch_rad(const DevScene& sc, const XKernelCfg& c, const RadIO& io, hipStream_t stream) {
    if (io.n <= 0) return hipSuccess;
    long long want = std::min<long long>((io.n + 4 * kRadRun - 1) / (4 * kRadRun), c.resident);
    if (const char* e = std::getenv("GI_RAD_MAX_GRID")) {
        if (std::atoi(e) > 0) want = std::min<long long>(want, std::atoi(e));
    }
    const dim3 grid((unsigned)std::max<long long>(1, want)), block(256);
    wf_dispatch(sc, c, false, [&](auto V) {
        hipLaunchKernelGGL(rad_kernel(V), grid, block, c.lds_bytes, stream, sc, io);
    });
    return hipGetLastError();
}

// gi_camera_rays*: the window's pixel rays as ray records (k_cam_rays), grid-stride over at most 2048
// workgroups.  Asynchronous on `stream`.
hipError_t launch_cam_rays(const CamDev& cam, int x0, int y0, int cols, int rows, double* rays, hipStream_t stream) {
    if (cols <= 0 || rows <= 0) return hipSuccess;
    const long long want = ((long long)cols * (long long)rows + 255) / 256;
    const dim3 grid((unsigned)std::min<long long>(want, 2048)), block(256);
    hipLaunchKernelGGL(k_cam_rays, grid, block, 0, stream, cam, x0, y0, cols, rows, rays);
    return hipGetLastError();
}

// the variant (LDS, W4, SH, TRI, CN, FLAT) wf_dispatch picks for a scene: what gi_kat_x_variant reports
void wf_variant(const DevScene& sc, const XKernelCfg& c, int32_t out[6]) {
    wf_dispatch(sc, c, false, [&](auto V) {
        out[0] = V.lds; out[1] = V.w4; out[2] = V.sh; out[3] = V.tri; out[4] = V.cn; out[5] = V.flat;
    });
}

}  // namespace gi
