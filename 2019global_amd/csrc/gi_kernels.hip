// gi_kernels.hip — gfx950 (CDNA4) kernels of the persistent Mode X form, and launch_render.
//
// Work decomposition: 8x8 pixel tiles dealt round-robin over shard ranks (tile t belongs to rank
// t % shard_count), so the same kernels serve 1 GPU and N-GPU tile sharding; four waves per
// 256-thread workgroup.  Mode X: persistent waves taking (pixel, run of samples) units from a device
// work list.  Mode R's kernels are in gi_mode_r.hip; k_wf_bounce, k_seg, k_cast and k_aov in gi_wf.hip;
// the host functions the units define for each other are declared in gi_launch.h.
//
// Mode X (build-defined): classify pass (background pixels) -> persistent path-tracing
//   kernel over (pixel, run of samples) work units, closest-hit + shadow any-hit through the 8-wide
//   BVH (front-to-back child slots by ray-direction octant) -> in-order per-sample reduce.
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (bit-level parity needs no FMA
// contraction; f64 div/sqrt are correctly rounded on gfx950).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <mutex>

#include "gi.h"
#include "gi_dev.h"
#include "gi_launch.h"
#include "gi_scene.h"

namespace gi {

namespace {

// Mode X path state machine.  A lane owns one pixel at a time and walks its spp samples in order;
// every loop iteration a lane either makes ONE traversal step of its current ray (pop a node: cull,
// push children, or test a leaf's primitives) or, once its ray has finished, runs the shading
// handler that consumes the hit and spawns the lane's next ray (shadow ray, next bounce, or the
// next sample's primary ray).  When a lane's pixel is complete it writes it and takes the next
// pixel from the device-wide slot counter (wave ballot + one atomic per refill), so lanes never
// wait for each other at sample, bounce or pixel boundaries (a fixed 8x8 tile per wave left ~1/4
// of the lanes idle behind the tile's slowest pixel).  The handler runs once at least half of the
// live lanes have a finished ray, or when none is still traversing, so it executes with a
// well-filled EXEC mask.  The per-path operation sequence is exactly the oracle's (pixel_mode_x in
// oracle/gi_oracle.cpp), so results are bit-identical whatever the schedule.
enum : int { PH_CLOSEST = 0, PH_SHADOW = 1, PH_NEED = 2, PH_START = 3, PH_DEAD = 4, PH_DONEPX = 5, PH_HELP = 6 };

#ifndef GI_X_START_BURST
#define GI_X_START_BURST 16   // primary rays a lane may resolve by the root test per handler run
#endif
#ifndef GI_X_MIN_WAVES
#define GI_X_MIN_WAVES 3       // minimum waves per SIMD (<= 168 VGPRs)
#endif

struct XCounters {
    uint64_t rays = 0, nodes = 0, prims = 0, px = 0, res = 0;   // res: samples resolved without traversal
    uint64_t iters = 0, trav = 0, handle = 0, hlanes = 0, hclose = 0, hshadow = 0;   // wave-level (lane 0)
    uint64_t cyc_trav = 0, cyc_hit = 0, cyc_next = 0, cyc_all = 0;                    // wave clock cycles
    // the longest sample path (primary ray to its end): (wall_clock64 ticks << 32) | (wave iterations
    // << 16) | traversal steps of that lane during it (both saturated at 65535), maximised as one word
    uint64_t path_t0 = 0, path_max = 0;
    uint32_t path_it = 0, path_st = 0;
    // divergence profile (wave-level, lane 0): loop iterations in which some lane ran a node test /
    // a leaf test / an inline bounce restart / a handler start-loop pass, and the lanes that did
    uint64_t it_node = 0, ln_node = 0, it_leaf = 0, ln_leaf = 0, it_rs = 0, ln_rs = 0, it_st = 0, ln_st = 0;
};

// Mode X work list (k_x_classify -> k_mode_x -> k_x_reduce).  A pixel whose every jittered primary
// ray misses the scene's root box is resolved by the classifier (all samples add exactly +0); the
// others are appended to `list` (their slot numbers in tile order).  k_mode_x's unit of work is one
// (listed pixel, run of k consecutive samples), k a power of two <= 8 chosen per launch from the
// amount of work (about 8 units per lane: k = 8 for a whole C3 frame, 1 for an 8-way shard of it).
// Units come in blocks of 64: block b = (group g of 64 listed pixels, run c), so one block is one
// run of 64 pixels; a wave takes a whole block with one atomic and one coalesced load of the
// group's 64 list entries, and hands its units to lanes as they need work (no per-unit round trip).
// With spp > 1 every sample's radiance is stored to part[pixel][sample] and k_x_reduce adds a
// pixel's samples in sample order from +0 (the oracle's sum), so results do not depend on k, on
// the schedule or on the shard count; with spp == 1 the unit writes the pixel.  Splitting pixels
// over lanes keeps every lane busy until the end of the frame (a whole 64-spp pixel per unit left
// the kernel waiting on its last lanes: rendering 1/8 of the C3 frame took 75% of the whole frame's
// time).
struct XWork {
    const unsigned* list;    // listed pixel slots (tile order)
    const unsigned* n_list;  // device count written by k_x_classify
    double* part;            // per-sample radiance [list index][sample][3] (spp > 1)
    unsigned* blocks;        // device counter of blocks taken
    int s0, s1;              // the launch's samples [s0, s1) of the spp (0, spp; or a progressive pass)
};

#ifndef GI_X_UNITS_PER_LANE
#define GI_X_UNITS_PER_LANE 8   // target units per lane when choosing the run length k
#endif
#ifndef GI_X_MAX_RUN
// largest run length k (samples per unit).  1: every unit is one sample -- measured fastest on the
// BASELINE Mode X workloads (C3 7.45 -> 6.72 ms, C5 338 -> 328 ms, X-zoo 7.7 -> 6.0 ms against k = 8;
// fewer wave iterations and fuller handler runs); scenes whose samples are mostly cheap background
// rays pay for the per-unit fetch instead (X-main 0.47 -> 0.72 ms) and are better served by 8
#define GI_X_MAX_RUN 1
#endif

// Shadow-ray handoff (HELP, XF_HANDOFF).  Once a wave has lanes with no work left (PH_DEAD: the
// end of the frame, or of a small shard), a lane that has shaded a hit whose path continues gives
// that hit's shadow ray to an idle lane and starts its next bounce ray at once, instead of tracing
// the two one after the other: the path's critical path becomes max(shadow_b, closest_{b+1}) per
// bounce instead of their sum.  The owner keeps both candidate sums (Lv lit, Lo dark) as before and
// picks one when the helper's answer arrives, before it shades the next hit, so the operations --
// and the frame, bit for bit -- are the oracle's.  Per lane in LDS (column layout, 256 lanes):
// ray[7][256] (origin, direction, tmax), own[256] (owner lane within the wave, -1: none) and
// res[256] (the owner's answer: 0 pending, 1 lit, 2 occluded).
struct XHelp {
    double* ray;
    int* own;
    int* res;
};
__device__ __forceinline__ int nth_set_bit(unsigned long long m, unsigned n) {
    for (unsigned i = 0; i < n; ++i) m &= m - 1;
    return __ffsll((long long)m) - 1;
}

// One wave of k_mode_x.  The traversal records are read from global memory: wide nodes W (XWNode, or
// the quantised XCNode), leaf records H, shading records XP / EN.
// nst: the wide-node index of every level of the current traversal path lives in LDS (nst[level *
// 256], one column per lane), so climbing out of exhausted levels is one ds_read instead of a chain
// of dependent parent-pointer loads from HBM / L2 (one per level climbed).
template <bool STATS, bool HELP, bool SH, bool TRI, typename NodeP, typename HotP, typename PrimP, typename EntP>
__device__ __forceinline__ void mode_x_wave(const DevScene& sc, NodeP W, HotP H, PrimP XP, EntP EN, int* nst, XHelp hp_,
                                            const CamDev& cam, V3 light,
                                            const TileMap& m, int spp, int depth, uint64_t seed, double* rgb,
                                            uint8_t* rgb8, unsigned* blk_list, const XWork& wk, int handle8,
                                            int xflags, XCounters& cnt) {
    const int lane = threadIdx.x & 63;
    const unsigned n_list = *wk.n_list;
    // run length k: the largest power of two <= the launch's maximum (xflags' XF_RUN bits: log2, from
    // GI_X_MAX_RUN or the environment variable of that name) and <= spp that still leaves about
    // GI_X_UNITS_PER_LANE units per lane of the grid (every wave computes the same k)
    int k = 1;
    {
        const double lanes = (double)gridDim.x * (double)blockDim.x;
        const double samples = (double)n_list * (double)(wk.s1 - wk.s0);
        const int max_run = 1 << ((xflags >> XF_RUN_SHIFT) & XF_RUN_MASK);
        while (2 * k <= max_run && 2 * k <= wk.s1 - wk.s0 && samples / (2.0 * k) >= GI_X_UNITS_PER_LANE * lanes) k *= 2;
    }
    const unsigned runs = (unsigned)((wk.s1 - wk.s0 + k - 1) / k);    // units per pixel (run c: samples s0 + c k ...)
    const unsigned n_groups = (n_list + 63u) >> 6;
    // XF_PIXEL_MAJOR (pixel-major blocks, launches of >= 64 units per pixel): a block is ONE pixel's
    // 64 consecutive runs instead of 64 pixels' run c, so a wave's lanes start on the same pixel's
    // samples -- nearly the same primary ray -- and walk the same nodes together
    const bool pm = (xflags & XF_PIXEL_MAJOR) != 0 && runs >= 64u;
    const unsigned rpb = (runs + 63u) >> 6;   // (pm) blocks per pixel
    const unsigned n_blocks = pm ? n_list * rpb : n_groups * runs;
    // XF_SPREAD: group g holds list entries g, g + G, g + 2G, ... (G groups) instead of
    // 64 consecutive ones, so a wave's 64 pixels come from all over the frame: the expensive pixels
    // of a frame cluster in space (the soup's core), and consecutive entries would give all of them
    // to a few waves, whose lanes then pace each other (every loop iteration waits for the others'
    // shading) while the rest of the chip idles.  Spread, each long path shares its wave with
    // cheap ones that finish early (fast iterations, idle lanes for its shadow rays).
    const bool spread = (xflags & XF_SPREAD) != 0;
    // the wave's current block lives in its LDS row: blk_list[0..63] = the group's list entries,
    // blk_meta = {units handed out, group, run}; lanes that do not run the handler keep no copy
    unsigned* blk_meta = blk_list + 64;
    if (lane == 0) { blk_meta[0] = 64u; blk_meta[3] = 0u; }
    __builtin_amdgcn_wave_barrier();
    const bool inline_shadow = (xflags & XF_INLINE_SHADOW) != 0;
    const bool no_shadow = (xflags & XF_NO_SHADOW) != 0;   // GI_FLAG_X_NO_SHADOW (tests): every light visible
    const bool handoff = HELP && (xflags & XF_HANDOFF) != 0 && !no_shadow;
    const int tid = threadIdx.x, wbase = tid & ~63;
    if (HELP) {
        hp_.own[tid] = -1;
        hp_.res[tid] = 0;
    }
    bool pend = false;       // this lane's last shadow ray is being traced by a helper
    bool any_gave = false;   // some lane of the wave handed a shadow ray over in the last iteration
    int howner = 0;          // PH_HELP: the owner lane
    uint32_t nnode = 0, nprim = 0, nrays = 0, nres = 0, npx = 0, nsteps = 0;
    long long idx = -1;
    int x = 0, y = 0;
    uint64_t key = 0;

    int phase = PH_NEED;
    int smp = 0, b = 0;
    // current ray
    V3 o = cam.pos, d = v3(1, 0, 0);
    int dmask = 0, best = -1, node = 0, level = 0;
    bool raying = false;
    // UL (quantised nodes): one load round trip per step for the node-test and leaf-test lanes
    // together
    // (round 5: in the build without the shadow handoff -- long launches, C5 -- the merged round
    // trip costs more than it saves: C5 178.3 -> 176.8 ms without it, C4 +2% without it, so it stays
    // in the handoff build only)
    constexpr bool UL = HELP && std::is_same<std::remove_cv_t<std::remove_pointer_t<NodeP>>, XCNode>::value;
    uint64_t mlo = 0, mhi = 0;
    double tbest = INFINITY, tmax = INFINITY;
    float tbest_f = INFINITY;
    F3 of = f3(0, 0, 0), ivf = f3(1, 1, 1);
    // path: Lv = L while the closest ray is traced; across the shadow ray Lv / Lo hold the two
    // candidate sums L + T*lit (light visible) and L + T*dark (occluded), and T already holds the
    // next bounce's throughput (the oracle's operations, split around the shadow query)
    V3 Lv = v3(0, 0, 0), Lo = v3(0, 0, 0), T = v3(1, 1, 1);
    V3 nextd = v3(0, 0, 0);   // carried across the shadow ray (its origin = the shadow ray's)
    bool has_next = false;

    // fp64 primitive tests of one leaf's records hp[0 .. cntl) (these decide the result), each
    // fetched one ahead of its test; the first one is already in registers (cur: UL below issues
    // that load itself).  A shadow ray (own or a helper's) stops at any hit.
    auto leaf_test_from = [&](XHotR cur, const auto* hp, int cntl) {
        for (int j = 0; j < cntl; ++j) {
            const XHotR rec = cur;
            // long launches (no handoff build): no load after the leaf's last record (C5 182.3 ->
            // 180.2 ms); the handoff build keeps the unconditional one-ahead load (C4 +3% without)
            if (HELP || j + 1 < cntl) cur = load_hot(hp + min(j + 1, cntl - 1));
            ++nprim;
            const double t = x_prim_t<TRI>(rec.h, o, d, MX_TMIN);
            const int pi = rec.h.prim;
            if (phase != PH_CLOSEST) {
                if (t < tmax) { best = pi; raying = false; return; }   // any hit occludes
            } else {   // (selects, not branches: | and & do not short-circuit)
                const bool u = (t < tbest) | ((t == tbest) & (pi < best));
                tbest = u ? t : tbest;
                best = u ? pi : best;
                tbest_f = u ? up32(t) : tbest_f;
            }
        }
    };
    // the same from the first record's load on.  (Kept a lambda: written out at its call site the
    // compiler orders 28 of the 32 kernels' instructions and registers differently -- DESIGN.md §5.)
    auto leaf_test = [&](const auto* hp, int cntl) { leaf_test_from(load_hot(hp), hp, cntl); };

    // The next pop's child reference and leaf count are fetched at the end of the step that sets up
    // the level (descend, climb or ray start), so the pop itself waits for no load: one dependent
    // round trip per step (the child's node or leaf records) instead of two.  (lvl mask, node) do
    // not change between that fetch and the pop.
    int pf_ch = 0, pf_cnt = 0;
    auto prefetch = [&]() {
        const uint32_t m = lvl_get<SH>(mlo, mhi, level);
        if (m) {
            const int c = __builtin_ctz(m) ^ dmask;
            pf_ch = W[node].child[c];
            pf_cnt = W[node].cnt[c];
        }
    };

    const uint64_t t_begin = STATS ? clock64() : 0;
    for (;;) {
        if (HELP && any_gave && phase == PH_DEAD) {   // an idle lane given a shadow ray starts it
            const int ow = hp_.own[tid];
            if (ow >= 0) {
                hp_.own[tid] = -1;
                howner = ow & 0xFF;
                const double* r = hp_.ray + tid;
                o = v3(r[0], r[256], r[512]);
                d = v3(r[768], r[1024], r[1280]);
                of = f3((float)o.x, (float)o.y, (float)o.z);
                ivf = inv_dir(d);
                dmask = (d.x < 0 ? 1 : 0) | (d.y < 0 ? 2 : 0) | (d.z < 0 ? 4 : 0);
                level = 0;
                mlo = mhi = 0;
                // a shadow ray
                tmax = r[1536];
                tbest = tmax;
                tbest_f = up32(tmax);
                phase = PH_HELP;
                best = -1;
                const uint32_t rm = children_mask<false>(W, of, ivf, tbest_f, dmask);
                node = 0;
                lvl_set<SH>(mlo, mhi, 0, rm);
                raying = rm != 0;
                if (raying) prefetch();
            }
        }
        const unsigned long long m_live = __ballot(phase != PH_DEAD);
        if (m_live == 0) break;
        const unsigned long long m_idle = HELP ? ~m_live : 0ull;   // lanes free to take a shadow ray
        bool gave = false;
        const bool trav = raying;
        const unsigned long long m_trav = __ballot(trav);
        const int n_wait = __popcll(m_live & ~m_trav);
        const bool handle = phase != PH_DEAD && !trav &&
                            (8 * n_wait >= handle8 * __popcll(m_live) || m_trav == 0);
        if (STATS) {   // ballots over the whole wave, accumulated by lane 0
            const unsigned long long m_h = __ballot(handle);
            const unsigned long long m_hc = __ballot(handle && phase == PH_CLOSEST);
            const unsigned long long m_hs = __ballot(handle && phase == PH_SHADOW);
            if (lane == 0) {
                ++cnt.iters;
                if (m_h) {
                    ++cnt.handle;
                    cnt.hlanes += __popcll(m_h);
                    cnt.hclose += __popcll(m_hc);
                    cnt.hshadow += __popcll(m_hs);
                }
            }
        }
        const uint64_t t0 = STATS ? clock64() : 0;
        if (STATS) ++cnt.path_it;
        if (trav) {
            if (STATS) {
                ++nsteps;
                ++cnt.path_st;
            }
            // ---- one traversal step (stackless: 8-bit "children left" mask per level).  Invariant:
            // the current level has a child left; the step pops it, then climbs past exhausted
            // levels, so a ray ends in the step that exhausts the root level (no empty iteration).
            // The popped child (the lowest set bit: next in front-to-back order) and its leaf count
            // were fetched by the step that set this level up (prefetch above).
            const uint32_t msk = lvl_get<SH>(mlo, mhi, level);
            lvl_set<SH>(mlo, mhi, level, msk & (msk - 1));
            const int ch = pf_ch;
            // A closer hit may have arrived since the mask was computed, but the child is not
            // re-culled against it: an interior child's own node test culls its children against the
            // same t, a leaf's fp64 tests run against the best t as it stands, and the re-cull would
            // cost a node-record fetch and ~60 instructions per step (round 3: C5 214 -> 199 ms, C4
            // 1.96 -> 1.82 without it).
            if (STATS) {
                const unsigned long long mn = __ballot(ch >= 0), ml = __ballot(ch < 0);
                if (lane == 0) {
                    cnt.it_node += mn != 0;
                    cnt.ln_node += __popcll(mn);
                    cnt.it_leaf += ml != 0;
                    cnt.ln_leaf += __popcll(ml);
                }
            }
            if (UL) {
                // one memory round trip for the wave's node-test AND leaf-test lanes: each lane's
                // load (the child's 64 slab bytes, or its leaf's first record) is issued before
                // either test waits, instead of a node-test block and a leaf-test block each
                // waiting on its own load
                XHotR ur;
                const int cntl = ch < 0 ? pf_cnt : 0;
                if (ch < 0) {
                    ur = load_hot(H + ~ch);
                } else {
                    const int4* qb = reinterpret_cast<const int4*>(W + ch);
                    ur.q[0] = qb[0];
                    ur.q[1] = qb[1];
                    ur.q[2] = qb[2];
                    ur.q[3] = qb[3];
                }
                if (ch < 0) leaf_test_from(ur, H + ~ch, cntl);
                if (ch >= 0) {
                    ++nnode;
                    const uint32_t cm = children_mask_q(ur.q[0], ur.q[1], ur.q[2], ur.q[3], of, ivf, tbest_f, dmask);
                    if (cm) {
                        node = ch;
                        ++level;
                        lvl_set<SH>(mlo, mhi, level, cm);
                        nst[level * 256] = ch;
                    }
                }
            } else if (ch < 0) {      // leaf: fp64 primitive tests (these decide the result)
                leaf_test(H + ~ch, pf_cnt);
            } else {                  // descend if any of the child's 8 children is hit (fp32)
                ++nnode;
                const uint32_t cm = children_mask<false>(W + ch, of, ivf, tbest_f, dmask);
                if (cm) {
                    node = ch;
                    ++level;
                    lvl_set<SH>(mlo, mhi, level, cm);
                    nst[level * 256] = ch;
                }
            }
            if (raying) {             // climb to the nearest level with children left
                uint32_t rest = lvl_get<SH>(mlo, mhi, level);
                if (rest == 0 && level > 0) {
                    // the deepest level below with children left, by one leading-zero count
                    const uint64_t lm = level >= 8 ? mlo : mlo & ((1ull << (8 * level)) - 1);
                    const uint64_t hm = level <= 8 ? 0ull : mhi & ((1ull << (8 * (level - 8))) - 1);
                    level = hm ? 8 + (63 - __clzll((long long)hm)) / 8 : lm ? (63 - __clzll((long long)lm)) / 8 : 0;
                    rest = lvl_get<SH>(mlo, mhi, level);
                    node = level == 0 ? 0 : nst[level * 256];
                }
                if (rest == 0) raying = false;   // ray finished
            }
            if (raying) prefetch();
            // a finished shadow ray whose path continues: resolve it and start the next bounce
            // right here (the bounce direction was drawn when the hit was shaded), so the lane
            // keeps traversing instead of waiting for the shading handler (short-traversal scenes;
            // for long ones the extra divergent root test costs more than it saves)
            if (STATS) {
                const unsigned long long mr = __ballot(inline_shadow && !raying && phase == PH_SHADOW && has_next);
                if (lane == 0) {
                    cnt.it_rs += mr != 0;
                    cnt.ln_rs += __popcll(mr);
                }
            }
            if (inline_shadow && !raying && phase == PH_SHADOW && has_next) {
                ++nrays;
                if (best >= 0) Lv = Lo;   // occluded: ambient term only
                d = nextd;                // o is still the hit point
                ++b;
                phase = PH_CLOSEST;
                tmax = INFINITY;
                tbest = INFINITY;
                tbest_f = INFINITY;
                of = f3((float)o.x, (float)o.y, (float)o.z);
                ivf = inv_dir(d);
                dmask = (d.x < 0 ? 1 : 0) | (d.y < 0 ? 2 : 0) | (d.z < 0 ? 4 : 0);
                best = -1;
                const uint32_t rm = children_mask<false>(W, of, ivf, tbest_f, dmask);
                node = 0;
                level = 0;
                mlo = mhi = 0;
                lvl_set<SH>(mlo, mhi, 0, rm);
                raying = rm != 0;
                if (raying) prefetch();
            }
        }
        const uint64_t t1 = STATS ? clock64() : 0;
        uint64_t t2 = t1;
        if (HELP && handle && phase == PH_HELP) {   // a helper's answer to its owner; idle again
            ++nrays;
            hp_.res[wbase + howner] = best >= 0 ? 2 : 1;
            phase = PH_DEAD;
        }
        bool hold = false;   // an owner whose helper has not answered yet: no handling this time
        if (HELP) {
            __builtin_amdgcn_wave_barrier();
            if (handle && pend) {
                const int r = hp_.res[tid];
                if (r == 0) {
                    hold = true;
                } else {
                    if (r == 2) Lv = Lo;   // occluded: ambient only
                    hp_.res[tid] = 0;
                    pend = false;
                }
            }
        }
        if (handle && !hold && phase != PH_DEAD) {
            // ---- the lane's ray is finished: consume it, spawn the next one --------------------
            bool end_path = false;
            if (phase == PH_CLOSEST) {
                ++nrays;
                if (best < 0) {
                    end_path = true;
                } else {
                    const V3 din = d;   // the incoming direction
                    const V3 P = o + tbest * d;
                    const XPrim& p = XP[best];   // by reference: only used fields are loaded
                    const REnt& e = EN[p.ent];
                    V3 N = (TRI || p.kind == 0) ? ld3(p.n) : normalize(P - ld3(p.a));
                    if (!(dot(din, N) < 0)) N = -N;
                    int32_t tu, tv;
                    x_texcoord<TRI>(sc, e, P, tu, tv);
                    const V3 tc = texel(ld3(e.color), tu, tv);
                    const V3 lv = light - P;
                    const double ldist = gsqrt(dot(lv, lv));
                    const V3 Ld = normalize(lv);
                    const V3 la = tc * e.shader[0];
                    const V3 ldf = (smax(0.0, dot(N, Ld)) * (tc * 0.5)) * e.shader[1];
                    const V3 bis = normalize(normalize(-din) + Ld);
                    const double spw = mx_pow(smax(0.0, dot(N, bis)), e.spec_pow);
                    const V3 ls = v3(spw, spw, spw) * e.shader[2];
                    const V3 lo = (la + ldf) + ls;
                    Lo = Lv + vmul(T, v3(smin(la.x, 1.0), smin(la.y, 1.0), smin(la.z, 1.0)));
                    Lv = Lv + vmul(T, v3(smin(lo.x, 1.0), smin(lo.y, 1.0), smin(lo.z, 1.0)));
                    has_next = false;
                    // mirror bounce with probability e.refl (uniform dim 4): T unchanged, d reflected
                    // about the facing normal; otherwise the diffuse bounce below
                    const bool mirror = b != depth - 1 && e.refl > 0.0 &&
                                        mx_u01k(key, smp, b, 4) < e.refl;
                    if (mirror) {
                        nextd = normalize(din - N * (2.0 * dot(din, N)));
                        has_next = true;
                    } else if (b != depth - 1) {
                        const V3 Tn = vmul(T, tc * 0.5);
                        T = Tn;
                        if (!(Tn.x == 0.0 && Tn.y == 0.0 && Tn.z == 0.0)) {
                            double sx, sy, r2;   // cosine-weighted: concentric disk + Malley
                            mx_disk(mx_u01k(key, smp, b, 2), mx_u01k(key, smp, b, 3), sx, sy, r2);
                            const double sz = gsqrt(1.0 - r2);
                            const double sg = N.z >= 0.0 ? 1.0 : -1.0;
                            const double aa = -1.0 / (sg + N.z);
                            const double bb = N.x * N.y * aa;
                            const V3 bt1 = v3(1.0 + sg * N.x * N.x * aa, sg * bb, -sg * N.x);
                            const V3 bt2 = v3(bb, sg + N.y * N.y * aa, -N.y);
                            nextd = normalize((bt1 * sx + bt2 * sy) + N * sz);
                            has_next = true;
                        }
                    }
                    // shadow ray toward the point light: handed to an idle lane of the wave when the
                    // path continues and one is free (the k-th giver takes the k-th idle lane), the
                    // lane then starts its next bounce at once; else traced here first
                    bool give = handoff && has_next;
                    if (HELP) {
                        const unsigned long long m_give = __ballot(give);
                        if (give) {
                            const unsigned r = (unsigned)__popcll(m_give & ((1ull << lane) - 1));
                            give = r < (unsigned)__popcll(m_idle);
                            if (give) {
                                const int ht = wbase + nth_set_bit(m_idle, r);
                                double* hr = hp_.ray + ht;
                                hr[0] = P.x; hr[256] = P.y; hr[512] = P.z;
                                hr[768] = Ld.x; hr[1024] = Ld.y; hr[1280] = Ld.z;
                                hr[1536] = ldist;
                                hp_.own[ht] = lane;
                                pend = true;
                                gave = true;
                                o = P;
                                d = nextd;
                                ++b;
                                phase = PH_CLOSEST;
                                tmax = INFINITY;
                                tbest = INFINITY;
                                tbest_f = INFINITY;
                            }
                        }
                    }
                    if (!give) {
                        phase = PH_SHADOW;
                        o = P;
                        d = Ld;
                        tmax = ldist;
                        tbest = ldist;
                        tbest_f = up32(ldist);
                    }
                }
            } else if (phase == PH_SHADOW) {
                ++nrays;
                if (best >= 0) Lv = Lo;   // occluded: ambient term only
                if (!has_next) {
                    end_path = true;
                } else {
                    d = nextd;   // o is still the hit point
                    ++b;
                    phase = PH_CLOSEST;
                    tmax = INFINITY;
                    tbest = INFINITY;
                    tbest_f = INFINITY;
                }
            }
            if (end_path) {
                if (STATS)
                    cnt.path_max = max(cnt.path_max, (((uint64_t)wall_clock64() - cnt.path_t0) << 32) |
                                                         ((uint64_t)min(cnt.path_it, 65535u) << 16) |
                                                         (uint64_t)min(cnt.path_st, 65535u));
                if (spp == 1) {   // the pixel: min((0 + L) / 1, 1), the reduce pass's operations
                    const double c0 = smin((0.0 + Lv.x) / 1.0, 1.0), c1 = smin((0.0 + Lv.y) / 1.0, 1.0),
                                 c2 = smin((0.0 + Lv.z) / 1.0, 1.0);
                    if (rgb) { rgb[3 * idx] = c0; rgb[3 * idx + 1] = c1; rgb[3 * idx + 2] = c2; }
                    if (rgb8) quantize(c0, c1, c2, rgb8 + 3 * idx);
                } else {   // the sample's radiance; k_x_reduce sums a pixel's samples in order
                    double* q = wk.part + 3 * ((size_t)idx * (size_t)spp + (size_t)smp);
                    q[0] = Lv.x; q[1] = Lv.y; q[2] = Lv.z;
                }
                ++smp;
                phase = (smp < wk.s1 && ((smp - wk.s0) & (k - 1)) != 0) ? PH_START : PH_DONEPX;
            }
            if (STATS) t2 = clock64();
            // ---- the lane's next ray.  A primary ray that misses every child box of the root
            // cannot hit anything: its sample adds exactly +0 to the pixel sums (the oracle traces
            // it and adds L = 0), so it is resolved here and the lane moves on to its next sample,
            // next pixel (fetched from the slot counter, one atomic per wave) -- up to
            // GI_X_START_BURST primary rays per lane per handler run.
            int burst = 0;
            for (;;) {
                if (STATS) {
                    const unsigned long long mb = __ballot(true);
                    if (lane == 0) {
                        cnt.it_st += 1;
                        cnt.ln_st += __popcll(mb);
                    }
                }
                if (phase == PH_DONEPX) phase = PH_NEED;   // unit complete (its samples are stored)
                const unsigned long long m_need = __ballot(phase == PH_NEED);
                if (m_need) {
                    // units of the wave's current block first, then of one new block (a refill asks
                    // for at most 64 units = one block).  The block's 64 list entries live in this
                    // wave's LDS row (the lanes that run the handler load them; the others may be
                    // traversing), so handing out a unit costs one ds_read.
                    const unsigned rank = (unsigned)__popcll(m_need & ((1ull << lane) - 1));
                    const unsigned n_need = (unsigned)__popcll(m_need);
                    const int leader = __ffsll((long long)m_need) - 1;
                    const unsigned used = blk_meta[0];
                    unsigned g = blk_meta[1], c = blk_meta[2];
                    const unsigned avail = 64u - used;
                    unsigned j = used + rank;
                    bool have = rank < avail;
                    unsigned ps = have ? blk_list[j] : 0u;
                    unsigned used_new = used + n_need;
                    if (n_need > avail) {                          // take the next block
                        // once the wave has seen the block counter run out (blk_meta[3]), no more atomics:
                        // each would be an L2 round trip for nothing (C4 spends ~90% of its loop
                        // iterations after that point, ending ~100 paths per wave)
                        unsigned nb = n_blocks;
                        if (blk_meta[3] == 0u) {
                            if (lane == leader) nb = atomicAdd(wk.blocks, 1u);
                            nb = __shfl(nb, leader);
                        }
                        used_new = 64u;
                        if (nb < n_blocks) {
                            // (pm: ng = the pixel's list index, nc = its block's first run)
                            const unsigned ng = pm ? nb / rpb : nb / runs, nc = pm ? (nb - ng * rpb) * 64u : nb - ng * runs;
                            const unsigned long long m_act = __ballot(true);
                            const unsigned ra = (unsigned)__popcll(m_act & ((1ull << lane) - 1));
                            const unsigned na = (unsigned)__popcll(m_act);
                            __builtin_amdgcn_wave_barrier();
                            const unsigned pm_ps = pm ? wk.list[ng] : 0u;
                            for (unsigned e = ra; e < 64u; e += na) {
                                if (pm) {
                                    blk_list[e] = nc + e < runs ? pm_ps : 0xFFFFFFFFu;
                                } else {
                                    const unsigned li = spread ? e * n_groups + ng : ng * 64u + e;
                                    blk_list[e] = li < n_list ? wk.list[li] : 0xFFFFFFFFu;
                                }
                            }
                            __builtin_amdgcn_wave_barrier();
                            used_new = n_need - avail;
                            if (lane == leader) { blk_meta[1] = ng; blk_meta[2] = nc; }
                            if (!have) {
                                j = rank - avail;
                                ps = blk_list[j];
                                c = nc;
                                g = ng;
                                have = true;
                            }
                        } else if (!have && phase == PH_NEED) {
                            phase = PH_DEAD;                        // no work left
                        }
                        if (nb >= n_blocks && lane == leader) blk_meta[3] = 1u;   // the frame's work is all handed out
                    }
                    if (lane == leader) blk_meta[0] = used_new;
                    __builtin_amdgcn_wave_barrier();
                    if (phase == PH_NEED && have) {
                        const unsigned i = pm ? g : spread ? j * n_groups + g : g * 64u + j;   // list index
                        const unsigned cu = pm ? c + j : c;        // the unit's run
                        if (ps != 0xFFFFFFFFu) {                   // else a padding unit: take another
                            slot_pixel(m, (long long)(ps >> 6), (int)(ps & 63), idx, x, y);
                            y += m.y0;
                            if (spp > 1) idx = (long long)i;        // per-sample radiance row
                            key = mx_key(seed, (uint64_t)y * (uint64_t)m.w + (uint64_t)x);
                            smp = wk.s0 + (int)cu * k;
                            phase = PH_START;
                            if (cu == 0) ++npx;
                        }
                    }
                }
                if (phase == PH_NEED) continue;   // got a padding unit: take another
                if (phase == PH_DEAD) break;
                if (phase == PH_START) {
                    double jx = 0.0, jy = 0.0;
                    if (spp > 1) {
                        jx = mx_u01k(key, smp, 0xFFFF, 0);
                        jy = mx_u01k(key, smp, 0xFFFF, 1);
                    }
                    const V3 d0 = primary_dir(cam, (double)x + jx, (double)y + jy);
                    if (burst < GI_X_START_BURST) {
                        // conservative fp32 test of the scene's root box on the unnormalised
                        // direction (slab test is scale-invariant; the padding covers rounding)
                        const F3 iv0 = f3(__builtin_amdgcn_rcpf((float)d0.x), __builtin_amdgcn_rcpf((float)d0.y),
                                          __builtin_amdgcn_rcpf((float)d0.z));
                        if (!root_hit(sc, f3((float)cam.pos.x, (float)cam.pos.y, (float)cam.pos.z), iv0)) {
                            ++nrays;   // background sample: L = 0
                            ++nres;
                            if (spp > 1) {
                                double* q = wk.part + 3 * ((size_t)idx * (size_t)spp + (size_t)smp);
                                q[0] = 0.0; q[1] = 0.0; q[2] = 0.0;
                            } else {   // spp == 1: the pixel is 0
                                if (rgb) { rgb[3 * idx] = 0.0; rgb[3 * idx + 1] = 0.0; rgb[3 * idx + 2] = 0.0; }
                                if (rgb8) { rgb8[3 * idx] = 0; rgb8[3 * idx + 1] = 0; rgb8[3 * idx + 2] = 0; }
                            }
                            ++burst;
                            ++smp;
                            phase = (smp < wk.s1 && ((smp - wk.s0) & (k - 1)) != 0) ? PH_START : PH_DONEPX;
                            continue;
                        }
                    }
                    if (STATS) {
                        cnt.path_t0 = (uint64_t)wall_clock64();
                        cnt.path_it = 0;
                        cnt.path_st = 0;
                    }
                    o = cam.pos;
                    d = normalize(d0);
                    Lv = v3(0, 0, 0);
                    T = v3(1, 1, 1);
                    b = 0;
                    tmax = INFINITY;
                    tbest = INFINITY;
                    tbest_f = INFINITY;
                }
                if (no_shadow && phase == PH_SHADOW) {   // unoccluded without a query
                    best = -1;
                    raying = false;
                    break;
                }
                // start traversing the lane's ray (fp32 reciprocal, 1 ulp: the culling error stays
                // far inside the 1e-5*extent box padding)
                of = f3((float)o.x, (float)o.y, (float)o.z);
                ivf = inv_dir(d);
                dmask = (d.x < 0 ? 1 : 0) | (d.y < 0 ? 2 : 0) | (d.z < 0 ? 4 : 0);
                const uint32_t rm = children_mask<false>(W, of, ivf, tbest_f, dmask);
                if (phase == PH_START) phase = PH_CLOSEST;
                best = -1;
                node = 0;   // root wide node
                level = 0;
                mlo = mhi = 0;
                lvl_set<SH>(mlo, mhi, 0, rm);
                raying = rm != 0;   // no root child hit: finished (consumed by the next handler run)
                if (raying) prefetch();
                break;
            }
        }
        if (HELP) any_gave = __ballot(gave) != 0;
        if (STATS) {
            const uint64_t t3 = clock64();
            cnt.cyc_trav += t1 - t0;
            cnt.cyc_hit += t2 - t1;
            cnt.cyc_next += t3 - t2;
        }
    }
    if (STATS) cnt.cyc_all += clock64() - t_begin;
    if (STATS) {   // lane traversal steps, summed over the wave into lane 0
        uint64_t ns = nsteps;
        for (int off = 32; off > 0; off >>= 1) ns += __shfl_xor(ns, off);
        cnt.trav += ns;
    }
    cnt.rays += nrays;
    cnt.nodes += nnode;
    cnt.prims += nprim;
    cnt.px += npx;
    cnt.res += nres;
}

// Persistent waves: the grid is sized to the resident capacity; every lane pulls pixel slots
// from one device counter (SURVEY §7 hard part 4: per-ray cost varies ~10x between background
// and scene pixels), so no lane idles behind a sibling, a workgroup or the grid tail.
// The scene is read from global memory, whether or not it would fit in LDS: by default
// (x_form_choice) the kernel runs large HBM-resident scenes only; a scene staged in LDS by k_seg
// comes here only when the form is forced (GI_FLAG_X_MEGA, GI_X_WF=0) and is traversed like any other.
// HELP (launch_render's rule): the shadow-ray handoff build (XHelp), chosen per launch for small launches,
// whose frame time is their longest paths' latency (C4: 3.01 -> 2.64 ms, with spread work groups
// 2.40 ms); in long launches (C5) the handoff build's heavier code costs 8%, so they run without.
// CN: traverse the quantised nodes (DevScene::xcnodes) instead of XWNode.
// SH: the per-level masks in one 64-bit word (trees of at most 8 levels).
// TR: the scene is triangle meshes of the 4-wave kinds only (DevScene::x_tri_only, e.g. the 100k
// soup): mode_x_wave's TRI specialisation.
// x_dispatch (below) names the instantiations that are launched: STATS x HELP x CN x SH x TR.
template <bool STATS, bool HELP, bool CN, bool SH, bool TR>
__global__ __launch_bounds__(256, GI_X_MIN_WAVES) void k_mode_x(DevScene sc, CamDev cam, V3 light, TileMap m, int spp, int depth,
                                                 uint64_t seed, double* rgb, uint8_t* rgb8,
                                                 unsigned long long* stats, XWork wk, int handle8, int xflags) {
    XCounters c;
    __shared__ unsigned s_blk[kWavesPerBlock][68];   // per wave: current block's list entries + state
    unsigned* blk = s_blk[threadIdx.x >> 6];
    // dynamic LDS: the 16 levels x 256 lanes of node indices, then the handoff
    // slots (7 x 256 doubles, 2 x 256 ints)
    extern __shared__ int lds_nst[];
    XHelp hp;
    hp.ray = reinterpret_cast<double*>(lds_nst + 16 * 256);
    hp.own = reinterpret_cast<int*>(hp.ray + 7 * 256);
    hp.res = hp.own + 256;
    if constexpr (CN)   // quantised nodes (the default for large HBM-resident scenes)
        mode_x_wave<STATS, HELP, SH, TR>(sc, sc.xcnodes, sc.xhot, sc.xprims, sc.ents, lds_nst + threadIdx.x, hp, cam, light, m,
                                         spp, depth, seed, rgb, rgb8, blk, wk, handle8, xflags, c);
    else
        mode_x_wave<STATS, HELP, SH, TR>(sc, sc.xwnodes, sc.xhot, sc.xprims, sc.ents, lds_nst + threadIdx.x, hp, cam, light, m,
                                         spp, depth, seed, rgb, rgb8, blk, wk, handle8, xflags, c);
    if (STATS) {
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(stats + GI_STAT_X_ITERS, (unsigned long long)c.iters);
            atomicAdd(stats + GI_STAT_X_TRAV, (unsigned long long)c.trav);
            atomicAdd(stats + GI_STAT_X_HANDLE, (unsigned long long)c.handle);
            atomicAdd(stats + GI_STAT_X_HLANES, (unsigned long long)c.hlanes);
            atomicAdd(stats + GI_STAT_X_HCLOSE, (unsigned long long)c.hclose);
            atomicAdd(stats + GI_STAT_X_HSHADOW, (unsigned long long)c.hshadow);
            atomicAdd(stats + GI_STAT_X_CYC_TRAV, (unsigned long long)c.cyc_trav);
            atomicAdd(stats + GI_STAT_X_CYC_HIT, (unsigned long long)c.cyc_hit);
            atomicAdd(stats + GI_STAT_X_CYC_NEXT, (unsigned long long)c.cyc_next);
            atomicAdd(stats + GI_STAT_X_CYC_ALL, (unsigned long long)c.cyc_all);
            atomicAdd(stats + GI_STAT_X_IT_NODE, (unsigned long long)c.it_node);
            atomicAdd(stats + GI_STAT_X_LN_NODE, (unsigned long long)c.ln_node);
            atomicAdd(stats + GI_STAT_X_IT_LEAF, (unsigned long long)c.it_leaf);
            atomicAdd(stats + GI_STAT_X_LN_LEAF, (unsigned long long)c.ln_leaf);
            atomicAdd(stats + GI_STAT_X_IT_RS, (unsigned long long)c.it_rs);
            atomicAdd(stats + GI_STAT_X_LN_RS, (unsigned long long)c.ln_rs);
            atomicAdd(stats + GI_STAT_X_IT_ST, (unsigned long long)c.it_st);
            atomicAdd(stats + GI_STAT_X_LN_ST, (unsigned long long)c.ln_st);
        }
        wave_add_stats(stats, c.rays, c.nodes, c.prims, c.px);
        uint64_t cr = c.res, pm = c.path_max;
        for (int off = 32; off > 0; off >>= 1) {
            cr += __shfl_xor(cr, off);
            pm = max(pm, (uint64_t)__shfl_xor(pm, off));
        }
        if ((threadIdx.x & 63) == 0) {
            atomicAdd(stats + GI_STAT_X_RESOLVED, (unsigned long long)cr);
            atomicMax(stats + GI_STAT_X_PATH_MAX, (unsigned long long)pm);
        }
    }
}

// Mode X pass 1: one thread per pixel slot (tile order; a wave = one 8x8 tile).  A pixel none of
// whose jittered primary rays can meet the scene's root box (conservative fp64 frustum test) is 0:
// every sample adds exactly +0, as in the oracle, which traces them.  Padding slots of a packed
// tile are zeroed.  The other pixels are appended to the work list: one atomic per 1024-thread
// workgroup (the waves' counts combined in LDS) -- one per wave on the single n_list counter
// serialised at L2: 49 us per frame for C2 and C3 alike.
// zero2: two words zeroed by the first thread (the wavefront forms' unit counters), saving a memset
// launch per frame.
constexpr int kClassifyBlock = 1024;
template <bool STATS>
__global__ __launch_bounds__(kClassifyBlock) void k_x_classify(DevScene sc, CamDev cam, TileMap m, int spp, double* rgb,
                                                     uint8_t* rgb8, unsigned* list, unsigned* n_list,
                                                     unsigned long long* stats, unsigned* zero2) {
    if (zero2 && blockIdx.x == 0 && threadIdx.x < 2) zero2[threadIdx.x] = 0u;
    const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    const long long lt = s >> 6;
    const int lane = threadIdx.x & 63;
    long long idx = -1;
    int x = 0, y = 0;
    bool scene = false, zero = false, bg = false;
    if (lt < m.n_local) {
        if (slot_pixel(m, lt, lane, idx, x, y)) {
            bg = pixel_misses_box(cam, x, y + m.y0, sc.root_lo, sc.root_hi);
            scene = !bg;
            zero = bg;
        } else {
            zero = idx >= 0 && m.shard_count > 1;   // padding slot of a packed tile
        }
    }
    if (zero) {
        if (rgb) { rgb[3 * idx] = 0; rgb[3 * idx + 1] = 0; rgb[3 * idx + 2] = 0; }
        if (rgb8) { rgb8[3 * idx] = 0; rgb8[3 * idx + 1] = 0; rgb8[3 * idx + 2] = 0; }
    }
    const unsigned long long ms = __ballot(scene && list != nullptr);   // (a progressive pass after the
    __shared__ unsigned s_cnt[kClassifyBlock / 64 + 1];                  //  first keeps the frame's list)
    const int wv = threadIdx.x >> 6;
    if (lane == 0) s_cnt[wv] = (unsigned)__popcll(ms);
    __syncthreads();
    if (threadIdx.x == 0) {   // exclusive offsets of the waves, then one atomic for the workgroup
        unsigned acc = 0;
        for (int k = 0; k < kClassifyBlock / 64; ++k) {
            const unsigned c = s_cnt[k];
            s_cnt[k] = acc;
            acc += c;
        }
        s_cnt[kClassifyBlock / 64] = acc ? atomicAdd(n_list, acc) : 0u;   // (acc > 0 only with a list)
    }
    __syncthreads();
    if (scene && list) list[s_cnt[kClassifyBlock / 64] + s_cnt[wv] + (unsigned)__popcll(ms & ((1ull << lane) - 1))] = (unsigned)s;
    if (STATS && (s & ~63ll) < m.n_local * 64) {
        wave_add_stats(stats, bg ? (uint64_t)spp : 0, 0, 0, bg ? 1 : 0);
        uint64_t r = bg ? (uint64_t)spp : 0;   // samples resolved here, without traversal
        for (int off = 32; off > 0; off >>= 1) r += __shfl_xor(r, off);
        if (lane == 0 && r) atomicAdd(stats + GI_STAT_X_RESOLVED, (unsigned long long)r);
    }
}

// Mode X pass 3 (spp > 1): a listed pixel's per-sample radiance added in sample order from +0, then
// min(sum / spp, 1) and the 8-bit store -- the oracle's operations (pixel_mode_x).  A progressive
// pass sums its frame's samples [0, s1): the frame of spp = s1, the one-shot frame for s1 = spp.
__global__ __launch_bounds__(256) void k_x_reduce(TileMap m, XWork wk, int spp, double* rgb, uint8_t* rgb8) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= *wk.n_list) return;
    const unsigned ps = wk.list[i];
    long long idx = -1;
    int x = 0, y = 0;
    slot_pixel(m, (long long)(ps >> 6), (int)(ps & 63), idx, x, y);
    double a = 0, b = 0, c = 0;
    const double* p = wk.part + 3 * (size_t)i * (size_t)spp;
    int s = 0;
    if ((spp & 1) == 0) {
        // even spp: the row is 16-byte aligned, so two samples (six doubles) come in three 16-byte
        // loads -- half the load instructions; the lanes' rows are 1.5 KB apart, so each load
        // instruction is 64 separate lines for the address unit, which bounds this kernel.  The
        // sums take the samples in the same order.
        const double2* q = reinterpret_cast<const double2*>(p);
        for (; s + 1 < wk.s1; s += 2) {
            const double2 v0 = q[3 * (s >> 1)], v1 = q[3 * (s >> 1) + 1], v2 = q[3 * (s >> 1) + 2];
            a = a + v0.x;
            b = b + v0.y;
            c = c + v1.x;
            a = a + v1.y;
            b = b + v2.x;
            c = c + v2.y;
        }
    }
    for (; s < wk.s1; ++s) {
        a = a + p[3 * s];
        b = b + p[3 * s + 1];
        c = c + p[3 * s + 2];
    }
    const double n = (double)wk.s1;
    const double c0 = smin(a / n, 1.0), c1 = smin(b / n, 1.0), c2 = smin(c / n, 1.0);
    if (rgb) { rgb[3 * idx] = c0; rgb[3 * idx + 1] = c1; rgb[3 * idx + 2] = c2; }
    if (rgb8) quantize(c0, c1, c2, rgb8 + 3 * idx);
}

// ---------------------------------------------------------------------------------------------
// Sample moments of the retained frame (gi.h "sample moments"; gi_frame_moments*): the per-sample radiance rows
// k_x_reduce sums, read again -- per listed pixel inside the window the mean of its first n rows (k_x_reduce's
// sum over n), the sample variance of that mean by a second pass over the rows (d = x - mean; m2 += d d, one
// multiply then one add), and the rows themselves.  Outputs are row-major over the window.  The pixels the
// classify pass did not list have no row: k_x_moments_fill writes their +0 (the same frustum test decides it, so
// the two kernels write disjoint pixels and together every pixel of the window).
// GI_MOMENTS_LDS: 1 the wave-cooperative form (a wave of 64 listed pixels loads their rows coalesced, a chunk of
// samples at a time, into padded LDS and every lane sums its own pixel from there); 0 one lane per listed pixel
// straight from global memory, k_x_reduce's access pattern (64 separate lines per load instruction).  Same sums in
// the same order.  A/B builds: build.py --variant NAME GI_MOMENTS_LDS=0|1 (DESIGN.md §9 "Sample moments").
// ---------------------------------------------------------------------------------------------
#ifndef GI_MOMENTS_LDS
#define GI_MOMENTS_LDS 0   // (the plain form won the A/B on the device)
#endif
struct XMoments {
    const unsigned* list;    // the retained frame's work list and its count (k_x_classify's)
    const unsigned* n_list;
    const double* part;      // its rows [list index][sample][3], row stride spp samples
    int spp, n;              // the frame's spp; the samples rendered so far (2 <= n <= spp)
    int x0, y0, cols, rows;  // the window
    double *mean, *var, *samples;   // each may be null
};

// the window index of listed pixel i, -1 outside the window
__device__ __forceinline__ long long moments_pixel(const TileMap& m, const XMoments& a, unsigned i) {
    const unsigned ps = a.list[i];
    long long idx = -1;
    int x = 0, y = 0;
    slot_pixel(m, (long long)(ps >> 6), (int)(ps & 63), idx, x, y);
    x -= a.x0;
    y -= a.y0;
    return (x >= 0 && x < a.cols && y >= 0 && y < a.rows) ? (long long)y * (long long)a.cols + (long long)x : -1;
}
__device__ __forceinline__ void moments_store(const XMoments& a, long long o, double sa, double sb, double sc, double va, double vb,
                                              double vc, bool second) {
    const double n = (double)a.n;
    if (!second) {
        if (a.mean) { a.mean[3 * o] = sa; a.mean[3 * o + 1] = sb; a.mean[3 * o + 2] = sc; }
    } else if (a.var) {
        const double n1 = (double)(a.n - 1);
        a.var[3 * o] = (va / n1) / n;
        a.var[3 * o + 1] = (vb / n1) / n;
        a.var[3 * o + 2] = (vc / n1) / n;
    }
}

#if !GI_MOMENTS_LDS
__global__ __launch_bounds__(256) void k_x_moments(TileMap m, XMoments a) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= *a.n_list) return;
    const long long o = moments_pixel(m, a, i);
    if (o < 0) return;
    const double* p = a.part + 3 * (size_t)i * (size_t)a.spp;
    // even spp: the row is 16-byte aligned and two samples come in three 16-byte loads, as in k_x_reduce (half the
    // load instructions); the sums take the samples in the same order
    const double2* q = reinterpret_cast<const double2*>(p);
    const bool pairs = (a.spp & 1) == 0;
    double sa = 0, sb = 0, sc = 0;
    int s = 0;
    if (pairs) {
        for (; s + 1 < a.n; s += 2) {
            const double2 v0 = q[3 * (s >> 1)], v1 = q[3 * (s >> 1) + 1], v2 = q[3 * (s >> 1) + 2];
            sa = sa + v0.x;
            sb = sb + v0.y;
            sc = sc + v1.x;
            sa = sa + v1.y;
            sb = sb + v2.x;
            sc = sc + v2.y;
        }
    }
    for (; s < a.n; ++s) {
        sa = sa + p[3 * s];
        sb = sb + p[3 * s + 1];
        sc = sc + p[3 * s + 2];
    }
    const double n = (double)a.n;
    const double ma = sa / n, mb = sb / n, mc = sc / n;
    moments_store(a, o, ma, mb, mc, 0, 0, 0, false);
    if (!a.var && !a.samples) return;
    double* out = a.samples ? a.samples + 3 * (size_t)o * (size_t)a.n : nullptr;
    double va = 0, vb = 0, vc = 0;
    const auto take = [&](int k, double x0, double x1, double x2) {
        const double da = x0 - ma, db = x1 - mb, dc = x2 - mc;
        va = va + da * da;
        vb = vb + db * db;
        vc = vc + dc * dc;
        if (out) { out[3 * k] = x0; out[3 * k + 1] = x1; out[3 * k + 2] = x2; }
    };
    s = 0;
    if (pairs) {
        for (; s + 1 < a.n; s += 2) {
            const double2 v0 = q[3 * (s >> 1)], v1 = q[3 * (s >> 1) + 1], v2 = q[3 * (s >> 1) + 2];
            take(s, v0.x, v0.y, v1.x);
            take(s + 1, v1.y, v2.x, v2.y);
        }
    }
    for (; s < a.n; ++s) take(s, p[3 * s], p[3 * s + 1], p[3 * s + 2]);
    moments_store(a, o, 0, 0, 0, va, vb, vc, true);
}
#else
// A workgroup is one wave and takes listed pixels [64 b, 64 b + 64).  Their rows lie one behind the other in
// `part`, so a chunk of kMomChunk samples of all 64 is 64 runs of 3 kMomChunk doubles: consecutive lanes load
// consecutive doubles of a run.  In LDS a pixel's chunk takes kMomRow = 3 kMomChunk + 1 doubles: the odd stride
// puts the lanes' rows on different banks when each reads its own row at the same offset.
constexpr int kMomChunk = 8, kMomRow = 3 * kMomChunk + 1;
__global__ __launch_bounds__(64) void k_x_moments(TileMap m, XMoments a) {
    __shared__ double s_row[64 * kMomRow];
    const unsigned n_list = *a.n_list, base = blockIdx.x * 64u;
    if (base >= n_list) return;
    const unsigned cnt = n_list - base < 64u ? n_list - base : 64u;
    const unsigned lane = threadIdx.x;
    const long long o = lane < cnt ? moments_pixel(m, a, base + lane) : -1;
    if (!__syncthreads_or(o >= 0)) return;   // none of the wave's pixels is in the window
    const double* rows = a.part + 3 * (size_t)base * (size_t)a.spp;
    const double* mine = s_row + lane * kMomRow;
    const double n = (double)a.n;
    double sa = 0, sb = 0, sc = 0, ma = 0, mb = 0, mc = 0;
    double* out = (a.samples && o >= 0) ? a.samples + 3 * (size_t)o * (size_t)a.n : nullptr;
    for (int pass = 0; pass < 2; ++pass) {   // 0: the sums of the mean; 1: of the variance, and the rows' copy
        if (pass == 1 && !a.var && !a.samples) break;
        for (int s0 = 0; s0 < a.n; s0 += kMomChunk) {
            const unsigned cn = (unsigned)(a.n - s0 < kMomChunk ? a.n - s0 : kMomChunk), per = 3u * cn, total = cnt * per;
            for (unsigned e = lane; e < total; e += 64u) {
                const unsigned px = e / per, k = e - px * per;
                s_row[px * kMomRow + k] = rows[3 * ((size_t)px * (size_t)a.spp + (size_t)s0) + k];
            }
            __syncthreads();
            if (o >= 0) {
                for (unsigned k = 0; k < cn; ++k) {
                    const double x0 = mine[3 * k], x1 = mine[3 * k + 1], x2 = mine[3 * k + 2];
                    if (pass == 0) {
                        sa = sa + x0;
                        sb = sb + x1;
                        sc = sc + x2;
                    } else {
                        const double da = x0 - ma, db = x1 - mb, dc = x2 - mc;
                        sa = sa + da * da;
                        sb = sb + db * db;
                        sc = sc + dc * dc;
                        if (out) { out[3 * (s0 + k)] = x0; out[3 * (s0 + k) + 1] = x1; out[3 * (s0 + k) + 2] = x2; }
                    }
                }
            }
            __syncthreads();
        }
        if (pass == 0) {
            ma = sa / n; mb = sb / n; mc = sc / n;
            if (o >= 0) moments_store(a, o, ma, mb, mc, 0, 0, 0, false);
            sa = sb = sc = 0;
        } else if (o >= 0) {
            moments_store(a, o, 0, 0, 0, sa, sb, sc, true);
        }
    }
}
#endif

// the window's pixels without a row: +0 in every output
__global__ __launch_bounds__(256) void k_x_moments_fill(DevScene sc, CamDev cam, XMoments a) {
    const long long n_px = (long long)a.cols * (long long)a.rows;
    for (long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x; o < n_px; o += (long long)gridDim.x * blockDim.x) {
        const int y = (int)(o / a.cols), x = (int)(o - (long long)y * a.cols);
        if (!pixel_misses_box(cam, x + a.x0, y + a.y0, sc.root_lo, sc.root_hi)) continue;
        if (a.mean) { a.mean[3 * o] = 0; a.mean[3 * o + 1] = 0; a.mean[3 * o + 2] = 0; }
        if (a.var) { a.var[3 * o] = 0; a.var[3 * o + 1] = 0; a.var[3 * o + 2] = 0; }
        if (a.samples) {
            double* out = a.samples + 3 * (size_t)o * (size_t)a.n;
            for (int k = 0; k < 3 * a.n; ++k) out[k] = 0;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// unshard: packed per-rank tiles -> row-major frame
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_unshard(TileMap m, const double* packed, const uint8_t* packed8, double* rgb,
                                                  uint8_t* rgb8) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;   // global pixel slot in tile order
    const long long t = i / (kTile * kTile);
    if (t >= m.n_tiles) return;
    const int lane = (int)(i % (kTile * kTile));
    const int ty = (int)(t / m.tiles_x), tx = (int)(t % m.tiles_x);
    const int x = tx * kTile + (lane & 7), y = ty * kTile + (lane >> 3);
    if (x >= m.w || y >= m.h) return;
    const long long r = t % m.shard_count, lt = t / m.shard_count;
    const long long src = (r * m.n_local + lt) * (kTile * kTile) + lane;
    const long long dst = (long long)y * m.w + x;
    if (rgb) { rgb[3 * dst] = packed[3 * src]; rgb[3 * dst + 1] = packed[3 * src + 1]; rgb[3 * dst + 2] = packed[3 * src + 2]; }
    if (rgb8) { rgb8[3 * dst] = packed8[3 * src]; rgb8[3 * dst + 1] = packed8[3 * src + 1]; rgb8[3 * dst + 2] = packed8[3 * src + 2]; }
}


}  // namespace

long long shard_tiles(int w, int h, int shard_count) { return make_map(w, h, shard_count, 0).n_local; }

const XEnv& x_env() {   // (the knobs: gi_launch.h XEnv)
    static XEnv env;
    static std::once_flag once;
    std::call_once(once, [] {
        if (const char* v = std::getenv("GI_X_HELP")) env.help = std::atoi(v) != 0;
        if (const char* v = std::getenv("GI_X_FLAT")) env.flat = std::atoi(v) != 0;
        if (const char* v = std::getenv("GI_X_FAN")) env.fan = std::atoi(v) != 0;
        if (const char* v = std::getenv("GI_SEG_RING")) env.seg_ring = std::atoi(v) != 0;
        if (const char* v = std::getenv("GI_R_FLAT")) env.r_flat = std::atoi(v);
        if (const char* v = std::getenv("GI_RF_PER_SLOT")) env.rf_per_slot = std::max(0, std::min(1024, std::atoi(v)));
        if (const char* v = std::getenv("GI_X_WF")) env.wf = std::atoi(v);
        if (const char* v = std::getenv("GI_RF_GROUP")) env.rf_group = (std::atoi(v) == 1 || std::atoi(v) == 4) ? std::atoi(v) : 0;
        const char* v = std::getenv("GI_X_MAX_RUN");
        const int r = v ? std::max(1, std::min(128, std::atoi(v))) : GI_X_MAX_RUN;
        int lg = 0;
        while ((2 << lg) <= r) ++lg;
        env.run_log2 = lg;
    });
    return env;
}

#ifndef GI_WF_MAX_DEPTH
#define GI_WF_MAX_DEPTH 64   // the wavefront form launches once per bounce: deeper paths run k_mode_x
#endif
// Mode X form of a launch (XForm).  GI_FLAG_X_MEGA / _WF / _SEG force one (tests, A/B), then GI_X_WF=0/1/2.
// By default: scenes staged in LDS run k_seg (C3 5.8 -> 5.2 ms, C2 0.29 ->
// 0.15-0.17 ms; short traversals, so a wave's lanes finish a segment together); large HBM-resident scenes
// keep k_mode_x, whose lanes refill independently (C4: k_seg 3.2 against 1.7 ms -- one long traversal
// would hold its whole wave).  The wavefront form loses everywhere (queue traffic and its atomics: C3
// 12.5-20 ms); it stays selectable.
XForm x_form_choice(const DevScene& sc, const XLaunchCfg& xc, const gi_opts& o) {
    if (o.mode != GI_MODE_X || (o.flags & GI_FLAG_X_MEGA)) return XFORM_MEGA;
    if (o.flags & GI_FLAG_X_SEG) return XFORM_SEG;
    const XForm wf = o.depth <= GI_WF_MAX_DEPTH ? XFORM_WF : XFORM_MEGA;
    if (o.flags & GI_FLAG_X_WF) return wf;
    const XEnv& env = x_env();
    if (env.wf >= 0) return env.wf == XFORM_WF ? wf : env.wf == XFORM_SEG ? XFORM_SEG : XFORM_MEGA;
    // small HBM-resident trees (<= 1 MB of wide nodes: L2-resident, short traversals -- X-zoo 5.7 ->
    // 4.8-5.0 ms, the 1k soup even) run k_seg too
    return (xc.var.lds || (size_t)sc.n_xwnodes * sizeof(XWNode) <= ((size_t)1 << 20)) ? XFORM_SEG : XFORM_MEGA;
}

namespace {
// The k_mode_x instantiation a launch runs: f(kernel) for the scene and the launch's handoff choice --
// STATS x HELP x CN x SH x TR, the 32 instantiations of the library.  A scene staged in LDS has no
// quantised nodes, so it runs the wide-node ones.
template <typename F>
void x_dispatch(const DevScene& sc, bool help, bool stats, F&& f) {
    with_bools([&](auto S, auto HP, auto C, auto H, auto T) { f(&k_mode_x<S.value, HP.value, C.value, H.value, T.value>); },
               stats, help, sc.xcnodes != nullptr, sc.x_max_depth <= 7, sc.x_tri_only != 0);
}

// An adaptive pass's work as the kernels of a form take it (launch_adaptive): the list of the active pixel slots and
// its device count in the work list's place, and the rows pointer biased by -3 s0 doubles, so that with the stride
// o.spp = k sample s of active entry i lands at rows[i][s - s0] (only such in-bounds addresses are dereferenced).
struct XPassWork {
    unsigned* list;
    unsigned* n_list;
    double* part;
};

// launch_render's Mode X half: classify, the form's pass between ev_begin and ev_end, reduce.  pw (an adaptive pass):
// the form's kernels run over pw's list; classify fills it on the frame's first pass and is not run on a later one
// (no pixel is written here: rgb and rgb8 are null), and the rows are left to k_x_adapt_fold instead of k_x_reduce.
hipError_t launch_mode_x(const DevScene& sc, const XLaunchCfg& xc, const CamDev& cam, V3 light, const TileMap& m,
                         const gi_opts& o, double* rgb, uint8_t* rgb8, const XScratch& xs, hipStream_t stream,
                         hipEvent_t ev_begin, hipEvent_t ev_end, const XPassWork* pw = nullptr) {
    const dim3 block(64 * kWavesPerBlock);
    unsigned long long* st = reinterpret_cast<unsigned long long*>(o.stats);
    const bool stats = (o.flags & GI_FLAG_STATS) && st;
    // persistent grid: as many 4-wave blocks as can be resident (xc, per scene), each wave pulls
    // blocks of work units
    const XEnv& env = x_env();
    const long long n_slots = m.n_local * (kTile * kTile);
    // the shadow-ray handoff build (and spread work groups) for launches of
    // at most 32 samples per resident lane -- their time is the longest paths' latency and lanes
    // run out of work early (C4: 10 per lane; X-soup1000, 169 per lane, is throughput-bound and
    // 25% slower spread)
    const bool help = env.help && n_slots * (long long)o.spp <= 32ll * 256ll * (long long)xc.resident;
    // up to one lane per (pixel slot, sample): single-sample units can occupy that many lanes
    const long long want = (n_slots * (long long)o.spp / 64 + kWavesPerBlock - 1) / kWavesPerBlock;
    const dim3 pgrid((unsigned)std::max<long long>(1, std::min<long long>(want, xc.resident)));
    if (!xs.list || (unsigned long long)xs.cap < (unsigned long long)n_slots || (o.spp > 1 && (!xs.part || xs.spp < o.spp)))
        return hipErrorInvalidValue;
    // the launch's samples: the whole spp, or a progressive pass [sample_begin, sample_end) -- a pass
    // after the first continues the frame: its work list (and count, work[1]) and the earlier
    // passes' per-sample rows stay; classify only rewrites the background pixels
    const int s0 = o.sample_end > 0 ? o.sample_begin : 0, s1 = o.sample_end > 0 ? o.sample_end : o.spp;
    const bool cont = s0 > 0;
    hipError_t e = hipMemsetAsync(sc.work, 0, (cont ? 1 : 16) * sizeof(unsigned), stream);
    if (e == hipSuccess && cont) e = hipMemsetAsync(sc.work + 2, 0, 14 * sizeof(unsigned), stream);
    if (e != hipSuccess) return e;
    unsigned* const n_list = pw ? pw->n_list : sc.work + 1;
    const XWork wk{pw ? pw->list : xs.list, n_list, pw ? pw->part : xs.part, sc.work, s0, s1};   // (list, its count, rows, block counter, samples)
    const dim3 sgrid((unsigned)((n_slots + 255) / 256));
    const dim3 cgrid((unsigned)((n_slots + kClassifyBlock - 1) / kClassifyBlock));
    const XForm form = x_form_choice(sc, xc, o);
    unsigned* zero2 = form == XFORM_SEG ? xs.wcnt : nullptr;   // k_seg's unit counter, zeroed by the classify pass
    unsigned* cl = cont ? nullptr : pw ? pw->list : xs.list;
    if (pw && cont && !stats) {   // (an adaptive pass after the first: only k_seg's unit counter, which classify would zero;
                                  //  with GI_FLAG_STATS classify runs for the resolved pixels' counts, as in a progressive pass)
        if (zero2 && (e = hipMemsetAsync(zero2, 0, 2 * sizeof(unsigned), stream)) != hipSuccess) return e;
    } else {
        with_bools([&](auto S) {
            hipLaunchKernelGGL(k_x_classify<S.value>, cgrid, dim3(kClassifyBlock), 0, stream, sc, cam, m, s1 - s0, rgb, rgb8, cl, n_list, st, zero2);
        }, stats);
    }
    // shading-handler threshold (eighths of the live lanes that must wait): the builder's
    // estimate for the scene (DevScene::x_handle8)
    const int h8 = sc.x_handle8;
    // schedule flags (XFlag, gi_scene.h): the scene's, the launch's and the maximum run length (log2)
    const int xf = sc.x_flags | (env.run_log2 << XF_RUN_SHIFT) | ((o.flags & GI_FLAG_X_NO_SHADOW) ? XF_NO_SHADOW : 0) |
                   (env.help ? XF_HANDOFF : 0) | (help ? XF_SPREAD : 0) | XF_PIXEL_MAJOR | (env.flat ? 0 : XF_NO_FLAT) |
                   (xc.seg_ring ? XF_SEG_RING : 0);
    if (form != XFORM_MEGA) {   // gi_wf.hip's forms, timed as one pass
        if (!xs.wcnt || (form == XFORM_WF && (!xs.wq[0] || !xs.wq[1] || xs.wcap <= 0))) return hipErrorInvalidValue;
        const bool seg = form == XFORM_SEG;
        const XKernelCfg c{xc.var, env.flat != 0, seg ? xc.seg_lds_bytes : xc.wf_lds_bytes, xc.wf_grid[seg ? WK_SEG : WK_BOUNCE]};
        XScratch xw = xs;   // (gi_wf.hip's forms read the list and the rows from the scratch record)
        if (pw) {
            xw.list = pw->list;
            xw.part = pw->part;
        }
        e = launch_wf(sc, c, form, cam, light, m.w, m.h, m.y0, o, rgb, rgb8, xw, n_list, stats ? st : nullptr, xf,
                      x_launch_live(sc, xc, cam.pos, light, o.flags), stream,
                      ev_begin, ev_end);
        if (e != hipSuccess) return e;
    } else {
        if (ev_begin) (void)hipEventRecord(ev_begin, stream);
        x_dispatch(sc, help, stats, [&](auto kernel) {
            hipLaunchKernelGGL(kernel, pgrid, block, xc.lds_bytes, stream, sc, cam, light, m, o.spp, o.depth, o.seed, rgb, rgb8, st, wk,
                               h8, xf);
        });
        if (ev_end) (void)hipEventRecord(ev_end, stream);
    }
    if (o.spp > 1 && !pw) hipLaunchKernelGGL(k_x_reduce, sgrid, dim3(256), 0, stream, m, wk, o.spp, rgb, rgb8);
    return hipSuccess;
}
}  // namespace

// One adaptive pass (gi_launch.h XAdaptPass): o.spp is the pass's k.  The grids, the handoff choice, k_seg's unit
// counter and the wavefront chunks all follow the frame's slots x k (the active count stays on the device; what lies
// past it returns at once there), none of them the frame's spp.
hipError_t launch_adaptive(const DevScene& sc, const XLaunchCfg& xc, const CamDev& cam, V3 light, int w, int h,
                           const gi_opts& o, const XAdaptPass& ap, const XScratch& xs, KTimer* kt, hipStream_t stream) {
    const int s0 = o.sample_begin, s1 = o.sample_end, k = s1 - s0;
    const TileMap m = make_map(w, h, 1, 0);
    const long long n_slots = m.n_local * (kTile * kTile);
    if (o.mode != GI_MODE_X || o.shard_count != 1 || k < 2 || o.spp != k || s0 < 0 || s1 > ap.spp_max || !xs.list || !xs.part ||
        !xs.ad_list || !xs.ad_cnt || !xs.ad_sum || !xs.ad_n || xs.cap < n_slots || xs.ad_cap < n_slots || xs.spp < k || (ap.cur & ~1))
        return hipErrorInvalidValue;
    const bool timed = (o.flags & GI_FLAG_TIME) && kt && kt->ev0[0];
    const int slot = timed ? (int)(kt->recorded % KTimer::kRing) : 0;
    hipEvent_t ev_begin = timed ? static_cast<hipEvent_t>(kt->ev0[slot]) : nullptr;
    hipEvent_t ev_end = timed ? static_cast<hipEvent_t>(kt->ev1[slot]) : nullptr;
    // the counts: on the first pass both are zeroed (classify counts list 0 up), later the survivors' alone
    hipError_t e = s0 == 0 ? hipMemsetAsync(xs.ad_cnt, 0, 2 * sizeof(unsigned), stream)
                           : hipMemsetAsync(xs.ad_cnt + (ap.cur ^ 1), 0, sizeof(unsigned), stream);
    if (e != hipSuccess) return e;
    if (s0 == 0 && ap.cur != 0) return hipErrorInvalidValue;
    XPassWork pw;
    pw.list = ap.cur ? xs.ad_list : xs.list;
    pw.n_list = xs.ad_cnt + ap.cur;
    pw.part = xs.part - 3 * (ptrdiff_t)s0;
    if ((e = launch_mode_x(sc, xc, cam, light, m, o, nullptr, nullptr, xs, stream, ev_begin, ev_end, &pw)) != hipSuccess) return e;
    if (s0 == 0 && (e = launch_adapt_init(sc, cam, w, h, xs, stream)) != hipSuccess) return e;
    if ((e = launch_adapt_fold(w, h, s0, s1, ap, xs, stream)) != hipSuccess) return e;
    if (timed) kt->recorded++;
    return hipGetLastError();
}

hipError_t x_launch_config(const DevScene& sc, int device, XLaunchCfg& cfg) {
    const bool lds = sc.x_lds_bytes > 0;   // (gi_wf.hip's kernels; k_mode_x reads every scene from global memory)
    cfg.lds_bytes = 16 * 256 * sizeof(int) + 256 * (7 * sizeof(double) + 2 * sizeof(int));   // level stack, handoff slots
    cfg.var = XVariant{lds, lds && sc.x_waves4};
    int cus = 0, per_cu = 0;
    hipError_t e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
    if (e != hipSuccess) return e;
    // the scene's own instantiation, STATS and handoff off (neither moves the occupancy: DESIGN.md §5)
    x_dispatch(sc, false, false, [&](auto kernel) {
        e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(kernel), 64 * kWavesPerBlock,
                                                         cfg.lds_bytes);
    });
    if (e != hipSuccess) return e;
    cfg.resident = std::max(1, cus) * std::max(1, per_cu);
    const bool flat = sc.x_flat && x_env().flat;   // (the launches' choice: launch_render's XF_NO_FLAT)
    cfg.wf_lds_bytes = wf_lds_bytes(sc, lds, flat);
    cfg.wf_tree_lds_bytes = wf_lds_bytes(sc, lds, false);
    int wf_per_cu[WK_COUNT] = {};
    for (int k = 0; k < WK_COUNT; ++k) {   // (WK_SEG_RING: with the ring's LDS behind the other kernels' bytes)
        const XKernelCfg c{cfg.var, flat, cfg.wf_lds_bytes + (k == WK_SEG_RING ? wf_seg_ring_bytes() : 0), 0};
        e = wf_occupancy(sc, (WfKernel)k, c, &wf_per_cu[k]);
        if (e != hipSuccess) return e;
        cfg.wf_grid[k] = std::max(1, cus) * std::max(1, wf_per_cu[k]);
    }
    // k_seg's per-wave ring of prepared primary rays (gi_wf.hip): only where its LDS leaves the kernel's
    // resident workgroups per CU as they are -- fewer waves cost more than the ring saves.  GI_SEG_RING=0
    // (tests): never
    cfg.seg_ring = x_env().seg_ring && wf_per_cu[WK_SEG_RING] >= wf_per_cu[WK_SEG] && wf_per_cu[WK_SEG] >= 1;
    cfg.seg_lds_bytes = cfg.wf_lds_bytes + (cfg.seg_ring ? wf_seg_ring_bytes() : 0);
    return hipSuccess;
}

hipError_t launch_render(const DevScene& sc, const XLaunchCfg& xc, const CamDev& cam, V3 light, int w, int h, int y0,
                         const gi_opts& o, double* rgb, uint8_t* rgb8, const XScratch& xs, KTimer* kt,
                         hipStream_t stream) {
    // GI_FLAG_TIME: events on the launch stream around the dominant kernel only (slot chosen by
    // the caller, gi_capi.cpp, which folds a reused pair before this call)
    const bool timed = (o.flags & GI_FLAG_TIME) && kt && kt->ev0[0];
    const int slot = timed ? (int)(kt->recorded % KTimer::kRing) : 0;
    hipEvent_t ev_begin = timed ? static_cast<hipEvent_t>(kt->ev0[slot]) : nullptr;
    hipEvent_t ev_end = timed ? static_cast<hipEvent_t>(kt->ev1[slot]) : nullptr;
    const TileMap m = make_map(w, h, o.shard_count, o.shard_index, y0);
    if (m.n_local == 0) return hipSuccess;
    const hipError_t e = o.mode == GI_MODE_R ? launch_mode_r(sc, cam, light, w, h, y0, o, rgb, rgb8, xs, stream, ev_begin, ev_end)
                                             : launch_mode_x(sc, xc, cam, light, m, o, rgb, rgb8, xs, stream, ev_begin, ev_end);
    if (e != hipSuccess) return e;
    if (timed) kt->recorded++;
    return hipGetLastError();
}

hipError_t launch_unshard(int w, int h, int shard_count, const double* packed, const uint8_t* packed8, double* rgb,
                          uint8_t* rgb8, hipStream_t stream) {
    const TileMap m = make_map(w, h, shard_count, 0);
    const long long n = m.n_tiles * kTile * kTile;
    hipLaunchKernelGGL(k_unshard, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream, m, packed, packed8, rgb, rgb8);
    return hipGetLastError();
}

// gi_frame_moments_device's launches on `stream`: the fill of the window's unlisted pixels, then k_x_moments over
// the slots of the whole w x h frame (the work list's length is on the device; slots past it return at once).
hipError_t launch_moments(const DevScene& sc, const XScratch& xs, const CamDev& cam, int w, int h, const MomentsIO& io,
                          hipStream_t stream) {
    const TileMap m = make_map(w, h, 1, 0);
    const long long n_slots = m.n_local * (kTile * kTile);
    if (!xs.list || !xs.part || xs.cap < n_slots || xs.spp < io.spp || io.n < 2 || io.n > io.spp) return hipErrorInvalidValue;
    const XMoments a{xs.list, sc.work + 1, xs.part, io.spp, io.n, io.x0, io.y0, io.cols, io.rows, io.mean, io.var, io.samples};
    const long long n_px = (long long)io.cols * (long long)io.rows;
    const long long fgrid = std::min<long long>((n_px + 255) / 256, 1ll << 20);
    hipLaunchKernelGGL(k_x_moments_fill, dim3((unsigned)fgrid), dim3(256), 0, stream, sc, cam, a);
    const int block = GI_MOMENTS_LDS ? 64 : 256;
    hipLaunchKernelGGL(k_x_moments, dim3((unsigned)((n_slots + block - 1) / block)), dim3(block), 0, stream, m, a);
    return hipGetLastError();
}

}  // namespace gi
