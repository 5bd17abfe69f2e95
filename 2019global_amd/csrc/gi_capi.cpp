// gi_capi.cpp — the extern "C" boundary (include/gi.h).  Host-side only: validates arguments,
// builds the scene (gi_build.cpp), owns its HBM copy, and launches the gfx950 kernels
// (gi_launch.h).  There is no CPU rendering path: without a gfx950 device every render fails.
// No exception crosses the boundary: every entry point that can allocate runs inside guard(),
// which maps std::bad_alloc to GI_ERR_NOMEM and anything else to GI_ERR_INTERNAL.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "gi.h"
#include "gi_internal.h"
#include "gi_launch.h"
#include "gi_scene.h"

using namespace gi;

// gi_render's band pipeline, owned by the scene handle and created on first use: band i renders
// into device slot i % 2 on `render` while band i-1 is copied to pinned staging on `copy`; the
// host then copies a finished band into the caller's buffers (or hands the staging to the
// callback).  Slots are reused only after their copy has completed (event `copied`).
struct HostPath {
    static constexpr int kSlots = 2;
    hipStream_t render = nullptr, copy = nullptr;
    hipEvent_t rendered[kSlots] = {}, copied[kSlots] = {};
    double* d_rgb[kSlots] = {};
    uint8_t* d_rgb8[kSlots] = {};
    double* h_rgb[kSlots] = {};    // pinned
    uint8_t* h_rgb8[kSlots] = {};  // pinned
    size_t cap_px = 0;             // pixels per slot
    int n_alloc = 0;               // slots allocated (1 for whole-frame renders)
};

struct gi_scene {
    HostScene host;
    DevScene dev;
    XLaunchCfg xcfg;   // Mode X launch configuration on this scene's device
    std::vector<void*> allocs;
    XScratch xs;       // Mode X work list + per-sample radiance, grown on demand
    KTimer kt;         // GI_FLAG_TIME events
    HostPath hp;       // gi_render's band pipeline (streams, device band slots, pinned staging)
    // every render launch of this scene waits on the device for the previous one (they share xs
    // and the work counters), whatever stream each is issued on
    hipEvent_t last = nullptr;
    bool launched = false;
    uint64_t prog_key = 0;   // progressive passes: the frame's key and the next pass's sample_begin
    int prog_next = -1;
    // the retained frame (gi.h "sample moments"): the last render, if it was a whole Mode X frame with spp > 1 on
    // one shard and was issued successfully -- its size, the samples rendered so far (0: no retained frame), the
    // rows' stride and its camera (k_x_moments_fill repeats the classify pass's test)
    int keep_w = 0, keep_h = 0, keep_n = 0, keep_spp = 0;
    CamDev keep_cam;
    // the adaptive frame (gi.h "adaptive sampling"): its key (prog_key's, with the gi_adaptive_params), the next
    // pass's sample_begin (-1: no pass can continue it), which of the two lists that pass reads, and what
    // gi_adaptive_info reports (ad_done 0: no adaptive frame).  Any other render of the scene ends it.
    uint64_t ad_key = 0;
    int ad_next = -1, ad_cur = 0;
    int ad_w = 0, ad_h = 0, ad_done = 0;
    std::mutex mu;     // host-side calls on one scene are serialised
    int device = -1;
    int64_t bytes = 0;
};

struct gi_octree {
    HostScene host;
};

namespace {
thread_local std::string g_err;

int fail(int code, const char* msg) noexcept {
    try {
        g_err = msg;
    } catch (...) {
        // the message is best effort; the status code is what the caller acts on
    }
    return code;
}
int fail(int code, const std::string& msg) noexcept { return fail(code, msg.c_str()); }
int hip_fail(hipError_t e, const char* what) noexcept {
    try {
        return fail(GI_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
    } catch (...) {
        return GI_ERR_DEVICE;
    }
}

template <typename T>
hipError_t upload(gi_scene* s, const std::vector<T>& v, const T** out) {
    *out = nullptr;
    const size_t bytes = std::max<size_t>(v.size() * sizeof(T), 16);
    void* p = nullptr;
    hipError_t e = hipMalloc(&p, bytes);
    if (e != hipSuccess) return e;
    s->allocs.push_back(p);
    s->bytes += (int64_t)bytes;
    if (!v.empty()) {
        e = hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice);
        if (e != hipSuccess) return e;
    }
    *out = static_cast<const T*>(p);
    return hipSuccess;
}

void free_rflat(XScratch& x) {
    for (void* p : {(void*)x.rf_pairs, (void*)x.rf_pt, (void*)x.rf_best, (void*)x.rf_dir, (void*)x.rf_cnt, (void*)x.rf_ovf,
                    (void*)x.rf_rcnt, (void*)x.rf_soff, (void*)x.rf_shc, (void*)x.rf_sreg, (void*)x.rf_hoff})
        (void)hipFree(p);
    x.rf_pairs = x.rf_pt = x.rf_cnt = x.rf_ovf = x.rf_rcnt = x.rf_soff = x.rf_shc = x.rf_sreg = x.rf_hoff = nullptr;
    x.rf_best = nullptr;
    x.rf_dir = nullptr;
    x.rf_pages = 0;
    x.rf_slots = 0;
    x.rf_bytes = 0;
}

// Mode X work buffers for a frame of w x h pixels cut into this call's shard (k_x_classify's list,
// k_mode_x's per-sample radiance for spp > 1); grown, never shrunk.  hipFree synchronises with
// work still using them.
int ensure_xscratch(gi_scene* s, int w, int h, const gi_opts* o) {
    const long long need = shard_tiles(w, h, o->shard_count) * GI_TILE * GI_TILE;
    hipError_t e;
    if (o->mode == GI_MODE_R) {
        // the flat Mode R phases' buffers, only when this launch runs them (r_kernel_choice: RK_FLAT).
        // Pairs are one word: per tile its own GI_RF_S0 (8 per pixel slot), plus a shared pool of
        // GI_RF_PER_SLOT (16) per pixel slot in pages; with the per-slot directions and best ranks a
        // 1080p frame takes 0.28 GB (R-C4 writes 5.0 M pairs: 20 MB).  A tile whose candidates do not
        // fit is rendered by k_mode_r_batch; if the buffers cannot be had at all, the whole frame is.
        XScratch& x = s->xs;
        if (r_kernel_choice(s->dev, *o) == RK_FLAT && x.rf_slots < need && !(x.rf_failed > 0 && need >= x.rf_failed)) {
            free_rflat(x);
            const hipError_t prior = hipPeekAtLastError();   // (a caller's unchecked error is left as it was)
            const long long tiles = need / 64;
            const long long pages = (long long)x_env().rf_per_slot * need / (long long)rf_page_pairs();
            const size_t pairs = (size_t)tiles * rf_own_pairs() + (size_t)pages * rf_page_pairs();
            // segments of k_rf_hit: a tile's pairs cut every rf_seg_pairs(), so at most one per tile
            // plus one per rf_seg_pairs() of the buffer
            const size_t segs = (size_t)tiles + pairs / rf_seg_pairs() + 1;
            const bool ok =
                hipMalloc((void**)&x.rf_pairs, pairs * sizeof(unsigned)) == hipSuccess &&
                hipMalloc((void**)&x.rf_pt, (size_t)tiles * rf_max_pages() * sizeof(unsigned)) == hipSuccess &&
                hipMalloc((void**)&x.rf_best, (size_t)need * sizeof(unsigned long long)) == hipSuccess &&
                hipMalloc((void**)&x.rf_dir, (size_t)need * 3 * sizeof(double)) == hipSuccess &&
                hipMalloc((void**)&x.rf_cnt, 8 * sizeof(unsigned)) == hipSuccess &&
                hipMalloc((void**)&x.rf_ovf, (size_t)tiles * sizeof(unsigned)) == hipSuccess &&
                hipMalloc((void**)&x.rf_rcnt, (size_t)tiles * sizeof(unsigned)) == hipSuccess &&
                hipMalloc((void**)&x.rf_soff, (size_t)(tiles + 1) * sizeof(unsigned)) == hipSuccess &&
                hipMalloc((void**)&x.rf_shc, (size_t)segs * sizeof(unsigned)) == hipSuccess &&
                hipMalloc((void**)&x.rf_sreg, (size_t)segs * sizeof(unsigned)) == hipSuccess &&
                hipMalloc((void**)&x.rf_hoff, (size_t)(segs + 1) * sizeof(unsigned)) == hipSuccess;
            if (!ok) {   // rendered by k_mode_r_batch (gi_scene_r_kernel reports 2); not retried per frame
                if (prior == hipSuccess) (void)hipGetLastError();   // (clears this allocation's error only)
                free_rflat(x);
                x.rf_failed = need;
                return GI_OK;
            }
            x.rf_failed = 0;
            x.rf_pages = (unsigned)pages;
            x.rf_slots = need;
            x.rf_bytes = pairs * sizeof(unsigned) + (size_t)tiles * (rf_max_pages() + 4) * sizeof(unsigned) + segs * 12 +
                         (size_t)need * (sizeof(unsigned long long) + 3 * sizeof(double));
        }
        return GI_OK;
    }
    if (o->mode != GI_MODE_X) return GI_OK;
    if ((unsigned long long)need >= 0xFFFFFFFFull) return fail(GI_ERR_ARG, "mode X frame too large: 2^32 pixel slots");
    XScratch& x = s->xs;
    if (x.cap < need) {
        (void)hipFree(x.list);
        (void)hipFree(x.part);
        x.list = nullptr;
        x.part = nullptr;
        x.cap = 0;
        x.spp = 0;
        if ((e = hipMalloc((void**)&x.list, (size_t)need * sizeof(unsigned))) != hipSuccess) return hip_fail(e, "hipMalloc (work list)");
        x.cap = need;
    }
    if (o->spp > 1 && x.spp < o->spp) {
        (void)hipFree(x.part);
        x.part = nullptr;
        x.spp = 0;
        if ((e = hipMalloc((void**)&x.part, (size_t)o->spp * (size_t)x.cap * 3 * sizeof(double))) != hipSuccess)
            return hip_fail(e, "hipMalloc (per-sample radiance)");
        x.spp = o->spp;
    }
    const XForm form = x_form_choice(s->dev, s->xcfg, *o);
    if (form != XFORM_MEGA) {   // gi_wf.hip's forms: counters; the wavefront form also path queues sized to a chunk of units
        const long long want = std::max(64ll, std::min(kXWfChunk, need * (long long)o->spp));
        if (!x.wcnt) {
            if ((e = hipMalloc((void**)&x.wcnt, 2 * 64 * sizeof(unsigned))) != hipSuccess) return hip_fail(e, "hipMalloc (wavefront counters)");
        }
        if (form == XFORM_WF && x.wcap < want) {
            for (int q = 0; q < 2; ++q) {
                (void)hipFree(x.wq[q]);
                (void)hipFree(x.wid[q]);
                x.wq[q] = nullptr;
                x.wid[q] = nullptr;
            }
            x.wcap = 0;
            for (int q = 0; q < 2; ++q) {
                if ((e = hipMalloc((void**)&x.wq[q], (size_t)want * 12 * sizeof(double))) != hipSuccess ||
                    (e = hipMalloc((void**)&x.wid[q], (size_t)want * 2 * sizeof(unsigned))) != hipSuccess)
                    return hip_fail(e, "hipMalloc (wavefront path queues)");
            }
            x.wcap = want;
        }
    }
    return GI_OK;
}

// folds ring slot i (its end event has been recorded) into the running sum
hipError_t fold_timer(KTimer& kt, int i) {
    hipError_t e = hipEventSynchronize(static_cast<hipEvent_t>(kt.ev1[i]));
    float ms = 0.f;
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, static_cast<hipEvent_t>(kt.ev0[i]), static_cast<hipEvent_t>(kt.ev1[i]));
    if (e == hipSuccess) { kt.sum_ms += ms; kt.folded++; }
    return e;
}

// GI_FLAG_TIME: create the event ring on first use; fold the pair the next launch will reuse
int ensure_timer(gi_scene* s, const gi_opts* o) {
    if (!(o->flags & GI_FLAG_TIME)) return GI_OK;
    KTimer& kt = s->kt;
    if (!kt.ev0[0]) {
        for (int i = 0; i < KTimer::kRing; i++) {
            hipEvent_t a = nullptr, b = nullptr;
            hipError_t e = hipEventCreate(&a);
            if (e == hipSuccess) e = hipEventCreate(&b);
            if (e != hipSuccess) {
                if (a) (void)hipEventDestroy(a);
                return hip_fail(e, "hipEventCreate");
            }
            kt.ev0[i] = a;
            kt.ev1[i] = b;
        }
    }
    if (kt.recorded >= KTimer::kRing) {
        const hipError_t e = fold_timer(kt, (int)(kt.recorded % KTimer::kRing));
        if (e != hipSuccess) return hip_fail(e, "timer event");
    }
    return GI_OK;
}

// One render launch of scene s on `stream`, ordered behind the scene's previous launch.
int issue_render(gi_scene* s, const CamDev& cd, V3 light, int w, int h, int y0, const gi_opts& o, double* d_rgb,
                 uint8_t* d_rgb8, hipStream_t stream, bool timer) {
    hipError_t e = hipSuccess;
    if (!s->last && (e = hipEventCreateWithFlags(&s->last, hipEventDisableTiming)) != hipSuccess)
        return hip_fail(e, "hipEventCreate");
    if (s->launched && (e = hipStreamWaitEvent(stream, s->last, 0)) != hipSuccess) return hip_fail(e, "hipStreamWaitEvent");
    e = launch_render(s->dev, s->xcfg, cd, light, w, h, y0, o, d_rgb, d_rgb8, s->xs, timer ? &s->kt : nullptr, stream);
    if (e != hipSuccess) return hip_fail(e, "render launch");
    if ((e = hipEventRecord(s->last, stream)) != hipSuccess) return hip_fail(e, "hipEventRecord");
    s->launched = true;
    return GI_OK;
}

void free_hostpath_buffers(HostPath& hp) {
    for (int i = 0; i < HostPath::kSlots; i++) {
        (void)hipFree(hp.d_rgb[i]);
        (void)hipFree(hp.d_rgb8[i]);
        (void)hipHostFree(hp.h_rgb[i]);
        (void)hipHostFree(hp.h_rgb8[i]);
        hp.d_rgb[i] = nullptr;
        hp.d_rgb8[i] = nullptr;
        hp.h_rgb[i] = nullptr;
        hp.h_rgb8[i] = nullptr;
    }
    hp.cap_px = 0;
    hp.n_alloc = 0;
}

// streams and events on first use; `slots` band slots of `px` pixels (grown, never shrunk)
int ensure_hostpath(gi_scene* s, size_t px, int slots) {
    HostPath& hp = s->hp;
    hipError_t e = hipSuccess;
    if (!hp.render) {
        if ((e = hipStreamCreateWithFlags(&hp.render, hipStreamNonBlocking)) != hipSuccess) return hip_fail(e, "hipStreamCreate");
        if ((e = hipStreamCreateWithFlags(&hp.copy, hipStreamNonBlocking)) != hipSuccess) return hip_fail(e, "hipStreamCreate");
        for (int i = 0; i < HostPath::kSlots; i++) {
            if ((e = hipEventCreateWithFlags(&hp.rendered[i], hipEventDisableTiming)) != hipSuccess ||
                (e = hipEventCreateWithFlags(&hp.copied[i], hipEventDisableTiming)) != hipSuccess)
                return hip_fail(e, "hipEventCreate");
        }
    }
    if (hp.cap_px < px || hp.n_alloc < slots) {
        px = std::max(px, hp.cap_px);
        slots = std::max(slots, hp.n_alloc);
        free_hostpath_buffers(hp);
        for (int i = 0; i < slots; i++) {
            if ((e = hipMalloc((void**)&hp.d_rgb[i], px * 3 * sizeof(double))) != hipSuccess ||
                (e = hipMalloc((void**)&hp.d_rgb8[i], px * 3)) != hipSuccess ||
                (e = hipHostMalloc((void**)&hp.h_rgb[i], px * 3 * sizeof(double), hipHostMallocDefault)) != hipSuccess ||
                (e = hipHostMalloc((void**)&hp.h_rgb8[i], px * 3, hipHostMallocDefault)) != hipSuccess) {
                free_hostpath_buffers(hp);
                return hip_fail(e, "band buffers");
            }
        }
        hp.cap_px = px;
        hp.n_alloc = slots;
    }
    return GI_OK;
}

void destroy_scene(gi_scene* s) noexcept {
    if (!s) return;
    if (s->device >= 0) (void)hipSetDevice(s->device);
    HostPath& hp = s->hp;
    if (hp.render) (void)hipStreamSynchronize(hp.render);
    if (hp.copy) (void)hipStreamSynchronize(hp.copy);
    if (s->last) (void)hipEventSynchronize(s->last);
    for (void* p : s->allocs) (void)hipFree(p);
    (void)hipFree(s->xs.list);
    (void)hipFree(s->xs.part);
    for (int q = 0; q < 2; ++q) {
        (void)hipFree(s->xs.wq[q]);
        (void)hipFree(s->xs.wid[q]);
    }
    (void)hipFree(s->xs.wcnt);
    (void)hipFree(s->xs.ad_list);
    (void)hipFree(s->xs.ad_cnt);
    (void)hipFree(s->xs.ad_sum);
    (void)hipFree(s->xs.ad_n);
    free_rflat(s->xs);
    for (int i = 0; i < KTimer::kRing; i++) {
        if (s->kt.ev0[i]) (void)hipEventDestroy(static_cast<hipEvent_t>(s->kt.ev0[i]));
        if (s->kt.ev1[i]) (void)hipEventDestroy(static_cast<hipEvent_t>(s->kt.ev1[i]));
    }
    free_hostpath_buffers(hp);
    for (int i = 0; i < HostPath::kSlots; i++) {
        if (hp.rendered[i]) (void)hipEventDestroy(hp.rendered[i]);
        if (hp.copied[i]) (void)hipEventDestroy(hp.copied[i]);
    }
    if (hp.render) (void)hipStreamDestroy(hp.render);
    if (hp.copy) (void)hipStreamDestroy(hp.copy);
    if (s->last) (void)hipEventDestroy(s->last);
    delete s;
}

// host-side reference octree query: Octree::intersect -> Node::intersect (octree.h:46-68, 132-155)
void octree_query(const HostScene& h, int ni, V3 o, V3 d, std::vector<int32_t>& out) {
    const RNode& nd = h.rnodes[(size_t)ni];
    if (nd.child0 < 0) {   // leaf: a copy of its list (octree.h:133-135)
        out.insert(out.end(), h.leaf_ents.begin() + nd.ent_off, h.leaf_ents.begin() + nd.ent_off + nd.ent_cnt);
        return;
    }
    for (int c = 0; c < 8; ++c) {   // children 0..7 (octree.h:139-152)
        const RNode& ch = h.rnodes[(size_t)nd.child0 + c];
        if (ch.ent_cnt == 0) continue;   // octree.h:140
        if (box_hit(ld3(ch.mn), ld3(ch.mx), o, d)) octree_query(h, nd.child0 + c, o, d, out);
    }
}

}  // namespace

// ---- internal entry points shared with gi_multi.cpp (gi_internal.h) -------------------------
namespace gi {

int error(int code, const std::string& msg) noexcept { return fail(code, msg); }
int hip_error(hipError_t e, const char* what) noexcept { return hip_fail(e, what); }

int bind_device(int device) {
    int cur = -1;
    hipError_t e = hipGetDevice(&cur);
    if (e != hipSuccess) return hip_fail(e, "hipGetDevice");
    if (cur != device) {
        e = hipSetDevice(device);
        if (e != hipSuccess) return hip_fail(e, "hipSetDevice");
    }
    return GI_OK;
}

int check_device(int dev) {
    hipDeviceProp_t prop;
    const hipError_t e = hipGetDeviceProperties(&prop, dev);
    if (e != hipSuccess) return hip_fail(e, "hipGetDeviceProperties");
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(GI_ERR_DEVICE, std::string("device ") + std::to_string(dev) + " is " + prop.gcnArchName +
                                       ", libgi is built for gfx950 only");
    return GI_OK;
}

// raytracer.h:26-30: camera basis and the frame's top-left (vertical offset uses w)
CamDev make_cam(const gi_camera& c, int w) {
    CamDev d;
    d.pos = v3(c.pos[0], c.pos[1], c.pos[2]);
    d.up = v3(c.up[0], c.up[1], c.up[2]);
    const V3 fwd = v3(c.forward[0], c.forward[1], c.forward[2]);
    d.rx = 0.0002;
    d.ry = 0.0002;
    d.left = normalize(cross(d.up, fwd));
    d.top_left = (((d.pos + c.focal * fwd) + ((d.left * (double)w) * 0.5) * d.rx) + ((d.up * (double)w) * 0.5) * d.ry) - d.pos;
    return d;
}

int check_opts(int w, int h, const gi_opts* o) {
    if (!o) return fail(GI_ERR_ARG, "null opts");
    if (w <= 0 || h <= 0 || (int64_t)w * h > (int64_t)1 << 34) return fail(GI_ERR_ARG, "bad frame size");
    if (o->mode != GI_MODE_R && o->mode != GI_MODE_X) return fail(GI_ERR_ARG, "bad mode");
    if (o->shard_count < 1 || o->shard_index < 0 || o->shard_index >= o->shard_count) return fail(GI_ERR_ARG, "bad shard");
    if (o->mode == GI_MODE_X && (o->spp < 1 || o->depth < 1 || o->depth > 0xFFFF))
        return fail(GI_ERR_ARG, "mode X needs spp >= 1, 1 <= depth <= 65535");
    if ((o->flags & GI_FLAG_STATS) && !o->stats) return fail(GI_ERR_ARG, "GI_FLAG_STATS without stats buffer");
    if ((o->sample_begin != 0 || o->sample_end != 0) &&
        (o->mode != GI_MODE_X || o->spp < 2 || o->sample_begin < 0 || o->sample_begin >= o->sample_end || o->sample_end > o->spp))
        return fail(GI_ERR_ARG, "progressive pass: mode X, spp > 1, 0 <= sample_begin < sample_end <= spp");
    return GI_OK;
}

// Progressive passes (gi_opts sample_begin / sample_end) continue one frame on one scene: the first
// pass (sample_begin 0) records the frame's key, a later one must match it and start where the
// previous pass ended.  Any other render of the scene ends the frame.
namespace {
uint64_t prog_key(const gi_camera& c, const double light[3], int w, int h, const gi_opts& o) {
    uint64_t k = 1469598103934665603ull;
    auto mix = [&](const void* p, size_t n) {
        for (size_t i = 0; i < n; ++i) k = (k ^ static_cast<const unsigned char*>(p)[i]) * 1099511628211ull;
    };
    mix(&c, sizeof c);
    mix(light, 3 * sizeof(double));
    const int64_t v[8] = {w, h, o.spp, o.depth, (int64_t)o.seed, o.shard_count, o.shard_index,
                          (int64_t)(o.flags & ~(GI_FLAG_STATS | GI_FLAG_TIME))};
    mix(v, sizeof v);
    return k;
}
int prog_check(gi_scene* s, const gi_camera& c, const double light[3], int w, int h, const gi_opts& o) {
    if (o.sample_end == 0) {
        s->prog_next = -1;
        return GI_OK;
    }
    const uint64_t key = prog_key(c, light, w, h, o);
    if (o.sample_begin > 0 && s->prog_next == o.sample_begin && s->launched) {
        // the previous pass was accepted when issued: a device error since ends the frame
        const hipError_t e = hipEventQuery(s->last);
        if (e != hipSuccess && e != hipErrorNotReady) {
            s->prog_next = -1;
            return hip_fail(e, "progressive pass: the previous pass failed on the device; restart the frame at sample 0");
        }
    }
    if (o.sample_begin > 0 && (s->prog_next != o.sample_begin || s->prog_key != key)) {
        s->prog_next = -1;
        return fail(GI_ERR_ARG, "progressive pass out of order: a pass continues the previous pass's frame "
                                "(same camera, light, size, spp, depth, seed, shard) from its sample_end");
    }
    s->prog_key = key;
    s->prog_next = -1;   // set once this pass has been issued
    return GI_OK;
}
void prog_done(gi_scene* s, const gi_opts& o) {
    s->prog_next = (o.sample_end > 0 && o.sample_end < o.spp) ? o.sample_end : -1;
}
// a whole frame has been issued: it is the retained frame if it left per-sample rows of one shard
void keep_frame(gi_scene* s, const CamDev& cd, int w, int h, const gi_opts& o) {
    if (o.mode != GI_MODE_X || o.spp < 2 || o.shard_count != 1) return;
    s->keep_w = w;
    s->keep_h = h;
    s->keep_n = o.sample_end > 0 ? o.sample_end : o.spp;
    s->keep_spp = o.spp;
    s->keep_cam = cd;
}
}  // namespace

int band_rows_of(const gi_opts* o, int h) {
    int band = o->band_rows > 0 ? o->band_rows : h;
    band = ((band + GI_TILE - 1) / GI_TILE) * GI_TILE;
    return std::min(band, ((h + GI_TILE - 1) / GI_TILE) * GI_TILE);
}

// Builds the scene on the host and uploads it to `device` (made current).
int scene_create_on(const gi_scene_desc* desc, int device, gi_scene** out) {
    *out = nullptr;
    int rc = bind_device(device);
    if (rc || (rc = check_device(device))) return rc;
    std::unique_ptr<gi_scene, void (*)(gi_scene*)> s(new gi_scene(), [](gi_scene* p) { destroy_scene(p); });
    s->device = device;
    std::string err;
    // Beyond GI_X_COORD_MAX the fp32 box tests cull boxes a ray is inside of (gi_dev.h inv_dir): no scene is
    // made, so no render, ray query, feature buffer, adaptive pass or test hook can be asked of one.  Mode R
    // of such a scene goes with it: its box tests clamp the reciprocal the same way.
    auto beyond = [](double reach) {
        char msg[200];
        snprintf(msg, sizeof msg, "scene coordinates reach %.9g: beyond the supported range, |coordinate| <= %.9g "
                 "(the fp32 box tests of axis-parallel rays overflow)", reach, GI_X_COORD_MAX);
        return fail(GI_ERR_SCENE, msg);
    };
    // (a triangle's vertices and a sphere's extent lie inside the structure's boxes: a scene they alone put
    // beyond the limit is refused before anything is built; the structure's own reach decides the rest)
    if (const double reach = x_desc_reach(*desc); !(reach <= GI_X_COORD_MAX)) return beyond(reach);
    if (!build_host_scene(*desc, s->host, err)) return fail(GI_ERR_SCENE, err);
    if (const double reach = x_coord_reach(s->host); !(reach <= GI_X_COORD_MAX)) return beyond(reach);
    DevScene& d = s->dev;
    memset(&d, 0, sizeof d);
    const HostScene& h = s->host;
    hipError_t e;
    gi_scene* sp = s.get();
    if ((e = upload(sp, h.rnodes, &d.rnodes)) != hipSuccess || (e = upload(sp, h.leaf_ents, &d.leaf_ents)) != hipSuccess ||
        (e = upload(sp, h.ents, &d.ents)) != hipSuccess || (e = upload(sp, h.tris, &d.tris)) != hipSuccess ||
        (e = upload(sp, h.xwnodes, &d.xwnodes)) != hipSuccess || (e = upload(sp, h.xhot, &d.xhot)) != hipSuccess ||
        (e = upload(sp, h.xbox, &d.xbox)) != hipSuccess ||
        (e = upload(sp, h.xprims, &d.xprims)) != hipSuccess || (e = upload(sp, xflat_device_table(h), &d.xflat)) != hipSuccess ||
        (e = upload(sp, std::vector<unsigned>(16, 0u), const_cast<const unsigned**>(&d.work))) != hipSuccess ||
        (e = upload(sp, h.app_off, &d.app_off)) != hipSuccess || (e = upload(sp, h.app_rec, &d.app_rec)) != hipSuccess ||
        (e = upload(sp, h.rpath_rec, &d.rpath_rec)) != hipSuccess || (e = upload(sp, h.rc_nodes, &d.rc_nodes)) != hipSuccess ||
        (e = upload(sp, h.rc_ent, &d.rc_ent)) != hipSuccess || (e = upload(sp, h.rc_maxkey, &d.rc_maxkey)) != hipSuccess ||
        (e = upload(sp, h.r_always, &d.r_always)) != hipSuccess ||
        (e = upload(sp, h.r_leaf_of_rank, &d.r_leaf_of_rank)) != hipSuccess)
        return hip_fail(e, "scene upload");
    d.n_rnodes = (int32_t)h.rnodes.size();
    d.n_ents = (int32_t)h.ents.size();
    d.n_xwnodes = (int32_t)h.xwnodes.size();
    d.n_xprims = (int32_t)h.xprims.size();
    d.x_max_depth = h.x_max_depth;
    d.x_handle8 = h.x_handle8;
    d.x_flags = h.x_flags;
    d.x_skip_a = h.x_skip_a;
    d.x_skip_b = h.x_skip_b;
    d.n_xhot = (int32_t)h.xhot.size();
    d.n_r_always = (int32_t)h.r_always.size();
    d.rc_ext = (float)h.rc_ext;
    {   // LDS-resident traversal + shading records for small scenes (<= 40 KB per workgroup: three
        // 256-thread workgroups per CU stay resident within the CU's 160 KB of LDS)
        const size_t bytes = h.xwnodes.size() * sizeof(XWNode) + h.xhot.size() * sizeof(XHot) +
                             h.xprims.size() * sizeof(XPrim) + h.ents.size() * sizeof(REnt);
        d.x_lds_bytes = bytes <= 40 * 1024 ? (int32_t)bytes : 0;
        // the flat leaf query (gi_wf.hip wf_flat): scenes staged in LDS whose leaf table fits
        d.n_xflat = (int32_t)h.xflat.size();
        d.x_flat = (d.x_lds_bytes > 0 && h.x_flat_ok) ? 1 : 0;
        // ... and one exact test per fan-pair leaf where its first step decides (gi_fan_pair.h; GI_X_FAN=0: both)
        d.x_fan = (d.x_flat && h.x_fan_all && x_env().fan) ? 1 : 0;
        // light shading (no acos texture mapping, no sphere primitives): gi_wf.hip's kernels (k_seg, k_cast)
        // run 4 waves per SIMD, provided four workgroups fit a CU's 160 KB.  The bound allows each, beside
        // the scene, 256 lanes x 80 B and 4 x 68 x 4 B -- more than their path slots (256 x 64 B) need: it
        // is the footprint of the LDS build k_mode_x once had, kept so that no scene changes its variant.
        // (k_seg's ring of prepared primary rays, 10 KB more, is decided by the occupancy query of
        // x_launch_config and changes no variant)
        const size_t per_wg = bytes + 256 * 10 * sizeof(double) + 4 * 68 * sizeof(unsigned);
        d.x_waves4 = (d.x_lds_bytes > 0 && 4 * per_wg <= 160 * 1024) ? 1 : 0;
        d.x_tri_only = 1;
        for (const REnt& r : h.ents)
            if (r.kind == K_IMP_SPHERE || r.kind == K_EXP_SPHERE || r.kind == K_EXP_CONE || r.kind == K_EXP_RECTANGLE) {
                d.x_waves4 = 0;
                d.x_tri_only = 0;
            }
        for (const XPrim& xp : h.xprims)
            if (xp.kind != 0) d.x_tri_only = 0;
        d.r_tri_only = 1;
        for (const REnt& r : h.ents)
            if (r.kind != K_IMP_TRIANGLE) d.r_tri_only = 0;
    }
    // HBM-resident scenes whose XWNode tree outgrows an XCD's L2 share (> 2 MB) traverse quantised
    // nodes (XCNode: one 128-byte line per node instead of two): C5 287 -> 270 ms; the 1k soup, whose
    // 84 KB tree stays in L2 anyway, pays the decoding (+6%) and keeps XWNode.
    const bool want_cn = h.xwnodes.size() * sizeof(XWNode) > (size_t)2 << 20;
    if (d.x_lds_bytes == 0 && want_cn && encode_xcnodes(h.xwnodes, s->host.xcnodes) &&
        (e = upload(sp, h.xcnodes, &d.xcnodes)) != hipSuccess)
        return hip_fail(e, "scene upload (quantised nodes)");
    for (int k = 0; k < 3; ++k) { d.root_lo[k] = INFINITY; d.root_hi[k] = -INFINITY; }
    if (!h.xwnodes.empty())
        for (int c = 0; c < 8; ++c)
            if (h.xwnodes[0].child[c] != XEMPTY)
                for (int k = 0; k < 3; ++k) {
                    d.root_lo[k] = std::min(d.root_lo[k], h.xwnodes[0].lo[k][c]);
                    d.root_hi[k] = std::max(d.root_hi[k], h.xwnodes[0].hi[k][c]);
                }
    d.x_far_r = INFINITY;
    for (int k = 0; k < 3; ++k)
        if (d.root_lo[k] <= d.root_hi[k]) {
            const float m = 16.0f * std::max(std::fabs(d.root_lo[k]), std::fabs(d.root_hi[k]));
            d.x_far_r = std::isinf(d.x_far_r) ? m : std::max(d.x_far_r, m);
        }
    if ((e = x_launch_config(d, device, s->xcfg)) != hipSuccess) return hip_fail(e, "occupancy query");
    s->xcfg.shadow = shadow_leaves_of(s->host);   // the boundary leaves a launch's light is tested against
    *out = s.release();
    return GI_OK;
}

void scene_destroy(gi_scene* s) noexcept { destroy_scene(s); }
int scene_device(const gi_scene* s) { return s->device; }
std::mutex& scene_mutex(gi_scene* s) { return s->mu; }

// Asynchronous render of a band (rows [y0, y0 + h) of a frame w pixels wide; the whole frame for
// y0 = 0, h = its height) or of one shard of it, into device buffers on `stream`.
int scene_render_band(gi_scene* s, const CamDev& cd, const double light[3], int w, int h, int y0, const gi_opts& o,
                      double* d_rgb, uint8_t* d_rgb8, hipStream_t stream, bool timer) {
    s->keep_n = 0;   // (every render ends the retained frame; a whole frame that succeeds becomes the next one)
    s->ad_next = -1;   // (and the adaptive frame)
    s->ad_done = 0;
    int rc = bind_device(s->device);
    if (rc || (rc = ensure_xscratch(s, w, h, &o)) || (timer && (rc = ensure_timer(s, &o)))) return rc;
    return issue_render(s, cd, v3(light[0], light[1], light[2]), w, h, y0, o, d_rgb, d_rgb8, stream, timer);
}

int unshard(int w, int h, int n, const double* packed, const uint8_t* packed8, double* rgb, uint8_t* rgb8,
            hipStream_t stream) {
    const hipError_t e = launch_unshard(w, h, n, packed, packed8, rgb, rgb8, stream);
    return e == hipSuccess ? GI_OK : hip_fail(e, "unshard launch");
}

}  // namespace gi

extern "C" {

int gi_abi_version(void) { return GI_ABI_VERSION; }
const char* gi_last_error(void) { return g_err.c_str(); }

int gi_device_list(int32_t* out, int cap) {
    int ndev = 0, n = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) return 0;
    for (int d = 0; d < ndev; ++d) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, d) == hipSuccess && std::strncmp(prop.gcnArchName, "gfx950", 6) == 0) {
            if (out && n < cap) out[n] = d;
            ++n;
        }
    }
    return n;
}

int gi_device_count(void) { return gi_device_list(nullptr, 0); }

#ifndef GI_BUILD_ID
#define GI_BUILD_ID "unknown"
#endif
const char* gi_build_id(void) { return GI_BUILD_ID; }

int gi_camera_init(const double pos[3], const double look_at[3], double focal, gi_camera* out) {
    if (!pos || !look_at || !out) return fail(GI_ERR_ARG, "null argument");
    // Camera(pos, lookAt, focal) (camera.h:8-10): up = (0,0,1); forward = normalize(lookAt - pos)
    const V3 p = v3(pos[0], pos[1], pos[2]);
    const V3 f = normalize(v3(look_at[0], look_at[1], look_at[2]) - p);
    st3(out->pos, p);
    out->up[0] = 0; out->up[1] = 0; out->up[2] = 1.0;
    st3(out->forward, f);
    out->focal = focal;
    return GI_OK;
}

int gi_scene_create(const gi_scene_desc* desc, gi_scene** out) {
    return guard([&]() -> int {
        if (!desc || !out || desc->n_entities < 0 || (desc->n_entities > 0 && !desc->entities))
            return fail(GI_ERR_ARG, "bad scene descriptor");
        *out = nullptr;
        int ndev = 0;
        hipError_t e = hipGetDeviceCount(&ndev);
        if (e != hipSuccess || ndev <= 0) return fail(GI_ERR_DEVICE, "no HIP device (libgi renders only on gfx950)");
        int dev = 0;
        if ((e = hipGetDevice(&dev)) != hipSuccess) return hip_fail(e, "hipGetDevice");
        return scene_create_on(desc, dev, out);
    });
}

void gi_scene_destroy(gi_scene* s) { destroy_scene(s); }

int gi_scene_get_info(const gi_scene* s, gi_scene_info* info) {
    if (!s || !info) return fail(GI_ERR_ARG, "null argument");
    info->n_entities = (int32_t)s->host.ents.size();
    info->n_nodes = (int32_t)s->host.rnodes.size();
    info->n_leaves = s->host.n_leaves;
    info->max_depth = s->host.max_depth;
    info->n_reachable = s->host.n_reachable;
    info->n_dropped = s->host.n_dropped;
    info->x_nodes = (int32_t)(s->host.xnodes.empty() ? s->host.xwnodes.size() : s->host.xnodes.size());
    info->x_prims = (int32_t)s->host.xprims.size();
    info->device_bytes = s->bytes;
    info->x_node_bytes = s->dev.xcnodes ? (int32_t)sizeof(XCNode) : (int32_t)sizeof(XWNode);
    info->x_lds_resident = s->dev.x_lds_bytes > 0 ? 1 : 0;
    info->x_flat_leaves = (int32_t)s->host.xflat.size();
    info->x_fan_leaves = s->host.n_fan_leaves;
    return GI_OK;
}

int64_t gi_shard_tiles(int w, int h, int shard_count) {
    if (w <= 0 || h <= 0 || shard_count < 1) return -1;
    return shard_tiles(w, h, shard_count);
}

int gi_render_device(gi_scene* s, const gi_camera* cam, const double light[3], int w, int h, const gi_opts* o,
                     double* d_rgb, uint8_t* d_rgb8, void* stream) {
    return guard([&]() -> int {
        DeviceRestore keep;   // the caller's current device, restored on return
        if (!s) return fail(GI_ERR_ARG, "null scene");
        std::lock_guard<std::mutex> lk(s->mu);
        s->keep_n = 0;   // (a refused render too ends the retained frame)
        s->ad_next = -1;   // (and the adaptive frame)
        s->ad_done = 0;
        int rc = check_opts(w, h, o);
        if (rc) return rc;
        if (!cam || !light) return fail(GI_ERR_ARG, "null camera or light");
        if ((rc = prog_check(s, *cam, light, w, h, *o))) return rc;
        const CamDev cd = make_cam(*cam, w);
        rc = scene_render_band(s, cd, light, w, h, 0, *o, d_rgb, d_rgb8, static_cast<hipStream_t>(stream), true);
        if (rc == GI_OK) {
            prog_done(s, *o);
            keep_frame(s, cd, w, h, *o);
        }
        return rc;
    });
}

int gi_render(gi_scene* s, const gi_camera* cam, const double light[3], int w, int h, const gi_opts* o, double* rgb,
              uint8_t* rgb8, const volatile int* cancel, gi_tile_cb cb, void* user) {
    return guard([&]() -> int {
        DeviceRestore keep;   // the caller's current device, restored on return
        if (!s) return fail(GI_ERR_ARG, "null scene");
        std::lock_guard<std::mutex> lk(s->mu);
        s->keep_n = 0;   // (a refused render too ends the retained frame)
        s->ad_next = -1;   // (and the adaptive frame)
        s->ad_done = 0;
        int rc = check_opts(w, h, o);
        if (rc) return rc;
        if (!cam || !light) return fail(GI_ERR_ARG, "null camera or light");
        if (o->shard_count != 1) return fail(GI_ERR_ARG, "gi_render renders whole frames; use gi_render_device or gi_multi to shard");
        if ((rc = bind_device(s->device))) return rc;
        // progressive bands of whole tile rows (the reference fills rows in order, raytracer.h:32-33,
        // and the Viewer repaints what is done, viewer.h:18-21); cancel is polled between bands.
        const int band = band_rows_of(o, h);
        const size_t band_px = (size_t)w * (size_t)band;
        const int n_bands = (h + band - 1) / band;
        if (o->sample_end > 0 && n_bands > 1)   // (a pass's rows are the whole frame's work list)
            return fail(GI_ERR_ARG, "progressive passes render whole frames: band_rows 0 or >= h");
        if ((rc = prog_check(s, *cam, light, w, h, *o))) return rc;
        if ((rc = ensure_hostpath(s, band_px, std::min(n_bands, HostPath::kSlots)))) return rc;
        HostPath& hp = s->hp;
        const CamDev cd = make_cam(*cam, w);
        const bool want_rgb = rgb || cb, want_rgb8 = rgb8 || cb;
        // a whole-frame call copies straight into the caller's buffers (no staging, nothing to overlap)
        const bool direct = n_bands == 1;
        double* const dst_rgb = direct && rgb ? rgb : hp.h_rgb[0];
        uint8_t* const dst_rgb8 = direct && rgb8 ? rgb8 : hp.h_rgb8[0];
        // band i: render into slot i % 2 (after that slot's previous copy), then copy to its staging
        auto issue = [&](int i) -> int {
            const int k = i % HostPath::kSlots, y0 = i * band, rows = std::min(band, h - y0);
            const size_t n = (size_t)w * rows * 3;
            hipError_t e = hipSuccess;
            if (i >= HostPath::kSlots && (e = hipStreamWaitEvent(hp.render, hp.copied[k], 0)) != hipSuccess)
                return hip_fail(e, "render");
            const int r = scene_render_band(s, cd, light, w, rows, y0, *o, hp.d_rgb[k], hp.d_rgb8[k], hp.render, false);
            if (r) return r;
            e = hipEventRecord(hp.rendered[k], hp.render);
            if (e == hipSuccess) e = hipStreamWaitEvent(hp.copy, hp.rendered[k], 0);
            double* const to = i == 0 ? dst_rgb : hp.h_rgb[k];
            uint8_t* const to8 = i == 0 ? dst_rgb8 : hp.h_rgb8[k];
            if (e == hipSuccess && want_rgb) e = hipMemcpyAsync(to, hp.d_rgb[k], n * sizeof(double), hipMemcpyDeviceToHost, hp.copy);
            if (e == hipSuccess && want_rgb8) e = hipMemcpyAsync(to8, hp.d_rgb8[k], n, hipMemcpyDeviceToHost, hp.copy);
            if (e == hipSuccess) e = hipEventRecord(hp.copied[k], hp.copy);
            return e == hipSuccess ? GI_OK : hip_fail(e, "render");
        };
        hipError_t e = hipSuccess;
        if (cancel && *cancel) rc = fail(GI_ERR_CANCELLED, "cancelled");
        else rc = issue(0);
        for (int i = 0; rc == GI_OK && i < n_bands; i++) {
            // the next band goes to the GPU before this one is delivered; cancel is polled between bands
            if (i + 1 < n_bands) {
                if (cancel && *cancel) { rc = fail(GI_ERR_CANCELLED, "cancelled"); break; }
                if ((rc = issue(i + 1)) != GI_OK) break;
            }
            const int k = i % HostPath::kSlots, y0 = i * band, rows = std::min(band, h - y0);
            const size_t n = (size_t)w * rows * 3;
            if ((e = hipEventSynchronize(hp.copied[k])) != hipSuccess) { rc = hip_fail(e, "render"); break; }
            const double* hr = i == 0 ? dst_rgb : hp.h_rgb[k];
            const uint8_t* hr8 = i == 0 ? dst_rgb8 : hp.h_rgb8[k];
            if (rgb && hr != rgb) { std::memcpy(rgb + (size_t)y0 * w * 3, hr, n * sizeof(double)); hr = rgb + (size_t)y0 * w * 3; }
            if (rgb8 && hr8 != rgb8) { std::memcpy(rgb8 + (size_t)y0 * w * 3, hr8, n); hr8 = rgb8 + (size_t)y0 * w * 3; }
            if (cb) cb(user, y0, rows, hr8, hr);
        }
        // nothing of this call stays in flight (a cancelled or failed call drains its bands)
        const hipError_t e1 = hipStreamSynchronize(hp.render), e2 = hipStreamSynchronize(hp.copy);
        if (rc == GI_OK && (e1 != hipSuccess || e2 != hipSuccess)) rc = hip_fail(e1 != hipSuccess ? e1 : e2, "render");
        if (rc == GI_OK) prog_done(s, *o);
        if (rc == GI_OK && n_bands == 1) keep_frame(s, cd, w, h, *o);
        else s->keep_n = 0;
        return rc;
    });
}

int gi_scene_kernel_ms(gi_scene* s, float* avg_ms, int64_t* n) {
    return guard([&]() -> int {
        DeviceRestore keep;   // the caller's current device, restored on return
        if (!s || !avg_ms) return fail(GI_ERR_ARG, "null argument");
        std::lock_guard<std::mutex> lk(s->mu);
        KTimer& kt = s->kt;
        if (kt.recorded == 0) return fail(GI_ERR_ARG, "no render issued with GI_FLAG_TIME since the last read");
        int rc = bind_device(s->device);
        if (rc) return rc;
        // the unfolded pairs are the last min(recorded, kRing) slots
        const long long first = kt.recorded > KTimer::kRing ? kt.recorded - KTimer::kRing : 0;
        for (long long r = std::max(first, kt.folded); r < kt.recorded; r++) {
            const hipError_t e = fold_timer(kt, (int)(r % KTimer::kRing));
            if (e != hipSuccess) return hip_fail(e, "gi_scene_kernel_ms");
        }
        *avg_ms = (float)(kt.sum_ms / (double)kt.folded);
        if (n) *n = kt.folded;
        kt.recorded = 0;
        kt.folded = 0;
        kt.sum_ms = 0.0;
        return GI_OK;
    });
}

int gi_scene_x_form(gi_scene* s, const gi_opts* o, int32_t* form) {
    return guard([&]() -> int {
        if (!s || !o || !form) return fail(GI_ERR_ARG, "null argument");
        std::lock_guard<std::mutex> lk(s->mu);
        *form = x_form_choice(s->dev, s->xcfg, *o);
        return GI_OK;
    });
}

int gi_scene_shadow_leaves(gi_scene* s, const double* light, const double* cam_pos, uint32_t* boundary_mask, uint32_t* live_mask) {
    return guard([&]() -> int {
        if (!s || !light || !cam_pos || !boundary_mask || !live_mask) return fail(GI_ERR_ARG, "null argument");
        std::lock_guard<std::mutex> lk(s->mu);
        const XShadowLeaves& sl = s->xcfg.shadow;
        const bool on = s->dev.x_flat != 0 && sl.n > 0;
        *boundary_mask = on ? sl.boundary_mask() : 0u;
        *live_mask = on ? (x_launch_live(s->dev, s->xcfg, v3(cam_pos[0], cam_pos[1], cam_pos[2]), v3(light[0], light[1], light[2]), 0u) & sl.table_mask())
                        : 0u;
        return GI_OK;
    });
}

int gi_scene_seg_ring(gi_scene* s, const gi_opts* o, int32_t* on) {
    return guard([&]() -> int {
        if (!s || !o || !on) return fail(GI_ERR_ARG, "null argument");
        std::lock_guard<std::mutex> lk(s->mu);
        *on = (x_form_choice(s->dev, s->xcfg, *o) == XFORM_SEG && s->xcfg.seg_ring) ? 1 : 0;
        return GI_OK;
    });
}

int gi_scene_r_kernel(gi_scene* s, const gi_opts* o, int32_t* kernel) {
    return guard([&]() -> int {
        if (!s || !o || !kernel) return fail(GI_ERR_ARG, "null argument");
        std::lock_guard<std::mutex> lk(s->mu);
        *kernel = r_kernel_choice(s->dev, *o);
        if (*kernel == RK_FLAT && s->xs.rf_failed > 0 && s->xs.rf_slots == 0) *kernel = RK_BATCH;   // (its buffers failed)
        return GI_OK;
    });
}

int gi_unshard_device(int w, int h, int shard_count, const double* d_packed, const uint8_t* d_packed8, double* d_rgb,
                      uint8_t* d_rgb8, void* stream) {
    return guard([&]() -> int {
        if (w <= 0 || h <= 0 || shard_count < 1) return fail(GI_ERR_ARG, "bad unshard arguments");
        if ((d_rgb && !d_packed) || (d_rgb8 && !d_packed8)) return fail(GI_ERR_ARG, "missing packed input");
        return unshard(w, h, shard_count, d_packed, d_packed8, d_rgb, d_rgb8, static_cast<hipStream_t>(stream));
    });
}

int gi_trace_ray(gi_scene* s, const double origin[3], const double dir[3], const double light[3], gi_hit* hit,
                 double rgb[3]) {
    return guard([&]() -> int {
        DeviceRestore keep;   // the caller's current device, restored on return
        if (!s || !origin || !dir || !light || !hit || !rgb) return fail(GI_ERR_ARG, "null argument");
        std::lock_guard<std::mutex> lk(s->mu);
        int rc = bind_device(s->device);
        if (rc) return rc;
        int32_t* d_i = nullptr;
        double* d_d = nullptr;
        hipError_t e;
        if ((e = hipMalloc((void**)&d_i, 4 * sizeof(int32_t))) != hipSuccess) return hip_fail(e, "hipMalloc");
        if ((e = hipMalloc((void**)&d_d, 9 * sizeof(double))) != hipSuccess) { (void)hipFree(d_i); return hip_fail(e, "hipMalloc"); }
        const V3 o = v3(origin[0], origin[1], origin[2]);
        const V3 d = normalize(v3(dir[0], dir[1], dir[2]));   // Ray ctor (ray.h:6)
        e = launch_trace_ray(s->dev, o, d, v3(light[0], light[1], light[2]), d_i, d_d, nullptr);
        int32_t hi[3] = {-1, 0, 0};
        double hd[9] = {0};
        if (e == hipSuccess) e = hipMemcpy(hi, d_i, 3 * sizeof(int32_t), hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(hd, d_d, 9 * sizeof(double), hipMemcpyDeviceToHost);
        (void)hipFree(d_i);
        (void)hipFree(d_d);
        if (e != hipSuccess) return hip_fail(e, "trace_ray");
        hit->entity = hi[0];
        hit->u = hi[1];
        hit->v = hi[2];
        for (int k = 0; k < 3; ++k) { hit->point[k] = hd[k]; hit->normal[k] = hd[3 + k]; rgb[k] = hd[6 + k]; }
        return GI_OK;
    });
}

// ---- batched ray queries (gi.h "batched ray queries"; gi_wf.hip k_cast) ------------------------
// The scene's immutable records and launch configuration only: no lock, no ordering against the
// scene's renders, nothing of the progressive-frame state (prog_key, prog_next, last) is touched.
namespace {
int check_ray_args(const gi_scene* s, int64_t n, const double* rays) {
    if (!s) return fail(GI_ERR_ARG, "null scene");
    if (n < 0) return fail(GI_ERR_ARG, "negative ray count");
    if (n > 0 && !rays) return fail(GI_ERR_ARG, "null rays");
    return GI_OK;
}
int ray_query_device(gi_scene* s, bool any, const CastIO& io, hipStream_t stream) {
    if (reinterpret_cast<uintptr_t>(io.rays) & 15) return fail(GI_ERR_ARG, "device ray records must be 16-byte aligned");
    int rc = bind_device(s->device);
    if (rc) return rc;
    const hipError_t e = launch_cast(s->dev, x_query_cfg(s->xcfg, 0, any ? WK_OCCL : WK_CAST), any, io, stream);
    return e == hipSuccess ? GI_OK : hip_fail(e, any ? "gi_occluded launch" : "gi_intersect launch");
}
// device staging of a host call: freed on scope exit
struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { (void)hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes); }
};
}  // namespace

int gi_intersect_device(gi_scene* s, int64_t n, const double* d_rays, double* d_t, int32_t* d_prim, int32_t* d_entity,
                        double* d_normal, void* stream) {
    return guard([&]() -> int {
        DeviceRestore keep;   // the caller's current device, restored on return
        int rc = check_ray_args(s, n, d_rays);
        if (rc) return rc;
        if (!d_t && !d_prim && !d_entity && !d_normal) return fail(GI_ERR_ARG, "gi_intersect: every output is null");
        if (n == 0) return GI_OK;
        return ray_query_device(s, false, CastIO{d_rays, (long long)n, d_t, d_prim, d_entity, d_normal, nullptr},
                                static_cast<hipStream_t>(stream));
    });
}

int gi_occluded_device(gi_scene* s, int64_t n, const double* d_rays, int32_t* d_occluded, void* stream) {
    return guard([&]() -> int {
        DeviceRestore keep;   // the caller's current device, restored on return
        int rc = check_ray_args(s, n, d_rays);
        if (rc) return rc;
        if (!d_occluded) return fail(GI_ERR_ARG, "gi_occluded: null output");
        if (n == 0) return GI_OK;
        return ray_query_device(s, true, CastIO{d_rays, (long long)n, nullptr, nullptr, nullptr, nullptr, d_occluded},
                                static_cast<hipStream_t>(stream));
    });
}

int gi_intersect(gi_scene* s, int64_t n, const double* rays, double* t, int32_t* prim, int32_t* entity, double* normal) {
    return guard([&]() -> int {
        DeviceRestore keep;   // the caller's current device, restored on return
        int rc = check_ray_args(s, n, rays);
        if (rc) return rc;
        if (!t && !prim && !entity && !normal) return fail(GI_ERR_ARG, "gi_intersect: every output is null");
        if (n == 0) return GI_OK;
        if ((rc = bind_device(s->device))) return rc;
        const size_t m = (size_t)n;
        DevBuf dr, dt, dp, de, dn;
        hipError_t e = dr.alloc(m * GI_RAY_DOUBLES * sizeof(double));
        if (e == hipSuccess && t) e = dt.alloc(m * sizeof(double));
        if (e == hipSuccess && prim) e = dp.alloc(m * sizeof(int32_t));
        if (e == hipSuccess && entity) e = de.alloc(m * sizeof(int32_t));
        if (e == hipSuccess && normal) e = dn.alloc(m * 3 * sizeof(double));
        if (e != hipSuccess) return hip_fail(e, "hipMalloc (ray query staging)");
        if ((e = hipMemcpy(dr.p, rays, m * GI_RAY_DOUBLES * sizeof(double), hipMemcpyHostToDevice)) != hipSuccess)
            return hip_fail(e, "gi_intersect");
        rc = ray_query_device(s, false, CastIO{static_cast<const double*>(dr.p), (long long)n, static_cast<double*>(dt.p),
                                               static_cast<int32_t*>(dp.p), static_cast<int32_t*>(de.p),
                                               static_cast<double*>(dn.p), nullptr}, nullptr);
        if (rc) return rc;
        if (t) e = hipMemcpy(t, dt.p, m * sizeof(double), hipMemcpyDeviceToHost);   // (synchronous copies on the launch's stream)
        if (e == hipSuccess && prim) e = hipMemcpy(prim, dp.p, m * sizeof(int32_t), hipMemcpyDeviceToHost);
        if (e == hipSuccess && entity) e = hipMemcpy(entity, de.p, m * sizeof(int32_t), hipMemcpyDeviceToHost);
        if (e == hipSuccess && normal) e = hipMemcpy(normal, dn.p, m * 3 * sizeof(double), hipMemcpyDeviceToHost);
        return e == hipSuccess ? GI_OK : hip_fail(e, "gi_intersect");
    });
}

int gi_occluded(gi_scene* s, int64_t n, const double* rays, int32_t* occluded) {
    return guard([&]() -> int {
        DeviceRestore keep;   // the caller's current device, restored on return
        int rc = check_ray_args(s, n, rays);
        if (rc) return rc;
        if (!occluded) return fail(GI_ERR_ARG, "gi_occluded: null output");
        if (n == 0) return GI_OK;
        if ((rc = bind_device(s->device))) return rc;
        const size_t m = (size_t)n;
        DevBuf dr, dc;
        hipError_t e = dr.alloc(m * GI_RAY_DOUBLES * sizeof(double));
        if (e == hipSuccess) e = dc.alloc(m * sizeof(int32_t));
        if (e != hipSuccess) return hip_fail(e, "hipMalloc (ray query staging)");
        if ((e = hipMemcpy(dr.p, rays, m * GI_RAY_DOUBLES * sizeof(double), hipMemcpyHostToDevice)) != hipSuccess)
            return hip_fail(e, "gi_occluded");
        rc = ray_query_device(s, true, CastIO{static_cast<const double*>(dr.p), (long long)n, nullptr, nullptr, nullptr, nullptr,
                                              static_cast<int32_t*>(dc.p)}, nullptr);
        if (rc) return rc;
        e = hipMemcpy(occluded, dc.p, m * sizeof(int32_t), hipMemcpyDeviceToHost);
        return e == hipSuccess ? GI_OK : hip_fail(e, "gi_occluded");
    });
}

// ---- first-hit feature buffers and camera rays (gi.h "feature buffers"; gi_wf.hip k_aov, k_cam_rays) ----
// Like the ray queries: the scene's immutable records and launch configuration only, no lock, no
// ordering against the scene's renders, nothing of the progressive-frame state is touched.
namespace {
// the frame, its window and the camera of an AOV / camera-ray call; *empty: the window holds no pixel
int check_frame_window(const gi_aov_frame* f, bool* empty) {
    if (f->w <= 0 || f->h <= 0 || (int64_t)f->w * f->h > (int64_t)1 << 34) return fail(GI_ERR_ARG, "bad frame size");
    if (f->x0 < 0 || f->y0 < 0 || f->x1 > f->w || f->y1 > f->h || f->x0 > f->x1 || f->y0 > f->y1)
        return fail(GI_ERR_ARG, "the window [x0, x1) x [y0, y1) is reversed or not inside the frame");
    *empty = f->x0 == f->x1 || f->y0 == f->y1;
    return GI_OK;
}
int check_aov_frame(const gi_camera* cam, const gi_aov_frame* f, bool* empty) {
    if (!cam || !f) return fail(GI_ERR_ARG, "null camera or frame");
    const int rc = check_frame_window(f, empty);
    if (rc) return rc;
    bool fin = std::isfinite(cam->focal);
    for (int k = 0; k < 3; ++k) fin = fin && std::isfinite(cam->pos[k]) && std::isfinite(cam->up[k]) && std::isfinite(cam->forward[k]);
    if (!fin) return fail(GI_ERR_ARG, "non-finite camera field");
    return GI_OK;
}
bool aov_all_null(const gi_aov& a) { return !a.t && !a.normal && !a.albedo && !a.prim && !a.entity && !a.uv; }
AovIO aov_io(const gi_aov_frame& f, const gi_aov& a) {
    return AovIO{f.x0, f.y0, f.x1 - f.x0, f.y1 - f.y0, a.t, a.normal, a.albedo, a.prim, a.entity, a.uv};
}
}  // namespace

int gi_render_aov_device(gi_scene* s, const gi_camera* cam, const gi_aov_frame* frame, const gi_aov* d_out, void* stream) {
    return guard([&]() -> int {
        DeviceRestore keep;   // the caller's current device, restored on return
        if (!s) return fail(GI_ERR_ARG, "null scene");
        if (!d_out) return fail(GI_ERR_ARG, "null output struct");
        bool empty = false;
        int rc = check_aov_frame(cam, frame, &empty);
        if (rc) return rc;
        if (aov_all_null(*d_out)) return fail(GI_ERR_ARG, "gi_render_aov: every output is null");
        if (empty) return GI_OK;
        if ((rc = bind_device(s->device))) return rc;
        const hipError_t e = launch_aov(s->dev, x_query_cfg(s->xcfg, 0, WK_AOV), make_cam(*cam, frame->w), aov_io(*frame, *d_out), static_cast<hipStream_t>(stream));
        return e == hipSuccess ? GI_OK : hip_fail(e, "gi_render_aov launch");
    });
}

int gi_render_aov(gi_scene* s, const gi_camera* cam, const gi_aov_frame* frame, const gi_aov* out) {
    return guard([&]() -> int {
        DeviceRestore keep;   // the caller's current device, restored on return
        if (!s) return fail(GI_ERR_ARG, "null scene");
        if (!out) return fail(GI_ERR_ARG, "null output struct");
        bool empty = false;
        int rc = check_aov_frame(cam, frame, &empty);
        if (rc) return rc;
        if (aov_all_null(*out)) return fail(GI_ERR_ARG, "gi_render_aov: every output is null");
        if (empty) return GI_OK;
        if ((rc = bind_device(s->device))) return rc;
        const size_t m = (size_t)(frame->x1 - frame->x0) * (size_t)(frame->y1 - frame->y0);
        DevBuf dt, dn, da, dp, de, du;
        hipError_t e = hipSuccess;
        if (out->t) e = dt.alloc(m * sizeof(double));
        if (e == hipSuccess && out->normal) e = dn.alloc(m * 3 * sizeof(double));
        if (e == hipSuccess && out->albedo) e = da.alloc(m * 3 * sizeof(double));
        if (e == hipSuccess && out->prim) e = dp.alloc(m * sizeof(int32_t));
        if (e == hipSuccess && out->entity) e = de.alloc(m * sizeof(int32_t));
        if (e == hipSuccess && out->uv) e = du.alloc(m * 2 * sizeof(int32_t));
        if (e != hipSuccess) return hip_fail(e, "hipMalloc (feature buffer staging)");
        const gi_aov d{static_cast<double*>(dt.p), static_cast<double*>(dn.p), static_cast<double*>(da.p),
                       static_cast<int32_t*>(dp.p), static_cast<int32_t*>(de.p), static_cast<int32_t*>(du.p)};
        e = launch_aov(s->dev, x_query_cfg(s->xcfg, 0, WK_AOV), make_cam(*cam, frame->w), aov_io(*frame, d), nullptr);
        if (e != hipSuccess) return hip_fail(e, "gi_render_aov launch");
        if (out->t) e = hipMemcpy(out->t, dt.p, m * sizeof(double), hipMemcpyDeviceToHost);   // (synchronous copies on the launch's stream)
        if (e == hipSuccess && out->normal) e = hipMemcpy(out->normal, dn.p, m * 3 * sizeof(double), hipMemcpyDeviceToHost);
        if (e == hipSuccess && out->albedo) e = hipMemcpy(out->albedo, da.p, m * 3 * sizeof(double), hipMemcpyDeviceToHost);
        if (e == hipSuccess && out->prim) e = hipMemcpy(out->prim, dp.p, m * sizeof(int32_t), hipMemcpyDeviceToHost);
        if (e == hipSuccess && out->entity) e = hipMemcpy(out->entity, de.p, m * sizeof(int32_t), hipMemcpyDeviceToHost);
        if (e == hipSuccess && out->uv) e = hipMemcpy(out->uv, du.p, m * 2 * sizeof(int32_t), hipMemcpyDeviceToHost);
        return e == hipSuccess ? GI_OK : hip_fail(e, "gi_render_aov");
    });
}

int gi_camera_rays_device(const gi_camera* cam, const gi_aov_frame* frame, double* d_rays, void* stream) {
    return guard([&]() -> int {
        bool empty = false;
        int rc = check_aov_frame(cam, frame, &empty);
        if (rc) return rc;
        if (!d_rays) return fail(GI_ERR_ARG, "null rays");
        if (reinterpret_cast<uintptr_t>(d_rays) & 15) return fail(GI_ERR_ARG, "device ray records must be 16-byte aligned");
        if (empty) return GI_OK;
        const hipError_t e = launch_cam_rays(make_cam(*cam, frame->w), frame->x0, frame->y0, frame->x1 - frame->x0,
                                             frame->y1 - frame->y0, d_rays, static_cast<hipStream_t>(stream));
        return e == hipSuccess ? GI_OK : hip_fail(e, "gi_camera_rays launch");
    });
}

int gi_camera_rays(const gi_camera* cam, const gi_aov_frame* frame, double* rays) {
    return guard([&]() -> int {
        bool empty = false;
        int rc = check_aov_frame(cam, frame, &empty);
        if (rc) return rc;
        if (!rays) return fail(GI_ERR_ARG, "null rays");
        if (empty) return GI_OK;
        const size_t bytes = (size_t)(frame->x1 - frame->x0) * (size_t)(frame->y1 - frame->y0) * GI_RAY_DOUBLES * sizeof(double);
        DevBuf dr;
        hipError_t e = dr.alloc(bytes);
        if (e != hipSuccess) return hip_fail(e, "hipMalloc (camera ray staging)");
        e = launch_cam_rays(make_cam(*cam, frame->w), frame->x0, frame->y0, frame->x1 - frame->x0, frame->y1 - frame->y0,
                            static_cast<double*>(dr.p), nullptr);
        if (e == hipSuccess) e = hipMemcpy(rays, dr.p, bytes, hipMemcpyDeviceToHost);
        return e == hipSuccess ? GI_OK : hip_fail(e, "gi_camera_rays");
    });
}

// ---- radiance along caller-supplied rays, sample rays, resolve (gi.h "radiance"; gi_wf.hip k_rad, gi_sample.hip) ----
// gi_radiance* like the ray queries: the scene's immutable records and launch configuration only, no lock, no
// ordering against the scene's renders, nothing of the progressive or adaptive frame state is touched.  The
// other two take no scene.
namespace {
// dev: the records are device memory, whose alignment the kernel's loads rely on
int check_radiance(const gi_scene* s, int64_t n, const double* rays, const gi_path_id* ids, const double* light,
                   const gi_radiance_params* p, const double* rgb, bool dev) {
    if (!rays || !light || !p || !rgb) return fail(GI_ERR_ARG, "gi_radiance: null rays, light, params or output");
    if (n < 0) return fail(GI_ERR_ARG, "negative ray count");
    if (n >= (int64_t)1 << 32) return fail(GI_ERR_ARG, "gi_radiance: at most 2^32 - 1 records per call");
    if (p->depth < 1 || p->depth > 0xFFFE) return fail(GI_ERR_ARG, "gi_radiance: 1 <= depth <= 65534");
    if (p->flags & ~GI_FLAG_X_NO_SHADOW) return fail(GI_ERR_ARG, "gi_radiance: unknown flag (GI_FLAG_X_NO_SHADOW only)");
    if (dev && (reinterpret_cast<uintptr_t>(rays) & 15)) return fail(GI_ERR_ARG, "device ray records must be 16-byte aligned");
    if (dev && (reinterpret_cast<uintptr_t>(ids) & 7)) return fail(GI_ERR_ARG, "device path ids must be 8-byte aligned");
    if (!s) return fail(GI_ERR_ARG, "null scene");   // (last: the other refusals need no scene to be seen)
    return GI_OK;
}
int radiance_device(gi_scene* s, int64_t n, const double* d_rays, const gi_path_id* d_ids, const double* light,
                    const gi_radiance_params& p, double* d_rgb, hipStream_t stream) {
    int rc = bind_device(s->device);
    if (rc) return rc;
    const RadIO io{d_rays, reinterpret_cast<const uint64_t*>(d_ids), (long long)n, d_rgb, v3(light[0], light[1], light[2]),
                   p.seed, p.depth, (p.flags & GI_FLAG_X_NO_SHADOW) ? 1 : 0};
    const hipError_t e = launch_rad(s->dev, x_query_cfg(s->xcfg, 0, WK_RAD), io, stream);
    return e == hipSuccess ? GI_OK : hip_fail(e, "gi_radiance launch");
}
// everything of a gi_sample_rays* call but its outputs; *n: the records (0: nothing to launch)
int check_sample(const gi_camera* cam, const gi_aov_frame* f, const gi_sample_params* p, int64_t* n) {
    bool empty = false;
    const int rc = check_aov_frame(cam, f, &empty);
    if (rc) return rc;
    if (!p) return fail(GI_ERR_ARG, "null sample params");
    if (p->sample_begin < 0 || p->sample_end < p->sample_begin)
        return fail(GI_ERR_ARG, "gi_sample_rays: 0 <= sample_begin <= sample_end");
    if (!(p->aperture >= 0.0) || !std::isfinite(p->aperture)) return fail(GI_ERR_ARG, "gi_sample_rays: aperture must be finite and >= 0");
    if (p->aperture > 0.0 && !(std::isfinite(p->focus) && p->focus > 0.0))
        return fail(GI_ERR_ARG, "gi_sample_rays: a lens needs a finite focus > 0");
    if (p->flags & ~GI_SAMPLE_JITTER) return fail(GI_ERR_ARG, "gi_sample_rays: unknown flag");
    if (p->reserved != 0) return fail(GI_ERR_ARG, "gi_sample_rays: reserved must be 0");
    const int64_t px = empty ? 0 : (int64_t)(f->x1 - f->x0) * (int64_t)(f->y1 - f->y0), ns = (int64_t)p->sample_end - p->sample_begin;
    if (px > 0 && ns > 0 && px > (((int64_t)1 << 32) - 1) / ns) return fail(GI_ERR_ARG, "gi_sample_rays: at most 2^32 - 1 records per call");
    *n = px * ns;
    return GI_OK;
}
SampleIO sample_io(const gi_camera& cam, const gi_aov_frame& f, const gi_sample_params& p, double* rays, gi_path_id* ids) {
    return SampleIO{f.x0, f.y0, f.x1 - f.x0, f.y1 - f.y0, f.w, p.sample_begin, p.sample_end, (p.flags & GI_SAMPLE_JITTER) ? 1 : 0,
                    p.seed, p.aperture, p.focus, v3(cam.forward[0], cam.forward[1], cam.forward[2]), rays,
                    reinterpret_cast<uint64_t*>(ids)};
}
int check_resolve(int64_t n_pix, int32_t ns, const double* rows, const double* rgb, const uint8_t* rgb8) {
    if (n_pix < 0) return fail(GI_ERR_ARG, "negative pixel count");
    if (ns < 1) return fail(GI_ERR_ARG, "gi_resolve_samples: ns >= 1");
    if (!rgb && !rgb8) return fail(GI_ERR_ARG, "gi_resolve_samples: every output is null");
    if (n_pix > 0 && !rows) return fail(GI_ERR_ARG, "null rows");
    if (rows && rgb == rows) return fail(GI_ERR_ARG, "gi_resolve_samples: rgb must not be the rows' buffer");
    return GI_OK;
}
}  // namespace

int gi_radiance_device(gi_scene* s, int64_t n, const double* d_rays, const gi_path_id* d_ids, const double light[3],
                       const gi_radiance_params* params, double* d_rgb, void* stream) {
    return guard([&]() -> int {
        DeviceRestore keep;   // the caller's current device, restored on return
        int rc = check_radiance(s, n, d_rays, d_ids, light, params, d_rgb, true);
        if (rc) return rc;
        if (n == 0) return GI_OK;
        return radiance_device(s, n, d_rays, d_ids, light, *params, d_rgb, static_cast<hipStream_t>(stream));
    });
}

int gi_radiance(gi_scene* s, int64_t n, const double* rays, const gi_path_id* ids, const double light[3],
                const gi_radiance_params* params, double* rgb) {
    return guard([&]() -> int {
        DeviceRestore keep;   // the caller's current device, restored on return
        int rc = check_radiance(s, n, rays, ids, light, params, rgb, false);
        if (rc) return rc;
        if (n == 0) return GI_OK;
        if ((rc = bind_device(s->device))) return rc;
        const size_t m = (size_t)n;
        DevBuf dr, di, dc;
        hipError_t e = dr.alloc(m * GI_RAY_DOUBLES * sizeof(double));
        if (e == hipSuccess && ids) e = di.alloc(m * sizeof(gi_path_id));
        if (e == hipSuccess) e = dc.alloc(m * 3 * sizeof(double));
        if (e != hipSuccess) return hip_fail(e, "hipMalloc (radiance staging)");
        e = hipMemcpy(dr.p, rays, m * GI_RAY_DOUBLES * sizeof(double), hipMemcpyHostToDevice);
        if (e == hipSuccess && ids) e = hipMemcpy(di.p, ids, m * sizeof(gi_path_id), hipMemcpyHostToDevice);
        if (e != hipSuccess) return hip_fail(e, "gi_radiance");
        rc = radiance_device(s, n, static_cast<const double*>(dr.p), static_cast<const gi_path_id*>(di.p), light, *params,
                             static_cast<double*>(dc.p), nullptr);
        if (rc) return rc;
        e = hipMemcpy(rgb, dc.p, m * 3 * sizeof(double), hipMemcpyDeviceToHost);   // (synchronous copy on the launch's stream)
        return e == hipSuccess ? GI_OK : hip_fail(e, "gi_radiance");
    });
}

int gi_sample_rays_device(const gi_camera* cam, const gi_aov_frame* frame, const gi_sample_params* params, double* d_rays,
                          gi_path_id* d_ids, void* stream) {
    return guard([&]() -> int {
        int64_t n = 0;
        int rc = check_sample(cam, frame, params, &n);
        if (rc) return rc;
        if (!d_rays && !d_ids) return fail(GI_ERR_ARG, "gi_sample_rays: every output is null");
        if (reinterpret_cast<uintptr_t>(d_rays) & 15) return fail(GI_ERR_ARG, "device ray records must be 16-byte aligned");
        if (reinterpret_cast<uintptr_t>(d_ids) & 7) return fail(GI_ERR_ARG, "device path ids must be 8-byte aligned");
        if (n == 0) return GI_OK;
        const hipError_t e = launch_sample_rays(make_cam(*cam, frame->w), sample_io(*cam, *frame, *params, d_rays, d_ids),
                                                static_cast<hipStream_t>(stream));
        return e == hipSuccess ? GI_OK : hip_fail(e, "gi_sample_rays launch");
    });
}

int gi_sample_rays(const gi_camera* cam, const gi_aov_frame* frame, const gi_sample_params* params, double* rays,
                   gi_path_id* ids) {
    return guard([&]() -> int {
        int64_t n = 0;
        int rc = check_sample(cam, frame, params, &n);
        if (rc) return rc;
        if (!rays && !ids) return fail(GI_ERR_ARG, "gi_sample_rays: every output is null");
        if (n == 0) return GI_OK;
        const size_t m = (size_t)n;
        DevBuf dr, di;
        hipError_t e = hipSuccess;
        if (rays) e = dr.alloc(m * GI_RAY_DOUBLES * sizeof(double));
        if (e == hipSuccess && ids) e = di.alloc(m * sizeof(gi_path_id));
        if (e != hipSuccess) return hip_fail(e, "hipMalloc (sample ray staging)");
        e = launch_sample_rays(make_cam(*cam, frame->w),
                               sample_io(*cam, *frame, *params, static_cast<double*>(dr.p), static_cast<gi_path_id*>(di.p)), nullptr);
        if (e == hipSuccess && rays) e = hipMemcpy(rays, dr.p, m * GI_RAY_DOUBLES * sizeof(double), hipMemcpyDeviceToHost);
        if (e == hipSuccess && ids) e = hipMemcpy(ids, di.p, m * sizeof(gi_path_id), hipMemcpyDeviceToHost);
        return e == hipSuccess ? GI_OK : hip_fail(e, "gi_sample_rays");
    });
}

int gi_resolve_samples_device(int64_t n_pix, int32_t ns, const double* d_rows, double* d_rgb, uint8_t* d_rgb8, void* stream) {
    return guard([&]() -> int {
        const int rc = check_resolve(n_pix, ns, d_rows, d_rgb, d_rgb8);
        if (rc) return rc;
        if (n_pix == 0) return GI_OK;
        const hipError_t e = launch_resolve((long long)n_pix, ns, d_rows, d_rgb, d_rgb8, static_cast<hipStream_t>(stream));
        return e == hipSuccess ? GI_OK : hip_fail(e, "gi_resolve_samples launch");
    });
}

int gi_resolve_samples(int64_t n_pix, int32_t ns, const double* rows, double* rgb, uint8_t* rgb8) {
    return guard([&]() -> int {
        const int rc = check_resolve(n_pix, ns, rows, rgb, rgb8);
        if (rc) return rc;
        if (n_pix == 0) return GI_OK;
        const size_t m = (size_t)n_pix;
        DevBuf dr, dc, d8;
        hipError_t e = dr.alloc(m * (size_t)ns * 3 * sizeof(double));
        if (e == hipSuccess && rgb) e = dc.alloc(m * 3 * sizeof(double));
        if (e == hipSuccess && rgb8) e = d8.alloc(m * 3);
        if (e != hipSuccess) return hip_fail(e, "hipMalloc (resolve staging)");
        e = hipMemcpy(dr.p, rows, m * (size_t)ns * 3 * sizeof(double), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = launch_resolve((long long)n_pix, ns, static_cast<const double*>(dr.p), static_cast<double*>(dc.p),
                                                static_cast<uint8_t*>(d8.p), nullptr);
        if (e == hipSuccess && rgb) e = hipMemcpy(rgb, dc.p, m * 3 * sizeof(double), hipMemcpyDeviceToHost);
        if (e == hipSuccess && rgb8) e = hipMemcpy(rgb8, d8.p, m * 3, hipMemcpyDeviceToHost);
        return e == hipSuccess ? GI_OK : hip_fail(e, "gi_resolve_samples");
    });
}

// ---- sample moments of the retained frame (gi.h "sample moments"; gi_kernels.hip k_x_moments) ----
// Unlike the queries above these read the scene's Mode X scratch: under the scene's mutex, and ordered on the
// device with the scene's `last` event in both directions.  Nothing of the progressive-frame state is touched.
namespace {
// everything of a moments call; the scene's mutex is held.  *empty: the window holds no pixel
int check_moments(const gi_scene* s, const gi_aov_frame* frame, const gi_moments* out, bool* empty) {
    if (!out->mean && !out->var && !out->samples) return fail(GI_ERR_ARG, "gi_frame_moments: every output is null");
    if (s->keep_n == 0)
        return fail(GI_ERR_ARG, "gi_frame_moments: no retained frame (the scene's last render was not a whole Mode X frame with "
                                "spp > 1 on one shard, or it failed)");
    if (s->keep_n < 2) return fail(GI_ERR_ARG, "gi_frame_moments: fewer than 2 samples rendered so far");
    const int rc = check_frame_window(frame, empty);
    if (rc) return rc;
    if (frame->w != s->keep_w || frame->h != s->keep_h) return fail(GI_ERR_ARG, "gi_frame_moments: the frame is not the retained frame's size");
    return GI_OK;
}
int issue_moments(gi_scene* s, const gi_aov_frame& f, const gi_moments& d, hipStream_t stream) {
    int rc = bind_device(s->device);
    if (rc) return rc;
    hipError_t e = hipSuccess;
    if (s->launched && (e = hipStreamWaitEvent(stream, s->last, 0)) != hipSuccess) return hip_fail(e, "hipStreamWaitEvent");
    const MomentsIO io{f.x0, f.y0, f.x1 - f.x0, f.y1 - f.y0, s->keep_spp, s->keep_n, d.mean, d.var, d.samples};
    if ((e = launch_moments(s->dev, s->xs, s->keep_cam, f.w, f.h, io, stream)) != hipSuccess) return hip_fail(e, "gi_frame_moments launch");
    // the scene's next render overwrites the rows: it waits for this call
    if ((e = hipEventRecord(s->last, stream)) != hipSuccess) return hip_fail(e, "hipEventRecord");
    return GI_OK;
}
}  // namespace

int gi_frame_samples_info(gi_scene* s, int32_t* w, int32_t* h, int32_t* n, int32_t* spp) {
    return guard([&]() -> int {
        if (!s) return fail(GI_ERR_ARG, "null scene");
        std::lock_guard<std::mutex> lk(s->mu);
        if (s->keep_n == 0) return fail(GI_ERR_ARG, "gi_frame_samples_info: no retained frame");
        if (w) *w = s->keep_w;
        if (h) *h = s->keep_h;
        if (n) *n = s->keep_n;
        if (spp) *spp = s->keep_spp;
        return GI_OK;
    });
}

int gi_frame_moments_device(gi_scene* s, const gi_aov_frame* frame, const gi_moments* d_out, void* stream) {
    return guard([&]() -> int {
        DeviceRestore keep;   // the caller's current device, restored on return
        if (!s) return fail(GI_ERR_ARG, "null scene");
        if (!frame || !d_out) return fail(GI_ERR_ARG, "null frame or output struct");
        std::lock_guard<std::mutex> lk(s->mu);
        bool empty = false;
        const int rc = check_moments(s, frame, d_out, &empty);
        if (rc || empty) return rc;
        return issue_moments(s, *frame, *d_out, static_cast<hipStream_t>(stream));
    });
}

int gi_frame_moments(gi_scene* s, const gi_aov_frame* frame, const gi_moments* out) {
    return guard([&]() -> int {
        DeviceRestore keep;   // the caller's current device, restored on return
        if (!s) return fail(GI_ERR_ARG, "null scene");
        if (!frame || !out) return fail(GI_ERR_ARG, "null frame or output struct");
        std::lock_guard<std::mutex> lk(s->mu);
        bool empty = false;
        int rc = check_moments(s, frame, out, &empty);
        if (rc || empty) return rc;
        if ((rc = bind_device(s->device))) return rc;
        const size_t m = (size_t)(frame->x1 - frame->x0) * (size_t)(frame->y1 - frame->y0), ns = m * 3 * (size_t)s->keep_n;
        DevBuf dm, dv, ds;
        hipError_t e = hipSuccess;
        if (out->mean) e = dm.alloc(m * 3 * sizeof(double));
        if (e == hipSuccess && out->var) e = dv.alloc(m * 3 * sizeof(double));
        if (e == hipSuccess && out->samples) e = ds.alloc(ns * sizeof(double));
        if (e != hipSuccess) return hip_fail(e, "hipMalloc (moments staging)");
        const gi_moments d{static_cast<double*>(dm.p), static_cast<double*>(dv.p), static_cast<double*>(ds.p)};
        if ((rc = issue_moments(s, *frame, d, nullptr))) return rc;
        if (out->mean) e = hipMemcpy(out->mean, dm.p, m * 3 * sizeof(double), hipMemcpyDeviceToHost);   // (synchronous copies on the launch's stream)
        if (e == hipSuccess && out->var) e = hipMemcpy(out->var, dv.p, m * 3 * sizeof(double), hipMemcpyDeviceToHost);
        if (e == hipSuccess && out->samples) e = hipMemcpy(out->samples, ds.p, ns * sizeof(double), hipMemcpyDeviceToHost);
        return e == hipSuccess ? GI_OK : hip_fail(e, "gi_frame_moments");
    });
}

// ---- adaptive sampling (gi.h "adaptive sampling"; gi_adapt.hip, gi_kernels.hip launch_adaptive) ----
// A pass is a render: under the scene's mutex, ordered on the device by the scene's `last` event, and it ends the
// retained frame and any plain progressive frame.  The frame's continuation state is the scene's ad_* fields.
namespace {
int check_adaptive(int w, int h, const gi_opts* o, const gi_adaptive_params* p, const gi_adaptive_out* out) {
    int rc = check_opts(w, h, o);
    if (rc) return rc;
    if (!p || !out) return fail(GI_ERR_ARG, "gi_render_adaptive: null params or output struct");
    if (!out->rgb && !out->rgb8 && !out->mean && !out->var && !out->n) return fail(GI_ERR_ARG, "gi_render_adaptive: every output is null");
    if (o->mode != GI_MODE_X) return fail(GI_ERR_ARG, "gi_render_adaptive: mode X only");
    if (o->shard_count != 1) return fail(GI_ERR_ARG, "gi_render_adaptive: whole frames only (shard_count 1)");
    if (o->sample_begin < 0 || o->sample_end > o->spp || (int64_t)o->sample_end - (int64_t)o->sample_begin < 2)
        return fail(GI_ERR_ARG, "gi_render_adaptive: a pass is 0 <= sample_begin, sample_begin + 2 <= sample_end <= spp");
    if (p->min_samples < 2) return fail(GI_ERR_ARG, "gi_render_adaptive: min_samples >= 2");
    if (p->flags & ~GI_ADAPTIVE_RELATIVE) return fail(GI_ERR_ARG, "gi_render_adaptive: unknown flag");
    if (!(p->tol > 0)) return fail(GI_ERR_ARG, "gi_render_adaptive: tol > 0 (+inf allowed)");
    if ((p->flags & GI_ADAPTIVE_RELATIVE) && !(p->y_floor > 0 && std::isfinite(p->y_floor)))
        return fail(GI_ERR_ARG, "gi_render_adaptive: GI_ADAPTIVE_RELATIVE needs a finite y_floor > 0");
    return GI_OK;
}
uint64_t adaptive_key(const gi_camera& c, const double light[3], int w, int h, const gi_opts& o, const gi_adaptive_params& p) {
    uint64_t k = prog_key(c, light, w, h, o);
    auto mix = [&](const void* q, size_t n) {
        for (size_t i = 0; i < n; ++i) k = (k ^ static_cast<const unsigned char*>(q)[i]) * 1099511628211ull;
    };
    const int64_t v[2] = {p.min_samples, (int64_t)p.flags};
    const double d[2] = {p.tol, (p.flags & GI_ADAPTIVE_RELATIVE) ? p.y_floor : 0.0};
    mix(v, sizeof v);
    mix(d, sizeof d);
    return k;
}
// the second list, the counts and the per-slot state for the slots the work list holds; grown, never shrunk
int ensure_adaptive(gi_scene* s) {
    XScratch& x = s->xs;
    if (x.ad_cap >= x.cap && x.ad_cap > 0) return GI_OK;
    for (void* q : {(void*)x.ad_list, (void*)x.ad_cnt, (void*)x.ad_sum, (void*)x.ad_n}) (void)hipFree(q);
    x.ad_list = x.ad_cnt = nullptr;
    x.ad_sum = nullptr;
    x.ad_n = nullptr;
    x.ad_cap = 0;
    hipError_t e;
    if ((e = hipMalloc((void**)&x.ad_list, (size_t)x.cap * sizeof(unsigned))) != hipSuccess ||
        (e = hipMalloc((void**)&x.ad_cnt, 4 * sizeof(unsigned))) != hipSuccess ||
        (e = hipMalloc((void**)&x.ad_sum, (size_t)x.cap * 6 * sizeof(double))) != hipSuccess ||
        (e = hipMalloc((void**)&x.ad_n, (size_t)x.cap * sizeof(int32_t))) != hipSuccess)
        return hip_fail(e, "hipMalloc (adaptive state)");
    x.ad_cap = x.cap;
    return GI_OK;
}
// one pass with device planes on `stream`; the scene's mutex is held
int adaptive_pass(gi_scene* s, const gi_camera* cam, const double light[3], int w, int h, const gi_opts* o,
                  const gi_adaptive_params* p, const gi_adaptive_out* d_out, hipStream_t stream) {
    // a render: it ends the retained frame and a plain progressive frame; a refused pass ends the adaptive frame too
    const int next = s->ad_next;
    s->keep_n = 0;
    s->prog_next = -1;
    s->ad_next = -1;
    if (!cam || !light) return fail(GI_ERR_ARG, "null camera or light");
    int rc = check_adaptive(w, h, o, p, d_out);
    if (rc) return rc;
    const uint64_t key = adaptive_key(*cam, light, w, h, *o, *p);
    if (o->sample_begin > 0) {
        if (next != o->sample_begin || s->ad_key != key || !s->launched)
            return fail(GI_ERR_ARG, "adaptive pass out of order: a pass continues the previous adaptive pass's frame (same camera, "
                                    "light, size, spp, depth, seed, flags and params) from its sample_end");
        // the previous pass was accepted when issued: a device error since ends the frame
        const hipError_t q = hipEventQuery(s->last);
        if (q != hipSuccess && q != hipErrorNotReady)
            return hip_fail(q, "adaptive pass: the previous pass failed on the device; restart the frame at sample 0");
    }
    gi_opts o2 = *o;   // the pass as the render kernels see it: the stride of its rows is its k samples
    o2.spp = o->sample_end - o->sample_begin;
    if ((rc = bind_device(s->device)) || (rc = ensure_xscratch(s, w, h, &o2)) || (rc = ensure_adaptive(s)) || (rc = ensure_timer(s, &o2)))
        return rc;
    const CamDev cd = make_cam(*cam, w);
    XAdaptPass ap;
    ap.p = *p;
    ap.out = *d_out;
    ap.spp_max = o->spp;
    ap.cur = o->sample_begin > 0 ? s->ad_cur : 0;
    hipError_t e = hipSuccess;
    if (!s->last && (e = hipEventCreateWithFlags(&s->last, hipEventDisableTiming)) != hipSuccess) return hip_fail(e, "hipEventCreate");
    if (s->launched && (e = hipStreamWaitEvent(stream, s->last, 0)) != hipSuccess) return hip_fail(e, "hipStreamWaitEvent");
    s->ad_done = 0;
    e = launch_adaptive(s->dev, s->xcfg, cd, v3(light[0], light[1], light[2]), w, h, o2, ap, s->xs, &s->kt, stream);
    if (e != hipSuccess) return hip_fail(e, "adaptive pass launch");
    if ((e = hipEventRecord(s->last, stream)) != hipSuccess) return hip_fail(e, "hipEventRecord");
    s->launched = true;
    s->ad_key = key;
    s->ad_cur = ap.cur ^ 1;   // the survivors' list: the next pass's, and the count gi_adaptive_info reads
    s->ad_next = o->sample_end < o->spp ? o->sample_end : -1;
    s->ad_w = w;
    s->ad_h = h;
    s->ad_done = o->sample_end;
    return GI_OK;
}
}  // namespace

int gi_render_adaptive_device(gi_scene* s, const gi_camera* cam, const double light[3], int w, int h, const gi_opts* o,
                              const gi_adaptive_params* p, const gi_adaptive_out* d_out, void* stream) {
    return guard([&]() -> int {
        DeviceRestore keep;   // the caller's current device, restored on return
        if (!s) return fail(GI_ERR_ARG, "null scene");
        std::lock_guard<std::mutex> lk(s->mu);
        return adaptive_pass(s, cam, light, w, h, o, p, d_out, static_cast<hipStream_t>(stream));
    });
}

int gi_render_adaptive(gi_scene* s, const gi_camera* cam, const double light[3], int w, int h, const gi_opts* o,
                       const gi_adaptive_params* p, const gi_adaptive_out* out) {
    return guard([&]() -> int {
        DeviceRestore keep;   // the caller's current device, restored on return
        if (!s) return fail(GI_ERR_ARG, "null scene");
        std::lock_guard<std::mutex> lk(s->mu);
        if (!out || w <= 0 || h <= 0 || (int64_t)w * h > (int64_t)1 << 34)   // (the rest: adaptive_pass)
            return adaptive_pass(s, cam, light, w, h, o, p, out, nullptr);
        int rc = bind_device(s->device);
        if (rc) return rc;
        const size_t px = (size_t)w * (size_t)h;
        DevBuf b_rgb, b_rgb8, b_mean, b_var, b_n;
        hipError_t e = hipSuccess;
        if (out->rgb) e = b_rgb.alloc(px * 3 * sizeof(double));
        if (e == hipSuccess && out->rgb8) e = b_rgb8.alloc(px * 3);
        if (e == hipSuccess && out->mean) e = b_mean.alloc(px * 3 * sizeof(double));
        if (e == hipSuccess && out->var) e = b_var.alloc(px * 3 * sizeof(double));
        if (e == hipSuccess && out->n) e = b_n.alloc(px * sizeof(int32_t));
        if (e != hipSuccess) return hip_fail(e, "hipMalloc (adaptive staging)");
        const gi_adaptive_out d{static_cast<double*>(b_rgb.p), static_cast<uint8_t*>(b_rgb8.p), static_cast<double*>(b_mean.p),
                                static_cast<double*>(b_var.p), static_cast<int32_t*>(b_n.p)};
        if ((rc = adaptive_pass(s, cam, light, w, h, o, p, &d, nullptr))) return rc;
        if (out->rgb) e = hipMemcpy(out->rgb, d.rgb, px * 3 * sizeof(double), hipMemcpyDeviceToHost);   // (synchronous copies on the launch's stream)
        if (e == hipSuccess && out->rgb8) e = hipMemcpy(out->rgb8, d.rgb8, px * 3, hipMemcpyDeviceToHost);
        if (e == hipSuccess && out->mean) e = hipMemcpy(out->mean, d.mean, px * 3 * sizeof(double), hipMemcpyDeviceToHost);
        if (e == hipSuccess && out->var) e = hipMemcpy(out->var, d.var, px * 3 * sizeof(double), hipMemcpyDeviceToHost);
        if (e == hipSuccess && out->n) e = hipMemcpy(out->n, d.n, px * sizeof(int32_t), hipMemcpyDeviceToHost);
        if (e != hipSuccess) {
            s->ad_next = -1;
            return hip_fail(e, "gi_render_adaptive");
        }
        return GI_OK;
    });
}

int gi_adaptive_info(gi_scene* s, int32_t* w, int32_t* h, int32_t* samples_done, int64_t* active) {
    return guard([&]() -> int {
        DeviceRestore keep;   // the caller's current device, restored on return
        if (!s) return fail(GI_ERR_ARG, "null scene");
        std::lock_guard<std::mutex> lk(s->mu);
        if (s->ad_done == 0) return fail(GI_ERR_ARG, "gi_adaptive_info: no adaptive frame");
        int rc = bind_device(s->device);
        if (rc) return rc;
        unsigned cnt = 0;
        if (active) {   // waits for the last pass, then reads the survivors' count
            hipError_t e = hipEventSynchronize(s->last);
            if (e == hipSuccess) e = hipMemcpy(&cnt, s->xs.ad_cnt + s->ad_cur, sizeof cnt, hipMemcpyDeviceToHost);
            if (e != hipSuccess) return hip_fail(e, "gi_adaptive_info");
        }
        if (w) *w = s->ad_w;
        if (h) *h = s->ad_h;
        if (samples_done) *samples_done = s->ad_done;
        if (active) *active = (int64_t)cnt;
        return GI_OK;
    });
}

// ---- denoiser (gi.h "denoiser"; gi_denoise.hip k_dn_prep, k_dn_level) ----
// No scene and no state: the caller's planes and scratch on the current device.
namespace {
int check_denoise_params(const gi_denoise_params* p) {
    if (!p) return fail(GI_ERR_ARG, "null denoise parameters");
    if (p->levels < 1 || p->levels > 8) return fail(GI_ERR_ARG, "gi_denoise: levels outside 1..8");
    if (p->normal_pow_log2 < 0 || p->normal_pow_log2 > 7) return fail(GI_ERR_ARG, "gi_denoise: normal_pow_log2 outside 0..7");
    if (p->flags & ~GI_DENOISE_ALBEDO_STOP) return fail(GI_ERR_ARG, "gi_denoise: unknown flag");
    if (p->reserved != 0) return fail(GI_ERR_ARG, "gi_denoise: reserved must be 0");
    if (!(p->sigma_c > 0) || !(p->sigma_p > 0)) return fail(GI_ERR_ARG, "gi_denoise: sigma_c and sigma_p must be > 0 (+inf: no stop)");
    return GI_OK;
}
// everything of a denoise call but the scratch; *empty: the window holds no pixel
int check_denoise(const gi_camera* cam, const gi_aov_frame* frame, const gi_denoise_params* p, const gi_denoise_io* io, bool* empty) {
    if (!io) return fail(GI_ERR_ARG, "null denoise io");
    int rc = check_aov_frame(cam, frame, empty);
    if (rc || (rc = check_denoise_params(p))) return rc;
    if (!io->rgb || !io->t || !io->normal) return fail(GI_ERR_ARG, "gi_denoise: null rgb, t or normal");
    if (!io->out_rgb && !io->out_rgb8) return fail(GI_ERR_ARG, "gi_denoise: both outputs are null");
    if ((p->flags & GI_DENOISE_ALBEDO_STOP) && !io->albedo) return fail(GI_ERR_ARG, "gi_denoise: the albedo stop needs the albedo plane");
    if (io->out_rgb == io->rgb) return fail(GI_ERR_ARG, "gi_denoise: out_rgb must not be rgb");
    return GI_OK;
}
int64_t denoise_bytes(const gi_aov_frame& f, const gi_denoise_params& p) {
    return dn_scratch_bytes((long long)(f.x1 - f.x0) * (long long)(f.y1 - f.y0), p.levels, (p.flags & GI_DENOISE_ALBEDO_STOP) != 0);
}
DnIO dn_io(const gi_aov_frame& f, const gi_denoise_io& d) {
    return DnIO{f.x0, f.y0, f.x1 - f.x0, f.y1 - f.y0, d.rgb, d.t, d.normal, d.albedo, d.out_rgb, d.out_rgb8};
}
}  // namespace

int64_t gi_denoise_scratch_bytes(const gi_aov_frame* frame, const gi_denoise_params* p) {   // (nothing here can throw)
    if (!frame) return fail(GI_ERR_ARG, "null frame");
    bool empty = false;
    int rc = check_frame_window(frame, &empty);
    if (rc || (rc = check_denoise_params(p))) return rc;
    return empty ? 0 : denoise_bytes(*frame, *p);
}

int gi_denoise_device(const gi_camera* cam, const gi_aov_frame* frame, const gi_denoise_params* p, const gi_denoise_io* d_io,
                      void* d_scratch, int64_t scratch_bytes, void* stream) {
    return guard([&]() -> int {
        bool empty = false;
        const int rc = check_denoise(cam, frame, p, d_io, &empty);
        if (rc) return rc;
        if (scratch_bytes < (empty ? 0 : denoise_bytes(*frame, *p))) return fail(GI_ERR_ARG, "gi_denoise: scratch_bytes below gi_denoise_scratch_bytes");
        if (empty) return GI_OK;
        if (!d_scratch || (reinterpret_cast<uintptr_t>(d_scratch) & 15)) return fail(GI_ERR_ARG, "gi_denoise: the device scratch must be non-null and 16-byte aligned");
        const hipError_t e = launch_denoise(make_cam(*cam, frame->w), dn_io(*frame, *d_io), *p, d_scratch, static_cast<hipStream_t>(stream));
        return e == hipSuccess ? GI_OK : hip_fail(e, "gi_denoise launch");
    });
}

int gi_denoise(const gi_camera* cam, const gi_aov_frame* frame, const gi_denoise_params* p, const gi_denoise_io* io) {
    return guard([&]() -> int {
        bool empty = false;
        const int rc = check_denoise(cam, frame, p, io, &empty);
        if (rc) return rc;
        if (empty) return GI_OK;
        const size_t m = (size_t)(frame->x1 - frame->x0) * (size_t)(frame->y1 - frame->y0);
        const bool stop = (p->flags & GI_DENOISE_ALBEDO_STOP) != 0;
        DevBuf drgb, dt, dn, da, dout, dout8, dscr;
        hipError_t e = drgb.alloc(m * 3 * sizeof(double));
        if (e == hipSuccess) e = dt.alloc(m * sizeof(double));
        if (e == hipSuccess) e = dn.alloc(m * 3 * sizeof(double));
        if (e == hipSuccess && stop) e = da.alloc(m * 3 * sizeof(double));
        if (e == hipSuccess && io->out_rgb) e = dout.alloc(m * 3 * sizeof(double));
        if (e == hipSuccess && io->out_rgb8) e = dout8.alloc(m * 3);
        if (e == hipSuccess) e = dscr.alloc((size_t)denoise_bytes(*frame, *p));
        if (e != hipSuccess) return hip_fail(e, "hipMalloc (denoiser staging)");
        e = hipMemcpy(drgb.p, io->rgb, m * 3 * sizeof(double), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(dt.p, io->t, m * sizeof(double), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(dn.p, io->normal, m * 3 * sizeof(double), hipMemcpyHostToDevice);
        if (e == hipSuccess && stop) e = hipMemcpy(da.p, io->albedo, m * 3 * sizeof(double), hipMemcpyHostToDevice);
        if (e != hipSuccess) return hip_fail(e, "gi_denoise");
        const gi_denoise_io d{static_cast<const double*>(drgb.p), static_cast<const double*>(dt.p), static_cast<const double*>(dn.p),
                              static_cast<const double*>(da.p), static_cast<double*>(dout.p), static_cast<uint8_t*>(dout8.p)};
        e = launch_denoise(make_cam(*cam, frame->w), dn_io(*frame, d), *p, dscr.p, nullptr);
        if (e != hipSuccess) return hip_fail(e, "gi_denoise launch");
        if (io->out_rgb) e = hipMemcpy(io->out_rgb, dout.p, m * 3 * sizeof(double), hipMemcpyDeviceToHost);   // (synchronous copies on the launch's stream)
        if (e == hipSuccess && io->out_rgb8) e = hipMemcpy(io->out_rgb8, dout8.p, m * 3, hipMemcpyDeviceToHost);
        return e == hipSuccess ? GI_OK : hip_fail(e, "gi_denoise");
    });
}

// ---- variance-guided denoiser (gi.h "variance-guided denoiser"; gi_denoise.hip k_dnv_g, k_dnv_level) ----
namespace {
int check_denoise_var_params(const gi_denoise_var_params* p) {
    if (!p) return fail(GI_ERR_ARG, "null denoise parameters");
    const gi_denoise_params q{p->levels, p->normal_pow_log2, p->flags, p->reserved, p->sigma_v, p->sigma_p};
    const int rc = check_denoise_params(&q);   // (sigma_v judged as sigma_c)
    if (rc) return rc;
    if (!(p->var_floor > 0) || !std::isfinite(p->var_floor)) return fail(GI_ERR_ARG, "gi_denoise_var: var_floor must be finite and > 0");
    return GI_OK;
}
int check_denoise_var(const gi_camera* cam, const gi_aov_frame* frame, const gi_denoise_var_params* p, const gi_denoise_var_io* io,
                      bool* empty) {
    if (!io) return fail(GI_ERR_ARG, "null denoise io");
    int rc = check_aov_frame(cam, frame, empty);
    if (rc || (rc = check_denoise_var_params(p))) return rc;
    if (!io->rgb || !io->var || !io->t || !io->normal) return fail(GI_ERR_ARG, "gi_denoise_var: null rgb, var, t or normal");
    if (!io->out_rgb && !io->out_var && !io->out_rgb8) return fail(GI_ERR_ARG, "gi_denoise_var: every output is null");
    if ((p->flags & GI_DENOISE_ALBEDO_STOP) && !io->albedo) return fail(GI_ERR_ARG, "gi_denoise_var: the albedo stop needs the albedo plane");
    if (io->out_rgb == io->rgb || io->out_var == io->var) return fail(GI_ERR_ARG, "gi_denoise_var: out_rgb must not be rgb, out_var not var");
    return GI_OK;
}
int64_t denoise_var_bytes(const gi_aov_frame& f, const gi_denoise_var_params& p) {
    return dnv_scratch_bytes((long long)(f.x1 - f.x0) * (long long)(f.y1 - f.y0), p.levels, (p.flags & GI_DENOISE_ALBEDO_STOP) != 0);
}
DnvIO dnv_io(const gi_aov_frame& f, const gi_denoise_var_io& d) {
    return DnvIO{f.x0, f.y0, f.x1 - f.x0, f.y1 - f.y0, d.rgb, d.var, d.t, d.normal, d.albedo, d.out_rgb, d.out_var, d.out_rgb8};
}
}  // namespace

int64_t gi_denoise_var_scratch_bytes(const gi_aov_frame* frame, const gi_denoise_var_params* p) {   // (nothing here can throw)
    if (!frame) return fail(GI_ERR_ARG, "null frame");
    bool empty = false;
    int rc = check_frame_window(frame, &empty);
    if (rc || (rc = check_denoise_var_params(p))) return rc;
    return empty ? 0 : denoise_var_bytes(*frame, *p);
}

int gi_denoise_var_device(const gi_camera* cam, const gi_aov_frame* frame, const gi_denoise_var_params* p, const gi_denoise_var_io* d_io,
                          void* d_scratch, int64_t scratch_bytes, void* stream) {
    return guard([&]() -> int {
        bool empty = false;
        const int rc = check_denoise_var(cam, frame, p, d_io, &empty);
        if (rc) return rc;
        if (scratch_bytes < (empty ? 0 : denoise_var_bytes(*frame, *p)))
            return fail(GI_ERR_ARG, "gi_denoise_var: scratch_bytes below gi_denoise_var_scratch_bytes");
        if (empty) return GI_OK;
        if (!d_scratch || (reinterpret_cast<uintptr_t>(d_scratch) & 15))
            return fail(GI_ERR_ARG, "gi_denoise_var: the device scratch must be non-null and 16-byte aligned");
        const hipError_t e = launch_denoise_var(make_cam(*cam, frame->w), dnv_io(*frame, *d_io), *p, d_scratch, static_cast<hipStream_t>(stream));
        return e == hipSuccess ? GI_OK : hip_fail(e, "gi_denoise_var launch");
    });
}

int gi_denoise_var(const gi_camera* cam, const gi_aov_frame* frame, const gi_denoise_var_params* p, const gi_denoise_var_io* io) {
    return guard([&]() -> int {
        bool empty = false;
        const int rc = check_denoise_var(cam, frame, p, io, &empty);
        if (rc) return rc;
        if (empty) return GI_OK;
        const size_t m = (size_t)(frame->x1 - frame->x0) * (size_t)(frame->y1 - frame->y0), b3 = m * 3 * sizeof(double);
        const bool stop = (p->flags & GI_DENOISE_ALBEDO_STOP) != 0;
        DevBuf drgb, dvar, dt, dn, da, dout, dovar, dout8, dscr;
        hipError_t e = drgb.alloc(b3);
        if (e == hipSuccess) e = dvar.alloc(b3);
        if (e == hipSuccess) e = dt.alloc(m * sizeof(double));
        if (e == hipSuccess) e = dn.alloc(b3);
        if (e == hipSuccess && stop) e = da.alloc(b3);
        if (e == hipSuccess && io->out_rgb) e = dout.alloc(b3);
        if (e == hipSuccess && io->out_var) e = dovar.alloc(b3);
        if (e == hipSuccess && io->out_rgb8) e = dout8.alloc(m * 3);
        if (e == hipSuccess) e = dscr.alloc((size_t)denoise_var_bytes(*frame, *p));
        if (e != hipSuccess) return hip_fail(e, "hipMalloc (denoiser staging)");
        e = hipMemcpy(drgb.p, io->rgb, b3, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(dvar.p, io->var, b3, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(dt.p, io->t, m * sizeof(double), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(dn.p, io->normal, b3, hipMemcpyHostToDevice);
        if (e == hipSuccess && stop) e = hipMemcpy(da.p, io->albedo, b3, hipMemcpyHostToDevice);
        if (e != hipSuccess) return hip_fail(e, "gi_denoise_var");
        const gi_denoise_var_io d{static_cast<const double*>(drgb.p), static_cast<const double*>(dvar.p), static_cast<const double*>(dt.p),
                                  static_cast<const double*>(dn.p), static_cast<const double*>(da.p), static_cast<double*>(dout.p),
                                  static_cast<double*>(dovar.p), static_cast<uint8_t*>(dout8.p)};
        e = launch_denoise_var(make_cam(*cam, frame->w), dnv_io(*frame, d), *p, dscr.p, nullptr);
        if (e != hipSuccess) return hip_fail(e, "gi_denoise_var launch");
        if (io->out_rgb) e = hipMemcpy(io->out_rgb, dout.p, b3, hipMemcpyDeviceToHost);   // (synchronous copies on the launch's stream)
        if (e == hipSuccess && io->out_var) e = hipMemcpy(io->out_var, dovar.p, b3, hipMemcpyDeviceToHost);
        if (e == hipSuccess && io->out_rgb8) e = hipMemcpy(io->out_rgb8, dout8.p, m * 3, hipMemcpyDeviceToHost);
        return e == hipSuccess ? GI_OK : hip_fail(e, "gi_denoise_var");
    });
}

// ---- temporal accumulation (gi.h "temporal accumulation"; gi_temporal.hip k_temporal) ----
// No scene, no state, no scratch: the caller's planes on the current device.
namespace {
// everything of a temporal call; *empty: the window holds no pixel
int check_temporal(const gi_camera* cam, const gi_camera* prev_cam, const gi_aov_frame* frame, const gi_temporal_params* p,
                   const gi_temporal_frame* cur, const gi_temporal_frame* hist, const gi_temporal_out* out, bool* empty) {
    if (!p || !cur || !out) return fail(GI_ERR_ARG, "gi_temporal: null parameters, current frame or outputs");
    int rc = check_aov_frame(cam, frame, empty);
    if (rc) return rc;
    if (hist) {
        if (!prev_cam) return fail(GI_ERR_ARG, "gi_temporal: a history needs the previous camera");
        bool e2 = false;
        if ((rc = check_aov_frame(prev_cam, frame, &e2))) return rc;
    }
    if (p->max_history < 1) return fail(GI_ERR_ARG, "gi_temporal: max_history must be >= 1");
    if (p->flags & ~GI_TEMPORAL_PRIM_STOP) return fail(GI_ERR_ARG, "gi_temporal: unknown flag");
    if (!(p->alpha_min >= 0 && p->alpha_min <= 1)) return fail(GI_ERR_ARG, "gi_temporal: alpha_min outside [0, 1]");
    if (!(p->cos_min >= -1 && p->cos_min <= 1)) return fail(GI_ERR_ARG, "gi_temporal: cos_min outside [-1, 1]");
    if (!(p->sigma_p > 0)) return fail(GI_ERR_ARG, "gi_temporal: sigma_p must be > 0 (+inf: no plane stop)");
    const bool stop = (p->flags & GI_TEMPORAL_PRIM_STOP) != 0;
    if (!cur->rgb || !cur->t || !cur->normal) return fail(GI_ERR_ARG, "gi_temporal: null rgb, t or normal of the current frame");
    if (hist && (!hist->rgb || !hist->t || !hist->normal || !hist->len)) return fail(GI_ERR_ARG, "gi_temporal: null rgb, t, normal or len of the history");
    if (stop && (!cur->prim || (hist && !hist->prim))) return fail(GI_ERR_ARG, "gi_temporal: the prim stop needs the prim planes");
    if (out->var && (!cur->var || (hist && !hist->var))) return fail(GI_ERR_ARG, "gi_temporal: out.var needs the var planes");
    if (!out->rgb && !out->var && !out->len) return fail(GI_ERR_ARG, "gi_temporal: every output is null");
    // the taps gather: no output may be an input
    const void* outs[3] = {out->rgb, out->var, out->len};
    const void* ins[11] = {cur->rgb, cur->var, cur->t, cur->normal, cur->prim,   // (cur.len is ignored)
                           hist ? hist->rgb : nullptr, hist ? hist->var : nullptr, hist ? hist->t : nullptr,
                           hist ? hist->normal : nullptr, hist ? hist->prim : nullptr, hist ? hist->len : nullptr};
    for (const void* o : outs) {
        if (!o) continue;
        for (const void* q : ins)
            if (o == q) return fail(GI_ERR_ARG, "gi_temporal: an output must not be an input plane");
    }
    return GI_OK;
}
TpIO tp_io(const gi_aov_frame& f, const gi_temporal_frame& cur, const gi_temporal_frame* hist, const gi_temporal_out& out) {
    return TpIO{f.x0, f.y0, f.x1 - f.x0, f.y1 - f.y0, cur, hist ? *hist : gi_temporal_frame{}, out};
}
}  // namespace

int gi_temporal_device(const gi_camera* cam, const gi_camera* prev_cam, const gi_aov_frame* frame, const gi_temporal_params* p,
                       const gi_temporal_frame* d_cur, const gi_temporal_frame* d_hist, const gi_temporal_out* d_out, void* stream) {
    return guard([&]() -> int {
        bool empty = false;
        const int rc = check_temporal(cam, prev_cam, frame, p, d_cur, d_hist, d_out, &empty);
        if (rc || empty) return rc;
        const CamDev c = make_cam(*cam, frame->w);
        const hipError_t e = launch_temporal(c, d_hist ? make_cam(*prev_cam, frame->w) : c, tp_io(*frame, *d_cur, d_hist, *d_out), *p,
                                             static_cast<hipStream_t>(stream));
        return e == hipSuccess ? GI_OK : hip_fail(e, "gi_temporal launch");
    });
}

int gi_temporal(const gi_camera* cam, const gi_camera* prev_cam, const gi_aov_frame* frame, const gi_temporal_params* p,
                const gi_temporal_frame* cur, const gi_temporal_frame* hist, const gi_temporal_out* out) {
    return guard([&]() -> int {
        bool empty = false;
        const int rc = check_temporal(cam, prev_cam, frame, p, cur, hist, out, &empty);
        if (rc || empty) return rc;
        const size_t m = (size_t)(frame->x1 - frame->x0) * (size_t)(frame->y1 - frame->y0), b1 = m * sizeof(double), b3 = 3 * b1,
                     bi = m * sizeof(int32_t);
        const bool stop = (p->flags & GI_TEMPORAL_PRIM_STOP) != 0, var = out->var != nullptr;
        // the planes the kernel reads, staged: {host plane, bytes, needed}
        struct Plane { const void* host; size_t bytes; bool on; DevBuf dev; };
        Plane in[11] = {{cur->rgb, b3, true, {}}, {cur->var, b3, var, {}}, {cur->t, b1, true, {}}, {cur->normal, b3, true, {}},
                        {cur->prim, bi, stop, {}},
                        {hist ? hist->rgb : nullptr, b3, hist != nullptr, {}}, {hist ? hist->var : nullptr, b3, hist && var, {}},
                        {hist ? hist->t : nullptr, b1, hist != nullptr, {}}, {hist ? hist->normal : nullptr, b3, hist != nullptr, {}},
                        {hist ? hist->prim : nullptr, bi, hist && stop, {}}, {hist ? hist->len : nullptr, bi, hist != nullptr, {}}};
        DevBuf orgb, ovar, olen;
        hipError_t e = hipSuccess;
        for (Plane& q : in)
            if (e == hipSuccess && q.on) e = q.dev.alloc(q.bytes);
        if (e == hipSuccess && out->rgb) e = orgb.alloc(b3);
        if (e == hipSuccess && out->var) e = ovar.alloc(b3);
        if (e == hipSuccess && out->len) e = olen.alloc(bi);
        if (e != hipSuccess) return hip_fail(e, "hipMalloc (temporal staging)");
        for (Plane& q : in)
            if (e == hipSuccess && q.on) e = hipMemcpy(q.dev.p, q.host, q.bytes, hipMemcpyHostToDevice);
        if (e != hipSuccess) return hip_fail(e, "gi_temporal");
        auto dp = [&](int k) { return static_cast<const double*>(in[k].dev.p); };
        auto ip = [&](int k) { return static_cast<const int32_t*>(in[k].dev.p); };
        const gi_temporal_frame dcur{dp(0), dp(1), dp(2), dp(3), ip(4), nullptr};
        const gi_temporal_frame dhist{dp(5), dp(6), dp(7), dp(8), ip(9), ip(10)};
        const gi_temporal_out dout{static_cast<double*>(orgb.p), static_cast<double*>(ovar.p), static_cast<int32_t*>(olen.p)};
        const CamDev c = make_cam(*cam, frame->w);
        e = launch_temporal(c, hist ? make_cam(*prev_cam, frame->w) : c, tp_io(*frame, dcur, hist ? &dhist : nullptr, dout), *p, nullptr);
        if (e != hipSuccess) return hip_fail(e, "gi_temporal launch");
        if (out->rgb) e = hipMemcpy(out->rgb, orgb.p, b3, hipMemcpyDeviceToHost);   // (synchronous copies on the launch's stream)
        if (e == hipSuccess && out->var) e = hipMemcpy(out->var, ovar.p, b3, hipMemcpyDeviceToHost);
        if (e == hipSuccess && out->len) e = hipMemcpy(out->len, olen.p, bi, hipMemcpyDeviceToHost);
        return e == hipSuccess ? GI_OK : hip_fail(e, "gi_temporal");
    });
}

int gi_kat_expbox(int n, const double* recs, int32_t* out) {
    return guard([&]() -> int {
        if (n < 0 || (n > 0 && (!recs || !out))) return fail(GI_ERR_ARG, "bad arguments");
        if (n == 0) return GI_OK;
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(GI_ERR_DEVICE, "no HIP device");
        double* d_r = nullptr;
        int32_t* d_o = nullptr;
        hipError_t e;
        if ((e = hipMalloc((void**)&d_r, (size_t)n * 12 * sizeof(double))) != hipSuccess) return hip_fail(e, "hipMalloc");
        if ((e = hipMalloc((void**)&d_o, (size_t)n * sizeof(int32_t))) != hipSuccess) { (void)hipFree(d_r); return hip_fail(e, "hipMalloc"); }
        e = hipMemcpy(d_r, recs, (size_t)n * 12 * sizeof(double), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = launch_box_kat(n, d_r, d_o, nullptr);
        if (e == hipSuccess) e = hipMemcpy(out, d_o, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost);
        (void)hipFree(d_r);
        (void)hipFree(d_o);
        return e == hipSuccess ? GI_OK : hip_fail(e, "gi_kat_expbox");
    });
}

int gi_kat_r_prims(int kind, int n, const double* recs, int32_t* hit, double* pn) {
    return guard([&]() -> int {
        if (kind < GI_KAT_R_TRI || kind > GI_KAT_R_BOX4) return fail(GI_ERR_ARG, "bad kind");
        const bool with_pn = kind == GI_KAT_R_TRI || kind == GI_KAT_R_SPHERE;
        if (n < 0 || (n > 0 && (!recs || !hit || (with_pn && !pn)))) return fail(GI_ERR_ARG, "bad arguments");
        if (n == 0) return GI_OK;
        int ndev = 0;
        if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(GI_ERR_DEVICE, "no HIP device");
        const size_t width = kind == GI_KAT_R_TRI ? 15 : kind == GI_KAT_R_SPHERE ? 10 : 12;
        const size_t rb = (size_t)n * width * sizeof(double), hb = (size_t)n * sizeof(int32_t), pb = (size_t)n * 6 * sizeof(double);
        std::vector<TriRec> tris;
        if (kind == GI_KAT_R_TRI) {   // the builder's records (gi_build.cpp builds an ImpTriangle's with make_tri too)
            tris.resize((size_t)n);
            for (int i = 0; i < n; ++i) {
                const double* q = recs + 15 * (size_t)i;
                make_tri(v3(q[0], q[1], q[2]), v3(q[3], q[4], q[5]), v3(q[6], q[7], q[8]), tris[(size_t)i]);
            }
        }
        DevBuf d_r, d_t, d_h, d_p;
        hipError_t e = d_r.alloc(rb);
        if (e == hipSuccess) e = d_h.alloc(hb);
        if (e == hipSuccess && with_pn) e = d_p.alloc(pb);
        if (e == hipSuccess && !tris.empty()) e = d_t.alloc(tris.size() * sizeof(TriRec));
        if (e != hipSuccess) return hip_fail(e, "hipMalloc (gi_kat_r_prims)");
        e = hipMemcpy(d_r.p, recs, rb, hipMemcpyHostToDevice);
        if (e == hipSuccess && !tris.empty()) e = hipMemcpy(d_t.p, tris.data(), tris.size() * sizeof(TriRec), hipMemcpyHostToDevice);
        if (e == hipSuccess)
            e = launch_r_prims_kat(kind, n, static_cast<const double*>(d_r.p), static_cast<const TriRec*>(d_t.p),
                                   static_cast<int32_t*>(d_h.p), static_cast<double*>(d_p.p), nullptr);
        if (e == hipSuccess) e = hipMemcpy(hit, d_h.p, hb, hipMemcpyDeviceToHost);
        if (e == hipSuccess && with_pn) e = hipMemcpy(pn, d_p.p, pb, hipMemcpyDeviceToHost);
        return e == hipSuccess ? GI_OK : hip_fail(e, "gi_kat_r_prims");
    });
}

int gi_kat_r_entities(gi_scene* s, int n, const double* rays, int32_t* hit, double* pn) {
    return guard([&]() -> int {
        DeviceRestore keep;   // the caller's current device, restored on return
        if (!s || n < 0 || (n > 0 && (!rays || !hit || !pn))) return fail(GI_ERR_ARG, "bad arguments");
        const size_t pairs = (size_t)n * (size_t)s->dev.n_ents;
        if (pairs == 0) return GI_OK;
        if (pairs > (size_t)1 << 28) return fail(GI_ERR_ARG, "gi_kat_r_entities: more than 2^28 (ray, entity) pairs");
        std::lock_guard<std::mutex> lk(s->mu);
        int rc = bind_device(s->device);
        if (rc) return rc;
        const size_t rb = (size_t)n * 6 * sizeof(double), hb = pairs * sizeof(int32_t), pb = pairs * 6 * sizeof(double);
        DevBuf d_r, d_h, d_p;
        hipError_t e = d_r.alloc(rb);
        if (e == hipSuccess) e = d_h.alloc(hb);
        if (e == hipSuccess) e = d_p.alloc(pb);
        if (e != hipSuccess) return hip_fail(e, "hipMalloc (gi_kat_r_entities)");
        e = hipMemcpy(d_r.p, rays, rb, hipMemcpyHostToDevice);
        if (e == hipSuccess)
            e = launch_r_entities_kat(s->dev, n, static_cast<const double*>(d_r.p), static_cast<int32_t*>(d_h.p),
                                      static_cast<double*>(d_p.p), nullptr);
        if (e == hipSuccess) e = hipMemcpy(hit, d_h.p, hb, hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(pn, d_p.p, pb, hipMemcpyDeviceToHost);
        return e == hipSuccess ? GI_OK : hip_fail(e, "gi_kat_r_entities");
    });
}

int gi_kat_x_query(gi_scene* s, int n, const double* recs, const double cam_pos[3], int flags, int32_t* prim1, double* t1,
                   int32_t* occl, int32_t* skip_s, int32_t* prim2, double* t2, int32_t* skip2, double* skip_cos) {
    return guard([&]() -> int {
        DeviceRestore keep;   // the caller's current device, restored on return
        if (!s || !cam_pos || n < 0 || (flags & ~3) != 0) return fail(GI_ERR_ARG, "bad arguments");
        if (n > 0 && (!recs || !prim1 || !t1 || !occl || !skip_s || !prim2 || !t2 || !skip2)) return fail(GI_ERR_ARG, "null argument");
        if (n == 0) return GI_OK;
        std::lock_guard<std::mutex> lk(s->mu);
        int rc = bind_device(s->device);
        if (rc) return rc;
        double *d_r = nullptr, *d_d = nullptr;
        int32_t* d_i = nullptr;
        std::vector<int32_t> hi((size_t)n * 5);
        std::vector<double> hd((size_t)n * 2 + 1);
        hipError_t e;
        if ((e = hipMalloc((void**)&d_r, (size_t)n * 12 * sizeof(double))) == hipSuccess &&
            (e = hipMalloc((void**)&d_i, hi.size() * sizeof(int32_t))) == hipSuccess)
            e = hipMalloc((void**)&d_d, hd.size() * sizeof(double));
        if (e == hipSuccess) e = hipMemcpy(d_r, recs, (size_t)n * 12 * sizeof(double), hipMemcpyHostToDevice);
        if (e == hipSuccess)
            e = launch_x_query_kat(s->dev, x_query_cfg(s->xcfg, flags, WK_SEG), v3(cam_pos[0], cam_pos[1], cam_pos[2]), n, d_r, d_i, d_d, nullptr);
        if (e == hipSuccess) e = hipMemcpy(hi.data(), d_i, hi.size() * sizeof(int32_t), hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(hd.data(), d_d, hd.size() * sizeof(double), hipMemcpyDeviceToHost);
        (void)hipFree(d_r);
        (void)hipFree(d_i);
        (void)hipFree(d_d);
        if (e != hipSuccess) return hip_fail(e, "gi_kat_x_query");
        for (size_t i = 0; i < (size_t)n; ++i) {
            prim1[i] = hi[5 * i];
            occl[i] = hi[5 * i + 1];
            skip_s[i] = hi[5 * i + 2];
            prim2[i] = hi[5 * i + 3];
            skip2[i] = hi[5 * i + 4];
            t1[i] = hd[2 * i];
            t2[i] = hd[2 * i + 1];
        }
        if (skip_cos) *skip_cos = hd[2 * (size_t)n];
        return GI_OK;
    });
}

int gi_kat_x_variant(gi_scene* s, int flags, int32_t out[6]) {
    return guard([&]() -> int {
        if (!s || !out || (flags & ~3) != 0) return fail(GI_ERR_ARG, "bad arguments");
        std::lock_guard<std::mutex> lk(s->mu);
        wf_variant(s->dev, x_query_cfg(s->xcfg, flags, WK_SEG), out);   // with flags 0, k_seg's for this scene
        return GI_OK;
    });
}

int gi_kat_x_texel(gi_scene* s, int n, const double* recs, int mode, double* texel, int32_t* how) {
    return guard([&]() -> int {
        DeviceRestore keep;   // the caller's current device, restored on return
        if (!s || n < 0 || (mode != 0 && mode != 1)) return fail(GI_ERR_ARG, "bad arguments");
        if (n > 0 && (!recs || !texel || !how)) return fail(GI_ERR_ARG, "null argument");
        if (n == 0) return GI_OK;
        std::lock_guard<std::mutex> lk(s->mu);
        for (size_t i = 0; i < (size_t)n; ++i) {   // (the kernel indexes the entity array with it)
            const double ent = recs[4 * i];
            if (!(ent >= 0.0 && ent < (double)s->dev.n_ents && ent == (double)(int32_t)ent))
                return fail(GI_ERR_ARG, "entity index out of range");
        }
        int rc = bind_device(s->device);
        if (rc) return rc;
        double *d_r = nullptr, *d_d = nullptr;
        int32_t* d_i = nullptr;
        hipError_t e;
        if ((e = hipMalloc((void**)&d_r, (size_t)n * 4 * sizeof(double))) == hipSuccess &&
            (e = hipMalloc((void**)&d_i, (size_t)n * sizeof(int32_t))) == hipSuccess)
            e = hipMalloc((void**)&d_d, (size_t)n * 3 * sizeof(double));
        if (e == hipSuccess) e = hipMemcpy(d_r, recs, (size_t)n * 4 * sizeof(double), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = launch_x_texel_kat(s->dev, s->xcfg.var, n, mode, d_r, d_i, d_d, nullptr);
        if (e == hipSuccess) e = hipMemcpy(how, d_i, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost);
        if (e == hipSuccess) e = hipMemcpy(texel, d_d, (size_t)n * 3 * sizeof(double), hipMemcpyDeviceToHost);
        (void)hipFree(d_r);
        (void)hipFree(d_i);
        (void)hipFree(d_d);
        return e == hipSuccess ? GI_OK : hip_fail(e, "gi_kat_x_texel");
    });
}

int gi_octree_create(const gi_scene_desc* desc, gi_octree** out) {
    return guard([&]() -> int {
        if (!desc || !out || desc->n_entities < 0 || (desc->n_entities > 0 && !desc->entities))
            return fail(GI_ERR_ARG, "bad scene descriptor");
        *out = nullptr;
        std::unique_ptr<gi_octree> t(new gi_octree());
        std::string err;
        if (!build_host_scene(*desc, t->host, err)) return fail(GI_ERR_SCENE, err);
        *out = t.release();
        return GI_OK;
    });
}

void gi_octree_destroy(gi_octree* t) { delete t; }

int gi_octree_intersect(const gi_octree* t, const double origin[3], const double dir[3], int32_t* out, int64_t cap,
                        int64_t* n) {
    return guard([&]() -> int {
        if (!t || !origin || !dir || !n || cap < 0 || (cap > 0 && !out)) return fail(GI_ERR_ARG, "bad arguments");
        std::vector<int32_t> list;
        if (!t->host.rnodes.empty())
            octree_query(t->host, 0, v3(origin[0], origin[1], origin[2]), v3(dir[0], dir[1], dir[2]), list);
        *n = (int64_t)list.size();
        const int64_t k = std::min<int64_t>(cap, (int64_t)list.size());
        if (k > 0) std::memcpy(out, list.data(), (size_t)k * sizeof(int32_t));
        return GI_OK;
    });
}

}  // extern "C"
