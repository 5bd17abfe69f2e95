// gi_adapt.hip — adaptive sampling between the passes of a Mode X frame (gi.h "adaptive sampling";
// gi_render_adaptive*): the kernels that run around the render kernels of a pass.  The render kernels themselves are
// the renders' own: a pass hands them the list of the pixels still active, its device count and a rows buffer of
// the pass's k samples (gi_kernels.hip launch_adaptive).
//
//   k_x_adapt_init   first pass: the per-slot state.  n = 0, S1 = S2 = +0 for the pixels the classify pass listed
//                    (the same frustum test decides it); the resolved pixels and the padding slots are marked.
//   k_x_adapt_fill   every pass, one lane per slot: the planes of the pixels that were NOT active in the pass -- the
//                    stopped ones from their final state, the resolved ones as +0 with their own n.
//   k_x_adapt_fold   every pass, one lane per active entry: folds the entry's k rows into S1 and S2 in sample order,
//                    sets n = e, judges the pixel, writes its planes and appends a survivor to the other list.
// k_x_adapt_fill and k_x_adapt_fold write disjoint pixels (a slot is active iff it is neither marked nor stopped)
// and together every pixel of the frame; fill runs first, because fold is what stops pixels.
//
// The state is per pixel slot (S1[3], S2[3], n: 56 B), the rows per active index, so no result depends on the
// order of a list.  The survivors keep their order inside a workgroup's 256 entries (wave ballots, the waves'
// counts combined in LDS, one atomic per workgroup as in k_x_classify); the workgroups' runs land in the order of
// their atomics, so the list is in tile order only run by run (DESIGN.md §5 "adaptive sampling").
//
// Build: -ffp-contract=off as every unit; the rule in gi.h is stated operation by operation and
// tests/adaptive_ref.py restates it in numpy.
#include <hip/hip_runtime.h>

#include "gi.h"
#include "gi_dev.h"
#include "gi_launch.h"
#include "gi_scene.h"

namespace gi {

namespace {

// XScratch::ad_n: the samples the slot's pixel has received, and
enum : int32_t {
    AD_STOP = (int32_t)0x80000000,   // the pixel has stopped: S1, S2 and n are final
    AD_RES = 0x40000000,             // the classify pass resolved it without traversal (every x is +0; never listed)
    AD_PAD = 0x20000000,             // no pixel in this slot (a tile that overhangs the frame)
    AD_N = 0x1FFFFFFF,
};

struct XAdapt {
    const unsigned* list;      // this pass's active slots and their count
    const unsigned* n_list;
    unsigned* next;            // the survivors' list and its count (zeroed before the pass)
    unsigned* n_next;
    const double* rows;        // this pass's rows [active index][k][3]
    double* sum;               // per slot S1[3], S2[3]
    int32_t* n;                // per slot n and the AD_ flags
    int k, e, spp, min_samples;
    unsigned flags;
    double tol, y_floor;
    gi_adaptive_out out;
};

// The pixel's outputs from its state, and the decision: true when the pixel stops after the pass ending at a.e
// (gi.h: the rule, exactly).
__device__ __forceinline__ bool adapt_judge(const XAdapt& a, long long idx, double s1a, double s1b, double s1c, double s2a,
                                            double s2b, double s2c, int n) {
    const double dn = (double)n, dn1 = (double)(n - 1);
    const double ma = s1a / dn, mb = s1b / dn, mc = s1c / dn;
    double va = ((s2a - s1a * ma) / dn1) / dn, vb = ((s2b - s1b * mb) / dn1) / dn, vc = ((s2c - s1c * mc) / dn1) / dn;
    va = va > 0 ? va : va != va ? va : 0;   // (a NaN stays: it must not stop the pixel)
    vb = vb > 0 ? vb : vb != vb ? vb : 0;
    vc = vc > 0 ? vc : vc != vc ? vc : 0;
    if (a.out.mean) { a.out.mean[3 * idx] = ma; a.out.mean[3 * idx + 1] = mb; a.out.mean[3 * idx + 2] = mc; }
    if (a.out.var) { a.out.var[3 * idx] = va; a.out.var[3 * idx + 1] = vb; a.out.var[3 * idx + 2] = vc; }
    const double c0 = smin(ma, 1.0), c1 = smin(mb, 1.0), c2 = smin(mc, 1.0);
    if (a.out.rgb) { a.out.rgb[3 * idx] = c0; a.out.rgb[3 * idx + 1] = c1; a.out.rgb[3 * idx + 2] = c2; }
    if (a.out.rgb8) quantize(c0, c1, c2, a.out.rgb8 + 3 * idx);
    if (a.out.n) a.out.n[idx] = n;
    bool stop = a.e == a.spp;
    if (n >= a.min_samples) {
        const double err = (va + vb) + vc;
        double thr = a.tol * a.tol;
        if (a.flags & GI_ADAPTIVE_RELATIVE) {
            const double y = (ma + mb) + mc;
            const double f = y > a.y_floor ? y : a.y_floor;
            thr = thr * (f * f);
        }
        stop = stop || err <= thr;   // (a NaN compares false)
    }
    return stop;
}

__global__ __launch_bounds__(256) void k_x_adapt_init(DevScene sc, CamDev cam, TileMap m, double* sum, int32_t* n) {
    const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= m.n_local * (kTile * kTile)) return;
    long long idx = -1;
    int x = 0, y = 0;
    int32_t st = AD_PAD;
    if (slot_pixel(m, s >> 6, (int)(s & 63), idx, x, y)) st = pixel_misses_box(cam, x, y, sc.root_lo, sc.root_hi) ? AD_RES : 0;
    n[s] = st;
    if (st == 0) {
        double2* q = reinterpret_cast<double2*>(sum + 6 * s);   // (48-byte records: 16-byte aligned)
        q[0] = make_double2(0.0, 0.0);
        q[1] = make_double2(0.0, 0.0);
        q[2] = make_double2(0.0, 0.0);
    }
}

__global__ __launch_bounds__(256) void k_x_adapt_fill(TileMap m, XAdapt a) {
    const long long s = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= m.n_local * (kTile * kTile)) return;
    const int32_t st = a.n[s];
    if ((st & AD_PAD) || !(st & (AD_STOP | AD_RES))) return;   // no pixel, or active in this pass: k_x_adapt_fold's
    long long idx = -1;
    int x = 0, y = 0;
    slot_pixel(m, s >> 6, (int)(s & 63), idx, x, y);
    if (st & AD_RES) {
        // a resolved pixel takes part in every pass (x = +0) until it is judged: err = 0 <= thr always
        int n = st & AD_N;
        if (!(st & AD_STOP)) {
            n = a.e;
            a.n[s] = n | AD_RES | ((n >= a.min_samples || n == a.spp) ? AD_STOP : 0);
        }
        if (a.out.mean) { a.out.mean[3 * idx] = 0; a.out.mean[3 * idx + 1] = 0; a.out.mean[3 * idx + 2] = 0; }
        if (a.out.var) { a.out.var[3 * idx] = 0; a.out.var[3 * idx + 1] = 0; a.out.var[3 * idx + 2] = 0; }
        if (a.out.rgb) { a.out.rgb[3 * idx] = 0; a.out.rgb[3 * idx + 1] = 0; a.out.rgb[3 * idx + 2] = 0; }
        if (a.out.rgb8) { a.out.rgb8[3 * idx] = 0; a.out.rgb8[3 * idx + 1] = 0; a.out.rgb8[3 * idx + 2] = 0; }
        if (a.out.n) a.out.n[idx] = n;
        return;
    }
    const double2* q = reinterpret_cast<const double2*>(a.sum + 6 * s);
    const double2 v0 = q[0], v1 = q[1], v2 = q[2];
    (void)adapt_judge(a, idx, v0.x, v0.y, v1.x, v1.y, v2.x, v2.y, st & AD_N);
}

__global__ __launch_bounds__(256) void k_x_adapt_fold(TileMap m, XAdapt a) {
    const unsigned i = blockIdx.x * blockDim.x + threadIdx.x;
    const unsigned n_list = *a.n_list;
    if (blockIdx.x * blockDim.x >= n_list) return;   // (the whole workgroup: the barriers below are uniform)
    bool keep = false;
    unsigned ps = 0;
    if (i < n_list) {
        ps = a.list[i];
        long long idx = -1;
        int x = 0, y = 0;
        slot_pixel(m, (long long)(ps >> 6), (int)(ps & 63), idx, x, y);
        double2* st = reinterpret_cast<double2*>(a.sum + 6 * (size_t)ps);
        const double2 t0 = st[0], t1 = st[1], t2 = st[2];
        double s1a = t0.x, s1b = t0.y, s1c = t1.x, s2a = t1.y, s2b = t2.x, s2c = t2.y;
        const double* p = a.rows + 3 * (size_t)i * (size_t)a.k;
        int s = 0;
        if ((a.k & 1) == 0) {
            // even k: the entry's rows are 16-byte aligned and two samples come in three 16-byte loads, as in
            // k_x_reduce; the sums take the samples in the same order
            const double2* q = reinterpret_cast<const double2*>(p);
            for (; s + 1 < a.k; s += 2) {
                const double2 v0 = q[3 * (s >> 1)], v1 = q[3 * (s >> 1) + 1], v2 = q[3 * (s >> 1) + 2];
                s1a = s1a + v0.x; s2a = s2a + v0.x * v0.x;
                s1b = s1b + v0.y; s2b = s2b + v0.y * v0.y;
                s1c = s1c + v1.x; s2c = s2c + v1.x * v1.x;
                s1a = s1a + v1.y; s2a = s2a + v1.y * v1.y;
                s1b = s1b + v2.x; s2b = s2b + v2.x * v2.x;
                s1c = s1c + v2.y; s2c = s2c + v2.y * v2.y;
            }
        }
        for (; s < a.k; ++s) {
            const double x0 = p[3 * s], x1 = p[3 * s + 1], x2 = p[3 * s + 2];
            s1a = s1a + x0; s2a = s2a + x0 * x0;
            s1b = s1b + x1; s2b = s2b + x1 * x1;
            s1c = s1c + x2; s2c = s2c + x2 * x2;
        }
        st[0] = make_double2(s1a, s1b);
        st[1] = make_double2(s1c, s2a);
        st[2] = make_double2(s2b, s2c);
        keep = !adapt_judge(a, idx, s1a, s1b, s1c, s2a, s2b, s2c, a.e);
        a.n[ps] = a.e | (keep ? 0 : AD_STOP);
    }
    // the survivors, in the workgroup's order: exclusive offsets of the waves, then one atomic for the workgroup
    const unsigned long long mk = __ballot(keep);
    __shared__ unsigned s_cnt[256 / 64 + 1];
    const int wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) s_cnt[wv] = (unsigned)__popcll(mk);
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned acc = 0;
        for (int q = 0; q < 256 / 64; ++q) {
            const unsigned c = s_cnt[q];
            s_cnt[q] = acc;
            acc += c;
        }
        s_cnt[256 / 64] = acc ? atomicAdd(a.n_next, acc) : 0u;
    }
    __syncthreads();
    if (keep) a.next[s_cnt[256 / 64] + s_cnt[wv] + (unsigned)__popcll(mk & ((1ull << lane) - 1))] = ps;
}

}  // namespace

hipError_t launch_adapt_init(const DevScene& sc, const CamDev& cam, int w, int h, const XScratch& xs, hipStream_t stream) {
    const TileMap m = make_map(w, h, 1, 0);
    const long long n_slots = m.n_local * (kTile * kTile);
    if (!xs.ad_sum || !xs.ad_n || xs.ad_cap < n_slots) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_x_adapt_init, dim3((unsigned)((n_slots + 255) / 256)), dim3(256), 0, stream, sc, cam, m, xs.ad_sum, xs.ad_n);
    return hipGetLastError();
}

hipError_t launch_adapt_fold(int w, int h, int s0, int e, const XAdaptPass& ap, const XScratch& xs, hipStream_t stream) {
    const TileMap m = make_map(w, h, 1, 0);
    const long long n_slots = m.n_local * (kTile * kTile);
    const int k = e - s0;
    if (!xs.list || !xs.part || !xs.ad_list || !xs.ad_cnt || !xs.ad_sum || !xs.ad_n || xs.cap < n_slots || xs.ad_cap < n_slots ||
        k < 2 || xs.spp < k || (ap.cur & ~1))
        return hipErrorInvalidValue;
    XAdapt a;
    a.list = ap.cur ? xs.ad_list : xs.list;
    a.n_list = xs.ad_cnt + ap.cur;
    a.next = ap.cur ? xs.list : xs.ad_list;
    a.n_next = xs.ad_cnt + (ap.cur ^ 1);
    a.rows = xs.part;
    a.sum = xs.ad_sum;
    a.n = xs.ad_n;
    a.k = k;
    a.e = e;
    a.spp = ap.spp_max;
    a.min_samples = ap.p.min_samples;
    a.flags = ap.p.flags;
    a.tol = ap.p.tol;
    a.y_floor = ap.p.y_floor;
    a.out = ap.out;
    // one lane per slot of the frame: the active count is on the device, the workgroups past it return at once
    const dim3 grid((unsigned)((n_slots + 255) / 256));
    hipLaunchKernelGGL(k_x_adapt_fill, grid, dim3(256), 0, stream, m, a);
    hipLaunchKernelGGL(k_x_adapt_fold, grid, dim3(256), 0, stream, m, a);
    return hipGetLastError();
}

}  // namespace gi
