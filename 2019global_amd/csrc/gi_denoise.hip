// gi_denoise.hip — the device denoiser (gi.h "denoiser"; DESIGN.md §5 "Denoiser"): an edge-avoiding
// a-trous filter of a frame over its first-hit feature buffers, for the first passes of a progressive
// Mode X frame.  A memory-bound 2-D stencil: no scene, no traversal; everything is fp64 and every sum is
// sequential in the order gi.h gives, so a numpy restatement (tests/denoise_ref.py) is exact bit for bit.
//   k_dn_prep    one 64-byte guide record per pixel in the caller's scratch (hit position, normal, the
//                plane stop's scale, validity), and the albedo as a 32-byte record where the albedo stop is on
//   k_dn_level   one a-trous level per launch, the direct-gather form: 25 taps straight from global memory
//                through the caches; the colour ping-pongs between two scratch planes, the last level writes
//                the outputs
//   k_dn_level_lds  the same level for steps 1 and 2 with the tile and its halo staged in LDS once: it won the
//                A/B against the direct form there (DESIGN.md §9 "Denoiser"; profiles/denoise_ab.txt)
//   k_dnv_g, k_dnv_level  the variance-guided filter (gi.h "variance-guided denoiser"): per level the 3 x 3 prefilter
//                of the variance plane, then k_dn_level's direct-gather level with the colour stop per pixel and
//                the variance carried along
// Lane mapping of all of them: workgroup tiles of 64 x 4 window pixels, a wave per tile row, lanes along x -- every
// tap of a wave is one contiguous run of records, and the four rows of a tile share their vertical taps; the direct
// levels' tiles are dealt to the XCDs in bands (dn_tile_of).
// 64-bit indices.  Resources and rates: DESIGN.md §9 "Denoiser".
#include <hip/hip_runtime.h>

#include "gi_dev.h"
#include "gi_launch.h"

// GI_DN_LDS_STEPS: how many of the first levels run the LDS-staged form (0: every level gathers from global
// memory; A/B builds: build.py --variant NAME GI_DN_LDS_STEPS=0|1|2)
#ifndef GI_DN_LDS_STEPS
#define GI_DN_LDS_STEPS 2
#endif
// GI_DN_XCD: 1 deals the direct-gather levels' tiles to the device's 8 XCDs in bands (dn_tile_of; 0: workgroup order)
#ifndef GI_DN_XCD
#define GI_DN_XCD 1
#endif

namespace gi {
namespace {

constexpr int kDnTileW = 64, kDnTileH = 4;
constexpr long long kDnMaxGrid = 1ll << 20;   // workgroups per launch; more tiles: a grid-stride loop

struct DnGuide {           // 64 bytes, 16-byte aligned in the scratch
    double P[3];           // cam.pos + t d
    double n[3];
    double sp;             // sigma_p * t
    double valid;          // 1: t < +inf; 0: the pixel passes through and is no tap
};
static_assert(sizeof(DnGuide) == 64, "DnGuide layout");
struct DnAlbedo {          // 32 bytes: the three doubles themselves (compared with ==), padded
    double a[3];
    double pad;
};
static_assert(sizeof(DnAlbedo) == 32, "DnAlbedo layout");

struct DnTiles {
    int tiles_x;
    long long n_tiles;
};
__host__ __device__ inline DnTiles dn_tiles(int cols, int rows) {
    DnTiles t;
    t.tiles_x = (cols + kDnTileW - 1) / kDnTileW;
    t.n_tiles = (long long)t.tiles_x * (long long)((rows + kDnTileH - 1) / kDnTileH);
    return t;
}
// The tile of workgroup slot b of the direct-gather levels.  Workgroups go round-robin to the device's 8 XCDs, each
// with an L2 of its own: in workgroup order every XCD reads every row of the frame, and at steps of 4 and more the
// taps of a tile share nothing in L1.  Bands of kDnXcdRows tile rows are dealt to the XCDs in turn instead: within a
// span of 8 bands, slot 8 q + r takes tile q of band r, so an XCD's L2 holds the rows its taps share, while bands
// this narrow still spread a frame whose valid pixels are in one place over all XCDs.  The tiles behind the last
// whole span keep their order.  A bijection whatever the hardware does with the slots.
constexpr int kDnXcdRows = 16;
__device__ __forceinline__ long long dn_tile_of(long long b, const DnTiles& tl) {
#if GI_DN_XCD
    const long long band = (long long)kDnXcdRows * tl.tiles_x, span = 8 * band;
    if (tl.n_tiles < (1ll << 32)) {   // (32-bit divisions, uniform over the workgroup)
        const unsigned full = (unsigned)tl.n_tiles / (unsigned)span * (unsigned)span;
        if ((unsigned)b < full) {
            const unsigned base = (unsigned)b / (unsigned)span * (unsigned)span, o = (unsigned)b - base;
            return (long long)base + (long long)(o & 7) * band + (long long)(o >> 3);
        }
    }
#endif
    return b;
}
// window pixel of this thread in tile `tile`; false: no pixel there.  The division is uniform over the
// workgroup and in 32 bits where the tile index allows it (a 64-bit one is a long software routine)
__device__ __forceinline__ bool dn_pixel(const DnTiles& tl, long long tile, int cols, int rows, int& px, int& py) {
    long long ty;
    if (tile < (1ll << 32)) ty = (long long)((unsigned)tile / (unsigned)tl.tiles_x);
    else ty = tile / tl.tiles_x;
    const int tx = (int)(tile - ty * tl.tiles_x);
    px = tx * kDnTileW + (int)threadIdx.x;
    const long long y = ty * kDnTileH + (long long)threadIdx.y;
    py = (int)y;
    return px < cols && y < rows;
}

__device__ __forceinline__ DnGuide dn_load_guide(const DnGuide* g, long long i) {
    const double2* q = reinterpret_cast<const double2*>(g + i);
    const double2 a = q[0], b = q[1], c = q[2], d = q[3];
    DnGuide r;
    r.P[0] = a.x; r.P[1] = a.y; r.P[2] = b.x;
    r.n[0] = b.y; r.n[1] = c.x; r.n[2] = c.y;
    r.sp = d.x; r.valid = d.y;
    return r;
}

__global__ __launch_bounds__(kDnTileW * kDnTileH) void k_dn_prep(CamDev cam, int x0, int y0, int cols, int rows, double sigma_p,
                                                                  const double* t, const double* nrm, const double* alb,
                                                                  DnGuide* guide, DnAlbedo* albedo) {
    const DnTiles tl = dn_tiles(cols, rows);
    for (long long slot = blockIdx.x; slot < tl.n_tiles; slot += gridDim.x) {
        const long long tile = slot;
        int px = 0, py = 0;
        if (!dn_pixel(tl, tile, cols, rows, px, py)) continue;
        const long long i = (long long)py * (long long)cols + (long long)px;
        const double tp = t[i];
        const bool valid = tp < INFINITY;
        double2* q = reinterpret_cast<double2*>(guide + i);
        if (valid) {
            const V3 d = normalize(primary_dir(cam, (double)(x0 + px), (double)(y0 + py)));
            const V3 P = cam.pos + tp * d;
            const double* n = nrm + 3 * i;
            q[0] = make_double2(P.x, P.y);
            q[1] = make_double2(P.z, n[0]);
            q[2] = make_double2(n[1], n[2]);
            q[3] = make_double2(sigma_p * tp, 1.0);
        } else {
            q[0] = q[1] = q[2] = q[3] = make_double2(0.0, 0.0);
        }
        if (albedo) {
            const double* a = alb + 3 * i;
            double2* qa = reinterpret_cast<double2*>(albedo + i);
            qa[0] = make_double2(a[0], a[1]);
            qa[1] = make_double2(a[2], 0.0);
        }
    }
}

// H = {1/16, 1/4, 3/8, 1/4, 1/16}; every product of two is exact
__device__ __forceinline__ double dn_h(int k) { return k == 2 ? 0.375 : ((k == 1 || k == 3) ? 0.25 : 0.0625); }

// One tap that counts: its weight by gi.h's order of operations, added to the sums
struct DnAcc {
    double w, r, g, b;
};
__device__ __forceinline__ double dn_weight(double k, V3 np, V3 Pp, double sp, V3 cp, V3 nq, V3 Pq, V3 cq, int npow, double sigma2) {
    double wn = dot(np, nq);
    wn = wn > 0.0 ? wn : 0.0;
    for (int s = 0; s < npow; ++s) wn = wn * wn;
    const double dist = fabs(dot(np, Pq - Pp));
    double wp = 1.0 - dist / sp;
    wp = wp > 0.0 ? wp : 0.0;
    const V3 e = cp - cq;
    const double wc = 1.0 / (1.0 + dot(e, e) / sigma2);
    return ((k * wn) * wp) * wc;
}
__device__ __forceinline__ void dn_tap(DnAcc& a, double k, V3 np, V3 Pp, double sp, V3 cp, V3 nq, V3 Pq, V3 cq, int npow, double sigma2) {
    const double wt = dn_weight(k, np, Pp, sp, cp, nq, Pq, cq, npow, sigma2);
    a.w += wt;
    a.r += wt * cq.x;
    a.g += wt * cq.y;
    a.b += wt * cq.z;
}
// the last level's clamp and outputs / a level's colour
template <bool LAST>
__device__ __forceinline__ void dn_store(long long i, double r, double g, double b, double* cout, uint8_t* out8) {
    if (LAST) {
        r = r < 1.0 ? r : 1.0;
        g = g < 1.0 ? g : 1.0;
        b = b < 1.0 ? b : 1.0;
        if (out8) quantize(r, g, b, out8 + 3 * i);
    }
    if (cout) {
        cout[3 * i] = r;
        cout[3 * i + 1] = g;
        cout[3 * i + 2] = b;
    }
}

// One level: c_out = the filtered c_in at step `step` and colour variance sigma2; LAST: min(c, 1) into out /
// out8 (either may be null) instead of c_out.  STOP: the albedo stop.  Invalid pixels copy through.
template <bool STOP, bool LAST>
__global__ __launch_bounds__(kDnTileW * kDnTileH) void k_dn_level(int cols, int rows, int step, int npow, double sigma2,
                                                                   const DnGuide* __restrict__ guide,
                                                                   const DnAlbedo* __restrict__ albedo,
                                                                   const double* __restrict__ cin, double* __restrict__ cout,
                                                                   uint8_t* __restrict__ out8) {
    const DnTiles tl = dn_tiles(cols, rows);
    for (long long slot = blockIdx.x; slot < tl.n_tiles; slot += gridDim.x) {
        const long long tile = dn_tile_of(slot, tl);
        int px = 0, py = 0;
        if (!dn_pixel(tl, tile, cols, rows, px, py)) continue;
        const long long i = (long long)py * (long long)cols + (long long)px;
        const DnGuide gp = dn_load_guide(guide, i);
        const double cr = cin[3 * i], cg = cin[3 * i + 1], cb = cin[3 * i + 2];
        double r = cr, g = cg, b = cb;
        if (gp.valid != 0.0) {
            double ar = 0.0, ag = 0.0, ab = 0.0;
            if (STOP) {
                const double2* qa = reinterpret_cast<const double2*>(albedo + i);
                const double2 a0 = qa[0], a1 = qa[1];
                ar = a0.x; ag = a0.y; ab = a1.x;
            }
            const V3 np = v3(gp.n[0], gp.n[1], gp.n[2]);
            const V3 Pp = v3(gp.P[0], gp.P[1], gp.P[2]);
            DnAcc acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
                for (int dx = -2; dx <= 2; ++dx) {
                    // every tap's loads are issued whether it counts or not (coordinates clamped into the
                    // window), so that they do not wait on each other's tests
                    const long long qy = (long long)py + (long long)step * dy, qx = (long long)px + (long long)step * dx;
                    const bool in = qy >= 0 && qy < rows && qx >= 0 && qx < cols;
                    const long long j = in ? qy * (long long)cols + qx : i;
                    const DnGuide gq = dn_load_guide(guide, j);
                    bool use = in && gq.valid != 0.0;
                    if (STOP) {
                        const double2* qa = reinterpret_cast<const double2*>(albedo + j);
                        const double2 a0 = qa[0], a1 = qa[1];
                        use = use && a0.x == ar && a0.y == ag && a1.x == ab;
                    }
                    const double qr = cin[3 * j], qg = cin[3 * j + 1], qb = cin[3 * j + 2];
                    if (!use) continue;
                    dn_tap(acc, dn_h(dx + 2) * dn_h(dy + 2), np, Pp, gp.sp, v3(cr, cg, cb), v3(gq.n[0], gq.n[1], gq.n[2]),
                           v3(gq.P[0], gq.P[1], gq.P[2]), v3(qr, qg, qb), npow, sigma2);
                }
            }
            r = acc.r / acc.w;
            g = acc.g / acc.w;
            b = acc.b / acc.w;
        }
        dn_store<LAST>(i, r, g, b, cout, out8);
    }
}

#if GI_DN_LDS_STEPS
// The LDS-staged form of the first GI_DN_LDS_STEPS levels (steps 1 and 2): the tile and its halo of 2 STEP pixels
// are staged in LDS once (68 x 8 pixels at step 1, 72 x 12 at step 2) and the 25 taps come from there.  Per staged pixel 96 bytes (80 without the
// albedo stop) in 16-byte columns, lanes along x: P and n in three, the colour's r, g in one, and (colour b,
// albedo b or validity) and the albedo's r, g -- an invalid or outside pixel has albedo r = NaN (validity 0), so
// the albedo comparison itself skips it.  Same arithmetic, same order: dn_tap.
template <bool STOP, bool LAST, int STEP>
__global__ __launch_bounds__(kDnTileW * kDnTileH) void k_dn_level_lds(int cols, int rows, int npow, double sigma2,
                                                                       const DnGuide* __restrict__ guide,
                                                                       const DnAlbedo* __restrict__ albedo,
                                                                       const double* __restrict__ cin, double* __restrict__ cout,
                                                                       uint8_t* __restrict__ out8) {
    constexpr int HALO = 2 * STEP, W = kDnTileW + 2 * HALO, HT = kDnTileH + 2 * HALO, NPX = W * HT;
    __shared__ double2 s_g[3][NPX];
    __shared__ double2 s_c01[NPX];
    __shared__ double2 s_cbx[NPX];                 // (colour b, STOP ? albedo b : validity)
    __shared__ double2 s_a01[STOP ? NPX : 1];
    const DnTiles tl = dn_tiles(cols, rows);
    const int tid = (int)(threadIdx.y * kDnTileW + threadIdx.x);
    for (long long slot = blockIdx.x; slot < tl.n_tiles; slot += gridDim.x) {
        const long long tile = slot;
        int px = 0, py = 0;
        const bool has = dn_pixel(tl, tile, cols, rows, px, py);
        const long long i = (long long)py * (long long)cols + (long long)px;
        DnGuide gp = {};
        if (has) gp = dn_load_guide(guide, i);
        // a tile without a valid pixel (the background of a frame) passes through without staging anything
        if (!__syncthreads_or(has && gp.valid != 0.0)) {
            if (has) dn_store<LAST>(i, cin[3 * i], cin[3 * i + 1], cin[3 * i + 2], cout, out8);
            continue;
        }
        const long long ox = (long long)px - (long long)threadIdx.x - HALO, oy = (long long)py - (long long)threadIdx.y - HALO;
        for (int k = tid; k < NPX; k += kDnTileW * kDnTileH) {
            const int ly = k / W, lx = k - ly * W;
            const long long qx = ox + lx, qy = oy + ly;
            const bool in = qx >= 0 && qx < cols && qy >= 0 && qy < rows;
            double2 g0 = make_double2(0.0, 0.0), g1 = g0, g2 = g0, c01 = g0, cbx = g0, a01 = make_double2(NAN, 0.0);
            if (in) {
                const long long j = qy * (long long)cols + qx;
                const double2* q = reinterpret_cast<const double2*>(guide + j);
                const double2 g3 = q[3];
                if (g3.y != 0.0) {
                    g0 = q[0]; g1 = q[1]; g2 = q[2];
                    c01 = make_double2(cin[3 * j], cin[3 * j + 1]);
                    cbx = make_double2(cin[3 * j + 2], 1.0);
                    if (STOP) {
                        const double2* qa = reinterpret_cast<const double2*>(albedo + j);
                        a01 = qa[0];
                        cbx.y = qa[1].x;
                    }
                }
            }
            s_g[0][k] = g0; s_g[1][k] = g1; s_g[2][k] = g2;
            s_c01[k] = c01;
            s_cbx[k] = cbx;
            if (STOP) s_a01[k] = a01;
        }
        __syncthreads();
        if (has) {
            const int kc = ((int)threadIdx.y + HALO) * W + (int)threadIdx.x + HALO;
            double r, g, b;
            if (gp.valid != 0.0) {
                const double2 pc01 = s_c01[kc], pcbx = s_cbx[kc];
                const double2 pa01 = STOP ? s_a01[kc] : make_double2(0.0, 0.0);
                const V3 np = v3(gp.n[0], gp.n[1], gp.n[2]), Pp = v3(gp.P[0], gp.P[1], gp.P[2]), cp = v3(pc01.x, pc01.y, pcbx.x);
                DnAcc acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
                    for (int dx = -2; dx <= 2; ++dx) {
                        const int kq = kc + STEP * dy * W + STEP * dx;
                        const double2 qcbx = s_cbx[kq];
                        bool use;
                        if (STOP) {
                            const double2 qa01 = s_a01[kq];
                            use = qa01.x == pa01.x && qa01.y == pa01.y && qcbx.y == pcbx.y;
                        } else {
                            use = qcbx.y != 0.0;
                        }
                        if (!use) continue;
                        const double2 g0 = s_g[0][kq], g1 = s_g[1][kq], g2 = s_g[2][kq], qc01 = s_c01[kq];
                        dn_tap(acc, dn_h(dx + 2) * dn_h(dy + 2), np, Pp, gp.sp, cp, v3(g1.y, g2.x, g2.y), v3(g0.x, g0.y, g1.x),
                               v3(qc01.x, qc01.y, qcbx.x), npow, sigma2);
                    }
                }
                r = acc.r / acc.w;
                g = acc.g / acc.w;
                b = acc.b / acc.w;
            } else {
                r = cin[3 * i]; g = cin[3 * i + 1]; b = cin[3 * i + 2];
            }
            dn_store<LAST>(i, r, g, b, cout, out8);
        }
        __syncthreads();
    }
}
#endif

// level i's launch
template <bool STOP, bool LAST>
hipError_t dn_level(dim3 grid, dim3 block, hipStream_t stream, const DnIO& io, int i, int npow, double sigma2, const DnGuide* guide,
                    const DnAlbedo* albedo, const double* cin, double* cout, uint8_t* out8) {
#if GI_DN_LDS_STEPS
    if (i == 0) {
        hipLaunchKernelGGL((k_dn_level_lds<STOP, LAST, 1>), grid, block, 0, stream, io.cols, io.rows, npow, sigma2, guide, albedo, cin, cout, out8);
        return hipGetLastError();
    }
    if (i == 1 && GI_DN_LDS_STEPS >= 2) {
        hipLaunchKernelGGL((k_dn_level_lds<STOP, LAST, 2>), grid, block, 0, stream, io.cols, io.rows, npow, sigma2, guide, albedo, cin, cout, out8);
        return hipGetLastError();
    }
#endif
    hipLaunchKernelGGL((k_dn_level<STOP, LAST>), grid, block, 0, stream, io.cols, io.rows, 1 << i, npow, sigma2, guide, albedo, cin, cout, out8);
    return hipGetLastError();
}

// ---- the variance-guided filter (gi.h "variance-guided denoiser"; gi_denoise_var*) ----
// The same taps and stops, with the level's colour stop per pixel from the variance of the mean: k_dnv_g writes the
// 3 x 3 prefiltered variance g of the level's variance plane, k_dnv_level reads g at the centre, forms sigma2_p and
// carries the variance through the level beside the colour (three more doubles per tap).  Every level gathers from
// global memory (k_dn_level's form and tile deal); the LDS-staged form is not built for it: DESIGN.md §9.

// g_p of a valid pixel: the G x G weighted mean of v = (V.r + V.g) + V.b over its valid 3 x 3 neighbours in the window
__global__ __launch_bounds__(kDnTileW * kDnTileH) void k_dnv_g(int cols, int rows, const DnGuide* __restrict__ guide,
                                                                const double* __restrict__ vin, double* __restrict__ g) {
    const DnTiles tl = dn_tiles(cols, rows);
    for (long long slot = blockIdx.x; slot < tl.n_tiles; slot += gridDim.x) {
        int px = 0, py = 0;
        if (!dn_pixel(tl, slot, cols, rows, px, py)) continue;
        const long long i = (long long)py * (long long)cols + (long long)px;
        const double2 gp3 = reinterpret_cast<const double2*>(guide + i)[3];
        double out = 0.0;
        if (gp3.y != 0.0) {
            double sum_k = 0.0, sum_v = 0.0;
#pragma unroll
            for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
                for (int dx = -1; dx <= 1; ++dx) {
                    const int qy = py + dy, qx = px + dx;
                    const bool in = qy >= 0 && qy < rows && qx >= 0 && qx < cols;
                    const long long j = in ? (long long)qy * (long long)cols + (long long)qx : i;
                    const double2 gq3 = reinterpret_cast<const double2*>(guide + j)[3];
                    const double v = (vin[3 * j] + vin[3 * j + 1]) + vin[3 * j + 2];
                    if (!in || gq3.y == 0.0) continue;
                    const double k = (dx == 0 ? 0.5 : 0.25) * (dy == 0 ? 0.5 : 0.25);
                    sum_k += k;
                    sum_v += k * v;
                }
            }
            out = sum_v / sum_k;
        }
        g[i] = out;
    }
}

struct DnvAcc {
    double w, r, g, b, vr, vg, vb;
};

// One level: c_out, v_out = the filtered c_in and the propagated v_in at step `step`; sv2 = sigma_v sigma_v
// (+inf: no colour stop, whatever g is).  LAST: min(c, 1) into cout / out8 and the variance, as it is, into vout
// (each may be null).  Invalid pixels copy both through.
template <bool STOP, bool LAST>
__global__ __launch_bounds__(kDnTileW * kDnTileH) void k_dnv_level(int cols, int rows, int step, int npow, double sv2, double var_floor,
                                                                    const DnGuide* __restrict__ guide,
                                                                    const DnAlbedo* __restrict__ albedo, const double* __restrict__ gpl,
                                                                    const double* __restrict__ cin, const double* __restrict__ vin,
                                                                    double* __restrict__ cout, double* __restrict__ vout,
                                                                    uint8_t* __restrict__ out8) {
    const DnTiles tl = dn_tiles(cols, rows);
    for (long long slot = blockIdx.x; slot < tl.n_tiles; slot += gridDim.x) {
        const long long tile = dn_tile_of(slot, tl);
        int px = 0, py = 0;
        if (!dn_pixel(tl, tile, cols, rows, px, py)) continue;
        const long long i = (long long)py * (long long)cols + (long long)px;
        const DnGuide gp = dn_load_guide(guide, i);
        const double cr = cin[3 * i], cg = cin[3 * i + 1], cb = cin[3 * i + 2];
        double r = cr, g = cg, b = cb;
        double vr = vin[3 * i], vg = vin[3 * i + 1], vb = vin[3 * i + 2];
        if (gp.valid != 0.0) {
            double ar = 0.0, ag = 0.0, ab = 0.0;
            if (STOP) {
                const double2* qa = reinterpret_cast<const double2*>(albedo + i);
                const double2 a0 = qa[0], a1 = qa[1];
                ar = a0.x; ag = a0.y; ab = a1.x;
            }
            const double sigma2 = sv2 < INFINITY ? sv2 * gpl[i] + var_floor : INFINITY;
            const V3 np = v3(gp.n[0], gp.n[1], gp.n[2]);
            const V3 Pp = v3(gp.P[0], gp.P[1], gp.P[2]);
            DnvAcc acc = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
                for (int dx = -2; dx <= 2; ++dx) {
                    // (every tap's loads are issued whether it counts or not: k_dn_level)
                    const long long qy = (long long)py + (long long)step * dy, qx = (long long)px + (long long)step * dx;
                    const bool in = qy >= 0 && qy < rows && qx >= 0 && qx < cols;
                    const long long j = in ? qy * (long long)cols + qx : i;
                    const DnGuide gq = dn_load_guide(guide, j);
                    bool use = in && gq.valid != 0.0;
                    if (STOP) {
                        const double2* qa = reinterpret_cast<const double2*>(albedo + j);
                        const double2 a0 = qa[0], a1 = qa[1];
                        use = use && a0.x == ar && a0.y == ag && a1.x == ab;
                    }
                    const double qr = cin[3 * j], qg = cin[3 * j + 1], qb = cin[3 * j + 2];
                    const double ur = vin[3 * j], ug = vin[3 * j + 1], ub = vin[3 * j + 2];
                    if (!use) continue;
                    const double wt = dn_weight(dn_h(dx + 2) * dn_h(dy + 2), np, Pp, gp.sp, v3(cr, cg, cb), v3(gq.n[0], gq.n[1], gq.n[2]),
                                                v3(gq.P[0], gq.P[1], gq.P[2]), v3(qr, qg, qb), npow, sigma2);
                    const double w2 = wt * wt;
                    acc.w += wt;
                    acc.r += wt * qr;
                    acc.g += wt * qg;
                    acc.b += wt * qb;
                    acc.vr += w2 * ur;
                    acc.vg += w2 * ug;
                    acc.vb += w2 * ub;
                }
            }
            const double ww = acc.w * acc.w;
            r = acc.r / acc.w;
            g = acc.g / acc.w;
            b = acc.b / acc.w;
            vr = acc.vr / ww;
            vg = acc.vg / ww;
            vb = acc.vb / ww;
        }
        dn_store<LAST>(i, r, g, b, cout, out8);
        if (vout) {
            vout[3 * i] = vr;
            vout[3 * i + 1] = vg;
            vout[3 * i + 2] = vb;
        }
    }
}

long long dn_round16(long long b) { return (b + 15) & ~15ll; }
int dn_planes(int levels) { return levels - 1 < 2 ? levels - 1 : 2; }

}  // namespace

// gi_denoise_var's scratch: gi_denoise's for the same window and levels, then as many variance planes as colour
// planes, then the g plane.
long long dnv_scratch_bytes(long long n_px, int levels, bool albedo_stop) {
    return dn_scratch_bytes(n_px, levels, albedo_stop) + (long long)dn_planes(levels) * dn_round16(n_px * 3 * (long long)sizeof(double)) +
           dn_round16(n_px * (long long)sizeof(double));
}

// gi_denoise_var_device's launches on `stream`: k_dn_prep, then per level k_dnv_g and k_dnv_level.
hipError_t launch_denoise_var(const CamDev& cam, const DnvIO& io, const gi_denoise_var_params& p, void* scratch, hipStream_t stream) {
    const long long n_px = (long long)io.cols * (long long)io.rows;
    const bool stop = (p.flags & GI_DENOISE_ALBEDO_STOP) != 0;
    const long long plane_b = dn_round16(n_px * 3 * (long long)sizeof(double));
    char* base = static_cast<char*>(scratch);
    DnGuide* guide = reinterpret_cast<DnGuide*>(base);
    base += dn_round16(n_px * (long long)sizeof(DnGuide));
    DnAlbedo* albedo = nullptr;
    if (stop) {
        albedo = reinterpret_cast<DnAlbedo*>(base);
        base += dn_round16(n_px * (long long)sizeof(DnAlbedo));
    }
    const int np = dn_planes(p.levels);
    double* cpl[2] = {reinterpret_cast<double*>(base), reinterpret_cast<double*>(base + plane_b)};
    base += np * plane_b;
    double* vpl[2] = {reinterpret_cast<double*>(base), reinterpret_cast<double*>(base + plane_b)};
    base += np * plane_b;
    double* g = reinterpret_cast<double*>(base);
    const DnTiles tl = dn_tiles(io.cols, io.rows);
    const dim3 grid((unsigned)(tl.n_tiles < kDnMaxGrid ? tl.n_tiles : kDnMaxGrid)), block(kDnTileW, kDnTileH);
    hipLaunchKernelGGL(k_dn_prep, grid, block, 0, stream, cam, io.x0, io.y0, io.cols, io.rows, p.sigma_p, io.t, io.nrm,
                       stop ? io.alb : nullptr, guide, albedo);
    hipError_t e = hipGetLastError();
    const double sv2 = p.sigma_v * p.sigma_v;
    const double* cin = io.rgb;
    const double* vin = io.var;
    for (int i = 0; i < p.levels && e == hipSuccess; ++i) {
        const bool last = i == p.levels - 1;
        double* cout = last ? io.out : cpl[i & 1];
        double* vout = last ? io.out_var : vpl[i & 1];
        uint8_t* o8 = last ? io.out8 : nullptr;
        if (sv2 < INFINITY) hipLaunchKernelGGL(k_dnv_g, grid, block, 0, stream, io.cols, io.rows, guide, vin, g);
        with_bools([&](auto S, auto L) {
            hipLaunchKernelGGL((k_dnv_level<S.value, L.value>), grid, block, 0, stream, io.cols, io.rows, 1 << i, p.normal_pow_log2, sv2,
                               p.var_floor, guide, albedo, g, cin, vin, cout, vout, o8);
        }, stop, last);
        e = hipGetLastError();
        cin = cout;
        vin = vout;
    }
    return e;
}

// The scratch of one call over n_px window pixels: the guide records, the albedo records (albedo stop), and
// the colour planes between levels (none for one level, one for two, else two), each section 16-byte aligned.
long long dn_scratch_bytes(long long n_px, int levels, bool albedo_stop) {
    return dn_round16(n_px * (long long)sizeof(DnGuide)) + (albedo_stop ? dn_round16(n_px * (long long)sizeof(DnAlbedo)) : 0) +
           (long long)dn_planes(levels) * dn_round16(n_px * 3 * (long long)sizeof(double));
}

// gi_denoise_device's launches on `stream`: k_dn_prep, then k_dn_level once per level.  sigma2 of level i is
// (sigma_c 2^-i)^2: ldexp and one multiply, as the restatement computes it.
hipError_t launch_denoise(const CamDev& cam, const DnIO& io, const gi_denoise_params& p, void* scratch, hipStream_t stream) {
    const long long n_px = (long long)io.cols * (long long)io.rows;
    const bool stop = (p.flags & GI_DENOISE_ALBEDO_STOP) != 0;
    char* base = static_cast<char*>(scratch);
    DnGuide* guide = reinterpret_cast<DnGuide*>(base);
    base += dn_round16(n_px * (long long)sizeof(DnGuide));
    DnAlbedo* albedo = nullptr;
    if (stop) {
        albedo = reinterpret_cast<DnAlbedo*>(base);
        base += dn_round16(n_px * (long long)sizeof(DnAlbedo));
    }
    double* plane[2] = {reinterpret_cast<double*>(base), reinterpret_cast<double*>(base + dn_round16(n_px * 3 * (long long)sizeof(double)))};
    const DnTiles tl = dn_tiles(io.cols, io.rows);
    const dim3 grid((unsigned)(tl.n_tiles < kDnMaxGrid ? tl.n_tiles : kDnMaxGrid)), block(kDnTileW, kDnTileH);
    hipLaunchKernelGGL(k_dn_prep, grid, block, 0, stream, cam, io.x0, io.y0, io.cols, io.rows, p.sigma_p, io.t, io.nrm,
                       stop ? io.alb : nullptr, guide, albedo);
    hipError_t e = hipGetLastError();
    const double* cin = io.rgb;
    for (int i = 0; i < p.levels && e == hipSuccess; ++i) {
        const double s = std::ldexp(p.sigma_c, -i);
        const double sigma2 = s * s;
        const bool last = i == p.levels - 1;
        double* cout = last ? io.out : plane[i & 1];
        uint8_t* o8 = last ? io.out8 : nullptr;
        if (stop) e = last ? dn_level<true, true>(grid, block, stream, io, i, p.normal_pow_log2, sigma2, guide, albedo, cin, cout, o8)
                           : dn_level<true, false>(grid, block, stream, io, i, p.normal_pow_log2, sigma2, guide, albedo, cin, cout, o8);
        else e = last ? dn_level<false, true>(grid, block, stream, io, i, p.normal_pow_log2, sigma2, guide, albedo, cin, cout, o8)
                      : dn_level<false, false>(grid, block, stream, io, i, p.normal_pow_log2, sigma2, guide, albedo, cin, cout, o8);
        cin = cout;
    }
    return e;
}

}  // namespace gi
