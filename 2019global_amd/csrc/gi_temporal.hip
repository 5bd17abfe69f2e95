// gi_temporal.hip — temporal accumulation (gi.h "temporal accumulation"; DESIGN.md §5 "Temporal accumulation"):
// the previous frame's accumulated colour and variance reprojected onto the current frame's first hits and
// blended with the current frame.  A memory-bound gather: no scene, no traversal, no scratch; everything is fp64
// and every sum is sequential in the order gi.h gives, so a numpy restatement (tests/temporal_ref.py) is exact
// bit for bit.
//   k_temporal   one lane per window pixel: the point the pixel shows, its pixel coordinate in the previous
//                camera (the inverse of primary_dir), the four bilinear taps of the history straight from global
//                memory, each tested against the pixel (validity, length, primitive, normal, plane), the blend
// Lane mapping: workgroup tiles of 64 x 4 window pixels, a wave per tile row, lanes along x (the denoiser's) -- under
// a camera that moved by a translation or a small rotation neighbouring lanes reproject to neighbouring history
// pixels, so each tap of a wave is one nearly contiguous run per plane and the tile's rows share their vertical
// taps in the caches.  The previous camera, with the vectors of the inversion made once on the host (the same
// fp64 operations, not contracted on either side), travels in the kernel arguments.  64-bit indices.
// Resources and rates: DESIGN.md §9 "Temporal accumulation".
#include <hip/hip_runtime.h>

#include "gi_dev.h"
#include "gi_launch.h"

namespace gi {
namespace {

constexpr int kTpTileW = 64, kTpTileH = 4;
constexpr long long kTpMaxGrid = 1ll << 20;   // workgroups per launch; more tiles: a grid-stride loop

// The previous camera as the kernel needs it: its own frame vectors (primary_dir of a tap) and, for x' and y',
// N = A x B, B x T, T x A and det = T . N with A = left rx, B = up ry, T = top_left (gi.h)
struct TpPrev {
    CamDev cam;
    V3 n, bxt, txa;
    double det;
};

struct TpParams {
    double alpha_min, cos_min, sigma_p;
    int max_history;
    int has_hist;
};

// PRIM: the prim stop; VAR: the variance is carried (out.var is written; cur.var and hist.var are read)
template <bool PRIM, bool VAR>
__global__ __launch_bounds__(kTpTileW * kTpTileH) void k_temporal(CamDev cam, TpPrev prev, TpParams p, int x0, int y0, int cols, int rows,
                                                                   gi_temporal_frame cur, gi_temporal_frame hist, gi_temporal_out out) {
    const int tiles_x = (cols + kTpTileW - 1) / kTpTileW;
    const long long n_tiles = (long long)tiles_x * (long long)((rows + kTpTileH - 1) / kTpTileH);
    for (long long tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        // (the division is uniform over the workgroup; 32 bits where the tile index allows it)
        const long long ty = tile < (1ll << 32) ? (long long)((unsigned)tile / (unsigned)tiles_x) : tile / tiles_x;
        const int px = (int)(tile - ty * tiles_x) * kTpTileW + (int)threadIdx.x;
        const long long pyl = ty * kTpTileH + (long long)threadIdx.y;
        if (px >= cols || pyl >= rows) continue;
        const int py = (int)pyl;
        const long long i = pyl * (long long)cols + (long long)px;
        const double tp = cur.t[i];
        double r = cur.rgb[3 * i], g = cur.rgb[3 * i + 1], b = cur.rgb[3 * i + 2];
        double vr = 0.0, vg = 0.0, vb = 0.0;
        if (VAR) {
            vr = cur.var[3 * i]; vg = cur.var[3 * i + 1]; vb = cur.var[3 * i + 2];
        }
        int len = 0;
        if (tp < INFINITY) {
            len = 1;
            if (p.has_hist) {
                const V3 d = normalize(primary_dir(cam, (double)(x0 + px), (double)(y0 + py)));
                const V3 P = cam.pos + tp * d;
                const V3 v = P - prev.cam.pos;
                const double den = dot(v, prev.n);
                const double xs = -dot(v, prev.bxt) / den, ys = -dot(v, prev.txa) / den;
                const double fx = floor(xs), fy = floor(ys);
                // compared as doubles: a far-away or NaN coordinate never reaches the conversion to int
                const bool seen = den * prev.det > 0.0 && fabs(xs) < INFINITY && fabs(ys) < INFINITY &&
                                  fx >= (double)x0 - 1.0 && fx <= (double)(x0 + cols) - 1.0 &&
                                  fy >= (double)y0 - 1.0 && fy <= (double)(y0 + rows) - 1.0;
                if (seen) {
                    const int qx0 = (int)fx - x0, qy0 = (int)fy - y0;   // window coordinates of tap (0, 0): -1 .. cols-1, -1 .. rows-1
                    const double wx = xs - fx, wy = ys - fy;
                    const V3 np = ld3(cur.normal + 3 * i);
                    const int prim_p = PRIM ? cur.prim[i] : 0;
                    const double sp = p.sigma_p * tp;
                    double sum_b = 0.0, cr = 0.0, cg = 0.0, cb = 0.0, hr = 0.0, hg = 0.0, hb = 0.0;
                    int len_h = 0x7fffffff;
                    bool any = false;
#pragma unroll
                    for (int tj = 0; tj < 2; ++tj) {
#pragma unroll
                        for (int ti = 0; ti < 2; ++ti) {
                            // every tap's loads are issued whether it counts or not (coordinates clamped to the
                            // pixel's own, which is inside the window), so that they do not wait on each other's tests
                            const int qx = qx0 + ti, qy = qy0 + tj;
                            const bool in = qx >= 0 && qx < cols && qy >= 0 && qy < rows;
                            const long long j = in ? (long long)qy * (long long)cols + (long long)qx : i;
                            const double tq = hist.t[j];
                            const int len_q = hist.len[j];
                            const int prim_q = PRIM ? hist.prim[j] : 0;
                            const V3 nq = ld3(hist.normal + 3 * j);
                            const V3 cq = ld3(hist.rgb + 3 * j);
                            V3 vq = v3(0.0, 0.0, 0.0);
                            if (VAR) vq = ld3(hist.var + 3 * j);
                            const double bw = (ti ? wx : 1.0 - wx) * (tj ? wy : 1.0 - wy);
                            const V3 dq = normalize(primary_dir(prev.cam, (double)(x0 + qx), (double)(y0 + qy)));
                            const V3 Pq = prev.cam.pos + tq * dq;
                            bool use = in && bw > 0.0 && tq < INFINITY && len_q >= 1 && dot(np, nq) >= p.cos_min &&
                                       fabs(dot(np, Pq - P)) <= sp;   // (a NaN fails its comparison)
                            if (PRIM) use = use && prim_q == prim_p;
                            if (!use) continue;
                            any = true;
                            sum_b += bw;
                            cr += bw * cq.x; cg += bw * cq.y; cb += bw * cq.z;
                            if (VAR) {
                                hr += bw * vq.x; hg += bw * vq.y; hb += bw * vq.z;
                            }
                            len_h = len_q < len_h ? len_q : len_h;
                        }
                    }
                    if (any) {
                        len = len_h >= p.max_history ? p.max_history : len_h + 1;   // min(len_h + 1, max_history)
                        const double inv = 1.0 / (double)len;
                        const double a = inv > p.alpha_min ? inv : p.alpha_min, na = 1.0 - a;
                        r = (na * (cr / sum_b)) + (a * r);
                        g = (na * (cg / sum_b)) + (a * g);
                        b = (na * (cb / sum_b)) + (a * b);
                        if (VAR) {
                            const double na2 = na * na, a2 = a * a;
                            vr = (na2 * (hr / sum_b)) + (a2 * vr);
                            vg = (na2 * (hg / sum_b)) + (a2 * vg);
                            vb = (na2 * (hb / sum_b)) + (a2 * vb);
                        }
                    }
                }
            }
        }
        if (out.rgb) {
            out.rgb[3 * i] = r; out.rgb[3 * i + 1] = g; out.rgb[3 * i + 2] = b;
        }
        if (VAR) {
            out.var[3 * i] = vr; out.var[3 * i + 1] = vg; out.var[3 * i + 2] = vb;
        }
        if (out.len) out.len[i] = len;
    }
}

}  // namespace

// gi_temporal_device's launch on `stream`.  io.hist.rgb null: no history (prev is not read).
hipError_t launch_temporal(const CamDev& cam, const CamDev& prev, const TpIO& io, const gi_temporal_params& p, hipStream_t stream) {
    TpPrev pv;
    pv.cam = prev;
    const V3 A = prev.left * prev.rx, B = prev.up * prev.ry, T = prev.top_left;
    pv.n = cross(A, B);
    pv.bxt = cross(B, T);
    pv.txa = cross(T, A);
    pv.det = dot(T, pv.n);
    const TpParams tp{p.alpha_min, p.cos_min, p.sigma_p, p.max_history, io.hist.rgb != nullptr};
    const long long n_tiles = (long long)((io.cols + kTpTileW - 1) / kTpTileW) * (long long)((io.rows + kTpTileH - 1) / kTpTileH);
    const dim3 grid((unsigned)(n_tiles < kTpMaxGrid ? n_tiles : kTpMaxGrid)), block(kTpTileW, kTpTileH);
    with_bools([&](auto PR, auto VA) {
        hipLaunchKernelGGL((k_temporal<PR.value, VA.value>), grid, block, 0, stream, cam, pv, tp, io.x0, io.y0, io.cols, io.rows, io.cur,
                           io.hist, io.out);
    }, (p.flags & GI_TEMPORAL_PRIM_STOP) != 0, io.out.var != nullptr);
    return hipGetLastError();
}

}  // namespace gi
