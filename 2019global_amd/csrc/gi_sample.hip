// gi_sample.hip — the two scene-less kernels around the radiance query (gi_radiance*, gi_wf.hip k_rad):
//   k_sample_rays  a frame's pixel-sample rays as the render kernels make them (wf_primary: the pixel's RNG key,
//                  the jitter of sample s, primary_dir), optionally through a thin lens, as ray records and path
//                  ids for gi_radiance*;
//   k_resolve      per-sample radiance rows to pixels: k_x_reduce's sum in sample order, mean, clamp and 8-bit form.
// Only + - * / sqrt, comparisons and the integer hash, without contraction: a numpy restatement is exact
// (tests/radiance_ref.py).
#include <hip/hip_runtime.h>

#include <algorithm>

#include "gi.h"
#include "gi_dev.h"
#include "gi_launch.h"
#include "gi_scene.h"

namespace gi {
namespace {

// Record g = pixel * ns + (s - s0) of the window, one lane each; pixel (px, py) row-major over the window.
//  stream = y w + x of the frame pixel, key = mx_key(seed, stream): the renders' (wf_primary)
//  jitter: (jx, jy) = mx_u01k(key, s, 0xFFFF, 0 / 1) -- a render's for spp > 1 -- or (0, 0)
//  d0 = primary_dir(cam, x + jx, y + jy), unnormalised: k_rad normalises as the renders do
//  aperture == 0: o = cam.pos, d = d0
//  aperture > 0 (gi.h "sample rays" fixes the order): (lx, ly) = mx_disk(mx_u01k(key, s, 0xFFFE, 0 / 1)),
//    F = pos + d0 * (focus / dot(d0, fwd)), o = (pos + left * (aperture * lx)) + up * (aperture * ly), d = F - o
__global__ __launch_bounds__(256) void k_sample_rays(CamDev cam, SampleIO io) {
    const unsigned long long ns = (unsigned long long)(io.s1 - io.s0);
    const unsigned long long total = (unsigned long long)io.cols * (unsigned long long)io.rows * ns;
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long g = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; g < total; g += stride) {
        unsigned long long pix, px, py;
        unsigned sj;
        if (g < (1ull << 32)) {   // 32-bit division where it suffices
            const unsigned p = (unsigned)g / (unsigned)ns;
            sj = (unsigned)g - p * (unsigned)ns;
            py = p / (unsigned)io.cols;
            px = p - (unsigned)py * (unsigned)io.cols;
            pix = p;
        } else {
            pix = g / ns;
            sj = (unsigned)(g - pix * ns);
            py = pix / (unsigned long long)io.cols;
            px = pix - py * (unsigned long long)io.cols;
        }
        const unsigned s = (unsigned)io.s0 + sj;
        const uint64_t x = (uint64_t)io.x0 + px, y = (uint64_t)io.y0 + py;
        const uint64_t stream = y * (uint64_t)io.w + x;
        const uint64_t key = mx_key(io.seed, stream);
        double jx = 0.0, jy = 0.0;
        if (io.jitter) {
            jx = mx_u01k(key, s, 0xFFFF, 0);
            jy = mx_u01k(key, s, 0xFFFF, 1);
        }
        const V3 d0 = primary_dir(cam, (double)x + jx, (double)y + jy);
        V3 o = cam.pos, d = d0;
        if (io.aperture > 0.0) {
            double lx, ly, r2;
            mx_disk(mx_u01k(key, s, 0xFFFE, 0), mx_u01k(key, s, 0xFFFE, 1), lx, ly, r2);
            const V3 F = cam.pos + d0 * (io.focus / dot(d0, io.fwd));
            o = (cam.pos + cam.left * (io.aperture * lx)) + cam.up * (io.aperture * ly);
            d = F - o;
        }
        if (io.rays) {   // a 64-byte record in four 16-byte stores
            double2* q = reinterpret_cast<double2*>(io.rays) + 4 * g;
            q[0] = make_double2(o.x, o.y);
            q[1] = make_double2(o.z, d.x);
            q[2] = make_double2(d.y, d.z);
            q[3] = make_double2(INFINITY, 0.0);
        }
        if (io.ids) {
            io.ids[2 * g] = stream;
            io.ids[2 * g + 1] = (uint64_t)s;   // sample, reserved = 0
        }
    }
}

// Pixel i of n_pix: sum = +0, sum += row s in sample order, mean = sum / (double)ns, min(mean, 1) as
// mean < 1 ? mean : 1 (smin), then quantize -- k_x_reduce's operations on rows [n_pix][ns][3].
__global__ __launch_bounds__(256) void k_resolve(long long n_pix, int ns, const double* rows, double* rgb, uint8_t* rgb8) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n_pix; i += stride) {
        const double* p = rows + 3 * (size_t)i * (size_t)ns;
        double a = 0, b = 0, c = 0;
        for (int s = 0; s < ns; ++s) {
            a = a + p[3 * s];
            b = b + p[3 * s + 1];
            c = c + p[3 * s + 2];
        }
        const double n = (double)ns;
        const double c0 = smin(a / n, 1.0), c1 = smin(b / n, 1.0), c2 = smin(c / n, 1.0);
        if (rgb) { rgb[3 * i] = c0; rgb[3 * i + 1] = c1; rgb[3 * i + 2] = c2; }
        if (rgb8) quantize(c0, c1, c2, rgb8 + 3 * i);
    }
}

}  // namespace

// gi_sample_rays*: grid-stride over at most 2048 workgroups, as k_cam_rays.  Asynchronous on `stream`.
hipError_t launch_sample_rays(const CamDev& cam, const SampleIO& io, hipStream_t stream) {
    if (io.cols <= 0 || io.rows <= 0 || io.s1 <= io.s0) return hipSuccess;
    const unsigned long long total = (unsigned long long)io.cols * (unsigned long long)io.rows * (unsigned long long)(io.s1 - io.s0);
    const dim3 grid((unsigned)std::min<unsigned long long>((total + 255) / 256, 2048)), block(256);
    hipLaunchKernelGGL(k_sample_rays, grid, block, 0, stream, cam, io);
    return hipGetLastError();
}

// gi_resolve_samples*: one lane per pixel, grid-stride over at most 2048 workgroups.  Asynchronous on `stream`.
hipError_t launch_resolve(long long n_pix, int ns, const double* rows, double* rgb, uint8_t* rgb8, hipStream_t stream) {
    if (n_pix <= 0) return hipSuccess;
    const dim3 grid((unsigned)std::min<long long>((n_pix + 255) / 256, 2048)), block(256);
    hipLaunchKernelGGL(k_resolve, grid, block, 0, stream, n_pix, ns, rows, rgb, rgb8);
    return hipGetLastError();
}

}  // namespace gi
