// gi_launch.h — the host functions that libgi's kernel units (gi_kernels.hip, gi_adapt.hip, gi_mode_r.hip, gi_wf.hip, gi_sample.hip, gi_denoise.hip, gi_temporal.hip)
// define for each other and for gi_capi.cpp.  The only place where a cross-unit function is declared: the
// unit that defines one and the units that call it all include this header.  Host-only, no device code.
#pragma once

#include <hip/hip_runtime_api.h>

#include "gi.h"
#include "gi_scene.h"

namespace gi {

// Read once per process from the environment (thread-safe; several host threads may each drive their
// own device and scene).  One user knob: GI_X_MAX_RUN, the largest Mode X work-unit run length (scenes
// of cheap background samples such as the main.cpp scene prefer 8).  The rest are TEST hooks that pick
// among kernels whose frames are identical bit for bit (tests/test_gpu_parity.py compares them):
// GI_X_WF (0/1/2: force a Mode X form for a whole suite run), GI_X_HELP=0 (no shadow-ray handoff),
// GI_X_FLAT=0 (k_seg / k_wf_bounce walk the tree even where the scene's flat leaf table applies),
// GI_X_FAN=0 (the flat leaf query runs both exact tests of every fan-pair leaf: scenes uploaded by the process
// get DevScene::x_fan = 0, in the same kernels),
// GI_SEG_RING=0 (k_seg's lanes make their own units even where the per-wave ring fits),
// GI_R_FLAT (0/1/2: force a Mode R kernel), GI_RF_PER_SLOT (the flat Mode R pool size: 0 forces the
// per-tile overflow path), GI_RF_GROUP (1/4: force k_rf_reach's lanes per hit).
struct XEnv {
    int run_log2 = 0, help = 1, wf = -1, flat = 1, seg_ring = 1, fan = 1;
    int r_flat = -1;                  // Mode R kernels (GI_R_FLAT): 1 the flat phases for every scene, 0 k_mode_r
                                      // for every scene, 2 k_mode_r_batch for the whole frame (tests); -1 by size
    int rf_per_slot = 16;             // flat Mode R: pool pairs per pixel slot of the frame (GI_RF_PER_SLOT)
    int rf_group = 0;                 // k_rf_reach lanes per hit (GI_RF_GROUP): 0 by the launch's hits, 1 or 4 (tests)
};
const XEnv& x_env();

// One launch of a gi_wf.hip kernel: the instantiation (var, flat: wf_dispatch), its dynamic LDS and the
// kernel's resident workgroups (XLaunchCfg::wf_grid; unused where the grid follows the input alone).
struct XKernelCfg {
    XVariant var;
    bool flat;
    size_t lds_bytes;
    int resident;
};

// ---- gi_kernels.hip: k_mode_x with its classify and reduce passes, k_x_moments, k_unshard ----
long long shard_tiles(int w, int h, int shard_count);
constexpr long long kXWfChunk = 8ll << 20;   // wavefront form: units (pixel samples) per chunk = queue capacity
hipError_t x_launch_config(const DevScene& sc, int device, XLaunchCfg& cfg);
XForm x_form_choice(const DevScene& sc, const XLaunchCfg& xc, const gi_opts& o);
hipError_t launch_render(const DevScene& sc, const XLaunchCfg& xc, const CamDev& cam, V3 light, int w, int h, int y0,
                         const gi_opts& o, double* rgb, uint8_t* rgb8, const XScratch& xs, KTimer* kt,
                         hipStream_t stream);
hipError_t launch_unshard(int w, int h, int shard_count, const double* packed, const uint8_t* packed8, double* rgb,
                          uint8_t* rgb8, hipStream_t stream);

// One call of the sample moments (gi_frame_moments*; k_x_moments, k_x_moments_fill): the window [x0, x0 + cols) x
// [y0, y0 + rows) of the retained frame, its spp (the rows' stride) and the n samples rendered so far, and the
// output planes, device pointers, row-major over the window; a null output is not written.
struct MomentsIO {
    int x0, y0, cols, rows;
    int spp, n;
    double *mean, *var, *samples;
};
hipError_t launch_moments(const DevScene& sc, const XScratch& xs, const CamDev& cam, int w, int h, const MomentsIO& io,
                          hipStream_t stream);

// One pass of an adaptive frame (gi_render_adaptive*).  `o` is the pass as the render kernels see it: the caller's
// gi_opts with spp = k = sample_end - sample_begin, the rows' stride of the pass (the kernels use spp as a stride and
// as a "> 1" switch only); spp_max is the frame's own spp.  cur: which of the two ping-pong lists (0: xs.list,
// 1: xs.ad_list) holds the pass's active pixels; its survivors are appended to the other.  The pass's launches, all
// on `stream`: (first pass) classify into list 0 and k_x_adapt_init; the form's kernels over the active list, their
// rows in xs.part; k_x_adapt_fill and k_x_adapt_fold (gi_adapt.hip).
struct XAdaptPass {
    gi_adaptive_params p;
    gi_adaptive_out out;
    int spp_max;
    int cur;
};
hipError_t launch_adaptive(const DevScene& sc, const XLaunchCfg& xc, const CamDev& cam, V3 light, int w, int h,
                           const gi_opts& o, const XAdaptPass& ap, const XScratch& xs, KTimer* kt, hipStream_t stream);

// ---- gi_adapt.hip: k_x_adapt_init, k_x_adapt_fill, k_x_adapt_fold ----
// The per-slot state of a frame's first pass: n = 0 and S1 = S2 = +0 for the pixels classify listed, the resolved and
// the padding slots marked.
hipError_t launch_adapt_init(const DevScene& sc, const CamDev& cam, int w, int h, const XScratch& xs, hipStream_t stream);
// After the render kernels of the pass [s0, e): the planes of the pixels that were not active in it (k_x_adapt_fill),
// then per active entry the fold of its k = e - s0 rows, the decision, its planes and the survivors' list
// (k_x_adapt_fold).
hipError_t launch_adapt_fold(int w, int h, int s0, int e, const XAdaptPass& ap, const XScratch& xs, hipStream_t stream);

// ---- gi_mode_r.hip: the Mode R kernels, k_trace_ray, k_box_kat, the primitive KATs ----
RKernel r_kernel_choice(const DevScene& sc, const gi_opts& o);
// the GI_RF_* values gi_mode_r.hip was compiled with: the build hands its -D flags to the kernel units only
unsigned rf_own_pairs();
unsigned rf_page_pairs();
unsigned rf_max_pages();
unsigned rf_seg_pairs();
// launch_render's Mode R half: the frame's kernels, between ev_begin and ev_end where they are not null
hipError_t launch_mode_r(const DevScene& sc, const CamDev& cam, V3 light, int w, int h, int y0, const gi_opts& o,
                         double* rgb, uint8_t* rgb8, const XScratch& xs, hipStream_t stream, hipEvent_t ev_begin,
                         hipEvent_t ev_end);
hipError_t launch_trace_ray(const DevScene& sc, V3 o, V3 d, V3 light, int32_t* out_i, double* out_d, hipStream_t stream);
hipError_t launch_box_kat(int n, const double* recs, int32_t* out, hipStream_t stream);
// gi_kat_r_prims: kind 0 tri_hit(TriRec) (tris: n host-built records), 1 sphere_hit, 2 box_hit, 3 r_box_test<4> with
// 4 lanes per record; pn (6 doubles per record) is written for kinds 0 and 1 only
hipError_t launch_r_prims_kat(int kind, int n, const double* recs, const TriRec* tris, int32_t* hit, double* pn,
                              hipStream_t stream);
// gi_kat_r_entities: n rays x sc.n_ents entities through ent_hit (the TRI instantiation for r_tri_only scenes)
hipError_t launch_r_entities_kat(const DevScene& sc, int n, const double* rays, int32_t* hit, double* pn, hipStream_t stream);

// ---- gi_wf.hip: k_wf_bounce, k_seg, k_cast, k_aov, k_rad, k_cam_rays, the query and texel KATs ----
size_t wf_lds_bytes(const DevScene& sc, bool lds, bool flat);   // of k_wf_bounce and its kin, without the ring
size_t wf_seg_ring_bytes();
hipError_t wf_occupancy(const DevScene& sc, WfKernel k, const XKernelCfg& c, int* per_cu);
// A query launch (k_cast, k_aov, the KAT) on a scene: the variant, the flat choice and the dynamic LDS of a
// k_seg launch (launch_render's), with kernel k's resident workgroups.  flags (the KAT's; 0 elsewhere) bit 0:
// the tree walk where the flat table would apply (GI_X_FLAT=0 in process); bit 1: the HBM-resident variants
// (the level stack instead of the staged scene) for a scene that would be staged in LDS.
XKernelCfg x_query_cfg(const XLaunchCfg& xc, int flags, WfKernel k);
hipError_t launch_wf(const DevScene& sc, const XKernelCfg& c, XForm form, const CamDev& cam, V3 light, int w, int h, int y0,
                     const gi_opts& o, double* rgb, uint8_t* rgb8, const XScratch& xs, const unsigned* n_list_dev,
                     unsigned long long* stats, int xflags, uint32_t live, hipStream_t stream, hipEvent_t ev_begin, hipEvent_t ev_end);
// The live mask of a Mode X launch's shadow queries (gi_scene.h x_shadow_live): full unless the launch runs the
// scene's flat query with shadow rays, without GI_FLAG_X_ALL_LEAVES, from a near camera.
inline uint32_t x_launch_live(const DevScene& sc, const XLaunchCfg& xc, V3 cam_pos, V3 light, unsigned flags) {
    const double L[3] = {light.x, light.y, light.z}, C[3] = {cam_pos.x, cam_pos.y, cam_pos.z};
    const bool full = !sc.x_flat || (flags & (GI_FLAG_X_NO_SHADOW | GI_FLAG_X_ALL_LEAVES)) != 0;
    return x_shadow_live(xc.shadow, L, C, (double)sc.x_far_r, full);
}
hipError_t launch_x_query_kat(const DevScene& sc, const XKernelCfg& c, V3 cam_pos, int n, const double* recs, int32_t* oi,
                              double* od, hipStream_t stream);
hipError_t launch_x_texel_kat(const DevScene& sc, XVariant var, int n, int mode, const double* recs, int32_t* oi, double* od,
                              hipStream_t stream);
hipError_t launch_cast(const DevScene& sc, const XKernelCfg& c, bool any, const CastIO& io, hipStream_t stream);
hipError_t launch_aov(const DevScene& sc, const XKernelCfg& c, const CamDev& cam, const AovIO& io, hipStream_t stream);
hipError_t launch_cam_rays(const CamDev& cam, int x0, int y0, int cols, int rows, double* rays, hipStream_t stream);
// gi_radiance*: k_rad over io's records.  GI_RAD_MAX_GRID (a TEST hook like those of XEnv, but read at every
// launch): the most workgroups a launch takes.
hipError_t launch_rad(const DevScene& sc, const XKernelCfg& c, const RadIO& io, hipStream_t stream);
void wf_variant(const DevScene& sc, const XKernelCfg& c, int32_t out[6]);

// ---- gi_sample.hip: k_sample_rays, k_resolve ----
// One call of the sample-ray generator (gi_sample_rays*): the window [x0, x0 + cols) x [y0, y0 + rows) of the
// frame cam was made for, the samples [s0, s1) of every pixel, and the outputs, device pointers laid out
// [window pixel, row-major][s - s0]; a null output is not written.  fwd: the camera's forward vector (the lens).
struct SampleIO {
    int x0, y0, cols, rows, w;
    int s0, s1;
    int jitter;
    uint64_t seed;
    double aperture, focus;
    V3 fwd;
    double* rays;     // GI_RAY_DOUBLES per record, 16-byte aligned
    uint64_t* ids;    // gi_path_id as two words per record
};
hipError_t launch_sample_rays(const CamDev& cam, const SampleIO& io, hipStream_t stream);
// gi_resolve_samples*: rows [n_pix][ns][3] to the pixels' clamped means and their 8-bit form
hipError_t launch_resolve(long long n_pix, int ns, const double* rows, double* rgb, uint8_t* rgb8, hipStream_t stream);

// ---- gi_denoise.hip: k_dn_prep, k_dn_level, k_dnv_g, k_dnv_level ----
// One call of the denoiser (gi_denoise*): the window [x0, x0 + cols) x [y0, y0 + rows) of the frame, its
// input planes and outputs, device pointers, row-major over the window; alb is read only with the albedo
// stop; a null output is not written.
struct DnIO {
    int x0, y0, cols, rows;
    const double *rgb, *t, *nrm, *alb;
    double* out;
    uint8_t* out8;
};
long long dn_scratch_bytes(long long n_px, int levels, bool albedo_stop);   // host only
hipError_t launch_denoise(const CamDev& cam, const DnIO& io, const gi_denoise_params& p, void* scratch, hipStream_t stream);
// One call of the variance-guided denoiser (gi_denoise_var*; k_dn_prep, k_dnv_g, k_dnv_level): as DnIO, with the
// variance plane of the mean and its filtered output.
struct DnvIO {
    int x0, y0, cols, rows;
    const double *rgb, *var, *t, *nrm, *alb;
    double *out, *out_var;
    uint8_t* out8;
};
long long dnv_scratch_bytes(long long n_px, int levels, bool albedo_stop);   // host only
hipError_t launch_denoise_var(const CamDev& cam, const DnvIO& io, const gi_denoise_var_params& p, void* scratch, hipStream_t stream);

// ---- gi_temporal.hip: k_temporal ----
// One call of the temporal accumulation (gi_temporal*): the window [x0, x0 + cols) x [y0, y0 + rows) of the frame,
// the current frame's planes, the history's (hist.rgb null: no history, every valid pixel resets; `prev` is then
// not read) and the outputs, device pointers, row-major over the window; a null output is not written.  The prim
// planes are read only with GI_TEMPORAL_PRIM_STOP, the var planes only where out.var is written.
struct TpIO {
    int x0, y0, cols, rows;
    gi_temporal_frame cur, hist;
    gi_temporal_out out;
};
hipError_t launch_temporal(const CamDev& cam, const CamDev& prev, const TpIO& io, const gi_temporal_params& p, hipStream_t stream);

}  // namespace gi
