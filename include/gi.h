/* gi.h — C-ABI of the MI355X-native (gfx950) per-pixel radiance path for preon7/2019global.
 *
 * This is the drop-in boundary for the reference's render driver.  The reference has no ABI: its
 * path is the header-only class RayTracer (include/raytracer.h:15-101) whose run(w, h)
 * (raytracer.h:23-87) loops over pixels and, per pixel, queries Octree::intersect
 * (octree.h:46-68), calls Entity::intersect / getTextureCoord (entities.h:26, 32) and
 * Material::blinn_phong_texture (material.h:48-62), and stores through Image::setPixel
 * (image.h:14-16).  The entry points below replace, one for one:
 *
 *   gi_scene_create      Octree(min,max) (octree.h:14) + Octree::push_back per entity
 *                        (octree.h:20-43) + the entity constructors (entities.h:45, 138, 581, ...)
 *   gi_camera_init       Camera(pos, lookAt, focal) (camera.h:8-10)
 *   gi_render            RayTracer::run(w, h) (raytracer.h:23-87), host buffers, progressive tiles,
 *                        cancel flag = RayTracer::stop() (raytracer.h:90)
 *   gi_render_device     the same frame into device-resident buffers on a HIP stream (bench,
 *                        multi-GPU tile sharding)
 *   gi_trace_ray         one iteration of raytracer.h:41-84 for an arbitrary ray
 *   gi_intersect*        batched ray queries over the Mode X acceleration structure (no reference
 *   gi_occluded*         counterpart): closest hit / any hit of caller-supplied rays, from host buffers
 *                        or device-resident on a HIP stream
 *   gi_render_aov*       first-hit feature buffers (AOVs) of a frame's pixels: distance, facing normal,
 *                        albedo, primitive, entity, texture coordinate (no reference counterpart)
 *   gi_camera_rays*      a frame's pixel rays (raytracer.h:41-43) as ray records for gi_intersect* /
 *                        gi_occluded*
 *   gi_denoise*          an edge-avoiding a-trous filter of a frame over those feature buffers: a preview of
 *                        the first progressive passes (no reference counterpart)
 *   gi_temporal*         reprojects the previous frame's accumulated colour and variance onto a frame's first
 *                        hits and blends them with it: samples kept while the camera moves (no reference counterpart)
 *   gi_render_adaptive*  a Mode X frame in sample passes that stop tracing the pixels whose error estimate has
 *                        fallen below a tolerance (no reference counterpart)
 *   gi_radiance*         Mode X's path tracer on caller-supplied rays: one path sample per ray record, its
 *                        radiance out (no reference counterpart)
 *   gi_sample_rays*      the rays a Mode X render traces for a frame's pixel samples, optionally through a thin
 *                        lens, as records for gi_radiance*
 *   gi_resolve_samples*  per-sample radiance rows to pixels, as the renders resolve theirs
 *   gi_unshard_device    reassembles a frame from per-rank packed tiles after the RCCL gather
 *   gi_scene_kernel_ms   HIP-event duration of the last timed render's dominant kernel (bench)
 *   gi_scene_x_form      which Mode X form (persistent kernel / wavefront) a render would run
 *   gi_scene_seg_ring    whether that form would refill its lanes from the per-wave ring of primary rays
 *   gi_kat_*             known-answer TEST hooks: the device's ExpBox node test and the Mode X
 *                        queries ray by ray (gi_kat_x_query, gi_kat_x_variant), the texel a hit
 *                        is shaded with (gi_kat_x_texel)
 *   gi_octree_*          Octree(min,max) + push_back (octree.h:14-43) and the public query
 *                        Octree::intersect(const Ray&) (octree.h:46-68 -> Node::intersect :132-155)
 *                        on the host, for reference-side callers of the candidate list
 *   gi_obj_parse         scene I/O: a Wavefront OBJ mesh as the run of
 *                        ImpTriangle(p1, p2, p3) pushes (entities.h:138) main.cpp:24-48 would write
 *   gi_multi_*           RayTracer::run over several GPUs of one process: a scene replica per
 *                        device, 8x8 tiles dealt round-robin, RCCL send/recv gather over xGMI to
 *                        the first device (the drop-in RayTracer uses it when GI_DEVICES lists
 *                        devices; by default it renders on the current device alone)
 *
 * Conventions: all pointers are plain C pointers; buffers are caller-owned; sizes are in elements;
 * every function returns 0 on success and a negative gi_status on error, with a thread-local
 * message from gi_last_error().  No exception crosses this boundary.  Rendering never falls back
 * to the CPU: without a usable gfx950 device gi_scene_create fails with GI_ERR_DEVICE.
 */
#ifndef GI_H_
#define GI_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GI_ABI_VERSION 21

typedef enum gi_status {
    GI_OK = 0,
    GI_ERR_ARG = -1,      /* invalid argument */
    GI_ERR_DEVICE = -2,   /* HIP error / no device */
    GI_ERR_SCENE = -3,    /* unsupported entity or material; coordinates beyond the supported range */
    GI_ERR_CANCELLED = -4,/* *cancel became non-zero; frame partially rendered */
    GI_ERR_NOMEM = -5,    /* host memory exhausted (std::bad_alloc inside the library) */
    GI_ERR_INTERNAL = -6  /* any other exception caught at the boundary */
} gi_status;

/* Entity kinds.  args[] holds the reference constructor's arguments in constructor order. */
typedef enum gi_entity_kind {
    GI_IMP_SPHERE = 1,   /* ImpSphere(pos, float radius, color)              entities.h:45  args: px py pz r cr cg cb            */
    GI_IMP_TRIANGLE = 2, /* ImpTriangle(p1, p2, p3) (material: red)          entities.h:138 args: p1 p2 p3 (9)                   */
    GI_EXP_QUAD = 3,     /* ExpQuad(pos, float w, float l, float alpha, col) entities.h:581 args: px py pz w l alpha cr cg cb    */
    GI_EXP_SPHERE = 4,   /* ExpSphere(pos, float radius, color)              entities.h:461 args: px py pz r cr cg cb            */
    GI_EXP_CUBE = 5,     /* ExpCube(pos, float w, float l, float h, color)   entities.h:652 args: px py pz w l h cr cg cb        */
    GI_EXP_CONE = 6,     /* ExpCone(pos, dir, float h, float r, color)       entities.h:823 args: px py pz dx dy dz h r cr cg cb */
                         /*   (dir is stored but unused: the reference cone always points along (-1,0,-10), :825)           */
    GI_EXP_RECTANGLE = 7,/* ExpRectangle(p1, p2, p3) (material: red)         entities.h:310 args: p1 p2 p3 (9)                   */
    GI_EXP_BOX = 8       /* ExpBox(min, max) (material: red)                 entities.h:381 args: min max (6)                    */
} gi_entity_kind;

typedef struct gi_entity_desc {
    int32_t kind;               /* gi_entity_kind */
    int32_t has_material;       /* 1: entity->material = Material(mat_color, mat_shader); specular_power set */
    double args[11];
    double mat_color[3];
    double mat_shader[3];       /* Material::shader_parameters (material.h:27) */
    double mat_specular_power;  /* Material::specular_power (material.h:29) */
    double mat_reflectivity;    /* Mode X only (the reference has no mirrors): probability in [0, 1] that a
                                   bounce leaves by mirror reflection instead of a diffuse sample (DESIGN.md
                                   "Mode X"); 0 (value-initialised descriptors) = diffuse only.  Mode R
                                   ignores it. */
} gi_entity_desc;

typedef struct gi_scene_desc {
    double octree_min[3];       /* Octree(min, max) */
    double octree_max[3];
    int32_t n_entities;         /* push_back order = candidate order */
    const gi_entity_desc* entities;
} gi_scene_desc;

/* Camera as the reference stores it (camera.h:16-20). */
typedef struct gi_camera {
    double pos[3];
    double up[3];
    double forward[3];          /* normalised */
    double focal;
} gi_camera;

typedef enum gi_mode {
    GI_MODE_R = 0,  /* the reference's semantics bit for bit (depth 1, 1 spp) */
    GI_MODE_X = 1   /* build-defined depth/spp integrator (DESIGN.md "Mode X") */
} gi_mode;

#define GI_FLAG_STATS 1u   /* accumulate work counters into opts->stats (device pointer) */
#define GI_FLAG_R_DFS 2u   /* Mode R: walk the whole reference octree in reverse DFS order instead of
                              reconstructing the candidate list (same result; A/B and tests) */
#define GI_FLAG_TIME 4u    /* record HIP events around the frame's dominant kernel (k_mode_r / k_mode_x; the
                              wavefront form and Mode R's flat phases: their whole sequence) on the render's
                              stream; averaged by gi_scene_kernel_ms */
#define GI_FLAG_X_NO_SHADOW 8u   /* Mode X, test only: no shadow rays (every light is visible).  With
                                    depth 1 and spp 1 this reduces Mode X to the reference's own
                                    shading (raytracer.h:41-84, material.h:48-62), so its stages can
                                    be checked against the reference's frames (tests) */
#define GI_FLAG_X_WF 16u         /* Mode X: the wavefront form (one launch per bounce over a compacted queue of
                                    live paths, gi_wf.hip) whatever the scene; same frame bit for bit.  A test
                                    reference (slower everywhere) */
#define GI_FLAG_X_MEGA 32u       /* Mode X: the persistent path-state kernel (k_mode_x) whatever the scene.  It reads
                                    every scene from global memory: a scene that k_seg stages in LDS
                                    (gi_scene_info.x_lds_resident) is traversed there like a large one -- same
                                    frame bit for bit, slower than the default; for tests and A/B */
#define GI_FLAG_X_SEG 64u        /* Mode X: the segment-synchronous persistent form (k_seg: every loop
                                    iteration one whole path segment per lane).  None of the three form
                                    flags: chosen per launch (GI_X_WF=0/1/2 overrides) */
#define GI_FLAG_X_ALL_LEAVES 128u /* Mode X, test only (ABI 19): the shadow queries of the flat leaf query visit every
                                    leaf of the table, also those the launch's light cannot be occluded by
                                    (gi_scene_shadow_leaves); same frame bit for bit */

typedef struct gi_opts {
    int32_t mode;          /* gi_mode */
    int32_t spp;           /* Mode X samples per pixel (>= 1) */
    int32_t depth;         /* Mode X path length (>= 1) */
    int32_t shard_count;   /* >= 1: number of ranks the frame is split over */
    int32_t shard_index;   /* this rank, 0 <= shard_index < shard_count */
    int32_t band_rows;     /* gi_render only: rows per progressive band (0 = whole frame) */
    uint32_t flags;        /* GI_FLAG_* */
    int32_t reserved;
    uint64_t seed;         /* Mode X RNG seed */
    uint64_t* stats;       /* device pointer to GI_STATS_N uint64 counters (GI_FLAG_STATS) */
    /* Mode X progressive passes (ABI 10; both 0: the whole frame at once).  A pass renders samples
     * [sample_begin, sample_end) of the spp-sample frame (spp > 1) and delivers the running estimate
     * min(sum over samples s < sample_end / sample_end, 1) -- for sample_end > 1 exactly the frame of
     * spp = sample_end, since the samples' jitter and paths do not depend on spp (a pass ending at
     * sample 1 holds the JITTERED sample 0 of the spp-sample frame, while a real spp = 1 frame is not
     * jittered); the pass with sample_end == spp is the one-shot frame bit for bit.  A pass is
     * accepted when it has been issued: a device error that surfaces later (a failed launch, a
     * fault) ends the progressive frame -- the next continuation is refused (GI_ERR_DEVICE) and the
     * frame restarts at sample 0.  Passes continue one frame: they are issued on one scene in
     * order (sample_begin = the previous pass's sample_end, the first at 0) with the same camera,
     * light, size, spp, depth, seed and shard, and no other render of the scene in between; the
     * scene keeps the frame's per-sample radiance rows and work list between them (GI_ERR_ARG
     * otherwise).  gi_render: whole-frame bands only (band_rows 0 or >= h). */
    int32_t sample_begin;
    int32_t sample_end;
} gi_opts;

/* stats[] slots */
#define GI_STAT_RAYS 0        /* rays traced (primary + bounce + shadow) */
#define GI_STAT_NODES 1       /* octree node records fetched & tested; Mode X queries answered from the flat
                                 leaf table (small LDS-resident scenes): the 256-byte units of table a
                                 query reads, so nodes x the node size stays a byte count */
#define GI_STAT_PRIMS 2       /* primitive records fetched & tested in fp64 */
#define GI_STAT_PIXELS 3
#define GI_STAT_X_PATH_MAX 4  /* Mode X: the longest sample path (primary ray to its end), a maximum:
                                 (ticks of the device's 100 MHz constant clock << 32) | (wave loop
                                 iterations << 16) | (that lane's traversal steps), both <= 65535 */
#define GI_STAT_X_ITERS 5     /* Mode X: wave loop iterations (per wave) */
#define GI_STAT_X_TRAV 6      /* Mode X: lane traversal steps (sum of active lanes over iterations) */
#define GI_STAT_X_HANDLE 7    /* Mode X: shading-handler executions (per wave) */
#define GI_STAT_X_HLANES 8    /* Mode X: lanes running the handler (sum over executions) */
#define GI_STAT_X_HCLOSE 9    /* Mode X: of those, lanes consuming a closest hit */
#define GI_STAT_X_HSHADOW 10  /* Mode X: of those, lanes consuming a shadow query */
#define GI_STAT_X_CYC_TRAV 11 /* Mode X: wave clock cycles in traversal steps */
#define GI_STAT_X_CYC_HIT 12  /* Mode X: wave clock cycles consuming finished rays (shading) */
#define GI_STAT_X_CYC_NEXT 13 /* Mode X: wave clock cycles starting rays (raygen, pixel fetch, root test) */
#define GI_STAT_X_CYC_ALL 14  /* Mode X: wave clock cycles in the whole loop */
#define GI_STAT_X_RESOLVED 15 /* Mode X: primary samples resolved without traversal (pixel-frustum classify
                                 and root-box pretest misses; each still adds exactly +0, as traced) */
/* Mode X divergence profile (wave-level): loop iterations in which some lane ran a node test (IT_NODE)
   and the lane node tests (LN_NODE); the same for leaf tests, inline bounce restarts (RS) and passes of
   the handler's ray-start loop (ST: lanes = lanes in the handler during the pass) */
#define GI_STAT_X_IT_NODE 16
#define GI_STAT_X_LN_NODE 17
#define GI_STAT_X_IT_LEAF 18
#define GI_STAT_X_LN_LEAF 19
#define GI_STAT_X_IT_RS 20
#define GI_STAT_X_LN_RS 21
#define GI_STAT_X_IT_ST 22
#define GI_STAT_X_LN_ST 23
#define GI_STAT_R_PAIRS 24      /* Mode R flat phases: candidate pairs (pixel, entity) the walk stored */
#define GI_STAT_R_OVF_TILES 25  /* Mode R flat phases: tiles whose candidates did not fit the pair
                                   buffer, rendered by the fallback kernel (k_mode_r_batch) instead */
#define GI_STATS_N 26

#define GI_TILE 8             /* shard granularity: 8x8 pixel tiles, dealt round-robin to ranks */

typedef struct gi_scene gi_scene;

typedef struct gi_scene_info {
    int32_t n_entities;
    int32_t n_nodes;          /* reference octree nodes (Mode R) */
    int32_t n_leaves;
    int32_t max_depth;
    int32_t n_reachable;      /* entities referenced by at least one leaf */
    int32_t n_dropped;        /* entities whose bbox misses the root (A.14) */
    int32_t x_nodes;          /* Mode X octree nodes */
    int32_t x_prims;          /* Mode X primitives */
    int64_t device_bytes;     /* scene bytes resident in HBM */
    int32_t x_node_bytes;     /* Mode X traversal node record: 256 (XWNode) or 128 (quantised XCNode,
                                 large HBM-resident scenes) -- bench.py's algorithmic bytes per visit */
    int32_t x_lds_resident;   /* 1: Mode X stages the scene in LDS per workgroup */
    int32_t x_flat_leaves;    /* leaves of the Mode X flat leaf table (ABI 16) */
    int32_t x_fan_leaves;     /* ... that are fan pairs: the two halves of one planar convex quad, whose
                                 exact tests the flat query decides between by the first one's first step
                                 when every leaf is one (ABI 16) */
} gi_scene_info;

typedef struct gi_hit {
    int32_t entity;           /* -1: no hit */
    int32_t u, v;             /* getTextureCoord */
    double point[3], normal[3];
} gi_hit;

/* progressive-display callback: rgb8 rows [y0, y0+rows) of the frame are final */
typedef void (*gi_tile_cb)(void* user, int y0, int rows, const uint8_t* rgb8_rows, const double* rgb_rows);

int gi_abi_version(void);
const char* gi_last_error(void);
/* gfx950 devices visible to this process (0 when there is none). */
int gi_device_count(void);
/* Their HIP device indices (a node may mix architectures): min(count, cap) indices written to out
 * (out may be NULL when cap is 0); returns the count. */
int gi_device_list(int32_t* out, int cap);
/* Provenance: a hash of the kernel and host sources this library was compiled from (build.py
 * passes it at compile time; tests compare it with the sources in the tree). */
const char* gi_build_id(void);

int gi_camera_init(const double pos[3], const double look_at[3], double focal, gi_camera* out);

/* Builds the reference octree and the Mode X acceleration structure on the host and uploads the
 * scene to the current HIP device (the scene is bound to that device).
 *
 * Coordinate range.  Supported are scenes whose geometry, with the acceleration structure's padding of
 * 1e-5 max(1, max |coordinate|), lies within |coordinate| <= 3.4e8 (FLT_MAX / 1e30: the kernels' fp32
 * box tests clamp a ray's reciprocal direction to +-1e30, and beyond that range the tests of
 * axis-parallel rays that start inside the scene overflow and cull what the rays hit).  A scene
 * beyond it is refused here -- GI_ERR_SCENE, gi_last_error() names the limit -- so neither mode
 * renders it and no ray query, feature buffer, adaptive pass or test hook can be asked of it.  Inside
 * the range Mode X answers are exact at any scale and placement, and rays may start at any distance.
 * Speed is not uniform over it: the padding grows with the distance from the world origin, not
 * with the scene's size, so a small scene far from the origin (or one much smaller than 1) traverses
 * more nodes per ray (DESIGN.md §5 "Scale and placement"). */
int gi_scene_create(const gi_scene_desc* desc, gi_scene** out);
void gi_scene_destroy(gi_scene* scene);
int gi_scene_get_info(const gi_scene* scene, gi_scene_info* info);

/* Renders a w x h frame into host buffers (rgb: w*h*3 fp64, rgb8: w*h*3 RGB888; either may be
 * NULL).  Polls *cancel (if non-NULL) between bands; calls cb (if non-NULL) after each band.
 * Threading: a scene may be used from any host thread; calls on one scene are serialised by the
 * library (a mutex for the host side, and every render of a scene is ordered on the device behind
 * the scene's previous one, whatever stream each was issued on: they share the Mode X work list). */
int gi_render(gi_scene* scene, const gi_camera* cam, const double light[3], int w, int h,
              const gi_opts* opts, double* rgb, uint8_t* rgb8, const volatile int* cancel,
              gi_tile_cb cb, void* user);

/* Device-resident variant, asynchronous on `stream` (hipStream_t; NULL = default stream).
 * shard_count == 1: d_rgb / d_rgb8 are row-major frames.  shard_count > 1: they hold this rank's
 * tiles packed as [gi_shard_tiles(w,h,n)][GI_TILE*GI_TILE][3], tile t = shard_index + k*n. */
int gi_render_device(gi_scene* scene, const gi_camera* cam, const double light[3], int w, int h,
                     const gi_opts* opts, double* d_rgb, uint8_t* d_rgb8, void* stream);

/* Tiles per rank (the packed buffer of every rank has this many tiles, padded). */
int64_t gi_shard_tiles(int w, int h, int shard_count);

/* d_packed: shard_count consecutive per-rank packed buffers (as gathered); writes row-major frames. */
int gi_unshard_device(int w, int h, int shard_count, const double* d_packed, const uint8_t* d_packed8,
                      double* d_rgb, uint8_t* d_rgb8, void* stream);

/* One ray through the Mode R per-pixel body (raytracer.h:43-82) on the device: origin, dir (the
 * Ray ctor normalises it), light.  rgb receives the shaded colour (0 if no hit). */
int gi_trace_ray(gi_scene* scene, const double origin[3], const double dir[3], const double light[3],
                 gi_hit* hit, double rgb[3]);

/* ---- batched ray queries (ABI 12) ------------------------------------------------------------
 * What does this ray hit?  n rays against the scene's Mode X acceleration structure, answered by the
 * kernel variant a Mode X render of the scene runs (gi_kat_x_variant(scene, 0, ...) describes it).
 *
 * A ray is GI_RAY_DOUBLES = 8 doubles (64 bytes): o[3], d[3], tmax, reserved.  d is used as given: it
 * is not normalised, and t is in units of d.  tmax may be +inf.  reserved is ignored.
 *
 * gi_intersect*: the closest hit -- the (t, primitive) minimum over t in (1e-7, tmax), ties to the
 * lower primitive index.  gi_occluded*: any hit -- occluded = 1 when some primitive has t in
 * (1e-7, tmax), else 0.
 *   Range of t   open on both sides: a tmax equal to the closest hit's t is a miss (the strictness
 *                the renders' own queries have).  tmax <= 1e-7 is a miss by the interval alone.
 *   prim         Mode X's primitive numbering, as gi_kat_x_query documents it: entities in push
 *                order, a meshed entity (ExpQuad, ExpCube, ...) as its triangles.
 *   entity       that primitive's entity (push order).
 *   normal       n*3: the unit geometric normal at the hit, flipped to face the ray (dot(d, normal)
 *                <= 0) -- the normal Mode X shades with.
 *   Miss         prim = entity = -1, t = +inf, normal = (0, 0, 0).
 *   Outputs      any output pointer of gi_intersect* may be NULL and is then not written; all four
 *                NULL is GI_ERR_ARG.
 *   Malformed    a ray with a non-finite component of o or d, a zero d or a NaN tmax is screened
 *                before any traversal and reported as a miss (occluded = 0); the other rays of the
 *                call are not affected.
 *   Arguments    n == 0 launches nothing and returns GI_OK; n < 0 is GI_ERR_ARG; NULL rays with
 *                n > 0 is GI_ERR_ARG.  Device ray records are 16-byte aligned (GI_ERR_ARG otherwise).
 * The _device variants take device pointers and are asynchronous on `stream` (hipStream_t; NULL =
 * default stream): they make no allocation, no host synchronisation and no copy.  gi_intersect and
 * gi_occluded do the same from / into host buffers (stage, launch, copy back) and are synchronous.
 * Scene state: the queries read only the scene's immutable records.  They touch none of the scene's
 * Mode X scratch (work list, counters, per-sample radiance rows) and are not ordered against the
 * scene's renders, so they may run concurrently with a render and with each other on any streams,
 * and a query between two progressive passes (gi_opts sample_begin / sample_end) does not end the
 * progressive frame. */
#define GI_RAY_DOUBLES 8
int gi_intersect_device(gi_scene* scene, int64_t n, const double* d_rays, double* d_t, int32_t* d_prim,
                        int32_t* d_entity, double* d_normal, void* stream);
int gi_occluded_device(gi_scene* scene, int64_t n, const double* d_rays, int32_t* d_occluded, void* stream);
int gi_intersect(gi_scene* scene, int64_t n, const double* rays, double* t, int32_t* prim, int32_t* entity,
                 double* normal);
int gi_occluded(gi_scene* scene, int64_t n, const double* rays, int32_t* occluded);

/* ---- first-hit feature buffers (AOVs) and camera rays (ABI 13) ----------------------------------
 * What does this pixel show?  For every pixel of the window [x0, x1) x [y0, y1) of a w x h frame, the
 * first surface its primary ray meets, answered by the kernel variant a Mode X render of the scene runs
 * (gi_kat_x_variant(scene, 0, ...) describes it).
 *
 * The pixel's ray is the primary ray of a 1-spp Mode X frame, formed by the functions the render
 * kernels use: o = cam.pos, d = normalize(top_left - left*x*res - up*y*res) (raytracer.h:41-43) at the
 * pixel's integer (x, y), without jitter.  The closest hit is the (t, primitive) minimum over t > 1e-7,
 * ties to the lower primitive index -- gi_intersect's answer for that ray with tmax = +inf.
 *
 * gi_aov: one device (gi_render_aov_device) or host (gi_render_aov) pointer per output, each a
 * row-major plane over the window (rows = y1 - y0, cols = x1 - x0; pixel (x, y) at index
 * (y - y0) * cols + (x - x0)):
 *   t        rows*cols fp64: the distance along the unit d, i.e. the Euclidean distance from the
 *            camera position; +inf without a hit.
 *   normal   rows*cols*3 fp64: the unit geometric normal at the hit, flipped to face the ray
 *            (dot(d, normal) < 0) -- the normal Mode X shades with, gi_intersect's; (0, 0, 0) without
 *            a hit.
 *   albedo   rows*cols*3 fp64: the texel of the hit entity's material colour at (u, v) (the
 *            reference's 32 x 32 checker pattern, material.h:48-62) -- the colour Mode X shades with
 *            and multiplies a diffuse path's throughput by (T *= albedo / 2); (0, 0, 0) without a hit.
 *   prim     rows*cols int32: Mode X's primitive index, as gi_intersect numbers them; -1 without a hit.
 *   entity   rows*cols int32: that primitive's entity (push order); -1 without a hit.
 *   uv       rows*cols*2 int32: the entity's getTextureCoord at the hit point P = o + t d, as Mode X
 *            computes it; (0, 0) without a hit.
 *   Outputs    any pointer may be NULL and is then not written; all six NULL is GI_ERR_ARG.
 *   Arguments  GI_ERR_ARG for a NULL scene, camera, frame or gi_aov; for w <= 0 or h <= 0 (or more
 *              than 2^34 pixels); for a window that is reversed (x0 > x1, y0 > y1) or not inside the
 *              frame; for a camera with a non-finite field.  An empty window (x0 == x1 or y0 == y1)
 *              launches nothing and returns GI_OK.
 * gi_camera_rays*: the same window's pixel rays as GI_RAY_DOUBLES records, row-major over the window:
 * o, the same normalised d bit for bit, tmax = +inf, reserved = 0 -- ready for gi_intersect_device /
 * gi_occluded_device (gi_intersect over them returns the t, prim, entity and normal planes above).  No
 * scene: they run on the current HIP device.  A NULL ray buffer is GI_ERR_ARG; device ray records are
 * 16-byte aligned (GI_ERR_ARG otherwise).
 * The _device variants take device pointers and are asynchronous on `stream` (hipStream_t; NULL =
 * default stream): they make no allocation, no host synchronisation and no copy.  gi_render_aov and
 * gi_camera_rays do the same from / into host buffers (stage, launch, copy back) and are synchronous.
 * Scene state: as the ray queries -- only the scene's immutable records are read, none of its Mode X
 * scratch is touched, the calls are not ordered against the scene's renders, and a call between two
 * progressive passes does not end the progressive frame.
 * Not provided: jittered or per-sample feature buffers (one unjittered ray per pixel); Mode R's
 * last-hit-wins choice (gi_trace_ray serves it); shard packing / gi_multi (a whole frame is one coherent
 * ray per pixel on one device). */
typedef struct gi_aov_frame { int32_t w, h, x0, y0, x1, y1; } gi_aov_frame;   /* window of a w x h frame */
typedef struct gi_aov { double* t; double* normal; double* albedo; int32_t* prim; int32_t* entity; int32_t* uv; } gi_aov;
int gi_render_aov_device(gi_scene* scene, const gi_camera* cam, const gi_aov_frame* frame, const gi_aov* d_out,
                         void* stream);
int gi_render_aov(gi_scene* scene, const gi_camera* cam, const gi_aov_frame* frame, const gi_aov* out);
int gi_camera_rays_device(const gi_camera* cam, const gi_aov_frame* frame, double* d_rays, void* stream);
int gi_camera_rays(const gi_camera* cam, const gi_aov_frame* frame, double* rays);

/* ---- denoiser: an edge-avoiding a-trous filter over the feature buffers (ABI 17) ----------------
 * A preview of a noisy frame -- the first passes of a progressive Mode X frame -- from the frame and the
 * t, normal and albedo planes of gi_render_aov* for the same camera and window.  No scene: like
 * gi_camera_rays* the calls run on the current HIP device.  All planes are row-major over the window
 * [x0, x1) x [y0, y1) of the w x h frame; the camera and the frame are needed because the plane stop
 * uses the pixels' hit positions.
 *
 * The filter, exactly.  Everything is fp64, no operation is contracted, dots are summed as
 * (x x' + y y') + z z'.  Per valid pixel p (t_p < +inf) at absolute pixel (x, y):
 *   d_p = normalize(primary_dir(cam, x, y))  (gi_camera_rays' d),  P_p = cam.pos + t_p d_p (per component
 *   one multiply, then one add),  s_p = sigma_p t_p,  c^0 = rgb.
 * Level i = 0 .. levels-1 has step s = 2^i and sigma2 = (sigma_c 2^-i)^2 (ldexp, then one multiply):
 *   sum_w = 0; sum_c = (0, 0, 0)
 *   for dy = -2..2 (outer), dx = -2..2 (inner), sums sequential in this order:
 *       q = p + s (dx, dy); skipped if q is outside the window, or invalid, or (GI_DENOISE_ALBEDO_STOP and
 *                           not albedo_q == albedo_p in all three doubles)
 *       k   = H[dx+2] H[dy+2],  H = {1/16, 1/4, 3/8, 1/4, 1/16}
 *       w_n = max(n_p . n_q, 0), squared normal_pow_log2 times
 *       w_p = max(1 - |n_p . (P_q - P_p)| / s_p, 0)
 *       e   = c_p - c_q;  w_c = 1 / (1 + ((e.r e.r + e.g e.g) + e.b e.b) / sigma2)
 *       wt  = ((k w_n) w_p) w_c;  sum_w += wt;  sum_c += wt c_q
 *   c^{i+1}_p = sum_c / sum_w        (the centre tap always counts)
 * max(v, 0) is v > 0 ? v : 0.  Invalid pixels (t = +inf) pass through every level unchanged and are never
 * taps.  After the last level out_rgb = min(c, 1) (c < 1 ? c : 1) and out_rgb8 = quantize(out_rgb), the
 * frames' (int)(255 c).  No transcendental function appears: a restatement with the same order is exact.
 *
 * The caller's planes are trusted: a non-finite value in a valid pixel (or a t <= 0, a normal that is
 * not a unit vector) gives unspecified pixels, never a fault.
 * sigma_c: about 0.5 / sqrt(samples accumulated so far) (README.md "Denoiser").
 * The _device form takes device pointers and is asynchronous on `stream` (hipStream_t; NULL = default
 * stream): it makes no allocation, no copy and no host synchronisation; the caller owns the scratch
 * (gi_denoise_scratch_bytes bytes, 16-byte aligned), which no other work may use until the call's
 * launches have run.  gi_denoise does the same from / into host buffers (stage, launch, copy back) and
 * is synchronous.
 *   Arguments  GI_ERR_ARG for a NULL cam, frame, p or io; a NULL rgb, t or normal; both outputs NULL; a
 *              NULL albedo with GI_DENOISE_ALBEDO_STOP; levels outside 1..8, normal_pow_log2 outside 0..7,
 *              a sigma_c or sigma_p that is not > 0 (NaN included; +inf is allowed), an unknown flag, a
 *              non-zero reserved; a bad frame or window and a camera with a non-finite field, as
 *              gi_render_aov judges them; out_rgb equal to rgb; scratch_bytes below
 *              gi_denoise_scratch_bytes, a NULL or not 16-byte aligned device scratch.  An empty window
 *              launches nothing and returns GI_OK.  gi_denoise_scratch_bytes (host only, no device): the
 *              bytes, or a negative gi_status for a bad frame or parameters (0 for an empty window).
 * Not provided: albedo demodulation, Mode R frames, shard-packed buffers / gi_multi (a per-pixel colour stop
 * from the samples' variance: gi_denoise_var* below; accumulation over frames: gi_temporal* below). */
#define GI_DENOISE_ALBEDO_STOP 1u  /* a tap contributes only if its albedo equals the centre's (three fp64 ==) */
typedef struct gi_denoise_params {
    int32_t levels;           /* 1..8 a-trous levels, level i has step 2^i */
    int32_t normal_pow_log2;  /* 0..7: w_n = max(n_p.n_q, 0)^(2^k), by k squarings */
    uint32_t flags;           /* GI_DENOISE_* */
    int32_t reserved;         /* 0 */
    double sigma_c;           /* > 0, +inf = no colour stop; level i uses sigma_c * 2^-i */
    double sigma_p;           /* > 0, +inf = no plane stop; plane distance in units of the centre's t */
} gi_denoise_params;
typedef struct gi_denoise_io {
    const double* rgb;        /* rows*cols*3: the frame to filter (gi_render_device's layout over the window) */
    const double* t;          /* rows*cols: gi_aov.t; a pixel is valid iff t < +inf */
    const double* normal;     /* rows*cols*3: gi_aov.normal */
    const double* albedo;     /* rows*cols*3: gi_aov.albedo; may be NULL without GI_DENOISE_ALBEDO_STOP */
    double* out_rgb;          /* rows*cols*3, may be NULL */
    uint8_t* out_rgb8;        /* rows*cols*3, may be NULL; quantize() of out_rgb (gi_math.h) */
} gi_denoise_io;
int64_t gi_denoise_scratch_bytes(const gi_aov_frame* frame, const gi_denoise_params* p);
int gi_denoise_device(const gi_camera* cam, const gi_aov_frame* frame, const gi_denoise_params* p,
                      const gi_denoise_io* d_io, void* d_scratch, int64_t scratch_bytes, void* stream);
int gi_denoise(const gi_camera* cam, const gi_aov_frame* frame, const gi_denoise_params* p, const gi_denoise_io* io);

/* ---- sample moments of the retained Mode X frame (ABI 18) -----------------------------------------
 * How noisy is each pixel?  For spp > 1 every Mode X form keeps each listed pixel's per-sample radiance rows in
 * the scene's scratch; these calls read them back as per-pixel moments.
 *
 * The retained frame is the scene's last render if that render was Mode X with spp > 1 and shard_count == 1,
 * a whole frame (gi_render_device, or gi_render with one band: band_rows 0 or >= h), and was issued
 * successfully; n is the number of samples rendered so far -- the last pass's sample_end, or spp for a one-shot
 * frame.  Any other render of the scene (Mode R, spp == 1, sharded or banded ones included) and a failed render
 * clear the record.  gi_frame_samples_info (host only) reports the retained frame's w, h, n and spp (any pointer
 * may be NULL); GI_ERR_ARG without a retained frame.
 *
 * Outputs: row-major planes over the window of `frame`, as gi_render_aov lays them out; frame->w and frame->h
 * must equal the retained frame's.  Per pixel, x_s is the radiance row of sample s < n: three doubles, unclamped.
 * A pixel the classify pass resolved without traversal has no row: x_s = +0 for all s.
 *   samples  rows*cols*n*3, [pixel][sample][3]: the rows themselves.
 *   mean     rows*cols*3: per channel sum = +0; sum = sum + x_s for s = 0 .. n-1 in order; mean = sum / (double)n.
 *            It is the render's own sum: min(mean, 1) is the delivered frame bit for bit.
 *   var      rows*cols*3: the sample variance OF THE MEAN, two-pass.  Per channel m2 = +0; for s = 0 .. n-1 in
 *            order d = x_s - mean, m2 = m2 + d d (one multiply, then one add, not contracted);
 *            var = (m2 / (double)(n-1)) / (double)n.
 *   Outputs    any pointer may be NULL and is then not written; all three NULL is GI_ERR_ARG.
 *   Arguments  GI_ERR_ARG for a NULL scene, frame or gi_moments; without a retained frame; for n < 2 (a first
 *              pass ending at sample 1); for a frame whose w, h are not the retained frame's, or a bad frame or
 *              window as gi_render_aov judges them.  An empty window launches nothing and returns GI_OK.
 * Ordering: unlike the ray queries these calls read the scene's Mode X scratch.  They run under the scene's
 * mutex and are ordered on the device with the scene's renders in both directions: behind the scene's previous
 * render, and the scene's next render (which overwrites the rows) behind them, whatever streams are used.  They
 * are not renders: nothing of the progressive-frame state is touched, and a call between two passes does not
 * end the frame.
 * gi_frame_moments_device takes device pointers and is asynchronous on `stream`: no allocation, no copy, no host
 * synchronisation.  gi_frame_moments does the same into host buffers (stage, launch, copy back), synchronous.
 * Not provided: sharded or banded frames, gi_multi, Mode R. */
typedef struct gi_moments { double* mean; double* var; double* samples; } gi_moments;
int gi_frame_samples_info(gi_scene* scene, int32_t* w, int32_t* h, int32_t* n, int32_t* spp);
int gi_frame_moments_device(gi_scene* scene, const gi_aov_frame* frame, const gi_moments* d_out, void* stream);
int gi_frame_moments(gi_scene* scene, const gi_aov_frame* frame, const gi_moments* out);

/* ---- variance-guided denoiser (ABI 18) -------------------------------------------------------------
 * gi_denoise's filter with the colour stop per pixel from the variance of the mean (gi_moments.var) instead of
 * one sigma_c for the frame.  Unchanged from gi_denoise: the fp64 rules, the window, validity and albedo-stop
 * rules, the 25 taps with dy outer and dx inner, H, w_n, w_p, the centre tap, the final min(c, 1) and quantize.
 * c^0 = rgb, V^0 = var.  At level i (step s = 2^i), for a valid pixel p:
 *   prefiltered variance   v_q = (V_q.r + V_q.g) + V_q.b;  sum_k = 0; sum_v = 0;
 *       for dy = -1..1 (outer), dx = -1..1 (inner): q = p + (dx, dy) -- step 1 at every level -- skipped if q is
 *       outside the window or invalid (no albedo test here); k = G[dx+1] G[dy+1], G = {1/4, 1/2, 1/4};
 *       sum_k += k; sum_v += k v_q.   g_p = sum_v / sum_k.
 *   per-pixel stop         sigma2_p = (sigma_v sigma_v) g_p + var_floor (two multiplies, then the add); where
 *       sigma_v sigma_v is +inf, sigma2_p = +inf whatever g_p is (no colour stop, also where g_p is 0).
 *       The level's w_c = 1 / (1 + e.e / sigma2_p): no 2^-i shrink, the variance falls by itself.
 *   variance propagation   beside sum_c += wt c_q, per channel sum_V += (wt wt) V_q;
 *       c^{i+1}_p = sum_c / sum_w,  V^{i+1}_p = sum_V / (sum_w sum_w).
 * Invalid pixels pass c and V through unchanged.  out_var = V^levels (not clamped).  The caller's planes are
 * trusted as in gi_denoise: a negative or non-finite var gives unspecified pixels, never a fault.
 * Defaults that serve the first passes of a Cornell-like frame: README.md "Sample moments / variance-guided
 * denoiser".  The _device and host forms, the scratch and the argument rules are gi_denoise's, with sigma_v in
 * sigma_c's place: GI_ERR_ARG also for a var_floor that is not finite and > 0, a NULL var, all three outputs
 * NULL, out_rgb equal to rgb or out_var equal to var.
 * Not provided: albedo demodulation, Mode R frames, shard-packed buffers / gi_multi (accumulation over frames:
 * gi_temporal* below). */
typedef struct gi_denoise_var_params {
    int32_t levels;           /* 1..8 */
    int32_t normal_pow_log2;  /* 0..7 */
    uint32_t flags;           /* GI_DENOISE_* */
    int32_t reserved;         /* 0 */
    double sigma_v;           /* > 0, +inf = no colour stop */
    double sigma_p;           /* > 0, +inf = no plane stop */
    double var_floor;         /* > 0, finite: added to every pixel's sigma2 */
} gi_denoise_var_params;
typedef struct gi_denoise_var_io {
    const double* rgb;        /* rows*cols*3: gi_moments.mean (or the frame) */
    const double* var;        /* rows*cols*3: gi_moments.var */
    const double* t;          /* rows*cols: gi_aov.t */
    const double* normal;     /* rows*cols*3: gi_aov.normal */
    const double* albedo;     /* rows*cols*3: gi_aov.albedo; may be NULL without GI_DENOISE_ALBEDO_STOP */
    double* out_rgb;          /* rows*cols*3, may be NULL */
    double* out_var;          /* rows*cols*3, may be NULL */
    uint8_t* out_rgb8;        /* rows*cols*3, may be NULL */
} gi_denoise_var_io;
int64_t gi_denoise_var_scratch_bytes(const gi_aov_frame* frame, const gi_denoise_var_params* p);
int gi_denoise_var_device(const gi_camera* cam, const gi_aov_frame* frame, const gi_denoise_var_params* p,
                          const gi_denoise_var_io* d_io, void* d_scratch, int64_t scratch_bytes, void* stream);
int gi_denoise_var(const gi_camera* cam, const gi_aov_frame* frame, const gi_denoise_var_params* p,
                   const gi_denoise_var_io* io);

/* ---- temporal accumulation: reproject the previous frame's history (ABI 20) --------------------------
 * More samples per pixel for a viewer whose camera moves over a static scene: the temporal stage of SVGF
 * (reproject, test, blend).  The previous frame's accumulated colour and variance are reprojected onto the
 * current frame's first hits and blended with the current frame (gi_moments.mean / var, or the frame).  No
 * scene, no state and no scratch: like gi_denoise* and gi_camera_rays* the calls run on the current HIP device;
 * the caller owns two sets of history planes (rgb, var, t, normal, prim, len) and swaps them each frame -- this
 * frame's outputs and its own t, normal and prim are the next frame's history.  `frame` is the window
 * [x0, x1) x [y0, y1) of the current w x h frame; the history planes cover the same window of the previous
 * frame, which has the same w and h.  All planes are row-major over the window, as gi_render_aov lays them
 * out.  d_hist == NULL (prev_cam may then be NULL) is the first frame: every valid pixel resets.
 *
 * The operation, exactly.  Everything is fp64, no operation is contracted, dots are summed as
 * (x x' + y y') + z z', every component of a cross product a x b is one subtraction of two products
 * (a.y b.z - b.y a.z, a.z b.x - b.z a.x, a.x b.y - b.x a.y).  c = cur.rgb_p, V = cur.var_p.  Per pixel p at
 * absolute pixel (x, y):
 *   invalid (t_p not < +inf):  out.rgb = c, out.var = V, out.len = 0.
 *   the point seen    d_p = normalize(primary_dir(cam, x, y)),  P = cam.pos + t_p d_p  (gi_denoise's P_p).
 *   where the previous camera saw it    with the previous camera's frame vectors as the renders make them for
 *       a frame of width w (left, up, top_left and the pixel pitches rx, ry; primary_dir(prev, x', y') =
 *       (top_left - (left x') rx) - (up y') ry):
 *       A = left rx,  B = up ry,  T = top_left,  N = A x B,  det = T . N,  v = P - prev.pos,  den = v . N,
 *       x' = -(v . (B x T)) / den,   y' = -(v . (T x A)) / den
 *       -- the inverse of primary_dir for any basis (up need not be orthogonal to forward).
 *   history exists only if  den det > 0  (the point lies in front of the previous camera),  x' and y' are
 *       finite, and fx = floor(x'), fy = floor(y') satisfy x0-1 <= fx <= x1-1 and y0-1 <= fy <= y1-1, compared
 *       as doubles before any conversion to an integer.
 *   four taps    wx = x' - fx,  wy = y' - fy;  sum_b = 0, sum_c = sum_V = (0, 0, 0), len_h = INT32_MAX;
 *       for j = 0, 1 (outer), i = 0, 1 (inner), sums sequential in this order:
 *       q = (fx + i, fy + j),  b = (i ? wx : 1 - wx) (j ? wy : 1 - wy);  the tap is skipped unless all of
 *           b > 0;  q inside the window;  hist.t_q < +inf;  hist.len_q >= 1;
 *           (GI_TEMPORAL_PRIM_STOP) hist.prim_q == cur.prim_p;
 *           n_p . n_q >= cos_min;
 *           |n_p . (P_q - P)| <= sigma_p t_p,  P_q = prev.pos + hist.t_q normalize(primary_dir(prev, q))
 *       hold (a NaN in a comparison skips the tap);  an accepted tap adds
 *           sum_b += b;  sum_c += b hist.rgb_q;  sum_V += b hist.var_q;  len_h = min(len_h, hist.len_q).
 *       The variance is interpolated linearly, as if the four taps were fully correlated: deliberately
 *       conservative (independent taps would give the smaller sum b^2 V_q / sum_b^2).
 *   blend    no accepted tap (or no history): the pixel resets, out.rgb = c, out.var = V, out.len = 1.
 *       Otherwise h_c = sum_c / sum_b,  h_V = sum_V / sum_b,  out.len = min(len_h + 1, max_history) (formed
 *       without overflow),  a = max(1 / (double)out.len, alpha_min)  (u > v ? u : v),
 *       out.rgb = ((1 - a) h_c) + (a c),   out.var = (((1 - a) (1 - a)) h_V) + ((a a) V).
 * Nothing is clamped (gi_denoise* clamps at the end).  Up to max_history samples the result is the running
 * mean of the reprojected frames, after that an exponential window.  No transcendental function appears: a
 * restatement with the same order is exact (tests/temporal_ref.py).
 *
 * The caller's planes are trusted as in gi_denoise: garbage values give unspecified pixels, never a fault;
 * hist.len and the prim planes are only compared and min'ed, never used as an index.
 * The _device form takes device pointers and is asynchronous on `stream` (hipStream_t; NULL = default
 * stream): it makes no allocation, no copy and no host synchronisation.  gi_temporal does the same from /
 * into host buffers (stage, launch, copy back) and is synchronous.
 *   Outputs    any pointer of gi_temporal_out may be NULL and is then not written.
 *   Arguments  GI_ERR_ARG for a NULL cam, frame, p, cur or out; a NULL prev_cam with a history; a NULL cur.rgb,
 *              cur.t or cur.normal; a NULL hist.rgb, hist.t, hist.normal or hist.len in a history; a NULL prim
 *              on either side with GI_TEMPORAL_PRIM_STOP; out.var set while cur.var is NULL, or while a history
 *              is given and hist.var is NULL; all three outputs NULL; an output pointer equal to a pointer of cur
 *              or hist (the taps gather: in place is not allowed); max_history < 1, alpha_min outside [0, 1],
 *              cos_min outside [-1, 1], a sigma_p that is not > 0 (+inf is allowed), a NaN in any of them, an
 *              unknown flag; a bad frame or window and a camera (either one) with a non-finite field, as
 *              gi_render_aov judges them.  An empty window launches nothing and returns GI_OK.
 * Defaults and what they do on the Cornell box: README.md "Temporal accumulation".
 * Not provided: albedo demodulation, a spatial variance estimate for short histories, motion of the scene itself
 * (static scenes: the camera moves), Mode R frames, shard-packed buffers / gi_multi, the C++ drop-in headers, an
 * RGB888 output (run gi_denoise* or quantise the plane). */
#define GI_TEMPORAL_PRIM_STOP 1u   /* a history tap counts only if its prim equals the pixel's */
typedef struct gi_temporal_params {
    int32_t max_history;   /* >= 1: out_len saturates here (an exponential window after that) */
    uint32_t flags;        /* GI_TEMPORAL_* */
    double alpha_min;      /* in [0, 1]: lower bound of the blend weight of the current frame */
    double cos_min;        /* in [-1, 1]: a tap needs n_p . n_q >= cos_min */
    double sigma_p;        /* > 0, +inf = no plane stop; plane distance in units of the pixel's t (gi_denoise's) */
} gi_temporal_params;
typedef struct gi_temporal_frame {      /* planes over the window, gi_render_aov's layout */
    const double* rgb;     /* rows*cols*3  cur: this frame (gi_moments.mean or the frame); hist: accumulated colour */
    const double* var;     /* rows*cols*3  variance of the mean; NULL in cur = no variance is carried */
    const double* t;       /* rows*cols    gi_aov.t; valid iff t < +inf */
    const double* normal;  /* rows*cols*3  gi_aov.normal */
    const int32_t* prim;   /* rows*cols    gi_aov.prim; may be NULL without GI_TEMPORAL_PRIM_STOP */
    const int32_t* len;    /* rows*cols    hist only: samples accumulated per pixel (0 = none); ignored in cur */
} gi_temporal_frame;
typedef struct gi_temporal_out { double* rgb; double* var; int32_t* len; } gi_temporal_out;
int gi_temporal_device(const gi_camera* cam, const gi_camera* prev_cam, const gi_aov_frame* frame,
                       const gi_temporal_params* p, const gi_temporal_frame* d_cur, const gi_temporal_frame* d_hist,
                       const gi_temporal_out* d_out, void* stream);
int gi_temporal(const gi_camera* cam, const gi_camera* prev_cam, const gi_aov_frame* frame,
                const gi_temporal_params* p, const gi_temporal_frame* cur, const gi_temporal_frame* hist,
                const gi_temporal_out* out);

/* ---- adaptive sampling: stop converged pixels between passes (ABI 21) ------------------------------
 * A Mode X frame rendered in sample passes, as the progressive passes of gi_opts render it, that stops tracing a
 * pixel once the variance of its mean is small enough.  One call is one pass of one adaptive frame, driven by the
 * gi_opts fields: mode = GI_MODE_X; spp is the frame's maximum number of samples; [sample_begin, sample_end) is this
 * pass, with sample_end - sample_begin >= 2 and sample_end <= spp; shard_count = 1.  The continuation rules are the
 * progressive passes' own: the first pass starts at 0 and each later pass begins where the last one ended, with the
 * same camera, light, size, spp, depth, seed, form flags and gi_adaptive_params, and no other render of the scene in
 * between (GI_ERR_ARG otherwise; a device error that surfaced since the previous pass: GI_ERR_DEVICE, and the frame
 * restarts at 0).  The form flags, GI_FLAG_STATS, GI_FLAG_TIME, GI_FLAG_X_NO_SHADOW and GI_FLAG_X_ALL_LEAVES work as
 * in a render: a pass hands the render kernels the list of the pixels still active and traces only those.
 *
 * The rule, exactly.  Everything is fp64, no operation is contracted.  Per pixel the state is S1[3], S2[3] (both +0
 * before sample 0) and n.  After a pass ending at e, for every pixel that was active in it: its radiance rows x of
 * that pass in sample order, per channel S1 = S1 + x, S2 = S2 + (x x); then n = e.  If n >= min_samples:
 *   per channel m = S1 / n,  v = ((S2 - S1 m) / (n-1)) / n,  then v = v > 0 ? v : 0 (a NaN v stays NaN);
 *   err = (v.r + v.g) + v.b;   thr = tol tol;
 *   GI_ADAPTIVE_RELATIVE:  y = (m.r + m.g) + m.b,  f = y > y_floor ? y : y_floor,  thr = (tol tol) (f f).
 * The pixel stops iff (n >= min_samples and err <= thr) or e == spp: a NaN never stops a pixel before spp.  A
 * stopped pixel is never traced again; its S1, n and var are final.  A pixel the classify pass resolved without
 * traversal has x = +0 throughout and stops at the first pass with e >= min_samples (or e == spp).
 * Outputs after every pass, for every pixel of the frame (row-major w*h planes): n; mean = S1 / n; var = the v
 * above at the pixel's n; rgb = min(mean, 1) (mean < 1 ? mean : 1 -- as the renders) and rgb8 = quantize(rgb).  S1
 * is the in-order sum from +0, so rgb of a pixel with n_p samples is the one-shot frame of spp = n_p at that pixel,
 * bit for bit.  var is ONE-PASS (from S1 and S2): it is not gi_frame_moments' two-pass value, though it estimates
 * the same quantity (equal where every operation is exact); cancellation can make S2 - S1 m slightly negative,
 * hence the clamp at 0.
 *
 * gi_render_adaptive_device takes device planes and is asynchronous on `stream`: it allocates nothing per call
 * beyond the scene's scratch grown on demand (as renders do), copies nothing and does not synchronise the host.
 * The count of active pixels lives on the device, and a pass over an empty list is a cheap no-op that still
 * delivers the planes: a caller may queue a fixed schedule of passes without reading anything back.
 * gi_render_adaptive does the same into host planes (stage, one pass, copy back) and is synchronous.
 * gi_adaptive_info is the one call that waits: it reports the adaptive frame's size, the samples issued so far (the
 * last pass's sample_end) and the pixels still active after it (any pointer may be NULL); GI_ERR_ARG without an
 * adaptive frame (none rendered, or another render of the scene since).
 * Scene state: an adaptive pass is a render and is ordered like one.  It clears the retained frame
 * (gi_frame_moments after it is GI_ERR_ARG: the rows of earlier passes are not kept).  A plain progressive pass
 * cannot continue an adaptive frame, nor the reverse; any plain render ends the adaptive frame.  The ray queries,
 * gi_render_aov*, the denoisers and gi_temporal* between passes do not end it.  With GI_FLAG_STATS every pass
 * counts the resolved pixels' samples of the pass, as a progressive pass does (they cost no traversal either way);
 * the traced rays are those of the active pixels alone.
 *   Arguments  GI_ERR_ARG for a NULL scene, camera, light, opts, params or out struct; every plane NULL;
 *              min_samples < 2; a tol that is NaN or <= 0 (+inf is allowed: everything stops at the first judged
 *              pass); with GI_ADAPTIVE_RELATIVE a y_floor that is not finite and > 0; an unknown flag; a mode
 *              other than GI_MODE_X; shard_count != 1; a pass of fewer than 2 samples or with sample_end > spp;
 *              a pass out of order or with a changed frame, as above.
 * Not provided: shards and gi_multi; banded gi_render; the C++ drop-in headers; passes of one sample; Mode R. */
#define GI_ADAPTIVE_RELATIVE 1u    /* the threshold scales with the pixel's brightness: thr = (tol tol) (f f) */
typedef struct gi_adaptive_params {
    int32_t min_samples;   /* >= 2: no pixel is judged before it has this many */
    uint32_t flags;        /* GI_ADAPTIVE_* */
    double tol;            /* > 0, +inf allowed: stop when the error estimate <= tol*tol (see above) */
    double y_floor;        /* RELATIVE only, > 0 finite */
} gi_adaptive_params;
typedef struct gi_adaptive_out {   /* row-major w*h planes, any may be NULL, all NULL = GI_ERR_ARG */
    double* rgb; uint8_t* rgb8;    /* delivered frame: min(mean, 1) and its quantize() */
    double* mean; double* var;     /* unclamped mean, variance of the mean at n */
    int32_t* n;                    /* samples this pixel has received so far */
} gi_adaptive_out;
int gi_render_adaptive_device(gi_scene* scene, const gi_camera* cam, const double light[3], int w, int h,
                              const gi_opts* opts, const gi_adaptive_params* params, const gi_adaptive_out* d_out,
                              void* stream);
int gi_render_adaptive(gi_scene* scene, const gi_camera* cam, const double light[3], int w, int h, const gi_opts* opts,
                       const gi_adaptive_params* params, const gi_adaptive_out* out);
int gi_adaptive_info(gi_scene* scene, int32_t* w, int32_t* h, int32_t* samples_done, int64_t* active);

/* ---- radiance along caller-supplied rays, sample rays, resolve (ABI 21: added functions only) ---------
 * What radiance arrives along this ray?  gi_radiance* runs Mode X's path tracer on n rays of the caller's:
 * every record is one path sample and yields one radiance row.  gi_sample_rays* writes the rays a render
 * traces for a frame's pixel samples (optionally through a thin lens) and gi_resolve_samples* turns rows into
 * pixels, so the three calls together are a renderer whose camera and sampling pattern the caller may replace.
 *
 * gi_radiance*.  rays: n records of GI_RAY_DOUBLES doubles as gi_intersect takes them (o[3], d[3], tmax,
 * reserved); tmax and reserved are ignored (a path's first ray has no far end).  ids: n gi_path_id records, or
 * NULL for stream = i, sample = 0.  rgb: n*3 fp64, the path's radiance L, unclamped.
 *   The path   the oracle's sample_mode_x from its first ray on: o as given and d = normalize(d) -- d IS
 *              normalised here, as the renders and gi_trace_ray do and unlike gi_intersect.  A caller who
 *              wants a render's bits passes the unnormalised pixel direction, as gi_sample_rays* writes it;
 *              gi_camera_rays' unit d is normalised a second time and may differ in the last place.
 *              Then the render's segment per bounce b = 0 .. depth-1: the closest hit over t > 1e-7, the
 *              shadow ray to `light`, the texel, Blinn-Phong, L += T * min(local, 1), the mirror choice on
 *              dim 4, else T *= texel / 2 (the path ends where T == 0) and the cosine-weighted direction on
 *              dims 2 and 3.  It is answered by the kernel variant a Mode X render of the scene runs.
 *   Random numbers  key = mx_key(seed, stream) and every draw is mx_u01k(key, sample, b, dim): stream takes the
 *              place of a render's pixel index y*w + x and sample that of its sample index.  The row of
 *              (stream, sample) over a render's own jittered primary ray is therefore the row that render
 *              writes for the sample (gi_frame_moments' samples plane), bit for bit, and with one sample per
 *              pixel min(row, 1) is the render's pixel.
 *   params     depth in [1, 65534] (bounce indices 0xFFFF and 0xFFFE belong to the jitter and the lens below);
 *              flags: GI_FLAG_X_NO_SHADOW only, as in a render; any other bit is GI_ERR_ARG.
 *   Malformed  a record with a non-finite component of o or d or a zero d is screened before any traversal
 *              and yields (0, 0, 0); the other records of the call are not affected.
 *   Arguments  GI_ERR_ARG for n < 0 or n >= 2^32 and for a NULL scene, rays, light, params or rgb (ids may be
 *              NULL); otherwise n == 0 launches nothing and returns GI_OK.  Device ray records are 16-byte
 *              aligned and device ids 8-byte aligned (GI_ERR_ARG otherwise).
 *   Scene state  as the ray queries: only the scene's immutable records are read, none of its Mode X scratch is
 *              touched, no device counter is used, the call is not ordered against the scene's renders, and a
 *              call between two progressive or adaptive passes ends neither frame.
 *
 * gi_sample_rays*.  For the window [x0, x1) x [y0, y1) of a w x h frame and the samples [sample_begin,
 * sample_end) of each of its pixels: one ray record and one gi_path_id per (pixel, sample), laid out
 * [window pixel, row-major][s - sample_begin]; either output may be NULL (both: GI_ERR_ARG).  No scene: it runs
 * on the current HIP device, like gi_camera_rays.  Everything is fp64, no operation is contracted, dots are
 * (x x' + y y') + z z'.  With left, up, top_left and res the renders' frame vectors (gi_render_aov above), per
 * pixel (x, y) and sample s:
 *   stream = y w + x;  key = mx_key(seed, stream);  id = (stream, s, 0)
 *   GI_SAMPLE_JITTER: jx = mx_u01k(key, s, 0xFFFF, 0), jy = mx_u01k(key, s, 0xFFFF, 1) -- what a render with
 *              spp > 1 draws; without the flag jx = jy = 0, a 1-spp render's ray
 *   d0 = (top_left - (left (x + jx)) res) - (up (y + jy)) res, NOT normalised
 *   aperture == 0:  o = pos, d = d0.  gi_radiance over these records is the render's rows bit for bit.
 *   aperture > 0:   (lx, ly) = mx_disk(mx_u01k(key, s, 0xFFFE, 0), mx_u01k(key, s, 0xFFFE, 1)), the concentric
 *              map of the unit square onto the unit disk that the cosine sampling uses;
 *              q = focus / ((d0.x f.x + d0.y f.y) + d0.z f.z) with f the camera's forward;
 *              F = pos + d0 q  (the point of the pinhole ray at distance `focus` along forward);
 *              o = (pos + left (aperture lx)) + up (aperture ly);   d = F - o.
 *   tmax = +inf, reserved = 0.
 *   Arguments  GI_ERR_ARG for a bad frame, window or camera as gi_render_aov judges them; a NULL params;
 *              sample_begin < 0 or sample_end < sample_begin; an aperture that is negative or not finite;
 *              aperture > 0 with a focus that is not finite and > 0; an unknown flag; reserved != 0; both outputs
 *              NULL; more than 2^32 - 1 records; device ray records that are not 16-byte aligned (ids: 8-byte).
 *              An empty window or an empty sample range launches nothing and returns GI_OK.
 *
 * gi_resolve_samples*.  rows: [n_pix][ns][3] fp64.  Per pixel and channel sum = +0, sum = sum + x_s in sample
 * order, mean = sum / (double)ns, rgb = mean < 1 ? mean : 1 and rgb8 = the renders' 8-bit quantisation of rgb:
 * the operations a render resolves its rows with.  Either output may be NULL (both: GI_ERR_ARG).  GI_ERR_ARG
 * for ns < 1, n_pix < 0, NULL rows with n_pix > 0, or an rgb that is the rows' own buffer; n_pix == 0 launches
 * nothing.  No scene.
 *
 * The _device variants take device pointers and are asynchronous on `stream` (hipStream_t; NULL = default
 * stream): they make no allocation, no host synchronisation and no copy.  The others do the same from / into
 * host buffers (stage, launch, copy back) and are synchronous.
 * Not provided: Mode R; shards and gi_multi; the C++ drop-in headers; GI_FLAG_STATS / GI_FLAG_TIME; a tmax on
 * the first ray; adaptive stopping; a retained frame (gi_frame_moments does not see these rows: the caller
 * has them). */
#define GI_SAMPLE_JITTER 1u   /* gi_sample_params.flags: jitter each sample inside its pixel, as a render with spp > 1 */
typedef struct gi_path_id { uint64_t stream; uint32_t sample; uint32_t reserved; } gi_path_id;
typedef struct gi_radiance_params { int32_t depth; uint32_t flags; uint64_t seed; } gi_radiance_params;
typedef struct gi_sample_params {
    uint64_t seed;
    int32_t sample_begin, sample_end;   /* the samples [sample_begin, sample_end) of every pixel */
    uint32_t flags;                     /* GI_SAMPLE_* */
    int32_t reserved;                   /* 0 */
    double aperture;                    /* lens radius, 0 = pinhole */
    double focus;                       /* aperture > 0: distance along forward of the plane in focus */
} gi_sample_params;
int gi_radiance_device(gi_scene* scene, int64_t n, const double* d_rays, const gi_path_id* d_ids, const double light[3],
                       const gi_radiance_params* params, double* d_rgb, void* stream);
int gi_radiance(gi_scene* scene, int64_t n, const double* rays, const gi_path_id* ids, const double light[3],
                const gi_radiance_params* params, double* rgb);
int gi_sample_rays_device(const gi_camera* cam, const gi_aov_frame* frame, const gi_sample_params* params,
                          double* d_rays, gi_path_id* d_ids, void* stream);
int gi_sample_rays(const gi_camera* cam, const gi_aov_frame* frame, const gi_sample_params* params, double* rays,
                   gi_path_id* ids);
int gi_resolve_samples_device(int64_t n_pix, int32_t ns, const double* d_rows, double* d_rgb, uint8_t* d_rgb8,
                              void* stream);
int gi_resolve_samples(int64_t n_pix, int32_t ns, const double* rows, double* rgb, uint8_t* rgb8);

/* Average duration in ms of the dominant kernel over the scene's renders issued with GI_FLAG_TIME
 * since the previous call (waits for the last one; *n = how many, may be NULL), then resets.
 * GI_ERR_ARG if there was none. */
int gi_scene_kernel_ms(gi_scene* scene, float* avg_ms, int64_t* n);
/* Mode X form a render of `scene` with `opts` would run (bench labels, tests): 0 = the persistent
 * path-state kernel k_mode_x, 1 = the wavefront form (k_wf_bounce once per bounce), 2 = the
 * segment-synchronous form (k_seg); Mode R: 0. */
int gi_scene_x_form(gi_scene* scene, const gi_opts* opts, int32_t* form);
/* Whether a render of `scene` with `opts` would refill k_seg's lanes from its per-wave ring of
 * prepared primary rays (ABI 14; bench labels, tests): 1 = the segment-synchronous form with the
 * ring -- chosen per scene where the ring's LDS does not lower the kernel's resident workgroups, unless
 * GI_SEG_RING=0 is set in the environment; 0 = k_seg's lanes make their own units, or another form
 * or mode runs.  Frames are the same bit for bit either way. */
int gi_scene_seg_ring(gi_scene* scene, const gi_opts* opts, int32_t* on);
/* The boundary leaves of the scene's flat leaf table and the leaves a render's shadow queries visit (ABI 19;
 * tests, bench labels).  *boundary_mask: bit k set when leaf k lies in a plane that has the whole scene on
 * one closed side.  *live_mask: bit k set when the shadow queries of a Mode X render with light[3] from
 * cam_pos[3] visit leaf k: every leaf of the table except the boundary leaves that have the light on the
 * scene's side, farther from their plane than the scene's bound -- no shadow ray toward that
 * light can cross them.  Every leaf for a camera farther out than 16 scene extents.  Both 0 for a scene that
 * does not answer its queries from the table.  GI_FLAG_X_ALL_LEAVES and GI_FLAG_X_NO_SHADOW renders visit
 * every leaf (the latter traces no shadow ray). */
int gi_scene_shadow_leaves(gi_scene* scene, const double* light, const double* cam_pos, uint32_t* boundary_mask,
                           uint32_t* live_mask);
/* Mode R kernel a render of `scene` with `opts` would run (ABI 10; bench labels, tests): 0 = k_mode_r
 * (one lane per pixel: small scenes, GI_FLAG_R_DFS), 1 = the flat phases (k_rf_walk, k_rf_hit,
 * k_rf_scan, k_rf_reach, k_rf_shade; scenes of more than 4096 entities; their overflowed tiles by
 * k_mode_r_batch), 2 = k_mode_r_batch for the whole frame -- also where the flat phases' buffers
 * could not be allocated for the scene's last frame size (not retried for that size or larger).
 * Mode X: 0. */
int gi_scene_r_kernel(gi_scene* scene, const gi_opts* opts, int32_t* kernel);

/* ---- host-side reference octree (no device needed) --------------------------------------------
 * gi_octree_create builds the reference octree from the same descriptors as gi_scene_create (push
 * order, node boxes, lost entities A.6, silent drop A.14 -- bit for bit the reference's tree).
 * gi_octree_intersect returns Octree::intersect(Ray(origin, dir))'s candidate list: DFS over the
 * children 0..7, a child skipped when its list is empty (octree.h:140), else tested by the ExpBox
 * node test (A.4) and descended; leaves contribute their lists; duplicates kept.  `dir` is used as
 * given (the reference's Ray ctor has already normalised it, ray.h:6).  Entity indices are push
 * order; min(*n, cap) of them are written to out, *n = the full length. */
typedef struct gi_octree gi_octree;
int gi_octree_create(const gi_scene_desc* desc, gi_octree** out);
void gi_octree_destroy(gi_octree* octree);
int gi_octree_intersect(const gi_octree* octree, const double origin[3], const double dir[3], int32_t* out,
                        int64_t cap, int64_t* n);

/* ---- several GPUs of one process ------------------------------------------------------------
 * gi_multi_create: n_shards >= 1 shards, shard i rendered on HIP device devices[i] (duplicates
 * allowed: several shards on one device render one after the other).  devices[0] is the root that
 * assembles the frame.  The frame's 8x8 tiles are dealt round-robin over the shards (tile t ->
 * shard t % n_shards, as gi_render_device's shard_count/shard_index); each shard renders its tiles
 * into a packed buffer on its device, and one RCCL group of ncclSend/ncclRecv (rccl.h:700-725;
 * librccl is loaded when a second device is used) brings them to the root over xGMI, where
 * gi_unshard_device's kernel reassembles the frame.  Shards on the root device need no copy.
 * gi_multi_render: as gi_render (bands, cancel, callback, host buffers); opts->shard_count and
 * shard_index must be 1 and 0 (the multi handle does the sharding).  Results are bit-identical to
 * gi_render on one device. */
typedef struct gi_multi gi_multi;
int gi_multi_create(const gi_scene_desc* desc, int n_shards, const int* devices, gi_multi** out);
void gi_multi_destroy(gi_multi* multi);
int gi_multi_info(const gi_multi* multi, int* n_shards, int* n_devices, int* uses_rccl);
int gi_multi_render(gi_multi* multi, const gi_camera* cam, const double light[3], int w, int h, const gi_opts* opts,
                    double* rgb, uint8_t* rgb8, const volatile int* cancel, gi_tile_cb cb, void* user);

/* ---- scene I/O --------------------------------------------------------------------------------
 * gi_obj_parse: Wavefront OBJ text (len bytes, need not be terminated) -> GI_IMP_TRIANGLE
 * descriptors, one per triangle of each face's fan (v0, v_k, v_k+1) in file order, args = the three
 * vertices.  Each descriptor is a copy of *tmpl (its material fields; NULL: zeroed, i.e. the
 * reference's default ImpTriangle material) with kind and args set.  Accepts v (extra values
 * ignored), f with i, i/t, i//n, i/t/n references (1-based, negative = relative), comments and
 * '\' continuations; vt, vn, vp, o, g, s, usemtl, mtllib, l, p are skipped.  min(*n, cap)
 * descriptors are written to out, *n = the full count (call with cap = 0 to size the buffer).
 * GI_ERR_ARG with the line number on a malformed v / f line or a vertex reference out of range. */
int gi_obj_parse(const char* text, int64_t len, const gi_entity_desc* tmpl, gi_entity_desc* out, int64_t cap,
                 int64_t* n);

/* Known-answer hook: the device's ExpBox node test (entities.h:379-440 as octree.h:141-146 uses
 * it) over n host records (min[3], max[3], origin[3], dir[3]); out[i] = 0/1. */
int gi_kat_expbox(int n, const double* recs, int32_t* out);

/* Known-answer hooks (TEST hooks): Mode R's primitive tests record by record, through the functions
 * the Mode R kernels call.  n host records; dir is normalised as the reference's Ray constructor does
 * (ray.h:6); hit[i] = 0/1; pn[6 i ..] = the point and normal, zeros on a miss.  kind:
 *   GI_KAT_R_TRI    15 doubles p1 p2 p3 o dir: the builder's triangle record (its normal, centre and fp32
 *                   edges, made on the host) through the prefiltered ImpTriangle test ent_hit calls;
 *   GI_KAT_R_SPHERE 10 doubles pos radius o dir: ImpSphere::intersect, the radius narrowed to float;
 *   GI_KAT_R_BOX    12 doubles min max o dir: the ExpBox node test of one lane (gi_kat_expbox's);
 *   GI_KAT_R_BOX4   the same records, each held by 4 consecutive lanes and decided by the grouped
 *                   node test of the flat Mode R phases (3 of the 12 faces per lane, a ballot).
 * pn is written for triangles and spheres only (may be NULL for boxes).  n = 0 launches nothing. */
#define GI_KAT_R_TRI 0
#define GI_KAT_R_SPHERE 1
#define GI_KAT_R_BOX 2
#define GI_KAT_R_BOX4 3
int gi_kat_r_prims(int kind, int n, const double* recs, int32_t* hit, double* pn);

/* Known-answer hook (a TEST hook): n host rays (o[3], dir[3]; dir normalised here) each against every
 * entity of the scene through the Mode R kernels' entity test, in the instantiation they use for this
 * scene.  hit[i * E + k] = 0/1 and pn[6 (i * E + k) ..] = the point and normal of ray i on entity k
 * (E entities in push order): both start as zeros and are stored as Entity::intersect leaves them (the
 * triangle groups overwrite them on a miss, entities.h:616-617).  No texture coordinates. */
int gi_kat_r_entities(gi_scene* s, int n, const double* rays, int32_t* hit, double* pn);

/* Known-answer hook (a TEST hook; ABI 11): the Mode X device queries ray by ray.  n host records of
 * 12 doubles -- o[3], d[3], light[3], d2[3]; d and d2 are used as given -- each run as one path
 * segment's three queries by the kernel variant the segment form (k_seg) runs for this scene, the
 * scene staged as k_seg stages it, through the functions a k_seg segment itself calls for its queries,
 * its hit frame and its own-plane skip rule (not a copy of them):
 *   prim1, t1 : the closest hit of the ray (o, d): primitive index (entities in push order, an
 *               ExpQuad as its 2 triangles) and distance; -1 and +inf without a hit;
 *   occl      : from the hit point P = o + t1 d, 1 / 0 whether anything lies between P and `light`
 *               (-1 without a hit); skip_s: the plane group this shadow ray skipped (254: none);
 *   prim2, t2 : the closest hit of the ray (P, d2); skip2: the plane group it skipped.
 * *skip_cos (may be NULL): the own-plane skip's bound on |d . n| for a camera at cam_pos.
 * flags: bit 0 walks the tree where the scene's flat leaf table would apply (as GI_X_FLAT=0); bit 1
 * runs the HBM-resident variant on a scene that is staged in LDS.  n = 0 launches nothing. */
int gi_kat_x_query(gi_scene* scene, int n, const double* recs, const double cam_pos[3], int flags, int32_t* prim1,
                   double* t1, int32_t* occl, int32_t* skip_s, int32_t* prim2, double* t2, int32_t* skip2,
                   double* skip_cos);
/* The kernel variant gi_kat_x_query runs for these flags -- with flags 0 the segment form's own for
 * this scene: out[0..5] = 1/0 for LDS (scene staged in LDS), W4 (4 waves per SIMD), SH (level masks
 * in one word: trees of at most 8 levels), TRI (triangles only), CN (quantised nodes), FLAT (the flat
 * leaf table answers the queries). */
int gi_kat_x_variant(gi_scene* scene, int flags, int32_t out[6]);

/* Known-answer hook (a TEST hook; ABI 15): the texel Mode X's segment kernels shade a hit with.  n host
 * records of 4 doubles -- the entity's index (push order, an integer in [0, entity count)) and a point
 * taken as the hit point on it.  mode 0 runs the shading helper itself (an fp32 filter decides the
 * checker's colour where it is sure, the exact texture-coordinate code everywhere else); mode 1 the
 * exact code alone.  texel: 3 doubles per record.  how[i]: 1 the filter decided the record, 2 it went
 * to the exact code, 0 neither was needed (a triangle whose truncated colour is (1, 1, 1)); mode 1: 2.
 * GI_ERR_ARG for an entity index out of range or another mode.  n = 0 launches nothing. */
int gi_kat_x_texel(gi_scene* scene, int n, const double* recs, int mode, double* texel, int32_t* how);

#ifdef __cplusplus
}
#endif
#endif /* GI_H_ */
