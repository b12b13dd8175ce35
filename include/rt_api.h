/*
 * rt_api.h — C ABI of the MI355X-native renderer core (librtgo.so).
 *
 * Drop-in boundary for the per-pixel ray-trace hot path of
 * JoshElkind/concurrent-raytracer-go.  The reference has no FFI; its seam is
 * the Go method set of *renderer.ParallelRenderer, called only from
 * cmd/raytracer/main.go:40-69.  Each entry point below names the reference
 * symbol (file:line, relative to the reference root) it replaces.
 *
 * Conventions:
 *   - every function returns 0 (RT_OK) on success and a negative RT_E* code
 *     on failure; rt_last_error() returns a thread-local message.  Nothing
 *     here aborts the process (the Go loader panics on a bad material;
 *     internal/scene/scene.go:105,109-145).
 *   - buffers are caller-owned; no pointer is retained after a call returns,
 *     except the scene a context uploads (copied to device memory).
 *   - rt_render is synchronous and blocking like Go's Render
 *     (internal/renderer/renderer.go:67-126).  A context is not safe for
 *     concurrent use from several threads (neither is the Go renderer: it
 *     mutates benchmarkData, renderer.go:103-112).
 *   - all arithmetic on the path is IEEE binary64, like the Go float64 code.
 */
#ifndef RT_API_H
#define RT_API_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_ABI_VERSION 8  /* 8: rt_settings.camera (was _pad2), rt_camera_frame (also added at 8, additive only: rt_adaptive, rt_context_progressive_set_adaptive / _counts_async / _state, rt_adaptive_step, rt_scene_cone_rows, rt_context_render_cameras_async, rt_camera_orbit, rt_stream_decode, rt_aov_buffers, rt_context_render_aov_async, rt_denoise, rt_denoise_inputs, rt_denoise_default, rt_denoise_workspace_bytes, rt_denoise_async, rt_denoise_host, rt_temporal, rt_temporal_frame, rt_temporal_default, rt_temporal_async, rt_temporal_host, rt_temporal_moments_async / _host, rt_variance, rt_variance_inputs, rt_variance_default, rt_variance_async / _host, rt_denoise_var, rt_denoise_var_default, rt_denoise_var_workspace_bytes, rt_denoise_var_async / _host, rt_aov_spec, rt_aov_spec_buffers, rt_aov_spec_default, rt_aov_spec_follows, rt_context_render_aov_spec_async, rt_motion, rt_temporal_motion_async / _host, rt_scene_motion); 7: rt_context_progressive_*, rt_rgba_delta_async; 6: rt_tuning stream* fields, rt_context_stats stream_*; 5: rt_tuning tail_* fields; 4: rt_renderer_rank_seconds takes a capacity */

/* status codes */
#define RT_OK 0
#define RT_E_INVALID (-1)   /* bad argument */
#define RT_E_IO (-2)        /* file read/write failed */
#define RT_E_PARSE (-3)     /* scene JSON malformed */
#define RT_E_DEVICE (-4)    /* HIP runtime / device error */
#define RT_E_NOMEM (-5)
#define RT_E_TIMEOUT (-6)   /* a multi-device frame did not finish in time (rt_renderer_set_watchdog) */

/* Object kinds — internal/scene/scene.go:69-82 ("sphere", "cube"; any other
 * type string is skipped by the loader with "Unknown object type"). */
#define RT_OBJ_SPHERE 0
#define RT_OBJ_CUBE 1

/* Material kinds reachable from JSON — internal/scene/scene.go:104-148. */
#define RT_MAT_LAMBERTIAN 0    /* material.go:18-55 (also the default case) */
#define RT_MAT_METAL 1         /* material.go:57-149 */
#define RT_MAT_SHINY 2         /* material.go:151-225 */
#define RT_MAT_PERFECTMIRROR 3 /* advanced_materials.go:111-171 */
#define RT_MAT_GLASS 4         /* advanced_materials.go:9-66 */
#define RT_MAT_DIELECTRIC 5    /* material.go:227-286 */
#define RT_MAT_DIFFUSELIGHT 6  /* material.go:288-318 */

/* Material parameters exactly as the JSON loader hands them to the Go
 * constructors (scene.go:104-148), i.e. with the loader's defaults already
 * applied (metal: roughness 0, metallic 1, specular 1; shiny: roughness 0,
 * metallic 0, specular 1; perfectmirror: roughness 0; glass/dielectric:
 * refractionIndex 1.5).  The constructors' clamps (NewMetal's
 * Min(x,1.0), material.go:65-73 etc.) are applied by the renderer, not here. */
typedef struct {
  int32_t kind;          /* RT_MAT_* */
  int32_t _pad;
  double color[3];       /* "color" (emit colour for diffuselight) */
  double roughness;
  double metallic;
  double specular;
  double refraction_index;
} rt_material;

/* One scene object — internal/scene/scene.go:26-32 (type Object). */
typedef struct {
  int32_t type;          /* RT_OBJ_* */
  int32_t _pad;
  double position[3];    /* sphere centre / cube centre */
  double size[3];        /* cube edge lengths (unused for spheres) */
  double radius;         /* sphere radius (unused for cubes) */
  rt_material material;
} rt_object;

/* Point light — scene.go:34-39.  "type" is ignored by the renderer
 * (renderer.go:248-294 treats every light as a point light). */
typedef struct {
  double position[3];
  double color[3];
  double intensity;
} rt_light;

/* Camera — scene.go:18-24.  Only position and aspect_ratio are used by the
 * reference's getRay (renderer.go:377-390), which is RT_CAMERA_REFERENCE, the
 * default; look_at, up and fov (the vertical field of view in degrees) are
 * read by the opt-in RT_CAMERA_LOOKAT model (rt_settings.camera). */
typedef struct {
  double position[3];
  double look_at[3];
  double up[3];
  double fov;
  double aspect_ratio;
} rt_camera;

/* Scene view — scene.go:12-16 (type Scene). */
typedef struct {
  rt_camera camera;
  const rt_object* objects;
  int32_t num_objects;
  int32_t _pad0;
  const rt_light* lights;
  int32_t num_lights;
  int32_t _pad1;
} rt_scene;

/* Renderer settings — the ParallelRenderer fields (renderer.go:20-29) and
 * their setters (settings.go:3-25).  Defaults: rt_settings_default(). */
typedef struct {
  int32_t samples;               /* SetSamples; default 100; any count in [0, 2^24] with W*H*samples < 2^40
                                    (past 1024 the linear-scan kernel renders in sample passes) */
  int32_t max_depth;             /* SetMaxDepth; default 50 */
  int32_t anti_aliasing;         /* SetAntiAliasing; inert in the reference (jitter is unconditional, renderer.go:155-156) */
  int32_t recursive_reflections; /* SetRecursiveReflections; default 1 */
  int32_t soft_shadows;          /* SetSoftShadows; default 1 */
  int32_t depth_of_field;        /* SetDepthOfField; inert (advanced.go unused) */
  int32_t num_workers;           /* NewParallelRenderer(n) (the Go CLI passes runtime.NumCPU(),
                                    cmd/raytracer/main.go:46); recorded in benchmark data only */
  int32_t num_devices;           /* rt_render: GPUs 0..n-1 render tiles t % n (0 or 1: device 0 only) */
  uint64_t seed;                 /* counter-based RNG seed (include/rt_rng.h); default 1 */
  int32_t sky;                   /* RT_SKY_*: radiance of a ray that hits nothing; default RT_SKY_NONE */
  int32_t camera;                /* RT_CAMERA_*: which camera model shoots the primary rays; default RT_CAMERA_REFERENCE */
} rt_settings;

/* The camera model.  RT_CAMERA_REFERENCE is the reference's getRay
 * (renderer.go:377-390): rays from camera.position down -Z through a fixed
 * 90-degree viewport of width 2 * aspect_ratio, whatever look_at, up and fov
 * say -- the default and the parity setting.  RT_CAMERA_LOOKAT is OPT-IN and
 * honours the scene's own camera: see rt_camera_frame for its definition.
 * Image row 0 is the BOTTOM of the viewport in both models (the image is
 * vertically flipped vs the camera's up, exactly like the reference). */
#define RT_CAMERA_REFERENCE 0
#define RT_CAMERA_LOOKAT 1

/* What a ray that hits nothing returns.  The reference's live path returns
 * black (traceRay, renderer.go:170-173): RT_SKY_NONE, the default and the
 * parity setting.  The others are OPT-IN and follow the reference's
 * (unlinked) atmosphere package: AtmosphereConfig.GetSkyColor
 * (internal/atmosphere/atmosphere.go:100-135) with the presets
 * NewDefaultAtmosphere / NewWhiteAtmosphere / NewSunsetAtmosphere /
 * NewNightAtmosphere (atmosphere.go:28-98); its undefined FastVec3* helpers
 * are taken as the Vec3 methods of the same name (Normalize, a.Lerp(b, t) =
 * a + (b - a) t, Dot, MulScalar; internal/math/vector.go). */
#define RT_SKY_NONE 0
#define RT_SKY_DEFAULT 1
#define RT_SKY_WHITE 2
#define RT_SKY_SUNSET 3
#define RT_SKY_NIGHT 4

typedef struct {
  double render_seconds;    /* wall time of rt_render, upload + kernels + download (Go Render semantics) */
  double kernel_seconds;    /* device time of the render kernels (HIP events) */
  double rays_per_second;   /* W*H*spp / render_seconds — the published metric (README.md:61) */
  double pixels_per_second; /* W*H / render_seconds (README.md:60) */
  int32_t objects;          /* len(hittables): a cube counts as one (renderer.go:109) */
  int32_t lights;
  /* Where render_seconds went (host wall clock): device state created
   * (rt_render only: contexts, streams, RCCL), scene flattened and uploaded
   * (0 when the renderer already holds it), of which building the BVH (the
   * published benchmark JSON's bvh_build_time / setup_time), the launches
   * enqueued (with a new work schedule: the pilot render and the scheduler,
   * DESIGN.md §4.1), the image copied to the host after the kernels, and
   * the device state freed again (rt_render only). */
  double create_seconds;
  double scene_seconds;
  double bvh_build_seconds;
  double launch_seconds;
  double download_seconds;
  double destroy_seconds;
} rt_stats;

/* Per-launch operation counts (for the roofline's algorithmic FLOPs). */
typedef struct {
  uint64_t camera_rays;      /* primary samples traced */
  uint64_t bounce_rays;      /* closest-hit queries (primary + scattered) */
  uint64_t shadow_rays;      /* any-hit queries (hard + soft) */
  uint64_t sphere_tests;     /* ray/sphere intersection tests executed */
  uint64_t triangle_tests;   /* ray/triangle tests executed */
  uint64_t box_tests;        /* BVH node slab tests executed */
  uint64_t shade_events;     /* surface hits shaded (direct lighting + scatter) */
  uint64_t light_evals;      /* per-light direct-lighting evaluations */
  uint64_t rng_draws;        /* uniform draws */
  /* The part of the nine counts above that the product never executes: the
   * counting variant walks every camera sample so that its counts are the
   * reference's (tracePixel traces them all, renderer.go:150-163), but the
   * product skips the samples of pixels whose camera rays provably miss
   * everything (primary-ray culling).  Executed work =
   * count - culled, in the same order (camera_rays .. rng_draws). */
  uint64_t culled[9];
  /* The wavefront path's soft-shadow traversal kernel alone (wf_occlude<soft>,
   * calculateSmartShadow's 16 jittered rays, renderer.go:311-327): its share
   * of the counts, for that kernel's own roofline (shadow_rays: the rays it
   * traced).  Zero on the megakernel. */
  uint64_t soft_occlusion[9];
  /* The wavefront path's closest-hit traversal (wf_extend, hitWorld
   * renderer.go:333-346) and hard-ray traversal (wf_occlude<hard>,
   * renderer.go:305) alone: their shares of the counts (box and sphere tests;
   * bounce_rays / shadow_rays: the rays each traversed), for each kernel's own
   * roofline.  Zero on the megakernel. */
  uint64_t extend[9];
  uint64_t hard_occlusion[9];
} rt_counts;

void rt_settings_default(rt_settings* s);
/* The library keeps device buffers freed by destroyed contexts and renderers
 * for reuse (rt_render creates and frees its device state every call), at
 * most 4 GB per device; this returns them to the device.  A caller that also
 * allocates device memory elsewhere (PyTorch, RCCL) and runs short should
 * call it: the cached blocks are invisible to other allocators. */
int rt_release_cached_memory(void);
int32_t rt_abi_version(void);
/* Debug: __shfl reads of the kernels whose source lane was inactive (they
 * return no data) since the last reset, on `device`.  Only the checking build
 * (`make xlane`, build/xlane/librtgo.so) counts them; a normal build returns
 * RT_E_INVALID. */
int rt_debug_xlane_faults(int32_t device, int32_t reset, uint64_t* out);
const char* rt_last_error(void);

/* ---------------------------------------------------------------- scene */

typedef struct rt_scene_buf rt_scene_buf; /* owns a parsed scene */

/* scene.LoadFromFile — internal/scene/scene.go:45-57 (+ Vec3.UnmarshalJSON,
 * internal/math/vector.go:176-193, and the material defaults of
 * createMaterial, scene.go:104-148).  Unknown object types are dropped like
 * GetHittables does (scene.go:80-82).  A material without "color" (Go
 * panics, scene.go:113) is loaded with colour (0,0,0) and counted in
 * rt_scene_warnings(). `verbose` != 0 prints the reference's stdout lines
 * (scene.go:62-88). */
int rt_scene_load_json(const char* path, int32_t verbose, rt_scene_buf** out);
int rt_scene_parse_json(const char* text, size_t len, int32_t verbose, rt_scene_buf** out);
const rt_scene* rt_scene_view(const rt_scene_buf* buf);
int32_t rt_scene_warnings(const rt_scene_buf* buf);
void rt_scene_free(rt_scene_buf* buf);
/* Print the lines (*Scene).GetHittables prints (scene.go:62-88), in Go's
 * fmt formatting, for a CLI that mirrors cmd/raytracer. */
int rt_scene_print_hittables(const rt_scene_buf* buf);

/* ------------------------------------------------------- blocking render */

/* (*ParallelRenderer).Render — internal/renderer/renderer.go:67-126.
 * out_linear_rgb: W*H*3 floats (may be NULL), pixel (x,y) at (y*W+x)*3, i.e.
 *   the Go image row y (row 0 is the BOTTOM of the viewport: the image is
 *   vertically flipped vs world up, exactly like the reference).  Value =
 *   mean radiance over samples before tone mapping.
 * out_rgba: W*H*4 bytes (may be NULL) — toneMap + ToRGB, alpha 255
 *   (renderer.go:92-97,348-367; vector.go:106-109).
 * stats may be NULL.  Renders on HIP device 0; returns RT_E_DEVICE (and a
 * message) when no device is present — there is no CPU fallback. */
int rt_render(const rt_scene* scene, int32_t width, int32_t height, const rt_settings* settings,
              float* out_linear_rgb, uint8_t* out_rgba, rt_stats* stats);
/* The argument checks rt_render makes before it touches a device (scene
 * arrays and kinds; 1 <= W, H <= 65536; samples range): RT_OK or RT_E_INVALID. */
int rt_validate(const rt_scene* scene, int32_t width, int32_t height, const rt_settings* settings);

/* The viewport frame of `cam` under camera model `model` (RT_CAMERA_*) for a
 * width x height image: out = origin, lower_left, horizontal, vertical, three
 * doubles each, in plain binary64 with Go Vec3 semantics and this order:
 *   reference: horizontal = (2 * aspect_ratio, 0, 0), vertical = (0, 2, 0),
 *     lower_left = origin - horizontal/2 - vertical/2 - (0, 0, 1)
 *     (getRay, renderer.go:377-390);
 *   look-at:   w = normalize(position - look_at), U = normalize(cross(up, w)),
 *     V = cross(w, U); h = 1.0 when fov == 90, else tan(fov * (pi / 360));
 *     a = aspect_ratio, or (double)width / height when aspect_ratio is 0;
 *     horizontal = U * (2 h a), vertical = V * (2 h),
 *     lower_left = origin - horizontal/2 - vertical/2 - w.
 * The exact 1.0 at 90 degrees (tan(pi/4) rounds to 0.9999999999999999) makes
 * a look-at camera that looks down -Z with up +Y shoot the reference's rays
 * bit for bit.  The ray of image coordinates (u, v) is, per component,
 * ((lower_left + horizontal * u) + vertical * v) - origin, not normalised;
 * row 0 of the image is v in [0, 1/height): the BOTTOM of the viewport.
 * RT_E_INVALID (with a message) for an unknown model and, in look-at mode,
 * for a camera whose fields are not finite, position == look_at, cross(up, w)
 * of zero length (a zero up included), fov outside (0, 180) or
 * aspect_ratio < 0 -- the checks rt_validate and every render entry point
 * make in look-at mode.  The reference model reads position and aspect_ratio
 * only and checks nothing. */
int rt_camera_frame(const rt_camera* cam, int32_t model, int32_t width, int32_t height, double out[12]);

/* The shadow-cone rows of `scene` as rt_context_set_scene(scene, force_bvh)
 * derives them (host only, no device): out[light * num_objects + hittable], one
 * 64-bit mask each, num_lights * num_objects of them (capacity: the rows `out`
 * holds; fewer is RT_E_INVALID).  Bit b of a row is CLEAR only when the b-th
 * sphere of the scene (in hittable order, cubes not counted) provably stays
 * clear of every shadow ray -- hard or soft -- that can leave a hit point on
 * that hittable towards that light, so the shadow-cone test of such a hit
 * never has to look at it.  The hit sphere's own bit is always set.  Every bit
 * of a row is set (~0) where nothing is proven: the hittable is a cube, a
 * centre, radius or light position of the scene is not finite, or the scene
 * has no shadow-cone masks (a tree, more than 64 spheres, more than 64
 * triangles). */
int rt_scene_cone_rows(const rt_scene* scene, int32_t force_bvh, uint64_t* out, size_t capacity);

/* The stream kernel's entry decode (host only, no device): entry entries[j] of
 * a streamed launch of `frames` frames, `nlive` live pixels and `spp` samples
 * in entry order `order` (rt_tuning.stream_order: 0 e = (frame * nlive + pixel)
 * * spp + sample, 1 e = (pixel * spp + sample) * frames + frame) as the kernel
 * decodes it -- the same function, with the multiply-high magic numbers the
 * launch computes -- into out[3 j .. 3 j + 2] = frame, live pixel, sample.
 * frames, nlive, spp in [1, 2^31) and every entry below 2^31 (a launch's own
 * bound), or RT_E_INVALID. */
int rt_stream_decode(int32_t order, uint32_t frames, uint32_t nlive, uint32_t spp, const uint32_t* entries, size_t n,
                     uint32_t* out);

/* The screen the spheres-only stream kernels put in front of the exact test of
 * a soft shadow ray (host only, no device; the same function the kernels
 * run).  Case j: the sphere of centre centers[3 j ..] and squared radius
 * r2[j], the ray from origins[3 j ..] along the UNNORMALISED direction
 * dirs[3 j ..], il[j] the caller's approximation of 1 / |dir|, over
 * [tmin[j], tmax[j]].  out[j] is RT_SOFT_MISS or RT_SOFT_HIT when the screen
 * is sure -- then Sphere.Hit on the normalised ray returns that boolean,
 * provided |il |dir| - 1| <= 2e-7 -- and RT_SOFT_UNDECIDED otherwise (always
 * for a NaN or an infinity in any input). */
#define RT_SOFT_UNDECIDED 0
#define RT_SOFT_MISS 1
#define RT_SOFT_HIT 2
int rt_soft_screen(const double* centers, const double* r2, const double* origins, const double* dirs, const double* il,
                   const double* tmin, const double* tmax, size_t n, int32_t* out);

/* ------------------------------------------ persistent multi-GPU renderer */

/* The ParallelRenderer object itself (NewParallelRenderer, renderer.go:54-65,
 * then Render per frame, renderer.go:67-126), on GPUs instead of goroutines.
 * One process drives `num_devices` ranks; rank r renders the 32x32 tiles
 * t with t % num_devices == r on devices[r] (devices NULL: 0..n-1).  Ranks
 * whose device is devices[0] render straight into the gather buffer there;
 * the others send their packed tiles (float3 + RGBA8, 16 B per pixel) to
 * devices[0] in ONE RCCL group over xGMI (ncclCommInitAll over the distinct
 * devices), where one kernel scatters them into the image.  Output is
 * bit-identical for every device count (the random stream is keyed by
 * global pixel and sample).  The renderer keeps each device's scene, work
 * schedule and buffers between calls: a call with the same scene content,
 * size and settings (any seed) re-uploads nothing.  A call drives every rank
 * from its own host thread (joined before it returns).  Not thread-safe
 * itself: one call at a time per renderer (nor is the Go renderer:
 * renderer.go:103-112). */
typedef struct rt_renderer rt_renderer;
int rt_renderer_create(const int32_t* devices, int32_t num_devices, rt_renderer** out);
/* Render with the renderer's devices (settings->num_devices is ignored). */
int rt_renderer_render(rt_renderer* r, const rt_scene* scene, int32_t width, int32_t height,
                       const rt_settings* settings, float* out_linear_rgb, uint8_t* out_rgba, rt_stats* stats);
void rt_renderer_destroy(rt_renderer* r);
/* Watchdog of a multi-rank Render (more than one rank): the frame gets one
 * deadline, `seconds` after Render starts (after the scene upload).  Every
 * host wait of the frame is bounded by it: each rank's waits inside its share
 * render (its previous render, the schedule build, a BVH scene's bounce loop),
 * the partition's measuring render, and the waits for the ranks' streams, the
 * RCCL gather into the first device (renderer.go:398-436 is the tile farm-out
 * it replaces) and the unpack.  Past it, Render stops waiting, aborts the
 * renderer's RCCL communicators and returns RT_E_TIMEOUT with the rank,
 * device, frame and partition in rt_last_error().  The renderer is then
 * unusable: later calls return RT_E_TIMEOUT, and rt_renderer_destroy releases
 * only what does not wait on the stalled work (exit the process to reclaim the
 * rest).  Default 0: no bound, as Go's Render (a large frame may take
 * minutes); callers opt in (the CLI: --watchdog SECONDS).  One-rank renders
 * have no collective and are never bounded. */
int rt_renderer_set_watchdog(rt_renderer* r, double seconds);
/* Test hook for the watchdog: the renderer's next multi-rank frame first
 * runs, on `rank`'s stream, one workgroup that sleeps for `ms` (0..60000)
 * milliseconds of device time and then exits -- a stall that always ends. */
int rt_renderer_test_stall(rt_renderer* r, int32_t rank, double ms);

/* ------------------------------------------- resident context (bench/MGPU) */

typedef struct rt_context rt_context;

int rt_context_create(int32_t device, rt_context** out);
void rt_context_destroy(rt_context* ctx);

/* Flatten (GetHittables, scene.go:59-90; createCube, scene.go:150-190) and
 * upload the scene to device memory.  Builds the BVH, one tree over the
 * spheres and the cubes (a cube is one primitive: its box, then its 12
 * triangles), when the scene is large: more than 64 spheres, or more than 64
 * cubes (or when force_bvh > 0; force_bvh < 0 forbids it).  The image is the
 * linear scan's bit for bit on either RT_PATH_*.  A scene with a
 * sphere whose centre or radius is not finite never gets a BVH, forced or
 * not: such a sphere has no bounding box (a NaN one is hit by every ray), and
 * the linear scan renders it whatever the number of spheres.  Non-finite
 * geometry is rendered for spheres alone: a cube whose position or size is not
 * finite, and a sphere whose centre or radius is not finite in a scene that
 * has a cube, are refused with RT_E_INVALID (by every entry point that takes
 * a scene, rt_validate included); the message names the object and the field.
 * Non-finite lights and materials are accepted. */
int rt_context_set_scene(rt_context* ctx, const rt_scene* scene, int32_t force_bvh);

/* Work-partition tuning.  No setting changes a single output bit (the GPU
 * parity tests render with each and compare against the oracle): they only
 * choose how the same work is cut into blocks and ordered, and exist for the
 * tests that force every kind of work block and for experiments.  The
 * library never reads the environment. */
#define RT_PATH_AUTO 0        /* wavefront kernels for BVH scenes, else the megakernel */
#define RT_PATH_MEGAKERNEL 1  /* the megakernel also for BVH scenes */
typedef struct {
  int32_t path;           /* RT_PATH_* */
  int32_t pilot;          /* 1: block sizes from a one-sample pilot render; 0: geometric estimate */
  int32_t frustum;        /* 1: primary-ray candidate masks (cull, black tiles) */
  int32_t stage;          /* 1: small scenes staged into LDS */
  double block_work;      /* path bounces x samples per block; 0: default (one frame per launch: 384, 256 with
                             triangles; several frames per launch: 1024, 2048 with triangles; BVH scenes 8192) */
  int32_t block_samples;  /* pixels x samples of a large block at most; 0: 1024 */
  int32_t bvh_bins;       /* SAH bins per axis; 0: 32 */
  int32_t bvh_leaf;       /* spheres per BVH leaf at most (1..7); 0: 4 */
  int32_t wf_paths;       /* wavefront path slots (at most 2^24); 0: 2^24, fewer when the frame has fewer samples */
  int64_t wf_chunk;       /* wavefront samples per chunk; 0: 2^30 */
  int32_t wf_lds_nodes;   /* BVH nodes staged into LDS; -1: as many as fit */
  int32_t wf_trav_block;  /* threads per traversal workgroup (64..1024); 0: 1024 */
  int32_t wf_trav_wgs;    /* traversal workgroups sharing a CU's LDS; 0: 1 */
  int32_t pilot_depth;    /* bounces the pilot render follows a path at most (default 12); 0: max_depth */
  int32_t split_samples;  /* samples per sub-block of a split (heavy) pixel, 1..64; 0: 64 */
  int32_t measure;        /* 1: the first frame of a schedule measures every pixel's path lengths and the
                             next frame re-cuts the blocks from them; 0: pilot schedule only (default) */
  int32_t split_depth;    /* measured schedules split a pixel with a path of more bounces than this; 0: 16 */
  int32_t partition;      /* rt_renderer with N > 1 ranks: RT_PARTITION_*; 0: auto (balanced for linear-scan
                             scenes, strided for BVH scenes, whose frames have thousands of busy tiles) */
  int32_t wf_list_tries;  /* wavefront list test: rejection tries a listed cone's accepted-try mask covers
                             (1..64; 0: 64); later points continue the sequential loop (tests force it low) */
  /* tail helpers (megakernel, staged scenes): a block's last
   * few long paths are handed to extra one-wave workgroups at the end of the
   * launch that run each alone, at the latency of a lone bounce */
  int32_t tail_helpers;   /* helper workgroups per launch; 0: 64; -1: none, the paths stay in their blocks
                             (rt_tuning_default: -1; DESIGN.md §4.6 measures 64 as a net loss) */
  int32_t tail_paths;     /* a block exports once at most this many paths are left; 0: 4 */
  int32_t tail_depth;     /* ... each at least this many bounces deep; 0: 2 */
  int32_t tail_every;     /* ... checked every this many iterations of the block's drain (rounded up to a power of 2, at most 64); 0: 4 */
  int32_t tail_at;        /* the helpers follow this percentage of the launch's main workgroups (1..100); 0: 100 */
  /* streamed launches (megakernel, staged linear-scan scenes):
   * the samples of the live pixels of a launch's frames form one queue that
   * persistent waves drain; a resolve kernel sums each pixel's per-sample rows */
  int32_t stream;         /* -1: auto (rt_tuning_default: launches of several frames, where it is measured to
                             gain); 0: never; 1: whenever eligible, one-frame launches too */
  int32_t stream_chunk;   /* queue entries a wave claims at a time (1..65536); 0: 512 */
  double stream_max_mb;   /* row buffer budget in MiB, fractions allowed (24 B per live pixel, sample and
                             frame); 0: 1024.  A launch whose rows exceed it runs as groups of consecutive
                             frames; when not even two frames (one, of a one-frame launch) fit, the launch
                             takes the block kernel */
  int32_t stream_order;   /* entry order; 0: frame-major (a chunk holds neighbouring samples of one pixel),
                             1: the launch's frames interleaved (rt_tuning_default: 1) */
  int32_t _stream_pad;
} rt_tuning;
#define RT_PARTITION_AUTO 0
#define RT_PARTITION_STRIDED 1
#define RT_PARTITION_BALANCED 2
void rt_tuning_default(rt_tuning* t);
/* Applies to later rt_context_set_scene (BVH shape) and render calls. */
int rt_context_set_tuning(rt_context* ctx, const rt_tuning* t);
int rt_renderer_set_tuning(rt_renderer* r, const rt_tuning* t);

#define RT_LAYOUT_IMAGE 0        /* write pixels of this rank's tiles into a W*H image */
#define RT_LAYOUT_PACKED_TILES 1 /* write this rank's tiles packed: [local_tile][32*32] */

/* Number of 32x32 tiles of a W*H image (createRenderTasks, renderer.go:398-436). */
int32_t rt_num_tiles(int32_t width, int32_t height);
/* Tiles owned by `rank` of `world` under strided assignment t -> t % world. */
int32_t rt_tiles_for_rank(int32_t width, int32_t height, int32_t rank, int32_t world);

/* Enqueue a render of the tiles t with t % world == rank on `hip_stream`
 * (a hipStream_t, NULL = default stream).  d_linear (float3 per pixel) and
 * d_rgba (4 B per pixel, may be NULL) are DEVICE pointers sized for the
 * layout: W*H pixels (IMAGE) or rt_tiles_for_rank()*1024 pixels (PACKED).
 * Asynchronous: returns after the launches are queued.  If counts != NULL a
 * counting variant runs instead and the counts are returned (synchronous). */
int rt_context_render_async(rt_context* ctx, int32_t width, int32_t height, const rt_settings* settings,
                            int32_t rank, int32_t world, int32_t layout, float* d_linear, uint8_t* d_rgba,
                            void* hip_stream, rt_counts* counts);

/* Several frames of the same scene, size and settings that differ only in
 * their seed (seeds[f]), rendered by ONE launch: the reference's Render
 * called nframes times (renderer.go:67-126), each frame bit-identical to its
 * own rt_context_render_async.  The frames share the work schedule; the
 * launch's workgroups interleave them (every frame's heaviest blocks first),
 * so the low-occupancy tail of long paths is paid once per launch instead of
 * once per frame.  d_linear[f] / d_rgba[f] (d_rgba may
 * be NULL, entries may be NULL) are laid out as in rt_context_render_async.
 * BVH scenes, sample passes and measuring frames render frame by frame. */
#define RT_MAX_FRAMES 32
int rt_context_render_frames_async(rt_context* ctx, int32_t width, int32_t height, const rt_settings* settings,
                                   int32_t nframes, const uint64_t* seeds, int32_t rank, int32_t world,
                                   int32_t layout, float* const* d_linear, uint8_t* const* d_rgba, void* hip_stream);

/* A camera sequence: nframes frames of the context's scene,
 * frame f seen from cameras[f] -- a turntable, a fly-through, a stereo pair.
 * Frame f is, byte for byte, what rt_context_render_async writes when the
 * scene's camera is cameras[f] and settings->seed is seeds[f] (seeds NULL:
 * settings->seed for every frame); settings->camera picks the camera model for
 * all frames.  Buffers, layout, rank and world as in
 * rt_context_render_frames_async.  Where a batched launch of nframes frames
 * would be streamed (rt_tuning.stream; auto: scenes of spheres alone, two
 * frames or more) the frames are ONE streamed launch on one work schedule,
 * whose live pixels are the union over the cameras.  Everything else -- one
 * frame, BVH scenes on the wavefront path, sample passes, a sky, measuring
 * schedules, tail helpers, scenes with triangles under the auto rule --
 * renders FRAME BY FRAME, each frame with its camera in place of the scene's:
 * correct and slow, with a new work schedule per frame.
 * RT_E_INVALID, with nothing enqueued and no buffer touched: nframes outside
 * [1, RT_MAX_FRAMES], NULL cameras or d_linear, and in look-at mode a camera
 * that rt_camera_frame refuses (the message names the frame's index).  The
 * cameras are copied before the call returns and no pointer is retained.  The
 * scene's own camera does not change: later renders show the scene's view.  A
 * progression of the context is not disturbed. */
int rt_context_render_cameras_async(rt_context* ctx, int32_t width, int32_t height, const rt_settings* settings,
                                    int32_t nframes, const rt_camera* cameras, const uint64_t* seeds,
                                    int32_t rank, int32_t world, int32_t layout,
                                    float* const* d_linear, uint8_t* const* d_rgba, void* hip_stream);
/* n views on a circle around the camera's look_at (host only): with a = up
 * normalised, v = position - look_at and theta_k = (degrees * k / n) * (pi / 180),
 * out[k] is cam with
 *   position = look_at + v cos(theta_k) + (a x v) sin(theta_k) + a (a . v) (1 - cos(theta_k))
 * per component, in plain binary64 in exactly this order; every other field
 * is copied, and out[0] is cam bit for bit.  RT_E_INVALID for n < 1, a field
 * or degrees that is not finite, and a zero up. */
int rt_camera_orbit(const rt_camera* cam, int32_t n, double degrees, rt_camera* out /* n */);

/* First-hit feature buffers: what a denoiser, object picking
 * and a depth or matte pass start from -- per pixel, the albedo, normal, depth,
 * coverage and object of the camera rays' first hits.  No image is rendered.
 *
 * The definition.  For a width x height (W x H) image and n = settings->samples
 * >= 1, sample s of pixel (x, y) has the render's own camera ray: its stream is
 * rt_rng_init(key, y * W + x, s) (include/rt_rng.h, key = rt_rng_seed_key(
 * settings->seed)), u = (x + draw0) / W, v = (y + draw1) / H, and its direction
 * is ((lower_left + horizontal * u) + vertical * v) - origin per component, not
 * normalised, from the frame of rt_camera_frame for the camera and the model
 * (settings->camera) in use.  The sample's hit is hitWorld(ray, 0.001, +Inf)
 * (renderer.go:333-346): the closest hittable, an exact tie going to the later
 * one.  Its HitRecord is the reference's (sphere.go:42-58, triangle.go:67-81):
 * T the ray parameter, Normal already turned against the ray; the material's
 * GetAlbedo() is the JSON colour, except (1, 1, 1) for dielectric and (0, 0, 0)
 * for diffuselight.  Per pixel, over the hitting samples in ascending s, with
 * binary64 sums sumA (albedo), sumN (normal), sumT and the integer `hits`:
 *   albedo    float3   (float)(sumA / n) per component (a miss adds black, as it does to the image)
 *   normal    float3   (float)(sumN / n), not renormalised
 *   depth     float    (float)(sumT / hits), +Inf when hits == 0
 *   coverage  float    (float)((double)hits / n)
 *   object    int32    the hittable index (the rt_object's index, a cube counts as one) of the
 *                      lowest hitting s, -1 when hits == 0
 * Divisions are plain IEEE binary64.  Pixel (x, y) is at y * W + x, row 0 the
 * BOTTOM of the viewport like the image.  In both camera models the view-axis
 * component of the direction is exactly the focal length 1, so T is the hit's
 * distance ALONG THE VIEW AXIS in world units: `depth` is a z-buffer, not a
 * distance from the eye.
 * The buffers depend on the scene, the size, the camera, the camera model,
 * samples and seed only: max_depth (0 included), recursive_reflections,
 * soft_shadows, sky and every rt_tuning field change no bit of them, nor does
 * force_bvh (the tree and the linear scan find the same hit).  A scene that
 * rt_context_set_scene accepts with non-finite sphere geometry does not fault;
 * the values at such hits carry no contract.
 *
 * The call.  Every pointer of rt_aov_buffers is a DEVICE pointer or NULL (that
 * buffer is not written).  Asynchronous on `hip_stream` like the render calls.
 * It covers the WHOLE frame in image layout: there are no rank / world shares
 * and no packed layout -- the pass is a small fraction of a render, one device
 * does it, and multi-device callers run it on their first device.  camera NULL:
 * the scene's; else it is copied before the call returns.  A progression and
 * the context's work schedules are not disturbed, a render after the call is
 * byte for byte the render before it, and nothing counts in rt_context_stats;
 * the call records HIP events around its own launch, so
 * rt_context_last_kernel_seconds reports its device time when it was the last
 * launch.
 * RT_E_INVALID with a message, nothing enqueued and no buffer touched: a NULL
 * ctx, settings or out; all five pointers NULL; no scene set; samples < 1; a
 * size or samples range that rt_validate refuses; in look-at mode a camera
 * that rt_camera_frame refuses. */
typedef struct {
  float* d_albedo;    /* W*H*3 */
  float* d_normal;    /* W*H*3 */
  float* d_depth;     /* W*H   */
  float* d_coverage;  /* W*H   */
  int32_t* d_object;  /* W*H   */
} rt_aov_buffers;
int rt_context_render_aov_async(rt_context* ctx, int32_t width, int32_t height, const rt_settings* settings,
                                const rt_camera* camera /* NULL: the scene's */, const rt_aov_buffers* out,
                                void* hip_stream);

/* Specular-through feature buffers: the same buffers, taken
 * not at the camera ray's first hit but at the first surface behind the
 * mirrors -- each sample follows IDEAL mirror reflections from its first hit
 * to the first surface that is not mirror-like -- plus a per-pixel specular
 * flag and the number of reflections followed.  A filter guided by them stops
 * at the edges of what a mirror shows, not only at the mirror's own.
 *
 * Parameters (rt_aov_spec; rt_aov_spec_default sets max_bounces 4 and
 * max_roughness 0.1 -- the 0.1 is a convention, "what still looks like a
 * mirror", not a measurement): max_bounces in [0, 16]; max_roughness finite
 * and >= 0.  Anything else (a NaN included) is RT_E_INVALID.
 *
 * Followed materials.  A material is followed iff its kind is RT_MAT_METAL,
 * RT_MAT_SHINY or RT_MAT_PERFECTMIRROR and Min(roughness, 1.0) <=
 * max_roughness (Go's math.Min, the constructors' clamp; a NaN roughness
 * compares false).  Glass and dielectric are never followed: their direction
 * is a random choice.  rt_aov_spec_follows is this predicate on the host, no
 * device needed: 1, 0, or RT_E_INVALID for a NULL or parameters out of range.
 *
 * The chain of sample s of pixel (x, y).  Ray 0 is the camera ray of the
 * first-hit pass, unchanged (the same stream, the same two draws, the same
 * frame).  Hit j is hitWorld(ray_j, 0.001, +Inf), with the same tie rule and
 * the same HitRecord.  While hit j exists, its material is followed and
 * j < max_bounces, ray j+1 has the origin Point_j (o + d * T, as the
 * HitRecord has it) and the direction d_j.Reflect(Normal_j) =
 * d - n * (2 * (d . n)), NOT normalised and without perturbation: exactly the
 * ray the reference's Scatter makes for a metal of roughness 0.  No random
 * number is drawn after the camera ray.
 * Per sample: it HITS iff hit 0 exists; its TERMINAL hit is the last existing
 * hit of the chain (the first surface that is not followed, or the last
 * mirror when the next ray misses or the cap is reached); k is the number of
 * reflections followed to reach the terminal hit (a reflected ray that misses
 * does not count).
 * Per pixel, sums over the hitting samples in ascending s, in binary64, with
 * n = samples:
 *   albedo    float3   (float)(sumA / n); each sample adds the per-component product, in chain
 *                      order, of GetAlbedo() of hits 0 .. terminal
 *   normal    float3   (float)(sumN / n), the terminal hit's Normal, not renormalised
 *   depth     float    (float)(sumT / hits), +Inf when hits == 0; each sample adds
 *                      T_0 + T_1 + ... + T_terminal, added in that order
 *   coverage  float    (float)((double)hits / n): identical to the first-hit pass
 *   object    int32    the terminal hittable index of the lowest hitting s, -1 when hits == 0
 *   specular  float    (float)((double)m / n), m the samples whose hit 0 has a followed material
 *   bounces   float    (float)(sumK / n)
 * Reflection keeps the direction's length up to rounding, so every T is in the
 * units of the first-hit depth and `depth` is a VIRTUAL z: the depth at which
 * the reflected surface appears behind the mirror.  Its finiteness -- valid(p)
 * to the filters -- is that of the first-hit depth.
 * With max_bounces == 0, or in a scene where no material is followed, the
 * first five buffers equal the first-hit pass bit for bit and bounces is 0.
 * The same independence holds as for the first-hit pass: max_depth, the shadow
 * and reflection switches, sky, every rt_tuning field and force_bvh change no
 * bit.
 * Known limit: a pixel that sees object A in a mirror and a pixel that sees A
 * directly carry the same `object`; only the normal and the virtual depth
 * separate them.  `bounces` is there for callers who want a stricter key.
 *
 * The call keeps the contract of rt_context_render_aov_async word for word:
 * device pointers or NULL (not written), asynchronous on `hip_stream`, the
 * WHOLE frame in image layout, camera NULL: the scene's (else copied before
 * the call returns), no progression or work schedule disturbed, a render after
 * the call byte for byte the render before it, nothing counted in
 * rt_context_stats, its own HIP events for rt_context_last_kernel_seconds.
 * RT_E_INVALID with a message, nothing enqueued and no buffer touched: what
 * rt_context_render_aov_async refuses (with all SEVEN pointers NULL), and a
 * NULL or out-of-range rt_aov_spec. */
typedef struct {
  int32_t max_bounces;   /* 0..16 reflections followed per sample */
  int32_t _pad;
  double max_roughness;  /* finite, >= 0 */
} rt_aov_spec;
typedef struct {
  float* d_albedo;    /* W*H*3 */
  float* d_normal;    /* W*H*3 */
  float* d_depth;     /* W*H   */
  float* d_coverage;  /* W*H   */
  int32_t* d_object;  /* W*H   */
  float* d_specular;  /* W*H   */
  float* d_bounces;   /* W*H   */
} rt_aov_spec_buffers;
void rt_aov_spec_default(rt_aov_spec* spec);
int rt_aov_spec_follows(const rt_material* material, const rt_aov_spec* spec);
int rt_context_render_aov_spec_async(rt_context* ctx, int32_t width, int32_t height, const rt_settings* settings,
                                     const rt_camera* camera /* NULL: the scene's */, const rt_aov_spec* spec,
                                     const rt_aov_spec_buffers* out, void* hip_stream);

/* Matte layers: per pixel, WHICH objects its camera rays hit
 * first and how many rays each -- what compositing calls a matte, and what
 * rt_matte_resolve_async below rebuilds an antialiased silhouette from.
 * rt_aov_buffers' d_object is only the id of the lowest hitting sample and
 * d_coverage only the total; this is the list behind them.
 *
 * The definition.  Rays and hits are as rt_aov_buffers: sample s of pixel
 * (x, y) is the render's own camera ray and its hit is hitWorld(ray, 0.001,
 * +Inf).  n = settings->samples >= 1 is the number of MATTE samples; it is
 * independent of a render's sample count, and since a ray depends on (seed,
 * pixel, s) only, the first samples are the render's.
 *   The key of a hitting sample.  level RT_MATTE_OBJECT: the hittable index,
 *   the value d_object uses.  level RT_MATTE_FACE: object * 16 + f, where f is
 *   0 for a sphere and for a cube the ordinal 0..11 of the hit triangle in
 *   createCube's order (scene.go:150-190: faces -z, +x, +z, -x, +y, -y of a
 *   positive size, two triangles each).  A miss has no key.
 *   Slots.  A pixel has RT_MATTE_SLOTS (key, count) slots.  Samples are walked
 *   in ascending s.  A hitting sample whose key is in a slot increments that
 *   slot's count; otherwise, if a slot is free, it takes the next one with
 *   count 1; otherwise `overflow` is incremented.  `hits` counts every hitting
 *   sample.
 *   Ranks.  The slots ordered by count descending, by key ascending among
 *   equal counts.  K = params->ranks.
 * Outputs, each a DEVICE pointer or NULL (not written), planar with plane r at
 * r * W * H, so plane 0 is an image; pixel (x, y) at y * W + x like the image:
 *   d_id     K planes of int32   the key of rank r, -1 for an empty rank
 *   d_count  K planes of int32   its count, 0 for an empty rank
 *   d_rest   one int32 plane     hits - (sum of the K counts): the dropped
 *                                ranks and the overflow
 * Counts are integers: sum(count) + rest == hits exactly, and hits equals
 * d_coverage * n of the first-hit pass.
 * The buffers depend on the scene, the size, the camera, the camera model,
 * samples, seed, level and ranks only; force_bvh changes no bit of them.
 *
 * The call obeys rt_context_render_aov_async's rules: asynchronous on
 * `hip_stream`, the WHOLE frame in image layout, camera NULL: the scene's (else
 * copied before the call returns), no progression or work schedule disturbed, a
 * render after the call byte for byte the render before it, nothing counted in
 * rt_context_stats, its own HIP events for rt_context_last_kernel_seconds.
 * RT_E_INVALID with a message, nothing enqueued and no buffer touched: what
 * rt_context_render_aov_async refuses (with all THREE pointers NULL), a NULL
 * params, ranks outside 1..RT_MATTE_MAX_RANKS, a level that is neither
 * constant, and at the face level a scene of 2^27 or more objects. */
#define RT_MATTE_SLOTS 16
#define RT_MATTE_MAX_RANKS 8
#define RT_MATTE_OBJECT 0
#define RT_MATTE_FACE 1
typedef struct {
  int32_t ranks;  /* K, 1..RT_MATTE_MAX_RANKS */
  int32_t level;  /* RT_MATTE_OBJECT or RT_MATTE_FACE */
} rt_matte;
typedef struct {
  int32_t* d_id;     /* K * W*H */
  int32_t* d_count;  /* K * W*H */
  int32_t* d_rest;   /* W*H     */
} rt_matte_buffers;
void rt_matte_default(rt_matte* m); /* ranks 4, level RT_MATTE_OBJECT */
int rt_context_render_matte_async(rt_context* ctx, int32_t width, int32_t height, const rt_settings* settings,
                                  const rt_camera* camera /* NULL: the scene's */, const rt_matte* params,
                                  const rt_matte_buffers* out, void* hip_stream);

/* Progressive rendering: one frame's samples rendered over
 * several calls, with the image of the samples so far after each.  A context
 * holds at most one progression.  begin: the frame (size, rank, world and
 * layout as rt_context_render_async), with settings->samples the CAP, the
 * most samples per pixel the progression may reach; it zeroes the
 * progression's own per-pixel sums and starts over when the context already
 * has one.  add_async: samples [done, done + nsamples) of every pixel of the
 * rank's tiles, each pixel's sum continued in sample order, then the mean
 * over done + nsamples samples written to d_linear / d_rgba (buffers as
 * rt_context_render_async; either may be NULL) -- after adds totalling n
 * samples the image is that of rt_context_render_async with samples = n,
 * byte for byte.  nsamples < 1, done + nsamples > cap, no progression or an
 * ended one: RT_E_INVALID, nothing changes.  samples: done so far, -1 without
 * a progression.  end: frees the sums.  rt_context_set_scene, _set_tuning and
 * _set_partition end a progression; ordinary renders between two adds do not
 * disturb it.  An add counts in rt_context_stats.frames and .launches like a
 * render; adds of equal nsamples share one work schedule. */
int rt_context_progressive_begin(rt_context* ctx, int32_t width, int32_t height, const rt_settings* settings,
                                 int32_t rank, int32_t world, int32_t layout);
int rt_context_progressive_add_async(rt_context* ctx, int32_t nsamples, float* d_linear, uint8_t* d_rgba,
                                     void* hip_stream);
int64_t rt_context_progressive_samples(const rt_context* ctx);
int rt_context_progressive_end(rt_context* ctx);

/* Adaptive sampling: every pixel of a progression stops on
 * its own once its displayed value has stopped moving.  Each in-image pixel
 * of the rank's tiles has a sample count, a streak and an active flag
 * (initially set).  An adaptive add of n samples renders samples [count,
 * count + n) of every ACTIVE pixel (all active pixels share count == the
 * samples done), continues its sum in sample order, and then, per active
 * pixel: new = the tone-mapped RGBA8 of (float)(sum / count); when the pixel
 * had an image before this add, d = the largest |new - old| over the four
 * bytes and streak = d <= tolerance ? streak + 1 : 0 (on the first add the
 * streak stays 0); the pixel stops for good when streak >= patience and
 * count >= min_samples, keeping its sum, count and image.  A stopped pixel is
 * neither traced nor changed by later adds.  After every add d_linear /
 * d_rgba hold (float)(sum / count) and its tone map for EVERY pixel, stopped
 * ones included: pixel p is that of rt_context_render_async with samples =
 * count[p], byte for byte.  The rule reads no neighbour, so image and counts
 * are the same for every partition, rank count, path and tuning. */
typedef struct { int32_t tolerance, patience, min_samples, _pad; } rt_adaptive;
/* After rt_context_progressive_begin and before its first add; NULL: off (the
 * default after every begin).  RT_E_INVALID (nothing changes) without a
 * progression, after an add, for tolerance outside 0..255, patience < 1,
 * min_samples < 0, and for a progression with a sky (its images match the
 * reference only to a tolerance, so its stop decisions could not be pinned). */
int rt_context_progressive_set_adaptive(rt_context* ctx, const rt_adaptive* a);
/* Per-pixel sample counts in the progression's layout (IMAGE: W*H words,
 * pixels outside this rank's tiles 0; PACKED: local tiles * 1024 words, pixels
 * outside the image 0), a device pointer, on `hip_stream` after the last add.
 * Without set_adaptive every pixel's count is the samples done. */
int rt_context_progressive_counts_async(rt_context* ctx, uint32_t* d_counts, void* hip_stream);
/* Waits for the last add.  out = in-image pixels of the rank's tiles, those of
 * them still active, the sum of their counts, adds so far. */
int rt_context_progressive_state(rt_context* ctx, int64_t out[4]);
/* The stop rule for one pixel on the host (the function the device kernel
 * applies, include/rt_adaptive.h): old / new displayed RGBA, whether the pixel
 * had an image before the add, its count including the add, its streak before
 * it.  Returns 1 stop, 0 go on, with *new_streak set; RT_E_INVALID on NULL
 * arguments or values out of range (a as for set_adaptive, count or streak < 0). */
int rt_adaptive_step(const uint8_t old_rgba[4], const uint8_t new_rgba[4], int32_t had_image, int32_t count,
                     int32_t streak, const rt_adaptive* a, int32_t* new_streak);
/* How much two RGBA8 images of npix pixels (device pointers) differ, into the
 * two device words d_out: [0] the pixels whose four bytes are not all equal,
 * [1] the largest |a - b| over all bytes.  Zeroes d_out on the stream first.
 * Exact and independent of order: a progression's stop criterion (how much
 * the preview still moved in the last pass). */
int rt_rgba_delta_async(const uint8_t* d_a, const uint8_t* d_b, size_t npix, uint32_t* d_out, void* hip_stream);

/* À-trous denoiser guided by the first-hit feature buffers:
 * an edge-stopping wavelet filter over a render's linear image, steered by the
 * buffers of rt_context_render_aov_async, so that a preview of a few samples
 * per pixel can be shown without most of its Monte-Carlo noise.  The
 * project's own feature (the reference has no denoiser), defined here to the
 * bit: binary64 `+ - * /` and comparisons only, in a fixed order, so that the
 * device kernels, rt_denoise_host and a restatement in any language agree
 * exactly (include/rt_denoise.h is the code both sides run).
 *
 * Inputs, per pixel p = y * W + x, laid out as rt_context_render_async and
 * rt_aov_buffers lay them out:
 *   color   float3  required: the linear mean radiance (d_linear of any render)
 *   normal  float3  required
 *   depth   float   required
 *   albedo  float3  optional (NULL: no demodulation)
 *   object  int32   optional (NULL: no id stop)
 * Coverage is not read.  valid(p) means depth[p] is finite (a miss has +Inf).
 * Float inputs are widened to binary64 before use.
 *
 * Parameters (rt_denoise; rt_denoise_default sets the defaults):
 *   levels        1..8                            default 4
 *   normal_power  0 (off) or a power of two <= 128 default 32
 *   sigma_color   >= 0, 0: off                    default 0.5
 *   sigma_depth   >= 0, 0: off                    default 0.05
 *   demodulate    0 or 1 (ignored when albedo is NULL)  default 1
 * Anything else -- a NaN or infinite sigma included -- is RT_E_INVALID.
 *
 * Prepare.  amin = 2^-6 and floor(a) = a > amin ? a : amin.  With
 * demodulation e_0(p)[k] = (float)((double)color[k] / floor((double)albedo[k]));
 * without it e_0 = color.
 *
 * Level i = 0 .. levels - 1, with the step s = 2^i, sc = sigma_color * 2^-i
 * (exact) and h = {3/8, 1/4, 1/16}.  For every valid p, sumw = 0 and
 * sum[3] = 0 in binary64, then the taps in this order: dy = -2..2 in the outer
 * loop, dx = -2..2 in the inner loop, q = (x + s * dx, y + s * dy).  A tap is
 * skipped when q is outside the image, when q is not valid, or when object is
 * given and object[q] != object[p].  Otherwise, in this order of operations:
 *   1. w = h[|dx|] * h[|dy|]
 *   2. if normal_power > 0: t = (nx_p * nx_q + ny_p * ny_q) + nz_p * nz_q,
 *      t = t > 0 ? t : 0, t squared log2(normal_power) times, w = w * t
 *   3. if sigma_depth > 0: r = (z_q - z_p) / (sigma_depth * z_p),
 *      w = w / (1 + r * r)
 *   4. if sigma_color > 0: D = e_i(q) - e_i(p), d2 = (D0 * D0 + D1 * D1) + D2 * D2,
 *      w = w / (1 + d2 / (sc * sc))
 *   5. sumw += w and sum[k] += w * e_i(q)[k]
 * Then e_{i+1}(p)[k] = sumw > 0 ? (float)(sum[k] / sumw) : e_i(p)[k].  A pixel
 * that is not valid keeps e_i(p).
 *
 * Output, with L = levels.  A valid p gets out[k] = (float)((double)e_L[k] *
 * floor((double)albedo[k])) with demodulation and e_L without it; a pixel
 * that is not valid gets color bit for bit.  out_rgba, if given, is
 * rt_tonemap_rgba of out, byte for byte.  Either output may be NULL, but not
 * both.  out_linear == color (in place) is allowed; any other overlap carries
 * no contract.  No memory address depends on a pixel's value, so non-finite
 * colours, zero normals and depth <= 0 cannot fault; their values carry no
 * contract beyond the sumw > 0 rule.
 *
 * What it cannot do: first-hit features say nothing about what a mirror shows
 * or where a shadow falls, so reflections on metal and shadow edges are
 * blurred (DESIGN.md §4.13 has the figures); sigma_color and levels are the
 * controls for it.
 *
 * rt_denoise_async takes no context, like rt_rgba_delta_async.  Every pointer
 * of `in`, both outputs and the workspace are DEVICE pointers of the current
 * device; the caller owns the workspace (rt_denoise_workspace_bytes(w, h)
 * bytes at least, at most 64 * w * h + 256; 0 for a size rt_validate refuses),
 * nothing is allocated, and the call is asynchronous on `hip_stream`.
 * RT_E_INVALID with a message, nothing enqueued and no buffer touched: NULL
 * params or inputs, a NULL required input, both outputs NULL, a size that
 * rt_validate refuses, a NULL or too small workspace, parameters out of range.
 * rt_denoise_host does the same with host pointers and no device. */
typedef struct {
  int32_t levels;
  int32_t normal_power;
  double sigma_color;
  double sigma_depth;
  int32_t demodulate;
  int32_t _pad;
} rt_denoise;
typedef struct {
  const float* color;     /* W*H*3, required */
  const float* normal;    /* W*H*3, required */
  const float* depth;     /* W*H,   required */
  const float* albedo;    /* W*H*3 or NULL */
  const int32_t* object;  /* W*H   or NULL */
} rt_denoise_inputs;
void rt_denoise_default(rt_denoise* d);
size_t rt_denoise_workspace_bytes(int32_t width, int32_t height);
int rt_denoise_async(const rt_denoise* params, int32_t width, int32_t height, const rt_denoise_inputs* in,
                     float* d_out_linear, uint8_t* d_out_rgba, void* d_workspace, size_t workspace_bytes,
                     void* hip_stream);
int rt_denoise_host(const rt_denoise* params, int32_t width, int32_t height, const rt_denoise_inputs* in,
                    float* out_linear, uint8_t* out_rgba);

/* Temporal accumulation over a camera sequence: the previous
 * frame's accumulated colour is reprojected into the current frame through the
 * current frame's depth and the two cameras, and blended with the current
 * render, so that a moving preview of a static scene gathers samples from
 * frame to frame instead of starting from none.  It traces no ray.  The
 * project's own feature, defined here to the bit like rt_denoise_async:
 * binary64 `+ - * /`, comparisons and floor only, in one written order, floats
 * widened before use and rounded once on store, so that the device kernel,
 * rt_temporal_host and a restatement in any language agree exactly
 * (include/rt_temporal.h is the code both sides run).
 *
 * A frame (rt_temporal_frame), laid out as rt_context_render_async and
 * rt_aov_buffers lay their buffers out (pixel (x, y) at y * W + x, row 0 the
 * bottom):
 *   color   float3  required: cur = this frame's render (d_linear); prev = the
 *                   PREVIOUS CALL's out_color
 *   depth   float   required: rt_aov_buffers.d_depth of that frame
 *   object  int32   optional (NULL: no id test)
 *   normal  float3  optional (NULL: no normal test)
 *   count   float   prev only: the previous call's out_count; ignored in cur
 *   frame   12 doubles: rt_camera_frame of that frame's camera -- origin o,
 *                   lower_left l, horizontal h, vertical v_vec
 * object and normal must each be NULL in both frames or in neither.
 * valid(p) means cur.depth[p] is finite (a miss has +Inf).
 *
 * Parameters (rt_temporal; rt_temporal_default sets the defaults):
 *   max_history  >= 1, finite                          default 32
 *   depth_tol    >= 0, finite; 0: no depth test        default 0.05
 *   normal_min   in [-1, 1]; -1 stops no unit normals  default 0.9
 *   min_weight   in (0, 1]                             default 0.25
 * Anything else, NaN included, is RT_E_INVALID.
 *
 * Per call, on the host, with o', l', h', v' the previous frame's vectors and
 * dot(a, b) = (a0 * b0 + a1 * b1) + a2 * b2:
 *   g = l' - o'                       per component
 *   a = (g + h' * 0.5) + v' * 0.5     the previous camera's centre ray: its view axis
 *   aa = dot(a, a), hh = dot(h', h'), vv = dot(v', v')
 * RT_E_INVALID when any of the 24 frame doubles is not finite or when aa, hh
 * or vv is not > 0.
 *
 * Per pixel p = (x, y):
 *   1. p is not valid: out_color = cur.color bit for bit, out_count = 0.
 *   2. prev == NULL: out_color = cur.color bit for bit, out_count = 1.
 *   3. The world point.  u = (x + 0.5) / W, v = (y + 0.5) / H,
 *      dir = ((l + h * u) + v_vec * v) - o, P = o + dir * z with z = cur.depth[p],
 *      d = P - o', all per component.  `depth` is T with the view-axis component
 *      of the direction exactly 1 (see rt_aov_buffers), so no root is taken.
 *   4. Into the previous camera.  t = dot(d, a) / aa; no history unless t > 0.
 *      e = d / t - g per component; fx = (dot(e, h') / hh) * W - 0.5 and
 *      fy = (dot(e, v') / vv) * H - 0.5; no history unless
 *      fx > -1 && fx < W && fy > -1 && fy < H (comparisons a NaN fails).
 *   5. The bilinear fetch.  ix = (int)floor(fx), wx = fx - floor(fx), likewise
 *      iy and wy.  sumw, sum[3] and sumn start at 0; the taps in this order:
 *      j = 0, 1 in the outer loop, i = 0, 1 in the inner loop, q = (ix + i, iy + j).
 *      A tap is skipped when q is outside the image; when prev.depth[q] is not
 *      finite; when ids are given and prev.object[q] != cur.object[p]; when
 *      normals are given and dot(cur.normal[p], prev.normal[q]) < normal_min;
 *      when depth_tol > 0 and |prev.depth[q] - t| > depth_tol * t (|r| is
 *      r < 0 ? -r : r).  Otherwise w = (i ? wx : 1 - wx) * (j ? wy : 1 - wy),
 *      sumw += w, sum[k] += w * prev.color[q][k], sumn += w * prev.count[q].
 *      There is a history iff sumw >= min_weight.
 *   6. The blend.  hist[k] = sum[k] / sumw, n = sumn / sumw, n1 = n + 1, and
 *      n1 = max_history when n1 > max_history;
 *      out_color[k] = (float)(hist[k] + ((double)cur.color[k] - hist[k]) / n1),
 *      out_count = (float)n1.  With no history: out_color = cur.color bit for
 *      bit, out_count = 1.
 *   7. out_rgba, if given, is rt_tonemap_rgba of the stored out_color.
 * A pixel that keeps its history is the running mean of its frames until
 * max_history, then an exponential average with weight 1 / max_history.
 *
 * Every address comes from x, y and the guarded integers ix, iy: non-finite
 * colours, depth <= 0 and absurd cameras cannot fault; their values carry no
 * contract.  Taps read neighbours, so out_color / out_count must not be
 * prev.color / prev.count -- the caller ping-pongs two pairs of buffers; equal
 * pointers are refused, any other overlap carries no contract.
 *
 * What it can and cannot do.  `depth` is the MEAN T of a pixel's jittered
 * samples, so P is the pixel centre's surface point only to within the pixel's
 * footprint: at a silhouette or a sharp edge the mean mixes surfaces, and the
 * depth, id and normal tests are what reject such taps.  The scene is static,
 * so direct light and shadows reproject correctly.  What a mirror SHOWS does
 * not: a reflection moves differently from the surface that carries it, so
 * reflections on metal lag and smear while the camera moves (DESIGN.md §4.14
 * has the figures).  max_history is the control for that: it bounds how long
 * an old frame keeps its weight.
 *
 * rt_temporal_async needs no workspace and no context and allocates nothing.
 * Every buffer pointer is a DEVICE pointer of the current device; the structs
 * are read before the call returns; the call is asynchronous on `hip_stream`.
 * d_out_rgba may be NULL.  RT_E_INVALID with a message, nothing enqueued and
 * no buffer touched: NULL params or cur; a NULL color or depth; a NULL
 * prev.count; object or normal given in one frame only; NULL d_out_color or
 * d_out_count; d_out_color == prev.color or d_out_count == prev.count; a size
 * that rt_validate refuses; parameters out of range; the frame rules above.
 * rt_temporal_host does the same with host pointers and no device. */
typedef struct { double max_history; double depth_tol; double normal_min; double min_weight; } rt_temporal;
typedef struct {
  const float* color;     /* W*H*3, required */
  const float* depth;     /* W*H,   required */
  const int32_t* object;  /* W*H   or NULL */
  const float* normal;    /* W*H*3 or NULL */
  const float* count;     /* W*H,   prev only */
  double frame[12];       /* rt_camera_frame: origin, lower_left, horizontal, vertical */
} rt_temporal_frame;
void rt_temporal_default(rt_temporal* t);
int rt_temporal_async(const rt_temporal* params, int32_t width, int32_t height, const rt_temporal_frame* cur,
                      const rt_temporal_frame* prev /* NULL: start a history */, float* d_out_color,
                      float* d_out_count, uint8_t* d_out_rgba /* may be NULL */, void* hip_stream);
int rt_temporal_host(const rt_temporal* params, int32_t width, int32_t height, const rt_temporal_frame* cur,
                     const rt_temporal_frame* prev, float* out_color, float* out_count, uint8_t* out_rgba);

/* Variance-guided denoising: temporal accumulation also
 * gathers the first two moments of the demodulated luminance, a variance pass
 * turns them into the per-pixel variance of the accumulated colour, and a
 * second à-trous filter scales its luminance stop by that variance, pixel by
 * pixel.  A pixel whose frames agree (a static reflection, a sharp shadow
 * edge) has a low variance and keeps its detail; one whose frames disagree
 * (soft-shadow and bounce noise) is smoothed.  Three calls beside
 * rt_temporal_async and rt_denoise_async, which stay what they are; all three
 * trace no ray and are defined to the bit like those: binary64 `+ - * /`,
 * comparisons and floor only, in one written order, floats widened before use
 * and rounded once on store (include/rt_variance.h is the code the kernels and
 * the _host twins run).  No address depends on a pixel's value, so non-finite
 * colours, moments and variances, zero normals and depth <= 0 cannot fault;
 * their values carry no contract.
 *
 * Common definitions, all in binary64:
 *   floor(a)    = a > 2^-6 ? a : 2^-6                      (rt_denoise_async's)
 *   e(c, a)[k]  = albedo given ? (double)c[k] / floor((double)a[k]) : (double)c[k]
 *                 (not rounded to binary32 in between)
 *   lum(e)      = (0.2126 * e0 + 0.7152 * e1) + 0.0722 * e2
 *   valid(p)    : depth[p] is finite
 *
 * 1. rt_temporal_moments_async: rt_temporal_async with three more buffers,
 *      cur_albedo    float3  optional: the current frame's albedo (NULL: lum of the colour itself)
 *      prev_moments  float2  required exactly when prev is given: the PREVIOUS CALL's out_moments
 *      out_moments   float2  required
 *    out_color, out_count and out_rgba are rt_temporal_async's, bit for bit, for
 *    every input: its steps 1 to 7 in its order.  Per pixel p,
 *    l = lum(e(cur.color[p], cur_albedo[p])) and mcur = (l, l * l).  Where step
 *    5 accepts a tap q with weight w it also continues
 *    summ[j] += w * (double)prev_moments[q][j] (j = 0, 1; after sumn), and where
 *    step 6 finds a history, hm[j] = summ[j] / sumw and
 *    out_moments[j] = (float)(hm[j] + (mcur[j] - hm[j]) / n1) with step 6's n1.
 *    In every other case (p not valid, prev NULL, no history)
 *    out_moments = ((float)l, (float)(l * l)).
 *    Refused like rt_temporal_async, and also: prev given without prev_moments
 *    or prev_moments without prev; a NULL out_moments; out_moments ==
 *    prev_moments (the third ping-pong pair).
 *
 * 2. rt_variance_async: the variance of the accumulated demodulated luminance.
 *    Inputs (rt_variance_inputs): color (the accumulated colour), normal and
 *    depth required; albedo and object optional; moments (float2) and count
 *    optional, both or neither.  Parameters (rt_variance; rt_variance_default):
 *      min_history   >= 1, finite                          default 4
 *      normal_power  0 (off) or a power of two <= 128      default 32
 *      sigma_depth   >= 0, finite; 0: off                  default 0.05
 *    Per pixel p, out_var[p] is
 *      0 when p is not valid; otherwise, with
 *      n = count given ? ((double)count[p] > 1 ? (double)count[p] : 1) : 1:
 *      temporal (moments given and (double)count[p] >= min_history):
 *        v = m2 - m1 * m1 with (m1, m2) = moments[p]; v = v > 0 ? v : 0;
 *        out_var = (float)(v / n).
 *      spatial (otherwise): sumw, s1, s2 start at 0; the 49 taps q = (x + dx,
 *        y + dy) with dy = -3..3 in the outer and dx = -3..3 in the inner loop.
 *        A tap is skipped when q is outside the image, not valid, or object is
 *        given and object[q] != object[p].  Otherwise w = 1, then steps 2 and 3
 *        of rt_denoise_async's tap weight (normal, depth) on w;
 *        (m1q, m2q) = moments[q] when moments is given, else lq = lum(e(color[q],
 *        albedo[q])) and (lq, lq * lq); s1 += w * m1q, s2 += w * m2q, sumw += w.
 *        Then a = s1 / sumw, v = s2 / sumw - a * a, v = v > 0 ? v : 0 and
 *        out_var = sumw > 0 ? (float)(v / n) : 0.
 *    The division by n makes it the variance of the MEAN of n samples; where
 *    the history is shorter than min_history the neighbourhood stands in for it.
 *
 * 3. rt_denoise_var_async: rt_denoise_async's inputs plus variance (float,
 *    required).  Parameters (rt_denoise_var; rt_denoise_var_default):
 *      levels, normal_power, sigma_depth, demodulate   as rt_denoise
 *      sigma_lum   >= 0, finite; 0: the luminance stop is off   default 2
 *      prefilter   0 or 1                                       default 1
 *    Prepare, the 25 taps and their order, the skip rules, steps 1 to 3 and 5,
 *    the sumw > 0 rule, remodulation, the tone map and the in-place rule are
 *    rt_denoise_async's.  The differences: every pixel carries var_i(p), with
 *    var_0 = variance.  Per level i and valid p, when sigma_lum > 0:
 *      g = (double)var_i(p) without the prefilter.  With it, sumg = sumk = 0,
 *        then the 9 taps q = (x + dx, y + dy) -- step 1 at every level -- with
 *        dy = -1..1 outer and dx = -1..1 inner, skipped by the same rules,
 *        k = {1/4, 1/8, 1/16}[|dx| + |dy|], sumg += k * (double)var_i(q),
 *        sumk += k; g = sumg / sumk.
 *      inv = 1 / ((sigma_lum * sigma_lum) * g + 2^-40), once per pixel.
 *    Step 4 becomes: if sigma_lum > 0, d = lum(e_i(q)) - lum(e_i(p)) (the
 *    binary32 records widened) and w = w / (1 + (d * d) * inv).  Step 5 also
 *    continues sumv += (w * w) * (double)var_i(q) (after sum[2]), and
 *    var_{i+1}(p) = sumw > 0 ? (float)(sumv / (sumw * sumw)) : var_i(p); a pixel
 *    that is not valid keeps var_i(p).  Outputs: d_out_linear and d_out_rgba as
 *    rt_denoise_async's (either may be NULL, not both); d_out_variance, if
 *    given, is var_levels.  out_linear == color and out_variance == variance
 *    (in place) are allowed; any other overlap carries no contract.
 *    With sigma_lum = 0 the colour is rt_denoise_async's with sigma_color = 0,
 *    bit for bit.
 *
 * Calls.  Every buffer pointer of an _async call is a DEVICE pointer of the
 * current device; the structs are read before the call returns; the calls are
 * asynchronous on `hip_stream`, take no context and allocate nothing.  The
 * moments and the variance pass need no workspace; the caller owns the
 * filter's (rt_denoise_var_workspace_bytes(w, h) bytes at least, at most
 * 64 * w * h + 256; 0 for a size rt_validate refuses).  RT_E_INVALID with a
 * message, nothing enqueued and no buffer touched: what is listed above; NULL
 * params or inputs; a NULL required buffer; a size that rt_validate refuses;
 * parameters out of range, NaN included; a NULL or too small workspace.  The
 * _host twins do the same with host pointers and no device. */
typedef struct { double min_history; double sigma_depth; int32_t normal_power; int32_t _pad; } rt_variance;
typedef struct {
  const float* color;     /* W*H*3, required */
  const float* normal;    /* W*H*3, required */
  const float* depth;     /* W*H,   required */
  const float* albedo;    /* W*H*3 or NULL */
  const int32_t* object;  /* W*H   or NULL */
  const float* moments;   /* W*H*2 or NULL */
  const float* count;     /* W*H   or NULL: given exactly when moments is */
} rt_variance_inputs;
typedef struct {
  int32_t levels;
  int32_t normal_power;
  double sigma_lum;
  double sigma_depth;
  int32_t demodulate;
  int32_t prefilter;
} rt_denoise_var;
int rt_temporal_moments_async(const rt_temporal* params, int32_t width, int32_t height, const rt_temporal_frame* cur,
                              const rt_temporal_frame* prev /* NULL: start a history */,
                              const float* d_cur_albedo /* may be NULL */, const float* d_prev_moments,
                              float* d_out_color, float* d_out_count, float* d_out_moments,
                              uint8_t* d_out_rgba /* may be NULL */, void* hip_stream);
int rt_temporal_moments_host(const rt_temporal* params, int32_t width, int32_t height, const rt_temporal_frame* cur,
                             const rt_temporal_frame* prev, const float* cur_albedo, const float* prev_moments,
                             float* out_color, float* out_count, float* out_moments, uint8_t* out_rgba);
void rt_variance_default(rt_variance* v);
int rt_variance_async(const rt_variance* params, int32_t width, int32_t height, const rt_variance_inputs* in,
                      float* d_out_var, void* hip_stream);
int rt_variance_host(const rt_variance* params, int32_t width, int32_t height, const rt_variance_inputs* in,
                     float* out_var);
void rt_denoise_var_default(rt_denoise_var* d);
size_t rt_denoise_var_workspace_bytes(int32_t width, int32_t height);
int rt_denoise_var_async(const rt_denoise_var* params, int32_t width, int32_t height, const rt_denoise_inputs* in,
                         const float* d_variance, float* d_out_linear, uint8_t* d_out_rgba,
                         float* d_out_variance /* may be NULL */, void* d_workspace, size_t workspace_bytes,
                         void* hip_stream);
int rt_denoise_var_host(const rt_denoise_var* params, int32_t width, int32_t height, const rt_denoise_inputs* in,
                        const float* variance, float* out_linear, uint8_t* out_rgba, float* out_variance);

/* Temporal accumulation with per-object motion: the
 * accumulation above for scenes whose objects move between the frames of a
 * sequence.  rt_temporal_async assumes that nothing but the camera moved, so
 * an object that moves loses its history, and where it overlaps its old place
 * it blends in another surface point.  Here every hittable has a translation
 * from the previous frame to the current one, and a pixel's world point is
 * moved back by its object's before it is taken into the previous camera.
 *
 * The table (rt_motion): `motion` holds num_objects rows of 3 doubles, row k
 * the translation of hittable k from the previous frame to the current one
 * (position in cur minus position in prev).  Hittable k is the rt_object index
 * that the `object` buffers hold (rt_aov_buffers.d_object).  rt_scene_motion
 * makes the table from two scenes.
 *
 * Per pixel, every step is rt_temporal_async's, and rt_temporal_moments_async's
 * when out_moments is given, bit for bit and in their order.  The one addition
 * is in step 3: after P = o + dir * z, let id = cur.object[p];
 * m = motion[id] when 0 <= id < num_objects, else m = (0, 0, 0);
 * Pm = P - m and d = Pm - o', per component.  t, fx, fy and the depth test of
 * steps 4 and 5 then refer to where that surface point WAS.  The id test and
 * the normal test are unchanged: a translation keeps both.
 *   - With a table of zeros every output equals the existing calls' bit for
 *     bit, for every input: x - 0.0 is x, signed zeros and NaNs included.
 *   - id is compared against the table's bounds before it forms an address;
 *     that guarded address is the only one that comes from a pixel's value.
 *   - Non-finite table entries cannot fault and carry no contract.
 *
 * Moments.  Without out_moments, cur_albedo and prev_moments must be NULL and
 * the call is the colour-only form (rt_temporal_async's outputs).  With it,
 * rt_temporal_moments_async's rules apply (cur_albedo optional, prev_moments
 * exactly when prev is given, out_moments != prev_moments).
 *
 * rt_temporal_motion_async: every buffer pointer, the table included, is a
 * DEVICE pointer of the current device; the rt_motion struct itself is read on
 * the host before the call returns.  No workspace, no context, no allocation;
 * asynchronous on `hip_stream`.  RT_E_INVALID with a message, nothing enqueued
 * and no buffer touched: whatever rt_temporal_async (or, with out_moments,
 * rt_temporal_moments_async) refuses; a NULL motion or a NULL table;
 * num_objects < 1; a NULL object in either frame (the table is indexed by it,
 * so ids are required here); cur_albedo or prev_moments without out_moments.
 * rt_temporal_motion_host does the same with host pointers and no device.
 *
 * rt_scene_motion runs on the host and needs no device.  It writes
 * out[k * 3 + j] = cur.objects[k].position[j] - prev.objects[k].position[j] and
 * returns num_objects.  RT_E_INVALID when the scenes differ in their object
 * count or in any object's type, size, radius or material (a rigid translation
 * is the only motion this models), when a position is not finite, or when
 * capacity (in doubles) is below num_objects * 3.  Lights and cameras are not
 * compared: the camera reaches the pass through the frames, and a moving light
 * is the caller's business.
 *
 * Known limits.  A static pixel under a moving object's shadow keeps its old
 * history, and what a moving mirror shows does not reproject (its lighting
 * changes as it moves; DESIGN.md §4.17 has the figures).  max_history bounds
 * both, and rt_temporal_clip_async (below) rectifies them.  Rotations and
 * deformations are not modelled. */
typedef struct {
  const double* motion;  /* num_objects * 3 */
  int32_t num_objects;
  int32_t _pad;
} rt_motion;
int rt_temporal_motion_async(const rt_temporal* params, int32_t width, int32_t height, const rt_temporal_frame* cur,
                             const rt_temporal_frame* prev /* NULL: start a history */,
                             const rt_motion* motion /* device table */, const float* d_cur_albedo,
                             const float* d_prev_moments, float* d_out_color, float* d_out_count,
                             float* d_out_moments /* may be NULL */, uint8_t* d_out_rgba /* may be NULL */,
                             void* hip_stream);
int rt_temporal_motion_host(const rt_temporal* params, int32_t width, int32_t height, const rt_temporal_frame* cur,
                            const rt_temporal_frame* prev, const rt_motion* motion, const float* cur_albedo,
                            const float* prev_moments, float* out_color, float* out_count, float* out_moments,
                            uint8_t* out_rgba);
int rt_scene_motion(const rt_scene* prev, const rt_scene* cur, double* out, size_t capacity);

/* History rectification: temporal accumulation that clips
 * the reprojected history to what the current frame's neighbourhood allows.
 * Every pass above reprojects geometry; none looks at whether the light a
 * surface point receives has changed, so a static pixel under a moving shadow,
 * what a moving mirror shows, a reflection under a moving camera and
 * everything under a moving light keep a history that no longer holds.  Here
 * the history colour is clipped to mean +- gamma * sigma of the demodulated
 * colour around the pixel in the CURRENT frame (variance clipping) before the
 * blend: a history the current frame contradicts by many sigma is pulled to
 * the edge of that range, one that agrees is left alone to the bit.
 *
 * The arguments are rt_temporal_motion_async's plus `clip` (rt_history_clip;
 * rt_history_clip_default) and the optional output out_clipped (float, W*H).
 *   radius    the window is (2 * radius + 1)^2; 0 (off) to 4
 *   min_taps  >= 1: no clip where the window has fewer valid taps
 *   gamma     finite and >= 0: the range's half width in sigmas
 *   min_half  finite and >= 0: added to the half width
 * Anything else, NaN included, is RT_E_INVALID.
 *
 * `motion` may be NULL here: then m = 0 and `object` is optional (NULL in both
 * frames or in neither), as in rt_temporal_async.  With a table ids are
 * required, as in rt_temporal_motion_async.
 *
 * Per pixel p = (x, y), steps 1 to 5 and 7 are rt_temporal_motion_async's, or
 * the moments form's when out_moments is given, bit for bit and in their
 * order.  Between step 5 and step 6, only where step 5 found a history and
 * radius > 0:
 *   5a. The window.  e(q)[k] = rt_variance's e(cur.color[q], cur_albedo[q])[k]:
 *       binary64 color / max(albedo, floor), the plain colour when cur_albedo
 *       is NULL.  nw = 0, s1[3] = s2[3] = 0.  Taps q = (x + dx, y + dy), dy =
 *       -r..r outer, dx = -r..r inner.  A tap is skipped when q is outside the
 *       image, when cur.depth[q] is not finite, or when ids are given and
 *       cur.object[q] != cur.object[p].  Otherwise nw += 1 and per k
 *       s1[k] += e, s2[k] += e * e.  If nw < min_taps there is no clip.  Else
 *       mu[k] = s1[k] / nw, var[k] = s2[k] / nw - mu[k] * mu[k],
 *       var = var > 0 ? var : 0, half[k] = gamma * sqrt(var[k]) + min_half
 *       (binary64 sqrt, correctly rounded).
 *   5b. The clip.  hist[k] = sum[k] / sumw (step 6's value), fa[k] =
 *       max(cur_albedo[p][k], floor) or 1 without albedo, he[k] = hist[k] /
 *       fa[k], lo = mu[k] - half[k], hi = mu[k] + half[k],
 *       hc[k] = he < lo ? lo : (he > hi ? hi : he); a NaN fails both
 *       comparisons and stays.  Where hc[k] != he[k], step 6 blends with
 *       hc[k] * fa[k] in that channel; where not, with hist[k] unchanged (no
 *       round trip through the division).  (A NaN compares unequal to
 *       itself: a NaN history is blended as hc * fa, a NaN again, and counts
 *       as clipped.  A NaN mu or half clips nothing.)
 *   out_clipped[p] = 1 when a channel was replaced, else 0; 0 for every pixel
 *   without a history.
 * n, the count and the moment sums are untouched: the moments keep the old
 * frames, so the variance of a clipped pixel stays high and the
 * variance-guided filter smooths it.
 *   - radius = 0: every output equals rt_temporal_motion_async's bit for bit,
 *     for every input; with motion = NULL, rt_temporal_async's or
 *     rt_temporal_moments_async's.
 *   - Every address comes from x, y, dx, dy and bounds checks; the one guarded
 *     address from a pixel's value is the motion table's.
 *
 * cur_albedo.  It demodulates the window, so it may be given WITHOUT
 * out_moments here (the one rule looser than the calls this extends);
 * prev_moments without out_moments is refused as there.
 *
 * rt_temporal_clip_async: device pointers, no workspace, no context, no
 * allocation; asynchronous on `hip_stream`.  RT_E_INVALID with a message,
 * nothing enqueued and no buffer touched: whatever the call it extends refuses
 * (rt_temporal_motion_async with a table, rt_temporal_async /
 * rt_temporal_moments_async without), a NULL clip, a parameter out of range,
 * out_clipped equal to another output.  rt_temporal_clip_host does the same
 * with host pointers and no device.
 *
 * Known limits.  The range is as wide as the current frame's noise: at 1 spp a
 * history inside mean +- gamma * sigma passes although it is stale, so slow
 * changes (a soft shadow's edge, a rough reflection) are narrowed, not removed
 * (DESIGN.md §4.18 and §9 have the figures). */
typedef struct {
  int32_t radius;
  int32_t min_taps;
  double gamma;
  double min_half;
} rt_history_clip;
void rt_history_clip_default(rt_history_clip* c);
int rt_temporal_clip_async(const rt_temporal* params, int32_t width, int32_t height, const rt_temporal_frame* cur,
                           const rt_temporal_frame* prev /* NULL: start a history */,
                           const rt_motion* motion /* device table; may be NULL */, const rt_history_clip* clip,
                           const float* d_cur_albedo, const float* d_prev_moments, float* d_out_color,
                           float* d_out_count, float* d_out_moments /* may be NULL */,
                           float* d_out_clipped /* may be NULL */, uint8_t* d_out_rgba /* may be NULL */,
                           void* hip_stream);
int rt_temporal_clip_host(const rt_temporal* params, int32_t width, int32_t height, const rt_temporal_frame* cur,
                          const rt_temporal_frame* prev, const rt_motion* motion, const rt_history_clip* clip,
                          const float* cur_albedo, const float* prev_moments, float* out_color, float* out_count,
                          float* out_moments, float* out_clipped, uint8_t* out_rgba);

/* The coverage-aware edge resolve: antialias the silhouettes
 * of a low-sample image from an OBJECT-level matte.  Every filter above stops
 * at object ids, so a 1-spp pixel on an object's edge stays one sample of one
 * object, where the converged picture holds a blend of two.  Here a pixel that
 * sees more than one object takes each object's share of its matte samples
 * times that object's colour, gathered from the neighbours that belong to it.
 * A pixel that sees one object is not changed at all.  Context-free like
 * rt_denoise_async.
 *
 * Inputs, image layout, pixel (x, y) at p = y * W + x:
 *   color   float3, required   any linear image of the frame: raw, denoised or accumulated
 *   object  int32, required    the frame's d_object: whose colour color[q] is
 *   id, count  K planes of int32 each, required: d_id and d_count of an
 *              RT_MATTE_OBJECT matte of the frame with K ranks
 *   rest    int32, optional    its d_rest; NULL counts as 0 everywhere
 *   samples n >= 1             the matte's sample count
 * Parameters (rt_matte_resolve; rt_matte_resolve_default):
 *   radius      R in 1..4, default 2: the gather window is (2R + 1)^2
 *   background  finite, default 0: the colour behind everything
 *
 * The arithmetic is binary64 `+ - * /` and comparisons only, floats widened
 * before use and rounded once on store.  Per pixel p:
 *   1. The parts, in this order: the ranks r = 0..K-1 with count_r[p] > 0, key
 *      id_r[p]; the miss part with count = n - sum(those count_r) - rest[p]
 *      and key -1, if that count is positive; the rest part with count
 *      rest[p], if rest[p] > 0.  With fewer than two parts out = color[p] bit
 *      for bit.
 *   2. A rank or miss part's colour: sw = 0, sc[3] = 0; dy = -R..R outer,
 *      dx = -R..R inner, q = (x + dx, y + dy); a tap is skipped when q is
 *      outside the image or object[q] != key; otherwise
 *      w = 1 / (1 + (dx * dx + dy * dy)), sw += w, sc[k] += w * color[q][k].
 *      The colour is sc[k] / sw when sw > 0, else background[k] for the miss
 *      part and color[p][k] for a rank.  The rest part's colour is color[p].
 *   3. acc[3] = 0; in part order acc[k] += ((double)count / (double)n) *
 *      part[k]; out[k] = (float)acc[k].
 * out_rgba, if given, is rt_tonemap_rgba of the stored out.
 *   - Every address comes from x, y, dx, dy and r: no input value can cause a
 *     fault.  Counts whose sum exceeds n carry no contract on their values.
 *   - Shares are geometric: a shadow's edge or a reflection's edge is not a
 *     part and is untouched.  An object whose only visible pixels are mixed
 *     has no neighbour to gather from and keeps the pixel's own colour.
 *
 * rt_matte_resolve_async: device pointers, no workspace, no context, no
 * allocation; asynchronous on `hip_stream`.  RT_E_INVALID with a message,
 * nothing enqueued and no buffer touched: a NULL params, color, object, id or
 * count; both outputs NULL; out_linear == color (taps read neighbours); a size
 * that rt_validate refuses; ranks outside 1..RT_MATTE_MAX_RANKS; samples < 1;
 * radius outside 1..4; a background that is not finite.
 * rt_matte_resolve_host does the same with host pointers and no device. */
typedef struct {
  int32_t radius;
  int32_t _pad;
  double background[3];
} rt_matte_resolve;
typedef struct {
  const float* color;     /* W*H*3 */
  const int32_t* object;  /* W*H   */
  const int32_t* id;      /* ranks * W*H */
  const int32_t* count;   /* ranks * W*H */
  const int32_t* rest;    /* W*H, or NULL */
  int32_t ranks;          /* K */
  int32_t samples;        /* n */
} rt_matte_resolve_inputs;
void rt_matte_resolve_default(rt_matte_resolve* r); /* radius 2, background 0 */
int rt_matte_resolve_async(const rt_matte_resolve* params, int32_t width, int32_t height,
                           const rt_matte_resolve_inputs* in, float* d_out_linear /* may be NULL */,
                           uint8_t* d_out_rgba /* may be NULL */, void* hip_stream);
int rt_matte_resolve_host(const rt_matte_resolve* params, int32_t width, int32_t height,
                          const rt_matte_resolve_inputs* in, float* out_linear, uint8_t* out_rgba);

/* What a context has done so far (diagnostics): work schedules built (a new
 * scene, frame, rank or settings key; a measured re-cut counts too),
 * measuring frames (rt_tuning.measure), frames rendered, render launches,
 * and the launches that rendered several frames at once. */
typedef struct {
  int64_t schedules_built, measuring_frames, frames, launches, batched_launches;
  int64_t blocks, split_pixels;  /* of the schedule last used: work blocks, pixels split over sub-blocks */
  /* tail helpers (rt_tuning.tail_*): paths exported to them since the
   * context's tail buffers were laid out, and a helper error word (0: none);
   * reading them waits for the context's last render */
  int64_t tail_exported, tail_errors;
  /* streamed launches (rt_tuning.stream): stream + resolve kernel pairs enqueued (a launch split under the
   * row budget counts one per group of frames), and the live pixels of the schedule last used (-1: the
   * schedule has no live-pixel list) */
  int64_t stream_launches, stream_live_pixels;
} rt_context_stats;
int rt_context_get_stats(const rt_context* ctx, rt_context_stats* out);
/* Debug (tail helpers), cumulative since the context's tail
 * buffers were laid out: out[0] paths exported, [1] paths the helpers ran,
 * [2] helpers' ticks running paths, [3] exporting waves' ticks in the export,
 * [4] helpers' lifetime ticks, [5] error word (ticks: s_memrealtime, 100 MHz).
 * Waits for the context's last render; all zero when no launch used helpers. */
int rt_context_tail_debug(const rt_context* ctx, uint64_t out[6]);

/* Packed share of one rank, as rt_comm_gather_tiles_async moves it:
 * [max_local_tiles * 1024 float3][max_local_tiles * 1024 RGBA8] = 16 B per
 * pixel of the largest share (rank 0's).  Render a share with layout
 * RT_LAYOUT_PACKED_TILES, d_linear = share, d_rgba = share + rt_packed_rgba_offset(). */
int32_t rt_max_local_tiles(int32_t width, int32_t height, int32_t world);
size_t rt_packed_bytes(int32_t width, int32_t height, int32_t world);
size_t rt_packed_rgba_offset(int32_t width, int32_t height, int32_t world);

/* Scatter the gathered shares [world][rt_packed_bytes] into W*H images
 * (d_linear float3 and/or d_rgba; either may be NULL). */
int rt_unpack_tiles_async(int32_t width, int32_t height, int32_t world, const void* d_gathered, float* d_linear,
                          uint8_t* d_rgba, void* hip_stream);

/* ---------------------------------------------- RCCL tile gather (xGMI) */

/* One communicator per process for multi-process runs (one process per GPU,
 * e.g. torch.distributed.run): rank 0 makes the id (ncclGetUniqueId), the
 * caller broadcasts its RT_COMM_ID_BYTES bytes, every rank calls
 * rt_comm_create (ncclCommInitRank) on its device. */
#define RT_COMM_ID_BYTES 128
typedef struct rt_comm rt_comm;
int rt_comm_unique_id(uint8_t* id);
int rt_comm_create(const uint8_t* id, int32_t world, int32_t rank, int32_t device, rt_comm** out);
void rt_comm_destroy(rt_comm* comm);
/* The frame's one collective: rank r > 0 sends its packed share
 * (rt_packed_bytes, device pointer d_share) to rank 0, which receives it
 * into d_gathered + r * rt_packed_bytes (one ncclSend/ncclRecv group on
 * `hip_stream`).  Rank 0 renders its own share into d_gathered directly
 * (d_share == d_gathered: nothing to copy). */
int rt_comm_gather_tiles_async(rt_comm* comm, int32_t width, int32_t height, const void* d_share, void* d_gathered,
                               void* hip_stream);

/* ------------------------------------------------ tile partitions (N ranks) */

/* createRenderTasks hands 32x32 tiles to the goroutines through one channel
 * (renderer.go:398-436), so a slow tile never holds the others up.  Ranks on
 * separate GPUs share no queue: each renders a fixed set of tiles.  The
 * default set is strided (t % world == rank).  A frame whose work sits in a
 * few tiles (the headline scene: 23 of its 475 tiles hold all the shading)
 * is better dealt by work: rt_partition_balanced renders the whole frame
 * once on ctx's device with every sample's path length recorded (DESIGN.md
 * §5; frames with more than 1024 samples, a sky or a BVH: the schedule's
 * one-sample pilot estimate instead), sums each tile's path work and deals
 * the tiles heaviest first to the least loaded rank.  Both are
 * deterministic, so every rank that plans the same frame derives the same
 * partition.  Every
 * pixel stays on one rank and the random stream is keyed by global pixel and
 * sample: the image is the same for every partition.
 * A rank's packed share holds its tiles in ascending order (local tile lt =
 * the lt-th of its tiles); every share is sized for the largest. */
typedef struct rt_partition rt_partition;
/* owner[t] = rank of tile t (rt_num_tiles entries, each in [0, world)); NULL: strided. */
int rt_partition_create(int32_t width, int32_t height, int32_t world, const int32_t* owner, rt_partition** out);
/* ctx must hold the scene (rt_context_set_scene); synchronous. */
int rt_partition_balanced(rt_context* ctx, int32_t width, int32_t height, const rt_settings* settings, int32_t world,
                          rt_partition** out);
void rt_partition_destroy(rt_partition* p);
int32_t rt_partition_world(const rt_partition* p);
int32_t rt_partition_owner(const rt_partition* p, int32_t tile);      /* -1: no such tile */
int32_t rt_partition_local_tiles(const rt_partition* p, int32_t rank); /* tiles of `rank` */
int32_t rt_partition_tile(const rt_partition* p, int32_t rank, int32_t local); /* its local-th tile, -1: none */
int32_t rt_partition_max_local(const rt_partition* p);
size_t rt_partition_packed_bytes(const rt_partition* p);  /* one share: max_local * 1024 * 16 */
size_t rt_partition_rgba_offset(const rt_partition* p);   /* max_local * 1024 * 12 */
/* Work of rank's tiles (path bounces summed over samples; balanced partitions, else 0). */
double rt_partition_work(const rt_partition* p, int32_t rank);
/* Later renders of ctx with the partition's (W, H, world) render rank's tiles
 * of it (packed: in its order); NULL (or other sizes): strided.  The
 * partition is copied: it may be destroyed afterwards. */
int rt_context_set_partition(rt_context* ctx, const rt_partition* p);
/* rt_unpack_tiles_async for a partition's shares ([world][rt_partition_packed_bytes]). */
int rt_unpack_partition_async(const rt_partition* p, const void* d_gathered, float* d_linear, uint8_t* d_rgba,
                              void* hip_stream);
/* The same for nframes frames gathered as [world][nframes][packed bytes] (each
 * rank's frames contiguous: one send per rank) into [nframes][W*H] images. */
int rt_unpack_partition_frames_async(const rt_partition* p, int32_t nframes, const void* d_gathered, float* d_linear,
                                     uint8_t* d_rgba, void* hip_stream);
/* rt_comm_gather_tiles_async with shares of share_bytes (a partition's packed bytes). */
int rt_comm_gather_bytes_async(rt_comm* comm, size_t share_bytes, const void* d_share, void* d_gathered,
                               void* hip_stream);
/* Per rank of the renderer's last render: device seconds of its render launches
 * (out[capacity], capacity >= rt_renderer_num_ranks(r), else RT_E_INVALID) --
 * the load balance of a multi-GPU frame. */
int rt_renderer_rank_seconds(const rt_renderer* r, double* out, int32_t capacity);
/* The renderer's rank count (the device list given to rt_renderer_create). */
int32_t rt_renderer_num_ranks(const rt_renderer* r);

/* Debug hook: a device buffer of 48 u64 per workgroup that
 * RT_WG_TIMING builds of the kernel fill: s_memrealtime at start / loop end
 * / end, then s_memtime clocks spent in closest hit, lighting and soft
 * shadows, coop/sequential soft-shadow counts and loop iterations
 * (scripts/wg_timing.py).  Product builds ignore it. */
int rt_context_set_debug_buffer(rt_context* ctx, void* d_buf);

/* Per-kernel device time of the wavefront path (BVH scenes):
 * with profiling on, HIP events are recorded at every kernel boundary of the
 * bounce loop on the render's stream; rt_context_kernel_seconds waits for
 * them and returns each kernel class's total seconds and launches since
 * profiling was switched on, in the order of RT_WF_*.  (The megakernel path
 * records nothing here: rt_context_last_kernel_seconds is its one launch.) */
#define RT_WF_EXTEND 0       /* closest hit of the live paths (hitWorld, renderer.go:333-346) */
#define RT_WF_SHADE1 1       /* hit records + hard shadow rays queued */
#define RT_WF_OCCLUDE_HARD 2 /* any-hit of the hard shadow rays (renderer.go:305) */
#define RT_WF_CONE 3         /* shadow cones of the clear hard rays: candidate lists (renderer.go:311-320) */
#define RT_WF_SOFTGEN 4      /* the 16 jittered points per clear light (renderer.go:311-318) */
#define RT_WF_CONE_RAYS 5    /* the soft rays of cones with a candidate list, against the list */
#define RT_WF_OCCLUDE_SOFT 6 /* any-hit of the other soft shadow rays through the BVH (renderer.go:320) */
#define RT_WF_SHADE 7        /* direct lighting + scatter (renderer.go:181-297) */
#define RT_WF_REGEN 8        /* new camera samples + loop bookkeeping */
#define RT_WF_RESOLVE 9      /* per-pixel in-order sums, tone map, write */
#define RT_WF_KERNELS 10
int rt_context_profile(rt_context* ctx, int32_t on);  /* on / off; resets the totals */
int rt_context_kernel_seconds(rt_context* ctx, double* seconds /* RT_WF_KERNELS */,
                              int64_t* launches /* RT_WF_KERNELS or NULL */);

/* Device time (seconds) of the last render launch enqueued on this context
 * (HIP events recorded around it on its stream); waits for it. */
int rt_context_last_kernel_seconds(rt_context* ctx, double* seconds);

/* ------------------------------------------------------------ output */

/* toneMap + ToRGB on host (renderer.go:348-367; vector.go:106-109). */
void rt_tonemap_rgba(const float* linear_rgb, int32_t npix, uint8_t* out_rgba);
/* SaveImage — renderer.go:438-451 (PNG, opaque 8-bit RGB like Go's encoder). */
int rt_write_png(const char* path, const uint8_t* rgba, int32_t width, int32_t height);
/* SavePPMFromVec3-style P3 writer (internal/output/ppm.go:34-59), from RGBA8. */
int rt_write_ppm(const char* path, const uint8_t* rgba, int32_t width, int32_t height);

#ifdef __cplusplus
}
#endif
#endif /* RT_API_H */
