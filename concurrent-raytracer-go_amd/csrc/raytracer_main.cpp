// raytracer_main.cpp — CLI mirroring cmd/raytracer/main.go:14-70.
//
//   raytracer <scene_file> <output_file> <width> <height>
//             [--samples N] [--max-depth N] [--seed N] [--no-soft-shadows]
//             [--no-recursive] [--devices N] [--watchdog SECONDS]
//             [--sky default|white|sunset|night] [--camera reference|lookat]
//             [--pass-samples N [--time-budget SECONDS] [--converge PIXELS]
//              [--adaptive TOL[,PATIENCE[,MIN]]] [--count-map FILE]]
//             [--orbit N[,DEGREES]] [--aov PREFIX]
//             [--denoise default|LEVELS[,SIGMA_COLOR[,SIGMA_DEPTH[,NORMAL_POWER]]]]
//             [--temporal default|MAX_HISTORY[,DEPTH_TOL[,NORMAL_MIN]]]
//             [--denoise-variance default|LEVELS[,SIGMA_LUM[,SIGMA_DEPTH[,NORMAL_POWER]]]]
//             [--aov-specular default|BOUNCES[,MAX_ROUGHNESS]]
//             [--move K:DX,DY,DZ]...
//             [--clip default|RADIUS[,GAMMA[,MIN_TAPS[,MIN_HALF]]]]
//             [--matte PREFIX[,SAMPLES[,RANKS[,object|face]]]]
//             [--edge-resolve default|SAMPLES[,RADIUS]]
//
// Same positional arguments, stdout lines, ".png" default extension
// (main.go:53-56) and benchmark_data.json next to the output
// (main.go:64-69, renderer.go:473-485).  The render itself is rt_render()
// on the GPU.  Deviations: ".ppm" outputs are written
// as P3 PPM (Go writes PNG bytes whatever the extension), benchmark_data.json
// gains the published rays_per_second / pixels_per_second fields
// (README.md:60-61), and the optional flags above (the Go CLI never calls
// the renderer's setters, settings.go:3-25; --sky is the opt-in atmosphere,
// include/rt_api.h RT_SKY_*; --camera lookat honours the scene's lookAt, up
// and fov instead of getRay's fixed -Z view, RT_CAMERA_*).  --pass-samples N renders progressively on one
// device: N samples per pass up to the cap --samples, one
// "Pass k: n samples[, c pixels changed]" line per pass, stopping early once
// --time-budget SECONDS have passed or at most --converge PIXELS pixels of the
// preview changed in a pass; the output is written once, at the end, and
// benchmark_data.json records the samples actually rendered.  --adaptive
//  stops every pixel on its own and the run once none is
// active ("Pass k: n samples, a pixels active"); --count-map FILE writes the
// per-pixel sample counts as a grey PNG, count * 255 / cap.  --orbit N[,DEGREES]
//  renders N views of the scene on one device, the scene's
// camera turned about its up axis around its lookAt by DEGREES (360) in all
// (rt_camera_orbit; --camera lookat makes the views differ in direction too),
// as camera sequences of at most RT_MAX_FRAMES frames, and writes
// <stem>_0000<ext> .. ; benchmark_data.json records "frames": N.
// --aov PREFIX (one view, --samples >= 1) writes, after the
// render, the first-hit feature buffers of the frame (the render's size,
// samples, seed and camera model; device 0) as PREFIX.albedo, PREFIX.normal,
// PREFIX.depth, PREFIX.coverage and PREFIX.object with the output image's
// extension (PNG, or P3 PPM for ".ppm"), 8 bits per channel, round(v) =
// floor(v + 0.5):
//   albedo    round(clamp01(a) * 255) per channel
//   normal    round(clamp01(n * 0.5 + 0.5) * 255) per channel
//   depth     grey round(255 * (far - d) / (far - near)), near and far the least and the largest finite
//             depth of the frame (nearer is brighter); a miss 0; every finite depth equal: 255
//   coverage  grey round(c * 255)
//   object    the bytes 0..2 of (index + 1) * 2654435761 mod 2^32, each with its top bit set; a miss black
// A size without pixels (a width or height <= 0) writes none.  Without --aov
// nothing changes.
// --denoise SPEC (one view, --samples >= 1, a size with
// pixels) writes the DENOISED image instead of the raw one: the frame's linear
// radiance is uploaded to device 0, where its first-hit feature buffers (the
// render's size, seed and camera model; its samples, or those of the first
// pass with --pass-samples) steer the à-trous filter (rt_denoise_async) whose
// tone-mapped output is the image saved -- the plain render's, or the last
// image of a progression (whose "pixels changed" lines and stop rules still
// read the raw images).  SPEC is `default` (rt_denoise_default) or up to four
// comma-separated fields that replace the defaults from the left.  It combines
// with --aov and is refused with --orbit unless --temporal is given.
// --temporal SPEC (only with --orbit, --samples >= 1) writes
// the ACCUMULATED views to the files --orbit writes: view f is rendered with
// seed --seed + f, gets a first-hit feature pass of its own, and
// rt_temporal_async reprojects view f - 1's result into it and blends.  SPEC is
// `default` (rt_temporal_default) or up to three comma-separated fields that
// replace the defaults from the left.  With --denoise each view written is the
// à-trous filter of its accumulation; the unfiltered accumulation is what the
// next view reprojects.
// --denoise-variance SPEC (--samples >= 1, a size with pixels;
// not with --denoise or --pass-samples) writes the variance-guided filter's
// image.  With --orbit N --temporal ... each view's accumulation also carries
// the luminance moments (rt_temporal_moments_async), rt_variance_async turns
// them into the view's variance and rt_denoise_var_async filters the
// accumulation; the unfiltered accumulation and moments are what the next view
// reprojects.  Without --orbit the single render is filtered with the spatial
// variance estimate (a single frame has no moments).  SPEC is `default`
// (rt_denoise_var_default, rt_variance_default) or up to four comma-separated
// fields that replace the defaults from the left; SIGMA_DEPTH and NORMAL_POWER
// go to the variance pass too.
// --aov-specular SPEC (with --aov, --denoise or
// --denoise-variance) makes the run's feature pass the specular-through one
// (rt_context_render_aov_spec_async): ideal mirror reflections are followed
// from each first hit, at most BOUNCES (0..16) of them, through metal, shiny
// and perfectmirror surfaces whose roughness is at most MAX_ROUGHNESS.  SPEC
// is `default` (rt_aov_spec_default: 4, 0.1).  --aov then writes SEVEN images:
// the five above taken behind the mirrors, PREFIX.specular (grey
// round(s * 255)) and PREFIX.bounces (grey round(clamp01(b / BOUNCES) * 255),
// black for BOUNCES 0).  --denoise and --denoise-variance guide their filter by
// the specular-through albedo, normal, depth and object; with --orbit
// --temporal the accumulation keeps the first-hit buffers (reprojection needs
// the geometric depth) and only the spatial filter changes its guide.
// --move K:DX,DY,DZ (repeatable, one per object; only with
// --orbit) makes the sequence an animation: at view f object K (its index in
// the scene file) stands at its position + f * (DX, DY, DZ).  The views then
// render one by one, each after rt_context_set_scene of its own scene, and the
// feature passes use the same scene.  With --temporal the accumulation is
// rt_temporal_motion_async, whose table is rt_scene_motion of the scenes of
// views f - 1 and f, so that a moving object keeps its history; --denoise,
// --denoise-variance and --aov-specular combine with it as above.  A K outside
// the scene, a K given twice and malformed or non-finite fields are refused
// before anything renders.
// --clip SPEC (only with --orbit N --temporal ...) rectifies
// the history: the accumulation is rt_temporal_clip_async, which clips each
// pixel's reprojected history to mean +- GAMMA sigma of the current view's
// demodulated colour in a (2 RADIUS + 1)^2 window (the view's albedo
// demodulates it).  SPEC is `default` (rt_history_clip_default) or up to four
// comma-separated fields that replace the defaults from the left.  It combines
// with --move, --denoise, --denoise-variance and --aov-specular as above.
// --matte PREFIX[,SAMPLES[,RANKS[,object|face]]] (one view, a
// size with pixels) writes, after the render, the matte layers of the frame
// (rt_context_render_matte_async with SAMPLES (16) camera rays per pixel, RANKS
// (4) ranks, the render's seed and camera model; device 0) as PREFIX.id<r> and
// PREFIX.coverage<r> for each rank r and PREFIX.rest, with the output image's
// extension: id in --aov's object colours of the key (an empty rank black),
// coverage grey round(count / SAMPLES * 255), rest grey round(rest / SAMPLES *
// 255).
// --edge-resolve SPEC (one view, --samples >= 1, a size with
// pixels) antialiases the silhouettes of the image written: the frame's linear
// image -- the filter's with --denoise or --denoise-variance -- goes through
// rt_matte_resolve_async with an object-level matte of SAMPLES camera rays per
// pixel (4 ranks) and the frame's first-hit object ids (the render's samples,
// or those of the first pass with --pass-samples).  SPEC is `default` (16
// samples, radius 2) or SAMPLES[,RADIUS].
#include <errno.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/stat.h>
#include <sys/time.h>
#include <time.h>
#include <unistd.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../include/rt_api.h"

static bool parse_int(const char* s, long long* out) {
  // strconv.Atoi: optional sign, decimal digits only
  if (!s || !*s) return false;
  const char* p = s;
  if (*p == '+' || *p == '-') ++p;
  if (!*p) return false;
  for (const char* q = p; *q; ++q)
    if (*q < '0' || *q > '9') return false;
  char* end = nullptr;
  *out = strtoll(s, &end, 10);
  return end && *end == 0;
}

static std::string dir_of(const std::string& path) {  // filepath.Dir
  size_t s = path.find_last_of('/');
  if (s == std::string::npos) return ".";
  if (s == 0) return "/";
  return path.substr(0, s);
}

static void mkdir_p(const std::string& dir) {  // os.MkdirAll(dir, 0755)
  for (size_t i = 1; i <= dir.size(); ++i)
    if (i == dir.size() || dir[i] == '/') (void)mkdir(dir.substr(0, i).c_str(), 0755);
}

static std::string ext_of(const std::string& path) {  // filepath.Ext
  for (size_t i = path.size(); i-- > 0;) {
    if (path[i] == '/') break;
    if (path[i] == '.') return path.substr(i);
  }
  return "";
}

static std::string rfc3339nano_now() {
  struct timespec ts;
  clock_gettime(CLOCK_REALTIME, &ts);
  struct tm tmv;
  localtime_r(&ts.tv_sec, &tmv);
  char date[64];
  strftime(date, sizeof date, "%Y-%m-%dT%H:%M:%S", &tmv);
  char frac[16] = "";
  if (ts.tv_nsec) {
    snprintf(frac, sizeof frac, ".%09ld", ts.tv_nsec);
    size_t n = strlen(frac);
    while (n > 1 && frac[n - 1] == '0') frac[--n] = 0;
  }
  long off = tmv.tm_gmtoff;
  char tz[24];
  if (off == 0)
    snprintf(tz, sizeof tz, "Z");
  else
    snprintf(tz, sizeof tz, "%c%02ld:%02ld", off < 0 ? '-' : '+', labs(off) / 3600, (labs(off) % 3600) / 60);
  return std::string(date) + frac + tz;
}

static const char* kFeatures[] = {
    "Improved metallic reflections with Fresnel effect",
    "Shiny materials with configurable roughness and specular",
    "Enhanced light source reflections",
    "Better specular highlights for metallic surfaces",
};

// Render's closing lines (renderer.go:119-123)
static void print_complete() {
  printf("Rendering complete!\n");
  printf("Enhanced materials features:\n");
  for (const char* f : kFeatures) printf("- %s\n", f);
}

// SaveBenchmarkData (renderer.go:473-485): BenchmarkData JSON, 2-space indent,
// next to the output (main.go:64-69)
static void save_benchmark(const std::string& out_path, long long w, long long h, const rt_settings& st,
                           const rt_stats& stats, double mean_samples = -1, long long frames = -1) {
  std::string bench_path = dir_of(out_path) + "/benchmark_data.json";
  FILE* f = fopen(bench_path.c_str(), "wb");
  if (!f) {
    printf("Error saving benchmark data: open %s failed\n", bench_path.c_str());
  } else {
    fprintf(f, "{\n");
    fprintf(f, "  \"scene_name\": \"demo_scene\",\n");  // GetSceneName, scene.go:100-102
    fprintf(f, "  \"resolution\": \"%lldx%lld\",\n", w, h);
    fprintf(f, "  \"render_time_seconds\": %.17g,\n", stats.render_seconds);
    fprintf(f, "  \"samples\": %d,\n", st.samples);
    // (--adaptive: the mean samples per pixel actually rendered)
    if (mean_samples >= 0) fprintf(f, "  \"mean_samples_per_pixel\": %.17g,\n", mean_samples);
    if (frames >= 0) fprintf(f, "  \"frames\": %lld,\n", frames);  // (--orbit)
    fprintf(f, "  \"max_depth\": %d,\n", st.max_depth);
    fprintf(f, "  \"num_workers\": %d,\n", st.num_workers);
    fprintf(f, "  \"objects\": %d,\n", stats.objects);
    fprintf(f, "  \"lights\": %d,\n", stats.lights);
    fprintf(f, "  \"timestamp\": \"%s\",\n", rfc3339nano_now().c_str());
    fprintf(f, "  \"features\": [\n");
    for (int i = 0; i < 4; ++i) fprintf(f, "    \"%s\"%s\n", kFeatures[i], i < 3 ? "," : "");
    fprintf(f, "  ],\n");
    fprintf(f, "  \"kernel_time_seconds\": %.17g,\n", stats.kernel_seconds);
    // the published benchmark JSON's setup_time / bvh_build_time
    // (demo-assets/*_benchmark.json; not produced by the snapshot's Go code)
    fprintf(f, "  \"setup_time\": %.17g,\n", stats.create_seconds + stats.scene_seconds);
    fprintf(f, "  \"bvh_build_time\": %.17g,\n", stats.bvh_build_seconds);
    fprintf(f, "  \"render_breakdown_seconds\": {\"create\": %.9g, \"scene\": %.9g, \"launch\": %.9g, "
               "\"kernels_and_download\": %.9g, \"destroy\": %.9g},\n",
            stats.create_seconds, stats.scene_seconds, stats.launch_seconds, stats.download_seconds,
            stats.destroy_seconds);
    fprintf(f, "  \"pixels_per_second\": %.17g,\n", stats.pixels_per_second);
    fprintf(f, "  \"rays_per_second\": %.17g\n", stats.rays_per_second);
    fprintf(f, "}");
    fclose(f);
    printf("Benchmark data saved\n");
  }
}

// --pass-samples: the frame through rt_context_progressive_* on device 0,
// pass_samples at a time up to the cap st.samples; fills rgba (host, w*h*4),
// stats and *rendered (samples per pixel actually rendered).  budget_s < 0 /
// converge < 0: that rule is off.  adapt (--adaptive; null:
// off): every pixel stops on its own, the progression also ends when none is
// active; *mean_samples is the mean samples per pixel, and count_map (when
// not empty) receives the counts as a grey PNG, count * 255 / cap.  linear
// (host, w*h*3 floats; null: not wanted) receives the last image's linear
// radiance (--denoise).
static int render_progressive(const rt_scene* scene, int32_t w, int32_t h, const rt_settings& st, int pass_samples,
                              double budget_s, long long converge, const rt_adaptive* adapt,
                              const std::string& count_map, uint8_t* rgba, rt_stats* stats, int* rendered,
                              double* mean_samples, float* linear) {
  const auto t_new = std::chrono::steady_clock::now();
  rt_context* ctx = nullptr;
  if (rt_context_create(0, &ctx) != RT_OK) return RT_E_DEVICE;
  stats->create_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_new).count();
  const auto t0 = std::chrono::steady_clock::now();
  const size_t npix = (size_t)w * (size_t)h;
  uint8_t* d_img[2] = {nullptr, nullptr};
  uint32_t* d_delta = nullptr;
  float* d_lin = nullptr;
  int rc = rt_context_set_scene(ctx, scene, 0);
  stats->scene_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  auto hip_ok = [&](hipError_t e, const char* what) {
    if (e == hipSuccess) return true;
    fprintf(stderr, "%s failed: %s\n", what, hipGetErrorString(e));
    rc = RT_E_DEVICE;
    return false;
  };
  if (rc == RT_OK) rc = rt_context_progressive_begin(ctx, w, h, &st, 0, 1, RT_LAYOUT_IMAGE);
  if (rc == RT_OK && adapt) rc = rt_context_progressive_set_adaptive(ctx, adapt);
  int64_t state[4] = {0, 0, 0, 0};
  if (rc == RT_OK && hip_ok(hipMalloc((void**)&d_img[0], npix * 4), "hipMalloc") &&
      hip_ok(hipMalloc((void**)&d_img[1], npix * 4), "hipMalloc"))
    hip_ok(hipMalloc((void**)&d_delta, 2 * sizeof(uint32_t)), "hipMalloc");
  if (rc == RT_OK && linear) hip_ok(hipMalloc((void**)&d_lin, npix * 3 * sizeof(float)), "hipMalloc");
  int done = 0, k = 0;
  double kernel_s = 0;
  while (rc == RT_OK) {
    const int n = std::min(pass_samples, st.samples - done);
    uint8_t* cur = d_img[k & 1];
    rc = rt_context_progressive_add_async(ctx, n, d_lin, cur, nullptr);
    if (rc != RT_OK) break;
    uint32_t delta[2] = {0, 0};
    if (k > 0) {  // how much the preview still moved in this pass
      rc = rt_rgba_delta_async(d_img[(k & 1) ^ 1], cur, npix, d_delta, nullptr);
      if (rc != RT_OK) break;
      if (!hip_ok(hipMemcpy(delta, d_delta, sizeof delta, hipMemcpyDeviceToHost), "hipMemcpy")) break;
    } else if (!hip_ok(hipStreamSynchronize(nullptr), "hipStreamSynchronize")) {
      break;
    }
    double ks = 0;
    if (rt_context_last_kernel_seconds(ctx, &ks) == RT_OK) kernel_s += ks;
    done += n;
    k += 1;
    if (adapt) {
      rc = rt_context_progressive_state(ctx, state);
      if (rc != RT_OK) break;
      printf("Pass %d: %d samples, %lld pixels active\n", k, done, (long long)state[1]);
    } else if (k > 1)
      printf("Pass %d: %d samples, %u pixels changed\n", k, done, delta[0]);
    else
      printf("Pass %d: %d samples\n", k, done);
    fflush(stdout);
    const double el = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (adapt && state[1] == 0) break;
    if (done >= st.samples || (budget_s >= 0 && el >= budget_s) || (converge >= 0 && k > 1 && (long long)delta[0] <= converge))
      break;
  }
  if (rc == RT_OK && k > 0)
    hip_ok(hipMemcpy(rgba, d_img[(k - 1) & 1], npix * 4, hipMemcpyDeviceToHost), "hipMemcpy");
  if (rc == RT_OK && k > 0 && linear)
    hip_ok(hipMemcpy(linear, d_lin, npix * 3 * sizeof(float), hipMemcpyDeviceToHost), "hipMemcpy");
  if (rc == RT_OK) rc = rt_context_progressive_state(ctx, state);
  if (rc == RT_OK) *mean_samples = state[0] > 0 ? (double)state[2] / (double)state[0] : 0.0;
  if (rc == RT_OK && !count_map.empty()) {
    uint32_t* d_counts = nullptr;
    std::vector<uint32_t> counts(npix);
    std::vector<uint8_t> grey(npix * 4);
    if (hip_ok(hipMalloc((void**)&d_counts, npix * sizeof(uint32_t)), "hipMalloc")) {
      rc = rt_context_progressive_counts_async(ctx, d_counts, nullptr);
      if (rc == RT_OK) hip_ok(hipMemcpy(counts.data(), d_counts, npix * sizeof(uint32_t), hipMemcpyDeviceToHost), "hipMemcpy");
      (void)hipFree(d_counts);
    }
    if (rc == RT_OK) {
      for (size_t i = 0; i < npix; ++i) {
        const uint8_t g = (uint8_t)std::min<uint64_t>(255, (uint64_t)counts[i] * 255 / (uint64_t)std::max(st.samples, 1));
        grey[4 * i + 0] = grey[4 * i + 1] = grey[4 * i + 2] = g;
        grey[4 * i + 3] = 255;
      }
      rc = rt_write_png(count_map.c_str(), grey.data(), w, h);
    }
  }
  const std::string err = rc != RT_OK ? rt_last_error() : "";  // (before the clean-up's calls)
  const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  (void)rt_context_progressive_end(ctx);
  for (void* p : {(void*)d_img[0], (void*)d_img[1], (void*)d_delta, (void*)d_lin})
    if (p) (void)hipFree(p);
  rt_context_destroy(ctx);
  if (rc != RT_OK) {
    if (!err.empty()) fprintf(stderr, "%s\n", err.c_str());
    return rc;
  }
  *rendered = done;
  stats->render_seconds = secs;
  stats->kernel_seconds = kernel_s;
  stats->objects = scene->num_objects;
  stats->lights = scene->num_lights;
  stats->rays_per_second = (double)npix * done / secs;
  stats->pixels_per_second = (double)npix / secs;
  return RT_OK;
}

// --orbit: n views of rt_camera_orbit of the scene's camera through
// rt_context_render_cameras_async on device 0, RT_MAX_FRAMES at a time; each
// launch's images go to save(first frame, frames, their RGBA8 images, w*h*4
// bytes each), which returns false to stop (RT_E_IO); fills stats.
// tp (--temporal): view f takes seed st.seed + f; after each
// launch its views, in order, get their feature buffers and are accumulated
// over the view before (rt_temporal_async; features, colour and count
// ping-pong), and the accumulated images are the ones saved -- filtered by
// rt_denoise_async first when dn is given.  vs (--denoise-variance, §4.15): the
// accumulation is rt_temporal_moments_async's, the moments ping-pong with it,
// and the image saved is rt_denoise_var_async's, steered by rt_variance_async.
// move (--move, §4.17; num_objects * 3 doubles, or null): view f renders the scene with object k at
// position + f * move[k], one rt_context_set_scene and one one-camera launch per view; the feature passes use
// the same scene, and the accumulation is rt_temporal_motion_async with rt_scene_motion(view f - 1's scene,
// view f's) as its table, so that a moving object keeps its history.
struct VarianceSpec {
  rt_denoise_var dv;
  rt_variance vr;
};
// --aov-specular: the run's feature pass is the specular-through one.  The guide a
// filter reads -- albedo, normal, depth, object -- comes from guide_pass: rt_context_render_aov_spec_async
// with these parameters when the flag is given, else the first-hit pass.
static bool g_spec_on = false;
static rt_aov_spec g_spec;
static int guide_pass(rt_context* ctx, int32_t w, int32_t h, const rt_settings* st, const rt_camera* cam, float* albedo,
                      float* normal, float* depth, int32_t* object) {
  if (g_spec_on) {
    const rt_aov_spec_buffers out = {albedo, normal, depth, nullptr, object, nullptr, nullptr};
    return rt_context_render_aov_spec_async(ctx, w, h, st, cam, &g_spec, &out, nullptr);
  }
  const rt_aov_buffers out = {albedo, normal, depth, nullptr, object};
  return rt_context_render_aov_async(ctx, w, h, st, cam, &out, nullptr);
}

template <class Save>
static int render_orbit(const rt_scene* scene, int32_t w, int32_t h, const rt_settings& st, int n, double degrees,
                        Save save, rt_stats* stats, const rt_temporal* tp = nullptr, const rt_denoise* dn = nullptr,
                        const VarianceSpec* vs = nullptr, const double* move = nullptr,
                        const rt_history_clip* hc = nullptr) {
  std::vector<rt_camera> cams((size_t)n);
  int rc = rt_camera_orbit(&scene->camera, n, degrees, cams.data());
  if (rc != RT_OK) return rc;
  const auto t_new = std::chrono::steady_clock::now();
  rt_context* ctx = nullptr;
  if (rt_context_create(0, &ctx) != RT_OK) return RT_E_DEVICE;
  stats->create_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_new).count();
  const auto t0 = std::chrono::steady_clock::now();
  const size_t npix = (size_t)w * (size_t)h;
  rc = rt_context_set_scene(ctx, scene, 0);
  stats->scene_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  auto hip_ok = [&](hipError_t e, const char* what) {
    if (e == hipSuccess) return true;
    fprintf(stderr, "%s failed: %s\n", what, hipGetErrorString(e));
    rc = RT_E_DEVICE;
    return false;
  };
  const int per = move ? 1 : std::min(n, RT_MAX_FRAMES);
  std::vector<uint8_t> rgba((size_t)per * npix * 4);
  // --move: view f's objects, and with --temporal every view's motion table on the device (view 0: zeros)
  const size_t nobj = (size_t)std::max(scene->num_objects, 0);
  std::vector<rt_object> moved[2];
  rt_scene moved_scene[2] = {*scene, *scene};
  auto move_to = [&](int f) {
    std::vector<rt_object>& o = moved[f & 1];
    o.assign(scene->objects, scene->objects + nobj);
    for (size_t k = 0; k < nobj; ++k)
      for (int j = 0; j < 3; ++j) o[k].position[j] = o[k].position[j] + (double)f * move[k * 3 + j];
    moved_scene[f & 1].objects = o.data();
  };
  double* d_motion = nullptr;
  if (rc == RT_OK && move && tp) {
    std::vector<double> tables((size_t)n * nobj * 3, 0.0);
    move_to(0);
    for (int f = 1; rc == RT_OK && f < n; ++f) {
      move_to(f);
      if (rt_scene_motion(&moved_scene[(f - 1) & 1], &moved_scene[f & 1], tables.data() + (size_t)f * nobj * 3, nobj * 3) < 0)
        rc = RT_E_INVALID;
    }
    if (rc == RT_OK && hip_ok(hipMalloc((void**)&d_motion, tables.size() * sizeof(double)), "hipMalloc"))
      hip_ok(hipMemcpy(d_motion, tables.data(), tables.size() * sizeof(double), hipMemcpyHostToDevice), "hipMemcpy");
  }
  float* d_lin = nullptr;
  uint8_t* d_img = nullptr;
  if (rc == RT_OK && hip_ok(hipMalloc((void**)&d_lin, (size_t)per * npix * 12), "hipMalloc"))
    hip_ok(hipMalloc((void**)&d_img, (size_t)per * npix * 4), "hipMalloc");
  // --temporal: two sets of albedo | normal | depth | object | accumulated colour | count (| moments | variance
  // with --denoise-variance), and the filter's workspace
  const size_t set_floats = npix * (vs ? 15 : 12);
  float* d_tp = nullptr;
  void* d_work = nullptr;
  const size_t work_bytes = dn ? rt_denoise_workspace_bytes(w, h) : vs ? rt_denoise_var_workspace_bytes(w, h) : 0;
  if (rc == RT_OK && tp && hip_ok(hipMalloc((void**)&d_tp, 2 * set_floats * sizeof(float)), "hipMalloc") && (dn || vs))
    hip_ok(hipMalloc(&d_work, work_bytes), "hipMalloc");
  // --aov-specular: the spatial filter's guide (albedo | normal | depth | object) beside the first-hit set,
  // which the accumulation keeps (reprojection needs the geometric depth)
  float* d_sg = nullptr;
  if (rc == RT_OK && tp && (dn || vs) && g_spec_on) hip_ok(hipMalloc((void**)&d_sg, npix * 8 * sizeof(float)), "hipMalloc");
  const float* prev_moments = nullptr;
  std::vector<uint64_t> seeds((size_t)n);
  for (int f = 0; f < n; ++f) seeds[(size_t)f] = st.seed + (uint64_t)f;
  rt_temporal_frame prev_frame = {};
  double kernel_s = 0, save_s = 0;
  for (int f0 = 0; rc == RT_OK && f0 < n; f0 += per) {
    const int m = std::min(per, n - f0);
    float* lin[RT_MAX_FRAMES];
    uint8_t* img[RT_MAX_FRAMES];
    for (int f = 0; f < m; ++f) {
      lin[f] = d_lin + (size_t)f * npix * 3;
      img[f] = d_img + (size_t)f * npix * 4;
    }
    if (move) {  // (per is 1: this view's scene, for its render and its feature passes)
      move_to(f0);
      rc = rt_context_set_scene(ctx, &moved_scene[f0 & 1], 0);
      if (rc != RT_OK) break;
    }
    rc = rt_context_render_cameras_async(ctx, w, h, &st, m, cams.data() + f0, tp ? seeds.data() + f0 : nullptr, 0, 1,
                                         RT_LAYOUT_IMAGE, lin, img, nullptr);
    if (rc != RT_OK) break;
    double ks = 0;  // (the render's own device time: read before the feature passes record theirs)
    if (tp && rt_context_last_kernel_seconds(ctx, &ks) == RT_OK) kernel_s += ks;
    for (int f = 0; tp && rc == RT_OK && f < m; ++f) {
      float* set = d_tp + (size_t)((f0 + f) & 1) * set_floats;
      float *albedo = set, *normal = set + npix * 3, *depth = set + npix * 6, *acc = set + npix * 8,
            *cnt = set + npix * 11;
      int32_t* object = (int32_t*)(set + npix * 7);
      rt_settings fst = st;
      fst.seed = seeds[(size_t)(f0 + f)];
      const rt_aov_buffers out = {albedo, normal, depth, nullptr, object};
      rc = rt_context_render_aov_async(ctx, w, h, &fst, &cams[(size_t)(f0 + f)], &out, nullptr);
      rt_temporal_frame cur = {lin[f], depth, object, normal, nullptr, {0}};
      if (rc == RT_OK) rc = rt_camera_frame(&cams[(size_t)(f0 + f)], st.camera, w, h, cur.frame);
      float *mom = set + npix * 12, *var = set + npix * 14;  // (only with vs)
      const float *g_albedo = albedo, *g_normal = normal, *g_depth = depth;  // the spatial filter's guide
      const int32_t* g_object = object;
      if (rc == RT_OK && d_sg) {
        rc = guide_pass(ctx, w, h, &fst, &cams[(size_t)(f0 + f)], d_sg, d_sg + npix * 3, d_sg + npix * 6,
                        (int32_t*)(d_sg + npix * 7));
        g_albedo = d_sg, g_normal = d_sg + npix * 3, g_depth = d_sg + npix * 6;
        g_object = (const int32_t*)(d_sg + npix * 7);
      }
      const rt_motion table = {d_motion ? d_motion + (size_t)(f0 + f) * nobj * 3 : nullptr, (int32_t)nobj, 0};
      if (rc == RT_OK && hc)  // --clip: the same outputs as the calls below, the history rectified (§4.18)
        rc = rt_temporal_clip_async(tp, w, h, &cur, f0 + f > 0 ? &prev_frame : nullptr, move ? &table : nullptr, hc, albedo,
                                    vs ? prev_moments : nullptr, acc, cnt, vs ? mom : nullptr, nullptr,
                                    vs ? nullptr : img[f], nullptr);
      if (rc == RT_OK && !vs && !hc)
        rc = move ? rt_temporal_motion_async(tp, w, h, &cur, f0 + f > 0 ? &prev_frame : nullptr, &table, nullptr, nullptr,
                                             acc, cnt, nullptr, img[f], nullptr)
                  : rt_temporal_async(tp, w, h, &cur, f0 + f > 0 ? &prev_frame : nullptr, acc, cnt, img[f], nullptr);
      if (rc == RT_OK && vs) {
        if (!hc)
          rc = move ? rt_temporal_motion_async(tp, w, h, &cur, f0 + f > 0 ? &prev_frame : nullptr, &table, albedo,
                                               prev_moments, acc, cnt, mom, nullptr, nullptr)
                    : rt_temporal_moments_async(tp, w, h, &cur, f0 + f > 0 ? &prev_frame : nullptr, albedo,
                                                prev_moments, acc, cnt, mom, nullptr, nullptr);
        prev_moments = mom;
        const rt_variance_inputs vin = {acc, g_normal, g_depth, g_albedo, g_object, mom, cnt};
        if (rc == RT_OK) rc = rt_variance_async(&vs->vr, w, h, &vin, var, nullptr);
        const rt_denoise_inputs in = {acc, g_normal, g_depth, g_albedo, g_object};
        if (rc == RT_OK)
          rc = rt_denoise_var_async(&vs->dv, w, h, &in, var, nullptr, img[f], nullptr, d_work, work_bytes, nullptr);
      }
      prev_frame = cur;
      prev_frame.color = acc;
      prev_frame.count = cnt;
      if (rc == RT_OK && dn) {
        const rt_denoise_inputs in = {acc, g_normal, g_depth, g_albedo, g_object};
        rc = rt_denoise_async(dn, w, h, &in, nullptr, img[f], d_work, work_bytes, nullptr);
      }
    }
    if (rc != RT_OK) break;
    if (!hip_ok(hipMemcpy(rgba.data(), d_img, (size_t)m * npix * 4, hipMemcpyDeviceToHost), "hipMemcpy")) break;
    if (!tp && rt_context_last_kernel_seconds(ctx, &ks) == RT_OK) kernel_s += ks;
    const auto t_save = std::chrono::steady_clock::now();  // (writing the files is not render time)
    if (!save(f0, m, rgba.data())) rc = RT_E_IO;
    save_s += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_save).count();
  }
  const std::string err = rc != RT_OK ? rt_last_error() : "";  // (before the clean-up's calls)
  const double secs = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count() - save_s;
  for (void* p : {(void*)d_lin, (void*)d_img, (void*)d_tp, (void*)d_sg, (void*)d_motion, d_work})
    if (p) (void)hipFree(p);
  rt_context_destroy(ctx);
  if (rc != RT_OK) {
    if (!err.empty()) fprintf(stderr, "%s\n", err.c_str());
    return rc;
  }
  stats->render_seconds = secs;
  stats->kernel_seconds = kernel_s;
  stats->objects = scene->num_objects;
  stats->lights = scene->num_lights;
  stats->rays_per_second = (double)npix * st.samples * n / secs;
  stats->pixels_per_second = (double)npix * n / secs;
  return RT_OK;
}

// --aov PREFIX: the first-hit feature buffers of the frame (DESIGN.md §4.12,
// rt_context_render_aov_async) on device 0, with the render's size, samples,
// seed and camera model, written as five images PREFIX.<name><ext> with the
// mappings of the usage text above.
static uint8_t aov_byte(double v) {  // round(clamp01(v) * 255), halves up; NaN: 0
  if (!(v > 0)) return 0;
  if (v > 1) v = 1;
  return (uint8_t)floor(v * 255.0 + 0.5);
}
static int write_aov(const rt_scene* scene, int32_t w, int32_t h, const rt_settings& st, const std::string& prefix,
                     const std::string& ext) {
  const size_t npix = (size_t)w * (size_t)h;
  rt_context* ctx = nullptr;
  int rc = rt_context_create(0, &ctx);
  if (rc != RT_OK) return rc;
  rc = rt_context_set_scene(ctx, scene, 0);
  // one device block: albedo | normal | depth | coverage | object | specular | bounces (the last two with
  // --aov-specular only)
  float* d = nullptr;
  std::vector<float> host(npix * 11);
  if (rc == RT_OK && hipMalloc((void**)&d, npix * 11 * sizeof(float)) != hipSuccess) {
    fprintf(stderr, "hipMalloc failed\n");
    rc = RT_E_DEVICE;
  }
  if (rc == RT_OK && g_spec_on) {
    const rt_aov_spec_buffers out = {d, d + npix * 3, d + npix * 6, d + npix * 7, (int32_t*)(d + npix * 8),
                                     d + npix * 9, d + npix * 10};
    rc = rt_context_render_aov_spec_async(ctx, w, h, &st, nullptr, &g_spec, &out, nullptr);
  } else if (rc == RT_OK) {
    const rt_aov_buffers out = {d, d + npix * 3, d + npix * 6, d + npix * 7, (int32_t*)(d + npix * 8)};
    rc = rt_context_render_aov_async(ctx, w, h, &st, nullptr, &out, nullptr);
  }
  if (rc == RT_OK && hipMemcpy(host.data(), d, npix * (g_spec_on ? 11 : 9) * sizeof(float), hipMemcpyDeviceToHost) !=
                         hipSuccess) {
    fprintf(stderr, "hipMemcpy failed\n");
    rc = RT_E_DEVICE;
  }
  const std::string err = rc != RT_OK ? rt_last_error() : "";  // (before the clean-up's calls)
  if (d) (void)hipFree(d);
  rt_context_destroy(ctx);
  if (rc != RT_OK) {
    if (!err.empty()) fprintf(stderr, "%s\n", err.c_str());
    return rc;
  }
  const float *albedo = host.data(), *normal = albedo + npix * 3, *depth = albedo + npix * 6,
              *coverage = albedo + npix * 7;
  const int32_t* object = reinterpret_cast<const int32_t*>(albedo + npix * 8);
  double near = INFINITY, far = -INFINITY;  // over the frame's finite depths
  for (size_t i = 0; i < npix; ++i)
    if (std::isfinite(depth[i])) {
      near = std::min(near, (double)depth[i]);
      far = std::max(far, (double)depth[i]);
    }
  std::vector<uint8_t> img(npix * 4);
  const float *specular = albedo + npix * 9, *bounces = albedo + npix * 10;
  const char* names[7] = {"albedo", "normal", "depth", "coverage", "object", "specular", "bounces"};
  for (int k = 0; k < (g_spec_on ? 7 : 5); ++k) {
    for (size_t i = 0; i < npix; ++i) {
      uint8_t* px = &img[4 * i];
      px[3] = 255;
      if (k == 0) {
        for (int c = 0; c < 3; ++c) px[c] = aov_byte(albedo[3 * i + c]);
      } else if (k == 1) {
        for (int c = 0; c < 3; ++c) px[c] = aov_byte((double)normal[3 * i + c] * 0.5 + 0.5);
      } else if (k == 2) {
        uint8_t g = 0;  // a miss
        if (std::isfinite(depth[i])) g = far > near ? aov_byte((far - (double)depth[i]) / (far - near)) : 255;
        px[0] = px[1] = px[2] = g;
      } else if (k == 3) {
        px[0] = px[1] = px[2] = aov_byte(coverage[i]);
      } else if (k == 5) {
        px[0] = px[1] = px[2] = aov_byte(specular[i]);
      } else if (k == 6) {  // grey bounces / max_bounces (max_bounces 0: bounces is 0 everywhere)
        px[0] = px[1] = px[2] = g_spec.max_bounces > 0 ? aov_byte((double)bounces[i] / g_spec.max_bounces) : 0;
      } else {
        // a fixed colour per hittable index: the bytes of (index + 1) * 2654435761 mod 2^32,
        // each with its top bit set (never black); a miss is black
        const uint32_t hsh = ((uint32_t)object[i] + 1u) * 2654435761u;
        for (int c = 0; c < 3; ++c) px[c] = object[i] < 0 ? 0 : (uint8_t)(((hsh >> (8 * c)) & 0xFFu) | 0x80u);
      }
    }
    const std::string fp = prefix + "." + names[k] + ext;
    printf("Saving to: %s\n", fp.c_str());
    fflush(stdout);
    rc = ext == ".ppm" ? rt_write_ppm(fp.c_str(), img.data(), w, h) : rt_write_png(fp.c_str(), img.data(), w, h);
    if (rc != RT_OK) {
      printf("Error saving image: %s\n", rt_last_error());
      return rc;
    }
  }
  return RT_OK;
}

// --edge-resolve: the matte's samples and the resolve's parameters.
struct EdgeResolve {
  int32_t samples;
  rt_matte_resolve rs;
};
// The resolve of the device image d_color into d_rgba on ctx's device: an object-level matte of the frame
// (er.samples rays per pixel, 4 ranks, st's seed and camera model), the frame's first-hit ids (d_object, or when
// that is null a first-hit pass with feature_samples samples) and rt_matte_resolve_async.
static int edge_resolve_device(rt_context* ctx, int32_t w, int32_t h, const rt_settings& st, int feature_samples,
                               const EdgeResolve& er, const float* d_color, const int32_t* d_object, uint8_t* d_rgba) {
  const size_t npix = (size_t)w * (size_t)h;
  rt_matte mp;
  rt_matte_default(&mp);
  int32_t* d = nullptr;  // id | count | rest | object
  if (hipMalloc((void**)&d, npix * (size_t)(2 * mp.ranks + 2) * sizeof(int32_t)) != hipSuccess) {
    fprintf(stderr, "hipMalloc failed\n");
    return RT_E_DEVICE;
  }
  int32_t *d_id = d, *d_count = d + npix * (size_t)mp.ranks, *d_rest = d + npix * (size_t)(2 * mp.ranks);
  int rc = RT_OK;
  if (!d_object) {
    rt_settings fst = st;
    fst.samples = feature_samples;
    const rt_aov_buffers out = {nullptr, nullptr, nullptr, nullptr, d_rest + npix};
    rc = rt_context_render_aov_async(ctx, w, h, &fst, nullptr, &out, nullptr);
    d_object = d_rest + npix;
  }
  if (rc == RT_OK) {
    rt_settings mst = st;
    mst.samples = er.samples;
    const rt_matte_buffers out = {d_id, d_count, d_rest};
    rc = rt_context_render_matte_async(ctx, w, h, &mst, nullptr, &mp, &out, nullptr);
  }
  if (rc == RT_OK) {
    const rt_matte_resolve_inputs in = {d_color, d_object, d_id, d_count, d_rest, mp.ranks, er.samples};
    rc = rt_matte_resolve_async(&er.rs, w, h, &in, nullptr, d_rgba, nullptr);
  }
  if (rc == RT_OK && hipStreamSynchronize(nullptr) != hipSuccess) rc = RT_E_DEVICE;
  const std::string err = rc != RT_OK ? rt_last_error() : "";
  (void)hipFree(d);
  if (rc != RT_OK && !err.empty()) fprintf(stderr, "%s\n", err.c_str());
  return rc;
}

// --edge-resolve without a filter: the frame's linear radiance `linear` (host, w*h*3) resolved on device 0 into
// rgba (host, w*h*4).
static int resolve_image(const rt_scene* scene, int32_t w, int32_t h, const rt_settings& st, int feature_samples,
                         const EdgeResolve& er, const float* linear, uint8_t* rgba) {
  const size_t npix = (size_t)w * (size_t)h;
  rt_context* ctx = nullptr;
  int rc = rt_context_create(0, &ctx);
  if (rc != RT_OK) return rc;
  rc = rt_context_set_scene(ctx, scene, 0);
  float* d = nullptr;
  uint8_t* d_rgba = nullptr;
  if (rc == RT_OK && (hipMalloc((void**)&d, npix * 3 * sizeof(float)) != hipSuccess ||
                      hipMalloc((void**)&d_rgba, npix * 4) != hipSuccess ||
                      hipMemcpy(d, linear, npix * 3 * sizeof(float), hipMemcpyHostToDevice) != hipSuccess)) {
    fprintf(stderr, "hipMalloc or hipMemcpy failed\n");
    rc = RT_E_DEVICE;
  }
  if (rc == RT_OK) rc = edge_resolve_device(ctx, w, h, st, feature_samples, er, d, nullptr, d_rgba);
  if (rc == RT_OK && hipMemcpy(rgba, d_rgba, npix * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = RT_E_DEVICE;
  for (void* p : {(void*)d, (void*)d_rgba})
    if (p) (void)hipFree(p);
  rt_context_destroy(ctx);
  return rc;
}

// --matte: the matte layers of the frame on device 0 (rt_context_render_matte_async), written as
// PREFIX.id<r>, PREFIX.coverage<r> and PREFIX.rest with the mappings of the usage text above.
static int write_matte(const rt_scene* scene, int32_t w, int32_t h, const rt_settings& st, const rt_matte& mp,
                       int32_t samples, const std::string& prefix, const std::string& ext) {
  const size_t npix = (size_t)w * (size_t)h, planes = (size_t)(2 * mp.ranks + 1);
  rt_context* ctx = nullptr;
  int rc = rt_context_create(0, &ctx);
  if (rc != RT_OK) return rc;
  rc = rt_context_set_scene(ctx, scene, 0);
  int32_t* d = nullptr;
  std::vector<int32_t> host(npix * planes);
  if (rc == RT_OK && hipMalloc((void**)&d, npix * planes * sizeof(int32_t)) != hipSuccess) {
    fprintf(stderr, "hipMalloc failed\n");
    rc = RT_E_DEVICE;
  }
  if (rc == RT_OK) {
    rt_settings mst = st;
    mst.samples = samples;
    const rt_matte_buffers out = {d, d + npix * (size_t)mp.ranks, d + npix * (size_t)(2 * mp.ranks)};
    rc = rt_context_render_matte_async(ctx, w, h, &mst, nullptr, &mp, &out, nullptr);
  }
  if (rc == RT_OK && hipMemcpy(host.data(), d, npix * planes * sizeof(int32_t), hipMemcpyDeviceToHost) != hipSuccess) {
    fprintf(stderr, "hipMemcpy failed\n");
    rc = RT_E_DEVICE;
  }
  const std::string err = rc != RT_OK ? rt_last_error() : "";  // (before the clean-up's calls)
  if (d) (void)hipFree(d);
  rt_context_destroy(ctx);
  if (rc != RT_OK) {
    if (!err.empty()) fprintf(stderr, "%s\n", err.c_str());
    return rc;
  }
  std::vector<uint8_t> img(npix * 4);
  for (size_t k = 0; k < planes; ++k) {
    const int32_t* v = host.data() + k * npix;
    const bool is_id = k < (size_t)mp.ranks;
    for (size_t i = 0; i < npix; ++i) {
      uint8_t* px = &img[4 * i];
      px[3] = 255;
      if (is_id) {
        const uint32_t hsh = ((uint32_t)v[i] + 1u) * 2654435761u;
        for (int c = 0; c < 3; ++c) px[c] = v[i] < 0 ? 0 : (uint8_t)(((hsh >> (8 * c)) & 0xFFu) | 0x80u);
      } else {
        px[0] = px[1] = px[2] = aov_byte((double)v[i] / (double)samples);
      }
    }
    const std::string name = k == planes - 1 ? std::string("rest")
                                             : (is_id ? "id" + std::to_string(k) : "coverage" + std::to_string(k - (size_t)mp.ranks));
    const std::string fp = prefix + "." + name + ext;
    printf("Saving to: %s\n", fp.c_str());
    fflush(stdout);
    rc = ext == ".ppm" ? rt_write_ppm(fp.c_str(), img.data(), w, h) : rt_write_png(fp.c_str(), img.data(), w, h);
    if (rc != RT_OK) {
      printf("Error saving image: %s\n", rt_last_error());
      return rc;
    }
  }
  return RT_OK;
}

// --denoise: the à-trous filter (rt_denoise_async) over the
// frame's linear radiance `linear` (host, w*h*3) on device 0: the first-hit
// feature buffers of the frame with feature_samples samples (st's seed and
// camera model), then the filter; rgba (host, w*h*4) receives its tone-mapped
// output.  vs (--denoise-variance): the filter is
// rt_denoise_var_async, steered by rt_variance_async's spatial estimate.  er (--edge-resolve): the
// filter's linear output goes through the edge resolve, whose image rgba then receives.
static int denoise_image(const rt_scene* scene, int32_t w, int32_t h, const rt_settings& st, int feature_samples,
                         const rt_denoise& dn, const float* linear, uint8_t* rgba, const VarianceSpec* vs = nullptr,
                         const EdgeResolve* er = nullptr) {
  const size_t npix = (size_t)w * (size_t)h;
  rt_context* ctx = nullptr;
  int rc = rt_context_create(0, &ctx);
  if (rc != RT_OK) return rc;
  rc = rt_context_set_scene(ctx, scene, 0);
  // one device block: color | albedo | normal | depth | object | variance, then the image and the workspace
  float* d = nullptr;
  uint8_t* d_rgba = nullptr;
  void* d_work = nullptr;
  float* d_den = nullptr;  // the filter's linear output, with --edge-resolve only
  const size_t work_bytes = vs ? rt_denoise_var_workspace_bytes(w, h) : rt_denoise_workspace_bytes(w, h);
  auto hip_ok = [&](hipError_t e, const char* what) {
    if (e == hipSuccess) return true;
    fprintf(stderr, "%s failed: %s\n", what, hipGetErrorString(e));
    rc = RT_E_DEVICE;
    return false;
  };
  if (rc == RT_OK && hip_ok(hipMalloc((void**)&d, npix * 12 * sizeof(float)), "hipMalloc") &&
      hip_ok(hipMalloc((void**)&d_rgba, npix * 4), "hipMalloc") && hip_ok(hipMalloc(&d_work, work_bytes), "hipMalloc"))
    hip_ok(hipMemcpy(d, linear, npix * 3 * sizeof(float), hipMemcpyHostToDevice), "hipMemcpy");
  if (rc == RT_OK && er) hip_ok(hipMalloc((void**)&d_den, npix * 3 * sizeof(float)), "hipMalloc");
  if (rc == RT_OK) {
    rt_settings fst = st;
    fst.samples = feature_samples;
    rc = guide_pass(ctx, w, h, &fst, nullptr, d + npix * 3, d + npix * 6, d + npix * 9, (int32_t*)(d + npix * 10));
  }
  if (rc == RT_OK) {
    const rt_denoise_inputs in = {d, d + npix * 6, d + npix * 9, d + npix * 3, (const int32_t*)(d + npix * 10)};
    if (vs) {
      const rt_variance_inputs vin = {in.color, in.normal, in.depth, in.albedo, in.object, nullptr, nullptr};
      rc = rt_variance_async(&vs->vr, w, h, &vin, d + npix * 11, nullptr);
      if (rc == RT_OK)
        rc = rt_denoise_var_async(&vs->dv, w, h, &in, d + npix * 11, d_den, d_rgba, nullptr, d_work, work_bytes, nullptr);
    } else {
      rc = rt_denoise_async(&dn, w, h, &in, d_den, d_rgba, d_work, work_bytes, nullptr);
    }
  }
  // (the first-hit ids: the guide's own unless it looked through the mirrors)
  if (rc == RT_OK && er)
    rc = edge_resolve_device(ctx, w, h, st, feature_samples, *er, d_den,
                             g_spec_on ? nullptr : (const int32_t*)(d + npix * 10), d_rgba);
  if (rc == RT_OK) hip_ok(hipMemcpy(rgba, d_rgba, npix * 4, hipMemcpyDeviceToHost), "hipMemcpy");
  const std::string err = rc != RT_OK ? rt_last_error() : "";  // (before the clean-up's calls)
  for (void* p : {(void*)d, (void*)d_rgba, d_work, (void*)d_den})
    if (p) (void)hipFree(p);
  rt_context_destroy(ctx);
  if (rc != RT_OK && !err.empty()) fprintf(stderr, "%s\n", err.c_str());
  return rc;
}

// --denoise SPEC: `default`, or LEVELS[,SIGMA_COLOR[,SIGMA_DEPTH[,NORMAL_POWER]]] over the defaults
// within rt_denoise's ranges (include/rt_api.h), checked before anything is rendered
static bool denoise_in_range(const rt_denoise& d) {
  const int32_t np = d.normal_power;
  return d.levels >= 1 && d.levels <= 8 && np >= 0 && np <= 128 && (np & (np - 1)) == 0 && std::isfinite(d.sigma_color) &&
         d.sigma_color >= 0 && std::isfinite(d.sigma_depth) && d.sigma_depth >= 0;
}
static bool parse_denoise(const std::string& x, rt_denoise* dn) {
  rt_denoise_default(dn);
  if (x == "default") return true;
  if (x.empty()) return false;
  size_t pos = 0;
  for (int nf = 0;; ++nf) {
    if (nf == 4) return false;  // a fifth field
    const size_t c = x.find(',', pos);
    const std::string part = x.substr(pos, c == std::string::npos ? std::string::npos : c - pos);
    long long v = 0;
    if (nf == 0 || nf == 3) {
      if (!parse_int(part.c_str(), &v) || v < -1000 || v > 1000) return false;
      (nf == 0 ? dn->levels : dn->normal_power) = (int32_t)v;
    } else {
      char* end = nullptr;
      errno = 0;
      const double f = strtod(part.c_str(), &end);
      if (part.empty() || !end || *end || errno != 0) return false;
      (nf == 1 ? dn->sigma_color : dn->sigma_depth) = f;
    }
    if (c == std::string::npos) return true;
    pos = c + 1;
  }
}

// --denoise-variance SPEC: `default`, or LEVELS[,SIGMA_LUM[,SIGMA_DEPTH[,NORMAL_POWER]]] over the defaults within
// rt_denoise_var's ranges (include/rt_api.h), checked before anything is rendered; SIGMA_DEPTH and NORMAL_POWER
// are the variance pass's too
static bool parse_denoise_variance(const std::string& x, VarianceSpec* vs) {
  rt_denoise_var_default(&vs->dv);
  rt_variance_default(&vs->vr);
  if (x == "default") return true;
  rt_denoise dn;  // (the same four fields in the same places: sigma_color stands for SIGMA_LUM)
  if (!parse_denoise(x, &dn)) return false;
  const bool has2 = std::count(x.begin(), x.end(), ',') >= 1, has3 = std::count(x.begin(), x.end(), ',') >= 2,
             has4 = std::count(x.begin(), x.end(), ',') >= 3;
  vs->dv.levels = dn.levels;
  if (has2) vs->dv.sigma_lum = dn.sigma_color;
  if (has3) vs->dv.sigma_depth = vs->vr.sigma_depth = dn.sigma_depth;
  if (has4) vs->dv.normal_power = vs->vr.normal_power = dn.normal_power;
  const int32_t np = vs->dv.normal_power;
  return vs->dv.levels >= 1 && vs->dv.levels <= 8 && np >= 0 && np <= 128 && (np & (np - 1)) == 0 &&
         std::isfinite(vs->dv.sigma_lum) && vs->dv.sigma_lum >= 0 && std::isfinite(vs->dv.sigma_depth) &&
         vs->dv.sigma_depth >= 0;
}

// --temporal SPEC: `default`, or MAX_HISTORY[,DEPTH_TOL[,NORMAL_MIN]] over the defaults within
// rt_temporal's ranges (include/rt_api.h), checked before anything is rendered
static bool parse_temporal(const std::string& x, rt_temporal* tp) {
  rt_temporal_default(tp);
  if (x == "default") return true;
  if (x.empty()) return false;
  size_t pos = 0;
  for (int nf = 0;; ++nf) {
    if (nf == 3) return false;  // a fourth field
    const size_t c = x.find(',', pos);
    const std::string part = x.substr(pos, c == std::string::npos ? std::string::npos : c - pos);
    char* end = nullptr;
    errno = 0;
    const double f = strtod(part.c_str(), &end);
    if (part.empty() || !end || *end || errno != 0) return false;
    (nf == 0 ? tp->max_history : nf == 1 ? tp->depth_tol : tp->normal_min) = f;
    if (c == std::string::npos) break;
    pos = c + 1;
  }
  return std::isfinite(tp->max_history) && tp->max_history >= 1 && std::isfinite(tp->depth_tol) && tp->depth_tol >= 0 &&
         tp->normal_min >= -1 && tp->normal_min <= 1;
}

// --clip SPEC: `default`, or RADIUS[,GAMMA[,MIN_TAPS[,MIN_HALF]]] over the defaults within rt_history_clip's
// ranges (include/rt_api.h), checked before anything is rendered
static bool parse_clip(const std::string& x, rt_history_clip* hc) {
  rt_history_clip_default(hc);
  if (x == "default") return true;
  if (x.empty()) return false;
  size_t pos = 0;
  for (int nf = 0;; ++nf) {
    if (nf == 4) return false;  // a fifth field
    const size_t c = x.find(',', pos);
    const std::string part = x.substr(pos, c == std::string::npos ? std::string::npos : c - pos);
    if (nf == 0 || nf == 2) {
      long long v = 0;
      if (!parse_int(part.c_str(), &v) || v < -1 || v > 1000000) return false;
      (nf == 0 ? hc->radius : hc->min_taps) = (int32_t)v;
    } else {
      char* end = nullptr;
      errno = 0;
      const double f = strtod(part.c_str(), &end);
      if (part.empty() || !end || *end || errno != 0) return false;
      (nf == 1 ? hc->gamma : hc->min_half) = f;
    }
    if (c == std::string::npos) break;
    pos = c + 1;
  }
  return hc->radius >= 0 && hc->radius <= 4 && hc->min_taps >= 1 && std::isfinite(hc->gamma) && hc->gamma >= 0 &&
         std::isfinite(hc->min_half) && hc->min_half >= 0;
}

// --edge-resolve SPEC: `default`, or SAMPLES[,RADIUS] over 16 and rt_matte_resolve_default's radius
static bool parse_edge_resolve(const std::string& x, EdgeResolve* er) {
  er->samples = 16;
  rt_matte_resolve_default(&er->rs);
  if (x == "default") return true;
  if (x.empty()) return false;
  const size_t c = x.find(',');
  long long v = 0;
  if (!parse_int(x.substr(0, c).c_str(), &v) || v < 1 || v > (1 << 24)) return false;
  er->samples = (int32_t)v;
  if (c != std::string::npos) {
    if (!parse_int(x.substr(c + 1).c_str(), &v) || v < 1 || v > 4) return false;
    er->rs.radius = (int32_t)v;
  }
  return true;
}

// --matte SPEC: PREFIX[,SAMPLES[,RANKS[,object|face]]] over 16 samples and rt_matte_default
static bool parse_matte(const std::string& x, std::string* prefix, int32_t* samples, rt_matte* mp) {
  *samples = 16;
  rt_matte_default(mp);
  size_t pos = 0;
  for (int nf = 0;; ++nf) {
    if (nf == 4) return false;  // a fifth field
    const size_t c = x.find(',', pos);
    const std::string part = x.substr(pos, c == std::string::npos ? std::string::npos : c - pos);
    long long v = 0;
    if (nf == 0) {
      if (part.empty()) return false;
      *prefix = part;
    } else if (nf == 1) {
      if (!parse_int(part.c_str(), &v) || v < 1 || v > (1 << 24)) return false;
      *samples = (int32_t)v;
    } else if (nf == 2) {
      if (!parse_int(part.c_str(), &v) || v < 1 || v > RT_MATTE_MAX_RANKS) return false;
      mp->ranks = (int32_t)v;
    } else if (part == "object" || part == "face") {
      mp->level = part == "face" ? RT_MATTE_FACE : RT_MATTE_OBJECT;
    } else {
      return false;
    }
    if (c == std::string::npos) return true;
    pos = c + 1;
  }
}

// --move SPEC: K:DX,DY,DZ -- an object index and three finite doubles
static bool parse_move(const std::string& x, long long* k, double v[3]) {
  const size_t colon = x.find(':');
  if (colon == std::string::npos || colon == 0) return false;
  if (!parse_int(x.substr(0, colon).c_str(), k) || *k < 0) return false;
  size_t pos = colon + 1;
  for (int nf = 0; nf < 3; ++nf) {
    const size_t c = x.find(',', pos);
    if ((c == std::string::npos) != (nf == 2)) return false;  // exactly three fields
    const std::string part = x.substr(pos, c == std::string::npos ? std::string::npos : c - pos);
    char* end = nullptr;
    errno = 0;
    v[nf] = strtod(part.c_str(), &end);
    if (part.empty() || !end || *end || errno != 0 || !std::isfinite(v[nf])) return false;
    pos = c + 1;
  }
  return true;
}

int main(int argc, char** argv) {
  std::vector<std::string> args;
  struct Move {
    long long k;
    double v[3];
  };
  std::vector<Move> moves;     // --move K:DX,DY,DZ, repeatable
  bool clip_on = false;        // --clip SPEC
  rt_history_clip hclip;
  rt_history_clip_default(&hclip);
  bool temporal_on = false;    // --temporal SPEC
  rt_temporal tpar;
  rt_temporal_default(&tpar);
  bool denoise_on = false;     // --denoise SPEC
  rt_denoise dn;
  rt_denoise_default(&dn);
  bool variance_on = false;    // --denoise-variance SPEC
  VarianceSpec vspec;
  rt_denoise_var_default(&vspec.dv);
  rt_variance_default(&vspec.vr);
  std::string aov_prefix;      // --aov PREFIX (empty: no feature buffers)
  std::string matte_prefix;    // --matte PREFIX[,...] (empty: no matte layers)
  int32_t matte_samples = 16;
  rt_matte mpar;
  rt_matte_default(&mpar);
  bool resolve_on = false;     // --edge-resolve SPEC
  EdgeResolve eres;
  long long orbit_n = 0;       // --orbit N[,DEGREES] (0: one render)
  double orbit_deg = 360.0;
  double watchdog_s = 0;  // --watchdog (0: no bound, as Go's Render)
  long long pass_samples = 0, converge = -1;  // --pass-samples (0: one render), --converge (-1: off)
  double budget_s = -1;                       // --time-budget (-1: off)
  bool adaptive_on = false;                   // --adaptive TOL[,PATIENCE[,MIN]]
  rt_adaptive adapt = {0, 1, 0, 0};
  std::string count_map;                      // --count-map FILE
  rt_settings st;
  rt_settings_default(&st);
  st.num_workers = (int32_t)sysconf(_SC_NPROCESSORS_ONLN);  // runtime.NumCPU(), main.go:46
  for (int i = 1; i < argc; ++i) {
    std::string a = argv[i];
    long long v;
    auto need = [&](const char* name) -> const char* {
      if (i + 1 >= argc) {
        fprintf(stderr, "flag needs an argument: %s\n", name);
        exit(2);
      }
      return argv[++i];
    };
    if (a == "--samples") {
      if (!parse_int(need("--samples"), &v) || v < 0) return 2;
      st.samples = (int32_t)v;
    } else if (a == "--max-depth") {
      if (!parse_int(need("--max-depth"), &v)) return 2;
      st.max_depth = (int32_t)v;
    } else if (a == "--seed") {
      if (!parse_int(need("--seed"), &v)) return 2;
      st.seed = (uint64_t)v;
    } else if (a == "--no-soft-shadows") {
      st.soft_shadows = 0;
    } else if (a == "--no-recursive") {
      st.recursive_reflections = 0;
    } else if (a == "--devices") {  // GPUs the tiles are sharded over (rt_settings.num_devices)
      if (!parse_int(need("--devices"), &v) || v < 1) return 2;
      st.num_devices = (int32_t)v;
    } else if (a == "--watchdog") {  // multi-device frames: RT_E_TIMEOUT after SECONDS (rt_renderer_set_watchdog)
      const char* x = need("--watchdog");
      char* end = nullptr;
      watchdog_s = strtod(x, &end);
      if (!end || *end || !(watchdog_s >= 0)) {
        fprintf(stderr, "invalid --watchdog %s\n", x);
        return 2;
      }
    } else if (a == "--pass-samples") {  // progressive: N samples per pass, --samples is the cap
      const char* x = need("--pass-samples");
      if (!parse_int(x, &v) || v < 1 || v > (1 << 24)) {
        fprintf(stderr, "invalid --pass-samples %s\n", x);
        return 2;
      }
      pass_samples = v;
    } else if (a == "--time-budget") {  // progressive: stop after the pass at which SECONDS have passed
      const char* x = need("--time-budget");
      char* end = nullptr;
      budget_s = strtod(x, &end);
      if (!end || end == x || *end || !(budget_s >= 0)) {
        fprintf(stderr, "invalid --time-budget %s\n", x);
        return 2;
      }
    } else if (a == "--converge") {  // progressive: stop once a pass changed at most PIXELS pixels
      const char* x = need("--converge");
      if (!parse_int(x, &v) || v < 0) {
        fprintf(stderr, "invalid --converge %s\n", x);
        return 2;
      }
      converge = v;
    } else if (a == "--adaptive") {  // progressive: every pixel stops on its own
      const std::string x = need("--adaptive");
      long long f[3] = {0, 1, 0};
      size_t pos = 0;
      int nf = 0;
      bool ok = !x.empty();
      while (ok && nf < 3) {
        const size_t c = x.find(',', pos);
        const std::string part = x.substr(pos, c == std::string::npos ? std::string::npos : c - pos);
        ok = parse_int(part.c_str(), &f[nf]);
        nf += 1;
        if (c == std::string::npos) break;
        pos = c + 1;
        if (nf == 3) ok = false;  // a fourth field
      }
      if (!ok || f[0] < 0 || f[0] > 255 || f[1] < 1 || f[1] > (1 << 24) || f[2] < 0 || f[2] > (1 << 24)) {
        fprintf(stderr, "invalid --adaptive %s (TOL[,PATIENCE[,MIN]]: 0..255, >= 1, >= 0)\n", x.c_str());
        return 2;
      }
      adapt.tolerance = (int32_t)f[0];
      adapt.patience = (int32_t)f[1];
      adapt.min_samples = (int32_t)f[2];
      adaptive_on = true;
    } else if (a == "--orbit") {  // N views around the scene's lookAt
      const std::string x = need("--orbit");
      const size_t comma = x.find(',');
      bool ok = parse_int(x.substr(0, comma).c_str(), &v) && v >= 1 && v <= 9999;  // (four digits name a file)
      if (ok && comma != std::string::npos) {
        char* end = nullptr;
        errno = 0;
        orbit_deg = strtod(x.c_str() + comma + 1, &end);
        ok = end && end != x.c_str() + comma + 1 && *end == 0 && errno == 0 && orbit_deg == orbit_deg &&
             orbit_deg - orbit_deg == 0;  // (finite)
      }
      if (!ok) {
        fprintf(stderr, "invalid --orbit %s (N[,DEGREES]: N in 1..9999)\n", x.c_str());
        return 2;
      }
      orbit_n = v;
    } else if (a == "--count-map") {  // --adaptive: the per-pixel sample counts as a grey PNG
      count_map = need("--count-map");
    } else if (a == "--aov") {  // the first-hit feature buffers as five images PREFIX.<name><ext>
      aov_prefix = need("--aov");
      if (aov_prefix.empty()) {
        fprintf(stderr, "invalid --aov (a file name prefix)\n");
        return 2;
      }
    } else if (a == "--matte") {  // the matte layers as images PREFIX.id<r>, .coverage<r>, .rest
      const std::string x = need("--matte");
      if (!parse_matte(x, &matte_prefix, &matte_samples, &mpar)) {
        fprintf(stderr, "invalid --matte %s (PREFIX[,SAMPLES[,RANKS[,object|face]]]: samples >= 1, ranks 1..8)\n", x.c_str());
        return 2;
      }
    } else if (a == "--edge-resolve") {  // antialias the written image's silhouettes
      const std::string x = need("--edge-resolve");
      if (!parse_edge_resolve(x, &eres)) {
        fprintf(stderr, "invalid --edge-resolve %s (default, or SAMPLES[,RADIUS]: samples >= 1, radius 1..4)\n", x.c_str());
        return 2;
      }
      resolve_on = true;
    } else if (a == "--aov-specular") {  // the feature pass follows mirrors
      const std::string x = need("--aov-specular");
      rt_aov_spec_default(&g_spec);
      bool ok = !x.empty();
      if (ok && x != "default") {
        const size_t comma = x.find(',');
        ok = parse_int(x.substr(0, comma).c_str(), &v) && v >= 0 && v <= 16;
        if (ok) g_spec.max_bounces = (int32_t)v;
        if (ok && comma != std::string::npos) {
          char* end = nullptr;
          errno = 0;
          g_spec.max_roughness = strtod(x.c_str() + comma + 1, &end);
          ok = end && end != x.c_str() + comma + 1 && *end == 0 && errno == 0 && std::isfinite(g_spec.max_roughness) &&
               g_spec.max_roughness >= 0;
        }
      }
      if (!ok) {
        fprintf(stderr, "invalid --aov-specular %s (default, or BOUNCES[,MAX_ROUGHNESS]: 0..16, finite and >= 0)\n",
                x.c_str());
        return 2;
      }
      g_spec_on = true;
    } else if (a == "--denoise") {  // write the à-trous-filtered image
      const std::string x = need("--denoise");
      if (!parse_denoise(x, &dn) || !denoise_in_range(dn)) {
        fprintf(stderr, "invalid --denoise %s (default, or LEVELS[,SIGMA_COLOR[,SIGMA_DEPTH[,NORMAL_POWER]]]: 1..8, "
                        ">= 0, >= 0, 0 or a power of two <= 128)\n", x.c_str());
        return 2;
      }
      denoise_on = true;
    } else if (a == "--denoise-variance") {  // write the variance-guided filter's image
      const std::string x = need("--denoise-variance");
      if (!parse_denoise_variance(x, &vspec)) {
        fprintf(stderr, "invalid --denoise-variance %s (default, or LEVELS[,SIGMA_LUM[,SIGMA_DEPTH[,NORMAL_POWER]]]: "
                        "1..8, >= 0, >= 0, 0 or a power of two <= 128)\n", x.c_str());
        return 2;
      }
      variance_on = true;
    } else if (a == "--temporal") {  // --orbit: write the accumulated views
      const std::string x = need("--temporal");
      if (!parse_temporal(x, &tpar)) {
        fprintf(stderr, "invalid --temporal %s (default, or MAX_HISTORY[,DEPTH_TOL[,NORMAL_MIN]]: >= 1, >= 0, "
                        "-1..1)\n", x.c_str());
        return 2;
      }
      temporal_on = true;
    } else if (a == "--clip") {  // --orbit --temporal: rectify the reprojected history
      const std::string x = need("--clip");
      if (!parse_clip(x, &hclip)) {
        fprintf(stderr, "invalid --clip %s (default, or RADIUS[,GAMMA[,MIN_TAPS[,MIN_HALF]]]: radius 0..4, gamma >= 0, "
                        "min_taps >= 1, min_half >= 0)\n", x.c_str());
        return 2;
      }
      clip_on = true;
    } else if (a == "--move") {  // --orbit: object K is offset by f * (DX, DY, DZ) at view f
      const std::string x = need("--move");
      Move mv;
      if (!parse_move(x, &mv.k, mv.v)) {
        fprintf(stderr, "invalid --move %s (K:DX,DY,DZ: an object index >= 0 and three finite numbers)\n", x.c_str());
        return 2;
      }
      for (const Move& o : moves)
        if (o.k == mv.k) {
          fprintf(stderr, "invalid --move %s (object %lld is given twice)\n", x.c_str(), mv.k);
          return 2;
        }
      moves.push_back(mv);
    } else if (a == "--sky") {  // opt-in sky on miss (atmosphere.go presets); default: black
      const std::string k = need("--sky");
      if (k == "none") st.sky = RT_SKY_NONE;
      else if (k == "default") st.sky = RT_SKY_DEFAULT;
      else if (k == "white") st.sky = RT_SKY_WHITE;
      else if (k == "sunset") st.sky = RT_SKY_SUNSET;
      else if (k == "night") st.sky = RT_SKY_NIGHT;
      else {
        fprintf(stderr, "unknown --sky %s\n", k.c_str());
        return 2;
      }
    } else if (a == "--camera") {  // reference (default): getRay's fixed -Z view; lookat: the scene's own camera
      const std::string k = need("--camera");
      if (k == "reference") st.camera = RT_CAMERA_REFERENCE;
      else if (k == "lookat") st.camera = RT_CAMERA_LOOKAT;
      else {
        fprintf(stderr, "unknown --camera %s (reference or lookat)\n", k.c_str());
        return 1;
      }
    } else {
      args.push_back(a);
    }
  }
  if (orbit_n > 0 && (pass_samples > 0 || adaptive_on || st.num_devices > 1)) {
    fprintf(stderr, "--orbit renders whole frames on one device: not with --pass-samples, --adaptive or --devices > 1\n");
    return 2;
  }
  if (!aov_prefix.empty() && (orbit_n > 0 || st.samples < 1)) {
    fprintf(stderr, "--aov needs --samples >= 1 and one view (not with --orbit)\n");
    return 2;
  }
  if (g_spec_on && aov_prefix.empty() && !denoise_on && !variance_on) {
    fprintf(stderr, "--aov-specular picks the feature pass of --aov, --denoise or --denoise-variance: give one of them\n");
    return 2;
  }
  if ((resolve_on || !matte_prefix.empty()) && orbit_n > 0) {
    fprintf(stderr, "--matte and --edge-resolve need one view (not with --orbit)\n");
    return 2;
  }
  if (resolve_on && st.samples < 1) {
    fprintf(stderr, "--edge-resolve needs --samples >= 1\n");
    return 2;
  }
  if (temporal_on && (orbit_n <= 0 || st.samples < 1)) {
    fprintf(stderr, "--temporal accumulates the views of --orbit and needs --samples >= 1\n");
    return 2;
  }
  if (clip_on && (orbit_n <= 0 || !temporal_on)) {
    fprintf(stderr, "--clip rectifies the history of --temporal and needs --orbit N --temporal SPEC\n");
    return 2;
  }
  if (!moves.empty() && orbit_n <= 0) {
    fprintf(stderr, "--move moves objects from view to view and needs --orbit\n");
    return 2;
  }
  if (denoise_on && ((orbit_n > 0 && !temporal_on) || st.samples < 1)) {
    fprintf(stderr, "--denoise needs --samples >= 1 and one view (with --orbit only together with --temporal)\n");
    return 2;
  }
  if (variance_on && (denoise_on || pass_samples > 0 || (orbit_n > 0 && !temporal_on) || st.samples < 1)) {
    fprintf(stderr, "--denoise-variance needs --samples >= 1 and one plain render, or --orbit together with --temporal; "
                    "not with --denoise or --pass-samples\n");
    return 2;
  }
  if (variance_on) denoise_on = true;  // (from here on: the filtered image is the one written; vspec says by which filter)
  if (pass_samples > 0 && st.num_devices > 1) {
    fprintf(stderr, "--pass-samples renders on one device (--devices %d)\n", st.num_devices);
    return 2;
  }
  if (pass_samples > 0 && st.samples < 1) {
    fprintf(stderr, "--pass-samples needs --samples >= 1 (the cap)\n");
    return 2;
  }
  if (pass_samples == 0 && (budget_s >= 0 || converge >= 0)) {
    fprintf(stderr, "--time-budget and --converge need --pass-samples\n");
    return 2;
  }
  if (pass_samples == 0 && (adaptive_on || !count_map.empty())) {
    fprintf(stderr, "--adaptive and --count-map need --pass-samples\n");
    return 2;
  }
  if (adaptive_on && st.sky != RT_SKY_NONE) {
    fprintf(stderr, "--adaptive does not support --sky\n");
    return 2;
  }
  if (args.size() < 4) {
    printf("Usage: raytracer <scene_file> <output_file> <width> <height>\n");
    printf("Example: raytracer scene.json output.png 800 600\n");
    return 1;
  }
  const std::string scene_file = args[0];
  const std::string output_file = args[1];
  long long w, h;
  if (!parse_int(args[2].c_str(), &w)) {
    printf("Invalid width: %s\n", args[2].c_str());
    return 1;
  }
  if (!parse_int(args[3].c_str(), &h)) {
    printf("Invalid height: %s\n", args[3].c_str());
    return 1;
  }
  if (denoise_on && (w <= 0 || h <= 0)) {
    fprintf(stderr, "%s needs a size with pixels (%lldx%lld)\n", variance_on ? "--denoise-variance" : "--denoise", w, h);
    return 2;
  }
  if ((resolve_on || !matte_prefix.empty()) && (w <= 0 || h <= 0)) {
    fprintf(stderr, "--matte and --edge-resolve need a size with pixels (%lldx%lld)\n", w, h);
    return 2;
  }
  const bool keep_linear = denoise_on || resolve_on;  // (the frame's linear image on the host)
  printf("Loading scene from: %s\n", scene_file.c_str());
  rt_scene_buf* sb = nullptr;
  if (rt_scene_load_json(scene_file.c_str(), 0, &sb) != RT_OK) {
    printf("Error loading scene: %s\n", rt_last_error());
    return 1;
  }
  std::vector<double> move_table;  // --move: num_objects * 3, each object's offset per view
  if (!moves.empty()) {
    const long long nobj = rt_scene_view(sb)->num_objects;
    move_table.assign((size_t)std::max(nobj, 0LL) * 3, 0.0);
    for (const Move& mv : moves) {
      if (mv.k >= nobj) {
        fprintf(stderr, "invalid --move %lld:...: the scene has %lld objects\n", mv.k, nobj);
        rt_scene_free(sb);
        return 2;
      }
      for (int j = 0; j < 3; ++j) move_table[(size_t)mv.k * 3 + j] = mv.v[j];
    }
  }
  const long long aw = llabs(w), ah = llabs(h);
  if ((w <= 0 || h <= 0) && aw <= 65536 && ah <= 65536) {
    // A size with no tile: createRenderTasks makes none (renderer.go:401-403:
    // (n + 31) / 32 <= 0), so Go renders nothing.  image.Rect canonicalizes
    // the rectangle (renderer.go:70): the image is |w| x |h|, every pixel
    // zero (transparent black), which png.Encode writes as RGBA8 (exit 0);
    // with |w| or |h| zero, SaveImage creates the file and png.Encode fails
    // ("invalid image size", exit 1).  No GPU is involved either way, so
    // this is decided before any device state exists.
    const auto t0 = std::chrono::steady_clock::now();
    printf("Rendering at %lldx%lld resolution...\n", w, h);
    rt_scene_print_hittables(sb);
    rt_stats stats;
    memset(&stats, 0, sizeof stats);
    stats.objects = rt_scene_view(sb)->num_objects;
    stats.lights = rt_scene_view(sb)->num_lights;
    stats.render_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    print_complete();
    std::string out_path = output_file;
    if (ext_of(out_path).empty()) out_path += ".png";
    printf("Saving to: %s\n", out_path.c_str());
    int rc = RT_OK;
    if (aw == 0 || ah == 0) {
      // os.Create succeeded, png.Encode refused the empty image
      mkdir_p(dir_of(out_path));  // os.MkdirAll (renderer.go:439-442)
      FILE* f = fopen(out_path.c_str(), "wb");
      if (!f) {
        printf("Error saving image: open %s: %s\n", out_path.c_str(), strerror(errno));
      } else {
        fclose(f);
        printf("Error saving image: png: invalid format: invalid image size: %lldx%lld\n", aw, ah);
      }
      rt_scene_free(sb);
      return 1;
    }
    std::vector<uint8_t> rgba((size_t)aw * (size_t)ah * 4, 0);
    rc = ext_of(out_path) == ".ppm" ? rt_write_ppm(out_path.c_str(), rgba.data(), (int32_t)aw, (int32_t)ah)
                                    : rt_write_png(out_path.c_str(), rgba.data(), (int32_t)aw, (int32_t)ah);
    if (rc != RT_OK) {
      printf("Error saving image: %s\n", rt_last_error());
      rt_scene_free(sb);
      return 1;
    }
    save_benchmark(out_path, w, h, st, stats);
    rt_scene_free(sb);
    return 0;
  }
  // (--denoise holds the frame's linear image on the host: sized only for a frame that will render)
  if (keep_linear && (w > 65536 || h > 65536 || rt_validate(rt_scene_view(sb), (int32_t)w, (int32_t)h, &st) != RT_OK)) {
    fprintf(stderr, "render failed: %s\n", w > 65536 || h > 65536 ? "invalid image size" : rt_last_error());
    rt_scene_free(sb);
    return 2;
  }
  if (orbit_n > 0) {
    printf("Rendering at %lldx%lld resolution...\n", w, h);
    fflush(stdout);
    rt_scene_print_hittables(sb);
    const size_t npix = (size_t)w * (size_t)h;
    rt_stats stats;
    memset(&stats, 0, sizeof stats);
    std::string out_path = output_file;
    if (ext_of(out_path).empty()) out_path += ".png";
    const std::string ext = ext_of(out_path), stem = out_path.substr(0, out_path.size() - ext.size());
    bool save_failed = false;
    // (each launch's frames are written as they arrive: the host holds one launch's images)
    auto save = [&](int f0, int m, const uint8_t* imgs) {
      for (int f = 0; f < m; ++f) {
        char num[32];
        snprintf(num, sizeof num, "_%04d", f0 + f);
        const std::string fp = stem + num + ext;
        printf("Saving to: %s\n", fp.c_str());
        fflush(stdout);
        const uint8_t* img = imgs + (size_t)f * npix * 4;
        const int rc = ext == ".ppm" ? rt_write_ppm(fp.c_str(), img, (int32_t)w, (int32_t)h)
                                     : rt_write_png(fp.c_str(), img, (int32_t)w, (int32_t)h);
        if (rc != RT_OK) {
          printf("Error saving image: %s\n", rt_last_error());
          save_failed = true;
          return false;
        }
      }
      return true;
    };
    if (rt_validate(rt_scene_view(sb), (int32_t)w, (int32_t)h, &st) != RT_OK ||
        render_orbit(rt_scene_view(sb), (int32_t)w, (int32_t)h, st, (int)orbit_n, orbit_deg, save, &stats,
                     temporal_on ? &tpar : nullptr, denoise_on && !variance_on ? &dn : nullptr,
                     variance_on ? &vspec : nullptr, moves.empty() ? nullptr : move_table.data(), clip_on ? &hclip : nullptr) != RT_OK) {
      if (!save_failed) fprintf(stderr, "render failed: %s\n", rt_last_error());
      rt_scene_free(sb);
      return save_failed ? 1 : 2;
    }
    print_complete();
    save_benchmark(out_path, w, h, st, stats, -1, orbit_n);
    rt_scene_free(sb);
    return 0;
  }
  if (pass_samples > 0) {
    printf("Rendering at %lldx%lld resolution...\n", w, h);
    fflush(stdout);
    rt_scene_print_hittables(sb);
    std::vector<uint8_t> rgba((size_t)w * (size_t)h * 4);
    rt_stats stats;
    memset(&stats, 0, sizeof stats);
    int rendered = 0;
    double mean_samples = -1;
    std::vector<float> linear(keep_linear ? (size_t)w * (size_t)h * 3 : 0);
    if (rt_validate(rt_scene_view(sb), (int32_t)w, (int32_t)h, &st) != RT_OK ||
        render_progressive(rt_scene_view(sb), (int32_t)w, (int32_t)h, st, (int)pass_samples, budget_s, converge,
                           adaptive_on ? &adapt : nullptr, count_map, rgba.data(), &stats, &rendered,
                           &mean_samples, keep_linear ? linear.data() : nullptr) != RT_OK) {
      fprintf(stderr, "render failed: %s\n", rt_last_error());
      rt_scene_free(sb);
      return 2;
    }
    // (the features of the first pass's samples, as ParallelRenderer.render_progressive takes them)
    if (denoise_on && denoise_image(rt_scene_view(sb), (int32_t)w, (int32_t)h, st,
                                    (int)std::min<long long>(st.samples, pass_samples), dn, linear.data(),
                                    rgba.data(), nullptr, resolve_on ? &eres : nullptr) != RT_OK) {
      fprintf(stderr, "denoise failed: %s\n", rt_last_error());
      rt_scene_free(sb);
      return 2;
    }
    if (resolve_on && !denoise_on &&
        resolve_image(rt_scene_view(sb), (int32_t)w, (int32_t)h, st, (int)std::min<long long>(st.samples, pass_samples),
                      eres, linear.data(), rgba.data()) != RT_OK) {
      fprintf(stderr, "edge resolve failed: %s\n", rt_last_error());
      rt_scene_free(sb);
      return 2;
    }
    print_complete();
    std::string out_path = output_file;
    if (ext_of(out_path).empty()) out_path += ".png";
    printf("Saving to: %s\n", out_path.c_str());
    fflush(stdout);
    const int rc = ext_of(out_path) == ".ppm" ? rt_write_ppm(out_path.c_str(), rgba.data(), (int32_t)w, (int32_t)h)
                                              : rt_write_png(out_path.c_str(), rgba.data(), (int32_t)w, (int32_t)h);
    if (rc != RT_OK) {
      printf("Error saving image: %s\n", rt_last_error());
      rt_scene_free(sb);
      return 1;
    }
    if (!aov_prefix.empty() &&
        write_aov(rt_scene_view(sb), (int32_t)w, (int32_t)h, st, aov_prefix, ext_of(out_path)) != RT_OK) {
      rt_scene_free(sb);
      return 1;
    }
    if (!matte_prefix.empty() && write_matte(rt_scene_view(sb), (int32_t)w, (int32_t)h, st, mpar, matte_samples,
                                             matte_prefix, ext_of(out_path)) != RT_OK) {
      rt_scene_free(sb);
      return 1;
    }
    rt_settings done_st = st;
    done_st.samples = rendered;  // (the samples actually rendered)
    save_benchmark(out_path, w, h, done_st, stats, adaptive_on ? mean_samples : -1);
    rt_scene_free(sb);
    return 0;
  }
  // renderer := renderer.NewParallelRenderer(numWorkers) (main.go:46-47):
  // the device state (HIP runtime, context, stream, the kernels' code
  // objects) is the GPU renderer's constructor work, made before Render and
  // outside its time, as the reference's worker pool is
  const auto t_new = std::chrono::steady_clock::now();
  rt_renderer* rr = nullptr;
  if (rt_renderer_create(nullptr, st.num_devices > 1 ? st.num_devices : 1, &rr) != RT_OK) {
    fprintf(stderr, "render failed: %s\n", rt_last_error());
    rt_scene_free(sb);
    return 2;
  }
  if (watchdog_s > 0) rt_renderer_set_watchdog(rr, watchdog_s);
  const double new_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_new).count();
  printf("Rendering at %lldx%lld resolution...\n", w, h);
  fflush(stdout);
  rt_scene_print_hittables(sb);
  const rt_scene* scene = rt_scene_view(sb);
  const size_t npix = (size_t)w * (size_t)h;
  std::vector<uint8_t> rgba(npix * 4);
  rt_stats stats;
  memset(&stats, 0, sizeof stats);
  // img := renderer.Render(scene, width, height) (main.go:51): timed by
  // Render itself (renderer.go:68,101: stats.render_seconds)
  std::vector<float> linear(keep_linear ? npix * 3 : 0);
  int rc = rt_renderer_render(rr, scene, (int32_t)w, (int32_t)h, &st, keep_linear ? linear.data() : nullptr, rgba.data(),
                              &stats);
  if (rc != RT_OK) {
    fprintf(stderr, "render failed: %s\n", rt_last_error());
    rt_renderer_destroy(rr);
    rt_scene_free(sb);
    return 2;
  }
  if (denoise_on &&
      denoise_image(scene, (int32_t)w, (int32_t)h, st, st.samples, dn, linear.data(), rgba.data(),
                    variance_on ? &vspec : nullptr, resolve_on ? &eres : nullptr) != RT_OK) {
    fprintf(stderr, "denoise failed: %s\n", rt_last_error());
    rt_renderer_destroy(rr);
    rt_scene_free(sb);
    return 2;
  }
  if (resolve_on && !denoise_on &&
      resolve_image(scene, (int32_t)w, (int32_t)h, st, st.samples, eres, linear.data(), rgba.data()) != RT_OK) {
    fprintf(stderr, "edge resolve failed: %s\n", rt_last_error());
    rt_renderer_destroy(rr);
    rt_scene_free(sb);
    return 2;
  }
  stats.create_seconds = new_seconds;  // (reported apart: setup_time, render_breakdown_seconds.create)
  print_complete();

  std::string out_path = output_file;
  if (ext_of(out_path).empty()) out_path += ".png";
  printf("Saving to: %s\n", out_path.c_str());
  fflush(stdout);
  rc = ext_of(out_path) == ".ppm" ? rt_write_ppm(out_path.c_str(), rgba.data(), (int32_t)w, (int32_t)h)
                                  : rt_write_png(out_path.c_str(), rgba.data(), (int32_t)w, (int32_t)h);
  if (rc != RT_OK) {
    printf("Error saving image: %s\n", rt_last_error());
    rt_renderer_destroy(rr);
    rt_scene_free(sb);
    return 1;
  }
  if (!aov_prefix.empty() && write_aov(scene, (int32_t)w, (int32_t)h, st, aov_prefix, ext_of(out_path)) != RT_OK) {
    rt_renderer_destroy(rr);
    rt_scene_free(sb);
    return 1;
  }
  if (!matte_prefix.empty() &&
      write_matte(scene, (int32_t)w, (int32_t)h, st, mpar, matte_samples, matte_prefix, ext_of(out_path)) != RT_OK) {
    rt_renderer_destroy(rr);
    rt_scene_free(sb);
    return 1;
  }
  save_benchmark(out_path, w, h, st, stats);
  rt_renderer_destroy(rr);
  rt_scene_free(sb);
  return 0;
}
