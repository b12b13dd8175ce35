// rt_api.cpp — C ABI of librtgo.so (include/rt_api.h): the context's life
// cycle, scene flattening and device residency, tuning, statistics, debug and
// profiling.  The render entry points are in rt_render.cpp (frames),
// rt_progressive.cpp (progressions) and rt_partition.cpp (partitions).
//
// Replaces the Go seam *renderer.ParallelRenderer (renderer.go:54-126,
// settings.go:3-25).  Compiled with -ffp-contract=off: the host-side
// precomputations (cube vertices, triangle edges and normals, material
// tables) must equal the values the reference computes per test.
#include <math.h>
#include <stdlib.h>

#include <chrono>
#include <mutex>
#include <thread>

#include "rt_context.h"

namespace rtgo {

static thread_local std::string g_last_error;
void set_error(const std::string& msg) { g_last_error = msg; }

static int validate_scene(const rt_scene* s) {
  if (!s) {
    set_error("scene is NULL");
    return RT_E_INVALID;
  }
  if (s->num_objects < 0 || s->num_lights < 0 || (s->num_objects > 0 && !s->objects) ||
      (s->num_lights > 0 && !s->lights)) {
    set_error("scene arrays inconsistent");
    return RT_E_INVALID;
  }
  for (int i = 0; i < s->num_objects; ++i) {
    const rt_object& o = s->objects[i];
    if (o.type != RT_OBJ_SPHERE && o.type != RT_OBJ_CUBE) {
      set_error("object " + std::to_string(i) + ": unknown type " + std::to_string(o.type));
      return RT_E_INVALID;
    }
    if (o.material.kind < RT_MAT_LAMBERTIAN || o.material.kind > RT_MAT_DIFFUSELIGHT) {
      set_error("object " + std::to_string(i) + ": unknown material kind");
      return RT_E_INVALID;
    }
  }
  // Non-finite geometry (rt_api.h, rt_context_set_scene): spheres alone are
  // rendered as the reference renders them; a cube with a non-finite position
  // or size, and a non-finite sphere in a scene that has cubes, are refused
  // (the closest hit scans spheres before triangles, which equals the
  // reference's hittable order only while the closest distance is not NaN).
  bool cubes = false;
  for (int i = 0; i < s->num_objects; ++i) cubes = cubes || s->objects[i].type == RT_OBJ_CUBE;
  for (int i = 0; i < s->num_objects && cubes; ++i) {
    const rt_object& o = s->objects[i];
    const char* field = nullptr;
    for (int k = 0; k < 3 && !field; ++k) {
      if (!std::isfinite(o.position[k])) field = "position";
      else if (o.type == RT_OBJ_CUBE && !std::isfinite(o.size[k])) field = "size";
    }
    if (!field && o.type == RT_OBJ_SPHERE && !std::isfinite(o.radius)) field = "radius";
    if (field) {
      set_error("object " + std::to_string(i) + ": " + (o.type == RT_OBJ_CUBE ? "cube " : "sphere ") + field +
                " is not finite" + (o.type == RT_OBJ_CUBE ? "" : " in a scene with cubes") +
                " (non-finite geometry is rendered for spheres alone)");
      return RT_E_INVALID;
    }
  }
  return RT_OK;
}

static int validate_settings(const rt_settings* st, int32_t w, int32_t h) {
  if (!st) {
    set_error("settings is NULL");
    return RT_E_INVALID;
  }
  // (each side at most 65536: the kernel's camera-jitter division relies on it)
  if (w <= 0 || h <= 0 || w > 65536 || h > 65536 || (long long)w * h > (1LL << 31) / 4) {
    set_error("invalid image size " + std::to_string(w) + "x" + std::to_string(h));
    return RT_E_INVALID;
  }
  // (any count: more than kMaxBlockSamples render in sample passes; the
  // bound keeps pixel x sample ids of a frame in 32 bits on every path)
  if (st->samples < 0 || (long long)st->samples * w * h >= (1LL << 40) || st->samples > (1 << 24)) {
    set_error("samples must be in [0, 2^24] with width * height * samples < 2^40");
    return RT_E_INVALID;
  }
  if (st->sky < RT_SKY_NONE || st->sky > RT_SKY_NIGHT) {
    set_error("sky must be one of RT_SKY_*");
    return RT_E_INVALID;
  }
  if (st->camera != RT_CAMERA_REFERENCE && st->camera != RT_CAMERA_LOOKAT) {
    set_error("camera must be RT_CAMERA_REFERENCE or RT_CAMERA_LOOKAT");
    return RT_E_INVALID;
  }
  return RT_OK;
}

int check_settings(const rt_settings* st, int32_t w, int32_t h) { return validate_settings(st, w, h); }

int check_frame(const rt_context* c, int32_t w, int32_t h, const rt_settings* st) {
  const int rc = validate_settings(st, w, h);
  if (rc) return rc;
  CamFrame cf;
  return camera_frame(c->flat.camera, st->camera, w, h, &cf);
}

int check_frame_args(const rt_context* c, int32_t w, int32_t h, const rt_settings* st, int32_t rank, int32_t world,
                     int32_t layout) {
  if (!c || !c->have_scene) {
    set_error("context has no scene");
    return RT_E_INVALID;
  }
  const int rc = check_frame(c, w, h, st);
  if (rc) return rc;
  if (world < 1 || rank < 0 || rank >= world) {
    set_error("invalid rank/world");
    return RT_E_INVALID;
  }
  if (layout != RT_LAYOUT_IMAGE && layout != RT_LAYOUT_PACKED_TILES) {
    set_error("invalid layout");
    return RT_E_INVALID;
  }
  return RT_OK;
}

// Adds the recorded blocks to the totals (waits for them)
int prof_collect(rt_context* c) {
  if (c->prof_pending.empty()) return RT_OK;
  const auto& lastb = c->prof_pending.back();
  HIP_TRY(hipEventSynchronize(c->prof_pool[lastb.base + lastb.last + 1]));
  for (const auto& b : c->prof_pending)
    for (int k = b.first; k <= b.last; ++k) {
      float ms = 0;
      HIP_TRY(hipEventElapsedTime(&ms, c->prof_pool[b.base + k], c->prof_pool[b.base + k + 1]));
      c->prof_secs[k] += ms * 1e-3;
      c->prof_launches[k] += 1;
    }
  c->prof_pending.clear();
  c->prof_used = 0;
  return RT_OK;
}

bool context_has_bvh(const rt_context* c) { return c && !c->flat.bvh.empty(); }
double context_bvh_seconds(const rt_context* c) { return c ? c->bvh_seconds : 0.0; }
void* context_stream(const rt_context* c) { return c ? (void*)c->stream : nullptr; }

double steady_now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

void context_set_deadline(rt_context* c, double deadline) {
  if (c) c->deadline = deadline;
}

// The context's host waits during a render.  Without a deadline they block
// (hipStreamSynchronize / hipEventSynchronize); with one (a multi-rank
// renderer's frame, rt_renderer_set_watchdog) they poll (yield, then 20 us
// sleeps) and return RT_E_TIMEOUT once it has passed, so a stalled rank ends
// the frame instead of blocking its host thread forever.
template <class Query>
int bounded_wait(rt_context* c, Query query, const char* what) {
  for (unsigned spin = 0;; ++spin) {
    const hipError_t e = query();
    if (e == hipSuccess) return RT_OK;
    if (e != hipErrorNotReady) {
      set_error(std::string(what) + " failed: " + hipGetErrorString(e));
      return RT_E_DEVICE;
    }
    if (steady_now_s() > c->deadline) {
      set_error(std::string("watchdog: ") + what + " did not complete before the frame's deadline");
      return RT_E_TIMEOUT;
    }
    if (spin < 256)
      std::this_thread::yield();
    else
      std::this_thread::sleep_for(std::chrono::microseconds(20));
  }
}

int wait_stream(rt_context* c, hipStream_t s) {
  if (c->deadline <= 0) {
    HIP_TRY(hipStreamSynchronize(s));
    return RT_OK;
  }
  return bounded_wait(c, [s] { return hipStreamQuery(s); }, "a wait for the render stream");
}

int wait_event(rt_context* c, hipEvent_t ev) {
  if (c->deadline <= 0) {
    HIP_TRY(hipEventSynchronize(ev));
    return RT_OK;
  }
  return bounded_wait(c, [ev] { return hipEventQuery(ev); }, "a wait for a render event");
}

}  // namespace rtgo

using namespace rtgo;

// ======================================================================== ABI
extern "C" {

int rt_context_set_tuning(rt_context* c, const rt_tuning* t) {
  if (!c || !t) {
    set_error("context or tuning is NULL");
    return RT_E_INVALID;
  }
  if (t->path != RT_PATH_AUTO && t->path != RT_PATH_MEGAKERNEL) {
    set_error("tuning.path must be RT_PATH_AUTO or RT_PATH_MEGAKERNEL");
    return RT_E_INVALID;
  }
  if (t->pilot_depth < 0 || t->split_samples < 0 || t->split_samples > 64 || t->bvh_leaf < 0 || t->bvh_leaf > 7 || t->bvh_bins < 0 || t->block_work < 0 || t->block_samples < 0 ||
      t->wf_paths < 0 || t->wf_chunk < 0 || t->wf_trav_block < 0 || t->wf_trav_block > 1024 || t->wf_trav_wgs < 0 ||
      t->wf_list_tries < 0 || t->wf_list_tries > 64 || t->tail_helpers < -1 || t->tail_helpers > 4096 ||
      t->tail_paths < 0 || t->tail_paths > 64 || t->tail_depth < 0 || t->tail_every < 0 || t->tail_every > 64 ||
      t->tail_at < 0 || t->tail_at > 100 || t->stream < -1 || t->stream > 1 || !(t->stream_max_mb >= 0) || t->stream_max_mb > 1e9 ||
      t->stream_chunk < 0 || t->stream_chunk > 65536 || t->stream_order < 0 || t->stream_order > 1) {
    set_error("tuning value out of range");
    return RT_E_INVALID;
  }
  c->tun = *t;
  c->order_key[0] = -1;  // rebuild the schedule
  c->prog_on = false;    // (a progression ends: its next add is refused)
  return RT_OK;
}

int32_t rt_abi_version(void) { return RT_ABI_VERSION; }

int rt_debug_xlane_faults(int32_t device, int32_t reset, uint64_t* out) {
  if (!out) {
    set_error("out is NULL");
    return RT_E_INVALID;
  }
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipDeviceSynchronize());
  // every unit that includes rt_device.h and shuffles
  const long long n[3] = {xlane_faults_kernel(reset != 0), xlane_faults_stream(reset != 0),
                          xlane_faults_wavefront(reset != 0)};
  uint64_t sum = 0;
  for (const long long v : n) {
    if (v == -1) {
      set_error("not a cross-lane checking build (make xlane)");
      return RT_E_INVALID;
    }
    if (v < 0) {
      set_error("reading the cross-lane fault counters failed");
      return RT_E_DEVICE;
    }
    sum += (uint64_t)v;
  }
  *out = sum;
  return RT_OK;
}

int rt_validate(const rt_scene* scene, int32_t w, int32_t h, const rt_settings* st) {
  int rc = validate_scene(scene);
  if (rc) return rc;
  rc = validate_settings(st, w, h);
  if (rc) return rc;
  CamFrame cf;  // (a degenerate look-at camera: RT_E_INVALID with its message)
  return camera_frame(scene->camera, st->camera, w, h, &cf);
}

int rt_camera_frame(const rt_camera* cam, int32_t model, int32_t w, int32_t h, double out[12]) {
  if (!cam || !out) {
    set_error("camera or out is NULL");
    return RT_E_INVALID;
  }
  CamFrame cf;
  const int rc = camera_frame(*cam, model, w, h, &cf);
  if (rc) return rc;
  memcpy(out, cf.o, 12 * sizeof(double));  // o, ll, h, v are contiguous
  return RT_OK;
}

int rt_scene_cone_rows(const rt_scene* scene, int32_t force_bvh, uint64_t* out, size_t capacity) {
  int rc = validate_scene(scene);
  if (rc) return rc;
  const size_t n = (size_t)scene->num_lights * (size_t)scene->num_objects;
  if (n > 0 && (!out || capacity < n)) {
    set_error("cone rows: out holds " + std::to_string(out ? capacity : 0) + " rows, the scene has " + std::to_string(n));
    return RT_E_INVALID;
  }
  FlatScene f;
  flatten_scene(*scene, &f);
  // (rt_context_set_scene's rule for a tree, and its default build)
  if ((force_bvh > 0 || (force_bvh == 0 && (f.spheres.size() > 64 || f.boxes.size() > (size_t)kAutoBvhCubes))) &&
      spheres_finite(f))
    build_bvh(&f, 0, 0);
  std::vector<unsigned long long> rows;
  cone_rows(f, &rows);
  for (size_t i = 0; i < n; ++i) out[i] = rows[i];
  return RT_OK;
}

int rt_stream_decode(int32_t order, uint32_t frames, uint32_t nlive, uint32_t spp, const uint32_t* entries, size_t n,
                     uint32_t* out) {
  if ((order != 0 && order != 1) || frames == 0 || nlive == 0 || spp == 0 || (n > 0 && (!entries || !out))) {
    set_error("stream decode: order is 0 or 1, frames, nlive and spp are at least 1, entries and out hold n");
    return RT_E_INVALID;
  }
  // (a launch holds fewer than 2^31 entries, so its divisors and entries are below that)
  bool small = ((frames | nlive | spp) >> 31) == 0;
  for (size_t j = 0; j < n && small; ++j) small = (entries[j] >> 31) == 0;
  if (!small) {
    set_error("stream decode: frames, nlive, spp and every entry are below 2^31");
    return RT_E_INVALID;
  }
  const StreamDecode k = stream_decode_of(order, frames, nlive, spp);  // (as render_stream fills StreamParams::dec)
  for (size_t j = 0; j < n; ++j) {
    const StreamEntry en = stream_decode(k, order, entries[j]);
    out[3 * j] = en.fl;
    out[3 * j + 1] = en.i;
    out[3 * j + 2] = en.s;
  }
  return RT_OK;
}

static_assert(kSoftUndecided == RT_SOFT_UNDECIDED && kSoftMiss == RT_SOFT_MISS && kSoftHit == RT_SOFT_HIT, "rt_api.h");
int rt_soft_screen(const double* centers, const double* r2, const double* origins, const double* dirs, const double* il,
                   const double* tmin, const double* tmax, size_t n, int32_t* out) {
  if (n > 0 && (!centers || !r2 || !origins || !dirs || !il || !tmin || !tmax || !out)) {
    set_error("soft screen: every array holds n cases");
    return RT_E_INVALID;
  }
  for (size_t j = 0; j < n; ++j) {
    const double *c = centers + 3 * j, *o = origins + 3 * j, *u = dirs + 3 * j;
    out[j] = soft_screen(c[0], c[1], c[2], r2[j], o[0], o[1], o[2], u[0], u[1], u[2], il[j], tmin[j], tmax[j]);
  }
  return RT_OK;
}

const char* rt_last_error(void) { return g_last_error.c_str(); }

// pinned scene staging made by rt_context_create (grown when a scene needs more)
constexpr size_t kStageDefault = 256 * 1024;
// pinned schedule staging: [0, 256) the counts read back, then the masks and
// costs uploaded (grown when a frame has more tiles)
constexpr size_t kSmallDefault = 64 * 1024;

int rt_context_create(int32_t device, rt_context** out) {
  if (!out) {
    set_error("out is NULL");
    return RT_E_INVALID;
  }
  *out = nullptr;
  int n = 0;
  HIP_TRY(hipGetDeviceCount(&n));
  if (device < 0 || device >= n) {
    set_error("device " + std::to_string(device) + " out of range (" + std::to_string(n) + " devices)");
    return RT_E_DEVICE;
  }
  HIP_TRY(hipSetDevice(device));
  {
    // the kernels' code objects, once per device and process: the
    // constructor's work (NewParallelRenderer), not the first Render's
    static std::mutex mu;
    static std::vector<bool> loaded;
    std::lock_guard<std::mutex> lock(mu);
    if ((int)loaded.size() < n) loaded.resize(n, false);
    if (!loaded[device]) {
      hipError_t e = (hipError_t)preload_render_kernels();
      if (e == hipSuccess) e = (hipError_t)preload_stream_kernels();
      if (e == hipSuccess) e = (hipError_t)preload_image_kernels();
      if (e == hipSuccess) e = (hipError_t)preload_sched_kernels();
      if (e == hipSuccess) e = (hipError_t)preload_wf_kernels();
      if (e == hipSuccess) e = (hipError_t)preload_aov_kernels();
      if (e == hipSuccess) e = (hipError_t)preload_denoise_kernels();
      if (e == hipSuccess) e = (hipError_t)preload_temporal_kernels();
      if (e == hipSuccess) e = (hipError_t)preload_variance_kernels();
      if (e == hipSuccess) e = (hipError_t)preload_motion_kernels();
      if (e == hipSuccess) e = (hipError_t)preload_clip_kernels();
      if (e == hipSuccess) e = (hipError_t)preload_matte_kernels();
      if (e != hipSuccess) {
        set_error(std::string("kernel code object load failed: ") + hipGetErrorString(e));
        return RT_E_DEVICE;
      }
      loaded[device] = true;
    }
  }
  rt_context* c = new rt_context();
  c->device = device;
  rt_tuning_default(&c->tun);
  hipError_t e = (hipError_t)dev_stream_get(&c->stream);
  if (e == hipSuccess) e = (hipError_t)dev_event_get(&c->ev0);
  if (e == hipSuccess) e = (hipError_t)dev_event_get(&c->ev1);
  {
    // the runtime's first-launch / first-copy set-up, once per device and
    // process, on the context's stream (constructor work, as above)
    static std::mutex mu;
    static std::vector<bool> warmed;
    std::lock_guard<std::mutex> lock(mu);
    if ((int)warmed.size() < n) warmed.resize(n, false);
    if (e == hipSuccess && !warmed[device]) {
      constexpr size_t kWarmBytes = size_t(4) << 20;  // a large copy each way (the copy engines)
      void* dbuf = nullptr;
      void* hbuf = nullptr;
      e = (hipError_t)dev_alloc(&dbuf, kWarmBytes);
      if (e == hipSuccess) e = (hipError_t)host_alloc(&hbuf, kWarmBytes);
      std::vector<char> pageable(kWarmBytes);
      if (e == hipSuccess) e = (hipError_t)warm_device(c->stream, dbuf, hbuf, pageable.data(), kWarmBytes);
      host_free(hbuf);
      dev_free(dbuf);
      if (e == hipSuccess) warmed[device] = true;
    }
  }

  // pinned staging of the scene upload (a copy from pageable memory makes the
  // runtime set up its own staging on first use: 9.6 ms of a fresh process's
  // first Render, profiles/r04_cli_trace.json)
  if (e == hipSuccess) {
    e = (hipError_t)host_alloc(&c->h_stage.p, kStageDefault);
    if (e == hipSuccess) c->h_stage.cap = kStageDefault;
  }
  if (e == hipSuccess) {
    e = (hipError_t)host_alloc(&c->h_small.p, kSmallDefault);
    if (e == hipSuccess) c->h_small.cap = kSmallDefault;
  }
  if (e != hipSuccess) {
    set_error(std::string("context init failed: ") + hipGetErrorString(e));
    rt_context_destroy(c);
    return RT_E_DEVICE;
  }
  *out = c;
  return RT_OK;
}

void rt_context_destroy(rt_context* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  // the last render (on the caller's stream) and the context's own stream
  // must be done before the buffers go back to the cache
  if (c->have_timing) (void)hipEventSynchronize(c->ev1);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  for (DevBuf& b : c->d) dev_free(b.p);
  for (DevBuf* b : {&c->h_stage, &c->h_small, &c->h_adapt}) host_free(b->p);
  if (c->wf_host) (void)hipHostFree(c->wf_host);
  for (hipEvent_t& e : c->wf_ev)
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : c->prof_pool) (void)hipEventDestroy(e);
  dev_event_put(c->ev0);  // (complete: ev1 was waited for, ev0 precedes it)
  dev_event_put(c->ev1);
  dev_stream_put(c->stream);  // (idle: synchronized above)
  delete c;
}

int rt_context_set_scene(rt_context* c, const rt_scene* s, int32_t force_bvh) {
  if (!c) {
    set_error("context is NULL");
    return RT_E_INVALID;
  }
  int rc = validate_scene(s);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  c->prog_on = false;  // (a progression ends with its scene)
  flatten_scene(*s, &c->flat);
  c->bvh_seconds = 0;
  // (a sphere with a non-finite centre or radius: no BVH, even when forced; rt_api.h)
  // (a cube is one primitive of the tree, bvh.cpp; kAutoBvhCubes: rt_api.h)
  const bool want_bvh =
      (force_bvh > 0 ||
       (force_bvh == 0 && (c->flat.spheres.size() > 64 || c->flat.boxes.size() > (size_t)kAutoBvhCubes))) &&
      spheres_finite(c->flat);
  if (want_bvh) {
    const auto t0 = std::chrono::steady_clock::now();
    build_bvh(&c->flat, c->tun.bvh_bins, c->tun.bvh_leaf);
    c->bvh_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  }
  const FlatScene& f = c->flat;
  auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
  size_t off_s = 0;
  size_t off_t = off_s + al(f.spheres.size() * sizeof(DSphere));
  size_t off_x = off_t + al(f.tris.size() * sizeof(DTri));
  size_t off_m = off_x + al(f.boxes.size() * sizeof(DBox));
  size_t off_l = off_m + al(f.mats.size() * sizeof(DMat));
  // shadow-cone rows of a scene of spheres alone, right behind the lights so
  // that they are staged with them (the spheres-only stream kernels read them)
  std::vector<unsigned long long> rows;
  if (!f.spheres.empty() && f.tris.empty() && f.boxes.empty() && !f.lights.empty() && cone_masks_apply(f))
    cone_rows(f, &rows);
  size_t off_r = off_l + f.lights.size() * sizeof(DLight);  // (a multiple of 16)
  size_t off_j = off_l + al(f.lights.size() * sizeof(DLight) + rows.size() * sizeof(unsigned long long));
  size_t off_b = off_j + al(kJump * 2 * sizeof(uint64_t));
  size_t off_q = off_b + al(f.bvh.size() * sizeof(DBVHNode));
  size_t off_q4 = off_q + al(f.qbvh.size() * sizeof(DQNode));
  size_t off_sky = off_q4 + al(f.qbvh4.size() * sizeof(DQNode));
  size_t total = off_sky + al(kSkies * sizeof(DSky)) + 256;
  // the last render may still read the scene (a buffer that grows waits in grow)
  rc = total > c->d.scene.cap ? grow(c, &c->d.scene, total, true) : quiesce(c);
  if (rc) return rc;
  char* base = c->d.scene.as<char>();
  rc = grow_pinned(&c->h_stage, total);  // (the last upload was synchronized: the buffer is free)
  if (rc) return rc;
  char* host = c->h_stage.as<char>();
  memset(host, 0, total);
  memcpy(host + off_s, f.spheres.data(), f.spheres.size() * sizeof(DSphere));
  memcpy(host + off_t, f.tris.data(), f.tris.size() * sizeof(DTri));
  memcpy(host + off_x, f.boxes.data(), f.boxes.size() * sizeof(DBox));
  memcpy(host + off_m, f.mats.data(), f.mats.size() * sizeof(DMat));
  memcpy(host + off_l, f.lights.data(), f.lights.size() * sizeof(DLight));
  memcpy(host + off_r, rows.data(), rows.size() * sizeof(unsigned long long));
  {
    uint64_t* jt = reinterpret_cast<uint64_t*>(host + off_j);
    uint64_t a = 1, cc = 0;  // x_{i+j} = A_j x_i + C_j, built incrementally (rt_pcg_jump_coeffs)
    for (int j = 0; j < 3 * kJump; ++j) {
      if (j % 3 == 0) {  // entry h = j / 3: the jump by 3h draws
        jt[2 * (j / 3)] = a;
        jt[2 * (j / 3) + 1] = cc;
      }
      cc = cc * RT_PCG_MULT + RT_PCG_INC;
      a = a * RT_PCG_MULT;
    }
  }
  memcpy(host + off_b, f.bvh.data(), f.bvh.size() * sizeof(DBVHNode));
  memcpy(host + off_q, f.qbvh.data(), f.qbvh.size() * sizeof(DQNode));
  memcpy(host + off_q4, f.qbvh4.data(), f.qbvh4.size() * sizeof(DQNode));
  sky_presets(reinterpret_cast<DSky*>(host + off_sky));
  HIP_TRY(hipMemcpyAsync(base, host, total, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->d_spheres = (const DSphere*)(base + off_s);
  c->d_tris = (const DTri*)(base + off_t);
  c->d_boxes = (const DBox*)(base + off_x);
  c->d_mats = (const DMat*)(base + off_m);
  c->d_lights = (const DLight*)(base + off_l);
  c->d_bvh = (const DBVHNode*)(base + off_b);
  c->d_qbvh = (const DQNode*)(base + off_q);
  c->d_qbvh4 = (const DQNode*)(base + off_q4);
  c->d_jump = (const uint64_t*)(base + off_j);
  c->d_sky = (const DSky*)(base + off_sky);
  // small linear-scan scenes are staged into LDS by every workgroup
  // (the 1 KB PCG jump table stays in global memory, L1-cached: only the
  // cooperative soft-shadow form reads it, and scenes near the LDS limit of 12
  // workgroups per CU ran faster without it)
  // (not with a non-finite sphere: the staged kernels' wide mode splits the
  // closest-hit scan among helper lanes and merges by distance, closest_wide,
  // which equals the sequential scan only while no hit distance is NaN)
  c->stage_bytes = (f.bvh.empty() && off_j <= 48 * 1024 && spheres_finite(f)) ? (int32_t)off_j : 0;
  c->cone_rows_off = (c->stage_bytes > 0 && !rows.empty()) ? (int32_t)off_r : 0;
  c->have_scene = true;
  c->scene_gen += 1;
  return RT_OK;
}

int rt_context_set_partition(rt_context* c, const rt_partition* p) {
  if (!c) {
    set_error("context is NULL");
    return RT_E_INVALID;
  }
  HIP_TRY(hipSetDevice(c->device));
  int rc = quiesce(c);  // the last render may still read the tile lists
  if (rc) return rc;
  c->prog_on = false;  // (a progression's tiles are those of its begin: it ends)
  if (!p) {
    c->part.reset();
    return RT_OK;
  }
  auto d = std::make_shared<const PartitionData>(partition_data(p));
  rc = grow(c, &c->d.part, std::max<size_t>(d->lists.size(), 1) * sizeof(int32_t));
  if (rc) return rc;
  if (!d->lists.empty())
    HIP_TRY(hipMemcpy(c->d.part.p, d->lists.data(), d->lists.size() * sizeof(int32_t), hipMemcpyHostToDevice));
  c->part = std::move(d);
  return RT_OK;
}

int rt_context_profile(rt_context* c, int32_t on) {
  if (!c) {
    set_error("context is NULL");
    return RT_E_INVALID;
  }
  HIP_TRY(hipSetDevice(c->device));
  int rc = prof_collect(c);
  if (rc) return rc;
  c->prof_on = on != 0;
  for (int k = 0; k < kWfClasses; ++k) {
    c->prof_secs[k] = 0;
    c->prof_launches[k] = 0;
  }
  return RT_OK;
}

int rt_context_kernel_seconds(rt_context* c, double* seconds, int64_t* launches) {
  if (!c || !seconds) {
    set_error("context or seconds is NULL");
    return RT_E_INVALID;
  }
  HIP_TRY(hipSetDevice(c->device));
  int rc = prof_collect(c);
  if (rc) return rc;
  for (int k = 0; k < kWfClasses; ++k) {
    seconds[k] = c->prof_secs[k];
    if (launches) launches[k] = c->prof_launches[k];
  }
  return RT_OK;
}

// The tail helpers' control block, once the last render has finished
static int read_tail_ctl(const rt_context* c, TailCtl* h) {
  int rc = quiesce(const_cast<rt_context*>(c));
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpy(h, c->d.tail.p, sizeof *h, hipMemcpyDeviceToHost));
  return RT_OK;
}

int rt_context_get_stats(const rt_context* c, rt_context_stats* out) {
  if (!c || !out) {
    set_error("context or out is NULL");
    return RT_E_INVALID;
  }
  *out = c->stats;
  out->blocks = c->num_blocks;
  out->split_pixels = c->nsplit;
  out->tail_exported = out->tail_errors = 0;
  out->stream_live_pixels = c->nlive;
  if (c->d.tail.p) {
    TailCtl h;
    int rc = read_tail_ctl(c, &h);
    if (rc) return rc;
    out->tail_exported = h.exported;
    out->tail_errors = h.err;
  }
  return RT_OK;
}

int rt_context_tail_debug(const rt_context* c, uint64_t out[6]) {
  if (!c || !out) {
    set_error("context or out is NULL");
    return RT_E_INVALID;
  }
  for (int i = 0; i < 6; ++i) out[i] = 0;
  if (!c->d.tail.p) return RT_OK;
  TailCtl h;
  int rc = read_tail_ctl(c, &h);
  if (rc) return rc;
  out[0] = h.exported;
  out[1] = h.paths_done;
  out[2] = h.solo_ticks;
  out[3] = h.export_ticks;
  out[4] = h.helper_ticks;
  out[5] = h.err;
  return RT_OK;
}

int rt_context_set_debug_buffer(rt_context* c, void* d_buf) {
  if (!c) {
    set_error("context is NULL");
    return RT_E_INVALID;
  }
  c->dbg = (unsigned long long*)d_buf;
  return RT_OK;
}

int rt_context_last_kernel_seconds(rt_context* c, double* seconds) {
  if (!c || !seconds || !c->have_timing) {
    set_error("no timed launch on this context");
    return RT_E_INVALID;
  }
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipEventSynchronize(c->ev1));
  float ms = 0;
  HIP_TRY(hipEventElapsedTime(&ms, c->ev0, c->ev1));
  *seconds = ms * 1e-3;
  return RT_OK;
}

}  // extern "C"
