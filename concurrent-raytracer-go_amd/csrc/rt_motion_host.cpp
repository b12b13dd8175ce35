// rt_motion_host.cpp — the C ABI of temporal accumulation with per-object motion
// (include/rt_api.h): argument checks, the device entry point
// (its kernels are rt_motion.hip), rt_temporal_motion_host, which runs the same
// inline function (include/rt_motion.h) over host arrays, and rt_scene_motion,
// which makes the table from two scenes.
#include <math.h>
#include <string.h>

#include <string>

#include "../../include/rt_motion.h"
#include "rt_context.h"
#include "rt_internal.h"

using namespace rtgo;

namespace {

// the size rule of rt_validate (rt_api.cpp validate_settings)
bool size_ok(int32_t w, int32_t h) {
  return w > 0 && h > 0 && w <= 65536 && h <= 65536 && (long long)w * h <= (1LL << 31) / 4;
}

int refuse(const std::string& msg) {
  set_error(msg);
  return RT_E_INVALID;
}

rt_tp_buffers buffers_of(const rt_temporal_frame* f) {
  rt_tp_buffers b;
  b.color = f ? f->color : nullptr;
  b.depth = f ? f->depth : nullptr;
  b.object = f ? f->object : nullptr;
  b.normal = f ? f->normal : nullptr;
  b.count = f ? f->count : nullptr;
  return b;
}

// Everything both entry points refuse (rt_temporal_async's rules, rt_temporal_moments_async's when out_moments is
// given, and the table's own), and the constants of a call that is not; `what` names the caller.
int check_motion(const char* what, const rt_temporal* tp, int32_t w, int32_t h, const rt_temporal_frame* cur,
                 const rt_temporal_frame* prev, const rt_motion* motion, const float* cur_albedo,
                 const float* prev_moments, const float* out_color, const float* out_count, const float* out_moments,
                 rt_tp_constants* C) {
  const std::string f = what;
  if (!tp || !cur) return refuse(f + ": params or the current frame is NULL");
  if (!motion || !motion->motion) return refuse(f + ": motion or its table is NULL");
  if (motion->num_objects < 1) return refuse(f + ": motion.num_objects must be >= 1");
  if (!cur->color || !cur->depth || (prev && (!prev->color || !prev->depth || !prev->count)))
    return refuse(f + ": color and depth are required in both frames, count in the previous one");
  if (!cur->object || (prev && !prev->object))
    return refuse(f + ": object is required in both frames (the motion table is indexed by it)");
  if (prev && (cur->normal == nullptr) != (prev->normal == nullptr))
    return refuse(f + ": normal must be NULL in both frames or in neither");
  if (!out_color || !out_count) return refuse(f + ": out_color and out_count are required");
  if (!out_moments && (cur_albedo || prev_moments))
    return refuse(f + ": cur_albedo and prev_moments must be NULL when out_moments is (the colour-only form)");
  if (out_moments && (prev != nullptr) != (prev_moments != nullptr))
    return refuse(f + ": prev_moments is required exactly when prev is given");
  if (prev && (out_color == prev->color || out_count == prev->count || (out_moments && out_moments == prev_moments)))
    return refuse(f + ": out_color / out_count / out_moments must not be the previous frame's color / count / "
                      "moments (taps read neighbours: ping-pong two buffers)");
  if (!size_ok(w, h)) return refuse(f + ": invalid image size " + std::to_string(w) + "x" + std::to_string(h));
  if (!rt_tp_params_ok(tp->max_history, tp->depth_tol, tp->normal_min, tp->min_weight))
    return refuse(f + ": max_history must be finite and >= 1, depth_tol finite and >= 0, normal_min in [-1, 1], "
                      "min_weight in (0, 1]");
  if (!rt_tp_constants_of(C, w, h, tp->max_history, tp->depth_tol, tp->normal_min, tp->min_weight, cur->frame,
                          prev ? prev->frame : nullptr))
    return refuse(f + ": a camera frame is not finite, or the previous frame's view axis, horizontal or vertical is zero");
  return RT_OK;
}

bool same_doubles(const double* a, const double* b, int n) { return memcmp(a, b, sizeof(double) * (size_t)n) == 0; }

// everything of an object but its position
bool same_shape(const rt_object& a, const rt_object& b) {
  const rt_material &ma = a.material, &mb = b.material;
  return a.type == b.type && same_doubles(a.size, b.size, 3) && same_doubles(&a.radius, &b.radius, 1) &&
         ma.kind == mb.kind && same_doubles(ma.color, mb.color, 3) && same_doubles(&ma.roughness, &mb.roughness, 1) &&
         same_doubles(&ma.metallic, &mb.metallic, 1) && same_doubles(&ma.specular, &mb.specular, 1) &&
         same_doubles(&ma.refraction_index, &mb.refraction_index, 1);
}

}  // namespace

extern "C" {

int rt_temporal_motion_async(const rt_temporal* tp, int32_t w, int32_t h, const rt_temporal_frame* cur,
                             const rt_temporal_frame* prev, const rt_motion* motion, const float* d_cur_albedo,
                             const float* d_prev_moments, float* d_out_color, float* d_out_count, float* d_out_moments,
                             uint8_t* d_out_rgba, void* stream) {
  TemporalMotionParams p;
  const int rc = check_motion("rt_temporal_motion_async", tp, w, h, cur, prev, motion, d_cur_albedo, d_prev_moments,
                              d_out_color, d_out_count, d_out_moments, &p.m.t.c);
  if (rc) return rc;
  p.m.t.cur = buffers_of(cur);
  p.m.t.prev = buffers_of(prev);
  p.m.t.out_color = d_out_color;
  p.m.t.out_count = d_out_count;
  p.m.t.out_rgba = d_out_rgba;
  p.m.cur_albedo = d_cur_albedo;
  p.m.prev_moments = d_prev_moments;
  p.m.out_moments = d_out_moments;
  p.motion = motion->motion;
  p.num_objects = motion->num_objects;
  const int e = launch_temporal_motion(p, stream);
  return e == hipSuccess ? (int)RT_OK : launch_failed("temporal_motion", e);
}

int rt_temporal_motion_host(const rt_temporal* tp, int32_t w, int32_t h, const rt_temporal_frame* cur,
                            const rt_temporal_frame* prev, const rt_motion* motion, const float* cur_albedo,
                            const float* prev_moments, float* out_color, float* out_count, float* out_moments,
                            uint8_t* out_rgba) {
  rt_tp_constants C;
  const int rc = check_motion("rt_temporal_motion_host", tp, w, h, cur, prev, motion, cur_albedo, prev_moments,
                              out_color, out_count, out_moments, &C);
  if (rc) return rc;
  const rt_tp_buffers bc = buffers_of(cur), bp = buffers_of(prev);
  for (int32_t y = 0; y < h; ++y)
    for (int32_t x = 0; x < w; ++x) {
      const size_t p = (size_t)y * (size_t)w + (size_t)x;
      float out[3], n, m[2];
      if (out_moments) {
        rt_mo_pixel(1, &C, &bc, &bp, motion->motion, motion->num_objects, cur_albedo, prev_moments, x, y, out, &n, m);
        out_moments[p * 2 + 0] = m[0];
        out_moments[p * 2 + 1] = m[1];
      } else {
        rt_mo_pixel(0, &C, &bc, &bp, motion->motion, motion->num_objects, nullptr, nullptr, x, y, out, &n, m);
      }
      out_color[p * 3 + 0] = out[0];
      out_color[p * 3 + 1] = out[1];
      out_color[p * 3 + 2] = out[2];
      out_count[p] = n;
      if (out_rgba) rt_tonemap_rgba(out, 1, out_rgba + p * 4);
    }
  return RT_OK;
}

int rt_scene_motion(const rt_scene* prev, const rt_scene* cur, double* out, size_t capacity) {
  const std::string f = "rt_scene_motion";
  if (!prev || !cur || !out) return refuse(f + ": a scene or out is NULL");
  if (prev->num_objects != cur->num_objects)
    return refuse(f + ": the scenes have " + std::to_string(prev->num_objects) + " and " +
                  std::to_string(cur->num_objects) + " objects");
  const int32_t n = cur->num_objects;
  if (n < 0 || (n > 0 && (!prev->objects || !cur->objects))) return refuse(f + ": a scene's objects are NULL");
  if (capacity < (size_t)n * 3)
    return refuse(f + ": out holds " + std::to_string(capacity) + " doubles, " + std::to_string((size_t)n * 3) +
                  " are needed");
  for (int32_t k = 0; k < n; ++k) {
    const rt_object &a = prev->objects[k], &b = cur->objects[k];
    if (!same_shape(a, b))
      return refuse(f + ": object " + std::to_string(k) + " differs in type, size, radius or material (a rigid "
                        "translation is the only motion this models)");
    for (int j = 0; j < 3; ++j)
      if (!rt_tp_finite(a.position[j]) || !rt_tp_finite(b.position[j]))
        return refuse(f + ": object " + std::to_string(k) + " has a position that is not finite");
  }
  for (int32_t k = 0; k < n; ++k)
    for (int j = 0; j < 3; ++j) out[(size_t)k * 3 + j] = cur->objects[k].position[j] - prev->objects[k].position[j];
  return n;
}

}  // extern "C"
