// rt_clip_host.cpp — the C ABI of temporal accumulation with history
// rectification (include/rt_api.h): argument checks, the
// device entry point (its kernels are rt_clip.hip) and rt_temporal_clip_host,
// which runs the same inline functions (include/rt_clip.h) over host arrays.
#include <math.h>

#include <string>

#include "../../include/rt_clip.h"
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

// Everything both entry points refuse: the rules of the call this extends (rt_temporal_motion_async with a table,
// rt_temporal_async / rt_temporal_moments_async without; cur_albedo alone is allowed, it feeds the window), and
// the clip's own.  The constants and the checked parameters of a call that is not refused; `what` names the caller.
int check_clip(const char* what, const rt_temporal* tp, int32_t w, int32_t h, const rt_temporal_frame* cur,
               const rt_temporal_frame* prev, const rt_motion* motion, const rt_history_clip* clip,
               const float* prev_moments, const float* out_color, const float* out_count, const float* out_moments,
               const float* out_clipped, rt_tp_constants* C, rt_cl_params* K) {
  const std::string f = what;
  if (!tp || !cur) return refuse(f + ": params or the current frame is NULL");
  if (!clip) return refuse(f + ": clip is NULL");
  if (motion && !motion->motion) return refuse(f + ": motion's table is NULL");
  if (motion && motion->num_objects < 1) return refuse(f + ": motion.num_objects must be >= 1");
  if (!cur->color || !cur->depth || (prev && (!prev->color || !prev->depth || !prev->count)))
    return refuse(f + ": color and depth are required in both frames, count in the previous one");
  if (motion && (!cur->object || (prev && !prev->object)))
    return refuse(f + ": object is required in both frames (the motion table is indexed by it)");
  if (prev && ((cur->object == nullptr) != (prev->object == nullptr) || (cur->normal == nullptr) != (prev->normal == nullptr)))
    return refuse(f + ": object and normal must each be NULL in both frames or in neither");
  if (!out_color || !out_count) return refuse(f + ": out_color and out_count are required");
  if (!out_moments && prev_moments) return refuse(f + ": prev_moments must be NULL when out_moments is");
  if (out_moments && (prev != nullptr) != (prev_moments != nullptr))
    return refuse(f + ": prev_moments is required exactly when prev is given");
  if (prev && (out_color == prev->color || out_count == prev->count || (out_moments && out_moments == prev_moments)))
    return refuse(f + ": out_color / out_count / out_moments must not be the previous frame's color / count / "
                      "moments (taps read neighbours: ping-pong two buffers)");
  if (out_clipped && (out_clipped == out_color || out_clipped == out_count || out_clipped == out_moments))
    return refuse(f + ": out_clipped must not be another output");
  if (!size_ok(w, h)) return refuse(f + ": invalid image size " + std::to_string(w) + "x" + std::to_string(h));
  if (!rt_tp_params_ok(tp->max_history, tp->depth_tol, tp->normal_min, tp->min_weight))
    return refuse(f + ": max_history must be finite and >= 1, depth_tol finite and >= 0, normal_min in [-1, 1], "
                      "min_weight in (0, 1]");
  if (!rt_cl_params_ok(clip->radius, clip->min_taps, clip->gamma, clip->min_half))
    return refuse(f + ": clip.radius must be in 0..4, min_taps >= 1, gamma and min_half finite and >= 0");
  if (!rt_tp_constants_of(C, w, h, tp->max_history, tp->depth_tol, tp->normal_min, tp->min_weight, cur->frame,
                          prev ? prev->frame : nullptr))
    return refuse(f + ": a camera frame is not finite, or the previous frame's view axis, horizontal or vertical is zero");
  K->radius = clip->radius;
  K->min_taps = clip->min_taps;
  K->gamma = clip->gamma;
  K->min_half = clip->min_half;
  return RT_OK;
}

}  // namespace

extern "C" {

// DESIGN.md §4.18 has the grid these come from.
void rt_history_clip_default(rt_history_clip* c) {
  if (!c) return;
  c->radius = 1;
  c->min_taps = 5;
  c->gamma = 1.0;
  c->min_half = 0;
}

int rt_temporal_clip_async(const rt_temporal* tp, int32_t w, int32_t h, const rt_temporal_frame* cur,
                           const rt_temporal_frame* prev, const rt_motion* motion, const rt_history_clip* clip,
                           const float* d_cur_albedo, const float* d_prev_moments, float* d_out_color,
                           float* d_out_count, float* d_out_moments, float* d_out_clipped, uint8_t* d_out_rgba,
                           void* stream) {
  TemporalClipParams p;
  const int rc = check_clip("rt_temporal_clip_async", tp, w, h, cur, prev, motion, clip, d_prev_moments, d_out_color,
                            d_out_count, d_out_moments, d_out_clipped, &p.mo.m.t.c, &p.clip);
  if (rc) return rc;
  p.mo.m.t.cur = buffers_of(cur);
  p.mo.m.t.prev = buffers_of(prev);
  p.mo.m.t.out_color = d_out_color;
  p.mo.m.t.out_count = d_out_count;
  p.mo.m.t.out_rgba = d_out_rgba;
  p.mo.m.cur_albedo = d_cur_albedo;
  p.mo.m.prev_moments = d_prev_moments;
  p.mo.m.out_moments = d_out_moments;
  p.mo.motion = motion ? motion->motion : nullptr;
  p.mo.num_objects = motion ? motion->num_objects : 0;
  p.out_clipped = d_out_clipped;
  const int e = launch_temporal_clip(p, stream);
  return e == hipSuccess ? (int)RT_OK : launch_failed("temporal_clip", e);
}

int rt_temporal_clip_host(const rt_temporal* tp, int32_t w, int32_t h, const rt_temporal_frame* cur,
                          const rt_temporal_frame* prev, const rt_motion* motion, const rt_history_clip* clip,
                          const float* cur_albedo, const float* prev_moments, float* out_color, float* out_count,
                          float* out_moments, float* out_clipped, uint8_t* out_rgba) {
  rt_tp_constants C;
  rt_cl_params K;
  const int rc = check_clip("rt_temporal_clip_host", tp, w, h, cur, prev, motion, clip, prev_moments, out_color,
                            out_count, out_moments, out_clipped, &C, &K);
  if (rc) return rc;
  const rt_tp_buffers bc = buffers_of(cur), bp = buffers_of(prev);
  const double* table = motion ? motion->motion : nullptr;
  const int32_t rows = motion ? motion->num_objects : 0;
  for (int32_t y = 0; y < h; ++y)
    for (int32_t x = 0; x < w; ++x) {
      const size_t p = (size_t)y * (size_t)w + (size_t)x;
      float out[3], n, m[2], clipped;
      if (out_moments) {
        rt_cl_pixel(1, &C, &K, &bc, &bp, table, rows, cur_albedo, prev_moments, x, y, out, &n, m, &clipped);
        out_moments[p * 2 + 0] = m[0];
        out_moments[p * 2 + 1] = m[1];
      } else {
        rt_cl_pixel(0, &C, &K, &bc, &bp, table, rows, cur_albedo, nullptr, x, y, out, &n, m, &clipped);
      }
      out_color[p * 3 + 0] = out[0];
      out_color[p * 3 + 1] = out[1];
      out_color[p * 3 + 2] = out[2];
      out_count[p] = n;
      if (out_clipped) out_clipped[p] = clipped;
      if (out_rgba) rt_tonemap_rgba(out, 1, out_rgba + p * 4);
    }
  return RT_OK;
}

}  // extern "C"
