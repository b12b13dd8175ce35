// rt_temporal_host.cpp — the C ABI of temporal accumulation (include/rt_api.h,
// DESIGN.md §4.14): argument checks, the per-call constants, the device entry
// point (its kernel is rt_temporal.hip) and rt_temporal_host, which runs the
// same inline function (include/rt_temporal.h) over host arrays.
#include <math.h>

#include <string>

#include "../../include/rt_temporal.h"
#include "rt_context.h"
#include "rt_internal.h"

using namespace rtgo;

namespace {

// the size rule of rt_validate (rt_api.cpp validate_settings)
bool size_ok(int32_t w, int32_t h) {
  return w > 0 && h > 0 && w <= 65536 && h <= 65536 && (long long)w * h <= (1LL << 31) / 4;
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

// Everything both entry points refuse, and the constants of a call that is not; `what` names the caller.
int check_call(const char* what, const rt_temporal* tp, int32_t w, int32_t h, const rt_temporal_frame* cur,
               const rt_temporal_frame* prev, const float* out_color, const float* out_count, rt_tp_constants* C) {
  const std::string f = what;
  if (!tp || !cur) {
    set_error(f + ": params or the current frame is NULL");
    return RT_E_INVALID;
  }
  if (!cur->color || !cur->depth || (prev && (!prev->color || !prev->depth || !prev->count))) {
    set_error(f + ": color and depth are required in both frames, count in the previous one");
    return RT_E_INVALID;
  }
  if (prev && ((cur->object == nullptr) != (prev->object == nullptr) || (cur->normal == nullptr) != (prev->normal == nullptr))) {
    set_error(f + ": object and normal must each be NULL in both frames or in neither");
    return RT_E_INVALID;
  }
  if (!out_color || !out_count) {
    set_error(f + ": out_color and out_count are required");
    return RT_E_INVALID;
  }
  if (prev && (out_color == prev->color || out_count == prev->count)) {
    set_error(f + ": out_color / out_count must not be the previous frame's color / count (taps read neighbours: "
                  "ping-pong two buffers)");
    return RT_E_INVALID;
  }
  if (!size_ok(w, h)) {
    set_error(f + ": invalid image size " + std::to_string(w) + "x" + std::to_string(h));
    return RT_E_INVALID;
  }
  if (!rt_tp_params_ok(tp->max_history, tp->depth_tol, tp->normal_min, tp->min_weight)) {
    set_error(f + ": max_history must be finite and >= 1, depth_tol finite and >= 0, normal_min in [-1, 1], "
                  "min_weight in (0, 1]");
    return RT_E_INVALID;
  }
  if (!rt_tp_constants_of(C, w, h, tp->max_history, tp->depth_tol, tp->normal_min, tp->min_weight, cur->frame,
                          prev ? prev->frame : nullptr)) {
    set_error(f + ": a camera frame is not finite, or the previous frame's view axis, horizontal or vertical is zero");
    return RT_E_INVALID;
  }
  return RT_OK;
}

}  // namespace

extern "C" {

void rt_temporal_default(rt_temporal* t) {
  if (!t) return;
  t->max_history = 32;
  t->depth_tol = 0.05;
  t->normal_min = 0.9;
  t->min_weight = 0.25;
}

int rt_temporal_async(const rt_temporal* tp, int32_t w, int32_t h, const rt_temporal_frame* cur,
                      const rt_temporal_frame* prev, float* d_out_color, float* d_out_count, uint8_t* d_out_rgba,
                      void* stream) {
  TemporalParams p;
  const int rc = check_call("rt_temporal_async", tp, w, h, cur, prev, d_out_color, d_out_count, &p.c);
  if (rc) return rc;
  p.cur = buffers_of(cur);
  p.prev = buffers_of(prev);
  p.out_color = d_out_color;
  p.out_count = d_out_count;
  p.out_rgba = d_out_rgba;
  const int e = launch_temporal(p, stream);
  return e == hipSuccess ? (int)RT_OK : launch_failed("temporal", e);
}

int rt_temporal_host(const rt_temporal* tp, int32_t w, int32_t h, const rt_temporal_frame* cur,
                     const rt_temporal_frame* prev, float* out_color, float* out_count, uint8_t* out_rgba) {
  rt_tp_constants C;
  const int rc = check_call("rt_temporal_host", tp, w, h, cur, prev, out_color, out_count, &C);
  if (rc) return rc;
  const rt_tp_buffers bc = buffers_of(cur), bp = buffers_of(prev);
  for (int32_t y = 0; y < h; ++y)
    for (int32_t x = 0; x < w; ++x) {
      const size_t p = (size_t)y * (size_t)w + (size_t)x;
      float out[3], n;
      rt_tp_pixel(&C, &bc, &bp, x, y, out, &n);
      out_color[p * 3 + 0] = out[0];
      out_color[p * 3 + 1] = out[1];
      out_color[p * 3 + 2] = out[2];
      out_count[p] = n;
      if (out_rgba) rt_tonemap_rgba(out, 1, out_rgba + p * 4);
    }
  return RT_OK;
}

}  // extern "C"
