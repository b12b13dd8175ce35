// rt_variance_host.cpp — the C ABI of variance-guided denoising (include/rt_api.h,
// DESIGN.md §4.15): argument checks, the device entry points (their kernels are
// rt_variance.hip) and the _host twins, which run the same inline functions
// (include/rt_variance.h) over host arrays in the same passes as the kernels.
#include <math.h>

#include <string>
#include <vector>

#include "../../include/rt_variance.h"
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

// Everything both moments entry points refuse (rt_temporal_async's rules and the moments' own), and the
// constants of a call that is not; `what` names the caller.
int check_moments(const char* what, const rt_temporal* tp, int32_t w, int32_t h, const rt_temporal_frame* cur,
                  const rt_temporal_frame* prev, const float* prev_moments, const float* out_color,
                  const float* out_count, const float* out_moments, rt_tp_constants* C) {
  const std::string f = what;
  if (!tp || !cur) return refuse(f + ": params or the current frame is NULL");
  if (!cur->color || !cur->depth || (prev && (!prev->color || !prev->depth || !prev->count)))
    return refuse(f + ": color and depth are required in both frames, count in the previous one");
  if (prev && ((cur->object == nullptr) != (prev->object == nullptr) || (cur->normal == nullptr) != (prev->normal == nullptr)))
    return refuse(f + ": object and normal must each be NULL in both frames or in neither");
  if ((prev != nullptr) != (prev_moments != nullptr))
    return refuse(f + ": prev_moments is required exactly when prev is given");
  if (!out_color || !out_count || !out_moments) return refuse(f + ": out_color, out_count and out_moments are required");
  if (prev && (out_color == prev->color || out_count == prev->count || out_moments == prev_moments))
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

int check_variance(const char* what, const rt_variance* v, int32_t w, int32_t h, const rt_variance_inputs* in,
                   const float* out_var) {
  const std::string f = what;
  if (!v || !in) return refuse(f + ": params or inputs is NULL");
  if (!in->color || !in->normal || !in->depth) return refuse(f + ": color, normal and depth are required");
  if ((in->moments == nullptr) != (in->count == nullptr))
    return refuse(f + ": moments and count are given both or neither");
  if (!out_var) return refuse(f + ": out_var is NULL");
  if (!size_ok(w, h)) return refuse(f + ": invalid image size " + std::to_string(w) + "x" + std::to_string(h));
  if (!rt_vr_params_ok(v->min_history, v->normal_power, v->sigma_depth))
    return refuse(f + ": min_history must be finite and >= 1, normal_power 0 or a power of two <= 128, sigma_depth "
                      "finite and >= 0");
  return RT_OK;
}

rt_vr_buffers variance_buffers(const rt_variance_inputs* in) {
  rt_vr_buffers b;
  b.color = in->color;
  b.normal = in->normal;
  b.depth = in->depth;
  b.albedo = in->albedo;
  b.object = in->object;
  b.moments = in->moments;
  b.count = in->count;
  return b;
}

int check_filter(const char* what, const rt_denoise_var* d, int32_t w, int32_t h, const rt_denoise_inputs* in,
                 const float* variance, const void* out_linear, const void* out_rgba) {
  const std::string f = what;
  if (!d || !in) return refuse(f + ": params or inputs is NULL");
  if (!in->color || !in->normal || !in->depth || !variance)
    return refuse(f + ": color, normal, depth and variance are required");
  if (!out_linear && !out_rgba) return refuse(f + ": out_linear and out_rgba are both NULL");
  if (!size_ok(w, h)) return refuse(f + ": invalid image size " + std::to_string(w) + "x" + std::to_string(h));
  if (!rt_vr_filter_params_ok(d->levels, d->normal_power, d->sigma_lum, d->sigma_depth, d->demodulate, d->prefilter))
    return refuse(f + ": levels must be in 1..8, normal_power 0 or a power of two <= 128, sigma_lum and sigma_depth "
                      "finite and >= 0, demodulate and prefilter 0 or 1");
  return RT_OK;
}

}  // namespace

extern "C" {

int rt_temporal_moments_async(const rt_temporal* tp, int32_t w, int32_t h, const rt_temporal_frame* cur,
                              const rt_temporal_frame* prev, const float* d_cur_albedo, const float* d_prev_moments,
                              float* d_out_color, float* d_out_count, float* d_out_moments, uint8_t* d_out_rgba,
                              void* stream) {
  TemporalMomentsParams p;
  const int rc = check_moments("rt_temporal_moments_async", tp, w, h, cur, prev, d_prev_moments, d_out_color,
                               d_out_count, d_out_moments, &p.t.c);
  if (rc) return rc;
  p.t.cur = buffers_of(cur);
  p.t.prev = buffers_of(prev);
  p.t.out_color = d_out_color;
  p.t.out_count = d_out_count;
  p.t.out_rgba = d_out_rgba;
  p.cur_albedo = d_cur_albedo;
  p.prev_moments = d_prev_moments;
  p.out_moments = d_out_moments;
  const int e = launch_temporal_moments(p, stream);
  return e == hipSuccess ? (int)RT_OK : launch_failed("temporal_moments", e);
}

int rt_temporal_moments_host(const rt_temporal* tp, int32_t w, int32_t h, const rt_temporal_frame* cur,
                             const rt_temporal_frame* prev, const float* cur_albedo, const float* prev_moments,
                             float* out_color, float* out_count, float* out_moments, uint8_t* out_rgba) {
  rt_tp_constants C;
  const int rc = check_moments("rt_temporal_moments_host", tp, w, h, cur, prev, prev_moments, out_color, out_count,
                               out_moments, &C);
  if (rc) return rc;
  const rt_tp_buffers bc = buffers_of(cur), bp = buffers_of(prev);
  for (int32_t y = 0; y < h; ++y)
    for (int32_t x = 0; x < w; ++x) {
      const size_t p = (size_t)y * (size_t)w + (size_t)x;
      float out[3], n, m[2];
      rt_vr_tp_pixel(&C, &bc, &bp, cur_albedo, prev_moments, x, y, out, &n, m);
      out_color[p * 3 + 0] = out[0];
      out_color[p * 3 + 1] = out[1];
      out_color[p * 3 + 2] = out[2];
      out_count[p] = n;
      out_moments[p * 2 + 0] = m[0];
      out_moments[p * 2 + 1] = m[1];
      if (out_rgba) rt_tonemap_rgba(out, 1, out_rgba + p * 4);
    }
  return RT_OK;
}

void rt_variance_default(rt_variance* v) {
  if (!v) return;
  v->min_history = 4;
  v->sigma_depth = 0.05;
  v->normal_power = 32;
  v->_pad = 0;
}

int rt_variance_async(const rt_variance* v, int32_t w, int32_t h, const rt_variance_inputs* in, float* d_out_var,
                      void* stream) {
  const int rc = check_variance("rt_variance_async", v, w, h, in, d_out_var);
  if (rc) return rc;
  VarianceParams p;
  p.vr = *v;
  p.W = w;
  p.H = h;
  p.in = variance_buffers(in);
  p.out_var = d_out_var;
  const int e = launch_variance(p, stream);
  return e == hipSuccess ? (int)RT_OK : launch_failed("variance", e);
}

int rt_variance_host(const rt_variance* v, int32_t w, int32_t h, const rt_variance_inputs* in, float* out_var) {
  const int rc = check_variance("rt_variance_host", v, w, h, in, out_var);
  if (rc) return rc;
  const rt_dn_level L = rt_dn_level_of(w, h, 0, v->normal_power, 0.0, v->sigma_depth);
  const rt_vr_buffers b = variance_buffers(in);
  for (int32_t y = 0; y < h; ++y)
    for (int32_t x = 0; x < w; ++x)
      out_var[(size_t)y * (size_t)w + (size_t)x] = rt_vr_variance_pixel(&L, v->min_history, &b, x, y);
  return RT_OK;
}

void rt_denoise_var_default(rt_denoise_var* d) {
  if (!d) return;
  d->levels = 4;
  d->normal_power = 32;
  d->sigma_lum = 2;  // (the sweep over 1, 2, 4, 8)
  d->sigma_depth = 0.05;
  d->demodulate = 1;
  d->prefilter = 1;
}

size_t rt_denoise_var_workspace_bytes(int32_t w, int32_t h) {
  if (!size_ok(w, h)) return 0;
  return kDenoiseVarRecordBytes * (size_t)w * (size_t)h + kDenoiseAlign;
}

int rt_denoise_var_async(const rt_denoise_var* d, int32_t w, int32_t h, const rt_denoise_inputs* in,
                         const float* d_variance, float* d_out_linear, uint8_t* d_out_rgba, float* d_out_variance,
                         void* d_workspace, size_t workspace_bytes, void* stream) {
  const int rc = check_filter("rt_denoise_var_async", d, w, h, in, d_variance, d_out_linear, d_out_rgba);
  if (rc) return rc;
  if (!d_workspace || workspace_bytes < rt_denoise_var_workspace_bytes(w, h))
    return refuse("rt_denoise_var_async: the workspace is NULL or smaller than rt_denoise_var_workspace_bytes (" +
                  std::to_string(rt_denoise_var_workspace_bytes(w, h)) + " bytes)");
  DenoiseVarParams p;
  p.dn = *d;
  p.W = w;
  p.H = h;
  p.color = in->color;
  p.normal = in->normal;
  p.depth = in->depth;
  p.albedo = in->albedo;
  p.object = in->object;
  p.variance = d_variance;
  p.out_linear = d_out_linear;
  p.out_rgba = d_out_rgba;
  p.out_variance = d_out_variance;
  p.workspace = d_workspace;
  const int e = launch_denoise_var(p, stream);
  return e == hipSuccess ? (int)RT_OK : launch_failed("denoise_var", e);
}

int rt_denoise_var_host(const rt_denoise_var* d, int32_t w, int32_t h, const rt_denoise_inputs* in,
                        const float* variance, float* out_linear, uint8_t* out_rgba, float* out_variance) {
  const int rc = check_filter("rt_denoise_var_host", d, w, h, in, variance, out_linear, out_rgba);
  if (rc) return rc;
  const size_t npix = (size_t)w * (size_t)h;
  const float* albedo = d->demodulate ? in->albedo : nullptr;
  // the kernels' passes: prepare, then levels that ping-pong between two colour buffers
  std::vector<rt_vr_color> e[2] = {std::vector<rt_vr_color>(npix), std::vector<rt_vr_color>(d->levels > 1 ? npix : 0)};
  std::vector<rt_dn_guide> g(npix);
  std::vector<int32_t> id(npix);
  for (size_t p = 0; p < npix; ++p)
    rt_vr_prepare(in->color, albedo, in->normal, in->depth, in->object, variance, p, &e[0][p], &g[p], &id[p]);
  for (int32_t i = 0; i < d->levels; ++i) {
    const rt_vr_level L = rt_vr_level_of(w, h, i, d->normal_power, d->sigma_lum, d->sigma_depth, d->prefilter);
    const rt_vr_color* src = e[i & 1].data();
    const bool last = i + 1 == d->levels;
    rt_vr_color* dst = last ? nullptr : e[(i & 1) ^ 1].data();
    for (int32_t y = 0; y < h; ++y)
      for (int32_t x = 0; x < w; ++x) {
        const size_t p = (size_t)y * (size_t)w + (size_t)x;
        const rt_vr_color o = rt_vr_level_pixel(&L, src, g.data(), id.data(), x, y);
        if (!last) {
          dst[p] = o;
          continue;
        }
        float out[3];
        rt_vr_finish(&o, rt_dn_valid(g[p].z), in->color, albedo, p, out);
        if (out_linear) {
          out_linear[p * 3 + 0] = out[0];
          out_linear[p * 3 + 1] = out[1];
          out_linear[p * 3 + 2] = out[2];
        }
        if (out_rgba) rt_tonemap_rgba(out, 1, out_rgba + p * 4);
        if (out_variance) out_variance[p] = o.var;
      }
  }
  return RT_OK;
}

}  // extern "C"
