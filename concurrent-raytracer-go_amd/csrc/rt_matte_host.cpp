// rt_matte_host.cpp — the C ABI of the coverage-aware edge resolve
// (include/rt_api.h): argument checks, the device entry point
// (its kernel is rt_matte.hip's) and rt_matte_resolve_host, which runs the same
// inline function (include/rt_matte.h) over host arrays.  The matte pass
// itself needs a context and is beside the feature passes in rt_render.cpp.
#include <string.h>

#include <string>

#include "../../include/rt_matte.h"
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

// Everything both entry points refuse; the checked parameters of a call that is not refused.
int check_resolve(const char* what, const rt_matte_resolve* params, int32_t w, int32_t h,
                  const rt_matte_resolve_inputs* in, const float* out_linear, const uint8_t* out_rgba,
                  rt_mt_resolve_params* P) {
  const std::string f = what;
  if (!params || !in) return refuse(f + ": params or in is NULL");
  if (!in->color || !in->object || !in->id || !in->count)
    return refuse(f + ": color, object, id and count are required");
  if (!out_linear && !out_rgba) return refuse(f + ": out_linear and out_rgba are both NULL");
  if (out_linear == in->color)
    return refuse(f + ": out_linear must not be color (taps read neighbours: use a second buffer)");
  if (!size_ok(w, h)) return refuse(f + ": invalid image size " + std::to_string(w) + "x" + std::to_string(h));
  if (!rt_mt_resolve_ok(in->ranks, in->samples, params->radius, params->background))
    return refuse(f + ": ranks must be in 1..8, samples >= 1, radius in 1..4 and the background finite");
  P->W = w;
  P->H = h;
  P->K = in->ranks;
  P->n = in->samples;
  P->R = params->radius;
  P->has_rest = in->rest ? 1 : 0;
  for (int k = 0; k < 3; ++k) P->bg[k] = params->background[k];
  return RT_OK;
}

}  // namespace

extern "C" {

void rt_matte_resolve_default(rt_matte_resolve* r) {
  if (!r) return;
  memset(r, 0, sizeof *r);
  r->radius = 2;  // the 5x5 window of the measurements in DESIGN.md §4.19
}

int rt_matte_resolve_async(const rt_matte_resolve* params, int32_t w, int32_t h, const rt_matte_resolve_inputs* in,
                           float* d_out_linear, uint8_t* d_out_rgba, void* stream) {
  MatteResolveParams q;
  const int rc = check_resolve("rt_matte_resolve_async", params, w, h, in, d_out_linear, d_out_rgba, &q.r);
  if (rc) return rc;
  q.color = in->color;
  q.object = in->object;
  q.id = in->id;
  q.count = in->count;
  q.rest = in->rest;
  q.out_linear = d_out_linear;
  q.out_rgba = d_out_rgba;
  const int e = launch_matte_resolve(q, stream);
  return e == hipSuccess ? (int)RT_OK : launch_failed("matte_resolve", e);
}

int rt_matte_resolve_host(const rt_matte_resolve* params, int32_t w, int32_t h, const rt_matte_resolve_inputs* in,
                          float* out_linear, uint8_t* out_rgba) {
  rt_mt_resolve_params P;
  const int rc = check_resolve("rt_matte_resolve_host", params, w, h, in, out_linear, out_rgba, &P);
  if (rc) return rc;
  for (int32_t y = 0; y < h; ++y)
    for (int32_t x = 0; x < w; ++x) {
      const size_t p = (size_t)y * (size_t)w + (size_t)x;
      float out[3];
      if (!rt_mt_resolve_pixel(&P, in->color, in->object, in->id, in->count, in->rest, x, y, out))
        memcpy(out, in->color + p * 3, sizeof out);
      if (out_linear) memcpy(out_linear + p * 3, out, sizeof out);
      if (out_rgba) rt_tonemap_rgba(out, 1, out_rgba + p * 4);
    }
  return RT_OK;
}

}  // extern "C"
