// rt_denoise_host.cpp — the C ABI of the à-trous denoiser (include/rt_api.h,
// DESIGN.md §4.13): argument checks, the device entry point (its kernels are
// rt_denoise.hip) and rt_denoise_host, which runs the same inline functions
// (include/rt_denoise.h) over host arrays in the same passes as the kernels.
#include <math.h>

#include <string>
#include <vector>

#include "../../include/rt_denoise.h"
#include "rt_context.h"
#include "rt_internal.h"

using namespace rtgo;

namespace {

// the size rule of rt_validate (rt_api.cpp validate_settings)
bool size_ok(int32_t w, int32_t h) {
  return w > 0 && h > 0 && w <= 65536 && h <= 65536 && (long long)w * h <= (1LL << 31) / 4;
}

bool params_ok(const rt_denoise* d) {
  if (d->levels < 1 || d->levels > 8) return false;
  const int32_t np = d->normal_power;
  if (np < 0 || np > 128 || (np & (np - 1)) != 0) return false;  // (0 passes: off)
  if (!isfinite(d->sigma_color) || d->sigma_color < 0) return false;
  if (!isfinite(d->sigma_depth) || d->sigma_depth < 0) return false;
  return d->demodulate == 0 || d->demodulate == 1;
}

// Everything both entry points refuse; `what` names the caller in the message.
int check_call(const char* what, const rt_denoise* d, int32_t w, int32_t h, const rt_denoise_inputs* in,
               const void* out_linear, const void* out_rgba) {
  const std::string f = what;
  if (!d || !in) {
    set_error(f + ": params or inputs is NULL");
    return RT_E_INVALID;
  }
  if (!in->color || !in->normal || !in->depth) {
    set_error(f + ": color, normal and depth are required");
    return RT_E_INVALID;
  }
  if (!out_linear && !out_rgba) {
    set_error(f + ": both outputs are NULL");
    return RT_E_INVALID;
  }
  if (!size_ok(w, h)) {
    set_error(f + ": invalid image size " + std::to_string(w) + "x" + std::to_string(h));
    return RT_E_INVALID;
  }
  if (!params_ok(d)) {
    set_error(f + ": levels must be in 1..8, normal_power 0 or a power of two <= 128, sigma_color and sigma_depth "
                  "finite and >= 0, demodulate 0 or 1");
    return RT_E_INVALID;
  }
  return RT_OK;
}

}  // namespace

extern "C" {

void rt_denoise_default(rt_denoise* d) {
  if (!d) return;
  d->levels = 4;
  d->normal_power = 32;
  d->sigma_color = 0.5;
  d->sigma_depth = 0.05;
  d->demodulate = 1;
  d->_pad = 0;
}

size_t rt_denoise_workspace_bytes(int32_t w, int32_t h) {
  if (!size_ok(w, h)) return 0;
  return kDenoiseRecordBytes * (size_t)w * (size_t)h + kDenoiseAlign;
}

int rt_denoise_async(const rt_denoise* d, int32_t w, int32_t h, const rt_denoise_inputs* in, float* d_out_linear,
                     uint8_t* d_out_rgba, void* d_workspace, size_t workspace_bytes, void* stream) {
  const int rc = check_call("rt_denoise_async", d, w, h, in, d_out_linear, d_out_rgba);
  if (rc) return rc;
  if (!d_workspace || workspace_bytes < rt_denoise_workspace_bytes(w, h)) {
    set_error("rt_denoise_async: the workspace is NULL or smaller than rt_denoise_workspace_bytes (" +
              std::to_string(rt_denoise_workspace_bytes(w, h)) + " bytes)");
    return RT_E_INVALID;
  }
  DenoiseParams p;
  p.dn = *d;
  p.W = w;
  p.H = h;
  p.color = in->color;
  p.normal = in->normal;
  p.depth = in->depth;
  p.albedo = in->albedo;
  p.object = in->object;
  p.out_linear = d_out_linear;
  p.out_rgba = d_out_rgba;
  p.workspace = d_workspace;
  const int e = launch_denoise(p, stream);
  return e == hipSuccess ? (int)RT_OK : launch_failed("denoise", e);
}

int rt_denoise_host(const rt_denoise* d, int32_t w, int32_t h, const rt_denoise_inputs* in, float* out_linear,
                    uint8_t* out_rgba) {
  const int rc = check_call("rt_denoise_host", d, w, h, in, out_linear, out_rgba);
  if (rc) return rc;
  const size_t npix = (size_t)w * (size_t)h;
  const float* albedo = d->demodulate ? in->albedo : nullptr;
  // the kernels' passes: prepare, then levels that ping-pong between two colour buffers
  std::vector<rt_dn_color> e[2] = {std::vector<rt_dn_color>(npix), std::vector<rt_dn_color>(d->levels > 1 ? npix : 0)};
  std::vector<rt_dn_guide> g(npix);
  for (size_t p = 0; p < npix; ++p) rt_dn_prepare(in->color, albedo, in->normal, in->depth, in->object, p, &e[0][p], &g[p]);
  for (int32_t i = 0; i < d->levels; ++i) {
    const rt_dn_level L = rt_dn_level_of(w, h, i, d->normal_power, d->sigma_color, d->sigma_depth);
    const rt_dn_color* src = e[i & 1].data();
    const bool last = i + 1 == d->levels;
    rt_dn_color* dst = last ? nullptr : e[(i & 1) ^ 1].data();
    for (int32_t y = 0; y < h; ++y)
      for (int32_t x = 0; x < w; ++x) {
        const size_t p = (size_t)y * (size_t)w + (size_t)x;
        const rt_dn_color o = rt_dn_level_pixel(&L, src, g.data(), x, y);
        if (!last) {
          dst[p] = o;
          continue;
        }
        float out[3];
        rt_dn_finish(&o, rt_dn_valid(g[p].z), in->color, albedo, p, out);
        if (out_linear) {
          out_linear[p * 3 + 0] = out[0];
          out_linear[p * 3 + 1] = out[1];
          out_linear[p * 3 + 2] = out[2];
        }
        if (out_rgba) rt_tonemap_rgba(out, 1, out_rgba + p * 4);
      }
  }
  return RT_OK;
}

}  // extern "C"
