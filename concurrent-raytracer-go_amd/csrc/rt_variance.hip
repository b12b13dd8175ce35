// rt_variance.hip — variance-guided denoising: the moments pass, the variance
// pass and the variance-guided à-trous filter (rt_temporal_moments_async,
// rt_variance_async, rt_denoise_var_async, include/rt_api.h).
// A file of its own: no other code object changes.
//
// The arithmetic is include/rt_variance.h, the functions the _host entry points
// run: the kernels only decide which lane handles which pixel.  Everywhere one
// lane per pixel, a wave covers 64 consecutive x of one row (rows are cut at
// the image edge), per-lane sums in tap order: no atomics, no cross-lane
// operation, no LDS.
//   temporal_moments_kernel  rt_temporal.hip's kernel with the two moments
//                            beside the colour: one launch, no workspace.
//   variance_kernel          reads the buffers as the passes before it wrote
//                            them; its 49 taps are contiguous per wave.
//   denoise_var_*            rt_denoise.hip's structure: a prepare kernel packs
//                            {e[3], var} and {n[3], z} into 16-byte records and
//                            the ids into a 4-byte plane; one launch per level
//                            ping-pongs the colour records, the last one writes
//                            the outputs instead.
#include <hip/hip_runtime.h>

#include "../../include/rt_variance.h"
#include "rt_device.h"
#include "rt_internal.h"

namespace rtgo {

// out_color / out_count / out_moments never alias the previous frame's color /
// count / moments (refused by the entry point), which the taps read at
// neighbouring pixels.
__global__ __launch_bounds__(256) void temporal_moments_kernel(const rt_tp_constants C, const rt_tp_buffers cur,
                                                               const rt_tp_buffers prev,
                                                               const float* __restrict__ cur_albedo,
                                                               const float* __restrict__ prev_moments,
                                                               float* __restrict__ out_color,
                                                               float* __restrict__ out_count,
                                                               float* __restrict__ out_moments,
                                                               uint8_t* __restrict__ out_rgba) {
  const int32_t x = (int32_t)(blockIdx.x * 64u + threadIdx.x), y = (int32_t)(blockIdx.y * 4u + threadIdx.y);
  if (x >= C.W || y >= C.H) return;
  const size_t p = (size_t)y * (size_t)C.W + (size_t)x;
  float out[3], n, m[2];
  rt_vr_tp_pixel(&C, &cur, &prev, cur_albedo, prev_moments, x, y, out, &n, m);
  out_color[p * 3 + 0] = out[0];
  out_color[p * 3 + 1] = out[1];
  out_color[p * 3 + 2] = out[2];
  out_count[p] = n;
  out_moments[p * 2 + 0] = m[0];
  out_moments[p * 2 + 1] = m[1];
  if (out_rgba)  // rt_tonemap_rgba of the stored floats
    *reinterpret_cast<uint32_t*>(out_rgba + p * 4) = tonemap_rgba8((double)out[0], (double)out[1], (double)out[2]);
}

__global__ __launch_bounds__(256) void variance_kernel(const rt_dn_level L, const double min_history,
                                                       const rt_vr_buffers in, float* __restrict__ out_var) {
  const int32_t x = (int32_t)(blockIdx.x * 64u + threadIdx.x), y = (int32_t)(blockIdx.y * 4u + threadIdx.y);
  if (x >= L.W || y >= L.H) return;
  out_var[(size_t)y * (size_t)L.W + (size_t)x] = rt_vr_variance_pixel(&L, min_history, &in, x, y);
}

__global__ __launch_bounds__(256) void denoise_var_prepare_kernel(const float* __restrict__ color,
                                                                  const float* __restrict__ albedo,
                                                                  const float* __restrict__ normal,
                                                                  const float* __restrict__ depth,
                                                                  const int32_t* __restrict__ object,
                                                                  const float* __restrict__ variance, size_t npix,
                                                                  rt_vr_color* __restrict__ e,
                                                                  rt_dn_guide* __restrict__ g,
                                                                  int32_t* __restrict__ id) {
  const size_t p = (size_t)blockIdx.x * 256u + threadIdx.x;  // (W * H <= 2^29)
  if (p >= npix) return;
  rt_vr_color ep;
  rt_dn_guide gp;
  int32_t idp;
  rt_vr_prepare(color, albedo, normal, depth, object, variance, p, &ep, &gp, &idp);
  e[p] = ep;
  g[p] = gp;
  id[p] = idp;
}

// kLast: the level's result goes to the outputs, not to e_out.  color may be
// out_linear and the call's variance may be out_variance (in place): the
// records hold what the levels read, a lane reads color[p] before it writes
// out_linear[p], and no other lane reads or writes that pixel of either.
template <bool kLast>
__global__ __launch_bounds__(256) void denoise_var_level_kernel(const rt_vr_level L, const rt_vr_color* __restrict__ e,
                                                                const rt_dn_guide* __restrict__ g,
                                                                const int32_t* __restrict__ id,
                                                                rt_vr_color* __restrict__ e_out, const float* color,
                                                                const float* albedo, float* out_linear,
                                                                uint8_t* out_rgba, float* out_variance) {
  const int32_t x = (int32_t)(blockIdx.x * 64u + threadIdx.x), y = (int32_t)(blockIdx.y * 4u + threadIdx.y);
  if (x >= L.dn.W || y >= L.dn.H) return;
  const size_t p = (size_t)y * (size_t)L.dn.W + (size_t)x;
  const rt_vr_color o = rt_vr_level_pixel(&L, e, g, id, x, y);
  if constexpr (!kLast) {
    e_out[p] = o;
  } else {
    float out[3];
    rt_vr_finish(&o, rt_dn_valid(g[p].z), color, albedo, p, out);
    if (out_linear) {
      out_linear[p * 3 + 0] = out[0];
      out_linear[p * 3 + 1] = out[1];
      out_linear[p * 3 + 2] = out[2];
    }
    if (out_rgba)  // rt_tonemap_rgba of the stored floats
      *reinterpret_cast<uint32_t*>(out_rgba + p * 4) = tonemap_rgba8((double)out[0], (double)out[1], (double)out[2]);
    if (out_variance) out_variance[p] = o.var;
  }
}

int launch_temporal_moments(const TemporalMomentsParams& p, void* stream) {
  const dim3 grid((unsigned)((p.t.c.W + 63) / 64), (unsigned)((p.t.c.H + 3) / 4)), block(64, 4);
  hipLaunchKernelGGL(temporal_moments_kernel, grid, block, 0, (hipStream_t)stream, p.t.c, p.t.cur, p.t.prev,
                     p.cur_albedo, p.prev_moments, p.t.out_color, p.t.out_count, p.out_moments, p.t.out_rgba);
  return (int)hipGetLastError();
}

int launch_variance(const VarianceParams& p, void* stream) {
  const rt_dn_level L = rt_dn_level_of(p.W, p.H, 0, p.vr.normal_power, 0.0, p.vr.sigma_depth);
  const dim3 grid((unsigned)((p.W + 63) / 64), (unsigned)((p.H + 3) / 4)), block(64, 4);
  hipLaunchKernelGGL(variance_kernel, grid, block, 0, (hipStream_t)stream, L, p.vr.min_history, p.in, p.out_var);
  return (int)hipGetLastError();
}

int launch_denoise_var(const DenoiseVarParams& p, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const size_t npix = (size_t)p.W * (size_t)p.H;
  if (npix == 0) return hipSuccess;
  const uintptr_t base = ((uintptr_t)p.workspace + (kDenoiseAlign - 1)) & ~(uintptr_t)(kDenoiseAlign - 1);
  rt_vr_color* e[2] = {reinterpret_cast<rt_vr_color*>(base), reinterpret_cast<rt_vr_color*>(base) + npix};
  rt_dn_guide* g = reinterpret_cast<rt_dn_guide*>(base + 2 * npix * sizeof(rt_vr_color));
  int32_t* id = reinterpret_cast<int32_t*>(base + 2 * npix * sizeof(rt_vr_color) + npix * sizeof(rt_dn_guide));
  const float* albedo = p.dn.demodulate ? p.albedo : nullptr;
  hipLaunchKernelGGL(denoise_var_prepare_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, p.color,
                     albedo, p.normal, p.depth, p.object, p.variance, npix, e[0], g, id);
  const dim3 grid((unsigned)((p.W + 63) / 64), (unsigned)((p.H + 3) / 4)), block(64, 4);
  for (int32_t i = 0; i < p.dn.levels; ++i) {
    const rt_vr_level L =
        rt_vr_level_of(p.W, p.H, i, p.dn.normal_power, p.dn.sigma_lum, p.dn.sigma_depth, p.dn.prefilter);
    const rt_vr_color* src = e[i & 1];
    if (i + 1 < p.dn.levels)
      hipLaunchKernelGGL(denoise_var_level_kernel<false>, grid, block, 0, st, L, src, g, id, e[(i & 1) ^ 1], p.color,
                         albedo, p.out_linear, p.out_rgba, p.out_variance);
    else
      hipLaunchKernelGGL(denoise_var_level_kernel<true>, grid, block, 0, st, L, src, g, id, (rt_vr_color*)nullptr,
                         p.color, albedo, p.out_linear, p.out_rgba, p.out_variance);
  }
  return (int)hipGetLastError();
}

int preload_variance_kernels() {
  hipFuncAttributes a;
  return (int)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(denoise_var_level_kernel<true>));
}

}  // namespace rtgo
