// rt_denoise.hip — the à-trous denoiser guided by the first-hit feature
// buffers (rt_denoise_async, include/rt_api.h).  A file of its
// own: no other code object changes.
//
// The arithmetic is include/rt_denoise.h, the functions rt_denoise_host runs:
// the kernels only decide which lane handles which pixel.  A prepare kernel
// packs the inputs into two 16-byte records per pixel (the demodulated colour
// with the object id, and normal + depth), so that a tap costs two 16-byte
// loads.  Each level is one launch that reads one colour buffer and writes the
// other; the last one writes the outputs instead (remodulation, tone map).
// One lane per pixel, a wave covers 64 consecutive x of one row (rows are cut
// at the image edge), so a tap of a wave is one contiguous 1 KiB load per
// record.  The sums are per lane, in tap order: no atomics, no cross-lane
// operation, no LDS -- at preview sizes the records sit in L2 and the
// Infinity Cache, and the taps' re-reads are cache traffic.
#include <hip/hip_runtime.h>

#include "../../include/rt_denoise.h"
#include "rt_device.h"
#include "rt_internal.h"

namespace rtgo {

__global__ __launch_bounds__(256) void denoise_prepare_kernel(const float* __restrict__ color,
                                                              const float* __restrict__ albedo,
                                                              const float* __restrict__ normal,
                                                              const float* __restrict__ depth,
                                                              const int32_t* __restrict__ object, size_t npix,
                                                              rt_dn_color* __restrict__ e, rt_dn_guide* __restrict__ g) {
  const size_t p = (size_t)blockIdx.x * 256u + threadIdx.x;  // (W * H <= 2^29)
  if (p >= npix) return;
  rt_dn_color ep;
  rt_dn_guide gp;
  rt_dn_prepare(color, albedo, normal, depth, object, p, &ep, &gp);
  e[p] = ep;
  g[p] = gp;
}

// kLast: the level's result goes to the outputs, not to e_out.  color may be
// out_linear (in place): a lane reads color[p] before it writes out_linear[p],
// and no other lane reads or writes that pixel of either.
template <bool kLast>
__global__ __launch_bounds__(256) void denoise_level_kernel(const rt_dn_level L, const rt_dn_color* __restrict__ e,
                                                            const rt_dn_guide* __restrict__ g,
                                                            rt_dn_color* __restrict__ e_out, const float* color,
                                                            const float* albedo, float* out_linear,
                                                            uint8_t* out_rgba) {
  const int32_t x = (int32_t)(blockIdx.x * 64u + threadIdx.x), y = (int32_t)(blockIdx.y * 4u + threadIdx.y);
  if (x >= L.W || y >= L.H) return;
  const size_t p = (size_t)y * (size_t)L.W + (size_t)x;
  const rt_dn_color o = rt_dn_level_pixel(&L, e, g, x, y);
  if constexpr (!kLast) {
    e_out[p] = o;
  } else {
    float out[3];
    rt_dn_finish(&o, rt_dn_valid(g[p].z), color, albedo, p, out);
    if (out_linear) {
      out_linear[p * 3 + 0] = out[0];
      out_linear[p * 3 + 1] = out[1];
      out_linear[p * 3 + 2] = out[2];
    }
    if (out_rgba)  // rt_tonemap_rgba of the stored floats
      *reinterpret_cast<uint32_t*>(out_rgba + p * 4) = tonemap_rgba8((double)out[0], (double)out[1], (double)out[2]);
  }
}

int launch_denoise(const DenoiseParams& p, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const size_t npix = (size_t)p.W * (size_t)p.H;
  if (npix == 0) return hipSuccess;
  const uintptr_t base = ((uintptr_t)p.workspace + (kDenoiseAlign - 1)) & ~(uintptr_t)(kDenoiseAlign - 1);
  rt_dn_color* e[2] = {reinterpret_cast<rt_dn_color*>(base), reinterpret_cast<rt_dn_color*>(base) + npix};
  rt_dn_guide* g = reinterpret_cast<rt_dn_guide*>(base + 2 * npix * sizeof(rt_dn_color));
  const float* albedo = p.dn.demodulate ? p.albedo : nullptr;
  hipLaunchKernelGGL(denoise_prepare_kernel, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, p.color, albedo,
                     p.normal, p.depth, p.object, npix, e[0], g);
  const dim3 grid((unsigned)((p.W + 63) / 64), (unsigned)((p.H + 3) / 4)), block(64, 4);
  for (int32_t i = 0; i < p.dn.levels; ++i) {
    const rt_dn_level L = rt_dn_level_of(p.W, p.H, i, p.dn.normal_power, p.dn.sigma_color, p.dn.sigma_depth);
    const rt_dn_color* src = e[i & 1];
    if (i + 1 < p.dn.levels)
      hipLaunchKernelGGL(denoise_level_kernel<false>, grid, block, 0, st, L, src, g, e[(i & 1) ^ 1], p.color, albedo,
                         p.out_linear, p.out_rgba);
    else
      hipLaunchKernelGGL(denoise_level_kernel<true>, grid, block, 0, st, L, src, g, (rt_dn_color*)nullptr, p.color,
                         albedo, p.out_linear, p.out_rgba);
  }
  return (int)hipGetLastError();
}

int preload_denoise_kernels() {
  hipFuncAttributes a;
  return (int)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(denoise_level_kernel<true>));
}

}  // namespace rtgo
