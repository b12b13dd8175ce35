// rt_adaptive.hip — the kernels of an adaptive progression:
// the per-pixel stop rule after an add, and the sample counts laid out for the
// caller.  A file of its own: the render kernels' code object stays what it
// was.
#include <hip/hip_runtime.h>

#include "../../include/rt_adaptive.h"
#include "rt_device.h"
#include "rt_internal.h"

namespace rtgo {

// ---- adaptive progressions
// After the render launches of an adaptive add, which only carried the sums:
// one lane per pixel of the rank's tiles.  An active pixel got n more samples:
// its count grows, its new displayed value is compared with the kept one by
// the stop rule (rt_adaptive_rule, include/rt_adaptive.h) and it may stop.
// Every in-image pixel, stopped ones included, then gets its mean over its own
// count written as store_pixel writes it -- the only writer of an adaptive
// add's image.  A wave counts its active pixels with a ballot and sums its
// counts across the lanes (wave-uniform: every lane of every wave gets here,
// the grid covers whole tiles), one atomic per wave for each.  Integers only.
__global__ __launch_bounds__(256) void adaptive_update_kernel(const AdaptParams p) {
  const unsigned t = blockIdx.x * 256u + threadIdx.x;
  bool act = false;
  unsigned int cnt = 0;
  if (t < (unsigned)p.npix) {
    const int lt = (int)(t >> 10), tp = (int)(t & 1023u);
    const int tile = p.tile_list ? p.tile_list[lt] : p.rank + lt * p.world;
    const int x = (tile % p.tiles_x) * 32 + (tp & 31), y = (tile / p.tiles_x) * 32 + (tp >> 5);
    if (tile < p.ntiles && x < p.W && y < p.H) {
      cnt = p.count[t];
      act = p.active[t] != 0u;
      const double sx = p.acc[(size_t)t * 3 + 0], sy = p.acc[(size_t)t * 3 + 1], sz = p.acc[(size_t)t * 3 + 2];
      if (act) cnt += (unsigned int)p.n;
      const double n = (double)cnt;
      const double mx = sx / n, my = sy / n, mz = sz / n;  // DivScalar(float64(samples)), as store_pixel
      const uint32_t px = tonemap_rgba8(mx, my, mz);
      if (act) {
        int32_t streak = 0;
        const int stop = rt_adaptive_rule(p.rgba[t], px, cnt > (unsigned int)p.n, (int32_t)cnt, (int32_t)p.streak[t],
                                          p.tolerance, p.patience, p.min_samples, &streak);
        p.count[t] = cnt;
        p.streak[t] = (uint32_t)streak;
        p.rgba[t] = px;
        if (stop) {
          p.active[t] = 0u;
          act = false;
        }
      }
      const size_t oi = p.layout == RT_LAYOUT_IMAGE ? (size_t)y * p.W + x : (size_t)t;
      if (p.out_linear) {
        p.out_linear[oi * 3 + 0] = (float)mx;
        p.out_linear[oi * 3 + 1] = (float)my;
        p.out_linear[oi * 3 + 2] = (float)mz;
      }
      if (p.out_rgba) *reinterpret_cast<uint32_t*>(p.out_rgba + oi * 4) = px;
    }
  }
  const unsigned int nact = (unsigned int)__popcll(__ballot(act));
  unsigned int csum = cnt;  // (at most 64 x 2^24)
  for (int off = 32; off >= 1; off >>= 1) csum += __shfl_xor(csum, off);
  if ((threadIdx.x & 63u) == 0) {
    if (nact) atomicAdd(&p.totals[0], (unsigned long long)nact);
    if (csum) atomicAdd(&p.totals[1], (unsigned long long)csum);
  }
}

int launch_adaptive_update(const AdaptParams& p, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(p.totals, 0, 2 * sizeof(unsigned long long), st);
  if (e != hipSuccess || p.npix <= 0) return (int)e;
  hipLaunchKernelGGL(adaptive_update_kernel, dim3((unsigned)((p.npix + 255) / 256)), dim3(256), 0, st, p);
  return (int)hipGetLastError();
}

// The sample counts in the caller's layout: one lane per local pixel.
__global__ __launch_bounds__(256) void progressive_counts_kernel(const AdaptParams p, uint32_t uniform,
                                                                 uint32_t* __restrict__ out) {
  const unsigned t = blockIdx.x * 256u + threadIdx.x;
  if (t >= (unsigned)p.npix) return;
  const int lt = (int)(t >> 10), tp = (int)(t & 1023u);
  const int tile = p.tile_list ? p.tile_list[lt] : p.rank + lt * p.world;
  const int x = (tile % p.tiles_x) * 32 + (tp & 31), y = (tile / p.tiles_x) * 32 + (tp >> 5);
  const bool in = tile < p.ntiles && x < p.W && y < p.H;
  const uint32_t v = in ? (p.count ? p.count[t] : uniform) : 0u;
  if (p.layout == RT_LAYOUT_IMAGE) {
    if (in) out[(size_t)y * p.W + x] = v;
  } else {
    out[t] = v;
  }
}

int launch_progressive_counts(const AdaptParams& p, uint32_t uniform, uint32_t* d_out, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (p.layout == RT_LAYOUT_IMAGE) {
    const hipError_t e = hipMemsetAsync(d_out, 0, (size_t)p.W * p.H * sizeof(uint32_t), st);
    if (e != hipSuccess) return (int)e;
  }
  if (p.npix <= 0) return hipSuccess;
  hipLaunchKernelGGL(progressive_counts_kernel, dim3((unsigned)((p.npix + 255) / 256)), dim3(256), 0, st, p, uniform,
                     d_out);
  return (int)hipGetLastError();
}

}  // namespace rtgo
