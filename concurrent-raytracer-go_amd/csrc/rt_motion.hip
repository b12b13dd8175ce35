// rt_motion.hip — temporal accumulation with per-object motion
// (rt_temporal_motion_async, include/rt_api.h).  A file of its
// own: no other code object changes.
//
// The arithmetic is include/rt_motion.h, the function rt_temporal_motion_host
// runs: the kernel only decides which lane handles which pixel.  One launch,
// one lane per pixel; a wave covers 64 consecutive x of one row (rows are cut
// at the image edge), as temporal_kernel does, so the current frame's loads and
// the stores of a wave are contiguous.  The sums are per lane, in tap order: no
// atomics, no cross-lane operation, no LDS.  The motion table is read where it
// lies: one guarded 24-byte gather per valid pixel, and the lanes of a wave
// mostly share an id and so a cache line (DESIGN.md §4.17 has the measurement
// that decided against staging a prefix of it in LDS).
#include <hip/hip_runtime.h>

#include "../../include/rt_motion.h"
#include "rt_device.h"
#include "rt_internal.h"

namespace rtgo {

// out_color / out_count / out_moments never alias the previous frame's color /
// count / moments (refused by the entry point), which the taps read at
// neighbouring pixels.  kMoments false: cur_albedo, prev_moments and
// out_moments are null and not used.
template <bool kMoments>
__global__ __launch_bounds__(256) void temporal_motion_kernel(const rt_tp_constants C, const rt_tp_buffers cur,
                                                              const rt_tp_buffers prev,
                                                              const double* __restrict__ motion,
                                                              const int32_t num_objects,
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
  rt_mo_pixel(kMoments ? 1 : 0, &C, &cur, &prev, motion, num_objects, cur_albedo, prev_moments, x, y, out, &n, m);
  out_color[p * 3 + 0] = out[0];
  out_color[p * 3 + 1] = out[1];
  out_color[p * 3 + 2] = out[2];
  out_count[p] = n;
  if constexpr (kMoments) {
    out_moments[p * 2 + 0] = m[0];
    out_moments[p * 2 + 1] = m[1];
  }
  if (out_rgba)  // rt_tonemap_rgba of the stored floats
    *reinterpret_cast<uint32_t*>(out_rgba + p * 4) = tonemap_rgba8((double)out[0], (double)out[1], (double)out[2]);
}

int launch_temporal_motion(const TemporalMotionParams& p, void* stream) {
  const TemporalParams& t = p.m.t;
  const dim3 grid((unsigned)((t.c.W + 63) / 64), (unsigned)((t.c.H + 3) / 4)), block(64, 4);
  if (p.m.out_moments)
    hipLaunchKernelGGL(temporal_motion_kernel<true>, grid, block, 0, (hipStream_t)stream, t.c, t.cur, t.prev, p.motion,
                       p.num_objects, p.m.cur_albedo, p.m.prev_moments, t.out_color, t.out_count, p.m.out_moments,
                       t.out_rgba);
  else
    hipLaunchKernelGGL(temporal_motion_kernel<false>, grid, block, 0, (hipStream_t)stream, t.c, t.cur, t.prev, p.motion,
                       p.num_objects, (const float*)nullptr, (const float*)nullptr, t.out_color, t.out_count,
                       (float*)nullptr, t.out_rgba);
  return (int)hipGetLastError();
}

int preload_motion_kernels() {
  hipFuncAttributes a;
  return (int)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(temporal_motion_kernel<true>));
}

}  // namespace rtgo
