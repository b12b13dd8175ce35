// rt_temporal.hip — temporal accumulation over a camera sequence
// (rt_temporal_async, include/rt_api.h).  A file of its own:
// no other code object changes.
//
// The arithmetic is include/rt_temporal.h, the function rt_temporal_host runs:
// the kernel only decides which lane handles which pixel.  One launch, one lane
// per pixel; a wave covers 64 consecutive x of one row (rows are cut at the
// image edge), so the current frame's loads and the stores of a wave are
// contiguous, and so are the four taps' loads wherever the previous camera is
// close to the current one (neighbouring pixels land on neighbouring pixels).
// The buffers are read as the render and the feature pass wrote them: there is
// no workspace to hold packed records, and packing them would cost a pass over
// more bytes than the taps re-read.  The sums are per lane,
// in tap order: no atomics, no cross-lane operation, no LDS.
#include <hip/hip_runtime.h>

#include "../../include/rt_temporal.h"
#include "rt_device.h"
#include "rt_internal.h"

namespace rtgo {

// out_color / out_count never alias the previous frame's color / count
// (refused by the entry point), which the taps read at neighbouring pixels.
__global__ __launch_bounds__(256) void temporal_kernel(const rt_tp_constants C, const rt_tp_buffers cur,
                                                       const rt_tp_buffers prev, float* __restrict__ out_color,
                                                       float* __restrict__ out_count, uint8_t* __restrict__ out_rgba) {
  const int32_t x = (int32_t)(blockIdx.x * 64u + threadIdx.x), y = (int32_t)(blockIdx.y * 4u + threadIdx.y);
  if (x >= C.W || y >= C.H) return;
  const size_t p = (size_t)y * (size_t)C.W + (size_t)x;
  float out[3], n;
  rt_tp_pixel(&C, &cur, &prev, x, y, out, &n);
  out_color[p * 3 + 0] = out[0];
  out_color[p * 3 + 1] = out[1];
  out_color[p * 3 + 2] = out[2];
  out_count[p] = n;
  if (out_rgba)  // rt_tonemap_rgba of the stored floats
    *reinterpret_cast<uint32_t*>(out_rgba + p * 4) = tonemap_rgba8((double)out[0], (double)out[1], (double)out[2]);
}

int launch_temporal(const TemporalParams& p, void* stream) {
  const dim3 grid((unsigned)((p.c.W + 63) / 64), (unsigned)((p.c.H + 3) / 4)), block(64, 4);
  hipLaunchKernelGGL(temporal_kernel, grid, block, 0, (hipStream_t)stream, p.c, p.cur, p.prev, p.out_color, p.out_count,
                     p.out_rgba);
  return (int)hipGetLastError();
}

int preload_temporal_kernels() {
  hipFuncAttributes a;
  return (int)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(temporal_kernel));
}

}  // namespace rtgo
