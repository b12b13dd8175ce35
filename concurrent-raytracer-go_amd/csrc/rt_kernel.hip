// rt_kernel.hip — the megakernel's block kernels: one one-wave workgroup
// renders one work block (render_kernel, render_kernel_mix, render_kernel_tail)
// through render_body (rt_body.h, which holds the design summary), and their
// launch.  The streamed launches' kernels are in rt_stream.hip.
#include "rt_body.h"

namespace rtgo {

template <bool kCount, bool kStage, bool kPilot, bool kSky>
__global__ __launch_bounds__(64, RT_WAVES_PER_SIMD) void render_kernel(const KParams pk) {
  render_body<BlockBody<kCount, kStage, kPilot, kSky>>(pk);
}
// The unstaged render_kernel whose BVH branches (closest_hit / any_hit, kMix)
// also take leaves of cubes: kernels of their own, picked by launch_render for
// a tree that has such leaves, so the others keep their code and registers
// (DESIGN.md §4.2).
template <bool kCount, bool kPilot, bool kSky>
__global__ __launch_bounds__(64, RT_WAVES_PER_SIMD) void render_kernel_mix(const KParams pk) {
  render_body<MixBody<kCount, kPilot, kSky>>(pk);
}
// the staged product render with tail helpers (rt_tuning.tail_helpers > 0)
__global__ __launch_bounds__(64, RT_WAVES_PER_SIMD) void render_kernel_tail(const KParams pk) {
  render_body<TailBody>(pk);
}

// A launch of one frame: frame entry 0 from the single-frame fields
// (launch_stream, launch_render)
void single_frame_entry(KParams& p) {
  if (p.nframes > 1) return;
  p.nframes = 1;
  p.frame_key[0] = p.seed_key;
  p.frame_lin[0] = p.out_linear;
  p.frame_rgba[0] = p.out_rgba;
}

size_t render_shmem(const KParams& p) {
  return (size_t)p.stack_off + (p.use_bvh ? sizeof(int) * p.stack_depth * 64 : 0);
}

// Loads this file's code object onto the current device now: with HIP's lazy
// loading it would otherwise be loaded inside the first render launch
// (rt_context_create calls it once per device and process).
int preload_render_kernels() {
  hipFuncAttributes a;
  return (int)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(render_kernel<false, true, false, false>));
}

int launch_render(const KParams& pin, bool count, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  if (pin.num_wgs <= 0) return hipSuccess;
  KParams p = pin;
  single_frame_entry(p);
  const size_t shmem = render_shmem(p);
  const bool stage = p.stage_bytes > 0;
  // tail helpers: render_kernel_tail exports paths;
  // tail_helpers one-wave workgroups follow its num_wgs main blocks
  const bool tail = p.tail && stage && !count && !p.sky && !p.work_max && p.acc_mode == 0 && p.tail_helpers > 0;
  if (!tail) p.tail = nullptr;
  const dim3 g(p.num_wgs + (tail ? p.tail_helpers : 0)), b(64);
  // (the opted-in sky has instantiations of its own: its code would cost the
  // others registers; the pilot and the counting variant ignore it -- path
  // lengths and counts do not depend on what a miss returns)
  if (count && p.sky) {
    // counts with an opted-in sky: the image comes from the sky variant, the
    // counts from a second, output-less launch of the counting variant (it
    // leaves the split rows zeroed like any launch and neither reads nor
    // writes the sample-pass sums)
    KParams q = p;
    q.counts = nullptr;
    const int e = launch_render(q, false, stream);
    if (e != hipSuccess) return e;
    q = p;
    q.sky = nullptr;
    q.out_linear = nullptr;
    q.out_rgba = nullptr;
    q.acc = nullptr;
    q.acc_mode = 0;
    return launch_render(q, true, stream);
  }
  if (p.use_bvh == 2) {  // a tree with leaves of cubes (never staged): render_kernel_mix
    if (p.work_max)
      hipLaunchKernelGGL((render_kernel_mix<false, true, false>), g, b, shmem, st, p);
    else if (count)
      hipLaunchKernelGGL((render_kernel_mix<true, false, false>), g, b, shmem, st, p);
    else if (p.sky)
      hipLaunchKernelGGL((render_kernel_mix<false, false, true>), g, b, shmem, st, p);
    else
      hipLaunchKernelGGL((render_kernel_mix<false, false, false>), g, b, shmem, st, p);
  } else if (p.work_max) {  // a measuring render (pilot or first frame): its own instantiation (and kernel name)
    if (stage)
      hipLaunchKernelGGL((render_kernel<false, true, true, false>), g, b, shmem, st, p);
    else
      hipLaunchKernelGGL((render_kernel<false, false, true, false>), g, b, shmem, st, p);
  } else if (count && stage) {
    hipLaunchKernelGGL((render_kernel<true, true, false, false>), g, b, shmem, st, p);
  } else if (count) {
    hipLaunchKernelGGL((render_kernel<true, false, false, false>), g, b, shmem, st, p);
  } else if (p.sky && stage) {
    hipLaunchKernelGGL((render_kernel<false, true, false, true>), g, b, shmem, st, p);
  } else if (p.sky) {
    hipLaunchKernelGGL((render_kernel<false, false, false, true>), g, b, shmem, st, p);
  } else if (stage && tail) {
    hipLaunchKernelGGL(render_kernel_tail, g, b, shmem, st, p);
  } else if (stage) {
    hipLaunchKernelGGL((render_kernel<false, true, false, false>), g, b, shmem, st, p);
  } else {
    hipLaunchKernelGGL((render_kernel<false, false, false, false>), g, b, shmem, st, p);
  }
  return (int)hipGetLastError();
}

// Cross-lane reads from inactive lanes counted by this file's kernels in an
// RT_CHECK_XLANE build (rt_device.h); -1 in a normal build.  reset: zero it.
long long xlane_faults_kernel(bool reset) { return xlane_faults_unit(reset); }

}  // namespace rtgo
