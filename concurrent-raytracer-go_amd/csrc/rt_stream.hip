// rt_stream.hip — the megakernel's streamed launches: the six
// stream kernels, builds of render_body (rt_body.h) whose persistent waves
// drain a launch-wide entry queue, resolve_rows_kernel and their launch.
#include "rt_body.h"

// ... of the spheres-only stream kernels (render_stream_sph_kernel): 4 fit
// without scratch (128 VGPRs) and measured 5 % faster than 3
#ifndef RT_STREAM_SPH_WAVES
#define RT_STREAM_SPH_WAVES 4
#endif

namespace rtgo {

// ---- streamed launches
// One persistent one-wave workgroup per resident wave slot; each drains the
// launch-wide entry queue (render_body<StreamBody> and its three siblings).
__global__ __launch_bounds__(64, RT_WAVES_PER_SIMD) void render_stream_kernel(const StreamKArgs a) {
  render_body<StreamBody>(a.k);
}
// The same with KParams::sample_base added to every entry's sample index (a
// progression's adds after its first).
__global__ __launch_bounds__(64, RT_WAVES_PER_SIMD) void render_stream_base_kernel(const StreamKArgs a) {
  render_body<StreamBaseBody>(a.k);
}
// The two for a scene of spheres alone (kSph; launch_stream picks them), with
// a waves-per-SIMD bound of their own.
__global__ __launch_bounds__(64, RT_STREAM_SPH_WAVES) void render_stream_sph_kernel(const StreamKArgs a) {
  render_body<StreamSphBody>(a.k);
}
__global__ __launch_bounds__(64, RT_STREAM_SPH_WAVES) void render_stream_sph_base_kernel(const StreamKArgs a) {
  render_body<StreamSphBaseBody>(a.k);
}
// The two of a camera sequence (kCams): frame fl of the launch
// shoots from StreamParams::cams[frame0 + fl].  No kBase twins: a progression
// has one camera.
__global__ __launch_bounds__(64, RT_WAVES_PER_SIMD) void render_stream_cams_kernel(const StreamKArgs a) {
  render_body<StreamCamsBody>(a.k);
}
__global__ __launch_bounds__(64, RT_STREAM_SPH_WAVES) void render_stream_sph_cams_kernel(const StreamKArgs a) {
  render_body<StreamSphCamsBody>(a.k);
}
// After it on the same stream: one lane per pixel of the rank's tiles, per
// frame of the launch (blockIdx.y).  Lane t writes local pixel t black when it
// is not live (what the block kernel's epilogue writes for it: a sum of +0),
// and sums live pixel t's spp rows in sample order from +0 -- tracePixel's sum
// (renderer.go:150-163), a miss having stored +0 -- then mean, tone map and
// write through store_pixel, as the block kernel's epilogue.  Consecutive
// lanes read consecutive rows (StreamParams: row = (fl * spp + s) * nlive + i).
__global__ __launch_bounds__(256) void resolve_rows_kernel(const StreamKArgs a) {
  const KArg k = fresh();
  const SArg sk = sfresh();
  const unsigned t = blockIdx.x * 256u + threadIdx.x;
  const int fl = (int)blockIdx.y, fr = sk->s.frame0 + fl;
  if (t < (unsigned)sk->s.npix && sk->s.live_pos[t] < 0) {
    const int lt = (int)(t >> 10), tp = (int)(t & 1023u);
    const int tile = sk->s.tile_list ? sk->s.tile_list[lt] : k->rank + lt * k->world;
    const int x = (tile % k->tiles_x) * 32 + (tp & 31), y = (tile / k->tiles_x) * 32 + (tp >> 5);
    if (tile < k->ntiles && x < k->W && y < k->H)
      store_pixel(k, fr, k->layout == RT_LAYOUT_IMAGE ? (size_t)y * k->W + x : (size_t)t, 0.0, 0.0, 0.0);
  }
  if (t < (unsigned)sk->s.nlive) {
    const int4 it = reinterpret_cast<const int4*>(sk->s.live)[t];
    const size_t nlive = (size_t)sk->s.nlive;
    const int spp = k->spp;
    const double* __restrict__ row = sk->s.rows + ((size_t)fl * spp * nlive + t) * 3;
    // (a progression's add, one frame: the pixel's sum over the earlier
    // samples is continued and stored back)
    double* const acc = sk->s.acc ? sk->s.acc + (size_t)it.w * 3 : nullptr;
    double sx = 0, sy = 0, sz = 0;
    if (acc) {
      sx = acc[0];
      sy = acc[1];
      sz = acc[2];
    }
    for (int s = 0; s < spp; ++s, row += nlive * 3) {
      sx += row[0];
      sy += row[1];
      sz += row[2];
    }
    if (acc) {
      acc[0] = sx;
      acc[1] = sy;
      acc[2] = sz;
    }
    store_pixel(k, fr, k->layout == RT_LAYOUT_IMAGE ? (size_t)(uint32_t)it.z : (size_t)it.w, sx, sy, sz);
  }
}

// The stream kernel of a launch (kStreamKernels of them): bit 0 the kBase
// twin, bit 1 the spheres-only build; 4 and 5: a camera sequence's generic and
// spheres-only kernels.
typedef void (*StreamKernel)(const StreamKArgs);
static StreamKernel stream_kernel_fn(int kernel) {
  switch (kernel) {
    case 0: return render_stream_kernel;
    case 1: return render_stream_base_kernel;
    case 2: return render_stream_sph_kernel;
    case 3: return render_stream_sph_base_kernel;
    case 4: return render_stream_cams_kernel;
    default: return render_stream_sph_cams_kernel;
  }
}
int stream_kernel_of(const KParams& p, bool cams) {
  const bool sph = p.nt == 0 && p.nb == 0;
  if (cams) return sph ? 5 : 4;
  return (p.sample_base != 0 ? 1 : 0) | (sph ? 2 : 0);
}

// Resident one-wave workgroups of that kernel on `device` (the current one)
// with `shmem` bytes of dynamic LDS: what the runtime reports per CU for the
// kernel's own registers and LDS, times the CUs.  0: no answer.
int stream_wave_slots(int device, int kernel, size_t shmem) {
  hipDeviceProp_t pr;
  if (hipGetDeviceProperties(&pr, device) != hipSuccess || pr.multiProcessorCount <= 0) return 0;
  int per_cu = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, reinterpret_cast<const void*>(stream_kernel_fn(kernel)), 64,
                                                   shmem) != hipSuccess ||
      per_cu <= 0)
    return 0;
  return pr.multiProcessorCount * per_cu;
}

int launch_stream(const KParams& pin, const StreamParams& sp, int wgs, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  StreamKArgs a;
  a.k = pin;
  a.s = sp;
  KParams& p = a.k;
  single_frame_entry(p);
  p.tail = nullptr;
  if (p.stage_bytes <= 0 || p.use_bvh || wgs <= 0 || sp.frames <= 0 || sp.npix <= 0) return (int)hipErrorInvalidValue;
  // (a sequence's table holds a frame per entry of frame_*; its kernels have no sample_base twin)
  if (sp.cams && (p.sample_base != 0 || sp.frame0 < 0 || sp.frame0 + sp.frames > kMaxFrames)) return (int)hipErrorInvalidValue;
  hipError_t e = hipMemsetAsync(sp.cursor, 0, sizeof(unsigned int), st);
  if (e != hipSuccess) return (int)e;
  // (a scene without triangles and cubes -- every scene the auto rule streams
  // -- takes the spheres-only build; triangles streamed by force the generic one)
  hipLaunchKernelGGL(stream_kernel_fn(stream_kernel_of(p, sp.cams != nullptr)), dim3(wgs), dim3(64), render_shmem(p), st, a);
  e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  hipLaunchKernelGGL(resolve_rows_kernel, dim3((unsigned)((sp.npix + 255) / 256), (unsigned)sp.frames), dim3(256), 0, st, a);
  return (int)hipGetLastError();
}

// (see preload_render_kernels)
int preload_stream_kernels() {
  hipFuncAttributes a;
  return (int)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(resolve_rows_kernel));
}

// Cross-lane reads from inactive lanes counted by this file's kernels in an
// RT_CHECK_XLANE build (rt_device.h); -1 in a normal build.  reset: zero it.
long long xlane_faults_stream(bool reset) { return xlane_faults_unit(reset); }

}  // namespace rtgo
