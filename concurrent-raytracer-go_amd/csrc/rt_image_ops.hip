// rt_image_ops.hip — kernels that never touch a ray: the gathered shares'
// unpack, the RGBA delta, the image download, the camera table's upload, the
// runtime's first-use warm-up and the bounded spin, each with its launch.
#include <hip/hip_runtime.h>

#include "rt_internal.h"

namespace rtgo {

// Gathered shares [world][share_bytes] (each: [max_local][1024] float3, then
// [max_local][1024] RGBA8 at rgba_off) -> W*H images.  One thread per image
// pixel, so the image writes are coalesced; a tile row's 32 pixels read 384
// contiguous bytes of its share.
__global__ __launch_bounds__(256) void unpack_kernel(int W, int H, int world, int tiles_x,
                                                     const uint8_t* __restrict__ g, size_t share_bytes,
                                                     size_t rgba_off, float* __restrict__ ol,
                                                     uint8_t* __restrict__ orgba) {
  const long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= (long long)W * H) return;
  const int y = (int)(o / W), x = (int)(o - (long long)y * W);
  const int t = (y >> 5) * tiles_x + (x >> 5);
  const int r = t % world, lt = t / world;
  const size_t pi = (size_t)lt * 1024 + (size_t)((y & 31) * 32 + (x & 31));
  const uint8_t* share = g + (size_t)r * share_bytes;
  if (ol) {
    const float* pl = reinterpret_cast<const float*>(share) + pi * 3;
    ol[o * 3 + 0] = pl[0];
    ol[o * 3 + 1] = pl[1];
    ol[o * 3 + 2] = pl[2];
  }
  if (orgba)
    *reinterpret_cast<uint32_t*>(orgba + o * 4) = *reinterpret_cast<const uint32_t*>(share + rgba_off + pi * 4);
}

// The same scatter for a partition: slot[t] = {owner rank, local tile}; frame
// blockIdx.y of nframes, gathered as [world][nframes][share], written to
// [nframes][W*H] images.
__global__ __launch_bounds__(256) void unpack_map_kernel(int W, int H, int tiles_x, int nframes,
                                                         const int2* __restrict__ slot, const uint8_t* __restrict__ g,
                                                         size_t share_bytes, size_t rgba_off, float* __restrict__ ol,
                                                         uint8_t* __restrict__ orgba) {
  const long long o = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= (long long)W * H) return;
  const int f = blockIdx.y;
  const long long oo = (long long)f * W * H + o;
  const int y = (int)(o / W), x = (int)(o - (long long)y * W);
  const int2 rl = slot[(y >> 5) * tiles_x + (x >> 5)];
  const size_t pi = (size_t)rl.y * 1024 + (size_t)((y & 31) * 32 + (x & 31));
  const uint8_t* share = g + ((size_t)rl.x * nframes + f) * share_bytes;
  if (ol) {
    const float* pl = reinterpret_cast<const float*>(share) + pi * 3;
    ol[oo * 3 + 0] = pl[0];
    ol[oo * 3 + 1] = pl[1];
    ol[oo * 3 + 2] = pl[2];
  }
  if (orgba)
    *reinterpret_cast<uint32_t*>(orgba + oo * 4) = *reinterpret_cast<const uint32_t*>(share + rgba_off + pi * 4);
}

// How much two RGBA8 images differ (rt_rgba_delta_async): out[0] += pixels
// whose four bytes are not all equal, out[1] = max(out[1], the largest byte
// difference).  One lane per pixel and step, one 32-bit load per image; a
// wave counts its differing pixels with a ballot (wave-uniform, every lane of
// the wave runs every step) and keeps each lane's largest difference, reduced
// across the wave once at the end: one add and one max per wave (none from a
// wave that saw no difference).  Integers only, so the result does not depend
// on the order.  Grid-stride: any npix.
__global__ __launch_bounds__(256) void rgba_delta_kernel(const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                         size_t npix, uint32_t* __restrict__ out) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const size_t lane = threadIdx.x & 63u;
  // the wave's first pixel of each step (wave-uniform, so is the trip count)
  size_t base = (size_t)blockIdx.x * blockDim.x + (threadIdx.x & ~63u);
  unsigned int changed = 0, dmax = 0;
  for (; base < npix; base += stride) {
    const size_t i = base + lane;
    unsigned int d = 0;
    bool diff = false;
    if (i < npix) {
      const uint32_t va = a[i], vb = b[i];
      diff = va != vb;
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int x = (int)((va >> (8 * c)) & 255u), y = (int)((vb >> (8 * c)) & 255u);
        d = max(d, (unsigned int)(x > y ? x - y : y - x));
      }
    }
    changed += (unsigned int)__popcll(__ballot(diff));
    dmax = max(dmax, d);
  }
  for (int off = 32; off >= 1; off >>= 1) dmax = max(dmax, __shfl_xor(dmax, off));
  if (lane == 0 && changed != 0) {
    atomicAdd(&out[0], changed);
    atomicMax(&out[1], dmax);
  }
}

int launch_rgba_delta(const uint8_t* d_a, const uint8_t* d_b, size_t npix, uint32_t* d_out, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(d_out, 0, 2 * sizeof(uint32_t), st);
  if (e != hipSuccess || npix == 0) return (int)e;
  const unsigned grid = (unsigned)((npix + 255) / 256 < 2048 ? (npix + 255) / 256 : 2048);
  hipLaunchKernelGGL(rgba_delta_kernel, dim3(grid), dim3(256), 0, st, reinterpret_cast<const uint32_t*>(d_a),
                     reinterpret_cast<const uint32_t*>(d_b), npix, d_out);
  return (int)hipGetLastError();
}

// The runtime's first-use set-up, on `stream`, so that it happens in the
// constructor (NewParallelRenderer, main.go:46-47) instead of inside the
// first Render (profiles/r04_cli_trace.json, a fresh `raytracer` process;
// scripts/copy_probe.hip):
//   - an empty launch (kernel argument pool);
//   - a launch with private (scratch) memory: the first kernel that needs
//     scratch makes the runtime allocate the device's scratch pool (the
//     first render launch started 1.26 ms after it was enqueued); 512 B per
//     lane covers every render kernel variant (<= 328 B);
//   - copies each way through pageable and pinned memory, and device->host
//     copies queued behind a kernel that is still running: the first time a
//     process's copy has to wait for a running kernel it starts ~8-9 ms after
//     the kernel ends (the CLI's image download; scripts/copy_probe.hip:
//     later ones start at once, 0.16 ms for 8 MB).  warm_busy runs ~0.2 ms
//     so the copies are queued while it still runs.
//     (Render itself copies only from an idle stream, rt_renderer_render.)
__global__ void warm_kernel(int* p) {
  if (p && threadIdx.x == 0 && blockIdx.x == 0) p[0] = 0;
}
__global__ void warm_scratch(int* p, int n) {
  volatile int a[128];  // (volatile: kept in private memory)
  for (int i = 0; i < 128; ++i) a[i] = i * n + (int)threadIdx.x;
  if (p && n < 0) p[threadIdx.x] = a[(threadIdx.x * 7) & 127];
}
__global__ void warm_busy(float* p, int iters) {
  float v = (float)threadIdx.x;
  for (int k = 0; k < iters; ++k) v = v * 0.999f + 1.0f;  // a dependent chain: ~4 clocks per step
  if (p && v < 0.f) p[threadIdx.x] = v;
}
int warm_device(void* stream, void* dev_buf, void* host_pinned, void* host_pageable, size_t bytes) {
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(warm_kernel, dim3(1), dim3(64), 0, st, (int*)dev_buf);
  hipLaunchKernelGGL(warm_scratch, dim3(1), dim3(64), 0, st, (int*)dev_buf, 1);
  static thread_local unsigned char host[4096];
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = hipMemcpyAsync(dev_buf, host, sizeof host, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(host, dev_buf, sizeof host, hipMemcpyDeviceToHost, st);
  if (e == hipSuccess) e = hipMemcpyAsync(dev_buf, host_pinned, bytes, hipMemcpyHostToDevice, st);
  if (e == hipSuccess) e = hipMemcpyAsync(dev_buf, host_pageable, bytes, hipMemcpyHostToDevice, st);
  for (int k = 0; k < 2 && e == hipSuccess; ++k) {  // behind a kernel: into pageable, then pinned memory
    hipLaunchKernelGGL(warm_busy, dim3(1), dim3(64), 0, st, (float*)dev_buf, 10000);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(k ? host_pinned : host_pageable, dev_buf, bytes, hipMemcpyDeviceToHost, st);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(st);
  return (int)e;
}

// The image to pinned host memory, written by the GPU itself (16 B per lane,
// coalesced): the first Render of a renderer, where a copy-engine transfer
// started 7-15 ms late in a fresh process (rt_renderer_render).
__global__ __launch_bounds__(256) void download_kernel(const uint4* __restrict__ src, uint4* __restrict__ dst, size_t n16) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x)
    dst[i] = src[i];
}
int launch_download(const void* d_src, void* h_dst_mapped, size_t bytes, void* stream) {
  if (bytes == 0) return hipSuccess;
  if ((bytes & 15) || ((uintptr_t)d_src & 15) || ((uintptr_t)h_dst_mapped & 15)) return hipErrorInvalidValue;
  const size_t n16 = bytes / 16;
  const unsigned grid = (unsigned)((n16 + 255) / 256 < 2048 ? (n16 + 255) / 256 : 2048);
  hipLaunchKernelGGL(download_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, (const uint4*)d_src,
                     (uint4*)h_dst_mapped, n16);
  return (int)hipGetLastError();
}

// A camera sequence's CamFrames from the launch's own arguments to the table
// the stream kernels read: the runtime copies the arguments
// when the launch is enqueued, so nothing of the caller's is read later and no
// staging buffer has to outlive the call.  One 8-byte word per lane.
__global__ __launch_bounds__(64) void cam_upload_kernel(const CamTable t, int words, uint64_t* __restrict__ dst) {
  static_assert(sizeof(CamFrame) % 8 == 0 && sizeof(CamTable) + 16 <= 4096, "the table travels as a kernel argument");
  const uint64_t* src = reinterpret_cast<const uint64_t*>(&t);
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i < words) dst[i] = src[i];
}
int launch_cam_upload(const CamTable& t, int n, CamFrame* d_cams, void* stream) {
  if (n < 1 || n > kMaxFrames || !d_cams) return (int)hipErrorInvalidValue;
  const int words = n * (int)(sizeof(CamFrame) / 8);
  hipLaunchKernelGGL(cam_upload_kernel, dim3((unsigned)((words + 63) / 64)), dim3(64), 0, (hipStream_t)stream, t, words,
                     reinterpret_cast<uint64_t*>(d_cams));
  return (int)hipGetLastError();
}

// s_memrealtime counts at 100 MHz: the wave sleeps until `ticks` have passed
// since it started (a bounded wait: it always ends)
__global__ void spin_kernel(unsigned long long ticks) {
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  while (__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(127);
}
int launch_spin(double ms, void* stream) {
  const double t = ms < 60000.0 ? ms : 60000.0;  // at most a minute
  hipLaunchKernelGGL(spin_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (unsigned long long)(t * 1e5));
  return (int)hipGetLastError();
}

int launch_unpack(int32_t W, int32_t H, int32_t world, const void* gathered, size_t share_bytes, size_t rgba_off,
                  float* ol, uint8_t* orgba, void* stream) {
  const long long total = (long long)W * H;
  if (total <= 0) return hipSuccess;
  const unsigned blocks = (unsigned)((total + 255) / 256);
  hipLaunchKernelGGL(unpack_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, W, H, world, (W + 31) / 32,
                     (const uint8_t*)gathered, share_bytes, rgba_off, ol, orgba);
  return (int)hipGetLastError();
}

int launch_unpack_map(int32_t W, int32_t H, int32_t nframes, const int32_t* slot, const void* gathered,
                      size_t share_bytes, size_t rgba_off, float* ol, uint8_t* orgba, void* stream) {
  const long long total = (long long)W * H;
  if (total <= 0 || nframes <= 0) return hipSuccess;
  const unsigned blocks = (unsigned)((total + 255) / 256);
  hipLaunchKernelGGL(unpack_map_kernel, dim3(blocks, nframes), dim3(256), 0, (hipStream_t)stream, W, H, (W + 31) / 32,
                     nframes, reinterpret_cast<const int2*>(slot), (const uint8_t*)gathered, share_bytes, rgba_off, ol,
                     orgba);
  return (int)hipGetLastError();
}

// (see preload_render_kernels)
int preload_image_kernels() {
  hipFuncAttributes a;
  return (int)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(unpack_kernel));
}

}  // namespace rtgo
