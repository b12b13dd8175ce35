// rt_matte.hip — matte layers and the coverage-aware edge resolve
// (rt_context_render_matte_async, rt_matte_resolve_async, include/rt_api.h;
// DESIGN.md §4.19).  A file of its own: no other code object changes.
//
// matte_kernel is aov_kernel's walk (rt_aov.hip): one lane per pixel, 64-lane
// blocks, the render's own camera rays in ascending s, closest_hit with every
// primitive as a candidate, no cross-lane operation.  Instead of summing
// features it counts which object (or which face of it) each ray hits first.
// The 16 (key, count) slots of a lane are indexed by data, so they live in
// dynamic LDS behind the BVH stacks, one 32-bit column per lane (word
// slot * 64 + lane).  LDS has 64 banks of 4 bytes, so lane l's words are all in
// bank l: whichever slot each lane is at, no two lanes of a wave meet in a
// bank.  Nothing of it is a per-lane array that could go to scratch, and there
// is no static LDS.  The insert and the ranking are include/rt_matte.h's, the
// functions the sanitizer program runs.
//
// matte_resolve_kernel is rt_mt_resolve_pixel (include/rt_matte.h), the
// function rt_matte_resolve_host runs, one lane per pixel in 64x4 blocks; a
// pixel with fewer than two parts (95 % and more of a frame) copies its colour
// and leaves.
#include <hip/hip_runtime.h>

#include "../../include/rt_matte.h"
#include "rt_device.h"
#include "rt_internal.h"

namespace rtgo {

// dynamic LDS, 16-byte aligned: the BVH stacks (stack_depth x 64 ints, only
// for a scene with a tree), then the key columns and the count columns
// (RT_MT_SLOTS x 64 ints each); one-wave workgroups, so a wave's base is 0
extern __shared__ __attribute__((aligned(16))) unsigned char matte_lds[];

static size_t matte_stack_words(const AovParams& p) { return p.g.use_bvh ? (size_t)p.stack_depth * 64 : 0; }

// kSph, kMix: as aov_kernel.
template <bool kSph, bool kMix>
__global__ __launch_bounds__(64) void matte_kernel(const MatteParams q, const uint32_t stack_words) {
  typedef typename Kind<kSph>::H HitK;
  const AovParams& p = q.a;
  const unsigned px = blockIdx.x * 64u + threadIdx.x;  // y * W + x (W * H <= 2^29)
  if (px >= (unsigned)p.W * (unsigned)p.H) return;
  int* stack = reinterpret_cast<int*>(matte_lds) + threadIdx.x;
  int32_t* key = reinterpret_cast<int32_t*>(matte_lds) + stack_words + threadIdx.x;
  int32_t* count = key + RT_MT_SLOTS * 64;
  const int y = (int)(px / (unsigned)p.W), x = (int)(px - (unsigned)y * (unsigned)p.W);
  const CamK ck = make_cam(p.seed_key, p.W, p.H, p.cf);
  Geo g = p.g;
  if constexpr (kSph) {
    g.nt = 0;
    g.nb = 0;
  }
  const typename Kind<kSph>::C all = cand_all<kSph>();
  Counters nc;  // (nothing counts here)
  rt_mt_state st;
  rt_mt_begin(&st);
  for (int s = 0; s < p.spp; ++s) {
    rt_rng rng;
    d3 o, d;
    camera_ray_c<false>(ck, p.cf, x, y, s, rng, o, d, nc);
    HitK hs;
    if (!closest_hit<false, kSph, kMix>(g, o, d, hs, stack, all, nc)) continue;  // hitWorld(ray, 0.001, +Inf)
    int32_t self, f = 0;
    if (!hit_is_tri(hs)) {
      self = g.spheres[hs.idx].obj;
    } else {
      // every triangle belongs to a cube, and a cube is 12 consecutive
      // triangles in createCube's order (flatten_scene): the cube's first
      // triangle is the multiple of 12 at or below the index
      self = g.tris[hs.idx].obj;
      f = hs.idx - (hs.idx / 12) * 12;
    }
    rt_mt_insert(key, count, 64, &st, q.level == RT_MATTE_FACE ? self * 16 + f : self);
  }
  const size_t plane = (size_t)p.W * (size_t)p.H;
  int32_t rest = st.hits;
  for (int r = 0; r < q.ranks; ++r) {
    int32_t k = -1, c = 0;
    if (!rt_mt_take(key, count, 64, &st, &k, &c)) {
      k = -1;
      c = 0;
    }
    if (q.id) q.id[(size_t)r * plane + px] = k;
    if (q.count) q.count[(size_t)r * plane + px] = c;
    rest -= c;
  }
  if (q.rest) q.rest[px] = rest;
}

__global__ __launch_bounds__(256) void matte_resolve_kernel(const MatteResolveParams q) {
  const int32_t x = (int32_t)(blockIdx.x * 64u + threadIdx.x), y = (int32_t)(blockIdx.y * 4u + threadIdx.y);
  if (x >= q.r.W || y >= q.r.H) return;
  const size_t p = (size_t)y * (size_t)q.r.W + (size_t)x;
  float out[3];
  if (!rt_mt_resolve_pixel(&q.r, q.color, q.object, q.id, q.count, q.rest, x, y, out)) {
    out[0] = q.color[p * 3 + 0];
    out[1] = q.color[p * 3 + 1];
    out[2] = q.color[p * 3 + 2];
  }
  if (q.out_linear) {
    q.out_linear[p * 3 + 0] = out[0];
    q.out_linear[p * 3 + 1] = out[1];
    q.out_linear[p * 3 + 2] = out[2];
  }
  if (q.out_rgba)  // rt_tonemap_rgba of the stored floats
    *reinterpret_cast<uint32_t*>(q.out_rgba + p * 4) = tonemap_rgba8((double)out[0], (double)out[1], (double)out[2]);
}

int launch_matte(const MatteParams& q, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const AovParams& p = q.a;
  const size_t npix = (size_t)p.W * (size_t)p.H;
  if (npix == 0) return hipSuccess;
  const dim3 g((unsigned)((npix + 63) / 64)), b(64);
  const size_t sw = matte_stack_words(p);
  const size_t shmem = sizeof(int) * (sw + 2 * (size_t)RT_MT_SLOTS * 64);
  if (p.g.use_bvh == 2)
    hipLaunchKernelGGL((matte_kernel<false, true>), g, b, shmem, st, q, (uint32_t)sw);
  else if (p.g.nt == 0 && p.g.nb == 0)
    hipLaunchKernelGGL((matte_kernel<true, false>), g, b, shmem, st, q, (uint32_t)sw);
  else
    hipLaunchKernelGGL((matte_kernel<false, false>), g, b, shmem, st, q, (uint32_t)sw);
  return (int)hipGetLastError();
}

int launch_matte_resolve(const MatteResolveParams& q, void* stream) {
  const dim3 grid((unsigned)((q.r.W + 63) / 64), (unsigned)((q.r.H + 3) / 4)), block(64, 4);
  hipLaunchKernelGGL(matte_resolve_kernel, grid, block, 0, (hipStream_t)stream, q);
  return (int)hipGetLastError();
}

int preload_matte_kernels() {
  hipFuncAttributes a;
  const int e = (int)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(matte_kernel<true, false>));
  if (e != hipSuccess) return e;
  return (int)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(matte_resolve_kernel));
}

}  // namespace rtgo
