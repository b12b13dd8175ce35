// rt_aov.hip — first-hit feature buffers (rt_context_render_aov_async,
// include/rt_api.h): per pixel, the albedo, normal, depth,
// coverage and object id of its camera rays' first hits.  One camera ray and
// one closest hit per sample: no lighting, no shadow rays, no bounces.  A file
// of its own: the render kernels' code objects stay what they were.
//
// One lane per pixel, each lane walking its n samples in ascending order, so
// the per-pixel binary64 sums are in sample order by construction and the
// writes of a wave are 64 consecutive pixels.  The camera ray is the render's
// own (make_cam / camera_ray_c), the hit is closest_hit with every primitive
// as a candidate, and the hit record is rt_body.h's hit_record, expression for
// expression.  No lane reads another: there is no cross-lane operation here.
// aov_spec_kernel (below) is the same pass taken through the
// scene's mirrors: the features of the first surface that is not mirror-like.
#include <hip/hip_runtime.h>

#include "rt_device.h"
#include "rt_internal.h"

namespace rtgo {

// dynamic LDS: the BVH stacks, stack_depth x 64 ints, one column per lane
// (closest_hit's stack[sp * 64]); one-wave workgroups, so a wave's base is 0
extern __shared__ __attribute__((aligned(16))) unsigned char aov_lds[];

// kSph: the scene has no triangle (no cube); kMix: its tree has leaves of
// cubes.  A tree over spheres alone is kSph with p.g.use_bvh set.
template <bool kSph, bool kMix>
__global__ __launch_bounds__(64) void aov_kernel(const AovParams p) {
  typedef typename Kind<kSph>::H HitK;
  const unsigned px = blockIdx.x * 64u + threadIdx.x;  // y * W + x (W * H <= 2^29)
  if (px >= (unsigned)p.W * (unsigned)p.H) return;
  int* stack = reinterpret_cast<int*>(aov_lds) + threadIdx.x;
  const int y = (int)(px / (unsigned)p.W), x = (int)(px - (unsigned)y * (unsigned)p.W);
  const CamK ck = make_cam(p.seed_key, p.W, p.H, p.cf);
  Geo g = p.g;
  if constexpr (kSph) {
    g.nt = 0;
    g.nb = 0;
  }
  const typename Kind<kSph>::C all = cand_all<kSph>();
  Counters nc;  // (nothing counts here)
  double ax = 0, ay = 0, az = 0, nx = 0, ny = 0, nz = 0, st = 0;
  int hits = 0, first = -1;
  for (int s = 0; s < p.spp; ++s) {
    rt_rng rng;
    d3 o, d;
    camera_ray_c<false>(ck, p.cf, x, y, s, rng, o, d, nc);
    HitK hs;
    if (!closest_hit<false, kSph, kMix>(g, o, d, hs, stack, all, nc)) continue;  // hitWorld(ray, 0.001, +Inf)
    // HitRecord (sphere.go:42-58, triangle.go:67-81), as hit_record (rt_body.h) writes it
    d3 N = mk(0, 0, 0);
    double t = 0;
    int mi = 0, self = -1;
    if (!hit_is_tri(hs)) {
      const DSphere& S0 = g.spheres[hs.idx];
      t = hs.num / len2(d);
      const d3 P = o + muls(d, t);
      const d3 outward = divs(P - ld3(S0.c), S0.r);
      const bool front = dot(d, outward) < 0;
      N = front ? outward : neg(outward);
      mi = S0.mat;
      self = S0.obj;
    } else if constexpr (!kSph) {
      const DTri& T0 = g.tris[hs.idx];
      t = hs.num;
      const double w = 1.0 - hs.u - hs.v;
      const d3 n = ld3(T0.n);
      N = normalize((muls(n, w) + muls(n, hs.u)) + muls(n, hs.v));
      const bool front = dot(d, N) < 0;
      if (!front) N = neg(N);
      mi = T0.mat;
      self = T0.obj;
    }
    const DMat& M = p.mats[mi];
    ax += M.albedo[0];
    ay += M.albedo[1];
    az += M.albedo[2];
    nx += N.x;
    ny += N.y;
    nz += N.z;
    st += t;
    if (hits == 0) first = self;
    ++hits;
  }
  const double n = (double)p.spp;
  if (p.albedo) {
    p.albedo[(size_t)px * 3 + 0] = (float)(ax / n);
    p.albedo[(size_t)px * 3 + 1] = (float)(ay / n);
    p.albedo[(size_t)px * 3 + 2] = (float)(az / n);
  }
  if (p.normal) {
    p.normal[(size_t)px * 3 + 0] = (float)(nx / n);
    p.normal[(size_t)px * 3 + 1] = (float)(ny / n);
    p.normal[(size_t)px * 3 + 2] = (float)(nz / n);
  }
  if (p.depth) p.depth[px] = hits ? (float)(st / (double)hits) : __builtin_inff();
  if (p.coverage) p.coverage[px] = (float)((double)hits / n);
  if (p.object) p.object[px] = first;
}

// ---- specular-through feature buffers (rt_context_render_aov_spec_async,
// include/rt_api.h): the same pass with a chain of ideal
// mirror reflections behind each camera ray, up to max_bounces, ending at the
// first hit whose material is not followed.  No draw after the camera ray.

// The HitRecord of hit `hs` of ray (o, d), as aov_kernel above writes it, with
// the record's Point (sphere.go:47, triangle.go:69: o + d * T).  A helper of
// the chain's alone: aov_kernel keeps its own text and its code.
struct AovHit {
  d3 P, N;
  double t;
  int mi, self;
};
template <bool kSph>
__device__ __forceinline__ AovHit aov_hit_record(const Geo& g, d3 o, d3 d, const typename Kind<kSph>::H& hs) {
  AovHit r;
  r.P = r.N = mk(0, 0, 0);
  r.t = 0;
  r.mi = 0;
  r.self = -1;
  if (!hit_is_tri(hs)) {
    const DSphere& S0 = g.spheres[hs.idx];
    r.t = hs.num / len2(d);
    r.P = o + muls(d, r.t);
    const d3 outward = divs(r.P - ld3(S0.c), S0.r);
    const bool front = dot(d, outward) < 0;
    r.N = front ? outward : neg(outward);
    r.mi = S0.mat;
    r.self = S0.obj;
  } else if constexpr (!kSph) {
    const DTri& T0 = g.tris[hs.idx];
    r.t = hs.num;
    r.P = o + muls(d, r.t);
    const double w = 1.0 - hs.u - hs.v;
    const d3 n = ld3(T0.n);
    r.N = normalize((muls(n, w) + muls(n, hs.u)) + muls(n, hs.v));
    const bool front = dot(d, r.N) < 0;
    if (!front) r.N = neg(r.N);
    r.mi = T0.mat;
    r.self = T0.obj;
  }
  return r;
}

// followed: metal, shiny or perfectmirror with the clamped roughness within
// the bound (a NaN roughness compares false)
__device__ __forceinline__ bool aov_follows(const DMat& M, double max_roughness) {
  const int k = M.kind;
  return (k == RT_MAT_METAL || k == RT_MAT_SHINY || k == RT_MAT_PERFECTMIRROR) && M.roughness <= max_roughness;
}

template <bool kSph, bool kMix>
__global__ __launch_bounds__(64) void aov_spec_kernel(const AovSpecParams q) {
  typedef typename Kind<kSph>::H HitK;
  const AovParams& p = q.a;
  const unsigned px = blockIdx.x * 64u + threadIdx.x;  // y * W + x (W * H <= 2^29)
  if (px >= (unsigned)p.W * (unsigned)p.H) return;
  int* stack = reinterpret_cast<int*>(aov_lds) + threadIdx.x;
  const int y = (int)(px / (unsigned)p.W), x = (int)(px - (unsigned)y * (unsigned)p.W);
  const CamK ck = make_cam(p.seed_key, p.W, p.H, p.cf);
  Geo g = p.g;
  if constexpr (kSph) {
    g.nt = 0;
    g.nb = 0;
  }
  const typename Kind<kSph>::C all = cand_all<kSph>();
  Counters nc;  // (nothing counts here)
  double ax = 0, ay = 0, az = 0, nx = 0, ny = 0, nz = 0, st = 0;
  int hits = 0, first = -1, m = 0, sk = 0;  // sk: sumK, at most 16 * 2^24
  for (int s = 0; s < p.spp; ++s) {
    rt_rng rng;
    d3 o, d;
    camera_ray_c<false>(ck, p.cf, x, y, s, rng, o, d, nc);
    // the chain: one closest hit per ray; r stays the last existing hit's record
    AovHit r;
    double ca = 0, cb = 0, cc = 0, tt = 0;
    int k = -1;
    for (int j = 0;; ++j) {
      HitK hs;
      if (!closest_hit<false, kSph, kMix>(g, o, d, hs, stack, all, nc)) break;  // (j > 0: the last mirror is terminal)
      r = aov_hit_record<kSph>(g, o, d, hs);
      const DMat& M = p.mats[r.mi];
      const bool follow = aov_follows(M, q.max_roughness);
      if (j == 0) {
        ca = M.albedo[0];
        cb = M.albedo[1];
        cc = M.albedo[2];
        tt = r.t;
        if (follow) ++m;
      } else {
        ca *= M.albedo[0];
        cb *= M.albedo[1];
        cc *= M.albedo[2];
        tt += r.t;
      }
      k = j;
      if (!follow || j >= q.max_bounces) break;
      o = r.P;
      d = reflect(d, r.N);  // Scatter of a roughness-0 metal: not normalised, no perturbation
    }
    if (k < 0) continue;  // hit 0 does not exist
    ax += ca;
    ay += cb;
    az += cc;
    nx += r.N.x;
    ny += r.N.y;
    nz += r.N.z;
    st += tt;
    sk += k;
    if (hits == 0) first = r.self;
    ++hits;
  }
  const double n = (double)p.spp;
  if (p.albedo) {
    p.albedo[(size_t)px * 3 + 0] = (float)(ax / n);
    p.albedo[(size_t)px * 3 + 1] = (float)(ay / n);
    p.albedo[(size_t)px * 3 + 2] = (float)(az / n);
  }
  if (p.normal) {
    p.normal[(size_t)px * 3 + 0] = (float)(nx / n);
    p.normal[(size_t)px * 3 + 1] = (float)(ny / n);
    p.normal[(size_t)px * 3 + 2] = (float)(nz / n);
  }
  if (p.depth) p.depth[px] = hits ? (float)(st / (double)hits) : __builtin_inff();
  if (p.coverage) p.coverage[px] = (float)((double)hits / n);
  if (p.object) p.object[px] = first;
  if (q.specular) q.specular[px] = (float)((double)m / n);
  if (q.bounces) q.bounces[px] = (float)((double)sk / n);
}

int launch_aov_spec(const AovSpecParams& q, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const AovParams& p = q.a;
  const size_t npix = (size_t)p.W * (size_t)p.H;
  if (npix == 0) return hipSuccess;
  const dim3 g((unsigned)((npix + 63) / 64)), b(64);
  const size_t shmem = p.g.use_bvh ? sizeof(int) * (size_t)p.stack_depth * 64 : 0;
  if (p.g.use_bvh == 2)
    hipLaunchKernelGGL((aov_spec_kernel<false, true>), g, b, shmem, st, q);
  else if (p.g.nt == 0 && p.g.nb == 0)
    hipLaunchKernelGGL((aov_spec_kernel<true, false>), g, b, shmem, st, q);
  else
    hipLaunchKernelGGL((aov_spec_kernel<false, false>), g, b, shmem, st, q);
  return (int)hipGetLastError();
}

int launch_aov(const AovParams& p, void* stream) {
  hipStream_t st = (hipStream_t)stream;
  const size_t npix = (size_t)p.W * (size_t)p.H;
  if (npix == 0) return hipSuccess;
  const dim3 g((unsigned)((npix + 63) / 64)), b(64);
  const size_t shmem = p.g.use_bvh ? sizeof(int) * (size_t)p.stack_depth * 64 : 0;
  if (p.g.use_bvh == 2)
    hipLaunchKernelGGL((aov_kernel<false, true>), g, b, shmem, st, p);
  else if (p.g.nt == 0 && p.g.nb == 0)
    hipLaunchKernelGGL((aov_kernel<true, false>), g, b, shmem, st, p);
  else
    hipLaunchKernelGGL((aov_kernel<false, false>), g, b, shmem, st, p);
  return (int)hipGetLastError();
}

int preload_aov_kernels() {
  hipFuncAttributes a;
  const int e = (int)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(aov_kernel<true, false>));
  if (e != hipSuccess) return e;
  return (int)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(aov_spec_kernel<true, false>));
}

}  // namespace rtgo
