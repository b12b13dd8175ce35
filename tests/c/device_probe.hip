// device_probe.hip — TEST INFRASTRUCTURE: the device functions of
// csrc/rt_device.h called one at a time (tests/test_gpu_probe.py).
//
// The kernels replace the reference's arithmetic in a dozen places with a
// cheaper form that is argued to give the same answer ("The
// shortcuts and what holds them").  A render decides such a shortcut only
// where one of its rays happens to land; here each one is a kernel of its own
// that runs the function on plain arrays, one lane per case, so a test can put
// it on the edges of its argument.
//
// Built by `make probe` into build/probe/librtprobe.so with the product's
// HIPFLAGS from rt_device.h / rt_internal.h as they are; never linked into
// librtgo.so.  Every kernel: one lane per case, every index checked against
// its count, no LDS, no atomics, no cross-lane operation; the only
// data-dependent loop is rand_in_unit_sphere's rejection loop (scatter).
//
// The host part flattens an rt_scene with the product's own flatten_scene /
// build_bvh (scene_flat.o, bvh.o, scene_json.o are linked in), so the records
// the functions read (DSphere, DTri, DBox, DMat, DBVHNode) are the product's.
#include <hip/hip_runtime.h>

#include <new>
#include <string>

#include "../../concurrent-raytracer-go_amd/csrc/rt_device.h"

namespace rtgo {
// (rt_api.cpp's is not linked: the host objects only report through it)
static thread_local std::string g_probe_error;
void set_error(const std::string& msg) { g_probe_error = msg; }
}  // namespace rtgo

using namespace rtgo;

namespace {

constexpr int kBlock = 256;

__device__ __forceinline__ int case_index() { return (int)(blockIdx.x * (unsigned)kBlock + threadIdx.x); }

// ---- div_by / refined_rcp: q = n / d as camera_ray_c forms u and v
__global__ void __launch_bounds__(kBlock) k_div(const double* n, const double* d, double* q, int count) {
  const int i = case_index();
  if (i >= count) return;
  q[i] = div_by(n[i], d[i], refined_rcp(d[i]));
}

// ---- root_out with approx_rcp, as closest_hit / any_hit call it
__global__ void __launch_bounds__(kBlock) k_root(const double* num, const double* a, const double* tmin,
                                                 const double* tmax, int32_t* out, int count) {
  const int i = case_index();
  if (i >= count) return;
  out[i] = root_out(num[i], a[i], approx_rcp(a[i]), tmin[i], tmax[i]) ? 1 : 0;
}

// ---- unit_ball_accept and the point rand_in_unit_sphere returns
__global__ void __launch_bounds__(kBlock) k_ball(const uint32_t* u, int32_t* acc, double* pt, int count) {
  const int i = case_index();
  if (i >= count) return;
  const uint32_t ux = u[3 * i], uy = u[3 * i + 1], uz = u[3 * i + 2];
  acc[i] = unit_ball_accept(ux, uy, uz) ? 1 : 0;
  const d3 p = unit_ball_point(ux, uy, uz);
  pt[3 * i] = p.x;
  pt[3 * i + 1] = p.y;
  pt[3 * i + 2] = p.z;
}

// ---- sphere_query: a and inv_a as closest_hit forms them; t = num / a
__global__ void __launch_bounds__(kBlock) k_sphere(const DSphere* spheres, int ns, const int32_t* idx, const double* o,
                                                   const double* d, const double* tmin, const double* tmax,
                                                   int32_t* which, double* t, int count) {
  const int i = case_index();
  if (i >= count) return;
  const int s = idx[i];
  which[i] = -1;
  t[i] = 0.0;
  if (s < 0 || s >= ns) return;
  const d3 ro = ld3(o + 3 * i), rd = ld3(d + 3 * i);
  const double a = len2(rd);
  double num = 0.0;
  const int w = sphere_query(spheres[s], ro, rd, a, approx_rcp(a), tmin[i], tmax[i], num);
  which[i] = w;
  if (w) t[i] = num / a;
}

// ---- tri_test
__global__ void __launch_bounds__(kBlock) k_tri(const DTri* tris, int nt, const int32_t* idx, const double* o,
                                                const double* d, const double* tmin, const double* tmax, int32_t* ok,
                                                double* tuv, int count) {
  const int i = case_index();
  if (i >= count) return;
  const int s = idx[i];
  ok[i] = -1;
  tuv[3 * i] = tuv[3 * i + 1] = tuv[3 * i + 2] = 0.0;
  if (s < 0 || s >= nt) return;
  double t = 0.0, u = 0.0, v = 0.0;
  const bool hit = tri_test(tris[s], ld3(o + 3 * i), ld3(d + 3 * i), tmin[i], tmax[i], t, u, v);
  ok[i] = hit ? 1 : 0;
  if (hit) {
    tuv[3 * i] = t;
    tuv[3 * i + 1] = u;
    tuv[3 * i + 2] = v;
  }
}

// ---- the slab tests of one (ray, node, cube box) case.  Bits of the answer:
//   1  box_hit with inv_dir              2  box_hit with inv_dir_fast
//   4  box_hit32, ray32 of inv_dir       8  box_hit32, ray32 of inv_dir_fast
//  16  ray_box with inv_dir (cases with a box; box < 0: none)
// the binary32 window is t_lo32(tmin), t_hi32(tmax) as in closest_hit.
__global__ void __launch_bounds__(kBlock) k_slab(const DBVHNode* nodes, int nn, const DBox* boxes, int nb,
                                                 const int32_t* node, const int32_t* box, const double* o,
                                                 const double* d, const double* tmin, const double* tmax,
                                                 int32_t* out, int count) {
  const int i = case_index();
  if (i >= count) return;
  const int k = node[i], b = box[i];
  out[i] = -1;
  if (k < 0 || k >= nn || b >= nb) return;
  const d3 ro = ld3(o + 3 * i), rd = ld3(d + 3 * i);
  const d3 id = inv_dir(rd), idf = inv_dir_fast(rd);
  const DBVHNode n = nodes[k];
  const float lo = t_lo32(tmin[i]), hi = t_hi32(tmax[i]);
  float tn;
  int r = 0;
  if (box_hit(n, ro, id, tmin[i], tmax[i])) r |= 1;
  if (box_hit(n, ro, idf, tmin[i], tmax[i])) r |= 2;
  if (box_hit32(n, ray32(ro, id), lo, hi, tn)) r |= 4;
  if (box_hit32(n, ray32(ro, idf), lo, hi, tn)) r |= 8;
  if (b >= 0 && ray_box(boxes[b], ro, id, tmin[i], tmax[i])) r |= 16;
  out[i] = r;
}

// ---- Go's scalar semantics.  out[10 i ..]: pow_n<5>(x), pow_n<2>(x), gmax0(x),
// gmin1_first(x), gmin_x1(x), clamp01(x), go_max2(x, y), go_min2(x, y),
// go_max2(y, x), go_min2(y, x); u8[i] = go_u8(x)
__global__ void __launch_bounds__(kBlock) k_scalar(const double* x, const double* y, double* out, uint32_t* u8,
                                                   int count) {
  const int i = case_index();
  if (i >= count) return;
  const double a = x[i], b = y[i];
  double* r = out + 10 * (size_t)i;
  r[0] = pow_n<5>(a);
  r[1] = pow_n<2>(a);
  r[2] = gmax0(a);
  r[3] = gmin1_first(a);
  r[4] = gmin_x1(a);
  r[5] = clamp01(a);
  r[6] = go_max2(a, b);
  r[7] = go_min2(a, b);
  r[8] = go_max2(b, a);
  r[9] = go_min2(b, a);
  u8[i] = go_u8(a);
}

// ---- tonemap_rgba8 of a pixel's mean radiance
__global__ void __launch_bounds__(kBlock) k_tonemap(const double* rgb, uint32_t* out, int count) {
  const int i = case_index();
  if (i >= count) return;
  out[i] = tonemap_rgba8(rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]);
}

// ---- scatter<false>, the product's instantiation; the stream's state after
// it tells how many draws it took
__global__ void __launch_bounds__(kBlock) k_scatter(const DMat* mats, int nm, const int32_t* mat, const double* d,
                                                    const double* N, const int32_t* front, const uint64_t* state,
                                                    int32_t* ok, double* out, uint64_t* state_out, int count) {
  const int i = case_index();
  if (i >= count) return;
  const int m = mat[i];
  ok[i] = -1;
  state_out[i] = 0;
  for (int k = 0; k < 6; ++k) out[6 * (size_t)i + k] = 0.0;
  if (m < 0 || m >= nm) return;
  rt_rng rng;
  rng.x = state[i];
  Counters c;
  const Scat r = scatter<false>(mats + m, ld3(d + 3 * i), ld3(N + 3 * i), front[i] != 0, rng, c);
  ok[i] = r.ok ? 1 : 0;
  double* w = out + 6 * (size_t)i;
  w[0] = r.nd.x;
  w[1] = r.nd.y;
  w[2] = r.nd.z;
  w[3] = r.A.x;
  w[4] = r.A.y;
  w[5] = r.A.z;
  state_out[i] = rng.x;
}

inline dim3 grid_of(int count) { return dim3((unsigned)((count + kBlock - 1) / kBlock)); }
inline int launched() { return (int)hipGetLastError(); }

}  // namespace

// Every launcher: device pointers, `count` cases, a hipStream_t; returns the
// launch's hipError_t (0 = hipSuccess), -1 for a bad argument.  count == 0 is
// a no-op.
#define PROBE_LAUNCH(kernel, ...)                                                        \
  do {                                                                                   \
    if (count < 0) return -1;                                                            \
    if (count == 0) return 0;                                                            \
    hipLaunchKernelGGL(kernel, grid_of(count), dim3(kBlock), 0, (hipStream_t)stream, __VA_ARGS__); \
    return launched();                                                                   \
  } while (0)

extern "C" {

int rtp_div(const double* n, const double* d, double* q, int count, void* stream) {
  PROBE_LAUNCH(k_div, n, d, q, count);
}
int rtp_root_out(const double* num, const double* a, const double* tmin, const double* tmax, int32_t* out, int count,
                 void* stream) {
  PROBE_LAUNCH(k_root, num, a, tmin, tmax, out, count);
}
int rtp_unit_ball(const uint32_t* u, int32_t* acc, double* pt, int count, void* stream) {
  PROBE_LAUNCH(k_ball, u, acc, pt, count);
}
int rtp_sphere_query(const void* spheres, int ns, const int32_t* idx, const double* o, const double* d,
                     const double* tmin, const double* tmax, int32_t* which, double* t, int count, void* stream) {
  PROBE_LAUNCH(k_sphere, (const DSphere*)spheres, ns, idx, o, d, tmin, tmax, which, t, count);
}
int rtp_tri_test(const void* tris, int nt, const int32_t* idx, const double* o, const double* d, const double* tmin,
                 const double* tmax, int32_t* ok, double* tuv, int count, void* stream) {
  PROBE_LAUNCH(k_tri, (const DTri*)tris, nt, idx, o, d, tmin, tmax, ok, tuv, count);
}
int rtp_slab(const void* nodes, int nn, const void* boxes, int nb, const int32_t* node, const int32_t* box,
             const double* o, const double* d, const double* tmin, const double* tmax, int32_t* out, int count,
             void* stream) {
  PROBE_LAUNCH(k_slab, (const DBVHNode*)nodes, nn, (const DBox*)boxes, nb, node, box, o, d, tmin, tmax, out, count);
}
int rtp_scalar(const double* x, const double* y, double* out, uint32_t* u8, int count, void* stream) {
  PROBE_LAUNCH(k_scalar, x, y, out, u8, count);
}
int rtp_tonemap(const double* rgb, uint32_t* out, int count, void* stream) {
  PROBE_LAUNCH(k_tonemap, rgb, out, count);
}
int rtp_scatter(const void* mats, int nm, const int32_t* mat, const double* d, const double* N, const int32_t* front,
                const uint64_t* state, int32_t* ok, double* out, uint64_t* state_out, int count, void* stream) {
  PROBE_LAUNCH(k_scatter, (const DMat*)mats, nm, mat, d, N, front, state, ok, out, state_out, count);
}

// ---- the product's records of a scene.  rtp_flatten: flatten_scene, then
// build_bvh(bins, leaf) when `tree` (0: the defaults); the handle owns host
// arrays.  rtp_array: array `which` (0 spheres, 1 triangles, 2 cube boxes,
// 3 materials, 4 tree nodes) as pointer, records and bytes per record.
void* rtp_flatten(const rt_scene* scene, int tree, int bins, int leaf) {
  if (!scene) return nullptr;
  FlatScene* fs = new (std::nothrow) FlatScene();
  if (!fs) return nullptr;
  flatten_scene(*scene, fs);
  if (tree) build_bvh(fs, bins, leaf);
  return fs;
}
void rtp_free(void* h) { delete (FlatScene*)h; }
int rtp_array(const void* h, int which, const void** data, int64_t* count, int64_t* stride) {
  const FlatScene* fs = (const FlatScene*)h;
  if (!fs || !data || !count || !stride) return -1;
  switch (which) {
    case 0: *data = fs->spheres.data(); *count = (int64_t)fs->spheres.size(); *stride = sizeof(DSphere); return 0;
    case 1: *data = fs->tris.data(); *count = (int64_t)fs->tris.size(); *stride = sizeof(DTri); return 0;
    case 2: *data = fs->boxes.data(); *count = (int64_t)fs->boxes.size(); *stride = sizeof(DBox); return 0;
    case 3: *data = fs->mats.data(); *count = (int64_t)fs->mats.size(); *stride = sizeof(DMat); return 0;
    case 4: *data = fs->bvh.data(); *count = (int64_t)fs->bvh.size(); *stride = sizeof(DBVHNode); return 0;
  }
  return -1;
}
int rtp_cube_leaf_bit() { return kCubeLeafBit; }

}  // extern "C"
