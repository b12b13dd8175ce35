// rt_blocks.h — what a render kernel reads from its arguments and writes to
// the image: the kernarg views (fresh, sfresh), work blocks, the per-phase
// scene view (Hot), shadow-cone rows, camera rays and the pixel write.
#pragma once
#include "rt_shadow.h"

namespace rtgo {

// ------------------------------------------------------------ kernel
// Kernel parameters that only the sample set-up and the epilogue need are
// re-read from the kernarg segment through a laundered pointer at each use
// (scalar-cache loads) instead of being held in SGPRs across the bounce
// loop: the loop's SGPR pressure otherwise spills uniform values into VGPR
// lanes and reloads them inside the intersection loops.
typedef const __attribute__((address_space(4))) KParams* KArg;  // constant (kernarg) address space
__device__ __forceinline__ KArg fresh() {
  // KParams is the kernel's only argument: it sits at offset 0 of the kernarg segment
  KArg k = (KArg)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(k));
  return k;
}

// This main workgroup's index: the grid's, less the tail helpers placed
// before it (KParams.tail_pos; launch_render)
__device__ __forceinline__ unsigned main_wg(KArg k) {
  const unsigned b = blockIdx.x;
  return (k->tail != nullptr && b >= (unsigned)k->tail_pos) ? b - (unsigned)k->tail_helpers : b;
}
// The launch's frame and block of this workgroup (KParams.nframes)
__device__ __forceinline__ int frame_of(KArg k) {
  return k->nframes > 1 ? (int)(main_wg(k) % (unsigned)k->nframes) : 0;
}
__device__ __forceinline__ int block_of(KArg k) {
  return k->nframes > 1 ? (int)(main_wg(k) / (unsigned)k->nframes) : (int)main_wg(k);
}
// a split pixel's radiance row / hit-bit words / sub-block counter in this frame's copy
__device__ __forceinline__ size_t split_index(KArg k, int slot) {
  return (size_t)frame_of(k) * (size_t)k->nsplit + (size_t)slot;
}

// ------------------------------------------------------------ work blocks
// A BLOCK is np consecutive row-major pixels of one 32x32 tile with all
// their spp samples: NB = np*spp sample ids, pixel-major (id = p*spp + s).
// One workgroup renders one block.  The host lists the blocks in its tile
// dispatch order (tiles sorted by estimated cost) and makes them small on
// tiles with geometry (schedule.cpp build_blocks).
struct BlockLoc {
  int lt, tile, tx, ty;  // local tile, global tile, tile coords
  int p0, np;            // first pixel (row-major in the tile), pixel count
  int s0, ns;            // samples [s0, s0+ns) of each pixel (all spp unless split)
  int slot, nsub;        // split pixel: its radiance slot row and number of sub-blocks (slot < 0: not split)
  bool black;            // kBlockBlack: no camera ray of the tile can hit anything
  unsigned long long ms, mt;  // primary masks: union over the block's pixels (fill_block_masks)
  unsigned long long live;    // its pixels whose own primary masks are not empty
};
__device__ __forceinline__ BlockLoc block_loc(KArg k, int b) {
  BlockLoc r;
  const int4 e = reinterpret_cast<const int4*>(k->blocks)[4 * b];
  const int4 f = reinterpret_cast<const int4*>(k->blocks)[4 * b + 1];
  const int4 g = reinterpret_cast<const int4*>(k->blocks)[4 * b + 2];
  const int4 l = reinterpret_cast<const int4*>(k->blocks)[4 * b + 3];
  r.ms = (unsigned long long)(uint32_t)g.x | ((unsigned long long)(uint32_t)g.y << 32);
  r.mt = (unsigned long long)(uint32_t)g.z | ((unsigned long long)(uint32_t)g.w << 32);
  r.live = (unsigned long long)(uint32_t)l.x | ((unsigned long long)(uint32_t)l.y << 32);
  r.lt = e.x;
  r.p0 = e.y;
  r.np = e.z;
  r.s0 = e.w;
  r.ns = f.x;
  r.slot = f.y;
  r.nsub = f.z;
  r.black = (f.w & kBlockBlack) != 0;
  r.tile = l.z;  // the block's global tile (sched_blocks: strided or a partition's list)
  r.tx = r.tile % k->tiles_x;
  r.ty = r.tile / k->tiles_x;
  return r;
}

// The scene view and switches of one phase of the bounce loop, re-read
// per phase (see fresh()).  Staged scenes address the LDS copy.
struct Hot {
  Geo g;
  const DMat* mats;
  const DLight* lights;
  const uint64_t* jump;
  int nl, max_depth;
  bool recursive, soft, masks;
};
extern __shared__ __attribute__((aligned(16))) unsigned char dyn_lds[];
template <bool kStage, bool kSph = false>
__device__ __forceinline__ Hot hot(KArg k) {
  Hot h;
  h.g = Geo{k->spheres, k->tris, k->boxes, k->bvh, k->ns, k->nt, k->use_bvh, k->nb};
  if constexpr (kSph) {  // launch_stream picks these kernels for nt == 0 && nb == 0 only
    h.g.nt = 0;
    h.g.nb = 0;
  }
  h.mats = k->mats;
  h.lights = k->lights;
  h.jump = k->jump;
  if constexpr (kStage) {
    const unsigned char* base = reinterpret_cast<const unsigned char*>(k->stage_src);
    h.g.spheres = reinterpret_cast<const DSphere*>(dyn_lds + (reinterpret_cast<const unsigned char*>(k->spheres) - base));
    h.g.tris = reinterpret_cast<const DTri*>(dyn_lds + (reinterpret_cast<const unsigned char*>(k->tris) - base));
    h.g.boxes = reinterpret_cast<const DBox*>(dyn_lds + (reinterpret_cast<const unsigned char*>(k->boxes) - base));
    h.mats = reinterpret_cast<const DMat*>(dyn_lds + (reinterpret_cast<const unsigned char*>(k->mats) - base));
    h.lights = reinterpret_cast<const DLight*>(dyn_lds + (reinterpret_cast<const unsigned char*>(k->lights) - base));
    const long jo = reinterpret_cast<const unsigned char*>(k->jump) - base;
    if (jo < k->stage_bytes) h.jump = reinterpret_cast<const uint64_t*>(dyn_lds + jo);
    // staged scenes are linear-scan scenes (set_scene stages only without a
    // BVH): the staged kernels carry no BVH traversal code at all
    h.g.use_bvh = 0;
  }
  h.nl = k->nl;
  h.max_depth = k->max_depth;
  h.recursive = k->recursive != 0;
  h.soft = k->soft != 0;
  h.masks = !h.g.use_bvh && h.g.ns <= 64 && h.g.nt <= 64;  // shadow-cone culling available
  return h;
}
template <bool kStage, bool kSph = false>
__device__ __forceinline__ Hot hot() {
  return hot<kStage, kSph>(fresh());
}

// Shadow-cone rows (the spheres-only stream kernels).  `row`
// is the lane's row of KParams::cone_rows_off for (light, self): the spheres
// that a hit on `self` can ever hold in its cone under that light, a superset
// of what in_cone admits for any P on it (scene_flat.cpp cone_rows), so the
// mask is cone_candidates' bit for bit.  A sphere in no active lane's row
// costs the wave one ballot and no in_cone.
__device__ __forceinline__ unsigned long long cone_row(KArg k, int li, int self) {
  const int off = k->cone_rows_off;
  if (off == 0) return ~0ull;
  return reinterpret_cast<const unsigned long long*>(dyn_lds + off)[li * k->ns + self];
}
__device__ __forceinline__ Kind<true>::C cone_candidates_rows(const Geo& p, d3 P, d3 N, bool front, int self, d3 ldir,
                                                              double ldist, unsigned long long row) {
  const bool sphere_out = front && dot(N, ldir) >= KC(0.1015);
  Kind<true>::C m{};
  for (int i = 0; i < p.ns; ++i) {
    const DSphere& S = p.spheres[i];
    const bool mine = ((row >> i) & 1) != 0 && !(sphere_out && S.obj == self && S.r > 0);
    if (__ballot(mine) == 0) continue;
    if (mine && in_cone(S.c, S.r, P, ldir, ldist)) m.s |= 1ull << i;
  }
  return m;
}

// Camera ray of sample s of pixel (x, y): tracePixel's jitter
// (renderer.go:155-156, the first two draws of the stream) and getRay
// (renderer.go:377-390).  Leaves `rng` after those two draws.  CamK holds
// the launch-uniform inputs; phase 1 loads it once per block (SGPRs), the
// shading loop rebuilds it from the kernarg segment where it needs it.
__device__ __forceinline__ CamK cam_k(KArg k) {
  return make_cam(k->frame_key[frame_of(k)], k->W, k->H, k->cf);
}
template <bool kCount>
__device__ __forceinline__ void camera_ray(KArg k, int x, int y, int s, rt_rng& rng, d3& o, d3& d, Counters& c) {
  camera_ray_c<kCount>(cam_k(k), k->cf, x, y, s, rng, o, d, c);
}

// One pixel's mean, tone map (renderer.go:348-367) and write, as the epilogue
// writes it: sum / spp (DivScalar(float64(samples))), float3 + RGBA8.
__device__ __forceinline__ void store_pixel(KArg k, int fr, size_t oi, double sx, double sy, double sz) {
  const double n = (double)k->spp_total;
  const double mx = sx / n, my = sy / n, mz = sz / n;
  float* const ol = k->frame_lin[fr];
  uint8_t* const orgba = k->frame_rgba[fr];
  if (ol) {
    ol[oi * 3 + 0] = (float)mx;
    ol[oi * 3 + 1] = (float)my;
    ol[oi * 3 + 2] = (float)mz;
  }
  if (orgba) *reinterpret_cast<uint32_t*>(orgba + oi * 4) = tonemap_rgba8(mx, my, mz);
}

// The stream kernel's part of its one argument (StreamKArgs: KParams first,
// so fresh() serves it too), re-read where it is used like KParams.
typedef const __attribute__((address_space(4))) StreamKArgs* SArg;
__device__ __forceinline__ SArg sfresh() {
  SArg k = (SArg)__builtin_amdgcn_kernarg_segment_ptr();
  asm volatile("" : "+s"(k));
  return k;
}

// (kSph) per lane: its path's throughput T, in LDS (render_body path_T; a
// function's array, so the other instantiations' LDS stays as it is)
__device__ __forceinline__ double (*tput_lds())[3] {
  __shared__ double tput[64][3];
  return tput;
}

// (render_body's ring, rt_body.h; here because the tail helpers' row_sum,
// rt_tail.h, loads its rows in chunks of it)
constexpr int kRound = 128;  // list entries shaded per round (LDS radiance slots)

}  // namespace rtgo
