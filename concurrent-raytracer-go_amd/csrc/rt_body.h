// rt_body.h — render_body<V>, the one body of the gfx950 render kernels: the
// block kernels (rt_kernel.hip) and the stream kernels (rt_stream.hip).
//
// One launch renders every 32x32 tile (createRenderTasks,
// internal/renderer/renderer.go:398-436) that this rank owns.  Design
// (DESIGN.md §4):
//   the host cuts this rank's tiles into work BLOCKS (pixels of one tile x
//     a range of their samples, schedule.cpp), sized and ordered heaviest
//     first from a one-sample pilot render; one one-wave workgroup renders
//     one block;
//   a block runs in three phases (render_body below): every camera sample
//     of the block's live pixels gets its closest hit (misses end at once);
//     the hit samples form a list that the wave drains through a ring of LDS
//     radiance slots, a lane without a path taking the next entry, so
//     traceRay (renderer.go:165-227, unrolled) runs on dense waves even when
//     almost every camera ray misses; finished entries are summed per pixel
//     in sample order (tracePixel, renderer.go:150-163), divided by spp,
//     tone-mapped (toneMap, renderer.go:348-367) and written once (float3
//     linear radiance + RGBA8);
//   per bounce and light, the 16 jittered shadow rays (calculateSmartShadow,
//     renderer.go:299-331) are produced in a wave-converged section: rays of
//     many owner lanes go through an LDS queue and are traced on full waves
//     (soft_queue); when only a few lanes need them, all 64 lanes evaluate
//     one owner's rejection tries in parallel (PCG jump-ahead,
//     include/rt_rng.h, soft_coop) -- same draws, same rays, same result as
//     the sequential loop; when few lanes still run paths, the idle lanes
//     split the closest-hit and cone scans of the others (wide mode).
// Large sphere scenes (a BVH) take the wavefront path instead
// (rt_wavefront.hip) unless rt_tuning.path asks for the megakernel.
// Small linear-scan scenes are staged into LDS by every workgroup; large
// sphere scenes use a BVH (bvh.cpp) with per-lane LDS stacks.  Primitives
// that provably cannot be hit (tile frustum / shadow cone tests with wide
// margins) are skipped; everything else gets the reference's exact test.
// All path arithmetic is binary64 in the reference's order, compiled with
// -ffp-contract=off, so every decision (hit / miss, root choice, rejection
// test, reflect vs refract) is bit-identical to the oracle's.  Divisions that
// only feed range tests are filtered by a reciprocal multiply with a 2^-40
// relative margin; the exact IEEE division runs whenever the filter cannot
// decide.
//
// Map of the render kernels' one body (render_body<V>, V a variant type that
// names its switches: BlockBody<..>, TailBody, Stream..Body):
//   phase 1 (visibility) and the hit-list scan    inline in render_body
//   the hit list, entry -> sample id              HitList::entry_id
//   phase 2, a pass's refill                      ring_low, resolve_entries, block_entry;
//                                                 the stream kernel: stream_claim_chunk, stream_entry
//                                                 (stream_decode, rt_internal.h; stream_cam_stage, stream_cam)
//   the tail export of pass 0                     tail_reserve, tail_pixel_row, the rest inline (next to
//                                                 them: tail_helper; rt_tail.h)
//   closest hit, lighting, soft shadows, scatter  closest_hit, scatter (rt_device.h); closest_wide,
//                                                 cone_candidates / cone_wide, shadow_blocked, soft_coop,
//                                                 soft_queue (rt_shadow.h)
//   kernel arguments, blocks, the pixel write     fresh / sfresh, block_loc, hot, store_pixel (rt_blocks.h)
//   the lone-path form (RT_SOLO builds)           solo_path (rt_solo.h)
//   the pilot's path lengths                      pilot_record
//   phase 3 (final)                               inline, tail_rows_give_back (rt_tail.h), reduce_counters
//   RT_WG_TIMING clocks and records               WgClock (rt_wg_clock.h)
// This header includes the others in the order their definitions had in the
// one file they were cut from; the kernels that instantiate render_body are in
// rt_kernel.hip and rt_stream.hip, which must see the same RT_* values.
#pragma once
#include "rt_shadow.h"
#include "rt_blocks.h"
#include "rt_wg_clock.h"
#include "rt_solo.h"
#include "rt_tail.h"

// waves per SIMD of render_kernel: measured best of 2/3/4 (4 spills the FP64 path state)
#ifndef RT_WAVES_PER_SIMD
#define RT_WAVES_PER_SIMD 3
#endif
// (measurement switch: cone_wide's helpers off)
#ifndef RT_CONE_HELPERS  // (not RT_CONE_WIDE: rt_internal.h's candidate-list width)
#define RT_CONE_HELPERS 1
#endif

namespace rtgo {

// Render kernel: one wave (64 lanes) per block, three phases.  A one-wave
// workgroup needs no barriers and leaves the CU as soon as its own work is
// done (4-wave workgroups held their slots until their slowest wave ended).
//   1 VISIBILITY - the lanes generate the block's NB camera rays (NB/64
//       each) and ask only "does it hit anything?" (an any-hit query over
//       [0.001, +inf), with the tile's frustum candidates).  A miss is black
//       (renderer.go:170-173) and is finished; a hit sets the sample's bit.
//       At 800x600x100 97% of the camera rays end here.
//   2 SHADE - the hit samples, ascending, form a list that the wave drains
//       through a ring of kRound LDS radiance slots: a lane without a path
//       takes the next entry, rebuilds its camera ray and runs the path
//       (traceRay, renderer.go:165-227, unrolled: closest hit, direct
//       lighting with hard + soft shadows, scatter) to its end, storing the
//       radiance in the entry's slot.  Shading runs on dense waves instead
//       of on the ~3% of lanes whose camera ray hit.  Soft shadows of the
//       few paths still running at the end run cooperatively (soft_coop).
//   3 RESOLVE - whenever the ring is full, every pixel adds the finished
//       entries before the earliest running path to its running sum, in
//       sample order (misses add +0: the same sum as tracePixel,
//       renderer.go:150-163, bit for bit); at the end the sum is divided by
//       spp, tone-mapped (renderer.go:348-367) and written once (float3
//       linear + RGBA8).

// second closest-hit pass of a shade iteration (render_kernel): taken when at
// least this many lanes are free after the first (0: never).  Measured (r05,
// K = 100 throughput, two rounds each): never 148.8 k, 4 155.6 k, 8 156.2 k,
// 16 157.5 k Mrays/s; one frame at a time unchanged (0.74-0.75 ms)
#ifndef RT_REFILL2_MIN
#define RT_REFILL2_MIN 16
#endif
constexpr int kRefill2Min = RT_REFILL2_MIN;

// The block's hit list: its hit samples' ids, ascending, as a view over
// render_body's hit bits (`bits`, one per sample id, set by phase 1) and the
// list offset of each bit word (`off`; off[nwords] = the number of hits).
template <int kWords>
struct HitList {
  uint32_t (&bits)[kWords];
  int (&off)[kWords + 1];
  const int& nwords;
  // sample id (pixel * ns + sample - s0) of hit-list entry e < off[nwords]: the bit
  // word holding it (the last word whose list offset is <= e, by binary
  // search over off), then the (e - offset)-th set bit of that word.  No
  // materialized list: its 2 KB of LDS cost occupancy.
  __device__ __forceinline__ int entry_id(int e) const {
    int w = 0;
    for (int step = 16; step; step >>= 1)
      if (w + step < nwords && off[w + step] <= e) w += step;
    uint32_t word = bits[w];
    int k = e - off[w], pos = 0;
    for (int sh = 16; sh; sh >>= 1) {
      const int n = __popc(word & ((1u << sh) - 1u));
      if (k >= n) {
        k -= n;
        word >>= sh;
        pos += sh;
      }
    }
    return w * 32 + pos;
  }
};
// (kPilot, a measuring render) a path of `depth + 1` bounces ended: its
// pixel's longest path and its bounces
template <int kWords>
__device__ __forceinline__ void pilot_record(const HitList<kWords>& hl, int entry, int depth) {
  KArg k = fresh();
  const BlockLoc loc = block_loc(k, block_of(k));
  const size_t px = (size_t)loc.lt * 1024 + loc.p0 + hl.entry_id(entry) / loc.ns;
  atomicMax(k->work_max + px, (unsigned)depth + 1u);
  atomicAdd(k->work_sum + px, (unsigned)depth + 1u);
}

// ------------------------------------------------------------ render_body's phases
// (each inlined into render_body, which declares the LDS arrays they work on
// and keeps the path state; DESIGN.md §4.1 maps the phases to these names)
//
// Every function here (and HitList, pilot_record above; tail_reserve,
// tail_pixel_row and tail_rows_give_back, rt_tail.h) was cut out of render_body under one rule: the
// render kernels (then 22, in one file) keep their instructions and registers, bit for bit
// (make isa + scripts/cmp_kernels.py against the commit before, the product
// build and the cross-lane checking build).  What that rule allowed, for the
// next cut:
//   - a path-state variable of render_body whose address was never taken
//     (alive, entry, depth, T, next, resolved, qbeg, qend, dry, blk) goes in
//     BY VALUE and comes back as the RETURN value; handed over by reference
//     it is no longer promoted to registers before the inlining, and the
//     kernels came out with other registers and spill slots.  rng, o, d, c
//     and the hit selection already went to helpers by reference and may;
//   - a `for` loop that stands before the pass loop cannot leave
//     render_body: render_kernel_tail carries the compiler's number of the
//     pass loop's exit as an immediate (s_mov_b32 s10, 16), and every loop
//     moved out before it renumbers it.
// Seams tried and left inline for that reason, each alone against the parent
// (kernels that differed; lines of their disassembly):
//   LDS staging of the scene prefix   render_kernel<0,1,0,0>, <0,1,1,0>: 14 of 10875 / 11281
//                                     (SGPR spill lanes renumbered); render_kernel_tail: 4 (the immediate)
//   phase 1, visibility               7 block kernels: 4 .. 187 lines (spill lanes, scratch stores
//                                     reordered); render_kernel_tail: 4 (the immediate)
//   the hit-list scan                 render_kernel<1,0,0,0>: 170 of 15954 (scratch stores reordered);
//                                     render_kernel_tail: 9 (the immediate, two VGPRs swapped)
//   the stream claim as one function  the 4 stream kernels: 5164 .. 6841 lines (registers)
//   the ring's refill as one function render_kernel_tail and the 4 stream kernels: all lines; 11
//                                     kernels with other VGPR / spill counts
//   the tail export as one function,  render_kernel_tail: 16596 .. 18754 of 20406 lines (registers;
//   per path, or its record's store   same VGPRs, SGPRs and scratch)
//   the hit record from HitK          13 kernels, 9312 .. 18680 lines; 10 with other register counts
//                                     (by reference, by value and as a returned struct alike)
//   the split pixel's last-finisher   9 block kernels: 1 line (s_and_b64's operands swapped), or all
//   sum, the pixel write              lines; 8 block kernels: 2 lines (two ds_reads swapped)
// The per-light lighting body and scatter-and-combine rest on that state
// (D, P, N, shade, fin, o, d, depth, T, L) throughout and were not cut.

// ---- phase 3, as the ring moves on: entries [a, b) of the hit list (all
// finished, their radiance in their ring slots) are added to their pixels'
// sums in order; a split pixel's block stores them in its radiance slot row
// instead (and a pixel with exported paths, kTail, in its tail row)
template <bool kTail, int kWords, int kSlots, int kPix, int kRows, int kMarks>
__device__ __forceinline__ void resolve_entries(const HitList<kWords>& hl, const int& nh, const BlockLoc& blk,
                                                double (&slot)[kSlots][3], double (&psum)[kPix][3], int (&prow)[kRows],
                                                short (&pk0)[kRows], uint32_t (&xm)[kMarks], int a, int b) {
  // the lane id laundered through a volatile move: keeps this rarely run
  // code's lane-dependent addresses from being hoisted out of the shading
  // loop (they would occupy registers, or scratch, for the whole loop)
  int lane;
  asm volatile("v_mov_b32 %0, %1" : "=v"(lane) : "v"((int)threadIdx.x));
  if (blk.slot >= 0) {
    KArg k = fresh();
    double* row = k->split_rad + split_index(k, blk.slot) * k->spp * 3;
    uint32_t* hw = k->split_hits + split_index(k, blk.slot) * ((k->spp + 31) >> 5);
    for (int e = a + lane; e < b; e += 64) {
      const int s = blk.s0 + hl.entry_id(e);  // one pixel: id = sample - s0
      const int q = e & (kRound - 1);
      if constexpr (kTail) {
        if ((xm[q >> 5] >> (q & 31)) & 1u) continue;  // exported: its helper writes the sample
      }
      if constexpr (kTail) {  // (written through: read sc1 by the pixel's last contributor, maybe a helper)
        st_wtd(row + 3 * s + 0, slot[q][0]);
        st_wtd(row + 3 * s + 1, slot[q][1]);
        st_wtd(row + 3 * s + 2, slot[q][2]);
      } else {  // (combined in L2, written back by the release fence below)
        row[3 * s + 0] = slot[q][0];
        row[3 * s + 1] = slot[q][1];
        row[3 * s + 2] = slot[q][2];
      }
      atomicOr(hw + (s >> 5), 1u << (s & 31));
    }
  } else {
    const int P = blk.np, spp = blk.ns;
    if (lane < P) {
      const int a0 = lane * spp, a1 = a0 + spp;
      int e0 = hl.off[a0 >> 5] + __popc(hl.bits[a0 >> 5] & ((1u << (a0 & 31)) - 1u));
      int e1 = (a1 >> 5) < hl.nwords ? hl.off[a1 >> 5] + __popc(hl.bits[a1 >> 5] & ((1u << (a1 & 31)) - 1u)) : nh;
      e0 = max(e0, a);
      e1 = min(e1, b);
      bool rowed = false;
      if constexpr (kTail) rowed = prow[lane] >= 0;
      if (rowed) {
        // a pixel with exported paths (tail helpers): samples before its
        // first exported one go to its running sum as below, the later
        // ones (the exported ones aside: their helpers write them) to its
        // row, which the pixel's last contributor sums in order
        KArg k = fresh();
        const int r = prow[lane], k0 = pk0[lane], bw = (k->spp_total + 31) >> 5;
        double* row = k->tail_rows + (size_t)r * k->spp_total * 3;
        uint32_t* hw = k->tail_bits + (size_t)r * bw;
        double ax = psum[lane][0], ay = psum[lane][1], az = psum[lane][2];
        for (int e = e0; e < e1; ++e) {
          const int q = e & (kRound - 1);
          if ((xm[q >> 5] >> (q & 31)) & 1u) continue;
          const int sl = hl.entry_id(e) - a0;
          if (sl < k0) {
            ax += slot[q][0];
            ay += slot[q][1];
            az += slot[q][2];
          } else {  // (written through: the row's last contributor reads it sc1)
            st_wtd(row + 3 * sl + 0, slot[q][0]);
            st_wtd(row + 3 * sl + 1, slot[q][1]);
            st_wtd(row + 3 * sl + 2, slot[q][2]);
            atomicOr(hw + (sl >> 5), 1u << (sl & 31));
          }
        }
        psum[lane][0] = ax;
        psum[lane][1] = ay;
        psum[lane][2] = az;
      } else if (e0 < e1) {
        double ax = psum[lane][0], ay = psum[lane][1], az = psum[lane][2];
        for (int e = e0; e < e1; ++e) {
          const int q = e & (kRound - 1);
          ax += slot[q][0];
          ay += slot[q][1];
          az += slot[q][2];
        }
        psum[lane][0] = ax;
        psum[lane][1] = ay;
        psum[lane][2] = az;
      }
    }
  }
}

// ---- (kStream) the queue claim: the next chunk of the launch-wide queue,
// [x, y) (empty: the cursor is past the last entry).  The wave claims entries
// a chunk at a time (one relaxed add by one lane on the launch's cursor: a
// claim per entry would put ~0.9 M adds per headline frame on one address).
__device__ __forceinline__ uint2 stream_claim_chunk() {
  const SArg sk = sfresh();
  unsigned v = 0;
  if (lane_now() == 0)
    v = __hip_atomic_fetch_add(sk->s.cursor, (unsigned)sk->s.chunk, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  v = __builtin_amdgcn_readfirstlane(v);
  // (the cursor stays below 2^32: total < 2^31, and every wave adds
  // at most one chunk of <= 2^16 entries past the end)
  return make_uint2(min(v, sk->s.total), min(v + (unsigned)sk->s.chunk, sk->s.total));
}
// ... and the set-up of queue entry e: its camera ray and soft-shadow key
// exactly as the block kernel's refill builds them (kBase: the frame's sample
// sample_base + s, a progression's add); returns its row.
// kCams (a camera sequence): the entry's frame shoots from its
// own CamFrame, row frame0 + fl of the launch's table in device memory (one
// load per lane: with order 1 neighbouring lanes hold different frames); only
// here, at entry set-up -- nothing after the camera ray reads a camera.
// The decode of e is stream_decode (rt_internal.h): two multiply-highs by the
// magic numbers render_stream put into StreamParams::dec, exact for every
// e < 2^31.  The launch's CamK comes from LDS (stream_cam_lds below) unless
// every frame has a camera of its own.
//
// (not kCams) The launch-uniform CamK, all but its key: make_cam's values,
// computed once per wave ahead of the loop (stream_cam_stage, before the
// barrier that ends the staging) and read back per entry set-up -- the same
// operations in the same order on the same inputs, so the same bits, without
// the two refined reciprocals, the conversions and the corner per refill and
// without a VGPR across the loop.  A function's array, as tput_lds.
constexpr int kCamLds = 7;  // dW, dH, rW, rH, llcx, llcy, llcz
__device__ __forceinline__ double* stream_cam_lds() {
  __shared__ double camk[kCamLds];
  return camk;
}
__device__ __forceinline__ void stream_cam_stage() {
  const SArg sk = sfresh();
  const CamK ck = make_cam(0, sk->k.W, sk->k.H, sk->k.cf);
  if (threadIdx.x == 0) {
    double* c = stream_cam_lds();
    c[0] = ck.dW;
    c[1] = ck.dH;
    c[2] = ck.rW;
    c[3] = ck.rH;
    c[4] = ck.llcx;
    c[5] = ck.llcy;
    c[6] = ck.llcz;
  }
}
__device__ __forceinline__ CamK stream_cam(uint64_t fkey) {
  const SArg sk = sfresh();
  const double* c = stream_cam_lds();
  CamK r;
  r.key = fkey;
  r.W = (uint32_t)sk->k.W;
  r.lookat = sk->k.cf.model;
  r.dW = c[0];
  r.dH = c[1];
  r.rW = c[2];
  r.rH = c[3];
  r.llcx = c[4];
  r.llcy = c[5];
  r.llcz = c[6];
  r.vw = sk->k.cf.h[0];
  r.ox = sk->k.cf.o[0];
  r.oy = sk->k.cf.o[1];
  r.oz = sk->k.cf.o[2];
  return r;
}
template <bool kBase, bool kCams>
__device__ __forceinline__ int stream_entry(unsigned e, rt_rng& rng, d3& o, d3& d, uint64_t (&skey)[64]) {
  const SArg sk = sfresh();
  const unsigned spp = (unsigned)sk->k.spp, nlive = (unsigned)sk->s.nlive;
  const StreamEntry en = stream_decode(sk->s.dec, sk->s.order, e);
  const unsigned fl = en.fl, i = en.i, s = en.s;
  const int4 it = reinterpret_cast<const int4*>(sk->s.live)[i];
  const uint64_t fkey = sk->k.frame_key[sk->s.frame0 + (int)fl];
  Counters nc;
  const unsigned fs = kBase ? (unsigned)sk->k.sample_base + s : s;
  if constexpr (kCams) {
    const CamFrame& cf = sk->s.cams[sk->s.frame0 + (int)fl];
    camera_ray_c<false>(make_cam(fkey, sk->k.W, sk->k.H, cf), cf, it.x, it.y, (int)fs, rng, o, d, nc);
  } else {
    camera_ray_c<false>(stream_cam(fkey), sk->k.cf, it.x, it.y, (int)fs, rng, o, d, nc);
  }
  skey[lane_now()] = rt_soft_key(fkey, (uint32_t)it.y * (uint32_t)sk->k.W + (uint32_t)it.x, (uint32_t)fs);
  return (int)((fl * spp + s) * nlive + i);
}
// ---- the block ring: the earliest entry still running (a wave-wide min over
// the live lanes: swizzles within each half-wave, then the two halves' lane 0)
__device__ __forceinline__ int ring_low(bool alive, int entry, int next) {
  int lo = alive ? entry : next;
  lo = min(lo, __builtin_amdgcn_ds_swizzle(lo, 0x1F | (16 << 10)));
  lo = min(lo, __builtin_amdgcn_ds_swizzle(lo, 0x1F | (8 << 10)));
  lo = min(lo, __builtin_amdgcn_ds_swizzle(lo, 0x1F | (4 << 10)));
  lo = min(lo, __builtin_amdgcn_ds_swizzle(lo, 0x1F | (2 << 10)));
  lo = min(lo, __builtin_amdgcn_ds_swizzle(lo, 0x1F | (1 << 10)));
  return min(__builtin_amdgcn_readlane(lo, 0), __builtin_amdgcn_readlane(lo, 32));
}
// ... and the set-up of hit-list entry e: its camera ray (it hits: phase 1
// found a hit for it) and soft-shadow key
template <int kWords>
__device__ __forceinline__ void block_entry(const HitList<kWords> hl, int e, rt_rng& rng, d3& o, d3& d, uint64_t (&skey)[64]) {
  KArg k = fresh();
  const BlockLoc loc = block_loc(k, block_of(k));
  const int id = hl.entry_id(e), ns = loc.ns;
  const int p = id / ns, s = k->sample_base + loc.s0 + id - p * ns;
  const int tp = loc.p0 + p;
  Counters nc;  // phase 1 counted this camera ray and its draws
  const int px = loc.tx * 32 + (tp & 31), py = loc.ty * 32 + (tp >> 5);
  camera_ray<false>(k, px, py, s, rng, o, d, nc);
  skey[lane_now()] = rt_soft_key(k->frame_key[frame_of(k)], (uint32_t)py * (uint32_t)k->W + (uint32_t)px, (uint32_t)s);
}

// (kCount) the block's counters: wave reduction, then one atomic per counter
__device__ __forceinline__ void reduce_counters(KArg k, int lane3, Counters c, Counters culled) {
  for (int i = 0; i < 2 * kCounters; ++i) {
    unsigned long long v = i < kCounters ? c.v[i] : culled.v[i - kCounters];
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    if (lane3 == 0) atomicAdd(&k->counts[i], v);
  }
}

// kStream (render_stream_kernel): no blocks, no visibility
// phase, no ring and no resolve -- the wave stages the scene once and then
// takes entries (frame, live pixel, sample) off the launch-wide queue for as
// long as there are any, with the SAME bounce code; a path's running L lives
// in its lane's slot, and its final value goes to its row in global memory
// (resolve_rows_kernel sums the rows).  The block-only LDS arrays shrink to
// one element there.  kBase (render_stream_base_kernel): entry
// sample s is the frame's sample sample_base + s (a progression's later adds);
// an instantiation of its own, so the product stream kernel keeps its code.
// kSph (render_stream_sph_kernel and its kBase twin): the
// launch's scene has no triangle and no cube, which is every scene the auto
// rule streams; the bounce code carries no triangle or cube test, mask, hit
// field or select (Kind<kSph>).  The other instantiations keep their code.
//
// A build of render_body is named by a variant type: the switches as named
// members, one variant per kernel below.
struct BodySwitches {  // (the defaults: a variant names only what it turns on)
  static constexpr bool count = false;   // work counters (rt_counts)
  static constexpr bool stage = false;   // the scene prefix staged into LDS
  static constexpr bool pilot = false;   // a measuring render: per-pixel path lengths
  static constexpr bool sky = false;     // a miss returns the opted-in sky
  static constexpr bool tail = false;    // exports its last long paths to tail helpers
  static constexpr bool stream = false;  // drains the launch-wide entry queue
  static constexpr bool base = false;    // (stream) entry samples start at sample_base
  static constexpr bool sph = false;     // (stream) the scene is spheres alone
  static constexpr bool cams = false;    // (stream) every frame of the launch has a camera of its own
  static constexpr bool mix = false;     // the BVH has leaves of cubes (bvh.cpp; KParams.use_bvh == 2)
};
template <bool kCount, bool kStage, bool kPilot, bool kSky>
struct BlockBody : BodySwitches {  // render_kernel<kCount, kStage, kPilot, kSky>
  static constexpr bool count = kCount, stage = kStage, pilot = kPilot, sky = kSky;
};
template <bool kCount, bool kPilot, bool kSky>
struct MixBody : BlockBody<kCount, false, kPilot, kSky> {  // render_kernel_mix<kCount, kPilot, kSky>
  static constexpr bool mix = true;
};
struct TailBody : BodySwitches {  // render_kernel_tail
  static constexpr bool stage = true, tail = true;
};
struct StreamBody : BodySwitches {  // render_stream_kernel
  static constexpr bool stage = true, stream = true;
};
struct StreamBaseBody : StreamBody {  // render_stream_base_kernel
  static constexpr bool base = true;
};
struct StreamSphBody : StreamBody {  // render_stream_sph_kernel
  static constexpr bool sph = true;
};
struct StreamSphBaseBody : StreamSphBody {  // render_stream_sph_base_kernel
  static constexpr bool base = true;
};
struct StreamCamsBody : StreamBody {  // render_stream_cams_kernel
  static constexpr bool cams = true;
};
struct StreamSphCamsBody : StreamSphBody {  // render_stream_sph_cams_kernel
  static constexpr bool cams = true;
};
template <class V>
constexpr bool body_variant_ok() {
  static_assert(!V::stream || (V::stage && !V::count && !V::pilot && !V::sky && !V::tail), "the stream kernel is the staged product body");
  static_assert(!V::sph || V::stream, "spheres-only is a build of the stream kernel");
  static_assert(!V::cams || (V::stream && !V::base), "a camera sequence is a streamed launch, never a progression's add");
  static_assert(!V::mix || (!V::stage && !V::stream && !V::tail), "a BVH scene is not staged");
  return true;
}

template <class V>
__device__ __forceinline__ void render_body(const KParams& pk) {
  static_assert(body_variant_ok<V>(), "");
  constexpr bool kCount = V::count, kStage = V::stage, kPilot = V::pilot, kSky = V::sky, kStream = V::stream,
                 kBase = V::base, kSph = V::sph, kMix = V::mix, kCams = V::cams;
  typedef typename Kind<kSph>::C CandK;
  typedef typename Kind<kSph>::H HitK;
  __shared__ uint32_t hbits[kStream ? 1 : kMaxBlockSamples / 32];  // hit samples of the block
  __shared__ int hoff[kStream ? 2 : kMaxBlockSamples / 32 + 1];    // list offset of each bit word; [words] = #hits
  __shared__ double slot[kStream ? 64 : kRound][3];  // radiance of the round's entries (kStream: of each lane's path)
  __shared__ double psum[kStream ? 1 : 64][3];       // per pixel: running sum over samples
  __shared__ uint8_t lpix[kStream ? 1 : 64];         // phase 1: the block's live pixels
  __shared__ uint64_t skey[64];                      // per lane: its path's soft-shadow key (rt_soft_key, spec v4)
  // dynamic LDS (dyn_lds): [staged scene prefix (kStage)][BVH stack (stack_depth x 64 ints)]
  // tail helpers: render_kernel_tail exports a block's last
  // few long paths to the helpers past its main blocks.  The product kernel
  // has none of that code (compiled in but unused it cost 2-3 % one frame,
  // 1.5 % batched: r06 A/B)
  constexpr bool kTail = V::tail && kStage && !kCount && !kPilot && !kSky;

  const int lane = threadIdx.x;
  int* stack = reinterpret_cast<int*>(dyn_lds + pk.stack_off) + lane;
  if constexpr (kTail) {
    if (pk.tail != nullptr && blockIdx.x - (unsigned)pk.tail_pos < (unsigned)pk.tail_helpers) {
      // a tail helper (launch_render adds them only with pk.tail set)
      // (the staging loop, here and below, stays inline: "render_body's phases")
      const uint4* __restrict__ src = reinterpret_cast<const uint4*>(pk.stage_src);
      uint4* dst = reinterpret_cast<uint4*>(dyn_lds);
      for (int i = lane; i < pk.stage_bytes / 16; i += 64) dst[i] = src[i];
      __syncthreads();
      tail_helper(fresh(), stack, slot);
      return;
    }
  }
  // a row pixel (tail helpers): its dynamic row and first row sample (-1: none)
  __shared__ int prow[kTail ? 64 : 1];
  __shared__ short pk0[kTail ? 64 : 1];
  __shared__ uint32_t xm[kTail ? kRound / 32 : 1];  // ring slots whose path was exported
  if constexpr (kTail) {
    prow[lane] = -1;
    if (lane < kRound / 32) xm[lane] = 0u;
  }
  const BlockLoc blk = kStream ? BlockLoc{} : block_loc(fresh(), block_of(fresh()));
  // a black block (up to 64 pixels x spp samples) sets no hit bits
  const int nwords = blk.black ? 0 : (blk.np * blk.ns + 31) >> 5;
  if (lane < nwords) hbits[lane] = 0;
  if constexpr (!kStream) {
    // a later sample pass continues each pixel's running sum (acc_mode bit 0)
    double a0 = 0, a1 = 0, a2 = 0;
    if ((pk.acc_mode & 1) && blk.slot < 0 && lane < blk.np && blk.p0 + lane < 1024) {
      const double* a = pk.acc + ((size_t)blk.lt * 1024 + blk.p0 + lane) * 3;
      a0 = a[0];
      a1 = a[1];
      a2 = a[2];
    }
    psum[lane][0] = a0;
    psum[lane][1] = a1;
    psum[lane][2] = a2;
  }
  if constexpr (kStage) {
    // LDS-staged scene primitives: spheres | triangles | boxes | materials |
    // lights [| jump table] (one contiguous prefix of the device scene buffer), so the
    // divergent per-lane reads of the shadow / scatter code hit LDS instead
    // of L1/L2 (measured: 55% of wave time in memory waits without it)
    const uint4* __restrict__ src = reinterpret_cast<const uint4*>(pk.stage_src);
    uint4* dst = reinterpret_cast<uint4*>(dyn_lds);
    for (int i = lane; i < pk.stage_bytes / 16; i += 64) dst[i] = src[i];
  }
  if constexpr (kStream && !kCams) stream_cam_stage();  // (stream_entry reads it: behind the barrier)
  __syncthreads();

  Counters c, culled;
  if constexpr (kCount) {
    for (int i = 0; i < kCounters; ++i) c.v[i] = culled.v[i] = 0;
  }
  WgClock clk;
  clk.start(lane);
  const CandK all = cand_all<kSph>();

  // ---- phase 1: visibility of the block's camera rays
  // (inline, like the scan after it: a loop before the pass loop cannot leave
  // this function, see "render_body's phases")
  if constexpr (!kStream) {
    // everything the loop needs is loaded once, before it (wave-uniform:
    // SGPRs); re-reading the kernarg segment inside the loop put scalar
    // load round trips on every iteration
    KArg k = fresh();
    const BlockLoc loc = block_loc(k, block_of(k));
    const int NB = loc.np * loc.ns, ns = loc.ns;
    // primary-ray frustum culling (host-computed per pixel, schedule.cpp):
    // only primitives whose bounding sphere meets the cone of a pixel's
    // camera rays can be hit by them.  A pixel with no candidate is black
    // (every sample misses, renderer.go:170-173, and adds +0): its samples
    // are not traced.  The others are tested against the union of the
    // block's pixel masks.  (The counting variant walks every sample, so the
    // path counts stay the reference's.)
    Cand prim = all;
    unsigned long long pxlive = loc.np >= 64 ? ~0ull : (1ull << loc.np) - 1ull;
    if (k->tile_masks) {
      prim = Cand{loc.ms, loc.mt};
      pxlive = loc.live;
    }
    // compact list of the live pixels (block-local indices)
    if (lane < loc.np && ((pxlive >> lane) & 1ull)) lpix[lanes_below(pxlive)] = (uint8_t)lane;
    __syncthreads();
    const int nlive = __popcll(pxlive);
    const CamK ck = cam_k(k);
    const int W = k->W, H = k->H;
    // traceRay's depth cut-off comes first: with max_depth <= 0 every sample is black
    const bool live = loc.tile < k->ntiles, trace = k->max_depth > 0;
    const int x0 = loc.tx * 32, y0 = loc.ty * 32, p0 = loc.p0, s0 = loc.s0, sbase = k->sample_base;
    const Hot h = hot<kStage>();
    // id / ns by a multiply-high with m = floor((2^32 - 1) / ns) + 1: exact
    // for id, ns < 2^16 (NB <= kMaxBlockSamples); ns == 1 has no 32-bit m
    const uint32_t mdiv = ns > 1 ? 0xFFFFFFFFu / (uint32_t)ns + 1u : 0u;
    // A black block's tile has empty primary masks: every camera ray misses
    // (renderer.go:170-173), every sample is +0, so nothing is traced.  The
    // counting variant still walks its samples for the path counts (its
    // queries have no candidates: no hit bit is ever set).
    const int NL = kCount ? NB : (loc.black ? 0 : nlive * ns);
    // with an opted-in sky a miss returns the sky (not +0): every camera
    // sample is shaded (no culling applies: the host disables the masks)
    constexpr bool sky = kSky;
    for (int j = lane; j < NL; j += 64) {
      // j -> (pixel, sample): every sample of the block (kCount) or of its
      // live pixels, in order
      const int pj = ns > 1 ? (int)__umulhi((uint32_t)j, mdiv) : j, sl = j - pj * ns;
      const int p = kCount ? pj : (int)lpix[pj], s = s0 + sl, id = p * ns + sl;
      const int tp = p0 + p;
      const int x = x0 + (tp & 31), y = y0 + (tp >> 5);
      // (kCount) this sample's counts; a sample the product never traces (a
      // black block, or a pixel without primary candidates) also goes to
      // `culled`, so the executed work is the difference (rt_counts.culled)
      Counters cs;
      if constexpr (kCount)
        for (int i = 0; i < kCounters; ++i) cs.v[i] = 0;
      [&] {
        if (tp >= 1024 || !live || x >= W || y >= H) return;
        cnt<kCount>(cs, C_CAM);
        rt_rng rng;
        d3 o, d;
        camera_ray_c<kCount>(ck, k->cf, x, y, sbase + s, rng, o, d, cs);
        if (!trace) return;
        cnt<kCount>(cs, C_BOUNCE);
        // hit or miss is all this phase needs: an any-hit query over
        // [0.001, +inf) decides exactly what hitWorld's closest hit would
        const bool hit = sky || (h.masks ? any_hit_masked<kCount>(h.g, o, d, __builtin_inf(), prim, cs)
                                         : any_hit<kCount, false, kMix>(h.g, o, d, __builtin_inf(), stack, cs));
        if (hit) atomicOr(&hbits[id >> 5], 1u << (id & 31));
      }();
      if constexpr (kCount) {
        const bool traced = !loc.black && ((pxlive >> p) & 1ull);
        for (int i = 0; i < kCounters; ++i) {
          c.v[i] += cs.v[i];
          if (!traced) culled.v[i] += cs.v[i];
        }
      }
    }
  }
  __syncthreads();
  // ---- the hit list: ascending sample ids (the <= 32 bit words scanned across the wave)
  if constexpr (!kStream) {
    const int cw = lane < nwords ? __popc(hbits[lane]) : 0;
    int incl = cw;  // inclusive scan over the wave (Hillis-Steele)
    for (int off = 1; off < 64; off <<= 1) {
      const int t = __shfl_up(incl, off);
      if (lane >= off) incl += t;
    }
    if (lane < nwords) hoff[lane] = incl - cw;
    if (lane == 63) hoff[nwords] = incl;
  }
  __syncthreads();
  const int nh = kStream ? 0 : hoff[nwords];
  const HitList<kStream ? 1 : kMaxBlockSamples / 32> hl{hbits, hoff, nwords};
  clk.visibility_done();

  // ---- phases 2 + 3: shade the hit list through a RING of kRound radiance
  // slots (entry e -> slot e % kRound).  Paths finish out of order; the
  // per-pixel sums are taken in entry order (= sample order) by
  // resolve_entries once every entry before the earliest path still running
  // has finished.  A long path therefore holds only its own slot: the other
  // lanes keep taking entries until the ring is full (a barrier per batch of
  // kRound entries made every batch wait for its longest path).
  static_assert((kRound & (kRound - 1)) == 0, "kRound must be a power of two");
  if (kStream || nh > 0) {
    d3 o = mk(0, 0, 0), d = mk(0, 0, 0), T = mk(1, 1, 1);
    rt_rng rng{0};
    int depth = 0, entry = 0;  // (kStream: `entry` is the path's row)
    bool alive = false;
    int next = 0, resolved = 0;  // wave-uniform: next entry to start; entries [0, resolved) summed
    int drain_it = 0;            // (tail helpers) iterations since every entry started
    // (kStream) wave-uniform: the claimed entries not handed out yet, [qbeg,
    // qend); dry: the launch's cursor is past the last entry
    unsigned qbeg = 0, qend = 0;
    bool dry = false;
    // The path's radiance L lives in its entry's ring slot (the slot is the
    // path's own until it finishes, and resolve_entries reads it only then):
    // read and written once per bounce, in VGPRs it held 6 registers through
    // the lighting section and pushed the loop into scratch spills
    // (scratch 40 -> 28 B/lane; headline 0.79 -> 0.775 ms).  Macros: the
    // same accessors as lambdas came out with 40 B/lane of scratch again.
    // (kStream: the lane's own slot; a finished path's L goes to its row in
    // global memory with plain stores, visible at the kernel's end)
#define path_q() (kStream ? (int)threadIdx.x : entry & (kRound - 1))
#define path_L() mk(slot[path_q()][0], slot[path_q()][1], slot[path_q()][2])
#define set_path_L(v)                    \
  do {                                   \
    const d3 v_ = (v);                   \
    const int q_ = path_q();             \
    slot[q_][0] = v_.x;                  \
    slot[q_][1] = v_.y;                  \
    slot[q_][2] = v_.z;                  \
  } while (0)
    // (kSph: the path's throughput T lives in LDS the same way -- used once
    // per bounce, after the lighting section, whose registers its six made
    // one too many at four waves per SIMD)
#define path_T()                                                       \
  ({                                                                   \
    d3 t_;                                                             \
    if constexpr (kSph) {                                              \
      double(*tp_)[3] = tput_lds();                                    \
      t_ = mk(tp_[threadIdx.x][0], tp_[threadIdx.x][1], tp_[threadIdx.x][2]); \
    } else {                                                           \
      t_ = T;                                                          \
    }                                                                  \
    t_;                                                                \
  })
#define set_path_T(v)                    \
  do {                                   \
    const d3 v_ = (v);                   \
    if constexpr (kSph) {                \
      double(*tp_)[3] = tput_lds();      \
      tp_[threadIdx.x][0] = v_.x;        \
      tp_[threadIdx.x][1] = v_.y;        \
      tp_[threadIdx.x][2] = v_.z;        \
    } else {                             \
      T = v_;                            \
    }                                    \
  } while (0)
#define stream_store_row()                                            \
  do {                                                                \
    if constexpr (kStream) {                                          \
      double* r_ = sfresh()->s.rows + (size_t)(unsigned)entry * 3;    \
      const int q_ = path_q();                                        \
      r_[0] = slot[q_][0];                                            \
      r_[1] = slot[q_][1];                                            \
      r_[2] = slot[q_][2];                                            \
    }                                                                 \
  } while (0)
    // HitRecord of the closest primitive `hs` of the lane's ray (sphere.go:42-58,
    // triangle.go:68-81).  The block kernels fill it where the pass finds the
    // hit.  kStream: only `hs` is kept across the passes, and the record of
    // both passes' hits is filled once behind them -- a lane that hit keeps
    // its o and d until the scatter, so the expressions see the same values;
    // one run at the width of both passes' hitters instead of two at half of
    // it each, and P, N, front, mi and self are not live through the second
    // pass.  (A macro, as the accessors above.)
#define hit_record(gg_)                                                 \
  do {                                                                  \
    if (!hit_is_tri(hs)) {                                              \
      const DSphere& S0 = (gg_).spheres[hs.idx];                        \
      const double t = hs.num / len2(d);                                \
      P = o + muls(d, t);                                               \
      d3 outward = divs(P - ld3(S0.c), S0.r);                           \
      front = dot(d, outward) < 0;                                      \
      N = front ? outward : neg(outward);                               \
      mi = S0.mat;                                                      \
      self = S0.obj;                                                    \
    } else if constexpr (!kSph) {                                       \
      const DTri& T0 = (gg_).tris[hs.idx];                              \
      P = o + muls(d, hs.num);                                          \
      double w = 1.0 - hs.u - hs.v;                                     \
      d3 n = ld3(T0.n);                                                 \
      N = normalize((muls(n, w) + muls(n, hs.u)) + muls(n, hs.v));      \
      front = dot(d, N) < 0;                                            \
      if (!front) N = neg(N);                                           \
      mi = T0.mat;                                                      \
      self = T0.obj;                                                    \
    }                                                                   \
  } while (0)
    for (;;) {
      // (1) closest hit (hitWorld, renderer.go:170), in up to two passes: a
      // lane whose ray missed (or reached the depth cut-off) finishes at once
      // and, while other lanes go on to light their hits, takes the next
      // entry (its camera ray hits: phase 1 found a hit for it) and runs that
      // closest hit in a second pass -- so lighting and scatter, the bulk of
      // an iteration, run on the lanes of both passes' hits instead of
      // idling every lane whose ray missed (57 % of the headline's traced
      // rays hit: the lighting used to run on ~60 % of the lanes)
      bool shade = false, front = false, fin = false;
      d3 P = mk(0, 0, 0), N = mk(0, 0, 0);
      int mi = 0, self = -1;
      HitK hs;
      int outer = 0;  // 1: continue the shade loop, 2: leave it
      for (int pass = 0;; ++pass) {
        if constexpr (kStream) {
          // Lanes without a path take the next entries of the launch-wide
          // queue, in lane order.  The wave claims entries a chunk at a time
          // (one relaxed add by one lane on the launch's cursor: a claim per
          // entry would put ~0.9 M adds per headline frame on one address);
          // when the claimed chunk runs out it claims the next one in the
          // same pass (two rounds at most).  No wave ever waits for another.
          unsigned long long fm = __ballot(!alive);
          const unsigned long long fm0 = fm;
          for (int r = 0; r < 2 && fm != 0; ++r) {
            if (qbeg == qend) {
              if (dry) break;
              const uint2 q = stream_claim_chunk();
              qbeg = q.x;
              qend = q.y;
              if (qbeg == qend) {
                dry = true;
                break;
              }
            }
            const unsigned e = qbeg + (unsigned)lanes_below(fm);
            if (!alive && e < qend) {
              entry = stream_entry<kBase, kCams>(e, rng, o, d, skey);
              set_path_T(mk(1, 1, 1));
              if constexpr (kSph) {
                // (the zero made here: held in a register pair from the
                // prologue on, it was spilled at four waves per SIMD)
                const double z = zero_now();
                set_path_L(mk(z, z, z));
              } else {
                set_path_L(mk(0, 0, 0));
              }
              depth = 0;
              alive = true;
            }
            qbeg = min(qend, qbeg + (unsigned)__popcll(fm));
            fm = __ballot(!alive);
          }
          clk.refill(pass > 0, fm0 & ~fm);
        }
        const unsigned long long freem = kStream ? 0ull : __ballot(!alive);
        int limit = kStream ? 0 : min(nh, resolved + kRound);
        if (freem != 0 && next == limit && next < nh) {
          // the ring is full and lanes are idle: sum every entry before the
          // earliest one still running (a wave-wide min over the live lanes)
          const int lo = ring_low(alive, entry, next);
          if (lo > resolved) {
            __syncthreads();
            resolve_entries<kTail>(hl, nh, blk, slot, psum, prow, pk0, xm, resolved, lo);
            __syncthreads();
            if constexpr (kTail) {
              // the resolved entries' ring slots take new entries now: their
              // exported marks go (slot s is in [resolved, lo) mod kRound iff
              // (s - resolved) mod kRound < lo - resolved)
              if (lane < kRound / 32) {
                uint32_t m = 0;
                for (int j = 0; j < 32; ++j)
                  m |= (uint32_t)(((32 * lane + j - resolved) & (kRound - 1)) < lo - resolved) << j;
                xm[lane] &= ~m;
              }
            }
            resolved = lo;
            limit = min(nh, resolved + kRound);
          }
        }
        // lanes without a path take the next entries, in lane order
        const int e = next + lanes_below(freem);
        if (!kStream && !alive && e < limit) {
          block_entry(hl, e, rng, o, d, skey);
          entry = e;
          T = mk(1, 1, 1);
          set_path_L(mk(0, 0, 0));
          depth = 0;
          alive = true;
        }
        next = min(limit, next + __popcll(freem));
        if (pass == 0) {
          if (__ballot(alive) == 0) {  // wave-uniform
            // every entry done / ring full of finished entries: resolve, then refill
            // (kStream: no lane found an entry, so the queue is dry: the wave leaves)
            outer = (kStream ? dry : next >= nh) ? 2 : 1;
            break;
          }
          clk.iteration(alive, lane);
          if constexpr (kTail) {
            // Tail helpers: every entry has started and at
            // most tail_kmax paths are left, each tail_dmin bounces deep or
            // more -- the block's drain.  Each goes to a helper wave (while
            // one is free), which runs it alone at solo latency; its radiance
            // reaches the pixel through the pixel's row (resolve_entries, the
            // epilogue), the same sum in the same order.
            // (every tail_every-th iteration of the drain, 4 by default: the gate read is a memory round
            // trip on the lone paths' chain, and a drain shorter than that
            // gains nothing from a helper)
            // The block's drain: every entry has started.  (Exporting at ring
            // stalls too -- the ring full behind a long path, whose export lets
            // the lanes take new entries -- measured slower: one frame 0.555 ->
            // 0.620 ms at 64 helpers; more, shorter paths queue for the helpers
            // ahead of the long ones.  The resolve below supports it: rows are
            // filled mid-loop and exported ring slots are unmarked on reuse.)
            if (next >= nh && (++drain_it & fresh()->tail_every_mask) == 0 && fresh()->tail != nullptr) {
              const unsigned long long am = __ballot(alive);
              if (__popcll(am) <= fresh()->tail_kmax) {
                for (unsigned long long em = __ballot(alive && depth >= fresh()->tail_dmin); em; em &= em - 1) {
                  const int ow = __builtin_ctzll(em);
                  const unsigned long long t_x = __builtin_amdgcn_s_memrealtime();
                  KArg k = fresh();
                  TailCtl* ctl = k->tail;
                  const int idx = tail_reserve(k);
                  // (all the handed-over bytes below are written through: st_wt*)
                  if (idx < 0) break;  // (no helper free: the paths stay here)
                  const int e = (int)rl32((uint32_t)entry, ow);
                  const BlockLoc loc = block_loc(k, block_of(k));
                  const int id = hl.entry_id(e), ns = loc.ns;
                  const int p = id / ns, sl = id - p * ns;
                  const int tp = loc.p0 + p;
                  const int px = loc.tx * 32 + (tp & 31), py = loc.ty * 32 + (tp >> 5);
                  const int64_t oi = k->layout == RT_LAYOUT_IMAGE ? (int64_t)py * k->W + px
                                                                  : (int64_t)loc.lt * 1024 + tp;
                  int kind, row, sample;
                  if (loc.slot >= 0) {  // a split pixel: its split row (its counter owes one more finisher)
                    kind = kTailSplit;
                    row = (int)split_index(k, loc.slot);
                    sample = loc.s0 + sl;
                    if (lane == 0) atomicSub(&k->split_cnt[row], 1);
                  } else {
                    kind = kTailRow;
                    sample = sl;
                    const int r = tail_pixel_row(k, p, sl, oi, prow, pk0);
                    row = r;
                  }
                  if (lane == ow) {
                    TailPath* q = k->tail_q + idx;
                    const int qs = e & (kRound - 1);
                    st_wtd(q->o, o.x); st_wtd(q->o + 1, o.y); st_wtd(q->o + 2, o.z);
                    st_wtd(q->d, d.x); st_wtd(q->d + 1, d.y); st_wtd(q->d + 2, d.z);
                    st_wtd(q->T, T.x); st_wtd(q->T + 1, T.y); st_wtd(q->T + 2, T.z);
                    st_wtd(q->L, slot[qs][0]); st_wtd(q->L + 1, slot[qs][1]); st_wtd(q->L + 2, slot[qs][2]);
                    st_wt64(&q->rng, rng.x);
                    st_wt64(&q->skey, skey[ow]);
                    st_wt32(&q->depth, (uint32_t)depth);
                    st_wt32(&q->sample, (uint32_t)sample);
                    st_wt32(&q->kind, (uint32_t)kind);
                    st_wt32(&q->row, (uint32_t)row);
                    st_wt32(&q->nsub, (uint32_t)loc.nsub);
                    st_wt32(&q->frame, (uint32_t)frame_of(k));
                    st_wt64(&q->oi, (uint64_t)oi);
                    alive = false;
                  }
                  if (lane == 0) {
                    const int qs = e & (kRound - 1);
                    xm[qs >> 5] |= 1u << (qs & 31);
                    atomicAdd(&ctl->exported, 1u);
                  }
                  wt_drain();  // every lane's write-through stores, then the flag
                  if (lane == ow) __hip_atomic_store(&k->tail_ready[idx], k->tail_epoch, __ATOMIC_RELAXED,
                                                     __HIP_MEMORY_SCOPE_AGENT);
                  if (lane == 0) atomicAdd(&ctl->export_ticks, (unsigned int)(__builtin_amdgcn_s_memrealtime() - t_x));
                }
                if (__ballot(alive) == 0) {  // every path left went to a helper
                  outer = next >= nh ? 2 : 1;  // done / the ring moves on: resolve, then refill
                  break;
                }
              }
            }
          }
          if constexpr (kStage && !kCount && !kPilot && !kStream && RT_SOLO) {
            // one path left (no free lane found an entry to start): the whole
            // wave runs it to its end (solo_path)
            const unsigned long long am = __ballot(alive);
            // (two or three paths run one after the other this way measured
            // slower: 0.79 / 0.93 vs 0.78 ms)
            if (__popcll(am) == 1 && hot<kStage>().masks) {
              const d3 Lr = solo_path<kSky>(fresh(), __builtin_ctzll(am), o, d, T, path_L(), rng.x, depth,
                                          skey[__builtin_ctzll(am)], stack);
              if (lane == __builtin_ctzll(am)) {
                const int q = entry & (kRound - 1);
                slot[q][0] = Lr.x;
                slot[q][1] = Lr.y;
                slot[q][2] = Lr.z;
                alive = false;
              }
              outer = 1;
              break;
            }
          }
        }  // pass 0

        bool wide_q = false, wide_found = false, wide_fb = false;
        if constexpr (kStage) {  // wave-uniform: few paths left -> helpers
          const Hot h = hot<kStage, kSph>();
          const bool need = alive && !shade && depth < h.max_depth;
          const unsigned long long qm = __ballot(need);
          const int nq = __popcll(qm);
          // (from 16 spheres on: below that the group set-up and merge cost more
          // than the short scan they split; measured on the 5-sphere scene)
          if (h.g.nt == 0 && h.g.ns >= 16 && nq > 0 && nq <= 16) {
            // (kCount: helpers count their sphere tests, primary queries included)
            if constexpr (kStream) {
              // (closest_wide writes every lane's hit: the first pass's hitters keep theirs for the record)
              HitK hw;
              wide_found = closest_wide<kCount, kSph>(h.g, need, qm, nq, o, d, hw, wide_fb, c);
              if (need) hs = hw;
            } else {
              wide_found = closest_wide<kCount, kSph>(h.g, need, qm, nq, o, d, hs, wide_fb, c);
            }
            wide_q = true;
          }
        }
        if (alive && !shade) {
          const Hot h = hot<kStage, kSph>();
          const Geo& gg = h.g;
          bool done = depth >= h.max_depth;  // traceRay depth cut-off: contributes 0
          bool missed = false;
          if (!done) {
            if (kCount && depth == 0) {  // phase 1 counted the primary query
              Counters nc;
              done = (wide_q && !wide_fb) ? !wide_found : !closest_hit<false, kSph, kMix>(gg, o, d, hs, stack, all, nc);
            } else {
              cnt<kCount>(c, C_BOUNCE);
              done = (wide_q && !wide_fb) ? !wide_found
                                          : !closest_hit<kCount, kSph, kMix>(gg, o, d, hs, stack, all, c);  // miss -> black
            }
            missed = done;
          }
          if (done) {
            if constexpr (kSky) {  // an opted-in sky instead of black (rt_settings.sky)
              if (missed) set_path_L(path_L() + mul(T, sky_color(fresh()->sky, d)));
            }
            if (depth > 0) set_path_L(path_end(path_L(), path_T()));  // (rt_device.h; T = 1 at depth 0)
            if constexpr (kPilot) pilot_record(hl, entry, depth);
            stream_store_row();
            alive = false;  // finished: its radiance is in its slot, the lane is free for the second pass
          } else {
            shade = true;
            cnt<kCount>(c, C_SHADE);
            // (kStream: one hit record per iteration, behind the passes)
            if constexpr (!kStream) hit_record(gg);
          }
        }
        // a second pass when enough lanes are free and entries are left
        if (pass > 0 || kRefill2Min <= 0 || __popcll(__ballot(!alive)) < kRefill2Min ||
            (kStream ? dry && qbeg == qend : next >= nh))
          break;
      }  // passes
      if (outer == 1) continue;
      if (outer == 2) break;

      if constexpr (kStream) {
        if (shade) hit_record((hot<kStage, kSph>().g));
      }
      clk.hit_done();
      if (__ballot(shade) != 0) {
        // (2) calculateDirectLighting (renderer.go:229-297), light by light
        const Hot h = hot<kStage, kSph>();
        const Geo& gg = h.g;
        const bool masks = h.masks, soft = h.soft;
        const DMat* __restrict__ m = h.mats + mi;
        d3 D = mk(0, 0, 0);
        if (shade) D = mk(m->ambient, m->ambient, m->ambient);
        for (int li = 0; li < h.nl; ++li) {
          const DLight& Lt = h.lights[li];
          d3 ldir = mk(0, 0, 0);
          double ldist = 0;
          CandK cm{};
          bool lit = false, occl = false;
          clk.begin(kClkHard);
          if (shade) {
            d3 lv = ld3(Lt.pos) - P;
            ldist = sqrt(lv.x * lv.x + lv.y * lv.y + lv.z * lv.z);
            ldir = ldist == 0 ? mk(0, 0, 0) : divs(lv, ldist);
            lit = !(ldist < 0.001);
            if (lit) {
              cnt<kCount>(c, C_LIGHT);
              cnt<kCount>(c, C_SHADOW);
            }
          }
          // (r05) an inert light (light_inert): its shadow rays are not
          // traced (the counting variant traces them, for the reference's
          // counts, and books them as culled)
          const bool dark = shade && lit && light_inert(m, Lt, N, ldir, D);
          const bool hard = shade && lit && (kCount || !dark);
          bool wide_c = false;
          if constexpr (kStage) {  // few lit hit points: the cone tests with helpers
            if (masks && gg.nt == 0 && RT_CONE_HELPERS) {
              const unsigned long long cq = __ballot(hard);
              const int ncq = __popcll(cq);
              if (ncq > 0 && ncq <= 16) {
                unsigned long long ms;
                if constexpr (kSph)
                  ms = cone_wide<true>(gg, hard, cq, ncq, P, N, front, self, ldir, ldist,
                                       hard ? cone_row(fresh(), li, self) : 0ull);
                else
                  ms = cone_wide(gg, hard, cq, ncq, P, N, front, self, ldir, ldist);
                if (hard) {
                  cm = CandK{};
                  cm.s = ms;
                }
                wide_c = true;
              }
            }
          }
          if (hard) {
            if constexpr (kSph) {
              if (masks && !wide_c)
                cm = cone_candidates_rows(gg, P, N, front, self, ldir, ldist, cone_row(fresh(), li, self));
            } else {
              if (masks && !wide_c) cm = cone_candidates<kSph>(gg, P, N, front, self, ldir, ldist);
            }
            if constexpr (kCount) {
              const unsigned long long s0 = c.v[C_SPH], t0 = c.v[C_TRI];
              occl = shadow_blocked<kCount, kSph, kMix>(gg, masks, P, ldir, ldist, cm, stack, c);  // hard shadow ray
              if (dark) {
                culled.v[C_SHADOW] += 1;
                culled.v[C_SPH] += c.v[C_SPH] - s0;
                culled.v[C_TRI] += c.v[C_TRI] - t0;
              }
            } else {
              occl = shadow_blocked<kCount, kSph, kMix>(gg, masks, P, ldir, ldist, cm, stack, c);  // hard shadow ray
            }
          }
          clk.end(kClkHard);
          const bool need_soft = lit && !occl && soft;
          // the 16 soft rays are traced unless their shadow cone is empty or
          // the light is inert (dark: the shading is the same whatever they hit)
          const bool trace = (!masks || cand_any(cm)) && !dark;
          int unocc = 0;
          // Spec v4 (include/rt_rng.h): the 16 points come from the stream of
          // (sample, depth, light), not from the path's.  A lane whose rays
          // cannot be blocked (empty shadow cone, or dark) needs none of them:
          // all 16 are unoccluded, nothing is drawn.  (The counting variant
          // still walks their tries, for the reference's draw count, and
          // books them as culled: executed work is the difference.)
          const bool free_soft = need_soft && !trace;
          if (free_soft) {
            unocc = 16;
            if constexpr (kCount) {
              rt_rng fr{rt_soft_state(skey[lane_now()], (uint32_t)depth, (uint32_t)li)};
              unsigned long long tries = 0;
              for (int got = 0; got < 16; ++tries) {
                const uint32_t ux = rt_rng_next(&fr), uy = rt_rng_next(&fr), uz = rt_rng_next(&fr);
                got += unit_ball_accept(ux, uy, uz) ? 1 : 0;
              }
              cnt<kCount>(c, C_SHADOW, 16);
              cnt<kCount>(c, C_RNG, 3ull * tries);
              culled.v[C_SHADOW] += 16;
              culled.v[C_RNG] += 3ull * tries;
            }
          }
          const bool traced_soft = need_soft && trace;
          rt_rng srng{traced_soft ? rt_soft_state(skey[lane_now()], (uint32_t)depth, (uint32_t)li) : 0ull};
          // soft shadows: wave-converged decision between the two forms
          const unsigned long long owners = __ballot(traced_soft);
          clk.begin(kClkSoft);
          if (owners != 0) {
            clk.soft_form(owners);
            // cooperative soft shadows when at most kCoopMax lanes need them
            if (__popcll(owners) <= kCoopMax) {
              for (unsigned long long b = owners; b; b &= b - 1) {
                const int ow = __builtin_ctzll(b);
                const CoopOut r = soft_coop<kCount, kSph, kMix>(
                    gg, masks, true, inv3(rl3(P, ow)), inv3(rl3(ldir, ow)),
                    inv(rld(ldist, ow)), cand_of_lane(cm, ow), rl64(srng.x, ow), h.jump, stack, c);
                if (lane == ow) {
                  unocc = r.unocc;
                  cnt<kCount>(c, C_SHADOW, 16);
                  cnt<kCount>(c, C_RNG, 3ull * r.tries);
                }
              }
            } else {
              const int uq =
                  soft_queue<kCount, kSph, kMix>(gg, masks, traced_soft, true, P, ldir, ldist, cm, srng, h.jump, stack, c);
              if (traced_soft) unocc = uq;  // (a free lane keeps its 16)
            }
          }
          clk.end(kClkSoft);
          if (lit) {
            const double sf = occl ? 0.0 : (soft ? (double)unocc / 16.0 : 1.0);  // shadowSum / 16
            if (sf > 0.0) {
              const double metallic = m->metallic;
              double cos_t = gmax0(dot(N, ldir));
              double intensity = cos_t * Lt.intensity / (ldist * ldist);
              D = D + muls(ld3(m->albedo), m->diffuse_strength * intensity * sf);
              if (metallic > 0.5) {
                d3 view = normalize(neg(P));
                d3 half = normalize(ldir + view);
                double hc = gmax0(dot(N, half));
                const int sp = m->spec_pow;
                double si = sp == 64 ? pow_n<64>(hc) : (sp == 48 ? pow_n<48>(hc) : pow_n<32>(hc));
                D = D + muls(ld3(Lt.color), si * intensity * sf * metallic * 3.0);
              }
            }
          }
        }
        clk.end(kClkLight);
        // (3) Material.Scatter and the traceRay combination (renderer.go:181-226)
        clk.begin(kClkScat);
        if (shade) {
          d3 E = ld3(m->emit);
          const Scat sc = scatter<kCount>(m, d, N, front, rng, c);
          if (!sc.ok) {
            const d3 Tp = path_T();
            set_path_L(path_end(path_L() + mul(Tp, E + D), Tp));
            fin = true;
          } else {
            d3 Tp = path_T();
            d3 Lp = path_L() + mul(Tp, E + muls(D, m->dw));
            path_step(Tp, Lp, sc.A, m->rw);  // (rt_device.h: also before a last bounce, whose black is multiplied too)
            fin = !h.recursive || depth + 1 >= h.max_depth;
            set_path_L(fin ? path_end(Lp, Tp) : Lp);
            if (!fin) {
              set_path_T(Tp);
              o = P;
              d = sc.nd;
              depth += 1;
            }
          }
        }
        clk.end(kClkScat);
      }
      if (fin) {  // the path's radiance goes to its entry's ring slot
        if constexpr (kPilot) pilot_record(hl, entry, depth);
        stream_store_row();
        alive = false;  // (its radiance is in its slot already)
      }
    }
    if constexpr (!kStream) {
      __syncthreads();
      resolve_entries<kTail>(hl, nh, blk, slot, psum, prow, pk0, xm, resolved, nh);
      __syncthreads();
    }
  }
#undef path_L
#undef set_path_L
#undef path_T
#undef set_path_T
#undef path_q
#undef stream_store_row
#undef hit_record
  clk.loop_done();
  if constexpr (kStream) {
    // every row of this wave's paths is written; resolve_rows_kernel, the next
    // kernel on the stream, sums them
    clk.stream_write(threadIdx.x);
    return;
  }

  // ---- phase 3 (final): mean, tone map, one write per pixel
  KArg k = fresh();
  // the lane id laundered (see resolve_entries): the LDS addresses of this
  // epilogue are computed here, not kept live (spilled) from the prologue
  int lane3;
  asm volatile("v_mov_b32 %0, %1" : "=v"(lane3) : "v"((int)threadIdx.x));
  bool resolve = true;
  if (blk.slot >= 0) {
    // a split pixel: the last of its sub-blocks to finish sums the hit
    // samples of the slot row in sample order (misses add +0) and writes it
    // Tail kernel: its row samples were written through, drained before the
    // counter, and the last contributor reads the row sc1 (the tail
    // helpers' hand-off, above).  Product kernel: plain stores, a release
    // fence before the counter and an acquire fence after it (the same
    // time, r06 A/B, and the row's samples reach HBM as whole lines: the
    // write-through form wrote 3.8 MB more per headline frame)
    if constexpr (kTail)
      wt_drain();
    else
      __threadfence();
    int old = 0;
    if (lane3 == 0) old = atomicAdd(&k->split_cnt[split_index(k, blk.slot)], 1);
    old = __builtin_amdgcn_readfirstlane(old);
    resolve = old == blk.nsub - 1;
    if (resolve) {
      if constexpr (!kTail) __threadfence();
      const double* row = k->split_rad + split_index(k, blk.slot) * k->spp * 3;
      uint32_t* hw = k->split_hits + split_index(k, blk.slot) * ((k->spp + 31) >> 5);
      // chunks of kRound samples: all lanes load (in parallel) into the LDS
      // slots, misses as +0, then one lane per channel adds them in order
      double a = 0;  // (a later sample pass continues the running sum)
      if ((k->acc_mode & 1) && lane3 < 3) a = k->acc[((size_t)blk.lt * 1024 + blk.p0) * 3 + lane3];
      a = row_sum<kTail>(slot, row, hw, 0, k->spp, a, lane3);
      if (lane3 < 3) psum[0][lane3] = a;
      // the slot's hit bits and counter are left zeroed for the next launch
      // (the host clears them only when it builds a schedule: no memset per frame)
      for (int i = lane3; i < ((k->spp + 31) >> 5); i += 64) hw[i] = 0u;
      if (lane3 == 0) k->split_cnt[split_index(k, blk.slot)] = 0;
      __syncthreads();
    }
  }
  if (resolve) {
    const BlockLoc loc = block_loc(k, block_of(k));
    const int p = lane3;
    const int tp = loc.p0 + p;
    const int x = loc.tx * 32 + (tp & 31), y = loc.ty * 32 + (tp >> 5);
    bool rowed = false;  // (tail helpers: the pixel's row writes it, below)
    if constexpr (kTail) rowed = prow[p] >= 0;
    if (rowed) {
    } else if ((k->acc_mode & 2) && p < loc.np && tp < 1024) {  // not the last sample pass: keep the running sum
      double* a = k->acc + ((size_t)loc.lt * 1024 + tp) * 3;
      a[0] = psum[p][0];
      a[1] = psum[p][1];
      a[2] = psum[p][2];
    } else if (p < loc.np && tp < 1024 && loc.tile < k->ntiles && x < k->W && y < k->H) {
      if (k->acc_mode & 4) {  // a progression's add: keep the sum and write the pixel
        double* a = k->acc + ((size_t)loc.lt * 1024 + tp) * 3;
        a[0] = psum[p][0];
        a[1] = psum[p][1];
        a[2] = psum[p][2];
      }
      const double n = (double)k->spp_total;
      const double mx = psum[p][0] / n, my = psum[p][1] / n, mz = psum[p][2] / n;  // DivScalar(float64(samples))
      const size_t oi = k->layout == RT_LAYOUT_IMAGE ? (size_t)y * k->W + x : (size_t)loc.lt * 1024 + (size_t)tp;
      const int fr = frame_of(k);
      float* const ol = k->frame_lin[fr];
      uint8_t* const orgba = k->frame_rgba[fr];
      if (ol) {
        ol[oi * 3 + 0] = (float)mx;
        ol[oi * 3 + 1] = (float)my;
        ol[oi * 3 + 2] = (float)mz;
      }
      if (orgba) {
        *reinterpret_cast<uint32_t*>(orgba + oi * 4) = tonemap_rgba8(mx, my, mz);
      }
    }
  }
  if constexpr (kTail) tail_rows_give_back(k, blk, lane3, slot, psum, prow, pk0);
  if constexpr (kCount) reduce_counters(k, lane3, c, culled);
  clk.write(k, lane3, true, (unsigned long long)blk.np * 65536ull + (unsigned long long)blk.ns, (unsigned long long)(blk.slot + 1));
  if constexpr (kTail) {
    if (k->tail != nullptr) {
      // this main block is done: it queues nothing more (no fence: its queue
      // reservations were returning atomics, complete before this one)
      if (lane3 == 0) atomicAdd(&k->tail->done[(blockIdx.x % kTailShards) * 32], 1u);
    }
  }
}

}  // namespace rtgo
