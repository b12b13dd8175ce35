// rt_shadow.h — shadow device code of the megakernel's body (rt_body.h): the
// lane helpers, shadow-cone culling, wide mode, inert lights and the soft
// shadows' two wave-converged forms (soft_coop, soft_queue).
#pragma once
#include <hip/hip_runtime.h>

#include "../../include/rt_rng.h"
#include "rt_device.h"
#include "rt_internal.h"

// cooperative soft shadows when at most this many lanes need them (measured
// best of 0/2/4/8 in round 1; 4 and 16 within noise in round 2)
#ifndef RT_COOP_MAX
#define RT_COOP_MAX 8
#endif
constexpr int kCoopMax = RT_COOP_MAX;
// soft_queue: the owners still drawing finish cooperatively once at most
// this many are left (measured best of 0/1/2/4, r03)
#ifndef RT_SQ_TAIL
#define RT_SQ_TAIL 2
#endif
constexpr int kSqTail = RT_SQ_TAIL;
// soft_queue: rejection tries per pass of its loop (measured best of 1..6
// within the LDS budget, r03)
#ifndef RT_SQ_TRIES
#define RT_SQ_TRIES 2
#endif
constexpr int kSqTries = RT_SQ_TRIES;

namespace rtgo {

// The lane id through a volatile move: an LDS address derived from it is
// computed where it is used instead of being kept live through the bounce
// loop (live across the lone-path call, such values are spilled to scratch
// once per wave: the one-frame launch's bulk HBM writes)
__device__ __forceinline__ int lane_now() {  // (one-wave workgroups: the lane is threadIdx.x)
  int l;
  asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
  return l;
}
// +0.0 through a volatile move, for the same reason: the constant is made
// where it is used instead of being kept in a register pair through the loop
__device__ __forceinline__ double zero_now() {
  double z;
  asm volatile("v_mov_b64 %0, 0" : "=v"(z));
  return z;
}
// Set bits of a wave mask below the calling lane (v_mbcnt): no 64-bit
// per-lane "below" mask has to stay live (it was spilled to scratch)
__device__ __forceinline__ int lanes_below(unsigned long long m) {
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

// ------------------------------------------------------------ culling
// Shadow-cone culling (linear-scan scenes with <= 64 spheres and <= 64
// triangles).  calculateSmartShadow's rays all leave the hit point P inside
// the cone around ldir of half-angle asin(0.1) (|RandomVec3InUnitSphere *
// 0.1| < 0.1, renderer.go:316-317) and end at the light (tMax = distance).
// A primitive whose bounding sphere cannot meet that cone segment can never
// be hit by the hard ray or by any of the 16 soft rays, so it is left out of
// their tests; everything else gets the exact Sphere.Hit / Triangle.Hit
// test, so occlusion results are unchanged.  Margins (~1e-7 relative) are
// eight orders of magnitude above binary64 rounding.
//
// The two square roots are single-precision hardware roots (v_sqrt_f32 of
// the binary64 value rounded to float: relative error < 2e-7, far inside
// the 1e-5 relative margins below).  A culling test only has to be
// conservative, not exact: float overflow gives dc = inf (kept), underflow
// gives dc = 0 (kept).  No early exits, so the compiler can batch the
// loads of consecutive spheres.
__device__ __forceinline__ bool in_cone(const double* cc, double r, d3 P, d3 ldir, double ldist) {
  const d3 v = ld3(cc) - P;
  const double dc2 = len2(v);
  const double dc = (double)__builtin_amdgcn_sqrtf((float)dc2);
  const double ra = fabs(r) * KC(1.0 + 1e-5) + KC(1e-5) * dc + KC(1e-12);  // inflated radius
  // Every test is "not provably missed": a NaN hit point, light direction,
  // centre or radius fails each comparison and the sphere is kept, as
  // Sphere.Hit accepts what it cannot compare (`disc < 0`, `root < tMin ||
  // tMax < root` are false for NaN, sphere.go:22-40), so a NaN shadow ray is
  // blocked by every sphere
  const bool inside = !(dc > ra);                                         // P inside / on it
  const bool beyond = dc - ra > ldist * KC(1.0 + 1e-5) + KC(1e-9);      // beyond the light
  // angle(v, ldir) <= alpha + beta, sin(alpha) = 0.1, sin(beta) = ra/dc:
  // v.ldir >= dc*cos(alpha+beta) = cos(alpha)*sqrt(dc^2-ra^2) - 0.1*ra
  const double tl = (double)__builtin_amdgcn_sqrtf((float)fmax(dc2 - ra * ra, 0.0));
  const bool meets = !(dot(v, ldir) < KC(0.99498) * tl - KC(0.1) * ra - KC(1e-5) * dc);
  return inside || (!beyond && meets);
}

// `self` is the hittable that was hit.  When the hit is on its OUTSIDE and
// every cone direction leaves the surface by a clear angle (N.ldir >= 0.1015
// > sin(alpha), N the normal facing the ray's side), a convex hittable
// (sphere of positive radius, or createCube's box) cannot be hit again at
// t >= 0.001.  A hit from inside is never left out: the shadow ray has to
// cross the object.  "Outside" per kind:
//   sphere: FrontFace (sphere.go:42-48 takes the true outward normal);
//   cube:   FrontFace != "its normals point in" (DBox.front_out): createCube
//           winds them inward, so FrontFace there means a hit from inside.
__device__ __forceinline__ bool box_self_out(const DBox& B, bool front) { return (int)front == B.front_out; }

// (kSph, here and below: the scene is spheres alone, DESIGN.md §4.7 -- no
// triangle or cube code, and the candidates are the sphere mask, Kind<kSph>)
template <bool kSph = false>
__device__ __forceinline__ typename Kind<kSph>::C cone_candidates(const Geo& p, d3 P, d3 N, bool front, int self,
                                                                  d3 ldir, double ldist) {
  const bool leaves = dot(N, ldir) >= KC(0.1015);
  const bool sphere_out = front && leaves;
  typename Kind<kSph>::C m{};
  for (int i = 0; i < p.ns; ++i) {
    const DSphere& S = p.spheres[i];
    if (sphere_out && S.obj == self && S.r > 0) continue;
    if (in_cone(S.c, S.r, P, ldir, ldist)) m.s |= 1ull << i;
  }
  if constexpr (!kSph) {
    // triangles by cube: one cone test against the bounding sphere of the
    // cube's box admits its 12 triangles (their exact tests follow per ray)
    for (int j = 0; j < p.nb; ++j) {
      const DBox& B = p.boxes[j];
      if (leaves && B.obj == self && box_self_out(B, front)) continue;
      if (in_cone(B.bc, B.br, P, ldir, ldist)) m.t |= 0xFFFull << B.first;
    }
  }
  return m;
}

// hitWorld(shadowRay, 0.001, dist) restricted to the candidates.
template <bool kCount, bool kSph = false>
__device__ __forceinline__ bool any_hit_masked(const Geo& p, d3 o, d3 d, double tmax, typename Kind<kSph>::C m,
                                               Counters& c) {
  if constexpr (!kSph) {
    if (m.t) {  // a cube whose box the ray misses cannot be hit: drop its 12 triangles
      const d3 id = inv_dir(d);
      for (int j = 0; j < p.nb; ++j) {
        const DBox& B = p.boxes[j];
        const unsigned long long g = 0xFFFull << B.first;
        if ((m.t & g) && !ray_box(B, o, id, 0.001, tmax)) m.t &= ~g;
      }
    }
  }
  if (m.s) {  // (most camera rays have no candidate at all)
    const double a = len2(d);
    const double inv_a = approx_rcp(a);
    for (unsigned long long b = m.s; b; b &= b - 1) {
      const int i = __builtin_ctzll(b);
      cnt<kCount>(c, C_SPH);
      double num;
      if (sphere_query(p.spheres[i], o, d, a, inv_a, 0.001, tmax, num)) return true;
    }
  }
  if constexpr (!kSph) {
    for (unsigned long long b = m.t; b; b &= b - 1) {
      const int i = __builtin_ctzll(b);
      cnt<kCount>(c, C_TRI);
      double t, u, v;
      if (tri_test(p.tris[i], o, d, 0.001, tmax, t, u, v)) return true;
    }
  }
  return false;
}

// Occlusion of one shadow ray: candidates when culling is on, else all.
// (kSph: any_hit's triangle loops fold away, hot() sets nt = nb = 0)
template <bool kCount, bool kSph = false, bool kMix = false>
__device__ __forceinline__ bool shadow_blocked(const Geo& p, bool masks, d3 o, d3 d, double tmax,
                                               typename Kind<kSph>::C m, int* stack, Counters& c) {
  if (masks) return cand_any(m) && any_hit_masked<kCount, kSph>(p, o, d, tmax, m, c);
  return any_hit<kCount, kSph, kMix>(p, o, d, tmax, stack, c);
}

// Occlusion of one SOFT shadow ray, from P towards ldir + 0.1 pt, in the
// spheres-only stream kernels: only the boolean leaves this
// code, so the candidates first go through soft_screen (rt_internal.h) on the
// unnormalised direction u and a binary32 1 / |u|.  |u|^2 lies in [0.81, 1.21]
// (ldir a unit vector, |pt| < 1); v_rsq_f32 is good to 1 ulp (AMD Instinct
// CDNA ISA guide) and its argument is |u|^2 rounded to binary32, so
// |il |u| - 1| < 2^-23 + 2^-25 + 2^-51 < kSoftScreenIl.  The first sure hit
// makes the ray occluded, sure misses of every candidate make it
// unoccluded; only a lane with an undecided candidate and no sure hit
// normalises the ray and runs the exact test as before, behind a branch the
// wave skips when it has no such lane.
template <bool kCount, bool kMix>
__device__ __forceinline__ bool soft_blocked_sph(const Geo& p, bool masks, d3 P, d3 ldir, d3 pt, double ldist, CandS m,
                                                 int* stack, Counters& c) {
  if (RT_SOFT_SCREEN && masks) {
    const d3 u = ldir + muls(pt, 0.1);
    const double il = (double)__builtin_amdgcn_rsqf((float)__builtin_fma(u.z, u.z, __builtin_fma(u.y, u.y, u.x * u.x)));
    bool undecided = false;
    for (unsigned long long b = m.s; b; b &= b - 1) {
      const DSphere& S = p.spheres[__builtin_ctzll(b)];
      const int r = soft_screen(S.c[0], S.c[1], S.c[2], S.r2, P.x, P.y, P.z, u.x, u.y, u.z, il, 0.001, ldist);
      if (r == kSoftHit) return true;
      undecided |= r == kSoftUndecided;
    }
    if (!undecided) return false;
    soft_note();
  }
  return shadow_blocked<kCount, true, kMix>(p, masks, P, normalize(ldir + muls(pt, 0.1)), ldist, m, stack, c);
}
// (RT_WG_TIMING builds) a trace pass of soft_queue or soft_coop starts, ends
__device__ __forceinline__ void soft_pass_begin(int lane) {
#ifdef RT_WG_TIMING
  if (lane == 0) soft_note_flag = 0;
#endif
}
__device__ __forceinline__ void soft_pass_done(int lane) {
#ifdef RT_WG_TIMING
  if (lane == 0) {
    soft_pass_cnt[0] += 1;
    soft_pass_cnt[1] += soft_note_flag;
    soft_note_flag = 0;
  }
#endif
}

// ------------------------------------------------------------ wide mode
// When few lanes of a wave still run paths (the end of a block, where one
// long path sets the launch's critical path), the idle lanes help: every
// lane that needs a query (an "owner", at most 16) gets a group of
// S = 64 / next_pow2(owners) helper lanes, which split the primitive scan
// (primitive i goes to helper i mod S) and merge their results.  Only for
// sphere-only linear-scan scenes (no triangles): the merges below are exact
// for spheres.  wide_groups: the owner table (LDS), this lane's owner and its
// index within the group; S is returned.
__device__ __forceinline__ int wide_groups(bool need, unsigned long long qmask, int nq, int* owner_tab, int& ow,
                                           int& k, bool& helper) {
  const int lane = (int)(threadIdx.x & 63);
  const int S = nq <= 4 ? 16 : (nq <= 8 ? 8 : 4);
  if (need) owner_tab[lanes_below(qmask)] = lane;
  __syncthreads();
  const int grp = lane / S;
  k = lane - grp * S;
  helper = grp < nq;
  ow = helper ? owner_tab[grp] : lane;
  __syncthreads();  // the table is reused by the next call
  return S;
}

// hitWorld's closest hit over the spheres (the scene has no triangles), with
// helpers.  Each helper scans its spheres in hittable order with the
// sequential rule; the group then keeps the smallest t, and of equal t the
// larger hittable index (what the sequential scan ends with: a tie replaces
// the current hit unless its index is larger).  Exact for finite rays; an
// owner with a non-finite ray (or a = 0) is flagged in `fallback` and scans
// on its own.  Returns found for owner lanes.
template <bool kCount, bool kSph = false>
__device__ __forceinline__ bool closest_wide(const Geo& g, bool need, unsigned long long qmask, int nq, d3 o, d3 d,
                                             typename Kind<kSph>::H& hs, bool& fallback, Counters& c) {
  __shared__ int owner_tab[16];
  const int lane = (int)(threadIdx.x & 63);
  int ow, k;
  bool helper;
  const int S = wide_groups(need, qmask, nq, owner_tab, ow, k, helper);
  const d3 ro = mk(__shfl(o.x, ow), __shfl(o.y, ow), __shfl(o.z, ow));
  const d3 rd = mk(__shfl(d.x, ow), __shfl(d.y, ow), __shfl(d.z, ow));
  const double a = len2(rd);
  const double inv_a = approx_rcp(a);
  double bt = __builtin_inf(), bnum = 0;
  int bobj = -1, bidx = -1;
  bool found = false;
  if (helper) {
    for (int i = k; i < g.ns; i += S) {
      cnt<kCount>(c, C_SPH);
      const DSphere& Sp = g.spheres[i];
      double num;
      if (sphere_query(Sp, ro, rd, a, inv_a, 0.001, bt, num)) {
        const double t = num / a;
        if (t == bt && bobj > Sp.obj) continue;
        bt = t;
        bnum = num;
        bidx = i;
        bobj = Sp.obj;
        found = true;
      }
    }
  }
  for (int off = S >> 1; off >= 1; off >>= 1) {  // within the group (aligned to S)
    const double t2 = __shfl_xor(bt, off), n2 = __shfl_xor(bnum, off);
    const int o2 = __shfl_xor(bobj, off), i2 = __shfl_xor(bidx, off), f2 = __shfl_xor((int)found, off);
    if (f2 && (!found || t2 < bt || (t2 == bt && o2 > bobj))) {
      bt = t2;
      bnum = n2;
      bobj = o2;
      bidx = i2;
      found = true;
    }
  }
  const int lead = need ? lanes_below(qmask) * S : lane;
  const double fnum = __shfl(bnum, lead);
  const int fidx = __shfl(bidx, lead), ffound = __shfl((int)found, lead);
  fallback = need && !(__builtin_isfinite(o.x + o.y + o.z) && a > 0 && __builtin_isfinite(__shfl(a, lead)));
  hs.num = fnum;
  hs.idx = fidx;
  if constexpr (!kSph) hs.is_tri = 0;
  return ffound != 0;
}

// cone_candidates (spheres only) with helpers: each helper tests its
// spheres, the group ORs the bits.  Same tests, same mask.
// (kRows, the spheres-only stream kernels: a helper tests a sphere only if
// its owner's shadow-cone row -- `row`, cone_row below -- has it)
template <bool kRows = false>
__device__ __forceinline__ unsigned long long cone_wide(const Geo& g, bool need, unsigned long long qmask, int nq,
                                                        d3 P, d3 N, bool front, int self, d3 ldir, double ldist,
                                                        unsigned long long row = ~0ull) {
  __shared__ int owner_tab2[16];
  const int lane = (int)(threadIdx.x & 63);
  int ow, k;
  bool helper;
  const int S = wide_groups(need, qmask, nq, owner_tab2, ow, k, helper);
  const d3 Po = mk(__shfl(P.x, ow), __shfl(P.y, ow), __shfl(P.z, ow));
  const d3 Lo = mk(__shfl(ldir.x, ow), __shfl(ldir.y, ow), __shfl(ldir.z, ow));
  const double dist = __shfl(ldist, ow);
  const bool self_out = __shfl((int)(front && dot(N, ldir) >= KC(0.1015)), ow) != 0;
  const int selfo = __shfl(self, ow);
  unsigned long long rowo = ~0ull;
  if constexpr (kRows) rowo = __shfl(row, ow);
  unsigned long long m = 0;
  if (helper) {
    for (int i = k; i < g.ns; i += S) {
      const DSphere& Sp = g.spheres[i];
      if constexpr (kRows) {
        if (!((rowo >> i) & 1)) continue;
      }
      if (self_out && Sp.obj == selfo && Sp.r > 0) continue;
      if (in_cone(Sp.c, Sp.r, Po, Lo, dist)) m |= 1ull << i;
    }
  }
  for (int off = S >> 1; off >= 1; off >>= 1) m |= __shfl_xor(m, off);
  const int lead = need ? lanes_below(qmask) * S : lane;
  return __shfl(m, lead);
}

// ------------------------------------------------------------ inert lights
// (r05) A lit light whose shadow rays cannot change the shading: cos =
// Max(0, N.L) is 0, so calculateDirectLighting's intensity is 0 * I / d^2 =
// +0 and each term it adds is (finite) * 0 * shadowFactor * ... = +-0, and
// adding +-0 to D, which has no zero component, leaves D's bits unchanged --
// whether the term is added (shadow factor > 0) or not (= 0).  Finite means:
// the light's intensity and colour, the material's albedo, metallic and
// diffuse strength (the specular power is of a unit or zero half vector:
// Vec3.Normalize keeps zero, vector.go:61-67, so it is finite).  Such a
// light's hard and soft
// shadow rays are not traced (their result is not observable) and its soft
// points are not drawn (spec v4).  `D` is the ambient plus the terms of the
// lights before this one.
__device__ __forceinline__ bool light_inert(const DMat* m, const DLight& Lt, d3 N, d3 ldir, d3 D) {
  return gmax0(dot(N, ldir)) == 0.0 && D.x != 0.0 && D.y != 0.0 && D.z != 0.0 && __builtin_isfinite(Lt.intensity) &&
         __builtin_isfinite(Lt.color[0] + Lt.color[1] + Lt.color[2]) &&
         __builtin_isfinite(m->albedo[0] + m->albedo[1] + m->albedo[2]) && __builtin_isfinite(m->metallic) &&
         __builtin_isfinite(m->diffuse_strength);
}

// ------------------------------------------------------------ soft shadows
// Cooperative form for ONE owner lane, executed by the whole (converged)
// wave: lane h evaluates rejection try h of the owner's stream (draws
// 3h..3h+2 via the PCG jump table), a ballot picks the first `need`
// accepted tries in order, those lanes trace their rays, and the owner's
// stream advances by exactly the draws the sequential loop would consume.
// All arguments are wave-uniform (the owner's values, read from its lane).
struct CoopOut {
  uint64_t x;  // the owner's stream state after its 16 points
  int unocc;   // unoccluded rays
  int tries;   // rejection tries consumed
};
// the candidates of lane `ow`, wave-uniform
__device__ __forceinline__ Cand cand_of_lane(Cand m, int ow) { return Cand{rl64(m.s, ow), rl64(m.t, ow)}; }
__device__ __forceinline__ CandS cand_of_lane(CandS m, int ow) { return CandS{rl64(m.s, ow)}; }
template <bool kCount, bool kSph = false, bool kMix = false>
__device__ __forceinline__ CoopOut soft_coop(const Geo p, bool masks, bool trace, d3 P, d3 ldir, double ldist,
                             typename Kind<kSph>::C cm, uint64_t x, const uint64_t* jump, int* stack, Counters& c) {
  // (kSph: read where it is used -- the jump table's byte offset of the lane
  // is otherwise kept in a register pair through the whole bounce loop)
  const int lane = kSph ? lane_now() & 63 : (int)(threadIdx.x & 63);
  int need = 16, unocc = 0, tries = 0;
  while (need > 0) {
    const uint64_t x0 = state_at3(x, jump, lane), x1 = x0 * RT_PCG_MULT + RT_PCG_INC,
                   x2 = x1 * RT_PCG_MULT + RT_PCG_INC;
    const uint32_t o0 = rt_pcg_out(x0), o1 = rt_pcg_out(x1), o2 = rt_pcg_out(x2);
    const bool acc = unit_ball_accept(o0, o1, o2);
    const unsigned long long am = __ballot(acc);
    const int rank = lanes_below(am);
    const bool chosen = acc && rank < need;
    const unsigned long long chm = __ballot(chosen);
    const int nch = __popcll(chm);
    // tries consumed: up to and including the last chosen one
    const int used = nch == need ? 64 - __clzll(chm) : 64;
    bool occ = false;
    if constexpr (kSph) {
      if (trace) soft_pass_begin(lane);
      if (chosen && trace) occ = soft_blocked_sph<kCount, kMix>(p, masks, P, ldir, unit_ball_point(o0, o1, o2), ldist, cm, stack, c);
      if (trace) soft_pass_done(lane);
    } else {
      if (chosen && trace)
        occ = shadow_blocked<kCount, kSph, kMix>(p, masks, P, normalize(ldir + muls(unit_ball_point(o0, o1, o2), 0.1)), ldist,
                                           cm, stack, c);
    }
    unocc += nch - __popcll(__ballot(chosen && occ));
    need -= nch;
    tries += used;
    x = state_at3(x, jump, used);
  }
  return CoopOut{x, unocc, tries};
}

// Queue form for many owners (more than kCoopMax lanes need soft
// shadows for this light), executed by the whole converged wave.  Each
// owner runs its own rejection tries on its own stream, in order (the same
// draws as 16 calls of RandomVec3InUnitSphere); an accepted point is
// appended to an LDS queue as its three raw 32-bit draws and the owner's
// lane.  Whenever 64 points are queued, every lane takes one, rebuilds the
// point from the raw draws, reads the owner's hit point, light direction,
// distance and candidates across lanes, and traces the jittered ray.  The
// sequential form traced a ray in nearly every try step at about half the
// lanes; here the tries run alone and the rays run on full waves.  The
// result is a count of unoccluded rays, so the order in which rays are
// traced does not change it.  Returns the owner's count (0 elsewhere).
template <bool kCount, bool kSph = false, bool kMix = false>
__device__ __forceinline__ int soft_queue(const Geo& p, bool masks, bool need_soft, bool trace, d3 P, d3 ldir,
                                          double ldist, typename Kind<kSph>::C cm, rt_rng& rng, const uint64_t* jump,
                                          int* stack, Counters& c) {
  // queued points: raw draws x, y, z, owner lane (a ring).  It holds what
  // a pass can leave: < 64 points not yet traced, 64 per try of the pass and
  // 16 per owner of the cooperative tail (256 or more entries; a power of 2
  // up to 256, so the index is a mask there)
  constexpr int kRingNeed = 64 * kSqTries + 64 + 16 * kSqTail;
  constexpr unsigned kRing = kRingNeed <= 256 ? 256u : (unsigned)kRingNeed;
  __shared__ uint4 sq[kRing];
  __shared__ int sq_unocc[64];  // per owner: unoccluded rays
  const int lane = lane_now() & 63;
  sq_unocc[lane] = 0;
  int need = need_soft ? 16 : 0, free_rays = 0;  // free_rays: points of an owner with nothing to trace
  int head = 0, tail = 0;  // wave-uniform ring positions
  for (;;) {
    // kSqTries tries per pass: the later tries are drawn ahead and each
    // is consumed only when the owner still needs a point after the ones
    // before it (so the stream advances by exactly the draws the sequential
    // loop takes).
    constexpr int K = kSqTries;
    bool acc[K];
    uint32_t u[K][3];
#pragma unroll
    for (int t = 0; t < K; ++t) {
      acc[t] = false;
      u[t][0] = u[t][1] = u[t][2] = 0;
    }
    if (need > 0) {
      rt_rng r = rng;
#pragma unroll
      for (int t = 0; t < K; ++t) {
        u[t][0] = rt_rng_next(&r);
        u[t][1] = rt_rng_next(&r);
        u[t][2] = rt_rng_next(&r);
        if (need > 0) {
          rng = r;
          cnt<kCount>(c, C_RNG, 3);
          if (unit_ball_accept(u[t][0], u[t][1], u[t][2])) {
            --need;
            cnt<kCount>(c, C_SHADOW);
            if (trace) acc[t] = true;  // only rays that can be blocked are queued
            else ++free_rays;
          }
        }
      }
    }
#pragma unroll
    for (int t = 0; t < K; ++t) {
      const unsigned long long am = __ballot(acc[t]);
      if (acc[t]) sq[(unsigned)(tail + lanes_below(am)) % kRing] = make_uint4(u[t][0], u[t][1], u[t][2], (uint32_t)lane);
      tail += __popcll(am);
    }
    if constexpr (kSqTail > 0) {
      // The last few owners still drawing finish cooperatively, one at a
      // time: lane h evaluates try h of the owner's stream (jump table), as
      // in soft_coop; the first `need` accepted tries are its points, queued
      // in try order, and the stream advances past the last one taken.  The
      // wave no longer loops on its unluckiest owners' tries one by one.
      // (at most 16 points per owner: the ring holds them, see kRing)
      const unsigned long long rem = __ballot(need > 0);
      if (rem != 0 && __popcll(rem) <= kSqTail) {
        for (unsigned long long b = rem; b; b &= b - 1) {
          const int ow = __builtin_ctzll(b);
          int nd = __builtin_amdgcn_readlane(need, ow);
          const bool tr = __builtin_amdgcn_readlane(trace ? 1 : 0, ow) != 0;
          uint64_t x = rl64(rng.x, ow);
          int got = 0, tries = 0;
          while (nd > 0) {
            const uint64_t x0 = state_at3(x, jump, lane), x1 = x0 * RT_PCG_MULT + RT_PCG_INC,
                           x2 = x1 * RT_PCG_MULT + RT_PCG_INC;
            const uint32_t o0 = rt_pcg_out(x0), o1 = rt_pcg_out(x1), o2 = rt_pcg_out(x2);
            const bool acc = unit_ball_accept(o0, o1, o2);
            const unsigned long long am = __ballot(acc);
            const bool chosen = acc && lanes_below(am) < nd;
            const unsigned long long chm = __ballot(chosen);
            const int nch = __popcll(chm);
            const int used = nch == nd ? 64 - __clzll(chm) : 64;
            if (tr) {
              if (chosen) sq[(unsigned)(tail + lanes_below(chm)) % kRing] = make_uint4(o0, o1, o2, (uint32_t)ow);
              tail += nch;
            }
            got += nch;
            nd -= nch;
            tries += used;
            x = state_at3(x, jump, used);
          }
          if (lane == ow) {
            rng.x = x;
            need = 0;
            if (!tr) free_rays += got;
            cnt<kCount>(c, C_RNG, 3ull * tries);
            cnt<kCount>(c, C_SHADOW, got);
          }
        }
      }
    }
    const bool more = __ballot(need > 0) != 0;
    while (tail - head >= 64 || (!more && tail > head)) {
      __syncthreads();
      const int n = min(64, tail - head);
      const uint4 e = sq[(unsigned)(head + lane) % kRing];
      const int ow = lane < n ? (int)e.w : lane;
      // the owner's ray inputs, read across lanes (every lane takes part)
      const d3 Po = mk(__shfl(P.x, ow), __shfl(P.y, ow), __shfl(P.z, ow));
      const d3 Lo = mk(__shfl(ldir.x, ow), __shfl(ldir.y, ow), __shfl(ldir.z, ow));
      const double dist = __shfl(ldist, ow);
      typename Kind<kSph>::C co;
      co.s = __shfl(cm.s, ow);
      if constexpr (!kSph) co.t = p.nt ? __shfl(cm.t, ow) : 0ull;  // (no triangles: cm.t is 0)
      if constexpr (kSph) soft_pass_begin(lane);
      if (lane < n) {
        const d3 pt = mk(rt_bits_to_unit(e.x) * 2 - 1, rt_bits_to_unit(e.y) * 2 - 1, rt_bits_to_unit(e.z) * 2 - 1);
        bool blocked;
        if constexpr (kSph)
          blocked = soft_blocked_sph<kCount, kMix>(p, masks, Po, Lo, pt, dist, co, stack, c);
        else
          blocked = shadow_blocked<kCount, kSph, kMix>(p, masks, Po, normalize(Lo + muls(pt, 0.1)), dist, co, stack, c);
        if (!blocked) atomicAdd(&sq_unocc[ow], 1);
      }
      if constexpr (kSph) soft_pass_done(lane);
      head += n;
      __syncthreads();
    }
    if (!more && head == tail) break;
  }
  __syncthreads();
  return need_soft ? sq_unocc[lane] + free_rays : 0;
}

}  // namespace rtgo
