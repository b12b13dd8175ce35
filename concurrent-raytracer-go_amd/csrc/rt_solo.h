// rt_solo.h — the lone-path form (solo_path): the whole wave runs the one
// path left in it.  Called by render_body in RT_SOLO builds only, and by the
// tail helpers (rt_tail.h).
#pragma once
#include "rt_wg_clock.h"

// The lone-path form (solo_path): off by default since r05.
// Under RNG spec v4 a lone bounce is cheap, and the form no longer shortens
// anything (K = 20 frames 229.7 k vs 231.7 k Mrays/s without it, six rounds;
// one frame 0.574 vs 0.571 ms), while its call frames left ~47 MB of dirty
// scratch per one-frame launch (74.7 vs 18.6 MB of HBM traffic).  The
// cross-lane checking build compiles it in (Makefile xlane), so it stays
// tested; RT_SOLO=1 restores it.
#ifndef RT_SOLO
#define RT_SOLO 0
#endif

namespace rtgo {

// ------------------------------------------------------------ solo paths
// When a single path is left running in a wave (the end of a block, where
// a long metal-metal interreflection sets the launch's critical path), the
// idle lanes join it: every lane holds the path's state and computes the
// same binary64 values (the serial parts need no cross-lane traffic), while
// the loops over primitives run in parallel, one primitive per lane, with
// exact merges:
//   closest hit - every lane tests its primitives over [0.001, +inf); the
//     hits are then replayed in hittable scan order with hitWorld's rule
//     (accept t <= closest; an equal t only for a hittable index not below
//     the current one).  A root that Sphere.Hit rejects against a smaller
//     tMax is larger than that tMax, and so is the other root, so the replay
//     accepts exactly what the sequential scan accepts (renderer.go:333-346);
//   shadow cones and the hard shadow ray - a ballot of per-primitive tests
//     (an occlusion query has no order);
//   soft shadows - soft_coop (already wave-wide for one owner).
// The path runs to its end; then the main loop takes over again.  Linear-
// scan scenes with at most 64 spheres and 64 triangles (the staged scenes);
// the counting and pilot variants keep the per-lane loop.  (Lone bounce,
// 2 lights with soft shadows: 9.8 -> 6.1 us, scripts/latency_probe.py.
// Two paths in 32-lane groups, same scheme with shuffles, measured slower:
// headline 0.82 vs 0.775 ms, the group form's registers spill.)
__device__ __forceinline__ bool solo_closest(const Geo& g, d3 o, d3 d, HitSel& hs) {
  const int lane = (int)(threadIdx.x & 63);
  const double a = len2(d);
  const double inv_a = approx_rcp(a);
  double closest = __builtin_inf();
  int best_obj = -1;
  bool found = false;
  // lane i tests sphere i, then triangle i; the hits are replayed in
  // hittable scan order (spheres before triangles)
#pragma unroll
  for (int tri = 0; tri < 2; ++tri) {
    double t = 0, nm = 0, u = 0, v = 0;
    bool f;
    int myobj = 0;  // (the lane's hittable index, read with its primitive: the replay takes it by readlane)
    if (!tri) {
      f = false;
      if (lane < g.ns) {
        const DSphere& S = g.spheres[lane];
        myobj = S.obj;
        f = sphere_query(S, o, d, a, inv_a, 0.001, __builtin_inf(), nm) != 0;
      }
      if (f) t = nm / a;
    } else {
      f = false;
      if (lane < g.nt) {
        myobj = g.tris[lane].obj;
        f = tri_test(g.tris[lane], o, d, 0.001, __builtin_inf(), t, u, v);
      }
    }
    for (unsigned long long b = __ballot(f); b; b &= b - 1) {
      const int i = __builtin_ctzll(b);
      const double ti = rld(t, i);
      const int obj = (int)rl32((uint32_t)myobj, i);
      if (closest < ti || (ti == closest && best_obj > obj)) continue;
      closest = ti;
      best_obj = obj;
      hs.num = tri ? ti : rld(nm, i);
      if (tri) {
        hs.u = rld(u, i);
        hs.v = rld(v, i);
      }
      hs.idx = i;
      hs.is_tri = tri;
      found = true;
    }
  }
  return found;
}

// ---- parallel direct lighting of a lone path (solo_lights)
// The tries of a bounce's soft-shadow streams, evaluated ahead: try k of the
// stream whose state is x uses draws 3k, 3k+1, 3k+2 (RandomVec3InUnitSphere,
// vector.go:132-139); lane h holds try h of light 0's stream (a) and of light
// 1's (b) (spec v4, include/rt_rng.h: each (sample, bounce, light) has a
// stream of its own).  A light whose hard ray is clear takes the first 16
// accepted tries of its stream, so all lights' soft rays are known once the
// hard rays are, and can be traced at once.
struct SoloTries {
  uint32_t a0, a1, a2, b0, b1, b2;  // the draws of try h of stream a, of stream b
  unsigned long long ma, mb;        // accepted tries 0..63 of each (wave-uniform)
};
__device__ __forceinline__ SoloTries solo_tries(uint64_t xa, uint64_t xb, uint64_t jA, uint64_t jC) {
  SoloTries t;
  uint64_t s = jA * xa + jC;  // state before draw 3h of stream a
  t.a0 = rt_pcg_out(s);
  s = s * RT_PCG_MULT + RT_PCG_INC;
  t.a1 = rt_pcg_out(s);
  s = s * RT_PCG_MULT + RT_PCG_INC;
  t.a2 = rt_pcg_out(s);
  s = jA * xb + jC;  // ... of stream b
  t.b0 = rt_pcg_out(s);
  s = s * RT_PCG_MULT + RT_PCG_INC;
  t.b1 = rt_pcg_out(s);
  s = s * RT_PCG_MULT + RT_PCG_INC;
  t.b2 = rt_pcg_out(s);
  t.ma = __ballot(unit_ball_accept(t.a0, t.a1, t.a2));
  t.mb = __ballot(unit_ball_accept(t.b0, t.b1, t.b2));
  return t;
}
// The index after the 16th accepted try of each stream's 64 (-1: fewer):
// every lane ranks its tries among the accepted ones (v_mbcnt) and two
// ballots find the 16th of each
__device__ __forceinline__ void solo_take16(const SoloTries& t, int& ia, int& ib) {
  const int lane = (int)(threadIdx.x & 63);
  const bool aa = (t.ma >> lane) & 1ull, ab = (t.mb >> lane) & 1ull;
  const unsigned long long a16 = __ballot(aa && lanes_below(t.ma) + 1 == 16);
  const unsigned long long b16 = __ballot(ab && lanes_below(t.mb) + 1 == 16);
  ia = a16 ? __builtin_ctzll(a16) + 1 : -1;
  ib = b16 ? __builtin_ctzll(b16) + 1 : -1;
}

// The path of lane `ow`, run to its end by the whole wave: its radiance.
// A real call (RT_SOLO_CALL, the default): its registers then do not add to
// the shade loop's, whose per-iteration scratch spills they caused when it
// was inlined.  A callee has no kernarg segment pointer of
// its own -- __builtin_amdgcn_kernarg_segment_ptr() lowers to a null pointer
// outside a kernel entry point, which is what made round 4's non-inlined
// variant fault on its first parameter load -- so the kernel passes it in
// (`karg`) and every per-bounce read launders that copy (launder()).
#ifndef RT_SOLO_CALL
#define RT_SOLO_CALL 0
#endif
#if RT_SOLO_CALL
#define RT_SOLO_ATTR __noinline__
#else
#define RT_SOLO_ATTR __forceinline__
#endif
__device__ __forceinline__ KArg launder(KArg k) {
  // (a call's arguments arrive in VGPRs: made wave-uniform first)
  const uint64_t v = (uint64_t)(uintptr_t)k;
  const uint32_t lo = __builtin_amdgcn_readfirstlane((uint32_t)v), hi = __builtin_amdgcn_readfirstlane((uint32_t)(v >> 32));
  KArg r = (KArg)(uintptr_t)(((uint64_t)hi << 32) | lo);
  asm volatile("" : "+s"(r));
  return r;
}
template <bool kSky>
__device__ RT_SOLO_ATTR d3 solo_path(KArg karg, int ow, d3 o, d3 d, d3 T, d3 L, uint64_t rx, int depth,
                                     uint64_t skey, int* stack, int* dep_out = nullptr) {
  const int lane = (int)(threadIdx.x & 63);
  o = rl3(o, ow);
  d = rl3(d, ow);
  T = rl3(T, ow);
  L = rl3(L, ow);
  rt_rng rng{rl64(rx, ow)};
  depth = (int)rl32((uint32_t)depth, ow);
  Counters c;
  WgClock clk;  // (the lone path's section clocks, RT_WG_TIMING builds)
  clk.solo_start();
  // the parallel lighting form (solo_lights): sphere-only scenes with one or
  // two lights, a (light, sphere) pair per lane
  bool par;
  // jump coefficients of try `lane` (solo_tries), held in VGPRs for the
  // lone path's bounces: no memory access per bounce
  uint64_t jA, jC;
  {
    const Hot h0 = hot<true>(launder(karg));
    par = h0.g.nt == 0 && h0.nl >= 1 && h0.nl <= 2 && h0.nl * h0.g.ns <= 64;
    jA = h0.jump[2 * lane];
    jC = h0.jump[2 * lane + 1];
  }
  clk.solo_count(7);
  for (;;) {
    const Hot h = hot<true>(launder(karg));
    const Geo& g = h.g;
    if (depth >= h.max_depth) {  // traceRay depth cut-off: contributes 0
      if (dep_out) *dep_out = depth;
      return path_end(L, T);
    }
    clk.solo_count(6);
    // (1) closest hit (hitWorld, renderer.go:170)
    HitSel hs;
    const bool found = solo_closest(g, o, d, hs);
    clk.solo_lap(0);
    if (!found) {  // miss -> black (or the opted-in sky)
      if constexpr (kSky) L = L + mul(T, sky_color(launder(karg)->sky, d));
      if (dep_out) *dep_out = depth + 1;
      return path_end(L, T);
    }
    d3 P, N;
    bool front;
    int mi, self;
    if (!hs.is_tri) {  // sphere.go:42-58
      const DSphere& S0 = g.spheres[hs.idx];
      const double t = hs.num / len2(d);
      P = o + muls(d, t);
      d3 outward = divs(P - ld3(S0.c), S0.r);
      front = dot(d, outward) < 0;
      N = front ? outward : neg(outward);
      mi = S0.mat;
      self = S0.obj;
    } else {  // triangle.go:68-81
      const DTri& T0 = g.tris[hs.idx];
      P = o + muls(d, hs.num);
      double w = 1.0 - hs.u - hs.v;
      d3 n = ld3(T0.n);
      N = normalize((muls(n, w) + muls(n, hs.u)) + muls(n, hs.v));
      front = dot(d, N) < 0;
      if (!front) N = neg(N);
      mi = T0.mat;
      self = T0.obj;
    }
    clk.solo_lap(1);
    // (2) calculateDirectLighting (renderer.go:229-297)
    const DMat* __restrict__ m = h.mats + mi;
    d3 D = mk(m->ambient, m->ambient, m->ambient);
    if (par) {
      // every light at once: lane li (< nl) its light vector; lane
      // li * ns + s the pair (light li, sphere s) for the shadow cone and the
      // hard ray; then all lights' soft rays from the tries; then the
      // lighting terms per lane li, added to D in light order (the same
      // operations and sums as the loop below, so the same bits)
      const int nl = h.nl, ns = g.ns;
      SoloTries tr{};
      if (h.soft) tr = solo_tries(rt_soft_state(skey, (uint32_t)depth, 0u), rt_soft_state(skey, (uint32_t)depth, 1u), jA, jC);
      clk.solo_mark(8);
      d3 lvd = mk(0, 0, 0);
      double lvl = 0;
      // the lighting terms' parts that do not depend on the shadows (lane
      // li < nl, light li): diffuse_strength * intensity and si * intensity,
      // the left operands of calculateDirectLighting's products, computed
      // here so their square roots and divisions overlap the light vector's
      // (the same operations in the same order: the same bits)
      double di = 0, sii = 0;
      const double metallic = m->metallic;
      if (lane < nl) {
        const d3 lv = ld3(h.lights[lane].pos) - P;
        const d3 view = normalize(neg(P));  // (independent of the light: interleaves with lv's chain)
        lvl = sqrt(lv.x * lv.x + lv.y * lv.y + lv.z * lv.z);
        lvd = lvl == 0 ? mk(0, 0, 0) : divs(lv, lvl);
        const double cos_t = gmax0(dot(N, lvd));
        const double intensity = cos_t * h.lights[lane].intensity / (lvl * lvl);
        di = m->diffuse_strength * intensity;
        if (metallic > 0.5) {
          const d3 half = normalize(lvd + view);
          const double hc = gmax0(dot(N, half));
          const int sp = m->spec_pow;
          const double si = sp == 64 ? pow_n<64>(hc) : (sp == 48 ? pow_n<48>(hc) : pow_n<32>(hc));
          sii = si * intensity;
        }
      }
      // (light values move across lanes by shuffles where they are used: held
      // as wave-uniform values they would take SGPRs the bounce loop needs)
      const unsigned long long litm = __ballot(lane < nl && !(lvl < 0.001));
      clk.solo_mark(9);
      const int lj = lane >= ns ? 1 : 0, sj = lane - lj * ns;  // this lane's pair
      const d3 ldj = mk(__shfl(lvd.x, lj), __shfl(lvd.y, lj), __shfl(lvd.z, lj));
      const double dlj = __shfl(lvl, lj);
      clk.solo_mark(10);
      bool cone = false, blk = false;
      if (lane < nl * ns && ((litm >> lj) & 1ull)) {
        const DSphere& S = g.spheres[sj];
        const bool self_out = front && dot(N, ldj) >= KC(0.1015);
        cone = !(self_out && S.obj == self && S.r > 0) && in_cone(S.c, S.r, P, ldj, dlj);
        // the hard ray against every sphere, as hitWorld does, independent
        // of the cone test so the two chains overlap (a sphere outside the
        // cone cannot be hit: the same answer as testing the candidates only)
        const double a = len2(ldj);
        double num;
        blk = sphere_query(S, P, ldj, a, approx_rcp(a), 0.001, dlj, num) != 0;
      }
      const unsigned long long cones = __ballot(cone), blks = __ballot(blk);
      clk.solo_mark(11);
      const unsigned long long sm = ns >= 64 ? ~0ull : (1ull << ns) - 1ull;
      const unsigned long long cm0 = cones & sm, cm1 = (cones >> ns) & sm;
      const bool lit0 = litm & 1ull, lit1 = (litm >> 1) & 1ull;
      const bool occ0 = (blks & sm) != 0, occ1 = ((blks >> ns) & sm) != 0;
      const bool need0 = lit0 && !occ0 && h.soft, need1 = lit1 && !occ1 && h.soft;
      // soft rays: each light takes the first 16 accepted tries of its own
      // stream (spec v4; a light without soft rays draws nothing)
      int i16a = -1, i16b = -1;
      solo_take16(tr, i16a, i16b);
      const int e0 = need0 ? i16a : 0, e1 = need1 ? i16b : 0;
      clk.solo_lap(2);
      int un0 = 16, un1 = 16;
      if (e0 >= 0 && e1 >= 0) {
        int cnt0 = 0, cnt1 = 0;
#pragma unroll
        for (int half = 0; half < 2; ++half) {  // light 0 (stream a), then light 1 (stream b)
          if (half == 1 && !need1) break;
          if (half == 0 && !need0) continue;
          const bool acc = ((half ? tr.mb : tr.ma) >> lane) & 1ull;
          const bool in = lane < (half ? e1 : e0);
          const d3 lD = mk(__shfl(lvd.x, half), __shfl(lvd.y, half), __shfl(lvd.z, half));
          const double lT = __shfl(lvl, half);
          bool occ = false;
          if (acc && in) {
            const d3 pt = half ? unit_ball_point(tr.b0, tr.b1, tr.b2) : unit_ball_point(tr.a0, tr.a1, tr.a2);
            const d3 sd = normalize(lD + muls(pt, 0.1));
            const double a = len2(sd);
            const double ia = approx_rcp(a);
            // (every candidate, no early exit: their loads issue together)
            for (unsigned long long b = half ? cm1 : cm0; b; b &= b - 1) {
              double num;
              occ = (sphere_query(g.spheres[__builtin_ctzll(b)], P, sd, a, ia, 0.001, lT, num) != 0) || occ;
            }
          }
          (half ? cnt1 : cnt0) = __popcll(__ballot(acc && in && !occ));
          if (half == 0) clk.solo_mark(12);
        }
        clk.solo_mark(13);
        un0 = cnt0;
        un1 = cnt1;
      } else {
        // (64 tries of a stream did not hold 16 points: that light's soft
        // rays cooperatively from its stream, as below)
        for (int li = 0; li < 2; ++li) {
          if (!(li ? need1 : need0)) continue;
          const Cand cl{li ? cm1 : cm0, 0ull};
          const CoopOut r = soft_coop<false>(g, true, cl.s != 0, P, rl3(lvd, li), rld(lvl, li), cl,
                                             rt_soft_state(skey, (uint32_t)depth, (uint32_t)li), h.jump, stack, c);
          (li ? un1 : un0) = r.unocc;
        }
      }
      clk.solo_lap(3);
      // the lighting terms of light lane (< nl), then D in light order
      d3 tdif = mk(0, 0, 0), tspec = mk(0, 0, 0);
      if (lane < nl) {
        const bool occ = lane ? occ1 : occ0;
        const int un = lane ? un1 : un0;
        const double sf = occ ? 0.0 : (h.soft ? (double)un / 16.0 : 1.0);  // shadowSum / 16
        tdif = muls(ld3(m->albedo), di * sf);
        if (metallic > 0.5) tspec = muls(ld3(h.lights[lane].color), sii * sf * metallic * 3.0);
      }
      clk.solo_mark(14);
#pragma unroll
      for (int li = 0; li < 2; ++li) {
        if (li >= nl) break;
        const bool lit = li ? lit1 : lit0, occ = li ? occ1 : occ0;
        const int un = li ? un1 : un0;
        const double sf = occ ? 0.0 : (h.soft ? (double)un / 16.0 : 1.0);
        if (lit && sf > 0.0) {
          D = D + rl3(tdif, li);
          if (metallic > 0.5) D = D + rl3(tspec, li);
        }
      }
      clk.solo_lap(4);
    } else
    for (int li = 0; li < h.nl; ++li) {
      const DLight& Lt = h.lights[li];
      const d3 lv = ld3(Lt.pos) - P;
      const double ldist = sqrt(lv.x * lv.x + lv.y * lv.y + lv.z * lv.z);
      const d3 ldir = ldist == 0 ? mk(0, 0, 0) : divs(lv, ldist);
      if (ldist < 0.001) continue;  // renderer.go:252-254
      // the shadow cone's candidates, one primitive per lane (cone_candidates)
      const bool leaves = dot(N, ldir) >= KC(0.1015);
      bool cs = false, cb = false;
      if (lane < g.ns) {
        const DSphere& S = g.spheres[lane];
        cs = !(front && leaves && S.obj == self && S.r > 0) && in_cone(S.c, S.r, P, ldir, ldist);
      }
      if (lane < g.nb) {  // (nb <= 5: 12 triangles per cube)
        const DBox& B = g.boxes[lane];
        cb = !(leaves && B.obj == self && box_self_out(B, front)) && in_cone(B.bc, B.br, P, ldir, ldist);
      }
      Cand cm{__ballot(cs), 0ull};
      for (unsigned long long b = __ballot(cb); b; b &= b - 1) cm.t |= 0xFFFull << g.boxes[__builtin_ctzll(b)].first;
      // the hard shadow ray (renderer.go:305), the candidates in parallel
      bool blk = false;
      if ((cm.s >> lane) & 1ull) {
        const double a = len2(ldir);
        double num;
        blk = sphere_query(g.spheres[lane], P, ldir, a, approx_rcp(a), 0.001, ldist, num) != 0;
      }
      if ((cm.t >> lane) & 1ull) {
        double t, u, v;
        blk = blk || tri_test(g.tris[lane], P, ldir, 0.001, ldist, t, u, v);
      }
      const bool occl = __ballot(blk) != 0;
      int unocc = 0;
      if (!occl && h.soft) {
        // the 16 soft rays (renderer.go:311-327), not traced for an inert light
        const bool trace = (cm.s | cm.t) != 0 && !light_inert(m, Lt, N, ldir, D);
        // (spec v4: the points come from the light's own stream; rays that
        // cannot be blocked need none of them)
        if (trace) {
          const CoopOut r = soft_coop<false>(g, true, true, P, ldir, ldist, cm,
                                             rt_soft_state(skey, (uint32_t)depth, (uint32_t)li), h.jump, stack, c);
          unocc = r.unocc;
        } else {
          unocc = 16;
        }
      }
      const double sf = occl ? 0.0 : (h.soft ? (double)unocc / 16.0 : 1.0);  // shadowSum / 16
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
    // (3) Material.Scatter and the traceRay combination (renderer.go:181-226)
    const d3 E = ld3(m->emit);
    const Scat sc = scatter<false>(m, d, N, front, rng, c);
    clk.solo_lap(5);
    if (!sc.ok) {
      if (dep_out) *dep_out = depth + 1;
      return path_end(L + mul(T, E + D), T);
    }
    L = L + mul(T, E + muls(D, m->dw));
    path_step(T, L, sc.A, m->rw);  // (rt_device.h: also before a last bounce, whose black is multiplied too)
    if (!h.recursive || depth + 1 >= h.max_depth) {
      if (dep_out) *dep_out = depth + 1;
      return path_end(L, T);
    }
    o = P;
    d = sc.nd;
    depth += 1;
  }
}

}  // namespace rtgo
