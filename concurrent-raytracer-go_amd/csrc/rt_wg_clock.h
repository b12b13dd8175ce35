// rt_wg_clock.h — WgClock: the per-workgroup clocks and records of an
// RT_WG_TIMING build (make timing), empty methods in every other build.
#pragma once
#include "rt_blocks.h"

namespace rtgo {

// ------------------------------------------------------------ workgroup clocks
// RT_WG_TIMING builds (make timing; scripts/wg_timing.py and
// scripts/latency_probe.py read the records): every counter and stamp of a
// workgroup, and the writers of its kDbgStride words of KParams.dbg.  In every
// other build the struct is empty and so is each method, so render_body,
// solo_path and tail_helper call them unconditionally.
//   a block's (or a stream wave's) record: r[0] start, r[1] loop end, r[2] end
//     (s_memrealtime); r[3..12] wave-uniform section clocks (s_memtime) and
//     counts: hit, lighting, soft, phase 1 (visibility), shade iterations,
//     cone + hard shadow, scatter, lane-iterations alive, coop owners served,
//     soft_queue passes; r[13] np * 65536 + ns, r[14] split slot + 1 (a stream
//     wave: 0, 0); r[15] the soft shadows' trace passes (soft_pass_done), and
//     shifted left by 32 those of them that a lane marked (soft_note,
//     rt_device.h); r[16 + i] the stamp of shade iteration 4 i (i < 16), or --
//     when a lone path ran -- its section clocks; r[32..36] / r[37..41]
//     shade-iteration clocks / counts by live lanes (1, 2, 3-4, 5-8, > 8);
//     r[42] lone-path bounces, r[43] entries into solo_path; (a stream wave)
//     r[44] / r[45] shade iterations whose top-of-loop refill set up at least
//     one entry / the lanes those served, r[46] / r[47] the same of the
//     second-pass refill;
//   a tail helper's record: r[0] start, r[1] first path, r[2] end, r[3] ticks in
//     solo_path, r[4..6] the last path's start and its depth when exported and
//     at its end, r[7] paths, r[8] their bounces, r[14] = -1;
//   a lone path's bounce by section (solo_clk[k], wave-uniform; PROBE_SECTIONS
//     of scripts/latency_probe.py): 0 loop top + closest hit, 1 hit record,
//     2 stream tries + light vectors + cones + hard rays, 3 soft rays,
//     4 lighting terms, 5 scatter, 6 bounces, 7 entries; solo_mark(k), k >= 8:
//     clocks from the start of the current section to that point of it (the
//     parallel-lights form: 8 tries, 9 light vectors, 10 their shuffles,
//     11 cones + hard rays + ballots; 12 the soft rays of tries 0..63, 13 of
//     tries 64..127; 14 the lighting terms before the sum).
enum WgSection { kClkHit, kClkLight, kClkSoft, kClkHard, kClkScat };
#ifdef RT_WG_TIMING
__shared__ unsigned long long solo_clk[16];
struct WgClock {
  unsigned long long t_start = 0, t_loop = 0, iter = 0;
  unsigned long long sec[5] = {0, 0, 0, 0, 0}, from[5] = {0, 0, 0, 0, 0};  // by WgSection: clocks, start of the open one
  unsigned long long vis = 0, alive = 0, coop = 0, seq = 0;
  unsigned long long rf_top = 0, rf_top_lanes = 0, rf_second = 0, rf_second_lanes = 0;  // (kStream) refills, see refill()
  // by live lanes (vectors: indexed by a variable, and an array member so
  // indexed would keep the whole struct in scratch)
  typedef unsigned long long Buckets __attribute__((ext_vector_type(5)));
  Buckets bclk = {0, 0, 0, 0, 0}, bcnt = {0, 0, 0, 0, 0};
  unsigned long long bts = 0;
  int bprev = -1;
  unsigned long long solo_t0 = 0;  // solo_path: start of the current section
  // tail_helper: first and last path's start, the last one's depths, paths, their ticks and bounces
  unsigned long long first = 0, last = 0, last_d0 = 0, last_d1 = 0, paths = 0, solo = 0, bounces = 0;

  __device__ __forceinline__ unsigned long long* record(KArg k) const { return k->dbg + (size_t)blockIdx.x * kDbgStride; }
  __device__ __forceinline__ void start(int lane) {
    if (lane < 16) solo_clk[lane] = 0;
    if (lane < 2) soft_pass_cnt[lane] = 0;
    t_start = __builtin_amdgcn_s_memrealtime();
    vis = __builtin_amdgcn_s_memtime();
  }
  __device__ __forceinline__ void visibility_done() { vis = __builtin_amdgcn_s_memtime() - vis; }
  // a shade iteration starts with `alive` lanes running paths (pass 0); opens kClkHit
  __device__ __forceinline__ void iteration(bool is_alive, int lane) {
    ++iter;
    alive += __popcll(__ballot(is_alive));
    {
      const unsigned long long now = __builtin_amdgcn_s_memtime();
      if (bprev >= 0) bclk[bprev] += now - bts;
      const int nal = __popcll(__ballot(is_alive));
      bprev = nal == 1 ? 0 : (nal == 2 ? 1 : (nal <= 4 ? 2 : (nal <= 8 ? 3 : 4)));
      bcnt[bprev] += 1;
      bts = now;
    }
    if (iter % 4 == 0 && iter / 4 < 16 && lane == 0 && fresh()->dbg) record(fresh())[16 + iter / 4] = __builtin_amdgcn_s_memrealtime();
    from[kClkHit] = __builtin_amdgcn_s_memtime();
  }
  __device__ __forceinline__ void begin(WgSection s) { from[s] = __builtin_amdgcn_s_memtime(); }
  __device__ __forceinline__ void end(WgSection s) { sec[s] += __builtin_amdgcn_s_memtime() - from[s]; }
  // kClkHit ends where kClkLight begins: one clock read
  __device__ __forceinline__ void hit_done() {
    from[kClkLight] = __builtin_amdgcn_s_memtime();
    sec[kClkHit] += from[kClkLight] - from[kClkHit];
  }
  __device__ __forceinline__ void soft_form(unsigned long long owners) {
    if (__popcll(owners) <= kCoopMax) coop += __popcll(owners); else ++seq;
  }
  // (kStream) a refill set up the entries of the lanes of `served`: at the top
  // of a shade iteration, or ahead of its second closest-hit pass
  __device__ __forceinline__ void refill(bool second, unsigned long long served) {
    if (served == 0) return;
    if (second) {
      rf_second += 1;
      rf_second_lanes += __popcll(served);
    } else {
      rf_top += 1;
      rf_top_lanes += __popcll(served);
    }
  }
  __device__ __forceinline__ void loop_done() {
    t_loop = __builtin_amdgcn_s_memrealtime();
    if (bprev >= 0) bclk[bprev] += __builtin_amdgcn_s_memtime() - bts;
  }
  // the record of a block (shape = np * 65536 + ns, split = slot + 1) or of a
  // stream wave (block = false: zeros there and for the lone-path words)
  __device__ __forceinline__ void write(KArg k, int lane, bool block, unsigned long long shape, unsigned long long split) const {
    if (k->dbg && lane == 0) {
      unsigned long long* r = record(k);
      r[0] = t_start;
      r[1] = t_loop;
      r[2] = __builtin_amdgcn_s_memrealtime();
      r[3] = sec[kClkHit];
      r[4] = sec[kClkLight];
      r[5] = sec[kClkSoft];
      r[6] = vis;
      r[7] = iter;
      r[8] = sec[kClkHard];
      r[9] = sec[kClkScat];
      r[10] = alive;
      r[11] = coop;
      r[12] = seq;
      r[13] = shape;
      r[14] = split;
      r[15] = soft_pass_cnt[0] | soft_pass_cnt[1] << 32;
      for (int i = 0; i < 5; ++i) {
        r[32 + i] = bclk[i];
        r[37 + i] = bcnt[i];
      }
      if (block && solo_clk[6])  // a lone path ran: its section clocks replace the iteration stamps
        for (int i = 0; i < 16; ++i) r[16 + i] = solo_clk[i];
      r[42] = block ? solo_clk[6] : 0;  // lone-path bounces (0: none ran)
      r[43] = block ? solo_clk[7] : 0;  // entries into solo_path
      r[44] = rf_top;
      r[45] = rf_top_lanes;
      r[46] = rf_second;
      r[47] = rf_second_lanes;
    }
  }
  __device__ __forceinline__ void stream_write(int lane) const { write(fresh(), lane, false, 0, 0); }
  // solo_path
  __device__ __forceinline__ void solo_start() { solo_t0 = __builtin_amdgcn_s_memtime(); }
  __device__ __forceinline__ void solo_count(int k) { solo_clk[k] += 1; }
  __device__ __forceinline__ void solo_lap(int k) {  // section k ends here, the next one starts
    const unsigned long long now = __builtin_amdgcn_s_memtime();
    solo_clk[k] += now - solo_t0;
    solo_t0 = now;
  }
  __device__ __forceinline__ void solo_mark(int k) { solo_clk[k] += __builtin_amdgcn_s_memtime() - solo_t0; }
  // tail_helper: a path taken at t_path ran from depth d0 to d1; the helper's record at its end
  __device__ __forceinline__ void helper_path(unsigned long long t_path, int d0, int d1) {
    if (!first) first = t_path;
    paths += 1;
    solo += __builtin_amdgcn_s_memrealtime() - t_path;
    last = t_path;
    last_d0 = (unsigned long long)d0;
    last_d1 = (unsigned long long)d1;
    bounces += (unsigned long long)(d1 - d0);
  }
  __device__ __forceinline__ void helper_write(KArg k, int lane, unsigned long long t_born) const {
    if (k->dbg && lane == 0) {
      unsigned long long* r = record(k);
      r[0] = t_born;
      r[1] = first;
      r[2] = __builtin_amdgcn_s_memrealtime();
      r[3] = solo;
      r[4] = last;     // the last path's start,
      r[5] = last_d0;  // its depth when exported,
      r[6] = last_d1;  // and at its end
      r[7] = paths;
      r[8] = bounces;
      r[14] = ~0ull;
    }
  }
};
#else
struct WgClock {
  __device__ __forceinline__ void start(int) {}
  __device__ __forceinline__ void visibility_done() {}
  __device__ __forceinline__ void iteration(bool, int) {}
  __device__ __forceinline__ void begin(WgSection) {}
  __device__ __forceinline__ void end(WgSection) {}
  __device__ __forceinline__ void hit_done() {}
  __device__ __forceinline__ void soft_form(unsigned long long) {}
  __device__ __forceinline__ void refill(bool, unsigned long long) {}
  __device__ __forceinline__ void loop_done() {}
  __device__ __forceinline__ void write(KArg, int, bool, unsigned long long, unsigned long long) const {}
  __device__ __forceinline__ void stream_write(int) const {}
  __device__ __forceinline__ void solo_start() {}
  __device__ __forceinline__ void solo_count(int) {}
  __device__ __forceinline__ void solo_lap(int) {}
  __device__ __forceinline__ void solo_mark(int) {}
  __device__ __forceinline__ void helper_path(unsigned long long, int, int) {}
  __device__ __forceinline__ void helper_write(KArg, int, unsigned long long) const {}
};
#endif

}  // namespace rtgo
