// rt_tail.h — the tail helpers of render_kernel_tail: write-through loads and
// stores, the row sum, the helper workgroups' loop and the main blocks' side
// of the hand-over.
#pragma once
#include "rt_solo.h"

namespace rtgo {

// ---- tail helpers (TailCtl in rt_internal.h)
// Device-scope hand-offs on MI355X (MI355X_MICROARCH.md, inter-workgroup
// visibility): the 8 XCDs' L2 caches are not coherent with each other, and an
// agent-scope release fence writes back the whole XCD L2's dirty lines
// (buffer_wbl2: microseconds, and tens of them when many waves fence at
// once).  The tail protocol hands its data over WITHOUT fences, in the
// guide's "8-B agent atomics both sides" form: every byte a helper or a
// block hands over (a queued path, a row's samples, bits and header) is
// stored write-through with relaxed agent-scope atomic stores (st_wt*, sc1),
// the storing wave drains them (s_waitcnt vmcnt(0)), and only then stores
// the flag or adds to the counter that signals them; the consumer polls the
// flag or takes the counter's returned value and reads every handed-over
// byte with relaxed agent-scope atomic loads (ld_wt*, sc1).  Counters that
// every block touches are sharded (TailCtl.done), and the export's gate
// reads before it adds.  (Measured on the headline frame: a __threadfence
// at every block's end, or 2 atomics per draining iteration on one line,
// made the launch 2-3x slower.)
__device__ __forceinline__ unsigned int ld_rlx(const unsigned int* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void wt_drain() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
__device__ __forceinline__ void st_wt64(void* p, uint64_t v) {
  __hip_atomic_store(reinterpret_cast<uint64_t*>(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_wt32(void* p, uint32_t v) {
  __hip_atomic_store(reinterpret_cast<uint32_t*>(p), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_wtd(double* p, double v) { st_wt64(p, __builtin_bit_cast(uint64_t, v)); }
__device__ __forceinline__ uint64_t ld_wt64(const void* p) {
  return __hip_atomic_load(reinterpret_cast<const uint64_t*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t ld_wt32(const void* p) {
  return __hip_atomic_load(reinterpret_cast<const uint32_t*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ double ld_wtd(const double* p) { return __builtin_bit_cast(double, ld_wt64(p)); }
// Samples [k0, n) of a per-sample radiance row added to `a` (lanes 0..2:
// channel `lane`) in sample order, a sample whose hit bit is clear adding +0
// (a miss: traceRay's black, renderer.go:170-173, summed as tracePixel sums,
// renderer.go:150-163).  The whole wave loads each chunk of kRound samples
// into `buf` (LDS); lanes 0..2 then add it in order.
// (kWT: the row was handed over write-through: every load of it is sc1)
template <bool kWT>
__device__ __forceinline__ double row_sum(double (*buf)[3], const double* row, const uint32_t* hw, int k0, int n,
                                          double a, int lane) {
  for (int c0 = k0; c0 < n; c0 += kRound) {
    const int cn = min(kRound, n - c0);
    for (int i = lane; i < cn; i += 64) {
      const int s = c0 + i;
      const bool hit = ((kWT ? ld_wt32(hw + (s >> 5)) : hw[s >> 5]) >> (s & 31)) & 1u;
      buf[i][0] = hit ? (kWT ? ld_wtd(row + 3 * s + 0) : row[3 * s + 0]) : 0.0;
      buf[i][1] = hit ? (kWT ? ld_wtd(row + 3 * s + 1) : row[3 * s + 1]) : 0.0;
      buf[i][2] = hit ? (kWT ? ld_wtd(row + 3 * s + 2) : row[3 * s + 2]) : 0.0;
    }
    __syncthreads();
    if (lane < 3)
      for (int i = 0; i < cn; ++i) a += buf[i][lane];
    __syncthreads();
  }
  return a;
}

// A tail helper: one of the one-wave workgroups past the grid's main blocks.
// It takes exported paths off the queue and runs each to its end with the
// whole wave (solo_path), delivers its radiance to the row of its pixel and,
// when it is the pixel's last contributor, sums the row and writes the
// pixel.  It leaves once every main block has finished and the queue is
// empty (main blocks never wait for a helper, so that always comes); the last
// helper to leave zeroes the control block for the context's next launch.
__device__ __forceinline__ void tail_helper(KArg karg, int* stack, double (*buf)[3]) {
  const int lane = (int)(threadIdx.x & 63);
  const KArg k0 = launder(karg);
  TailCtl* const ctl = k0->tail;
  const unsigned int epoch = k0->tail_epoch, cap = (unsigned int)k0->tail_cap, main_wgs = (unsigned int)k0->num_wgs;
  if (lane == 0) atomicAdd(ctl->gate, 1ull << 32);  // one more helper
  const unsigned long long t_born = __builtin_amdgcn_s_memrealtime();
  unsigned long long t_idle = t_born;
  int polls = 0;
  WgClock clk;
  for (;;) {
    int idx = -1;
    if (lane == 0) {
      for (;;) {
        const unsigned int t = min(ld_rlx(ctl->tail), cap), h = ld_rlx(ctl->head);
        if (h >= t) break;
        if (atomicCAS(ctl->head, h, h + 1u) == h) {
          idx = (int)h;
          break;
        }
      }
    }
    idx = __builtin_amdgcn_readfirstlane(idx);
    if (idx < 0) {
      // every main block finished (the sharded counters, one per lane; read
      // every 32nd idle poll)?  Then nothing more can be queued: leave once
      // the queue is empty
      if ((++polls & 31) == 0) {
        unsigned int dn = lane < kTailShards ? ld_rlx(&ctl->done[lane * 32]) : 0u;
        for (int off = 32; off >= 1; off >>= 1) dn += __shfl_xor(dn, off);
        if (__builtin_amdgcn_readfirstlane(dn) >= main_wgs) {
          const unsigned int h = ld_rlx(ctl->head), t = min(ld_rlx(ctl->tail), cap);
          if (__builtin_amdgcn_readfirstlane(h >= t ? 1 : 0)) break;
          continue;
        }
      }
      // (a bound that is never expected to bite: main blocks are at most a
      // 1024-sample block each; a stuck helper must not hang the device)
      if (__builtin_amdgcn_s_memrealtime() - t_idle > 1000000000ull) {  // 10 s at 100 MHz
        if (lane == 0) atomicOr(&ctl->err, 1u);
        break;
      }
      __builtin_amdgcn_s_sleep(96);  // (~2.6 us between polls: idle helpers must not crowd the lines they poll)
      continue;
    }
    // the entry was reserved by a block that writes it at once
    bool ready = true;
    for (const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
         __hip_atomic_load(&k0->tail_ready[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != epoch;) {
      if (__builtin_amdgcn_s_memrealtime() - t0 > 1000000000ull) {  // (never expected: 10 s)
        ready = false;
        break;
      }
      __builtin_amdgcn_s_sleep(1);
    }
    if (!__builtin_amdgcn_readfirstlane(ready ? 1 : 0)) {
      if (lane == 0) atomicOr(&ctl->err, 2u);
      break;
    }
    // the record: written through by its exporter, drained before the flag
    const unsigned long long t_path = __builtin_amdgcn_s_memrealtime();
    const TailPath* q = k0->tail_q + idx;
    const d3 o = mk(ld_wtd(q->o), ld_wtd(q->o + 1), ld_wtd(q->o + 2)), d = mk(ld_wtd(q->d), ld_wtd(q->d + 1), ld_wtd(q->d + 2));
    const d3 T = mk(ld_wtd(q->T), ld_wtd(q->T + 1), ld_wtd(q->T + 2)), L0 = mk(ld_wtd(q->L), ld_wtd(q->L + 1), ld_wtd(q->L + 2));
    const uint64_t rx = ld_wt64(&q->rng), sk = ld_wt64(&q->skey);
    const int depth = (int)ld_wt32(&q->depth), sample = (int)ld_wt32(&q->sample), kind = (int)ld_wt32(&q->kind),
              row = (int)ld_wt32(&q->row), nsub = (int)ld_wt32(&q->nsub), fr = (int)ld_wt32(&q->frame);
    const int64_t oi = (int64_t)ld_wt64(&q->oi);
    int dep_end = depth;
    const d3 L = solo_path<false>(karg, 0, o, d, T, L0, rx, depth, sk, stack, &dep_end);
    const KArg k = launder(karg);
    clk.helper_path(t_path, depth, dep_end);
    const int spp = k->spp_total, bw = (spp + 31) >> 5;
    int last = 0;
    if (lane == 0) {
      atomicAdd(&ctl->solo_ticks, (unsigned int)(__builtin_amdgcn_s_memrealtime() - t_path));
      atomicAdd(&ctl->paths_done, 1u);
      // the sample, written through and drained before the counter
      if (kind == kTailRow) {
        double* r = k->tail_rows + ((size_t)row * spp + sample) * 3;
        st_wtd(r, L.x);
        st_wtd(r + 1, L.y);
        st_wtd(r + 2, L.z);
        atomicOr(k->tail_bits + (size_t)row * bw + (sample >> 5), 1u << (sample & 31));
        wt_drain();
        last = atomicSub(&k->tail_hdr[row].counter, 1) == 1 ? 1 : 0;
      } else {
        double* r = k->split_rad + ((size_t)row * spp + sample) * 3;
        st_wtd(r, L.x);
        st_wtd(r + 1, L.y);
        st_wtd(r + 2, L.z);
        atomicOr(k->split_hits + (size_t)row * bw + (sample >> 5), 1u << (sample & 31));
        wt_drain();
        last = atomicAdd(&k->split_cnt[row], 1) == nsub - 1 ? 1 : 0;
      }
      atomicAdd(ctl->gate, ~0ull);  // one exported path fewer in flight (-1 on the low half)
    }
    last = __builtin_amdgcn_readfirstlane(last);
    if (last) {
      // the pixel's last contributor: its row in sample order, then the pixel
      // (every byte of the row read sc1: written through or by atomics)
      double a;
      int pfr = fr;
      size_t poi = (size_t)oi;
      if (kind == kTailRow) {
        const TailRow* hd = k->tail_hdr + row;
        a = lane < 3 ? ld_wtd(hd->prefix + lane) : 0.0;
        a = row_sum<true>(buf, k->tail_rows + (size_t)row * spp * 3, k->tail_bits + (size_t)row * bw,
                          (int)ld_wt32(&hd->k0), spp, a, lane);
        pfr = (int)ld_wt32(&hd->frame);
        poi = (size_t)ld_wt64(&hd->oi);
      } else {
        uint32_t* hw = k->split_hits + (size_t)row * bw;
        a = row_sum<true>(buf, k->split_rad + (size_t)row * spp * 3, hw, 0, spp, 0.0, lane);
        // the slot's hit bits and counter are left zeroed for the next launch
        for (int i = lane; i < bw; i += 64) hw[i] = 0u;
        if (lane == 0) k->split_cnt[row] = 0;
      }
      const double sx = rld(a, 0), sy = rld(a, 1), sz = rld(a, 2);
      if (lane == 0) store_pixel(k, pfr, poi, sx, sy, sz);
    }
    t_idle = __builtin_amdgcn_s_memrealtime();
  }
  int gone = 0;
  clk.helper_write(k0, lane, t_born);
  if (lane == 0) {
    atomicAdd(&ctl->helper_ticks, (unsigned int)(__builtin_amdgcn_s_memrealtime() - t_born));
    atomicAdd(ctl->gate, ~0ull << 32);  // one helper fewer (-2^32)
    gone = (int)atomicAdd(ctl->helpers_gone, 1u);
  }
  if (__builtin_amdgcn_readfirstlane(gone) + 1 == k0->tail_helpers) {
    // every helper and every main block is done: ready for the next launch
    if (lane < kTailShards) ctl->done[lane * 32] = 0u;
    if (lane == 0) {
      ctl->tail[0] = 0;
      ctl->head[0] = 0;
      ctl->gate[0] = 0;
      ctl->rows_used[0] = 0;
      ctl->helpers_gone[0] = 0;
    }
  }
}

// A block's export of a path, in parts (render_body, pass 0 of a shade
// iteration).  tail_reserve: a helper for it (paths in flight < live helpers:
// the gate word is read first, so draining waves do not add to it in vain)
// and a queue entry; -1: no helper is free.
__device__ __forceinline__ int tail_reserve(KArg k) {
  const int lane = threadIdx.x;
  TailCtl* ctl = k->tail;
  int idx = -1;
  if (lane == 0) {
    const unsigned long long g0 = __hip_atomic_load(ctl->gate, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((uint32_t)g0 < (uint32_t)(g0 >> 32)) {
      const unsigned long long g = atomicAdd(ctl->gate, 1ull);
      if ((uint32_t)g < (uint32_t)(g >> 32)) {
        const unsigned int t = atomicAdd(ctl->tail, 1u);
        if (t < (unsigned int)k->tail_cap) idx = (int)t;  // (entries past the cap are never taken)
      }
      if (idx < 0) atomicAdd(ctl->gate, ~0ull);
    }
  }
  return __builtin_amdgcn_readfirstlane(idx);
}
// ... and the dynamic row of block pixel p, whose sample sl is exported: a
// new one (one row per export at most: rows_used < cap), or the one it has
__device__ __forceinline__ int tail_pixel_row(KArg k, int p, int sl, int64_t oi, int (&prow)[64], short (&pk0)[64]) {
  const int lane = threadIdx.x;
  TailCtl* ctl = k->tail;
  int r = prow[p];
  if (r < 0) {
    if (lane == 0) r = (int)atomicAdd(ctl->rows_used, 1u);
    r = __builtin_amdgcn_readfirstlane(r);
    const int bw = (k->spp_total + 31) >> 5;
    for (int w = lane; w < bw; w += 64) st_wt32(k->tail_bits + (size_t)r * bw + w, 0u);
    if (lane == 0) {
      TailRow* hd = k->tail_hdr + r;
      st_wt32(&hd->counter, 2u);  // the block's own share (given back in its epilogue) + this path
      st_wt32(&hd->k0, (uint32_t)sl);
      st_wt32(&hd->frame, (uint32_t)frame_of(k));
      st_wt64(&hd->oi, (uint64_t)oi);
      prow[p] = r;
      pk0[p] = (short)sl;
    }
  } else if (lane == 0) {
    pk0[p] = (short)min((int)pk0[p], sl);
    atomicAdd(&k->tail_hdr[r].counter, 1);  // one more path owes the row a sample
  }
  return r;
}
// The epilogue of a block with exported paths (render_body, phase 3): the
// block gives back its share of each of its pixels' rows (the running sum of
// the samples before the row's first one), and the row's last contributor
// sums it and writes the pixel
__device__ __forceinline__ void tail_rows_give_back(KArg k, const BlockLoc& blk, int lane3, double (*slot)[3],
                                                    double (*psum)[3], const int* prow, const short* pk0) {
  if (k->tail != nullptr && blk.slot < 0) {
    int last = 0;
    if (prow[lane3] >= 0) {
      TailRow* hd = k->tail_hdr + prow[lane3];
      st_wtd(hd->prefix, psum[lane3][0]);
      st_wtd(hd->prefix + 1, psum[lane3][1]);
      st_wtd(hd->prefix + 2, psum[lane3][2]);
      st_wt32(&hd->k0, (uint32_t)pk0[lane3]);
    }
    wt_drain();  // (the resolve's row samples too) before the counter
    if (prow[lane3] >= 0) last = atomicSub(&k->tail_hdr[prow[lane3]].counter, 1) == 1 ? 1 : 0;
    for (unsigned long long b = __ballot(last); b; b &= b - 1) {
      const int r = prow[__builtin_ctzll(b)], spp = k->spp_total, bw = (spp + 31) >> 5;
      const TailRow* hd = k->tail_hdr + r;
      double a = lane3 < 3 ? ld_wtd(hd->prefix + lane3) : 0.0;
      a = row_sum<true>(slot, k->tail_rows + (size_t)r * spp * 3, k->tail_bits + (size_t)r * bw, (int)ld_wt32(&hd->k0),
                        spp, a, lane3);
      const double sx = rld(a, 0), sy = rld(a, 1), sz = rld(a, 2);
      if (lane3 == 0) store_pixel(k, (int)ld_wt32(&hd->frame), (size_t)ld_wt64(&hd->oi), sx, sy, sz);
    }
  }
}

}  // namespace rtgo
