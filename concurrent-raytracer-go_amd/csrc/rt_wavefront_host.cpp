// rt_wavefront_host.cpp — the host side of the wavefront path.
// BVH scenes render through the staged kernels of rt_wavefront.hip (DESIGN.md
// §4.2).  Buffers live in the context and grow on demand; a frame is cut into
// chunks of whole pixels (all their samples) so the per-sample radiance
// buffer stays below kWfMaxChunkSamples entries (24 B each).
#include <stdlib.h>

#include "rt_context.h"

namespace rtgo {

constexpr int kWfRing = 4;
// (each chunk ends in its own drain of long paths: C5 on one GPU, 2.1 G
// samples, took 7.72 s per frame in chunks of 2^28 samples)
constexpr uint64_t kWfMaxChunkSamples = 1ull << 30;  // 24 GB of radiance (HBM: 288 GB)

// Events for kernel classes [first, last] of one launch sequence: ev[k] opens
// class k (null when not profiling)
static hipEvent_t* prof_block(rt_context* c, int first, int last) {
  if (!c->prof_on) return nullptr;
  const size_t need = kWfProfEvents;
  while (c->prof_pool.size() < c->prof_used + need) {
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess) return nullptr;
    c->prof_pool.push_back(e);
  }
  hipEvent_t* ev = c->prof_pool.data() + c->prof_used;
  c->prof_pending.push_back({c->prof_used, first, last});
  c->prof_used += need;
  return ev;
}

// path slots per shard (a multiple of kWfBlockSlots: every shard receives the
// survivors of the workgroups b % kWfShards == shard, at most shard_cap)
// More slots mean fewer, longer bounce iterations (each persistent traversal
// launch pays a fill and a drain): C4 with 2^20 slots 680 ms per frame, 2^21
// 589, 2^22 536, 2^23 510, 1.5 * 2^23 501, 2^24 499.  No more slots than the
// chunk has samples (a path slot holds one sample's path).
static int wf_shard_cap(int nl, const rt_tuning& tn, uint64_t samples) {
  long long cap = 1 << 24;
  if (tn.wf_paths > 0) cap = std::min(1ll << 24, (long long)tn.wf_paths);
  cap = std::min<long long>(cap, (long long)std::min<uint64_t>(samples, 1ull << 40));
  // soft queues: cap * nl * 16 entries of 16 B, at most 8 GB; keys slot * nl + light fit 32 bits
  cap = std::min<long long>(cap, (1ll << 29) / (16ll * std::max(nl, 1)));
  const long long per = kWfShards * kWfBlockSlots;
  return (int)(std::max(1ll, cap / per) * kWfBlockSlots);
}

// The layout of the context's one wavefront allocation: two path arrays | hit
// records | per-light state | queues, for `cap` path slots, nlk lights (at
// least 1) and qcap hard rays per shard.  Places p's arrays from `base` on
// and returns the bytes they take (base null: only sizes the buffer).
static size_t wf_carve(WfParams* p, char* base, size_t cap, size_t nlk, size_t qcap) {
  size_t used = 0;
  auto take = [&](size_t bytes) {
    void* r = base ? base + used : nullptr;
    used += (bytes + 255) & ~size_t(255);
    return r;
  };
  for (WfPaths* a : {&p->cur, &p->next}) {
    double** dd[12] = {&a->ox, &a->oy, &a->oz, &a->dx, &a->dy, &a->dz,
                       &a->tx, &a->ty, &a->tz, &a->lx, &a->ly, &a->lz};
    for (double** q : dd) *q = (double*)take(cap * sizeof(double));
    a->rng = (uint64_t*)take(cap * sizeof(uint64_t));
    a->sid = (uint32_t*)take(cap * sizeof(uint32_t));
    a->depth = (int32_t*)take(cap * sizeof(int32_t));
  }
  double** hh[3] = {&p->px, &p->py, &p->pz};
  for (double** q : hh) *q = (double*)take(cap * sizeof(double));
  p->hidx = (int32_t*)take(cap * sizeof(int32_t));
  p->lstate = (uint32_t*)take(cap * nlk * sizeof(uint32_t));
  p->hardq = (uint32_t*)take((size_t)kWfShards * qcap * sizeof(uint32_t));
  p->softq = (uint32_t*)take((size_t)kWfShards * qcap * 16 * 4 * sizeof(uint32_t));
  p->coneq = (uint32_t*)take((size_t)kWfShards * qcap * sizeof(uint32_t));
  p->cand = (int32_t*)take(cap * nlk * kWfConeWide * sizeof(int32_t));
  p->wideq = (uint32_t*)take((size_t)kWfShards * qcap * 2 * 4 * sizeof(uint32_t));
  return used;
}

int render_wavefront(rt_context* c, const KParams& kp, const rt_settings* st, hipStream_t s, bool count,
                     const uint32_t* active) {
  const FlatScene& f = c->flat;
  if (c->prof_on) {  // the last frame's kernel times (its events are reused)
    int rc = prof_collect(c);
    if (rc) return rc;
  }
  const int nl = (int)f.lights.size();
  const int local = local_tiles(c, kp.W, kp.H, kp.rank, kp.world);
  const uint64_t local_px = (uint64_t)local * 1024;
  const uint64_t spp = (uint64_t)std::max(st->samples, 1);
  uint64_t max_chunk = kWfMaxChunkSamples;
  if (c->tun.wf_chunk > 0) max_chunk = std::min<uint64_t>((uint64_t)c->tun.wf_chunk, max_chunk);
  const uint64_t chunk_px = std::max<uint64_t>(1, std::min<uint64_t>(local_px, max_chunk / spp));
  const int shard_cap = wf_shard_cap(nl, c->tun, chunk_px * spp);
  const size_t cap = (size_t)shard_cap * kWfShards;
  const size_t nlk = (size_t)std::max(nl, 1);
  // hard rays per shard: at most every light of every path of the workgroups
  // b % kWfShards == shard of wf_shade1 / wf_softgen, which cover at most
  // shard_cap paths (their grid has at most cap / kWfBlockSlots workgroups)
  const size_t qcap = (size_t)shard_cap * nlk;
  WfParams p;
  memset(&p, 0, sizeof p);
  int rc = grow(c, &c->d.wf_mem, wf_carve(&p, nullptr, cap, nlk, qcap), true);
  if (rc) return rc;
  if (!c->d.wf_ctl.p) {
    rc = grow(c, &c->d.wf_ctl, sizeof(WfCtl));
    if (rc) return rc;
    HIP_TRY(hipHostMalloc((void**)&c->wf_host, kWfRing * sizeof(WfCtl), hipHostMallocDefault));
    for (hipEvent_t& e : c->wf_ev) HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  rc = grow(c, &c->d.wf_rad, (size_t)(chunk_px * spp * 3 * sizeof(double)), true);
  if (rc) return rc;
  p.g = Geo{kp.spheres, kp.tris, kp.boxes, kp.bvh, kp.ns, kp.nt, kp.use_bvh, kp.nb};
  p.jump = kp.jump;
  p.list_tries = c->tun.wf_list_tries > 0 ? std::min(64, c->tun.wf_list_tries) : 64;
  p.qbvh = c->d_qbvh;
  memcpy(p.q0, f.q0, sizeof p.q0);
  memcpy(p.qd, f.qd, sizeof p.qd);
  p.mats = kp.mats;
  p.lights = kp.lights;
  p.sky = kp.sky;
  p.nl = nl;
  p.max_depth = kp.max_depth;
  p.recursive = kp.recursive;
  p.soft = kp.soft;
  p.spp = st->samples;  // (0: the mean is 0/0 = NaN, as DivScalar(0) in Go)
  // a progression's add: samples [sample_base, sample_base +
  // spp) of spp_total, the resolve continuing the sums; else 0, spp, none
  p.sample_base = kp.sample_base;
  p.spp_total = kp.spp_total;
  p.acc = (kp.acc_mode & 4) ? kp.acc : nullptr;
  p.W = kp.W;
  p.H = kp.H;
  p.rank = kp.rank;
  p.world = kp.world;
  p.tiles_x = kp.tiles_x;
  p.ntiles = kp.ntiles;
  p.layout = kp.layout;
  p.tile_list = dev_tiles(c, kp.W, kp.H, kp.rank, kp.world);
  // a lane holds at most one pending child per internal node above its leaf:
  // depth - 1 entries (leaves at level bvh_depth, the root at level 1)
  p.stack_depth = std::max(1, f.bvh_depth - 1);
  // traversal workgroups: trav_block threads (64..1024), LDS shared by
  // trav_wgs of them per CU (tuning; default one of 1024)
  const rt_tuning& tn = c->tun;
  p.trav_block = kWfTravBlock;
  int trav_wgs = 1;
  if (tn.wf_trav_block > 0) p.trav_block = std::max(1, std::min(16, tn.wf_trav_block / 64)) * 64;
  if (tn.wf_trav_wgs > 0) trav_wgs = std::min(32, tn.wf_trav_wgs);
  p.bvh_nodes = (int)f.qbvh.size();
  p.lds_nodes = wf_lds_nodes(p.stack_depth, (int)f.qbvh.size(), p.trav_block, trav_wgs);
  if (tn.wf_lds_nodes >= 0)  // stage fewer nodes (an odd count: child pairs never split)
    p.lds_nodes = std::min(p.lds_nodes, tn.wf_lds_nodes | 1);
  // the occlusion kernels' 4-wide tree, where it fits the LDS whole beside
  // its stacks (C4: 4,801 slots and 20 stack entries, 157 KB at 1024
  // threads).  RTGO_BVH4=0 (measurement switch) keeps the binary walk.
  p.qbvh4 = c->d_qbvh4;
  p.nodes4 = (int)f.qbvh4.size();
  p.stack4 = std::max(1, f.bvh4_stack);
  p.root4 = f.bvh4_root;
  {
    const char* e4 = getenv("RTGO_BVH4");
    p.use4 = !(e4 && atoi(e4) == 0) && p.nodes4 > 0 && tn.wf_lds_nodes < 0 &&
             wf_lds_nodes(p.stack4, p.nodes4, p.trav_block, trav_wgs) >= p.nodes4;
  }
  p.shard_cap = shard_cap;
  p.hard_cap = (int64_t)qcap;
  p.soft_cap = (int64_t)qcap * 16;
  p.wide_cap = (int64_t)qcap * 2;
  p.cf = kp.cf;
  p.seed_key = kp.seed_key;
  p.ctl = c->d.wf_ctl.as<WfCtl>();
  p.counts = kp.counts;
  p.out_linear = kp.out_linear;
  p.out_rgba = kp.out_rgba;
  p.rad = c->d.wf_rad.as<double>();
  if (wf_carve(&p, c->d.wf_mem.as<char>(), cap, nlk, qcap) > c->d.wf_mem.cap) {
    set_error("wavefront buffer layout overflow");
    return RT_E_NOMEM;
  }
  for (uint64_t lp0 = 0; lp0 < local_px; lp0 += chunk_px) {
    const uint64_t npx = std::min(chunk_px, local_px - lp0);
    p.lp0 = (uint32_t)lp0;
    const uint64_t total = npx * (uint64_t)st->samples;
    HIP_TRY(hipMemsetAsync(p.rad, 0, (size_t)(npx * spp * 3 * sizeof(double)), s));
    if (total > 0) {
      WfCtl init;
      memset(&init, 0, sizeof init);
      init.total = total;
      HIP_TRY(hipMemcpyAsync(p.ctl, &init, sizeof init, hipMemcpyHostToDevice, s));
      // the first samples, then bounces until every sample has finished; the
      // host reads the loop state one bounce behind the GPU
      p.live_bound = (int32_t)cap;
      p.dry = 0;
      // (active: an adaptive add -- stopped pixels' samples become dead slots)
      int e = wf_launch_bounce(p, true, count, s, prof_block(c, kWfRegen, kWfRegen), active);
      if (e) return launch_failed("wavefront", e);
      std::swap(p.cur, p.next);
      const long long max_iter = (long long)total + std::max(kp.max_depth, 0) + 8;
      for (long long it = 0;; ++it) {
        if (it > max_iter) {
          set_error("wavefront loop did not terminate");
          return RT_E_DEVICE;
        }
        e = wf_launch_bounce(p, false, count, s, prof_block(c, kWfExtend, kWfRegen), active);
        if (e) return launch_failed("wavefront", e);
        std::swap(p.cur, p.next);
        const int r = (int)(it % kWfRing);
        HIP_TRY(hipMemcpyAsync(c->wf_host + r, p.ctl, sizeof(WfCtl), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipEventRecord(c->wf_ev[r], s));
        if (it >= 1) {
          const int pr = (int)((it - 1) % kWfRing);
          const int rw = wait_event(c, c->wf_ev[pr]);  // (bounded under a renderer's deadline)
          if (rw) return rw;
          const WfCtl& h = c->wf_host[pr];
          if (h.live == 0 && h.dry) break;  // bounce `it` had nothing to do
          // once dry, live counts only fall: bounce it + 1 has at most h.live paths
          if (h.dry) {
            p.live_bound = h.live;
            p.dry = 1;
          }
        }
      }
    }
    hipEvent_t* rev = prof_block(c, kWfResolve, kWfResolve);
    if (rev) HIP_TRY(hipEventRecord(rev[kWfResolve], s));
    int e = wf_launch_resolve(p, (int)npx, s);
    if (e) return launch_failed("wavefront resolve", e);
    if (rev) HIP_TRY(hipEventRecord(rev[kWfResolve + 1], s));
  }
  return RT_OK;
}

}  // namespace rtgo
