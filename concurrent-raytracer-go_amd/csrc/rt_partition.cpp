// rt_partition.cpp — the balanced partition planner rt_partition_balanced
// (include/rt_api.h).  rt_context_set_partition is in rt_api.cpp, beside the
// context's other owners of its shared_ptr.
#include "rt_context.h"

using namespace rtgo;

// Balanced partition (include/rt_api.h): a one-sample pilot of the whole
// frame (the schedule's pilot, prepare_schedule, over all tiles as one rank),
// each tile's estimated work (spp x the sum of its pixels' estimates,
// sched_tile_work), then longest-processing-time-first: tiles by decreasing
// work (ties: lower tile first) to the least loaded rank (ties: lower rank).
// The measured work of every tile of the frame (r04): the frame rendered
// once at its full sample count through the context's own (one-rank)
// schedule, with the measuring instantiation recording every sample's path
// length; a tile weighs the sum of its pixels' mean path lengths x spp.  The
// one-sample pilot's estimate (the neighbourhood's longest path, which the
// block cutting wants) misjudges whole tiles: with it the slowest of 8 ranks
// of the headline frame took 1.22x the mean share.  Path lengths are
// integers of an exact render, so every rank that measures the same frame on
// its own device derives the same partition.  (r05) measure_spp < spp: the
// measuring render takes only the frame's first measure_spp samples of every
// pixel; a tile weighs its pixels' mean path length over them x spp.  The
// renderer (rt_renderer_render) plans its partition that way with 16
// samples, because its first Render -- and every one-shot rt_render with
// num_devices > 1 -- pays this render before its own frame (at
// the full 100 samples it cost a whole one-GPU frame); the public
// rt_partition_balanced, which a caller plans once for many frames, measures
// every sample (8 ranks of the headline frame, rank shares alone on one GPU:
// predicted 874 k Mrays/s with all 100 samples, 853 k with 16, 815 k with the
// one-sample pilot; profiles/r04_rank_share_probe.json, r05_rank_share_probe.json).
static int measured_tile_work(rt_context* c, int w, int h, const rt_settings* st, int measure_spp,
                              std::vector<float>* work) {
  hipStream_t s = c->stream;
  rt_settings sm = *st;
  sm.samples = std::min(st->samples, measure_spp);
  KParams p;
  base_params(c, w, h, &sm, 0, 1, RT_LAYOUT_PACKED_TILES, &p);
  p.spp = sm.samples;
  p.spp_total = sm.samples;
  p.sample_base = 0;
  p.acc_mode = 0;
  p.acc = nullptr;
  p.counts = nullptr;
  int rc = prepare_schedule(c, &p, &sm, s);
  if (rc) return rc;
  p.num_wgs = p.num_blocks;
  const int ntiles = rt_num_tiles(w, h);
  const size_t npx = (size_t)ntiles * 1024;
  std::vector<int32_t> tiles;
  strided_tiles(w, h, 0, 1, &tiles);
  auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
  const size_t o_meas = al(npx * 16);  // [linear | rgba] image, packed tiles
  const size_t o_sched = o_meas + al(npx * 8);
  const size_t o_tw = o_sched + al(sched_scratch_bytes(ntiles));
  const size_t total = o_tw + al((size_t)ntiles * sizeof(float));
  char* buf = nullptr;
  HIP_TRY((hipError_t)dev_alloc((void**)&buf, total));
  auto done = [&](int code) {
    (void)hipStreamSynchronize(s);
    dev_free(buf);
    return code;
  };
  p.out_linear = (float*)buf;
  p.out_rgba = (uint8_t*)(buf + npx * 12);
  unsigned int* meas = (unsigned int*)(buf + o_meas);
  p.work_max = meas;
  p.work_sum = meas + npx;
  if (hipMemsetAsync(meas, 0, npx * 8, s) != hipSuccess) return done(RT_E_DEVICE);
  if (p.num_blocks > 0) {
    const int e = launch_render(p, false, s);
    if (e != hipSuccess) return done(launch_failed("partition measuring", e));
  }
  SchedParams sp = sched_params(c, p, st, tiles, nullptr, false, false, default_block_work(c),
                                big_block_pixels(st->samples, c->tun), buf + o_sched, nullptr, nullptr);
  sp.work_max = meas;
  sp.work_sum = meas + npx;
  sp.work_n = sm.samples;
  sp.work_mean = 1;          // (the measured samples' mean, times the frame's spp)
  sp.split_depth = 1 << 30;  // (weights only: no pixel is marked heavy)
  float* d_tw = (float*)(buf + o_tw);
  int e = sched_launch_tile_work(sp, d_tw, s);
  if (e == hipSuccess) e = hipMemcpyAsync(work->data(), d_tw, (size_t)ntiles * sizeof(float), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    set_error(std::string("partition measurement failed: ") + hipGetErrorString((hipError_t)e));
    return done(RT_E_DEVICE);
  }
  return done(RT_OK);
}

int rtgo::partition_balanced(rt_context* c, int32_t w, int32_t h, const rt_settings* st, int32_t world,
                             int measure_spp, rt_partition** out) {
  if (!c || !c->have_scene || !out) {
    set_error("rt_partition_balanced: context without a scene, or out is NULL");
    return RT_E_INVALID;
  }
  *out = nullptr;
  int rc = check_frame(c, w, h, st);
  if (rc) return rc;
  if (world < 1 || world > 65536) {
    set_error("rt_partition_balanced: world must be in [1, 65536]");
    return RT_E_INVALID;
  }
  HIP_TRY(hipSetDevice(c->device));
  const FlatScene& f = c->flat;
  const rt_tuning& tn = c->tun;
  hipStream_t s = c->stream;
  const int ntiles = rt_num_tiles(w, h);
  std::vector<float> work(ntiles, 0.0f);
  // the tiles' work to a partition of them over `world` ranks
  auto plan = [&]() {
    PartitionData d;
    d.w = w;
    d.h = h;
    d.world = world;
    lpt_partition(work, &d);
    finish_partition(&d);
    *out = make_partition(std::move(d));
    return (int)RT_OK;
  };
  if (tn.pilot != 0 && !use_wavefront(c) && st->sky == RT_SKY_NONE && st->samples > 0 &&
      st->samples <= kMaxBlockSamples && st->max_depth > 0) {
    rc = measured_tile_work(c, w, h, st, std::max(1, measure_spp), &work);
    return rc ? rc : plan();
  }
  std::vector<int32_t> tiles;
  strided_tiles(w, h, 0, 1, &tiles);
  KParams p;
  base_params(c, w, h, st, 0, 1, RT_LAYOUT_PACKED_TILES, &p);
  const bool masks = masks_apply(f);
  const bool frustum = tn.frustum != 0 && st->sky == RT_SKY_NONE;
  std::vector<unsigned long long> mh;
  if (masks) tile_primary_masks(f, p.cf, w, h, tiles, &mh);
  std::vector<float> cost;
  tile_cost(f, p.cf, w, h, tiles, &cost);
  auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
  const size_t npx = (size_t)ntiles * 1024;
  const size_t o_in = al(sched_scratch_bytes(ntiles));
  const size_t o_cost = o_in + al(mh.size() * sizeof(unsigned long long));
  const size_t o_pilot = o_cost + al(cost.size() * sizeof(float));
  const size_t o_tw = o_pilot + al(npx * 24);
  const size_t total = o_tw + al((size_t)ntiles * sizeof(float));
  char* buf = nullptr;
  HIP_TRY((hipError_t)dev_alloc((void**)&buf, total));
  auto fail = [&](int code) {
    (void)hipStreamSynchronize(s);
    dev_free(buf);
    return code;
  };
  {
    unsigned long long* d_masks = masks ? (unsigned long long*)(buf + o_in) : nullptr;
    float* d_cost = (float*)(buf + o_cost);
    float* d_tw = (float*)(buf + o_tw);
    if (!mh.empty() &&
        hipMemcpyAsync(d_masks, mh.data(), mh.size() * sizeof(unsigned long long), hipMemcpyHostToDevice, s))
      return fail(RT_E_DEVICE);
    if (!cost.empty() && hipMemcpyAsync(d_cost, cost.data(), cost.size() * sizeof(float), hipMemcpyHostToDevice, s))
      return fail(RT_E_DEVICE);
    SchedParams sp = sched_params(c, p, st, tiles, nullptr, masks, frustum, default_block_work(c),
                                  big_block_pixels(st->samples, tn), buf, d_masks, d_cost);
    int e = sched_launch_pixels(sp, s);
    if (e != hipSuccess) return fail(launch_failed("partition pilot", e));
    if (tn.pilot != 0 && st->samples > 0 && st->max_depth > 0) {
      rc = run_pilot(c, p, &sp, buf + o_pilot, s);
      if (rc) return fail(rc);
    }
    e = sched_launch_tile_work(sp, d_tw, s);
    if (e != hipSuccess) return fail(launch_failed("partition estimate", e));
    if (hipMemcpyAsync(work.data(), d_tw, (size_t)ntiles * sizeof(float), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
      set_error("partition estimate read-back failed");
      return fail(RT_E_DEVICE);
    }
  }
  (void)fail(RT_OK);
  return plan();
}

extern "C" {

int rt_partition_balanced(rt_context* c, int32_t w, int32_t h, const rt_settings* st, int32_t world,
                          rt_partition** out) {
  return partition_balanced(c, w, h, st, world, st ? st->samples : 0, out);
}

}  // extern "C"
