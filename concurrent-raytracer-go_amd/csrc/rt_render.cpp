// rt_render.cpp — a frame's launch sequence: the work schedule, the tail
// helpers, the streamed launch, the sample passes, and the single-frame,
// batched and camera-sequence render entry points (include/rt_api.h).
#include <math.h>

#include "rt_context.h"

namespace rtgo {

// Pixels per work block.  Tiles without geometry: up to
// kMaxBlockSamples sample ids (the block's hit list lives in LDS), at most
// 64 pixels; tiles with work get smaller blocks (prepare_schedule).
int big_block_pixels(int spp, const rt_tuning& tn) {
  int cap = kMaxBlockSamples;
  if (tn.block_samples > 0) cap = std::min(cap, tn.block_samples);
  if (spp <= 0) return 64;
  return std::max(1, std::min(64, cap / spp));
}

// Per (scene, frame, rank, settings) schedule, cached in the context: the
// tiles' primary-ray candidate masks (host: tiles x primitives) and the work
// blocks, built on the GPU by rt_schedule.hip from a ONE-SAMPLE PILOT render
// of this rank's pixels (same kernel, kPilot instantiation) that reports
// each pixel's path length: pixels whose paths bounce a lot go into small
// blocks (or are split into sample ranges) dispatched first, empty sky into
// large blocks.  The pilot traces hard shadows only: the soft rays do not
// change how long a path is, only what a bounce costs, and tracing them
// would make the pilot's own tail (one 50-bounce path) several times longer.
// One 12-byte device->host copy (block and split counts) sizes the launch.
// This only partitions and orders the work; every block is rendered by the
// same code, so the image does not depend on it (tests/test_gpu_schedules.py).
static size_t split_flags_bytes(int nsplit, int spp) {
  return (size_t)nsplit * ((spp + 31) / 32) * sizeof(uint32_t) + (size_t)nsplit * sizeof(int32_t);
}

// Tail helpers for a megakernel launch of p: render_kernel_tail
// (the staged product body) on a linear-scan scene with shadow-cone masks (what
// solo_path needs), one sample pass, no sky, not measuring.  Lays out the
// context's queue and rows for p.spp_total samples per pixel (the control
// block and ready flags zeroed once per layout: each launch's last helper
// leaves the control block zeroed, and a ready flag holds its launch's epoch)
// and sets p's tail fields; leaves them null (off) otherwise.
static int setup_tail(rt_context* c, KParams* p, hipStream_t s) {
  const rt_tuning& tn = c->tun;
  p->tail = nullptr;
  const bool masks = !p->use_bvh && p->ns <= 64 && p->nt <= 64;
  if (tn.tail_helpers < 0 || p->stage_bytes <= 0 || !masks || p->sky || p->work_max || p->counts || p->acc_mode != 0 ||
      p->spp_total < 1 || p->spp_total > kMaxBlockSamples || p->max_depth < 2 || !p->recursive)
    return RT_OK;
  const int spp = p->spp_total, bw = (spp + 31) / 32;
  const size_t per = (size_t)spp * 24 + (size_t)bw * 4 + sizeof(TailPath) + sizeof(TailRow) + 4;
  // one queue entry and at most one row per exported path; 64 MB at most
  const int cap = (int)std::max<size_t>(1024, std::min<size_t>(16384, (size_t(64) << 20) / per));
  auto al = [](size_t b) { return (b + 255) & ~size_t(255); };
  const size_t o_q = al(sizeof(TailCtl)), o_ready = o_q + al((size_t)cap * sizeof(TailPath));
  const size_t o_rows = o_ready + al((size_t)cap * 4), o_bits = o_rows + al((size_t)cap * spp * 24);
  const size_t o_hdr = o_bits + al((size_t)cap * bw * 4), total = o_hdr + al((size_t)cap * sizeof(TailRow));
  if (c->tail_spp != spp || c->tail_cap != cap) {
    int rc = grow(c, &c->d.tail, total);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(c->d.tail.p, 0, o_rows, s));  // control block, queue, ready flags
    c->tail_spp = spp;
    c->tail_cap = cap;
    c->tail_epoch = 0;
  }
  if (++c->tail_epoch == 0) c->tail_epoch = 1;
  char* b = c->d.tail.as<char>();
  p->tail = (TailCtl*)b;
  p->tail_q = (TailPath*)(b + o_q);
  p->tail_ready = (unsigned int*)(b + o_ready);
  p->tail_rows = (double*)(b + o_rows);
  p->tail_bits = (uint32_t*)(b + o_bits);
  p->tail_hdr = (TailRow*)(b + o_hdr);
  p->tail_cap = cap;
  p->tail_helpers = tn.tail_helpers > 0 ? tn.tail_helpers : 64;
  p->tail_kmax = tn.tail_paths > 0 ? tn.tail_paths : 4;
  p->tail_dmin = tn.tail_depth > 0 ? tn.tail_depth : 2;
  int every = tn.tail_every > 0 ? tn.tail_every : 4, pow2 = 1;
  while (pow2 < every && pow2 < 64) pow2 <<= 1;
  p->tail_every_mask = pow2 - 1;
  const int at = tn.tail_at > 0 ? std::min(tn.tail_at, 100) : 100;
  p->tail_pos = (int32_t)((int64_t)p->num_wgs * at / 100);
  p->tail_epoch = c->tail_epoch;
  return RT_OK;
}

// The scheduler's inputs for `tiles` (host masks and costs uploaded into
// `in`, the scratch layout at `scratch`), as SchedParams.
SchedParams sched_params(rt_context* c, const KParams& p, const rt_settings* st, const std::vector<int32_t>& tiles,
                         const int32_t* d_tiles, bool masks, bool frustum, double block_work, int bigP, void* scratch,
                         unsigned long long* d_masks, float* d_cost) {
  const rt_tuning& tn = c->tun;
  SchedParams sp;
  memset(&sp, 0, sizeof sp);
  sched_layout(scratch, (int)tiles.size(), &sp);
  sp.spheres = c->d_spheres;
  sp.tris = c->d_tris;
  sp.cf = p.cf;
  sp.W = p.W;
  sp.H = p.H;
  sp.rank = p.rank;
  sp.world = p.world;
  sp.tiles_x = (p.W + 31) / 32;
  sp.ntiles = rt_num_tiles(p.W, p.H);
  sp.local = (int)tiles.size();
  sp.spp = st->samples;
  sp.big_pixels = bigP;
  sp.frustum = frustum;
  sp.split_samples = tn.split_samples > 0 ? std::min(64, tn.split_samples) : 64;
  sp.split_depth = tn.split_depth > 0 ? tn.split_depth : 16;
  sp.block_work = block_work;
  sp.tile_masks = masks ? d_masks : nullptr;
  sp.tile_cost = d_cost;
  sp.tile_list = d_tiles;
  return sp;
}

// The one-sample pilot render of sp's tiles (blocks of 64 pixels, packed
// output into `buf`, npx * 24 bytes): each pixel's longest path and its
// bounces into sp.work_max / work_sum.
int run_pilot(const rt_context* c, const KParams& p, SchedParams* sp, char* buf, hipStream_t s) {
  const size_t npx = (size_t)sp->local * 1024;
  float* plin = (float*)buf;
  uint8_t* prgba = (uint8_t*)buf + npx * 12;
  unsigned int* plen = (unsigned int*)((uint8_t*)buf + npx * 16);
  KParams q = p;
  q.spp = 1;
  q.blocks = sp->pilot_blocks;
  q.num_blocks = sp->local * 16;
  q.num_wgs = q.num_blocks;
  q.layout = RT_LAYOUT_PACKED_TILES;
  q.out_linear = plin;
  q.out_rgba = prgba;
  q.counts = nullptr;
  q.dbg = nullptr;
  q.work_max = plen;
  q.work_sum = plen + npx;
  q.soft = 0;  // path lengths only (see above)
  if (c->tun.pilot_depth > 0) q.max_depth = std::min(q.max_depth, c->tun.pilot_depth);
  q.tile_masks = sp->tile_masks;
  q.split_rad = nullptr;
  q.split_hits = nullptr;
  q.split_cnt = nullptr;
  q.acc = nullptr;
  q.acc_mode = 0;
  q.sample_base = 0;
  q.spp_total = 1;
  HIP_TRY(hipMemsetAsync(plen, 0, 2 * npx * sizeof(unsigned int), s));
  const int e = launch_render(q, false, s);
  if (e != hipSuccess) return launch_failed("pilot", e);
  sp->work_max = plen;
  sp->work_sum = plen + npx;
  sp->work_n = 1;
  return RT_OK;
}

// path bounces per block: 8 full-wave bounce steps; 16x that with a BVH,
// whose bounces are long divergent traversals that need full waves more
// than short blocks (C4: 2.10 s at 512, 1.77 s at 8192)
// (triangle scenes: 256 -- a bounce there tests 12 triangles per cube, so
// fewer bounces make a block: silver C3 0.56 -> 0.46 ms; sphere scenes:
// 384 since solo paths (r02, headline 0.785 -> 0.745 ms; 320: 0.755,
// 448: 0.79, 512 was the r01 optimum)
// Blocks' estimated work (bounce-samples).  A launch of ONE frame ends when
// its slowest block does, so its blocks are small: a long path shares its
// wave with few others (the latency schedule).  A launch of several frames
// (rt_context_render_frames_async) is rendered for throughput: its tail is
// paid once for all of them and overlaps the next launch, and larger blocks
// cost less per sample (fewer visibility passes, splits and block starts).
// Measured (bench.py --tuning block_work=..., 2 launches of 8 frames in
// flight, one MI355X): C2 384 -> 128.7 k, 512 135.5 k, 768 141.3 k, 1024
// 144.8 k, 1536 143.0 k, 2048 139.9 k Mrays/s; C3 256 -> 393.9 k, 512
// 419.8 k, 768 461.8 k, 1024 474.9 k, 2048 480.1 k (16 frames per launch:
// C2 896 144.4 k, 1024 146.2 k, 1280 145.4 k; C3 1024 463.7 k, 1536 476.1 k,
// 2048 479.1 k).  (r05, RNG spec v4: a bounce-sample costs less, so blocks
// grow: the driver's 20 frames as 2 launches of 10, C2 1024 -> 212.5 k, 1536
// 223.7 k, 2048 215.0 k, 3072 212.6 k, 4096 208.6 k; 100 frames as 4 of 25:
// 247.8 k, 251.6 k, 251.0 k, 249.6 k, 248.3 k; scripts/k20_tuning.sh)
// (r06, one frame per launch, sphere scenes, scripts/tail_probe.py, median
// of 40 frames: 384 and 512 bounce-samples per block equal when the order of
// the settings is balanced, 0.571-0.583 vs 0.574-0.586 ms -- a first sweep
// that always ran 384 first had put 512 2 % ahead; 768 0.725, 256 0.60-0.62)
double default_block_work(const rt_context* c, int frames) {
  const FlatScene& f = c->flat;
  double block_work = !f.bvh.empty() ? 8192.0
                      : frames > 1    ? (f.tris.empty() ? 1536.0 : 2048.0)
                                      : (f.tris.empty() ? 384.0 : 256.0);
  if (c->tun.block_work > 0) block_work = std::max(1.0, c->tun.block_work);
  return block_work;
}

bool masks_apply(const FlatScene& f) { return f.bvh.empty() && f.spheres.size() <= 64 && f.tris.size() <= 64; }

// Could a render of these settings be streamed?  A staged
// linear-scan scene, no sky, one sample pass (or a progression's add of one
// launch), tail helpers off, no measured schedule; `frames`: the frames per
// launch of the schedule's key.
static bool stream_wanted(const rt_context* c, const KParams& p, const rt_settings* st, int frames) {
  const rt_tuning& tn = c->tun;
  // auto: launches of several frames of sphere-only scenes, where the A/B shows a
  // gain (headline +22 %); with triangles it loses (C3 0.65x: the stream
  // kernel's camera rays scan every primitive, the block kernel's visibility
  // pass only the block's frustum candidates)
  if (tn.stream == 0 || (tn.stream < 0 && (frames < 2 || !c->flat.tris.empty()))) return false;
  return tn.stage && c->stage_bytes > 0 && c->flat.bvh.empty() && st->sky == RT_SKY_NONE && st->samples >= 1 &&
         st->samples <= kMaxBlockSamples && (p.spp_total == st->samples || p.acc_mode == kAccProgressive) &&
         tn.tail_helpers < 0 && !tn.measure;
}

// active (an adaptive progression's add): the per-pixel active
// flags folded into the pixels' primary masks, the schedule keyed by the
// active set's generation `active_gen`; null: an ordinary schedule.
// cam: a render whose camera is not the scene's is keyed by
// cam.gen; a sequence (cam.n frames, their table in d.cams) gets the union of
// its cameras' pixel masks, so its live-pixel list holds every pixel that any
// frame's rays may hit.
int prepare_schedule(rt_context* c, KParams* p, const rt_settings* st, hipStream_t s, int frames,
                     const uint32_t* active, int64_t active_gen, const CamKey& cam) {
  const FlatScene& f = c->flat;
  const int w = p->W, h = p->H, rank = p->rank, world = p->world;
  const rt_tuning& tn = c->tun;
  // the live-pixel list of the streamed launches is built (and cached) with the blocks
  const bool want_live = stream_wanted(c, *p, st, frames);
  int bigP = big_block_pixels(st->samples, tn);
  const double block_work = default_block_work(c, frames);
  const bool pilot = tn.pilot != 0;
  // a sky makes every camera sample count (a miss returns the sky, not +0):
  // no primary-ray culling, no black tiles
  const bool sky = st->sky != RT_SKY_NONE;
  const bool frustum = tn.frustum != 0 && !sky;
  const bool part = use_partition(c, w, h, world);
  const int64_t key[16] = {(int64_t)c->scene_gen, w, h, rank, world, st->samples, st->max_depth,
                           st->recursive_reflections, st->soft_shadows, bigP, (int64_t)(block_work * 16),
                           (pilot ? 1 + tn.pilot_depth : 0) | (int64_t)tn.split_samples << 16,
                           (frustum ? 1 : 0) | (sky ? 2 : 0) | (tn.measure ? 4 : 0) | (want_live ? 8 : 0) | (st->camera ? 16 : 0) |
                               (int64_t)tn.split_depth << 8,
                           part ? (int64_t)c->part->id : 0,
                           active ? active_gen + 1 : 0,
                           cam.gen};
  // the pixels' primary masks: the scene's candidate masks where they apply; an
  // adaptive add without them (or without primary culling) gets masks of its
  // own that hold every primitive and only carry the active flags
  const bool prim_masks = masks_apply(f);
  const bool own_masks = active && !(prim_masks && frustum);
  const bool masks = prim_masks || own_masks;
  const bool new_key = memcmp(key, c->order_key, sizeof key) != 0;
  // a measured re-cut: the previous frame of this key measured every pixel
  const bool remeasured = !new_key && c->meas_state == 2;
  if (new_key || remeasured) {
    int rc = quiesce(c);  // the last render may still read the blocks, masks and split rows
    if (rc) return rc;
    std::vector<int32_t> tiles;
    host_tiles(c, w, h, rank, world, &tiles);
    const int local = (int)tiles.size();
    c->num_blocks = 0;
    c->nsplit = 0;
    c->split_frames = 0;  // (the split rows are laid out again below)
    c->nlive = -1;
    c->live_local = local;
    c->masks_host.clear();
    c->d_masks = nullptr;
    if (local > 0) {
      // per-tile inputs (host): primary-ray candidate masks, projected-primitive counts
      if (own_masks) {
        auto bits = [](size_t n) { return n >= 64 ? ~0ull : (1ull << n) - 1ull; };
        const unsigned long long ms = prim_masks ? bits(f.spheres.size()) : ~0ull;
        const unsigned long long mt = prim_masks ? bits(f.tris.size()) : ~0ull;
        c->masks_host.resize((size_t)local * 2);
        for (int lt = 0; lt < local; ++lt) {
          c->masks_host[2 * lt] = ms;
          c->masks_host[2 * lt + 1] = mt;
        }
      } else if (masks && cam.n > 0) {
        // a sequence: [the OR of the cameras' tile masks][camera 0's][camera 1's] ...
        c->masks_host.assign((size_t)local * 2 * (size_t)(cam.n + 1), 0ull);
        std::vector<unsigned long long> one;
        for (int k = 0; k < cam.n; ++k) {
          tile_primary_masks(f, cam.frames[k], w, h, tiles, &one);
          for (size_t i = 0; i < (size_t)local * 2; ++i) {
            c->masks_host[i] |= one[i];
            c->masks_host[(size_t)local * 2 * (size_t)(k + 1) + i] = one[i];
          }
        }
      } else if (masks) {
        tile_primary_masks(f, p->cf, w, h, tiles, &c->masks_host);
      }
      std::vector<float> cost;
      tile_cost(f, p->cf, w, h, tiles, &cost);
      const size_t scratch = sched_scratch_bytes(local);
      const size_t mbytes = c->masks_host.size() * sizeof(unsigned long long), cbytes = cost.size() * sizeof(float);
      const size_t inputs = mbytes + cbytes;
      rc = grow(c, &c->d.sched, scratch + inputs + 256);
      if (rc) return rc;
      rc = grow_pinned(&c->h_small, 256 + inputs);  // (its last use was synchronized below)
      if (rc) return rc;
      char* const small = c->h_small.as<char>();
      char* in = c->d.sched.as<char>() + ((scratch + 255) & ~size_t(255));
      c->d_masks = masks ? (unsigned long long*)in : nullptr;
      float* d_cost = (float*)(in + mbytes);
      // (through pinned staging: a pageable copy sets up the runtime's own
      // staging on first use, milliseconds of a fresh process's first frame)
      memcpy(small + 256, c->masks_host.data(), mbytes);
      memcpy(small + 256 + mbytes, cost.data(), cbytes);
      // From the first copy on, h_small may be read by a DMA still in flight:
      // every return before the synchronize below waits for the stream first
      // (the next schedule writes h_small again; host_free hands it to the
      // process-wide cache).
      auto fail_synced = [&](int code) {
        (void)hipStreamSynchronize(s);
        return code;
      };
      auto hip_ok = [&](hipError_t err, const char* what) {
        if (err == hipSuccess) return true;
        set_error(std::string(what) + " failed: " + hipGetErrorString(err));
        return false;
      };
      // a scheduler launch (its hipError_t as int): RT_OK, or the error set
      auto launched = [](int err) { return err == hipSuccess ? (int)RT_OK : launch_failed("schedule", err); };
      if (mbytes && !hip_ok(hipMemcpyAsync(c->d_masks, small + 256, mbytes, hipMemcpyHostToDevice, s),
                            "schedule mask upload"))
        return fail_synced(RT_E_DEVICE);
      if (cbytes && !hip_ok(hipMemcpyAsync(d_cost, small + 256 + mbytes, cbytes, hipMemcpyHostToDevice, s),
                            "schedule cost upload"))
        return fail_synced(RT_E_DEVICE);
      SchedParams sp = sched_params(c, *p, st, tiles, dev_tiles(c, w, h, rank, world), masks, frustum, block_work,
                                    bigP, c->d.sched.p, c->d_masks, d_cost);
      sp.active = active;
      sp.own_masks = own_masks ? 1 : 0;
      rc = launched(cam.n > 0 ? sched_launch_pixels_seq(sp, c->d.cams.as<const CamFrame>(), cam.n,
                                                        masks ? c->d_masks + (size_t)local * 2 : nullptr, s)
                              : sched_launch_pixels(sp, s));
      if (rc) return fail_synced(rc);
      if (remeasured) {  // every sample's path of the last frame (the measuring render)
        sp.work_max = c->d.meas.as<const unsigned int>();
        sp.work_sum = sp.work_max + (size_t)local * 1024;
        sp.work_n = st->samples;
      } else if (pilot && st->samples > 0 && st->max_depth > 0) {
        rc = grow(c, &c->d.pilot, (size_t)local * 1024 * 24 + 256);
        if (rc) return fail_synced(rc);
        rc = run_pilot(c, *p, &sp, c->d.pilot.as<char>(), s);
        if (rc) return fail_synced(rc);
      }
      rc = launched(sched_launch_blocks(sp, false, s));
      // live pixels per weight class and their number (totals[3])
      if (!rc && want_live) rc = launched(sched_launch_live(sp, false, s));
      if (rc) return fail_synced(rc);
      if (!hip_ok(hipMemcpyAsync(small, sp.totals, 4 * sizeof(int32_t), hipMemcpyDeviceToHost, s),
                  "schedule count read-back"))
        return fail_synced(RT_E_DEVICE);
      rc = wait_stream(c, s);  // (bounded under a renderer's deadline)
      if (rc) return rc;
      memcpy(c->h_totals, small, 4 * sizeof(int32_t));
      const int nblocks = c->h_totals[0], nsplit = c->h_totals[1];
      rc = grow(c, &c->d.blocks, (size_t)std::max(nblocks, 1) * kBlockInts * sizeof(int32_t));
      if (rc) return rc;
      sp.blocks = c->d.blocks.as<int32_t>();
      rc = launched(sched_launch_blocks(sp, true, s));
      if (rc) return rc;
      c->num_blocks = nblocks;
      c->nsplit = nsplit;
      if (want_live) {  // the list itself: nlive items, then every local pixel's position in it
        const int nlive = std::max(0, std::min(c->h_totals[3], local * 1024));
        rc = grow(c, &c->d.live, (size_t)std::max(nlive, 1) * 16 + (size_t)local * 1024 * sizeof(int32_t));
        if (rc) return rc;
        sp.live = c->d.live.as<int32_t>();
        sp.live_pos = (int32_t*)(c->d.live.as<char>() + (size_t)std::max(nlive, 1) * 16);
        rc = launched(sched_launch_live(sp, true, s));
        if (rc) return rc;
        c->nlive = nlive;
      }
    }
    // (a rank with no tiles -- more ranks than the frame has tiles -- renders
    // nothing: no scheduler launch, no read-back of counts it never wrote)
    memcpy(c->order_key, key, sizeof key);
    c->stats.schedules_built += 1;
    // a new key's first frame measures (state 1), the next re-cuts (2 -> 3)
    c->meas_state = remeasured ? 3 : (tn.measure && local > 0 ? 1 : 0);
  }
  // split pixels: one copy of their radiance rows, hit bits and sub-block
  // counters per frame a launch renders (`frames`), laid out as [copies of
  // the rows][copies of the bits][copies of the counters].  Bits and counters
  // start at zero; each launch's last sub-block of a pixel zeroes them again
  // (rt_body.h), so they are cleared only when the layout changes.
  const size_t rows = (size_t)c->nsplit * st->samples * 3 * sizeof(double);
  const size_t flags = split_flags_bytes(c->nsplit, st->samples);
  if (c->nsplit && c->split_frames < frames) {
    int rc = quiesce(c);  // earlier launches may still use the rows
    if (rc) return rc;
    rc = grow(c, &c->d.split, (rows + flags) * (size_t)frames + 256);
    if (rc) return rc;
    HIP_TRY(hipMemsetAsync(c->d.split.as<char>() + rows * (size_t)frames, 0, flags * (size_t)frames, s));
    c->split_frames = frames;
  }
  const size_t nf = (size_t)std::max(c->split_frames, 1);
  char* const split = c->d.split.as<char>();
  p->blocks = c->d.blocks.as<int32_t>();
  p->num_blocks = c->num_blocks;
  p->nsplit = c->nsplit;
  p->split_frames = c->split_frames;
  p->split_rad = c->nsplit ? (double*)split : nullptr;
  p->split_hits = c->nsplit ? (uint32_t*)(split + rows * nf) : nullptr;
  p->split_cnt = c->nsplit ? (int32_t*)(p->split_hits + (size_t)c->nsplit * ((st->samples + 31) / 32) * nf) : nullptr;
  p->tile_masks = ((masks && frustum) || active) ? c->d_masks : nullptr;
  return RT_OK;
}

// A streamed launch of the nframes frames of p (its frame_*
// entries; one frame: the single-frame fields), whose schedule holds a
// live-pixel list: render_stream_kernel + resolve_rows_kernel per group of
// consecutive frames whose rows (24 B per live pixel, sample and frame) fit
// the budget rt_tuning.stream_max_mb (default 1 GiB: the headline launch's 25
// frames take 573 MB).  *streamed stays false when the launch is not eligible
// or not even two of its frames (the frame of a one-frame launch) fit: it then
// takes the block kernel as before.
// cams (a camera sequence): the frames' CamFrame table.
static int render_stream(rt_context* c, const KParams& p, const rt_settings* st, int nframes, int key_frames,
                         hipStream_t s, bool* streamed, const CamFrame* cams = nullptr) {
  *streamed = false;
  const bool prog = p.acc_mode == kAccProgressive && nframes == 1;
  if (!stream_wanted(c, p, st, key_frames) || c->nlive < 0 || p.counts || p.work_max || (p.acc_mode != 0 && !prog) ||
      p.sky)
    return RT_OK;
  const rt_tuning& tn = c->tun;
  const size_t budget = (size_t)((tn.stream_max_mb > 0 ? tn.stream_max_mb : 1024.0) * 1048576.0);
  const size_t per_entries = (size_t)c->nlive * (size_t)p.spp, per_bytes = per_entries * 24;
  size_t fit = (size_t)nframes;
  if (per_entries > 0) fit = std::min(budget / per_bytes, (size_t)0x7FFFFFFF / per_entries);
  const int group = (int)std::min<size_t>((size_t)nframes, fit);
  if (group < std::min(nframes, 2)) return RT_OK;
  // the grid: the resident waves of the kernel this launch takes (cached per
  // kernel; a new scene can change its dynamic LDS)
  const int kid = stream_kernel_of(p, cams != nullptr);
  const size_t shmem = render_shmem(p);
  if (c->wave_slots[kid] <= 0 || c->wave_shmem[kid] != shmem) {
    c->wave_slots[kid] = stream_wave_slots(c->device, kid, shmem);
    c->wave_shmem[kid] = shmem;
  }
  const int wave_slots = c->wave_slots[kid];
  if (wave_slots <= 0) {
    set_error("stream launch: the device reports no resident waves for the stream kernel");
    return RT_E_DEVICE;
  }
  // [cursor word, 256 B][rows of the largest group]
  int rc = grow(c, &c->d.rows, 256 + std::max<size_t>((size_t)group * per_bytes, 24));
  if (rc) return rc;
  StreamParams sp;
  memset(&sp, 0, sizeof sp);
  sp.live = c->d.live.as<const int32_t>();
  sp.live_pos = (const int32_t*)(c->d.live.as<char>() + (size_t)std::max(c->nlive, 1) * 16);
  sp.tile_list = dev_tiles(c, p.W, p.H, p.rank, p.world);
  sp.cursor = c->d.rows.as<unsigned int>();
  sp.rows = (double*)(c->d.rows.as<char>() + 256);
  sp.nlive = c->nlive;
  sp.npix = c->live_local * 1024;
  sp.chunk = tn.stream_chunk > 0 ? tn.stream_chunk : 512;
  sp.order = tn.stream_order;
  sp.acc = prog ? p.acc : nullptr;  // (the resolve continues the progression's sums)
  sp.cams = cams;
  for (int f0 = 0; f0 < nframes; f0 += group) {
    sp.frame0 = f0;
    sp.frames = std::min(group, nframes - f0);
    sp.total = (uint32_t)((size_t)sp.frames * per_entries);
    sp.dec = stream_decode_of(sp.order, (uint32_t)sp.frames, (uint32_t)sp.nlive, (uint32_t)p.spp);
    const int e = launch_stream(p, sp, wave_slots, s);
    if (e != hipSuccess) return launch_failed("stream", e);
    c->stats.stream_launches += 1;
  }
  *streamed = true;
  return RT_OK;
}

// One megakernel launch of p's nframes frames (key_frames: the frames per
// launch of its schedule key): streamed where that applies, else the block
// kernel, with tail helpers where those apply.  Every caller goes through
// here, so the guards their copies once differed in are these:
//  - dropped as implied: an order of setup_tail and render_stream (setup_tail
//    has no effect unless rt_tuning.tail_helpers >= 0, a stream needs it < 0),
//    and a caller's "one pass, not counting" test around both (each refuses
//    p->counts, p->work_max and the acc_mode of a frame's sample passes itself);
//  - kept, as one_pass: the last sub-pass of a progression's add of several
//    has acc_mode kAccProgressive like an add of one launch, which may
//    stream; every sub-pass of such an add takes the block kernel.
static int launch_megakernel(rt_context* c, KParams* p, const rt_settings* st, int nframes, int key_frames,
                             hipStream_t s, bool one_pass = true) {
  bool streamed = false;
  int rc = one_pass ? render_stream(c, *p, st, nframes, key_frames, s, &streamed) : RT_OK;
  if (rc || streamed) return rc;
  rc = setup_tail(c, p, s);
  if (rc) return rc;
  const int e = launch_render(*p, p->counts != nullptr, s);
  return e == hipSuccess ? (int)RT_OK : launch_failed("render", e);
}

// Sample passes a frame or an add of n samples takes.  The megakernel holds
// at most kMaxBlockSamples samples of a pixel in one block: more samples per
// pixel render as consecutive SAMPLE PASSES of at most that many, each
// continuing every pixel's running sum in sample order (KParams.acc), so the
// sum is tracePixel's bit for bit.
static int sample_passes(int n) { return std::max(1, (n + kMaxBlockSamples - 1) / kMaxBlockSamples); }

int render_passes(rt_context* c, KParams* pp, const rt_settings* st, hipStream_t s, const PassOpts& o) {
  KParams& p = *pp;
  const int w = p.W, h = p.H, rank = p.rank, world = p.world;
  const bool wf = use_wavefront(c);
  const int npass = wf ? 1 : sample_passes(o.n);
  const size_t npx = (size_t)local_tiles(c, w, h, rank, world) * 1024;
  rt_counts* const counts = o.counts;
  int rc;
  p.spp_total = o.spp_total;  // the divisor of the mean
  if (npass > 1 && !o.keep && (rc = grow(c, o.acc, npx * 3 * sizeof(double)))) return rc;
  if (npass > 1 || o.keep) p.acc = o.acc->as<double>();
  unsigned long long total[kCountSlots] = {0};
  bool measuring = false;
  for (int pass = 0; pass < npass; ++pass) {
    rt_settings ps = *st;
    const int s0 = (int)((long long)o.n * pass / npass), s1 = (int)((long long)o.n * (pass + 1) / npass);
    const bool last = pass == npass - 1;
    ps.samples = s1 - s0;
    p.spp = ps.samples;
    p.sample_base = o.first + s0;
    // a progression's sums start at zero, so its first add continues them like
    // any other, and only its last pass writes the image (keeping the sums)
    p.acc_mode = o.keep ? (1 | (last ? 4 : 2)) : ((pass > 0 ? 1 : 0) | (last ? 0 : 2));
    if (!wf) {
      // (keyed by the pass's sample count, not by sample_base: equal adds share a schedule)
      rc = prepare_schedule(c, &p, &ps, s, o.key_frames, o.active, o.active_gen, o.cam);
      if (rc) return rc;
    }
    p.num_wgs = p.num_blocks;
    // the first frame of a new schedule measures every pixel's paths (the same
    // image; a separate instantiation records the lengths): the next frame's
    // blocks are cut from them (prepare_schedule)
    if (o.may_measure && !wf && npass == 1 && c->meas_state == 1 && !counts && st->sky == RT_SKY_NONE &&
        p.num_blocks > 0) {
      rc = grow(c, &c->d.meas, npx * 8);
      if (rc) return rc;
      p.work_max = c->d.meas.as<unsigned int>();
      p.work_sum = p.work_max + npx;
      measuring = true;
    }
    if (counts) HIP_TRY(hipMemsetAsync(p.counts, 0, kCountSlots * sizeof(unsigned long long), s));
    if (measuring) HIP_TRY(hipMemsetAsync(c->d.meas.p, 0, npx * 8, s));
    if (pass == 0) HIP_TRY(hipEventRecord(c->ev0, s));
    rc = wf ? render_wavefront(c, p, &ps, s, counts != nullptr, o.active)
            : launch_megakernel(c, &p, &ps, 1, o.key_frames, s, npass == 1);
    if (rc) return rc;
    if (counts) {
      unsigned long long h_c[kCountSlots];
      HIP_TRY(hipMemcpyAsync(h_c, p.counts, sizeof h_c, hipMemcpyDeviceToHost, s));
      HIP_TRY(hipStreamSynchronize(s));
      for (int i = 0; i < kCountSlots; ++i) total[i] += h_c[i];
    }
  }
  if (measuring) {
    c->meas_state = 2;
    c->stats.measuring_frames += 1;
  }
  c->stats.frames += 1;
  c->stats.launches += npass;
  if (counts) {
    const unsigned long long* h_c = total;
    counts->camera_rays = h_c[0];
    counts->bounce_rays = h_c[1];
    counts->shadow_rays = h_c[2];
    counts->sphere_tests = h_c[3];
    counts->triangle_tests = h_c[4];
    counts->box_tests = h_c[5];
    counts->shade_events = h_c[6];
    counts->light_evals = h_c[7];
    counts->rng_draws = h_c[8];
    for (int i = 0; i < kCounters; ++i) {
      counts->culled[i] = h_c[kCounters + i];
      counts->soft_occlusion[i] = h_c[kGroupSoft * kCounters + i];
      counts->extend[i] = h_c[kGroupExtend * kCounters + i];
      counts->hard_occlusion[i] = h_c[kGroupHard * kCounters + i];
    }
  }
  return RT_OK;
}

}  // namespace rtgo

using namespace rtgo;

// One frame (rt_context_render_async).  key_frames: the frames per launch
// whose schedule this frame uses -- 1 for a frame of its own; n when it is
// one of n frames that rt_context_render_frames_async renders one at a time
// (a measuring frame): the schedule key then stays the batched launch's, so
// the measured re-cut is the one the next batched launch reuses.
// cam: the frame shoots from this CamFrame instead of the scene's camera (a
// camera sequence's frame rendered alone): the override goes
// into base_params, the flattened scene keeps its camera, and the frame's
// schedule is keyed by a generation of its own -- never shared, rebuilt for
// every such frame.
static int render_one(rt_context* c, int32_t w, int32_t h, const rt_settings* st, int32_t rank, int32_t world,
                      int32_t layout, float* d_linear, uint8_t* d_rgba, void* stream, rt_counts* counts,
                      int key_frames, const CamFrame* cam = nullptr) {
  int rc = check_frame_args(c, w, h, st, rank, world, layout);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  KParams p;
  base_params(c, w, h, st, rank, world, layout, &p, cam);
  p.out_linear = d_linear;
  p.out_rgba = d_rgba;
  if (counts && (rc = grow(c, &c->d.counts, kCountSlots * sizeof(unsigned long long)))) return rc;
  p.counts = counts ? c->d.counts.as<unsigned long long>() : nullptr;
  hipStream_t s = (hipStream_t)stream;
  PassOpts o;
  o.n = o.spp_total = st->samples;
  o.acc = &c->d.acc;
  o.key_frames = key_frames;
  o.counts = counts;
  o.may_measure = true;
  if (cam) o.cam.gen = -(++c->cam_gen);
  rc = enter_stream(c, s);
  if (!rc) rc = render_passes(c, &p, st, s, o);
  return rc ? rc : leave_stream(c, s);
}

extern "C" {

int rt_context_render_async(rt_context* c, int32_t w, int32_t h, const rt_settings* st, int32_t rank,
                            int32_t world, int32_t layout, float* d_linear, uint8_t* d_rgba, void* stream,
                            rt_counts* counts) {
  return render_one(c, w, h, st, rank, world, layout, d_linear, d_rgba, stream, counts, 1);
}

// Several frames of one schedule in ONE launch (include/rt_api.h).
int rt_context_render_frames_async(rt_context* c, int32_t w, int32_t h, const rt_settings* st, int32_t nframes,
                                   const uint64_t* seeds, int32_t rank, int32_t world, int32_t layout,
                                   float* const* d_linear, uint8_t* const* d_rgba, void* stream) {
  // (a context without a scene is check_frame_args's first finding, as ever)
  if (c && c->have_scene && (nframes < 1 || nframes > RT_MAX_FRAMES || !seeds || !d_linear)) {
    set_error("rt_context_render_frames_async: nframes must be in [1, RT_MAX_FRAMES] with seeds and d_linear given");
    return RT_E_INVALID;
  }
  int rc = check_frame_args(c, w, h, st, rank, world, layout);
  if (rc) return rc;
  // one frame at a time where a launch cannot hold several: the wavefront
  // path (host-driven bounce loop), sample passes, a measuring frame
  // (frame by frame under the batched launch's schedule key: a measuring
  // frame then measures the schedule the next batched launch uses)
  auto one_by_one = [&]() {
    for (int f = 0; f < nframes; ++f) {
      rt_settings sf = *st;
      sf.seed = seeds[f];
      int r = render_one(c, w, h, &sf, rank, world, layout, d_linear[f], d_rgba ? d_rgba[f] : nullptr, stream,
                         nullptr, nframes);
      if (r) return r;
    }
    return (int)RT_OK;
  };
  if (nframes == 1 || use_wavefront(c) || sample_passes(st->samples) > 1 || (c->tun.measure && c->meas_state != 3))
    return one_by_one();
  HIP_TRY(hipSetDevice(c->device));
  KParams p;
  base_params(c, w, h, st, rank, world, layout, &p);
  hipStream_t s = (hipStream_t)stream;
  rc = enter_stream(c, s);
  if (rc) return rc;
  p.spp_total = st->samples;
  rc = prepare_schedule(c, &p, st, s, nframes);
  if (rc) return rc;
  // a new schedule key whose first frame is to measure (rt_tuning.measure):
  // that frame goes through the single-frame path, which records the paths
  if (c->tun.measure && c->meas_state == 1) return one_by_one();
  p.nframes = nframes;
  for (int f = 0; f < nframes; ++f) {
    p.frame_key[f] = rt_rng_seed_key(seeds[f]);
    p.frame_lin[f] = d_linear[f];
    p.frame_rgba[f] = d_rgba ? d_rgba[f] : nullptr;
  }
  p.num_wgs = p.num_blocks * nframes;
  HIP_TRY(hipEventRecord(c->ev0, s));
  rc = launch_megakernel(c, &p, st, nframes, nframes, s);
  if (rc) return rc;
  c->stats.frames += nframes;
  c->stats.launches += 1;
  c->stats.batched_launches += 1;
  return leave_stream(c, s);
}

// The frames of one launch, each with a camera of its own (include/rt_api.h,
// DESIGN.md §4.11).  Where a batched launch of nframes frames would stream
// (stream_wanted), the frames are ONE streamed launch on one schedule whose
// live-pixel list is the union over the cameras; everywhere else -- one frame,
// the wavefront path, sample passes, a sky, a measuring schedule, tail
// helpers, triangles under the auto rule, a row budget that holds fewer than
// two frames -- they render frame by frame, each with its camera as an
// override of base_params: correct and slow, a new schedule per frame.
int rt_context_render_cameras_async(rt_context* c, int32_t w, int32_t h, const rt_settings* st, int32_t nframes,
                                    const rt_camera* cameras, const uint64_t* seeds, int32_t rank, int32_t world,
                                    int32_t layout, float* const* d_linear, uint8_t* const* d_rgba, void* stream) {
  if (c && c->have_scene && (nframes < 1 || nframes > RT_MAX_FRAMES || !cameras || !d_linear)) {
    set_error("rt_context_render_cameras_async: nframes must be in [1, RT_MAX_FRAMES] with cameras and d_linear given");
    return RT_E_INVALID;
  }
  int rc = check_frame_args(c, w, h, st, rank, world, layout);
  if (rc) return rc;
  // every frame's CamFrame, before anything is enqueued (the caller's cameras are not read again)
  CamTable tab;
  memset(&tab, 0, sizeof tab);
  for (int f = 0; f < nframes; ++f) {
    rc = camera_frame(cameras[f], st->camera, w, h, &tab.f[f]);
    if (rc) {
      set_error("rt_context_render_cameras_async: camera of frame " + std::to_string(f) + ": " + rt_last_error());
      return rc;
    }
  }
  auto seed_of = [&](int f) { return seeds ? seeds[f] : st->seed; };
  auto one_by_one = [&]() {
    for (int f = 0; f < nframes; ++f) {
      rt_settings sf = *st;
      sf.seed = seed_of(f);
      int r = render_one(c, w, h, &sf, rank, world, layout, d_linear[f], d_rgba ? d_rgba[f] : nullptr, stream, nullptr,
                         1, &tab.f[f]);
      if (r) return r;
    }
    return (int)RT_OK;
  };
  KParams p;
  base_params(c, w, h, st, rank, world, layout, &p, &tab.f[0]);
  p.spp_total = st->samples;
  if (nframes == 1 || use_wavefront(c) || !stream_wanted(c, p, st, nframes)) return one_by_one();
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  rc = enter_stream(c, s);
  if (rc) return rc;
  // the set's table in d.cams: written when the set differs from the last one
  // (the same set again, other seeds, reuses table, generation and schedule)
  if (c->seq_n != nframes || memcmp(&c->seq_cams, &tab, sizeof tab) != 0) {
    rc = grow(c, &c->d.cams, sizeof(CamTable));
    if (rc) return rc;
    const int e = launch_cam_upload(tab, nframes, c->d.cams.as<CamFrame>(), s);
    if (e != hipSuccess) {
      c->seq_n = 0;
      return launch_failed("camera table", e);
    }
    c->seq_cams = tab;
    c->seq_n = nframes;
    c->seq_gen = ++c->cam_gen;
  }
  // (the shadow-cone rows hold for every frame's rays, or for the launch not at all)
  for (int f = 1; f < nframes && p.cone_rows_off; ++f)
    if (!cone_rows_hold(c->flat, tab.f[f].o)) p.cone_rows_off = 0;
  CamKey key;
  key.gen = c->seq_gen;
  key.frames = c->seq_cams.f;
  key.n = nframes;
  rc = prepare_schedule(c, &p, st, s, nframes, nullptr, 0, key);
  if (rc) return rc;
  p.nframes = nframes;
  for (int f = 0; f < nframes; ++f) {
    p.frame_key[f] = rt_rng_seed_key(seed_of(f));
    p.frame_lin[f] = d_linear[f];
    p.frame_rgba[f] = d_rgba ? d_rgba[f] : nullptr;
  }
  p.num_wgs = p.num_blocks * nframes;
  HIP_TRY(hipEventRecord(c->ev0, s));
  bool streamed = false;
  rc = render_stream(c, p, st, nframes, nframes, s, &streamed, c->d.cams.as<const CamFrame>());
  if (rc) return rc;
  // (a rank without tiles, or rows of two frames past the budget: the block
  // kernel has no camera per frame)
  if (!streamed) return one_by_one();
  c->stats.frames += nframes;
  c->stats.launches += 1;
  c->stats.batched_launches += 1;
  return leave_stream(c, s);
}

// First-hit feature buffers (include/rt_api.h): one launch of
// rt_aov.hip's kernel over the whole frame, timed like a render (ev0 .. ev1) and
// ordered behind the context's last launch, but with no schedule, no counts in
// the statistics and no state of a progression touched.
// The checks and parameters that both feature passes share (`who`: the call's
// name for the messages; the five common outputs are the caller's to set).
static int aov_setup(rt_context* c, int32_t w, int32_t h, const rt_settings* st, const rt_camera* camera,
                     const char* who, AovParams* p) {
  if (!c->have_scene) {
    set_error("context has no scene");
    return RT_E_INVALID;
  }
  if (st->samples < 1) {
    set_error(std::string(who) + ": samples must be at least 1");
    return RT_E_INVALID;
  }
  int rc = check_settings(st, w, h);
  if (rc) return rc;
  memset(p, 0, sizeof *p);
  // (the caller's camera is read here and not again)
  rc = camera_frame(camera ? *camera : c->flat.camera, st->camera, w, h, &p->cf);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const FlatScene& f = c->flat;
  const int32_t use_bvh = f.bvh.empty() ? 0 : (bvh_has_cubes(f) ? 2 : 1);
  p->g = Geo{c->d_spheres, c->d_tris, c->d_boxes, c->d_bvh, (int32_t)f.spheres.size(), (int32_t)f.tris.size(), use_bvh,
             (int32_t)f.boxes.size()};
  p->mats = c->d_mats;
  p->seed_key = rt_rng_seed_key(st->seed);
  p->W = w;
  p->H = h;
  p->spp = st->samples;
  p->stack_depth = std::max(1, f.bvh_depth);
  return RT_OK;
}

int rt_context_render_aov_async(rt_context* c, int32_t w, int32_t h, const rt_settings* st, const rt_camera* camera,
                                const rt_aov_buffers* out, void* stream) {
  if (!c || !st || !out) {
    set_error("rt_context_render_aov_async: context, settings or out is NULL");
    return RT_E_INVALID;
  }
  if (!out->d_albedo && !out->d_normal && !out->d_depth && !out->d_coverage && !out->d_object) {
    set_error("rt_context_render_aov_async: every buffer of out is NULL");
    return RT_E_INVALID;
  }
  AovParams p;
  int rc = aov_setup(c, w, h, st, camera, "rt_context_render_aov_async", &p);
  if (rc) return rc;
  p.albedo = out->d_albedo;
  p.normal = out->d_normal;
  p.depth = out->d_depth;
  p.coverage = out->d_coverage;
  p.object = out->d_object;
  hipStream_t s = (hipStream_t)stream;
  rc = enter_stream(c, s);
  if (rc) return rc;
  HIP_TRY(hipEventRecord(c->ev0, s));
  const int e = launch_aov(p, s);
  if (e != hipSuccess) return launch_failed("feature buffers", e);
  return leave_stream(c, s);
}

// Specular-through feature buffers (include/rt_api.h): the
// same call around rt_aov.hip's aov_spec_kernel.
void rt_aov_spec_default(rt_aov_spec* spec) {
  if (!spec) return;
  memset(spec, 0, sizeof *spec);
  spec->max_bounces = 4;
  spec->max_roughness = 0.1;  // a convention (what still looks like a mirror), not a measurement
}

static bool aov_spec_ok(const rt_aov_spec* sp) {
  return sp && sp->max_bounces >= 0 && sp->max_bounces <= 16 && std::isfinite(sp->max_roughness) &&
         sp->max_roughness >= 0;
}

int rt_aov_spec_follows(const rt_material* material, const rt_aov_spec* spec) {
  if (!material || !aov_spec_ok(spec)) {
    set_error("rt_aov_spec_follows: a material, max_bounces in [0, 16] and a finite max_roughness >= 0 are needed");
    return RT_E_INVALID;
  }
  return material_followed(*material, spec->max_roughness) ? 1 : 0;
}

int rt_context_render_aov_spec_async(rt_context* c, int32_t w, int32_t h, const rt_settings* st,
                                     const rt_camera* camera, const rt_aov_spec* spec, const rt_aov_spec_buffers* out,
                                     void* stream) {
  if (!c || !st || !out) {
    set_error("rt_context_render_aov_spec_async: context, settings or out is NULL");
    return RT_E_INVALID;
  }
  if (!aov_spec_ok(spec)) {
    set_error("rt_context_render_aov_spec_async: spec must be given, max_bounces in [0, 16], max_roughness finite and >= 0");
    return RT_E_INVALID;
  }
  if (!out->d_albedo && !out->d_normal && !out->d_depth && !out->d_coverage && !out->d_object && !out->d_specular &&
      !out->d_bounces) {
    set_error("rt_context_render_aov_spec_async: every buffer of out is NULL");
    return RT_E_INVALID;
  }
  AovSpecParams q;
  memset(&q, 0, sizeof q);
  int rc = aov_setup(c, w, h, st, camera, "rt_context_render_aov_spec_async", &q.a);
  if (rc) return rc;
  q.a.albedo = out->d_albedo;
  q.a.normal = out->d_normal;
  q.a.depth = out->d_depth;
  q.a.coverage = out->d_coverage;
  q.a.object = out->d_object;
  q.specular = out->d_specular;
  q.bounces = out->d_bounces;
  q.max_bounces = spec->max_bounces;
  q.max_roughness = spec->max_roughness;
  hipStream_t s = (hipStream_t)stream;
  rc = enter_stream(c, s);
  if (rc) return rc;
  HIP_TRY(hipEventRecord(c->ev0, s));
  const int e = launch_aov_spec(q, s);
  if (e != hipSuccess) return launch_failed("specular-through feature buffers", e);
  return leave_stream(c, s);
}

// Matte layers (include/rt_api.h): the same call around
// rt_matte.hip's matte_kernel.
void rt_matte_default(rt_matte* m) {
  if (!m) return;
  memset(m, 0, sizeof *m);
  m->ranks = 4;
  m->level = RT_MATTE_OBJECT;
}

int rt_context_render_matte_async(rt_context* c, int32_t w, int32_t h, const rt_settings* st, const rt_camera* camera,
                                  const rt_matte* params, const rt_matte_buffers* out, void* stream) {
  if (!c || !st || !out || !params) {
    set_error("rt_context_render_matte_async: context, settings, params or out is NULL");
    return RT_E_INVALID;
  }
  if (params->ranks < 1 || params->ranks > RT_MATTE_MAX_RANKS ||
      (params->level != RT_MATTE_OBJECT && params->level != RT_MATTE_FACE)) {
    set_error("rt_context_render_matte_async: ranks must be in 1..8 and level RT_MATTE_OBJECT or RT_MATTE_FACE");
    return RT_E_INVALID;
  }
  if (!out->d_id && !out->d_count && !out->d_rest) {
    set_error("rt_context_render_matte_async: every buffer of out is NULL");
    return RT_E_INVALID;
  }
  MatteParams q;
  memset(&q, 0, sizeof q);
  int rc = aov_setup(c, w, h, st, camera, "rt_context_render_matte_async", &q.a);
  if (rc) return rc;
  if (params->level == RT_MATTE_FACE && c->flat.objects >= (1 << 27)) {
    set_error("rt_context_render_matte_async: the face level serves scenes of fewer than 2^27 objects");
    return RT_E_INVALID;
  }
  q.level = params->level;
  q.ranks = params->ranks;
  q.id = out->d_id;
  q.count = out->d_count;
  q.rest = out->d_rest;
  hipStream_t s = (hipStream_t)stream;
  rc = enter_stream(c, s);
  if (rc) return rc;
  HIP_TRY(hipEventRecord(c->ev0, s));
  const int e = launch_matte(q, s);
  if (e != hipSuccess) return launch_failed("matte layers", e);
  return leave_stream(c, s);
}

// rt_camera_orbit (include/rt_api.h states the formula and its order)
int rt_camera_orbit(const rt_camera* cam, int32_t n, double degrees, rt_camera* out) {
  if (!cam || !out || n < 1) {
    set_error("rt_camera_orbit: cam and out must be given and n >= 1");
    return RT_E_INVALID;
  }
  const double fields[12] = {cam->position[0], cam->position[1], cam->position[2], cam->look_at[0],
                             cam->look_at[1],  cam->look_at[2],  cam->up[0],       cam->up[1],
                             cam->up[2],       cam->fov,         cam->aspect_ratio, degrees};
  for (double v : fields)
    if (!std::isfinite(v)) {
      set_error("rt_camera_orbit: the camera's fields and degrees must be finite");
      return RT_E_INVALID;
    }
  const double ul = sqrt(cam->up[0] * cam->up[0] + cam->up[1] * cam->up[1] + cam->up[2] * cam->up[2]);
  if (!(ul > 0)) {
    set_error("rt_camera_orbit: up is zero");
    return RT_E_INVALID;
  }
  const double a[3] = {cam->up[0] / ul, cam->up[1] / ul, cam->up[2] / ul};
  double v[3];
  for (int k = 0; k < 3; ++k) v[k] = cam->position[k] - cam->look_at[k];
  const double axv[3] = {a[1] * v[2] - a[2] * v[1], a[2] * v[0] - a[0] * v[2], a[0] * v[1] - a[1] * v[0]};
  const double adv = a[0] * v[0] + a[1] * v[1] + a[2] * v[2];
  const rt_camera in = *cam;  // (out may alias cam)
  for (int32_t k = 0; k < n; ++k) {
    out[k] = in;
    if (k == 0) continue;  // bit for bit the input
    const double th = (degrees * k / n) * (M_PI / 180);
    const double ct = cos(th), st = sin(th);
    for (int i = 0; i < 3; ++i)
      out[k].position[i] = in.look_at[i] + v[i] * ct + axv[i] * st + a[i] * adv * (1 - ct);
  }
  return RT_OK;
}

}  // extern "C"
