// sched_probe.cpp — TEST INFRASTRUCTURE: the GPU work scheduler
// (csrc/rt_schedule.hip) and its host half (csrc/schedule.cpp) run on plain
// arrays (tests/test_gpu_sched_probe.py, tests/sched_cases.py).
//
// An image does not depend on how the work is cut and ordered, so no render can
// tell whether the schedule is the one its definitions describe.  Here the
// product's own launchers run the product's own sequence (prepare_schedule,
// rt_render.cpp) on inputs a test chooses, and every buffer they write comes
// back to the host.
//
// Host only.  Linked into build/probe/librtprobe.so with the product's
// build/rt_schedule.o and build/schedule.o as they are, so the library carries
// its own copy of rtgo::sched_* and tile_primary_masks, as it does of
// flatten_scene.  The library is linked with -Bsymbolic (Makefile): a call from
// here binds to that copy even when librtgo.so, which exports the same names,
// is loaded into the same process first.
//
// Safety before coverage: only parameter sets that prepare_schedule can produce
// are launched (the checks at the head of rtp_sched_run), every input array
// must have exactly the expected length, every launch's return value is checked
// and the sequence stops at the first error.  The probe owns its device memory; every buffer the kernels
// write is filled with 0xA5 first and followed by a 4-KiB guard of the same
// byte, and the run reports whether every guard came back untouched.
#include <hip/hip_runtime_api.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <vector>

#include "../../concurrent-raytracer-go_amd/csrc/rt_internal.h"

using namespace rtgo;

namespace {

constexpr size_t kGuard = 4096;
constexpr unsigned char kPoison = 0xA5;
constexpr int kMaxLocal = 16;
constexpr int kBuckets = 128;  // rt_schedule.hip's weight classes

// One device buffer of the probe: `bytes` of payload, then the guard.
struct Buf {
  char* d = nullptr;
  size_t bytes = 0;
  ~Buf() {
    if (d) (void)hipFree(d);
  }
  int alloc(size_t n) {
    bytes = n;
    if (hipMalloc((void**)&d, n + kGuard) != hipSuccess) return -2;
    if (hipMemset(d, kPoison, n + kGuard) != hipSuccess) return -2;
    return 0;
  }
  int upload(const void* src, size_t n) {
    if (int rc = alloc(n)) return rc;
    return n && hipMemcpy(d, src, n, hipMemcpyHostToDevice) != hipSuccess ? -2 : 0;
  }
  // 1: the guard holds the poison byte everywhere; 0: it was written; < 0: error
  int guard_ok() const {
    unsigned char g[kGuard];
    if (hipMemcpy(g, d + bytes, kGuard, hipMemcpyDeviceToHost) != hipSuccess) return -2;
    for (size_t i = 0; i < kGuard; ++i)
      if (g[i] != kPoison) return 0;
    return 1;
  }
  int download(void* dst, size_t off, size_t n) const {
    if (off + n > bytes) return -1;
    return n && hipMemcpy(dst, d + off, n, hipMemcpyDeviceToHost) != hipSuccess ? -2 : 0;
  }
};

void frame_of(const double f[12], int32_t model, CamFrame* cf) {
  memset(cf, 0, sizeof *cf);
  for (int k = 0; k < 3; ++k) {
    cf->o[k] = f[k];
    cf->ll[k] = f[3 + k];
    cf->h[k] = f[6 + k];
    cf->v[k] = f[9 + k];
  }
  cf->model = model;
}

bool model_ok(int32_t m) { return m == RT_CAMERA_REFERENCE || m == RT_CAMERA_LOOKAT; }

}  // namespace

extern "C" {

// The run's description.  Every pointer is a HOST pointer; an optional input
// is null with length 0.  Lengths are in elements.
struct rtp_sched_args {
  int32_t W, H, rank, world, spp, big_pixels, frustum, split_samples;
  int32_t split_depth, work_n, work_mean, own_masks, ncams, model, want_tile_work, want_live;
  double block_work;
  const double* frames;  // 12 doubles (ncams == 0) or ncams * 12 (a sequence; frames[0..11] also fill SchedParams::cf)
  const void* spheres;   // DSphere records
  const void* tris;      // DTri records
  int64_t ns, nt;
  const int32_t* tile_list;
  const unsigned long long* tile_masks;  // local * 2, or (ncams + 1) * local * 2: [the OR][camera 0's] ...
  const float* tile_cost;
  const uint32_t* work_max;
  const uint32_t* work_sum;
  const uint32_t* active;
  int64_t n_tile_list, n_tile_masks, n_tile_cost, n_work_max, n_work_sum, n_active;
  // outputs, caller-allocated: per local pixel pixmask (2 u64), est, live_pos;
  // per local tile 16 pilot records and tile_work; hist, cursor, live_hist,
  // live_cursor: 128 ints each; totals: 4; blocks: cap_blocks records of 16
  // ints; live: local * 1024 items of 4 ints.  guards: the number of guards
  // found written (0 = all intact).
  unsigned long long* pixmask;
  float* est;
  int32_t* pilot_blocks;
  int32_t* hist;
  int32_t* cursor;
  int32_t* totals;
  int32_t* blocks;
  int32_t* live_hist;
  int32_t* live_cursor;
  int32_t* live;
  int32_t* live_pos;
  float* tile_work;
  int64_t cap_blocks;
  int32_t guards_written, local;
};

// A FlatScene that holds the given records and nothing else (what
// tile_primary_masks reads); freed with rtp_free.
void* rtp_flat_from_records(const void* spheres, int64_t ns, const void* tris, int64_t nt) {
  if (ns < 0 || nt < 0 || ns > 64 || nt > 64 || (ns && !spheres) || (nt && !tris)) return nullptr;
  FlatScene* fs = new (std::nothrow) FlatScene();
  if (!fs) return nullptr;
  fs->spheres.assign((const DSphere*)spheres, (const DSphere*)spheres + ns);
  fs->tris.assign((const DTri*)tris, (const DTri*)tris + nt);
  return fs;
}

// tile_primary_masks of the host: out[2 k], out[2 k + 1] for tiles[k].
int rtp_sched_tile_masks(const void* h, const double frame[12], int32_t model, int32_t W, int32_t H,
                         const int32_t* tiles, int64_t ntiles, unsigned long long* out) {
  const FlatScene* fs = (const FlatScene*)h;
  if (!fs || !frame || !out || !tiles || !model_ok(model) || W < 1 || H < 1 || W > 65536 || H > 65536) return -1;
  const int all = rt_num_tiles(W, H);
  if (ntiles < 1 || ntiles > all) return -1;
  for (int64_t k = 0; k < ntiles; ++k)
    if (tiles[k] < 0 || tiles[k] >= all) return -1;
  CamFrame cf;
  frame_of(frame, model, &cf);
  std::vector<int32_t> tl(tiles, tiles + ntiles);
  std::vector<unsigned long long> m;
  tile_primary_masks(*fs, cf, W, H, tl, &m);
  if ((int64_t)m.size() != 2 * ntiles) return -1;
  memcpy(out, m.data(), m.size() * sizeof(unsigned long long));
  return 0;
}

// The product's sequence as prepare_schedule runs it.  0: done (a->local,
// a->guards_written and the outputs set); -1: a parameter set the probe does
// not launch (nothing was launched); -2: a HIP call failed; -3: cap_blocks too
// small for totals[0]; > 0: the hipError_t of a launch (the sequence stopped).
int rtp_sched_run(rtp_sched_args* a) {
  if (!a) return -1;
  // ---- what prepare_schedule can produce
  if (a->W < 1 || a->H < 1 || a->W > 65536 || a->H > 65536) return -1;
  const int ntiles = rt_num_tiles(a->W, a->H);
  std::vector<int32_t> tiles;
  if (a->tile_list) {
    if (a->n_tile_list < 1 || a->n_tile_list > kMaxLocal) return -1;
    std::vector<char> seen(ntiles, 0);
    for (int64_t k = 0; k < a->n_tile_list; ++k) {
      const int32_t t = a->tile_list[k];
      if (t < 0 || t >= ntiles || seen[t]) return -1;
      seen[t] = 1;
      tiles.push_back(t);
    }
  } else {
    if (a->n_tile_list != 0 || a->world < 1 || a->rank < 0 || a->rank >= a->world) return -1;
    strided_tiles(a->W, a->H, a->rank, a->world, &tiles);
  }
  const int local = (int)tiles.size();
  if (local < 1 || local > kMaxLocal) return -1;
  if (a->spp < 1 || a->spp > 1024 || a->big_pixels < 1 || a->big_pixels > 64) return -1;
  if (a->split_samples < 1 || a->split_samples > 64 || a->split_depth < 1) return -1;
  if (!std::isfinite(a->block_work) || !(a->block_work >= 1.0)) return -1;
  if (!model_ok(a->model) || !a->frames || a->ncams < 0 || a->ncams > kMaxFrames) return -1;
  if (a->ns < 0 || a->ns > 64 || a->nt < 0 || a->nt > 64 || (a->ns && !a->spheres) || (a->nt && !a->tris)) return -1;
  if ((a->frustum != 0 && a->frustum != 1) || (a->own_masks != 0 && a->own_masks != 1)) return -1;
  if ((a->work_mean != 0 && a->work_mean != 1)) return -1;
  const size_t npx = (size_t)local * 1024;
  auto len_ok = [](const void* p, int64_t n, size_t want) { return p ? (size_t)n == want : n == 0; };
  const size_t nmask = (size_t)local * 2 * (size_t)(a->ncams > 0 ? a->ncams + 1 : 1);
  if (!len_ok(a->tile_masks, a->n_tile_masks, nmask) || !len_ok(a->tile_cost, a->n_tile_cost, (size_t)local) ||
      !len_ok(a->work_max, a->n_work_max, npx) || !len_ok(a->work_sum, a->n_work_sum, npx) ||
      !len_ok(a->active, a->n_active, npx))
    return -1;
  if (!a->tile_cost) return -1;                          // prepare_schedule always uploads the costs
  if ((a->work_max != nullptr) != (a->work_sum != nullptr)) return -1;
  if (a->work_max && (a->work_n < 1 || a->work_n > a->spp)) return -1;
  if (!a->work_max && (a->work_n != 0 || a->work_mean != 0)) return -1;
  if (a->active && (a->ncams > 0 || !a->tile_masks)) return -1;  // an adaptive add always has masks, never a sequence
  if (a->own_masks && !a->active) return -1;
  if (a->want_tile_work && a->active) return -1;  // (partitions are planned from plain pilots; it would redo the estimates)
  if (a->tile_masks && !a->own_masks) {  // the kernels index the records by the masks' bits
    const unsigned long long ok_s = a->ns >= 64 ? ~0ull : (1ull << a->ns) - 1ull;
    const unsigned long long ok_t = a->nt >= 64 ? ~0ull : (1ull << a->nt) - 1ull;
    for (size_t k = 0; k < nmask; k += 2)
      if ((a->tile_masks[k] & ~ok_s) || (a->tile_masks[k + 1] & ~ok_t)) return -1;
  }
  if (!a->pixmask || !a->est || !a->pilot_blocks || !a->hist || !a->cursor || !a->totals || !a->blocks ||
      !a->live_hist || !a->live_cursor || !a->live || !a->live_pos || !a->tile_work || a->cap_blocks < 1)
    return -1;

  // ---- device memory: inputs, then the scratch laid out by sched_layout
  Buf d_sph, d_tri, d_masks, d_cost, d_list, d_wmax, d_wsum, d_active, d_cams, d_scratch, d_blocks, d_live, d_tw;
  int rc;
  if ((rc = d_sph.upload(a->spheres, (size_t)a->ns * sizeof(DSphere)))) return rc;
  if ((rc = d_tri.upload(a->tris, (size_t)a->nt * sizeof(DTri)))) return rc;
  if (a->tile_masks && (rc = d_masks.upload(a->tile_masks, nmask * 8))) return rc;
  if ((rc = d_cost.upload(a->tile_cost, (size_t)local * 4))) return rc;
  if (a->tile_list && (rc = d_list.upload(a->tile_list, (size_t)local * 4))) return rc;
  if (a->work_max && ((rc = d_wmax.upload(a->work_max, npx * 4)) || (rc = d_wsum.upload(a->work_sum, npx * 4))))
    return rc;
  if (a->active && (rc = d_active.upload(a->active, npx * 4))) return rc;
  std::vector<CamFrame> cams((size_t)std::max(a->ncams, 1));
  for (size_t k = 0; k < cams.size(); ++k) frame_of(a->frames + 12 * k, a->model, &cams[k]);
  if (a->ncams > 0 && (rc = d_cams.upload(cams.data(), cams.size() * sizeof(CamFrame)))) return rc;
  const size_t scratch = sched_scratch_bytes(local);
  if ((rc = d_scratch.alloc(scratch))) return rc;
  if ((rc = d_tw.alloc((size_t)local * 4))) return rc;

  SchedParams sp;
  memset(&sp, 0, sizeof sp);
  sched_layout(d_scratch.d, local, &sp);
  sp.spheres = (const DSphere*)d_sph.d;
  sp.tris = (const DTri*)d_tri.d;
  sp.cf = cams[0];
  sp.W = a->W;
  sp.H = a->H;
  sp.rank = a->tile_list ? 0 : a->rank;
  sp.world = a->tile_list ? 1 : a->world;
  sp.tiles_x = (a->W + 31) / 32;
  sp.ntiles = ntiles;
  sp.local = local;
  sp.spp = a->spp;
  sp.big_pixels = a->big_pixels;
  sp.frustum = a->frustum;
  sp.split_samples = a->split_samples;
  sp.split_depth = a->split_depth;
  sp.block_work = a->block_work;
  sp.tile_masks = a->tile_masks ? (const unsigned long long*)d_masks.d : nullptr;
  sp.tile_cost = (const float*)d_cost.d;
  sp.tile_list = a->tile_list ? (const int32_t*)d_list.d : nullptr;
  sp.active = a->active ? (const uint32_t*)d_active.d : nullptr;
  sp.own_masks = a->own_masks;

  // ---- the sequence (every step on the null stream; the copies synchronize)
  rc = a->ncams > 0 ? sched_launch_pixels_seq(sp, (const CamFrame*)d_cams.d, a->ncams,
                                              sp.tile_masks ? sp.tile_masks + (size_t)local * 2 : nullptr, nullptr)
                    : sched_launch_pixels(sp, nullptr);
  if (rc) return rc > 0 ? rc : -2;
  if (a->work_max) {
    sp.work_max = (const unsigned int*)d_wmax.d;
    sp.work_sum = (const unsigned int*)d_wsum.d;
    sp.work_n = a->work_n;
    sp.work_mean = a->work_mean;
  }
  if ((rc = sched_launch_blocks(sp, false, nullptr))) return rc > 0 ? rc : -2;
  if (a->want_live && (rc = sched_launch_live(sp, false, nullptr))) return rc > 0 ? rc : -2;
  int32_t totals[4];
  if (hipMemcpy(totals, sp.totals, sizeof totals, hipMemcpyDeviceToHost) != hipSuccess) return -2;
  const int nblocks = totals[0];
  if (nblocks < 0 || nblocks > a->cap_blocks) return -3;
  if ((rc = d_blocks.alloc((size_t)std::max(nblocks, 1) * kBlockInts * sizeof(int32_t)))) return rc;
  sp.blocks = (int32_t*)d_blocks.d;
  if ((rc = sched_launch_blocks(sp, true, nullptr))) return rc > 0 ? rc : -2;
  int nlive = 0;
  if (a->want_live) {
    nlive = std::max(0, std::min(totals[3], local * 1024));
    const size_t list = (size_t)std::max(nlive, 1) * 16;
    if ((rc = d_live.alloc(list + npx * sizeof(int32_t)))) return rc;
    sp.live = (int32_t*)d_live.d;
    sp.live_pos = (int32_t*)(d_live.d + list);
    if ((rc = sched_launch_live(sp, true, nullptr))) return rc > 0 ? rc : -2;
  }
  if (a->want_tile_work && (rc = sched_launch_tile_work(sp, (float*)d_tw.d, nullptr))) return rc > 0 ? rc : -2;
  if (hipDeviceSynchronize() != hipSuccess) return -2;

  // ---- results
  const char* base = d_scratch.d;
  auto off = [&](const void* p) { return (size_t)((const char*)p - base); };
  if ((rc = d_scratch.download(a->pixmask, off(sp.pixmask), npx * 16))) return rc;
  if ((rc = d_scratch.download(a->est, off(sp.est), npx * 4))) return rc;
  if ((rc = d_scratch.download(a->pilot_blocks, off(sp.pilot_blocks), (size_t)local * 16 * kBlockInts * 4))) return rc;
  if ((rc = d_scratch.download(a->hist, off(sp.hist), kBuckets * 4))) return rc;
  if ((rc = d_scratch.download(a->cursor, off(sp.cursor), kBuckets * 4))) return rc;
  if ((rc = d_scratch.download(a->totals, off(sp.totals), 4 * 4))) return rc;
  if ((rc = d_scratch.download(a->live_hist, off(sp.live_hist), kBuckets * 4))) return rc;
  if ((rc = d_scratch.download(a->live_cursor, off(sp.live_cursor), kBuckets * 4))) return rc;
  if ((rc = d_blocks.download(a->blocks, 0, (size_t)nblocks * kBlockInts * 4))) return rc;
  if (a->want_live) {
    if ((rc = d_live.download(a->live, 0, (size_t)nlive * 16))) return rc;
    if ((rc = d_live.download(a->live_pos, (size_t)std::max(nlive, 1) * 16, npx * 4))) return rc;
  }
  if (a->want_tile_work && (rc = d_tw.download(a->tile_work, 0, (size_t)local * 4))) return rc;
  int written = 0;
  for (const Buf* b : {&d_scratch, &d_blocks, &d_live, &d_tw}) {
    if (!b->d) continue;
    const int g = b->guard_ok();
    if (g < 0) return g;
    if (!g) written += 1;
  }
  a->guards_written = written;
  a->local = local;
  return 0;
}

}  // extern "C"
