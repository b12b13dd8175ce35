// rt_internal.h — host-side interfaces between the C ABI (rt_api.cpp and the
// files around rt_context.h), the kernels (rt_kernel.hip, rt_stream.hip,
// rt_image_ops.hip, rt_wavefront.hip, rt_schedule.hip, rt_adaptive.hip, rt_aov.hip, rt_denoise.hip,
// rt_temporal.hip, rt_variance.hip), the
// scene loader (scene_json.cpp), the BVH builder (bvh.cpp) and the output
// writers (image_io.cpp).
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

#include <hip/hip_runtime_api.h>

#include "../../include/rt_api.h"
#include "../../include/rt_temporal.h"
#include "../../include/rt_variance.h"
#include "../../include/rt_clip.h"
#include "../../include/rt_matte.h"
#include "rt_scene_dev.h"

namespace rtgo {

void set_error(const std::string& msg);

// Device memory through a per-device cache of freed blocks (dev_pool.cpp):
// hipMalloc / hipFree semantics (hipError_t as int), the block must no longer
// be in use by any stream when it is freed.
int dev_alloc(void** p, size_t n);
void dev_free(void* p);
// pinned host staging buffers, cached per process (dev_pool.cpp)
int host_alloc(void** p, size_t n, bool* fresh = nullptr);  // fresh: newly pinned (not from the cache)
void host_free(void* p);
// non-blocking streams and timing events, reused the same way (current device)
int dev_stream_get(hipStream_t* s);
void dev_stream_put(hipStream_t s);
int dev_event_get(hipEvent_t* e);
void dev_event_put(hipEvent_t e);

// ---------------------------------------------------------------- scene
struct FlatScene {
  std::vector<DSphere> spheres;
  std::vector<DTri> tris;
  std::vector<DBox> boxes;    // one per cube, over its 12 triangles
  std::vector<DMat> mats;
  std::vector<DLight> lights;
  std::vector<DBVHNode> bvh;  // empty => linear scan
  int32_t bvh_depth = 0;      // levels of the BVH (root = 1): the traversal stack holds fewer entries
  std::vector<DQNode> qbvh;   // the BVH with quantized bounds (same node order)
  // the same tree collapsed to groups of 2..4 nodes (bvh.cpp): DQNode slots,
  // groups back to back, breadth-first; the root group's code
  std::vector<DQNode> qbvh4;
  int32_t bvh4_stack = 0;     // the most pending children a 4-wide traversal holds
  int32_t bvh4_root = 0;
  double q0[3] = {0, 0, 0}, qd[3] = {1, 1, 1};  // its grid: coordinate = q0 + q * qd
  double cam_pos[3] = {0, 0, 0};
  double aspect = 0;
  rt_camera camera{};         // the scene's camera as given (the look-at model reads all of it)
  int32_t objects = 0;        // len(hittables)
};

// The viewport frame of a launch's camera rays (rt_camera_frame,
// include/rt_api.h): ray(u, v) = ((ll + h * u) + v * v) - o per component.
// model RT_CAMERA_REFERENCE: h = (2 * aspect, 0, 0), v = (0, 2, 0) and the
// kernels evaluate getRay's own expressions (renderer.go:377-390).
struct CamFrame {
  double o[3], ll[3], h[3], v[3];
  int32_t model, _pad;
};
// Fills out->o .. out->v and out->model; RT_E_INVALID (message set) for an
// unknown model or a degenerate look-at camera.
int camera_frame(const rt_camera& cam, int32_t model, int32_t w, int32_t h, CamFrame* out);

// The AtmosphereConfig presets of RT_SKY_DEFAULT .. RT_SKY_NIGHT
// (internal/atmosphere/atmosphere.go:28-98), index sky - 1.
constexpr int kSkies = 4;
void sky_presets(DSky out[kSkies]);

// GetHittables + createCube + material constructors (scene.go:59-190).
void flatten_scene(const rt_scene& s, FlatScene* out);
// Shadow-cone rows (scene_flat.cpp; rt_scene_cone_rows, include/rt_api.h):
// rows[light * fs.objects + hittable], bit b clear when sphere b (its index in
// fs.spheres) can never be a shadow-cone candidate of a hit on that hittable
// under that light.  Full rows (~0) without shadow-cone masks (cone_masks_apply:
// a tree, or more than 64 spheres or triangles), for cubes and non-finite scenes.
bool cone_masks_apply(const FlatScene& fs);
// The extent E those rows' margins are derived for (centres + radii, lights,
// the scene's camera): a camera ray from farther out than the proof allows
// (cone_rows_hold) must not use the rows.
double cone_extent(const FlatScene& fs);
// Do the rows hold for camera rays that start at `origin`?  The hit point's
// error bound 2e-7 E (scene_flat.cpp) covers sqrt(1e-15) |o - c| for every
// |o| <= 2 E: |o - c| <= 3 E gives 9.5e-8 E.
bool cone_rows_hold(const FlatScene& fs, const double origin[3]);
void cone_rows(const FlatScene& fs, std::vector<unsigned long long>* rows);
// Binned-SAH BVH over out->spheres and out->boxes, a cube being one primitive
// (reorders both arrays; the triangles stay).  Leaves hold one kind.
// bins / leaf: SAH bins per axis and spheres per leaf at most (0: defaults);
// cubes per leaf is a constant of bvh.cpp.
// Leaves fs->bvh empty (the linear scan) when !spheres_finite(*fs).
void build_bvh(FlatScene* fs, int bins, int leaf);
// The same (its name from when the tree held spheres alone): without cubes
// the tree is node for node what it always was.
void build_sphere_bvh(FlatScene* fs, int bins, int leaf);
// The tree has a leaf of cubes.
bool bvh_has_cubes(const FlatScene& fs);
// Every sphere's centre and radius is finite (a BVH can hold it).
bool spheres_finite(const FlatScene& fs);
// The global tiles a rank renders, in local-tile order (local tile lt is
// tiles[lt]): t % world == rank (strided, createRenderTasks order dealt
// round-robin) or a partition's list (rt_partition, rt_multi.cpp).
void strided_tiles(int32_t W, int32_t H, int32_t rank, int32_t world, std::vector<int32_t>* tiles);
// Per local tile: primitives whose projected bounds overlap it (the work
// estimate of a schedule without a pilot render).
void tile_cost(const FlatScene& fs, const CamFrame& cf, int32_t W, int32_t H, const std::vector<int32_t>& tiles,
               std::vector<float>* local_cost);
// (the reference camera of fs.camera: the schedule inputs as they were before the frame)
void tile_cost(const FlatScene& fs, int32_t W, int32_t H, const std::vector<int32_t>& tiles,
               std::vector<float>* local_cost);
constexpr int32_t kBlockBlack = 1;  // block flag (8th int): black tile, nothing to trace
constexpr int kBlockInts = 16;      // ints per work block record (KParams::blocks)
// Primary-ray candidate masks per local tile (2 x u64: spheres, triangles;
// scenes with <= 64 of each): bit i set unless primitive i's bounding sphere
// provably misses the cone of the tile's camera rays.
void tile_primary_masks(const FlatScene& fs, const CamFrame& cf, int32_t W, int32_t H,
                        const std::vector<int32_t>& tiles, std::vector<unsigned long long>* masks);
void tile_primary_masks(const FlatScene& fs, int32_t W, int32_t H, const std::vector<int32_t>& tiles,
                        std::vector<unsigned long long>* masks);

// The GPU work scheduler (rt_schedule.hip).
struct SchedParams {
  const DSphere* spheres;
  const DTri* tris;
  CamFrame cf;                 // the camera rays' frame (getRay, renderer.go:377-390, or the look-at model)
  int32_t W, H, rank, world, tiles_x, ntiles, local;
  int32_t spp, big_pixels, frustum;
  int32_t split_samples;       // samples per sub-block of a split pixel (<= 64: one path per lane)
  double block_work;
  const unsigned long long* tile_masks;  // per local tile (2 u64) or null (no primary culling)
  const float* tile_cost;      // per local tile: projected primitives (estimate without a pilot)
  const int32_t* tile_list;    // per local tile: its global tile (a partition), or null: rank + lt * world
  const unsigned int* work_max;  // measured per local pixel: the longest path (bounces + 1) ...
  const unsigned int* work_sum;  // ... and the sum over the measured samples, or null (no measurement)
  int32_t work_n;              // samples measured per pixel (1..16: a pilot; spp: a whole frame)
  int32_t work_mean;           // 1: work_n < spp samples of every pixel measured: use their mean (partitions)
  int32_t split_depth;         // a pixel whose longest path has this many bounces is split (measured frames)
  // scratch (sched_layout)
  unsigned long long* pixmask; // per local pixel: 2 u64
  float* est;                  // per local pixel: estimated work of one sample
  int32_t* pilot_blocks;       // 16 records per local tile: the pilot's 64-pixel blocks
  int32_t* hist;               // per weight class: blocks (pass 1)
  int32_t* cursor;             // per weight class: next record (pass 2)
  int32_t* totals;             // [0] blocks, [1] split pixels, [2] split-slot cursor
  int32_t* blocks;             // the records, heaviest class first (pass 2)
  // the live-pixel list of the streamed launches (sched_launch_live)
  int32_t* live_hist;          // per weight class: live pixels
  int32_t* live_cursor;        // per weight class: next list position
  int32_t* live;               // the list, heaviest class first, 4 ints each: {x, y, y * W + x (u32), lt * 1024 + pixel}
  int32_t* live_pos;           // per local pixel: its list position, -1: not live
  // an adaptive progression's add: per local pixel, nonzero while it is active, or null.
  // A stopped pixel gets empty primary masks, so it is in no block's live bits and not in the live list.
  const uint32_t* active;
  // 1: the schedule has no primary culling of its own (rt_tuning.frustum = 0, or a scene without
  // candidate masks): tile_masks then hold every primitive for every tile and a pixel's masks are its
  // tile's, untested, so that they only carry the active flags
  int32_t own_masks;
};
size_t sched_scratch_bytes(int local);
void sched_layout(void* scratch, int local, SchedParams* p);
// masks + pilot blocks (zeroes the class counters first)
int sched_launch_pixels(const SchedParams& p, void* stream);
// The same for a camera sequence: a pixel's masks are the OR
// over the ncams cameras of its masks under camera k -- d_cams[k] within
// d_cam_masks[(k * p.local + lt) * 2 ..], camera k's own tile masks -- so the
// live-pixel list built from them is the union of the cameras' live pixels.
// p.tile_masks: the OR of the cameras' tile masks (black tiles, the pilot).
// A kernel of its own: the schedulers of every other render keep their code.
int sched_launch_pixels_seq(const SchedParams& p, const CamFrame* d_cams, int ncams,
                            const unsigned long long* d_cam_masks, void* stream);
// write = false: estimates, pass 1 (class counts, split count), scan;
// write = true: pass 2 (the records)
int sched_launch_blocks(const SchedParams& p, bool write, void* stream);
// The live pixels of the rank's tiles (image pixels whose primary masks are
// not empty; every image pixel without primary culling), after the estimates
// of sched_launch_blocks(write = false).  write = false: counts per weight
// class, scan, totals[3] = live pixels; write = true: live and live_pos.
int sched_launch_live(const SchedParams& p, bool write, void* stream);

// ---------------------------------------------------------------- kernels
// PCG jump-ahead entries: cooperative soft shadows evaluate up to 64
// rejection tries (3 draws each) per round and then advance by 3*used
// draws; entry h holds (A_3h, C_3h), h = 0..64 (draws 3h+1, 3h+2 are plain
// steps from 3h).
constexpr int kJump = 64 + 1;
// Largest block (pixels x spp) a workgroup renders (its hit list and
// radiance slots live in LDS: 24 KB); the host picks P = floor(1024 / spp)
// pixels per block (at most 64), so spp <= 1024.
constexpr int kMaxBlockSamples = 1024;
constexpr int kMaxFrames = RT_MAX_FRAMES;  // frames per launch at most (rt_context_render_frames_async)
constexpr int kDbgStride = 48;  // RT_WG_TIMING: 64-bit words per workgroup in the debug buffer
// Counters of the counting variants: the nine of rt_counts, then the same
// nine for the work the counting variant walks only to report the
// reference's counts (camera samples of culled pixels, rt_counts.culled),
// then the soft-shadow traversal kernel's share (rt_counts.soft_occlusion).
constexpr int kCounters = 9;
constexpr int kCountSlots = 5 * kCounters;
// count groups after the totals (rt_counts): culled, then the wavefront
// kernels' own shares -- soft-shadow stage, closest hit, hard occlusion
constexpr int kGroupSoft = 2, kGroupExtend = 3, kGroupHard = 4;
// Deepest BVH the kernels accept (per-lane LDS stack entries; bvh.cpp keeps
// the linear scan for deeper trees).  The stacks are allocated per launch for
// the scene's actual depth (10k spheres: 15 levels).
constexpr int kStack = 40;
// A leaf of cubes (bvh.cpp): this bit of DBVHNode.left_or_first, the rest of
// it the first DBox of the leaf; kCubeCode is the same bit in a traversal
// code (first << 3 | count).  Sphere leaves and internal nodes never set it.
constexpr int kCubeLeafBit = 1 << 27;
constexpr int kCubeCode = kCubeLeafBit << 3;
// Cubes per leaf at most: each is a box test and up to 12 triangle tests
// (rt_tuning.bvh_leaf stays the spheres per leaf).
constexpr int kBvhCubeLeaf = 2;
// rt_context_set_scene, force_bvh == 0: a scene of at most 64 spheres gets a
// tree once it has more cubes than this.  Cubes-only grids at 640x480x16,
// linear scan / tree on the wavefront path (scripts/mixed_bvh_ab.py sweep,
// profiles/mixed_bvh_ab.txt): 8 cubes 5.1 / 19.4 ms, 16: 14.3 / 19.7, 32: 9.9 /
// 20.1, 64: 17.3 / 20.5, 128: 31.8 / 21.0 -- 64 is the largest count at which
// the scan still wins.
constexpr int kAutoBvhCubes = 64;

// ---- tail helpers: a launch's long paths handed to idle waves
// When a block's wave has started every entry of its hit list and only a
// few paths are left (at most tail_kmax, each at least tail_dmin bounces
// deep), it EXPORTS them: each path's state goes to a queue, and one of
// tail_helpers extra one-wave workgroups at the end of the grid runs it to
// its end with the whole wave (solo_path: ~5 us per bounce against ~9-17
// us for a few paths sharing a wave).  Its radiance goes to a per-sample row
// of its pixel (the block's own pixels: a dynamic row; split pixels: the
// split row), and the last contributor of a pixel -- the block or a helper --
// sums the row in sample order and writes the pixel, so the image is the
// same bit for bit.  Main blocks never wait for a helper; helpers leave when
// every main block is done and the queue is empty, so the launch always
// drains.
constexpr int kTailShards = 64;
// Every word that many waves touch sits on a 128-B line of its own
// (`unsigned int x[32]`, word 0 used): polling helpers and draining blocks
// on one shared line made each of their accesses wait on the others
// (measured: a draining block's iteration 2.4x slower, an export 45 us).
struct TailCtl {
  unsigned int tail[32];          // queue entries reserved (exporters add; helpers read)
  unsigned int head[32];          // queue entries taken by helpers (CAS)
  // the export gate, one 64-bit word: helpers started and not yet gone (high
  // half) | exported paths not yet finished (low half); an exporter reads it
  // (one load), then reserves with one add whose returned value decides
  unsigned long long gate[16];
  unsigned int rows_used[32];     // dynamic rows allocated
  unsigned int helpers_gone[32];  // helpers finished (the last one zeroes the block for the next launch)
  // statistics since the layout (ticks: s_memrealtime, 100 MHz): paths
  // exported, helpers' time running paths, exporting waves' time in the
  // export, helper lifetimes, paths run; the error word (never expected)
  unsigned int exported, solo_ticks, export_ticks, helper_ticks, paths_done, err, pad[26];
  // main workgroups finished, sharded (block b adds to shard b % kTailShards,
  // 128 B apart): one counter took every block's add and serialized them
  unsigned int done[kTailShards * 32];
};
// one exported path (its state after `depth` bounces, renderer.go:165-227)
struct TailPath {
  double o[3], d[3], T[3], L[3];
  uint64_t rng, skey;
  int32_t depth, sample;   // bounces so far; its sample within the destination row
  int32_t kind, row;       // kTailRow: dynamic row `row`; kTailSplit: split slot index `row`
  int32_t nsub, frame;     // split pixel: its sub-blocks; the frame of the launch
  int64_t oi;              // output pixel index (layout-resolved, as the epilogue writes it)
};
// the header of a dynamic row: its pixel's running sum over the samples
// before k0 (summed by the block), and who still owes a sample
struct TailRow {
  double prefix[3];
  int32_t counter;         // contributors still to finish: the block (1) + its exported paths
  int32_t k0;              // first sample held by the row
  int32_t frame, _pad;
  int64_t oi;
};
constexpr int kTailRow = 1, kTailSplit = 2;

struct KParams {
  const DSphere* spheres;
  const DTri* tris;
  const DBox* boxes;
  const DMat* mats;
  const DLight* lights;
  const DBVHNode* bvh;
  const uint64_t* jump;        // PCG jump table: (A_3h, C_3h) for h = 0..kJump-1 (rt_rng.h)
  float* out_linear;
  uint8_t* out_rgba;
  unsigned long long* counts;  // kCounters counters (rt_counts order, then the culled ones) or null
  unsigned long long* dbg;     // per-WG timing records (RT_WG_TIMING builds only) or null
  const int32_t* blocks;       // per block, kBlockInts ints: {local tile, first pixel, pixel count, first sample,
                               //   samples, split slot (-1: none), sub-blocks of the split pixel, flags,
                               //   primary masks (spheres u64, tris u64), live pixels u64, 0, 0}
  double* split_rad;           // split pixels: [slot][spp][3] radiance of the hit samples
  uint32_t* split_hits;        // split pixels: [slot][(spp+31)/32] hit-sample bits (zeroed per launch)
  int32_t* split_cnt;          // split pixels: sub-blocks finished (zeroed per launch)
  unsigned int* work_max;      // measuring renders: per local pixel, its longest path (bounces + 1) ...
  unsigned int* work_sum;      // ... and the bounces + 1 of all its samples' paths (else null)
  const unsigned long long* tile_masks;  // per local tile: primary-ray candidate masks (spheres, tris) or null
  const DSky* sky;             // miss radiance (rt_settings.sky) or null: black (renderer.go:170-173)
  const void* stage_src;       // start of the scene prefix staged into LDS (spheres..lights)
  int32_t stage_bytes;         // bytes to stage (multiple of 16); 0 = read the scene from global memory
  int32_t stack_off;           // byte offset of the BVH stacks in dynamic LDS
  int32_t stack_depth;         // entries per lane of a BVH stack (the tree's depth)
  CamFrame cf;               // the camera rays' frame (rt_camera_frame)
  uint64_t seed_key;
  int32_t ns, nt, nl, use_bvh, nb;
  int32_t W, H;
  int32_t spp, max_depth;
  int32_t recursive, soft;
  int32_t rank, world;
  int32_t tiles_x, ntiles;
  int32_t num_blocks;        // this rank's blocks (one workgroup each)
  int32_t layout;     // RT_LAYOUT_*
  int32_t num_wgs;         // = num_blocks * nframes
  // sample passes (more samples per pixel than a block holds, DESIGN.md
  // §4.1): this launch renders samples [sample_base, sample_base + spp) of
  // spp_total; acc holds each local pixel's running sum (lt * 1024 + pixel,
  // 3 doubles) between passes.  acc_mode: bit 0 = start from acc (not the
  // first pass), bit 1 = store the sum to acc instead of writing the image
  // (not the last pass).  Single pass: acc_mode 0, spp_total = spp.
  // Bit 2 (a progression's add): store the sum to acc AND
  // write the image, the mean over spp_total = samples done + this add's.
  double* acc;
  int32_t sample_base, spp_total, acc_mode;
  // FRAMES of one launch (rt_context_render_frames_async): the same schedule
  // rendered nframes times, each frame with its own seed and outputs.
  // Workgroup g renders block g / nframes of frame g % nframes, so every
  // frame's heaviest blocks start first and one launch's tail covers all
  // its frames.  launch_render fills entry 0 from seed_key / out_linear /
  // out_rgba when nframes <= 1.  Split pixels: a copy of the split rows and
  // flags per frame, nsplit slots each (split_frames copies in memory).
  int32_t nframes, nsplit, split_frames, _fpad;
  uint64_t frame_key[kMaxFrames];
  float* frame_lin[kMaxFrames];
  uint8_t* frame_rgba[kMaxFrames];
  // tail helpers (null tail: off): the control block, the queue and its
  // ready flags (== tail_epoch when written), the dynamic rows ([row][spp][3]
  // radiance, [row][(spp+31)/32] hit bits, headers); tail_cap entries and rows
  TailCtl* tail;
  TailPath* tail_q;
  unsigned int* tail_ready;
  double* tail_rows;
  uint32_t* tail_bits;
  TailRow* tail_hdr;
  int32_t tail_cap, tail_helpers, tail_kmax, tail_dmin;
  uint32_t tail_epoch;
  int32_t tail_every_mask;  // the drain's iterations between export checks - 1 (a power of 2 - 1)
  int32_t tail_pos;         // the helpers are workgroups [tail_pos, tail_pos + tail_helpers) of the grid
  // shadow-cone rows of a scene of spheres alone (cone_rows: [light][sphere]):
  // their byte offset in the staged prefix (after the lights), 0: none.  Read
  // by the spheres-only stream kernels.  (In the struct's former tail padding:
  // StreamKArgs places StreamParams behind KParams, and no offset of either moves.)
  int32_t cone_rows_off;
};

// ---- streamed launches: the samples of the live pixels of
// `frames` frames form one queue of ENTRIES that a fixed set of persistent
// one-wave workgroups drains (render_stream_kernel); each path's radiance
// goes to its row, and resolve_rows_kernel sums a pixel's rows in sample
// order and writes it.  Entry e -> (frame fl, live pixel i, sample s):
//   order 0: e = (fl * nlive + i) * spp + s   (a chunk: neighbouring samples of one pixel)
//   order 1: e = (i * spp + s) * frames + fl  (the frames interleaved)
// Row of (fl, i, s): (fl * spp + s) * nlive + i, so the resolve's lanes (one
// per live pixel) read consecutive rows.
//
// The decode e -> (fl, i, s) divides twice by launch constants: e by d0, the
// quotient by d1 (order 0: d0 = spp, d1 = nlive; order 1: d0 = frames,
// d1 = spp).  The host finds, per divisor d, l = ceil(log2 d) and
// m = ceil(2^(31 + l) / d) (stream_div_of); m fits 32 bits (d > 2^(l-1) gives
// m <= 2^32 - 1 for l <= 31, and d = 1 gives 2^31), and
//   2^(31 + l) <= m d < 2^(31 + l) + d <= 2^(31 + l) + 2^l,
// which is the condition under which floor(m n / 2^(31 + l)) = floor(n / d)
// for EVERY n < 2^31 (Granlund & Montgomery 1994, theorem 4.2 with N = 31):
// the launch's bound on e, and a quotient is no larger.  The kernel forms it
// as the high word of (2 n) m, shifted right by l: n < 2^31 keeps 2 n in 32
// bits.  One function for the kernel, the host and the CPU test
// (rt_stream_decode, include/rt_api.h).
#if defined(__HIPCC__)
#define RT_HOST_DEVICE __host__ __device__
#else
#define RT_HOST_DEVICE
#endif
struct StreamDiv {
  uint32_t d, m, l, _pad;
};
struct StreamDecode {
  StreamDiv d0, d1;
};
struct StreamEntry {
  uint32_t fl, i, s;  // the launch's frame, the live pixel, the sample
};
inline StreamDiv stream_div_of(uint32_t d) {  // 1 <= d < 2^31
  StreamDiv r{d, 0, 0, 0};
  while ((1ull << r.l) < d) ++r.l;
  r.m = (uint32_t)(((1ull << (31 + r.l)) + d - 1) / d);
  return r;
}
inline StreamDecode stream_decode_of(int32_t order, uint32_t frames, uint32_t nlive, uint32_t spp) {
  // (an empty launch -- no live pixel -- has no entry to decode: any divisor does)
  const uint32_t a = order == 0 ? spp : frames, b = order == 0 ? nlive : spp;
  return StreamDecode{stream_div_of(a ? a : 1u), stream_div_of(b ? b : 1u)};
}
// (Div, Decode: StreamDiv, StreamDecode in whatever address space the caller holds them)
template <class Div>
RT_HOST_DEVICE inline uint32_t stream_div(uint32_t n, const Div& k) {  // n / k.d, n < 2^31
  return (uint32_t)(((uint64_t)(n << 1) * k.m) >> 32) >> k.l;
}
template <class Decode>
RT_HOST_DEVICE inline StreamEntry stream_decode(const Decode& k, int32_t order, uint32_t e) {
  const uint32_t t = stream_div(e, k.d0), r0 = e - t * k.d0.d;
  const uint32_t q = stream_div(t, k.d1), r1 = t - q * k.d1.d;
  return order == 0 ? StreamEntry{q, r1, r0} : StreamEntry{r0, q, r1};
}
// A screen in front of the exact test of a SOFT shadow ray (DESIGN.md §4.7,
// "Soft rays decided without normalising them").  Only the occlusion boolean
// of such a ray is used, and in real arithmetic Sphere.Hit's boolean does not
// depend on the direction's length: with u the unnormalised direction, il an
// approximation of 1 / |u|, oc = P - c, h = (oc.u) il, cc = |oc|^2 - r^2, the
// ray P + t u/|u| meets the sphere where g(t) = t^2 + 2 h t + cc = 0, and
// g(t) = (t + h)^2 - D with D = h^2 - cc.  Each test below is "surely ...":
// it carries a margin over the magnitudes of its terms -- eps on those that
// il's error moves (|il |u| - 1| <= kSoftScreenIl), eps2 on |oc|^2 + r^2,
// which only rounding moves -- at least 16 times what il and the screen's own
// roundings can add up to and thousands of times the reference's roundings
// (the proof is in DESIGN.md), so a sure answer is the boolean Sphere.Hit
// (sphere.go:22-40) returns on the reference's normalised ray; anything else
// -- a grazing ray, a root near tmin or tmax, NaN, infinity (every comparison
// with one is false) -- is undecided and the caller runs the exact test.  The
// operations are explicit fused multiply-adds: the same bits on the host and
// in the kernel (rt_soft_screen, include/rt_api.h, runs this function).
constexpr int kSoftScreenBits = 17;      // eps = 2^-17 >= 16 (2 kSoftScreenIl + 12 * 2^-53): the terms il's error moves (h^2: twice)
constexpr int kSoftScreenBits2 = 16;     // eps2 = eps 2^-16 = 2^-33 >= 2^16 * 14 * 2^-53: the terms only rounding moves
constexpr double kSoftScreenIl = 2e-7;   // il from v_rsq_f32 of the binary32-rounded |u|^2 (1 ulp), |u|^2 in [0.81, 1.21]
enum SoftScreen { kSoftUndecided = 0, kSoftMiss = 1, kSoftHit = 2 };
// x / eps, exact (a test reads `x / eps > magnitudes`: the shift is an inline
// operand of v_ldexp_f64, where eps as a factor would hold a register pair)
RT_HOST_DEVICE inline double soft_scaled(double x) { return __builtin_ldexp(x, kSoftScreenBits); }
RT_HOST_DEVICE inline int soft_screen(double cx, double cy, double cz, double r2, double px, double py, double pz,
                                      double ux, double uy, double uz, double il, double tmin, double tmax) {
  // the guards.  Of the interval (the same for every candidate of a ray): not
  // empty, tmin far above the underflow range; of the magnitudes: with
  // tmax < 2^500 and |oc|^2 + r^2 < 2^1000 nothing overflows, here or in the
  // reference.  A NaN fails them or every comparison below.
  if (!(tmin >= 0x1p-40 && tmin <= tmax && tmax < 0x1p500)) return kSoftUndecided;
  const double ocx = px - cx, ocy = py - cy, ocz = pz - cz;
  const double o2 = __builtin_fma(ocz, ocz, __builtin_fma(ocy, ocy, ocx * ocx));
  const double h = __builtin_fma(ocz, uz, __builtin_fma(ocy, uy, ocx * ux)) * il;
  const double cc = o2 - r2, q = o2 + __builtin_fabs(r2);
  if (!(q < 0x1p1000)) return kSoftUndecided;
  // (cc cancels when P is on the sphere, so the margins carry q -- at eps2: il does not touch cc)
  const double q2 = __builtin_ldexp(q, -kSoftScreenBits2);
  const double D = soft_scaled(__builtin_fma(h, h, -cc)), mD = __builtin_fma(h, h, q2);
  if (-D > mD) return kSoftMiss;  // no real root, and the reference's discriminant is negative too
  const double ah = __builtin_fabs(h);
  const double g0 = soft_scaled(__builtin_fma(tmin, __builtin_fma(2.0, h, tmin), cc));
  const double m0 = __builtin_fma(tmin, __builtin_fma(2.0, ah, tmin), q2);
  const double g1 = soft_scaled(__builtin_fma(tmax, __builtin_fma(2.0, h, tmax), cc));
  const double m1 = __builtin_fma(tmax, __builtin_fma(2.0, ah, tmax), q2);
  const bool p0 = g0 > m0, n0 = -g0 > m0, p1 = g1 > m1, n1 = -g1 > m1;
  if ((p0 && n1) || (n0 && p1)) return kSoftHit;  // exactly one root inside: Hit takes the first root in range, else the second
  if (n0 && n1) return kSoftMiss;                 // the interval lies between the roots
  if (p0 && p1) {
    // t + h: t's side of the vertex -h
    const double v0 = soft_scaled(tmin + h), v1 = soft_scaled(tmax + h), w0 = tmin + ah, w1 = tmax + ah;
    if (v0 > w0 || -v1 > w1) return kSoftMiss;            // both roots, if any, on one side of the interval
    if (-v0 > w0 && v1 > w1 && D > mD) return kSoftHit;   // both roots inside
  }
  return kSoftUndecided;
}

struct StreamParams {
  const int32_t* live;         // SchedParams::live (4 ints per live pixel)
  const int32_t* live_pos;     // SchedParams::live_pos
  const int32_t* tile_list;    // per local tile: its global tile, or null: rank + lt * world
  double* rows;                // [row][3] radiance
  unsigned int* cursor;        // first entry not claimed yet (zeroed before the launch)
  uint32_t total;              // entries: frames * nlive * spp (< 2^31)
  int32_t nlive, npix;         // live pixels; local pixels (local tiles * 1024)
  int32_t frame0, frames;      // the launch's frames [frame0, frame0 + frames) of KParams::frame_*
  int32_t chunk, order;        // entries per claim; the entry order
  // a progression's add: each local pixel's running sum
  // (KParams::acc layout), which the resolve continues and stores back; null: from +0
  double* acc;
  // a camera sequence: the CamFrame of each frame of KParams::frame_* (device memory,
  // kMaxFrames rows; 32 of them do not fit the 4-KB argument block beside KParams), which frame fl of the
  // launch shoots from instead of KParams::cf; null: every frame shoots from KParams::cf.  Last, so that
  // no offset of the kernels' argument moves.
  const CamFrame* cams;
  // the entry decode's divisors and magic numbers (stream_decode_of, per group:
  // `frames` is the group's); behind cams for the same reason
  StreamDecode dec;
};
struct StreamKArgs {           // the kernels' one argument: KParams at offset 0 (rt_blocks.h fresh())
  KParams k;
  StreamParams s;
};
// The launch's stream kernel (stream_kernel_of: generic or spheres-only, each
// with its sample_base twin and its camera-sequence build, sp.cams) on `wgs`
// one-wave workgroups, then resolve_rows_kernel; the cursor is zeroed first.
int launch_stream(const KParams& p, const StreamParams& sp, int wgs, void* stream);
constexpr int kStreamKernels = 6;
int stream_kernel_of(const KParams& p, bool cams = false);
// Writes the n CamFrames (passed by value, in the launch's arguments: no host
// buffer outlives the call) to d_cams on the stream.
struct CamTable {
  CamFrame f[kMaxFrames];
};
int launch_cam_upload(const CamTable& t, int n, CamFrame* d_cams, void* stream);
// resident one-wave workgroups of stream kernel `kernel` with `shmem` bytes of
// dynamic LDS on `device` (the runtime's occupancy x CUs; 0: no answer)
int stream_wave_slots(int device, int kernel, size_t shmem);

// Enqueue the render kernel; returns hipError_t as int.
int launch_render(const KParams& p, bool count, void* stream);
size_t render_shmem(const KParams& p);
// a launch of one frame: frame entry 0 from the single-frame fields (launch_render, launch_stream)
void single_frame_entry(KParams& p);
// device -> mapped pinned host memory by a kernel (16-byte aligned, a multiple of 16 bytes)
int launch_download(const void* d_src, void* h_dst_mapped, size_t bytes, void* stream);
// one workgroup that sleeps for `ms` of device time, then exits (the
// renderer watchdog's test hook, rt_multi.cpp test_stall)
int launch_spin(double ms, void* stream);
// rt_partition_balanced measuring only the first measure_spp samples of every
// pixel (rt_partition.cpp measured_tile_work; the renderer's partitions: 16)
int partition_balanced(rt_context* c, int32_t w, int32_t h, const rt_settings* st, int32_t world, int measure_spp,
                       rt_partition** out);
constexpr int kRendererPartitionSpp = 16;
// d_out[0] = pixels of a, b (RGBA8, npix each) that differ, d_out[1] = the
// largest byte difference; zeroes d_out on the stream first (rt_rgba_delta_async)
int launch_rgba_delta(const uint8_t* d_a, const uint8_t* d_b, size_t npix, uint32_t* d_out, void* stream);
// ---- adaptive progressions
// The per-pixel state of an adaptive progression, one word per local pixel
// (lt * 1024 + pixel) each, and what adaptive_update_kernel needs to apply the
// stop rule (include/rt_adaptive.h) after an add of n samples and to write the
// image of every pixel of the rank's tiles.
struct AdaptParams {
  const double* acc;           // the progression's running sums (KParams::acc layout)
  uint32_t* count;             // samples in the pixel's sum
  uint32_t* streak;            // adds in a row within the tolerance
  uint32_t* active;            // nonzero: still sampled
  uint32_t* rgba;              // its displayed pixel after the last add that rendered it
  unsigned long long* totals;  // [0] += active pixels after this add, [1] += sum of counts (zeroed before)
  const int32_t* tile_list;    // per local tile: its global tile, or null: rank + lt * world
  float* out_linear;           // the add's image (either may be null), laid out by `layout`
  uint8_t* out_rgba;
  int32_t npix, n;             // local pixels (local tiles * 1024); samples this add gave every active pixel
  int32_t W, H, rank, world, tiles_x, ntiles, layout;
  int32_t tolerance, patience, min_samples;
};
int launch_adaptive_update(const AdaptParams& p, void* stream);
// The counts laid out for the caller (rt_context_progressive_counts_async):
// count null: every in-image pixel gets `uniform`.  IMAGE layout: d_out (W*H
// words) is zeroed on the stream first.
int launch_progressive_counts(const AdaptParams& p, uint32_t uniform, uint32_t* d_out, void* stream);
int launch_unpack(int32_t W, int32_t H, int32_t world, const void* gathered, size_t share_bytes, size_t rgba_off,
                  float* ol, uint8_t* orgba, void* stream);
// The same for a partition: slot[t] = {owner rank, local tile} of global tile t;
// nframes frames gathered as [world][nframes][share] into [nframes][W*H] images.
int launch_unpack_map(int32_t W, int32_t H, int32_t nframes, const int32_t* slot, const void* gathered,
                      size_t share_bytes, size_t rgba_off, float* ol, uint8_t* orgba, void* stream);
// Per global tile of a frame, the sum of its pixels' estimated work (rt_schedule.hip
// sched_est of a whole-frame pilot): the input of a balanced partition.
int sched_launch_tile_work(const SchedParams& p, float* tile_work, void* stream);

// The geometry an occlusion / closest-hit query needs (device pointers).
struct Geo {
  const DSphere* spheres;
  const DTri* tris;
  const DBox* boxes;  // one per cube: its 12 consecutive triangles
  const DBVHNode* bvh;
  int32_t ns, nt, use_bvh, nb;
};

// ---- first-hit feature buffers (rt_aov.hip; rt_context_render_aov_async)
// One lane per pixel of the W x H frame, image layout; every output may be null.
struct AovParams {
  Geo g;                       // use_bvh as KParams: 0 linear scan, 1 a tree of spheres, 2 a tree with leaves of cubes
  const DMat* mats;
  CamFrame cf;                 // the camera rays' frame (rt_camera_frame)
  uint64_t seed_key;
  int32_t W, H, spp;
  int32_t stack_depth;         // entries per lane of a BVH stack (the tree's depth)
  float* albedo;               // W*H*3
  float* normal;               // W*H*3
  float* depth;                // W*H
  float* coverage;             // W*H
  int32_t* object;             // W*H
};
int launch_aov(const AovParams& p, void* stream);
int preload_aov_kernels();

// ---- specular-through feature buffers (rt_aov.hip; rt_context_render_aov_spec_async)
// The first-hit pass's parameters and the chain's: a material is followed iff
// its kind is metal, shiny or perfectmirror and DMat::roughness (the
// constructors' Min(roughness, 1.0), scene_flat.cpp) <= max_roughness.
struct AovSpecParams {
  AovParams a;
  double max_roughness;        // checked: finite, >= 0
  int32_t max_bounces;         // checked: 0..16
  int32_t pad;
  float* specular;             // W*H
  float* bounces;              // W*H
};
int launch_aov_spec(const AovSpecParams& p, void* stream);
bool material_followed(const rt_material& m, double max_roughness);  // scene_flat.cpp: the same test on the host

// ---- à-trous denoiser (rt_denoise.hip; rt_denoise_async)
// Checked arguments of one call: image layout, device pointers.  The workspace
// holds three 16-byte records per pixel (two colour buffers that ping-pong and
// the guide buffer, include/rt_denoise.h), 256-byte aligned by the launcher.
constexpr size_t kDenoiseRecordBytes = 48;  // per pixel
constexpr size_t kDenoiseAlign = 256;
struct DenoiseParams {
  rt_denoise dn;               // checked (rt_denoise_check)
  int32_t W, H;
  const float* color;          // W*H*3
  const float* normal;         // W*H*3
  const float* depth;          // W*H
  const float* albedo;         // W*H*3, or null: no demodulation (also when dn.demodulate is 0)
  const int32_t* object;       // W*H, or null
  float* out_linear;           // W*H*3 (may be color), or null
  uint8_t* out_rgba;           // W*H*4, or null
  void* workspace;             // at least kDenoiseRecordBytes * W * H + kDenoiseAlign bytes
};
int launch_denoise(const DenoiseParams& p, void* stream);
int preload_denoise_kernels();

// ---- temporal accumulation (rt_temporal.hip; rt_temporal_async)
// Checked arguments of one call: the per-call constants (include/rt_temporal.h),
// both frames' buffers and the outputs, image layout, device pointers.
struct TemporalParams {
  rt_tp_constants c;           // rt_tp_constants_of: parameters, both cameras, W and H
  rt_tp_buffers cur, prev;     // prev is read only when c.has_prev
  float* out_color;            // W*H*3, not prev.color
  float* out_count;            // W*H, not prev.count
  uint8_t* out_rgba;           // W*H*4, or null
};
int launch_temporal(const TemporalParams& p, void* stream);
int preload_temporal_kernels();

// ---- variance-guided denoising (rt_variance.hip; rt_temporal_moments_async, rt_variance_async,
// rt_denoise_var_async).  Checked arguments of one call each, image layout, device pointers.
struct TemporalMomentsParams {
  TemporalParams t;            // rt_temporal_async's arguments
  const float* cur_albedo;     // W*H*3, or null
  const float* prev_moments;   // W*H*2, given exactly when t.c.has_prev
  float* out_moments;          // W*H*2, not prev_moments
};
struct VarianceParams {
  rt_variance vr;              // checked
  int32_t W, H;
  rt_vr_buffers in;            // color, normal, depth; albedo, object, moments + count or null
  float* out_var;              // W*H
};
// The filter's workspace holds two colour records that ping-pong ({e[3], var}, 16 bytes each), the guide
// record (16 bytes) and the id plane (4 bytes) per pixel, 256-byte aligned by the launcher.
constexpr size_t kDenoiseVarRecordBytes = 52;  // per pixel
struct DenoiseVarParams {
  rt_denoise_var dn;           // checked
  int32_t W, H;
  const float* color;          // W*H*3
  const float* normal;         // W*H*3
  const float* depth;          // W*H
  const float* albedo;         // W*H*3, or null: no demodulation (also when dn.demodulate is 0)
  const int32_t* object;       // W*H, or null
  const float* variance;       // W*H
  float* out_linear;           // W*H*3 (may be color), or null
  uint8_t* out_rgba;           // W*H*4, or null
  float* out_variance;         // W*H (may be variance), or null
  void* workspace;             // at least kDenoiseVarRecordBytes * W * H + kDenoiseAlign bytes
};
int launch_temporal_moments(const TemporalMomentsParams& p, void* stream);
int launch_variance(const VarianceParams& p, void* stream);
int launch_denoise_var(const DenoiseVarParams& p, void* stream);
int preload_variance_kernels();

// ---- temporal accumulation with per-object motion (rt_motion.hip; rt_temporal_motion_async)
struct TemporalMotionParams {
  TemporalMomentsParams m;     // out_moments null: the colour-only form (cur_albedo and prev_moments null too)
  const double* motion;        // num_objects * 3, a device pointer
  int32_t num_objects;         // >= 1
};
int launch_temporal_motion(const TemporalMotionParams& p, void* stream);
int preload_motion_kernels();

// ---- temporal accumulation with history rectification (rt_clip.hip; rt_temporal_clip_async)
struct TemporalClipParams {
  TemporalMotionParams mo;     // motion null: no table (m = 0, ids optional); m.cur_albedo may be given without moments
  rt_cl_params clip;           // checked
  float* out_clipped;          // W*H, or null
};
// launch_temporal_clip takes the staged form from this radius on when RTGO_CLIP_FORM does not say (DESIGN.md
// §4.18 has the A/B: at radius 1 the staged form's gain did not clear twice the spread in every case)
constexpr int32_t kClipStagedFromRadius = 2;
int launch_temporal_clip(const TemporalClipParams& p, void* stream);
int preload_clip_kernels();

// ---- matte layers and the edge resolve (rt_matte.hip; rt_context_render_matte_async, rt_matte_resolve_async,
// DESIGN.md §4.19)
struct MatteParams {
  AovParams a;                 // the first-hit pass's rays and scene (aov_setup); its five outputs stay null
  int32_t level;               // checked: RT_MATTE_OBJECT or RT_MATTE_FACE
  int32_t ranks;               // checked: 1..8
  int32_t* id;                 // ranks * W*H, or null
  int32_t* count;              // ranks * W*H, or null
  int32_t* rest;               // W*H, or null
};
struct MatteResolveParams {
  rt_mt_resolve_params r;      // checked (rt_mt_resolve_ok, the size rule)
  const float* color;          // W*H*3
  const int32_t* object;       // W*H
  const int32_t* id;           // K * W*H
  const int32_t* count;        // K * W*H
  const int32_t* rest;         // W*H, or null
  float* out_linear;           // W*H*3, not color; or null
  uint8_t* out_rgba;           // W*H*4, or null
};
int launch_matte(const MatteParams& p, void* stream);
int launch_matte_resolve(const MatteResolveParams& p, void* stream);
int preload_matte_kernels();

// ---------------------------------------------------------------- wavefront path
// (rt_wavefront.hip: BVH scenes)
constexpr int kWfShards = 8;           // queues / path arrays are split in 8 shards (one atomic word each)
constexpr int kWfBlockSlots = 256;     // threads per workgroup of the wavefront kernels
constexpr int kWfTravBlock = 1024;     // ... of the traversal kernels (extend, occlude): one per CU, BVH in LDS
constexpr uint32_t kDeadSid = 0xFFFFFFFFu;  // a slot with no sample (out-of-image pixel of an edge tile)
// soft shadows: candidate spheres kept per shadow cone (more: its rays are
// traced).  Host allocation and kernels must agree: a constant, not a build
// knob (C4: 16 -> 412.6 ms per frame, 24 -> 416.0, 32 -> 421.1; with the
// list tests ordered by length: 16 -> 403.4, 32 -> 405.7)
constexpr int kWfConeK = 16;
// (r05) a cone with kWfConeK < candidates <= kWfConeWide is "wide": its 16 rays
// are tested against its list, one ray per lane (wf_widetest), instead of
// being traced; the candidate lists hold kWfConeWide entries per (path, light)
#ifndef RT_CONE_WIDE
#define RT_CONE_WIDE 32
#endif
constexpr int kWfConeWide = RT_CONE_WIDE;
struct WfCtl {                 // device-resident loop state; counters of shard s at [32 s] (own 128-B line)
  int32_t cur_cnt[kWfShards * 32];   // live paths per shard of the current array
  int32_t next_cnt[kWfShards * 32];  // survivors appended per shard of the next array
  int32_t hard_cnt[kWfShards * 32];  // hard shadow rays queued per shard
  int32_t soft_cnt[kWfShards * 32];  // soft shadow rays queued per shard
  int32_t cone_cnt[kWfShards * 32];  // shadow cones queued per shard
  int32_t list_cnt[kWfShards * 32];  // entries of listed cones per shard (two each, from the far end of the soft queue)
  int32_t wide_cnt[kWfShards * 32];  // entries of wide cones per shard (two each, in the wide queue)
  int32_t job_head[4][kWfShards * 32];  // persistent kernels (extend, hard, soft, cone): jobs taken per range
  unsigned long long next_sample;    // first sample id of the chunk not started yet
  unsigned long long total;          // sample ids in the chunk
  int32_t live;                // live paths after the last bounce (wf_book)
  int32_t dry;                 // every sample started
  int32_t iter;                // bounces done
  int32_t pad;
};
struct WfPaths {             // structure of arrays, kWfShards * shard_cap slots
  double *ox, *oy, *oz, *dx, *dy, *dz;  // ray
  double *tx, *ty, *tz, *lx, *ly, *lz;  // throughput, radiance so far
  uint64_t* rng;             // stream state
  uint32_t* sid;             // sample id within the chunk (local pixel * spp + sample), kDeadSid: none
  int32_t* depth;
};
struct WfParams {
  Geo g;
  const DQNode* qbvh;        // quantized BVH (FlatScene::qbvh) and its grid
  double q0[3], qd[3];
  const DMat* mats;
  const DLight* lights;
  const DSky* sky;           // miss radiance or null (black)
  int32_t nl, max_depth, recursive, soft, spp;
  int32_t W, H, rank, world, tiles_x, ntiles, layout;
  const int32_t* tile_list;  // per local tile: its global tile (a partition), or null: rank + lt * world
  int32_t stack_depth;       // BVH stack entries per lane (the tree's depth - 1)
  int32_t lds_nodes;         // leading quantized nodes (breadth-first: the top levels) staged in LDS
  int32_t bvh_nodes;         // quantized nodes in all
  const DQNode* qbvh4;       // the 4-wide form (FlatScene::qbvh4): wf_occlude4 walks it when use4
  int32_t nodes4, stack4, use4;  // its slots, stack entries per lane; 1: staged whole in LDS and used
  int32_t root4;             // the root group's code
  int32_t trav_block;        // threads per workgroup of the traversal kernels (<= kWfTravBlock)
  int32_t shard_cap;         // path slots per shard
  int32_t live_bound;        // the host's bound on this bounce's live paths (launch sizes only)
  int32_t dry;               // 1: every sample of the chunk has started (no regen work left)
  int64_t hard_cap, soft_cap;  // queue entries per shard
  uint32_t lp0;              // first local pixel of the chunk (local tile * 1024 + pixel in tile)
  CamFrame cf;               // the camera rays' frame (rt_camera_frame)
  uint64_t seed_key;
  WfPaths cur, next;
  WfCtl* ctl;
  int32_t* hidx;             // per slot of the current array: sphere hit (-1: none; kTriHit | triangle, rt_wavefront.hip)
  double *px, *py, *pz;      // hit point
  uint32_t* lstate;          // [slot][light]: kHardBit | blocked soft rays
  uint32_t* hardq;           // kWfShards queues of hard_cap entries: slot * nl + light
  uint32_t* softq;           // kWfShards queues of soft_cap entries, 4 words: {slot * nl + light, draws x, y, z}
                             // (listed cones, from the far end: 2 entries, wf_softgen)
  const uint64_t* jump;      // PCG jump table (KParams::jump)
  int32_t list_tries;        // tries a listed cone's accepted-try mask covers (1..64, rt_tuning.wf_list_tries)
  uint32_t* coneq;           // kWfShards queues of hard_cap entries: slot * nl + light (clear hard ray)
  int32_t* cand;             // [slot * nl + light][kWfConeWide]: the shadow cone's candidate spheres, -1 ends
  uint32_t* wideq;           // kWfShards queues of wide_cap 4-word entries: two per wide cone (as the listed cones')
  int64_t wide_cap;
  double* rad;               // [sample id][3] radiance
  unsigned long long* counts;
  float* out_linear;
  uint8_t* out_rgba;
  // a progression's add: the chunk's sample s of a pixel is
  // the frame's sample sample_base + s; wf_resolve continues the pixel's sum
  // in acc (KParams::acc layout; null: from +0) and divides by spp_total
  double* acc;
  int32_t sample_base, spp_total;
};
// Kernel classes of one bounce (rt_context_profile): prof, when not null,
// holds kWfProfEvents hipEvent_t recorded at their boundaries (event k opens
// class k, event k + 1 closes it; a skipped kernel takes no time).
enum { kWfExtend = 0, kWfShade1, kWfHard, kWfCone, kWfSoftgen, kWfList, kWfSoft, kWfShade, kWfRegen, kWfResolve, kWfClasses };
constexpr int kWfProfEvents = kWfClasses + 1;  // (one block serves any class range)
// active (an adaptive progression's add; null: every pixel
// renders): per local pixel, nonzero while it is active -- the samples of a
// stopped pixel become dead slots (wf_regen_active, a kernel of its own: the
// kernels of a plain frame take WfParams alone, as they were).
int wf_launch_bounce(const WfParams& p, bool first, bool count, void* stream, const void* prof,
                     const uint32_t* active = nullptr);
// Quantized nodes the traversal kernels can stage in LDS next to their stacks
// (all of them when they fit; else an odd count, so no child pair is split).
// Load each kernel file's code object onto the current device (HIP loads
// them lazily, at a file's first launch otherwise): rt_context_create.
int preload_render_kernels();
// An empty launch and a 4-KB copy each way on the stream (dev4k: 4 KB of
// device memory): the runtime's first-launch and first-copy set-up.
int warm_device(void* stream, void* dev_buf, void* host_pinned, void* host_pageable, size_t bytes);
int preload_stream_kernels();
int preload_image_kernels();
int preload_sched_kernels();
int preload_wf_kernels();
// RT_CHECK_XLANE builds: inactive-lane __shfl reads per file (-1: not such a build)
long long xlane_faults_kernel(bool reset);
long long xlane_faults_stream(bool reset);
long long xlane_faults_wavefront(bool reset);
int wf_lds_nodes(int stack_depth, int nodes, int block, int wgs_per_cu);
int wf_launch_resolve(const WfParams& p, int npix, void* stream);

// ---------------------------------------------------------------- partitions
// A tile -> rank assignment (rt_partition, include/rt_api.h): every rank's
// tiles ascending, each tile with its owner and its index in the owner's list
// (its local tile: the slot range [local * 1024, local * 1024 + 1024) of the
// owner's packed share).
struct PartitionData {
  int32_t w = 0, h = 0, world = 1;
  std::vector<int32_t> owner;    // per global tile
  std::vector<int32_t> local;    // per global tile
  std::vector<int32_t> offsets;  // world + 1: rank r's tiles are lists[offsets[r], offsets[r + 1])
  std::vector<int32_t> lists;
  std::vector<double> work;      // per rank: the estimated work of its tiles (balanced partitions), else empty
  int32_t max_local = 0;
  uint64_t id = 0;               // unique per partition object (part of a context's schedule key)
};
// Fills local / offsets / lists / max_local / id from w, h, world, owner.
void finish_partition(PartitionData* d);
// owner and work of a balanced partition of tiles with estimated `work` over
// d->world ranks (longest processing time first), then finish_partition.
void lpt_partition(const std::vector<float>& work, PartitionData* d);
rt_partition* make_partition(PartitionData&& d);
bool context_has_bvh(const rt_context* c);
double context_bvh_seconds(const rt_context* c);
void* context_stream(const rt_context* c);  // its own non-blocking stream (hipStream_t)
// A multi-rank renderer's frame deadline on a context (steady_now_s() clock,
// <= 0: none): the context's host waits during a render (the previous render
// before buffers are reused, the schedule's count read-back, the wavefront
// loop's per-bounce state) poll until it and return RT_E_TIMEOUT after it.
void context_set_deadline(rt_context* c, double deadline);
double steady_now_s();
const PartitionData& partition_data(const rt_partition* p);

// ---------------------------------------------------------------- output
double go_pow_tonemap(double x);  // Pow(x, 1/2.2) with Go's special cases
void tonemap_to_rgba(const double c[3], uint8_t out[4]);

}  // namespace rtgo
