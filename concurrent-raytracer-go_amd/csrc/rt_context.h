// rt_context.h — the context behind the C ABI and the helpers its parts share:
// rt_api.cpp (life cycle, scene, tuning, stats), rt_render.cpp (schedule and
// launches), rt_wavefront_host.cpp, rt_progressive.cpp, rt_partition.cpp.
#pragma once
#include <hip/hip_runtime_api.h>
#include <string.h>

#include <algorithm>
#include <memory>
#include <string>
#include <vector>

#include "../../include/rt_adaptive.h"
#include "../../include/rt_rng.h"
#include "rt_internal.h"

#define HIP_TRY(expr)                                                                   \
  do {                                                                                  \
    hipError_t e_ = (expr);                                                             \
    if (e_ != hipSuccess) {                                                             \
      rtgo::set_error(std::string(#expr) + " failed: " + hipGetErrorString(e_));       \
      return RT_E_DEVICE;                                                               \
    }                                                                                   \
  } while (0)

// A buffer and its capacity in bytes: device memory (grow) or pinned host
// memory (grow_pinned).
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  template <class T>
  T* as() const {
    return (T*)p;
  }
};

struct rt_context {
  int device = 0;
  rt_tuning tun;  // work partition (rt_context_set_tuning); never changes the image
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool have_scene = false;
  rtgo::FlatScene flat;
  // The context's device buffers (DevBuf members only, `scene` first:
  // rt_context_destroy frees [begin, end)).
  struct DevBufs {
    DevBuf scene;   // one allocation: spheres | tris | mats | lights | jump table | bvh
    DevBuf counts;  // kCountSlots counters of a counting render
    DevBuf blocks;  // work blocks, kBlockInts ints each, heaviest first
    DevBuf pilot;   // pilot render scratch: packed float3 + rgba + path lengths (max, sum)
    DevBuf acc;     // sample passes: running per-pixel sums (KParams.acc)
    DevBuf meas;    // a measuring frame's path lengths (max | sum)
    DevBuf split;   // split pixels' per-sample radiance rows + sub-block counters
    DevBuf sched;   // scheduler scratch (sched_layout) + the per-tile inputs
    DevBuf part;    // every rank's tile list of the partition
    DevBuf wf_mem;  // wavefront path (BVH scenes): path arrays + queues,
    DevBuf wf_rad;  //   per-chunk radiance,
    DevBuf wf_ctl;  //   loop control (WfCtl)
    // tail helpers: control block | queue | ready flags | rows
    // | row bits | row headers, laid out for tail_spp samples per pixel
    DevBuf tail;
    // streamed launches: the schedule's live-pixel list
    // (nlive x 4 ints, then live_pos per local pixel), cached with the blocks;
    // the per-sample rows behind the queue cursor word, allocated lazily
    DevBuf live, rows;
    // a progression's own per-pixel running sums (KParams.acc layout; not acc,
    // which ordinary sample passes use)
    DevBuf prog;
    // adaptive sampling: [totals, 256 B][count][streak][active][rgba], one
    // word per local pixel each
    DevBuf adapt;
    // a camera sequence's CamFrames: kMaxFrames rows, the
    // table of the set last rendered (seq_cams)
    DevBuf cams;
    DevBuf* begin() { return &scene; }
    DevBuf* end() { return begin() + sizeof(DevBufs) / sizeof(DevBuf); }
  } d;
  DevBuf h_stage;  // pinned host image of the scene buffer (its upload), made by the constructor
  const rtgo::DSphere* d_spheres = nullptr;
  const rtgo::DTri* d_tris = nullptr;
  const rtgo::DBox* d_boxes = nullptr;
  const rtgo::DMat* d_mats = nullptr;
  const rtgo::DLight* d_lights = nullptr;
  const rtgo::DBVHNode* d_bvh = nullptr;
  const rtgo::DQNode* d_qbvh = nullptr;
  const rtgo::DQNode* d_qbvh4 = nullptr;
  const uint64_t* d_jump = nullptr;
  const rtgo::DSky* d_sky = nullptr;  // the kSkies presets
  hipStream_t last_stream = nullptr;
  bool have_timing = false;
  unsigned long long* dbg = nullptr;
  // the work schedule (rt_schedule.hip), cached per (scene, W, H, rank, world, settings)
  uint64_t scene_gen = 0;
  int64_t order_key[16] = {-1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1, -1};
  int32_t num_blocks = 0;
  int32_t nsplit = 0;        // split pixels of the current schedule
  int32_t split_frames = 0;  // frames whose copies of the split rows are laid out in d.split
  // measured schedule (rt_tuning.measure): 0 none, 1 the next render measures
  // every pixel's paths into d.meas, 2 measured (the next schedule is re-cut
  // from them), 3 done
  int meas_state = 0;
  rt_context_stats stats{};            // rt_context_get_stats
  int32_t h_totals[4] = {0, 0, 0, 0};  // block and split counts of the last schedule (12 bytes read back)
  // pinned staging of the schedule's small copies (the counts read back, the
  // per-tile masks and costs uploaded), made by the constructor
  DevBuf h_small;
  std::vector<unsigned long long> masks_host;  // per local tile primary-ray masks
  unsigned long long* d_masks = nullptr;       // (inside d.sched)
  int32_t stage_bytes = 0;  // scene prefix staged into LDS per workgroup (0 = none)
  int32_t cone_rows_off = 0;  // the staged shadow-cone rows' offset in it (KParams::cone_rows_off; 0 = none)
  rtgo::WfCtl* wf_host = nullptr;  // pinned ring of kWfRing snapshots of d.wf_ctl
  hipEvent_t wf_ev[4] = {nullptr, nullptr, nullptr, nullptr};
  // tile partition (rt_context_set_partition): its data; d.part holds every
  // rank's tile list on this device (null part: strided)
  std::shared_ptr<const rtgo::PartitionData> part;
  double bvh_seconds = 0;  // host time of the last BVH build (rt_stats.bvh_build_seconds)
  // per-kernel device time of the wavefront path (rt_context_profile): an
  // event pool, the blocks of it the last frame recorded ({first event,
  // first class, last class}) and the totals
  bool prof_on = false;
  std::vector<hipEvent_t> prof_pool;
  size_t prof_used = 0;
  struct ProfBlock {
    size_t base;
    int first, last;
  };
  std::vector<ProfBlock> prof_pending;
  double prof_secs[rtgo::kWfClasses] = {0};
  int64_t prof_launches[rtgo::kWfClasses] = {0};
  // a multi-rank renderer's frame deadline (steady_now_s() clock; <= 0:
  // none), set by rt_renderer_render for the frame (context_set_deadline)
  double deadline = 0;
  int32_t tail_cap = 0, tail_spp = -1;  // the layout of d.tail
  uint32_t tail_epoch = 0;
  int32_t nlive = -1, live_local = 0;  // d.live's pixels (nlive < 0: this schedule has none)
  // per stream kernel (stream_kernel_of): its resident waves on this device
  // (its grid) at wave_shmem bytes of dynamic LDS, as the runtime reports them
  int32_t wave_slots[rtgo::kStreamKernels] = {0};
  size_t wave_shmem[rtgo::kStreamKernels] = {0};
  // a progression: its frame (prog_st.samples: the cap) and
  // the samples of every pixel done so far
  bool prog_on = false;
  int32_t prog_w = 0, prog_h = 0, prog_rank = 0, prog_world = 1, prog_layout = 0;
  rt_settings prog_st{};
  int64_t prog_done = 0;
  // adaptive sampling of the progression: the rule, the
  // totals of the last add read back into pinned memory (active pixels, sum
  // of counts), the in-image pixels of the rank's tiles, the adds so far, and
  // the generation of the active set: it grows when an add stopped pixels,
  // and keys the adaptive adds' schedules
  bool adapt_on = false;
  rt_adaptive adapt{};
  DevBuf h_adapt;
  int64_t adapt_inimg = 0, adapt_active = 0, adapt_sum = 0, adapt_gen = 0;
  int64_t prog_adds = 0;
  bool adapt_pending = false;  // an add's totals are on their way to h_adapt
  // camera sequences.  The scene's camera reaches the
  // schedule key through scene_gen; a camera given with a render reaches it
  // through a generation of this counter: a sequence takes a new one when its
  // set of frames differs from the last sequence's (seq_cams, seq_n: the set in
  // d.cams, keyed seq_gen), a frame rendered alone with a camera of its own
  // takes a new one every time (keyed by its negative).  0 keys the scene's view.
  int64_t cam_gen = 0, seq_gen = 0;
  int32_t seq_n = 0;
  rtgo::CamTable seq_cams{};
};

namespace rtgo {

// The context's host waits during a render (rt_api.cpp): blocking, or polling
// until the context's deadline.
int wait_stream(rt_context* c, hipStream_t s);
int wait_event(rt_context* c, hipEvent_t ev);

// What follows is shared between the context's files only: hidden, so the
// library's dynamic symbols stay those of include/rt_api.h and rt_internal.h.
#pragma GCC visibility push(hidden)

// KParams.acc_mode of a progression's add that is one launch (DESIGN.md
// §4.8): start from the sums, keep them, write the image
constexpr int32_t kAccProgressive = 1 | 4;

// A kernel launch (its hipError_t e, as the launch_* functions return it) failed
inline int launch_failed(const char* what, int e) {
  set_error(std::string(what) + " launch failed: " + hipGetErrorString((hipError_t)e));
  return RT_E_DEVICE;
}

// Does a render of (w, h, world) use the context's partition?
inline bool use_partition(const rt_context* c, int w, int h, int world) {
  return c->part && world > 1 && c->part->w == w && c->part->h == h && c->part->world == world;
}
// Tiles of `rank`: the partition's list or the strided set (createRenderTasks's
// tiles t % world == rank)
inline int local_tiles(const rt_context* c, int w, int h, int rank, int world) {
  if (use_partition(c, w, h, world)) return c->part->offsets[rank + 1] - c->part->offsets[rank];
  return rt_tiles_for_rank(w, h, rank, world);
}
inline void host_tiles(const rt_context* c, int w, int h, int rank, int world, std::vector<int32_t>* out) {
  if (use_partition(c, w, h, world)) {
    const PartitionData& d = *c->part;
    out->assign(d.lists.begin() + d.offsets[rank], d.lists.begin() + d.offsets[rank + 1]);
  } else {
    strided_tiles(w, h, rank, world, out);
  }
}
inline const int32_t* dev_tiles(const rt_context* c, int w, int h, int rank, int world) {
  return use_partition(c, w, h, world) ? c->d.part.as<int32_t>() + c->part->offsets[rank] : nullptr;
}

// Wait until the last render enqueued on this context has finished: before
// the host overwrites buffers it reads (scene, schedule, wavefront state).
inline int quiesce(rt_context* c) {
  int rc = c->have_timing ? wait_event(c, c->ev1) : RT_OK;
  if (!rc && c->stream) rc = wait_stream(c, c->stream);
  return rc;
}

// Device buffer b grown to at least n bytes.  dev_free hands the old block
// straight to the device cache (no implicit device sync, unlike hipFree),
// where another context may take it at once: the context's last render, which
// may still use it, is waited for first (always: also before a first
// allocation, as the scene and wavefront buffers ever did).
inline int grow(rt_context* c, DevBuf* b, size_t n, bool always = false) {
  if (n <= b->cap) return RT_OK;
  if (b->p || always) {
    int rc = quiesce(c);
    if (rc) return rc;
  }
  dev_free(b->p);
  *b = DevBuf{};
  HIP_TRY((hipError_t)dev_alloc(&b->p, n));
  b->cap = n;
  return RT_OK;
}
// The same for pinned staging (the caller has synchronized its last copy)
inline int grow_pinned(DevBuf* b, size_t n) {
  if (n <= b->cap) return RT_OK;
  host_free(b->p);
  *b = DevBuf{};
  HIP_TRY((hipError_t)host_alloc(&b->p, n));
  b->cap = n;
  return RT_OK;
}

// A render enters the caller's stream `s`, as given (NULL = the legacy default
// stream): enqueued on another stream than this context's last one it waits
// for that one first (they share the split rows and the wavefront state) ...
inline int enter_stream(rt_context* c, hipStream_t s) {
  if (c->have_timing && s != c->last_stream) HIP_TRY(hipStreamWaitEvent(s, c->ev1, 0));
  return RT_OK;
}
// ... and leaves it: ev1 closes the timed region and is what the next one waits for
inline int leave_stream(rt_context* c, hipStream_t s) {
  HIP_TRY(hipEventRecord(c->ev1, s));
  c->last_stream = s;
  c->have_timing = true;
  return RT_OK;
}

// The launch parameters of a render of (w, h, st) by `rank` of `world`
// (outputs, counters and schedule are filled in by the caller).
// cam: the frame to shoot from instead of the scene's camera (a camera
// sequence's frame rendered alone; validated by its caller).
inline void base_params(const rt_context* c, int w, int h, const rt_settings* st, int rank, int world, int layout,
                        KParams* out, const CamFrame* cam = nullptr) {
  const FlatScene& f = c->flat;
  KParams& p = *out;
  memset(&p, 0, sizeof p);
  p.spheres = c->d_spheres;
  p.tris = c->d_tris;
  p.boxes = c->d_boxes;
  p.mats = c->d_mats;
  p.lights = c->d_lights;
  p.bvh = c->d_bvh;
  p.jump = c->d_jump;
  p.sky = st->sky != RT_SKY_NONE ? c->d_sky + (st->sky - 1) : nullptr;
  p.dbg = c->dbg;
  // (the entry points have validated st and the camera: check_frame)
  if (cam) p.cf = *cam;
  else (void)camera_frame(f.camera, st->camera, w, h, &p.cf);
  p.seed_key = rt_rng_seed_key(st->seed);
  p.ns = (int32_t)f.spheres.size();
  p.nt = (int32_t)f.tris.size();
  p.nl = (int32_t)f.lights.size();
  p.nb = (int32_t)f.boxes.size();
  p.use_bvh = f.bvh.empty() ? 0 : (bvh_has_cubes(f) ? 2 : 1);  // (2: leaves of cubes, launch_render's kMix kernels)
  p.W = w;
  p.H = h;
  p.spp = st->samples;
  p.max_depth = st->max_depth;
  p.recursive = st->recursive_reflections != 0;
  p.soft = st->soft_shadows != 0;
  p.rank = rank;
  p.world = world;
  p.tiles_x = (w + 31) / 32;
  p.ntiles = rt_num_tiles(w, h);
  p.layout = layout;
  // LDS staging of the scene prefix + BVH stack placement
  p.stage_src = c->d.scene.p;
  p.stage_bytes = c->tun.stage ? c->stage_bytes : 0;
  p.cone_rows_off = p.stage_bytes > 0 ? c->cone_rows_off : 0;
  // (the rows' margins are derived for rays from within the scene's extent)
  if (cam && p.cone_rows_off && !cone_rows_hold(f, cam->o)) p.cone_rows_off = 0;
  p.stack_off = (p.stage_bytes + 15) & ~15;
  p.stack_depth = std::max(1, f.bvh_depth);
}

inline bool use_wavefront(const rt_context* c) { return !c->flat.bvh.empty() && c->tun.path != RT_PATH_MEGAKERNEL; }

// ---- rt_api.cpp
// st, the image size and the scene's camera under st's camera model (a
// degenerate look-at camera is RT_E_INVALID): what every planner and render
// entry point checks; check_frame_args: the scene, those, rank/world, layout.
// (check_settings: st and the size alone, for a call that brings its own camera)
int check_settings(const rt_settings* st, int32_t w, int32_t h);
int check_frame(const rt_context* c, int32_t w, int32_t h, const rt_settings* st);
int check_frame_args(const rt_context* c, int32_t w, int32_t h, const rt_settings* st, int32_t rank, int32_t world,
                     int32_t layout);
int prof_collect(rt_context* c);  // adds the recorded profiling blocks to the totals (waits for them)

// ---- rt_render.cpp
int big_block_pixels(int spp, const rt_tuning& tn);
double default_block_work(const rt_context* c, int frames = 1);
bool masks_apply(const FlatScene& f);  // primary-ray candidate masks apply (small linear-scan scenes)
SchedParams sched_params(rt_context* c, const KParams& p, const rt_settings* st, const std::vector<int32_t>& tiles,
                         const int32_t* d_tiles, bool masks, bool frustum, double block_work, int bigP, void* scratch,
                         unsigned long long* d_masks, float* d_cost);
int run_pilot(const rt_context* c, const KParams& p, SchedParams* sp, char* buf, hipStream_t s);
// A render whose camera is not the scene's: the generation
// that keys its schedule (rt_context::cam_gen; 0: the scene's view) and, for a
// sequence, its n frames -- the schedule's pixel masks and live-pixel list
// are then the union over them (the table is in d.cams when it is built).
struct CamKey {
  int64_t gen = 0;
  const CamFrame* frames = nullptr;
  int n = 0;
};
int prepare_schedule(rt_context* c, KParams* p, const rt_settings* st, hipStream_t s, int frames = 1,
                     const uint32_t* active = nullptr, int64_t active_gen = 0, const CamKey& cam = CamKey());
// The sample passes of one frame or of one add of a progression (between
// enter_stream and leave_stream): samples [first, first + n) of spp_total.
struct PassOpts {
  int first = 0, n = 0, spp_total = 0;
  DevBuf* acc = nullptr;  // the running sums between passes
  bool keep = false;      // a progression: the sums continue *acc and the last pass keeps them
  // a single frame's options: the frames per launch of its schedule key, the
  // counting variant, and whether it may be the schedule's measuring frame
  int key_frames = 1;
  rt_counts* counts = nullptr;
  bool may_measure = false;
  // an adaptive add's active flags and their generation (prepare_schedule)
  const uint32_t* active = nullptr;
  int64_t active_gen = 0;
  CamKey cam;  // a frame with a camera of its own (its p.cf is base_params's override)
};
int render_passes(rt_context* c, KParams* p, const rt_settings* st, hipStream_t s, const PassOpts& o);

// ---- rt_wavefront_host.cpp
int render_wavefront(rt_context* c, const KParams& kp, const rt_settings* st, hipStream_t s, bool count,
                     const uint32_t* active = nullptr);

#pragma GCC visibility pop

}  // namespace rtgo
