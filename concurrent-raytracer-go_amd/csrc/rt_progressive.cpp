// rt_progressive.cpp — progressive rendering and its adaptive sampling
// (include/rt_api.h).  The random streams are keyed by
// (seed, pixel, sample), so samples [done, done + n) of a pixel do not depend
// on how many follow; an add renders them and continues the pixel's binary64
// sum in sample order, as the sample passes of a frame of more than
// kMaxBlockSamples do (rt_render.cpp render_passes).
#include "rt_context.h"

using namespace rtgo;

// ---- adaptive sampling
// The in-image pixels of the progression's tiles.
static int64_t prog_image_pixels(const rt_context* c) {
  std::vector<int32_t> tiles;
  host_tiles(c, c->prog_w, c->prog_h, c->prog_rank, c->prog_world, &tiles);
  const int tiles_x = (c->prog_w + 31) / 32, ntiles = rt_num_tiles(c->prog_w, c->prog_h);
  int64_t n = 0;
  for (int32_t t : tiles) {
    if (t < 0 || t >= ntiles) continue;
    const int x0 = (t % tiles_x) * 32, y0 = (t / tiles_x) * 32;
    n += (int64_t)std::max(0, std::min(32, c->prog_w - x0)) * std::max(0, std::min(32, c->prog_h - y0));
  }
  return n;
}

// The state arrays and frame of the progression, as the adaptive kernels take them.
static void adapt_params(const rt_context* c, AdaptParams* a) {
  memset(a, 0, sizeof *a);
  const int w = c->prog_w, h = c->prog_h, rank = c->prog_rank, world = c->prog_world;
  const size_t npx = (size_t)local_tiles(c, w, h, rank, world) * 1024;
  a->acc = c->d.prog.as<const double>();
  if (c->adapt_on) {
    a->totals = c->d.adapt.as<unsigned long long>();
    a->count = (uint32_t*)(c->d.adapt.as<char>() + 256);
    a->streak = a->count + npx;
    a->active = a->streak + npx;
    a->rgba = a->active + npx;
  }
  a->tile_list = dev_tiles(c, w, h, rank, world);
  a->npix = (int32_t)npx;
  a->W = w;
  a->H = h;
  a->rank = rank;
  a->world = world;
  a->tiles_x = (w + 31) / 32;
  a->ntiles = rt_num_tiles(w, h);
  a->layout = c->prog_layout;
  a->tolerance = c->adapt.tolerance;
  a->patience = c->adapt.patience;
  a->min_samples = c->adapt.min_samples;
}

static bool adaptive_ok(const rt_adaptive* a) {
  return a->tolerance >= 0 && a->tolerance <= 255 && a->patience >= 1 && a->min_samples >= 0;
}

// The totals of the last adaptive add (its update kernel's counts), once it has finished.
static int adapt_collect(rt_context* c) {
  if (!c->adapt_pending) return RT_OK;
  const int rc = quiesce(c);
  if (rc) return rc;
  const unsigned long long* totals = c->h_adapt.as<unsigned long long>();
  const int64_t active = (int64_t)totals[0];
  if (active != c->adapt_active) c->adapt_gen += 1;  // pixels stopped: the next add's schedule leaves them out
  c->adapt_active = active;
  c->adapt_sum = (int64_t)totals[1];
  c->adapt_pending = false;
  return RT_OK;
}

// The context's progression, for the entry point `who` (its name)
static int check_progression(const rt_context* c, const char* who) {
  if (c && c->prog_on && c->have_scene) return RT_OK;
  set_error(std::string(who) + ": the context has no progression (none begun, or it was ended)");
  return RT_E_INVALID;
}

extern "C" {

int rt_context_progressive_begin(rt_context* c, int32_t w, int32_t h, const rt_settings* st, int32_t rank,
                                 int32_t world, int32_t layout) {
  int rc = check_frame_args(c, w, h, st, rank, world, layout);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  c->prog_on = false;
  rc = quiesce(c);  // an add of the progression this one replaces may still use the sums
  if (rc) return rc;
  const size_t bytes = std::max<size_t>((size_t)local_tiles(c, w, h, rank, world) * 1024 * 3 * sizeof(double), 256);
  rc = grow(c, &c->d.prog, bytes);
  if (rc) return rc;
  HIP_TRY(hipMemsetAsync(c->d.prog.p, 0, bytes, c->stream));
  rc = wait_stream(c, c->stream);
  if (rc) return rc;
  c->prog_w = w;
  c->prog_h = h;
  c->prog_rank = rank;
  c->prog_world = world;
  c->prog_layout = layout;
  c->prog_st = *st;
  c->prog_done = 0;
  c->prog_adds = 0;
  c->adapt_on = false;  // (adaptive sampling is off after every begin)
  c->adapt_pending = false;
  c->prog_on = true;
  return RT_OK;
}

int rt_context_progressive_set_adaptive(rt_context* c, const rt_adaptive* a) {
  int rc = check_progression(c, "rt_context_progressive_set_adaptive");
  if (rc) return rc;
  if (c->prog_adds > 0) {
    set_error("rt_context_progressive_set_adaptive: the progression already has samples (call it before the first add)");
    return RT_E_INVALID;
  }
  if (!a) {
    c->adapt_on = false;
    return RT_OK;
  }
  if (!adaptive_ok(a)) {
    set_error("rt_context_progressive_set_adaptive: tolerance must be in 0..255, patience >= 1, min_samples >= 0");
    return RT_E_INVALID;
  }
  if (c->prog_st.sky != RT_SKY_NONE) {
    set_error("rt_context_progressive_set_adaptive: adaptive sampling does not support a sky (sky must be RT_SKY_NONE)");
    return RT_E_INVALID;
  }
  HIP_TRY(hipSetDevice(c->device));
  const size_t npx = (size_t)local_tiles(c, c->prog_w, c->prog_h, c->prog_rank, c->prog_world) * 1024;
  rc = grow(c, &c->d.adapt, 256 + std::max<size_t>(npx, 1) * 4 * sizeof(uint32_t));
  if (!rc) rc = grow_pinned(&c->h_adapt, 256);
  if (!rc) rc = quiesce(c);  // (an earlier adaptive progression's last add may still use the state)
  if (rc) return rc;
  // totals, counts and streaks 0; every pixel active; no kept image yet
  char* const state = c->d.adapt.as<char>();
  HIP_TRY(hipMemsetAsync(state, 0, 256 + npx * 2 * sizeof(uint32_t), c->stream));
  HIP_TRY(hipMemsetAsync(state + 256 + npx * 2 * sizeof(uint32_t), 1, npx * sizeof(uint32_t), c->stream));
  HIP_TRY(hipMemsetAsync(state + 256 + npx * 3 * sizeof(uint32_t), 0, npx * sizeof(uint32_t), c->stream));
  rc = wait_stream(c, c->stream);
  if (rc) return rc;
  c->adapt = *a;
  c->adapt._pad = 0;
  c->adapt_inimg = prog_image_pixels(c);
  c->adapt_active = c->adapt_inimg;
  c->adapt_sum = 0;
  c->adapt_gen += 1;  // (a new active set: no schedule of an earlier progression fits it)
  c->adapt_pending = false;
  c->adapt_on = true;
  return RT_OK;
}

int rt_context_progressive_counts_async(rt_context* c, uint32_t* d_counts, void* stream) {
  int rc = check_progression(c, "rt_context_progressive_counts_async");
  if (rc) return rc;
  if (!d_counts) {
    set_error("rt_context_progressive_counts_async: d_counts is NULL");
    return RT_E_INVALID;
  }
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = (hipStream_t)stream;
  rc = enter_stream(c, s);
  if (rc) return rc;
  AdaptParams a;
  adapt_params(c, &a);
  const int e = launch_progressive_counts(a, (uint32_t)c->prog_done, d_counts, s);
  return e == hipSuccess ? (int)RT_OK : launch_failed("progressive counts", e);
}

int rt_context_progressive_state(rt_context* c, int64_t out[4]) {
  int rc = check_progression(c, "rt_context_progressive_state");
  if (rc) return rc;
  if (!out) {
    set_error("rt_context_progressive_state: out is NULL");
    return RT_E_INVALID;
  }
  HIP_TRY(hipSetDevice(c->device));
  rc = quiesce(c);  // waits for the last add
  if (rc) return rc;
  if (c->adapt_on) {
    rc = adapt_collect(c);
    if (rc) return rc;
    out[0] = c->adapt_inimg;
    out[1] = c->adapt_active;
    out[2] = c->adapt_sum;
  } else {
    out[0] = out[1] = prog_image_pixels(c);
    out[2] = out[0] * c->prog_done;
  }
  out[3] = c->prog_adds;
  return RT_OK;
}

int rt_adaptive_step(const uint8_t old_rgba[4], const uint8_t new_rgba[4], int32_t had_image, int32_t count,
                     int32_t streak, const rt_adaptive* a, int32_t* new_streak) {
  if (!old_rgba || !new_rgba || !a || !new_streak) {
    set_error("rt_adaptive_step: NULL argument");
    return RT_E_INVALID;
  }
  if (!adaptive_ok(a) || count < 0 || streak < 0) {
    set_error("rt_adaptive_step: tolerance must be in 0..255, patience >= 1, min_samples, count and streak >= 0");
    return RT_E_INVALID;
  }
  uint32_t o = 0, n = 0;
  memcpy(&o, old_rgba, 4);
  memcpy(&n, new_rgba, 4);
  return rt_adaptive_rule(o, n, had_image != 0, count, streak, a->tolerance, a->patience, a->min_samples, new_streak);
}

int rt_context_progressive_add_async(rt_context* c, int32_t nsamples, float* d_linear, uint8_t* d_rgba,
                                     void* stream) {
  int rc = check_progression(c, "rt_context_progressive_add_async");
  if (rc) return rc;
  if (nsamples < 1 || c->prog_done + nsamples > c->prog_st.samples) {
    set_error("rt_context_progressive_add_async: nsamples must be >= 1 and stay within the cap (" +
              std::to_string(c->prog_done) + " of " + std::to_string(c->prog_st.samples) + " done)");
    return RT_E_INVALID;
  }
  HIP_TRY(hipSetDevice(c->device));
  const rt_settings* st = &c->prog_st;
  // adaptive: the render launches below only carry the sums
  // of the pixels still active (no image pointers, the active flags folded
  // into the schedule / the wavefront's sample ids); adaptive_update_kernel
  // then applies the stop rule and writes the image of every pixel.  The add
  // first learns how many pixels the last one left active (its totals).
  const bool adaptive = c->adapt_on;
  AdaptParams ap;
  if (adaptive) {
    rc = adapt_collect(c);
    if (rc) return rc;
    adapt_params(c, &ap);
    ap.n = nsamples;
    ap.out_linear = d_linear;
    ap.out_rgba = d_rgba;
  }
  KParams p;
  base_params(c, c->prog_w, c->prog_h, st, c->prog_rank, c->prog_world, c->prog_layout, &p);
  p.out_linear = adaptive ? nullptr : d_linear;
  p.out_rgba = adaptive ? nullptr : d_rgba;
  hipStream_t s = (hipStream_t)stream;
  rc = enter_stream(c, s);
  if (rc) return rc;
  if (adaptive && c->adapt_active == 0) {
    // every pixel has stopped: no render pass, the image is written all the same
    HIP_TRY(hipEventRecord(c->ev0, s));
  } else {
    // more samples than a block holds: sub-passes, as a frame's sample passes
    PassOpts o;
    o.first = (int)c->prog_done;
    o.n = nsamples;
    o.spp_total = o.first + nsamples;
    o.acc = &c->d.prog;
    o.keep = true;
    o.active = adaptive ? ap.active : nullptr;
    o.active_gen = c->adapt_gen;
    rc = render_passes(c, &p, st, s, o);
    if (rc) return rc;
  }
  if (adaptive) {  // after the render launches: the update, and its totals to the host
    const int e = launch_adaptive_update(ap, s);
    if (e != hipSuccess) return launch_failed("adaptive update", e);
    HIP_TRY(hipMemcpyAsync(c->h_adapt.p, ap.totals, 2 * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    c->adapt_pending = true;
  }
  c->prog_done += nsamples;
  c->prog_adds += 1;
  return leave_stream(c, s);
}

int64_t rt_context_progressive_samples(const rt_context* c) { return c && c->prog_on ? c->prog_done : -1; }

int rt_context_progressive_end(rt_context* c) {
  if (!c) {
    set_error("context is NULL");
    return RT_E_INVALID;
  }
  c->prog_on = false;
  c->adapt_on = false;
  if (!c->d.prog.p) return RT_OK;
  HIP_TRY(hipSetDevice(c->device));
  int rc = quiesce(c);  // the last add may still use the sums
  if (rc) return rc;
  dev_free(c->d.prog.p);
  c->d.prog = DevBuf{};
  return RT_OK;
}

int rt_rgba_delta_async(const uint8_t* d_a, const uint8_t* d_b, size_t npix, uint32_t* d_out, void* stream) {
  if (!d_out || (npix > 0 && (!d_a || !d_b))) {
    set_error("rt_rgba_delta_async: NULL buffer");
    return RT_E_INVALID;
  }
  const int e = launch_rgba_delta(d_a, d_b, npix, d_out, stream);
  return e == hipSuccess ? (int)RT_OK : launch_failed("rgba delta", e);
}

}  // extern "C"
