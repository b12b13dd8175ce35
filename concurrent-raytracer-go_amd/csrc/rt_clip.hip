// rt_clip.hip — temporal accumulation with history rectification
// (rt_temporal_clip_async, include/rt_api.h).  A file of its
// own: no other code object changes.
//
// The arithmetic is include/rt_clip.h, the functions rt_temporal_clip_host
// runs.  One launch, one lane per pixel, 64x4 blocks as temporal_motion_kernel:
// a wave covers 64 consecutive x of one row.  Two forms of step 5a's window:
//
//   plain   rt_cl_pixel as it is: every tap reads the frame and divides its
//           colour by its albedo, up to 3 * 81 binary64 divisions per pixel.
//   staged  the block computes e(q) once for its 64x4 tile plus a halo of
//           `radius` pixels and keeps it in LDS as binary64, with the tap's
//           validity and id; the window reads LDS.  The same doubles summed in
//           the same order, so the outputs are the plain form's to the bit.
//           The image is three planes of doubles with rows of 72 (64 + 2 * 4):
//           the lanes of a wave read consecutive 8-byte words (ds_read_b64,
//           256 bytes per 32 lanes: one bank row, no conflict at any offset).
//           24.5 KB per block, so LDS allows 6 blocks (24 waves) per CU.
//           Every lane of the block stages and reaches the one barrier before
//           any lane leaves (lanes outside the image, without a history, all).
//
// DESIGN.md §4.18 has the A/B that chose the form: staged from radius 2 on,
// plain at radius 1; RTGO_CLIP_FORM (plain | staged) overrides it for tests
// and the probe.
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/rt_clip.h"
#include "rt_device.h"
#include "rt_internal.h"

namespace rtgo {

namespace {
constexpr int kTileW = 64, kTileH = 4;
constexpr int kStageW = kTileW + 2 * RT_CL_MAX_RADIUS;  // 72: the row stride at every radius
constexpr int kStageH = kTileH + 2 * RT_CL_MAX_RADIUS;  // 12
constexpr int kStageN = kStageW * kStageH;              // 864
}  // namespace

// out_color / out_count / out_moments never alias the previous frame's color /
// count / moments (refused by the entry point).  kMoments false: prev_moments
// and out_moments are null and not used.  K.radius >= 1 in the staged form.
template <bool kMoments, bool kStaged>
__global__ __launch_bounds__(256) void temporal_clip_kernel(const rt_tp_constants C, const rt_cl_params K,
                                                            const rt_tp_buffers cur, const rt_tp_buffers prev,
                                                            const double* __restrict__ motion,
                                                            const int32_t num_objects,
                                                            const float* __restrict__ cur_albedo,
                                                            const float* __restrict__ prev_moments,
                                                            float* __restrict__ out_color,
                                                            float* __restrict__ out_count,
                                                            float* __restrict__ out_moments,
                                                            float* __restrict__ out_clipped,
                                                            uint8_t* __restrict__ out_rgba) {
  const int32_t x = (int32_t)(blockIdx.x * 64u + threadIdx.x), y = (int32_t)(blockIdx.y * 4u + threadIdx.y);
  float out[3], n, m[2], clipped = 0.0f;
  if constexpr (kStaged) {
    __shared__ double s_e[3][kStageN];
    __shared__ int32_t s_id[kStageN];
    __shared__ uint8_t s_ok[kStageN];
    const int32_t r = K.radius;
    const int32_t sw = kTileW + 2 * r, sn = sw * (kTileH + 2 * r);
    const int32_t x0 = (int32_t)(blockIdx.x * 64u) - r, y0 = (int32_t)(blockIdx.y * 4u) - r;
    for (int32_t i = (int32_t)(threadIdx.y * 64u + threadIdx.x); i < sn; i += 256) {
      const int32_t sy = i / sw, sx = i - sy * sw;  // sx < 72, sy < 12
      const int32_t qx = x0 + sx, qy = y0 + sy;
      const int32_t slot = sy * kStageW + sx;
      uint8_t ok = 0;
      if (qx >= 0 && qx < C.W && qy >= 0 && qy < C.H) {
        const size_t q = (size_t)qy * (size_t)C.W + (size_t)qx;
        if (rt_tp_valid(cur.depth[q])) {
          double e[3];
          rt_cl_e(cur.color, cur_albedo, q, e);
          s_e[0][slot] = e[0];
          s_e[1][slot] = e[1];
          s_e[2][slot] = e[2];
          s_id[slot] = cur.object ? cur.object[q] : 0;
          ok = 1;
        }
      }
      s_ok[slot] = ok;
    }
    __syncthreads();  // the only barrier: nobody has left yet
    if (x >= C.W || y >= C.H) return;
    rt_cl_history Hs;
    if (rt_cl_gather(kMoments ? 1 : 0, &C, &cur, &prev, motion, num_objects, cur_albedo, prev_moments, x, y, out, &n, m,
                     &Hs)) {
      const int32_t cx = (int32_t)threadIdx.x + r, cy = (int32_t)threadIdx.y + r;  // the pixel's slot
      const int32_t idp = cur.object ? cur.object[(size_t)y * (size_t)C.W + (size_t)x] : 0;
      double s1[3] = {0, 0, 0}, s2[3] = {0, 0, 0};
      int32_t nw = 0;
      for (int32_t dy = -r; dy <= r; ++dy)
        for (int32_t dx = -r; dx <= r; ++dx) {  // (a tap outside the image was staged as not ok)
          const int32_t slot = (cy + dy) * kStageW + (cx + dx);
          if (!s_ok[slot] || s_id[slot] != idp) continue;
          nw += 1;
          for (int k = 0; k < 3; ++k) {
            const double e = s_e[k][slot];
            s1[k] += e;
            s2[k] += e * e;
          }
        }
      const float c[3] = {out[0], out[1], out[2]};
      double fa[3];
      rt_cl_fa(cur_albedo, (size_t)y * (size_t)C.W + (size_t)x, fa);
      if (rt_cl_blend(kMoments ? 1 : 0, &C, &K, &Hs, c, fa, nw, s1, s2, out, &n, m)) clipped = 1.0f;
    }
  } else {
    if (x >= C.W || y >= C.H) return;
    rt_cl_pixel(kMoments ? 1 : 0, &C, &K, &cur, &prev, motion, num_objects, cur_albedo, prev_moments, x, y, out, &n, m,
                &clipped);
  }
  const size_t p = (size_t)y * (size_t)C.W + (size_t)x;
  out_color[p * 3 + 0] = out[0];
  out_color[p * 3 + 1] = out[1];
  out_color[p * 3 + 2] = out[2];
  out_count[p] = n;
  if constexpr (kMoments) {
    out_moments[p * 2 + 0] = m[0];
    out_moments[p * 2 + 1] = m[1];
  }
  if (out_clipped) out_clipped[p] = clipped;
  if (out_rgba)  // rt_tonemap_rgba of the stored floats
    *reinterpret_cast<uint32_t*>(out_rgba + p * 4) = tonemap_rgba8((double)out[0], (double)out[1], (double)out[2]);
}

template <bool kMoments, bool kStaged>
static void launch_form(const TemporalClipParams& p, void* stream) {
  const TemporalParams& t = p.mo.m.t;
  const dim3 grid((unsigned)((t.c.W + 63) / 64), (unsigned)((t.c.H + 3) / 4)), block(64, 4);
  hipLaunchKernelGGL((temporal_clip_kernel<kMoments, kStaged>), grid, block, 0, (hipStream_t)stream, t.c, p.clip, t.cur,
                     t.prev, p.mo.motion, p.mo.num_objects, p.mo.m.cur_albedo, p.mo.m.prev_moments, t.out_color,
                     t.out_count, p.mo.m.out_moments, p.out_clipped, t.out_rgba);
}

int launch_temporal_clip(const TemporalClipParams& p, void* stream) {
  bool staged = p.clip.radius >= kClipStagedFromRadius;
  if (const char* form = getenv("RTGO_CLIP_FORM")) {
    if (!strcmp(form, "plain")) staged = false;
    if (!strcmp(form, "staged")) staged = true;
  }
  // without a window, or without a previous frame to rectify, there is nothing to stage
  if (p.clip.radius < 1 || !p.mo.m.t.c.has_prev) staged = false;
  const bool moments = p.mo.m.out_moments != nullptr;
  if (moments && staged) launch_form<true, true>(p, stream);
  if (moments && !staged) launch_form<true, false>(p, stream);
  if (!moments && staged) launch_form<false, true>(p, stream);
  if (!moments && !staged) launch_form<false, false>(p, stream);
  return (int)hipGetLastError();
}

int preload_clip_kernels() {
  hipFuncAttributes a;
  return (int)hipFuncGetAttributes(&a, reinterpret_cast<const void*>(temporal_clip_kernel<true, false>));
}

}  // namespace rtgo
