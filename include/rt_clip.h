/*
 * rt_clip.h — temporal accumulation with history rectification (DESIGN.md
 * §4.18; the definition is in include/rt_api.h at rt_temporal_clip_async), as
 * inline functions shared by the device kernels that apply it (rt_clip.hip),
 * the host entry point that runs it without a device (rt_temporal_clip_host,
 * rt_clip_host.cpp) and the sanitizer program (tests/c/clip_sanitize.cpp).
 *
 * A pixel is three functions, so that a kernel may take the window's sums from
 * somewhere else than global memory and still run the same arithmetic:
 *   rt_cl_gather   steps 1 to 5: rt_mo_pixel's (rt_motion.h) restated, not
 *                  changed, so that its kernels' code objects stay what they
 *                  are; without a table m = 0 and ids are optional, which is
 *                  rt_tp_pixel's / rt_vr_tp_pixel's steps to the bit.
 *   rt_cl_window   step 5a's sums over the (2r+1)^2 window, from the frame.
 *   rt_cl_blend    step 5a's range, step 5b and step 6.
 * rt_cl_pixel is the three in a row.  kMoments is a constant at every call.
 *
 * Binary64 `+ - * /`, sqrt (correctly rounded on both sides), comparisons and
 * floor only, in a fixed order, on values widened from binary32: host and
 * device agree to the bit under -ffp-contract=off.  Every address comes from
 * the pixel's coordinates, the window's offsets and integers that were
 * compared against their bounds first; the one guarded address from a pixel's
 * value is the motion table's.
 */
#ifndef RT_CLIP_H
#define RT_CLIP_H

#include <stddef.h>
#include <stdint.h>

#include "rt_denoise.h"
#include "rt_temporal.h"
#include "rt_variance.h"

#if defined(__HIPCC__)
#define RT_CLIP_FN __host__ __device__ static inline __attribute__((always_inline))
#else
#define RT_CLIP_FN static inline __attribute__((always_inline))
#endif

#define RT_CL_MAX_RADIUS 4

/* rt_history_clip's fields, checked (rt_cl_params_ok). */
typedef struct {
  int32_t radius, min_taps;
  double gamma, min_half;
} rt_cl_params;

/* The parameter rules of rt_history_clip: 1 when all four are in range. */
RT_CLIP_FN int rt_cl_params_ok(int32_t radius, int32_t min_taps, double gamma, double min_half) {
  if (radius < 0 || radius > RT_CL_MAX_RADIUS || min_taps < 1) return 0;
  if (!(rt_tp_finite(gamma) && gamma >= 0)) return 0;
  return rt_tp_finite(min_half) && min_half >= 0;
}

/* What steps 1 to 5 leave for the blend of a pixel that found a history. */
typedef struct {
  double sumw, s[3], sumn, sm[2];
  double l, ll; /* with kMoments: the current luminance and its square */
} rt_cl_history;

/* e(color[q], albedo[q]): rt_variance's demodulated colour in binary64. */
RT_CLIP_FN void rt_cl_e(const float* color, const float* albedo, size_t q, double e[3]) {
  for (int k = 0; k < 3; ++k) {
    const double c = (double)color[q * 3 + k];
    e[k] = albedo ? c / rt_dn_floor_albedo(albedo[q * 3 + k]) : c;
  }
}

/* Steps 1 to 5 for pixel (x, y), 0 <= x < W and 0 <= y < H.  out[3],
 * *out_count and with kMoments out_m[2] are set to the values of a pixel
 * without a history; returns 1 when step 5 found one (Hs is then filled and
 * rt_cl_blend finishes the pixel), else 0.  motion may be NULL (m = 0;
 * cur->object may then be NULL too); prev is read only when C->has_prev;
 * cur_albedo is read only with kMoments. */
RT_CLIP_FN int rt_cl_gather(const int kMoments, const rt_tp_constants* C, const rt_tp_buffers* cur,
                            const rt_tp_buffers* prev, const double* motion, int32_t num_objects,
                            const float* cur_albedo, const float* prev_moments, int32_t x, int32_t y, float out[3],
                            float* out_count, float out_m[2], rt_cl_history* Hs) {
  const size_t W = (size_t)C->W;
  const size_t p = (size_t)y * W + (size_t)x;
  const float c0 = cur->color[p * 3 + 0], c1 = cur->color[p * 3 + 1], c2 = cur->color[p * 3 + 2];
  const float zf = cur->depth[p];
  double l = 0, ll = 0;
  if (kMoments) {
    l = rt_vr_pixel_lum(cur->color, cur_albedo, p);
    ll = l * l;
    out_m[0] = (float)l;
    out_m[1] = (float)ll;
  }
  out[0] = c0;
  out[1] = c1;
  out[2] = c2;
  if (!rt_tp_valid(zf)) {
    *out_count = 0.0f;
    return 0;
  }
  *out_count = 1.0f;
  if (!C->has_prev) return 0;
  /* 3. the world point, and where it was: the id is compared against the
   * table's bounds before it forms an address */
  const int32_t idp = cur->object ? cur->object[p] : 0;
  double m[3] = {0.0, 0.0, 0.0};
  if (motion && idp >= 0 && idp < num_objects) {
    const double* row = motion + (size_t)idp * 3;
    m[0] = row[0];
    m[1] = row[1];
    m[2] = row[2];
  }
  const double z = (double)zf;
  const double u = ((double)x + 0.5) / (double)C->W, v = ((double)y + 0.5) / (double)C->H;
  double d[3];
  for (int k = 0; k < 3; ++k) {
    const double dir = ((C->l[k] + C->h[k] * u) + C->v[k] * v) - C->o[k];
    const double P = C->o[k] + dir * z;
    const double Pm = P - m[k]; /* (x - 0.0 is x: without a table this is rt_tp_pixel's d) */
    d[k] = Pm - C->po[k];
  }
  /* 4. into the previous camera */
  const double t = rt_tp_dot(d, C->a) / C->aa;
  if (!(t > 0)) return 0;
  double e[3];
  for (int k = 0; k < 3; ++k) e[k] = d[k] / t - C->g[k];
  const double fx = (rt_tp_dot(e, C->ph) / C->hh) * (double)C->W - 0.5;
  const double fy = (rt_tp_dot(e, C->pv) / C->vv) * (double)C->H - 0.5;
  if (!(fx > -1 && fx < (double)C->W && fy > -1 && fy < (double)C->H)) return 0; /* (a NaN fails) */
  /* 5. the bilinear fetch: ix in [-1, W - 1], iy in [-1, H - 1] */
  const double flx = __builtin_floor(fx), fly = __builtin_floor(fy);
  const int32_t ix = (int32_t)flx, iy = (int32_t)fly;
  const double wx = fx - flx, wy = fy - fly;
  double n0 = 0, n1 = 0, n2 = 0;
  if (cur->normal) {
    n0 = (double)cur->normal[p * 3 + 0];
    n1 = (double)cur->normal[p * 3 + 1];
    n2 = (double)cur->normal[p * 3 + 2];
  }
  double sumw = 0, s0 = 0, s1 = 0, s2 = 0, sumn = 0, sm0 = 0, sm1 = 0;
  for (int32_t j = 0; j < 2; ++j) {
    const int32_t qy = iy + j;
    if (qy < 0 || qy >= C->H) continue;
    for (int32_t i = 0; i < 2; ++i) {
      const int32_t qx = ix + i;
      if (qx < 0 || qx >= C->W) continue;
      const size_t q = (size_t)qy * W + (size_t)qx;
      const float zq = prev->depth[q];
      if (!rt_tp_valid(zq)) continue;
      if (cur->object && prev->object[q] != idp) continue;
      if (cur->normal) {
        const double nd = (n0 * (double)prev->normal[q * 3 + 0] + n1 * (double)prev->normal[q * 3 + 1]) +
                          n2 * (double)prev->normal[q * 3 + 2];
        if (nd < C->normal_min) continue;
      }
      if (C->depth_tol > 0) {
        const double dz = (double)zq - t;
        if ((dz < 0 ? -dz : dz) > C->depth_tol * t) continue;
      }
      const double w = (i ? wx : 1.0 - wx) * (j ? wy : 1.0 - wy);
      sumw += w;
      s0 += w * (double)prev->color[q * 3 + 0];
      s1 += w * (double)prev->color[q * 3 + 1];
      s2 += w * (double)prev->color[q * 3 + 2];
      sumn += w * (double)prev->count[q];
      if (kMoments) {
        sm0 += w * (double)prev_moments[q * 2 + 0];
        sm1 += w * (double)prev_moments[q * 2 + 1];
      }
    }
  }
  if (!(sumw >= C->min_weight)) return 0;
  Hs->sumw = sumw;
  Hs->s[0] = s0;
  Hs->s[1] = s1;
  Hs->s[2] = s2;
  Hs->sumn = sumn;
  Hs->sm[0] = sm0;
  Hs->sm[1] = sm1;
  Hs->l = l;
  Hs->ll = ll;
  return 1;
}

/* 5a, the window's sums from the current frame: the taps of pixel (x, y) in
 * the definition's order (dy outer, dx inner).  Returns nw. */
RT_CLIP_FN int32_t rt_cl_window(int32_t W, int32_t H, int32_t radius, const rt_tp_buffers* cur, const float* cur_albedo,
                                int32_t x, int32_t y, double s1[3], double s2[3]) {
  const int32_t idp = cur->object ? cur->object[(size_t)y * (size_t)W + (size_t)x] : 0;
  int32_t nw = 0;
  s1[0] = s1[1] = s1[2] = 0;
  s2[0] = s2[1] = s2[2] = 0;
  for (int32_t dy = -radius; dy <= radius; ++dy) {
    const int32_t qy = y + dy;
    if (qy < 0 || qy >= H) continue;
    for (int32_t dx = -radius; dx <= radius; ++dx) {
      const int32_t qx = x + dx;
      if (qx < 0 || qx >= W) continue;
      const size_t q = (size_t)qy * (size_t)W + (size_t)qx;
      if (!rt_tp_valid(cur->depth[q])) continue;
      if (cur->object && cur->object[q] != idp) continue;
      double e[3];
      rt_cl_e(cur->color, cur_albedo, q, e);
      nw += 1;
      for (int k = 0; k < 3; ++k) {
        s1[k] += e[k];
        s2[k] += e[k] * e[k];
      }
    }
  }
  return nw;
}

/* The rest of a pixel that found a history: 5a's range from the window's sums
 * (skipped when radius is 0 or nw < min_taps), 5b and step 6.  c[3] is the
 * pixel's current colour and fa[3] its floored albedo (1 without albedo).
 * Returns 1 when a channel's history was replaced. */
RT_CLIP_FN int rt_cl_blend(const int kMoments, const rt_tp_constants* C, const rt_cl_params* K,
                           const rt_cl_history* Hs, const float c[3], const double fa[3], int32_t nw,
                           const double s1[3], const double s2[3], float out[3], float* out_count, float out_m[2]) {
  const double sumw = Hs->sumw;
  double h[3];
  int clipped = 0;
  for (int k = 0; k < 3; ++k) h[k] = Hs->s[k] / sumw;
  if (K->radius > 0 && nw >= K->min_taps) {
    const double n = (double)nw;
    for (int k = 0; k < 3; ++k) {
      const double mu = s1[k] / n;
      double var = s2[k] / n - mu * mu;
      var = var > 0 ? var : 0;
      const double half = K->gamma * __builtin_sqrt(var) + K->min_half;
      const double he = h[k] / fa[k], lo = mu - half, hi = mu + half;
      const double hc = he < lo ? lo : (he > hi ? hi : he); /* (a NaN fails both and stays) */
      if (hc != he) {
        h[k] = hc * fa[k];
        clipped = 1;
      }
    }
  }
  /* 6. the blend */
  const double n = Hs->sumn / sumw;
  double nn = n + 1.0;
  if (nn > C->max_history) nn = C->max_history;
  out[0] = (float)(h[0] + ((double)c[0] - h[0]) / nn);
  out[1] = (float)(h[1] + ((double)c[1] - h[1]) / nn);
  out[2] = (float)(h[2] + ((double)c[2] - h[2]) / nn);
  *out_count = (float)nn;
  if (kMoments) {
    const double hm0 = Hs->sm[0] / sumw, hm1 = Hs->sm[1] / sumw;
    out_m[0] = (float)(hm0 + (Hs->l - hm0) / nn);
    out_m[1] = (float)(hm1 + (Hs->ll - hm1) / nn);
  }
  return clipped;
}

/* fa[k] of pixel p: the floored albedo, or 1 without albedo. */
RT_CLIP_FN void rt_cl_fa(const float* cur_albedo, size_t p, double fa[3]) {
  for (int k = 0; k < 3; ++k) fa[k] = cur_albedo ? rt_dn_floor_albedo(cur_albedo[p * 3 + k]) : 1.0;
}

/* Pixel (x, y) whole.  out[3], *out_count, with kMoments out_m[2], and
 * *out_clipped (0 or 1) are the values to store.  cur_albedo feeds the window
 * with and without kMoments. */
RT_CLIP_FN void rt_cl_pixel(const int kMoments, const rt_tp_constants* C, const rt_cl_params* K,
                            const rt_tp_buffers* cur, const rt_tp_buffers* prev, const double* motion,
                            int32_t num_objects, const float* cur_albedo, const float* prev_moments, int32_t x,
                            int32_t y, float out[3], float* out_count, float out_m[2], float* out_clipped) {
  rt_cl_history Hs;
  *out_clipped = 0.0f;
  if (!rt_cl_gather(kMoments, C, cur, prev, motion, num_objects, cur_albedo, prev_moments, x, y, out, out_count, out_m,
                    &Hs))
    return;
  const size_t p = (size_t)y * (size_t)C->W + (size_t)x;
  const float c[3] = {out[0], out[1], out[2]};
  double fa[3], s1[3] = {0, 0, 0}, s2[3] = {0, 0, 0};
  int32_t nw = 0;
  rt_cl_fa(cur_albedo, p, fa);
  if (K->radius > 0) nw = rt_cl_window(C->W, C->H, K->radius, cur, cur_albedo, x, y, s1, s2);
  if (rt_cl_blend(kMoments, C, K, &Hs, c, fa, nw, s1, s2, out, out_count, out_m)) *out_clipped = 1.0f;
}

#endif /* RT_CLIP_H */
