/*
 * rt_motion.h — temporal accumulation with per-object motion (DESIGN.md §4.17;
 * the definition is in include/rt_api.h at rt_temporal_motion_async), as one
 * inline function shared by the device kernels that apply it (rt_motion.hip)
 * and the host entry point that runs it without a device
 * (rt_temporal_motion_host, rt_motion_host.cpp).
 *
 * rt_mo_pixel restates rt_tp_pixel's steps 1 to 6 (rt_temporal.h) and, with
 * kMoments, rt_vr_tp_pixel's moment sums beside them (rt_variance.h) instead of
 * changing either, so that their kernels' code objects stay what they are;
 * tests hold a table of zeros to their bits.  The one addition is in step 3:
 * the world point is moved back by its object's translation before it is
 * taken into the previous camera.  kMoments is a constant at every call, so
 * the colour-only form carries nothing of the moments.
 *
 * Binary64 `+ - * /`, comparisons and floor only, in a fixed order, on values
 * widened from binary32: host and device agree to the bit under
 * -ffp-contract=off.  Every address comes from the pixel's coordinates and
 * from integers that were compared against their bounds first: ix and iy
 * against the image's, the pixel's object id against the table's.
 */
#ifndef RT_MOTION_H
#define RT_MOTION_H

#include <stddef.h>
#include <stdint.h>

#include "rt_temporal.h"
#include "rt_variance.h"

#if defined(__HIPCC__)
#define RT_MOTION_FN __host__ __device__ static inline __attribute__((always_inline))
#else
#define RT_MOTION_FN static inline __attribute__((always_inline))
#endif

/* Pixel (x, y) of the image, 0 <= x < W and 0 <= y < H.  cur->object is not
 * NULL; prev (and prev->object, and with kMoments prev_moments) is read only
 * when C->has_prev.  motion holds num_objects rows of 3 doubles.  out[3] and
 * *out_count are the values to store, and with kMoments out_m[2]; without it
 * cur_albedo, prev_moments and out_m are not used. */
RT_MOTION_FN void rt_mo_pixel(const int kMoments, const rt_tp_constants* C, const rt_tp_buffers* cur,
                              const rt_tp_buffers* prev, const double* motion, int32_t num_objects,
                              const float* cur_albedo, const float* prev_moments, int32_t x, int32_t y, float out[3],
                              float* out_count, float out_m[2]) {
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
    return;
  }
  *out_count = 1.0f;
  if (!C->has_prev) return;
  /* 3. the world point, and where it was: the id is compared against the
   * table's bounds before it forms an address */
  const int32_t idp = cur->object[p];
  double m[3] = {0.0, 0.0, 0.0};
  if (idp >= 0 && idp < num_objects) {
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
    const double Pm = P - m[k];
    d[k] = Pm - C->po[k];
  }
  /* 4. into the previous camera */
  const double t = rt_tp_dot(d, C->a) / C->aa;
  if (!(t > 0)) return;
  double e[3];
  for (int k = 0; k < 3; ++k) e[k] = d[k] / t - C->g[k];
  const double fx = (rt_tp_dot(e, C->ph) / C->hh) * (double)C->W - 0.5;
  const double fy = (rt_tp_dot(e, C->pv) / C->vv) * (double)C->H - 0.5;
  if (!(fx > -1 && fx < (double)C->W && fy > -1 && fy < (double)C->H)) return; /* (a NaN fails) */
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
      if (prev->object[q] != idp) continue;
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
  if (!(sumw >= C->min_weight)) return;
  /* 6. the blend */
  const double h0 = s0 / sumw, h1 = s1 / sumw, h2 = s2 / sumw, n = sumn / sumw;
  double nn = n + 1.0;
  if (nn > C->max_history) nn = C->max_history;
  out[0] = (float)(h0 + ((double)c0 - h0) / nn);
  out[1] = (float)(h1 + ((double)c1 - h1) / nn);
  out[2] = (float)(h2 + ((double)c2 - h2) / nn);
  *out_count = (float)nn;
  if (kMoments) {
    const double hm0 = sm0 / sumw, hm1 = sm1 / sumw;
    out_m[0] = (float)(hm0 + (l - hm0) / nn);
    out_m[1] = (float)(hm1 + (ll - hm1) / nn);
  }
}

#endif /* RT_MOTION_H */
