/*
 * rt_variance.h — variance-guided denoising (the definitions
 * are in include/rt_api.h at rt_temporal_moments_async, rt_variance_async and
 * rt_denoise_var_async), as inline functions shared by the device kernels that
 * apply them (rt_variance.hip) and the host entry points that run them without
 * a device (rt_variance_host.cpp): one pixel of the moments pass, one pixel of
 * the variance pass, and the records, one level and the output of the
 * variance-guided à-trous filter.
 *
 * The arithmetic that is rt_denoise_async's or rt_temporal_async's is taken
 * from rt_denoise.h and rt_temporal.h (validity, the albedo floor, h, the
 * level constants, dot, the parameter rules).  rt_vr_tp_pixel restates
 * rt_tp_pixel's steps 1 to 6 with the moment sums beside the colour sums
 * instead of changing rt_tp_pixel, so that the temporal kernel's code object
 * stays what it is; tests hold its colour and count to rt_tp_pixel's bits.
 *
 * Binary64 `+ - * /`, comparisons and floor only, in a fixed order, on values
 * widened from binary32: host and device agree to the bit under
 * -ffp-contract=off.  No address depends on a pixel's value.
 */
#ifndef RT_VARIANCE_H
#define RT_VARIANCE_H

#include <stddef.h>
#include <stdint.h>

#include "rt_denoise.h"
#include "rt_temporal.h"

#if defined(__HIPCC__)
#define RT_VARIANCE_FN __host__ __device__ static inline
#else
#define RT_VARIANCE_FN static inline
#endif

#define RT_VR_EPS 9.094947017729282379150390625e-13 /* 2^-40: keeps 1 / (sigma_lum^2 * g + eps) finite at g = 0 */

/* lum(e) = (0.2126 * e0 + 0.7152 * e1) + 0.0722 * e2 */
RT_VARIANCE_FN double rt_vr_lum(double e0, double e1, double e2) { return (0.2126 * e0 + 0.7152 * e1) + 0.0722 * e2; }

/* lum(e(color[p], albedo[p])): the demodulated luminance in binary64, not
 * rounded to binary32 in between (albedo NULL: the colour's own luminance). */
RT_VARIANCE_FN double rt_vr_pixel_lum(const float* color, const float* albedo, size_t p) {
  double e[3];
  for (int k = 0; k < 3; ++k) {
    const double c = (double)color[p * 3 + k];
    e[k] = albedo ? c / rt_dn_floor_albedo(albedo[p * 3 + k]) : c;
  }
  return rt_vr_lum(e[0], e[1], e[2]);
}

/* ---- 1. the moments pass (rt_temporal_moments_async) ---- */

/* Pixel (x, y): rt_tp_pixel's steps 1 to 6 in its order of operations, with
 * summ[2] continued beside sum[3] at every accepted tap.  prev and
 * prev_moments are read only when C->has_prev.  out[3], *out_count and
 * out_m[2] are the values to store. */
RT_VARIANCE_FN void rt_vr_tp_pixel(const rt_tp_constants* C, const rt_tp_buffers* cur, const rt_tp_buffers* prev,
                                   const float* cur_albedo, const float* prev_moments, int32_t x, int32_t y,
                                   float out[3], float* out_count, float out_m[2]) {
  const size_t W = (size_t)C->W;
  const size_t p = (size_t)y * W + (size_t)x;
  const float c0 = cur->color[p * 3 + 0], c1 = cur->color[p * 3 + 1], c2 = cur->color[p * 3 + 2];
  const float zf = cur->depth[p];
  const double l = rt_vr_pixel_lum(cur->color, cur_albedo, p);
  const double ll = l * l;
  out[0] = c0;
  out[1] = c1;
  out[2] = c2;
  out_m[0] = (float)l;
  out_m[1] = (float)ll;
  if (!rt_tp_valid(zf)) {
    *out_count = 0.0f;
    return;
  }
  *out_count = 1.0f;
  if (!C->has_prev) return;
  /* 3. the world point */
  const double z = (double)zf;
  const double u = ((double)x + 0.5) / (double)C->W, v = ((double)y + 0.5) / (double)C->H;
  double d[3];
  for (int k = 0; k < 3; ++k) {
    const double dir = ((C->l[k] + C->h[k] * u) + C->v[k] * v) - C->o[k];
    const double P = C->o[k] + dir * z;
    d[k] = P - C->po[k];
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
  const int32_t idp = cur->object ? cur->object[p] : 0;
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
      sm0 += w * (double)prev_moments[q * 2 + 0];
      sm1 += w * (double)prev_moments[q * 2 + 1];
    }
  }
  if (!(sumw >= C->min_weight)) return;
  /* 6. the blend */
  const double h0 = s0 / sumw, h1 = s1 / sumw, h2 = s2 / sumw, n = sumn / sumw;
  const double hm0 = sm0 / sumw, hm1 = sm1 / sumw;
  double nn = n + 1.0;
  if (nn > C->max_history) nn = C->max_history;
  out[0] = (float)(h0 + ((double)c0 - h0) / nn);
  out[1] = (float)(h1 + ((double)c1 - h1) / nn);
  out[2] = (float)(h2 + ((double)c2 - h2) / nn);
  *out_count = (float)nn;
  out_m[0] = (float)(hm0 + (l - hm0) / nn);
  out_m[1] = (float)(hm1 + (ll - hm1) / nn);
}

/* ---- the guide weight both spatial passes share ---- */

/* Steps 2 and 3 of rt_denoise_async's tap weight, in its order of operations,
 * continued from w (h[|dx|] * h[|dy|] in the filter, 1 in the variance pass).
 * L carries nsq, depth_on and sigma_depth (rt_dn_level_of). */
RT_VARIANCE_FN double rt_vr_guide_weight(const rt_dn_level* L, double w, const rt_dn_guide* gp, const rt_dn_guide* gq) {
  if (L->nsq >= 0) {
    double t = ((double)gp->n[0] * (double)gq->n[0] + (double)gp->n[1] * (double)gq->n[1]) +
               (double)gp->n[2] * (double)gq->n[2];
    t = t > 0 ? t : 0;
    for (int32_t j = 0; j < L->nsq; ++j) t = t * t;
    w = w * t;
  }
  if (L->depth_on) {
    const double r = ((double)gq->z - (double)gp->z) / (L->sigma_depth * (double)gp->z);
    w = w / (1.0 + r * r);
  }
  return w;
}

/* ---- 2. the variance pass (rt_variance_async) ---- */

typedef struct {
  const float* color;    /* W*H*3 */
  const float* normal;   /* W*H*3 */
  const float* depth;    /* W*H */
  const float* albedo;   /* W*H*3 or NULL */
  const int32_t* object; /* W*H or NULL */
  const float* moments;  /* W*H*2 or NULL */
  const float* count;    /* W*H or NULL (given exactly when moments is) */
} rt_vr_buffers;

/* The parameter rules of rt_variance: 1 when all three are in range. */
RT_VARIANCE_FN int rt_vr_params_ok(double min_history, int32_t normal_power, double sigma_depth) {
  if (!(rt_tp_finite(min_history) && min_history >= 1)) return 0;
  if (normal_power < 0 || normal_power > 128 || (normal_power & (normal_power - 1)) != 0) return 0;
  return rt_tp_finite(sigma_depth) && sigma_depth >= 0;
}

RT_VARIANCE_FN rt_dn_guide rt_vr_guide_at(const rt_vr_buffers* B, size_t p) {
  rt_dn_guide g;
  g.n[0] = B->normal[p * 3 + 0];
  g.n[1] = B->normal[p * 3 + 1];
  g.n[2] = B->normal[p * 3 + 2];
  g.z = B->depth[p];
  return g;
}

/* Pixel (x, y)'s variance.  L = rt_dn_level_of(W, H, 0, normal_power, 0,
 * sigma_depth): the step is 1 and the colour stop is not used. */
RT_VARIANCE_FN float rt_vr_variance_pixel(const rt_dn_level* L, double min_history, const rt_vr_buffers* B, int32_t x,
                                          int32_t y) {
  const size_t W = (size_t)L->W;
  const size_t p = (size_t)y * W + (size_t)x;
  const rt_dn_guide gp = rt_vr_guide_at(B, p);
  if (!rt_dn_valid(gp.z)) return 0.0f;
  double n = 1.0;
  if (B->count) {
    const double c = (double)B->count[p];
    n = c > 1.0 ? c : 1.0;
  }
  if (B->moments && (double)B->count[p] >= min_history) { /* temporal */
    const double m1 = (double)B->moments[p * 2 + 0], m2 = (double)B->moments[p * 2 + 1];
    double v = m2 - m1 * m1;
    v = v > 0 ? v : 0;
    return (float)(v / n);
  }
  /* spatial: 7 x 7 at step 1 */
  const int32_t idp = B->object ? B->object[p] : 0;
  double sumw = 0, s1 = 0, s2 = 0;
  for (int32_t dy = -3; dy <= 3; ++dy) {
    const int32_t qy = y + dy;
    if (qy < 0 || qy >= L->H) continue;
    for (int32_t dx = -3; dx <= 3; ++dx) {
      const int32_t qx = x + dx;
      if (qx < 0 || qx >= L->W) continue;
      const size_t q = (size_t)qy * W + (size_t)qx;
      const rt_dn_guide gq = rt_vr_guide_at(B, q);
      if (!rt_dn_valid(gq.z)) continue;
      if (B->object && B->object[q] != idp) continue;
      const double w = rt_vr_guide_weight(L, 1.0, &gp, &gq);
      double m1q, m2q;
      if (B->moments) {
        m1q = (double)B->moments[q * 2 + 0];
        m2q = (double)B->moments[q * 2 + 1];
      } else {
        m1q = rt_vr_pixel_lum(B->color, B->albedo, q);
        m2q = m1q * m1q;
      }
      s1 += w * m1q;
      s2 += w * m2q;
      sumw += w;
    }
  }
  if (!(sumw > 0)) return 0.0f;
  const double a = s1 / sumw;
  double v = s2 / sumw - a * a;
  v = v > 0 ? v : 0;
  return (float)(v / n);
}

/* ---- 3. the variance-guided filter (rt_denoise_var_async) ---- */

/* A pixel's colour record: e_i(p) and var_i(p), ping-ponged from level to
 * level.  The guide record is rt_dn_guide, written once, and the ids are a
 * plane of their own (0 everywhere when no ids are given). */
typedef struct __attribute__((aligned(16))) {
  float c[3]; /* e_i(p) */
  float var;  /* var_i(p) */
} rt_vr_color;

/* One level's constants: rt_denoise's with the colour stop off, and the
 * luminance stop's. */
typedef struct {
  rt_dn_level dn;   /* W, H, step, nsq, depth_on, sigma_depth (color_on is 0) */
  int32_t lum_on;   /* sigma_lum > 0 */
  int32_t prefilter;
  double sl2;       /* sigma_lum * sigma_lum */
} rt_vr_level;

RT_VARIANCE_FN rt_vr_level rt_vr_level_of(int32_t W, int32_t H, int32_t level, int32_t normal_power, double sigma_lum,
                                          double sigma_depth, int32_t prefilter) {
  rt_vr_level L;
  L.dn = rt_dn_level_of(W, H, level, normal_power, 0.0, sigma_depth);
  L.lum_on = sigma_lum > 0;
  L.prefilter = prefilter;
  L.sl2 = sigma_lum * sigma_lum;
  return L;
}

/* The parameter rules of rt_denoise_var: 1 when all are in range. */
RT_VARIANCE_FN int rt_vr_filter_params_ok(int32_t levels, int32_t normal_power, double sigma_lum, double sigma_depth,
                                          int32_t demodulate, int32_t prefilter) {
  if (levels < 1 || levels > 8) return 0;
  if (normal_power < 0 || normal_power > 128 || (normal_power & (normal_power - 1)) != 0) return 0;
  if (!(rt_tp_finite(sigma_lum) && sigma_lum >= 0)) return 0;
  if (!(rt_tp_finite(sigma_depth) && sigma_depth >= 0)) return 0;
  return (demodulate == 0 || demodulate == 1) && (prefilter == 0 || prefilter == 1);
}

/* Prepare: pixel p's records (rt_dn_prepare's, with the variance in the
 * colour record's fourth word and the id in its plane). */
RT_VARIANCE_FN void rt_vr_prepare(const float* color, const float* albedo, const float* normal, const float* depth,
                                  const int32_t* object, const float* variance, size_t p, rt_vr_color* e,
                                  rt_dn_guide* g, int32_t* id) {
  rt_dn_color t;
  rt_dn_prepare(color, albedo, normal, depth, object, p, &t, g);
  e->c[0] = t.c[0];
  e->c[1] = t.c[1];
  e->c[2] = t.c[2];
  e->var = variance[p];
  *id = t.id;
}

RT_VARIANCE_FN double rt_vr_k(int32_t dx, int32_t dy) { /* {1/4, 1/8, 1/16} by |dx| + |dy| */
  const int32_t a = (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy);
  return a == 0 ? 0.25 : (a == 1 ? 0.125 : 0.0625);
}

/* One level for pixel (x, y): e_{i+1}(p) and var_{i+1}(p) from the records of
 * level i.  The prefilter's 9 taps, then the 25 taps, both in the definition's
 * order (dy outer, dx inner), binary64 sums per pixel.  Every index is
 * computed from coordinates and bounds alone. */
RT_VARIANCE_FN rt_vr_color rt_vr_level_pixel(const rt_vr_level* L, const rt_vr_color* e, const rt_dn_guide* g,
                                             const int32_t* id, int32_t x, int32_t y) {
  const int32_t W = L->dn.W, H = L->dn.H;
  const size_t p = (size_t)y * (size_t)W + (size_t)x;
  const rt_vr_color ep = e[p];
  const rt_dn_guide gp = g[p];
  if (!rt_dn_valid(gp.z)) return ep;
  const int32_t idp = id[p];
  double inv = 0, lp = 0;
  if (L->lum_on) {
    double gv = (double)ep.var;
    if (L->prefilter) {
      double sumg = 0, sumk = 0;
      for (int32_t dy = -1; dy <= 1; ++dy) {
        const int32_t qy = y + dy;
        if (qy < 0 || qy >= H) continue;
        for (int32_t dx = -1; dx <= 1; ++dx) {
          const int32_t qx = x + dx;
          if (qx < 0 || qx >= W) continue;
          const size_t q = (size_t)qy * (size_t)W + (size_t)qx;
          if (!rt_dn_valid(g[q].z) || id[q] != idp) continue;
          const double k = rt_vr_k(dx, dy);
          sumg += k * (double)e[q].var;
          sumk += k;
        }
      }
      gv = sumg / sumk; /* (the centre tap is never skipped: sumk >= 1/4) */
    }
    inv = 1.0 / (L->sl2 * gv + RT_VR_EPS);
    lp = rt_vr_lum((double)ep.c[0], (double)ep.c[1], (double)ep.c[2]);
  }
  double sumw = 0, s0 = 0, s1 = 0, s2 = 0, sumv = 0;
  for (int32_t dy = -2; dy <= 2; ++dy) {
    const int32_t qy = y + L->dn.step * dy;
    if (qy < 0 || qy >= H) continue;
    for (int32_t dx = -2; dx <= 2; ++dx) {
      const int32_t qx = x + L->dn.step * dx;
      if (qx < 0 || qx >= W) continue;
      const size_t q = (size_t)qy * (size_t)W + (size_t)qx;
      const rt_dn_guide gq = g[q];
      if (!rt_dn_valid(gq.z) || id[q] != idp) continue;
      const rt_vr_color eq = e[q];
      double w = rt_vr_guide_weight(&L->dn, rt_dn_h(dx) * rt_dn_h(dy), &gp, &gq);
      if (L->lum_on) {
        const double d = rt_vr_lum((double)eq.c[0], (double)eq.c[1], (double)eq.c[2]) - lp;
        w = w / (1.0 + (d * d) * inv);
      }
      sumw += w;
      s0 += w * (double)eq.c[0];
      s1 += w * (double)eq.c[1];
      s2 += w * (double)eq.c[2];
      sumv += (w * w) * (double)eq.var;
    }
  }
  rt_vr_color o = ep;
  if (sumw > 0) {
    o.c[0] = (float)(s0 / sumw);
    o.c[1] = (float)(s1 / sumw);
    o.c[2] = (float)(s2 / sumw);
    o.var = (float)(sumv / (sumw * sumw));
  }
  return o;
}

/* Output of pixel p from e_L: rt_dn_finish's. */
RT_VARIANCE_FN void rt_vr_finish(const rt_vr_color* eL, int valid, const float* color, const float* albedo, size_t p,
                                 float out[3]) {
  rt_dn_color t;
  t.c[0] = eL->c[0];
  t.c[1] = eL->c[1];
  t.c[2] = eL->c[2];
  t.id = 0;
  rt_dn_finish(&t, valid, color, albedo, p, out);
}

#endif /* RT_VARIANCE_H */
