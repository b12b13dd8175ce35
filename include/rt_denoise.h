/*
 * rt_denoise.h — the à-trous denoiser guided by the first-hit feature buffers
 * (the definition is in include/rt_api.h at rt_denoise_async),
 * as inline functions shared by the device kernels that apply it
 * (rt_denoise.hip) and the host entry point that runs it without a device
 * (rt_denoise_host, rt_denoise_host.cpp): one pixel's records, one tap's
 * weight, one pixel of one level, one pixel's output.
 *
 * Binary64 `+ - * /` and comparisons only, in a fixed order, on values widened
 * from binary32: host and device agree to the bit under -ffp-contract=off.  No
 * address depends on a pixel's value.
 */
#ifndef RT_DENOISE_H
#define RT_DENOISE_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RT_DENOISE_FN __host__ __device__ static inline
#else
#define RT_DENOISE_FN static inline
#endif

/* The two 16-byte records of a pixel: a tap reads one of each.  The colour
 * record ping-pongs between two buffers from level to level and carries the
 * object id along (0 everywhere when no ids are given: no tap is stopped); the
 * guide record is written once.  A pixel is valid when its z is finite. */
typedef struct __attribute__((aligned(16))) {
  float c[3];   /* e_i(p): the (demodulated) colour after i levels */
  int32_t id;   /* object[p], or 0 */
} rt_dn_color;
typedef struct __attribute__((aligned(16))) {
  float n[3];   /* normal[p] */
  float z;      /* depth[p] */
} rt_dn_guide;

#define RT_DN_AMIN 0.015625 /* 2^-6: the least albedo a colour is divided by */

/* One level's constants, derived from rt_denoise by rt_dn_level_of(). */
typedef struct {
  int32_t W, H;
  int32_t step;      /* 2^i */
  int32_t nsq;       /* log2(normal_power); -1: the normal weight is off */
  int32_t depth_on;  /* sigma_depth > 0 */
  int32_t color_on;  /* sigma_color > 0 */
  double sigma_depth;
  double sc2;        /* sc * sc with sc = sigma_color * 2^-i */
} rt_dn_level;

RT_DENOISE_FN rt_dn_level rt_dn_level_of(int32_t W, int32_t H, int32_t level, int32_t normal_power, double sigma_color,
                                         double sigma_depth) {
  rt_dn_level L;
  L.W = W;
  L.H = H;
  L.step = (int32_t)1 << level;
  L.nsq = -1;
  for (int32_t j = 0; j < 8; ++j)
    if (normal_power == ((int32_t)1 << j)) L.nsq = j;
  L.depth_on = sigma_depth > 0;
  L.color_on = sigma_color > 0;
  L.sigma_depth = sigma_depth;
  const double sc = sigma_color * (1.0 / (double)((int32_t)1 << level)); /* exact: a power of two */
  L.sc2 = sc * sc;
  return L;
}

RT_DENOISE_FN int rt_dn_valid(float z) { return __builtin_isfinite(z) ? 1 : 0; }
RT_DENOISE_FN double rt_dn_floor_albedo(float a) { return (double)a > RT_DN_AMIN ? (double)a : RT_DN_AMIN; }
RT_DENOISE_FN double rt_dn_h(int32_t d) { /* h[|d|] = {3/8, 1/4, 1/16} */
  const int32_t a = d < 0 ? -d : d;
  return a == 0 ? 0.375 : (a == 1 ? 0.25 : 0.0625);
}

/* Prepare: pixel p's records.  albedo NULL: no demodulation; object NULL: id 0. */
RT_DENOISE_FN void rt_dn_prepare(const float* color, const float* albedo, const float* normal, const float* depth,
                                 const int32_t* object, size_t p, rt_dn_color* e, rt_dn_guide* g) {
  for (int k = 0; k < 3; ++k) {
    const float c = color[p * 3 + k];
    e->c[k] = albedo ? (float)((double)c / rt_dn_floor_albedo(albedo[p * 3 + k])) : c;
    g->n[k] = normal[p * 3 + k];
  }
  e->id = object ? object[p] : 0;
  g->z = depth[p];
}

/* The weight of the tap (dx, dy) of pixel p on its neighbour q (both valid,
 * same id): steps 1 to 4 of the definition, in its order of operations. */
RT_DENOISE_FN double rt_dn_tap_weight(const rt_dn_level* L, int32_t dx, int32_t dy, const rt_dn_color* ep,
                                      const rt_dn_guide* gp, const rt_dn_color* eq, const rt_dn_guide* gq) {
  double w = rt_dn_h(dx) * rt_dn_h(dy);
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
  if (L->color_on) {
    const double d0 = (double)eq->c[0] - (double)ep->c[0], d1 = (double)eq->c[1] - (double)ep->c[1],
                 d2 = (double)eq->c[2] - (double)ep->c[2];
    const double dd = (d0 * d0 + d1 * d1) + d2 * d2;
    w = w / (1.0 + dd / L->sc2);
  }
  return w;
}

/* One level for pixel (x, y): e_{i+1}(p) from the records of level i.  The 25
 * taps in the definition's order (dy outer, dx inner), binary64 sums per pixel.
 * Every index is computed from coordinates and bounds alone. */
RT_DENOISE_FN rt_dn_color rt_dn_level_pixel(const rt_dn_level* L, const rt_dn_color* e, const rt_dn_guide* g, int32_t x,
                                            int32_t y) {
  const size_t p = (size_t)y * (size_t)L->W + (size_t)x;
  const rt_dn_color ep = e[p];
  const rt_dn_guide gp = g[p];
  if (!rt_dn_valid(gp.z)) return ep;
  double sumw = 0, s0 = 0, s1 = 0, s2 = 0;
  for (int32_t dy = -2; dy <= 2; ++dy) {
    const int32_t qy = y + L->step * dy;
    if (qy < 0 || qy >= L->H) continue;
    for (int32_t dx = -2; dx <= 2; ++dx) {
      const int32_t qx = x + L->step * dx;
      if (qx < 0 || qx >= L->W) continue;
      const size_t q = (size_t)qy * (size_t)L->W + (size_t)qx;
      const rt_dn_guide gq = g[q];
      const rt_dn_color eq = e[q];
      if (!rt_dn_valid(gq.z) || eq.id != ep.id) continue;
      const double w = rt_dn_tap_weight(L, dx, dy, &ep, &gp, &eq, &gq);
      sumw += w;
      s0 += w * (double)eq.c[0];
      s1 += w * (double)eq.c[1];
      s2 += w * (double)eq.c[2];
    }
  }
  rt_dn_color o = ep;
  if (sumw > 0) {
    o.c[0] = (float)(s0 / sumw);
    o.c[1] = (float)(s1 / sumw);
    o.c[2] = (float)(s2 / sumw);
  }
  return o;
}

/* Output of pixel p from e_L: remodulated when albedo is given, the input
 * colour bit for bit when p is not valid.  color[p] is read before out is
 * written, so out may be color. */
RT_DENOISE_FN void rt_dn_finish(const rt_dn_color* eL, int valid, const float* color, const float* albedo, size_t p,
                                float out[3]) {
  for (int k = 0; k < 3; ++k) {
    if (!valid)
      out[k] = color[p * 3 + k];
    else
      out[k] = albedo ? (float)((double)eL->c[k] * rt_dn_floor_albedo(albedo[p * 3 + k])) : eL->c[k];
  }
}

#endif /* RT_DENOISE_H */
