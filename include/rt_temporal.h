/*
 * rt_temporal.h — temporal accumulation over a camera sequence (DESIGN.md
 * §4.14; the definition is in include/rt_api.h at rt_temporal_async), as inline
 * functions shared by the device kernel that applies it (rt_temporal.hip) and
 * the host entry point that runs it without a device (rt_temporal_host,
 * rt_temporal_host.cpp): the per-call constants, and one pixel in, its colour
 * and history length out.
 *
 * Binary64 `+ - * /`, comparisons and floor only, in a fixed order, on values
 * widened from binary32: host and device agree to the bit under
 * -ffp-contract=off.  Every address comes from the pixel's coordinates and
 * from integers that were compared against the image's bounds first, never
 * from a pixel's value alone.
 */
#ifndef RT_TEMPORAL_H
#define RT_TEMPORAL_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RT_TEMPORAL_FN __host__ __device__ static inline
#else
#define RT_TEMPORAL_FN static inline
#endif

/* One frame's buffers in image layout (pixel (x, y) at y * W + x). */
typedef struct {
  const float* color;    /* W*H*3 */
  const float* depth;    /* W*H */
  const int32_t* object; /* W*H or NULL */
  const float* normal;   /* W*H*3 or NULL */
  const float* count;    /* W*H, the previous frame's only */
} rt_tp_buffers;

/* One call's constants: the parameters, the current frame's vectors and what
 * the previous camera contributes (rt_tp_constants_of). */
typedef struct {
  int32_t W, H;
  int32_t has_prev; /* 0: every valid pixel starts a history */
  int32_t _pad;
  double max_history, depth_tol, normal_min, min_weight;
  double o[3], l[3], h[3], v[3]; /* the current frame: origin, lower_left, horizontal, vertical */
  double po[3];                  /* o' */
  double g[3];                   /* l' - o' */
  double a[3];                   /* (g + h' * 0.5) + v' * 0.5: the previous view axis */
  double ph[3], pv[3];           /* h', v' */
  double aa, hh, vv;             /* dot(a, a), dot(h', h'), dot(v', v') */
} rt_tp_constants;

RT_TEMPORAL_FN double rt_tp_dot(const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
RT_TEMPORAL_FN int rt_tp_finite(double v) { return __builtin_isfinite(v) ? 1 : 0; }
RT_TEMPORAL_FN int rt_tp_valid(float z) { return __builtin_isfinite(z) ? 1 : 0; }

/* The parameter rules of rt_temporal: 1 when all four are in range. */
RT_TEMPORAL_FN int rt_tp_params_ok(double max_history, double depth_tol, double normal_min, double min_weight) {
  if (!(rt_tp_finite(max_history) && max_history >= 1)) return 0;
  if (!(rt_tp_finite(depth_tol) && depth_tol >= 0)) return 0;
  if (!(normal_min >= -1 && normal_min <= 1)) return 0;
  return min_weight > 0 && min_weight <= 1;
}

/* The per-call constants from the parameters and the frames (prev_frame NULL:
 * no previous frame).  Returns 1, or 0 when a frame double is not finite or
 * aa, hh or vv is not > 0 (C is then not to be used). */
RT_TEMPORAL_FN int rt_tp_constants_of(rt_tp_constants* C, int32_t W, int32_t H, double max_history, double depth_tol,
                                      double normal_min, double min_weight, const double cur_frame[12],
                                      const double* prev_frame) {
  C->W = W;
  C->H = H;
  C->has_prev = prev_frame ? 1 : 0;
  C->_pad = 0;
  C->max_history = max_history;
  C->depth_tol = depth_tol;
  C->normal_min = normal_min;
  C->min_weight = min_weight;
  for (int k = 0; k < 12; ++k)
    if (!rt_tp_finite(cur_frame[k])) return 0;
  for (int k = 0; k < 3; ++k) {
    C->o[k] = cur_frame[k];
    C->l[k] = cur_frame[3 + k];
    C->h[k] = cur_frame[6 + k];
    C->v[k] = cur_frame[9 + k];
    C->po[k] = C->g[k] = C->a[k] = C->ph[k] = C->pv[k] = 0;
  }
  C->aa = C->hh = C->vv = 1;
  if (!prev_frame) return 1;
  for (int k = 0; k < 12; ++k)
    if (!rt_tp_finite(prev_frame[k])) return 0;
  for (int k = 0; k < 3; ++k) {
    C->po[k] = prev_frame[k];
    C->ph[k] = prev_frame[6 + k];
    C->pv[k] = prev_frame[9 + k];
    C->g[k] = prev_frame[3 + k] - prev_frame[k];
    C->a[k] = (C->g[k] + C->ph[k] * 0.5) + C->pv[k] * 0.5;
  }
  C->aa = rt_tp_dot(C->a, C->a);
  C->hh = rt_tp_dot(C->ph, C->ph);
  C->vv = rt_tp_dot(C->pv, C->pv);
  return (C->aa > 0 && C->hh > 0 && C->vv > 0) ? 1 : 0;
}

/* Pixel (x, y) of the image, 0 <= x < W and 0 <= y < H: steps 1 to 6 of the
 * definition in its order of operations.  prev is read only when C->has_prev.
 * out[3] and *out_count are the values to store. */
RT_TEMPORAL_FN void rt_tp_pixel(const rt_tp_constants* C, const rt_tp_buffers* cur, const rt_tp_buffers* prev, int32_t x,
                                int32_t y, float out[3], float* out_count) {
  const size_t W = (size_t)C->W;
  const size_t p = (size_t)y * W + (size_t)x;
  const float c0 = cur->color[p * 3 + 0], c1 = cur->color[p * 3 + 1], c2 = cur->color[p * 3 + 2];
  const float zf = cur->depth[p];
  out[0] = c0;
  out[1] = c1;
  out[2] = c2;
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
  double sumw = 0, s0 = 0, s1 = 0, s2 = 0, sumn = 0;
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
}

#endif /* RT_TEMPORAL_H */
