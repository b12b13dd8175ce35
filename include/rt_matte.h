/*
 * rt_matte.h — matte layers and the coverage-aware edge resolve (DESIGN.md
 * §4.19; the definitions are in include/rt_api.h at
 * rt_context_render_matte_async and rt_matte_resolve_async), as inline
 * functions shared by the device kernels (rt_matte.hip), the host entry point
 * that resolves without a device (rt_matte_resolve_host, rt_matte_host.cpp)
 * and the sanitizer program (tests/c/matte_sanitize.cpp).
 *
 * The slots of a pixel are two columns of RT_MT_SLOTS 32-bit words, key and
 * count, addressed as column[slot * stride]: the matte kernel keeps them in
 * LDS with stride 64 (one column per lane), a host caller in plain arrays with
 * stride 1.  The functions index them by data, which is why they are memory
 * and not registers.
 *
 * The resolve is binary64 `+ - * /` and comparisons only, in a fixed order, on
 * values widened from binary32 and integers: host and device agree to the bit
 * under -ffp-contract=off.  Every address comes from the pixel's coordinates,
 * the window's offsets, the rank index and bounds checks; an id or a count is
 * compared and converted, never used as an address.
 */
#ifndef RT_MATTE_H
#define RT_MATTE_H

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RT_MATTE_FN __host__ __device__ static inline __attribute__((always_inline))
#else
#define RT_MATTE_FN static inline __attribute__((always_inline))
#endif

#define RT_MT_SLOTS 16      /* RT_MATTE_SLOTS of rt_api.h */
#define RT_MT_MAX_RANKS 8
#define RT_MT_MAX_RADIUS 4

/* What a pixel's walk carries beside the two columns. */
typedef struct {
  int32_t used;     /* slots taken, 0..RT_MT_SLOTS */
  int32_t hits;     /* hitting samples */
  int32_t overflow; /* hitting samples that found neither their key nor a free slot */
} rt_mt_state;

RT_MATTE_FN void rt_mt_begin(rt_mt_state* s) {
  s->used = 0;
  s->hits = 0;
  s->overflow = 0;
}

/* One hitting sample with key k (samples come in ascending s): its slot's
 * count goes up, else it takes the next free slot with count 1, else it
 * overflows.  hits counts it in every case. */
RT_MATTE_FN void rt_mt_insert(int32_t* key, int32_t* count, int32_t stride, rt_mt_state* s, int32_t k) {
  s->hits += 1;
  for (int32_t i = 0; i < s->used; ++i)
    if (key[i * stride] == k) {
      count[i * stride] += 1;
      return;
    }
  if (s->used < RT_MT_SLOTS) {
    key[s->used * stride] = k;
    count[s->used * stride] = 1;
    s->used += 1;
  } else {
    s->overflow += 1;
  }
}

/* The next rank: of the slots not taken yet, the one with the largest count,
 * the smallest key among equal counts.  1 with its key and count, and the slot
 * marked taken (its count set to 0: a used slot's count is >= 1); 0 when none
 * is left.  K calls in a row give ranks 0..K-1. */
RT_MATTE_FN int rt_mt_take(const int32_t* key, int32_t* count, int32_t stride, const rt_mt_state* s, int32_t* out_key,
                           int32_t* out_count) {
  int32_t best = -1, bk = 0, bc = 0;
  for (int32_t i = 0; i < s->used; ++i) {
    const int32_t c = count[i * stride], k = key[i * stride];
    if (c > bc || (c == bc && c > 0 && k < bk)) {
      best = i;
      bk = k;
      bc = c;
    }
  }
  if (best < 0) return 0;
  count[best * stride] = 0;
  *out_key = bk;
  *out_count = bc;
  return 1;
}

/* Ranks 0..K-1 of a finished walk into id[r] / count[r] (-1 / 0 for an empty
 * rank); returns `rest` = hits - sum of the K counts (the dropped ranks and the
 * overflow).  The columns are consumed. */
RT_MATTE_FN int32_t rt_mt_ranks(const int32_t* key, int32_t* count, int32_t stride, const rt_mt_state* s, int32_t K,
                                int32_t* id, int32_t* cnt) {
  int32_t rest = s->hits;
  for (int32_t r = 0; r < K; ++r) {
    int32_t k = -1, c = 0;
    if (!rt_mt_take(key, count, stride, s, &k, &c)) {
      k = -1;
      c = 0;
    }
    id[r] = k;
    cnt[r] = c;
    rest -= c;
  }
  return rest;
}

/* ---- the edge resolve ---- */

/* rt_matte_resolve's fields and the call's integers, checked. */
typedef struct {
  int32_t W, H, K, n, R, has_rest;
  double bg[3];
} rt_mt_resolve_params;

RT_MATTE_FN int rt_mt_finite(double v) { return v - v == 0.0; }

/* The parameter rules of rt_matte_resolve_async: 1 when all are in range. */
RT_MATTE_FN int rt_mt_resolve_ok(int32_t K, int32_t n, int32_t R, const double bg[3]) {
  if (K < 1 || K > RT_MT_MAX_RANKS || n < 1 || R < 1 || R > RT_MT_MAX_RADIUS) return 0;
  return rt_mt_finite(bg[0]) && rt_mt_finite(bg[1]) && rt_mt_finite(bg[2]);
}

/* Step 2 for a rank or the miss part with `key`: the inverse-distance mean of
 * the window's taps whose object is key.  1 with part[3] when a tap counted. */
RT_MATTE_FN int rt_mt_gather(const rt_mt_resolve_params* P, const float* color, const int32_t* object, int32_t x,
                             int32_t y, int32_t key, double part[3]) {
  double sw = 0, sc[3] = {0, 0, 0};
  for (int32_t dy = -P->R; dy <= P->R; ++dy)
    for (int32_t dx = -P->R; dx <= P->R; ++dx) {
      const int32_t qx = x + dx, qy = y + dy;
      if (qx < 0 || qx >= P->W || qy < 0 || qy >= P->H) continue;
      const size_t q = (size_t)qy * (size_t)P->W + (size_t)qx;
      if (object[q] != key) continue;
      const double w = 1.0 / (1.0 + (double)(dx * dx + dy * dy));
      sw += w;
      for (int k = 0; k < 3; ++k) sc[k] += w * (double)color[q * 3 + k];
    }
  if (!(sw > 0)) return 0;
  for (int k = 0; k < 3; ++k) part[k] = sc[k] / sw;
  return 1;
}

/* Pixel (x, y), 0 <= x < W and 0 <= y < H: 0 when it has fewer than two parts
 * (the caller copies color[p]'s bits), else 1 with out[3].  id and count are K
 * planes of W * H, rest one plane or NULL. */
RT_MATTE_FN int rt_mt_resolve_pixel(const rt_mt_resolve_params* P, const float* color, const int32_t* object,
                                    const int32_t* id, const int32_t* count, const int32_t* rest, int32_t x, int32_t y,
                                    float out[3]) {
  const size_t plane = (size_t)P->W * (size_t)P->H, p = (size_t)y * (size_t)P->W + (size_t)x;
  const int64_t rs = (P->has_rest && rest) ? (int64_t)rest[p] : 0;
  int64_t sum = 0;
  int32_t parts = 0;
  for (int32_t r = 0; r < P->K; ++r) {
    const int32_t c = count[(size_t)r * plane + p];
    if (c > 0) {
      sum += c;
      parts += 1;
    }
  }
  const int64_t miss = (int64_t)P->n - sum - rs;
  if (miss > 0) parts += 1;
  if (rs > 0) parts += 1;
  if (parts < 2) return 0;
  const double n = (double)P->n;
  const double own[3] = {(double)color[p * 3 + 0], (double)color[p * 3 + 1], (double)color[p * 3 + 2]};
  double acc[3] = {0, 0, 0};
  for (int32_t r = 0; r < P->K; ++r) {
    const int32_t c = count[(size_t)r * plane + p];
    if (!(c > 0)) continue;
    double part[3];
    if (!rt_mt_gather(P, color, object, x, y, id[(size_t)r * plane + p], part))
      for (int k = 0; k < 3; ++k) part[k] = own[k];
    const double share = (double)c / n;
    for (int k = 0; k < 3; ++k) acc[k] += share * part[k];
  }
  if (miss > 0) {
    double part[3];
    if (!rt_mt_gather(P, color, object, x, y, -1, part))
      for (int k = 0; k < 3; ++k) part[k] = P->bg[k];
    const double share = (double)miss / n;
    for (int k = 0; k < 3; ++k) acc[k] += share * part[k];
  }
  if (rs > 0) {
    const double share = (double)rs / n;
    for (int k = 0; k < 3; ++k) acc[k] += share * own[k];
  }
  for (int k = 0; k < 3; ++k) out[k] = (float)acc[k];
  return 1;
}

#endif /* RT_MATTE_H */
