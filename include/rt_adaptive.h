/*
 * rt_adaptive.h — the stop rule of an adaptive progression,
 * one inline function shared by the device kernel that applies it
 * (adaptive_update_kernel, rt_adaptive.hip) and the host entry point that
 * restates it for one pixel (rt_adaptive_step, include/rt_api.h).
 *
 * Integers only: the rule reads a pixel's displayed RGBA8 before and after an
 * add, its sample count and its streak, and nothing of any other pixel, so
 * which pixel stops when is the same for every partition, rank count and path.
 */
#ifndef RT_ADAPTIVE_H
#define RT_ADAPTIVE_H

#include <stdint.h>

#if defined(__HIPCC__)
#define RT_ADAPTIVE_FN __host__ __device__ static inline
#else
#define RT_ADAPTIVE_FN static inline
#endif

/* One active pixel after an add.  old_rgba / new_rgba: its displayed pixel
 * before and after, four bytes in one word (any byte order, the same in
 * both); had_image: it had samples before this add (count - n > 0); count:
 * its samples including this add's; streak: adds in a row so far whose
 * largest byte difference was <= tolerance.  Rule 3: with an earlier image,
 * d = max over the four bytes |new - old| and the streak grows by one when
 * d <= tolerance, else falls to 0; without one it stays as it is.  Rule 4:
 * the pixel stops (returns 1) when streak >= patience and count >=
 * min_samples.  *new_streak receives the streak after rule 3. */
RT_ADAPTIVE_FN int rt_adaptive_rule(uint32_t old_rgba, uint32_t new_rgba, int32_t had_image, int32_t count,
                                    int32_t streak, int32_t tolerance, int32_t patience, int32_t min_samples,
                                    int32_t* new_streak) {
  if (had_image) {
    int32_t d = 0;
    for (int c = 0; c < 4; ++c) {
      const int32_t a = (int32_t)((old_rgba >> (8 * c)) & 255u), b = (int32_t)((new_rgba >> (8 * c)) & 255u);
      const int32_t e = a > b ? a - b : b - a;
      d = e > d ? e : d;
    }
    streak = d <= tolerance ? streak + 1 : 0;
  }
  *new_streak = streak;
  return streak >= patience && count >= min_samples ? 1 : 0;
}

#endif /* RT_ADAPTIVE_H */
