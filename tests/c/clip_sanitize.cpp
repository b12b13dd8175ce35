// clip_sanitize.cpp — the per-pixel functions of temporal accumulation with
// history rectification (include/rt_clip.h) over adversarial
// inputs, as a stand-alone program for -fsanitize=address,undefined
// (tests/test_clip_cpu.py compiles and runs it).  Every buffer, the motion
// table included, is a heap allocation of exactly its size, so a window tap or
// a bilinear tap outside the image, or a table row taken from an id out of
// range, is an error the sanitizer reports; the values that come out carry no
// contract and are only summed, so that nothing is optimised away.
#include <math.h>
#include <stdio.h>

#include <vector>

#include "rt_clip.h"

namespace {

const float kInf = INFINITY, kNan = NAN;

struct Image {
  int32_t w, h;
  std::vector<float> color, depth, normal, count, albedo, moments;
  std::vector<int32_t> object;
  Image(int32_t w_, int32_t h_, unsigned seed) : w(w_), h(h_) {
    const size_t n = (size_t)w * (size_t)h;
    color.resize(n * 3);
    depth.resize(n);
    normal.resize(n * 3);
    count.resize(n);
    albedo.resize(n * 3);
    moments.resize(n * 2);
    object.resize(n);
    // adversarial values in a fixed rotation: NaN, +-Inf, zero, negative, huge, denormal, ordinary (ordinary
    // ones more often, so that windows fill up and histories are found)
    const float vals[] = {kNan, kInf, -kInf, 0.0f, -0.0f, -2.5f, 3.0e38f, 1.0e-42f, 1.0f, 2.0f, 0.5f, 1.75f,
                          2.0f, 2.0f, 1.5f, 2.25f, 1.0f, 0.25f};
    const unsigned nv = sizeof vals / sizeof vals[0];
    unsigned s = seed;
    auto next = [&]() { return vals[((s = s * 1664525u + 1013904223u) >> 16) % nv]; };
    for (auto& v : color) v = next();
    for (auto& v : depth) v = next();
    for (auto& v : normal) v = next();
    for (auto& v : count) v = next();
    for (auto& v : albedo) v = next();
    for (auto& v : moments) v = next();
    // ids in and out of every table below: -1 and the extremes, 0..3, one past, far past
    const int32_t ids[] = {-1, 0, 1, 2, 3, 4, 5, 1000000, INT32_MAX, INT32_MIN, -2, 1, 0, 2, 1, 1, 1, 0};
    const unsigned ni = sizeof ids / sizeof ids[0];
    for (auto& v : object) v = ids[((s = s * 1664525u + 1013904223u) >> 16) % ni];
  }
  rt_tp_buffers buffers(bool normals, bool objects) const {
    rt_tp_buffers b;
    b.color = color.data();
    b.depth = depth.data();
    b.object = objects ? object.data() : nullptr;
    b.normal = normals ? normal.data() : nullptr;
    b.count = count.data();
    return b;
  }
};

// a table of exactly `rows` rows: ordinary translations, then non-finite and huge entries
std::vector<double> table_of(int rows, bool adversarial) {
  const double plain[] = {0.12, 0.05, -0.04, -0.10, 0.08, 0.06, 0.0, -0.0, 0.0};
  const double bad[] = {NAN, 1.0, INFINITY, -INFINITY, 1e300, -1e300, 5e-324, NAN, NAN};
  std::vector<double> t((size_t)rows * 3);
  for (size_t k = 0; k < t.size(); ++k) t[k] = adversarial ? bad[k % 9] : plain[k % 9];
  return t;
}

long clipped_total = 0, history_total = 0;

double run(int32_t w, int32_t h, const double cur_frame[12], const double* prev_frame, double depth_tol,
           double normal_min, unsigned seed) {
  const Image cur(w, h, seed), prev(w, h, seed + 77u);
  double sum = 0;
  // radius 0 (off) to 4, every one larger than the smallest images; a gamma of 0 and a huge one; min_taps 1 and many
  const rt_cl_params clips[] = {{0, 1, 1.0, 0.0}, {1, 1, 0.0, 0.0}, {2, 5, 1.0, 0.0}, {3, 1, 1e300, 1e300},
                                {4, 81, 0.5, 0.25}, {4, 2, 2.0, 0.0}};
  for (int rows = 0; rows <= 4; rows += 2)  // no table, two rows (ids 2.. are out of range) and four
    for (int adversarial = 0; adversarial < (rows ? 2 : 1); ++adversarial) {
      const std::vector<double> table = table_of(rows, adversarial != 0);
      for (int flags = 0; flags < 4; ++flags) {
        const bool normals = (flags & 1) != 0, objects = rows > 0 || (flags & 2) != 0;
        rt_tp_constants C;
        if (!rt_tp_constants_of(&C, w, h, 32.0, depth_tol, normal_min, 0.25, cur_frame, prev_frame)) continue;
        const rt_tp_buffers bc = cur.buffers(normals, objects), bp = prev.buffers(normals, objects);
        for (const rt_cl_params& K : clips)
          for (int32_t y = 0; y < h; ++y)
            for (int32_t x = 0; x < w; ++x) {
              float out[3], n, m[2] = {0, 0}, cl;
              rt_cl_pixel(0, &C, &K, &bc, &bp, rows ? table.data() : nullptr, rows, normals ? cur.albedo.data() : nullptr,
                          nullptr, x, y, out, &n, m, &cl);
              for (int k = 0; k < 3; ++k)
                if (isfinite(out[k])) sum += out[k];
              if (isfinite(n)) sum += n;
              clipped_total += cl != 0;
              history_total += n > 1;
              rt_cl_pixel(1, &C, &K, &bc, &bp, rows ? table.data() : nullptr, rows, normals ? nullptr : cur.albedo.data(),
                          prev.moments.data(), x, y, out, &n, m, &cl);
              for (int k = 0; k < 3; ++k)
                if (isfinite(out[k])) sum += out[k];
              for (int k = 0; k < 2; ++k)
                if (isfinite(m[k])) sum += m[k];
              sum += cl;
            }
      }
    }
  return sum;
}

}  // namespace

int main() {
  // origin, lower_left, horizontal, vertical of a camera at (0, 0, 3) looking down -Z
  const double base[12] = {0, 0, 3, -2, -1, 2, 4, 0, 0, 0, 2, 0};
  double sum = 0;
  int runs = 0;
  auto go = [&](int32_t w, int32_t h, const double* cf, const double* pf) {
    for (const double tol : {0.05, 0.0})
      for (const double nmin : {0.9, -1.0}) {
        sum += run(w, h, cf, pf, tol, nmin, 4321u + (unsigned)runs);
        runs += 1;
      }
  };
  const int32_t sizes[][2] = {{1, 1}, {5, 3}, {7, 9}, {33, 17}, {70, 3}};
  for (const auto& wh : sizes) {
    const int32_t w = wh[0], h = wh[1];
    go(w, h, base, nullptr);  // no previous frame
    go(w, h, base, base);     // a static camera: NaN, infinite, zero and negative depths and colours
    double f[12];
    // a previous camera BEHIND the point: at z = -50, looking the same way (t < 0 for the depths around 2)
    for (int k = 0; k < 12; ++k) f[k] = base[k];
    f[2] = -50;
    f[5] = -51;
    go(w, h, base, f);
    // frames that send fx and fy to +-1e300: a tiny viewport far to either side
    for (const double big : {1e300, -1e300}) {
      for (int k = 0; k < 12; ++k) f[k] = base[k];
      f[3] = big;
      f[4] = -big;
      f[6] = 1e-300;
      f[10] = 1e-300;
      go(w, h, base, f);
    }
    // a sheared frame whose taps straddle every edge and corner
    for (int k = 0; k < 12; ++k) f[k] = base[k];
    f[0] = 0.37;
    f[1] = -0.21;
    f[7] = 0.9;
    f[9] = -0.7;
    go(w, h, base, f);
  }
  if (history_total < 1000 || clipped_total < 100) {  // (the window and the clip did run)
    printf("clip_sanitize: only %ld histories and %ld clips\n", history_total, clipped_total);
    return 1;
  }
  printf("clip_sanitize ok: %d runs, %ld histories, %ld clipped, sum %g\n", runs, history_total, clipped_total, sum);
  return 0;
}
