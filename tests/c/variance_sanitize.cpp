// variance_sanitize.cpp — the per-pixel functions of variance-guided denoising
// (include/rt_variance.h) over adversarial inputs, as a
// stand-alone program for -fsanitize=address,undefined (tests/test_variance_cpu.py
// compiles and runs it).  Every buffer is a heap allocation of exactly the
// image's size, so a tap outside the image is an error the sanitizer reports;
// the values that come out carry no contract and are only summed, so that
// nothing is optimised away.
#include <math.h>
#include <stdio.h>

#include <vector>

#include "rt_variance.h"

namespace {

const float kInf = INFINITY, kNan = NAN;

struct Image {
  int32_t w, h;
  std::vector<float> color, albedo, depth, normal, count, moments, variance;
  std::vector<int32_t> object;
  Image(int32_t w_, int32_t h_, unsigned seed) : w(w_), h(h_) {
    const size_t n = (size_t)w * (size_t)h;
    color.resize(n * 3);
    albedo.resize(n * 3);
    depth.resize(n);
    normal.resize(n * 3);
    count.resize(n);
    moments.resize(n * 2);
    variance.resize(n);
    object.resize(n);
    // adversarial values in a fixed rotation: NaN, +-Inf, zero, negative, huge, denormal, ordinary
    const float vals[] = {kNan, kInf, -kInf, 0.0f, -0.0f, -2.5f, 3.0e38f, 1.0e-42f, 1.0f, 2.0f, 0.5f, 1.75f};
    const unsigned nv = sizeof vals / sizeof vals[0];
    unsigned s = seed;
    auto next = [&]() { return vals[((s = s * 1664525u + 1013904223u) >> 16) % nv]; };
    for (auto* v : {&color, &albedo, &depth, &normal, &count, &moments, &variance})
      for (auto& x : *v) x = next();
    for (auto& v : object) v = (int32_t)((s = s * 1664525u + 1013904223u) >> 30) - 1;
  }
  rt_tp_buffers frame(bool guides) const {
    rt_tp_buffers b;
    b.color = color.data();
    b.depth = depth.data();
    b.object = guides ? object.data() : nullptr;
    b.normal = guides ? normal.data() : nullptr;
    b.count = count.data();
    return b;
  }
};

double add(double sum, float v) { return isfinite(v) ? sum + v : sum; }

// the moments pass: a static camera, a camera behind the point, absurd frames (temporal_sanitize.cpp's)
double run_moments(int32_t w, int32_t h, const double cur_frame[12], const double* prev_frame, unsigned seed) {
  const Image cur(w, h, seed), prev(w, h, seed + 77u);
  double sum = 0;
  for (int guides = 0; guides < 2; ++guides)
    for (int alb = 0; alb < 2; ++alb) {
      rt_tp_constants C;
      if (!rt_tp_constants_of(&C, w, h, 32.0, guides ? 0.05 : 0.0, guides ? 0.9 : -1.0, 0.25, cur_frame, prev_frame))
        continue;
      const rt_tp_buffers bc = cur.frame(guides != 0), bp = prev.frame(guides != 0);
      for (int32_t y = 0; y < h; ++y)
        for (int32_t x = 0; x < w; ++x) {
          float out[3], n, m[2];
          rt_vr_tp_pixel(&C, &bc, &bp, alb ? cur.albedo.data() : nullptr, prev_frame ? prev.moments.data() : nullptr,
                         x, y, out, &n, m);
          for (int k = 0; k < 3; ++k) sum = add(sum, out[k]);
          sum = add(add(add(sum, n), m[0]), m[1]);
        }
    }
  return sum;
}

// the variance pass and every level of the filter, each mechanism on and off
double run_spatial(int32_t w, int32_t h, unsigned seed) {
  const Image im(w, h, seed);
  const size_t npix = (size_t)w * (size_t)h;
  double sum = 0;
  for (int mode = 0; mode < 8; ++mode) {
    const bool guides = mode & 1, mom = mode & 2, alb = mode & 4;
    rt_vr_buffers B;
    B.color = im.color.data();
    B.normal = im.normal.data();
    B.depth = im.depth.data();
    B.albedo = alb ? im.albedo.data() : nullptr;
    B.object = guides ? im.object.data() : nullptr;
    B.moments = mom ? im.moments.data() : nullptr;
    B.count = mom ? im.count.data() : nullptr;
    for (const double min_history : {1.0, 4.0, 1e9}) {
      const rt_dn_level L = rt_dn_level_of(w, h, 0, guides ? 32 : 0, 0.0, guides ? 0.05 : 0.0);
      for (int32_t y = 0; y < h; ++y)
        for (int32_t x = 0; x < w; ++x) sum = add(sum, rt_vr_variance_pixel(&L, min_history, &B, x, y));
    }
    std::vector<rt_vr_color> e[2] = {std::vector<rt_vr_color>(npix), std::vector<rt_vr_color>(npix)};
    std::vector<rt_dn_guide> g(npix);
    std::vector<int32_t> id(npix);
    for (size_t p = 0; p < npix; ++p)
      rt_vr_prepare(B.color, B.albedo, B.normal, B.depth, B.object, im.variance.data(), p, &e[0][p], &g[p], &id[p]);
    for (int32_t i = 0; i < 8; ++i) {  // steps 1 .. 128: past every image here
      const rt_vr_level L = rt_vr_level_of(w, h, i, guides ? 32 : 0, mom ? 4.0 : 0.0, guides ? 0.05 : 0.0, alb ? 1 : 0);
      for (int32_t y = 0; y < h; ++y)
        for (int32_t x = 0; x < w; ++x)
          e[(i & 1) ^ 1][(size_t)y * (size_t)w + (size_t)x] =
              rt_vr_level_pixel(&L, e[i & 1].data(), g.data(), id.data(), x, y);
    }
    for (size_t p = 0; p < npix; ++p) {
      float out[3];
      rt_vr_finish(&e[0][p], rt_dn_valid(g[p].z), B.color, B.albedo, p, out);
      for (int k = 0; k < 3; ++k) sum = add(sum, out[k]);
      sum = add(sum, e[0][p].var);
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
  const int32_t sizes[][2] = {{1, 1}, {3, 2}, {7, 5}, {33, 17}, {70, 3}};
  for (const auto& wh : sizes) {
    const int32_t w = wh[0], h = wh[1];
    double f[12];
    sum += run_moments(w, h, base, nullptr, 100u + (unsigned)runs++);  // no previous frame
    sum += run_moments(w, h, base, base, 100u + (unsigned)runs++);     // a static camera over absurd depths
    for (int k = 0; k < 12; ++k) f[k] = base[k];
    f[2] = -50;  // a previous camera behind the point
    f[5] = -51;
    sum += run_moments(w, h, base, f, 100u + (unsigned)runs++);
    for (const double big : {1e300, -1e300}) {  // frames that send fx and fy to +-1e300
      for (int k = 0; k < 12; ++k) f[k] = base[k];
      f[3] = big;
      f[4] = -big;
      f[6] = 1e-300;
      f[10] = 1e-300;
      sum += run_moments(w, h, base, f, 100u + (unsigned)runs++);
      sum += run_moments(w, h, f, base, 100u + (unsigned)runs++);
    }
    for (int k = 0; k < 12; ++k) f[k] = base[k];
    f[0] = 0.37;  // a sheared frame whose taps straddle every edge and corner
    f[1] = -0.21;
    f[7] = 0.9;
    f[9] = -0.7;
    sum += run_moments(w, h, base, f, 100u + (unsigned)runs++);
    for (unsigned s = 0; s < 3; ++s) sum += run_spatial(w, h, 500u + s + (unsigned)runs++);
  }
  // rejected parameters stay rejected
  const int refused = !rt_vr_params_ok(NAN, 32, 0.05) + !rt_vr_params_ok(0.5, 32, 0.05) + !rt_vr_params_ok(4, 3, 0.05) +
                      !rt_vr_params_ok(4, 32, -1) + !rt_vr_filter_params_ok(0, 32, 2, 0.05, 1, 1) +
                      !rt_vr_filter_params_ok(4, 32, NAN, 0.05, 1, 1) + !rt_vr_filter_params_ok(4, 32, 2, 0.05, 1, 2);
  if (refused != 7 || !rt_vr_params_ok(4, 32, 0.05) || !rt_vr_filter_params_ok(4, 32, 2, 0.05, 1, 1)) {
    printf("variance_sanitize: the parameter rules changed (%d)\n", refused);
    return 1;
  }
  printf("variance_sanitize ok: %d runs, sum %g\n", runs, sum);
  return 0;
}
