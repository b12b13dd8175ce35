// matte_sanitize.cpp — the slot insert, the ranking and the per-pixel edge
// resolve (include/rt_matte.h) over adversarial inputs, as a
// stand-alone program for -fsanitize=address,undefined
// (tests/test_matte_cpu.py compiles and runs it).  Every buffer is a heap
// allocation of exactly its size -- the slot columns too, in the kernel's
// strided layout -- so a slot past the sixteenth, a tap outside the image or an
// address taken from an id or a count is an error the sanitizer reports.  The
// walk's results are checked against a plain restatement; the resolve's values
// carry no contract and are only summed, so that nothing is optimised away.
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <vector>

#include "rt_matte.h"

namespace {

unsigned g_seed = 12345u;
unsigned next_u() { return (g_seed = g_seed * 1664525u + 1013904223u) >> 8; }

int fail(const char* what, int a, int b) {
  printf("matte_sanitize FAILED: %s (%d, %d)\n", what, a, b);
  return 1;
}

// One pixel's walk over `n` keys drawn from `distinct` values, in columns of `stride` words of which this
// pixel's is `lane`, against a map and a sort.
int walk_case(int n, int distinct, int32_t stride, int32_t lane, int32_t K) {
  std::vector<int32_t> key((size_t)(RT_MT_SLOTS - 1) * stride + lane + 1), count(key.size());
  std::vector<int32_t> order;  // first appearance
  std::map<int32_t, int32_t> seen;
  rt_mt_state st;
  rt_mt_begin(&st);
  int overflow = 0;
  for (int s = 0; s < n; ++s) {
    // keys at the extremes too: the face level's largest, 0, and a negative one (no contract excludes it here)
    const int32_t pool[] = {0, INT32_MAX, -5, ((1 << 27) - 1) * 16 + 11};
    const unsigned u = next_u() % (unsigned)distinct;
    const int32_t k = u < 4 ? pool[u] : (int32_t)u * 7;
    rt_mt_insert(key.data() + lane, count.data() + lane, stride, &st, k);
    if (seen.count(k)) {
      seen[k] += 1;
    } else if ((int)order.size() < RT_MT_SLOTS) {
      order.push_back(k);
      seen[k] = 1;
    } else {
      overflow += 1;
    }
  }
  if (st.hits != n || st.overflow != overflow || st.used != (int32_t)order.size())
    return fail("walk state", st.hits, st.overflow);
  std::vector<std::pair<int32_t, int32_t>> want;  // (-count, key): count descending, key ascending
  for (int32_t k : order) want.push_back({-seen[k], k});
  std::sort(want.begin(), want.end());
  std::vector<int32_t> id((size_t)K), cnt((size_t)K);
  const int32_t rest = rt_mt_ranks(key.data() + lane, count.data() + lane, stride, &st, K, id.data(), cnt.data());
  int32_t sum = 0;
  for (int32_t r = 0; r < K; ++r) {
    const bool has = r < (int32_t)want.size();
    if (id[(size_t)r] != (has ? want[(size_t)r].second : -1) || cnt[(size_t)r] != (has ? -want[(size_t)r].first : 0))
      return fail("rank", r, id[(size_t)r]);
    sum += cnt[(size_t)r];
  }
  if (sum + rest != n) return fail("sum + rest == hits", sum, rest);
  return 0;
}

double resolve_case(int32_t w, int32_t h, int32_t K, int32_t n, int32_t R, bool with_rest) {
  const size_t np = (size_t)w * (size_t)h;
  std::vector<float> color(np * 3);
  std::vector<int32_t> object(np), id(np * (size_t)K), count(np * (size_t)K), rest(np);
  const float vals[] = {NAN, INFINITY, -INFINITY, 0.0f, -0.0f, -2.5f, 3.0e38f, 1.0e-42f, 1.0f, 2.0f, 0.5f, 1.75f, 0.25f};
  const int32_t ids[] = {-1, 0, 1, 2, 3, 1000000, INT32_MAX, INT32_MIN, -2, 1, 0, 2, 1};
  const int32_t counts[] = {0, 1, 2, 3, n, n - 1, n + 5, -1, INT32_MAX, INT32_MIN, 1, 0, 4};
  for (auto& v : color) v = vals[next_u() % 13];
  for (auto& v : object) v = ids[next_u() % 13];
  for (auto& v : id) v = ids[next_u() % 13];
  for (auto& v : count) v = counts[next_u() % 13];
  for (auto& v : rest) v = counts[next_u() % 13];
  rt_mt_resolve_params P;
  P.W = w;
  P.H = h;
  P.K = K;
  P.n = n;
  P.R = R;
  P.has_rest = with_rest ? 1 : 0;
  P.bg[0] = 0.25;
  P.bg[1] = 0;
  P.bg[2] = -1e300;
  double sum = 0;
  int mixed = 0;
  for (int32_t y = 0; y < h; ++y)
    for (int32_t x = 0; x < w; ++x) {  // every pixel: the corners and edges are where a window leaves the image
      float out[3] = {0, 0, 0};
      if (rt_mt_resolve_pixel(&P, color.data(), object.data(), id.data(), count.data(),
                              with_rest ? rest.data() : nullptr, x, y, out)) {
        mixed += 1;
        for (int k = 0; k < 3; ++k)
          if (out[k] == out[k] && fabs((double)out[k]) < 1e30) sum += out[k];
      }
    }
  return sum + mixed;
}

}  // namespace

int main() {
  // the walk: fewer keys than slots, exactly 16, more (overflow), one key, no sample; the kernel's stride and 1
  const int ns[] = {0, 1, 2, 17, 64, 200};
  const int ds[] = {1, 3, 16, 17, 40};
  for (int n : ns)
    for (int d : ds)
      for (int32_t K = 1; K <= RT_MT_MAX_RANKS; K += (K == 1 ? 3 : 4)) {
        if (walk_case(n, d, 1, 0, K)) return 1;
        if (walk_case(n, d, 64, 63, K)) return 1;
        if (walk_case(n, d, 64, 0, K)) return 1;
      }
  // the resolve: a single pixel, images smaller than the window at radius 4, a row, a column, ordinary ones
  const int32_t sizes[][2] = {{1, 1}, {2, 2}, {5, 3}, {9, 1}, {1, 9}, {17, 11}};
  double sum = 0;
  for (const auto& s : sizes)
    for (int32_t R = 1; R <= RT_MT_MAX_RADIUS; ++R)
      for (int32_t K : {1, 4, 8})
        for (int32_t n : {1, 8, 1 << 24}) {
          sum += resolve_case(s[0], s[1], K, n, R, true);
          sum += resolve_case(s[0], s[1], K, n, R, false);
        }
  double bg[3] = {0, 0, 0};
  if (!rt_mt_resolve_ok(4, 16, 2, bg) || rt_mt_resolve_ok(0, 16, 2, bg) || rt_mt_resolve_ok(9, 16, 2, bg) ||
      rt_mt_resolve_ok(4, 0, 2, bg) || rt_mt_resolve_ok(4, 16, 0, bg) || rt_mt_resolve_ok(4, 16, 5, bg))
    return fail("parameter rules", 0, 0);
  bg[1] = NAN;
  if (rt_mt_resolve_ok(4, 16, 2, bg)) return fail("a NaN background", 0, 0);
  bg[1] = INFINITY;
  if (rt_mt_resolve_ok(4, 16, 2, bg)) return fail("an infinite background", 0, 0);
  printf("matte_sanitize ok (%g)\n", sum);
  return 0;
}
