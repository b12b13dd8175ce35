// schedule.cpp — the per-tile inputs of the work schedule, on the host.
//
// The schedule itself (per-pixel masks, pilot render, blocks, dispatch
// order) is built on the GPU (rt_schedule.hip).  Its per-TILE inputs are
// cheap (tiles x primitives) and stay here:
//   - tile_primary_masks: the primitives whose bounding sphere meets the cone
//     of a tile's camera rays (the per-pixel masks refine these);
//   - tile_cost: primitives projected onto each tile, the work estimate of a
//     schedule built without a pilot render.
#include <math.h>

#include <algorithm>
#include <atomic>
#include <numeric>
#include <vector>

#include "rt_internal.h"

namespace rtgo {

void strided_tiles(int32_t W, int32_t H, int32_t rank, int32_t world, std::vector<int32_t>* tiles) {
  tiles->clear();
  const int ntiles = rt_num_tiles(W, H);
  for (int t = rank; t < ntiles; t += world) tiles->push_back(t);
}

// Look-at model: the same projection in camera coordinates.  The frame's
// horizontal = U * (2 a h), vertical = V * (2 h) and lower_left give back the
// unit axes U, V, w and the half-extents a h and h; a centre is (dot U, dot V,
// dot w) of its offset from the origin, and the camera looks down -w.
void tile_cost(const FlatScene& fs, const CamFrame& cf, int32_t W, int32_t H, const std::vector<int32_t>& tiles,
               std::vector<float>* local_cost) {
  const int tiles_x = (W + 31) / 32, tiles_y = (H + 31) / 32, ntiles = tiles_x * tiles_y;
  std::vector<float> cost(ntiles, 0.0f);
  const bool lookat = cf.model != RT_CAMERA_REFERENCE;
  double U[3] = {1, 0, 0}, V[3] = {0, 1, 0}, Wv[3] = {0, 0, 1}, vh = 2.0;
  double vw = cf.h[0];
  if (lookat) {
    vw = sqrt(cf.h[0] * cf.h[0] + cf.h[1] * cf.h[1] + cf.h[2] * cf.h[2]);
    vh = sqrt(cf.v[0] * cf.v[0] + cf.v[1] * cf.v[1] + cf.v[2] * cf.v[2]);
    for (int k = 0; k < 3; ++k) {
      U[k] = cf.h[k] / vw;
      V[k] = cf.v[k] / vh;
      // w = origin - horizontal/2 - vertical/2 - lower_left
      Wv[k] = cf.o[k] - cf.h[k] / 2 - cf.v[k] / 2 - cf.ll[k];
    }
  }
  auto add_sphere = [&](const double* c, double r) {
    const double R = fabs(r);
    double cx = c[0] - cf.o[0], cy = c[1] - cf.o[1], cz = c[2] - cf.o[2];
    if (lookat) {
      const double ox = cx, oy = cy, oz = cz;
      cx = ox * U[0] + oy * U[1] + oz * U[2];
      cy = ox * V[0] + oy * V[1] + oz * V[2];
      cz = ox * Wv[0] + oy * Wv[1] + oz * Wv[2];
    }
    if (cz - R >= 0) return;  // entirely behind the camera: no camera ray reaches it
    // straddles the camera plane, or cannot be placed (a non-finite centre or
    // radius: Sphere.Hit accepts every ray for a NaN one): everywhere
    if (cz + R > -1e-9 || !(fabs(vw) > 0) || !std::isfinite(cx + cy + cz + R)) {
      for (auto& v : cost) v += 1.0f;
      return;
    }
    // image bounds of the bounding box corners (perspective keeps convexity)
    double u0 = INFINITY, u1 = -INFINITY, v0 = INFINITY, v1 = -INFINITY;
    for (int k = 0; k < 8; ++k) {
      const double qx = cx + ((k & 1) ? R : -R), qy = cy + ((k & 2) ? R : -R), qz = cz + ((k & 4) ? R : -R);
      const double u = 0.5 + qx / (-qz * vw), v = 0.5 + qy / (-qz * vh);
      u0 = fmin(u0, u);
      u1 = fmax(u1, u);
      v0 = fmin(v0, v);
      v1 = fmax(v1, v);
    }
    const double px0 = u0 * W, px1 = u1 * W, py0 = v0 * H, py1 = v1 * H;
    if (px1 < 0 || py1 < 0 || px0 >= W || py0 >= H) return;
    // (clamped before the conversion: a projection far outside the image does not fit an int)
    const int tx0 = (int)floor(fmax(px0, 0.0)) / 32, tx1 = std::min(tiles_x - 1, (int)floor(fmin(px1, W - 1)) / 32);
    const int ty0 = (int)floor(fmax(py0, 0.0)) / 32, ty1 = std::min(tiles_y - 1, (int)floor(fmin(py1, H - 1)) / 32);
    for (int ty = ty0; ty <= ty1; ++ty)
      for (int tx = tx0; tx <= tx1; ++tx) cost[ty * tiles_x + tx] += 1.0f;
  };
  for (const DSphere& s : fs.spheres) add_sphere(s.c, s.r);
  for (const DTri& t : fs.tris) add_sphere(t.bc, t.br);

  local_cost->clear();
  for (int32_t t : tiles) local_cost->push_back(cost[t]);
}

// Does the cone (apex, unit axis, cos/sin of its half-angle) meet the sphere
// (c, r)?  Same conservative test as the kernel's cone_meets_sphere: radius
// inflated by ~1e-7, far above binary64 rounding of the ray directions.
// Written as "not provably missed": a sphere with a NaN centre or radius fails
// every comparison and is kept (Sphere.Hit accepts every ray for it).
static bool cone_meets_sphere(const double c[3], double r, const double apex[3], const double axis[3], double cos_t,
                              double sin_t) {
  const double v[3] = {c[0] - apex[0], c[1] - apex[1], c[2] - apex[2]};
  const double dc2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2];
  const double dc = sqrt(dc2);
  const double ra = fabs(r) * (1.0 + 1e-7) + 1e-7 * dc + 1e-12;
  if (!(dc > ra)) return true;
  const double tl = sqrt(fmax(dc2 - ra * ra, 0.0));
  const double vd = v[0] * axis[0] + v[1] * axis[1] + v[2] * axis[2];
  return !(vd < cos_t * (1.0 - 1e-9) * tl - (sin_t + 1e-9) * ra - 1e-7 * dc);
}

// The cone around the camera rays of the image rectangle [x0, x1) x [y0, y1)
// (pixels): getRay direction (vw*(u-1/2), 2*(v-1/2), -1) with u in
// [x0/W, x1/W], v in [y0/H, y1/H] (renderer.go:155-156,377-390): unit axis
// and the cosine / sine of its half-angle.  Look-at model: the four corner
// directions from the frame, the normalised centre direction as the axis and
// the widest corner's angle (pixel_cone of rt_schedule.hip, for a rectangle).
static void rect_cone(const CamFrame& cf, int32_t W, int32_t H, int x0, int x1, int y0, int y1, double axis[3],
                      double* cmin, double* smax) {
  if (cf.model != RT_CAMERA_REFERENCE) {
    const double u[2] = {(double)x0 / W, (double)x1 / W}, v[2] = {(double)y0 / H, (double)y1 / H};
    double cd[4][3];
    for (int k = 0; k < 4; ++k)
      for (int a = 0; a < 3; ++a) cd[k][a] = ((cf.ll[a] + cf.h[a] * u[k & 1]) + cf.v[a] * v[k >> 1]) - cf.o[a];
    for (int a = 0; a < 3; ++a) axis[a] = 0.25 * ((cd[0][a] + cd[1][a]) + (cd[2][a] + cd[3][a]));
    const double al = sqrt(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2]);
    for (int a = 0; a < 3; ++a) axis[a] /= al;
    double c = 1.0;
    for (int k = 0; k < 4; ++k) {
      const double cl = sqrt(cd[k][0] * cd[k][0] + cd[k][1] * cd[k][1] + cd[k][2] * cd[k][2]);
      c = fmin(c, (axis[0] * cd[k][0] + axis[1] * cd[k][1] + axis[2] * cd[k][2]) / cl);
    }
    *cmin = c;
    *smax = sqrt(fmax(0.0, 1.0 - c * c));
    return;
  }
  const double vw = cf.h[0];
  const double dx0 = vw * ((double)x0 / W - 0.5), dx1 = vw * ((double)x1 / W - 0.5);
  const double dy0 = 2.0 * ((double)y0 / H - 0.5), dy1 = 2.0 * ((double)y1 / H - 0.5);
  axis[0] = 0.5 * (dx0 + dx1);
  axis[1] = 0.5 * (dy0 + dy1);
  axis[2] = -1.0;
  const double al = sqrt(axis[0] * axis[0] + axis[1] * axis[1] + axis[2] * axis[2]);
  for (int k = 0; k < 3; ++k) axis[k] /= al;
  double c = 1.0;  // the widest corner: the angle is quasiconvex on the image plane
  for (int k = 0; k < 4; ++k) {
    const double cx = (k & 1) ? dx1 : dx0, cy = (k & 2) ? dy1 : dy0;
    const double cl = sqrt(cx * cx + cy * cy + 1.0);
    c = fmin(c, (axis[0] * cx + axis[1] * cy - axis[2]) / cl);
  }
  *cmin = c;
  *smax = sqrt(fmax(0.0, 1.0 - c * c));
}

// candidates among `cand` (bit i: sphere / triangle i) whose bounding sphere
// meets the cone
static void cone_masks(const FlatScene& fs, const double apex[3], const double axis[3], double cmin, double smax, unsigned long long cand_s,
                       unsigned long long cand_t, unsigned long long* ms, unsigned long long* mt) {
  *ms = 0;
  *mt = 0;
  for (unsigned long long b = cand_s; b; b &= b - 1) {
    const int i = __builtin_ctzll(b);
    if (cone_meets_sphere(fs.spheres[i].c, fs.spheres[i].r, apex, axis, cmin, smax)) *ms |= 1ull << i;
  }
  for (unsigned long long b = cand_t; b; b &= b - 1) {
    const int i = __builtin_ctzll(b);
    if (cone_meets_sphere(fs.tris[i].bc, fs.tris[i].br, apex, axis, cmin, smax)) *mt |= 1ull << i;
  }
}

static unsigned long long low_bits(int n) { return n >= 64 ? ~0ull : (1ull << n) - 1ull; }

void tile_primary_masks(const FlatScene& fs, const CamFrame& cf, int32_t W, int32_t H,
                        const std::vector<int32_t>& tiles, std::vector<unsigned long long>* masks) {
  masks->clear();
  const int tiles_x = (W + 31) / 32;
  const int ns = (int)fs.spheres.size(), nt = (int)fs.tris.size();
  for (int32_t t : tiles) {
    const int tx = t % tiles_x, ty = t / tiles_x;
    double axis[3], cmin, smax;
    rect_cone(cf, W, H, tx * 32, std::min(tx * 32 + 32, (int)W), ty * 32, std::min(ty * 32 + 32, (int)H), axis, &cmin,
              &smax);
    unsigned long long ms, mt;
    cone_masks(fs, cf.o, axis, cmin, smax, low_bits(std::min(ns, 64)), low_bits(std::min(nt, 64)), &ms, &mt);
    masks->push_back(ms);
    masks->push_back(mt);
  }
}

// The same under the reference camera (RT_CAMERA_REFERENCE never fails)
static CamFrame reference_frame(const FlatScene& fs, int32_t W, int32_t H) {
  CamFrame cf;
  (void)camera_frame(fs.camera, RT_CAMERA_REFERENCE, W, H, &cf);
  return cf;
}
void tile_cost(const FlatScene& fs, int32_t W, int32_t H, const std::vector<int32_t>& tiles,
               std::vector<float>* local_cost) {
  tile_cost(fs, reference_frame(fs, W, H), W, H, tiles, local_cost);
}
void tile_primary_masks(const FlatScene& fs, int32_t W, int32_t H, const std::vector<int32_t>& tiles,
                        std::vector<unsigned long long>* masks) {
  tile_primary_masks(fs, reference_frame(fs, W, H), W, H, tiles, masks);
}

// ------------------------------------------------------------ partitions
void finish_partition(PartitionData* d) {
  static std::atomic<uint64_t> next_id{1};
  const int ntiles = (int)d->owner.size();
  d->offsets.assign(d->world + 1, 0);
  for (int t = 0; t < ntiles; ++t) d->offsets[d->owner[t] + 1] += 1;
  d->max_local = 0;
  for (int r = 0; r < d->world; ++r) {
    d->max_local = std::max(d->max_local, d->offsets[r + 1]);
    d->offsets[r + 1] += d->offsets[r];
  }
  d->lists.assign(ntiles, 0);
  d->local.assign(ntiles, 0);
  std::vector<int32_t> fill(d->offsets.begin(), d->offsets.end() - 1);
  for (int t = 0; t < ntiles; ++t) {  // ascending within each rank
    const int r = d->owner[t];
    d->local[t] = fill[r] - d->offsets[r];
    d->lists[fill[r]++] = t;
  }
  d->id = next_id.fetch_add(1);
}

// Longest processing time first: tiles by decreasing estimated work (ties:
// the lower tile first) to the least loaded rank (ties: the lower rank).
// Each tile weighs its estimate + 1: tiles with no estimated work still cost
// a launch slot, and spread evenly instead of piling onto one rank.
void lpt_partition(const std::vector<float>& work, PartitionData* d) {
  const int ntiles = (int)work.size(), world = d->world;
  d->owner.assign(ntiles, 0);
  std::vector<int32_t> order(ntiles);
  std::iota(order.begin(), order.end(), 0);
  auto wt = [&](int t) { return (double)work[t] + 1.0; };
  std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return wt(a) > wt(b); });
  d->work.assign(world, 0.0);
  for (int t : order) {
    int r = 0;
    for (int k = 1; k < world; ++k)
      if (d->work[k] < d->work[r]) r = k;
    d->owner[t] = r;
    d->work[r] += wt(t);
  }
  finish_partition(d);
}

}  // namespace rtgo
