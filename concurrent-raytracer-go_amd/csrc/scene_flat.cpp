// scene_flat.cpp — GetHittables + createCube + the material constructors
// (internal/scene/scene.go:59-190, internal/material/*.go) as flat device
// records (rt_scene_dev.h), the opt-in sky presets, and the host-only entry
// points of the ABI (settings defaults, tile arithmetic).  No HIP calls, so
// the sanitizer build (tests/c/Makefile) links it directly.
//
// Compiled with -ffp-contract=off: the precomputations (cube vertices,
// triangle edges and normals, material tables) must equal the values the
// reference computes per test.
#include <math.h>
#include <string.h>

#include "rt_internal.h"

namespace rtgo {

// ---------------------------------------------------------------- Go math
static double go_min(double x, double y) {
  if ((isinf(x) && x < 0) || (isinf(y) && y < 0)) return -INFINITY;
  if (isnan(x) || isnan(y)) return NAN;
  if (x == 0 && x == y) return signbit(x) ? x : y;
  return x < y ? x : y;
}

struct v3 {
  double x, y, z;
};
static v3 mk(double x, double y, double z) { return v3{x, y, z}; }
static v3 add(v3 a, v3 b) { return mk(a.x + b.x, a.y + b.y, a.z + b.z); }
static v3 sub(v3 a, v3 b) { return mk(a.x - b.x, a.y - b.y, a.z - b.z); }
static v3 divs(v3 a, double s) { return mk(a.x / s, a.y / s, a.z / s); }
static v3 cross(v3 a, v3 b) { return mk(a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x); }
static v3 normalize(v3 a) {
  double l = sqrt(a.x * a.x + a.y * a.y + a.z * a.z);
  if (l == 0) return mk(0, 0, 0);
  return divs(a, l);
}
static v3 arr(const double* p) { return mk(p[0], p[1], p[2]); }
static void put(double* d, v3 v) {
  d[0] = v.x;
  d[1] = v.y;
  d[2] = v.z;
}

// Material constructors (material.go:22-73,159-167,231-233,292-294;
// advanced_materials.go:14-19,117-123) and the metallic tables the renderer
// derives from GetMetallic (renderer.go:193-226,236-246,262-287).
static DMat make_mat(const rt_material& m) {
  DMat d;
  memset(&d, 0, sizeof d);
  d.kind = m.kind;
  put(d.color, arr(m.color));
  double metallic = 0.0;
  switch (m.kind) {
    case RT_MAT_METAL:
    case RT_MAT_SHINY:
      d.roughness = go_min(m.roughness, 1.0);
      metallic = go_min(m.metallic, 1.0);
      d.ior = 1.5;
      put(d.albedo, arr(m.color));
      if (m.kind == RT_MAT_METAL) {
        d.rough_draw = d.roughness > 0.001;
        d.fs = 0.6 + metallic * 0.4;
        d.mf = 0.4 + metallic * 0.5;
        d.blend_metal = metallic > 0.8;
      } else {
        d.rough_draw = d.roughness > 0;
        d.fs = 0.4 + go_min(m.specular, 1.0) * 0.4;
      }
      break;
    case RT_MAT_PERFECTMIRROR:
      d.roughness = go_min(m.roughness, 1.0);
      d.rough_draw = d.roughness > 0.001;
      metallic = 1.0;
      d.ior = 2.0;
      put(d.albedo, arr(m.color));
      break;
    case RT_MAT_GLASS:
      d.ior = m.refraction_index;
      put(d.albedo, arr(m.color));
      break;
    case RT_MAT_DIELECTRIC:  // attenuation and GetAlbedo are (1,1,1), material.go:236,266-268
      d.ior = m.refraction_index;
      put(d.color, mk(1.0, 1.0, 1.0));
      put(d.albedo, mk(1.0, 1.0, 1.0));
      break;
    case RT_MAT_DIFFUSELIGHT:
      put(d.emit, arr(m.color));
      break;
    default:  // lambertian
      d.kind = RT_MAT_LAMBERTIAN;
      put(d.albedo, arr(m.color));
      break;
  }
  d.metallic = metallic;
  {  // Schlick f0 = Pow((IOR-1)/(IOR+1), 2) — Go's Pow(x,2) rounds as x*x
    double r = (d.ior - 1.0) / (d.ior + 1.0);
    d.f0 = r * r;
  }
  d.ambient = 0.1;
  if (metallic > 0.9)
    d.ambient = 0.05;
  else if (metallic > 0.7)
    d.ambient = 0.07;
  else if (metallic > 0.5)
    d.ambient = 0.08;
  d.diffuse_strength = 0.25;
  if (metallic > 0.95)
    d.diffuse_strength = 0.05;
  else if (metallic > 0.9)
    d.diffuse_strength = 0.08;
  else if (metallic > 0.8)
    d.diffuse_strength = 0.12;
  else if (metallic > 0.7)
    d.diffuse_strength = 0.15;
  else if (metallic > 0.5)
    d.diffuse_strength = 0.2;
  d.spec_pow = metallic > 0.9 ? 64 : (metallic > 0.8 ? 48 : 32);
  if (metallic > 0.95) {
    d.rw = 0.85; d.dw = 0.15;
  } else if (metallic > 0.9) {
    d.rw = 0.8; d.dw = 0.2;
  } else if (metallic > 0.8) {
    d.rw = 0.75; d.dw = 0.25;
  } else if (metallic > 0.7) {
    d.rw = 0.7; d.dw = 0.3;
  } else if (metallic > 0.5) {
    d.rw = 0.6; d.dw = 0.4;
  } else if (metallic > 0.2) {
    d.rw = 0.4; d.dw = 0.6;
  } else {
    d.rw = 1.0; d.dw = 1.0;
  }
  return d;
}

// The followed-material predicate of the specular-through feature pass
// (rt_aov_spec_follows, include/rt_api.h) on the record the device tests:
// make_mat's kind and clamped roughness.
bool material_followed(const rt_material& m, double max_roughness) {
  const DMat d = make_mat(m);
  return (d.kind == RT_MAT_METAL || d.kind == RT_MAT_SHINY || d.kind == RT_MAT_PERFECTMIRROR) &&
         d.roughness <= max_roughness;
}

static void push_tri(FlatScene* fs, v3 v0, v3 v1, v3 v2, int mat, int obj) {
  DTri t;
  memset(&t, 0, sizeof t);
  v3 e1 = sub(v1, v0), e2 = sub(v2, v0);
  put(t.v0, v0);
  put(t.e1, e1);
  put(t.e2, e2);
  put(t.n, normalize(cross(e1, e2)));  // NewTriangle, triangle.go:13-34
  // bounding sphere for the shadow-cone culling (rt_shadow.h); any
  // rounding here is covered by the kernel's inflation margins
  const v3 bc = divs(add(add(v0, v1), v2), 3.0);
  double br = 0;
  for (v3 v : {v0, v1, v2}) {
    v3 dv = sub(v, bc);
    br = fmax(br, sqrt(dv.x * dv.x + dv.y * dv.y + dv.z * dv.z));
  }
  put(t.bc, bc);
  t.br = br;
  t.mat = mat;
  t.obj = obj;
  fs->tris.push_back(t);
}

void sky_presets(DSky out[kSkies]) {
  memset(out, 0, sizeof(DSky) * kSkies);
  struct P {
    double top[3], bottom[3], sun_dir[3], sun_color[3], sun_intensity, sun_size, rayleigh[3], mie[3], depth, fog,
        fog_color[3], haze, tod;
  };
  // NewDefaultAtmosphere, NewWhiteAtmosphere, NewSunsetAtmosphere,
  // NewNightAtmosphere (atmosphere.go:28-98); HazeIntensity is unused by GetSkyColor
  static const P presets[kSkies] = {
      {{0.6, 0.8, 1.0}, {0.9, 0.95, 1.0}, {0.0, 0.8, -0.6}, {1.0, 0.98, 0.95}, 1.2, 0.015, {0.6, 0.8, 1.0},
       {1.0, 0.98, 0.95}, 0.3, 0.0, {0.9, 0.92, 0.95}, 0.05, 0.6},
      {{0.98, 0.98, 1.0}, {0.92, 0.92, 0.95}, {0.0, 0.8, -0.6}, {1.0, 0.99, 0.97}, 0.8, 0.012, {0.9, 0.9, 0.95},
       {0.95, 0.95, 0.98}, 0.2, 0.0, {0.95, 0.95, 0.98}, 0.02, 0.6},
      {{1.0, 0.4, 0.2}, {1.0, 0.8, 0.6}, {0.0, 0.3, -0.9}, {1.0, 0.6, 0.3}, 1.2, 0.03, {1.0, 0.4, 0.2},
       {1.0, 0.8, 0.6}, 0.8, 0.1, {1.0, 0.8, 0.6}, 0.3, 0.8},
      {{0.1, 0.1, 0.3}, {0.2, 0.2, 0.4}, {0.0, -0.7, -0.7}, {0.8, 0.8, 1.0}, 0.3, 0.005, {0.1, 0.1, 0.3},
       {0.8, 0.8, 1.0}, 0.2, 0.0, {0.1, 0.1, 0.2}, 0.0, 0.0},
  };
  for (int i = 0; i < kSkies; ++i) {
    const P& p = presets[i];
    DSky& d = out[i];
    memcpy(d.top, p.top, sizeof d.top);
    memcpy(d.bottom, p.bottom, sizeof d.bottom);
    memcpy(d.sun_dir, p.sun_dir, sizeof d.sun_dir);
    memcpy(d.sun_color, p.sun_color, sizeof d.sun_color);
    d.sun_intensity = p.sun_intensity;
    d.sun_size = p.sun_size;
    memcpy(d.rayleigh, p.rayleigh, sizeof d.rayleigh);
    memcpy(d.mie, p.mie, sizeof d.mie);
    d.depth = p.depth;
    d.fog_density = p.fog;
    memcpy(d.fog_color, p.fog_color, sizeof d.fog_color);
    d.time_of_day = p.tod;
  }
}

void flatten_scene(const rt_scene& s, FlatScene* fs) {
  *fs = FlatScene();
  for (int i = 0; i < s.num_objects; ++i) {
    const rt_object& o = s.objects[i];
    const int mat = (int)fs->mats.size();
    fs->mats.push_back(make_mat(o.material));
    if (o.type == RT_OBJ_SPHERE) {
      DSphere sp;
      memset(&sp, 0, sizeof sp);
      put(sp.c, arr(o.position));
      sp.r = o.radius;
      sp.r2 = o.radius * o.radius;
      sp.mat = mat;
      sp.obj = i;
      fs->spheres.push_back(sp);
    } else {  // createCube, scene.go:150-190
      v3 pos = arr(o.position);
      v3 h = divs(arr(o.size), 2.0);
      v3 v[8] = {add(pos, mk(-h.x, -h.y, -h.z)), add(pos, mk(h.x, -h.y, -h.z)), add(pos, mk(h.x, h.y, -h.z)),
                 add(pos, mk(-h.x, h.y, -h.z)),  add(pos, mk(-h.x, -h.y, h.z)), add(pos, mk(h.x, -h.y, h.z)),
                 add(pos, mk(h.x, h.y, h.z)),    add(pos, mk(-h.x, h.y, h.z))};
      static const int faces[6][4] = {{0, 1, 2, 3}, {1, 5, 6, 2}, {5, 4, 7, 6},
                                      {4, 0, 3, 7}, {3, 2, 6, 7}, {4, 5, 1, 0}};
      DBox b;
      memset(&b, 0, sizeof b);
      b.first = (int32_t)fs->tris.size();
      b.count = 12;
      b.obj = i;
      for (int f = 0; f < 6; ++f) {
        push_tri(fs, v[faces[f][0]], v[faces[f][1]], v[faces[f][2]], mat, i);
        push_tri(fs, v[faces[f][0]], v[faces[f][2]], v[faces[f][3]], mat, i);
      }
      // the box of the 8 corners, padded outward (culling only; the
      // triangle tests stay exact)
      for (int a = 0; a < 3; ++a) {
        double lo = INFINITY, hi = -INFINITY;
        for (const v3& q : v) {
          const double c = a == 0 ? q.x : (a == 1 ? q.y : q.z);
          lo = fmin(lo, c);
          hi = fmax(hi, c);
        }
        const double pad = (fmax(fabs(lo), fabs(hi)) + (hi - lo)) * 1e-9 + 1e-12;
        b.lo[a] = lo - pad;
        b.hi[a] = hi + pad;
      }
      double r2 = 0;
      for (int a = 0; a < 3; ++a) {
        b.bc[a] = 0.5 * (b.lo[a] + b.hi[a]);
        r2 += (b.hi[a] - b.bc[a]) * (b.hi[a] - b.bc[a]);
      }
      b.br = sqrt(r2) * (1.0 + 1e-12);  // covers the padded box (the kernel adds its own margins)
      // the winding of createCube's face table (scene.go:164-171): normals
      // inward for a positive size product, outward for a negative one
      // (DBox.front_out).  A size difference that rounds away in a vertex
      // makes the box flat in that axis (its other faces zero-area, normal 0),
      // where leaving the plane never returns, whichever side is "out".
      const double vol = h.x * h.y * h.z;
      b.front_out = vol > 0 && isfinite(vol) ? 0 : (vol < 0 && isfinite(vol) ? 1 : -1);
      fs->boxes.push_back(b);
    }
  }
  for (int i = 0; i < s.num_lights; ++i) {
    DLight l;
    memset(&l, 0, sizeof l);
    put(l.pos, arr(s.lights[i].position));
    put(l.color, arr(s.lights[i].color));
    l.intensity = s.lights[i].intensity;
    fs->lights.push_back(l);
  }
  put(fs->cam_pos, arr(s.camera.position));
  fs->aspect = s.camera.aspect_ratio;
  fs->camera = s.camera;
  fs->objects = s.num_objects;
}

// ---------------------------------------------------------------- shadow-cone rows
// Which spheres can ever be a shadow-cone candidate (rt_shadow.h in_cone)
// of a hit on sphere A under light L?  The hit point P lies on A, so every
// shadow ray of (A, L) stays in one solid that depends on the scene alone,
// and a sphere clear of it is never admitted.
//
// What in_cone admits.  With v = c_B - P, dc = |v|, ra its inflated radius,
// sin(beta) = ra / dc, theta = angle(v, ldir), l = ldist (1 + 1e-5) + 1e-9:
//   inside: dc <= ra;   or   dc - ra <= l  and  theta <= alpha~ + beta,
// alpha~ = asin(0.1) + d.  d covers the slack of `meets`: dividing it by dc,
//   cos(theta) >= 0.99498 cos(beta) (1 - 2e-7) - 0.1 sin(beta) - 1e-5 (1 + 2e-7)
//              >= cos(alpha' + beta) - 1.77e-5
// (the binary32 roots are 2e-7 wide; |(0.99498, 0.1)| = 1 - 7.4e-6; alpha' =
// atan(0.1 / 0.99498) = asin(0.1) + 7e-8), and sin(alpha' + beta) >= 0.0999
// turns 1.77e-5 of cosine into d <= 1.8e-4 rad.
// Let S be the sector {P + s u : 0 <= s <= l, angle(u, ldir) <= alpha~}.
//   inside:            P is in S and |c_B - P| <= ra;
//   theta <= alpha~:   P + min(dc, l) v/dc is in S, max(0, dc - l) <= ra away;
//   else, phi = theta - alpha~ <= beta and w the cone's edge towards v:
//     dc cos(phi) <= l:  P + dc cos(phi) w is in S, dc sin(phi) <= ra away;
//     dc cos(phi) >  l:  the far corner P + l w is
//       sqrt((dc sin(phi))^2 + (dc cos(phi) - l)^2) <= sqrt(2) ra away,
//       since 0 < dc cos(phi) - l <= dc - (dc - ra) = ra.
// So an admitted B has dist(c_B, S) <= ra, or is within sqrt(2) ra of a far
// corner of S.
//
// The solid.  P is within RA = |r_A| + eP of c_A (eP below).  A point of S
// at ray parameter s = tau * ldist is 2 sin(alpha~ / 2) s <= 0.100306 s from
// the axis point a = P + tau (L - P), and ldist <= D + RA, D = |L - c_A|.
//   tau <= 1: a is (1 - tau) RA from c(tau) = (1 - tau) c_A + tau L, so the
//     point is in the ball around c(tau) of radius RA + tau (kK (D + RA) - RA);
//   1 < tau <= l / ldist <= 1 + 2e-5 (ldist >= 0.001 for a lit light): a is
//     2e-5 (D + RA) from L, the point within (0.100306 (1 + 2e-5) + 2e-5)
//     (D + RA) <= kK (D + RA) of L: the ball of tau = 1, far corners included.
// kK = 0.1004 leaves 7e-5 over both.  f(t) = |c_B - c(t)| - radius(t) is
// convex in t, so for any t in [0, 1] its tangent bounds it from below:
//   min f >= f(t) + min(-t f'(t), (1 - t) f'(t)),
// evaluated at the stationary point of the closed form (clamped to [0, 1]);
// a badly rounded t only loosens the bound, it stays one.
//
// Margins.  ra <= |r_B| (1 + 1e-5) + 1e-5 (1 + 1e-6) (|c_B - c_A| + RA) + 1e-12
// (dc <= |c_B - c_A| + RA; 1e-6 for the binary32 root of dc).  eP = 2e-7 E,
// E the scene's extent (centres + radii, lights, camera): a hit point o + t d
// has |o - c| <= 2 E, its discriminant an absolute error below 1e-15 a
// |o - c|^2, so the root moves P by at most sqrt(1e-15) |o - c| < 7e-8 E;
// the roundings of o + t d are nine orders below that.  This arithmetic is
// binary64: 1e-9 of the lengths involved covers it a million times over.
// Scenes of extent beyond 1e15 (binary32 roots of squares overflow) or below
// 1e-100 (squares underflow) and non-finite scenes get full rows.
namespace {
constexpr double kConeK = 0.1004;
double vdot(v3 a, v3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
double vnorm(v3 a) { return sqrt(vdot(a, a)); }
v3 vscale(v3 a, double s) { return mk(a.x * s, a.y * s, a.z * s); }

// sphere B is provably clear of the solid of (hit sphere A, light L)
bool cone_clear(const DSphere& A, const DSphere& B, v3 L, double E) {
  const double RA = fabs(A.r) + 2e-7 * E;
  const v3 w = sub(L, arr(A.c)), q = sub(arr(B.c), arr(A.c));
  const double D = vnorm(w), Q = vnorm(q);
  const double k = kConeK * (D + RA) - RA;  // d radius / dt
  const double ra = fabs(B.r) * (1.0 + 1e-5) + 1e-5 * (1.0 + 1e-6) * (Q + RA) + 1e-12;
  const double slack = 1e-9 * (Q + D + RA + fabs(B.r));
  double t = k > 0 ? 1.0 : 0.0;  // D == 0: f is linear in t
  if (D > 0) {
    const double qa = vdot(q, w) / D;                    // q along the axis
    const double qn = vnorm(sub(q, vscale(w, qa / D)));  // and across it
    const double kp = k / D;                             // (< kConeK; below -1: f rises, t = 0)
    t = kp > -1.0 ? (qa + kp * qn / sqrt(1.0 - kp * kp)) / D : 0.0;
    t = t > 0 ? (t < 1 ? t : 1.0) : 0.0;                 // (NaN: 0)
  }
  const v3 d = sub(q, vscale(w, t));
  const double dl = vnorm(d);
  const double f = dl - (RA + t * k);
  const double df = -vdot(d, w) / dl - k;
  const double low = f + fmin(-t * df, (1.0 - t) * df);
  const double f1 = vnorm(sub(q, w)) - kConeK * (D + RA);
  return low - slack > ra && f1 - slack > 1.41422 * ra;  // (a NaN: not clear)
}
}  // namespace

bool cone_masks_apply(const FlatScene& fs) {
  return fs.bvh.empty() && fs.spheres.size() <= 64 && fs.tris.size() <= 64;
}

double cone_extent(const FlatScene& fs) {
  double E = vnorm(arr(fs.cam_pos));
  for (const DSphere& s : fs.spheres) E = fmax(E, vnorm(arr(s.c)) + fabs(s.r));
  for (const DLight& l : fs.lights) E = fmax(E, vnorm(arr(l.pos)));
  return E;
}

bool cone_rows_hold(const FlatScene& fs, const double origin[3]) {
  return vnorm(arr(origin)) <= 2.0 * cone_extent(fs);  // (a NaN origin: no)
}

void cone_rows(const FlatScene& fs, std::vector<unsigned long long>* rows) {
  const size_t nl = fs.lights.size(), no = (size_t)fs.objects;
  rows->assign(nl * no, ~0ull);
  if (!cone_masks_apply(fs)) return;
  const double E = cone_extent(fs);
  for (const DSphere& s : fs.spheres)  // (fmax drops a NaN)
    if (!isfinite(s.c[0] + s.c[1] + s.c[2] + s.r)) return;
  for (const DLight& l : fs.lights)
    if (!isfinite(l.pos[0] + l.pos[1] + l.pos[2])) return;
  if (!(E <= 1e15 && E >= 1e-100)) return;
  for (size_t li = 0; li < nl; ++li)
    for (const DSphere& A : fs.spheres) {  // (a cube's row stays full)
      unsigned long long m = 0;
      for (size_t b = 0; b < fs.spheres.size(); ++b)
        if (&fs.spheres[b] == &A || !cone_clear(A, fs.spheres[b], arr(fs.lights[li].pos), E)) m |= 1ull << b;
      (*rows)[li * no + (size_t)A.obj] = m;
    }
}

// Go's Vec3 methods (internal/math/vector.go) on the host, for the frame
namespace {
struct V3 {
  double x, y, z;
};
V3 vsub(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
V3 vmuls(V3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
V3 vdivs(V3 a, double s) { return {a.x / s, a.y / s, a.z / s}; }
V3 vcross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
double vlen(V3 a) { return sqrt(a.x * a.x + a.y * a.y + a.z * a.z); }
V3 varr(const double* p) { return {p[0], p[1], p[2]}; }
void vput(double* p, V3 a) {
  p[0] = a.x;
  p[1] = a.y;
  p[2] = a.z;
}
}  // namespace

// rt_camera_frame (include/rt_api.h states the definition and the order)
int camera_frame(const rt_camera& cam, int32_t model, int32_t w, int32_t h, CamFrame* out) {
  memset(out, 0, sizeof *out);
  const V3 origin = varr(cam.position);
  V3 horizontal, vertical, ll;
  if (model == RT_CAMERA_REFERENCE) {
    // getRay (renderer.go:377-390): aspect and position only
    horizontal = {2.0 * cam.aspect_ratio, 0, 0};
    vertical = {0, 2.0, 0};
    ll = vsub(vsub(vsub(origin, vdivs(horizontal, 2)), vdivs(vertical, 2)), V3{0, 0, 1.0});
  } else if (model == RT_CAMERA_LOOKAT) {
    if (w <= 0 || h <= 0) {
      set_error("camera frame: invalid image size " + std::to_string(w) + "x" + std::to_string(h));
      return RT_E_INVALID;
    }
    const double fields[11] = {cam.position[0], cam.position[1], cam.position[2], cam.look_at[0],
                               cam.look_at[1],  cam.look_at[2],  cam.up[0],       cam.up[1],
                               cam.up[2],       cam.fov,         cam.aspect_ratio};
    for (double v : fields)
      if (!std::isfinite(v)) {
        set_error("look-at camera: position, lookAt, up, fov and aspectRatio must be finite");
        return RT_E_INVALID;
      }
    if (!(cam.fov > 0 && cam.fov < 180)) {
      set_error("look-at camera: fov must be in (0, 180) degrees");
      return RT_E_INVALID;
    }
    if (cam.aspect_ratio < 0) {
      set_error("look-at camera: aspectRatio must not be negative (0: width / height)");
      return RT_E_INVALID;
    }
    const V3 back = vsub(origin, varr(cam.look_at));
    const double bl = vlen(back);
    if (bl == 0) {
      set_error("look-at camera: position equals lookAt");
      return RT_E_INVALID;
    }
    const V3 wv = vdivs(back, bl);  // Vec3.Normalize
    const V3 side = vcross(varr(cam.up), wv);
    const double sl = vlen(side);
    if (sl == 0) {
      set_error("look-at camera: up is zero or parallel to the viewing direction");
      return RT_E_INVALID;
    }
    const V3 U = vdivs(side, sl);
    const V3 V = vcross(wv, U);
    // exactly 1 at 90 degrees, the reference's viewport (tan(pi/4) rounds below 1)
    const double hh = cam.fov == 90 ? 1.0 : tan(cam.fov * (M_PI / 360));
    const double a = cam.aspect_ratio != 0 ? cam.aspect_ratio : (double)w / h;
    const double vh = 2.0 * hh, vw = vh * a;
    horizontal = vmuls(U, vw);
    vertical = vmuls(V, vh);
    ll = vsub(vsub(vsub(origin, vdivs(horizontal, 2)), vdivs(vertical, 2)), wv);
    const double fr[9] = {horizontal.x, horizontal.y, horizontal.z, vertical.x, vertical.y, vertical.z, ll.x, ll.y, ll.z};
    for (double v : fr)
      if (!std::isfinite(v)) {
        set_error("look-at camera: the viewport frame overflows binary64");
        return RT_E_INVALID;
      }
  } else {
    set_error("camera must be RT_CAMERA_REFERENCE or RT_CAMERA_LOOKAT");
    return RT_E_INVALID;
  }
  vput(out->o, origin);
  vput(out->ll, ll);
  vput(out->h, horizontal);
  vput(out->v, vertical);
  out->model = model;
  return RT_OK;
}

}  // namespace rtgo

extern "C" {

void rt_settings_default(rt_settings* s) {
  if (!s) return;
  memset(s, 0, sizeof *s);
  // NewParallelRenderer defaults, renderer.go:54-65
  s->samples = 100;
  s->max_depth = 50;
  s->anti_aliasing = 1;
  s->recursive_reflections = 1;
  s->soft_shadows = 1;
  s->depth_of_field = 0;
  s->num_workers = 1;
  s->num_devices = 1;
  s->seed = 1;
  s->camera = RT_CAMERA_REFERENCE;  // getRay's fixed -Z view; the scene's lookAt / up / fov are opt-in
}

void rt_tuning_default(rt_tuning* t) {
  if (!t) return;
  memset(t, 0, sizeof *t);
  t->path = RT_PATH_AUTO;
  t->pilot = 1;
  t->frustum = 1;
  t->stage = 1;
  t->wf_lds_nodes = -1;
  // a pilot path is followed for 12 bounces at most: every longer path is
  // "heavy" alike (split, dispatched first), and the pilot's own tail is one
  // 12-bounce path instead of a 50-bounce one (C2 first frame 1.39 -> 1.07 ms,
  // the main launch unchanged; scripts/first_frame_probe.py)
  t->pilot_depth = 12;
  // measured re-cuts are exact but do not shorten the launch: its tail is
  // the chains of the longest paths, not the block sizes (C2 0.80 pilot-only
  // vs 0.84 ms measured, C3 0.59 vs 0.56; scripts/tuning_sweep.py)
  t->measure = 0;
  // tail helpers: 64 at the end of the launch; drains
  // checked every 4th iteration, paths of >= 2 bounces, <= 4 left (the 0s)
  t->tail_helpers = -1;  // measured a net loss on the headline frame
  // streamed launches: auto; the frames of a launch
  // interleaved, 512 entries per claim (the 0) -- the measured best of the sweep
  t->stream = -1;
  t->stream_order = 1;
}

int32_t rt_num_tiles(int32_t w, int32_t h) {
  if (w <= 0 || h <= 0) return 0;
  return ((w + 31) / 32) * ((h + 31) / 32);
}

int32_t rt_tiles_for_rank(int32_t w, int32_t h, int32_t rank, int32_t world) {
  int32_t n = rt_num_tiles(w, h);
  if (world < 1 || rank < 0 || rank >= world || rank >= n) return 0;
  return (n - rank + world - 1) / world;
}

}  // extern "C"
