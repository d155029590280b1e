// Nodal fields of a 2-D cell complex sampled at points (include/bsms_hip_sample.h: bsms_raster_owner, bsms_point_owner,
// bsms_field_gather), built into the third companion library libbsms_hip_sample.so: the surfaces of libbsms_hip.so,
// libbsms_hip_ext.so and libbsms_hip_stats.so are closed.  One containment / barycentric function (tri_edges) serves the three
// entries: the rasteriser walks bounding boxes of pixel centres and takes atomicMin on the owner image, the point locator lets a
// wave stride the triangles, the gather turns owners into weights once per sample and reuses them over S * C values.
// Compiled with -ffp-contract=off (build.py): every orient() keeps the roundings of separate fp64 multiplies and subtractions, which
// is what makes a NumPy restatement bit-comparable.
#include <algorithm>
#include <cmath>

#include "../common.h"
#include "../../../include/bsms_hip_sample.h"

#pragma clang fp contract(off)

using namespace bsms;

namespace {

constexpr int kThreads = 256;                           // four waves of 64
constexpr int kGroup = 8;                               // lanes that hold one triangle in k_raster_tris (a power of two below 64)
constexpr int kSmallBox = 64;                           // pixels a group walks at most (the measured default: DESIGN.md 4.26)
constexpr int kWaveBox = 16384;                         // pixels the triangle's wave walks at most (256 per lane); above, k_raster_listed
constexpr int kListBlocks = 256;                        // blocks of k_raster_listed: 65536 threads stride every listed box
constexpr int kListCap = 1023;                          // listed triangles; one more is left to its wave
constexpr int64_t kMaxSide = 32768;                     // W, H: W * H <= 2^30 fits 32-bit pixel indices
constexpr int64_t kMaxIndex = (int64_t(1) << 31) - 2;   // N, T

struct RasterWork {
  unsigned count;                                       // triangles that asked for a place in the list (may exceed kListCap)
  int32_t list[kListCap];
};

struct Mesh {
  const float* pos;
  int64_t pos_stride, N;
  const int32_t* tris;
  int64_t T;
};
struct Grid {
  int32_t W, H;
  double x0, y0, dx, dy;
};

struct Tri {
  int32_t a, b, c;
  double ax, ay, bx, by, cx, cy;
  double A;                                             // orient(a, b, c)
};

__device__ __forceinline__ double orient(double ux, double uy, double vx, double vy, double qx, double qy) {
  return (vx - ux) * (qy - uy) - (vy - uy) * (qx - ux);
}

// triangle t with its corners promoted to fp64; false (nothing is read from pos) when it names a node outside [0, N)
__device__ __forceinline__ bool load_tri(const Mesh& m, int64_t t, Tri& tr) {
  tr.a = m.tris[3 * t], tr.b = m.tris[3 * t + 1], tr.c = m.tris[3 * t + 2];
  if (tr.a < 0 || tr.b < 0 || tr.c < 0 || tr.a >= m.N || tr.b >= m.N || tr.c >= m.N) return false;
  const float *pa = m.pos + tr.a * m.pos_stride, *pb = m.pos + tr.b * m.pos_stride, *pc = m.pos + tr.c * m.pos_stride;
  tr.ax = double(pa[0]), tr.ay = double(pa[1]);
  tr.bx = double(pb[0]), tr.by = double(pb[1]);
  tr.cx = double(pc[0]), tr.cy = double(pc[1]);
  tr.A = orient(tr.ax, tr.ay, tr.bx, tr.by, tr.cx, tr.cy);
  return true;
}

// THE containment / barycentric function of the contract: the three edge functions of q, and whether the triangle contains it
__device__ __forceinline__ bool tri_edges(const Tri& tr, double qx, double qy, double& e0, double& e1, double& e2) {
  e0 = orient(tr.bx, tr.by, tr.cx, tr.cy, qx, qy);
  e1 = orient(tr.cx, tr.cy, tr.ax, tr.ay, qx, qy);
  e2 = orient(tr.ax, tr.ay, tr.bx, tr.by, qx, qy);
  if (!(tr.A != 0.0) || !isfinite(tr.A)) return false;  // NaN fails the first test
  const double sg = tr.A > 0.0 ? 1.0 : -1.0;
  return e0 * sg >= 0.0 && e1 * sg >= 0.0 && e2 * sg >= 0.0;
}

__device__ __forceinline__ double centre(double o, double d, int k) { return o + (double(k) + 0.5) * d; }

// pixels [k0, k1] of an axis of n pixels whose centres o + (k + 0.5) d may lie in [lo_c, hi_c], one more on either side; false when
// there are none.  The conversions to int see values in [0, n - 1] only.
__device__ __forceinline__ bool pixel_range(double lo_c, double hi_c, double o, double d, int n, int& k0, int& k1) {
  const double u0 = (lo_c - o) / d - 0.5, u1 = (hi_c - o) / d - 0.5;
  if (isnan(u0) || isnan(u1)) return false;
  const double lo = floor(fmin(u0, u1)) - 1.0, hi = ceil(fmax(u0, u1)) + 1.0, last = double(n - 1);
  if (hi < 0.0 || lo > last) return false;
  k0 = lo <= 0.0 ? 0 : int(lo);
  k1 = hi >= last ? n - 1 : int(hi);
  return true;
}

struct Box {
  int i0, i1, j0, j1;
  __device__ int width() const { return i1 - i0 + 1; }
  __device__ int pixels() const { return (i1 - i0 + 1) * (j1 - j0 + 1); }   // <= W * H <= 2^30
};

// the triangle and the clipped box of pixel centres it may own; false for a triangle that owns nothing
__device__ __forceinline__ bool tri_box(const Mesh& m, const Grid& g, int64_t t, Tri& tr, Box& b) {
  if (!load_tri(m, t, tr)) return false;
  if (!(tr.A != 0.0) || !isfinite(tr.A)) return false;
  const double xl = fmin(tr.ax, fmin(tr.bx, tr.cx)), xh = fmax(tr.ax, fmax(tr.bx, tr.cx));
  const double yl = fmin(tr.ay, fmin(tr.by, tr.cy)), yh = fmax(tr.ay, fmax(tr.by, tr.cy));
  if (!isfinite(xl) || !isfinite(xh) || !isfinite(yl) || !isfinite(yh)) return false;
  return pixel_range(xl, xh, g.x0, g.dx, g.W, b.i0, b.i1) && pixel_range(yl, yh, g.y0, g.dy, g.H, b.j0, b.j1);
}

// pixel `idx` of the box: the triangle claims it when it contains the centre.  -1 is the largest unsigned word.
__device__ __forceinline__ void claim(const Tri& tr, const Box& b, const Grid& g, int idx, int32_t t, int32_t* owner) {
  const int bw = b.width(), j = b.j0 + idx / bw, i = b.i0 + idx % bw;
  double e0, e1, e2;
  if (tri_edges(tr, centre(g.x0, g.dx, i), centre(g.y0, g.dy, j), e0, e1, e2))
    atomicMin(reinterpret_cast<unsigned*>(owner) + (size_t(j) * g.W + i), unsigned(t));
}

// kGroup lanes per triangle: small boxes by the group itself, then the wave's larger boxes one after the other by its 64 lanes; boxes
// above kWaveBox go to the list.  The lanes of a group read the same triangle (one address) and find the same box.
__global__ __launch_bounds__(kThreads) void k_raster_tris(const Mesh m, const Grid g, int small_box, int32_t* __restrict__ owner,
                                                          RasterWork* __restrict__ work) {
  const int64_t gtid = int64_t(blockIdx.x) * kThreads + int(threadIdx.x);
  const int64_t t = gtid / kGroup;
  const int lane = int(threadIdx.x) & 63, sub = int(threadIdx.x) % kGroup;
  Tri tr;
  Box b;
  const bool live = t < m.T && tri_box(m, g, t, tr, b);
  const int n = live ? b.pixels() : 0;
  bool shared = sub == 0 && n > small_box;              // the group's first lane speaks for it
  if (n > small_box) {
    if (shared && n > kWaveBox) {
      const unsigned slot = atomicAdd(&work->count, 1u);
      if (slot < unsigned(kListCap)) {
        work->list[slot] = int32_t(t);
        shared = false;
      }
    }
  } else {
    for (int idx = sub; idx < n; idx += kGroup) claim(tr, b, g, idx, int32_t(t), owner);
  }
  unsigned long long todo = __ballot(shared);
  while (todo) {                                        // wave-uniform
    const int src = __ffsll(todo) - 1;
    todo &= todo - 1;
    const int64_t ts = (gtid - lane + src) / kGroup;    // the triangle of lane `src`: every lane reads it again (one cached address)
    Tri trs;
    Box bs;
    if (!tri_box(m, g, ts, trs, bs)) continue;          // as lane `src` found it: never taken
    const int ns = bs.pixels();
    for (int idx = lane; idx < ns; idx += 64) claim(trs, bs, g, idx, int32_t(ts), owner);
  }
}

// every listed triangle's box over the whole grid
__global__ __launch_bounds__(kThreads) void k_raster_listed(const Mesh m, const Grid g, int32_t* __restrict__ owner,
                                                            const RasterWork* __restrict__ work) {
  const unsigned asked = work->count;
  const int count = int(asked < unsigned(kListCap) ? asked : unsigned(kListCap));
  const int first = int(blockIdx.x) * kThreads + int(threadIdx.x);
  for (int k = 0; k < count; ++k) {
    const int32_t t = work->list[k];
    Tri tr;
    Box b;
    if (t < 0 || t >= m.T || !tri_box(m, g, t, tr, b)) continue;
    const int n = b.pixels();
    for (int idx = first; idx < n; idx += kListBlocks * kThreads) claim(tr, b, g, idx, t, owner);
  }
}

// a wave per query point: lane l tests the triangles l, l + 64, ...; the first round with a hit ends the search
__global__ __launch_bounds__(kThreads) void k_point_owner(const Mesh m, const double* __restrict__ points, int64_t P,
                                                          int32_t* __restrict__ owner) {
  const int lane = int(threadIdx.x) & 63;
  const int64_t p = int64_t(blockIdx.x) * (kThreads / 64) + (int(threadIdx.x) >> 6);
  if (p >= P) return;                                   // wave-uniform
  const double qx = points[2 * p], qy = points[2 * p + 1];
  int32_t best = INT32_MAX;
  for (int64_t t0 = 0; t0 < m.T; t0 += 64) {
    const int64_t t = t0 + lane;
    Tri tr;
    double e0, e1, e2;
    const bool hit = t < m.T && load_tri(m, t, tr) && tri_edges(tr, qx, qy, e0, e1, e2);
    if (hit) best = int32_t(t);
    if (__ballot(hit)) break;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) best = min(best, __shfl_xor(best, off, 64));
  if (lane == 0) owner[p] = best == INT32_MAX ? -1 : best;
}

struct GatherArgs {
  Mesh m;
  Grid g;
  const int32_t* owner;
  const double* points;                                 // null: the grid
  int64_t n;                                            // samples: P or W * H
  const float* fields;
  int64_t S, C, set_stride, row_stride;
  int64_t out_s, out_c, out_k;                          // out[s * out_s + c * out_c + k * out_k]
  float fill;
  float* out;
};

// a thread per sample: owner -> weights once, then S * C values; for the grid the stores of a wave are 256 contiguous bytes
__global__ __launch_bounds__(kThreads) void k_field_gather(const GatherArgs a) {
  const int64_t k = int64_t(blockIdx.x) * kThreads + int(threadIdx.x);
  if (k >= a.n) return;
  double qx, qy;
  if (a.points) {
    qx = a.points[2 * k], qy = a.points[2 * k + 1];
  } else {
    qx = centre(a.g.x0, a.g.dx, int(k % a.g.W)), qy = centre(a.g.y0, a.g.dy, int(k / a.g.W));
  }
  const int32_t t = a.owner[k];
  Tri tr;
  const bool owned = t >= 0 && t < a.m.T && load_tri(a.m, t, tr);
  double w0 = 0.0, w1 = 0.0, w2 = 0.0;
  if (owned) {
    double e0, e1, e2;
    tri_edges(tr, qx, qy, e0, e1, e2);
    const double s = (e0 + e1) + e2;
    w0 = e0 / s, w1 = e1 / s, w2 = e2 / s;
  }
  float* out = a.out + k * a.out_k;
  const int C = int(a.C);
  for (int64_t s = 0; s < a.S; ++s) {
    const float* f = a.fields + s * a.set_stride;
    if (owned) {
      const float *fa = f + tr.a * a.row_stride, *fb = f + tr.b * a.row_stride, *fc = f + tr.c * a.row_stride;
      float va[kMaxC], vb[kMaxC], vc[kMaxC];
#pragma unroll
      for (int c = 0; c < kMaxC; ++c)
        if (c < C) va[c] = fa[c], vb[c] = fb[c], vc[c] = fc[c];
#pragma unroll
      for (int c = 0; c < kMaxC; ++c)
        if (c < C) out[s * a.out_s + c * a.out_c] = float((w0 * double(va[c]) + w1 * double(vb[c])) + w2 * double(vc[c]));
    } else {
      for (int c = 0; c < C; ++c) out[s * a.out_s + c * a.out_c] = a.fill;
    }
  }
}

int check_mesh(const char* who, const float* pos, int64_t pos_stride, int64_t N, const int32_t* tris, int64_t T) {
  BSMS_REQUIRE(N >= 0 && T >= 0 && pos_stride >= 2, BSMS_E_INVALID_ARG, "%s: N=%lld T=%lld pos_stride=%lld (N, T >= 0, pos_stride >= 2)", who,
               (long long)N, (long long)T, (long long)pos_stride);
  BSMS_REQUIRE(N <= kMaxIndex && T <= kMaxIndex, BSMS_E_SHAPE, "%s: N=%lld T=%lld (at most 2^31 - 2)", who, (long long)N, (long long)T);
  BSMS_REQUIRE((pos || N == 0) && (tris || T == 0), BSMS_E_INVALID_ARG, "%s: null mesh argument", who);
  return BSMS_OK;
}

int check_grid(const char* who, int64_t W, int64_t H, double x0, double y0, double dx, double dy) {
  BSMS_REQUIRE(W >= 1 && H >= 1 && W <= kMaxSide && H <= kMaxSide, BSMS_E_INVALID_ARG, "%s: W=%lld H=%lld (1..32768)", who, (long long)W,
               (long long)H);
  BSMS_REQUIRE(std::isfinite(x0) && std::isfinite(y0) && std::isfinite(dx) && std::isfinite(dy) && dx != 0.0 && dy != 0.0, BSMS_E_INVALID_ARG,
               "%s: x0=%g y0=%g dx=%g dy=%g (finite, steps non-zero)", who, x0, y0, dx, dy);
  return BSMS_OK;
}

}  // namespace

extern "C" size_t bsms_raster_work_bytes(void) { return sizeof(RasterWork); }

extern "C" int bsms_raster_owner(const float* pos, int64_t pos_stride, int64_t N, const int32_t* tris, int64_t T, int64_t W, int64_t H,
                                 double x0, double y0, double dx, double dy, int64_t small_box, int32_t* owner, void* work,
                                 bsms_stream_t stream) {
  if (int rc = check_mesh("raster_owner", pos, pos_stride, N, tris, T)) return rc;
  if (int rc = check_grid("raster_owner", W, H, x0, y0, dx, dy)) return rc;
  BSMS_REQUIRE(owner && work, BSMS_E_INVALID_ARG, "raster_owner: null argument");
  hipStream_t s = as_stream(stream);
  BSMS_HIP_CHECK(hipMemsetAsync(owner, 0xFF, size_t(W) * size_t(H) * sizeof(int32_t), s));       // -1 everywhere
  if (T == 0) return BSMS_OK;
  RasterWork* rw = static_cast<RasterWork*>(work);
  BSMS_HIP_CHECK(hipMemsetAsync(&rw->count, 0, sizeof(unsigned), s));
  const Mesh m{pos, pos_stride, N, tris, T};
  const Grid g{int32_t(W), int32_t(H), x0, y0, dx, dy};
  const int small = small_box <= 0 ? kSmallBox : int(std::min<int64_t>(small_box, kWaveBox));
  hipLaunchKernelGGL(k_raster_tris, dim3(unsigned(ceil_div(T * kGroup, kThreads))), dim3(kThreads), 0, s, m, g, small, owner, rw);
  BSMS_LAUNCH_CHECK();
  hipLaunchKernelGGL(k_raster_listed, dim3(kListBlocks), dim3(kThreads), 0, s, m, g, owner, rw);
  BSMS_LAUNCH_CHECK();
  return BSMS_OK;
}

extern "C" int bsms_point_owner(const float* pos, int64_t pos_stride, int64_t N, const int32_t* tris, int64_t T, const double* points,
                                int64_t P, int32_t* owner, bsms_stream_t stream) {
  if (int rc = check_mesh("point_owner", pos, pos_stride, N, tris, T)) return rc;
  BSMS_REQUIRE(P >= 0 && P <= kMaxIndex, BSMS_E_INVALID_ARG, "point_owner: P=%lld", (long long)P);
  if (P == 0) return BSMS_OK;
  BSMS_REQUIRE(points && owner, BSMS_E_INVALID_ARG, "point_owner: null argument");
  const Mesh m{pos, pos_stride, N, tris, T};
  hipLaunchKernelGGL(k_point_owner, dim3(unsigned(ceil_div(P, kThreads / 64))), dim3(kThreads), 0, as_stream(stream), m, points, P, owner);
  BSMS_LAUNCH_CHECK();
  return BSMS_OK;
}

extern "C" int bsms_field_gather(const float* pos, int64_t pos_stride, int64_t N, const int32_t* tris, int64_t T, const int32_t* owner,
                                 const double* points, int64_t P, int64_t W, int64_t H, double x0, double y0, double dx, double dy,
                                 const float* fields, int64_t S, int64_t C, int64_t set_stride, int64_t row_stride, float fill, float* out,
                                 bsms_stream_t stream) {
  BSMS_REQUIRE(C >= 1 && C <= kMaxC, BSMS_E_UNSUPPORTED, "field_gather: C=%lld (C in 1..8)", (long long)C);
  if (int rc = check_mesh("field_gather", pos, pos_stride, N, tris, T)) return rc;
  GatherArgs a;
  a.g = Grid{1, 1, 0.0, 0.0, 1.0, 1.0};
  if (points) {
    BSMS_REQUIRE(P >= 0 && P <= kMaxIndex, BSMS_E_INVALID_ARG, "field_gather: P=%lld", (long long)P);
    a.n = P, a.out_s = P * C, a.out_c = 1, a.out_k = C;
  } else {
    if (int rc = check_grid("field_gather", W, H, x0, y0, dx, dy)) return rc;
    a.g = Grid{int32_t(W), int32_t(H), x0, y0, dx, dy};
    a.n = W * H, a.out_s = C * a.n, a.out_c = a.n, a.out_k = 1;
  }
  BSMS_REQUIRE(S >= 0 && row_stride >= C, BSMS_E_INVALID_ARG, "field_gather: S=%lld row_stride=%lld (S >= 0, row_stride >= C=%lld)", (long long)S,
               (long long)row_stride, (long long)C);
  if (S == 0 || a.n == 0) return BSMS_OK;
  BSMS_REQUIRE(owner && out && (fields || N == 0), BSMS_E_INVALID_ARG, "field_gather: null argument");
  a.m = Mesh{pos, pos_stride, N, tris, T};
  a.owner = owner, a.points = points, a.fields = fields;
  a.S = S, a.C = C, a.set_stride = set_stride, a.row_stride = row_stride;
  a.fill = fill, a.out = out;
  hipLaunchKernelGGL(k_field_gather, dim3(unsigned(ceil_div(a.n, kThreads))), dim3(kThreads), 0, as_stream(stream), a);
  BSMS_LAUNCH_CHECK();
  return BSMS_OK;
}
