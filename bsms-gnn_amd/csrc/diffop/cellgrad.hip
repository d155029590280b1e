// P1 gradients of nodal fields on a 2-D triangle complex (include/bsms_hip_diffop.h: bsms_cell_gradient, bsms_node_gradient,
// bsms_cell_gradient_sums, bsms_cell_gradient_bwd), built into the fifth companion library libbsms_hip_diffop.so: the
// surfaces of libbsms_hip.so and of the four other companions are closed.  One geometry function (load_geo: corners, A2, the edge
// normals) and one gradient function (normal) serve the four entries.  The per-triangle values are written by a thread per
// triangle; everything that lands on a node is added by the thread that owns the node, through the node -> triangle incidence in
// list order; the sums follow piece_sum.h.  No atomics anywhere.
// Compiled with -ffp-contract=off (build.py): every operation of the header's contract keeps its own fp64 rounding, which is what
// makes a NumPy restatement bit-comparable.
#include <algorithm>
#include <cmath>

#include "../piece_sum.h"
#include "../../../include/bsms_hip_diffop.h"

#pragma clang fp contract(off)

using namespace bsms;

namespace {

constexpr int kThreads = 256;                           // four waves of 64
constexpr int kPiece = 1024;                            // triangles of a segment per block of the sums: one per thread, sixteen waves
constexpr int kMaxCols = 1 + 2 * kMaxC + 4;             // A | GE | GT | DP DT WE WT
constexpr int kCellSets = 8;                            // sets a thread of k_cell_gradient walks with one triangle's geometry
constexpr int64_t kMaxGridY = 65535;
constexpr int kLongList = 32;                           // incidence entries above which a node is walked by its wave
constexpr int64_t kMaxIndex = (int64_t(1) << 31) - 2;   // N, T
constexpr int64_t kMaxBlocks = (int64_t(1) << 31) - 1;  // blocks of one launch
constexpr int64_t kMaxBlocksPerLaunch = int64_t(1) << 21;   // of 1024 threads: below the 2^32 work items of one dispatch

struct Mesh {
  const float* pos;
  int64_t pos_stride, N;
  const int32_t* tris;
  int64_t T;
};
struct Inc {
  const int32_t *ptr, *tri;
  int64_t nnz;
};
struct Field {                                          // f[s * set + n * row + c]
  const float* f;
  int64_t set, row;
};

struct Geo {
  int32_t n[3];
  double kx[3], ky[3];                                  // the edge normals of the corners
  double A2;                                            // orient(a, b, c)
};

// triangle t: its corners, A2 and the edge normals.  False for an invalid one; nothing is read from pos when it names a node outside
// [0, N)
__device__ __forceinline__ bool load_geo(const Mesh& m, int64_t t, Geo& g) {
  g.n[0] = m.tris[3 * t], g.n[1] = m.tris[3 * t + 1], g.n[2] = m.tris[3 * t + 2];
  if (g.n[0] < 0 || g.n[1] < 0 || g.n[2] < 0 || g.n[0] >= m.N || g.n[1] >= m.N || g.n[2] >= m.N) return false;
  const float *pa = m.pos + g.n[0] * m.pos_stride, *pb = m.pos + g.n[1] * m.pos_stride, *pc = m.pos + g.n[2] * m.pos_stride;
  const double ax = double(pa[0]), ay = double(pa[1]), bx = double(pb[0]), by = double(pb[1]), cx = double(pc[0]), cy = double(pc[1]);
  g.A2 = (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
  g.kx[0] = by - cy, g.kx[1] = cy - ay, g.kx[2] = ay - by;
  g.ky[0] = cx - bx, g.ky[1] = ax - cx, g.ky[2] = bx - ax;
  return g.A2 != 0.0 && isfinite(g.A2);                 // NaN fails the first test
}

// nx(f) or ny(f) of the contract from the three nodal values and kx or ky
__device__ __forceinline__ double normal(double fa, double fb, double fc, const double (&k)[3]) { return (fa * k[0] + fb * k[1]) + fc * k[2]; }

// the corner of g that is node n (the first one), or -1
__device__ __forceinline__ int corner_of(const Geo& g, int64_t n) { return g.n[0] == n ? 0 : g.n[1] == n ? 1 : g.n[2] == n ? 2 : -1; }

// entry q of node n's list: the triangle when it lies in [0, T), is valid and contains n (k: the corner)
__device__ __forceinline__ bool incident(const Mesh& m, const Inc& inc, int64_t q, int64_t n, Geo& g, int& k) {
  const int32_t t = inc.tri[q];
  if (t < 0 || t >= m.T) return false;
  const bool valid = load_geo(m, t, g);
  k = corner_of(g, n);
  return valid && k >= 0;
}

__device__ __forceinline__ void list_range(const Inc& inc, int64_t n, int64_t& q0, int64_t& q1) {
  q0 = std::max<int64_t>(inc.ptr[n], 0), q1 = std::min<int64_t>(inc.ptr[n + 1], inc.nnz);
}

// ------------------------------------------------------------------------------------------------------ cell gradient
struct CellArgs {
  Mesh m;
  Field f;
  int64_t S, sets;                                      // sets per block row (gridDim.y rows cover S)
  int C;
  float fill;
  float* out;
};

__global__ __launch_bounds__(kThreads) void k_cell_gradient(const CellArgs a) {
  const int64_t t = int64_t(blockIdx.x) * kThreads + int(threadIdx.x);
  if (t >= a.m.T) return;
  Geo g;
  const bool valid = load_geo(a.m, t, g);
  const int C = a.C;
  const int64_t s0 = int64_t(blockIdx.y) * a.sets, s1 = std::min(s0 + a.sets, a.S);
  for (int64_t s = s0; s < s1; ++s) {
    float2* out = reinterpret_cast<float2*>(a.out) + (s * a.m.T + t) * C;
    if (valid) {
      const float* f = a.f.f + s * a.f.set;
      const float *fa = f + g.n[0] * a.f.row, *fb = f + g.n[1] * a.f.row, *fc = f + g.n[2] * a.f.row;
      float va[kMaxC], vb[kMaxC], vc[kMaxC];
#pragma unroll
      for (int c = 0; c < kMaxC; ++c)
        if (c < C) va[c] = fa[c], vb[c] = fb[c], vc[c] = fc[c];
#pragma unroll
      for (int c = 0; c < kMaxC; ++c)
        if (c < C)
          out[c] = make_float2(float(normal(double(va[c]), double(vb[c]), double(vc[c]), g.kx) / g.A2),
                               float(normal(double(va[c]), double(vb[c]), double(vc[c]), g.ky) / g.A2));
    } else {
      for (int c = 0; c < C; ++c) out[c] = make_float2(a.fill, a.fill);
    }
  }
}

// ------------------------------------------------------------------------------------------------------ node gradient
struct NodeArgs {
  Mesh m;
  Inc inc;
  Field f;
  int64_t S, node_blocks;
  int C, long_list;
  float fill;
  float* out;
};

// node n, sets s0 .. s0 + NJ (those below S), channels c0 .. c0 + NC (those below C): the list once, in order
template <int NC, int NJ>
__device__ __forceinline__ void node_walk(const NodeArgs& a, int64_t n, int64_t s0, int c0, int64_t q0, int64_t q1) {
  double den = 0.0, numx[NJ][NC], numy[NJ][NC];
#pragma unroll
  for (int j = 0; j < NJ; ++j)
#pragma unroll
    for (int c = 0; c < NC; ++c) numx[j][c] = numy[j][c] = 0.0;
  bool any = false;
  for (int64_t q = q0; q < q1; ++q) {
    Geo g;
    int k;
    if (!incident(a.m, a.inc, q, n, g, k)) continue;
    any = true;
    den += fabs(g.A2);
    const double sg = g.A2 > 0.0 ? 1.0 : -1.0;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      if (s0 + j >= a.S) break;
      const float* f = a.f.f + (s0 + j) * a.f.set + c0;
      const float *fa = f + g.n[0] * a.f.row, *fb = f + g.n[1] * a.f.row, *fc = f + g.n[2] * a.f.row;
#pragma unroll
      for (int c = 0; c < NC; ++c) {
        if (c0 + c < a.C) {
          const double va = double(fa[c]), vb = double(fb[c]), vc = double(fc[c]);
          numx[j][c] += sg * normal(va, vb, vc, g.kx);
          numy[j][c] += sg * normal(va, vb, vc, g.ky);
        }
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j) {
    if (s0 + j >= a.S) break;
    float2* out = reinterpret_cast<float2*>(a.out) + ((s0 + j) * a.m.N + n) * a.C + c0;
#pragma unroll
    for (int c = 0; c < NC; ++c)
      if (c0 + c < a.C) out[c] = any ? make_float2(float(numx[j][c] / den), float(numy[j][c] / den)) : make_float2(a.fill, a.fill);
  }
}

// a thread per (node, group of NJ sets); the nodes of a wave whose lists are long are then walked by the wave, one after the other, a
// lane per (set, channel) of the group
template <int C, int NJ>
__global__ __launch_bounds__(kThreads) void k_node_gradient(const NodeArgs a) {
  static_assert(C * NJ <= 64, "a wave holds one lane per (set, channel) of a group");
  const int64_t blk = blockIdx.x, grp = blk / a.node_blocks, nb = blk - grp * a.node_blocks;
  const int lane = int(threadIdx.x) & 63;
  const int64_t n = nb * kThreads + int(threadIdx.x), s0 = grp * NJ;
  int64_t q0 = 0, q1 = 0;
  const bool live = n < a.m.N;
  if (live) list_range(a.inc, n, q0, q1);
  const bool lng = live && q1 - q0 > a.long_list;
  if (live && !lng) node_walk<C, NJ>(a, n, s0, 0, q0, q1);
  unsigned long long todo = __ballot(lng);
  while (todo) {                                        // wave-uniform
    const int src = __ffsll(todo) - 1;
    todo &= todo - 1;
    const int64_t ns = n - lane + src;                  // the node of lane `src`: every lane reads its range again (one cached address)
    int64_t r0, r1;
    list_range(a.inc, ns, r0, r1);
    if (lane < C * NJ) node_walk<1, 1>(a, ns, s0 + lane / C, lane % C, r0, r1);
  }
}

// ------------------------------------------------------------------------------------------------------ sums and their adjoint
struct SumArgs {
  Mesh m;
  Inc inc;                                              // the adjoint only
  Field pred, target;
  const float* mask;                                    // null: 1
  int64_t mask_stride, S, pieces, blk0;
  int cu, cv;                                           // cu < 0: no velocity pair
};

__device__ __forceinline__ double mask_product(const SumArgs& a, int64_t s, const Geo& g) {
  if (!a.mask) return 1.0;
  const float* m = a.mask + s * a.mask_stride;
  return (double(m[g.n[0]]) * double(m[g.n[1]])) * double(m[g.n[2]]);
}

// the nodal values of channel c at the three corners: d = fl32(pred - target), t = target, p = pred
struct Corner3 {
  double d[3], t[3], p[3];
};
__device__ __forceinline__ Corner3 load_corners(const SumArgs& a, int64_t s, const Geo& g, int c) {
  Corner3 v;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float p = a.pred.f[s * a.pred.set + g.n[k] * a.pred.row + c], t = a.target.f[s * a.target.set + g.n[k] * a.target.row + c];
    v.d[k] = double(p - t), v.t[k] = double(t), v.p[k] = double(p);
  }
  return v;
}

template <int C>
__global__ __launch_bounds__(kPiece) void k_cell_pieces(const SumArgs a, double* __restrict__ partials) {
  constexpr int ncol = 1 + 2 * C + 4;
  const psum::Split at = psum::split(a.blk0, a.pieces);
  const int64_t s = at.seg, t = at.piece * kPiece + int(threadIdx.x);     // triangle inside the segment's mesh
  double acc[ncol];
#pragma unroll
  for (int k = 0; k < ncol; ++k) acc[k] = 0.0;
  Geo g;
  if (t < a.m.T && load_geo(a.m, t, g)) {
    const double w = mask_product(a, s, g) * (fabs(g.A2) * 0.5);
    acc[0] = w;
    double pux = 0.0, pvy = 0.0, tux = 0.0, tuy = 0.0, tvx = 0.0, tvy = 0.0, duy = 0.0, dvx = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const Corner3 v = load_corners(a, s, g, c);
      const double dx = normal(v.d[0], v.d[1], v.d[2], g.kx) / g.A2, dy = normal(v.d[0], v.d[1], v.d[2], g.ky) / g.A2;
      const double tx = normal(v.t[0], v.t[1], v.t[2], g.kx) / g.A2, ty = normal(v.t[0], v.t[1], v.t[2], g.ky) / g.A2;
      acc[1 + c] = w * (dx * dx + dy * dy);
      acc[1 + C + c] = w * (tx * tx + ty * ty);
      if (c == a.cu) pux = normal(v.p[0], v.p[1], v.p[2], g.kx) / g.A2, tux = tx, tuy = ty, duy = dy;
      if (c == a.cv) pvy = normal(v.p[0], v.p[1], v.p[2], g.ky) / g.A2, tvx = tx, tvy = ty, dvx = dx;
    }
    if (a.cu >= 0) {
      const double divp = pux + pvy, divt = tux + tvy, curld = dvx - duy, curlt = tvx - tuy;
      acc[1 + 2 * C] = w * (divp * divp);
      acc[2 + 2 * C] = w * (divt * divt);
      acc[3 + 2 * C] = w * (curld * curld);
      acc[4 + 2 * C] = w * (curlt * curlt);
    }
  }
  psum::block_sum<kPiece>(acc, psum::Dense<ncol>(), partials + at.blk * ncol);
}

// thread (s, n): the header's accumulation over n's list, then grad[s, n, :] = fl32(2 acc)
template <int C>
__global__ __launch_bounds__(kThreads) void k_cell_bwd(const SumArgs a, const double* __restrict__ coef, int accumulate,
                                                      float* __restrict__ grad, int64_t grad_stride) {
  const psum::Split at = psum::split(a.blk0, a.pieces);
  const int64_t s = at.seg, n = at.piece * kThreads + int(threadIdx.x);
  if (n >= a.m.N) return;
  double kc[C], acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) kc[c] = coef[s * (C + 2) + c], acc[c] = 0.0;
  const double kD = coef[s * (C + 2) + C], kW = coef[s * (C + 2) + C + 1];
  int64_t q0, q1;
  list_range(a.inc, n, q0, q1);
  for (int64_t q = q0; q < q1; ++q) {
    Geo g;
    int k;
    if (!incident(a.m, a.inc, q, n, g, k)) continue;
    const double w = mask_product(a, s, g) * (fabs(g.A2) * 0.5);
    const double bx = (k == 0 ? g.kx[0] : k == 1 ? g.kx[1] : g.kx[2]) / g.A2, by = (k == 0 ? g.ky[0] : k == 1 ? g.ky[1] : g.ky[2]) / g.A2;
    double pux = 0.0, pvy = 0.0, duy = 0.0, dvx = 0.0;
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const Corner3 v = load_corners(a, s, g, c);
      const double dx = normal(v.d[0], v.d[1], v.d[2], g.kx) / g.A2, dy = normal(v.d[0], v.d[1], v.d[2], g.ky) / g.A2;
      acc[c] += (w * kc[c]) * (dx * bx + dy * by);
      if (c == a.cu) pux = normal(v.p[0], v.p[1], v.p[2], g.kx) / g.A2, duy = dy;
      if (c == a.cv) pvy = normal(v.p[0], v.p[1], v.p[2], g.ky) / g.A2, dvx = dx;
    }
    if (a.cu >= 0) {
      const double divp = pux + pvy, curld = dvx - duy;
      const double du = (w * kD) * (divp * bx), dv = (w * kD) * (divp * by);
      const double wu = (w * kW) * (curld * (-by)), wv = (w * kW) * (curld * bx);
#pragma unroll
      for (int c = 0; c < C; ++c) {
        if (c == a.cu) acc[c] = (acc[c] + du) + wu;
        if (c == a.cv) acc[c] = (acc[c] + dv) + wv;
      }
    }
  }
  float* out = grad + (s * grad_stride + n) * C;
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const float v = float(2.0 * acc[c]);                // the one rounding to fp32
    out[c] = accumulate ? out[c] + v : v;
  }
}

// ------------------------------------------------------------------------------------------------------ checks
int check_mesh(const char* who, const float* pos, int64_t pos_stride, int64_t N, const int32_t* tris, int64_t T) {
  BSMS_REQUIRE(N >= 0 && T >= 0 && pos_stride >= 2, BSMS_E_INVALID_ARG, "%s: N=%lld T=%lld pos_stride=%lld (N, T >= 0, pos_stride >= 2)", who,
               (long long)N, (long long)T, (long long)pos_stride);
  BSMS_REQUIRE(N <= kMaxIndex && T <= kMaxIndex, BSMS_E_SHAPE, "%s: N=%lld T=%lld (at most 2^31 - 2)", who, (long long)N, (long long)T);
  BSMS_REQUIRE((pos || N == 0) && (tris || T == 0), BSMS_E_INVALID_ARG, "%s: null mesh argument", who);
  return BSMS_OK;
}

int check_channels(const char* who, int64_t C) {
  BSMS_REQUIRE(C >= 1 && C <= kMaxC, BSMS_E_UNSUPPORTED, "%s: C=%lld (C in 1..8)", who, (long long)C);
  return BSMS_OK;
}

int check_inc(const char* who, const int32_t* inc_ptr, const int32_t* inc_tri, int64_t nnz, int64_t N) {
  BSMS_REQUIRE(nnz >= 0 && nnz <= INT32_MAX, BSMS_E_INVALID_ARG, "%s: nnz=%lld (0..2^31 - 1)", who, (long long)nnz);
  BSMS_REQUIRE((inc_ptr || N == 0) && (inc_tri || nnz == 0), BSMS_E_INVALID_ARG, "%s: null incidence argument", who);
  return BSMS_OK;
}

// the checks the sums and their adjoint share; fills `a`
int sum_args(const char* who, const float* pos, int64_t pos_stride, int64_t N, const int32_t* tris, int64_t T, const float* pred,
             int64_t pred_set_stride, int64_t pred_row_stride, const float* target, int64_t target_set_stride, int64_t target_row_stride,
             const float* mask, int64_t mask_stride, int64_t S, int64_t C, int64_t cu, int64_t cv, SumArgs* a) {
  if (int rc = check_channels(who, C)) return rc;
  if (int rc = check_mesh(who, pos, pos_stride, N, tris, T)) return rc;
  BSMS_REQUIRE(S >= 0 && pred_row_stride >= C && target_row_stride >= C && mask_stride >= 0, BSMS_E_INVALID_ARG,
               "%s: S=%lld pred_row_stride=%lld target_row_stride=%lld mask_stride=%lld (S, mask_stride >= 0, row strides >= C=%lld)", who,
               (long long)S, (long long)pred_row_stride, (long long)target_row_stride, (long long)mask_stride, (long long)C);
  BSMS_REQUIRE(cu < 0 || (cu < C && cv >= 0 && cv < C && cu != cv), BSMS_E_INVALID_ARG, "%s: velocity pair (%lld, %lld) of C=%lld channels", who,
               (long long)cu, (long long)cv, (long long)C);
  BSMS_REQUIRE((pred && target) || N == 0 || S == 0, BSMS_E_INVALID_ARG, "%s: null argument", who);
  a->m = Mesh{pos, pos_stride, N, tris, T};
  a->inc = Inc{nullptr, nullptr, 0};
  a->pred = Field{pred, pred_set_stride, pred_row_stride};
  a->target = Field{target, target_set_stride, target_row_stride};
  a->mask = mask, a->mask_stride = mask_stride, a->S = S, a->pieces = 0, a->blk0 = 0;
  a->cu = cu < 0 ? -1 : int(cu), a->cv = cu < 0 ? -1 : int(cv);
  return BSMS_OK;
}

template <int C>
constexpr int sets_per_thread() { return C <= 2 ? 8 : C <= 4 ? 4 : 2; }

}  // namespace

extern "C" int bsms_cell_gradient(const float* pos, int64_t pos_stride, int64_t N, const int32_t* tris, int64_t T, const float* fields,
                                  int64_t S, int64_t C, int64_t set_stride, int64_t row_stride, float fill, float* out, bsms_stream_t stream) {
  if (int rc = check_channels("cell_gradient", C)) return rc;
  if (int rc = check_mesh("cell_gradient", pos, pos_stride, N, tris, T)) return rc;
  BSMS_REQUIRE(S >= 0 && row_stride >= C, BSMS_E_INVALID_ARG, "cell_gradient: S=%lld row_stride=%lld (S >= 0, row_stride >= C=%lld)", (long long)S,
               (long long)row_stride, (long long)C);
  if (S == 0 || T == 0) return BSMS_OK;
  BSMS_REQUIRE(out && (fields || N == 0), BSMS_E_INVALID_ARG, "cell_gradient: null argument");
  const int64_t sets = std::max<int64_t>(kCellSets, ceil_div(S, kMaxGridY));    // the geometry once per kCellSets sets; gridDim.y <= 65535
  const CellArgs a{Mesh{pos, pos_stride, N, tris, T}, Field{fields, set_stride, row_stride}, S, sets, int(C), fill, out};
  hipLaunchKernelGGL(k_cell_gradient, dim3(unsigned(ceil_div(T, kThreads)), unsigned(ceil_div(S, sets))), dim3(kThreads), 0, as_stream(stream), a);
  BSMS_LAUNCH_CHECK();
  return BSMS_OK;
}

extern "C" int bsms_node_gradient(const float* pos, int64_t pos_stride, int64_t N, const int32_t* tris, int64_t T, const int32_t* inc_ptr,
                                  const int32_t* inc_tri, int64_t nnz, const float* fields, int64_t S, int64_t C, int64_t set_stride,
                                  int64_t row_stride, float fill, int64_t long_list, float* out, bsms_stream_t stream) {
  if (int rc = check_channels("node_gradient", C)) return rc;
  if (int rc = check_mesh("node_gradient", pos, pos_stride, N, tris, T)) return rc;
  if (int rc = check_inc("node_gradient", inc_ptr, inc_tri, nnz, N)) return rc;
  BSMS_REQUIRE(S >= 0 && row_stride >= C, BSMS_E_INVALID_ARG, "node_gradient: S=%lld row_stride=%lld (S >= 0, row_stride >= C=%lld)", (long long)S,
               (long long)row_stride, (long long)C);
  if (S == 0 || N == 0) return BSMS_OK;
  BSMS_REQUIRE(out && fields, BSMS_E_INVALID_ARG, "node_gradient: null argument");
  NodeArgs a{Mesh{pos, pos_stride, N, tris, T}, Inc{inc_ptr, inc_tri, nnz}, Field{fields, set_stride, row_stride}, S, ceil_div(N, kThreads),
             int(C), long_list <= 0 ? kLongList : int(std::min<int64_t>(long_list, INT32_MAX)), fill, out};
  int rc = BSMS_OK;
  psum::by_channels(int(C), [&](auto c) {
    constexpr int Cc = decltype(c)::value, NJ = sets_per_thread<Cc>();
    const int64_t blocks = ceil_div(S, NJ) * a.node_blocks;
    if (blocks > kMaxBlocks) {
      set_error("node_gradient: S=%lld sets of N=%lld nodes exceed one launch", (long long)S, (long long)N);
      rc = BSMS_E_UNSUPPORTED;
      return;
    }
    hipLaunchKernelGGL((k_node_gradient<Cc, NJ>), dim3(unsigned(blocks)), dim3(kThreads), 0, as_stream(stream), a);
  });
  if (rc) return rc;
  BSMS_LAUNCH_CHECK();
  return BSMS_OK;
}

extern "C" size_t bsms_cell_gradient_work_bytes(int64_t S, int64_t T) {
  if (S < 0 || T < 0) return 0;
  return size_t(std::max<int64_t>(S, 1)) * size_t(std::max<int64_t>(ceil_div(T, kPiece), 1)) * kMaxCols * sizeof(double) + 256;
}

extern "C" int bsms_cell_gradient_sums(const float* pos, int64_t pos_stride, int64_t N, const int32_t* tris, int64_t T, const float* pred,
                                       int64_t pred_set_stride, int64_t pred_row_stride, const float* target, int64_t target_set_stride,
                                       int64_t target_row_stride, const float* mask, int64_t mask_stride, int64_t S, int64_t C, int64_t cu,
                                       int64_t cv, double* sums, void* work, bsms_stream_t stream) {
  SumArgs a;
  if (int rc = sum_args("cell_gradient_sums", pos, pos_stride, N, tris, T, pred, pred_set_stride, pred_row_stride, target, target_set_stride,
                        target_row_stride, mask, mask_stride, S, C, cu, cv, &a))
    return rc;
  if (S == 0) return BSMS_OK;
  a.pieces = ceil_div(T, kPiece);
  BSMS_REQUIRE(sums && (a.pieces == 0 || work), BSMS_E_INVALID_ARG, "cell_gradient_sums: null argument");
  const int ncol = 1 + 2 * int(C) + 4;
  // the finishing kernel runs one thread per output element in one dispatch
  BSMS_REQUIRE(S <= (int64_t(1) << 30) / ncol, BSMS_E_UNSUPPORTED, "cell_gradient_sums: S=%lld segments of %d sums exceed one dispatch", (long long)S,
               ncol);
  hipStream_t s = as_stream(stream);
  double* partials = reinterpret_cast<double*>(work);
  const int rc = psum::for_block_slices(S * a.pieces, kMaxBlocksPerLaunch, [&](int64_t first, unsigned nb) {
    a.blk0 = first;
    psum::by_channels(int(C), [&](auto c) { hipLaunchKernelGGL((k_cell_pieces<decltype(c)::value>), dim3(nb), dim3(kPiece), 0, s, a, partials); });
  });
  if (rc) return rc;
  psum::launch_finish(partials, S, a.pieces, ncol, ncol, sums, s);
  BSMS_LAUNCH_CHECK();
  return BSMS_OK;
}

extern "C" int bsms_cell_gradient_bwd(const float* pos, int64_t pos_stride, int64_t N, const int32_t* tris, int64_t T, const int32_t* inc_ptr,
                                      const int32_t* inc_tri, int64_t nnz, const float* pred, int64_t pred_set_stride, int64_t pred_row_stride,
                                      const float* target, int64_t target_set_stride, int64_t target_row_stride, const float* mask,
                                      int64_t mask_stride, int64_t S, int64_t C, int64_t cu, int64_t cv, const double* coef, int accumulate,
                                      float* grad, int64_t grad_stride, bsms_stream_t stream) {
  SumArgs a;
  if (int rc = sum_args("cell_gradient_bwd", pos, pos_stride, N, tris, T, pred, pred_set_stride, pred_row_stride, target, target_set_stride,
                        target_row_stride, mask, mask_stride, S, C, cu, cv, &a))
    return rc;
  if (int rc = check_inc("cell_gradient_bwd", inc_ptr, inc_tri, nnz, N)) return rc;
  BSMS_REQUIRE(grad_stride >= N, BSMS_E_INVALID_ARG, "cell_gradient_bwd: grad_stride=%lld is shorter than a segment (%lld rows)",
               (long long)grad_stride, (long long)N);
  if (S == 0 || N == 0) return BSMS_OK;
  BSMS_REQUIRE(coef && grad, BSMS_E_INVALID_ARG, "cell_gradient_bwd: null argument");
  a.inc = Inc{inc_ptr, inc_tri, nnz};
  a.pieces = ceil_div(N, kThreads);                      // blocks per segment: one thread per node
  hipStream_t s = as_stream(stream);
  return psum::for_block_slices(S * a.pieces, kMaxBlocksPerLaunch * (kPiece / kThreads), [&](int64_t first, unsigned nb) {
    a.blk0 = first;
    psum::by_channels(int(C), [&](auto c) {
      hipLaunchKernelGGL((k_cell_bwd<decltype(c)::value>), dim3(nb), dim3(kThreads), 0, s, a, coef, accumulate, grad, grad_stride);
    });
  });
}
