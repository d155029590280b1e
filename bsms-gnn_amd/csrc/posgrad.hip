// Gradients w.r.t. narrow inputs: the node positions of a GMP block (the fiber [pos_i - pos_j, |pos_i - pos_j|] of
// ops/basic.py:77-85 is the only place `pos` enters the block) and the input of an MLP whose first Linear is narrow
// (the encoder, models/model.py:20; ops/basic.py:6-23).  Both are one transposed product with the narrow columns of a
// first Linear:
//     t[r][c] = sum_f G[r][f] * W[f][c],   c < K <= 8
// where G [R, D] is the gradient at that Linear's output (after the ReLU mask).  For a GMP block, edge e = (i -> j) in
// plan order, G = gE[0], W = the fiber columns of mlp_edge.seq.0.weight (K = p + 1), r_e = pos_i - pos_j, n_e = |r_e|:
//     d r_e   = t[0:p] + r_e * (t[p] / n_e)          (0 instead of the norm term where n_e == 0: torch's norm backward)
//     gpos[i] += d r_e,   gpos[j] -= d r_e
// k_narrow_t streams G once (HBM-bound: R * D * 4 bytes, bf16 rows half that) and writes t (MLP input) or d r_e (GMP);
// k_pos_node gathers d r_e per node in a fixed order (sources through the transpose CSR, then targets in plan order)
// and, for a position tensor shared by the batch, sums the batch items in order.  No atomics: run-to-run bit-identical.
#include "chain.h"

using namespace bsms;

namespace {

struct NarrowArgs {
  const float* G;        // [R, D] rows: fp32, or bf16 (XBF)
  const float* W;        // [D, ldw] row-major: columns 0..K-1 are used
  int ldw;
  int64_t R;
  const float* fiber;    // POS: [R, fld] the fiber rows the forward kept ([r_e, n_e, 0 ...])
  float* out;            // POS: [R, fld] d r_e (padding columns zero); otherwise [R, K]
  int fld;
};

template <bool XBF>
__device__ __forceinline__ float4 ld_row4(const float* base, int64_t e) {   // four features at ELEMENT offset e
  if (XBF) {
    const uint2 u = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned short*>(base) + e);
    return make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xffff0000u), __uint_as_float(u.y << 16),
                       __uint_as_float(u.y & 0xffff0000u));
  }
  return *reinterpret_cast<const float4*>(base + e);
}

// LPR lanes per row, each owning NF4 float4 column groups (lane + i * LPR): one 256-byte segment per 16 lanes and
// instruction.  The lane's W entries stay in registers for the whole grid-stride loop.
template <int LPR, int NF4, int K, bool XBF, bool POS>
__global__ __launch_bounds__(256) void k_narrow_t(NarrowArgs a) {
  constexpr int D = 4 * LPR * NF4;
  constexpr int RPB = 256 / LPR;   // rows per workgroup and pass
  const int lane = threadIdx.x % LPR;
  float w[NF4][4][K];
#pragma unroll
  for (int i = 0; i < NF4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int c = 0; c < K; ++c) w[i][j][c] = a.W[int64_t((i * LPR + lane) * 4 + j) * a.ldw + c];
  const int64_t stride = int64_t(gridDim.x) * RPB;
  for (int64_t r = int64_t(blockIdx.x) * RPB + threadIdx.x / LPR; r < a.R; r += stride) {
    float4 v[NF4];
#pragma unroll
    for (int i = 0; i < NF4; ++i) v[i] = ld_row4<XBF>(a.G, r * D + (i * LPR + lane) * 4);
    float t[K];
#pragma unroll
    for (int c = 0; c < K; ++c) t[c] = 0.f;
#pragma unroll
    for (int i = 0; i < NF4; ++i)
#pragma unroll
      for (int c = 0; c < K; ++c) {
        t[c] = fmaf(v[i].x, w[i][0][c], t[c]);
        t[c] = fmaf(v[i].y, w[i][1][c], t[c]);
        t[c] = fmaf(v[i].z, w[i][2][c], t[c]);
        t[c] = fmaf(v[i].w, w[i][3][c], t[c]);
      }
    // butterfly over the LPR lanes of the row (they are active together: same r); fixed order
#pragma unroll
    for (int off = LPR / 2; off > 0; off >>= 1)
#pragma unroll
      for (int c = 0; c < K; ++c) t[c] += __shfl_xor(t[c], off, LPR);
    if (lane != 0) continue;
    if (POS) {
      constexpr int P = K - 1;
      const float* f = a.fiber + r * a.fld;
      const float n = f[P];
      const float s = n > 0.f ? t[P] / n : 0.f;
      float d[8];
#pragma unroll
      for (int c = 0; c < 8; ++c) d[c] = c < P ? fmaf(f[c], s, t[c < P ? c : 0]) : 0.f;
      float4* o = reinterpret_cast<float4*>(a.out + r * a.fld);
      o[0] = make_float4(d[0], d[1], d[2], d[3]);
      if (P >= 4) o[1] = make_float4(d[4], d[5], d[6], d[7]);
    } else {
#pragma unroll
      for (int c = 0; c < K; ++c) a.out[r * K + c] = t[c];
    }
  }
}

struct PosNodeArgs {
  const int32_t *rowptr, *t_rowptr, *t_pos;   // plan: targets (plan order), sources (transpose CSR -> plan slot)
  const float* dr;                            // [B, E, FLD] d r_e in plan order
  float* out;                                 // [B, N, p] or, shared, [N, p]
  int32_t N, E, B, p;
  int accumulate;                             // out += instead of out =
};

template <int FLD>
__device__ __forceinline__ void add_row(float (&acc)[FLD], const float* row) {
  const float4 a = *reinterpret_cast<const float4*>(row);
  acc[0] += a.x; acc[1] += a.y; acc[2] += a.z; acc[3] += a.w;
  if (FLD == 8) {
    const float4 b = *reinterpret_cast<const float4*>(row + 4);
    acc[FLD == 8 ? 4 : 0] += b.x; acc[FLD == 8 ? 5 : 1] += b.y; acc[FLD == 8 ? 6 : 2] += b.z; acc[FLD == 8 ? 7 : 3] += b.w;
  }
}

// one thread per output row (b, n) -- or per node n with the batch summed in order when the positions are shared
template <int FLD, bool SHARED>
__global__ __launch_bounds__(256) void k_pos_node(PosNodeArgs a) {
  const int64_t t = int64_t(blockIdx.x) * 256 + threadIdx.x;
  if (t >= (SHARED ? int64_t(a.N) : int64_t(a.B) * a.N)) return;
  const int n = int(t % a.N);
  const int b0 = SHARED ? 0 : int(t / a.N), b1 = SHARED ? a.B : b0 + 1;
  float tot[FLD];
#pragma unroll
  for (int c = 0; c < FLD; ++c) tot[c] = 0.f;
  const int s0 = a.t_rowptr[n], s1 = a.t_rowptr[n + 1], d0 = a.rowptr[n], d1 = a.rowptr[n + 1];
  for (int b = b0; b < b1; ++b) {
    const float* base = a.dr + int64_t(b) * a.E * FLD;
    float sp[FLD], sm[FLD];
#pragma unroll
    for (int c = 0; c < FLD; ++c) sp[c] = sm[c] = 0.f;
#pragma unroll 4
    for (int q = s0; q < s1; ++q) add_row<FLD>(sp, base + int64_t(a.t_pos[q]) * FLD);   // edges leaving n: + d r_e
#pragma unroll 4
    for (int q = d0; q < d1; ++q) add_row<FLD>(sm, base + int64_t(q) * FLD);            // edges entering n: - d r_e
#pragma unroll
    for (int c = 0; c < FLD; ++c) tot[c] += sp[c] - sm[c];
  }
  float* o = a.out + (SHARED ? 0 : int64_t(b0) * a.N * a.p) + int64_t(n) * a.p;
#pragma unroll
  for (int c = 0; c < FLD; ++c)
    if (c < a.p) o[c] = a.accumulate ? o[c] + tot[c] : tot[c];
}

int narrow_grid(int64_t R, int rpb) {
  return (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(R, rpb), int64_t(device_cu_count()) * 16));
}

template <int K, bool XBF, bool POS>
int launch_narrow_k(const NarrowArgs& a, int64_t D, hipStream_t s) {
  switch (D) {
    case 32: hipLaunchKernelGGL((k_narrow_t<8, 1, K, XBF, POS>), dim3(narrow_grid(a.R, 32)), dim3(256), 0, s, a); break;
    case 64: hipLaunchKernelGGL((k_narrow_t<16, 1, K, XBF, POS>), dim3(narrow_grid(a.R, 16)), dim3(256), 0, s, a); break;
    case 128: hipLaunchKernelGGL((k_narrow_t<16, 2, K, XBF, POS>), dim3(narrow_grid(a.R, 16)), dim3(256), 0, s, a); break;
    case 256: hipLaunchKernelGGL((k_narrow_t<16, 4, K, XBF, POS>), dim3(narrow_grid(a.R, 16)), dim3(256), 0, s, a); break;
    default:
      if constexpr (!XBF) {   // fp32 rows at the other multiples of 32: 8 lanes x 4 x NF4 features (16 x 4 x 3 at 192)
        if (D == 96) { hipLaunchKernelGGL((k_narrow_t<8, 3, K, XBF, POS>), dim3(narrow_grid(a.R, 32)), dim3(256), 0, s, a); break; }
        if (D == 160) { hipLaunchKernelGGL((k_narrow_t<8, 5, K, XBF, POS>), dim3(narrow_grid(a.R, 32)), dim3(256), 0, s, a); break; }
        if (D == 192) { hipLaunchKernelGGL((k_narrow_t<16, 3, K, XBF, POS>), dim3(narrow_grid(a.R, 16)), dim3(256), 0, s, a); break; }
        if (D == 224) { hipLaunchKernelGGL((k_narrow_t<8, 7, K, XBF, POS>), dim3(narrow_grid(a.R, 32)), dim3(256), 0, s, a); break; }
      }
      BSMS_FAIL(BSMS_E_UNSUPPORTED, "narrow input gradient: D=%lld (fp32 rows: multiples of 32 up to 256; bf16 rows: 32, 64, 128, 256)", (long long)D);
  }
  BSMS_LAUNCH_CHECK();
  return BSMS_OK;
}

}  // namespace

namespace bsms {

size_t pos_edge_scratch_bytes(int64_t B, int64_t E, int64_t p) { return align_up(size_t(B) * E * fiber_ld(p) * sizeof(float)); }

int gmp_pos_grad(const bsms_plan* plan, const void* gE0, bool g_bf16, const float* fiber, const float* W0_edge, int64_t B,
                 int64_t D, int64_t p, int64_t pos_bstride, float* grad_pos, bool accumulate, float* scratch, hipStream_t s) {
  BSMS_REQUIRE(p >= 1 && p <= 7, BSMS_E_INVALID_ARG, "gmp position gradient: pos_dim=%lld (1..7)", (long long)p);
  BSMS_REQUIRE(!g_bf16 || ((D == 128 || D == 256) && p <= 3), BSMS_E_UNSUPPORTED, "gmp position gradient: bf16 rows need D = 128 / 256, pos_dim <= 3");
  const int64_t E = plan->E, N = plan->N, R = B * E;
  const int fld = fiber_ld(p);
  if (R > 0) {
    NarrowArgs a{};
    a.G = reinterpret_cast<const float*>(gE0); a.W = W0_edge; a.ldw = int(2 * D + p + 1); a.R = R;
    a.fiber = fiber; a.out = scratch; a.fld = fld;
    int rc;
    if (g_bf16) {   // the bf16 precisions store gE[0] as bf16 rows (efuse.hip / chain.hip)
      switch (p + 1) {
        case 2: rc = launch_narrow_k<2, true, true>(a, D, s); break;
        case 3: rc = launch_narrow_k<3, true, true>(a, D, s); break;
        default: rc = launch_narrow_k<4, true, true>(a, D, s); break;
      }
    } else {
      switch (p + 1) {
        case 2: rc = launch_narrow_k<2, false, true>(a, D, s); break;
        case 3: rc = launch_narrow_k<3, false, true>(a, D, s); break;
        case 4: rc = launch_narrow_k<4, false, true>(a, D, s); break;
        case 5: rc = launch_narrow_k<5, false, true>(a, D, s); break;
        case 6: rc = launch_narrow_k<6, false, true>(a, D, s); break;
        case 7: rc = launch_narrow_k<7, false, true>(a, D, s); break;
        default: rc = launch_narrow_k<8, false, true>(a, D, s); break;
      }
    }
    if (rc) return rc;
  }
  const bool shared = pos_bstride == 0;
  const int64_t threads = shared ? N : B * N;
  if (threads == 0) return BSMS_OK;
  if (shared && B == 0) {   // nothing to sum: the gradient of a shared position tensor is zero
    if (!accumulate) BSMS_HIP_CHECK(hipMemsetAsync(grad_pos, 0, size_t(N) * p * sizeof(float), s));
    return BSMS_OK;
  }
  PosNodeArgs n{};
  n.rowptr = plan->rowptr; n.t_rowptr = plan->t_rowptr; n.t_pos = plan->t_pos;
  n.dr = scratch; n.out = grad_pos;
  n.N = (int32_t)N; n.E = (int32_t)E; n.B = (int32_t)B; n.p = (int32_t)p; n.accumulate = accumulate ? 1 : 0;
  const dim3 grid((unsigned)ceil_div(threads, 256));
  if (fld == 4) {
    if (shared) hipLaunchKernelGGL((k_pos_node<4, true>), grid, dim3(256), 0, s, n);
    else hipLaunchKernelGGL((k_pos_node<4, false>), grid, dim3(256), 0, s, n);
  } else {
    if (shared) hipLaunchKernelGGL((k_pos_node<8, true>), grid, dim3(256), 0, s, n);
    else hipLaunchKernelGGL((k_pos_node<8, false>), grid, dim3(256), 0, s, n);
  }
  BSMS_LAUNCH_CHECK();
  return BSMS_OK;
}

int narrow_input_grad(const float* G, int64_t R, int64_t D, const float* W, int K, float* out, hipStream_t s) {
  if (R == 0) return BSMS_OK;
  NarrowArgs a{};
  a.G = G; a.W = W; a.ldw = K; a.R = R; a.out = out;
  switch (K) {
    case 1: return launch_narrow_k<1, false, false>(a, D, s);
    case 2: return launch_narrow_k<2, false, false>(a, D, s);
    case 3: return launch_narrow_k<3, false, false>(a, D, s);
    case 4: return launch_narrow_k<4, false, false>(a, D, s);
    case 5: return launch_narrow_k<5, false, false>(a, D, s);
    case 6: return launch_narrow_k<6, false, false>(a, D, s);
    case 7: return launch_narrow_k<7, false, false>(a, D, s);
    case 8: return launch_narrow_k<8, false, false>(a, D, s);
    default: BSMS_FAIL(BSMS_E_UNSUPPORTED, "narrow input gradient: in_dim=%d (1..8)", K);
  }
}

// Bias gradient of a Linear whose output goes through LayerNorm (no affine), from fp32: db[f] = sum_r g[r][f] with the LayerNorm
// backward g[r] = rstd_r (dy[r] - mean(dy[r]) - yln[r] mean(dy[r] yln[r])).  BSMS_BF16_NODES stores that gradient as bf16 rows for the
// weight-gradient products; a column sum of the rounded rows sits 2^-9 from the fp32 one at any depth (the roundings do not
// average out against a sum that cancels), so the bias takes this sum of the unrounded rows instead (gmp.hip: GmpBwd::node_chain).
// Two launches in a fixed order, no atomics: run-to-run bit-identical.  Streams dy and yln once (HBM-bound: R * D * 8 bytes).
namespace {
constexpr int kLnBiasMaxBlocks = 128;   // partial rows: the second launch adds them in 128 / 8 (D = 128) or 128 / 4 dependent steps

struct LnBiasArgs {
  const float *dy, *yln, *rstd;   // [R, D], [R, D], [R]
  int64_t R;
  float* part;                    // [gridDim.x, D] one partial row per workgroup
  float* db;                      // [D]
  int nblk;
};

template <int LPR>   // lanes per row = D / 4 (32 or 64): a wave takes 64 / LPR rows per pass
__global__ __launch_bounds__(256) void k_ln_bias_part(LnBiasArgs a) {
  constexpr int RPW = 64 / LPR, D = 4 * LPR;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane / LPR, l = lane % LPR;
  const int64_t step = int64_t(gridDim.x) * 4 * RPW;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
  for (int64_t r0 = (int64_t(blockIdx.x) * 4 + wave) * RPW; r0 < a.R; r0 += step) {   // r0 is uniform over the wave: every lane reaches the shuffles
    const int64_t r = r0 + sub;
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f), y = g;
    float rs = 0.f;
    if (r < a.R) {
      g = *reinterpret_cast<const float4*>(a.dy + r * D + 4 * l);
      y = *reinterpret_cast<const float4*>(a.yln + r * D + 4 * l);
      rs = a.rstd[r];
    }
    float s1 = (g.x + g.y) + (g.z + g.w), s2 = (g.x * y.x + g.y * y.y) + (g.z * y.z + g.w * y.w);
#pragma unroll
    for (int m = LPR / 2; m >= 1; m >>= 1) {
      s1 += __shfl_xor(s1, m, LPR);
      s2 += __shfl_xor(s2, m, LPR);
    }
    s1 *= 1.f / D;
    s2 *= 1.f / D;
    acc.x += rs * (g.x - s1 - y.x * s2);
    acc.y += rs * (g.y - s1 - y.y * s2);
    acc.z += rs * (g.z - s1 - y.z * s2);
    acc.w += rs * (g.w - s1 - y.w * s2);
  }
  __shared__ float4 sh[256];
  sh[threadIdx.x] = acc;
  __syncthreads();
  if (threadIdx.x < LPR) {   // waves, then row slots, in order
    float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int w = 0; w < 4; ++w)
      for (int q = 0; q < RPW; ++q) {
        const float4 v = sh[w * 64 + q * LPR + threadIdx.x];
        t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
      }
    *reinterpret_cast<float4*>(a.part + int64_t(blockIdx.x) * D + 4 * threadIdx.x) = t;
  }
}

template <int LPR>   // 256 / LPR groups of threads take the partial rows in turn, then the groups are added in order
__global__ __launch_bounds__(256) void k_ln_bias_sum(LnBiasArgs a) {
  constexpr int G = 256 / LPR, D = 4 * LPR;
  const int q = threadIdx.x / LPR, l = threadIdx.x % LPR;
  float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll 4
  for (int b = q; b < a.nblk; b += G) {
    const float4 v = *reinterpret_cast<const float4*>(a.part + int64_t(b) * D + 4 * l);
    t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
  }
  __shared__ float4 sh[256];
  sh[threadIdx.x] = t;
  __syncthreads();
  if (threadIdx.x < LPR) {
    float4 r = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int g = 0; g < G; ++g) {
      const float4 v = sh[g * LPR + threadIdx.x];
      r.x += v.x; r.y += v.y; r.z += v.z; r.w += v.w;
    }
    float* const out = a.db + 4 * threadIdx.x;   // (scalar stores: a bias gradient may sit at any 4-byte offset of a flat buffer)
    out[0] = r.x; out[1] = r.y; out[2] = r.z; out[3] = r.w;
  }
}
}  // namespace

size_t ln_bias_grad_work_floats(int64_t D) { return size_t(kLnBiasMaxBlocks) * size_t(D); }

int ln_bias_grad(const float* dy, const float* yln, const float* rstd, int64_t R, int64_t D, float* part, float* db, hipStream_t s) {
  BSMS_REQUIRE(D == 128 || D == 256, BSMS_E_UNSUPPORTED, "ln_bias_grad: D=%lld (128 / 256: the widths of the bf16 precisions)", (long long)D);
  BSMS_REQUIRE(dy && yln && rstd && part && db && R >= 0, BSMS_E_INVALID_ARG, "ln_bias_grad: null argument");
  LnBiasArgs a{};
  a.dy = dy; a.yln = yln; a.rstd = rstd; a.R = R; a.part = part; a.db = db;
  const int rows_per_wg = D == 128 ? 8 : 4;
  a.nblk = (int)std::max<int64_t>(1, std::min<int64_t>(ceil_div(R, rows_per_wg), kLnBiasMaxBlocks));
  if (D == 128) hipLaunchKernelGGL((k_ln_bias_part<32>), dim3(a.nblk), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((k_ln_bias_part<64>), dim3(a.nblk), dim3(256), 0, s, a);
  BSMS_LAUNCH_CHECK();
  if (D == 128) hipLaunchKernelGGL((k_ln_bias_sum<32>), dim3(1), dim3(256), 0, s, a);
  else hipLaunchKernelGGL((k_ln_bias_sum<64>), dim3(1), dim3(256), 0, s, a);
  BSMS_LAUNCH_CHECK();
  return BSMS_OK;
}

}  // namespace bsms
