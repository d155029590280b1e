// Fused optimizer step on the flat parameter / gradient buffers: global-norm gradient clipping + AdamW.
// Replaces, for one training step, torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW.step over ~180 parameter
// tensors (trainer/trainer.py:150-152) by two launches over one contiguous 1.9 M-element array.  HBM bound:
// 4 streams read + 3 written per element.  The update follows torch.optim.AdamW (decoupled weight decay,
// bias-corrected moments) operation for operation.
#include <algorithm>
#include <cmath>

#include "common.h"

using namespace bsms;

namespace {
constexpr int NPART = 256;

__global__ __launch_bounds__(256) void k_sumsq_partials(const float* g, int64_t n, float* part) {
  __shared__ float red[256];
  float s = 0.f;
  for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < n; i += int64_t(NPART) * 256) s = fmaf(g[i], g[i], s);
  red[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}

struct AdamArgs {
  float* p; const float* g; float* m; float* v;
  int64_t n;
  float lr, beta1, beta2, eps, wd, bc1, sqrt_bc2, max_norm;
  const float* part;   // NPART partial sums of g^2 (null: no clipping)
  float* norm_out;     // optional device scalar: total gradient norm before clipping
};

__global__ __launch_bounds__(256) void k_adamw(AdamArgs a) {
  __shared__ float red[256];
  float clip = 1.f;
  if (a.part) {  // every block re-reduces the 256 partials in the same fixed order: identical value everywhere
    red[threadIdx.x] = a.part[threadIdx.x];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
      __syncthreads();
    }
    const float total = sqrtf(red[0]);
    if (a.norm_out && blockIdx.x == 0 && threadIdx.x == 0) *a.norm_out = total;
    if (a.max_norm > 0.f) clip = fminf(a.max_norm / (total + 1e-6f), 1.f);   // clip_grad_norm_ semantics
  }
  for (int64_t i = int64_t(blockIdx.x) * 256 + threadIdx.x; i < a.n; i += int64_t(gridDim.x) * 256) {
    const float g = a.g[i] * clip;
    float p = a.p[i] * (1.f - a.lr * a.wd);                   // p.mul_(1 - lr * weight_decay)
    const float m = a.m[i] + (g - a.m[i]) * (1.f - a.beta1);  // exp_avg.lerp_(grad, 1 - beta1)
    const float v = a.v[i] * a.beta2 + (1.f - a.beta2) * g * g;
    const float denom = sqrtf(v) / a.sqrt_bc2 + a.eps;
    p -= (a.lr / a.bc1) * (m / denom);                        // p.addcdiv_(exp_avg, denom, value=-lr/bc1)
    a.p[i] = p; a.m[i] = m; a.v[i] = v;
  }
}
}  // namespace

extern "C" size_t bsms_adamw_work_bytes(void) { return NPART * sizeof(float); }

extern "C" int bsms_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n, float lr,
                               float beta1, float beta2, float eps, float weight_decay, int64_t step,
                               float max_grad_norm, float* grad_norm_out, void* work, bsms_stream_t stream) {
  BSMS_REQUIRE((params && grads && exp_avg && exp_avg_sq) || n == 0, BSMS_E_INVALID_ARG, "adamw_step: null argument");
  BSMS_REQUIRE(n >= 0 && step >= 1, BSMS_E_SHAPE, "adamw_step: n=%lld step=%lld (step counts from 1)", (long long)n, (long long)step);
  const bool need_norm = max_grad_norm > 0.f || grad_norm_out != nullptr;
  BSMS_REQUIRE(!need_norm || work, BSMS_E_INVALID_ARG, "adamw_step: work buffer needed for the gradient norm");
  if (n == 0) return BSMS_OK;
  hipStream_t s = as_stream(stream);
  AdamArgs a{};
  a.p = params; a.g = grads; a.m = exp_avg; a.v = exp_avg_sq; a.n = n;
  a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.wd = weight_decay;
  a.bc1 = 1.f - (float)std::pow((double)beta1, (double)step);
  a.sqrt_bc2 = (float)std::sqrt(1.0 - std::pow((double)beta2, (double)step));
  a.max_norm = max_grad_norm; a.norm_out = grad_norm_out;
  if (need_norm) {
    a.part = reinterpret_cast<float*>(work);
    hipLaunchKernelGGL(k_sumsq_partials, dim3(NPART), dim3(256), 0, s, grads, n, reinterpret_cast<float*>(work));
    BSMS_LAUNCH_CHECK();
  }
  const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(n, 256), 2048);
  hipLaunchKernelGGL(k_adamw, dim3(grid), dim3(256), 0, s, a);
  BSMS_LAUNCH_CHECK();
  return BSMS_OK;
}

// ---- gradient accumulation over the steps of an unrolled loss (step.py).  The weight-gradient kernels OVERWRITE their slots, so
// step k's backward writes a scratch flat buffer with the GradBuckets layout and this folds it into the real one:
// acc[i] = first ? g[i] : acc[i] + g[i].  One read-modify-write stream over the flat buffer (7.7 MB at airfoil size), 16-byte
// accesses; every element is touched by exactly one thread, so the sum is deterministic.
namespace {
__global__ __launch_bounds__(256) void k_grad_accumulate(float* __restrict__ acc, const float* __restrict__ g, int64_t n4,
                                                         int64_t n, int first) {
  const int64_t stride = int64_t(gridDim.x) * 256;
  const int64_t t = int64_t(blockIdx.x) * 256 + threadIdx.x;
  float4* a4 = reinterpret_cast<float4*>(acc);
  const float4* g4 = reinterpret_cast<const float4*>(g);
  for (int64_t i = t; i < n4; i += stride) {
    float4 v = g4[i];
    if (!first) {
      const float4 o = a4[i];
      v.x = o.x + v.x; v.y = o.y + v.y; v.z = o.z + v.z; v.w = o.w + v.w;
    }
    a4[i] = v;
  }
  for (int64_t i = 4 * n4 + t; i < n; i += stride) acc[i] = first ? g[i] : acc[i] + g[i];   // tail (and unaligned buffers: n4 = 0)
}
}  // namespace

extern "C" int bsms_grad_accumulate(float* acc, const float* g, int64_t n, int first, bsms_stream_t stream) {
  BSMS_REQUIRE(n >= 0, BSMS_E_SHAPE, "grad_accumulate: n=%lld", (long long)n);
  if (n == 0) return BSMS_OK;
  BSMS_REQUIRE(acc && g, BSMS_E_INVALID_ARG, "grad_accumulate: null argument");
  BSMS_REQUIRE(acc != g, BSMS_E_INVALID_ARG, "grad_accumulate: acc and g are the same buffer");
  const bool aligned = ((reinterpret_cast<uintptr_t>(acc) | reinterpret_cast<uintptr_t>(g)) & 15) == 0;
  const int64_t n4 = aligned ? n / 4 : 0;
  const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(std::max<int64_t>(n4, n - 4 * n4), 256), 2048);
  hipLaunchKernelGGL(k_grad_accumulate, dim3(grid), dim3(256), 0, as_stream(stream), acc, g, n4, n, first ? 1 : 0);
  BSMS_LAUNCH_CHECK();
  return BSMS_OK;
}

// ---- gradient accumulation over micro-batches (step.py): acc = a * acc + b * g with (a, b) read from the device
// (bsms_accum_coef wrote them on the same stream; the host never sees them).  k_grad_accumulate's grid, 16-byte path and tail; every
// element goes through the same three separately rounded fp32 operations on either path, so the result does not depend on it.
namespace {
// (HIP's __fmul_rn / __fadd_rn are plain * and +, which the default contraction fuses once they are inlined: the pragma, as in
// optim_element, is what keeps the three roundings.)
__device__ __forceinline__ float fold_element(float a, float b, float acc, float g) {
#pragma clang fp contract(off)
  const float x = a * acc;
  const float y = b * g;
  return x + y;
}

__global__ __launch_bounds__(256) void k_grad_fold(float* __restrict__ acc, const float* __restrict__ g, int64_t n4, int64_t n,
                                                   const float* __restrict__ coef) {
  const float a = coef[0], b = coef[1];
  const int64_t stride = int64_t(gridDim.x) * 256;
  const int64_t t = int64_t(blockIdx.x) * 256 + threadIdx.x;
  float4* a4 = reinterpret_cast<float4*>(acc);
  const float4* g4 = reinterpret_cast<const float4*>(g);
  for (int64_t i = t; i < n4; i += stride) {
    const float4 v = g4[i];
    float4 o = a4[i];
    o.x = fold_element(a, b, o.x, v.x); o.y = fold_element(a, b, o.y, v.y);
    o.z = fold_element(a, b, o.z, v.z); o.w = fold_element(a, b, o.w, v.w);
    a4[i] = o;
  }
  for (int64_t i = 4 * n4 + t; i < n; i += stride) acc[i] = fold_element(a, b, acc[i], g[i]);   // tail (and unaligned buffers: n4 = 0)
}
}  // namespace

extern "C" int bsms_grad_fold(float* acc, const float* g, int64_t n, const float* coef, bsms_stream_t stream) {
  BSMS_REQUIRE(n >= 0, BSMS_E_SHAPE, "grad_fold: n=%lld", (long long)n);
  if (n == 0) return BSMS_OK;
  BSMS_REQUIRE(acc && g && coef, BSMS_E_INVALID_ARG, "grad_fold: null argument");
  BSMS_REQUIRE(acc != g, BSMS_E_INVALID_ARG, "grad_fold: acc and g are the same buffer");
  const bool aligned = ((reinterpret_cast<uintptr_t>(acc) | reinterpret_cast<uintptr_t>(g)) & 15) == 0;
  const int64_t n4 = aligned ? n / 4 : 0;
  const unsigned grid = (unsigned)std::min<int64_t>(ceil_div(std::max<int64_t>(n4, n - 4 * n4), 256), 2048);
  hipLaunchKernelGGL(k_grad_fold, dim3(grid), dim3(256), 0, as_stream(stream), acc, g, n4, n, coef);
  BSMS_LAUNCH_CHECK();
  return BSMS_OK;
}

// ---- the general step (bsms_optim_step): parameter groups, an exponential moving average of the weights and a
// non-finite guard in the one pass over params / grads / exp_avg / exp_avg_sq.  k_adamw above stays the degenerate case's yardstick:
// for lr_scale = 1 (or lr pre-multiplied) this kernel reproduces its bits, and the tests hold it to that.
//
// Work is cut into CHUNKS of at most kOptChunk elements that never straddle a group: with a group table the chunks are listed in a
// device table (first, count, group) built once by bsms_optim_groups_create -- boundaries at the group boundaries and at the absolute
// multiples of kOptChunk, so a full chunk starts on a multiple of kOptChunk; without one chunk c is [c * kOptChunk, ...).  A block
// takes chunks blockIdx.x, + gridDim.x, ...: the hyper-parameters are uniform per chunk, no thread searches.  A full chunk is read
// and written with 16-byte accesses when every array is 16-byte aligned (one float4 per thread), any other chunk -- the ragged ends
// of a group, a 3-element bias -- element by element; either way an element is handled by exactly one thread with the same
// arithmetic, so the result does not depend on the path.
namespace {
constexpr int kOptChunk = 1024;
constexpr int kOptMaxGrid = 2048;
constexpr int kOptTotalSlot = NPART;   // work[NPART]: the gradient norm of this call, for the commit launch

struct OptimChunk { int64_t first; int32_t count; int32_t group; };   // 16 bytes, one scalar load
struct OptimHyper { float lr_scale, wd; };

struct OptimArgs {
  float* p; const float* g; float* m; float* v;
  float* ema;                    // nullable
  int64_t n, nchunks;
  const OptimChunk* chunks;      // null: implicit chunks, one group (lr_scale 1, `wd`)
  const OptimHyper* hyper;
  float lr, beta1, beta2, eps, wd, bc1, sqrt_bc2, max_norm, ema_decay;
  const float* part;             // NPART partial sums of g^2 (null: no norm)
  float* norm_out;               // nullable
  float* total_slot;             // with counters: where block 0 leaves the norm for k_optim_commit
  const int64_t* counters;       // nullable: {applied, skipped}; read only here
  int vec;                       // every array is 16-byte aligned
};

struct OptimStep { float clip, decay, step_size, omb1, omb2, beta2, sqrt_bc2, eps, ema_coeff; bool ema_from_old; };

// One element.  The operation sequence is k_adamw's AS COMPILED (hipcc's default contraction fuses only two places there, the decay
// factor 1 - lr * wd and g * clip - m; the second moment, the moment update and the final subtraction stay separate multiplies and
// adds), written out with contraction off so that it cannot drift: the (clipped) gradient rounded once for the second moment,
// unrounded inside the first moment's difference.
__device__ __forceinline__ void optim_element(const OptimStep& s, float graw, float& p, float& m, float& v) {
#pragma clang fp contract(off)
  const float g = graw * s.clip;
  const float d = __builtin_fmaf(s.clip, graw, -m);
  const float t = s.omb1 * d;
  m = m + t;
  const float a = s.beta2 * v;
  const float b = (s.omb2 * g) * g;
  v = a + b;
  const float denom = sqrtf(v) / s.sqrt_bc2 + s.eps;
  const float q = m / denom;
  const float u = s.step_size * q;
  const float w = s.decay * p;
  p = w - u;
}

// torch.lerp(ema, p, 1 - decay): ema + (p - ema) * (1 - decay) for 1 - decay < 0.5 and p - (p - ema) * decay otherwise -- the same
// value, formed from the nearer end, one fused multiply-add.  decay = 0 gives p and decay = 1 gives ema, bit for bit.
__device__ __forceinline__ float optim_ema(const OptimStep& s, float e, float p) {
#pragma clang fp contract(off)
  return __builtin_fmaf(s.ema_coeff, p - e, s.ema_from_old ? e : p);
}

// beta^t in fp64 by repeated squaring: at most 63 + 63 multiplies, each within half an ulp -- far below the one rounding to fp32
// that follows (1 - beta^t cancels at most log2(1 / (1 - beta)) bits: 10 for beta2 = 0.999).
__device__ inline double optim_powi(double b, int64_t t) {
  double r = 1.0;
  while (t > 0) {
    if (t & 1) r *= b;
    b *= b;
    t >>= 1;
  }
  return r;
}

__global__ __launch_bounds__(256) void k_optim(OptimArgs a) {
  __shared__ float red[256];
  __shared__ float bc[2];
  OptimStep s;
  s.clip = 1.f;
  if (a.part) {  // as k_adamw: every block re-reduces the partials in the same fixed order
    red[threadIdx.x] = a.part[threadIdx.x];
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
      if (threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
      __syncthreads();
    }
    const float total = sqrtf(red[0]);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      if (a.norm_out) *a.norm_out = total;
      if (a.total_slot) *a.total_slot = total;
    }
    if (a.counters && !(fabsf(total) <= 3.402823466e38f)) return;   // the guard: inf or NaN, the same value in every block -- nothing is written
    if (a.max_norm > 0.f) s.clip = fminf(a.max_norm / (total + 1e-6f), 1.f);
  }
  float bc1 = a.bc1;
  s.sqrt_bc2 = a.sqrt_bc2;
  if (a.counters) {   // the step number is the device's: applied steps so far + 1
    if (threadIdx.x == 0) {
      const int64_t t = a.counters[0] + 1;
      bc[0] = (float)(1.0 - optim_powi((double)a.beta1, t));
      bc[1] = (float)sqrt(1.0 - optim_powi((double)a.beta2, t));
    }
    __syncthreads();
    bc1 = bc[0];
    s.sqrt_bc2 = bc[1];
  }
  s.omb1 = 1.f - a.beta1;
  s.omb2 = 1.f - a.beta2;
  s.beta2 = a.beta2;
  s.eps = a.eps;
  const float ema_w = 1.f - a.ema_decay;
  s.ema_from_old = ema_w < 0.5f;
  s.ema_coeff = s.ema_from_old ? ema_w : -a.ema_decay;   // p - (p - e) * decay
  const int tid = threadIdx.x;
  for (int64_t c = blockIdx.x; c < a.nchunks; c += gridDim.x) {
    int64_t first;
    int count;
    float lr_scale = 1.f, wd = a.wd;
    if (a.chunks) {
      const OptimChunk ch = a.chunks[c];
      const OptimHyper h = a.hyper[ch.group];
      first = ch.first; count = ch.count; lr_scale = h.lr_scale; wd = h.wd;
    } else {
      first = c * kOptChunk;
      count = (int)(a.n - first < kOptChunk ? a.n - first : kOptChunk);
    }
    {
#pragma clang fp contract(off)
      const float lr_k = a.lr * lr_scale;
      s.decay = __builtin_fmaf(-lr_k, wd, 1.f);
      s.step_size = lr_k / bc1;
    }
    if (a.vec && count == kOptChunk && (first & 3) == 0) {
      const int64_t i = first + 4 * tid;
      const float4 g4 = *reinterpret_cast<const float4*>(a.g + i);
      float4 p4 = *reinterpret_cast<const float4*>(a.p + i);
      float4 m4 = *reinterpret_cast<const float4*>(a.m + i);
      float4 v4 = *reinterpret_cast<const float4*>(a.v + i);
      optim_element(s, g4.x, p4.x, m4.x, v4.x);
      optim_element(s, g4.y, p4.y, m4.y, v4.y);
      optim_element(s, g4.z, p4.z, m4.z, v4.z);
      optim_element(s, g4.w, p4.w, m4.w, v4.w);
      *reinterpret_cast<float4*>(a.p + i) = p4;
      *reinterpret_cast<float4*>(a.m + i) = m4;
      *reinterpret_cast<float4*>(a.v + i) = v4;
      if (a.ema) {
        float4 e4 = *reinterpret_cast<const float4*>(a.ema + i);
        e4.x = optim_ema(s, e4.x, p4.x); e4.y = optim_ema(s, e4.y, p4.y);
        e4.z = optim_ema(s, e4.z, p4.z); e4.w = optim_ema(s, e4.w, p4.w);
        *reinterpret_cast<float4*>(a.ema + i) = e4;
      }
    } else {
      for (int j = tid; j < count; j += 256) {
        const int64_t i = first + j;
        float p = a.p[i], m = a.m[i], v = a.v[i];
        optim_element(s, a.g[i], p, m, v);
        a.p[i] = p; a.m[i] = m; a.v[i] = v;
        if (a.ema) a.ema[i] = optim_ema(s, a.ema[i], p);
      }
    }
  }
}

// One thread, after every block of k_optim in stream order: the same float decides here as there.
__global__ void k_optim_commit(const float* total, int64_t* counters) {
  if (threadIdx.x == 0 && blockIdx.x == 0) counters[fabsf(*total) <= 3.402823466e38f ? 0 : 1] += 1;
}
}  // namespace

struct bsms_optim_groups {
  int64_t n = 0, nchunks = 0;
  int ngroups = 0;
  void* block = nullptr;   // the one device allocation: nchunks OptimChunk, then ngroups OptimHyper
};

extern "C" int bsms_optim_groups_create(const bsms_optim_group_t* host_groups, int ngroups, int64_t n, bsms_optim_groups_t** out) {
  BSMS_REQUIRE(out, BSMS_E_INVALID_ARG, "optim_groups_create: out is null");
  *out = nullptr;
  BSMS_REQUIRE(host_groups, BSMS_E_INVALID_ARG, "optim_groups_create: group table is null");
  BSMS_REQUIRE(ngroups >= 1 && ngroups <= 4096, BSMS_E_INVALID_ARG, "optim_groups_create: ngroups=%d outside 1..4096", ngroups);
  BSMS_REQUIRE(n >= 1, BSMS_E_SHAPE, "optim_groups_create: n=%lld", (long long)n);
  int64_t expect = 0, nchunks = 0;
  for (int k = 0; k < ngroups; ++k) {
    const bsms_optim_group_t& g = host_groups[k];
    BSMS_REQUIRE(std::isfinite(g.lr_scale) && g.lr_scale >= 0.f, BSMS_E_INVALID_ARG,
                 "optim_groups_create: group %d: lr_scale=%g is not a finite non-negative number", k, (double)g.lr_scale);
    BSMS_REQUIRE(std::isfinite(g.weight_decay) && g.weight_decay >= 0.f, BSMS_E_INVALID_ARG,
                 "optim_groups_create: group %d: weight_decay=%g is not a finite non-negative number", k, (double)g.weight_decay);
    BSMS_REQUIRE(g.count >= 1, BSMS_E_SHAPE, "optim_groups_create: group %d: count=%lld (an empty group)", k, (long long)g.count);
    BSMS_REQUIRE(k == 0 || g.offset >= host_groups[k - 1].offset, BSMS_E_SHAPE,
                 "optim_groups_create: group %d: groups are not sorted by offset (%lld after %lld)", k, (long long)g.offset,
                 (long long)host_groups[k - 1].offset);
  }
  for (int k = 0; k < ngroups; ++k) {   // sorted: what is left is how the groups tile [0, n)
    const bsms_optim_group_t& g = host_groups[k];
    BSMS_REQUIRE(g.offset >= expect, BSMS_E_SHAPE, "optim_groups_create: group %d: overlap (offset %lld, the group before ends at %lld)", k,
                 (long long)g.offset, (long long)expect);
    BSMS_REQUIRE(g.offset == expect, BSMS_E_SHAPE, "optim_groups_create: group %d: gap (offset %lld, the group before ends at %lld)", k,
                 (long long)g.offset, (long long)expect);
    BSMS_REQUIRE(g.count <= n - g.offset, BSMS_E_SHAPE, "optim_groups_create: group %d: runs past n (offset %lld + count %lld > %lld)", k,
                 (long long)g.offset, (long long)g.count, (long long)n);
    expect = g.offset + g.count;
    nchunks += (expect - 1) / kOptChunk - g.offset / kOptChunk + 1;
  }
  BSMS_REQUIRE(expect == n, BSMS_E_SHAPE, "optim_groups_create: the groups stop short of n (%lld of %lld elements)", (long long)expect, (long long)n);
  std::vector<OptimChunk> chunks;
  chunks.reserve((size_t)nchunks);
  for (int k = 0; k < ngroups; ++k) {
    const int64_t end = host_groups[k].offset + host_groups[k].count;
    for (int64_t first = host_groups[k].offset; first < end;) {
      const int64_t stop = std::min(end, (first / kOptChunk + 1) * kOptChunk);
      chunks.push_back(OptimChunk{first, (int32_t)(stop - first), k});
      first = stop;
    }
  }
  std::vector<OptimHyper> hyper((size_t)ngroups);
  for (int k = 0; k < ngroups; ++k) hyper[(size_t)k] = OptimHyper{host_groups[k].lr_scale, host_groups[k].weight_decay};
  const size_t chunk_bytes = chunks.size() * sizeof(OptimChunk), hyper_bytes = hyper.size() * sizeof(OptimHyper);
  std::vector<char> host(chunk_bytes + hyper_bytes);
  std::copy_n(reinterpret_cast<const char*>(chunks.data()), chunk_bytes, host.data());
  std::copy_n(reinterpret_cast<const char*>(hyper.data()), hyper_bytes, host.data() + chunk_bytes);
  void* block = nullptr;
  BSMS_HIP_CHECK(hipMalloc(&block, host.size()));
  const hipError_t e = hipMemcpy(block, host.data(), host.size(), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    (void)hipFree(block);
    BSMS_FAIL(BSMS_E_HIP, "optim_groups_create: upload: %s", hipGetErrorString(e));
  }
  bsms_optim_groups* h = new bsms_optim_groups;
  h->n = n; h->nchunks = (int64_t)chunks.size(); h->ngroups = ngroups; h->block = block;
  *out = h;
  return BSMS_OK;
}

extern "C" int bsms_optim_groups_destroy(bsms_optim_groups_t* groups) {
  if (!groups) return BSMS_OK;
  const hipError_t e = hipFree(groups->block);
  delete groups;
  BSMS_REQUIRE(e == hipSuccess, BSMS_E_HIP, "optim_groups_destroy: %s", hipGetErrorString(e));
  return BSMS_OK;
}

extern "C" size_t bsms_optim_work_bytes(void) { return (NPART + 4) * sizeof(float); }

extern "C" int bsms_optim_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, int64_t n,
                               const bsms_optim_groups_t* groups, float lr, float beta1, float beta2, float eps, float weight_decay,
                               int64_t step, float max_grad_norm, float* ema, float ema_decay, int64_t* counters,
                               float* grad_norm_out, void* work, bsms_stream_t stream) {
  BSMS_REQUIRE((params && grads && exp_avg && exp_avg_sq) || n == 0, BSMS_E_INVALID_ARG, "optim_step: null argument");
  BSMS_REQUIRE(n >= 0, BSMS_E_SHAPE, "optim_step: n=%lld", (long long)n);
  BSMS_REQUIRE(ema_decay >= 0.f && ema_decay <= 1.f, BSMS_E_INVALID_ARG, "optim_step: ema_decay=%g outside [0, 1]", (double)ema_decay);
  if (counters) {
    BSMS_REQUIRE(work, BSMS_E_INVALID_ARG, "optim_step: the guard (counters) needs the work buffer: the norm is always formed");
    BSMS_REQUIRE(step == 0, BSMS_E_INVALID_ARG, "optim_step: step=%lld with counters (the device counts: pass 0)", (long long)step);
  } else {
    BSMS_REQUIRE(step >= 1, BSMS_E_SHAPE, "optim_step: step=%lld (step counts from 1)", (long long)step);
  }
  BSMS_REQUIRE(!groups || groups->n == n, BSMS_E_SHAPE, "optim_step: the group table covers %lld elements, the call %lld",
               (long long)(groups ? groups->n : 0), (long long)n);
  const bool need_norm = counters || max_grad_norm > 0.f || grad_norm_out != nullptr;
  BSMS_REQUIRE(!need_norm || work, BSMS_E_INVALID_ARG, "optim_step: work buffer needed for the gradient norm");
  if (n == 0) return BSMS_OK;
  hipStream_t s = as_stream(stream);
  OptimArgs a{};
  a.p = params; a.g = grads; a.m = exp_avg; a.v = exp_avg_sq; a.ema = ema; a.n = n;
  a.lr = lr; a.beta1 = beta1; a.beta2 = beta2; a.eps = eps; a.wd = weight_decay;
  a.max_norm = max_grad_norm; a.ema_decay = ema_decay; a.norm_out = grad_norm_out; a.counters = counters;
  if (!counters) {
    a.bc1 = 1.f - (float)std::pow((double)beta1, (double)step);
    a.sqrt_bc2 = (float)std::sqrt(1.0 - std::pow((double)beta2, (double)step));
  }
  if (groups) {
    a.chunks = reinterpret_cast<const OptimChunk*>(groups->block);
    a.hyper = reinterpret_cast<const OptimHyper*>(a.chunks + groups->nchunks);
    a.nchunks = groups->nchunks;
  } else {
    a.nchunks = ceil_div(n, kOptChunk);
  }
  const uintptr_t bits = reinterpret_cast<uintptr_t>(params) | reinterpret_cast<uintptr_t>(grads) | reinterpret_cast<uintptr_t>(exp_avg) |
                         reinterpret_cast<uintptr_t>(exp_avg_sq) | reinterpret_cast<uintptr_t>(ema);
  a.vec = (bits & 15) == 0;
  if (need_norm) {
    a.part = reinterpret_cast<float*>(work);
    if (counters) a.total_slot = reinterpret_cast<float*>(work) + kOptTotalSlot;
    hipLaunchKernelGGL(k_sumsq_partials, dim3(NPART), dim3(256), 0, s, grads, n, reinterpret_cast<float*>(work));
    BSMS_LAUNCH_CHECK();
  }
  const unsigned grid = (unsigned)std::min<int64_t>(a.nchunks, kOptMaxGrid);
  hipLaunchKernelGGL(k_optim, dim3(grid), dim3(256), 0, s, a);
  BSMS_LAUNCH_CHECK();
  if (counters) {
    hipLaunchKernelGGL(k_optim_commit, dim3(1), dim3(64), 0, s, a.total_slot, counters);
    BSMS_LAUNCH_CHECK();
  }
  return BSMS_OK;
}
