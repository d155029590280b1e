// Batch assembly from device-resident trajectories (include/bsms_hip.h: bsms_batch_assemble): the level-0 node tensors of a
// training batch -- what datasets/base.py:238-289 (`proc_data`) plus the collate build on the host per step -- written by ONE
// launch from fields that already live in HBM:
//   node_in  [R, C+p+1] = [state_t + noise | mesh_pos | node_type]
//   node_tar [R, C]     = state_{t+1} + g * noise                    g = fl32(1 - noise_gamma)
//   node_mask[R]        = node_type is one of the valid codes
//   noise               = fl32(std_c) * z, 0 where the mask is 0;  z from Philox4x32-10 + Box-Muller (contract in the header)
// The per-sample pointers travel as a kernel argument (kBatchSamples per launch): no upload, no synchronisation.
// Compiled with -ffp-contract=off (build.py): `state + noise` and `tar + g * noise` round like the host's separate torch ops.
#include "common.h"

#pragma clang fp contract(off)

using namespace bsms;

namespace {

constexpr int kMaxValid = 4;         // node-type codes that count for the loss
constexpr int kBatchSamples = 64;    // samples per launch: the table is a kernel argument (64 * 48 B + header < 4 KB)
constexpr int kRowsPerBlock = 256;

struct BatchSample {
  const float *state_in, *state_tar, *pos, *type;
  int64_t row0;       // batch-global row of the sample's first node
  int32_t blk0;       // first block of the sample in this launch (a block never straddles two samples)
  int32_t n;          // rows of the sample
};
struct BatchArgs {
  BatchSample s[kBatchSamples];
  int32_t n_samples, C, p, n_valid;
  float std[kMaxC];
  float valid[kMaxValid];
  float g;
  int32_t noisy;
  uint32_t seed_lo, seed_hi, draw_lo, draw_hi;
};

struct Philox4 { uint32_t x[4]; };

// Philox4x32-10 (Salmon et al., SC'11), counter c[0..3], key k[0..1]
__host__ __device__ inline Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
  for (int round = 0; round < 10; ++round) {
    const uint64_t m0 = uint64_t(0xD2511F53u) * c0, m1 = uint64_t(0xCD9E8D57u) * c2;
    const uint32_t n0 = uint32_t(m1 >> 32) ^ c1 ^ k0, n1 = uint32_t(m1), n2 = uint32_t(m0 >> 32) ^ c3 ^ k1, n3 = uint32_t(m0);
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}

// Box-Muller pair from two 32-bit words.  u = (k + 0.5) * 2^-24 with k = x >> 8 needs 25 bits when k >= 2^23, so u itself is
// never formed: w = min(u, 1 - u) = (j + 0.5) * 2^-24 with j < 2^23 IS exact in fp32, and
//   ln u = logf(w) (lower half) or log1pf(-w) (upper half);  cos 2 pi u = cos 2 pi w;  sin 2 pi u = +/- sin 2 pi w
// -- the only roundings are those of logf / log1pf / sqrtf / sincosf and of the angle fl32(fl32(2 pi) * w).
__device__ __forceinline__ void box_muller(uint32_t xa, uint32_t xb, float& z_cos, float& z_sin) {
  const uint32_t ka = xa >> 8, kb = xb >> 8;
  const bool up_a = ka >= (1u << 23), up_b = kb >= (1u << 23);
  const float wa = (float(up_a ? (1u << 24) - 1u - ka : ka) + 0.5f) * 5.9604644775390625e-8f;   // 2^-24
  const float wb = (float(up_b ? (1u << 24) - 1u - kb : kb) + 0.5f) * 5.9604644775390625e-8f;
  const float ln_u = up_a ? log1pf(-wa) : logf(wa);
  const float r = sqrtf(-2.0f * ln_u);
  float sn, cs;
  sincosf(6.28318530717958647692f * wb, &sn, &cs);
  z_cos = r * cs;
  z_sin = r * (up_b ? -sn : sn);
}

__global__ __launch_bounds__(kRowsPerBlock) void k_batch_assemble(const BatchArgs a, float* __restrict__ node_in,
                                                                  float* __restrict__ node_tar, float* __restrict__ node_mask,
                                                                  float* __restrict__ noise_out) {
  // which sample does this block belong to: block-uniform search over at most 64 entries of the argument table
  int lo = 0, hi = a.n_samples - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (a.s[mid].blk0 <= int(blockIdx.x)) lo = mid; else hi = mid - 1;
  }
  const BatchSample& sm = a.s[lo];
  const int i = (int(blockIdx.x) - sm.blk0) * kRowsPerBlock + int(threadIdx.x);   // row inside the sample
  if (i >= sm.n) return;
  const int C = a.C, p = a.p, W = C + p + 1;
  const int64_t r = sm.row0 + i;                                                   // batch-global row

  const float type = sm.type[i];
  bool valid = false;
  for (int k = 0; k < a.n_valid; ++k) valid |= (type == a.valid[k]);

  float nz[kMaxC];
#pragma unroll
  for (int c = 0; c < kMaxC; ++c) nz[c] = 0.f;
  if (a.noisy && valid) {
#pragma unroll
    for (int q = 0; q < kMaxC / 4; ++q) {
      if (4 * q < C) {
        const Philox4 x = philox4x32_10(uint32_t(uint64_t(r)), uint32_t(q), a.draw_lo, a.draw_hi, a.seed_lo, a.seed_hi);
        float z[4];
        box_muller(x.x[0], x.x[1], z[0], z[1]);
        box_muller(x.x[2], x.x[3], z[2], z[3]);
#pragma unroll
        for (int j = 0; j < 4; ++j) nz[4 * q + j] = a.std[4 * q + j] * z[j];
      }
    }
  }

  float* in_row = node_in + r * W;
#pragma unroll
  for (int c = 0; c < kMaxC; ++c) {
    if (c < C) {
      const float s = sm.state_in[int64_t(i) * C + c], t = sm.state_tar[int64_t(i) * C + c];
      if (a.noisy) {
        const float gn = a.g * nz[c];
        in_row[c] = s + nz[c];
        node_tar[r * C + c] = t + gn;
      } else {
        in_row[c] = s;
        node_tar[r * C + c] = t;
      }
      if (noise_out) noise_out[r * C + c] = nz[c];
    }
  }
  for (int c = 0; c < p; ++c) in_row[C + c] = sm.pos[int64_t(i) * p + c];
  in_row[W - 1] = type;
  node_mask[r] = valid ? 1.f : 0.f;
}

}  // namespace

extern "C" int bsms_batch_assemble(const bsms_batch_sample* samples, int64_t n_samples, int64_t C, int64_t p,
                                   const float* noise_std, double noise_gamma, const float* valid_types, int64_t n_valid,
                                   uint64_t seed, uint64_t draw, float* node_in, float* node_tar, float* node_mask,
                                   float* noise_out, bsms_stream_t stream) {
  BSMS_REQUIRE(C >= 1 && C <= kMaxC && p >= 1 && p <= 7 && n_valid >= 1 && n_valid <= kMaxValid, BSMS_E_UNSUPPORTED,
               "batch_assemble: C=%lld p=%lld n_valid=%lld (C in 1..8, p in 1..7, n_valid in 1..4)", (long long)C, (long long)p,
               (long long)n_valid);
  BSMS_REQUIRE(n_samples >= 0, BSMS_E_INVALID_ARG, "batch_assemble: n_samples=%lld", (long long)n_samples);
  if (n_samples == 0) return BSMS_OK;
  BSMS_REQUIRE(samples && valid_types && node_in && node_tar && node_mask, BSMS_E_INVALID_ARG, "batch_assemble: null argument");
  // the block index and the row inside a sample are 32-bit in the kernel: the largest launch (64 samples) must keep both there
  constexpr int64_t kMaxRows = (int64_t(1) << 31) / kBatchSamples - kRowsPerBlock;
  for (int64_t i = 0; i < n_samples; ++i) {
    BSMS_REQUIRE(samples[i].n >= 0 && samples[i].n <= kMaxRows, BSMS_E_UNSUPPORTED, "batch_assemble: sample %lld has %lld rows (at most %lld)",
                 (long long)i, (long long)samples[i].n, (long long)kMaxRows);
    BSMS_REQUIRE(samples[i].n == 0 || (samples[i].state_in && samples[i].state_tar && samples[i].pos && samples[i].type), BSMS_E_INVALID_ARG,
                 "batch_assemble: sample %lld has a null field", (long long)i);
  }
  BatchArgs a;
  a.C = int32_t(C);
  a.p = int32_t(p);
  a.n_valid = int32_t(n_valid);
  for (int c = 0; c < kMaxC; ++c) a.std[c] = (noise_std && c < C) ? noise_std[c] : 0.f;
  for (int k = 0; k < kMaxValid; ++k) a.valid[k] = k < n_valid ? valid_types[k] : valid_types[0];
  a.g = float(1.0 - noise_gamma);
  a.noisy = noise_std ? 1 : 0;
  a.seed_lo = uint32_t(seed);
  a.seed_hi = uint32_t(seed >> 32);
  a.draw_lo = uint32_t(draw);
  a.draw_hi = uint32_t(draw >> 32);
  hipStream_t s = as_stream(stream);
  int64_t row0 = 0;
  for (int64_t first = 0; first < n_samples; first += kBatchSamples) {   // the row offset carries across launches
    const int cnt = int(std::min<int64_t>(kBatchSamples, n_samples - first));
    int64_t blocks = 0;
    for (int k = 0; k < kBatchSamples; ++k) {
      const bsms_batch_sample& src = samples[first + std::min(k, cnt - 1)];
      BatchSample& d = a.s[k];
      d.state_in = src.state_in; d.state_tar = src.state_tar; d.pos = src.pos; d.type = src.type;
      d.row0 = row0;
      d.blk0 = int32_t(blocks);
      d.n = k < cnt ? int32_t(src.n) : 0;
      if (k < cnt) {
        row0 += src.n;
        blocks += ceil_div(src.n, kRowsPerBlock);
      }
    }
    a.n_samples = cnt;
    if (blocks == 0) continue;
    hipLaunchKernelGGL(k_batch_assemble, dim3((unsigned)blocks), dim3(kRowsPerBlock), 0, s, a, node_in, node_tar, node_mask, noise_out);
    BSMS_LAUNCH_CHECK();
  }
  return BSMS_OK;
}

// ---- later targets of an unrolled (K-step) loss: frames t+2 .. t+K of every pick.  The resident state is [T, N, C], so frame
// t+1+(j+1) lies (j+1) * n * C floats behind `state_tar`.  A sample is copied as a flat run of n * C floats (coalesced on both
// sides); blockIdx.y is the later frame j.  No noise: only node_in / node_tar carry it.
namespace {

struct TargetsArgs {
  const float* tar[kBatchSamples];
  int64_t elem0[kBatchSamples];   // batch-global first element (row0 * C) of the sample
  int64_t elems[kBatchSamples];   // n * C
  int32_t blk0[kBatchSamples];    // first block of the sample in this launch (a block never straddles two samples)
  int32_t n_samples;
  int64_t frame;                  // elements of one later frame of the batch: R * C
};

__global__ __launch_bounds__(kRowsPerBlock) void k_batch_targets(const TargetsArgs a, float* __restrict__ later) {
  int lo = 0, hi = a.n_samples - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (a.blk0[mid] <= int(blockIdx.x)) lo = mid; else hi = mid - 1;
  }
  const int64_t i = int64_t(int(blockIdx.x) - a.blk0[lo]) * kRowsPerBlock + int(threadIdx.x);   // element inside the sample
  if (i >= a.elems[lo]) return;
  const int64_t j = blockIdx.y;
  later[j * a.frame + a.elem0[lo] + i] = a.tar[lo][(j + 1) * a.elems[lo] + i];
}

}  // namespace

extern "C" int bsms_batch_targets(const bsms_batch_sample* samples, int64_t n_samples, int64_t C, int64_t n_later, float* later,
                                  bsms_stream_t stream) {
  BSMS_REQUIRE(C >= 1 && C <= kMaxC, BSMS_E_UNSUPPORTED, "batch_targets: C=%lld (C in 1..8)", (long long)C);
  BSMS_REQUIRE(n_samples >= 0 && n_later >= 0, BSMS_E_INVALID_ARG, "batch_targets: n_samples=%lld n_later=%lld", (long long)n_samples,
               (long long)n_later);
  BSMS_REQUIRE(n_later <= 65535, BSMS_E_UNSUPPORTED, "batch_targets: n_later=%lld (at most 65535 later frames)", (long long)n_later);
  if (n_samples == 0 || n_later == 0) return BSMS_OK;
  BSMS_REQUIRE(samples && later, BSMS_E_INVALID_ARG, "batch_targets: null argument");
  constexpr int64_t kMaxRows = (int64_t(1) << 31) / kBatchSamples - kRowsPerBlock;   // as bsms_batch_assemble
  int64_t rows = 0;
  for (int64_t i = 0; i < n_samples; ++i) {
    BSMS_REQUIRE(samples[i].n >= 0 && samples[i].n <= kMaxRows, BSMS_E_UNSUPPORTED, "batch_targets: sample %lld has %lld rows (at most %lld)",
                 (long long)i, (long long)samples[i].n, (long long)kMaxRows);
    BSMS_REQUIRE(samples[i].n == 0 || samples[i].state_tar, BSMS_E_INVALID_ARG, "batch_targets: sample %lld has a null state_tar", (long long)i);
    rows += samples[i].n;
  }
  TargetsArgs a;
  a.frame = rows * C;
  hipStream_t s = as_stream(stream);
  int64_t elem0 = 0;
  for (int64_t first = 0; first < n_samples; first += kBatchSamples) {
    const int cnt = int(std::min<int64_t>(kBatchSamples, n_samples - first));
    int64_t blocks = 0;     // at most 64 * ceil(8 * kMaxRows / 256) < 2^27
    for (int k = 0; k < kBatchSamples; ++k) {
      const bsms_batch_sample& src = samples[first + std::min(k, cnt - 1)];
      a.tar[k] = src.state_tar;
      a.elem0[k] = elem0;
      a.blk0[k] = int32_t(blocks);
      a.elems[k] = k < cnt ? src.n * C : 0;
      if (k < cnt) {
        elem0 += src.n * C;
        blocks += ceil_div(src.n * C, kRowsPerBlock);
      }
    }
    a.n_samples = cnt;
    if (blocks == 0) continue;
    hipLaunchKernelGGL(k_batch_targets, dim3((unsigned)blocks, (unsigned)n_later), dim3(kRowsPerBlock), 0, s, a, later);
    BSMS_LAUNCH_CHECK();
  }
  return BSMS_OK;
}

// ---- frame augmentation: bsms_batch_assemble with one rigid transform per sample, and the same transform on the rows of any
// [F, R, C] tensor (later targets, predictions, node_in itself).  For a vector group v = (v[0] .. v[p-1]) and Q = xf[s]:
//   y[a] = fl32( .. fl32( fl32(Q[a][0] * v[0]) + fl32(Q[a][1] * v[1]) ) .. )        b ascending, every product rounded, no FMA
// The matrices ride in the kernel-argument table next to the pointers, which makes an entry 88 B: 40 samples per launch keep
// the argument block under HIP's 4 KB.  A transformed channel re-reads its group's p inputs from the row (the same cache
// line) with block-uniform offsets instead of indexing a register array with a runtime channel.
namespace {

constexpr int kMaxVec = 4;           // vector groups per row
constexpr int kXfSamples = 40;       // samples per launch of the two transform kernels
constexpr int kMaxRowW = 16;         // row width of bsms_rows_transform: node_in rows are C + p + 1 <= 12 wide

struct XfSample {
  const float *state_in, *state_tar, *pos, *type;
  int64_t row0;
  int32_t blk0, n;
  float q[9];                        // row-major [p, p]
};
struct XfArgs {
  XfSample s[kXfSamples];
  int32_t n_samples, C, p, n_valid;
  float std[kMaxC];
  float valid[kMaxValid];
  float g;
  int32_t noisy;
  uint32_t seed_lo, seed_hi, draw_lo, draw_hi;
  int8_t first[kMaxC];               // first channel of the vector group that channel c belongs to, -1 for a scalar channel
};
static_assert(sizeof(XfArgs) + 4 * sizeof(void*) <= 4096, "k_batch_assemble_xf: the argument block exceeds 4 KB");

// y[a] of the group whose inputs are v[0 .. p): products and sums rounded one by one (fp contract is off in this file)
__device__ __forceinline__ float xf_row(const float* q, int p, int a, const float* v) {
  float acc = q[a * p] * v[0];
  for (int b = 1; b < p; ++b) {
    const float t = q[a * p + b] * v[b];
    acc = acc + t;
  }
  return acc;
}

__global__ __launch_bounds__(kRowsPerBlock) void k_batch_assemble_xf(const XfArgs a, float* __restrict__ node_in,
                                                                     float* __restrict__ node_tar, float* __restrict__ node_mask,
                                                                     float* __restrict__ noise_out) {
  int lo = 0, hi = a.n_samples - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (a.s[mid].blk0 <= int(blockIdx.x)) lo = mid; else hi = mid - 1;
  }
  const XfSample& sm = a.s[lo];
  const int i = (int(blockIdx.x) - sm.blk0) * kRowsPerBlock + int(threadIdx.x);   // row inside the sample
  if (i >= sm.n) return;
  const int C = a.C, p = a.p, W = C + p + 1;
  const int64_t r = sm.row0 + i;                                                   // batch-global row

  const float type = sm.type[i];
  bool valid = false;
  for (int k = 0; k < a.n_valid; ++k) valid |= (type == a.valid[k]);

  float nz[kMaxC];                   // the noise of k_batch_assemble, word for word: same counter, same key, same channels
#pragma unroll
  for (int c = 0; c < kMaxC; ++c) nz[c] = 0.f;
  if (a.noisy && valid) {
#pragma unroll
    for (int q = 0; q < kMaxC / 4; ++q) {
      if (4 * q < C) {
        const Philox4 x = philox4x32_10(uint32_t(uint64_t(r)), uint32_t(q), a.draw_lo, a.draw_hi, a.seed_lo, a.seed_hi);
        float z[4];
        box_muller(x.x[0], x.x[1], z[0], z[1]);
        box_muller(x.x[2], x.x[3], z[2], z[3]);
#pragma unroll
        for (int j = 0; j < 4; ++j) nz[4 * q + j] = a.std[4 * q + j] * z[j];
      }
    }
  }

  const float* s_row = sm.state_in + int64_t(i) * C;
  const float* t_row = sm.state_tar + int64_t(i) * C;
  float* in_row = node_in + r * W;
#pragma unroll
  for (int c = 0; c < kMaxC; ++c) {
    if (c < C) {
      const int f = a.first[c];      // block-uniform
      float s, t;
      if (f >= 0) {
        s = xf_row(sm.q, p, c - f, s_row + f);
        t = xf_row(sm.q, p, c - f, t_row + f);
      } else {
        s = s_row[c];
        t = t_row[c];
      }
      if (a.noisy) {
        const float gn = a.g * nz[c];
        in_row[c] = s + nz[c];
        node_tar[r * C + c] = t + gn;
      } else {
        in_row[c] = s;
        node_tar[r * C + c] = t;
      }
      if (noise_out) noise_out[r * C + c] = nz[c];
    }
  }
  const float* p_row = sm.pos + int64_t(i) * p;
  for (int c = 0; c < p; ++c) in_row[C + c] = xf_row(sm.q, p, c, p_row);
  in_row[W - 1] = type;
  node_mask[r] = valid ? 1.f : 0.f;
}

// the vector groups of a row of `width` channels: envelope first, then the table itself.  `first` gets, per channel, the first
// channel of its group or -1.
int xf_groups(const char* who, int64_t width, int64_t p, const int32_t* vec_first, int64_t n_vec, int8_t* first, int n_first) {
  BSMS_REQUIRE(vec_first || n_vec == 0, BSMS_E_INVALID_ARG, "%s: vec_first is null with n_vec=%lld", who, (long long)n_vec);
  for (int c = 0; c < n_first; ++c) first[c] = -1;
  for (int64_t g = 0; g < n_vec; ++g) {
    const int64_t f = vec_first[g];
    BSMS_REQUIRE(f >= 0 && f + p <= width, BSMS_E_INVALID_ARG, "%s: vector group %lld covers channels [%lld, %lld) of %lld", who,
                 (long long)g, (long long)f, (long long)(f + p), (long long)width);
    for (int64_t c = f; c < f + p; ++c) {
      BSMS_REQUIRE(first[c] < 0, BSMS_E_INVALID_ARG, "%s: vector groups %lld and an earlier one overlap at channel %lld", who,
                   (long long)g, (long long)c);
      first[c] = int8_t(f);
    }
  }
  return BSMS_OK;
}

}  // namespace

extern "C" int bsms_batch_assemble_xf(const bsms_batch_sample* samples, int64_t n_samples, int64_t C, int64_t p, const float* xf,
                                      const int32_t* vec_first, int64_t n_vec, const float* noise_std, double noise_gamma,
                                      const float* valid_types, int64_t n_valid, uint64_t seed, uint64_t draw, float* node_in,
                                      float* node_tar, float* node_mask, float* noise_out, bsms_stream_t stream) {
  BSMS_REQUIRE(C >= 1 && C <= kMaxC && (p == 2 || p == 3) && n_valid >= 1 && n_valid <= kMaxValid && n_vec >= 0 && n_vec <= kMaxVec,
               BSMS_E_UNSUPPORTED, "batch_assemble_xf: C=%lld p=%lld n_valid=%lld n_vec=%lld (C in 1..8, p in 2..3, n_valid in 1..4, n_vec in 0..4)",
               (long long)C, (long long)p, (long long)n_valid, (long long)n_vec);
  BSMS_REQUIRE(n_samples >= 0, BSMS_E_INVALID_ARG, "batch_assemble_xf: n_samples=%lld", (long long)n_samples);
  XfArgs a;
  if (const int rc = xf_groups("batch_assemble_xf", C, p, vec_first, n_vec, a.first, kMaxC)) return rc;
  if (n_samples == 0) return BSMS_OK;
  BSMS_REQUIRE(samples && xf && valid_types && node_in && node_tar && node_mask, BSMS_E_INVALID_ARG, "batch_assemble_xf: null argument");
  constexpr int64_t kMaxRows = (int64_t(1) << 31) / kBatchSamples - kRowsPerBlock;   // as bsms_batch_assemble
  for (int64_t i = 0; i < n_samples; ++i) {
    BSMS_REQUIRE(samples[i].n >= 0 && samples[i].n <= kMaxRows, BSMS_E_UNSUPPORTED, "batch_assemble_xf: sample %lld has %lld rows (at most %lld)",
                 (long long)i, (long long)samples[i].n, (long long)kMaxRows);
    BSMS_REQUIRE(samples[i].n == 0 || (samples[i].state_in && samples[i].state_tar && samples[i].pos && samples[i].type), BSMS_E_INVALID_ARG,
                 "batch_assemble_xf: sample %lld has a null field", (long long)i);
  }
  a.C = int32_t(C);
  a.p = int32_t(p);
  a.n_valid = int32_t(n_valid);
  for (int c = 0; c < kMaxC; ++c) a.std[c] = (noise_std && c < C) ? noise_std[c] : 0.f;
  for (int k = 0; k < kMaxValid; ++k) a.valid[k] = k < n_valid ? valid_types[k] : valid_types[0];
  a.g = float(1.0 - noise_gamma);
  a.noisy = noise_std ? 1 : 0;
  a.seed_lo = uint32_t(seed);
  a.seed_hi = uint32_t(seed >> 32);
  a.draw_lo = uint32_t(draw);
  a.draw_hi = uint32_t(draw >> 32);
  const int pp = int(p * p);
  hipStream_t s = as_stream(stream);
  int64_t row0 = 0;
  for (int64_t first = 0; first < n_samples; first += kXfSamples) {   // the row offset carries across launches
    const int cnt = int(std::min<int64_t>(kXfSamples, n_samples - first));
    int64_t blocks = 0;
    for (int k = 0; k < kXfSamples; ++k) {
      const int64_t src_i = first + std::min(k, cnt - 1);
      const bsms_batch_sample& src = samples[src_i];
      XfSample& d = a.s[k];
      d.state_in = src.state_in; d.state_tar = src.state_tar; d.pos = src.pos; d.type = src.type;
      d.row0 = row0;
      d.blk0 = int32_t(blocks);
      d.n = k < cnt ? int32_t(src.n) : 0;
      for (int e = 0; e < 9; ++e) d.q[e] = e < pp ? xf[src_i * pp + e] : 0.f;
      if (k < cnt) {
        row0 += src.n;
        blocks += ceil_div(src.n, kRowsPerBlock);
      }
    }
    a.n_samples = cnt;
    if (blocks == 0) continue;
    hipLaunchKernelGGL(k_batch_assemble_xf, dim3((unsigned)blocks), dim3(kRowsPerBlock), 0, s, a, node_in, node_tar, node_mask, noise_out);
    BSMS_LAUNCH_CHECK();
  }
  return BSMS_OK;
}

namespace {

struct RowsSeg {
  int64_t row0;                      // first row of the segment inside a frame
  int32_t blk0, n;
  float q[9];                        // row-major [p, p], already transposed on the host when the call asks for Q^T
};
struct RowsArgs {
  RowsSeg s[kXfSamples];
  int32_t n_samples, C, p;
  int64_t frame;                     // elements of one frame: R * C
  int8_t first[kMaxRowW];
};
static_assert(sizeof(RowsArgs) + 2 * sizeof(void*) <= 4096, "k_rows_transform: the argument block exceeds 4 KB");

// x and out may be the same tensor: no __restrict__, and a thread forms every output of its row before it writes the first.
__global__ __launch_bounds__(kRowsPerBlock) void k_rows_transform(const RowsArgs a, const float* x, float* out) {
  int lo = 0, hi = a.n_samples - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (a.s[mid].blk0 <= int(blockIdx.x)) lo = mid; else hi = mid - 1;
  }
  const RowsSeg& sg = a.s[lo];
  const int i = (int(blockIdx.x) - sg.blk0) * kRowsPerBlock + int(threadIdx.x);
  if (i >= sg.n) return;
  const int C = a.C, p = a.p;
  const int64_t base = int64_t(blockIdx.y) * a.frame + (sg.row0 + i) * C;
  const float* row = x + base;
  float y[kMaxRowW];
#pragma unroll
  for (int c = 0; c < kMaxRowW; ++c) {
    if (c < C) {
      const int f = a.first[c];      // block-uniform
      y[c] = f >= 0 ? xf_row(sg.q, p, c - f, row + f) : row[c];
    }
  }
#pragma unroll
  for (int c = 0; c < kMaxRowW; ++c)
    if (c < C) out[base + c] = y[c];
}

}  // namespace

extern "C" int bsms_rows_transform(const float* x, float* out, int64_t F, int64_t R, int64_t C, const int64_t* rows, int64_t n_samples,
                                   int64_t p, const float* xf, int transpose, const int32_t* vec_first, int64_t n_vec,
                                   bsms_stream_t stream) {
  BSMS_REQUIRE(C >= 1 && C <= kMaxRowW && (p == 2 || p == 3) && n_vec >= 0 && n_vec <= kMaxVec, BSMS_E_UNSUPPORTED,
               "rows_transform: C=%lld p=%lld n_vec=%lld (C in 1..16, p in 2..3, n_vec in 0..4)", (long long)C, (long long)p, (long long)n_vec);
  BSMS_REQUIRE(F <= 65535, BSMS_E_UNSUPPORTED, "rows_transform: F=%lld (at most 65535 frames)", (long long)F);
  BSMS_REQUIRE(n_samples >= 0 && F >= 0 && R >= 0, BSMS_E_INVALID_ARG, "rows_transform: n_samples=%lld F=%lld R=%lld", (long long)n_samples,
               (long long)F, (long long)R);
  RowsArgs a;
  if (const int rc = xf_groups("rows_transform", C, p, vec_first, n_vec, a.first, kMaxRowW)) return rc;
  if (n_samples == 0 || F == 0) return BSMS_OK;
  BSMS_REQUIRE(x && out && rows && xf, BSMS_E_INVALID_ARG, "rows_transform: null argument");
  constexpr int64_t kMaxRows = (int64_t(1) << 31) / kBatchSamples - kRowsPerBlock;   // as bsms_batch_assemble
  int64_t total = 0;
  for (int64_t i = 0; i < n_samples; ++i) {
    BSMS_REQUIRE(rows[i] >= 0 && rows[i] <= kMaxRows, BSMS_E_UNSUPPORTED, "rows_transform: segment %lld has %lld rows (at most %lld)", (long long)i,
                 (long long)rows[i], (long long)kMaxRows);
    total += rows[i];
    BSMS_REQUIRE(total <= R, BSMS_E_INVALID_ARG, "rows_transform: the segments up to %lld hold %lld rows, a frame has %lld", (long long)i,
                 (long long)total, (long long)R);
  }
  a.C = int32_t(C);
  a.p = int32_t(p);
  a.frame = R * C;
  const int pi = int(p), pp = pi * pi;
  hipStream_t s = as_stream(stream);
  int64_t row0 = 0;
  for (int64_t first = 0; first < n_samples; first += kXfSamples) {
    const int cnt = int(std::min<int64_t>(kXfSamples, n_samples - first));
    int64_t blocks = 0;
    for (int k = 0; k < kXfSamples; ++k) {
      const int64_t src_i = first + std::min(k, cnt - 1);
      RowsSeg& d = a.s[k];
      d.row0 = row0;
      d.blk0 = int32_t(blocks);
      d.n = k < cnt ? int32_t(rows[src_i]) : 0;
      for (int e = 0; e < 9; ++e) d.q[e] = 0.f;
      for (int r = 0; r < pi; ++r)
        for (int c = 0; c < pi; ++c) d.q[r * pi + c] = transpose ? xf[src_i * pp + c * pi + r] : xf[src_i * pp + r * pi + c];
      if (k < cnt) {
        row0 += rows[src_i];
        blocks += ceil_div(rows[src_i], kRowsPerBlock);
      }
    }
    a.n_samples = cnt;
    if (blocks == 0) continue;
    hipLaunchKernelGGL(k_rows_transform, dim3((unsigned)blocks, (unsigned)F), dim3(kRowsPerBlock), 0, s, a, x, out);
    BSMS_LAUNCH_CHECK();
  }
  return BSMS_OK;
}
