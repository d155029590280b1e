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

constexpr int kMaxC = 8;             // state channels (sim.hip keeps the same bound)
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
