// What the resident-weight edge kernels of the bf16 precisions (efwd.hip: k_edge_fwd_res; efuse.hip: k_edge_fused_bwd, k_edge_data_bwd)
// share with each other and with nobody else.  Everything the chain kernels have too (pk_bf16, glds16, group_sum, load_rows,
// axpy_features, ...) comes from chain_dev.h, which wants `#pragma clang fp contract(off)` in front of this include.
#pragma once
#include "chain_dev.h"

namespace {

using u32x2 = __attribute__((ext_vector_type(2))) unsigned;

// one bf16 product with BOTH operands in registers as packed pairs (chain_dev.h: mma_bf takes its A operand as the float4 of an LDS ring)
__device__ __forceinline__ f32x4 mma(const u32x4& a, const u32x4& b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8, a), __builtin_bit_cast(bf16x8, b), c, 0, 0, 0);
}

// relu + round to bf16: the B operand of the next Linear (chain_dev.h: relu_into + round_block) -- and, in the backward, the
// activation a_l itself
template <int NB>
__device__ __forceinline__ void relu_pack(u32x4 (&bb)[NB / 2], const f32x4 (&acc)[NB]) {
  // round first, then clamp the PAIR with one packed signed-integer max: a bf16 with its sign bit set (a negative value or
  // -0) is a negative int16, so max(., 0) is +0, and a non-negative one is left alone -- the bits of pk_bf16(max(x, 0), max(y, 0))
  // for every non-NaN input (rounding keeps the sign), in two operations per pair instead of three
#pragma unroll
  for (int c = 0; c < NB / 2; ++c)
#pragma unroll
    for (int v = 0; v < 4; ++v) {
      const unsigned w = pk_bf16(acc[2 * c + (v >> 1)][2 * (v & 1)], acc[2 * c + (v >> 1)][2 * (v & 1) + 1]);
      asm("v_pk_max_i16 %0, %1, 0" : "=v"(bb[c][v]) : "v"(w));
    }
}

// chain_dev.h's edge_ref with an exact fallback: these kernels take any [B, E] with B E < 2^31 (their launchers), and with a tiny
// E and a huge B the reciprocal estimate can be off by more than the one step edge_ref corrects
__device__ __forceinline__ EdgeRef edge_ref_exact(unsigned row, unsigned E, float rcpE) {
  EdgeRef e = edge_ref(row, E, rcpE);
  if (unsigned(e.q) >= E) { e.b = int(row / E); e.q = int(row - unsigned(e.b) * E); }
  return e;
}

}  // namespace
