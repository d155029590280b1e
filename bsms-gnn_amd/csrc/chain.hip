// Weight prepack and the dispatch of a chain launch on the latent width (see chain.h for the register-layout idea).
// The chain kernels are templates over the width (chain_kernels.h, chain_edge.h) and their launchers live in chain_launch.h;
// each width is compiled in a translation unit of its own (chain_d32.hip ... chain_d256.hip).
#pragma clang fp contract(off)   // before the device helpers: chain_dev.h says why
#include <algorithm>

#include "chain_dev.h"

namespace {

// The whole prepack table in ONE launch (a training step packs 13 weight sets, three of them in front of kernels on the
// caller's stream): every workgroup of a pack repeats the scan for the matrix maximum (64-128 KB from L2) -> 2^-k_w, header
// float kScaleSlot of chunk 0, where the chain kernels read it -- and then writes its share of the pack.
__global__ __launch_bounds__(1024) void k_prepack_fused(PackTable tab) {
  const int nwg = gridDim.x * gridDim.y, wg = blockIdx.y * gridDim.x + blockIdx.x;
  if (tab.zero)   // clear the block's bound slots (chain.h: kBoundWidth), spread over the launch
    for (int o = wg * 1024 + threadIdx.x; o < kBoundSlots * kBoundWidth / 4; o += nwg * 1024)
      reinterpret_cast<float4*>(tab.zero)[o] = make_float4(0.f, 0.f, 0.f, 0.f);
  const PackDesc d = tab.d[blockIdx.y];
  if (d.kind == PACK_ROWS_BF16) { pack_rows_bf16(d, blockIdx.x * 1024 + threadIdx.x, gridDim.x * 1024); return; }
  if (d.kind == PACK_TRANSPOSE) {
    const int total = d.N * d.K;
    for (int o = blockIdx.x * 1024 + threadIdx.x; o < total; o += gridDim.x * 1024) {
      const int k = o / d.N, n = o % d.N;
      d.dst[o] = d.W[int64_t(d.row0 + n) * d.ld + d.col0 + k];
    }
    return;
  }
  float sw = 1.f;
  unsigned hdr_scale = 0;
  if (!d.bf16) {
    __shared__ float red[16];
    float m = 0.f;
    auto scan = [&](const PackDesc& e) {   // coalesced along the rows of W whatever the logical orientation
      const int rows = (e.kind == PACK_FRAG_T) ? e.K : e.N, cols = (e.kind == PACK_FRAG_T) ? e.N : e.K;
      const int tr = threadIdx.x / cols, tc = threadIdx.x % cols, step = 1024 / cols;   // cols divides 1024 (32 .. 256)
      const float* base = e.W + int64_t(e.row0) * e.ld + e.col0 + tc;
      int r = tr;
      for (; r + 7 * step < rows; r += 8 * step) {   // eight independent loads in flight (one at a time: 16-64 dependent L2 round trips)
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = base[int64_t(r + u * step) * e.ld];
#pragma unroll
        for (int u = 0; u < 8; ++u) m = fmaxf(m, fabsf(v[u]));
      }
      for (; r < rows; r += step) m = fmaxf(m, fabsf(base[int64_t(r) * e.ld]));
    };
    scan(d);
    if (d.mate) scan(tab.d[d.mate - 1]);
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) m = fmaxf(m, __shfl_xor(m, o, 64));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    m = red[0];
#pragma unroll
    for (int w = 1; w < 16; ++w) m = fmaxf(m, red[w]);
    int Ew = int(__float_as_uint(m) >> 23);
    Ew = Ew < 13 ? 13 : (Ew > 254 ? 254 : Ew);            // 2^(139 - Ew) and its inverse are normal floats
    hdr_scale = unsigned(Ew - 12) << 23;                   // 2^(Ew - 139) = 2^-k_w  (header float kScaleSlot of chunk 0)
    sw = __uint_as_float(unsigned(254 - (Ew - 12)) << 23); // 2^k_w
  }
  const int nb = d.N >> 4, planes = d.bf16 ? 1 : kPL, chf = kChunkHdrFloats + nb * 256 * planes, nch = d.K >> 5;
  const int total = nch * chf;
  unsigned* dst = reinterpret_cast<unsigned*>(d.dst);
  // four pack dwords per round: their eight weight loads are in flight together
  const int stride = gridDim.x * 1024;
  for (int o0 = blockIdx.x * 1024 + threadIdx.x; o0 < total; o0 += 4 * stride) {
    float x0[4], x1[4];
    bool body_[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int o = o0 + u * stride, w = o % chf;
      body_[u] = o < total && w >= kChunkHdrFloats;
      x0[u] = x1[u] = 0.f;
      if (body_[u]) {
        const int c = o / chf, q = w - kChunkHdrFloats;
        const int v = q & 3, lane = (q >> 2) & 63, tp = q >> 8, t = tp / planes;
        const int n = 16 * t + (lane & 15), k = 16 * (2 * c + ((2 * v) >> 2)) + 4 * (lane >> 4) + ((2 * v) & 3);   // slots 2v, 2v + 1
        x0[u] = pack_elem(d, n, k);
        x1[u] = pack_elem(d, n, k + 1);
      }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int o = o0 + u * stride;
      if (o >= total) break;
      const int c = o / chf, w = o % chf;
      if (!body_[u]) {   // chunk header
        float v = 0.f;
        if (d.bf16) {
          if (c == 0 && d.bias && w < d.N) v = d.bias[w];
        } else {
          if (c == nch - 1 && d.bias && w < d.N) v = d.bias[w];
          if (c == 0 && w == kScaleSlot) { dst[o] = hdr_scale; continue; }   // (nch == 1 means N = 32: no clash with the bias)
        }
        d.dst[o] = v;
        continue;
      }
      const int plane = ((w - kChunkHdrFloats) >> 8) % planes;
      if (d.bf16) {
        dst[o] = pk_bf16(x0[u], x1[u]);
      } else {
        unsigned h, l;
        split_h2(x0[u], x1[u], sw, h, l);
        dst[o] = plane == 0 ? h : l;
      }
    }
  }
}

}  // namespace

namespace bsms {

int launch_prepack(const PackTable& t, hipStream_t s) {
  if (t.n == 0) return BSMS_OK;
  int biggest = 0;
  for (int i = 0; i < t.n; ++i) biggest = biggest > t.d[i].N * t.d[i].K ? biggest : t.d[i].N * t.d[i].K;
  hipLaunchKernelGGL(k_prepack_fused, dim3((unsigned)std::min<int64_t>(ceil_div(biggest, 4096), 16), t.n), dim3(1024), 0, s, t);
  BSMS_LAUNCH_CHECK();
  return BSMS_OK;
}

int launch_chain_fwd(int D, int in_mode, int out_mode, const ChainFwdArgs& a, hipStream_t s) {
  if (a.R == 0) return BSMS_OK;
  switch (D) {   // one translation unit per width: chain_d32.hip ... chain_d256.hip
    case 32: return launch_chain_fwd_nb<2>(in_mode, out_mode, a, s);
    case 64: return launch_chain_fwd_nb<4>(in_mode, out_mode, a, s);
    case 96: return launch_chain_fwd_nb<6>(in_mode, out_mode, a, s);
    case 128: return launch_chain_fwd_nb<8>(in_mode, out_mode, a, s);
    case 160: return launch_chain_fwd_nb<10>(in_mode, out_mode, a, s);
    case 192: return launch_chain_fwd_nb<12>(in_mode, out_mode, a, s);
    case 224: return launch_chain_fwd_nb<14>(in_mode, out_mode, a, s);
    case 256: return launch_chain_fwd_nb<16>(in_mode, out_mode, a, s);
  }
  BSMS_FAIL(BSMS_E_UNSUPPORTED, "latent width D=%d not supported (a multiple of 32, 32..256)", D);
}

int launch_chain_bwd(int D, int gin, int first, const ChainBwdArgs& a, hipStream_t s) {
  if (a.R == 0) return BSMS_OK;
  switch (D) {
    case 32: return launch_chain_bwd_nb<2>(gin, first, a, s);
    case 64: return launch_chain_bwd_nb<4>(gin, first, a, s);
    case 96: return launch_chain_bwd_nb<6>(gin, first, a, s);
    case 128: return launch_chain_bwd_nb<8>(gin, first, a, s);
    case 160: return launch_chain_bwd_nb<10>(gin, first, a, s);
    case 192: return launch_chain_bwd_nb<12>(gin, first, a, s);
    case 224: return launch_chain_bwd_nb<14>(gin, first, a, s);
    case 256: return launch_chain_bwd_nb<16>(gin, first, a, s);
  }
  BSMS_FAIL(BSMS_E_UNSUPPORTED, "latent width D=%d not supported (a multiple of 32, 32..256)", D);
}

}  // namespace bsms
