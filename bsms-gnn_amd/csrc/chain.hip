// Weight prepack and the dispatch of a chain launch on the latent width (see chain.h for the register-layout idea).
// The chain kernels are templates over the width (chain_kernels.h, chain_edge.h) and their launchers live in chain_launch.h;
// each width is compiled in a translation unit of its own (chain_d32.hip ... chain_d256.hip).
#pragma clang fp contract(off)   // before the device helpers: chain_dev.h says why
#include <algorithm>

#include "chain_dev.h"

namespace {

// Exact x / m for the small operands of the pack loops: multiply and shift instead of an integer division per element.  With
// inv = ceil(2^16 / m) the quotient is exact while x * (inv * m - 2^16) < 2^16, which x * (m - 1) < 2^16 ensures (here x < 400, m <= 33)
struct SmallDiv {
  unsigned inv;
  __device__ explicit SmallDiv(int m) : inv((65536u + unsigned(m) - 1u) / unsigned(m)) {}
  __device__ int operator()(int x) const { return int((unsigned(x) * inv) >> 16); }
};

// One pack, written by `nx` workgroups of 1024 threads (this one: `bx`).  Each of the nx workgroups of a FRAG pack scans for the
// matrix maximum itself (64-128 KB from L2; k_prepack_group runs nx = 1 up to 128 x 128: one scan per pack) -> 2^-k_w, header float kScaleSlot of chunk 0, where the chain kernels read it -- and then
// writes its share of the pack.  SU: scan loads in flight per thread; PU: pack dwords per round (2 PU weight loads in flight).
// What is written does not depend on nx, SU or PU.
template <int SU, int PU>
__device__ __forceinline__ void prepack_one(const PackDesc& d, const PackDesc& mate, int bx, int nx) {
  if (d.kind == PACK_ROWS_BF16) { pack_rows_bf16(d, bx * 1024 + threadIdx.x, nx * 1024); return; }
  if (d.kind == PACK_TRANSPOSE) {
    const int total = d.N * d.K;
    for (int o = bx * 1024 + threadIdx.x; o < total; o += nx * 1024) {
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
      for (; r + (SU - 1) * step < rows; r += SU * step) {   // SU independent loads in flight (one at a time: 16-64 dependent L2 round trips)
        float v[SU];
#pragma unroll
        for (int u = 0; u < SU; ++u) v[u] = base[int64_t(r + u * step) * e.ld];
#pragma unroll
        for (int u = 0; u < SU; ++u) m = fmaxf(m, fabsf(v[u]));
      }
      for (; r < rows; r += step) m = fmaxf(m, fabsf(base[int64_t(r) * e.ld]));
    };
    scan(d);
    if (d.mate) scan(mate);
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
  const int nb = d.N >> 4, pshift = d.bf16 ? 0 : 1, planes = 1 << pshift;   // kPL = 2 planes in the fp32 path
  static_assert(kPL == 2, "prepack_one: the plane index is a shift");
  const int chq = 1 + nb * planes, chf = chq << 8, nch = d.K >> 5;   // chunk = kChunkHdrFloats + nb * 256 * planes dwords, a multiple of 256
  static_assert(kChunkHdrFloats == 256, "prepack_one: chunks are counted in 256-dword pieces");
  const SmallDiv by_chq(chq);                            // (o >> 8) < nch * chq <= 8 * 33
  const int total = nch * chf;
  unsigned* dst = reinterpret_cast<unsigned*>(d.dst);
  // PU pack dwords per round: their 2 PU weight loads are in flight together
  const int stride = nx * 1024;
  for (int o0 = bx * 1024 + threadIdx.x; o0 < total; o0 += PU * stride) {
    float x0[PU], x1[PU];
    bool body_[PU];
#pragma unroll
    for (int u = 0; u < PU; ++u) {
      const int o = o0 + u * stride, c = by_chq(o >> 8), w = o - c * chf;
      body_[u] = o < total && w >= kChunkHdrFloats;
      x0[u] = x1[u] = 0.f;
      if (body_[u]) {
        const int q = w - kChunkHdrFloats;
        const int v = q & 3, lane = (q >> 2) & 63, tp = q >> 8, t = tp >> pshift;
        const int n = 16 * t + (lane & 15), k = 16 * (2 * c + ((2 * v) >> 2)) + 4 * (lane >> 4) + ((2 * v) & 3);   // slots 2v, 2v + 1
        x0[u] = pack_elem(d, n, k);
        x1[u] = pack_elem(d, n, k + 1);
      }
    }
#pragma unroll
    for (int u = 0; u < PU; ++u) {
      const int o = o0 + u * stride;
      if (o >= total) break;
      const int c = by_chq(o >> 8), w = o - c * chf;
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
      const int plane = ((w - kChunkHdrFloats) >> 8) & (planes - 1);
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

// The whole prepack table of one MLP / GMP block in ONE launch: grid (workgroups per pack, packs)
__global__ __launch_bounds__(1024) void k_prepack_fused(PackTable tab) {
  const int nwg = gridDim.x * gridDim.y, wg = blockIdx.y * gridDim.x + blockIdx.x;
  if (tab.zero)   // clear the block's bound slots (chain.h: kBoundWidth), spread over the launch
    for (int o = wg * 1024 + threadIdx.x; o < kBoundSlots * kBoundWidth / 4; o += nwg * 1024)
      reinterpret_cast<float4*>(tab.zero)[o] = make_float4(0.f, 0.f, 0.f, 0.f);
  const PackDesc d = tab.d[blockIdx.y];
  prepack_one<8, 4>(d, tab.d[d.mate ? d.mate - 1 : blockIdx.y], blockIdx.x, gridDim.x);
}

// The tables of a whole training step (chain.h: PackGroup), descriptors and clear list in device memory.  A training step packs 13
// tables, three of them in front of kernels on the caller's stream; as 13 launches of k_prepack_fused they are 13 latency chains of
// 23-27 us on 84 CUs each.  Here a D <= 128 pack is ONE workgroup's (its matrix is scanned once, not four times), the scan keeps 16
// and the pack loop 12 loads in flight, and 273 workgroups fill the chip once
// (55 registers under the cap of 64: two workgroups fit a CU, so the 17 beyond 256 do not wait for a first wave of workgroups to end).
constexpr int kBoundFloat4 = kBoundSlots * kBoundWidth / 4;
static_assert((kBoundFloat4 & (kBoundFloat4 - 1)) == 0, "k_prepack_group: array index and offset by shift and mask");
__global__ __launch_bounds__(1024, 8) void k_prepack_group(const PackDesc* __restrict__ descs, float* const* __restrict__ zeros, int nzero) {
  const int nwg = gridDim.x * gridDim.y, wg = blockIdx.y * gridDim.x + blockIdx.x;
  for (int o = wg * 1024 + threadIdx.x; o < nzero * kBoundFloat4; o += nwg * 1024)   // every member's bound slots, spread over the launch
    reinterpret_cast<float4*>(zeros[o / kBoundFloat4])[o % kBoundFloat4] = make_float4(0.f, 0.f, 0.f, 0.f);
  const PackDesc d = descs[blockIdx.y];
  prepack_one<16, 6>(d, descs[d.mate ? d.mate - 1 : blockIdx.y], blockIdx.x, gridDim.x);
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

void pack_group_append(PackGroup& g, const PackTable& t) {
  const int base = int(g.descs.size());
  for (int i = 0; i < t.n; ++i) {
    PackDesc d = t.d[i];
    if (d.mate) d.mate += base;
    g.biggest = std::max(g.biggest, d.N * d.K);
    g.descs.push_back(d);
  }
  if (t.zero) g.zeros.push_back(t.zero);
}

int launch_prepack_group(PackGroup& g, hipStream_t s) {
  if (g.descs.empty() && g.zeros.empty()) return BSMS_OK;
  BSMS_REQUIRE(g.descs.size() <= 65535 && g.zeros.size() < size_t(1) << 14, BSMS_E_SHAPE, "pack_group_launch: %zu packs, %zu bound arrays",
               g.descs.size(), g.zeros.size());
  BSMS_REQUIRE(!g.descs.empty(), BSMS_E_INVALID_ARG, "pack_group_launch: bound arrays without a pack");
  int dev = 0;
  BSMS_HIP_CHECK(hipGetDevice(&dev));
  const size_t dbytes = align_up(g.descs.size() * sizeof(PackDesc)), zbytes = std::max<size_t>(g.zeros.size(), 1) * sizeof(float*);
  if (!g.dev) {   // the one upload: a blocking copy, so never inside a stream capture
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    BSMS_HIP_CHECK(hipStreamIsCapturing(s, &cap));
    BSMS_REQUIRE(cap == hipStreamCaptureStatusNone, BSMS_E_INVALID_ARG,
                 "pack_group_launch: the first launch of a group uploads its tables and cannot be captured (launch it once before the capture)");
    void* p = nullptr;
    BSMS_HIP_CHECK(hipMalloc(&p, dbytes + zbytes));
    hipError_t e = hipMemcpy(p, g.descs.data(), g.descs.size() * sizeof(PackDesc), hipMemcpyHostToDevice);
    if (e == hipSuccess && !g.zeros.empty())
      e = hipMemcpy(static_cast<char*>(p) + dbytes, g.zeros.data(), g.zeros.size() * sizeof(float*), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
      (void)hipFree(p);
      BSMS_FAIL(BSMS_E_HIP, "pack_group_launch: upload: %s", hipGetErrorString(e));
    }
    g.dev = p;
    g.device = dev;
  }
  BSMS_REQUIRE(g.device == dev, BSMS_E_INVALID_ARG, "pack_group_launch: the group was uploaded to device %d, the current device is %d", g.device, dev);
  // one workgroup per pack up to 128 x 128, two to four for the wider ones (their scan and their pack loop are four times as long)
  const unsigned nx = (unsigned)std::min<int64_t>(ceil_div(g.biggest, 16384), 4);
  hipLaunchKernelGGL(k_prepack_group, dim3(nx, (unsigned)g.descs.size()), dim3(1024), 0, s, static_cast<const PackDesc*>(g.dev),
                     reinterpret_cast<float* const*>(static_cast<char*>(g.dev) + dbytes), int(g.zeros.size()));
  BSMS_LAUNCH_CHECK();
  return BSMS_OK;
}

int launch_chain_fwd(int D, int in_mode, int out_mode, const ChainFwdArgs& a, hipStream_t s) {
  if (a.R == 0) return BSMS_OK;
  return with_width(D, [&](auto nb) { return launch_chain_fwd_nb<decltype(nb)::value>(in_mode, out_mode, a, s); });
}

int launch_chain_bwd(int D, int gin, int first, const ChainBwdArgs& a, hipStream_t s) {
  if (a.R == 0) return BSMS_OK;
  return with_width(D, [&](auto nb) { return launch_chain_bwd_nb<decltype(nb)::value>(gin, first, a, s); });
}

}  // namespace bsms

// The pack group behind its ABI handle (bsms_pack_group_*; the members are added by bsms_pack_group_add_mlp, mlp.hip, and
// bsms_pack_group_add_bsgmp, bsgmp.hip)
struct bsms_pack_group {
  bsms::PackGroup g;
};

extern "C" int bsms_pack_group_create(bsms_pack_group_t** out) {
  BSMS_REQUIRE(out != nullptr, BSMS_E_INVALID_ARG, "pack_group_create: null argument");
  *out = new bsms_pack_group();   // host state only: the device image is made by the first launch
  return BSMS_OK;
}

extern "C" void bsms_pack_group_destroy(bsms_pack_group_t* group) {
  if (!group) return;
  if (group->g.dev) (void)hipFree(group->g.dev);   // waits for a launch still reading the tables
  delete group;
}

int bsms::pack_group_open(bsms_pack_group_t* group, const char* who, PackGroup** g) {
  BSMS_REQUIRE(group != nullptr, BSMS_E_INVALID_ARG, "%s: the group is null", who);
  BSMS_REQUIRE(group->g.dev == nullptr, BSMS_E_INVALID_ARG, "%s: the group has been launched and is sealed (other pointers, shapes or "
               "precision: build a new group)", who);
  *g = &group->g;
  return BSMS_OK;
}

extern "C" int bsms_pack_group_launch(bsms_pack_group_t* group, bsms_stream_t stream) {
  BSMS_REQUIRE(group != nullptr, BSMS_E_INVALID_ARG, "pack_group_launch: the group is null");
  return bsms::launch_prepack_group(group->g, bsms::as_stream(stream));
}
