// Normaliser moments of resident trajectories (include/bsms_hip_stats.h: bsms_moment_sums, bsms_moment_fold), built
// into the second companion library libbsms_hip_stats.so: the surfaces of libbsms_hip.so and libbsms_hip_ext.so are closed.
// Per table entry (one trajectory, the pairs (t, t+1) of `frames` frames) over its R = frames * n rows:
//   [ R | M | SX[C] | ST | QX[C] | QT | SD[C] | QD[C] ],   d = fl32(state[t+1] - state[t]), every product and sum after it fp64.
// A memory-bound streaming reduction.  A frame is a flat array of E = n * C floats (rows of 12 bytes when C = 3, frames that start
// at any multiple of 4 bytes): a thread owns kElems elements kThreads apart -- every load of a wave is one contiguous run of 256
// bytes, whatever n * C is -- and walks the frames of its chunk through a ring of kRing frames in registers (two being summed, the
// others in flight), so every state element is read once (a chunk re-reads its first frame).  Deterministic, no atomics: the piece
// sum of piece_sum.h with a piece = slab x frame chunk; k_moment_finish is table-driven (R comes from the shapes)
// and adds the pieces of an entry with the shared in-order add, bsms_moment_fold is the shared row fold.
// Compiled with -ffp-contract=off (build.py): the sums keep the roundings of separate fp64 multiplies and adds.
#include "../piece_sum.h"
#include "../../../include/bsms_hip_stats.h"

#pragma clang fp contract(off)

using namespace bsms;

namespace {

constexpr int kMaxValid = 4;                            // node-type codes that count for the mask (batch.hip)
constexpr int kMaxW = 4 * kMaxC + 4;                    // columns of a row of `sums`
constexpr int kThreads = 256;                           // four waves of 64
constexpr int kElems = 4;                               // elements of a frame per thread
constexpr int kSlab = kThreads * kElems;                // 1024 elements of a frame per block
constexpr int kFrameChunk = 32;                         // frame pairs per block
constexpr int kRing = 4;                                // frames a thread holds: two being summed, the others in flight
constexpr int kEntries = 64;                            // table entries per launch: the table is a kernel argument
constexpr int64_t kMinPieces = 4096;                    // pieces the work area holds at least
constexpr int64_t kMaxBlocksPerLaunch = int64_t(1) << 20;   // 2^28 threads: well below the 2^32 work items of one dispatch
constexpr int64_t kMaxRows = int64_t(1) << 40;

struct MomentEntry {
  const float *state, *type;                            // frame frame0 of each
  int64_t n, frames, type_stride;
  int64_t blk0;                                         // first piece of the entry in this launch
};
struct MomentArgs {
  MomentEntry e[kEntries];
  float valid[kMaxValid];
  int32_t n_entries, n_valid;
  int64_t blk_off;                                      // piece index of block 0 of this dispatch (a launch of many pieces is cut)
};
static_assert(sizeof(MomentArgs) + 4 * sizeof(void*) <= 4096, "k_moment_pieces: the argument block exceeds 4 KB");

inline int64_t slabs_of(int64_t n, int64_t C) { return ceil_div(n * C, kSlab); }
inline int64_t pieces_of(int64_t n, int64_t frames, int64_t C) { return (n == 0 || frames == 0) ? 0 : slabs_of(n, C) * ceil_div(frames, kFrameChunk); }

// pieces of any entry of at most `rows` rows: ceil(n C / 1024) ceil(frames / 32) <= (n / 128 + 1)(frames / 32 + 1) with C <= 8, and
// n, frames <= rows
inline int64_t piece_cap(int64_t rows) { return std::max(kMinPieces, rows / 4096 + rows / 128 + rows / 32 + 4); }

// a row of type `ty` added to what a thread's rows add to M, ST and QT per frame
__device__ __forceinline__ void type_terms(float ty, const MomentArgs& a, double& m, double& y, double& y2) {
  bool valid = false;
  for (int k = 0; k < a.n_valid; ++k) valid |= (ty == a.valid[k]);
  const double v = double(ty);
  m += valid ? 1.0 : 0.0;
  y += v;
  y2 += v * v;
}

// columns of a piece: [ M | SX[C] | ST | QX[C] | QT | SD[C] | QD[C] ] -- a row of `sums` without R, which the shapes give
template <int C>
__global__ __launch_bounds__(kThreads) void k_moment_pieces(const MomentArgs a, double* __restrict__ partials) {
  constexpr int kCols = 4 * C + 3;
  const int64_t blk = a.blk_off + int64_t(blockIdx.x);
  // which entry does this block belong to: block-uniform search over at most 64 entries of the argument table
  int lo = 0, hi = a.n_entries - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (a.e[mid].blk0 <= blk) lo = mid; else hi = mid - 1;
  }
  const MomentEntry& en = a.e[lo];
  const int64_t E = en.n * C, slabs = (E + kSlab - 1) / kSlab;
  const int64_t piece = blk - en.blk0, chunk = piece / slabs, slab = piece - chunk * slabs;
  const int64_t t0 = chunk * kFrameChunk;
  const int t_cnt = int(en.frames - t0 < kFrameChunk ? en.frames - t0 : kFrameChunk);      // >= 1: the piece exists
  const bool per_frame = en.type_stride != 0;
  const float* state = en.state + t0 * E;
  const float* type = en.type + t0 * en.type_stride;

  int64_t elem[kElems], node[kElems];
  int ch[kElems];
  bool ok[kElems], head[kElems];                        // head: the element is channel 0 of its row -- it carries the row's type
  float ring[kRing][kElems];                            // ring[k % kRing] holds frame t0 + k while it is needed
  double Mt = 0.0, Yt = 0.0, Y2t = 0.0;                 // what the thread's head elements add to M, ST, QT per frame (q ascending)
  const float* slab_state = state + slab * kSlab;       // block-uniform base + a 32-bit lane offset per load
  const unsigned lane_off = threadIdx.x;
#pragma unroll
  for (int q = 0; q < kElems; ++q) {
    elem[q] = slab * kSlab + q * kThreads + int(threadIdx.x);
    ok[q] = elem[q] < E;
    node[q] = elem[q] / C;
    ch[q] = int(elem[q] - node[q] * C);
    head[q] = ok[q] && ch[q] == 0;
    if (head[q] && !per_frame) type_terms(type[node[q]], a, Mt, Yt, Y2t);
  }
  // frames t0 .. t0 + kRing - 1 in flight before the first sum; frame t0 + t_cnt exists (the caller's guarantee)
#pragma unroll
  for (int k = 0; k < kRing; ++k) {
#pragma unroll
    for (int q = 0; q < kElems; ++q) ring[k][q] = (k <= t_cnt && ok[q]) ? (slab_state + k * E)[q * kThreads + lane_off] : 0.f;
  }

  double sx[kElems], qx[kElems], sd[kElems], qd[kElems];
  double M = 0.0, ST = 0.0, QT = 0.0;
#pragma unroll
  for (int q = 0; q < kElems; ++q) sx[q] = qx[q] = sd[q] = qd[q] = 0.0;

  // pair t reads ring[t % kRing] and ring[(t + 1) % kRing], then refills the slot it has finished with frame t + kRing: kRing - 1
  // frames stay in flight per thread.  The loop is unrolled by kRing so that every ring index is static.
  for (int tb = 0; tb < t_cnt; tb += kRing) {
#pragma unroll
    for (int k = 0; k < kRing; ++k) {
      const int t = tb + k;
      if (t < t_cnt) {                                  // block-uniform
        const float* prev = ring[k];
        const float* cur = ring[(k + 1) % kRing];
        if (per_frame) {
          Mt = Yt = Y2t = 0.0;
#pragma unroll
          for (int q = 0; q < kElems; ++q)
            if (head[q]) type_terms(type[t * en.n + node[q]], a, Mt, Yt, Y2t);
        }
        M += Mt;
        ST += Yt;
        QT += Y2t;
#pragma unroll
        for (int q = 0; q < kElems; ++q) {              // an element past the frame holds zeros and adds +0.0
          const float d = cur[q] - prev[q];             // the fp32 subtraction of the reference
          const double x = double(prev[q]), dd = double(d);
          sx[q] += x;
          qx[q] += x * x;
          sd[q] += dd;
          qd[q] += dd * dd;
        }
        const bool more = t + kRing <= t_cnt;
#pragma unroll
        for (int q = 0; q < kElems; ++q) ring[k][q] = (more && ok[q]) ? (slab_state + (t + kRing) * E)[q * kThreads + lane_off] : 0.f;
      }
    }
  }

  // the thread's four elements into the channel columns, q ascending (a select per channel: no register array under a runtime index)
  double acc[kCols];
#pragma unroll
  for (int k = 0; k < kCols; ++k) acc[k] = 0.0;
  acc[0] = M;
  acc[1 + C] = ST;
  acc[2 + 2 * C] = QT;
#pragma unroll
  for (int q = 0; q < kElems; ++q) {
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const bool mine = ok[q] && ch[q] == c;
      acc[1 + c] += mine ? sx[q] : 0.0;
      acc[2 + C + c] += mine ? qx[q] : 0.0;
      acc[3 + 2 * C + c] += mine ? sd[q] : 0.0;
      acc[3 + 3 * C + c] += mine ? qd[q] : 0.0;
    }
  }
  psum::block_sum<kThreads>(acc, psum::Dense<kCols>(), partials + blk * kCols);
}

// row of entry k of the launch: R from the shapes, every other column the entry's pieces in index order; one block per entry
__global__ __launch_bounds__(64) void k_moment_finish(const MomentArgs a, int C, const double* __restrict__ partials,
                                                      double* __restrict__ sums /* row of the launch's first entry */) {
  const MomentEntry& en = a.e[blockIdx.x];
  const int col = int(threadIdx.x), W = 4 * C + 4, cols = W - 1;
  if (col >= W) return;
  const int64_t E = en.n * C;
  const int64_t pieces = (en.n == 0 || en.frames == 0) ? 0 : ((E + kSlab - 1) / kSlab) * ((en.frames + kFrameChunk - 1) / kFrameChunk);
  sums[int64_t(blockIdx.x) * W + col] =
      col == 0 ? double(en.frames * en.n) : psum::add_in_order(partials + en.blk0 * cols + (col - 1), pieces, cols);
}

}  // namespace

extern "C" size_t bsms_moment_work_bytes(int64_t max_rows) {
  return size_t(piece_cap(std::max<int64_t>(max_rows, 0))) * (kMaxW - 1) * sizeof(double);
}

// The checks in the order of the header, all before any device call.
extern "C" int bsms_moment_sums(const bsms_moment_traj* trajs, int64_t S, int64_t C, const float* valid_types, int64_t n_valid,
                                double* sums, void* work, bsms_stream_t stream) {
  BSMS_REQUIRE(C >= 1 && C <= kMaxC && n_valid >= 1 && n_valid <= kMaxValid, BSMS_E_UNSUPPORTED,
               "moment_sums: C=%lld n_valid=%lld (C in 1..8, n_valid in 1..4)", (long long)C, (long long)n_valid);
  BSMS_REQUIRE(S >= 0, BSMS_E_INVALID_ARG, "moment_sums: S=%lld", (long long)S);
  if (S == 0) return BSMS_OK;
  BSMS_REQUIRE(trajs && valid_types && sums && work, BSMS_E_INVALID_ARG, "moment_sums: null argument");
  int64_t max_rows = 0;
  for (int64_t i = 0; i < S; ++i) {
    const bsms_moment_traj& t = trajs[i];
    BSMS_REQUIRE(t.n >= 0 && t.frame0 >= 0 && t.frames >= 0, BSMS_E_INVALID_ARG, "moment_sums: entry %lld has n=%lld frame0=%lld frames=%lld",
                 (long long)i, (long long)t.n, (long long)t.frame0, (long long)t.frames);
    BSMS_REQUIRE(t.type_stride == 0 || t.type_stride == t.n, BSMS_E_INVALID_ARG, "moment_sums: entry %lld has type_stride=%lld (0 or n=%lld)",
                 (long long)i, (long long)t.type_stride, (long long)t.n);
    const bool empty = t.n == 0 || t.frames == 0;
    BSMS_REQUIRE(empty || (t.state && t.type), BSMS_E_INVALID_ARG, "moment_sums: entry %lld has a null field", (long long)i);
    BSMS_REQUIRE(empty || t.frames <= (kMaxRows - 1) / t.n, BSMS_E_SHAPE, "moment_sums: entry %lld has %lld x %lld rows (below 2^40)",
                 (long long)i, (long long)t.frames, (long long)t.n);
    if (!empty) max_rows = std::max(max_rows, t.frames * t.n);
  }
  const int64_t cap = piece_cap(max_rows);              // what `work` holds: every entry fits (piece_cap bounds its pieces)
  const int W = int(4 * C + 4);
  double* partials = static_cast<double*>(work);
  hipStream_t s = as_stream(stream);
  MomentArgs a;
  a.n_valid = int32_t(n_valid);
  for (int k = 0; k < kMaxValid; ++k) a.valid[k] = k < n_valid ? valid_types[k] : valid_types[0];
  for (int64_t first = 0; first < S;) {                 // one launch pair: up to 64 entries whose pieces fit the work area
    int cnt = 0;
    int64_t blocks = 0;
    while (cnt < kEntries && first + cnt < S) {
      const bsms_moment_traj& t = trajs[first + cnt];
      const int64_t pieces = pieces_of(t.n, t.frames, C);
      if (cnt > 0 && blocks + pieces > cap) break;
      MomentEntry& d = a.e[cnt];
      d.state = t.state ? t.state + t.frame0 * t.n * C : nullptr;
      d.type = t.type ? t.type + t.frame0 * t.type_stride : nullptr;
      d.n = t.n; d.frames = t.frames; d.type_stride = t.type_stride;
      d.blk0 = blocks;
      blocks += pieces;
      ++cnt;
    }
    // an entry without pieces shares blk0 with its successor (or lies above every block): the search takes the LAST entry whose
    // blk0 is not above the block, which is the one that owns it.  The unused tail repeats the last entry and is never searched.
    for (int k = cnt; k < kEntries; ++k) {
      a.e[k] = a.e[cnt - 1];
      a.e[k].blk0 = blocks;
    }
    a.n_entries = cnt;
    const int rc = psum::for_block_slices(blocks, kMaxBlocksPerLaunch, [&](int64_t b0, unsigned nb) {
      a.blk_off = b0;
      psum::by_channels(int(C), [&](auto c) {
        hipLaunchKernelGGL((k_moment_pieces<decltype(c)::value>), dim3(nb), dim3(kThreads), 0, s, a, partials);
      });
    });
    if (rc) return rc;
    a.blk_off = 0;
    hipLaunchKernelGGL(k_moment_finish, dim3(unsigned(cnt)), dim3(64), 0, s, a, int(C), partials, sums + first * W);
    BSMS_LAUNCH_CHECK();
    first += cnt;
  }
  return BSMS_OK;
}

extern "C" int bsms_moment_fold(const double* sums, int64_t S, int64_t W, double* out, bsms_stream_t stream) {
  BSMS_REQUIRE(W >= 1 && W <= 65536, BSMS_E_UNSUPPORTED, "moment_fold: W=%lld (W in 1..65536)", (long long)W);
  BSMS_REQUIRE(S >= 0, BSMS_E_INVALID_ARG, "moment_fold: S=%lld", (long long)S);
  BSMS_REQUIRE(out && (sums || S == 0), BSMS_E_INVALID_ARG, "moment_fold: null argument");
  psum::launch_fold(sums, S, W, W, out, as_stream(stream));
  BSMS_LAUNCH_CHECK();
  return BSMS_OK;
}
