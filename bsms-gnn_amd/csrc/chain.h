// MLP "chain" kernels for gfx950: the dense per-edge / per-node MLPs of the BSMS path on the matrix cores.
//
// Orientation.  Every Linear y = x W^T is computed TRANSPOSED, Y^T = W X^T: the A operand of an MFMA is a weight
// fragment (rows = output features), the B operand an activation fragment (columns = rows of x, i.e. edges /
// nodes).  Each wave owns 16 rows of x: lane l <-> row (l & 15), lane group g = l >> 4.  The 16x16 result block
// leaves a lane holding, for ITS row, output features  f = 16 t + 4 g + r  (r = accumulator register 0..3,
// t = 16-feature block).  An MFMA sums over K slots (g, i) supplied by the four lane groups; we are free to decide
// WHICH input feature each slot stands for, as long as A and B agree.  Choosing, for the 32-feature K block kb2,
//          feature(g, i) = 16 (2 kb2 + (i >> 2)) + 4 g + (i & 3),      i = 0..7
// makes the accumulator layout of one layer exactly the B-operand layout of the next: activations never leave
// registers between layers -- no LDS round trip, no HBM traffic.  LayerNorm over a row is 32 in-lane values + two
// cross-group exchanges.
//
// Arithmetic: fp32 results from v_mfma_f32_16x16x32_f16 by TWO-WAY fp16 splitting with power-of-two scaling.
// A value is written as  x * 2^k = h + l,  h = fp16(x 2^k), l = fp16(x 2^k - h)  (round to nearest: 11 + 11 significand
// bits, sign included in each piece); k is chosen per ROW of the activation tile (row maximum -> [2^12, 2^13), so h never
// overflows and l stays a normal fp16 for every element within 2^15 of the row maximum) and per weight MATRIX.  A product
// is accumulated in fp32 as the three partial products
//          h_w * l_x  +  h_w * h_x  +  l_w * h_x;
// the dropped l_w * l_x is <= 2^-22 |x w|, and the result is un-scaled by the exact power of two 2^-(k_x + k_w).
// Measured against an fp64 product (profiles/census/f16split.hip, profiles/r03_f16split.md) this is MORE accurate than
// the exact three-way bf16 split of rounds 1-2 (six products, truncated pieces), than v_mfma_f32_16x16x4_f32 and than a
// sequential fp32 dot product, for activations, gradients of magnitude 1e-7, rows mixing 1e4 / 1 / 1e-6 and rows of 1e-30
// or 1e30 alike -- at half the matrix instructions (3 instead of 6 per fragment pair), 2/3 of the weight bytes and 4
// instead of 9-11 VALU operations per pair of elements (v_fma_mix{lo,hi}_f16 folds scaling, subtraction and rounding).
// Inputs, outputs, accumulation, bias, LayerNorm and everything stored to HBM stay fp32.
//
// Weights are re-laid out once per call ("prepack") into chunks, one per 32-feature K block:
//          [1 KB header]  [t][plane h|l][lane] 16 bytes = the 8 fp16 of A-fragment (t, kb2) for that lane
// (17 KB per chunk at D = 128).  Header of chunk 0: float 255 = 2^-k_w (the un-scaling factor of the matrix); header of
// the LAST chunk: the Linear's bias (needed when the stage finishes).  A LOADER wave streams chunks L2 -> LDS with
// LDS-DMA (global_load_lds_dwordx4, no registers, two chunks in flight) through a 3-deep ring, one workgroup barrier per
// chunk; compute waves read their A fragments with conflict-free lane-linear ds_read_b128.
// (The bf16 PRECISION of the edge MLP -- bsms_precision -- keeps one bf16 plane per weight and its bias in chunk 0.)
#pragma once
#include <type_traits>

#include "../../include/bsms_hip_query.h"
#include "common.h"

namespace bsms {

constexpr int kMaxStages = 8;   // max Linear layers per MLP handled by one chain launch
constexpr int kComputeWaves = 4;                       // compute waves per workgroup (each owns 16 rows)
constexpr int kTileRows = kComputeWaves * 16;          // rows of x per workgroup
constexpr int kChainThreads = (kComputeWaves + 1) * 64;  // + 1 loader wave
constexpr int kChainMaxThreads = 8 * 64;               // generic chain kernels: up to 7 compute waves (launcher's choice)
constexpr int kChunkHdrFloats = 256;                     // 1 KB chunk header (bias)
// Precision of the EDGE-level tensors of a GMP block (include/bsms_hip.h: bsms_precision).  BF16: the saved edge
// activations, the messages y and the edge layer gradients are stored as bf16 and the edge MLP's products take bf16
// operands (weights rounded once per call) with fp32 accumulation; everything at node level stays fp32.
// A saved activation [rows, D] is followed by its ReLU sign bits, one bit per element packed per (row, lane group):
// the backward chain masks gradients from 16 bytes per row instead of re-reading 4 D bytes.  Each of the 4 lane groups
// of a row holds D / 4 elements, i.e. ceil(D / 128) words of bits (chain_dev.h: mask_words).
constexpr size_t mask_words_per_row(int64_t D) { return size_t(4) * size_t((D + 127) / 128); }
// Tensors the chain kernels write with their paired streaming stores are allocated for whole tiles (the largest tile:
// kPadRows rows, the edge kernels with two row blocks per wave): the stores then need no per-lane bounds test (rows
// past R hold garbage nobody reads; the sign bits start after the padding and are padded the same way).
constexpr int kPadRows = 2 * kTileRows;
constexpr size_t pad_rows(size_t rows) { return (rows + kPadRows - 1) / kPadRows * kPadRows + 2 * kPadRows; }   // + 256 rows: covers the last tile of any tile size up to 7 waves x 32 rows
constexpr size_t act_floats(size_t rows, int64_t D) { return pad_rows(rows) * (size_t(D) + mask_words_per_row(D)); }
// row pitch (floats) of the saved fiber tensor: p + 1 values padded to one or two 16-byte pieces
constexpr int fiber_ld(int64_t p) { return p + 1 <= 4 ? 4 : 8; }
constexpr int kScaleSlot = 255;                          // header float of chunk 0 that holds 2^-k_w
// floats in one weight pack of a D x D Linear (fp16 x 2 planes + headers)
constexpr size_t pack_floats(int64_t D) { return size_t(D / 32) * (kChunkHdrFloats + size_t(D / 16) * 512); }

enum ChainIn { IN_ROWS = 0, IN_ROWS2 = 1, IN_SMALL = 2, IN_EDGE = 3 };
enum ChainOut { OUT_LN = 0, OUT_PLAIN = 1, OUT_SMALL = 2, OUT_PLAIN2 = 3 };  // PLAIN2: stage 0 -> y, stage 1 -> y2, same input
enum GradIn { G_ROWS_LN = 0, G_EDGE_LN = 1, G_SMALL = 2 };
enum GradFirst { F_NONE = 0, F_HEADS1 = 1, F_HEADS2 = 2 };

struct ChainFwdArgs {
  int64_t R;  // rows
  int ntiles; // filled by the launcher: ceil(R / (16 RB cw)), the tiles of this launch's cw compute waves x RB row blocks (ChainLaunch); workgroups stride over tiles (persistent)
  // ---- input stage
  const float* x;    // IN_ROWS/IN_ROWS2: [R,D]; IN_SMALL: [R,K0]
  const float* x2;   // IN_ROWS2: second source [R,D]
  int K0;            // IN_SMALL: input width; IN_EDGE: p+1
  const float* w0t;  // IN_SMALL: W0^T [K0][D]; IN_EDGE: fiber weights^T [p+1][D]
  const float* bias_in;  // IN_SMALL: b0 [D]
  float* store_in;   // IN_SMALL/IN_EDGE: activation after the input stage, act_floats(R, D) floats (nullable)
  const int32_t *src, *dst;  // IN_EDGE: plan-order endpoints
  int32_t E, N;
  const float *Ps, *Pd;      // IN_EDGE: per-node pre-projections [B*N, D]
  const float* pos;          // IN_EDGE
  int64_t pos_bstride;
  int p;
  float* fiber_out;          // IN_EDGE: [R, fiber_ld(p)] the fiber [pos_i - pos_j, |pos_i - pos_j|, 0...] of every edge row, kept
                             // for the backward's narrow weight gradient (nullable)
  // ---- MFMA stages
  int nstage;
  const float4* wp[kMaxStages];  // packs (the Linear's bias travels in the pack header, see PackDesc)
  const float4* wp0b;  // IN_ROWS2: pack for x2 in stage 0 (same scale as wp[0]: PackDesc::mate; the stage's bias rides in THIS pack)
  float* store[kMaxStages];  // post-ReLU activation of stage l, act_floats(R, D) floats: values + sign bits (nullable)
  // ---- output
  float* y;           // OUT_LN / OUT_PLAIN: [R,D]; OUT_SMALL: [R,C]
  float* y2;          // OUT_PLAIN2: second head [R,D]
  float* yln;         // OUT_LN: normalised output before the residual (nullable)
  float* rstd;        // OUT_LN: [R] (nullable)
  const float* resid; // OUT_LN: residual rows added to y (nullable)
  const float* resid2; // OUT_LN: second residual (the U-Net skip connection, ops/BSMS.py:102), added after `resid` (nullable)
  int accumulate;     // OUT_PLAIN: y += result
  const float* wout;  // OUT_SMALL: [C][D]
  const float* bout;  // OUT_SMALL: [C]
  int C;
  unsigned long long* timing;  // experiments only: per-workgroup s_memtime stamps (16 slots), null in production
  int bf16;           // bf16 precision (IN_EDGE / OUT_LN only): bf16 MFMA operands, saved activations and y stored as bf16
  int store_mode;     // saved-activation stores: 0 plain, 1 non-temporal (keeps L2 for weights / gathered rows)
  int out_mode;       // same for the final output y
  // ---- filled by launch_chain_fwd: weight packs in execution order for the loader wave(s)
  int nseq;
  const float4* wseq[kMaxStages + 2];
  int nload;          // loader waves per workgroup (the last `nload` waves of the block)
  int nring;          // depth of the LDS weight ring of this launch (3..6)
  // ---- magnitude bounds for the weight-gradient kernel (wgrad.hip): bound slots (kBoundWidth floats each, see above)
  // for the tensor ENTERING stage l -- amax[0]: x / [x, x2] / the activation of the narrow or edge input stage;
  // amax[l + 1]: the post-ReLU activation of stage l.  Nullable.
  float* amax[kMaxStages + 1];
};

struct ChainBwdArgs {
  int64_t R;
  int ntiles;         // filled by the launcher (persistent workgroups stride over tiles)
  const float* dy;    // G_ROWS_LN: [R,D]; G_EDGE_LN: [B*N,D] node gradient gathered by dst; G_SMALL: [R,C]
  const float* yln;   // LN cases: normalised forward output [R,D]
  const float* rstd;  // LN cases: [R]
  const int32_t* dst; // G_EDGE_LN
  int32_t E, N;
  const float* wout;  // G_SMALL: [C][D]
  int C;
  const float* mask_in;  // G_SMALL: activation masking the VALU-produced gradient
  int nstage;
  const float4* wpt[kMaxStages];  // transposed packs, execution order (top layer first)
  const float* mask[kMaxStages];  // saved activation (act_floats layout) whose sign BITS mask the output of stage k
  float* gstore[kMaxStages + 1];  // [0]: gradient entering stage 0; [k+1]: output of stage k (nullable)
  // ---- first-layer input gradient
  const float4 *wh0, *wh1;
  float *dx, *dx2;
  const float* dres;  // added to dx (residual branch), nullable
  int store_mode;     // layer-gradient stores: 0 plain, 1 non-temporal
  int bf16;           // bf16 precision (G_EDGE_LN / F_NONE only): yln is bf16, layer gradients are stored as bf16
  // ---- filled by launch_chain_bwd: weight packs in execution order for the loader wave(s)
  int nseq;
  const float4* wseq[kMaxStages + 2];
  int nload;          // loader waves per workgroup (the last `nload` waves of the block)
  int nring;          // depth of the LDS weight ring of this launch (3..6)
  float* gmax[kMaxStages + 1];   // like ChainFwdArgs::amax for gstore[k] (the gradient entering stage k; [nstage]: the last one). Nullable.
  int ablate;         // experiment builds only (k_edge_bwd): every tile stores its layer gradients gstore[0..nstage-1] to tile 0 (no HBM stream)
};

// prepack table ---------------------------------------------------------------------------------
enum PackKind { PACK_FRAG = 0, PACK_FRAG_T = 1, PACK_TRANSPOSE = 2, PACK_ROWS_BF16 = 3 };
struct PackDesc {
  const float* W;  // row-major, leading dimension ld
  const float* bias;  // FRAG kinds: [N] copied into the header of the last chunk (bf16: of chunk 0); nullable -> zeros
  float* dst;      // FRAG kinds: pack_floats(N) floats
  int ld, row0, col0;
  int N, K;  // logical matrix M[n][k], n < N (outputs), k < K (reduction)
  int kind;  // FRAG: M[n][k] = W[row0+n][col0+k]; FRAG_T: M[n][k] = W[row0+k][col0+n];   (N == K, multiple of 32)
             // TRANSPOSE: dst[k*N+n] = W[row0+n][col0+k] (plain, for the small VALU layers)
             // ROWS_BF16 (N = K = 128): the LDS image of efuse.hip -- row n at byte 288 n, its 8-byte piece `q` (bf16 of
             //   M[n][4 q .. 4 q + 3], M as FRAG) at piece slot q ^ ((n >> 2) & 3); 36 KB, copied into LDS by LDS-DMA
  int bf16;  // FRAG kinds: ONE plane = the weight rounded to bf16 (bf16 precision)
  int mate;  // FRAG kinds, fp32 path: 1 + index of a pack of the same table that must share this pack's scale 2^k_w (the two
             // halves of a Linear over concatenated inputs accumulate into one set of registers); 0 = none
};
constexpr int kMaxPack = 40;
// Magnitude bounds of the tensors the weight-gradient kernel multiplies (ChainFwdArgs::amax, ChainBwdArgs::gmax,
// WgradJob::g_bound).  A bound "slot" is an array of kBoundWidth floats: every compute wave of a chain launch writes the
// largest |value| it saw into its own entry (blockIdx * 8 + wave; plain stores, no atomics: same-address atomics from
// ~10^5 waves cost milliseconds), the consumer takes the maximum over the whole array (unused entries are zero: the
// prepack of the forward call clears all slots of a block).
constexpr int kBoundWidth = 8192;  // 8 x the largest persistent chain grid (4 workgroups per CU at D <= 64, 256 CUs); beyond that: atomic max on the last entry
constexpr int kBoundSlots = 32;    // slots of one GMP block / MLP
struct PackTable {
  int n;
  PackDesc d[kMaxPack];
  float* zero;   // nullable: kBoundSlots x kBoundWidth floats the prepack sets to zero
};
int launch_prepack(const PackTable& t, hipStream_t s);

// Pack group (bsms_pack_group_*): the pack tables of every MLP / GMP block of a training step, concatenated, in ONE launch.
// The descriptors (13 tables x 21 at the airfoil step: too many for a kernarg) and the list of bound-slot arrays to clear live in
// device memory, uploaded by the first launch; from then on the group is sealed (a caller whose pointers, shapes or precision
// change builds a new group).  Every pack comes out byte for byte as launch_prepack writes it: the two kernels share their body.
struct PackGroup {
  std::vector<PackDesc> descs;   // `mate` re-based to this list
  std::vector<float*> zeros;     // kBoundSlots x kBoundWidth floats each
  int biggest = 0;               // largest N * K of a member (the launch shape)
  void* dev = nullptr;           // device image: the descriptors, then the pointer list; null until the first launch
  int device = -1;               // where `dev` lives
};
void pack_group_append(PackGroup& g, const PackTable& t);
int launch_prepack_group(PackGroup& g, hipStream_t s);
// the group behind an ABI handle, refused (BSMS_E_INVALID_ARG) when null or sealed
int pack_group_open(bsms_pack_group_t* group, const char* who, PackGroup** g);

int launch_chain_fwd(int D, int in_mode, int out_mode, const ChainFwdArgs& a, hipStream_t s);
int launch_chain_bwd(int D, int gin_mode, int first_mode, const ChainBwdArgs& a, hipStream_t s);
// The choice of a chain launch as data (chain_launch.h: plan_fwd / plan_bwd decide, the launch path and bsms_chain_launch_query read).
// The key: what the choice reads from ChainFwdArgs / ChainBwdArgs, and nothing else (bsms_hip_query.h spells out the fields).
using ChainLaunchKey = ::bsms_chain_launch_key;
enum ChainStores { CHAIN_STORES_NONE = 0, CHAIN_STORES_ALL = 1, CHAIN_STORES_MIXED = 2 };   // a set of nullable store pointers
enum ChainFamily { CHAIN_FS = 0, CHAIN_EDGE = 1, CHAIN_RING = 2, CHAIN_UNBUILT = 3 };   // k_fs_* / k_edge_* / k_chain_*; UNBUILT: refused, never launched
struct ChainLaunch {
  int family;                    // ChainFamily
  int rb;                        // EDGE: row blocks per wave (1 / 2)
  bool save, store;              // EDGE: the SAVE build of the forward / the STORE build of the backward
  bool lone, bf16, timing;       // EDGE / RING: the single-round build; RING: the bf16 and the TIMING builds
  int cw, nload, nring, ntiles;  // compute waves, loader waves, ring slots, tiles of 16 rb cw rows
  unsigned grid, threads;
  size_t lds, lds_max;           // dynamic LDS of this launch and the most any launch of the kernel asks for (launch_dyn_lds)
  const char *what, *build;      // launcher and variant in the error text (launch_dyn_lds)
};
// the chain kernels of one width, NB = D / 16 = 2, 4, ... 16: defined in chain_launch.h, instantiated by one translation unit each (chain_d*.hip)
template <int NB>
int launch_chain_fwd_nb(int in_mode, int out_mode, const ChainFwdArgs& a, hipStream_t s);
template <int NB>
int launch_chain_bwd_nb(int gin_mode, int first_mode, const ChainBwdArgs& a, hipStream_t s);
template <int NB>
int chain_launch_query_nb(int backward, int mode_a, int mode_b, const ChainLaunchKey& k, int cus, ChainLaunch* out);
// the dispatch on the latent width: f(NB as an integral constant), one translation unit per width (chain_d32.hip ... chain_d256.hip)
template <class F>
int with_width(int D, F&& f) {
  switch (D) {
    case 32: return f(std::integral_constant<int, 2>{});
    case 64: return f(std::integral_constant<int, 4>{});
    case 96: return f(std::integral_constant<int, 6>{});
    case 128: return f(std::integral_constant<int, 8>{});
    case 160: return f(std::integral_constant<int, 10>{});
    case 192: return f(std::integral_constant<int, 12>{});
    case 224: return f(std::integral_constant<int, 14>{});
    case 256: return f(std::integral_constant<int, 16>{});
  }
  BSMS_FAIL(BSMS_E_UNSUPPORTED, "latent width D=%d not supported (a multiple of 32, 32..256)", D);
}

// weight gradients ------------------------------------------------------------------------------
struct WgradJob {
  const float* G;  // [R, ldg] gradient w.r.t. the Linear's output
  const float* A;  // [R, lda] the Linear's input
  float* dW;       // dW[n*ldw + col0 + k] = sum_r G[r][n] * A[r][k]   (n,k < D)
  float* db;       // db[n] = sum_r G[r][n]   (nullable)
  int64_t R;
  int ldg, lda, ldw, col0;
  int bf16;        // G and A are bf16 tensors (ld in elements): one bf16 product instead of the split products
  // Magnitude bounds of the two operands (bound slots written by the chain kernels, ChainFwdArgs::amax / ChainBwdArgs::gmax;
  // bound = max(slot[0 .. kBoundWidth)) * mul >= max |value|).  Both given: the products run as fp16 x 2 pieces with per-TENSOR power-of-two
  // scales (chain.h; the reduction index is the row, so a scale cannot vary by row) -- three MFMAs per fragment pair.
  // Either missing: the exact three-way bf16 split of rounds 1-2 (six MFMAs), which needs no range information.
  const float *g_bound, *a_bound;
  float g_mul, a_mul;
};
constexpr int kMaxWgradJobs = 20;
size_t wgrad_work_bytes(int D, int njobs);
// `skip_mask` (bit j = job j): jobs of a frozen MLP -- not run, but counted when the launch shape is chosen, so that the jobs that remain are
// partitioned (and rounded) exactly as in the launch with nothing frozen; a launch whose jobs are all skipped is not issued
int launch_wgrad(int D, const WgradJob* jobs, int njobs, void* work, hipStream_t s, unsigned skip_mask);
static_assert(kMaxWgradJobs <= 32, "launch_wgrad: one bit per job");

// The depth envelope, hidden = 1 .. kMaxStages - 1 (GmpShape::check, check_mlp), against every fixed-size table that grows with it
// (DESIGN.md 4.28).  The counts are those of the code that fills the tables: gmp.hip block_pack_table / GmpBwd::lane0_wgrads,
// mlp.hip mlp_pack_table / bsms_mlp_bwd_ex, chain_launch.h (the loader sequences).
constexpr int kMaxHidden = kMaxStages - 1;
constexpr int gmp_block_packs(int H) { return 9 + 4 * H; }       // a training block: 5 of the first edge Linear, 4 of the first node Linear, 2 per D x D Linear of either MLP
constexpr int mlp_packs(int H) { return 1 + 2 * (H + 1); }       // a training MLP: the narrow transpose, 2 per Linear
constexpr int gmp_block_wgrad_jobs(int H) { return 2 * H + 2; }  // lane 0: H edge Linears, H node Linears, the two halves of the first node Linear
static_assert(gmp_block_packs(kMaxHidden) <= kMaxPack && mlp_packs(kMaxHidden) <= kMaxPack, "PackTable::d holds the packs of the deepest block");
static_assert(gmp_block_wgrad_jobs(kMaxHidden) <= kMaxWgradJobs && kMaxHidden + 1 <= kMaxWgradJobs, "one wgrad launch holds the jobs of the deepest block");
static_assert(kBoundSlots == 4 * 8 && kMaxHidden + 1 <= 8, "bound slots: four groups of 8, hidden + 1 entries used in each ([16 + H], [24 + H] are the last)");
static_assert(kMaxHidden + 2 <= kMaxStages + 2, "wseq: the node chains stream hidden + 2 packs (IN_ROWS2 forward, F_HEADS2 backward)");

// small-side weight gradients: out[s*os + f*of] = sum_r G[r][f] * S[r][s],  s < S (<= 8)
struct SmallWgradArgs {
  const float* G;  // [R,D]
  const float* S;  // [R,S_ld] narrow matrix, S_cols <= S_ld columns used (null when fiber mode)
  int S_cols;
  int S_ld;        // row pitch of S (0 = S_cols)
  // fiber mode: S[r] = [pos_i - pos_j, |pos_i - pos_j|] recomputed from the plan (edge layer 0)
  const int32_t *src, *dst;
  int32_t E, N;
  const float* pos;
  int64_t pos_bstride;
  int p;
  float* out;  // element (s,f) at out[s*os + f*of]
  int64_t os, of;
  float* colsum;  // optional: colsum[f] = sum_r G[r][f]
  float* colsum_S;  // optional: colsum_S[s] = sum_r S[r][s]  (decoder output bias)
  int64_t R;
  int D;
};
size_t small_wgrad_work_bytes(int D);
size_t small_wgrad_work_bytes_rows(int D, int64_t workers);   // sized for the fused pair kernel: one block per 256 / (D/4) row workers
int launch_small_wgrad(const SmallWgradArgs& a, void* work, hipStream_t s);

// efuse.hip: the fused backward of the edge MLP in the bf16 precisions (D = 128, hidden = 3): forward recompute + LayerNorm
// backward + dgrad chain + the weight / bias gradients of Linears 1..3 accumulated on chip; g_0 leaves as bf16
struct EdgeFusedBwdArgs {
  int64_t R;                  // B * E edge rows (plan order)
  int32_t E, N;
  const int32_t *src, *dst;   // plan-order endpoints
  const float *Ps, *Pd;       // the forward's node projections [B*N, D] (kept in the saved blob in this mode)
  const float* fiber;         // [R, 4]: the fiber rows the forward kept
  const float* wft;           // fiber weights^T [p+1][D]
  int p;
  const float4* wr[3];        // PACK_ROWS_BF16 images of edge Linears 1..3 (the rounding of the forward's packs)
  const float* b[3];          // their biases (fp32 parameters)
  const float* dy;            // [B*N, D] gradient of the aggregate (gathered by target)
  const void* y;              // [R, D] bf16 messages
  const float* rstd;          // [R]
  void* g0;                   // [pad_rows(R), D] bf16: gradient w.r.t. the first edge Linear's output
  float* gmax;                // bound slot of g0 (kBoundWidth floats), nullable
  float* part;                // per-workgroup partials, edge_fused_part_floats() floats
  int ntiles;                 // filled by the launcher
  unsigned long long* timing; // experiments only: phase stamps (null in production)
};
constexpr int kEdgeFusedMaxWg = 256;
bool edge_fused_supported(int64_t D, int H, int64_t p, int precision);
size_t edge_fused_part_floats(int64_t rows);   // for a launch over `rows` edge rows: one partial per workgroup, at most kEdgeFusedMaxWg
int launch_edge_fused_bwd(EdgeFusedBwdArgs a, int* nwg_out, hipStream_t s);
// the data-only form for a frozen edge MLP: the same g0, bit for bit; `part`, `gmax` and `timing` are not used
int launch_edge_data_bwd(EdgeFusedBwdArgs a, hipStream_t s);
int launch_edge_fused_reduce(const float* part, int nwg, float* const dW[3], float* const db[3], hipStream_t s);

// efwd.hip: the edge MLP forward of the bf16 precisions with the three D x D weights resident in LDS (D = 128, hidden = 3):
// 16 independent waves per workgroup, no weight ring, no barriers; bit-identical to k_chain_fwd<8, IN_EDGE, OUT_LN, BF>
struct EdgeFwdResArgs {
  int64_t R;                  // B * E edge rows (plan order)
  int32_t E, N;
  const int32_t *src, *dst;   // plan-order endpoints
  const float *Ps, *Pd;       // node projections [B*N, D]
  const float* pos;           // [B, N, p] (batch stride pos_bstride; 0 = one point set for every sample)
  int64_t pos_bstride;
  int p;
  const float* wft;           // fiber weights^T [p+1][D]
  const float4* wp[3];        // the one-plane bf16 packs of edge Linears 1..3 (PackDesc::bf16; bias in the header of chunk 0)
  void* y;                    // [R, D] bf16 messages
  float* rstd;                // [R] (nullable: inference)
  float* fiber_out;           // [R, 4] (nullable: inference)
  int ntiles;                 // filled by the launcher
};
bool edge_fwd_res_supported(int64_t D, int H, int64_t p, int precision);
int launch_edge_fwd_res(EdgeFwdResArgs a, hipStream_t s);

// from rowsum.hip
int rowsum_plan_order(const bsms_plan* p, const float* x, int64_t B, int64_t D, float* out, hipStream_t s);
int rowsum_by_source(const bsms_plan* p, const float* x, int64_t B, int64_t D, float* out, hipStream_t s);
int rowsum_source_and_target(const bsms_plan* p, const float* x, int64_t B, int64_t D, float* outS, float* outD, hipStream_t s,
                             bool x_bf16 = false);
int rowsum_source_target_fiber(const bsms_plan* p, const float* x, int64_t B, int64_t D, float* outS, float* outD,
                               const float* fiber, int ld, int ncols, float* part, int64_t part_blocks, int* nwg, hipStream_t s,
                               bool x_bf16);
int rowsum_plan_order_bf16(const bsms_plan* p, const float* x_bf16, int64_t B, int64_t D, float* out, hipStream_t s);
// wgrad.hip: partial blocks of the narrow weight gradients ([blocks][10][D] floats) and their fixed-order reduction
int64_t small_wgrad_part_blocks(size_t work_bytes, int D);
int launch_small_reduce(const SmallWgradArgs& a, const void* work, int nwg, hipStream_t s);

}  // namespace bsms
