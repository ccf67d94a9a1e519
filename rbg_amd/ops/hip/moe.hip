// Mixture-of-experts FFN for decode- and prefill-sized batches (gfx950):
// fused top-k router + expert grouping, grouped gate_up GEMM with a SwiGLU
// epilogue, grouped down GEMM, weighted combine.  docs/FEATURES.md "Mixture
// of experts" has the contract; the rounding points are
//   g, u = x[t] w1[e]^T   f32, never rounded
//   h    = bf16(silu(g) * u)
//   o    = h w2[e]^T      f32
//   y[t] = bf16(sum_j w[t, j] * o[t, j])   f32 mul, f32 add, slot order
//
// Why hand-written: with top-8 of 128 experts a decode batch of 128 is 1024
// (token, expert) rows, about 8 per expert: 128 GEMMs of M ~ 8 per projection.
// That is the weight stream with a short M of skinny_gemm.hip, once per
// expert, plus a gather in front and a scatter behind.  Every grid depends on
// (T, k, E, H, I) only and nothing is read back, so a layer is capturable.
//
//   1 moe_route_kernel   one wave per token: wave max + sum over E <= 256
//                        (4 logits per lane), k rounds of wave argmax on
//                        (order-preserving key, ~index) pairs.  The LAST
//                        workgroup to finish (one integer ticket, which it
//                        puts back to zero) then groups the T*k pair indices
//                        p = t*k + j by expert: a stable counting sort in one
//                        workgroup, see group_pairs().
//   2 moe_gemm_kernel<1> grid E x I/32: expert e, 32 gate rows + the matching
//                        32 up rows of w1[e] = a 64-row W stage.  A rows are
//                        gathered: tile row r is x[sorted[off + r] / k].
//                        Epilogue pairs the gate and up accumulators of a
//                        wave in registers and stores bf16 h in SORTED order.
//   3 moe_gemm_kernel<0> grid E x H/64: A = h[off : off + n] (contiguous),
//                        W = 64 rows of w2[e], K = I; f32 rows to opart[p].
//   4 moe_combine_kernel y[t] = bf16(sum_j w[t, j] * opart[t*k + j]).
//
// GEMM workgroup (both 2 and 3): 4 waves = 2 k-slices (32 k of each 64-k
// step) x 2 tile pairs; a wave owns W tiles t and t + 2 of the 64-row stage
// (gate tile t and up tile t in kernel 2) and MT row tiles of A, so a W
// fragment feeds MT MFMAs and an A fragment two.  v_mfma_f32_16x16x32_bf16
// with W as the first operand: a lane then holds 4 CONSECUTIVE output columns
// of one token row, so h is stored 8 bytes and opart 16 bytes per lane.
// Staging is skinny_gemm.hip's: 16-byte pieces, 8 lanes per 128-byte row
// segment, double-buffered LDS, two NAMED register load sets issued 2-3 steps
// ahead, one barrier per step (that file's header has what was measured, and
// how arrays of such registers ended in scratch memory).  The step count may
// be odd (K = I = 192 is 3 steps), so the two-step loop can leave in the
// middle.
//
// Row tiles per pass are compile-time: an expert with n <= 16 rows (the
// decode case) runs MT = 1 and stages 2 KB of A per 8 KB of W; more rows run
// MT = 4, and an expert with more than 64 makes further passes over its
// panel, L2-resident by then.  Which MT or pass serves a row changes nothing:
// every output element is the same two MFMA chains (k offsets [0, 32) and
// [32, 64) of each step, in step order) added in f32, whatever rows share its
// tile.  Rows past the expert's count are clamped to a live row on the way
// in and never stored.
//
// e4m3 experts (docs/FEATURES.md "FP8 experts"): w1 / w2 as e4m3 bytes with
// one int8 exponent per expert output row, dq = e4m3 * 2^e.  Kernels 2 and 3
// have a second instantiation (WT = uint8_t) that differs in how W travels:
//   stage = 128 k, two 64-k steps per barrier.  W's 64 rows x 128 B are two
//           16-byte pieces per thread, 8 lanes per 128-byte row segment (the
//           bf16 request shape at half the rows' bytes); A's 16 MT rows x
//           256 B are MT pieces per thread, 16 lanes per row.
//   LDS   = W stays BYTES: a lane's fragment is one 8-byte read and four
//           v_cvt_scalef32_pk_bf16_fp8 at scale 1 (exact).  Each W fragment
//           is read by one lane per pass, so nothing is converted twice and
//           W's LDS write traffic halves.  Row pitch 144 B (36 banks: the 16
//           rows of a tile start 4 banks apart in a permutation of 0 .. 60
//           and the two 8-byte reads of a row pair fill the 4: conflict-free;
//           the 16-byte writes see what the bf16 stage's 144 B pitch sees).
//           A rows are 128 + 8 bf16.  Two buffers = a ring four 64-k steps
//           deep, 53 248 B at MT = 4 (three workgroups per CU).
//   tail  = an odd step count (K = 192) ends in half a stage: the pieces
//           past K are re-reads of the row's last piece (never past the
//           tensor) and the second 64-k step is skipped.
//   chain = unchanged: k-slice s takes [32 s, 32 s + 32) of step 2 j, then
//           of step 2 j + 1, so every output is the two chains above on
//           e4m3 -> bf16 values, and 2^e[row] multiplies the folded f32 sum
//           (before SiLU for gate and up, each with its own exponent).  That
//           is the bf16 kernel's result on dq bit for bit: a power of two
//           commutes with every rounding on the way.
//
// MXFP4 experts (docs/FEATURES.md "MXFP4 experts"): w1 / w2 as e2m1 codes,
// two per byte (element 2i in the low nibble), with one int8 exponent per 32
// consecutive k of a row, dq = e2m1 * 2^e.  The third instantiation
// (WT = mxfp4_t) again differs in how W travels only:
//   stage = 128 k as above, and A's staging is the e4m3 pass's.  W's 64 rows
//           x 64 B of codes are ONE 16-byte piece per thread (row tid >> 2,
//           piece tid & 3), which is exactly one 32-k scale block: the thread
//           loads that block's exponent byte with it (the exponents of a row
//           are K/32 bytes, 2-byte aligned at K = 192: byte loads only).
//   LDS   = W stays CODES.  Row pitch 80 B = 64 B of codes, the stage's four
//           exponent bytes of the row, pad.  80 B is 20 banks: the 16 rows
//           of a tile start on 16 distinct multiples of 4 banks and the four
//           4-byte reads of a row's k-groups fill the gaps, so the fragment
//           reads are conflict-free and the 16-byte writes stay aligned.
//           Two buffers are 45 056 B at MT = 4 (three workgroups per CU).
//   frag  = a lane's 8 consecutive k are one 4-byte read and four
//           v_cvt_scalef32_pk_bf16_fp4 (byte select 0 .. 3) whose scale
//           operand is the f32 2^e of the lane's (row, block), one byte read:
//           the bf16x8 of dq, exact.  The MFMA consumes 32 k per W row, one
//           scale block, so nothing is left for the epilogue to scale.
//   tail  = as above: blocks past K are re-reads of the row's last block
//           with that block's exponent, and the second 64-k step is skipped.
//   chain = unchanged, so the result is the bf16 kernel's on dq bit for bit.
//
// No atomics on floats anywhere; the one atomic is the integer ticket (and
// integer LDS counters inside the sort, whose totals do not depend on order).
// All global writes are plain vector stores.
//
// No packed-fp32 VALU in this file's device code, and the runtime headers
// inside the region: attn_prefill_paged.hip has the reasons.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                               \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#include <type_traits>

#include "skinny_gemm_tile.h"   // lds_frag
#include "launch.h"

namespace {

typedef unsigned long long u64;

// ---------------------------------------------------------------------------
// 1. route + group

constexpr int MR_NT = 1024;                  // 16 waves: 16 tokens / workgroup
constexpr int MR_WAVES = MR_NT / 64;
constexpr int MR_EMAX = 256;

// exp(z) for z <= 0 to about an ulp: v_exp_f32 of z * log2(e) with the
// product's rounding error (up to 2^-19 at z = -32) put back to first order.
DEV_INLINE float exp_neg(float z) {
  if (!(z > -100.f)) return 0.f;             // -inf (and NaN) contribute 0
  const float l2e = 1.44269502162933349609375f;
  const float l2e_lo = 1.925963033500011e-8f;
  const float t = z * l2e;
  const float lo = __fmaf_rn(z, l2e, -t) + z * l2e_lo;
  const float e = __builtin_amdgcn_exp2f(t);
  return __fmaf_rn(e, lo * 0.693147182464599609375f, e);
}

// order-preserving float -> uint32 (no NaN reaches it; -0 was made +0)
DEV_INLINE unsigned fkey(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

DEV_INLINE u64 wave_max_u64(u64 x) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const u64 y = __shfl_xor(x, off, 64);
    x = y > x ? y : x;
  }
  return x;
}

// One token on one wave.  Lane l holds experts l, l + 64, l + 128, l + 192.
DEV_INLINE void route_token(const __hip_bfloat16* __restrict__ lg, const int E,
                            const int k, const bool renorm, int* ids_out,
                            float* w_out, const int lane) {
  float v[4];
  u64 key[4];
  float m = -INFINITY;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int e = lane + 64 * c;
    float x = -INFINITY;
    if (e < E) x = bf2f(lg[e]);
    if (x != x) x = -INFINITY;               // NaN compares as -inf
    if (x == 0.f) x = 0.f;                   // -0 ties with +0
    v[c] = x;
    key[c] = e < E ? ((u64)fkey(x) << 32) | (unsigned)~(unsigned)e : 0ull;
    m = fmaxf(m, x);
  }
  m = wave_max(m);
  float p[4];
  float s = 0.f;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    p[c] = lane + 64 * c < E ? exp_neg(v[c] - m) : 0.f;
    s += p[c];
  }
  s = wave_sum(s);

  int my_id = 0;
  float my_p = 0.f;
  for (int j = 0; j < k; ++j) {
    u64 best = key[0];
#pragma unroll
    for (int c = 1; c < 4; ++c) best = key[c] > best ? key[c] : best;
    best = wave_max_u64(best);
    const int e_win = (int)~(unsigned)(best & 0xffffffffull);
    float pw = 0.f;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if ((e_win >> 6) == c) pw = p[c];      // uniform c, no dynamic index
      if (lane + 64 * c == e_win) key[c] = 0ull;
    }
    pw = __shfl(pw, e_win & 63, 64);
    if (lane == j) {
      my_id = e_win;
      my_p = pw;
    }
  }
  float wj = my_p / s;
  if (renorm) {
    float tot = 0.f;
    for (int j = 0; j < k; ++j) tot += __shfl(wj, j, 64);   // slot order
    wj = wj / tot;
  }
  if (lane < k) {
    ids_out[lane] = my_id;
    w_out[lane] = wj;
  }
}

// Stable counting sort of the pair indices 0 .. n-1 by ids[p], one workgroup
// of MR_NT threads.  Wave w owns the contiguous range [w * per, (w + 1) * per)
// and walks it in order, 64 pairs at a time: (1) per-wave histograms, (2)
// hist[w][e] becomes the pairs of e in earlier waves and base[e] the pairs of
// earlier experts, (3) each lane's slot is base + hist + its rank among the
// lanes of this step with the same expert (8 ballots), after which the last
// such lane advances hist.  Nothing depends on timing.  An id outside [0, E)
// is skipped (ops.moe_ffn has refused it on the host).
DEV_INLINE void group_pairs(const int* ids, const int n, const int E,
                            int* __restrict__ offsets, int* __restrict__ sorted,
                            int* hist, int* base) {
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int i = tid; i < MR_WAVES * MR_EMAX; i += MR_NT) hist[i] = 0;
  __syncthreads();
  const int per = ((n + MR_WAVES * 64 - 1) / (MR_WAVES * 64)) * 64;
  const int lo = min(n, wave * per), hi = min(n, lo + per);
  for (int i = lo + lane; i < hi; i += 64) {
    const int e = ids[i];
    if ((unsigned)e < (unsigned)E) atomicAdd(&hist[wave * MR_EMAX + e], 1);
  }
  __syncthreads();
  if (tid < MR_EMAX) {
    int run = 0;
    for (int w = 0; w < MR_WAVES; ++w) {
      const int c = hist[w * MR_EMAX + tid];
      hist[w * MR_EMAX + tid] = run;
      run += c;
    }
    base[tid] = run;
  }
  __syncthreads();
  if (wave == 0) {                           // exclusive scan of 256 totals
    int a[4], sum = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      a[i] = base[4 * lane + i];
      sum += a[i];
    }
    int incl = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const int t = __shfl_up(incl, off, 64);
      if (lane >= off) incl += t;
    }
    int run = incl - sum;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      base[4 * lane + i] = run;
      run += a[i];
    }
    if (lane == 63) base[MR_EMAX] = incl;
  }
  __syncthreads();
  if (tid <= E) offsets[tid] = base[tid];

  volatile int* vh = hist + wave * MR_EMAX;
  for (int i0 = lo; i0 < hi; i0 += 64) {
    const int i = i0 + lane;
    const int e = i < hi ? ids[i] : -1;
    const bool ok = (unsigned)e < (unsigned)E;
    u64 peers = __ballot(ok);
#pragma unroll
    for (int b = 0; b < 8; ++b) {
      const bool bit = (e >> b) & 1;
      const u64 bb = __ballot(bit);
      peers &= bit ? bb : ~bb;
    }
    const int rank = __popcll(peers & ((1ull << lane) - 1ull));
    const int cnt = __popcll(peers);
    if (ok) {
      const int pos = base[e] + vh[e] + rank;
      if (pos < n) sorted[pos] = i;
    }
    __builtin_amdgcn_wave_barrier();
    if (ok && rank == cnt - 1) vh[e] = vh[e] + cnt;
    __builtin_amdgcn_wave_barrier();
  }
}

__global__ __launch_bounds__(MR_NT) void moe_route_kernel(
    const __hip_bfloat16* __restrict__ logits,   // [T, E]
    int* ids,                                    // [T, k]
    float* __restrict__ wts,                     // [T, k]
    int* __restrict__ offsets,                   // [E + 1]
    int* __restrict__ sorted,                    // [T * k]
    int* ticket,                                 // [1], zero between launches
    const int T, const int E, const int k, const int renorm) {
  __shared__ int hist[MR_WAVES * MR_EMAX];
  __shared__ int base[MR_EMAX + 1];
  __shared__ int is_last;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int t = blockIdx.x * MR_WAVES + wave;
  if (t < T)
    route_token(logits + (size_t)t * E, E, k, renorm != 0, ids + (size_t)t * k,
                wts + (size_t)t * k, lane);
  // the last workgroup to get here groups what all of them wrote
  __threadfence();
  __syncthreads();
  if (tid == 0) is_last = atomicAdd(ticket, 1) == (int)gridDim.x - 1;
  __syncthreads();
  if (!is_last) return;
  __threadfence();
  if (tid == 0) *ticket = 0;
  group_pairs(ids, T * k, E, offsets, sorted, hist, base);
}

// The grouping alone, for ids that did not come from moe_route_kernel.
__global__ __launch_bounds__(MR_NT) void moe_group_kernel(
    const int* ids, int* __restrict__ offsets, int* __restrict__ sorted,
    const int n, const int E) {
  __shared__ int hist[MR_WAVES * MR_EMAX];
  __shared__ int base[MR_EMAX + 1];
  group_pairs(ids, n, E, offsets, sorted, hist, base);
}

// ---------------------------------------------------------------------------
// 2, 3. grouped GEMMs

constexpr int MG_KSTEP = 64;                 // k per LDS stage
constexpr int MG_PITCH = MG_KSTEP + 8;       // +8 bf16: bank-conflict pad
constexpr int MG_NT = 256;                   // threads (4 waves)
constexpr int MG_MT = 4;                     // row tiles per pass, n > 16
constexpr int MG_STAGE_BYTES = 2 * (64 + 16 * MG_MT) * MG_PITCH * 2;
constexpr int MG_RED_BYTES = 2 * MG_MT * 2 * 256 * 4;
constexpr int MG_LDS_BYTES =
    MG_STAGE_BYTES > MG_RED_BYTES ? MG_STAGE_BYTES : MG_RED_BYTES;

// One pass of one workgroup: acc[mt][i] += W tile (t0 + 2i) x A tile mt over
// nsteps 64-k steps.  wb0/wb1 are this thread's two W pieces (stage rows srow
// and 32 + srow), ab0/ab1 its A pieces (tile rows srow and 32 + srow, clamped
// to a live row by the caller), all at k = 0.
template <int MT>
DEV_INLINE void mg_pass(__hip_bfloat16* stage,
                        const __hip_bfloat16* __restrict__ wb0,
                        const __hip_bfloat16* __restrict__ wb1,
                        const __hip_bfloat16* __restrict__ ab0,
                        const __hip_bfloat16* __restrict__ ab1,
                        const int nsteps, f32x4 (&acc)[MT][2]) {
  constexpr int A_ROWS = MT * 16;
  constexpr int BUF = (64 + A_ROWS) * MG_PITCH;
  constexpr bool A2 = A_ROWS > 32;           // a second A piece per thread
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int gl = lane & 15, gslice = lane >> 4;
  const int t0 = wave & 1, k_slice = wave >> 1;
  const int srow = tid >> 3, schk = (tid & 7) * 8;
  const bool a_live = A2 || srow < A_ROWS;

  // the two in-flight load sets, named scalars (skinny_gemm.hip)
  uint4 w00, w01, a00, a01 = {};
  uint4 w10, w11, a10, a11 = {};
#define MG_LD(p, kb) (*reinterpret_cast<const uint4*>((p) + (kb)))
#define MG_ISSUE(step, wa, wb, aa, ab)                                      \
  do {                                                                      \
    const int kb = min(step, nsteps - 1) * MG_KSTEP;                        \
    aa = MG_LD(ab0, kb);                                                    \
    if (A2) ab = MG_LD(ab1, kb);                                            \
    wa = MG_LD(wb0, kb);                                                    \
    wb = MG_LD(wb1, kb);                                                    \
  } while (0)
#define MG_ST(st, row) reinterpret_cast<uint4*>(&st[(row) * MG_PITCH + schk])
#define MG_WRITE(st, wa, wb, aa, ab)                                        \
  do {                                                                      \
    *MG_ST(st, srow) = wa;                                                  \
    *MG_ST(st, 32 + srow) = wb;                                             \
    if (a_live) *MG_ST(st, 64 + srow) = aa;                                 \
    if (A2) *MG_ST(st, 96 + srow) = ab;                                     \
  } while (0)

  const int kf = k_slice * 32 + gslice * 8;
  auto compute = [&](const __hip_bfloat16* st) {
    const bf16x8 wf0 = lds_frag(&st[(t0 * 16 + gl) * MG_PITCH + kf]);
    const bf16x8 wf1 = lds_frag(&st[((t0 + 2) * 16 + gl) * MG_PITCH + kf]);
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      const bf16x8 af = lds_frag(&st[(64 + mt * 16 + gl) * MG_PITCH + kf]);
      acc[mt][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf0, af, acc[mt][0],
                                                           0, 0, 0);
      acc[mt][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf1, af, acc[mt][1],
                                                           0, 0, 0);
    }
  };

  __hip_bfloat16* buf0 = stage;
  __hip_bfloat16* buf1 = stage + BUF;
  MG_ISSUE(0, w00, w01, a00, a01);
  MG_ISSUE(1, w10, w11, a10, a11);
  MG_WRITE(buf0, w00, w01, a00, a01);
  MG_ISSUE(2, w00, w01, a00, a01);
  for (int step = 0; step < nsteps; step += 2) {
    __syncthreads();
    compute(buf0);
    MG_WRITE(buf1, w10, w11, a10, a11);
    MG_ISSUE(step + 3, w10, w11, a10, a11);
    if (step + 1 >= nsteps) break;           // odd step count
    __syncthreads();
    compute(buf1);
    MG_WRITE(buf0, w00, w01, a00, a01);
    MG_ISSUE(step + 4, w00, w01, a00, a01);
  }
#undef MG_WRITE
#undef MG_ST
#undef MG_ISSUE
#undef MG_LD
}

// e4m3 W: 128-k stages, W as bytes in LDS (the file header has the layout)
constexpr int M8_KSTAGE = 128;
constexpr int M8_WPITCH = M8_KSTAGE + 16;    // bytes per staged W row
constexpr int M8_APITCH = M8_KSTAGE + 8;     // bf16 per staged A row
constexpr int M8_W_BYTES = 64 * M8_WPITCH;
constexpr int M8_STAGE_BYTES =
    2 * (M8_W_BYTES + 16 * MG_MT * M8_APITCH * 2);
constexpr int M8_LDS_BYTES =
    M8_STAGE_BYTES > MG_RED_BYTES ? M8_STAGE_BYTES : MG_RED_BYTES;

// mg_pass for e4m3 W.  wb0/wb1: this thread's W rows (stage rows srow and
// 32 + srow) at k = 0; ab0..ab3: its A rows (tile rows arow + 16 i, clamped
// by the caller; ab1..ab3 are read at MT = 4 only) at k = 0.  The thread's
// piece within a stage is added here, clamped to the row's last piece.
template <int MT>
DEV_INLINE void mg_pass_w8(unsigned char* stage,
                           const uint8_t* __restrict__ wb0,
                           const uint8_t* __restrict__ wb1,
                           const __hip_bfloat16* __restrict__ ab0,
                           const __hip_bfloat16* __restrict__ ab1,
                           const __hip_bfloat16* __restrict__ ab2,
                           const __hip_bfloat16* __restrict__ ab3,
                           const int nsteps, f32x4 (&acc)[MT][2]) {
  constexpr int BUF = M8_W_BYTES + 16 * MT * M8_APITCH * 2;
  constexpr bool A4 = MT > 1;                // four A pieces per thread
  static_assert(MT == 1 || MT == 4, "one or four A pieces per thread");
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int gl = lane & 15, gslice = lane >> 4;
  const int t0 = wave & 1, k_slice = wave >> 1;
  const int srow = tid >> 3, wchk = (tid & 7) * 16;   // W: bytes
  const int arow = tid >> 4, achk = (tid & 15) * 8;   // A: bf16
  const int K = nsteps * MG_KSTEP;
  const int nstages = (nsteps + 1) >> 1;

  uint4 w00, w01, a00, a01 = {}, a02 = {}, a03 = {};
  uint4 w10, w11, a10, a11 = {}, a12 = {}, a13 = {};
#define M8_LD(p, kb) (*reinterpret_cast<const uint4*>((p) + (kb)))
#define M8_ISSUE(stg, wa, wb, aa, ab, ac, ad)                               \
  do {                                                                      \
    const int kb = min(stg, nstages - 1) * M8_KSTAGE;                       \
    const int ka = min(kb + achk, K - 8);                                   \
    const int kw = min(kb + wchk, K - 16);                                  \
    aa = M8_LD(ab0, ka);                                                    \
    if (A4) {                                                               \
      ab = M8_LD(ab1, ka);                                                  \
      ac = M8_LD(ab2, ka);                                                  \
      ad = M8_LD(ab3, ka);                                                  \
    }                                                                       \
    wa = M8_LD(wb0, kw);                                                    \
    wb = M8_LD(wb1, kw);                                                    \
  } while (0)
#define M8_WST(st, row)                                                     \
  reinterpret_cast<uint4*>((st) + (row) * M8_WPITCH + wchk)
#define M8_AST(st, row)                                                     \
  reinterpret_cast<uint4*>((st) + M8_W_BYTES +                              \
                           ((row) * M8_APITCH + achk) * 2)
#define M8_WRITE(st, wa, wb, aa, ab, ac, ad)                                \
  do {                                                                      \
    *M8_WST(st, srow) = wa;                                                 \
    *M8_WST(st, 32 + srow) = wb;                                            \
    *M8_AST(st, arow) = aa;                                                 \
    if (A4) {                                                               \
      *M8_AST(st, 16 + arow) = ab;                                          \
      *M8_AST(st, 32 + arow) = ac;                                          \
      *M8_AST(st, 48 + arow) = ad;                                          \
    }                                                                       \
  } while (0)

  // stage `stg` of buffer st: its first 64-k step, and its second unless the
  // step count is odd and this is the last stage
  auto compute = [&](const unsigned char* st, const int stg) {
    const __hip_bfloat16* ast =
        reinterpret_cast<const __hip_bfloat16*>(st + M8_W_BYTES);
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      if (half == 1 && 2 * stg + 1 >= nsteps) break;
      const int kf = half * MG_KSTEP + k_slice * 32 + gslice * 8;
      const bf16x8 wf0 = lds_frag_w8(&st[(t0 * 16 + gl) * M8_WPITCH + kf]);
      const bf16x8 wf1 =
          lds_frag_w8(&st[((t0 + 2) * 16 + gl) * M8_WPITCH + kf]);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const bf16x8 af = lds_frag(&ast[(mt * 16 + gl) * M8_APITCH + kf]);
        acc[mt][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            wf0, af, acc[mt][0], 0, 0, 0);
        acc[mt][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            wf1, af, acc[mt][1], 0, 0, 0);
      }
    }
  };

  unsigned char* buf0 = stage;
  unsigned char* buf1 = stage + BUF;
  M8_ISSUE(0, w00, w01, a00, a01, a02, a03);
  M8_ISSUE(1, w10, w11, a10, a11, a12, a13);
  M8_WRITE(buf0, w00, w01, a00, a01, a02, a03);
  M8_ISSUE(2, w00, w01, a00, a01, a02, a03);
  for (int stg = 0; stg < nstages; stg += 2) {
    __syncthreads();
    compute(buf0, stg);
    M8_WRITE(buf1, w10, w11, a10, a11, a12, a13);
    M8_ISSUE(stg + 3, w10, w11, a10, a11, a12, a13);
    if (stg + 1 >= nstages) break;           // odd stage count
    __syncthreads();
    compute(buf1, stg + 1);
    M8_WRITE(buf0, w00, w01, a00, a01, a02, a03);
    M8_ISSUE(stg + 4, w00, w01, a00, a01, a02, a03);
  }
#undef M8_WRITE
#undef M8_AST
#undef M8_WST
#undef M8_ISSUE
#undef M8_LD
}

// MXFP4 W: 128-k stages, W as codes with their exponents in LDS (the file
// header has the layout).  The tag type tells the instantiation from e4m3's.
struct mxfp4_t { uint8_t codes; };
constexpr int M4_WPITCH = 80;                // 64 B codes, 4 exponents, pad
constexpr int M4_W_BYTES = 64 * M4_WPITCH;
constexpr int M4_STAGE_BYTES =
    2 * (M4_W_BYTES + 16 * MG_MT * M8_APITCH * 2);
constexpr int M4_LDS_BYTES =
    M4_STAGE_BYTES > MG_RED_BYTES ? M4_STAGE_BYTES : MG_RED_BYTES;

// MFMA fragment from 8 staged e2m1 codes of one row: row points at the
// staged row, cb is the byte of the lane's first code and blk its scale
// block within the stage.  dq = e2m1 * 2^e comes out of the conversion.
DEV_INLINE bf16x8 lds_frag_w4(const unsigned char* row, const int cb,
                              const int blk) {
  const unsigned codes = *reinterpret_cast<const unsigned*>(row + cb);
  const float scale =
      w8_exp2i(reinterpret_cast<const signed char*>(row)[64 + blk]);
  union { bf16x2 v; unsigned u; } p0, p1, p2, p3;
  p0.v = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(codes, scale, 0);
  p1.v = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(codes, scale, 1);
  p2.v = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(codes, scale, 2);
  p3.v = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp4(codes, scale, 3);
  union { uint4 u; bf16x8 v; } cvt;
  cvt.u = make_uint4(p0.u, p1.u, p2.u, p3.u);
  return cvt.v;
}

// mg_pass for MXFP4 W.  wrow / erow: the codes and the exponents of this
// thread's W row (stage row tid >> 2) at k = 0; ab0..ab3 as in mg_pass_w8.
// The thread's block within a stage is added here, clamped to the row's last.
template <int MT>
DEV_INLINE void mg_pass_w4(unsigned char* stage,
                           const uint8_t* __restrict__ wrow,
                           const int8_t* __restrict__ erow,
                           const __hip_bfloat16* __restrict__ ab0,
                           const __hip_bfloat16* __restrict__ ab1,
                           const __hip_bfloat16* __restrict__ ab2,
                           const __hip_bfloat16* __restrict__ ab3,
                           const int nsteps, f32x4 (&acc)[MT][2]) {
  constexpr int BUF = M4_W_BYTES + 16 * MT * M8_APITCH * 2;
  constexpr bool A4 = MT > 1;                // four A pieces per thread
  static_assert(MT == 1 || MT == 4, "one or four A pieces per thread");
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int gl = lane & 15, gslice = lane >> 4;
  const int t0 = wave & 1, k_slice = wave >> 1;
  const int wr = tid >> 2, wblk = tid & 3;            // W: row, block of stage
  const int arow = tid >> 4, achk = (tid & 15) * 8;   // A: bf16
  const int K = nsteps * MG_KSTEP;
  const int nstages = (nsteps + 1) >> 1;
  const int nblocks = K / 32;

  uint4 w0, a00, a01 = {}, a02 = {}, a03 = {};
  uint4 w1, a10, a11 = {}, a12 = {}, a13 = {};
  int e0, e1;
#define M4_LD(p, kb) (*reinterpret_cast<const uint4*>((p) + (kb)))
#define M4_ISSUE(stg, wa, ea, aa, ab, ac, ad)                               \
  do {                                                                      \
    const int s = min(stg, nstages - 1);                                    \
    const int ka = min(s * M8_KSTAGE + achk, K - 8);                        \
    const int blk = min(s * 4 + wblk, nblocks - 1);                         \
    aa = M4_LD(ab0, ka);                                                    \
    if (A4) {                                                               \
      ab = M4_LD(ab1, ka);                                                  \
      ac = M4_LD(ab2, ka);                                                  \
      ad = M4_LD(ab3, ka);                                                  \
    }                                                                       \
    wa = M4_LD(wrow, blk * 16);                                             \
    ea = erow[blk];                                                         \
  } while (0)
#define M4_AST(st, row)                                                     \
  reinterpret_cast<uint4*>((st) + M4_W_BYTES +                              \
                           ((row) * M8_APITCH + achk) * 2)
#define M4_WRITE(st, wa, ea, aa, ab, ac, ad)                                \
  do {                                                                      \
    *reinterpret_cast<uint4*>((st) + wr * M4_WPITCH + wblk * 16) = wa;      \
    (st)[wr * M4_WPITCH + 64 + wblk] = (unsigned char)ea;                   \
    *M4_AST(st, arow) = aa;                                                 \
    if (A4) {                                                               \
      *M4_AST(st, 16 + arow) = ab;                                          \
      *M4_AST(st, 32 + arow) = ac;                                          \
      *M4_AST(st, 48 + arow) = ad;                                          \
    }                                                                       \
  } while (0)

  // stage `stg` of buffer st: its first 64-k step, and its second unless the
  // step count is odd and this is the last stage
  auto compute = [&](const unsigned char* st, const int stg) {
    const __hip_bfloat16* ast =
        reinterpret_cast<const __hip_bfloat16*>(st + M4_W_BYTES);
#pragma unroll
    for (int half = 0; half < 2; ++half) {
      if (half == 1 && 2 * stg + 1 >= nsteps) break;
      const int kf = half * MG_KSTEP + k_slice * 32 + gslice * 8;
      const int blk = half * 2 + k_slice;
      const bf16x8 wf0 =
          lds_frag_w4(&st[(t0 * 16 + gl) * M4_WPITCH], kf >> 1, blk);
      const bf16x8 wf1 =
          lds_frag_w4(&st[((t0 + 2) * 16 + gl) * M4_WPITCH], kf >> 1, blk);
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const bf16x8 af = lds_frag(&ast[(mt * 16 + gl) * M8_APITCH + kf]);
        acc[mt][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            wf0, af, acc[mt][0], 0, 0, 0);
        acc[mt][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            wf1, af, acc[mt][1], 0, 0, 0);
      }
    }
  };

  unsigned char* buf0 = stage;
  unsigned char* buf1 = stage + BUF;
  M4_ISSUE(0, w0, e0, a00, a01, a02, a03);
  M4_ISSUE(1, w1, e1, a10, a11, a12, a13);
  M4_WRITE(buf0, w0, e0, a00, a01, a02, a03);
  M4_ISSUE(2, w0, e0, a00, a01, a02, a03);
  for (int stg = 0; stg < nstages; stg += 2) {
    __syncthreads();
    compute(buf0, stg);
    M4_WRITE(buf1, w1, e1, a10, a11, a12, a13);
    M4_ISSUE(stg + 3, w1, e1, a10, a11, a12, a13);
    if (stg + 1 >= nstages) break;           // odd stage count
    __syncthreads();
    compute(buf1, stg + 1);
    M4_WRITE(buf0, w0, e0, a00, a01, a02, a03);
    M4_ISSUE(stg + 4, w0, e0, a00, a01, a02, a03);
  }
#undef M4_WRITE
#undef M4_AST
#undef M4_ISSUE
#undef M4_LD
}

struct MoeGemmArgs {
  void* out;                  // GATE_UP: h bf16 [TK, N]; else opart f32 [TK, N]
  const __hip_bfloat16* a;    // GATE_UP: x [T, K]; else h [TK, K]
  const void* w;              // GATE_UP: w1 [E, 2N, K]; else w2 [E, N, K]
  const int* offsets;         // [E + 1]
  const int* sorted;          // [TK]
  int TK, k, K, N, panels;
  // e4m3 w: [E, 2N] or [E, N] exponents; MXFP4 w: [E, 2N, K / 32] or
  // [E, N, K / 32]; else null
  const int8_t* wexp;
};

// All passes of one expert's rows at MT row tiles per pass.
// WT: __hip_bfloat16, or uint8_t for e4m3 W, whose exponents for this panel's
// stage rows start at we (gate rows; the up rows' are g.N further), or
// mxfp4_t: wb0 and we are then the codes and the exponents of this thread's
// one W row.
template <int MT, bool GATE_UP, typename WT>
DEV_INLINE void mg_expert(const MoeGemmArgs& g, unsigned char* smem,
                          const WT* wb0, const WT* wb1, const int8_t* we,
                          const int off, const int n, const int panel) {
  constexpr bool W8 = std::is_same<WT, uint8_t>::value;
  constexpr bool W4 = std::is_same<WT, mxfp4_t>::value;
  __hip_bfloat16* stage = reinterpret_cast<__hip_bfloat16*>(smem);
  float* red = reinterpret_cast<float*>(smem);
  const int tid = threadIdx.x;
  const int wave = tid >> 6, lane = tid & 63;
  const int gl = lane & 15, gslice = lane >> 4;
  const int t0 = wave & 1, k_slice = wave >> 1;
  const int srow = tid >> 3, schk = (tid & 7) * 8;
  const int nsteps = g.K / MG_KSTEP;

  for (int r0 = 0; r0 < n; r0 += 16 * MT) {
    const int live = min(n - r0, 16 * MT);
    // sorted row -> A row: the pair's token (gather) or the row itself
    const int s0 = off + r0 + min(srow, live - 1);
    const int s1 = off + r0 + min(32 + srow, live - 1);
    size_t ar0, ar1;
    if (GATE_UP) {
      ar0 = (size_t)(min(max(g.sorted[s0], 0), g.TK - 1) / g.k);
      ar1 = (size_t)(min(max(g.sorted[s1], 0), g.TK - 1) / g.k);
    } else {
      ar0 = (size_t)s0;
      ar1 = (size_t)s1;
    }
    f32x4 acc[MT][2];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
      acc[mt][0] = {0.f, 0.f, 0.f, 0.f};
      acc[mt][1] = {0.f, 0.f, 0.f, 0.f};
    }
    if constexpr (W8 || W4) {
      // tile rows arow + 16 i of this pass, 16 lanes per row
      const __hip_bfloat16* ab[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int s = off + r0 + min((tid >> 4) + 16 * i, live - 1);
        const size_t ar = GATE_UP ? (size_t)(min(max(g.sorted[s], 0),
                                                 g.TK - 1) / g.k)
                                  : (size_t)s;
        ab[i] = g.a + ar * g.K;
      }
      if constexpr (W4)
        mg_pass_w4<MT>(smem, &wb0->codes, we, ab[0], ab[1], ab[2], ab[3],
                       nsteps, acc);
      else
        mg_pass_w8<MT>(smem, wb0, wb1, ab[0], ab[1], ab[2], ab[3], nsteps,
                       acc);
    } else {
      mg_pass<MT>(stage, wb0, wb1, g.a + ar0 * g.K + schk,
                  g.a + ar1 * g.K + schk, nsteps, acc);
    }

    // fold the two k-slices: slice 1 -> LDS -> slice 0 adds and stores
    __syncthreads();
    if (k_slice == 1) {
#pragma unroll
      for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            red[((t0 * MT + mt) * 2 + i) * 256 + r * 64 + lane] =
                acc[mt][i][r];
    }
    __syncthreads();
    if (k_slice == 0) {
      // lane: token row gl of tile mt, W rows 4 * gslice + r of both tiles
#pragma unroll
      for (int mt = 0; mt < MT; ++mt) {
        const int m = r0 + mt * 16 + gl;
        if (m >= n) continue;
        float v[2][4];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
          for (int r = 0; r < 4; ++r)
            v[i][r] = acc[mt][i][r] +
                      red[((t0 * MT + mt) * 2 + i) * 256 + r * 64 + lane];
        if constexpr (W8) {
          // 2^e of W rows 4 * gslice + r: four int8 of one word per tile
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            const int row = (GATE_UP ? i * g.N + t0 * 16
                                     : (t0 + 2 * i) * 16) + gslice * 4;
            const unsigned word =
                *reinterpret_cast<const unsigned*>(we + row);
#pragma unroll
            for (int r = 0; r < 4; ++r)   // byte r, sign-extended
              v[i][r] *= w8_exp2i((int)(word << (24 - 8 * r)) >> 24);
          }
        }
        if (GATE_UP) {
          union { __hip_bfloat16 e[4]; uint2 u; } hv;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const float gv = v[0][r];
            const float silu = gv / (1.f + __expf(-gv));
            hv.e[r] = f2bf(silu * v[1][r]);
          }
          __hip_bfloat16* h = reinterpret_cast<__hip_bfloat16*>(g.out);
          *reinterpret_cast<uint2*>(h + (size_t)(off + m) * g.N + panel * 32 +
                                    t0 * 16 + gslice * 4) = hv.u;
        } else {
          const int p = min(max(g.sorted[off + m], 0), g.TK - 1);
          float* o = reinterpret_cast<float*>(g.out) + (size_t)p * g.N +
                     panel * 64 + gslice * 4;
#pragma unroll
          for (int i = 0; i < 2; ++i)
            *reinterpret_cast<float4*>(o + (t0 + 2 * i) * 16) =
                make_float4(v[i][0], v[i][1], v[i][2], v[i][3]);
        }
      }
    }
    __syncthreads();                         // red aliases the next stage
  }
}

template <bool GATE_UP, typename WT>
__global__ __launch_bounds__(MG_NT) void moe_gemm_kernel(const MoeGemmArgs g) {
  constexpr bool W8 = std::is_same<WT, uint8_t>::value;
  constexpr bool W4 = std::is_same<WT, mxfp4_t>::value;
  __shared__ __attribute__((aligned(16))) unsigned char
      smem[W8 ? M8_LDS_BYTES : W4 ? M4_LDS_BYTES : MG_LDS_BYTES];
  const int e = blockIdx.x / g.panels;
  const int panel = blockIdx.x % g.panels;
  const int off = min(max(g.offsets[e], 0), g.TK);
  const int n = min(max(g.offsets[e + 1], off), g.TK) - off;
  if (n <= 0) return;
  // (an e4m3 pass adds the thread's piece itself: it clamps it to the row)
  const int srow = threadIdx.x >> 3, schk = W8 ? 0 : (threadIdx.x & 7) * 8;
  const WT* w = reinterpret_cast<const WT*>(g.w);
  const WT* wb0;
  const WT* wb1;
  const int8_t* we = nullptr;
  if constexpr (W4) {         // one W row per thread: stage row tid >> 2
    const int r = threadIdx.x >> 2;
    const size_t row =
        GATE_UP ? (size_t)e * 2 * g.N + (r >> 5) * g.N + panel * 32 + (r & 31)
                : (size_t)e * g.N + panel * 64 + r;
    wb0 = wb1 = w + row * (g.K / 2);
    we = g.wexp + row * (g.K / 32);
  } else if (GATE_UP) {       // stage rows [0, 32) gate, [32, 64) up
    wb0 = w + ((size_t)e * 2 * g.N + panel * 32 + srow) * g.K + schk;
    wb1 = wb0 + (size_t)g.N * g.K;
    if (W8) we = g.wexp + (size_t)e * 2 * g.N + panel * 32;
  } else {
    wb0 = w + ((size_t)e * g.N + panel * 64 + srow) * g.K + schk;
    wb1 = wb0 + (size_t)32 * g.K;
    if (W8) we = g.wexp + (size_t)e * g.N + panel * 64;
  }
  if (n <= 16)
    mg_expert<1, GATE_UP>(g, smem, wb0, wb1, we, off, n, panel);
  else
    mg_expert<MG_MT, GATE_UP>(g, smem, wb0, wb1, we, off, n, panel);
}

// ---------------------------------------------------------------------------
// 4. combine: 8 columns per thread, like reduce_splits with weights

__global__ void moe_combine_kernel(__hip_bfloat16* __restrict__ y,   // [T, H]
                                   const float* __restrict__ opart,  // [TK, H]
                                   const float* __restrict__ wts,    // [T, k]
                                   const int k, const int hvec,
                                   const long total) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const long t = i / hvec;
  const int c = (int)(i % hvec) * 8;
  const int H = hvec * 8;
  float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  for (int j = 0; j < k; ++j) {
    // The product is rounded before it is added.  HIP's __fmul_rn / __fadd_rn
    // are a plain * and + that the compiler's default contraction fused into
    // v_fmac_f32 (one rounding); the pragma is what keeps them apart.
#pragma clang fp contract(off)
    const float w = wts[t * k + j];
    const float* o = opart + (size_t)(t * k + j) * H + c;
    const float4 lo = *reinterpret_cast<const float4*>(o);
    const float4 hi = *reinterpret_cast<const float4*>(o + 4);
    const float ov[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
#pragma unroll
    for (int q = 0; q < 8; ++q)
      acc[q] = acc[q] + w * ov[q];                       // two roundings
  }
  Bf16x8U out;
#pragma unroll
  for (int q = 0; q < 8; ++q) out.e[q] = f2bf(acc[q]);
  *reinterpret_cast<uint4*>(y + (size_t)t * H + c) = out.u;
}

}  // namespace

extern "C" {

hipError_t launch_moe_route(void* ids, void* weights, void* expert_offsets,
                            void* sorted_pairs, void* ticket,
                            const void* logits, int T, int E, int k,
                            int renormalize, hipStream_t stream) {
  if (T < 1 || E < 1 || E > MR_EMAX || k < 1 || k > 8 || k > E)
    return hipErrorInvalidValue;
  moe_route_kernel<<<dim3((T + MR_WAVES - 1) / MR_WAVES), dim3(MR_NT), 0,
                     stream>>>((const __hip_bfloat16*)logits, (int*)ids,
                               (float*)weights, (int*)expert_offsets,
                               (int*)sorted_pairs, (int*)ticket, T, E, k,
                               renormalize);
  return hipGetLastError();
}

hipError_t launch_moe_group(void* expert_offsets, void* sorted_pairs,
                            const void* ids, int n, int E,
                            hipStream_t stream) {
  if (n < 1 || E < 1 || E > MR_EMAX) return hipErrorInvalidValue;
  moe_group_kernel<<<dim3(1), dim3(MR_NT), 0, stream>>>(
      (const int*)ids, (int*)expert_offsets, (int*)sorted_pairs, n, E);
  return hipGetLastError();
}

hipError_t launch_moe_ffn(const MoeFfnLaunch& a, hipStream_t stream) {
  if (a.T < 1 || a.k < 1 || a.k > 8 || a.E < 1 || a.E > MR_EMAX ||
      a.H < 256 || a.H % 256 || a.I < 64 || a.I % 64)
    return hipErrorInvalidValue;
  const bool scaled = a.w1_exp != nullptr;
  if (scaled != (a.w2_exp != nullptr) ||
      scaled != (a.format != MoeFfnLaunch::BF16))
    return hipErrorInvalidValue;
  const int TK = a.T * a.k;
  const MoeGemmArgs gu = {a.h, (const __hip_bfloat16*)a.x, a.w1,
                          (const int*)a.expert_offsets,
                          (const int*)a.sorted_pairs, TK, a.k, a.H, a.I,
                          a.I / 32, (const int8_t*)a.w1_exp};
  const MoeGemmArgs dn = {a.opart, (const __hip_bfloat16*)a.h, a.w2,
                          (const int*)a.expert_offsets,
                          (const int*)a.sorted_pairs, TK, a.k, a.I, a.H,
                          a.H / 64, (const int8_t*)a.w2_exp};
  const dim3 ggu(a.E * gu.panels), gdn(a.E * dn.panels), block(MG_NT);
  if (a.format == MoeFfnLaunch::MXFP4) {
    moe_gemm_kernel<true, mxfp4_t><<<ggu, block, 0, stream>>>(gu);
    moe_gemm_kernel<false, mxfp4_t><<<gdn, block, 0, stream>>>(dn);
  } else if (a.format == MoeFfnLaunch::E4M3) {
    moe_gemm_kernel<true, uint8_t><<<ggu, block, 0, stream>>>(gu);
    moe_gemm_kernel<false, uint8_t><<<gdn, block, 0, stream>>>(dn);
  } else {
    moe_gemm_kernel<true, __hip_bfloat16><<<ggu, block, 0, stream>>>(gu);
    moe_gemm_kernel<false, __hip_bfloat16><<<gdn, block, 0, stream>>>(dn);
  }
  const int hvec = a.H / 8;
  const long total = (long)a.T * hvec;
  moe_combine_kernel<<<dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                       stream>>>((__hip_bfloat16*)a.y, (const float*)a.opart,
                                 (const float*)a.weights, a.k, hvec, total);
  return hipGetLastError();
}

}  // extern "C"

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
