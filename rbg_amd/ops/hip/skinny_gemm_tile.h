// Skinny-GEMM building blocks shared by skinny_gemm.hip, skinny_gemm_w8.hip
// and moe.hip (gfx950, v_mfma_f32_16x16x32_bf16): the LDS fragment load, the
// split-count dispatcher, and the 64-column-panel kernel that the bf16 and the
// e4m3 weight formats both instantiate.
#pragma once

#include "common.h"

namespace {

// MFMA A/B fragment: 8 bf16 of one staged row, contiguous in k
DEV_INLINE bf16x8 lds_frag(const __hip_bfloat16* p) {
  union { uint4 u; bf16x8 v; } cvt;
  cvt.u = *reinterpret_cast<const uint4*>(p);
  return cvt.v;
}

// Four e4m3 bytes -> four bf16, two per v_cvt_scalef32_pk_bf16_fp8 at scale 1
// (exact: e4m3's four significant bits and exponent range fit a bf16).
DEV_INLINE uint2 w8_cvt4(unsigned w) {
  union { bf16x2 v; unsigned u; } lo, hi;
  lo.v = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, false);
  hi.v = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, true);
  uint2 r;
  r.x = lo.u;
  r.y = hi.u;
  return r;
}

// 16 e4m3 bytes -> 16 bf16 as two 16-byte pieces (elements 0-7, 8-15)
DEV_INLINE void w8_cvt16(const uint4& b, uint4& lo, uint4& hi) {
  const uint2 a0 = w8_cvt4(b.x), a1 = w8_cvt4(b.y);
  const uint2 a2 = w8_cvt4(b.z), a3 = w8_cvt4(b.w);
  lo = make_uint4(a0.x, a0.y, a1.x, a1.y);
  hi = make_uint4(a2.x, a2.y, a3.x, a3.y);
}

// MFMA fragment from 8 staged e4m3 bytes of one row: one 8-byte LDS read,
// converted by the lane that feeds it to the MFMA
DEV_INLINE bf16x8 lds_frag_w8(const uint8_t* p) {
  const uint2 b = *reinterpret_cast<const uint2*>(p);
  const uint2 lo = w8_cvt4(b.x), hi = w8_cvt4(b.y);
  union { uint4 u; bf16x8 v; } cvt;
  cvt.u = make_uint4(lo.x, lo.y, hi.x, hi.y);
  return cvt.v;
}

// 2^e as f32 bits; |e| <= 64 keeps the exponent field normal
DEV_INLINE float w8_exp2i(int e) {
  return __uint_as_float((unsigned)(e + 127) << 23);
}

// One kernel per split count the GEMMs are instantiated for.  KERNEL is a
// template over (row tiles, SPLITS, ...); grid, block, stream and splits are
// the launcher's.
#define LAUNCH_SPLITS(KERNEL, MT, ...)                                       \
  switch (splits) {                                                          \
    case 1:                                                                  \
      KERNEL<MT, 1><<<grid, block, 0, stream>>>(__VA_ARGS__);                \
      break;                                                                 \
    case 2:                                                                  \
      KERNEL<MT, 2><<<grid, block, 0, stream>>>(__VA_ARGS__);                \
      break;                                                                 \
    case 4:                                                                  \
      KERNEL<MT, 4><<<grid, block, 0, stream>>>(__VA_ARGS__);                \
      break;                                                                 \
    case 8:                                                                  \
      KERNEL<MT, 8><<<grid, block, 0, stream>>>(__VA_ARGS__);                \
      break;                                                                 \
    default:                                                                 \
      return hipErrorInvalidValue;                                           \
  }

// ---------------------------------------------------------------------------
// 64-column-panel kernel for M <= 128, N % 64 == 0, K % (SPLITS * 256) == 0.
//
// Why: a CU fills LDS from an L2-resident source at a fixed ~70 GB/s, and
// the 32-column kernel (skinny_gemm.hip) spends 4/5 of that fill on A (16 KB
// of A per 4 KB of W per step at M = 128).  Owning 64 columns stages A once
// per 8 KB of W, so the same fill rate carries twice the weight stream.
//
//   grid  = (N/64) * SPLITS workgroups of 8 waves: (k_slice 0..1) x
//           (4 row groups of MTW m-tiles); each wave holds MTW x 4 n-tile
//           accumulators, so an A fragment feeds 4 MFMAs and a W fragment
//           MTW.  MTW = 1 serves M <= 64 (64 staged rows), MTW = 2 M <= 128
//   stage = Fmt::KSTAGE k of W[64 rows] + A[64 MTW rows] through LDS as
//           16-byte pieces.  A thread carries ONE piece of W (row tid >> 3,
//           8 lanes per contiguous 128-byte row segment: the HBM request
//           shape) and KSTAGE/64 * MTW pieces of A (KSTAGE/8 lanes per row)
//   pipe  = double-buffered LDS with one barrier per stage: a buffer's
//           previous stage was fully read before the barrier.  A (L2) rides
//           two register sets 2-3 stages ahead; W (HBM) rides a ring of FOUR
//           registers 4-5 stages ahead, because one workgroup per CU at twice
//           the 32-column kernel's step rate halves the time a 2-deep set
//           would give an HBM miss to land.  A is issued before W in every
//           stage so the in-order vmcnt wait for A(t+1) never waits on the
//           younger W loads.  Stage numbers past the last are clamped to it:
//           those loads stay inside the split's k range and what they fetch
//           is written to a buffer nobody reads again
//   regs  = every load set is NAMED scalars, guarded by if (PIECES > n).  A
//           runtime-indexed set[2] array, a struct array passed through
//           lambda references, and an array with unrolled constant indices
//           were each demoted to scratch memory, and every prefetch then
//           round-tripped through HBM (ISA: scratch_load/store_dwordx4 in
//           the hot loop, 5x slower)
//   end   = k_slice 1 hands its accumulators to k_slice 0 through LDS, which
//           adds, scales the column where the format has a scale, and stores
//           bf16 c (SPLITS == 1) or f32 partials ws
//
// Bit contract, every format: identical to skinny_gemm_kernel on the bf16
// tensor the format stands for, at equal (M, N, K, SPLITS).  Per output
// element chain c in {0, 1} accumulates the 32-k blocks with index = c
// (mod 2) in increasing k (k-slice c takes offset c*32 of every 64-k
// sub-step), the two chains are added in f32, and splits are folded in split
// order by the same reduce / norm kernels; which wave owns a chain is the
// only difference.
//
// A weight format Fmt (passed by value, so that it may carry pointers; next to
// w, so that they are fetched with it and not when the epilogue asks) provides
//   W                      element type of w
//   KSTAGE                 k per stage, a multiple of 64; a 16-byte piece of
//                          W must be KSTAGE/8 elements
//   stage_w(dst, r)        writes register r, KSTAGE/8 elements of one W row,
//                          to LDS at dst as bf16
//   SCALED, col_scale(n)   whether, and by what, the epilogue multiplies
//                          column n's f32 sum

constexpr int SG64_NT = 512;                 // threads (8 waves)

// acc[mt][nt] += A tile (row0 + mt) x W tile nt over one 64-k sub-step of a
// stage st; kf is this lane's k offset in the stage.
template <int MTW, int PITCH>
DEV_INLINE void sg64_mfma_step(f32x4 (&acc)[MTW][4], const __hip_bfloat16* st,
                               const int kf, const int row0, const int gl) {
  const bf16x8 wf0 = lds_frag(&st[gl * PITCH + kf]);
  const bf16x8 wf1 = lds_frag(&st[(16 + gl) * PITCH + kf]);
  const bf16x8 wf2 = lds_frag(&st[(32 + gl) * PITCH + kf]);
  const bf16x8 wf3 = lds_frag(&st[(48 + gl) * PITCH + kf]);
#pragma unroll
  for (int mt = 0; mt < MTW; ++mt) {
    const bf16x8 af =
        lds_frag(&st[(64 + (row0 + mt) * 16 + gl) * PITCH + kf]);
    acc[mt][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, wf0, acc[mt][0],
                                                         0, 0, 0);
    acc[mt][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, wf1, acc[mt][1],
                                                         0, 0, 0);
    acc[mt][2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, wf2, acc[mt][2],
                                                         0, 0, 0);
    acc[mt][3] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, wf3, acc[mt][3],
                                                         0, 0, 0);
  }
}

// Fold the two k-slices and store: slice 1 -> red -> slice 0 adds, scales
// and writes c (SPLITS == 1) or this split's plane of ws.  All 8 waves call
// it; red is this wave's row group's MTW * 4 * 256 floats, aliasing the
// stage buffers.
template <int MTW, int SPLITS, class Fmt>
DEV_INLINE void sg64_fold_store(const f32x4 (&acc)[MTW][4], float* red,
                                const Fmt& fmt, __hip_bfloat16* __restrict__ c,
                                float* __restrict__ ws, const int M,
                                const int N, const int split, const int n0,
                                const int row0, const int k_slice,
                                const int lane) {
  const int gl = lane & 15, gslice = lane >> 4;
  // fetched before the barriers, so that the exchange hides the latency
  float scale[4];
  if constexpr (Fmt::SCALED) {
#pragma unroll
    for (int nt = 0; nt < 4; ++nt)
      scale[nt] = fmt.col_scale(n0 + (nt << 4) + gl);
  }
  __syncthreads();
  if (k_slice == 1) {
#pragma unroll
    for (int mt = 0; mt < MTW; ++mt)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        F32x4U u;
        u.v = acc[mt][nt];
#pragma unroll
        for (int r = 0; r < 4; ++r)
          red[(mt * 4 + nt) * 256 + r * 64 + lane] = u.e[r];
      }
  }
  __syncthreads();
  if (k_slice == 0) {
    // MFMA C layout: reg r of lane l is row 4*(l>>4)+r, column l&15
#pragma unroll
    for (int mt = 0; mt < MTW; ++mt)
#pragma unroll
      for (int nt = 0; nt < 4; ++nt) {
        F32x4U u;
        u.v = acc[mt][nt];
        const int n = n0 + (nt << 4) + gl;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float v = u.e[r] + red[(mt * 4 + nt) * 256 + r * 64 + lane];
          if constexpr (Fmt::SCALED) v *= scale[nt];
          const int m = (row0 + mt) * 16 + (gslice << 2) + r;
          if (m < M) {
            if (SPLITS == 1)
              c[(size_t)m * N + n] = f2bf(v);
            else
              ws[((size_t)split * M + m) * N + n] = v;
          }
        }
      }
  }
}

template <int MTW, int SPLITS, class Fmt>
__global__ __launch_bounds__(SG64_NT) void skinny_gemm64_kernel(
    const __hip_bfloat16* __restrict__ a,     // [M, K]
    const typename Fmt::W* __restrict__ w,    // [N, K]
    const Fmt fmt,
    __hip_bfloat16* __restrict__ c,           // [M, N]   (SPLITS == 1)
    float* __restrict__ ws,                   // [SPLITS, M, N] (SPLITS > 1)
    const int M, const int N, const int K) {
  constexpr int KSTAGE = Fmt::KSTAGE;
  constexpr int PITCH = KSTAGE + 8;          // +8 bf16: bank-conflict pad
  constexpr int A_LANES = KSTAGE / 8;        // 16-byte pieces per A row
  constexpr int A_STRIDE = SG64_NT / A_LANES;   // rows between a thread's pieces
  constexpr int A_ROWS = MTW * 64;
  constexpr int PIECES = A_ROWS / A_STRIDE;  // A pieces per thread
  static_assert(KSTAGE % 64 == 0 && PIECES >= 1 && PIECES <= 4,
                "PIECES outside the named register sets");
  // K % (SPLITS * 256) == 0 (host-side) makes a split a multiple of
  // 256 / KSTAGE stages; where that is no multiple of the ring's 4 the loop
  // below leaves after a pair
  constexpr bool TAIL = (256 / KSTAGE) % 4 != 0;

  // the builtins, not blockIdx / threadIdx: those go through device-library
  // functions, which a unit built without packed-fp32 ops (skinny_gemm_w8.hip)
  // cannot inline and calls instead
  const unsigned wg = __builtin_amdgcn_workgroup_id_x();
  const int n_groups = N >> 6;
  const int n_group = wg % n_groups;
  const int split = wg / n_groups;
  const int tid = (int)__builtin_amdgcn_workitem_id_x();
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int gl = lane & 15;
  const int gslice = lane >> 4;

  const int row_group = wave & 3;            // MTW m-tiles each
  const int k_slice = wave >> 2;             // 0..1, 32 k of each sub-step
  const int k_wg = K / SPLITS;
  const int k0 = split * k_wg;
  const int nstages = k_wg / KSTAGE;

  constexpr int BUF = (64 + A_ROWS) * PITCH;
  __shared__ union {
    __hip_bfloat16 stage[2][BUF];
    float red[4][MTW * 4 * 256];
  } lds;

  // W piece: row tid >> 3 at element (tid & 7) * KSTAGE/8, which is also its
  // k offset.  A piece s: row arow + A_STRIDE * s at k offset achk; rows past
  // M - 1 re-read row M - 1 and are never stored.
  const int wrow = tid >> 3, wchk = (tid & 7) * (KSTAGE / 8);
  const int arow = tid / A_LANES, achk = (tid % A_LANES) * 8;
  const typename Fmt::W* wbase = w + (size_t)((n_group << 6) + wrow) * K + wchk;
#define SG64_ABASE(s)                                                       \
  (a + (size_t)min(arow + A_STRIDE * (PIECES > (s) ? (s) : 0), M - 1) * K + \
   achk)
  const __hip_bfloat16* ab0 = SG64_ABASE(0);
  const __hip_bfloat16* ab1 = SG64_ABASE(1);
  const __hip_bfloat16* ab2 = SG64_ABASE(2);
  const __hip_bfloat16* ab3 = SG64_ABASE(3);
#undef SG64_ABASE

  uint4 w0, w1, w2, w3;
  uint4 a00, a01 = {}, a02 = {}, a03 = {};
  uint4 a10, a11 = {}, a12 = {}, a13 = {};

#define SG64_KB(t) (k0 + min(t, nstages - 1) * KSTAGE)
#define SG64_LD(p, kb) (*reinterpret_cast<const uint4*>((p) + (kb)))
#define SG64_ISSUE_A(t, x0, x1, x2, x3)                                     \
  do {                                                                      \
    const int kb = SG64_KB(t);                                              \
    x0 = SG64_LD(ab0, kb);                                                  \
    if (PIECES > 1) x1 = SG64_LD(ab1, kb);                                  \
    if (PIECES > 2) x2 = SG64_LD(ab2, kb);                                  \
    if (PIECES > 3) x3 = SG64_LD(ab3, kb);                                  \
  } while (0)
#define SG64_ISSUE_W(t, wr) wr = SG64_LD(wbase, SG64_KB(t))
#define SG64_AST(st, s)                                                     \
  reinterpret_cast<uint4*>(&st[(64 + arow + A_STRIDE * (s)) * PITCH + achk])
#define SG64_WRITE(st, wr, x0, x1, x2, x3)                                  \
  do {                                                                      \
    Fmt::stage_w(&st[wrow * PITCH + wchk], wr);                             \
    *SG64_AST(st, 0) = x0;                                                  \
    if (PIECES > 1) *SG64_AST(st, 1) = x1;                                  \
    if (PIECES > 2) *SG64_AST(st, 2) = x2;                                  \
    if (PIECES > 3) *SG64_AST(st, 3) = x3;                                  \
  } while (0)

  f32x4 acc[MTW][4];
#pragma unroll
  for (int mt = 0; mt < MTW; ++mt)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = {0.f, 0.f, 0.f, 0.f};

  const int kf = k_slice * 32 + gslice * 8;
  auto compute = [&](const __hip_bfloat16* st) {
#pragma unroll
    for (int h = 0; h < KSTAGE / 64; ++h)
      sg64_mfma_step<MTW, PITCH>(acc, st, h * 64 + kf, row_group * MTW, gl);
  };

  __hip_bfloat16* buf0 = lds.stage[0];
  __hip_bfloat16* buf1 = lds.stage[1];

  // prologue: A stages 0,1 and W stages 0..3 in flight; stage 0 lands in
  // buffer 0 and its registers are re-issued
  SG64_ISSUE_A(0, a00, a01, a02, a03);
  SG64_ISSUE_W(0, w0);
  SG64_ISSUE_A(1, a10, a11, a12, a13);
  SG64_ISSUE_W(1, w1);
  SG64_ISSUE_W(2, w2);
  SG64_ISSUE_W(3, w3);
  SG64_WRITE(buf0, w0, a00, a01, a02, a03);
  SG64_ISSUE_A(2, a00, a01, a02, a03);
  SG64_ISSUE_W(4, w0);

  // stage t: compute stage t, write stage t+1 (W ring slot (t+1)&3, A set
  // (t+1)&1) into the other buffer, re-issue those registers for A stage
  // t+3 and W stage t+5
#define SG64_STAGE(t, cur, nxt, wr, x0, x1, x2, x3)                         \
  do {                                                                      \
    __syncthreads();                                                        \
    compute(cur);                                                           \
    SG64_WRITE(nxt, wr, x0, x1, x2, x3);                                    \
    SG64_ISSUE_A((t) + 3, x0, x1, x2, x3);                                  \
    SG64_ISSUE_W((t) + 5, wr);                                              \
  } while (0)
  for (int t = 0; t < nstages; t += 4) {
    SG64_STAGE(t, buf0, buf1, w1, a10, a11, a12, a13);
    SG64_STAGE(t + 1, buf1, buf0, w2, a00, a01, a02, a03);
    if (TAIL && t + 2 >= nstages) break;
    SG64_STAGE(t + 2, buf0, buf1, w3, a10, a11, a12, a13);
    SG64_STAGE(t + 3, buf1, buf0, w0, a00, a01, a02, a03);
  }
#undef SG64_STAGE
#undef SG64_WRITE
#undef SG64_AST
#undef SG64_ISSUE_W
#undef SG64_ISSUE_A
#undef SG64_LD
#undef SG64_KB

  sg64_fold_store<MTW, SPLITS>(acc, lds.red[row_group], fmt, c, ws, M, N,
                               split, n_group << 6, row_group * MTW, k_slice,
                               lane);
}

}  // namespace
