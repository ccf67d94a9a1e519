// W8A16 skinny GEMM for decode-shape projections with FP8 weights (gfx950):
//   C[M,N] = A[M,K] x dq(W8)[N,K]^T,  dq(W8)[n,k] = e4m3(w8[n,k]) * 2^e[n]
// A bf16, W8 OCP e4m3fn bytes, e int8 [N] (one power-of-two exponent per
// output row, docs/FEATURES.md "FP8 weights"), f32 accumulate, bf16 out,
// 1 <= M <= 128, N % 64 == 0, K % (SPLITS * 256) == 0.
//
// Why: at decode batch sizes a projection is a weight stream (skinny_gemm.hip,
// ideal time = W bytes / HBM bandwidth), and e4m3 halves the bytes.  No
// library multiplies bf16 activations by fp8 weights, so this kernel serves
// EVERY N, the wide ones (qkv, gate_up) the bf16 path hands to hipBLASLt
// included.
//
// Geometry is skinny_gemm_wide_kernel's: a 64-column panel per workgroup,
// 8 waves = 2 k-slices x 4 row groups of MTW m-tiles (MTW = 1: M <= 64,
// MTW = 2: M <= 128), MTW x 4 accumulators per wave, v_mfma_f32_16x16x32_bf16.
// What differs:
//   stage = 128 k, not 64.  A 16-byte piece of W is then 16 k, a stage's W is
//           64 rows x 128 B = 512 pieces = ONE uint4 per thread, and 8 lanes
//           cover a contiguous 128-byte row segment: the HBM request shape of
//           the bf16 kernel.  (At 64 k the W loads would shrink to 8 B per
//           lane.)  A is 64 * MTW rows x 256 B = 2 * MTW uint4 per thread,
//           16 lanes per row.
//   cvt   = once per element, on the way INTO LDS: 16 bytes become two
//           16-byte bf16 pieces (v_cvt_scalef32_pk_bf16_fp8 at scale 1, exact
//           and the conversion the e4m3 attention kernels pin against torch).
//           LDS then holds what the bf16 kernel would hold for dq with e = 0,
//           and compute() is that kernel's, twice per stage.  Converting after
//           the fragment read instead would make each of the 4 row-group waves
//           convert the same W fragment.
//   LDS   = (64 + 64 MTW) rows x (128 + 8) bf16, double-buffered: 104 448 B at
//           MTW = 2, one workgroup per CU, as the wide kernel already runs.
//   pipe  = one barrier per stage; A (L2) two stages ahead in two named
//           register sets, W (HBM) in a ring of four named uint4 four to five
//           stages ahead, A issued before W in every stage (skinny_gemm.hip
//           has the reasons, and the three ways arrays of such registers
//           ended in scratch memory: every load set here is named scalars).
//           A split is an even number of stages, so the ring loop leaves
//           after a pair where the count is no multiple of 4.
//   scale = 2^e[n] multiplies the f32 sum once per output, in the epilogue,
//           before the bf16 store or the f32 partial store: exact.
//
// Bit contract: identical to skinny_gemm_kernel / skinny_gemm_wide_kernel on
// the bf16 tensor dq(W8) at equal (M, N, K, SPLITS).  Per output element
// chain c in {0, 1} accumulates the 32-k blocks with index = c (mod 2) in
// increasing k (k-slice c takes offsets c*32 and 64 + c*32 of each stage),
// the two chains are added in f32, and splits are folded in split order by
// the same reduce / norm kernels.  Scaling a row by 2^e commutes with every
// rounding on the way (|e| <= 64: nothing under- or overflows).
//
// No packed-fp32 VALU in this file's device code, and the runtime headers
// inside the region: attn_prefill_paged.hip has the reasons.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                               \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#include "common.h"
#include "launch.h"

namespace {

constexpr int W8_KSTAGE = 128;               // k per LDS stage
constexpr int W8_PITCH = W8_KSTAGE + 8;      // +8 bf16: bank-conflict pad
constexpr int W8_NT = 512;                   // threads (8 waves)

DEV_INLINE bf16x8 w8_frag(const __hip_bfloat16* p) {
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

// 2^e as f32 bits; |e| <= 64 keeps the exponent field normal
DEV_INLINE float w8_exp2i(int e) {
  return __uint_as_float((unsigned)(e + 127) << 23);
}

template <int MTW, int SPLITS>
__global__ __launch_bounds__(W8_NT) void skinny_gemm_w8_kernel(
    const __hip_bfloat16* __restrict__ a,   // [M, K]
    const uint8_t* __restrict__ w8,         // [N, K] e4m3
    const int8_t* __restrict__ wexp,        // [N]
    __hip_bfloat16* __restrict__ c,         // [M, N]   (SPLITS == 1)
    float* __restrict__ ws,                 // [SPLITS, M, N] (SPLITS > 1)
    const int M, const int N, const int K) {
  const int wg = (int)__builtin_amdgcn_workgroup_id_x();
  const int n_groups = N >> 6;
  const int n_group = wg % n_groups;
  const int split = wg / n_groups;
  const int tid = (int)__builtin_amdgcn_workitem_id_x();
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int gl = lane & 15;
  const int gslice = lane >> 4;

  const int row_group = wave & 3;            // MTW m-tiles each
  const int k_slice = wave >> 2;             // 0..1
  const int k_wg = K / SPLITS;
  const int k0 = split * k_wg;
  const int nstages = k_wg / W8_KSTAGE;      // even, >= 2 (host-side)

  constexpr int A_ROWS = MTW * 64;
  constexpr int BUF = (64 + A_ROWS) * W8_PITCH;
  __shared__ union {
    __hip_bfloat16 stage[2][BUF];
    float red[4][MTW * 4 * 256];
  } lds;

  // staging pieces of 16 B.  W: row tid >> 3, bytes (tid & 7) * 16, which are
  // also that row's k offsets.  A: piece s is row (tid >> 4) + 32 s, k offset
  // (tid & 15) * 8; rows past M - 1 re-read row M - 1 and are never stored.
  const int wrow = tid >> 3, wchk = (tid & 7) * 16;
  const int arow = tid >> 4, achk = (tid & 15) * 8;
  const uint8_t* wbase = w8 + (size_t)((n_group << 6) + wrow) * K + wchk;
#define W8_ABASE(s) (a + (size_t)min(arow + 32 * (s), M - 1) * K + achk)
  const __hip_bfloat16* ab0 = W8_ABASE(0);
  const __hip_bfloat16* ab1 = W8_ABASE(1);
  const __hip_bfloat16* ab2 = W8_ABASE(MTW > 1 ? 2 : 0);
  const __hip_bfloat16* ab3 = W8_ABASE(MTW > 1 ? 3 : 0);
#undef W8_ABASE

  uint4 w0, w1, w2, w3;
  uint4 a00, a01, a02 = {}, a03 = {};
  uint4 a10, a11, a12 = {}, a13 = {};

#define W8_KB(stage) (k0 + min(stage, nstages - 1) * W8_KSTAGE)
#define W8_LD(p, kb) (*reinterpret_cast<const uint4*>((p) + (kb)))
#define W8_ISSUE_A(stage, x0, x1, x2, x3)                                   \
  do {                                                                      \
    const int kb = W8_KB(stage);                                            \
    x0 = W8_LD(ab0, kb);                                                    \
    x1 = W8_LD(ab1, kb);                                                    \
    if (MTW > 1) {                                                          \
      x2 = W8_LD(ab2, kb);                                                  \
      x3 = W8_LD(ab3, kb);                                                  \
    }                                                                       \
  } while (0)
#define W8_ISSUE_W(stage, wr) wr = W8_LD(wbase, W8_KB(stage))
#define W8_AST(st, s)                                                       \
  reinterpret_cast<uint4*>(&st[(64 + arow + 32 * (s)) * W8_PITCH + achk])
#define W8_WRITE(st, wr, x0, x1, x2, x3)                                    \
  do {                                                                      \
    uint4 lo, hi;                                                           \
    w8_cvt16(wr, lo, hi);                                                   \
    *reinterpret_cast<uint4*>(&st[wrow * W8_PITCH + wchk]) = lo;            \
    *reinterpret_cast<uint4*>(&st[wrow * W8_PITCH + wchk + 8]) = hi;        \
    *W8_AST(st, 0) = x0;                                                    \
    *W8_AST(st, 1) = x1;                                                    \
    if (MTW > 1) {                                                          \
      *W8_AST(st, 2) = x2;                                                  \
      *W8_AST(st, 3) = x3;                                                  \
    }                                                                       \
  } while (0)

  f32x4 acc[MTW][4];
#pragma unroll
  for (int mt = 0; mt < MTW; ++mt)
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) acc[mt][nt] = {0.f, 0.f, 0.f, 0.f};

  // a stage is two 64-k sub-steps of the bf16 kernel's compute()
  const int kf = k_slice * 32 + gslice * 8;
  auto compute = [&](const __hip_bfloat16* st) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int kh = h * 64 + kf;
      const bf16x8 wf0 = w8_frag(&st[gl * W8_PITCH + kh]);
      const bf16x8 wf1 = w8_frag(&st[(16 + gl) * W8_PITCH + kh]);
      const bf16x8 wf2 = w8_frag(&st[(32 + gl) * W8_PITCH + kh]);
      const bf16x8 wf3 = w8_frag(&st[(48 + gl) * W8_PITCH + kh]);
#pragma unroll
      for (int mt = 0; mt < MTW; ++mt) {
        const bf16x8 af = w8_frag(
            &st[(64 + (row_group * MTW + mt) * 16 + gl) * W8_PITCH + kh]);
        acc[mt][0] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            af, wf0, acc[mt][0], 0, 0, 0);
        acc[mt][1] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            af, wf1, acc[mt][1], 0, 0, 0);
        acc[mt][2] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            af, wf2, acc[mt][2], 0, 0, 0);
        acc[mt][3] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
            af, wf3, acc[mt][3], 0, 0, 0);
      }
    }
  };

  __hip_bfloat16* buf0 = lds.stage[0];
  __hip_bfloat16* buf1 = lds.stage[1];

  // prologue: A stages 0,1 and W stages 0..3 in flight; stage 0 lands in
  // buffer 0 and its registers are re-issued.  Stage numbers past the last
  // are clamped to it (W8_KB): those loads stay inside the split's k range
  // and what they fetch is written to a buffer nobody reads again.
  W8_ISSUE_A(0, a00, a01, a02, a03);
  W8_ISSUE_W(0, w0);
  W8_ISSUE_A(1, a10, a11, a12, a13);
  W8_ISSUE_W(1, w1);
  W8_ISSUE_W(2, w2);
  W8_ISSUE_W(3, w3);
  W8_WRITE(buf0, w0, a00, a01, a02, a03);
  W8_ISSUE_A(2, a00, a01, a02, a03);
  W8_ISSUE_W(4, w0);

  // stage t: compute stage t, write stage t+1 (W ring slot (t+1)&3, A set
  // (t+1)&1) into the other buffer, re-issue those registers for A stage
  // t+3 and W stage t+5.  A buffer's previous stage was fully read before
  // the barrier, so one barrier per stage suffices
#define W8_STAGE(t, cur, nxt, wr, x0, x1, x2, x3)                           \
  do {                                                                      \
    __syncthreads();                                                        \
    compute(cur);                                                           \
    W8_WRITE(nxt, wr, x0, x1, x2, x3);                                      \
    W8_ISSUE_A((t) + 3, x0, x1, x2, x3);                                    \
    W8_ISSUE_W((t) + 5, wr);                                                \
  } while (0)
  for (int t = 0; t < nstages; t += 4) {
    W8_STAGE(t, buf0, buf1, w1, a10, a11, a12, a13);
    W8_STAGE(t + 1, buf1, buf0, w2, a00, a01, a02, a03);
    if (t + 2 >= nstages) break;
    W8_STAGE(t + 2, buf0, buf1, w3, a10, a11, a12, a13);
    W8_STAGE(t + 3, buf1, buf0, w0, a00, a01, a02, a03);
  }
#undef W8_STAGE
#undef W8_WRITE
#undef W8_AST
#undef W8_ISSUE_W
#undef W8_ISSUE_A
#undef W8_LD
#undef W8_KB

  // ---- fold the two k-slices: slice 1 -> LDS -> slice 0 adds, scales by
  // 2^e[n] and stores ------------------------------------------------------
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
          lds.red[row_group][(mt * 4 + nt) * 256 + r * 64 + lane] = u.e[r];
      }
  }
  __syncthreads();
  if (k_slice == 0) {
    // MFMA C layout: reg r of lane l is row 4*(l>>4)+r, column l&15
#pragma unroll
    for (int nt = 0; nt < 4; ++nt) {
      const int n = (n_group << 6) + (nt << 4) + gl;
      const float scale = w8_exp2i((int)wexp[n]);
#pragma unroll
      for (int mt = 0; mt < MTW; ++mt) {
        F32x4U u;
        u.v = acc[mt][nt];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float v =
              (u.e[r] +
               lds.red[row_group][(mt * 4 + nt) * 256 + r * 64 + lane]) *
              scale;
          const int m = (row_group * MTW + mt) * 16 + (gslice << 2) + r;
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
}

// bf16 [N, K] = e4m3(w8) * 2^e[row], for the shapes the GEMM above does not
// serve (M > 128: ops.linear hands the result to the library).  One 16-byte
// load and two 16-byte stores per piece of 16 k, grid-stride; the product
// with 2^e is exact in f32 and is a bf16 value (|e| <= 64), so keeping its
// high half rounds nothing.
__global__ __launch_bounds__(256) void w8_dequant_kernel(
    __hip_bfloat16* __restrict__ out,       // [N, K]
    const uint8_t* __restrict__ w8,         // [N, K]
    const int8_t* __restrict__ wexp,        // [N]
    const long pieces, const int pieces_per_row) {
  const long stride = (long)__builtin_amdgcn_grid_size_x();
  for (long i = (long)__builtin_amdgcn_workgroup_id_x() * 256 +
                (long)__builtin_amdgcn_workitem_id_x();
       i < pieces; i += stride) {
    const float scale = w8_exp2i((int)wexp[i / pieces_per_row]);
    const uint4 b = *reinterpret_cast<const uint4*>(w8 + i * 16);
    uint4 lo, hi;
    w8_cvt16(b, lo, hi);
    // two bf16 of one word, each widened, scaled and narrowed again
    auto scale2 = [&](unsigned p) {
      const float x = __uint_as_float(p << 16) * scale;
      const float y = __uint_as_float(p & 0xffff0000u) * scale;
      return (__float_as_uint(x) >> 16) | (__float_as_uint(y) & 0xffff0000u);
    };
    lo = make_uint4(scale2(lo.x), scale2(lo.y), scale2(lo.z), scale2(lo.w));
    hi = make_uint4(scale2(hi.x), scale2(hi.y), scale2(hi.z), scale2(hi.w));
    uint4* o = reinterpret_cast<uint4*>(out + i * 16);
    o[0] = lo;
    o[1] = hi;
  }
}

}  // namespace

extern "C" {

// One kernel per split count the GEMM is instantiated for.
#define LAUNCH_W8_SPLITS(MT)                                                 \
  switch (splits) {                                                          \
    case 1:                                                                  \
      skinny_gemm_w8_kernel<MT, 1><<<grid, block, 0, stream>>>(              \
          ap, wp, ep, cp, nullptr, M, N, K);                                 \
      break;                                                                 \
    case 2:                                                                  \
      skinny_gemm_w8_kernel<MT, 2><<<grid, block, 0, stream>>>(              \
          ap, wp, ep, cp, wsp, M, N, K);                                     \
      break;                                                                 \
    case 4:                                                                  \
      skinny_gemm_w8_kernel<MT, 4><<<grid, block, 0, stream>>>(              \
          ap, wp, ep, cp, wsp, M, N, K);                                     \
      break;                                                                 \
    case 8:                                                                  \
      skinny_gemm_w8_kernel<MT, 8><<<grid, block, 0, stream>>>(              \
          ap, wp, ep, cp, wsp, M, N, K);                                     \
      break;                                                                 \
    default:                                                                 \
      return hipErrorInvalidValue;                                           \
  }

hipError_t launch_skinny_gemm_w8(void* c, void* ws, const void* a,
                                 const void* w8, const void* e, int M, int N,
                                 int K, int splits, hipStream_t stream) {
  // the kernel indexes whole 64-column panels and an even number of 128-k
  // stages per split, and writes c or ws according to the split count
  if (M < 1 || M > 128 || N < 64 || N % 64 != 0 || splits < 1 || K < 1 ||
      K % (splits * 256) != 0 || (splits == 1 ? c == nullptr : ws == nullptr))
    return hipErrorInvalidValue;
  const dim3 grid((N >> 6) * splits), block(W8_NT);
  const __hip_bfloat16* ap = (const __hip_bfloat16*)a;
  const uint8_t* wp = (const uint8_t*)w8;
  const int8_t* ep = (const int8_t*)e;
  __hip_bfloat16* cp = (__hip_bfloat16*)c;
  float* wsp = (float*)ws;
  if (M <= 64) LAUNCH_W8_SPLITS(1)
  else LAUNCH_W8_SPLITS(2)
  return hipGetLastError();
}
#undef LAUNCH_W8_SPLITS

hipError_t launch_w8_dequant(void* out, const void* w8, const void* e, long N,
                             long K, hipStream_t stream) {
  if (N < 1 || K < 16 || K % 16 != 0 || K / 16 > INT32_MAX)
    return hipErrorInvalidValue;
  const long pieces = N * (K / 16);
  const long blocks = (pieces + 255) / 256;
  // 1024 blocks = 4 per CU: larger weights go round the grid-stride loop
  const dim3 grid((unsigned)(blocks < 1024 ? blocks : 1024)), block(256);
  w8_dequant_kernel<<<grid, block, 0, stream>>>(
      (__hip_bfloat16*)out, (const uint8_t*)w8, (const int8_t*)e, pieces,
      (int)(K / 16));
  return hipGetLastError();
}

}  // extern "C"

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
