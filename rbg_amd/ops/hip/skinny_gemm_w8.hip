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
// The kernel is skinny_gemm_tile.h's 64-column-panel kernel (geometry, pipeline
// and epilogue are stated there) with the W8Weights format below:
//   stage = 128 k, not 64.  A 16-byte piece of W is then 16 k, a stage's W is
//           64 rows x 128 B = 512 pieces = ONE uint4 per thread, and 8 lanes
//           cover a contiguous 128-byte row segment: the HBM request shape of
//           the bf16 kernel.  (At 64 k the W loads would shrink to 8 B per
//           lane.)  A is 64 * MTW rows x 256 B = 2 * MTW uint4 per thread,
//           16 lanes per row.
//   cvt   = once per element, on the way INTO LDS: 16 bytes become two
//           16-byte bf16 pieces (v_cvt_scalef32_pk_bf16_fp8 at scale 1, exact
//           and the conversion the e4m3 attention kernels pin against torch).
//           LDS then holds what the bf16 instantiation would hold for dq with
//           e = 0, and a stage is two of its 64-k MFMA sub-steps.  Converting
//           after the fragment read instead would make each of the 4 row-group
//           waves convert the same W fragment.
//   LDS   = (64 + 64 MTW) rows x (128 + 8) bf16, double-buffered: 104 448 B at
//           MTW = 2, one workgroup per CU, as the bf16 instantiation already
//           runs.
//   pipe  = a split is an even number of stages, so the ring loop leaves
//           after a pair where the count is no multiple of 4.
//   scale = 2^e[n] multiplies the f32 sum once per output, in the epilogue,
//           before the bf16 store or the f32 partial store: exact.
//
// Bit contract: the shared kernel's, on the bf16 tensor dq(W8).  Scaling a row
// by 2^e commutes with every rounding on the way (|e| <= 64: nothing under-
// or overflows).
//
// No packed-fp32 VALU in this file's device code, and the runtime headers
// inside the region: attn_prefill_paged.hip has the reasons.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(                                               \
    __attribute__((target("no-packed-fp32-ops"))), apply_to = function)
#endif

#include "skinny_gemm_tile.h"
#include "launch.h"

namespace {

// (w8_cvt4 / w8_cvt16 / w8_exp2i: skinny_gemm_tile.h, shared with moe.hip)

// e4m3 weights for the 64-column kernel (skinny_gemm_tile.h): 128-k stages, a
// W register is 16 e4m3 bytes and goes to LDS as two bf16 pieces, column n's
// sum is multiplied by 2^e[n].
struct W8Weights {
  typedef uint8_t W;
  static constexpr int KSTAGE = 128;
  static constexpr bool SCALED = true;
  const int8_t* wexp;                        // [N]
  static DEV_INLINE void stage_w(__hip_bfloat16* dst, const uint4& r) {
    uint4 lo, hi;
    w8_cvt16(r, lo, hi);
    *reinterpret_cast<uint4*>(dst) = lo;
    *reinterpret_cast<uint4*>(dst + 8) = hi;
  }
  DEV_INLINE float col_scale(int n) const { return w8_exp2i((int)wexp[n]); }
};

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

hipError_t launch_skinny_gemm_w8(void* c, void* ws, const void* a,
                                 const void* w8, const void* e, int M, int N,
                                 int K, int splits, hipStream_t stream) {
  // the kernel indexes whole 64-column panels and an even number of 128-k
  // stages per split, and writes c or ws according to the split count
  if (M < 1 || M > 128 || N < 64 || N % 64 != 0 || splits < 1 || K < 1 ||
      K % (splits * 256) != 0 || (splits == 1 ? c == nullptr : ws == nullptr))
    return hipErrorInvalidValue;
  const dim3 grid((N >> 6) * splits), block(SG64_NT);
  const __hip_bfloat16* ap = (const __hip_bfloat16*)a;
  const uint8_t* wp = (const uint8_t*)w8;
  __hip_bfloat16* cp = (__hip_bfloat16*)c;
  float* wsp = (float*)ws;
  const W8Weights fmt = {(const int8_t*)e};
  if (M <= 64)
    LAUNCH_SPLITS(skinny_gemm64_kernel, 1, ap, wp, fmt, cp, wsp, M, N, K)
  else
    LAUNCH_SPLITS(skinny_gemm64_kernel, 2, ap, wp, fmt, cp, wsp, M, N, K)
  return hipGetLastError();
}

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
