// FP8 (OCP e4m3fn) paged KV cache: the quantising store and the dequantising
// gather (gfx950).  The dequantising decode kernel lives with its bf16
// siblings in attn_decode.hip.
//
// A cached element is q8(x) = sat_rne_e4m3fn(x * 2^-e) for the bf16 value x
// the bf16 engine would have cached, and reads back as e4m3(b) * 2^e
// (docs/FEATURES.md "FP8 KV cache").  Both scalings are by powers of two and
// therefore exact, so every reader agrees on what a cached value is.
#include "common.h"

namespace {

// Saturating round-to-nearest-even e4m3fn of four floats.  The clamp runs in
// fp32 BEFORE the conversion, so finite overflow and +-inf become +-448
// without relying on the instruction's own overflow behaviour; NaN passes
// the clamp untouched and converts to NaN.
DEV_INLINE float clamp_e4m3(float x) {
  const float c = fminf(fmaxf(x, -448.f), 448.f);
  return x != x ? x : c;
}

DEV_INLINE unsigned quant4_e4m3(float a, float b, float c, float d,
                                float inv_scale) {
  int w = 0;
  w = __builtin_amdgcn_cvt_pk_fp8_f32(clamp_e4m3(a * inv_scale),
                                      clamp_e4m3(b * inv_scale), w, false);
  w = __builtin_amdgcn_cvt_pk_fp8_f32(clamp_e4m3(c * inv_scale),
                                      clamp_e4m3(d * inv_scale), w, true);
  return (unsigned)w;
}

DEV_INLINE float bfbits2f(unsigned short b) {
  return __uint_as_float((unsigned)b << 16);
}

// 8 bf16 (one 16-byte vector) -> 8 e4m3 bytes
DEV_INLINE uint2 quant8_e4m3(const uint4& v, float inv_scale) {
  uint2 r;
  r.x = quant4_e4m3(bfbits2f(v.x & 0xffff), bfbits2f(v.x >> 16),
                    bfbits2f(v.y & 0xffff), bfbits2f(v.y >> 16), inv_scale);
  r.y = quant4_e4m3(bfbits2f(v.z & 0xffff), bfbits2f(v.z >> 16),
                    bfbits2f(v.w & 0xffff), bfbits2f(v.w >> 16), inv_scale);
  return r;
}

// grid.x = tokens; block = 256.  Q and K are rotated in place exactly as in
// rope_kv.hip; the cache receives bytes.  head_dim is 128 (host-checked).
__global__ void rope_store_kv_fp8_kernel(
    __hip_bfloat16* __restrict__ q,          // [T, QH*D]
    __hip_bfloat16* __restrict__ k,          // [T, KVH*D]
    const __hip_bfloat16* __restrict__ v,    // [T, KVH*D]
    uint8_t* __restrict__ key_cache,         // [pages, KVH, page, D] e4m3
    uint8_t* __restrict__ val_cache,
    const float* __restrict__ cos_sin,       // [max_pos, D] = [cos | sin]
    const int* __restrict__ positions,       // [T]
    const int* __restrict__ slot_mapping,    // [T] page*page_size+off; -1 skip
    const int num_q_heads, const int num_kv_heads, const int page_size,
    const int q_stride, const int kv_stride,
    const float k_inv_scale, const float v_inv_scale) {   // 2^-ek, 2^-ev
  constexpr int head_dim = 128, half = 64;
  const int token = blockIdx.x;
  const int tid = threadIdx.x;
  const int pos = positions[token];
  const int slot = slot_mapping[token];
  const float* cs = cos_sin + (size_t)pos * head_dim;

  // ---- rotate Q (same arithmetic as the bf16 kernel) ---------------------
  __hip_bfloat16* q_tok = q + (size_t)token * q_stride;
  const int q_pairs = num_q_heads * half;
  for (int i = tid; i < q_pairs; i += blockDim.x) {
    const int h = i / half, d = i % half;
    __hip_bfloat16* base = q_tok + h * head_dim;
    const float x1 = bf2f(base[d]), x2 = bf2f(base[d + half]);
    const float c = cs[d], s = cs[half + d];
    base[d] = f2bf(x1 * c - x2 * s);
    base[d + half] = f2bf(x2 * c + x1 * s);
  }

  // ---- rotate K four pairs per lane; the cache gets q8 of the ROUNDED
  // bf16 value, 4 bytes per store -----------------------------------------
  __hip_bfloat16* k_tok = k + (size_t)token * kv_stride;
  const __hip_bfloat16* v_tok = v + (size_t)token * kv_stride;
  const int page = slot >= 0 ? slot / page_size : 0;
  const int poff = slot >= 0 ? slot % page_size : 0;
  const int kv_quads = num_kv_heads * (half / 4);
  for (int i = tid; i < kv_quads; i += blockDim.x) {
    const int h = i / (half / 4), d = (i % (half / 4)) * 4;
    __hip_bfloat16* base = k_tok + h * head_dim;
    float r1[4], r2[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const float x1 = bf2f(base[d + j]), x2 = bf2f(base[d + j + half]);
      const float c = cs[d + j], s = cs[half + d + j];
      const __hip_bfloat16 b1 = f2bf(x1 * c - x2 * s);
      const __hip_bfloat16 b2 = f2bf(x2 * c + x1 * s);
      base[d + j] = b1;
      base[d + j + half] = b2;
      r1[j] = bf2f(b1);
      r2[j] = bf2f(b2);
    }
    if (slot >= 0) {
      uint8_t* kdst = key_cache +
          (((size_t)page * num_kv_heads + h) * page_size + poff) * head_dim;
      *reinterpret_cast<unsigned*>(kdst + d) =
          quant4_e4m3(r1[0], r1[1], r1[2], r1[3], k_inv_scale);
      *reinterpret_cast<unsigned*>(kdst + d + half) =
          quant4_e4m3(r2[0], r2[1], r2[2], r2[3], k_inv_scale);
    }
  }
  if (slot >= 0) {
    // V: 16 bf16 in (two 16-byte loads), one 16-byte store of bytes per lane
    const int nvec = num_kv_heads * head_dim / 16;
    for (int i = tid; i < nvec; i += blockDim.x) {
      const int h = (i * 16) / head_dim;
      const int d = (i * 16) % head_dim;
      const uint4 a =
          *reinterpret_cast<const uint4*>(v_tok + h * head_dim + d);
      const uint4 b =
          *reinterpret_cast<const uint4*>(v_tok + h * head_dim + d + 8);
      const uint2 qa = quant8_e4m3(a, v_inv_scale);
      const uint2 qb = quant8_e4m3(b, v_inv_scale);
      uint8_t* vdst = val_cache +
          (((size_t)page * num_kv_heads + h) * page_size + poff) * head_dim;
      *reinterpret_cast<uint4*>(vdst + d) = make_uint4(qa.x, qa.y, qb.x, qb.y);
    }
  }
}

// e4m3 * 2^e as bf16: the conversion and the power-of-two multiply are exact
// in fp32 and the product keeps its four significant bits, so the high half
// of the f32 IS the bf16.
DEV_INLINE uint2 dequant4_bf16(unsigned w, float scale) {
  const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(w, false);
  const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8(w, true);
  uint2 r;
  r.x = (__float_as_uint(lo.x * scale) >> 16) |
        (__float_as_uint(lo.y * scale) & 0xffff0000u);
  r.y = (__float_as_uint(hi.x * scale) >> 16) |
        (__float_as_uint(hi.y * scale) & 0xffff0000u);
  return r;
}

// out[t, h, :] = dq(cache[page(t), h, off(t), :]).  One lane per 16 bytes of
// a 128-byte row: a 16-byte load, two 16-byte stores.
__global__ void kv_gather_dequant_kernel(
    __hip_bfloat16* __restrict__ out,        // [Tkv, KVH, 128]
    const uint8_t* __restrict__ cache,       // [pages, KVH, page, 128] e4m3
    const int* __restrict__ slots,           // [Tkv]
    const long total_vecs,                   // Tkv * KVH * 8
    const int num_slots,                     // pages * page_size
    const int num_kv_heads, const int page_size, const float scale) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total_vecs) return;
  const int c = (int)(i & 7);
  const long row = i >> 3;
  const int h = (int)(row % num_kv_heads);
  const long t = row / num_kv_heads;
  const int slot = slots[t];
  uint4* dst = reinterpret_cast<uint4*>(out + row * 128 + c * 16);
  if (slot < 0 || slot >= num_slots) {       // never read outside the pool
    dst[0] = make_uint4(0, 0, 0, 0);
    dst[1] = make_uint4(0, 0, 0, 0);
    return;
  }
  const int page = slot / page_size, poff = slot % page_size;
  const uint8_t* src = cache + c * 16 +
      (((size_t)page * num_kv_heads + h) * page_size + poff) * 128;
  const uint4 b = *reinterpret_cast<const uint4*>(src);
  const uint2 a0 = dequant4_bf16(b.x, scale), a1 = dequant4_bf16(b.y, scale);
  const uint2 a2 = dequant4_bf16(b.z, scale), a3 = dequant4_bf16(b.w, scale);
  dst[0] = make_uint4(a0.x, a0.y, a1.x, a1.y);
  dst[1] = make_uint4(a2.x, a2.y, a3.x, a3.y);
}

}  // namespace

extern "C" {

void launch_rope_store_kv_fp8(void* q, void* k, const void* v, void* key_cache,
                              void* val_cache, const void* cos_sin,
                              const void* positions, const void* slot_mapping,
                              int tokens, int num_q_heads, int num_kv_heads,
                              int page_size, int q_stride, int kv_stride,
                              float k_inv_scale, float v_inv_scale,
                              hipStream_t stream) {
  hipLaunchKernelGGL(rope_store_kv_fp8_kernel, dim3(tokens), dim3(256), 0,
                     stream, (__hip_bfloat16*)q, (__hip_bfloat16*)k,
                     (const __hip_bfloat16*)v, (uint8_t*)key_cache,
                     (uint8_t*)val_cache, (const float*)cos_sin,
                     (const int*)positions, (const int*)slot_mapping,
                     num_q_heads, num_kv_heads, page_size, q_stride,
                     kv_stride, k_inv_scale, v_inv_scale);
}

void launch_kv_gather_dequant(void* out, const void* cache, const void* slots,
                              long tokens, int num_slots, int num_kv_heads,
                              int page_size, float scale,
                              hipStream_t stream) {
  const long total = tokens * num_kv_heads * 8;
  const int block = 256;
  const long grid = (total + block - 1) / block;
  hipLaunchKernelGGL(kv_gather_dequant_kernel, dim3((unsigned)grid),
                     dim3(block), 0, stream, (__hip_bfloat16*)out,
                     (const uint8_t*)cache, (const int*)slots, total,
                     num_slots, num_kv_heads, page_size, scale);
}

}  // extern "C"
