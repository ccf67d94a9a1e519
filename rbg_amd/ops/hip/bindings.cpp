// PyTorch bindings for the rbg_amd CDNA4 HIP kernels.
// Shape/dtype checks here; all math lives in the .hip translation units,
// whose launchers are declared in launch.h and nowhere else.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "launch.h"

// Calls a launcher of launch.h; an error it returns (no kernel for the
// arguments, or a failed launch) raises RuntimeError.
#define LAUNCH(launcher, ...)                                               \
  do {                                                                      \
    const hipError_t launch_err_ = launcher(__VA_ARGS__);                   \
    TORCH_CHECK(launch_err_ == hipSuccess, #launcher, " failed: ",          \
                hipGetErrorString(launch_err_));                            \
  } while (0)

namespace {

hipStream_t current_stream() {
  return at::hip::getCurrentHIPStream().stream();
}

void check_bf16_contig(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, name, " must be bf16");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

void check_i32_gpu(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.scalar_type() == torch::kInt32, name, " must be int32");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

// bf16 on GPU, [T, H, D] with contiguous (H, D) rows, or [T, W] where
// allow_2d; the TOKEN stride may be wider (a column slice of the fused QKV
// buffer).
void check_bf16_rowslice(const torch::Tensor& t, const char* name,
                         bool allow_2d = false) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, name, " must be bf16");
  if (allow_2d && t.dim() == 2) {
    TORCH_CHECK(t.stride(1) == 1, name, " rows must be contiguous");
  } else {
    TORCH_CHECK(t.dim() == 3 && t.stride(2) == 1 &&
                t.stride(1) == t.size(2), name,
                " must be [T, H, D] with contiguous (H, D) rows");
  }
}

// One paged KV pool view [pages, KVH, page_size, head_dim] of bf16 or e4m3:
// the kernels index it densely with a power-of-two page (shift/mask slot
// math) and 16-byte row vectors, so anything else must raise instead of
// launching.
void check_kv_cache(const torch::Tensor& t, const char* name,
                    torch::ScalarType dtype) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.scalar_type() == dtype, name, " must be ",
              dtype == torch::kBFloat16 ? "bf16" : "float8_e4m3fn");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.dim() == 4, name,
              " must be [pages, KVH, page_size, head_dim]");
  const int64_t page_size = t.size(2);
  TORCH_CHECK(page_size > 0 && (page_size & (page_size - 1)) == 0,
              "page_size must be a power of two");
  TORCH_CHECK(t.size(1) > 0, "cache needs at least one KV head");
  if (dtype == torch::kBFloat16) {
    TORCH_CHECK(t.size(3) > 0 && t.size(3) % 8 == 0,
                "cache head_dim must be a multiple of 8");
  } else {
    TORCH_CHECK(t.size(3) == 128, "fp8 cache head_dim must be 128");
  }
  // slots and rows reach the kernels as int32.  (The bf16 kernels widen to
  // size_t before they multiply, and 2^31 bf16 rows exceed the HBM anyway:
  // for them the check is only there to be the same one.)
  TORCH_CHECK(t.numel() / t.size(3) <= INT32_MAX, "cache has too many slots");
}

void check_kv_caches(const torch::Tensor& key_cache,
                     const torch::Tensor& value_cache,
                     torch::ScalarType dtype) {
  check_kv_cache(key_cache, "key_cache", dtype);
  check_kv_cache(value_cache, "value_cache", dtype);
  TORCH_CHECK(value_cache.sizes() == key_cache.sizes(),
              "key_cache/value_cache shape mismatch");
  TORCH_CHECK(value_cache.device() == key_cache.device(),
              "key_cache/value_cache device mismatch");
}

// Shared by both norms: the kernels read weight[0 .. hidden) as 16-byte
// vectors, so a short, strided or non-bf16 weight must raise here.
int check_norm_args(const torch::Tensor& x, const torch::Tensor& weight) {
  check_bf16_contig(x, "x");
  check_bf16_contig(weight, "weight");
  TORCH_CHECK(x.dim() >= 1, "x must have a hidden dimension");
  const int64_t hidden = x.size(-1);
  TORCH_CHECK(hidden > 0 && hidden % 8 == 0,
              "hidden must be a positive multiple of 8");
  TORCH_CHECK(weight.numel() == hidden, "weight must have hidden elements");
  TORCH_CHECK(weight.device() == x.device(), "x/weight device mismatch");
  return (int)hidden;
}

torch::Tensor rmsnorm(torch::Tensor x, torch::Tensor weight, double eps) {
  const int hidden = check_norm_args(x, weight);
  const int tokens = x.numel() / hidden;
  auto out = torch::empty_like(x);
  if (tokens == 0) return out;
  LAUNCH(launch_rmsnorm, out.data_ptr(), x.data_ptr(), weight.data_ptr(),
         (float)eps, tokens, hidden, current_stream());
  return out;
}

void fused_add_rmsnorm(torch::Tensor x, torch::Tensor residual,
                       torch::Tensor weight, double eps) {
  const int hidden = check_norm_args(x, weight);
  check_bf16_contig(residual, "residual");
  TORCH_CHECK(residual.sizes() == x.sizes(), "x/residual shape mismatch");
  TORCH_CHECK(residual.device() == x.device(), "x/residual device mismatch");
  const int tokens = x.numel() / hidden;
  if (tokens == 0) return;
  LAUNCH(launch_fused_add_rmsnorm, x.data_ptr(), residual.data_ptr(),
         weight.data_ptr(), (float)eps, tokens, hidden, current_stream());
}

torch::Tensor silu_mul(torch::Tensor x) {
  check_bf16_contig(x, "x");
  TORCH_CHECK(x.dim() >= 1, "x must be [..., 2*inter]");
  const int inter2 = x.size(-1);
  TORCH_CHECK(inter2 > 0 && inter2 % 16 == 0,
              "2*inter must be a positive multiple of 16");
  const int inter = inter2 / 2;
  const int tokens = x.numel() / inter2;
  // the kernel writes numel / (2*inter) rows: keep every leading dimension
  auto out_sizes = x.sizes().vec();
  out_sizes.back() = inter;
  auto out = torch::empty(out_sizes, x.options());
  if (tokens == 0) return out;
  LAUNCH(launch_silu_mul, out.data_ptr(), x.data_ptr(), tokens, inter,
         current_stream());
  return out;
}

// Scales of the e4m3 cache are powers of two given as integer exponents.
float check_scale_log2(int64_t e, const char* name) {
  TORCH_CHECK(e >= -16 && e <= 16, name, " must be in [-16, 16], got ", e);
  return std::ldexp(1.0f, (int)e);
}

// Everything rope_store_kv checks and passes on for either cache dtype; the
// e4m3 binding adds its scales.
RopeStoreLaunch rope_store_args(const torch::Tensor& q, const torch::Tensor& k,
                                const torch::Tensor& v,
                                const torch::Tensor& key_cache,
                                const torch::Tensor& value_cache,
                                torch::ScalarType cache_dtype,
                                const torch::Tensor& cos_sin,
                                const torch::Tensor& positions,
                                const torch::Tensor& slot_mapping) {
  check_bf16_rowslice(q, "q", true);
  check_bf16_rowslice(k, "k", true);
  check_bf16_rowslice(v, "v", true);
  TORCH_CHECK(k.stride(0) == v.stride(0), "k/v stride mismatch");
  check_kv_caches(key_cache, value_cache, cache_dtype);
  check_i32_gpu(positions, "positions");
  check_i32_gpu(slot_mapping, "slot_mapping");
  TORCH_CHECK(cos_sin.scalar_type() == torch::kFloat32 && cos_sin.is_cuda() &&
              cos_sin.is_contiguous() && cos_sin.dim() == 2,
              "cos_sin must be a contiguous 2-D fp32 GPU tensor");
  const int64_t tokens = q.size(0);
  const int64_t head_dim = key_cache.size(3);
  const int64_t num_kv_heads = key_cache.size(1);
  TORCH_CHECK(cos_sin.size(1) == head_dim,
              "cos_sin row width must equal the cache head_dim");
  TORCH_CHECK(k.size(0) == tokens && v.size(0) == tokens &&
              positions.numel() == tokens && slot_mapping.numel() == tokens,
              "q/k/v/positions/slot_mapping token counts differ");
  const int64_t q_width = q.numel() / std::max<int64_t>(tokens, 1);
  const int64_t k_width = k.numel() / std::max<int64_t>(tokens, 1);
  const int64_t v_width = v.numel() / std::max<int64_t>(tokens, 1);
  TORCH_CHECK(k_width == num_kv_heads * head_dim && v_width == k_width,
              "k/v rows must be cache KVH * head_dim wide");
  TORCH_CHECK(q_width % head_dim == 0,
              "q row width must be a multiple of the cache head_dim");
  // both kernels read V rows as 16-byte vectors
  TORCH_CHECK(reinterpret_cast<uintptr_t>(v.data_ptr()) % 16 == 0 &&
              v.stride(0) % 8 == 0, "v rows must be 16-byte aligned");
  RopeStoreLaunch a;
  a.q = q.data_ptr();
  a.k = k.data_ptr();
  a.v = v.data_ptr();
  a.key_cache = key_cache.data_ptr();
  a.val_cache = value_cache.data_ptr();
  a.cos_sin = cos_sin.data_ptr();
  a.positions = positions.data_ptr();
  a.slot_mapping = slot_mapping.data_ptr();
  a.tokens = (int)tokens;
  a.num_q_heads = (int)(q_width / head_dim);
  a.num_kv_heads = (int)num_kv_heads;
  a.head_dim = (int)head_dim;
  a.page_size = (int)key_cache.size(2);
  a.q_stride = (int)q.stride(0);
  a.kv_stride = (int)k.stride(0);
  a.k_inv_scale = 1.f;
  a.v_inv_scale = 1.f;
  return a;
}

void rope_store_kv(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                   torch::Tensor key_cache, torch::Tensor value_cache,
                   torch::Tensor cos_sin, torch::Tensor positions,
                   torch::Tensor slot_mapping) {
  const RopeStoreLaunch a =
      rope_store_args(q, k, v, key_cache, value_cache, torch::kBFloat16,
                      cos_sin, positions, slot_mapping);
  if (a.tokens == 0) return;
  LAUNCH(launch_rope_store_kv, a, current_stream());
}

// ---- FP8 (OCP e4m3fn) paged KV cache --------------------------------------
// Separate entry points: the bf16 ones keep rejecting every non-bf16 cache.

void rope_store_kv_fp8(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                       torch::Tensor key_cache, torch::Tensor value_cache,
                       torch::Tensor cos_sin, torch::Tensor positions,
                       torch::Tensor slot_mapping, int64_t k_scale_log2,
                       int64_t v_scale_log2) {
  RopeStoreLaunch a =
      rope_store_args(q, k, v, key_cache, value_cache, torch::kFloat8_e4m3fn,
                      cos_sin, positions, slot_mapping);
  a.k_inv_scale = check_scale_log2(-k_scale_log2, "kv_k_scale_log2");
  a.v_inv_scale = check_scale_log2(-v_scale_log2, "kv_v_scale_log2");
  if (a.tokens == 0) return;
  LAUNCH(launch_rope_store_kv_fp8, a, current_stream());
}

torch::Tensor kv_gather_dequant(torch::Tensor cache, torch::Tensor slots,
                                int64_t scale_log2) {
  check_kv_cache(cache, "cache", torch::kFloat8_e4m3fn);
  check_i32_gpu(slots, "slots");
  TORCH_CHECK(slots.dim() == 1 && slots.device() == cache.device(),
              "slots must be 1-D on the cache's device");
  const float scale = check_scale_log2(scale_log2, "scale_log2");
  const int64_t tokens = slots.numel();
  const int num_kv_heads = cache.size(1);
  auto out = torch::empty({tokens, (int64_t)num_kv_heads, (int64_t)128},
                          cache.options().dtype(torch::kBFloat16));
  if (tokens == 0) return out;
  LAUNCH(launch_kv_gather_dequant, out.data_ptr(), cache.data_ptr(),
         slots.data_ptr(), (long)tokens,
         (int)(cache.numel() / 128 / num_kv_heads), num_kv_heads,
         (int)cache.size(2), scale, current_stream());
  return out;
}

// How the partials of num_splits > 1 are merged.  combine 0: inside the
// workgroup where a kernel for it exists (the page-pair MFMA kernels at 2 or
// 4 splits), else by decode_combine_kernel; 1: always the separate kernel;
// 2: inside the workgroup, raising where that is not possible.
bool pick_in_wg_combine(int64_t combine, int64_t num_splits, bool mfma_pair,
                        const char* what) {
  TORCH_CHECK(combine >= 0 && combine <= 2,
              "combine must be 0 (auto), 1 (kernel) or 2 (in-workgroup)");
  // the in-workgroup kernels run exactly WS = num_splits splits and get no
  // partial buffers: never hand them another count
  const bool can = mfma_pair && (num_splits == 2 || num_splits == 4);
  TORCH_CHECK(combine != 2 || can, "combine = 2 needs ", what,
              ", a page size of 16 and 2 or 4 splits");
  return combine != 1 && can;
}

// What both decode bindings check, derive and allocate.  The launch struct
// comes back complete but for the scale.
struct DecodeGeometry {
  DecodeLaunch launch;
  int page_size;
  torch::Tensor out, partial_o, partial_ml;
};

// pair_variant: the caller's kernel is a page-pair MFMA one wherever the
// page size is 16 (variant 4, or the e4m3 kernel, named by `what`).
DecodeGeometry decode_geometry(const torch::Tensor& q,
                               const torch::Tensor& key_cache,
                               const torch::Tensor& value_cache,
                               torch::ScalarType cache_dtype,
                               const torch::Tensor& block_tables,
                               const torch::Tensor& context_lens,
                               int64_t num_splits, int64_t combine,
                               bool pair_variant, const char* what) {
  // q may be a slice of the fused QKV projection
  check_bf16_rowslice(q, "q");
  const int64_t num_seqs = q.size(0), num_q_heads = q.size(1);
  TORCH_CHECK(q.size(2) == 128, "head_dim must be 128");
  check_kv_caches(key_cache, value_cache, cache_dtype);
  TORCH_CHECK(key_cache.size(3) == 128, "cache head_dim must be 128");
  const int64_t num_kv_heads = key_cache.size(1);
  TORCH_CHECK(num_q_heads % num_kv_heads == 0,
              "q heads must be a multiple of the cache KV heads");
  const int64_t qpg = num_q_heads / num_kv_heads;
  TORCH_CHECK(qpg == 1 || qpg == 2 || qpg == 4 || qpg == 8,
              "GQA group must be 1/2/4/8");
  check_i32_gpu(block_tables, "block_tables");
  check_i32_gpu(context_lens, "context_lens");
  TORCH_CHECK(block_tables.dim() == 2 && block_tables.size(0) == num_seqs,
              "block_tables must be [num_seqs, max_pages]");
  TORCH_CHECK(context_lens.dim() == 1 && context_lens.size(0) == num_seqs,
              "context_lens must be [num_seqs]");
  TORCH_CHECK(num_splits >= 1, "num_splits must be >= 1");
  DecodeGeometry g;
  g.page_size = (int)key_cache.size(2);
  const bool in_wg = pick_in_wg_combine(
      combine, num_splits, pair_variant && g.page_size == 16, what);
  g.out = torch::empty({num_seqs, num_q_heads, 128}, q.options());
  if (num_splits > 1 && !in_wg) {
    auto opts = q.options().dtype(torch::kFloat32);
    g.partial_o = torch::empty({num_splits, num_seqs, num_q_heads, 128}, opts);
    g.partial_ml = torch::empty({num_splits, num_seqs, num_q_heads, 2}, opts);
  }
  DecodeLaunch& a = g.launch;
  a.out = g.out.data_ptr();
  a.partial_o = g.partial_o.defined() ? g.partial_o.data_ptr() : nullptr;
  a.partial_ml = g.partial_ml.defined() ? g.partial_ml.data_ptr() : nullptr;
  a.q = q.data_ptr();
  a.key_cache = key_cache.data_ptr();
  a.val_cache = value_cache.data_ptr();
  a.block_tables = block_tables.data_ptr();
  a.context_lens = context_lens.data_ptr();
  a.scale = 0.f;
  a.num_seqs = (int)num_seqs;
  a.num_q_heads = (int)num_q_heads;
  a.num_kv_heads = (int)num_kv_heads;
  a.max_pages = (int)block_tables.size(1);
  a.num_splits = (int)num_splits;
  a.q_stride = (int)q.stride(0);
  a.in_wg = in_wg;
  return g;
}

torch::Tensor decode_attention(torch::Tensor q, torch::Tensor key_cache,
                               torch::Tensor value_cache,
                               torch::Tensor block_tables,
                               torch::Tensor context_lens, double scale,
                               int64_t num_splits, int64_t variant,
                               int64_t combine = 0) {
  DecodeGeometry g = decode_geometry(q, key_cache, value_cache,
                                     torch::kBFloat16, block_tables,
                                     context_lens, num_splits, combine,
                                     variant == 4, "variant 4");
  if (g.launch.num_seqs == 0) return g.out;
  g.launch.scale = (float)scale;
  LAUNCH(launch_decode_attention, g.launch, g.page_size, (int)variant,
         current_stream());
  return g.out;
}

torch::Tensor decode_attention_fp8(torch::Tensor q, torch::Tensor key_cache,
                                   torch::Tensor value_cache,
                                   torch::Tensor block_tables,
                                   torch::Tensor context_lens, double scale,
                                   int64_t num_splits, int64_t k_scale_log2,
                                   int64_t v_scale_log2,
                                   int64_t combine = 0) {
  DecodeGeometry g = decode_geometry(q, key_cache, value_cache,
                                     torch::kFloat8_e4m3fn, block_tables,
                                     context_lens, num_splits, combine, true,
                                     "the fp8 kernel");
  TORCH_CHECK(g.page_size == 16, "fp8 decode needs a page size of 16");
  const float k_scale = check_scale_log2(k_scale_log2, "kv_k_scale_log2");
  const float v_scale = check_scale_log2(v_scale_log2, "kv_v_scale_log2");
  if (g.launch.num_seqs == 0) return g.out;
  // 2^ek folds into the score scale: a power of two, so the product is exact
  g.launch.scale = (float)scale * k_scale;
  LAUNCH(launch_decode_attention_fp8, g.launch, v_scale, current_stream());
  return g.out;
}

torch::Tensor prefill_attention(torch::Tensor q, torch::Tensor k,
                                torch::Tensor v, torch::Tensor block_info,
                                torch::Tensor seq_lens, double scale,
                                int64_t swz) {
  check_bf16_rowslice(q, "q");
  check_bf16_rowslice(k, "k");
  check_bf16_rowslice(v, "v");
  TORCH_CHECK(k.device() == q.device() && v.device() == q.device(),
              "q/k/v device mismatch");
  TORCH_CHECK(k.sizes() == v.sizes(), "k/v shape mismatch");
  TORCH_CHECK(k.stride(0) == v.stride(0), "k/v stride mismatch");
  TORCH_CHECK(q.size(2) == 128 && k.size(2) == 128, "head_dim must be 128");
  const int64_t num_q_heads = q.size(1), num_kv_heads = k.size(1);
  TORCH_CHECK(num_kv_heads >= 1 && num_q_heads % num_kv_heads == 0,
              "q heads must be a multiple of the (>= 1) KV heads");
  // reference.prefill_block_info: one row of 4 and one KV length per block
  check_i32_gpu(block_info, "block_info");
  check_i32_gpu(seq_lens, "seq_lens");
  TORCH_CHECK(block_info.device() == q.device() &&
              seq_lens.device() == q.device(),
              "block_info and seq_lens must be on q's device");
  TORCH_CHECK(block_info.dim() == 2 && block_info.size(1) == 4,
              "block_info must be [nblocks, 4]");
  const int64_t nblocks = block_info.size(0);
  TORCH_CHECK(seq_lens.dim() == 1 && seq_lens.size(0) == nblocks,
              "seq_lens must be [nblocks]");
  // the grid is one workgroup per (block, q head)
  TORCH_CHECK(nblocks * num_q_heads <= INT32_MAX, "too many blocks");
  auto out = torch::empty({q.size(0), num_q_heads, 128}, q.options());
  if (q.size(0) == 0 || nblocks == 0) return out;
  PrefillLaunch a;
  a.out = out.data_ptr();
  a.q = q.data_ptr();
  a.k = k.data_ptr();
  a.v = v.data_ptr();
  a.block_info = block_info.data_ptr();
  a.seq_lens = seq_lens.data_ptr();
  a.scale = (float)scale;
  a.nblocks = (int)nblocks;
  a.num_q_heads = (int)num_q_heads;
  a.num_kv_heads = (int)num_kv_heads;
  a.swz = (int)swz;
  a.q_stride = (int)q.stride(0);
  a.kv_stride = (int)k.stride(0);
  LAUNCH(launch_prefill_attention, a, current_stream());
  return out;
}

// Prefill over the paged pool itself (attn_prefill_paged.hip).  block_info and
// seq_lens are reference.prefill_block_info_paged's map (qtile 128): the
// caller vouches that every sequence index is a row of block_tables and that
// the table is ceil(seq_len / 16) columns wide (ops.prefill_attention_paged
// checks both on the host); the exponents are ignored for a bf16 pool.
torch::Tensor prefill_attention_paged(torch::Tensor q, torch::Tensor key_cache,
                                      torch::Tensor value_cache,
                                      torch::Tensor block_tables,
                                      torch::Tensor block_info,
                                      torch::Tensor seq_lens, double scale,
                                      int64_t k_scale_log2,
                                      int64_t v_scale_log2) {
  check_bf16_rowslice(q, "q");
  TORCH_CHECK(q.size(2) == 128, "head_dim must be 128");
  const auto cache_dtype = key_cache.scalar_type();
  TORCH_CHECK(cache_dtype == torch::kBFloat16 ||
                  cache_dtype == torch::kFloat8_e4m3fn,
              "key_cache must be bf16 or float8_e4m3fn");
  const bool fp8 = cache_dtype == torch::kFloat8_e4m3fn;
  check_kv_caches(key_cache, value_cache, cache_dtype);
  TORCH_CHECK(key_cache.device() == q.device(), "q/cache device mismatch");
  TORCH_CHECK(key_cache.size(2) == 16 && key_cache.size(3) == 128,
              "paged prefill needs a page size of 16 and head_dim 128");
  const int64_t num_q_heads = q.size(1), num_kv_heads = key_cache.size(1);
  TORCH_CHECK(num_kv_heads >= 1 && num_q_heads % num_kv_heads == 0,
              "q heads must be a multiple of the (>= 1) KV heads");
  check_i32_gpu(block_tables, "block_tables");
  check_i32_gpu(block_info, "block_info");
  check_i32_gpu(seq_lens, "seq_lens");
  TORCH_CHECK(block_tables.device() == q.device() &&
                  block_info.device() == q.device() &&
                  seq_lens.device() == q.device(),
              "block_tables, block_info and seq_lens must be on q's device");
  TORCH_CHECK(block_tables.dim() == 2,
              "block_tables must be [num_seqs, max_pages]");
  TORCH_CHECK(block_info.dim() == 2 && block_info.size(1) == 4,
              "block_info must be [nblocks, 4]");
  const int64_t nblocks = block_info.size(0);
  TORCH_CHECK(seq_lens.dim() == 1 && seq_lens.size(0) == nblocks,
              "seq_lens must be [nblocks]");
  TORCH_CHECK(nblocks * num_q_heads <= INT32_MAX, "too many blocks");
  const float k_scale =
      fp8 ? check_scale_log2(k_scale_log2, "kv_k_scale_log2") : 1.f;
  const float v_scale =
      fp8 ? check_scale_log2(v_scale_log2, "kv_v_scale_log2") : 1.f;
  auto out = torch::empty({q.size(0), num_q_heads, 128}, q.options());
  if (q.size(0) == 0 || nblocks == 0) return out;
  TORCH_CHECK(block_tables.size(0) >= 1 && block_tables.size(1) >= 1,
              "block_tables is empty but there are blocks to run");
  PrefillPagedLaunch a;
  a.out = out.data_ptr();
  a.q = q.data_ptr();
  a.key_cache = key_cache.data_ptr();
  a.val_cache = value_cache.data_ptr();
  a.block_tables = block_tables.data_ptr();
  a.block_info = block_info.data_ptr();
  a.seq_lens = seq_lens.data_ptr();
  // 2^ek folds into the score scale: a power of two, so the product is exact
  a.scale = (float)scale * k_scale;
  a.v_scale = v_scale;
  a.nblocks = (int)nblocks;
  a.num_seqs = (int)block_tables.size(0);
  a.max_pages = (int)block_tables.size(1);
  a.num_q_heads = (int)num_q_heads;
  a.num_kv_heads = (int)num_kv_heads;
  a.q_stride = (int)q.stride(0);
  a.fp8 = fp8;
  LAUNCH(launch_prefill_attention_paged, a, current_stream());
  return out;
}

torch::Tensor mfma_probe(torch::Tensor a, torch::Tensor b, int64_t a_split,
                         int64_t b_split) {
  auto d = torch::zeros({16, 16}, a.options().dtype(torch::kFloat32));
  LAUNCH(launch_mfma_probe, d.data_ptr(), a.data_ptr(), b.data_ptr(),
         (int)a_split, (int)b_split, current_stream());
  return d;
}

torch::Tensor mfma_probe32(torch::Tensor a, torch::Tensor b, int64_t a_split,
                           int64_t b_split, int64_t dmap) {
  auto d = torch::zeros({32, 32}, a.options().dtype(torch::kFloat32));
  LAUNCH(launch_mfma_probe32, d.data_ptr(), a.data_ptr(), b.data_ptr(),
         (int)a_split, (int)b_split, (int)dmap, current_stream());
  return d;
}

}  // namespace

static int pick_gemm_splits(int N, int K) {
  // fill the chip with 16-wave workgroups (>= ~256 WGs); each split's K
  // range divides into 8 x 32-k wave slices (K % (splits*256) == 0)
  const int n_groups = N >> 5;
  for (int s : {8, 4, 2})
    if (n_groups * s <= 512 && n_groups * s >= 192 && K % (s * 256) == 0)
      return s;
  for (int s : {4, 2})
    if (n_groups * s >= 128 && K % (s * 256) == 0) return s;
  return 1;
}

bool skinny_gemm_supported(int64_t M, int64_t N, int64_t K) {
  // M <= 256: the cross-slice LDS reduce holds 4 waves x M_TILES x 1 KB
  // (64 KB at M_TILES=16); larger batches fall back to hipBLASLt
  return M >= 1 && M <= 256 && (N % 32) == 0 && (K % 256) == 0;
}

// The 64-column-panel kernel (skinny_gemm_tile.h) on bf16 weights: 8 waves
// over 4 row groups of at most 2 m-tiles, whole 64-column panels.
bool skinny_gemm_wide_supported(int64_t M, int64_t N) {
  return M >= 1 && M <= 128 && (N % 64) == 0;
}

static int pick_gemm_panel(int64_t M, int64_t N) {
  // measured policy (profiles/sg_micro8_cold.json, weights streamed from
  // HBM, o and down of Llama-3-8B): the 64-column panel wins at M = 64
  // (o 14.5 -> 12.9 us, down 35.1 -> 28.4) and M = 128 (o 20.4 -> 15.9,
  // down 50.8 -> 36.1); at M <= 32, where A is at most a fifth of a
  // 32-column panel's staging anyway, it ties or loses by up to 7 %
  // (o at M = 16: 11.4 -> 12.2)
  return M > 32 && skinny_gemm_wide_supported(M, N) ? 64 : 32;
}

namespace {

// What the bf16 and the e4m3 GEMM launch share once their operands are
// checked: the split count (the bf16 GEMM's policy for both, so that both
// engines split alike) and the output it implies.  With splits > 1 the f32
// partials [splits, M, N] go to `ws` for the caller to fold, with splits == 1
// the bf16 result goes to `c`; the other of *cp / *wsp stays null.  `k_unit`
// is what the caller's message calls the split count that K must hold.
int plan_gemm_splits(const torch::Tensor& a, int64_t N, int64_t force_splits,
                     const char* k_unit, torch::Tensor& c, torch::Tensor& ws,
                     void** cp, void** wsp) {
  const int64_t M = a.size(0), K = a.size(1);
  // only SPLITS 1/2/4/8 are instantiated, and each split's k range must be
  // whole 256-k groups (an even, >= 4 step count): anything else would
  // launch a kernel whose grid and workspace disagree with its k span
  TORCH_CHECK(force_splits == 0 || force_splits == 1 || force_splits == 2 ||
                  force_splits == 4 || force_splits == 8,
              "force_splits must be 0 (auto), 1, 2, 4 or 8");
  const int splits = force_splits > 0 ? (int)force_splits
                                      : pick_gemm_splits((int)N, (int)K);
  TORCH_CHECK(K >= 256 && K % (splits * 256) == 0, "K must be a multiple of ",
              k_unit, " * 256");
  if (splits > 1) {
    ws = torch::empty({splits, M, N}, a.options().dtype(torch::kFloat32));
    *wsp = ws.data_ptr();
  } else {
    c = torch::empty({M, N}, a.options());
    *cp = c.data_ptr();
  }
  return splits;
}

// Shape, dtype, device and contiguity checks shared by skinny_gemm and
// skinny_gemm_add_rmsnorm, then the GEMM launch.  Returns the split count
// and leaves the result in `c` or `ws` as plan_gemm_splits says.
int skinny_gemm_launch(const torch::Tensor& a, const torch::Tensor& w,
                       int64_t force_splits, int64_t panel, torch::Tensor& c,
                       torch::Tensor& ws) {
  check_bf16_contig(a, "a");
  check_bf16_contig(w, "w");
  TORCH_CHECK(a.dim() == 2 && w.dim() == 2, "a and w must be 2-D");
  TORCH_CHECK(a.device() == w.device(), "a/w device mismatch");
  const int64_t M = a.size(0), K = a.size(1), N = w.size(0);
  TORCH_CHECK(w.size(1) == K, "K mismatch");
  TORCH_CHECK(skinny_gemm_supported(M, N, K), "unsupported skinny shape");
  TORCH_CHECK(panel == 0 || panel == 32 || panel == 64,
              "panel must be 0 (auto), 32 or 64");
  TORCH_CHECK(panel != 64 || skinny_gemm_wide_supported(M, N),
              "panel 64 needs M <= 128 and N % 64 == 0");
  void* cp = nullptr;
  void* wsp = nullptr;
  const int splits =
      plan_gemm_splits(a, N, force_splits, "force_splits", c, ws, &cp, &wsp);
  if (panel == 0) panel = pick_gemm_panel(M, N);
  if (panel == 64)
    LAUNCH(launch_skinny_gemm_wide, cp, wsp, a.data_ptr(), w.data_ptr(),
           (int)M, (int)N, (int)K, splits, current_stream());
  else
    LAUNCH(launch_skinny_gemm, cp, wsp, a.data_ptr(), w.data_ptr(), (int)M,
           (int)N, (int)K, splits, current_stream());
  return splits;
}

// What both GEMMs leave to be done: fold the f32 partials of splits > 1.
torch::Tensor fold_gemm_splits(const torch::Tensor& a, int64_t N, int splits,
                               torch::Tensor c, const torch::Tensor& ws) {
  if (splits > 1) {
    c = torch::empty({a.size(0), N}, a.options());
    LAUNCH(launch_reduce_splits, c.data_ptr(), ws.data_ptr(), splits,
           (long)c.numel(), current_stream());
  }
  return c;
}

// The add + RMSNorm arguments of both fused GEMMs, checked before the GEMM
// allocates or launches anything.
void check_add_rmsnorm_args(const torch::Tensor& a, const torch::Tensor& w,
                            const torch::Tensor& residual,
                            const torch::Tensor& norm_weight) {
  check_bf16_contig(residual, "residual");
  check_bf16_contig(norm_weight, "norm_weight");
  TORCH_CHECK(a.dim() == 2 && w.dim() == 2, "a and w must be 2-D");
  TORCH_CHECK(residual.dim() == 2 && residual.size(0) == a.size(0) &&
                  residual.size(1) == w.size(0),
              "residual must be [M, N]");
  TORCH_CHECK(norm_weight.numel() == w.size(0),
              "norm_weight must have N elements");
  TORCH_CHECK(residual.device() == a.device() &&
                  norm_weight.device() == a.device(),
              "a/residual/norm_weight device mismatch");
}

// residual += gemm; return rmsnorm(residual) * norm_weight, from the bf16
// result `c` (splits == 1) or the partials `ws`, which the norm kernel folds
// in its prologue instead of a reduce_splits launch (and a bf16 round trip)
// of its own.
torch::Tensor add_rmsnorm_after_gemm(const torch::Tensor& a, int64_t N,
                                     int splits, torch::Tensor c,
                                     const torch::Tensor& ws,
                                     torch::Tensor& residual,
                                     const torch::Tensor& norm_weight,
                                     double eps) {
  const int M = (int)a.size(0);
  if (splits == 1) {
    LAUNCH(launch_fused_add_rmsnorm, c.data_ptr(), residual.data_ptr(),
           norm_weight.data_ptr(), (float)eps, M, (int)N, current_stream());
    return c;
  }
  c = torch::empty({a.size(0), N}, a.options());
  LAUNCH(launch_fold_add_rmsnorm, c.data_ptr(), ws.data_ptr(),
         residual.data_ptr(), norm_weight.data_ptr(), (float)eps, splits, M,
         (int)N, current_stream());
  return c;
}

// ---- FP8 weights (skinny_gemm_w8.hip; docs/FEATURES.md "FP8 weights") ------

// w8 e4m3 [N, K] and its exponents e int8 [N], on `device`.
void check_w8_pair(const torch::Tensor& w8, const torch::Tensor& e,
                   const torch::Device& device) {
  TORCH_CHECK(w8.is_cuda(), "w8 must be on GPU");
  TORCH_CHECK(w8.scalar_type() == torch::kFloat8_e4m3fn,
              "w8 must be float8_e4m3fn");
  TORCH_CHECK(w8.is_contiguous() && w8.dim() == 2,
              "w8 must be contiguous and 2-D");
  TORCH_CHECK(e.scalar_type() == torch::kChar, "e must be int8");
  TORCH_CHECK(e.is_contiguous() && e.numel() == w8.size(0),
              "e must be contiguous with one exponent per row of w8");
  TORCH_CHECK(w8.device() == device && e.device() == device,
              "a, w8 and e must be on one device");
}

// skinny_gemm_launch for an e4m3 weight: every check, then the GEMM.
int skinny_gemm_w8_launch(const torch::Tensor& a, const torch::Tensor& w8,
                          const torch::Tensor& e, int64_t force_splits,
                          torch::Tensor& c, torch::Tensor& ws) {
  check_bf16_contig(a, "a");
  TORCH_CHECK(a.dim() == 2, "a must be 2-D");
  check_w8_pair(w8, e, a.device());
  const int64_t M = a.size(0), K = a.size(1), N = w8.size(0);
  TORCH_CHECK(w8.size(1) == K, "K mismatch");
  TORCH_CHECK(M >= 1 && M <= 128, "M must be in [1, 128], got ", M);
  TORCH_CHECK(N >= 64 && N % 64 == 0, "N must be a multiple of 64, got ", N);
  void* cp = nullptr;
  void* wsp = nullptr;
  const int splits =
      plan_gemm_splits(a, N, force_splits, "splits", c, ws, &cp, &wsp);
  LAUNCH(launch_skinny_gemm_w8, cp, wsp, a.data_ptr(), w8.data_ptr(),
         e.data_ptr(), (int)M, (int)N, (int)K, splits, current_stream());
  return splits;
}

}  // namespace

torch::Tensor skinny_gemm(torch::Tensor a, torch::Tensor w,
                          int64_t force_splits = 0, int64_t panel = 0) {
  torch::Tensor c, ws;
  const int splits = skinny_gemm_launch(a, w, force_splits, panel, c, ws);
  return fold_gemm_splits(a, w.size(0), splits, c, ws);
}

// h = rmsnorm(a w^T + residual) * norm_weight with residual := a w^T +
// residual in place: bit for bit skinny_gemm followed by fused_add_rmsnorm.
torch::Tensor skinny_gemm_add_rmsnorm(torch::Tensor a, torch::Tensor w,
                                      torch::Tensor residual,
                                      torch::Tensor norm_weight, double eps,
                                      int64_t force_splits = 0,
                                      int64_t panel = 0) {
  check_add_rmsnorm_args(a, w, residual, norm_weight);
  torch::Tensor c, ws;
  const int splits = skinny_gemm_launch(a, w, force_splits, panel, c, ws);
  return add_rmsnorm_after_gemm(a, w.size(0), splits, c, ws, residual,
                                norm_weight, eps);
}

// C = a dq(w8)^T, bit for bit skinny_gemm(a, dq(w8), force_splits).
torch::Tensor skinny_gemm_w8(torch::Tensor a, torch::Tensor w8,
                             torch::Tensor e, int64_t force_splits = 0) {
  torch::Tensor c, ws;
  const int splits = skinny_gemm_w8_launch(a, w8, e, force_splits, c, ws);
  return fold_gemm_splits(a, w8.size(0), splits, c, ws);
}

torch::Tensor skinny_gemm_w8_add_rmsnorm(torch::Tensor a, torch::Tensor w8,
                                         torch::Tensor e,
                                         torch::Tensor residual,
                                         torch::Tensor norm_weight, double eps,
                                         int64_t force_splits = 0) {
  check_add_rmsnorm_args(a, w8, residual, norm_weight);
  torch::Tensor c, ws;
  const int splits = skinny_gemm_w8_launch(a, w8, e, force_splits, c, ws);
  return add_rmsnorm_after_gemm(a, w8.size(0), splits, c, ws, residual,
                                norm_weight, eps);
}

// bf16 [N, K] = e4m3(w8) * 2^e[row] (exact), for the shapes the GEMM above
// does not serve.
torch::Tensor w8_dequant(torch::Tensor w8, torch::Tensor e) {
  check_w8_pair(w8, e, w8.device());
  const int64_t N = w8.size(0), K = w8.size(1);
  TORCH_CHECK(K % 16 == 0, "K must be a multiple of 16, got ", K);
  auto out = torch::empty({N, K}, w8.options().dtype(torch::kBFloat16));
  if (out.numel() == 0) return out;
  LAUNCH(launch_w8_dequant, out.data_ptr(), w8.data_ptr(), e.data_ptr(),
         (long)N, (long)K, current_stream());
  return out;
}


// ---- mixture of experts (moe.hip; docs/FEATURES.md "Mixture of experts") ---

namespace {

constexpr int64_t kMoeMaxExperts = 256, kMoeMaxTopK = 8;
// T * k pair indices and their rows of H or I elements are int32 / size_t in
// the kernels; the bound keeps T * k * 8 far inside int32 too
constexpr int64_t kMoeMaxPairs = 1 << 24;

void check_i32_on(const torch::Tensor& t, const char* name,
                  const torch::Device& device, int64_t numel) {
  check_i32_gpu(t, name);
  TORCH_CHECK(t.device() == device, name, " is on another device");
  TORCH_CHECK(t.numel() == numel, name, " must have ", numel, " elements");
}

// The expert weights of one layer, w1 [E, 2I, H] and w2 [E, H, I] on x's
// device, for the shapes the grouped GEMMs serve: both bf16 and no exponents,
// or both e4m3 with e1 int8 [E, 2I] and e2 int8 [E, H] (docs/FEATURES.md "FP8
// experts"), or both uint8 e2m1 codes, w1 [E, 2I, H/2] and w2 [E, H, I/2],
// with e1 int8 [E, 2I, H/32] and e2 int8 [E, H, I/32] ("MXFP4 experts").
// Returns I.
int64_t check_moe_experts(const torch::Tensor& x, const torch::Tensor& w1,
                          const torch::Tensor& w2,
                          const c10::optional<torch::Tensor>& e1,
                          const c10::optional<torch::Tensor>& e2) {
  check_bf16_contig(x, "x");
  TORCH_CHECK(w1.scalar_type() == w2.scalar_type(),
              "w1 and w2 must have one dtype");
  const bool w4 = w1.scalar_type() == torch::kByte;
  if (w4) {
    TORCH_CHECK(e1.has_value() && e2.has_value(),
                "MXFP4 experts need w1_scale_log2 and w2_scale_log2");
    const torch::Tensor* w[2] = {&w1, &w2};
    const torch::Tensor* e[2] = {&*e1, &*e2};
    for (int i = 0; i < 2; ++i) {
      TORCH_CHECK(w[i]->is_cuda() && w[i]->is_contiguous() &&
                      (uintptr_t)w[i]->data_ptr() % 16 == 0,
                  "an MXFP4 expert weight must be contiguous on GPU");
      TORCH_CHECK(e[i]->scalar_type() == torch::kChar &&
                      e[i]->is_contiguous() && e[i]->dim() == 3 &&
                      w[i]->dim() == 3 && e[i]->size(0) == w[i]->size(0) &&
                      e[i]->size(1) == w[i]->size(1) &&
                      e[i]->size(2) * 16 == w[i]->size(2) &&
                      e[i]->device() == x.device(),
                  "an MXFP4 expert scale must be contiguous int8 [E, rows of "
                  "its weight, K / 32] on x's device");
    }
  } else if (w1.scalar_type() == torch::kFloat8_e4m3fn) {
    TORCH_CHECK(e1.has_value() && e2.has_value(),
                "e4m3 experts need w1_scale_log2 and w2_scale_log2");
    const torch::Tensor* w[2] = {&w1, &w2};
    const torch::Tensor* e[2] = {&*e1, &*e2};
    for (int i = 0; i < 2; ++i) {
      TORCH_CHECK(w[i]->is_cuda() && w[i]->is_contiguous() &&
                      (uintptr_t)w[i]->data_ptr() % 16 == 0,
                  "an e4m3 expert weight must be contiguous on GPU");
      TORCH_CHECK(e[i]->scalar_type() == torch::kChar &&
                      e[i]->is_contiguous() && e[i]->dim() == 2 &&
                      w[i]->dim() == 3 && e[i]->size(0) == w[i]->size(0) &&
                      e[i]->size(1) == w[i]->size(1) &&
                      e[i]->device() == x.device() &&
                      (uintptr_t)e[i]->data_ptr() % 4 == 0,
                  "an expert scale must be contiguous int8 [E, rows of its "
                  "weight] on x's device");
    }
  } else {
    TORCH_CHECK(!e1.has_value() && !e2.has_value(),
                "a scale was given for experts that are not e4m3");
    check_bf16_contig(w1, "w1");
    check_bf16_contig(w2, "w2");
  }
  TORCH_CHECK(x.dim() == 2, "x must be [T, H]");
  TORCH_CHECK(w1.dim() == 3 && w2.dim() == 3,
              "w1 must be [E, 2I, H] and w2 [E, H, I]");
  TORCH_CHECK(w1.device() == x.device() && w2.device() == x.device(),
              "x/w1/w2 device mismatch");
  // two codes per MXFP4 byte: I from the scales, as H is from x
  const int64_t H = x.size(1), E = w1.size(0);
  const int64_t I = w4 ? e2->size(2) * 32 : w2.size(2), per = w4 ? 2 : 1;
  TORCH_CHECK(E >= 1 && E <= kMoeMaxExperts, "E must be in [1, 256], got ", E);
  TORCH_CHECK(H >= 256 && H % 256 == 0, "H must be a multiple of 256, got ",
              H);
  TORCH_CHECK(I >= 64 && I % 64 == 0, "I must be a multiple of 64, got ", I);
  TORCH_CHECK(w1.size(1) == 2 * I && w1.size(2) * per == H,
              "w1 must be [E, 2I, H] (MXFP4: [E, 2I, H/2])");
  TORCH_CHECK(w2.size(0) == E && w2.size(1) == H && w2.size(2) * per == I,
              "w2 must be [E, H, I] (MXFP4: [E, H, I/2])");
  return I;
}

}  // namespace

// (ids int32 [T, k], weights f32 [T, k], expert_offsets int32 [E + 1],
// sorted_pairs int32 [T * k]) of bf16 router logits [T, E]; ticket is the
// caller's zeroed int32 [1].
std::vector<torch::Tensor> moe_route(torch::Tensor logits, torch::Tensor ticket,
                                     int64_t top_k, bool renormalize) {
  check_bf16_contig(logits, "router_logits");
  TORCH_CHECK(logits.dim() == 2, "router_logits must be [T, E]");
  const int64_t T = logits.size(0), E = logits.size(1);
  TORCH_CHECK(E >= 1 && E <= kMoeMaxExperts, "E must be in [1, 256], got ", E);
  TORCH_CHECK(top_k >= 1 && top_k <= kMoeMaxTopK && top_k <= E,
              "top_k must be in [1, min(8, E)], got ", top_k);
  TORCH_CHECK(T * top_k <= kMoeMaxPairs, "too many (token, expert) pairs");
  check_i32_on(ticket, "ticket", logits.device(), 1);
  auto i32 = logits.options().dtype(torch::kInt32);
  auto ids = torch::empty({T, top_k}, i32);
  auto w = torch::empty({T, top_k}, logits.options().dtype(torch::kFloat32));
  auto sorted = torch::empty({T * top_k}, i32);
  if (T == 0) return {ids, w, torch::zeros({E + 1}, i32), sorted};
  auto offsets = torch::empty({E + 1}, i32);
  LAUNCH(launch_moe_route, ids.data_ptr(), w.data_ptr(), offsets.data_ptr(),
         sorted.data_ptr(), ticket.data_ptr(), logits.data_ptr(), (int)T,
         (int)E, (int)top_k, renormalize ? 1 : 0, current_stream());
  return {ids, w, offsets, sorted};
}

// (expert_offsets, sorted_pairs) of ids [T, k] whose values the caller has
// checked to lie in [0, E).
std::vector<torch::Tensor> moe_group(torch::Tensor ids, int64_t E) {
  check_i32_gpu(ids, "ids");
  TORCH_CHECK(ids.dim() == 2, "ids must be [T, k]");
  TORCH_CHECK(E >= 1 && E <= kMoeMaxExperts, "E must be in [1, 256], got ", E);
  TORCH_CHECK(ids.numel() <= kMoeMaxPairs, "too many (token, expert) pairs");
  auto sorted = torch::empty({ids.numel()}, ids.options());
  if (ids.numel() == 0) return {torch::zeros({E + 1}, ids.options()), sorted};
  auto offsets = torch::empty({E + 1}, ids.options());
  LAUNCH(launch_moe_group, offsets.data_ptr(), sorted.data_ptr(),
         ids.data_ptr(), (int)ids.numel(), (int)E, current_stream());
  return {offsets, sorted};
}

// y bf16 [T, H] from the grouping of moe_route / moe_group.  e4m3 w1 and w2
// come with their int8 exponents and stand for dq = e4m3 * 2^e[expert, row];
// uint8 ones are MXFP4 codes and stand for e2m1 * 2^e[expert, row, k / 32].
torch::Tensor moe_ffn(torch::Tensor x, torch::Tensor w1, torch::Tensor w2,
                      torch::Tensor weights, torch::Tensor expert_offsets,
                      torch::Tensor sorted_pairs,
                      c10::optional<torch::Tensor> w1_scale_log2,
                      c10::optional<torch::Tensor> w2_scale_log2) {
  const int64_t I = check_moe_experts(x, w1, w2, w1_scale_log2, w2_scale_log2);
  const int64_t T = x.size(0), H = x.size(1), E = w1.size(0);
  TORCH_CHECK(weights.is_cuda() && weights.device() == x.device() &&
                  weights.scalar_type() == torch::kFloat32 &&
                  weights.is_contiguous() && weights.dim() == 2 &&
                  weights.size(0) == T,
              "weights must be contiguous fp32 [T, k] on x's device");
  const int64_t k = weights.size(1);
  TORCH_CHECK(k >= 1 && k <= kMoeMaxTopK && k <= E,
              "k must be in [1, min(8, E)], got ", k);
  TORCH_CHECK(T * k <= kMoeMaxPairs, "too many (token, expert) pairs");
  check_i32_on(expert_offsets, "expert_offsets", x.device(), E + 1);
  check_i32_on(sorted_pairs, "sorted_pairs", x.device(), T * k);
  auto y = torch::empty({T, H}, x.options());
  if (T == 0) return y;
  auto h = torch::empty({T * k, I}, x.options());
  auto opart = torch::empty({T * k, H}, x.options().dtype(torch::kFloat32));
  MoeFfnLaunch a;
  a.y = y.data_ptr();
  a.h = h.data_ptr();
  a.opart = opart.data_ptr();
  a.x = x.data_ptr();
  a.w1 = w1.data_ptr();
  a.w2 = w2.data_ptr();
  a.weights = weights.data_ptr();
  a.expert_offsets = expert_offsets.data_ptr();
  a.sorted_pairs = sorted_pairs.data_ptr();
  a.T = (int)T;
  a.k = (int)k;
  a.E = (int)E;
  a.H = (int)H;
  a.I = (int)I;
  if (w1_scale_log2.has_value()) {
    a.w1_exp = w1_scale_log2->data_ptr();
    a.w2_exp = w2_scale_log2->data_ptr();
    a.format = w1.scalar_type() == torch::kByte ? MoeFfnLaunch::MXFP4
                                                : MoeFfnLaunch::E4M3;
  }
  LAUNCH(launch_moe_ffn, a, current_stream());
  return y;
}

// ---- fused seeded sampler (ops.sample) -----------------------------------
// logits fp32 [n, V] contiguous; every per-row parameter is a device tensor
// of length n, so nothing here reads a value back or synchronises.
std::vector<torch::Tensor> sample(torch::Tensor logits,
                                  torch::Tensor temperature,
                                  torch::Tensor top_k, torch::Tensor top_p,
                                  torch::Tensor min_p, torch::Tensor seed,
                                  torch::Tensor pos) {
  TORCH_CHECK(logits.is_cuda(), "logits must be on GPU");
  TORCH_CHECK(logits.scalar_type() == torch::kFloat32, "logits must be fp32");
  TORCH_CHECK(logits.dim() == 2, "logits must be [n, V]");
  TORCH_CHECK(logits.is_contiguous(), "logits must be contiguous");
  const int64_t n = logits.size(0), V = logits.size(1);
  TORCH_CHECK(V >= 1, "V must be >= 1");
  TORCH_CHECK(V <= INT32_MAX && n <= INT32_MAX, "n and V must fit int32");
  auto check_param = [&](const torch::Tensor& t, torch::ScalarType dt,
                         const char* name) {
    TORCH_CHECK(t.is_cuda() && t.device() == logits.device(), name,
                " must be on the logits' device");
    TORCH_CHECK(t.scalar_type() == dt, name, " has the wrong dtype");
    TORCH_CHECK(t.dim() == 1 && t.size(0) == n, name,
                " must have one entry per row");
    TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  };
  check_param(temperature, torch::kFloat32, "temperature");
  check_param(top_k, torch::kInt32, "top_k");
  check_param(top_p, torch::kFloat32, "top_p");
  check_param(min_p, torch::kFloat32, "min_p");
  check_param(seed, torch::kInt64, "seed");
  check_param(pos, torch::kInt32, "pos");
  auto tokens = torch::empty({n}, logits.options().dtype(torch::kInt64));
  auto kept = torch::empty({n}, logits.options().dtype(torch::kInt32));
  if (n == 0) return {tokens, kept};
  LAUNCH(launch_sample, tokens.data_ptr(), kept.data_ptr(),
         logits.data_ptr(), temperature.data_ptr(), top_k.data_ptr(),
         top_p.data_ptr(), min_p.data_ptr(), seed.data_ptr(), pos.data_ptr(),
         (int)n, (int)V, current_stream());
  return {tokens, kept};
}

// ---- KV-pool IPC export + xGMI peer push (parallel/kv_peer.py) -----------
// The decode engine's KV pool is allocated with hipMalloc directly (not the
// caching allocator) so data_ptr() IS the allocation base hipIpcGetMemHandle
// requires; the prefill process maps it with lazy peer access (the xGMI
// route) and pushes pages with the kv_peer_copy kernel.

// hipMalloc-backed tensor of any element type (bf16 and e4m3 KV pools).
torch::Tensor ipc_alloc(std::vector<int64_t> sizes, torch::ScalarType dtype) {
  int64_t numel = 1;
  for (auto s : sizes) numel *= s;
  const int64_t bytes = numel * (int64_t)c10::elementSize(dtype);
  void* ptr = nullptr;
  hipError_t err = hipMalloc(&ptr, bytes);
  TORCH_CHECK(err == hipSuccess, "hipMalloc(", bytes,
              " B) failed: ", hipGetErrorString(err));
  int dev = 0;
  (void)hipGetDevice(&dev);
  auto opts = torch::TensorOptions().dtype(dtype).device(torch::kCUDA, dev);
  return torch::from_blob(
      ptr, sizes, [](void* p) { (void)hipFree(p); }, opts);
}

torch::Tensor ipc_alloc_bf16(std::vector<int64_t> sizes) {
  return ipc_alloc(std::move(sizes), torch::kBFloat16);
}

py::bytes kv_ipc_export(torch::Tensor pool) {
  TORCH_CHECK(pool.is_cuda(), "pool must be on GPU");
  hipIpcMemHandle_t handle;
  hipError_t err = hipIpcGetMemHandle(&handle, pool.data_ptr());
  TORCH_CHECK(err == hipSuccess,
              "hipIpcGetMemHandle failed (pool must be an ipc_alloc_bf16 "
              "base allocation): ", hipGetErrorString(err));
  return py::bytes(reinterpret_cast<const char*>(&handle), sizeof(handle));
}

int64_t kv_ipc_open(std::string raw) {
  // std::string parameter: converted from py::bytes during argument
  // processing (GIL held) so the gil_scoped_release guard is safe
  TORCH_CHECK(raw.size() == sizeof(hipIpcMemHandle_t), "bad handle size");
  hipIpcMemHandle_t handle;
  memcpy(&handle, raw.data(), sizeof(handle));
  void* ptr = nullptr;
  hipError_t err =
      hipIpcOpenMemHandle(&ptr, handle, hipIpcMemLazyEnablePeerAccess);
  TORCH_CHECK(err == hipSuccess,
              "hipIpcOpenMemHandle failed: ", hipGetErrorString(err));
  return reinterpret_cast<int64_t>(ptr);
}

void kv_ipc_close(int64_t ptr) {
  hipError_t err = hipIpcCloseMemHandle(reinterpret_cast<void*>(ptr));
  TORCH_CHECK(err == hipSuccess,
              "hipIpcCloseMemHandle failed: ", hipGetErrorString(err));
}

void kv_peer_copy(int64_t dst_base, torch::Tensor src_kv,
                  torch::Tensor src_pages, torch::Tensor dst_pages,
                  int64_t dst_num_pages) {
  // src_kv: [L, 2, Ps, kvh, ps, hd] bf16 or e4m3, contiguous; dst pool has
  // the SAME element type and per-page layout but its own page count
  // (dst_num_pages).  The copy moves bytes: chunks are counted in 16-byte
  // vectors.
  TORCH_CHECK(src_kv.is_cuda(), "src_kv must be on GPU");
  TORCH_CHECK(src_kv.scalar_type() == torch::kBFloat16 ||
                  src_kv.scalar_type() == torch::kFloat8_e4m3fn,
              "src_kv must be bf16 or float8_e4m3fn");
  TORCH_CHECK(src_kv.is_contiguous(), "src_kv must be contiguous");
  TORCH_CHECK(src_kv.dim() == 6 && src_kv.size(1) == 2, "kv must be 6-D");
  TORCH_CHECK(src_pages.is_cuda() && dst_pages.is_cuda() &&
                  src_pages.scalar_type() == torch::kInt32 &&
                  dst_pages.scalar_type() == torch::kInt32,
              "page lists must be int32 on GPU");
  TORCH_CHECK(src_pages.numel() == dst_pages.numel(), "page count mismatch");
  // the page indices themselves are range-checked by the caller
  // (PeerKVPusher.push) before they are uploaded
  TORCH_CHECK(dst_base != 0, "dst_base is null");
  TORCH_CHECK(dst_num_pages >= 1, "dst_num_pages must be >= 1, got ",
              dst_num_pages);
  const int n_pages = src_pages.numel();
  if (n_pages == 0) return;
  const int layers = src_kv.size(0);
  const long Ps = src_kv.size(2);
  const long chunk_bytes = src_kv.size(3) * src_kv.size(4) * src_kv.size(5) *
                           (long)src_kv.element_size();
  TORCH_CHECK(chunk_bytes % 16 == 0, "chunk must be 16B-aligned");
  const long chunk_vec = chunk_bytes / 16;  // uint4 vectors
  KvPeerCopyLaunch a;
  a.dst_base = reinterpret_cast<void*>(dst_base);
  a.src_base = src_kv.data_ptr();
  a.src_pages = src_pages.data_ptr();
  a.dst_pages = dst_pages.data_ptr();
  a.n_pages = n_pages;
  a.n_chunks = 2 * layers;
  a.chunk_vec = (int)chunk_vec;
  a.src_page_stride_vec = chunk_vec;
  a.dst_page_stride_vec = chunk_vec;
  a.src_chunk_stride_vec = Ps * chunk_vec;
  a.dst_chunk_stride_vec = dst_num_pages * chunk_vec;
  LAUNCH(launch_kv_peer_copy, a, current_stream());
}

// ---- one-shot xGMI all-reduce (parallel/xgmi_allreduce.py) ---------------
// Data buffer: ordinary hipMalloc (IPC-exportable base).  Signal buffer:
// UNCACHED device memory so remote flag stores are immediately visible to
// the local spin loops.

int64_t ar_alloc_signals() {
  void* ptr = nullptr;
  hipError_t err = hipExtMallocWithFlags(
      &ptr, (size_t)xgmi_allreduce_signal_bytes(), hipDeviceMallocUncached);
  TORCH_CHECK(err == hipSuccess,
              "uncached signal alloc failed: ", hipGetErrorString(err));
  (void)hipMemset(ptr, 0, (size_t)xgmi_allreduce_signal_bytes());
  (void)hipDeviceSynchronize();
  return reinterpret_cast<int64_t>(ptr);
}

py::bytes ar_export_ptr(int64_t ptr) {
  hipIpcMemHandle_t handle;
  hipError_t err =
      hipIpcGetMemHandle(&handle, reinterpret_cast<void*>(ptr));
  TORCH_CHECK(err == hipSuccess,
              "hipIpcGetMemHandle failed: ", hipGetErrorString(err));
  return py::bytes(reinterpret_cast<const char*>(&handle), sizeof(handle));
}

unsigned ar_error_flag(int64_t sig_ptr) {
  unsigned err_word = 0;
  // offsetof, NOT sizeof-4: the 128-byte struct alignment pads the tail,
  // so sizeof-4 read the padding and timeouts were invisible (r2 GPU run)
  char* base = reinterpret_cast<char*>(sig_ptr);
  (void)hipMemcpy(&err_word, base + xgmi_allreduce_error_offset(),
                  sizeof(unsigned), hipMemcpyDeviceToHost);
  return err_word;
}

torch::Tensor ar_dump_signals(int64_t sig_ptr) {
  // debug: the whole Signals block as int32 on CPU
  long n = xgmi_allreduce_signal_bytes() / 4;
  auto t = torch::empty({n}, torch::TensorOptions().dtype(torch::kInt32));
  (void)hipMemcpy(t.data_ptr(), reinterpret_cast<void*>(sig_ptr), n * 4,
                  hipMemcpyDeviceToHost);
  return t;
}

torch::Tensor xgmi_allreduce(torch::Tensor inp,
                             std::vector<int64_t> sig_ptrs,
                             std::vector<int64_t> data_ptrs, int64_t rank) {
  check_bf16_contig(inp, "inp");
  const int world = (int)sig_ptrs.size();
  TORCH_CHECK(world >= 1 && world <= 8 &&
                  data_ptrs.size() == (size_t)world && rank >= 0 &&
                  rank < world,
              "bad world/rank");
  TORCH_CHECK(inp.numel() % 8 == 0, "numel must be a multiple of 8");
  auto out = torch::empty_like(inp);
  void* sp[8];
  void* dp[8];
  for (int i = 0; i < world; ++i) {
    sp[i] = reinterpret_cast<void*>(sig_ptrs[i]);
    dp[i] = reinterpret_cast<void*>(data_ptrs[i]);
  }
  LAUNCH(launch_xgmi_allreduce, out.data_ptr(), inp.data_ptr(), sp, dp, world,
         (int)rank, (long)inp.numel(), current_stream());
  return out;
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("rmsnorm", &rmsnorm, "RMSNorm (bf16)");
  m.def("fused_add_rmsnorm", &fused_add_rmsnorm, "x,residual += ; rmsnorm");
  m.def("silu_mul", &silu_mul, "silu(gate)*up");
  m.def("rope_store_kv", &rope_store_kv, "RoPE + paged KV write");
  m.def("decode_attention", &decode_attention, "paged flash-decode",
        py::arg("q"), py::arg("key_cache"), py::arg("value_cache"),
        py::arg("block_tables"), py::arg("context_lens"), py::arg("scale"),
        py::arg("num_splits"), py::arg("variant"), py::arg("combine") = 0);
  m.def("rope_store_kv_fp8", &rope_store_kv_fp8,
        "RoPE + quantising (e4m3) paged KV write");
  m.def("kv_gather_dequant", &kv_gather_dequant,
        "gather e4m3 cache rows by slot -> bf16 [Tkv, KVH, D]");
  m.def("decode_attention_fp8", &decode_attention_fp8,
        "paged flash-decode over an e4m3 cache (page-pair MFMA)",
        py::arg("q"), py::arg("key_cache"), py::arg("value_cache"),
        py::arg("block_tables"), py::arg("context_lens"), py::arg("scale"),
        py::arg("num_splits"), py::arg("k_scale_log2"),
        py::arg("v_scale_log2"), py::arg("combine") = 0);
  m.def("prefill_attention", &prefill_attention, "varlen causal flash prefill");
  m.def("prefill_attention_paged", &prefill_attention_paged,
        "varlen causal flash prefill reading K/V through the block table "
        "(bf16 or e4m3 pool)");
  m.def("mfma_probe", &mfma_probe, "MFMA layout probe");
  m.def("mfma_probe32", &mfma_probe32, "32x32x16 MFMA layout probe");
  m.def("skinny_gemm", &skinny_gemm, "decode-shape GEMM (M<=128)",
        py::arg("a"), py::arg("w"), py::arg("force_splits") = 0,
        py::arg("panel") = 0);
  m.def("skinny_gemm_add_rmsnorm", &skinny_gemm_add_rmsnorm,
        "skinny_gemm + fused_add_rmsnorm with the split-K fold inside the "
        "norm kernel; returns h, updates residual in place",
        py::arg("a"), py::arg("w"), py::arg("residual"),
        py::arg("norm_weight"), py::arg("eps"), py::arg("force_splits") = 0,
        py::arg("panel") = 0);
  m.def("skinny_gemm_w8", &skinny_gemm_w8,
        "decode-shape GEMM over e4m3 weights with per-row 2^e scales",
        py::arg("a"), py::arg("w8"), py::arg("e"),
        py::arg("force_splits") = 0);
  m.def("skinny_gemm_w8_add_rmsnorm", &skinny_gemm_w8_add_rmsnorm,
        "skinny_gemm_w8 + fused_add_rmsnorm with the split-K fold inside the "
        "norm kernel; returns h, updates residual in place",
        py::arg("a"), py::arg("w8"), py::arg("e"), py::arg("residual"),
        py::arg("norm_weight"), py::arg("eps"), py::arg("force_splits") = 0);
  m.def("w8_dequant", &w8_dequant,
        "e4m3 [N, K] + int8 exponents [N] -> bf16 [N, K]");
  m.def("moe_route", &moe_route,
        "top-k routing + grouping by expert -> (ids, weights, "
        "expert_offsets, sorted_pairs)");
  m.def("moe_group", &moe_group,
        "grouping of given ids by expert -> (expert_offsets, sorted_pairs)");
  m.def("moe_ffn", &moe_ffn,
        "grouped gate_up + SwiGLU, grouped down, weighted combine; e4m3 w1 "
        "and w2 take their int8 per-row exponents",
        py::arg("x"), py::arg("w1"), py::arg("w2"), py::arg("weights"),
        py::arg("expert_offsets"), py::arg("sorted_pairs"),
        py::arg("w1_scale_log2") = py::none(),
        py::arg("w2_scale_log2") = py::none());
  m.def("sample", &sample,
        "seeded top-k/min-p/top-p Gumbel-max sampler -> (tokens, num_kept)");
  // gil_scoped_release on the IPC/copy entry points: mapping or launching
  // against a dying peer can block inside the HIP runtime, and holding the
  // GIL there freezes heartbeats until the controller kills the process
  m.def("ipc_alloc_bf16", &ipc_alloc_bf16,
        "hipMalloc-backed bf16 tensor (IPC-exportable base allocation)",
        py::call_guard<py::gil_scoped_release>());
  m.def("ipc_alloc", &ipc_alloc,
        "hipMalloc-backed tensor of any dtype (IPC-exportable allocation)",
        py::call_guard<py::gil_scoped_release>());
  m.def("kv_ipc_export", &kv_ipc_export, "hipIpcGetMemHandle of a KV pool");
  m.def("kv_ipc_open", &kv_ipc_open,
        "map a peer KV pool (lazy xGMI peer access)",
        py::call_guard<py::gil_scoped_release>());
  m.def("kv_ipc_close", &kv_ipc_close, "unmap a peer KV pool",
        py::call_guard<py::gil_scoped_release>());
  m.def("kv_peer_copy", &kv_peer_copy,
        "gather local pages -> scatter into peer pool over xGMI",
        py::call_guard<py::gil_scoped_release>());
  m.def("ar_alloc_signals", &ar_alloc_signals,
        "uncached signal buffer for the xGMI all-reduce");
  m.def("ar_export_ptr", &ar_export_ptr, "hipIpc handle of a raw pointer");
  m.def("ar_error_flag", &ar_error_flag, "read the all-reduce error word");
  m.def("ar_dump_signals", &ar_dump_signals, "debug: dump the signal block");
  m.def("ar_counter_offset", &xgmi_allreduce_counter_offset);
  m.def("xgmi_allreduce", &xgmi_allreduce,
        "one-shot all-reduce over peer-mapped HBM (graph-capturable)");
}
