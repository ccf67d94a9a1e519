// PyTorch bindings for the rbg_amd CDNA4 HIP kernels.
// Thin shape/dtype checks here; all math lives in the .hip translation units.
#include <torch/extension.h>
#include <ATen/hip/HIPContext.h>

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

extern "C" {
void launch_rmsnorm(void*, void*, const void*, float, int, int, hipStream_t);
void launch_fused_add_rmsnorm(void*, void*, const void*, float, int, int,
                              hipStream_t);
void launch_silu_mul(void*, const void*, int, int, hipStream_t);
void launch_rope_store_kv(void*, void*, const void*, void*, void*,
                          const void*, const void*, const void*, int, int,
                          int, int, int, int, int, hipStream_t);
void launch_decode_attention(void*, void*, void*, const void*, const void*,
                             const void*, const void*, const void*, float,
                             int, int, int, int, int, int, int, int, int,
                             hipStream_t);
void launch_prefill_attention(void*, const void*, const void*, const void*,
                              const void*, const void*, float, int, int, int,
                              int, int, int, hipStream_t);
void launch_mfma_probe(void*, const void*, const void*, int, int, hipStream_t);
void launch_mfma_probe32(void*, const void*, const void*, int, int, int,
                         hipStream_t);
void launch_skinny_gemm(void*, void*, const void*, const void*, int, int,
                        int, int, hipStream_t);
void launch_skinny_gemm_wide(void*, void*, const void*, const void*, int, int,
                             int, int, hipStream_t);
void launch_reduce_splits(void*, const void*, int, long, hipStream_t);
void launch_fold_add_rmsnorm(void*, const void*, void*, const void*, float,
                             int, int, int, hipStream_t);
void launch_kv_peer_copy(void*, const void*, const void*, const void*, int,
                         int, int, long, long, long, long, hipStream_t);
void launch_xgmi_allreduce(void*, const void*, void**, void**, int, int,
                           long, hipStream_t);
void launch_sample(void*, void*, const void*, const void*, const void*,
                   const void*, const void*, const void*, const void*, int,
                   int, hipStream_t);
void launch_rope_store_kv_fp8(void*, void*, const void*, void*, void*,
                              const void*, const void*, const void*, int, int,
                              int, int, int, int, float, float, hipStream_t);
void launch_kv_gather_dequant(void*, const void*, const void*, long, int, int,
                              int, float, hipStream_t);
void launch_decode_attention_fp8(void*, void*, void*, const void*, const void*,
                                 const void*, const void*, const void*, float,
                                 float, int, int, int, int, int, int, int,
                                 hipStream_t);
long xgmi_allreduce_signal_bytes();
long xgmi_allreduce_error_offset();
long xgmi_allreduce_counter_offset();
}

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

// Paged KV pool views [pages, KVH, page_size, head_dim]: the kernels index
// them as dense bf16 with a power-of-two page (shift/mask slot math) and
// 16-byte row vectors, so anything else must raise instead of launching.
void check_kv_caches(const torch::Tensor& key_cache,
                     const torch::Tensor& value_cache) {
  check_bf16_contig(key_cache, "key_cache");
  check_bf16_contig(value_cache, "value_cache");
  TORCH_CHECK(key_cache.dim() == 4,
              "key_cache must be [pages, KVH, page_size, head_dim]");
  TORCH_CHECK(value_cache.sizes() == key_cache.sizes(),
              "key_cache/value_cache shape mismatch");
  const int64_t page_size = key_cache.size(2);
  TORCH_CHECK(page_size > 0 && (page_size & (page_size - 1)) == 0,
              "page_size must be a power of two");
  TORCH_CHECK(key_cache.size(1) > 0, "cache needs at least one KV head");
  TORCH_CHECK(key_cache.size(3) > 0 && key_cache.size(3) % 8 == 0,
              "cache head_dim must be a multiple of 8");
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
  launch_rmsnorm(out.data_ptr(), x.data_ptr(), weight.data_ptr(), (float)eps,
                 tokens, hidden, current_stream());
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
  launch_fused_add_rmsnorm(x.data_ptr(), residual.data_ptr(),
                           weight.data_ptr(), (float)eps, tokens, hidden,
                           current_stream());
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
  launch_silu_mul(out.data_ptr(), x.data_ptr(), tokens, inter,
                  current_stream());
  return out;
}

static void check_bf16_rowslice(const torch::Tensor& t, const char* name) {
  // bf16 on GPU, [T, W] or [T, H, D], innermost dims contiguous; the
  // TOKEN stride may be wider (a column slice of the fused QKV buffer)
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, name, " must be bf16");
  if (t.dim() == 2) {
    TORCH_CHECK(t.stride(1) == 1, name, " rows must be contiguous");
  } else {
    TORCH_CHECK(t.dim() == 3 && t.stride(2) == 1 &&
                t.stride(1) == t.size(2), name,
                " must be [T, H, D] with contiguous (H, D) rows");
  }
}

void rope_store_kv(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                   torch::Tensor key_cache, torch::Tensor value_cache,
                   torch::Tensor cos_sin, torch::Tensor positions,
                   torch::Tensor slot_mapping) {
  check_bf16_rowslice(q, "q");
  check_bf16_rowslice(k, "k");
  check_bf16_rowslice(v, "v");
  TORCH_CHECK(k.stride(0) == v.stride(0), "k/v stride mismatch");
  TORCH_CHECK(cos_sin.scalar_type() == torch::kFloat32, "cos_sin fp32");
  TORCH_CHECK(positions.scalar_type() == torch::kInt32, "positions int32");
  TORCH_CHECK(slot_mapping.scalar_type() == torch::kInt32, "slots int32");
  check_kv_caches(key_cache, value_cache);
  check_i32_gpu(positions, "positions");
  check_i32_gpu(slot_mapping, "slot_mapping");
  TORCH_CHECK(cos_sin.is_cuda() && cos_sin.is_contiguous() &&
              cos_sin.dim() == 2, "cos_sin must be a contiguous 2-D GPU tensor");
  const int tokens = q.size(0);
  const int head_dim = key_cache.size(3);
  const int num_kv_heads = key_cache.size(1);
  const int page_size = key_cache.size(2);
  TORCH_CHECK(cos_sin.size(1) == head_dim,
              "cos_sin row width must equal the cache head_dim");
  TORCH_CHECK(k.size(0) == tokens && v.size(0) == tokens &&
              positions.numel() == tokens && slot_mapping.numel() == tokens,
              "q/k/v/positions/slot_mapping token counts differ");
  const int64_t q_width = q.numel() / std::max(tokens, 1);
  const int64_t k_width = k.numel() / std::max(tokens, 1);
  const int64_t v_width = v.numel() / std::max(tokens, 1);
  TORCH_CHECK(k_width == (int64_t)num_kv_heads * head_dim && v_width == k_width,
              "k/v rows must be cache KVH * head_dim wide");
  TORCH_CHECK(q_width % head_dim == 0,
              "q row width must be a multiple of the cache head_dim");
  if (tokens == 0) return;
  const int num_q_heads = (int)(q_width / head_dim);
  launch_rope_store_kv(q.data_ptr(), k.data_ptr(), v.data_ptr(),
                       key_cache.data_ptr(), value_cache.data_ptr(),
                       cos_sin.data_ptr(), positions.data_ptr(),
                       slot_mapping.data_ptr(), tokens, num_q_heads,
                       num_kv_heads, head_dim, page_size,
                       (int)q.stride(0), (int)k.stride(0),
                       current_stream());
}

// How the partials of num_splits > 1 are merged.  combine 0: inside the
// workgroup where a kernel for it exists (the page-pair MFMA kernels at 2 or
// 4 splits), else by decode_combine_kernel; 1: always the separate kernel;
// 2: inside the workgroup, raising where that is not possible.
bool pick_in_wg_combine(int64_t combine, int64_t num_splits, bool mfma_pair,
                        const char* what) {
  TORCH_CHECK(combine >= 0 && combine <= 2,
              "combine must be 0 (auto), 1 (kernel) or 2 (in-workgroup)");
  const bool can = mfma_pair && (num_splits == 2 || num_splits == 4);
  TORCH_CHECK(combine != 2 || can, "combine = 2 needs ", what,
              ", a page size of 16 and 2 or 4 splits");
  const bool in_wg = combine != 1 && can;
  // the in-workgroup kernels run exactly WS = num_splits splits and get no
  // partial buffers: never hand them another count
  TORCH_CHECK(!in_wg || num_splits == 2 || num_splits == 4,
              "in-workgroup combine with ", num_splits, " splits");
  return in_wg;
}

torch::Tensor decode_attention(torch::Tensor q, torch::Tensor key_cache,
                               torch::Tensor value_cache,
                               torch::Tensor block_tables,
                               torch::Tensor context_lens, double scale,
                               int64_t num_splits, int64_t variant,
                               int64_t combine = 0) {
  // q may be a slice of the fused QKV projection: 3-D bf16 with
  // contiguous (head, dim) rows and an arbitrary token stride
  TORCH_CHECK(q.is_cuda() && q.scalar_type() == torch::kBFloat16 &&
              q.dim() == 3 && q.stride(2) == 1 &&
              q.stride(1) == q.size(2), "q must be [T, QH, D] row-sliced");
  const int num_seqs = q.size(0);
  const int num_q_heads = q.size(1);
  const int head_dim = q.size(2);
  TORCH_CHECK(head_dim == 128, "head_dim must be 128");
  check_kv_caches(key_cache, value_cache);
  TORCH_CHECK(key_cache.size(3) == 128, "cache head_dim must be 128");
  const int num_kv_heads = key_cache.size(1);
  const int page_size = key_cache.size(2);
  TORCH_CHECK(num_q_heads % num_kv_heads == 0,
              "q heads must be a multiple of the cache KV heads");
  const int qpg = num_q_heads / num_kv_heads;
  TORCH_CHECK(qpg == 1 || qpg == 2 || qpg == 4 || qpg == 8,
              "GQA group must be 1/2/4/8");
  check_i32_gpu(block_tables, "block_tables");
  check_i32_gpu(context_lens, "context_lens");
  TORCH_CHECK(block_tables.dim() == 2 && block_tables.size(0) == num_seqs,
              "block_tables must be [num_seqs, max_pages]");
  TORCH_CHECK(context_lens.dim() == 1 && context_lens.size(0) == num_seqs,
              "context_lens must be [num_seqs]");
  TORCH_CHECK(num_splits >= 1, "num_splits must be >= 1");
  const bool in_wg = pick_in_wg_combine(
      combine, num_splits, variant == 4 && page_size == 16, "variant 4");
  const int max_pages = block_tables.size(1);
  auto out = torch::empty({num_seqs, num_q_heads, head_dim}, q.options());
  if (num_seqs == 0) return out;
  torch::Tensor partial_o, partial_ml;
  void *po = nullptr, *pml = nullptr;
  if (num_splits > 1 && !in_wg) {
    auto opts = q.options().dtype(torch::kFloat32);
    partial_o = torch::empty({num_splits, num_seqs, num_q_heads, head_dim}, opts);
    partial_ml = torch::empty({num_splits, num_seqs, num_q_heads, 2}, opts);
    po = partial_o.data_ptr();
    pml = partial_ml.data_ptr();
  }
  launch_decode_attention(out.data_ptr(), po, pml, q.data_ptr(),
                          key_cache.data_ptr(), value_cache.data_ptr(),
                          block_tables.data_ptr(), context_lens.data_ptr(),
                          (float)scale, num_seqs, num_q_heads, num_kv_heads,
                          page_size, max_pages, (int)num_splits, (int)variant,
                          (int)q.stride(0), in_wg, current_stream());
  return out;
}

// ---- FP8 (OCP e4m3fn) paged KV cache --------------------------------------
// Separate entry points: the bf16 ones above keep rejecting every non-bf16
// cache.  Scales are powers of two given as integer exponents.

float check_scale_log2(int64_t e, const char* name) {
  TORCH_CHECK(e >= -16 && e <= 16, name, " must be in [-16, 16], got ", e);
  return std::ldexp(1.0f, (int)e);
}

void check_fp8_cache(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.scalar_type() == torch::kFloat8_e4m3fn, name,
              " must be float8_e4m3fn");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.dim() == 4, name,
              " must be [pages, KVH, page_size, head_dim]");
  const int64_t page_size = t.size(2);
  TORCH_CHECK(page_size > 0 && (page_size & (page_size - 1)) == 0,
              "page_size must be a power of two");
  TORCH_CHECK(t.size(1) > 0, "cache needs at least one KV head");
  TORCH_CHECK(t.size(3) == 128, "fp8 cache head_dim must be 128");
  TORCH_CHECK(t.numel() / 128 <= INT32_MAX, "cache has too many slots");
}

void check_fp8_caches(const torch::Tensor& key_cache,
                      const torch::Tensor& value_cache) {
  TORCH_CHECK(key_cache.scalar_type() == value_cache.scalar_type(),
              "key_cache/value_cache dtype mismatch");
  check_fp8_cache(key_cache, "key_cache");
  check_fp8_cache(value_cache, "value_cache");
  TORCH_CHECK(value_cache.sizes() == key_cache.sizes(),
              "key_cache/value_cache shape mismatch");
  TORCH_CHECK(value_cache.device() == key_cache.device(),
              "key_cache/value_cache device mismatch");
}

void rope_store_kv_fp8(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                       torch::Tensor key_cache, torch::Tensor value_cache,
                       torch::Tensor cos_sin, torch::Tensor positions,
                       torch::Tensor slot_mapping, int64_t k_scale_log2,
                       int64_t v_scale_log2) {
  check_bf16_rowslice(q, "q");
  check_bf16_rowslice(k, "k");
  check_bf16_rowslice(v, "v");
  TORCH_CHECK(k.stride(0) == v.stride(0), "k/v stride mismatch");
  check_fp8_caches(key_cache, value_cache);
  const float k_inv = check_scale_log2(-k_scale_log2, "kv_k_scale_log2");
  const float v_inv = check_scale_log2(-v_scale_log2, "kv_v_scale_log2");
  check_i32_gpu(positions, "positions");
  check_i32_gpu(slot_mapping, "slot_mapping");
  TORCH_CHECK(cos_sin.scalar_type() == torch::kFloat32 && cos_sin.is_cuda() &&
              cos_sin.is_contiguous() && cos_sin.dim() == 2,
              "cos_sin must be a contiguous 2-D fp32 GPU tensor");
  const int tokens = q.size(0);
  const int num_kv_heads = key_cache.size(1);
  const int page_size = key_cache.size(2);
  TORCH_CHECK(cos_sin.size(1) == 128,
              "cos_sin row width must equal the cache head_dim");
  TORCH_CHECK(k.size(0) == tokens && v.size(0) == tokens &&
              positions.numel() == tokens && slot_mapping.numel() == tokens,
              "q/k/v/positions/slot_mapping token counts differ");
  const int64_t q_width = q.numel() / std::max(tokens, 1);
  const int64_t k_width = k.numel() / std::max(tokens, 1);
  const int64_t v_width = v.numel() / std::max(tokens, 1);
  TORCH_CHECK(k_width == (int64_t)num_kv_heads * 128 && v_width == k_width,
              "k/v rows must be cache KVH * head_dim wide");
  TORCH_CHECK(q_width % 128 == 0,
              "q row width must be a multiple of the cache head_dim");
  // V rows are read as 16-byte vectors
  TORCH_CHECK(reinterpret_cast<uintptr_t>(v.data_ptr()) % 16 == 0 &&
              v.stride(0) % 8 == 0, "v rows must be 16-byte aligned");
  if (tokens == 0) return;
  launch_rope_store_kv_fp8(q.data_ptr(), k.data_ptr(), v.data_ptr(),
                           key_cache.data_ptr(), value_cache.data_ptr(),
                           cos_sin.data_ptr(), positions.data_ptr(),
                           slot_mapping.data_ptr(), tokens,
                           (int)(q_width / 128), num_kv_heads, page_size,
                           (int)q.stride(0), (int)k.stride(0), k_inv, v_inv,
                           current_stream());
}

torch::Tensor kv_gather_dequant(torch::Tensor cache, torch::Tensor slots,
                                int64_t scale_log2) {
  check_fp8_cache(cache, "cache");
  check_i32_gpu(slots, "slots");
  TORCH_CHECK(slots.dim() == 1 && slots.device() == cache.device(),
              "slots must be 1-D on the cache's device");
  const float scale = check_scale_log2(scale_log2, "scale_log2");
  const int64_t tokens = slots.numel();
  const int num_kv_heads = cache.size(1);
  auto out = torch::empty({tokens, (int64_t)num_kv_heads, (int64_t)128},
                          cache.options().dtype(torch::kBFloat16));
  if (tokens == 0) return out;
  launch_kv_gather_dequant(out.data_ptr(), cache.data_ptr(), slots.data_ptr(),
                           (long)tokens, (int)(cache.numel() / 128 /
                                               num_kv_heads),
                           num_kv_heads, (int)cache.size(2), scale,
                           current_stream());
  return out;
}

torch::Tensor decode_attention_fp8(torch::Tensor q, torch::Tensor key_cache,
                                   torch::Tensor value_cache,
                                   torch::Tensor block_tables,
                                   torch::Tensor context_lens, double scale,
                                   int64_t num_splits, int64_t k_scale_log2,
                                   int64_t v_scale_log2,
                                   int64_t combine = 0) {
  TORCH_CHECK(q.is_cuda() && q.scalar_type() == torch::kBFloat16 &&
              q.dim() == 3 && q.stride(2) == 1 &&
              q.stride(1) == q.size(2), "q must be [T, QH, D] row-sliced");
  const int num_seqs = q.size(0);
  const int num_q_heads = q.size(1);
  TORCH_CHECK(q.size(2) == 128, "head_dim must be 128");
  check_fp8_caches(key_cache, value_cache);
  TORCH_CHECK(key_cache.size(2) == 16,
              "fp8 decode needs a page size of 16");
  const float k_scale = check_scale_log2(k_scale_log2, "kv_k_scale_log2");
  const float v_scale = check_scale_log2(v_scale_log2, "kv_v_scale_log2");
  const int num_kv_heads = key_cache.size(1);
  TORCH_CHECK(num_q_heads % num_kv_heads == 0,
              "q heads must be a multiple of the cache KV heads");
  const int qpg = num_q_heads / num_kv_heads;
  TORCH_CHECK(qpg == 1 || qpg == 2 || qpg == 4 || qpg == 8,
              "GQA group must be 1/2/4/8");
  check_i32_gpu(block_tables, "block_tables");
  check_i32_gpu(context_lens, "context_lens");
  TORCH_CHECK(block_tables.dim() == 2 && block_tables.size(0) == num_seqs,
              "block_tables must be [num_seqs, max_pages]");
  TORCH_CHECK(context_lens.dim() == 1 && context_lens.size(0) == num_seqs,
              "context_lens must be [num_seqs]");
  TORCH_CHECK(num_splits >= 1, "num_splits must be >= 1");
  const bool in_wg =
      pick_in_wg_combine(combine, num_splits, true, "the fp8 kernel");
  const int max_pages = block_tables.size(1);
  auto out = torch::empty({num_seqs, num_q_heads, 128}, q.options());
  if (num_seqs == 0) return out;
  torch::Tensor partial_o, partial_ml;
  void *po = nullptr, *pml = nullptr;
  if (num_splits > 1 && !in_wg) {
    auto opts = q.options().dtype(torch::kFloat32);
    partial_o = torch::empty({num_splits, num_seqs, num_q_heads, 128}, opts);
    partial_ml = torch::empty({num_splits, num_seqs, num_q_heads, 2}, opts);
    po = partial_o.data_ptr();
    pml = partial_ml.data_ptr();
  }
  // 2^ek folds into the score scale: a power of two, so the product is exact
  launch_decode_attention_fp8(out.data_ptr(), po, pml, q.data_ptr(),
                              key_cache.data_ptr(), value_cache.data_ptr(),
                              block_tables.data_ptr(),
                              context_lens.data_ptr(), (float)scale * k_scale,
                              v_scale, num_seqs, num_q_heads, num_kv_heads,
                              max_pages, (int)num_splits, (int)q.stride(0),
                              in_wg, current_stream());
  return out;
}

torch::Tensor prefill_attention(torch::Tensor q, torch::Tensor k,
                                torch::Tensor v, torch::Tensor block_info,
                                torch::Tensor seq_lens, double scale,
                                int64_t swz) {
  auto rowsliced3 = [](const torch::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kBFloat16 &&
                t.dim() == 3 && t.stride(2) == 1 &&
                t.stride(1) == t.size(2), name,
                " must be [T, H, D] row-sliced");
  };
  rowsliced3(q, "q");
  rowsliced3(k, "k");
  rowsliced3(v, "v");
  TORCH_CHECK(k.stride(0) == v.stride(0), "k/v stride mismatch");
  TORCH_CHECK(q.size(2) == 128, "head_dim must be 128");
  TORCH_CHECK(block_info.scalar_type() == torch::kInt32, "block_info int32");
  TORCH_CHECK(seq_lens.scalar_type() == torch::kInt32, "seq_lens int32");
  const int nblocks = block_info.size(0);
  const int num_q_heads = q.size(1);
  const int num_kv_heads = k.size(1);
  auto out = torch::empty({q.size(0), (int64_t)num_q_heads, (int64_t)128},
                          q.options());
  launch_prefill_attention(out.data_ptr(), q.data_ptr(), k.data_ptr(),
                           v.data_ptr(), block_info.data_ptr(),
                           seq_lens.data_ptr(), (float)scale, nblocks,
                           num_q_heads, num_kv_heads, (int)swz,
                           (int)q.stride(0), (int)k.stride(0),
                           current_stream());
  return out;
}

torch::Tensor mfma_probe(torch::Tensor a, torch::Tensor b, int64_t a_split,
                         int64_t b_split) {
  auto d = torch::zeros({16, 16}, a.options().dtype(torch::kFloat32));
  launch_mfma_probe(d.data_ptr(), a.data_ptr(), b.data_ptr(), (int)a_split,
                    (int)b_split, current_stream());
  return d;
}

torch::Tensor mfma_probe32(torch::Tensor a, torch::Tensor b, int64_t a_split,
                           int64_t b_split, int64_t dmap) {
  auto d = torch::zeros({32, 32}, a.options().dtype(torch::kFloat32));
  launch_mfma_probe32(d.data_ptr(), a.data_ptr(), b.data_ptr(), (int)a_split,
                      (int)b_split, (int)dmap, current_stream());
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

// The 64-column-panel kernel (skinny_gemm_wide_kernel): 8 waves over
// 4 row groups of at most 2 m-tiles, whole 64-column panels.
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

// Shape, dtype, device and contiguity checks shared by skinny_gemm and
// skinny_gemm_add_rmsnorm, then the GEMM launch.  Returns the split count;
// with splits > 1 the f32 partials [splits, M, N] are left in `ws` for the
// caller to fold, with splits == 1 the bf16 result is in `c`.
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
  // only SPLITS 1/2/4/8 are instantiated, and each split's k range must be
  // whole 256-k groups (an even, >= 4 step count): anything else would
  // launch a kernel whose grid and workspace disagree with its k span
  TORCH_CHECK(force_splits == 0 || force_splits == 1 || force_splits == 2 ||
                  force_splits == 4 || force_splits == 8,
              "force_splits must be 0 (auto), 1, 2, 4 or 8");
  TORCH_CHECK(force_splits == 0 || K % (force_splits * 256) == 0,
              "K must be a multiple of force_splits * 256");
  TORCH_CHECK(panel == 0 || panel == 32 || panel == 64,
              "panel must be 0 (auto), 32 or 64");
  TORCH_CHECK(panel != 64 || skinny_gemm_wide_supported(M, N),
              "panel 64 needs M <= 128 and N % 64 == 0");
  const int splits = force_splits > 0 ? (int)force_splits
                                      : pick_gemm_splits((int)N, (int)K);
  if (panel == 0) panel = pick_gemm_panel(M, N);
  void* cp = nullptr;
  void* wsp = nullptr;
  if (splits > 1) {
    ws = torch::empty({splits, M, N}, a.options().dtype(torch::kFloat32));
    wsp = ws.data_ptr();
  } else {
    c = torch::empty({M, N}, a.options());
    cp = c.data_ptr();
  }
  (panel == 64 ? launch_skinny_gemm_wide : launch_skinny_gemm)(
      cp, wsp, a.data_ptr(), w.data_ptr(), (int)M, (int)N, (int)K, splits,
      current_stream());
  return splits;
}

}  // namespace

torch::Tensor skinny_gemm(torch::Tensor a, torch::Tensor w,
                          int64_t force_splits = 0, int64_t panel = 0) {
  torch::Tensor c, ws;
  const int splits = skinny_gemm_launch(a, w, force_splits, panel, c, ws);
  if (splits > 1) {
    c = torch::empty({a.size(0), w.size(0)}, a.options());
    launch_reduce_splits(c.data_ptr(), ws.data_ptr(), splits,
                         (long)c.numel(), current_stream());
  }
  return c;
}

// h = rmsnorm(a w^T + residual) * norm_weight with residual := a w^T +
// residual in place: bit for bit skinny_gemm followed by fused_add_rmsnorm,
// but the split-K fold happens in the norm kernel's prologue instead of a
// reduce_splits launch (and a bf16 round trip) of its own.
torch::Tensor skinny_gemm_add_rmsnorm(torch::Tensor a, torch::Tensor w,
                                      torch::Tensor residual,
                                      torch::Tensor norm_weight, double eps,
                                      int64_t force_splits = 0,
                                      int64_t panel = 0) {
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
  torch::Tensor c, ws;
  const int splits = skinny_gemm_launch(a, w, force_splits, panel, c, ws);
  const int M = (int)a.size(0), N = (int)w.size(0);
  if (splits == 1) {
    launch_fused_add_rmsnorm(c.data_ptr(), residual.data_ptr(),
                             norm_weight.data_ptr(), (float)eps, M, N,
                             current_stream());
    return c;
  }
  c = torch::empty({a.size(0), w.size(0)}, a.options());
  launch_fold_add_rmsnorm(c.data_ptr(), ws.data_ptr(), residual.data_ptr(),
                          norm_weight.data_ptr(), (float)eps, splits, M, N,
                          current_stream());
  return c;
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
  launch_sample(tokens.data_ptr(), kept.data_ptr(), logits.data_ptr(),
                temperature.data_ptr(), top_k.data_ptr(), top_p.data_ptr(),
                min_p.data_ptr(), seed.data_ptr(), pos.data_ptr(), (int)n,
                (int)V, current_stream());
  return {tokens, kept};
}

// ---- KV-pool IPC export + xGMI peer push (parallel/kv_peer.py) -----------
// The decode engine's KV pool is allocated with hipMalloc directly (not the
// caching allocator) so data_ptr() IS the allocation base hipIpcGetMemHandle
// requires; the prefill process maps it with lazy peer access (the xGMI
// route) and pushes pages with the kv_peer_copy kernel.

torch::Tensor ipc_alloc_bf16(std::vector<int64_t> sizes) {
  int64_t numel = 1;
  for (auto s : sizes) numel *= s;
  void* ptr = nullptr;
  hipError_t err = hipMalloc(&ptr, numel * 2);
  TORCH_CHECK(err == hipSuccess, "hipMalloc(", numel * 2,
              " B) failed: ", hipGetErrorString(err));
  int dev = 0;
  (void)hipGetDevice(&dev);
  auto opts = torch::TensorOptions()
                  .dtype(torch::kBFloat16)
                  .device(torch::kCUDA, dev);
  return torch::from_blob(
      ptr, sizes, [](void* p) { (void)hipFree(p); }, opts);
}

// The same allocation for any element type (the fp8 KV pool).
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
  launch_kv_peer_copy(reinterpret_cast<void*>(dst_base), src_kv.data_ptr(),
                      src_pages.data_ptr(), dst_pages.data_ptr(), n_pages,
                      2 * layers, (int)chunk_vec, chunk_vec,
                      chunk_vec, Ps * chunk_vec, dst_num_pages * chunk_vec,
                      current_stream());
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
  launch_xgmi_allreduce(out.data_ptr(), inp.data_ptr(), sp, dp, world,
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
