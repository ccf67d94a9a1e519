// The host interface of the kernels: the only declaration of every launcher.
// bindings.cpp and each .hip file that defines one include this header, so a
// definition that drifts from its declaration is a "conflicting types"
// compile error instead of a call that passes the wrong registers.
//
// Every launcher returns hipErrorInvalidValue, with nothing launched, when it
// has no kernel for its arguments, and hipGetLastError() after its last
// launch otherwise.  No device code and no torch in here.
#pragma once

#include <hip/hip_runtime_api.h>

// RoPE on q and k in place + the paged KV write, for a bf16 cache
// (launch_rope_store_kv) and an e4m3 one (launch_rope_store_kv_fp8).
struct RopeStoreLaunch {
  void* q;                   // [T, QH * D] bf16, rows q_stride apart
  void* k;                   // [T, KVH * D] bf16, rows kv_stride apart
  const void* v;             // as k
  void* key_cache;           // [pages, KVH, page_size, D]
  void* val_cache;
  const void* cos_sin;       // [max_pos, D] f32
  const void* positions;     // [T] int32
  const void* slot_mapping;  // [T] int32, -1 skips the write
  int tokens;
  int num_q_heads;
  int num_kv_heads;
  int head_dim;              // the e4m3 kernel has 128 only
  int page_size;
  int q_stride;              // token strides in elements
  int kv_stride;
  float k_inv_scale;         // 2^-ek, 2^-ev: e4m3 only
  float v_inv_scale;
};

// What the bf16 and the e4m3 decode launchers share.  head_dim is 128.
struct DecodeLaunch {
  void* out;                 // [seqs, QH, 128] bf16
  void* partial_o;           // [splits, seqs, QH, 128] f32, null if unused
  void* partial_ml;          // [splits, seqs, QH, 2] f32, null if unused
  const void* q;             // [seqs, QH, 128] bf16, rows q_stride apart
  const void* key_cache;     // [pages, KVH, page_size, 128]
  const void* val_cache;
  const void* block_tables;  // [seqs, max_pages] int32
  const void* context_lens;  // [seqs] int32
  float scale;               // softmax scale (times 2^ek for e4m3)
  int num_seqs;
  int num_q_heads;
  int num_kv_heads;
  int max_pages;
  int num_splits;
  int q_stride;
  // the splits are the waves of one workgroup (num_splits 2 or 4, 16-token
  // pages, variant 4 or e4m3) and the partials are unused
  bool in_wg;
};

struct PrefillLaunch {
  void* out;                 // [T, QH, 128] bf16
  const void* q;             // [T, QH, 128] bf16, rows q_stride apart
  const void* k;             // [Tk, KVH, 128] bf16, rows kv_stride apart
  const void* v;
  const void* block_info;    // [nblocks, 4] int32
  const void* seq_lens;      // [nblocks] int32
  float scale;
  int nblocks;
  int num_q_heads;
  int num_kv_heads;
  int swz;                   // kernel choice, see prefill_kernel()
  int q_stride;
  int kv_stride;
};

// Prefill that reads K/V in place from the paged pool (16-token pages,
// head_dim 128); fp8 picks the e4m3 instantiation.
struct PrefillPagedLaunch {
  void* out;                 // [T, QH, 128] bf16
  const void* q;             // [T, QH, 128] bf16, rows q_stride apart
  const void* key_cache;     // [pages, KVH, 16, 128] bf16 or e4m3
  const void* val_cache;
  const void* block_tables;  // [num_seqs, max_pages] int32
  const void* block_info;    // [nblocks, 4] int32, column 2 = sequence index
  const void* seq_lens;      // [nblocks] int32
  float scale;               // softmax scale (times 2^ek for e4m3)
  float v_scale;             // 2^ev, e4m3 only
  int nblocks;
  int num_seqs;              // rows of block_tables: the kernel clamps to them
  int max_pages;
  int num_q_heads;
  int num_kv_heads;
  int q_stride;
  bool fp8;
};

// Strides and chunk_vec count 16-byte vectors.
struct KvPeerCopyLaunch {
  void* dst_base;            // peer-mapped pool
  const void* src_base;      // local pool
  const void* src_pages;     // [n_pages] int32
  const void* dst_pages;     // [n_pages] int32
  int n_pages;
  int n_chunks;              // 2 * layers
  int chunk_vec;             // one (layer, k|v, page) chunk
  long src_page_stride_vec;
  long dst_page_stride_vec;
  long src_chunk_stride_vec;
  long dst_chunk_stride_vec;
};

// The three launches behind the grouping of a mixture-of-experts FFN
// (moe.hip): grouped gate_up + SwiGLU, grouped down, weighted combine.
// 1 <= k <= 8, E <= 256, H % 256 == 0, I % 64 == 0.  format tells what w1
// and w2 hold.  BF16: w1_exp and w2_exp are null.  E4M3: bytes, and the
// exponents one int8 per expert output row, 4-byte aligned.  MXFP4: e2m1
// codes, two per byte (w1 [E, 2 * I, H / 2], w2 [E, H, I / 2], 16-byte
// aligned), and the exponents one int8 per 32 k of a row.
struct MoeFfnLaunch {
  enum Format { BF16, E4M3, MXFP4 };
  void* y;                     // [T, H] bf16
  void* h;                     // [T * k, I] bf16 workspace, sorted order
  void* opart;                 // [T * k, H] f32 workspace, pair order
  const void* x;               // [T, H] bf16
  const void* w1;              // [E, 2 * I, H]: gate rows, then up rows
  const void* w2;              // [E, H, I]
  const void* weights;         // [T, k] f32
  const void* expert_offsets;  // [E + 1] int32
  const void* sorted_pairs;    // [T * k] int32: pairs t * k + j by expert
  int T, k, E, H, I;
  const void* w1_exp = nullptr;  // [E, 2 * I] int8; MXFP4 [E, 2 * I, H / 32]
  const void* w2_exp = nullptr;  // [E, H] int8; MXFP4 [E, H, I / 32]
  Format format = BF16;
};

extern "C" {

// Top-k routing of bf16 logits [T, E] plus the grouping of the T * k pairs
// by expert, one launch; ticket is one int32 that is zero between launches.
// launch_moe_group is the grouping alone, for ids from elsewhere.
hipError_t launch_moe_route(void* ids, void* weights, void* expert_offsets,
                            void* sorted_pairs, void* ticket,
                            const void* logits, int T, int E, int k,
                            int renormalize, hipStream_t stream);
hipError_t launch_moe_group(void* expert_offsets, void* sorted_pairs,
                            const void* ids, int n, int E, hipStream_t stream);
hipError_t launch_moe_ffn(const MoeFfnLaunch& a, hipStream_t stream);

hipError_t launch_rmsnorm(void* out, void* input, const void* weight,
                          float eps, int tokens, int hidden,
                          hipStream_t stream);
hipError_t launch_fused_add_rmsnorm(void* input, void* residual,
                                    const void* weight, float eps, int tokens,
                                    int hidden, hipStream_t stream);
hipError_t launch_fold_add_rmsnorm(void* out, const void* ws, void* residual,
                                   const void* weight, float eps, int splits,
                                   int tokens, int hidden, hipStream_t stream);
hipError_t launch_silu_mul(void* out, const void* x, int tokens, int inter,
                           hipStream_t stream);

hipError_t launch_rope_store_kv(const RopeStoreLaunch& a, hipStream_t stream);
hipError_t launch_rope_store_kv_fp8(const RopeStoreLaunch& a,
                                    hipStream_t stream);
hipError_t launch_kv_gather_dequant(void* out, const void* cache,
                                    const void* slots, long tokens,
                                    int num_slots, int num_kv_heads,
                                    int page_size, float scale,
                                    hipStream_t stream);

hipError_t launch_decode_attention(const DecodeLaunch& a, int page_size,
                                   int variant, hipStream_t stream);
hipError_t launch_decode_attention_fp8(const DecodeLaunch& a, float v_scale,
                                       hipStream_t stream);
hipError_t launch_prefill_attention(const PrefillLaunch& a,
                                    hipStream_t stream);
hipError_t launch_prefill_attention_paged(const PrefillPagedLaunch& a,
                                          hipStream_t stream);

hipError_t launch_mfma_probe(void* d, const void* a, const void* b,
                             int a_split, int b_split, hipStream_t stream);
hipError_t launch_mfma_probe32(void* d, const void* a, const void* b,
                               int a_split, int b_split, int dmap,
                               hipStream_t stream);

// c: bf16 [M, N] when splits == 1, else ws: f32 [splits, M, N]
hipError_t launch_skinny_gemm(void* c, void* ws, const void* a, const void* w,
                              int M, int N, int K, int splits,
                              hipStream_t stream);
hipError_t launch_skinny_gemm_wide(void* c, void* ws, const void* a,
                                   const void* w, int M, int N, int K,
                                   int splits, hipStream_t stream);
hipError_t launch_reduce_splits(void* c, const void* ws, int splits, long mn,
                                hipStream_t stream);

// FP8 weights (skinny_gemm_w8.hip): w8 e4m3 [N, K] with one power-of-two
// exponent per row, e int8 [N].  The GEMM has 1 <= M <= 128, N % 64 == 0,
// K % (splits * 256) == 0 and writes c / ws as launch_skinny_gemm does, the
// rows already scaled; the dequant writes bf16 [N, K], K % 16 == 0.
hipError_t launch_skinny_gemm_w8(void* c, void* ws, const void* a,
                                 const void* w8, const void* e, int M, int N,
                                 int K, int splits, hipStream_t stream);
hipError_t launch_w8_dequant(void* out, const void* w8, const void* e, long N,
                             long K, hipStream_t stream);

hipError_t launch_sample(void* out_tok, void* out_kept, const void* logits,
                         const void* temperature, const void* top_k,
                         const void* top_p, const void* min_p,
                         const void* seed, const void* pos, int n, int V,
                         hipStream_t stream);

hipError_t launch_kv_peer_copy(const KvPeerCopyLaunch& a, hipStream_t stream);

hipError_t launch_xgmi_allreduce(void* out, const void* in, void** sig_ptrs,
                                 void** data_ptrs, int world, int rank, long n,
                                 hipStream_t stream);
long xgmi_allreduce_signal_bytes();
long xgmi_allreduce_error_offset();
long xgmi_allreduce_counter_offset();

}  // extern "C"
