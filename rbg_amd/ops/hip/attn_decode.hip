// Paged flash-decode attention (gfx950) — single query token per sequence.
//
// HBM-bound: the cost is streaming the sequence's paged K/V once, with all
// q-heads of a kv-head (the GQA group, QPG) computed in one pass so K/V
// bytes are read exactly once.  Split-KV partitions ("flash-decoding") keep
// the chip full at small batch; partials merge in decode_combine_kernel via
// the (m, l) log-sum-exp algebra.
//
// Kernels, selected at run time by `variant` (RBG_DECODE_VARIANT):
//   0-3  decode_attn_kernel: the dot2 family.  K/V rows (128 bf16, 256 B)
//        are read as 16-byte lane vectors by 16-lane groups, 4 keys per
//        wave-instruction; any power-of-two page size.
//   4,5  decode_attn_mfma_kernel: 32-key page-pair tiles on
//        v_mfma_f32_16x16x32_bf16, one wave per sequence (5 = register
//        diet).  4 is the default.
//   6    decode_attn_pc_kernel: the same math split into a producer and a
//        consumer wave.
// Variants 4-6 need page_size == 16; with any other page size, and for
// out-of-range variants, the launcher falls back to variant 1.
// An FP8 (e4m3) cache has one kernel of its own, decode_attn_mfma_fp8_kernel:
// variant 4 with a dequantising stage (launch_decode_attention_fp8).
//
// Capability analog: the decode-side paged attention of the engines the
// reference orchestrates (SURVEY §2.3 decode engine row).
#include "attn_mfma.h"

namespace {

// Keys and 16-token pages of one split: the context is cut into 16-key
// chunks, ceil-divided over the splits (tests/attn_cases._split_range
// mirrors this rule).  A trailing split may be empty (key_begin >= key_end).
struct SplitRange { int key_begin, key_end, pg_begin, pg_end; };

DEV_INLINE SplitRange split_range(int ctx, int split, int num_splits) {
  const int chunk = 16;
  const int nchunks = (ctx + chunk - 1) / chunk;
  const int per_split = (nchunks + num_splits - 1) / num_splits;
  SplitRange r;
  r.key_begin = split * per_split * chunk;
  r.key_end = min(ctx, (split + 1) * per_split * chunk);
  r.pg_begin = r.key_begin >> 4;
  r.pg_end = (r.key_end + 15) >> 4;
  return r;
}

// QPG = q heads per kv head (GQA group). One block = (seq, kv_head, split).
// 4 waves; each wave covers 4 keys per iteration (16-lane groups, 16 B/lane).
// VARIANT 0: f32 FMA scores (more VGPRs, 3-4 waves/SIMD), 1-ahead prefetch;
// VARIANT 1: packed-bf16 v_dot2 scores (96 VGPRs, 5 waves/SIMD for QPG<=4);
// VARIANT 2: variant 1 with the page-table address one more iteration ahead;
// VARIANT 3: variant 1 with a 2-ahead K/V prefetch in named register pairs.
template <int QPG, int VARIANT>
__global__ __launch_bounds__(256,
    (VARIANT == 3) ? 4 : ((VARIANT >= 1 && QPG <= 4) ? 5 : 2))
// V3 doubles the in-flight K/V state: 4 waves/SIMD (128-VGPR budget) so
// the extra pairs stay in registers instead of spilling
void decode_attn_kernel(
    float* __restrict__ partial_o,        // [splits, seqs, QH, D]
    float* __restrict__ partial_ml,       // [splits, seqs, QH, 2]
    __hip_bfloat16* __restrict__ out,     // [seqs, QH, D] (splits==1 path)
    const __hip_bfloat16* __restrict__ q, // [seqs, QH, D]
    const __hip_bfloat16* __restrict__ key_cache,  // [pages, KVH, page, D]
    const __hip_bfloat16* __restrict__ val_cache,
    const int* __restrict__ block_tables, // [seqs, max_pages]
    const int* __restrict__ context_lens, // [seqs]
    const float scale, const int num_kv_heads, const int page_size,
    const int max_pages, const int num_splits, const int q_stride) {
  const int kvh = blockIdx.x;
  const int seq = blockIdx.y;
  const int split = blockIdx.z;
  const int num_q_heads = num_kv_heads * QPG;
  const int ctx = context_lens[seq];

  const int tid = threadIdx.x;
  const int wave = tid >> 6;
  const int lane = tid & 63;
  const int group = lane >> 4;        // which of the wave's 4 keys
  const int gl = lane & 15;           // lane within the 16-lane group
  const int dbase = gl * 8;           // this lane's 8 dims

  const SplitRange sr = split_range(ctx, split, num_splits);
  const int key_begin = sr.key_begin, key_end = sr.key_end;

  // q fragment: VARIANT 1 keeps it packed bf16 (v_dot2 pairs, half the
  // registers); VARIANT 0 pre-converts to f32 with the scale folded in
  typedef __attribute__((ext_vector_type(2))) __bf16 bfpair;
  bfpair qp[VARIANT >= 1 ? QPG : 1][4];
  float qf[VARIANT == 0 ? QPG : 1][8];
  {
    const __hip_bfloat16* qrow =
        q + (size_t)seq * q_stride + (size_t)kvh * QPG * HEAD_DIM;
#pragma unroll
    for (int h = 0; h < QPG; ++h) {
      Bf16x8U qv;
      qv.u = *reinterpret_cast<const uint4*>(qrow + h * HEAD_DIM + dbase);
      if (VARIANT >= 1) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          qp[h][j] = reinterpret_cast<const bfpair*>(&qv)[j];
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) qf[h][j] = bf2f(qv.e[j]) * scale;
      }
    }
  }

  float m[QPG], l[QPG], acc[QPG][8];
#pragma unroll
  for (int h = 0; h < QPG; ++h) {
    m[h] = NEG_INF;
    l[h] = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[h][j] = 0.f;
  }

  const int* btab = block_tables + (size_t)seq * max_pages;
  // page_size is a power of two (engine config); shift/mask beats idiv
  const int ps_shift = 31 - __clz(page_size);
  const int ps_mask = page_size - 1;

  auto row_offset = [&](int base) -> size_t {
    const int key = base + group;
    const int kslot = key < key_end ? key : key_begin;  // clamp: safe addr
    const int page = btab[kslot >> ps_shift];
    return (((size_t)page * num_kv_heads + kvh) * page_size +
            (kslot & ps_mask)) * HEAD_DIM;
  };

  // One 4-key quad of online-softmax work (scores via 16-lane-group dot
  // reduction, tile max/psum across the wave's quad, V accumulate).
  auto process4 = [&](const Bf16x8U& kv, const Bf16x8U& vv, bool valid) {
    const bfpair* kp = reinterpret_cast<const bfpair*>(&kv);
    float kf[VARIANT == 0 ? 8 : 1];
    if (VARIANT == 0) {
#pragma unroll
      for (int j = 0; j < 8; ++j) kf[j] = bf2f(kv.e[j]);
    }
    float p[QPG];
    float tile_max[QPG];
#pragma unroll
    for (int h = 0; h < QPG; ++h) {
      float s = 0.f;
      if (VARIANT >= 1) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
          s = __builtin_amdgcn_fdot2_f32_bf16(qp[h][j], kp[j], s, false);
        s *= scale;
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) s += qf[h][j] * kf[j];
      }
      s = group16_sum(s);             // full dot across the 16-lane group
      if (!valid) s = NEG_INF;
      float tm = s;
      tm = fmaxf(tm, __shfl_xor(tm, 16, 64));
      tm = fmaxf(tm, __shfl_xor(tm, 32, 64));
      tile_max[h] = tm;
      p[h] = s;
    }
#pragma unroll
    for (int h = 0; h < QPG; ++h) {
      const float m_new = fmaxf(m[h], tile_max[h]);
      const float alpha = __expf(m[h] - m_new);
      const float pv = valid ? __expf(p[h] - m_new) : 0.f;
      float psum = pv;
      psum += __shfl_xor(psum, 16, 64);
      psum += __shfl_xor(psum, 32, 64);
      l[h] = l[h] * alpha + psum;
      m[h] = m_new;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        acc[h][j] = acc[h][j] * alpha + pv * bf2f(vv.e[j]);
    }
  };

  auto load_pair = [&](int b, Bf16x8U& kd, Bf16x8U& vd) {
    const size_t off = row_offset(b);
    kd.u = *reinterpret_cast<const uint4*>(key_cache + off + dbase);
    vd.u = *reinterpret_cast<const uint4*>(val_cache + off + dbase);
  };

  // 4 keys per wave-iteration with 1-ahead data prefetch.  (Wider 8-key
  // and 2-ahead-ring variants measured null-to-negative —
  // profiles/decode_breakdown.md.)  VARIANT 2 additionally computes the
  // page-table address one MORE iteration ahead so the btab read never
  // serializes in front of the K/V loads.
  if (VARIANT == 2) {
    int base = key_begin + wave * 4;
    Bf16x8U k_pref, v_pref;
    size_t off_next = 0;
    if (base < key_end) {
      const size_t off0 = row_offset(base);
      k_pref.u = *reinterpret_cast<const uint4*>(key_cache + off0 + dbase);
      v_pref.u = *reinterpret_cast<const uint4*>(val_cache + off0 + dbase);
      off_next = row_offset(base + 16);
    }
    for (; base < key_end; base += 16) {
      const bool valid = base + group < key_end;
      Bf16x8U kv = k_pref, vv = v_pref;
      k_pref.u = *reinterpret_cast<const uint4*>(key_cache + off_next + dbase);
      v_pref.u = *reinterpret_cast<const uint4*>(val_cache + off_next + dbase);
      off_next = row_offset(base + 32);
      process4(kv, vv, valid);
    }
  } else if (VARIANT == 3) {
    // 2-ahead prefetch with SCALAR named register pairs, unrolled by 2.
    // An earlier 2-ahead used a ring array indexed by (i & 1) — which the
    // compiler demoted to scratch memory (docs/cdna_lessons.md §1), so it
    // measured -22%; with named pairs both iterations' loads stay in
    // flight and the per-iteration vmcnt slack doubles.
    int base = key_begin + wave * 4;
    Bf16x8U k0, v0, k1, v1;
    // guarded like the other variants: for an EMPTY split key_begin lies
    // past the context, so row_offset's clamp-to-key_begin would index the
    // block table beyond the sequence's pages
    if (base < key_end) {
      load_pair(base, k0, v0);        // row_offset clamps out-of-range
      load_pair(base + 16, k1, v1);
    }
    for (; base < key_end; base += 32) {
      const bool valid0 = base + group < key_end;
      Bf16x8U a = k0, b = v0;
      load_pair(base + 32, k0, v0);
      process4(a, b, valid0);
      const bool valid1 = base + 16 + group < key_end;
      Bf16x8U c = k1, d = v1;
      load_pair(base + 48, k1, v1);
      process4(c, d, valid1);
    }
  } else {
    int base = key_begin + wave * 4;
    Bf16x8U k_pref, v_pref;
    if (base < key_end)
      load_pair(base, k_pref, v_pref);
    for (; base < key_end; base += 16) {
      const bool valid = base + group < key_end;
      Bf16x8U kv = k_pref, vv = v_pref;
      // unconditional clamped prefetch (row_offset clamps): a branch
      // around the loads forces a vmcnt drain per iteration (guide trap 4c)
      load_pair(base + 16, k_pref, v_pref);
      process4(kv, vv, valid);
    }
  }

  // fold the 4 key-groups of the wave (same dims, disjoint keys, same m/l)
#pragma unroll
  for (int h = 0; h < QPG; ++h)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      acc[h][j] += __shfl_xor(acc[h][j], 16, 64);
      acc[h][j] += __shfl_xor(acc[h][j], 32, 64);
    }

  // cross-wave combine through LDS
  __shared__ float lds_acc[4][QPG][HEAD_DIM];
  __shared__ float lds_ml[4][QPG][2];
  if (lane < 16) {
#pragma unroll
    for (int h = 0; h < QPG; ++h) {
#pragma unroll
      for (int j = 0; j < 8; ++j) lds_acc[wave][h][dbase + j] = acc[h][j];
      if (gl == 0) {
        lds_ml[wave][h][0] = m[h];
        lds_ml[wave][h][1] = l[h];
      }
    }
  }
  __syncthreads();

  // threads cover (head, dim): QPG*128 outputs
  for (int i = tid; i < QPG * HEAD_DIM; i += blockDim.x) {
    const int h = i / HEAD_DIM, d = i % HEAD_DIM;
    float m_star = NEG_INF;
#pragma unroll
    for (int w = 0; w < 4; ++w) m_star = fmaxf(m_star, lds_ml[w][h][0]);
    float o = 0.f, lsum = 0.f;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float f = __expf(lds_ml[w][h][0] - m_star);
      o += lds_acc[w][h][d] * f;
      lsum += lds_ml[w][h][1] * f;
    }
    const int qh = kvh * QPG + h;
    if (num_splits == 1) {
      out[((size_t)seq * num_q_heads + qh) * HEAD_DIM + d] =
          f2bf(lsum > 0.f ? o / lsum : 0.f);
    } else {
      partial_o[(((size_t)split * gridDim.y + seq) * num_q_heads + qh) *
                    HEAD_DIM + d] = o;
      if (d == 0) {
        float* ml = partial_ml +
            (((size_t)split * gridDim.y + seq) * num_q_heads + qh) * 2;
        ml[0] = m_star;
        ml[1] = lsum;
      }
    }
  }
}


// ---------------------------------------------------------------------------
// MFMA-tiled decode (variants 4-6): 32-key page-pair tiles on
// v_mfma_f32_16x16x32_bf16 — the prefill kernel's engine applied to decode.
// The dot2 kernel (V1) is latency-bound on its serial cross-lane shuffle
// chain (a group16 reduction round every 4 keys, SQ_WAIT_ANY 68%); here one
// MFMA chain scores 32 keys and the reduction round runs once per PAIR of
// pages (8x fewer), with PV through the same 32-k fragment +
// ds_read_b64_tr_b16 V image as attn_prefill.hip (attn_mfma.h).
//
// Layout notes:
//  * page_size must be 16: a KV page slice [16 tokens][128 d] is 4 KB
//    contiguous; two pages form one 32-key MFMA step.
//  * q A-fragment rows = the kv-head's QPG query heads (rows >= QPG
//    replicate the last head; their outputs are never written).
//  * S is C-layout: key col = lane&15, q row = 4*(lane>>4)+reg; the two
//    pages' columns combine lane-locally before ONE group16 max/sum.
// The pieces below are shared by the one-wave kernel (4/5) and the
// producer/consumer kernel (6).

constexpr int DM_KP = 132;      // K panel pitch (bf16)
constexpr int DM_PP = 40;       // P tile pitch (bf16)

// Merge of the splits' (O, m, l) partials of one output element by the
// log-sum-exp algebra, in split order.  decode_combine_kernel (partials in
// HBM) and the in-workgroup epilogue of the MFMA kernels (partials in LDS)
// both call it, so the two produce the same bits.  An empty split (m = -inf,
// l = 0) contributes 0 and a ctx == 0 row comes out 0.
template <class GetM, class GetL, class GetO>
DEV_INLINE __hip_bfloat16 merge_splits(int num_splits, GetM m_of, GetL l_of,
                                       GetO o_of) {
  float m_star = NEG_INF;
  for (int s = 0; s < num_splits; ++s) m_star = fmaxf(m_star, m_of(s));
  float o = 0.f, lsum = 0.f;
  for (int s = 0; s < num_splits; ++s) {
    const float f = __expf(m_of(s) - m_star);
    o += o_of(s) * f;
    lsum += l_of(s) * f;
  }
  return f2bf(lsum > 0.f ? o / lsum : 0.f);
}

// q A-fragments: row = head (clamped), 4 k-steps of 32 dims
template <int QPG>
DEV_INLINE void load_q_frags(bf8 (&qa)[4], const __hip_bfloat16* q_seq,
                             int kvh, int gl, int gslice) {
  const __hip_bfloat16* qrow =
      q_seq + (size_t)(kvh * QPG + min(gl, QPG - 1)) * HEAD_DIM;
#pragma unroll
  for (int ks = 0; ks < 4; ++ks)
    qa[ks] = load_bf8(qrow + ks * 32 + gslice * 8);
}

// S = q K^T over the pair's 32 keys (B-frag: key row = gl / gl+16)
DEV_INLINE void score_pair(f32x4& sA, f32x4& sB, const bf8 (&qa)[4],
                           const __hip_bfloat16* k_lds, int gl, int gslice) {
  sA = {0.f, 0.f, 0.f, 0.f};
  sB = sA;
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    const bf8 kfA = load_bf8(&k_lds[gl * DM_KP + ks * 32 + gslice * 8]);
    const bf8 kfB = load_bf8(&k_lds[(16 + gl) * DM_KP + ks * 32 + gslice * 8]);
    sA = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[ks], kfA, sA, 0, 0, 0);
    sB = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qa[ks], kfB, sB, 0, 0, 0);
  }
}

// Online softmax of the page pair starting at page pg: the lane holds rows
// 4*gslice+r for key cols (pg*16+gl, pg*16+16+gl); ONE group16 round covers
// both pages.  Rescales acc_o and leaves P (bf16) in p_lds.
DEV_INLINE void pair_softmax(const f32x4& sA, const f32x4& sB, float scale,
                             int pg, const SplitRange& sr, float (&m)[4],
                             float (&l)[4], f32x4 (&acc_o)[8],
                             __hip_bfloat16* p_lds, int gl, int gslice) {
  const int keyA = pg * 16 + gl;
  const int keyB = keyA + 16;
  const bool vA = keyA >= sr.key_begin && keyA < sr.key_end;
  const bool vB = keyB >= sr.key_begin && keyB < sr.key_end;
  float pA[4], pB[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const float a = vA ? sA[r] * scale : NEG_INF;
    const float b = vB ? sB[r] * scale : NEG_INF;
    const float tm = group16_max(fmaxf(a, b));
    const float m_new = fmaxf(m[r], tm);
    const float alpha = __expf(m[r] - m_new);
    pA[r] = vA ? __expf(a - m_new) : 0.f;
    pB[r] = vB ? __expf(b - m_new) : 0.f;
    l[r] = l[r] * alpha + group16_sum(pA[r] + pB[r]);
    m[r] = m_new;
#pragma unroll
    for (int dt = 0; dt < 8; ++dt) acc_o[dt][r] *= alpha;
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    p_lds[(4 * gslice + r) * DM_PP + gl] = f2bf(pA[r]);
    p_lds[(4 * gslice + r) * DM_PP + 16 + gl] = f2bf(pB[r]);
  }
}

// P A-fragment of the pair: row = gl, the lane's 8 keys from gslice*8
DEV_INLINE bf8 load_p_frag(const __hip_bfloat16* p_lds, int gl, int gslice) {
  union { uint4 u; bf8 v; } paf;
  const __hip_bfloat16* p = &p_lds[gl * DM_PP + gslice * 8];
  paf.u.x = *reinterpret_cast<const uint*>(p);
  paf.u.y = *reinterpret_cast<const uint*>(p + 2);
  paf.u.z = *reinterpret_cast<const uint*>(p + 4);
  paf.u.w = *reinterpret_cast<const uint*>(p + 6);
  return paf.v;
}

// Epilogue: the lane holds O rows 4*gslice+r at dim cols dt*16+gl.  One
// split writes the normalised output, more write (O, m, l) partials.
template <int QPG>
DEV_INLINE void store_pair_output(float* partial_o, float* partial_ml,
                                  __hip_bfloat16* out,
                                  const f32x4 (&acc_o)[8], const float (&m)[4],
                                  const float (&l)[4], int seq, int num_seqs,
                                  int split, int num_splits, int kvh,
                                  int num_kv_heads, int gl, int gslice) {
  const int num_q_heads = num_kv_heads * QPG;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = 4 * gslice + r;
    if (row >= QPG) continue;
    const int qh = kvh * QPG + row;
    if (num_splits == 1) {
      const float inv_l = l[r] > 0.f ? 1.f / l[r] : 0.f;
#pragma unroll
      for (int dt = 0; dt < 8; ++dt)
        out[((size_t)seq * num_q_heads + qh) * HEAD_DIM + dt * 16 + gl] =
            f2bf(acc_o[dt][r] * inv_l);
    } else {
#pragma unroll
      for (int dt = 0; dt < 8; ++dt)
        partial_o[(((size_t)split * num_seqs + seq) * num_q_heads + qh) *
                      HEAD_DIM + dt * 16 + gl] = acc_o[dt][r];
      if (gl == 0) {
        float* ml = partial_ml +
            (((size_t)split * num_seqs + seq) * num_q_heads + qh) * 2;
        ml[0] = m[r];
        ml[1] = l[r];
      }
    }
  }
}

// In-workgroup split merge (WS > 1): the WS waves of the workgroup are the WS
// splits of one (seq, kv_head).  Each wave parks the rows < QPG of its
// (O, m, l) partial as f32 in its OWN K/V panel (QPG x 128 + 2 QPG floats, at
// most 4.1 KB of the panel's 8.4 KB; same-wave DS ordering puts the writes
// behind the last PV reads), one barrier, then all 64 * WS threads share the
// QPG x 128 outputs and merge them in split order: what decode_combine_kernel
// does with partials from HBM, without the partials or the launch.
//
// The kernels call this when num_splits == WS and keep store_pair_output for
// every other multiple of WS (split = blockIdx.z * WS + wave).  The launcher
// starts them with num_splits == WS only, yet that second branch must stay:
// with this epilogue alone the compiler schedules the pair loop, whose source
// is the same, in another order (V's LDS writes and their vmcnt(0) ahead of
// the softmax, one shuffle in flight at a time), and bf16 B128 x 2048 at 2
// splits then LOSES 5.5 us to attention + combine kernel instead of winning
// 6.1 us (profiles/decode_fused_ab.json, both builds in one job).
// profiles/decode_wg_combine_resources.txt has the loop-by-loop comparison;
// after a compiler update or a change to either epilogue run
// tools/decode_loop_compare.py --check, which fails when the order moves.
template <int QPG, int WS>
DEV_INLINE void merge_in_workgroup(__hip_bfloat16* out, __hip_bfloat16* panels,
                                   const f32x4 (&acc_o)[8], const float (&m)[4],
                                   const float (&l)[4], int wave, int seq,
                                   int kvh, int num_kv_heads, int gl,
                                   int gslice) {
  constexpr int PANEL_F = 32 * DM_KP / 2;     // floats per K/V panel
  constexpr int ML = QPG * HEAD_DIM;          // m at ML + h, l at ML + QPG + h
  static_assert(ML + 2 * QPG <= PANEL_F, "partial does not fit the panel");
  float* part = reinterpret_cast<float*>(panels);
  float* mine = part + wave * PANEL_F;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int row = 4 * gslice + r;
    if (row >= QPG) continue;
#pragma unroll
    for (int dt = 0; dt < 8; ++dt)
      mine[row * HEAD_DIM + dt * 16 + gl] = acc_o[dt][r];
    if (gl == 0) {
      mine[ML + row] = m[r];
      mine[ML + QPG + row] = l[r];
    }
  }
  __syncthreads();
  const int num_q_heads = num_kv_heads * QPG;
  for (int i = threadIdx.x; i < QPG * HEAD_DIM; i += 64 * WS) {
    const int h = i / HEAD_DIM, d = i % HEAD_DIM;
    out[((size_t)seq * num_q_heads + kvh * QPG + h) * HEAD_DIM + d] =
        merge_splits(
            WS, [&](int s) { return part[s * PANEL_F + ML + h]; },
            [&](int s) { return part[s * PANEL_F + ML + QPG + h]; },
            [&](int s) { return part[s * PANEL_F + h * HEAD_DIM + d]; });
  }
}

// Global -> LDS staging of one page pair.  The lane covers K/V key row
// srow = lane>>1 (32 rows: page myloc = srow>>4 of the pair) and the 64-elem
// chunk schunk = (lane&1)*64, i.e. 8 x 16 B pieces; 2 lanes x 128 B = one
// contiguous page row.  The pieces live in NAMED SCALAR registers R0..R7
// (docs/cdna_lessons.md §1: local arrays are demoted to scratch memory,
// round-tripping every staged page via HBM).  The macros use the kernel's
// btab, pg_last, srow, schunk, myloc, k_lds and v_img.  Pages past the
// split clamp to its last real page (pg_last, itself clamped at 0 so a
// ctx == 0 row reads btab[0], never btab[-1]).
#define DM_REGS(R) uint4 R##0, R##1, R##2, R##3, R##4, R##5, R##6, R##7
#define DM_ISSUE(cache, R, pg)                                              \
  do {                                                                      \
    const int p_ = btab[min((pg) + myloc, pg_last)];                        \
    const __hip_bfloat16* src_ = (cache) + schunk +                         \
        (((size_t)p_ * num_kv_heads + kvh) * 16 + (srow & 15)) * HEAD_DIM;  \
    R##0 = *reinterpret_cast<const uint4*>(src_);                           \
    R##1 = *reinterpret_cast<const uint4*>(src_ + 8);                       \
    R##2 = *reinterpret_cast<const uint4*>(src_ + 16);                      \
    R##3 = *reinterpret_cast<const uint4*>(src_ + 24);                      \
    R##4 = *reinterpret_cast<const uint4*>(src_ + 32);                      \
    R##5 = *reinterpret_cast<const uint4*>(src_ + 40);                      \
    R##6 = *reinterpret_cast<const uint4*>(src_ + 48);                      \
    R##7 = *reinterpret_cast<const uint4*>(src_ + 56);                      \
  } while (0)
#define DM_K_AT(c) (&k_lds[srow * DM_KP + schunk + (c)])
#define DM_V_AT(c) (&v_img[v_img_off(srow, schunk + (c))])
#define DM_WRITE(R, AT)                                                     \
  do {                                                                      \
    *reinterpret_cast<uint4*>(AT(0)) = R##0;                                \
    *reinterpret_cast<uint4*>(AT(8)) = R##1;                                \
    *reinterpret_cast<uint4*>(AT(16)) = R##2;                               \
    *reinterpret_cast<uint4*>(AT(24)) = R##3;                               \
    *reinterpret_cast<uint4*>(AT(32)) = R##4;                               \
    *reinterpret_cast<uint4*>(AT(40)) = R##5;                               \
    *reinterpret_cast<uint4*>(AT(48)) = R##6;                               \
    *reinterpret_cast<uint4*>(AT(56)) = R##7;                               \
  } while (0)

// One wave per sequence (variant 4; DIET = variant 5), two sequences per
// 2-wave workgroup, 19 KB LDS per workgroup.  MFMA depth inside the wave
// covers the low waves/SIMD (the same budget shape as the 8-wave prefill
// kernel).
// DIET: the round-2 register diet targeting 4 waves/SIMD
// (docs/ROUND2_DESIGNS.md §1a+1b).  Two changes vs variant 4:
//  (a) q fragments are RELOADED from global per page pair instead of held
//      in 16 persistent VGPRs — the rows are the same cache lines every
//      pair, so after the first touch they come from L1.  Issued BEFORE
//      the V stage so the compiler's dependency waitcnt for the first S
//      MFMA is vmcnt(8) (V still in flight), not a pipeline drain.
//  (b) V issues AFTER the S MFMAs, when the q fragments are dead, so the
//      allocator colors V's staging registers into theirs, and PV runs in
//      two 4-tile halves (PV_STEP8) so only 16 tr-read VGPRs are live at a
//      time.  The round-67 FULL merge (one 8-set for K and V) hit in-loop
//      spills and lost 27%.
// The diet does not fit 128 VGPRs cleanly: with the compiler in this tree all
// four DIET instantiations spill (36-60 B of scratch per lane, see
// profiles/attn_refactor_resources.txt); variant 4 has no scratch.
// WS (workgroup splits): 1 is the layout above, with the split in blockIdx.z
// and decode_combine_kernel behind it when num_splits > 1.  WS = 2 or 4
// (variant 4) makes WS splits of ONE sequence the waves of a workgroup, grid
// (KVH, num_seqs, num_splits / WS); with num_splits == WS they merge in LDS
// (merge_in_workgroup): no partials in HBM, no second launch.
template <int QPG, int DIET, int WS = 1>
__global__ __launch_bounds__(WS == 1 ? 128 : 64 * WS, DIET ? 4 : 3)
void decode_attn_mfma_kernel(
    float* __restrict__ partial_o,        // [splits, seqs, QH, D]
    float* __restrict__ partial_ml,       // [splits, seqs, QH, 2]
    __hip_bfloat16* __restrict__ out,     // [seqs, QH, D] (splits==1 path)
    const __hip_bfloat16* __restrict__ q, // [seqs, QH, D]
    const __hip_bfloat16* __restrict__ key_cache,  // [pages, KVH, 16, D]
    const __hip_bfloat16* __restrict__ val_cache,
    const int* __restrict__ block_tables, // [seqs, max_pages]
    const int* __restrict__ context_lens, // [seqs]
    const float scale, const int num_kv_heads, const int max_pages,
    const int num_splits, const int num_seqs, const int q_stride) {
  static_assert(WS == 1 || ((WS == 2 || WS == 4) && !DIET), "WS is 1, 2, 4");
  const int kvh = blockIdx.x;
  const int wave = threadIdx.x >> 6;
  const int seq = WS == 1 ? blockIdx.y * 2 + wave : blockIdx.y;
  const int split = WS == 1 ? blockIdx.z : blockIdx.z * WS + wave;
  const int lane = threadIdx.x & 63;
  const int gl = lane & 15;
  const int gslice = lane >> 4;

  // per-wave LDS (no cross-wave sharing, no barriers).  K and V SHARE one
  // buffer: the pair's K panel serves the S MFMAs, then the V image
  // overwrites it for PV (same-wave DS ops retire in order, so the
  // write-after-read needs no fence) — halving LDS doubles resident
  // waves.  V is fully rewritten every pair (tail pages clamp to real
  // pages and are masked through P=0), so no zero-init is needed.
  constexpr int NW = WS == 1 ? 2 : WS;              // waves per workgroup
  __shared__ __hip_bfloat16 kv_all[NW][32 * DM_KP];  // K panel / V tr image
  __shared__ __hip_bfloat16 p_lds_all[NW][16 * DM_PP];
  __hip_bfloat16* k_lds = kv_all[wave];
  __hip_bfloat16* v_img = kv_all[wave];
  __hip_bfloat16* p_lds = p_lds_all[wave];
  // WS > 1: seq is uniform in the workgroup and every wave reaches the
  // epilogue's barrier
  if constexpr (WS == 1) {
    if (seq >= num_seqs) return;
  }
  const SplitRange sr = split_range(context_lens[seq], split, num_splits);

  // DIET: fragments reload per pair (L1)
  const __hip_bfloat16* q_seq = q + (size_t)seq * q_stride;
  bf8 qa[4];
  if constexpr (!DIET) load_q_frags<QPG>(qa, q_seq, kvh, gl, gslice);

  const int* btab = block_tables + (size_t)seq * max_pages;
  const int srow = lane >> 1, schunk = (lane & 1) * 64, myloc = srow >> 4;
  const int pg_last = max(sr.pg_end - 1, 0);
  DM_REGS(ka);

  float m[4], l[4];
  f32x4 acc_o[8];
#pragma unroll
  for (int r = 0; r < 4; ++r) { m[r] = NEG_INF; l[r] = 0.f; }
#pragma unroll
  for (int dt = 0; dt < 8; ++dt) acc_o[dt] = {0.f, 0.f, 0.f, 0.f};

  DM_ISSUE(key_cache, ka, sr.pg_begin);

  for (int pg = sr.pg_begin; pg < sr.pg_end; pg += 2) {
    // DIET: reload q fragments BEFORE the V issue, so the dependency wait
    // in front of the first S MFMA is vmcnt(8) — V keeps streaming
    if constexpr (DIET) load_q_frags<QPG>(qa, q_seq, kvh, gl, gslice);
    DM_WRITE(ka, DM_K_AT);
    DM_REGS(va);
    if constexpr (!DIET) DM_ISSUE(val_cache, va, pg);  // V hides under S
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

    f32x4 sA, sB;
    score_pair(sA, sB, qa, k_lds, gl, gslice);
    // DIET: q fragments are dead now — V stages into their registers and
    // its latency hides under the softmax shuffle chain below
    if constexpr (DIET) DM_ISSUE(val_cache, va, pg);

    pair_softmax(sA, sB, scale, pg, sr, m, l, acc_o, p_lds, gl, gslice);
    // V overwrites the K panel: same-wave DS ordering protects the S
    // fragment reads issued above
    DM_WRITE(va, DM_V_AT);
    DM_ISSUE(key_cache, ka, pg + 2);      // next pair's K hides under PV
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

    // O += P V via the 32-k fragment + tr-read V image
    const bf8 pa = load_p_frag(p_lds, gl, gslice);
    const unsigned vaddr = v_img_lane_addr(v_img, gl, gslice);
    if constexpr (!DIET) {
      PV_STEP16(acc_o, pa, vaddr);
    } else {
      PV_STEP8(acc_o, pa, vaddr, 0);
      PV_STEP8(acc_o, pa, vaddr, 1);
    }
  }

  // num_splits == WS (gridDim.z == 1, the only way the launcher starts a
  // WS > 1 kernel): merge in LDS.  Any other multiple of WS would write
  // partials like WS = 1; see the note on that branch at merge_in_workgroup.
  if (WS == 1 || num_splits != WS)
    store_pair_output<QPG>(partial_o, partial_ml, out, acc_o, m, l, seq,
                           num_seqs, split, num_splits, kvh, num_kv_heads, gl,
                           gslice);
  else
    merge_in_workgroup<QPG, WS>(out, &kv_all[0][0], acc_o, m, l, wave, seq,
                                kvh, num_kv_heads, gl, gslice);
}

// ---------------------------------------------------------------------------
// Producer/consumer MFMA decode (variant 6, ROUND2 §1c): TWO waves per
// sequence — wave 1 (producer) owns all global->LDS staging, wave 0
// (consumer) owns all math (S, softmax, PV) and never issues a global
// load, so the math pipeline never parks on vmcnt.  Unlike a double
// buffer, K and V keep ONE LDS panel each with a fine-grained flag
// interlock (monotonic pair counters in LDS):
//   producer pair i: wait cons_s >= i-1  -> write K_i, flag prod_k = i,
//                    issue K_{i+1};
//                    wait cons_pv >= i-1 -> write V_i, flag prod_v = i,
//                    issue V_{i+1}
//   consumer pair i: wait prod_k >= i -> S + softmax, flag cons_s = i;
//                    wait prod_v >= i -> PV, flag cons_pv = i
// LDS stays ~17 KB/WG (like variant 4's shared panel) and the producer
// runs a full pair ahead.  Cross-wave LDS ordering: panel ds_writes are
// drained (lgkmcnt(0)) before each flag write.
template <int QPG>
__global__ __launch_bounds__(128, 4) void decode_attn_pc_kernel(
    float* __restrict__ partial_o,        // [splits, seqs, QH, D]
    float* __restrict__ partial_ml,       // [splits, seqs, QH, 2]
    __hip_bfloat16* __restrict__ out,     // [seqs, QH, D] (splits==1 path)
    const __hip_bfloat16* __restrict__ q, // [seqs, QH, D]
    const __hip_bfloat16* __restrict__ key_cache,  // [pages, KVH, 16, D]
    const __hip_bfloat16* __restrict__ val_cache,
    const int* __restrict__ block_tables, // [seqs, max_pages]
    const int* __restrict__ context_lens, // [seqs]
    const float scale, const int num_kv_heads, const int max_pages,
    const int num_splits, const int num_seqs, const int q_stride) {
  const int kvh = blockIdx.x;
  const int seq = blockIdx.y;
  const int split = blockIdx.z;
  const int wave = threadIdx.x >> 6;     // 0 = consumer, 1 = producer
  const int lane = threadIdx.x & 63;
  const int gl = lane & 15;
  const int gslice = lane >> 4;

  __shared__ __hip_bfloat16 k_lds[32 * DM_KP];
  __shared__ __hip_bfloat16 v_img[32 * 128];
  __shared__ __hip_bfloat16 p_lds[16 * DM_PP];
  __shared__ int flags[4];   // prod_k, prod_v, cons_s, cons_pv (pair idx)
  if (threadIdx.x == 0) {
    flags[0] = -1; flags[1] = -1; flags[2] = -1; flags[3] = -1;
  }
  __syncthreads();
  volatile int* f_prod_k = &flags[0];
  volatile int* f_prod_v = &flags[1];
  volatile int* f_cons_s = &flags[2];
  volatile int* f_cons_pv = &flags[3];

  const SplitRange sr = split_range(context_lens[seq], split, num_splits);
  const int npairs = max(0, (sr.pg_end - sr.pg_begin + 1) >> 1);

#define PC_SPIN(fl, want)                                                    \
  while (*(fl) < (want)) __builtin_amdgcn_s_sleep(2)

  if (wave == 1) {
    // ---- producer -------------------------------------------------------
    const int* btab = block_tables + (size_t)seq * max_pages;
    const int srow = lane >> 1, schunk = (lane & 1) * 64, myloc = srow >> 4;
    const int pg_last = max(sr.pg_end - 1, 0);
    DM_REGS(ka);
    DM_REGS(va);
    if (npairs > 0) {
      DM_ISSUE(key_cache, ka, sr.pg_begin);
      DM_ISSUE(val_cache, va, sr.pg_begin);
    }
    for (int i = 0; i < npairs; ++i) {
      const int pg_next = sr.pg_begin + 2 * (i + 1);
      PC_SPIN(f_cons_s, i - 1);          // K panel free
      DM_WRITE(ka, DM_K_AT);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (lane == 0) *f_prod_k = i;
      if (i + 1 < npairs) DM_ISSUE(key_cache, ka, pg_next);
      PC_SPIN(f_cons_pv, i - 1);         // V image free
      DM_WRITE(va, DM_V_AT);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      if (lane == 0) *f_prod_v = i;
      if (i + 1 < npairs) DM_ISSUE(val_cache, va, pg_next);
    }
    return;
  }

  // ---- consumer ---------------------------------------------------------
  bf8 qa[4];
  load_q_frags<QPG>(qa, q + (size_t)seq * q_stride, kvh, gl, gslice);
  float m[4], l[4];
  f32x4 acc_o[8];
#pragma unroll
  for (int r = 0; r < 4; ++r) { m[r] = NEG_INF; l[r] = 0.f; }
#pragma unroll
  for (int dt = 0; dt < 8; ++dt) acc_o[dt] = {0.f, 0.f, 0.f, 0.f};

  for (int i = 0; i < npairs; ++i) {
    PC_SPIN(f_prod_k, i);
    f32x4 sA, sB;
    score_pair(sA, sB, qa, k_lds, gl, gslice);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // frag reads done
    if (lane == 0) *f_cons_s = i;        // K panel may be overwritten

    pair_softmax(sA, sB, scale, sr.pg_begin + 2 * i, sr, m, l, acc_o, p_lds,
                 gl, gslice);

    PC_SPIN(f_prod_v, i);
    const bf8 pa = load_p_frag(p_lds, gl, gslice);
    const unsigned vaddr = v_img_lane_addr(v_img, gl, gslice);
    PV_STEP8(acc_o, pa, vaddr, 0);
    PV_STEP8(acc_o, pa, vaddr, 1);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    if (lane == 0) *f_cons_pv = i;       // V image may be overwritten
  }
#undef PC_SPIN

  store_pair_output<QPG>(partial_o, partial_ml, out, acc_o, m, l, seq,
                         num_seqs, split, num_splits, kvh, num_kv_heads, gl,
                         gslice);
}

// ---------------------------------------------------------------------------
// FP8 (OCP e4m3fn) cache decode: variant 4 with a dequantising stage.  A
// page slice [16 tokens][128 d] is 2 KB of bytes, so the lane's share of a
// page pair is 64 B = 4 x 16 B pieces (named scalars Q0..Q3, as above).  The
// bytes become bf16 on their way into the K panel / V image; the conversion
// is exact, since e4m3's four significant bits and its exponent range fit a
// bf16.  LDS then
// holds exactly what variant 4 would have staged from the dequantised cache
// with both exponents 0; the power-of-two scales are applied where they are
// exact and free: 2^ek folded into the score scale, 2^ev into the epilogue.
// Everything after the stage (S MFMAs, softmax, PV, epilogue) is variant 4's
// code, in variant 4's order.

DEV_INLINE uint2 fp8x4_to_bf16x4(unsigned w) {
  // v_cvt_scalef32_pk_bf16_fp8 with scale 1: two e4m3 bytes -> two packed
  // bf16 in ONE instruction (half the VALU work of v_cvt_pk_f32_fp8 plus a
  // v_perm of the high halves, which measured slower: docs/STATUS.md)
  typedef __attribute__((ext_vector_type(2))) __bf16 bf2;
  union { bf2 v; unsigned u; } lo, hi;
  lo.v = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, false);
  hi.v = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, 1.0f, true);
  uint2 r;
  r.x = lo.u;
  r.y = hi.u;
  return r;
}

// 16 e4m3 bytes -> 16 bf16 as two 16-byte pieces (elements 0-7, 8-15)
DEV_INLINE void fp8x16_to_bf16(const uint4& b, uint4& lo, uint4& hi) {
  const uint2 a0 = fp8x4_to_bf16x4(b.x), a1 = fp8x4_to_bf16x4(b.y);
  const uint2 a2 = fp8x4_to_bf16x4(b.z), a3 = fp8x4_to_bf16x4(b.w);
  lo = make_uint4(a0.x, a0.y, a1.x, a1.y);
  hi = make_uint4(a2.x, a2.y, a3.x, a3.y);
}

#define DQ_REGS(R) uint4 R##0, R##1, R##2, R##3
#define DQ_ISSUE(cache, R, pg)                                              \
  do {                                                                      \
    const int p_ = btab[min((pg) + myloc, pg_last)];                        \
    const uint8_t* src_ = (cache) + schunk +                                \
        (((size_t)p_ * num_kv_heads + kvh) * 16 + (srow & 15)) * HEAD_DIM;  \
    R##0 = *reinterpret_cast<const uint4*>(src_);                           \
    R##1 = *reinterpret_cast<const uint4*>(src_ + 16);                      \
    R##2 = *reinterpret_cast<const uint4*>(src_ + 32);                      \
    R##3 = *reinterpret_cast<const uint4*>(src_ + 48);                      \
  } while (0)
#define DQ_WRITE1(r, AT, c)                                                 \
  do {                                                                      \
    uint4 lo_, hi_;                                                         \
    fp8x16_to_bf16(r, lo_, hi_);                                            \
    *reinterpret_cast<uint4*>(AT(c)) = lo_;                                 \
    *reinterpret_cast<uint4*>(AT((c) + 8)) = hi_;                           \
  } while (0)
#define DQ_WRITE(R, AT)                                                     \
  do {                                                                      \
    DQ_WRITE1(R##0, AT, 0);                                                 \
    DQ_WRITE1(R##1, AT, 16);                                                \
    DQ_WRITE1(R##2, AT, 32);                                                \
    DQ_WRITE1(R##3, AT, 48);                                                \
  } while (0)

template <int QPG, int WS = 1>
__global__ __launch_bounds__(WS == 1 ? 128 : 64 * WS, 3)
void decode_attn_mfma_fp8_kernel(
    float* __restrict__ partial_o,        // [splits, seqs, QH, D]
    float* __restrict__ partial_ml,       // [splits, seqs, QH, 2]
    __hip_bfloat16* __restrict__ out,     // [seqs, QH, D] (splits==1 path)
    const __hip_bfloat16* __restrict__ q, // [seqs, QH, D]
    const uint8_t* __restrict__ key_cache,   // [pages, KVH, 16, D] e4m3
    const uint8_t* __restrict__ val_cache,
    const int* __restrict__ block_tables, // [seqs, max_pages]
    const int* __restrict__ context_lens, // [seqs]
    const float scale,                    // softmax scale * 2^ek
    const float v_scale,                  // 2^ev
    const int num_kv_heads, const int max_pages,
    const int num_splits, const int num_seqs, const int q_stride) {
  static_assert(WS == 1 || ((WS == 2 || WS == 4)), "WS is 1, 2, 4");
  const int kvh = blockIdx.x;
  const int wave = threadIdx.x >> 6;
  const int seq = WS == 1 ? blockIdx.y * 2 + wave : blockIdx.y;
  const int split = WS == 1 ? blockIdx.z : blockIdx.z * WS + wave;
  const int lane = threadIdx.x & 63;
  const int gl = lane & 15;
  const int gslice = lane >> 4;

  // per-wave LDS, K panel and V image sharing one buffer (see variant 4)
  constexpr int NW = WS == 1 ? 2 : WS;
  __shared__ __hip_bfloat16 kv_all[NW][32 * DM_KP];
  __shared__ __hip_bfloat16 p_lds_all[NW][16 * DM_PP];
  __hip_bfloat16* k_lds = kv_all[wave];
  __hip_bfloat16* v_img = kv_all[wave];
  __hip_bfloat16* p_lds = p_lds_all[wave];
  if constexpr (WS == 1) {
    if (seq >= num_seqs) return;
  }
  const SplitRange sr = split_range(context_lens[seq], split, num_splits);

  bf8 qa[4];
  load_q_frags<QPG>(qa, q + (size_t)seq * q_stride, kvh, gl, gslice);

  const int* btab = block_tables + (size_t)seq * max_pages;
  // the lane's key row of the pair and its 64-element (= 64-byte) half row
  const int srow = lane >> 1, schunk = (lane & 1) * 64, myloc = srow >> 4;
  const int pg_last = max(sr.pg_end - 1, 0);
  DQ_REGS(ka);

  float m[4], l[4];
  f32x4 acc_o[8];
#pragma unroll
  for (int r = 0; r < 4; ++r) { m[r] = NEG_INF; l[r] = 0.f; }
#pragma unroll
  for (int dt = 0; dt < 8; ++dt) acc_o[dt] = {0.f, 0.f, 0.f, 0.f};

  DQ_ISSUE(key_cache, ka, sr.pg_begin);

  for (int pg = sr.pg_begin; pg < sr.pg_end; pg += 2) {
    DQ_WRITE(ka, DM_K_AT);
    DQ_REGS(va);
    DQ_ISSUE(val_cache, va, pg);          // V hides under S
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

    f32x4 sA, sB;
    score_pair(sA, sB, qa, k_lds, gl, gslice);
    pair_softmax(sA, sB, scale, pg, sr, m, l, acc_o, p_lds, gl, gslice);
    // V overwrites the K panel: same-wave DS ordering protects the S
    // fragment reads issued above
    DQ_WRITE(va, DM_V_AT);
    DQ_ISSUE(key_cache, ka, pg + 2);      // next pair's K hides under PV
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");

    const bf8 pa = load_p_frag(p_lds, gl, gslice);
    const unsigned vaddr = v_img_lane_addr(v_img, gl, gslice);
    PV_STEP16(acc_o, pa, vaddr);
  }

  // 2^ev: exact, and the split combine is linear in O
#pragma unroll
  for (int dt = 0; dt < 8; ++dt)
#pragma unroll
    for (int r = 0; r < 4; ++r) acc_o[dt][r] *= v_scale;

  // num_splits == WS (gridDim.z == 1, the only way the launcher starts a
  // WS > 1 kernel): merge in LDS.  Any other multiple of WS would write
  // partials like WS = 1; see the note on that branch at merge_in_workgroup.
  if (WS == 1 || num_splits != WS)
    store_pair_output<QPG>(partial_o, partial_ml, out, acc_o, m, l, seq,
                           num_seqs, split, num_splits, kvh, num_kv_heads, gl,
                           gslice);
  else
    merge_in_workgroup<QPG, WS>(out, &kv_all[0][0], acc_o, m, l, wave, seq,
                                kvh, num_kv_heads, gl, gslice);
}

#undef DQ_REGS
#undef DQ_ISSUE
#undef DQ_WRITE1
#undef DQ_WRITE
#undef DM_REGS
#undef DM_ISSUE
#undef DM_K_AT
#undef DM_V_AT
#undef DM_WRITE

// Merge split partials: one block per (seq, q_head).
__global__ void decode_combine_kernel(
    __hip_bfloat16* __restrict__ out,       // [seqs, QH, D]
    const float* __restrict__ partial_o,    // [splits, seqs, QH, D]
    const float* __restrict__ partial_ml,   // [splits, seqs, QH, 2]
    const int num_splits, const int num_q_heads) {
  const int seq = blockIdx.x, qh = blockIdx.y, d = threadIdx.x;
  const int seqs = gridDim.x;
  auto row = [&](int s) { return ((size_t)s * seqs + seq) * num_q_heads + qh; };
  out[((size_t)seq * num_q_heads + qh) * HEAD_DIM + d] = merge_splits(
      num_splits, [&](int s) { return partial_ml[row(s) * 2]; },
      [&](int s) { return partial_ml[row(s) * 2 + 1]; },
      [&](int s) { return partial_o[row(s) * HEAD_DIM + d]; });
}

// Every decode kernel takes 8 pointers, the scale and 5 ints; only the
// meaning of the middle ints differs (see launch_decode_attention).
typedef void (*DecodeKernel)(float*, float*, __hip_bfloat16*,
                             const __hip_bfloat16*, const __hip_bfloat16*,
                             const __hip_bfloat16*, const int*, const int*,
                             float, int, int, int, int, int);

template <int QPG>
DecodeKernel decode_kernel(int variant) {
  switch (variant) {
    case 0: return decode_attn_kernel<QPG, 0>;
    case 1: return decode_attn_kernel<QPG, 1>;
    case 2: return decode_attn_kernel<QPG, 2>;
    case 3: return decode_attn_kernel<QPG, 3>;
    case 4: return decode_attn_mfma_kernel<QPG, 0>;
    case 5: return decode_attn_mfma_kernel<QPG, 1>;
    case 6: return decode_attn_pc_kernel<QPG>;
    default: return nullptr;
  }
}

// Variant 4 with the splits as the waves of one workgroup (WS = 2, 4)
template <int QPG>
DecodeKernel decode_wg_kernel(int ws) {
  return ws == 2   ? decode_attn_mfma_kernel<QPG, 0, 2>
         : ws == 4 ? decode_attn_mfma_kernel<QPG, 0, 4>
                   : nullptr;
}

typedef void (*Fp8Kernel)(float*, float*, __hip_bfloat16*,
                          const __hip_bfloat16*, const uint8_t*,
                          const uint8_t*, const int*, const int*, float,
                          float, int, int, int, int, int);

template <int QPG>
Fp8Kernel decode_fp8_kernel(int ws) {
  return ws == 1   ? decode_attn_mfma_fp8_kernel<QPG, 1>
         : ws == 2 ? decode_attn_mfma_fp8_kernel<QPG, 2>
         : ws == 4 ? decode_attn_mfma_fp8_kernel<QPG, 4>
                   : nullptr;
}

}  // namespace

extern "C" {

// in_wg: the splits are merged inside the workgroup (variant 4, 16-token
// pages, num_splits 2 or 4; validated host-side) and the partials are unused.
void launch_decode_attention(void* out, void* partial_o, void* partial_ml,
                             const void* q, const void* key_cache,
                             const void* val_cache, const void* block_tables,
                             const void* context_lens, float scale,
                             int num_seqs, int num_q_heads, int num_kv_heads,
                             int page_size, int max_pages, int num_splits,
                             int variant, int q_stride, int in_wg,
                             hipStream_t stream) {
  const int qpg = num_q_heads / num_kv_heads;
  if (in_wg) {
    // ws == num_splits and gridDim.z == 1 always: the kernels' partial-
    // writing branch (num_splits != WS) is never started, so the partial
    // pointers may be null; any other split count has no kernel here
    const int ws = num_splits;
    if (ws != 2 && ws != 4) return;   // a WS kernel only ever runs WS splits
    const DecodeKernel wg = qpg == 1   ? decode_wg_kernel<1>(ws)
                            : qpg == 2 ? decode_wg_kernel<2>(ws)
                            : qpg == 4 ? decode_wg_kernel<4>(ws)
                            : qpg == 8 ? decode_wg_kernel<8>(ws)
                                       : nullptr;
    if (wg == nullptr) return;     // validated host-side
    hipLaunchKernelGGL(wg, dim3(num_kv_heads, num_seqs, 1), dim3(64 * ws), 0,
                       stream, (float*)nullptr, (float*)nullptr,
                       (__hip_bfloat16*)out, (const __hip_bfloat16*)q,
                       (const __hip_bfloat16*)key_cache,
                       (const __hip_bfloat16*)val_cache,
                       (const int*)block_tables, (const int*)context_lens,
                       scale, num_kv_heads, max_pages, num_splits, num_seqs,
                       q_stride);
    return;
  }
  // the MFMA kernels need 16-token pages; otherwise, and for out-of-range
  // variants, fall back to the dot2 kernel (variant 1)
  const bool mfma = variant >= 4 && variant <= 6 && page_size == 16;
  const int v = (mfma || (variant >= 0 && variant <= 3)) ? variant : 1;
  const DecodeKernel kernel = qpg == 1   ? decode_kernel<1>(v)
                              : qpg == 2 ? decode_kernel<2>(v)
                              : qpg == 4 ? decode_kernel<4>(v)
                              : qpg == 8 ? decode_kernel<8>(v)
                                         : nullptr;
  if (kernel == nullptr) return;   // validated host-side
  // variants 4/5 pack two sequences (one per wave) into a workgroup
  const int seq_blocks = (v == 4 || v == 5) ? (num_seqs + 1) / 2 : num_seqs;
  const dim3 grid(num_kv_heads, seq_blocks, num_splits);
  const dim3 block(mfma ? 128 : 256);
  // int tail: dot2 (page_size, max_pages, num_splits),
  //           MFMA (max_pages, num_splits, num_seqs)
  hipLaunchKernelGGL(kernel, grid, block, 0, stream, (float*)partial_o,
                     (float*)partial_ml, (__hip_bfloat16*)out,
                     (const __hip_bfloat16*)q,
                     (const __hip_bfloat16*)key_cache,
                     (const __hip_bfloat16*)val_cache,
                     (const int*)block_tables, (const int*)context_lens,
                     scale, num_kv_heads, mfma ? max_pages : page_size,
                     mfma ? num_splits : max_pages,
                     mfma ? num_seqs : num_splits, q_stride);
  if (num_splits > 1) {
    dim3 cgrid(num_seqs, num_q_heads), cblock(HEAD_DIM);
    hipLaunchKernelGGL(decode_combine_kernel, cgrid, cblock, 0, stream,
                       (__hip_bfloat16*)out, (const float*)partial_o,
                       (const float*)partial_ml, num_splits, num_q_heads);
  }
}

// e4m3 caches with 16-token pages (validated host-side).  k_scale is the
// softmax scale times 2^ek, v_scale is 2^ev.
void launch_decode_attention_fp8(void* out, void* partial_o, void* partial_ml,
                                 const void* q, const void* key_cache,
                                 const void* val_cache,
                                 const void* block_tables,
                                 const void* context_lens, float k_scale,
                                 float v_scale, int num_seqs, int num_q_heads,
                                 int num_kv_heads, int max_pages,
                                 int num_splits, int q_stride, int in_wg,
                                 hipStream_t stream) {
  const int qpg = num_q_heads / num_kv_heads;
  const int ws = in_wg ? num_splits : 1;
  // a WS kernel only ever runs WS splits (its partial pointers are null)
  if (in_wg && ws != 2 && ws != 4) return;
  const Fp8Kernel kernel = qpg == 1   ? decode_fp8_kernel<1>(ws)
                           : qpg == 2 ? decode_fp8_kernel<2>(ws)
                           : qpg == 4 ? decode_fp8_kernel<4>(ws)
                           : qpg == 8 ? decode_fp8_kernel<8>(ws)
                                      : nullptr;
  if (kernel == nullptr) return;   // validated host-side
  const dim3 grid(num_kv_heads, ws == 1 ? (num_seqs + 1) / 2 : num_seqs,
                  ws == 1 ? num_splits : 1);
  hipLaunchKernelGGL(kernel, grid, dim3(ws == 1 ? 128 : 64 * ws), 0, stream,
                     (float*)partial_o,
                     (float*)partial_ml, (__hip_bfloat16*)out,
                     (const __hip_bfloat16*)q, (const uint8_t*)key_cache,
                     (const uint8_t*)val_cache, (const int*)block_tables,
                     (const int*)context_lens, k_scale, v_scale, num_kv_heads,
                     max_pages, num_splits, num_seqs, q_stride);
  if (ws == 1 && num_splits > 1) {
    dim3 cgrid(num_seqs, num_q_heads), cblock(HEAD_DIM);
    hipLaunchKernelGGL(decode_combine_kernel, cgrid, cblock, 0, stream,
                       (__hip_bfloat16*)out, (const float*)partial_o,
                       (const float*)partial_ml, num_splits, num_q_heads);
  }
}

}  // extern "C"
