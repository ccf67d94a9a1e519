// Fused seeded sampler (gfx950): temperature, top-k, min-p, top-p and a
// Gumbel-max draw over Philox4x32-10 noise, one 1024-thread workgroup per
// row of fp32 logits [n, V].  The semantics are specified in
// docs/FEATURES.md ("Seeded sampling"); ops/reference.py::sample is the CPU
// twin and tests/sampling_cases.py the fp64 oracle.
//
// A 128 256-entry row is 512 KB and does not fit LDS, so the row is re-read
// from L2/MALL once per pass and only 256-bin histograms live in LDS:
//   pass A      row max + lowest-index argmax (+ first top-k histogram)
//   top-k       8-bit radix select of the k-th largest order-preserving key
//               (integer counts), 4 levels, level 0 fused into pass A
//   min-p       one scalar threshold, no pass
//   top-p       the same select over a histogram of softmax MASS held as
//               64-bit fixed point (units of 2^-40): integer adds commute, so
//               the boundary token is the same on every run
//   draw        Philox once per 4 tokens (only for groups with a kept token),
//               block argmax of z + g packed as (score key, ~index)
// Every filter collapses into ONE lower bound on the key (`lo`), so a filter
// that is switched off costs nothing: temperature-only is pass A + draw.
//
// Nothing depends on blockIdx except the row pointer and the per-row
// parameters, and every cross-thread combine is an integer max or add: the
// result is independent of batch position, batch size and arrival order.
#include "common.h"

#include <math.h>

namespace {

constexpr int NT = 1024;              // threads per row
constexpr int NW = NT / WAVE_SIZE;    // 16 waves
// Histogram bins are replicated per lane group: the top byte of an fp32 key
// takes only a handful of values for real logits, and 64 lanes adding to one
// LDS word serialize.
constexpr int COPIES = 16;
constexpr uint32_t KEY_NEGINF = 0x007fffffu;   // fkey(-inf)

typedef unsigned long long u64;

// Order-preserving map fp32 -> u32 (a < b  <=>  fkey(a) < fkey(b)); NaN
// compares as -inf and -0 as +0, so key equality is fp32 equality.
DEV_INLINE uint32_t fkey(float f) {
  if (!(f == f)) return KEY_NEGINF;
  const uint32_t b = (f == 0.f) ? 0u : __float_as_uint(f);
  return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

DEV_INLINE float fkey_inv(uint32_t k) {
  return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

DEV_INLINE u64 shfl_xor_u64(u64 x, int off) {
  const uint32_t lo = __shfl_xor((uint32_t)x, off, 64);
  const uint32_t hi = __shfl_xor((uint32_t)(x >> 32), off, 64);
  return ((u64)hi << 32) | lo;
}

// Block max of a u64 and block sum of a u32; every thread gets both.
DEV_INLINE void block_max_sum(u64& best, uint32_t& cnt, u64* s_best,
                              uint32_t* s_cnt) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const u64 y = shfl_xor_u64(best, off);
    best = y > best ? y : best;
    cnt += __shfl_xor(cnt, off, 64);
  }
  if (lane == 0) {
    s_best[wave] = best;
    s_cnt[wave] = cnt;
  }
  __syncthreads();
  best = 0;
  cnt = 0;
#pragma unroll
  for (int w = 0; w < NW; ++w) {
    best = s_best[w] > best ? s_best[w] : best;
    cnt += s_cnt[w];
  }
  __syncthreads();     // the scratch is reused by the next reduction
}

// Tokens 4j .. 4j+3 of a row (one Philox block).  16-byte load when the row
// base is aligned and the group is whole; otherwise guarded scalar loads.
// Returns how many of the four exist; the rest read as NaN (never kept).
DEV_INLINE int load_group(const float* __restrict__ row, int j, int V,
                          bool vec, float (&v)[4]) {
  const int i0 = j * 4;
  if (vec && i0 + 4 <= V) {
    const float4 t = *reinterpret_cast<const float4*>(row + i0);
    v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    return 4;
  }
  const int nvalid = min(4, V - i0);
#pragma unroll
  for (int c = 0; c < 4; ++c)
    v[c] = c < nvalid ? row[i0 + c] : __uint_as_float(0x7fc00000u);
  return nvalid;
}

DEV_INLINE void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2,
                              uint32_t c3, uint32_t k0, uint32_t k1,
                              uint32_t (&out)[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    // one 32x32->64 multiply per product (v_mad_u64_u32) instead of a
    // quarter-rate mul_hi + mul_lo pair: the multiplies are what the draw
    // pass spends its time on
    const u64 p0 = (u64)0xD2511F53u * c0, p1 = (u64)0xCD9E8D57u * c2;
    const uint32_t hi0 = (uint32_t)(p0 >> 32), lo0 = (uint32_t)p0;
    const uint32_t hi1 = (uint32_t)(p1 >> 32), lo1 = (uint32_t)p1;
    c0 = hi1 ^ c1 ^ k0;
    c1 = lo1;
    c2 = hi0 ^ c3 ^ k1;
    c3 = lo0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// g = -log(-log u), u = ((x >> 8) + 0.5) * 2^-24.  m + 0.5 is exact in fp32
// only for m < 2^23; for the upper half 1 - u = ((2^24 - m) - 0.5) * 2^-24
// is the exact quantity, and -log1p(-(1 - u)) keeps the inner log at ~1 ulp
// where a rounded u would lose it entirely (u == 1 would give g = +inf).
DEV_INLINE float gumbel(uint32_t x) {
  const uint32_t m = x >> 8;
  float w;
  if (m < (1u << 23)) {
    w = -logf(((float)m + 0.5f) * 0x1p-24f);
  } else {
    w = -log1pf(-(((float)((1u << 24) - m) - 0.5f) * 0x1p-24f));
  }
  return -logf(w);
}

// Cheap UPPER estimate of gumbel(x) for the draw's pre-filter: hardware
// log2 (v_log_f32, ~1 ulp on normal inputs; every input here is >= 2^-25).
// Lower half of u: the same formula, error ~1e-5.  Upper half: with the
// exact v = 1 - u, -log(1 - v) >= v + v^2/2, so -log of that bounds g from
// above (by at most 0.11 at v = 0.5, tight as v -> 0).
DEV_INLINE float gumbel_upper_fast(uint32_t x) {
  const float LN2 = 0.69314718056f;
  const uint32_t m = x >> 8;
  float w;
  if (m < (1u << 23)) {
    w = -LN2 * __builtin_amdgcn_logf(((float)m + 0.5f) * 0x1p-24f);
  } else {
    const float v = ((float)((1u << 24) - m) - 0.5f) * 0x1p-24f;
    w = fmaf(0.5f * v, v, v);
  }
  return -LN2 * __builtin_amdgcn_logf(w);
}

// Softmax weight of one survivor in units of 2^-40 (<= 2^40 each, so a row
// of up to 2^23 tokens sums without overflow).
DEV_INLINE u64 mass_units(float l, float T, float zmax) {
  const float e = expf(l / T - zmax);
  return (e >= 0.f) ? (u64)(e * 0x1p40f) : 0;
}

// Wave 0 only: walk the 256 bins from the top and pick the first bin at
// which the running total reaches the target.  With frac >= 0 the target is
// that fraction of the grand total (clamped to [1, total]); otherwise it is
// `target` as given (>= 1).  Publishes the bin, the total strictly above it
// and the target used.
template <bool MASS>
DEV_INLINE void scan_select(const u64* hist, u64 target, double frac,
                            int* s_bin, u64* s_above, u64* s_target) {
  const int lane = threadIdx.x;          // 0..63
  const uint32_t* h32 = reinterpret_cast<const uint32_t*>(hist);
  u64 v[4], tot = 0;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const int b = 255 - (lane * 4 + c);
    u64 s = 0;
#pragma unroll
    for (int k = 0; k < COPIES; ++k)
      s += MASS ? hist[b * COPIES + k] : (u64)h32[b * COPIES + k];
    v[c] = s;
    tot += s;
  }
  u64 incl = tot;
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t lo = __shfl_up((uint32_t)incl, off, 64);
    const uint32_t hi = __shfl_up((uint32_t)(incl >> 32), off, 64);
    if (lane >= off) incl += ((u64)hi << 32) | lo;
  }
  const uint32_t glo = __shfl((uint32_t)incl, 63, 64);
  const uint32_t ghi = __shfl((uint32_t)(incl >> 32), 63, 64);
  const u64 grand = ((u64)ghi << 32) | glo;
  if (frac >= 0.0) {
    target = (u64)(frac * (double)grand);
    if (target > grand) target = grand;
    if (target < 1) target = 1;
  }
  u64 run = incl - tot, above = 0;
  int found = -1;
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    if (found < 0 && run + v[c] >= target) {
      found = 255 - (lane * 4 + c);
      above = run;
    }
    run += v[c];
  }
  const u64 m = __ballot(found >= 0);
  if (m == 0) {
    // only when the table is empty or short of the target: take the lowest
    // bin, i.e. keep everything that was counted
    if (lane == 63) {
      *s_bin = 0;
      *s_above = incl - v[3];
      *s_target = target;
    }
  } else if (lane == __ffsll((long long)m) - 1) {
    *s_bin = found;
    *s_above = above;
    *s_target = target;
  }
}

// 8-bit radix select, most significant digit first, over the keys of one
// row.  COUNT mode (MASS = false): the key of the target-th largest logit
// among all V (level 0's histogram was built by pass A).  MASS mode: the
// largest key t such that the softmax mass of {key >= t}, among the
// survivors {key >= lo}, reaches frac of the survivors' total.
template <bool MASS>
DEV_INLINE uint32_t radix_select(const float* __restrict__ row, int V,
                                 bool vec, uint32_t lo, u64 target,
                                 double frac, float T, float zmax, u64* hist,
                                 int* s_bin, u64* s_above, u64* s_target) {
  const int tid = threadIdx.x;
  const int ngroups = (V + 3) >> 2;
  const int copy = tid & (COPIES - 1);
  uint32_t* h32 = reinterpret_cast<uint32_t*>(hist);
  uint32_t prefix = 0;
  for (int level = 0; level < 4; ++level) {
    const int shift = 24 - 8 * level;
    if (MASS || level > 0) {
      for (int i = tid; i < 256 * COPIES; i += NT) hist[i] = 0;
      __syncthreads();
#pragma unroll 4
      for (int j = tid; j < ngroups; j += NT) {
        float v[4];
        const int nvalid = load_group(row, j, V, vec, v);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          if (c >= nvalid) continue;
          const uint32_t key = fkey(v[c]);
          if (MASS && key < lo) continue;
          if (level > 0 && ((key ^ prefix) >> (shift + 8)) != 0) continue;
          const int bin = (key >> shift) & 255;
          if (MASS) {
            const u64 w = mass_units(v[c], T, zmax);
            if (w) atomicAdd(&hist[bin * COPIES + copy], w);
          } else {
            atomicAdd(&h32[bin * COPIES + copy], 1u);
          }
        }
      }
    }
    __syncthreads();
    if (tid < 64)
      scan_select<MASS>(hist, target, level == 0 ? frac : -1.0, s_bin,
                        s_above, s_target);
    __syncthreads();
    prefix |= (uint32_t)(*s_bin) << shift;
    target = *s_target - *s_above;
    __syncthreads();
  }
  return prefix;
}

__global__ void __launch_bounds__(NT)
sample_kernel(int64_t* __restrict__ out_tok, int* __restrict__ out_kept,
              const float* __restrict__ logits,
              const float* __restrict__ temperature,
              const int* __restrict__ top_k, const float* __restrict__ top_p,
              const float* __restrict__ min_p,
              const int64_t* __restrict__ seed, const int* __restrict__ pos,
              const int V) {
  __shared__ u64 hist[256 * COPIES];      // 32 KB; counts use the first half
  __shared__ u64 s_best[NW];
  __shared__ uint32_t s_cnt[NW];
  __shared__ int s_bin;
  __shared__ u64 s_above, s_target;

  const int row_id = blockIdx.x;
  const int tid = threadIdx.x;
  const float* row = logits + (size_t)row_id * V;
  const bool vec = (reinterpret_cast<uintptr_t>(row) & 15) == 0;
  const int ngroups = (V + 3) >> 2;
  const int copy = tid & (COPIES - 1);
  uint32_t* h32 = reinterpret_cast<uint32_t*>(hist);

  const float T = temperature[row_id];
  const bool greedy = !(T > 0.f);
  const int k = top_k[row_id];
  const float p = top_p[row_id];
  const float mp = min_p[row_id];
  const bool use_topk = !greedy && k > 0 && k < V;

  // ---- pass A: max key, lowest index among its ties ---------------------
  if (use_topk) {
    for (int i = tid; i < 256 * COPIES; i += NT) hist[i] = 0;
    __syncthreads();
  }
  u64 best = 0;
  uint32_t cnt = 0;
#pragma unroll 4
  for (int j = tid; j < ngroups; j += NT) {
    float v[4];
    const int nvalid = load_group(row, j, V, vec, v);
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      if (c >= nvalid) continue;
      const uint32_t key = fkey(v[c]);
      const u64 packed = ((u64)key << 32) | (uint32_t)~(uint32_t)(j * 4 + c);
      best = packed > best ? packed : best;
      if (use_topk) atomicAdd(&h32[(key >> 24) * COPIES + copy], 1u);
    }
  }
  block_max_sum(best, cnt, s_best, s_cnt);
  const uint32_t maxkey = (uint32_t)(best >> 32);
  if (maxkey <= KEY_NEGINF) {            // nothing above -inf in this row
    if (tid == 0) {
      out_tok[row_id] = 0;
      out_kept[row_id] = 0;
    }
    return;
  }
  if (greedy) {
    if (tid == 0) {
      out_tok[row_id] = (int64_t)(~(uint32_t)best);
      out_kept[row_id] = 1;
    }
    return;
  }

  const float lmax = fkey_inv(maxkey);
  uint32_t lo = KEY_NEGINF + 1;          // -inf (and NaN) is never kept

  // ---- 1. top-k: keep key >= key of the k-th largest (ties kept) --------
  if (use_topk) {
    const uint32_t kth = radix_select<false>(row, V, vec, lo, (u64)k, -1.0,
                                             T, 0.f, hist, &s_bin, &s_above,
                                             &s_target);
    lo = kth > lo ? kth : lo;
  }
  // ---- 2. min-p: l >= lmax + T ln(min_p) --------------------------------
  if (mp > 0.f) {
    const uint32_t mk = fkey(lmax + T * logf(mp));
    lo = mk > lo ? mk : lo;
  }
  // ---- 3. top-p over the survivors of 1 and 2 ---------------------------
  if (p < 1.f) {
    const uint32_t t = radix_select<true>(row, V, vec, lo, 0, (double)p, T,
                                          lmax / T, hist, &s_bin, &s_above,
                                          &s_target);
    lo = t > lo ? t : lo;
  }

  // ---- 4. Gumbel-max draw over {key >= lo} ------------------------------
  const uint64_t sd = (uint64_t)seed[row_id];
  const uint32_t k0 = (uint32_t)sd, k1 = (uint32_t)(sd >> 32);
  const uint32_t ps = (uint32_t)pos[row_id];
  // The accurate score costs two logf and a division per token, and with
  // one workgroup per row that arithmetic, not the row read, would set the
  // kernel's time.  So each token first gets an estimate that is never more
  // than `slack` below its accurate score; a token whose estimate cannot
  // reach the best accurate score its WAVE has seen is strictly beaten and is
  // skipped.  The bound is shared across the wave once per iteration: with a
  // per-lane bound some lane of 64 sets a new record at almost every step
  // and the whole wave pays for the accurate path.  The winner is always an
  // argmax over ACCURATE scores, so the result does not depend on which
  // tokens were skipped.
  const float inv_t = 1.0f / T;
  float best_s = -INFINITY;
  best = 0;
  cnt = 0;
  for (int base = 0; base < ngroups; base += NT) {   // wave-uniform trips
    const int j = base + tid;
    float v[4];
    const int nvalid = j < ngroups ? load_group(row, j, V, vec, v) : 0;
    bool kept[4], any = false;
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      kept[c] = c < nvalid && fkey(v[c]) >= lo;
      any |= kept[c];
    }
    if (any) {
      uint32_t x[4];
      philox4x32_10((uint32_t)j, ps, 0u, 0u, k0, k1, x);
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        if (!kept[c]) continue;
        ++cnt;
        const float z_est = v[c] * inv_t;
        // estimate errors: z by 2 roundings, g by ~1e-5; slack is far above
        const float slack = 0x1p-8f + 0x1p-12f * fabsf(z_est);
        if (z_est + gumbel_upper_fast(x[c]) + slack < best_s) continue;
        const float score = v[c] / T + gumbel(x[c]);
        const u64 packed =
            ((u64)fkey(score) << 32) | (uint32_t)~(uint32_t)(j * 4 + c);
        best = packed > best ? packed : best;
        best_s = fmaxf(best_s, score);
      }
    }
    best_s = wave_max(best_s);
  }
  block_max_sum(best, cnt, s_best, s_cnt);
  if (tid == 0) {
    out_tok[row_id] = cnt ? (int64_t)(~(uint32_t)best) : 0;
    out_kept[row_id] = (int)cnt;
  }
}

}  // namespace

extern "C" {

// One workgroup per row; all per-row parameters are device arrays of n.
void launch_sample(void* out_tok, void* out_kept, const void* logits,
                   const void* temperature, const void* top_k,
                   const void* top_p, const void* min_p, const void* seed,
                   const void* pos, int n, int V, hipStream_t stream) {
  hipLaunchKernelGGL(sample_kernel, dim3(n), dim3(NT), 0, stream,
                     (int64_t*)out_tok, (int*)out_kept, (const float*)logits,
                     (const float*)temperature, (const int*)top_k,
                     (const float*)top_p, (const float*)min_p,
                     (const int64_t*)seed, (const int*)pos, V);
}

}  // extern "C"
