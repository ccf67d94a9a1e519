// MFMA attention building blocks shared by attn_decode.hip and
// attn_prefill.hip (gfx950, v_mfma_f32_16x16x32_bf16): the fragment type,
// the ds_read_b64_tr_b16 V image layout and the P.V step that reads it.
#pragma once

#include "common.h"

namespace {

constexpr int HEAD_DIM = 128;
constexpr float NEG_INF = -1e30f;

// MFMA A/B fragment: 8 bf16 per lane
typedef bf16x8 bf8;

DEV_INLINE bf8 load_bf8(const __hip_bfloat16* p) {
  union { uint4 u; bf8 v; } cvt;
  cvt.u = *reinterpret_cast<const uint4*>(p);
  return cvt.v;
}

// V image element offset for the ds_read_b64_tr_b16 PV path.  Per 32-key
// step (ks) and 16-dim column tile (dt), a 16-lane group's [4 key][16 dim]
// block lives at elems {q*64 + j*16 + d16} with the tr-read redistributing
// it so lane l ends with keys q*8+half*4+j at its dim column (l&15) —
// exactly the MFMA B-fragment (guide §2 tr-read layout; conflict-free
// subtiling).  Writes land as contiguous 8-element (16 B) runs per
// (key, 8-dim chunk), so staging stays fully vectorized.  Decode's 32-key
// page-pair image is the ks == 0 step.
DEV_INLINE int v_img_off(int key, int dim) {
  const int ks = key >> 5, kk = key & 31, q = kk >> 3, jj = kk & 7;
  return ks * 4096 + (dim >> 4) * 512 + (jj >> 2) * 256 + q * 64 +
         (jj & 3) * 16 + (dim & 15);
}

// LDS byte address a lane hands to the tr-reads of one 32-key image step
DEV_INLINE unsigned v_img_lane_addr(const __hip_bfloat16* step, int gl,
                                    int gslice) {
  return (unsigned)(unsigned long long)(&step[gslice * 64 + gl * 4]);
}

// The P.V steps are macros, not functions: in the 8-wave prefill kernel (the
// default prefill path) handing the accumulator array to an inlined function
// made the compiler split and re-vectorise it differently and rescheduled the
// whole k-tile loop (+13% instructions).
#define PV_MFMAS_(acc_o, pa, first, n)                                      \
  _Pragma("unroll") for (int dt_ = 0; dt_ < (n); ++dt_) {                   \
    union { struct { unsigned long long lo, hi; } u; bf8 v; } vf_;          \
    vf_.u.lo = vlo_[dt_];                                                   \
    vf_.u.hi = vhi_[dt_];                                                   \
    acc_o[(first) + dt_] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(         \
        pa, vf_.v, acc_o[(first) + dt_], 0, 0, 0);                          \
  }

// f32x4 acc_o[8] += P V over one 32-key image step: all 16 tr-reads in one
// batch, then the 8 dim-tile MFMAs (pa: P A-fragment, vaddr: the lane's
// v_img_lane_addr).  The sched_barrier keeps the MFMAs below the reads.
#define PV_STEP16(acc_o, pa, vaddr)                                         \
  do {                                                                      \
    unsigned long long vlo_[8], vhi_[8];                                    \
    asm volatile(                                                           \
        "ds_read_b64_tr_b16 %0, %16\n\t"                                    \
        "ds_read_b64_tr_b16 %1, %16 offset:512\n\t"                         \
        "ds_read_b64_tr_b16 %2, %16 offset:1024\n\t"                        \
        "ds_read_b64_tr_b16 %3, %16 offset:1536\n\t"                        \
        "ds_read_b64_tr_b16 %4, %16 offset:2048\n\t"                        \
        "ds_read_b64_tr_b16 %5, %16 offset:2560\n\t"                        \
        "ds_read_b64_tr_b16 %6, %16 offset:3072\n\t"                        \
        "ds_read_b64_tr_b16 %7, %16 offset:3584\n\t"                        \
        "ds_read_b64_tr_b16 %8, %16 offset:4096\n\t"                        \
        "ds_read_b64_tr_b16 %9, %16 offset:4608\n\t"                        \
        "ds_read_b64_tr_b16 %10, %16 offset:5120\n\t"                       \
        "ds_read_b64_tr_b16 %11, %16 offset:5632\n\t"                       \
        "ds_read_b64_tr_b16 %12, %16 offset:6144\n\t"                       \
        "ds_read_b64_tr_b16 %13, %16 offset:6656\n\t"                       \
        "ds_read_b64_tr_b16 %14, %16 offset:7168\n\t"                       \
        "ds_read_b64_tr_b16 %15, %16 offset:7680\n\t"                       \
        "s_waitcnt lgkmcnt(0)"                                              \
        : "=&v"(vlo_[0]), "=&v"(vhi_[0]), "=&v"(vlo_[1]), "=&v"(vhi_[1]),   \
          "=&v"(vlo_[2]), "=&v"(vhi_[2]), "=&v"(vlo_[3]), "=&v"(vhi_[3]),   \
          "=&v"(vlo_[4]), "=&v"(vhi_[4]), "=&v"(vlo_[5]), "=&v"(vhi_[5]),   \
          "=&v"(vlo_[6]), "=&v"(vhi_[6]), "=&v"(vlo_[7]), "=&v"(vhi_[7])    \
        : "v"(vaddr)                                                        \
        : "memory");                                                        \
    __builtin_amdgcn_sched_barrier(0);                                      \
    PV_MFMAS_(acc_o, pa, 0, 8)                                              \
  } while (0)

// The same step for one half of the dim tiles (HALF 0: tiles 0-3, HALF 1:
// 4-7), so only 16 tr-read VGPRs are live at a time.
#define PV_STEP8(acc_o, pa, vaddr, HALF)                                    \
  do {                                                                      \
    unsigned long long vlo_[4], vhi_[4];                                    \
    asm volatile(                                                           \
        "ds_read_b64_tr_b16 %0, %8 offset:%9\n\t"                           \
        "ds_read_b64_tr_b16 %1, %8 offset:%10\n\t"                          \
        "ds_read_b64_tr_b16 %2, %8 offset:%11\n\t"                          \
        "ds_read_b64_tr_b16 %3, %8 offset:%12\n\t"                          \
        "ds_read_b64_tr_b16 %4, %8 offset:%13\n\t"                          \
        "ds_read_b64_tr_b16 %5, %8 offset:%14\n\t"                          \
        "ds_read_b64_tr_b16 %6, %8 offset:%15\n\t"                          \
        "ds_read_b64_tr_b16 %7, %8 offset:%16\n\t"                          \
        "s_waitcnt lgkmcnt(0)"                                              \
        : "=&v"(vlo_[0]), "=&v"(vhi_[0]), "=&v"(vlo_[1]), "=&v"(vhi_[1]),   \
          "=&v"(vlo_[2]), "=&v"(vhi_[2]), "=&v"(vlo_[3]), "=&v"(vhi_[3])    \
        : "v"(vaddr), "i"((HALF) * 4096), "i"((HALF) * 4096 + 512),         \
          "i"((HALF) * 4096 + 1024), "i"((HALF) * 4096 + 1536),             \
          "i"((HALF) * 4096 + 2048), "i"((HALF) * 4096 + 2560),             \
          "i"((HALF) * 4096 + 3072), "i"((HALF) * 4096 + 3584)              \
        : "memory");                                                        \
    __builtin_amdgcn_sched_barrier(0);                                      \
    PV_MFMAS_(acc_o, pa, (HALF) * 4, 4)                                     \
  } while (0)

}  // namespace

