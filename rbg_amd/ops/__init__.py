"""rbg_amd.ops — dispatch layer over the CDNA4 HIP kernels.

On a GPU the compiled in-tree extension (_hip_ops, built by setup.py for
gfx950) is MANDATORY: a missing extension raises instead of silently running
an eager fallback, so GPU tests always exercise the native path.  On CPU
(unit tests, GPU-less CI) the fp32 torch references in ops.reference serve
as the implementation.
"""
from __future__ import annotations

import os
from typing import NamedTuple

import torch

from . import reference

_hip = None
_hip_err: Exception | None = None
try:
    from . import _hip_ops as _hip   # type: ignore[attr-defined]
except Exception as e:  # noqa: BLE001
    _hip_err = e

HAVE_HIP = _hip is not None


def _check_stale() -> None:
    """Fail loudly on a GPU box if the shipped .so predates the kernel
    sources (stale-binary guard; the stamp is written by
    __graft_entry__.build())."""
    import hashlib
    here = os.path.dirname(os.path.abspath(__file__))
    stamp = os.path.join(here, "_hip_ops.srchash")
    if not os.path.exists(stamp):
        return
    h = hashlib.sha256()
    hip_dir = os.path.join(here, "hip")
    for name in sorted(os.listdir(hip_dir)):
        if name.endswith(("_hip.hip", "_hip.h")):
            continue
        if name.endswith((".hip", ".cpp", ".h")):
            with open(os.path.join(hip_dir, name), "rb") as f:
                h.update(name.encode() + b"\0" + f.read() + b"\0")
    with open(stamp) as f:
        recorded = f.read().strip()
    if recorded and recorded != h.hexdigest():
        raise RuntimeError(
            "rbg_amd HIP extension is STALE: kernel sources changed after "
            "the last build.  Rebuild in-tree: PYTORCH_ROCM_ARCH=gfx950 "
            "python setup.py build_ext --inplace")


if HAVE_HIP and torch.cuda.is_available():
    _check_stale()


def _require_hip():
    if _hip is None:
        raise RuntimeError(
            "rbg_amd HIP extension is not built but a GPU tensor was passed. "
            "Build it in-tree: PYTORCH_ROCM_ARCH=gfx950 python setup.py "
            f"build_ext --inplace (import error: {_hip_err!r})")
    return _hip


def _on_gpu(t: torch.Tensor) -> bool:
    return t.is_cuda


SKINNY_GEMM = int(os.environ.get("RBG_SKINNY_GEMM", "1"))


FP8 = torch.float8_e4m3fn
WEIGHT_DTYPES = reference.WEIGHT_DTYPES
quantize_weight_e4m3 = reference.quantize_weight_e4m3
dequantize_weight_e4m3 = reference.dequantize_weight_e4m3
EXPERT_WEIGHT_DTYPES = reference.EXPERT_WEIGHT_DTYPES
quantize_weight_mxfp4 = reference.quantize_weight_mxfp4
dequantize_weight_mxfp4 = reference.dequantize_weight_mxfp4


def _is_w8(w: torch.Tensor, w_scale_log2) -> bool:
    """True for an e4m3 weight with its exponents (docs/FEATURES.md "FP8
    weights"); half a pair raises before anything is launched."""
    if w.dtype == FP8:
        if w_scale_log2 is None:
            raise ValueError("an e4m3 weight needs w_scale_log2, its int8 "
                             "per-row exponents")
        return True
    if w_scale_log2 is not None:
        raise ValueError("w_scale_log2 was given for a %s weight: only an "
                         "e4m3 weight has exponents" % w.dtype)
    return False


def _use_skinny_gemm_w8(x: torch.Tensor, w: torch.Tensor) -> bool:
    # every N: an e4m3 weight has no library to prefer on the wide shapes
    return bool(x.dim() == 2 and x.dtype == torch.bfloat16 and
                1 <= x.shape[0] <= 128 and w.shape[0] % 64 == 0 and
                x.shape[1] >= 256 and x.shape[1] % 256 == 0)


def dequantize_weight(w: torch.Tensor, e: torch.Tensor) -> torch.Tensor:
    """bf16 [N, K] = e4m3 * 2^e[row], exact (hip/skinny_gemm_w8.hip's
    w8_dequant_kernel on a GPU)."""
    if _on_gpu(w):
        return _require_hip().w8_dequant(w, e)
    return reference.dequantize_weight_e4m3(w, e)


def _use_skinny_gemm(x: torch.Tensor, w: torch.Tensor) -> bool:
    # measured policy (profiles/sg_micro7_b*.json): the custom kernel wins
    # on narrow-N shapes (o/down, N<=4096) at any decode batch, on mid-N
    # (qkv, 6144) only up to M=64, and never on wide-N (gate_up 28672,
    # where hipBLASLt already streams at ~6 TB/s)
    return bool(SKINNY_GEMM and _on_gpu(x) and x.dim() == 2 and
                x.dtype == torch.bfloat16 and 1 <= x.shape[0] <= 128 and
                w.shape[0] % 32 == 0 and x.shape[1] % 512 == 0 and
                (w.shape[0] <= 4608 or
                 (x.shape[0] <= 64 and w.shape[0] <= 8192)))


def _gemm_path(x: torch.Tensor, w: torch.Tensor, w_scale_log2) -> str:
    """What linear() and linear_add_rmsnorm() run x w^T on: "w8"
    (hip/skinny_gemm_w8.hip), "bf16" (hip/skinny_gemm.hip) or "library"."""
    if _is_w8(w, w_scale_log2):
        return "w8" if _on_gpu(x) and _use_skinny_gemm_w8(x, w) else "library"
    return "bf16" if _use_skinny_gemm(x, w) else "library"


def linear(x: torch.Tensor, w: torch.Tensor,
           w_scale_log2=None) -> torch.Tensor:
    """Projection GEMM with decode-shape dispatch: for M <= 128 rows the
    hand-written split-K streaming kernel (hip/skinny_gemm.hip) replaces
    hipBLASLt, which leaves 2-5x on narrow-N skinny shapes
    (profiles/gemm_ab_b128.json).  Prefill-sized M goes to the library.

    An e4m3 `w` with its int8 exponents `w_scale_log2` is the bf16 weight
    dq = e4m3 * 2^e: M <= 128 takes hip/skinny_gemm_w8.hip at every N,
    anything else is dequantised (exactly) and goes to the library."""
    path = _gemm_path(x, w, w_scale_log2)
    if path == "w8":
        return _require_hip().skinny_gemm_w8(
            x if x.is_contiguous() else x.contiguous(), w, w_scale_log2)
    if path == "bf16":
        return _require_hip().skinny_gemm(
            x if x.is_contiguous() else x.contiguous(), w)
    if w_scale_log2 is not None:
        w = dequantize_weight(w, w_scale_log2)
    return torch.nn.functional.linear(x, w)


def linear_add_rmsnorm(x: torch.Tensor, w: torch.Tensor,
                       residual: torch.Tensor, norm_weight: torch.Tensor,
                       eps: float, w_scale_log2=None) -> torch.Tensor:
    """h = linear(x, w); residual += h; return rmsnorm(residual) — bit for
    bit `h = linear(x, w); fused_add_rmsnorm(h, residual, ...)`.  Where
    linear() would take the custom GEMM, the split-K partials are folded
    inside the norm kernel instead of by a reduce launch of their own
    (hip/rmsnorm.hip, NORM_FOLD_ADD).  w_scale_log2: as in linear()."""
    path = _gemm_path(x, w, w_scale_log2)
    if path == "w8":
        return _require_hip().skinny_gemm_w8_add_rmsnorm(
            x if x.is_contiguous() else x.contiguous(), w, w_scale_log2,
            residual, norm_weight, eps)
    if path == "bf16":
        return _require_hip().skinny_gemm_add_rmsnorm(
            x if x.is_contiguous() else x.contiguous(), w, residual,
            norm_weight, eps)
    h = linear(x, w) if w_scale_log2 is None else linear(x, w, w_scale_log2)
    fused_add_rmsnorm(h, residual, norm_weight, eps)
    return h


def rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float) -> torch.Tensor:
    if _on_gpu(x):
        return _require_hip().rmsnorm(x, weight, eps)
    return reference.rmsnorm(x, weight, eps)


def fused_add_rmsnorm(x: torch.Tensor, residual: torch.Tensor,
                      weight: torch.Tensor, eps: float) -> None:
    if _on_gpu(x):
        _require_hip().fused_add_rmsnorm(x, residual, weight, eps)
        return
    reference.fused_add_rmsnorm(x, residual, weight, eps)


def silu_mul(x: torch.Tensor) -> torch.Tensor:
    if _on_gpu(x):
        return _require_hip().silu_mul(x)
    return reference.silu_mul(x)


# ---- mixture of experts (docs/FEATURES.md "Mixture of experts") -----------

MOE_MAX_EXPERTS = reference.MOE_MAX_EXPERTS
MOE_MAX_TOP_K = reference.MOE_MAX_TOP_K

_moe_tickets: dict = {}


def _moe_ticket(device) -> torch.Tensor:
    """The int32 the route kernel's workgroups count themselves off on; the
    last one puts it back to zero, so one per device serves every launch
    (launches that follow each other on a stream, as the engine's do; two
    streams routing at once would need a ticket each)."""
    t = _moe_tickets.get(device)
    if t is None:
        t = _moe_tickets[device] = torch.zeros(1, dtype=torch.int32,
                                               device=device)
    return t


def moe_route(router_logits: torch.Tensor, top_k: int,
              renormalize: bool = True):
    """Top-k routing of bf16 router logits [T, E] -> (ids int32 [T, k],
    w fp32 [T, k]): the k largest logits (ties to the lower index, NaN as
    -inf) in descending order and their fp32 softmax weights, renormalised
    over the k selected if asked.  On a GPU the same launch also groups the
    (token, slot) pairs by expert; the grouping rides on `ids` for
    moe_ffn."""
    if router_logits.dim() != 2 or router_logits.dtype != torch.bfloat16:
        raise ValueError("router_logits must be bf16 [T, E]")
    E = router_logits.shape[1]
    if not 1 <= E <= MOE_MAX_EXPERTS:
        raise ValueError("E must be in [1, %d], got %d" % (MOE_MAX_EXPERTS, E))
    if not 1 <= top_k <= min(MOE_MAX_TOP_K, E):
        raise ValueError("top_k must be in [1, min(%d, E)], got %d" % (
            MOE_MAX_TOP_K, top_k))
    if not _on_gpu(router_logits):
        return reference.moe_route(router_logits, top_k, renormalize)
    ids, w, offsets, pairs = _require_hip().moe_route(
        router_logits if router_logits.is_contiguous()
        else router_logits.contiguous(),
        _moe_ticket(router_logits.device), top_k, bool(renormalize))
    # in [0, E) by construction: moe_ffn neither groups nor checks them again,
    # unless ids was written to since (its version counter moved)
    ids._moe_group = (E, offsets, pairs)
    ids._moe_group_version = _tensor_version(ids)
    return ids, w


def _tensor_version(t: torch.Tensor):
    """t._version, or None for an inference tensor (the model's forward runs
    under torch.inference_mode, where tensors keep no version counter and an
    in-place edit cannot be told; the model makes none)."""
    try:
        return t._version
    except RuntimeError:
        return None


def moe_ffn(x: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor,
            ids: torch.Tensor, w: torch.Tensor, w1_scale_log2=None,
            w2_scale_log2=None) -> torch.Tensor:
    """y bf16 [T, H] = sum_j w[t, j] * FFN_{ids[t, j]}(x[t]) with expert
    weights w1 [E, 2I, H] (gate rows, then up rows) and w2 [E, H, I]:
    hip/moe.hip on a GPU, reference.moe_ffn on CPU tensors.  Everything is
    checked before anything is launched; ids that did not come from
    moe_route, or were written to since, are read back once for their range
    and grouped again.

    e4m3 w1 and w2 with their int8 exponents w1_scale_log2 [E, 2I] and
    w2_scale_log2 [E, H] (ops.quantize_weight_e4m3 of the weights viewed
    [E * rows, K]) are the bf16 experts dq = e4m3 * 2^e: on a GPU the e4m3
    instantiation of the grouped GEMMs, bit for bit the bf16 one on dq.

    uint8 w1 [E, 2I, H/2] and w2 [E, H, I/2] are MXFP4 (docs/FEATURES.md
    "MXFP4 experts"): two e2m1 codes per byte with int8 exponents per 32 k,
    w1_scale_log2 [E, 2I, H/32] and w2_scale_log2 [E, H, I/32]
    (ops.quantize_weight_mxfp4 of the weights viewed [E * rows, K]).  They
    are the bf16 experts dq = e2m1 * 2^e: the MXFP4 instantiation on a GPU,
    again bit for bit the bf16 one on dq."""
    if w1.dtype != w2.dtype:
        raise ValueError("w1 and w2 must have one dtype, got %s and %s" % (
            w1.dtype, w2.dtype))
    w4 = w1.dtype == torch.uint8
    if w4:
        for e in (w1_scale_log2, w2_scale_log2):
            if e is None or e.dim() != 3:
                raise ValueError("an MXFP4 weight needs its scale_log2, the "
                                 "3-D int8 exponents per 32 k")
        w8, wdt = False, torch.uint8
    else:
        w8 = _is_w8(w1, w1_scale_log2)
        _is_w8(w2, w2_scale_log2)
        wdt = FP8 if w8 else torch.bfloat16
    for t, name, dt, nd in ((x, "x", torch.bfloat16, 2),
                            (w1, "w1", wdt, 3),
                            (w2, "w2", wdt, 3),
                            (ids, "ids", torch.int32, 2),
                            (w, "w", torch.float32, 2)):
        if t.dtype != dt or t.dim() != nd:
            raise ValueError("%s must be %d-D %s, got %s %s" % (
                name, nd, dt, tuple(t.shape), t.dtype))
        if t.device != x.device:
            raise ValueError("%s is on %s but x is on %s" % (
                name, t.device, x.device))
        if not t.is_contiguous():
            raise ValueError("%s must be contiguous" % name)
    T, H = x.shape
    E, I, k = w1.shape[0], w2.shape[2], ids.shape[1]
    if w4:
        # H is x's and I the scales': a byte count cannot tell I from I + 1
        I = w2_scale_log2.shape[2] * reference.MXFP4_BLOCK
        if (tuple(w1.shape) != (E, 2 * I, H // 2) or
                tuple(w2.shape) != (E, H, I // 2)):
            raise ValueError("MXFP4 w1 must be [E, 2I, H/2] and w2 [E, H, "
                             "I/2], got %s and %s for H = %d, I = %d" % (
                                 tuple(w1.shape), tuple(w2.shape), H, I))
    elif tuple(w1.shape) != (E, 2 * I, H) or tuple(w2.shape) != (E, H, I):
        raise ValueError("w1 must be [E, 2I, H] and w2 [E, H, I], got %s and "
                         "%s for H = %d" % (tuple(w1.shape), tuple(w2.shape),
                                            H))
    if tuple(ids.shape) != (T, k) or tuple(w.shape) != (T, k):
        raise ValueError("ids and w must be [T, k], got %s and %s for T = %d"
                         % (tuple(ids.shape), tuple(w.shape), T))
    if (not 1 <= E <= MOE_MAX_EXPERTS or not 1 <= k <= min(MOE_MAX_TOP_K, E)
            or H % 256 or I % 64):
        raise ValueError("moe_ffn needs E <= %d, k <= min(%d, E), H %% 256 == "
                         "0 and I %% 64 == 0, got E = %d, k = %d, H = %d, I = "
                         "%d" % (MOE_MAX_EXPERTS, MOE_MAX_TOP_K, E, k, H, I))
    if w8 or w4:
        for e, name, shape in (
                (w1_scale_log2, "w1_scale_log2",
                 (E, 2 * I, H // 32) if w4 else (E, 2 * I)),
                (w2_scale_log2, "w2_scale_log2",
                 (E, H, I // 32) if w4 else (E, H))):
            if (e.dtype != torch.int8 or tuple(e.shape) != shape or
                    not e.is_contiguous() or e.device != x.device):
                raise ValueError("%s must be contiguous int8 %s on %s, got "
                                 "%s %s on %s" % (name, shape, x.device,
                                                  tuple(e.shape), e.dtype,
                                                  e.device))
    if T == 0:
        return torch.empty_like(x)
    group = getattr(ids, "_moe_group", None)
    if group is not None and (getattr(ids, "_moe_group_version", -1)
                              != _tensor_version(ids)):
        group = None            # ids was edited in place after moe_route
    if group is None or group[0] != E:
        lo, hi = int(ids.min()), int(ids.max())
        if lo < 0 or hi >= E:
            raise ValueError("ids must lie in [0, %d), got [%d, %d]" % (
                E, lo, hi))
        if _on_gpu(x):
            group = (E,) + tuple(_require_hip().moe_group(ids, E))
    if not _on_gpu(x):
        if w8:
            w1, w2 = (reference.dequantize_weight_e4m3(
                t.view(-1, t.shape[2]), e.view(-1)).view(t.shape)
                for t, e in ((w1, w1_scale_log2), (w2, w2_scale_log2)))
        if w4:
            w1, w2 = (reference.dequantize_weight_mxfp4(
                t.view(-1, t.shape[2]), e.view(-1, e.shape[2])).view(
                    t.shape[0], t.shape[1], -1)
                for t, e in ((w1, w1_scale_log2), (w2, w2_scale_log2)))
        return reference.moe_ffn(x, w1, w2, ids, w)
    if w8 or w4:
        return _require_hip().moe_ffn(x, w1, w2, w, group[1], group[2],
                                      w1_scale_log2, w2_scale_log2)
    return _require_hip().moe_ffn(x, w1, w2, w, group[1], group[2])


KV_CACHE_DTYPES = reference.KV_CACHE_DTYPES
KV_SCALE_LOG2_RANGE = reference.KV_SCALE_LOG2_RANGE
check_kv_scale_log2 = reference.check_kv_scale_log2


def _is_fp8_pair(key_cache, value_cache) -> bool:
    """True for an e4m3 cache pair (docs/FEATURES.md "FP8 KV cache"); a pair
    of differing dtypes raises before anything is launched."""
    if key_cache.dtype != value_cache.dtype:
        raise ValueError("key_cache is %s but value_cache is %s" % (
            key_cache.dtype, value_cache.dtype))
    return key_cache.dtype == FP8


def rope_store_kv(q, k, v, key_cache, value_cache, cos_sin, positions,
                  slot_mapping, k_scale_log2: int = 0,
                  v_scale_log2: int = 0) -> None:
    """RoPE on q, k in place, then the paged KV write.  An e4m3 cache
    receives sat_rne_e4m3fn(x * 2^-e) of the bf16 value a bf16 cache would
    have received; the exponents are ignored for a bf16 cache."""
    fp8 = _is_fp8_pair(key_cache, value_cache)
    scales = ()
    if fp8:
        check_kv_scale_log2(k_scale_log2, "kv_k_scale_log2")
        check_kv_scale_log2(v_scale_log2, "kv_v_scale_log2")
        scales = (k_scale_log2, v_scale_log2)
    args = (q, k, v, key_cache, value_cache, cos_sin, positions,
            slot_mapping) + scales
    if not _on_gpu(q):
        reference.rope_store_kv(*args)
    elif fp8:
        _require_hip().rope_store_kv_fp8(*args)
    else:
        _require_hip().rope_store_kv(*args)


def kv_gather_dequant(cache, slots, scale_log2: int = 0) -> torch.Tensor:
    """Rows of an e4m3 cache [pages, KVH, page, D] by slot, dequantised:
    bf16 [Tkv, KVH, D] = e4m3(byte) * 2^scale_log2 (exact)."""
    if cache.dtype != FP8:
        raise ValueError("kv_gather_dequant needs a float8_e4m3fn cache, "
                         "got %s" % cache.dtype)
    check_kv_scale_log2(scale_log2, "scale_log2")
    if _on_gpu(cache):
        return _require_hip().kv_gather_dequant(cache, slots, scale_log2)
    return reference.kv_gather_dequant(cache, slots, scale_log2)


def pick_decode_splits(num_seqs: int, num_kv_heads: int,
                       max_context: int, variant: int = -1) -> int:
    """Fill the chip: MI355X has 256 CUs / 8 XCDs; measured optimum is
    ~1024 workgroups for BOTH kernels (profiles/decode_breakdown r59
    sweep: V4 B128 peaks at splits=2 = 1024 WGs, B64 at splits=4 = 1024).
    The MFMA kernel packs 2 sequences per WG, so its base WG count is
    half the dot2 kernel's at equal splits."""
    if variant < 0:
        variant = DECODE_VARIANT
    if variant >= 4:
        # v4/v5 pack 2 seqs per WG; v6 runs 1 seq per (2-wave) WG
        per_wg = 2 if variant in (4, 5) else 1
        base = num_kv_heads * ((num_seqs + per_wg - 1) // per_wg)
        by_ctx = max(1, max_context // 32)      # >= one page pair per split
    else:
        base = num_seqs * num_kv_heads
        by_ctx = max(1, max_context // 256)
    if base >= 1024:
        return 1
    want = max(1, 1024 // max(base, 1))
    return int(min(want, by_ctx, 16))


DECODE_VARIANT = int(os.environ.get("RBG_DECODE_VARIANT", "4"))  # MFMA page-pair decode: 5.6 TB/s vs 4.0 dot2 (B128, within-probe)
PREFILL_SWZ = int(os.environ.get("RBG_PREFILL_SWZ", "6"))  # 8-wave + K/V double-buffer (305 TF/s vs 252 @ swz=4, within-probe)


def decode_attention(q, key_cache, value_cache, block_tables, context_lens,
                     scale: float, num_splits: int = 0,
                     variant: int = -1, k_scale_log2: int = 0,
                     v_scale_log2: int = 0, combine: int = 0) -> torch.Tensor:
    """Paged flash-decode.  combine says how the partials of num_splits > 1
    are merged on the GPU: 0 picks (inside the workgroup for the page-pair
    MFMA kernels at 2 or 4 splits, where the splits are the waves of one
    workgroup and neither partials nor a second launch exist; else by
    decode_combine_kernel), 1 forces the separate kernel, 2 the in-workgroup
    merge (raising where no kernel has it).  Both give the same bits."""
    fp8 = _is_fp8_pair(key_cache, value_cache)
    scales = ()
    if fp8:
        # one kernel reads an e4m3 cache: the page-pair MFMA one (variant 4)
        if variant not in (-1, 4):
            raise ValueError("an fp8 KV cache has no decode variant %d: only "
                             "variant 4 reads e4m3" % variant)
        check_kv_scale_log2(k_scale_log2, "kv_k_scale_log2")
        check_kv_scale_log2(v_scale_log2, "kv_v_scale_log2")
        if key_cache.shape[2] != 16 or key_cache.shape[3] != 128:
            raise ValueError("fp8 decode needs page size 16 and head_dim 128, "
                             "got %d and %d" % (key_cache.shape[2],
                                                key_cache.shape[3]))
        scales = (k_scale_log2, v_scale_log2)
    args = (q, key_cache, value_cache, block_tables, context_lens, scale)
    if not _on_gpu(q):
        return reference.decode_attention(*args, *scales)
    if num_splits <= 0:
        max_ctx = int(context_lens.max().item()) if context_lens.numel() else 1
        # a bf16 cache gets the default variant's split policy whatever
        # `variant` says
        num_splits = pick_decode_splits(q.shape[0], key_cache.shape[1],
                                        max_ctx, 4 if fp8 else -1)
    if fp8:
        return _require_hip().decode_attention_fp8(*args, num_splits, *scales,
                                                   combine)
    return _require_hip().decode_attention(
        *args, num_splits, DECODE_VARIANT if variant < 0 else variant, combine)


def prefill_attention(q, k, v, cu_seqlens, scale: float,
                      cu_seqlens_k=None) -> torch.Tensor:
    if _on_gpu(q):
        # bit 2 = 8-wave 16x16 blocks; bit 3 = 4-wave 32x32 blocks
        qtile = 128 if (PREFILL_SWZ & 12) else 64
        block_info, seq_lens = reference.prefill_block_info(
            cu_seqlens.cpu(), qtile=qtile,
            cu_seqlens_k=None if cu_seqlens_k is None else cu_seqlens_k.cpu())
        return _require_hip().prefill_attention(
            q, k, v, block_info.to(q.device), seq_lens.to(q.device), scale,
            PREFILL_SWZ)
    return reference.prefill_attention(q, k, v, cu_seqlens, scale,
                                       cu_seqlens_k)


PAGED_PREFILL_QTILE = 128      # q rows per workgroup of the paged kernel


class PagedBlockMap(NamedTuple):
    """The paged prefill kernel's block map and what it was checked against:
    it indexes rows [0, num_seqs) of a table at least table_width wide."""
    block_info: torch.Tensor
    seq_lens: torch.Tensor
    num_seqs: int
    table_width: int


def prefill_paged_block_map(cu_seqlens, cu_seqlens_k, table_width: int,
                            device):
    """(block_info, seq_lens) of ops.prefill_attention_paged on `device`,
    from HOST lists (or CPU tensors) of cumulative q and KV lengths.  Raises
    ValueError where the kernel would read outside a sequence's table row."""
    cu = reference._int_list(cu_seqlens)
    cuk = cu if cu_seqlens_k is None else reference._int_list(cu_seqlens_k)
    if len(cu) != len(cuk):
        raise ValueError("cu_seqlens has %d entries but cu_seqlens_k has %d"
                         % (len(cu), len(cuk)))
    for b in range(len(cu) - 1):
        Lq, Lk = cu[b + 1] - cu[b], cuk[b + 1] - cuk[b]
        if Lq < 0 or Lk < Lq:
            raise ValueError("sequence %d has %d q rows but %d keys"
                             % (b, Lq, Lk))
        if (Lk + 15) // 16 > table_width:
            raise ValueError("sequence %d needs %d block-table columns, the "
                             "table has %d" % (b, (Lk + 15) // 16,
                                               table_width))
    block_info, seq_lens = reference.prefill_block_info_paged(
        cu, PAGED_PREFILL_QTILE, cuk, device=device)
    return PagedBlockMap(block_info, seq_lens, len(cu) - 1, table_width)


def prefill_attention_paged(q, key_cache, value_cache, block_tables,
                            cu_seqlens, scale: float, cu_seqlens_k=None,
                            k_scale_log2: int = 0, v_scale_log2: int = 0,
                            block_map=None) -> torch.Tensor:
    """Varlen causal prefill attention that reads K and V in place from the
    paged pool (bf16 or e4m3, 16-token pages, head_dim 128) through
    block_tables [num_seqs, max_pages]: sequence b's q rows are the LAST Lq
    positions of its Lk keys (docs/FEATURES.md "Paged prefill").  An e4m3
    pool is read as e4m3 * 2^e; the exponents are ignored for bf16.

    block_map = prefill_paged_block_map(...) lets a caller that has the
    lengths on the host build (and check) the map once per step; without it
    the op reads cu_seqlens back and builds it itself.  A PagedBlockMap is
    checked against block_tables' shape here.  A bare (block_info, seq_lens)
    pair is taken on trust: the caller vouches that every sequence index in
    it is a row of block_tables and that every sequence's pages fit the
    table's width, which nothing below this function can check."""
    fp8 = _is_fp8_pair(key_cache, value_cache)
    if fp8:
        check_kv_scale_log2(k_scale_log2, "kv_k_scale_log2")
        check_kv_scale_log2(v_scale_log2, "kv_v_scale_log2")
    else:
        k_scale_log2 = v_scale_log2 = 0
    if key_cache.dim() != 4 or key_cache.shape[2] != 16 or \
            key_cache.shape[3] != 128:
        raise ValueError("paged prefill needs caches [pages, KVH, 16, 128], "
                         "got %s" % (tuple(key_cache.shape),))
    if block_tables.dim() != 2 or block_tables.dtype != torch.int32:
        raise ValueError("block_tables must be int32 [num_seqs, max_pages]")
    if block_map is None:
        cu = cu_seqlens.cpu()
        cuk = None if cu_seqlens_k is None else cu_seqlens_k.cpu()
        if cu.numel() - 1 > block_tables.shape[0]:
            raise ValueError("%d sequences but %d block-table rows" % (
                cu.numel() - 1, block_tables.shape[0]))
        block_map = prefill_paged_block_map(cu, cuk, block_tables.shape[1],
                                            q.device)
    if isinstance(block_map, PagedBlockMap) and (
            block_map.num_seqs > block_tables.shape[0] or
            block_map.table_width > block_tables.shape[1]):
        raise ValueError("block_map was built for %d sequences and a table "
                         "%d wide, block_tables is %s" % (
                             block_map.num_seqs, block_map.table_width,
                             tuple(block_tables.shape)))
    if not _on_gpu(q):
        return reference.prefill_attention_paged(
            q, key_cache, value_cache, block_tables, cu_seqlens, scale,
            cu_seqlens_k, k_scale_log2, v_scale_log2)
    block_info, seq_lens = block_map[0], block_map[1]
    return _require_hip().prefill_attention_paged(
        q, key_cache, value_cache, block_tables, block_info, seq_lens, scale,
        k_scale_log2, v_scale_log2)


build_cos_sin_table = reference.build_cos_sin_table


def sample(logits, temperature, top_k, top_p, min_p, seed, pos):
    """Seeded sampling, one row per request (docs/FEATURES.md "Seeded
    sampling").  logits fp32 [n, V]; per-row tensors of length n on the
    logits' device: fp32 temperature / top_p / min_p, int32 top_k / pos,
    int64 seed (the 64-bit seed's two's-complement bits).  Returns (tokens
    int64 [n], num_kept int32 [n]) with no host synchronisation."""
    if _on_gpu(logits):
        toks, kept = _require_hip().sample(logits, temperature, top_k, top_p,
                                           min_p, seed, pos)
        return toks, kept
    return reference.sample(logits, temperature, top_k, top_p, min_p, seed,
                            pos)

