"""Pure-PyTorch fp32 reference implementations of every HIP op.

Two jobs (SURVEY §4 test strategy): (a) the numerics oracle the GPU kernels
are compared against in tests/test_ops_gpu.py, and (b) the CPU execution
path that lets the whole engine run (tiny configs) in GPU-less CI.  These
are NOT a production fallback — on a GPU the HIP extension is mandatory and
its absence raises (ops/__init__.py).
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch


def rmsnorm(x: torch.Tensor, weight: torch.Tensor, eps: float) -> torch.Tensor:
    xf = x.float()
    inv = torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + eps)
    return (xf * inv * weight.float()).to(x.dtype)


def fused_add_rmsnorm(x: torch.Tensor, residual: torch.Tensor,
                      weight: torch.Tensor, eps: float) -> None:
    """In-place contract of the HIP kernel: residual += x; x = rmsnorm(residual)."""
    summed = (residual.float() + x.float())
    residual.copy_(summed.to(residual.dtype))
    x.copy_(rmsnorm(residual, weight, eps))


def silu_mul(x: torch.Tensor) -> torch.Tensor:
    gate, up = x.float().chunk(2, dim=-1)
    return (torch.nn.functional.silu(gate) * up).to(x.dtype)


def build_cos_sin_table(head_dim: int, max_positions: int,
                        theta: float = 500000.0,
                        device="cpu") -> torch.Tensor:
    """[max_pos, head_dim] fp32 = [cos(half) | sin(half)] — host-precomputed
    (guide Appendix B: no on-device trig in the RoPE kernel)."""
    half = head_dim // 2
    inv_freq = 1.0 / (theta ** (torch.arange(0, half, dtype=torch.float64,
                                             device=device) / half))
    pos = torch.arange(max_positions, dtype=torch.float64, device=device)
    freqs = torch.outer(pos, inv_freq)
    return torch.cat([freqs.cos(), freqs.sin()], dim=-1).float().contiguous()


def apply_rope(x: torch.Tensor, positions: torch.Tensor,
               cos_sin: torch.Tensor) -> torch.Tensor:
    """x [T, H, D]; rotate-half (Llama/NeoX) in fp32."""
    T, H, D = x.shape
    half = D // 2
    cs = cos_sin[positions.long()]            # [T, D]
    cos = cs[:, :half].unsqueeze(1)           # [T,1,half]
    sin = cs[:, half:].unsqueeze(1)
    xf = x.float()
    x1, x2 = xf[..., :half], xf[..., half:]
    out = torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1)
    return out.to(x.dtype)


# ---------------------------------------------------------------------------
# FP8 (OCP e4m3fn) KV cache (docs/FEATURES.md "FP8 KV cache")
# ---------------------------------------------------------------------------

KV_CACHE_DTYPES = {"bf16": torch.bfloat16, "fp8_e4m3": torch.float8_e4m3fn}
KV_SCALE_LOG2_RANGE = (-16, 16)
E4M3_MAX = 448.0


def check_kv_scale_log2(e, name: str = "scale_log2") -> int:
    lo, hi = KV_SCALE_LOG2_RANGE
    if isinstance(e, bool) or not isinstance(e, int) or not lo <= e <= hi:
        raise ValueError("%s must be an integer in [%d, %d], got %r" % (
            name, lo, hi, e))
    return e


def quantize_e4m3(x: torch.Tensor, scale_log2: int = 0) -> torch.Tensor:
    """q8(x) = sat_rne_e4m3fn(x * 2^-e): round to nearest even, finite
    overflow and +-inf saturate to +-448, NaN stays NaN.  The clamp comes
    first because torch's own conversion turns overflow into NaN."""
    y = x.float() * (2.0 ** -scale_log2)
    return y.clamp(-E4M3_MAX, E4M3_MAX).to(torch.float8_e4m3fn)


def dequantize_e4m3(b: torch.Tensor, scale_log2: int = 0,
                    dtype=torch.bfloat16) -> torch.Tensor:
    """dq(b) = e4m3(b) * 2^e, exact in bf16 (four significant bits)."""
    return (b.float() * (2.0 ** scale_log2)).to(dtype)


# FP8 (e4m3) projection weights (docs/FEATURES.md "FP8 weights"): bytes
# [N, K] with one power-of-two exponent per output row, int8 [N].
WEIGHT_DTYPES = ("bf16", "fp8_e4m3")
W_SCALE_LOG2_RANGE = (-64, 64)


def weight_scale_log2(w: torch.Tensor) -> torch.Tensor:
    """int8 [N]: per row the smallest e with amax <= 448 * 2^e, clamped to
    W_SCALE_LOG2_RANGE, 0 for an all-zero row.  From the exponent and
    mantissa of amax, not from a division that could round: amax = m * 2^x
    with m in [0.5, 1) and 448 = 0.875 * 2^9, so e = x - 9 where m <= 0.875
    and x - 8 above."""
    amax = w.float().abs().amax(dim=1)
    m, x = torch.frexp(amax)
    e = torch.where(m <= 0.875, x - 9, x - 8)
    e = torch.where(amax > 0, e, torch.zeros_like(e))
    return e.clamp(*W_SCALE_LOG2_RANGE).to(torch.int8)


def quantize_weight_e4m3(w: torch.Tensor
                         ) -> Tuple[torch.Tensor, torch.Tensor]:
    """W [N, K] -> (w8 e4m3 [N, K], e int8 [N]): row n is quantize_e4m3 of
    W[n] * 2^-e[n] (the scaling is exact, so the one rounding is e4m3's)."""
    if w.dim() != 2:
        raise ValueError("a projection weight is 2-D, got %s" % (
            tuple(w.shape),))
    e = weight_scale_log2(w)
    scaled = torch.ldexp(w.float(), -e.to(torch.int32).unsqueeze(1))
    return quantize_e4m3(scaled), e


def dequantize_weight_e4m3(w8: torch.Tensor, e: torch.Tensor
                           ) -> torch.Tensor:
    """dq[n, k] = e4m3(w8[n, k]) * 2^e[n] as bf16: exact, and a normal bf16
    or zero for every |e| <= 64."""
    if w8.dtype != torch.float8_e4m3fn or e.dtype != torch.int8 or \
            w8.dim() != 2 or e.numel() != w8.shape[0]:
        raise ValueError("need e4m3 [N, K] and int8 [N], got %s %s and %s %s"
                         % (w8.dtype, tuple(w8.shape), e.dtype,
                            tuple(e.shape)))
    return torch.ldexp(w8.float(),
                       e.to(torch.int32).view(-1, 1)).to(torch.bfloat16)


# MXFP4 expert weights (docs/FEATURES.md "MXFP4 experts"): e2m1 codes, two per
# byte (element 2i in the low nibble), with one power-of-two exponent per 32
# consecutive k of a row, int8 [N, K / 32].  Code = s eem; the dense
# projections have no MXFP4, so the experts' option has a tuple of its own.
EXPERT_WEIGHT_DTYPES = WEIGHT_DTYPES + ("mxfp4",)
MXFP4_BLOCK = 32
E2M1_GRID = (0.0, 0.5, 1.0, 1.5, 2.0, 3.0, 4.0, 6.0)
# (midpoint between codes c and c + 1, whether the tie goes up to c + 1: it
# does where c + 1 has mantissa bit 0, that is where c is odd)
_E2M1_MIDPOINTS = tuple(((E2M1_GRID[c] + E2M1_GRID[c + 1]) / 2, c % 2 == 1)
                        for c in range(7))


def quantize_weight_mxfp4(w: torch.Tensor
                          ) -> Tuple[torch.Tensor, torch.Tensor]:
    """W bf16 [N, K] -> (codes uint8 [N, K / 2], e int8 [N, K / 32]).  Per
    block of 32 k, e is the smallest integer with amax <= 6 * 2^e (clamped to
    W_SCALE_LOG2_RANGE, 0 for a zero block): amax = m * 2^x with m in
    [0.5, 1) and 6 = 0.75 * 2^3, so e = x - 3 where m <= 0.75 and x - 2
    above; no division.  W * 2^-e (exact) is rounded to the nearest e2m1
    value, ties to the code with mantissa bit 0, saturating at +-6."""
    if w.dim() != 2 or w.shape[1] % MXFP4_BLOCK:
        raise ValueError("an MXFP4 weight is [N, K] with K %% %d == 0, got %s"
                         % (MXFP4_BLOCK, tuple(w.shape)))
    wf = w.float()
    if not bool(torch.isfinite(wf).all()):
        raise ValueError("a non-finite weight has no e2m1 code")
    N, K = wf.shape
    blocks = wf.view(N, K // MXFP4_BLOCK, MXFP4_BLOCK)
    amax = blocks.abs().amax(dim=2)
    m, x = torch.frexp(amax)
    e = torch.where(m <= 0.75, x - 3, x - 2)
    e = torch.where(amax > 0, e, torch.zeros_like(e))
    e = e.clamp(*W_SCALE_LOG2_RANGE)
    mag = torch.ldexp(blocks.abs(), -e.to(torch.int32).unsqueeze(2))
    code = torch.zeros_like(mag, dtype=torch.uint8)
    for mid, tie_up in _E2M1_MIDPOINTS:
        code += (mag >= mid if tie_up else mag > mid).to(torch.uint8)
    code |= torch.signbit(blocks).to(torch.uint8) << 3
    code = code.view(N, K // 2, 2)
    return code[..., 0] | (code[..., 1] << 4), e.to(torch.int8)


def dequantize_weight_mxfp4(codes: torch.Tensor, e: torch.Tensor
                            ) -> torch.Tensor:
    """dq[n, k] = e2m1(code[n, k]) * 2^e[n, k / 32] as bf16: exact, and a
    normal bf16 or zero for every |e| <= 64."""
    if codes.dtype != torch.uint8 or e.dtype != torch.int8 or \
            codes.dim() != 2 or e.dim() != 2 or \
            codes.shape[1] % (MXFP4_BLOCK // 2) or \
            tuple(e.shape) != (codes.shape[0],
                               codes.shape[1] // (MXFP4_BLOCK // 2)):
        raise ValueError("need uint8 [N, K / 2] and int8 [N, K / 32], got %s "
                         "%s and %s %s" % (codes.dtype, tuple(codes.shape),
                                           e.dtype, tuple(e.shape)))
    N = codes.shape[0]
    nib = torch.stack((codes & 15, codes >> 4), dim=2).view(N, -1).long()
    grid = torch.tensor(E2M1_GRID + tuple(-v for v in E2M1_GRID),
                        device=codes.device)
    exp = e.to(torch.int32).repeat_interleave(MXFP4_BLOCK, dim=1)
    return torch.ldexp(grid[nib], exp).to(torch.bfloat16)


def kv_gather_dequant(cache: torch.Tensor, slots: torch.Tensor,
                      scale_log2: int = 0) -> torch.Tensor:
    page_size = cache.shape[2]
    sl = slots.long()
    rows = cache.view(torch.uint8)[sl // page_size, :, sl % page_size]
    return dequantize_e4m3(rows.view(torch.float8_e4m3fn), scale_log2)


def rope_store_kv(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                  key_cache: torch.Tensor, value_cache: torch.Tensor,
                  cos_sin: torch.Tensor, positions: torch.Tensor,
                  slot_mapping: torch.Tensor, k_scale_log2: int = 0,
                  v_scale_log2: int = 0) -> None:
    """Mutates q,k in place (rotated) and scatters k,v into the paged caches.
    Cache layout: [pages, kv_heads, page_size, head_dim].  An e4m3 cache
    receives quantize_e4m3 of the bf16 rows a bf16 cache would receive."""
    T = q.shape[0]
    head_dim = key_cache.shape[3]
    kvh = key_cache.shape[1]
    page_size = key_cache.shape[2]
    qh = q.numel() // (T * head_dim)
    q3 = q.view(T, qh, head_dim)
    k3 = k.view(T, kvh, head_dim)
    v3 = v.view(T, kvh, head_dim)
    q3.copy_(apply_rope(q3, positions, cos_sin))
    k3.copy_(apply_rope(k3, positions, cos_sin))
    slots = slot_mapping.long()
    valid = slots >= 0
    pages = torch.div(slots[valid], page_size, rounding_mode="floor")
    offs = slots[valid] % page_size
    if key_cache.dtype == torch.float8_e4m3fn:
        # index_put_ has no float8 kernel: move the bytes
        key_cache.view(torch.uint8)[pages, :, offs] = quantize_e4m3(
            k3[valid], k_scale_log2).view(torch.uint8)
        value_cache.view(torch.uint8)[pages, :, offs] = quantize_e4m3(
            v3[valid], v_scale_log2).view(torch.uint8)
        return
    key_cache[pages, :, offs] = k3[valid]
    value_cache[pages, :, offs] = v3[valid]


def decode_attention(q: torch.Tensor, key_cache: torch.Tensor,
                     value_cache: torch.Tensor, block_tables: torch.Tensor,
                     context_lens: torch.Tensor, scale: float,
                     k_scale_log2: int = 0,
                     v_scale_log2: int = 0) -> torch.Tensor:
    """q [S, QH, D] one token per sequence; paged KV.  An e4m3 cache is read
    as e4m3(byte) * 2^e."""
    S, QH, D = q.shape
    fp8 = key_cache.dtype == torch.float8_e4m3fn
    if fp8:      # index the bytes: advanced indexing has no float8 kernel
        key_cache = key_cache.view(torch.uint8)
        value_cache = value_cache.view(torch.uint8)
    kvh = key_cache.shape[1]
    page_size = key_cache.shape[2]
    qpg = QH // kvh
    out = torch.empty_like(q)
    for s in range(S):
        ctx = int(context_lens[s])
        npages = (ctx + page_size - 1) // page_size
        pages = block_tables[s, :npages].long()
        k = key_cache[pages].permute(1, 0, 2, 3).reshape(kvh, -1, D)[:, :ctx]
        v = value_cache[pages].permute(1, 0, 2, 3).reshape(kvh, -1, D)[:, :ctx]
        if fp8:
            k = dequantize_e4m3(k.contiguous().view(torch.float8_e4m3fn),
                                k_scale_log2, torch.float32)
            v = dequantize_e4m3(v.contiguous().view(torch.float8_e4m3fn),
                                v_scale_log2, torch.float32)
        qs = q[s].float().view(kvh, qpg, D)
        attn = torch.einsum("hgd,hkd->hgk", qs, k.float()) * scale
        p = torch.softmax(attn, dim=-1)
        o = torch.einsum("hgk,hkd->hgd", p, v.float())
        out[s] = o.reshape(QH, D).to(q.dtype)
    return out


def prefill_attention(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor,
                      cu_seqlens: torch.Tensor, scale: float,
                      cu_seqlens_k: Optional[torch.Tensor] = None
                      ) -> torch.Tensor:
    """Varlen causal attention; q [Tq,QH,D], k/v [Tkv,KVH,D].  With
    cu_seqlens_k, each sequence's q rows are its LAST (Lq) positions of the
    Lk-token KV (prefix caching / chunked prefill)."""
    Tq, QH, D = q.shape
    kvh = k.shape[1]
    qpg = QH // kvh
    out = torch.empty_like(q)
    cu = cu_seqlens.long().tolist()
    cuk = (cu_seqlens_k.long().tolist()
           if cu_seqlens_k is not None else cu)
    for b in range(len(cu) - 1):
        s, e = cu[b], cu[b + 1]
        sk, ek = cuk[b], cuk[b + 1]
        Lq, Lk = e - s, ek - sk
        off = Lk - Lq
        qs = q[s:e].float().view(Lq, kvh, qpg, D)
        ks = k[sk:ek].float()
        vs = v[sk:ek].float()
        attn = torch.einsum("qhgd,khd->hgqk", qs, ks) * scale
        qpos = torch.arange(off, Lk, device=q.device).unsqueeze(1)
        kpos = torch.arange(Lk, device=q.device).unsqueeze(0)
        attn.masked_fill_(kpos > qpos, float("-inf"))
        p = torch.softmax(attn, dim=-1)
        o = torch.einsum("hgqk,khd->qhgd", p, vs)
        out[s:e] = o.reshape(Lq, QH, D).to(q.dtype)
    return out


def prefill_block_info(cu_seqlens: torch.Tensor, qtile: int = 64,
                       cu_seqlens_k: Optional[torch.Tensor] = None
                       ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Host-side block map for the prefill kernel: per block
    (q_start_row, q_block_index, kv_start_row, q_offset) plus the block's
    total KV length."""
    infos = []
    lens = []
    cu = cu_seqlens.tolist()
    cuk = cu_seqlens_k.tolist() if cu_seqlens_k is not None else cu
    for b in range(len(cu) - 1):
        qs, qe = cu[b], cu[b + 1]
        ks, ke = cuk[b], cuk[b + 1]
        Lq, Lk = qe - qs, ke - ks
        off = Lk - Lq
        for qb in range((Lq + qtile - 1) // qtile):
            infos.append((qs, qb, ks, off))
            lens.append(Lk)
    device = cu_seqlens.device
    return (torch.tensor(infos, dtype=torch.int32, device=device).view(-1, 4),
            torch.tensor(lens, dtype=torch.int32, device=device))


def _int_list(x) -> list:
    return x.tolist() if isinstance(x, torch.Tensor) else list(x)


def prefill_block_info_paged(cu_seqlens, qtile: int = 128, cu_seqlens_k=None,
                             device=None
                             ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Block map of the paged prefill kernel: prefill_block_info with the
    sequence's index (its block-table row) where kv_start_row was.  Takes
    tensors or plain host lists, so a caller that has the lists builds the
    map without reading anything back from the device."""
    cu = _int_list(cu_seqlens)
    cuk = _int_list(cu_seqlens_k) if cu_seqlens_k is not None else cu
    infos = []
    lens = []
    for b in range(len(cu) - 1):
        Lq, Lk = cu[b + 1] - cu[b], cuk[b + 1] - cuk[b]
        for qb in range((Lq + qtile - 1) // qtile):
            infos.append((cu[b], qb, b, Lk - Lq))
            lens.append(Lk)
    if device is None and isinstance(cu_seqlens, torch.Tensor):
        device = cu_seqlens.device
    return (torch.tensor(infos, dtype=torch.int32, device=device).view(-1, 4),
            torch.tensor(lens, dtype=torch.int32, device=device))


def paged_kv_slots(block_tables: torch.Tensor, seq_lens, page_size: int
                   ) -> torch.Tensor:
    """Slots of keys 0 .. L-1 of every sequence, in order, read through its
    block-table row: int32 [sum L] on the table's device."""
    out = []
    for b, L in enumerate(_int_list(seq_lens)):
        pos = torch.arange(L, device=block_tables.device)
        pages = block_tables[b, :(L + page_size - 1) // page_size].long()
        out.append(pages[pos // page_size] * page_size + pos % page_size)
    if not out:
        return torch.zeros(0, dtype=torch.int32, device=block_tables.device)
    return torch.cat(out).to(torch.int32)


def prefill_attention_paged(q, key_cache, value_cache, block_tables,
                            cu_seqlens, scale: float, cu_seqlens_k=None,
                            k_scale_log2: int = 0, v_scale_log2: int = 0
                            ) -> torch.Tensor:
    """Prefill attention over the paged pool: the keys are gathered through
    the block tables (dequantised for an e4m3 pool), then prefill_attention."""
    cuk = _int_list(cu_seqlens_k if cu_seqlens_k is not None else cu_seqlens)
    page_size = key_cache.shape[2]
    slots = paged_kv_slots(block_tables,
                           [cuk[b + 1] - cuk[b] for b in range(len(cuk) - 1)],
                           page_size)
    if key_cache.dtype == torch.float8_e4m3fn:
        k_full = kv_gather_dequant(key_cache, slots, k_scale_log2)
        v_full = kv_gather_dequant(value_cache, slots, v_scale_log2)
    else:
        sl = slots.long()
        pages, offs = sl // page_size, sl % page_size
        k_full = key_cache[pages, :, offs]
        v_full = value_cache[pages, :, offs]
    cu_k = torch.tensor(cuk, dtype=torch.int32, device=q.device)
    return prefill_attention(q, k_full, v_full, cu_seqlens, scale, cu_k)


# ---------------------------------------------------------------------------
# seeded sampling (docs/FEATURES.md "Seeded sampling"; hip/sampling.hip)
# ---------------------------------------------------------------------------

_PHILOX_M0, _PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
_PHILOX_W0, _PHILOX_W1 = 0x9E3779B9, 0xBB67AE85


def philox4x32_10(counter, key):
    """Philox4x32-10 over numpy uint64 lanes holding 32-bit words.
    counter: 4 arrays (or ints), key: 2 ints -> 4 uint64 arrays < 2^32."""
    import numpy as np
    mask = np.uint64(0xFFFFFFFF)
    c = [np.asarray(w, dtype=np.uint64) & mask for w in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(_PHILOX_M0) * c[0]
        p1 = np.uint64(_PHILOX_M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & mask,
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & mask]
        k0 = (k0 + _PHILOX_W0) & 0xFFFFFFFF
        k1 = (k1 + _PHILOX_W1) & 0xFFFFFFFF
    return c


def _gumbel_f32(x):
    """g = -log(-log u), u = ((x >> 8) + 0.5) * 2^-24, in fp32.  The upper
    half goes through log1p of the exactly representable 1 - u (m + 0.5 is
    not an fp32 number for m >= 2^23)."""
    import numpy as np
    m = (x >> np.uint64(8)).astype(np.int64)
    f32 = np.float32
    low = m < (1 << 23)
    scale = f32(2.0 ** -24)
    u = (m.astype(f32) + f32(0.5)) * scale
    v = (((1 << 24) - m).astype(f32) - f32(0.5)) * scale
    with np.errstate(divide="ignore", invalid="ignore"):
        w = np.where(low, -np.log(np.where(low, u, f32(0.5))),
                     -np.log1p(-np.where(low, f32(0.5), v))).astype(f32)
        return (-np.log(w)).astype(f32)


def _sample_row(l, T, k, p, mp, seed, pos):
    import numpy as np
    f32 = np.float32
    V = l.shape[0]
    l = np.where(np.isnan(l), f32(-np.inf), l).astype(f32)
    keep = l > f32(-np.inf)
    if not keep.any():
        return 0, 0
    if not T > 0:
        return int(np.argmax(l)), 1
    T = f32(T)
    lmax = l.max()
    if 0 < k < V:
        keep &= l >= np.partition(l, V - k)[V - k]
    if mp > 0:
        keep &= l >= f32(lmax + f32(T * np.log(f32(mp))))
    with np.errstate(over="ignore", invalid="ignore"):
        z = (l / T).astype(f32)
    if p < 1:
        # softmax mass as integers in units of 2^-40, like the kernel: the
        # prefix sums are then exact and independent of summation order
        idx = np.flatnonzero(keep)
        with np.errstate(over="ignore", invalid="ignore"):
            e = np.exp((z[idx] - f32(lmax / T)).astype(f32)).astype(f32)
        e = np.where(e >= 0, e, f32(0))
        w = [int(x) for x in np.floor(e.astype(np.float64) * 2.0 ** 40)]
        order = sorted(range(len(idx)), key=lambda i: -float(l[idx[i]]))
        total = sum(w)
        target = max(1, min(total, int(float(f32(p)) * float(total))))
        acc = 0
        cut = l[idx[order[-1]]]
        for i in order:
            acc += w[i]
            if acc >= target:
                cut = l[idx[i]]
                break
        keep &= l >= cut
    idx = np.flatnonzero(keep)
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    words = philox4x32_10((idx >> 2, int(pos) & 0xFFFFFFFF, 0, 0),
                          (seed & 0xFFFFFFFF, seed >> 32))
    x = np.choose(idx & 3, words)
    with np.errstate(over="ignore", invalid="ignore"):
        score = (z[idx] + _gumbel_f32(x)).astype(f32)
    return int(idx[int(np.argmax(score))]), int(idx.size)


def sample(logits: torch.Tensor, temperature: torch.Tensor,
           top_k: torch.Tensor, top_p: torch.Tensor, min_p: torch.Tensor,
           seed: torch.Tensor, pos: torch.Tensor
           ) -> Tuple[torch.Tensor, torch.Tensor]:
    """CPU twin of hip/sampling.hip: per-row temperature / top-k / min-p /
    top-p filters, then a Gumbel-max draw over Philox4x32-10 noise keyed by
    (seed, pos).  fp32 arithmetic in the kernel's order; returns (tokens
    int64 [n], num_kept int32 [n])."""
    n = logits.shape[0]
    rows = logits.detach().float().cpu().numpy()
    toks = torch.empty(n, dtype=torch.int64)
    kept = torch.empty(n, dtype=torch.int32)
    for r in range(n):
        t, c = _sample_row(rows[r], float(temperature[r]), int(top_k[r]),
                           float(top_p[r]), float(min_p[r]), int(seed[r]),
                           int(pos[r]))
        toks[r], kept[r] = t, c
    return toks.to(logits.device), kept.to(logits.device)


# ---------------------------------------------------------------------------
# Mixture of experts (docs/FEATURES.md "Mixture of experts")
# ---------------------------------------------------------------------------

MOE_MAX_EXPERTS = 256
MOE_MAX_TOP_K = 8


def moe_route(router_logits: torch.Tensor, top_k: int,
              renormalize: bool = True) -> Tuple[torch.Tensor, torch.Tensor]:
    """(ids int32 [T, k], w fp32 [T, k]) of bf16 logits [T, E].  The k largest
    logits by comparison, exact ties to the lower index, NaN as -inf, ordered
    by descending logit; w = fp32 softmax over all E at the selected experts,
    with `renormalize` divided by their fp32 sum added in slot order."""
    x = router_logits.float()
    x = torch.where(torch.isnan(x), torch.full_like(x, float("-inf")), x)
    # a stable descending sort keeps equal logits in index order
    order = torch.sort(x, dim=-1, descending=True, stable=True).indices
    ids = order[:, :top_k]
    w = torch.softmax(x, dim=-1).gather(1, ids)
    if renormalize:
        total = w[:, 0].clone()
        for j in range(1, top_k):
            total = total + w[:, j]
        w = w / total.unsqueeze(1)
    return ids.to(torch.int32).contiguous(), w.contiguous()


def moe_ffn(x: torch.Tensor, w1: torch.Tensor, w2: torch.Tensor,
            ids: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """y bf16 [T, H] with the kernels' rounding points, one expert at a time:
    g, u = x w1[e]^T in fp32 (not rounded), h = bf16(silu(g) * u),
    o = h w2[e]^T in fp32, y[t] = bf16(sum_j w[t, j] * o[t, j]) in slot
    order."""
    T, H = x.shape
    E, inter, k = w1.shape[0], w2.shape[2], ids.shape[1]
    xf = x.float()
    o = torch.zeros(T, k, H, dtype=torch.float32, device=x.device)
    for e in range(E):
        t_idx, j_idx = (ids == e).nonzero(as_tuple=True)
        if t_idx.numel() == 0:
            continue
        gu = xf[t_idx] @ w1[e].float().t()
        h = torch.nn.functional.silu(gu[:, :inter]) * gu[:, inter:]
        o[t_idx, j_idx] = h.to(x.dtype).float() @ w2[e].float().t()
    y = torch.zeros(T, H, dtype=torch.float32, device=x.device)
    for j in range(k):
        y = y + w[:, j:j + 1].float() * o[:, j]
    return y.to(x.dtype)
