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
