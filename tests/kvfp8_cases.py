"""Shared inputs, references and checks for the FP8 (e4m3) KV cache tests.

A plain helper module (not a conftest): tests/test_kvfp8_cases_cpu.py runs
its self-test and the CPU-level checks, tests/test_kvfp8_gpu.py runs the same
cases against the HIP kernels.

Semantics under test (docs/FEATURES.md "FP8 KV cache"): a cached element is
q8(x) = sat_rne_e4m3fn(x * 2^-e) of the bf16 value a bf16 cache would hold,
and reads back as dq(b) = e4m3(b) * 2^e.  Both steps are exact in the formats
involved, so the kernel-level checks are exact where the bf16 ones are:

  quantiser  bytes equal the torch reference (clamp, then .to(float8_e4m3fn))
             for all 65 536 bf16 bit patterns; NaN compares as NaN.
  gather     torch.equal against cache.to(bf16)[pages, :, offs] * 2^e.
  decode     the attn_cases decode cases with their caches quantised; the
             fp64 reference and A = sum p|v| are recomputed on the
             DEQUANTISED caches, and attn_cases.check judges with unchanged
             bounds (torch.equal for needle, TOL = 2^-7 + 2^-12 otherwise):
             dequantisation and power-of-two scales add no rounding.

Poison is byte 0x7E (448) for V and +-4 for K: attn_cases' V poison 32768
saturates to 0x7E under every exponent used here, and +-4 * 2^-e is an e4m3
number.
"""
from __future__ import annotations

import functools
from typing import Dict, Optional, Tuple

import torch

import attn_cases as ac
import kernel_cases as kc
from rbg_amd.ops import reference

BF16 = torch.bfloat16
FP8 = torch.float8_e4m3fn
U8 = torch.uint8
V_POISON_BYTE = 0x7E
K_POISON = ac.K_POISON

QUANT_EXPONENTS = (-3, 0, 2)
QUANT_HEADS = ((2, 1), (32, 8))            # (QH, KVH)
QUANT_TS = (1, 37)
DECODE_EXPONENTS = ((0, 0), (-2, 3))       # (ek, ev)
GATHER_TKV = (1, 17, 300)
GATHER_KVH = (1, 8)

q8 = reference.quantize_e4m3


def dq(b: torch.Tensor, e: int) -> torch.Tensor:
    """e4m3 tensor -> bf16, exactly."""
    out = reference.dequantize_e4m3(b, e)
    assert out.dtype == BF16
    return out


def is_nan_byte(b: torch.Tensor) -> torch.Tensor:
    return (b & 0x7F) == 0x7F


def bytes_match(got: torch.Tensor, want: torch.Tensor
                ) -> Tuple[bool, str]:
    """uint8 tensors equal byte for byte, a NaN code matching any NaN code."""
    got, want = got.cpu(), want.cpu()
    if got.shape != want.shape:
        return False, "shape %s, want %s" % (tuple(got.shape),
                                             tuple(want.shape))
    bad = (got != want) & ~(is_nan_byte(got) & is_nan_byte(want))
    if not bool(bad.any()):
        return True, ""
    i = bad.nonzero()[0].tolist()
    return False, "%d of %d bytes differ; first at %s: got 0x%02X want 0x%02X" \
        % (int(bad.sum()), bad.numel(), i, int(got[tuple(i)]),
           int(want[tuple(i)]))


# ---------------------------------------------------------------------------
# quantiser
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=1)
def all_bf16_patterns() -> torch.Tensor:
    """Every bf16 bit pattern once: [512, 1, 128]."""
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    return bits.view(BF16).view(512, 1, 128).clone()


def exhaustive_inputs(permuted: bool) -> Dict:
    """All 65 536 patterns as V and as K (512 tokens x 1 head x 128), every
    token at position 0 of the quarter-turn table: the rotation is an exact
    sign/swap permutation there, so every finite pattern reaches the K
    quantiser unrounded (an inf or NaN turns its rotation partner into NaN,
    in the reference as in the kernel).  permuted: a shuffled slot_mapping
    with -1 entries instead of the identity."""
    g = kc._gen(("kvfp8-exhaustive", permuted))
    pats = all_bf16_patterns()
    T = pats.shape[0]
    pages = T // 16 + 3
    if permuted:
        slots = torch.randperm(pages * 16, generator=g)[:T]
        slots[torch.arange(T) % 5 == 3] = -1
    else:
        slots = torch.arange(16, 16 + T)
    return {"q": torch.randn(T, 2, 128, generator=g).to(BF16),
            "k": pats.clone(), "v": pats.clone(), "pages": pages,
            "slots": slots.to(torch.int32),
            "pos": torch.zeros(T, dtype=torch.int32),
            "table": kc.quarter_table()}


def quant_inputs(qh: int, kvh: int, T: int, seed: int) -> Dict:
    """q/k/v [T, H, 128] whose K and V draw from all bf16 bit patterns
    (specials included), a permuted slot_mapping with -1 entries."""
    g = kc._gen(("kvfp8", qh, kvh, T, seed))
    pats = all_bf16_patterns().reshape(-1)

    def draw(h):
        idx = torch.randint(0, 65536, (T, h, 128), generator=g)
        return pats[idx]
    q = torch.randn(T, qh, 128, generator=g).to(BF16)
    k, v = draw(kvh), draw(kvh)
    pages = (T + 15) // 16 + 2
    slots = torch.randperm(pages * 16, generator=g)[:T]
    slots[torch.arange(T) % 5 == 3] = -1
    pos = (torch.arange(T) * 29 + 7) % kc.ROPE_QUARTER_ROWS
    return {"q": q, "k": k, "v": v, "pages": pages,
            "slots": slots.to(torch.int32), "pos": pos.to(torch.int32),
            "table": kc.quarter_table()}


def poison_pool(pages: int, kvh: int, gen: Optional[torch.Generator] = None
                ) -> Tuple[torch.Tensor, torch.Tensor]:
    """All-poison e4m3 pools: K = +-4, V = byte 0x7E."""
    gen = gen or torch.Generator().manual_seed(11)
    shape = (pages, kvh, 16, 128)
    k = ((torch.randint(0, 2, shape, generator=gen) * 2 - 1) * K_POISON
         ).to(BF16)
    kq = q8(k, 0)
    assert torch.equal(dq(kq, 0), k)
    vq = torch.full(shape, V_POISON_BYTE, dtype=U8).view(FP8)
    return kq, vq


def fused_slices(q, k, v):
    """q, k, v as column slices of one fused QKV buffer [T, (QH+2KVH)*128]."""
    T, qh, kvh = q.shape[0], q.shape[1], k.shape[1]
    width = (qh + 2 * kvh) * 128
    qkv = torch.full((T, width), 3.0, dtype=BF16, device=q.device)
    a, b = qh * 128, (qh + kvh) * 128
    qkv[:, :a] = q.reshape(T, -1)
    qkv[:, a:b] = k.reshape(T, -1)
    qkv[:, b:] = v.reshape(T, -1)
    return qkv, qkv[:, :a], qkv[:, a:b], qkv[:, b:]


def store_expected(data: Dict, kq0, vq0, ek: int, ev: int):
    """What rope_store_kv must leave behind, by the torch reference on the
    CPU: (q, k in place, key bytes, value bytes)."""
    q, k = data["q"].clone(), data["k"].clone()
    kq, vq = kq0.clone(), vq0.clone()
    reference.rope_store_kv(q, k, data["v"], kq, vq, data["table"],
                            data["pos"], data["slots"], ek, ev)
    return q, k, kq.view(U8), vq.view(U8)


# ---------------------------------------------------------------------------
# gather
# ---------------------------------------------------------------------------

def gather_inputs(tkv: int, kvh: int, seed: int = 3):
    """A cache of random finite e4m3 bytes and permuted slots."""
    g = kc._gen(("kvfp8-gather", tkv, kvh, seed))
    pages = (tkv + 15) // 16 + 3
    b = torch.randint(0, 256, (pages, kvh, 16, 128), generator=g).to(U8)
    b = torch.where(is_nan_byte(b), torch.full_like(b, V_POISON_BYTE), b)
    slots = torch.randperm(pages * 16, generator=g)[:tkv].to(torch.int32)
    return b.view(FP8), slots


def gather_expected(cache: torch.Tensor, slots: torch.Tensor, e: int
                    ) -> torch.Tensor:
    sl = slots.long().cpu()
    rows = cache.cpu().to(BF16)[sl // 16, :, sl % 16]
    out = (rows.float() * 2.0 ** e).to(BF16)
    assert torch.equal(out.float(), rows.float() * 2.0 ** e)    # exact
    return out


# ---------------------------------------------------------------------------
# decode
# ---------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def decode_data(case: ac.DecodeCase, family: str, ek: int, ev: int) -> Dict:
    """An attn_cases decode case with its caches quantised.  Keys: q, bt,
    ctx, scale, kq, vq (e4m3), kd, vd (the dequantised bf16 caches), and the
    expectation attn_cases.check reads (expect | ref64 [, abs64])."""
    base = ac.decode_data(case, family)
    kq, vq = q8(base["kc"], ek), q8(base["vc"], ev)
    kd, vd = dq(kq, ek), dq(vq, ev)
    # poison: V byte 0x7E wherever attn_cases holds 32768, K still +-4
    poison_v = base["vc"] == ac.V_POISON
    assert bool((vq.view(U8)[poison_v] == V_POISON_BYTE).all())
    assert bool(poison_v.any())
    pp = base["meta"].poison_page
    assert bool((kd[pp].abs() == K_POISON).all())
    data = {k: base[k] for k in ("family", "case", "meta", "scale", "q", "bt",
                                 "ctx", "rows")}
    data.update(kq=kq, vq=vq, kd=kd, vd=vd, ek=ek, ev=ev)
    if family == "needle":
        # the needle family quantises losslessly: K = +-1, V = x/8 with
        # x in 1..16 (four significant bits), so the expectation stands
        assert torch.equal(kd, base["kc"])
        assert torch.equal(vd[~poison_v], base["vc"][~poison_v])
        data["expect"] = base["expect"]
        data["targets"] = base["targets"]
        return data
    args = (data["q"], kd, vd, data["bt"], data["ctx"], ac.SCALE)
    data["ref64"] = ac.decode_ref64(*args)
    if family == "scaled":
        data["abs64"] = ac.attn_abs64(ac.decode_ref64, *args)
    return data


def decode_cpu(data: Dict) -> torch.Tensor:
    """The project's CPU path on the quantised caches."""
    return reference.decode_attention(data["q"], data["kq"], data["vq"],
                                      data["bt"], data["ctx"], data["scale"],
                                      data["ek"], data["ev"])


def decode_emulated(data: Dict) -> torch.Tensor:
    """attn_cases' bf16-faithful kernel emulation on the dequantised caches:
    what the fp8 kernel computes once its stage has converted the bytes."""
    return ac.decode_emulated(data["q"], data["kd"], data["vd"], data["bt"],
                              data["ctx"], data["scale"])


FP8_MUTANTS = ("dq_e_plus_1", "k_bytes_as_v")
DECODE_MUTANTS = tuple(m for m in ac.DECODE_MUTANTS) + FP8_MUTANTS


def decode_mutant_applies(mut: str, case: ac.DecodeCase) -> bool:
    if mut in FP8_MUTANTS:
        return True
    return ac.decode_mutant_applies(mut, case)


def decode_mutant(data: Dict, mut: str) -> torch.Tensor:
    """A wrong fp8 decode: attn_cases' mutants over the dequantised caches,
    'dequantise with e + 1', and 'read K bytes as V'."""
    kd, vd = data["kd"], data["vd"]
    inner = mut
    if mut == "dq_e_plus_1":
        kd, vd = dq(data["kq"], data["ek"] + 1), dq(data["vq"], data["ev"] + 1)
        inner = None
    elif mut == "k_bytes_as_v":
        vd = dq(data["kq"], data["ev"])
        inner = None
    return ac._decode64(data["q"], kd, vd, data["bt"], data["ctx"],
                        data["scale"], mut=inner).to(BF16)
