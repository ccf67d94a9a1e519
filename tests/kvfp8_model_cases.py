"""Model-level checks of the FP8 (e4m3) KV cache: the scenarios, pool and
shapes of tests/model_cases.py with the engine in fp8 mode.

  reference  model_cases' dense fp64 forward with K and V replaced by
             dq(q8(bf16(.))) in every layer: what the fp8 semantics define
             (docs/FEATURES.md "FP8 KV cache"), nothing else rounded.
  yardstick  e_cpu8: the project's CPU path in fp8 mode (one full-history
             prefill through the gather path) against that same reference.
  statistic  relative L2 over the stacked logits rows of all the scenario's
             sequences (C1) and over each (layer, K|V) block of all their
             dequantised cache rows (C2).  Not a per-row maximum: a value near
             an e4m3 rounding boundary can flip by a whole code (2^-3
             relative), and a maximum over rows is dominated by the rare row
             where that happens.  Per sequence it was still too noisy: the
             fp32-upcast CPU emulation reached 2.03 x e_cpu8 on one
             (sequence, layer, V) block, so the aggregate is the scenario.
  bound      model_cases.FACTOR (2) x e_cpu8, as for the bf16 engine.
  C3         every byte no sequence wrote still holds its poison (V byte
             0x7E, K +-4); slot 0 of page 0 is exempt in graph mode.

model_cases offers no hook for engine kwargs or for the fp8 entry points in
its call trace, so run_scenario, the trace and the judge are restated here;
the scenario drivers, the recorder, the weights and the poison check are
model_cases' own.
"""
from __future__ import annotations

import math
from typing import Dict, List, Tuple

import torch

import kvfp8_cases as k8
import model_cases as mc
from rbg_amd import ops
from rbg_amd.engine.engine import LLMEngine
from rbg_amd.engine.kv_cache import BlockTable, PagedKVCache
from rbg_amd.models.llama import ForwardBatch, LlamaForCausalLM

BF16, FP8, U8 = torch.bfloat16, torch.float8_e4m3fn, torch.uint8
EK, EV = -2, -3                      # both pools scale their values up
SCENARIOS = ("mixed", "churn", "chunked", "prefix")
FP8_KW = dict(kv_cache_dtype="fp8_e4m3", kv_k_scale_log2=EK,
              kv_v_scale_log2=EV)


def dq_q8(x: torch.Tensor, e: int) -> torch.Tensor:
    """fp64 -> dq(q8(bf16(x))) as fp64."""
    return k8.dq(k8.q8(x.to(BF16), e), e).double()


def dense_forward64_q8(model: LlamaForCausalLM, tokens: List[int]
                       ) -> Tuple[torch.Tensor, torch.Tensor]:
    """model_cases.dense_forward64 with every layer's K (after qk-norm and
    RoPE) and V replaced by dq(q8(bf16(.))) before attention.  Returns
    logits [T, vocab] and the dequantised kv [T, layers, 2, KVH, D]."""
    cfg = model.cfg
    T = len(tokens)
    D, H, KVH = cfg.head_dim, cfg.num_heads, cfg.num_kv_heads
    G = H // KVH
    half = D // 2
    eps = float(torch.tensor(cfg.rms_eps, dtype=torch.float32))
    scale = 1.0 / math.sqrt(D)
    cs = model.cos_sin.detach().cpu().double()[:T]
    cos, sin = cs[:, None, :half], cs[:, None, half:]

    def w(p):
        return p.detach().cpu().double()

    def rms(x, weight):
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * weight

    def rope(x):
        x1, x2 = x[..., :half], x[..., half:]
        return torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1)

    future = torch.arange(T).unsqueeze(0) > torch.arange(T).unsqueeze(1)
    r = w(model.embed)[torch.tensor(tokens, dtype=torch.long)]
    kvs = []
    for layer in model.layers:
        a = layer.attn
        qkv = rms(r, w(layer.input_norm)) @ w(a.wqkv).T
        q = qkv[:, :H * D].reshape(T, H, D)
        k = qkv[:, H * D:(H + KVH) * D].reshape(T, KVH, D)
        v = qkv[:, (H + KVH) * D:].reshape(T, KVH, D)
        if a.q_norm is not None:
            q, k = rms(q, w(a.q_norm)), rms(k, w(a.k_norm))
        q, k = rope(q), rope(k)
        k, v = dq_q8(k, EK), dq_q8(v, EV)
        kvs.append(torch.stack([k, v], dim=1))
        sc = torch.einsum("qhgd,khd->hgqk", q.view(T, KVH, G, D), k) * scale
        p = torch.softmax(sc.masked_fill(future, float("-inf")), dim=-1)
        o = torch.einsum("hgqk,khd->qhgd", p, v).reshape(T, H * D)
        r = r + o @ w(a.wo).T
        gate, up = (rms(r, w(layer.post_norm)) @
                    w(layer.mlp.w_gate_up).T).chunk(2, dim=-1)
        r = r + (torch.nn.functional.silu(gate) * up) @ w(layer.mlp.w_down).T
    logits = rms(r, w(model.final_norm)) @ w(model.lm_head).T
    return logits, torch.stack(kvs, dim=1)


def dequant_rows(rows: torch.Tensor) -> torch.Tensor:
    """[count, layers, 2, KVH, D] e4m3 rows -> the bf16 values they mean."""
    rows = rows.cpu()
    return torch.stack([k8.dq(rows[:, :, 0], EK), k8.dq(rows[:, :, 1], EV)],
                       dim=2)


def cpu_forward8(model: LlamaForCausalLM, conf: str, tokens: List[int]
                 ) -> Tuple[torch.Tensor, torch.Tensor]:
    """The project's CPU path in fp8 mode: one full-history prefill into a
    fresh fp8 PagedKVCache, attention through the gather path.  `model` may
    be the bf16 CPU model (the yardstick) or its fp32 upcast (a second,
    independent emulation).  Returns logits and the dequantised rows."""
    T = len(tokens)
    cfg = mc.engine_config(conf, "cpu", True, enable_prefix_cache=False,
                           **FP8_KW)
    cache = PagedKVCache(cfg, torch.device("cpu"),
                         num_pages=(T + mc.PAGE - 1) // mc.PAGE + 1)
    assert cache.kv.dtype == FP8
    table = BlockTable(cache)
    slots = torch.tensor(table.slots_for(0, T), dtype=torch.int32)
    cu = torch.tensor([0, T], dtype=torch.int32)
    batch = ForwardBatch(mode="prefill",
                         positions=torch.arange(T, dtype=torch.int32),
                         slot_mapping=slots, cu_seqlens=cu, cu_seqlens_k=cu,
                         kv_gather_slots=slots)
    hidden = model.forward(torch.tensor(tokens, dtype=torch.int64), batch,
                           cache)
    rows = mc.gather_rows(cache.kv.view(U8), table.pages, T).view(FP8)
    return model.logits(hidden), dequant_rows(rows)


def poison_pool8(cache: PagedKVCache, seed: int = 7) -> torch.Tensor:
    """K = +-4 (as cached: the byte of +-4 * 2^-ek), V = byte 0x7E."""
    gen = torch.Generator().manual_seed(seed)
    shape = cache.kv.shape
    k = ((torch.randint(0, 2, shape[:1] + shape[2:], generator=gen) * 2 - 1)
         * k8.K_POISON).to(BF16)
    kq = k8.q8(k, EK)
    assert torch.equal(k8.dq(kq, EK), k)
    poison = torch.full(shape, k8.V_POISON_BYTE, dtype=U8)
    poison[:, 0] = kq.view(U8)
    cache.kv.view(U8).copy_(poison)
    return poison.view(FP8)


class Trace8:
    """Counts the calls that reach each KV-touching entry point of the HIP
    extension (GPU) or of ops.reference (CPU)."""

    FP8_NAMES = ("rope_store_kv_fp8", "kv_gather_dequant",
                 "decode_attention_fp8")
    BF16_NAMES = ("rope_store_kv", "decode_attention")

    def __init__(self, gpu: bool):
        self.gpu = gpu
        self.calls: Dict[str, int] = {}
        self.cache_dtypes = set()

    def _wrap(self, obj, name):
        fn = getattr(obj, name)
        self._saved.append((obj, name, fn))

        def wrapped(*a, **kw):
            self.calls[name] = self.calls.get(name, 0) + 1
            self.cache_dtypes.update(
                t.dtype for t in a if isinstance(t, torch.Tensor) and
                t.dim() == 4)
            return fn(*a, **kw)
        setattr(obj, name, wrapped)

    def __enter__(self):
        self._saved = []
        if self.gpu:
            for name in self.FP8_NAMES + self.BF16_NAMES:
                self._wrap(ops._hip, name)
        else:
            for name in ("rope_store_kv", "kv_gather_dequant",
                         "decode_attention"):
                self._wrap(ops.reference, name)
        return self

    def __exit__(self, *exc):
        for obj, name, fn in self._saved:
            setattr(obj, name, fn)
        return False

    def assert_fp8_paths(self, graph_mode: bool) -> None:
        if self.gpu:
            for name in self.FP8_NAMES:
                assert self.calls.get(name, 0) > 0, (name, self.calls)
            for name in self.BF16_NAMES:
                assert self.calls.get(name, 0) == 0, (name, self.calls)
        else:
            for name in ("rope_store_kv", "kv_gather_dequant",
                         "decode_attention"):
                assert self.calls.get(name, 0) > 0, (name, self.calls)
        assert self.cache_dtypes == {FP8}, self.cache_dtypes


def run_scenario8(scenario: str, conf: str, device: str, eager: bool
                  ) -> mc.Run:
    """model_cases.run_scenario with an fp8 pool."""
    run = mc.Run(scenario, conf, device, eager)
    run.engine = LLMEngine(mc.engine_config(
        conf, device, eager, **FP8_KW, **mc._SCENARIO_KW.get(scenario, {})))
    cache = run.engine.runner.cache
    assert cache.kv.dtype == FP8 and cache.fp8
    assert cache.num_pages == mc.POOL_TOKENS // mc.PAGE
    mc.draw_norm_weights(run.engine.runner.model)
    run.poison = poison_pool8(cache)
    run.rec = mc.Recorder(run.engine, conf)
    run.trace = Trace8(device != "cpu")

    gather_rows = mc.gather_rows

    def gather_bytes(kv, pages, count):
        return gather_rows(kv.view(U8), pages, count)
    with mc._patched(mc, "gather_rows", gather_bytes), run.trace, run.rec:
        mc._SCENARIO_FN[scenario](run)
    run.kv_after = cache.kv.cpu().clone()
    return run


def judge8(run: mc.Run, upcast_run: bool = False):
    """(c1, c2, c3): c1 is (what, err, e_cpu8) over the stacked logits rows
    of ALL the scenario's sequences, c2 one entry per (layer, K|V) over all
    their dequantised cache rows, c3 the poison violations.  err and e_cpu8
    are relative L2: sqrt(sum |x - ref|^2 / sum |ref|^2) over the whole
    scenario.  (Per sequence the statistic is too noisy for a factor of 2:
    a block of ~2 000 elements sees a handful of whole-code e4m3 flips, and
    the fp32-upcast emulation measured 2.03 x e_cpu8 on one such block.)
    With upcast_run the judged logits and rows are not the engine's but the
    fp32-upcast CPU path's: the second, independent emulation whose ratios
    must also stay under FACTOR."""
    rec = run.rec
    table = run.engine.runner.model.cos_sin
    model = mc.cpu_model(run.conf, rec.weights[0], table)
    up = mc.cpu_model(run.conf, rec.weights[0], table).float()
    sums: Dict[str, List[float]] = {}      # what -> [err^2, cpu err^2, ref^2]

    def add(what, got, cpu, ref):
        acc = sums.setdefault(what, [0.0, 0.0, 0.0])
        acc[0] += float((got.double() - ref).pow(2).sum())
        acc[1] += float((cpu.double() - ref).pow(2).sum())
        acc[2] += float(ref.pow(2).sum())

    for rec_seq in rec.seqs.values():
        seq = rec_seq.seq
        tokens = seq.prompt_tokens + seq.output_tokens
        T = len(tokens)
        assert rec_seq.final_kv is not None and rec_seq.final_count == T - 1
        pos = [r[0] - 1 for r in rec_seq.rows]
        assert pos == list(range(seq.num_prompt_tokens - 1, T - 1))
        ref_logits, ref_kv = dense_forward64_q8(model, tokens)
        cpu_logits, cpu_kv = cpu_forward8(model, run.conf, tokens)
        if upcast_run:
            got_logits, got_kv = cpu_forward8(up, run.conf, tokens)
            got_logits, got_kv = got_logits[pos], got_kv[:T - 1]
        else:
            got_logits = torch.stack([r[1] for r in rec_seq.rows])
            got_kv = dequant_rows(rec_seq.final_kv.view(FP8))
        add("logits", got_logits, cpu_logits[pos], ref_logits[pos])
        for layer in range(ref_kv.shape[1]):
            for j, name in enumerate("KV"):
                add("layer %d %s" % (layer, name), got_kv[:, layer, j],
                    cpu_kv[:T - 1, layer, j], ref_kv[:T - 1, layer, j])
    rows = [(what, math.sqrt(a / r), math.sqrt(c / r))
            for what, (a, c, r) in sums.items()]
    c3 = mc.poison_violations(run.kv_after, run.poison, rec.written_mask(),
                              rec.owned, run.graph_mode)
    return rows[:1], rows[1:], c3


def failures(c1, c2, c3) -> List[str]:
    out = ["C1 %s: err %.4g > %g * e_cpu8 %.4g" % (w, e, mc.FACTOR, y)
           for w, e, y in c1 if not e <= mc.FACTOR * y]
    out += ["C2 %s: err %.4g > %g * e_cpu8 %.4g" % (w, e, mc.FACTOR, y)
            for w, e, y in c2 if not e <= mc.FACTOR * y]
    return out + ["C3 " + v for v in c3]


def worst(c1, c2) -> Tuple[float, float]:
    """Worst err / e_cpu8 over the sequences' logits and over the K/V
    blocks."""
    def ratio(e, y):
        return e / y if y > 0 else (0.0 if e == 0 else float("inf"))
    return (max(ratio(e, y) for _, e, y in c1),
            max(ratio(e, y) for _, e, y in c2))
