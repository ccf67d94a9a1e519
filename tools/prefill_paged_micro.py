#!/usr/bin/env python
"""Micro-benchmark of paged prefill attention (docs/FEATURES.md "Paged
prefill"): one layer's attention over a paged KV pool, three ways, for a bf16
and an e4m3 pool, 32 q heads / 8 KV heads:

  gather  what the model runs with prefill_kv_read = "gather": slot index
          math + two torch gathers (bf16) or two kv_gather_dequant launches
          (e4m3), then ops.prefill_attention on the gathered rows
  paged   ops.prefill_attention_paged on the pool, block map prebuilt (the
          model runner builds it once per step)
  floor   ops.prefill_attention alone on rows gathered beforehand: what the
          paged kernel is judged against, not the code under test.  It still
          pays the per-call cu_seqlens read-back of ops.prefill_attention.

Shapes (Lq, Lk): one sequence of (2048, 2048), (2048, 8192), (512, 8192) and
16 sequences of (128, 2048).  The three paths alternate launch by launch in
one process; median and min of --iters event-timed rounds after --warmup.
Bytes are computed from the shapes: K and V of the history once per path that
streams them (the kernels re-read tiles per q block and q head out of L2;
that is not counted), plus the gathered copy's write and read-back.

    python tools/prefill_paged_micro.py --out profiles/prefill_paged_micro.json
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from rbg_amd import ops  # noqa: E402

QH, KVH, D, PAGE = 32, 8, 128, 16
SCALE = 1.0 / 128 ** 0.5
BF16 = torch.bfloat16
SHAPES = ((1, 2048, 2048), (1, 2048, 8192), (1, 512, 8192), (16, 128, 2048))


def alternate(fns, warmup, iters):
    """Per round one event-timed call of each fn; {name: [us, ...]}."""
    out = {name: [] for name in fns}
    start, stop = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    for it in range(warmup + iters):
        for name, fn in fns.items():
            start.record()
            fn()
            stop.record()
            stop.synchronize()
            if it >= warmup:
                out[name].append(start.elapsed_time(stop) * 1e3)
    return out


def moved_bytes(path, tkv, elem):
    """HBM bytes of one layer's K and V traffic, from the shapes alone."""
    row = KVH * D
    if path == "paged":
        return 2 * tkv * row * elem
    if path == "floor":
        return 2 * tkv * row * 2
    # gather: read the pool, write the bf16 copy, read it back, + the slots
    return 2 * tkv * row * (elem + 2 + 2) + tkv * 4


def shape_rows(nseq, lq, lk, args, gen):
    dev = "cuda"
    pages_per = lk // PAGE
    total = nseq * pages_per + 1
    pool = {"bf16": tuple(torch.randn(total, KVH, PAGE, D, device=dev,
                                      generator=gen).to(BF16)
                          for _ in range(2))}
    pool["fp8"] = tuple(ops.reference.quantize_e4m3(c, 0) for c in pool["bf16"])
    q = torch.randn(nseq * lq, QH, D, device=dev, generator=gen).to(BF16)
    perm = torch.randperm(total - 1, device=dev, generator=gen) + 1
    bt = perm[:nseq * pages_per].view(nseq, pages_per).to(torch.int32)
    cu = [i * lq for i in range(nseq + 1)]
    cuk = [i * lk for i in range(nseq + 1)]
    cu_d = torch.tensor(cu, dtype=torch.int32, device=dev)
    cuk_d = torch.tensor(cuk, dtype=torch.int32, device=dev)
    slots = ops.reference.paged_kv_slots(bt, [lk] * nseq, PAGE)
    block_map = ops.prefill_paged_block_map(cu, cuk, pages_per, dev)
    rows = []
    for name, elem in (("bf16", 2), ("fp8", 1)):
        kc, vc = pool[name]

        def gather():
            if name == "fp8":
                return (ops.kv_gather_dequant(kc, slots, 0),
                        ops.kv_gather_dequant(vc, slots, 0))
            sl = slots.long()            # as LlamaAttention.forward does
            pages, offs = sl // PAGE, sl % PAGE
            return kc[pages, :, offs], vc[pages, :, offs]

        k_rows, v_rows = gather()
        fns = {
            "gather": lambda: ops.prefill_attention(q, *gather(), cu_d, SCALE,
                                                    cuk_d),
            "paged": lambda: ops.prefill_attention_paged(
                q, kc, vc, bt, cu_d, SCALE, cuk_d, block_map=block_map),
            "floor": lambda: ops.prefill_attention(q, k_rows, v_rows, cu_d,
                                                   SCALE, cuk_d),
        }
        same = torch.equal(fns["paged"](), fns["gather"]())
        times = alternate(fns, args.warmup, args.iters)
        for path, t in times.items():
            med = statistics.median(t)
            nbytes = moved_bytes(path, nseq * lk, elem)
            rows.append(dict(
                dtype=name, seqs=nseq, lq=lq, lk=lk, path=path,
                median_us=round(med, 1), min_us=round(min(t), 1),
                kv_bytes=nbytes, paged_equals_gather=same))
            print(json.dumps(rows[-1]), flush=True)
    return rows


def engine_rows(args):
    """Submit to first token of one 8192-token prompt on Llama-3-8B chunked
    at max_prefill_tokens = 2048 (prefix cache off, so every run prefills
    everything): one engine per (dtype, prefill_kv_read), gather and paged
    alternated --engine-rounds times after one warm-up run each."""
    import time
    from rbg_amd.engine.config import EngineConfig, ModelConfig
    from rbg_amd.engine.engine import LLMEngine
    from rbg_amd.engine.sequence import SamplingParams
    model = ModelConfig.preset("llama-3-8b")
    prompt = torch.randint(0, model.vocab_size, (8192,),
                           generator=torch.Generator().manual_seed(3)).tolist()
    rows = []
    for name in ("bf16", "fp8"):
        kw = {} if name == "bf16" else dict(kv_cache_dtype="fp8_e4m3")
        engines = {read: LLMEngine(EngineConfig(
            model=model, device="cuda", max_seq_len=8192 + 16,
            kv_pool_tokens=16384, max_prefill_tokens=2048,
            enable_prefix_cache=False, enforce_eager=True,
            prefill_kv_read=read, **kw)) for read in ("gather", "paged")}
        times = {read: [] for read in engines}
        tokens = {}
        for rnd in range(1 + args.engine_rounds):
            for read, eng in engines.items():
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                (seq,) = eng.generate([prompt], SamplingParams(max_new_tokens=1))
                torch.cuda.synchronize()
                if rnd:
                    times[read].append(round((time.perf_counter() - t0) * 1e3,
                                             2))
                tokens[read] = seq.output_tokens
        for read in engines:
            rows.append(dict(kind="engine_ttft", dtype=name, path=read,
                             prompt=8192, max_prefill_tokens=2048,
                             ttft_ms=times[read],
                             same_token=tokens[read] == tokens["gather"]))
            print(json.dumps(rows[-1]), flush=True)
        del engines
        torch.cuda.empty_cache()
    return rows


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--engine", action="store_true",
                    help="also time submit-to-first-token through LLMEngine")
    ap.add_argument("--engine-rounds", type=int, default=3)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    assert ops.HAVE_HIP, ops._hip_err
    gen = torch.Generator(device="cuda").manual_seed(0)
    results = []
    for nseq, lq, lk in SHAPES:
        results += shape_rows(nseq, lq, lk, args, gen)
    if args.engine:
        results += engine_rows(args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
