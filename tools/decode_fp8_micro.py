#!/usr/bin/env python
"""Micro-benchmark of the FP8 (e4m3) KV cache against bf16 on the same tree,
in one process (docs/FEATURES.md "FP8 KV cache").

  decode   ops.decode_attention, bf16 variant 4 against fp8, at B x ctx =
           128 x 2048 (the bench's shape), 64 x 4096 and 8 x 8192, 32 q heads
           / 8 KV heads, splits from pick_decode_splits.  Effective bytes/s =
           the K and V bytes of the live context (2 * B * ctx * KVH * 128 *
           element size) over the time.
  store    ops.rope_store_kv in both dtypes at T = 128 and 8192.
  step     one full engine decode step at B = 128, ctx 2048 through LLMEngine
           in graph mode, bf16 against fp8 (--no-engine skips it).

Every timing alternates the two dtypes: per round one event-timed launch of
each, median and min over --iters rounds after --warmup rounds.

    python tools/decode_fp8_micro.py --out profiles/decode_fp8_micro.json
"""
import argparse
import json
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from rbg_amd import ops  # noqa: E402

QH, KVH, D, PAGE = 32, 8, 128, 16
SCALE = 1.0 / 128 ** 0.5
FP8 = torch.float8_e4m3fn
DECODE_SHAPES = ((128, 2048), (64, 4096), (8, 8192))
STORE_TOKENS = (128, 8192)


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


def summary(times):
    return {"median_us": round(statistics.median(times), 1),
            "min_us": round(min(times), 1)}


def decode_rows(args):
    gen = torch.Generator(device="cuda").manual_seed(0)
    rows = []
    for B, ctx in DECODE_SHAPES:
        pages_per = ctx // PAGE
        total = B * pages_per + 1
        kc = torch.randn(total, KVH, PAGE, D, device="cuda", generator=gen,
                         dtype=torch.float32).to(torch.bfloat16)
        vc = torch.randn(total, KVH, PAGE, D, device="cuda", generator=gen,
                         dtype=torch.float32).to(torch.bfloat16)
        k8 = ops.reference.quantize_e4m3(kc, 0)
        v8 = ops.reference.quantize_e4m3(vc, 0)
        q = torch.randn(B, QH, D, device="cuda", generator=gen,
                        dtype=torch.float32).to(torch.bfloat16)
        perm = torch.randperm(total - 1, device="cuda", generator=gen) + 1
        bt = perm[:B * pages_per].view(B, pages_per).to(torch.int32)
        cl = torch.full((B,), ctx, dtype=torch.int32, device="cuda")
        splits = ops.pick_decode_splits(B, KVH, ctx, 4)
        fns = {
            "bf16": lambda: ops.decode_attention(
                q, kc, vc, bt, cl, SCALE, num_splits=splits, variant=4),
            "fp8": lambda: ops.decode_attention(
                q, k8, v8, bt, cl, SCALE, num_splits=splits),
        }
        # same inputs up to quantisation: the outputs must be close
        ref = ops.decode_attention(q, k8.to(torch.bfloat16),
                                   v8.to(torch.bfloat16), bt, cl, SCALE,
                                   num_splits=splits, variant=4)
        same = torch.equal(ref, fns["fp8"]())
        times = alternate(fns, args.warmup, args.iters)
        for name, elem in (("bf16", 2), ("fp8", 1)):
            nbytes = 2 * B * ctx * KVH * D * elem
            s = summary(times[name])
            rows.append(dict(
                kind="decode", dtype=name, batch=B, ctx=ctx, splits=splits,
                kv_bytes=nbytes,
                eff_tb_per_s=round(nbytes / s["median_us"] / 1e6, 3),
                equals_bf16_on_dequantised=same, **s))
            print(json.dumps(rows[-1]), flush=True)
        del kc, vc, k8, v8
    return rows


def store_rows(args):
    gen = torch.Generator(device="cuda").manual_seed(1)
    rows = []
    for T in STORE_TOKENS:
        pages = T // PAGE + 1
        qkv = torch.randn(T, (QH + 2 * KVH) * D, device="cuda", generator=gen,
                          dtype=torch.float32).to(torch.bfloat16)
        q, k, v = (qkv[:, :QH * D], qkv[:, QH * D:(QH + KVH) * D],
                   qkv[:, (QH + KVH) * D:])
        cs = ops.build_cos_sin_table(D, T, device="cuda")
        pos = torch.arange(T, dtype=torch.int32, device="cuda")
        slots = (torch.randperm(T, device="cuda", generator=gen) + PAGE
                 ).to(torch.int32)
        kb = torch.zeros(pages, KVH, PAGE, D, dtype=torch.bfloat16,
                         device="cuda")
        vb = torch.zeros_like(kb)
        k8 = torch.zeros(pages, KVH, PAGE, D, dtype=torch.uint8,
                         device="cuda").view(FP8)
        v8 = torch.zeros_like(k8.view(torch.uint8)).view(FP8)
        fns = {
            "bf16": lambda: ops.rope_store_kv(q, k, v, kb, vb, cs, pos, slots),
            "fp8": lambda: ops.rope_store_kv(q, k, v, k8, v8, cs, pos, slots),
        }
        times = alternate(fns, args.warmup, args.iters)
        for name in fns:
            rows.append(dict(kind="rope_store_kv", dtype=name, tokens=T,
                             **summary(times[name])))
            print(json.dumps(rows[-1]), flush=True)
    return rows


def engine_rows(args):
    """Wall time of LLMEngine.step() in steady decode at B = 128, contexts
    around 2048, graph mode: one engine per dtype, alternated per round of
    --engine-steps steps."""
    from rbg_amd.engine.config import EngineConfig, ModelConfig
    from rbg_amd.engine.engine import LLMEngine
    from rbg_amd.engine.sequence import SamplingParams
    B, ctx, new = 128, 2048, 4 + args.engine_rounds * args.engine_steps + 8
    engines = {}
    for name in ("bf16", "fp8"):
        kw = {} if name == "bf16" else dict(kv_cache_dtype="fp8_e4m3")
        cfg = EngineConfig(model=ModelConfig.preset("llama-3-8b"),
                           device="cuda", max_batch_size=B,
                           max_seq_len=ctx + new + 16,
                           kv_pool_tokens=B * (ctx + new + 32),
                           enable_prefix_cache=False, **kw)
        eng = LLMEngine(cfg)
        gen = torch.Generator().manual_seed(2)
        for _ in range(B):
            eng.add_request(
                torch.randint(0, cfg.model.vocab_size, (ctx - 64,),
                              generator=gen).tolist(),
                SamplingParams(max_new_tokens=new))
        while eng.step() != "decode":      # prefill everything, then warm up
            pass
        for _ in range(3):
            assert eng.step() == "decode"
        engines[name] = eng
    times = {name: [] for name in engines}
    for _ in range(args.engine_rounds):
        for name, eng in engines.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.engine_steps):
                eng.step()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e6 /
                               args.engine_steps)
    rows = []
    for name, eng in engines.items():
        rows.append(dict(kind="engine_decode_step", dtype=name, batch=B,
                         ctx=ctx, kv_pages=eng.runner.cache.num_pages,
                         pool_gb=round(eng.runner.cache.kv.numel() *
                                       eng.runner.cache.kv.element_size()
                                       / 1e9, 2),
                         **summary(times[name])))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--engine-rounds", type=int, default=5)
    ap.add_argument("--engine-steps", type=int, default=20)
    ap.add_argument("--no-engine", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    assert ops.HAVE_HIP, ops._hip_err
    results = decode_rows(args) + store_rows(args)
    if not args.no_engine:
        results += engine_rows(args)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
