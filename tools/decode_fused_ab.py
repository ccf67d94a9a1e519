#!/usr/bin/env python3
"""In-process interleaved A/B of the decode-attention launch sequence.

Arms (each timed with events over `--iters` calls, `--rounds` rounds, the arms
taking turns inside every round):

  c1, c1_again  splits merged by decode_combine_kernel (attention + combine
                timed together); the pair is the A/A noise floor
  c2            splits merged inside the workgroup (2 or 4 splits only)

for bf16 variant 4 at every shape and for the fp8 kernel at the 2- and 4-split
shapes.

Shapes are Llama-3-8B's (32 q heads, 8 kv heads, 128 dims, 16-token pages).
Where one cache pair is under 512 MiB the calls rotate over enough distinct
pairs that 512 MiB pass between two reads of the same bytes, so K/V streams
from HBM as it does in a real step (34 GB of K/V per step against a 256 MiB
Infinity Cache).

"wins" in the summary means: faster than the other arm by more than twice the
A/A spread of the same shape.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from rbg_amd import ops

KVH, D, PAGE, QH = 8, 128, 16, 32
SCALE = 0.088
COLD_BYTES = 512 << 20
# (batch, ctx, splits): the bench shape, the 4-split shapes, one split, and
# 16 splits as the control (no in-workgroup kernel there)
SHAPES = ((128, 2048, 2), (64, 2048, 4), (64, 4096, 4), (256, 2048, 1),
          (8, 8192, 16))


def make_caches(batch, ctx, dev, fp8=False):
    """Enough distinct (key, value, block table) sets for a cold stream."""
    pages = batch * ((ctx + PAGE - 1) // PAGE) + 1
    kv_bytes = 2 * batch * ctx * KVH * D * (1 if fp8 else 2)
    n = max(1, -(-COLD_BYTES // kv_bytes))
    sets = []
    for _ in range(n):
        if fp8:     # finite e4m3 codes
            kc = torch.randint(0, 120, (pages, KVH, PAGE, D), device=dev,
                               dtype=torch.uint8).view(torch.float8_e4m3fn)
            vc = kc.clone()
        else:
            kc = torch.randn(pages, KVH, PAGE, D, dtype=torch.bfloat16,
                             device=dev)
            vc = torch.randn_like(kc)
        bt = torch.arange(1, pages, dtype=torch.int32,
                          device=dev).view(batch, -1)
        sets.append((kc, vc, bt))
    return sets, kv_bytes


def interleaved(arms, n_sets, rounds, iters, warmup=3):
    """arms: name -> fn(i), i cycling over the cache sets.  Returns
    name -> list of us per call, one entry per round."""
    for fn in arms.values():
        for i in range(warmup):
            fn(i % n_sets)
    torch.cuda.synchronize()
    times = {name: [] for name in arms}
    for _ in range(rounds):
        for name, fn in arms.items():
            s = torch.cuda.Event(enable_timing=True)
            e = torch.cuda.Event(enable_timing=True)
            s.record()
            for i in range(iters):
                fn(i % n_sets)
            e.record()
            torch.cuda.synchronize()
            times[name].append(s.elapsed_time(e) / iters * 1e3)
    return times


def summarise(times):
    return {name: {"median_us": round(statistics.median(t), 2),
                   "min_us": round(min(t), 2)} for name, t in times.items()}


def verdict(row, a, b, aa):
    """Which of arms a, b wins by more than twice the A/A spread."""
    spread = abs(row[aa[0]]["median_us"] - row[aa[1]]["median_us"])
    diff = row[a]["median_us"] - row[b]["median_us"]
    win = b if diff > 2 * spread else a if -diff > 2 * spread else "tie"
    return {"aa_spread_us": round(spread, 2), "diff_us": round(diff, 2),
            "wins": win}


def decode_arms(batch, ctx, splits, dev, fp8=False):
    sets, kv_bytes = make_caches(batch, ctx, dev, fp8)
    ctx_t = torch.full((batch,), ctx, dtype=torch.int32, device=dev)
    q = torch.randn(batch, QH, D, dtype=torch.bfloat16, device=dev)

    def attn(combine):
        def fn(i):
            kc, vc, bt = sets[i]
            if fp8:
                return ops._hip.decode_attention_fp8(
                    q, kc, vc, bt, ctx_t, SCALE, splits, 0, 0, combine)
            return ops._hip.decode_attention(q, kc, vc, bt, ctx_t, SCALE,
                                             splits, 4, combine)
        return fn

    arms = {"c1": attn(1), "c1_again": attn(1)}
    if splits in (2, 4):
        arms["c2"] = attn(2)
    return arms, len(sets), kv_bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    out = {}
    for fp8 in (False, True):
        for batch, ctx, splits in SHAPES:
            if fp8 and splits not in (2, 4):
                continue
            arms, n_sets, kv_bytes = decode_arms(batch, ctx, splits, dev, fp8)
            row = summarise(interleaved(arms, n_sets, args.rounds,
                                        args.iters))
            row["cache_sets"] = n_sets
            row["kv_GB"] = round(kv_bytes / 1e9, 3)
            if "c2" in row:
                row["c1_vs_c2"] = verdict(row, "c1", "c2", ("c1", "c1_again"))
            out["%sB%d_ctx%d_s%d" % ("fp8_" if fp8 else "", batch, ctx,
                                     splits)] = row
            del arms
            torch.cuda.empty_cache()
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
