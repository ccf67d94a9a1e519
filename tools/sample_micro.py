#!/usr/bin/env python
"""Micro-benchmark of ModelRunner.sample_device alone (no model forward).

Shapes n in {1, 32, 128} x V = 128 256 fp32 logits, two parameter sets:
  (a) temperature only        (b) top_k = 50 with top_p = 0.9
(a) also runs on a tree from before the fused sampler, where it measures the
softmax + multinomial path; (b) needs SamplingParams.top_k and is skipped
there.  Each timing is the wall time of one sample_device call including the
host copy of the tokens it returns (that copy is part of the call in the
serving loop), median and min over --iters calls after --warmup calls.  The
logits are one resident buffer, as in serving where the LM-head GEMM has just
written them.

    python tools/sample_micro.py --out profiles/sample_micro.json
"""
import argparse
import dataclasses
import json
import os
import statistics
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch  # noqa: E402

from rbg_amd.engine.model_runner import ModelRunner  # noqa: E402
from rbg_amd.engine.sequence import SamplingParams, Sequence  # noqa: E402

V = 128256
SETS = {
    "a_temperature": dict(temperature=1.0),
    "b_topk50_topp0.9": dict(temperature=1.0, top_k=50, top_p=0.9),
}


def kernel_time_us(logits, seqs, iters: int = 50) -> float:
    """GPU time of ops.sample alone (parameters already on the device):
    events around `iters` back-to-back launches."""
    from rbg_amd import ops
    n = len(seqs)
    sp = [s.sampling for s in seqs]
    f32 = dict(dtype=torch.float32, device="cuda")
    i32 = dict(dtype=torch.int32, device="cuda")
    args = (logits, torch.tensor([s.temperature for s in sp], **f32),
            torch.tensor([s.top_k for s in sp], **i32),
            torch.tensor([s.top_p for s in sp], **f32),
            torch.tensor([s.min_p for s in sp], **f32),
            torch.tensor([s.seed for s in sp], dtype=torch.int64,
                         device="cuda"),
            torch.full((n,), 8, **i32))
    for _ in range(5):
        ops.sample(*args)
    start, stop = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    torch.cuda.synchronize()
    start.record()
    for _ in range(iters):
        ops.sample(*args)
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / iters


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    fields = {f.name for f in dataclasses.fields(SamplingParams)}
    fused = "top_k" in fields
    runner = types.SimpleNamespace()          # sample_device reads no state
    gen = torch.Generator(device="cuda").manual_seed(0)
    results = []
    for n in (1, 32, 128):
        logits = torch.randn(n, V, device="cuda", generator=gen) * 3
        for name, kw in SETS.items():
            if not set(kw) <= fields:
                continue
            if fused:
                kw = dict(kw, seed=1)
            seqs = [Sequence([1] * 8, SamplingParams(max_new_tokens=4, **kw))
                    for _ in range(n)]
            times = []
            for it in range(args.warmup + args.iters):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                ModelRunner.sample_device(runner, logits, seqs)
                dt = time.perf_counter() - t0
                if it >= args.warmup:
                    times.append(dt * 1e6)
            row = {"n": n, "V": V, "params": name,
                   "path": "fused" if fused else "softmax+multinomial",
                   "median_us": round(statistics.median(times), 1),
                   "min_us": round(min(times), 1)}
            if fused:
                row["kernel_us"] = round(kernel_time_us(logits, seqs), 1)
            print(json.dumps(row), flush=True)
            results.append(row)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
