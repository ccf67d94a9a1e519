#!/usr/bin/env python3
"""Within-probe A/B: skinny_gemm (32- and 64-column panels) vs hipBLASLt on
the decode projection shapes, and GEMM + split-K fold + add + RMSNorm fused
against unfused.

Cold by default: every call of a candidate reads the next of enough distinct
weight tensors that their total is at least twice the 256 MiB Infinity Cache,
so each weight streams from HBM as it does in a real decode step (16 GB of
weights per step).  `--warm` keeps the older behaviour, one weight tensor
timed over and over (a 33 MB weight then sits in the Infinity Cache), so that
profiles/sg_micro7_b*.json stay comparable.
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch

from rbg_amd import ops

L3_BYTES = 256 << 20


def timeit(fn, n_weights, iters=40, warmup=10):
    """ms per call of fn(i), i cycling over the weight tensors."""
    for i in range(warmup):
        fn(i % n_weights)
    torch.cuda.synchronize()
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    s.record()
    for i in range(iters):
        fn(i % n_weights)
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", default="128",
                    help="decode batch sizes, comma separated")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--shapes", default="qkv,o,gate_up,down")
    ap.add_argument("--splits", default="0",
                    help="force_splits values to time, comma separated "
                         "(0 = the launcher's choice)")
    ap.add_argument("--warm", action="store_true",
                    help="one weight tensor per shape, re-read every call")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    H, I, QH, KVH, D = 4096, 14336, 32, 8, 128
    shapes = {"qkv": (H, (QH + 2 * KVH) * D), "o": (QH * D, H),
              "gate_up": (H, 2 * I), "down": (I, H)}
    shapes = {n: shapes[n] for n in args.shapes.split(",")}
    splits = [int(s) for s in args.splits.split(",")]
    hip = ops._hip
    out = {"mode": "warm" if args.warm else "cold"}
    for M in (int(b) for b in args.batch.split(",")):
        best = {}
        for name, (k, n) in shapes.items():
            n_w = 1 if args.warm else -(-2 * L3_BYTES // (k * n * 2))
            ws = [torch.randn(n, k, dtype=torch.bfloat16, device=dev)
                  for _ in range(n_w)]
            x = torch.randn(M, k, dtype=torch.bfloat16, device=dev)
            cands = [("lib", lambda i: torch.nn.functional.linear(x, ws[i]))]
            for s in splits:
                if k % (max(s, 1) * 256):
                    continue
                for panel in (32, 64):
                    if panel == 64 and (M > 128 or n % 64):
                        continue
                    cands.append((
                        "s%s_p%d" % (s or "auto", panel),
                        lambda i, s=s, panel=panel: hip.skinny_gemm(
                            x, ws[i], s, panel)))
            if n == H:
                # o / down: the projection with the add + norm behind it
                res = torch.randn(M, n, dtype=torch.bfloat16, device=dev)
                nw = torch.ones(n, dtype=torch.bfloat16, device=dev)

                def unfused(i):
                    h = hip.skinny_gemm(x, ws[i])
                    hip.fused_add_rmsnorm(h, res, nw, 1e-5)

                cands.append(("norm_unfused", unfused))
                cands.append(("norm_fused",
                              lambda i: hip.skinny_gemm_add_rmsnorm(
                                  x, ws[i], res, nw, 1e-5)))
            for _ in range(args.rounds):
                for impl, fn in cands:
                    ms = timeit(fn, n_w)
                    key = f"{name}/{impl}"
                    best[key] = min(best.get(key, 1e9), ms)
            del ws
        row = {}
        for key, ms in sorted(best.items()):
            k, n = shapes[key.split("/")[0]]
            row[key + "_us"] = round(ms * 1e3, 2)
            row[key + "_GBps"] = round(
                (k * n * 2 + M * (k + n) * 2) / ms / 1e6, 1)
        out["batch%d" % M] = row
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
