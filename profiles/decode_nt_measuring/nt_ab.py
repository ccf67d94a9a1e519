#!/usr/bin/env python3
"""nt-load A/B (measuring build only: needs the kv_nt / w_nt binding flags)."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch
from rbg_amd import ops
import decode_fused_ab as ab

dev = torch.device("cuda:0")
out = {"kv": {}, "kv_fp8": {}, "w": {}}
for batch, ctx, splits in ab.SHAPES:
    sets, kv_bytes = ab.make_caches(batch, ctx, dev)
    ctx_t = torch.full((batch,), ctx, dtype=torch.int32, device=dev)
    q = torch.randn(batch, ab.QH, ab.D, dtype=torch.bfloat16, device=dev)
    def attn(nt):
        def fn(i):
            kc, vc, bt = sets[i]
            return ops._hip.decode_attention(q, kc, vc, bt, ctx_t, ab.SCALE, splits, 4, 0, nt)
        return fn
    arms = {"plain": attn(0), "plain_again": attn(0), "nt": attn(1)}
    row = ab.summarise(ab.interleaved(arms, len(sets), 7, 20))
    row["verdict"] = ab.verdict(row, "plain", "nt", ("plain", "plain_again"))
    out["kv"]["B%d_ctx%d_s%d" % (batch, ctx, splits)] = row
    print(batch, ctx, splits, json.dumps(row), flush=True)
    del sets, arms
    torch.cuda.empty_cache()

# fp8 at the bench shape and one 4-split shape
for batch, ctx, splits in ((128, 2048, 2), (64, 4096, 4), (256, 2048, 1)):
    pages = batch * (ctx // 16) + 1
    kv_bytes = 2 * batch * ctx * 8 * 128
    n = max(1, -(-ab.COLD_BYTES // kv_bytes))
    sets = []
    for _ in range(n):
        kc = torch.randint(0, 120, (pages, 8, 16, 128), dtype=torch.uint8, device=dev).view(torch.float8_e4m3fn)
        vc = torch.randint(0, 120, (pages, 8, 16, 128), dtype=torch.uint8, device=dev).view(torch.float8_e4m3fn)
        bt = torch.arange(1, pages, dtype=torch.int32, device=dev).view(batch, -1)
        sets.append((kc, vc, bt))
    ctx_t = torch.full((batch,), ctx, dtype=torch.int32, device=dev)
    q = torch.randn(batch, ab.QH, ab.D, dtype=torch.bfloat16, device=dev)
    def attn8(nt):
        def fn(i):
            kc, vc, bt = sets[i]
            return ops._hip.decode_attention_fp8(q, kc, vc, bt, ctx_t, ab.SCALE, splits, 0, 0, 0, nt)
        return fn
    arms = {"plain": attn8(0), "plain_again": attn8(0), "nt": attn8(1)}
    row = ab.summarise(ab.interleaved(arms, len(sets), 7, 20))
    row["verdict"] = ab.verdict(row, "plain", "nt", ("plain", "plain_again"))
    out["kv_fp8"]["B%d_ctx%d_s%d" % (batch, ctx, splits)] = row
    print("fp8", batch, ctx, splits, json.dumps(row), flush=True)
    del sets, arms
    torch.cuda.empty_cache()

# W loads of the 64-column skinny GEMM, cold weights (as skinny_gemm_micro.py)
H, I = 4096, 14336
for name, (k, n) in {"o": (4096, H), "down": (I, H)}.items():
    n_w = -(-2 * (256 << 20) // (k * n * 2))
    ws = [torch.randn(n, k, dtype=torch.bfloat16, device=dev) for _ in range(n_w)]
    for M in (16, 64, 128):
        x = torch.randn(M, k, dtype=torch.bfloat16, device=dev)
        def gemm(nt):
            return lambda i: ops._hip.skinny_gemm(x, ws[i], 0, 64, nt)
        arms = {"plain": gemm(0), "plain_again": gemm(0), "nt": gemm(1)}
        row = ab.summarise(ab.interleaved(arms, n_w, 7, 40, warmup=n_w))
        row["verdict"] = ab.verdict(row, "plain", "nt", ("plain", "plain_again"))
        out["w"]["%s_M%d" % (name, M)] = row
        print(name, M, json.dumps(row), flush=True)
    del ws
    torch.cuda.empty_cache()
os.makedirs(os.path.join(ROOT, "out"), exist_ok=True)
with open(os.path.join(ROOT, "out", "nt_ab.json"), "w") as f:
    json.dump(out, f, indent=1)
