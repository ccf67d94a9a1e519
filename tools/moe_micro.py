#!/usr/bin/env python3
"""Within-probe A/B of ops.moe_ffn (hip/moe.hip) against a per-expert
F.linear loop on the same tensors, on one Qwen3-30B-A3B layer's experts
(E = 128, top-8, H = 2048, I = 768) at T in {1, 16, 128, 2048}.

The loop is the baseline: what a model has without the kernels.  It is given
every advantage a host-driven loop can have: the routing is already on the
host, so it visits only the experts that have rows, with its index tensors
built outside the timed region.

Cold: every call reads the next of `--layers` distinct expert sets with
routings of their own, enough that the experts touched by consecutive calls
total at least twice the 256 MiB Infinity Cache, so weights stream from HBM as
they do in a decode step.  Each call is timed with its own pair of device
events; the figure is the median after warm-up, the two candidates alternating
round by round.  TB/s counts the weight bytes of the experts actually touched.
"""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import torch
import torch.nn.functional as F

from rbg_amd import ops

L3_BYTES = 256 << 20


def time_calls(fn, n_layers, rounds, warmup=2):
    """us of every timed call of fn(i), i cycling over the layers."""
    times = []
    for r in range(warmup + rounds):
        for i in range(n_layers):
            s = torch.cuda.Event(enable_timing=True)
            e = torch.cuda.Event(enable_timing=True)
            s.record()
            fn(i)
            e.record()
            torch.cuda.synchronize()
            if r >= warmup:
                times.append(s.elapsed_time(e) * 1e3)
    return times


def quantised_main(args, dev, shape):
    """--w8: ops.moe_ffn with bf16 against e4m3 experts (the quantisation of
    the same weights), the two alternating call by call over the cold layer
    sets; --w4: MXFP4 experts as a third format in the same alternation.
    TB/s counts each format's own weight bytes of the experts touched
    (exponents included)."""
    E, K, H, I = shape
    names = ("bf16", "e4m3", "mxfp4") if args.w4 else ("bf16", "e4m3")
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g)
    sets = []
    for _ in range(args.layers):
        w1 = (rnd(E, 2 * I, H) * 0.02).bfloat16()
        w2 = (rnd(E, H, I) * 0.02).bfloat16()
        q = [ops.quantize_weight_e4m3(w.view(-1, w.shape[2])) for w in (w1, w2)]
        sets.append({"bf16": (w1, w2, None, None),
                     "e4m3": (q[0][0].view(w1.shape), q[1][0].view(w2.shape),
                              q[0][1].view(E, 2 * I), q[1][1].view(E, H))})
        if args.w4:
            q = [ops.quantize_weight_mxfp4(w.view(-1, w.shape[2]))
                 for w in (w1, w2)]
            sets[-1]["mxfp4"] = (q[0][0].view(E, 2 * I, -1),
                                 q[1][0].view(E, H, -1),
                                 q[0][1].view(E, 2 * I, -1),
                                 q[1][1].view(E, H, -1))
    per_expert = {"bf16": 3 * I * H * 2, "e4m3": 3 * I * H + 2 * I + H,
                  "mxfp4": 3 * I * H // 2 + 3 * I * H // 32}
    out = {"shape": {"E": E, "k": K, "H": H, "I": I}, "layers": args.layers}
    for T in (int(t) for t in args.tokens.split(",")):
        x = (rnd(T, H) * 0.5).bfloat16()
        routed = [ops.moe_route(rnd(T, E).bfloat16(), K, True)
                  for _ in range(args.layers)]
        touched = [ids.unique().numel() for ids, _ in routed]

        def call(name, i):
            w1, w2, e1, e2 = sets[i][name]
            if e1 is None:
                return ops.moe_ffn(x, w1, w2, *routed[i])
            return ops.moe_ffn(x, w1, w2, *routed[i], e1, e2)

        times = {name: [] for name in names}
        for r in range(2 + args.rounds):
            for i in range(args.layers):
                for name in times:
                    s = torch.cuda.Event(enable_timing=True)
                    e = torch.cuda.Event(enable_timing=True)
                    s.record()
                    call(name, i)
                    e.record()
                    torch.cuda.synchronize()
                    if r >= 2:
                        times[name].append(s.elapsed_time(e) * 1e3)
        row = {"experts_touched": touched[0],
               "cold": sum(touched) * per_expert[names[-1]] >= 2 * L3_BYTES}
        for name, ts in times.items():
            med = statistics.median(ts)
            row[name + "_us"] = round(med, 1)
            row[name + "_us_min_max"] = [round(min(ts), 1), round(max(ts), 1)]
            row[name + "_weight_TBps"] = round(
                sum(touched) / len(touched) * per_expert[name] / med / 1e6, 2)
        for name in names[1:]:
            row[name + "_over_bf16"] = round(row[name + "_us"] /
                                             row["bf16_us"], 3)
        if args.w4:
            row["mxfp4_over_e4m3"] = round(row["mxfp4_us"] / row["e4m3_us"], 3)
        out["T%d" % T] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tokens", default="1,16,128,2048")
    ap.add_argument("--layers", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON here")
    ap.add_argument("--w8", action="store_true",
                    help="bf16 against e4m3 experts instead of hip against "
                         "the loop")
    ap.add_argument("--w4", action="store_true",
                    help="bf16, e4m3 and MXFP4 experts, alternating")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    E, K, H, I = 128, 8, 2048, 768
    if args.w8 or args.w4:
        text = json.dumps(quantised_main(args, dev, (E, K, H, I)), indent=1)
        print(text, flush=True)
        if args.out:
            with open(args.out, "w") as f:
                f.write(text + "\n")
        return
    g = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, device=dev, generator=g)
    w1 = [(rnd(E, 2 * I, H) * 0.02).bfloat16() for _ in range(args.layers)]
    w2 = [(rnd(E, H, I) * 0.02).bfloat16() for _ in range(args.layers)]
    out = {"shape": {"E": E, "k": K, "H": H, "I": I}, "layers": args.layers}
    for T in (int(t) for t in args.tokens.split(",")):
        x = (rnd(T, H) * 0.5).bfloat16()
        routed = [ops.moe_route(rnd(T, E).bfloat16(), K, True)
                  for _ in range(args.layers)]
        plans, touched = [], []
        for ids, w in routed:
            plan = []
            for e in ids.unique().tolist():
                t_idx, j_idx = (ids == e).nonzero(as_tuple=True)
                plan.append((e, t_idx, w[t_idx, j_idx, None]))
            plans.append(plan)
            touched.append(len(plan) * 3 * I * H * 2)

        def hip(i):
            return ops.moe_ffn(x, w1[i], w2[i], *routed[i])

        def loop(i):
            y = torch.zeros(T, H, dtype=torch.float32, device=dev)
            for e, t_idx, we in plans[i]:
                h = ops.silu_mul(F.linear(x[t_idx], w1[i][e]))
                y.index_add_(0, t_idx, F.linear(h, w2[i][e]).float() * we)
            return y.bfloat16()

        err = (hip(0).float() - loop(0).float()).norm() / loop(0).float().norm()
        times = {"hip": [], "loop": []}
        for _ in range(args.rounds):
            for name, fn in (("hip", hip), ("loop", loop)):
                times[name] += time_calls(fn, args.layers, 1)
        row = {"experts_touched": len(plans[0]),
               "touched_MB_per_call": round(sum(touched) / len(touched) / 1e6,
                                            1),
               "cold": sum(touched) >= 2 * L3_BYTES,
               "hip_vs_loop_rel_l2": float(err)}
        for name, ts in times.items():
            med = statistics.median(ts)
            row[name + "_us"] = round(med, 1)
            row[name + "_us_min_max"] = [round(min(ts), 1), round(max(ts), 1)]
            row[name + "_weight_TBps"] = round(
                sum(touched) / len(touched) / med / 1e6, 2)
        out["T%d" % T] = row
    text = json.dumps(out, indent=1)
    print(text, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
