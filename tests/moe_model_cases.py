"""Model-level checks of the mixture-of-experts model: the scenarios, pool,
recorder and checks of tests/model_cases.py with `conf-moe`
(test_moe_cpu.moe_config: 8 experts, top-2, I 192, H 512, qk_norm, 2 layers).

A plain fp64 forward cannot judge a MoE model: the engine routes on bf16
router logits, and where the k-th and (k+1)-th logit are closer than the
rounding error of the path that made them, a correct engine and an fp64
forward pick different experts.  So routing and values are judged apart.

  record     (eager runs) every `ops.moe_route` call: its bf16 logits and the
             ids it returned, per row, keyed (sequence, position, layer).
             The position comes from the ForwardBatch, the sequence from
             cu_seqlens and the seqs handed to runner.prefill / decode, the
             layer from the call's index within the step.  Every (sequence,
             position < num_tokens - 1, layer) is recorded exactly once;
             positions adopted from the prefix cache have no record.
  reference  model_cases' dense fp64 forward with the MoE block in fp64 and
             ROUTING FORCED: router logits l64 from its own hidden state,
             the engine's recorded ids, weights = fp64 softmax of l64 at
             those ids (renormalised if norm_topk_prob), the k experts in
             fp64.  An adopted position takes the record of the earlier
             sequence with the same token prefix.  The reference covers
             positions 0 .. num_tokens - 2: the last token was never fed to
             the engine, so it has no routing (model_cases runs the last
             position too; leaving it out can only lower e_cpu's maximum).
  yardstick  model_cases.cpu_forward on the CPU model with ops.moe_route
             returning the same forced ids and the reference path's own fp32
             softmax of its own bf16 logits l_cpu at those ids.  Forcing both
             sides keeps e_cpu from inflating on a near-tie row.

  C1 C2 C3   as in model_cases (factor 2, the same statistics).
  R0         every recorded ids row equals the stable descending top-k (NaN
             as -inf) of the recorded bf16 logits of that row.
  R1         for every recorded (row, layer) with chosen set S:
             max_{e not in S} l64_e - min_{e in S} l64_e <= 2 * FACTOR *
             delta, where delta = max |l_cpu - l64| over the scenario's (row,
             layer) pairs: two logits are compared, each allowed FACTOR
             times the yardstick's own error.
  cap        R1 cannot tell a right choice from a wrong one where the fp64
             gap between the k-th and (k+1)-th logit is itself <= 2 * FACTOR
             * delta.  The share of such pairs must be <= 1/4 (AMBIGUOUS_CAP)
             in every scenario, asserted from the reference alone.

Graph mode.  The ids live in buffers allocated inside the capture and cannot
be recorded.  A graph run is judged by C3 on its own pool and by torch.equal
with its eager twin on every logits row and every sequence's final K/V rows.
"""
from __future__ import annotations

import contextlib
import math
from typing import Dict, List, NamedTuple, Optional, Set, Tuple

import torch

import model_cases as mc
import test_moe_cpu as moe
from rbg_amd import ops
from rbg_amd.engine.model_runner import ModelRunner
from rbg_amd.models.llama import LlamaForCausalLM, MoEBlock

BF16 = torch.bfloat16
CONF = "conf-moe"
SCENARIOS = mc.SCENARIOS
FACTOR = mc.FACTOR
AMBIGUOUS_CAP = 0.25


def _model_config(conf: str):
    assert conf == CONF
    return moe.moe_config()


def moe_conf():
    """model_cases' helpers build their engines and CPU models from
    model_cases.model_config; inside this context it knows `conf-moe`
    (CONFS itself is left alone: eight test files parametrise over it)."""
    return mc._patched(mc, "model_config", _model_config)


# ---------------------------------------------------------------------------
# the routing record
# ---------------------------------------------------------------------------

Key = Tuple[int, int, int]                       # (seq_id, position, layer)


class RouteRecorder:
    """Wraps ops.moe_route (outermost: it sees what the model sees),
    LlamaForCausalLM.forward (positions, cu_seqlens) and ModelRunner.prefill
    / decode (the sequences of the step)."""

    def __init__(self):
        self.records: Dict[Key, List[Tuple[torch.Tensor, torch.Tensor]]] = {}
        self.calls: List[Tuple[str, int]] = []   # (mode, rows) per moe_route
        self._seqs = None
        self._step = None

    def __enter__(self):
        self._stack = contextlib.ExitStack()
        route, forward = ops.moe_route, LlamaForCausalLM.forward
        prefill, decode = ModelRunner.prefill, ModelRunner.decode
        rr = self

        def prefill_(runner, seqs):
            rr._seqs = list(seqs)
            return prefill(runner, seqs)

        def decode_(runner, seqs):
            rr._seqs = list(seqs)
            return decode(runner, seqs)

        def forward_(model, tokens, batch, kv, hidden=None):
            pos = batch.positions.tolist()
            if batch.mode == "prefill":
                cu = batch.cu_seqlens.tolist()
                row_seq = [b for b in range(len(cu) - 1)
                           for _ in range(cu[b + 1] - cu[b])]
            else:
                row_seq = list(range(len(pos)))
            assert len(row_seq) == len(pos)
            rr._step = [batch.mode, pos, row_seq, 0]
            return forward(model, tokens, batch, kv, hidden=hidden)

        def route_(logits, top_k, renormalize=True):
            ids, w = route(logits, top_k, renormalize)
            mode, pos, row_seq, layer = rr._step
            rr._step[3] += 1
            rr.calls.append((mode, int(logits.shape[0])))
            assert logits.shape[0] == len(pos) == ids.shape[0]
            lg, chosen = logits.detach().cpu().clone(), ids.detach().cpu().clone()
            for i, (p, b) in enumerate(zip(pos, row_seq)):
                key = (rr._seqs[b].seq_id, p, layer)
                rr.records.setdefault(key, []).append((lg[i], chosen[i]))
            return ids, w

        for obj, name, fn in ((ModelRunner, "prefill", prefill_),
                              (ModelRunner, "decode", decode_),
                              (LlamaForCausalLM, "forward", forward_),
                              (ops, "moe_route", route_)):
            self._stack.enter_context(mc._patched(obj, name, fn))
        return self

    def __exit__(self, *exc):
        return self._stack.__exit__(*exc)


class MoeTrace:
    """(name, rows) of every call that reaches ops.moe_route / ops.moe_ffn
    and, on a GPU, the extension's moe_group."""

    def __init__(self):
        self.calls: List[Tuple[str, int]] = []

    def __enter__(self):
        self._stack = contextlib.ExitStack()

        def noted(name, fn, arg=0):
            def wrapped(*a, **kw):
                self.calls.append((name, int(a[arg].shape[0])))
                return fn(*a, **kw)
            return wrapped

        for name in ("moe_route", "moe_ffn"):
            self._stack.enter_context(mc._patched(
                ops, name, noted(name, getattr(ops, name))))
        if ops._hip is not None:
            self._stack.enter_context(mc._patched(
                ops._hip, "moe_group", noted("moe_group", ops._hip.moe_group)))
        return self

    def __exit__(self, *exc):
        return self._stack.__exit__(*exc)

    def rows(self, name: str) -> Set[int]:
        return {n for m, n in self.calls if m == name}


# ---------------------------------------------------------------------------
# running
# ---------------------------------------------------------------------------

def run_scenario(scenario: str, device: str, eager: bool,
                 mutant=None) -> mc.Run:
    """model_cases.run_scenario with `conf-moe`, the MoE call trace and, in
    eager mode, the routing record.  mutant: engine -> context manager,
    patched in beneath the record for the engine's run only."""
    stack = contextlib.ExitStack()
    route = RouteRecorder() if (eager or device == "cpu") else None
    trace = MoeTrace()

    def after_build(engine):
        if mutant is not None:
            stack.enter_context(mutant(engine))
        stack.enter_context(trace)
        if route is not None:
            stack.enter_context(route)

    with moe_conf(), stack:
        run = mc.run_scenario(scenario, CONF, device, eager,
                              after_build=after_build)
    run.route, run.moe_trace = route, trace
    return run


def assert_paths(run: mc.Run) -> None:
    """model_cases.assert_paths, and: moe_route and moe_ffn were reached in
    both phases with the expected row counts, moe_group never, and the model
    has no dense MLP weights."""
    mc.assert_paths(run)
    runner, tr = run.engine.runner, run.moe_trace
    names = [n for n, _ in runner.model.named_parameters()]
    assert not any("w_gate_up" in n or "w_down" in n for n in names)
    assert sum(n.endswith("mlp.w_router") for n in names) == 2
    sizes = {len(b) for b in run.rec.decode_batches}
    # python reaches a captured step only to warm up and to capture it
    decode_rows = set(runner._graphs) if run.graph_mode else sizes
    assert not tr.rows("moe_group"), tr.rows("moe_group")
    for name in ("moe_route", "moe_ffn"):
        rows = tr.rows(name)
        assert decode_rows <= rows, (name, rows, decode_rows)
        assert rows - decode_rows, (name, rows)              # prefill too
        if run.scenario == "mixed":
            assert {158, 40} <= rows, (name, rows)
    layers = run.engine.cfg.model.num_layers
    assert [n for m, n in tr.calls if m == "moe_route"] == \
        [n for m, n in tr.calls if m == "moe_ffn"]
    assert len(tr.calls) % (2 * layers) == 0


# ---------------------------------------------------------------------------
# fp64 reference with forced routing, and the forced yardstick
# ---------------------------------------------------------------------------

def moe_forward64(model: LlamaForCausalLM, tokens: List[int],
                  forced: torch.Tensor):
    """model_cases.dense_forward64 for a model of MoE blocks.  forced: the
    ids to route by, long [T, layers, k].  Returns logits [T, vocab], kv [T,
    layers, 2, KVH, D] and the router logits l64 [T, layers, E]."""
    cfg = model.cfg
    T = len(tokens)
    D, H, KVH = cfg.head_dim, cfg.num_heads, cfg.num_kv_heads
    G = H // KVH
    half = D // 2
    eps = float(torch.tensor(cfg.rms_eps, dtype=torch.float32))  # as launched
    scale = 1.0 / math.sqrt(D)
    cs = model.cos_sin.detach().cpu().double()[:T]
    cos, sin = cs[:, None, :half], cs[:, None, half:]

    def w(p):
        return p.detach().cpu().double()

    def rms(x, weight):
        return x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + eps) * weight

    def rope(x):                                   # [T, heads, D]
        x1, x2 = x[..., :half], x[..., half:]
        return torch.cat([x1 * cos - x2 * sin, x2 * cos + x1 * sin], dim=-1)

    future = torch.arange(T).unsqueeze(0) > torch.arange(T).unsqueeze(1)
    r = w(model.embed)[torch.tensor(tokens, dtype=torch.long)]
    kvs, l64 = [], []
    for li, layer in enumerate(model.layers):
        a = layer.attn
        qkv = rms(r, w(layer.input_norm)) @ w(a.wqkv).T
        q = qkv[:, :H * D].reshape(T, H, D)
        k = qkv[:, H * D:(H + KVH) * D].reshape(T, KVH, D)
        v = qkv[:, (H + KVH) * D:].reshape(T, KVH, D)
        if a.q_norm is not None:
            q, k = rms(q, w(a.q_norm)), rms(k, w(a.k_norm))
        q, k = rope(q), rope(k)
        kvs.append(torch.stack([k, v], dim=1))     # [T, 2, KVH, D]
        sc = torch.einsum("qhgd,khd->hgqk", q.view(T, KVH, G, D), k) * scale
        p = torch.softmax(sc.masked_fill(future, float("-inf")), dim=-1)
        o = torch.einsum("hgqk,khd->qhgd", p, v).reshape(T, H * D)
        r = r + o @ w(a.wo).T
        block = layer.mlp
        assert isinstance(block, MoEBlock)
        x = rms(r, w(layer.post_norm))
        lg = x @ w(block.w_router).T
        l64.append(lg)
        ids = forced[:, li]
        wts = torch.softmax(lg, dim=-1).gather(1, ids)
        if block.renormalize:
            wts = wts / wts.sum(1, keepdim=True)
        w1, w2 = w(block.w1), w(block.w2)
        inter = w2.shape[2]
        y = torch.zeros_like(r)
        for e in ids.unique().tolist():
            t_idx, j_idx = (ids == e).nonzero(as_tuple=True)
            gu = x[t_idx] @ w1[e].T
            hh = torch.nn.functional.silu(gu[:, :inter]) * gu[:, inter:]
            y.index_add_(0, t_idx, wts[t_idx, j_idx, None] * (hh @ w2[e].T))
        r = r + y
    logits = rms(r, w(model.final_norm)) @ w(model.lm_head).T
    return logits, torch.stack(kvs, dim=1), torch.stack(l64, dim=1)


def cpu_forward_forced(model: LlamaForCausalLM, tokens: List[int],
                       forced: torch.Tensor):
    """model_cases.cpu_forward with ops.moe_route returning forced[:, layer]
    and ops.reference's own weights for them: the fp32 softmax of its own
    bf16 logits at those ids, renormalised in slot order.  Returns logits,
    kv and l_cpu [T, layers, E]."""
    seen: List[torch.Tensor] = []

    def route(logits, top_k, renormalize=True):
        ids = forced[:, len(seen)]
        assert ids.shape == (logits.shape[0], top_k)
        x = logits.float()
        seen.append(x)
        x = torch.where(torch.isnan(x), torch.full_like(x, float("-inf")), x)
        w = torch.softmax(x, dim=-1).gather(1, ids)
        if renormalize:
            total = w[:, 0].clone()
            for j in range(1, top_k):
                total = total + w[:, j]
            w = w / total.unsqueeze(1)
        return ids.to(torch.int32).contiguous(), w.contiguous()

    with mc._patched(ops, "moe_route", route):
        logits, kv = mc.cpu_forward(model, CONF, tokens)
    assert len(seen) == forced.shape[1]
    return logits, kv, torch.stack(seen, dim=1)


# ---------------------------------------------------------------------------
# checks
# ---------------------------------------------------------------------------

class MoeVerdict(NamedTuple):
    values: mc.Verdict                       # C1, C2, C3
    r0: List[str]                            # rows whose ids are not the top-k
    r1: List[Tuple[str, float]]              # (what, l64 margin) per record
    delta: float                             # max |l_cpu - l64|
    ambiguous: float                         # share of pairs R1 cannot judge
    pairs: int

    @property
    def r1_bound(self) -> float:
        return 2 * FACTOR * self.delta

    def failures(self) -> List[str]:
        out = self.values.failures() + ["R0 " + s for s in self.r0]
        out += ["R1 %s: margin %.4g > 2 * %g * delta %.4g" % (
            what, m, FACTOR, self.delta)
            for what, m in self.r1 if not m <= self.r1_bound]
        if not self.ambiguous <= AMBIGUOUS_CAP:
            out.append("cap: %.3f of the %d (row, layer) pairs have an fp64 "
                       "gap within 2 * FACTOR * delta = %.4g: change the "
                       "scenario's prompt seed" % (
                           self.ambiguous, self.pairs, self.r1_bound))
        return out

    def failed_checks(self) -> Set[str]:
        """Subset of {"C1", "C2K", "C2V", "C3", "R0", "R1"} (the cap is a
        condition on the scenario, not a check of the engine)."""
        out = self.values.failed_checks()
        if self.r0:
            out.add("R0")
        if any(not m <= self.r1_bound for _, m in self.r1):
            out.add("R1")
        return out


def forced_ids(run: mc.Run, rec_seq, count: int) -> torch.Tensor:
    """The recorded ids of positions [0, count) of one sequence, long [count,
    layers, k]; asserts the record's completeness on the way.  A position
    without a record is one the sequence adopted from the prefix cache: it
    takes the record of the earlier sequence with the same token prefix."""
    records = run.route.records
    seq = rec_seq.seq
    tokens = seq.prompt_tokens + seq.output_tokens
    layers = run.engine.cfg.model.num_layers
    adopted = seq.cached_prefix_len
    rows = []
    for pos in range(count):
        own = [records.get((seq.seq_id, pos, li), []) for li in range(layers)]
        if pos < adopted:
            assert not any(own), "an adopted position was computed again"
            donor = next(
                r.seq for r in run.rec.seqs.values()
                if r.seq.seq_id < seq.seq_id and r.weights == rec_seq.weights
                and (r.seq.prompt_tokens + r.seq.output_tokens)[:pos + 1]
                == tokens[:pos + 1] and (r.seq.seq_id, pos, 0) in records)
            own = [records[(donor.seq_id, pos, li)] for li in range(layers)]
        assert all(len(o) == 1 for o in own), (
            "seq %d position %d recorded %s times per layer" % (
                seq.seq_id, pos, [len(o) for o in own]))
        rows.append(torch.stack([o[0][1] for o in own]))
    return torch.stack(rows).long()


def judge(run: mc.Run) -> MoeVerdict:
    """C1, C2, C3, R0, R1 and the cap for a finished eager run.  Must be
    called outside any mutant."""
    assert run.route is not None, "a graph run has no routing record"
    rec, records = run.rec, run.route.records
    table = run.engine.runner.model.cos_sin
    cfg = run.engine.cfg.model
    k, layers = cfg.num_experts_per_tok, cfg.num_layers
    with moe_conf():
        models = [mc.cpu_model(CONF, params, table) for params in rec.weights]
    c1, c2, r0, r1 = [], [], [], []
    delta, gaps, expected = 0.0, [], set()
    margins = []
    for n, rec_seq in enumerate(rec.seqs.values()):
        seq = rec_seq.seq
        tokens = seq.prompt_tokens + seq.output_tokens
        T = len(tokens)
        assert rec_seq.final_kv is not None and rec_seq.final_count == T - 1
        assert [r[0] for r in rec_seq.rows] == list(
            range(seq.num_prompt_tokens, T))
        model = models[rec_seq.weights]
        forced = forced_ids(run, rec_seq, T - 1)
        ref_logits, ref_kv, l64 = moe_forward64(model, tokens[:-1], forced)
        with moe_conf():
            cpu_logits, cpu_kv, l_cpu = cpu_forward_forced(
                model, tokens[:-1], forced)
        delta = max(delta, float((l_cpu.double() - l64).abs().max()))
        srt = l64.sort(dim=-1, descending=True).values
        gaps.append((srt[..., k - 1] - srt[..., k]).flatten())
        e_logits = max(mc.rel_l2(cpu_logits[t], ref_logits[t])
                       for t in range(T - 1))
        what = "seq %d (prompt %d)" % (n, seq.num_prompt_tokens)
        for num_tokens, row in rec_seq.rows:
            c1.append(("%s row %d" % (what, num_tokens),
                       mc.rel_l2(row, ref_logits[num_tokens - 1]), e_logits))
        for layer in range(layers):
            for j, name in enumerate("KV"):
                c2.append(("%s layer %d %s" % (what, layer, name),
                           mc.rel_l2(rec_seq.final_kv[:, layer, j],
                                     ref_kv[:, layer, j]),
                           mc.rel_l2(cpu_kv[:, layer, j],
                                     ref_kv[:, layer, j])))
        for pos in range(seq.cached_prefix_len, T - 1):
            for layer in range(layers):
                key = (seq.seq_id, pos, layer)
                expected.add(key)
                (lg, ids), = records[key]
                where = "%s position %d layer %d" % (what, pos, layer)
                if not torch.equal(ids, moe.route_ref(lg[None], k, True)[0][0]):
                    r0.append("%s: ids %s" % (where, ids.tolist()))
                chosen = torch.zeros(l64.shape[-1], dtype=torch.bool)
                chosen[ids.long()] = True
                row = l64[pos, layer]
                margins.append((where, float(row[~chosen].max() -
                                             row[chosen].min())))
    assert set(records) == expected, "records of rows no sequence owns"
    r1 = margins
    gaps = torch.cat(gaps)
    ambiguous = float((gaps <= 2 * FACTOR * delta).double().mean())
    c3 = mc.poison_violations(run.kv_after, run.poison, rec.written_mask(),
                              rec.owned, run.graph_mode)
    return MoeVerdict(mc.Verdict(c1, c2, c3), r0, r1, delta, ambiguous,
                      int(gaps.numel()))


def graph_failures(graph: mc.Run, eager: mc.Run) -> List[str]:
    """A graph run against its eager twin: C3 on its own pool, every logits
    row and every sequence's final K/V rows bit for bit."""
    out = ["C3 " + v for v in mc.poison_violations(
        graph.kv_after, graph.poison, graph.rec.written_mask(),
        graph.rec.owned, graph.graph_mode)]
    a, b = list(graph.rec.seqs.values()), list(eager.rec.seqs.values())
    assert len(a) == len(b)
    for n, (g, e) in enumerate(zip(a, b)):
        assert g.seq.prompt_tokens == e.seq.prompt_tokens
        if g.sampled != e.sampled:
            out.append("seq %d: tokens %s != %s" % (n, g.sampled, e.sampled))
        for (ng, rg), (ne, re_) in zip(g.rows, e.rows):
            if ng != ne or not torch.equal(rg, re_):
                out.append("seq %d: logits row %d differs (max |diff| %.3g)"
                           % (n, ng, float((rg - re_).abs().max())))
        if g.final_count != e.final_count or not torch.equal(
                g.final_kv.view(torch.int16), e.final_kv.view(torch.int16)):
            out.append("seq %d: final K/V rows differ" % n)
    return out


# ---------------------------------------------------------------------------
# mutants: wrong engines, used only by the CPU self-test
# ---------------------------------------------------------------------------

def _wrap_ffn(edit):
    ffn = ops.moe_ffn
    return mc._patched(ops, "moe_ffn", lambda x, w1, w2, ids, w: ffn(
        *edit(x, w1, w2, ids, w)))


def _mut_no_renormalize(engine):
    route = ops.moe_route
    return mc._patched(ops, "moe_route",
                       lambda lg, k, rn=True: route(lg, k, False))


def _mut_weights_reversed(engine):
    return _wrap_ffn(lambda x, w1, w2, ids, w:
                     (x, w1, w2, ids, w.flip(1).contiguous()))


def _mut_expert_plus_1(engine):
    return _wrap_ffn(lambda x, w1, w2, ids, w:
                     (x, w1, w2, (ids + 1) % w1.shape[0], w))


def _mut_gate_up_swapped(engine):
    def edit(x, w1, w2, ids, w):
        inter = w2.shape[2]
        return x, torch.cat([w1[:, inter:], w1[:, :inter]], 1).contiguous(), \
            w2, ids, w
    return _wrap_ffn(edit)


def _mut_layer_0_experts(engine):
    first, second = (l.mlp for l in engine.runner.model.layers)

    def edit(x, w1, w2, ids, w):
        if w1 is second.w1:
            w1, w2 = first.w1, first.w2
        return x, w1, w2, ids, w
    return _wrap_ffn(edit)


def _mut_router_unnormed(engine):
    """The router reads the residual stream, not its post-attention norm."""
    box = {}
    fused = ops.linear_add_rmsnorm

    def fused_(x, w, residual, norm_weight, eps, *rest):
        out = fused(x, w, residual, norm_weight, eps, *rest)
        box["residual"] = residual
        return out

    def forward(self, x):
        ids, w = ops.moe_route(ops.linear(box["residual"], self.w_router),
                               self.top_k, self.renormalize)
        return ops.moe_ffn(x, self.w1, self.w2, ids, w)

    stack = contextlib.ExitStack()
    stack.enter_context(mc._patched(ops, "linear_add_rmsnorm", fused_))
    stack.enter_context(mc._patched(MoEBlock, "forward", forward))
    return stack


def _route_by(order_of):
    """A router that picks by order_of(logits) [T, E] -> expert order, with
    the weights a correct router gives those experts."""
    def route(logits, top_k, renormalize=True):
        x = logits.float()
        ids = order_of(x)[:, :top_k]
        w = torch.softmax(x, dim=-1).gather(1, ids)
        if renormalize:
            w = w / w.sum(1, keepdim=True)
        return ids.to(torch.int32).contiguous(), w.contiguous()
    return route


def _mut_k_smallest(engine):
    return mc._patched(ops, "moe_route", _route_by(
        lambda x: torch.sort(x, dim=-1, stable=True).indices))


def _mut_ties_to_higher(engine):
    def order(x):
        E = x.shape[1]
        return E - 1 - torch.sort(x.flip(1), dim=-1, descending=True,
                                  stable=True).indices
    return mc._patched(ops, "moe_route", _route_by(order))


def _mut_stale_grouping(engine):
    """A decode step computes with the ids of the call before it (the
    grouping a kernel would find left over), while returning fresh ones."""
    box = {}

    def edit(x, w1, w2, ids, w):
        stale = box.get("ids")
        box["ids"] = ids
        if stale is not None and stale.shape == ids.shape and \
                ids.shape[0] <= 8:
            ids = stale
        return x, w1, w2, ids, w
    return _wrap_ffn(edit)


class Mutant(NamedTuple):
    make: object                         # engine -> context manager
    checks: Tuple[str, ...]              # every one of these must fail
    passes: Tuple[str, ...] = ()         # and these must not


MUTANTS: Dict[str, Mutant] = {
    "no_renormalize": Mutant(_mut_no_renormalize, ("C1",)),
    "weights_reversed": Mutant(_mut_weights_reversed, ("C1",)),
    "expert_plus_1": Mutant(_mut_expert_plus_1, ("C1",)),
    "gate_up_swapped": Mutant(_mut_gate_up_swapped, ("C1",)),
    "layer_0_experts": Mutant(_mut_layer_0_experts, ("C1",)),
    "router_unnormed": Mutant(_mut_router_unnormed, ("R1", "C1")),
    # the reference follows the recorded ids and the weights are the right
    # ones for them, so the values agree: only the routing checks can see it
    "k_smallest": Mutant(_mut_k_smallest, ("R1",), ("C1",)),
    "ties_to_higher": Mutant(_mut_ties_to_higher, ("R0",)),
    "stale_grouping": Mutant(_mut_stale_grouping, ("C1",)),
}


def has_ties(run: mc.Run) -> bool:
    """Whether some recorded row has equal bf16 logits among its k + 1
    largest: where ties_to_higher changes what the router returns."""
    k = run.engine.cfg.model.num_experts_per_tok
    for (lg, _), in run.route.records.values():
        top = lg.float().sort(descending=True).values[:k + 1]
        if bool((top[1:] == top[:-1]).any()):
            return True
    return False
