"""Shared scenarios, references and checks for the model-level conformance
tests.

A plain helper module (not a conftest, no `gpu` marker, needs no HIP
extension): tests/test_model_cases_cpu.py proves on the CPU that the checks
accept the engine running `ops.reference` and reject wrong engines (the
mutants), and tests/test_model_conformance_gpu.py runs the same scenarios and
the same checks against the engine on the GPU, where every op is a HIP kernel.

What is compared.  The engine (scheduler, model runner, paged cache, model)
runs a scenario with greedy sampling on a pool filled with finite poison.  A
recorder around `runner.sample_device` keeps every logits row the engine
sampled from and, at a sequence's last step, its K/V rows read through its
block table.  Afterwards, outside the engine:

  reference  a dense causal fp64 forward over each sequence's whole token
             history (prompt plus what the engine generated: teacher-forced,
             so a differing greedy token never matters).  No paging, no
             batching, no `ops.reference`; parameters are the bf16 weights
             upcast, the rotary table is the model's own (checked separately
             against a CPU-built one to one fp32 ulp).
  yardstick  the project's CPU path (`LlamaForCausalLM` on `ops.reference`,
             one full-history prefill per sequence) measured against that
             reference: e_cpu, a relative L2 error.  It rounds to bf16 at the
             same points as the kernels and differs from them only in fp32
             accumulation order and the fast exp (<= 2^-16 per operation
             against u = 2^-8), so the two errors are two draws from one
             distribution.

  C1 logits  every recorded row: relative L2 error <= 2 * e_cpu(logits) of its
             sequence (per position, maximum over the sequence's positions).
  C2 cache   per (sequence, layer, K|V), rows 0 .. num_tokens - 2: relative
             L2 error <= 2 * e_cpu of the same quantity.
  C3 poison  every slot that no sequence ever wrote still holds its poison
             bit for bit: never-owned pages, the tails of owned pages, and
             page 0 (in graph mode slot 0 of page 0 is exempt: padding rows
             and the capture warm-up write there).

The K/V rows of a sequence are read when it takes its last step, not after
the run: pages are released on finish and the next request reuses them.
"""
from __future__ import annotations

import contextlib
import math
from typing import Callable, Dict, List, NamedTuple, Optional, Set, Tuple

import torch

import attn_cases as ac
from rbg_amd import ops
from rbg_amd.engine.config import EngineConfig, ModelConfig
from rbg_amd.engine.engine import LLMEngine
from rbg_amd.engine.kv_cache import BlockTable, PagedKVCache, PrefixCache
from rbg_amd.engine.sequence import SamplingParams
from rbg_amd.models.llama import LlamaForCausalLM, LlamaLayer

BF16 = torch.bfloat16
PAGE = 16
MAX_SEQ_LEN = 512
POOL_TOKENS = 2048
FACTOR = 2.0                 # C1 / C2: err <= FACTOR * e_cpu
TABLE_TOL = 2.0 ** -23       # one fp32 ulp of a value in [-1, 1]
NORM_SEED = 20240607
RELOAD_SEED = 4321

CONFS = ("conf-llama", "conf-qwen")
SCENARIOS = ("mixed", "churn", "chunked", "prefix", "reload")


def model_config(conf: str) -> ModelConfig:
    if conf == "conf-llama":
        return ModelConfig(name=conf, hidden_size=512, intermediate_size=1024,
                           num_layers=2, num_heads=8, num_kv_heads=2,
                           head_dim=128, vocab_size=512, max_position=2048)
    if conf == "conf-qwen":
        return ModelConfig(name=conf, hidden_size=512, intermediate_size=1024,
                           num_layers=2, num_heads=4, num_kv_heads=1,
                           head_dim=128, vocab_size=512, max_position=2048,
                           qk_norm=True, rms_eps=1e-6)
    raise ValueError(conf)


def engine_config(conf: str, device: str, eager: bool,
                  pool_tokens: int = POOL_TOKENS, **kw) -> EngineConfig:
    return EngineConfig(model=model_config(conf), device=device,
                        page_size=PAGE, max_seq_len=MAX_SEQ_LEN,
                        kv_pool_tokens=pool_tokens, enforce_eager=eager, **kw)


# ---------------------------------------------------------------------------
# weights
# ---------------------------------------------------------------------------

def norm_params(model: LlamaForCausalLM) -> List[torch.nn.Parameter]:
    out = []
    for layer in model.layers:
        out += [layer.input_norm, layer.post_norm]
        if layer.attn.q_norm is not None:
            out += [layer.attn.q_norm, layer.attn.k_norm]
    out.append(model.final_norm)
    return out


def draw_norm_weights(model: LlamaForCausalLM, seed: int = NORM_SEED) -> None:
    """Every norm weight ~ U(0.5, 1.5) rounded to bf16, from a seeded CPU
    generator: with all-ones weights a swapped or missing one is invisible."""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for p in norm_params(model):
            w = (torch.rand(p.numel(), generator=gen) + 0.5).to(BF16)
            p.copy_(w.view(p.shape))


def snapshot_params(model: LlamaForCausalLM) -> List[torch.Tensor]:
    return [p.detach().cpu().clone() for p in model.parameters()]


def expected_params(conf: str, device: str, seed: int) -> List[torch.Tensor]:
    """The parameters a model built from `seed` has, constructed apart from
    the engine under test (device generators differ from CPU ones, so the
    model is built where the engine's is)."""
    model = LlamaForCausalLM(model_config(conf), torch.device(device),
                             base_seed=seed)
    draw_norm_weights(model)
    return snapshot_params(model)


def cpu_model(conf: str, params: List[torch.Tensor],
              cos_sin: torch.Tensor) -> LlamaForCausalLM:
    model = LlamaForCausalLM(model_config(conf), torch.device("cpu"))
    with torch.no_grad():
        own = list(model.parameters())
        assert len(own) == len(params)
        for p, q in zip(own, params):
            p.copy_(q)
    model.cos_sin = cos_sin.detach().cpu().clone()
    return model


def cos_sin_table_error(model: LlamaForCausalLM) -> float:
    """max |device-built table - CPU-built table|.  Both are made in fp64
    and rounded once, so two correct tables differ by at most one fp32 ulp
    of a value in [-1, 1]: TABLE_TOL."""
    cfg = model.cfg
    want = ops.reference.build_cos_sin_table(cfg.head_dim, cfg.max_position,
                                             cfg.rope_theta, device="cpu")
    got = model.cos_sin.detach().cpu()
    assert got.shape == want.shape and got.dtype == want.dtype
    return float((got.double() - want.double()).abs().max())


# ---------------------------------------------------------------------------
# fp64 dense reference and the CPU yardstick
# ---------------------------------------------------------------------------

def dense_forward64(model: LlamaForCausalLM, tokens: List[int]
                    ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Plain causal forward of one whole sequence in float64, nothing
    rounded.  `model` is a CPU model (its parameters are upcast; its cos_sin
    table is used as is).  Returns logits [T, vocab] and kv [T, layers, 2,
    KVH, D] (K after qk-norm and RoPE, V as projected)."""
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
        kvs.append(torch.stack([k, v], dim=1))     # [T, 2, KVH, D]
        sc = torch.einsum("qhgd,khd->hgqk", q.view(T, KVH, G, D), k) * scale
        p = torch.softmax(sc.masked_fill(future, float("-inf")), dim=-1)
        o = torch.einsum("hgqk,khd->qhgd", p, v).reshape(T, H * D)
        r = r + o @ w(a.wo).T
        gate, up = (rms(r, w(layer.post_norm)) @
                    w(layer.mlp.w_gate_up).T).chunk(2, dim=-1)
        r = r + (torch.nn.functional.silu(gate) * up) @ w(layer.mlp.w_down).T
    logits = rms(r, w(model.final_norm)) @ w(model.lm_head).T
    return logits, torch.stack(kvs, dim=1)


def gather_rows(kv: torch.Tensor, pages: List[int], count: int
                ) -> torch.Tensor:
    """Pool rows of positions [0, count) read through a block table:
    [count, layers, 2, KVH, D] on the CPU."""
    pos = torch.arange(count)
    pg = torch.tensor(pages, dtype=torch.long)[pos // PAGE].to(kv.device)
    off = (pos % PAGE).to(kv.device)
    return kv[:, :, pg, :, off].cpu()


def cpu_forward(model: LlamaForCausalLM, conf: str, tokens: List[int],
                cache_dtype=BF16) -> Tuple[torch.Tensor, torch.Tensor]:
    """The project's CPU path: one full-history prefill into a fresh CPU
    PagedKVCache.  Returns logits [T, vocab] fp32 and kv [T, layers, 2, KVH,
    D] as cached."""
    from rbg_amd.models.llama import ForwardBatch
    T = len(tokens)
    cfg = engine_config(conf, "cpu", True, enable_prefix_cache=False)
    cache = PagedKVCache(cfg, torch.device("cpu"),
                         num_pages=(T + PAGE - 1) // PAGE + 1)
    cache.kv = cache.kv.to(cache_dtype)
    table = BlockTable(cache)
    batch = ForwardBatch(
        mode="prefill",
        positions=torch.arange(T, dtype=torch.int32),
        slot_mapping=torch.tensor(table.slots_for(0, T), dtype=torch.int32),
        cu_seqlens=torch.tensor([0, T], dtype=torch.int32))
    hidden = model.forward(torch.tensor(tokens, dtype=torch.int64), batch,
                           cache)
    return model.logits(hidden), gather_rows(cache.kv, table.pages, T)


def rel_l2(got: torch.Tensor, ref: torch.Tensor) -> float:
    return float((got.double() - ref).norm() / ref.norm())


# ---------------------------------------------------------------------------
# poison
# ---------------------------------------------------------------------------

def poison_pool(cache: PagedKVCache, seed: int = 7) -> torch.Tensor:
    """Fill the whole pool with finite poison (K = +-4, V = 32768, the
    constants of attn_cases) and return the CPU copy it is judged against."""
    gen = torch.Generator().manual_seed(seed)
    poison = torch.empty(cache.kv.shape, dtype=BF16)
    poison[:, 0] = ((torch.randint(0, 2, poison[:, 0].shape, generator=gen)
                     * 2 - 1) * ac.K_POISON).to(BF16)
    poison[:, 1] = ac.V_POISON
    cache.kv.copy_(poison)
    return poison


def poison_violations(kv: torch.Tensor, poison: torch.Tensor,
                      written: torch.Tensor, owned: Set[int],
                      graph_mode: bool) -> List[str]:
    """C3.  kv / poison [layers, 2, pages, KVH, page, D]; written [pages,
    page] bool, the slots some sequence legitimately wrote."""
    changed = (kv.cpu().view(torch.int16) != poison.view(torch.int16)
               ).any(5).any(3).any(1).any(0)              # [pages, page]
    allowed = written.clone()
    assert not bool(allowed[0].any()), "page 0 is never a sequence's"
    if graph_mode:
        allowed[0, 0] = True
    out = []
    for pg, slot in (changed & ~allowed).nonzero().tolist():
        where = ("page 0" if pg == 0 else
                 "tail of owned page" if pg in owned else "never-owned page")
        out.append("%s: page %d slot %d" % (where, pg, slot))
    return out


# ---------------------------------------------------------------------------
# recording
# ---------------------------------------------------------------------------

class SeqRecord:
    def __init__(self, seq, weights: int):
        self.seq = seq
        self.weights = weights          # index into Recorder.weights
        self.rows: List[Tuple[int, torch.Tensor]] = []   # (num_tokens, logits)
        self.sampled: List[int] = []    # the token drawn from each row
        self.pages: List[int] = []
        self.final_kv: Optional[torch.Tensor] = None
        self.final_count = 0


class Recorder:
    """Wraps `runner.sample_device` (every logits row the engine samples
    from passes through it), `runner.decode` and `runner._decode_graph`."""

    def __init__(self, engine: LLMEngine, conf: str):
        self.engine = engine
        self.conf = conf
        self.runner = engine.runner
        self.seqs: Dict[int, SeqRecord] = {}
        self.owned: Set[int] = set()
        self.weights: List[List[torch.Tensor]] = []
        self.decode_batches: List[Tuple[int, ...]] = []
        self.graph_replays = 0
        self.use_weights(snapshot_params(self.runner.model))

    def use_weights(self, params: List[torch.Tensor]) -> None:
        """Sequences first seen from now on are judged against `params`."""
        self.weights.append(params)

    def __enter__(self):
        runner = self.runner
        self._orig = (runner.sample_device, runner.decode,
                      runner._decode_graph)
        sample, decode, graph = self._orig

        def sample_device(logits, seqs):
            rows = logits.detach().float().cpu()
            assert rows.shape[0] == len(seqs)
            for i, seq in enumerate(seqs):
                rec = self.seqs.get(seq.seq_id)
                if rec is None:
                    rec = self.seqs[seq.seq_id] = SeqRecord(
                        seq, len(self.weights) - 1)
                rec.rows.append((seq.num_tokens, rows[i].clone()))
                rec.pages = list(seq.block_table.pages)
                self.owned.update(rec.pages)
                if len(seq.output_tokens) + 1 >= seq.sampling.max_new_tokens:
                    # last step: rows 0 .. num_tokens - 1 are all written
                    rec.final_count = seq.num_tokens
                    rec.final_kv = gather_rows(self.runner.cache.kv,
                                               rec.pages, seq.num_tokens)
            out = sample(logits, seqs)
            for seq, tok in zip(seqs, out[1]):
                self.seqs[seq.seq_id].sampled.append(int(tok))
            return out

        def decode_(seqs):
            self.decode_batches.append(tuple(s.seq_id for s in seqs))
            return decode(seqs)

        def decode_graph(state, slots, n):
            self.graph_replays += 1
            return graph(state, slots, n)

        runner.sample_device = sample_device
        runner.decode = decode_
        runner._decode_graph = decode_graph
        return self

    def __exit__(self, *exc):
        for name in ("sample_device", "decode", "_decode_graph"):
            delattr(self.runner, name)     # back to the class's methods
        return False

    def written_mask(self) -> torch.Tensor:
        cache = self.runner.cache
        mask = torch.zeros(cache.num_pages, PAGE, dtype=torch.bool)
        for rec in self.seqs.values():
            for pos in range(rec.final_count):
                mask[rec.pages[pos // PAGE], pos % PAGE] = True
        return mask


class Trace:
    """Which kernels' entry points a run went through (shapes only)."""

    def __init__(self):
        self.linear_m: Set[int] = set()
        self.skinny_m: Set[int] = set()
        self.prefill: List[List[Tuple[int, int]]] = []    # per call (Lq, Lk)
        self.decode: List[Tuple[int, int]] = []           # (rows, splits)

    def __enter__(self):
        self._saved = [(ops, n, getattr(ops, n)) for n in
                       ("linear", "prefill_attention", "decode_attention")]
        linear, prefill, decode = (s[2] for s in self._saved)

        def linear_(x, w):
            self.linear_m.add(int(x.shape[0]))
            return linear(x, w)

        def prefill_(q, k, v, cu, scale, cu_k=None):
            lq = cu.diff().tolist()
            lk = cu_k.diff().tolist() if cu_k is not None else lq
            self.prefill.append(list(zip(lq, lk)))
            return prefill(q, k, v, cu, scale, cu_k)

        def decode_(q, kc, vc, bt, ctx, scale, num_splits=0, variant=-1,
                    **fp8_exponents):
            self.decode.append((int(q.shape[0]), int(num_splits)))
            return decode(q, kc, vc, bt, ctx, scale, num_splits=num_splits,
                          variant=variant, **fp8_exponents)

        ops.linear, ops.prefill_attention, ops.decode_attention = \
            linear_, prefill_, decode_
        if ops._hip is not None:
            skinny = ops._hip.skinny_gemm
            self._saved.append((ops._hip, "skinny_gemm", skinny))

            def skinny_(x, w, *rest):
                self.skinny_m.add(int(x.shape[0]))
                return skinny(x, w, *rest)

            ops._hip.skinny_gemm = skinny_
        return self

    def __exit__(self, *exc):
        for obj, name, fn in self._saved:
            setattr(obj, name, fn)
        return False


# ---------------------------------------------------------------------------
# scenarios
# ---------------------------------------------------------------------------

class Run:
    def __init__(self, scenario: str, conf: str, device: str, eager: bool):
        self.scenario, self.conf = scenario, conf
        self.device, self.eager = device, eager
        self.graph_mode = (not eager) and device != "cpu"
        self.engine: Optional[LLMEngine] = None
        self.rec: Optional[Recorder] = None
        self.trace = Trace()
        self.poison: Optional[torch.Tensor] = None
        self.kv_after: Optional[torch.Tensor] = None
        self.extra: Dict = {}

    @property
    def id(self) -> str:
        return "%s-%s-%s" % (self.scenario, self.conf,
                             "eager" if self.eager else "graph")


def _prompts(seed: int, lens, vocab: int = 512) -> List[List[int]]:
    gen = torch.Generator().manual_seed(seed)
    return [torch.randint(0, vocab, (n,), generator=gen).tolist()
            for n in lens]


def _greedy(n: int) -> SamplingParams:
    return SamplingParams(max_new_tokens=n, temperature=0.0)


def _drain(engine: LLMEngine) -> None:
    steps = 0
    while engine.scheduler.has_work():
        assert engine.step() != "idle", "engine stuck"
        steps += 1
        assert steps < 200


MIXED_BATCHES = ((1, 17, 40, 100), (40,), (5, 33, 64), (3, 16, 31, 48, 70))


def _mixed(run: Run) -> None:
    # 158 prefill rows (library GEMM); a lone 40 (skinny_gemm at M = 40);
    # decode batches of 4, 1, 3 and 5: graph buckets 4, 1, 4 (one padding
    # row) and 8 (three padding rows)
    for i, lens in enumerate(MIXED_BATCHES):
        run.engine.generate(_prompts(100 + i, lens), _greedy(6))


def _churn(run: Run) -> None:
    eng = run.engine
    seqs = [eng.add_request(p, _greedy(n)) for p, n in
            zip(_prompts(200, (9, 30, 50)), (2, 4, 7))]
    assert eng.step() == "prefill" and eng.step() == "decode"
    assert seqs[0].status == "finished"
    seqs.append(eng.add_request(_prompts(201, (21,))[0], _greedy(5)))
    _drain(eng)
    run.extra["ids"] = [s.seq_id for s in seqs]


def _chunked(run: Run) -> None:
    run.engine.generate(_prompts(300, (100, 40)), _greedy(4))


def _prefix(run: Run) -> None:
    eng = run.engine
    kv = eng.runner.cache.kv
    base = _prompts(400, (50,))[0]
    tail = _prompts(401, (7,))[0]
    assert tail[0] != base[48]
    (first,) = eng.generate([base], _greedy(4))
    shared = run.rec.seqs[first.seq_id].pages[:3]      # 48 tokens: 3 pages
    before = kv[:, :, shared].cpu().clone()
    later = []
    identical = []
    for prompt in (base, base[:48] + tail):
        (seq,) = eng.generate([prompt], _greedy(4))
        later.append(seq)
        identical.append(torch.equal(
            kv[:, :, shared].cpu().view(torch.int16),
            before.view(torch.int16)))
    run.extra.update(shared=shared, identical=identical,
                     cached=[s.cached_prefix_len for s in later],
                     later_pages=[run.rec.seqs[s.seq_id].pages[:3]
                                  for s in later])


def _reload(run: Run) -> None:
    eng = run.engine
    eng.generate(_prompts(500, (20,)), _greedy(5))
    graphs = dict(eng.runner._graphs)
    replays = run.rec.graph_replays
    eng.reload_weights(RELOAD_SEED)
    draw_norm_weights(eng.runner.model)
    # judged against a model built apart from reload_weights
    run.rec.use_weights(expected_params(run.conf, run.device, RELOAD_SEED))
    eng.generate(_prompts(501, (35,)), _greedy(5))
    run.extra.update(
        graphs_kept=all(eng.runner._graphs.get(b) is g
                        for b, g in graphs.items()),
        buckets_before=sorted(graphs),
        replays_after=run.rec.graph_replays - replays)


_SCENARIO_FN: Dict[str, Callable[[Run], None]] = {
    "mixed": _mixed, "churn": _churn, "chunked": _chunked,
    "prefix": _prefix, "reload": _reload}
_SCENARIO_KW = {"chunked": {"max_prefill_tokens": 24}}


def run_scenario(scenario: str, conf: str, device: str, eager: bool,
                 after_build: Optional[Callable[[LLMEngine], None]] = None
                 ) -> Run:
    """Build one small engine, poison its pool and drive the scenario."""
    run = Run(scenario, conf, device, eager)
    run.engine = LLMEngine(engine_config(conf, device, eager,
                                         **_SCENARIO_KW.get(scenario, {})))
    draw_norm_weights(run.engine.runner.model)
    run.poison = poison_pool(run.engine.runner.cache)
    if after_build is not None:
        after_build(run.engine)
    run.rec = Recorder(run.engine, conf)
    with run.trace, run.rec:
        _SCENARIO_FN[scenario](run)
    run.kv_after = run.engine.runner.cache.kv.cpu().clone()
    return run


def assert_paths(run: Run) -> None:
    """The path a scenario is meant to reach actually ran."""
    eng, rec, tr = run.engine, run.rec, run.trace
    runner = eng.runner
    gpu = run.device != "cpu"
    sizes = [len(b) for b in rec.decode_batches]
    assert runner._splits_for(1) == 16          # empty splits at model level
    if run.graph_mode:
        assert rec.graph_replays == len(rec.decode_batches) > 0
        # python reaches the decode kernel only to warm up and to capture
        assert sorted(n for n, _ in tr.decode) == sorted(
            b for b in runner._graphs
            for _ in range(2 * eng.cfg.model.num_layers))
    else:
        assert rec.graph_replays == 0 and not runner._graphs
        assert [n for n, _ in tr.decode] == [
            n for n in sizes for _ in range(eng.cfg.model.num_layers)]
        assert all(s == runner._splits_for(n) for n, s in tr.decode)
    if run.scenario == "mixed":
        assert sum(MIXED_BATCHES[0]) == 158 and 158 in tr.linear_m
        assert 40 in tr.linear_m
        if gpu:
            assert 40 in tr.skinny_m and 158 not in tr.skinny_m
            # decode rows: as batched in eager mode, as captured otherwise
            assert ({1, 4, 8} if run.graph_mode else {1, 3, 4, 5}) \
                <= tr.skinny_m
        assert set(sizes) == {4, 1, 3, 5}
        if run.graph_mode:
            assert set(runner._graphs) == {1, 4, 8}
    elif run.scenario == "churn":
        a, b, c, d = run.extra["ids"]
        batches = [k for i, k in enumerate(rec.decode_batches)
                   if i == 0 or k != rec.decode_batches[i - 1]]
        assert batches == [(a, b, c), (b, c, d), (c, d), (c,)], batches
        # two prefill steps, the second between two decode steps
        assert len(tr.prefill) == 2 * eng.cfg.model.num_layers
        if run.graph_mode:
            assert set(runner._graphs) == {1, 2, 4}
    elif run.scenario == "chunked":
        assert eng.stats.prefill_steps > 2
        per_call = tr.prefill[::eng.cfg.model.num_layers]
        assert len(per_call) == eng.stats.prefill_steps
        assert all(sum(lq for lq, _ in call) <= 24 for call in per_call)
        # one step batches a sequence with a past and one without
        assert any(len(call) == 2 and call[0][1] > call[0][0] and
                   call[1][1] == call[1][0] for call in per_call), per_call
    elif run.scenario == "prefix":
        assert runner.cache.prefix.hits > 0
        assert run.extra["cached"] == [48, 48]
        assert run.extra["later_pages"] == [run.extra["shared"]] * 2
        assert [(2, 50), (7, 55)] == [
            call[0] for call in tr.prefill[eng.cfg.model.num_layers::
                                           eng.cfg.model.num_layers]]
        assert run.extra["identical"] == [True, True], \
            "adopted pages changed under a later request"
    elif run.scenario == "reload":
        assert len(rec.weights) == 2
        assert {r.weights for r in rec.seqs.values()} == {0, 1}
        assert any(not torch.equal(p, q) for p, q in zip(*rec.weights))
        if run.graph_mode:
            assert run.extra["buckets_before"] == [1]
            assert run.extra["graphs_kept"] and set(runner._graphs) == {1}
            assert run.extra["replays_after"] == 4


# ---------------------------------------------------------------------------
# checks
# ---------------------------------------------------------------------------

class Verdict(NamedTuple):
    c1: List[Tuple[str, float, float]]      # (what, err, e_cpu)
    c2: List[Tuple[str, float, float]]
    c3: List[str]

    def failures(self) -> List[str]:
        out = ["C1 %s: err %.4g > %g * e_cpu %.4g" % (w, e, FACTOR, y)
               for w, e, y in self.c1 if not e <= FACTOR * y]
        out += ["C2 %s: err %.4g > %g * e_cpu %.4g" % (w, e, FACTOR, y)
                for w, e, y in self.c2 if not e <= FACTOR * y]
        return out + ["C3 " + v for v in self.c3]

    def failed_checks(self) -> Set[str]:
        """Subset of {"C1", "C2K", "C2V", "C3"}."""
        out = set()
        if any(not e <= FACTOR * y for _, e, y in self.c1):
            out.add("C1")
        for w, e, y in self.c2:
            if not e <= FACTOR * y:
                out.add("C2K" if w.endswith("K") else "C2V")
        if self.c3:
            out.add("C3")
        return out

    def worst(self) -> Tuple[float, float]:
        """Worst err / e_cpu over the logits rows and over the K/V blocks."""
        return (max(e / y for _, e, y in self.c1),
                max(e / y for _, e, y in self.c2))


def judge(run: Run) -> Verdict:
    """C1, C2 and C3 for a finished run.  Must be called outside any mutant:
    the reference and the yardstick run the unmodified project code."""
    rec = run.rec
    table = run.engine.runner.model.cos_sin
    models = [cpu_model(run.conf, params, table) for params in rec.weights]
    c1, c2 = [], []
    for n, rec_seq in enumerate(rec.seqs.values()):
        seq = rec_seq.seq
        tokens = seq.prompt_tokens + seq.output_tokens
        T = len(tokens)
        assert rec_seq.final_kv is not None and rec_seq.final_count == T - 1
        assert [r[0] for r in rec_seq.rows] == list(
            range(seq.num_prompt_tokens, T))
        model = models[rec_seq.weights]
        ref_logits, ref_kv = dense_forward64(model, tokens)
        cpu_logits, cpu_kv = cpu_forward(model, run.conf, tokens)
        e_logits = max(rel_l2(cpu_logits[t], ref_logits[t]) for t in range(T))
        for num_tokens, row in rec_seq.rows:
            c1.append(("seq %d (prompt %d) row %d" % (
                n, seq.num_prompt_tokens, num_tokens),
                rel_l2(row, ref_logits[num_tokens - 1]), e_logits))
        for layer in range(ref_kv.shape[1]):
            for j, name in enumerate("KV"):
                c2.append(("seq %d (prompt %d) layer %d %s" % (
                    n, seq.num_prompt_tokens, layer, name),
                    rel_l2(rec_seq.final_kv[:, layer, j],
                           ref_kv[:T - 1, layer, j]),
                    rel_l2(cpu_kv[:T - 1, layer, j],
                           ref_kv[:T - 1, layer, j])))
    c3 = poison_violations(run.kv_after, run.poison, rec.written_mask(),
                           rec.owned, run.graph_mode)
    return Verdict(c1, c2, c3)


# ---------------------------------------------------------------------------
# mutants: wrong engines, used only by the CPU self-test
# ---------------------------------------------------------------------------

@contextlib.contextmanager
def _patched(obj, name, value):
    saved = getattr(obj, name)
    setattr(obj, name, value)
    try:
        yield
    finally:
        setattr(obj, name, saved)


def _edit_batches(edit: Callable) -> contextlib.AbstractContextManager:
    """Run every model step on an edited ForwardBatch."""
    orig = LlamaForCausalLM.forward

    def forward(self, tokens, batch, kv, hidden=None):
        import dataclasses
        batch = dataclasses.replace(batch)
        edit(batch)
        return orig(self, tokens, batch, kv, hidden=hidden)

    return _patched(LlamaForCausalLM, "forward", forward)


def _mut_ctx_minus_1(engine):
    def edit(b):
        if b.mode == "decode":
            b.context_lens = b.context_lens - 1
    return _edit_batches(edit)


def _mut_rope_plus_1(engine):
    def edit(b):
        if b.mode == "decode":
            b.positions = b.positions + 1
    return _edit_batches(edit)


def _mut_slot_plus_1(engine):
    def edit(b):
        if b.mode == "decode":
            b.slot_mapping = b.slot_mapping + 1
    return _edit_batches(edit)


def _mut_stale_block_table(engine):
    runner = engine.runner
    build = runner._build_decode_state

    def stale(seqs):
        old = getattr(runner, "_dstate", None)
        state = build(seqs)
        if old is not None:
            r = min(old["bt"].shape[0], state["bt"].shape[0])
            c = min(old["bt"].shape[1], state["bt"].shape[1])
            state["bt"][:r, :c] = old["bt"][:r, :c]
        return state

    return _patched(runner, "_build_decode_state", stale)


def _mut_ignore_past(engine):
    def edit(b):
        if b.mode == "prefill":
            b.kv_gather_slots = None
            b.cu_seqlens_k = None
    return _edit_batches(edit)


def _mut_prefix_swap(engine):
    match = PrefixCache.match

    def swapped(self, prompt):
        got = match(self, prompt)
        if len(got) >= 2:
            got[0], got[1] = got[1], got[0]
        return got

    return _patched(PrefixCache, "match", swapped)


def _mut_reload_noop(engine):
    return _patched(LlamaForCausalLM, "reload_weights",
                    lambda self, seed: None)


def _mut_norm_swap(engine):
    def forward(self, x, residual, batch, kv, cos_sin):
        if residual is None:
            residual = x.clone()
            h = ops.rmsnorm(x, self.post_norm, self.eps)
        else:
            ops.fused_add_rmsnorm(x, residual, self.post_norm, self.eps)
            h = x
        h = self.attn(h, batch, kv, cos_sin)
        ops.fused_add_rmsnorm(h, residual, self.input_norm, self.eps)
        return self.mlp(h), residual

    return _patched(LlamaLayer, "forward", forward)


def _mut_k_norm_from_q(engine):
    swap = {id(l.attn.k_norm): l.attn.q_norm
            for l in engine.runner.model.layers}
    rmsnorm = ops.rmsnorm
    return _patched(ops, "rmsnorm", lambda x, w, eps: rmsnorm(
        x, swap.get(id(w), w), eps))


def _mut_cache_layer_0(engine):
    stack = contextlib.ExitStack()
    stack.enter_context(_patched(PagedKVCache, "key_cache",
                                 lambda self, layer: self.kv[0, 0]))
    stack.enter_context(_patched(PagedKVCache, "value_cache",
                                 lambda self, layer: self.kv[0, 1]))
    return stack


class Mutant(NamedTuple):
    make: Callable                       # engine -> context manager
    scenarios: Tuple[str, ...]           # where the scenario has what it breaks
    confs: Tuple[str, ...]
    checks: Tuple[str, ...]              # at least one of these must fail


# "applies" is decided from the scenario alone: a stale block table needs a
# decode batch whose tables differ from its predecessor's (chunked has one
# batch; prefix re-issues the same pages to every request), ignoring the past
# needs a prefill with a past, and so on
MUTANTS: Dict[str, Mutant] = {
    "ctx_minus_1": Mutant(_mut_ctx_minus_1, SCENARIOS, CONFS, ("C1",)),
    "rope_plus_1": Mutant(_mut_rope_plus_1, SCENARIOS, CONFS, ("C2K",)),
    "slot_plus_1": Mutant(_mut_slot_plus_1, SCENARIOS, CONFS,
                          ("C2K", "C2V", "C3")),
    "stale_block_table": Mutant(_mut_stale_block_table,
                                ("mixed", "churn", "reload"), CONFS,
                                ("C1", "C2K", "C2V")),
    "ignore_past": Mutant(_mut_ignore_past, ("chunked", "prefix"), CONFS,
                          ("C1",)),
    # C1 cannot see this one: K carries its rotation, so softmax attention
    # is invariant to the order the keys are read in; the rows are in the
    # wrong places of the block table, which is C2's business
    "prefix_swap": Mutant(_mut_prefix_swap, ("prefix",), CONFS,
                          ("C2K", "C2V")),
    "reload_noop": Mutant(_mut_reload_noop, ("reload",), CONFS, ("C1",)),
    "norm_swap": Mutant(_mut_norm_swap, SCENARIOS, CONFS, ("C1",)),
    "k_norm_from_q": Mutant(_mut_k_norm_from_q, SCENARIOS, ("conf-qwen",),
                            ("C2K",)),
    "cache_layer_0": Mutant(_mut_cache_layer_0, SCENARIOS, CONFS,
                            ("C1", "C2K", "C2V")),
}


def run_mutant(name: str, scenario: str, conf: str) -> Run:
    """The scenario on a CPU engine with the mutant patched in for the
    engine's run only (judge() is called by the test, outside it)."""
    stack = contextlib.ExitStack()
    with stack:
        return run_scenario(
            scenario, conf, "cpu", True,
            after_build=lambda eng: stack.enter_context(
                MUTANTS[name].make(eng)))
