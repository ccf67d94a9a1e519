"""P/D-disaggregated benchmark harness — the BASELINE headline config.

Realizes "Llama-3-8B P/D-disagg" (BASELINE.json configs 3-5) in the driver's
bench contract: ONE prefill engine (rank 0) feeds a decode engine on EVERY
rank.  Prompts are prefilled on the prefill engine (first token sampled
there), then their KV pages migrate to the target decode engine:

  rank 0 -> rank 0   same process: gather/scatter copy kernel via the
                     pool's raw pointer (CPU: tensor index_copy)
  rank 0 -> rank r   hipIpc-mapped peer pool + kv_peer_copy kernel — the
                     stores ride the point-to-point xGMI link (CPU test
                     path: gloo send/recv with the bf16 wire helpers)

Control metadata (page counts, token ids, commits) travels over a gloo
process group — tiny, latency-tolerant — so the GPU dataplane needs NO
collective library at all: this is the reference's Mooncake transfer path
(keps/74-mooncake-integration) reduced to one xGMI hop.

The timed region is pure decode on every rank (prefill rank idles after the
fill phase), so `value` scales with ranks like the dp mode while TTFT
captures the real prefill + migration + enqueue path per request.
"""
from __future__ import annotations

import time
from typing import Any, Dict, List, Optional

import torch

from .config import EngineConfig, ModelConfig
from .engine import LLMEngine
from .kv_cache import BlockTable
from .sequence import SamplingParams, Sequence


def _park_finished_pages(engine: LLMEngine, parked: Dict[int, List[int]]):
    """Prefill engines keep finished sequences' pages for migration
    (the serve_worker retire_keep_pages pattern)."""
    sched = engine.scheduler
    orig = sched._retire_finished

    def retire_keep_pages():
        for s in list(sched.running):
            if s.should_stop() and s.block_table is not None:
                parked[s.seq_id] = list(s.block_table.pages)
                s.block_table.pages = []
                s.block_table.num_shared = 0
        orig()
    sched._retire_finished = retire_keep_pages


def _make_engine(args, device: str, role: str,
                 max_new: int) -> LLMEngine:
    model_cfg = ModelConfig.preset(args.model)
    horizon = args.seq_len + max_new + 64
    cfg = EngineConfig(
        model=model_cfg, device=device,
        max_batch_size=max(args.batch, 8),
        max_seq_len=horizon,
        max_prefill_tokens=8192,
        enforce_eager=args.eager or device != "cuda" or role == "prefill",
        enable_prefix_cache=False,           # random prompts: no reuse
        kv_pool_tokens=args.batch * horizon + 4096)
    return LLMEngine(cfg)


class _Migrator:
    """Moves a batch of parked page-sets from the prefill cache into a
    decode pool, by whichever dataplane applies (see module docstring)."""

    def __init__(self, device: str):
        self.device = device
        self._pusher = None

    def push_local(self, src_cache, dst_cache, src_pages: List[int],
                   dst_pages: List[int]) -> None:
        if self.device == "cuda":
            from ..parallel.kv_peer import PeerKVPusher, export_meta_local
            if self._pusher is None:
                self._pusher = PeerKVPusher(src_cache.kv.device)
            pending = self._pusher.push(src_cache, src_pages,
                                        export_meta_local(dst_cache),
                                        dst_pages)
            pending.wait()
        else:
            # the same refusals as the kernel path, then a byte copy (an
            # e4m3 pool has no index kernels of its own: pool_bytes)
            from ..parallel.comm import check_kv_signature, pool_bytes
            from ..parallel.kv_peer import check_push_args
            check_kv_signature(src_cache.signature(), dst_cache.signature(),
                               "local push")
            check_push_args(list(src_cache.kv.shape), src_pages,
                            {"shape": list(dst_cache.kv.shape),
                             "num_pages": int(dst_cache.kv.shape[2])},
                            dst_pages)
            src_idx = torch.tensor(src_pages, dtype=torch.int64)
            dst_idx = torch.tensor(dst_pages, dtype=torch.int64)
            pool_bytes(dst_cache.kv).index_copy_(
                2, dst_idx,
                pool_bytes(src_cache.kv).index_select(2, src_idx))

    def push_remote(self, src_cache, peer_meta: Dict[str, Any],
                    src_pages: List[int], dst_pages: List[int],
                    dst_rank: int) -> None:
        from ..parallel.kv_peer import PeerKVPusher
        if self._pusher is None:
            self._pusher = PeerKVPusher(src_cache.kv.device)
        pending = self._pusher.push(src_cache, src_pages, peer_meta,
                                    dst_pages)
        pending.wait()


def _enqueue_imported(engine: LLMEngine, tokens: List[int],
                      first_token: int, pages: List[int],
                      max_new: int) -> Sequence:
    seq = Sequence(tokens, SamplingParams(max_new_tokens=max_new,
                                          ignore_eos=True))
    seq.imported_kv = True
    bt = BlockTable(engine.runner.cache)
    bt.pages = list(pages)
    seq.block_table = bt
    seq.append_token(int(first_token))
    bt.ensure(seq.num_tokens + max_new)
    seq.status = "running"
    engine.scheduler.running.append(seq)
    return seq


def _verify() -> bool:
    import os
    return bool(os.environ.get("RBG_PD_VERIFY"))


_DIGEST_MUL = 0x9E3779B97F4A7C15         # odd: a bijection mod 2^64
_DIGEST_MASK = (1 << 64) - 1


def _page_checksum(cache, pages: List[int]) -> int:
    """Exact, order-sensitive digest of the selected pages' bytes, as an
    unsigned 64-bit Python int (compared with ==).

    Per list position i the page's [layers * 2, words] int16 words (uint8
    for an e4m3 pool) are summed with the odd weight 2 * (c * words + w) + 1
    of their (chunk c = layer * 2 + k|v, offset w) place, in wrap-around
    int64; the per-page sums are then chained, d = d * M + s_i + i + 1
    (mod 2^64, M odd).  Moving data between layers, between K and V, between
    offsets inside a page or between list positions changes a weight that
    multiplies it; the plain sum this replaces was blind to all four.  One
    page at a time, so the temporary is one page of int64."""
    kv = cache.kv
    raw = kv.view(torch.uint8) if kv.element_size() == 1 \
        else kv.view(torch.int16)
    chunks = raw.shape[0] * raw.shape[1]
    words = raw.shape[3] * raw.shape[4] * raw.shape[5]
    weight = (torch.arange(chunks * words, dtype=torch.int64,
                           device=kv.device) * 2 + 1).view(chunks, words)
    digest = 0
    for i, pg in enumerate(pages):
        page = raw[:, :, int(pg)].reshape(chunks, words).to(torch.int64)
        s = int((page * weight).sum().item())          # wraps mod 2^64
        digest = (digest * _DIGEST_MUL + s + i + 1) & _DIGEST_MASK
    return digest


def _prefill_batch(engine: LLMEngine, prompts: List[List[int]],
                   parked: Dict[int, List[int]]):
    """Prefill `prompts` to completion (1 token each); returns
    [(seq, pages)] with per-seq pages parked for migration."""
    seqs = [engine.add_request(p, SamplingParams(max_new_tokens=1,
                                                 ignore_eos=True))
            for p in prompts]
    while engine.scheduler.has_work():
        engine.step()
    return [(s, parked.pop(s.seq_id)) for s in seqs]


def watch_logits(engine: LLMEngine) -> Dict[str, torch.Tensor]:
    """Keep a reference (no copy, no sync) to the logits each step samples
    from, so the last timed step's can be written out afterwards."""
    runner = engine.runner
    box: Dict[str, torch.Tensor] = {}
    orig = runner.sample_device

    def sample_device(logits, seqs):
        box["logits"] = logits
        return orig(logits, seqs)
    runner.sample_device = sample_device
    return box


DUMP_LOGIT_COLS = 8192


def dump_outputs(out_dir: str, seqs: List[Sequence],
                 box: Dict[str, torch.Tensor]) -> None:
    """Write what the last decode step produced as ``out_dir/<name>.npy``:

      next_tokens        float64 [B]     the token each sequence received
      logits_sample      float32 [B, C]  the logits they were sampled from,
                                         at a fixed seeded set of C columns
      logits_sample_cols float64 [C]     those vocabulary columns

    The column sample keeps a 128 x 128k-vocab step at 4 MB."""
    import os

    import numpy as np
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "next_tokens.npy"),
            np.asarray([s.last_token for s in seqs], dtype=np.float64))
    if "logits" not in box:         # pp: only the last stage samples
        return
    logits = box["logits"].float().cpu().numpy()
    vocab = logits.shape[-1]
    cols = np.arange(vocab)
    if vocab > DUMP_LOGIT_COLS:
        cols = np.sort(np.random.default_rng(0).choice(
            vocab, DUMP_LOGIT_COLS, replace=False))
    np.save(os.path.join(out_dir, "logits_sample.npy"),
            np.ascontiguousarray(logits[:, cols], dtype=np.float32))
    np.save(os.path.join(out_dir, "logits_sample_cols.npy"),
            cols.astype(np.float64))


def run_pd(args, rank: int, world: int, device: str) -> Optional[dict]:
    """Returns the result dict on rank 0, None elsewhere.  With world==1
    both engines share the process (and GPU); with world>1 rank 0 hosts
    prefill + decode[0] and every other rank one decode engine."""
    import torch.distributed as dist
    distributed = world > 1
    max_new = args.steps + args.warmup + 32
    decode_engine = _make_engine(args, device, "decode", max_new)
    torch.manual_seed(1234)            # same prompt stream on every rank
    migrator = _Migrator(device)
    alloc = decode_engine.runner.cache

    t_fill0 = time.monotonic()
    ttfts: List[float] = []
    if rank == 0:
        prefill_engine = _make_engine(args, device, "prefill", 1)
        parked: Dict[int, List[int]] = {}
        _park_finished_pages(prefill_engine, parked)
        vocab = prefill_engine.cfg.model.vocab_size
        for r in range(world):
            prompts = [torch.randint(0, vocab, (args.seq_len,)).tolist()
                       for _ in range(args.batch)]
            done = _prefill_batch(prefill_engine, prompts, parked)
            if r == 0:
                # local migration into my own decode engine
                for s, pages in done:
                    dst = alloc.alloc(len(pages))
                    migrator.push_local(prefill_engine.runner.cache,
                                        alloc, pages, dst)
                    if _verify():
                        src_ck = _page_checksum(
                            prefill_engine.runner.cache, pages)
                        dst_ck = _page_checksum(alloc, dst)
                        assert src_ck == dst_ck, (src_ck, dst_ck)
                    _enqueue_imported(decode_engine, s.prompt_tokens,
                                      s.output_tokens[0], dst, max_new)
                    prefill_engine.runner.cache.free(pages)
                    ttfts.append(time.monotonic() - s.arrival_time)
            else:
                # ask rank r to allocate target pages
                dist.send_object_list(
                    [[len(pages) for _s, pages in done]], dst=r)
                reply: List[Any] = [None]
                dist.recv_object_list(reply, src=r)
                dst_lists, peer_meta = reply[0]
                pushed = False
                if device == "cuda":
                    try:
                        # ONE batched kernel launch for the whole batch
                        src_all = [p for _s, pages in done for p in pages]
                        dst_all = [p for lst in dst_lists for p in lst]
                        migrator.push_remote(prefill_engine.runner.cache,
                                             peer_meta, src_all, dst_all, r)
                        pushed = True
                    except Exception as e:  # noqa: BLE001
                        # first-multi-GPU safety net: if the cross-device
                        # hipIpc mapping is refused, fall back to the gloo
                        # wire path instead of failing the run
                        print(f"[pd_bench] xGMI push to rank {r} failed "
                              f"({e!r}); falling back to gloo wire",
                              flush=True)
                checks = None
                if _verify():
                    if device == "cuda":
                        torch.cuda.synchronize()
                    checks = [_page_checksum(prefill_engine.runner.cache,
                                             pages)
                              for _s, pages in done]
                commit = [([(s.prompt_tokens, s.output_tokens[0], lst)
                            for (s, _pg), lst in zip(done, dst_lists)],
                           checks, pushed)]
                dist.send_object_list(commit, dst=r)
                if not pushed:
                    from ..parallel.comm import pool_bytes, to_wire
                    for (_s, pages), _lst in zip(done, dst_lists):
                        idx = torch.tensor(
                            pages, dtype=torch.int64,
                            device=prefill_engine.runner.cache.kv.device)
                        buf = pool_bytes(
                            prefill_engine.runner.cache.kv).index_select(
                            2, idx).contiguous().cpu()
                        dist.send(to_wire(buf), r)
                now = time.monotonic()
                for s, pages in done:
                    prefill_engine.runner.cache.free(pages)
                    ttfts.append(now - s.arrival_time)
        prefill_wall = time.monotonic() - t_fill0
    else:
        req: List[Any] = [None]
        dist.recv_object_list(req, src=0)
        dst_lists = [alloc.alloc(n) for n in req[0]]
        if device == "cuda":
            from ..parallel.kv_peer import export_meta
            meta = export_meta(alloc)
        else:
            meta = None
        dist.send_object_list([(dst_lists, meta)], dst=0)
        commit: List[Any] = [None]
        dist.recv_object_list(commit, src=0)
        entries, checks, pushed = commit[0]
        if not pushed:
            # CPU path, or the sender's cross-device hipIpc push was
            # refused: page data arrives over the gloo wire AFTER the
            # commit message, one set per sequence
            from ..parallel.comm import from_wire, pool_bytes, wire_dtype
            pool = pool_bytes(alloc.kv)
            m = alloc.kv.shape
            for _tokens, _ft, pages in entries:
                buf = torch.empty(
                    (m[0], m[1], len(pages), m[3], m[4], m[5]),
                    dtype=wire_dtype(alloc.kv.dtype, torch.device("cpu")),
                    device="cpu")
                dist.recv(buf, 0)
                idx = torch.tensor(pages, dtype=torch.int64,
                                   device=alloc.kv.device)
                pool.index_copy_(2, idx,
                                 from_wire(buf, pool.dtype).to(
                                     alloc.kv.device))
        if checks is not None:
            # byte-exact transfer proof (RBG_PD_VERIFY=1): the imported
            # pages must digest identically to the sender's parked pages,
            # in the order the sender listed them
            for (_t, _f, pages), src_ck in zip(entries, checks):
                dst_ck = _page_checksum(alloc, pages)
                assert src_ck == dst_ck, (src_ck, dst_ck)
        for tokens, first_token, pages in entries:
            _enqueue_imported(decode_engine, tokens, first_token, pages,
                              max_new)
        prefill_wall = time.monotonic() - t_fill0

    assert len(decode_engine.scheduler.running) == args.batch, \
        f"rank {rank}: {len(decode_engine.scheduler.running)} running"
    if device == "cuda":
        torch.cuda.synchronize()

    # ---- warmup decode steps (captures hipGraphs) -------------------------
    for _ in range(args.warmup):
        m = decode_engine.step()
        assert m == "decode", m
    if device == "cuda":
        torch.cuda.synchronize()
    if distributed:
        dist.barrier()
    dump_dir = getattr(args, "dump_outputs", None) if rank == 0 else None
    if dump_dir:
        timed_seqs = list(decode_engine.scheduler.running)
        box = watch_logits(decode_engine)

    # ---- timed region: exactly K decode steps -----------------------------
    t_start = time.monotonic()
    for _ in range(args.steps):
        m = decode_engine.step()
        assert m == "decode", m
    if device == "cuda":
        torch.cuda.synchronize()
    elapsed = time.monotonic() - t_start
    if distributed:
        dist.barrier()
        t = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())

    if dump_dir:
        dump_outputs(dump_dir, timed_seqs, box)
    if rank != 0:
        return None
    ttfts.sort()
    total_tok_s = args.batch * world * args.steps / elapsed
    return {
        "total_tok_s": total_tok_s,
        "ms_per_step": elapsed / args.steps * 1000.0,
        "p50_ttft_ms": ttfts[len(ttfts) // 2] * 1000.0 if ttfts else 0.0,
        "prefill_wall_s": prefill_wall,
        "prefill_tok_s": args.batch * world * args.seq_len / prefill_wall,
        "parallelism": f"pd{world} (1 prefill + {world} decode, "
                       "prefill colocated with decode0)",
    }
