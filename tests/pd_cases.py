"""Shared cases, harnesses and mutants for the prefill/decode (P/D) handoff
conformance tests.

A plain helper module (not a conftest, no `gpu` marker, needs no HIP
extension): tests/test_pd_cases_cpu.py proves on the CPU that the checks
accept the project's own handoff and reject wrong ones (the mutants), and
tests/test_pd_conformance_gpu.py runs the same cases with the
`kv_peer_copy` kernel and the HIP engines.

Three layers.

  copy cases   `kv_peer_copy` alone on plain pools [L, 2, P, 1, 1, hd].
               Every 16-byte vector of the source is unique (an int32 ramp
               of chunk, page and vector index); the destination holds a
               second, disjoint ramp and sits between two guard bands of a
               third.  After the copy the whole allocation, guards included,
               must `torch.equal` the `index_copy_` of `index_select` built
               on the CPU, and the source must be unchanged.
  H1           two engines driven through the functions
               `pd_bench.run_pd` is made of.  P (eager, 2048-token pool)
               prefills and samples the first token; its parked pages are
               pushed into D (eager or graph, 1536-token pool), which
               continues the sequence.  Both pools start as different
               poison.
  H2           the serving handshake: `ServeWorker`'s real `_rpc_prefill`,
               `_rpc_import_seq`, `_rpc_import_commit` and what they call, on
               two `SimpleNamespace` workers joined by a JSON round-tripping
               fake `RpcClient`.

Checks (C1 to C3 as in model_cases, the bound is its FACTOR x e_cpu):

  C0 transfer  right after each push D's whole pool equals its content
               before the push with P's parked pages copied to the
               destination pages, bit for bit.
  C1 logits    the row P sampled the first token from and every row D
               sampled from, against the dense fp64 forward of prompt +
               first token + D's tokens (teacher-forced).
  C2 cache     at D's last step, rows 0 .. num_tokens - 2 read through D's
               block table: rows below N were written by P's prefill.
  C3 poison    D: every slot D's decode never wrote equals the running
               expectation of C0 (D's poison, overlaid by every push in
               order: the tail of an imported page holds P's poison).  P:
               model_cases' C3 as it stands.
  C4 identity  D's prompt is the request's prompt, D's first appended token
               is the one P's recorder saw sampled for it, D's first decode
               step runs at num_tokens = N + 1, and P's row and D's rows
               together are positions N .. T - 1 once each.  Teacher
               forcing cannot see a wrong first token; C4 does.

The fp8 pair is judged with kvfp8_model_cases' reference and its
scenario-level statistic.
"""
from __future__ import annotations

import contextlib
import json
import math
import queue
import threading
import types
from typing import Callable, Dict, List, NamedTuple, Optional, Set, Tuple

import torch

import kvfp8_model_cases as m8
import model_cases as mc
from rbg_amd import ops
from rbg_amd.engine import pd_bench
from rbg_amd.engine import serve_worker as sw
from rbg_amd.engine.engine import LLMEngine
from rbg_amd.engine.sequence import FINISHED
from rbg_amd.parallel import kv_peer

BF16, FP8 = torch.bfloat16, torch.float8_e4m3fn
I16, I32, U8 = torch.int16, torch.int32, torch.uint8
PAGE = mc.PAGE


def raw(t: torch.Tensor) -> torch.Tensor:
    """The tensor's bytes as integers: int16 words of bf16, uint8 of e4m3."""
    return t.view(U8) if t.element_size() == 1 else t.view(I16)


# ---------------------------------------------------------------------------
# copy cases: kv_peer_copy alone
# ---------------------------------------------------------------------------

SRC_TAG, DST_TAG, GUARD_TAG = 0x5A000000, 0x3C000000, 0x11000000
DTYPES = {"bf16": BF16, "fp8": FP8}


def ramp(tag: int, chunks: int, pages: int, chunk_vec: int) -> torch.Tensor:
    """int32 [chunks, pages, chunk_vec, 4]: one 16-byte vector per row of
    four words (tag + chunk, page, vector index, ~tag).  Unique per vector
    and disjoint between tags."""
    out = torch.empty(chunks, pages, chunk_vec, 4, dtype=I32)
    out[..., 0] = tag + torch.arange(chunks, dtype=I32).view(-1, 1, 1)
    out[..., 1] = torch.arange(pages, dtype=I32).view(1, -1, 1)
    out[..., 2] = torch.arange(chunk_vec, dtype=I32).view(1, 1, -1)
    out[..., 3] = ~tag
    return out


def as_pool(words: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """[2L, P, chunk_vec, 4] int32 -> the same bytes as a KV pool
    [L, 2, P, 1, 1, hd] of `dtype` (hd = chunk_vec * 16 / element size)."""
    chunks, pages = words.shape[:2]
    return words.view(dtype).reshape(chunks // 2, 2, pages, 1, 1, -1)


class CopyCase(NamedTuple):
    chunk_vec: int
    layers: int
    ps: int             # source pool pages
    pd: int             # destination pool pages
    dtype: str
    kind: str           # identity | reversed | random | edges | dup_src
    n: int              # pages asked for; min(n, ps, pd) are pushed

    @property
    def id(self) -> str:
        return "cv%d-L%d-%dto%d-%s-%s-n%d" % self


CHUNK_VECS = (1, 63, 64, 65, 255, 256, 257, 300, 512, 2048)
POOL_PAGES = ((24, 40), (40, 24), (1, 1), (8, 8))
KINDS = ("identity", "reversed", "random", "edges", "dup_src")
FULL = 10 ** 6          # n = min(Ps, Pd)

# every value of every axis appears; not every combination.  Threads: 64
# below chunk_vec 256, 256 from there; 1 and 63 are tails below one pass of
# 64, 65 and 255 tails after full passes of 64, 257, 300 and 2048 the same
# for 256.
COPY_CASES = (
    CopyCase(1, 1, 24, 40, "bf16", "identity", 1),
    CopyCase(63, 2, 40, 24, "fp8", "reversed", 7),
    CopyCase(64, 3, 24, 40, "bf16", "random", FULL),
    CopyCase(65, 2, 8, 8, "fp8", "edges", 2),
    CopyCase(255, 1, 40, 24, "bf16", "edges", 7),
    CopyCase(256, 2, 24, 40, "fp8", "dup_src", 2),
    CopyCase(257, 3, 40, 24, "bf16", "random", FULL),
    CopyCase(300, 2, 1, 1, "bf16", "identity", 1),
    CopyCase(300, 1, 1, 1, "fp8", "edges", FULL),
    CopyCase(512, 3, 24, 40, "fp8", "edges", FULL),
    CopyCase(2048, 2, 40, 24, "bf16", "dup_src", 7),
    CopyCase(2048, 1, 8, 8, "fp8", "reversed", FULL),
    CopyCase(256, 3, 8, 8, "bf16", "random", 7),
    CopyCase(64, 2, 24, 40, "fp8", "reversed", FULL),
)


def page_lists(case: CopyCase) -> Tuple[List[int], List[int]]:
    ps, pd = case.ps, case.pd
    n = min(case.n, ps, pd)
    gen = torch.Generator().manual_seed(1000 + 7 * case.chunk_vec + n)

    def fill(head: List[int], pool: int) -> List[int]:
        head = list(dict.fromkeys(head))[:n]
        rest = [p for p in torch.randperm(pool, generator=gen).tolist()
                if p not in head]
        return head + rest[:n - len(head)]

    if case.kind == "identity":
        return list(range(n)), list(range(n))
    if case.kind == "reversed":         # from the bottom to the top, backwards
        return list(range(n)), [pd - 1 - i for i in range(n)]
    if case.kind == "random":
        return fill([], ps), fill([], pd)
    if case.kind == "edges":            # page 0 and the last page, each side
        return fill([0, ps - 1], ps), fill([pd - 1, 0], pd)
    if case.kind == "dup_src":          # one source page to two destinations
        src = fill([], ps)
        if n >= 2:
            src[1] = src[0]
        return src, fill([pd - 1], pd)
    raise ValueError(case.kind)


class CopySetup(NamedTuple):
    src_words: torch.Tensor     # int32 [2L, Ps, cv, 4], CPU
    alloc: torch.Tensor         # int32 [guard + 2L * Pd * cv + guard, 4], CPU
    guard_vec: int
    src_pages: List[int]
    dst_pages: List[int]
    expect: torch.Tensor        # alloc after a correct copy


def copy_setup(case: CopyCase) -> CopySetup:
    cv, chunks = case.chunk_vec, 2 * case.layers
    guard_vec = cv + 3                       # one chunk and an odd bit more
    src_words = ramp(SRC_TAG, chunks, case.ps, cv)
    body = ramp(DST_TAG, chunks, case.pd, cv).reshape(-1, 4)
    guard = ramp(GUARD_TAG, 1, 2, guard_vec)[0]
    alloc = torch.cat([guard[0], body, guard[1]])
    src_pages, dst_pages = page_lists(case)
    assert len(src_pages) == len(dst_pages) == min(case.n, case.ps, case.pd)
    assert len(set(dst_pages)) == len(dst_pages)
    expect = alloc.clone()
    mid = raw(as_pool(expect[guard_vec:guard_vec + body.shape[0]]
                      .view(chunks, case.pd, cv, 4), DTYPES[case.dtype]))
    assert mid.data_ptr() == expect[guard_vec].data_ptr()      # a view
    mid.index_copy_(
        2, torch.tensor(dst_pages, dtype=torch.long),
        raw(as_pool(src_words, DTYPES[case.dtype])).index_select(
            2, torch.tensor(src_pages, dtype=torch.long)))
    return CopySetup(src_words, alloc, guard_vec, src_pages, dst_pages,
                     expect)


def emulated_copy(alloc: torch.Tensor, guard_vec: int, src: torch.Tensor,
                  src_pages: List[int], dst_pages: List[int], pd: int,
                  dst_stride_pages: Optional[int] = None) -> None:
    """What the kernel computes, on the CPU with the kernel's own pointer
    arithmetic on flat 16-byte vectors (no index_copy_): block (i, chunk)
    copies chunk_vec vectors from chunk * Ps * cv + src[i] * cv to
    chunk * Pd * cv + dst[i] * cv.  `dst_stride_pages` replaces Pd in the
    destination chunk stride (the mutant).  A store outside the allocation,
    which the GPU would perform, raises here."""
    chunks, ps = src.shape[0] * 2, src.shape[2]
    flat = src.contiguous().view(-1).view(I32).view(-1, 4)
    cv = flat.shape[0] // (chunks * ps)
    stride = (pd if dst_stride_pages is None else dst_stride_pages) * cv
    for i, (sp, dp) in enumerate(zip(src_pages, dst_pages)):
        for chunk in range(chunks):
            s = chunk * ps * cv + sp * cv
            d = guard_vec + chunk * stride + dp * cv
            if d + cv > alloc.shape[0]:
                raise IndexError("store past the destination allocation")
            alloc[d:d + cv] = flat[s:s + cv]


def hip_copy(alloc: torch.Tensor, guard_vec: int, src: torch.Tensor,
             src_pages: List[int], dst_pages: List[int], pd: int) -> None:
    """The kernel itself; `alloc` and `src` are on the GPU."""
    dev = src.device
    ops._require_hip().kv_peer_copy(
        alloc.data_ptr() + 16 * guard_vec, src,
        torch.tensor(src_pages, dtype=I32, device=dev),
        torch.tensor(dst_pages, dtype=I32, device=dev), pd)
    torch.cuda.synchronize()


def run_copy_case(case: CopyCase, copy: Callable, device: str) -> List[str]:
    """Run `copy` on the case; the differences from the expectation."""
    su = copy_setup(case)
    src = as_pool(su.src_words.clone(), DTYPES[case.dtype]).to(device)
    alloc = su.alloc.clone().to(device)
    copy(alloc, su.guard_vec, src, su.src_pages, su.dst_pages, case.pd)
    out = []
    got = alloc.cpu()
    if not torch.equal(got, su.expect):
        bad = (got != su.expect).any(1).nonzero().flatten()
        body = su.expect.shape[0] - 2 * su.guard_vec
        where = ["guard before" if v < su.guard_vec else
                 "guard after" if v >= su.guard_vec + body else
                 "chunk %d page %d vec %d" % (
                     (v - su.guard_vec) // (case.pd * case.chunk_vec),
                     (v - su.guard_vec) // case.chunk_vec % case.pd,
                     (v - su.guard_vec) % case.chunk_vec)
                 for v in bad[:3].tolist()]
        out.append("destination: %d vectors differ, first %s" % (
            bad.numel(), where))
    if not torch.equal(src.cpu().view(-1).view(I32).view(-1, 4),
                       su.src_words.view(-1, 4)):
        out.append("source changed")
    return out


# ---------------------------------------------------------------------------
# pushes `PeerKVPusher.push` must refuse
# ---------------------------------------------------------------------------

def reject_cases(src_shape: List[int], meta: Dict) -> Dict[str, tuple]:
    """name -> (src_pages, dst_meta, dst_pages), each wrong in one way.
    `meta` describes a destination pool that differs from the source in the
    page count alone; both pools hold at least 8 pages."""
    ps, pd = src_shape[2], int(meta["num_pages"])
    assert meta["shape"][2] == pd and min(ps, pd) >= 8 and ps != pd

    def shape(axis, value):
        out = list(meta["shape"])
        out[axis] = value
        return dict(meta, shape=out)

    return {
        "unequal lengths": ([1, 2, 3], meta, [4, 5]),
        "source page == Ps": ([1, ps], meta, [4, 5]),
        "source page < 0": ([-1, 2], meta, [4, 5]),
        "destination page == num_pages": ([1, 2], meta, [4, pd]),
        "destination page < 0": ([1, 2], meta, [-1, 5]),
        "duplicate destination": ([1, 2, 3], meta, [4, 5, 4]),
        "other layer count": ([1], shape(0, src_shape[0] + 1), [4]),
        "no K|V axis": ([1], shape(1, 1), [4]),
        "other kv heads": ([1], shape(3, src_shape[3] + 1), [4]),
        "other page size": ([1], shape(4, 32), [4]),
        "other head_dim": ([1], shape(5, 64), [4]),
        "num_pages != shape[2]": ([1], dict(meta, num_pages=pd + 8), [4]),
        "num_pages 0": ([], dict(shape(2, 0), num_pages=0), []),
    }


# ---------------------------------------------------------------------------
# the digest of RBG_PD_VERIFY
# ---------------------------------------------------------------------------

def old_page_sum(cache, pages: List[int]) -> float:
    """What `pd_bench._page_checksum` was before the digest: kept here only
    to show what it accepts."""
    idx = torch.tensor(pages, dtype=torch.int64, device=cache.kv.device)
    return float(cache.kv.index_select(2, idx).double().sum().item())


# ---------------------------------------------------------------------------
# H1: the bench's own path
# ---------------------------------------------------------------------------

P_POOL, D_POOL = 2048, 1536
P_POISON_SEED, D_POISON_SEED = 7, 11
SCENARIOS = ("handoff", "trickle", "prefix")
HANDOFF_PROMPTS = (1, 15, 16, 17, 40, 100)
HANDOFF_NEW = 6


class Req:
    """One request across the handoff."""

    def __init__(self, prompt: List[int], d_new: int, p_seq,
                 src_pages: List[int], num_shared: int):
        self.prompt = list(prompt)
        self.d_new = d_new              # tokens D generates
        self.p_seq = p_seq
        self.src_pages = list(src_pages)
        self.num_shared = num_shared
        self.dst_pages: List[int] = []
        self.d_seq = None

    @property
    def n(self) -> int:
        return len(self.prompt)


def park_with_shared(engine: LLMEngine, parked: Dict) -> None:
    """The prefill role's parking (`ServeWorker.run`, mode=prefill): pages
    AND how many of them belong to the prefix cache."""
    sched = engine.scheduler
    orig = sched._retire_finished

    def retire_keep_pages():
        for s in list(sched.running):
            if s.should_stop() and s.block_table is not None:
                parked[s.seq_id] = (list(s.block_table.pages),
                                    s.block_table.num_shared)
                s.block_table.pages = []
                s.block_table.num_shared = 0
        orig()
    sched._retire_finished = retire_keep_pages


# the two places where H1 restates what `run_pd` does inline; mutants patch
# them
def _push_lists(reqs: List[Req]) -> Tuple[List[int], List[int]]:
    """ONE batched push: every source page and every destination page."""
    return ([p for r in reqs for p in r.src_pages],
            [p for r in reqs for p in r.dst_pages])


def _commit_entries(reqs: List[Req]) -> List[Tuple[List[int], int, List[int]]]:
    return [(r.p_seq.prompt_tokens, r.p_seq.output_tokens[0], lst)
            for r, lst in zip(reqs, [r.dst_pages for r in reqs])]


class Pair:
    def __init__(self, scenario: str, conf: str, device: str, d_eager: bool,
                 fp8: bool = False, d_fp8: Optional[bool] = None):
        self.scenario, self.conf, self.device = scenario, conf, device
        self.d_eager, self.fp8 = d_eager, fp8
        self.graph_mode = (not d_eager) and device != "cpu"
        prefix = scenario == "prefix"
        d_fp8 = fp8 if d_fp8 is None else d_fp8
        self.P = LLMEngine(mc.engine_config(
            conf, device, True, pool_tokens=P_POOL,
            enable_prefix_cache=prefix, **(m8.FP8_KW if fp8 else {})))
        self.D = LLMEngine(mc.engine_config(
            conf, device, d_eager, pool_tokens=D_POOL,
            enable_prefix_cache=False, **(m8.FP8_KW if d_fp8 else {})))
        for eng in (self.P, self.D):
            mc.draw_norm_weights(eng.runner.model)
        self.pc, self.dc = self.P.runner.cache, self.D.runner.cache
        assert (self.pc.num_pages, self.dc.num_pages) == (
            P_POOL // PAGE, D_POOL // PAGE)
        self.p_poison = (m8.poison_pool8 if fp8 else mc.poison_pool)(
            self.pc, seed=P_POISON_SEED)
        self.d_poison = (m8.poison_pool8 if d_fp8 else mc.poison_pool)(
            self.dc, seed=D_POISON_SEED)
        self.expect = self.d_poison.clone()      # D's unwritten slots
        self.parked: Dict = {}
        if prefix:
            park_with_shared(self.P, self.parked)
        else:
            pd_bench._park_finished_pages(self.P, self.parked)
        self.p_free0 = sorted(self.pc._free)
        self.migrator = pd_bench._Migrator(device)
        self.recP = mc.Recorder(self.P, conf)
        self.recD = mc.Recorder(self.D, conf)
        self.trace = mc.Trace()
        self.reqs: List[Req] = []
        self.c0: List[str] = []
        self.pushes = 0
        self.kernel_calls = 0
        self.extra: Dict = {}
        self.p_after = self.d_after = None

    @property
    def id(self) -> str:
        return "%s-%s-%s%s" % (self.scenario, self.conf,
                               "eager" if self.d_eager else "graph",
                               "-fp8" if self.fp8 else "")

    # -- P side --------------------------------------------------------------

    def prefill(self, prompts: List[List[int]], d_new: List[int]
                ) -> List[Req]:
        """One P prefill batch; the requests with their parked pages."""
        decodes = len(self.trace.decode)
        steps = self.P.stats.prefill_steps
        done = pd_bench._prefill_batch(self.P, prompts, self.parked)
        assert len(self.trace.decode) == decodes, "P decoded"
        assert self.P.stats.prefill_steps == steps + 1, "one prefill batch"
        out = []
        for (seq, parked), prompt, k in zip(done, prompts, d_new):
            pages, shared = (parked if isinstance(parked, tuple)
                             else (parked, 0))
            out.append(Req(prompt, k, seq, pages, shared))
        self.reqs += out
        return out

    def release(self, reqs: List[Req]) -> None:
        for r in reqs:
            if self.scenario == "prefix":
                sw.ServeWorker._release_parked(
                    types.SimpleNamespace(engine=self.P),
                    (r.src_pages, r.num_shared))
            else:
                self.pc.free(r.src_pages)          # as run_pd does

    # -- the handoff ---------------------------------------------------------

    def check_transfer(self, before: torch.Tensor, p_now: torch.Tensor,
                       reqs: List[Req], what: str) -> None:
        """C0, and the running expectation moves on."""
        src = torch.tensor([p for r in reqs for p in r.src_pages],
                           dtype=torch.long)
        dst = torch.tensor([p for r in reqs for p in r.dst_pages],
                           dtype=torch.long)
        moved = raw(p_now).index_select(2, src)
        raw(before).index_copy_(2, dst, moved)
        raw(self.expect).index_copy_(2, dst, moved)
        after = self.dc.kv.cpu()
        if not torch.equal(raw(after), raw(before)):
            diff = raw(after) != raw(before)
            pages = diff.transpose(0, 2).flatten(1).any(1)
            self.c0.append("%s: pages %s of D differ from the expectation"
                           % (what, pages.nonzero().flatten().tolist()[:12]))

    def migrate(self, reqs: List[Req]) -> None:
        """Allocate on D, ONE push for all of `reqs`, C0, enqueue on D,
        release on P."""
        for r in reqs:
            r.dst_pages = self.dc.alloc(len(r.src_pages))
        src_all, dst_all = _push_lists(reqs)
        before = self.dc.kv.cpu().clone()
        p_now = self.pc.kv.cpu()
        self.migrator.push_local(self.pc, self.dc, src_all, dst_all)
        self.pushes += 1
        self.check_transfer(before, p_now, reqs,
                            "push %d (%d pages)" % (self.pushes, len(src_all)))
        for r, (tokens, first, pages) in zip(reqs, _commit_entries(reqs)):
            r.d_seq = pd_bench._enqueue_imported(self.D, tokens, first,
                                                 pages, r.d_new + 1)
        self.release(reqs)

    # -- D side --------------------------------------------------------------

    def step_d(self, k: int = 1) -> None:
        prefills = len(self.trace.prefill)
        for _ in range(k):
            assert self.D.step() == "decode"
        assert len(self.trace.prefill) == prefills, "D prefilled"

    def drain_d(self) -> None:
        steps = 0
        while self.D.scheduler.has_work():
            self.step_d()
            steps += 1
            assert steps < 100

    def batches(self) -> List[Tuple[int, ...]]:
        """D's decode batches as request indices, repeats folded."""
        idx = {r.d_seq.seq_id: i for i, r in enumerate(self.reqs)
               if r.d_seq is not None}
        out: List[Tuple[int, ...]] = []
        for b in self.recD.decode_batches:
            b = tuple(idx[s] for s in b)
            if not out or out[-1] != b:
                out.append(b)
        return out


def _handoff(pair: Pair) -> None:
    prompts = mc._prompts(700, HANDOFF_PROMPTS)
    reqs = pair.prefill(prompts, [HANDOFF_NEW] * len(prompts))
    pair.migrate(reqs)
    pair.drain_d()


def _trickle(pair: Pair) -> None:
    pa, pb, pc, pd_ = mc._prompts(710, (20, 45, 9, 33))
    # three P batches up front: parked pages must outlive later prefills
    a, b = pair.prefill([pa, pb], [3, 8])
    (c,) = pair.prefill([pc], [5])
    (d,) = pair.prefill([pd_], [6])
    pair.migrate([a])
    pair.migrate([b])
    pair.step_d(2)
    pair.migrate([c])
    pair.step_d(1)
    retired = a.d_seq.status == FINISHED
    a_pages = list(pair.recD.seqs[a.d_seq.seq_id].pages) if \
        a.d_seq.seq_id in pair.recD.seqs else []
    pair.step_d(1)
    pair.migrate([d])
    pair.extra.update(a_retired=retired, a_pages=a_pages,
                      overlap=sorted(set(a_pages) & set(d.dst_pages)))
    pair.drain_d()


def _prefix(pair: Pair) -> None:
    base = mc._prompts(400, (50,))[0]
    tail = mc._prompts(401, (7,))[0]
    other = mc._prompts(402, (60,))[0]
    assert tail[0] != base[48]
    kv = pair.pc.kv
    (r0,) = pair.prefill([base], [4])
    shared = r0.src_pages[:3]
    before = raw(kv)[:, :, shared].cpu().clone()
    pair.migrate([r0])
    pair.step_d(1)
    freed = set(r0.src_pages[3:])
    (r1,) = pair.prefill([base[:48] + tail], [4])
    pair.migrate([r1])
    pair.step_d(1)
    freed |= set(r1.src_pages[3:])
    (r2,) = pair.prefill([other], [4])
    pair.migrate([r2])
    pair.step_d(1)
    (r3,) = pair.prefill([base], [4])
    identical = torch.equal(raw(kv)[:, :, shared].cpu(), before)
    pair.migrate([r3])
    pair.drain_d()
    pair.extra.update(
        shared=shared, identical=identical,
        cached=[r.p_seq.cached_prefix_len for r in (r0, r1, r2, r3)],
        num_shared=[r.num_shared for r in (r0, r1, r2, r3)],
        heads=[r.src_pages[:3] for r in (r1, r3)],
        reused=sorted(freed & set(r2.src_pages)))


_SCENARIO_FN = {"handoff": _handoff, "trickle": _trickle, "prefix": _prefix}


@contextlib.contextmanager
def _count_kernel(pair: Pair):
    if ops._hip is None:
        yield
        return
    orig = ops._hip.kv_peer_copy

    def counted(*a):
        pair.kernel_calls += 1
        return orig(*a)
    with mc._patched(ops._hip, "kv_peer_copy", counted):
        yield


def run_pair(scenario: str, conf: str, device: str, d_eager: bool,
             fp8: bool = False, mutant: Optional[str] = None) -> Pair:
    pair = Pair(scenario, conf, device, d_eager, fp8)
    stack = contextlib.ExitStack()
    with stack:
        if fp8:
            gather = mc.gather_rows
            stack.enter_context(mc._patched(
                mc, "gather_rows",
                lambda kv, pages, count: gather(kv.view(U8), pages, count)))
        if mutant is not None:
            stack.enter_context(MUTANTS[mutant].make(pair))
        for cm in (_count_kernel(pair), pair.trace, pair.recP, pair.recD):
            stack.enter_context(cm)
        _SCENARIO_FN[scenario](pair)
    pair.p_after = pair.pc.kv.cpu().clone()
    pair.d_after = pair.dc.kv.cpu().clone()
    return pair


def assert_same_weights(pair: Pair) -> None:
    a = mc.snapshot_params(pair.P.runner.model)
    b = mc.snapshot_params(pair.D.runner.model)
    assert len(a) == len(b) and all(
        torch.equal(raw(x), raw(y)) for x, y in zip(a, b))
    assert torch.equal(pair.P.runner.model.cos_sin.cpu(),
                       pair.D.runner.model.cos_sin.cpu())
    assert not torch.equal(raw(pair.p_poison)[:, :, :D_POOL // PAGE],
                           raw(pair.d_poison))


def assert_paths(pair: Pair) -> None:
    """The path a scenario is meant to reach actually ran (clean runs)."""
    gpu = pair.device != "cpu"
    P, D, recP, recD = pair.P, pair.D, pair.recP, pair.recD
    assert recP.decode_batches == [] and P.stats.decode_steps == 0
    assert D.stats.prefill_steps == 0
    assert len(pair.trace.prefill) == (P.stats.prefill_steps *
                                       P.cfg.model.num_layers)
    assert pair.kernel_calls == (pair.pushes if gpu else 0)
    assert pair.pc.kv.is_cuda == pair.dc.kv.is_cuda == gpu
    sizes = {len(b) for b in recD.decode_batches}
    if pair.graph_mode:
        assert recD.graph_replays == len(recD.decode_batches) > 0
    else:
        assert recD.graph_replays == 0 and not D.runner._graphs
    assert all(r.d_seq.status == FINISHED and
               len(r.d_seq.output_tokens) == r.d_new + 1 for r in pair.reqs)
    # every parked page is back in P's pool, each once
    if pair.scenario != "prefix":
        assert sorted(pair.pc._free) == pair.p_free0
    if pair.scenario == "handoff":
        assert [r.n for r in pair.reqs] == list(HANDOFF_PROMPTS)
        assert P.stats.prefill_steps == 1 and pair.pushes == 1
        assert sizes == {6} and len(recD.decode_batches) == HANDOFF_NEW
        # prompt 16: a second parked page that no token ever touched
        r16 = pair.reqs[2]
        assert len(r16.src_pages) == 2
        assert [len(r.src_pages) for r in pair.reqs] == [1, 1, 2, 2, 3, 7]
        if pair.graph_mode:
            assert set(D.runner._graphs) == {8}
    elif pair.scenario == "trickle":
        assert P.stats.prefill_steps == 3 and pair.pushes == 4
        assert pair.batches() == [(0, 1), (0, 1, 2), (1, 2), (1, 2, 3),
                                  (1, 3), (3,)], pair.batches()
        assert pair.extra["a_retired"] and pair.extra["overlap"], pair.extra
        if pair.graph_mode:
            assert set(D.runner._graphs) == {1, 2, 4}
    elif pair.scenario == "prefix":
        x = pair.extra
        assert P.runner.cache.prefix.hits > 0
        assert x["cached"] == [0, 48, 0, 48], x
        assert x["num_shared"] == [3, 3, 3, 3], x
        assert x["heads"] == [x["shared"]] * 2, x
        assert x["reused"], "the unrelated prompt reused no freed page"
        assert x["identical"], "shared pages changed while parked in the cache"
        free = pair.pc._free
        assert len(set(free)) == len(free)
        assert not set(free) & set(pair.pc.prefix.page_info)


# ---------------------------------------------------------------------------
# the judge
# ---------------------------------------------------------------------------

class PairVerdict(NamedTuple):
    c0: List[str]
    c1: List[Tuple[str, float, float]]
    c2: List[Tuple[str, float, float]]
    c3: List[str]
    c4: List[str]

    def failures(self) -> List[str]:
        out = ["C0 " + v for v in self.c0]
        out += ["C1 %s: err %.4g > %g * e_cpu %.4g" % (w, e, mc.FACTOR, y)
                for w, e, y in self.c1 if not e <= mc.FACTOR * y]
        out += ["C2 %s: err %.4g > %g * e_cpu %.4g" % (w, e, mc.FACTOR, y)
                for w, e, y in self.c2 if not e <= mc.FACTOR * y]
        return (out + ["C3 " + v for v in self.c3] +
                ["C4 " + v for v in self.c4])

    def failed_checks(self) -> Set[str]:
        out = set()
        for name, rows in (("C1", self.c1), ("C2", self.c2)):
            if any(not e <= mc.FACTOR * y for _, e, y in rows):
                out.add(name)
        for name, rows in (("C0", self.c0), ("C3", self.c3), ("C4", self.c4)):
            if rows:
                out.add(name)
        return out

    def worst(self) -> Tuple[float, float]:
        def ratio(rows):
            return max((e / y if y > 0 else (0.0 if e == 0 else math.inf))
                       for _, e, y in rows)
        return ratio(self.c1), ratio(self.c2)


def d_written_mask(pair) -> torch.Tensor:
    """The slots D's own decode wrote: positions N .. final_count - 1 of
    each D sequence through its block table."""
    mask = torch.zeros(pair.dc.num_pages, PAGE, dtype=torch.bool)
    for rec in pair.recD.seqs.values():
        for pos in range(rec.seq.num_prompt_tokens, rec.final_count):
            mask[rec.pages[pos // PAGE], pos % PAGE] = True
    return mask


def judge_pair(pair) -> PairVerdict:
    """C0 to C4 for a finished run of H1 or H2.  Called outside any mutant:
    the reference and the yardstick run the unmodified project code.  Never
    raises on a wrong handoff; what is wrong is in the verdict."""
    fp8 = pair.fp8
    model = mc.cpu_model(pair.conf, pair.recP.weights[0],
                         pair.P.runner.model.cos_sin)
    forward64 = m8.dense_forward64_q8 if fp8 else mc.dense_forward64
    cpu_fwd = (lambda t: m8.cpu_forward8(model, pair.conf, t)) if fp8 else \
        (lambda t: mc.cpu_forward(model, pair.conf, t))
    c1, c2, c4 = [], [], []
    sums: Dict[str, List[float]] = {}

    def add(what, got, cpu, ref):
        acc = sums.setdefault(what, [0.0, 0.0, 0.0])
        acc[0] += float((got.double() - ref).pow(2).sum())
        acc[1] += float((cpu.double() - ref).pow(2).sum())
        acc[2] += float(ref.pow(2).sum())

    for i, r in enumerate(pair.reqs):
        who = "req %d (prompt %d)" % (i, r.n)
        p_rec = pair.recP.seqs.get(r.p_seq.seq_id)
        d_rec = pair.recD.seqs.get(r.d_seq.seq_id) if r.d_seq else None
        if p_rec is None or d_rec is None:
            c4.append("%s: never sampled on %s" % (
                who, "P" if p_rec is None else "D"))
            continue
        d_seq = r.d_seq
        n = r.n
        # C4
        if d_seq.prompt_tokens != r.prompt:
            c4.append("%s: D holds another prompt" % who)
        if len(p_rec.sampled) != 1 or \
                d_seq.output_tokens[:1] != p_rec.sampled:
            c4.append("%s: D's first token %s, P sampled %s" % (
                who, d_seq.output_tokens[:1], p_rec.sampled))
        if d_rec.rows[0][0] != n + 1:
            c4.append("%s: D's first decode step at num_tokens %d, not %d"
                      % (who, d_rec.rows[0][0], n + 1))
        tokens = d_seq.prompt_tokens + d_seq.output_tokens
        T = len(tokens)
        rows = p_rec.rows + d_rec.rows
        if [nt for nt, _ in rows] != list(range(n, T)) or T != n + r.d_new + 1:
            c4.append("%s: rows at %s, expected %d .. %d" % (
                who, [nt for nt, _ in rows], n, n + r.d_new))
        if d_rec.final_kv is None or d_rec.final_count != T - 1:
            c4.append("%s: D's cache read at %s rows, expected %d" % (
                who, d_rec.final_count, T - 1))
        # C1, C2
        ref_logits, ref_kv = forward64(model, tokens)
        cpu_logits, cpu_kv = cpu_fwd(tokens)
        rows = [(nt, row) for nt, row in rows if 1 <= nt <= T]
        count = min(d_rec.final_count, T) if d_rec.final_kv is not None else 0
        got_kv = d_rec.final_kv[:count] if count else None
        if fp8:
            pos = [nt - 1 for nt, _ in rows]
            add("logits", torch.stack([row for _, row in rows]),
                cpu_logits[pos], ref_logits[pos])
            if count:
                got_kv = m8.dequant_rows(got_kv.view(FP8))
        else:
            e_logits = max(mc.rel_l2(cpu_logits[t], ref_logits[t])
                           for t in range(T))
            for nt, row in rows:
                c1.append(("%s row %d" % (who, nt),
                           mc.rel_l2(row, ref_logits[nt - 1]), e_logits))
        for layer in range(ref_kv.shape[1]):
            for j, name in enumerate("KV"):
                if not count:
                    continue
                got, cpu, ref = (got_kv[:, layer, j], cpu_kv[:count, layer, j],
                                 ref_kv[:count, layer, j])
                if fp8:
                    add("layer %d %s" % (layer, name), got, cpu, ref)
                else:
                    c2.append(("%s layer %d %s" % (who, layer, name),
                               mc.rel_l2(got, ref), mc.rel_l2(cpu, ref)))
    if fp8:
        stats = [(what, math.sqrt(a / r), math.sqrt(c / r))
                 for what, (a, c, r) in sums.items()]
        c1 = [s for s in stats if s[0] == "logits"]
        c2 = [s for s in stats if s[0] != "logits"]
    c3 = ["D " + v for v in mc.poison_violations(
        pair.d_after, pair.expect, d_written_mask(pair), pair.recD.owned,
        pair.graph_mode)]
    c3 += ["P " + v for v in mc.poison_violations(
        pair.p_after, pair.p_poison, pair.recP.written_mask(),
        pair.recP.owned, False)]
    return PairVerdict(list(pair.c0), c1, c2, c3, c4)


# ---------------------------------------------------------------------------
# mutants: wrong handoffs, used only by the CPU self-test
# ---------------------------------------------------------------------------

def _wrong_push(copy: Callable) -> contextlib.AbstractContextManager:
    """Replace the CPU branch of `_Migrator.push_local` by `copy(src_kv,
    dst_kv, src_idx, dst_idx)` on the pools' raw views."""
    def push_local(self, src_cache, dst_cache, src_pages, dst_pages):
        copy(raw(src_cache.kv), raw(dst_cache.kv),
             torch.tensor(src_pages, dtype=torch.long),
             torch.tensor(dst_pages, dtype=torch.long))
    return mc._patched(pd_bench._Migrator, "push_local", push_local)


def _mut_reversed_dst(pair):
    return _wrong_push(lambda s, d, si, di: d.index_copy_(
        2, di.flip(0), s.index_select(2, si)))


def _mut_kv_swapped(pair):
    return _wrong_push(lambda s, d, si, di: d.index_copy_(
        2, di, s.index_select(2, si).flip(1)))


def _mut_layer0_only(pair):
    return _wrong_push(lambda s, d, si, di: d[:1].index_copy_(
        2, di, s[:1].index_select(2, si)))


def _mut_layer_xor_1(pair):
    def copy(s, d, si, di):
        for layer in range(s.shape[0]):
            d[layer ^ 1].index_copy_(1, di, s[layer].index_select(1, si))
    return _wrong_push(copy)


def _mut_src_chunk_stride(pair):
    """The destination chunk stride taken from the source pool's page
    count, with the kernel's flat arithmetic.  Stores past D's pool, which
    the GPU would perform, are dropped."""
    def copy(s, d, si, di):
        chunks, ps = s.shape[0] * 2, s.shape[2]
        sflat = s.reshape(chunks * ps, -1)
        dflat = d.view(-1, sflat.shape[1])
        for chunk in range(chunks):
            for sp, dp in zip(si.tolist(), di.tolist()):
                row = chunk * ps + dp
                if row < dflat.shape[0]:
                    dflat[row] = sflat[chunk * ps + sp]
    return _wrong_push(copy)


def _patch_here(name: str, fn) -> contextlib.AbstractContextManager:
    import sys
    return mc._patched(sys.modules[__name__], name, fn)


def _mut_drop_last_page(pair):
    return _patch_here("_push_lists", lambda reqs: (
        [p for r in reqs for p in r.src_pages[:-1]],
        [p for r in reqs for p in r.dst_pages[:-1]]))


def _mut_prompt_pages_only(pair):
    def lists(reqs):
        keep = [(r.n + PAGE - 1) // PAGE for r in reqs]
        return ([p for r, k in zip(reqs, keep) for p in r.src_pages[:k]],
                [p for r, k in zip(reqs, keep) for p in r.dst_pages[:k]])
    return _patch_here("_push_lists", lists)


def _mut_first_tokens_rotated(pair):
    def entries(reqs):
        firsts = [r.p_seq.output_tokens[0] for r in reqs]
        firsts = firsts[1:] + firsts[:1]
        return [(r.p_seq.prompt_tokens, f, r.dst_pages)
                for r, f in zip(reqs, firsts)]
    return _patch_here("_commit_entries", entries)


def _mut_no_first_token(pair):
    orig = pd_bench._enqueue_imported

    def enqueue(engine, tokens, first_token, pages, max_new):
        seq = orig(engine, tokens, first_token, pages, max_new)
        seq.output_tokens.pop()
        return seq
    return mc._patched(pd_bench, "_enqueue_imported", enqueue)


def _mut_free_before_push(pair):
    orig = pd_bench._prefill_batch

    def prefill_batch(engine, prompts, parked):
        done = orig(engine, prompts, parked)
        for _s, pages in done:
            engine.runner.cache.free(
                pages[0] if isinstance(pages, tuple) else pages)
        return done
    return mc._patched(pd_bench, "_prefill_batch", prefill_batch)


def _mut_free_shared(pair):
    def release(self, parked):
        self.engine.runner.cache.free(parked[0])
    return mc._patched(sw.ServeWorker, "_release_parked", release)


class Mutant(NamedTuple):
    make: Callable                       # pair -> context manager
    what: str
    applies: Tuple[str, ...]             # scenarios that have what it breaks


# "applies" is decided from the scenario alone.  first_tokens_rotated needs
# a commit list of two or more (handoff); free_before_push needs a P batch
# between a prefill and its push (trickle); free_shared needs shared pages
# (prefix); prompt_pages_only needs a prompt that is a multiple of the page
# size, so that prompt + first token opens a page the prompt does not
# (handoff's 16)
MUTANTS: Dict[str, Mutant] = {
    "reversed_dst": Mutant(
        _mut_reversed_dst,
        "destination pages written in reversed order", SCENARIOS),
    "drop_last_page": Mutant(
        _mut_drop_last_page, "last parked page of a sequence not pushed",
        SCENARIOS),
    "kv_swapped": Mutant(_mut_kv_swapped, "K and V planes swapped",
                         SCENARIOS),
    "layer0_only": Mutant(_mut_layer0_only, "only layer 0 pushed",
                          SCENARIOS),
    "layer_xor_1": Mutant(_mut_layer_xor_1, "layer l written to layer l^1",
                          SCENARIOS),
    "src_chunk_stride": Mutant(
        _mut_src_chunk_stride,
        "destination chunk stride from the source pool's page count",
        SCENARIOS),
    "first_tokens_rotated": Mutant(
        _mut_first_tokens_rotated,
        "first tokens rotated by one sequence in the commit list",
        ("handoff",)),
    "no_first_token": Mutant(
        _mut_no_first_token, "_enqueue_imported not appending the first token",
        SCENARIOS),
    "free_before_push": Mutant(
        _mut_free_before_push,
        "P's pages freed and reused by the next prefill batch before the push",
        ("trickle",)),
    "free_shared": Mutant(
        _mut_free_shared,
        "every parked page freed to the free list regardless of num_shared",
        ("prefix",)),
    "prompt_pages_only": Mutant(
        _mut_prompt_pages_only,
        "pushed pages limited to ceil(N/16) when the block table holds more",
        ("handoff",)),
}


def differs(a: Pair, b: Pair) -> bool:
    """Did the mutant change anything a correct handoff determines: either
    pool's bytes or any token or recorded row of D?"""
    if not torch.equal(raw(a.d_after), raw(b.d_after)) or \
            not torch.equal(raw(a.p_after), raw(b.p_after)):
        return True
    for ra, rb in zip(a.reqs, b.reqs):
        if ra.d_seq.output_tokens != rb.d_seq.output_tokens:
            return True
        ka = a.recD.seqs.get(ra.d_seq.seq_id)
        kb = b.recD.seqs.get(rb.d_seq.seq_id)
        if ka is None or kb is None or \
                [n for n, _ in ka.rows] != [n for n, _ in kb.rows]:
            return True
    return False


# ---------------------------------------------------------------------------
# H2: the serving handshake
# ---------------------------------------------------------------------------

H2_PROMPTS = (17, 40, 100)
H2_NEW = 5


class _Wire:
    """torch.distributed.send / recv between the two workers of one
    process."""

    def __init__(self):
        self.q: "queue.Queue[torch.Tensor]" = queue.Queue()
        self.sent: List[Tuple[torch.dtype, Tuple[int, ...]]] = []

    def send(self, tensor, dst, *a, **kw):
        self.sent.append((tensor.dtype, tuple(tensor.shape)))
        self.q.put(tensor.detach().cpu().clone())

    def recv(self, tensor, src=None, *a, **kw):
        got = self.q.get(timeout=60)
        assert got.dtype == tensor.dtype and got.shape == tensor.shape
        tensor.copy_(got)


class _Threads:
    """Stands in for the `threading` module inside serve_worker so the
    receive thread `_rpc_import_seq` starts can be joined."""

    Lock, Event = threading.Lock, threading.Event

    def __init__(self):
        self.started: List[threading.Thread] = []

    def Thread(self, target=None, daemon=None):
        t = threading.Thread(target=target, daemon=daemon)
        self.started.append(t)
        return t

    def join_all(self) -> None:
        for t in self.started:
            t.join(60)
            assert not t.is_alive(), "receive thread still running"
        self.started.clear()


def _bind(ns, *names) -> None:
    for name in names:
        setattr(ns, name, types.MethodType(getattr(sw.ServeWorker, name), ns))


class Serving(Pair):
    """H2.  `reqs`, the recorders, `expect` and the pools are Pair's, so
    judge_pair applies unchanged."""

    def __init__(self, conf: str, device: str, d_eager: bool):
        super().__init__("serving", conf, device, d_eager)
        # the prefill role parks (pages, num_shared): undo Pair's parking
        del self.P.scheduler._retire_finished
        self.parked_log: Dict[int, List[int]] = {}
        self.rpc_log: List[Tuple[str, dict, dict]] = []
        self.wire = _Wire()
        self.threads = _Threads()
        gcomm = types.SimpleNamespace(backend="gloo")
        pw = self.pw = types.SimpleNamespace(
            tp=None, engine=self.P, results={}, gcomm=gcomm,
            my_instance="p-0", _finished_pages={}, _peer_pusher=None,
            _xfer_lock=threading.Lock(),
            _xfer_stats={"pushes": 0, "bytes": 0, "seconds": 0.0},
            _decode_port=lambda inst: 1, _peer_rank=lambda inst: 1)
        park_with_shared(self.P, pw._finished_pages)
        _bind(pw, "_peer_possible", "_peer_push", "_release_parked",
              "_send_pages", "_xfer_buf_device")

        def poll(seq_id):
            # stands in for the prefill role's engine loop
            while self.P.scheduler.has_work():
                assert self.P.step() == "prefill"
            self.parked_log[seq_id] = list(pw._finished_pages[seq_id][0])
            return sw.ServeWorker._rpc_poll(pw, seq_id)
        pw._rpc_poll = poll
        dw = self.dw = types.SimpleNamespace(
            tp=None, engine=self.D, results={}, gcomm=gcomm,
            my_instance="d-0", _pending_imports={}, lock=threading.Lock(),
            _pause=threading.Event(), _xfer_lock=threading.Lock(),
            _peer_rank=lambda inst: 0)
        _bind(dw, "_peer_possible", "_import_alloc", "_import_finish",
              "_import_enqueue", "_recv_pages", "_xfer_buf_device")
        serving = self

        class Client:
            def __init__(self, host, port):
                pass

            def call(self, method, **params):
                params = json.loads(json.dumps(params))
                fn = getattr(sw.ServeWorker, "_rpc_" + method)
                reply = json.loads(json.dumps(fn(dw, **params)))
                serving.rpc_log.append((method, params, reply))
                return reply

            def close(self):
                pass
        self.client = Client

    def handoff(self, prompt: List[int], d_new: int) -> Req:
        """One request through `_rpc_prefill`; C0 on what arrived."""
        import torch.distributed as dist
        before = self.dc.kv.cpu().clone()
        calls = len(self.rpc_log)
        stack = contextlib.ExitStack()
        with stack:
            for obj, name, value in (
                    (sw, "RpcClient", self.client),
                    (sw, "threading", self.threads),
                    (dist, "send", self.wire.send),
                    (dist, "recv", self.wire.recv),
                    (kv_peer, "export_meta", kv_peer.export_meta_local)):
                stack.enter_context(mc._patched(obj, name, value))
            decodes = len(self.trace.decode)
            out = sw.ServeWorker._rpc_prefill(
                self.pw, list(prompt), d_new + 1, "d-0")
            self.threads.join_all()
            assert len(self.trace.decode) == decodes, "P decoded"
        if self.device != "cpu":
            torch.cuda.synchronize()
        (method, params, reply) = self.rpc_log[calls]
        assert method == "import_seq"
        d_seq = self.dw.results[reply["seq_id"]]
        p_seq = next(s for s in self.pw.results.values()
                     if s.prompt_tokens == list(prompt) and
                     s.seq_id in self.parked_log and
                     all(s is not r.p_seq for r in self.reqs))
        r = Req(prompt, d_new, p_seq, self.parked_log[p_seq.seq_id], 0)
        r.dst_pages = list(d_seq.block_table.pages[:params["num_pages"]])
        r.d_seq = d_seq
        self.reqs.append(r)
        self.pushes += 1
        self.extra.setdefault("replies", []).append(out)
        # P's pages are released already, but nothing ran on P since
        self.check_transfer(before, self.pc.kv.cpu(), [r],
                            "handoff %d" % self.pushes)
        return r


def run_serving(conf: str, device: str, d_eager: bool) -> Serving:
    s = Serving(conf, device, d_eager)
    with _count_kernel(s), s.trace, s.recP, s.recD:
        for prompt in mc._prompts(720, H2_PROMPTS):
            s.handoff(prompt, H2_NEW)
            s.step_d(2)
        s.drain_d()
    s.p_after = s.pc.kv.cpu().clone()
    s.d_after = s.dc.kv.cpu().clone()
    return s


def assert_serving_paths(s: Serving) -> None:
    gpu = s.device != "cpu"
    assert s.recP.decode_batches == [] and s.D.stats.prefill_steps == 0
    assert s.P.stats.prefill_steps == len(H2_PROMPTS)
    methods = [m for m, _p, _r in s.rpc_log]
    chunk = s.pc.kv[:, :, 0].numel() * s.pc.kv.element_size()
    pages = sum(len(r.src_pages) for r in s.reqs)
    assert [len(r.src_pages) for r in s.reqs] == [2, 3, 7]
    if gpu:
        # the peer branch: the kernel moved every page, nothing on the wire
        assert methods == ["import_seq", "import_commit"] * len(H2_PROMPTS)
        assert s.kernel_calls == len(H2_PROMPTS) and not s.wire.sent
        assert s.pw._xfer_stats["pushes"] == len(H2_PROMPTS)
        assert s.pw._xfer_stats["bytes"] == pages * chunk
        assert all(rep["peer"] is not None for m, _p, rep in s.rpc_log
                   if m == "import_seq")
        assert not s.dw._pending_imports
    else:
        # declined: to_wire / from_wire over the (in-memory) collective
        assert methods == ["import_seq"] * len(H2_PROMPTS)
        assert s.kernel_calls == 0
        m = s.pc.kv.shape
        assert s.wire.sent == [
            (I16, (m[0], 2, len(r.src_pages), m[3], m[4], m[5]))
            for r in s.reqs]
    for r, rep in zip(s.reqs, s.extra["replies"]):
        assert rep["decode_seq_id"] == r.d_seq.seq_id
        assert rep["first_token"] == r.p_seq.output_tokens[0]
        assert r.d_seq.status == FINISHED
        assert len(r.d_seq.output_tokens) == H2_NEW + 1
    assert s.batches() == [(0,), (0, 1), (0, 1, 2), (1, 2), (2,)], s.batches()
    if s.graph_mode:
        assert set(s.D.runner._graphs) == {1, 2, 4}
        assert s.recD.graph_replays == len(s.recD.decode_batches)
    # P's parked pages are all back, each once
    assert not s.pw._finished_pages
    assert sorted(s.pc._free) == s.p_free0
    assert s.pc.free_pages == s.pc.num_pages - 1
