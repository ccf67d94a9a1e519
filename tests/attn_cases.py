"""Shared inputs, references and checks for the attention conformance tests.

A plain helper module (not a conftest): tests/test_attn_cases_cpu.py proves
on the CPU that the checks accept a correct kernel (an fp64 reference and a
bf16-faithful emulation) and reject wrong ones (the mutants), and
tests/test_attention_conformance_gpu.py runs the same cases and the same
checks against the HIP kernels.

Three input families, each for decode and prefill:

  needle  K is random +-1, V comes from {x/8}, and q = 8 * K[target].  At
          scale 0.088 the target's score is 0.704 * 128 = 90.1 and every
          other key's is 0.704 * (a +-1 dot product, sigma 11.3): typically
          a lead above 60, and the builder asserts (else redraws) a lead
          above NEEDLE_GAP = 40 over the 10^5 (row, key) pairs of a batch.
          All other keys together then weigh < 2047 * e^-40 < 1e-14, far
          under half a bf16 ulp (2^-9 relative) of any |v| >= 1/8, and
          under half an fp32 ulp of l = 1.  The output must EQUAL V[target]
          bit for bit: no tolerance.
  prob    q, K are randn and V is one-hot, so the output is the softmax row
          itself (aliased by residue).  Bound: TOL * p, and exactly 0 where
          the reference is exactly 0.
  scaled  q, K, V are randn.  Bound per element: TOL * A + 1e-6 with
          A = sum_i p_i |v_i|, i.e. relative to the signal, not a constant.

TOL = 2^-7 + 2^-12: P and the output are each rounded to bf16 once (round
to nearest, relative error <= 2^-8 each); 2^-12 covers fp32 accumulation
and the fast exp.
"""
from __future__ import annotations

import functools
from typing import Callable, Dict, List, NamedTuple, Optional, Tuple

import torch

D = 128
PAGE = 16
SCALE = 0.088
TOL = 2.0 ** -7 + 2.0 ** -12
ABS_FLOOR = 1e-6            # family "scaled" only
V_POISON = 32768.0
K_POISON = 4.0
NEEDLE_GAP = 40.0
BF16 = torch.bfloat16

DECODE_VARIANTS = (0, 1, 2, 3, 4, 5, 6)
DECODE_SPLITS = (1, 2, 3, 4, 16)
DECODE_CTXS = (1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 80, 100, 257, 530, 2047)
DECODE_FAMILIES = ("needle", "prob_key", "prob_page", "scaled")

PREFILL_SWZ = tuple(range(12))
PREFILL_HEADS = ((8, 8), (8, 2), (16, 4), (32, 8), (16, 2))   # (QH, KVH)
# (Lk, Lq) per sequence; Lk == Lq means no cached prefix
PREFILL_LENS = (
    ((1, 1),),
    ((63, 63), (65, 65)),
    ((127, 127), (129, 129), (1, 1)),
    ((64, 64), (64, 64), (64, 64)),
    ((200, 200),),
    ((130, 1),),
    ((129, 64),),
    ((64, 64),),
    ((200, 7),),
    ((192, 160),),
)
PREFILL_FAMILIES = ("needle", "prob", "scaled")


# ---------------------------------------------------------------------------
# fp64 references (same signatures as rbg_amd.ops.reference, float64 out)
# ---------------------------------------------------------------------------

def _split_range(ctx: int, splits: int, split: int) -> Tuple[int, int]:
    """Key range of one split, as every decode kernel computes it."""
    nchunks = (ctx + 15) // 16
    per_split = (nchunks + splits - 1) // splits
    return split * per_split * 16, min(ctx, (split + 1) * per_split * 16)


def _decode_keys(ctx: int, mut: Optional[str]):
    """Logical key indices a (possibly mutated) decode attends, and the
    block-table column each is read through."""
    idx = torch.arange(ctx)
    if mut == "leak_key":
        idx = torch.arange(ctx + 1)
    elif mut == "drop_last" and ctx > 1:
        idx = torch.arange(ctx - 1)
    npages = (ctx + PAGE - 1) // PAGE
    if mut == "drop_page" and npages >= 2:
        idx = idx[idx // PAGE != npages // 2]
    if mut is not None and mut.startswith("drop_split@"):
        splits = int(mut.split("@")[1])
        live = [s for s in range(splits)
                if _split_range(ctx, splits, s)[0] < ctx]
        b, e = _split_range(ctx, splits, live[len(live) // 2])
        idx = idx[(idx < b) | (idx >= e)]
    cols = idx // PAGE
    if mut == "wrong_page":
        j = npages // 2
        wrong = (j + 1) % npages if npages >= 2 else npages
        cols = torch.where(cols == j, torch.full_like(cols, wrong), cols)
    return idx, cols


def _decode64(q, key_cache, value_cache, block_tables, context_lens, scale,
              mut: Optional[str] = None, absv: bool = False) -> torch.Tensor:
    S, QH, Dh = q.shape
    kvh = key_cache.shape[1]
    page = key_cache.shape[2]
    qpg = QH // kvh
    out = torch.zeros(S, QH, Dh, dtype=torch.float64)
    for s in range(S):
        ctx = int(context_lens[s])
        if ctx == 0:
            continue
        idx, cols = _decode_keys(ctx, mut)
        if idx.numel() == 0:
            continue
        pages = block_tables[s, cols].long()
        k = key_cache[pages, :, idx % page].double()      # [n, KVH, D]
        v = value_cache[pages, :, idx % page].double()
        if mut == "wrong_kv_head":
            k, v = k.roll(-1, dims=1), v.roll(-1, dims=1)
        if absv:
            v = v.abs()
        qs = q[s].double().view(kvh, qpg, Dh)
        p = torch.softmax(torch.einsum("hgd,nhd->hgn", qs, k) * scale, -1)
        o = torch.einsum("hgn,nhd->hgd", p, v)
        if mut == "swap_heads" and qpg >= 2:
            o = o[:, [1, 0] + list(range(2, qpg))]
        out[s] = o.reshape(QH, Dh)
    return out


def decode_ref64(q, key_cache, value_cache, block_tables, context_lens,
                 scale) -> torch.Tensor:
    """Paged decode attention in float64, unrounded.  A row with
    context_lens == 0 is all zeros."""
    return _decode64(q, key_cache, value_cache, block_tables, context_lens,
                     scale)


def _prefill64(q, k, v, cu_seqlens, scale, cu_seqlens_k=None,
               mut: Optional[str] = None) -> torch.Tensor:
    Tq, QH, Dh = q.shape
    kvh = k.shape[1]
    qpg = QH // kvh
    out = torch.zeros(Tq, QH, Dh, dtype=torch.float64)
    cu = [int(x) for x in cu_seqlens]
    cuk = [int(x) for x in cu_seqlens_k] if cu_seqlens_k is not None else cu
    nseq = len(cu) - 1
    for b in range(nseq):
        s, e, sk, ek = cu[b], cu[b + 1], cuk[b], cuk[b + 1]
        Lq, Lk = e - s, ek - sk
        off = 0 if mut == "no_prefix" else Lk - Lq
        ek_read = ek
        if mut == "next_seq" and b + 1 < nseq:
            ek_read = ek + 1              # first key of the next sequence
        ks = k[sk:ek_read].double()
        vs = v[sk:ek_read].double()
        qs = q[s:e].double().view(Lq, kvh, qpg, Dh)
        sc = torch.einsum("qhgd,khd->hgqk", qs, ks) * scale
        qpos = torch.arange(off, off + Lq).unsqueeze(1)
        kpos = torch.arange(ek_read - sk).unsqueeze(0)
        if mut == "future":
            masked = (kpos > qpos + 1) | (kpos >= Lk)
        elif mut == "next_seq":
            masked = (kpos > qpos) & (kpos < Lk)
        else:
            masked = kpos > qpos
        sc = sc.masked_fill(masked, float("-inf"))
        p = torch.softmax(sc, -1)
        out[s:e] = torch.einsum("hgqk,khd->qhgd", p, vs).reshape(Lq, QH, Dh)
    return out


def prefill_ref64(q, k, v, cu_seqlens, scale,
                  cu_seqlens_k=None) -> torch.Tensor:
    """Varlen causal attention in float64, unrounded."""
    return _prefill64(q, k, v, cu_seqlens, scale, cu_seqlens_k)


def attn_abs64(ref: Callable, q, k, v, *rest, **kw) -> torch.Tensor:
    """A = sum_i p_i |v_i| per output element: `ref` (decode_ref64 or
    prefill_ref64) called with |V|."""
    return ref(q, k, v.abs(), *rest, **kw)


# ---------------------------------------------------------------------------
# bf16-faithful emulation of the kernels' arithmetic
# ---------------------------------------------------------------------------

def _online_softmax_bf16(sc, valid, v, tile: int = 32) -> torch.Tensor:
    """sc [H, G, R, n] fp32 scores, valid [R, n] bool, v [n, H, D] fp32.
    Online softmax over `tile`-key tiles, P rounded to bf16 before PV, l
    summed in fp32, output rounded to bf16.  Returns [R, H*G, D] bf16."""
    H, G, R, n = sc.shape
    m = torch.full((H, G, R), -1e30)
    l = torch.zeros(H, G, R)
    acc = torch.zeros(H, G, R, v.shape[-1])
    for t0 in range(0, n, tile):
        ok = valid[:, t0:t0 + tile]
        s = torch.where(ok, sc[..., t0:t0 + tile], torch.tensor(-1e30))
        m_new = torch.maximum(m, s.amax(-1))
        alpha = torch.exp(m - m_new)
        p = torch.where(ok, torch.exp(s - m_new.unsqueeze(-1)),
                        torch.tensor(0.0))
        l = l * alpha + p.sum(-1)
        pb = p.to(BF16).float()
        acc = acc * alpha.unsqueeze(-1) + torch.einsum(
            "hgrk,khd->hgrd", pb, v[t0:t0 + tile])
        m = m_new
    o = torch.where(l.unsqueeze(-1) > 0, acc / l.unsqueeze(-1).clamp_min(1e-38),
                    torch.tensor(0.0))
    return o.permute(2, 0, 1, 3).reshape(R, H * G, -1).to(BF16)


def decode_emulated(q, key_cache, value_cache, block_tables, context_lens,
                    scale) -> torch.Tensor:
    S, QH, Dh = q.shape
    kvh = key_cache.shape[1]
    page = key_cache.shape[2]
    qpg = QH // kvh
    out = torch.zeros(S, QH, Dh, dtype=BF16)
    for s in range(S):
        ctx = int(context_lens[s])
        if ctx == 0:
            continue
        # stage whole pages like the kernels do, and mask by position
        npages = (ctx + page - 1) // page
        idx = torch.arange(npages * page)
        pages = block_tables[s, idx // page].long()
        k = key_cache[pages, :, idx % page].float()
        v = value_cache[pages, :, idx % page].float()
        qs = q[s].float().view(kvh, qpg, 1, Dh)
        sc = torch.einsum("hgrd,nhd->hgrn", qs, k) * scale
        valid = (idx < ctx).unsqueeze(0)
        out[s] = _online_softmax_bf16(sc, valid, v)[0]
    return out


def prefill_emulated(q, k, v, cu_seqlens, scale,
                     cu_seqlens_k=None) -> torch.Tensor:
    Tq, QH, Dh = q.shape
    kvh = k.shape[1]
    qpg = QH // kvh
    out = torch.zeros(Tq, QH, Dh, dtype=BF16)
    cu = [int(x) for x in cu_seqlens]
    cuk = [int(x) for x in cu_seqlens_k] if cu_seqlens_k is not None else cu
    for b in range(len(cu) - 1):
        s, e, sk, ek = cu[b], cu[b + 1], cuk[b], cuk[b + 1]
        Lq, Lk = e - s, ek - sk
        off = Lk - Lq
        qs = q[s:e].float().view(Lq, kvh, qpg, Dh)
        sc = torch.einsum("rhgd,nhd->hgrn", qs, k[sk:ek].float()) * scale
        valid = (torch.arange(Lk).unsqueeze(0) <=
                 torch.arange(off, Lk).unsqueeze(1))
        out[s:e] = _online_softmax_bf16(sc, valid, v[sk:ek].float())
    return out


# ---------------------------------------------------------------------------
# adversarial paged cache
# ---------------------------------------------------------------------------

class CacheMeta(NamedTuple):
    poison_page: int
    live_pages: List[List[int]]     # per sequence, in logical order
    min_width: int


def build_poisoned_cache_meta(k_seqs, v_seqs, splits_max: int,
                              gen: torch.Generator, spare_pages: int = 3):
    """k_seqs/v_seqs: per sequence a [KVH, ctx, D] bf16 tensor (ctx may be
    0).  Returns ((kc, vc, block_tables, ctx), CacheMeta).

    Physical pages are a random permutation, page 0 is never used by a
    sequence, and every slot no live key owns (last-page tails, spare pages,
    page 0, one dedicated poison page) holds poison: V = 32768 in every dim,
    K = 4 * (random +-1).  Poison is finite on purpose: a correct kernel
    multiplies it by P = 0 exactly.  Block tables are at least
    ceil(ctx_max/16) + 2*splits_max + 2 wide and every unused column holds
    the poison page's (valid) index."""
    kvh = k_seqs[0].shape[0]
    ctxs = [int(k.shape[1]) for k in k_seqs]
    npages = [(c + PAGE - 1) // PAGE for c in ctxs]
    total = 1 + sum(npages) + 1 + spare_pages
    kc = (torch.randint(0, 2, (total, kvh, PAGE, D), generator=gen) * 2 - 1
          ).to(BF16) * K_POISON
    vc = torch.full((total, kvh, PAGE, D), V_POISON, dtype=BF16)
    perm = (torch.randperm(total - 1, generator=gen) + 1).tolist()
    poison_page = perm.pop()
    # deal pages round-robin so no sequence's pages are contiguous
    live: List[List[int]] = [[] for _ in ctxs]
    order = [s for j in range(max(npages + [0])) for s in range(len(ctxs))
             if j < npages[s]]
    for s in order:
        live[s].append(perm.pop())
    min_width = (max(ctxs) + PAGE - 1) // PAGE + 2 * splits_max + 2
    bt = torch.full((len(ctxs), min_width), poison_page, dtype=torch.int32)
    for s, pages in enumerate(live):
        c = ctxs[s]
        for j, pg in enumerate(pages):
            n = min(PAGE, c - j * PAGE)
            kc[pg, :, :n] = k_seqs[s][:, j * PAGE:j * PAGE + n]
            vc[pg, :, :n] = v_seqs[s][:, j * PAGE:j * PAGE + n]
            bt[s, j] = pg
    ctx = torch.tensor(ctxs, dtype=torch.int32)
    return (kc, vc, bt, ctx), CacheMeta(poison_page, live, min_width)


def build_poisoned_cache(k_seqs, v_seqs, splits_max: int,
                         gen: torch.Generator):
    """Returns kc, vc, block_tables, ctx (see build_poisoned_cache_meta)."""
    return build_poisoned_cache_meta(k_seqs, v_seqs, splits_max, gen)[0]


# ---------------------------------------------------------------------------
# cases
# ---------------------------------------------------------------------------

class DecodeCase(NamedTuple):
    group: int
    kvh: int
    ctxs: Tuple[int, ...]
    replicate: bool      # needle: add rows until every target spot is hit

    @property
    def id(self) -> str:
        tail = "all" if self.replicate else "b%d" % len(self.ctxs)
        return "g%d-kvh%d-%s" % (self.group, self.kvh, tail)


# the full context batch plus one ctx == 0 row, at every (group, KVH); then
# batch sizes 1 and 3 (odd tail wave of the 2-sequences-per-workgroup
# kernels), where needle rows are NOT replicated so the row count holds
DECODE_CASES: Tuple[DecodeCase, ...] = tuple(
    DecodeCase(g, h, DECODE_CTXS + (0,), True)
    for g in (1, 2, 4, 8) for h in (1, 2, 8)) + (
    DecodeCase(4, 2, (100,), False),
    DecodeCase(4, 2, (257, 1, 48), False),
    DecodeCase(8, 1, (530,), False),
    DecodeCase(1, 8, (33, 2047, 17), False),
)


class PrefillCase(NamedTuple):
    qh: int
    kvh: int
    lens: Tuple[Tuple[int, int], ...]

    @property
    def id(self) -> str:
        return "qh%d-kvh%d-%s" % (self.qh, self.kvh, "_".join(
            str(lk) if lk == lq else "%dp%d" % (lk, lq)
            for lk, lq in self.lens))

    @property
    def has_prefix(self) -> bool:
        return any(lk != lq for lk, lq in self.lens)


PREFILL_CASES: Tuple[PrefillCase, ...] = tuple(
    PrefillCase(qh, kvh, lens)
    for qh, kvh in PREFILL_HEADS for lens in PREFILL_LENS)


def prefill_families(case: PrefillCase) -> Tuple[str, ...]:
    """Family prob needs every sequence to fit its 64 one-hot columns."""
    if all(lk <= 64 for lk, _ in case.lens):
        return PREFILL_FAMILIES
    return ("needle", "scaled")


def swizzle_branches(case: PrefillCase, qtile: int) -> set:
    """Which branches of the prefill kernels' XCD swizzle a case runs:
    'off' (group 1), 'full' (lin < full) and/or 'rem' (lin >= full)."""
    if case.qh == case.kvh:
        return {"off"}
    nblocks = sum((lq + qtile - 1) // qtile for _, lq in case.lens)
    G = nblocks * case.kvh
    out = set()
    if G // 8:
        out.add("full")
    if G % 8:
        out.add("rem")
    return out


def _needle_values(shape, gen) -> torch.Tensor:
    x = torch.randint(1, 17, shape, generator=gen)
    sign = torch.randint(0, 2, shape, generator=gen) * 2 - 1
    return (x * sign).to(torch.float32).div(8).to(BF16)


def _pm1(shape, gen) -> torch.Tensor:
    return (torch.randint(0, 2, shape, generator=gen) * 2 - 1).to(BF16)


def _randn(shape, gen) -> torch.Tensor:
    return torch.randn(shape, generator=gen).to(BF16)


def decode_target_spots(ctx: int) -> List[int]:
    """Key positions a needle must hit: key 0, the last key, the last key
    of a full page, the first key of the last page, and both sides of every
    split boundary (all DECODE_SPLITS) and of the first page pair."""
    spots = {0, ctx - 1, ((ctx - 1) // PAGE) * PAGE}
    if ctx >= PAGE:
        spots.add((ctx // PAGE) * PAGE - 1)
    spots.update(x for x in (31, 32) if x < ctx)    # first page pair's edge
    for splits in DECODE_SPLITS:
        for s in range(1, splits):
            b = _split_range(ctx, splits, s)[0]
            if b < ctx:
                spots.update((b - 1, b))
    return sorted(spots)


def _check_needle_gap(q, k, targets, scale, valid=None) -> bool:
    """q [R, KVH, G, D], k [KVH, n, D], targets [R, KVH, G]: the target's
    score must lead every other (valid) key's by more than NEEDLE_GAP; this
    also rejects a K row duplicated within its sequence."""
    sc = torch.einsum("rhgd,hnd->rhgn", q.double(), k.double()) * scale
    if valid is not None:
        sc = sc.masked_fill(~valid[:, None, None, :], float("-inf"))
    tgt = sc.gather(-1, targets.unsqueeze(-1))
    sc = sc.scatter(-1, targets.unsqueeze(-1), float("-inf"))
    return bool(((tgt.squeeze(-1) - sc.amax(-1)) > NEEDLE_GAP).all())


@functools.lru_cache(maxsize=None)
def decode_data(case: DecodeCase, family: str) -> Dict:
    """Inputs and expectations of one decode case (CPU tensors; cached and
    shared: callers must not modify them)."""
    for attempt in range(8):
        data = _decode_data(case, family, 1000 * attempt + 17)
        if data is not None:
            return data
    raise AssertionError("no needle draw with gap > %g" % NEEDLE_GAP)


def _decode_data(case: DecodeCase, family: str, seed: int):
    gen = torch.Generator().manual_seed(
        seed + 7919 * (case.group * 100 + case.kvh * 10 + len(case.ctxs)) +
        DECODE_FAMILIES.index(family))
    kvh, qpg = case.kvh, case.group
    QH = kvh * qpg
    k_seqs, v_seqs = [], []
    for c in case.ctxs:
        if family == "needle":
            k_seqs.append(_pm1((kvh, c, D), gen))
            v_seqs.append(_needle_values((kvh, c, D), gen))
        else:
            k_seqs.append(_randn((kvh, c, D), gen))
            if family == "scaled":
                v_seqs.append(_randn((kvh, c, D), gen))
            else:
                key = torch.arange(c)
                hot = (key if family == "prob_key" else key // PAGE) % D
                v = torch.zeros(kvh, c, D, dtype=BF16)
                v[:, key, hot] = 1.0
                v_seqs.append(v)
    (kc, vc, bt_u, ctx_u), meta = build_poisoned_cache_meta(
        k_seqs, v_seqs, max(DECODE_SPLITS), gen)

    rows: List[int] = []
    data: Dict = {"family": family, "case": case, "meta": meta,
                  "scale": SCALE, "kc": kc, "vc": vc}
    if family == "needle":
        qs, exps, tgts = [], [], []
        for u, c in enumerate(case.ctxs):
            if c == 0:
                rows.append(u)
                qs.append(_randn((1, QH, D), gen))
                exps.append(torch.zeros(1, QH, D, dtype=BF16))
                tgts.append(torch.full((1, QH), -1))
                continue
            spots = decode_target_spots(c)
            # enough distinct targets for the heads of one GQA group
            extra = [x for x in torch.randperm(c, generator=gen).tolist()
                     if x not in spots]
            spots = spots + extra[:max(0, min(c, qpg) - len(spots))]
            nrows = -(-len(spots) // QH) if case.replicate else 1
            start = int(torch.randint(0, len(spots), (1,), generator=gen))
            t = (torch.arange(nrows * QH) + (0 if case.replicate else start)
                 ) % len(spots)
            t = torch.tensor(spots)[t].view(nrows, kvh, qpg)
            K, V = k_seqs[u], v_seqs[u]
            hidx = torch.arange(kvh).view(1, kvh, 1).expand_as(t)
            q = (K[hidx, t].float() * 8).to(BF16)          # [R, KVH, G, D]
            if not _check_needle_gap(q, K, t, SCALE):
                return None
            rows += [u] * nrows
            qs.append(q.reshape(nrows, QH, D))
            exps.append(V[hidx, t].reshape(nrows, QH, D))
            tgts.append(t.reshape(nrows, QH))
        data["q"] = torch.cat(qs)
        data["expect"] = torch.cat(exps)
        data["targets"] = torch.cat(tgts)
    else:
        rows = list(range(len(case.ctxs)))
        data["q"] = _randn((len(rows), QH, D), gen)
    r = torch.tensor(rows)
    data["rows"] = r
    data["bt"] = bt_u[r].contiguous()
    data["ctx"] = ctx_u[r].contiguous()
    if family != "needle":
        args = (data["q"], kc, vc, data["bt"], data["ctx"], SCALE)
        data["ref64"] = decode_ref64(*args)
        if family == "scaled":
            data["abs64"] = attn_abs64(decode_ref64, *args)
    return data


@functools.lru_cache(maxsize=None)
def prefill_data(case: PrefillCase, family: str) -> Dict:
    for attempt in range(8):
        data = _prefill_data(case, family, 1000 * attempt + 29)
        if data is not None:
            return data
    raise AssertionError("no needle draw with gap > %g" % NEEDLE_GAP)


def _prefill_targets(Lk: int, Lq: int, kvh: int, qpg: int,
                     gen: torch.Generator) -> torch.Tensor:
    """[Lq, KVH, G] target key of every (row, head): at or before the row's
    position, cycling through key 0, the row's own position (the causal
    edge), both sides of the last 64-key tile boundary, and a random key;
    distinct across the heads of a group wherever the row sees >= G keys."""
    off = Lk - Lq
    t = torch.zeros(Lq, kvh, qpg, dtype=torch.long)
    rnd = torch.randint(0, 1 << 30, (Lq, kvh, qpg), generator=gen)
    for i in range(Lq):
        pos = off + i
        tile = (pos // 64) * 64
        spots = [pos, 0, tile, max(tile - 1, 0)]
        for h in range(kvh):
            used = set()
            for j in range(qpg):
                c = (i + h + j) % 5
                x = spots[c] if c < 4 else int(rnd[i, h, j]) % (pos + 1)
                while x in used and len(used) <= pos:
                    x = (x + 1) % (pos + 1)
                used.add(x)
                t[i, h, j] = x
    return t


def _prefill_data(case: PrefillCase, family: str, seed: int):
    gen = torch.Generator().manual_seed(
        seed + 104729 * PREFILL_CASES.index(case) +
        PREFILL_FAMILIES.index(family))
    QH, kvh = case.qh, case.kvh
    qpg = QH // kvh
    Tk = sum(lk for lk, _ in case.lens)
    Tq = sum(lq for _, lq in case.lens)
    cu_q, cu_k = [0], [0]
    for lk, lq in case.lens:
        cu_q.append(cu_q[-1] + lq)
        cu_k.append(cu_k[-1] + lk)
    data: Dict = {"family": family, "case": case, "scale": SCALE,
                  "cu_q": torch.tensor(cu_q, dtype=torch.int32),
                  "cu_k": (torch.tensor(cu_k, dtype=torch.int32)
                           if case.has_prefix else None)}
    if family == "needle":
        k = _pm1((Tk, kvh, D), gen)
        v = _needle_values((Tk, kvh, D), gen)
        q = torch.zeros(Tq, QH, D, dtype=BF16)
        expect = torch.zeros(Tq, QH, D, dtype=BF16)
        for b, (lk, lq) in enumerate(case.lens):
            K = k[cu_k[b]:cu_k[b + 1]].permute(1, 0, 2)     # [KVH, Lk, D]
            V = v[cu_k[b]:cu_k[b + 1]].permute(1, 0, 2)
            t = _prefill_targets(lk, lq, kvh, qpg, gen)
            hidx = torch.arange(kvh).view(1, kvh, 1).expand_as(t)
            qb = (K[hidx, t].float() * 8).to(BF16)
            valid = (torch.arange(lk).unsqueeze(0) <=
                     torch.arange(lk - lq, lk).unsqueeze(1))
            if not _check_needle_gap(qb, K, t, SCALE, valid):
                return None
            q[cu_q[b]:cu_q[b + 1]] = qb.reshape(lq, QH, D)
            expect[cu_q[b]:cu_q[b + 1]] = V[hidx, t].reshape(lq, QH, D)
        data.update(q=q, k=k, v=v, expect=expect)
        return data
    q = _randn((Tq, QH, D), gen)
    k = _randn((Tk, kvh, D), gen)
    if family == "scaled":
        v = _randn((Tk, kvh, D), gen)
    else:
        # sequence b owns columns [64*(b%2), +64): a neighbour's keys, or a
        # row's own future keys, land in columns that must be exactly 0
        v = torch.zeros(Tk, kvh, D, dtype=BF16)
        for b, (lk, _) in enumerate(case.lens):
            j = torch.arange(lk)
            v[cu_k[b] + j, :, 64 * (b % 2) + j] = 1.0
    data.update(q=q, k=k, v=v)
    args = (q, k, v, data["cu_q"], SCALE, data["cu_k"])
    data["ref64"] = prefill_ref64(*args)
    if family == "scaled":
        data["abs64"] = attn_abs64(prefill_ref64, *args)
    return data


# ---------------------------------------------------------------------------
# checks (shared by the CPU self-test and the GPU tests)
# ---------------------------------------------------------------------------

def check(got: torch.Tensor, data: Dict) -> Tuple[bool, str, float]:
    """Judge a kernel output [rows, QH, D] (bf16) against a case's
    expectation.  Returns (ok, message, worst error / bound)."""
    got = got.detach().cpu()
    fam = data["family"]
    if fam == "needle":
        exp = data["expect"]
        if got.dtype == exp.dtype and torch.equal(got, exp):
            return True, "", 0.0
        bad = (got.float() != exp.float()).any(-1).nonzero()
        r, h = (int(x) for x in bad[0])
        return False, ("needle: %d (row, head) outputs differ from V[target];"
                       " first row %d head %d, max |diff| %g" % (
                           len(bad), r, h,
                           (got.float() - exp.float()).abs().max())), \
            float("inf")
    ref = data["ref64"]
    err = (got.double() - ref).abs()
    if fam == "scaled":
        bound = TOL * data["abs64"] + ABS_FLOOR
    else:
        bound = TOL * ref          # exactly 0 where the reference is 0
    bad = err > bound
    ratio = float((err / bound.clamp_min(1e-300)).max()) if err.numel() else 0.
    if not bool(bad.any()):
        return True, "", ratio
    r, h, d = (int(x) for x in bad.nonzero()[0])
    leak = bool((bad & (ref == 0)).any())
    return False, ("%s: %d elements out of bound%s; first [%d, %d, %d] got %g "
                   "ref %g bound %g" % (
                       fam, int(bad.sum()),
                       " (nonzero where the reference is exactly 0)"
                       if leak else "", r, h, d, float(got[r, h, d]),
                       float(ref[r, h, d]), float(bound[r, h, d]))), ratio


# ---------------------------------------------------------------------------
# mutants: wrong references, used only by the CPU self-test
# ---------------------------------------------------------------------------

DECODE_MUTANTS = ("leak_key", "drop_last", "drop_page", "wrong_page",
                  "swap_heads", "wrong_kv_head") + tuple(
    "drop_split@%d" % s for s in DECODE_SPLITS if s > 1)
PREFILL_MUTANTS = ("future", "next_seq", "no_prefix")


def decode_mutant_applies(mut: str, case: DecodeCase) -> bool:
    """Whether the configuration HAS what the mutant gets wrong (decided
    from the case alone, never from outputs)."""
    if mut == "swap_heads":
        return case.group >= 2          # a group of one has no two heads
    if mut == "wrong_kv_head":
        return case.kvh >= 2            # one KV head cannot be mis-mapped
    return True


def prefill_mutant_applies(mut: str, case: PrefillCase) -> bool:
    if mut == "future":
        return any(lq >= 2 for _, lq in case.lens)   # some row has a future
    if mut == "next_seq":
        return len(case.lens) >= 2
    if mut == "no_prefix":
        return case.has_prefix
    return True


def decode_mutant(data: Dict, mut: str) -> torch.Tensor:
    return _decode64(data["q"], data["kc"], data["vc"], data["bt"],
                     data["ctx"], data["scale"], mut=mut).to(BF16)


def prefill_mutant(data: Dict, mut: str) -> torch.Tensor:
    return _prefill64(data["q"], data["k"], data["v"], data["cu_q"],
                      data["scale"], data["cu_k"], mut=mut).to(BF16)
