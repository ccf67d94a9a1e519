"""Mixture of experts on the CPU (docs/FEATURES.md "Mixture of experts"): the
torch references against fp64, the argument checks, the engine with the
`conf-moe` model.  The case builders and fp64 references here also serve
tests/test_moe_gpu.py.

moe_ffn is judged in three families of inputs: "integer" (every value a small
whole number, the result exact), "scaled" (random, judged against fp64 by the
error of ops.reference on the same rows, whole tensor and per token row) and
"order" (exact expert outputs, random fp32 weights: only the combine rounds,
so its contract, f32 mul, f32 add, slot order, is checked bit for bit).  The
self-tests at the bottom prove that check_ffn rejects wrong kernels
(ffn_emulate's faults) and wrong combines."""
import pytest
import torch

import rbg_amd.ops as ops
from rbg_amd.engine.config import EngineConfig, ModelConfig
from rbg_amd.engine.engine import LLMEngine
from rbg_amd.engine.sequence import SamplingParams
from rbg_amd.models.llama import LlamaForCausalLM, TPContext

BF16 = torch.bfloat16
FACTOR = 2.0
ROUTE_CASES = [(E, k, T, rn) for E in (8, 128, 256) for k in (1, 2, 8)
               for T in (1, 37) for rn in (True, False)]
# (E, k, H, I, rows per expert): every count the kernel treats differently,
# 0 / 1 / 15 / 16 / 17 and 65 = one more than a 64-row pass
FFN_CASES = [(4, 1, 256, 64, (0, 1, 15, 17)),
             (8, 2, 768, 192, (16, 0, 1, 17, 15, 65, 33, 1)),
             (8, 8, 256, 192, (65,) * 8),
             (4, 2, 768, 64, (16, 16, 0, 0)),
             # I = 128: two steps in the down GEMM.  k = 3, 194 tokens: a
             # third pass with 0, 1 and 2 live rows (128, 129, 130), a full
             # MT = 4 pass (64), two full tiles (32), three (48), three and
             # one row (49), and a two-row expert
             (8, 3, 256, 128, (128, 129, 130, 32, 48, 49, 64, 2)),
             # k = 7, 64 tokens: exactly one full pass for six experts
             (8, 7, 256, 128, (64,) * 6 + (32, 32))]
# expert counts off a multiple of 64 and E = 1; k = 3, 6, 7 (where k <= E)
ROUTE_CASES_WIDE = sorted(
    {(E, k, T, rn) for E in (1, 3, 60, 64, 65, 100, 255)
     for k in (1, 2, 3, 6, 7, 8) for T in (1, 37) for rn in (True, False)} |
    {(E, k, T, rn) for E in (8, 128, 256) for k in (3, 6, 7) for T in (1, 37)
     for rn in (True, False)})
ROUTE_CASES_WIDE = [c for c in ROUTE_CASES_WIDE if c[1] <= c[0]]
# T * k = 1023, 1024, 1025 and 2049: either side of the sort's per-wave range
# growing from 64 to 128 pairs, and of 128 to 192
ROUTE_CASES_PAIRS = [(E, k, T, True) for E in (60, 256)
                     for T, k in ((1023, 1), (128, 8), (1025, 1), (683, 3))]
# (E, k, T, hot expert): every row's largest logit is the hot expert's
ROUTE_CASES_SKEWED = [(256, k, 2500, hot) for k in (1, 8) for hot in (0, 255)]


def moe_config(**kw):
    return ModelConfig(**{**dict(
        name="conf-moe", hidden_size=512, intermediate_size=1024, num_layers=2,
        num_heads=4, num_kv_heads=1, head_dim=128, vocab_size=512,
        max_position=2048, qk_norm=True, num_experts=8, num_experts_per_tok=2,
        moe_intermediate_size=192), **kw})


def moe_engine(device, eager=True):
    return LLMEngine(EngineConfig(model=moe_config(), device=device,
                                  page_size=16, kv_pool_tokens=2048,
                                  max_batch_size=8, max_seq_len=256,
                                  enforce_eager=eager))


def route_logits(E, T, seed=0):
    """bf16 logits in [-16, 16] (bf16 alone makes ties plentiful at E = 256);
    with T >= 3, row 0 ties everywhere and row 1 mixes NaN and -inf."""
    g = torch.Generator().manual_seed(seed)
    x = ((torch.rand(T, E, generator=g) * 32 - 16).to(BF16))
    if T >= 3:
        x[0] = 1.5
        x[0, E // 2:] = 3.0
    if T >= 3 and E >= 3:       # (below 3 experts no finite logit would stay)
        x[1, 0::3] = float("nan")
        x[1, 1::3] = float("-inf")
    return x


def skewed_logits(E, T, hot, seed=0):
    """bf16 logits in [-4, 4] with expert `hot` at 12 in every row: with
    k = 1 every pair goes to one expert; with k > 1 the other slots are
    random."""
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand(T, E, generator=g) * 8 - 4).to(BF16)
    x[:, hot] = 12.0
    return x


def route_ref(logits, k, renorm):
    x = logits.double().cpu()
    x = torch.where(torch.isnan(x), torch.full_like(x, float("-inf")), x)
    ids = torch.sort(x, dim=-1, descending=True, stable=True).indices[:, :k]
    w = torch.softmax(x, dim=-1).gather(1, ids)
    return ids.to(torch.int32), w / w.sum(1, keepdim=True) if renorm else w


def check_route(ids, w, logits, k, renorm):
    ref_ids, ref_w = route_ref(logits, k, renorm)
    assert ids.dtype == torch.int32 and w.dtype == torch.float32
    assert torch.equal(ids.cpu(), ref_ids)
    err = (w.double().cpu() - ref_w).abs()
    print("route max rel err * 2^18:",
          float((err / ref_w.clamp_min(1e-300)).max() * 2 ** 18))
    assert bool((err <= 2.0 ** -18 * ref_w).all())


def ids_from_counts(counts, k):
    """ids [T, k] in which expert e holds counts[e] pairs and every token k
    distinct experts, the slots of token t rotated by t."""
    lab = torch.repeat_interleave(torch.arange(len(counts)),
                                  torch.tensor(counts))
    T = lab.numel() // k
    assert T * k == lab.numel() and max(counts) <= T
    ids = lab.view(k, T).t()
    rot = (torch.arange(k) + torch.arange(T)[:, None]) % k
    return ids.gather(1, rot).to(torch.int32).contiguous()


def ffn_f64(x, w1, w2, ids, w, silu=torch.nn.functional.silu):
    """(h, y) in fp64 with nothing rounded; h as [T, k, I]."""
    x, w1, w2, w = (t.double().cpu() for t in (x, w1, w2, w))
    ids, I = ids.cpu().long(), w2.shape[2]
    gu = torch.einsum("th,tjnh->tjn", x, w1[ids])
    h = silu(gu[..., :I]) * gu[..., I:]
    return h, torch.einsum("tj,tji,tjhi->th", w, h, w2[ids])


def ffn_slots_f64(x, w1, w2, ids, w, silu=torch.nn.functional.silu):
    """o [T, k, H] in fp64: every slot's expert output before the weights."""
    h = ffn_f64(x, w1, w2, ids, w, silu)[0]
    return torch.einsum("tji,tjhi->tjh", h, w2.double().cpu()[ids.cpu().long()])


def switch_silu(g):
    """silu on the integer family's gate values, where it is g or 0 to the
    last bit of an fp32 (1 + e^-32 rounds to 1, 128 * e^-128 to 0)."""
    assert bool(((g == 0) | (g == 32) | (g == 64) | (g == -128)).all())
    return g.clamp_min(0)


def ffn_case(case, family, seed=0):
    E, k, H, I, counts = case
    g = torch.Generator().manual_seed(seed)
    ids = ids_from_counts(counts, k)
    T = ids.shape[0]
    if family == "scaled":
        x = torch.randn(T, H, generator=g) * 0.5
        w1 = torch.randn(E, 2 * I, H, generator=g) * 0.05
        w2 = torch.randn(E, H, I, generator=g) * 0.05
        w = torch.rand(T, k, generator=g) + 0.1
        w = w / w.sum(1, keepdim=True)
    else:
        # x in {-1, 0, 1} with a 1 in column 0 of every k-step; gate row i
        # holds one of 0 / 32 / 64 / -128 in such a column, so g is that
        # value and silu(g) is g or 0; two +-1 per up row and one per w2
        # row keep |h| <= 128 and |y| <= 240; w in {1/2 .. 1/16}
        x = torch.randint(-1, 2, (T, H), generator=g).float()
        x[:, ::64] = 1.0
        w1 = torch.zeros(E, 2 * I, H)
        gate = torch.tensor([0.0, 32.0, 64.0, -128.0])
        col = 64 * torch.randint(0, H // 64, (E, I), generator=g)
        w1[:, :I].scatter_(2, col[..., None], gate[
            torch.randint(0, 4, (E, I, 1), generator=g)])
        sign = lambda *s: torch.randint(0, 2, s, generator=g) * 2.0 - 1
        w1[:, I:].scatter_(2, torch.randint(0, H, (E, I, 2), generator=g),
                           sign(E, I, 2))
        w2 = torch.zeros(E, H, I).scatter_(
            2, torch.randint(0, I, (E, H, 1), generator=g), sign(E, H, 1))
        w = 2.0 ** -(1 + (torch.arange(T)[:, None] + torch.arange(k)) % 4)
        h, y = ffn_f64(x, w1, w2, ids, w, switch_silu)
        for t in (h, y):
            assert torch.equal(t, t.round()) and float(t.abs().max()) <= 256
        assert float(h.abs().max()) > 0 and float(y.abs().max()) > 0
        if family == "order":
            # o = +-3 h, not a power of two as +-h is: w * o then needs 26
            # bits and the product itself rounds
            w2 = w2 * 3
            w = order_weights(x, w1, w2, ids, g)
    return (x.to(BF16), w1.to(BF16), w2.to(BF16), ids,
            w.float().contiguous())


# ---- the combine's contract: f32 mul, f32 add, slot order, two roundings ---

def combine(o, w, order=None, fused=False):
    """bf16(((w0 * o0) + (w1 * o1)) + ...) for o fp32 [T, k, H] and w fp32
    [T, k], every product and every sum rounded to fp32 (torch's CPU mul and
    add are single IEEE operations).  order: the slot sequence; fused: a +
    w * o with one rounding (exact in fp64, then rounded)."""
    order = range(o.shape[1]) if order is None else order
    acc = torch.zeros_like(o[:, 0])
    for j in order:
        if fused:
            acc = (acc.double() + w[:, j:j + 1].double() * o[:, j].double()
                   ).float()
        else:
            acc = acc + w[:, j:j + 1] * o[:, j]
    return acc.to(BF16)


def equivalent_orders(k):
    """The slot orders that give the bits of 0, 1 .. k-1 whatever the data:
    itself and, fp32 addition being commutative, the first two swapped."""
    return {tuple(range(k)), (1, 0) + tuple(range(2, k))}


def probed_orders(k):
    """The orders order_weights proves distinguishable from slot order.  For
    k = 3 all of them.  Above that, the ones that move a planted slot (the
    reversal, every rotation, every transposition with slot 0 or k - 1):
    between the two planted slots every small term is rounded to a whole
    number whatever the order it arrives in (A + s rounds to A + round(s)
    while A is a whole number of the same binade), so two orders that differ
    only there give the same bits by arithmetic, not by luck."""
    import itertools
    if k <= 3:
        return set(itertools.permutations(range(k)))
    ident = tuple(range(k))
    out = {ident, (1, 0) + ident[2:], ident[::-1]}
    out |= {ident[r:] + ident[:r] for r in range(1, k)}
    for a in (0, k - 1):
        for b in range(k):
            p = list(ident)
            p[a], p[b] = p[b], p[a]
            out.add(tuple(p))
    return out


def order_weights(x, w1, w2, ids, g):
    """fp32 weights in (0, 1), none a power of two.  With k >= 3, the token
    in the middle gets w[0] * o[0] = 2^24 - 5 and w[k-1] * o[k-1] = -(2^24 +
    4) in one column: a sum that carries one of them is rounded to whole
    numbers (or even ones), one that carries neither is not, so the bf16 row
    depends on where in the order each slot is added.  Asserted here: no
    other order of probed_orders (equivalent_orders apart) gives the row
    that slot order gives.  With k = 2 the two orders are one (fp32 addition
    commutes) and only the roundings can be told."""
    T, k = ids.shape
    w = torch.rand(T, k, generator=g) * 0.98 + 0.01
    o = ffn_slots_f64(x, w1, w2, ids, w, switch_silu)
    assert torch.equal(o.float().double(), o)
    t2 = -1
    if k >= 2:
        # a token whose first two slots cancel in a column the others leave
        # alone gets the same weight for both: mul-then-add gives 0 there,
        # an fma the rounding error of the product
        pair = ((o[:, 0] == -o[:, 1]) & (o[:, 0] != 0) &
                (o[:, 2:] == 0).all(1)).nonzero()
        # (the first such token whose 3 * w does not fit 24 bits)
        for t2 in pair[:, 0].unique().tolist():
            wt = w[t2:t2 + 1].clone()
            wt[0, 1] = wt[0, 0]
            ot = o[t2:t2 + 1].float()
            if not torch.equal(combine(ot, wt, fused=True), combine(ot, wt)):
                w[t2] = wt[0]
                break
        else:
            raise AssertionError("no token shows an fma")
    if k >= 3:
        # (the first token, from the middle on, where the claim holds)
        for t in list(range(T // 2, T)) + list(range(T // 2)):
            both = ((o[t, 0] != 0) & (o[t, k - 1] != 0)).nonzero()
            if t == t2 or not both.numel():
                continue
            c = int(both[0])
            ot, wt = o[t:t + 1].float(), w[t:t + 1].clone()
            wt[0, 0] = (2.0 ** 24 - 5) / float(o[t, 0, c])
            wt[0, k - 1] = -(2.0 ** 24 + 4) / float(o[t, k - 1, c])
            want = combine(ot, wt)
            same = {p for p in probed_orders(k)
                    if torch.equal(combine(ot, wt, p), want)}
            if same == equivalent_orders(k):
                w[t] = wt[0]
                break
        else:
            raise AssertionError("no token tells the probed orders apart")
    mant = torch.frexp(w.float())[0].abs()
    assert bool((mant != 0.5).all()) and bool((w != 0).all())
    return w


def order_expected(args):
    """What the kernel must give bit for bit in the "order" family: its o is
    exact (integers), so only the combine rounds."""
    o = ffn_slots_f64(*args, switch_silu)
    assert torch.equal(o, o.round()) and float(o.abs().max()) <= 1024
    return combine(o.float(), args[4].float().cpu())


def rel_l2(y, ref):
    return float((y.double().cpu() - ref).norm() / ref.norm())


def ffn_refs(args, family):
    """What check_ffn compares with, computed once for a set of arguments:
    the exact result ("integer", "order") or (fp64 y, ops.reference's y)."""
    if family == "integer":
        return ffn_f64(*args, switch_silu)[1].float()
    if family == "order":
        return order_expected(args)
    return ffn_f64(*args)[1], ops.reference.moe_ffn(*(t.cpu() for t in args))


def check_ffn(args, family, y, refs=None):
    refs = ffn_refs(args, family) if refs is None else refs
    if family == "integer":
        assert torch.equal(y.float().cpu(), refs)
        return
    if family == "order":
        assert torch.equal(y.cpu(), refs)
        return
    ref, cpu = refs
    err, base = rel_l2(y, ref), rel_l2(cpu, ref)
    print("moe_ffn rel L2: %.3e, reference %.3e, ratio %.2f"
          % (err, base, err / base))
    assert err <= FACTOR * base
    # per token row, against the reference path's error on the same row: both
    # round h and y at the same points and those roundings dominate, so the
    # two are two draws from one distribution (the argument of model_cases'
    # C1); one wrong row of 130 moves the aggregate by less than a percent
    d = (y.double().cpu() - ref).norm(dim=1)
    b = (cpu.double() - ref).norm(dim=1)
    assert bool((b > 0).all())
    print("moe_ffn worst row ratio: %.3f (row %d of %d)"
          % (float((d / b).max()), int((d / b).argmax()), d.numel()))
    assert bool((d <= FACTOR * b).all())


def bad_ffn_args(args, name):
    x, w1, w2, ids, w = args
    E = w1.shape[0]
    wide = torch.cat([x, x], dim=1)
    return {
        "id_high": (x, w1, w2, ids.clone().index_fill_(
            1, torch.tensor([0], device=ids.device), E), w),
        "id_negative": (x, w1, w2, -1 - ids, w),
        "w1_shape": (x, w1[:, :-64].contiguous(), w2, ids, w),
        "w2_shape": (x, w1, w2[:-1], ids, w),
        "ids_shape": (x, w1, w2, ids[:-1], w),
        "w_shape": (x, w1, w2, ids, w[:, :-1].contiguous()),
        "hidden_not_256": (x[:, :192].contiguous(), w1[..., :192].contiguous(),
                           w2[:, :192].contiguous(), ids, w),
        "x_dtype": (x.float(), w1, w2, ids, w),
        "ids_dtype": (x, w1, w2, ids.long(), w),
        "w_dtype": (x, w1, w2, ids, w.to(BF16)),
        "x_strided": (wide[:, :x.shape[1]], w1, w2, ids, w),
        "w_device": (x, w1, w2, ids, w.to("meta")),
    }[name]


BAD_ARGS = ("id_high", "id_negative", "w1_shape", "w2_shape", "ids_shape",
            "w_shape", "hidden_not_256", "x_dtype", "ids_dtype", "w_dtype",
            "x_strided", "w_device")


# ---- wrong kernels, for the self-test of check_ffn ------------------------

FFN_MUTANTS = ("odd_last_step", "half_step", "row64_from_63", "clamp_15",
               "up_tile_plus_1", "slot_lost", "truncate_h")


def ffn_emulate(args, mutant=None):
    """moe.hip's data flow in torch on the CPU (rows grouped by expert in
    ascending pair order, fp32 GEMMs, bf16 h, fp32 rows per pair, combine in
    slot order), with one fault of FFN_MUTANTS if named:
      odd_last_step   a GEMM with an odd number of 64-k steps drops the last
      half_step       both GEMMs drop k in [32, 64) of every step
      row64_from_63   sorted row 64 of an expert gathers row 63's token
      clamp_15        rows >= 16 of an expert with 17..64 rows gather row 15's
      up_tile_plus_1  gate tile t (16 columns) meets up tile t + 1
      slot_lost       the pair's row lands in slot 0 of its token
      truncate_h      h is cut, not rounded, to bf16"""
    x, w1, w2, ids, w = (t.cpu() for t in args)
    (T, H), E, I, k = x.shape, w1.shape[0], w2.shape[2], ids.shape[1]
    flat = ids.flatten().long()
    order = torch.sort(flat, stable=True).indices
    counts = torch.bincount(flat, minlength=E).tolist()

    def kept(K):
        keep = torch.ones(K)
        if mutant == "half_step":
            keep[torch.arange(K) % 64 >= 32] = 0
        if mutant == "odd_last_step" and (K // 64) % 2:
            keep[K - 64:] = 0
        return keep

    opart = torch.zeros(T * k, H)
    off = 0
    for e, n in enumerate(counts):
        pairs = order[off:off + n]
        off += n
        if n == 0:
            continue
        src = torch.arange(n)
        if mutant == "row64_from_63" and n > 64:
            src[64] = 63
        if mutant == "clamp_15" and 17 <= n <= 64:
            src = src.clamp_max(15)
        gu = (x.float()[pairs[src] // k] * kept(H)) @ w1[e].float().t()
        gate, up = gu[:, :I], gu[:, I:]
        if mutant == "up_tile_plus_1":
            up = up.view(n, I // 16, 16).roll(-1, 1).reshape(n, I)
        h = torch.nn.functional.silu(gate) * up
        if mutant == "truncate_h":
            h = (h.contiguous().view(torch.int32) & -65536).view(torch.float32)
        h = h.to(BF16).float()
        opart[pairs // k * k if mutant == "slot_lost" else pairs] = \
            (h * kept(I)) @ w2[e].float().t()
    return combine(opart.view(T, k, H), w)


def ffn_verdict(args, family, mutant, refs, clean):
    """"no-op" (the fault changes no bit of this case), "caught" or
    "missed"."""
    y = ffn_emulate(args, mutant)
    if torch.equal(y, clean):
        return "no-op"
    try:
        check_ffn(args, family, y, refs)
    except AssertionError:
        return "caught"
    return "missed"


@pytest.mark.parametrize("E,k,T,renorm", [c for c in ROUTE_CASES
                                          if c[0] != 128 and c[2] == 37])
def test_reference_route(E, k, T, renorm):
    logits = route_logits(E, T)
    check_route(*ops.moe_route(logits, k, renorm), logits, k, renorm)


@pytest.mark.parametrize("E,k,T,renorm", [
    c for c in ROUTE_CASES_WIDE if c[2] == 37 and c[3]] + ROUTE_CASES_PAIRS[:4])
def test_reference_route_wide(E, k, T, renorm):
    logits = route_logits(E, T)
    check_route(*ops.moe_route(logits, k, renorm), logits, k, renorm)


@pytest.mark.parametrize("E,k,T,hot", ROUTE_CASES_SKEWED)
def test_skewed_builder(E, k, T, hot):
    logits = skewed_logits(E, T, hot)
    assert float((logits[:, hot:hot + 1].float() - logits.float()
                  ).masked_fill(torch.arange(E) == hot, 99).min()) >= 8
    ids, w = ops.moe_route(logits, k, True)
    check_route(ids, w, logits, k, True)
    assert bool((ids[:, 0] == hot).all())
    assert k == 1 or ids[:, 1:].unique().numel() > 200


# the cases of the self-tests below: between them every fault of FFN_MUTANTS
# has something to break (an odd step count, 65 and 17..64 rows, k > 1)
SELF_CASES = (FFN_CASES[1], FFN_CASES[4], FFN_CASES[5])


@pytest.mark.parametrize("family", ("integer", "scaled", "order"))
@pytest.mark.parametrize("case", SELF_CASES, ids=str)
def test_ffn_checks_reject_wrong_kernels(case, family):
    """The emulation passes check_ffn; each fault is a no-op on this case or
    is caught.  A "missed" is allowed only where the docstring of
    FFN_EXPECTED_MISSES names it."""
    args = ffn_case(case, family)
    refs = ffn_refs(args, family)
    clean = ffn_emulate(args)
    check_ffn(args, family, clean, refs)
    got = {m: ffn_verdict(args, family, m, refs, clean) for m in FFN_MUTANTS}
    print("\n%s %s: %s" % (family, case[:4], got))
    for m, v in got.items():
        assert v != "missed" or (family, m) in FFN_EXPECTED_MISSES, (m, got)
    FFN_TABLE[(case, family)] = got


# nothing is allowed to slip through.  truncate_h is a no-op in the integer
# and order families (h is a whole number there) and is caught per row in the
# scaled one: cutting instead of rounding doubles the dominant error
FFN_EXPECTED_MISSES = set()
FFN_TABLE = {}


def test_every_ffn_fault_is_caught_somewhere():
    for case in SELF_CASES:
        for family in ("integer", "scaled", "order"):
            if (case, family) not in FFN_TABLE:
                test_ffn_checks_reject_wrong_kernels(case, family)
    for m in FFN_MUTANTS:
        for family in ("integer", "scaled", "order"):
            got = {FFN_TABLE[(c, family)][m] for c in SELF_CASES}
            if m == "truncate_h" and family != "scaled":
                assert got == {"no-op"}
            else:
                assert "caught" in got and "missed" not in got, (m, family)


@pytest.mark.parametrize("case", FFN_CASES, ids=str)
def test_combine_contract_rejects_other_combines(case):
    """The "order" family's expected bits differ from a reversed slot order
    (k > 1), from an fma, and from weights rounded to bf16."""
    x, w1, w2, ids, w = args = ffn_case(case, "order")
    want = order_expected(args)
    o = ffn_slots_f64(*args, switch_silu).float()
    k = ids.shape[1]
    if k > 2:       # (two slots: a + b = b + a)
        assert not torch.equal(combine(o, w, reversed(range(k))), want)
    if k > 1:       # (one slot: 0 + w * o rounds once either way)
        assert not torch.equal(combine(o, w, fused=True), want)
    assert not torch.equal(combine(o, w.to(BF16).float()), want)
    assert torch.equal(ops.moe_ffn(*args), want)


def test_stale_grouping_is_dropped():
    """An in-place edit of ids after moe_route: moe_ffn must see the edit
    (and check its range again)."""
    args = ffn_case(FFN_CASES[0], "scaled")
    x, w1, w2, _, w = args
    E, k = w1.shape[0], 1
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(x.shape[0], E, generator=g).to(BF16)
    ids, w = ops.moe_route(logits, k, True)
    # a CPU route attaches no grouping; attach a marker as a GPU route does
    ids._moe_group = (E, None, None)
    ids._moe_group_version = ids._version
    ids[0, 0] = (int(ids[0, 0]) + 1) % E
    assert torch.equal(ops.moe_ffn(x, w1, w2, ids, w),
                       ops.moe_ffn(x, w1, w2, ids.clone(), w))
    ids[0, 0] = E
    with pytest.raises(ValueError):
        ops.moe_ffn(x, w1, w2, ids, w)


@pytest.mark.parametrize("family", ("integer", "scaled"))
@pytest.mark.parametrize("case", FFN_CASES[:2], ids=str)
def test_reference_ffn(case, family):
    args = ffn_case(case, family)
    check_ffn(args, family, ops.moe_ffn(*args))
    empty = ops.moe_ffn(args[0][:0], args[1], args[2], args[3][:0],
                        args[4][:0])
    assert empty.shape == (0, case[2]) and empty.dtype == BF16


@pytest.mark.parametrize("name", BAD_ARGS)
def test_ffn_rejects(name):
    with pytest.raises(ValueError):
        ops.moe_ffn(*bad_ffn_args(ffn_case(FFN_CASES[0], "scaled"), name))


def test_engine_generates_and_reloads():
    eng = moe_engine("cpu")
    prompts = [[7], list(range(17)), list(range(100, 140))]
    greedy = SamplingParams(max_new_tokens=4)
    first = [s.output_tokens for s in eng.generate(prompts, greedy)]
    assert all(len(t) == 4 for t in first)
    assert first == [s.output_tokens for s in
                     moe_engine("cpu").generate(prompts, greedy)]
    eng.reload_weights(99)
    assert first != [s.output_tokens for s in eng.generate(prompts, greedy)]


@pytest.mark.parametrize("kw", [
    dict(num_experts=257), dict(num_experts_per_tok=9),
    dict(num_experts=4, num_experts_per_tok=5),
    dict(moe_intermediate_size=96), dict(hidden_size=384, num_heads=3)],
    ids=str)
def test_refused_configurations(kw):
    with pytest.raises(ValueError):
        LlamaForCausalLM(moe_config(**kw), torch.device("cpu"))


def test_refused_tp_and_fp8_experts():
    dev = torch.device("cpu")
    with pytest.raises(ValueError):
        LlamaForCausalLM(moe_config(), dev, TPContext(size=2, rank=0))
    with pytest.raises(ValueError):
        LlamaForCausalLM(moe_config(), dev, weight_dtype="fp8_e4m3")
    with pytest.raises(ValueError):
        EngineConfig(model=moe_config(), device="cpu", tp_size=2)


DENSE_TINY_PARAMS = [
    ("embed", (512, 256)), ("final_norm", (256,)), ("lm_head", (512, 256))] + [
    ("layers.%d.%s" % (i, n), s) for i in (0, 1) for n, s in (
        ("input_norm", (256,)), ("post_norm", (256,)),
        ("attn.wqkv", (512, 256)), ("attn.wo", (256, 256)),
        ("mlp.w_gate_up", (1024, 256)), ("mlp.w_down", (256, 512)))]


def test_dense_parameter_list_unchanged():
    assert ModelConfig().num_experts == 0
    model = LlamaForCausalLM(ModelConfig.preset("tiny"), torch.device("cpu"))
    assert [(n, tuple(p.shape)) for n, p in model.named_parameters()] == \
        DENSE_TINY_PARAMS
    moe = LlamaForCausalLM(moe_config(), torch.device("cpu"))
    assert [tuple(p.shape) for n, p in moe.named_parameters()
            if n.startswith("layers.1.mlp.")] == [
                (8, 512), (8, 384, 512), (8, 512, 192)]
    preset = ModelConfig.preset("qwen3-30b-a3b")
    assert (preset.num_experts, preset.num_experts_per_tok,
            preset.moe_intermediate_size, preset.hidden_size,
            preset.num_layers, preset.num_kv_heads) == (128, 8, 768, 2048,
                                                        48, 4)
