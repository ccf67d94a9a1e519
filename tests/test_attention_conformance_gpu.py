"""Exact-routing and mask-leak conformance of the decode and prefill
attention kernels (MI355X; marked gpu).

Inputs, fp64 references, bounds and checks come from tests/attn_cases.py,
whose CPU self-test (tests/test_attn_cases_cpu.py) shows that they accept a
correct kernel and reject each wrong one.  Only two tolerances exist: exact
equality (needle; zero columns of prob), and (2^-7 + 2^-12) relative to p
(prob) or to A = sum p|v| (scaled).

Every decode input lives in a permuted paged cache whose unowned slots and
unused block-table columns hold finite poison (V = 32768), so a key read
from the wrong place, or one masked key leaking, cannot hide.
"""
import pytest
import torch

import attn_cases as ac
import rbg_amd.ops as ops

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    assert ops.HAVE_HIP, f"HIP extension missing: {ops._hip_err!r}"
    return torch.device("cuda:0")


_DEV_CACHE = {}


def _on_dev(kind, case, family, dev):
    """Device copies of one case's inputs, shared by every variant."""
    key = (kind, case, family)
    if key not in _DEV_CACHE:
        data = (ac.decode_data if kind == "decode" else ac.prefill_data)(
            case, family)
        names = (("q", "kc", "vc", "bt", "ctx") if kind == "decode"
                 else ("q", "k", "v", "cu_q", "cu_k"))
        _DEV_CACHE[key] = (data, {
            n: (None if data[n] is None else data[n].to(dev)) for n in names})
    return _DEV_CACHE[key]


# ---------------------------------------------------------------------------
# decode
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("variant", ac.DECODE_VARIANTS)
@pytest.mark.parametrize("family", ac.DECODE_FAMILIES)
@pytest.mark.parametrize("case", ac.DECODE_CASES, ids=lambda c: c.id)
def test_decode_matrix(dev, case, family, variant):
    """variants 0-6 x GQA group {1,2,4,8} x KVH {1,2,8} x splits
    {1,2,3,4,16} (16 > chunk count: empty splits) over contexts 1..2047 plus
    a ctx = 0 row whose output must be all zeros; batches of 1 and 3 rows
    for the odd tail wave of the 2-sequences-per-workgroup kernels."""
    data, d = _on_dev("decode", case, family, dev)
    fails, worst = [], 0.0
    for splits in ac.DECODE_SPLITS:
        got = ops._hip.decode_attention(d["q"], d["kc"], d["vc"], d["bt"],
                                        d["ctx"], ac.SCALE, splits, variant)
        ok, msg, ratio = ac.check(got, data)
        worst = max(worst, ratio)
        if not ok:
            fails.append("splits=%d: %s" % (splits, msg))
    print("decode %s %s v%d: worst err/bound %.3f" % (
        case.id, family, variant, worst))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("variant", ac.DECODE_VARIANTS)
@pytest.mark.parametrize("family", ("needle", "scaled"))
def test_decode_q_from_fused_qkv_slice(dev, family, variant):
    """q as a column slice of a fused QKV buffer: the kernels must honour
    the token stride."""
    case = ac.DECODE_CASES[7]            # group 4, KVH 2, full batch
    data, d = _on_dev("decode", case, family, dev)
    R, QH, D = d["q"].shape
    width = (QH + 2 * case.kvh) * D
    qkv = torch.full((R, width), 3.0, dtype=torch.bfloat16, device=dev)
    q = qkv[:, :QH * D].view(R, QH, D)
    q.copy_(d["q"])
    assert q.stride(0) == width
    for splits in (1, 3):
        got = ops._hip.decode_attention(q, d["kc"], d["vc"], d["bt"],
                                        d["ctx"], ac.SCALE, splits, variant)
        ok, msg, _ = ac.check(got, data)
        assert ok, (splits, msg)


@pytest.mark.parametrize("variant", (-1, 1))
@pytest.mark.parametrize("family", ac.DECODE_FAMILIES)
@pytest.mark.parametrize("case", ac.DECODE_CASES[1::5] + ac.DECODE_CASES[12:],
                         ids=lambda c: c.id)
def test_decode_auto_splits(dev, case, family, variant):
    """ops.decode_attention with num_splits = 0: pick_decode_splits picks,
    for the default variant and for a dot2 one."""
    data, d = _on_dev("decode", case, family, dev)
    got = ops.decode_attention(d["q"], d["kc"], d["vc"], d["bt"], d["ctx"],
                               ac.SCALE, num_splits=0, variant=variant)
    ok, msg, _ = ac.check(got, data)
    assert ok, msg


# ---------------------------------------------------------------------------
# prefill
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("swz", ac.PREFILL_SWZ)
@pytest.mark.parametrize("heads", ac.PREFILL_HEADS,
                         ids=lambda h: "qh%d-kvh%d" % h)
def test_prefill_matrix(dev, heads, swz, monkeypatch):
    """every swz 0-11 x (QH, KVH) x length sets that put nblocks * KVH below
    8, off a multiple of 8 and on one (all three XCD-swizzle branches), with
    and without a cached prefix; family prob where lengths are <= 64."""
    monkeypatch.setattr(ops, "PREFILL_SWZ", swz)
    fails, worst = [], 0.0
    for case in ac.PREFILL_CASES:
        if (case.qh, case.kvh) != heads:
            continue
        for family in ac.prefill_families(case):
            data, d = _on_dev("prefill", case, family, dev)
            got = ops.prefill_attention(d["q"], d["k"], d["v"], d["cu_q"],
                                        ac.SCALE, d["cu_k"])
            ok, msg, ratio = ac.check(got, data)
            worst = max(worst, ratio)
            if not ok:
                fails.append("%s: %s" % (case.id, msg))
    print("prefill qh%d-kvh%d swz%d: worst err/bound %.3f" % (
        heads + (swz, worst)))
    assert not fails, "\n".join(fails)


# ---------------------------------------------------------------------------
# rope_store_kv -> decode round trip
# ---------------------------------------------------------------------------

def test_rope_store_then_decode_round_trip(dev):
    """rope_store_kv writes a needle batch into an all-poison pool, with
    slot = -1 tokens mixed in.  Afterwards the pool equals the expected one
    bit for bit (so the poison page, page 0 and every unowned slot are
    untouched and the -1 tokens wrote nothing), and needle decode over the
    cache it wrote is exact.  Positions are 0, where RoPE is the identity,
    so the stored K is known exactly."""
    case = ac.DecodeCase(4, 2, (17, 1, 80, 33), False)
    data = ac.decode_data(case, "needle")
    meta = data["meta"]
    want_k, want_v = data["kc"], data["vc"]
    pool_k = want_k.clone()
    pool_v = want_v.clone()
    gen = torch.Generator().manual_seed(5)
    ks, vs, slots = [], [], []
    for u, c in enumerate(case.ctxs):
        for i in range(c):
            pg, off = meta.live_pages[u][i // 16], i % 16
            ks.append(want_k[pg, :, off])
            vs.append(want_v[pg, :, off])
            slots.append(pg * 16 + off)
            # un-write the live slot: the pool starts as poison everywhere
            pool_k[pg, :, off] = ac.K_POISON * want_k[pg, :, off]
            pool_v[pg, :, off] = ac.V_POISON
            if i % 7 == 3:           # a dead token that must write nothing
                ks.append(torch.randn(case.kvh, ac.D, generator=gen).bfloat16())
                vs.append(torch.randn(case.kvh, ac.D, generator=gen).bfloat16())
                slots.append(-1)
    assert (pool_v == ac.V_POISON).all()
    T = len(slots)
    QH = case.group * case.kvh
    k = torch.stack(ks).to(dev)                       # [T, KVH, D]
    v = torch.stack(vs).to(dev)
    q = torch.randn(T, QH, ac.D, generator=gen).bfloat16().to(dev)
    k0, q0 = k.clone(), q.clone()
    cos_sin = ops.build_cos_sin_table(ac.D, 16, device=dev)
    pos = torch.zeros(T, dtype=torch.int32, device=dev)
    slot_t = torch.tensor(slots, dtype=torch.int32, device=dev)
    pool_k, pool_v = pool_k.to(dev), pool_v.to(dev)
    ops._hip.rope_store_kv(q, k, v, pool_k, pool_v, cos_sin, pos, slot_t)
    assert torch.equal(q, q0) and torch.equal(k, k0)   # identity at pos 0
    pp = meta.poison_page
    assert torch.equal(pool_k[pp].cpu(), want_k[pp])
    assert torch.equal(pool_v[pp].cpu(), want_v[pp])
    assert torch.equal(pool_k.cpu(), want_k)
    assert torch.equal(pool_v.cpu(), want_v)
    bt, ctx, dq = data["bt"].to(dev), data["ctx"].to(dev), data["q"].to(dev)
    for variant in ac.DECODE_VARIANTS:
        for splits in (1, 2):
            got = ops._hip.decode_attention(dq, pool_k, pool_v, bt, ctx,
                                            ac.SCALE, splits, variant)
            ok, msg, _ = ac.check(got, data)
            assert ok, (variant, splits, msg)


# ---------------------------------------------------------------------------
# inputs the kernels would mishandle must raise instead of launching
# ---------------------------------------------------------------------------

def _good_decode_args(dev, kvh=2, qh=8, page=16, d=128, seqs=3):
    kc = torch.zeros(6, kvh, page, d, dtype=torch.bfloat16, device=dev)
    return dict(
        q=torch.zeros(seqs, qh, 128, dtype=torch.bfloat16, device=dev),
        kc=kc, vc=torch.zeros_like(kc),
        bt=torch.ones(seqs, 4, dtype=torch.int32, device=dev),
        ctx=torch.ones(seqs, dtype=torch.int32, device=dev))


def _decode(a, splits=1, variant=4):
    return ops._hip.decode_attention(a["q"], a["kc"], a["vc"], a["bt"],
                                     a["ctx"], ac.SCALE, splits, variant)


def test_decode_accepts_the_baseline_arguments(dev):
    # the mutations below each change ONE thing of an input that works
    out = _decode(_good_decode_args(dev))
    assert torch.equal(out, torch.zeros_like(out))


def _mutations():
    def page_not_pow2(a, dev):
        a["kc"] = torch.zeros(6, 2, 12, 128, dtype=torch.bfloat16, device=dev)
        a["vc"] = torch.zeros_like(a["kc"])

    def cache_not_contiguous(a, dev):
        big = torch.zeros(6, 4, 16, 128, dtype=torch.bfloat16, device=dev)
        a["kc"] = big[:, :2]
        a["vc"] = torch.zeros_like(big)[:, :2]

    def value_cache_not_contiguous(a, dev):
        a["vc"] = torch.zeros(6, 4, 16, 128, dtype=torch.bfloat16,
                              device=dev)[:, :2]

    def cache_not_bf16(a, dev):
        a["kc"] = a["kc"].to(torch.float16)
        a["vc"] = a["vc"].to(torch.float16)

    def cache_head_dim_64(a, dev):
        a["kc"] = torch.zeros(6, 2, 16, 64, dtype=torch.bfloat16, device=dev)
        a["vc"] = torch.zeros_like(a["kc"])

    def cache_shapes_differ(a, dev):
        a["vc"] = torch.zeros(7, 2, 16, 128, dtype=torch.bfloat16, device=dev)

    def heads_not_divisible(a, dev):
        a["q"] = torch.zeros(3, 3, 128, dtype=torch.bfloat16, device=dev)

    def block_tables_on_cpu(a, dev):
        a["bt"] = a["bt"].cpu()

    def context_lens_on_cpu(a, dev):
        a["ctx"] = a["ctx"].cpu()

    def block_tables_rows(a, dev):
        a["bt"] = torch.ones(2, 4, dtype=torch.int32, device=dev)

    def context_lens_rows(a, dev):
        a["ctx"] = torch.ones(4, dtype=torch.int32, device=dev)

    def block_tables_not_contiguous(a, dev):
        a["bt"] = torch.ones(3, 8, dtype=torch.int32, device=dev)[:, ::2]

    return [page_not_pow2, cache_not_contiguous, value_cache_not_contiguous,
            cache_not_bf16, cache_head_dim_64, cache_shapes_differ,
            heads_not_divisible, block_tables_on_cpu, context_lens_on_cpu,
            block_tables_rows, context_lens_rows, block_tables_not_contiguous]


@pytest.mark.parametrize("mutate", _mutations(), ids=lambda f: f.__name__)
def test_decode_rejects_bad_input(dev, mutate):
    a = _good_decode_args(dev)
    mutate(a, dev)
    with pytest.raises(RuntimeError):
        _decode(a)


def test_decode_rejects_zero_splits(dev):
    with pytest.raises(RuntimeError):
        _decode(_good_decode_args(dev), splits=0)


def _good_rope_args(dev, kvh=2, qh=8, T=5):
    kc = torch.zeros(6, kvh, 16, 128, dtype=torch.bfloat16, device=dev)
    return dict(
        q=torch.zeros(T, qh, 128, dtype=torch.bfloat16, device=dev),
        k=torch.zeros(T, kvh, 128, dtype=torch.bfloat16, device=dev),
        v=torch.zeros(T, kvh, 128, dtype=torch.bfloat16, device=dev),
        kc=kc, vc=torch.zeros_like(kc),
        cs=ops.build_cos_sin_table(128, 16, device=dev),
        pos=torch.zeros(T, dtype=torch.int32, device=dev),
        slots=torch.arange(16, 16 + T, dtype=torch.int32, device=dev))


def _rope(a):
    ops._hip.rope_store_kv(a["q"], a["k"], a["v"], a["kc"], a["vc"], a["cs"],
                           a["pos"], a["slots"])


def test_rope_store_accepts_the_baseline_arguments(dev):
    a = _good_rope_args(dev)
    a["v"].fill_(2.0)
    _rope(a)
    assert (a["vc"][1, :, :5] == 2.0).all() and a["vc"].sum() == 2.0 * 5 * 256


def _rope_mutations():
    def page_not_pow2(a, dev):
        a["kc"] = torch.zeros(6, 2, 12, 128, dtype=torch.bfloat16, device=dev)
        a["vc"] = torch.zeros_like(a["kc"])

    def cache_not_contiguous(a, dev):
        big = torch.zeros(6, 4, 16, 128, dtype=torch.bfloat16, device=dev)
        a["kc"] = big[:, :2]
        a["vc"] = torch.zeros_like(big)[:, :2]

    def cache_not_bf16(a, dev):
        a["kc"] = a["kc"].to(torch.float16)
        a["vc"] = a["vc"].to(torch.float16)

    def cache_head_dim_64(a, dev):
        a["kc"] = torch.zeros(6, 2, 16, 64, dtype=torch.bfloat16, device=dev)
        a["vc"] = torch.zeros_like(a["kc"])

    def cache_kv_heads_differ(a, dev):
        a["kc"] = torch.zeros(6, 4, 16, 128, dtype=torch.bfloat16, device=dev)
        a["vc"] = torch.zeros_like(a["kc"])

    def slots_on_cpu(a, dev):
        a["slots"] = a["slots"].cpu()

    def positions_on_cpu(a, dev):
        a["pos"] = a["pos"].cpu()

    def slots_too_few(a, dev):
        a["slots"] = a["slots"][:3].contiguous()

    return [page_not_pow2, cache_not_contiguous, cache_not_bf16,
            cache_head_dim_64, cache_kv_heads_differ, slots_on_cpu,
            positions_on_cpu, slots_too_few]


@pytest.mark.parametrize("mutate", _rope_mutations(),
                         ids=lambda f: f.__name__)
def test_rope_store_rejects_bad_input(dev, mutate):
    a = _good_rope_args(dev)
    mutate(a, dev)
    with pytest.raises(RuntimeError):
        _rope(a)
