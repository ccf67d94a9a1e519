"""FP8 (e4m3) KV cache on the GPU (MI355X; marked gpu): the quantising
rope_store_kv, kv_gather_dequant, the dequantising decode kernel, the
byte-based peer push, the rejects, and the engine at model level.

Inputs, references and bounds come from tests/kvfp8_cases.py (kernel level)
and tests/kvfp8_model_cases.py (model level); tests/test_kvfp8_cases_cpu.py
shows on the CPU that they accept a correct implementation and reject wrong
ones.  Kernel-level bounds are exact (bytes, torch.equal) or attn_cases'
unchanged TOL = 2^-7 + 2^-12.
"""
import pytest
import torch

import attn_cases as ac
import kvfp8_cases as k8
import rbg_amd.ops as ops

pytestmark = pytest.mark.gpu

BF16, FP8, U8 = torch.bfloat16, torch.float8_e4m3fn, torch.uint8


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    assert ops.HAVE_HIP, f"HIP extension missing: {ops._hip_err!r}"
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------
# quantiser
# ---------------------------------------------------------------------------

def _store_and_check(d, dev, ek, ev, fused=False):
    kq0, vq0 = k8.poison_pool(d["pages"], d["k"].shape[1])
    want_q, want_k, want_kb, want_vb = k8.store_expected(d, kq0, vq0, ek, ev)
    q, k, v = (d[n].to(dev) for n in "qkv")
    if fused:
        _, q, k, v = k8.fused_slices(q, k, v)
        assert not q.is_contiguous() or q.shape[0] == 1
    kq, vq = kq0.to(dev), vq0.to(dev)
    ops.rope_store_kv(q, k, v, kq, vq, d["table"].to(dev), d["pos"].to(dev),
                      d["slots"].to(dev), k_scale_log2=ek, v_scale_log2=ev)
    torch.cuda.synchronize()
    T = d["q"].shape[0]
    # the cache bytes: the written rows AND every unwritten (poison) byte
    ok, msg = k8.bytes_match(vq.view(U8), want_vb)
    assert ok, "value_cache (ev=%d): %s" % (ev, msg)
    ok, msg = k8.bytes_match(kq.view(U8), want_kb)
    assert ok, "key_cache (ek=%d): %s" % (ek, msg)
    # q and k were rotated in place: quarter turns are exact
    for name, got, want in (("q", q, want_q), ("k", k, want_k)):
        got = got.reshape(T, -1).cpu().float()
        want = want.reshape(T, -1).float()
        same = (got == want) | (got.isnan() & want.isnan())
        assert bool(same.all()), "rotated %s differs" % name
    return vq, kq


@pytest.mark.parametrize("e", k8.QUANT_EXPONENTS)
def test_quantiser_exhaustive(dev, e):
    """All 65 536 bf16 bit patterns as V and as K (512 tokens x 1 head x
    128): the bytes equal the torch reference, NaN compared as NaN.  Second
    pass: a permuted slot_mapping with -1 entries into an all-poison pool,
    whose unwritten bytes stay intact bit for bit."""
    d = k8.exhaustive_inputs(permuted=False)
    vq, kq = _store_and_check(d, dev, e, e)
    # every token was written, in order: compare against the definition too
    rows = vq.view(U8)[1:33].cpu().permute(0, 2, 1, 3).reshape(512, 1, 128)
    ok, msg = k8.bytes_match(rows, k8.q8(d["v"], e).view(U8))
    assert ok, msg
    d2 = k8.exhaustive_inputs(permuted=True)
    assert bool((d2["slots"] < 0).any())
    vq2, _ = _store_and_check(d2, dev, e, e)
    written = torch.zeros(d2["pages"] * 16, dtype=torch.bool)
    written[d2["slots"][d2["slots"] >= 0].long()] = True
    untouched = vq2.view(U8).cpu().permute(0, 2, 1, 3).reshape(-1, 128)[~written]
    assert untouched.numel() and bool((untouched == k8.V_POISON_BYTE).all())


@pytest.mark.parametrize("fused", (False, True), ids=("contig", "fusedqkv"))
@pytest.mark.parametrize("T", k8.QUANT_TS)
@pytest.mark.parametrize("heads", k8.QUANT_HEADS, ids=lambda h: "qh%d-kvh%d" % h)
def test_quantising_store_shapes(dev, heads, T, fused):
    d = k8.quant_inputs(heads[0], heads[1], T, 1)
    for ek, ev in ((-3, 2), (0, 0), (2, -3)):
        _store_and_check(d, dev, ek, ev, fused)


# ---------------------------------------------------------------------------
# gather
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("kvh", k8.GATHER_KVH)
@pytest.mark.parametrize("tkv", k8.GATHER_TKV)
def test_gather_dequant(dev, tkv, kvh):
    cache, slots = k8.gather_inputs(tkv, kvh)
    for e in (0, -2, 3):
        got = ops.kv_gather_dequant(cache.to(dev), slots.to(dev), e)
        assert got.dtype == BF16 and got.is_contiguous()
        assert torch.equal(got.cpu(), k8.gather_expected(cache, slots, e))


# ---------------------------------------------------------------------------
# decode
# ---------------------------------------------------------------------------

_DEV_CACHE = {}


def _on_dev(case, family, exps, dev):
    key = (case, family, exps)
    if key not in _DEV_CACHE:
        data = k8.decode_data(case, family, *exps)
        _DEV_CACHE[key] = (data, {n: data[n].to(dev) for n in
                                  ("q", "kq", "vq", "kd", "vd", "bt", "ctx")})
    return _DEV_CACHE[key]


@pytest.mark.parametrize("exps", k8.DECODE_EXPONENTS, ids=lambda e: "e%d_%d" % e)
@pytest.mark.parametrize("family", ac.DECODE_FAMILIES)
@pytest.mark.parametrize("case", ac.DECODE_CASES, ids=lambda c: c.id)
def test_decode_matrix(dev, case, family, exps):
    """GQA group {1,2,4,8} x KVH {1,2,8} x splits {1,2,3,4,16} over contexts
    1..2047 plus a ctx = 0 row, batches of 1 and 3, exponent pairs (0, 0) and
    (-2, 3).  The fp8 kernel keeps variant 4's arithmetic order, so its
    output also equals, bit for bit, the bf16 variant 4 on the dequantised
    cache."""
    data, d = _on_dev(case, family, exps, dev)
    ek, ev = exps
    fails, worst = [], 0.0
    for splits in ac.DECODE_SPLITS:
        got = ops.decode_attention(d["q"], d["kq"], d["vq"], d["bt"],
                                   d["ctx"], ac.SCALE, num_splits=splits,
                                   k_scale_log2=ek, v_scale_log2=ev)
        ok, msg, ratio = ac.check(got, data)
        worst = max(worst, ratio)
        if not ok:
            fails.append("splits=%d: %s" % (splits, msg))
        twin = ops._hip.decode_attention(d["q"], d["kd"], d["vd"], d["bt"],
                                         d["ctx"], ac.SCALE, splits, 4)
        if not torch.equal(got.view(torch.int16), twin.view(torch.int16)):
            fails.append("splits=%d: differs from bf16 variant 4 on the "
                         "dequantised cache" % splits)
    print("fp8 decode %s %s e=%s: worst err/bound %.3f" % (
        case.id, family, exps, worst))
    assert not fails, "\n".join(fails)


def test_decode_every_byte_code(dev):
    """K and V caches of uniformly random finite e4m3 codes: all 254 occur,
    subnormals and -0 included.  The kernel's byte -> bf16 stage must agree
    with torch's conversion: the output equals bf16 variant 4 on the cache
    dequantised by torch, bit for bit."""
    ek, ev = -2, 3
    kq, _ = k8.gather_inputs(40 * 16 - 48, 2, seed=5)      # 40 pages
    vq, _ = k8.gather_inputs(40 * 16 - 48, 2, seed=6)
    for c in (kq, vq):
        seen = torch.bincount(c.view(U8).reshape(-1).long(), minlength=256)
        assert int((seen > 0).sum()) == 254
    gen = torch.Generator().manual_seed(8)
    ctx = torch.tensor([33, 257, 100, 0], dtype=torch.int32)
    bt = (torch.randperm(39, generator=gen)[:4 * 9].view(4, 9) + 1
          ).repeat(1, 2).to(torch.int32)                    # 18 columns
    q = (torch.randn(4, 8, 128, generator=gen) * 0.02).to(BF16)
    args = [t.to(dev) for t in (q, kq, vq, bt, ctx)]
    twin_kv = [k8.dq(kq, ek).to(dev), k8.dq(vq, ev).to(dev)]
    for splits in (1, 3):
        got = ops.decode_attention(*args, ac.SCALE, num_splits=splits,
                                   k_scale_log2=ek, v_scale_log2=ev)
        twin = ops._hip.decode_attention(args[0], *twin_kv, args[3], args[4],
                                         ac.SCALE, splits, 4)
        assert bool(got.float().isfinite().all())
        assert float(got[:3].float().abs().max()) > 0
        assert torch.equal(got.view(torch.int16), twin.view(torch.int16))


@pytest.mark.parametrize("family", ("needle", "scaled"))
def test_decode_q_from_fused_qkv_slice_and_auto_splits(dev, family):
    case = ac.DECODE_CASES[7]            # group 4, KVH 2, full batch
    exps = k8.DECODE_EXPONENTS[1]
    data, d = _on_dev(case, family, exps, dev)
    R, QH, D = d["q"].shape
    width = (QH + 2 * case.kvh) * D
    qkv = torch.full((R, width), 3.0, dtype=BF16, device=dev)
    q = qkv[:, :QH * D].view(R, QH, D)
    q.copy_(d["q"])
    assert q.stride(0) == width
    for splits in (0, 1, 3):             # 0: pick_decode_splits chooses
        got = ops.decode_attention(q, d["kq"], d["vq"], d["bt"], d["ctx"],
                                   ac.SCALE, num_splits=splits,
                                   k_scale_log2=exps[0], v_scale_log2=exps[1])
        ok, msg, _ = ac.check(got, data)
        assert ok, (splits, msg)


# ---------------------------------------------------------------------------
# rejects: nothing is launched
# ---------------------------------------------------------------------------

def _good(dev, page=16, d=128):
    kc = torch.zeros(6, 2, page, d, dtype=U8, device=dev).view(FP8)
    return dict(q=torch.zeros(3, 8, d, dtype=BF16, device=dev), key_cache=kc,
                value_cache=kc.clone(),
                block_tables=torch.ones(3, 4, dtype=torch.int32, device=dev),
                context_lens=torch.ones(3, dtype=torch.int32, device=dev),
                scale=ac.SCALE, num_splits=1)


def test_decode_accepts_the_baseline_arguments(dev):
    out = ops.decode_attention(**_good(dev))
    assert torch.equal(out, torch.zeros_like(out))


def test_fp8_rejects(dev, monkeypatch):
    launched = []
    for name in ("decode_attention_fp8", "rope_store_kv_fp8",
                 "kv_gather_dequant"):
        orig = getattr(ops._hip, name)
        monkeypatch.setattr(ops._hip, name, lambda *a, _o=orig, _n=name:
                            (launched.append(_n), _o(*a))[1])
    bf = torch.zeros(6, 2, 16, 128, dtype=BF16, device=dev)
    bad = [dict(_good(dev, page=32)), dict(_good(dev, d=64)),
           dict(_good(dev), value_cache=bf),
           dict(_good(dev), key_cache=bf),
           dict(_good(dev), k_scale_log2=17),
           dict(_good(dev), v_scale_log2=-17),
           dict(_good(dev), variant=1), dict(_good(dev), variant=6)]
    for kw in bad:
        with pytest.raises((RuntimeError, ValueError)):
            ops.decode_attention(**kw)
    assert launched == []
    # the bindings check for themselves as well
    g = _good(dev)
    args = [g["q"], g["key_cache"], g["value_cache"], g["block_tables"],
            g["context_lens"], ac.SCALE, 1]
    for e in ((17, 0), (0, -17)):
        with pytest.raises(RuntimeError):
            ops._hip.decode_attention_fp8(*args, *e)
    g32 = _good(dev, page=32)
    with pytest.raises(RuntimeError):
        ops._hip.decode_attention_fp8(g["q"], g32["key_cache"],
                                      g32["value_cache"], g["block_tables"],
                                      g["context_lens"], ac.SCALE, 1, 0, 0)
    with pytest.raises(RuntimeError):
        ops._hip.decode_attention_fp8(g["q"], g["key_cache"], bf,
                                      g["block_tables"], g["context_lens"],
                                      ac.SCALE, 1, 0, 0)
    with pytest.raises(RuntimeError):
        ops._hip.kv_gather_dequant(bf, torch.zeros(1, dtype=torch.int32,
                                                   device=dev), 0)
    # and the bf16 entry points still reject an fp8 cache
    with pytest.raises(RuntimeError):
        ops._hip.decode_attention(g["q"], g["key_cache"], g["value_cache"],
                                  g["block_tables"], g["context_lens"],
                                  ac.SCALE, 1, 4)


def test_engine_config_rejects():
    from rbg_amd.engine.config import EngineConfig
    for kw in (dict(kv_cache_dtype="int8"),
               dict(kv_cache_dtype="fp8_e4m3", kv_k_scale_log2=-17),
               dict(kv_cache_dtype="fp8_e4m3", kv_v_scale_log2=17)):
        with pytest.raises(ValueError):
            EngineConfig(**kw)


# ---------------------------------------------------------------------------
# transfer: byte-based peer push between two fp8 pools
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("n", (1, 3, 8))
def test_local_peer_push_between_fp8_pools(dev, n):
    from rbg_amd.engine.config import EngineConfig, ModelConfig
    from rbg_amd.engine.kv_cache import PagedKVCache
    from rbg_amd.parallel.kv_peer import (PeerKVPusher, export_meta_local,
                                          peer_capable)
    fp8 = dict(kv_cache_dtype="fp8_e4m3", kv_k_scale_log2=-1,
               kv_v_scale_log2=2)
    cfg = EngineConfig(model=ModelConfig.preset("tiny"), device="cuda",
                       kv_pool_tokens=24 * 16, **fp8)
    src, dst = PagedKVCache(cfg, dev), PagedKVCache(cfg, dev)
    assert src.kv.dtype == FP8 and peer_capable(src) and peer_capable(dst)
    gen = torch.Generator().manual_seed(7 + n)
    src.kv.view(U8).copy_(torch.randint(0, 256, src.kv.shape, generator=gen)
                          .to(U8))
    dst.kv.view(U8).fill_(k8.V_POISON_BYTE)
    src_pages = torch.randperm(23, generator=gen)[:n].add(1).tolist()
    dst_pages = torch.randperm(23, generator=gen)[:n].add(1).tolist()
    want = dst.kv.view(U8).clone()
    want.index_copy_(2, torch.tensor(dst_pages, device=dev),
                     src.kv.view(U8).index_select(
                         2, torch.tensor(src_pages, device=dev)))
    pusher = PeerKVPusher(dev)
    pending = pusher.push(src, src_pages, export_meta_local(dst), dst_pages)
    pending.wait()
    assert pending.nbytes == n * src.kv[:, :, 0].numel()
    assert torch.equal(dst.kv.view(U8), want)
    # a bf16 pool, or other exponents, on the far side: refused up front
    other = PagedKVCache(EngineConfig(
        model=ModelConfig.preset("tiny"), device="cuda",
        kv_pool_tokens=24 * 16), dev)
    with pytest.raises(ValueError):
        pusher.push(src, src_pages, export_meta_local(other), dst_pages)
    meta = dict(export_meta_local(dst), kv_v_scale_log2=3)
    with pytest.raises(ValueError):
        pusher.push(src, src_pages, meta, dst_pages)


# ---------------------------------------------------------------------------
# model level: the engine in fp8 mode against the quantised dense fp64 forward
# ---------------------------------------------------------------------------

import kvfp8_model_cases as m8          # noqa: E402
import model_cases as mc                # noqa: E402

MODEL_CASES = [(s, c, m) for c in mc.CONFS for s in m8.SCENARIOS
               for m in ("eager", "graph")]


@pytest.mark.parametrize("scenario,conf,mode", MODEL_CASES)
def test_fp8_engine_matches_quantised_dense_fp64(scenario, conf, mode):
    """C1 logits and C2 dequantised cache rows within 2 x e_cpu8 (relative
    L2 over the scenario, see kvfp8_model_cases), C3 every unwritten byte
    still poison, and the fp8 store, gather and decode kernels, not their
    bf16 siblings, were the ones reached."""
    assert ops.HAVE_HIP, ops._hip_err
    run = m8.run_scenario8(scenario, conf, "cuda", mode == "eager")
    assert run.engine.runner.cache.kv.is_cuda
    assert run.graph_mode == (mode == "graph")
    run.trace.assert_fp8_paths(run.graph_mode)
    if run.graph_mode:
        assert run.rec.graph_replays == len(run.rec.decode_batches) > 0
    c1, c2, c3 = m8.judge8(run)
    print("\n%s fp8: worst err / e_cpu8 logits %.3f, K/V %.3f" % (
        (run.id,) + m8.worst(c1, c2)))
    assert not m8.failures(c1, c2, c3), m8.failures(c1, c2, c3)[:8]
