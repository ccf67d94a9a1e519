"""Paged prefill attention on the GPU (docs/FEATURES.md "Paged prefill"):
ops.prefill_attention_paged against fp64 on adversarial paged caches, bit
for bit against the gather path, its e4m3 instantiation bit for bit against
the bf16 one on the dequantised pool, its argument checks, and two engines
(prefill_kv_read "gather" and "paged") that must leave identical KV pools."""
import functools

import pytest
import torch

import attn_cases as ac
import kvfp8_cases as k8
import model_cases as mc
from rbg_amd import ops
from rbg_amd.engine.engine import LLMEngine
from rbg_amd.engine.sequence import SamplingParams

pytestmark = pytest.mark.gpu

BF16, U8 = torch.bfloat16, torch.uint8
# contexts of 9, 17 and 5 tiles: the library's longest is 4
PIPE_LENS = (((530, 530),), ((1040, 17), (33, 33)), ((257, 257), (16, 16)))
LIB = [(c, f) for c in ac.PREFILL_CASES for f in ac.prefill_families(c)]
PIPE = [(i, "scaled") for i in range(len(PIPE_LENS))]
SCALED = [(c, f) for c, f in LIB + PIPE if f == "scaled"]


def _id(key):
    return key.id if isinstance(key, ac.PrefillCase) else "pipe%d" % key


def _params(cases):
    return pytest.mark.parametrize(
        "key,family", cases, ids=["%s-%s" % (_id(k), f) for k, f in cases])


def _with_ref(data, k, v):
    args = (data["q"], k, v, data["cu_q"], ac.SCALE, data["cu_k"])
    return dict(data, ref64=ac.prefill_ref64(*args),
                abs64=ac.attn_abs64(ac.prefill_ref64, *args))


@functools.lru_cache(maxsize=None)
def _pipe_data(i):
    lens = PIPE_LENS[i]
    gen = torch.Generator().manual_seed(4201 + i)
    cu_q, cu_k = [0], [0]
    for lk, lq in lens:
        cu_q.append(cu_q[-1] + lq)
        cu_k.append(cu_k[-1] + lk)
    data = {"family": "scaled", "case": ac.PrefillCase(8, 2, lens),
            "scale": ac.SCALE, "cu_q": torch.tensor(cu_q, dtype=torch.int32),
            "cu_k": torch.tensor(cu_k, dtype=torch.int32),
            "q": ac._randn((cu_q[-1], 8, ac.D), gen),
            "k": ac._randn((cu_k[-1], 2, ac.D), gen),
            "v": ac._randn((cu_k[-1], 2, ac.D), gen)}
    return _with_ref(data, data["k"], data["v"])


@functools.lru_cache(maxsize=None)
def _load(key, family):
    """(data, key cache, value cache, block tables) of a case, on the CPU."""
    data = (ac.prefill_data(key, family) if isinstance(key, ac.PrefillCase)
            else _pipe_data(key))
    lens = [lk for lk, _ in data["case"].lens]
    k_seqs = [t.permute(1, 0, 2) for t in data["k"].split(lens)]
    v_seqs = [t.permute(1, 0, 2) for t in data["v"].split(lens)]
    gen = torch.Generator().manual_seed(977 + sum(lens))
    kc, vc, bt, _ = ac.build_poisoned_cache(k_seqs, v_seqs, 1, gen)
    return data, kc, vc, bt


def _cu_k(data):
    return None if data["cu_k"] is None else data["cu_k"].cuda()


def _paged(data, kc, vc, bt, ek=0, ev=0):
    return ops.prefill_attention_paged(
        data["q"].cuda(), kc.cuda(), vc.cuda(), bt.cuda(), data["cu_q"].cuda(),
        ac.SCALE, _cu_k(data), ek, ev)


@_params(LIB + PIPE)
def test_paged_matches_fp64(key, family):
    data, kc, vc, bt = _load(key, family)
    ok, msg, ratio = ac.check(_paged(data, kc, vc, bt), data)
    print("\nworst err / bound %.3f" % ratio)
    assert ok, msg


@_params(SCALED)
def test_paged_same_bits_as_gather_path(key, family):
    assert ops.PREFILL_SWZ == 6
    data, kc, vc, bt = _load(key, family)
    want = ops.prefill_attention(data["q"].cuda(), data["k"].cuda(),
                                 data["v"].cuda(), data["cu_q"].cuda(),
                                 ac.SCALE, _cu_k(data))
    assert torch.equal(_paged(data, kc, vc, bt), want)


@pytest.mark.parametrize("ek,ev", k8.DECODE_EXPONENTS)
@_params([(c, f) for c, f in LIB + PIPE if f != "prob"])
def test_paged_fp8(key, family, ek, ev):
    data, kc, vc, bt = _load(key, family)
    kq, vq = k8.q8(kc, ek), k8.q8(vc, ev)
    kd, vd = k8.dq(kq, ek), k8.dq(vq, ev)
    got = _paged(data, kq, vq, bt, ek, ev)
    if family == "needle":
        # K = +-1 and V = x/8, x in 1..16, quantise losslessly
        live = vc != ac.V_POISON
        assert torch.equal(kd, kc) and torch.equal(vd[live], vc[live])
        ok, msg, _ = ac.check(got, data)
        assert ok, msg
        return
    assert torch.equal(got, _paged(data, kd, vd, bt))
    ref = _with_ref(data, k8.dq(k8.q8(data["k"], ek), ek),
                    k8.dq(k8.q8(data["v"], ev), ev))
    ok, msg, ratio = ac.check(got, ref)
    print("\nworst err / bound %.3f" % ratio)
    assert ok, msg


def _good(dtype=BF16, page=16, d=128):
    dev = "cuda"
    kc = torch.zeros(4, 2, page, d, dtype=U8 if dtype != BF16 else BF16,
                     device=dev).view(dtype)
    i32 = functools.partial(torch.tensor, dtype=torch.int32, device=dev)
    return dict(q=torch.zeros(3, 4, 128, dtype=BF16, device=dev),
                key_cache=kc, value_cache=kc.clone(),
                block_tables=i32([[1, 2]]), cu_seqlens=i32([0, 3]),
                scale=ac.SCALE, cu_seqlens_k=i32([0, 20]))


def test_paged_rejects(monkeypatch):
    launched = []
    orig = ops._hip.prefill_attention_paged
    monkeypatch.setattr(ops._hip, "prefill_attention_paged",
                        lambda *a: (launched.append(1), orig(*a))[1])
    out = ops.prefill_attention_paged(**_good())
    assert launched == [1] and torch.equal(out, torch.zeros_like(out))
    fp8, g = _good(k8.FP8), _good()
    i32 = functools.partial(torch.tensor, dtype=torch.int32, device="cuda")
    bad = [dict(g, value_cache=fp8["value_cache"]),
           dict(g, key_cache=fp8["key_cache"]),
           dict(fp8, k_scale_log2=17), dict(fp8, v_scale_log2=-17),
           _good(page=32), _good(d=64),
           dict(g, block_tables=i32([[1]])),
           dict(g, block_tables=g["block_tables"].long()),
           dict(g, cu_seqlens_k=i32([0, 20, 25])),
           dict(g, cu_seqlens_k=i32([0, 2]))]
    for kw in bad:
        with pytest.raises(ValueError):
            ops.prefill_attention_paged(**kw)
    assert launched == [1]


FP8_KW = dict(kv_cache_dtype="fp8_e4m3", kv_k_scale_log2=-2,
              kv_v_scale_log2=-3)


@pytest.mark.parametrize("kv", ({}, FP8_KW), ids=("bf16", "fp8"))
@pytest.mark.parametrize("conf", mc.CONFS)
def test_engines_leave_identical_pools(conf, kv, monkeypatch):
    calls = []
    for name in ("prefill_attention_paged", "kv_gather_dequant"):
        orig = getattr(ops._hip, name)
        monkeypatch.setattr(ops._hip, name, lambda *a, _o=orig, _n=name:
                            (calls.append(_n), _o(*a))[1])
    gen = torch.Generator().manual_seed(5)
    long, short = (torch.randint(0, 512, (n,), generator=gen).tolist()
                   for n in (100, 40))
    runs = {}
    for read in ("gather", "paged"):
        del calls[:]
        eng = LLMEngine(mc.engine_config(conf, "cuda", True,
                                         max_prefill_tokens=24,
                                         prefill_kv_read=read, **kv))
        sp = SamplingParams(max_new_tokens=4)
        toks = [s.output_tokens for s in eng.generate([long, short], sp)]
        toks += [s.output_tokens for s in eng.generate([long], sp)]
        runs[read] = (toks, eng.runner.cache.kv.view(U8).clone(), list(calls))
    assert "prefill_attention_paged" not in runs["gather"][2]
    assert runs["paged"][2].count("prefill_attention_paged") > 0
    assert "kv_gather_dequant" not in runs["paged"][2]
    assert runs["paged"][0] == runs["gather"][0]
    assert torch.equal(runs["paged"][1], runs["gather"][1])
