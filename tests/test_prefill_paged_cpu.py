"""Paged prefill on the CPU: the op against the reference on gathered rows,
the engine option, and the block map (docs/FEATURES.md "Paged prefill")."""
import pytest
import torch

import attn_cases as ac
from rbg_amd import ops
from rbg_amd.engine.config import EngineConfig, ModelConfig
from rbg_amd.engine.engine import LLMEngine
from rbg_amd.engine.sequence import SamplingParams
from rbg_amd.ops import reference

FP8_KW = dict(kv_cache_dtype="fp8_e4m3", kv_k_scale_log2=-2,
              kv_v_scale_log2=-3)
PREFIX_CASES = [c for c in ac.PREFILL_CASES if c.has_prefix][:3]


@pytest.mark.parametrize("kv", ({}, FP8_KW), ids=("bf16", "fp8"))
@pytest.mark.parametrize("preset", ("tiny", "tiny-qwen"))
def test_engines_leave_identical_pools(preset, kv, monkeypatch):
    calls = []
    orig = ops.prefill_attention_paged
    monkeypatch.setattr(ops, "prefill_attention_paged", lambda *a, **k:
                        (calls.append(1), orig(*a, **k))[1])
    gen = torch.Generator().manual_seed(5)
    long, short = (torch.randint(0, 500, (n,), generator=gen).tolist()
                   for n in (100, 40))
    runs = {}
    for read in ("gather", "paged"):
        del calls[:]
        eng = LLMEngine(EngineConfig(
            model=ModelConfig.preset(preset), device="cpu",
            kv_pool_tokens=2048, max_prefill_tokens=24, enforce_eager=True,
            prefill_kv_read=read, **kv))
        sp = SamplingParams(max_new_tokens=4)
        toks = [s.output_tokens for s in eng.generate([long, short], sp)]
        toks += [s.output_tokens for s in eng.generate([long], sp)]
        runs[read] = (toks, eng.runner.cache.kv.view(torch.uint8).clone(),
                      len(calls))
    assert runs["gather"][2] == 0 and runs["paged"][2] > 0
    assert runs["paged"][0] == runs["gather"][0]
    assert torch.equal(runs["paged"][1], runs["gather"][1])


@pytest.mark.parametrize("case", PREFIX_CASES, ids=lambda c: c.id)
def test_cpu_op_equals_reference_on_gathered_rows(case):
    data = ac.prefill_data(case, "scaled")
    lens = [lk for lk, _ in case.lens]
    kc, vc, bt, _ = ac.build_poisoned_cache(
        [t.permute(1, 0, 2) for t in data["k"].split(lens)],
        [t.permute(1, 0, 2) for t in data["v"].split(lens)], 1,
        torch.Generator().manual_seed(3))
    got = ops.prefill_attention_paged(data["q"], kc, vc, bt, data["cu_q"],
                                      ac.SCALE, data["cu_k"])
    want = reference.prefill_attention(data["q"], data["k"], data["v"],
                                       data["cu_q"], ac.SCALE, data["cu_k"])
    assert torch.equal(got, want)


def test_engine_config_rejects():
    assert EngineConfig().prefill_kv_read == "gather"
    EngineConfig(prefill_kv_read="paged")
    for kw in (dict(prefill_kv_read="scatter"),
               dict(prefill_kv_read="paged", page_size=32)):
        with pytest.raises(ValueError):
            EngineConfig(**kw)


@pytest.mark.parametrize("qtile", (64, 128))
def test_block_map_matches_the_gather_kernels(qtile):
    cu = torch.tensor([0, 1, 161, 290], dtype=torch.int32)
    cuk = torch.tensor([0, 130, 322, 451], dtype=torch.int32)
    info, lens = reference.prefill_block_info(cu, qtile, cuk)
    pinfo, plens = reference.prefill_block_info_paged(cu, qtile, cuk)
    assert torch.equal(pinfo[:, [0, 1, 3]], info[:, [0, 1, 3]])
    assert torch.equal(plens, lens)
    assert pinfo[:, 2].tolist() == [0] + [1] * (-(-160 // qtile)) + \
        [2] * (-(-129 // qtile))
