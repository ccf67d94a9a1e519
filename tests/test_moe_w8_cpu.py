"""FP8 (e4m3) expert weights on the CPU (docs/FEATURES.md "FP8 experts"): the
op's CPU path, the model's parameters and the option's way from a role
argument to the stats RPC.  quantise() and w8_case() also serve
tests/test_moe_w8_gpu.py."""
import types

import pytest
import torch

import rbg_amd.ops as ops
import test_moe_cpu as mc
from rbg_amd.engine import serve_worker as sw
from rbg_amd.engine.config import EngineConfig, ModelConfig
from rbg_amd.engine.engine import LLMEngine
from rbg_amd.engine.sequence import SamplingParams
from rbg_amd.models.llama import LlamaForCausalLM

FP8, CPU = torch.float8_e4m3fn, torch.device("cpu")


def quantise(w):
    """bf16 [E, N, K] -> (e4m3 [E, N, K], int8 [E, N], dq bf16 [E, N, K])."""
    w8, e = ops.quantize_weight_e4m3(w.view(-1, w.shape[2]))
    dq = ops.dequantize_weight_e4m3(w8, e)
    return w8.view(w.shape), e.view(w.shape[:2]), dq.view(w.shape)


def w8_case(case, family):
    """(x, w1_8, w2_8, ids, w, e1, e2) and the bf16 twin's (dq1, dq2)."""
    x, w1, w2, ids, w = mc.ffn_case(case, family)
    (w1_8, e1, dq1), (w2_8, e2, dq2) = quantise(w1), quantise(w2)
    return (x, w1_8, w2_8, ids, w, e1, e2), (dq1, dq2)


def fp8_engine(device, eager=True, dtype="fp8_e4m3"):
    return LLMEngine(EngineConfig(
        model=mc.moe_config(), device=device, page_size=16,
        kv_pool_tokens=2048, max_batch_size=8, max_seq_len=256,
        enforce_eager=eager, expert_weight_dtype=dtype))


@pytest.mark.parametrize("case", mc.FFN_CASES[:2], ids=str)
def test_cpu_op_is_the_reference_on_dq(case):
    args, (dq1, dq2) = w8_case(case, "scaled")
    x, _, _, ids, w = args[:5]
    assert torch.equal(ops.moe_ffn(*args),
                       ops.reference.moe_ffn(x, dq1, dq2, ids, w))
    for bad in (args[:5], args[:6], (x, dq1, dq2, ids, w) + args[5:],
                (x, args[1], dq2, ids, w, args[5], None),
                args[:6] + (args[6].int(),),
                args[:6] + (args[6][:, :-1].contiguous(),)):
        with pytest.raises(ValueError):
            ops.moe_ffn(*bad)


def test_parameters_of_an_fp8_expert_model():
    model = LlamaForCausalLM(mc.moe_config(), CPU,
                             expert_weight_dtype="fp8_e4m3")
    assert [(n, p.dtype, tuple(p.shape)) for n, p in model.named_parameters()
            if n.startswith("layers.1.mlp.")] == [
        ("layers.1.mlp.w_router", mc.BF16, (8, 512)),
        ("layers.1.mlp.w1", FP8, (8, 384, 512)),
        ("layers.1.mlp.w1_scale", torch.int8, (8, 384)),
        ("layers.1.mlp.w2", FP8, (8, 512, 192)),
        ("layers.1.mlp.w2_scale", torch.int8, (8, 512))]
    bf16 = LlamaForCausalLM(mc.moe_config(), CPU)
    assert [n for n, _ in bf16.named_parameters()
            if n.startswith("layers.1.mlp.")] == [
        "layers.1.mlp.w_router", "layers.1.mlp.w1", "layers.1.mlp.w2"]
    assert all(p.dtype == mc.BF16 for p in bf16.parameters())


def test_fp8_experts_quantise_the_bf16_model_of_the_seed():
    model = LlamaForCausalLM(mc.moe_config(), CPU,
                             expert_weight_dtype="fp8_e4m3")
    for seed in (1234, 99):
        if seed != 1234:
            model.reload_weights(seed)
        bf16 = LlamaForCausalLM(mc.moe_config(), CPU, base_seed=seed)
        for l8, l16 in zip(model.layers, bf16.layers):
            assert torch.equal(l8.mlp.w_router, l16.mlp.w_router)
            for name in ("w1", "w2"):
                w8, e, _ = quantise(getattr(l16.mlp, name).data)
                assert torch.equal(getattr(l8.mlp, name).view(torch.uint8),
                                   w8.view(torch.uint8))
                assert torch.equal(getattr(l8.mlp, name + "_scale"), e)


def test_option_is_checked_and_reaches_engine_and_stats(monkeypatch):
    for kw in (dict(model=ModelConfig.preset("tiny"),
                    expert_weight_dtype="fp8_e4m3"),
               dict(model=mc.moe_config(), expert_weight_dtype="int4"),
               dict(model=mc.moe_config(), expert_weight_dtype="fp8_e4m3",
                    weight_dtype="fp8_e4m3")):
        with pytest.raises(ValueError):
            EngineConfig(device="cpu", **kw)
    with pytest.raises(ValueError):
        LlamaForCausalLM(ModelConfig.preset("tiny"), CPU,
                         expert_weight_dtype="fp8_e4m3")
    assert EngineConfig(device="cpu").expert_weight_dtype == "bf16"
    monkeypatch.setattr(ModelConfig, "preset",
                        staticmethod(lambda name: mc.moe_config()))
    ctx = types.SimpleNamespace(gpu_ids=[], args={
        "model": "qwen3-30b-a3b", "expert_weight_dtype": "fp8_e4m3"})
    cfg = sw._engine_cfg(ctx)
    assert (cfg.expert_weight_dtype, cfg.weight_dtype) == ("fp8_e4m3", "bf16")

    class Worker(types.SimpleNamespace):
        def __getattr__(self, name):        # the RPC handlers not called here
            return None

    handlers = {}
    eng = fp8_engine("cpu")
    sw.ServeWorker._register_rpc(Worker(
        rpc=types.SimpleNamespace(register=handlers.__setitem__), engine=eng,
        cfg=eng.cfg, mode="colocated", _xfer_stats={"pushes": 0}))
    stats = handlers["stats"]()
    assert (stats["expert_weight_dtype"], stats["weight_dtype"]) == (
        "fp8_e4m3", "bf16")


def test_cpu_engine_generates_and_regenerates():
    prompts = [[7], list(range(17)), list(range(100, 140))]
    greedy = SamplingParams(max_new_tokens=4)
    first = [s.output_tokens for s in fp8_engine("cpu").generate(prompts,
                                                                 greedy)]
    assert all(len(t) == 4 for t in first)
    assert first == [s.output_tokens for s in
                     fp8_engine("cpu").generate(prompts, greedy)]
