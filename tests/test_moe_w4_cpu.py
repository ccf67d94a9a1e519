"""MXFP4 expert weights on the CPU (docs/FEATURES.md "MXFP4 experts"): the
quantiser against the format's definition, the op's CPU path, the model's
parameters and the option's way from a role argument to the stats RPC.
quantise(), w4_case() and w4_engine() also serve tests/test_moe_w4_gpu.py."""
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

CPU = torch.device("cpu")
# code = s eem: exponent field 0 is 0 or 0.5, else (1 + m / 2) * 2^(ee - 1)
TABLE = [(-1.0 if c & 8 else 1.0) *
         ((c & 1) * 0.5 if not c & 6 else
          (1 + (c & 1) / 2) * 2.0 ** (((c >> 1) & 3) - 1)) for c in range(16)]


def quantise(w):
    """bf16 [E, N, K] -> (codes [E, N, K/2], int8 [E, N, K/32], dq bf16)."""
    q, e = ops.quantize_weight_mxfp4(w.view(-1, w.shape[2]))
    dq = ops.dequantize_weight_mxfp4(q, e)
    return (q.view(*w.shape[:2], -1), e.view(*w.shape[:2], -1),
            dq.view(w.shape))


def w4_case(case, family):
    """(x, w1_4, w2_4, ids, w, e1, e2) and the bf16 twin's (dq1, dq2)."""
    x, w1, w2, ids, w = mc.ffn_case(case, family)
    (w1_4, e1, dq1), (w2_4, e2, dq2) = quantise(w1), quantise(w2)
    return (x, w1_4, w2_4, ids, w, e1, e2), (dq1, dq2)


def w4_engine(device, eager=True, dtype="mxfp4"):
    return LLMEngine(EngineConfig(
        model=mc.moe_config(), device=device, page_size=16,
        kv_pool_tokens=2048, max_batch_size=8, max_seq_len=256,
        enforce_eager=eager, expert_weight_dtype=dtype))


@pytest.mark.parametrize("e", (-64, -3, 0, 2, 64))
def test_dequantise_is_the_table_times_2_e(e):
    lo = torch.arange(16, dtype=torch.uint8).repeat(16)      # [256]: all pairs
    hi = torch.arange(16, dtype=torch.uint8).repeat_interleave(16)
    codes = (lo | (hi << 4)).view(1, 256)
    exps = torch.full((1, 16), e, dtype=torch.int8)
    dq = ops.dequantize_weight_mxfp4(codes, exps).double().view(256, 2)
    table = torch.tensor(TABLE, dtype=torch.float64) * 2.0 ** e
    assert torch.equal(dq[:, 0], table[lo.long()])
    assert torch.equal(dq[:, 1], table[hi.long()])


def test_midpoints_round_to_the_even_code():
    w = torch.zeros(2, 32)
    w[:, 0] = 6.0                                             # e = 0
    w[0, 1:8] = torch.tensor([0.25, 0.75, 1.25, 1.75, 2.5, 3.5, 5.0])
    w[1] = -w[0]
    q, e = ops.quantize_weight_mxfp4(w.to(mc.BF16))
    dq = ops.dequantize_weight_mxfp4(q, e)
    assert dq[0, 1:8].tolist() == [0, 1, 1, 2, 2, 4, 4]
    assert torch.equal(dq[1], -dq[0])


def test_block_exponents_and_saturation():
    amax = [6.0, 7.0, 3.0, 4.0, 0.5 * 2.0 ** -70, 6 * 2.0 ** 70, 0.0]
    w = torch.zeros(1, 32 * len(amax))
    w[0, 5::32] = -torch.tensor(amax)
    w[0, 6::32] = w[0, 5::32] / -4
    q, e = ops.quantize_weight_mxfp4(w.to(mc.BF16))
    assert e.tolist() == [[0, 1, -1, 0, -64, 64, 0]]
    dq = ops.dequantize_weight_mxfp4(q, e).double()
    # 6 * 2^70 and its quarter both saturate at 6 * 2^64; 2^-71 and its
    # quarter are 2^-7 and 2^-9 of the clamped scale: 0
    assert dq[0, 5::32].tolist() == [-6, -8, -3, -4, 0, -6 * 2.0 ** 64, 0]
    assert dq[0, 6::32].tolist() == [1.5, 2, 0.75, 1, 0, 6 * 2.0 ** 64, 0]


def test_quantiser_round_trip_and_rejects():
    g = torch.Generator().manual_seed(0)
    q = torch.randint(0, 256, (24, 48), generator=g).to(torch.uint8)
    q[:, ::16] |= 7                     # a 6 per block: e survives the trip
    e = torch.randint(-64, 65, (24, 3), generator=g).to(torch.int8)
    q2, e2 = ops.quantize_weight_mxfp4(ops.dequantize_weight_mxfp4(q, e))
    assert torch.equal(q2, q) and torch.equal(e2, e)
    for bad in (torch.zeros(4, 48), torch.zeros(4, 64, 2),
                torch.full((4, 64), float("inf")),
                torch.full((4, 64), float("nan"))):
        with pytest.raises(ValueError):
            ops.quantize_weight_mxfp4(bad.to(mc.BF16))


@pytest.mark.parametrize("case", mc.FFN_CASES[:2], ids=str)
def test_cpu_op_is_the_reference_on_dq(case):
    args, (dq1, dq2) = w4_case(case, "scaled")
    x, w1, w2, ids, w, e1, e2 = args
    assert torch.equal(ops.moe_ffn(*args),
                       ops.reference.moe_ffn(x, dq1, dq2, ids, w))
    for bad in (args[:5], args[:6], (x, w1, dq2, ids, w, e1, None),
                (x, w1, w2.view(torch.float8_e4m3fn), ids, w, e1, e2),
                (x, w1[:, :, :-16].contiguous(), w2, ids, w, e1, e2),
                (x, w1, w2[:, :, :-16].contiguous(), ids, w, e1, e2),
                (x, w1, w2, ids, w, e1[:, :, 0].contiguous(), e2[:, :, 0]),
                args[:6] + (e2.int(),),
                args[:6] + (e2[:, :-1].contiguous(),),
                args[:6] + (e2.transpose(1, 2).contiguous().transpose(1, 2),)):
        with pytest.raises(ValueError):
            ops.moe_ffn(*bad)


def test_option_reaches_model_engine_and_stats(monkeypatch):
    model = LlamaForCausalLM(mc.moe_config(), CPU, expert_weight_dtype="mxfp4")
    assert [(n, p.dtype, tuple(p.shape)) for n, p in model.named_parameters()
            if n.startswith("layers.1.mlp.")] == [
        ("layers.1.mlp.w_router", mc.BF16, (8, 512)),
        ("layers.1.mlp.w1", torch.uint8, (8, 384, 256)),
        ("layers.1.mlp.w1_scale", torch.int8, (8, 384, 16)),
        ("layers.1.mlp.w2", torch.uint8, (8, 512, 96)),
        ("layers.1.mlp.w2_scale", torch.int8, (8, 512, 6))]
    model.reload_weights(99)
    bf16 = LlamaForCausalLM(mc.moe_config(), CPU, base_seed=99)
    for l4, l16 in zip(model.layers, bf16.layers):
        assert torch.equal(l4.mlp.w_router, l16.mlp.w_router)
        for name in ("w1", "w2"):
            q, e, _ = quantise(getattr(l16.mlp, name).data)
            assert torch.equal(getattr(l4.mlp, name), q)
            assert torch.equal(getattr(l4.mlp, name + "_scale"), e)
    for kw in (dict(model=ModelConfig.preset("tiny"),
                    expert_weight_dtype="mxfp4"),
               dict(model=mc.moe_config(), weight_dtype="mxfp4"),
               dict(model=ModelConfig.preset("tiny"), weight_dtype="mxfp4"),
               dict(model=mc.moe_config(), expert_weight_dtype="mxfp4",
                    weight_dtype="fp8_e4m3")):
        with pytest.raises(ValueError):
            EngineConfig(device="cpu", **kw)
    monkeypatch.setattr(ModelConfig, "preset",
                        staticmethod(lambda name: mc.moe_config()))
    cfg = sw._engine_cfg(types.SimpleNamespace(gpu_ids=[], args={
        "model": "qwen3-30b-a3b", "expert_weight_dtype": "mxfp4"}))
    assert (cfg.expert_weight_dtype, cfg.weight_dtype) == ("mxfp4", "bf16")

    class Worker(types.SimpleNamespace):
        def __getattr__(self, name):        # the RPC handlers not called here
            return None

    handlers = {}
    eng = w4_engine("cpu")
    sw.ServeWorker._register_rpc(Worker(
        rpc=types.SimpleNamespace(register=handlers.__setitem__), engine=eng,
        cfg=eng.cfg, mode="colocated", _xfer_stats={"pushes": 0}))
    assert handlers["stats"]()["expert_weight_dtype"] == "mxfp4"


def test_cpu_engine_generates_the_tokens_of_a_bf16_engine_on_dq():
    prompts = [[7], list(range(17)), list(range(100, 140))]
    e4, e16 = w4_engine("cpu"), w4_engine("cpu", dtype="bf16")
    for l4, l16 in zip(e4.runner.model.layers, e16.runner.model.layers):
        for name in ("w1", "w2"):
            p, e = getattr(l4.mlp, name), getattr(l4.mlp, name + "_scale")
            getattr(l16.mlp, name).data.copy_(ops.dequantize_weight_mxfp4(
                p.data.view(-1, p.shape[2]),
                e.data.view(-1, e.shape[2])).view(*p.shape[:2], -1))
    runs = [[s.output_tokens for s in
             eng.generate(prompts, SamplingParams(max_new_tokens=4))]
            for eng in (e4, e16)]
    assert all(len(t) == 4 for t in runs[0]) and runs[0] == runs[1]
