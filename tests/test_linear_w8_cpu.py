"""FP8 (e4m3) projection weights on the CPU: the exponent rule, TP shards,
reload, the config option and a whole engine against the bf16 engine that
carries the dequantised weights (docs/FEATURES.md "FP8 weights")."""
import pytest
import torch

from rbg_amd import ops
from rbg_amd.engine.config import EngineConfig, ModelConfig
from rbg_amd.engine.engine import LLMEngine
from rbg_amd.models.llama import LlamaForCausalLM, TPContext

import model_cases as mc

BF16 = torch.bfloat16
PROJECTIONS = (("attn", "wqkv"), ("attn", "wo"), ("mlp", "w_gate_up"),
               ("mlp", "w_down"))


def _row(amax):
    return torch.tensor([[amax, -amax / 2, 0.0, amax / 4]], dtype=BF16)


# 224 = 0.875 * 2^8 is 448 * 2^-1 exactly, so the smallest e with
# amax <= 448 * 2^e is -1 (the rule of the format, in both its statements)
@pytest.mark.parametrize("amax,e,top", [
    (448.0, 0, 448.0), (450.0, 1, 224.0), (224.0, -1, 448.0),
    (448.0 * 2 ** -3, -3, 448.0), (0.0, 0, 0.0),
    (2.0 ** 100, 64, 448.0)])       # clamped at 64: the row saturates
def test_exponent_rule(amax, e, top):
    w8, got = ops.quantize_weight_e4m3(_row(amax))
    assert got.dtype == torch.int8 and got.tolist() == [e]
    assert w8.dtype == torch.float8_e4m3fn
    sat = amax > 448.0 * 2.0 ** 64      # then amax / 4 saturates as well
    assert w8.float()[0].tolist() == [
        top, -top if sat else -top / 2, 0.0, top if sat else top / 4]


def test_dequantised_weight_requantises_to_itself():
    g = torch.Generator().manual_seed(5)
    w = (torch.randn(64, 256, generator=g) *
         torch.logspace(-3, 3, 64, base=2.0).unsqueeze(1)).to(BF16)
    w[7] = 0
    dq = ops.dequantize_weight_e4m3(*ops.quantize_weight_e4m3(w))
    assert dq.dtype == BF16 and not torch.equal(dq, w)
    assert torch.equal(ops.dequantize_weight_e4m3(
        *ops.quantize_weight_e4m3(dq)), dq)
    assert (dq - w).abs().max() <= 2.0 ** -4 * w.abs().max()


def test_tp_shards_are_slices_of_the_tp1_model():
    cfg = ModelConfig.preset("tiny-tp")
    dev = torch.device("cpu")
    full = LlamaForCausalLM(cfg, dev, weight_dtype="fp8_e4m3")
    ranks = [LlamaForCausalLM(cfg, dev, TPContext(2, r),
                              weight_dtype="fp8_e4m3") for r in (0, 1)]

    def parts(model, mod, name):
        m = getattr(model.layers[1], mod)
        return (getattr(m, name).view(torch.uint8),
                getattr(m, name + "_scale"))

    # row-sharded: bytes and exponents by rows; column-sharded: bytes by
    # columns under all the exponents
    w, e = parts(full, "mlp", "w_gate_up")
    halves = [parts(m, "mlp", "w_gate_up") for m in ranks]
    for blk in (0, 1):          # gate rows, then up rows
        wb, eb = w.chunk(2)[blk], e.chunk(2)[blk]
        for r, (wr, er) in enumerate(halves):
            assert torch.equal(wr.chunk(2)[blk], wb.chunk(2)[r])
            assert torch.equal(er.chunk(2)[blk], eb.chunk(2)[r])
    w, e = parts(full, "mlp", "w_down")
    for r, m in enumerate(ranks):
        wr, er = parts(m, "mlp", "w_down")
        assert torch.equal(wr, w.chunk(2, dim=1)[r]) and torch.equal(er, e)


def test_reload_rebuilds_an_fp8_model():
    cfg = ModelConfig.preset("tiny")
    dev = torch.device("cpu")
    model = LlamaForCausalLM(cfg, dev, weight_dtype="fp8_e4m3")
    before = [p.detach().clone() for p in model.parameters()]
    model.reload_weights(mc.RELOAD_SEED)
    fresh = LlamaForCausalLM(cfg, dev, base_seed=mc.RELOAD_SEED,
                             weight_dtype="fp8_e4m3")
    pairs = list(zip(model.parameters(), fresh.parameters()))
    assert len(pairs) == len(before)
    for p, q in pairs:
        assert p.dtype == q.dtype and not p.requires_grad
        assert torch.equal(p.view(torch.uint8), q.view(torch.uint8))
    assert any(p.dtype == torch.float8_e4m3fn and
               not torch.equal(p.view(torch.uint8), b.view(torch.uint8))
               for p, b in zip(model.parameters(), before))


def test_options_and_half_pairs_are_rejected():
    with pytest.raises(ValueError, match="weight_dtype"):
        EngineConfig(weight_dtype="int4")
    x = torch.zeros(2, 256, dtype=BF16)
    w8, e = ops.quantize_weight_e4m3(torch.ones(64, 256, dtype=BF16))
    with pytest.raises(ValueError, match="w_scale_log2"):
        ops.linear(x, w8)
    with pytest.raises(ValueError, match="w_scale_log2"):
        ops.linear(x, torch.ones(64, 256, dtype=BF16), e)
    # N = 2 * 3 * 128 per fused qkv row block is fine; 96 rows are not
    bad = ModelConfig(name="bad", hidden_size=96, intermediate_size=128,
                      num_layers=1, num_heads=1, num_kv_heads=1,
                      head_dim=128, vocab_size=64, max_position=64)
    with pytest.raises(ValueError, match="64"):
        LlamaForCausalLM(bad, torch.device("cpu"), weight_dtype="fp8_e4m3")


@pytest.mark.parametrize("conf", mc.CONFS)
def test_cpu_engine_equals_bf16_engine_on_dq(conf):
    e8 = LLMEngine(mc.engine_config(conf, "cpu", True,
                                    weight_dtype="fp8_e4m3"))
    e16 = LLMEngine(mc.engine_config(conf, "cpu", True))
    for l8, l16 in zip(e8.runner.model.layers, e16.runner.model.layers):
        for mod, name in PROJECTIONS:
            w8 = getattr(getattr(l8, mod), name)
            assert w8.dtype == torch.float8_e4m3fn
            getattr(getattr(l16, mod), name).copy_(w8.dequantize())
    toks = []
    for eng in (e8, e16):
        mc.draw_norm_weights(eng.runner.model)
        seqs = eng.generate(mc._prompts(77, (1, 17, 40)), mc._greedy(6))
        toks.append([s.output_tokens for s in seqs])
    assert toks[0] == toks[1] and all(len(t) == 6 for t in toks[0])
    assert torch.equal(e8.runner.cache.kv.view(torch.int16),
                       e16.runner.cache.kv.view(torch.int16))
