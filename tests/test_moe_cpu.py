"""Mixture of experts on the CPU (docs/FEATURES.md "Mixture of experts"): the
torch references against fp64, the argument checks, the engine with the
`conf-moe` model.  The case builders and fp64 references here also serve
tests/test_moe_gpu.py."""
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
             (4, 2, 768, 64, (16, 16, 0, 0))]


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
        x[1, 0::3] = float("nan")
        x[1, 1::3] = float("-inf")
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
    return (x.to(BF16), w1.to(BF16), w2.to(BF16), ids,
            w.float().contiguous())


def rel_l2(y, ref):
    return float((y.double().cpu() - ref).norm() / ref.norm())


def check_ffn(args, family, y):
    if family == "integer":
        ref = ffn_f64(*args, switch_silu)[1]
        assert torch.equal(y.float().cpu(), ref.float())
        return
    ref = ffn_f64(*args)[1]
    cpu = [t.cpu() for t in args]
    err, base = rel_l2(y, ref), rel_l2(ops.reference.moe_ffn(*cpu), ref)
    print("moe_ffn rel L2: %.3e, reference %.3e, ratio %.2f"
          % (err, base, err / base))
    assert err <= FACTOR * base


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


@pytest.mark.parametrize("E,k,T,renorm", [c for c in ROUTE_CASES
                                          if c[0] != 128 and c[2] == 37])
def test_reference_route(E, k, T, renorm):
    logits = route_logits(E, T)
    check_route(*ops.moe_route(logits, k, renorm), logits, k, renorm)


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
