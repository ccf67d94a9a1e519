"""FP8 (e4m3) expert weights on the GPU (hip/moe.hip, WT = uint8_t): the
e4m3 grouped GEMMs against the bf16 kernels on the dequantised weights (bit
for bit), against fp64, and through the engine."""
import pytest
import torch

import rbg_amd.ops as ops
import test_moe_cpu as mc
import test_moe_w8_cpu as w8
from rbg_amd.engine.sequence import SamplingParams

pytestmark = pytest.mark.gpu

# 3 and 12 steps with 0 / 1 / 15 / 16 / 17 / 33 / 65 rows (both sides of the
# MT = 1 / MT = 4 switch), several passes with clamped last tiles, full
# passes at k = 7, and one token
CASES = [mc.FFN_CASES[1], mc.FFN_CASES[4], mc.FFN_CASES[5],
         (8, 2, 256, 64, (0, 1, 0, 0, 0, 1, 0, 0))]


def all_codes(shape, seed):
    """Bytes uniform over the 254 finite e4m3 codes (subnormals and -0
    included) and a different exponent in [-12, -6] per row."""
    g = torch.Generator().manual_seed(seed)
    c = torch.randint(0, 254, shape, generator=g)
    c = (c + (c >= 127)).to(torch.uint8).view(torch.float8_e4m3fn)
    e = torch.randint(-12, -5, shape[:2], generator=g).to(torch.int8)
    assert bool(torch.isfinite(c.float()).all()) and e.unique().numel() == 7
    return c, e, ops.dequantize_weight_e4m3(
        c.view(-1, shape[2]), e.view(-1)).view(shape)


def case_on_gpu(case, family):
    if family == "all-codes":
        E, k, H, I, _ = case
        x, _, _, ids, w = mc.ffn_case(case, "scaled")
        (w1, e1, dq1), (w2, e2, dq2) = (all_codes((E, 2 * I, H), 1),
                                        all_codes((E, H, I), 2))
        args = (x, w1, w2, ids, w, e1, e2)
    else:
        args, (dq1, dq2) = w8.w8_case(case, family)
    return [t.cuda() for t in args], (dq1.cuda(), dq2.cuda())


@pytest.mark.parametrize("family", ("scaled", "all-codes"))
@pytest.mark.parametrize("case", CASES, ids=str)
def test_twin(case, family):
    args, dq = case_on_gpu(case, family)
    x, _, _, ids, w = args[:5]
    y = ops.moe_ffn(*args)
    assert bool(torch.isfinite(y.float()).all()) and float(y.abs().max()) > 0
    assert torch.equal(y, ops.moe_ffn(x, *dq, ids, w))
    flipped = ops.moe_ffn(*(t.flip(0).contiguous() if i in (0, 3, 4) else t
                            for i, t in enumerate(args)))
    assert torch.equal(flipped.flip(0), y)
    assert ops.moe_ffn(x[:0], args[1], args[2], ids[:0], w[:0],
                       *args[5:]).shape == (0, case[2])


@pytest.mark.parametrize("family", ("integer", "scaled"))
@pytest.mark.parametrize("case", CASES, ids=str)
def test_reference(case, family):
    args, dq = case_on_gpu(case, family)
    x, _, _, ids, w = args[:5]
    if family == "integer":
        # lossless, with a non-zero exponent on every row that has a value
        # (gate rows 2^-3 .. 2^-1 by their 32 / 64 / -128, up and w2 2^-8)
        _, w1, w2, _, _ = mc.ffn_case(case, family)
        for full, d, e in zip((w1, w2), dq, args[5:]):
            assert torch.equal(d.cpu(), full)
            assert torch.equal(e.cpu() != 0, (full != 0).any(2))
        assert args[5].unique().numel() >= 4
    mc.check_ffn((x, *dq, ids, w), family, ops.moe_ffn(*args))


def bad_w8_args(args, dq, name):
    """(w1, w2, e1, e2) of every reject docs/FEATURES.md lists."""
    _, w1, w2, _, _, e1, e2 = args
    return {
        "no_scales": (w1, w2, None, None),
        "no_w2_scale": (w1, w2, e1, None),
        "scale_on_bf16": (dq[0], dq[1], e1, e2),
        "mixed_dtypes": (w1, dq[1], e1, None),
        "scale_dtype": (w1, w2, e1.int(), e2),
        "scale_shape": (w1, w2, e1, e2[:, :-1].contiguous()),
        "scale_strided": (w1, w2, e1.t().contiguous().t(), e2),
        "scale_device": (w1, w2, e1, e2.cpu()),
    }[name]


def test_rejects():
    args, dq = case_on_gpu(CASES[0], "scaled")
    x, _, _, ids, w = args[:5]
    grouping = ops._hip.moe_group(ids, 8)
    for name in ("no_scales", "no_w2_scale", "scale_on_bf16", "mixed_dtypes",
                 "scale_dtype", "scale_shape", "scale_strided",
                 "scale_device"):
        w1, w2, e1, e2 = bad_w8_args(args, dq, name)
        with pytest.raises(ValueError):
            ops.moe_ffn(x, w1, w2, ids, w, e1, e2)
        with pytest.raises(RuntimeError):
            ops._hip.moe_ffn(x, w1, w2, w, *grouping, e1, e2)
    assert torch.equal(ops.moe_ffn(*args), ops.moe_ffn(x, *dq, ids, w))


@pytest.mark.parametrize("eager", (True, False), ids=("eager", "graph"))
def test_engine_equals_bf16_engine_on_dq(eager, monkeypatch):
    prompts = [[7], list(range(17)), list(range(100, 140))]
    seen, ffn = [], ops._hip.moe_ffn
    monkeypatch.setattr(ops._hip, "moe_ffn", lambda *a: (
        seen.append((a[1].dtype, a[2].dtype, len(a))), ffn(*a))[1])
    e8 = w8.fp8_engine("cuda", eager)
    e16 = w8.fp8_engine("cuda", eager, dtype="bf16")
    for l8, l16 in zip(e8.runner.model.layers, e16.runner.model.layers):
        for name in ("w1", "w2"):
            p, e = getattr(l8.mlp, name), getattr(l8.mlp, name + "_scale")
            assert p.dtype == torch.float8_e4m3fn
            getattr(l16.mlp, name).data.copy_(ops.dequantize_weight(
                p.data.view(-1, p.shape[2]), e.data.view(-1)).view(p.shape))
    runs = []
    for eng in (e8, e16):
        del seen[:]
        seqs = eng.generate(prompts, SamplingParams(max_new_tokens=7))
        # (page 0: the scratch page a graph's padding rows write)
        runs.append(([s.output_tokens for s in seqs],
                     eng.runner.cache.kv[:, :, 1:].view(torch.int16).clone()))
        want = ((torch.float8_e4m3fn,) * 2 + (8,) if eng is e8
                else (torch.bfloat16,) * 2 + (6,))
        assert seen and set(seen) == {want}, set(seen)
    assert all(len(t) == 7 for t in runs[0][0])
    assert runs[0][0] == runs[1][0]
    assert torch.equal(runs[0][1], runs[1][1])
