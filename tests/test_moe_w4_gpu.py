"""MXFP4 experts on the GPU (hip/moe.hip, WT = mxfp4_t) against the bf16
kernels on the dequantised weights, bit for bit: no tolerance in this file."""
import pytest
import torch

import rbg_amd.ops as ops
import test_moe_cpu as mc
import test_moe_w4_cpu as w4
from rbg_amd.engine.sequence import SamplingParams

pytestmark = pytest.mark.gpu

# rows per expert: MT = 1 and MT = 4, a clamped last tile, one and two extra
# passes; and one token.  H: 4 and 12 steps of gate_up; I: 1, 3 and 5 steps of
# down (a lone half stage, an odd tail, an odd tail after a full ring turn)
COUNTS = ((1, (0, 1, 15, 16, 17, 65, 130, 0)), (2, (0, 1, 0, 0, 0, 1, 0, 0)))
CASES = [(8, k, H, I, c) for H in (256, 768) for I in (64, 192, 320)
         for k, c in COUNTS]


def all_codes(shape, seed, big):
    """Code bytes uniform over all 256 values, exponents uniform over
    [-8, 8] with single blocks at -64 and, if `big`, at 64 (in experts 1
    and 5, which every case routes to)."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randint(0, 256, shape, generator=g).to(torch.uint8)
    e = torch.randint(-8, 9, shape[:2] + (shape[2] // 16,), generator=g
                      ).to(torch.int8)
    e[1, 1, 0], e[5, -1, -1] = -64, 64 if big else -64
    assert q.unique().numel() == 256 and e.unique().numel() == 18 + big
    return q, e, ops.dequantize_weight_mxfp4(
        q.view(-1, shape[2]), e.view(-1, e.shape[2])).view(*shape[:2], -1)


def case_on_gpu(case, family):
    if family == "all-codes":
        E, k, H, I, _ = case
        x, _, _, ids, w = mc.ffn_case(case, "scaled")
        # the 2^64 block sits in w2 alone, and x is small: nothing overflows
        (w1, e1, dq1), (w2, e2, dq2) = (all_codes((E, 2 * I, H // 2), 1, 0),
                                        all_codes((E, H, I // 2), 2, 1))
        args = (x * 2.0 ** -12, w1, w2, ids, w, e1, e2)
    else:
        args, (dq1, dq2) = w4.w4_case(case, family)
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


@pytest.mark.parametrize("case", (CASES[2], CASES[10]), ids=str)
def test_integer_family_is_exact(case):
    args, dq = case_on_gpu(case, "integer")
    x, _, _, ids, w = args[:5]
    # lossless: the builder's 32 / 64 / -128 gates and +-1 are e2m1 * 2^e
    _, w1, w2, _, _ = mc.ffn_case(case, "integer")
    for full, d in zip((w1, w2), dq):
        assert torch.equal(d.cpu(), full)
    assert args[5].unique().numel() >= 4
    mc.check_ffn((x, *dq, ids, w), "integer", ops.moe_ffn(*args))


@pytest.mark.parametrize("eager", (True, False), ids=("eager", "graph"))
def test_engine_equals_bf16_engine_on_dq(eager, monkeypatch):
    prompts = [[7], list(range(17)), list(range(100, 140))]
    seen, ffn = [], ops._hip.moe_ffn
    monkeypatch.setattr(ops._hip, "moe_ffn", lambda *a: (
        seen.append((a[1].dtype, a[2].dtype, len(a))), ffn(*a))[1])
    e4 = w4.w4_engine("cuda", eager)
    e16 = w4.w4_engine("cuda", eager, dtype="bf16")
    for l4, l16 in zip(e4.runner.model.layers, e16.runner.model.layers):
        for name in ("w1", "w2"):
            p, e = getattr(l4.mlp, name), getattr(l4.mlp, name + "_scale")
            assert p.dtype == torch.uint8
            # no block exponent was clamped: dq is the nearest-grid model
            assert int(e.abs().max()) < 64
            getattr(l16.mlp, name).data.copy_(ops.dequantize_weight_mxfp4(
                p.data.cpu().view(-1, p.shape[2]),
                e.data.cpu().view(-1, e.shape[2])).view(*p.shape[:2], -1))
    runs = []
    for eng in (e4, e16):
        del seen[:]
        seqs = eng.generate(prompts, SamplingParams(max_new_tokens=7))
        # (page 0: the scratch page a graph's padding rows write)
        runs.append(([s.output_tokens for s in seqs],
                     eng.runner.cache.kv[:, :, 1:].view(torch.int16).clone()))
        want = ((torch.uint8,) * 2 + (8,) if eng is e4
                else (torch.bfloat16,) * 2 + (6,))
        assert seen and set(seen) == {want}, set(seen)
    assert all(len(t) == 7 for t in runs[0][0])
    assert runs[0][0] == runs[1][0]
    assert torch.equal(runs[0][1], runs[1][1])
