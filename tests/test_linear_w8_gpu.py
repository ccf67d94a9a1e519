"""FP8 (e4m3) projection weights on the GPU (hip/skinny_gemm_w8.hip;
docs/FEATURES.md "FP8 weights").

  bit contract  skinny_gemm_w8(a, w8, e, s) against skinny_gemm(a, dq, s),
                which test_kernel_conformance_gpu.py pins against fp64
  independent   integer inputs (exact) and the shared fp64 bound at the
                automatic split policy, N up to 129 panels
  fused         ops.linear_add_rmsnorm on (w8, e) against the same op on dq
  M > 128       dequantise + library, and the dequant kernel on every byte
  rejects       host-side checks: nothing is launched
  engine        an fp8-weight engine against the bf16 engine that carries dq
"""
import pytest
import torch

import kernel_cases as kc
import model_cases as mc
import rbg_amd.ops as ops
from rbg_amd.engine.engine import LLMEngine
from rbg_amd.ops import reference

pytestmark = pytest.mark.gpu

FP8 = torch.float8_e4m3fn
W8_MS = (1, 16, 17, 64, 65, 128)   # both MTW values, a clamped last row in each
W8_NS = (64, 192)
AUTO_NK = ((768, 2048), (1536, 1024), (4096, 512), (8256, 512))
AUTO_MS = (1, 17, 128)
FUSED_NK = ((512, 1024),           # one split: the plain fused norm
            (4096, 512))           # two splits: the fold inside the norm
FINITE = torch.tensor([c for c in range(256) if c & 0x7f != 0x7f],
                      dtype=torch.uint8)            # no NaN code; -0 stays
PROJECTIONS = (("attn", "wqkv"), ("attn", "wo"), ("mlp", "w_gate_up"),
               ("mlp", "w_down"))
EPS = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    assert ops.HAVE_HIP, f"HIP extension missing: {ops._hip_err!r}"
    return torch.device("cuda:0")


def _random_w8(N, K, g, dev):
    """Bytes uniform over the 254 finite codes, a different exponent in
    [-9, 3] per row, and the bf16 weight they stand for (by the CPU
    reference)."""
    w8 = FINITE[torch.randint(0, 254, (N, K), generator=g)].view(FP8)
    e = torch.randint(-9, 4, (N,), generator=g).to(torch.int8)
    dq = reference.dequantize_weight_e4m3(w8, e)
    return w8.to(dev), e.to(dev), dq.to(dev)


@pytest.mark.parametrize("M", W8_MS)
def test_w8_equals_bf16_kernel_on_dq(dev, M):
    """Every instantiation at 2 stages per split (the prologue alone) and at
    6 (the ring loop, left after a pair)."""
    fails = []
    for N in W8_NS:
        for s in kc.GEMM_SPLITS:
            for kmul in kc.GEMM_KMULS:
                K = s * kmul
                g = kc._gen(("w8", M, N, K))
                a = torch.randn(M, K, generator=g).to(kc.BF16).to(dev)
                w8, e, dq = _random_w8(N, K, g, dev)
                got = ops._hip.skinny_gemm_w8(a, w8, e, s)
                if not kc.bits_equal(got, ops._hip.skinny_gemm(a, dq, s)):
                    fails.append("m%d-n%d-k%d-s%d" % (M, N, K, s))
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("M", AUTO_MS)
@pytest.mark.parametrize("N,K", AUTO_NK)
def test_w8_is_a_gemm_at_the_automatic_policy(dev, M, N, K):
    case = kc.GemmCase(M, N, K, 0)
    # integer: A, W in {-1, 0, 1} are lossless in e4m3, the rows scaled by
    # different powers of two: exact
    data = kc.gemm_data(case, "integer")
    e = torch.randint(-9, 4, (N,), generator=kc._gen(("w8e", N))).to(torch.int8)
    got = ops._hip.skinny_gemm_w8(data["a"].to(dev), data["w"].to(FP8).to(dev),
                                  e.to(dev))
    want = torch.ldexp(data["want"].double(), e.int()).to(dev)
    ok, msg, _ = kc.exact_check(got.double(), want, "w8 integer")
    assert ok, msg
    # scaled: the quantiser's own (w8, e) against fp64 on dq
    data = kc.gemm_data(case, "scaled")
    a = data["a"].to(dev)
    w8, e = ops.quantize_weight_e4m3(data["w"])
    dq = reference.dequantize_weight_e4m3(w8, e).to(dev).double()
    got = ops._hip.skinny_gemm_w8(a, w8.to(dev), e.to(dev))
    ok, msg, _ = kc.check_gemm(got, {
        "family": "scaled", "K": K, "ref64": a.double() @ dq.T,
        "S": a.double().abs() @ dq.abs().T})
    assert ok, msg


@pytest.mark.parametrize("M", (1, 40, 128))
@pytest.mark.parametrize("N,K", FUSED_NK)
def test_fused_add_rmsnorm_equals_bf16_op_on_dq(dev, M, N, K):
    g = kc._gen(("w8_fused", M, N))
    a = torch.randn(M, K, generator=g).to(kc.BF16).to(dev)
    w8, e, dq = _random_w8(N, K, g, dev)
    res = torch.randn(M, N, generator=g).to(kc.BF16).to(dev)
    nw = (torch.rand(N, generator=g) + 0.5).to(kc.BF16).to(dev)
    want_res, got_res = res.clone(), res.clone()
    want = ops.linear_add_rmsnorm(a, dq, want_res, nw, EPS)
    got = ops.linear_add_rmsnorm(a, w8, got_res, nw, EPS, e)
    assert kc.bits_equal(got, want) and kc.bits_equal(got_res, want_res)
    assert not kc.bits_equal(got_res, res), "residual was not updated"


@pytest.mark.parametrize("M,N,K", [(129, 8256, 512),     # grid-stride tail
                                   (158, 192, 272)])
def test_large_m_is_the_library_on_dq(dev, M, N, K):
    g = kc._gen(("w8_large", M))
    x = torch.randn(M, K, generator=g).to(kc.BF16).to(dev)
    w8, e, dq = _random_w8(N, K, g, dev)
    assert torch.equal(ops.linear(x, w8, e), torch.nn.functional.linear(x, dq))


@pytest.mark.parametrize("K", (256, 272))
def test_dequant_kernel_on_every_finite_code(dev, K):
    e = torch.tensor([-64, -3, 0, 2, 64], dtype=torch.int8)
    w8 = FINITE[torch.arange(5 * K).view(5, K) % 254].view(FP8)
    want = reference.dequantize_weight_e4m3(w8, e)
    assert want.float().abs().max() == 448.0 * 2.0 ** 64
    got = ops._hip.w8_dequant(w8.to(dev), e.to(dev))
    assert kc.bits_equal(got.cpu(), want)


def test_rejects_launch_nothing(dev):
    g = kc._gen("w8_rejects")
    M, N, K = 16, 128, 1024
    a = torch.randn(M, K, generator=g).to(kc.BF16).to(dev)
    w8, e, dq = _random_w8(N, K, g, dev)
    control = ops._hip.skinny_gemm_w8(a, w8, e)
    with pytest.raises(ValueError, match="w_scale_log2"):
        ops.linear(a, dq, e)
    with pytest.raises(ValueError, match="w_scale_log2"):
        ops.linear(a, w8)
    fn = ops._hip.skinny_gemm_w8
    wide = torch.zeros(N, 2 * K, dtype=torch.uint8, device=dev).view(FP8)
    for bad, match in (
            ((a, w8, e.int()), "e must be int8"),
            ((a, w8, e[:-1]), "one exponent per row"),
            ((a, w8, e.cpu()), "one device"),
            ((a, wide[:, :K], e), "w8 must be contiguous"),
            ((a, w8[:96], e[:96]), "multiple of 64"),
            ((torch.zeros(129, K, dtype=kc.BF16, device=dev), w8, e),
             r"M must be in \[1, 128\]"),
            ((a, w8, e, 3), "force_splits"),
            ((a, w8, e, 8), r"multiple of splits \* 256")):
        with pytest.raises(RuntimeError, match=match):
            fn(*bad)
    res = torch.ones(M, N, dtype=kc.BF16, device=dev)
    with pytest.raises(RuntimeError, match="e must be int8"):
        ops._hip.skinny_gemm_w8_add_rmsnorm(a, w8, e.int(), res, res[0], EPS)
    with pytest.raises(RuntimeError, match="multiple of 16"):
        ops._hip.w8_dequant(w8[:, :8].contiguous(), e)
    torch.cuda.synchronize()
    assert bool((res == 1).all()), "a rejected call wrote to residual"
    assert kc.bits_equal(ops._hip.skinny_gemm_w8(a, w8, e), control)


class _CountingHip:
    """ops._hip with every call counted by name."""

    def __init__(self, hip):
        self._hip, self.calls = hip, {}

    def __getattr__(self, name):
        fn = getattr(self._hip, name)

        def counted(*args, **kw):
            self.calls[name] = self.calls.get(name, 0) + 1
            return fn(*args, **kw)
        return counted


@pytest.mark.parametrize("eager", (True, False), ids=("eager", "graph"))
@pytest.mark.parametrize("conf", mc.CONFS)
def test_engine_equals_bf16_engine_on_dq(dev, conf, eager, monkeypatch):
    e8 = LLMEngine(mc.engine_config(conf, "cuda", eager,
                                    weight_dtype="fp8_e4m3"))
    e16 = LLMEngine(mc.engine_config(conf, "cuda", eager))
    for l8, l16 in zip(e8.runner.model.layers, e16.runner.model.layers):
        for mod, name in PROJECTIONS:
            m8, w16 = getattr(l8, mod), getattr(getattr(l16, mod), name)
            w8, scale = getattr(m8, name), getattr(m8, name + "_scale")
            assert w8.dtype == FP8 and scale.dtype == torch.int8
            assert (w8.numel() + scale.numel() ==
                    w16.numel() * w16.element_size() // 2 + w16.shape[0])
            w16.copy_(w8.dequantize())
    out = []
    for eng in (e8, e16):
        mc.draw_norm_weights(eng.runner.model)
        hip = _CountingHip(ops._hip)
        monkeypatch.setattr(ops, "_hip", hip)
        # one prefill of 158 rows (dequant + library), then a lone 40-token
        # prompt (the w8 kernel at M = 40); decode at M = 4 and M = 1
        seqs = [s for i in (0, 1) for s in eng.generate(
            mc._prompts(100 + i, mc.MIXED_BATCHES[i]), mc._greedy(6))]
        monkeypatch.undo()
        out.append(([s.output_tokens for s in seqs], hip.calls,
                    eng.runner.cache.kv.view(torch.int16).clone()))
    (tok8, calls8, kv8), (tok16, calls16, kv16) = out
    assert tok8 == tok16 and all(len(t) == 6 for t in tok8)
    assert torch.equal(kv8, kv16)
    assert calls8["skinny_gemm_w8"] and calls8["skinny_gemm_w8_add_rmsnorm"]
    assert calls8["w8_dequant"]
    assert not {"skinny_gemm", "skinny_gemm_add_rmsnorm"} & set(calls8)
    assert calls16["skinny_gemm"] and calls16["skinny_gemm_add_rmsnorm"]
    assert not any(name.endswith("w8") or "w8_" in name for name in calls16)
