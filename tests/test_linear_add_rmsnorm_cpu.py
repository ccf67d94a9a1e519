"""ops.linear_add_rmsnorm and the model wiring built on it (CPU).

The op is defined as `h = linear(x, w); fused_add_rmsnorm(h, residual, ...)`;
off the custom-GEMM path it is literally that composition.  In the model,
o_proj takes the layer's post_norm and down_proj the NEXT layer's input_norm,
so a two-layer engine run pins the cross-layer hand-off: every logits row it
samples from and the whole KV pool must equal, bit for bit, the run with the
op replaced by the two calls and the run with the fusion switched off.
"""
import pytest
import torch

import kernel_cases as kc
import model_cases as mc
import rbg_amd.ops as ops
from rbg_amd.engine.engine import LLMEngine


def _two_calls(x, w, residual, norm_weight, eps):
    h = ops.linear(x, w)
    ops.fused_add_rmsnorm(h, residual, norm_weight, eps)
    return h


@pytest.mark.parametrize("M,N,K", ((1, 64, 512), (17, 96, 1024),
                                   (128, 128, 512), (130, 64, 256)))
def test_op_equals_two_calls(M, N, K):
    g = kc._gen(("linear_add_rmsnorm", M, N, K))
    x = (torch.randn(M, K, generator=g) * 0.5).to(kc.BF16)
    w = (torch.randn(N, K, generator=g) * 0.05).to(kc.BF16)
    res = torch.randn(M, N, generator=g).to(kc.BF16)
    nw = (torch.rand(N, generator=g) + 0.5).to(kc.BF16)
    want_res = res.clone()
    want_h = _two_calls(x, w, want_res, nw, 1e-5)
    got_res = res.clone()
    got_h = ops.linear_add_rmsnorm(x, w, got_res, nw, 1e-5)
    assert kc.bits_equal(got_h, want_h)
    assert kc.bits_equal(got_res, want_res)
    assert not kc.bits_equal(got_res, res)


def test_op_reaches_linear_through_the_module_attribute(monkeypatch):
    """tests/model_cases.py traces ops.linear by replacing the attribute."""
    seen = []
    linear = ops.linear
    monkeypatch.setattr(ops, "linear",
                        lambda x, w: seen.append(tuple(x.shape)) or
                        linear(x, w))
    x = torch.zeros(3, 512, dtype=kc.BF16)
    ops.linear_add_rmsnorm(x, torch.zeros(64, 512, dtype=kc.BF16),
                           torch.zeros(3, 64, dtype=kc.BF16),
                           torch.ones(64, dtype=kc.BF16), 1e-5)
    assert seen == [(3, 512)]


def _run(conf, monkeypatch, how):
    engine = LLMEngine(mc.engine_config(conf, "cpu", True))
    model = engine.runner.model
    mc.draw_norm_weights(model)
    assert len(model.layers) == 2
    fused = [(l.fuse_norms, l.input_prenormed, len(l.next_input_norm))
             for l in model.layers]
    assert fused == [(True, False, 1), (True, True, 0)]
    assert model.layers[0].next_input_norm[0] is model.layers[1].input_norm
    calls = []
    if how == "two_calls":
        monkeypatch.setattr(ops, "linear_add_rmsnorm",
                            lambda *a: calls.append(a[0].shape[0]) or
                            _two_calls(*a))
    elif how == "unfused":
        model.link_norm_fusion(False)
        monkeypatch.setattr(ops, "linear_add_rmsnorm", None)
    rows = []
    logits = model.logits
    monkeypatch.setattr(model, "logits", lambda *a, **k: (
        rows.append(logits(*a, **k)) or rows[-1]))
    seqs = engine.generate(mc._prompts(900, (5, 20, 33)), mc._greedy(4))
    # o_proj of both layers and down_proj of the first, prefill and decode
    assert how != "two_calls" or (len(calls) == 3 * 4 and 58 in calls)
    return ([s.output_tokens for s in seqs], rows,
            engine.runner.cache.kv.clone())


@pytest.mark.parametrize("conf", mc.CONFS)
def test_two_layer_model_equals_unfused_wiring(conf, monkeypatch):
    tokens, rows, kv = _run(conf, monkeypatch, "fused")
    assert len(rows) == 4 and all(len(t) == 4 for t in tokens)
    for how in ("two_calls", "unfused"):
        with monkeypatch.context() as mp:
            tokens2, rows2, kv2 = _run(conf, mp, how)
        assert tokens2 == tokens, how
        assert len(rows2) == len(rows)
        for a, b in zip(rows, rows2):
            assert torch.equal(a, b), how
        assert torch.equal(kv.view(torch.int16), kv2.view(torch.int16)), how
