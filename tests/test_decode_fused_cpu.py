"""`combine` of ops.decode_attention without a GPU: it reaches the extension's
entry points unchanged (default 0), and the CPU reference path, which has no
splits, ignores it.  The GPU side is tests/test_decode_fused_gpu.py."""
import pytest
import torch

import attn_cases as ac
import kvfp8_cases as k8
import rbg_amd.ops as ops

CASE = ac.DECODE_CASES[13]          # group 4, 2 kv heads, contexts 257, 1, 48


class _FakeTensor:
    """Stands in for a GPU tensor at ops' dispatch: ops looks at is_cuda,
    shape and dtype only before it hands the arguments on."""

    def __init__(self, t):
        self.t, self.is_cuda, self.shape, self.dtype = t, True, t.shape, t.dtype


class _FakeHip:
    def __init__(self):
        self.calls = []

    def decode_attention(self, *a):
        self.calls.append(("bf16", a))
        return "bf16-out"

    def decode_attention_fp8(self, *a):
        self.calls.append(("fp8", a))
        return "fp8-out"


@pytest.mark.parametrize("combine", (None, 0, 1, 2))
def test_combine_reaches_the_extension(monkeypatch, combine):
    d = ac.decode_data(CASE, "scaled")
    fake = _FakeHip()
    monkeypatch.setattr(ops, "_hip", fake)
    kw = {} if combine is None else {"combine": combine}
    want = 0 if combine is None else combine
    q = _FakeTensor(d["q"])
    out = ops.decode_attention(q, d["kc"], d["vc"], d["bt"], d["ctx"],
                               ac.SCALE, num_splits=2, variant=4, **kw)
    assert out == "bf16-out"
    kind, a = fake.calls[-1]
    assert kind == "bf16" and a[0] is q and a[6:] == (2, 4, want)
    kq, vq = k8.q8(d["kc"], -2), k8.q8(d["vc"], 3)
    out = ops.decode_attention(q, kq, vq, d["bt"], d["ctx"], ac.SCALE,
                               num_splits=4, k_scale_log2=-2, v_scale_log2=3,
                               **kw)
    assert out == "fp8-out"
    kind, a = fake.calls[-1]
    assert kind == "fp8" and a[6:] == (4, -2, 3, want)
    assert len(fake.calls) == 2


@pytest.mark.parametrize("combine", (0, 1, 2))
def test_cpu_path_ignores_combine(combine):
    d = ac.decode_data(CASE, "scaled")
    args = (d["q"], d["kc"], d["vc"], d["bt"], d["ctx"], ac.SCALE)
    want = ops.reference.decode_attention(*args)
    got = ops.decode_attention(*args, num_splits=2, combine=combine)
    assert torch.equal(got, want)
    ok, msg, _ = ac.check(got, d)
    assert ok, msg
