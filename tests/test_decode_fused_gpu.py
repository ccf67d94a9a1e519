"""Decode attention with the splits merged inside the workgroup (MI355X;
marked gpu).

At 2 or 4 splits the page-pair MFMA kernels (bf16 variant 4 and the fp8
kernel) can run the splits of one (sequence, kv head) as the waves of one
workgroup and merge them through LDS (`combine = 2`) instead of writing f32
partials for decode_combine_kernel (`combine = 1`).  Both run the same merge
function over the same partial values in the same order, so every comparison
here is torch.equal on the bf16 bits: there is no tolerance in this file.

Inputs are the decode cases of tests/attn_cases.py (contexts 1 .. 2047 and a
ctx = 0 row, GQA groups 1/2/4/8, 1/2/8 kv heads, batches of 1 and 3; ctx = 1
at 4 splits leaves three empty waves, ctx = 17 at 2 splits a one-key second
wave) and their e4m3 quantisations by tests/kvfp8_cases.py.
"""
import pytest
import torch

import attn_cases as ac
import kvfp8_cases as k8
import rbg_amd.ops as ops

pytestmark = pytest.mark.gpu

BF16 = torch.bfloat16
WG_SPLITS = (2, 4)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    assert ops.HAVE_HIP, f"HIP extension missing: {ops._hip_err!r}"
    return torch.device("cuda:0")


_DEV_CACHE = {}


def _on_dev(case, family, dev):
    """The case's tensors on the GPU, with its caches quantised at both
    exponent pairs (uploaded once, never modified)."""
    key = (case, family)
    if key not in _DEV_CACHE:
        data = ac.decode_data(case, family)
        d = {n: data[n].to(dev) for n in ("q", "kc", "vc", "bt", "ctx")}
        for ek, ev in k8.DECODE_EXPONENTS:
            d["kq", ek] = k8.q8(data["kc"], ek).to(dev)
            d["vq", ev] = k8.q8(data["vc"], ev).to(dev)
        _DEV_CACHE[key] = d
    return _DEV_CACHE[key]


def _bits(t):
    return t.view(torch.int16)


def _both(fn):
    """fn(combine) for the separate kernel and the in-workgroup merge."""
    want, got = fn(1), fn(2)
    assert want.dtype == BF16 and got.dtype == BF16
    return torch.equal(_bits(got), _bits(want))


def _compare_all(d, q):
    fails = []
    for splits in WG_SPLITS:
        if not _both(lambda c: ops.decode_attention(
                q, d["kc"], d["vc"], d["bt"], d["ctx"], ac.SCALE,
                num_splits=splits, variant=4, combine=c)):
            fails.append("bf16 variant 4, %d splits" % splits)
        for ek, ev in k8.DECODE_EXPONENTS:
            if not _both(lambda c: ops.decode_attention(
                    q, d["kq", ek], d["vq", ev], d["bt"], d["ctx"], ac.SCALE,
                    num_splits=splits, k_scale_log2=ek, v_scale_log2=ev,
                    combine=c)):
                fails.append("fp8 e=(%d, %d), %d splits" % (ek, ev, splits))
    return fails


@pytest.mark.parametrize("family", ac.DECODE_FAMILIES)
@pytest.mark.parametrize("case", ac.DECODE_CASES, ids=lambda c: c.id)
def test_combine_identity(dev, case, family):
    """combine = 2 equals combine = 1 bit for bit: bf16 variant 4 and the fp8
    kernel at exponent pairs (0, 0) and (-2, 3), 2 and 4 splits."""
    d = _on_dev(case, family, dev)
    fails = _compare_all(d, d["q"])
    assert not fails, fails


@pytest.mark.parametrize("family", ac.DECODE_FAMILIES)
@pytest.mark.parametrize("case", ac.DECODE_CASES, ids=lambda c: c.id)
def test_combine_identity_q_from_fused_qkv_slice(dev, case, family):
    """The same identity with q a column slice of a fused QKV buffer."""
    d = _on_dev(case, family, dev)
    R, QH, D = d["q"].shape
    width = (QH + 2 * case.kvh) * D
    qkv = torch.full((R, width), 3.0, dtype=BF16, device=dev)
    # as_strided: a one-row view would otherwise report a compact stride
    q = qkv.as_strided((R, QH, D), (width, D, 1))
    q.copy_(d["q"])
    assert q.stride(0) == width and q.data_ptr() == qkv.data_ptr()
    fails = _compare_all(d, q)
    assert not fails, fails
    # and the in-workgroup result is the right answer, not merely the same
    data = ac.decode_data(case, family)
    for splits in WG_SPLITS:
        got = ops.decode_attention(q, d["kc"], d["vc"], d["bt"], d["ctx"],
                                   ac.SCALE, num_splits=splits, variant=4,
                                   combine=2)
        ok, msg, _ = ac.check(got, data)
        assert ok, (splits, msg)


def test_auto_takes_the_in_workgroup_merge_and_allocates_no_partials(dev):
    """combine = 0 at 2 and 4 splits equals both forced modes, and asks the
    allocator for the output alone."""
    case = ac.DECODE_CASES[7]
    d = _on_dev(case, "scaled", dev)
    args = (d["q"], d["kc"], d["vc"], d["bt"], d["ctx"], ac.SCALE)
    out_bytes = d["q"].numel() * 2
    for splits in WG_SPLITS:
        want = ops.decode_attention(*args, num_splits=splits, variant=4,
                                    combine=1)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        got = ops.decode_attention(*args, num_splits=splits, variant=4)
        torch.cuda.synchronize()
        grown = torch.cuda.max_memory_allocated() - base
        assert torch.equal(_bits(got), _bits(want))
        # partials would add splits * rows * QH * (128 + 2) * 4 bytes
        assert grown < 2 * out_bytes + 4096, (splits, grown, out_bytes)


def test_combine_2_raises_where_no_kernel_has_it(dev):
    case = ac.DECODE_CASES[7]
    d = _on_dev(case, "scaled", dev)
    args = (d["q"], d["kc"], d["vc"], d["bt"], d["ctx"], ac.SCALE)
    fp8 = (d["q"], d["kq", 0], d["vq", 0], d["bt"], d["ctx"], ac.SCALE)
    for kw in (dict(num_splits=3, variant=4), dict(num_splits=1, variant=4),
               dict(num_splits=16, variant=4), dict(num_splits=2, variant=1),
               dict(num_splits=4, variant=5), dict(num_splits=2, variant=6)):
        with pytest.raises(RuntimeError):
            ops.decode_attention(*args, combine=2, **kw)
        # the other two modes run these
        ops.decode_attention(*args, combine=0, **kw)
        ops.decode_attention(*args, combine=1, **kw)
    for splits in (1, 3, 8):
        with pytest.raises(RuntimeError):
            ops.decode_attention(*fp8, num_splits=splits, combine=2)
    with pytest.raises(RuntimeError):
        ops.decode_attention(*args, num_splits=2, variant=4, combine=3)
    # a 32-token page has no page-pair kernel: variant 4 falls back to dot2
    kc32 = torch.zeros(4, case.kvh, 32, 128, dtype=BF16, device=dev)
    with pytest.raises(RuntimeError):
        ops._hip.decode_attention(d["q"], kc32, kc32.clone(),
                                  torch.zeros_like(d["bt"]),
                                  torch.ones_like(d["ctx"]), ac.SCALE, 2, 4, 2)
    torch.cuda.synchronize()
