"""Conformance of the skinny GEMM, RMSNorm, SwiGLU and RoPE/KV-store kernels
(MI355X; marked gpu).

Inputs, fp64 references, bounds and checks come from tests/kernel_cases.py,
whose CPU self-test (tests/test_kernel_cases_cpu.py) shows that they accept a
correct kernel and reject each wrong one.  Two kinds of check exist: exact
equality (one-hot and integer GEMMs, spike zeros, saturated gates,
quarter-turn rotations, every copy), and the bounds derived in
kernel_cases' docstring from u = 2^-8 and the fp32 arithmetic.  Each test
prints its worst error / bound (run with -s).
"""
import pytest
import torch

import kernel_cases as kc
import rbg_amd.ops as ops

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    assert ops.HAVE_HIP, f"HIP extension missing: {ops._hip_err!r}"
    return torch.device("cuda:0")


def _report(kernel, worst):
    for family, ratio in sorted(worst.items()):
        print("CONF %s %s worst err/bound %.3f" % (kernel, family, ratio))


# ---------------------------------------------------------------------------
# skinny GEMM
# ---------------------------------------------------------------------------

def _run_gemm_case(case, dev, fails, worst):
    for family in kc.GEMM_FAMILIES:
        data = kc.gemm_data(case, family)
        for a, w, exp in kc.gemm_batches(data, dev):
            L = max(a.shape[0], w.shape[0])
            outs = [ops._hip.skinny_gemm(a[l if a.shape[0] > 1 else 0],
                                         w[l if w.shape[0] > 1 else 0],
                                         case.force) for l in range(L)]
            ok, msg, ratio = kc.check_gemm(torch.stack(outs), exp)
            worst[family] = max(worst.get(family, 0.0), ratio)
            if not ok:
                fails.append("%s %s" % (case.id, msg))
                break


@pytest.mark.parametrize("splits", kc.GEMM_SPLITS)
@pytest.mark.parametrize("M", kc.GEMM_MS)
def test_gemm_forced_splits(dev, M, splits):
    """All five M_TILES (each with a clamped last row) x every SPLITS
    instantiation, at the shortest pipeline the host allows (4 steps) and in
    steady state (12), on one, two and three 32-column panels.  The needle
    families put a one-hot at every k; the integer family is exact in any
    summation order; scaled and sparse use the derived bound."""
    fails, worst = [], {}
    for case in kc.GEMM_CASES:
        if case.M == M and case.force == splits:
            _run_gemm_case(case, dev, fails, worst)
    _report("skinny_gemm", worst)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("nk", kc.GEMM_AUTO_NK, ids=lambda nk: "n%d-k%d" % nk)
def test_gemm_automatic_splits(dev, nk):
    """force_splits = 0 on shapes where the launcher picks 8, 4, 2 and 1."""
    fails, worst = [], {}
    for case in kc.GEMM_CASES:
        if not case.force and (case.N, case.K) == nk:
            _run_gemm_case(case, dev, fails, worst)
    _report("skinny_gemm_auto", worst)
    assert not fails, "\n".join(fails)


def test_gemm_rejects_bad_splits_and_ranks(dev):
    """Host-side checks: nothing is launched."""
    a = torch.zeros(16, 4096, dtype=kc.BF16, device=dev)
    w = torch.zeros(32, 4096, dtype=kc.BF16, device=dev)
    for bad in (16, 3, 5, 6, 7, -1, 32):
        with pytest.raises(RuntimeError, match="force_splits"):
            ops._hip.skinny_gemm(a, w, bad)
    a768 = torch.zeros(16, 768, dtype=kc.BF16, device=dev)
    w768 = torch.zeros(32, 768, dtype=kc.BF16, device=dev)
    for bad in (2, 4, 8):           # 768 is not a multiple of splits * 256
        with pytest.raises(RuntimeError, match="multiple of force_splits"):
            ops._hip.skinny_gemm(a768, w768, bad)
    with pytest.raises(RuntimeError, match="force_splits"):
        ops._hip.skinny_gemm(a768, w768, 3)
    with pytest.raises(RuntimeError, match="2-D"):
        ops._hip.skinny_gemm(a.view(2, 8, 4096), w, 0)
    with pytest.raises(RuntimeError, match="2-D"):
        ops._hip.skinny_gemm(a, w.view(32, 4096, 1), 0)
    with pytest.raises(RuntimeError, match="2-D"):
        ops._hip.skinny_gemm(a[0], w, 0)
    # the valid neighbours still run
    assert ops._hip.skinny_gemm(a768, w768, 1).shape == (16, 32)
    assert ops._hip.skinny_gemm(a, w, 8).shape == (16, 32)


LINEAR_SHAPES = ((128, 4608), (129, 4608), (128, 4640), (64, 8192),
                 (65, 8192))


@pytest.mark.parametrize("M,N", LINEAR_SHAPES)
def test_linear_noncontiguous_x_each_side_of_the_limits(dev, M, N):
    """ops.linear on a column slice of a wider buffer, one shape on each
    side of the M and N dispatch limits: the custom kernel and the library
    both have to meet the GEMM bound."""
    K = 512
    g = kc._gen(("linear", M, N))
    wide = (torch.randn(M, 2 * K + 8, generator=g) * 0.5).to(kc.BF16).to(dev)
    x = wide[:, K + 8:]
    assert not x.is_contiguous() and x.shape == (M, K)
    w = (torch.randn(N, K, generator=g) * 0.05).to(kc.BF16).to(dev)
    got = ops.linear(x, w)
    exp = {"family": "scaled", "K": K,
           "ref64": x.double() @ w.double().T,
           "S": x.double().abs() @ w.double().abs().T}
    ok, msg, ratio = kc.check_gemm(got, exp)
    print("CONF linear m%d-n%d worst err/bound %.3f" % (M, N, ratio))
    assert ok, msg


def test_linear_with_no_rows_returns_empty(dev):
    x = torch.zeros(0, 512, dtype=kc.BF16, device=dev)
    w = torch.zeros(64, 512, dtype=kc.BF16, device=dev)
    out = ops.linear(x, w)
    assert out.shape == (0, 64) and out.dtype == kc.BF16


# ---------------------------------------------------------------------------
# rmsnorm / fused_add_rmsnorm
# ---------------------------------------------------------------------------

def _run_norm(case, dev):
    data = kc.norm_data(case)
    x = data["x"].to(dev)
    w = data["w"].to(dev)
    if case.fused:
        res = data["res"].to(dev)
        ops._hip.fused_add_rmsnorm(x, res, w, case.eps)
        return kc.check_norm(x, res, data)
    x_before = x.clone()
    out = ops._hip.rmsnorm(x, w, case.eps)
    assert kc.bits_equal(x, x_before), "rmsnorm wrote to its input"
    return kc.check_norm(out, None, data)


@pytest.mark.parametrize("fused", (False, True), ids=("norm", "fused"))
@pytest.mark.parametrize("H", kc.NORM_HS)
def test_norm_matrix(dev, H, fused):
    """spike: one non-zero per row, at every element (or one lane of every
    8-chunk), three heights x eps in {0, 1e-5}: a chunk missing from the sum
    of squares sends that row to inf/huge, and everything off the spike must
    be exactly 0.  scaled: randn rows of scale 1e-3, 1, 1e3 with randn
    weights, T = 1 and 3.  H = 8 .. 136 leave three of the block's four
    waves idle; 2056 is one vector past a full block."""
    fails, worst = [], {}
    for case in kc.NORM_CASES:
        if case.H == H and case.fused == fused and len(case.shape) == 2 \
                and case.shape != kc.NORM_QK_SHAPE:
            ok, msg, ratio = _run_norm(case, dev)
            worst[case.family] = max(worst.get(case.family, 0.0), ratio)
            if not ok:
                fails.append("%s: %s" % (case.id, msg))
    _report("fused_add_rmsnorm" if fused else "rmsnorm", worst)
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("fused", (False, True), ids=("norm", "fused"))
@pytest.mark.parametrize("shape", (kc.NORM_QK_SHAPE, kc.NORM_3D_SHAPE),
                         ids=("qk-norm", "3d"))
def test_norm_call_shapes(dev, shape, fused):
    """The QK-norm call shape (tokens x heads rows of 128) and a 3-D input."""
    case = next(c for c in kc.NORM_CASES
                if c.shape == shape and c.fused == fused)
    ok, msg, ratio = _run_norm(case, dev)
    print("CONF %s %s worst err/bound %.3f" % (
        "fused_add_rmsnorm" if fused else "rmsnorm", case.id, ratio))
    assert ok, msg


def test_norm_rejects_bad_weight_and_residual(dev):
    """Host-side checks: nothing is launched."""
    x = torch.zeros(4, 128, dtype=kc.BF16, device=dev)
    res = torch.zeros(4, 128, dtype=kc.BF16, device=dev)
    w = torch.ones(128, dtype=kc.BF16, device=dev)
    bad_weights = (
        (torch.ones(120, dtype=kc.BF16, device=dev), "hidden elements"),
        (torch.ones(136, dtype=kc.BF16, device=dev), "hidden elements"),
        (torch.ones(128, dtype=torch.float32, device=dev), "bf16"),
        (torch.ones(128, dtype=kc.BF16), "GPU"),
        (torch.ones(256, dtype=kc.BF16, device=dev)[::2], "contiguous"),
    )
    for bad, match in bad_weights:
        with pytest.raises(RuntimeError, match=match):
            ops._hip.rmsnorm(x, bad, 1e-5)
        with pytest.raises(RuntimeError, match=match):
            ops._hip.fused_add_rmsnorm(x, res, bad, 1e-5)
    for bad in (torch.zeros(3, 128, dtype=kc.BF16, device=dev),
                torch.zeros(4, 136, dtype=kc.BF16, device=dev),
                torch.zeros(2, 2, 128, dtype=kc.BF16, device=dev)):
        with pytest.raises(RuntimeError, match="shape mismatch"):
            ops._hip.fused_add_rmsnorm(x, bad, w, 1e-5)
    assert not x.any() and not res.any()


def test_norm_with_no_tokens_launches_nothing(dev):
    x = torch.zeros(0, 128, dtype=kc.BF16, device=dev)
    w = torch.ones(128, dtype=kc.BF16, device=dev)
    assert ops._hip.rmsnorm(x, w, 1e-5).shape == (0, 128)
    ops._hip.fused_add_rmsnorm(x, x.clone(), w, 1e-5)
    torch.cuda.synchronize()
    # no launch error was left behind for the next call to trip over
    one = torch.ones(1, 128, dtype=kc.BF16, device=dev)
    assert torch.equal(ops._hip.rmsnorm(one, w, 0.0), one)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------
# silu_mul
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("family", kc.SILU_FAMILIES)
@pytest.mark.parametrize("case", kc.SILU_CASES, ids=lambda c: c.id)
def test_silu_matrix(dev, case, family):
    """switch: gates of 32 / 0 / -100 give exactly 32 * up / 0 / 0.  scaled:
    gates uniform in [-16, 16] under (u + 2^-16).  The last case has 17.2 M
    outputs, past the 8192-block grid cap, so the grid-stride loop runs;
    inputs and the fp64 reference are built on the device."""
    x = kc.silu_input(case, family, dev)
    x_before = x.clone()
    got = ops._hip.silu_mul(x)
    assert kc.bits_equal(x, x_before), "silu_mul wrote to its input"
    ok, msg, ratio = kc.check_silu(got, x, family)
    print("CONF silu_mul %s %s worst err/bound %.3f" % (family, case.id,
                                                        ratio))
    assert ok, msg


@pytest.mark.parametrize("family", kc.SILU_FAMILIES)
def test_silu_keeps_leading_dimensions(dev, family):
    x = kc.silu_input(kc.SiluCase(6, 24), family, dev)
    flat = ops._hip.silu_mul(x)
    got = ops._hip.silu_mul(x.view(2, 3, 48))
    assert got.shape == (2, 3, 24)
    assert kc.bits_equal(got.reshape(6, 24), flat)
    ok, msg, _ = kc.check_silu(got.reshape(6, 24), x, family)
    assert ok, msg
    assert ops._hip.silu_mul(x.view(-1)[:48]).shape == (24,)
    assert ops._hip.silu_mul(x[:0]).shape == (0, 24)


# ---------------------------------------------------------------------------
# rope_store_kv
# ---------------------------------------------------------------------------

PAD = 8          # columns after q|k|v in the fused buffer nobody may touch
PAD_VALUE = 7.0


def _rope_inputs(data, layout, dev):
    case = data["case"]
    T = case.T
    if layout == "contiguous":
        return (data["q"].to(dev), data["k"].to(dev), data["v"].to(dev),
                None)
    qw, kw = case.qh * kc.ROPE_D, case.kvh * kc.ROPE_D
    qkv = torch.full((T, qw + 2 * kw + PAD), PAD_VALUE, dtype=kc.BF16,
                     device=dev)
    q = qkv[:, :qw].view(T, case.qh, kc.ROPE_D)
    k = qkv[:, qw:qw + kw].view(T, case.kvh, kc.ROPE_D)
    v = qkv[:, qw + kw:qw + 2 * kw].view(T, case.kvh, kc.ROPE_D)
    q.copy_(data["q"])
    k.copy_(data["k"])
    v.copy_(data["v"])
    assert T == 1 or not q.is_contiguous()
    return q, k, v, qkv


@pytest.mark.parametrize("layout", ("contiguous", "fused-qkv"))
@pytest.mark.parametrize("family", kc.ROPE_FAMILIES)
@pytest.mark.parametrize("case", kc.ROPE_CASES, ids=lambda c: c.id)
def test_rope_store_kv_matrix(dev, case, family, layout):
    """quarter: a table of quarter turns makes the rotation an exact
    sign/swap permutation (position routing, the (d, d + 64) pairing, the
    sign of sin).  scaled: the real table with positions 0 and max - 1.  In
    both, the pool starts as finite poison and slot_mapping is permuted with
    -1 entries: written V rows equal v, written K rows equal the rotated k,
    and every other slot keeps its poison bit for bit."""
    data = kc.rope_data(case, family)
    q, k, v, qkv = _rope_inputs(data, layout, dev)
    kcache, vcache = kc.rope_pool(data, dev)
    ops._hip.rope_store_kv(q, k, v, kcache, vcache, data["table"].to(dev),
                           data["pos"].to(dev), data["slots"].to(dev))
    ok, msg, ratio = kc.check_rope(q, k, kcache, vcache, data)
    print("CONF rope_store_kv %s %s %s worst err/bound %.3f" % (
        family, case.id, layout, ratio))
    assert ok, msg
    assert torch.equal(v, data["v"].to(dev)), "v was modified"
    if qkv is not None:
        assert bool((qkv[:, -PAD:] == PAD_VALUE).all())
