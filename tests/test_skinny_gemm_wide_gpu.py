"""The 64-column-panel skinny GEMM and the split-K fold fused into
add + RMSNorm (MI355X; marked gpu).

Both are pure re-schedulings of arithmetic the older kernels already do, so
every check here is torch.equal, no tolerance:

  wide vs narrow   skinny_gemm(panel=64) against panel=32 at the same
                   (M, N, K, splits): each output element is the same two
                   MFMA chains per split, added in f32, folded over splits in
                   ascending order and rounded once.
  fused vs unfused skinny_gemm_add_rmsnorm against skinny_gemm followed by
                   fused_add_rmsnorm: same fold, same rounding to bf16 before
                   the residual add, same reduction tree.

Inputs are kernel_cases' "scaled" family; the narrow kernel itself is held to
the fp64 reference by tests/test_kernel_conformance_gpu.py.
"""
import pytest
import torch

import kernel_cases as kc
import rbg_amd.ops as ops

pytestmark = pytest.mark.gpu

WIDE_MS = (1, 17, 128)            # one row, a clamped last tile, the full tile
WIDE_NS = (64, 128, 192)          # one panel, two panels, an odd panel count
WIDE_AUTO = (128, 4096, 1024)     # (M, N, K): the launcher picks 4 splits
FUSED_NKF = ((64, 512, 1),        # splits == 1: plain GEMM + the existing norm
             (96, 1024, 2),       # N % 64 != 0: the 32-column kernel
             (128, 2048, 8),      # 8 splits; the 64-column kernel at M = 128
             (4096, 1024, 0))     # automatic: 4 splits, 64 columns at M = 128
EPS = 1e-5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    assert ops.HAVE_HIP, f"HIP extension missing: {ops._hip_err!r}"
    return torch.device("cuda:0")


def _scaled(M, N, K, force, dev):
    data = kc.gemm_data(kc.GemmCase(M, N, K, force), "scaled")
    return data["a"].to(dev), data["w"].to(dev)


@pytest.mark.parametrize("M", WIDE_MS)
def test_wide_panel_equals_narrow(dev, M):
    """Every SPLITS instantiation of both MTW variants (M <= 64 and M > 64)
    at the shortest pipeline the host allows (4 steps per split) and at 12
    steps, where the four-deep W ring wraps three times."""
    fails = []
    for N in WIDE_NS:
        for s in kc.GEMM_SPLITS:
            for kmul in kc.GEMM_KMULS:
                a, w = _scaled(M, N, s * kmul, s, dev)
                wide = ops._hip.skinny_gemm(a, w, s, panel=64)
                narrow = ops._hip.skinny_gemm(a, w, s, panel=32)
                if not kc.bits_equal(wide, narrow):
                    fails.append("m%d-n%d-k%d-s%d: %d elements differ" % (
                        M, N, s * kmul, s, int((wide != narrow).sum())))
    assert not fails, "\n".join(fails)


def test_wide_panel_equals_narrow_auto_splits(dev):
    M, N, K = WIDE_AUTO
    assert kc.pick_gemm_splits(N, K) == 4
    a, w = _scaled(M, N, K, 0, dev)
    wide = ops._hip.skinny_gemm(a, w, panel=64)
    assert kc.bits_equal(wide, ops._hip.skinny_gemm(a, w, panel=32))
    assert kc.bits_equal(wide, ops._hip.skinny_gemm(a, w, 4, 64))
    # and the result is a GEMM: the shared bound against fp64
    data = kc.gemm_data(kc.GemmCase(M, N, K, 0), "scaled")
    ok, msg, _ = kc.check_gemm(wide, {
        "family": "scaled", "K": K, "ref64": data["ref64"].to(dev),
        "S": data["S"].to(dev)})
    assert ok, msg


def test_wide_panel_rejects_unsupported_shapes(dev):
    """Host-side checks: nothing is launched."""
    a = torch.zeros(16, 512, dtype=kc.BF16, device=dev)
    w96 = torch.zeros(96, 512, dtype=kc.BF16, device=dev)
    with pytest.raises(RuntimeError, match="panel 64"):
        ops._hip.skinny_gemm(a, w96, 0, panel=64)
    a129 = torch.zeros(129, 512, dtype=kc.BF16, device=dev)
    w64 = torch.zeros(64, 512, dtype=kc.BF16, device=dev)
    with pytest.raises(RuntimeError, match="panel 64"):
        ops._hip.skinny_gemm(a129, w64, 0, panel=64)
    for bad in (16, 48, 128, -1):
        with pytest.raises(RuntimeError, match="panel must be"):
            ops._hip.skinny_gemm(a, w64, 0, panel=bad)
    # the valid neighbours still run
    assert ops._hip.skinny_gemm(a, w96, 0, panel=32).shape == (16, 96)
    assert ops._hip.skinny_gemm(a129, w64, 0, panel=32).shape == (129, 64)
    assert ops._hip.skinny_gemm(a, w64, 0, panel=64).shape == (16, 64)


def _norm_inputs(M, N, dev):
    g = kc._gen(("gemm_add_rmsnorm", M, N))
    res = torch.randn(M, N, generator=g).to(kc.BF16).to(dev)
    nw = (torch.rand(N, generator=g) + 0.5).to(kc.BF16).to(dev)
    return res, nw


@pytest.mark.parametrize("M", WIDE_MS)
def test_gemm_add_rmsnorm_equals_two_calls(dev, M):
    fails = []
    for N, K, force in FUSED_NKF:
        a, w = _scaled(M, N, K, force, dev)
        res, nw = _norm_inputs(M, N, dev)
        want_h = ops._hip.skinny_gemm(a, w, force)
        want_res = res.clone()
        ops._hip.fused_add_rmsnorm(want_h, want_res, nw, EPS)
        got_res = res.clone()
        got_h = ops._hip.skinny_gemm_add_rmsnorm(a, w, got_res, nw, EPS,
                                                 force)
        for what, got, want in (("h", got_h, want_h),
                                ("residual", got_res, want_res)):
            if not kc.bits_equal(got, want):
                fails.append("m%d-n%d-k%d-s%d %s: %d elements differ" % (
                    M, N, K, force, what, int((got != want).sum())))
        assert not kc.bits_equal(got_res, res), "residual was not updated"
    assert not fails, "\n".join(fails)


def test_gemm_add_rmsnorm_rejects_bad_arguments(dev):
    """Host-side checks: nothing is launched, nothing is written."""
    M, N, K = 16, 128, 1024
    a = torch.zeros(M, K, dtype=kc.BF16, device=dev)
    w = torch.zeros(N, K, dtype=kc.BF16, device=dev)
    res = torch.ones(M, N, dtype=kc.BF16, device=dev)
    nw = torch.ones(N, dtype=kc.BF16, device=dev)
    fn = ops._hip.skinny_gemm_add_rmsnorm
    for bad in (torch.ones(M + 1, N, dtype=kc.BF16, device=dev),
                torch.ones(M, N + 8, dtype=kc.BF16, device=dev),
                torch.ones(M * N, dtype=kc.BF16, device=dev),
                torch.ones(1, M, N, dtype=kc.BF16, device=dev)):
        with pytest.raises(RuntimeError, match=r"residual must be \[M, N\]"):
            fn(a, w, bad, nw, EPS)
    for bad in (torch.ones(N - 8, dtype=kc.BF16, device=dev),
                torch.ones(N + 8, dtype=kc.BF16, device=dev)):
        with pytest.raises(RuntimeError, match="N elements"):
            fn(a, w, res, bad, EPS)
    with pytest.raises(RuntimeError, match="residual must be bf16"):
        fn(a, w, res.float(), nw, EPS)
    with pytest.raises(RuntimeError, match="norm_weight must be bf16"):
        fn(a, w, res, nw.float(), EPS)
    with pytest.raises(RuntimeError, match="a must be bf16"):
        fn(a.float(), w, res, nw, EPS)
    with pytest.raises(RuntimeError, match="residual must be contiguous"):
        fn(a, w, torch.ones(M, 2 * N, dtype=kc.BF16, device=dev)[:, :N], nw,
           EPS)
    with pytest.raises(RuntimeError, match="force_splits"):
        fn(a, w, res, nw, EPS, 3)
    with pytest.raises(RuntimeError, match="panel 64"):
        fn(torch.zeros(129, K, dtype=kc.BF16, device=dev), w,
           torch.ones(129, N, dtype=kc.BF16, device=dev), nw, EPS, 0, 64)
    torch.cuda.synchronize()
    assert bool((res == 1).all()), "a rejected call wrote to residual"
    # the valid call still runs: a zero GEMM leaves residual and norms ones
    h = fn(a, w, res, nw, 0.0, 2)
    assert bool((res == 1).all()) and bool((h == 1).all())
