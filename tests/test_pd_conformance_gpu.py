"""P/D handoff conformance on the GPU (MI355X; marked gpu): the
`kv_peer_copy` kernel alone, `PeerKVPusher.push` and its refusals, and a
sequence followed across two engines against the dense fp64 forward.

Cases, harnesses and checks live in tests/pd_cases.py and are proven on the
CPU by tests/test_pd_cases_cpu.py (every mutant there fails a check).  Here
the same code runs with `device="cuda"`: the push is the kernel, both
engines run the HIP kernels, the decode engine also under hipGraphs.

  copy cases  the whole destination allocation, guard bands included,
              `torch.equal` the CPU-built expectation; source unchanged.
              One 5 GiB destination puts byte offsets beyond 2^32 and bf16
              element offsets beyond 2^31.  (Offsets beyond 2^31 16-byte
              vectors would need a 32 GiB pool; that the strides are `long`
              from the binding to the kernel is verified by reading.)
  rejects     the destination pool bit-identical and no launch counted.
  H1, H2      C0 to C4 of pd_cases, bound model_cases.FACTOR x e_cpu, and
              the paths each scenario is meant to reach.

Run with -s to see the measured err / e_cpu per scenario.
"""
import pytest
import torch

import kvfp8_model_cases as m8
import model_cases as mc
import pd_cases as pc
import rbg_amd.ops as ops
from rbg_amd.parallel import kv_peer

pytestmark = pytest.mark.gpu

MODES = ("eager", "graph")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    assert ops.HAVE_HIP, f"HIP extension missing: {ops._hip_err!r}"
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------
# 1. kv_peer_copy alone
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("case", pc.COPY_CASES, ids=lambda c: c.id)
def test_kv_peer_copy_case(dev, case):
    assert pc.run_copy_case(case, pc.hip_copy, "cuda") == []


def test_kv_peer_copy_of_no_pages_changes_nothing(dev):
    case = pc.COPY_CASES[2]
    su = pc.copy_setup(case)
    src = pc.as_pool(su.src_words.clone(), pc.BF16).to(dev)
    alloc = su.alloc.clone().to(dev)
    pc.hip_copy(alloc, su.guard_vec, src, [], [], case.pd)
    assert torch.equal(alloc.cpu(), su.alloc)
    assert torch.equal(src.cpu().view(-1).view(pc.I32).view(-1, 4),
                       su.src_words.view(-1, 4))


def test_kv_peer_copy_offsets_beyond_4gib(dev):
    """Destination [2, 2, 40960, 8, 16, 128] bf16 = 5 GiB, never filled:
    the last plane starts at 3.75 GiB, so its pages lie beyond 2^32 bytes
    and 2^31 elements."""
    free, _total = torch.cuda.mem_get_info(dev)
    if free < 16 << 30:
        pytest.skip("needs 16 GiB of free device memory, %.1f GiB free"
                    % (free / 2 ** 30))
    P, cv = 40960, 8 * 16 * 128 * 2 // 16
    dst = torch.empty((2, 2, P, 8, 16, 128), dtype=pc.BF16, device=dev)
    assert dst.numel() * 2 == 5 << 30
    assert dst[1, 1, P - 1].data_ptr() - dst.data_ptr() > 2 ** 32
    assert dst[1, 1, P - 1].storage_offset() > 2 ** 31
    src_words = pc.ramp(pc.SRC_TAG, 4, 8, cv)
    src = pc.as_pool(src_words, pc.BF16).reshape(2, 2, 8, 8, 16, 128).to(dev)
    other = pc.as_pool(pc.ramp(pc.DST_TAG, 4, 2, cv), pc.BF16).reshape(
        2, 2, 2, 8, 16, 128)
    kept = [2, P - 2]
    for i, page in enumerate(kept):         # plain slices: no index kernels
        dst[:, :, page].copy_(other[:, :, i])
    src_pages, dst_pages = [5, 0, 7], [0, 1, P - 1]
    ops._hip.kv_peer_copy(
        dst.data_ptr(), src,
        torch.tensor(src_pages, dtype=pc.I32, device=dev),
        torch.tensor(dst_pages, dtype=pc.I32, device=dev), P)
    torch.cuda.synchronize()
    got = torch.stack([dst[:, :, page] for page in dst_pages + kept],
                      dim=2).cpu()
    del dst
    torch.cuda.empty_cache()
    want = torch.cat([src.cpu()[:, :, src_pages], other], dim=2)
    for plane in range(4):
        assert torch.equal(pc.raw(got)[plane // 2, plane % 2],
                           pc.raw(want)[plane // 2, plane % 2]), plane
    assert torch.equal(pc.raw(src.cpu()),
                       pc.raw(pc.as_pool(src_words, pc.BF16)).reshape(
                           2, 2, 8, 8, 16, 128))


def _two_caches(conf, fp8, dev):
    kw = m8.FP8_KW if fp8 else {}
    src = mc.PagedKVCache(mc.engine_config(
        conf, "cuda", True, pool_tokens=pc.P_POOL, **kw), dev)
    dst = mc.PagedKVCache(mc.engine_config(
        conf, "cuda", True, pool_tokens=pc.D_POOL, **kw), dev)
    assert kv_peer.peer_capable(src) and kv_peer.peer_capable(dst)
    assert (src.kv.shape[2], dst.kv.shape[2]) == (128, 96)
    gen = torch.Generator().manual_seed(31)
    for cache, lo in ((src, 0), (dst, 128)):      # disjoint byte values
        pc.raw(cache.kv).copy_(torch.randint(
            lo, lo + 128, cache.kv.shape, generator=gen).to(
                pc.raw(cache.kv).dtype))
    return src, dst


@pytest.mark.parametrize("fp8", (False, True), ids=("bf16", "fp8"))
@pytest.mark.parametrize("conf", mc.CONFS)
def test_pusher_between_pools_of_different_size(dev, conf, fp8):
    src, dst = _two_caches(conf, fp8, dev)
    src_before = src.kv.cpu()
    gen = torch.Generator().manual_seed(32)
    src_pages = [0, 127] + torch.randperm(126, generator=gen)[:9].add(
        1).tolist()
    src_pages[4] = src_pages[3]                   # one page sent twice
    dst_pages = [95, 0] + torch.randperm(94, generator=gen)[:9].add(
        1).tolist()
    want = dst.kv.cpu()
    pc.raw(want).index_copy_(
        2, torch.tensor(dst_pages),
        pc.raw(src_before).index_select(2, torch.tensor(src_pages)))
    pending = kv_peer.PeerKVPusher(dev).push(
        src, src_pages, kv_peer.export_meta_local(dst), dst_pages)
    pending.wait()
    assert pending.nbytes == (len(src_pages) * src.kv[:, :, 0].numel() *
                              src.kv.element_size())
    assert torch.equal(pc.raw(dst.kv.cpu()), pc.raw(want))
    assert torch.equal(pc.raw(src.kv.cpu()), pc.raw(src_before))


# ---------------------------------------------------------------------------
# 2. refusals: nothing launched, nothing changed
# ---------------------------------------------------------------------------

def test_push_rejects_leave_the_destination_untouched(dev):
    src, dst = _two_caches("conf-llama", False, dev)
    before = dst.kv.cpu()
    meta = kv_peer.export_meta_local(dst)
    pusher = kv_peer.PeerKVPusher(dev)
    calls = []
    orig = ops._hip.kv_peer_copy
    with mc._patched(ops._hip, "kv_peer_copy",
                     lambda *a: calls.append(a) or orig(*a)):
        for why, (s, m, d) in pc.reject_cases(list(src.kv.shape),
                                              meta).items():
            with pytest.raises(ValueError):
                pusher.push(src, s, m, d)
            assert not calls, why
        # the control: a well-formed push is launched and does land
        pusher.push(src, [1], meta, [4]).wait()
        assert len(calls) == 1
    torch.cuda.synchronize()
    after = dst.kv.cpu()
    assert torch.equal(pc.raw(after)[:, :, 4], pc.raw(src.kv.cpu())[:, :, 1])
    pc.raw(after)[:, :, 4] = pc.raw(before)[:, :, 4]
    assert torch.equal(pc.raw(after), pc.raw(before))


def test_binding_rejects_null_base_and_empty_pool(dev):
    src, dst = _two_caches("conf-qwen", False, dev)
    before = dst.kv.cpu()
    one = torch.tensor([1], dtype=pc.I32, device=dev)
    for base, pages in ((0, 96), (dst.kv.data_ptr(), 0),
                        (dst.kv.data_ptr(), -1)):
        with pytest.raises(RuntimeError):
            ops._hip.kv_peer_copy(base, src.kv, one, one, pages)
    with pytest.raises(RuntimeError):       # page lists of unequal length
        ops._hip.kv_peer_copy(dst.kv.data_ptr(), src.kv, one,
                              torch.tensor([1, 2], dtype=pc.I32, device=dev),
                              96)
    torch.cuda.synchronize()
    assert torch.equal(pc.raw(dst.kv.cpu()), pc.raw(before))


# ---------------------------------------------------------------------------
# 3. two engines against the dense fp64 reference
# ---------------------------------------------------------------------------

H1_CASES = [(s, c, m) for c in mc.CONFS for s in pc.SCENARIOS for m in MODES]


def _judge_and_report(pair, what="e_cpu"):
    verdict = pc.judge_pair(pair)
    print("\n%s: worst err / %s logits %.3f, K/V %.3f (%d rows, %d blocks)"
          % ((pair.id, what) + verdict.worst() +
             (len(verdict.c1), len(verdict.c2))))
    assert not verdict.failures(), verdict.failures()[:8]


@pytest.mark.parametrize("scenario,conf,mode", H1_CASES)
def test_h1_handoff_matches_dense_fp64(dev, scenario, conf, mode):
    pair = pc.run_pair(scenario, conf, "cuda", mode == "eager")
    assert pair.graph_mode == (mode == "graph")
    pc.assert_same_weights(pair)
    pc.assert_paths(pair)
    _judge_and_report(pair)


@pytest.mark.parametrize("conf", mc.CONFS)
@pytest.mark.parametrize("mode", MODES)
def test_h1_fp8_handoff_matches_quantised_dense_fp64(dev, conf, mode):
    pair = pc.run_pair("handoff", conf, "cuda", mode == "eager", fp8=True)
    assert pair.pc.kv.dtype == pair.dc.kv.dtype == pc.FP8
    pc.assert_same_weights(pair)
    pc.assert_paths(pair)
    _judge_and_report(pair, "e_cpu8")


def test_h1_bf16_to_fp8_raises_before_any_byte_moves(dev):
    pair = pc.Pair("handoff", "conf-llama", "cuda", True, fp8=False,
                   d_fp8=True)
    with pc._count_kernel(pair):
        (req,) = pair.prefill(mc._prompts(700, (17,)), [2])
        with pytest.raises(ValueError, match="mismatched KV pools"):
            pair.migrate([req])
    torch.cuda.synchronize()
    assert pair.kernel_calls == 0
    assert torch.equal(pc.raw(pair.dc.kv.cpu()), pc.raw(pair.d_poison))


@pytest.mark.parametrize("conf", mc.CONFS)
@pytest.mark.parametrize("mode", MODES)
def test_h2_serving_handshake_matches_dense_fp64(dev, conf, mode):
    s = pc.run_serving(conf, "cuda", mode == "eager")
    assert s.graph_mode == (mode == "graph")
    pc.assert_same_weights(s)
    pc.assert_serving_paths(s)
    _judge_and_report(s)
