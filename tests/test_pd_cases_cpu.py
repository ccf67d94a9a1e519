"""CPU self-test of tests/pd_cases.py: the checks the GPU P/D conformance
tests apply must accept the project's own handoff and reject wrong ones.

  * the copy cases accept an emulation of `kv_peer_copy` that uses the
    kernel's own pointer arithmetic and reject it with the destination chunk
    stride taken from the source pool, exactly where the pools differ in
    size; equal-sized pools (all the suite had) cannot tell;
  * `PeerKVPusher.push` refuses every malformed push with ValueError before
    anything is mapped or launched (a stub extension whose `kv_peer_copy`
    raises);
  * the old `RBG_PD_VERIFY` sum accepts pages in reversed order, K and V
    swapped and layer l in l^1; the digest rejects all three;
  * H1 (`pd_bench`'s functions) and H2 (`ServeWorker`'s handshake) on two
    `device="cpu"` engines pass C0 to C4 and reach the paths they are meant
    to;
  * every mutant, patched in for the run only, fails a check in every
    scenario where it applies and is never a no-op there.

Run with -s to see the mutant table and the measured err / e_cpu.
"""
import functools
import threading
import types

import pytest
import torch

import model_cases as mc
import pd_cases as pc
from rbg_amd.engine import pd_bench
from rbg_amd.parallel import kv_peer


# ---------------------------------------------------------------------------
# copy cases
# ---------------------------------------------------------------------------

def test_copy_cases_cover_every_axis_value():
    cases = pc.COPY_CASES
    assert {c.chunk_vec for c in cases} == set(pc.CHUNK_VECS)
    assert {c.layers for c in cases} == {1, 2, 3}
    assert {(c.ps, c.pd) for c in cases} == set(pc.POOL_PAGES)
    assert {c.dtype for c in cases} == {"bf16", "fp8"}
    assert {c.kind for c in cases} == set(pc.KINDS)
    assert {c.n for c in cases} == {1, 2, 7, pc.FULL}
    assert len({c.id for c in cases}) == len(cases)
    # both thread counts meet a ragged tail, a sub-pass chunk and both dtypes
    for lo, hi in ((1, 255), (256, 2048)):
        group = [c for c in cases if lo <= c.chunk_vec <= hi]
        assert {c.dtype for c in group} == {"bf16", "fp8"}
        assert any(c.chunk_vec % (64 if hi == 255 else 256) for c in group)
    # page 0 and the last page of each pool, a repeated source page
    src, dst = pc.page_lists(cases[4])
    assert {0, 39} <= set(src) and {0, 23} <= set(dst)
    for c in cases:
        src, dst = pc.page_lists(c)
        assert len(set(dst)) == len(dst) == min(c.n, c.ps, c.pd)
        assert all(0 <= p < c.ps for p in src)
        assert all(0 <= p < c.pd for p in dst)
        if c.kind == "dup_src":
            assert src[0] == src[1]


def test_ramp_vectors_are_unique_and_disjoint():
    a = pc.ramp(pc.SRC_TAG, 6, 5, 7).view(-1, 4)
    b = pc.ramp(pc.DST_TAG, 6, 5, 7).view(-1, 4)
    g = pc.ramp(pc.GUARD_TAG, 1, 2, 10).view(-1, 4)
    both = torch.cat([a, b, g])
    assert torch.unique(both, dim=0).shape[0] == both.shape[0]
    pool = pc.as_pool(pc.ramp(pc.SRC_TAG, 6, 5, 7), pc.FP8)
    assert pool.shape == (3, 2, 5, 1, 1, 7 * 16)
    assert pc.as_pool(pc.ramp(pc.SRC_TAG, 6, 5, 7), pc.BF16).shape[-1] == 56


@pytest.mark.parametrize("case", pc.COPY_CASES, ids=lambda c: c.id)
def test_copy_case_accepts_the_kernels_arithmetic(case):
    assert pc.run_copy_case(case, pc.emulated_copy, "cpu") == []


@pytest.mark.parametrize("case", pc.COPY_CASES, ids=lambda c: c.id)
def test_copy_case_rejects_source_chunk_stride(case):
    """The destination chunk stride taken from the source pool: wrong for
    every case whose pools differ in size, invisible where they are equal
    (the two tests the suite had)."""
    def swapped(alloc, guard_vec, src, src_pages, dst_pages, pd):
        pc.emulated_copy(alloc, guard_vec, src, src_pages, dst_pages, pd,
                         dst_stride_pages=case.ps)
    try:
        diffs = pc.run_copy_case(case, swapped, "cpu")
    except IndexError:
        diffs = ["store past the allocation"]
    assert bool(diffs) == (case.ps != case.pd), diffs


def test_copy_case_sees_a_guard_store_and_a_changed_source():
    case = pc.COPY_CASES[3]

    def low(alloc, guard_vec, src, *rest):
        pc.emulated_copy(alloc, guard_vec, src, *rest)
        alloc[guard_vec - 1, 2] ^= 1

    def high(alloc, guard_vec, src, *rest):
        pc.emulated_copy(alloc, guard_vec, src, *rest)
        alloc[-guard_vec, 0] ^= 1

    def touch(alloc, guard_vec, src, *rest):
        pc.emulated_copy(alloc, guard_vec, src, *rest)
        pc.raw(src)[0, 1, 2, 0, 0, 5] ^= 1
    assert "guard before" in pc.run_copy_case(case, low, "cpu")[0]
    assert "guard after" in pc.run_copy_case(case, high, "cpu")[0]
    assert pc.run_copy_case(case, touch, "cpu") == ["source changed"]


# ---------------------------------------------------------------------------
# host-side rejects
# ---------------------------------------------------------------------------

SHAPE = [2, 2, 24, 2, 16, 128]


def _meta(**kw):
    meta = {"local_ptr": 4096, "num_pages": 40,
            "shape": [2, 2, 40, 2, 16, 128], "kv_cache_dtype": "bf16",
            "kv_k_scale_log2": 0, "kv_v_scale_log2": 0}
    meta.update(kw)
    return meta


REJECTS = pc.reject_cases(SHAPE, _meta())


def _stub_pusher(monkeypatch):
    """A pusher whose every step past the checks raises AssertionError."""
    import rbg_amd.ops as ops_mod

    class StubHip:
        def kv_peer_copy(self, *a):
            raise AssertionError("kv_peer_copy was launched")

        def kv_ipc_open(self, raw):
            raise AssertionError("a pool was mapped")

    monkeypatch.setattr(ops_mod, "_hip", StubHip())
    monkeypatch.setattr(ops_mod, "HAVE_HIP", True)
    pusher = kv_peer.PeerKVPusher.__new__(kv_peer.PeerKVPusher)
    pusher._open, pusher._bad, pusher._streams = {}, set(), {}
    pusher._lock = threading.Lock()

    def no_stream(uid):
        raise AssertionError("a stream was opened")
    pusher._stream_for = no_stream
    pusher._map = lambda meta: (_ for _ in ()).throw(
        AssertionError("a pool was mapped"))
    cache = types.SimpleNamespace(
        kv=torch.zeros(SHAPE, dtype=torch.bfloat16),
        signature=lambda: {"kv_cache_dtype": "bf16", "kv_k_scale_log2": 0,
                           "kv_v_scale_log2": 0})
    return pusher, cache


@pytest.mark.parametrize("why", sorted(REJECTS))
def test_push_rejects_before_any_launch(monkeypatch, why):
    pusher, cache = _stub_pusher(monkeypatch)
    src, meta, dst = REJECTS[why]
    with pytest.raises(ValueError):
        pusher.push(cache, src, meta, dst)


def test_push_reaches_the_launch_when_nothing_is_wrong(monkeypatch):
    """The control: the same stub IS reached by a well-formed push, with
    page 0 and the last page of either pool and a repeated source page."""
    pusher, cache = _stub_pusher(monkeypatch)
    kv_peer.check_push_args(SHAPE, [0, 23, 23], _meta(), [39, 0, 7])
    with pytest.raises(AssertionError, match="a pool was mapped"):
        pusher.push(cache, [0, 23, 23], _meta(), [39, 0, 7])
    # a pool of another element type is refused first, as before
    with pytest.raises(ValueError, match="mismatched KV pools"):
        pusher.push(cache, [1], _meta(kv_cache_dtype="fp8_e4m3"), [4])


def test_local_push_on_the_cpu_refuses_the_same():
    cfg = mc.engine_config("conf-llama", "cpu", True, pool_tokens=64)
    src = mc.PagedKVCache(cfg, torch.device("cpu"))
    dst = mc.PagedKVCache(cfg, torch.device("cpu"), num_pages=6)
    dst.kv.fill_(3.0)
    before = dst.kv.clone()
    mig = pd_bench._Migrator("cpu")
    for s, d in (([1, 2], [3]), ([4], [2]), ([1], [6]), ([1, 2], [3, 3])):
        with pytest.raises(ValueError):
            mig.push_local(src, dst, s, d)
    assert torch.equal(dst.kv, before)


# ---------------------------------------------------------------------------
# the RBG_PD_VERIFY digest
# ---------------------------------------------------------------------------

def _digest_pools(dtype):
    gen = torch.Generator().manual_seed(5)
    shape = (2, 2, 12, 2, 16, 128)
    if dtype == pc.FP8:
        kv = torch.randint(0, 256, shape, generator=gen).to(pc.U8).view(pc.FP8)
    else:
        kv = torch.randn(shape, generator=gen).to(pc.BF16)
    src = types.SimpleNamespace(kv=kv)
    dst = types.SimpleNamespace(kv=torch.zeros((2, 2, 9) + shape[3:],
                                               dtype=dtype))
    return src, dst


DIGEST_MUTANTS = {
    "reversed order": lambda moved: moved.flip(2),
    "K and V swapped": lambda moved: moved.flip(1),
    "layer l in l^1": lambda moved: moved.flip(0),
}


@pytest.mark.parametrize("dtype", [pc.BF16, pc.FP8], ids=["bf16", "fp8"])
def test_old_sum_accepts_what_the_digest_rejects(dtype):
    src_pages, dst_pages = [3, 7, 1, 10], [5, 2, 8, 4]
    si, di = torch.tensor(src_pages), torch.tensor(dst_pages)
    src, dst = _digest_pools(dtype)
    moved = pc.raw(src.kv).index_select(2, si)
    pc.raw(dst.kv).index_copy_(2, di, moved)
    want = pd_bench._page_checksum(src, src_pages)
    assert isinstance(want, int) and 0 <= want < 2 ** 64
    assert pd_bench._page_checksum(dst, dst_pages) == want
    if dtype == pc.BF16:
        assert pc.old_page_sum(dst, dst_pages) == pc.old_page_sum(
            src, src_pages)
    for name, wrong in DIGEST_MUTANTS.items():
        pc.raw(dst.kv).index_copy_(2, di, wrong(moved))
        assert not torch.equal(pc.raw(dst.kv).index_select(2, di), moved)
        if dtype == pc.BF16:        # the old sum had no e4m3 kernels at all
            old_src = pc.old_page_sum(src, src_pages)
            old_dst = pc.old_page_sum(dst, dst_pages)
            assert abs(old_src - old_dst) <= 1e-6 * max(1.0, abs(old_src)), \
                "the old sum was expected to accept: " + name
        assert pd_bench._page_checksum(dst, dst_pages) != want, name
    # one 16-byte vector moved to another offset of its page; one bit
    pc.raw(dst.kv).index_copy_(2, di, moved)
    words = 16 // dst.kv.element_size()
    row = pc.raw(dst.kv)[1, 0, 8, 1, 3]
    row[:words], row[words:2 * words] = (row[words:2 * words].clone(),
                                         row[:words].clone())
    assert pd_bench._page_checksum(dst, dst_pages) != want
    pc.raw(dst.kv).index_copy_(2, di, moved)
    pc.raw(dst.kv)[0, 1, 4, 0, 15, 127] ^= 1
    assert pd_bench._page_checksum(dst, dst_pages) != want


# ---------------------------------------------------------------------------
# H1 and H2 on the CPU
# ---------------------------------------------------------------------------

H1_CASES = [(s, c) for c in mc.CONFS for s in pc.SCENARIOS]


@functools.lru_cache(maxsize=None)
def _clean(scenario, conf, fp8=False):
    pair = pc.run_pair(scenario, conf, "cpu", True, fp8=fp8)
    return pair, pc.judge_pair(pair)


@pytest.mark.parametrize("scenario,conf", H1_CASES)
def test_h1_cpu_pair_passes_every_check(scenario, conf):
    pair, verdict = _clean(scenario, conf)
    pc.assert_same_weights(pair)
    pc.assert_paths(pair)
    print("\n%s: worst err / e_cpu logits %.3f, K/V %.3f (%d rows, %d blocks)"
          % ((pair.id,) + verdict.worst() + (len(verdict.c1),
                                             len(verdict.c2))))
    assert not verdict.failures(), verdict.failures()[:8]


@pytest.mark.parametrize("conf", mc.CONFS)
def test_h1_cpu_fp8_pair_passes_every_check(conf):
    pair, verdict = _clean("handoff", conf, True)
    assert pair.pc.kv.dtype == pair.dc.kv.dtype == pc.FP8
    pc.assert_same_weights(pair)
    pc.assert_paths(pair)
    print("\n%s: worst err / e_cpu8 logits %.3f, K/V %.3f" % (
        (pair.id,) + verdict.worst()))
    assert not verdict.failures(), verdict.failures()[:8]


def test_h1_bf16_to_fp8_raises_before_any_byte_moves():
    pair = pc.Pair("handoff", "conf-llama", "cpu", True, fp8=False,
                   d_fp8=True)
    (req,) = pair.prefill(mc._prompts(700, (17,)), [2])
    with pytest.raises(ValueError, match="mismatched KV pools"):
        pair.migrate([req])
    assert torch.equal(pc.raw(pair.dc.kv), pc.raw(pair.d_poison))


@pytest.mark.parametrize("conf", mc.CONFS)
def test_h2_cpu_handshake_passes_every_check(conf):
    s = pc.run_serving(conf, "cpu", True)
    verdict = pc.judge_pair(s)
    pc.assert_same_weights(s)
    pc.assert_serving_paths(s)
    print("\nserving-%s: worst err / e_cpu logits %.3f, K/V %.3f" % (
        (conf,) + verdict.worst()))
    assert not verdict.failures(), verdict.failures()[:8]


def test_judge_sees_one_flipped_element_of_each_pool():
    """C3 on both pools: one bit in the tail of an imported page of D (it
    holds P's poison there), in a page D never owned, and in P."""
    pair, verdict = _clean("handoff", "conf-llama")
    assert verdict.c3 == []
    r16 = pair.reqs[2]
    spots = {"D": [(r16.dst_pages[1], 9), (max(pair.recD.owned) + 1, 3)],
             "P": [(r16.src_pages[1], 9)]}
    for side, where in spots.items():
        for pg, slot in where:
            kv = (pair.d_after if side == "D" else pair.p_after)
            x = kv[1, 0, pg, 0, slot, 5:6].view(torch.int16)
            x ^= 1
            try:
                got = pc.judge_pair(pair).c3
            finally:
                x ^= 1
            assert len(got) == 1 and got[0].startswith(side) and \
                got[0].endswith("page %d slot %d" % (pg, slot)), got
    # D's first write opened that page and its six steps filled slots
    # 0 .. 5; the rest of it is P's poison, not D's
    new = pc.HANDOFF_NEW
    tail = pc.raw(pair.d_after)[:, :, r16.dst_pages[1], :, new:]
    assert torch.equal(
        tail, pc.raw(pair.p_poison)[:, :, r16.src_pages[1], :, new:])
    assert not torch.equal(
        tail, pc.raw(pair.d_poison)[:, :, r16.dst_pages[1], :, new:])


# ---------------------------------------------------------------------------
# mutants
# ---------------------------------------------------------------------------

MUTANT_CONF = "conf-llama"
MUTANT_CASES = [(m, s) for m in pc.MUTANTS for s in pc.SCENARIOS]
# prompt_pages_only leaves a page unpushed that holds nothing but poison: no
# logit and no cached row can differ, so only the byte-level checks may fire
BYTES_ONLY = {"prompt_pages_only"}


@pytest.mark.parametrize("mutant,scenario", MUTANT_CASES)
def test_mutant_is_caught_where_it_applies(mutant, scenario):
    clean, _ = _clean(scenario, MUTANT_CONF)
    pair = pc.run_pair(scenario, MUTANT_CONF, "cpu", True, mutant=mutant)
    failed = pc.judge_pair(pair).failed_checks()
    changed = pc.differs(pair, clean)
    applies = scenario in pc.MUTANTS[mutant].applies
    print("\n| %s | %s | %s | %s |" % (
        mutant, scenario,
        "applies" if applies else ("no-op" if not changed else "also bites"),
        " ".join(sorted(failed)) or "-"))
    if applies:
        assert changed, "%s is a no-op in %s" % (mutant, scenario)
        assert failed, "%s was missed in %s" % (mutant, scenario)
    else:
        # outside its scenarios it either changes nothing or is caught
        assert failed or not changed
    if mutant in BYTES_ONLY and applies:
        assert failed == {"C0", "C3"}, failed
    if mutant == "first_tokens_rotated" and applies:
        assert failed == {"C4"}, failed


def test_every_listed_mutant_applies_somewhere():
    for name, mut in pc.MUTANTS.items():
        assert mut.applies and set(mut.applies) <= set(pc.SCENARIOS), name
    assert len(pc.MUTANTS) == 11
