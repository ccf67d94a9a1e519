"""CPU self-test of tests/kvfp8_cases.py and CPU-level checks of the FP8
(e4m3) KV cache: the torch quantiser reference against an independent
table-driven one, the quantised decode cases (reference, emulation and the
project's CPU path accepted; every mutant rejected), pool capacity, the
config and op rejects, and P/D transfer between fp8 pools over gloo.

Run with -s to see which family caught which mutant.
"""
import socket

import pytest
import torch

import attn_cases as ac
import kvfp8_cases as k8
import rbg_amd.ops as ops
from rbg_amd.engine.config import EngineConfig, ModelConfig
from rbg_amd.engine.kv_cache import PagedKVCache
from rbg_amd.ops import reference

BF16, FP8, U8 = torch.bfloat16, torch.float8_e4m3fn, torch.uint8


# ---------------------------------------------------------------------------
# the quantiser reference itself
# ---------------------------------------------------------------------------

def _table_quantise(x: torch.Tensor, e: int) -> torch.Tensor:
    """sat_rne_e4m3fn(x * 2^-e) without torch's conversion: nearest of the
    127 non-negative finite e4m3 values, built from the format's definition,
    ties to the even code."""
    codes = torch.arange(127)
    exp, man = codes >> 3, (codes & 7).double()
    vals = torch.where(exp == 0, man / 8 * 2.0 ** -6,
                       (1 + man / 8) * 2.0 ** (exp.double() - 7))
    assert float(vals[126]) == 448.0 and float(vals[1]) == 2.0 ** -9
    y = x.double() * 2.0 ** -e
    mag = y.abs().clamp(max=448.0)
    hi = torch.searchsorted(vals, mag).clamp(max=126)
    lo = (hi - 1).clamp(min=0)
    dlo, dhi = (mag - vals[lo]).abs(), (vals[hi] - mag).abs()
    pick = torch.where(dlo < dhi, lo, torch.where(dhi < dlo, hi,
                       torch.where(lo % 2 == 0, lo, hi)))
    out = pick.to(U8) | (torch.signbit(y).to(U8) << 7)
    return torch.where(torch.isnan(y), torch.full_like(out, 0x7F), out)


@pytest.mark.parametrize("e", k8.QUANT_EXPONENTS + (-16, 16))
def test_reference_quantiser_is_sat_rne_e4m3fn(e):
    x = k8.all_bf16_patterns().reshape(-1)
    got = reference.quantize_e4m3(x, e).view(U8)
    ok, msg = k8.bytes_match(got, _table_quantise(x, e))
    assert ok, msg
    # saturation, not NaN, for overflow and infinities
    big = torch.tensor([1e30, float("inf"), -float("inf"), 449.0, 464.0, 480.0])
    assert reference.quantize_e4m3(big.to(BF16), 0).view(U8).tolist() == [
        0x7E, 0x7E, 0xFE, 0x7E, 0x7E, 0x7E]


def test_dequantise_is_exact_in_bf16():
    b = torch.arange(256, dtype=torch.int32).to(U8)
    b = b[~k8.is_nan_byte(b)].view(FP8)
    for e in (-16, -2, 0, 3, 16):
        got = k8.dq(b, e)
        assert torch.equal(got.double(), b.double() * 2.0 ** e)
        # and a value that was cached reads back as the same byte
        assert torch.equal(k8.q8(got, e).view(U8), b.view(U8))


def test_cpu_store_matches_the_definition():
    """ops.rope_store_kv on the CPU: bytes are q8 of the rotated, rounded K
    and of V; -1 slots and unwritten slots keep their poison."""
    d = k8.quant_inputs(2, 1, 37, 0)
    kq0, vq0 = k8.poison_pool(d["pages"], 1)
    q, k = d["q"].clone(), d["k"].clone()
    kq, vq = kq0.clone(), vq0.clone()
    ops.rope_store_kv(q, k, d["v"], kq, vq, d["table"], d["pos"], d["slots"],
                      k_scale_log2=-3, v_scale_log2=2)
    want_k, want_v = kq0.view(U8).clone(), vq0.view(U8).clone()
    for t, s in enumerate(d["slots"].tolist()):
        if s >= 0:
            want_k[s // 16, :, s % 16] = k8.q8(k[t], -3).view(U8)
            want_v[s // 16, :, s % 16] = k8.q8(d["v"][t], 2).view(U8)
    assert k8.bytes_match(kq.view(U8), want_k) == (True, "")
    assert k8.bytes_match(vq.view(U8), want_v) == (True, "")
    assert int((vq.view(U8) == k8.V_POISON_BYTE).all(-1).sum()) >= 16 * 3


@pytest.mark.parametrize("kvh", k8.GATHER_KVH)
@pytest.mark.parametrize("tkv", k8.GATHER_TKV)
def test_cpu_gather(tkv, kvh):
    cache, slots = k8.gather_inputs(tkv, kvh)
    for e in (0, -2, 3):
        got = ops.kv_gather_dequant(cache, slots, e)
        assert got.dtype == BF16
        assert torch.equal(got, k8.gather_expected(cache, slots, e))


# ---------------------------------------------------------------------------
# decode cases
# ---------------------------------------------------------------------------

def _base_out(data):
    return ac.decode_ref64(data["q"], data["kd"], data["vd"], data["bt"],
                           data["ctx"], data["scale"]).to(BF16)


@pytest.mark.parametrize("exps", k8.DECODE_EXPONENTS, ids=lambda e: "e%d_%d" % e)
@pytest.mark.parametrize("case", ac.DECODE_CASES, ids=lambda c: c.id)
def test_decode_reference_emulation_and_cpu_path_pass(case, exps):
    for family in ac.DECODE_FAMILIES:
        data = k8.decode_data(case, family, *exps)
        for name, out in (("fp64 reference", _base_out(data)),
                          ("bf16 emulation", k8.decode_emulated(data)),
                          ("ops.reference", k8.decode_cpu(data))):
            ok, msg, _ = ac.check(out, data)
            assert ok, (name, family, msg)


def test_decode_mutants_are_rejected():
    """attn_cases' decode mutants (leak key, drop last, drop page, wrong
    page, swapped heads, wrong KV head, drop split) through the quantised
    reference, plus 'dequantise with e + 1' and 'read K bytes as V': none is
    missed where it applies."""
    ek, ev = k8.DECODE_EXPONENTS[1]
    print("\n%-16s %7s %5s %6s  caught by" % ("mutant", "applies", "noop",
                                               "missed"))
    for mut in k8.DECODE_MUTANTS:
        applies, noop, missed, by = 0, [], [], {}
        for case in ac.DECODE_CASES:
            if not k8.decode_mutant_applies(mut, case):
                continue
            applies += 1
            changed, caught = False, []
            for family in ac.DECODE_FAMILIES:
                data = k8.decode_data(case, family, ek, ev)
                out = k8.decode_mutant(data, mut)
                if torch.equal(out, _base_out(data)):
                    continue
                changed = True
                if not ac.check(out, data)[0]:
                    caught.append(family)
            if not changed:
                noop.append(case.id)
            elif not caught:
                missed.append(case.id)
            for f in caught:
                by[f] = by.get(f, 0) + 1
        print("%-16s %7d %5d %6d  %s" % (mut, applies, len(noop),
                                         len(missed), by))
        assert applies > 0, mut
        assert not missed, (mut, "changed the output uncaught at", missed)
        assert len(noop) <= 0.10 * applies, (mut, "no-op at", noop)


# ---------------------------------------------------------------------------
# capacity
# ---------------------------------------------------------------------------

def _cfg(**kw):
    return EngineConfig(model=ModelConfig.preset("tiny"), device="cpu",
                        enforce_eager=True, **kw)


def test_fp8_pool_has_twice_the_pages():
    cpu = torch.device("cpu")
    bf = PagedKVCache._size_pool(_cfg(), cpu)
    f8 = PagedKVCache._size_pool(_cfg(kv_cache_dtype="fp8_e4m3"), cpu)
    assert f8 == 2 * bf
    m = ModelConfig.preset("llama-3-8b")
    assert m.kv_bytes_per_token() == 131072                   # unchanged
    assert m.kv_bytes_per_token("fp8_e4m3") * 2 == m.kv_bytes_per_token("bf16")
    cache = PagedKVCache(_cfg(kv_cache_dtype="fp8_e4m3", kv_pool_tokens=256,
                              kv_k_scale_log2=-2, kv_v_scale_log2=3), cpu)
    assert cache.kv.dtype == FP8 and cache.kv.element_size() == 1
    assert cache.key_cache(0).dtype == FP8
    assert (cache.k_scale_log2, cache.v_scale_log2) == (-2, 3)
    assert PagedKVCache(_cfg(kv_pool_tokens=256), cpu).kv.dtype == BF16


def test_default_config_is_bf16():
    cfg = EngineConfig()
    assert (cfg.kv_cache_dtype, cfg.kv_k_scale_log2, cfg.kv_v_scale_log2) == (
        "bf16", 0, 0)


# ---------------------------------------------------------------------------
# rejects
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [
    dict(kv_cache_dtype="fp8"), dict(kv_cache_dtype="fp8_e5m2"),
    dict(kv_cache_dtype="fp8_e4m3", kv_k_scale_log2=17),
    dict(kv_cache_dtype="fp8_e4m3", kv_v_scale_log2=-17),
    dict(kv_k_scale_log2=1.0), dict(kv_cache_dtype="fp8_e4m3", page_size=32)],
    ids=lambda kw: "-".join("%s=%s" % i for i in kw.items()))
def test_config_rejects(kw):
    with pytest.raises(ValueError):
        _cfg(**kw)


def _decode_args(page=16, d=128):
    kc = torch.zeros(4, 1, page, d, dtype=BF16).to(FP8)
    return dict(q=torch.zeros(2, 2, d, dtype=BF16), key_cache=kc,
                value_cache=kc.clone(),
                block_tables=torch.ones(2, 2, dtype=torch.int32),
                context_lens=torch.ones(2, dtype=torch.int32), scale=0.1)


def test_ops_reject_before_running(monkeypatch):
    """Each bad fp8 call raises ValueError or RuntimeError, and neither the
    CPU reference nor a kernel is reached."""
    def boom(*a, **k):
        raise AssertionError("reached the implementation")
    monkeypatch.setattr(reference, "decode_attention", boom)
    monkeypatch.setattr(reference, "rope_store_kv", boom)
    monkeypatch.setattr(reference, "kv_gather_dequant", boom)
    bad = [dict(_decode_args(page=32)), dict(_decode_args(d=64)),
           dict(_decode_args(), variant=1), dict(_decode_args(), variant=5),
           dict(_decode_args(), k_scale_log2=17),
           dict(_decode_args(), v_scale_log2=-17),
           dict(_decode_args(), value_cache=torch.zeros(4, 1, 16, 128,
                                                        dtype=BF16))]
    for kw in bad:
        with pytest.raises((ValueError, RuntimeError)):
            ops.decode_attention(**kw)
    a = _decode_args()
    with pytest.raises((ValueError, RuntimeError)):
        ops.kv_gather_dequant(a["key_cache"], torch.zeros(1, dtype=torch.int32),
                              20)
    with pytest.raises((ValueError, RuntimeError)):
        ops.kv_gather_dequant(a["key_cache"].to(BF16),
                              torch.zeros(1, dtype=torch.int32), 0)
    d = k8.quant_inputs(2, 1, 1, 0)
    kq, vq = k8.poison_pool(d["pages"], 1)
    for kw in (dict(k_scale_log2=-17), dict(v_scale_log2=17)):
        with pytest.raises((ValueError, RuntimeError)):
            ops.rope_store_kv(d["q"], d["k"], d["v"], kq, vq, d["table"],
                              d["pos"], d["slots"], **kw)
    with pytest.raises((ValueError, RuntimeError)):
        ops.rope_store_kv(d["q"], d["k"], d["v"], kq, vq.to(BF16), d["table"],
                          d["pos"], d["slots"])
    # and the good call does reach it
    with pytest.raises(AssertionError, match="reached"):
        ops.decode_attention(**_decode_args())


# ---------------------------------------------------------------------------
# engine and transfer
# ---------------------------------------------------------------------------

def _engine(**kw):
    from rbg_amd.engine.engine import LLMEngine
    return LLMEngine(_cfg(kv_pool_tokens=1024, max_batch_size=8, **kw))


def test_logits_do_not_depend_on_prefix_hit_or_chunking():
    """In fp8 mode every attention read sees dq(q8(.)), keys of the same
    prefill step included, so a whole prefill, a chunked one and a prefix
    hit generate the same tokens from bit-identical cache bytes."""
    from rbg_amd.engine.sequence import SamplingParams
    gen = torch.Generator().manual_seed(5)
    prompt = torch.randint(0, 512, (70,), generator=gen).tolist()
    fp8 = dict(kv_cache_dtype="fp8_e4m3", kv_k_scale_log2=-1,
               kv_v_scale_log2=-3)
    outs, pools = [], []
    for kw in (dict(), dict(max_prefill_tokens=24)):
        eng = _engine(**fp8, **kw)
        (seq,) = eng.generate([prompt], SamplingParams(max_new_tokens=5))
        outs.append(list(seq.output_tokens))
        if not kw:        # same engine again: the prompt's pages are cached
            (again,) = eng.generate([prompt], SamplingParams(max_new_tokens=5))
            assert again.cached_prefix_len == 64
            outs.append(list(again.output_tokens))
    assert outs[0] == outs[1] == outs[2], outs


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _pd_gloo_worker(rank, world, port):
    """Rank 0 prefills a prompt in fp8 and sends its pages; rank 1 imports
    them into its own fp8 pool: the bytes equal the ones rank 1 gets by
    prefilling the same prompt itself (same seed, same model)."""
    from rbg_amd.engine.sequence import SamplingParams
    from rbg_amd.parallel.kv_transfer import TransferEngine
    fp8 = dict(kv_cache_dtype="fp8_e4m3", kv_k_scale_log2=-2,
               kv_v_scale_log2=1, enable_prefix_cache=False)
    eng = _engine(**fp8)
    cache = eng.runner.cache
    gen = torch.Generator().manual_seed(9)
    prompt = torch.randint(0, 512, (40,), generator=gen).tolist()
    te = TransferEngine(rank=rank, world_size=world, master_addr="127.0.0.1",
                        master_port=port, backend="gloo")
    seq = eng.add_request(prompt, SamplingParams(max_new_tokens=2))
    assert eng.step() == "prefill"
    pages = list(seq.block_table.pages)[:3]          # 40 tokens: 3 pages
    mine = cache.kv.view(U8)[:, :, pages].clone()
    assert bool((mine[:, :, :2] != 0).any())
    if rank == 0:
        te.send_pages(cache, pages, dst_rank=1,
                      peer_signature=cache.signature())
    else:
        dst = cache.alloc(3)
        te.recv_pages(cache, dst, src_rank=0,
                      peer_signature=cache.signature())
        got = cache.kv.view(U8)[:, :, dst]
        assert got.dtype == U8 and torch.equal(got, mine), "pages differ"
    import torch.distributed as dist
    dist.barrier()
    dist.destroy_process_group()


def test_pd_over_gloo_between_fp8_engines():
    import multiprocessing as mp
    ctx = mp.get_context("spawn")
    port = _free_port()
    procs = [ctx.Process(target=_pd_gloo_worker, args=(r, 2, port))
             for r in range(2)]
    for p in procs:
        p.start()
    for p in procs:
        p.join(timeout=240)
    assert [p.exitcode for p in procs] == [0, 0]


def test_signature_mismatch_raises_before_any_byte_moves():
    from rbg_amd.parallel.comm import check_kv_signature
    from rbg_amd.parallel.kv_transfer import TransferEngine
    cpu = torch.device("cpu")
    f8 = PagedKVCache(_cfg(kv_cache_dtype="fp8_e4m3", kv_pool_tokens=64), cpu)
    f8b = PagedKVCache(_cfg(kv_cache_dtype="fp8_e4m3", kv_pool_tokens=64,
                            kv_v_scale_log2=1), cpu)
    bf = PagedKVCache(_cfg(kv_pool_tokens=64), cpu)
    check_kv_signature(f8.signature(), f8.signature())
    check_kv_signature(bf.signature(), None)       # a peer from before fp8
    for a, b in ((f8, bf), (bf, f8), (f8, f8b)):
        with pytest.raises(ValueError, match="mismatched KV pools"):
            check_kv_signature(a.signature(), b.signature())
    # the transfer engine checks before it even connects
    te = TransferEngine(0, 2, "127.0.0.1", 1, backend="gloo")
    te.connect = lambda: (_ for _ in ()).throw(AssertionError("connected"))
    with pytest.raises(ValueError):
        te.send_pages(f8, [1], 1, peer_signature=bf.signature())
    with pytest.raises(ValueError):
        te.recv_pages(bf, [1], 0, peer_signature=f8.signature())
    with pytest.raises(ValueError):
        te.recv_pages(f8, [1], 0, peer_signature=f8b.signature())


def test_wire_format_carries_fp8_as_uint8():
    from rbg_amd.parallel.comm import from_wire, to_wire, wire_dtype
    cpu = torch.device("cpu")
    t = torch.randint(0, 256, (3, 5), dtype=torch.int32).to(U8).view(FP8)
    w = to_wire(t)
    assert w.dtype == U8 and wire_dtype(FP8, cpu) == U8
    assert wire_dtype(FP8, torch.device("cuda")) == U8
    assert torch.equal(from_wire(w, FP8).view(U8), t.view(U8))
    assert wire_dtype(BF16, cpu) == torch.int16                # unchanged


# ---------------------------------------------------------------------------
# model level: the checks of tests/kvfp8_model_cases.py on the CPU
# ---------------------------------------------------------------------------

import kvfp8_model_cases as m8          # noqa: E402
import model_cases as mc                # noqa: E402


@pytest.mark.parametrize("conf", mc.CONFS)
@pytest.mark.parametrize("scenario", m8.SCENARIOS)
def test_model_level_checks_on_the_cpu(scenario, conf):
    """The CPU engine in fp8 mode passes C1-C3 against the quantised dense
    fp64 reference, and a second independent emulation (the fp32-upcast CPU
    path) stays under the same factor 2 of e_cpu8: the bound the GPU test
    uses is one that two correct implementations meet."""
    run = m8.run_scenario8(scenario, conf, "cpu", True)
    run.trace.assert_fp8_paths(False)
    c1, c2, c3 = m8.judge8(run)
    print("\n%s fp8 cpu engine: worst err / e_cpu8 logits %.3f, K/V %.3f" % (
        (run.id,) + m8.worst(c1, c2)))
    assert not m8.failures(c1, c2, c3), m8.failures(c1, c2, c3)[:8]
    u1, u2, _ = m8.judge8(run, upcast_run=True)
    print("%s fp32-upcast emulation: worst err / e_cpu8 logits %.3f, K/V %.3f"
          % ((run.id,) + m8.worst(u1, u2)))
    assert not m8.failures(u1, u2, []), m8.failures(u1, u2, [])[:8]


def test_quantised_reference_differs_from_the_plain_one():
    """The fp8 reference is not the bf16 one: judged against model_cases'
    unquantised dense forward, fp8 cache rows are ~2^-4 off."""
    engine = mc.LLMEngine(mc.engine_config("conf-llama", "cpu", True))
    mc.draw_norm_weights(engine.runner.model)
    model = mc.cpu_model("conf-llama", mc.snapshot_params(engine.runner.model),
                         engine.runner.model.cos_sin)
    tokens = mc._prompts(1, (45,))[0]
    _, plain = mc.dense_forward64(model, tokens)
    _, quant = m8.dense_forward64_q8(model, tokens)
    err = mc.rel_l2(quant[:, 0, 1], plain[:, 0, 1])
    assert 2.0 ** -7 < err < 2.0 ** -3, err


def test_serve_worker_import_refuses_a_mismatched_pool():
    """`import_seq` from a prefill engine whose pool differs in dtype or in
    an exponent raises before a page is allocated; a matching one goes on."""
    import types

    from rbg_amd.engine import serve_worker as sw
    eng = _engine(kv_cache_dtype="fp8_e4m3", kv_k_scale_log2=-2)
    sig = eng.runner.cache.signature()
    assert sig == {"kv_cache_dtype": "fp8_e4m3", "kv_k_scale_log2": -2,
                   "kv_v_scale_log2": 0}
    reached = []

    def alloc(*a, **k):
        reached.append("alloc")
        raise KeyError("stop here")
    w = types.SimpleNamespace(engine=eng, tp=None, gcomm=None,
                              _peer_possible=lambda: False,
                              _import_alloc=alloc)
    call = dict(tokens=[1, 2, 3], first_token=4, num_pages=1,
                max_new_tokens=2, src_rank=0)
    for kv in (None, {"kv_cache_dtype": "bf16"}, dict(sig, kv_k_scale_log2=0),
               dict(sig, kv_v_scale_log2=1)):
        with pytest.raises(ValueError, match="mismatched KV pools"):
            sw.ServeWorker._rpc_import_seq(w, kv=kv, **call)
    assert reached == []
    with pytest.raises(KeyError):
        sw.ServeWorker._rpc_import_seq(w, kv=dict(sig), **call)
    assert reached == ["alloc"]


def test_role_args_reach_the_engine_config():
    import types

    from rbg_amd.engine import serve_worker as sw
    ctx = types.SimpleNamespace(gpu_ids=[], args={
        "model": "tiny", "kv_cache_dtype": "fp8_e4m3", "kv_k_scale_log2": -2,
        "kv_v_scale_log2": "3"})
    cfg = sw._engine_cfg(ctx)
    assert cfg.kv_signature() == {"kv_cache_dtype": "fp8_e4m3",
                                  "kv_k_scale_log2": -2, "kv_v_scale_log2": 3}
    ctx.args = {"model": "tiny"}
    assert sw._engine_cfg(ctx).kv_cache_dtype == "bf16"
    ctx.args = {"model": "tiny", "kv_cache_dtype": "fp4"}
    with pytest.raises(ValueError):
        sw._engine_cfg(ctx)
