"""CPU self-test of the seeded-sampling reference, cases and checks
(tests/sampling_cases.py), of `ops.reference.sample`, of the engine's sampling
path on device="cpu", and of the wire plumbing.  No GPU, no HIP extension.
"""
import json
import threading
import types
import urllib.error
import urllib.request
from http.server import ThreadingHTTPServer

import numpy as np
import pytest
import torch

import sampling_cases as sc
from rbg_amd import ops
from rbg_amd.engine.sequence import SamplingParams
from rbg_amd.ops import reference

CASES = sc.op_cases()


# ---------------------------------------------------------------------------
# specification fixed points
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("impl", ["oracle", "ops.reference"])
def test_philox_known_answers(impl):
    for counter, key, want in sc.PHILOX_KNOWN_ANSWERS:
        if impl == "oracle":
            got = sc.philox4x32_10(*counter, *key)
        else:
            got = reference.philox4x32_10(counter, key)
        assert tuple(int(x) for x in got) == want


def test_noise_layout():
    """Token i takes word i & 3 of the block with counter (i >> 2, pos, 0, 0)
    and key (seed low, seed high); u = ((x >> 8) + 0.5) * 2^-24."""
    seed, pos = 0x0123456789abcdef, 77
    idx = np.arange(11)
    g = sc.gumbel_noise(idx, [seed], [pos])[0]
    for i in idx:
        words = sc.philox4x32_10(i >> 2, pos, 0, 0, seed & 0xffffffff,
                                 seed >> 32)
        x = int(words[i & 3])
        u = ((x >> 8) + 0.5) * 2.0 ** -24
        assert g[i] == -np.log(-np.log(u))
    assert 0 < ((0xffffffff >> 8) + 0.5) * 2.0 ** -24 < 1


def test_fp32_gumbel_matches_fp64():
    """The fp32 noise path (log1p for the upper half of u) stays within the
    draw tolerance's per-score share, also at both ends of the range."""
    x = np.array([0, 255, 256, 1 << 31, (1 << 31) - 256, 0xffffffff,
                  0xffffff00, 0x7fffffff, 12345678], dtype=np.uint64)
    m = (x >> np.uint64(8)).astype(np.float64)
    want = -np.log(-np.log((m + 0.5) * 2.0 ** -24))
    got = reference._gumbel_f32(x).astype(np.float64)
    assert np.all(np.isfinite(got))
    assert np.all(np.abs(got - want) <= 2.0 ** -22 * (1 + np.abs(want)))


def test_case_matrix_covers_the_issue():
    by_name = {c.name: c for c in CASES}
    assert set(by_name) == {"V1", "V7", "V64", "V1000", "V4099", "V128256"}
    assert by_name["V128256"].rows == 4
    for V in (1, 7, 64, 1000, 4099):
        groups = by_name["V%d" % V].groups
        prms = [g.prm for g in groups]
        assert {p.T for p in prms} >= {0.0, 0.5, 1.0, 2.0}
        assert {p.top_k for p in prms} >= {0, 1, 2, 50, V - 1, V, V + 5}
        assert {p.top_p for p in prms} >= {1.0, 0.95, 0.5, 1e-6}
        assert {p.min_p for p in prms} >= {0.0, 0.05, 0.5, 1.0}
        seeds = {s for g in groups for s in g.seeds}
        assert {0, sc.SEED_MAX, 0x189abcdef, 0x8000000189abcdef} <= seeds
        assert any(0 in g.poss for g in groups)
        assert max(len(g.seeds) for g in groups) == 64


def test_tied_fixture_keeps_more_than_k():
    g = sc.tied_fixture()
    assert g.ref.num_kept == 4
    assert sorted(np.flatnonzero(g.ref.kept)) == [1, 2, 3, 5]
    toks, kept = sc.run_sampler(ops.sample, [g])
    assert not sc.judge("tied", [g], toks, kept).failures
    assert set(toks) == {1, 2, 3, 5}


# ---------------------------------------------------------------------------
# the checks accept the CPU implementation ...
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("case", CASES, ids=lambda c: c.name)
def test_cpu_sampler_passes(case):
    toks, kept = sc.run_sampler(ops.sample, case.groups)
    v = sc.judge(case.name, case.groups, toks, kept)
    print("%s: %d draws, %d near ties, %d by the runner-up clause"
          % (case.name, v.draws, v.near_ties, v.runner_up_used))
    assert not v.failures, "\n".join(v.failures[:10])


def test_extreme_uniforms_cpu():
    groups = sc.extreme_uniform_groups()
    toks, kept = sc.run_sampler(ops.sample, groups)
    assert not sc.judge("extreme", groups, toks, kept).failures


def test_small_kept_sets_cpu():
    for g in sc.small_kept_groups():
        toks, kept = sc.run_sampler(ops.sample, [g])
        assert not sc.judge("small", [g], toks, kept).failures
        assert set(toks) == set(np.flatnonzero(g.ref.kept)), g.prm
        assert set(g.ref.token) == set(np.flatnonzero(g.ref.kept)), g.prm


def test_invariance_cpu():
    g = CASES[3].groups[-2]                   # V = 1000, top-k + top-p
    row = sc.Group(g.logits, g.prm, g.seeds[:1], g.poss[:1], None)
    other = CASES[3].groups[0]
    filler = sc.Group(other.logits, other.prm, other.seeds[:1],
                      other.poss[:1], None)
    a = ops.sample(*sc.case_tensors([row]))[0]
    b = ops.sample(*sc.case_tensors([filler, filler, row]))[0]
    assert a[0] == b[2] == g.ref.token[0]


@pytest.mark.parametrize("top_p", [1.0, 0.9])
def test_reference_frequencies(top_p):
    """The reference's own counts over 65 536 seeds: within 4 sigma of N p in
    every cell.  Fixed numbers: a failure means the specification or the
    reference is wrong."""
    g = sc.freq_group(top_p)
    counts = np.bincount(g.ref.token, minlength=8)
    want = sc.freq_expected(g)
    sigma = np.sqrt(want * (1 - want / sc.FREQ_N))
    print("counts", counts.tolist(), "expected", np.round(want, 1).tolist())
    assert g.ref.num_kept == (8 if top_p == 1.0 else 5)
    assert np.all(counts[~g.ref.kept] == 0)
    assert np.all(np.abs(counts - want) <= 4 * sigma)
    assert int(g.ref.near_tie.sum()) <= sc.NEAR_TIE_BUDGET * sc.FREQ_N


# ---------------------------------------------------------------------------
# ... and reject wrong ones
# ---------------------------------------------------------------------------

def test_mutants_are_caught():
    """Each mutant is a wrong reference.  Per family: in how many cases its
    output differs from the reference's (applies), in how many it does not
    (no-op), and in how many it differs and the checks pass all the same
    (missed; none allowed)."""
    cases = [(c.name, c.groups) for c in CASES[:5]]
    cases.append(("tied", [sc.tied_fixture()]))
    cases.append(("small", sc.small_kept_groups()))
    cases.append(("extreme", sc.extreme_uniform_groups()))
    report = {}
    for mutant in sc.MUTANTS:
        applies = noop = missed = 0
        for name, groups in cases:
            toks, kept = sc.mutant_outputs(groups, mutant)
            same = all(
                np.array_equal(toks[a:b], g.ref.token) and
                np.all(kept[a:b] == g.ref.num_kept)
                for g, a, b in _spans(groups))
            if same:
                noop += 1
                continue
            applies += 1
            if not sc.judge(name, groups, toks, kept).failures:
                missed += 1
        report[mutant] = (applies, noop, missed)
    for mutant, row in report.items():
        print("%-28s applies %d  no-op %d  missed %d" % ((mutant,) + row))
    for mutant, (applies, _, missed) in report.items():
        assert applies > 0, "%s never applies" % mutant
        assert missed == 0, "%s missed" % mutant


def _spans(groups):
    at = 0
    for g in groups:
        yield g, at, at + len(g.seeds)
        at += len(g.seeds)


def test_greedy_row_in_mixed_batch_is_exact():
    """A greedy row among sampled rows is the exact lowest-index argmax
    (it used to be a draw at T = 1e-5), whatever the seed."""
    logits = torch.tensor([[0.0, 1.0, 1.0 - 1e-6, -2.0]] * 2)
    toks, kept = ops.sample(
        logits, torch.tensor([0.0, 1.0]),
        torch.zeros(2, dtype=torch.int32), torch.ones(2), torch.zeros(2),
        torch.tensor([5, 5]), torch.tensor([9, 9], dtype=torch.int32))
    assert toks[0] == 1 and kept.tolist() == [1, 4]


# ---------------------------------------------------------------------------
# SamplingParams and the engine
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("kw", [
    dict(temperature=-0.1), dict(temperature=float("nan")),
    dict(top_p=0.0), dict(top_p=1.5), dict(top_k=-1), dict(top_k=1.5),
    dict(min_p=-0.1), dict(min_p=1.1), dict(seed=-1), dict(seed=2 ** 64),
])
def test_validate_rejects(kw):
    with pytest.raises(ValueError):
        SamplingParams(**kw).validate()


def test_validate_accepts_the_domain_edges():
    for kw in (dict(), dict(temperature=0.0), dict(top_p=1.0),
               dict(top_p=1e-6), dict(top_k=0), dict(min_p=0.0),
               dict(min_p=1.0), dict(seed=0), dict(seed=2 ** 64 - 1)):
        SamplingParams(**kw).validate()


def _tiny_engine(seed=0):
    import model_cases as mc
    from rbg_amd.engine.engine import LLMEngine
    cfg = mc.engine_config("conf-llama", "cpu", True)
    cfg.seed = seed
    return LLMEngine(cfg)


def test_add_request_validates_and_assigns_seeds():
    eng = _tiny_engine()
    with pytest.raises(ValueError):
        eng.add_request([1, 2, 3], SamplingParams(top_p=0.0))
    shared = SamplingParams(max_new_tokens=2, temperature=1.0)
    a = eng.add_request([1, 2, 3], shared)
    b = eng.add_request([1, 2, 3], shared)
    c = eng.add_request([1, 2, 3], SamplingParams(max_new_tokens=2, seed=42))
    assert shared.seed is None              # the caller's object is not ours
    for s in (a, b):
        assert isinstance(s.sampling.seed, int)
        assert 0 <= s.sampling.seed < 2 ** 64
    assert a.sampling.seed != b.sampling.seed
    assert c.sampling.seed == 42
    # another engine built alike assigns the same seeds in the same order
    other = _tiny_engine()
    assert other.add_request([9], shared).sampling.seed == a.sampling.seed


@pytest.mark.parametrize("conf", ["conf-llama", "conf-qwen"])
@pytest.mark.parametrize("scenario", sc.ENGINE_SCENARIOS)
def test_engine_cpu_teacher_forced(scenario, conf):
    engine, rec, seqs = sc.run_engine_scenario(scenario, conf, "cpu", True)
    v = sc.assert_engine_run(scenario, engine, rec, seqs)
    print("%s-%s: %d rows, %d near ties, %d by the runner-up clause"
          % (scenario, conf, v.draws, v.near_ties, v.runner_up_used))


def test_engine_cpu_is_reproducible():
    runs = [sc.run_engine_scenario("five", "conf-llama", "cpu", True)[2]
            for _ in range(2)]
    assert [s.output_tokens for s in runs[0]] == \
        [s.output_tokens for s in runs[1]]
    assert [s.sampling.seed for s in runs[0]] == \
        [s.sampling.seed for s in runs[1]]


def test_top_p_is_read_now():
    """`top_p` used to be ignored: with top_p = 1e-6 a hot request must
    produce the argmax at every step."""
    import model_cases as mc
    eng = _tiny_engine()
    rec = sc.SampleRecorder(eng)
    with rec:
        (s,) = eng.generate(mc._prompts(640, (12,)), SamplingParams(
            max_new_tokens=6, temperature=5.0, top_p=1e-6, seed=1))
    assert s.output_tokens == [int(np.argmax(r.logits)) for r in rec.rows]


# ---------------------------------------------------------------------------
# wire plumbing
# ---------------------------------------------------------------------------

FULL = {"temperature": 0.7, "top_p": 0.9, "top_k": 5, "min_p": 0.1,
        "seed": 2 ** 64 - 3}


class _FakeEngine:
    def __init__(self):
        self.got = []

    def add_request(self, tokens, sampling):
        self.got.append(sampling)
        sampling.validate()
        return types.SimpleNamespace(seq_id=len(self.got), sampling=sampling)


def _fake_worker():
    from rbg_amd.engine.config import ModelConfig
    eng = _FakeEngine()
    cfg = types.SimpleNamespace(model=ModelConfig.preset("tiny"))
    return types.SimpleNamespace(cfg=cfg, tp=None, engine=eng, results={})


def _fields(sp):
    return {k: getattr(sp, k) for k in FULL}


def test_worker_ops_carry_every_parameter():
    from rbg_amd.engine.serve_worker import ServeWorker
    w = _fake_worker()
    ServeWorker._rpc_submit(w, [1, 2, 3], 4, **FULL)
    assert _fields(w.engine.got[-1]) == FULL
    assert w.engine.got[-1].max_new_tokens == 4
    # the TP lockstep op built from the same call
    ServeWorker._tp_apply_op(w, {"kind": "submit", "tokens": [1, 2],
                                 "max_new_tokens": 3, **FULL})
    assert _fields(w.engine.got[-1]) == FULL
    # peers that send temperature only behave as before
    ServeWorker._rpc_submit(w, [1, 2, 3], 4, 0.5)
    assert _fields(w.engine.got[-1]) == {
        "temperature": 0.5, "top_p": 1.0, "top_k": 0, "min_p": 0.0,
        "seed": None}
    with pytest.raises(ValueError):
        ServeWorker._rpc_submit(w, [1, 2, 3], 4, top_p=0.0)


def test_import_keeps_parameters_and_seed():
    from rbg_amd.engine.serve_worker import ServeWorker
    cache = types.SimpleNamespace(alloc=lambda n: list(range(n)))
    w = types.SimpleNamespace(
        engine=types.SimpleNamespace(
            runner=types.SimpleNamespace(cache=cache)), results={})
    seq = ServeWorker._import_alloc(w, [1, 2, 3], 2, 8, dict(FULL))
    assert _fields(seq.sampling) == FULL
    assert seq.sampling.max_new_tokens == 8


@pytest.fixture
def http_router():
    """The real HTTP handler over the real Router.generate, with the
    dispatch to worker processes replaced by a recorder."""
    from rbg_amd.server.router_worker import Router, _Handler
    router = Router.__new__(Router)
    router.ctx = types.SimpleNamespace(args={})
    router.mode = "colocated"
    router.vocab_size = 500
    router._gc_stale = lambda: None
    sent = []

    def dispatch(tokens, max_new_tokens, sampling, t0):
        sent.append((router.mode, max_new_tokens, sampling))
        return {"tokens": [0] * max_new_tokens, "finished": True}

    router._generate_colocated = dispatch
    router._generate_pd = dispatch
    handler = type("H", (_Handler,), {"router": router})
    httpd = ThreadingHTTPServer(("127.0.0.1", 0), handler)
    threading.Thread(target=httpd.serve_forever, args=(0.02,),
                     daemon=True).start()
    yield router, sent, httpd.server_address[1]
    httpd.shutdown()
    httpd.server_close()


def _post(port, path, payload):
    req = urllib.request.Request(
        "http://127.0.0.1:%d%s" % (port, path),
        data=json.dumps(payload).encode(),
        headers={"Content-Type": "application/json"})
    try:
        with urllib.request.urlopen(req, timeout=30) as resp:
            return resp.status, json.loads(resp.read())
    except urllib.error.HTTPError as e:
        return e.code, json.loads(e.read())


@pytest.mark.parametrize("mode", ["colocated", "pd"])
def test_http_body_reaches_the_dispatch_unchanged(http_router, mode):
    router, sent, port = http_router
    router.mode = mode
    body = dict(FULL, prompt_tokens=[1, 2, 3], max_new_tokens=4)
    code, res = _post(port, "/generate", body)
    assert code == 200 and len(res["tokens"]) == 4
    assert sent[-1] == (mode, 4, FULL)
    # the OpenAI-shaped path too; absent fields keep their defaults
    code, _ = _post(port, "/v1/completions", {"prompt": "a b", "max_tokens": 2})
    assert code == 200
    assert sent[-1] == (mode, 2, {"temperature": 0.0, "top_p": 1.0,
                                  "top_k": 0, "min_p": 0.0, "seed": None})


@pytest.mark.parametrize("bad", [
    {"temperature": -1}, {"top_p": 0}, {"top_p": 1.01}, {"top_k": -2},
    {"top_k": 2.5}, {"min_p": 2}, {"seed": -1}, {"seed": 2 ** 64},
    {"seed": "x"},
])
def test_invalid_values_give_400(http_router, bad):
    _, sent, port = http_router
    code, res = _post(port, "/generate",
                      dict(bad, prompt_tokens=[1, 2, 3], max_new_tokens=2))
    assert code == 400, res
    assert "error" in res and not sent


def test_pd_prefill_samples_under_the_request_and_forwards_the_seed():
    """`_rpc_prefill` with a CPU engine: the first token is the reference
    draw at pos = prompt length (it used to be the argmax), and what travels
    to the decode side carries the parameters and the RESOLVED seed."""
    import model_cases as mc
    from rbg_amd.engine import serve_worker as sw
    eng = _tiny_engine()
    prompt = mc._prompts(650, (20,))[0]
    calls = []

    class Client:
        def __init__(self, host, port):
            pass

        def call(self, method, **params):
            calls.append((method, params))
            return {"seq_id": 7, "peer": None}

        def close(self):
            pass

    w = types.SimpleNamespace(
        tp=None, engine=eng, results={}, gcomm=object(), my_instance="p-0",
        _finished_pages={}, _peer_possible=lambda: False,
        _decode_port=lambda inst: 1, _peer_rank=lambda inst: 1,
        _send_pages=lambda pages, rank: None,
        _release_parked=lambda parked: None)

    def poll(seq_id):
        # stands in for the engine loop: run the request to completion and
        # park its pages as the prefill role does
        while eng.scheduler.has_work():
            eng.step()
        w._finished_pages.setdefault(seq_id, ([0], 0))
        return {"finished": True}

    w._rpc_poll = poll
    rec = sc.SampleRecorder(eng)
    orig = sw.RpcClient
    sw.RpcClient = Client
    try:
        with rec:
            out = sw.ServeWorker._rpc_prefill(
                w, prompt, 6, "d-0", temperature=1.5, top_k=40, top_p=0.95,
                min_p=0.01, seed=None)
    finally:
        sw.RpcClient = orig
    (row,) = rec.rows
    assert row.pos == len(prompt)
    prm = sc.Params(1.5, 40, 0.95, 0.01)
    assert sc.seq_params(row.seq) == prm
    seed = row.seq.sampling.seed
    assert seed is not None
    ref = sc.ref_row(row.logits, prm, seed, len(prompt), check=False)
    assert not ref.near_tie[0]
    assert out["first_token"] == ref.token[0]
    assert out["first_token"] != int(np.argmax(row.logits)), \
        "pick another prompt: this draw happens to be the argmax"
    (method, meta), = calls
    assert method == "import_seq"
    assert {k: meta[k] for k in FULL} == {
        "temperature": 1.5, "top_p": 0.95, "top_k": 40, "min_p": 0.01,
        "seed": seed}
    assert meta["first_token"] == out["first_token"]
    assert meta["max_new_tokens"] == 6

    # the decode side: the imported sequence continues the same stream
    cache = types.SimpleNamespace(alloc=lambda n: list(range(n)))
    d = types.SimpleNamespace(
        engine=types.SimpleNamespace(
            runner=types.SimpleNamespace(cache=cache)), results={})
    seq = sw.ServeWorker._import_alloc(
        d, meta["tokens"], meta["num_pages"], meta["max_new_tokens"],
        {k: meta[k] for k in FULL})
    assert seq.sampling.seed == seed
    assert sc.seq_params(seq) == prm
    seq.append_token(meta["first_token"])
    assert seq.num_tokens == len(prompt) + 1       # the next draw's pos
