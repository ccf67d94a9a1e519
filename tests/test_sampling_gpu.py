"""GPU conformance of the fused sampler (hip/sampling.hip) and of the engine's
sampling path, against the fp64 reference in tests/sampling_cases.py.  The
cases, margins and the draw-tolerance clause are described there and proven on
the CPU in tests/test_sampling_cases_cpu.py.
"""
import numpy as np
import pytest
import torch

import sampling_cases as sc
from rbg_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda"


@pytest.fixture(scope="module")
def cases():
    assert ops.HAVE_HIP, f"HIP extension missing: {ops._hip_err!r}"
    return {c.name: c for c in sc.op_cases()}


def _run(groups):
    toks, kept = sc.run_sampler(ops.sample, groups, DEV)
    return toks, kept


@pytest.mark.parametrize("name", ["V1", "V7", "V64", "V1000", "V4099",
                                  "V128256"])
def test_op_matrix(cases, name):
    case = cases[name]
    toks, kept = _run(case.groups)
    v = sc.judge(name, case.groups, toks, kept)
    print("%s: %d draws, %d near ties, %d by the runner-up clause"
          % (name, v.draws, v.near_ties, v.runner_up_used))
    assert not v.failures, "\n".join(v.failures[:10])


def test_tied_fixture_keeps_more_than_k():
    g = sc.tied_fixture()
    toks, kept = _run([g])
    assert not sc.judge("tied", [g], toks, kept).failures
    assert np.all(kept == 4) and g.prm.top_k == 2
    assert set(toks) <= {1, 2, 3, 5}


def test_extreme_uniforms():
    groups = sc.extreme_uniform_groups()
    toks, kept = _run(groups)
    assert not sc.judge("extreme", groups, toks, kept).failures


def test_small_kept_sets():
    """Over 256 seeds every kept token is drawn at least once and nothing
    else is."""
    for g in sc.small_kept_groups():
        toks, kept = _run([g])
        assert not sc.judge("small", [g], toks, kept).failures
        assert set(toks) == set(np.flatnonzero(g.ref.kept)), g.prm


def test_invariance(cases):
    """One (row, params, seed, pos) at row 0 of n = 1, row 2 of n = 3 and row
    129 of n = 130 gives the same token; identical calls are identical."""
    groups = cases["V1000"].groups
    for g in (groups[-2], groups[-1], groups[20]):
        row = sc.Group(g.logits, g.prm, g.seeds[:1], g.poss[:1], None)
        fill = [sc.Group(o.logits, o.prm, o.seeds[:1], o.poss[:1], None)
                for o in groups[:33]] * 4
        assert len(fill) >= 129
        want = g.ref.token[0]
        assert _run([row])[0][0] == want
        assert _run(fill[:2] + [row])[0][2] == want
        assert _run(fill[:129] + [row])[0][129] == want
    args = sc.case_tensors(cases["V4099"].groups, DEV)
    a, b = ops.sample(*args), ops.sample(*args)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("top_p", [1.0, 0.9])
def test_frequencies(top_p):
    """V = 8, 65 536 rows in one launch, seeds 0 .. 65 535: the counts equal
    the reference's counts to within the number of near-tie draws."""
    g = sc.freq_group(top_p)
    toks, kept = _run([g])
    v = sc.judge("freq", [g], toks, kept)
    assert not v.failures, "\n".join(v.failures[:10])
    got = np.bincount(toks, minlength=8)
    want = np.bincount(g.ref.token, minlength=8)
    print("counts", got.tolist(), "reference", want.tolist(),
          "near ties", v.near_ties, "runner-up clause", v.runner_up_used)
    assert np.abs(got - want).sum() <= 2 * v.near_ties


def test_rejected_inputs():
    """Everything bindings.cpp rejects raises RuntimeError before a launch."""
    good = list(sc.case_tensors(sc.small_kept_groups()[:1], DEV))
    ops.sample(*good)

    def bad(i, t):
        args = list(good)
        args[i] = t
        with pytest.raises(RuntimeError):
            ops._hip.sample(*args)

    logits = good[0]
    bad(0, logits.double())                       # dtype
    bad(0, logits.to(torch.bfloat16))
    bad(0, logits.t().contiguous().t())           # non-contiguous
    bad(0, logits[:, ::2])
    bad(0, logits[0])                             # not 2-D
    bad(0, logits[:, :0])                         # V < 1
    bad(0, logits.cpu())                          # device
    for i in range(1, 7):
        bad(i, good[i][:-1])                      # length != n
        bad(i, good[i].cpu())
        wrong = torch.float64 if good[i].is_floating_point() else torch.int16
        bad(i, good[i].to(wrong))
    # n = 0 is not an error
    empty = [t[:0] for t in good]
    toks, kept = ops.sample(*empty)
    assert toks.shape == (0,) and toks.dtype == torch.int64
    assert kept.shape == (0,) and kept.dtype == torch.int32


def test_no_host_sync_and_current_stream():
    """Launches go on the current stream: a call on a side stream is ordered
    after work queued there before it."""
    g = sc.small_kept_groups()[1]
    args = list(sc.case_tensors([g], DEV))
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        logits = torch.zeros_like(args[0])
        logits.copy_(args[0], non_blocking=True)
        toks, kept = ops.sample(logits, *args[1:])
    side.synchronize()
    assert not sc.judge("stream", [g], toks.cpu().numpy(),
                        kept.cpu().numpy()).failures


# ---------------------------------------------------------------------------
# engine level
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("eager", [True, False], ids=["eager", "graph"])
@pytest.mark.parametrize("conf", ["conf-llama", "conf-qwen"])
@pytest.mark.parametrize("scenario", sc.ENGINE_SCENARIOS)
def test_engine_teacher_forced(scenario, conf, eager):
    engine, rec, seqs = sc.run_engine_scenario(scenario, conf, DEV, eager)
    v = sc.assert_engine_run(scenario, engine, rec, seqs)
    print("%s-%s-%s: %d rows, %d near ties, %d by the runner-up clause"
          % (scenario, conf, "eager" if eager else "graph", v.draws,
             v.near_ties, v.runner_up_used))


@pytest.mark.parametrize("eager", [True, False], ids=["eager", "graph"])
def test_engine_is_reproducible(eager):
    runs = [sc.run_engine_scenario("five", "conf-llama", DEV, eager)[2]
            for _ in range(2)]
    assert [s.output_tokens for s in runs[0]] == \
        [s.output_tokens for s in runs[1]]
    assert [s.sampling.seed for s in runs[0]] == \
        [s.sampling.seed for s in runs[1]]
