"""CPU self-test of tests/moe_model_cases.py: the checks the GPU MoE model
tests apply must accept a correct engine and reject wrong ones.

  * every scenario, on a `device="cpu"` engine, reaches the path it is meant
    to, records every (sequence, position, layer) once and passes C1, C2, C3,
    R0 and R1; the share of (row, layer) pairs R1 cannot judge stays under
    the cap;
  * the forced fp64 reference agrees with the project's CPU path run in fp32
    under the same forced routing;
  * every mutant (a wrong engine, patched in for the engine's run only)
    fails the checks named for it in every scenario.  No miss is allowed;
    `ties_to_higher` applies where the run has a tie among a row's k + 1
    largest bf16 logits and must be a no-op elsewhere.

Run with -s to see delta, the ambiguous share and what each mutant failed.
"""
import functools

import pytest
import torch

import model_cases as mc
import moe_model_cases as mm

# as in test_model_cases_cpu: K * 2^-24 with K = 1024 bounds one GEMM, 2^-12
# leaves room for the chain and is 16 times under one bf16 rounding
FP32_TOL = 2.0 ** -12


@functools.lru_cache(maxsize=None)
def _clean(scenario):
    run = mm.run_scenario(scenario, "cpu", True)
    return run, mm.judge(run)


@pytest.mark.parametrize("scenario", mm.SCENARIOS)
def test_cpu_engine_passes_every_check(scenario):
    run, verdict = _clean(scenario)
    mm.assert_paths(run)
    assert not verdict.failures(), verdict.failures()[:8]
    print("\n%s: worst err / e_cpu logits %.3f, K/V %.3f; delta %.4g, worst "
          "R1 margin %.4g of %.4g, ambiguous %.3f of %d pairs" % (
              (run.id,) + verdict.values.worst() + (
                  verdict.delta, max(m for _, m in verdict.r1),
                  verdict.r1_bound, verdict.ambiguous, verdict.pairs)))
    assert verdict.ambiguous <= mm.AMBIGUOUS_CAP


def test_prefix_scenario_borrows_records():
    """The adopted positions have no record of their own and take the first
    sequence's."""
    run, _ = _clean("prefix")
    first, second, third = (r.seq for r in run.rec.seqs.values())
    assert [s.cached_prefix_len for s in (first, second, third)] == [0, 48, 48]
    assert (second.seq_id, 47, 0) not in run.route.records
    assert (second.seq_id, 48, 0) in run.route.records
    got = mm.forced_ids(run, list(run.rec.seqs.values())[2], 48)
    want = mm.forced_ids(run, list(run.rec.seqs.values())[0], 48)
    assert torch.equal(got, want)


def test_forced_reference_matches_fp32_cpu_path():
    run, _ = _clean("churn")
    rec_seq = list(run.rec.seqs.values())[2]
    tokens = (rec_seq.seq.prompt_tokens + rec_seq.seq.output_tokens)[:-1]
    forced = mm.forced_ids(run, rec_seq, len(tokens))
    table = run.engine.runner.model.cos_sin
    with mm.moe_conf():
        model = mc.cpu_model(mm.CONF, run.rec.weights[0], table)
        ref_logits, ref_kv, l64 = mm.moe_forward64(model, tokens, forced)
        up = mc.cpu_model(mm.CONF, run.rec.weights[0], table).float()
        # ops.moe_ffn insists on bf16; the reference behind it rounds to the
        # dtype it is given, fp32 here
        with mc._patched(mm.ops, "moe_ffn", mm.ops.reference.moe_ffn), \
                mc._patched(mc, "cpu_forward", functools.partial(
                    mc.cpu_forward, cache_dtype=torch.float32)):
            got_logits, got_kv, l32 = mm.cpu_forward_forced(up, tokens, forced)
    assert got_logits.dtype == got_kv.dtype == l32.dtype == torch.float32
    worst = max(mc.rel_l2(got_logits[t], ref_logits[t])
                for t in range(len(tokens)))
    assert worst <= FP32_TOL, worst
    assert mc.rel_l2(l32, l64) <= FP32_TOL
    for layer in range(ref_kv.shape[1]):
        for j in range(2):
            err = mc.rel_l2(got_kv[:, layer, j], ref_kv[:, layer, j])
            assert err <= FP32_TOL, (layer, "KV"[j], err)


def test_r1_sees_one_wrong_expert():
    """One recorded id replaced by the row's worst expert: R1 fails on that
    record (and only the routing checks are consulted for it)."""
    run, verdict = _clean("chunked")
    key, (where, margin) = next(iter(run.route.records)), verdict.r1[0]
    assert margin <= verdict.r1_bound
    (lg, ids), = run.route.records[key]
    worst = int(lg.float().argmin())
    assert worst not in ids.tolist()
    run.route.records[key] = [(lg, torch.tensor([int(ids[0]), worst],
                                                dtype=ids.dtype))]
    try:
        failed = mm.judge(run).failed_checks()
    finally:
        run.route.records[key] = [(lg, ids)]
    assert {"R0", "R1"} <= failed


MUTANT_CASES = [(m, s) for m in mm.MUTANTS for s in mm.SCENARIOS]


@pytest.mark.parametrize("mutant,scenario", MUTANT_CASES)
def test_mutant_fails_its_checks(mutant, scenario):
    mut = mm.MUTANTS[mutant]
    run = mm.run_scenario(scenario, "cpu", True, mutant=mut.make)
    if mutant == "ties_to_higher" and not mm.has_ties(_clean(scenario)[0]):
        # nothing for it to break here: it must then change nothing
        clean = _clean(scenario)[0]
        assert [r.sampled for r in run.rec.seqs.values()] == \
            [r.sampled for r in clean.rec.seqs.values()]
        assert not mm.judge(run).failures()
        print("\n%s in %s: no tie among the k + 1 largest, a no-op" % (
            mutant, run.id))
        return
    verdict = mm.judge(run)
    failed = verdict.failed_checks()
    print("\n%s in %s: failed %s (delta %.4g)" % (
        mutant, run.id, sorted(failed), verdict.delta))
    assert set(mut.checks) <= failed, (
        "%s must fail %s, failed %s" % (mutant, mut.checks, sorted(failed)))
    assert not set(mut.passes) & failed, (mutant, sorted(failed))


def test_ties_to_higher_applies_somewhere():
    assert any(mm.has_ties(_clean(s)[0]) for s in mm.SCENARIOS)
