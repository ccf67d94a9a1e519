"""CPU self-test of tests/model_cases.py: the checks the GPU model
conformance tests apply must accept a correct engine and reject wrong ones.

  * every scenario, on a `device="cpu"` engine (all ops are
    `ops.reference`), reaches the path it is meant to and passes C1, C2, C3;
  * the dense fp64 reference agrees with the project's CPU path run in fp32;
  * the C3 checker sees one flipped element in a never-owned page, in the
    tail of an owned page and in page 0 slot 1;
  * every mutant (a wrong engine, monkeypatched in for the engine's run
    only) fails the check named for it in every scenario where it applies.

Mutant accounting.  A mutant "applies" to a scenario that has the thing it
breaks, decided from the scenario alone (model_cases.MUTANTS).  Where it
applies, one of its named checks must fail: no no-op and no miss is allowed.
Run with -s to see which checks each mutant failed.
"""
import functools

import pytest
import torch

import model_cases as mc

# Dense reference against the fp32 CPU path.  fp32 round-off is 2^-24 per
# operation and the longest dot product has K = 1024 terms, so K * 2^-24 =
# 2^-14 bounds one GEMM in the worst case; 2^-12 leaves room for the chain of
# them and is still 16 times under one bf16 rounding (2^-8) anywhere.
FP32_TOL = 2.0 ** -12

CASES = [(s, c) for c in mc.CONFS for s in mc.SCENARIOS]


@functools.lru_cache(maxsize=None)
def _clean(scenario, conf):
    run = mc.run_scenario(scenario, conf, "cpu", True)
    return run, mc.judge(run)


@pytest.mark.parametrize("scenario,conf", CASES)
def test_cpu_engine_passes_every_check(scenario, conf):
    run, verdict = _clean(scenario, conf)
    mc.assert_paths(run)
    assert not verdict.failures(), verdict.failures()[:8]
    print("\n%s: worst err / e_cpu logits %.3f, K/V %.3f" % (
        (run.id,) + verdict.worst()))


@pytest.mark.parametrize("conf", mc.CONFS)
def test_dense_reference_matches_fp32_cpu_path(conf):
    engine = mc.LLMEngine(mc.engine_config(conf, "cpu", True))
    mc.draw_norm_weights(engine.runner.model)
    assert mc.cos_sin_table_error(engine.runner.model) <= mc.TABLE_TOL
    model = mc.cpu_model(conf, mc.snapshot_params(engine.runner.model),
                         engine.runner.model.cos_sin)
    tokens = mc._prompts(1, (45,))[0]
    ref_logits, ref_kv = mc.dense_forward64(model, tokens)
    got_logits, got_kv = mc.cpu_forward(model.float(), conf, tokens,
                                        cache_dtype=torch.float32)
    assert got_logits.dtype == got_kv.dtype == torch.float32
    worst = max(mc.rel_l2(got_logits[t], ref_logits[t])
                for t in range(len(tokens)))
    assert worst <= FP32_TOL, worst
    for layer in range(ref_kv.shape[1]):
        for j in range(2):
            err = mc.rel_l2(got_kv[:, layer, j], ref_kv[:, layer, j])
            assert err <= FP32_TOL, (layer, "KV"[j], err)


def test_norm_weights_are_drawn_apart():
    """All five kinds of norm weight are non-trivial and pairwise different,
    so swapping any two changes the model."""
    model = mc.LLMEngine(mc.engine_config("conf-qwen", "cpu", True)
                         ).runner.model
    mc.draw_norm_weights(model)
    ws = mc.norm_params(model)
    assert len(ws) == 2 * 4 + 1
    for i, a in enumerate(ws):
        assert 0.5 <= float(a.min()) and float(a.max()) <= 1.5
        assert float(a.float().std()) > 0.2
        for b in ws[i + 1:]:
            assert a.shape != b.shape or not torch.equal(a, b)


@pytest.mark.parametrize("graph_mode", [False, True])
def test_poison_checker_sees_one_flipped_element(graph_mode):
    run, verdict = _clean("mixed", "conf-llama")
    assert verdict.c3 == []
    written, owned = run.rec.written_mask(), run.rec.owned
    never = max(owned) + 1
    tail_page, tail_slot = next(
        (pg, int((~written[pg]).nonzero()[0])) for pg in sorted(owned)
        if not bool(written[pg].all()))
    spots = {"never-owned page": (never, 5), "page 0": (0, 1),
             "tail of owned page": (tail_page, tail_slot)}
    for where, (pg, slot) in spots.items():
        kv = run.kv_after.clone()
        x = kv[1, 1, pg, 0, slot, 77:78].view(torch.int16)
        x ^= 1                                        # one bit of one element
        got = mc.poison_violations(kv, run.poison, written, owned, graph_mode)
        assert got == ["%s: page %d slot %d" % (where, pg, slot)]
    # page 0 slot 0: a violation in eager mode, the scratch slot otherwise
    kv = run.kv_after.clone()
    kv[0, 0, 0, 0, 0, 0] = 1.0
    got = mc.poison_violations(kv, run.poison, written, owned, graph_mode)
    assert got == ([] if graph_mode else ["page 0: page 0 slot 0"])


MUTANT_CASES = [(m, s, c) for m, mut in mc.MUTANTS.items()
                for c in mut.confs for s in mut.scenarios]


@pytest.mark.parametrize("mutant,scenario,conf", MUTANT_CASES)
def test_mutant_fails_its_check(mutant, scenario, conf):
    run = mc.run_mutant(mutant, scenario, conf)
    failed = mc.judge(run).failed_checks()
    print("\n%s in %s: failed %s" % (mutant, run.id, sorted(failed)))
    assert failed & set(mc.MUTANTS[mutant].checks), (
        "%s must fail one of %s, failed %s" % (
            mutant, mc.MUTANTS[mutant].checks, sorted(failed)))


def test_every_scenario_and_conf_has_mutants():
    for scenario, conf in CASES:
        assert sum(1 for m, s, c in MUTANT_CASES
                   if (s, c) == (scenario, conf)) >= 5
    assert set(mc.MUTANTS["k_norm_from_q"].confs) == {"conf-qwen"}
