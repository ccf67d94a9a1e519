"""The mixture-of-experts model on the GPU: the engine (scheduler, model
runner, paged cache, hipGraph decode) driving hip/moe.hip through
models/llama.py's MoEBlock, against an fp64 forward with the engine's own
routing forced on it.

Scenarios, references and checks live in tests/moe_model_cases.py (its
docstring has the definitions of C1, C2, C3, R0, R1 and the cap) and are
proven on the CPU by tests/test_moe_model_cases_cpu.py, where every mutant
fails the checks named for it.

An eager run is judged by all of them.  A graph run's ids live in buffers
allocated inside the capture, so it is judged by C3 on its own pool and by
torch.equal with its eager twin on every logits row and every sequence's
final K/V rows.  Run with -s for the measured figures.
"""
import functools

import pytest

import moe_model_cases as mm

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _eager(scenario):
    return mm.run_scenario(scenario, "cuda", True)


@pytest.mark.parametrize("scenario", mm.SCENARIOS)
def test_eager_engine_matches_forced_fp64(scenario):
    assert mm.ops.HAVE_HIP, mm.ops._hip_err
    run = _eager(scenario)
    assert run.engine.runner.cache.kv.is_cuda and not run.graph_mode
    mm.assert_paths(run)
    verdict = mm.judge(run)
    print("\n%s: worst err / e_cpu logits %.3f, K/V %.3f (%d rows, %d "
          "blocks); delta %.4g, worst R1 margin %.4g of %.4g, ambiguous %.3f "
          "of %d pairs" % (
              (run.id,) + verdict.values.worst() + (
                  len(verdict.values.c1), len(verdict.values.c2),
                  verdict.delta, max(m for _, m in verdict.r1),
                  verdict.r1_bound, verdict.ambiguous, verdict.pairs)))
    assert not verdict.failures(), verdict.failures()[:8]


@pytest.mark.parametrize("scenario", mm.SCENARIOS)
def test_graph_engine_equals_its_eager_twin(scenario):
    run = mm.run_scenario(scenario, "cuda", False)
    assert run.graph_mode and run.route is None
    mm.assert_paths(run)
    failures = mm.graph_failures(run, _eager(scenario))
    assert not failures, failures[:8]
