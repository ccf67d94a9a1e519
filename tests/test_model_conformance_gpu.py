"""Model-level conformance on the GPU: the engine (scheduler, model runner,
paged cache, hipGraph decode) driving the HIP kernels through
models/llama.py, against a dense fp64 forward of the same weights.

Scenarios, references and checks live in tests/model_cases.py and are proven
on the CPU by tests/test_model_cases_cpu.py (every mutant there fails the
check named for it).  Here the same code runs with `device="cuda"`: hidden
512, so all four projections reach `skinny_gemm` for M <= 128 and the library
above; 16 decode splits at batch 1, so empty splits occur; the pool starts as
finite poison.

Checks: C1 logits and C2 cache rows within 2 x the error of the project's
own CPU path against fp64 (e_cpu), C3 poison bit for bit; the device-built
rotary table within one fp32 ulp of the CPU-built one.  Each test also
asserts that the path it is meant to reach ran (model_cases.assert_paths).
Run with -s to see the measured err / e_cpu per scenario.

Every conf-qwen scenario decodes at batch 1 somewhere: the regression test
for the one-row `qk_norm` step, which used to raise `k/v stride mismatch`.
"""
import pytest
import torch

import model_cases as mc

pytestmark = pytest.mark.gpu

MODES = ("eager", "graph")
# reload is about captured graphs replaying the live parameters: graph mode
CASES = [(s, c, m) for c in mc.CONFS for s in mc.SCENARIOS for m in MODES
         if not (s == "reload" and m == "eager")]


@pytest.mark.parametrize("conf", mc.CONFS)
def test_rotary_table_built_on_device(conf):
    model = mc.LlamaForCausalLM(mc.model_config(conf), torch.device("cuda"))
    assert model.cos_sin.is_cuda
    err = mc.cos_sin_table_error(model)
    print("\n%s: device vs CPU rotary table, max |diff| %.3g" % (conf, err))
    assert err <= mc.TABLE_TOL


@pytest.mark.parametrize("scenario,conf,mode", CASES)
def test_engine_matches_dense_fp64(scenario, conf, mode):
    assert mc.ops.HAVE_HIP, mc.ops._hip_err
    run = mc.run_scenario(scenario, conf, "cuda", mode == "eager")
    assert run.engine.runner.cache.kv.is_cuda
    assert run.graph_mode == (mode == "graph")
    mc.assert_paths(run)
    verdict = mc.judge(run)
    print("\n%s: worst err / e_cpu logits %.3f, K/V %.3f (%d rows, %d blocks)"
          % ((run.id,) + verdict.worst() + (len(verdict.c1), len(verdict.c2))))
    assert not verdict.failures(), verdict.failures()[:8]
