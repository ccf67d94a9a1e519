"""The mixture-of-experts kernels (hip/moe.hip) on the GPU, against the fp64
references and case builders of tests/test_moe_cpu.py."""
import pytest
import torch

import rbg_amd.ops as ops
import test_moe_cpu as mc
from rbg_amd.engine.sequence import SamplingParams
from rbg_amd.models.llama import LlamaForCausalLM

pytestmark = pytest.mark.gpu


def check_grouping(ids, k, E):
    """expert_offsets / sorted_pairs: a permutation of the pairs, grouped by
    expert, ascending pair index (token-major) inside an expert."""
    groupedE, offsets, pairs = ids._moe_group
    flat = ids.flatten().cpu().long()
    offsets, pairs = offsets.cpu().long(), pairs.cpu().long()
    assert groupedE == E and offsets.tolist() == [0] + torch.bincount(
        flat, minlength=E).cumsum(0).tolist()
    assert torch.equal(pairs, torch.sort(flat, stable=True).indices)


@pytest.mark.parametrize("E,k,T,renorm", mc.ROUTE_CASES)
def test_route(E, k, T, renorm):
    logits = mc.route_logits(E, T).cuda()
    ids, w = ops.moe_route(logits, k, renorm)
    mc.check_route(ids, w, logits, k, renorm)
    check_grouping(ids, k, E)


def test_route_groups_a_prefill_batch():
    """2500 tokens x 8: many workgroups, and 5 steps for every wave of the
    one that groups."""
    logits = mc.route_logits(128, 2500, seed=1).cuda()
    ids, w = ops.moe_route(logits, 8, True)
    mc.check_route(ids, w, logits, 8, True)
    check_grouping(ids, 8, 128)


@pytest.mark.parametrize("family", ("integer", "scaled"))
@pytest.mark.parametrize("case", mc.FFN_CASES, ids=str)
def test_ffn(case, family):
    args = [t.cuda() for t in mc.ffn_case(case, family)]
    y = ops.moe_ffn(*args)
    mc.check_ffn(args, family, y)
    # neither the row order inside an expert nor the rest of the batch
    # matters: the reversed batch gives the reversed rows
    flipped = ops.moe_ffn(*(t.flip(0).contiguous() if i in (0, 3, 4) else t
                            for i, t in enumerate(args)))
    assert torch.equal(flipped.flip(0), y)
    assert ops.moe_ffn(args[0][:0], args[1], args[2], args[3][:0],
                       args[4][:0]).shape == (0, case[2])


@pytest.mark.parametrize("name", mc.BAD_ARGS)
def test_ffn_rejects(name):
    args = [t.cuda() for t in mc.ffn_case(mc.FFN_CASES[0], "scaled")]
    with pytest.raises(ValueError):
        ops.moe_ffn(*mc.bad_ffn_args(args, name))


def test_block_on_its_own_logits():
    model = LlamaForCausalLM(mc.moe_config(), torch.device("cuda"))
    block = model.layers[0].mlp
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(40, 512, generator=g) * 0.5).to(mc.BF16).cuda()
    logits = ops.linear(x, block.w_router)
    ids, w = ops.moe_route(logits, 2, True)
    mc.check_route(ids, w, logits, 2, True)
    mc.check_ffn((x, block.w1.data, block.w2.data, ids, w), "scaled",
                 block(x))


class _Recorder:
    """ops._hip with the token count of every moe call noted."""

    def __init__(self, hip):
        self._hip, self.calls = hip, []

    def __getattr__(self, name):
        fn = getattr(self._hip, name)
        if not name.startswith("moe_"):
            return fn

        def noted(*args):
            self.calls.append((name, args[0].shape[0]))
            return fn(*args)
        return noted


def test_engine_eager_equals_graph(monkeypatch):
    prompts = [[7], list(range(17)), list(range(100, 140))]
    runs = []
    for eager in (True, False):
        hip = _Recorder(ops._hip)
        monkeypatch.setattr(ops, "_hip", hip)
        eng = mc.moe_engine("cuda", eager)
        seqs = eng.generate(prompts, SamplingParams(max_new_tokens=7))
        monkeypatch.undo()
        # every page a sequence can own: page 0 is the scratch page that the
        # padding row of the graph's batch-4 bucket writes (kv_cache.py)
        runs.append(([s.output_tokens for s in seqs],
                     eng.runner.cache.kv[:, :, 1:].view(torch.int16).clone()))
        for name in ("moe_route", "moe_ffn"):
            sizes = {T for n, T in hip.calls if n == name}
            assert 58 in sizes and sizes & {3, 4}, (name, sizes)  # both phases
        assert not any(n == "moe_group" for n, T in hip.calls)
    assert all(len(t) == 7 for t in runs[0][0])
    assert runs[0][0] == runs[1][0]
    assert torch.equal(runs[0][1], runs[1][1])
