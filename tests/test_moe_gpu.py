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


@pytest.mark.parametrize("E,k,T,renorm",
                         mc.ROUTE_CASES_WIDE + mc.ROUTE_CASES_PAIRS)
def test_route_wide(E, k, T, renorm):
    """Expert counts off a multiple of 64 and E = 1, k = 3 / 6 / 7, and pair
    counts either side of the sort's per-wave range."""
    logits = mc.route_logits(E, T).cuda()
    ids, w = ops.moe_route(logits, k, renorm)
    mc.check_route(ids, w, logits, k, renorm)
    check_grouping(ids, k, E)


@pytest.mark.parametrize("E,k,T,hot", mc.ROUTE_CASES_SKEWED)
def test_route_skewed(E, k, T, hot):
    """Every pair (k = 1) or every token's first (k = 8) on one expert, the
    first or the last: 64 peers in every ballot step of the sort."""
    logits = mc.skewed_logits(E, T, hot).cuda()
    ids, w = ops.moe_route(logits, k, True)
    mc.check_route(ids, w, logits, k, True)
    check_grouping(ids, k, E)
    assert bool((ids[:, 0] == hot).all())


@pytest.mark.parametrize("case", mc.FFN_CASES, ids=str)
def test_ffn_combine_order(case):
    """The combine's contract, bit for bit: f32 mul, f32 add, slot order."""
    args = [t.cuda() for t in mc.ffn_case(case, "order")]
    mc.check_ffn(args, "order", ops.moe_ffn(*args))


def test_ffn_sees_an_edit_of_ids():
    """ids edited in place after moe_route: moe_ffn regroups (and checks the
    range again) instead of computing with the routing it no longer has."""
    x, w1, w2, _, _ = (t.cuda() for t in mc.ffn_case(mc.FFN_CASES[1],
                                                     "scaled"))
    g = torch.Generator().manual_seed(5)
    logits = torch.randn(x.shape[0], 8, generator=g).to(mc.BF16).cuda()
    ids, w = ops.moe_route(logits, 2, True)
    before = ops.moe_ffn(x, w1, w2, ids, w)
    old = ids[0].tolist()
    ids[0, 0] = next(e for e in range(8) if e not in old)
    assert ids._moe_group_version != ids._version
    after = ops.moe_ffn(x, w1, w2, ids, w)
    assert torch.equal(after, ops.moe_ffn(x, w1, w2, ids.clone(), w))
    assert not torch.equal(after[0], before[0])
    assert torch.equal(after[1:], before[1:])
    ids[0, 0] = 8
    with pytest.raises(ValueError):
        ops.moe_ffn(x, w1, w2, ids, w)


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
