"""CPU self-test of tests/attn_cases.py: the checks the GPU conformance
tests apply must accept a correct kernel and reject wrong ones.

For every case the GPU file parametrises over (the lists are shared, not
copied):
  * the fp64 reference rounded to bf16 passes all families;
  * a bf16-faithful emulation of the kernels' arithmetic (online softmax
    over 32-key tiles, P rounded to bf16 before PV, l summed in fp32, bf16
    output) passes all families -- so the derived bounds are reachable;
  * every mutant (a wrong reference) is rejected by at least one family
    wherever it changes the output.

Mutant accounting.  A mutant "applies" to a case when the configuration has
the thing it gets wrong (attn_cases.*_mutant_applies: a GQA group of one has
no two heads to swap, one KV head cannot be mis-mapped, a lone token has no
future key, ...), decided from the case alone.  Where it applies, it may be
a no-op at a few cases (e.g. "drop last key" on a ctx = 1 row falls back to
the same key): those count as undetected and are capped at 10 % of the
applicable cases.  Where it changes any family's output it MUST be caught.
Run with -s to see which family caught which mutant.
"""
import pytest
import torch

import attn_cases as ac


def _ref_out(data, kind):
    if kind == "decode":
        if data["family"] == "needle":
            return ac.decode_ref64(data["q"], data["kc"], data["vc"],
                                   data["bt"], data["ctx"], data["scale"])
        return data["ref64"]
    if data["family"] == "needle":
        return ac.prefill_ref64(data["q"], data["k"], data["v"],
                                data["cu_q"], data["scale"], data["cu_k"])
    return data["ref64"]


@pytest.mark.parametrize("case", ac.DECODE_CASES, ids=lambda c: c.id)
def test_decode_reference_and_emulation_pass(case):
    for family in ac.DECODE_FAMILIES:
        data = ac.decode_data(case, family)
        ok, msg, _ = ac.check(_ref_out(data, "decode").to(ac.BF16), data)
        assert ok, ("fp64 reference", family, msg)
        emu = ac.decode_emulated(data["q"], data["kc"], data["vc"],
                                 data["bt"], data["ctx"], data["scale"])
        ok, msg, ratio = ac.check(emu, data)
        assert ok, ("bf16 emulation", family, msg)


@pytest.mark.parametrize("case", ac.PREFILL_CASES, ids=lambda c: c.id)
def test_prefill_reference_and_emulation_pass(case):
    for family in ac.prefill_families(case):
        data = ac.prefill_data(case, family)
        ok, msg, _ = ac.check(_ref_out(data, "prefill").to(ac.BF16), data)
        assert ok, ("fp64 reference", family, msg)
        emu = ac.prefill_emulated(data["q"], data["k"], data["v"],
                                  data["cu_q"], data["scale"], data["cu_k"])
        ok, msg, ratio = ac.check(emu, data)
        assert ok, ("bf16 emulation", family, msg)


def _mutant_table(kind, cases, mutants, applies, families_of, get_data,
                  mutate):
    """Per mutant: applicable cases, no-ops, misses, and catches by family."""
    table = {}
    for mut in mutants:
        row = {"applies": 0, "noop": [], "missed": [], "by": {}}
        for case in cases:
            if not applies(mut, case):
                continue
            row["applies"] += 1
            changed, caught = False, []
            for family in families_of(case):
                data = get_data(case, family)
                out = mutate(data, mut)
                base = _ref_out(data, kind).to(ac.BF16)
                if torch.equal(out, base):
                    continue
                changed = True
                if not ac.check(out, data)[0]:
                    caught.append(family)
            if not changed:
                row["noop"].append(case.id)
            elif not caught:
                row["missed"].append(case.id)
            for family in caught:
                row["by"][family] = row["by"].get(family, 0) + 1
        table[mut] = row
    return table


def _print_and_assert(kind, table, families):
    print("\n%s mutants: cases caught per family" % kind)
    print("%-16s %7s %5s %6s  %s" % ("mutant", "applies", "noop", "missed",
                                     "  ".join("%9s" % f for f in families)))
    for mut, row in table.items():
        print("%-16s %7d %5d %6d  %s" % (
            mut, row["applies"], len(row["noop"]), len(row["missed"]),
            "  ".join("%9d" % row["by"].get(f, 0) for f in families)))
    for mut, row in table.items():
        assert row["applies"] > 0, mut
        assert not row["missed"], (mut, "changed the output uncaught at",
                                   row["missed"])
        assert len(row["noop"]) <= 0.10 * row["applies"], (
            mut, "no-op at more than 10 % of its cases", row["noop"])


def test_decode_mutants_are_rejected():
    table = _mutant_table(
        "decode", ac.DECODE_CASES, ac.DECODE_MUTANTS,
        ac.decode_mutant_applies, lambda c: ac.DECODE_FAMILIES,
        ac.decode_data, ac.decode_mutant)
    _print_and_assert("decode", table, ac.DECODE_FAMILIES)


def test_prefill_mutants_are_rejected():
    table = _mutant_table(
        "prefill", ac.PREFILL_CASES, ac.PREFILL_MUTANTS,
        ac.prefill_mutant_applies, ac.prefill_families,
        ac.prefill_data, ac.prefill_mutant)
    _print_and_assert("prefill", table, ac.PREFILL_FAMILIES)


@pytest.mark.parametrize("case", ac.DECODE_CASES[:12:5] + ac.DECODE_CASES[12:],
                         ids=lambda c: c.id)
@pytest.mark.parametrize("family", ac.DECODE_FAMILIES)
def test_poisoned_cache_invariants(case, family):
    data = ac.decode_data(case, family)
    meta, kc, vc = data["meta"], data["kc"], data["vc"]
    bt_u = torch.full((len(case.ctxs), data["bt"].shape[1]), -1,
                      dtype=torch.int32)
    bt_u[data["rows"]] = data["bt"]
    assert (bt_u >= 0).all() and (bt_u < kc.shape[0]).all()
    # width rule
    need = (max(case.ctxs) + 15) // 16 + 2 * max(ac.DECODE_SPLITS) + 2
    assert data["bt"].shape[1] >= need == meta.min_width
    owned = torch.zeros(kc.shape[0], 16, dtype=torch.bool)
    seen = set()
    for s, c in enumerate(case.ctxs):
        n = (c + 15) // 16
        live = bt_u[s, :n].tolist()
        assert live == meta.live_pages[s]
        # no live page is the poison page or page 0; none is shared
        assert meta.poison_page not in live and 0 not in live
        assert not seen.intersection(live)
        seen.update(live)
        # unused columns point at the (valid) poison page
        assert (bt_u[s, n:] == meta.poison_page).all()
        for j, pg in enumerate(live):
            owned[pg, :min(16, c - j * 16)] = True
    assert 0 < meta.poison_page < kc.shape[0]
    # physical pages are permuted: not one ascending contiguous run
    flat = [p for pages in meta.live_pages for p in pages]
    if len(flat) > 3:
        assert flat != sorted(flat)
        for pages in meta.live_pages:
            if len(pages) > 2:
                assert any(b != a + 1 for a, b in zip(pages, pages[1:]))
    # every slot no live key owns holds finite poison
    free = ~owned
    assert (vc.float().permute(0, 2, 1, 3)[free] == ac.V_POISON).all()
    assert (kc.float().permute(0, 2, 1, 3)[free].abs() == ac.K_POISON).all()
    assert torch.isfinite(kc.float()).all() and torch.isfinite(vc.float()).all()
    if family != "needle":
        live_v = vc.float().permute(0, 2, 1, 3)[owned]
        assert (live_v.abs() < ac.V_POISON).all()


def test_needle_targets_cover_every_spot():
    """Replicated needle batches hit key 0, the last key, the page edges and
    both sides of every split boundary of every context."""
    for case in ac.DECODE_CASES:
        if not case.replicate:
            continue
        data = ac.decode_data(case, "needle")
        for u, c in enumerate(case.ctxs):
            if c == 0:
                continue
            hit = set(data["targets"][data["rows"] == u].flatten().tolist())
            assert set(ac.decode_target_spots(c)) <= hit, (case.id, c)
            # targets differ across the heads of one GQA group
            t = data["targets"][data["rows"] == u].view(
                -1, case.kvh, case.group)
            want = min(c, case.group)
            assert all(len(set(g.tolist())) == want
                       for row in t for g in row), (case.id, c)


def test_decode_spots_include_split_boundaries():
    spots = ac.decode_target_spots(80)
    # ctx = 80, splits = 4: per_split = 2 chunks -> boundaries 32, 64
    assert {0, 79, 64, 63, 31, 32} <= set(spots)
    assert ac._split_range(80, 4, 3) == (96, 80)      # an empty split


def test_prefill_cases_run_every_swizzle_branch():
    """nblocks * KVH below 8, a non-multiple of 8 and a multiple of 8 all
    occur, for the 64-row and the 128-row q tile."""
    for qtile in (64, 128):
        seen = set()
        for case in ac.PREFILL_CASES:
            br = ac.swizzle_branches(case, qtile)
            seen |= br
            if br == {"rem"}:
                seen.add("below8")
            if br == {"full", "rem"}:
                seen.add("mixed")
            if br == {"full"}:
                seen.add("multiple")
        assert {"off", "below8", "mixed", "multiple"} <= seen, (qtile, seen)
