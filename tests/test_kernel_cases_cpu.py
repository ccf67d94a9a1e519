"""CPU self-test of tests/kernel_cases.py: the checks the GPU conformance
tests apply must accept a correct kernel and reject wrong ones.

For every case the GPU file runs (the lists are shared, not copied):
  * the fp64 reference rounded to bf16 once passes every family;
  * a bf16-faithful emulation (fp32 torch arithmetic in the kernel's order,
    outputs rounded to bf16 once) passes every family, so the derived bounds
    are reachable;
  * every mutant (a deliberately wrong reference) is rejected by at least
    one family in every configuration where it applies.

Mutant accounting.  A mutant "applies" to a configuration that has the thing
it gets wrong (one split has no partial to drop, a single row has no row
above it, a hidden size that fills whole blocks has no padding, ...), decided
from the configuration alone.  Where it applies it must change some family's
output and be caught by one: no no-op and no miss is allowed.  Run with -s
to see the applies / caught table.
"""
import pytest
import torch

import kernel_cases as kc


def _same(a, b):
    return a.shape == b.shape and bool((a.double() == b.double()).all())


def _print_table(title, families, table):
    print("\n%s mutants: configurations caught per family" % title)
    print("%-18s %7s %5s %6s  %s" % ("mutant", "applies", "noop", "missed",
                                     "  ".join("%9s" % f for f in families)))
    for mut, row in table.items():
        print("%-18s %7d %5d %6d  %s" % (
            mut, row["applies"], len(row["noop"]), len(row["missed"]),
            "  ".join("%9d" % row["by"].get(f, 0) for f in families)))
    for mut, row in table.items():
        assert row["applies"] > 0, mut
        assert not row["missed"], (mut, "uncaught at", row["missed"][:8])
        assert not row["noop"], (mut, "changed nothing at", row["noop"][:8])


def _tally(row, config_id, changed, caught):
    row["applies"] += 1
    if not changed:
        row["noop"].append(config_id)
    elif not caught:
        row["missed"].append(config_id)
    for family in set(caught):
        row["by"][family] = row["by"].get(family, 0) + 1


def _new_table(mutants):
    return {m: {"applies": 0, "noop": [], "missed": [], "by": {}}
            for m in mutants}


# ---------------------------------------------------------------------------
# GEMM
# ---------------------------------------------------------------------------

def _gemm_case_results(case, mutants):
    """{mut: (changed, [families that caught it])}, plus the reference and
    emulation asserts, in one pass over the case's batches."""
    res = {m: [False, []] for m in mutants}
    for family in kc.GEMM_FAMILIES:
        data = kc.gemm_data(case, family)
        lo = 0
        for a, w, exp in kc.gemm_batches(data, max_rows=2048):
            L = max(a.shape[0], w.shape[0])
            base = kc.gemm_mutant(data, a, w, lo, None)
            ok, msg, _ = kc.check_gemm(base, exp)
            assert ok, ("fp64 reference", case.id, family, msg)
            # the emulation really multiplies; for the one-hot sweeps a few
            # launches of each chunk are enough to show the check takes it
            pick = sorted({0, L // 2, L - 1})
            emu = kc.gemm_emulated(a[pick] if a.shape[0] > 1 else a,
                                   w[pick] if w.shape[0] > 1 else w)
            sub = {k: (v[pick] if torch.is_tensor(v) and v.shape[0] == L
                       and L > 1 else v) for k, v in exp.items()}
            ok, msg, _ = kc.check_gemm(emu, sub)
            assert ok, ("bf16 emulation", case.id, family, msg)
            for mut in mutants:
                out = kc.gemm_mutant(data, a, w, lo, mut)
                if _same(out, base):
                    continue
                res[mut][0] = True
                if not kc.check_gemm(out, exp)[0]:
                    res[mut][1].append(family)
            lo += L
    return res


def test_gemm_checks_accept_correct_and_reject_mutants():
    table = _new_table(kc.GEMM_MUTANTS)
    for case in kc.GEMM_CASES:
        muts = [m for m in kc.GEMM_MUTANTS
                if kc.gemm_mutant_applies(m, case)]
        for mut, (changed, caught) in _gemm_case_results(case, muts).items():
            _tally(table[mut], case.id, changed, caught)
    _print_table("GEMM", kc.GEMM_FAMILIES, table)


def test_gemm_cases_cover_the_issue_matrix():
    forced = {(c.M, c.force, c.K, c.N) for c in kc.GEMM_CASES if c.force}
    assert forced == {(M, s, s * km, N) for M in kc.GEMM_MS
                      for s in (1, 2, 4, 8) for km in (256, 768)
                      for N in (32, 64, 96)}
    # the automatic choice reaches every instantiated split count
    assert {c.splits for c in kc.GEMM_CASES if not c.force} == {1, 2, 4, 8}
    # all five M_TILES, each with a clamped last row
    tiles = {}
    for M in kc.GEMM_MS:
        mt = next(t for t in (1, 2, 4, 8, 16) if (M + 15) // 16 <= t)
        tiles.setdefault(mt, []).append(M)
    assert sorted(tiles) == [1, 2, 4, 8, 16]
    assert all(any(M % (16 * mt) for M in Ms) for mt, Ms in tiles.items())


def test_gemm_needle_sweeps_hit_every_k_and_every_boundary():
    assert {0, 31, 32, 63, 64, 191, 192, 223, 224, 255, 256, 287, 288, 319,
            320, 511} <= set(kc.gemm_needle_spots(512, 2))
    for case in kc.GEMM_CASES:
        for family, rows in (("needle_a", case.M), ("needle_w", case.N)):
            kidx = kc.gemm_data(case, family)["kidx"]
            assert kidx.shape[1] == rows
            assert set(kidx.flatten().tolist()) == set(range(case.K))


def test_gemm_integer_family_is_exact_in_any_order():
    data = kc.gemm_data(kc.GemmCase(129, 96, 6144, 8), "integer")
    a, w = data["a"].float(), data["w"].float()
    assert set(a.unique().tolist()) <= {-1.0, 0.0, 1.0}
    assert 0.2 < float((a != 0).float().mean()) < 0.3
    want = data["want"].float()
    assert float(want.abs().max()) <= 256
    # split-K in fp32, partials summed back to front: still the same bits
    parts = [a[:, s * 768:(s + 1) * 768] @ w[:, s * 768:(s + 1) * 768].T
             for s in range(8)]
    assert torch.equal(sum(reversed(parts)), want)


# ---------------------------------------------------------------------------
# norms
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("case", kc.NORM_CASES, ids=lambda c: c.id)
def test_norm_reference_and_emulation_pass(case):
    data = kc.norm_data(case)
    out, res = kc.norm_mutant(data, None)
    ok, msg, _ = kc.check_norm(out, res, data)
    assert ok, ("fp64 reference", msg)
    out, res = kc.norm_emulated(data)
    ok, msg, ratio = kc.check_norm(out, res, data)
    assert ok, ("bf16 emulation", msg)
    assert ratio <= 1.0


def test_norm_mutants_are_rejected():
    """A configuration is (op, hidden size): every mutant that applies to it
    must be caught by the spike or the scaled family there."""
    table = _new_table(kc.NORM_MUTANTS)
    configs = {}
    for case in kc.NORM_CASES:
        configs.setdefault((case.fused, case.H), []).append(case)
    for (fused, H), cases in configs.items():
        assert {c.family for c in cases} == set(kc.NORM_FAMILIES)
        res = {m: [False, []] for m in kc.NORM_MUTANTS
               if kc.norm_mutant_applies(m, cases[0])}
        for case in cases:
            if case.family == "spike" and H >= 2048 and case.a != 1.0:
                continue        # the big spike sets: one height is enough
            data = kc.norm_data(case)
            base = kc.norm_mutant(data, None)
            for mut in res:
                out, r = kc.norm_mutant(data, mut)
                if _same(out, base[0]) and (r is None or _same(r, base[1])):
                    continue
                res[mut][0] = True
                if not kc.check_norm(out, r, data)[0]:
                    res[mut][1].append(case.family)
        for mut, (changed, caught) in res.items():
            _tally(table[mut], "%s-h%d" % ("fused" if fused else "norm", H),
                   changed, caught)
    _print_table("norm", kc.NORM_FAMILIES, table)


def test_norm_cases_cover_the_issue_matrix():
    for fused in (False, True):
        mine = [c for c in kc.NORM_CASES if c.fused == fused]
        scaled = {c.shape for c in mine if c.family == "scaled"}
        assert {(T, H) for H in kc.NORM_HS for T in (1, 3)} <= scaled
        assert (160, 128) in scaled and any(len(s) == 3 for s in scaled)
        spikes = {(c.H, c.a, c.eps) for c in mine if c.family == "spike"}
        assert spikes == {(H, a, e) for H in kc.NORM_HS
                          for a in (1 / 64, 1.0, 64.0) for e in (0.0, 1e-5)}
    # the spike visits every element, or one lane of every 8-chunk
    for H in kc.NORM_HS:
        data = kc.norm_data(kc.NormCase("spike", (kc._spike_rows(H), H),
                                        1.0, 0.0, True))
        p = data["spike_at"]
        if H <= 2056:
            assert p.tolist() == list(range(H))
        else:
            assert (p // 8).tolist() == list(range(H // 8))
            assert len(set((p % 8).tolist())) > 1
        # split across x and residual, the other operand zero
        nz_x = (data["x"] != 0).sum(-1)
        nz_r = (data["res"] != 0).sum(-1)
        assert bool(((nz_x + nz_r) == 1).all())
        assert H == 8 or (bool(nz_x.any()) and bool(nz_r.any()))


# ---------------------------------------------------------------------------
# SwiGLU
# ---------------------------------------------------------------------------

@pytest.mark.parametrize("case", kc.SILU_CASES, ids=lambda c: c.id)
def test_silu_checks_accept_correct_and_reject_mutants(case):
    res = {m: [False, []] for m in kc.SILU_MUTANTS
           if kc.silu_mutant_applies(m, case)}
    for family in kc.SILU_FAMILIES:
        x = kc.silu_input(case, family)
        ref64 = kc.silu_ref64(x)
        base = ref64.to(kc.BF16)
        ok, msg, _ = kc.check_silu(base, x, family, ref64)
        assert ok, ("fp64 reference", family, msg)
        ok, msg, ratio = kc.check_silu(kc.silu_emulated(x), x, family, ref64)
        assert ok, ("bf16 emulation", family, msg)
        for mut in res:
            out = kc.silu_mutant(x, mut)
            if _same(out, base):
                continue
            res[mut][0] = True
            if not kc.check_silu(out, x, family, ref64)[0]:
                res[mut][1].append(family)
    table = _new_table(res)
    for mut, (changed, caught) in res.items():
        _tally(table[mut], case.id, changed, caught)
    _print_table("SwiGLU %s" % case.id, kc.SILU_FAMILIES, table)


def test_silu_switch_gates_are_exact_in_fp32():
    g = torch.tensor(kc.SILU_GATES)
    assert torch.equal(1 + torch.exp(-g[:1]), torch.ones(1))
    assert torch.isinf(torch.exp(-g[2:])).all()
    assert torch.equal(g / (1 + torch.exp(-g)), torch.tensor([32.0, 0, -0.0]))
    assert set(kc.SILU_MUTANTS) == {
        m for c in kc.SILU_CASES for m in kc.SILU_MUTANTS
        if kc.silu_mutant_applies(m, c)}


# ---------------------------------------------------------------------------
# RoPE + KV store
# ---------------------------------------------------------------------------

def test_rope_checks_accept_correct_and_reject_mutants():
    table = _new_table(kc.ROPE_MUTANTS)
    for case in kc.ROPE_CASES:
        res = {m: [False, []] for m in kc.ROPE_MUTANTS}
        for family in kc.ROPE_FAMILIES:
            data = kc.rope_data(case, family)
            base = kc.rope_mutant(data, None)
            ok, msg, _ = kc.check_rope(*base, data)
            assert ok, ("fp64 reference", case.id, family, msg)
            ok, msg, ratio = kc.check_rope(*kc.rope_emulated(data), data)
            assert ok, ("bf16 emulation", case.id, family, msg)
            for mut in res:
                out = kc.rope_mutant(data, mut)
                if all(_same(o, b) for o, b in zip(out, base)):
                    continue
                res[mut][0] = True
                if not kc.check_rope(*out, data)[0]:
                    res[mut][1].append(family)
        for mut, (changed, caught) in res.items():
            _tally(table[mut], case.id, changed, caught)
    _print_table("RoPE", kc.ROPE_FAMILIES, table)


def test_rope_check_sees_overwritten_poison_and_a_wrong_v_row():
    data = kc.rope_data(kc.RopeCase(2, 1, 37), "quarter")
    q, k, kcache, vcache = kc.rope_mutant(data, None)
    free = [s for s in range(data["pages"] * kc.ROPE_PAGE)
            if s not in data["slots"].tolist()]
    assert len(free) > 16 and (data["slots"] < 0).sum() >= 7
    bad = kcache.clone()
    bad[free[3] // kc.ROPE_PAGE, 0, free[3] % kc.ROPE_PAGE, 5] = 0.0
    assert not kc.check_rope(q, k, bad, vcache, data)[0]
    bad = vcache.clone()         # -poison: same magnitude, one bit off
    bad[free[0] // kc.ROPE_PAGE, 0, free[0] % kc.ROPE_PAGE, 0] *= -1
    assert not kc.check_rope(q, k, kcache, bad, data)[0]
    s = int(data["slots"][0])
    bad = vcache.clone()
    bad[s // kc.ROPE_PAGE, 0, s % kc.ROPE_PAGE, 127] += 1
    assert not kc.check_rope(q, k, kcache, bad, data)[0]


def test_rope_quarter_table_and_positions():
    table = kc.quarter_table()
    assert table.shape == (64, 128)
    c, s = table[:, :64], table[:, 64:]
    assert bool(((c.abs() + s.abs()) == 1).all())
    assert bool(((c == 0) | (s == 0)).all())
    for case in kc.ROPE_CASES:
        scaled = kc.rope_data(case, "scaled")["pos"].tolist()
        assert kc.ROPE_MAX_POS - 1 in scaled
        assert case.T == 1 or 0 in scaled
