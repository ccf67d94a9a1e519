"""Shared reference, cases and checks for the seeded-sampling tests.

A plain helper module (not a conftest, no `gpu` marker, needs no HIP
extension).  tests/test_sampling_cases_cpu.py proves on the CPU that the
reference meets the specification's fixed points, that the checks accept
`ops.reference.sample` and the engine on `device="cpu"`, and that they reject
wrong samplers (the mutants); tests/test_sampling_gpu.py runs the same cases
and the same checks against hip/sampling.hip and the engine on the GPU.

Reference.  `ref_group` is an fp64 numpy implementation of the semantics in
docs/FEATURES.md ("Seeded sampling"), written apart from `ops.reference`:
integer-exact Philox4x32-10, fp64 filters, fp64 Gumbel scores.  For every draw
it returns the kept set, the winner, the runner-up and the gap between their
scores.

Margins (conditions on the INPUTS, asserted by the reference itself, so the
kept set of a case is unambiguous for any fp32 implementation):

  top-k   none: comparisons only.
  min-p   no logit within 2^-20 * (1 + |l_max| + T |ln min_p|) of the
          threshold l_max + T ln(min_p).  min_p == 1 is exempt: ln 1 is
          exactly 0 in every format, the threshold IS l_max, and the test is
          the exact comparison l >= l_max.
  top-p   the renormalised prefix mass at the last kept token and at its
          predecessor both differ from float32(top_p) by more than 2^-16.

Draw tolerance.  With fp32 arithmetic and 1-ulp logs a score is off by at
most 2^-22 * (1 + |z| + |g|), so with
    delta = 2^-22 * (2 + |z_a| + |g_a| + |z_b| + |g_b|)
for winner a and runner-up b: a sampler's token must be the winner; where the
reference's own gap is below delta the runner-up is accepted too.  At most
0.2 % of a case's draws may be such near ties (asserted for the reference
alone when the case is built).
"""
from __future__ import annotations

import functools
import math
from typing import Callable, Dict, List, NamedTuple, Optional, Sequence, Tuple

import numpy as np
import torch

U64 = np.uint64
MASK32 = U64(0xFFFFFFFF)
NEAR_TIE_BUDGET = 0.002
MINP_MARGIN = 2.0 ** -20
TOPP_MARGIN = 2.0 ** -16

PHILOX_KNOWN_ANSWERS = (
    ((0, 0, 0, 0), (0, 0),
     (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2,
     (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344),
     (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
)

MUTANTS = (
    "topk_keeps_k_minus_1", "topk_drops_ties", "topp_stops_before_boundary",
    "topp_at_T1", "topp_over_all_tokens", "minp_relative_to_sum",
    "filter_order_swapped", "noise_ignores_pos", "noise_keyed_by_row",
    "noise_block_is_i", "seed_high_word_dropped", "u_without_half",
)


# ---------------------------------------------------------------------------
# noise
# ---------------------------------------------------------------------------

def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Philox4x32-10 on broadcastable uint64 arrays of 32-bit words."""
    c = [np.asarray(x, dtype=U64) & MASK32 for x in (c0, c1, c2, c3)]
    k0 = np.asarray(k0, dtype=U64) & MASK32
    k1 = np.asarray(k1, dtype=U64) & MASK32
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*c, k0, k1)
    for _ in range(10):
        p0 = U64(0xD2511F53) * c0
        p1 = U64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> U64(32)) ^ c1 ^ k0, p1 & MASK32,
                          (p0 >> U64(32)) ^ c3 ^ k1, p0 & MASK32)
        k0 = (k0 + U64(0x9E3779B9)) & MASK32
        k1 = (k1 + U64(0xBB67AE85)) & MASK32
    return c0, c1, c2, c3


def gumbel_noise(idx: np.ndarray, seeds: np.ndarray, poss: np.ndarray,
                 mutant: Optional[str] = None,
                 rows: Optional[np.ndarray] = None) -> np.ndarray:
    """g[m, K] in fp64 for token indices idx[K] and m (seed, pos) pairs."""
    idx = np.asarray(idx, dtype=U64)[None, :]
    seeds = np.asarray(seeds, dtype=U64)[:, None]
    poss = np.asarray(poss, dtype=np.int64).astype(U64)[:, None] & MASK32
    if mutant == "noise_ignores_pos":
        poss = np.zeros_like(poss)
    if mutant == "noise_keyed_by_row":
        seeds = np.asarray(rows, dtype=U64)[:, None]
    k0, k1 = seeds & MASK32, seeds >> U64(32)
    if mutant == "seed_high_word_dropped":
        k1 = np.zeros_like(k1)
    block = idx if mutant == "noise_block_is_i" else idx >> U64(2)
    words = philox4x32_10(block, poss, 0, 0, k0, k1)
    lane = np.broadcast_to(idx & U64(3), words[0].shape).astype(np.int64)
    x = np.choose(lane, words)
    m = (x >> U64(8)).astype(np.float64)
    half = 0.0 if mutant == "u_without_half" else 0.5
    with np.errstate(divide="ignore"):
        return -np.log(-np.log((m + half) * 2.0 ** -24))


# ---------------------------------------------------------------------------
# filters
# ---------------------------------------------------------------------------

class Params(NamedTuple):
    T: float = 1.0
    top_k: int = 0
    top_p: float = 1.0
    min_p: float = 0.0


def _f32(x: float) -> float:
    return float(np.float32(x))


def _topk(l, keep, k, mutant):
    V = l.shape[0]
    if mutant == "topk_keeps_k_minus_1":
        k -= 1
    if not 0 < k < V:
        return keep
    order = np.argsort(-l, kind="stable")
    if mutant == "topk_drops_ties":
        out = np.zeros(V, dtype=bool)
        out[order[:k]] = True
        return keep & out
    return keep & (l >= l[order[k - 1]])


def _minp(l, keep, T, mp, mutant, check):
    if not mp > 0:
        return keep
    lmax = l.max()
    if mutant == "minp_relative_to_sum":
        with np.errstate(over="ignore"):
            e = np.where(l > -np.inf, np.exp((l - lmax) / T), 0.0)
        return keep & (e / e.sum() >= mp)
    thr = lmax + T * math.log(mp)
    if check and mp != 1.0:
        fin = l[l > -np.inf]
        margin = MINP_MARGIN * (1 + abs(lmax) + T * abs(math.log(mp)))
        assert np.abs(fin - thr).min() > margin, \
            "min_p margin violated: choose other logits for this case"
    return keep & (l >= thr)


def _topp(l, keep, T, p, mutant, check):
    if not p < 1:
        return keep
    if mutant == "topp_at_T1":
        T = 1.0
    idx = np.flatnonzero(keep)
    if idx.size == 0:                    # only a mutant can get here
        return keep
    order = idx[np.argsort(-l[idx], kind="stable")]
    lmax = l.max()
    w = np.exp((l[order] - lmax) / T)
    total = w.sum()
    if mutant == "topp_over_all_tokens":
        fin = l > -np.inf
        total = np.exp((l[fin] - lmax) / T).sum()
    cum = np.cumsum(w) / total
    hit = np.flatnonzero(cum >= p)
    j = int(hit[0]) if hit.size else len(order) - 1
    if check and mutant is None:
        assert abs(cum[j] - p) > TOPP_MARGIN and \
            (j == 0 or abs(cum[j - 1] - p) > TOPP_MARGIN), \
            "top_p margin violated: choose other logits for this case"
    if mutant == "topp_stops_before_boundary":
        j = max(j - 1, 0)
    return keep & (l >= l[order[j]])


def kept_set(logits32: np.ndarray, prm: Params, mutant: Optional[str] = None,
             check: bool = True) -> np.ndarray:
    """Boolean kept mask of one row for T > 0 (fp64; margins asserted)."""
    l = np.asarray(logits32, dtype=np.float32).astype(np.float64)
    l = np.where(np.isnan(l), -np.inf, l)
    T, p, mp = _f32(prm.T), _f32(prm.top_p), _f32(prm.min_p)
    keep = l > -np.inf
    if not keep.any():
        return keep
    if mutant == "filter_order_swapped":
        keep = _topp(l, keep, T, p, mutant, check)
        keep = _minp(l, keep, T, mp, mutant, check)
        return _topk_among(l, keep, int(prm.top_k))
    keep = _topk(l, keep, int(prm.top_k), mutant)
    keep = _minp(l, keep, T, mp, mutant, check)
    return _topp(l, keep, T, p, mutant, check)


def _topk_among(l, keep, k):
    """top-k applied last, among what is left (the swapped-order mutant)."""
    idx = np.flatnonzero(keep)
    if not 0 < k < l.shape[0] or idx.size <= k:
        return keep
    kth = np.sort(l[idx])[::-1][k - 1]
    return keep & (l >= kth)


# ---------------------------------------------------------------------------
# reference draw
# ---------------------------------------------------------------------------

class GroupRef(NamedTuple):
    kept: np.ndarray          # bool [V]
    num_kept: int
    token: np.ndarray         # int64 [m]
    runner_up: np.ndarray     # int64 [m], -1 where there is none
    gap: np.ndarray           # fp64 [m], inf where there is no runner-up
    delta: np.ndarray         # fp64 [m]

    @property
    def near_tie(self) -> np.ndarray:
        return self.gap < self.delta


def ref_group(logits32, prm: Params, seeds, poss,
              mutant: Optional[str] = None, rows=None,
              check: bool = True) -> GroupRef:
    """Reference for one logits row and one parameter set under m (seed,
    pos) pairs."""
    seeds = np.asarray(seeds, dtype=U64)
    m = seeds.shape[0]
    l = np.asarray(logits32, dtype=np.float32).astype(np.float64)
    l = np.where(np.isnan(l), -np.inf, l)
    none = np.full(m, -1, dtype=np.int64)
    inf = np.full(m, np.inf)
    if not (l > -np.inf).any():
        return GroupRef(np.zeros(l.shape, bool), 0,
                        np.zeros(m, np.int64), none, inf, np.zeros(m))
    T = _f32(prm.T)
    if T == 0:
        kept = np.zeros(l.shape, bool)
        kept[int(np.argmax(l))] = True
        return GroupRef(kept, 1, np.full(m, int(np.argmax(l)), np.int64),
                        none, inf, np.zeros(m))
    kept = kept_set(logits32, prm, mutant, check)
    idx = np.flatnonzero(kept)
    if idx.size == 0:                    # only a mutant can get here
        return GroupRef(kept, 0, np.zeros(m, np.int64), none, inf,
                        np.zeros(m))
    z = l[idx] / T
    g = gumbel_noise(idx, seeds, poss, mutant, rows)
    score = z[None, :] + g
    a = np.argmax(score, axis=1)                     # first (lowest) maximum
    ar = np.arange(m)
    token = idx[a].astype(np.int64)
    if idx.size == 1:
        return GroupRef(kept, 1, token, none, inf, np.zeros(m))
    rest = score.copy()
    rest[ar, a] = -np.inf
    b = np.argmax(rest, axis=1)
    gap = score[ar, a] - score[ar, b]
    delta = 2.0 ** -22 * (2 + np.abs(z[a]) + np.abs(g[ar, a]) +
                          np.abs(z[b]) + np.abs(g[ar, b]))
    return GroupRef(kept, int(idx.size), token, idx[b].astype(np.int64), gap,
                    delta)


def ref_row(logits32, prm: Params, seed: int, pos: int,
            mutant: Optional[str] = None, row: int = 0,
            check: bool = True) -> GroupRef:
    return ref_group(logits32, prm, [seed], [pos], mutant, [row], check)


# ---------------------------------------------------------------------------
# cases: groups of (one logits row, one parameter set, m (seed, pos) pairs)
# ---------------------------------------------------------------------------

SEED_MAX = 2 ** 64 - 1


def seed_pos_pairs(m: int, salt: int) -> Tuple[List[int], List[int]]:
    """m pairs: seed 0, seed 2^64-1, two seeds differing only in the high
    word, pos 0, then a fixed pseudo-random tail."""
    rng = np.random.Generator(np.random.PCG64(1000 + salt))
    seeds = [0, SEED_MAX, 0x00000001_89abcdef, 0x80000001_89abcdef,
             0x89abcdef, 12345]
    poss = [0, 1, 7, 7, 7, 0]
    while len(seeds) < m:
        seeds.append(int(rng.integers(0, 2 ** 64, dtype=np.uint64)))
        poss.append(int(rng.integers(0, 4096)))
    return seeds[:m], poss[:m]


def make_logits(family: str, V: int, rng: np.random.Generator) -> np.ndarray:
    if family == "randn3":
        return (rng.standard_normal(V) * 3).astype(np.float32)
    if family == "peaked":
        l = (rng.standard_normal(V) * 0.5).astype(np.float32)
        l[int(rng.integers(0, V))] += np.float32(9.0)
        return l
    if family == "tied":
        # few distinct values: ties at the argmax and at every k-th value
        vals = np.array([2.0, 1.0, 0.5, -1.0, -3.0], dtype=np.float32)
        return vals[rng.integers(0, len(vals), V)]
    if family == "holes":
        l = (rng.standard_normal(V) * 3).astype(np.float32)
        l[rng.random(V) < 0.3] = -np.inf
        l[rng.random(V) < 0.2] = np.nan
        if not (l > -np.inf).any():
            l[V // 2] = 0.25
        return l
    if family == "allneginf":
        l = np.full(V, -np.inf, dtype=np.float32)
        l[::3] = np.nan
        return l
    raise ValueError(family)


class Group(NamedTuple):
    logits: np.ndarray        # fp32 [V]
    prm: Params
    seeds: List[int]
    poss: List[int]
    ref: GroupRef


class Case(NamedTuple):
    name: str
    groups: List[Group]

    @property
    def rows(self) -> int:
        return sum(len(g.seeds) for g in self.groups)


def build_group(family: str, V: int, prm: Params, m: int, salt: int
                ) -> Group:
    """Logits for which the margins hold: the first of a fixed stream of
    candidate rows that satisfies them (a condition on the inputs)."""
    seeds, poss = seed_pos_pairs(m, salt)
    for attempt in range(64):
        rng = np.random.Generator(np.random.PCG64([salt, attempt, V]))
        logits = make_logits(family, V, rng)
        try:
            ref = ref_group(logits, prm, seeds, poss)
        except AssertionError:
            continue
        return Group(logits, prm, seeds, poss, ref)
    raise AssertionError("no candidate row meets the margins: %s V=%d %r"
                         % (family, V, prm))


def finish_case(name: str, groups: List[Group]) -> Case:
    case = Case(name, groups)
    near = sum(int(g.ref.near_tie.sum()) for g in groups)
    assert near <= NEAR_TIE_BUDGET * case.rows, \
        "%s: %d of %d reference draws are near ties" % (name, near, case.rows)
    return case


def _k_values(V: int) -> List[int]:
    return [0, 1, 2, 50, V - 1, V, V + 5]


@functools.lru_cache(maxsize=None)
def op_cases() -> Tuple[Case, ...]:
    """The op-level matrix.  One case per vocabulary size; inside a case the
    groups differ in parameters, so every launch mixes them (greedy rows
    included)."""
    cases = []
    for V in (1, 7, 64, 1000, 4099):
        groups = []
        salt = V * 100
        m = 8

        def add(family, prm, m=m):
            nonlocal salt
            salt += 1
            groups.append(build_group(family, V, prm, m, salt))

        for T in (0.0, 0.5, 1.0, 2.0):
            add("randn3", Params(T))
        for k in _k_values(V):
            add("randn3", Params(1.0, top_k=k))
            add("tied", Params(1.0, top_k=k))
        for p in (0.95, 0.5, 1e-6):
            add("randn3", Params(1.0, top_p=p))
            add("peaked", Params(0.5, top_p=p))
        for mp in (0.05, 0.5, 1.0):
            add("randn3", Params(1.0, min_p=mp))
            add("tied", Params(2.0, min_p=mp))
        # all three filters together
        add("randn3", Params(1.0, top_k=50, top_p=0.95, min_p=0.05))
        add("randn3", Params(0.5, top_k=V - 1, top_p=0.5, min_p=0.5))
        add("peaked", Params(2.0, top_k=2, top_p=0.95, min_p=0.05))
        add("tied", Params(1.0, top_k=2, top_p=0.95, min_p=0.5))
        add("randn3", Params(0.0, top_k=2, top_p=0.5, min_p=0.5))  # greedy
        # -inf / NaN rows
        add("holes", Params(1.0))
        add("holes", Params(1.0, top_k=2, top_p=0.95))
        add("holes", Params(0.0))
        add("allneginf", Params(1.0, top_k=2, top_p=0.5, min_p=0.05))
        add("allneginf", Params(0.0))
        # one group with the full set of (seed, pos) pairs
        add("randn3", Params(1.0, top_k=50, top_p=0.95), m=64)
        add("randn3", Params(1.0), m=64)
        cases.append(finish_case("V%d" % V, groups))
    # the flagship vocabulary: one batch of 4 rows
    V = 128256
    groups = [build_group("randn3", V, prm, 1, 7000 + i) for i, prm in
              enumerate((Params(1.0), Params(1.0, top_k=50, top_p=0.9),
                         Params(0.5, top_p=0.5, min_p=0.05), Params(0.0)))]
    cases.append(finish_case("V128256", groups))
    return tuple(cases)


def tied_fixture() -> Group:
    """k = 2 over [1, 3, 3, 3, 0, 3]: four tokens tie at the k-th value, so
    num_kept (4) exceeds k."""
    logits = np.array([1, 3, 3, 3, 0, 3], dtype=np.float32)
    seeds, poss = seed_pos_pairs(64, 1)
    prm = Params(1.0, top_k=2)
    g = Group(logits, prm, seeds, poss, ref_group(logits, prm, seeds, poss))
    assert g.ref.num_kept == 4 > prm.top_k
    return g


def small_kept_groups() -> List[Group]:
    """Kept sets of 1..4 tokens under 256 seeds at one position."""
    out = []
    seeds = list(range(256))
    poss = [5] * 256
    base = np.array([0.3, 2.0, -1.0, 1.5, 1.9, -4.0, 0.0, 1.0, 2.0, -2.0],
                    dtype=np.float32)
    for prm in (Params(1.0, top_k=1), Params(1.0, top_k=3),
                Params(2.0, top_k=4), Params(1.0, min_p=0.5),
                Params(1.0, top_k=8, top_p=0.5)):
        out.append(Group(base, prm, seeds, poss,
                         ref_group(base, prm, seeds, poss)))
        assert 1 <= out[-1].ref.num_kept <= 4
    return out


def extreme_uniform_groups() -> List[Group]:
    """(seed, pos, token) triples, found by search, whose 24-bit uniform sits
    at an end of its range.
    x >> 8 == 0 at token 1: u = 2^-25 and g = -ln(25 ln 2) = -2.85, so a
    token 12 above the rest still wins; without the +0.5, u = 0 and it
    cannot.  x >> 8 == 2^24 - 1 at token 4: u = 1 - 2^-25 is not an fp32
    number, g = 17.33; a u rounded to 1 makes g infinite and lets a token 30
    below the rest win."""
    out = []
    lo = np.array([0.0, 12.0, 0.5, -1.0, 0.25, 1.0, -0.5, 0.75], np.float32)
    hi = np.array([0.0, 0.5, -1.0, 0.25, -30.0, 1.0, -0.5, 0.75], np.float32)
    for logits, seed, tok, wins in ((lo, 1212062, 1, True),
                                    (hi, 2810418, 4, False)):
        words = philox4x32_10(tok >> 2, 3, 0, 0, seed, 0)
        m = int(words[tok & 3]) >> 8
        assert m == (0 if wins else 2 ** 24 - 1)
        prm = Params(1.0)
        ref = ref_group(logits, prm, [seed], [3])
        assert (ref.token[0] == tok) == wins and not ref.near_tie[0]
        out.append(Group(logits, prm, [seed], [3], ref))
    return out


FREQ_LOGITS = np.array([1.5, 0.0, -1.0, 2.25, 0.5, -2.5, 1.0, -0.25],
                       dtype=np.float32)
FREQ_N = 65536


@functools.lru_cache(maxsize=None)
def freq_group(top_p: float) -> Group:
    seeds = list(range(FREQ_N))
    poss = [3] * FREQ_N
    prm = Params(1.0, top_p=top_p)
    return Group(FREQ_LOGITS, prm, seeds, poss,
                 ref_group(FREQ_LOGITS, prm, seeds, poss))


def freq_expected(group: Group) -> np.ndarray:
    """N * p over the kept set (fp64 softmax renormalised)."""
    l = group.logits.astype(np.float64) / _f32(group.prm.T)
    w = np.where(group.ref.kept, np.exp(l - l.max()), 0.0)
    return FREQ_N * w / w.sum()


# ---------------------------------------------------------------------------
# running a sampler on a case and judging it
# ---------------------------------------------------------------------------

def seed_i64(seed: int) -> int:
    seed &= SEED_MAX
    return seed - 2 ** 64 if seed >= 2 ** 63 else seed


def case_tensors(groups: Sequence[Group], device: str = "cpu"):
    """The seven tensors of one launch: every (seed, pos) pair of every group
    is a row."""
    rows, T, k, p, mp, sd, ps = [], [], [], [], [], [], []
    for g in groups:
        m = len(g.seeds)
        rows.append(torch.from_numpy(g.logits).unsqueeze(0).expand(m, -1))
        T += [g.prm.T] * m
        k += [g.prm.top_k] * m
        p += [g.prm.top_p] * m
        mp += [g.prm.min_p] * m
        sd += [seed_i64(s) for s in g.seeds]
        ps += list(g.poss)
    f32 = dict(dtype=torch.float32, device=device)
    i32 = dict(dtype=torch.int32, device=device)
    return (torch.cat(rows).contiguous().to(device), torch.tensor(T, **f32),
            torch.tensor(k, **i32), torch.tensor(p, **f32),
            torch.tensor(mp, **f32),
            torch.tensor(sd, dtype=torch.int64, device=device),
            torch.tensor(ps, **i32))


Sampler = Callable[..., Tuple[torch.Tensor, torch.Tensor]]


def run_sampler(sampler: Sampler, groups: Sequence[Group],
                device: str = "cpu") -> Tuple[np.ndarray, np.ndarray]:
    toks, kept = sampler(*case_tensors(groups, device))
    assert toks.dtype == torch.int64 and kept.dtype == torch.int32
    return toks.cpu().numpy(), kept.cpu().numpy()


class Verdict(NamedTuple):
    failures: List[str]
    draws: int
    near_ties: int            # reference draws with gap < delta
    runner_up_used: int       # draws accepted only by the runner-up clause


def judge(name: str, groups: Sequence[Group], toks: np.ndarray,
          kept: np.ndarray) -> Verdict:
    fails: List[str] = []
    at = near = used = 0
    for gi, g in enumerate(groups):
        m = len(g.seeds)
        t, c, ref = toks[at:at + m], kept[at:at + m], g.ref
        at += m
        near += int(ref.near_tie.sum())
        tag = "%s group %d (%r)" % (name, gi, g.prm)
        bad = np.flatnonzero(c != ref.num_kept)
        if bad.size:
            fails.append("%s: num_kept %d != %d at draw %d"
                         % (tag, c[bad[0]], ref.num_kept, bad[0]))
        if ref.num_kept:
            inside = (t >= 0) & (t < g.logits.shape[0])
            inside[inside] = ref.kept[t[inside]]
            if not inside.all():
                fails.append("%s: token %d outside the kept set"
                             % (tag, t[np.flatnonzero(~inside)[0]]))
        ok = t == ref.token
        alt = ~ok & ref.near_tie & (t == ref.runner_up)
        used += int(alt.sum())
        bad = np.flatnonzero(~(ok | alt))
        if bad.size:
            i = bad[0]
            fails.append("%s: draw %d (seed %d pos %d) token %d, reference "
                         "%d (runner-up %d, gap %.3g, delta %.3g); %d draws "
                         "differ" % (tag, i, g.seeds[i], g.poss[i], t[i],
                                     ref.token[i], ref.runner_up[i],
                                     ref.gap[i], ref.delta[i], bad.size))
        finite = np.where(np.isnan(g.logits), -np.inf, g.logits)
        if (finite > -np.inf).any():
            amax = int(np.argmax(finite))
            # greedy: the lowest-index argmax; top_k = 1 and top_p = 1e-6
            # keep the maximum and its ties, so a unique maximum is certain
            unique = (finite == finite.max()).sum() == 1
            if _f32(g.prm.T) == 0 or (unique and (
                    g.prm.top_k == 1 or g.prm.top_p <= 1e-6)):
                if not (t == amax).all():
                    fails.append("%s: expected the argmax %d" % (tag, amax))
    return Verdict(fails, at, near, used)


def mutant_outputs(groups: Sequence[Group], mutant: str
                   ) -> Tuple[np.ndarray, np.ndarray]:
    """What a sampler with this defect would return for the case."""
    toks, kept, at = [], [], 0
    for g in groups:
        m = len(g.seeds)
        ref = ref_group(g.logits, g.prm, g.seeds, g.poss, mutant,
                        rows=np.arange(at, at + m), check=False)
        toks.append(ref.token)
        kept.append(np.full(m, ref.num_kept, dtype=np.int32))
        at += m
    return np.concatenate(toks), np.concatenate(kept)


# ---------------------------------------------------------------------------
# engine level: teacher-forced check of every sampled row
# ---------------------------------------------------------------------------

class Sampled(NamedTuple):
    seq: object
    pos: int
    logits: np.ndarray        # fp32 [V], the row the engine sampled from
    batch: int                # rows in that sample_device call


class SampleRecorder:
    """Wraps `runner.sample_device`: keeps every logits row together with the
    sequence that was sampled and the position the token will take."""

    def __init__(self, engine):
        self.runner = engine.runner
        self.rows: List[Sampled] = []
        self.batches: List[Tuple[int, ...]] = []

    def __enter__(self):
        orig = self.runner.sample_device

        def sample_device(logits, seqs):
            rows = logits.detach().float().cpu().numpy()
            assert rows.shape[0] == len(seqs)
            self.batches.append(tuple(s.seq_id for s in seqs))
            for i, seq in enumerate(seqs):
                self.rows.append(Sampled(seq, seq.num_tokens, rows[i].copy(),
                                         len(seqs)))
            return orig(logits, seqs)

        self.runner.sample_device = sample_device
        return self

    def __exit__(self, *exc):
        del self.runner.sample_device      # back to the class's method
        return False


def seq_params(seq) -> Params:
    s = seq.sampling
    return Params(s.temperature, s.top_k, s.top_p, s.min_p)


def judge_engine(rec: SampleRecorder) -> Verdict:
    """Teacher-forced: the token the engine appended at `pos` must be the
    reference draw from the recorded row under the sequence's own parameters,
    seed and pos (same delta clause).  Margins are not asserted on engine
    logits (they are not ours to choose); a row on a filter boundary would
    show up as a failure to be looked at, not hidden."""
    fails: List[str] = []
    near = used = 0
    for i, r in enumerate(rec.rows):
        seq = r.seq
        assert seq.sampling.seed is not None
        all_tokens = seq.prompt_tokens + seq.output_tokens
        got = all_tokens[r.pos]
        ref = ref_row(r.logits, seq_params(seq), seq.sampling.seed, r.pos,
                      check=False)
        if ref.near_tie[0]:
            near += 1
        if got == ref.token[0]:
            continue
        if ref.near_tie[0] and got == ref.runner_up[0]:
            used += 1
            continue
        fails.append("row %d seq %d pos %d (%r, seed %d): engine %d, "
                     "reference %d (gap %.3g)"
                     % (i, seq.seq_id, r.pos, seq_params(seq),
                        seq.sampling.seed, got, ref.token[0], ref.gap[0]))
    return Verdict(fails, len(rec.rows), near, used)


ENGINE_SCENARIOS = ("five", "churn", "chunked", "prefix")


def _sp(n, T=0.0, **kw):
    from rbg_amd.engine.sequence import SamplingParams
    return SamplingParams(max_new_tokens=n, temperature=T, **kw)


FIVE_PARAMS = (
    dict(T=0.0),                                            # greedy
    dict(T=1.0, seed=11),
    dict(T=0.7, top_k=20, seed=2 ** 64 - 1),
    dict(T=1.5, top_p=0.9, seed=0),
    dict(T=1.0, top_k=50, top_p=0.95, min_p=0.02),          # engine's seed
)


def run_engine_scenario(scenario: str, conf: str, device: str, eager: bool):
    """Build one small engine and drive a non-greedy scenario through it.
    Returns (engine, recorder, sequences)."""
    import model_cases as mc
    from rbg_amd.engine.engine import LLMEngine
    kw = {"max_prefill_tokens": 24} if scenario == "chunked" else {}
    engine = LLMEngine(mc.engine_config(conf, device, eager, **kw))
    mc.draw_norm_weights(engine.runner.model)
    rec = SampleRecorder(engine)
    with rec:
        if scenario == "five":
            prompts = mc._prompts(600, (3, 17, 31, 48, 70))
            seqs = [engine.add_request(p, _sp(6, **kw)) for p, kw in
                    zip(prompts, FIVE_PARAMS)]
            mc._drain(engine)
        elif scenario == "churn":
            seqs = [engine.add_request(p, _sp(n, **kw)) for p, n, kw in zip(
                mc._prompts(610, (9, 30, 50)), (2, 4, 7),
                (dict(T=1.0, seed=5), dict(T=0.0),
                 dict(T=0.8, top_k=10, top_p=0.9, seed=6)))]
            assert engine.step() == "prefill" and engine.step() == "decode"
            assert seqs[0].status == "finished"
            seqs.append(engine.add_request(
                mc._prompts(611, (21,))[0],
                _sp(5, T=1.2, min_p=0.05, seed=7)))
            mc._drain(engine)
        elif scenario == "chunked":
            seqs = [engine.add_request(p, _sp(4, **kw)) for p, kw in zip(
                mc._prompts(620, (100, 40)),
                (dict(T=1.0, top_p=0.9, seed=21), dict(T=0.5, seed=22)))]
            mc._drain(engine)
        elif scenario == "prefix":
            base = mc._prompts(630, (50,))[0]
            seqs = []
            for sd in (31, 32):
                seqs += engine.generate(
                    [base], _sp(4, T=1.0, top_k=40, seed=sd))
            assert seqs[1].cached_prefix_len > 0
        else:
            raise ValueError(scenario)
    return engine, rec, seqs


def assert_engine_run(scenario: str, engine, rec: SampleRecorder, seqs
                      ) -> Verdict:
    for s in seqs:
        assert s.status == "finished"
        assert len(s.output_tokens) == s.sampling.max_new_tokens
        assert s.sampling.seed is not None
    verdict = judge_engine(rec)
    assert not verdict.failures, "\n".join(verdict.failures[:10])
    # a greedy request in mixed batches: the exact argmax of its own rows
    for r in rec.rows:
        if r.seq.sampling.temperature == 0:
            got = (r.seq.prompt_tokens + r.seq.output_tokens)[r.pos]
            assert got == int(np.argmax(r.logits))
    if scenario in ("five", "churn"):
        assert any(r.batch > 1 and r.seq.sampling.temperature == 0
                   for r in rec.rows), "no greedy row in a mixed batch"
    if scenario == "churn":
        sizes = {len(b) for b in rec.batches}
        assert len(sizes) > 1, "the batch never changed shape"
    return verdict
