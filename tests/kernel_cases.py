"""Shared inputs, references, bounds and checks for the GEMM / norm / SwiGLU /
RoPE conformance tests.

A plain helper module (not a conftest): tests/test_kernel_cases_cpu.py proves
on the CPU that every check accepts a correct kernel (the fp64 reference and
a bf16-faithful fp32 emulation) and rejects wrong ones (the mutants), and
tests/test_kernel_conformance_gpu.py runs the same cases and the same checks
against the HIP kernels.

Two kinds of input family:
  exact   inputs built so that the arithmetic has no rounding at all (one-hot
          operands, small integers, quarter-turn rotations, saturated gates,
          pure copies).  The check is torch.equal: no tolerance.
  scaled  random data against an fp64 reference computed from the bf16
          inputs, under a bound derived from the arithmetic.  u = 2^-8 is the
          bf16 round-to-nearest relative error.

    GEMM     |got - ref| <= u |ref| + K 2^-24 S + 1e-30,  S = sum_k |a_k w_k|
             (one output rounding + fp32 accumulation in any order)
    rmsnorm  |got - ref| <= (u + H 2^-25 + 2^-20) |ref|, exactly 0 where the
             reference is 0 (output rounding; the fp32 sum of H non-negative
             squares, halved by the rsqrt; rsqrtf and the two fp32 products)
    fused    the new residual is bit-identical to bf16(fp32(x) + fp32(res));
             the normed output is compared with the fp64 norm OF THAT ROUNDED
             residual under (2u + H 2^-25 + 2^-20) |ref|: the kernel sums the
             squares of the unrounded sums, each off by <= u, so the sum of
             squares by <= 2u and its rsqrt by <= u
    SwiGLU   |got - ref| <= (u + 2^-16) |ref| for gates in [-16, 16]: the
             fast exp is x * log2(e) rounded to fp32 then exp2, a relative
             error of |x| 2^-24 <= 2^-20, plus the division and the product
    RoPE     |got - ref| <= u |ref| + 2^-22 (|x1 c| + |x2 s|): two fp32
             products and their sum, then one output rounding
"""
from __future__ import annotations

import functools
import math
import zlib
from typing import Dict, Iterator, List, NamedTuple, Optional, Tuple

import torch

U = 2.0 ** -8
BF16 = torch.bfloat16
INF = float("inf")


def _gen(seed, device="cpu") -> torch.Generator:
    """A generator seeded from an int or from anything with a stable repr
    (str hashes change from process to process; a case's inputs must not)."""
    if not isinstance(seed, int):
        seed = zlib.crc32(repr(seed).encode())
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    return g


def truncate_bf16(x: torch.Tensor) -> torch.Tensor:
    """fp32 -> bf16 by dropping the low 16 bits (the 'forgot to round' bug)."""
    bits = x.float().contiguous().view(torch.int32) & -65536
    return bits.view(torch.float32).to(BF16)


def bits_equal(a: torch.Tensor, b: torch.Tensor) -> bool:
    """Bit-for-bit equality of two bf16 tensors (tells -0 from 0)."""
    return (a.shape == b.shape and a.dtype == b.dtype == BF16 and
            torch.equal(a.contiguous().view(torch.int16),
                        b.contiguous().view(torch.int16)))


def exact_check(got: torch.Tensor, want: torch.Tensor, what: str
                ) -> Tuple[bool, str, float]:
    """Every element equal in value (zeros compare with ==, NaN with
    nothing), with a readable message."""
    if got.shape != want.shape:
        return False, "%s: shape %s, want %s" % (
            what, tuple(got.shape), tuple(want.shape)), INF
    if got.dtype == want.dtype and torch.equal(got, want):
        return True, "", 0.0
    bad = ~(got.double() == want.double())
    if not bool(bad.any()):
        return True, "", 0.0
    first = bad.nonzero()[0].tolist() if bad.any() else []
    return False, "%s: %d of %d elements differ (dtype %s), first at %s" % (
        what, int(bad.sum()), bad.numel(), got.dtype, first), INF


def bound_check(got: torch.Tensor, ref: torch.Tensor, bound: torch.Tensor,
                what: str) -> Tuple[bool, str, float]:
    """|got - ref| <= bound elementwise; a NaN anywhere fails.  Returns
    (ok, message, worst err / bound); a zero bound demands a zero error."""
    if got.shape != ref.shape:
        return False, "%s: shape %s, want %s" % (
            what, tuple(got.shape), tuple(ref.shape)), INF
    err = (got.double() - ref).abs()
    ok = err <= bound
    ratio = torch.where(bound > 0, err / bound,
                        torch.where(err == 0, torch.zeros_like(err),
                                    torch.full_like(err, INF)))
    ratio = torch.nan_to_num(ratio, nan=INF, posinf=INF)
    worst = float(ratio.max()) if ratio.numel() else 0.0
    if bool(ok.all()):
        return True, "", worst
    i = int(ratio.flatten().argmax())
    return False, "%s: %d of %d outside the bound; worst got %r ref %r " \
        "bound %r" % (what, int((~ok).sum()), ok.numel(),
                      float(got.flatten()[i]), float(ref.flatten()[i]),
                      float(bound.flatten()[i])), worst


def _merge(*results) -> Tuple[bool, str, float]:
    ok = all(r[0] for r in results)
    msg = "; ".join(r[1] for r in results if not r[0])
    return ok, msg, max([r[2] for r in results] + [0.0])


# ===========================================================================
# skinny GEMM   C[M,N] = A[M,K] W[N,K]^T
# ===========================================================================

GEMM_MS = (1, 15, 16, 17, 32, 33, 64, 65, 128, 129, 256)
GEMM_SPLITS = (1, 2, 4, 8)
GEMM_KMULS = (256, 768)          # K = splits * 256: 4 steps; * 768: 12 steps
GEMM_NS = (32, 64, 96)
GEMM_AUTO_NK = ((768, 2048), (1536, 1024), (4096, 512), (32, 256))
GEMM_AUTO_MS = (1, 17, 129, 256)
GEMM_FAMILIES = ("needle_a", "needle_w", "integer", "scaled", "sparse")
GEMM_KSTEP = 64
GEMM_MUTANTS = ("drop_last_step", "double_last_step", "drop_slice",
                "drop_split", "swap_cols", "dup_row", "truncate")


def pick_gemm_splits(N: int, K: int) -> int:
    """The launcher's automatic split choice (bindings.cpp), mirrored here
    only to know where the split boundaries of an automatic launch fall."""
    groups = N >> 5
    for s in (8, 4, 2):
        if groups * s <= 512 and groups * s >= 192 and K % (s * 256) == 0:
            return s
    for s in (4, 2):
        if groups * s >= 128 and K % (s * 256) == 0:
            return s
    return 1


class GemmCase(NamedTuple):
    M: int
    N: int
    K: int
    force: int               # force_splits argument; 0 = automatic

    @property
    def splits(self) -> int:
        return self.force or pick_gemm_splits(self.N, self.K)

    @property
    def id(self) -> str:
        return "m%d-n%d-k%d-s%s" % (self.M, self.N, self.K,
                                    self.force or "auto")


GEMM_CASES: List[GemmCase] = [
    GemmCase(M, N, s * kmul, s)
    for M in GEMM_MS for s in GEMM_SPLITS for kmul in GEMM_KMULS
    for N in GEMM_NS
] + [GemmCase(M, N, K, 0) for (N, K) in GEMM_AUTO_NK for M in GEMM_AUTO_MS]


def gemm_needle_spots(K: int, splits: int) -> List[int]:
    """k indices a needle sweep has to hit: 0, K-1, both sides of every 32-
    and 64-boundary of each split's first and last step, and both sides of
    every split boundary."""
    k_wg = K // splits
    spots = {0, K - 1}
    for s in range(splits):
        b, e = s * k_wg, (s + 1) * k_wg
        for edge in (b, b + 32, b + 64, e - 64, e - 32, e):
            spots.update(k for k in (edge - 1, edge) if 0 <= k < K)
    return sorted(spots)


def _sweep(K: int, rows: int) -> torch.Tensor:
    """[launches, rows] k indices that visit every k of K once, in order
    (the tail of the last launch wraps round to k = 0...)."""
    launches = (K + rows - 1) // rows
    return (torch.arange(launches * rows) % K).view(launches, rows)


@functools.lru_cache(maxsize=8)
def gemm_data(case: GemmCase, family: str) -> Dict:
    """Inputs of one (case, family).  The needle families need several
    launches to sweep every k; gemm_batches() materialises them in chunks."""
    M, N, K, _ = case
    g = _gen(("gemm", tuple(case), family))
    data = {"family": family, "case": case}
    if family == "needle_a":
        data["kidx"] = _sweep(K, M)                              # [L, M]
        data["w"] = torch.randn(N, K, generator=g).to(BF16)
        assert set(gemm_needle_spots(K, case.splits)) <= set(
            data["kidx"].flatten().tolist())
    elif family == "needle_w":
        data["kidx"] = _sweep(K, N)                              # [L, N]
        data["a"] = torch.randn(M, K, generator=g).to(BF16)
    elif family == "integer":
        for _ in range(20):
            a = (torch.randint(-1, 2, (M, K), generator=g) *
                 (torch.rand(M, K, generator=g) < 0.375)).to(BF16)
            w = (torch.randint(-1, 2, (N, K), generator=g) *
                 (torch.rand(N, K, generator=g) < 0.375)).to(BF16)
            # randint gives {-1, 0, 1} with 2/3 non-zero; * 3/8 = 1/4
            want = a.double() @ w.double().T
            if float(want.abs().max()) <= 256:
                break
        else:
            raise AssertionError("integer GEMM exceeded 256 twenty times")
        data.update(a=a, w=w, want=want.to(BF16))
        assert torch.equal(data["want"].double(), want)
    elif family == "scaled":
        a = (torch.randn(M, K, generator=g) * 0.5).to(BF16)
        w = (torch.randn(N, K, generator=g) * 0.05).to(BF16)
        data.update(a=a, w=w, ref64=a.double() @ w.double().T,
                    S=a.double().abs() @ w.double().abs().T)
    elif family == "sparse":
        # two non-zeros per row of A: S stays within a small factor of |ref|,
        # so the accumulation term K 2^-24 S is far below u |ref| and the
        # bound pins the output ROUNDING even at K = 6144, where the dense
        # family's accumulation term (about sqrt(K) |ref|) would hide it
        a = torch.zeros(M, K)
        first = torch.randint(0, K, (M, 1), generator=g)
        at = torch.cat([first, (first + 1 + torch.randint(
            0, K - 1, (M, 1), generator=g)) % K], dim=1)     # two distinct k
        a.scatter_(1, at, torch.randn(M, 2, generator=g) * 0.5)
        a = a.to(BF16)
        w = (torch.randn(N, K, generator=g) * 0.05).to(BF16)
        data.update(a=a, w=w, ref64=a.double() @ w.double().T,
                    S=a.double().abs() @ w.double().abs().T)
    else:
        raise ValueError(family)
    return data


def _one_hot_rows(kidx: torch.Tensor, K: int, device) -> torch.Tensor:
    """[L, R] indices -> [L, R, K] bf16 with a single 1 per row."""
    out = torch.zeros(kidx.shape + (K,), dtype=BF16, device=device)
    out.scatter_(-1, kidx.to(device).unsqueeze(-1), 1.0)
    return out


def gemm_batches(data: Dict, device="cpu", max_rows: int = 4096
                 ) -> Iterator[Tuple[torch.Tensor, torch.Tensor, Dict]]:
    """Yield (a [La, M, K], w [Lw, N, K], expect) chunks; La or Lw is 1 when
    that operand is shared by the chunk's launches.  Launch l of the chunk
    multiplies a[l or 0] by w[l or 0]; stack the outputs to [L, M, N] and
    hand them to check_gemm with `expect`."""
    family, case = data["family"], data["case"]
    if family in ("integer", "scaled", "sparse"):
        exp = {"family": family, "K": case.K}
        if family == "integer":
            exp["want"] = data["want"].unsqueeze(0).to(device)
        else:
            exp["ref64"] = data["ref64"].unsqueeze(0).to(device)
            exp["S"] = data["S"].unsqueeze(0).to(device)
        yield (data["a"].unsqueeze(0).to(device),
               data["w"].unsqueeze(0).to(device), exp)
        return
    kidx = data["kidx"]
    L, R = kidx.shape
    step = max(1, max_rows // R)
    for lo in range(0, L, step):
        kc = kidx[lo:lo + step]
        hot = _one_hot_rows(kc, case.K, device)
        if family == "needle_a":
            w = data["w"].to(device)
            # out[l, m, n] = W[n, k_(l, m)]
            want = w.T[kc.to(device)]
            yield hot, w.unsqueeze(0), {"family": family, "want": want}
        else:
            a = data["a"].to(device)
            # out[l, m, n] = A[m, k_(l, n)]
            want = a[:, kc.to(device)].permute(1, 0, 2).contiguous()
            yield a.unsqueeze(0), hot, {"family": family, "want": want}


def check_gemm(got: torch.Tensor, exp: Dict) -> Tuple[bool, str, float]:
    family = exp["family"]
    if family not in ("scaled", "sparse"):
        return exact_check(got, exp["want"], "gemm " + family)
    ref = exp["ref64"]
    bound = U * ref.abs() + exp["K"] * 2.0 ** -24 * exp["S"] + 1e-30
    return bound_check(got, ref, bound, "gemm " + family)


def gemm_emulated(a: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """bf16-faithful: fp32 products and sums, one rounding to bf16."""
    return torch.matmul(a.float(), w.float().transpose(-1, -2)).to(BF16)


def gemm_mutant_applies(mut: Optional[str], case: GemmCase) -> bool:
    if mut == "drop_split":
        return case.splits > 1
    if mut == "dup_row":
        return case.M >= 2
    return True


def _gemm_kmask(case: GemmCase, mut: Optional[str]) -> torch.Tensor:
    """Weight of each k in a (mutated) launch: 1 = summed once."""
    K, splits = case.K, case.splits
    k_wg = K // splits
    t = splits // 2                        # the split that goes wrong
    mask = torch.ones(K, dtype=torch.float64)
    if mut == "drop_last_step":
        mask[(t + 1) * k_wg - GEMM_KSTEP:(t + 1) * k_wg] = 0
    elif mut == "double_last_step":
        mask[(t + 1) * k_wg - GEMM_KSTEP:(t + 1) * k_wg] = 2
    elif mut == "drop_slice":
        mask[torch.arange(K) % GEMM_KSTEP >= 32] = 0
    elif mut == "drop_split":
        mask[t * k_wg:(t + 1) * k_wg] = 0
    return mask


def gemm_mutant(data: Dict, a: torch.Tensor, w: torch.Tensor, lo: int,
                mut: Optional[str]) -> torch.Tensor:
    """The [L, M, N] bf16 output of a wrong kernel (mut = None: the fp64
    reference rounded once) for one gemm_batches chunk that starts at launch
    `lo`.  One-hot operands are multiplied by gathering, which is what the
    product is."""
    family, case = data["family"], data["case"]
    mask = _gemm_kmask(case, mut)
    if family == "needle_a":
        kc = data["kidx"][lo:lo + a.shape[0]]
        out = w[0].double().T[kc] * mask[kc].unsqueeze(-1)
    elif family == "needle_w":
        kc = data["kidx"][lo:lo + w.shape[0]]
        out = (a[0].double() * mask)[:, kc].permute(1, 0, 2)
    else:
        out = torch.matmul(a.double() * mask, w.double().transpose(-1, -2))
    out = out.clone()
    if mut == "swap_cols":
        out = out[..., torch.arange(case.N) ^ 16]
    if mut == "dup_row" and case.M >= 2:
        out[:, case.M - 1] = out[:, case.M - 2]
    if mut == "truncate":
        return truncate_bf16(out.float())
    return out.to(BF16)


# ===========================================================================
# rmsnorm / fused_add_rmsnorm
# ===========================================================================

NORM_HS = (8, 64, 128, 136, 2048, 2056, 4096, 8192)
NORM_TS = (1, 3)
NORM_QK_SHAPE = (4 * 40, 128)          # tokens x heads rows of QK-norm
NORM_3D_SHAPE = (2, 3, 136)
NORM_SPIKES = (1.0 / 64, 1.0, 64.0)
NORM_EPS = (0.0, 1e-5)
NORM_ROW_SCALES = (1e-3, 1.0, 1e3)
NORM_BLOCK = 256                       # threads per row in the kernel
NORM_FAMILIES = ("spike", "scaled")
NORM_MUTANTS = ("drop_chunk", "pad_divisor", "shift_weight",
                "fused_norm_x", "fused_unrounded")


class NormCase(NamedTuple):
    family: str
    shape: Tuple[int, ...]     # x shape; spike: (T, H) with T from H
    a: float                   # spike height (scaled: 0)
    eps: float
    fused: bool

    @property
    def H(self) -> int:
        return self.shape[-1]

    @property
    def id(self) -> str:
        s = "x".join(str(d) for d in self.shape)
        tag = "a%g" % self.a if self.family == "spike" else "rand"
        return "%s-%s-%s-eps%g" % ("fused" if self.fused else "norm", s, tag,
                                   self.eps)


def _spike_rows(H: int) -> int:
    return H if H <= 2056 else H // 8


NORM_CASES: List[NormCase] = [
    NormCase("spike", (_spike_rows(H), H), a, eps, fused)
    for fused in (False, True) for H in NORM_HS for a in NORM_SPIKES
    for eps in NORM_EPS
] + [
    NormCase("scaled", shape, 0.0, 1e-5, fused)
    for fused in (False, True)
    for shape in [(T, H) for H in NORM_HS for T in NORM_TS] +
    [NORM_QK_SHAPE, NORM_3D_SHAPE]
]


@functools.lru_cache(maxsize=4)
def norm_data(case: NormCase) -> Dict:
    """x (and residual) and weight of one case, with the fp64 reference.
    spike: row t is zero except one element of height a at p_t; p_t visits
    every element (H <= 2056) or one random lane of every 8-chunk.  For the
    fused op the spike sits in x on even rows and in the residual on odd
    ones, the other operand being zero."""
    H = case.H
    rows = math.prod(case.shape[:-1])
    g = _gen(("norm", tuple(case)))
    w = torch.randn(H, generator=g).to(BF16)
    if case.family == "spike":
        if rows == H:
            p = torch.arange(H)
        else:
            p = torch.arange(rows) * 8 + torch.randint(0, 8, (rows,),
                                                       generator=g)
        total = torch.zeros(rows, H, dtype=BF16)
        total[torch.arange(rows), p] = case.a
        total = total.view(case.shape)
    else:
        scale = torch.tensor(NORM_ROW_SCALES)[torch.arange(rows) % 3]
        total = None
    data = {"case": case, "w": w}
    if case.family == "spike":
        if case.fused:
            even = (torch.arange(rows) % 2 == 0).view(
                case.shape[:-1] + (1,))
            data["x"] = torch.where(even, total, torch.zeros_like(total))
            data["res"] = torch.where(even, torch.zeros_like(total), total)
        else:
            data["x"] = total
        data["spike_at"] = p
    else:
        def draw():
            r = torch.randn(rows, H, generator=g) * scale.unsqueeze(-1)
            return r.to(BF16).view(case.shape)
        data["x"] = draw()
        if case.fused:
            data["res"] = draw()
    if case.fused:
        # the same IEEE operation as the kernel: fp32 add, one rounding
        data["res_exp"] = (data["x"].float() + data["res"].float()).to(BF16)
    normed_from = data["res_exp"] if case.fused else data["x"]
    data["ref64"] = norm_ref64(normed_from, w, case.eps)
    return data


def _eps64(eps: float) -> float:
    """eps as the kernel sees it: an fp32 launch parameter."""
    return float(torch.tensor(eps, dtype=torch.float32).double())


def norm_ref64(x: torch.Tensor, w: torch.Tensor, eps: float,
               mut: Optional[str] = None) -> torch.Tensor:
    """x rsqrt(mean(x^2) + eps) w in fp64, unrounded, with the sum-of-squares
    and weight mutants."""
    H = x.shape[-1]
    xd = x.double()
    sq = xd * xd
    if mut == "drop_chunk":
        c = (H // 8) // 2
        sq = sq.clone()
        sq[..., c * 8:(c + 1) * 8] = 0
    div = H
    if mut == "pad_divisor":
        nvec = H // 8
        div = (nvec + NORM_BLOCK - 1) // NORM_BLOCK * NORM_BLOCK * 8
    wd = w.double()
    if mut == "shift_weight":
        wd = wd.roll(-8)
    inv = torch.rsqrt(sq.sum(-1, keepdim=True) / div + _eps64(eps))
    return xd * inv * wd


def norm_mutant_applies(mut: Optional[str], case: NormCase) -> bool:
    if mut in ("fused_norm_x", "fused_unrounded"):
        return case.fused
    if mut == "pad_divisor":
        return (case.H // 8) % NORM_BLOCK != 0
    if mut == "shift_weight":
        return case.H > 8
    return True


def norm_mutant(data: Dict, mut: Optional[str]
                ) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """(normed output bf16, new residual or None) of a wrong kernel;
    mut = None is the fp64 reference rounded once."""
    case = data["case"]
    if not case.fused:
        return norm_ref64(data["x"], data["w"], case.eps, mut).to(BF16), None
    res_out = data["res_exp"]
    src = res_out
    if mut == "fused_norm_x":
        src = data["x"]
    elif mut == "fused_unrounded":
        # the sum never rounded to bf16: normed from it, and stored as is
        src = res_out = data["x"].double() + data["res"].double()
    out = norm_ref64(src, data["w"], case.eps,
                     None if mut and mut.startswith("fused") else mut)
    return out.to(BF16), res_out


def norm_emulated(data: Dict) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """fp32 torch arithmetic as the kernel orders it: squares of the
    UNROUNDED sums, the normed values from the rounded residual."""
    case = data["case"]
    w = data["w"].float()
    eps = torch.tensor(case.eps, dtype=torch.float32)
    if case.fused:
        s = data["x"].float() + data["res"].float()
        res_out = s.to(BF16)
        src = res_out.float()
    else:
        s = src = data["x"].float()
        res_out = None
    inv = torch.rsqrt((s * s).sum(-1, keepdim=True) / case.H + eps)
    return (src * inv * w).to(BF16), res_out


def check_norm(out: torch.Tensor, res_out: Optional[torch.Tensor],
               data: Dict) -> Tuple[bool, str, float]:
    case = data["case"]
    ref = data["ref64"].to(out.device)
    k = 2 if case.fused else 1
    bound = (k * U + case.H * 2.0 ** -25 + 2.0 ** -20) * ref.abs()
    results = [bound_check(out, ref, bound, "normed output")]
    if case.family == "spike":
        # belt and braces: everything off the spike is exactly zero
        off = torch.ones(ref.shape, dtype=torch.bool, device=out.device)
        rows = math.prod(case.shape[:-1])
        off.view(rows, case.H)[torch.arange(rows, device=out.device),
                               data["spike_at"].to(out.device)] = False
        assert bool((ref[off] == 0).all()) and bool((ref[~off] != 0).all())
        if out.shape == ref.shape and not bool((out[off] == 0).all()):
            results.append((False, "non-zero off the spike", INF))
    if case.fused:
        if res_out is None:
            results.append((False, "no residual returned", INF))
        else:
            results.append(exact_check(
                res_out, data["res_exp"].to(res_out.device), "new residual"))
    return _merge(*results)


# ===========================================================================
# silu_mul   out = silu(x[..., :I]) * x[..., I:]
# ===========================================================================

SILU_SHAPES = ((1, 8), (3, 24), (5, 4104), (2, 14336))
SILU_GRID_STRIDE_SHAPE = (1200, 14336)          # 17.2 M outputs
SILU_GRID_CAP_VECS = 8192 * 256                 # one pass of the capped grid
SILU_FAMILIES = ("switch", "scaled")
SILU_MUTANTS = ("swap_gate_up", "up_row_stride", "stop_at_cap", "truncate")
SILU_GATES = (32.0, 0.0, -100.0)
_SILU_CHUNK = 64                                # rows per fp64 chunk


class SiluCase(NamedTuple):
    T: int
    I: int

    @property
    def id(self) -> str:
        return "t%d-i%d" % self


SILU_CASES = [SiluCase(*s) for s in SILU_SHAPES + (SILU_GRID_STRIDE_SHAPE,)]
assert SILU_GRID_STRIDE_SHAPE[0] * SILU_GRID_STRIDE_SHAPE[1] // 8 > \
    SILU_GRID_CAP_VECS


def silu_input(case: SiluCase, family: str, device="cpu") -> torch.Tensor:
    """x [T, 2I] bf16, drawn on `device` (the grid-stride case is built where
    it is used).  switch: every gate is 32, 0 or -100; scaled: gates uniform
    in [-16, 16]; up is randn in both."""
    T, I = case
    g = _gen(3000 + T * 7 + I + SILU_FAMILIES.index(family), device)
    x = torch.empty(T, 2 * I, dtype=BF16, device=device)
    if family == "switch":
        pick = torch.randint(0, 3, (T, I), generator=g, device=device)
        x[:, :I] = torch.tensor(SILU_GATES, device=device)[pick].to(BF16)
    else:
        x[:, :I] = ((torch.rand(T, I, generator=g, device=device) * 32 - 16)
                    .to(BF16))
    x[:, I:] = torch.randn(T, I, generator=g, device=device).to(BF16)
    return x


def _silu_rows(x: torch.Tensor, mut: Optional[str]):
    """(gate, up) bf16 views [T, I] as a (mutated) kernel addresses them."""
    T, I2 = x.shape
    I = I2 // 2
    gate, up = x[:, :I], x[:, I:]
    if mut == "swap_gate_up":
        gate, up = up, gate
    elif mut == "up_row_stride":
        # up of row r read at r * I + I + col instead of r * 2I + I + col
        up = torch.as_strided(x.contiguous().view(-1), (T, I), (I, 1), I)
    return gate, up


def silu_ref64(x: torch.Tensor, mut: Optional[str] = None) -> torch.Tensor:
    """fp64 silu(gate) * up, unrounded, in row chunks."""
    gate, up = _silu_rows(x, mut)
    out = torch.empty(gate.shape, dtype=torch.float64, device=x.device)
    for lo in range(0, gate.shape[0], _SILU_CHUNK):
        gd = gate[lo:lo + _SILU_CHUNK].double()
        out[lo:lo + _SILU_CHUNK] = (gd * torch.sigmoid(gd) *
                                    up[lo:lo + _SILU_CHUNK].double())
    return out


def silu_switch_expected(x: torch.Tensor) -> torch.Tensor:
    """What the arithmetic gives exactly for gates in {32, 0, -100}:
    1 + e^-32 rounds to 1 in fp32, so 32 * up; 0; and -100 / inf = 0."""
    I = x.shape[-1] // 2
    gate, up = x[..., :I], x[..., I:]
    return torch.where(gate == 32, (up.float() * 32).to(BF16),
                       torch.zeros_like(up))


def silu_mutant_applies(mut: Optional[str], case: SiluCase) -> bool:
    if mut == "up_row_stride":
        return case.T >= 2
    if mut == "stop_at_cap":
        return case.T * case.I // 8 > SILU_GRID_CAP_VECS
    return True


def silu_mutant(x: torch.Tensor, mut: Optional[str]) -> torch.Tensor:
    ref = silu_ref64(x, mut)
    if mut == "truncate":
        out = torch.empty(ref.shape, dtype=BF16, device=x.device)
        for lo in range(0, ref.shape[0], _SILU_CHUNK):
            out[lo:lo + _SILU_CHUNK] = truncate_bf16(
                ref[lo:lo + _SILU_CHUNK].float())
        return out
    out = ref.to(BF16)
    if mut == "stop_at_cap":
        out.view(-1)[SILU_GRID_CAP_VECS * 8:] = 0
    return out


def silu_emulated(x: torch.Tensor) -> torch.Tensor:
    """fp32: g / (1 + exp(-g)) * up, one rounding."""
    I = x.shape[-1] // 2
    out = torch.empty(x.shape[:-1] + (I,), dtype=BF16, device=x.device)
    for lo in range(0, x.shape[0], _SILU_CHUNK):
        g = x[lo:lo + _SILU_CHUNK, :I].float()
        up = x[lo:lo + _SILU_CHUNK, I:].float()
        out[lo:lo + _SILU_CHUNK] = (g / (1 + torch.exp(-g)) * up).to(BF16)
    return out


def check_silu(got: torch.Tensor, x: torch.Tensor, family: str,
               ref64: Optional[torch.Tensor] = None
               ) -> Tuple[bool, str, float]:
    if family == "switch":
        return exact_check(got, silu_switch_expected(x), "silu switch")
    ref = silu_ref64(x) if ref64 is None else ref64
    if got.shape != ref.shape:
        return False, "silu scaled: shape %s" % (tuple(got.shape),), INF
    # in row chunks: the grid-stride case is 17 M elements of fp64
    worst, bad, msg = 0.0, 0, ""
    step = max(1, (1 << 22) // max(1, ref.shape[-1]))
    for lo in range(0, ref.shape[0], step):
        r = ref[lo:lo + step]
        ok, m, ratio = bound_check(got[lo:lo + step], r,
                                   (U + 2.0 ** -16) * r.abs(), "silu scaled")
        worst = max(worst, ratio)
        if not ok:
            bad += 1
            msg = msg or "rows %d..: %s" % (lo, m)
    return bad == 0, msg, worst


# ===========================================================================
# rope_store_kv
# ===========================================================================

ROPE_D = 128
ROPE_HALF = ROPE_D // 2
ROPE_PAGE = 16
ROPE_HEADS = ((1, 1), (2, 1), (32, 8), (64, 8))          # (QH, KVH)
ROPE_TS = (1, 37)
ROPE_FAMILIES = ("quarter", "scaled")
ROPE_MUTANTS = ("flip_sin", "interleaved", "token_as_pos", "cache_unrotated")
ROPE_QUARTER_ROWS = 64
ROPE_MAX_POS = 4096
ROPE_K_POISON = 24576.0
ROPE_V_POISON = -12288.0
_QUARTER = ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))


class RopeCase(NamedTuple):
    qh: int
    kvh: int
    T: int

    @property
    def id(self) -> str:
        return "qh%d-kvh%d-t%d" % self


ROPE_CASES = [RopeCase(qh, kvh, T) for (qh, kvh) in ROPE_HEADS
              for T in ROPE_TS]


@functools.lru_cache(maxsize=1)
def quarter_table() -> torch.Tensor:
    """[64, 128] fp32 [cos | sin] whose every (pos, d) pair is a quarter
    turn picked by a fixed hash, so the rotation is an exact sign/swap
    permutation and every row differs from every other."""
    pos = torch.arange(ROPE_QUARTER_ROWS).unsqueeze(1)
    d = torch.arange(ROPE_HALF).unsqueeze(0)
    x = pos * ROPE_HALF + d + 1                 # multiply-xorshift mix
    x = (x * 2654435761) % (1 << 32)
    x = x ^ (x >> 15)
    x = (x * 2246822519) % (1 << 32)
    h = (x ^ (x >> 13)) % 4
    cs = torch.tensor(_QUARTER, dtype=torch.float32)[h]       # [64, 64, 2]
    table = torch.cat([cs[..., 0], cs[..., 1]], dim=-1).contiguous()
    assert len({tuple(r.tolist()) for r in table}) == ROPE_QUARTER_ROWS
    for turn in range(4):                 # every row uses all four turns
        assert bool((h == turn).any(dim=1).all())
    return table


@functools.lru_cache(maxsize=1)
def real_table() -> torch.Tensor:
    half = ROPE_HALF
    inv_freq = 1.0 / (500000.0 ** (torch.arange(half, dtype=torch.float64)
                                   / half))
    f = torch.outer(torch.arange(ROPE_MAX_POS, dtype=torch.float64), inv_freq)
    return torch.cat([f.cos(), f.sin()], dim=-1).float().contiguous()


@functools.lru_cache(maxsize=4)
def rope_data(case: RopeCase, family: str) -> Dict:
    """q/k/v [T, H, D] randn, a cos/sin table, positions (never the token
    index), a permuted slot_mapping with -1 entries, and a poison pool."""
    qh, kvh, T = case
    g = _gen(("rope", tuple(case), family))
    q = torch.randn(T, qh, ROPE_D, generator=g).to(BF16)
    k = torch.randn(T, kvh, ROPE_D, generator=g).to(BF16)
    v = torch.randn(T, kvh, ROPE_D, generator=g).to(BF16)
    t = torch.arange(T)
    if family == "quarter":
        table = quarter_table()
        pos = (t * 29 + 7) % ROPE_QUARTER_ROWS
    else:
        table = real_table()
        pos = torch.randint(1, ROPE_MAX_POS - 1, (T,), generator=g)
        pos[0] = ROPE_MAX_POS - 1
        if T > 1:
            pos[1] = 0
    assert bool((pos != t).all())
    pages = (T + ROPE_PAGE - 1) // ROPE_PAGE + 2
    slots = torch.randperm(pages * ROPE_PAGE, generator=g)[:T]
    slots[t % 5 == 3] = -1
    assert T == 1 or (bool((slots < 0).any()) and
                      slots[slots >= 0].tolist() !=
                      sorted(slots[slots >= 0].tolist()))
    data = {"case": case, "family": family, "q": q, "k": k, "v": v,
            "table": table, "pos": pos.to(torch.int32),
            "slots": slots.to(torch.int32), "pages": pages}
    (data["q64"], data["qmag"]), (data["k64"], data["kmag"]) = (
        rope_ref64(x, pos, table) for x in (q, k))
    return data


def rope_pool(data: Dict, device="cpu") -> Tuple[torch.Tensor, torch.Tensor]:
    shape = (data["pages"], data["case"].kvh, ROPE_PAGE, ROPE_D)
    return (torch.full(shape, ROPE_K_POISON, dtype=BF16, device=device),
            torch.full(shape, ROPE_V_POISON, dtype=BF16, device=device))


def rope_ref64(x: torch.Tensor, pos: torch.Tensor, table: torch.Tensor,
               mut: Optional[str] = None
               ) -> Tuple[torch.Tensor, torch.Tensor]:
    """Rotate-half RoPE of x [T, H, D] in fp64 from the fp32 table, and the
    magnitude |x1 c| + |x2 s| each output's rounding bound scales with."""
    T = x.shape[0]
    if mut == "token_as_pos":
        pos = torch.arange(T)
    cs = table[pos.long()].double()
    c, s = cs[:, None, :ROPE_HALF], cs[:, None, ROPE_HALF:]
    if mut == "flip_sin":
        s = -s
    xd = x.double()
    if mut == "interleaved":
        x1, x2 = xd[..., 0::2], xd[..., 1::2]
        out = torch.empty_like(xd)
        out[..., 0::2] = x1 * c - x2 * s
        out[..., 1::2] = x2 * c + x1 * s
        return out, torch.zeros_like(out)
    x1, x2 = xd[..., :ROPE_HALF], xd[..., ROPE_HALF:]
    out = torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], dim=-1)
    mag = torch.cat([(x1 * c).abs() + (x2 * s).abs(),
                     (x2 * c).abs() + (x1 * s).abs()], dim=-1)
    return out, mag


def _scatter_kv(kc, vc, k_rows, v_rows, slots):
    valid = slots >= 0
    sl = slots[valid].long()
    kc[sl // ROPE_PAGE, :, sl % ROPE_PAGE] = k_rows[valid]
    vc[sl // ROPE_PAGE, :, sl % ROPE_PAGE] = v_rows[valid]


def rope_mutant(data: Dict, mut: Optional[str]):
    """(q, k, key_cache, value_cache) a wrong kernel leaves behind; mut =
    None is the fp64 reference rounded once."""
    rot = None if mut == "cache_unrotated" else mut
    q = rope_ref64(data["q"], data["pos"], data["table"], rot)[0].to(BF16)
    k = rope_ref64(data["k"], data["pos"], data["table"], rot)[0].to(BF16)
    kc, vc = rope_pool(data)
    _scatter_kv(kc, vc, data["k"] if mut == "cache_unrotated" else k,
                data["v"], data["slots"])
    return q, k, kc, vc


def rope_emulated(data: Dict):
    """fp32 products and sums, one rounding; K goes to the cache rotated."""
    cs = data["table"][data["pos"].long()]
    c, s = cs[:, None, :ROPE_HALF], cs[:, None, ROPE_HALF:]

    def rot(x):
        x1, x2 = x.float()[..., :ROPE_HALF], x.float()[..., ROPE_HALF:]
        return torch.cat([x1 * c - x2 * s, x2 * c + x1 * s], -1).to(BF16)
    q, k = rot(data["q"]), rot(data["k"])
    kc, vc = rope_pool(data)
    _scatter_kv(kc, vc, k, data["v"], data["slots"])
    return q, k, kc, vc


def check_rope(q: torch.Tensor, k: torch.Tensor, kc: torch.Tensor,
               vc: torch.Tensor, data: Dict) -> Tuple[bool, str, float]:
    """q, k: what the kernel left in place, [T, H, D]; kc, vc: the pool it
    wrote into, which began as rope_pool(data)."""
    dev = q.device
    results = []
    for name, got, ref, mag in (("q", q, data["q64"], data["qmag"]),
                                ("k", k, data["k64"], data["kmag"])):
        ref, mag = ref.to(dev), mag.to(dev)
        if data["family"] == "quarter":
            want = ref.to(BF16)
            assert torch.equal(want.double(), ref)      # exact by design
            results.append(exact_check(got, want, "rotated " + name))
        else:
            results.append(bound_check(
                got, ref, U * ref.abs() + 2.0 ** -22 * mag,
                "rotated " + name))
    # data movement: bit-exact.  The cache copy of K is the rotated k the
    # kernel left in place; V is v; every other slot still holds poison
    want_kc, want_vc = rope_pool(data, dev)
    _scatter_kv(want_kc, want_vc, k, data["v"].to(dev),
                data["slots"].to(dev))
    for name, got, want in (("key_cache", kc, want_kc),
                            ("value_cache", vc, want_vc)):
        ok = bits_equal(got, want)
        results.append((ok, "" if ok else name + " differs: a written row "
                        "is not the source row, or poison was overwritten",
                        0.0 if ok else INF))
    return _merge(*results)
