"""Request/sequence state for continuous batching.

The in-engine analog of one routed request in the reference's P/D flow
(reference examples/inference/pd-disagg-standalone.yaml router role:
a request is prefills on one engine, decodes on another; here Sequence
carries the KV page list that migrates between them).
"""
from __future__ import annotations

import itertools
import time
from dataclasses import dataclass
from typing import List, Optional

from .kv_cache import BlockTable

_ids = itertools.count()

WAITING = "waiting"
RUNNING = "running"
FINISHED = "finished"


@dataclass
class SamplingParams:
    max_new_tokens: int = 128
    temperature: float = 0.0       # 0 = greedy
    top_p: float = 1.0
    stop_token: Optional[int] = None
    ignore_eos: bool = True        # random-init weights: run to max tokens
    top_k: int = 0                 # 0 = off
    min_p: float = 0.0             # 0 = off
    # 64-bit draw seed; None = LLMEngine.add_request assigns one from the
    # engine's own generator (docs/FEATURES.md "Seeded sampling")
    seed: Optional[int] = None

    def validate(self) -> None:
        """Raise ValueError for parameters outside the sampler's domain."""
        t, p, mp = self.temperature, self.top_p, self.min_p
        if not (isinstance(t, (int, float)) and t >= 0 and t < float("inf")):
            raise ValueError(f"temperature must be finite and >= 0, got {t!r}")
        if not (isinstance(p, (int, float)) and 0 < p <= 1):
            raise ValueError(f"top_p must be in (0, 1], got {p!r}")
        if isinstance(self.top_k, bool) or not isinstance(self.top_k, int) \
                or not 0 <= self.top_k < 2 ** 31:
            raise ValueError(f"top_k must be an integer >= 0, got "
                             f"{self.top_k!r}")
        if not (isinstance(mp, (int, float)) and 0 <= mp <= 1):
            raise ValueError(f"min_p must be in [0, 1], got {mp!r}")
        if self.seed is not None and (
                isinstance(self.seed, bool) or not isinstance(self.seed, int)
                or not 0 <= self.seed < 2 ** 64):
            raise ValueError(f"seed must be an integer in [0, 2^64), got "
                             f"{self.seed!r}")

    def wire(self) -> dict:
        """The sampler's parameters as they travel in RPCs and TP ops."""
        return {"temperature": self.temperature, "top_p": self.top_p,
                "top_k": self.top_k, "min_p": self.min_p, "seed": self.seed}

    @classmethod
    def from_wire(cls, max_new_tokens: int, d: Optional[dict] = None,
                  **legacy) -> "SamplingParams":
        """Build from a (possibly partial) wire dict; absent fields keep
        their defaults, so peers that send temperature only still work."""
        d = dict(d or {})
        d.update({k: v for k, v in legacy.items() if v is not None})
        seed = d.get("seed")
        return cls(max_new_tokens=int(max_new_tokens),
                   temperature=float(d.get("temperature", 0.0)),
                   top_p=float(d.get("top_p", 1.0)),
                   top_k=int(d.get("top_k", 0)),
                   min_p=float(d.get("min_p", 0.0)),
                   seed=None if seed is None else int(seed))


class Sequence:
    def __init__(self, prompt_tokens: List[int],
                 sampling: Optional[SamplingParams] = None,
                 seq_id: Optional[int] = None):
        self.seq_id = seq_id if seq_id is not None else next(_ids)
        self.prompt_tokens = list(prompt_tokens)
        self.output_tokens: List[int] = []
        self.sampling = sampling or SamplingParams()
        self.status = WAITING
        self.block_table: Optional[BlockTable] = None
        self.arrival_time = time.monotonic()
        self.first_token_time: Optional[float] = None
        self.finish_time: Optional[float] = None
        # P/D disaggregation: sequences migrated from a prefill engine carry
        # their KV pages + first generated token instead of re-prefilling
        self.imported_kv = False
        # prefix cache: leading tokens whose KV pages were adopted from the
        # cache (prefill runs only on the suffix)
        self.cached_prefix_len = 0
        # chunked prefill: prompt tokens whose KV is already computed; the
        # scheduler feeds [num_prefilled, num_prefilled+chunk) per step
        self.num_prefilled = 0
        self.chunk_len = 0

    @property
    def num_prompt_tokens(self) -> int:
        return len(self.prompt_tokens)

    @property
    def num_tokens(self) -> int:
        return len(self.prompt_tokens) + len(self.output_tokens)

    @property
    def last_token(self) -> int:
        return (self.output_tokens[-1] if self.output_tokens
                else self.prompt_tokens[-1])

    def append_token(self, tok: int) -> None:
        if self.first_token_time is None:
            self.first_token_time = time.monotonic()
        self.output_tokens.append(tok)

    def should_stop(self) -> bool:
        if len(self.output_tokens) >= self.sampling.max_new_tokens:
            return True
        if (not self.sampling.ignore_eos and self.sampling.stop_token is not None
                and self.output_tokens
                and self.output_tokens[-1] == self.sampling.stop_token):
            return True
        return False

    def ttft(self) -> Optional[float]:
        if self.first_token_time is None:
            return None
        return self.first_token_time - self.arrival_time
