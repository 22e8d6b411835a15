"""
Presence / frequency penalty in front of the sampler chain (test infrastructure), exactly as include/dtk.h states it:

  c[i]   occurrences of id i among the counted ids
  c > 0  z'[i] = z[i] - (float32)((float64)pp + (float64)fp * (float64)c[i])      one fp32 subtraction on the raw fp32 logit
  c = 0  z'[i] = z[i], untouched bits

then tests/trunc_oracle.draw (sampling) / oracle.sampling.greedy (arg-max, lowest id on ties) over z'.
"""
from __future__ import annotations

from collections import Counter
from typing import Iterable, Tuple

import numpy as np
import torch

from oracle import sampling

from . import trunc_oracle


def penalise(logits: torch.Tensor, ids: Iterable[int], pp: float, fp: float) -> torch.Tensor:
    """z' of the fp32 row `logits` under the counts of `ids`; pp, fp as the float32 values the device holds"""
    z = logits.detach().to(torch.float32).numpy().copy()
    pp64, fp64 = np.float64(np.float32(pp)), np.float64(np.float32(fp))
    for i, c in Counter(int(t) for t in ids).items():
        pen = np.float32(pp64 + fp64 * np.float64(c))
        z[i] = np.float32(z[i]) - pen          # float32 - float32: one rounding
    return torch.from_numpy(z)


def draw(logits, ids, pp, fp, temperature, top_k, top_p, seed: int, n: int, min_p=0.0, eps=0.0, bad=(), begin=(), first=False,
         always=()) -> Tuple[int, torch.Tensor, float]:
    """(token, filtered probabilities, sample_logprob) of draw index n over the penalised row"""
    return trunc_oracle.draw(penalise(logits, ids, pp, fp), temperature, top_k, top_p, seed, n, min_p, eps, bad, begin, first, always)


def greedy(logits, ids, pp, fp, bad=(), begin=(), first=False) -> int:
    return sampling.greedy(penalise(logits, ids, pp, fp), list(bad), list(begin), first)
