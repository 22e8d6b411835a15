"""
DRY in front of the sampler chain (test infrastructure), exactly as include/dtk.h states it:

  table   pen[L] = 0 for L < a;  p = (float64)m;  for L = a .. 64: pen[L] = (float32)min(p, 1e30), p *= (float64)b
  h       the sequence's ids at positions [dry_start, next_pos)
  n < 2 or h[n-1] in B: nothing.  Otherwise for every i in [0, n-2] with h[i] == h[n-1] and h[i+1] not in B:
          L(i) = the largest L in [1, 64] such that for every k in [1, L): i-k >= 0, h[i-k] == h[n-1-k], h[n-1-k] not in B
  M[t]    max L(i) over the i with h[i+1] == t (0: none)
  z'[t]   z[t] - pen[M[t]] where M[t] >= a (one fp32 subtraction), else the untouched bits

behind tests/penalty_oracle.penalise where a presence / frequency pair is on too (two fp32 subtractions in that order), then
tests/trunc_oracle.draw (sampling) / oracle.sampling.greedy (arg-max, lowest id on ties) over z'.
"""
from __future__ import annotations

from typing import Dict, Iterable, Sequence, Tuple

import numpy as np
import torch

from oracle import sampling

from . import penalty_oracle, trunc_oracle

MAX_MATCH = 64
MAX_BREAKERS = 16


def table(m: float, b: float, a: int) -> np.ndarray:
    """pen[0 .. 64] as float32; m, b as the float32 values the device holds"""
    pen = np.zeros(MAX_MATCH + 1, dtype=np.float32)
    p = np.float64(np.float32(m))
    b64 = np.float64(np.float32(b))
    for L in range(a, MAX_MATCH + 1):
        pen[L] = np.float32(min(p, np.float64(1e30)))
        p = p * b64
    return pen


def match_lengths(h: Sequence[int], breakers: Iterable[int] = ()) -> Dict[int, int]:
    """M as a dict id -> match length, over the whole history (no allowed_length here)"""
    B = set(int(t) for t in breakers)
    h = [int(t) for t in h]
    n = len(h)
    M: Dict[int, int] = {}
    if n < 2 or h[n - 1] in B:
        return M
    for i in range(n - 1):
        if h[i] != h[n - 1] or h[i + 1] in B:
            continue
        L = 1
        while L < MAX_MATCH:
            k = L              # is L + 1 possible: the condition at k = L
            if i - k >= 0 and h[i - k] == h[n - 1 - k] and h[n - 1 - k] not in B:
                L += 1
            else:
                break
        t = h[i + 1]
        M[t] = max(M.get(t, 0), L)
    return M


def penalised_ids(h: Sequence[int], a: int, breakers: Iterable[int] = ()) -> Dict[int, int]:
    """the ids DRY touches: M[t] >= a"""
    return {t: L for t, L in match_lengths(h, breakers).items() if L >= a}


def penalise(logits: torch.Tensor, h: Sequence[int], m: float, b: float = 1.75, a: int = 2, breakers: Iterable[int] = ()) -> torch.Tensor:
    """z' of the fp32 row `logits` under the history h"""
    z = logits.detach().to(torch.float32).numpy().copy()
    if np.float32(m) == 0:
        return torch.from_numpy(z)
    pen = table(m, b, a)
    for t, L in penalised_ids(h, a, breakers).items():
        if 0 <= t < z.shape[0]:
            z[t] = np.float32(z[t]) - pen[L]
    return torch.from_numpy(z)


def both(logits, counted, pp, fp, h, m, b=1.75, a=2, breakers=()) -> torch.Tensor:
    """the presence / frequency subtraction first, DRY's second"""
    return penalise(penalty_oracle.penalise(logits, counted, pp, fp), h, m, b, a, breakers)


def draw(logits, h, m, b, a, breakers, temperature, top_k, top_p, seed: int, n: int, min_p=0.0, eps=0.0, bad=(), begin=(), first=False,
         always=(), counted=(), pp=0.0, fp=0.0) -> Tuple[int, torch.Tensor, float]:
    """(token, filtered probabilities, sample_logprob) of draw index n over the penalised row"""
    return trunc_oracle.draw(both(logits, counted, pp, fp, h, m, b, a, breakers), temperature, top_k, top_p, seed, n, min_p, eps, bad, begin,
                             first, always)


def greedy(logits, h, m, b=1.75, a=2, breakers=(), bad=(), begin=(), first=False, counted=(), pp=0.0, fp=0.0) -> int:
    return sampling.greedy(both(logits, counted, pp, fp, h, m, b, a, breakers), list(bad), list(begin), first)
