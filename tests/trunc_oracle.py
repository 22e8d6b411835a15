"""
min-p and epsilon cut-off on top of oracle/sampling.py (test infrastructure): the two stages the sampler runs behind top-p, and the
draw over the final set.  Everything is integer arithmetic on the masses q_i = floor(exp(z_i - zmax) * 2^31) of oracle.sampling:

  min_p   keep i iff kept so far and q_i >= qmin,  qmin = (int64)((double)(float)min_p * 2^31)
  eps     total_m = mass of the set kept after top-k, top-p and min-p;  qe = (int64)((double)(float)eps * (double)total_m);
          keep i iff kept so far and q_i >= qe;  nothing left: the single kept entry of maximal z, lowest id on ties
  draw    kept_total = mass of the final set; target = (kept_total * rand32(seed, n)) >> 32; first index whose running mass exceeds it
"""
from __future__ import annotations

import math
from typing import Tuple

import numpy as np
import torch

from oracle.sampling import integer_masses, kept_mask, rand32

ONE = 1 << 31


def qmin_of(min_p: float) -> int:
    return int(np.float64(np.float32(min_p)) * np.float64(2147483648.0))


def trunc_mask(z: torch.Tensor, q: torch.Tensor, keep: torch.Tensor, min_p: float = 0.0, eps: float = 0.0) -> torch.Tensor:
    """the kept set after min-p and epsilon, from the set `keep` that top-k / top-p left"""
    keep = keep.clone()
    if min_p > 0:
        keep &= q >= qmin_of(min_p)
    if eps > 0:
        total_m = int(torch.where(keep, q, torch.zeros_like(q)).sum())
        qe = int(np.float64(np.float32(eps)) * np.float64(total_m))
        after = keep & (q >= qe)
        if not bool(after.any()):
            zk = torch.where(keep, z, torch.full_like(z, float("-inf")))
            after = torch.zeros_like(keep)
            after[int((zk == zk.max()).nonzero()[0])] = True          # the lowest id among equal maxima
        keep = after
    return keep


def kept_set(logits, temperature, top_k, top_p, min_p=0.0, eps=0.0, bad=(), begin=(), first=False, always=()):
    """(z, q, keep) of the whole chain: suppression lists -> temperature -> top-k -> top-p -> min-p -> epsilon"""
    z, q = integer_masses(logits, temperature, bad, begin, first, always)
    keep = trunc_mask(z, q, kept_mask(z, q, top_k, top_p), min_p, eps)
    return z, q, keep


def draw(logits, temperature, top_k, top_p, seed: int, n: int, min_p=0.0, eps=0.0, bad=(), begin=(), first=False,
         always=()) -> Tuple[int, torch.Tensor, float]:
    """(token, filtered probabilities, sample_logprob = log(q[token] / kept_total)) of draw index n"""
    z, q, keep = kept_set(logits, temperature, top_k, top_p, min_p, eps, bad, begin, first, always)
    qk = torch.where(keep, q, torch.zeros_like(q))
    kept_total = int(qk.sum())
    target = (kept_total * rand32(seed, n)) >> 32
    run = torch.cumsum(qk, 0)
    tok = int(torch.searchsorted(run, torch.tensor(target, dtype=torch.int64), right=True))
    return tok, (qk.double() / float(kept_total)).float(), math.log(int(qk[tok]) / kept_total)
