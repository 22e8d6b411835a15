"""
Length control and logit bias around the penalties (test infrastructure), exactly as include/dtk.h states it.  With cur = the number of
tokens the sequence holds when a token is sampled, n = cur - length_start, E the sequence's EOS ids, for the fp32 row z:

  1. bias     b[i] != 0: z1[i] = z[i] + b[i], one fp32 addition; b[i] == 0: the untouched bits
  2.          tests/penalty_oracle.penalise, then tests/dry_oracle.penalise, on z1, unchanged
  3. decay    i in E and n > decay_start: k = n - decay_start, z3[i] = fl32(z2[i] + fl32(|z2[i]| * m[k])), two fp32 roundings,
              m[k] = min((float32)(pow(factor, k) - 1.0), 2^100), factor a float64
  4. minimum  i in E and n < min_new_tokens: -inf

then tests/trunc_oracle.draw (sampling) / oracle.sampling.greedy (arg-max, lowest id on ties) over the result.  For single-token
biases these are HF's SequenceBiasLogitsProcessor, ExponentialDecayLengthPenalty and MinNewTokensLengthLogitsProcessor, bit for bit,
up to the saturation of m (HF's pow overflows to inf there).
"""
from __future__ import annotations

import math
from typing import Dict, Iterable, Optional, Sequence, Tuple

import numpy as np
import torch

from oracle import sampling

from . import dry_oracle, penalty_oracle, trunc_oracle

M_MAX = np.float32(2.0 ** 100)
BIAS_MAX = 256


def decay_m(factor: float, k: int) -> np.float32:
    """m[k]; the factor is a float64 on the device too"""
    f = float(factor)
    try:
        p = math.pow(f, float(k))
    except OverflowError:
        p = math.inf
    with np.errstate(over="ignore"):
        v = np.float32(np.float64(p) - np.float64(1.0))
    return v if v < M_MAX else M_MAX


def bias(logits: torch.Tensor, pairs: Optional[Dict[int, float]]) -> torch.Tensor:
    """rule 1 on the fp32 row"""
    z = logits.detach().to(torch.float32).numpy().copy()
    for i, b in dict(pairs or {}).items():
        b32 = np.float32(b)
        if b32 != 0:
            z[int(i)] = np.float32(z[int(i)]) + b32          # float32 + float32: one rounding
    return torch.from_numpy(z)


def eos_rules(logits: torch.Tensor, cur: int, eos: Iterable[int] = (), min_new: int = 0, decay: Optional[Tuple[int, float]] = None,
              start: int = 0) -> torch.Tensor:
    """rules 3 and 4 on the (biased, penalised) fp32 row"""
    z = logits.detach().to(torch.float32).numpy().copy()
    n = int(cur) - int(start)
    E = sorted({int(t) for t in eos if 0 <= int(t) < z.shape[0]})
    if decay is not None and n > int(decay[0]):
        m = decay_m(decay[1], n - int(decay[0]))
        with np.errstate(over="ignore", invalid="ignore"):
            for i in E:
                z[i] = np.float32(z[i]) + np.float32(np.abs(np.float32(z[i])) * m)      # two float32 roundings
    if n < int(min_new):
        for i in E:
            z[i] = -np.inf
    return torch.from_numpy(z)


def transform(logits, cur, eos=(), min_new=0, decay=None, start=0, pairs=None, counted=(), pp=0.0, fp=0.0, h=(), dry_m=0.0, dry_b=1.75,
              dry_a=2, breakers=()) -> torch.Tensor:
    """the whole transform in front of the sampler chain: bias, presence / frequency, DRY, decay, minimum length"""
    z = bias(logits, pairs)
    z = dry_oracle.both(z, counted, pp, fp, h, dry_m, dry_b, dry_a, breakers)
    return eos_rules(z, cur, eos, min_new, decay, start)


def draw(logits, cur, temperature, top_k, top_p, seed: int, n: int, min_p=0.0, eps=0.0, bad=(), begin=(), first=False, always=(),
         **shape) -> Tuple[int, torch.Tensor, float]:
    """(token, filtered probabilities, sample_logprob) of draw index n over the transformed row; shape: transform()'s arguments"""
    return trunc_oracle.draw(transform(logits, cur, **shape), temperature, top_k, top_p, seed, n, min_p, eps, bad, begin, first, always)


def greedy(logits, cur, bad=(), begin=(), first=False, **shape) -> int:
    return sampling.greedy(transform(logits, cur, **shape), list(bad), list(begin), first)


def generate(step_logits: Sequence[torch.Tensor], prompt_len: int, eos: Iterable[int], pick, **shape):
    """the oracle loop over given per-step raw logits: token i is pick(transformed row, i) at cur = prompt_len + i; stops behind an EOS"""
    E = {int(t) for t in eos}
    out = []
    for i, z in enumerate(step_logits):
        t = int(pick(transform(z, prompt_len + i, eos=eos, **shape), i))
        out.append(t)
        if t in E:
            break
    return out
