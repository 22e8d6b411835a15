"""
The planner of model.score_candidates(): which candidates of one prompt share a packed scoring pass (dtk_score_packed).

A pass holds the prompt's first P-1 positions once and one row per candidate token, so it fits when
P - 1 + sum(len_i) <= capacity (the context's max_positions).  Pure host arithmetic: no torch, no library.
"""
from __future__ import annotations

from typing import List, Sequence


def plan_packed_passes(P: int, lens: Sequence[int], capacity: int) -> List[List[int]]:
    """Candidate indices per pass: greedy, in input order — a pass takes candidates while they fit, the first that does not
    opens the next pass.  Concatenating the passes gives 0 .. len(lens)-1; every pass satisfies P - 1 + sum(len_i) <= capacity.
    ValueError: P < 1, an empty candidate, or a candidate that does not fit a pass of its own."""
    P, capacity = int(P), int(capacity)
    if P < 1:
        raise ValueError(f"a prompt of {P} tokens: scoring needs at least one context token")
    room = capacity - (P - 1)
    passes: List[List[int]] = []
    used = 0
    for i, n in enumerate(int(n) for n in lens):
        if n < 1:
            raise ValueError(f"candidate {i} is empty")
        if n > room:
            raise ValueError(f"candidate {i}: {n} tokens behind a prompt of {P} do not fit max_positions {capacity} "
                             f"(at most {max(room, 0)})")
        if not passes or used + n > room:
            passes.append([])
            used = 0
        passes[-1].append(i)
        used += n
    return passes
