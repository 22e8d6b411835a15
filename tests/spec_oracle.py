"""Prompt-lookup speculative decoding in plain Python (no GPU, no torch): the lookup rule of HF's PromptLookupCandidateGenerator as the
device kernel states it, a brute-force restatement to check it against, and the acceptance pattern a table of drafts must produce."""
from __future__ import annotations

from typing import List, Optional, Sequence


def lookup(ids: Sequence[int], K: int, max_ngram: int, max_positions: Optional[int] = None) -> List[int]:
    """the drafts behind ids: for n = min(max_ngram, len - 1) down to 1 take the windows equal to the last n ids in ascending index;
    the first whose continuation ids[idx + n : min(idx + n + K, len)] is not empty gives the drafts (possibly fewer than K); no match:
    none.  max_positions: the drafts are cut so that no position reaches it (the last id sits at position len - 1)."""
    ids = list(ids)
    L = len(ids)
    if max_positions is not None:
        K = max(0, min(K, max_positions - 1 - (L - 1)))
    if K <= 0:
        return []
    for n in range(min(max_ngram, L - 1), 0, -1):
        tail = ids[L - n:]
        for idx in range(0, L - n + 1):
            if ids[idx:idx + n] != tail:
                continue
            cont = ids[idx + n:min(idx + n + K, L)]
            if cont:
                return cont
    return []


def lookup_brute(ids: Sequence[int], K: int, max_ngram: int, max_positions: Optional[int] = None) -> List[int]:
    """the same answer from the set of ALL (n, idx) whose window matches the tail and is followed by at least one id: the candidate
    with the longest n wins, the smallest idx among those"""
    ids = list(ids)
    L = len(ids)
    if max_positions is not None:
        K = max(0, min(K, max_positions - L))
    cands = [(-n, idx) for n in range(1, max_ngram + 1) if n <= L - 1
             for idx in range(L) if idx + n < L and all(ids[idx + j] == ids[L - n + j] for j in range(n))]
    if not cands or K <= 0:
        return []
    n, idx = min(cands)
    n = -n
    return ids[idx + n:idx + n + K][:max(0, L - idx - n)]


def drafts_from_table(table: Sequence[int], pos: int, K: int, max_positions: int) -> int:
    """how many drafts a step carries whose vector 0 sits at position pos - 1: table[pos], table[pos + 1], .. up to the first -1"""
    kmax = max(0, min(K, max_positions - pos))
    k = 0
    while k < kmax and pos + k < len(table) and table[pos + k] >= 0:
        k += 1
    return k


def accept_pattern(seq: Sequence[int], table: Sequence[int], T: int, K: int, n_new: int, max_positions: int) -> List[int]:
    """tokens every speculative step accepts when the sequence is seq (prompt of T ids + the plain run's tokens, at least K more than
    n_new of them) and the drafts come from table: the first step has only the prompt's pending row; a step whose previous forward
    carried k drafts accepts the leading drafts that equal the sequence and one more token.  Steps until n_new tokens are out."""
    out, pos, live = [], T, 0
    while pos < T + n_new:
        n = 0
        while n < live and table[pos + n] == seq[pos + n]:
            n += 1
        out.append(n + 1)
        pos += n + 1
        live = drafts_from_table(table, pos, K, max_positions)
    return out
