"""Prompt-lookup drafting with a corpus of earlier programs in plain Python (no GPU, no torch): the rule of include/dtk.h in the
single-pass formulation the two device kernels use, the nested loops of the rule verbatim to check it against, and the tokens every
speculative step accepts when the drafts come from that lookup.

A corpus is a flat list of ids in which a negative entry separates two sequences.  Every lookup returns (drafts, source, n): source is
NONE / HISTORY / CORPUS (DTK_SPEC_FROM_*), n the n-gram size that matched (0: none)."""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

NONE, HISTORY, CORPUS = 0, 1, 2
MAX_NGRAM, CORPUS_MAX, BLOCK = 16, 65536, 1024


def _kmax(L: int, K: int, max_positions: Optional[int]) -> int:
    """K cut as the step cuts it: K, max_positions - 1 - (len - 1), NV - 1 = K, 3"""
    k = min(K, 3)
    if max_positions is not None:
        k = min(k, max_positions - 1 - (L - 1))
    return max(0, k)


def flatten(seqs: Sequence[Sequence[int]]) -> List[int]:
    """the non-empty sequences joined by one -1 separator: what generate(prompt_lookup_corpus=seqs) hands to the device"""
    flat: List[int] = []
    for s in seqs:
        s = [int(t) for t in s]
        if not s:
            continue
        if flat:
            flat.append(-1)
        flat += s
    return flat


def lookup_corpus_brute(ids: Sequence[int], corpus: Sequence[int], K: int, max_ngram: int,
                        max_positions: Optional[int] = None) -> Tuple[List[int], int, int]:
    """the nested loops of the rule, verbatim"""
    h, c = list(ids), list(corpus)
    L, C = len(h), len(c)
    kmax = _kmax(L, K, max_positions)
    if kmax <= 0:
        return [], NONE, 0
    for n in range(min(max_ngram, L - 1), 0, -1):
        tail = h[L - n:]
        for idx in range(0, L - n):             # 1. own history, unchanged HF rule
            if h[idx:idx + n] == tail:
                return h[idx + n:idx + n + kmax], HISTORY, n
        for idx in range(0, C - n):             # 2. otherwise the corpus
            if c[idx:idx + n] == tail and c[idx + n] >= 0:
                drafts = []
                for t in c[idx + n:idx + n + kmax]:
                    if t < 0:
                        break
                    drafts.append(t)
                return drafts, CORPUS, n
    return [], NONE, 0


def corpus_best(ids: Sequence[int], corpus: Sequence[int], max_ngram: int) -> List[int]:
    """k_spec_corpus: per block of BLOCK end positions the largest key (L << 32) | (0xffffffff - e) over the positions e with c[e] equal
    to the tail's last id and a continuation id behind them, L = the backward equalities capped at nmax; 0 = none"""
    h, c = list(ids), list(corpus)
    L, C = len(h), len(c)
    nmax = min(max_ngram, MAX_NGRAM, L - 1)
    blocks = [0] * ((C + BLOCK - 1) // BLOCK)
    if nmax < 1:
        return blocks
    tail = h[L - nmax:]
    for e in range(C):
        if e + 1 < C and c[e] == tail[-1] and c[e + 1] >= 0:
            n = 1
            while n < nmax and e - n >= 0 and c[e - n] == tail[nmax - 1 - n]:
                n += 1
            blocks[e // BLOCK] = max(blocks[e // BLOCK], (n << 32) | (0xffffffff - e))
    return blocks


def lookup_corpus(ids: Sequence[int], corpus: Sequence[int], K: int, max_ngram: int,
                  max_positions: Optional[int] = None) -> Tuple[List[int], int, int]:
    """the kernels' formulation: one pass over the corpus gives (n_c, e_c), the longest n-gram it matches and the lowest end position of
    such a window; the descending-n loop over the history then takes the corpus continuation at n == n_c when the history has no window"""
    h, c = list(ids), list(corpus)
    L, C = len(h), len(c)
    kmax = _kmax(L, K, max_positions)
    best = max(corpus_best(h, c, max_ngram), default=0)
    n_c, e_c = best >> 32, 0xffffffff - (best & 0xffffffff)
    if kmax <= 0 or L < 2:
        return [], NONE, 0
    for n in range(min(max_ngram, L - 1), 0, -1):
        tail = h[L - n:]
        first = next((idx for idx in range(L - n) if h[idx:idx + n] == tail), None)
        if first is not None:
            return h[first + n:first + n + kmax], HISTORY, n
        if n == n_c:
            drafts = []
            while len(drafts) < kmax and e_c + 1 + len(drafts) < C and c[e_c + 1 + len(drafts)] >= 0:
                drafts.append(c[e_c + 1 + len(drafts)])
            return drafts, CORPUS, n
    return [], NONE, 0


def steps_corpus(seq: Sequence[int], T: int, K: int, max_ngram: int, corpus: Sequence[int], n_new: int,
                 max_positions: int) -> List[Tuple[int, int, int]]:
    """the speculative steps of a sequence whose true tokens are seq (prompt of T ids + the plain run's tokens, at least K more than
    n_new of them), drafts from the lookup: per step (tokens accepted, drafts it verified, source of those drafts).  The first step
    has only the prompt's pending row; a step whose previous forward carried k drafts accepts the leading drafts that equal the
    sequence and one more token.  Steps until n_new tokens are out."""
    seq = list(seq)
    out, pos, drafts, src = [], T, [], NONE
    while pos < T + n_new:
        n = 0
        while n < len(drafts) and drafts[n] == seq[pos + n]:
            n += 1
        out.append((n + 1, len(drafts), src))
        pos += n + 1
        drafts, src, _ = lookup_corpus(seq[:pos], corpus, K, max_ngram, max_positions)
    return out


def accept_pattern_corpus(seq: Sequence[int], T: int, K: int, max_ngram: int, corpus: Sequence[int], n_new: int,
                          max_positions: int) -> List[int]:
    """given the true token sequence, the tokens every step accepts"""
    return [a for a, _, _ in steps_corpus(seq, T, K, max_ngram, corpus, n_new, max_positions)]
