"""Prompt-lookup drafting from a corpus of earlier programs (dtk_spec_set_corpus), on the device: k_spec_corpus +
k_spec_draft alone against the plain-Python rule — bit-equal drafts, count, source and n-gram size at the thread, wave and block edges
of the corpus pass — then generate(prompt_lookup_corpus=...) against PLAIN STEPS OF SLOT 0 on the same context: the same tokens and
bit-equal log-probabilities whatever the corpus holds, the accepted tokens per step exactly the oracle's, and the life of the corpus
(cleared after every call, one re-capture per change between none and some, none for a replacement, the refusals)."""
from __future__ import annotations

import ctypes as C
import gc

import numpy as np
import pytest
import torch

from detikzify_amd import _lib
from tests import spec_corpus_oracle as oracle
from tests.helpers import TINY
from tests.test_gpu_spec import EOS, EXTRA, GREEDY, IMG, N_NEW, SAMPLED, _bits, _load, _prompt, plain_slot0, same_as_plain
from tests.test_spec_corpus_host import KNOWN

pytestmark = pytest.mark.gpu

NONE, HISTORY, CORPUS = oracle.NONE, oracle.HISTORY, oracle.CORPUS
BLOCK = oracle.BLOCK
TAIL = (77, 30, 9, 77, 30)
K, NGRAM = 3, 16


@pytest.fixture(scope="module")
def ctx4():
    """detikzify-tiny with 4 slots + the plain runs of slot 0 on it, before anything speculated"""
    model, proc = _load(4)
    ids, px = _prompt(proc, tail=TAIL)
    truth = {name: plain_slot0(model, ids, px, N_NEW + EXTRA, cfg) for name, cfg in (("greedy", GREEDY), ("sampled", SAMPLED))}
    yield model, proc, ids, px, truth
    del model
    gc.collect()


def _same(model, ids, corpus, k, ng, cap=None):
    got = model.spec_lookup_corpus(ids, corpus, k, ng, max_positions=cap)
    want = oracle.lookup_corpus(ids, corpus, k, ng, cap)
    assert got == want, (len(ids), len(corpus), k, ng, cap, got, want)
    return got


# ------------------------------------------------------------------------------------------ the two kernels alone
@pytest.mark.parametrize("case, want", KNOWN)
def test_known_answers(ctx4, case, want):
    ids, corpus, k, ng, cap = case
    assert ctx4[0].spec_lookup_corpus(ids, corpus, k, ng, max_positions=cap) == want


@pytest.mark.parametrize("C_len", [1, 2, 63, 64, 65, 1023, 1024, 1025, 4097, 65536])
def test_lookup_equals_the_rule_at_every_corpus_length(ctx4, C_len):
    """a 4-symbol alphabet, so that many windows match; separators now and then; the last entries of the corpus decide the edge cases
    (a window that ends on the last entry has no continuation)"""
    model = ctx4[0]
    rng = np.random.default_rng(C_len)
    corpus = [int(v) for v in rng.integers(3, 7, C_len)]
    for i in rng.integers(0, C_len, C_len // 9):
        corpus[int(i)] = -1
    by_source = {NONE: 0, HISTORY: 0, CORPUS: 0}
    for L in (2, 3, 9, 40):
        ids = [int(v) for v in rng.integers(3, 7, L)]
        for k, ng in ((1, 1), (2, 2), (3, 16), (3, 2)):
            by_source[_same(model, ids, corpus, k, ng)[1]] += 1
    ids = [int(v) for v in rng.integers(3, 7, 30)]
    for cap in (30, 31, 32, 33):        # the cut: the last id sits at position 29 of a context of `cap` positions
        _same(model, ids, corpus, 3, 16, cap)
    # the end of the corpus: a history that ends in the corpus's last ids matches there only if an id follows the window
    if C_len >= 2 and min(corpus[-2:]) >= 0:
        for ng in (1, 2, 16):
            _same(model, [8, 8] + corpus[-2:], corpus, 3, ng)
            _same(model, [8, 8] + corpus[-2:-1], corpus, 3, ng)
    if C_len >= 63:
        assert by_source[CORPUS] > 0 and by_source[HISTORY] > 0, by_source


def _planted(C_len, at, pattern, cont, fill=100):
    """a corpus of `fill` ids with pattern + cont written so that the pattern's last id lies on the entries `at`"""
    corpus = [fill] * C_len
    for j, e in enumerate(at):
        w = list(pattern) + [c + j for c in cont]
        s = e - len(pattern) + 1
        corpus[s:s + len(w)] = w
    return corpus[:C_len]          # (a continuation that runs over the end is cut there)


def test_block_edges_and_two_blocks(ctx4):
    model = ctx4[0]
    pat = [11, 12, 13, 14, 15]
    ids = [9] + pat
    # the winning window ends on the first / the last entry of a block's range, or spans the boundary behind it: (e, C)
    for e in (BLOCK - 1, BLOCK, BLOCK + 2, 2 * BLOCK - 1, 2 * BLOCK, 63 * BLOCK, 64 * BLOCK - 2, 4):
        for C_len in sorted({e + 2, e + 3, e + 5, 4 * BLOCK + 1, 64 * BLOCK}):
            if C_len < e + 2 or C_len > oracle.CORPUS_MAX:
                continue
            corpus = _planted(C_len, [e], pat, [40, 50, 60])
            got = _same(model, ids, corpus, 3, 16)
            assert got[1:] == (CORPUS, 5) and got[0] == [40, 50, 60][:C_len - e - 1], (e, C_len, got)
    # a window whose last id is the corpus's last entry is skipped: nothing else matches
    assert _same(model, ids, _planted(2 * BLOCK, [2 * BLOCK - 1], pat, []), 3, 16) == ([], NONE, 0)
    # two matches in different blocks: the lower index wins, whichever block finishes first
    for at in ([5 * BLOCK + 7, 2 * BLOCK + 9], [63 * BLOCK + 100, 200], [3 * BLOCK, 3 * BLOCK - 1 - len(pat) - 3]):
        corpus = _planted(64 * BLOCK, at, pat, [40, 50, 60])
        j = at.index(min(at))
        assert _same(model, ids, corpus, 3, 16) == ([40 + j, 50 + j, 60 + j], CORPUS, 5)
    # ... unless the later one matches a longer n-gram: the earlier window holds the last 3 ids only
    corpus = _planted(64 * BLOCK, [40 * BLOCK + 1], pat, [40, 50, 60])
    corpus[300:306] = [13, 14, 15, 70, 71, 72]
    assert _same(model, ids, corpus, 3, 16) == ([40, 50, 60], CORPUS, 5)
    assert _same(model, ids, corpus, 3, 3) == ([70, 71, 72], CORPUS, 3)
    # the history wins at equal n, loses to a longer n-gram of the corpus
    own = pat + [21, 22, 23] + pat
    assert _same(model, own, corpus, 3, 16) == ([21, 22, 23], HISTORY, 5)
    assert _same(model, [15, 33, 9] + pat, corpus, 3, 16) == ([40, 50, 60], CORPUS, 5)
    # a separator behind the window / inside the continuation
    cut = list(corpus)
    cut[40 * BLOCK + 3] = -1
    assert _same(model, ids, cut, 3, 16) == ([40], CORPUS, 5)
    cut[40 * BLOCK + 2] = -1
    assert _same(model, ids, cut, 3, 16) == ([70, 71, 72], CORPUS, 3)


def test_op_refusals(ctx4):
    model = ctx4[0]
    out, k, src, ng = (C.c_int32 * 4)(), C.c_int(0), C.c_int(0), C.c_int(0)
    ids = (C.c_int32 * 2)(4, 5)

    def rc(corpus, n=None, kk=3, ngram=2):
        arr = (C.c_int32 * max(1, len(corpus)))(*corpus)
        return model.lib.dtk_op_spec_lookup_corpus(model._ctx, ids, 2, arr, len(corpus) if n is None else n, kk, ngram, 16, out, C.byref(k),
                                                   C.byref(src), C.byref(ng))

    assert rc([5, 6]) == 0 and k.value == 1 and out[0] == 6
    assert rc([5, TINY.vocab]) == -1 and rc([5, 6], kk=4) == -1 and rc([5, 6], ngram=17) == -1 and rc([5, 6], n=-1) == -1
    assert rc([5] * (_lib.DTK_SPEC_CORPUS_MAX + 1)) == -4


# ------------------------------------------------------------------------------------------ generate with a corpus
def _spec(model, ids, px, cfg, corpus=None, n=N_NEW, **kw):
    return model.generate(input_ids=ids[None], pixel_values=px, bad_words_ids=[[IMG]], begin_suppress_tokens=[EOS], suppress_tokens=[EOS],
                          eos_token_id=-1, max_new_tokens=n, return_logprobs=True, prompt_lookup_num_tokens=K, max_matching_ngram_size=NGRAM,
                          **({"prompt_lookup_corpus": corpus} if corpus is not None else {}), **cfg, **kw)


@pytest.mark.parametrize("name, cfg", [("sampled", SAMPLED), ("greedy", GREEDY)])
def test_generate_with_the_plain_run_as_corpus(ctx4, name, cfg):
    model, proc, ids, px, truth = ctx4
    T = ids.numel()
    toks = truth[name][0]
    seq = ids.tolist() + toks
    program = list(TAIL) + toks                     # the prompt tail plus what the plain run produced
    steps = oracle.steps_corpus(seq, T, K, NGRAM, program, N_NEW, TINY.max_positions)
    without = oracle.accept_pattern_corpus(seq, T, K, NGRAM, [], N_NEW, TINY.max_positions)
    if name == "sampled":      # conditions on the inputs (seed 4711 gives them): the corpus must decide something in this run
        assert any(a == K + 1 and src == CORPUS for a, _, src in steps) and len(steps) < len(without), (steps, without)
    out = _spec(model, ids, px, cfg, [torch.tensor(program)])
    print(name, "accepted per step:", out.accepted_per_step, "sources:", out.draft_sources)
    same_as_plain(out, T, truth[name], N_NEW)
    assert out.accepted_per_step == [a for a, _, _ in steps]
    from_corpus = sum(src == CORPUS for _, _, src in steps[1:])      # (step i made the drafts step i + 1 verified)
    assert out.draft_sources[1] >= from_corpus > 0 and len(steps) <= sum(out.draft_sources) <= len(steps) + 2
    assert model.spec_corpus_len() == 0 and model.cached_ids(0) == out.sequences[0].tolist()
    # the same call without the corpus: today's pattern, the same tokens
    plain = _spec(model, ids, px, cfg)
    same_as_plain(plain, T, truth[name], N_NEW)
    assert plain.accepted_per_step == without and plain.draft_sources is None and model.spec_corpus_len() == 0
    # a corpus that drafts wrong tokens changes the steps and nothing else
    wrong = [[t, (t + 1) % 3 + 3] for t in set(toks)]
    out = _spec(model, ids, px, cfg, wrong)
    same_as_plain(out, T, truth[name], N_NEW)
    assert out.accepted_per_step == oracle.accept_pattern_corpus(seq, T, K, NGRAM, oracle.flatten(wrong), N_NEW, TINY.max_positions)
    assert out.draft_sources[1] > 0 and model.spec_corpus_len() == 0


# ------------------------------------------------------------------------------------------ the life of the corpus
def test_captures_and_a_persistent_corpus(ctx4):
    model, proc, ids, px, truth = ctx4
    T = ids.numel()
    toks = truth["sampled"][0]
    seq = ids.tolist() + toks
    program = list(TAIL) + toks
    _spec(model, ids, px, SAMPLED)                      # (the step without a corpus is captured by now)
    c0 = model.batch_graph_captures
    assert model.spec_set_corpus([program]) == len(program) == model.spec_corpus_len()
    a = _spec(model, ids, px, SAMPLED)                  # no argument: the corpus set by hand stays, and drafts
    assert model.batch_graph_captures == c0 + 1 and model.spec_corpus_len() == len(program)
    same_as_plain(a, T, truth["sampled"], N_NEW)
    assert a.accepted_per_step == oracle.accept_pattern_corpus(seq, T, K, NGRAM, program, N_NEW, TINY.max_positions)
    other = [[5, 6, 7], program[:20]]
    assert model.spec_set_corpus(other) == 24
    b = _spec(model, ids, px, SAMPLED)                  # one corpus replaced by another: nothing is captured again
    assert model.batch_graph_captures == c0 + 1
    same_as_plain(b, T, truth["sampled"], N_NEW)
    assert b.accepted_per_step == oracle.accept_pattern_corpus(seq, T, K, NGRAM, oracle.flatten(other), N_NEW, TINY.max_positions)
    assert model.spec_counters()[1] > 0
    assert model.spec_set_corpus([]) == 0 == model.spec_corpus_len()
    c = _spec(model, ids, px, SAMPLED)                  # back to none: one more capture, today's steps
    assert model.batch_graph_captures == c0 + 2
    same_as_plain(c, T, truth["sampled"], N_NEW)
    assert c.accepted_per_step == oracle.accept_pattern_corpus(seq, T, K, NGRAM, [], N_NEW, TINY.max_positions)
    # replay equals plain launches with a corpus too
    model.set_graph_mode(0)
    try:
        d = _spec(model, ids, px, SAMPLED, [program])
    finally:
        model.set_graph_mode(1)
    assert d.accepted_per_step == a.accepted_per_step and torch.equal(d.sequences, a.sequences) and _bits(d.logprobs[0]) == _bits(a.logprobs[0])


def test_refusals(ctx4):
    model, proc, ids, px, truth = ctx4
    arr = (C.c_int32 * 4)(5, 6, -1, 7)
    bad = (C.c_int32 * 2)(5, TINY.vocab)
    big = (C.c_int32 * (_lib.DTK_SPEC_CORPUS_MAX + 1))()
    assert model.lib.dtk_spec_set_corpus(model._ctx, bad, 2) == -1 and model.lib.dtk_spec_set_corpus(model._ctx, arr, -1) == -1
    assert model.lib.dtk_spec_set_corpus(model._ctx, big, _lib.DTK_SPEC_CORPUS_MAX + 1) == -4 and model.spec_corpus_len() == 0
    with pytest.raises(ValueError, match="prompt_lookup_corpus"):
        model.spec_set_corpus([[TINY.vocab]])
    model.set_sampling(**GREEDY, bad_ids=[IMG], begin_suppress_ids=[EOS], always_suppress_ids=[EOS], slot=0)
    model.prefill(ids, px, slot=0)
    model.spec_begin(2, 2)
    assert model.lib.dtk_spec_set_corpus(model._ctx, arr, 4) == 0 and model.spec_corpus_len() == 4      # speculating, nothing in flight
    model.spec_launch()
    counters = (C.c_int64 * 3)()
    assert model.lib.dtk_spec_set_corpus(model._ctx, arr, 4) == -3 and model.lib.dtk_spec_set_corpus(model._ctx, arr, 0) == -3
    assert model.lib.dtk_spec_counters(model._ctx, counters) == -3 and model.spec_corpus_len() == 4
    assert model.spec_wait() == truth["greedy"][0][:1]
    assert sum(model.spec_counters()) == 1
    model.spec_end(ids.numel() + 1)
    assert model.spec_corpus_len() == 4                  # the corpus persists over spec_end until it is cleared
    assert model.spec_set_corpus([]) == 0 and model.spec_corpus_len() == 0
    other, _ = _load(16)                                 # outside the multi-vector family: no speculative step, no corpus
    assert other.lib.dtk_spec_set_corpus(other._ctx, arr, 4) == -3 and other.spec_corpus_len() == 0
    with pytest.raises(_lib.DtkError, match="dtk_spec_set_corpus"):
        other.spec_set_corpus([[5, 6]])
    del other
    gc.collect()
