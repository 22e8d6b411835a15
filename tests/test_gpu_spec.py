"""Prompt-lookup speculative decoding in the multi-vector step (dtk_spec_*), on the device: the lookup kernel alone
against the plain-Python rule, and generate(prompt_lookup_num_tokens=K) against PLAIN STEPS OF SLOT 0 on the same context
(decode_batch_launch([0])) — the same tokens and bit-equal log-probabilities, greedy and sampled, with drafts from a table (which
decides acceptance exactly) and from the real lookup; graph replay, fp8 rows, the context end, a stop inside an accepted run, the
slots afterwards, and the refusals."""
from __future__ import annotations

import gc

import numpy as np
import pytest
import torch

from detikzify_amd import _lib
from oracle import sampling
from tests import spec_oracle
from tests.helpers import TINY, peaked_lm_head, sketch_image

pytestmark = pytest.mark.gpu

IMG, EOS = TINY.image_token_id, TINY.eos_token_id
N_NEW = 40
EXTRA = 4          # the plain run goes this much further: the last speculative step may accept past N_NEW
GREEDY = dict(do_sample=False)
SAMPLED = dict(do_sample=True, temperature=0.8, top_p=0.95, top_k=0, seed=4711)
MINP = dict(do_sample=True, temperature=0.8, top_p=0.95, top_k=0, seed=99, min_p=0.02)


def _load(slots, **kw):
    from detikzify_amd.model import load
    model, proc = load("detikzify-tiny", synthetic=1234, batch_slots=slots, **kw)
    model.enable_logprobs()
    return model, proc


def _prompt(proc, seed=2, tail=(77, 30, 9, 77, 30)):
    enc = proc(images=sketch_image(seed, 96), return_tensors="pt")
    return torch.cat([enc.input_ids[0], torch.tensor(list(tail), dtype=torch.int64)]), enc.pixel_values


def _bits(values):
    return np.asarray(values, dtype=np.float32).tobytes()


def plain_slot0(model, ids, px, n, cfg, want_logits=False):
    """n plain steps of slot 0 behind a prefill: (tokens, logprobs, sample_logprobs[, the logits every token was sampled from])"""
    cfg = dict(cfg)
    min_p = cfg.pop("min_p", 0.0)
    model.set_sampling(**cfg, bad_ids=[IMG], begin_suppress_ids=[EOS], always_suppress_ids=[EOS], slot=0, min_p=min_p)
    model.prefill(ids, px, slot=0)
    toks, lps, slps, rows = [], [], [], []
    for _ in range(n):
        if want_logits:
            rows.append(model.get_logits_slot(0).clone())
        model.decode_batch_launch([0])
        t, lp, slp = model.decode_batch_wait_lp()
        toks.append(t[0]); lps.append(lp[0]); slps.append(slp[0])
    return (toks, lps, slps, rows) if want_logits else (toks, lps, slps)


def spec_run(model, ids, px, n, cfg, K, table=None, ngram=2, **kw):
    out = model.generate(input_ids=ids[None], pixel_values=px, bad_words_ids=[[IMG]], begin_suppress_tokens=[EOS], suppress_tokens=[EOS],
                         eos_token_id=kw.pop("eos_token_id", -1), max_new_tokens=n, return_logprobs=True, prompt_lookup_num_tokens=K,
                         max_matching_ngram_size=ngram, prompt_lookup_drafts=table, **cfg, **kw)
    return out


def same_as_plain(out, T, truth, n=None):
    toks, lps, slps = truth[:3]
    new = out.sequences[0, T:].tolist()
    n = len(new) if n is None else n
    assert len(new) == n and new == toks[:n], (new, toks[:n])
    assert _bits(out.logprobs[0]) == _bits(lps[:n]) and _bits(out.sample_logprobs[0]) == _bits(slps[:n])


@pytest.fixture(scope="module")
def ctx4():
    """detikzify-tiny with 4 slots + what a context that never speculated gives: the plain runs of slot 0 and a pair of plain sequences"""
    model, proc = _load(4)
    assert model.max_decode_slots() == 4
    ids, px = _prompt(proc)
    truth = {}
    for name, cfg in (("greedy", GREEDY), ("sampled", SAMPLED), ("minp", MINP)):
        truth[name] = plain_slot0(model, ids, px, N_NEW + EXTRA, cfg, want_logits=(name == "sampled"))
    pair = _pair_steps(model, proc)
    yield model, proc, ids, px, truth, pair
    del model
    gc.collect()


def _pair_steps(model, proc, n=6):
    a, pa = _prompt(proc, 5, (40, 41))
    b, pb = _prompt(proc, 9, (50,))
    for slot in (0, 1):
        model.set_sampling(do_sample=True, temperature=0.9, top_p=0.9, seed=11 + slot, bad_ids=[IMG], slot=slot)
    model.prefill(a, pa, slot=0)
    model.prefill(b, pb, slot=1)
    steps = []
    for _ in range(n):
        model.decode_batch_launch([0, 1])
        t, lp, slp = model.decode_batch_wait_lp()
        steps.append((t[:2], _bits(lp[:2]), _bits(slp[:2])))
    return steps


def _table(ids, toks, corrupt=(), wrong_all=False):
    T = ids.numel()
    tab = [-1] * T + [int(t) for t in toks]
    for i in range(T, len(tab)):
        if wrong_all or (i - T) in corrupt:
            tab[i] = tab[i] + 1 if tab[i] + 1 not in (IMG, EOS) and tab[i] + 1 < TINY.vocab else tab[i] - 1
    return tab


# ------------------------------------------------------------------------------------------ the lookup kernel alone
@pytest.mark.parametrize("dense", [True, False], ids=["alphabet-6", "random-ids"])
def test_lookup_kernel_equals_the_rule(ctx4, dense):
    model = ctx4[0]
    rng = np.random.default_rng(3 if dense else 4)
    hits = 0
    for L in (0, 1, 2, 3, 64, 65, 1023, 1025, 1100):
        ids = [int(v) for v in (rng.integers(0, 6, L) if dense else rng.choice(2_000_000, L, replace=False))]
        for K in (1, 2, 3):
            for ng in (1, 2, 3, 4):
                got = model.op_spec_lookup(ids, K, ng)
                assert got == spec_oracle.lookup(ids, K, ng), (L, K, ng, got)
                hits += len(got) > 0
        for cap in (L, L + 1, L + 2, L + 3):        # the cut: the last id sits at position L - 1 of a context of `cap` positions
            if cap >= 1:
                assert model.op_spec_lookup(ids, 3, 2, max_positions=cap) == spec_oracle.lookup(ids, 3, 2, max_positions=cap), (L, cap)
    assert (hits >= 60) if dense else (hits == 0)      # dense: every (K, n) of the five long histories finds a match


def test_lookup_kernel_picks_the_longest_ngram_and_the_first_window(ctx4):
    model = ctx4[0]
    assert model.op_spec_lookup([2, 6, 6, 1, 2, 4, 1, 2], 2, 2) == [4, 1]
    assert model.op_spec_lookup([2, 6, 6, 1, 2, 4, 1, 2], 2, 1) == [6, 6]
    assert model.op_spec_lookup([7, 7, 7, 7], 3, 2) == [7, 7] and model.op_spec_lookup([9, 9, 1, 2, 1, 2], 3, 2) == [1, 2]
    # a match that only a thread beyond the first pass of the block finds, and an earlier one that must win
    far = list(range(100, 1400)) + [5, 6, 8] + list(range(2000, 2300)) + [5, 6]
    assert model.op_spec_lookup(far, 3, 2) == [8, 2000, 2001]
    assert model.op_spec_lookup([5, 6, 3] + far, 3, 2) == [3, 100, 101]


# ------------------------------------------------------------------------------------------ forced drafts
@pytest.mark.parametrize("K", [1, 2, 3])
def test_forced_drafts_greedy(ctx4, K):
    model, proc, ids, px, truth, _ = ctx4
    T = ids.numel()
    tab = _table(ids, truth["greedy"][0], corrupt=(3, 4, 11, 30))
    out = spec_run(model, ids, px, N_NEW, GREEDY, K, tab)
    same_as_plain(out, T, truth["greedy"], N_NEW)
    want = spec_oracle.accept_pattern(ids.tolist() + truth["greedy"][0], tab, T, K, N_NEW, TINY.max_positions)
    print("accepted per step:", out.accepted_per_step)
    assert out.accepted_per_step == want and max(want) == K + 1
    assert model.cached_ids(0) == out.sequences[0].tolist()


def test_all_wrong_and_all_right_tables(ctx4):
    model, proc, ids, px, truth, _ = ctx4
    T = ids.numel()
    out = spec_run(model, ids, px, N_NEW, GREEDY, 3, _table(ids, truth["greedy"][0], wrong_all=True))
    same_as_plain(out, T, truth["greedy"], N_NEW)
    assert out.accepted_per_step == [1] * N_NEW
    out = spec_run(model, ids, px, N_NEW, GREEDY, 3, _table(ids, truth["greedy"][0]))
    same_as_plain(out, T, truth["greedy"], N_NEW)
    assert out.accepted_per_step == [1] + [4] * 10
    out = spec_run(model, ids, px, N_NEW, GREEDY, 2, [-1] * T)      # an empty table: plain steps through the speculative launch
    same_as_plain(out, T, truth["greedy"], N_NEW)
    assert out.accepted_per_step == [1] * N_NEW


@pytest.mark.parametrize("name, cfg", [("sampled", SAMPLED), ("minp", MINP)])
def test_forced_drafts_sampled(ctx4, name, cfg):
    model, proc, ids, px, truth, _ = ctx4
    T = ids.numel()
    tab = _table(ids, truth[name][0], corrupt=(3, 4, 11, 30))
    out = spec_run(model, ids, px, N_NEW, cfg, 3, tab)
    same_as_plain(out, T, truth[name], N_NEW)
    assert out.accepted_per_step == spec_oracle.accept_pattern(ids.tolist() + truth[name][0], tab, T, 3, N_NEW, TINY.max_positions)
    assert any(v != 0.0 for v in out.sample_logprobs[0].tolist())
    if name == "sampled":      # every draw is the oracle's at its own index: a draft that is accepted used the draw index of its position
        new = out.sequences[0, T:].tolist()
        for i, row in enumerate(truth[name][3][:N_NEW]):
            tok, _ = sampling.draw(row, cfg["temperature"], cfg["top_k"], cfg["top_p"], cfg["seed"], i, bad=[IMG], begin=[EOS], first=(i == 0),
                                   always=[EOS])
            assert tok == new[i], (i, tok, new[i])


def test_graph_replay_equals_plain_launches(ctx4):
    model, proc, ids, px, truth, _ = ctx4
    T = ids.numel()
    tab = _table(ids, truth["sampled"][0], corrupt=(5, 6, 20))
    model.set_graph_mode(0)
    try:
        out = spec_run(model, ids, px, N_NEW, SAMPLED, 3, tab)
    finally:
        model.set_graph_mode(1)
    same_as_plain(out, T, truth["sampled"], N_NEW)
    again = spec_run(model, ids, px, N_NEW, SAMPLED, 3, tab)
    assert again.accepted_per_step == out.accepted_per_step and torch.equal(again.sequences, out.sequences)
    assert _bits(again.logprobs[0]) == _bits(out.logprobs[0])


def test_two_slots_one_draft(ctx4):
    """batch_slots=2: the 2-vector step"""
    _, proc, ids, px, _, _ = ctx4
    model, _ = _load(2)
    T = ids.numel()
    truth = plain_slot0(model, ids, px, 24, SAMPLED)
    tab = _table(ids, truth[0], corrupt=(2, 9))
    out = spec_run(model, ids, px, 20, SAMPLED, 1, tab)
    same_as_plain(out, T, truth, 20)
    assert out.accepted_per_step == spec_oracle.accept_pattern(ids.tolist() + truth[0], tab, T, 1, 20, TINY.max_positions)
    with pytest.raises(ValueError, match="batch_slots=3"):
        spec_run(model, ids, px, 4, SAMPLED, 2)
    del model
    gc.collect()


def test_fp8_weights(ctx4):
    _, proc, ids, px, _, _ = ctx4
    model, _ = _load(4, weight_format="fp8")
    T = ids.numel()
    truth = plain_slot0(model, ids, px, 24, SAMPLED)
    tab = _table(ids, truth[0], corrupt=(4, 13))
    out = spec_run(model, ids, px, 20, SAMPLED, 3, tab)
    same_as_plain(out, T, truth, 20)
    assert max(out.accepted_per_step) == 4
    del model
    gc.collect()


# ------------------------------------------------------------------------------------------ the real lookup
@pytest.mark.parametrize("head", ["peaked", "uniform"])
def test_real_lookup(ctx4, head):
    _, proc, ids, px, _, _ = ctx4
    model, _ = _load(4)
    if head == "peaked":      # a few rows dominate every step: greedy decoding runs into a cycle, which the lookup then predicts
        w = model.read_tensor("lm_head.weight").float().reshape(TINY.vocab, -1)
        model.load_tensor("lm_head.weight", peaked_lm_head(w, 2.0, 0).to(torch.bfloat16))
    T = ids.numel()
    truth = plain_slot0(model, ids, px, 64, GREEDY)
    for K, ng in ((3, 2), (2, 3), (1, 1)):
        out = spec_run(model, ids, px, 60, GREEDY, K, None, ngram=ng)
        same_as_plain(out, T, truth, 60)
        print(head, K, ng, "accepted per step:", out.accepted_per_step)
        assert sum(out.accepted_per_step) >= 60 and all(1 <= a <= K + 1 for a in out.accepted_per_step)
        if head == "peaked":
            assert max(out.accepted_per_step) > 1
    del model
    gc.collect()


# ------------------------------------------------------------------------------------------ ends
def test_context_end(ctx4):
    """a prompt that ends 2 rows before max_positions"""
    _, proc, ids, px, _, _ = ctx4
    T = ids.numel()
    model, _ = _load(4, max_positions=T + 2)
    truth = plain_slot0(model, ids, px, 2, SAMPLED)
    for K in (1, 3):
        out = spec_run(model, ids, px, 10 ** 6 - T, SAMPLED, K, _table(ids, truth[0]))
        same_as_plain(out, T, truth, 2)
        assert out.accepted_per_step == [1, 1] and model.context_len_slot(0) == T + 2
    out = spec_run(model, ids, px, 10 ** 6 - T, SAMPLED, 3, None)
    same_as_plain(out, T, truth, 2)
    del model
    gc.collect()


def test_stop_inside_an_accepted_run(ctx4):
    model, proc, ids, px, truth, _ = ctx4
    T = ids.numel()
    toks = truth["greedy"][0]
    tab = _table(ids, toks)                          # all right: steps accept positions [0], [1..4], [5..8], ...
    at = next(i for i in (6, 7, 10, 11, 14, 15) if toks[i] not in toks[:i])      # an id that first occurs inside an accepted run
    out = spec_run(model, ids, px, N_NEW, GREEDY, 3, tab, eos_token_id=toks[at])
    same_as_plain(out, T, truth["greedy"], at + 1)
    assert model.cached_ids(0) == out.sequences[0].tolist() and model.context_len_slot(0) == T + at + 1
    model.reuse_prefix = True                        # the next call on the same prompt keeps the prompt's rows and recomputes the rest
    try:
        again = spec_run(model, ids, px, N_NEW, GREEDY, 3, tab)
    finally:
        model.reuse_prefix = False
    same_as_plain(again, T, truth["greedy"], N_NEW)


def test_slots_decode_plain_sequences_after_spec_end(ctx4):
    model, proc, ids, px, truth, pair = ctx4
    out = spec_run(model, ids, px, 12, SAMPLED, 3, _table(ids, truth["sampled"][0], corrupt=(3,)))
    same_as_plain(out, ids.numel(), truth["sampled"], 12)
    assert _pair_steps(model, proc) == pair


def test_refusals_leave_slot_0_alone(ctx4):
    model, proc, ids, px, truth, _ = ctx4
    model.set_sampling(**GREEDY, bad_ids=[IMG], begin_suppress_ids=[EOS], always_suppress_ids=[EOS], slot=0)
    model.prefill(ids, px, slot=0)
    row, held = model.get_logits_slot(0).clone(), model.cached_ids(0)

    def refused(code, *args, undo=None):
        rc = model.lib.dtk_spec_begin(model._ctx, *args)
        if undo:
            undo()
        assert rc == code, (args, rc)
        assert torch.equal(model.get_logits_slot(0), row) and model.cached_ids(0) == held

    for args in ((0, 2, 0), (4, 2, 0), (2, 0, 0), (2, _lib.DTK_SPEC_MAX_NGRAM + 1, 0), (2, 2, 2)):
        refused(-1, *args)
    model.set_penalties(0.5, 0.0, 0, slot=0)
    refused(-3, 2, 2, 0, undo=lambda: model.set_penalties(0.0, 0.0, 0, slot=0))
    model.set_dry(0.8, slot=0)
    refused(-3, 2, 2, 0, undo=lambda: model.set_dry(0.0, slot=0))
    model.set_length_control(min_new_tokens=3, eos_ids=[EOS], slot=0)
    refused(-3, 2, 2, 0, undo=lambda: model.set_length_control(slot=0))
    model.set_logit_bias({5: 1.0}, slot=0)
    refused(-3, 2, 2, 0, undo=lambda: model.set_logit_bias(None, slot=0))
    model.set_sampling(slot=1)
    model.prefill(ids, px, slot=1)
    model.set_guidance(2.0, 0, 1)
    refused(-3, 2, 2, 0, undo=lambda: model.set_guidance(None, 0, None))
    model.enable_top_logprobs(2)
    refused(-3, 2, 2, 0, undo=lambda: model.enable_top_logprobs(0))
    model.decode_batch_launch([1])                   # a step in flight
    refused(-3, 2, 2, 0, undo=model.decode_batch_wait)
    for name in ("dtk_spec_launch", "dtk_spec_end"):          # nothing to launch or end outside a speculation
        assert getattr(model.lib, name)(model._ctx, *((1,) if name == "dtk_spec_end" else ())) == -3
    # inside one: the batched entry points are refused, and slot 0 comes back as spec_end says
    model.spec_begin(2, 2)
    with pytest.raises(_lib.DtkError):
        model.decode_batch_launch([0])
    with pytest.raises(_lib.DtkError):
        model.prefill(ids, px, slot=1)
    with pytest.raises(_lib.DtkError):
        model.spec_begin(2, 2)
    model.spec_launch()
    got = model.spec_wait()
    assert got == truth["greedy"][0][:1]
    with pytest.raises(_lib.DtkError):
        model.spec_end(len(held) + 5)
    model.spec_end(len(held))
    assert model.cached_ids(0) == held
    with pytest.raises(_lib.DtkError):               # no pending logits: a prefill comes first
        model.decode_batch_launch([0])
    for slots, kw in ((16, {}), (4, dict(kv_format="mxfp8"))):      # outside the multi-vector family; MXFP8 key/value rows
        other, _ = _load(slots, **kw)
        other.set_sampling(slot=0)
        other.prefill(ids, px, slot=0)
        assert other.lib.dtk_spec_begin(other._ctx, 2, 2, 0) == -3
        with pytest.raises(NotImplementedError, match="prompt_lookup_num_tokens"):
            spec_run(other, ids, px, 4, GREEDY, 2)
        other.decode_batch_launch([0])
        assert other.decode_batch_wait()[0] >= 0
        del other
        gc.collect()
