"""Guided sequences in the batch engine's slots, on the device: standing pairs (dtk_reserve_guidance) are invisible in the
bits and re-capture nothing; the forced step of a resumed pair; a guided sequence in the native engine is generate()'s, alone and in
company; resume in place of a pair; the fork paths; MXFP8 key/value rows.  The tiny presets, at most 16 new tokens."""
from __future__ import annotations

import ctypes as C
import gc
import threading

import numpy as np
import pytest
import torch

from detikzify_amd import _lib
from detikzify_amd.infer.batching import BatchEngine
from detikzify_amd.infer.engine import NativeBatchEngine
from tests.cfg_engine_cases import bits, pair_steps, threads
from tests.helpers import TINY, sketch_image

pytestmark = pytest.mark.gpu

IMG = TINY.image_token_id
GREEDY = dict(do_sample=False)
SAMPLED = dict(do_sample=True, temperature=0.8, top_k=20, top_p=0.9, seed=4711)
GEN = dict(bad_words_ids=[[IMG]], eos_token_id=-1)


def _load(slots, **kw):
    from detikzify_amd.model import load
    model, proc = load("detikzify-tiny", synthetic=1234, batch_slots=slots, **kw)
    model.enable_logprobs()
    return model, proc


@pytest.fixture(scope="module", params=[5, 17, 65], ids=["mv-5", "mfma-17", "mfma-65"])
def ctx(request):
    model, proc = _load(request.param)
    yield model, proc
    del model
    gc.collect()


@pytest.fixture(scope="module", params=[17, 65], ids=["slots-17", "slots-65"])
def big(request):
    model, proc = _load(request.param)
    yield model, proc
    del model
    gc.collect()


def _prompts(proc):
    a, b = proc(images=sketch_image(2, 96), return_tensors="pt"), proc(images=sketch_image(7, 96), return_tensors="pt")
    tail = torch.tensor([77, 30, 9], dtype=torch.int64)
    return torch.cat([a.input_ids[0], tail]), a.pixel_values, b.pixel_values


def _by_hand(model, c, u, ids, px, px2, cfg, g, steps, company=None, **kw):
    T = int(ids.numel())
    model.set_sampling(slot=c, bad_ids=[IMG], **cfg)
    model.set_sampling(slot=u)
    if company is not None:
        model.set_sampling(slot=company, bad_ids=[IMG], **({**cfg, "seed": 99} if cfg["do_sample"] else cfg))
        model.prefill(ids, px2, slot=company)
    model.prefill(ids, px, slot=c)
    model.prefill(ids, px2, slot=u)
    model.set_guidance(g, c, u)
    try:
        return pair_steps(model, c, u, cfg, g, steps, T, [IMG], company=company, **kw)
    finally:
        model.set_guidance(None, c, None)


# ------------------------------------------------------------------------------------------ standing pairs
def test_standing_pairs_are_invisible_in_the_bits_and_recapture_nothing(ctx):
    model, proc = ctx
    ids, px, px2 = _prompts(proc)
    assert model.batch_graph_captures == 0
    base, bbits, _ = _by_hand(model, 0, 1, ids, px, px2, SAMPLED, 2.0, 8)
    n_unreserved = model.batch_graph_captures
    assert n_unreserved >= 1
    model.reserve_guidance(4)
    try:
        moved, mbits, beside = _by_hand(model, 3, 2, ids, px, px2, SAMPLED, 2.0, 8, company=0)
        assert moved == base and mbits == bbits
        # the unguided neighbour draws what it draws alone
        model.set_sampling(slot=0, bad_ids=[IMG], **{**SAMPLED, "seed": 99})
        model.prefill(ids, px2, slot=0)
        alone = []
        for _ in range(8):
            model.decode_batch_launch([0])
            alone.append(model.decode_batch_wait()[0])
        assert alone == beside
        # within the reservation no change of the pair set re-captures a step: dissolve -> another pair -> a new scale, the same step
        # family (highest active slot 3) each time
        model.set_sampling(slot=3, bad_ids=[IMG], **GREEDY)
        model.set_sampling(slot=2)
        model.prefill(ids, px, slot=3)
        model.prefill(ids, px2, slot=2)
        model.set_guidance(2.0, 3, 2)
        pair_steps(model, 3, 2, GREEDY, 2.0, 1, int(ids.numel()), [IMG])
        n = model.batch_graph_captures
        model.set_guidance(None, 3, None)
        assert model.guidance(3) is None
        model.prefill(ids, px2, slot=3)
        model.prefill(ids, px, slot=2)
        model.set_sampling(slot=2, bad_ids=[IMG], **GREEDY)
        model.set_sampling(slot=3)
        model.set_guidance(1.5, 2, 3)
        t1, _, _ = pair_steps(model, 2, 3, GREEDY, 1.5, 2, int(ids.numel()), [IMG])
        model.set_guidance(3.0, 2, 3)
        assert model.guidance(2)["scale"] == 3.0
        pair_steps(model, 2, 3, GREEDY, 3.0, 2, int(ids.numel()) + 2, [IMG], n0=2)
        model.set_guidance(None, 2, None)
        model.decode_batch_launch([3])          # no live pair: the reserved blocks all return at once
        model.decode_batch_wait()
        assert model.batch_graph_captures == n
        # a fifth pair would not fit 4: refused sizes
        assert model.lib.dtk_reserve_guidance(model._ctx, 33) == -1 and model.lib.dtk_reserve_guidance(model._ctx, -1) == -1
    finally:
        model.reserve_guidance(0)
    # without a reservation every change re-captures, as before
    again, abits, _ = _by_hand(model, 0, 1, ids, px, px2, SAMPLED, 2.0, 8)
    assert again == base and abits == bbits
    assert model.batch_graph_captures > n


# ------------------------------------------------------------------------------------------ the forced step of a resumed pair
def test_the_forced_step_of_a_resumed_pair(ctx):
    model, proc = ctx
    ids, px, px2 = _prompts(proc)
    T = int(ids.numel())
    model.reserve_guidance(2)
    try:
        first, _, _ = _by_hand(model, 0, 1, ids, px, px2, SAMPLED, 2.0, 12)
        ids2 = torch.cat([ids, torch.tensor(first[:6], dtype=torch.int64)])
        k1, k2 = model.image_key(px), model.image_key(px2)
        # the mixed launch is refused: one slot resumed, the other prefilled
        model.set_sampling(slot=0, bad_ids=[IMG], **SAMPLED)
        model.set_sampling(slot=1)
        model.resume_slot(0, ids2, k1)
        model.prefill(ids2, px2, slot=1)
        model.set_guidance(2.0, 0, 1)
        steps = model.stats()["decode_steps"]
        active = (C.c_int32 * _lib.DTK_MAX_BATCH)(1, 1)
        assert model.lib.dtk_decode_batch_launch(model._ctx, active) == -1
        assert b"forwards its last prompt token" in model.lib.dtk_last_error(model._ctx)
        assert model.stats()["decode_steps"] == steps          # nothing launched
        # the next consistent launch works: both prefilled
        model.prefill(ids2, px, slot=0)
        want, wbits, _ = pair_steps(model, 0, 1, SAMPLED, 2.0, 6, T + 6, [IMG])
        model.set_guidance(None, 0, None)
        # both resumed: the first step forwards the forced token in both slots, every later token is the oracle's over the mixed rows
        for s, (p, k) in enumerate(((px, k1), (px2, k2))):
            model.prefill(ids, p, slot=s)
        model.set_sampling(slot=0, bad_ids=[IMG], **SAMPLED)
        model.set_sampling(slot=1)
        model.set_guidance(2.0, 0, 1)
        run, _, _ = pair_steps(model, 0, 1, SAMPLED, 2.0, 12, T, [IMG])
        assert run == first
        model.set_guidance(None, 0, None)
        model.set_sampling(slot=0, bad_ids=[IMG], **SAMPLED)
        model.set_sampling(slot=1)
        # the negative prompt ends in a token of its own: the forced step must leave each slot with ITS last prompt token (a
        # k_cfg_follow that handed the conditional slot's token over would make both report ids2[-1])
        other = int(ids2[-1]) + 1 if int(ids2[-1]) + 1 != IMG else int(ids2[-1]) + 2
        ids2u = torch.cat([ids2[:-1], torch.tensor([other], dtype=torch.int64)])
        model.resume_slot(0, ids2, k1)
        model.resume_slot(1, ids2u, k2)
        model.set_guidance(2.0, 0, 1)
        lse_before = model.guidance(0)["lse"]
        model.decode_batch_launch([0, 1])
        t, lp, slp = model.decode_batch_wait_lp()
        assert t[0] == int(ids2[-1]) and t[1] == other and all(np.isnan(v) for v in (lp[0], lp[1], slp[0], slp[1]))
        assert model.cached_ids(0)[: T + 6] == ids2.tolist() and model.cached_ids(1)[: T + 6] == ids2u.tolist()
        assert bits(model.guidance(0)["lse"]) == bits(lse_before)           # the pair's blocks did not run
        # every later token is the oracle's pick over the mix of the two rows read back before its step (the resumed rows were written
        # by the decode kernels, the prefilled ones by the GEMMs, so this run is checked against its own rows, not against `want`)
        got, gbits, _ = pair_steps(model, 0, 1, SAMPLED, 2.0, 6, T + 6, [IMG])
        assert not any(np.isnan(np.frombuffer(b, np.float32)).any() for b in gbits)
        model.set_guidance(None, 0, None)
    finally:
        model.reserve_guidance(0)


# ------------------------------------------------------------------------------------------ a guided sequence in the engine
def _generate(model, ids, px, neg, g, cfg, n=12, owner=None, **kw):
    out = model.generate(input_ids=ids[None], pixel_values=px, max_new_tokens=n, guidance_scale=g, negative_pixel_values=neg,
                         return_logprobs=True, sequence_owner=owner, **{**GEN, **cfg, **kw})
    return out.sequences[0].tolist(), bits(out.logprobs), bits(out.sample_logprobs)


def _plain(model, ids, px, cfg, n=12, owner=None):
    out = model.generate(input_ids=ids[None], pixel_values=px, max_new_tokens=n, return_logprobs=True, sequence_owner=owner, **{**GEN, **cfg})
    return out.sequences[0].tolist(), bits(out.logprobs), bits(out.sample_logprobs)


SHAPED = dict(presence_penalty=0.7, logit_bias={5: 2.5, 77: -3.0})


@pytest.fixture(scope="module")
def solo(big):
    """generate() without an engine, once per context: the guided runs at three scales (greedy, sampled, shaped)"""
    model, proc = big
    ids, px, px2 = _prompts(proc)
    white = torch.ones_like(px)
    ref = {}
    for name, cfg, g, extra in (("greedy", GREEDY, 2.0, {}), ("sampled", SAMPLED, 1.5, {}), ("shaped", SAMPLED, 3.0, SHAPED)):
        ref[name] = _generate(model, ids, px, white, g, cfg, **extra)
    return ref


CASES = (("greedy", GREEDY, 2.0, {}), ("sampled", SAMPLED, 1.5, {}), ("shaped", SAMPLED, 3.0, SHAPED))


@pytest.mark.parametrize("make", [NativeBatchEngine, BatchEngine], ids=["native", "python"])
def test_a_guided_sequence_in_the_engine_is_generates(big, solo, make):
    model, proc = big
    ids, px, px2 = _prompts(proc)
    white = torch.ones_like(px)
    # full-prefill joins, as generate()'s own: a forked prefix is attended to by the grouped prefix kernel, whose fp32 summation order is
    # another one (tests/test_gpu_parity.py: same tokens, logits within 1e-2) — the fork paths have their test below
    eng = make(model, guided_pairs=3, share_prefix=False, resume_in_place=False)
    try:
        for name, cfg, g, extra in CASES:          # alone
            assert _generate(model, ids, px, white, g, cfg, **extra) == solo[name], name
        # the unguided neighbour's own solo run: alone in the engine's slots (without an engine generate() decodes with the
        # single-sequence kernels, another family with other last bits).  Every run has an owner of its own, so none resumes in the
        # slot another one left (resumed rows were written by the decode kernels, prefilled ones by the GEMMs)
        plain = _plain(model, ids, px2, SAMPLED, owner=100)
        got = {}

        def worker(k):                              # and all at once, with unguided neighbours
            if k < 3:
                name, cfg, g, extra = CASES[k]
                got[name] = _generate(model, ids, px, white, g, cfg, **extra)
            else:
                got[("plain", k)] = _plain(model, ids, px2, SAMPLED, owner=100 + k)
        eng.expect(5, 5.0)
        threads(5, worker)
        for name, *_ in CASES:
            assert got[name] == solo[name], name
        assert got[("plain", 3)] == plain and got[("plain", 4)] == plain
        assert not eng.busy()
    finally:
        eng.close()
    assert all(model.guidance(s) is None for s in range(model.max_decode_slots()))


@pytest.mark.parametrize("make", [NativeBatchEngine, BatchEngine], ids=["native", "python"])
def test_a_pair_resumes_in_place_in_the_engine(make):
    """a guided sequence of 12 tokens, then — same owner — its prompt + its first 6 tokens: the pair resumes in place, and what it
    decodes is what a pair resumed by hand decodes, whose every token pair_steps checks against the oracle over dtk_op_cfg_mix of the
    rows read back.  Both sides on the per-slot attention: the engine's first join forks its prefixes, the by-hand one prefills
    (the same rows, attended to by another kernel with prefix_mfma on)"""
    model, proc = _load(17)
    try:
        ids, px, _ = _prompts(proc)
        T = int(ids.numel())
        white = torch.ones_like(px)
        model.set_option("prefix_mfma", 0)
        cfg2 = {**SAMPLED, "seed": 5}
        first, _, _ = _by_hand(model, 0, 1, ids, px, white, SAMPLED, 2.0, 12)
        ids2 = torch.cat([ids, torch.tensor(first[:6], dtype=torch.int64)])
        model.set_sampling(slot=0, bad_ids=[IMG], **cfg2)
        model.set_sampling(slot=1)
        model.resume_slot(0, ids2, model.image_key(px))
        model.resume_slot(1, ids2, model.image_key(white))
        model.set_guidance(2.0, 0, 1)
        model.decode_batch_launch([0, 1])
        assert model.decode_batch_wait()[0] == int(ids2[-1])
        hand, hbits, _ = pair_steps(model, 0, 1, cfg2, 2.0, 8, T + 6, [IMG])
        model.set_guidance(None, 0, None)
        eng = make(model, guided_pairs=2)
        try:
            run1 = _generate(model, ids, px, white, 2.0, SAMPLED, n=12, owner=1)[0]
            assert run1[T:] == first
            toks, lp, slp = _generate(model, ids2, px, white, 2.0, cfg2, n=8, owner=1)
            st = eng.stats()
            assert st["resumed_in_place"] == 1 and (make is BatchEngine or eng.native_stats()["resumed"] == 1)
            assert toks[: T + 6] == ids2.tolist() and toks[T + 6:] == hand          # the forced token dropped once, then the oracle's picks
            assert not np.isnan(np.frombuffer(lp, np.float32)).any() and not np.isnan(np.frombuffer(slp, np.float32)).any()
        finally:
            eng.close()
    finally:
        del model
        gc.collect()


def test_guided_trees_of_one_image_fork_their_prefixes(big):
    """four guided trees of one image against a white canvas: each image is encoded once and forked into the trees' slots, and the
    trees' tokens are the full-prefill join's.  Forked rows are the source's rows bit for bit; what a fork changes is which kernel
    attends to them: by default, in a 64-slot context, the grouped prefix kernel, another fp32 summation order with logits within 1e-2 and the same greedy
    tokens (tests/test_gpu_parity.py, tests/test_gpu_parity_attn.py), under which a sampled near-tie may fall the other way.  So: on
    the default path a greedy tree's tokens are the full-prefill join's; sampled trees are compared on the per-slot attention
    (prefix_mfma 0), where a slot's arithmetic is the same whatever it shares."""
    model, proc = big
    ids, px, _ = _prompts(proc)
    white = torch.ones_like(px)
    try:
        greedy_full = _generate(model, ids, px, white, 2.0, GREEDY)
        eng = NativeBatchEngine(model, guided_pairs=4)
        try:
            vit0 = model.stats()["vit_images"]
            got = [None] * 4

            def tree(k):
                got[k] = _generate(model, ids, px, white, 2.0, GREEDY, owner=k)
            threads(4, tree)
            assert model.stats()["vit_images"] - vit0 == 2          # one ViT encode per distinct image key: the sketch and the white canvas
            assert eng.stats()["prefix_encodes"] == 2
            assert [g[0] for g in got] == [greedy_full[0]] * 4      # the default path (k_attn_prefix_g groups the forks by source)
        finally:
            eng.close()
        model.set_option("prefix_mfma", 0)
        full = [_generate(model, ids, px, white, 2.0, {**SAMPLED, "seed": 10 + k}) for k in range(4)]
        eng = NativeBatchEngine(model, guided_pairs=4)
        try:
            def worker(k):
                got[k] = _generate(model, ids, px, white, 2.0, {**SAMPLED, "seed": 10 + k}, owner=10 + k)
            threads(4, worker)
            assert [g[0] for g in got] == [f[0] for f in full]          # the full-prefill join's tokens
        finally:
            eng.close()
    finally:
        model.set_option("prefix_mfma", 1 if model.max_decode_slots() >= 64 else 0)      # the context's default (64-slot contexts: on)


def test_mxfp8_rows_one_guided_engine_sequence_is_the_pair_by_hand():
    model, proc = _load(5, kv_format="mxfp8")
    ids, px, px2 = _prompts(proc)
    try:
        toks, lpb, _ = _by_hand(model, 0, 1, ids, px, px2, SAMPLED, 2.0, 10)
        eng = NativeBatchEngine(model, guided_pairs=1)
        try:
            seq, lp, slp = _generate(model, ids, px, px2, 2.0, SAMPLED, n=10)
        finally:
            eng.close()
        assert seq[ids.numel():] == toks
        assert [bits([a, b]) for a, b in zip(np.frombuffer(lp, np.float32), np.frombuffer(slp, np.float32))] == lpb
    finally:
        del model
        gc.collect()


def test_text_adapter_negative_text_only_and_the_text_only_prompt():
    """tiny-v2 with the adapter: the negative branch differs from the prompt in its text alone (same image, same ids); under the engine
    (full-prefill joins) the sequence is generate()'s.  A text-only search without negative_text raises before any thread starts"""
    from detikzify_amd.infer import DetikzifyPipeline, SyntheticTikzDocument
    from detikzify_amd.infer.batching import simulate_parallel
    from detikzify_amd.model import load
    model, proc = load("detikzify-tiny-v2", synthetic=4321, batch_slots=17, adapter=True, cross_attn_every_n_layers=2)
    model.enable_logprobs()
    try:
        enc = proc(images=sketch_image(3, 84), return_tensors="pt")
        ids, px = enc.input_ids[0], enc.pixel_values
        gen_ = torch.Generator().manual_seed(3)
        text, neg = (torch.randint(0, 300, (n,), generator=gen_, dtype=torch.int64) for n in (7, 5))
        kw = dict(input_ids=ids[None], pixel_values=px, adapter_input_ids=text[None], negative_adapter_input_ids=neg[None], guidance_scale=2.0,
                  max_new_tokens=10, return_logprobs=True, eos_token_id=-1, bad_words_ids=[[model.config.image_token_id]], **SAMPLED)
        solo = model.generate(**kw)
        eng = NativeBatchEngine(model, guided_pairs=1, share_prefix=False, resume_in_place=False)
        try:
            got = model.generate(**kw)
        finally:
            eng.close()
        assert torch.equal(got.sequences, solo.sequences)
        assert bits(got.logprobs) == bits(solo.logprobs) and bits(got.sample_logprobs) == bits(solo.sample_logprobs)
        pipe = DetikzifyPipeline(model, proc, metric="model", document_class=SyntheticTikzDocument, max_length=12 + 40, compile_timeout=None)
        n_threads = threading.active_count()
        with pytest.raises(ValueError, match="needs negative_text"):
            list(simulate_parallel(pipe, None, trees=2, expansions_per_tree=1, text="a circle", guidance_scale=2.0))
        assert threading.active_count() == n_threads and model.batch_engine is None
    finally:
        del model
        gc.collect()


def test_guided_search_leaves_no_pair_and_no_held_slot():
    from detikzify_amd.infer import DetikzifyPipeline, SyntheticTikzDocument
    from detikzify_amd.infer.batching import simulate_parallel
    model, proc = _load(17)
    try:
        pipe = DetikzifyPipeline(model, proc, metric="model", document_class=SyntheticTikzDocument, max_length=12 + 40, compile_timeout=None)
        res = list(simulate_parallel(pipe, sketch_image(6, 84), trees=3, expansions_per_tree=1, guidance_scale=1.5))
        assert len(res) == 3
        assert model.batch_engine is None and all(model.guidance(s) is None for s in range(model.max_decode_slots()))
        assert model.last_batch_stats["joins"] >= 3
        model.set_option("logprobs", 1)          # refused while an engine holds a sequence: none does
    finally:
        del model
        gc.collect()
