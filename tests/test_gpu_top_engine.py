"""Top-k alternatives in the batch engines on the MI355X: sequences of an engine built with top_logprobs=3 deliver, per token, the
bits the same prompts, seeds and slots give when stepped by hand (decode_batch_launch / decode_batch_wait(top=True)) on the same
context — on detikzify-tiny and detikzify-tiny-v2, in the multi-vector family (batch_slots=5) and the 16-column family (17), with
the automatic kernel and with the sliced pair forced at 128 logits per slice (5 slices at V = 640, 4 at V = 512)."""
from __future__ import annotations

import gc
import math
import threading

import numpy as np
import pytest
import torch

from tests.helpers import sketch_image

pytestmark = pytest.mark.gpu
SAMPLED = dict(do_sample=True, temperature=0.8, top_p=0.95)
K, NEW = 3, 8
bits = lambda v: np.asarray(v, np.float32).view(np.uint32).tolist()


@pytest.fixture(scope="module", params=[("detikzify-tiny", 5), ("detikzify-tiny", 17), ("detikzify-tiny-v2", 5), ("detikzify-tiny-v2", 17)],
                ids=lambda p: f"{p[0]}-{p[1]}slots")
def ctx(request):
    from detikzify_amd.model import load
    name, n = request.param
    model, proc = load(name, synthetic=1234 if name.endswith("tiny") else 4321, batch_slots=n)
    enc = proc(images=sketch_image(7, 96), return_tensors="pt")
    base, px = enc.input_ids[0], enc.pixel_values
    count = 3 if n == 5 else 5
    prompts = [torch.cat([base, torch.tensor([20 + 3 * s, 41 + s][: 1 + s % 2], dtype=torch.int64)]) for s in range(count)]
    yield model, proc, prompts, px
    del model
    gc.collect()


def sampling_of(model, s):
    """sequence s: sequence 0 greedy, the others sampled with their own seed"""
    img = model.config.image_token_id
    return dict(seed=700 + s, bad_ids=[img], **(SAMPLED if s else dict(do_sample=False)))


def by_engine(model, prompts, px, make, guidance=None, **engine_kw):
    """every prompt as one sequence of an engine built with top_logprobs=K, all decoding at once -> per sequence (slot, tokens, logprobs,
    sample_logprobs, top_ids, top_logprobs).  Full prefills (no shared prefix, no resume): the joins a hand-driven run makes"""
    eng = make(model, share_prefix=False, resume_in_place=False, top_logprobs=K, **engine_kw)
    assert model.top_logprobs_enabled == K and model.logprobs_enabled
    got, errs = {}, []
    gate = threading.Barrier(len(prompts))

    def run(s):
        try:
            toks = []

            def emit(t):
                toks.append(int(t))
                return len(toks) >= NEW
            emit.many = lambda ts: any([emit(t) for t in ts])
            with eng.sequence(prompts[s], px, sampling_of(model, s), max_new_tokens=NEW, stop_ids=(), per_token=False, logprobs=True,
                              top_logprobs=K, **({"guidance": guidance} if guidance else {})) as seq:
                gate.wait(timeout=60)
                seq.run(emit)
                got[s] = (seq.slot, toks[:NEW], seq.logprobs[:NEW], seq.sample_logprobs[:NEW], seq.top_ids[:NEW], seq.top_logprobs[:NEW],
                          getattr(seq, "uncond_slot", None))
        except BaseException as e:  # noqa: BLE001
            errs.append(e)
            gate.abort()
    try:
        ths = [threading.Thread(target=run, args=(s,)) for s in range(len(prompts))]
        [t.start() for t in ths]
        [t.join(timeout=120) for t in ths]
        assert not any(t.is_alive() for t in ths) and not errs, errs[:1]
    finally:
        eng.close()
    assert model.top_logprobs_enabled == 0 and model.batch_engine is None
    return got


def by_hand(model, prompts, px, slots, guided=None):
    """the same prompts in the same slots, stepped together by hand; guided = (cond slot, uncond slot, scale, negative pixels)"""
    model.enable_top_logprobs(K)
    step_slots = sorted(slots.values())
    for s, slot in slots.items():
        model.set_sampling(slot=slot, **sampling_of(model, s))
        model.prefill(prompts[s], px, slot=slot)
    if guided:
        c, u, scale, neg_px = guided
        model.set_sampling(slot=u)
        model.prefill(prompts[0], neg_px, slot=u)
        model.set_guidance(scale, c, u)
        step_slots = sorted(step_slots + [u])
    out = {s: ([], [], [], [], []) for s in slots}
    argmax_first = 0
    try:
        for _ in range(NEW):
            rows = {s: model.get_logits_slot(slot).numpy().copy() for s, slot in slots.items()} if not guided else {}
            model.decode_batch_launch(step_slots)
            t, lp, slp, ti, tl = model.decode_batch_wait(top=True)
            for s, slot in slots.items():
                for dst, v in zip(out[s], (t[slot], lp[slot], slp[slot], ti[slot], tl[slot])):
                    dst.append(v)
                if s in rows:       # entry 0 is the row's argmax (lowest id among equal maxima), and the entries are in order
                    z = rows[s]
                    order = np.lexsort((np.arange(z.size), -z.astype(np.float64)))[:K]
                    assert ti[slot] == order.tolist(), (s, slot)
                    argmax_first += 1
                if t[slot] in ti[slot]:       # the sampled token's entry is its logprob, bit for bit
                    assert bits(tl[slot][ti[slot].index(t[slot])]) == bits(lp[slot])
    finally:
        if guided:
            model.set_guidance(None, guided[0], None)
        model.enable_top_logprobs(0)
    assert guided or argmax_first == NEW * len(slots)
    return out


def same_records(got, hand):
    for s, (slot, toks, lps, slps, tis, tls, _) in got.items():
        ht, hlp, hslp, hti, htl = hand[s]
        assert toks == ht, (s, slot)
        assert bits(lps) == bits(hlp) and bits(slps) == bits(hslp), (s, slot)
        assert [list(r) for r in tis] == hti, (s, slot)
        assert [bits(r) for r in tls] == [bits(r) for r in htl], (s, slot)
        assert all(len(r) == K for r in tis) and len(tis) == NEW


@pytest.mark.parametrize("engine", ["native", "python"])
def test_engine_against_hand_driven_steps(ctx, engine):
    """(a), then (d): the whole comparison again with the sliced pair forced at 128 logits per slice, identical bits; then (e)"""
    from detikzify_amd.infer.batching import BatchEngine
    from detikzify_amd.infer.engine import NativeBatchEngine
    model, proc, prompts, px = ctx
    make = NativeBatchEngine if engine == "native" else BatchEngine
    kw = dict(input_ids=prompts[1][None], pixel_values=px, max_new_tokens=NEW, eos_token_id=-1, seed=31, return_logprobs=True,
              bad_words_ids=[[model.config.image_token_id]], **SAMPLED)
    before = model.generate(top_logprobs=K, **kw)
    got = by_engine(model, prompts, px, make)
    slots = {s: g[0] for s, g in got.items()}
    assert len(set(slots.values())) == len(prompts)
    hand = by_hand(model, prompts, px, slots)
    same_records(got, hand)
    assert got[0][1] == [r[0] for r in got[0][4]] or model.config.image_token_id in [r[0] for r in got[0][4]]      # the greedy sequence takes entry 0
    # (d) the sliced pair, several slices at these vocabularies
    model.set_option("top_kernel", 2)
    model.set_option("top_slice", 128)
    try:
        assert model.config.vocab in (640, 512)
        sliced = by_engine(model, prompts, px, make)
        same_records(sliced, by_hand(model, prompts, px, {s: g[0] for s, g in sliced.items()}))
        same_records(got, by_hand(model, prompts, px, slots))       # in the first run's slots: the bits the single-block kernel gave
    finally:
        model.set_option("top_kernel", 0)
        model.set_option("top_slice", 8192)
    # (e) an engine without the argument still refuses; generate() without an engine returns what it returned before
    plain = make(model, share_prefix=False)
    try:
        with pytest.raises(NotImplementedError, match="top_logprobs: not in the batch engines yet"):
            with plain.sequence(prompts[0], px, dict(do_sample=False), max_new_tokens=2, logprobs=True, top_logprobs=K):
                pass
        with pytest.raises(NotImplementedError, match="top_logprobs: not in the batch engines yet"):
            model.generate(top_logprobs=K, **kw)
    finally:
        plain.close()
    after = model.generate(top_logprobs=K, **kw)
    assert torch.equal(after.sequences, before.sequences) and torch.equal(after.top_ids, before.top_ids)
    assert bits(after.top_logprobs) == bits(before.top_logprobs) and bits(after.logprobs) == bits(before.logprobs)


def test_generate_under_the_engine_returns_j_columns(ctx):
    from detikzify_amd.infer.engine import NativeBatchEngine
    model, proc, prompts, px = ctx
    kw = dict(input_ids=prompts[1][None], pixel_values=px, max_new_tokens=NEW, eos_token_id=-1, seed=31, return_logprobs=True,
              bad_words_ids=[[model.config.image_token_id]], **SAMPLED)
    eng = NativeBatchEngine(model, share_prefix=False, resume_in_place=False, top_logprobs=K)
    try:
        full = model.generate(top_logprobs=K, **kw)
        two = model.generate(top_logprobs=2, **kw)
        with pytest.raises(ValueError, match=f"top_logprobs={K}"):
            model.generate(top_logprobs=K + 1, **kw)
    finally:
        eng.close()
    assert full.top_ids.shape == full.top_logprobs.shape == (1, NEW, K) and two.top_ids.shape == (1, NEW, 2)
    assert torch.equal(two.sequences, full.sequences) and torch.equal(two.top_ids, full.top_ids[..., :2])
    assert bits(two.top_logprobs) == bits(full.top_logprobs[..., :2])
    assert bool((full.top_logprobs[..., :-1] >= full.top_logprobs[..., 1:]).all())


@pytest.mark.parametrize("engine", ["native", "python"])
def test_guided_pair_delivers_the_leaders_records(ctx, engine):
    """(b): a guided sequence's records are its conditional slot's, of the guided distribution: those of the pair stepped by hand, and
    not those of the unguided run"""
    from detikzify_amd.infer.batching import BatchEngine
    from detikzify_amd.infer.engine import NativeBatchEngine
    model, proc, prompts, px = ctx
    make = NativeBatchEngine if engine == "native" else BatchEngine
    neg_px = proc(images=sketch_image(3, 96), return_tensors="pt").pixel_values
    scale = 2.5
    one = prompts[:1]
    guided = by_engine(model, one, px, make, guidance=dict(scale=scale, pixel_values=neg_px), guided_pairs=1)
    plain = by_engine(model, one, px, make)
    slot, toks, lps, slps, tis, tls, uslot = guided[0]
    assert uslot is not None and uslot != slot
    hand = by_hand(model, one, px, {0: slot}, guided=(slot, uslot, scale, neg_px))
    same_records(guided, hand)
    assert [bits(r) for r in tls] != [bits(r) for r in plain[0][5]], "the guided records are the unguided run's"
    assert all(math.isfinite(v) for r in tls for v in r)


def test_a_resumed_slot_has_no_record_for_its_forced_token(ctx):
    """(c), by hand (an engine drops the forced token of a slot it resumed, and its record with it)"""
    model, proc, prompts, px = ctx
    key = model.image_key(px)
    model.enable_top_logprobs(K)
    try:
        model.set_sampling(slot=1, **sampling_of(model, 1))
        model.prefill(prompts[1], px, slot=1)
        first = []
        for _ in range(4):
            model.decode_batch_launch([1])
            first.append(model.decode_batch_wait(top=True)[0][1])
        model.resume_slot(1, torch.cat([prompts[1], torch.tensor(first[:2])]), key)
        model.decode_batch_launch([1])
        t, lp, slp, ti, tl = model.decode_batch_wait(top=True)
        assert t[1] == first[1] and ti[1] == [-1] * K and all(math.isnan(v) for v in tl[1]) and math.isnan(lp[1])
        model.decode_batch_launch([1])
        t, lp, slp, ti, tl = model.decode_batch_wait(top=True)
        assert t[1] >= 0 and all(i >= 0 for i in ti[1]) and all(math.isfinite(v) for v in tl[1])
    finally:
        model.enable_top_logprobs(0)
