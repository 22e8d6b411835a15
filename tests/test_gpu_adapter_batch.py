"""Text-conditioned sequences (the TikZero adapter) in the batch engine's slots on the MI355X: the toy v2 model with its toy adapter
in contexts of 4, 16 and 64 decoding slots, against tests/adapter_oracle.AdapterOracle and against themselves in other company;
the search entry points end to end; and one full-size run of detikzify-v2.5-8b with a seeded adapter and 64 slots."""
from __future__ import annotations

import threading
import time

import pytest
import torch

from oracle import sampling
from oracle.model import DetikzifyOracle
from oracle.synth import tensor_specs
from tests.adapter_oracle import AdapterOracle
from tests.helpers import ENVELOPE, SLACK_LOGITS, TINY_V2, TINY_V2_CFG, rel_l2, sketch_image

pytestmark = pytest.mark.gpu

TEXT_VOCAB = 300
BAD = [TINY_V2.image_token_id]


def _load(slots, adapter=True, name="detikzify-tiny-v2", seed=4321):
    from detikzify_amd.model import load
    kw = dict(adapter=True, cross_attn_every_n_layers=2) if adapter else {}
    return load(name, synthetic=seed, batch_slots=slots, **kw)


def _text(n, seed=0, vocab=TEXT_VOCAB):
    return torch.randint(0, vocab, (n,), generator=torch.Generator().manual_seed(seed), dtype=torch.int64)


def _run(model, jobs, first=0):
    """every job (ids, pixel_values, text ids or None, generate kwargs) as its own thread through model.generate -> new tokens.
    jobs[:first] join before the others start: a sequence's join path (fork of the prefix-cache slot, donor, encode) decides the
    bits of its prompt's KV, so the company test holds that fixed and varies only who decodes next to it"""
    out, errs = [None] * len(jobs), []
    j0 = model.batch_engine.stats()["joins"]

    def worker(k):
        try:
            ids, px, t, kw = jobs[k]
            extra = {"adapter_input_ids": t[None]} if t is not None else {}
            out[k] = model.generate(input_ids=ids[None], pixel_values=px, eos_token_id=-1, bad_words_ids=[BAD], **extra, **kw)[0, ids.numel():].tolist()
        except BaseException as e:  # noqa: BLE001
            errs.append(e)
    ths = [threading.Thread(target=worker, args=(k,)) for k in range(len(jobs))]
    [t.start() for t in ths[:first]]
    deadline = time.perf_counter() + 120
    while first and model.batch_engine.stats()["joins"] < j0 + first and time.perf_counter() < deadline and not errs:
        time.sleep(0.002)
    [t.start() for t in ths[first:]]
    [t.join(timeout=300) for t in ths]
    assert not any(t.is_alive() for t in ths) and not errs, errs[:1]
    return out


def _company(proc, n, seed):
    """n other sequences: other texts on the same image, texts on other images, image-only prompts, text-only (dummy) prompts"""
    jobs = []
    for k in range(n):
        kind = k % 4
        enc = proc(images=sketch_image(1 if kind == 0 else 10 + k % 5, 84), return_tensors="pt")
        ids, px = enc.input_ids[0], enc.pixel_values
        t = _text(5 + k % 7, 100 + k % 6)
        if kind == 2:
            t = None
        if kind == 3:
            px = None
        jobs.append((ids, px, t, dict(do_sample=True, seed=seed + k, max_new_tokens=10 + k % 5)))
    return jobs


@pytest.mark.parametrize("slots", [5, 17, 65])
def test_text_sequence_in_a_slot_matches_the_oracle_alone_and_in_company(slots):
    from detikzify_amd.infer.batching import BatchEngine
    from detikzify_amd.infer.engine import NativeBatchEngine
    model, proc = _load(slots)
    cap = model.max_decode_slots()
    enc = proc(images=sketch_image(1, 84), return_tensors="pt")
    ids, px = enc.input_ids[0], enc.pixel_values
    t = _text(40, 3)
    target = (ids, px, t, dict(do_sample=False, max_new_tokens=12))
    sampled = (ids, px, t, dict(do_sample=True, temperature=0.8, top_p=0.95, top_k=0, seed=77, max_new_tokens=12))
    others = _company(proc, cap - 2, 900)
    results = {}
    for make in (NativeBatchEngine, BatchEngine):
        runs = []
        for jobs, first in (([target], 0), ([sampled], 0), ([target, sampled] + others, 2)):
            eng = make(model, max_batch=cap)        # (a fresh engine: every run's target joins by the same path)
            runs.append(_run(model, jobs, first))
            eng.close()
        alone, alone_s, full = runs[0][0], runs[1][0], runs[2]
        assert full[0] == alone and full[1] == alone_s, make.__name__        # company independence, bit for bit
        results[make.__name__] = (alone, alone_s)
    assert results["NativeBatchEngine"] == results["BatchEngine"]
    toks, toks_s = results["NativeBatchEngine"]
    assert len(toks) == 12 and len(toks_s) == 12
    # greedy against the CPU oracle (criteria of test_gpu_adapter.test_text_conditioned_prefill_and_greedy_decode)
    w = {n: model.read_tensor(n).float().reshape(s) for n, s, _, _ in tensor_specs(TINY_V2_CFG)}
    for n in model.tensor_names():
        if n.startswith(("adapter.", "embedding_model.")):
            w[n] = model.read_tensor(n).float()
    acfg = model.adapter_config.oracle_dict()
    feats = AdapterOracle(TINY_V2_CFG, acfg, w, "bf16").features(px[0], t)
    feats32 = AdapterOracle(TINY_V2_CFG, acfg, w, "fp32").features(px[0], t)
    main = {n: v for n, v in w.items() if not n.startswith(("adapter.", "embedding_model."))}
    oracle = DetikzifyOracle(TINY_V2_CFG, main, precision="bf16")
    logits = oracle.prefill(ids, px[0], vit_feats=feats)
    truth = DetikzifyOracle(TINY_V2_CFG, main, precision="fp32").prefill(ids, px[0], vit_feats=feats32)
    model.set_sampling(do_sample=False, bad_ids=BAD, slot=0)
    dev = model.prefill(ids, px, slot=0, return_logits=True, adapter_input_ids=t)
    e_dev, e_orc = rel_l2(dev, truth), rel_l2(logits, truth)
    assert e_dev < ENVELOPE * e_orc + SLACK_LOGITS, (e_dev, e_orc)
    for i, tok in enumerate(toks):
        rt = sampling.greedy(logits, BAD, [], False)
        if rt != tok:
            top2 = torch.topk(sampling.mask_scores(logits, BAD, [], False), 2)[0]
            assert float(top2[0] - top2[1]) <= 2 * float(top2[0].abs()) * 2.0 ** -7 + 1e-6, (i, tok, rt)
        logits = oracle.step(tok)
    # the 12 sampled draws: the oracle's sampler on the slot's own logits of every step (integer work: exact).  The slot gets its
    # prompt as the engine gave it — the pair's prefix-cache slot forked whole — so it reads its prefix rows the same way
    src = model.num_slots() - 1
    n_img = int((ids == TINY_V2.image_token_id).sum())
    assert n_img == ids.numel()
    model.set_sampling(do_sample=False, slot=src)
    model.prefill(ids, px, slot=src, reuse=False, adapter_input_ids=t)
    model.set_sampling(do_sample=True, temperature=0.8, top_p=0.95, seed=77, bad_ids=BAD, slot=0)
    model.kv_fork(src, 0, n_img)
    for i in range(12):
        lg = model.get_logits_slot(0)
        model.decode_batch_launch([0])
        got = model.decode_batch_wait()[0]
        rt, _ = sampling.draw(lg, 0.8, 0, 0.95, 77, i, BAD, [], False)
        assert got == rt == toks_s[i], (i, got, rt, toks_s[i])


def test_fork_tail_and_whole_fork_equal_a_full_text_prefill():
    """the pair's prefix-cache slot forked (whole: KV + logits; + tail prefill) is bit-identical to prefill_slot_text of the same
    prompt in a fresh slot; the same pixels under another text, or none, are another prefix"""
    model, proc = _load(17)
    src = 16
    enc = proc(images=sketch_image(2, 84), return_tensors="pt")
    ids, px = enc.input_ids[0], enc.pixel_values
    n_img = int((ids == TINY_V2.image_token_id).sum())
    full = torch.cat([ids, torch.tensor([40, 41, 42])])
    t = _text(20, 5)
    for s in range(4):
        model.set_sampling(do_sample=False, slot=s)
    model.set_sampling(do_sample=False, slot=src)
    head = model.prefill(ids[:n_img], px, slot=src, reuse=False, adapter_input_ids=t, return_logits=True)
    model.kv_fork(src, 0, n_img)
    assert torch.equal(model.get_logits_slot(0), head)
    model.kv_fork(src, 1, n_img)
    tail = model.prefill(full, px, slot=1, reuse=True, adapter_input_ids=t, return_logits=True)
    fresh = model.prefill(full, px, slot=2, reuse=False, adapter_input_ids=t, return_logits=True)
    assert torch.equal(tail, fresh)
    key = model.image_key(px)
    from detikzify_amd.model.modeling import text_image_key, text_key
    assert model.slot_lcp(src, ids[:n_img], text_image_key(key, text_key(t))) == n_img
    assert model.slot_lcp(src, ids[:n_img], key) == 0 and model.slot_lcp(src, ids[:n_img], text_image_key(key, text_key(_text(20, 6)))) == 0
    plain = model.prefill(full, px, slot=3, reuse=False, return_logits=True)
    assert not torch.equal(plain, fresh)
    # decode: the forked slot and the fresh one go on identically
    model.decode_batch_launch([1, 2])
    a = model.decode_batch_wait()
    assert a[1] == a[2]


def test_resume_in_place_under_a_text():
    """a tree returns to its own text-conditioned rollout: it resumes in the slot and continues bit for bit (greedy: the original
    continuation); the same prompt under another text does not resume and decodes from a fresh prefix"""
    from detikzify_amd.infer.engine import NativeBatchEngine
    model, proc = _load(5)
    enc = proc(images=sketch_image(3, 84), return_tensors="pt")
    ids, px = enc.input_ids[0], enc.pixel_values
    ta, tb = _text(30, 7), _text(30, 8)
    kw = dict(do_sample=False, max_new_tokens=10, eos_token_id=-1, bad_words_ids=[BAD])
    eng = NativeBatchEngine(model, max_batch=4)
    first = model.generate(input_ids=ids[None], pixel_values=px, sequence_owner=0, adapter_input_ids=ta[None], **kw)[0]
    back = first[: ids.numel() + 5]
    again = model.generate(input_ids=back[None], pixel_values=px, sequence_owner=0, adapter_input_ids=ta[None], max_length=first.numel(),
                           **{k: v for k, v in kw.items() if k != "max_new_tokens"})[0]
    st = eng.stats()
    other = model.generate(input_ids=back[None], pixel_values=px, sequence_owner=0, adapter_input_ids=tb[None], **kw)[0]
    st2 = eng.stats()
    eng.close()
    assert st["resumed_in_place"] == 1 and st2["resumed_in_place"] == 1
    assert torch.equal(again, first)
    fresh_eng = NativeBatchEngine(model, max_batch=4, resume_in_place=False)
    fresh = model.generate(input_ids=back[None], pixel_values=px, adapter_input_ids=ta[None], **kw)[0]
    fresh_b = model.generate(input_ids=back[None], pixel_values=px, adapter_input_ids=tb[None], **kw)[0]
    fresh_eng.close()
    assert torch.equal(fresh_b, other)
    assert fresh[back.numel()] == again[back.numel()]       # (resumed rows are the decode kernels', fresh ones the GEMMs': first token)


def test_search_entry_points_end_to_end_and_unload():
    from detikzify_amd.infer import DetikzifyPipeline, SyntheticTikzDocument
    from detikzify_amd.infer.batching import simulate_parallel, simulate_parallel_images
    model, proc = _load(17)
    pipe = DetikzifyPipeline(model, proc, metric="model", document_class=SyntheticTikzDocument, max_length=12 + 40, compile_timeout=None)
    got = list(pipe.simulate(text="a red circle", trees=4, expansions=2))
    assert len(got) == 8 and all(-1.0 <= float(s) <= 1.0 + 1e-6 for s, _ in got) and model.batch_engine is None
    assert model.last_batch_stats["engine"] == "native"
    images = [sketch_image(4, 84), None, sketch_image(5, 84)]
    res = list(simulate_parallel_images(pipe, images, 2, 2, texts=["a red circle", "a blue square", None]))
    assert len(res) == 12 and {i for i, _, _ in res} == {0, 1, 2} and all(-1.0 <= float(s) <= 1.0 + 1e-6 for _, s, _ in res)
    # after unload_cross_attn_adapter an image-only search is bit-identical to a model that never had the adapter
    model.unload_cross_attn_adapter()
    plain, pproc = _load(17, adapter=False)
    image = sketch_image(6, 84)
    out = []
    for m, p in ((model, pproc), (plain, pproc)):
        pp = DetikzifyPipeline(m, p, metric="model", document_class=SyntheticTikzDocument, max_length=12 + 40, compile_timeout=None)
        out.append(sorted((doc.code, float(s)) for s, doc in simulate_parallel(pp, image, trees=4, expansions_per_tree=2)))
    assert out[0] == out[1] and len(out[0]) == 8


def test_full_size_v2_5_8b_text_sequence_alone_and_in_a_full_batch():
    """detikzify-v2.5-8b + a seeded Llama-3.2-1B adapter, 64 decoding slots: a text-conditioned sequence is token-identical alone and
    among 63 others (other texts, images, image-only and text-only prompts); its first step's logits are prefill_slot_text's.  The
    context has 8 prefix-cache slots and the batch 5 (image, text) keys: no prefix is evicted while the target decodes, so its prefix
    rows are read from the same source alone and in company"""
    from detikzify_amd.infer.engine import NativeBatchEngine
    from detikzify_amd.model import load
    model, proc = load("detikzify-v2.5-8b", synthetic=11, adapter=True, batch_slots=72, max_positions=1024)
    assert model.max_decode_slots() == 64
    S = model.config.vit_image
    enc = proc(images=sketch_image(4, S), text="a red circle", return_tensors="pt")
    ids, px, t = enc["input_ids"][0], enc["pixel_values"], enc["adapter_input_ids"][0]
    vocab = model.adapter_config.vocab
    jobs = []
    texts = [_text(4 + k, 50 + k, vocab) for k in range(3)]
    for k in range(63):
        e = proc(images=sketch_image(20 + k % 4, S), return_tensors="pt")
        kind = k % 4          # (image 20, text 0), (image 21, text 1), image 22 alone, text 2 alone (the dummy image)
        jobs.append((e.input_ids[0], None if kind == 3 else e.pixel_values, None if kind == 2 else texts[min(kind, 2)],
                     dict(do_sample=True, seed=k, max_new_tokens=12)))
    target = (ids, px, t, dict(do_sample=False, max_new_tokens=16))
    runs = []
    for js, first in (([target], 0), ([target] + jobs, 1)):
        eng = NativeBatchEngine(model, max_batch=64)
        runs.append(_run(model, js, first))
        eng.close()
    alone, full = runs[0][0], runs[1]
    assert full[0] == alone and len(alone) == 16
    model.set_sampling(do_sample=False, bad_ids=BAD, slot=0)
    lg = model.prefill(ids, px, slot=0, return_logits=True, adapter_input_ids=t)
    assert torch.equal(model.get_logits_slot(0), lg)
    assert int(sampling.greedy(lg, BAD, [], False)) == alone[0]
